// Batched primal linear SVM passes for the linear separability metric (ls) on gfx950.
//
// Behavioural contract: the reference fits sklearn.svm.LinearSVC() per attribute and space and predicts the samples it
// fitted (metrics/linear_separability.py:162-165): squared hinge, L2, C = 1, the bias a regularised extra feature of value 1,
//     f_a(w) = 1/2 |w|^2 + C * sum_{i kept for a} max(0, 1 - y_ai * w.(x_i, 1))^2,      y_ai in {-1, +1}, 0 = pruned.
// f_a is strongly convex; its minimiser is the specification.  A Newton-CG solve of it needs, per iterate, the gradient and
// products with the generalised Hessian I + 2C X_act^T X_act -- dense products with X and nothing else -- and all A
// attributes of one space share X.
// MI355X design: ONE pass over X serves all A <= 64 problems of a gradient or a Hessian-vector product.  A workgroup (8 waves)
// owns a contiguous range of rows and walks it in slabs of 32 rows.  A slab [32 x F] is read from HBM once into LDS and used
// twice from there on the exact-fp32 MFMA (v_mfma_f32_32x32x2_f32):
//     phase 1   dec[32 x 64] = slab . V^T          (V = W or S; K = F, split over the waves by 32-column tile)
//     between   m = 1 - y dec, active mask, loss, r = y m active          (Hv: r = active z)
//     phase 2   G[F x 64]   += slab^T . r          (K = the 32 rows; wave w owns the same column tiles w, w + 8, ..)
// G stays in accumulator registers over the workgroup's rows (fp32 inside the tile), the loss and the bias column in fp64.
// Every workgroup writes its partials; a second kernel adds them in workgroup order in fp64.  No atomics: the grid is a
// function of n alone, so the same inputs give the same bits on every run.
#include "igan_common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int SVC_BM = 32;           // rows per slab
constexpr int SVC_NA = 64;           // attribute columns per launch (two 32-wide MFMA tiles)
constexpr int SVC_NW = 8;            // waves per workgroup
constexpr int SVC_NT = SVC_NW * 64;
constexpr int SVC_DP = SVC_NA + 1;   // pitch of the dec / r image
constexpr int SVC_MAX_WG = 256;      // one workgroup per CU: a slab of F = 1024 takes 128 KiB of the CU's 160 KiB LDS
constexpr int SVC_MAX_F = 1024;
constexpr int SVC_MAX_T = 8;         // step sizes per line-search call
constexpr int SVC_LS_ROWS = 4;       // rows per pass of a line-search workgroup (256 threads = 4 rows x 64 attributes)

struct SvcArgs {
    const float* X;            // [n][F]
    const signed char* Y;      // [n][A]           (gradient pass)
    const float* V;            // [A][F + 1]       W (gradient) or S (Hessian-vector)
    float* dec;                // [n][A]           out: dec (gradient) or z (Hessian-vector)
    unsigned char* act;        // [n][A]           out (gradient) / in (Hessian-vector)
    float* part;               // [G][FP][64]      per-workgroup column sums
    double* dpart;             // [G][2][64]       per-workgroup loss and bias-column sums
    int n, F, A, FP, LDX, spw; // FP = F rounded up to 32; LDX = FP + 1; spw = slabs per workgroup
};

inline int svc_slabs(int n) { return (n + SVC_BM - 1) / SVC_BM; }
inline int svc_spw(int n) { return (svc_slabs(n) + SVC_MAX_WG - 1) / SVC_MAX_WG; }
inline int svc_grid(int n) { return (svc_slabs(n) + svc_spw(n) - 1) / svc_spw(n); }
inline int svc_ls_rpw(int n) { const int per = SVC_LS_ROWS * 64; return ((n + per * SVC_MAX_WG - 1) / (per * SVC_MAX_WG)) * per; }
inline int svc_ls_grid(int n) { return (n + svc_ls_rpw(n) - 1) / svc_ls_rpw(n); }

// B fragments of phase 1 for column tile t: o[tn][j] = V[tn * 32 + l31][t * 32 + 2 j + h], zero outside [A] x [F].
__device__ __forceinline__ void svc_load_vfrag(const SvcArgs& a, int t, int l31, int h, float (&o)[2][16]) {
#pragma unroll
    for (int tn = 0; tn < 2; tn++) {
        const int at = tn * 32 + l31;
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const int f = t * 32 + 2 * j + h;
            o[tn][j] = (at < a.A && f < a.F) ? a.V[(size_t)at * (a.F + 1) + f] : 0.0f;
        }
    }
}

// TPW: column tiles per wave (ceil(F / 32 / 8)).  With TPW <= 2 a wave keeps its V fragments in registers for the whole
// range of rows; above that they would not fit beside the accumulators and are fetched again per slab (V is L2-resident).
template <int TPW, bool HV>
__global__ __launch_bounds__(SVC_NT) void svc_pass_kernel(SvcArgs a) {
    constexpr bool HOLD = TPW <= 2;
    extern __shared__ __attribute__((aligned(16))) float svc_smem[];
    float* Xs = svc_smem;                          // [32][LDX]
    float* D = svc_smem + SVC_BM * a.LDX;          // [32][SVC_DP]

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const int ntiles = a.FP >> 5;
    const int nwv = ntiles < SVC_NW ? ntiles : SVC_NW;   // waves that own a column tile
    const int ecol = tid & 63, erow = tid >> 6;          // this thread's element column in the step between the phases

    f32x16 acc[TPW][2];
#pragma unroll
    for (int i = 0; i < TPW; i++)
#pragma unroll
        for (int tn = 0; tn < 2; tn++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[i][tn][r] = 0.0f;

    float vf[HOLD ? TPW : 1][2][16];
    if constexpr (HOLD) {
#pragma unroll
        for (int i = 0; i < TPW; i++) svc_load_vfrag(a, wave + SVC_NW * i, l31, h, vf[i]);
    }
    const float vbias = (ecol < a.A) ? a.V[(size_t)ecol * (a.F + 1) + a.F] : 0.0f;
    double loss = 0.0, bsum = 0.0;

    const bool vec = ((a.F & 3) == 0) && ((((uintptr_t)a.X) & 15) == 0);
    const int slab0 = blockIdx.x * a.spw;
    const int nslabs = (a.n + SVC_BM - 1) / SVC_BM;
    for (int s = slab0; s < slab0 + a.spw && s < nslabs; s++) {
        const int row0 = s * SVC_BM;
        // ---- the slab: HBM -> LDS, once; rows past n and columns past F are zero
        if (vec) {
            const int q4 = a.FP >> 2;
            for (int e = tid; e < SVC_BM * q4; e += SVC_NT) {
                const int r = e / q4, c = (e - r * q4) * 4;
                float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (row0 + r < a.n && c < a.F) v = *reinterpret_cast<const float4*>(a.X + (size_t)(row0 + r) * a.F + c);
                float* p = Xs + r * a.LDX + c;
                p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
            }
        } else {
            for (int e = tid; e < SVC_BM * a.FP; e += SVC_NT) {
                const int r = e / a.FP, c = e - r * a.FP;
                Xs[r * a.LDX + c] = (row0 + r < a.n && c < a.F) ? a.X[(size_t)(row0 + r) * a.F + c] : 0.0f;
            }
        }
        __syncthreads();

        // ---- phase 1: this wave's share of dec = slab . V^T   (A[i = row][k = f], B[k = f][j = attribute])
        f32x16 d[2];
#pragma unroll
        for (int r = 0; r < 16; r++) { d[0][r] = 0.0f; d[1][r] = 0.0f; }
#pragma unroll
        for (int i = 0; i < TPW; i++) {
            const int t = wave + SVC_NW * i;
            if (t < ntiles) {
                float vt[2][16];
                if constexpr (!HOLD) svc_load_vfrag(a, t, l31, h, vt);
                const float* xp = Xs + l31 * a.LDX + t * 32 + h;
#pragma unroll
                for (int j = 0; j < 16; j++) {
                    const float av = xp[2 * j];
                    if constexpr (HOLD) {
                        d[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, vf[i][0][j], d[0], 0, 0, 0);
                        d[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, vf[i][1][j], d[1], 0, 0, 0);
                    } else {
                        d[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, vt[0][j], d[0], 0, 0, 0);
                        d[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, vt[1][j], d[1], 0, 0, 0);
                    }
                }
            }
        }
        // the waves' shares are added in wave order (accumulator layout: column = l31, row = (r & 3) + 8 (r >> 2) + 4 h)
        for (int w = 0; w < nwv; w++) {
            if (wave == w) {
#pragma unroll
                for (int tn = 0; tn < 2; tn++)
#pragma unroll
                    for (int r = 0; r < 16; r++) {
                        const int idx = ((r & 3) + 8 * (r >> 2) + 4 * h) * SVC_DP + tn * 32 + l31;
                        D[idx] = (w == 0) ? d[tn][r] : D[idx] + d[tn][r];
                    }
            }
            __syncthreads();
        }

        // ---- between the phases: one thread per (row, attribute); its attribute is the same in every slab
#pragma unroll
        for (int q = 0; q < SVC_BM / SVC_NW; q++) {
            const int r = erow + SVC_NW * q;
            const float v = D[r * SVC_DP + ecol] + vbias;
            float rr = 0.0f;
            if (row0 + r < a.n && ecol < a.A) {
                const size_t o = (size_t)(row0 + r) * a.A + ecol;
                a.dec[o] = v;
                if constexpr (!HV) {
                    const int y = a.Y[o];
                    const float m = 1.0f - (float)y * v;
                    const bool on = (y != 0) && (m > 0.0f);
                    a.act[o] = on ? 1 : 0;
                    if (on) {
                        rr = (float)y * m;
                        loss += (double)m * (double)m;
                    }
                } else {
                    if (a.act[o]) rr = v;
                }
                bsum += (double)rr;
            }
            D[r * SVC_DP + ecol] = rr;
        }
        __syncthreads();

        // ---- phase 2: G += slab^T . r   (A[i = f][k = row], B[k = row][j = attribute])
        float bf[2][16];
#pragma unroll
        for (int j = 0; j < 16; j++) {
            bf[0][j] = D[(2 * j + h) * SVC_DP + l31];
            bf[1][j] = D[(2 * j + h) * SVC_DP + 32 + l31];
        }
#pragma unroll
        for (int i = 0; i < TPW; i++) {
            const int t = wave + SVC_NW * i;
            if (t < ntiles) {
                const float* xp = Xs + h * a.LDX + t * 32 + l31;
#pragma unroll
                for (int j = 0; j < 16; j++) {
                    const float av = xp[2 * j * a.LDX];
                    acc[i][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bf[0][j], acc[i][0], 0, 0, 0);
                    acc[i][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bf[1][j], acc[i][1], 0, 0, 0);
                }
            }
        }
        __syncthreads();      // the next slab overwrites Xs and D
    }

    // ---- this workgroup's partials
    float* part = a.part + (size_t)blockIdx.x * a.FP * SVC_NA;
#pragma unroll
    for (int i = 0; i < TPW; i++) {
        const int t = wave + SVC_NW * i;
        if (t < ntiles) {
#pragma unroll
            for (int tn = 0; tn < 2; tn++)
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int f = t * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                    part[(size_t)f * SVC_NA + tn * 32 + l31] = acc[i][tn][r];
                }
        }
    }
    double* red = reinterpret_cast<double*>(svc_smem);       // [2][8][64] doubles = 8 KiB <= the D image alone
    red[erow * 64 + ecol] = loss;
    red[SVC_NW * 64 + erow * 64 + ecol] = bsum;
    __syncthreads();
    if (tid < 64) {
        double l = 0.0, b = 0.0;
        for (int w = 0; w < SVC_NW; w++) {
            l += red[w * 64 + tid];
            b += red[SVC_NW * 64 + w * 64 + tid];
        }
        a.dpart[(size_t)blockIdx.x * 128 + tid] = l;
        a.dpart[(size_t)blockIdx.x * 128 + 64 + tid] = b;
    }
}

// Second stage: out[a][f] = scale * sum over workgroups, in workgroup order, in fp64; f == F is the bias column.
__global__ __launch_bounds__(256) void svc_reduce_kernel(const float* __restrict__ part, const double* __restrict__ dpart,
                                                         double* __restrict__ out, double* __restrict__ loss, int G, int F,
                                                         int FP, int A, double scale) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    const int at = idx & 63, f = idx >> 6;
    if (f > F || at >= A) return;
    double s = 0.0;
    if (f < F) {
        for (int g = 0; g < G; g++) s += (double)part[((size_t)g * FP + f) * SVC_NA + at];
    } else {
        for (int g = 0; g < G; g++) s += dpart[(size_t)g * 128 + 64 + at];
    }
    out[(size_t)at * (F + 1) + f] = scale * s;
    if (f == 0 && loss != nullptr) {
        double l = 0.0;
        for (int g = 0; g < G; g++) l += dpart[(size_t)g * 128 + at];
        loss[at] = l;
    }
}

// Line search: sum over kept samples of max(0, 1 - y (dec + t z))^2 for T step sizes per attribute, from the stored fp32
// dec and z alone (dec(w + t s) = dec(w) + t z), evaluated in fp64.  256 threads = 4 rows x 64 attributes.
__global__ __launch_bounds__(256) void svc_linesearch_kernel(const float* __restrict__ dec, const float* __restrict__ z,
                                                             const signed char* __restrict__ Y, const double* __restrict__ t,
                                                             double* __restrict__ part, int n, int A, int T, int rpw) {
    __shared__ double red[SVC_LS_ROWS][SVC_MAX_T][64];
    const int at = threadIdx.x & 63, sub = threadIdx.x >> 6;
    double ts[SVC_MAX_T], acc[SVC_MAX_T];
#pragma unroll
    for (int k = 0; k < SVC_MAX_T; k++) {
        ts[k] = (k < T && at < A) ? t[(size_t)k * A + at] : 0.0;
        acc[k] = 0.0;
    }
    const int r0 = blockIdx.x * rpw;
    const int r1 = (r0 + rpw < n) ? r0 + rpw : n;
    if (at < A) {
        for (int r = r0 + sub; r < r1; r += SVC_LS_ROWS) {
            const size_t o = (size_t)r * A + at;
            const int y = Y[o];
            if (y != 0) {
                const double yd = (double)y, dv = (double)dec[o], zv = (double)z[o];
#pragma unroll
                for (int k = 0; k < SVC_MAX_T; k++) {
                    const double m = 1.0 - yd * (dv + ts[k] * zv);
                    acc[k] += (m > 0.0) ? m * m : 0.0;
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < SVC_MAX_T; k++) red[sub][k][at] = acc[k];
    __syncthreads();
    for (int e = threadIdx.x; e < SVC_MAX_T * 64; e += 256) {
        const int k = e >> 6, c = e & 63;
        double s = 0.0;
        for (int q = 0; q < SVC_LS_ROWS; q++) s += red[q][k][c];
        part[((size_t)blockIdx.x * SVC_MAX_T + k) * 64 + c] = s;
    }
}

__global__ __launch_bounds__(256) void svc_linesearch_reduce_kernel(const double* __restrict__ part, double* __restrict__ out,
                                                                    int G, int A, int T) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    const int k = e >> 6, c = e & 63;
    if (k >= T || c >= A) return;
    double s = 0.0;
    for (int g = 0; g < G; g++) s += part[((size_t)g * SVC_MAX_T + k) * 64 + c];
    out[(size_t)k * A + c] = s;
}

__global__ __launch_bounds__(256) void svc_predict_kernel(const float* __restrict__ dec, int* __restrict__ pred, int count) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < count) pred[i] = (dec[i] > 0.0f) ? 1 : 0;
}

size_t svc_pass_bytes(int n, int F) {
    const size_t G = (size_t)svc_grid(n), FP = (size_t)((F + 31) / 32 * 32);
    return G * 128 * sizeof(double) + G * FP * SVC_NA * sizeof(float);
}
size_t svc_ls_bytes(int n) { return (size_t)svc_ls_grid(n) * SVC_MAX_T * 64 * sizeof(double); }

template <int TPW, bool HV>
int svc_launch(hipStream_t stream, const SvcArgs& a, int grid, size_t lds) {
    IGAN_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&svc_pass_kernel<TPW, HV>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds), "linear_svc: LDS size");
    hipLaunchKernelGGL((svc_pass_kernel<TPW, HV>), dim3(grid), dim3(SVC_NT), lds, stream, a);
    IGAN_LAUNCH_CHECK("linear_svc pass launch");
    return IGAN_OK;
}

template <bool HV>
int svc_pass(hipStream_t stream, SvcArgs a, void* workspace, double* out, double* loss, double scale) {
    const int G = svc_grid(a.n);
    a.FP = (a.F + 31) / 32 * 32;
    a.LDX = a.FP + 1;
    a.spw = svc_spw(a.n);
    a.dpart = reinterpret_cast<double*>(workspace);
    a.part = reinterpret_cast<float*>(a.dpart + (size_t)G * 128);
    const size_t lds = (size_t)(SVC_BM * a.LDX + SVC_BM * SVC_DP) * sizeof(float);
    const int tpw = (a.FP / 32 + SVC_NW - 1) / SVC_NW;
    int rc;
    switch (tpw) {
        case 1: rc = svc_launch<1, HV>(stream, a, G, lds); break;
        case 2: rc = svc_launch<2, HV>(stream, a, G, lds); break;
        case 3: rc = svc_launch<3, HV>(stream, a, G, lds); break;
        default: rc = svc_launch<4, HV>(stream, a, G, lds); break;
    }
    if (rc) return rc;
    const int cells = (a.F + 1) * SVC_NA;
    hipLaunchKernelGGL(svc_reduce_kernel, dim3(igan::ceil_div(cells, 256)), dim3(256), 0, stream, a.part, a.dpart, out, loss, G,
                       a.F, a.FP, a.A, scale);
    IGAN_LAUNCH_CHECK("linear_svc reduce launch");
    return IGAN_OK;
}

}  // namespace

#define IGAN_SVC_REQUIRE_NA(name)                                                                                              \
    IGAN_REQUIRE(n >= 1 && A >= 1, name ": n and A must be positive");                                                         \
    if (A > SVC_NA) return ::igan::fail(IGAN_ERR_UNSUPPORTED, name ": at most 64 attributes per launch (group larger sets)");  \
    IGAN_REQUIRE((long long)n * A <= INT32_MAX, name ": n * A exceeds the int32 element count")

#define IGAN_SVC_REQUIRE_X(name)                                                                                               \
    IGAN_REQUIRE(F >= 1, name ": F must be positive");                                                                         \
    if (F > SVC_MAX_F) return ::igan::fail(IGAN_ERR_UNSUPPORTED, name ": at most 1024 features (one slab must fit the LDS)");  \
    IGAN_REQUIRE((long long)n * F * 4 <= 0x7FFFFFF0LL, name ": sample matrix too large (2 GiB per operand)")

extern "C" size_t igan_linear_svc_workspace_bytes(int n, int F, int A) {
    if (n < 1 || F < 1 || F > SVC_MAX_F || A < 1 || A > SVC_NA) return 0;
    const size_t p = svc_pass_bytes(n, F), l = svc_ls_bytes(n);
    return p > l ? p : l;
}

extern "C" int igan_linear_svc_grad(igan_stream_t stream_, const float* X, const signed char* Y, const float* W, float* dec,
                                    unsigned char* active, double* loss, double* grad, void* workspace, size_t workspace_bytes,
                                    int n, int F, int A, double C) {
    using namespace igan;
    IGAN_REQUIRE(X && Y && W && dec && active && loss && grad && workspace, "linear_svc_grad: null buffer");
    IGAN_SVC_REQUIRE_NA("linear_svc_grad");
    IGAN_SVC_REQUIRE_X("linear_svc_grad");
    IGAN_REQUIRE(C > 0.0, "linear_svc_grad: C must be positive");
    IGAN_REQUIRE(workspace_bytes >= svc_pass_bytes(n, F), "linear_svc_grad: workspace too small (igan_linear_svc_workspace_bytes)");
    SvcArgs a{};
    a.X = X; a.Y = Y; a.V = W; a.dec = dec; a.act = active; a.n = n; a.F = F; a.A = A;
    return svc_pass<false>((hipStream_t)stream_, a, workspace, grad, loss, -2.0 * C);
}

extern "C" int igan_linear_svc_hv(igan_stream_t stream_, const float* X, const unsigned char* active, const float* S, float* z,
                                  double* hv, void* workspace, size_t workspace_bytes, int n, int F, int A, double C) {
    using namespace igan;
    IGAN_REQUIRE(X && active && S && z && hv && workspace, "linear_svc_hv: null buffer");
    IGAN_SVC_REQUIRE_NA("linear_svc_hv");
    IGAN_SVC_REQUIRE_X("linear_svc_hv");
    IGAN_REQUIRE(C > 0.0, "linear_svc_hv: C must be positive");
    IGAN_REQUIRE(workspace_bytes >= svc_pass_bytes(n, F), "linear_svc_hv: workspace too small (igan_linear_svc_workspace_bytes)");
    SvcArgs a{};
    a.X = X; a.Y = nullptr; a.V = S; a.dec = z; a.act = const_cast<unsigned char*>(active); a.n = n; a.F = F; a.A = A;
    return svc_pass<true>((hipStream_t)stream_, a, workspace, hv, nullptr, 2.0 * C);
}

extern "C" int igan_linear_svc_linesearch(igan_stream_t stream_, const float* dec, const float* z, const signed char* Y,
                                          const double* t, double* out, void* workspace, size_t workspace_bytes, int n, int A,
                                          int T) {
    using namespace igan;
    IGAN_REQUIRE(dec && z && Y && t && out && workspace, "linear_svc_linesearch: null buffer");
    IGAN_SVC_REQUIRE_NA("linear_svc_linesearch");
    IGAN_REQUIRE(T >= 1 && T <= SVC_MAX_T, "linear_svc_linesearch: T must be in [1, 8]");
    IGAN_REQUIRE(workspace_bytes >= svc_ls_bytes(n), "linear_svc_linesearch: workspace too small (igan_linear_svc_workspace_bytes)");
    hipStream_t stream = (hipStream_t)stream_;
    const int G = svc_ls_grid(n);
    double* part = reinterpret_cast<double*>(workspace);
    hipLaunchKernelGGL(svc_linesearch_kernel, dim3(G), dim3(256), 0, stream, dec, z, Y, t, part, n, A, T, svc_ls_rpw(n));
    IGAN_LAUNCH_CHECK("linear_svc_linesearch launch");
    hipLaunchKernelGGL(svc_linesearch_reduce_kernel, dim3(ceil_div(SVC_MAX_T * 64, 256)), dim3(256), 0, stream, part, out, G, A, T);
    IGAN_LAUNCH_CHECK("linear_svc_linesearch reduce launch");
    return IGAN_OK;
}

extern "C" int igan_linear_svc_predict(igan_stream_t stream_, const float* dec, int* pred, int n, int A) {
    using namespace igan;
    IGAN_REQUIRE(dec && pred, "linear_svc_predict: null buffer");
    IGAN_REQUIRE(n >= 1 && A >= 1, "linear_svc_predict: n and A must be positive");
    IGAN_REQUIRE((long long)n * A <= INT32_MAX, "linear_svc_predict: n * A exceeds the int32 element count");
    hipLaunchKernelGGL(svc_predict_kernel, dim3(ceil_div(n * A, 256)), dim3(256), 0, (hipStream_t)stream_, dec, pred, n * A);
    IGAN_LAUNCH_CHECK("linear_svc_predict launch");
    return IGAN_OK;
}
