// Streaming first and second moments of feature rows for the FID metric (fid30k) on gfx950.
//
// Behavioural contract: the reference keeps every activation on the host and calls np.mean / np.cov(rowvar=False)
// (metrics/frechet_inception_distance.py:43-44,64-65).  Here the activations never leave the device: each batch is folded into
//   sum[j] += sum_i d_ij      gram[j][k] += sum_i d_ij d_ik  (j <= k)      d_ij = (double)X[i][j] - shift[j]
// and igan_moments_finalize turns (sum, gram, shift, n) into (mean, cov).  The shift (a column mean of the first rows) keeps
// sum^2 / n tiny against gram, so the one-pass formula does not cancel.
// MI355X design:
//   tile       a workgroup (4 wavefronts) owns one 64 x 64 tile of gram on or above the diagonal; a wavefront owns 32 x 32 of
//              it as 2 x 2 accumulators of v_mfma_f64_16x16x4_f64.  gram = D^T D, so both operands of a k-step (4 rows) are
//              row pieces of D: lane l holds A = d[row l>>4][j0 + (l&15)] and B = d[row l>>4][k0 + (l&15)].
//   staging    32 rows x 64 columns per operand, converted and shifted ONCE on the way into LDS (fp64, row stride 80 so that
//              the four rows of a fragment read fall on different banks); rows past n and columns past F are stored as 0.0
//              -- the SHIFTED value is padded.  The next 32 rows are loaded into registers while the MFMAs of this block run.
//   sum        the workgroup of a diagonal tile adds its 64 columns down the staged rows, one thread per column, in row order.
//   ownership  the workgroup walks the n rows in order and does the read-modify-write of its tile itself: no split over n, no
//              floating-point atomic; the bits are a function of (n, F) and the sequence of calls.
// A non-finite X[i][j] reaches d_ij only: row / column j of gram and sum[j], nothing else (0 * NaN products exist only in
// padded cells, which are never stored).
#include "igan_common.h"

namespace {

typedef double mom_d4 __attribute__((ext_vector_type(4)));

constexpr int MOM_MAX_F = 4096;
constexpr int MOM_TILE = 64;      // output tile side of a workgroup
constexpr int MOM_ROWS = 32;      // rows staged per block: 8 k-steps of 4
constexpr int MOM_LD = 80;        // LDS row stride in doubles: 640 B = 2.5 bank rows
constexpr int MOM_NT = 256;
constexpr int MOM_PER_THREAD = MOM_ROWS * MOM_TILE / MOM_NT;   // 8 staged values per operand per thread

// rows r0 + 4 i + (t >> 6), column c of X into v[i]; anything outside [0, n) x [0, F) is marked by ok = false at use
__device__ inline void mom_load(const float* __restrict__ X, float (&v)[MOM_PER_THREAD], int r0, int rsub, int col, int n, int F) {
#pragma unroll
    for (int i = 0; i < MOM_PER_THREAD; i++) {
        const int r = r0 + 4 * i + rsub;
        v[i] = (r < n && col < F) ? X[(size_t)r * F + col] : 0.0f;
    }
}

__device__ inline void mom_store(double* __restrict__ lds, const float (&v)[MOM_PER_THREAD], int r0, int rsub, int c, int col, int n,
                                 int F, double shift) {
#pragma unroll
    for (int i = 0; i < MOM_PER_THREAD; i++) {
        const int rl = 4 * i + rsub;
        const bool ok = (r0 + rl < n) && (col < F);
        lds[rl * MOM_LD + c] = ok ? (double)v[i] - shift : 0.0;
    }
}

__global__ __launch_bounds__(MOM_NT) void moments_update_kernel(const float* __restrict__ X, const double* __restrict__ shift,
                                                                double* __restrict__ sum, double* __restrict__ gram, int n, int F) {
    const int tk = blockIdx.x, tj = blockIdx.y;
    if (tj > tk) return;                                   // tiles on or above the diagonal only (uniform per workgroup)
    __shared__ double lds[2 * MOM_ROWS * MOM_LD];
    const bool diag = (tj == tk);
    double* As = lds;
    double* Bs = diag ? lds : lds + MOM_ROWS * MOM_LD;
    const int t = threadIdx.x;
    const int c = t & 63, rsub = t >> 6;
    const int colA = tj * MOM_TILE + c, colB = tk * MOM_TILE + c;
    const double shA = (shift && colA < F) ? shift[colA] : 0.0;
    const double shB = (shift && colB < F) ? shift[colB] : 0.0;
    const int wave = t >> 6, lane = t & 63;
    const int wj = (wave >> 1) * 32, wk = (wave & 1) * 32;  // the wavefront's 32 x 32 corner inside the tile
    const int fr = lane & 15, fq = lane >> 4;

    mom_d4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++) acc[a][b] = mom_d4{0.0, 0.0, 0.0, 0.0};
    double colsum = 0.0;

    float va[MOM_PER_THREAD], vb[MOM_PER_THREAD];
    mom_load(X, va, 0, rsub, colA, n, F);
    if (!diag) mom_load(X, vb, 0, rsub, colB, n, F);
    for (int r0 = 0; r0 < n; r0 += MOM_ROWS) {
        __syncthreads();                                   // the previous block's fragment reads are done
        mom_store(As, va, r0, rsub, c, colA, n, F, shA);
        if (!diag) mom_store(Bs, vb, r0, rsub, c, colB, n, F, shB);
        __syncthreads();
        if (r0 + MOM_ROWS < n) {                           // next block's loads fly under this block's MFMAs
            mom_load(X, va, r0 + MOM_ROWS, rsub, colA, n, F);
            if (!diag) mom_load(X, vb, r0 + MOM_ROWS, rsub, colB, n, F);
        }
        if (diag && wave == 0) {
#pragma unroll
            for (int r = 0; r < MOM_ROWS; r++) colsum += As[r * MOM_LD + lane];      // padded rows add an exact 0
        }
#pragma unroll
        for (int ks = 0; ks < MOM_ROWS / 4; ks++) {
            const double* ar = As + (ks * 4 + fq) * MOM_LD + wj + fr;
            const double* br = Bs + (ks * 4 + fq) * MOM_LD + wk + fr;
            const double a0 = ar[0], a1 = ar[16], b0 = br[0], b1 = br[16];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
    // C/D map of the f64 instruction: col = lane & 15, row = (lane >> 4) + 4 * reg
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                const int j = tj * MOM_TILE + wj + a * 16 + fq + 4 * reg;
                const int k = tk * MOM_TILE + wk + b * 16 + fr;
                if (j <= k && k < F) gram[(size_t)j * F + k] += acc[a][b][reg];
            }
    if (diag && wave == 0 && colA < F) sum[colA] += colsum;
}

// mean and the full symmetric covariance; thread (r, c) evaluates the (min, max) entry, so cov[r][c] and cov[c][r] get the same bits
__global__ __launch_bounds__(256) void moments_finalize_kernel(const double* __restrict__ sum, const double* __restrict__ gram,
                                                               const double* __restrict__ shift, double* __restrict__ mean,
                                                               double* __restrict__ cov, double n_total, int F) {
    const int c = blockIdx.x * 64 + (threadIdx.x & 63);
    const int r = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (r >= F || c >= F) return;
    const int j = r < c ? r : c, k = r < c ? c : r;
    const double corr = sum[j] * sum[k] / n_total;
    cov[(size_t)r * F + c] = (gram[(size_t)j * F + k] - corr) / (n_total - 1.0);
    if (r == 0) mean[c] = (shift ? shift[c] : 0.0) + sum[c] / n_total;
}

// State B (n_b rows about shift_b) folded into state A, re-expressed about A's shift: with e_ij = x_ij - shift_b[j] and
// dl_j = shift_b[j] - shift_a[j], x_ij - shift_a[j] = e_ij + dl_j, hence
//   sum_i (e_ij + dl_j)               = sumB_j + n_b dl_j
//   sum_i (e_ij + dl_j) (e_ik + dl_k) = gramB_jk + dl_j sumB_k + sumB_j dl_k + n_b dl_j dl_k.
// Same tiling as moments_update_kernel; thread t owns column (t & 63) of rows (t >> 6) + 4 i of its tile and does the one
// read-modify-write of each element: no atomic, no reduction.  Every operand of element (j, k) carries index j or k, so a
// non-finite value at index m reaches row / column m only (there is no product with an operand of a third index).  Only
// j <= k of gram_b is read.
__global__ __launch_bounds__(MOM_NT) void moments_merge_kernel(double* __restrict__ sum_a, double* __restrict__ gram_a,
                                                               const double* __restrict__ shift_a, const double* __restrict__ sum_b,
                                                               const double* __restrict__ gram_b, const double* __restrict__ shift_b,
                                                               double n_b, int F) {
    const int tk = blockIdx.x, tj = blockIdx.y;
    if (tj > tk) return;                                   // tiles on or above the diagonal only (uniform per workgroup)
    const int t = threadIdx.x;
    const int c = t & 63, rsub = t >> 6;
    const int k = tk * MOM_TILE + c;
    if (k >= F) return;                                    // no barrier below: a thread past the last column has nothing to do
    const double dk = (shift_b ? shift_b[k] : 0.0) - (shift_a ? shift_a[k] : 0.0);
    const double sk = sum_b[k];
    const double right = sk + n_b * dk;                    // dl_j * right = dl_j sumB_k + n_b dl_j dl_k
#pragma unroll 4
    for (int i = 0; i < MOM_TILE / 4; i++) {
        const int j = tj * MOM_TILE + 4 * i + rsub;
        if (j > k) continue;                               // j <= k < F
        const double dj = (shift_b ? shift_b[j] : 0.0) - (shift_a ? shift_a[j] : 0.0);
        const size_t at = (size_t)j * F + k;
        gram_a[at] += gram_b[at] + (dj * right + sum_b[j] * dk);
    }
    if (tj == tk && rsub == 0) sum_a[k] += right;
}

}  // namespace

extern "C" size_t igan_moments_workspace_bytes(int n, int F) {
    (void)n; (void)F;
    return 0;         // every tile is accumulated in registers by its one owner: nothing is staged in global memory
}

extern "C" int igan_moments_update(igan_stream_t stream_, const float* X, const double* shift, double* sum, double* gram,
                                   void* workspace, size_t workspace_bytes, int n, int F) {
    using namespace igan;
    (void)workspace; (void)workspace_bytes;
    IGAN_REQUIRE(X && sum && gram, "moments_update: null buffer");
    IGAN_REQUIRE(n >= 1, "moments_update: n must be positive");
    if (F < 1 || F > MOM_MAX_F) return fail(IGAN_ERR_UNSUPPORTED, "moments_update: 1 <= F <= 4096");
    IGAN_REQUIRE((long long)n * F * 4 < 0x80000000LL, "moments_update: row matrix too large (2 GiB per call; pass it in chunks)");
    IGAN_REQUIRE((((uintptr_t)X) & 3) == 0 && (((uintptr_t)sum) & 7) == 0 && (((uintptr_t)gram) & 7) == 0 && (((uintptr_t)shift) & 7) == 0,
                 "moments_update: X must be 4-byte aligned, shift / sum / gram 8-byte aligned");
    const int tiles = ceil_div(F, MOM_TILE);
    hipLaunchKernelGGL(moments_update_kernel, dim3(tiles, tiles), dim3(MOM_NT), 0, (hipStream_t)stream_, X, shift, sum, gram, n, F);
    IGAN_LAUNCH_CHECK("moments_update launch");
    return IGAN_OK;
}

extern "C" int igan_moments_finalize(igan_stream_t stream_, const double* sum, const double* gram, const double* shift, double* mean,
                                     double* cov, long long n_total, int F) {
    using namespace igan;
    IGAN_REQUIRE(sum && gram && mean && cov, "moments_finalize: null buffer");
    IGAN_REQUIRE(n_total >= 2, "moments_finalize: n_total must be at least 2 (the covariance divides by n_total - 1)");
    if (F < 1 || F > MOM_MAX_F) return fail(IGAN_ERR_UNSUPPORTED, "moments_finalize: 1 <= F <= 4096");
    IGAN_REQUIRE(cov != gram, "moments_finalize: cov must not alias gram");
    hipLaunchKernelGGL(moments_finalize_kernel, dim3(ceil_div(F, 64), ceil_div(F, 4)), dim3(256), 0, (hipStream_t)stream_, sum, gram, shift,
                       mean, cov, (double)n_total, F);
    IGAN_LAUNCH_CHECK("moments_finalize launch");
    return IGAN_OK;
}

extern "C" int igan_moments_merge(igan_stream_t stream_, double* sum_a, double* gram_a, const double* shift_a, const double* sum_b,
                                  const double* gram_b, const double* shift_b, long long n_b, int F) {
    using namespace igan;
    if (F > MOM_MAX_F) return fail(IGAN_ERR_UNSUPPORTED, "moments_merge: 1 <= F <= 4096");
    IGAN_REQUIRE(F >= 1, "moments_merge: F must be positive (1 <= F <= 4096)");
    IGAN_REQUIRE(n_b >= 1, "moments_merge: n_b must be positive (an empty state is skipped by the caller)");
    IGAN_REQUIRE(sum_a && gram_a && sum_b && gram_b, "moments_merge: null buffer");
    IGAN_REQUIRE(sum_a != sum_b && gram_a != gram_b, "moments_merge: state B must not alias state A");
    IGAN_REQUIRE(((((uintptr_t)sum_a) | ((uintptr_t)gram_a) | ((uintptr_t)shift_a) | ((uintptr_t)sum_b) | ((uintptr_t)gram_b) | ((uintptr_t)shift_b)) & 7) == 0,
                 "moments_merge: shift / sum / gram must be 8-byte aligned");
    const int tiles = ceil_div(F, MOM_TILE);
    hipLaunchKernelGGL(moments_merge_kernel, dim3(tiles, tiles), dim3(MOM_NT), 0, (hipStream_t)stream_, sum_a, gram_a, shift_a, sum_b, gram_b,
                       shift_b, (double)n_b, F);
    IGAN_LAUNCH_CHECK("moments_merge launch");
    return IGAN_OK;
}
