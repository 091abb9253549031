// Sums of the cubic polynomial kernel over pairs of gathered feature rows, for the Kernel Inception Distance (kid50k) on gfx950.
//
// Behavioural contract: the published KID code (Binkowski et al., "Demystifying MMD GANs", ICLR 2018) draws subsets of m real and
// m fake Inception features, forms a = Kxx + Kyy and b = Kxy with k(u, v) = (u.v / F + 1)^3 on the host and reduces them with
// a.sum() - diag(a).sum() and b.sum().  Here, for every subset s, with x_i = X[idx_x[s][i]] and y_j = Y[idx_y[s][j]]:
//   out[s][0] = sum over positions i != j of k(x_i, x_j)      out[s][1] = the same over y      out[s][2] = sum over all i, j of k(x_i, y_j)
// k(u, v) = (gamma * u.v + coef0)^3.  "Diagonal" means equal POSITIONS: a subset that lists one row twice counts that pair.
// MI355X design:
//   tile       a workgroup (4 wavefronts) owns one 64 x 64 tile of one of the three pair matrices of one subset; a wavefront
//              owns 32 x 32 of it as 2 x 2 accumulators of v_mfma_f64_16x16x4_f64.  The reduction runs over F: lane l holds
//              A = a_row[l & 15][k = l >> 4] and B = b_row[l & 15][k = l >> 4] of a k-step of 4 features.  The two symmetric
//              sums have tiles on or above the diagonal only; a tile strictly above it adds its sum times 2.0 (exact).
//   staging    64 rows x 32 features per operand, GATHERED by row number and widened to fp64 once on the way into LDS (row
//              stride 34 doubles: the 16 rows x 2 k of a half-wave's fragment read fall on 32 different bank pairs); positions
//              past m and features past F are stored as 0.0.  The next 32 features are loaded into registers while the MFMAs
//              of this chunk run.  A diagonal tile stages one panel and reads it as both operands.
//   epilogue   v = fma(gamma, dot, coef0) and (v * v) * v in fp64 on the finished dot product; a cell with i >= m, j >= m or, in
//              a symmetric sum, i == j is replaced by +0.0 AFTER the cube (with coef0 = 1 a padded cell would add 1, and a
//              padded cell next to a non-finite row holds 0 * inf).
//   sum order  lane-local over the 16 cells in register order (a, b, reg), igan::wave_sum over the wavefront, the four
//              wavefronts in wave order by thread 0 through LDS, one fp64 partial per (subset, sum, tile); the second kernel
//              adds a (subset, sum)'s partials in tile order with igan::serial_sum_f64.  No atomic, no split over F: out[s] is a
//              function of subset s's indices and features alone, the same bits alone or among others, on every run.
// A non-finite feature of row r reaches the cells of row / column r of the pair matrices that list r, hence only those sums of
// those subsets.  Indices are NOT range-checked on the device: the caller of igan_poly3_kernel_sums owns that check.
#include "igan_common.h"
#include "fixed_order_sum.h"

namespace {

typedef double pks_d4 __attribute__((ext_vector_type(4)));

constexpr int PKS_MAX_F = 4096;
constexpr int PKS_TILE = 64;      // output tile side of a workgroup
constexpr int PKS_KC = 32;        // features staged per chunk: 8 k-steps of 4
constexpr int PKS_LD = 34;        // LDS row stride in doubles: row r, feature k sits on bank pair (2 r + k) mod 32
constexpr int PKS_NT = 256;
constexpr int PKS_PER_THREAD = PKS_TILE * PKS_KC / PKS_NT;   // 8 staged values per operand per thread

// tiles of one subset: the two triangles, then the square
__host__ __device__ inline long long pks_tri(int T) { return (long long)T * (T + 1) / 2; }

// feature `col` of rows row[i] (row number in M, -1 = a position past m) into v[i]; 0 outside
__device__ inline void pks_load(const float* __restrict__ M, const int (&row)[PKS_PER_THREAD], float (&v)[PKS_PER_THREAD], int col, int F) {
#pragma unroll
    for (int i = 0; i < PKS_PER_THREAD; i++) v[i] = (row[i] >= 0 && col < F) ? M[(size_t)row[i] * F + col] : 0.0f;
}

// panel rows 8 i + rsub, chunk column c: widened here, the only conversion of the kernel
__device__ inline void pks_store(double* __restrict__ lds, const float (&v)[PKS_PER_THREAD], int rsub, int c) {
#pragma unroll
    for (int i = 0; i < PKS_PER_THREAD; i++) lds[(8 * i + rsub) * PKS_LD + c] = (double)v[i];
}

// the row numbers of positions p0 + 8 i + rsub of one subset's list
__device__ inline void pks_rows(const int* __restrict__ idx, int (&row)[PKS_PER_THREAD], int p0, int rsub, int m) {
#pragma unroll
    for (int i = 0; i < PKS_PER_THREAD; i++) {
        const int p = p0 + 8 * i + rsub;
        row[i] = p < m ? idx[p] : -1;
    }
}

__global__ __launch_bounds__(PKS_NT) void poly3_tile_sums_kernel(const float* __restrict__ X, const float* __restrict__ Y,
                                                                  const int* __restrict__ idx_x, const int* __restrict__ idx_y, int m, int F,
                                                                  int T, int tiles_per_subset, double gamma, double coef0,
                                                                  double* __restrict__ partials) {
    __shared__ double lds[2 * PKS_TILE * PKS_LD];
    __shared__ double red[4];
    const int s = blockIdx.x / tiles_per_subset;
    int q = blockIdx.x - s * tiles_per_subset;
    const int ntri = (int)pks_tri(T);
    // which sum and which tile (uniform per workgroup): triangles row by row, then the square row by row
    const int which = q < ntri ? 0 : (q < 2 * ntri ? 1 : 2);
    q -= which * ntri;
    int ti, tj;
    if (which < 2) {
        ti = 0;
        for (int len = T; q >= len; len--) { q -= len; ti++; }
        tj = ti + q;
    } else {
        ti = q / T;
        tj = q - ti * T;
    }
    const bool sym = which < 2;
    const bool diag = sym && ti == tj;                      // one panel serves both operands
    const float* __restrict__ Ma = which == 1 ? Y : X;
    const float* __restrict__ Mb = which == 0 ? X : Y;
    const int* __restrict__ ia = (which == 1 ? idx_y : idx_x) + (size_t)s * m;
    const int* __restrict__ ib = (which == 0 ? idx_x : idx_y) + (size_t)s * m;

    double* As = lds;
    double* Bs = diag ? lds : lds + PKS_TILE * PKS_LD;
    const int t = threadIdx.x;
    const int c = t & 31, rsub = t >> 5;
    const int wave = t >> 6, lane = t & 63;
    const int wi = (wave >> 1) * 32, wj = (wave & 1) * 32;  // the wavefront's 32 x 32 corner inside the tile
    const int fr = lane & 15, fq = lane >> 4;

    int ra[PKS_PER_THREAD], rb[PKS_PER_THREAD];
    pks_rows(ia, ra, ti * PKS_TILE, rsub, m);
    pks_rows(ib, rb, tj * PKS_TILE, rsub, m);

    pks_d4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++) acc[a][b] = pks_d4{0.0, 0.0, 0.0, 0.0};

    float va[PKS_PER_THREAD], vb[PKS_PER_THREAD];
    pks_load(Ma, ra, va, c, F);
    if (!diag) pks_load(Mb, rb, vb, c, F);
    for (int k0 = 0; k0 < F; k0 += PKS_KC) {
        __syncthreads();                                   // the previous chunk's fragment reads are done
        pks_store(As, va, rsub, c);
        if (!diag) pks_store(Bs, vb, rsub, c);
        __syncthreads();
        if (k0 + PKS_KC < F) {                             // next chunk's loads fly under this chunk's MFMAs
            pks_load(Ma, ra, va, k0 + PKS_KC + c, F);
            if (!diag) pks_load(Mb, rb, vb, k0 + PKS_KC + c, F);
        }
#pragma unroll
        for (int ks = 0; ks < PKS_KC / 4; ks++) {
            const double* ar = As + (wi + fr) * PKS_LD + ks * 4 + fq;
            const double* br = Bs + (wj + fr) * PKS_LD + ks * 4 + fq;
            const double a0 = ar[0], a1 = ar[16 * PKS_LD], b0 = br[0], b1 = br[16 * PKS_LD];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
    // C/D map of the f64 instruction: col = lane & 15, row = (lane >> 4) + 4 * reg
    double local = 0.0;
    {
#pragma clang fp contract(off)                              // the products and the sum below are the stated ones: no fused cube-and-add
#pragma unroll
        for (int a = 0; a < 2; a++)
#pragma unroll
            for (int b = 0; b < 2; b++)
#pragma unroll
                for (int reg = 0; reg < 4; reg++) {
                    const int i = ti * PKS_TILE + wi + a * 16 + fq + 4 * reg;
                    const int j = tj * PKS_TILE + wj + b * 16 + fr;
                    const bool counted = i < m && j < m && !(sym && i == j);
                    const double v = __builtin_fma(gamma, acc[a][b][reg], coef0);
                    const double cube = (v * v) * v;
                    local += counted ? cube : 0.0;
                }
    }
    local = igan::wave_sum(local);
    if (lane == 0) red[wave] = local;
    __syncthreads();
    if (t == 0) {
        double tile;
        {
#pragma clang fp contract(off)
            tile = ((red[0] + red[1]) + red[2]) + red[3];
            if (sym && tj > ti) tile = tile * 2.0;         // the mirrored tile below the diagonal
        }
        partials[blockIdx.x] = tile;
    }
}

// out[s][which] = the partials of (s, which) added in tile order by one thread
__global__ __launch_bounds__(64) void poly3_reduce_kernel(const double* __restrict__ partials, double* __restrict__ out, int S, int T,
                                                          int tiles_per_subset) {
    const int g = blockIdx.x * 64 + threadIdx.x;
    if (g >= 3 * S) return;
    const int s = g / 3, which = g - 3 * s;
    const int ntri = (int)pks_tri(T);
    const double* p = partials + (size_t)s * tiles_per_subset + which * ntri;
    const int count = which < 2 ? ntri : T * T;
    out[g] = igan::serial_sum_f64(0.0, 0, count, [&](int j) { return p[j]; });
}

// tiles of one subset, or 0 when the sizes are outside what one launch addresses with 32-bit block and position numbers
long long pks_tiles_per_subset(int S, int m) {
    if (S < 1 || m < 2) return 0;
    if ((long long)S * m > 0x7FFFFFFFLL) return 0;         // positions of idx_x / idx_y
    const int T = igan::ceil_div(m, PKS_TILE);
    const long long per = 2 * pks_tri(T) + (long long)T * T;
    if (per * S > 0x7FFFFFFFLL) return 0;                  // blockIdx.x
    return per;
}

}  // namespace

extern "C" size_t igan_poly3_kernel_sums_workspace_bytes(int S, int m) {
    return (size_t)(pks_tiles_per_subset(S, m) * S) * sizeof(double);       // 0 tiles for sizes outside the limits
}

extern "C" int igan_poly3_kernel_sums(igan_stream_t stream_, const float* X, int nx, const float* Y, int ny, const int* idx_x,
                                      const int* idx_y, int S, int m, int F, double gamma, double coef0, double* partials, double* out) {
    using namespace igan;
    IGAN_REQUIRE(X && Y && idx_x && idx_y && partials && out, "poly3_kernel_sums: null buffer");
    IGAN_REQUIRE(nx >= 1 && ny >= 1, "poly3_kernel_sums: nx and ny must be positive");
    IGAN_REQUIRE(S >= 1, "poly3_kernel_sums: S must be positive");
    IGAN_REQUIRE(m >= 2, "poly3_kernel_sums: m must be at least 2 (the unbiased estimator divides by m - 1)");
    if (F < 1 || F > PKS_MAX_F) return fail(IGAN_ERR_UNSUPPORTED, "poly3_kernel_sums: 1 <= F <= 4096");
    const long long per = pks_tiles_per_subset(S, m);
    if (per == 0) return fail(IGAN_ERR_UNSUPPORTED, "poly3_kernel_sums: S * m and the tile count S * (2 T^2 + T), T = ceil(m / 64), must fit 31 bits");
    IGAN_REQUIRE(((((uintptr_t)X) | ((uintptr_t)Y) | ((uintptr_t)idx_x) | ((uintptr_t)idx_y)) & 3) == 0 &&
                 ((((uintptr_t)partials) | ((uintptr_t)out)) & 7) == 0,
                 "poly3_kernel_sums: X / Y / idx_x / idx_y must be 4-byte aligned, partials / out 8-byte aligned");
    const int T = ceil_div(m, PKS_TILE);
    hipLaunchKernelGGL(poly3_tile_sums_kernel, dim3((unsigned)(per * S)), dim3(PKS_NT), 0, (hipStream_t)stream_, X, Y, idx_x, idx_y, m, F, T,
                       (int)per, gamma, coef0, partials);
    IGAN_LAUNCH_CHECK("poly3_kernel_sums launch");
    hipLaunchKernelGGL(poly3_reduce_kernel, dim3(ceil_div(3 * S, 64)), dim3(64), 0, (hipStream_t)stream_, partials, out, S, T, (int)per);
    IGAN_LAUNCH_CHECK("poly3_kernel_sums reduce launch");
    return IGAN_OK;
}
