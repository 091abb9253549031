// One exact k-means step (assignment + cluster sums) for the PRD metric (prd30k) on gfx950.
//
// Behavioural contract: the reference bins the union of two embeddings with scikit-learn's MiniBatchKMeans
// (precision-recall-distributions/prd_score.py:125-127); every step of that algorithm is "nearest centre of each row, then
// the per-centre sums of the rows".  The nearest centre is the lexicographic minimum of (d2(x, c_j), j) with the ONE exact
// distance of exact_distance.h -- what an fp64 brute force on the same fp32 rows returns, ties to the lower index.
// MI355X design: the 1-NN pattern (exact_search.hip) with the centres as the candidate batch, k <= 64 so that a lane owns a centre.
//   products   [n x dim] x [dim x k] on the exact-fp32 MFMA through distance_products(): |x|^2 + |c|^2 - 2 x.c only SCREENS
//   assign     one wavefront per row: smallest upper bound, then every centre whose interval reaches below it is measured
//              as a direct difference in fp64 (wave_sqdist)
//   sums       a workgroup owns (row slice, 128 columns); a lane owns one column, walks the slice's rows in order and adds
//              into the row of its cluster in LDS (fp64); the slice partials are folded in slice order by a second kernel
//   totals     one workgroup: counts (integers) and the inertia as a fixed tree over fixed strided partial sums
// Slices, strides and trees are functions of (n, k, dim) alone and there is no floating-point atomic: two calls give the
// same bits.
#include "igan_common.h"
#include "exact_search.h"

#include <cmath>

namespace {

using namespace igan;        // exact_search.h: the screening procedure, shared with exact_search.hip

constexpr int KM_MAX_K = 64;
constexpr int KM_MAX_DIM = 4096;
constexpr int KM_COLS = 128;         // columns (= threads) of a sums workgroup: k * 128 fp64 cells <= 64 KiB of LDS
constexpr int KM_SLICE_ROWS = 64;    // smallest row slice
constexpr int KM_MAX_WG = 2048;      // sums workgroups aimed at (8 per CU)
constexpr int KM_TOT_NT = 1024;

inline int km_colblocks(int dim) { return (dim + KM_COLS - 1) / KM_COLS; }
// rows per slice: at least KM_SLICE_ROWS, and no more slices than KM_MAX_WG / column blocks
inline int km_slice_rows(int n, int dim) {
    const int max_slices = std::max(1, KM_MAX_WG / km_colblocks(dim));
    const int rows = (n + max_slices - 1) / max_slices;
    return std::max(rows, KM_SLICE_ROWS);
}
inline int km_slices(int n, int dim) { const int r = km_slice_rows(n, dim); return (n + r - 1) / r; }
inline size_t km_partial_bytes(int n, int k, int dim) { return ((size_t)km_slices(n, dim) * k * dim * sizeof(double) + 15) & ~(size_t)15; }
inline size_t km_dots_bytes(int n, int k) { return ((size_t)n * k * sizeof(float) + 15) & ~(size_t)15; }

// One wavefront per row, lane j owns centre j.  a = |x|^2 + |c|^2 - 2 x.c with the interval [a - t, a + t] of nn1_tol.
//   u = the smallest upper bound: the nearest centre's exact distance is at most u;
//   a centre whose lower bound exceeds u cannot be nearest; every other one -- a non-finite bound decides nothing -- is
//   measured exactly, in index order, and the choice is made on (exact distance, index).
// A non-finite exact distance never wins: a row with no finite distance keeps label -1 and d2 = +inf.
__global__ __launch_bounds__(256) void kmeans_assign_kernel(const float* __restrict__ dots, const float* __restrict__ xnorm,
                                                            const float* __restrict__ cnorm, const float* __restrict__ X,
                                                            const float* __restrict__ C, int* __restrict__ label,
                                                            double* __restrict__ d2, int n, int k, int dim) {
    const int row = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (row >= n) return;
    const double inf = (double)INFINITY;
    const Screen s{dots + (size_t)row * k, cnorm, (double)xnorm[row], nn1_tol(dim)};
    Interval iv{0.0, inf};
    if (lane < k) iv = s(lane);
    double u = wave_min((iv.hi < inf) ? iv.hi : inf);       // a NaN bound counts as +inf
    const float* xrow = X + (size_t)row * dim;
    double bd = inf;
    int bi = -1;
    int j;
    for (ContenderStrip strip(lane < k && contends_unless_ruled_out(iv.lo, u)); strip.next(j);) {
        if (!contends_unless_ruled_out(__shfl(iv.lo, j, 64), u)) continue;      // u has come down since the ballot
        const double e = wave_sqdist(xrow, C + (size_t)j * dim, dim, lane);
        if (e < bd) { bd = e; bi = j; }                          // ascending j: a tie keeps the lower index; false for NaN / +inf
        u = (e < u) ? e : u;
    }
    if (lane == 0) { label[row] = bi; d2[row] = bd; }
}

// Workgroup (blockIdx.x = column block, blockIdx.y = slice): thread t owns column blockIdx.x * 128 + t.
__global__ __launch_bounds__(KM_COLS) void kmeans_sums_kernel(const float* __restrict__ X, const int* __restrict__ label,
                                                              double* __restrict__ partial, int n, int k, int dim, int slice_rows) {
    extern __shared__ __attribute__((aligned(16))) double km_acc[];     // [k][KM_COLS]
    const int t = threadIdx.x;
    const int col = blockIdx.x * KM_COLS + t;
    for (int j = 0; j < k; j++) km_acc[j * KM_COLS + t] = 0.0;           // a thread touches its own column only: no barrier
    const int r0 = blockIdx.y * slice_rows;
    const int r1 = (r0 + slice_rows < n) ? r0 + slice_rows : n;
    if (col < dim) {
        const float* xp = X + col;
        int r = r0;
        for (; r + 4 <= r1; r += 4) {                                   // four loads in flight, added in row order
            const int l0 = label[r], l1 = label[r + 1], l2 = label[r + 2], l3 = label[r + 3];
            const float v0 = xp[(size_t)r * dim], v1 = xp[(size_t)(r + 1) * dim];
            const float v2 = xp[(size_t)(r + 2) * dim], v3 = xp[(size_t)(r + 3) * dim];
            if (l0 >= 0) km_acc[l0 * KM_COLS + t] += (double)v0;
            if (l1 >= 0) km_acc[l1 * KM_COLS + t] += (double)v1;
            if (l2 >= 0) km_acc[l2 * KM_COLS + t] += (double)v2;
            if (l3 >= 0) km_acc[l3 * KM_COLS + t] += (double)v3;
        }
        for (; r < r1; r++) {
            const int l = label[r];
            if (l >= 0) km_acc[l * KM_COLS + t] += (double)xp[(size_t)r * dim];
        }
        double* out = partial + (size_t)blockIdx.y * k * dim + col;
        for (int j = 0; j < k; j++) out[(size_t)j * dim] = km_acc[j * KM_COLS + t];
    }
}

// sums[cell] = partial[0][cell] + partial[1][cell] + ... in slice order
__global__ __launch_bounds__(256) void kmeans_fold_kernel(const double* __restrict__ partial, double* __restrict__ sums, int cells,
                                                          int slices) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= cells) return;
    double s = partial[c];
    for (int i = 1; i < slices; i++) s += partial[(size_t)i * cells + c];
    sums[c] = s;
}

// One workgroup: count[j] and the inertia.  Thread t adds d2 of rows t, t + 1024, ... in order; the 1024 partial sums go
// through a fixed binary tree.
__global__ __launch_bounds__(KM_TOT_NT) void kmeans_totals_kernel(const int* __restrict__ label, const double* __restrict__ d2,
                                                                  long long* __restrict__ count, double* __restrict__ inertia, int n,
                                                                  int k) {
    __shared__ double tree[KM_TOT_NT];
    __shared__ unsigned int cnt[KM_MAX_K];
    const int t = threadIdx.x;
    if (t < KM_MAX_K) cnt[t] = 0u;
    __syncthreads();
    double s = 0.0;
    for (int r = t; r < n; r += KM_TOT_NT) {
        const int l = label[r];
        if (l >= 0) {
            s += d2[r];
            atomicAdd(&cnt[l], 1u);          // integers: the order does not matter
        }
    }
    tree[t] = s;
    __syncthreads();
    for (int w = KM_TOT_NT / 2; w > 0; w >>= 1) {
        if (t < w) tree[t] += tree[t + w];
        __syncthreads();
    }
    if (t < k) count[t] = (long long)cnt[t];
    if (t == 0) inertia[0] = tree[0];
}

}  // namespace

extern "C" size_t igan_kmeans_workspace_bytes(int n, int k, int dim) {
    if (n < 1 || k < 1 || k > KM_MAX_K || dim < 1 || dim > KM_MAX_DIM) return 0;
    if ((long long)n * dim * 4 > 0x7FFFFFF0LL) return 0;
    return km_partial_bytes(n, k, dim) + km_dots_bytes(n, k);
}

extern "C" int igan_kmeans_step(igan_stream_t stream_, const float* X, const float* xnorm, const float* C, const float* cnorm,
                                int* label, double* d2, double* sums, long long* count, double* inertia, void* workspace, int n,
                                int k, int dim) {
    using namespace igan;
    IGAN_REQUIRE(X && xnorm && C && cnorm && label && d2 && sums && count && inertia && workspace, "kmeans_step: null buffer");
    IGAN_REQUIRE(n >= 1, "kmeans_step: n must be positive");
    if (k < 1 || k > KM_MAX_K) return fail(IGAN_ERR_UNSUPPORTED, "kmeans_step: 1 <= k <= 64 centres (a lane owns a centre)");
    if (dim < 1 || dim > KM_MAX_DIM) return fail(IGAN_ERR_UNSUPPORTED, "kmeans_step: 1 <= dim <= 4096");
    IGAN_REQUIRE((long long)n * dim * 4 <= 0x7FFFFFF0LL, "kmeans_step: row matrix too large (2 GiB per operand; pass it in chunks)");
    IGAN_REQUIRE((long long)n * k <= INT32_MAX, "kmeans_step: n * k exceeds the int32 element count of the product block");
    IGAN_REQUIRE((((uintptr_t)workspace) & 15) == 0, "kmeans_step: workspace must be 16-byte aligned");
    hipStream_t stream = (hipStream_t)stream_;
    double* partial = reinterpret_cast<double*>(workspace);
    float* dots = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + km_partial_bytes(n, k, dim));
    if (int rc = distance_products(stream_, X, C, dots, n, k, dim)) return rc;
    hipLaunchKernelGGL(kmeans_assign_kernel, dim3(ceil_div(n, 4)), dim3(256), 0, stream, dots, xnorm, cnorm, X, C, label, d2, n, k, dim);
    IGAN_LAUNCH_CHECK("kmeans_assign launch");
    const int slice_rows = km_slice_rows(n, dim), slices = km_slices(n, dim);
    hipLaunchKernelGGL(kmeans_sums_kernel, dim3(km_colblocks(dim), slices), dim3(KM_COLS), (size_t)k * KM_COLS * sizeof(double), stream,
                       X, label, partial, n, k, dim, slice_rows);
    IGAN_LAUNCH_CHECK("kmeans_sums launch");
    hipLaunchKernelGGL(kmeans_fold_kernel, dim3(ceil_div(k * dim, 256)), dim3(256), 0, stream, partial, sums, k * dim, slices);
    IGAN_LAUNCH_CHECK("kmeans_fold launch");
    hipLaunchKernelGGL(kmeans_totals_kernel, dim3(1), dim3(KM_TOT_NT), 0, stream, label, d2, count, inertia, n, k);
    IGAN_LAUNCH_CHECK("kmeans_totals launch");
    return IGAN_OK;
}
