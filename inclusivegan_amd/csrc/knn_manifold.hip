// Exact k-NN manifold search for the precision / recall metric (pr50k3) on gfx950.
//
// Behavioural contract: the reference estimates a manifold as one hypersphere per point, its radius the distance to the
// point's k-th neighbour (metrics/precision_recall.py:73-90: np.partition of a [10 000 x n] fp16 distance block on the
// host), and calls a sample "in" when it lies within the radius of any point (:119-120, `<=`).
// MI355X design: the same streaming pattern as the 1-NN (nn1.hip).  A candidate batch is one [nq x dim] x [dim x nc]
// product on the exact-fp32 MFMA; |q|^2 + |c|^2 - 2 q.c only SCREENS, with the error interval nn1.hip trusts it to, and
// every pair the interval cannot decide is measured as a direct difference in fp64.  Two folds, one wavefront per query:
//   knn_radius_fold      a running sorted list of the kcap smallest exact distances (a MULTISET of values: duplicates
//                        count, so the value at position k is what np.partition leaves there);
//   manifold_member_fold an any-within-radius reduction against per-candidate radii.
// Both results are functions of exact distances only, hence independent of the order the batches arrive in.
#include "igan_common.h"
#include "exact_distance.h"

#include <cmath>

namespace {

// nn1_tol and wave_sqdist have ONE definition (exact_distance.h), which nn1.hip compiles too.
using igan::nn1_tol;
using igan::wave_sqdist;

// Insert v into the ascending list l[0..KC) and drop the largest.  Static indices only: the list stays in registers.
template <int KC>
__device__ __forceinline__ void sorted_insert(double (&l)[KC], double v) {
#pragma unroll
    for (int i = 0; i < KC; i++) {
        const double lo = (v < l[i]) ? v : l[i];
        v = (v < l[i]) ? l[i] : v;
        l[i] = lo;
    }
}

// One wavefront per query; KC >= kcap is the compiled list length.
//   pass 1  U = the kcap-th smallest UPPER bound a + t over this batch and the running state (whose exact values are their
//           own upper bounds): kcap distinct points lie within U, so the kcap-th smallest exact distance does too.  Every
//           lane keeps the KC smallest bounds it met in registers; kcap rounds of a wave minimum then pop them in order.
//   pass 2  a candidate whose LOWER bound a - t exceeds U cannot be among the kcap smallest; every other one is measured
//           exactly and inserted; U follows the running exact value at position kcap - 1 down.
// A non-finite bound decides nothing (such a candidate is measured); a non-finite exact distance counts as +inf.
template <int KC>
__global__ __launch_bounds__(256) void knn_radius_fold_kernel(const float* __restrict__ dots, const float* __restrict__ qnorm,
                                                              const float* __restrict__ cnorm, const float* __restrict__ query,
                                                              const float* __restrict__ cand, double* __restrict__ kth_d2,
                                                              int nq, int nc, int dim, int kcap) {
    const int q = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (q >= nq) return;
    const double inf = (double)INFINITY;
    const double qn = (double)qnorm[q];
    const double tol = nn1_tol(dim);
    const float* drow = dots + (size_t)q * nc;
    double st[KC], l[KC];
#pragma unroll
    for (int i = 0; i < KC; i++) {
        const double v = (i < kcap) ? kth_d2[(size_t)q * kcap + i] : inf;
        st[i] = (v < inf) ? v : inf;
        l[i] = (lane == 0) ? st[i] : inf;
    }
    // pass 1
    for (int c = lane; c < nc; c += 64) {
        const double cn = (double)cnorm[c];
        const double a = qn + cn - 2.0 * (double)drow[c];
        const double hi = a + tol * (qn + cn);
        if (hi < l[KC - 1]) sorted_insert<KC>(l, hi);      // false for a NaN bound
    }
    double u = inf;
    for (int r = 0; r < kcap; r++) {
        double m = l[0];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double o = __shfl_xor(m, off, 64);
            m = (o < m) ? o : m;
        }
        const unsigned long long owners = __ballot(l[0] == m);
        if (lane == __ffsll((long long)owners) - 1) {
#pragma unroll
            for (int i = 0; i + 1 < KC; i++) l[i] = l[i + 1];
            l[KC - 1] = inf;
        }
        u = m;
    }
    // pass 2
    const float* qrow = query + (size_t)q * dim;
    for (int c0 = 0; c0 < nc; c0 += 64) {
        const int c = c0 + lane;
        bool contender = false;
        if (c < nc) {
            const double cn = (double)cnorm[c];
            const double a = qn + cn - 2.0 * (double)drow[c];
            contender = !((a - tol * (qn + cn)) > u);
        }
        unsigned long long mask = __ballot(contender);
        while (mask) {
            const int j = __ffsll((long long)mask) - 1;
            mask &= mask - 1;
            const double e = wave_sqdist(qrow, cand + (size_t)(c0 + j) * dim, dim, lane);
            if (e < st[KC - 1]) {                              // false for NaN and +inf: neither can move a finite entry
                sorted_insert<KC>(st, e);
                double b = inf;
#pragma unroll
                for (int i = 0; i < KC; i++) b = (i == kcap - 1) ? st[i] : b;
                u = (b < u) ? b : u;
            }
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < KC; i++)
            if (i < kcap) kth_d2[(size_t)q * kcap + i] = st[i];
    }
}

// One wavefront per query; bit s of `in` is member[q][s].  For a pair (q, c) and column s with radius R = cand_radius[c][s]:
//   a + t <= R (and finite)  definitely inside;   a - t > R  definitely outside;   otherwise the exact distance decides
//   (isfinite(e) && e <= R, the reference's `<=` at precision_recall.py:119).
// A NaN anywhere fails the first two tests and the exact one: such a pair is never a witness.
__global__ __launch_bounds__(256) void manifold_member_fold_kernel(const float* __restrict__ dots, const float* __restrict__ qnorm,
                                                                   const float* __restrict__ cnorm, const float* __restrict__ query,
                                                                   const float* __restrict__ cand, const double* __restrict__ cand_radius,
                                                                   int* __restrict__ member, int nq, int nc, int dim, int nk) {
    const int q = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (q >= nq) return;
    const double inf = (double)INFINITY;
    const unsigned full = (1u << nk) - 1u;
    unsigned in = 0;
    for (int s = 0; s < nk; s++)
        if (member[(size_t)q * nk + s] != 0) in |= 1u << s;
    if (in == full) return;
    const double qn = (double)qnorm[q];
    const double tol = nn1_tol(dim);
    const float* drow = dots + (size_t)q * nc;
    const float* qrow = query + (size_t)q * dim;
    for (int c0 = 0; c0 < nc && in != full; c0 += 64) {
        const int c = c0 + lane;
        unsigned sure = 0, need = 0;
        if (c < nc) {
            const double cn = (double)cnorm[c];
            const double a = qn + cn - 2.0 * (double)drow[c];
            const double t = tol * (qn + cn);
            const double hi = a + t, lo = a - t;
            for (int s = 0; s < nk; s++) {
                const double R = cand_radius[(size_t)c * nk + s];
                if (hi < inf && hi <= R) sure |= 1u << s;
                else if (!(lo > R)) need |= 1u << s;
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) sure |= __shfl_xor(sure, off, 64);
        in |= sure;
        if (in == full) break;
        unsigned long long mask = __ballot((need & ~in) != 0u);
        while (mask) {
            const int j = __ffsll((long long)mask) - 1;
            mask &= mask - 1;
            const unsigned todo = (unsigned)__shfl((int)need, j, 64) & ~in;
            if (todo == 0u) continue;
            const double e = wave_sqdist(qrow, cand + (size_t)(c0 + j) * dim, dim, lane);
            if (e < inf) {
                for (int s = 0; s < nk; s++)
                    if (((todo >> s) & 1u) && e <= cand_radius[(size_t)(c0 + j) * nk + s]) in |= 1u << s;
            }
            if (in == full) break;
        }
    }
    if (lane == 0) {
        for (int s = 0; s < nk; s++)
            if ((in >> s) & 1u) member[(size_t)q * nk + s] = 1;
    }
}

}  // namespace

#define IGAN_KNN_REQUIRE_SIZES(name)                                                                                          \
    IGAN_REQUIRE(nq >= 1 && nc >= 1 && dim >= 1, name ": sizes must be positive");                                             \
    IGAN_REQUIRE((long long)nq * dim * 4 <= 0x7FFFFFF0LL, name ": query batch too large (2 GiB per operand)");                 \
    IGAN_REQUIRE((long long)nc * dim * 4 <= 0x7FFFFFF0LL, name ": candidate batch too large (2 GiB per operand)");             \
    IGAN_REQUIRE((long long)nq * nc <= INT32_MAX, name ": product block too large")

extern "C" int igan_knn_radius_update(igan_stream_t stream_, const float* query, const float* qnorm,
                                      const float* cand, const float* cnorm, double* kth_d2,
                                      float* dots, int nq, int nc, int dim, int kcap) {
    using namespace igan;
    IGAN_REQUIRE(query && qnorm && cand && cnorm && kth_d2 && dots, "knn_radius_update: null buffer");
    IGAN_KNN_REQUIRE_SIZES("knn_radius_update");
    IGAN_REQUIRE(kcap >= 1 && kcap <= 16, "knn_radius_update: kcap must be in [1, 16]");
    if (int rc = distance_products(stream_, query, cand, dots, nq, nc, dim)) return rc;
    const dim3 grid(ceil_div(nq, 4)), block(256);
    hipStream_t stream = (hipStream_t)stream_;
    if (kcap <= 4)
        hipLaunchKernelGGL(knn_radius_fold_kernel<4>, grid, block, 0, stream, dots, qnorm, cnorm, query, cand, kth_d2, nq, nc, dim, kcap);
    else if (kcap <= 8)
        hipLaunchKernelGGL(knn_radius_fold_kernel<8>, grid, block, 0, stream, dots, qnorm, cnorm, query, cand, kth_d2, nq, nc, dim, kcap);
    else
        hipLaunchKernelGGL(knn_radius_fold_kernel<16>, grid, block, 0, stream, dots, qnorm, cnorm, query, cand, kth_d2, nq, nc, dim, kcap);
    IGAN_LAUNCH_CHECK("knn_radius_fold launch");
    return IGAN_OK;
}

extern "C" int igan_manifold_member_update(igan_stream_t stream_, const float* query, const float* qnorm,
                                           const float* cand, const float* cnorm, const double* cand_radius,
                                           int* member, float* dots, int nq, int nc, int dim, int nk) {
    using namespace igan;
    IGAN_REQUIRE(query && qnorm && cand && cnorm && cand_radius && member && dots, "manifold_member_update: null buffer");
    IGAN_KNN_REQUIRE_SIZES("manifold_member_update");
    IGAN_REQUIRE(nk >= 1 && nk <= 8, "manifold_member_update: nk must be in [1, 8]");
    if (int rc = distance_products(stream_, query, cand, dots, nq, nc, dim)) return rc;
    hipLaunchKernelGGL(manifold_member_fold_kernel, dim3(ceil_div(nq, 4)), dim3(256), 0, (hipStream_t)stream_, dots, qnorm, cnorm,
                       query, cand, cand_radius, member, nq, nc, dim, nk);
    IGAN_LAUNCH_CHECK("manifold_member_fold launch");
    return IGAN_OK;
}
