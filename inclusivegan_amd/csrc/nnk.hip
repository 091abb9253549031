// Exact streaming k-nearest-neighbours WITH indices for the exclusive IMLE assignment on gfx950.
//
// Behavioural contract: with `exclusive_retrieved_code` the reference asks its index for num_samples_factor neighbours per
// real image (training/training_loop.py:382-396, dci_query(num_neighbours = k)) and picks greedily among them; what the loop
// consumes is, per real, the k nearest candidates in ascending order with their Euclidean distances.
// MI355X design: the kernel between its two neighbours.  nn1.hip keeps ONE (distance, index) pair per query, knn_manifold.hip
// the kcap smallest distances without indices; this one keeps the k lexicographically smallest (distance, index) pairs.  The
// scheme is theirs: a candidate batch is one [nq x dim] x [dim x nc] product on the exact-fp32 MFMA, |q|^2 + |c|^2 - 2 q.c
// only SCREENS with the nn1_tol interval, every pair the interval cannot rule out is measured as a direct difference in fp64
// (wave_sqdist) and the choice is made on (exact distance, index).  The state is therefore a function of the SET of
// (row, index) pairs fed -- not of the order or the boundaries of the batches, bits of the distances included -- and
// candidates can be generated, folded and discarded, pack after pack.
#include "igan_common.h"
#include "exact_distance.h"

#include <cmath>

namespace {

using igan::nn1_tol;         // exact_distance.h: the one definition, shared with nn1.hip and knn_manifold.hip
using igan::wave_sqdist;

// knn_manifold.hip's sorted_insert, values only: the list of upper bounds of pass 1.
template <int KC>
__device__ __forceinline__ void bound_insert(double (&l)[KC], double v) {
#pragma unroll
    for (int i = 0; i < KC; i++) {
        const double lo = (v < l[i]) ? v : l[i];
        v = (v < l[i]) ? l[i] : v;
        l[i] = lo;
    }
}

// The same insertion carrying the index: (v, vi) goes into the list ascending by (distance, index), the largest pair drops out.
// Static indices only: both lists stay in registers.
template <int KC>
__device__ __forceinline__ void pair_insert(double (&d)[KC], int (&x)[KC], double v, int vi) {
#pragma unroll
    for (int i = 0; i < KC; i++) {
        const bool first = (v < d[i]) || (v == d[i] && vi < x[i]);
        const double dl = first ? v : d[i];
        const int xl = first ? vi : x[i];
        v = first ? d[i] : v;
        vi = first ? x[i] : vi;
        d[i] = dl;
        x[i] = xl;
    }
}

// One wavefront per query; KC >= k is the compiled list length.
//   pass 1  U = the k-th smallest UPPER bound a + t over this batch and the running state (whose exact values are their own
//           bounds): k distinct points lie within U, so the k-th smallest exact distance does too.  Every lane keeps the KC
//           smallest bounds it met in registers; k rounds of a wave minimum then pop them in order.
//   pass 2  in index order: a candidate whose LOWER bound a - t exceeds U cannot be among the k smallest pairs (equality
//           stays in: a candidate that ties the k-th distance with a lower index displaces it); every other one is measured
//           exactly and inserted when (e, index) < the k-th pair; U follows the running k-th exact distance down.
// A NaN bound decides nothing (such a candidate is measured); a non-finite exact distance never enters.
template <int KC>
__global__ __launch_bounds__(256) void nnk_fold_kernel(const float* __restrict__ dots, const float* __restrict__ qnorm,
                                                       const float* __restrict__ cnorm, const float* __restrict__ query,
                                                       const float* __restrict__ cand, double* __restrict__ best_d2,
                                                       int* __restrict__ best_idx, int nq, int nc, int dim, int k, int idx_base) {
    const int q = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (q >= nq) return;
    const double inf = (double)INFINITY;
    const double qn = (double)qnorm[q];
    const double tol = nn1_tol(dim);
    const float* drow = dots + (size_t)q * nc;
    // pass 1 (lane 0's list starts as the state's distances; the state itself is read after this pass, which keeps the
    // wave-uniform copy out of the scalar registers while the bound lists are live)
    double l[KC];
#pragma unroll
    for (int i = 0; i < KC; i++) {
        double v = inf;
        if (lane == 0 && i < k) v = best_d2[(size_t)q * k + i];
        l[i] = (v < inf) ? v : inf;
    }
    for (int c = lane; c < nc; c += 64) {
        const double cn = (double)cnorm[c];
        const double a = qn + cn - 2.0 * (double)drow[c];
        const double hi = a + tol * (qn + cn);
        if (hi < l[KC - 1]) bound_insert<KC>(l, hi);        // false for a NaN bound
    }
    double u = inf;
    for (int r = 0; r < k; r++) {
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
    // The k pairs sit RIGHT-aligned in the KC slots, behind KC - k sentinels (-inf, INT32_MIN) that nothing displaces: the k-th
    // pair is always slot KC - 1, a static index.
    const int pad = KC - k;
    double sd[KC];
    int si[KC];
#pragma unroll
    for (int i = 0; i < KC; i++) {
        const int s = (i >= pad) ? i - pad : 0;          // always a valid slot: the loads need no branch
        const double v = best_d2[(size_t)q * k + s];
        const int vi = best_idx[(size_t)q * k + s];
        sd[i] = (i >= pad) ? ((v < inf) ? v : inf) : -inf;
        si[i] = (i >= pad) ? ((v < inf) ? vi : INT32_MAX) : INT32_MIN;
    }
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
            const int gi = idx_base + c0 + j;
            if (e < inf && (e < sd[KC - 1] || (e == sd[KC - 1] && gi < si[KC - 1]))) {      // false for NaN and +inf
                pair_insert<KC>(sd, si, e, gi);
                u = (sd[KC - 1] < u) ? sd[KC - 1] : u;
            }
        }
    }
    // lane i writes slot i: one store per list instead of KC guarded ones
    double od = inf;
    int oi = INT32_MAX;
#pragma unroll
    for (int i = 0; i < KC; i++) {
        od = (lane == i) ? sd[i] : od;
        oi = (lane == i) ? si[i] : oi;
    }
    if (lane >= pad && lane < KC) {
        best_d2[(size_t)q * k + (lane - pad)] = od;
        best_idx[(size_t)q * k + (lane - pad)] = oi;
    }
}

}  // namespace

extern "C" int igan_nnk_update(igan_stream_t stream_, const float* query, const float* qnorm,
                               const float* cand, const float* cnorm, double* best_d2, int* best_idx,
                               float* dots, int nq, int nc, int dim, int k, int idx_base) {
    using namespace igan;
    IGAN_REQUIRE(query && qnorm && cand && cnorm && best_d2 && best_idx && dots, "nnk_update: null buffer");
    IGAN_REQUIRE(nq >= 1 && nc >= 1 && dim >= 1, "nnk_update: sizes must be positive");
    if (k < 1 || k > 16) return fail(IGAN_ERR_UNSUPPORTED, "nnk_update: 1 <= k <= 16 neighbours (the lists live in registers)");
    IGAN_REQUIRE(idx_base >= 0 && (long long)idx_base + nc <= INT32_MAX, "nnk_update: candidate index overflows int32");
    IGAN_REQUIRE((long long)nq * dim * 4 <= 0x7FFFFFF0LL, "nnk_update: query batch too large (2 GiB per operand)");
    IGAN_REQUIRE((long long)nc * dim * 4 <= 0x7FFFFFF0LL, "nnk_update: candidate batch too large (2 GiB per operand)");
    IGAN_REQUIRE((long long)nq * nc <= INT32_MAX, "nnk_update: product block too large");
    if (int rc = distance_products(stream_, query, cand, dots, nq, nc, dim)) return rc;
    const dim3 grid(ceil_div(nq, 4)), block(256);
    hipStream_t stream = (hipStream_t)stream_;
    if (k <= 4)
        hipLaunchKernelGGL(nnk_fold_kernel<4>, grid, block, 0, stream, dots, qnorm, cnorm, query, cand, best_d2, best_idx, nq, nc, dim, k, idx_base);
    else if (k <= 8)
        hipLaunchKernelGGL(nnk_fold_kernel<8>, grid, block, 0, stream, dots, qnorm, cnorm, query, cand, best_d2, best_idx, nq, nc, dim, k, idx_base);
    else
        hipLaunchKernelGGL(nnk_fold_kernel<16>, grid, block, 0, stream, dots, qnorm, cnorm, query, cand, best_d2, best_idx, nq, nc, dim, k, idx_base);
    IGAN_LAUNCH_CHECK("nnk_fold launch");
    return IGAN_OK;
}
