// The procedure every exact search shares (exact_search.hip: 1-NN, k-NN with indices, k-th radius, manifold membership, ball
// count; kmeans.hip: nearest centre), each piece defined once.  One wavefront owns a query.  The fp32 MFMA product only SCREENS:
// a = |q|^2 + |c|^2 - 2 q.c is trusted to the interval of nn1_tol (exact_distance.h), a candidate the interval cannot rule out is
// a CONTENDER, every contender is measured by wave_sqdist in fp64 and the choice is made on exact values.  A mistake here is a
// silently wrong neighbour in all six kernels.
#pragma once
#include "exact_distance.h"

namespace igan {

struct Interval { double lo, hi; };

// [a - t, a + t] with a = qn + cn - 2 dot and t = tol * (qn + cn): the exact squared distance lies inside (nn1_tol).
__device__ __forceinline__ Interval screen_interval(double qn, double cn, double dot, double tol) {
    const double a = qn + cn - 2.0 * dot;
    const double t = tol * (qn + cn);
    return {a - t, a + t};
}

// One query's view of a candidate batch: the interval of candidate c from the query's row of the product block.
struct Screen {
    const float* drow;       // dots[q][0 .. nc)
    const float* cnorm;
    double qn, tol;
    __device__ __forceinline__ Interval operator()(int c) const { return screen_interval(qn, (double)cnorm[c], (double)drow[c], tol); }
};

// NaN policy.  An fp32 product or norm that overflowed makes the interval NaN: it decides nothing.  Whether a candidate with
// lower bound `lo` contends against the bound `u` is one of these two predicates, which differ for a NaN `lo` only:
//   the 1-NN DROPS an undecidable candidate -- it is never measured and never wins, whatever its exact distance;
//   the k-lists, the membership test, the ball count and k-means MEASURE it -- it enters when its fp64 distance is finite.
// So igan_nnk_update with k = 1 and igan_nn1_update agree while the screening values are not NaN (include/igan_hip.h).
__device__ __forceinline__ bool contends_if_decided(double lo, double u) { return lo <= u; }
__device__ __forceinline__ bool contends_unless_ruled_out(double lo, double u) { return !(lo > u); }

// Minimum over the wavefront, in every lane.  A NaN never replaces a number.
__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_xor(v, off, 64);
        v = (o < v) ? o : v;
    }
    return v;
}

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

// U = the k-th smallest value over the lanes' ascending lists l (k <= KC), which it consumes: k rounds of a wave minimum, the
// first lane that owns the minimum pops it.  With l holding every lane's KC smallest UPPER bounds a + t of a batch (and the
// running state's exact values, their own bounds), k distinct points lie within U, so the k-th smallest exact distance does too.
template <int KC>
__device__ __forceinline__ double kth_smallest(double (&l)[KC], int k, int lane) {
    double u = (double)INFINITY;
    for (int r = 0; r < k; r++) {
        u = wave_min(l[0]);
        const unsigned long long owners = __ballot(l[0] == u);
        if (lane == __ffsll((long long)owners) - 1) {
#pragma unroll
            for (int i = 0; i + 1 < KC; i++) l[i] = l[i + 1];
            l[KC - 1] = (double)INFINITY;
        }
    }
    return u;
}

// The same, after adding the upper bounds of the batch to the lists (a NaN bound is no bound: it is not inserted).
template <int KC>
__device__ __forceinline__ double kth_upper_bound(const Screen& s, int nc, double (&l)[KC], int k, int lane) {
    for (int c = lane; c < nc; c += 64) {
        const double hi = s(c).hi;
        if (hi < l[KC - 1]) sorted_insert<KC>(l, hi);
    }
    return kth_smallest<KC>(l, k, lane);
}

// The contender walk: the contenders of one strip of 64 candidates (lane j holds candidate c0 + j), handed to the whole wave in
// index order.  A kernel supplies the lane-local test and the body, which is wave-uniform and may `continue` past a contender
// that a bound lowered since the ballot no longer admits, or `break`:
//     for (ContenderStrip strip(c < nc && contends_...(lo, u)); strip.next(j);) { e = wave_sqdist(qrow, cand + (c0 + j) * dim, ...); ... }
// An iterator, not a function taking two lambdas: with the lambdas knn_radius_fold_kernel<8> needed 94 VGPRs for 80 and lost a
// wave per SIMD (profiles/exact_search.txt).
struct ContenderStrip {
    unsigned long long mask;
    __device__ __forceinline__ explicit ContenderStrip(bool contends) : mask(__ballot(contends)) {}
    __device__ __forceinline__ bool next(int& j) {
        if (!mask) return false;
        j = __ffsll((long long)mask) - 1;
        mask &= mask - 1;
        return true;
    }
};

}  // namespace igan
