// The ONE definition of the summation orders of the element-wise kernels: DESIGN.md's "every reduction has a fixed order".
// The bits of a float sum depend on which term meets which and when, so each function below states its order exactly --
// which lane or thread adds what, in which sequence, and who holds the result.  Those comments are the contract: the
// graph == eager bitwise test, the non-finite suite's "bit-identical on the unreachable elements" and the digests under
// tools/ hold because every kernel compiles these definitions and none spells an order of its own.
// Wavefronts are 64 lanes and workgroups 256 threads throughout.
#pragma once
#include <hip/hip_runtime.h>

namespace igan {

// Butterfly sum of one value per lane over a wavefront; EVERY lane holds the sum.
// Six steps, off = 32, 16, 8, 4, 2, 1: lane l replaces v by v(l) + v(l ^ off).  After the step with offset `off` a lane holds
// the sum of the lanes that differ from it only in the bits >= off, so the final value is the balanced tree over lane
// indices (((l0 + l32) + (l16 + l48)) + ...), with the operands of each addition in an order that depends on the lane:
// floating-point addition commutes, so all lanes agree on the bits.  T is float, double or int.
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// Shift sum of one value per lane over a wavefront; ONLY LANE 0 holds the sum (every other lane holds a partial sum that
// mixed in values from lanes that wrapped: unspecified).
// Six steps, off = 32, 16, 8, 4, 2, 1: lane l replaces v by v(l) + v(l + off) (its own value again where l + off >= 64).  Lane 0
// ends with the same balanced tree over lane indices as wave_sum, every addition with the lower lane's operand on the left.
// A different contract from wave_sum, not another spelling: the two compile to different code and a site keeps its form.
template <typename T>
__device__ __forceinline__ T wave_sum_lane0(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// Sum of one value per thread over a workgroup of 256; EVERY thread holds the sum.
// Each of the four wavefronts runs wave_sum_lane0; lane 0 of wavefront w stores its sum to red[w] (red: >= 4 floats of LDS);
// one barrier; every thread returns (red[0] + red[1]) + (red[2] + red[3]).
// Barriers: exactly one, between the stores and the reads, unless RED_HELD_V: then v was read from red[threadIdx.x] itself
// and a second barrier stands between the shuffles and the stores, so that no wavefront overwrites red[0..3] before every
// thread has read its own slot.  No barrier follows the reads: a caller that writes red again (a second call included)
// puts one between.  All 256 threads must reach the call.
template <bool RED_HELD_V = false>
__device__ __forceinline__ float block_sum_256(float v, float* red) {
    v = wave_sum_lane0(v);
    if (RED_HELD_V) __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// The thread layout of the channel-minor streaming reductions (scale_dot, bias_act_noise backward): a workgroup of 256 is
// rl row lanes x cvt float4 columns, thread t = row lane t / cvt, column t % cvt; the 256 % cvt last threads idle.
struct RowLanes {
    int cvt;      // float4 columns per workgroup: min(C / 4, 256)
    int rl;       // row lanes: 256 / cvt
};
__host__ __device__ inline RowLanes row_lanes(int C) {      // C >= 4, a multiple of 4
    const int cv = C >> 2;
    const int cvt = cv < 256 ? cv : 256;
    return {cvt, 256 / cvt};
}
// workgroups that leave every row lane >= 8 rows of `rows` (0 when there are too few rows for one: callers clamp)
inline int row_lane_blocks(int rows, int C) { return rows / (row_lanes(C).rl * 8); }

// Fold of the row lanes of N float4 accumulator arrays (red[a][256] in LDS, slot t written by thread t, a barrier passed
// since) into out[a][0..3].  Called by the threads t < cvt that own a live column; thread t computes, per array and per
// component, ((red[t] + red[t + cvt]) + red[t + 2 cvt]) + ... + red[t + (rl - 1) cvt]: row lanes in ascending order, serially,
// and stores x, y, z, w to out[a][0], [1], [2], [3].  One loop over the row lanes serves all N arrays; no barrier inside.
template <int N>
__device__ __forceinline__ void row_lane_fold(const float4* const (&red)[N], RowLanes L, float* const (&out)[N]) {
    float4 t[N];
#pragma unroll
    for (int a = 0; a < N; a++) t[a] = red[a][threadIdx.x];
    for (int j = 1; j < L.rl; j++) {
        float4 u[N];
#pragma unroll
        for (int a = 0; a < N; a++) u[a] = red[a][threadIdx.x + j * L.cvt];
#pragma unroll
        for (int a = 0; a < N; a++) { t[a].x += u[a].x; t[a].y += u[a].y; t[a].z += u[a].z; t[a].w += u[a].w; }
    }
#pragma unroll
    for (int a = 0; a < N; a++) { out[a][0] = t[a].x; out[a][1] = t[a].y; out[a][2] = t[a].z; out[a][3] = t[a].w; }
}

// Sum over the blocks b0 <= j < b1 of partial[j * stride + column] by a workgroup of 256 seen as 16 columns x 16 groups: thread t
// serves one column (the caller's `column`, its own for each t & 15) in group g = t >> 4; `live` says whether that column
// exists.  The sum is valid in group 0 (t < 16) of live columns; every other thread gets 0.
//   1. group g walks j = b0 + g, b0 + g + 16, ... in ascending order.  While four of its terms remain (j + 48 < b1) they go
//      to s0, s1, s2, s3 in turn (s_k += term j + 16 k), then j += 64; the at most three terms left all go to s0.
//      s = (s0 + s1) + (s2 + s3).
//   2. s to red[t] (red: 256 floats of LDS; dead columns store 0), one barrier -- all 256 threads must reach the call.
//   3. thread t < 16 returns ((0 + red[t]) + red[16 + t]) + ... + red[240 + t]: groups in ascending order, serially.
__device__ __forceinline__ float column_fold_16x16(const float* partial, int stride, int b0, int b1, int column, bool live, float* red) {
    const int grp = threadIdx.x >> 4;
    float s = 0.f;
    if (live) {
        // four independent partial sums: four loads in flight per lane instead of a chain of dependent L2 round trips
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        int j = b0 + grp;
        for (; j + 48 < b1; j += 64) {
            s0 += partial[(size_t)j * stride + column];        s1 += partial[(size_t)(j + 16) * stride + column];
            s2 += partial[(size_t)(j + 32) * stride + column]; s3 += partial[(size_t)(j + 48) * stride + column];
        }
        for (; j < b1; j += 16) s0 += partial[(size_t)j * stride + column];
        s = (s0 + s1) + (s2 + s3);
    }
    red[threadIdx.x] = s;
    __syncthreads();
    float t = 0.f;
    if (grp == 0 && live) {
#pragma unroll
        for (int g = 0; g < 16; g++) t += red[g * 16 + threadIdx.x];
    }
    return t;
}

// Sum over first <= j < end of p[j * stride + column] by ONE thread, four accumulators: while four terms remain (j + 3 < end) they go
// to s0, s1, s2, s3 in turn (s_k += term j + k), then j += 4; the at most three terms left all go to s0 in ascending order.
// Returns (s0 + s1) + (s2 + s3).  Four loads in flight instead of a chain of dependent L2 round trips.
__device__ __forceinline__ float serial_sum4(const float* p, int stride, int first, int end, int column) {
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int j = first;
    for (; j + 3 < end; j += 4) {
        s0 += p[(long long)(j + 0) * stride + column];
        s1 += p[(long long)(j + 1) * stride + column];
        s2 += p[(long long)(j + 2) * stride + column];
        s3 += p[(long long)(j + 3) * stride + column];
    }
    for (; j < end; j++) s0 += p[(long long)j * stride + column];
    return (s0 + s1) + (s2 + s3);
}

// acc + the terms term(first), term(first + 1), ..., term(end - 1) by ONE thread with ONE fp64 accumulator that starts at acc:
// (((acc + term(first)) + term(first + 1)) + ...) + term(end - 1), ascending, serially, one rounding per term.  `term` is called
// once per j in that order and may keep counts of its own; a term that must not take part returns +0.0 (x + 0.0 == x for every
// x but -0.0).  The loads behind `term` do not depend on the sum, so an unrolled loop keeps several in flight; the additions
// stay one chain.
template <typename F>
__device__ __forceinline__ double serial_sum_f64(double acc, int first, int end, F term) {
#pragma unroll 4
    for (int j = first; j < end; j++) acc += term(j);
    return acc;
}

}  // namespace igan
