// The ONE definition of the exact distance that the searches of exact_search.hip (IMLE 1-NN and k-NN, pr50k3) and kmeans.hip share.
// The radii the manifold search produces, the distances it compares with them and the 1-NN distances are the SAME function of
// two rows (symmetric, d2(a, a) == 0, summation order fixed by dim and the 16-byte alignment of the rows alone) because every
// kernel compiles these definitions; the screening product and its error interval are shared for the same reason, and the
// procedure built on them is exact_search.h.
#pragma once
#include "igan_common.h"
#include "fixed_order_sum.h"
#include <cmath>

namespace igan {

// Relative half-width of the interval the fp32 cancellation form a = |q|^2 + |c|^2 - 2 q.c is trusted to:
//     |a - d2_exact(q, c)|  <=  nn1_tol(dim) * (|q|^2 + |c|^2)
// as a BOUND, not an estimate: a pair the interval rules out is never measured, so a violation is a silently wrong neighbour.
//   * the product.  The widest chain any product family runs is ONE accumulator over the whole reduction (distance_products()
//     passes splits = 1): conv_fwd_kernel / conv_fwd_dma_kernel issue dim / 2 v_mfma_f32_32x32x2_f32 into one register, and the
//     instruction adds its two products one after the other, each with a rounding -- L = dim accumulate steps (measured: the
//     device's error on flat rows is that of a sequential fp32 sum with one product per step, not two).  dense_small_kernel and
//     thin_out_kernel split the reduction among lanes and fold: shorter chains.  Every order of `dim` products in which a term
//     meets at most `dim` roundings obeys |fl(q.c) - q.c| <= gamma_dim * sum|q_i c_i| <= gamma_dim * (|q|^2 + |c|^2) / 2 with
//     gamma_n = n u / (1 - n u), u = 2^-24; a holds twice that error.
//   * the norms are fp64 sums rounded to fp32: u * (|q|^2 + |c|^2) more, and the kernels' t is formed from the rounded norms,
//     which can fall short of the true ones by (1 - u).
// (dim + 2) u / (1 - (dim + 2) u) covers the three (2.9e-3 at dim 49 152).  The bound is attained to within a factor of a few
// by rows whose products all have one sign and one size -- flat images: blank or saturated frames, a collapsed generator --
// where every step rounds the same way and the error grows like dim: worst measured use of the interval 0.249 on flat rows on
// every tile kernel (conv_fwd_dma_kernel and the 128x128, 128x64, 128x32 and 32x128 instantiations of conv_fwd_kernel, vector
// and scalar loads) at every dim from 768 to 49 152, 0.025 on dense_small_kernel, 0.005 on thin_out_kernel; on rows that are
// not flat at most 0.035 (all-positive, offset and noisy-flat rows) and 0.01 (zero-mean rows) -- profiles/screening_interval.txt,
// asserted <= 0.5 per family by tests/test_gpu_screening.py.  The earlier statistical interval 2^-22 sqrt(dim)
// (errors as a random walk) was exceeded 13.8 times over on flat rows at dim 49 152 and lost the true neighbour there.
// A wider interval only costs more exact evaluations, never a wrong answer.
__device__ __forceinline__ double nn1_tol(int dim) {
    const double x = ((double)dim + 2.0) * 5.9604644775390625e-08;      // (dim + 2) * 2^-24
    return (x <= 0.5) ? x / (1.0 - x) : 1e300;     // 1 at dim = 2^23 - 2, still a bound; past it, it says nothing: every pair is measured
}

// Squared distance of two rows as a direct difference with fp64 accumulation (compute_dist, dci_code/src/util.c:62-69,
// before its sqrt), by one whole wavefront; the result is in every lane.  Fixed summation order: deterministic.
__device__ __forceinline__ double wave_sqdist(const float* __restrict__ a, const float* __restrict__ b, int dim, int lane) {
    double s0 = 0.0, s1 = 0.0;
    int i = lane * 4;
    if ((dim & 3) == 0 && ((((uintptr_t)a | (uintptr_t)b) & 15) == 0)) {
        for (; i + 256 < dim; i += 512) {      // two 16 B loads per operand in flight
            const float4 x0 = *reinterpret_cast<const float4*>(a + i), y0 = *reinterpret_cast<const float4*>(b + i);
            const float4 x1 = *reinterpret_cast<const float4*>(a + i + 256), y1 = *reinterpret_cast<const float4*>(b + i + 256);
            double d;
            d = (double)x0.x - (double)y0.x; s0 += d * d; d = (double)x0.y - (double)y0.y; s0 += d * d;
            d = (double)x0.z - (double)y0.z; s0 += d * d; d = (double)x0.w - (double)y0.w; s0 += d * d;
            d = (double)x1.x - (double)y1.x; s1 += d * d; d = (double)x1.y - (double)y1.y; s1 += d * d;
            d = (double)x1.z - (double)y1.z; s1 += d * d; d = (double)x1.w - (double)y1.w; s1 += d * d;
        }
        for (; i < dim; i += 256) {
            const float4 x0 = *reinterpret_cast<const float4*>(a + i), y0 = *reinterpret_cast<const float4*>(b + i);
            double d;
            d = (double)x0.x - (double)y0.x; s0 += d * d; d = (double)x0.y - (double)y0.y; s0 += d * d;
            d = (double)x0.z - (double)y0.z; s0 += d * d; d = (double)x0.w - (double)y0.w; s0 += d * d;
        }
    } else {
        for (int j = lane; j < dim; j += 64) {
            const double d = (double)a[j] - (double)b[j];
            s0 += d * d;
        }
    }
    return wave_sum(s0 + s1);
}

// The [nq x dim] x [dim x nc] product q.c of a query batch and a candidate batch on the exact-fp32 MFMA: a 1x1 convolution with the
// candidate matrix as a transposed filter -- both operands are read in their natural row-major [rows][dim] layout.
inline int distance_products(igan_stream_t stream_, const float* query, const float* cand, float* dots, int nq, int nc, int dim) {
    igan_conv2d_params p{};          // every optional field (epilogue, noise) zero
    p.x = query; p.w = cand; p.y = dots;
    p.in_scale = nullptr; p.out_scale = nullptr;
    p.workspace = nullptr; p.workspace_floats = 0;
    p.N = nq; p.H = 1; p.W = 1; p.Cin = dim;
    p.OH = 1; p.OW = 1; p.Cout = nc;
    p.KH = 1; p.KW = 1; p.stride = 1; p.up = 1; p.pad_y = 0; p.pad_x = 0;
    p.w_transposed = 1;  // cand is [nc][dim] == forward-layout [1][1][Cout][Cin]
    p.splits = 1;
    p.sliced_tiles = 0;
    p.alpha = 1.0f;
    p.bias = nullptr; p.act = 0; p.act_alpha = 0.0f; p.act_gain = 1.0f;
    return igan_conv2d(stream_, &p);
}

}  // namespace igan
