// np.argmax of one fp32 row by one wavefront, shared by class_stats.hip (igan_class_hist_update) and softmax_xent.hip
// (igan_softmax_xent_fwd): the lowest index among equal maxima with -0.0 == +0.0, the index of the first NaN of a row that
// holds one, 0 for a row of -infinity.
//   lanes      lane l holds columns 4 g .. 4 g + 3 for g = l, l + 64, ... and column 4 (K / 4) + l of the K % 4 last ones -- an
//              assignment by COLUMN INDEX, so what a lane sees does not depend on where the matrix lies.  A group is one 16-byte
//              load declared 4-byte aligned: rows of an odd K start anywhere, the hardware's global loads need dword alignment only.
//   order      a lane walks its columns in ascending order under a STRICT comparison (a later equal value never wins, a NaN
//              beats every number and is beaten by nothing), then six xor steps reduce (value, index) lexicographically.
//              That order is total, so every lane ends with the same pair.
#pragma once
#include <hip/hip_runtime.h>

namespace {

typedef float cs_f4 __attribute__((ext_vector_type(4), aligned(4)));

constexpr int CS_NONE = 0x7fffffff;    // "no column yet"

// a lane's running best, columns offered in ascending order
__device__ inline void cs_offer(float v, int idx, float& bv, int& bi) {
    const bool bnan = bv != bv;
    if (bi == CS_NONE || (!bnan && (v != v || v > bv))) {
        bv = v;
        bi = idx;
    }
}

// does (ov, oi) come before (bv, bi)?  NaN first, then the larger value (-0.0 == +0.0), then the lower index
__device__ inline bool cs_beats(float ov, int oi, float bv, int bi) {
    if (oi == CS_NONE) return false;
    if (bi == CS_NONE) return true;
    const bool onan = ov != ov, bnan = bv != bv;
    if (onan != bnan) return onan;
    if (!onan && ov != bv) return ov > bv;
    return oi < bi;
}

__device__ inline int cs_row_argmax(const float* __restrict__ row, int K, int lane) {
    float bv = -__builtin_huge_valf();
    int bi = CS_NONE;
    const int groups = K >> 2;
    for (int g = lane; g < groups; g += 64) {
        const cs_f4 v = *reinterpret_cast<const cs_f4*>(row + 4 * g);
        cs_offer(v.x, 4 * g, bv, bi);
        cs_offer(v.y, 4 * g + 1, bv, bi);
        cs_offer(v.z, 4 * g + 2, bv, bi);
        cs_offer(v.w, 4 * g + 3, bv, bi);
    }
    const int c = 4 * groups + lane;
    if (lane < (K & 3)) cs_offer(row[c], c, bv, bi);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(bv, off, 64);
        const int oi = __shfl_xor(bi, off, 64);
        if (cs_beats(ov, oi, bv, bi)) {
            bv = ov;
            bi = oi;
        }
    }
    return bi;
}

}  // namespace
