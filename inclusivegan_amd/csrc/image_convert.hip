// fp32 image batch <-> uint8 on gfx950: the two inference transforms of dnnlib/tflib/tfutil.py:245-267
// (convert_images_from_uint8 / convert_images_to_uint8), the statements every generator script and every metric's fake
// image path put between G and its consumer.
//
//   igan_images_to_uint8     box-mean shrink, range change, saturating cast and the optional NCHW -> NHWC transpose in one
//                            pass over G's image batch in whatever strides it has: 4 bytes read and 1 written per value,
//                            against four element-wise passes plus a permuted copy.
//   igan_images_from_uint8   the way back (NCHW or NHWC bytes -> NCHW fp32).
// Both are streaming kernels.  One thread owns four consecutive pixels of an output row for all channels: 16-byte loads where
// the addresses allow them, bytes packed into dwords before the store, nothing staged.
//
// The range change is a multiply and an add that are never contracted (file-level fp contract(off)): images that were uint8 once
// sit one ulp from (k - 128) / 127.5, where a fused multiply-add gives another byte than the reference's two roundings.
#include "igan_common.h"

#include <climits>

// Whole file: no multiply is ever fused with an add.  hipcc contracts by default -- also across __fmul_rn / __fadd_rn, whose
// bodies are plain operators compiled under the header's own (contracting) mode: measured, the two intrinsics came out as one
// v_fma_f32.  So the arithmetic below is written with plain operators, under this pragma.
#pragma clang fp contract(off)

namespace {

// tf.saturate_cast(v, uint8) for finite v; NaN -> 0 (the reference leaves it to an undefined cast, this kernel defines it).
__device__ __forceinline__ unsigned to_byte(float m, float scale, float bias) {
    const float v = m * scale + bias;     // two roundings (see the pragma above)
    if (!(v >= 0.0f)) return 0u;        // negatives, -inf, NaN
    if (v >= 255.0f) return 255u;       // +inf included
    return (unsigned)(int)v;            // truncates
}

struct ToU8Args {
    const float* x;
    unsigned char* y;
    int sn, sc, sh, sw;     // element strides of x[n][c][h][w]; every offset fits int32 (checked on the host)
    int C, oh, ow, qw;      // qw = ceil(ow / 4) threads per output row
    int shrink, nhwc;
    int items;              // N * oh * qw
    float inv, scale, bias; // inv = 1 / shrink^2
};

// Box means of up to four consecutive output pixels of one channel, m[k] for k < cnt; src = the first value of the first box.
// S: compile-time shrink (1, 2, 4), 0 = p.shrink.  The sum runs rows then columns from 0.f in fp32, then one multiply by inv;
// S == 1 passes x through.  vec: cnt == 4, sw == 1 and every row of the boxes starts 16-byte aligned.
template <int S>
__device__ __forceinline__ void box_means(const ToU8Args& p, const float* __restrict__ src, int cnt, bool vec, float (&m)[4]) {
    if (S == 1) {
        if (vec) {
            const float4 v = *reinterpret_cast<const float4*>(src);
            m[0] = v.x; m[1] = v.y; m[2] = v.z; m[3] = v.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) m[k] = (k < cnt) ? src[k * p.sw] : 0.0f;
        }
        return;
    }
    if (S > 1 && vec) {
        float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int dy = 0; dy < S; dy++) {
            const float4* row = reinterpret_cast<const float4*>(src + dy * p.sh);
#pragma unroll
            for (int j = 0; j < S; j++) {       // 4 S values of the row = S float4; value 4 j + e belongs to pixel (4 j + e) / S
                const float4 v = row[j];
                s[(4 * j + 0) / S] = s[(4 * j + 0) / S] + v.x;
                s[(4 * j + 1) / S] = s[(4 * j + 1) / S] + v.y;
                s[(4 * j + 2) / S] = s[(4 * j + 2) / S] + v.z;
                s[(4 * j + 3) / S] = s[(4 * j + 3) / S] + v.w;
            }
        }
#pragma unroll
        for (int k = 0; k < 4; k++) m[k] = s[k] * p.inv;
        return;
    }
    const int f = S ? S : p.shrink;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        float s = 0.0f;
        if (k < cnt) {
            const float* b = src + k * f * p.sw;
            for (int dy = 0; dy < f; dy++)
                for (int dx = 0; dx < f; dx++) s += b[dy * p.sh + dx * p.sw];
        }
        m[k] = s * p.inv;
    }
}

// CT: compile-time channel count 1..4, 0 = p.C (any).  Grid-stride over the N * oh * qw quads.
template <int CT, int S>
__global__ __launch_bounds__(256) void images_to_uint8_kernel(ToU8Args p) {
    const int C = CT ? CT : p.C;
    const int f = S ? S : p.shrink;
    const int step = (int)(gridDim.x * blockDim.x);
    for (long long it = (long long)blockIdx.x * blockDim.x + threadIdx.x; it < p.items; it += step) {
        const int item = (int)it;
        const int q = item % p.qw;
        const int r = item / p.qw;
        const int oy = r % p.oh;
        const int n = r / p.oh;
        const int ox = q * 4;
        const int cnt = min(4, p.ow - ox);
        const float* base = p.x + n * p.sn + (oy * f) * p.sh + (ox * f) * p.sw;
        // 16-byte loads: a full quad of a unit-stride row whose box rows all start on a 16-byte boundary
        bool vec = S != 0 && cnt == 4 && p.sw == 1 && (p.sc & 3) == 0 && ((uintptr_t)base & 15) == 0;
        if (S > 1) vec = vec && (p.sh & 3) == 0;
        const int pix = (n * p.oh + oy) * p.ow + ox;        // first output pixel of the quad, NHWC pixel index

        if (p.nhwc) {
            unsigned char* dst = p.y + (long long)pix * C;
            if (CT) {
                unsigned b[4 * (CT ? CT : 1)];              // byte k * C + c: pixel-major, the order of the output run
                if (S == 1 && cnt == 4 && p.sc == 1 && p.sw == CT && ((uintptr_t)base & 15) == 0) {
                    // channel-minor input with dense pixels: the quad's 4 C values are one contiguous run in the output's order
#pragma unroll
                    for (int j = 0; j < (CT ? CT : 1); j++) {
                        const float4 v = reinterpret_cast<const float4*>(base)[j];
                        b[4 * j] = to_byte(v.x, p.scale, p.bias);
                        b[4 * j + 1] = to_byte(v.y, p.scale, p.bias);
                        b[4 * j + 2] = to_byte(v.z, p.scale, p.bias);
                        b[4 * j + 3] = to_byte(v.w, p.scale, p.bias);
                    }
                } else {
#pragma unroll
                    for (int c = 0; c < (CT ? CT : 1); c++) {
                        float m[4];
                        box_means<S>(p, base + c * p.sc, cnt, vec, m);
#pragma unroll
                        for (int k = 0; k < 4; k++) b[k * CT + c] = to_byte(m[k], p.scale, p.bias);
                    }
                }
                if (cnt == 4 && ((uintptr_t)dst & 3) == 0) {
                    unsigned w[CT ? CT : 1];
#pragma unroll
                    for (int d = 0; d < (CT ? CT : 1); d++) w[d] = b[4 * d] | (b[4 * d + 1] << 8) | (b[4 * d + 2] << 16) | (b[4 * d + 3] << 24);
                    if (CT == 4 && ((uintptr_t)dst & 15) == 0) {
                        *reinterpret_cast<uint4*>(dst) = make_uint4(w[0], w[CT > 1 ? 1 : 0], w[CT > 2 ? 2 : 0], w[CT > 3 ? 3 : 0]);
                    } else {
#pragma unroll
                        for (int d = 0; d < (CT ? CT : 1); d++) reinterpret_cast<unsigned*>(dst)[d] = w[d];
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < 4; k++)
                        if (k < cnt) {
#pragma unroll
                            for (int c = 0; c < (CT ? CT : 1); c++) dst[k * CT + c] = (unsigned char)b[k * CT + c];
                        }
                }
            } else {
                for (int c = 0; c < C; c++) {
                    float m[4];
                    box_means<S>(p, base + c * p.sc, cnt, vec, m);
#pragma unroll
                    for (int k = 0; k < 4; k++)
                        if (k < cnt) dst[k * C + c] = (unsigned char)to_byte(m[k], p.scale, p.bias);
                }
            }
        } else {
            for (int c = 0; c < C; c++) {
                float m[4];
                box_means<S>(p, base + c * p.sc, cnt, vec, m);
                unsigned char* dst = p.y + ((long long)(n * C + c) * p.oh + oy) * p.ow + ox;
                unsigned b[4];
#pragma unroll
                for (int k = 0; k < 4; k++) b[k] = to_byte(m[k], p.scale, p.bias);
                if (cnt == 4 && ((uintptr_t)dst & 3) == 0) {
                    *reinterpret_cast<unsigned*>(dst) = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
                } else {
#pragma unroll
                    for (int k = 0; k < 4; k++)
                        if (k < cnt) dst[k] = (unsigned char)b[k];
                }
            }
        }
    }
}

template <int CT>
void launch_to_uint8(hipStream_t stream, const ToU8Args& p, int blocks) {
    const dim3 grid(blocks), block(256);
    switch (p.shrink) {
    case 1: hipLaunchKernelGGL((images_to_uint8_kernel<CT, 1>), grid, block, 0, stream, p); break;
    case 2: hipLaunchKernelGGL((images_to_uint8_kernel<CT, 2>), grid, block, 0, stream, p); break;
    case 4: hipLaunchKernelGGL((images_to_uint8_kernel<CT, 4>), grid, block, 0, stream, p); break;
    default: hipLaunchKernelGGL((images_to_uint8_kernel<CT, 0>), grid, block, 0, stream, p); break;
    }
}

struct FromU8Args {
    const unsigned char* x;
    float* y;
    int C, HW, nhwc;
    int total;              // N * C * H * W
    float scale, bias;
};

__device__ __forceinline__ float from_byte(unsigned b, float scale, float bias) {
    return (float)b * scale + bias;       // two roundings
}

// One thread per four consecutive values of y (NCHW).  NCHW bytes: the same four positions of x, one dword when aligned.
__global__ __launch_bounds__(256) void images_from_uint8_kernel(FromU8Args p) {
    const int quads = (p.total + 3) >> 2;
    const int step = (int)(gridDim.x * blockDim.x);
    for (long long it = (long long)blockIdx.x * blockDim.x + threadIdx.x; it < quads; it += step) {
        const int o = (int)it * 4;
        const int cnt = min(4, p.total - o);
        unsigned b[4] = {0u, 0u, 0u, 0u};
        if (!p.nhwc) {
            if (cnt == 4 && ((uintptr_t)(p.x + o) & 3) == 0) {
                const unsigned w = *reinterpret_cast<const unsigned*>(p.x + o);
                b[0] = w & 255u; b[1] = (w >> 8) & 255u; b[2] = (w >> 16) & 255u; b[3] = w >> 24;
            } else {
#pragma unroll
                for (int k = 0; k < 4; k++)
                    if (k < cnt) b[k] = p.x[o + k];
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (k < cnt) {
                    const int e = o + k;                    // y index ((n C + c) HW + s)  ->  x index ((n HW + s) C + c)
                    const int s = e % p.HW;
                    const int nc = e / p.HW;
                    const int c = nc % p.C;
                    const int n = nc / p.C;
                    b[k] = p.x[((long long)n * p.HW + s) * p.C + c];
                }
        }
        if (cnt == 4 && ((uintptr_t)(p.y + o) & 15) == 0) {
            *reinterpret_cast<float4*>(p.y + o) = make_float4(from_byte(b[0], p.scale, p.bias), from_byte(b[1], p.scale, p.bias),
                                                              from_byte(b[2], p.scale, p.bias), from_byte(b[3], p.scale, p.bias));
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (k < cnt) p.y[o + k] = from_byte(b[k], p.scale, p.bias);
        }
    }
}

int grid_blocks(long long threads) {
    const long long want = igan::ceil_div_ll(threads, 256);
    return (int)(want < 8192 ? want : 8192);        // 256 CUs x 32 resident blocks; the grid-stride loop takes the rest
}

}  // namespace

extern "C" int igan_images_to_uint8(igan_stream_t stream_, const float* x, unsigned char* y, int N, int C, int H, int W, int shrink,
                                    float scale, float bias, int nhwc,
                                    long long stride_n, long long stride_c, long long stride_h, long long stride_w) {
    using namespace igan;
    IGAN_REQUIRE(x && y, "images_to_uint8: null buffer");
    IGAN_REQUIRE(shrink >= 1, "images_to_uint8: shrink must be >= 1");
    IGAN_REQUIRE(C >= 1, "images_to_uint8: C must be >= 1");
    IGAN_REQUIRE(N >= 1 && H >= 1 && W >= 1, "images_to_uint8: sizes must be positive");
    IGAN_REQUIRE(nhwc == 0 || nhwc == 1, "images_to_uint8: nhwc must be 0 or 1");
    IGAN_REQUIRE(stride_n >= 0 && stride_c >= 0 && stride_h >= 0 && stride_w >= 0, "images_to_uint8: strides must not be negative");
    const int oh = H / shrink, ow = W / shrink;     // floors, like VALID pooling
    IGAN_REQUIRE(oh >= 1 && ow >= 1, "images_to_uint8: empty output (shrink exceeds a side)");
    IGAN_REQUIRE((long long)N * C * H * W <= INT32_MAX, "images_to_uint8: image batch too large (N*C*H*W must fit 32 bits)");
    const long long last = (long long)(N - 1) * stride_n + (long long)(C - 1) * stride_c + (long long)(H - 1) * stride_h + (long long)(W - 1) * stride_w;
    IGAN_REQUIRE(stride_n <= INT32_MAX && stride_c <= INT32_MAX && stride_h <= INT32_MAX && stride_w <= INT32_MAX && last <= INT32_MAX,
                 "images_to_uint8: image batch too large (strided offsets must fit 32 bits)");
    ToU8Args p;
    p.x = x; p.y = y;
    p.sn = (int)stride_n; p.sc = (int)stride_c; p.sh = (int)stride_h; p.sw = (int)stride_w;
    p.C = C; p.oh = oh; p.ow = ow; p.qw = ceil_div(ow, 4);
    p.shrink = shrink; p.nhwc = nhwc;
    p.items = N * oh * p.qw;                        // <= N * H * W
    p.inv = 1.0f / ((float)shrink * (float)shrink);
    p.scale = scale; p.bias = bias;
    hipStream_t stream = (hipStream_t)stream_;
    const int blocks = grid_blocks(p.items);
    switch (C) {
    case 1: launch_to_uint8<1>(stream, p, blocks); break;
    case 2: launch_to_uint8<2>(stream, p, blocks); break;
    case 3: launch_to_uint8<3>(stream, p, blocks); break;
    case 4: launch_to_uint8<4>(stream, p, blocks); break;
    default: launch_to_uint8<0>(stream, p, blocks); break;
    }
    IGAN_LAUNCH_CHECK("images_to_uint8 launch");
    return IGAN_OK;
}

extern "C" int igan_images_from_uint8(igan_stream_t stream_, const unsigned char* x, float* y, int N, int C, int H, int W,
                                      float scale, float bias, int nhwc_in) {
    using namespace igan;
    IGAN_REQUIRE(x && y, "images_from_uint8: null buffer");
    IGAN_REQUIRE(C >= 1, "images_from_uint8: C must be >= 1");
    IGAN_REQUIRE(N >= 1 && H >= 1 && W >= 1, "images_from_uint8: sizes must be positive");
    IGAN_REQUIRE(nhwc_in == 0 || nhwc_in == 1, "images_from_uint8: nhwc_in must be 0 or 1");
    IGAN_REQUIRE((long long)N * C * H * W <= INT32_MAX - 3, "images_from_uint8: image batch too large (N*C*H*W must fit 32 bits)");
    FromU8Args p;
    p.x = x; p.y = y;
    p.C = C; p.HW = H * W; p.nhwc = nhwc_in;
    p.total = N * C * H * W;
    p.scale = scale; p.bias = bias;
    hipLaunchKernelGGL(images_from_uint8_kernel, dim3(grid_blocks(ceil_div(p.total, 4))), dim3(256), 0, (hipStream_t)stream_, p);
    IGAN_LAUNCH_CHECK("images_from_uint8 launch");
    return IGAN_OK;
}
