// Perceptual path length (ppl_zfull .. ppl2_wend) on gfx950: the two pieces of metrics/perceptual_path_length.py that are
// neither G nor the LPIPS network.
//
//   igan_ppl_endpoints   the two path endpoints of every pair (:19-30 normalize / slerp, :59-77 lerp / slerp at t and
//                        t + epsilon, interleaved).  The two rows of a pair differ by about epsilon = 1e-4 of their size, and the
//                        metric divides what that difference does to the image by epsilon^2: the formulas run in fp64 from the
//                        fp32 inputs and every output is rounded to fp32 once, so that the difference carries no more than the
//                        two final roundings.  lerp is the three fp64 operations a + (b - a) * t, never contracted into an FMA
//                        (equal to numpy bit for bit).  slerp: one wavefront per pair, the pair's rows in registers for
//                        dim <= 1024 (16 values per lane), five wave reductions through lane shuffles, no LDS memory.
//   igan_ppl_crop_prep   crop, box-mean downsample and range change (:84-96) in one pass over G's image batch in whatever
//                        strides it has, written channel-minor for the VGG convolutions.
// Both are streaming kernels: 16-byte accesses where the addresses allow them, nothing staged.
#include "igan_common.h"
#include "fixed_order_sum.h"

#include <cmath>

namespace {

using igan::wave_sum;

// ---------------------------------------------------------------------------------------------------------------------
// lerp

__device__ __forceinline__ void lerp2(float a, float b, double t0, double t1, float& o0, float& o1) {
#pragma clang fp contract(off)
    const double x = (double)a, d = (double)b - (double)a;
    const double p0 = d * t0, p1 = d * t1;
    o0 = (float)(x + p0);
    o1 = (float)(x + p1);
}

// VEC: dim % 4 == 0 and 16-byte aligned buffers; one thread per four values of one pair.  Otherwise one thread per value.
template <bool VEC>
__global__ __launch_bounds__(256) void ppl_lerp_kernel(const float* __restrict__ lat, const float* __restrict__ t,
                                                       float* __restrict__ out, int n, int dim, double epsilon) {
    const int per_row = VEC ? dim >> 2 : dim;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)n * per_row) return;
    const int i = (int)(idx / per_row);
    const int j = (int)(idx - (long long)i * per_row) * (VEC ? 4 : 1);
    const double t0 = (double)t[i];
    const double t1 = t0 + epsilon;
    const size_t ra = (size_t)(2 * i) * dim + j, rb = ra + dim;
    if (VEC) {
        const float4 a = *reinterpret_cast<const float4*>(lat + ra), b = *reinterpret_cast<const float4*>(lat + rb);
        float4 o0, o1;
        lerp2(a.x, b.x, t0, t1, o0.x, o1.x);
        lerp2(a.y, b.y, t0, t1, o0.y, o1.y);
        lerp2(a.z, b.z, t0, t1, o0.z, o1.z);
        lerp2(a.w, b.w, t0, t1, o0.w, o1.w);
        *reinterpret_cast<float4*>(out + ra) = o0;
        *reinterpret_cast<float4*>(out + rb) = o1;
    } else {
        float o0, o1;
        lerp2(lat[ra], lat[rb], t0, t1, o0, o1);
        out[ra] = o0;
        out[rb] = o1;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// slerp


// The lane's share of one pair's two rows.  each(f) calls f(a_j, b_j) for every element j < dim the lane owns;
// each_store(g) does the same with g(a_j, b_j, o0, o1) and writes o0 to the row at t, o1 to the row at t + epsilon.
// REG: dim <= 1024, the values are loaded once and stay in registers (static indices only).  VEC as in the lerp kernel:
// lane l owns the float4 at 4 l of every 256-value chunk, otherwise the values l, l + 64, ...
template <bool REG, bool VEC>
struct PairRows {
    const float* pa;
    const float* pb;
    float* q0;
    float* q1;
    int dim, lane;
    float a[REG ? 16 : 1], b[REG ? 16 : 1];

    __device__ __forceinline__ PairRows(const float* lat, float* out, int pair, int dim_, int lane_) : dim(dim_), lane(lane_) {
        pa = lat + (size_t)(2 * pair) * dim;
        pb = pa + dim;
        q0 = out + (size_t)(2 * pair) * dim;
        q1 = q0 + dim;
        if (REG) {
            if (VEC) {
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    const int j = c * 256 + lane * 4;
                    float4 x = make_float4(0.f, 0.f, 0.f, 0.f), y = x;
                    if (j < dim) {
                        x = *reinterpret_cast<const float4*>(pa + j);
                        y = *reinterpret_cast<const float4*>(pb + j);
                    }
                    a[4 * c] = x.x; a[4 * c + 1] = x.y; a[4 * c + 2] = x.z; a[4 * c + 3] = x.w;
                    b[4 * c] = y.x; b[4 * c + 1] = y.y; b[4 * c + 2] = y.z; b[4 * c + 3] = y.w;
                }
            } else {
#pragma unroll
                for (int k = 0; k < 16; k++) {
                    const int j = k * 64 + lane;
                    a[k] = (j < dim) ? pa[j] : 0.f;
                    b[k] = (j < dim) ? pb[j] : 0.f;
                }
            }
        }
    }

    template <class F>
    __device__ __forceinline__ void each(F&& f) const {
        if (REG) {
#pragma unroll
            for (int k = 0; k < 16; k++) {
                const int j = VEC ? ((k >> 2) * 256 + lane * 4 + (k & 3)) : (k * 64 + lane);
                if (j < dim) f(a[k], b[k]);
            }
        } else if (VEC) {
            for (int j = lane * 4; j < dim; j += 256) {
                const float4 x = *reinterpret_cast<const float4*>(pa + j), y = *reinterpret_cast<const float4*>(pb + j);
                f(x.x, y.x); f(x.y, y.y); f(x.z, y.z); f(x.w, y.w);
            }
        } else {
            for (int j = lane; j < dim; j += 64) f(pa[j], pb[j]);
        }
    }

    template <class G>
    __device__ __forceinline__ void each_store(G&& g) const {
        if (REG && VEC) {
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const int j = c * 256 + lane * 4;
                if (j < dim) {
                    float4 o0, o1;
                    g(a[4 * c], b[4 * c], o0.x, o1.x);
                    g(a[4 * c + 1], b[4 * c + 1], o0.y, o1.y);
                    g(a[4 * c + 2], b[4 * c + 2], o0.z, o1.z);
                    g(a[4 * c + 3], b[4 * c + 3], o0.w, o1.w);
                    *reinterpret_cast<float4*>(q0 + j) = o0;
                    *reinterpret_cast<float4*>(q1 + j) = o1;
                }
            }
        } else if (REG) {
#pragma unroll
            for (int k = 0; k < 16; k++) {
                const int j = k * 64 + lane;
                if (j < dim) g(a[k], b[k], q0[j], q1[j]);
            }
        } else if (VEC) {
            for (int j = lane * 4; j < dim; j += 256) {
                const float4 x = *reinterpret_cast<const float4*>(pa + j), y = *reinterpret_cast<const float4*>(pb + j);
                float4 o0, o1;
                g(x.x, y.x, o0.x, o1.x);
                g(x.y, y.y, o0.y, o1.y);
                g(x.z, y.z, o0.z, o1.z);
                g(x.w, y.w, o0.w, o1.w);
                *reinterpret_cast<float4*>(q0 + j) = o0;
                *reinterpret_cast<float4*>(q1 + j) = o1;
            }
        } else {
            for (int j = lane; j < dim; j += 64) g(pa[j], pb[j], q0[j], q1[j]);
        }
    }
};

// perceptual_path_length.py:23-30, statement for statement, in fp64:
//   a^ = a / |a|;  b^ = b / |b|;  d = a^ . b^;  c = b^ - d a^;  c^ = c / |c|;  p = t acos(d);  v = a^ cos p + c^ sin p;  v / |v|
// No special case: a zero row or a pair with c == 0 divides by zero and the row is NaN, as in the reference.
template <bool REG, bool VEC>
__global__ __launch_bounds__(256) void ppl_slerp_kernel(const float* __restrict__ lat, const float* __restrict__ t,
                                                        float* __restrict__ out, int n, int dim, double epsilon) {
    const int pair = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (pair >= n) return;          // whole wavefronts leave together
    const PairRows<REG, VEC> rows(lat, out, pair, dim, lane);

    double sa = 0.0, sb = 0.0;
    rows.each([&](float x, float y) { sa += (double)x * (double)x; sb += (double)y * (double)y; });
    const double na = sqrt(wave_sum(sa)), nb = sqrt(wave_sum(sb));

    double sd = 0.0;
    rows.each([&](float x, float y) { sd += ((double)x / na) * ((double)y / nb); });
    const double d = wave_sum(sd);

    double sc = 0.0;
    rows.each([&](float x, float y) {
        const double c = (double)y / nb - d * ((double)x / na);
        sc += c * c;
    });
    const double nc = sqrt(wave_sum(sc));

    const double omega = acos(d);
    const double t0 = (double)t[pair];
    const double t1 = t0 + epsilon;
    const double p0 = t0 * omega, p1 = t1 * omega;
    const double c0 = cos(p0), s0 = sin(p0), c1 = cos(p1), s1 = sin(p1);

    double sv0 = 0.0, sv1 = 0.0;
    rows.each([&](float x, float y) {
        const double ah = (double)x / na;
        const double ch = ((double)y / nb - d * ah) / nc;
        const double v0 = ah * c0 + ch * s0, v1 = ah * c1 + ch * s1;
        sv0 += v0 * v0;
        sv1 += v1 * v1;
    });
    const double nv0 = sqrt(wave_sum(sv0)), nv1 = sqrt(wave_sum(sv1));

    rows.each_store([&](float x, float y, float& o0, float& o1) {
        const double ah = (double)x / na;
        const double ch = ((double)y / nb - d * ah) / nc;
        o0 = (float)((ah * c0 + ch * s0) / nv0);
        o1 = (float)((ah * c1 + ch * s1) / nv1);
    });
}

// ---------------------------------------------------------------------------------------------------------------------
// crop + box mean + range change

struct CropArgs {
    const float* x;
    float* y;
    long long sn, sc, sh, sw;       // element strides of x[n][c][h][w]
    int C, oh, ow, y0, x0, factor;
    long long total;                // N * oh * ow * C outputs
    float inv;                      // 1 / factor^2
    int packed;                     // x is channel-minor with dense pixels (sc == 1, sw == C) and factor == 1
};

__device__ __forceinline__ float crop_value(const CropArgs& p, int o) {      // total <= INT32_MAX
#pragma clang fp contract(off)
    const int c = o % p.C;
    int r = o / p.C;
    const int ox = r % p.ow;
    r /= p.ow;
    const int oy = r % p.oh;
    const long long n = r / p.oh;
    const float* src = p.x + n * p.sn + c * p.sc + (long long)(p.y0 + oy * p.factor) * p.sh + (long long)(p.x0 + ox * p.factor) * p.sw;
    float s = 0.f;
    for (int dy = 0; dy < p.factor; dy++)
        for (int dx = 0; dx < p.factor; dx++) s += src[dy * p.sh + dx * p.sw];
    const float m = s * p.inv;
    return (m + 1.0f) * 127.5f;
}

// One thread per four consecutive outputs (one 16-byte store; the last thread may own fewer).  A packed input row is a
// contiguous run of the output row's values: four outputs inside one row come from one 16-byte load when it is aligned.
__global__ __launch_bounds__(256) void ppl_crop_prep_kernel(CropArgs p) {
    const long long o = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (o >= p.total) return;
    if (o + 4 <= p.total) {
        float4 v;
        const int row = p.ow * p.C;
        const int in_row = (int)o % row;
        bool done = false;
        if (p.packed && in_row + 4 <= row) {
            const int r = (int)o / row;
            const int oy = r % p.oh;
            const long long n = r / p.oh;
            const float* src = p.x + n * p.sn + (long long)(p.y0 + oy) * p.sh + (long long)p.x0 * p.sw + in_row;
            if (((uintptr_t)src & 15) == 0) {
                const float4 u = *reinterpret_cast<const float4*>(src);
                v.x = (u.x * p.inv + 1.0f) * 127.5f;        // inv == 1: the product is exact, contracted or not
                v.y = (u.y * p.inv + 1.0f) * 127.5f;
                v.z = (u.z * p.inv + 1.0f) * 127.5f;
                v.w = (u.w * p.inv + 1.0f) * 127.5f;
                done = true;
            }
        }
        if (!done) {
            v.x = crop_value(p, (int)o);
            v.y = crop_value(p, (int)o + 1);
            v.z = crop_value(p, (int)o + 2);
            v.w = crop_value(p, (int)o + 3);
        }
        *reinterpret_cast<float4*>(p.y + o) = v;
    } else {
        for (int k = (int)o; k < p.total; k++) p.y[k] = crop_value(p, k);
    }
}

template <bool REG, bool VEC>
void launch_slerp(hipStream_t stream, const float* lat, const float* t, float* out, int n, int dim, double epsilon) {
    hipLaunchKernelGGL((ppl_slerp_kernel<REG, VEC>), dim3(igan::ceil_div(n, 4)), dim3(256), 0, stream, lat, t, out, n, dim, epsilon);
}

}  // namespace

extern "C" int igan_ppl_endpoints(igan_stream_t stream_, const float* lat, const float* t, float* out, int n, int dim,
                                  double epsilon, int mode) {
    using namespace igan;
    IGAN_REQUIRE(lat && t && out, "ppl_endpoints: null buffer");
    IGAN_REQUIRE(n >= 1 && dim >= 1, "ppl_endpoints: sizes must be positive");
    IGAN_REQUIRE((long long)2 * n * dim <= INT32_MAX, "ppl_endpoints: latent batch too large");
    IGAN_REQUIRE(mode == 0 || mode == 1, "ppl_endpoints: mode must be 0 (lerp) or 1 (slerp)");
    IGAN_REQUIRE(std::isfinite(epsilon), "ppl_endpoints: epsilon must be finite");
    {
        const uintptr_t l0 = (uintptr_t)lat, o0 = (uintptr_t)out, bytes = (uintptr_t)2 * n * dim * sizeof(float);
        IGAN_REQUIRE(o0 + bytes <= l0 || l0 + bytes <= o0, "ppl_endpoints: out must not alias lat");
    }
    hipStream_t stream = (hipStream_t)stream_;
    const bool vec = (dim & 3) == 0 && ((((uintptr_t)lat | (uintptr_t)out) & 15) == 0);
    if (mode == 0) {
        const long long threads = (long long)n * (vec ? dim >> 2 : dim);
        const dim3 grid((unsigned)ceil_div_ll(threads, 256)), block(256);
        if (vec) hipLaunchKernelGGL(ppl_lerp_kernel<true>, grid, block, 0, stream, lat, t, out, n, dim, epsilon);
        else hipLaunchKernelGGL(ppl_lerp_kernel<false>, grid, block, 0, stream, lat, t, out, n, dim, epsilon);
    } else {
        const bool reg = dim <= 1024;
        if (reg && vec) launch_slerp<true, true>(stream, lat, t, out, n, dim, epsilon);
        else if (reg) launch_slerp<true, false>(stream, lat, t, out, n, dim, epsilon);
        else if (vec) launch_slerp<false, true>(stream, lat, t, out, n, dim, epsilon);
        else launch_slerp<false, false>(stream, lat, t, out, n, dim, epsilon);
    }
    IGAN_LAUNCH_CHECK("ppl_endpoints launch");
    return IGAN_OK;
}

extern "C" int igan_ppl_crop_prep(igan_stream_t stream_, const float* x, float* y, int N, int C, int H, int W,
                                  int y0, int y1, int x0, int x1, int factor,
                                  long long stride_n, long long stride_c, long long stride_h, long long stride_w) {
    using namespace igan;
    IGAN_REQUIRE(x && y, "ppl_crop_prep: null buffer");
    IGAN_REQUIRE(((uintptr_t)y & 15) == 0, "ppl_crop_prep: y must be 16-byte aligned");
    IGAN_REQUIRE(N >= 1 && C >= 1 && H >= 1 && W >= 1, "ppl_crop_prep: sizes must be positive");
    IGAN_REQUIRE(0 <= y0 && y0 < y1 && y1 <= H && 0 <= x0 && x0 < x1 && x1 <= W, "ppl_crop_prep: crop window must be non-empty and inside the image");
    IGAN_REQUIRE(factor >= 1, "ppl_crop_prep: factor must be >= 1");
    IGAN_REQUIRE((y1 - y0) % factor == 0 && (x1 - x0) % factor == 0, "ppl_crop_prep: factor must divide both sides of the crop window");
    IGAN_REQUIRE(stride_n >= 0 && stride_c >= 0 && stride_h >= 0 && stride_w >= 0, "ppl_crop_prep: strides must not be negative");
    const int oh = (y1 - y0) / factor, ow = (x1 - x0) / factor;
    const long long total = (long long)N * oh * ow * C;
    IGAN_REQUIRE(total <= INT32_MAX && (long long)ow * C <= INT32_MAX, "ppl_crop_prep: output too large");
    CropArgs p;
    p.x = x; p.y = y;
    p.sn = stride_n; p.sc = stride_c; p.sh = stride_h; p.sw = stride_w;
    p.C = C; p.oh = oh; p.ow = ow; p.y0 = y0; p.x0 = x0; p.factor = factor;
    p.total = total;
    p.inv = 1.0f / ((float)factor * (float)factor);
    p.packed = (factor == 1 && stride_c == 1 && stride_w == C) ? 1 : 0;
    hipLaunchKernelGGL(ppl_crop_prep_kernel, dim3((unsigned)ceil_div_ll(ceil_div_ll(total, 4), 256)), dim3(256), 0, (hipStream_t)stream_, p);
    IGAN_LAUNCH_CHECK("ppl_crop_prep launch");
    return IGAN_OK;
}
