// Differentiable augmentation of the images D sees (Zhao et al., "Differentiable Augmentation for Data-Efficient GAN Training",
// NeurIPS 2020; the reference has no such step) on gfx950: colour, translation and cutout of a channel-minor fp32 batch
// x[n][H][W][C], 1 <= C <= 4, forward and the exact transpose, from one row u[b][0..7] of fp32 uniforms in [0, 1) per sample.
//
// Behavioural contract (include/igan_hip.h states it in full; DESIGN.md "Differentiable augmentation"):
//   draw(u, k) = min(floor(fl32(u * k)), k - 1)                 the product rounded to fp32; the clamp holds it below k whatever that rounding does
//   colour       b = u0 - 1/2, s = 2 u1, c = u2 + 1/2;  m = mean of the sample's C H W inputs (fp64 sum, rounded to fp32 once);  M = m + b
//                per pixel xb_c = x_c + b, p = (xb_0 + ... + xb_{C-1}) / C,  v_c = ((xb_c - p) s + p - M) c + M      fp32, never contracted
//   translation  S = (H + 4) / 8 rows, t_y = draw(u4, 2 S + 1) - S (columns: W, u3);  w(i, j) = v(i + t_y, j + t_x) inside the image, else 0
//   cutout       K = (H + 1) / 2 rows, r = 1 - K % 2, o = draw(u6, H + r);  rows o - K / 2 <= i < o - K / 2 + K are cut (columns: W, u5);
//                a pixel whose row AND column are cut is 0
//   backward     g(i, j) = dy(i - t_y, j - t_x) where that position is inside the image and not cut, else 0;  without colour dx = g;
//                with colour G = mean of the sample's C H W values of g (fp64 sum, rounded once), q = (g_0 + ... + g_{C-1}) / C,
//                dx_c = (c s) g_c + (c (1 - s)) q + (1 - c) G
// A cut or shifted-out value is a SELECT of 0, never a product: it is exactly +0 whatever its source holds.  Without colour a kept
// value is a bit copy.  With colour a non-finite input makes m, and with it every kept value of ITS sample, non-finite; other
// samples share nothing with it.
//
// MI355X design.  The op moves 2 * n H W C * 4 bytes (4.7 MB at [12, 3, 128, 128]; colour reads the batch once more) and computes a dozen operations per value: it is a
// launch and a memory round trip, so the work is to keep it at ONE pass (two with colour) and every access whole pixels.
//   apply   one thread per output pixel, 256 per workgroup, a workgroup inside one sample: the sample's parameters are wave-uniform
//           (the eight uniforms arrive as scalar loads), the C channels of a pixel are one vector load and one vector store (dword,
//           dwordx2, dwordx3, dwordx4 for C = 1 .. 4), adjacent lanes take adjacent pixels of a row, so a wavefront's accesses are one
//           contiguous segment of 64 C dwords shifted by the translation.  The source pixel is loaded only where it is kept.
//   reduce  (colour only) sample b's H W pixels are cut into DA slices(H W) contiguous slices of pixels_per_slice(H W) pixels, one
//           workgroup of 256 per slice, and the summation order is
//             1. thread t walks the pixels lo + t, lo + t + 256, ... of its slice in ascending order with ONE fp64 accumulator that
//                starts at +0.0 (igan::serial_sum_f64); the term of a pixel is ((x_0 + x_1) + x_2) + x_3 in fp64 over its C channels
//                (backward: over the C values of dy at a kept position; +0.0 at a position that is cut or shifted out);
//             2. each of the four wavefronts folds its 64 accumulators with igan::wave_sum_lane0<double>; lane 0 of wavefront w stores
//                the sum to red[w]; one barrier; thread 0 stores (red[0] + red[1]) + (red[2] + red[3]) to partial[b * slices + slice];
//             3. the apply kernel: every thread adds its sample's partials 0, 1, ..., slices - 1 in ascending order to +0.0 with one fp64
//                accumulator (igan::serial_sum_f64), divides by C H W in fp64 and rounds to fp32 once.
//           The slice count depends on H W alone, so a sample's bits do not depend on n or on its place in the batch.  No atomic.
// Nothing is allocated, nothing is read back, every launch is on the caller's stream: the two launches capture into a hipGraph, and
// the bits of every output are a function of (n, C, H, W, policy) and the data.
#include "igan_common.h"
#include "fixed_order_sum.h"

namespace {

constexpr int DA_NT = 256;
constexpr int DA_SLICE_PIXELS = 1024;     // a slice is at least this long (four pixels per thread) until DA_MAX_SLICES is reached
constexpr int DA_MAX_SLICES = 16;

enum { DA_COLOR = 1, DA_TRANSLATION = 2, DA_CUTOUT = 4, DA_ALL = 7 };

__host__ __device__ inline int da_slices(int hw) {
    const int s = (hw + DA_SLICE_PIXELS - 1) / DA_SLICE_PIXELS;
    return s < DA_MAX_SLICES ? s : DA_MAX_SLICES;
}
__host__ __device__ inline int da_pixels_per_slice(int hw) { return (hw + da_slices(hw) - 1) / da_slices(hw); }

template <int C>
struct Pixel {
    float v[C];
};
template <>
struct alignas(8) Pixel<2> {
    float v[2];
};
template <>
struct alignas(16) Pixel<4> {
    float v[4];
};

// min(floor(fl32(u * k)), k - 1), and never below 0: u is a uniform in [0, 1), and whatever else arrives (a NaN, a value outside the
// interval) still names a parameter inside its range
__device__ __forceinline__ int da_draw(float u, int k) {
#pragma clang fp contract(off)
    const float f = u * (float)k;
    if (!(f >= 1.0f)) return 0;               // a NaN fails the comparison
    return f >= (float)(k - 1) ? k - 1 : (int)f;
}

struct Geometry {
    int ty, tx;                 // translation
    int cy0, cy1, cx0, cx1;     // cut rows [cy0, cy1) and columns [cx0, cx1), not yet intersected with the image; empty without cutout
};

__device__ __forceinline__ Geometry da_geometry(const float* __restrict__ u, int H, int W, int policy) {
    Geometry g = {0, 0, 0, 0, 0, 0};
    if (policy & DA_TRANSLATION) {
        const int sy = (H + 4) >> 3, sx = (W + 4) >> 3;
        g.tx = da_draw(u[3], 2 * sx + 1) - sx;
        g.ty = da_draw(u[4], 2 * sy + 1) - sy;
    }
    if (policy & DA_CUTOUT) {
        const int ky = (H + 1) >> 1, kx = (W + 1) >> 1;
        g.cx0 = da_draw(u[5], W + 1 - (kx & 1)) - (kx >> 1);
        g.cy0 = da_draw(u[6], H + 1 - (ky & 1)) - (ky >> 1);
        g.cx1 = g.cx0 + kx;
        g.cy1 = g.cy0 + ky;
    }
    return g;
}

__device__ __forceinline__ bool da_cut(const Geometry& g, int i, int j) { return i >= g.cy0 && i < g.cy1 && j >= g.cx0 && j < g.cx1; }
__device__ __forceinline__ bool da_inside(int i, int j, int H, int W) { return (unsigned)i < (unsigned)H && (unsigned)j < (unsigned)W; }

// Output position (i, j) -> the position (si, sj) its value comes from, and whether it is kept.
//   forward:  y(i, j)  <- x(i + t_y, j + t_x), kept where the source is inside the image and (i, j) itself is not cut
//   backward: dx(i, j) <- dy(i - t_y, j - t_x), kept where that position is inside the image and not cut
template <bool BWD>
__device__ __forceinline__ bool da_source(const Geometry& g, int i, int j, int H, int W, int& si, int& sj) {
    si = BWD ? i - g.ty : i + g.ty;
    sj = BWD ? j - g.tx : j + g.tx;
    return da_inside(si, sj, H, W) && !(BWD ? da_cut(g, si, sj) : da_cut(g, i, j));
}

// Steps 1 and 2 of the order above.  grid: n * slices workgroups, workgroup b * slices + slice.
template <int C, bool BWD>
__global__ __launch_bounds__(DA_NT) void diffaugment_reduce_kernel(const float* __restrict__ X, const float* __restrict__ U,
                                                                   double* __restrict__ partial, int H, int W, int policy) {
    __shared__ double red[DA_NT / 64];
    const int hw = H * W, slices = da_slices(hw), per = da_pixels_per_slice(hw);
    const int b = blockIdx.x / slices, slice = blockIdx.x - b * slices;
    const int lo = slice * per, hi = min(lo + per, hw);
    const Pixel<C>* __restrict__ xp = reinterpret_cast<const Pixel<C>*>(X) + (size_t)b * hw;
    Geometry g = {0, 0, 0, 0, 0, 0};
    if (BWD) g = da_geometry(U + (size_t)b * 8, H, W, policy);
    const int first = lo + (int)threadIdx.x;
    const int count = first < hi ? (hi - first + DA_NT - 1) / DA_NT : 0;
    double acc = igan::serial_sum_f64(0.0, 0, count, [&](int k) -> double {
        const int p = first + k * DA_NT;
        const Pixel<C> v = xp[p];
        double t = (double)v.v[0];
#pragma unroll
        for (int ch = 1; ch < C; ch++) t += (double)v.v[ch];
        if (BWD) {      // the sum of g runs over the positions of dy that reach an input pixel
            const int i = p / W, j = p - i * W;
            const bool kept = !da_cut(g, i, j) && da_inside(i + g.ty, j + g.tx, H, W);
            t = kept ? t : 0.0;
        }
        return t;
    });
    acc = igan::wave_sum_lane0(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// grid: n * ceil(H W / 256) workgroups; a workgroup stays inside one sample.
template <int C, bool BWD>
__global__ __launch_bounds__(DA_NT) void diffaugment_apply_kernel(const float* __restrict__ X, float* __restrict__ Y,
                                                                  const float* __restrict__ U, const double* __restrict__ partial,
                                                                  int H, int W, int policy, int blocks_per_sample) {
#pragma clang fp contract(off)
    const int hw = H * W;
    const int b = blockIdx.x / blocks_per_sample;
    const int p = (blockIdx.x - b * blocks_per_sample) * DA_NT + (int)threadIdx.x;
    if (p >= hw) return;
    const float* __restrict__ u = U + (size_t)b * 8;
    const Geometry g = da_geometry(u, H, W, policy);
    const int i = p / W, j = p - i * W;
    int si, sj;
    const bool kept = da_source<BWD>(g, i, j, H, W, si, sj);
    const Pixel<C>* __restrict__ xp = reinterpret_cast<const Pixel<C>*>(X) + (size_t)b * hw;
    Pixel<C>* __restrict__ yp = reinterpret_cast<Pixel<C>*>(Y) + (size_t)b * hw;
    Pixel<C> v;
#pragma unroll
    for (int ch = 0; ch < C; ch++) v.v[ch] = 0.0f;
    if (kept) v = xp[si * W + sj];
    if (policy & DA_COLOR) {
        const int slices = da_slices(hw);
        const double* __restrict__ part = partial + (size_t)b * slices;
        const double total = igan::serial_sum_f64(0.0, 0, slices, [&](int k) -> double { return part[k]; });
        const float mean = (float)(total / ((double)hw * (double)C));
        const float bri = u[0] - 0.5f, sat = 2.0f * u[1], con = u[2] + 0.5f;
        if (!BWD) {
            if (kept) {
                const float M = mean + bri;
                float xb[C];
                float sum = 0.0f;
#pragma unroll
                for (int ch = 0; ch < C; ch++) {
                    xb[ch] = v.v[ch] + bri;
                    sum = ch == 0 ? xb[0] : sum + xb[ch];
                }
                const float pm = sum / (float)C;
#pragma unroll
                for (int ch = 0; ch < C; ch++) v.v[ch] = ((xb[ch] - pm) * sat + pm - M) * con + M;
            }
        } else {
            float sum = v.v[0];
#pragma unroll
            for (int ch = 1; ch < C; ch++) sum += v.v[ch];
            const float q = sum / (float)C;
            const float a0 = con * sat, a1 = con * (1.0f - sat), a2 = (1.0f - con) * mean;
#pragma unroll
            for (int ch = 0; ch < C; ch++) v.v[ch] = a0 * v.v[ch] + a1 * q + a2;
        }
    }
    yp[p] = v;
}

template <int C, bool BWD>
int da_launch(hipStream_t stream, const float* x, float* y, const float* u, int n, int h, int w, int policy, double* partial) {
    const int hw = h * w;
    if (policy & DA_COLOR) {
        hipLaunchKernelGGL((diffaugment_reduce_kernel<C, BWD>), dim3((unsigned)(n * da_slices(hw))), dim3(DA_NT), 0, stream, x, u, partial, h, w, policy);
        IGAN_LAUNCH_CHECK("diffaugment reduce launch");
    }
    const int bps = igan::ceil_div(hw, DA_NT);
    hipLaunchKernelGGL((diffaugment_apply_kernel<C, BWD>), dim3((unsigned)((long long)n * bps)), dim3(DA_NT), 0, stream, x, y, u, partial, h, w, policy, bps);
    IGAN_LAUNCH_CHECK("diffaugment apply launch");
    return IGAN_OK;
}

bool da_supported(int n, int c, int h, int w) {
    return n >= 1 && c >= 1 && c <= 4 && h >= 1 && w >= 1 && (long long)n * c * h * w < (1LL << 31);
}

template <bool BWD>
int da_entry(const char* name, hipStream_t stream, const float* x, float* y, const float* u, int n, int c, int h, int w, int policy, void* workspace) {
    using namespace igan;
    IGAN_REQUIRE(x && y && u, "%s: null buffer", name);
    IGAN_REQUIRE(n >= 1 && c >= 1 && h >= 1 && w >= 1, "%s: n, c, h and w must be positive (got %d, %d, %d, %d)", name, n, c, h, w);
    IGAN_REQUIRE((policy & ~DA_ALL) == 0, "%s: unknown policy bits %d (1 = color, 2 = translation, 4 = cutout)", name, policy);
    IGAN_REQUIRE(!(policy & DA_COLOR) || workspace, "%s: the color policy needs a workspace of igan_diffaugment_workspace_bytes(n, c, h, w) bytes", name);
    IGAN_REQUIRE(x != y, "%s: the output must not be the input (a translated pixel is read from another position)", name);
    if (c > 4) return fail(IGAN_ERR_UNSUPPORTED, "%s: at most 4 channels (a thread moves a whole pixel; got %d)", name, c);
    if (!da_supported(n, c, h, w)) return fail(IGAN_ERR_UNSUPPORTED, "%s: n * c * h * w must stay below 2^31 (pass the batch in chunks)", name);
    const uintptr_t align = c == 4 ? 15 : (c == 2 ? 7 : 3);
    IGAN_REQUIRE(((((uintptr_t)x) | ((uintptr_t)y)) & align) == 0, "%s: x and y must be %d-byte aligned (a pixel of %d channels is one access)", name, (int)align + 1, c);
    IGAN_REQUIRE((((uintptr_t)u) & 3) == 0 && (((uintptr_t)workspace) & 7) == 0, "%s: u must be 4-byte and the workspace 8-byte aligned", name);
    double* partial = static_cast<double*>(workspace);
    switch (c) {
        case 1: return da_launch<1, BWD>(stream, x, y, u, n, h, w, policy, partial);
        case 2: return da_launch<2, BWD>(stream, x, y, u, n, h, w, policy, partial);
        case 3: return da_launch<3, BWD>(stream, x, y, u, n, h, w, policy, partial);
        default: return da_launch<4, BWD>(stream, x, y, u, n, h, w, policy, partial);
    }
}

}  // namespace

extern "C" size_t igan_diffaugment_workspace_bytes(int n, int c, int h, int w) {
    return da_supported(n, c, h, w) ? (size_t)n * da_slices(h * w) * sizeof(double) : 0;
}

extern "C" int igan_diffaugment_fwd(igan_stream_t stream, const float* x, float* y, const float* u, int n, int c, int h, int w, int policy,
                                    void* workspace) {
    return da_entry<false>("diffaugment_fwd", (hipStream_t)stream, x, y, u, n, c, h, w, policy, workspace);
}

extern "C" int igan_diffaugment_bwd(igan_stream_t stream, const float* dy, float* dx, const float* u, int n, int c, int h, int w, int policy,
                                    void* workspace) {
    return da_entry<true>("diffaugment_bwd", (hipStream_t)stream, dy, dx, u, n, c, h, w, policy, workspace);
}
