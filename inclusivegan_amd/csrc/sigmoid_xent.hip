// Sigmoid (binary) cross-entropy of classifier logits against {0, 1} targets on gfx950: the multi-label loss of the CelebA
// attribute classifier (train_classifier.py --mode attributes), forward, backward, the running per-attribute statistics of a
// trainer tick, and the probability pairs linear separability (metrics/linear_separability.py) takes from such a classifier.
//
// Behavioural contract: torch.nn.functional.binary_cross_entropy_with_logits(x, t, pos_weight=w, reduction='none') as fp64
// states it, with softplus(z) = max(z, 0) + log1p(exp(-|z|)) evaluated in fp64 from the fp32 logit (the max written as a
// comparison: a NaN logit fails it, and the NaN then arrives through exp) and each result rounded to fp32 once:
//   target == 1 (positive)   loss = (float)(w * softplus(-x))    dlogits = (float)(dloss * (-w / (1 + exp(x))))
//   target == 0 (negative)   loss = (float)(softplus(x))         dlogits = (float)(dloss * (1 / (1 + exp(-x))))
//   anything else (ignored)  loss = 0                            dlogits = 0            (NaN and the trainer's -1 included)
//   pred = x > 0 (a NaN predicts 0)
// The two gradient forms, not sigmoid(x) - t: a confident correct element has sigmoid(x) within a few ulp of t, and the
// difference would leave its small gradient with no correct digit; exp(x) of the right sign has them all.  x = +inf with a
// positive target is softplus(-inf) = 0 + log1p(0) = 0, not inf - inf.
//   probs[a][i] = ((float)(1 / (1 + exp(-2x))), (float)(1 / (1 + exp(2x))))      softmax of the pair (x, -x): mind the 2
// MI355X design:
//   forward, backward   one thread per element in row-major order: coalesced dword loads and stores (a byte store for pred), the
//              attribute index only where pos_weight is read.  Dense [n][A] needs 4-byte alignment only, so a row of an odd A
//              starts anywhere; no wider access is attempted -- an element costs an fp64 exp and an fp64 log1p (hundreds of
//              instructions), a [256, 40] call is 40 KB and one launch gap, and neither is bound by memory.
//   probabilities       one thread per OUTPUT pair in attribute-major order: the 8-byte stores are coalesced, the dword loads
//              stride by a row (the whole matrix sits in L2 at any minibatch the metric uses).
//   statistics one thread owns an attribute column and walks the rows in ascending order with one fp64 accumulator
//              (igan::serial_sum_f64) and four integer counts; adjacent threads read adjacent columns, so a wavefront's loads
//              of a row are one segment.  All three loads of an element are unconditional and the ignored rule is a select:
//              loads stay in flight across the unrolled rows.  No LDS, no atomic of any kind.
// A non-finite logit changes its own element only: nothing is shared between elements outside the statistics' column sums.
// The bits of every output are a function of (n, A), the data and the sequence of calls.
#include "igan_common.h"
#include "fixed_order_sum.h"

namespace {

constexpr int BX_NT = 256;
constexpr int BX_STATS_NT = 64;      // attribute columns per workgroup of the statistics kernel: one wavefront

enum { BX_IGNORED = 0, BX_NEGATIVE = 1, BX_POSITIVE = 2 };

__device__ inline int bx_kind(float t) { return t == 1.0f ? BX_POSITIVE : (t == 0.0f ? BX_NEGATIVE : BX_IGNORED); }

// max(z, 0) + log1p(exp(-|z|)); NaN > 0 is false and exp(-|NaN|) is NaN, so a NaN stays one; +inf gives +inf, -inf gives 0
__device__ inline double bx_softplus(double z) { return (z > 0.0 ? z : 0.0) + log1p(exp(-fabs(z))); }

__global__ __launch_bounds__(BX_NT) void sigmoid_xent_fwd_kernel(const float* __restrict__ X, const float* __restrict__ T,
                                                                 const float* __restrict__ pos_weight, float* __restrict__ loss,
                                                                 signed char* __restrict__ pred, int n, int A) {
    const unsigned e = blockIdx.x * BX_NT + threadIdx.x;       // n * A < 2^29 (validated): 32-bit indices and a 32-bit divide
    if (e >= (unsigned)n * (unsigned)A) return;
    const float xf = X[e];
    const int kind = bx_kind(T[e]);
    const double x = (double)xf;
    float l = 0.0f;
    if (kind == BX_POSITIVE) {
        const double w = pos_weight ? (double)pos_weight[e % (unsigned)A] : 1.0;
        l = (float)(w * bx_softplus(-x));
    } else if (kind == BX_NEGATIVE) {
        l = (float)bx_softplus(x);
    }
    loss[e] = l;
    if (pred) pred[e] = xf > 0.0f ? 1 : 0;
}

__global__ __launch_bounds__(BX_NT) void sigmoid_xent_bwd_kernel(const float* __restrict__ X, const float* __restrict__ T,
                                                                 const float* __restrict__ pos_weight, const float* __restrict__ dloss,
                                                                 float* __restrict__ dX, int n, int A) {
    const unsigned e = blockIdx.x * BX_NT + threadIdx.x;
    if (e >= (unsigned)n * (unsigned)A) return;
    const int kind = bx_kind(T[e]);
    const double x = (double)X[e];
    float d = 0.0f;
    if (kind == BX_POSITIVE) {
        const double w = pos_weight ? (double)pos_weight[e % (unsigned)A] : 1.0;
        d = (float)((double)dloss[e] * (-w / (1.0 + exp(x))));
    } else if (kind == BX_NEGATIVE) {
        d = (float)((double)dloss[e] * (1.0 / (1.0 + exp(-x))));
    }
    dX[e] = d;
}

__global__ __launch_bounds__(BX_STATS_NT) void sigmoid_xent_stats_kernel(const float* __restrict__ loss, const float* __restrict__ X,
                                                                         const float* __restrict__ T, double* __restrict__ loss_sum,
                                                                         long long* __restrict__ counts, int n, int A) {
    const int a = blockIdx.x * BX_STATS_NT + threadIdx.x;
    if (a >= A) return;
    int tp = 0, fp = 0, tn = 0, fn = 0;                        // n * A * 4 < 2 GiB: n fits an int
    loss_sum[a] = igan::serial_sum_f64(loss_sum[a], 0, n, [&](int r) -> double {
        const int e = r * A + a;
        const float l = loss[e], x = X[e];
        const int kind = bx_kind(T[e]);
        const bool p = x > 0.0f;
        tp += (kind == BX_POSITIVE && p) ? 1 : 0;
        fn += (kind == BX_POSITIVE && !p) ? 1 : 0;
        fp += (kind == BX_NEGATIVE && p) ? 1 : 0;
        tn += (kind == BX_NEGATIVE && !p) ? 1 : 0;
        return kind != BX_IGNORED ? (double)l : 0.0;           // a select, not a product: an ignored element's loss is never added
    });
    counts[4 * a + 0] += tp;
    counts[4 * a + 1] += fp;
    counts[4 * a + 2] += tn;
    counts[4 * a + 3] += fn;
}

__global__ __launch_bounds__(BX_NT) void binary_probs_kernel(const float* __restrict__ X, float2* __restrict__ probs, int n, int A) {
    const unsigned o = blockIdx.x * BX_NT + threadIdx.x;       // output pair a * n + i
    if (o >= (unsigned)n * (unsigned)A) return;
    const unsigned a = o / (unsigned)n, i = o - a * (unsigned)n;
    const double x2 = 2.0 * (double)X[i * (unsigned)A + a];    // exact
    probs[o] = make_float2((float)(1.0 / (1.0 + exp(-x2))), (float)(1.0 / (1.0 + exp(x2))));
}

}  // namespace

#define BX_REQUIRE_SHAPE(name)                                                                                              \
    IGAN_REQUIRE(n >= 1, name ": n must be positive");                                                                      \
    IGAN_REQUIRE(A >= 1, name ": A must be positive");                                                                      \
    IGAN_REQUIRE((long long)n * A < (1LL << 29), name ": logit matrix too large (2 GiB per call; pass it in chunks)")

extern "C" int igan_sigmoid_xent_fwd(igan_stream_t stream_, const float* logits, const float* targets, const float* pos_weight,
                                     float* loss, int8_t* pred, int n, int A) {
    using namespace igan;
    IGAN_REQUIRE(logits && targets && loss, "sigmoid_xent_fwd: null buffer");
    BX_REQUIRE_SHAPE("sigmoid_xent_fwd");
    IGAN_REQUIRE(((((uintptr_t)logits) | ((uintptr_t)targets) | ((uintptr_t)pos_weight) | ((uintptr_t)loss)) & 3) == 0,
                 "sigmoid_xent_fwd: logits / targets / pos_weight / loss must be 4-byte aligned");
    const long long total = (long long)n * A;
    hipLaunchKernelGGL(sigmoid_xent_fwd_kernel, dim3((unsigned)ceil_div_ll(total, BX_NT)), dim3(BX_NT), 0, (hipStream_t)stream_,
                       logits, targets, pos_weight, loss, reinterpret_cast<signed char*>(pred), n, A);
    IGAN_LAUNCH_CHECK("sigmoid_xent_fwd launch");
    return IGAN_OK;
}

extern "C" int igan_sigmoid_xent_bwd(igan_stream_t stream_, const float* logits, const float* targets, const float* pos_weight,
                                     const float* dloss, float* dlogits, int n, int A) {
    using namespace igan;
    IGAN_REQUIRE(logits && targets && dloss && dlogits, "sigmoid_xent_bwd: null buffer");
    BX_REQUIRE_SHAPE("sigmoid_xent_bwd");
    IGAN_REQUIRE(((((uintptr_t)logits) | ((uintptr_t)targets) | ((uintptr_t)pos_weight) | ((uintptr_t)dloss) | ((uintptr_t)dlogits)) & 3) == 0,
                 "sigmoid_xent_bwd: logits / targets / pos_weight / dloss / dlogits must be 4-byte aligned");
    const long long total = (long long)n * A;
    hipLaunchKernelGGL(sigmoid_xent_bwd_kernel, dim3((unsigned)ceil_div_ll(total, BX_NT)), dim3(BX_NT), 0, (hipStream_t)stream_,
                       logits, targets, pos_weight, dloss, dlogits, n, A);
    IGAN_LAUNCH_CHECK("sigmoid_xent_bwd launch");
    return IGAN_OK;
}

extern "C" int igan_sigmoid_xent_stats_update(igan_stream_t stream_, const float* loss, const float* logits, const float* targets,
                                              double* loss_sum, long long* counts, int n, int A) {
    using namespace igan;
    IGAN_REQUIRE(loss && logits && targets && loss_sum && counts, "sigmoid_xent_stats_update: null buffer");
    BX_REQUIRE_SHAPE("sigmoid_xent_stats_update");
    IGAN_REQUIRE(((((uintptr_t)loss_sum) | ((uintptr_t)counts)) & 7) == 0, "sigmoid_xent_stats_update: loss_sum / counts must be 8-byte aligned");
    IGAN_REQUIRE(((((uintptr_t)loss) | ((uintptr_t)logits) | ((uintptr_t)targets)) & 3) == 0,
                 "sigmoid_xent_stats_update: loss / logits / targets must be 4-byte aligned");
    hipLaunchKernelGGL(sigmoid_xent_stats_kernel, dim3(ceil_div(A, BX_STATS_NT)), dim3(BX_STATS_NT), 0, (hipStream_t)stream_, loss, logits,
                       targets, loss_sum, counts, n, A);
    IGAN_LAUNCH_CHECK("sigmoid_xent_stats_update launch");
    return IGAN_OK;
}

extern "C" int igan_binary_probs(igan_stream_t stream_, const float* logits, float* probs, int n, int A) {
    using namespace igan;
    IGAN_REQUIRE(logits && probs, "binary_probs: null buffer");
    BX_REQUIRE_SHAPE("binary_probs");
    IGAN_REQUIRE((((uintptr_t)probs) & 7) == 0, "binary_probs: probs must be 8-byte aligned");
    IGAN_REQUIRE((((uintptr_t)logits) & 3) == 0, "binary_probs: logits must be 4-byte aligned");
    const long long total = (long long)n * A;
    hipLaunchKernelGGL(binary_probs_kernel, dim3((unsigned)ceil_div_ll(total, BX_NT)), dim3(BX_NT), 0, (hipStream_t)stream_, logits,
                       reinterpret_cast<float2*>(probs), n, A);
    IGAN_LAUNCH_CHECK("binary_probs launch");
    return IGAN_OK;
}
