// Softmax cross-entropy of classifier logits against integer labels on gfx950: the loss of the Stacked-MNIST mode classifier
// (training/networks_classifier.py, train_classifier.py), forward, backward and the running statistics of a trainer tick.
//
// Behavioural contract: torch.nn.functional.cross_entropy(logits, labels, reduction='none') as fp64 states it,
//   lse_i     = m_i + log sum_k exp((double)x_ik - m_i),  m_i the row maximum        (fp64, stored as fp64; evaluated as
//               m_i + log1p(sum over k != argmax of exp(x_ik - m_i)): the arg-max column's term is exactly 1, and log of a
//               sum rounded next to 1 would lose the digits of a confident row's lse)
//   loss_i    = (float)(lse_i - x_i,label)
//   dlogits_ik = (float)(dloss_i * (exp((double)x_ik - lse_i) - [k == label_i]))      (the difference in fp64 -- expm1 at the
//                                                                                       label's column -- rounded once)
// with rows whose label lies outside [0, K) ignored (loss 0, gradient row 0, nothing read at the label's column), and
// pred_i = np.argmax(x_i) under the rules of igan_class_hist_update (class_argmax.h).
// MI355X design:
//   forward    a wavefront owns a row, lanes own columns by index as in class_stats.hip (class_argmax.h).  The arg-max pass
//              gives pred and with it the maximum m = x[pred]; the second pass over the row (L1 / L2 hits: a row of 1000
//              columns is 4 KB) sums exp(x - m) over the other columns per lane in ascending column order and over the lanes in the xor tree (fp
//              addition commutes, so all lanes agree).  No LDS: at K = 10 a row is a quarter of one load, at K = 1000 four
//              16-byte loads per lane, and nothing is shared between rows.
//   non-finite m is NaN for a row that holds a NaN (the arg-max picks it), +inf for a row that holds +inf, -inf for a row of
//              -inf: x - m is then NaN at the arg-max column, whose term is x - m itself, the sum is NaN and so are lse, loss and the gradient row.  A -inf
//              among finite logits gives exp(-inf) = 0 exactly.  Rows never mix.
//   backward   one thread per element: the row's lse, label and dloss are three broadcast loads, the probability is
//              re-derived from the stored fp64 lse.  Loads and stores are coalesced dwords.
//   statistics one workgroup: a round parks 256 rows' losses in LDS, thread 0 adds them in row order into fp64; the two
//              integer counts are summed over the workgroup (order-free) and added by thread 0.  No atomic of any kind.
// The bits of every output are a function of (n, K), the data and the sequence of calls.
#include "igan_common.h"
#include "fixed_order_sum.h"
#include "class_argmax.h"

namespace {

constexpr int SX_NT = 256;
constexpr int SX_WAVES = SX_NT / 64;          // rows per workgroup of the forward kernel: one per wavefront

// a column's term of the sum behind log1p: exp(x - m), and for the arg-max column -- whose exp(0) is the 1 of log1p -- x - m
// itself: an exact 0 for a finite maximum, NaN for a maximum of +-inf or NaN, which is what makes such a row NaN
__device__ inline double sx_term(float x, double m, bool is_best) {
    const double a = (double)x - m;
    return is_best ? a : exp(a);
}

__global__ __launch_bounds__(SX_NT) void softmax_xent_fwd_kernel(const float* __restrict__ X, const int* __restrict__ labels,
                                                                 float* __restrict__ loss, double* __restrict__ lse,
                                                                 int* __restrict__ pred, int n, int K) {
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const long long r = (long long)blockIdx.x * SX_WAVES + wave;                  // uniform per wavefront
    if (r >= n) return;
    const float* row = X + (size_t)r * K;
    const int best = cs_row_argmax(row, K, lane);
    const double m = (double)row[best];
    const int groups = K >> 2;
    double s = 0.0;                                                                 // sum over k != best of exp(x_k - m)
    for (int g = lane; g < groups; g += 64) {
        const cs_f4 v = *reinterpret_cast<const cs_f4*>(row + 4 * g);
        s += sx_term(v.x, m, 4 * g == best);
        s += sx_term(v.y, m, 4 * g + 1 == best);
        s += sx_term(v.z, m, 4 * g + 2 == best);
        s += sx_term(v.w, m, 4 * g + 3 == best);
    }
    if (lane < (K & 3)) s += sx_term(row[4 * groups + lane], m, 4 * groups + lane == best);
    s = igan::wave_sum(s);
    if (lane == 0) {
        const double l = m + log1p(s);
        const int lab = labels[r];
        lse[r] = l;
        loss[r] = (lab >= 0 && lab < K) ? (float)(l - (double)row[lab]) : 0.0f;
        if (pred) pred[r] = best;
    }
}

__global__ __launch_bounds__(SX_NT) void softmax_xent_bwd_kernel(const float* __restrict__ X, const int* __restrict__ labels,
                                                                 const double* __restrict__ lse, const float* __restrict__ dloss,
                                                                 float* __restrict__ dX, int n, int K) {
    const unsigned e = blockIdx.x * SX_NT + threadIdx.x;       // n * K < 2^29 (validated): 32-bit indices and a 32-bit divide
    if (e >= (unsigned)n * (unsigned)K) return;
    const int r = (int)(e / (unsigned)K), k = (int)(e - (unsigned)r * (unsigned)K);
    const int lab = labels[r];
    float d = 0.0f;
    if (lab >= 0 && lab < K) {
        // at the label's column p - 1 is expm1: a confident row has p within a few ulp of 1, and exp() - 1.0 would leave
        // the gradient of exactly that column with no correct digit
        const double a = (double)X[e] - lse[r];
        d = (float)((double)dloss[r] * (k == lab ? expm1(a) : exp(a)));
    }
    dX[e] = d;
}

__global__ __launch_bounds__(SX_NT) void xent_stats_kernel(const float* __restrict__ loss, const int* __restrict__ labels,
                                                           const int* __restrict__ pred, double* __restrict__ loss_sum,
                                                           long long* __restrict__ counts, int n, int K) {
    __shared__ float park[SX_NT];             // an ignored row parks +0.0f: x + 0.0 == x for every x a sum of losses can hold
    __shared__ int wsum[2][SX_WAVES];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    double total = 0.0;                       // thread 0's
    int counted = 0, correct = 0;             // n * K * 4 < 2 GiB: n fits an int
    for (int r0 = 0; r0 < n; r0 += SX_NT) {
        const int r = r0 + t;
        float v = 0.0f;
        if (r < n) {
            const int lab = labels[r];
            if (lab >= 0 && lab < K) {
                v = loss[r];
                counted += 1;
                correct += pred[r] == lab ? 1 : 0;
            }
        }
        park[t] = v;
        __syncthreads();
        if (t == 0) {
            const int rows = (n - r0 < SX_NT) ? n - r0 : SX_NT;
            for (int i = 0; i < rows; i++) total += (double)park[i];
        }
        __syncthreads();                      // the next round overwrites park
    }
    counted = igan::wave_sum(counted);
    correct = igan::wave_sum(correct);
    if (lane == 0) {
        wsum[0][wave] = counted;
        wsum[1][wave] = correct;
    }
    __syncthreads();
    if (t == 0) {
        long long c0 = 0, c1 = 0;
        for (int w = 0; w < SX_WAVES; w++) {
            c0 += wsum[0][w];
            c1 += wsum[1][w];
        }
        loss_sum[0] += total;
        counts[0] += c0;
        counts[1] += c1;
    }
}

}  // namespace

extern "C" int igan_softmax_xent_fwd(igan_stream_t stream_, const float* logits, const int* labels, float* loss, double* lse,
                                     int* pred, int n, int K) {
    using namespace igan;
    IGAN_REQUIRE(logits && labels && loss && lse, "softmax_xent_fwd: null buffer");
    IGAN_REQUIRE(n >= 1, "softmax_xent_fwd: n must be positive");
    IGAN_REQUIRE(K >= 1, "softmax_xent_fwd: K must be positive");
    IGAN_REQUIRE((long long)n * K < (1LL << 29), "softmax_xent_fwd: logit matrix too large (2 GiB per call; pass it in chunks)");
    IGAN_REQUIRE((((uintptr_t)lse) & 7) == 0, "softmax_xent_fwd: lse must be 8-byte aligned");
    IGAN_REQUIRE(((((uintptr_t)logits) | ((uintptr_t)labels) | ((uintptr_t)loss) | ((uintptr_t)pred)) & 3) == 0,
                 "softmax_xent_fwd: logits / labels / loss / pred must be 4-byte aligned");
    hipLaunchKernelGGL(softmax_xent_fwd_kernel, dim3(ceil_div(n, SX_WAVES)), dim3(SX_NT), 0, (hipStream_t)stream_, logits, labels,
                       loss, lse, pred, n, K);
    IGAN_LAUNCH_CHECK("softmax_xent_fwd launch");
    return IGAN_OK;
}

extern "C" int igan_softmax_xent_bwd(igan_stream_t stream_, const float* logits, const int* labels, const double* lse,
                                     const float* dloss, float* dlogits, int n, int K) {
    using namespace igan;
    IGAN_REQUIRE(logits && labels && lse && dloss && dlogits, "softmax_xent_bwd: null buffer");
    IGAN_REQUIRE(n >= 1, "softmax_xent_bwd: n must be positive");
    IGAN_REQUIRE(K >= 1, "softmax_xent_bwd: K must be positive");
    IGAN_REQUIRE((long long)n * K < (1LL << 29), "softmax_xent_bwd: logit matrix too large (2 GiB per call; pass it in chunks)");
    IGAN_REQUIRE((((uintptr_t)lse) & 7) == 0, "softmax_xent_bwd: lse must be 8-byte aligned");
    IGAN_REQUIRE(((((uintptr_t)logits) | ((uintptr_t)labels) | ((uintptr_t)dloss) | ((uintptr_t)dlogits)) & 3) == 0,
                 "softmax_xent_bwd: logits / labels / dloss / dlogits must be 4-byte aligned");
    const long long total = (long long)n * K;
    hipLaunchKernelGGL(softmax_xent_bwd_kernel, dim3((unsigned)ceil_div_ll(total, SX_NT)), dim3(SX_NT), 0, (hipStream_t)stream_,
                       logits, labels, lse, dloss, dlogits, n, K);
    IGAN_LAUNCH_CHECK("softmax_xent_bwd launch");
    return IGAN_OK;
}

extern "C" int igan_xent_stats_update(igan_stream_t stream_, const float* loss, const int* labels, const int* pred,
                                      double* loss_sum, long long* counts, int n, int K) {
    using namespace igan;
    IGAN_REQUIRE(loss && labels && pred && loss_sum && counts, "xent_stats_update: null buffer");
    IGAN_REQUIRE(n >= 1, "xent_stats_update: n must be positive");
    IGAN_REQUIRE(K >= 1, "xent_stats_update: K must be positive");
    IGAN_REQUIRE((long long)n * K < (1LL << 29), "xent_stats_update: logit matrix too large (2 GiB per call; pass it in chunks)");
    IGAN_REQUIRE(((((uintptr_t)loss_sum) | ((uintptr_t)counts)) & 7) == 0, "xent_stats_update: loss_sum / counts must be 8-byte aligned");
    IGAN_REQUIRE(((((uintptr_t)loss) | ((uintptr_t)labels) | ((uintptr_t)pred)) & 3) == 0,
                 "xent_stats_update: loss / labels / pred must be 4-byte aligned");
    hipLaunchKernelGGL(xent_stats_kernel, dim3(1), dim3(SX_NT), 0, (hipStream_t)stream_, loss, labels, pred, loss_sum, counts, n, K);
    IGAN_LAUNCH_CHECK("xent_stats_update launch");
    return IGAN_OK;
}
