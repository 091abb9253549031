// Per-class statistics of classifier outputs for the Stacked-MNIST metrics (mode_counts_24k, KL24k) and the Inception Score
// (is50k) on gfx950.
//
// Behavioural contract: the reference copies every minibatch of logits / probabilities to the host and works there --
// np.argmax(logits, axis=1) into a label array that np.unique / np.histogram read (metrics/mode_counts.py:41-46,
// metrics/KL.py:41-49), and per split  part * (log(part) - log(mean(part, 0)))  summed over classes, averaged over images
// (metrics/inception_score.py:50-54).  Both are sums over rows, so here each minibatch is folded on the device:
//   counts[argmax_k X[i][k]] += 1                                                  (igan_class_hist_update)
//   psum[k] += sum_i (double)P[i][k]      plogp += sum_i sum_k (double)P[i][k] log((double)P[i][k])   (igan_prob_stats_update)
// and the few numbers a metric needs (K integers; K + 1 doubles per split) are the one device -> host copy.
// MI355X design:
//   rows       a wavefront owns a row.  Lane l holds columns 4 g .. 4 g + 3 for g = l, l + 64, ... and column 4 (K / 4) + l
//              of the K % 4 last ones -- an assignment by COLUMN INDEX, so what a lane sees (and the order of every sum) does
//              not depend on where the matrix lies.  A group is one 16-byte load declared 4-byte aligned: rows of an odd K
//              start anywhere, and the hardware's global loads need dword alignment only.
//   argmax     a lane walks its columns in ascending order under a STRICT comparison (a later equal value never wins, a NaN
//              beats every number and is beaten by nothing), then six xor steps reduce (value, index) lexicographically.
//              That order is total, so every lane ends with the same pair.
//   counts     integers: a workgroup (4 wavefronts x 4 rows) keeps its 16 labels in LDS, the first row of each distinct
//              label adds that label's multiplicity with ONE 64-bit integer vector atomic.  Integer sums do not depend on
//              order.  There is no floating-point atomic in this file.
//   psum       one thread owns a column and walks the n rows in order (workgroups 1 ..).
//   plogp      workgroup 0: lane sums in ascending column order, the xor tree over the lanes (fp addition commutes, so all
//              lanes agree), row sums parked in LDS, thread 0 adds them in row order and does the one read-modify-write.
//              One compute unit evaluates every logarithm of a call: the metrics call with 8 .. 32 rows of 1000 columns.
// The bits of psum / plogp are a function of (n, K) and the sequence of calls.
#include "igan_common.h"
#include "fixed_order_sum.h"
#include "class_argmax.h"      // cs_f4, cs_row_argmax: the row arg-max, shared with softmax_xent.hip

namespace {

constexpr int CS_NT = 256;
constexpr int CS_WAVES = CS_NT / 64;
constexpr int CS_HIST_ROWS = 16;       // rows per workgroup of the histogram kernel: 4 per wavefront
constexpr int CS_ROUND = 64;           // rows per round of the plogp workgroup: 16 per wavefront, one barrier pair per round
__global__ __launch_bounds__(CS_NT) void class_hist_kernel(const float* __restrict__ X, unsigned long long* __restrict__ counts,
                                                           int* __restrict__ labels, int n, int K) {
    __shared__ int lab[CS_HIST_ROWS];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    constexpr int per_wave = CS_HIST_ROWS / CS_WAVES;
    for (int r = 0; r < per_wave; r++) {
        const int slot = wave * per_wave + r;
        const long long row = (long long)blockIdx.x * CS_HIST_ROWS + slot;          // uniform per wavefront
        int best = -1;
        if (row < n) {
            best = cs_row_argmax(X + (size_t)row * K, K, lane);
            if (lane == 0 && labels) labels[row] = best;
        }
        if (lane == 0) lab[slot] = best;
    }
    __syncthreads();
    if (t < CS_HIST_ROWS) {
        const int mine = lab[t];
        if (mine >= 0) {
            bool first = true;
            unsigned long long same = 0;
            for (int j = 0; j < CS_HIST_ROWS; j++) {
                const bool eq = lab[j] == mine;
                if (eq && j < t) first = false;
                same += eq ? 1ull : 0ull;
            }
            if (first) atomicAdd(counts + mine, same);
        }
    }
}

__device__ inline double cs_plogp(float p) {
    const double d = (double)p;
    return d * log(d);
}

__global__ __launch_bounds__(CS_NT) void prob_stats_kernel(const float* __restrict__ P, double* __restrict__ psum,
                                                           double* __restrict__ plogp, int n, int K) {
    const int t = threadIdx.x;
    if (blockIdx.x > 0) {                                      // column owners
        const int c = (blockIdx.x - 1) * CS_NT + t;
        if (c >= K) return;
        double acc = 0.0;
#pragma unroll 8
        for (int i = 0; i < n; i++) acc += (double)P[(size_t)i * K + c];
        psum[c] += acc;
        return;
    }
    __shared__ double rowsum[CS_ROUND];
    const int wave = t >> 6, lane = t & 63;
    const int groups = K >> 2;
    double total = 0.0;                                        // thread 0's
    for (int r0 = 0; r0 < n; r0 += CS_ROUND) {
        for (int r = wave; r < CS_ROUND && r0 + r < n; r += CS_WAVES) {
            const float* row = P + (size_t)(r0 + r) * K;
            double s = 0.0;
            for (int g = lane; g < groups; g += 64) {
                const cs_f4 v = *reinterpret_cast<const cs_f4*>(row + 4 * g);
                s += cs_plogp(v.x);
                s += cs_plogp(v.y);
                s += cs_plogp(v.z);
                s += cs_plogp(v.w);
            }
            if (lane < (K & 3)) s += cs_plogp(row[4 * groups + lane]);
            s = igan::wave_sum(s);
            if (lane == 0) rowsum[r] = s;
        }
        __syncthreads();
        if (t == 0) {
            const int rows = (n - r0 < CS_ROUND) ? n - r0 : CS_ROUND;
            for (int r = 0; r < rows; r++) total += rowsum[r];
        }
        __syncthreads();                                       // the next round overwrites rowsum
    }
    if (t == 0) plogp[0] += total;
}

}  // namespace

extern "C" int igan_class_hist_update(igan_stream_t stream_, const float* logits, long long* counts, int* labels, int n, int K) {
    using namespace igan;
    IGAN_REQUIRE(logits && counts, "class_hist_update: null buffer");
    IGAN_REQUIRE(n >= 1, "class_hist_update: n must be positive");
    IGAN_REQUIRE(K >= 1, "class_hist_update: K must be positive");
    IGAN_REQUIRE((long long)n * K < (1LL << 29), "class_hist_update: logit matrix too large (2 GiB per call; pass it in chunks)");
    IGAN_REQUIRE((((uintptr_t)counts) & 7) == 0, "class_hist_update: counts must be 8-byte aligned");
    IGAN_REQUIRE((((uintptr_t)logits) & 3) == 0 && (((uintptr_t)labels) & 3) == 0, "class_hist_update: logits / labels must be 4-byte aligned");
    hipLaunchKernelGGL(class_hist_kernel, dim3(ceil_div(n, CS_HIST_ROWS)), dim3(CS_NT), 0, (hipStream_t)stream_, logits,
                       reinterpret_cast<unsigned long long*>(counts), labels, n, K);
    IGAN_LAUNCH_CHECK("class_hist_update launch");
    return IGAN_OK;
}

extern "C" int igan_prob_stats_update(igan_stream_t stream_, const float* probs, double* psum, double* plogp, int n, int K) {
    using namespace igan;
    IGAN_REQUIRE(probs && psum && plogp, "prob_stats_update: null buffer");
    IGAN_REQUIRE(n >= 1, "prob_stats_update: n must be positive");
    IGAN_REQUIRE(K >= 1, "prob_stats_update: K must be positive");
    IGAN_REQUIRE((long long)n * K < (1LL << 29), "prob_stats_update: probability matrix too large (2 GiB per call; pass it in chunks)");
    IGAN_REQUIRE(((((uintptr_t)psum) | ((uintptr_t)plogp)) & 7) == 0, "prob_stats_update: psum / plogp must be 8-byte aligned");
    IGAN_REQUIRE((((uintptr_t)probs) & 3) == 0, "prob_stats_update: probs must be 4-byte aligned");
    hipLaunchKernelGGL(prob_stats_kernel, dim3(1 + ceil_div(K, CS_NT)), dim3(CS_NT), 0, (hipStream_t)stream_, probs, psum, plogp, n, K);
    IGAN_LAUNCH_CHECK("prob_stats_update launch");
    return IGAN_OK;
}
