// The exact streaming nearest-neighbour searches on gfx950: no index, candidate batches are generated, folded and discarded.
//
// Behavioural contracts:
//   nn1         the reference builds a Prioritized-DCI index over the generated candidates and asks for ONE neighbour per real
//               image (training/training_loop.py:367-368,398; dci_code/src/dci.c:108-337,788-828) with Euclidean distances
//               (dci_code/src/util.c:62-69).  DCI is approximate and seeded from time(NULL) (dci.c:77,860); what the training
//               loop consumes is the arg-min candidate per real and its distance.
//   nnk         with `exclusive_retrieved_code` it asks for num_samples_factor neighbours (training_loop.py:382-396,
//               dci_query(num_neighbours = k)) and picks greedily among them: per real, the k nearest candidates in ascending
//               order with their distances.
//   knn_radius, manifold_member
//               the reference estimates a manifold as one hypersphere per point, its radius the distance to the point's k-th
//               neighbour (metrics/precision_recall.py:73-90: np.partition of a [10 000 x n] fp16 distance block on the
//               host), and calls a sample "in" when it lies within the radius of any point (:119-120, `<=`).
//   ball_count  no counterpart in the reference: density and coverage (Naeem et al., ICML 2020; the `prdc` package) count, per
//               real, the fakes strictly inside the real's own k-NN ball (`<`, where pr50k3 has `<=`).
// MI355X design: |q - c|^2 = |q|^2 + |c|^2 - 2 q.c, so a batch of candidates is one [nq x dim] x [dim x nc] product on the
// exact-fp32 MFMA (distance_products(): the implicit-GEMM kernel of conv2d as a 1x1 conv, both operands in their natural
// row-major [rows][dim] layout), followed by a fold with one wavefront per query.  The product only SCREENS; the procedure
// around it -- interval, contenders, exact fp64 measurement -- is exact_search.h, and a kernel here is its state, its insert
// rule and its radius test.  Every state is a function of the SET of (row, index) pairs fed -- not of the order or the
// boundaries of the batches, bits of the distances included -- so the reference's 118 GB fp64 host array
// (training_loop.py:358) never exists.
//   nn1_fold             ONE (distance, index) pair per query
//   nnk_fold             the k lexicographically smallest (distance, index) pairs
//   knn_radius_fold      the kcap smallest exact distances (a MULTISET of values: duplicates count, so the value at position k
//                        is what np.partition leaves there)
//   manifold_member_fold an any-within-radius reduction against per-candidate radii
//   ball_count_fold      an integer count of the candidates within per-QUERY radii
#include "igan_common.h"
#include "exact_search.h"

#include <cmath>
#include <type_traits>

namespace {

using namespace igan;

__global__ __launch_bounds__(256) void row_sqnorm_kernel(const float* a, float* out, int rows, int dim) {
    // one wavefront per row, fp64 accumulation
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (wave >= rows) return;
    const float* p = a + (size_t)wave * dim;
    double s = 0.0;
    for (int i = lane; i < dim; i += 64) {
        const double v = (double)p[i];
        s += v * v;
    }
    s = wave_sum_lane0(s);
    if (lane == 0) out[wave] = (float)s;
}

// A candidate stays a contender while its interval reaches below the best upper bound known (the running exact minimum, or
// the smallest a + t of this batch); the choice is made on (exact distance, index) -- lexicographic, ties to the lower
// index, exactly what an fp64 brute-force search returns (oracle/nn.py; the reference's dci_query(num_neighbours=1)
// approximates it).  A non-finite dot product or distance compares false everywhere: such a candidate can never win
// (contends_if_decided).
__global__ __launch_bounds__(256) void nn1_fold_kernel(const float* __restrict__ dots, const float* __restrict__ qnorm,
                                                       const float* __restrict__ cnorm, const float* __restrict__ query,
                                                       const float* __restrict__ cand, double* __restrict__ best_d2,
                                                       int* __restrict__ best_idx, int nq, int nc, int dim, int idx_base) {
    const int q = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (q >= nq) return;
    const Screen s{dots + (size_t)q * nc, cnorm, (double)qnorm[q], nn1_tol(dim)};
    double bd = best_d2[q];
    int bi = best_idx[q];
    // pass 1: smallest upper bound of this batch
    double u = bd;
    for (int c = lane; c < nc; c += 64) {
        const double hi = s(c).hi;
        u = (hi < u) ? hi : u;
    }
    u = wave_min(u);
    // pass 2: exact evaluation of the contenders, in index order
    const float* qrow = query + (size_t)q * dim;
    for (int c0 = 0; c0 < nc; c0 += 64) {
        const int c = c0 + lane;
        int j;
        for (ContenderStrip strip(c < nc && contends_if_decided(s(c).lo, u)); strip.next(j);) {
            const double e = wave_sqdist(qrow, cand + (size_t)(c0 + j) * dim, dim, lane);
            const int gi = idx_base + c0 + j;
            if (e < bd || (e == bd && gi < bi)) { bd = e; bi = gi; }
            u = (e < u) ? e : u;
        }
    }
    if (lane == 0) { best_d2[q] = bd; best_idx[q] = bi; }
}

// sorted_insert carrying the index: (v, vi) goes into the list ascending by (distance, index), the largest pair drops out.
// Static indices only: both lists stay in registers.
template <int KC>
__device__ __forceinline__ void pair_insert(double (&d)[KC], int (&x)[KC], double v, int vi) {
#pragma unroll
    for (int i = 0; i < KC; i++) {
        const bool first = (v < d[i]) || (v == d[i] && vi < x[i]);
        const double dl = first ? v : d[i];
        const int xl = first ? vi : x[i];
        v = first ? d[i] : v;
        vi = first ? x[i] : vi;
        d[i] = dl;
        x[i] = xl;
    }
}

// KC >= k is the compiled list length.
//   pass 1  U = the k-th smallest upper bound over this batch and the running state (kth_upper_bound).
//   pass 2  in index order: a candidate whose LOWER bound a - t exceeds U cannot be among the k smallest pairs (equality
//           stays in: a candidate that ties the k-th distance with a lower index displaces it); every other one is measured
//           exactly and inserted when (e, index) < the k-th pair; U follows the running k-th exact distance down.
// A NaN bound decides nothing (contends_unless_ruled_out); a non-finite exact distance never enters.
template <int KC>
__global__ __launch_bounds__(256) void nnk_fold_kernel(const float* __restrict__ dots, const float* __restrict__ qnorm,
                                                       const float* __restrict__ cnorm, const float* __restrict__ query,
                                                       const float* __restrict__ cand, double* __restrict__ best_d2,
                                                       int* __restrict__ best_idx, int nq, int nc, int dim, int k, int idx_base) {
    const int q = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (q >= nq) return;
    const double inf = (double)INFINITY;
    const Screen s{dots + (size_t)q * nc, cnorm, (double)qnorm[q], nn1_tol(dim)};
    // pass 1 (lane 0's list starts as the state's distances; the state itself is read after this pass, which keeps the
    // wave-uniform copy out of the scalar registers while the bound lists are live)
    double l[KC];
#pragma unroll
    for (int i = 0; i < KC; i++) {
        double v = inf;
        if (lane == 0 && i < k) v = best_d2[(size_t)q * k + i];
        l[i] = (v < inf) ? v : inf;
    }
    double u = kth_upper_bound<KC>(s, nc, l, k, lane);
    // pass 2
    // The k pairs sit RIGHT-aligned in the KC slots, behind KC - k sentinels (-inf, INT32_MIN) that nothing displaces: the k-th
    // pair is always slot KC - 1, a static index.
    const int pad = KC - k;
    double sd[KC];
    int si[KC];
#pragma unroll
    for (int i = 0; i < KC; i++) {
        const int slot = (i >= pad) ? i - pad : 0;          // always a valid slot: the loads need no branch
        const double v = best_d2[(size_t)q * k + slot];
        const int vi = best_idx[(size_t)q * k + slot];
        sd[i] = (i >= pad) ? ((v < inf) ? v : inf) : -inf;
        si[i] = (i >= pad) ? ((v < inf) ? vi : INT32_MAX) : INT32_MIN;
    }
    const float* qrow = query + (size_t)q * dim;
    for (int c0 = 0; c0 < nc; c0 += 64) {
        const int c = c0 + lane;
        int j;
        for (ContenderStrip strip(c < nc && contends_unless_ruled_out(s(c).lo, u)); strip.next(j);) {
            const double e = wave_sqdist(qrow, cand + (size_t)(c0 + j) * dim, dim, lane);
            const int gi = idx_base + c0 + j;
            if (e < inf && (e < sd[KC - 1] || (e == sd[KC - 1] && gi < si[KC - 1]))) {      // false for NaN and +inf
                pair_insert<KC>(sd, si, e, gi);
                u = (sd[KC - 1] < u) ? sd[KC - 1] : u;
            }
        }
    }
    // lane i writes slot i: one store per list instead of KC guarded ones
    double od = inf;
    int oi = INT32_MAX;
#pragma unroll
    for (int i = 0; i < KC; i++) {
        od = (lane == i) ? sd[i] : od;
        oi = (lane == i) ? si[i] : oi;
    }
    if (lane >= pad && lane < KC) {
        best_d2[(size_t)q * k + (lane - pad)] = od;
        best_idx[(size_t)q * k + (lane - pad)] = oi;
    }
}

// KC >= kcap is the compiled list length; the list is LEFT-aligned, its kcap-th value at the dynamic position kcap - 1.
//   pass 1  U = the kcap-th smallest upper bound over this batch and the running state (kth_upper_bound).
//   pass 2  a candidate whose LOWER bound a - t exceeds U cannot be among the kcap smallest; every other one is measured
//           exactly and inserted; U follows the running exact value at position kcap - 1 down.
// A non-finite bound decides nothing (contends_unless_ruled_out); a non-finite exact distance counts as +inf.
template <int KC>
__global__ __launch_bounds__(256) void knn_radius_fold_kernel(const float* __restrict__ dots, const float* __restrict__ qnorm,
                                                              const float* __restrict__ cnorm, const float* __restrict__ query,
                                                              const float* __restrict__ cand, double* __restrict__ kth_d2,
                                                              int nq, int nc, int dim, int kcap) {
    const int q = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (q >= nq) return;
    const double inf = (double)INFINITY;
    const Screen s{dots + (size_t)q * nc, cnorm, (double)qnorm[q], nn1_tol(dim)};
    double st[KC], l[KC];
#pragma unroll
    for (int i = 0; i < KC; i++) {
        const double v = (i < kcap) ? kth_d2[(size_t)q * kcap + i] : inf;
        st[i] = (v < inf) ? v : inf;
        l[i] = (lane == 0) ? st[i] : inf;
    }
    double u = kth_upper_bound<KC>(s, nc, l, kcap, lane);
    const float* qrow = query + (size_t)q * dim;
    for (int c0 = 0; c0 < nc; c0 += 64) {
        const int c = c0 + lane;
        int j;
        for (ContenderStrip strip(c < nc && contends_unless_ruled_out(s(c).lo, u)); strip.next(j);) {
            const double e = wave_sqdist(qrow, cand + (size_t)(c0 + j) * dim, dim, lane);
            if (e < st[KC - 1]) {                              // false for NaN and +inf: neither can move a finite entry
                sorted_insert<KC>(st, e);
                double b = inf;
#pragma unroll
                for (int i = 0; i < KC; i++) b = (i == kcap - 1) ? st[i] : b;
                u = (b < u) ? b : u;
            }
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < KC; i++)
            if (i < kcap) kth_d2[(size_t)q * kcap + i] = st[i];
    }
}

// Bit s of `in` is member[q][s].  For a pair (q, c) and column s with radius R = cand_radius[c][s]:
//   a + t <= R (and finite)  definitely inside;   a - t > R  definitely outside;   otherwise the exact distance decides
//   (isfinite(e) && e <= R, the reference's `<=` at precision_recall.py:119).
// A NaN anywhere fails the first two tests (contends_unless_ruled_out) and the exact one: such a pair is never a witness.
// A strip is skipped once every column is set, and a contender is measured only for the columns still open when it comes up.
__global__ __launch_bounds__(256) void manifold_member_fold_kernel(const float* __restrict__ dots, const float* __restrict__ qnorm,
                                                                   const float* __restrict__ cnorm, const float* __restrict__ query,
                                                                   const float* __restrict__ cand, const double* __restrict__ cand_radius,
                                                                   int* __restrict__ member, int nq, int nc, int dim, int nk) {
    const int q = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (q >= nq) return;
    const double inf = (double)INFINITY;
    const unsigned full = (1u << nk) - 1u;
    unsigned in = 0;
    for (int s = 0; s < nk; s++)
        if (member[(size_t)q * nk + s] != 0) in |= 1u << s;
    if (in == full) return;
    const Screen screen{dots + (size_t)q * nc, cnorm, (double)qnorm[q], nn1_tol(dim)};
    const float* qrow = query + (size_t)q * dim;
    for (int c0 = 0; c0 < nc && in != full; c0 += 64) {
        const int c = c0 + lane;
        unsigned sure = 0, need = 0;
        if (c < nc) {
            const Interval iv = screen(c);
            for (int s = 0; s < nk; s++) {
                const double R = cand_radius[(size_t)c * nk + s];
                if (iv.hi < inf && iv.hi <= R) sure |= 1u << s;
                else if (contends_unless_ruled_out(iv.lo, R)) need |= 1u << s;
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) sure |= __shfl_xor(sure, off, 64);
        in |= sure;
        if (in == full) break;
        int j;
        for (ContenderStrip strip((need & ~in) != 0u); strip.next(j);) {
            const unsigned todo = (unsigned)__shfl((int)need, j, 64) & ~in;
            if (todo == 0u) continue;
            const double e = wave_sqdist(qrow, cand + (size_t)(c0 + j) * dim, dim, lane);
            if (e < inf) {
                for (int s = 0; s < nk; s++)
                    if (((todo >> s) & 1u) && e <= cand_radius[(size_t)(c0 + j) * nk + s]) in |= 1u << s;
            }
            if (in == full) break;
        }
    }
    if (lane == 0) {
        for (int s = 0; s < nk; s++)
            if ((in >> s) & 1u) member[(size_t)q * nk + s] = 1;
    }
}

// The radius test of the ball count: strict (prdc's `<`) or inclusive (the `<=` of the membership test).
template <bool INCLUSIVE>
__device__ __forceinline__ bool within(double d, double R) { return INCLUSIVE ? d <= R : d < R; }

// count[q][s] += #{c of the batch : d2(q, c) within R = query_radius[q][s]} -- the radii belong to the QUERIES, so R is
// wave-uniform.  For a pair (q, c) and column s:
//   a + t within R (and finite)  surely inside: counted in a lane-local integer, never measured;
//   a - t beyond R               ruled out (strict: a - t >= R; inclusive: a - t > R);
//   otherwise a contender: measured once for all of its open columns, counted in a wave-uniform integer when the exact
//   distance is finite and within R.
// The contender test is the NEGATION of "ruled out", so a NaN interval or a NaN radius falls through to measurement
// (contends_unless_ruled_out) and the exact test then fails for a NaN.  There is no early exit -- every strip is screened --
// no atomic and no floating-point sum: the state is a function of the multiset of (query, candidate) pairs fed.
// The per-column counters sit under static indices (unrolled to 8, guarded by s < nk): registers, not scratch.
template <bool INCLUSIVE>
__global__ __launch_bounds__(256) void ball_count_fold_kernel(const float* __restrict__ dots, const float* __restrict__ qnorm,
                                                              const float* __restrict__ cnorm, const float* __restrict__ query,
                                                              const float* __restrict__ cand, const double* __restrict__ query_radius,
                                                              long long* __restrict__ count, int nq, int nc, int dim, int nk) {
    // q by readfirstlane: the compiler then knows the radii, the row pointers and the query's norm to be wave-uniform and keeps
    // them in scalar registers (104 VGPRs without it, 4 waves per SIMD)
    const int q = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    const int lane = threadIdx.x & 63;
    if (q >= nq) return;
    const double inf = (double)INFINITY;
    double R[8];
    int sure[8], measured[8];       // lane-local / wave-uniform; a batch has fewer than 2^31 candidates
#pragma unroll
    for (int s = 0; s < 8; s++) {
        R[s] = (s < nk) ? query_radius[(size_t)q * nk + s] : 0.0;
        sure[s] = 0;
        measured[s] = 0;
    }
    const Screen screen{dots + (size_t)q * nc, cnorm, (double)qnorm[q], nn1_tol(dim)};
    const float* qrow = query + (size_t)q * dim;
    for (int c0 = 0; c0 < nc; c0 += 64) {
        const int c = c0 + lane;
        unsigned need = 0;
        if (c < nc) {
            const Interval iv = screen(c);
#pragma unroll
            for (int s = 0; s < 8; s++) {
                if (s < nk) {
                    const bool inside = iv.hi < inf && within<INCLUSIVE>(iv.hi, R[s]);
                    const bool contends = INCLUSIVE ? contends_unless_ruled_out(iv.lo, R[s]) : !(iv.lo >= R[s]);
                    sure[s] += inside ? 1 : 0;
                    need |= (!inside && contends) ? 1u << s : 0u;
                }
            }
        }
        int j;
        for (ContenderStrip strip(need != 0u); strip.next(j);) {
            const unsigned todo = (unsigned)__shfl((int)need, j, 64);
            const double e = wave_sqdist(qrow, cand + (size_t)(c0 + j) * dim, dim, lane);
            if (e < inf) {                                     // false for NaN and +inf: never counted
#pragma unroll
                for (int s = 0; s < 8; s++)
                    if (s < nk) measured[s] += (((todo >> s) & 1u) && within<INCLUSIVE>(e, R[s])) ? 1 : 0;
            }
        }
    }
#pragma unroll
    for (int s = 0; s < 8; s++) {
        if (s < nk) {
            int n = sure[s];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off, 64);
            if (lane == 0) count[(size_t)q * nk + s] += (long long)n + (long long)measured[s];
        }
    }
}

// What every search entry requires of a batch: the operand limits of igan_conv2d, which forms the products.
int check_batch(const char* name, int nq, int nc, int dim) {
    if (!(nq >= 1 && nc >= 1 && dim >= 1)) return fail(IGAN_ERR_INVALID_ARGUMENT, "%s: sizes must be positive", name);
    if ((long long)nq * dim * 4 > 0x7FFFFFF0LL) return fail(IGAN_ERR_INVALID_ARGUMENT, "%s: query batch too large (2 GiB per operand)", name);
    if ((long long)nc * dim * 4 > 0x7FFFFFF0LL) return fail(IGAN_ERR_INVALID_ARGUMENT, "%s: candidate batch too large (2 GiB per operand)", name);
    if ((long long)nq * nc > INT32_MAX) return fail(IGAN_ERR_INVALID_ARGUMENT, "%s: product block too large", name);
    return IGAN_OK;
}

// launch(KC) with the compiled list length for k <= 16 entries, an integral constant: 4, 8 or 16.
template <class Launch>
void with_list_length(int k, Launch launch) {
    if (k <= 4) launch(std::integral_constant<int, 4>());
    else if (k <= 8) launch(std::integral_constant<int, 8>());
    else launch(std::integral_constant<int, 16>());
}

}  // namespace

extern "C" int igan_row_sqnorm(igan_stream_t stream_, const float* a, float* out, int rows, int dim) {
    IGAN_REQUIRE(a && out, "row_sqnorm: null buffer");
    IGAN_REQUIRE(rows >= 1 && dim >= 1, "row_sqnorm: sizes must be positive");
    hipLaunchKernelGGL(row_sqnorm_kernel, dim3(ceil_div(rows, 4)), dim3(256), 0, (hipStream_t)stream_, a, out, rows, dim);
    IGAN_LAUNCH_CHECK("row_sqnorm launch");
    return IGAN_OK;
}

extern "C" int igan_nn1_update(igan_stream_t stream_, const float* query, const float* qnorm,
                               const float* cand, const float* cnorm, double* best_d2, int* best_idx,
                               float* dots, int nq, int nc, int dim, int idx_base) {
    IGAN_REQUIRE(query && qnorm && cand && cnorm && best_d2 && best_idx && dots, "nn1_update: null buffer");
    if (int rc = check_batch("nn1_update", nq, nc, dim)) return rc;
    IGAN_REQUIRE(idx_base >= 0 && (long long)idx_base + nc <= INT32_MAX, "nn1_update: candidate index overflows int32");
    if (int rc = distance_products(stream_, query, cand, dots, nq, nc, dim)) return rc;
    hipLaunchKernelGGL(nn1_fold_kernel, dim3(ceil_div(nq, 4)), dim3(256), 0, (hipStream_t)stream_, dots, qnorm, cnorm, query, cand,
                       best_d2, best_idx, nq, nc, dim, idx_base);
    IGAN_LAUNCH_CHECK("nn1_fold launch");
    return IGAN_OK;
}

extern "C" int igan_nnk_update(igan_stream_t stream_, const float* query, const float* qnorm,
                               const float* cand, const float* cnorm, double* best_d2, int* best_idx,
                               float* dots, int nq, int nc, int dim, int k, int idx_base) {
    IGAN_REQUIRE(query && qnorm && cand && cnorm && best_d2 && best_idx && dots, "nnk_update: null buffer");
    if (int rc = check_batch("nnk_update", nq, nc, dim)) return rc;
    if (k < 1 || k > 16) return fail(IGAN_ERR_UNSUPPORTED, "nnk_update: 1 <= k <= 16 neighbours (the lists live in registers)");
    IGAN_REQUIRE(idx_base >= 0 && (long long)idx_base + nc <= INT32_MAX, "nnk_update: candidate index overflows int32");
    if (int rc = distance_products(stream_, query, cand, dots, nq, nc, dim)) return rc;
    with_list_length(k, [&](auto kc) {
        hipLaunchKernelGGL(nnk_fold_kernel<decltype(kc)::value>, dim3(ceil_div(nq, 4)), dim3(256), 0, (hipStream_t)stream_, dots, qnorm,
                           cnorm, query, cand, best_d2, best_idx, nq, nc, dim, k, idx_base);
    });
    IGAN_LAUNCH_CHECK("nnk_fold launch");
    return IGAN_OK;
}

extern "C" int igan_knn_radius_update(igan_stream_t stream_, const float* query, const float* qnorm,
                                      const float* cand, const float* cnorm, double* kth_d2,
                                      float* dots, int nq, int nc, int dim, int kcap) {
    IGAN_REQUIRE(query && qnorm && cand && cnorm && kth_d2 && dots, "knn_radius_update: null buffer");
    if (int rc = check_batch("knn_radius_update", nq, nc, dim)) return rc;
    IGAN_REQUIRE(kcap >= 1 && kcap <= 16, "knn_radius_update: kcap must be in [1, 16]");
    if (int rc = distance_products(stream_, query, cand, dots, nq, nc, dim)) return rc;
    with_list_length(kcap, [&](auto kc) {
        hipLaunchKernelGGL(knn_radius_fold_kernel<decltype(kc)::value>, dim3(ceil_div(nq, 4)), dim3(256), 0, (hipStream_t)stream_, dots,
                           qnorm, cnorm, query, cand, kth_d2, nq, nc, dim, kcap);
    });
    IGAN_LAUNCH_CHECK("knn_radius_fold launch");
    return IGAN_OK;
}

extern "C" int igan_manifold_member_update(igan_stream_t stream_, const float* query, const float* qnorm,
                                           const float* cand, const float* cnorm, const double* cand_radius,
                                           int* member, float* dots, int nq, int nc, int dim, int nk) {
    IGAN_REQUIRE(query && qnorm && cand && cnorm && cand_radius && member && dots, "manifold_member_update: null buffer");
    if (int rc = check_batch("manifold_member_update", nq, nc, dim)) return rc;
    IGAN_REQUIRE(nk >= 1 && nk <= 8, "manifold_member_update: nk must be in [1, 8]");
    if (int rc = distance_products(stream_, query, cand, dots, nq, nc, dim)) return rc;
    hipLaunchKernelGGL(manifold_member_fold_kernel, dim3(ceil_div(nq, 4)), dim3(256), 0, (hipStream_t)stream_, dots, qnorm, cnorm,
                       query, cand, cand_radius, member, nq, nc, dim, nk);
    IGAN_LAUNCH_CHECK("manifold_member_fold launch");
    return IGAN_OK;
}

extern "C" int igan_ball_count_update(igan_stream_t stream_, const float* query, const float* qnorm, const double* query_radius,
                                      const float* cand, const float* cnorm, long long* count, float* dots,
                                      int nq, int nc, int dim, int nk, int inclusive) {
    IGAN_REQUIRE(query && qnorm && query_radius && cand && cnorm && count && dots, "ball_count_update: null buffer");
    if (int rc = check_batch("ball_count_update", nq, nc, dim)) return rc;
    IGAN_REQUIRE(nk >= 1 && nk <= 8, "ball_count_update: nk must be in [1, 8]");
    IGAN_REQUIRE(inclusive == 0 || inclusive == 1, "ball_count_update: inclusive must be 0 (d2 < R) or 1 (d2 <= R)");
    if (int rc = distance_products(stream_, query, cand, dots, nq, nc, dim)) return rc;
    if (inclusive)
        hipLaunchKernelGGL(ball_count_fold_kernel<true>, dim3(ceil_div(nq, 4)), dim3(256), 0, (hipStream_t)stream_, dots, qnorm, cnorm,
                           query, cand, query_radius, count, nq, nc, dim, nk);
    else
        hipLaunchKernelGGL(ball_count_fold_kernel<false>, dim3(ceil_div(nq, 4)), dim3(256), 0, (hipStream_t)stream_, dots, qnorm, cnorm,
                           query, cand, query_radius, count, nq, nc, dim, nk);
    IGAN_LAUNCH_CHECK("ball_count_fold launch");
    return IGAN_OK;
}

// Membership and nearest neighbour of one candidate batch on ONE product block: distance_products() once, then the two fold
// kernels above, unchanged, on the same `dots`.  Each fold keeps its own early exit and its own NaN policy, so member, best_d2
// and best_idx are those of igan_manifold_member_update followed by igan_nn1_update by construction; the folds only read
// `dots`, and the stream orders them after the product.
extern "C" int igan_manifold_member_nn1_update(igan_stream_t stream_, const float* query, const float* qnorm,
                                               const float* cand, const float* cnorm, const double* cand_radius,
                                               int* member, double* best_d2, int* best_idx, float* dots,
                                               int nq, int nc, int dim, int nk, int idx_base) {
    IGAN_REQUIRE(query && qnorm && cand && cnorm && cand_radius && member && best_d2 && best_idx && dots,
                 "manifold_member_nn1_update: null buffer");
    if (int rc = check_batch("manifold_member_nn1_update", nq, nc, dim)) return rc;
    IGAN_REQUIRE(nk >= 1 && nk <= 8, "manifold_member_nn1_update: nk must be in [1, 8]");
    IGAN_REQUIRE(idx_base >= 0 && (long long)idx_base + nc <= INT32_MAX, "manifold_member_nn1_update: candidate index overflows int32");
    if (int rc = distance_products(stream_, query, cand, dots, nq, nc, dim)) return rc;
    hipLaunchKernelGGL(manifold_member_fold_kernel, dim3(ceil_div(nq, 4)), dim3(256), 0, (hipStream_t)stream_, dots, qnorm, cnorm,
                       query, cand, cand_radius, member, nq, nc, dim, nk);
    IGAN_LAUNCH_CHECK("manifold_member_fold launch");
    hipLaunchKernelGGL(nn1_fold_kernel, dim3(ceil_div(nq, 4)), dim3(256), 0, (hipStream_t)stream_, dots, qnorm, cnorm, query, cand,
                       best_d2, best_idx, nq, nc, dim, idx_base);
    IGAN_LAUNCH_CHECK("nn1_fold launch");
    return IGAN_OK;
}
