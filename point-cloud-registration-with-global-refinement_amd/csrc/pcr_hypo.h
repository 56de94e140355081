// pcr_hypo.h -- the frame of the hypothesise-and-score rounds: what RANSAC registration (pcr_ransac.hip), plane segmentation
// (pcr_segment.hip) and the SC2 seeds (pcr_sc2.hip) do alike, written once over a compile-time policy per unit: the loop state and its init, the
// score of a round (one lane per hypothesis, a tile of rows as doubles in LDS, the rows split over blockIdx.y), the sum of the splits, the
// sequential better-than and stop rule over a round, the index-pair emit, and on the host the split sizes, the dispatch over ransac_n, the
// round loop with its read-back cadence and the loop of the test hooks.  Nothing here branches on the unit at run time.
//
// FLOATING POINT.  This header sets no `fp contract` pragma: a unit includes it AFTER its own (on in pcr_ransac.hip, off in pcr_segment.hip and
// pcr_sc2.hip), and it holds no expression in which a product feeds a sum or a difference.  Every such expression (the residual, the root mean
// square of better-than) is a policy function, defined in the unit under the unit's pragma.
//
// A policy `P` names
//   DIM, ROWD, Row            doubles of a model; doubles of a staged row (6: a source and a target point, 3: a point); float4 or float
//   TILE, SPLIT_ROWS, MAX_SPLITS   rows of an LDS tile; rows one lane walks, about; the splits at most (beyond, a lane walks more rows)
//   LISTED                    the score runs over the round's list of valid hypotheses (list, *n_list; workgroups past the list return) and the
//                             sum writes cnt[list[j]]; otherwise over all `count`, and the sum writes valid[j] ? c : -1
//   STOPS                     score and sum return when *stop is set, and a wavefront past the round's end only helps to load
//   UNROLL, SUM_UNROLL        `#pragma unroll` counts of the row loop and of the split sum (1: rolled), so that each unit keeps the loop it had
//   stride(count)             hypotheses between two splits of the partials
//   residual(model, row)      the number compared with the threshold and summed over the inliers
// and, where the unit runs the sequential loop (select): State (HypoState<DIM> or a struct derived from it), ROUND, SEL_BS, init_model(State *),
// better(c, e, bc, be) and est_k(State &, c, rows, n, confidence, log_fail), the whole confidence rule of the unit.
#pragma once
#include <algorithm>
#include <type_traits>
#include "pcr_internal.h"

#define HYPO_BS 256                // threads of the score, sum, init and emit workgroups
#define HYPO_ROUNDS_PER_READBACK 4
static inline unsigned hypo_blocks(int64_t n) { return (unsigned)((n + HYPO_BS - 1) / HYPO_BS); }

template <int DIM> struct HypoState {      // the sequential loop's state between rounds (device; the host reads it per chunk of rounds)
    long long est_k, iterations_run, best_iter, n_valid;
    double best_err, best[DIM];
    int best_count, stop;
};

// ================================================================ kernels
template <class P> __global__ void k_hypo_init(typename P::State *st, long long max_iteration) {
    st->est_k = max_iteration; st->iterations_run = 0; st->best_iter = -1; st->n_valid = 0; st->best_err = 0; st->best_count = 0;
    st->stop = max_iteration <= 0 ? 1 : 0;
    P::init_model(st);
}

// rows [base, base + m) as doubles into the tile
__device__ static inline void hypo_stage(double *sh, const float4 *__restrict__ ps, const float4 *__restrict__ pt, int base, int m) {
    for (int q = threadIdx.x; q < m; q += HYPO_BS) {
        const float4 s = ps[base + q], t = pt[base + q];
        sh[q * 6 + 0] = s.x; sh[q * 6 + 1] = s.y; sh[q * 6 + 2] = s.z; sh[q * 6 + 3] = t.x; sh[q * 6 + 4] = t.y; sh[q * 6 + 5] = t.z;
    }
}
__device__ static inline void hypo_stage(double *sh, const float *__restrict__ xyz, const float *__restrict__, int base, int m) {
    for (int q = threadIdx.x; q < 3 * m; q += HYPO_BS) sh[q] = (double)xyz[(size_t)base * 3 + q];
}

// One lane per hypothesis, its model in registers, a tile of rows in LDS (every lane reads the same address: a broadcast), the rows split over
// blockIdx.y -> per-split (count, sum of residuals) in row order.  (A late split of a short list may start past the end: no rows.)
template <class P>
__global__ void __launch_bounds__(HYPO_BS) k_hypo_score(const typename P::Row *__restrict__ ra, const typename P::Row *__restrict__ rb, int rows, int rows_per_split, double thr,
                                                        const double *__restrict__ model, int count, const int *__restrict__ list, const int *__restrict__ n_list,
                                                        const int *__restrict__ stop, int *__restrict__ pcnt, double *__restrict__ perr) {
    if (P::STOPS && stop && *stop) return;
    const int nl = P::LISTED ? *n_list : count;
    if (P::LISTED && (int)(blockIdx.x * HYPO_BS) >= nl) return;
    __shared__ double sh[P::TILE * P::ROWD];
    const int j = blockIdx.x * HYPO_BS + threadIdx.x;
    const bool live = j < nl;
    const int h = P::LISTED ? list[live ? j : nl - 1] : (live ? j : nl - 1);
    double M[P::DIM];
#pragma unroll
    for (int k = 0; k < P::DIM; k++) M[k] = model[(size_t)h * P::DIM + k];
    const long long r0l = (long long)blockIdx.y * rows_per_split;
    const int r0 = (int)min(r0l, (long long)rows), r1 = (int)min(r0l + rows_per_split, (long long)rows);
    const bool wave_live = !P::STOPS || (int)(blockIdx.x * HYPO_BS + (threadIdx.x & ~63)) < nl;
    int cnt = 0; double e = 0.0;
    for (int base = r0; base < r1; base += P::TILE) {
        const int m = min(P::TILE, r1 - base);
        __syncthreads();
        hypo_stage(sh, ra, rb, base, m);
        __syncthreads();
        if (!wave_live) continue;
#pragma unroll P::UNROLL
        for (int q = 0; q < m; q++) {
            const double d = P::residual(M, sh + q * P::ROWD);
            const bool in = d < thr;
            cnt += in ? 1 : 0; e += in ? d : 0.0;
        }
    }
    if (live) { pcnt[(size_t)blockIdx.y * P::stride(count) + j] = cnt; perr[(size_t)blockIdx.y * P::stride(count) + j] = e; }
}

// the splits summed in ascending order of their row ranges
template <class P>
__global__ void __launch_bounds__(HYPO_BS) k_hypo_sum(const int *__restrict__ pcnt, const double *__restrict__ perr, int splits, int count, const int *__restrict__ list,
                                                      const int *__restrict__ n_list, const uint8_t *__restrict__ valid, const int *__restrict__ stop,
                                                      int *__restrict__ cnt, double *__restrict__ err) {
    const int j = blockIdx.x * HYPO_BS + threadIdx.x;
    if (j >= (P::LISTED ? *n_list : count)) return;
    if (P::STOPS && stop && *stop) return;
    int c = 0; double e = 0.0;
#pragma unroll P::SUM_UNROLL
    for (int y = 0; y < splits; y++) { c += pcnt[(size_t)y * P::stride(count) + j]; e += perr[(size_t)y * P::stride(count) + j]; }
    if (P::LISTED) { cnt[list[j]] = c; err[list[j]] = e; }
    else { const bool ok = valid[j] != 0; cnt[j] = ok ? c : -1; err[j] = ok ? e : 0.0; }
}

template <class P> struct HypoSelectArgs {
    typename P::State *st; const int *cnt; const double *err; const double *model;
    long long first; int count, rows, n; double confidence;      // this round: iterations [first, first + count); rows scored, sample size
};
// The sequential loop over the round in one workgroup.  Each thread folds CHUNK consecutive hypotheses into (first strict best, valid count);
// thread 0 then walks the SEL_BS chunk records in order.  est_k is a function of the best COUNT so far alone (k' falls as the count grows, an
// equal count leaves it where it is), so a chunk that ends before est_k and holds no count above the running best can neither stop the loop nor
// move est_k: only its best enters.  Every other chunk is walked hypothesis by hypothesis.
template <class P> __global__ void __launch_bounds__(P::SEL_BS) k_hypo_select(HypoSelectArgs<P> a) {
    constexpr int CHUNK = P::ROUND / P::SEL_BS;
    if (a.st->stop) return;
    __shared__ int l_idx[P::SEL_BS], l_cnt[P::SEL_BS], l_nv[P::SEL_BS];
    __shared__ double l_err[P::SEL_BS];
    {
        const int b = threadIdx.x * CHUNK, m = min(CHUNK, a.count - b);
        int bi = -1, bc = 0, nv = 0; double be = 0.0;
        for (int q = 0; q < m; q++) {
            const int c = a.cnt[b + q];
            nv += c >= 0 ? 1 : 0;
            if (c > 0) { const double e = a.err[b + q]; if (P::better(c, e, bc, be)) { bi = b + q; bc = c; be = e; } }
        }
        l_idx[threadIdx.x] = bi; l_cnt[threadIdx.x] = bc; l_nv[threadIdx.x] = nv; l_err[threadIdx.x] = be;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    typename P::State s = *a.st;
    const double log_fail = log(1.0 - a.confidence);
    int stop = 0; long long run = a.first + a.count;
    for (int ch = 0; ch < P::SEL_BS && !stop; ch++) {
        const int b = ch * CHUNK, m = min(CHUNK, a.count - b);
        if (m <= 0) break;
        if (a.first + b + m <= s.est_k && (l_idx[ch] < 0 || l_cnt[ch] <= s.best_count)) {
            if (l_idx[ch] >= 0 && P::better(l_cnt[ch], l_err[ch], s.best_count, s.best_err)) { s.best_count = l_cnt[ch]; s.best_err = l_err[ch]; s.best_iter = a.first + l_idx[ch]; }
            s.n_valid += l_nv[ch];
            continue;
        }
        for (int q = 0; q < m; q++) {
            const long long i = a.first + b + q;
            if (i >= s.est_k) { stop = 1; run = i; break; }
            const int c = a.cnt[b + q];
            if (c >= 0) s.n_valid++;
            if (c <= 0) continue;
            const double e = a.err[b + q];
            if (!P::better(c, e, s.best_count, s.best_err)) continue;
            s.best_count = c; s.best_err = e; s.best_iter = i;
            P::est_k(s, c, a.rows, a.n, a.confidence, log_fail);
        }
    }
    if (!stop && run >= s.est_k) stop = 1;
    s.iterations_run = run; s.stop = stop;
    if (s.best_iter >= a.first)
        for (int k = 0; k < P::DIM; k++) s.best[k] = a.model[(size_t)(s.best_iter - a.first) * P::DIM + k];
    *a.st = s;
}

// the flagged rows of an index-pair list, each at its scanned position (a template only so that two units may take it from this header)
template <int BS = HYPO_BS> __global__ void __launch_bounds__(BS) k_hypo_emit(const int32_t *__restrict__ corres, const uint8_t *__restrict__ flags, const int *__restrict__ pos, int C, int32_t *__restrict__ out) {
    const int i = blockIdx.x * BS + threadIdx.x;
    if (i >= C || !flags[i]) return;
    out[2 * (size_t)pos[i]] = corres[2 * (size_t)i]; out[2 * (size_t)pos[i] + 1] = corres[2 * (size_t)i + 1];
}

// ================================================================ host
struct HypoSplits { int splits, rows_per_split; };
static inline HypoSplits hypo_splits(int64_t rows, int split_rows, int max_splits) {
    const int splits = (int)std::max<int64_t>(1, std::min<int64_t>(max_splits, (rows + split_rows - 1) / split_rows));
    return {splits, (int)((rows + splits - 1) / splits)};
}

template <class P> struct HypoScore {      // what the score of a round reads and writes (device)
    const typename P::Row *ra, *rb; int rows; double thr;            // the rows (rb: the target points of a pair list), the threshold as the residual has it
    const double *model; const uint8_t *valid; const int *list, *n_list;      // per hypothesis; list and n_list where LISTED, valid where not
    int *cnt; double *err;                                           // per hypothesis: inliers (-1: invalid) and their summed residuals
    HypoSplits sp; int *pcnt; double *perr;
};
// the split sizes and the partials of rounds of at most `count` hypotheses, from the arena
template <class P> static int hypo_score_alloc(pcr_context *ctx, HypoScore<P> &s, int64_t rows, int count) {
    s.sp = hypo_splits(rows, P::SPLIT_ROWS, P::MAX_SPLITS);
    s.pcnt = arena<int>(ctx, (size_t)s.sp.splits * P::stride(count)); s.perr = arena<double>(ctx, (size_t)s.sp.splits * P::stride(count));
    return s.pcnt && s.perr ? PCR_OK : PCR_ENOMEM;
}
template <class P> static void hypo_score(pcr_context *ctx, const HypoScore<P> &s, int count, const int *stop) {
    const dim3 g(hypo_blocks(count)), b(HYPO_BS);
    PCR_LAUNCH(ctx, k_hypo_score<P>, dim3(g.x, s.sp.splits), b, 0, ctx->stream, s.ra, s.rb, s.rows, s.sp.rows_per_split, s.thr, s.model, count, s.list, s.n_list, stop, s.pcnt, s.perr);
    PCR_LAUNCH(ctx, k_hypo_sum<P>, g, b, 0, ctx->stream, s.pcnt, s.perr, s.sp.splits, count, s.list, s.n_list, s.valid, stop, s.cnt, s.err);
}

// f(std::integral_constant<int, N>) for the sample size n in 3..8
template <class F> static inline int hypo_dispatch_n(int n, F f) {
    switch (n) {
        case 3: return f(std::integral_constant<int, 3>());
        case 4: return f(std::integral_constant<int, 4>());
        case 5: return f(std::integral_constant<int, 5>());
        case 6: return f(std::integral_constant<int, 6>());
        case 7: return f(std::integral_constant<int, 7>());
        case 8: return f(std::integral_constant<int, 8>());
        default: return PCR_EINVAL;
    }
}

// The loop of rounds: round(first, count) enqueues the hypotheses and scores of iterations [first, first + count), the select follows, and
// the host reads the state back after the first round and then after every HYPO_ROUNDS_PER_READBACK, calls check(h) and stops on the flag.
// max_iteration 0: no round, one read-back (the state as k_hypo_init left it and what the unit's setup added to it).
template <class P, class Round, class Check>
static int hypo_run(pcr_context *ctx, HypoSelectArgs<P> sa, long long max_iteration, typename P::State &h, Round round, Check check) {
    long long first = 0; int rounds = 1;
    do {
        for (int r = 0; r < rounds && first < max_iteration; r++) {
            sa.first = first; sa.count = (int)std::min<long long>(P::ROUND, max_iteration - first);
            PCR_TRY(round(sa.first, sa.count));
            PCR_LAUNCH(ctx, k_hypo_select<P>, dim3(1), dim3(P::SEL_BS), 0, ctx->stream, sa);
            first += sa.count;
        }
        PCR_HIP_CHECK(ctx, hipMemcpyAsync(&h, sa.st, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
        PCR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        PCR_TRY(check(h));
        if (h.stop) break;
        rounds = HYPO_ROUNDS_PER_READBACK;
    } while (first < max_iteration);
    return PCR_OK;
}
// the test hooks: hypotheses [first, first + count) round by round, dump(done, c) after each round of c
template <class Round, class Dump> static int hypo_debug_rounds(int round_size, int64_t first, int64_t count, Round round, Dump dump) {
    for (int64_t done = 0; done < count; done += round_size) {
        const int c = (int)std::min<int64_t>(round_size, count - done);
        PCR_TRY(round((long long)(first + done), c));
        dump(done, c);
    }
    return PCR_OK;
}
