// pcr_segment.hip -- plane segmentation on gfx950: PointCloud.segment_plane of Open3D as ONE sequential RANSAC loop over hypotheses
// i = 0, 1, ... (include/pcr_hip.h states the rules SAMPLE, FIT, SCORE, BETTER, STOP and RESULT), evaluated in rounds of PS_ROUND by the frame of
// pcr_hypo.h with a 4-number model (PsPolicy): score, split sum, and the sequential better-than and stop rule in ONE workgroup, so that the
// answer depends neither on PS_ROUND nor on how many rounds are enqueued before the host looks at the state.  This unit's own:
//   k_ps_hypo    one lane per hypothesis: counter-based draw and the fit of pcr_plane.h -> valid flag and 4 doubles.  Nearly every sample is
//                valid (a repeated row or three collinear points are not), so there is no list of valid hypotheses: an invalid one is scored
//                like the others and its count is replaced by -1 in the split sum
//   PsPolicy     the residual pcr_plane_dist, better-than, the probability rule
// and a final pass: inlier flags of the winner by the expression that counted them, their ascending indices, and the fixed-order float64
// centroid and centred second moments of the inliers, which the host hands to the moment fit of pcr_plane.h (Open3D's last step).
// Every loop is bounded by a count; no kernel waits on another workgroup; no float atomics.  Contraction is off: pcr_plane.h's expressions
// have the bits of a host recomputation.
#pragma clang fp contract(off)
#include <algorithm>
#include <cmath>
#include <cstring>
#include "pcr_device.h"
#include "pcr_umeyama.h"
#include "pcr_plane.h"
#include "pcr_hypo.h"

#define PS_ROUND 1024              // hypotheses per round (internal: the results do not depend on it)
#define PS_BS 256
#define PS_TILE 512                // points per LDS tile: 3 doubles each, 12 KB
#define PS_SPLIT_ROWS 1024         // rows one lane of the score walks, about
#define PS_MAX_SPLITS 256          // from PS_MAX_SPLITS * PS_SPLIT_ROWS points on a lane walks more rows instead
#define PS_SEL_BS 64               // threads of the select: thread 0 walks one chunk record per thread, so few and long chunks
#define PS_MOM_MAX_BLOCKS 256
#define PS_MAX_POINTS 0x7fffffffLL    // the clouds of this library are counted in int

typedef HypoState<4> PsState;      // best_err is a sum of distances

struct PsArgs {
    const float *xyz; int n;
    uint64_t seed;
    long long first; int count;          // this round: iterations [first, first + count)
    const PsState *st;                    // null: no early exit (test hook)
    uint8_t *valid; double *plane;        // per hypothesis of the round
};

// what the frame of pcr_hypo.h takes from this unit
struct PsPolicy {
    typedef PsState State; typedef float Row;
    static constexpr int DIM = 4, ROWD = 3, TILE = PS_TILE, SPLIT_ROWS = PS_SPLIT_ROWS, MAX_SPLITS = PS_MAX_SPLITS, ROUND = PS_ROUND, SEL_BS = PS_SEL_BS, UNROLL = 4, SUM_UNROLL = 8;
    static constexpr bool LISTED = false, STOPS = true;
    __host__ __device__ static constexpr int stride(int) { return PS_ROUND; }
    __device__ static inline double residual(const double *pl, const double *p) { return pcr_plane_dist(pl, p[0], p[1], p[2]); }
    __device__ static inline void init_model(PsState *st) { for (int k = 0; k < 4; k++) st->best[k] = 0.0; }
    // better-than rule: more inliers, or as many with a strictly smaller rmse = err / sqrt(count); (bc == 0: the empty start, beaten by any inlier at all)
    __device__ static inline bool better(int c, double e, int bc, double be) {
        if (c <= 0) return false;
        if (c != bc) return c > bc;
        return e / sqrt((double)c) < be / sqrt((double)bc);
    }
    __device__ static inline void est_k(PsState &s, int c, int n, int ransac_n, double probability, double log_fail) {
        if (!(probability < 1.0)) return;                     // probability == 1 never stops early
        const double rho = (double)c / (double)n;
        double p = 1.0;
        for (int k = 0; k < ransac_n; k++) p *= rho;
        // k' = log(1 - probability) / log(1 - rho^n), the denominator as log1p(-p): 1 - p rounds to 1 for p below 1e-16, where k' is
        // astronomically large, not -inf; every point an inlier: k' = 0.  Only a finite k' >= 0 below est_k shortens the run.
        const double kp = c == n ? 0.0 : log_fail / log1p(-p);
        if (isfinite(kp) && kp >= 0.0 && kp < (double)s.est_k) s.est_k = (long long)ceil(kp);
    }
};

template <int N> __global__ void __launch_bounds__(PS_BS) k_ps_hypo(PsArgs a) {
    const int h = blockIdx.x * PS_BS + threadIdx.x;
    if (h >= a.count) return;
    if (a.st && a.st->stop) return;
    const uint64_t i = (uint64_t)a.first + (uint64_t)h;
    float s[N][3];
#pragma unroll
    for (int k = 0; k < N; k++) {
        const size_t r = (size_t)(pcr_splitmix64(a.seed + (uint64_t)N * i + (uint64_t)k) % (uint64_t)a.n);
        s[k][0] = a.xyz[3 * r]; s[k][1] = a.xyz[3 * r + 1]; s[k][2] = a.xyz[3 * r + 2];
    }
    double pl[4];
    bool ok;
    if (N == 3) {
        const double p0[3] = {(double)s[0][0], (double)s[0][1], (double)s[0][2]}, p1[3] = {(double)s[1][0], (double)s[1][1], (double)s[1][2]},
                     p2[3] = {(double)s[2][0], (double)s[2][1], (double)s[2][2]};
        ok = pcr_plane_from_3(p0, p1, p2, pl);
    } else {
        ok = pcr_plane_from_sample<N>(s, pl);
    }
    a.valid[h] = ok ? 1 : 0;
#pragma unroll
    for (int k = 0; k < 4; k++) a.plane[(size_t)h * 4 + k] = pl[k];
}

// the inlier rows of the winner, by the expression that counted them
__global__ void __launch_bounds__(PS_BS) k_ps_inlier_flags(const float *__restrict__ xyz, int n, const PsState *__restrict__ st, double thr, uint8_t *__restrict__ flags) {
    const int i = blockIdx.x * PS_BS + threadIdx.x;
    if (i >= n) return;
    double pl[4];
#pragma unroll
    for (int k = 0; k < 4; k++) pl[k] = st->best[k];
    flags[i] = pcr_plane_dist(pl, (double)xyz[(size_t)i * 3], (double)xyz[(size_t)i * 3 + 1], (double)xyz[(size_t)i * 3 + 2]) < thr ? 1 : 0;
}

// Float64 sums over the flagged rows, in the frame of the cloud moments of pcr_query.hip: wavefront reduction, one slab per workgroup, and a
// one-workgroup launch that adds the slabs in a fixed tree; the grid depends on n alone, so two runs give the same bits.  Pass 1
// (centre_sums == nullptr): the three coordinate sums.  Pass 2: the six products of (p - c), c = sums of pass 1 / count, each a rounded quotient.
__global__ void __launch_bounds__(PS_BS) k_ps_moments_partial(const float *__restrict__ xyz, const uint8_t *__restrict__ flags, int n, const double *__restrict__ centre_sums,
                                                              double count, double *__restrict__ slabs) {
    const double cx = centre_sums ? centre_sums[0] / count : 0.0, cy = centre_sums ? centre_sums[1] / count : 0.0, cz = centre_sums ? centre_sums[2] / count : 0.0;
    double s[6] = {0, 0, 0, 0, 0, 0};
    for (long long i = blockIdx.x * PS_BS + threadIdx.x; i < n; i += gridDim.x * PS_BS) {
        if (!flags[i]) continue;
        const double x = (double)xyz[(size_t)i * 3] - cx, y = (double)xyz[(size_t)i * 3 + 1] - cy, z = (double)xyz[(size_t)i * 3 + 2] - cz;
        if (!centre_sums) { s[0] += x; s[1] += y; s[2] += z; }
        else { s[0] += x * x; s[1] += x * y; s[2] += x * z; s[3] += y * y; s[4] += y * z; s[5] += z * z; }
    }
    __shared__ double w[PS_BS / PCR_WAVE][6];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int t = 0; t < 6; t++) { const double r = pcr_wave_sum(s[t]); if (lane == 0) w[wv][t] = r; }
    __syncthreads();
    if (threadIdx.x < 6) {
        double v = w[0][threadIdx.x];
        for (int k = 1; k < PS_BS / PCR_WAVE; k++) v += w[k][threadIdx.x];
        slabs[(size_t)blockIdx.x * 6 + threadIdx.x] = v;
    }
}
// one wavefront per column: lane l adds the slabs l, l + 64, ... in that order, then the fixed tree of pcr_wave_sum
__global__ void __launch_bounds__(6 * PCR_WAVE) k_ps_moments_final(const double *__restrict__ slabs, int nb, double *__restrict__ out6) {
    const int col = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double v = 0.0;
    for (int k = lane; k < nb; k += PCR_WAVE) v += slabs[(size_t)k * 6 + col];
    v = pcr_wave_sum(v);
    if (lane == 0) out6[col] = v;
}

// test hook: what the round left for its hypotheses, copied to the caller's arrays
__global__ void __launch_bounds__(PS_BS) k_ps_dump(const uint8_t *__restrict__ valid, const double *__restrict__ plane, const int *__restrict__ cnt, const double *__restrict__ err, int count,
                                                   uint8_t *__restrict__ valid_out, double *__restrict__ plane_out, int32_t *__restrict__ inl_out, double *__restrict__ err_out) {
    const int h = blockIdx.x * PS_BS + threadIdx.x;
    if (h >= count) return;
    valid_out[h] = valid[h]; inl_out[h] = cnt[h]; err_out[h] = err[h];
    for (int k = 0; k < 4; k++) plane_out[(size_t)h * 4 + k] = plane[(size_t)h * 4 + k];
}

// ------------------------------------------------------------------------------------------------------------------ host
struct PsRun {                     // the device image of one call
    PsArgs a; PsState *st; HypoScore<PsPolicy> s;
};

static size_t ps_scratch_bytes(int64_t n) {
    return (size_t)n * (1 + 4) + (size_t)n / 16 + (size_t)PS_ROUND * (1 + 4 * 8 + 4 + 8) + (size_t)PS_MAX_SPLITS * PS_ROUND * 12 + (size_t)PS_MOM_MAX_BLOCKS * 6 * 8 + (1u << 20);
}

static int ps_check(pcr_context *ctx, const float *xyz, int64_t n, double thr, const pcr_plane_params *p) {
    if (!p) { ctx->err = "segment_plane: no parameters"; return PCR_EINVAL; }
    if (p->ransac_n < 3 || p->ransac_n > 8) { ctx->err = "segment_plane: ransac_n must be in 3..8"; return PCR_EINVAL; }
    if (n < 0 || n > PS_MAX_POINTS) { ctx->err = "segment_plane: bad point count"; return PCR_EINVAL; }
    if (n < p->ransac_n) { ctx->err = "segment_plane: fewer points than ransac_n"; return PCR_EINVAL; }
    if (!xyz) { ctx->err = "segment_plane: missing cloud"; return PCR_EINVAL; }
    if (!(thr >= 0.0) || !std::isfinite(thr)) { ctx->err = "segment_plane: distance_threshold negative or not finite"; return PCR_EINVAL; }
    if (p->num_iterations < 0) { ctx->err = "segment_plane: num_iterations < 0"; return PCR_EINVAL; }
    if (!(p->probability > 0.0 && p->probability <= 1.0)) { ctx->err = "segment_plane: probability must be in (0, 1]"; return PCR_EINVAL; }
    return PCR_OK;
}

// lays out the round buffers (scratch from the arena above the current mark; the caller has reserved ps_scratch_bytes)
static int ps_setup(pcr_context *ctx, PsRun &R, const float *xyz, int n, double thr, const pcr_plane_params *p) {
    memset(&R, 0, sizeof R);
    PsArgs &a = R.a;
    R.st = arena<PsState>(ctx, 1);
    a.valid = arena<uint8_t>(ctx, PS_ROUND); a.plane = arena<double>(ctx, (size_t)PS_ROUND * 4);
    R.s.cnt = arena<int>(ctx, PS_ROUND); R.s.err = arena<double>(ctx, PS_ROUND);
    if (!R.st || !a.valid || !a.plane || !R.s.cnt || !R.s.err) return PCR_ENOMEM;
    PCR_TRY(hypo_score_alloc(ctx, R.s, n, PS_ROUND));
    a.xyz = xyz; a.n = n; a.seed = p->seed;
    R.s.ra = xyz; R.s.rows = n; R.s.thr = thr; R.s.model = a.plane; R.s.valid = a.valid;
    PCR_LAUNCH(ctx, k_hypo_init<PsPolicy>, dim3(1), dim3(1), 0, ctx->stream, R.st, (long long)p->num_iterations);
    return PCR_OK;
}

// hypotheses, scores and the per-hypothesis (count, err) of iterations [first, first + count), count <= PS_ROUND
static int ps_round(pcr_context *ctx, PsRun &R, int ransac_n, long long first, int count, bool early_exit) {
    PsArgs a = R.a;
    a.first = first; a.count = count; a.st = early_exit ? R.st : nullptr;
    PCR_TRY(hypo_dispatch_n(ransac_n, [&](auto N) -> int {
        PCR_LAUNCH(ctx, k_ps_hypo<decltype(N)::value>, dim3((count + PS_BS - 1) / PS_BS), dim3(PS_BS), 0, ctx->stream, a);
        return PCR_OK;
    }));
    hypo_score(ctx, R.s, count, a.st ? &a.st->stop : nullptr);
    return PCR_OK;
}

extern "C" int pcr_segment_plane(pcr_context *ctx, const float *xyz, int64_t n, double distance_threshold, const pcr_plane_params *params, double *plane4,
                                 uint8_t *inlier_mask, int64_t *out_index, int64_t *out_n, pcr_plane_info *info) {
    return pcr_api_call(ctx, [&]() -> int {
        PCR_TRY(ps_check(ctx, xyz, n, distance_threshold, params));
        if (!plane4) { ctx->err = "segment_plane: no plane output"; return PCR_EINVAL; }
        for (int k = 0; k < 4; k++) plane4[k] = 0.0;
        if (out_n) *out_n = 0;
        if (info) { memset(info, 0, sizeof *info); info->best_iteration = -1; }
        if (inlier_mask) PCR_HIP_CHECK(ctx, hipMemsetAsync(inlier_mask, 0, (size_t)n, ctx->stream));
        if (params->num_iterations == 0) return PCR_OK;
        PCR_TRY(pcr_arena_reserve(ctx, ps_scratch_bytes(n)));
        PsRun R;
        PCR_TRY(ps_setup(ctx, R, xyz, (int)n, distance_threshold, params));
        PsState h; memset(&h, 0, sizeof h);
        h.best_iter = -1;
        HypoSelectArgs<PsPolicy> sa;
        sa.st = R.st; sa.cnt = R.s.cnt; sa.err = R.s.err; sa.model = R.a.plane; sa.rows = (int)n; sa.n = params->ransac_n; sa.confidence = params->probability;
        PCR_TRY(hypo_run(ctx, sa, params->num_iterations, h, [&](long long first, int count) { return ps_round(ctx, R, params->ransac_n, first, count, true); },
                         [](const PsState &) { return PCR_OK; }));
        if (info) { info->iterations_run = h.iterations_run; info->best_iteration = h.best_iter; info->n_valid = h.n_valid; }
        if (h.best_iter < 0) return PCR_OK;                      // no valid hypothesis with an inlier: the zero plane, no inliers
        if (info) {
            info->n_inliers = h.best_count; info->fitness = (double)h.best_count / (double)n;
            info->inlier_rmse = h.best_err / sqrt((double)h.best_count);
        }
        // final pass: the winner's inlier rows, their indices, and the moment fit over them
        uint8_t *flags = inlier_mask ? inlier_mask : arena<uint8_t>(ctx, n);
        if (!flags) return PCR_ENOMEM;
        const dim3 g((unsigned)((n + PS_BS - 1) / PS_BS)), b(PS_BS);
        PCR_LAUNCH(ctx, k_ps_inlier_flags, g, b, 0, ctx->stream, xyz, (int)n, (const PsState *)R.st, distance_threshold, flags);
        int64_t n_in = 0;
        PCR_TRY(pcr_emit_kept_rows(ctx, xyz, n, flags, nullptr, out_index, &n_in));
        if (n_in != h.best_count) { ctx->err = "segment_plane: the inlier pass disagrees with the score of the winner"; return PCR_ENUMERIC; }
        if (out_n) *out_n = n_in;
        const int nb = (int)std::min<int64_t>((n + PS_BS - 1) / PS_BS, PS_MOM_MAX_BLOCKS);
        double *slabs = arena<double>(ctx, (size_t)nb * 6), *out = arena<double>(ctx, 12);
        if (!slabs || !out) return PCR_ENOMEM;
        PCR_HIP_CHECK(ctx, hipMemsetAsync(out, 0, 12 * sizeof(double), ctx->stream));
        for (int pass = 0; pass < 2; pass++) {                   // (pass 2 reuses the slabs: the stream orders it after the final launch of pass 1)
            PCR_LAUNCH(ctx, k_ps_moments_partial, dim3(nb), b, 0, ctx->stream, xyz, (const uint8_t *)flags, (int)n, pass == 0 ? (const double *)nullptr : (const double *)out,
                       (double)n_in, slabs);
            PCR_LAUNCH(ctx, k_ps_moments_final, dim3(1), dim3(6 * PCR_WAVE), 0, ctx->stream, (const double *)slabs, nb, out + 6 * pass);
        }
        double s[12];
        PCR_HIP_CHECK(ctx, hipMemcpyAsync(s, out, sizeof s, hipMemcpyDeviceToHost, ctx->stream));
        PCR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        const double c[3] = {s[0] / (double)n_in, s[1] / (double)n_in, s[2] / (double)n_in};      // the centre pass 2 took
        pcr_plane_from_moments(c, s + 6, plane4);                // degenerate: the zero plane
        return PCR_OK;
    });
}

extern "C" int pcr_debug_plane_hypotheses(pcr_context *ctx, const float *xyz, int64_t n, double distance_threshold, const pcr_plane_params *params, int64_t first,
                                          int64_t count, uint8_t *valid_out, double *plane_out, int32_t *inliers_out, double *err_out) {
    return pcr_api_call(ctx, [&]() -> int {
        PCR_TRY(ps_check(ctx, xyz, n, distance_threshold, params));
        if (!valid_out || !plane_out || !inliers_out || !err_out || first < 0 || count < 0) { ctx->err = "segment_plane hypotheses: bad range or output pointer"; return PCR_EINVAL; }
        PCR_TRY(pcr_arena_reserve(ctx, ps_scratch_bytes(n)));
        PsRun R;
        PCR_TRY(ps_setup(ctx, R, xyz, (int)n, distance_threshold, params));
        return hypo_debug_rounds(PS_ROUND, first, count, [&](long long f, int c) { return ps_round(ctx, R, params->ransac_n, f, c, false); }, [&](int64_t done, int c) {
            PCR_LAUNCH(ctx, k_ps_dump, dim3((c + PS_BS - 1) / PS_BS), dim3(PS_BS), 0, ctx->stream, (const uint8_t *)R.a.valid, (const double *)R.a.plane, (const int *)R.s.cnt,
                       (const double *)R.s.err, c, valid_out + done, plane_out + done * 4, inliers_out + done, err_out + done);
        });
    });
}
