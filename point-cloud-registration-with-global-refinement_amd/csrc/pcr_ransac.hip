// pcr_ransac.hip -- RANSAC global registration on gfx950: registration_ransac_based_on_correspondence and
// registration_ransac_based_on_feature_matching of Open3D (0.13 and later; the reference itself calls neither: include/pcr_hip.h states the
// algorithm).  The semantics are those of ONE sequential loop over hypotheses i = 0, 1, ...; the device evaluates them in rounds of RS_ROUND:
//   k_rs_hypo    one lane per hypothesis: counter-based draw, edge-length check, float64 moments, icp_umeyama, distance / normal checks
//                -> valid flag, 12 doubles, and (an integer atomic: the ORDER of the list does not reach any result) a slot in the list of
//                valid hypotheses of the round
// and the frame of pcr_hypo.h with RsPolicy scores them, sums the row splits in fixed order and runs the sequential better-than and stop rule
// over the round in ONE workgroup, so that the answer does not depend on RS_ROUND.  This unit's own: k_rs_gather, k_rs_hypo<3..8>, rs_d2,
// RsPolicy (better-than, the confidence rule), k_rs_inlier_flags, k_rs_dump (test hook), the parameter checks and the entry points.
// The host reads one small record back per chunk of rounds.  Every loop is bounded by a count; no kernel waits on another workgroup.
// Floating-point contraction per source expression only, as in pcr_gicp.hip: rs_d2 gives the same bits in every kernel it is inlined into.
#pragma clang fp contract(on)
#include <algorithm>
#include <cmath>
#include <cstring>
#include <cstdlib>
#include "pcr_internal.h"
#include "pcr_umeyama.h"
#include "pcr_hypo.h"

#define RS_ROUND 16384             // hypotheses per round (internal: the results do not depend on it)
#define RS_BS 256
#define RS_TILE 512                // correspondence rows per LDS tile: 6 doubles each, 24 KB
#define RS_SPLIT_ROWS 1024         // rows one lane of the score walks, about
#define RS_MAX_SPLITS 64

struct RsState : HypoState<12> { int bad_index, pad; };      // best_err is a sum of d^2; bad_index: k_rs_gather met a row outside the clouds

struct RsArgs {
    const float4 *ps, *pt, *ns, *nt;     // gathered rows of the correspondence list: source / target point, source / target normal (null: no normal check)
    int C, with_scaling;
    uint64_t seed;
    double edge_thr, dist_thr2, cos_thr;  // negative edge_thr / dist_thr2: checker absent
    long long first; int count;           // this round: iterations [first, first + count)
    const RsState *st;                    // null: no early exit (test hook)
    uint8_t *valid; double *T; int *cnt; double *err2; int *list, *n_list;
};

// |T s - t|^2 in float64 on the float32 inputs; the one expression every kernel decides inliers with
__device__ static inline double rs_d2(const double *T, double sx, double sy, double sz, double tx, double ty, double tz) {
    const double x = T[0] * sx + T[1] * sy + T[2] * sz + T[3] - tx;
    const double y = T[4] * sx + T[5] * sy + T[6] * sz + T[7] - ty;
    const double z = T[8] * sx + T[9] * sy + T[10] * sz + T[11] - tz;
    return x * x + y * y + z * z;
}

// what the frame of pcr_hypo.h takes from this unit
struct RsPolicy {
    typedef RsState State; typedef float4 Row;
    static constexpr int DIM = 12, ROWD = 6, TILE = RS_TILE, SPLIT_ROWS = RS_SPLIT_ROWS, MAX_SPLITS = RS_MAX_SPLITS, ROUND = RS_ROUND, SEL_BS = RS_BS, UNROLL = 4, SUM_UNROLL = 1;
    static constexpr bool LISTED = true, STOPS = false;
    __host__ __device__ static constexpr int stride(int) { return RS_ROUND; }
    __device__ static inline double residual(const double *T, const double *p) { return rs_d2(T, p[0], p[1], p[2], p[3], p[4], p[5]); }
    __device__ static inline void init_model(RsState *st) {
        st->bad_index = 0; st->pad = 0;
        for (int k = 0; k < 12; k++) st->best[k] = (k % 5 == 0) ? 1.0 : 0.0;
    }
    // better-than rule: more inliers, or as many with a strictly smaller RMSE; (bc == 0: the empty start, beaten by any inlier at all)
    __device__ static inline bool better(int c, double e, int bc, double be) {
        if (c <= 0) return false;
        if (c != bc) return c > bc;
        return sqrt(e / (double)c) < sqrt(be / (double)bc);
    }
    __device__ static inline void est_k(RsState &s, int c, int C, int n, double confidence, double log_fail) {
        const double rho = (double)c / (double)C;
        double p = 1.0;
        for (int k = 0; k < n; k++) p *= rho;
        // k' = log(1 - confidence) / log(1 - rho^n), the denominator as log1p(-p): 1 - p rounds to 1 for p below 1e-16 (a handful of inliers
        // at n >= 5), where k' is astronomically large, not -inf.  Only a finite k' >= 0 below est_k shortens the run.
        const double kp = log_fail / log1p(-p);
        if (p > 0.0 && isfinite(kp) && kp >= 0.0 && kp < (double)s.est_k) s.est_k = (long long)ceil(kp);
    }
};

__global__ void __launch_bounds__(RS_BS) k_rs_gather(const float *__restrict__ src, int n_src, const float *__restrict__ tgt, int n_tgt, const float *__restrict__ src_n,
                                                     const float *__restrict__ tgt_n, const int32_t *__restrict__ corres, int C, float4 *__restrict__ ps,
                                                     float4 *__restrict__ pt, float4 *__restrict__ ns, float4 *__restrict__ nt, RsState *st) {
    const int i = blockIdx.x * RS_BS + threadIdx.x;
    if (i >= C) return;
    int a = corres[2 * (size_t)i], b = corres[2 * (size_t)i + 1];
    if (a < 0 || a >= n_src || b < 0 || b >= n_tgt) { atomicOr(&st->bad_index, 1); a = 0; b = 0; }
    ps[i] = make_float4(src[3 * (size_t)a], src[3 * (size_t)a + 1], src[3 * (size_t)a + 2], 0.f);
    pt[i] = make_float4(tgt[3 * (size_t)b], tgt[3 * (size_t)b + 1], tgt[3 * (size_t)b + 2], 0.f);
    if (ns) {
        ns[i] = make_float4(src_n[3 * (size_t)a], src_n[3 * (size_t)a + 1], src_n[3 * (size_t)a + 2], 0.f);
        nt[i] = make_float4(tgt_n[3 * (size_t)b], tgt_n[3 * (size_t)b + 1], tgt_n[3 * (size_t)b + 2], 0.f);
    }
}

template <int N> __global__ void __launch_bounds__(RS_BS) k_rs_hypo(RsArgs a) {
    const int h = blockIdx.x * RS_BS + threadIdx.x;
    if (h >= a.count) return;
    if (a.st && a.st->stop) return;
    const uint64_t i = (uint64_t)a.first + (uint64_t)h;
    int r[N]; float s[N][3], t[N][3];
#pragma unroll
    for (int k = 0; k < N; k++) {
        r[k] = (int)(pcr_splitmix64(a.seed + (uint64_t)N * i + (uint64_t)k) % (uint64_t)a.C);
        const float4 p = a.ps[r[k]], q = a.pt[r[k]];
        s[k][0] = p.x; s[k][1] = p.y; s[k][2] = p.z; t[k][0] = q.x; t[k][1] = q.y; t[k][2] = q.z;
    }
    bool ok = true;
    if (a.edge_thr >= 0.0) {         // CorrespondenceCheckerBasedOnEdgeLength: every pair of the sample
#pragma unroll
        for (int u = 0; u < N; u++)
#pragma unroll
            for (int v = u + 1; v < N; v++) {
                const double sx = (double)s[u][0] - (double)s[v][0], sy = (double)s[u][1] - (double)s[v][1], sz = (double)s[u][2] - (double)s[v][2];
                const double tx = (double)t[u][0] - (double)t[v][0], ty = (double)t[u][1] - (double)t[v][1], tz = (double)t[u][2] - (double)t[v][2];
                const double ls = sqrt(sx * sx + sy * sy + sz * sz), lt = sqrt(tx * tx + ty * ty + tz * tz);
                if (ls < lt * a.edge_thr || lt < ls * a.edge_thr) ok = false;
            }
    }
    double U[16];
#pragma unroll
    for (int k = 0; k < 16; k++) U[k] = 0.0;
    if (ok) {
        const double o[3] = {(double)t[0][0], (double)t[0][1], (double)t[0][2]};      // moments about the first sampled target point
        double M[16];
#pragma unroll
        for (int k = 0; k < 16; k++) M[k] = 0.0;
#pragma unroll
        for (int k = 0; k < N; k++) {
            const double u[3] = {(double)s[k][0] - o[0], (double)s[k][1] - o[1], (double)s[k][2] - o[2]};
            const double v[3] = {(double)t[k][0] - o[0], (double)t[k][1] - o[1], (double)t[k][2] - o[2]};
#pragma unroll
            for (int d = 0; d < 3; d++) {
                M[d] += u[d]; M[3 + d] += v[d];
#pragma unroll
                for (int e = 0; e < 3; e++) M[6 + 3 * d + e] += v[d] * u[e];
            }
            M[15] += u[0] * u[0] + u[1] * u[1] + u[2] * u[2];
        }
        icp_umeyama(M, (double)N, o, a.with_scaling != 0, U);
#pragma unroll
        for (int k = 0; k < 12; k++) if (!isfinite(U[k])) ok = false;
        if (ok && a.dist_thr2 >= 0.0) {      // CorrespondenceCheckerBasedOnDistance
#pragma unroll
            for (int k = 0; k < N; k++)
                if (rs_d2(U, s[k][0], s[k][1], s[k][2], t[k][0], t[k][1], t[k][2]) > a.dist_thr2) ok = false;
        }
        if (ok && a.ns) {                    // CorrespondenceCheckerBasedOnNormal: the 3x3 block of T as it is (c R under with_scaling, as Open3D)
#pragma unroll
            for (int k = 0; k < N; k++) {
                const float4 p = a.ns[r[k]], q = a.nt[r[k]];
                const double nx = U[0] * p.x + U[1] * p.y + U[2] * p.z, ny = U[4] * p.x + U[5] * p.y + U[6] * p.z, nz = U[8] * p.x + U[9] * p.y + U[10] * p.z;
                if (nx * q.x + ny * q.y + nz * q.z < a.cos_thr) ok = false;
            }
        }
    }
    a.valid[h] = ok ? 1 : 0;
    a.cnt[h] = ok ? 0 : -1;
    a.err2[h] = 0.0;
#pragma unroll
    for (int k = 0; k < 12; k++) a.T[(size_t)h * 12 + k] = U[k];
    if (ok) a.list[atomicAdd(a.n_list, 1)] = h;
}

// the inlier rows of the winner, by the expression that counted them
__global__ void __launch_bounds__(RS_BS) k_rs_inlier_flags(const float4 *__restrict__ ps, const float4 *__restrict__ pt, int C, const RsState *__restrict__ st, double d2max,
                                                           uint8_t *__restrict__ flags) {
    const int i = blockIdx.x * RS_BS + threadIdx.x;
    if (i >= C) return;
    double Tm[12];
#pragma unroll
    for (int k = 0; k < 12; k++) Tm[k] = st->best[k];
    const float4 s = ps[i], t = pt[i];
    flags[i] = rs_d2(Tm, s.x, s.y, s.z, t.x, t.y, t.z) < d2max ? 1 : 0;
}
// test hook: what the round left for its hypotheses, copied to the caller's arrays
__global__ void __launch_bounds__(RS_BS) k_rs_dump(const uint8_t *__restrict__ valid, const double *__restrict__ T, const int *__restrict__ cnt, const double *__restrict__ err2, int count,
                                                   uint8_t *__restrict__ valid_out, double *__restrict__ T_out, int32_t *__restrict__ inl_out, double *__restrict__ err2_out) {
    const int h = blockIdx.x * RS_BS + threadIdx.x;
    if (h >= count) return;
    valid_out[h] = valid[h]; inl_out[h] = cnt[h]; err2_out[h] = err2[h];
    for (int k = 0; k < 12; k++) T_out[(size_t)h * 16 + k] = T[(size_t)h * 12 + k];
    T_out[(size_t)h * 16 + 12] = 0; T_out[(size_t)h * 16 + 13] = 0; T_out[(size_t)h * 16 + 14] = 0; T_out[(size_t)h * 16 + 15] = 1;
}

// ------------------------------------------------------------------------------------------------------------------ host
struct RsRun {                     // the device image of one call
    RsArgs a; RsState *st; HypoScore<RsPolicy> s;
};

static size_t rs_scratch_bytes(int64_t C) {
    return (size_t)C * (4 * 16 + 1 + 4 + 8) + (size_t)RS_ROUND * (1 + 12 * 8 + 4 + 8 + 4) + (size_t)RS_MAX_SPLITS * RS_ROUND * 12 + (1u << 20);
}

static int rs_check_params(pcr_context *ctx, const pcr_ransac_params *p, double max_dist) {
    if (!p) return PCR_EINVAL;
    if (!(max_dist > 0.0)) { ctx->err = "max_correspondence_distance <= 0"; return PCR_EINVAL; }
    if (p->ransac_n < 3 || p->ransac_n > 8) { ctx->err = "ransac_n must be in 3..8"; return PCR_EINVAL; }
    if (p->max_iteration < 0) { ctx->err = "max_iteration < 0"; return PCR_EINVAL; }
    if (!(p->confidence > 0.0 && p->confidence <= 1.0)) { ctx->err = "confidence must be in (0, 1]"; return PCR_EINVAL; }
    return PCR_OK;
}

// gathers the rows and lays out the round buffers (scratch from the arena above the current mark; the caller has reserved rs_scratch_bytes)
static int rs_setup(pcr_context *ctx, RsRun &R, const float *src_xyz, const float *src_nrm, int64_t n_src, const float *tgt_xyz, const float *tgt_nrm, int64_t n_tgt,
                    const int32_t *corres, int C, double max_dist, const pcr_ransac_params *p) {
    memset(&R, 0, sizeof R);
    RsArgs &a = R.a;
    const bool normal_check = p->normal_angle_threshold >= 0.0 && src_nrm && tgt_nrm;      // no normals on either cloud: the checker passes (Open3D warns)
    float4 *ps = arena<float4>(ctx, C), *pt = arena<float4>(ctx, C);
    float4 *ns = normal_check ? arena<float4>(ctx, C) : nullptr, *nt = normal_check ? arena<float4>(ctx, C) : nullptr;
    R.st = arena<RsState>(ctx, 1);
    a.valid = arena<uint8_t>(ctx, RS_ROUND); a.T = arena<double>(ctx, (size_t)RS_ROUND * 12); a.cnt = arena<int>(ctx, RS_ROUND); a.err2 = arena<double>(ctx, RS_ROUND);
    a.list = arena<int>(ctx, RS_ROUND); a.n_list = arena<int>(ctx, 1);
    if (!ps || !pt || (normal_check && (!ns || !nt)) || !R.st || !a.valid || !a.T || !a.cnt || !a.err2 || !a.list || !a.n_list) return PCR_ENOMEM;
    PCR_TRY(hypo_score_alloc(ctx, R.s, C, RS_ROUND));
    a.ps = ps; a.pt = pt; a.ns = ns; a.nt = nt; a.C = C; a.with_scaling = p->with_scaling; a.seed = p->seed;
    a.edge_thr = p->edge_length_threshold >= 0.0 ? p->edge_length_threshold : -1.0;
    a.dist_thr2 = p->distance_threshold >= 0.0 ? p->distance_threshold * p->distance_threshold : -1.0;
    a.cos_thr = normal_check ? cos(p->normal_angle_threshold) : -2.0;
    R.s.ra = ps; R.s.rb = pt; R.s.rows = C; R.s.thr = max_dist * max_dist; R.s.model = a.T; R.s.list = a.list; R.s.n_list = a.n_list; R.s.cnt = a.cnt; R.s.err = a.err2;
    PCR_LAUNCH(ctx, k_hypo_init<RsPolicy>, dim3(1), dim3(1), 0, ctx->stream, R.st, (long long)p->max_iteration);
    PCR_LAUNCH(ctx, k_rs_gather, dim3((C + RS_BS - 1) / RS_BS), dim3(RS_BS), 0, ctx->stream, src_xyz, (int)n_src, tgt_xyz, (int)n_tgt, normal_check ? src_nrm : nullptr,
               normal_check ? tgt_nrm : nullptr, corres, C, ps, pt, ns, nt, R.st);
    return PCR_OK;
}

// hypotheses, scores and the per-hypothesis (count, err2) of iterations [first, first + count), count <= RS_ROUND
static int rs_round(pcr_context *ctx, RsRun &R, int n, long long first, int count, bool early_exit) {
    RsArgs a = R.a;
    a.first = first; a.count = count; a.st = early_exit ? R.st : nullptr;
    PCR_HIP_CHECK(ctx, hipMemsetAsync(a.n_list, 0, sizeof(int), ctx->stream));
    PCR_TRY(hypo_dispatch_n(n, [&](auto N) -> int {
        PCR_LAUNCH(ctx, k_rs_hypo<decltype(N)::value>, dim3((count + RS_BS - 1) / RS_BS), dim3(RS_BS), 0, ctx->stream, a);
        return PCR_OK;
    }));
    hypo_score(ctx, R.s, count, nullptr);
    return PCR_OK;
}

static void rs_empty_result(pcr_result *result, pcr_ransac_info *info, int64_t C) {
    memset(result, 0, sizeof *result);
    for (int k = 0; k < 4; k++) result->transformation[5 * k] = 1.0;
    if (info) { info->iterations_run = 0; info->best_iteration = -1; info->n_valid = 0; info->n_corres = C; }
}

// the correspondence form on a device list (scratch reserved by the caller)
static int rs_run(pcr_context *ctx, const float *src_xyz, const float *src_nrm, int64_t n_src, const float *tgt_xyz, const float *tgt_nrm, int64_t n_tgt,
                  const int32_t *corres, int64_t C, double max_dist, const pcr_ransac_params *p, pcr_result *result, int32_t *correspondences, pcr_ransac_info *info) {
    rs_empty_result(result, info, C);
    if (C < p->ransac_n) return PCR_OK;                 // Open3D: too few correspondences, the empty result
    RsRun R;
    PCR_TRY(rs_setup(ctx, R, src_xyz, src_nrm, n_src, tgt_xyz, tgt_nrm, n_tgt, corres, (int)C, max_dist, p));
    RsState h; memset(&h, 0, sizeof h);
    h.best_iter = -1;
    HypoSelectArgs<RsPolicy> sa;
    sa.st = R.st; sa.cnt = R.a.cnt; sa.err = R.a.err2; sa.model = R.a.T; sa.rows = (int)C; sa.n = p->ransac_n; sa.confidence = p->confidence;
    const auto check = [&](const RsState &s) -> int {      // (max_iteration 0: nothing ran; the list is still checked)
        if (s.bad_index) { ctx->err = "correspondence index out of range"; return PCR_EINVAL; }
        return PCR_OK;
    };
    PCR_TRY(hypo_run(ctx, sa, p->max_iteration, h, [&](long long first, int count) { return rs_round(ctx, R, p->ransac_n, first, count, true); }, check));
    if (info) { info->iterations_run = h.iterations_run; info->best_iteration = h.best_iter; info->n_valid = h.n_valid; }
    result->iterations = (int32_t)h.iterations_run;
    if (h.best_iter < 0) return PCR_OK;
    for (int k = 0; k < 12; k++) result->transformation[k] = h.best[k];
    result->fitness = (double)h.best_count / (double)C;
    result->inlier_rmse = sqrt(h.best_err / (double)h.best_count);
    result->n_correspondences = h.best_count;
    result->converged = 1;
    if (correspondences) {
        ArenaMark mark(ctx);
        uint8_t *flags = arena<uint8_t>(ctx, C); int *pos = arena<int>(ctx, C), *total = arena<int>(ctx, 1);
        if (!flags || !pos || !total) return PCR_ENOMEM;
        const dim3 g((unsigned)((C + RS_BS - 1) / RS_BS)), b(RS_BS);
        PCR_LAUNCH(ctx, k_rs_inlier_flags, g, b, 0, ctx->stream, R.a.ps, R.a.pt, (int)C, R.st, R.s.thr, flags);
        PCR_TRY(pcr_dev_flag_scan(ctx, flags, nullptr, (int)C, pos, total));
        PCR_LAUNCH(ctx, k_hypo_emit<>, dim3(hypo_blocks(C)), dim3(HYPO_BS), 0, ctx->stream, corres, flags, pos, (int)C, correspondences);
        int64_t n_in = 0;
        PCR_TRY(pcr_read_count(ctx, total, &n_in));
        if (n_in != h.best_count) { ctx->err = "RANSAC: the inlier pass disagrees with the score of the winner"; return PCR_ENUMERIC; }
    }
    return PCR_OK;
}

static int rs_check_clouds(pcr_context *ctx, const float *src_xyz, int64_t n_src, const float *tgt_xyz, int64_t n_tgt, int64_t C) {
    if (n_src < 0 || n_tgt < 0 || C < 0) return PCR_EINVAL;
    if (n_src > 0x7fffffff / 8 || n_tgt > 0x7fffffff / 8 || C > 0x7fffffff / 8) { ctx->err = "cloud or correspondence list too large"; return PCR_EINVAL; }
    if ((n_src > 0 && !src_xyz) || (n_tgt > 0 && !tgt_xyz)) { ctx->err = "missing cloud"; return PCR_EINVAL; }
    return PCR_OK;
}

extern "C" int pcr_registration_ransac_correspondence(pcr_context *ctx, const float *src_xyz, const float *src_normals, int64_t n_src, const float *tgt_xyz,
                                                      const float *tgt_normals, int64_t n_tgt, const int32_t *corres, int64_t n_corres, double max_distance,
                                                      const pcr_ransac_params *params, pcr_result *result, int32_t *correspondences, pcr_ransac_info *info) {
    return pcr_api_call(ctx, [&]() -> int {
        if (!result) return PCR_EINVAL;
        PCR_TRY(rs_check_params(ctx, params, max_distance));
        PCR_TRY(rs_check_clouds(ctx, src_xyz, n_src, tgt_xyz, n_tgt, n_corres));
        if (n_corres > 0 && (!corres || n_src == 0 || n_tgt == 0)) { ctx->err = "correspondences without a list or without points"; return PCR_EINVAL; }
        PCR_TRY(pcr_arena_reserve(ctx, rs_scratch_bytes(n_corres)));
        return rs_run(ctx, src_xyz, src_normals, n_src, tgt_xyz, tgt_normals, n_tgt, corres, n_corres, max_distance, params, result, correspondences, info);
    });
}

extern "C" int pcr_registration_ransac_feature_matching(pcr_context *ctx, const float *src_xyz, const float *src_normals, int64_t n_src, const float *src_feat33,
                                                        const float *tgt_xyz, const float *tgt_normals, int64_t n_tgt, const float *tgt_feat33, int mutual_filter,
                                                        double max_distance, const pcr_ransac_params *params, pcr_result *result, int32_t *correspondences,
                                                        pcr_ransac_info *info) {
    return pcr_api_call(ctx, [&]() -> int {
        if (!result) return PCR_EINVAL;
        PCR_TRY(rs_check_params(ctx, params, max_distance));
        PCR_TRY(rs_check_clouds(ctx, src_xyz, n_src, tgt_xyz, n_tgt, 0));
        if ((n_src > 0 && !src_feat33) || (n_tgt > 0 && !tgt_feat33)) { ctx->err = "missing features"; return PCR_EINVAL; }
        PCR_TRY(pcr_arena_reserve(ctx, pcr_feature_corres_scratch_bytes(n_src, n_tgt) + rs_scratch_bytes(n_src) + (size_t)(n_src + 1) * 8));
        int32_t *corres = arena<int32_t>(ctx, (size_t)(n_src > 0 ? n_src : 1) * 2);
        if (!corres) return PCR_ENOMEM;
        int64_t C = 0;
        PCR_TRY(pcr_feature_corres(ctx, src_feat33, (int)n_src, tgt_feat33, (int)n_tgt, mutual_filter, params->ransac_n, corres, &C));
        return rs_run(ctx, src_xyz, src_normals, n_src, tgt_xyz, tgt_normals, n_tgt, corres, C, max_distance, params, result, correspondences, info);
    });
}

extern "C" int pcr_debug_ransac_hypotheses(pcr_context *ctx, const float *src_xyz, const float *src_normals, int64_t n_src, const float *tgt_xyz, const float *tgt_normals,
                                           int64_t n_tgt, const int32_t *corres, int64_t n_corres, double max_distance, const pcr_ransac_params *params, int64_t first,
                                           int64_t count, uint8_t *valid_out, double *T_out, int32_t *inliers_out, double *err2_out) {
    return pcr_api_call(ctx, [&]() -> int {
        if (!valid_out || !T_out || !inliers_out || !err2_out || first < 0 || count < 0) return PCR_EINVAL;
        PCR_TRY(rs_check_params(ctx, params, max_distance));
        PCR_TRY(rs_check_clouds(ctx, src_xyz, n_src, tgt_xyz, n_tgt, n_corres));
        if (n_corres < params->ransac_n || !corres || n_src == 0 || n_tgt == 0) { ctx->err = "fewer correspondences than ransac_n"; return PCR_EINVAL; }
        PCR_TRY(pcr_arena_reserve(ctx, rs_scratch_bytes(n_corres)));
        RsRun R;
        PCR_TRY(rs_setup(ctx, R, src_xyz, src_normals, n_src, tgt_xyz, tgt_normals, n_tgt, corres, (int)n_corres, max_distance, params));
        PCR_TRY(hypo_debug_rounds(RS_ROUND, first, count, [&](long long f, int c) { return rs_round(ctx, R, params->ransac_n, f, c, false); }, [&](int64_t done, int c) {
            PCR_LAUNCH(ctx, k_rs_dump, dim3((c + RS_BS - 1) / RS_BS), dim3(RS_BS), 0, ctx->stream, R.a.valid, R.a.T, R.a.cnt, R.a.err2, c, valid_out + done, T_out + done * 16,
                       inliers_out + done, err2_out + done);
        }));
        RsState h;
        PCR_HIP_CHECK(ctx, hipMemcpyAsync(&h, R.st, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
        PCR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        if (h.bad_index) { ctx->err = "correspondence index out of range"; return PCR_EINVAL; }
        return PCR_OK;
    });
}
