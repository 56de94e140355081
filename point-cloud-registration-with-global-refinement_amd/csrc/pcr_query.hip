// pcr_query.hip -- the measuring half of the PointCloud surface on gfx950: nearest-neighbour distances inside a cloud, cloud-to-cloud
// distances, the radius outlier filter and the cloud's mean and covariance.
// Reference behaviour: Open3D PointCloud::{ComputeNearestNeighborDistance, ComputePointCloudDistance, RemoveRadiusOutliers,
// ComputeMeanAndCovariance, GetCenter} as called at ALL_FUNCTIONS.py:1077-1078, :1035, :1043, :1022 (the rules are stated next to the
// entry points in include/pcr_hip.h).  The searches walk the Morton-sorted octree of pcr_octree.h like the k-NN, radius and GICP
// kernels; nothing here touches those kernels.
#include <cstring>
#include <vector>
#include "pcr_octree.h"

#define QRY_BS 256
#define QRY_FAR 3.4e38f

// distance of two float32 points in float64, from the squared distance without fused multiply-adds: the value a host recomputation in the
// same order gives, bit for bit
__device__ static inline double qry_dist_f64(float qx, float qy, float qz, const float4 p) { return sqrt(pcr_d2_f64_unfused(make_float4(qx, qy, qz, 0.0f), p)); }

// ====================================================== nearest-neighbour distance (ComputeNearestNeighborDistance)
// The 2-best search of every point over its own tree: one query per octet, the 8 Morton-consecutive queries of a wavefront share one
// walk (oct_search_group), seeded with the Morton neighbours of the group.  Every lane keeps the two smallest float32 d^2 of the
// candidates IT tested (the point itself is one of them, at 0); the octet's second smallest -- the smallest entry left once the head of
// the lane that holds the octet minimum is taken out -- is the pruning bound and, at the end, the answer.  A point is tested at most
// once per query (seed range and walk are disjoint), so the point itself cannot fill both places.
struct NnDistArgs { OctView t; const uint32_t *perm; double *dist; };
__global__ void __launch_bounds__(QRY_BS) k_nn_distance(NnDistArgs a) {
    oct_group_frame<QRY_BS>(a.t, [&](const OctGroupQuery &g) {
    const int n = g.n, qi = g.qi, ol = g.ol, g0 = g.g0; const bool live = g.live; const float4 q = g.q;
    const int glast = g0 + OCT - 1 < n - 1 ? g0 + OCT - 1 : n - 1;
    const int plo = g0 - OCT < 0 ? 0 : g0 - OCT, phi = glast + OCT > n - 1 ? n - 1 : glast + OCT;
    bool seeding = true;
    float d0 = QRY_FAR, d1 = QRY_FAR; int i0 = -1, i1 = -1;
    float bound = QRY_FAR;                                                      // octet-uniform: second smallest d^2 of the query so far
    // this lane's entry once the head of the lowest lane that holds the octet minimum is taken out: the octet minimum of these is the second smallest
    auto rest_is_second = [&]() {
        const float m0 = pcr_octet_min(d0);
        return ol == pcr_octet_min_i(d0 == m0 ? ol : OCT);
    };
    auto visit = [&](int first, int count) {                                    // wave-uniform range, tested for all 8 queries
        for (int base = first; base < first + count; base += OCT) {
            const int idx = base + ol;
            if (live && idx < first + count && (seeding || idx < plo || idx > phi)) {
                const float4 p = a.t.pts[idx];
                const float d = pcr_d2(p.x - q.x, p.y - q.y, p.z - q.z);
                const bool lt0 = d < d0, lt1 = d < d1;                           // (selects on values: the four entries stay in registers)
                const float nd1 = lt0 ? d0 : (lt1 ? d : d1); const int ni1 = lt0 ? i0 : (lt1 ? idx : i1);
                d0 = lt0 ? d : d0; i0 = lt0 ? idx : i0; d1 = nd1; i1 = ni1;
            }
        }
        const float h0 = d0, h1 = d1;
        bound = pcr_octet_min(rest_is_second() ? h1 : h0);
    };
    visit(plo, phi - plo + 1);
    seeding = false;
    oct_search_group(a.t, g.m, g.stk, live, a.t.leaf_of[g0], q.x, q.y, q.z, [&]() { return bound; }, visit,
                     [&](int f, int c) { return f >= plo && f + c - 1 <= phi; }, ol);
    const bool holder = rest_is_second();
    const float h0 = d0, h1 = d1; const int j0 = i0, j1 = i1;
    const float v = holder ? h1 : h0; const int vi = holder ? j1 : j0;
    const float sec = pcr_octet_min(v);
    const int nb = pcr_octet_min_i((v == sec && vi >= 0) ? vi : 0x7fffffff);     // ties -> lower index
    if (live && ol == 0) a.dist[a.perm[qi]] = nb != 0x7fffffff ? qry_dist_f64(q.x, q.y, q.z, a.t.pts[nb]) : 0.0;
    });
}

int pcr_dev_nn_distance(pcr_context *ctx, const DevCloud *c, const uint32_t *perm, double *dist_caller) {
    if (c->cap <= 0) return PCR_OK;
    NnDistArgs a; a.t = oct_view(c); a.perm = perm; a.dist = dist_caller;
    PCR_LAUNCH(ctx, k_nn_distance, dim3((unsigned)(((size_t)c->cap * OCT + QRY_BS - 1) / QRY_BS)), dim3(QRY_BS), 0, ctx->stream, a);
    return PCR_OK;
}

// ============================================================== cloud-to-cloud distance (ComputePointCloudDistance)
// The queries are another cloud, in the caller's order: one query per octet, each with its own bottom-up walk (oct_search) from its
// greedy leaf -- the unbounded form of the GICP correspondence search (pcr_gicp.hip, oct_nn_query), pruned with the best float32 d^2.
// The greedy leaf gives a finite bound before the first climb, so a query far outside the target's box ends too.
struct CloudDistArgs { OctView t; const uint32_t *perm; const float *src; int n_src; double *dist; int32_t *nearest; };
__global__ void __launch_bounds__(QRY_BS) k_cloud_distance(CloudDistArgs a) {
    constexpr int OPB = QRY_BS / OCT;
    __shared__ OctMeta m;
    __shared__ OctStack<OPB> stk;
    if (threadIdx.x == 0) m = *a.t.meta;
    __syncthreads();
    const int lane = threadIdx.x & 63, oct = lane >> 3, ol = lane & 7, ob = threadIdx.x >> 3;
    const int i = blockIdx.x * OPB + ob;
    const bool live = i < a.n_src && m.nl >= 1 && m.n >= 1;
    if (__ballot(live) == 0ull) return;
    const size_t ic = live ? (size_t)i : 0;
    const float qx = a.src[ic * 3], qy = a.src[ic * 3 + 1], qz = a.src[ic * 3 + 2];
    int best = -1; float bestd = QRY_FAR;
    auto visit = [&](int first, int count) {                 // wave-wide; count == 0: octet idle
        int base = first; const int end = first + count;
        float d = QRY_FAR; int id = -1;
        while (__ballot(base < end) != 0ull) {
            float4 p[4];
#pragma unroll
            for (int u = 0; u < 4; u++) { const int idx = base + OCT * u + ol; p[u] = a.t.pts[idx < end ? idx : (end > first ? end - 1 : 0)]; }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int idx = base + OCT * u + ol;
                const float du = pcr_d2(p[u].x - qx, p[u].y - qy, p[u].z - qz);
                if (idx < end && du < d) { d = du; id = idx; }          // increasing idx: ties keep the lower index
            }
            base += 4 * OCT;
        }
        const float dmin = pcr_octet_min(d);
        const int cand = pcr_octet_min_i((d == dmin && id >= 0) ? id : 0x7fffffff);
        if (cand != 0x7fffffff && (dmin < bestd || (dmin == bestd && (unsigned)cand < (unsigned)best))) { bestd = dmin; best = cand; }
    };
    int node = 0, s_first = 0, s_count = 0, s_parent = 0, s_sib = 0, s_nsib = 1; uint64_t s_key = 0;
    const int g = oct_greedy_leaf(a.t, m, live, qx, qy, qz, ol);
    if (live) {
        node = g;
        const size_t j = (size_t)(m.off[0] + g);
        s_first = __float_as_int(a.t.nodes[2 * j].w); s_count = __float_as_int(a.t.nodes[2 * j + 1].w);
        const int4 u = a.t.up[j]; s_key = a.t.keys[s_first];
        s_parent = u.x; s_sib = u.y; s_nsib = u.z;
    }
    oct_search<OPB>(a.t, m, stk, live, node, 0, s_first, s_count, s_key, s_parent, s_sib, s_nsib, qx, qy, qz, [&]() { return bestd; }, visit,
                    [](int, int) { return false; }, ol, oct, ob);
    if (live && ol == 0) {
        a.dist[i] = best >= 0 ? qry_dist_f64(qx, qy, qz, a.t.pts[best]) : 0.0;
        if (a.nearest) a.nearest[i] = best >= 0 ? (int32_t)a.perm[best] : -1;
    }
}

static int pcr_dev_cloud_distance(pcr_context *ctx, const float *src_xyz, int64_t n_src, const DevCloud *tgt, const uint32_t *tgt_perm, double *dist, int32_t *nearest) {
    if (n_src <= 0 || tgt->cap <= 0) return PCR_OK;
    CloudDistArgs a; a.t = oct_view(tgt); a.perm = tgt_perm; a.src = src_xyz; a.n_src = (int)n_src; a.dist = dist; a.nearest = nearest;
    PCR_LAUNCH(ctx, k_cloud_distance, dim3((unsigned)(((size_t)n_src * OCT + QRY_BS - 1) / QRY_BS)), dim3(QRY_BS), 0, ctx->stream, a);
    return PCR_OK;
}

// ============================================================================ radius outlier filter (RemoveRadiusOutliers)
// The fixed-radius walk with a counter (the point itself counted).  A query whose count has passed nb_points is finished; the flag goes to
// the caller's row of the mask the flag scan compacts.
struct RadCountArgs { OctView t; const uint32_t *perm; float r2f; double r2; int nb_points; uint8_t *keep; };
__global__ void __launch_bounds__(QRY_BS) k_radius_count(RadCountArgs a) {
    oct_group_frame<QRY_BS>(a.t, [&](const OctGroupQuery &g) {
    int cnt = 0, total = 0;                                   // this lane's count; the octet's (octet-uniform, refreshed after every range)
    // active until the count has passed nb_points: total changes in the per-range step only, as active() must
    oct_ball_walk(a.t, g, a.r2f, [&]() { return g.live && total <= a.nb_points; },
                  [&](int idx) { if (oct_ball_member<false>(g.q, a.t.pts[idx], a.r2f, a.r2)) cnt++; },
                  [&]() { total = pcr_octet_sum_i(cnt); });
    if (g.live && g.ol == 0) a.keep[a.perm[g.qi]] = total > a.nb_points ? 1 : 0;
    });
}

static int pcr_dev_radius_count(pcr_context *ctx, const DevCloud *c, const uint32_t *perm, int nb_points, double radius, uint8_t *keep_caller) {
    if (c->cap <= 0) return PCR_OK;
    RadCountArgs a; a.t = oct_view(c); a.perm = perm; a.r2 = radius * radius; a.r2f = pcr_wide_r2f(a.r2); a.nb_points = nb_points; a.keep = keep_caller;
    PCR_LAUNCH(ctx, k_radius_count, dim3((unsigned)(((size_t)c->cap * OCT + QRY_BS - 1) / QRY_BS)), dim3(QRY_BS), 0, ctx->stream, a);
    return PCR_OK;
}

// ================================================================================ mean and covariance (ComputeMeanAndCovariance)
// Float64 sums of (p - c) and of its six products over the float32 points: wavefront reduction, one slab of 9 sums per workgroup, and a
// one-workgroup launch that adds the slabs in their order.  The grid depends on n alone and every sum has a fixed tree: two runs give
// the same bits.  Pass 1 has c = 0 and gives the mean; pass 2 reads the sums of pass 1 on the device, takes c = that mean and gives the
// CENTRED second moments (SURVEY.md hard part 3: raw second moments of coordinates hundreds of metres from the origin cancel against
// the squared mean).  The host waits once, for both results; the mean alone (get_center) is pass 1.
#define MOM_MAX_BLOCKS 256
__global__ void __launch_bounds__(QRY_BS) k_moments_partial(const float *__restrict__ xyz, int64_t n, const double *__restrict__ centre_sums, double inv_n,
                                                           double *__restrict__ slabs) {
    // c = sum * (1 / n), one rounded product: the value the host forms from the same sums as the mean it returns
    const double cx = centre_sums ? __dmul_rn(centre_sums[0], inv_n) : 0.0, cy = centre_sums ? __dmul_rn(centre_sums[1], inv_n) : 0.0,
                 cz = centre_sums ? __dmul_rn(centre_sums[2], inv_n) : 0.0;
    double s[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int64_t i = blockIdx.x * (int64_t)QRY_BS + threadIdx.x; i < n; i += (int64_t)gridDim.x * QRY_BS) {
        const double x = (double)xyz[i * 3] - cx, y = (double)xyz[i * 3 + 1] - cy, z = (double)xyz[i * 3 + 2] - cz;
        s[0] += x; s[1] += y; s[2] += z;
        s[3] += x * x; s[4] += x * y; s[5] += x * z; s[6] += y * y; s[7] += y * z; s[8] += z * z;
    }
    __shared__ double w[QRY_BS / PCR_WAVE][9];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int t = 0; t < 9; t++) { const double r = pcr_wave_sum(s[t]); if (lane == 0) w[wv][t] = r; }
    __syncthreads();
    if (threadIdx.x < 9) {
        double v = w[0][threadIdx.x];
        for (int k = 1; k < QRY_BS / PCR_WAVE; k++) v += w[k][threadIdx.x];
        slabs[(size_t)blockIdx.x * 9 + threadIdx.x] = v;
    }
}
__global__ void k_moments_final(const double *__restrict__ slabs, int nb, double *__restrict__ out9) {
    if (threadIdx.x < 9) {
        double v = slabs[threadIdx.x];
        for (int k = 1; k < nb; k++) v += slabs[(size_t)k * 9 + threadIdx.x];
        out9[threadIdx.x] = v;
    }
}

// mean3 and (cov9 != nullptr) the population covariance on the host; one synchronisation
static int pcr_dev_mean_and_covariance(pcr_context *ctx, const float *xyz, int64_t n, double *mean3, double *cov9) {
    ArenaMark mark(ctx);
    const int64_t want = (n + QRY_BS - 1) / QRY_BS;
    const int nb = (int)(want < MOM_MAX_BLOCKS ? want : MOM_MAX_BLOCKS);
    const int passes = cov9 ? 2 : 1;
    double *slabs = arena<double>(ctx, (size_t)nb * 9);
    double *out = arena<double>(ctx, 18);                       // sums of pass 1, sums of pass 2
    if (!slabs || !out) return PCR_ENOMEM;
    const double inv = 1.0 / (double)n;
    for (int p = 0; p < passes; p++) {                          // (pass 2 reuses the slabs: the stream orders it after the final launch of pass 1)
        PCR_LAUNCH(ctx, k_moments_partial, dim3(nb), dim3(QRY_BS), 0, ctx->stream, xyz, n, p == 0 ? (const double *)nullptr : (const double *)out, inv, slabs);
        PCR_LAUNCH(ctx, k_moments_final, dim3(1), dim3(64), 0, ctx->stream, slabs, nb, out + 9 * p);
    }
    double s[18];
    PCR_HIP_CHECK(ctx, hipMemcpyAsync(s, out, (size_t)passes * 9 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    PCR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < 3; k++) mean3[k] = s[k] * inv;
    if (!cov9) return PCR_OK;
    const double *c2 = s + 9;
    const double d[3] = {c2[0] * inv, c2[1] * inv, c2[2] * inv};             // what the centre is off the true mean by (rounding of the sums of pass 1)
    const double xx = c2[3] * inv - d[0] * d[0], xy = c2[4] * inv - d[0] * d[1], xz = c2[5] * inv - d[0] * d[2];
    const double yy = c2[6] * inv - d[1] * d[1], yz = c2[7] * inv - d[1] * d[2], zz = c2[8] * inv - d[2] * d[2];
    const double C[9] = {xx, xy, xz, xy, yy, yz, xz, yz, zz};
    for (int k = 0; k < 9; k++) cov9[k] = C[k];
    return PCR_OK;
}

// ====================================================================================================== C ABI
#define QRY_MAX_POINTS 0x7fffffffLL          // the clouds of this library are counted in int

extern "C" int pcr_nearest_neighbor_distance(pcr_context *ctx, const float *xyz, int64_t n, double *dist) {
    return pcr_api_call(ctx, [&]() -> int {
    if (n < 0 || n > QRY_MAX_POINTS || (n > 0 && (!xyz || !dist))) { ctx->err = "nearest_neighbor_distance: bad cloud or output pointer"; return PCR_EINVAL; }
    if (n == 0) return PCR_OK;
    PCR_TRY(pcr_arena_reserve(ctx, pcr_scratch_bytes_for(n) + (size_t)n * 64));
    DevCloud c; uint32_t *perm = nullptr;
    PCR_TRY(pcr_import_cloud(ctx, xyz, nullptr, n, &c, &perm, false));
    return pcr_dev_nn_distance(ctx, &c, perm, dist);            // device output only: asynchronous on the context's stream
    });
}

extern "C" int pcr_point_cloud_distance(pcr_context *ctx, const float *src_xyz, int64_t n_src, const float *tgt_xyz, int64_t n_tgt, double *dist, int32_t *nearest) {
    return pcr_api_call(ctx, [&]() -> int {
    if (n_src < 0 || n_tgt < 0 || n_src > QRY_MAX_POINTS || n_tgt > QRY_MAX_POINTS || (n_src > 0 && (!src_xyz || !dist)) || (n_tgt > 0 && !tgt_xyz)) {
        ctx->err = "point_cloud_distance: bad cloud or output pointer"; return PCR_EINVAL;
    }
    if (n_src == 0) return PCR_OK;
    if (n_tgt == 0) {                                           // Open3D: nothing to measure against, distances 0
        PCR_HIP_CHECK(ctx, hipMemsetAsync(dist, 0, (size_t)n_src * sizeof(double), ctx->stream));
        if (nearest) PCR_HIP_CHECK(ctx, hipMemsetAsync(nearest, 0xff, (size_t)n_src * sizeof(int32_t), ctx->stream));
        return PCR_OK;
    }
    PCR_TRY(pcr_arena_reserve(ctx, pcr_scratch_bytes_for(n_tgt) + (size_t)n_tgt * 64));
    DevCloud t; uint32_t *perm = nullptr;
    PCR_TRY(pcr_import_cloud(ctx, tgt_xyz, nullptr, n_tgt, &t, &perm, false));
    return pcr_dev_cloud_distance(ctx, src_xyz, n_src, &t, perm, dist, nearest);
    });
}

extern "C" int pcr_remove_radius_outlier(pcr_context *ctx, const float *xyz, int64_t n, int nb_points, double radius, uint8_t *keep_mask, float *out_xyz,
                                         int64_t *out_index, int64_t *out_n) {
    return pcr_api_call(ctx, [&]() -> int {
    if (n < 0 || n > QRY_MAX_POINTS || (n > 0 && !xyz)) { ctx->err = "remove_radius_outlier: bad cloud pointer"; return PCR_EINVAL; }
    if (nb_points < 1 || !(radius > 0.0)) { ctx->err = "nb_points < 1 or radius <= 0"; return PCR_EINVAL; }
    if (out_n) *out_n = 0;
    if (n == 0) return PCR_OK;
    PCR_TRY(pcr_arena_reserve(ctx, pcr_scratch_bytes_for(n) + (size_t)n * 64));
    DevCloud c; uint32_t *perm = nullptr;
    PCR_TRY(pcr_import_cloud(ctx, xyz, nullptr, n, &c, &perm, false));
    uint8_t *keep_caller = keep_mask ? keep_mask : arena<uint8_t>(ctx, n);
    if (!keep_caller) return PCR_ENOMEM;
    PCR_TRY(pcr_dev_radius_count(ctx, &c, perm, nb_points, radius, keep_caller));
    return pcr_emit_kept_rows(ctx, xyz, n, keep_caller, out_xyz, out_index, out_n);
    });
}

extern "C" int pcr_mean_and_covariance(pcr_context *ctx, const float *xyz, int64_t n, double *mean3, double *cov9) {
    return pcr_api_call(ctx, [&]() -> int {
    if (n < 0 || !mean3 || (n > 0 && !xyz)) { ctx->err = "mean_and_covariance: bad cloud or output pointer"; return PCR_EINVAL; }
    if (n == 0) {                                               // Open3D: zero mean and the identity
        for (int k = 0; k < 3; k++) mean3[k] = 0.0;
        for (int k = 0; cov9 && k < 9; k++) cov9[k] = (k % 4 == 0) ? 1.0 : 0.0;
        return PCR_OK;
    }
    PCR_TRY(pcr_arena_reserve(ctx, 1 << 20));
    return pcr_dev_mean_and_covariance(ctx, xyz, n, mean3, cov9);
    });
}
