// pcr_multiway.hip -- the device half of joint multiway registration (include/pcr_hip.h: pcr_multiway_create, pcr_multiway_linearize): for a
// whole list of graph edges at once, search every source point's correspondence in the edge's target, form the estimator's rows and reduce
// them to the edge's 6x6 system.  The assembly of the joint system, its gauge, the solve and the loop are host float64 (multiway.py).
//
// A problem keeps, per cloud, a search index (pcr_search.hip: the Morton-sorted cloud with its octree, every point tagged with its caller row)
// and a copy of the normals in caller order, in device memory of its own.  One call is two launches:
//   k_mw_tiles<MODE>   one workgroup per (edge, tile) of a flat work list; a tile is MW_TILE consecutive points of the SOURCE index's own Morton
//                      order, so neighbouring octets walk neighbouring leaves of the target.  Phase 1: 32 octets x 8 rounds, one query per octet,
//                      the bottom-up walk of the exact 1-NN search (k_index_knn<1, HYBRID, ONE> restated: one k-best place, the same screen, key
//                      and tie order), the match's place in the target left in LDS.  Phase 2: one source point per lane forms its rows in
//                      float64 and the workgroup reduces them in a fixed order (DPP inside the 16-lane rows, then the 16 rows in order: the
//                      reduction of k_corr_rows) to ONE partial row per tile.
//   k_mw_sum           one workgroup per edge adds the edge's partial rows in ascending tile order.
// No state is handed from one launch to the next and no workgroup waits for another: no ticket, no counter, no spin; the kernel boundary is all
// the ordering there is, and every loop is bounded by a count.  The order of an edge's sum depends on its two clouds and MW_TILE only.
#include <cmath>
#include <cstring>
#include <vector>
#include "pcr_vgicp.h"
#include "pcr_solve6.h"

#define MW_BS 256
#define MW_TILE PCR_MULTIWAY_TILE
#define MW_NV 31                 // 21 JTJ (upper triangle) + 6 JTr + sum r^2, sum w r^2, sum d^2, rows
#define MW_NVP 32                // doubles per partial row
#define MW_EMPTY_K 0xffffffffffffffffull
#define MW_EMPTY_I 0x7fffffff
static_assert(MW_TILE == MW_BS, "phase 2 takes one source point per lane");
enum { MW_P2P = 0, MW_P2PL = 1, MW_GICP = 2 };

struct MwCloud { OctView t; const float *nrm; int n; };
struct MwEdge { double M[12]; long long match_off; int a, b, first, tiles; };
struct MwArgs {
    const MwCloud *clouds; const MwEdge *edges; const int2 *items;       // items[w] = (edge, tile)
    double *partials; int32_t *match;
    int loss; double loss_k, a, r2; float r2f;                           // a = 1 - epsilon (GICP)
};

struct pcr_multiway {
    int device = 0;
    std::vector<pcr_index *> index;
    std::vector<int64_t> n;
    std::vector<const float *> nrm;      // into `block`, or null
    char *block = nullptr;               // the one allocation of the problem's own: the cloud table, then the normals
    MwCloud *clouds = nullptr;
};

__device__ static inline bool mw_lt(unsigned long long ak, int ai, unsigned long long bk, int bi) { return ak < bk || (ak == bk && ai < bi); }
template <int CTRL> __device__ static inline unsigned long long mw_dpp_u64(unsigned long long v) {
    const unsigned lo = (unsigned)pcr_dpp_i<CTRL>((int)(unsigned)v), hi = (unsigned)pcr_dpp_i<CTRL>((int)(unsigned)(v >> 32));
    return ((unsigned long long)hi << 32) | lo;
}
// smallest (key, caller index) of the octet with its place in the sorted cloud, in all 8 lanes
template <int CTRL> __device__ static inline void mw_min_step(unsigned long long &k, int &i, int &p) {
    const unsigned long long o = mw_dpp_u64<CTRL>(k); const int oi = pcr_dpp_i<CTRL>(i), op = pcr_dpp_i<CTRL>(p);
    if (mw_lt(o, oi, k, i)) { k = o; i = oi; p = op; }
}

__device__ static inline void mw_row6(double w, const double *J, double r, double *acc) {
    int t = 0;
#pragma unroll
    for (int p = 0; p < 6; p++) {
        const double wj = w * J[p];
#pragma unroll
        for (int q = p; q < 6; q++) acc[t++] += wj * J[q];
        acc[21 + p] += wj * r;
    }
    acc[27] += r * r;
    acc[28] += w * (r * r);
}

// the rows of one match: s = the source point at the edge's pose (float64), tp = the matched target point, ci / mi = their caller rows
template <int MODE>
__device__ static inline void mw_rows(const MwArgs &a, const double *T, double sx, double sy, double sz, const float4 tp, int ci, int mi, const float *src_nrm,
                                      const float *tgt_nrm, double *acc) {
    const double dx = sx - (double)tp.x, dy = sy - (double)tp.y, dz = sz - (double)tp.z;
    if (MODE == MW_P2PL) {
        const float *np_ = tgt_nrm + (size_t)mi * 3;
        const double nx = np_[0], ny = np_[1], nz = np_[2];
        const double r = nx * dx + ny * dy + nz * dz;
        const double J[6] = {sy * nz - sz * ny, sz * nx - sx * nz, sx * ny - sy * nx, nx, ny, nz};
        mw_row6(icp_weight(a.loss, a.loss_k, r), J, r, acc);
        return;
    }
    double W[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if (MODE == MW_GICP) {
        // icp_point<ICP_MODE_GICP> (pcr_gicp.hip): C = I - a m m^T, m the normalised normal, e1 when n.x < -0.99; the source normal turned by R
        const float *sn = src_nrm + (size_t)ci * 3, *tn = tgt_nrm + (size_t)mi * 3;
        double ax = sn[0], ay = sn[1], az = sn[2], vx = tn[0], vy = tn[1], vz = tn[2];
        if (ax < -0.99) { ax = 1; ay = 0; az = 0; }
        if (vx < -0.99) { vx = 1; vy = 0; vz = 0; }
        double inv = 1.0 / sqrt(ax * ax + ay * ay + az * az);
        ax *= inv; ay *= inv; az *= inv;
        inv = 1.0 / sqrt(vx * vx + vy * vy + vz * vz);
        vx *= inv; vy *= inv; vz *= inv;
        const double ux = T[0] * ax + T[1] * ay + T[2] * az, uy = T[4] * ax + T[5] * ay + T[6] * az, uz = T[8] * ax + T[9] * ay + T[10] * az;
        const double c = ux * vx + uy * vy + uz * vz;
        // M = 2I - a(uu^T + vv^T): eigenpairs (2 - a(1+c), u+v), (2 - a(1-c), u-v), (2, u x v)
        const double SQ2 = 1.4142135623730951;
        const double lp = 2.0 - a.a * (1.0 + c), lm = 2.0 - a.a * (1.0 - c);
        const double slp = sqrt(lp), slm = sqrt(lm);
        const double gp = a.a / (2.0 * SQ2 * slp * (SQ2 + slp)), gm = a.a / (2.0 * SQ2 * slm * (SQ2 + slm));
        const double ex = ux + vx, ey = uy + vy, ez = uz + vz, fx = ux - vx, fy = uy - vy, fz = uz - vz;
        const double w0 = 1.0 / SQ2;
        W[0] = w0 + gp * ex * ex + gm * fx * fx; W[1] = gp * ex * ey + gm * fx * fy; W[2] = gp * ex * ez + gm * fx * fz;
        W[4] = w0 + gp * ey * ey + gm * fy * fy; W[5] = gp * ey * ez + gm * fy * fz; W[8] = w0 + gp * ez * ez + gm * fz * fz;
        W[3] = W[1]; W[6] = W[2]; W[7] = W[5];
    }
#pragma unroll
    for (int row = 0; row < 3; row++) {
        const double wx = W[row * 3], wy = W[row * 3 + 1], wz = W[row * 3 + 2];
        const double J[6] = {sy * wz - sz * wy, sz * wx - sx * wz, sx * wy - sy * wx, wx, wy, wz};      // s x W_row, W_row  (W = I: -skew(s) | I)
        const double r = wx * dx + wy * dy + wz * dz;
        mw_row6(MODE == MW_GICP ? icp_weight(a.loss, a.loss_k, r) : 1.0, J, r, acc);
    }
}

template <int MODE>
__global__ void __launch_bounds__(MW_BS) k_mw_tiles(MwArgs a) {
    constexpr int OPB = MW_BS / OCT;
    __shared__ OctMeta m;
    __shared__ OctStack<OPB> stk;
    __shared__ unsigned long long s_key[MW_TILE];        // per source point of the tile: the bits of the match's d^2 ...
    __shared__ int s_pos[MW_TILE];                       // ... and its place in the target's sorted cloud, -1: none
    __shared__ double red[MW_BS / 16][MW_NVP];
    const int2 it = a.items[blockIdx.x];
    const MwEdge *e = a.edges + it.x;
    const MwCloud src = a.clouds[e->a], tgt = a.clouds[e->b];
    double T[12];
#pragma unroll
    for (int k = 0; k < 12; k++) T[k] = e->M[k];
    if (threadIdx.x == 0 && tgt.n > 0) m = *tgt.t.meta;
    s_pos[threadIdx.x] = -1; s_key[threadIdx.x] = 0ull;
    __syncthreads();
    const int lane = threadIdx.x & 63, oct = lane >> 3, ol = lane & 7, ob = threadIdx.x >> 3;
    const int base = it.y * MW_TILE;

    // ---- phase 1: the correspondences, one query per octet and round
    for (int rd = 0; rd < MW_TILE / OPB; rd++) {
        const int slot = base + rd * OPB + ob;
        const bool inr = slot < src.n;
        if (__ballot(inr) == 0ull) break;                       // (slots ascend: the wavefront's later rounds are empty too)
        const float4 p = src.t.pts[inr ? slot : 0];
        double qx, qy, qz;
        vg_transform(T, p.x, p.y, p.z, qx, qy, qz);
        const float4 q = make_float4((float)qx, (float)qy, (float)qz, 0.0f);
        // a query with a non-finite coordinate finds nothing; neither does any query in an empty target
        const bool live = inr && tgt.n >= 1 && fabsf(q.x) <= 3.4028235e38f && fabsf(q.y) <= 3.4028235e38f && fabsf(q.z) <= 3.4028235e38f && m.nl >= 1 && m.n >= 1;
        if (__ballot(live) == 0ull) continue;
        int node = 0, s_first = 0, s_count = 0, s_parent = 0, s_sib = 0, s_nsib = 1; uint64_t s_k = 0;
        const int g = oct_greedy_leaf(tgt.t, m, live, q.x, q.y, q.z, ol);
        if (live) {
            node = g;
            const size_t j = (size_t)(m.off[0] + g);
            s_first = __float_as_int(tgt.t.nodes[2 * j].w); s_count = __float_as_int(tgt.t.nodes[2 * j + 1].w);
            const int4 u = tgt.t.up[j]; s_k = tgt.t.keys[s_first];
            s_parent = u.x; s_sib = u.y; s_nsib = u.z;
        }
        unsigned long long wk = MW_EMPTY_K; int wi = MW_EMPTY_I, wp = -1;      // the octet's best (octet-uniform)
        float bnd = a.r2f;
        auto visit = [&](int first, int count) {                 // wave-wide; count == 0: octet idle
            int b0 = first; const int end = first + count;
            unsigned long long mk = MW_EMPTY_K; int mi = MW_EMPTY_I, mp = -1;   // the best candidate this lane tested in the range
            while (__ballot(b0 < end) != 0ull) {
                float4 pp[4];
#pragma unroll
                for (int u = 0; u < 4; u++) { const int idx = b0 + OCT * u + ol; pp[u] = tgt.t.pts[idx < end ? idx : (end > first ? end - 1 : 0)]; }
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int idx = b0 + OCT * u + ol;
                    if (idx < end && pcr_d2(pp[u].x - q.x, pp[u].y - q.y, pp[u].z - q.z) < bnd) {
                        const double d = pcr_d2_f64_unfused(q, pp[u]);
                        if (d < a.r2) {
                            const unsigned long long ck = (unsigned long long)__double_as_longlong(d); const int ci = __float_as_int(pp[u].w);
                            if (mw_lt(ck, ci, wk, wi) && mw_lt(ck, ci, mk, mi)) { mk = ck; mi = ci; mp = idx; }
                        }
                    }
                }
                b0 += 4 * OCT;
            }
            mw_min_step<PCR_DPP_XOR1>(mk, mi, mp); mw_min_step<PCR_DPP_XOR2>(mk, mi, mp); mw_min_step<PCR_DPP_HMIRROR>(mk, mi, mp);
            if (mw_lt(mk, mi, wk, wi)) {
                wk = mk; wi = mi; wp = mp;
                // the float32 bound of the walk: the wide float of the best key, never below the smallest normal float, never above the cap
                bnd = fminf(fmaxf((float)(__longlong_as_double((long long)wk) * (1.0 + 1e-6)), 1.17549435e-38f), a.r2f);
            }
        };
        oct_search<OPB>(tgt.t, m, stk, live, node, 0, s_first, s_count, s_k, s_parent, s_sib, s_nsib, q.x, q.y, q.z,
                        [&]() { return bnd; }, visit, [](int, int) { return false; }, ol, oct, ob);
        if (ol == 0 && inr && wk != MW_EMPTY_K) { s_pos[rd * OPB + ob] = wp; s_key[rd * OPB + ob] = wk; }
    }
    __syncthreads();

    // ---- phase 2: one source point per lane, its rows in float64
    double acc[MW_NV];
#pragma unroll
    for (int k = 0; k < MW_NV; k++) acc[k] = 0.0;
    {
        const int slot = base + (int)threadIdx.x;
        if (slot < src.n) {
            const float4 p = src.t.pts[slot];
            const int ci = __float_as_int(p.w), pos = s_pos[threadIdx.x];
            int mi = -1;
            if (pos >= 0) {
                const float4 tp = tgt.t.pts[pos];
                mi = __float_as_int(tp.w);
                double sx, sy, sz;
                vg_transform(T, p.x, p.y, p.z, sx, sy, sz);
                mw_rows<MODE>(a, T, sx, sy, sz, tp, ci, mi, src.nrm, tgt.nrm, acc);
                acc[29] += __longlong_as_double((long long)s_key[threadIdx.x]);
                acc[30] += 1.0;
            }
            if (a.match) a.match[e->match_off + ci] = mi;
        }
    }
    // every lane of the workgroup is here (lanes without a row hold zeros): DPP butterfly inside every 16-lane row, then the rows in order
    const int r16 = lane & 15, row = threadIdx.x >> 4;
    double lo, hi;
    pcr_row16_sum_halving<MW_NV>(acc, lane, &lo, &hi);
    red[row][r16] = lo;
    if (16 + r16 < MW_NV) red[row][16 + r16] = hi;
    __syncthreads();
    if (threadIdx.x < MW_NVP) {
        double s = 0.0;
        if ((int)threadIdx.x < MW_NV) {
            s = red[0][threadIdx.x];
#pragma unroll
            for (int w = 1; w < MW_BS / 16; w++) s += red[w][threadIdx.x];
        }
        a.partials[(size_t)blockIdx.x * MW_NVP + threadIdx.x] = s;
    }
}

// the partial rows of every edge in ascending tile order
__global__ void __launch_bounds__(64) k_mw_sum(const MwEdge *__restrict__ edges, const double *__restrict__ partials, double *__restrict__ out) {
    if (threadIdx.x >= MW_NVP) return;
    const MwEdge *e = edges + blockIdx.x;
    const double *p = partials + (size_t)e->first * MW_NVP + threadIdx.x;
    const int tiles = e->tiles;
    double s = 0.0;
#pragma unroll 8
    for (int t = 0; t < tiles; t++) s += p[(size_t)t * MW_NVP];
    out[(size_t)blockIdx.x * MW_NVP + threadIdx.x] = s;
}

// ====================================================================================================== C ABI
extern "C" int pcr_multiway_destroy(pcr_multiway *problem) {
    if (!problem) return PCR_OK;
    int rc = PCR_OK;
    for (pcr_index *ix : problem->index)
        if (pcr_index_destroy(ix) != PCR_OK) rc = PCR_EHIP;
    if (problem->block) {
        if (hipSetDevice(problem->device) != hipSuccess) rc = PCR_EHIP;
        else (void)hipFree(problem->block);                   // waits for the device: no linearisation is still reading the block
    }
    delete problem;
    return rc;
}

extern "C" int pcr_multiway_create(pcr_context *ctx, int n_clouds, const float *const *xyz, const float *const *normals, const int64_t *n, pcr_multiway **problem) {
    if (!ctx) return PCR_EINVAL;
    if (!problem || n_clouds < 0 || (n_clouds > 0 && (!xyz || !n))) {
        return pcr_api_call(ctx, [&]() -> int { ctx->err = "multiway_create: bad cloud count, cloud table or output pointer"; return PCR_EINVAL; });
    }
    *problem = nullptr;
    for (int i = 0; i < n_clouds; i++)
        if (n[i] < 0 || (n[i] > 0 && !xyz[i])) {
            return pcr_api_call(ctx, [&]() -> int { ctx->err = "multiway_create: cloud " + std::to_string(i) + " has a negative count or no points"; return PCR_EINVAL; });
        }
    pcr_multiway *mw = new pcr_multiway();
    mw->device = ctx->device;
    for (int i = 0; i < n_clouds; i++) {                      // (every index is a call of its own: built and finished when it returns)
        pcr_index *ix = nullptr;
        const int rc = pcr_index_create(ctx, xyz[i], n[i], &ix);
        if (rc != PCR_OK) { (void)pcr_multiway_destroy(mw); return rc; }
        mw->index.push_back(ix); mw->n.push_back(n[i]);
    }
    const int rc = pcr_api_call(ctx, [&]() -> int {
        const size_t table = ((size_t)(n_clouds > 0 ? n_clouds : 1) * sizeof(MwCloud) + 255) & ~(size_t)255;
        size_t bytes = table;
        std::vector<size_t> off((size_t)n_clouds, 0);
        for (int i = 0; i < n_clouds; i++)
            if (normals && normals[i] && n[i] > 0) { off[i] = bytes; bytes += ((size_t)n[i] * 3 * sizeof(float) + 255) & ~(size_t)255; }
        if (hipMalloc((void **)&mw->block, bytes) != hipSuccess) { mw->block = nullptr; ctx->err = "hipMalloc(multiway problem)"; return PCR_ENOMEM; }
        mw->clouds = (MwCloud *)mw->block;
        std::vector<MwCloud> host((size_t)(n_clouds > 0 ? n_clouds : 1));
        std::memset(host.data(), 0, host.size() * sizeof(MwCloud));
        for (int i = 0; i < n_clouds; i++) {
            const float *nd = nullptr;
            if (off[i]) {
                nd = (const float *)(mw->block + off[i]);
                PCR_HIP_CHECK(ctx, hipMemcpyAsync((void *)nd, normals[i], (size_t)n[i] * 3 * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
            }
            mw->nrm.push_back(nd);
            int64_t cnt = 0;
            const DevCloud *c = pcr_index_cloud(mw->index[i], nullptr, &cnt);
            if (cnt > 0) host[i].t = oct_view(c);
            host[i].nrm = nd; host[i].n = (int)cnt;
        }
        PCR_HIP_CHECK(ctx, hipMemcpyAsync(mw->clouds, host.data(), host.size() * sizeof(MwCloud), hipMemcpyHostToDevice, ctx->stream));
        // finished before the call returns: the caller may free its arrays, and any context of the device may linearise
        PCR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        return PCR_OK;
    });
    if (rc != PCR_OK) { (void)pcr_multiway_destroy(mw); return rc; }
    *problem = mw;
    return PCR_OK;
}

template <int MODE>
static void mw_launch(pcr_context *ctx, const MwArgs &a, int64_t tiles) {
    PCR_LAUNCH(ctx, k_mw_tiles<MODE>, dim3((unsigned)tiles), dim3(MW_BS), 0, ctx->stream, a);
}

extern "C" int pcr_multiway_linearize(pcr_context *ctx, const pcr_multiway *problem, const int32_t *edges2, int64_t E, const double *M,
                                      double max_correspondence_distance, const pcr_estimation *estimation, double *JTJ, double *JTr, double *stats,
                                      int64_t *rows, int32_t *match) {
    return pcr_api_call(ctx, [&]() -> int {
        const char *fn = "multiway_linearize: ";
        if (!problem) { ctx->err = std::string(fn) + "problem is null"; return PCR_EINVAL; }
        if (problem->device != ctx->device) { ctx->err = std::string(fn) + "the problem lives on another device than the context"; return PCR_EINVAL; }
        if (E < 0 || E > 0x7fffffffLL / MW_NVP) { ctx->err = std::string(fn) + "edges: the count is negative or too large"; return PCR_EINVAL; }
        if (!estimation) { ctx->err = std::string(fn) + "estimation is null"; return PCR_EINVAL; }
        const pcr_estimation &est = *estimation;
        if (est.kind < PCR_EST_POINT_TO_POINT || est.kind > PCR_EST_GENERALIZED_ICP) { ctx->err = std::string(fn) + "estimation: unknown kind (pcr_estimation_kind)"; return PCR_EINVAL; }
        if (est.kind != PCR_EST_POINT_TO_POINT && (est.loss < PCR_LOSS_L2 || est.loss > PCR_LOSS_GM)) { ctx->err = std::string(fn) + "estimation: unknown loss (pcr_loss_kind)"; return PCR_EINVAL; }
        if (est.kind == PCR_EST_POINT_TO_POINT && est.with_scaling != 0) { ctx->err = std::string(fn) + "estimation: with_scaling has no joint form"; return PCR_EINVAL; }
        if (est.kind != PCR_EST_POINT_TO_POINT && !std::isfinite(est.loss_k)) { ctx->err = std::string(fn) + "estimation: loss_k is not finite"; return PCR_EINVAL; }
        if (est.kind == PCR_EST_GENERALIZED_ICP && !std::isfinite(est.epsilon)) { ctx->err = std::string(fn) + "estimation: epsilon is not finite"; return PCR_EINVAL; }
        if (!std::isfinite(max_correspondence_distance) || !(max_correspondence_distance > 0.0)) {
            ctx->err = std::string(fn) + "max_correspondence_distance must be finite and > 0"; return PCR_EINVAL;
        }
        if (E == 0) return PCR_OK;
        if (!edges2 || !M || !JTJ || !JTr || !stats || !rows) { ctx->err = std::string(fn) + "null edges, M or output pointer"; return PCR_EINVAL; }
        const int nc = (int)problem->index.size();
        std::vector<MwEdge> edges((size_t)E);
        int64_t tiles = 0, points = 0;
        for (int64_t k = 0; k < E; k++) {
            const int a = edges2[2 * k], b = edges2[2 * k + 1];
            if (a < 0 || a >= nc || b < 0 || b >= nc) {
                ctx->err = std::string(fn) + "edges: row " + std::to_string((long long)k) + " (" + std::to_string(a) + ", " + std::to_string(b) + ") names a cloud outside 0.." + std::to_string(nc - 1);
                return PCR_EINVAL;
            }
            if (a == b) { ctx->err = std::string(fn) + "edges: row " + std::to_string((long long)k) + " joins cloud " + std::to_string(a) + " to itself"; return PCR_EINVAL; }
            for (int j = 0; j < 16; j++)
                if (!std::isfinite(M[16 * k + j])) { ctx->err = std::string(fn) + "M: the pose of edge " + std::to_string((long long)k) + " has a non-finite entry"; return PCR_EINVAL; }
            // (an empty cloud has no rows to miss a normal)
            const int need[2] = {est.kind == PCR_EST_GENERALIZED_ICP ? a : -1, est.kind != PCR_EST_POINT_TO_POINT ? b : -1};
            for (int c : need)
                if (c >= 0 && problem->n[c] > 0 && !problem->nrm[c]) {
                    ctx->err = std::string(fn) + "normals: the estimator needs the normals of cloud " + std::to_string(c) + ", which carries none (edge " + std::to_string((long long)k) + ")";
                    return PCR_EINVAL;
                }
            MwEdge &e = edges[k];
            std::memcpy(e.M, M + 16 * k, sizeof e.M);
            e.a = a; e.b = b; e.match_off = points;
            const int64_t nt = (problem->n[a] + MW_TILE - 1) / MW_TILE;
            e.first = (int)tiles; e.tiles = (int)nt;
            tiles += nt; points += problem->n[a];
            if (tiles > 0x7fffffffLL / MW_NVP) { ctx->err = std::string(fn) + "edges: too many source points in one call"; return PCR_EINVAL; }
        }
        std::vector<int2> items((size_t)tiles);
        for (int64_t k = 0; k < E; k++)
            for (int t = 0; t < edges[k].tiles; t++) items[(size_t)edges[k].first + t] = make_int2((int)k, t);
        const size_t b_edges = (size_t)E * sizeof(MwEdge), b_items = (size_t)tiles * sizeof(int2), b_part = (size_t)tiles * MW_NVP * sizeof(double),
                     b_out = (size_t)E * MW_NVP * sizeof(double);
        PCR_TRY(pcr_arena_reserve(ctx, b_edges + b_items + b_part + b_out + 8 * 256));
        MwEdge *d_edges = (MwEdge *)pcr_arena_alloc(ctx, b_edges);
        int2 *d_items = (int2 *)pcr_arena_alloc(ctx, b_items > 0 ? b_items : 8);
        double *d_part = (double *)pcr_arena_alloc(ctx, b_part > 0 ? b_part : 8);
        double *d_out = (double *)pcr_arena_alloc(ctx, b_out);
        if (!d_edges || !d_items || !d_part || !d_out) return PCR_ENOMEM;
        PCR_HIP_CHECK(ctx, hipMemcpyAsync(d_edges, edges.data(), b_edges, hipMemcpyHostToDevice, ctx->stream));
        if (tiles > 0) PCR_HIP_CHECK(ctx, hipMemcpyAsync(d_items, items.data(), b_items, hipMemcpyHostToDevice, ctx->stream));
        MwArgs a; std::memset(&a, 0, sizeof a);
        a.clouds = problem->clouds; a.edges = d_edges; a.items = d_items; a.partials = d_part; a.match = match;
        a.loss = est.loss; a.loss_k = est.loss_k; a.a = 1.0 - est.epsilon;
        a.r2 = max_correspondence_distance * max_correspondence_distance; a.r2f = pcr_wide_r2f(a.r2);
        if (tiles > 0) {
            if (est.kind == PCR_EST_POINT_TO_POINT) mw_launch<MW_P2P>(ctx, a, tiles);
            else if (est.kind == PCR_EST_POINT_TO_PLANE) mw_launch<MW_P2PL>(ctx, a, tiles);
            else mw_launch<MW_GICP>(ctx, a, tiles);
        }
        PCR_LAUNCH(ctx, k_mw_sum, dim3((unsigned)E), dim3(64), 0, ctx->stream, (const MwEdge *)d_edges, (const double *)d_part, d_out);
        std::vector<double> h((size_t)E * MW_NVP);
        PCR_HIP_CHECK(ctx, hipMemcpyAsync(h.data(), d_out, b_out, hipMemcpyDeviceToHost, ctx->stream));
        PCR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        for (int64_t k = 0; k < E; k++) {
            const double *s = h.data() + (size_t)k * MW_NVP;
            int t = 0;
            for (int p = 0; p < 6; p++)
                for (int q = p; q < 6; q++) { JTJ[36 * k + 6 * p + q] = s[t]; JTJ[36 * k + 6 * q + p] = s[t]; t++; }
            for (int p = 0; p < 6; p++) JTr[6 * k + p] = s[21 + p];
            stats[3 * k] = s[29]; stats[3 * k + 1] = s[27]; stats[3 * k + 2] = s[28];
            rows[k] = (int64_t)s[30];
        }
        return PCR_OK;
    });
}
