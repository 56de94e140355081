// pcr_cluster.hip -- DBSCAN clustering (Ester et al. 1996) on gfx950.
// Reference behaviour: Open3D PointCloud::ClusterDBSCAN (cpp/open3d/geometry/PointCloudCluster.cpp); the reference scripts do not call it,
// Open3D users put it between the outlier filters and a registration.  The six rules (neighbourhood, core, clusters, numbering, border,
// noise) are stated next to the entry point in include/pcr_hip.h; they fix every label, so the result is Open3D's, not a renaming of it.
// Three kernels are fixed-radius walks of the Morton-sorted octree (oct_group_frame / oct_ball_walk, pcr_octree.h): the core count, the union of the core-core pairs in a lock-free union-find, and the border labels.  Everything between the kernels is
// in SORTED order, next to pts; only the outputs go through perm to the caller's rows.  Nothing here touches the other units' kernels.
#include <cmath>
#include "pcr_octree.h"

#define DBS_BS 256
#define DBS_NONE 0x7fffffff

// Membership of p in the neighbourhood of q is oct_ball_member<true> in all three walks: d^2 < eps^2 (strict) with d^2 formed without fused
// multiply-adds, so that a host recomputation in the order x, y, z gives the same bits and an exact tie d^2 == eps^2 is decided (not a
// member), not left to rounding.

// ============================================================================================================ core points
// The walk at eps with a counter: a query whose count has reached min_points is finished (only "at least min_points" matters).  Writes the
// core flag of the sorted row and sets up the row's union-find entries: parent = itself, smallest caller index of its tree = none yet.
struct DbsCoreArgs { OctView t; float r2f; double r2; int min_points; uint8_t *core; int *parent; int *min_caller; };
__global__ void __launch_bounds__(DBS_BS) k_dbscan_core(DbsCoreArgs a) {
    oct_group_frame<DBS_BS>(a.t, [&](const OctGroupQuery &g) {
    int cnt = 0, total = 0;                                   // this lane's count; the octet's (octet-uniform, refreshed after every range)
    // active until the count has reached min_points: total changes in the per-range step only, as active() must
    oct_ball_walk(a.t, g, a.r2f, [&]() { return g.live && total < a.min_points; },
                  [&](int idx) { if (oct_ball_member<true>(g.q, a.t.pts[idx], a.r2f, a.r2)) cnt++; },
                  [&]() { total = pcr_octet_sum_i(cnt); });
    if (g.live && g.ol == 0) { a.core[g.qi] = total >= a.min_points ? 1 : 0; a.parent[g.qi] = g.qi; a.min_caller[g.qi] = DBS_NONE; }
    });
}

// ============================================================================================= union-find over the core-core pairs
// parent[] is a forest over the sorted rows with ONE invariant: every value ever stored in parent[x] is <= x, and it is x exactly while
// x is a root.  A root is hooked once, by the compare-and-swap below, under a smaller row of a tree it is connected to; afterwards its
// entry only moves to other ancestors (path halving).  So a tree's root is its smallest row, trees only merge, and no cycle can form.
//
// Memory: the lanes of other compute units hook and halve while this lane reads.  A plain load may be served for the whole launch from
// a line this unit's L1 already holds -- a retry after a lost compare-and-swap would then read the same stale "root" for ever -- so
// every load and store of parent[] inside k_dbscan_union is a relaxed agent-scope atomic (L1 bypassed; no fence, no read-modify-write),
// and the hook is an agent-scope atomicCAS.  No ordering between different entries is needed: whatever mix of old and new values a lane
// reads, each is <= its index and names a row of the same tree (trees only merge), which is all the loops below rely on.
//
// TERMINATION (what stands between a bug and a hung device).  No lane waits for another lane, wavefront or workgroup: there is no lock,
// no spin on a value somebody else has to write, no barrier.  dbs_find: x strictly decreases in every iteration (g < p < x) and is
// >= 0, so it ends after at most x steps whatever other lanes do.  dbs_unite: a lost compare-and-swap returns the value found in
// parent[hi], which by the invariant is < hi (hi was hooked by somebody else: only finitely many hooks exist); the lane goes on from
// that value, so ra + rb strictly decreases with every retry and is >= 0: at most a + b retries, again independent of any other lane.
// Both loops compare as unsigned and leave when a value does NOT decrease, so even a parent[] that broke the invariant could not hold
// a lane.
//
// DETERMINISM.  Whatever the interleaving, after the kernel two core rows are in one tree iff a chain of core-core pairs joins them
// (every pair is united by the larger of its two rows; a hook joins only connected trees), and the root of a tree is its smallest row.
// The shape of the trees differs from run to run; k_dbscan_roots reads only the roots.
__device__ static inline int dbs_load(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ static inline void dbs_store(int *p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of x's tree as this lane sees it, halving the path on the way (x's entry is moved to its grandparent)
__device__ static inline int dbs_find(int *parent, int x) {
    for (;;) {
        const int p = dbs_load(parent + x);
        if (!((unsigned)p < (unsigned)x)) return x;           // p == x: a root
        const int g = dbs_load(parent + p);
        if (!((unsigned)g < (unsigned)p)) return p;
        dbs_store(parent + x, g);                             // x is hooked (p < x) and stays so: the store cannot undo a hook
        x = g;
    }
}
// joins the trees of a and b, given pb, a value read from parent[b] (a row of b's tree); returns a row of a's tree that is not larger
// than a (the next union of the same query starts there).  The common case costs no further load: the caller has seen pb == a already,
// or the root of b's tree is a -- the same tree, whether or not a is still a root.
__device__ static inline int dbs_unite(int *parent, int a, int b, int pb) {
    int rb = (unsigned)pb < (unsigned)b ? dbs_find(parent, pb) : b;
    if (rb == a) return a;
    int ra = dbs_find(parent, a);
    while (ra != rb) {
        const int hi = ra > rb ? ra : rb, lo = ra > rb ? rb : ra;
        const int old = atomicCAS(parent + hi, hi, lo);       // hook the larger root under the smaller
        if (old == hi) return lo;
        if (!((unsigned)old < (unsigned)hi)) return a;        // (the invariant excludes it)
        ra = dbs_find(parent, old); rb = dbs_find(parent, lo);   // lost: hi hangs under old < hi now; lo may have been hooked as well
    }
    return ra;
}

// The walk at eps for the CORE queries (a wavefront without one does not walk; a non-core query's bound is 0).  Every member idx < qi that
// is core is united with qi: each core-core pair once, by its larger row.  The eight lanes of a query unite independently, each keeping
// the last root it saw for qi as the starting point of its next find.  Lanes diverge inside the loops and meet again behind them; nothing
// in between needs another lane.
struct DbsUnionArgs { OctView t; float r2f; double r2; const uint8_t *core; int *parent; };
__global__ void __launch_bounds__(DBS_BS) k_dbscan_union(DbsUnionArgs a) {
    oct_group_frame<DBS_BS>(a.t, [&](const OctGroupQuery &g) {
    const int qi = g.qi;
    const bool cq = g.live && a.core[qi] != 0;                // octet-uniform
    if (__ballot(cq) == 0ull) return;
    int from = qi;                                            // a row of qi's tree, <= qi: the last root this lane saw
    // active = cq, fixed for the whole walk
    oct_ball_walk(a.t, g, a.r2f, [&]() { return cq; }, [&](int idx) {
        if (idx < qi) {
            // the three loads are independent and go out together; a row that is not core, or hangs under `from` already, needs no test
            const float4 p = a.t.pts[idx];
            const int c = a.core[idx], pb = dbs_load(a.parent + idx);
            if (c != 0 && pb != from && oct_ball_member<true>(g.q, p, a.r2f, a.r2)) from = dbs_unite(a.parent, from, idx, pb);
        }
    });
    });
}

// ======================================================================================================== roots and numbering
// After the unions (a kernel boundary: every hook is visible, nothing writes parent[] any more): the root of every core row, and per
// root the smallest CALLER index among its core rows -- Open3D seeds a cluster at the first unvisited core point in index order, and the
// smallest-index core point of a component cannot have been reached from an earlier seed.
__global__ void __launch_bounds__(DBS_BS) k_dbscan_roots(const uint8_t *__restrict__ core, const int *__restrict__ parent, const uint32_t *__restrict__ perm, int n,
                                                        int *__restrict__ root, int *min_caller) {
    const int i = blockIdx.x * DBS_BS + threadIdx.x;
    if (i >= n) return;
    int r = -1;
    if (core[i]) {
        r = i;
        for (int p = parent[r]; (unsigned)p < (unsigned)r; p = parent[r]) r = p;
        // the entry only decreases, so a value read earlier is an upper bound: a row that is not below it cannot be the minimum.  Without the
        // look every core row of a large cluster queues at ONE address (measured: 1.6 ms for a cluster of 141,000 rows, 0.36 - 0.61 ms with
        // the look; the rows that read before the first atomics land still queue: DESIGN.md 4.10).
        const int v = (int)perm[i];
        if (dbs_load(min_caller + r) > v) atomicMin(min_caller + r, v);
    }
    root[i] = r;
}
// flag (caller index space, zeroed) <- 1 at the seed row of every cluster; its scan numbers the clusters in ascending seed order
__global__ void __launch_bounds__(DBS_BS) k_dbscan_seeds(const int *__restrict__ root, const int *__restrict__ min_caller, int n, uint8_t *__restrict__ flag) {
    const int i = blockIdx.x * DBS_BS + threadIdx.x;
    if (i < n && root[i] == i) flag[min_caller[i]] = 1;
}
// label of a core row = the number of seeds before its cluster's seed; sorted copy for the border walk (-1 for non-core rows), caller rows
// of the core points and the optional core mask
__global__ void __launch_bounds__(DBS_BS) k_dbscan_core_labels(const int *__restrict__ root, const int *__restrict__ min_caller, const int *__restrict__ pos,
                                                              const uint32_t *__restrict__ perm, int n, int *__restrict__ label_sorted, int32_t *__restrict__ labels,
                                                              uint8_t *__restrict__ core_mask) {
    const int i = blockIdx.x * DBS_BS + threadIdx.x;
    if (i >= n) return;
    const int r = root[i];
    const int lab = r >= 0 ? pos[min_caller[r]] : -1;
    label_sorted[i] = lab;
    const size_t row = perm[i];
    if (r >= 0) labels[row] = lab;
    if (core_mask) core_mask[row] = r >= 0 ? 1 : 0;
}

// ============================================================================================================ border and noise
// The walk once more for the NON-core queries: the smallest label among the core members, or -1 (noise) without one -- Open3D's flood
// fills run in label order and relabel a point only from "unvisited" or "noise", so the first cluster to reach a border point keeps it.
struct DbsBorderArgs { OctView t; const uint32_t *perm; float r2f; double r2; const uint8_t *core; const int *label_sorted; int32_t *labels; };
__global__ void __launch_bounds__(DBS_BS) k_dbscan_border(DbsBorderArgs a) {
    oct_group_frame<DBS_BS>(a.t, [&](const OctGroupQuery &g) {
    const bool bq = g.live && a.core[g.qi] == 0;              // octet-uniform
    if (__ballot(bq) == 0ull) return;
    int best = DBS_NONE;
    // active = bq, fixed for the whole walk
    oct_ball_walk(a.t, g, a.r2f, [&]() { return bq; }, [&](int idx) {
        if (a.core[idx] != 0 && oct_ball_member<true>(g.q, a.t.pts[idx], a.r2f, a.r2)) best = min(best, a.label_sorted[idx]);     // the flag first: a non-core row gives no label
    });
    best = pcr_octet_min_i(best);
    if (bq && g.ol == 0) a.labels[a.perm[g.qi]] = best == DBS_NONE ? -1 : best;
    });
}

// ====================================================================================================== C ABI
extern "C" int pcr_cluster_dbscan(pcr_context *ctx, const float *xyz, int64_t n, double eps, int min_points,
                                  int32_t *labels, uint8_t *core_mask, int64_t *out_n_clusters) {
    return pcr_api_call(ctx, [&]() -> int {
    if (n < 0 || n > 0x7fffffffLL) { ctx->err = "cluster_dbscan: n is negative or over the int limit"; return PCR_EINVAL; }
    if (n > 0 && (!xyz || !labels)) { ctx->err = "cluster_dbscan: null cloud or labels pointer"; return PCR_EINVAL; }
    if (!std::isfinite(eps) || !(eps > 0.0)) { ctx->err = "cluster_dbscan: eps must be finite and > 0"; return PCR_EINVAL; }
    if (min_points < 1) { ctx->err = "cluster_dbscan: min_points < 1"; return PCR_EINVAL; }
    if (out_n_clusters) *out_n_clusters = 0;
    if (n == 0) return PCR_OK;
    PCR_TRY(pcr_arena_reserve(ctx, pcr_scratch_bytes_for(n) + (size_t)n * 64));
    DevCloud c; uint32_t *perm = nullptr;
    PCR_TRY(pcr_import_cloud(ctx, xyz, nullptr, n, &c, &perm, false));
    uint8_t *core = arena<uint8_t>(ctx, n), *flag = arena<uint8_t>(ctx, n);
    int *parent = arena<int>(ctx, n), *root = arena<int>(ctx, n), *min_caller = arena<int>(ctx, n), *pos = arena<int>(ctx, n), *label_sorted = arena<int>(ctx, n);
    int *total = arena<int>(ctx, 1);
    if (!core || !flag || !parent || !root || !min_caller || !pos || !label_sorted || !total) return PCR_ENOMEM;
    const dim3 walk((unsigned)(((size_t)c.cap * OCT + DBS_BS - 1) / DBS_BS)), rows((unsigned)((n + DBS_BS - 1) / DBS_BS));
    const double r2 = eps * eps;
    const float r2f = pcr_wide_r2f(r2);
    DbsCoreArgs ca; ca.t = oct_view(&c); ca.r2 = r2; ca.r2f = r2f; ca.min_points = min_points; ca.core = core; ca.parent = parent; ca.min_caller = min_caller;
    PCR_LAUNCH(ctx, k_dbscan_core, walk, dim3(DBS_BS), 0, ctx->stream, ca);
    DbsUnionArgs ua; ua.t = ca.t; ua.r2 = r2; ua.r2f = r2f; ua.core = core; ua.parent = parent;
    PCR_LAUNCH(ctx, k_dbscan_union, walk, dim3(DBS_BS), 0, ctx->stream, ua);
    PCR_LAUNCH(ctx, k_dbscan_roots, rows, dim3(DBS_BS), 0, ctx->stream, (const uint8_t *)core, (const int *)parent, (const uint32_t *)perm, (int)n, root, min_caller);
    PCR_HIP_CHECK(ctx, hipMemsetAsync(flag, 0, (size_t)n, ctx->stream));
    PCR_LAUNCH(ctx, k_dbscan_seeds, rows, dim3(DBS_BS), 0, ctx->stream, (const int *)root, (const int *)min_caller, (int)n, flag);
    PCR_TRY(pcr_dev_flag_scan(ctx, flag, nullptr, (int)n, pos, total));
    PCR_LAUNCH(ctx, k_dbscan_core_labels, rows, dim3(DBS_BS), 0, ctx->stream, (const int *)root, (const int *)min_caller, (const int *)pos, (const uint32_t *)perm, (int)n,
               label_sorted, labels, core_mask);
    DbsBorderArgs ba; ba.t = ca.t; ba.perm = perm; ba.r2 = r2; ba.r2f = r2f; ba.core = core; ba.label_sorted = label_sorted; ba.labels = labels;
    PCR_LAUNCH(ctx, k_dbscan_border, walk, dim3(DBS_BS), 0, ctx->stream, ba);
    if (out_n_clusters) {                                       // the only host wait of the call, and only when the count is asked for
        int64_t clusters = 0;
        PCR_TRY(pcr_read_count(ctx, total, &clusters));
        *out_n_clusters = clusters;
    }
    return PCR_OK;
    });
}
