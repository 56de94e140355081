// pcr_pmap.hip -- the voxel point map (at most M raw points per cell of a fixed grid: KISS-ICP's local map) and scan-to-map ICP on it; the
// specification is the statement in include/pcr_hip.h (voxel point map).  What an ICP loop is made of is pcr_icp_loop.h; the block builder of
// the maps that grow is pcr_mapgrow.h.
//   a sequence        every way of making rows ends in ONE pass over a sequence of (key, source row) sorted by key and stable inside a key: the
//                     members of a cloud after the project's stable radix sort (create, and the scan of an insert), the merge path of two such
//                     sequences (merge, insert), or the map's own rows with a far flag (remove_far).  pm_build ranks every entry inside its
//                     cell (head flags, their scan, the segment's start), keeps rank < M (and the flag), compacts, finds the cells of the
//                     kept rows, and gathers rows, keys and the cell table into a new block whose cell hash map_build_block makes
//   pm_search         (pcr_pmap.h, shared with pcr_ctime.hip) the ROW rule, eight lanes per query: each lane probes one candidate cell of the cell hash per round (1 / 1 / 4 rounds for
//                     neighbourhood 1 / 7 / 27), then the octet scans the member range of every occupied cell together, lane l rows first + l,
//                     first + l + 8, ... -- consecutive rows, so the loads of an octet are one contiguous stretch -- keeping the smallest
//                     (float64 d^2, row); three exchange steps give the octet's minimum.  min over (d^2, row) does not depend on who saw what
//   k_icp_iter_pmap   the whole iteration, one launch: workgroup b owns the source points [512 b, 512 b + 512) in caller order; octet o searches
//                     for its own eight points in eight rounds (every cross-lane exchange stands in wave-uniform control flow), then EVERY lane
//                     forms the rows of its own point and icp_finish reduces them (a fixed tree per workgroup, workgroups ascending)
//   k_pmap_normals    ESTIMATE, in pm_search's shape: an octet per map row probes the 27 cells around the row's own cell and scans their members
//                     together for the count and the nine float64 sums of the differences; pm_build runs it on the NEW block, behind its cell
//                     hash and before the swap, so a map that estimates its normals is never seen with stale ones.  The iteration kernel learns
//                     validity through its compile-time flag EST, instantiated for point to plane on an estimated map alone
// Nothing in this unit is contracted: every product and sum of the rule is rounded once.
#pragma clang fp contract(off)
#include <cmath>
#include <cstring>
#include <limits>
#include "pcr_icp_loop.h"
#include "pcr_pmap.h"
#include "pcr_eigen3.h"

#define PM_BS 256
#define PM_MAX_POINTS 64
static unsigned pm_blocks(size_t n) { return (unsigned)((n + PM_BS - 1) / PM_BS); }

struct PmPose { double T[12]; };

// ================================================================ the iteration
struct IcpPmapArgs {
    const float *src_xyz;      // packed, caller order
    PmapView map;
    int ns, nbh, plane;        // plane: 1 point to plane, 0 point to point
    double max_d2;
    const int32_t *ncount;     // k_icp_iter_pmap<true> alone (point to plane on an estimated map): a match whose row has ncount < kmin is no row
    int kmin;
};
// EST: the map's normals are its own (ESTIMATE) and the estimator reads them; instantiated for that case alone
template <bool EST>
__global__ void __launch_bounds__(LIN_BS) k_icp_iter_pmap(IcpArgs a, IcpPmapArgs v) {
    // (to icp_finish this is point to plane: the 6x6 LDLT update, fitness = rows / ns)
    icp_iter_frame<ICP_MODE_P2PL, LIN_BS>(a, v.ns, [&](int i, bool live, const double *T, double *acc) {
        double qx = 0.0, qy = 0.0, qz = 0.0;
        if (live) vg_transform(T, v.src_xyz[(size_t)i * 3], v.src_xyz[(size_t)i * 3 + 1], v.src_xyz[(size_t)i * 3 + 2], qx, qy, qz);
        double d2; int row;
        pm_match_own(v.map, v.nbh, live, qx, qy, qz, v.max_d2, d2, row);
        if (EST && row >= 0 && v.ncount[row] < v.kmin) row = -1;
        if (live && row >= 0) {      // the rows (pm_row27, the lever is q) into the 30 sums: [27] sum r^2, [28] sum d^2, [29] rows
            acc[28] += d2; acc[29] += 1.0;
            acc[27] += pm_row27(v.map, v.plane, a.loss, a.loss_k, row, qx, qy, qz, qx, qy, qz, acc);
        }
    });
}

// match[i] = the row of source point i at the pose, or -1; flags for the scan
__global__ void __launch_bounds__(PM_BS) k_pmap_match(const float *__restrict__ src_xyz, int ns, PmPose pose, PmapView m, int nbh, double max_d2, int32_t *__restrict__ match,
                                                      uint8_t *__restrict__ flags) {
    const int i = blockIdx.x * PM_BS + threadIdx.x;
    const bool live = i < ns;
    double qx = 0.0, qy = 0.0, qz = 0.0;
    if (live) vg_transform(pose.T, src_xyz[(size_t)i * 3], src_xyz[(size_t)i * 3 + 1], src_xyz[(size_t)i * 3 + 2], qx, qy, qz);
    double d2; int row;
    pm_match_own(m, nbh, live, qx, qy, qz, max_d2, d2, row);
    if (live) { match[i] = row; flags[i] = row >= 0 ? 1 : 0; }
}
// point to plane on an estimated map: a match whose row is not valid is no row
__global__ void __launch_bounds__(PM_BS) k_pmap_drop_invalid(const int32_t *__restrict__ ncount, int kmin, int ns, int32_t *__restrict__ match, uint8_t *__restrict__ flags) {
    const int i = blockIdx.x * PM_BS + threadIdx.x;
    if (i >= ns || !flags[i]) return;
    if (ncount[match[i]] < kmin) { match[i] = -1; flags[i] = 0; }
}

// The map loop (icp_map_loop, pcr_icp_loop.h) with this unit's kernel forms and argument block.
// single: linearise once at T0 and stop (pcr_point_map_linearize); *sums then receives the 30 sums.
static int pmap_loop(pcr_context *ctx, const char *call, const float *src_xyz, int64_t n_src, const pcr_point_map *map, int neighborhood, double max_d2, const pcr_estimation *est,
                     const double *T0, double rel_fit, double rel_rmse, int max_it, bool single, pcr_result *out, double *sums) {
    IcpArgs a; memset(&a, 0, sizeof a);           // (the bytes of both argument blocks are the graph key)
    a.loss = est->loss; a.loss_k = est->loss_k; a.a = 1.0;
    a.rel_fit = rel_fit; a.rel_rmse = rel_rmse; a.max_it = max_it;
    IcpPmapArgs v; memset(&v, 0, sizeof v);
    v.src_xyz = src_xyz; v.map = map->view; v.ns = (int)n_src; v.nbh = neighborhood; v.plane = est->kind == PCR_EST_POINT_TO_PLANE ? 1 : 0; v.max_d2 = max_d2;
    const bool validity = pm_reads_validity(map, est);      // (point to point never reads it: on an estimated map it runs the launch of a map without normals)
    if (validity) { v.ncount = map->ncount; v.kmin = map->est_min; }
    auto launch = [&](int nb) {
        if (validity) PCR_LAUNCH(ctx, k_icp_iter_pmap<true>, dim3(nb), dim3(LIN_BS), 0, ctx->stream, a, v);
        else PCR_LAUNCH(ctx, k_icp_iter_pmap<false>, dim3(nb), dim3(LIN_BS), 0, ctx->stream, a, v);
    };
    return icp_map_loop(ctx, call, a, &v, sizeof v, v.ns, validity ? 10 : 9 /* the tag of the kernel form (the ICP_MODE_* numbers end at 8) */, launch, T0, single, out, sums);
}

// ================================================================ the map: kernels
// p' = float32(q) (vg_place_point) and n' = float32(R n), entry by entry (a0 b0 + a1 b1) + a2 b2 in float64, not normalised
__global__ void __launch_bounds__(PM_BS) k_pmap_place(const float *__restrict__ xyz, const float *__restrict__ nrm, int n, PmPose pose, float *__restrict__ out_xyz,
                                                      float *__restrict__ out_nrm, int *__restrict__ bad) {
    const int i = blockIdx.x * PM_BS + threadIdx.x;
    if (i >= n) return;
    vg_place_point(pose.T, xyz, i, out_xyz, bad);
    if (!nrm) return;
    const double a = nrm[(size_t)i * 3], b = nrm[(size_t)i * 3 + 1], c = nrm[(size_t)i * 3 + 2];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        double s = pose.T[4 * r] * a + pose.T[4 * r + 1] * b;
        s = s + pose.T[4 * r + 2] * c;
        const float f = (float)s;
        out_nrm[(size_t)i * 3 + r] = f;
        if (!isfinite(f)) atomicOr(bad, 1);
    }
}
// the Morton key of every point's cell on the grid (the float64 expression of k_voxel_keys; the caller has checked that no index is negative or
// past 2^21) and the point's index as the value the stable sort carries
__global__ void __launch_bounds__(PM_BS) k_pmap_keys(const float *__restrict__ xyz, int n, double ox, double oy, double oz, double voxel, uint64_t *__restrict__ keys,
                                                     uint32_t *__restrict__ vals) {
    const int i = blockIdx.x * PM_BS + threadIdx.x;
    if (i >= n) return;
    const double x = (double)xyz[(size_t)i * 3], y = (double)xyz[(size_t)i * 3 + 1], z = (double)xyz[(size_t)i * 3 + 2];
    const uint32_t ix = (uint32_t)(int)floor((x - ox) / voxel), iy = (uint32_t)(int)floor((y - oy) / voxel), iz = (uint32_t)(int)floor((z - oz) / voxel);
    keys[i] = pcr_morton3(ix, iy, iz);
    vals[i] = (uint32_t)i;
}
// the merge path of A's rows and the sorted sequence B: an entry of A goes behind the entries of B with a smaller key, an entry of B behind the
// entries of A with a key that is not larger -- in a shared cell A's members stand first, each side in its own order.  b_vals: the source row of
// B's entry j (nullptr: j); sources of B are numbered from a_n on
__device__ static inline int pm_upper_bound(const uint64_t *__restrict__ keys, int n, uint64_t key) {
    int lo = 0, hi = n;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (keys[mid] <= key) lo = mid + 1; else hi = mid; }
    return lo;
}
__global__ void __launch_bounds__(PM_BS) k_pmap_merge_path(const uint64_t *__restrict__ a_keys, int a_n, const uint64_t *__restrict__ b_keys, const uint32_t *__restrict__ b_vals,
                                                           int b_n, uint64_t *__restrict__ keys, uint32_t *__restrict__ src) {
    const int t = blockIdx.x * PM_BS + threadIdx.x;
    if (t >= a_n + b_n) return;
    if (t < a_n) {
        const uint64_t key = a_keys[t];
        const int o = t + vg_lower_bound(b_keys, b_n, key);
        keys[o] = key; src[o] = (uint32_t)t;
    } else {
        const int j = t - a_n;
        const uint64_t key = b_keys[j];
        const int o = j + pm_upper_bound(a_keys, a_n, key);
        keys[o] = key; src[o] = (uint32_t)a_n + (b_vals ? b_vals[j] : (uint32_t)j);
    }
}
__global__ void __launch_bounds__(PM_BS) k_pmap_heads(const uint64_t *__restrict__ keys, int n, uint8_t *__restrict__ head) {
    const int i = blockIdx.x * PM_BS + threadIdx.x;
    if (i < n) head[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1 : 0;
}
__global__ void __launch_bounds__(PM_BS) k_pmap_seg_start(const uint8_t *__restrict__ head, const int *__restrict__ hpos, int n, int *__restrict__ seg_start) {
    const int i = blockIdx.x * PM_BS + threadIdx.x;
    if (i < n && head[i]) seg_start[hpos[i]] = i;
}
// keep[i] = (rank of entry i inside its cell) < M, and the far flag where there is one
__global__ void __launch_bounds__(PM_BS) k_pmap_keep(const uint8_t *__restrict__ head, const int *__restrict__ hpos, const int *__restrict__ seg_start, const uint8_t *__restrict__ near,
                                                     int n, int max_points, uint8_t *__restrict__ keep) {
    const int i = blockIdx.x * PM_BS + threadIdx.x;
    if (i >= n) return;
    const int seg = hpos[i] + (head[i] ? 1 : 0) - 1;
    keep[i] = (i - seg_start[seg] < max_points && (!near || near[i])) ? 1 : 0;
}
__global__ void __launch_bounds__(PM_BS) k_pmap_compact(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ src, const uint8_t *__restrict__ keep,
                                                        const int *__restrict__ kpos, int n, int cap, uint64_t *__restrict__ out_keys, uint32_t *__restrict__ out_src) {
    const int i = blockIdx.x * PM_BS + threadIdx.x;
    if (i >= n || !keep[i]) return;
    const int o = kpos[i];
    if (o < 0 || o >= cap) return;
    out_keys[o] = keys[i]; out_src[o] = src ? src[i] : (uint32_t)i;
}
// near[i] = d^2 < r^2 of row i (vg_within's arithmetic on the float32 point)
__global__ void __launch_bounds__(PM_BS) k_pmap_near(const float *__restrict__ xyz, int n, double cx, double cy, double cz, double r2, uint8_t *__restrict__ near) {
    const int i = blockIdx.x * PM_BS + threadIdx.x;
    if (i >= n) return;
    near[i] = vg_within(make_float4(xyz[(size_t)i * 3], xyz[(size_t)i * 3 + 1], xyz[(size_t)i * 3 + 2], 0.0f), cx, cy, cz, r2) ? 1 : 0;
}
// row o of the new block: the bits of its source row (A's below a_n, B's from a_n on), its key, and -- for the first row of a cell -- the cell table
struct PmSources { const float *a_xyz, *a_nrm; int a_n; const float *b_xyz, *b_nrm; int b_n; };
__global__ void __launch_bounds__(PM_BS) k_pmap_gather(PmSources s, const uint64_t *__restrict__ keys, const uint32_t *__restrict__ src, const uint8_t *__restrict__ chead,
                                                       const int *__restrict__ cpos, int rows, int cells, float *__restrict__ out_xyz, float *__restrict__ out_nrm,
                                                       uint64_t *__restrict__ out_keys, int *__restrict__ cell_first) {
    const int o = blockIdx.x * PM_BS + threadIdx.x;
    if (o == 0) cell_first[cells] = rows;
    if (o >= rows) return;
    const int r = (int)src[o];
    const bool from_a = r < s.a_n;
    const int q = from_a ? r : r - s.a_n;
    if (q < 0 || q >= (from_a ? s.a_n : s.b_n)) return;
    const float *px = (from_a ? s.a_xyz : s.b_xyz) + (size_t)q * 3;
    const float x = px[0], y = px[1], z = px[2];
    out_xyz[(size_t)o * 3] = x; out_xyz[(size_t)o * 3 + 1] = y; out_xyz[(size_t)o * 3 + 2] = z;
    if (out_nrm) {
        const float *pn = (from_a ? s.a_nrm : s.b_nrm) + (size_t)q * 3;
        const float a = pn[0], b = pn[1], c = pn[2];
        out_nrm[(size_t)o * 3] = a; out_nrm[(size_t)o * 3 + 1] = b; out_nrm[(size_t)o * 3 + 2] = c;
    }
    out_keys[o] = keys[o];
    if (chead[o]) { const int c = cpos[o]; if (c >= 0 && c < cells) cell_first[c] = o; }
}
__device__ static inline int pm_compact21(uint64_t x) {      // inverse of pcr_spread21
    x &= 0x1249249249249249ull;
    x = (x | (x >> 2)) & 0x10c30c30c30c30c3ull;
    x = (x | (x >> 4)) & 0x100f00f00f00f00full;
    x = (x | (x >> 8)) & 0x1f0000ff0000ffull;
    x = (x | (x >> 16)) & 0x1f00000000ffffull;
    x = (x | (x >> 32)) & 0x1fffffull;
    return (int)x;
}
__global__ void __launch_bounds__(PM_BS) k_pmap_read_cells(const uint64_t *__restrict__ keys, const int *__restrict__ cell_first, int cells, int32_t *__restrict__ cell3,
                                                           int32_t *__restrict__ start, int32_t *__restrict__ count) {
    const int c = blockIdx.x * PM_BS + threadIdx.x;
    if (c >= cells) return;
    const int f = cell_first[c];
    if (cell3) { const uint64_t k = keys[f]; cell3[(size_t)c * 3] = pm_compact21(k); cell3[(size_t)c * 3 + 1] = pm_compact21(k >> 1); cell3[(size_t)c * 3 + 2] = pm_compact21(k >> 2); }
    if (start) start[c] = f;
    if (count) count[c] = cell_first[c + 1] - f;
}

// ================================================================ ESTIMATE: the normals of a map from its own rows
// An octet per row, in pm_search's shape: lane l probes candidate cell 8 r + l of the row's own cell (from its key) in round r, then the octet scans
// every occupied cell together, lane l the members first + l, first + l + 8, ...  Each lane keeps its count and the nine float64 sums of the
// differences e = p_j - p_i of its neighbours (d^2 < rho^2), in the order it meets them: candidate cells ascending, members ascending.  A lane's
// share is therefore fixed by the rows alone (the members of a cell whose rank inside the cell is l mod 8), and the xor tree of width 8 adds the
// eight shares in one fixed shape, ((0 + 1) + (2 + 3)) + ((4 + 5) + (6 + 7)).  Lane 0 of the octet finishes the row.
struct PmNormalArgs {
    PmapView map;              // of the block the rows live in: xyz, the cell hash (nrm is what is written, through `nrm` below)
    const uint64_t *keys;      // the Morton key of every row's cell
    int rows, kmin;
    double r2;                 // rho^2, one float64 product
    float *nrm; int32_t *ncount; int *nvalid;
};
__global__ void __launch_bounds__(PM_BS) k_pmap_normals(PmNormalArgs a) {
    const int ol = threadIdx.x & 7;
    const int i = blockIdx.x * (PM_BS / 8) + (threadIdx.x >> 3);
    const bool live = i < a.rows;
    const unsigned mask = *a.map.dmask;
    GridView g;
    g.tab = a.map.tab; g.dmask = a.map.dmask; g.L = 0;
    double qx = 0.0, qy = 0.0, qz = 0.0;
    int cx = 0, cy = 0, cz = 0;
    if (live) {
        const float *q = a.map.xyz + (size_t)i * 3;
        qx = q[0]; qy = q[1]; qz = q[2];
        const uint64_t key = a.keys[i];
        cx = pm_compact21(key); cy = pm_compact21(key >> 1); cz = pm_compact21(key >> 2);
    }
    double s[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int n = 0;
    for (int r = 0; r < 4; r++) {                                        // (wave-uniform)
        const int k = r * 8 + ol;
        int first = 0, cnt = 0;
        if (live && k < 27) {
            int dx, dy, dz;
            vg_offset(27, k, dx, dy, dz);
            const int2 e = pcr_grid_lookup(g, mask, cx + dx, cy + dy, cz + dz);      // (a cell outside [0, 2^21) does not exist: not probed)
            if (e.y > 0 && e.x >= 0 && e.x < a.rows) { first = e.x; cnt = min(e.y, a.rows - e.x); }
        }
        if (__ballot(cnt > 0) == 0ull) continue;                         // (wave-uniform)
        for (int l = 0; l < 8; l++) {                                    // (wave-uniform: the exchanges below are reached by all 64 lanes together)
            const int f = __shfl(first, l, 8), c = __shfl(cnt, l, 8);
            for (int j = ol; j < c; j += 8) {
                const float *p = a.map.xyz + (size_t)(f + j) * 3;
                const double px = p[0], py = p[1], pz = p[2];
                const double dx = qx - px, dy = qy - py, dz = qz - pz;
                const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
                double d2 = xx + yy;
                d2 = d2 + zz;
                if (d2 < a.r2) {
                    const double ex = px - qx, ey = py - qy, ez = pz - qz;
                    n++;
                    s[0] += ex; s[1] += ey; s[2] += ez;
                    s[3] += ex * ex; s[4] += ex * ey; s[5] += ex * ez; s[6] += ey * ey; s[7] += ey * ez; s[8] += ez * ez;
                }
            }
        }
    }
#pragma unroll
    for (int w = 1; w < 8; w <<= 1) {
        n += __shfl_xor(n, w, 8);
#pragma unroll
        for (int t = 0; t < 9; t++) s[t] += __shfl_xor(s[t], w, 8);
    }
    bool valid = false;
    if (live && ol == 0) {
        double C6[6] = {1.0, 0.0, 0.0, 1.0, 0.0, 1.0};                   // fewer than 3 neighbours: the identity
        if (n >= 3) {
            const double c = (double)n;
            const double mx = s[0] / c, my = s[1] / c, mz = s[2] / c;
            C6[0] = s[3] / c - mx * mx; C6[1] = s[4] / c - mx * my; C6[2] = s[5] / c - mx * mz;
            C6[3] = s[6] / c - my * my; C6[4] = s[7] / c - my * mz; C6[5] = s[8] / c - mz * mz;
        }
        double nv[3];
        d_fast_eigen3x3(C6, nv);
        const double nn = sqrt(nv[0] * nv[0] + nv[1] * nv[1] + nv[2] * nv[2]);
        if (nn == 0.0 || !(nn == nn)) { nv[0] = 0.0; nv[1] = 0.0; nv[2] = 1.0; }
        a.nrm[(size_t)i * 3] = (float)nv[0]; a.nrm[(size_t)i * 3 + 1] = (float)nv[1]; a.nrm[(size_t)i * 3 + 2] = (float)nv[2];
        a.ncount[i] = n;
        valid = n >= a.kmin;
    }
    const unsigned long long vb = __ballot(valid);
    if ((threadIdx.x & 63) == 0 && vb != 0ull) atomicAdd(a.nvalid, __popcll(vb));
}

// ================================================================ the map: host
struct PmGrid { double grid_min[3], voxel; };
static void pm_origin(const PmGrid &g, double *org) { for (int d = 0; d < 3; d++) org[d] = g.grid_min[d] - g.voxel * 0.5; }      // (pcr_dev_voxel's expression)
// a sequence of (key, source row), sorted by key and stable inside a key; src == nullptr: entry i is source row i
struct PmSeq { const uint64_t *keys; const uint32_t *src; int n; };
// scratch of the context's arena for sequences of `entries` entries in all (the placed members, the sort, the passes of pm_build)
static size_t pm_scratch(int64_t entries) { return 2 * pcr_scratch_bytes_for(entries) + pcr_sort_temp_bytes((size_t)(entries > 0 ? entries : 1)) + (size_t)entries * 192 + (4u << 20); }

static int pm_check_map(pcr_context *ctx, const pcr_point_map *map, const char *call) { return vg_check_handle(ctx, map, call); }
static int pm_check_max_points(pcr_context *ctx, const char *call, int max_points) {
    if (max_points < 1 || max_points > PM_MAX_POINTS) { ctx->err = std::string(call) + ": max_points_per_voxel must lie in 1 .. 64"; return PCR_EINVAL; }
    return PCR_OK;
}
static int pm_check_cloud(pcr_context *ctx, const char *call, const float *xyz, int64_t n, const double *T) {
    if (n < 1 || n > 0x7fffffff / 8 || !xyz) { ctx->err = std::string(call) + ": xyz must hold 1 .. 2^28 - 1 points"; return PCR_EINVAL; }
    if (T) PCR_TRY(vg_check_T(ctx, call, "T", T));
    return PCR_OK;
}

// The members of a cloud at a pose as a sequence on the grid g, in the context's arena (reserved by the caller): *xyz_out / *nrm_out are the member
// arrays the sequence's source rows index (the inputs themselves without a pose).  own_grid: the grid is the cloud's own (grid_min = its minimum,
// written to g).  PCR_EINVAL when a member leaves the grid.
static int pm_cloud_seq(pcr_context *ctx, const char *call, const float *xyz, const float *normals, int64_t n, const double *T, PmGrid *g, bool own_grid, PmSeq *seq,
                        const float **xyz_out, const float **nrm_out) {
    {
        const float *ptr[2] = {xyz, normals}; const size_t cnt[2] = {(size_t)n * 3, (size_t)n * 3}; const char *name[2] = {"xyz", "normals"};
        PCR_TRY(vg_check_finite(ctx, call, ptr, cnt, name, 2));
    }
    int *bad = nullptr;
    if (T) {
        float *placed = arena<float>(ctx, (size_t)n * 3), *pn = normals ? arena<float>(ctx, (size_t)n * 3) : nullptr;
        bad = arena<int>(ctx, 1);
        if (!placed || (normals && !pn) || !bad) return PCR_ENOMEM;
        PmPose pose; memcpy(pose.T, T, sizeof pose.T);
        PCR_HIP_CHECK(ctx, hipMemsetAsync(bad, 0, sizeof(int), ctx->stream));
        PCR_LAUNCH(ctx, k_pmap_place, dim3(pm_blocks((size_t)n)), dim3(PM_BS), 0, ctx->stream, xyz, normals, (int)n, pose, placed, pn, bad);
        xyz = placed; normals = pn;
    }
    double pb[6], org[3];
    PCR_TRY(pcr_dev_bounds(ctx, xyz, n, pb));
    int64_t nonfinite = 0;
    if (bad) PCR_TRY(pcr_read_count(ctx, bad, &nonfinite));
    if (own_grid) for (int d = 0; d < 3; d++) g->grid_min[d] = pb[d];
    pm_origin(*g, org);
    if (nonfinite != 0 || !vg_inside_grid(pb, g->grid_min, g->voxel)) { ctx->err = std::string(call) + ": xyz lies outside the map's grid (cell indices must stay in [0, 2^21) on every axis)"; return PCR_EINVAL; }
    uint32_t top = 0;
    for (int d = 0; d < 3; d++) { const uint32_t e = (uint32_t)floor((pb[3 + d] - org[d]) / g->voxel); top = e > top ? e : top; }
    int end_bit = 0;
    while (top) { end_bit += 3; top >>= 1; }
    uint64_t *k0 = arena<uint64_t>(ctx, (size_t)n), *k1 = arena<uint64_t>(ctx, (size_t)n);
    uint32_t *v0 = arena<uint32_t>(ctx, (size_t)n), *v1 = arena<uint32_t>(ctx, (size_t)n);
    const size_t tb = pcr_sort_temp_bytes((size_t)n);
    void *temp = pcr_arena_alloc(ctx, tb);
    if (!k0 || !k1 || !v0 || !v1 || !temp) return PCR_ENOMEM;
    PCR_LAUNCH(ctx, k_pmap_keys, dim3(pm_blocks((size_t)n)), dim3(PM_BS), 0, ctx->stream, xyz, (int)n, org[0], org[1], org[2], g->voxel, k0, v0);
    PCR_TRY(pcr_sort_pairs(ctx, temp, tb, k0, k1, v0, v1, (size_t)n, end_bit));
    *seq = PmSeq{k1, v1, (int)n};
    *xyz_out = xyz; *nrm_out = normals;
    return PCR_OK;
}

// The one pass from a sequence to a map block (see the head of this file).  near: optional flag per entry that must hold too (remove_far).  On
// PCR_OK the block is adopted by m (a new map has block == nullptr; an old block is freed, which waits for the device) and m holds the counts; on
// an error m is untouched.  No row kept: PCR_EINVAL (would leave the map empty).
// The normals of the new block (PmKind): none; the sources' own, row by row; or ESTIMATE(radius, min_neighbors) on the new block's rows, enqueued
// behind its cell hash and finished before the block is adopted -- the sources' normals are not read then.
struct PmKind { bool normals, estimated; double radius; int min_neighbors; };
static PmKind pm_kind_of(const pcr_point_map *m) { return PmKind{m->normals, m->estimated, m->est_radius, m->est_min}; }
template <bool NRM, bool EST>
static int pm_build_t(pcr_context *ctx, const char *call, const PmSeq &seq, const uint8_t *near, const PmSources &s, int max_points, const PmKind &kind, pcr_point_map *m) {
    const int n = seq.n;
    uint8_t *head = arena<uint8_t>(ctx, (size_t)n), *keep = arena<uint8_t>(ctx, (size_t)n), *chead = arena<uint8_t>(ctx, (size_t)n);
    int *hpos = arena<int>(ctx, (size_t)n), *seg_start = arena<int>(ctx, (size_t)n), *kpos = arena<int>(ctx, (size_t)n), *cpos = arena<int>(ctx, (size_t)n), *word = arena<int>(ctx, 3);
    uint64_t *ckeys = arena<uint64_t>(ctx, (size_t)n);
    uint32_t *csrc = arena<uint32_t>(ctx, (size_t)n);
    if (!head || !keep || !chead || !hpos || !seg_start || !kpos || !cpos || !word || !ckeys || !csrc) return PCR_ENOMEM;
    const dim3 gn(pm_blocks((size_t)n)), bs(PM_BS);
    PCR_LAUNCH(ctx, k_pmap_heads, gn, bs, 0, ctx->stream, seq.keys, n, head);
    PCR_TRY(pcr_dev_flag_scan(ctx, head, nullptr, n, hpos, word));
    PCR_LAUNCH(ctx, k_pmap_seg_start, gn, bs, 0, ctx->stream, (const uint8_t *)head, (const int *)hpos, n, seg_start);
    PCR_LAUNCH(ctx, k_pmap_keep, gn, bs, 0, ctx->stream, (const uint8_t *)head, (const int *)hpos, (const int *)seg_start, near, n, max_points, keep);
    PCR_TRY(pcr_dev_flag_scan(ctx, keep, nullptr, n, kpos, word + 1));
    int64_t rows = 0;
    PCR_TRY(pcr_read_count(ctx, word + 1, &rows));
    if (rows < 0 || rows > n) { ctx->err = std::string(call) + ": the scan of the kept rows is out of range"; return PCR_EHIP; }
    if (rows == 0) { ctx->err = std::string(call) + ": would leave the map empty"; return PCR_EINVAL; }
    PCR_LAUNCH(ctx, k_pmap_compact, gn, bs, 0, ctx->stream, seq.keys, seq.src, (const uint8_t *)keep, (const int *)kpos, n, (int)rows, ckeys, csrc);
    const dim3 gr(pm_blocks((size_t)rows));
    PCR_LAUNCH(ctx, k_pmap_heads, gr, bs, 0, ctx->stream, (const uint64_t *)ckeys, (int)rows, chead);
    PCR_TRY(pcr_dev_flag_scan(ctx, chead, nullptr, (int)rows, cpos, word + 2));
    int64_t cells = 0;
    PCR_TRY(pcr_read_count(ctx, word + 2, &cells));
    if (cells < 1 || cells > rows) { ctx->err = std::string(call) + ": the scan of the cells is out of range"; return PCR_EHIP; }
    typedef PmapRow<NRM, EST> Row;
    MapBlock<Row> nb;
    PCR_TRY(map_build_block<Row>(ctx, call, rows, &nb, [&](const typename Row::Out &o) -> int {
        PCR_LAUNCH(ctx, k_pmap_gather, gr, bs, 0, ctx->stream, s, (const uint64_t *)ckeys, (const uint32_t *)csrc, (const uint8_t *)chead, (const int *)cpos, (int)rows, (int)cells,
                   o.xyz, EST ? (float *)nullptr : o.nrm, o.keys, o.cell_first);
        if (EST) PCR_HIP_CHECK(ctx, hipMemsetAsync(o.nvalid, 0, sizeof(int), ctx->stream));
        return PCR_OK;
    }, [&](const MapBlock<Row> &b) -> int {
        if (!EST) return PCR_OK;
        PmNormalArgs a; memset(&a, 0, sizeof a);
        a.map = m->view;                                      // the grid (origin, voxel size); the arrays are the new block's
        a.map.tab = b.gv.tab; a.map.dmask = b.gv.dmask; a.map.xyz = b.out.xyz; a.map.nrm = nullptr;
        a.keys = b.out.keys; a.rows = (int)rows; a.kmin = kind.min_neighbors; a.r2 = kind.radius * kind.radius;
        a.nrm = b.out.nrm; a.ncount = b.out.ncount; a.nvalid = b.out.nvalid;
        PCR_LAUNCH(ctx, k_pmap_normals, dim3(pm_blocks((size_t)rows * 8)), dim3(PM_BS), 0, ctx->stream, a);
        return PCR_OK;
    }));
    int valid = 0;
    if (EST) {                                                // (the stream is idle: map_build_block has waited)
        const hipError_t e = hipMemcpy(&valid, nb.out.nvalid, sizeof(int), hipMemcpyDeviceToHost);
        if (e != hipSuccess || valid < 0 || valid > rows) {
            (void)hipFree(nb.block);
            ctx->err = std::string(call) + ": the count of the valid rows could not be read";
            return PCR_EHIP;
        }
    }
    map_adopt<Row>(m, nb, rows);
    m->n_cells = cells;
    m->normals = NRM; m->estimated = EST;
    m->est_radius = EST ? kind.radius : 0.0; m->est_min = EST ? kind.min_neighbors : 0; m->valid_rows = valid;
    return PCR_OK;
}
static int pm_build(pcr_context *ctx, const char *call, const PmSeq &seq, const uint8_t *near, const PmSources &s, int max_points, const PmKind &kind, pcr_point_map *m) {
    if (kind.estimated) return pm_build_t<true, true>(ctx, call, seq, near, s, max_points, kind, m);
    return kind.normals ? pm_build_t<true, false>(ctx, call, seq, near, s, max_points, kind, m) : pm_build_t<false, false>(ctx, call, seq, near, s, max_points, kind, m);
}

static int pm_create(pcr_context *ctx, const char *call, const float *xyz, const float *normals, int64_t n, double voxel_size, int max_points, const double *grid_min3,
                     const double *T, pcr_point_map **out) {
    const std::string who(call);
    if (!out) { ctx->err = who + ": out is null"; return PCR_EINVAL; }
    *out = nullptr;
    if (!(voxel_size > 0.0) || !std::isfinite(voxel_size)) { ctx->err = who + ": voxel_size <= 0"; return PCR_EINVAL; }
    PCR_TRY(pm_check_max_points(ctx, call, max_points));
    if (grid_min3) PCR_TRY(vg_check_grid_min(ctx, call, grid_min3));
    PCR_TRY(pm_check_cloud(ctx, call, xyz, n, T));
    PCR_TRY(pcr_arena_reserve(ctx, pm_scratch(n)));
    PmGrid g; g.voxel = voxel_size;
    if (grid_min3) memcpy(g.grid_min, grid_min3, sizeof g.grid_min);
    PmSeq seq; const float *mx, *mn;
    PCR_TRY(pm_cloud_seq(ctx, call, xyz, normals, n, T, &g, grid_min3 == nullptr, &seq, &mx, &mn));
    pcr_point_map *m = new pcr_point_map();
    m->device = ctx->device; m->max_points = max_points; m->normals = normals != nullptr;
    memcpy(m->grid_min, g.grid_min, sizeof m->grid_min);
    pm_origin(g, m->view.org);
    m->view.voxel = voxel_size;
    const PmSources s{mx, mn, (int)n, nullptr, nullptr, 0};
    const int rc = pm_build(ctx, call, seq, nullptr, s, max_points, PmKind{m->normals, false, 0.0, 0}, m);
    if (rc != PCR_OK) { delete m; return rc; }
    *out = m;
    return PCR_OK;
}

extern "C" int pcr_point_map_create(pcr_context *ctx, const float *xyz, const float *normals, int64_t n, double voxel_size, int max_points_per_voxel, pcr_point_map **out) {
    return pcr_api_call(ctx, [&]() -> int { return pm_create(ctx, "point_map_create", xyz, normals, n, voxel_size, max_points_per_voxel, nullptr, nullptr, out); });
}
extern "C" int pcr_point_map_create_on_grid(pcr_context *ctx, const float *xyz, const float *normals, int64_t n, double voxel_size, int max_points_per_voxel,
                                            const double *grid_min3, const double *T, pcr_point_map **out) {
    return pcr_api_call(ctx, [&]() -> int {
    if (!grid_min3) { ctx->err = "point_map_create_on_grid: grid_min3 is null"; return PCR_EINVAL; }
    return pm_create(ctx, "point_map_create_on_grid", xyz, normals, n, voxel_size, max_points_per_voxel, grid_min3, T, out);
    });
}

extern "C" int pcr_point_map_destroy(pcr_point_map *map) {
    if (!map) return PCR_OK;
    if (map->block) {
        if (hipSetDevice(map->device) != hipSuccess) return PCR_EHIP;
        (void)hipFree(map->block);                            // waits for the device: no call is still reading the block
    }
    delete map;
    return PCR_OK;
}

extern "C" int pcr_point_map_size(const pcr_point_map *map, int64_t *rows, int64_t *cells) {
    if (!map) return PCR_EINVAL;
    if (rows) *rows = map->cells;
    if (cells) *cells = map->n_cells;
    return PCR_OK;
}

extern "C" int pcr_point_map_grid(const pcr_point_map *map, double *grid_min3, double *origin3, double *voxel_size, int *max_points_per_voxel, int *has_normals) {
    if (!map) return PCR_EINVAL;
    if (grid_min3) memcpy(grid_min3, map->grid_min, sizeof map->grid_min);
    if (origin3) memcpy(origin3, map->view.org, sizeof map->view.org);
    if (voxel_size) *voxel_size = map->view.voxel;
    if (max_points_per_voxel) *max_points_per_voxel = map->max_points;
    if (has_normals) *has_normals = map->normals ? 1 : 0;
    return PCR_OK;
}

extern "C" int pcr_point_map_read(pcr_context *ctx, const pcr_point_map *map, int32_t *cell3, int32_t *first_row, int32_t *count, float *xyz, float *normals) {
    return pcr_api_call(ctx, [&]() -> int {
    PCR_TRY(pm_check_map(ctx, map, "point_map_read"));
    if (normals && !map->normals) { ctx->err = "point_map_read: normals asked of a map without normals"; return PCR_EINVAL; }
    if (cell3 || first_row || count)
        PCR_LAUNCH(ctx, k_pmap_read_cells, dim3(pm_blocks((size_t)map->n_cells)), dim3(PM_BS), 0, ctx->stream, (const uint64_t *)map->keys, (const int *)map->cell_first,
                   (int)map->n_cells, cell3, first_row, count);
    if (xyz) PCR_HIP_CHECK(ctx, hipMemcpyAsync(xyz, map->view.xyz, sizeof(float) * 3 * (size_t)map->cells, hipMemcpyDeviceToDevice, ctx->stream));
    if (normals) PCR_HIP_CHECK(ctx, hipMemcpyAsync(normals, map->view.nrm, sizeof(float) * 3 * (size_t)map->cells, hipMemcpyDeviceToDevice, ctx->stream));
    return PCR_OK;
    });
}

// ESTIMATE: the map's own sequence through pm_build once more -- every row is kept (its rank is below M), so the new block has the same rows bit
// for bit, with room for the normals and the counts, which the build computes before it swaps the block in
extern "C" int pcr_point_map_estimate_normals(pcr_context *ctx, pcr_point_map *map, double radius, int min_neighbors, int64_t *valid_rows) {
    return pcr_api_call(ctx, [&]() -> int {
    const char *call = "point_map_estimate_normals";
    if (valid_rows) *valid_rows = 0;
    PCR_TRY(pm_check_map(ctx, map, call));
    if (map->normals && !map->estimated) { ctx->err = "point_map_estimate_normals: the map has normals of the caller's (normals are estimated on a map without)"; return PCR_EINVAL; }
    if (!std::isfinite(radius) || !(radius > 0.0) || !(radius <= map->view.voxel)) { ctx->err = "point_map_estimate_normals: radius must be finite, greater than 0 and at most voxel_size"; return PCR_EINVAL; }
    if (min_neighbors < 3) { ctx->err = "point_map_estimate_normals: min_neighbors must be at least 3"; return PCR_EINVAL; }
    PCR_TRY(pcr_arena_reserve(ctx, pm_scratch(map->cells)));
    const int n = (int)map->cells;
    const PmSources s{map->view.xyz, nullptr, n, nullptr, nullptr, 0};
    PCR_TRY(pm_build(ctx, call, PmSeq{map->keys, nullptr, n}, nullptr, s, map->max_points, PmKind{true, true, radius, min_neighbors}, map));
    if (valid_rows) *valid_rows = map->valid_rows;
    return PCR_OK;
    });
}

extern "C" int pcr_point_map_read_normal_counts(pcr_context *ctx, const pcr_point_map *map, int32_t *counts) {
    return pcr_api_call(ctx, [&]() -> int {
    PCR_TRY(pm_check_map(ctx, map, "point_map_read_normal_counts"));
    if (!map->estimated) { ctx->err = "point_map_read_normal_counts: the map does not estimate its normals"; return PCR_EINVAL; }
    if (!counts) { ctx->err = "point_map_read_normal_counts: counts is null"; return PCR_EINVAL; }
    PCR_HIP_CHECK(ctx, hipMemcpyAsync(counts, map->ncount, sizeof(int32_t) * (size_t)map->cells, hipMemcpyDeviceToDevice, ctx->stream));
    return PCR_OK;
    });
}

extern "C" int pcr_point_map_normal_rule(const pcr_point_map *map, int *estimated, double *radius, int *min_neighbors) {
    if (!map) return PCR_EINVAL;
    if (estimated) *estimated = map->estimated ? 1 : 0;
    if (radius) *radius = map->est_radius;
    if (min_neighbors) *min_neighbors = map->est_min;
    return PCR_OK;
}

// map <- the rows of the merge path of the map's rows and the sequence b (sources: the arrays bx / bn with b_rows rows)
static int pm_merge_into(pcr_context *ctx, const char *call, pcr_point_map *map, const PmSeq &b, const float *bx, const float *bn, int b_rows) {
    const size_t total = (size_t)map->cells + (size_t)b.n;
    if (total > (size_t)(0x7fffffff / 8)) { ctx->err = std::string(call) + ": the merged sequence would hold 2^28 entries or more"; return PCR_EINVAL; }
    uint64_t *mk = arena<uint64_t>(ctx, total);
    uint32_t *ms = arena<uint32_t>(ctx, total);
    if (!mk || !ms) return PCR_ENOMEM;
    PCR_LAUNCH(ctx, k_pmap_merge_path, dim3(pm_blocks(total)), dim3(PM_BS), 0, ctx->stream, (const uint64_t *)map->keys, (int)map->cells, b.keys, b.src, b.n, mk, ms);
    const PmSources s{map->view.xyz, map->view.nrm, (int)map->cells, bx, bn, b_rows};
    return pm_build(ctx, call, PmSeq{mk, ms, (int)total}, nullptr, s, map->max_points, pm_kind_of(map), map);
}

extern "C" int pcr_point_map_insert(pcr_context *ctx, pcr_point_map *map, const float *xyz, const float *normals, int64_t n, const double *T) {
    return pcr_api_call(ctx, [&]() -> int {
    const char *call = "point_map_insert";
    PCR_TRY(pm_check_map(ctx, map, call));
    PCR_TRY(pm_check_cloud(ctx, call, xyz, n, T));
    if (map->estimated && normals) { ctx->err = "point_map_insert: normals must be null for a map that estimates its normals"; return PCR_EINVAL; }
    if (!map->estimated && (normals != nullptr) != map->normals) { ctx->err = "point_map_insert: normals must be given exactly when the map has normals"; return PCR_EINVAL; }
    PCR_TRY(pcr_arena_reserve(ctx, pm_scratch(2 * n + map->cells)));
    PmGrid g; memcpy(g.grid_min, map->grid_min, sizeof g.grid_min); g.voxel = map->view.voxel;
    PmSeq seq; const float *mx, *mn;
    PCR_TRY(pm_cloud_seq(ctx, call, xyz, normals, n, T, &g, false, &seq, &mx, &mn));
    return pm_merge_into(ctx, call, map, seq, mx, mn, (int)n);
    });
}

extern "C" int pcr_point_map_merge(pcr_context *ctx, pcr_point_map *map, const pcr_point_map *other) {
    return pcr_api_call(ctx, [&]() -> int {
    const char *call = "point_map_merge";
    PCR_TRY(pm_check_map(ctx, map, call));
    if (!other || !other->block) { ctx->err = "point_map_merge: other is null"; return PCR_EINVAL; }
    if (other == map) { ctx->err = "point_map_merge: other is the map itself"; return PCR_EINVAL; }
    if (other->device != ctx->device) { ctx->err = "point_map_merge: other lives on another device than the context"; return PCR_EINVAL; }
    if (memcmp(&map->view.voxel, &other->view.voxel, sizeof(double)) != 0 || memcmp(map->view.org, other->view.org, sizeof map->view.org) != 0) {
        ctx->err = "point_map_merge: other is not on the map's grid (voxel size and origin must be equal bit for bit)"; return PCR_EINVAL;
    }
    if (map->max_points != other->max_points) { ctx->err = "point_map_merge: other has another max_points_per_voxel"; return PCR_EINVAL; }
    if ((map->normals && !map->estimated) != (other->normals && !other->estimated)) { ctx->err = "point_map_merge: one map has normals and the other has none"; return PCR_EINVAL; }
    PCR_TRY(pcr_arena_reserve(ctx, pm_scratch(map->cells + other->cells)));
    return pm_merge_into(ctx, call, map, PmSeq{other->keys, nullptr, (int)other->cells}, other->view.xyz, other->view.nrm, (int)other->cells);
    });
}

extern "C" int pcr_point_map_remove_far(pcr_context *ctx, pcr_point_map *map, const double *center3, double max_distance, int64_t *removed) {
    return pcr_api_call(ctx, [&]() -> int {
    const char *call = "point_map_remove_far";
    if (removed) *removed = 0;
    PCR_TRY(pm_check_map(ctx, map, call));
    if (!center3) { ctx->err = "point_map_remove_far: center3 is null"; return PCR_EINVAL; }
    for (int d = 0; d < 3; d++) if (!std::isfinite(center3[d])) { ctx->err = "point_map_remove_far: center3 holds a non-finite value"; return PCR_EINVAL; }
    if (!std::isfinite(max_distance) || !(max_distance > 0.0)) { ctx->err = "point_map_remove_far: max_distance must be finite and greater than 0"; return PCR_EINVAL; }
    PCR_TRY(pcr_arena_reserve(ctx, pm_scratch(map->cells)));
    const int n = (int)map->cells;
    uint8_t *near = arena<uint8_t>(ctx, (size_t)n);
    int *pos = arena<int>(ctx, (size_t)n), *total = arena<int>(ctx, 1);
    if (!near || !pos || !total) return PCR_ENOMEM;
    PCR_LAUNCH(ctx, k_pmap_near, dim3(pm_blocks((size_t)n)), dim3(PM_BS), 0, ctx->stream, map->view.xyz, n, center3[0], center3[1], center3[2], max_distance * max_distance, near);
    PCR_TRY(pcr_dev_flag_scan(ctx, near, nullptr, n, pos, total));
    int64_t kept = 0;
    PCR_TRY(pcr_read_count(ctx, total, &kept));
    if (kept == n) return PCR_OK;                             // every row stays, with its bits and its place
    const PmSources s{map->view.xyz, map->view.nrm, n, nullptr, nullptr, 0};
    PCR_TRY(pm_build(ctx, call, PmSeq{map->keys, nullptr, n}, near, s, map->max_points, pm_kind_of(map), map));
    if (removed) *removed = (int64_t)n - map->cells;
    return PCR_OK;
    });
}

// ================================================================ search and registration: host
int pm_check_search(pcr_context *ctx, const char *call, const pcr_point_map *map, const float *src_xyz, int64_t n_src, const double *T, const char *T_name, int nbh,
                           double max_distance) {
    PCR_TRY(pm_check_map(ctx, map, call));
    PCR_TRY(vg_check_nbh(ctx, call, nbh));
    if (n_src < 0 || (n_src > 0 && !src_xyz) || n_src > 0x7fffffff / 8) { ctx->err = std::string(call) + ": src_xyz is null or too large"; return PCR_EINVAL; }
    if (!std::isfinite(max_distance) || !(max_distance > 0.0)) { ctx->err = std::string(call) + ": max_correspondence_distance must be finite and greater than 0"; return PCR_EINVAL; }
    return vg_check_T(ctx, call, T_name, T);
}
int pm_check_estimation(pcr_context *ctx, const char *call, const pcr_point_map *map, const pcr_estimation *est) {
    if (!est) { ctx->err = std::string(call) + ": estimation is null"; return PCR_EINVAL; }
    if (est->kind != PCR_EST_POINT_TO_POINT && est->kind != PCR_EST_POINT_TO_PLANE) { ctx->err = std::string(call) + ": estimation.kind must be point to point or point to plane"; return PCR_EINVAL; }
    if (est->kind == PCR_EST_POINT_TO_POINT && est->with_scaling) { ctx->err = std::string(call) + ": estimation.with_scaling is not supported (the update is the Gauss-Newton form)"; return PCR_EINVAL; }
    if (est->loss < PCR_LOSS_L2 || est->loss > PCR_LOSS_GM) { ctx->err = std::string(call) + ": estimation.loss is no robust kernel (pcr_loss_kind)"; return PCR_EINVAL; }
    if (!std::isfinite(est->loss_k)) { ctx->err = std::string(call) + ": estimation.loss_k is not finite"; return PCR_EINVAL; }
    if (est->kind == PCR_EST_POINT_TO_PLANE && !map->normals) { ctx->err = std::string(call) + ": point to plane needs a map with normals"; return PCR_EINVAL; }
    return PCR_OK;
}
int pm_check_src_finite(pcr_context *ctx, const char *call, const float *src_xyz, int64_t n_src) {
    const float *ptr[1] = {src_xyz}; const size_t cnt[1] = {(size_t)n_src * 3}; const char *name[1] = {"src_xyz"};
    return vg_check_finite(ctx, call, ptr, cnt, name, 1);
}
size_t pm_search_scratch(int64_t n_src) { return (size_t)(n_src > 0 ? n_src : 1) * 24 + (4u << 20); }

// the rows at the pose T (16 doubles, host) into rows2; scratch from the arena the caller has reserved
// valid_only: a match whose row is not valid (ESTIMATE) is no row
static int pm_rows_at(pcr_context *ctx, const pcr_point_map *map, const float *src_xyz, int64_t n_src, const double *T, int nbh, double max_d2, bool valid_only, int32_t *rows2,
                      int64_t *n_rows) {
    *n_rows = 0;
    if (n_src == 0) return PCR_OK;
    ArenaMark mark(ctx);
    int32_t *match = arena<int32_t>(ctx, (size_t)n_src);
    uint8_t *flags = arena<uint8_t>(ctx, (size_t)n_src);
    if (!match || !flags) return PCR_ENOMEM;
    PmPose pose; memcpy(pose.T, T, sizeof pose.T);
    PCR_LAUNCH(ctx, k_pmap_match, dim3(pm_blocks((size_t)n_src)), dim3(PM_BS), 0, ctx->stream, src_xyz, (int)n_src, pose, map->view, nbh, max_d2, match, flags);
    if (valid_only) PCR_LAUNCH(ctx, k_pmap_drop_invalid, dim3(pm_blocks((size_t)n_src)), dim3(PM_BS), 0, ctx->stream, (const int32_t *)map->ncount, map->est_min, (int)n_src, match, flags);
    return vg_emit_rows(ctx, match, flags, (size_t)n_src, 1, rows2, n_rows);      // (one candidate per source point)
}

extern "C" int pcr_point_map_correspondences(pcr_context *ctx, const pcr_point_map *map, const float *src_xyz, int64_t n_src, const double *T, double max_correspondence_distance,
                                             int neighborhood, int32_t *rows2, int64_t *n_rows) {
    return pcr_api_call(ctx, [&]() -> int {
    const char *call = "point_map_correspondences";
    PCR_TRY(pm_check_search(ctx, call, map, src_xyz, n_src, T, "T", neighborhood, max_correspondence_distance));
    if (!n_rows || (n_src > 0 && !rows2)) { ctx->err = "point_map_correspondences: rows2 / n_rows is null"; return PCR_EINVAL; }
    PCR_TRY(pcr_arena_reserve(ctx, pm_search_scratch(n_src)));
    PCR_TRY(pm_check_src_finite(ctx, call, src_xyz, n_src));
    return pm_rows_at(ctx, map, src_xyz, n_src, T, neighborhood, max_correspondence_distance * max_correspondence_distance, false, rows2, n_rows);
    });
}

extern "C" int pcr_point_map_linearize(pcr_context *ctx, const pcr_point_map *map, const float *src_xyz, int64_t n_src, const double *T, double max_correspondence_distance,
                                       int neighborhood, const pcr_estimation *estimation, double *JTJ, double *JTr, int64_t *rows, double *sum_d2, double *sum_r2) {
    return pcr_api_call(ctx, [&]() -> int {
    const char *call = "point_map_linearize";
    PCR_TRY(pm_check_search(ctx, call, map, src_xyz, n_src, T, "T", neighborhood, max_correspondence_distance));
    PCR_TRY(pm_check_estimation(ctx, call, map, estimation));
    PCR_TRY(pcr_arena_reserve(ctx, pm_search_scratch(n_src)));
    PCR_TRY(pm_check_src_finite(ctx, call, src_xyz, n_src));
    double h[NV];
    PCR_TRY(pmap_loop(ctx, call, src_xyz, n_src, map, neighborhood, max_correspondence_distance * max_correspondence_distance, estimation, T, 0.0, 0.0, 0, true, nullptr, h));
    if (JTJ) {
        int t = 0;
        for (int p = 0; p < 6; p++) for (int q = p; q < 6; q++) { JTJ[p * 6 + q] = h[t]; JTJ[q * 6 + p] = h[t]; t++; }
    }
    if (JTr) for (int p = 0; p < 6; p++) JTr[p] = h[21 + p];
    if (sum_r2) *sum_r2 = h[27];
    if (sum_d2) *sum_d2 = h[28];
    if (rows) *rows = (int64_t)(h[29] + 0.5);
    return PCR_OK;
    });
}

extern "C" int pcr_registration_point_map(pcr_context *ctx, const float *src_xyz, int64_t n_src, const pcr_point_map *map, double max_correspondence_distance,
                                          const double *init_T, const pcr_point_map_params *params, pcr_result *result, int32_t *correspondences) {
    return pcr_api_call(ctx, [&]() -> int {
    const char *call = "registration_point_map";
    if (!params || !result) { ctx->err = "registration_point_map: params / result is null"; return PCR_EINVAL; }
    PCR_TRY(pm_check_search(ctx, call, map, src_xyz, n_src, init_T, "init_T", params->neighborhood, max_correspondence_distance));
    PCR_TRY(pm_check_estimation(ctx, call, map, &params->estimation));
    if (params->max_iteration < 0) { ctx->err = "registration_point_map: params.max_iteration < 0"; return PCR_EINVAL; }
    PCR_TRY(pcr_arena_reserve(ctx, pm_search_scratch(n_src)));
    PCR_TRY(pm_check_src_finite(ctx, call, src_xyz, n_src));
    const double max_d2 = max_correspondence_distance * max_correspondence_distance;
    PCR_TRY(pmap_loop(ctx, call, src_xyz, n_src, map, params->neighborhood, max_d2, &params->estimation, init_T, params->relative_fitness, params->relative_rmse,
                      params->max_iteration, false, result, nullptr));
    if (correspondences) {      // the rows of the last launch: those at the returned pose
        int64_t rows = 0;
        PCR_TRY(pm_rows_at(ctx, map, src_xyz, n_src, result->transformation, params->neighborhood, max_d2, pm_reads_validity(map, &params->estimation), correspondences, &rows));
        if (rows != result->n_correspondences) { ctx->err = "registration_point_map: the correspondence set does not match the last iteration's rows"; return PCR_EHIP; }
    }
    return PCR_OK;
    });
}
