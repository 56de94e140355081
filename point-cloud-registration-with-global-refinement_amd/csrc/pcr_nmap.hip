// pcr_nmap.hip -- a normal-distributions map that grows: create on a given grid at a pose, insert a scan, merge two maps, drop far cells.  The rule
// is the statement in include/pcr_hip.h (RULE OF A MAP / MAP ON A GIVEN GRID / MERGE / INSERT / REMOVE_FAR of the NDT section); the map and what
// its kernels share is pcr_ndt.h.  A unit of its own so that the kernels of pcr_ndt.hip and pcr_vmap.hip keep their code.
//   create_on_grid     ndt_map_build (pcr_ndt.hip) with the grid given and the members placed by k_ndt_place
//   insert             the map of the scan on the map's grid by the same builder, then merge, then the scan's map is freed
//   merge, remove_far  the frame of the maps that grow (pcr_mapgrow.h: k_map_merge_mark, k_map_merge_write, k_map_far_flags, k_map_gather, the block
//                      builder, map_merge_into, map_remove_far) with the row policy NmapRow (pcr_ndt.h); what is this map's own is
//                      NmapRow::combine: the count-weighted mean, the covariances moved to it by the parallel-axis term, and validity and A_v
//                      once more from (N, C) by ndt_cell_information, the function the builder's k_ndt_cell calls
// Every mutating call builds a new block (rows, keys, count word, cell hash), waits for it, swaps it in and frees the old one; on an error the map
// is untouched.  The expressions of the rule are not contracted.
#pragma clang fp contract(off)
#include <cmath>
#include <cstring>
#include "pcr_ndt.h"
#include "pcr_mapgrow.h"

// ================================================================ a cell in both maps
// one channel: float32((N_a a + N_b b) / N) in float64, the two products, the sum, then the division, then one rounding
__device__ static inline float nm_mix(double na, double a, double nb, double b, double n) {
#pragma clang fp contract(off)
    const double pa = na * a, pb = nb * b;
    const double s = pa + pb;
    return (float)(s / n);
}
// one covariance channel rc: M = float64(C[rc]) + d[r] d[c] about the new mean for either cell (the product rounded first), then nm_mix
__device__ static inline float nm_cov(double na, float ca, double dar, double dac, double nb, float cb, double dbr, double dbc, double n) {
#pragma clang fp contract(off)
    const double qa = dar * dac, qb = dbr * dbc;
    const double ma = (double)ca + qa, mb = (double)cb + qb;
    return nm_mix(na, ma, nb, mb, n);
}
__device__ inline void NmapRow::combine(const Merged &g, float4 &m, float4 &c0, float4 &c1, double *A6, const float4 mb, const float4 d0, const float4 d1) {
#pragma clang fp contract(off)
    const int na = count(m), nb = count(mb), n = na + nb;
    const double fa = (double)na, fb = (double)nb, fn = (double)n;
    const float mx = nm_mix(fa, (double)m.x, fb, (double)mb.x, fn), my = nm_mix(fa, (double)m.y, fb, (double)mb.y, fn), mz = nm_mix(fa, (double)m.z, fb, (double)mb.z, fn);
    const double ax = (double)m.x - (double)mx, ay = (double)m.y - (double)my, az = (double)m.z - (double)mz;
    const double bx = (double)mb.x - (double)mx, by = (double)mb.y - (double)my, bz = (double)mb.z - (double)mz;
    c0 = make_float4(nm_cov(fa, c0.x, ax, ax, fb, d0.x, bx, bx, fn), nm_cov(fa, c0.y, ax, ay, fb, d0.y, bx, by, fn), nm_cov(fa, c0.z, ax, az, fb, d0.z, bx, bz, fn),
                     nm_cov(fa, c0.w, ay, ay, fb, d0.w, by, by, fn));
    c1 = make_float4(nm_cov(fa, c1.x, ay, az, fb, d1.x, by, bz, fn), nm_cov(fa, c1.y, az, az, fb, d1.y, bz, bz, fn), 0.0f, 0.0f);
    const bool valid = ndt_cell_information(n, c0, c1, g.min_points, g.ratio, A6);
    m = make_float4(mx, my, mz, __int_as_float(valid ? n : -n));
}

// ================================================================ host
// scratch of the context's arena that a merge or a trim of `cells` rows takes (where, positions, flags, the scan's and the hash build's own)
static size_t nm_scratch(int64_t cells) { return (size_t)cells * 32 + (4u << 20); }

extern "C" int pcr_ndt_map_create_on_grid(pcr_context *ctx, const float *xyz, int64_t n, double voxel_size, int min_points_per_voxel, double eigenvalue_ratio,
                                          const double *grid_min3, const double *T, pcr_ndt_map **out) {
    return pcr_api_call(ctx, [&]() -> int {
    const char *call = "ndt_map_create_on_grid";
    if (!out) { ctx->err = "ndt_map_create_on_grid: out is null"; return PCR_EINVAL; }
    *out = nullptr;
    PCR_TRY(vg_check_grid_min(ctx, call, grid_min3));
    if (T) PCR_TRY(vg_check_T(ctx, call, "T", T));
    return ndt_map_build(ctx, call, xyz, n, voxel_size, min_points_per_voxel, eigenvalue_ratio, grid_min3, T ? T : vg_eye, out);
    });
}

extern "C" int pcr_ndt_map_insert(pcr_context *ctx, pcr_ndt_map *map, const float *xyz, int64_t n, const double *T) {
    return pcr_api_call(ctx, [&]() -> int {
    const char *call = "ndt_map_insert";
    PCR_TRY(ndt_check_map(ctx, map, call));
    if (T) PCR_TRY(vg_check_T(ctx, call, "T", T));
    pcr_ndt_map *scan = nullptr;      // INSERT is MERGE with the map of the scan: built by the one builder, merged, freed
    PCR_TRY(ndt_map_build(ctx, call, xyz, n, map->view.voxel, map->min_points, map->ratio, map->grid_min, T ? T : vg_eye, &scan));
    int rc = pcr_arena_reserve(ctx, nm_scratch(map->cells + scan->cells));      // (the scan's rows lie in its own block, not in the arena)
    if (rc == PCR_OK) rc = map_merge_into<NmapRow>(ctx, call, map, NmapRow::rows_of(scan));
    (void)hipFree(scan->block);
    delete scan;
    return rc;
    });
}

extern "C" int pcr_ndt_map_merge(pcr_context *ctx, pcr_ndt_map *map, const pcr_ndt_map *other) {
    return pcr_api_call(ctx, [&]() -> int {
    const char *call = "ndt_map_merge";
    PCR_TRY(ndt_check_map(ctx, map, call));
    if (!other || !other->block) { ctx->err = "ndt_map_merge: other is null"; return PCR_EINVAL; }
    if (other == map) { ctx->err = "ndt_map_merge: other is the map itself"; return PCR_EINVAL; }
    if (other->device != ctx->device) { ctx->err = "ndt_map_merge: other lives on another device than the context"; return PCR_EINVAL; }
    if (memcmp(&map->view.voxel, &other->view.voxel, sizeof(double)) != 0 || memcmp(map->grid_min, other->grid_min, sizeof map->grid_min) != 0) {
        ctx->err = "ndt_map_merge: other is not on the map's grid (voxel size and grid_min must be equal bit for bit)"; return PCR_EINVAL;
    }
    if (map->min_points != other->min_points || memcmp(&map->ratio, &other->ratio, sizeof(double)) != 0) {
        ctx->err = "ndt_map_merge: other does not follow the map's rule (min_points_per_voxel and eigenvalue_ratio must be equal bit for bit)"; return PCR_EINVAL;
    }
    PCR_TRY(pcr_arena_reserve(ctx, nm_scratch(map->cells + other->cells)));
    return map_merge_into<NmapRow>(ctx, call, map, NmapRow::rows_of(other));
    });
}

extern "C" int pcr_ndt_map_remove_far(pcr_context *ctx, pcr_ndt_map *map, const double *center3, double max_distance, int64_t *removed) {
    return pcr_api_call(ctx, [&]() -> int {
    const char *call = "ndt_map_remove_far";
    if (removed) *removed = 0;
    PCR_TRY(ndt_check_map(ctx, map, call));
    return map_remove_far<NmapRow>(ctx, call, map, center3, max_distance, removed, nm_scratch(map->cells));
    });
}

extern "C" int pcr_ndt_map_rule(const pcr_ndt_map *map, double *grid_min3, int *min_points_per_voxel, double *eigenvalue_ratio) {
    if (!map) return PCR_EINVAL;
    if (grid_min3) memcpy(grid_min3, map->grid_min, sizeof map->grid_min);
    if (min_points_per_voxel) *min_points_per_voxel = map->min_points;
    if (eigenvalue_ratio) *eigenvalue_ratio = map->ratio;
    return PCR_OK;
}
