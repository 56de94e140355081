// pcr_nmap.hip -- a normal-distributions map that grows: create on a given grid at a pose, insert a scan, merge two maps, drop far cells.  The rule
// is the statement in include/pcr_hip.h (RULE OF A MAP / MAP ON A GIVEN GRID / MERGE / INSERT / REMOVE_FAR of the NDT section); the map and what
// its kernels share is pcr_ndt.h.  A unit of its own so that the kernels of pcr_ndt.hip and pcr_vmap.hip keep their code.
//   create_on_grid     ndt_map_build (pcr_ndt.hip) with the grid given and the members placed by k_ndt_place
//   insert             the map of the scan on the map's grid by the same builder, then merge, then the scan's map is freed
//   merge              k_nmap_merge_mark: every row searches its key in the other list; the rows of B that A does not hold are flagged and scanned
//                      (pcr_dev_flag_scan), which gives every row its place in the union; k_nmap_merge_write, one lane per row, copies the row
//                      or combines the two cells: the count-weighted mean, the covariances moved to it by the parallel-axis term, and validity
//                      and A_v once more from (N, C) by ndt_cell_information, the function the builder's k_ndt_cell calls
//   remove_far         k_nmap_far_flags, the flag scan, k_nmap_gather
// Every mutating call builds a new block (rows, keys, count word, cell hash by pcr_dev_build_grid_batch), waits for it, swaps it in and frees the old
// one; on an error the map is untouched.  The expressions of the rule are not contracted.
#pragma clang fp contract(off)
#include <cmath>
#include <cstring>
#include "pcr_ndt.h"

#define NM_BS 256

static unsigned nm_blocks(size_t n) { return (unsigned)((n + NM_BS - 1) / NM_BS); }

// the rows of a map on the device, in ascending Morton order of the cell
struct NmRows { const float4 *mean4, *cov8; const double *info6; const uint64_t *keys; int n; };

// ================================================================ kernels
// N_v of a row: the count word carries the validity in its sign
__device__ static inline int nm_count(const float4 m) { const int w = __float_as_int(m.w); return w < 0 ? -w : w; }

// lane t < a.n: row t of A finds where its key stands in B (where[t] = lower bound); lane a.n + j: row j of B finds where it stands in A and is
// flagged when A does not hold its cell.  A shared cell whose counts add up past 2^31 - 1 sets *overflow.
__global__ void __launch_bounds__(NM_BS) k_nmap_merge_mark(NmRows a, NmRows b, int *__restrict__ where, uint8_t *__restrict__ only_b, int *__restrict__ overflow) {
    const int t = blockIdx.x * NM_BS + threadIdx.x;
    if (t >= a.n + b.n) return;
    if (t < a.n) { where[t] = vg_lower_bound(b.keys, b.n, a.keys[t]); return; }
    const int j = t - a.n;
    const uint64_t key = b.keys[j];
    const int i = vg_lower_bound(a.keys, a.n, key);
    const bool shared = i < a.n && a.keys[i] == key;
    where[t] = i;
    only_b[j] = shared ? 0 : 1;
    if (shared && (int64_t)nm_count(a.mean4[i]) + (int64_t)nm_count(b.mean4[j]) > 0x7fffffffll) atomicOr(overflow, 1);
}
// one channel of a cell in both maps: float32((N_a a + N_b b) / N) in float64, the two products, the sum, then the division, then one rounding
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
// the union's rows: row t of A lands at t + (rows of B alone below it), combined with its partner where B holds the cell too; a row of B alone
// lands at (rows of B alone before it) + (rows of A below it)
__global__ void __launch_bounds__(NM_BS) k_nmap_merge_write(NmRows a, NmRows b, const int *__restrict__ where, const uint8_t *__restrict__ only_b,
                                                            const int *__restrict__ pos_b, const int *__restrict__ total_b, int cap, int min_points, double ratio,
                                                            float4 *__restrict__ mean4, float4 *__restrict__ cov8, double *__restrict__ info6, uint64_t *__restrict__ keys) {
#pragma clang fp contract(off)
    const int t = blockIdx.x * NM_BS + threadIdx.x;
    if (t >= a.n + b.n) return;
    float4 m, c0, c1; uint64_t key; int o;
    double A6[6];
    if (t < a.n) {
        const int j = where[t];
        key = a.keys[t]; m = a.mean4[t]; c0 = a.cov8[2 * (size_t)t]; c1 = a.cov8[2 * (size_t)t + 1];
        o = t + (j < b.n ? pos_b[j] : *total_b);
        if (j < b.n && b.keys[j] == key) {
            const float4 mb = b.mean4[j], d0 = b.cov8[2 * (size_t)j], d1 = b.cov8[2 * (size_t)j + 1];
            const int na = nm_count(m), nb = nm_count(mb), n = na + nb;
            const double fa = (double)na, fb = (double)nb, fn = (double)n;
            const float mx = nm_mix(fa, (double)m.x, fb, (double)mb.x, fn), my = nm_mix(fa, (double)m.y, fb, (double)mb.y, fn), mz = nm_mix(fa, (double)m.z, fb, (double)mb.z, fn);
            const double ax = (double)m.x - (double)mx, ay = (double)m.y - (double)my, az = (double)m.z - (double)mz;
            const double bx = (double)mb.x - (double)mx, by = (double)mb.y - (double)my, bz = (double)mb.z - (double)mz;
            c0 = make_float4(nm_cov(fa, c0.x, ax, ax, fb, d0.x, bx, bx, fn), nm_cov(fa, c0.y, ax, ay, fb, d0.y, bx, by, fn), nm_cov(fa, c0.z, ax, az, fb, d0.z, bx, bz, fn),
                             nm_cov(fa, c0.w, ay, ay, fb, d0.w, by, by, fn));
            c1 = make_float4(nm_cov(fa, c1.x, ay, az, fb, d1.x, by, bz, fn), nm_cov(fa, c1.y, az, az, fb, d1.y, bz, bz, fn), 0.0f, 0.0f);
            const bool valid = ndt_cell_information(n, c0, c1, min_points, ratio, A6);
            m = make_float4(mx, my, mz, __int_as_float(valid ? n : -n));
        } else {
#pragma unroll
            for (int k = 0; k < 6; k++) A6[k] = a.info6[6 * (size_t)t + k];
        }
    } else {
        const int j = t - a.n;
        if (!only_b[j]) return;
        key = b.keys[j]; m = b.mean4[j]; c0 = b.cov8[2 * (size_t)j]; c1 = b.cov8[2 * (size_t)j + 1];
#pragma unroll
        for (int k = 0; k < 6; k++) A6[k] = b.info6[6 * (size_t)j + k];
        o = pos_b[j] + where[t];
    }
    if (o < 0 || o >= cap) return;
    mean4[o] = m; cov8[2 * (size_t)o] = c0; cov8[2 * (size_t)o + 1] = c1; keys[o] = key;
#pragma unroll
    for (int k = 0; k < 6; k++) info6[6 * (size_t)o + k] = A6[k];
}

// keep[v] = d^2 < r^2 (vg_within, pcr_vgicp.h: the voxel covariance map's test; the count word in p.w plays no part)
__global__ void __launch_bounds__(NM_BS) k_nmap_far_flags(const float4 *__restrict__ mean4, int n, double cx, double cy, double cz, double r2, uint8_t *__restrict__ keep) {
    const int v = blockIdx.x * NM_BS + threadIdx.x;
    if (v >= n) return;
    keep[v] = vg_within(mean4[v], cx, cy, cz, r2) ? 1 : 0;
}
__global__ void __launch_bounds__(NM_BS) k_nmap_gather(NmRows a, const uint8_t *__restrict__ keep, const int *__restrict__ pos, int cap, float4 *__restrict__ mean4,
                                                       float4 *__restrict__ cov8, double *__restrict__ info6, uint64_t *__restrict__ keys) {
    const int v = blockIdx.x * NM_BS + threadIdx.x;
    if (v >= a.n || !keep[v]) return;
    const int o = pos[v];
    if (o < 0 || o >= cap) return;
    mean4[o] = a.mean4[v]; cov8[2 * (size_t)o] = a.cov8[2 * (size_t)v]; cov8[2 * (size_t)o + 1] = a.cov8[2 * (size_t)v + 1]; keys[o] = a.keys[v];
#pragma unroll
    for (int k = 0; k < 6; k++) info6[6 * (size_t)o + k] = a.info6[6 * (size_t)v + k];
}

// ================================================================ host
static NmRows nm_rows_of(const pcr_ndt_map *m) { return NmRows{m->view.mean4, m->view.cov8, m->view.info6, m->keys, (int)m->cells}; }

// scratch of the context's arena that a merge or a trim of `cells` rows takes (where, positions, flags, the scan's and the hash build's own)
static size_t nm_scratch(int64_t cells) { return (size_t)cells * 32 + (4u << 20); }

// A new block of `cells` rows: `fill` enqueues what writes the rows and the keys; then the count word and the cell hash.  Finished (the stream is
// idle) when it returns PCR_OK; on an error nothing of it is left.
struct NmBlock { char *block = nullptr; size_t bytes = 0; float4 *mean4 = nullptr, *cov8 = nullptr; double *info6 = nullptr; uint64_t *keys = nullptr; int *n_dev = nullptr; GridView gv; };
template <class Fill> static int nm_build_block(pcr_context *ctx, const char *call, int64_t cells, NmBlock *b, Fill &&fill) {
    b->bytes = ndt_block_bytes(cells);
    if (hipMalloc((void **)&b->block, b->bytes) != hipSuccess) { b->block = nullptr; ctx->err = std::string("hipMalloc(") + call + ")"; return PCR_ENOMEM; }
    auto body = [&]() -> int {
        SideLane own(ctx, b->block, b->bytes, ctx->stream);      // the rows and the hash table come out of the block, on the call's own stream
        b->mean4 = arena<float4>(ctx, (size_t)cells); b->cov8 = arena<float4>(ctx, 2 * (size_t)cells); b->info6 = arena<double>(ctx, 6 * (size_t)cells);
        b->keys = arena<uint64_t>(ctx, (size_t)cells); b->n_dev = arena<int>(ctx, 1);
        if (!b->mean4 || !b->cov8 || !b->info6 || !b->keys || !b->n_dev) return PCR_ENOMEM;
        PCR_TRY(fill(*b));
        PCR_HIP_CHECK(ctx, hipMemsetD32Async((hipDeviceptr_t)b->n_dev, (int)cells, 1, ctx->stream));
        DevCloud mc;                                             // the cells as a voxel-lattice cloud: what the hash build reads (keys, count, capacity)
        mc.keys = b->keys; mc.n = b->n_dev; mc.cap = (int)cells; mc.voxel_lattice = true;
        const DevCloud *pmc = &mc; const int level = 0;
        PCR_TRY(pcr_dev_build_grid_batch(ctx, &pmc, &level, 1, &b->gv));
        if (!b->gv.tab) { ctx->err = std::string(call) + ": no cell hash"; return PCR_EHIP; }
        PCR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        if (ctx->launch_err != hipSuccess) return PCR_EHIP;      // (pcr_leave names the launch)
        return PCR_OK;
    };
    const int rc = body();
    if (rc != PCR_OK) { (void)hipStreamSynchronize(ctx->stream); (void)hipFree(b->block); b->block = nullptr; }
    return rc;
}
// the new block in, the old one out (hipFree waits for the device: no call is still reading the old block)
static void nm_adopt(pcr_ndt_map *m, const NmBlock &b, int64_t cells) {
    char *old = m->block;
    m->cells = cells; m->block = b.block; m->bytes = b.bytes; m->keys = b.keys; m->n_dev = b.n_dev;
    m->view.tab = b.gv.tab; m->view.dmask = b.gv.dmask; m->view.mean4 = b.mean4; m->view.cov8 = b.cov8; m->view.info6 = b.info6;
    (void)hipFree(old);
}

// map <- MERGE(map, b); b's rows live in another map.  Reserves the arena for itself.
static int nm_merge_into(pcr_context *ctx, const char *call, pcr_ndt_map *map, const NmRows &b) {
    const NmRows a = nm_rows_of(map);
    const size_t total = (size_t)a.n + (size_t)b.n;
    if (total > (size_t)(0x7fffffff / 8)) { ctx->err = std::string(call) + ": the merged map would hold 2^28 rows or more"; return PCR_EINVAL; }
    PCR_TRY(pcr_arena_reserve(ctx, nm_scratch((int64_t)total)));
    int *where = arena<int>(ctx, total), *pos_b = arena<int>(ctx, (size_t)b.n), *word = arena<int>(ctx, 2);
    uint8_t *only_b = arena<uint8_t>(ctx, (size_t)b.n);
    if (!where || !pos_b || !word || !only_b) return PCR_ENOMEM;
    int *total_b = word, *overflow = word + 1;
    PCR_HIP_CHECK(ctx, hipMemsetAsync(word, 0, 2 * sizeof(int), ctx->stream));
    PCR_LAUNCH(ctx, k_nmap_merge_mark, dim3(nm_blocks(total)), dim3(NM_BS), 0, ctx->stream, a, b, where, only_b, overflow);
    PCR_TRY(pcr_dev_flag_scan(ctx, only_b, nullptr, b.n, pos_b, total_b));
    int h[2] = {0, 0};
    PCR_HIP_CHECK(ctx, hipMemcpyAsync(h, word, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
    PCR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    if (h[1]) { ctx->err = std::string(call) + ": the member count of a cell would pass 2^31 - 1"; return PCR_EINVAL; }
    if (h[0] < 0 || h[0] > b.n) { ctx->err = std::string(call) + ": the scan of the new cells is out of range"; return PCR_EHIP; }
    const int64_t cells = (int64_t)a.n + h[0];
    NmBlock nb;
    PCR_TRY(nm_build_block(ctx, call, cells, &nb, [&](const NmBlock &o) -> int {
        PCR_LAUNCH(ctx, k_nmap_merge_write, dim3(nm_blocks(total)), dim3(NM_BS), 0, ctx->stream, a, b, (const int *)where, (const uint8_t *)only_b, (const int *)pos_b,
                   (const int *)total_b, (int)cells, map->min_points, map->ratio, o.mean4, o.cov8, o.info6, o.keys);
        return PCR_OK;
    }));
    nm_adopt(map, nb, cells);
    return PCR_OK;
}

extern "C" int pcr_ndt_map_create_on_grid(pcr_context *ctx, const float *xyz, int64_t n, double voxel_size, int min_points_per_voxel, double eigenvalue_ratio,
                                          const double *grid_min3, const double *T, pcr_ndt_map **out) {
    return pcr_api_call(ctx, [&]() -> int {
    const char *call = "ndt_map_create_on_grid";
    if (!out) { ctx->err = "ndt_map_create_on_grid: out is null"; return PCR_EINVAL; }
    *out = nullptr;
    if (!grid_min3) { ctx->err = "ndt_map_create_on_grid: grid_min3 is null"; return PCR_EINVAL; }
    for (int d = 0; d < 3; d++) if (!std::isfinite(grid_min3[d])) { ctx->err = "ndt_map_create_on_grid: grid_min3 holds a non-finite value"; return PCR_EINVAL; }
    if (T) PCR_TRY(vg_check_T(ctx, call, "T", T));
    static const double eye[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};      // no pose is the identity, applied all the same
    return ndt_map_build(ctx, call, xyz, n, voxel_size, min_points_per_voxel, eigenvalue_ratio, grid_min3, T ? T : eye, out);
    });
}

extern "C" int pcr_ndt_map_insert(pcr_context *ctx, pcr_ndt_map *map, const float *xyz, int64_t n, const double *T) {
    return pcr_api_call(ctx, [&]() -> int {
    const char *call = "ndt_map_insert";
    PCR_TRY(ndt_check_map(ctx, map, call));
    if (T) PCR_TRY(vg_check_T(ctx, call, "T", T));
    static const double eye[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    pcr_ndt_map *scan = nullptr;      // INSERT is MERGE with the map of the scan: built by the one builder, merged, freed
    PCR_TRY(ndt_map_build(ctx, call, xyz, n, map->view.voxel, map->min_points, map->ratio, map->grid_min, T ? T : eye, &scan));
    const int rc = nm_merge_into(ctx, call, map, nm_rows_of(scan));
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
    return nm_merge_into(ctx, call, map, nm_rows_of(other));
    });
}

extern "C" int pcr_ndt_map_remove_far(pcr_context *ctx, pcr_ndt_map *map, const double *center3, double max_distance, int64_t *removed) {
    return pcr_api_call(ctx, [&]() -> int {
    const char *call = "ndt_map_remove_far";
    if (removed) *removed = 0;
    PCR_TRY(ndt_check_map(ctx, map, call));
    if (!center3) { ctx->err = "ndt_map_remove_far: center3 is null"; return PCR_EINVAL; }
    for (int d = 0; d < 3; d++) if (!std::isfinite(center3[d])) { ctx->err = "ndt_map_remove_far: center3 holds a non-finite value"; return PCR_EINVAL; }
    if (!std::isfinite(max_distance) || !(max_distance > 0.0)) { ctx->err = "ndt_map_remove_far: max_distance must be finite and greater than 0"; return PCR_EINVAL; }
    PCR_TRY(pcr_arena_reserve(ctx, nm_scratch(map->cells)));
    const NmRows a = nm_rows_of(map);
    uint8_t *keep = arena<uint8_t>(ctx, (size_t)a.n);
    int *pos = arena<int>(ctx, (size_t)a.n), *total = arena<int>(ctx, 1);
    if (!keep || !pos || !total) return PCR_ENOMEM;
    const double r2 = max_distance * max_distance;
    PCR_LAUNCH(ctx, k_nmap_far_flags, dim3(nm_blocks((size_t)a.n)), dim3(NM_BS), 0, ctx->stream, a.mean4, a.n, center3[0], center3[1], center3[2], r2, keep);
    PCR_TRY(pcr_dev_flag_scan(ctx, keep, nullptr, a.n, pos, total));
    int64_t kept = 0;
    PCR_TRY(pcr_read_count(ctx, total, &kept));
    if (kept < 0 || kept > a.n) { ctx->err = "ndt_map_remove_far: the scan of the kept rows is out of range"; return PCR_EHIP; }
    if (kept == 0) { ctx->err = "ndt_map_remove_far: would leave the map empty"; return PCR_EINVAL; }
    if (kept == a.n) return PCR_OK;                           // every row stays, with its bits and its place
    NmBlock nb;
    PCR_TRY(nm_build_block(ctx, call, kept, &nb, [&](const NmBlock &o) -> int {
        PCR_LAUNCH(ctx, k_nmap_gather, dim3(nm_blocks((size_t)a.n)), dim3(NM_BS), 0, ctx->stream, a, (const uint8_t *)keep, (const int *)pos, (int)kept, o.mean4, o.cov8, o.info6, o.keys);
        return PCR_OK;
    }));
    if (removed) *removed = (int64_t)a.n - kept;
    nm_adopt(map, nb, kept);
    return PCR_OK;
    });
}

extern "C" int pcr_ndt_map_rule(const pcr_ndt_map *map, double *grid_min3, int *min_points_per_voxel, double *eigenvalue_ratio) {
    if (!map) return PCR_EINVAL;
    if (grid_min3) memcpy(grid_min3, map->grid_min, sizeof map->grid_min);
    if (min_points_per_voxel) *min_points_per_voxel = map->min_points;
    if (eigenvalue_ratio) *eigenvalue_ratio = map->ratio;
    return PCR_OK;
}
