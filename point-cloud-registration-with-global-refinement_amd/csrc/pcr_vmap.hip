// pcr_vmap.hip -- a voxel covariance map that grows: create on a given grid at a pose, insert a scan, merge two maps, drop far cells.  The rule is
// the statement in include/pcr_hip.h (GRID / MAP ON A GIVEN GRID / MERGE / INSERT / REMOVE_FAR); the map and what its kernels share is pcr_vgicp.h.
// A unit of its own so that the kernels of pcr_vgicp.hip keep their code.
//   k_vmap_place       one lane per point: p' = float32(T p), C' = float32((R C) R^T) of the member covariance, as the two 3-vectors the voxel pass carries
//   rows of a cloud    one voxel pass for all nine channels: k_vmap_keys (the keys of k_voxel_keys on the map's grid), the project's stable radix sort,
//                      k_vmap_heads and the flag scan, k_vmap_cell_rows (float64 sums over the members in input order; the count is the segment length)
//   merge, remove_far  the frame of the maps that grow (pcr_mapgrow.h: k_map_merge_mark, k_map_merge_write, k_map_far_flags, k_map_gather, the block
//                      builder, map_merge_into, map_remove_far) with the row policy VmapRow (pcr_vgicp.h); what is this map's own is
//                      VmapRow::combine, the count-weighted mean of the nine channels of a cell that both maps hold
// Every mutating call builds a new block (rows, keys, count word, cell hash), waits for it, swaps it in and frees the old one; on an error the map
// is untouched.  The expressions of the rule are not contracted.
#pragma clang fp contract(off)
#include <cmath>
#include <cstring>
#include "pcr_mapgrow.h"

#define VM_BS 256

static unsigned vm_blocks(size_t n) { return (unsigned)((n + VM_BS - 1) / VM_BS); }

typedef VmapRow::Rows VmRows;      // what a map holds, and what a scan becomes before it is merged
struct VmPose { double T[12]; };

// ================================================================ kernels
// p' = float32(q) with q the ROWS expression (vg_transform); C' = float32((R C) R^T) of the float32 member covariance, R the upper 3x3 of the pose.
// bad: set when a placed coordinate is not finite (a pose whose products overflow)
__global__ void __launch_bounds__(VM_BS) k_vmap_place(const float *__restrict__ xyz, const float *__restrict__ cov6, int n, VmPose pose, float *__restrict__ out_xyz,
                                                      float *__restrict__ lo3, float *__restrict__ hi3, int *__restrict__ bad) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * VM_BS + threadIdx.x;
    if (i >= n) return;
    vg_place_point(pose.T, xyz, i, out_xyz, bad);
    const float *c = cov6 + (size_t)i * 6;
    const double C[9] = {c[0], c[1], c[2], c[1], c[3], c[4], c[2], c[4], c[5]};
    const double R[9] = {pose.T[0], pose.T[1], pose.T[2], pose.T[4], pose.T[5], pose.T[6], pose.T[8], pose.T[9], pose.T[10]};
    double RC[9], Cr[9];
    vg_mul3(R, C, RC);
    vg_mul3_bt(RC, R, Cr);
    lo3[(size_t)i * 3] = (float)Cr[0]; lo3[(size_t)i * 3 + 1] = (float)Cr[1]; lo3[(size_t)i * 3 + 2] = (float)Cr[2];
    hi3[(size_t)i * 3] = (float)Cr[4]; hi3[(size_t)i * 3 + 1] = (float)Cr[5]; hi3[(size_t)i * 3 + 2] = (float)Cr[8];
}

// the Morton key of every point's cell on the map's grid (k_voxel_keys' float64 expression; the caller has checked that no index is negative or
// past 2^21) and the point's index as the value the stable sort carries
__global__ void __launch_bounds__(VM_BS) k_vmap_keys(const float *__restrict__ xyz, int n, double ox, double oy, double oz, double voxel,
                                                     uint64_t *__restrict__ keys, uint32_t *__restrict__ vals) {
    const int i = blockIdx.x * VM_BS + threadIdx.x;
    if (i >= n) return;
    const double x = (double)xyz[(size_t)i * 3], y = (double)xyz[(size_t)i * 3 + 1], z = (double)xyz[(size_t)i * 3 + 2];
    const uint32_t ix = (uint32_t)(int)floor((x - ox) / voxel), iy = (uint32_t)(int)floor((y - oy) / voxel), iz = (uint32_t)(int)floor((z - oz) / voxel);
    keys[i] = pcr_morton3(ix, iy, iz);
    vals[i] = (uint32_t)i;
}
__global__ void __launch_bounds__(VM_BS) k_vmap_heads(const uint64_t *__restrict__ keys, int n, uint8_t *__restrict__ head) {
    const int i = blockIdx.x * VM_BS + threadIdx.x;
    if (i < n) head[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1 : 0;
}
// one lane per cell (the first of its sorted keys): the float64 sums of the nine channels over the members in input order (the sort is stable),
// divided by the count and rounded to float32 once, as k_voxel_mean does for a point and one attribute; the count is the segment's length
__global__ void __launch_bounds__(VM_BS) k_vmap_cell_rows(const float *__restrict__ xyz, const float *__restrict__ lo3, const float *__restrict__ hi3,
                                                          const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals, const uint8_t *__restrict__ head,
                                                          const int *__restrict__ pos, int n, float4 *__restrict__ mean4, float4 *__restrict__ cov8,
                                                          uint64_t *__restrict__ out_keys) {
    const int i = blockIdx.x * VM_BS + threadIdx.x;
    if (i >= n || !head[i]) return;
    const uint64_t key = keys[i];
    double s[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    int j = i;
    do {
        const size_t v = (size_t)vals[j] * 3;
#pragma unroll
        for (int t = 0; t < 3; t++) { s[t] += (double)xyz[v + t]; s[3 + t] += (double)lo3[v + t]; s[6 + t] += (double)hi3[v + t]; }
        j++;
    } while (j < n && keys[j] == key);
    const double c = (double)(j - i);
    const int o = pos[i];
    mean4[o] = make_float4((float)(s[0] / c), (float)(s[1] / c), (float)(s[2] / c), __int_as_float(j - i));
    cov8[2 * (size_t)o] = make_float4((float)(s[3] / c), (float)(s[4] / c), (float)(s[5] / c), (float)(s[6] / c));
    cov8[2 * (size_t)o + 1] = make_float4((float)(s[7] / c), (float)(s[8] / c), 0.0f, 0.0f);
    out_keys[o] = key;
}

// one channel of a cell in both maps: float32((N_a a + N_b b) / N) in float64, the sum, then the division, then one rounding
__device__ static inline float vm_mix(double na, float a, double nb, float b, double n) {
#pragma clang fp contract(off)
    const double pa = na * (double)a, pb = nb * (double)b;
    const double s = pa + pb;
    return (float)(s / n);
}
__device__ static inline float4 vm_mix4(double na, float4 a, double nb, float4 b, double n) {
    return make_float4(vm_mix(na, a.x, nb, b.x, n), vm_mix(na, a.y, nb, b.y, n), vm_mix(na, a.z, nb, b.z, n), vm_mix(na, a.w, nb, b.w, n));
}
// a cell in both maps: the counts add up, every one of the nine channels is the count-weighted mean
__device__ inline void VmapRow::combine(const Merged &, float4 &m, float4 &c0, float4 &c1, double *, const float4 mb, const float4 d0, const float4 d1) {
    const int na = __float_as_int(m.w), nb = __float_as_int(mb.w), n = na + nb;
    const double fa = (double)na, fb = (double)nb, fn = (double)n;
    m = make_float4(vm_mix(fa, m.x, fb, mb.x, fn), vm_mix(fa, m.y, fb, mb.y, fn), vm_mix(fa, m.z, fb, mb.z, fn), __int_as_float(n));
    c0 = vm_mix4(fa, c0, fb, d0, fn);
    c1 = make_float4(vm_mix(fa, c1.x, fb, d1.x, fn), vm_mix(fa, c1.y, fb, d1.y, fn), 0.0f, 0.0f);
}

// ================================================================ host
struct VmGrid { double grid_min[3], voxel; };
static void vm_origin(const VmGrid &g, double *org) { for (int d = 0; d < 3; d++) org[d] = g.grid_min[d] - g.voxel * 0.5; }      // (pcr_dev_voxel's expression)

// scratch of the context's arena that the rows of an n-point cloud take (placed points, covariances, the voxel pass, rows) plus a merge with `cells` rows
static size_t vm_scratch(int64_t n, int64_t cells) { return 2 * pcr_scratch_bytes_for(n) + (size_t)n * 256 + (size_t)cells * 16 + (4u << 20); }

static int vm_check_cloud(pcr_context *ctx, const char *call, const float *xyz, const float *cov6, const float *normals, int64_t n, double epsilon, const double *T) {
    if (!std::isfinite(epsilon)) { ctx->err = std::string(call) + ": epsilon is not finite"; return PCR_EINVAL; }
    if (n < 1 || n > 0x7fffffff / 8 || !xyz) { ctx->err = std::string(call) + ": xyz must hold 1 .. 2^28 - 1 points"; return PCR_EINVAL; }
    if ((cov6 != nullptr) == (normals != nullptr)) { ctx->err = std::string(call) + ": exactly one of cov6 / normals must be given"; return PCR_EINVAL; }
    if (T) PCR_TRY(vg_check_T(ctx, call, "T", T));
    return PCR_OK;
}

// The rows of the MAP ON A GIVEN GRID rule for a cloud, in the context's arena (reserved by the caller).  PCR_EINVAL when a member leaves the grid.
static int vm_cloud_rows(pcr_context *ctx, const char *call, const float *xyz, const float *cov6, const float *normals, int64_t n, double epsilon, const double *T,
                         const VmGrid &g, VmRows *out) {
    {
        const float *ptr[3] = {xyz, cov6, normals}; const size_t cnt[3] = {(size_t)n * 3, (size_t)n * 6, (size_t)n * 3}; const char *name[3] = {"xyz", "cov6", "normals"};
        PCR_TRY(vg_check_finite(ctx, call, ptr, cnt, name, 3));
    }
    VmPose pose;
    memcpy(pose.T, T ? T : vg_eye, sizeof pose.T);
    const float *member = cov6;
    if (!member) {
        float *c6 = arena<float>(ctx, (size_t)n * 6);
        if (!c6) return PCR_ENOMEM;
        PCR_TRY(vg_member_cov6(ctx, nullptr, normals, epsilon, n, c6));
        member = c6;
    }
    float *placed = arena<float>(ctx, (size_t)n * 3), *lo3 = arena<float>(ctx, (size_t)n * 3), *hi3 = arena<float>(ctx, (size_t)n * 3);
    int *bad = arena<int>(ctx, 1);
    if (!placed || !lo3 || !hi3 || !bad) return PCR_ENOMEM;
    PCR_HIP_CHECK(ctx, hipMemsetAsync(bad, 0, sizeof(int), ctx->stream));
    PCR_LAUNCH(ctx, k_vmap_place, dim3(vm_blocks((size_t)n)), dim3(VM_BS), 0, ctx->stream, xyz, member, (int)n, pose, placed, lo3, hi3, bad);
    // both ends of the placed points in one read-back; the lower end against the origin before any key is formed (k_voxel_keys has no defence
    // against a negative index), the upper end as pcr_dev_voxel checks it
    double pb[6], org[3];
    PCR_TRY(pcr_dev_bounds(ctx, placed, n, pb));
    int64_t nonfinite = 0;
    PCR_TRY(pcr_read_count(ctx, bad, &nonfinite));
    vm_origin(g, org);
    if (nonfinite != 0 || !vg_inside_grid(pb, g.grid_min, g.voxel)) { ctx->err = std::string(call) + ": xyz lies outside the map's grid (cell indices must stay in [0, 2^21) on every axis)"; return PCR_EINVAL; }
    // one voxel pass for all nine channels: the keys of k_voxel_keys on the map's grid, the project's stable sort (members of a cell stay in input
    // order), head flags and their scan, and one lane per cell that sums its members.  Rows (cap n) in the arena; the count comes back once.
    uint32_t top = 0;
    for (int d = 0; d < 3; d++) { const uint32_t e = (uint32_t)floor((pb[3 + d] - org[d]) / g.voxel); top = e > top ? e : top; }
    int end_bit = 0;
    while (top) { end_bit += 3; top >>= 1; }
    uint64_t *k0 = arena<uint64_t>(ctx, (size_t)n), *k1 = arena<uint64_t>(ctx, (size_t)n), *keys = arena<uint64_t>(ctx, (size_t)n);
    uint32_t *v0 = arena<uint32_t>(ctx, (size_t)n), *v1 = arena<uint32_t>(ctx, (size_t)n);
    uint8_t *head = arena<uint8_t>(ctx, (size_t)n);
    int *pos = arena<int>(ctx, (size_t)n), *total = arena<int>(ctx, 1);
    float4 *mean4 = arena<float4>(ctx, (size_t)n), *cov8 = arena<float4>(ctx, 2 * (size_t)n);
    const size_t tb = pcr_sort_temp_bytes((size_t)n);
    void *temp = pcr_arena_alloc(ctx, tb);
    if (!k0 || !k1 || !keys || !v0 || !v1 || !head || !pos || !total || !mean4 || !cov8 || !temp) return PCR_ENOMEM;
    PCR_LAUNCH(ctx, k_vmap_keys, dim3(vm_blocks((size_t)n)), dim3(VM_BS), 0, ctx->stream, (const float *)placed, (int)n, org[0], org[1], org[2], g.voxel, k0, v0);
    PCR_TRY(pcr_sort_pairs(ctx, temp, tb, k0, k1, v0, v1, (size_t)n, end_bit));
    PCR_LAUNCH(ctx, k_vmap_heads, dim3(vm_blocks((size_t)n)), dim3(VM_BS), 0, ctx->stream, (const uint64_t *)k1, (int)n, head);
    PCR_TRY(pcr_dev_flag_scan(ctx, head, nullptr, (int)n, pos, total));
    PCR_LAUNCH(ctx, k_vmap_cell_rows, dim3(vm_blocks((size_t)n)), dim3(VM_BS), 0, ctx->stream, (const float *)placed, (const float *)lo3, (const float *)hi3,
               (const uint64_t *)k1, (const uint32_t *)v1, (const uint8_t *)head, (const int *)pos, (int)n, mean4, cov8, keys);
    int64_t cells = 0;
    PCR_TRY(pcr_read_count(ctx, total, &cells));
    if (cells < 1 || cells > n) { ctx->err = std::string(call) + ": the voxel pass returned no cells"; return PCR_EHIP; }
    *out = VmRows{mean4, cov8, keys, (int)cells};
    return PCR_OK;
}

static int vm_copy_rows(pcr_context *ctx, const VmRows &r, const VmapRow::Out &o) {
    PCR_HIP_CHECK(ctx, hipMemcpyAsync(o.mean4, r.mean4, sizeof(float4) * (size_t)r.n, hipMemcpyDeviceToDevice, ctx->stream));
    PCR_HIP_CHECK(ctx, hipMemcpyAsync(o.cov8, r.cov8, sizeof(float4) * 2 * (size_t)r.n, hipMemcpyDeviceToDevice, ctx->stream));
    PCR_HIP_CHECK(ctx, hipMemcpyAsync(o.keys, r.keys, sizeof(uint64_t) * (size_t)r.n, hipMemcpyDeviceToDevice, ctx->stream));
    return PCR_OK;
}

extern "C" int pcr_voxel_map_create_on_grid(pcr_context *ctx, const float *xyz, const float *cov6, const float *normals, int64_t n, double voxel_size, double epsilon,
                                            const double *grid_min3, const double *T, pcr_voxel_map **out) {
    return pcr_api_call(ctx, [&]() -> int {
    const char *call = "voxel_map_create_on_grid";
    if (!out) { ctx->err = "voxel_map_create_on_grid: out is null"; return PCR_EINVAL; }
    *out = nullptr;
    if (!(voxel_size > 0.0) || !std::isfinite(voxel_size)) { ctx->err = std::string(call) + ": voxel_size <= 0"; return PCR_EINVAL; }
    PCR_TRY(vg_check_grid_min(ctx, call, grid_min3));
    PCR_TRY(vm_check_cloud(ctx, call, xyz, cov6, normals, n, epsilon, T));
    PCR_TRY(pcr_arena_reserve(ctx, vm_scratch(n, 0)));
    VmGrid g; memcpy(g.grid_min, grid_min3, sizeof g.grid_min); g.voxel = voxel_size;
    VmRows rows;
    PCR_TRY(vm_cloud_rows(ctx, call, xyz, cov6, normals, n, epsilon, T, g, &rows));
    MapBlock<VmapRow> nb;
    PCR_TRY(map_build_block<VmapRow>(ctx, call, rows.n, &nb, [&](const VmapRow::Out &o) -> int { return vm_copy_rows(ctx, rows, o); },
                                     [](const MapBlock<VmapRow> &) -> int { return PCR_OK; }));
    pcr_voxel_map *m = new pcr_voxel_map();
    m->device = ctx->device;
    map_adopt<VmapRow>(m, nb, rows.n);
    memcpy(m->grid_min, g.grid_min, sizeof m->grid_min);
    vm_origin(g, m->view.org);
    m->view.voxel = voxel_size;
    *out = m;
    return PCR_OK;
    });
}

extern "C" int pcr_voxel_map_insert(pcr_context *ctx, pcr_voxel_map *map, const float *xyz, const float *cov6, const float *normals, int64_t n, double epsilon,
                                    const double *T) {
    return pcr_api_call(ctx, [&]() -> int {
    const char *call = "voxel_map_insert";
    PCR_TRY(vg_check_map(ctx, map, call));
    PCR_TRY(vm_check_cloud(ctx, call, xyz, cov6, normals, n, epsilon, T));
    PCR_TRY(pcr_arena_reserve(ctx, vm_scratch(n, map->cells + n)));
    VmGrid g; memcpy(g.grid_min, map->grid_min, sizeof g.grid_min); g.voxel = map->view.voxel;
    VmRows rows;
    PCR_TRY(vm_cloud_rows(ctx, call, xyz, cov6, normals, n, epsilon, T, g, &rows));
    return map_merge_into<VmapRow>(ctx, call, map, rows);      // the rows lie in the arena reserved above
    });
}

extern "C" int pcr_voxel_map_merge(pcr_context *ctx, pcr_voxel_map *map, const pcr_voxel_map *other) {
    return pcr_api_call(ctx, [&]() -> int {
    const char *call = "voxel_map_merge";
    PCR_TRY(vg_check_map(ctx, map, call));
    if (!other || !other->block) { ctx->err = "voxel_map_merge: other is null"; return PCR_EINVAL; }
    if (other == map) { ctx->err = "voxel_map_merge: other is the map itself"; return PCR_EINVAL; }
    if (other->device != ctx->device) { ctx->err = "voxel_map_merge: other lives on another device than the context"; return PCR_EINVAL; }
    if (memcmp(&map->view.voxel, &other->view.voxel, sizeof(double)) != 0 || memcmp(map->view.org, other->view.org, sizeof map->view.org) != 0) {
        ctx->err = "voxel_map_merge: other is not on the map's grid (voxel size and origin must be equal bit for bit)"; return PCR_EINVAL;
    }
    PCR_TRY(pcr_arena_reserve(ctx, vm_scratch(0, map->cells + other->cells)));
    return map_merge_into<VmapRow>(ctx, call, map, VmapRow::rows_of(other));
    });
}

extern "C" int pcr_voxel_map_remove_far(pcr_context *ctx, pcr_voxel_map *map, const double *center3, double max_distance, int64_t *removed) {
    return pcr_api_call(ctx, [&]() -> int {
    const char *call = "voxel_map_remove_far";
    if (removed) *removed = 0;
    PCR_TRY(vg_check_map(ctx, map, call));
    return map_remove_far<VmapRow>(ctx, call, map, center3, max_distance, removed, vm_scratch(0, map->cells));
    });
}

extern "C" int pcr_voxel_map_grid(const pcr_voxel_map *map, double *grid_min3, double *origin3, double *voxel_size) {
    if (!map) return PCR_EINVAL;
    if (grid_min3) memcpy(grid_min3, map->grid_min, sizeof map->grid_min);
    if (origin3) memcpy(origin3, map->view.org, sizeof map->view.org);
    if (voxel_size) *voxel_size = map->view.voxel;
    return PCR_OK;
}
