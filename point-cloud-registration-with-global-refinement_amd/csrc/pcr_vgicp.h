// pcr_vgicp.h -- what the kernels of pcr_vgicp.hip share on the device (the map's count and row kernels, the voxelized GICP iteration kernel):
// the map as they see it, the pose applied to a source point with every operation rounded once, the cell of the result, the neighbourhood's
// offsets and the probe of the cell hash; and what the maps that grow take from here: the map's row policy (VmapRow; pcr_mapgrow.h), the key
// search, the far test, the placing of a point, the host checks.  The rule is the statement in include/pcr_hip.h.
#pragma once
#include "pcr_octree.h"

// One map row per occupied cell, in Morton order of the cell: mean4[v] = (mean, w = bit pattern of the count N_v), cov8[2 v], cov8[2 v + 1] =
// (xx, xy, xz, yy), (yz, zz, 0, 0); `tab` is the cell hash of level 0 (pcr_dev_build_grid_batch): cell -> (row, 1).
struct VgicpMapView {
    const GridEntry *tab; const unsigned *dmask;
    const float4 *mean4, *cov8;
    double org[3], voxel;                  // origin = min - voxel / 2 in float64: the grid of voxel_down_sample
};

// The map behind the C handle (pcr_vgicp.hip creates, reads and destroys it; pcr_vmap.hip grows and trims it by swapping in a new block).
struct pcr_voxel_map {
    int device = 0;
    int64_t cells = 0;
    char *block = nullptr;       // the one allocation: rows, keys, count word, cell hash
    size_t bytes = 0;
    VgicpMapView view;
    uint64_t *keys = nullptr;    // Morton keys of the rows (ascending)
    int *n_dev = nullptr;        // the row count on the device (what the hash build reads)
    double grid_min[3] = {0, 0, 0};     // g of the GRID rule: view.org = g - voxel / 2
};
// device bytes of a map of `cells` rows: rows, keys, the count word, the cell hash and its mask word (every array rounded up to 256 B)
static inline size_t vg_block_bytes(int64_t cells) {
    return (size_t)cells * (sizeof(float4) * 3 + sizeof(uint64_t)) + (size_t)pcr_grid_slots((unsigned)cells) * sizeof(GridEntry) + 16 * 256;
}

// The map's row policy for the frame of the maps that grow (pcr_mapgrow.h states what each member is); count and combine are pcr_vmap.hip's.
struct VmapRow {
    typedef pcr_voxel_map Map;
    struct Rows { const float4 *mean4, *cov8; const uint64_t *keys; int n; };
    struct Out { float4 *mean4, *cov8; uint64_t *keys; };
    struct Merged { int cap; Out out; };
    static constexpr int EXTRA = 0;
    __device__ static inline const double *extra(const Rows &) { return nullptr; }
    __device__ static inline double *extra(const Out &) { return nullptr; }
    static size_t block_bytes(int64_t cells) { return vg_block_bytes(cells); }
    static bool carve(pcr_context *ctx, int64_t cells, Out *o) {
        o->mean4 = arena<float4>(ctx, (size_t)cells); o->cov8 = arena<float4>(ctx, 2 * (size_t)cells); o->keys = arena<uint64_t>(ctx, (size_t)cells);
        return o->mean4 && o->cov8 && o->keys;
    }
    static Rows rows_of(const Map *m) { return Rows{m->view.mean4, m->view.cov8, m->keys, (int)m->cells}; }
    static void set_view(Map *m, const Out &o) { m->view.mean4 = o.mean4; m->view.cov8 = o.cov8; }
    static Merged merged(const Map *, int cap, const Out &o) { return Merged{cap, o}; }
    __device__ static inline int count(const float4 m) { return __float_as_int(m.w); }
    __device__ static inline void combine(const Merged &g, float4 &m, float4 &c0, float4 &c1, double *x, const float4 mb, const float4 d0, const float4 d1);
};

// host helpers of pcr_vgicp.hip that the units of the maps that grow call too: PCR_EINVAL naming the first of up to three arrays that holds a
// non-finite value (one read-back); the map / pose / grid_min3 argument checks; the member covariances of n points as packed cov6 (enqueues only);
// whether both ends of the members (bounds6: minimum, maximum) lie inside the 2^21 cells per axis of the grid of grid_min3; and what every unit
// that searches a map shares: the neighbourhood and source checks, and the tail of a correspondence set (flag scan, emit, count read-back)
int vg_check_finite(pcr_context *ctx, const char *call, const float *const *ptr, const size_t *count, const char *const *name, int arrays);
int vg_check_map(pcr_context *ctx, const pcr_voxel_map *map, const char *call);
template <class Map> static int vg_check_handle(pcr_context *ctx, const Map *map, const char *call) {      // (what vg_check_map asks, of any map's handle)
    if (!map || !map->block) { ctx->err = std::string(call) + ": map is null"; return PCR_EINVAL; }
    if (map->device != ctx->device) { ctx->err = std::string(call) + ": map lives on another device than the context"; return PCR_EINVAL; }
    return PCR_OK;
}
int vg_check_nbh(pcr_context *ctx, const char *call, int neighborhood);
int vg_check_src(pcr_context *ctx, const char *call, const float *src_xyz, int64_t n_src, int nbh);
int vg_emit_rows(pcr_context *ctx, const int32_t *slot, const uint8_t *flags, size_t total, int nbh, int32_t *rows2, int64_t *n_rows);
int vg_check_T(pcr_context *ctx, const char *call, const char *name, const double *T);
int vg_check_grid_min(pcr_context *ctx, const char *call, const double *grid_min3);
int vg_member_cov6(pcr_context *ctx, const float *cov6, const float *normals, double eps, int64_t n, float *out6);
bool vg_inside_grid(const double *bounds6, const double *grid_min3, double voxel);
static const double vg_eye[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};      // no pose is the identity, applied all the same

#define VG_NO_CELL (-4)                   // a coordinate with every candidate cell outside the grid (also: a non-finite coordinate)

// q = T p with q_r = ((T_r0 x + T_r1 y) + T_r2 z) + T_r3 in float64, every product and sum rounded once: numpy's elementwise expression gives
// the same bits, so the cell of q is decided (T: the first three rows of the pose, row-major)
__device__ static inline void vg_transform(const double *T, float x, float y, float z, double &qx, double &qy, double &qz) {
#pragma clang fp contract(off)
    const double px = x, py = y, pz = z;
    const double ax = T[0] * px, bx = T[1] * py, cx = T[2] * pz;
    const double ay = T[4] * px, by = T[5] * py, cy = T[6] * pz;
    const double az = T[8] * px, bz = T[9] * py, cz = T[10] * pz;
    double sx = ax + bx, sy = ay + by, sz = az + bz;
    sx = sx + cx; sy = sy + cy; sz = sz + cz;
    qx = sx + T[3]; qy = sy + T[7]; qz = sz + T[11];
}
// the point half of placing a member at a pose: p' = float32(q) with q the ROWS expression above; *bad is set when a placed coordinate is not finite
// (a pose whose products overflow)
__device__ static inline void vg_place_point(const double *T, const float *__restrict__ xyz, int i, float *__restrict__ out_xyz, int *__restrict__ bad) {
#pragma clang fp contract(off)
    double qx, qy, qz;
    vg_transform(T, xyz[(size_t)i * 3], xyz[(size_t)i * 3 + 1], xyz[(size_t)i * 3 + 2], qx, qy, qz);
    const float px = (float)qx, py = (float)qy, pz = (float)qz;
    out_xyz[(size_t)i * 3] = px; out_xyz[(size_t)i * 3 + 1] = py; out_xyz[(size_t)i * 3 + 2] = pz;
    if (!(isfinite(px) && isfinite(py) && isfinite(pz))) atomicOr(bad, 1);
}
// floor((q - origin) / voxel) of one axis as an int; everything from which no offset of -1, 0, +1 leads into [0, 2^21) becomes VG_NO_CELL
__device__ static inline int vg_cell(double q, double org, double voxel) {
#pragma clang fp contract(off)
    const double d = q - org;
    const double c = floor(d / voxel);
    return (c >= -1.0 && c <= 2097152.0) ? (int)c : VG_NO_CELL;
}
// offset k of the neighbourhood nbh: 1: the cell; 7: the cell, then +x, -x, +y, -y, +z, -z; 27: {-1, 0, 1}^3 in lexicographic order, dx slowest
__device__ static inline void vg_offset(int nbh, int k, int &dx, int &dy, int &dz) {
    if (nbh == 27) { dx = k / 9 - 1; dy = (k / 3) % 3 - 1; dz = k % 3 - 1; return; }
    const int axis = (k - 1) >> 1, s = k == 0 ? 0 : ((k & 1) ? 1 : -1);
    dx = axis == 0 ? s : 0; dy = axis == 1 ? s : 0; dz = axis == 2 ? s : 0;
}
// map row of the cell (x, y, z), or -1: outside [0, 2^21)^3 or unoccupied.  pcr_grid_lookup's probe loop: one 16-B load per probe
__device__ static inline int vg_row(const VgicpMapView &m, unsigned mask, int x, int y, int z) {
    GridView g;
    g.tab = m.tab; g.dmask = m.dmask; g.L = 0;
    const int2 r = pcr_grid_lookup(g, mask, x, y, z);
    return r.y > 0 ? r.x : -1;
}
// what the maps that grow share (pcr_vmap.hip, pcr_nmap.hip): first index of the ascending keys[0, n) that is not below key, the search of MERGE ...
__device__ static inline int vg_lower_bound(const uint64_t *__restrict__ keys, int n, uint64_t key) {
    int lo = 0, hi = n;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (keys[mid] < key) lo = mid + 1; else hi = mid; }
    return lo;
}
// ... and REMOVE_FAR's test d^2 < r^2 with d^2 in float64 from the float32 mean: differences, squares and sums in the order x, y, z, each rounded once
__device__ static inline bool vg_within(const float4 p, double cx, double cy, double cz, double r2) {
#pragma clang fp contract(off)
    const double dx = (double)p.x - cx, dy = (double)p.y - cy, dz = (double)p.z - cz;
    const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
    double d2 = xx + yy;
    d2 = d2 + zz;
    return d2 < r2;
}
// c = a b and c = a b^T of row-major 3x3 matrices, every entry (a_i0 b_0j + a_i1 b_1j) + a_i2 b_2j with its zero terms and without contraction: the
// oracle's m3_mul / m3_mul_bt
__device__ static inline void vg_mul3(const double *a, const double *b, double *c) {
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) { double s = a[i * 3] * b[j]; s = s + a[i * 3 + 1] * b[3 + j]; s = s + a[i * 3 + 2] * b[6 + j]; c[i * 3 + j] = s; }
}
__device__ static inline void vg_mul3_bt(const double *a, const double *b, double *c) {
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) { double s = a[i * 3] * b[j * 3]; s = s + a[i * 3 + 1] * b[j * 3 + 1]; s = s + a[i * 3 + 2] * b[j * 3 + 2]; c[i * 3 + j] = s; }
}
