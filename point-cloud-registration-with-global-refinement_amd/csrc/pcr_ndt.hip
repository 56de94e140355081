// pcr_ndt.hip -- NDT registration (Biber & Strasser 2003, Magnusson 2009) on a normal-distributions voxel map: the map, the iteration kernel and
// its loop, the one-launch linearisation and the entry points; the specification is the statement in include/pcr_hip.h.  The grid, the cell
// hash and the pose expression are voxelized GICP's (pcr_vgicp.h); what an ICP loop is made of is pcr_icp_loop.h.
//   map build      the means through the voxel pass (pcr_dev_voxel: float64 sums in input order); the cells' Morton keys go into the cell hash
//                  of level 0 inside the map's own allocation (map_build_block, pcr_mapgrow.h: the builder of every map block, here with what
//                  follows in its after-hook); k_ndt_member forms the six products of every member against its cell's float32
//                  mean, found through that hash, as two 3-vectors that ride in the attribute slot of two more voxel passes (the same keys, the
//                  same stable sort: row v of all three passes is the same cell) and counts the members; k_ndt_cell lays the rows out and
//                  computes A_v with a float64 Jacobi eigen-solve (ndt_cell_information, pcr_ndt.h).  One builder, ndt_map_build, on the
//                  cloud's own grid or on a given one, with the members as they lie or placed at a pose (k_ndt_place): pcr_ndt_map_create and
//                  the calls of pcr_nmap.hip (the map that grows) all make their rows through it
//   k_icp_iter_ndt the whole iteration, a sibling of k_icp_iter_vgicp: one lane per source point, 1 / 7 / 27 hash probes, per hit one gather of
//                  (mean, +-N_v) and one of A_v (80 B with the probe), the row added straight into the 30 sums that icp_finish reduces
//   k_ndt_lin      the same row plus the score for one pose, with a reduction of its own in a fixed order
// Floating-point contraction per source expression only; the expressions that decide a cell (pcr_vgicp.h) are not contracted at all.
#pragma clang fp contract(on)
#include <cmath>
#include <cstring>
#include "pcr_icp_loop.h"
#include "pcr_ndt.h"
#include "pcr_mapgrow.h"

#define NDT_BS 256
#define NDT_NL 32                      // sums of the linearisation: the loop's 30, the score, one unused

// ================================================================ the row
// Row (i, v) of UPDATE: delta = q - mu, m = delta^T A delta, e = exp(-d2 m / 2), w = -d1 d2 e, J = [S | I] with S = -skew(q).  With B = A J = [A S | A]
// (row r of A S is q x A_r, A being symmetric) the matrix w J^T B has the rows q x B_c above (S^T x = q x x) and B itself below, and the right-hand
// side is w [q x (A delta); A delta].  Slots as icp_row6 fills them: 0..20 the upper triangle row by row, 21..26 the right-hand side.
struct NdtScore { double wk, hd2, d1; };              // wk = -d1 d2, hd2 = d2 / 2
template <bool SCORE>
__device__ static inline void ndt_row(const NdtScore &sc, double qx, double qy, double qz, const float4 mu, const double *__restrict__ A6, double *acc) {
    const double dx = qx - (double)mu.x, dy = qy - (double)mu.y, dz = qz - (double)mu.z;
    acc[28] += dx * dx + dy * dy + dz * dz; acc[29] += 1.0;
    const double axx = A6[0], axy = A6[1], axz = A6[2], ayy = A6[3], ayz = A6[4], azz = A6[5];
    const double ux = axx * dx + axy * dy + axz * dz, uy = axy * dx + ayy * dy + ayz * dz, uz = axz * dx + ayz * dy + azz * dz;      // A delta
    const double m = dx * ux + dy * uy + dz * uz;
    const double e = exp(-(sc.hd2 * m));
    const double w = sc.wk * e;
    if (SCORE) acc[30] += -(sc.d1 * e);
    // B = [A S | A], 3 x 6
    double B[3][6];
    B[0][0] = qy * axz - qz * axy; B[0][1] = qz * axx - qx * axz; B[0][2] = qx * axy - qy * axx; B[0][3] = axx; B[0][4] = axy; B[0][5] = axz;
    B[1][0] = qy * ayz - qz * ayy; B[1][1] = qz * axy - qx * ayz; B[1][2] = qx * ayy - qy * axy; B[1][3] = axy; B[1][4] = ayy; B[1][5] = ayz;
    B[2][0] = qy * azz - qz * ayz; B[2][1] = qz * axz - qx * azz; B[2][2] = qx * ayz - qy * axz; B[2][3] = axz; B[2][4] = ayz; B[2][5] = azz;
    // rows 0..2 of J^T B: q x (column c of B); only c >= p is kept
#pragma unroll
    for (int c = 0; c < 6; c++) {
        const double h0 = qy * B[2][c] - qz * B[1][c], h1 = qz * B[0][c] - qx * B[2][c], h2 = qx * B[1][c] - qy * B[0][c];
        acc[c] += w * h0;                              // (0, c): slot c
        if (c >= 1) acc[6 + (c - 1)] += w * h1;        // (1, c): slot 6 + c - 1
        if (c >= 2) acc[11 + (c - 2)] += w * h2;       // (2, c): slot 11 + c - 2
    }
    acc[15] += w * axx; acc[16] += w * axy; acc[17] += w * axz; acc[18] += w * ayy; acc[19] += w * ayz; acc[20] += w * azz;
    acc[21] += w * (qy * uz - qz * uy); acc[22] += w * (qz * ux - qx * uz); acc[23] += w * (qx * uy - qy * ux);
    acc[24] += w * ux; acc[25] += w * uy; acc[26] += w * uz;
}
// every row of source point (x, y, z) at the pose T (its first three rows) into acc
template <bool SCORE>
__device__ static inline void ndt_point(const NdtMapView &m, int nbh, const NdtScore &sc, const double *T, float x, float y, float z, double *acc) {
    double qx, qy, qz;
    vg_transform(T, x, y, z, qx, qy, qz);
    const int cx = vg_cell(qx, m.org[0], m.voxel), cy = vg_cell(qy, m.org[1], m.voxel), cz = vg_cell(qz, m.org[2], m.voxel);
    const VgicpMapView h = ndt_hash(m);
    const unsigned mask = *m.dmask;
    bool any = false;
    for (int k = 0; k < nbh; k++) {
        int dx, dy, dz;
        vg_offset(nbh, k, dx, dy, dz);
        const int row = vg_row(h, mask, cx + dx, cy + dy, cz + dz);
        if (row < 0) continue;
        const float4 mu = m.mean4[row];
        if (__float_as_int(mu.w) <= 0) continue;      // an invalid cell
        const double2 *ap = reinterpret_cast<const double2 *>(m.info6 + 6 * (size_t)row);
        const double2 a0 = ap[0], a1 = ap[1], a2 = ap[2];
        const double A6[6] = {a0.x, a0.y, a1.x, a1.y, a2.x, a2.y};
        ndt_row<SCORE>(sc, qx, qy, qz, mu, A6, acc);
        any = true;
    }
    if (any) acc[27] += 1.0;
}

// ================================================================ the iteration
struct IcpNdtArgs {
    const float *src_xyz;              // packed, caller order
    NdtMapView map;
    NdtScore sc;
    int ns, nbh;
};
__global__ void __launch_bounds__(LIN_BS) k_icp_iter_ndt(IcpArgs a, IcpNdtArgs v) {
    icp_iter_frame<ICP_MODE_NDT, LIN_BS>(a, v.ns, [&](int i, bool live, const double *T, double *acc) {
        if (live) ndt_point<false>(v.map, v.nbh, v.sc, T, v.src_xyz[(size_t)i * 3], v.src_xyz[(size_t)i * 3 + 1], v.src_xyz[(size_t)i * 3 + 2], acc);
    });
}

// The map loop (icp_map_loop, pcr_icp_loop.h) with this unit's kernel and argument block.
static int ndt_loop(pcr_context *ctx, const float *src_xyz, int64_t n_src, const NdtMapView *map, const NdtScore &sc, const double *T0, const pcr_ndt_params *p, pcr_result *out) {
    IcpArgs a; memset(&a, 0, sizeof a);           // (the bytes of both argument blocks are the graph key)
    a.loss = PCR_LOSS_L2; a.loss_k = 1.0; a.a = 1.0;
    a.rel_fit = p->relative_fitness; a.rel_rmse = p->relative_rmse; a.max_it = p->max_iteration;
    IcpNdtArgs v; memset(&v, 0, sizeof v);
    v.src_xyz = src_xyz; v.map = *map; v.sc = sc; v.ns = (int)n_src; v.nbh = p->neighborhood;
    auto launch = [&](int nb) { PCR_LAUNCH(ctx, k_icp_iter_ndt, dim3(nb), dim3(LIN_BS), 0, ctx->stream, a, v); };
    return icp_map_loop(ctx, "registration_ndt", a, &v, sizeof v, v.ns, ICP_MODE_NDT, launch, T0, false, out, nullptr);
}

// ================================================================ the linearisation at one pose
// One launch.  Workgroup b owns points [LIN_BS b, LIN_BS b + LIN_BS); its NDT_NL sums are reduced by a shuffle butterfly inside every wavefront and
// then wavefront by wavefront in order; the last workgroup to arrive (ticket) adds the workgroups' rows in order of b.  Every sum is therefore
// taken in an order that depends on nothing but n_src: the same bits on every run.  partials and out are written and read at agent scope.
struct NdtPose { double T[12]; };
__device__ static inline double ndt_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__global__ void __launch_bounds__(LIN_BS) k_ndt_lin(const float *__restrict__ src_xyz, int ns, NdtPose pose, NdtMapView m, int nbh, NdtScore sc,
                                                    double *__restrict__ partials, unsigned *__restrict__ ticket, double *__restrict__ out) {
    __shared__ double red[LIN_BS / 64][NDT_NL];
    __shared__ int is_last;
    const int nb = (int)gridDim.x;
    double acc[NDT_NL];
#pragma unroll
    for (int k = 0; k < NDT_NL; k++) acc[k] = 0.0;
    const int i = blockIdx.x * LIN_BS + threadIdx.x;
    if (i < ns) ndt_point<true>(m, nbh, sc, pose.T, src_xyz[(size_t)i * 3], src_xyz[(size_t)i * 3 + 1], src_xyz[(size_t)i * 3 + 2], acc);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < NDT_NL - 1; k++) { const double s = ndt_wave_sum(acc[k]); if (lane == 0) red[wave][k] = s; }
    if (lane == 0) red[wave][NDT_NL - 1] = 0.0;
    __syncthreads();
    if (threadIdx.x < NDT_NL) {
        double s = red[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < LIN_BS / 64; w++) s += red[w][threadIdx.x];
        __hip_atomic_store(&partials[(size_t)blockIdx.x * NDT_NL + threadIdx.x], s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) is_last = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)(nb - 1);
    __syncthreads();
    if (!is_last) return;
    __threadfence();
    if (threadIdx.x < NDT_NL) {
        double s = 0.0;
        for (int b = 0; b < nb; b++) s += __hip_atomic_load(&partials[(size_t)b * NDT_NL + threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        out[threadIdx.x] = s;
    }
}

// ================================================================ the map
__device__ static inline int ndt_compact21(uint64_t x) {      // inverse of pcr_spread21
    x &= 0x1249249249249249ull;
    x = (x | (x >> 2)) & 0x10c30c30c30c30c3ull;
    x = (x | (x >> 4)) & 0x100f00f00f00f00full;
    x = (x | (x >> 8)) & 0x1f0000ff0000ffull;
    x = (x | (x >> 16)) & 0x1f00000000ffffull;
    x = (x | (x >> 32)) & 0x1fffffull;
    return (int)x;
}
// ---- the member statistic: every target point finds its cell's row through the hash (the float64 cell expression of k_voxel_keys), counts itself and
// forms the six products of d = p - mu_v, each rounded once to float64 and then to float32 (lo = xx,xy,xz; hi = yy,yz,zz)
__global__ void __launch_bounds__(NDT_BS) k_ndt_member(const float *__restrict__ xyz, int n, NdtMapView m, const float4 *__restrict__ mean, int cells,
                                                       int *__restrict__ count, float *__restrict__ lo3, float *__restrict__ hi3) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * NDT_BS + threadIdx.x;
    if (i >= n) return;
    const float x = xyz[(size_t)i * 3], y = xyz[(size_t)i * 3 + 1], z = xyz[(size_t)i * 3 + 2];
    const int cx = vg_cell((double)x, m.org[0], m.voxel), cy = vg_cell((double)y, m.org[1], m.voxel), cz = vg_cell((double)z, m.org[2], m.voxel);
    const int row = vg_row(ndt_hash(m), *m.dmask, cx, cy, cz);
    float l0 = 0, l1 = 0, l2 = 0, h0 = 0, h1 = 0, h2 = 0;
    if (row >= 0 && row < cells) {
        atomicAdd(&count[row], 1);
        const float4 mu = mean[row];
        const double dx = (double)x - (double)mu.x, dy = (double)y - (double)mu.y, dz = (double)z - (double)mu.z;
        const double xx = dx * dx, xy = dx * dy, xz = dx * dz, yy = dy * dy, yz = dy * dz, zz = dz * dz;
        l0 = (float)xx; l1 = (float)xy; l2 = (float)xz; h0 = (float)yy; h1 = (float)yz; h2 = (float)zz;
    }
    lo3[(size_t)i * 3] = l0; lo3[(size_t)i * 3 + 1] = l1; lo3[(size_t)i * 3 + 2] = l2;
    hi3[(size_t)i * 3] = h0; hi3[(size_t)i * 3 + 1] = h1; hi3[(size_t)i * 3 + 2] = h2;
}
// ---- one lane per cell: the row, with validity and A_v by ndt_cell_information (pcr_ndt.h)
__global__ void __launch_bounds__(NDT_BS) k_ndt_cell(const float4 *__restrict__ mean, const float4 *__restrict__ lo, const float4 *__restrict__ hi,
                                                     const int *__restrict__ count, int cells, int min_points, double ratio,
                                                     float4 *__restrict__ mean4, float4 *__restrict__ cov8, double *__restrict__ info6) {
#pragma clang fp contract(off)
    const int v = blockIdx.x * NDT_BS + threadIdx.x;
    if (v >= cells) return;
    const float4 p = mean[v], l = lo[v], h = hi[v];
    const int nv = count[v];
    const float4 c0 = make_float4(l.x, l.y, l.z, h.x), c1 = make_float4(h.y, h.z, 0.0f, 0.0f);
    cov8[2 * (size_t)v] = c0;
    cov8[2 * (size_t)v + 1] = c1;
    double A6[6];
    const bool valid = ndt_cell_information(nv, c0, c1, min_points, ratio, A6);
    mean4[v] = make_float4(p.x, p.y, p.z, __int_as_float(valid ? nv : -nv));
#pragma unroll
    for (int t = 0; t < 6; t++) info6[6 * (size_t)v + t] = A6[t];
}
// ---- the members at a pose: vg_place_point (pcr_vgicp.h), which k_vmap_place calls too
struct NdtPlace { double T[12]; };
__global__ void __launch_bounds__(NDT_BS) k_ndt_place(const float *__restrict__ xyz, int n, NdtPlace pose, float *__restrict__ out_xyz, int *__restrict__ bad) {
    const int i = blockIdx.x * NDT_BS + threadIdx.x;
    if (i < n) vg_place_point(pose.T, xyz, i, out_xyz, bad);
}
__global__ void __launch_bounds__(NDT_BS) k_ndt_read(const uint64_t *__restrict__ keys, NdtMapView m, int cells, int32_t *__restrict__ cell3, int32_t *__restrict__ count,
                                                     float *__restrict__ mean3, float *__restrict__ cov6, double *__restrict__ info6, uint8_t *__restrict__ valid) {
    const int v = blockIdx.x * NDT_BS + threadIdx.x;
    if (v >= cells) return;
    const float4 p = m.mean4[v];
    const int w = __float_as_int(p.w);
    if (cell3) { const uint64_t k = keys[v]; cell3[(size_t)v * 3] = ndt_compact21(k); cell3[(size_t)v * 3 + 1] = ndt_compact21(k >> 1); cell3[(size_t)v * 3 + 2] = ndt_compact21(k >> 2); }
    if (count) count[v] = w < 0 ? -w : w;
    if (valid) valid[v] = w > 0 ? 1 : 0;
    if (mean3) { mean3[(size_t)v * 3] = p.x; mean3[(size_t)v * 3 + 1] = p.y; mean3[(size_t)v * 3 + 2] = p.z; }
    if (cov6) {
        const float4 a = m.cov8[2 * (size_t)v], b = m.cov8[2 * (size_t)v + 1];
        float *o = cov6 + (size_t)v * 6;
        o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w; o[4] = b.x; o[5] = b.y;
    }
    if (info6) for (int t = 0; t < 6; t++) info6[(size_t)v * 6 + t] = m.info6[(size_t)v * 6 + t];
}

// ---- rows at a pose: slot[i * nbh + k] = map row of candidate k of source point i, or -1; flags for the scan (the tail: vg_emit_rows, pcr_vgicp.hip)
__global__ void __launch_bounds__(NDT_BS) k_ndt_rows(const float *__restrict__ src_xyz, int ns, NdtPose pose, NdtMapView m, int nbh, int32_t *__restrict__ slot,
                                                     uint8_t *__restrict__ flags) {
    const int i = blockIdx.x * NDT_BS + threadIdx.x;
    if (i >= ns) return;
    double qx, qy, qz;
    vg_transform(pose.T, src_xyz[(size_t)i * 3], src_xyz[(size_t)i * 3 + 1], src_xyz[(size_t)i * 3 + 2], qx, qy, qz);
    const int cx = vg_cell(qx, m.org[0], m.voxel), cy = vg_cell(qy, m.org[1], m.voxel), cz = vg_cell(qz, m.org[2], m.voxel);
    const VgicpMapView h = ndt_hash(m);
    const unsigned mask = *m.dmask;
    for (int k = 0; k < nbh; k++) {
        int dx, dy, dz;
        vg_offset(nbh, k, dx, dy, dz);
        int row = vg_row(h, mask, cx + dx, cy + dy, cz + dz);
        if (row >= 0 && __float_as_int(m.mean4[row].w) <= 0) row = -1;
        slot[(size_t)i * nbh + k] = row;
        flags[(size_t)i * nbh + k] = row >= 0 ? 1 : 0;
    }
}

static unsigned ndt_blocks(size_t n) { return (unsigned)((n + NDT_BS - 1) / NDT_BS); }

int ndt_check_map(pcr_context *ctx, const pcr_ndt_map *map, const char *call) { return vg_check_handle(ctx, map, call); }      // (pcr_nmap.hip calls it too)
// SCORE CONSTANTS of the rule, in float64 on the host
static int ndt_score(pcr_context *ctx, const char *call, double outlier_ratio, double voxel, NdtScore *sc) {
    if (!(outlier_ratio > 0.0) || !(outlier_ratio < 1.0)) { ctx->err = std::string(call) + ": outlier_ratio must lie in (0, 1)"; return PCR_EINVAL; }
    const double c1 = 10.0 * (1.0 - outlier_ratio), c2 = outlier_ratio / (voxel * voxel * voxel);
    const double d3 = -log(c2), d1 = -log(c1 + c2) - d3;
    const double d2 = -2.0 * log((-log(c1 * exp(-0.5) + c2) - d3) / d1);
    if (!std::isfinite(d1) || !std::isfinite(d2)) { ctx->err = std::string(call) + ": outlier_ratio and voxel_size give no finite score constants"; return PCR_ENUMERIC; }
    sc->wk = -d1 * d2; sc->hd2 = d2 / 2.0; sc->d1 = d1;
    return PCR_OK;
}

int ndt_map_build(pcr_context *ctx, const char *call, const float *xyz, int64_t n, double voxel_size, int min_points_per_voxel, double eigenvalue_ratio,
                  const double *grid_min3, const double *T, pcr_ndt_map **out) {
    const std::string who(call);
    if (!out) { ctx->err = who + ": out is null"; return PCR_EINVAL; }
    *out = nullptr;
    if (!(voxel_size > 0.0) || !std::isfinite(voxel_size)) { ctx->err = who + ": voxel_size <= 0"; return PCR_EINVAL; }
    if (min_points_per_voxel < 2) { ctx->err = who + ": min_points_per_voxel < 2"; return PCR_EINVAL; }
    if (!(eigenvalue_ratio > 0.0) || !(eigenvalue_ratio <= 1.0)) { ctx->err = who + ": eigenvalue_ratio must lie in (0, 1]"; return PCR_EINVAL; }
    if (n < 1 || n > 0x7fffffff / 8 || !xyz) { ctx->err = who + ": xyz must hold 1 .. 2^28 - 1 points"; return PCR_EINVAL; }
    PCR_TRY(pcr_arena_reserve(ctx, 3 * pcr_scratch_bytes_for(n) + (size_t)n * 112 + 4096));
    {
        const float *ptr[1] = {xyz}; const size_t cnt[1] = {(size_t)n * 3}; const char *name[1] = {"xyz"};
        PCR_TRY(vg_check_finite(ctx, call, ptr, cnt, name, 1));
    }
    int *bad = nullptr;
    if (T) {      // the members at the pose
        float *placed = arena<float>(ctx, (size_t)n * 3);
        bad = arena<int>(ctx, 1);
        if (!placed || !bad) return PCR_ENOMEM;
        NdtPlace pose; memcpy(pose.T, T, sizeof pose.T);
        PCR_HIP_CHECK(ctx, hipMemsetAsync(bad, 0, sizeof(int), ctx->stream));
        PCR_LAUNCH(ctx, k_ndt_place, dim3(ndt_blocks((size_t)n)), dim3(NDT_BS), 0, ctx->stream, xyz, (int)n, pose, placed, bad);
        xyz = placed;
    }
    double b6[6];
    PCR_TRY(pcr_dev_bounds(ctx, xyz, n, b6));
    if (grid_min3) {
        // both ends of the members against the grid before any key is formed; the voxel pass then runs with grid_min3 in place of the members' minimum
        int64_t nonfinite = 0;
        if (bad) PCR_TRY(pcr_read_count(ctx, bad, &nonfinite));
        if (nonfinite != 0 || !vg_inside_grid(b6, grid_min3, voxel_size)) { ctx->err = who + ": xyz lies outside the map's grid (cell indices must stay in [0, 2^21) on every axis)"; return PCR_EINVAL; }
        for (int d = 0; d < 3; d++) b6[d] = grid_min3[d];
    }
    float *lo3 = arena<float>(ctx, (size_t)n * 3), *hi3 = arena<float>(ctx, (size_t)n * 3);
    if (!lo3 || !hi3) return PCR_ENOMEM;
    // the voxel pass three times over the same points: the same keys, the same stable sort, so row v of every pass is the same cell
    DevCloud vm, va, vb;
    PCR_TRY(pcr_alloc_cloud(ctx, &vm, (int)n, false, false));
    PCR_TRY(pcr_alloc_cloud(ctx, &va, (int)n, true, false));
    PCR_TRY(pcr_alloc_cloud(ctx, &vb, (int)n, true, false));
    PCR_TRY(pcr_dev_voxel(ctx, xyz, nullptr, n, b6, voxel_size, &vm));
    int64_t cells = 0;
    PCR_TRY(pcr_read_count(ctx, vm.n, &cells));
    if (cells < 1 || cells > n) { ctx->err = who + ": the voxel pass returned no cells"; return PCR_EHIP; }

    pcr_ndt_map *m = new pcr_ndt_map();
    m->device = ctx->device;
    for (int d = 0; d < 3; d++) m->grid_min[d] = b6[d];
    m->min_points = min_points_per_voxel; m->ratio = eigenvalue_ratio;
    for (int d = 0; d < 3; d++) m->view.org[d] = b6[d] - voxel_size * 0.5;      // (pcr_dev_voxel's origin)
    m->view.voxel = voxel_size;
    // the map's arrays and the hash table come out of the map's block; the member statistic, through that hash, is scratch of the context's arena
    MapBlock<NmapRow> nb;
    const int rc = map_build_block<NmapRow>(ctx, call, cells, &nb, [&](const NmapRow::Out &o) -> int {
        PCR_HIP_CHECK(ctx, hipMemcpyAsync(o.keys, vm.keys, sizeof(uint64_t) * (size_t)cells, hipMemcpyDeviceToDevice, ctx->stream));
        return PCR_OK;
    }, [&](const MapBlock<NmapRow> &b) -> int {
        map_adopt<NmapRow>(m, b, cells);      // (the builder frees the block if anything after this fails)
        int *count = arena<int>(ctx, (size_t)cells);
        if (!count) return PCR_ENOMEM;
        PCR_HIP_CHECK(ctx, hipMemsetAsync(count, 0, sizeof(int) * (size_t)cells, ctx->stream));
        PCR_LAUNCH(ctx, k_ndt_member, dim3(ndt_blocks((size_t)n)), dim3(NDT_BS), 0, ctx->stream, xyz, (int)n, m->view, (const float4 *)vm.pts, (int)cells, count, lo3, hi3);
        PCR_TRY(pcr_dev_voxel(ctx, xyz, lo3, n, b6, voxel_size, &va));
        PCR_TRY(pcr_dev_voxel(ctx, xyz, hi3, n, b6, voxel_size, &vb));
        PCR_LAUNCH(ctx, k_ndt_cell, dim3(ndt_blocks((size_t)cells)), dim3(NDT_BS), 0, ctx->stream, (const float4 *)vm.pts, (const float4 *)va.nrm, (const float4 *)vb.nrm,
                   (const int *)count, (int)cells, min_points_per_voxel, eigenvalue_ratio, b.out.mean4, b.out.cov8, b.out.info6);
        return PCR_OK;
    });
    if (rc != PCR_OK) { delete m; return rc; }
    *out = m;
    return PCR_OK;
}

extern "C" int pcr_ndt_map_create(pcr_context *ctx, const float *xyz, int64_t n, double voxel_size, int min_points_per_voxel, double eigenvalue_ratio, pcr_ndt_map **out) {
    return pcr_api_call(ctx, [&]() -> int {
    return ndt_map_build(ctx, "ndt_map_create", xyz, n, voxel_size, min_points_per_voxel, eigenvalue_ratio, nullptr, nullptr, out);
    });
}

extern "C" int pcr_ndt_map_destroy(pcr_ndt_map *map) {
    if (!map) return PCR_OK;
    if (map->block) {
        if (hipSetDevice(map->device) != hipSuccess) return PCR_EHIP;
        (void)hipFree(map->block);                            // waits for the device: no call is still reading the block
    }
    delete map;
    return PCR_OK;
}

extern "C" int pcr_ndt_map_size(const pcr_ndt_map *map, int64_t *cells) {
    if (!map || !cells) return PCR_EINVAL;
    *cells = map->cells;
    return PCR_OK;
}

extern "C" int pcr_ndt_map_grid(const pcr_ndt_map *map, double *origin3, double *voxel_size) {
    if (!map) return PCR_EINVAL;
    if (origin3) for (int d = 0; d < 3; d++) origin3[d] = map->view.org[d];
    if (voxel_size) *voxel_size = map->view.voxel;
    return PCR_OK;
}

extern "C" int pcr_ndt_map_read(pcr_context *ctx, const pcr_ndt_map *map, int32_t *cell3, int32_t *count, float *mean3, float *cov6, double *info6, uint8_t *valid) {
    return pcr_api_call(ctx, [&]() -> int {
    PCR_TRY(ndt_check_map(ctx, map, "ndt_map_read"));
    PCR_LAUNCH(ctx, k_ndt_read, dim3(ndt_blocks((size_t)map->cells)), dim3(NDT_BS), 0, ctx->stream, (const uint64_t *)map->keys, map->view, (int)map->cells, cell3, count, mean3, cov6,
               info6, valid);
    return PCR_OK;
    });
}

// rows of the rule at the pose T (16 doubles, host) into rows2; scratch from the arena the caller has reserved
static int ndt_rows(pcr_context *ctx, const pcr_ndt_map *map, const float *src_xyz, int64_t n_src, const double *T, int nbh, int32_t *rows2, int64_t *n_rows) {
    *n_rows = 0;
    if (n_src == 0) return PCR_OK;
    ArenaMark mark(ctx);
    const size_t total = (size_t)n_src * nbh;
    int32_t *slot = arena<int32_t>(ctx, total);
    uint8_t *flags = arena<uint8_t>(ctx, total);
    if (!slot || !flags) return PCR_ENOMEM;
    NdtPose pose; memcpy(pose.T, T, sizeof pose.T);
    PCR_LAUNCH(ctx, k_ndt_rows, dim3(ndt_blocks((size_t)n_src)), dim3(NDT_BS), 0, ctx->stream, src_xyz, (int)n_src, pose, map->view, nbh, slot, flags);
    return vg_emit_rows(ctx, slot, flags, total, nbh, rows2, n_rows);
}
static size_t ndt_rows_scratch(int64_t n_src, int nbh) { return (size_t)(n_src > 0 ? n_src : 1) * nbh * 10 + (1u << 20); }

extern "C" int pcr_ndt_map_correspondences(pcr_context *ctx, const pcr_ndt_map *map, const float *src_xyz, int64_t n_src, const double *T, int neighborhood, int32_t *rows2,
                                           int64_t *n_rows) {
    return pcr_api_call(ctx, [&]() -> int {
    const char *call = "ndt_map_correspondences";
    PCR_TRY(ndt_check_map(ctx, map, call));
    PCR_TRY(vg_check_nbh(ctx, call, neighborhood));
    PCR_TRY(vg_check_src(ctx, call, src_xyz, n_src, neighborhood));
    if (!n_rows || (n_src > 0 && !rows2)) { ctx->err = "ndt_map_correspondences: rows2 / n_rows is null"; return PCR_EINVAL; }
    PCR_TRY(vg_check_T(ctx, call, "T", T));
    PCR_TRY(pcr_arena_reserve(ctx, ndt_rows_scratch(n_src, neighborhood)));
    const float *ptr[1] = {src_xyz}; const size_t cnt[1] = {(size_t)n_src * 3}; const char *name[1] = {"src_xyz"};
    PCR_TRY(vg_check_finite(ctx, call, ptr, cnt, name, 1));
    return ndt_rows(ctx, map, src_xyz, n_src, T, neighborhood, rows2, n_rows);
    });
}

extern "C" int pcr_ndt_linearize(pcr_context *ctx, const pcr_ndt_map *map, const float *src_xyz, int64_t n_src, const double *T, int neighborhood, double outlier_ratio,
                                 double *JTJ, double *JTr, double *score, int64_t *rows, int64_t *points_with_rows, double *sum_d2) {
    return pcr_api_call(ctx, [&]() -> int {
    const char *call = "ndt_linearize";
    PCR_TRY(ndt_check_map(ctx, map, call));
    PCR_TRY(vg_check_nbh(ctx, call, neighborhood));
    PCR_TRY(vg_check_src(ctx, call, src_xyz, n_src, neighborhood));
    PCR_TRY(vg_check_T(ctx, call, "T", T));
    NdtScore sc;
    PCR_TRY(ndt_score(ctx, call, outlier_ratio, map->view.voxel, &sc));
    const int ns = (int)n_src;
    const int nb = ns > 0 ? (ns + LIN_BS - 1) / LIN_BS : 1;
    PCR_TRY(pcr_arena_reserve(ctx, (size_t)nb * NDT_NL * sizeof(double) + (1u << 20)));
    const float *ptr[1] = {src_xyz}; const size_t cnt[1] = {(size_t)n_src * 3}; const char *name[1] = {"src_xyz"};
    PCR_TRY(vg_check_finite(ctx, call, ptr, cnt, name, 1));
    ArenaMark mark(ctx);
    double *partials = arena<double>(ctx, (size_t)nb * NDT_NL), *sums = arena<double>(ctx, NDT_NL);
    unsigned *ticket = arena<unsigned>(ctx, 1);
    if (!partials || !sums || !ticket) return PCR_ENOMEM;
    PCR_HIP_CHECK(ctx, hipMemsetAsync(ticket, 0, sizeof(unsigned), ctx->stream));
    NdtPose pose; memcpy(pose.T, T, sizeof pose.T);
    PCR_LAUNCH(ctx, k_ndt_lin, dim3(nb), dim3(LIN_BS), 0, ctx->stream, src_xyz, ns, pose, map->view, neighborhood, sc, partials, ticket, sums);
    double h[NDT_NL];
    PCR_HIP_CHECK(ctx, hipMemcpyAsync(h, sums, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
    PCR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    if (JTJ) {
        int t = 0;
        for (int p = 0; p < 6; p++) for (int q = p; q < 6; q++) { JTJ[p * 6 + q] = h[t]; JTJ[q * 6 + p] = h[t]; t++; }
    }
    if (JTr) for (int p = 0; p < 6; p++) JTr[p] = h[21 + p];
    if (points_with_rows) *points_with_rows = (int64_t)(h[27] + 0.5);
    if (sum_d2) *sum_d2 = h[28];
    if (rows) *rows = (int64_t)(h[29] + 0.5);
    if (score) *score = h[30];
    return PCR_OK;
    });
}

extern "C" int pcr_registration_ndt(pcr_context *ctx, const float *src_xyz, int64_t n_src, const pcr_ndt_map *map, const double *init_T, const pcr_ndt_params *params,
                                    pcr_result *result, int32_t *correspondences) {
    return pcr_api_call(ctx, [&]() -> int {
    const char *call = "registration_ndt";
    if (!params || !result) { ctx->err = "registration_ndt: params / result is null"; return PCR_EINVAL; }
    PCR_TRY(ndt_check_map(ctx, map, call));
    PCR_TRY(vg_check_nbh(ctx, call, params->neighborhood));
    PCR_TRY(vg_check_src(ctx, call, src_xyz, n_src, params->neighborhood));
    if (params->max_iteration < 0) { ctx->err = "registration_ndt: params.max_iteration < 0"; return PCR_EINVAL; }
    NdtScore sc;
    PCR_TRY(ndt_score(ctx, call, params->outlier_ratio, map->view.voxel, &sc));
    PCR_TRY(vg_check_T(ctx, call, "init_T", init_T));
    PCR_TRY(pcr_arena_reserve(ctx, ndt_rows_scratch(n_src, params->neighborhood) + (size_t)(n_src > 0 ? n_src : 1) * 8 + (4u << 20)));
    {
        const float *ptr[1] = {src_xyz}; const size_t cnt[1] = {(size_t)n_src * 3}; const char *name[1] = {"src_xyz"};
        PCR_TRY(vg_check_finite(ctx, call, ptr, cnt, name, 1));
    }
    PCR_TRY(ndt_loop(ctx, src_xyz, n_src, &map->view, sc, init_T, params, result));
    if (correspondences) {      // the rows of the last launch: those at the returned pose
        int64_t rows = 0;
        PCR_TRY(ndt_rows(ctx, map, src_xyz, n_src, result->transformation, params->neighborhood, correspondences, &rows));
        if (rows != result->n_correspondences) { ctx->err = "registration_ndt: the correspondence set does not match the last iteration's rows"; return PCR_EHIP; }
    }
    return PCR_OK;
    });
}
