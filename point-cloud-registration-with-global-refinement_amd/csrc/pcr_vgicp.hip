// pcr_vgicp.hip -- voxelized GICP (Koide et al., ICRA 2021): the voxel covariance map, the iteration kernel and its loop, and the entry points; the
// specification is the statement in include/pcr_hip.h.  What an ICP loop is made of -- state, icp_finish, graph cache, chunk pump -- is
// pcr_icp_loop.h, shared with pcr_gicp.hip.
//   map build   the member covariances (given, or from the normals as the GICP estimator forms them) are split into two 3-vectors that ride
//                in the attribute slot of the voxel pass (pcr_dev_voxel: float64 sums in input order), one pass each; the cells' Morton keys go
//                into the cell hash of level 0 inside the map's own allocation (map_build_block, pcr_mapgrow.h: the builder of every map block,
//                here with the count and pack kernels in its after-hook); the member counts are integer atomics through that hash; k_vmap_pack
//                lays the rows out as the iteration kernel gathers them.  The host checks that pcr_vmap.hip and pcr_nmap.hip call too (vg_check_*,
//                vg_inside_grid) are defined here and declared in pcr_vgicp.h
//   k_vmap_rows  the candidate rows of every source point at a pose (slot k of point i = map row or -1); the correspondence set is their
//                compaction by the flag scan (pcr_dev_flag_scan) and k_vmap_emit
// Floating-point contraction per source expression only, as in pcr_gicp.hip; the expressions that decide a cell are not contracted at all.
#pragma clang fp contract(on)
#include <cmath>
#include <cstring>
#include "pcr_icp_loop.h"
#include "pcr_mapgrow.h"

#define VG_BS 256

// ================================================================ the iteration
// A sibling of k_icp_iter<ICP_MODE_GICP_COV> (pcr_gicp.hip), not a mode of it, and the whole iteration: there is no search kernel in front of it.
// One lane per source point (caller order, workgroup b owns points [512 b, 512 b + 512) as in k_icp_lin): q = T p with every operation rounded
// once, the cell of q on the map's grid, then 1 / 7 / 27 probes of the map's cell hash.  A probe that finds a cell of at least min_points members
// gathers the row -- (mean, N_v) in one float4, C_v in two -- and adds the three whitened rows of (q, R C_i R^T, mean_v, C_v) into the 30 sums of
// icp_point<ICP_MODE_GICP_COV>, each weighted by the kernel's weight of its own residual times N_v.  sums[28] / sums[29]: squared distances and
// number of the rows; sums[27]: source points with at least one row.  Reduction, ticket, convergence test, LDLT and pose update are icp_finish's.
struct IcpVoxelArgs {
    const float *src_xyz, *src_cov6;   // packed, caller order
    VgicpMapView map;
    int ns, nbh, min_points;
};
// The per-row arithmetic is the REFERENCE's, operation by operation and without contraction (oracle/gicp.c orc_gicp_linearize, cloud_ops.c
// orc_sym3_inv_sqrt): M = C_v + R C_i R^T entry by entry over all nine entries, the cyclic Jacobi sweeps with the oracle's stopping rule,
// W = sum_k V_ik V_jk / sqrt(w_k), J = W [-skew(q) | I] as a 3x3 product with its zero terms, r = (W_r0 d_x + W_r1 d_y) + W_r2 d_z.  Why not
// icp_sym3_inv_sqrt and the fused expressions of icp_point<ICP_MODE_GICP_COV>, which compute the same numbers to 1e-16: under L1 the weight 1 / |r|
// turns a last-bit difference of r into a change of the update that the loop multiplies by 100 to 1000 per iteration, and after
// five iterations the fused form sat 1.8e-3 m from the reference.  With the residuals of a row the reference's own bits, what is left is the order
// of the sums.
__device__ static inline void vg_sym3_inv_sqrt(const double *M /* 9, row-major */, double *W) {
#pragma clang fp contract(off)
    double a[9], v[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
#pragma unroll
    for (int k = 0; k < 9; k++) a[k] = M[k];
    for (int sweep = 0; sweep < 64; sweep++) {
        double off = a[1] * a[1]; off = off + a[2] * a[2]; off = off + a[5] * a[5];
        double diag = a[0] * a[0]; diag = diag + a[4] * a[4]; diag = diag + a[8] * a[8];
        if (off <= 1e-300 || off <= 1e-34 * diag) break;
#pragma unroll
        for (int pq = 0; pq < 3; pq++) {
            const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
            const double apq = a[p * 3 + q];
            if (apq != 0.0) {
                const double theta = (a[q * 3 + q] - a[p * 3 + p]) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
#pragma unroll
                for (int k = 0; k < 3; k++) { const double akp = a[k * 3 + p], akq = a[k * 3 + q]; a[k * 3 + p] = c * akp - sn * akq; a[k * 3 + q] = sn * akp + c * akq; }
#pragma unroll
                for (int k = 0; k < 3; k++) { const double apk = a[p * 3 + k], aqk = a[q * 3 + k]; a[p * 3 + k] = c * apk - sn * aqk; a[q * 3 + k] = sn * apk + c * aqk; }
#pragma unroll
                for (int k = 0; k < 3; k++) { const double vkp = v[k * 3 + p], vkq = v[k * 3 + q]; v[k * 3 + p] = c * vkp - sn * vkq; v[k * 3 + q] = sn * vkp + c * vkq; }
            }
        }
    }
    const double s0 = sqrt(a[0]), s1 = sqrt(a[4]), s2 = sqrt(a[8]);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            double s = 0.0;
            s = s + v[i * 3] * v[j * 3] / s0; s = s + v[i * 3 + 1] * v[j * 3 + 1] / s1; s = s + v[i * 3 + 2] * v[j * 3 + 2] / s2;
            W[i * 3 + j] = s;
        }
}
__device__ static inline double vg_weight(int loss, double k, double r) {
#pragma clang fp contract(off)
    if (loss == PCR_LOSS_L1) return 1.0 / fmax(fabs(r), 1e-300);      // (the oracle: 1 / |r|; the guard only against r == 0)
    if (loss == PCR_LOSS_GM) { const double rr = r * r; const double d = k + rr; return k / (d * d); }
    return 1.0;
}
__device__ static inline void icp_row_vgicp(const IcpArgs &a, const double *Cs /* 9: R C_i R^T, not symmetrised */, double qx, double qy, double qz,
                                            const float4 mu, const float4 c0, const float4 c1, double *acc) {
#pragma clang fp contract(off)
    const double nv = (double)__float_as_int(mu.w);
    const double dx = qx - (double)mu.x, dy = qy - (double)mu.y, dz = qz - (double)mu.z;
    acc[28] += dx * dx + dy * dy + dz * dz; acc[29] += 1.0;
    const double Ct[9] = {c0.x, c0.y, c0.z, c0.y, c0.w, c1.x, c0.z, c1.x, c1.y};
    double M[9], W[9], WS[9];
#pragma unroll
    for (int k = 0; k < 9; k++) M[k] = Ct[k] + Cs[k];
    vg_sym3_inv_sqrt(M, W);
    const double S[9] = {0.0, qz, -qy, -qz, 0.0, qx, qy, -qx, 0.0};      // -skew(q)
    vg_mul3(W, S, WS);
#pragma unroll
    for (int row = 0; row < 3; row++) {
        const double J[6] = {WS[row * 3], WS[row * 3 + 1], WS[row * 3 + 2], W[row * 3], W[row * 3 + 1], W[row * 3 + 2]};
        double r = W[row * 3] * dx; r = r + W[row * 3 + 1] * dy; r = r + W[row * 3 + 2] * dz;
        icp_row6(vg_weight(a.loss, a.loss_k, r) * nv, J, r, acc);
    }
}
__global__ void __launch_bounds__(LIN_BS) k_icp_iter_vgicp(IcpArgs a, IcpVoxelArgs v) {
    icp_iter_frame<ICP_MODE_VGICP, LIN_BS>(a, v.ns, [&](int i, bool live, const double *T, double *acc) {
        if (!live) return;
        double qx, qy, qz;
        vg_transform(T, v.src_xyz[(size_t)i * 3], v.src_xyz[(size_t)i * 3 + 1], v.src_xyz[(size_t)i * 3 + 2], qx, qy, qz);
        const int cx = vg_cell(qx, v.map.org[0], v.map.voxel), cy = vg_cell(qy, v.map.org[1], v.map.voxel), cz = vg_cell(qz, v.map.org[2], v.map.voxel);
        // R C_i R^T once per point: (R C) R^T as the oracle's two 3x3 products, all nine entries
        const float *cs = v.src_cov6 + (size_t)i * 6;
        const double C9[9] = {cs[0], cs[1], cs[2], cs[1], cs[3], cs[4], cs[2], cs[4], cs[5]};
        const double R9[9] = {T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10]};
        double RC[9], RCR[9];
        vg_mul3(R9, C9, RC);
        vg_mul3_bt(RC, R9, RCR);
        const unsigned mask = *v.map.dmask;
        bool any = false;
        for (int k = 0; k < v.nbh; k++) {
            int dx, dy, dz;
            vg_offset(v.nbh, k, dx, dy, dz);
            const int row = vg_row(v.map, mask, cx + dx, cy + dy, cz + dz);
            if (row < 0) continue;
            const float4 mu = v.map.mean4[row];
            if (__float_as_int(mu.w) < v.min_points) continue;
            icp_row_vgicp(a, RCR, qx, qy, qz, mu, v.map.cov8[2 * (size_t)row], v.map.cov8[2 * (size_t)row + 1], acc);
            any = true;
        }
        if (any) acc[27] += 1.0;
    });
}

// The map loop (icp_map_loop, pcr_icp_loop.h) with this unit's kernel and argument block.
static int vgicp_loop(pcr_context *ctx, const float *src_xyz, const float *src_cov6, int64_t n_src, const VgicpMapView *map, int neighborhood, int min_points,
                      const double *T0, const pcr_gicp_params *p, pcr_result *out) {
    if (p->loss < PCR_LOSS_L2 || p->loss > PCR_LOSS_GM) { ctx->err = "registration_voxelized_gicp: params.loss is no robust kernel (pcr_loss_kind)"; return PCR_EINVAL; }
    IcpArgs a; memset(&a, 0, sizeof a);           // (the bytes of both argument blocks are the graph key)
    a.loss = p->loss; a.loss_k = p->loss_k; a.a = 1.0 - p->epsilon;
    a.rel_fit = p->relative_fitness; a.rel_rmse = p->relative_rmse; a.max_it = p->max_iteration;
    IcpVoxelArgs v; memset(&v, 0, sizeof v);
    v.src_xyz = src_xyz; v.src_cov6 = src_cov6; v.map = *map; v.ns = (int)n_src; v.nbh = neighborhood; v.min_points = min_points;
    auto launch = [&](int nb) { PCR_LAUNCH(ctx, k_icp_iter_vgicp, dim3(nb), dim3(LIN_BS), 0, ctx->stream, a, v); };
    return icp_map_loop(ctx, "registration_voxelized_gicp", a, &v, sizeof v, v.ns, ICP_MODE_VGICP, launch, T0, false, out, nullptr);
}

// ================================================================ the map

// (struct pcr_voxel_map: pcr_vgicp.h)

// ---- input checks on the device: *flag |= bit when a value is not finite
__global__ void __launch_bounds__(VG_BS) k_vg_nonfinite(const float *__restrict__ v, size_t count, int bit, int *__restrict__ flag) {
    bool bad = false;
    for (size_t i = (size_t)blockIdx.x * VG_BS + threadIdx.x; i < count; i += (size_t)gridDim.x * VG_BS) bad |= !isfinite(v[i]);
    if (bad) atomicOr(flag, bit);
}

// ---- member covariances as two 3-vectors per point (lo = xx,xy,xz; hi = yy,yz,zz), or packed as cov6 (out6).  From normals: the oracle's
// orc_covariances_from_normals operation by operation -- R = I + [v]x + [v]x^2 / (1 + c) with v = e1 x n, c = n.x (R = I when c < -0.99), then
// (R diag(eps, 1, 1)) R^T as two 3x3 products with their zero terms -- in float64 without contraction, rounded to float32 once
__global__ void __launch_bounds__(VG_BS) k_vmap_member_cov(const float *__restrict__ cov6, const float *__restrict__ normals, double eps, int n,
                                                           float *__restrict__ lo3, float *__restrict__ hi3, float *__restrict__ out6) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * VG_BS + threadIdx.x;
    if (i >= n) return;
    float c6[6];
    if (cov6) {
        for (int t = 0; t < 6; t++) c6[t] = cov6[(size_t)i * 6 + t];
    } else {
        const double x0 = normals[(size_t)i * 3], x1 = normals[(size_t)i * 3 + 1], x2 = normals[(size_t)i * 3 + 2];
        double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        const double c = x0;
        if (!(c < -0.99)) {
            const double v[3] = {0.0, -x2, x1};
            const double sv[9] = {0.0, -v[2], v[1], v[2], 0.0, -v[0], -v[1], v[0], 0.0};
            double sv2[9];
            vg_mul3(sv, sv, sv2);
            const double f = 1.0 / (1.0 + c);
            for (int k = 0; k < 9; k++) { const double t = sv2[k] * f; const double u = sv[k] + t; R[k] = R[k] + u; }
        }
        const double Cd[9] = {eps, 0, 0, 0, 1, 0, 0, 0, 1};
        double RC[9], Cv[9];
        vg_mul3(R, Cd, RC);
        vg_mul3_bt(RC, R, Cv);
        c6[0] = (float)Cv[0]; c6[1] = (float)Cv[1]; c6[2] = (float)Cv[2]; c6[3] = (float)Cv[4]; c6[4] = (float)Cv[5]; c6[5] = (float)Cv[8];
    }
    if (out6) for (int t = 0; t < 6; t++) out6[(size_t)i * 6 + t] = c6[t];
    if (lo3) for (int t = 0; t < 3; t++) { lo3[(size_t)i * 3 + t] = c6[t]; hi3[(size_t)i * 3 + t] = c6[3 + t]; }
}

// ---- member counts: every target point finds its cell's row through the hash (the float64 cell expression of k_voxel_keys) and counts itself
__global__ void __launch_bounds__(VG_BS) k_vmap_count(const float *__restrict__ xyz, int n, VgicpMapView m, int cells, int *__restrict__ count) {
    const int i = blockIdx.x * VG_BS + threadIdx.x;
    if (i >= n) return;
    const int cx = vg_cell((double)xyz[(size_t)i * 3], m.org[0], m.voxel), cy = vg_cell((double)xyz[(size_t)i * 3 + 1], m.org[1], m.voxel),
              cz = vg_cell((double)xyz[(size_t)i * 3 + 2], m.org[2], m.voxel);
    const int row = vg_row(m, *m.dmask, cx, cy, cz);
    if (row >= 0 && row < cells) atomicAdd(&count[row], 1);
}
__global__ void __launch_bounds__(VG_BS) k_vmap_pack(const float4 *__restrict__ mean, const float4 *__restrict__ lo, const float4 *__restrict__ hi,
                                                     const int *__restrict__ count, int cells, float4 *__restrict__ mean4, float4 *__restrict__ cov8) {
    const int v = blockIdx.x * VG_BS + threadIdx.x;
    if (v >= cells) return;
    const float4 p = mean[v], a = lo[v], b = hi[v];
    mean4[v] = make_float4(p.x, p.y, p.z, __int_as_float(count[v]));
    cov8[2 * (size_t)v] = make_float4(a.x, a.y, a.z, b.x);
    cov8[2 * (size_t)v + 1] = make_float4(b.y, b.z, 0.0f, 0.0f);
}
__device__ static inline int vg_compact21(uint64_t x) {      // inverse of pcr_spread21
    x &= 0x1249249249249249ull;
    x = (x | (x >> 2)) & 0x10c30c30c30c30c3ull;
    x = (x | (x >> 4)) & 0x100f00f00f00f00full;
    x = (x | (x >> 8)) & 0x1f0000ff0000ffull;
    x = (x | (x >> 16)) & 0x1f00000000ffffull;
    x = (x | (x >> 32)) & 0x1fffffull;
    return (int)x;
}
__global__ void __launch_bounds__(VG_BS) k_vmap_read(const uint64_t *__restrict__ keys, VgicpMapView m, int cells, int32_t *__restrict__ cell3,
                                                     int32_t *__restrict__ count, float *__restrict__ mean3, float *__restrict__ cov6) {
    const int v = blockIdx.x * VG_BS + threadIdx.x;
    if (v >= cells) return;
    const float4 p = m.mean4[v];
    if (cell3) { const uint64_t k = keys[v]; cell3[(size_t)v * 3] = vg_compact21(k); cell3[(size_t)v * 3 + 1] = vg_compact21(k >> 1); cell3[(size_t)v * 3 + 2] = vg_compact21(k >> 2); }
    if (count) count[v] = __float_as_int(p.w);
    if (mean3) { mean3[(size_t)v * 3] = p.x; mean3[(size_t)v * 3 + 1] = p.y; mean3[(size_t)v * 3 + 2] = p.z; }
    if (cov6) {
        const float4 a = m.cov8[2 * (size_t)v], b = m.cov8[2 * (size_t)v + 1];
        float *o = cov6 + (size_t)v * 6;
        o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w; o[4] = b.x; o[5] = b.y;
    }
}

// ---- rows at a pose: slot[i * nbh + k] = map row of candidate k of source point i, or -1; flags for the scan
struct VgPose { double T[12]; };
__global__ void __launch_bounds__(VG_BS) k_vmap_rows(const float *__restrict__ src_xyz, int ns, VgPose pose, VgicpMapView m, int nbh, int min_points,
                                                     int32_t *__restrict__ slot, uint8_t *__restrict__ flags) {
    const int i = blockIdx.x * VG_BS + threadIdx.x;
    if (i >= ns) return;
    double qx, qy, qz;
    vg_transform(pose.T, src_xyz[(size_t)i * 3], src_xyz[(size_t)i * 3 + 1], src_xyz[(size_t)i * 3 + 2], qx, qy, qz);
    const int cx = vg_cell(qx, m.org[0], m.voxel), cy = vg_cell(qy, m.org[1], m.voxel), cz = vg_cell(qz, m.org[2], m.voxel);
    const unsigned mask = *m.dmask;
    for (int k = 0; k < nbh; k++) {
        int dx, dy, dz;
        vg_offset(nbh, k, dx, dy, dz);
        int row = vg_row(m, mask, cx + dx, cy + dy, cz + dz);
        if (row >= 0 && __float_as_int(m.mean4[row].w) < min_points) row = -1;
        slot[(size_t)i * nbh + k] = row;
        flags[(size_t)i * nbh + k] = row >= 0 ? 1 : 0;
    }
}
// the emit kernel of every correspondence set (vg_emit_rows): candidate e belongs to source point e / nbh
__global__ void __launch_bounds__(VG_BS) k_vmap_emit(const int32_t *__restrict__ slot, const uint8_t *__restrict__ flags, const int *__restrict__ pos, int total, int nbh,
                                                     int32_t *__restrict__ rows2) {
    const int e = blockIdx.x * VG_BS + threadIdx.x;
    if (e >= total || !flags[e]) return;
    const int o = pos[e];
    rows2[2 * (size_t)o] = e / nbh; rows2[2 * (size_t)o + 1] = slot[e];
}

static unsigned vg_blocks(size_t n) { return (unsigned)((n + VG_BS - 1) / VG_BS); }

// PCR_EINVAL naming the first of up to three arrays that holds a non-finite value (one read-back)
int vg_check_finite(pcr_context *ctx, const char *call, const float *const *ptr, const size_t *count, const char *const *name, int arrays) {
    int *flag = arena<int>(ctx, 1);
    if (!flag) return PCR_ENOMEM;
    PCR_HIP_CHECK(ctx, hipMemsetAsync(flag, 0, sizeof(int), ctx->stream));
    for (int k = 0; k < arrays; k++) {
        if (!ptr[k] || count[k] == 0) continue;
        const unsigned nb = vg_blocks(count[k]);
        PCR_LAUNCH(ctx, k_vg_nonfinite, dim3(nb < 1024u ? nb : 1024u), dim3(VG_BS), 0, ctx->stream, ptr[k], count[k], 1 << k, flag);
    }
    int h = 0;
    PCR_HIP_CHECK(ctx, hipMemcpyAsync(&h, flag, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    PCR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < arrays; k++) if (h & (1 << k)) { ctx->err = std::string(call) + ": " + name[k] + " holds a non-finite value"; return PCR_EINVAL; }
    return PCR_OK;
}

// The tail of every correspondence set (this unit's, pcr_ndt.hip's and, with nbh = 1, pcr_pmap.hip's): slot[e] is the map row of candidate e --
// nbh candidates per source point -- and flags[e] whether it is a row; the flag scan and k_vmap_emit compact the flagged candidates in order into
// rows2 as (source point, map row), and *n_rows is read back.  Scratch from the arena the caller has reserved and marked.
int vg_emit_rows(pcr_context *ctx, const int32_t *slot, const uint8_t *flags, size_t total, int nbh, int32_t *rows2, int64_t *n_rows) {
    int *pos = arena<int>(ctx, total), *count = arena<int>(ctx, 1);
    if (!pos || !count) return PCR_ENOMEM;
    PCR_TRY(pcr_dev_flag_scan(ctx, flags, nullptr, (int)total, pos, count));
    PCR_LAUNCH(ctx, k_vmap_emit, dim3(vg_blocks(total)), dim3(VG_BS), 0, ctx->stream, slot, flags, (const int *)pos, (int)total, nbh, rows2);
    return pcr_read_count(ctx, count, n_rows);
}

int vg_check_map(pcr_context *ctx, const pcr_voxel_map *map, const char *call) { return vg_check_handle(ctx, map, call); }
// the member covariances of n points (k_vmap_member_cov) for the units that grow a map: packed cov6 into out6; enqueues only
int vg_member_cov6(pcr_context *ctx, const float *cov6, const float *normals, double eps, int64_t n, float *out6) {
    PCR_LAUNCH(ctx, k_vmap_member_cov, dim3(vg_blocks((size_t)n)), dim3(VG_BS), 0, ctx->stream, cov6, normals, eps, (int)n, (float *)nullptr, (float *)nullptr, out6);
    return PCR_OK;
}
int vg_check_grid_min(pcr_context *ctx, const char *call, const double *grid_min3) {
    if (!grid_min3) { ctx->err = std::string(call) + ": grid_min3 is null"; return PCR_EINVAL; }
    for (int d = 0; d < 3; d++) if (!std::isfinite(grid_min3[d])) { ctx->err = std::string(call) + ": grid_min3 holds a non-finite value"; return PCR_EINVAL; }
    return PCR_OK;
}
// both ends of the members against the grid, on the host before any key is formed (k_voxel_keys has no defence against a negative index)
bool vg_inside_grid(const double *bounds6, const double *grid_min3, double voxel) {
    for (int d = 0; d < 3; d++) {
        const double org = grid_min3[d] - voxel * 0.5;
        const double lo = floor((bounds6[d] - org) / voxel), hi = floor((bounds6[3 + d] - org) / voxel);
        if (!(lo >= 0.0 && hi < 2097152.0)) return false;
    }
    return true;
}
int vg_check_nbh(pcr_context *ctx, const char *call, int neighborhood) {
    if (neighborhood != 1 && neighborhood != 7 && neighborhood != 27) { ctx->err = std::string(call) + ": neighborhood must be 1, 7 or 27"; return PCR_EINVAL; }
    return PCR_OK;
}
static int vg_check_rule(pcr_context *ctx, const char *call, int neighborhood, int min_points) {
    PCR_TRY(vg_check_nbh(ctx, call, neighborhood));
    if (min_points < 1) { ctx->err = std::string(call) + ": min_points_per_voxel < 1"; return PCR_EINVAL; }
    return PCR_OK;
}

extern "C" int pcr_voxel_map_create(pcr_context *ctx, const float *xyz, const float *cov6, const float *normals, int64_t n, double voxel_size, double epsilon,
                                    pcr_voxel_map **out) {
    return pcr_api_call(ctx, [&]() -> int {
    const char *call = "voxel_map_create";
    if (!out) { ctx->err = "voxel_map_create: out is null"; return PCR_EINVAL; }
    *out = nullptr;
    if (!(voxel_size > 0.0) || !std::isfinite(voxel_size)) { ctx->err = "voxel_map_create: voxel_size <= 0"; return PCR_EINVAL; }
    if (!std::isfinite(epsilon)) { ctx->err = "voxel_map_create: epsilon is not finite"; return PCR_EINVAL; }
    if (n < 1 || n > 0x7fffffff / 8 || !xyz) { ctx->err = "voxel_map_create: xyz must hold 1 .. 2^28 - 1 points"; return PCR_EINVAL; }
    if ((cov6 != nullptr) == (normals != nullptr)) { ctx->err = "voxel_map_create: exactly one of cov6 / normals must be given"; return PCR_EINVAL; }
    PCR_TRY(pcr_arena_reserve(ctx, 2 * pcr_scratch_bytes_for(n) + (size_t)n * 96));
    {
        const float *ptr[3] = {xyz, cov6, normals}; const size_t cnt[3] = {(size_t)n * 3, (size_t)n * 6, (size_t)n * 3}; const char *name[3] = {"xyz", "cov6", "normals"};
        PCR_TRY(vg_check_finite(ctx, call, ptr, cnt, name, 3));
    }
    double b6[6];
    PCR_TRY(pcr_dev_bounds(ctx, xyz, n, b6));
    float *lo3 = arena<float>(ctx, (size_t)n * 3), *hi3 = arena<float>(ctx, (size_t)n * 3);
    if (!lo3 || !hi3) return PCR_ENOMEM;
    PCR_LAUNCH(ctx, k_vmap_member_cov, dim3(vg_blocks((size_t)n)), dim3(VG_BS), 0, ctx->stream, cov6, normals, epsilon, (int)n, lo3, hi3, (float *)nullptr);
    // the voxel pass twice over the same points: the same keys, the same stable sort, so row v of both passes is the same cell
    DevCloud va, vb;
    PCR_TRY(pcr_alloc_cloud(ctx, &va, (int)n, true, false));
    PCR_TRY(pcr_alloc_cloud(ctx, &vb, (int)n, true, false));
    PCR_TRY(pcr_dev_voxel(ctx, xyz, lo3, n, b6, voxel_size, &va));
    PCR_TRY(pcr_dev_voxel(ctx, xyz, hi3, n, b6, voxel_size, &vb));
    int64_t cells = 0;
    PCR_TRY(pcr_read_count(ctx, va.n, &cells));
    if (cells < 1 || cells > n) { ctx->err = "voxel_map_create: the voxel pass returned no cells"; return PCR_EHIP; }

    pcr_voxel_map *m = new pcr_voxel_map();
    m->device = ctx->device;
    for (int d = 0; d < 3; d++) m->view.org[d] = b6[d] - voxel_size * 0.5;      // (pcr_dev_voxel's origin)
    m->view.voxel = voxel_size;
    for (int d = 0; d < 3; d++) m->grid_min[d] = b6[d];
    // the map's arrays and the hash table come out of the map's block; the counts, through that hash, are scratch of the context's arena
    MapBlock<VmapRow> nb;
    const int rc = map_build_block<VmapRow>(ctx, call, cells, &nb, [&](const VmapRow::Out &o) -> int {
        PCR_HIP_CHECK(ctx, hipMemcpyAsync(o.keys, va.keys, sizeof(uint64_t) * (size_t)cells, hipMemcpyDeviceToDevice, ctx->stream));
        return PCR_OK;
    }, [&](const MapBlock<VmapRow> &b) -> int {
        map_adopt<VmapRow>(m, b, cells);      // (the builder frees the block if anything after this fails)
        int *count = arena<int>(ctx, (size_t)cells);
        if (!count) return PCR_ENOMEM;
        PCR_HIP_CHECK(ctx, hipMemsetAsync(count, 0, sizeof(int) * (size_t)cells, ctx->stream));
        PCR_LAUNCH(ctx, k_vmap_count, dim3(vg_blocks((size_t)n)), dim3(VG_BS), 0, ctx->stream, xyz, (int)n, m->view, (int)cells, count);
        PCR_LAUNCH(ctx, k_vmap_pack, dim3(vg_blocks((size_t)cells)), dim3(VG_BS), 0, ctx->stream, (const float4 *)va.pts, (const float4 *)va.nrm, (const float4 *)vb.nrm,
                   (const int *)count, (int)cells, b.out.mean4, b.out.cov8);
        return PCR_OK;
    });
    if (rc != PCR_OK) { delete m; return rc; }
    *out = m;
    return PCR_OK;
    });
}

extern "C" int pcr_voxel_map_destroy(pcr_voxel_map *map) {
    if (!map) return PCR_OK;
    if (map->block) {
        if (hipSetDevice(map->device) != hipSuccess) return PCR_EHIP;
        (void)hipFree(map->block);                            // waits for the device: no call is still reading the block
    }
    delete map;
    return PCR_OK;
}

extern "C" int pcr_voxel_map_size(const pcr_voxel_map *map, int64_t *cells) {
    if (!map || !cells) return PCR_EINVAL;
    *cells = map->cells;
    return PCR_OK;
}

extern "C" int pcr_voxel_map_read(pcr_context *ctx, const pcr_voxel_map *map, int32_t *cell3, int32_t *count, float *mean3, float *cov6) {
    return pcr_api_call(ctx, [&]() -> int {
    PCR_TRY(vg_check_map(ctx, map, "voxel_map_read"));
    PCR_LAUNCH(ctx, k_vmap_read, dim3(vg_blocks((size_t)map->cells)), dim3(VG_BS), 0, ctx->stream, (const uint64_t *)map->keys, map->view, (int)map->cells, cell3, count, mean3, cov6);
    return PCR_OK;
    });
}

// rows of the rule at the pose T (16 doubles, host) into rows2; scratch from the arena the caller has reserved
static int vg_rows(pcr_context *ctx, const pcr_voxel_map *map, const float *src_xyz, int64_t n_src, const double *T, int nbh, int min_points, int32_t *rows2, int64_t *n_rows) {
    *n_rows = 0;
    if (n_src == 0) return PCR_OK;
    ArenaMark mark(ctx);
    const size_t total = (size_t)n_src * nbh;
    int32_t *slot = arena<int32_t>(ctx, total);
    uint8_t *flags = arena<uint8_t>(ctx, total);
    if (!slot || !flags) return PCR_ENOMEM;
    VgPose pose; memcpy(pose.T, T, sizeof pose.T);
    PCR_LAUNCH(ctx, k_vmap_rows, dim3(vg_blocks((size_t)n_src)), dim3(VG_BS), 0, ctx->stream, src_xyz, (int)n_src, pose, map->view, nbh, min_points, slot, flags);
    return vg_emit_rows(ctx, slot, flags, total, nbh, rows2, n_rows);
}
static size_t vg_rows_scratch(int64_t n_src, int nbh) { return (size_t)(n_src > 0 ? n_src : 1) * nbh * 10 + (1u << 20); }

int vg_check_T(pcr_context *ctx, const char *call, const char *name, const double *T) {
    if (!T) { ctx->err = std::string(call) + ": " + name + " is null"; return PCR_EINVAL; }
    for (int k = 0; k < 16; k++) if (!std::isfinite(T[k])) { ctx->err = std::string(call) + ": " + name + " holds a non-finite value"; return PCR_EINVAL; }
    return PCR_OK;
}
int vg_check_src(pcr_context *ctx, const char *call, const float *src_xyz, int64_t n_src, int nbh) {
    if (n_src < 0 || (n_src > 0 && !src_xyz) || (double)n_src * nbh > (double)(0x7fffffff / 4)) { ctx->err = std::string(call) + ": src_xyz is null or too large"; return PCR_EINVAL; }
    return PCR_OK;
}

extern "C" int pcr_voxel_map_correspondences(pcr_context *ctx, const pcr_voxel_map *map, const float *src_xyz, int64_t n_src, const double *T, int neighborhood,
                                             int min_points_per_voxel, int32_t *rows2, int64_t *n_rows) {
    return pcr_api_call(ctx, [&]() -> int {
    const char *call = "voxel_map_correspondences";
    PCR_TRY(vg_check_map(ctx, map, call));
    PCR_TRY(vg_check_rule(ctx, call, neighborhood, min_points_per_voxel));
    PCR_TRY(vg_check_src(ctx, call, src_xyz, n_src, neighborhood));
    if (!n_rows || (n_src > 0 && !rows2)) { ctx->err = "voxel_map_correspondences: rows2 / n_rows is null"; return PCR_EINVAL; }
    PCR_TRY(vg_check_T(ctx, call, "T", T));
    PCR_TRY(pcr_arena_reserve(ctx, vg_rows_scratch(n_src, neighborhood)));
    const float *ptr[1] = {src_xyz}; const size_t cnt[1] = {(size_t)n_src * 3}; const char *name[1] = {"src_xyz"};
    PCR_TRY(vg_check_finite(ctx, call, ptr, cnt, name, 1));
    return vg_rows(ctx, map, src_xyz, n_src, T, neighborhood, min_points_per_voxel, rows2, n_rows);
    });
}

extern "C" int pcr_registration_voxelized_gicp(pcr_context *ctx, const float *src_xyz, const float *src_cov6, const float *src_normals, int64_t n_src,
                                               const pcr_voxel_map *map, const double *init_T, const pcr_vgicp_params *params, pcr_result *result,
                                               int32_t *correspondences) {
    return pcr_api_call(ctx, [&]() -> int {
    const char *call = "registration_voxelized_gicp";
    if (!params || !result) { ctx->err = "registration_voxelized_gicp: params / result is null"; return PCR_EINVAL; }
    PCR_TRY(vg_check_map(ctx, map, call));
    PCR_TRY(vg_check_rule(ctx, call, params->neighborhood, params->min_points_per_voxel));
    PCR_TRY(vg_check_src(ctx, call, src_xyz, n_src, params->neighborhood));
    if (n_src > 0 && !src_cov6 && !src_normals) { ctx->err = "registration_voxelized_gicp: src_cov6 is missing (and there are no src_normals to form it from)"; return PCR_EINVAL; }
    if (params->max_iteration < 0) { ctx->err = "registration_voxelized_gicp: params.max_iteration < 0"; return PCR_EINVAL; }
    if (!std::isfinite(params->epsilon) || !std::isfinite(params->loss_k)) { ctx->err = "registration_voxelized_gicp: params.epsilon / loss_k is not finite"; return PCR_EINVAL; }
    PCR_TRY(vg_check_T(ctx, call, "init_T", init_T));
    PCR_TRY(pcr_arena_reserve(ctx, vg_rows_scratch(n_src, params->neighborhood) + (size_t)(n_src > 0 ? n_src : 1) * 32 + (4u << 20)));
    {
        const float *ptr[3] = {src_xyz, src_cov6, src_cov6 ? nullptr : src_normals}; const size_t cnt[3] = {(size_t)n_src * 3, (size_t)n_src * 6, (size_t)n_src * 3};
        const char *name[3] = {"src_xyz", "src_cov6", "src_normals"};
        PCR_TRY(vg_check_finite(ctx, call, ptr, cnt, name, 3));
    }
    const float *cov = src_cov6;
    if (!cov && n_src > 0) {
        float *c6 = arena<float>(ctx, (size_t)n_src * 6);
        if (!c6) return PCR_ENOMEM;
        PCR_LAUNCH(ctx, k_vmap_member_cov, dim3(vg_blocks((size_t)n_src)), dim3(VG_BS), 0, ctx->stream, (const float *)nullptr, src_normals, params->epsilon, (int)n_src,
                   (float *)nullptr, (float *)nullptr, c6);
        cov = c6;
    }
    pcr_gicp_params g;
    memset(&g, 0, sizeof g);
    g.loss = params->loss; g.loss_k = params->loss_k; g.epsilon = params->epsilon;
    g.relative_fitness = params->relative_fitness; g.relative_rmse = params->relative_rmse; g.max_iteration = params->max_iteration;
    PCR_TRY(vgicp_loop(ctx, src_xyz, cov, n_src, &map->view, params->neighborhood, params->min_points_per_voxel, init_T, &g, result));
    if (correspondences) {      // the rows of the last launch: those at the returned pose
        int64_t rows = 0;
        PCR_TRY(vg_rows(ctx, map, src_xyz, n_src, result->transformation, params->neighborhood, params->min_points_per_voxel, correspondences, &rows));
        if (rows != result->n_correspondences) { ctx->err = "registration_voxelized_gicp: the correspondence set does not match the last iteration's rows"; return PCR_EHIP; }
    }
    return PCR_OK;
    });
}
