// pcr_boundary.hip -- boundary point detection by the angle criterion on gfx950.
// Reference behaviour: Open3D t::geometry::PointCloud::ComputeBoundaryPoints (the criterion of PCL's BoundaryEstimation); the reference
// scripts do not call it.  The rule (neighbourhood, tangent frame, angles, largest circular gap, verdict) is stated next to the entry
// point in include/pcr_hip.h.  The neighbour rows are those of the search index's hybrid kernel (pcr_dev_tagged_hybrid, pcr_search.hip)
// over the cloud's own sorted copy; k_boundary_gap is the unit's own kernel.
#include <cmath>
#include "pcr_device.h"

#define BND_BS 256
#define BND_OCT 8
#define BND_OPB (BND_BS / BND_OCT)
#define BND_MAX_NN 200                      // the search index's limit
#define BND_MAX_POINTS (0x7fffffffLL / 4)   // what the sorted copy of a caller cloud takes (pcr_dev_sort_cloud)

// ============================================================================================= the search's view of the cloud
// Rows with a non-finite coordinate become (NaN, NaN, NaN): a NaN fails every distance test, so such a row is nobody's neighbour, and
// as a query it finds nothing; an infinite coordinate no longer reaches the bounds of the Morton lattice.  Finite rows keep their bits.
__global__ void __launch_bounds__(BND_BS) k_bnd_clean(const float *__restrict__ xyz, int n, float *__restrict__ out) {
    const int i = blockIdx.x * BND_BS + threadIdx.x;
    if (i >= n) return;
    const float x = xyz[(size_t)i * 3], y = xyz[(size_t)i * 3 + 1], z = xyz[(size_t)i * 3 + 2];
    const bool fin = fabsf(x) <= 3.4028235e38f && fabsf(y) <= 3.4028235e38f && fabsf(z) <= 3.4028235e38f;
    const float bad = __builtin_nanf("");
    out[(size_t)i * 3] = fin ? x : bad; out[(size_t)i * 3 + 1] = fin ? y : bad; out[(size_t)i * 3 + 2] = fin ? z : bad;
}
// the caller row of every sorted point into its w: what the k-best kernels of the search index order equal distances by
__global__ void __launch_bounds__(BND_BS) k_bnd_tag(float4 *pts, const uint32_t *__restrict__ perm, int n) {
    const int i = blockIdx.x * BND_BS + threadIdx.x;
    if (i < n) pts[i].w = __int_as_float((int)perm[i]);
}

// ========================================================================================================= rules 2 to 4
// Float64 on the float32 data, every product, sum and difference rounded on its own: contraction is switched off inside these
// functions (the form of pcr_d2_f64_unfused), not for the translation unit.
struct BndFrame { double ux, uy, uz, vx, vy, vz; };
__device__ static inline bool bnd_finite(double a) { return fabs(a) <= 1.7976931348623157e308; }
__device__ static inline BndFrame bnd_frame(double nx, double ny, double nz) {
#pragma clang fp contract(off)
    const double ax = fabs(nx), ay = fabs(ny), az = fabs(nz);
    const int a = (ax <= ay && ax <= az) ? 0 : (ay <= az ? 1 : 2);      // smallest |component|; on a tie x before y before z
    const double ex = a == 0 ? 1.0 : 0.0, ey = a == 1 ? 1.0 : 0.0, ez = a == 2 ? 1.0 : 0.0;
    BndFrame f;
    f.vx = ny * ez - nz * ey; f.vy = nz * ex - nx * ez; f.vz = nx * ey - ny * ex;             // v = n x e
    f.ux = f.vy * nz - f.vz * ny; f.uy = f.vz * nx - f.vx * nz; f.uz = f.vx * ny - f.vy * nx; // u = v x n
    return f;
}
__device__ static inline void bnd_project(const BndFrame &f, double dx, double dy, double dz, double *x, double *y) {
#pragma clang fp contract(off)
    *x = (f.ux * dx + f.uy * dy) + f.uz * dz;
    *y = (f.vx * dx + f.vy * dy) + f.vz * dz;
}

// largest value of the octet (values >= 0), in all 8 lanes
__device__ static inline double bnd_octet_max(double v) {
    union { double d; int i[2]; } a, b;
    a.d = v; b.i[0] = pcr_dpp_i<PCR_DPP_XOR1>(a.i[0]); b.i[1] = pcr_dpp_i<PCR_DPP_XOR1>(a.i[1]); v = b.d > v ? b.d : v;
    a.d = v; b.i[0] = pcr_dpp_i<PCR_DPP_XOR2>(a.i[0]); b.i[1] = pcr_dpp_i<PCR_DPP_XOR2>(a.i[1]); v = b.d > v ? b.d : v;
    a.d = v; b.i[0] = pcr_dpp_i<PCR_DPP_HMIRROR>(a.i[0]); b.i[1] = pcr_dpp_i<PCR_DPP_HMIRROR>(a.i[1]); v = b.d > v ? b.d : v;
    return v;
}

// ============================================================================================================ the gap kernel
// One point per octet, the octets in the cloud's Morton order (perm), so that the eight rows of a wavefront read neighbouring points.
// Lane l of the octet takes members l, l + 8, ... of the row: the angle of each goes to place t of the octet's LDS slab, NaN for a
// member that rule 4 skips.  Then every lane looks, for each of its own angles a, for the nearest angle counter-clockwise -- the smallest
// b > a of the slab -- and for the smallest angle of all: the gap after a is b - a, or 2 pi - (a - smallest) for the largest angle.  A NaN
// fails both comparisons, so skipped members need no compaction.  Equal angles give a gap of 0 between them and the same successor.
// The largest gap is an exact maximum: no order of the lanes can change it.  The slab has `cap` doubles per octet, cap = max_nn | 1 (odd:
// the eight octets of a wavefront, which read their slabs at the same place, fall on different banks); the launch asks for that much
// dynamic LDS, so rows of 30 hold 8 KB per workgroup and only max_nn = 200 holds 50 KB.  The loops run to the row's own length.
// No __syncthreads: an octet's slab is written and read by one wavefront, whose LDS operations complete in order.
struct BndArgs {
    const float *xyz;            // the search's view (k_bnd_clean)
    const float *nrm;            // the caller's normals
    const uint32_t *perm;        // sorted -> caller row
    const int32_t *idx;          // n x max_nn caller rows, the first cnt[i] of row i in the rule's order
    const int32_t *cnt;
    int n, max_nn, cap;
    double thresh;               // T of rule 6
    uint8_t *mask; double *gap;  // caller rows; gap optional
};
__global__ void __launch_bounds__(BND_BS) k_boundary_gap(BndArgs a) {
    extern __shared__ double bnd_slab[];
    const int ol = threadIdx.x & 7, ob = threadIdx.x >> 3;
    const int slot = blockIdx.x * BND_OPB + ob;
    const bool inr = slot < a.n;
    if (__ballot(inr) == 0ull) return;
    double *const slab = bnd_slab + (size_t)ob * a.cap;
    const int row = inr ? (int)a.perm[slot] : 0;
    int cnt = inr ? a.cnt[row] : 0;
    cnt = cnt < 0 ? 0 : (cnt > a.max_nn ? a.max_nn : cnt);
    double px = 0.0, py = 0.0, pz = 0.0, nx = 0.0, ny = 0.0, nz = 0.0;
    if (inr) {
        px = (double)a.xyz[(size_t)row * 3]; py = (double)a.xyz[(size_t)row * 3 + 1]; pz = (double)a.xyz[(size_t)row * 3 + 2];
        nx = (double)a.nrm[(size_t)row * 3]; ny = (double)a.nrm[(size_t)row * 3 + 1]; nz = (double)a.nrm[(size_t)row * 3 + 2];
    }
    // rule 2: octet-uniform
    const bool decided = inr && bnd_finite(px) && bnd_finite(py) && bnd_finite(pz) && bnd_finite(nx) && bnd_finite(ny) && bnd_finite(nz) &&
                         !(nx == 0.0 && ny == 0.0 && nz == 0.0);
    if (!decided) cnt = 0;
    const BndFrame f = bnd_frame(nx, ny, nz);
    const int32_t *const ri = a.idx + (size_t)row * (size_t)a.max_nn;
    int m = 0;
    for (int t = ol; t < cnt; t += BND_OCT) {
        const int j = ri[t];
        double ang = __builtin_nan("");
        if (j >= 0 && j < a.n) {
            const double dx = (double)a.xyz[(size_t)j * 3] - px, dy = (double)a.xyz[(size_t)j * 3 + 1] - py, dz = (double)a.xyz[(size_t)j * 3 + 2] - pz;
            double x, y;
            bnd_project(f, dx, dy, dz, &x, &y);
            if (!(x == 0.0 && y == 0.0)) { ang = atan2(y, x); m++; }
        }
        slab[t] = ang;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    const double two_pi = 2.0 * M_PI, inf = (double)__builtin_inff();
    double g = 0.0;
    for (int t = ol; t < cnt; t += BND_OCT) {
        const double av = slab[t];
        if (av != av) continue;
        double succ = inf, lo = av;
        for (int u = 0; u < cnt; u++) {
            const double b = slab[u];
            if (b > av && b < succ) succ = b;
            if (b < lo) lo = b;
        }
        const double d = succ < inf ? succ - av : two_pi - (av - lo);
        g = d > g ? d : g;
    }
    m = pcr_octet_sum_i(m);
    g = bnd_octet_max(g);
    if (inr && ol == 0) {
        const double gap = m > 0 ? g : 0.0;
        a.mask[row] = (m > 0 && gap > a.thresh) ? 1 : 0;
        if (a.gap) a.gap[row] = gap;
    }
}

// ====================================================================================================== C ABI
extern "C" int pcr_boundary_points(pcr_context *ctx, const float *xyz, const float *normals, int64_t n, double radius, int max_nn, double angle_threshold,
                                   uint8_t *boundary_mask, float *out_xyz, int64_t *out_index, int64_t *out_n, double *max_gap, int32_t *counts) {
    return pcr_api_call(ctx, [&]() -> int {
    if (n < 0 || n > BND_MAX_POINTS) { ctx->err = "boundary_points: n is negative or over the int limit"; return PCR_EINVAL; }
    if (n > 0 && (!xyz || !normals)) { ctx->err = "boundary_points: null cloud or normals pointer"; return PCR_EINVAL; }
    if (!std::isfinite(radius) || !(radius > 0.0)) { ctx->err = "boundary_points: radius must be finite and > 0"; return PCR_EINVAL; }
    if (max_nn < 1 || max_nn > BND_MAX_NN) { ctx->err = "boundary_points: max_nn outside 1..200"; return PCR_EINVAL; }
    if (!std::isfinite(angle_threshold) || angle_threshold < 0.0 || angle_threshold > 360.0) {
        ctx->err = "boundary_points: angle_threshold must be finite and in [0, 360]"; return PCR_EINVAL;
    }
    if (out_n) *out_n = 0;
    if (n == 0) return PCR_OK;
    const size_t rows = (size_t)n * (size_t)max_nn;
    PCR_TRY(pcr_arena_reserve(ctx, pcr_scratch_bytes_for(n) + (size_t)n * 96 + rows * 12 + (1u << 16)));
    float *clean = arena<float>(ctx, (size_t)n * 3);
    if (!clean) return PCR_ENOMEM;
    const dim3 flat((unsigned)((n + BND_BS - 1) / BND_BS));
    PCR_LAUNCH(ctx, k_bnd_clean, flat, dim3(BND_BS), 0, ctx->stream, xyz, (int)n, clean);
    DevCloud c; uint32_t *perm = nullptr;
    PCR_TRY(pcr_import_cloud(ctx, clean, nullptr, n, &c, &perm, false));
    PCR_LAUNCH(ctx, k_bnd_tag, flat, dim3(BND_BS), 0, ctx->stream, c.pts, (const uint32_t *)perm, (int)n);
    int32_t *idx = arena<int32_t>(ctx, rows); double *d2 = arena<double>(ctx, rows);
    int32_t *cnt = counts ? counts : arena<int32_t>(ctx, n);
    uint8_t *mask = boundary_mask ? boundary_mask : arena<uint8_t>(ctx, n);
    if (!idx || !d2 || !cnt || !mask) return PCR_ENOMEM;
    // rule 1: the rows in caller order, the queries taken in the cloud's Morton order
    PCR_TRY(pcr_dev_tagged_hybrid(ctx, &c, clean, n, perm, radius, max_nn, idx, d2, cnt));
    BndArgs a; a.xyz = clean; a.nrm = normals; a.perm = perm; a.idx = idx; a.cnt = cnt; a.n = (int)n; a.max_nn = max_nn; a.cap = max_nn | 1;
    a.thresh = angle_threshold * M_PI / 180.0; a.mask = mask; a.gap = max_gap;
    PCR_LAUNCH(ctx, k_boundary_gap, dim3((unsigned)(((size_t)n + BND_OPB - 1) / BND_OPB)), dim3(BND_BS), (size_t)BND_OPB * a.cap * sizeof(double), ctx->stream, a);
    return pcr_emit_kept_rows(ctx, xyz, n, mask, out_xyz, out_index, out_n);      // the boundary points in CALLER order, ascending
    });
}
