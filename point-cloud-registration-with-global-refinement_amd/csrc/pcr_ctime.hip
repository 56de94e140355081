// pcr_ctime.hip -- continuous time: per-point times, scan deskewing and the continuous-time iteration on the voxel point map; the specification is
// the statement in include/pcr_hip.h (continuous time).  The map, its search (pm_match_own / pm_search) and the robust kernels are pcr_pmap.h's.
//   the pose of a point   every lane forms alpha = (time - t0) / (t1 - t0), E(alpha phi) and R(alpha) = R_b E for its own point in float64; phi =
//                         Log(R_b^T R_e) is formed once per call on the host (ct_log3)
//   k_deskew              one point per lane, one pass: the point into the sensor frame at alpha_ref, its normal rotated the same way
//   k_pmap_lin_ct         the whole linearisation, one launch, in k_icp_iter_pmap's shape: workgroup b owns the source points [512 b, 512 b + 512) in
//                         caller order; every lane places its point, the octets search (eight rounds, every exchange in wave-uniform control flow),
//                         every lane forms the 27 sums of its rigid row(s) -- upper J6^T J6 and J6^T r -- and the workgroup reduces them three
//                         times, weighted by the alpha moments (1 - a)^2 / a (1 - a) / a^2, through the halving butterfly of the 16-lane rows
//                         (30 + 27 + 21 = 78 sums; a lane never holds more than 32 at once) and the rows of an LDS table in order.  The
//                         workgroup's 78 sums go out write-through; the workgroup that takes the last ticket adds the tiles in ascending order
//                         and writes the 160 doubles the host reads: H (144), g (12), rows, sum d^2, sum r^2, 0
// Nothing in this unit is contracted: every product and sum of the rule is rounded once.
#pragma clang fp contract(off)
#include <cmath>
#include <cstring>
#include <string>
#include "pcr_icp_loop.h"
#include "pcr_pmap.h"

#define CT_BS LIN_BS          // the tile of the SUMS rule: 512 source points
#define CT_DS 256
#define CT_NV 78              // [0, 21) H_bb  [21, 27) g_b  [27] sum r^2  [28] sum d^2  [29] rows  [30, 51) H_be  [51, 57) g_e  [57, 78) H_ee
#define CT_NVP 80
#define CT_OUT 160

// E(v) = I + A [v]x + B [v]x^2, row-major; theta^2 is the sum (x x + y y) + z z and theta its root; v == 0 gives I exactly
__host__ __device__ static inline void ct_exp3(double x, double y, double z, double *E) {
    const double xx = x * x, yy = y * y, zz = z * z;
    double t2 = xx + yy;
    t2 = t2 + zz;
    const double th = sqrt(t2);
    double A, B;
    if (th >= 1e-4) { A = sin(th) / th; B = (1.0 - cos(th)) / t2; }
    else { A = 1.0 - t2 / 6.0; B = 0.5 - t2 / 24.0; }
    const double xy = x * y, xz = x * z, yz = y * z;
    E[0] = 1.0 - B * (yy + zz); E[1] = B * xy - A * z;       E[2] = B * xz + A * y;
    E[3] = B * xy + A * z;       E[4] = 1.0 - B * (xx + zz); E[5] = B * yz - A * x;
    E[6] = B * xz - A * y;       E[7] = B * yz + A * x;       E[8] = 1.0 - B * (xx + yy);
}
// c = a b of row-major 3x3 matrices, every entry (a_i0 b_0j + a_i1 b_1j) + a_i2 b_2j (vg_mul3's expression, for the host too)
__host__ __device__ static inline void ct_mul3(const double *a, const double *b, double *c) {
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) { double s = a[i * 3] * b[j]; s = s + a[i * 3 + 1] * b[3 + j]; s = s + a[i * 3 + 2] * b[6 + j]; c[i * 3 + j] = s; }
}
// the rotated point ((r0 x + r1 y) + r2 z) of every row: the ROWS expression of the voxel maps before the translation is added
__device__ static inline void ct_rotate(const double *R, double x, double y, double z, double &ux, double &uy, double &uz) {
    const double ax = R[0] * x, bx = R[1] * y, cx = R[2] * z;
    const double ay = R[3] * x, by = R[4] * y, cy = R[5] * z;
    const double az = R[6] * x, bz = R[7] * y, cz = R[8] * z;
    double sx = ax + bx, sy = ay + by, sz = az + bz;
    ux = sx + cx; uy = sy + cy; uz = sz + cz;
}
// phi = Log(R), the rotation vector with its angle in [0, pi] (host, float64).  w = the vector of (R - R^T) / 2 has length sin(theta) and
// c = (trace - 1) / 2 is cos(theta): theta = atan2(|w|, c).  Away from pi the axis is w / |w|; near pi, where w vanishes, it is read from the
// diagonal (R + R^T) / 2 = cos I + (1 - cos) a a^T, its largest entry first and the signs of the others from the off-diagonal sums, the whole
// vector turned so that it agrees with w.
static void ct_log3(const double *R, double *phi) {
    const double w[3] = {(R[7] - R[5]) * 0.5, (R[2] - R[6]) * 0.5, (R[3] - R[1]) * 0.5};
    const double s = sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
    const double c = ((R[0] + R[4]) + R[8] - 1.0) * 0.5;
    const double theta = atan2(s, c);
    if (s < 1e-8 && c > 0.0) { phi[0] = w[0]; phi[1] = w[1]; phi[2] = w[2]; return; }      // theta / sin(theta) = 1 + theta^2 / 6: below 1e-16 here
    if (c > -0.99) { const double f = theta / s; phi[0] = w[0] * f; phi[1] = w[1] * f; phi[2] = w[2] * f; return; }
    const double d[3] = {R[0], R[4], R[8]};
    int k = 0;
    if (d[1] > d[k]) k = 1;
    if (d[2] > d[k]) k = 2;
    double a[3];
    const double one_c = 1.0 - c;
    a[k] = sqrt(fmax((d[k] - c) / one_c, 0.0));
    for (int j = 0; j < 3; j++) if (j != k) a[j] = a[k] > 0.0 ? (R[k * 3 + j] + R[j * 3 + k]) * 0.5 / (one_c * a[k]) : 0.0;
    const double n = sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]);
    double sign = (a[0] * w[0] + a[1] * w[1]) + a[2] * w[2] < 0.0 ? -1.0 : 1.0;
    for (int j = 0; j < 3; j++) phi[j] = n > 0.0 ? sign * theta * a[j] / n : 0.0;
}

// ================================================================ deskew
struct CtDeskewArgs {
    const float *xyz, *nrm, *times; int n;
    double phi[3], tau[3];       // of the motion D: Log(R_D), t_D
    double t0, span;             // alpha = (time - t0) / span
    double Rr[9], tr[3];         // R(alpha_ref) and alpha_ref tau
    float *out_xyz, *out_nrm;
};
__global__ void __launch_bounds__(CT_DS) k_deskew(CtDeskewArgs a) {
    const int i = blockIdx.x * CT_DS + threadIdx.x;
    if (i >= a.n) return;
    const double alpha = ((double)a.times[i] - a.t0) / a.span;
    double R[9];
    ct_exp3(alpha * a.phi[0], alpha * a.phi[1], alpha * a.phi[2], R);      // (T_b = I: R(alpha) = I E is E, entry by entry)
    double w[3];
    ct_rotate(R, a.xyz[(size_t)i * 3], a.xyz[(size_t)i * 3 + 1], a.xyz[(size_t)i * 3 + 2], w[0], w[1], w[2]);
#pragma unroll
    for (int d = 0; d < 3; d++) { w[d] = w[d] + alpha * a.tau[d]; w[d] = w[d] - a.tr[d]; }
#pragma unroll
    for (int d = 0; d < 3; d++) {                                          // R(alpha_ref)^T w
        double s = a.Rr[d] * w[0] + a.Rr[3 + d] * w[1];
        s = s + a.Rr[6 + d] * w[2];
        a.out_xyz[(size_t)i * 3 + d] = (float)s;
    }
    if (!a.nrm) return;
    double m[3];
    ct_rotate(R, a.nrm[(size_t)i * 3], a.nrm[(size_t)i * 3 + 1], a.nrm[(size_t)i * 3 + 2], m[0], m[1], m[2]);
#pragma unroll
    for (int d = 0; d < 3; d++) {
        double s = a.Rr[d] * m[0] + a.Rr[3 + d] * m[1];
        s = s + a.Rr[6 + d] * m[2];
        a.out_nrm[(size_t)i * 3 + d] = (float)s;
    }
}

// ================================================================ host checks
static int ct_check_pose(pcr_context *ctx, const char *call, const char *name, const double *T) {
    PCR_TRY(vg_check_T(ctx, call, name, T));
    if (T[12] != 0.0 || T[13] != 0.0 || T[14] != 0.0 || T[15] != 1.0) { ctx->err = std::string(call) + ": " + name + " is no pose (its last row must be 0 0 0 1)"; return PCR_EINVAL; }
    return PCR_OK;
}
static int ct_check_span(pcr_context *ctx, const char *call, double t0, double t1) {
    if (!std::isfinite(t0)) { ctx->err = std::string(call) + ": t0 is not finite"; return PCR_EINVAL; }
    if (!std::isfinite(t1)) { ctx->err = std::string(call) + ": t1 is not finite"; return PCR_EINVAL; }
    if (!(t1 > t0)) { ctx->err = std::string(call) + ": t1 must be greater than t0"; return PCR_EINVAL; }
    return PCR_OK;
}

extern "C" int pcr_deskew(pcr_context *ctx, const float *xyz, const float *normals, const float *times, int64_t n, const double *motion16, double t0, double t1, double alpha_ref,
                          float *out_xyz, float *out_normals) {
    return pcr_api_call(ctx, [&]() -> int {
    const char *call = "deskew";
    if (n < 0 || n > 0x7fffffff / 8 || (n > 0 && !xyz)) { ctx->err = "deskew: xyz is null or too large"; return PCR_EINVAL; }
    if (n > 0 && !times) { ctx->err = "deskew: times is null"; return PCR_EINVAL; }
    if (n > 0 && !out_xyz) { ctx->err = "deskew: out_xyz is null"; return PCR_EINVAL; }
    if ((normals != nullptr) != (out_normals != nullptr)) { ctx->err = "deskew: out_normals must be given exactly when normals is"; return PCR_EINVAL; }
    PCR_TRY(ct_check_pose(ctx, call, "motion16", motion16));
    PCR_TRY(ct_check_span(ctx, call, t0, t1));
    if (!std::isfinite(alpha_ref)) { ctx->err = "deskew: alpha_ref is not finite"; return PCR_EINVAL; }
    if (n == 0) return PCR_OK;
    PCR_TRY(pcr_arena_reserve(ctx, 4u << 20));
    {
        const float *ptr[3] = {xyz, normals, times}; const size_t cnt[3] = {(size_t)n * 3, (size_t)n * 3, (size_t)n}; const char *name[3] = {"xyz", "normals", "times"};
        PCR_TRY(vg_check_finite(ctx, call, ptr, cnt, name, 3));
    }
    CtDeskewArgs a; memset(&a, 0, sizeof a);
    a.xyz = xyz; a.nrm = normals; a.times = times; a.n = (int)n; a.out_xyz = out_xyz; a.out_nrm = out_normals;
    const double RD[9] = {motion16[0], motion16[1], motion16[2], motion16[4], motion16[5], motion16[6], motion16[8], motion16[9], motion16[10]};
    ct_log3(RD, a.phi);
    a.t0 = t0; a.span = t1 - t0;
    ct_exp3(alpha_ref * a.phi[0], alpha_ref * a.phi[1], alpha_ref * a.phi[2], a.Rr);
    for (int d = 0; d < 3; d++) { a.tau[d] = motion16[4 * d + 3]; a.tr[d] = alpha_ref * a.tau[d]; }
    PCR_LAUNCH(ctx, k_deskew, dim3((unsigned)((n + CT_DS - 1) / CT_DS)), dim3(CT_DS), 0, ctx->stream, a);
    return PCR_OK;
    });
}

// ================================================================ the continuous-time iteration
struct CtLinArgs {
    const float *src_xyz, *src_times;      // packed, caller order
    PmapView map;
    int ns, nbh, plane, loss;              // plane: 1 point to plane, 0 point to point
    double loss_k, max_d2;
    const int32_t *ncount; int kmin;       // k_pmap_lin_ct<true> alone (point to plane on an estimated map): a match whose row has ncount < kmin is no row
    double Rb[9], tb[3], dt[3], phi[3];    // R_b, t_b, t_e - t_b, Log(R_b^T R_e)
    double t0, span;
    double *partials;                      // one row of CT_NVP per workgroup
    unsigned *ticket;                      // zeroed before every launch
    double *out;                           // CT_OUT doubles
    int32_t *matches;                      // optional: the map row of every source point, or -1
};
template <bool EST>
__global__ void __launch_bounds__(CT_BS) k_pmap_lin_ct(CtLinArgs a) {
    __shared__ double red[CT_BS / 16][CT_NVP];      // one row per 16-lane DPP row; the last workgroup stages the tiles' rows through it
    __shared__ double fin[CT_NVP];
    __shared__ int is_last;
    const int nb = (int)gridDim.x;
    const int i = blockIdx.x * CT_BS + threadIdx.x;
    const bool live = i < a.ns;
    double alpha = 0.0, qx = 0.0, qy = 0.0, qz = 0.0, ux = 0.0, uy = 0.0, uz = 0.0;
    if (live) {
        alpha = ((double)a.src_times[i] - a.t0) / a.span;
        double E[9], R[9];
        ct_exp3(alpha * a.phi[0], alpha * a.phi[1], alpha * a.phi[2], E);
        ct_mul3(a.Rb, E, R);
        ct_rotate(R, a.src_xyz[(size_t)i * 3], a.src_xyz[(size_t)i * 3 + 1], a.src_xyz[(size_t)i * 3 + 2], ux, uy, uz);
        const double tx = a.tb[0] + alpha * a.dt[0], ty = a.tb[1] + alpha * a.dt[1], tz = a.tb[2] + alpha * a.dt[2];
        qx = ux + tx; qy = uy + ty; qz = uz + tz;
    }
    double d2; int row;
    pm_match_own(a.map, a.nbh, live, qx, qy, qz, a.max_d2, d2, row);
    if (EST && row >= 0 && a.ncount[row] < a.kmin) row = -1;
    if (live && a.matches) a.matches[i] = row;
    // the rigid part of this lane's row(s): [0, 21) upper w J6^T J6, [21, 27) w J6^T r
    double A[27];
#pragma unroll
    for (int k = 0; k < 27; k++) A[k] = 0.0;
    double sr2 = 0.0, sd2 = 0.0, cnt = 0.0;
    if (live && row >= 0) {
        sd2 = d2; cnt = 1.0;
        sr2 = pm_row27(a.map, a.plane, a.loss, a.loss_k, row, qx, qy, qz, ux, uy, uz, A);      // (the lever is u = R p)
    }
    // ---- the workgroup's sums: three passes of the halving butterfly (lane r of a 16-lane row ends with the sums of values r and 16 + r), so that a
    // lane holds one alpha moment of the rigid part at a time, then the 32 rows in order
    const int lane = threadIdx.x & 63, r16 = lane & 15, wrow = threadIdx.x >> 4;
    const double b1 = 1.0 - alpha;
    {
        const double m = b1 * b1;
        double v[30], lo, hi;
#pragma unroll
        for (int k = 0; k < 21; k++) v[k] = m * A[k];
#pragma unroll
        for (int k = 21; k < 27; k++) v[k] = b1 * A[k];
        v[27] = sr2; v[28] = sd2; v[29] = cnt;
        pcr_row16_sum_halving<30>(v, lane, &lo, &hi);
        red[wrow][r16] = lo;
        if (16 + r16 < 30) red[wrow][16 + r16] = hi;
    }
    {
        const double m = alpha * b1;
        double v[27], lo, hi;
#pragma unroll
        for (int k = 0; k < 21; k++) v[k] = m * A[k];
#pragma unroll
        for (int k = 21; k < 27; k++) v[k] = alpha * A[k];
        pcr_row16_sum_halving<27>(v, lane, &lo, &hi);
        red[wrow][30 + r16] = lo;
        if (16 + r16 < 27) red[wrow][30 + 16 + r16] = hi;
    }
    {
        const double m = alpha * alpha;
        double v[21], lo, hi;
#pragma unroll
        for (int k = 0; k < 21; k++) v[k] = m * A[k];
        pcr_row16_sum_halving<21>(v, lane, &lo, &hi);
        red[wrow][57 + r16] = lo;
        if (16 + r16 < 21) red[wrow][57 + 16 + r16] = hi;
    }
    __syncthreads();
    if (threadIdx.x < CT_NV) {
        double s = red[0][threadIdx.x];
#pragma unroll 8
        for (int w = 1; w < CT_BS / 16; w++) s += red[w][threadIdx.x];
        // published write-through, as icp_finish publishes its partial row: no release fence
        __hip_atomic_store(&a.partials[(size_t)blockIdx.x * CT_NVP + threadIdx.x], s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // every storing wave drains its stores ...
    __syncthreads();                                       // ... before ONE lane signals for the workgroup
    if (threadIdx.x == 0) {
        const unsigned int t = __hip_atomic_fetch_add(a.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        is_last = (t == (unsigned int)(nb - 1));
    }
    __syncthreads();
    if (!is_last) return;
    // ---- the last workgroup: the tiles in ascending order.  32 rows at a time are read by all lanes at once (agent-scope loads, which do not read
    // this compute unit's cache) into the table, and column c's lane adds them in order
    double s = 0.0;
    for (int b0 = 0; b0 < nb; b0 += CT_BS / 16) {           // (uniform over the workgroup)
        const int rows = min(CT_BS / 16, nb - b0);
        __syncthreads();
        for (int k = threadIdx.x; k < rows * CT_NVP; k += CT_BS) {
            const int r = k / CT_NVP, c = k - r * CT_NVP;
            red[r][c] = c < CT_NV ? __hip_atomic_load(&a.partials[(size_t)(b0 + r) * CT_NVP + c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
        }
        __syncthreads();
        if (threadIdx.x < CT_NV) for (int r = 0; r < rows; r++) s += red[r][threadIdx.x];
    }
    if (threadIdx.x < CT_NVP) fin[threadIdx.x] = threadIdx.x < CT_NV ? s : 0.0;
    __syncthreads();
    if (threadIdx.x < CT_OUT) {
        const int t = threadIdx.x;
        double o = 0.0;
        if (t < 144) {
            const int p = t / 12, q = t - p * 12;
            const int bp = p / 6, bq = q / 6, pp = p - bp * 6, qq = q - bq * 6;
            const int lo = pp < qq ? pp : qq, hi = pp < qq ? qq : pp;
            const int tri = lo * 6 - lo * (lo - 1) / 2 + (hi - lo);
            o = fin[(bp == bq ? (bp == 0 ? 0 : 57) : 30) + tri];
        } else if (t < 156) {
            const int p = t - 144;
            o = p < 6 ? fin[21 + p] : fin[51 + p - 6];
        } else if (t == 156) o = fin[29];
        else if (t == 157) o = fin[28];
        else if (t == 158) o = fin[27];
        a.out[t] = o;
    }
}

extern "C" int pcr_point_map_linearize_continuous(pcr_context *ctx, const pcr_point_map *map, const float *src_xyz, const float *src_times, int64_t n_src, const double *T_begin16,
                                                  const double *T_end16, double t0, double t1, double max_correspondence_distance, int neighborhood,
                                                  const pcr_estimation *estimation, double *H144, double *g12, int64_t *rows, double *sum_d2, double *sum_r2, int32_t *matches) {
    return pcr_api_call(ctx, [&]() -> int {
    const char *call = "point_map_linearize_continuous";
    PCR_TRY(pm_check_search(ctx, call, map, src_xyz, n_src, T_begin16, "T_begin16", neighborhood, max_correspondence_distance));
    PCR_TRY(ct_check_pose(ctx, call, "T_begin16", T_begin16));
    PCR_TRY(ct_check_pose(ctx, call, "T_end16", T_end16));
    PCR_TRY(pm_check_estimation(ctx, call, map, estimation));
    if (n_src > 0 && !src_times) { ctx->err = "point_map_linearize_continuous: src_times is null"; return PCR_EINVAL; }
    PCR_TRY(ct_check_span(ctx, call, t0, t1));
    const int ns = (int)n_src;
    const int nb = ns > 0 ? (ns + CT_BS - 1) / CT_BS : 1;
    PCR_TRY(pcr_arena_reserve(ctx, pm_search_scratch(n_src) + (size_t)nb * CT_NVP * sizeof(double)));
    {
        const float *ptr[2] = {src_xyz, src_times}; const size_t cnt[2] = {(size_t)n_src * 3, (size_t)n_src}; const char *name[2] = {"src_xyz", "src_times"};
        PCR_TRY(vg_check_finite(ctx, call, ptr, cnt, name, 2));
    }
    ArenaMark mark(ctx);
    unsigned *ticket = arena<unsigned>(ctx, 4);            // a block of its own, 16 bytes
    double *out = arena<double>(ctx, CT_OUT), *partials = arena<double>(ctx, (size_t)nb * CT_NVP);
    if (!ticket || !out || !partials) return PCR_ENOMEM;
    CtLinArgs a; memset(&a, 0, sizeof a);
    a.src_xyz = src_xyz; a.src_times = src_times; a.map = map->view; a.ns = ns; a.nbh = neighborhood;
    a.plane = estimation->kind == PCR_EST_POINT_TO_PLANE ? 1 : 0; a.loss = estimation->loss; a.loss_k = estimation->loss_k;
    a.max_d2 = max_correspondence_distance * max_correspondence_distance;
    const bool validity = pm_reads_validity(map, estimation);
    if (validity) { a.ncount = map->ncount; a.kmin = map->est_min; }
    double RbT[9], Re[9], D[9];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) { a.Rb[r * 3 + c] = T_begin16[r * 4 + c]; RbT[c * 3 + r] = T_begin16[r * 4 + c]; Re[r * 3 + c] = T_end16[r * 4 + c]; }
    ct_mul3(RbT, Re, D);
    ct_log3(D, a.phi);
    for (int d = 0; d < 3; d++) { a.tb[d] = T_begin16[4 * d + 3]; a.dt[d] = T_end16[4 * d + 3] - T_begin16[4 * d + 3]; }
    a.t0 = t0; a.span = t1 - t0;
    a.partials = partials; a.ticket = ticket; a.out = out; a.matches = matches;
    PCR_HIP_CHECK(ctx, hipMemsetAsync(ticket, 0, 16, ctx->stream));
    if (validity) PCR_LAUNCH(ctx, k_pmap_lin_ct<true>, dim3(nb), dim3(CT_BS), 0, ctx->stream, a);
    else PCR_LAUNCH(ctx, k_pmap_lin_ct<false>, dim3(nb), dim3(CT_BS), 0, ctx->stream, a);
    double h[CT_OUT];
    PCR_HIP_CHECK(ctx, hipMemcpyAsync(h, out, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
    PCR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    if (H144) memcpy(H144, h, sizeof(double) * 144);
    if (g12) memcpy(g12, h + 144, sizeof(double) * 12);
    if (rows) *rows = (int64_t)(h[156] + 0.5);
    if (sum_d2) *sum_d2 = h[157];
    if (sum_r2) *sum_r2 = h[158];
    return PCR_OK;
    });
}
