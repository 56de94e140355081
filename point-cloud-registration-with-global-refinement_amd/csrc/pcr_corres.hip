// pcr_corres.hip -- one-shot fits over a correspondence list the caller holds (include/pcr_hip.h: pcr_estimation_compute_transformation,
// pcr_estimation_compute_rmse, pcr_correspondences_from_features): compute_transformation / compute_rmse of the three ICP estimators and the
// feature matcher of the global registrations as a call of its own.
//
// The ICP loop (pcr_gicp.hip, k_icp_iter<MODE>) reads one target index per SOURCE ROW from its match array and applies the radius test; a free
// list holds any rows in any order, repeats source indices and is shorter or longer than the source cloud, so the reduction over it is a kernel
// of its own:
//   k_corr_check        flags rows out of range; the host reads the count before any row is read through the list
//   k_corr_rows<MODE>   one lane per row, grid-stride; gathers the two points (and the target normal / the two covariance sextets), accumulates
//                       the row's sums in registers, reduces them in the workgroup in a fixed order (DPP inside the 16-lane rows, then the 16
//                       rows in order: the reduction of icp_finish) and writes ONE partial row per workgroup
//   k_corr_fit<MODE>    one wavefront: adds the partial rows in ascending order and does the fit (icp_umeyama, pcr_umeyama.h) or the 6x6 solve
//                       (pcr_solve6.h: the LDLT of the loop with its pivoted fall-back) and the Rz Ry Rx pose
// No workgroup waits for another: no ticket, no barrier across workgroups, no spin; every loop is bounded by a count.  The fits are single
// calls, and the kernel boundary between the two launches is all the ordering they need.
// The row arithmetic restates icp_point<MODE> (pcr_gicp.hip) at T = identity; the hot kernels' source is not shared.
#include <climits>
#include <cmath>
#include <cstring>
#include "pcr_device.h"
#include "pcr_umeyama.h"
#include "pcr_solve6.h"

enum { CORR_P2P = 0, CORR_P2PL = 1, CORR_GICP = 2, CORR_GICP_COV = 3, CORR_RMSE_POINT = 4, CORR_RMSE_PLANE = 5 };
#define CORR_BS 256              // rows per workgroup and grid step (the tile)
#define CORR_MAX_BLOCKS 256      // partial rows at most: lists beyond CORR_BS * CORR_MAX_BLOCKS rows go round the grid again
#define CORR_NVP 32              // doubles per partial row
// sums per row: 16 moments (icp_umeyama's M) for point-to-point; 21 (JTJ, upper triangle) + 6 (JTr) + 1 (sum r^2) for the 6x6 forms; 1 for an RMSE
template <int MODE> struct CorrNV { static constexpr int value = MODE == CORR_P2P ? 16 : (MODE >= CORR_RMSE_POINT ? 1 : 28); };

struct CorrArgs {
    const float *src, *tgt;                  // packed float32 xyz rows, caller order
    const float *src_nrm, *tgt_nrm;          // packed normals (P2PL: target; GICP: both)
    const float *src_cov6, *tgt_cov6;        // GICP_COV
    const int32_t *corres; int C;
    int loss; double loss_k, a;              // a = 1 - epsilon (GICP)
    double *partials;                        // [workgroups][CORR_NVP]
};

__global__ void __launch_bounds__(CORR_BS) k_corr_check(const int32_t *__restrict__ corres, int C, int n_src, int n_tgt, int *__restrict__ bad) {
    int cnt = 0;
    for (int c = blockIdx.x * CORR_BS + threadIdx.x; c < C; c += gridDim.x * CORR_BS) {
        const int i = corres[2 * (size_t)c], j = corres[2 * (size_t)c + 1];
        if ((unsigned)i >= (unsigned)n_src || (unsigned)j >= (unsigned)n_tgt) cnt++;
    }
    if (cnt) atomicAdd(bad, cnt);
}

__device__ static inline void corr_row6(double w, const double *J, double r, double *acc) {
    int t = 0;
#pragma unroll
    for (int p = 0; p < 6; p++) {
        const double wj = w * J[p];
#pragma unroll
        for (int q = p; q < 6; q++) acc[t++] += wj * J[q];
        acc[21 + p] += wj * r;
    }
}

// the sums of row c (icp_point<MODE> at T = identity, without the radius test)
template <int MODE>
__device__ static inline void corr_row(const CorrArgs &a, int c, const double *o, double *acc) {
    const int i = a.corres[2 * (size_t)c], j = a.corres[2 * (size_t)c + 1];
    const float *sp = a.src + (size_t)i * 3, *tp = a.tgt + (size_t)j * 3;
    const double qx = sp[0], qy = sp[1], qz = sp[2], tx = tp[0], ty = tp[1], tz = tp[2];
    const double dx = qx - tx, dy = qy - ty, dz = qz - tz;
    if (MODE == CORR_RMSE_POINT) {
        acc[0] += dx * dx + dy * dy + dz * dz;
    } else if (MODE == CORR_P2P) {
        // u = s - os about the source point of row 0, v = t - o about its target point (each cloud about a point of its own: the list may pair
        // clouds that lie far apart): [0..2] sum u, [3..5] sum v, [6..14] sum v u^T, [15] sum |u|^2
        const double ux = qx - o[3], uy = qy - o[4], uz = qz - o[5], vx = tx - o[0], vy = ty - o[1], vz = tz - o[2];
        acc[0] += ux; acc[1] += uy; acc[2] += uz;
        acc[3] += vx; acc[4] += vy; acc[5] += vz;
        acc[6] += vx * ux; acc[7] += vx * uy; acc[8] += vx * uz;
        acc[9] += vy * ux; acc[10] += vy * uy; acc[11] += vy * uz;
        acc[12] += vz * ux; acc[13] += vz * uy; acc[14] += vz * uz;
        acc[15] += ux * ux + uy * uy + uz * uz;
    } else if (MODE == CORR_P2PL || MODE == CORR_RMSE_PLANE) {
        // r = (s - t).n, J = [s x n, n] with the target normal AS STORED
        const float *np_ = a.tgt_nrm + (size_t)j * 3;
        const double nx = np_[0], ny = np_[1], nz = np_[2];
        const double r = nx * dx + ny * dy + nz * dz;
        if (MODE == CORR_RMSE_PLANE) {
            acc[0] += r * r;
        } else {
            const double J[6] = {qy * nz - qz * ny, qz * nx - qx * nz, qx * ny - qy * nx, nx, ny, nz};
            corr_row6(icp_weight(a.loss, a.loss_k, r), J, r, acc);
            acc[27] += r * r;
        }
    } else {
        double W[9];
        if (MODE == CORR_GICP_COV) {
            // the given covariances untouched: M = Cs + Ct, W = M^(-1/2)
            const float *cs = a.src_cov6 + (size_t)i * 6, *ct = a.tgt_cov6 + (size_t)j * 6;
            const double M6[6] = {(double)cs[0] + ct[0], (double)cs[1] + ct[1], (double)cs[2] + ct[2], (double)cs[3] + ct[3], (double)cs[4] + ct[4], (double)cs[5] + ct[5]};
            icp_sym3_inv_sqrt(M6, W);
        } else {
            // covariances from normals: C = I - a m m^T, m the normalised normal, e1 when n.x < -0.99 (Open3D GetRotationFromE1ToX)
            const float *sn = a.src_nrm + (size_t)i * 3, *tn = a.tgt_nrm + (size_t)j * 3;
            double ux = sn[0], uy = sn[1], uz = sn[2], vx = tn[0], vy = tn[1], vz = tn[2];
            if (ux < -0.99) { ux = 1; uy = 0; uz = 0; }
            if (vx < -0.99) { vx = 1; vy = 0; vz = 0; }
            double inv = 1.0 / sqrt(ux * ux + uy * uy + uz * uz);
            ux *= inv; uy *= inv; uz *= inv;
            inv = 1.0 / sqrt(vx * vx + vy * vy + vz * vz);
            vx *= inv; vy *= inv; vz *= inv;
            const double cs = ux * vx + uy * vy + uz * vz;
            // M = 2I - a(uu^T + vv^T): eigenpairs (2 - a(1+c), u+v), (2 - a(1-c), u-v), (2, u x v)
            const double SQ2 = 1.4142135623730951;
            const double lp = 2.0 - a.a * (1.0 + cs), lm = 2.0 - a.a * (1.0 - cs);
            const double slp = sqrt(lp), slm = sqrt(lm);
            const double gp = a.a / (2.0 * SQ2 * slp * (SQ2 + slp)), gm = a.a / (2.0 * SQ2 * slm * (SQ2 + slm));
            const double ex = ux + vx, ey = uy + vy, ez = uz + vz, fx = ux - vx, fy = uy - vy, fz = uz - vz;
            const double w0 = 1.0 / SQ2;
            W[0] = w0 + gp * ex * ex + gm * fx * fx; W[1] = gp * ex * ey + gm * fx * fy; W[2] = gp * ex * ez + gm * fx * fz;
            W[4] = w0 + gp * ey * ey + gm * fy * fy; W[5] = gp * ey * ez + gm * fy * fz; W[8] = w0 + gp * ez * ez + gm * fz * fz;
            W[3] = W[1]; W[6] = W[2]; W[7] = W[5];
        }
        double r2 = 0;
#pragma unroll
        for (int row = 0; row < 3; row++) {
            const double wx = W[row * 3], wy = W[row * 3 + 1], wz = W[row * 3 + 2];
            const double J[6] = {qy * wz - qz * wy, qz * wx - qx * wz, qx * wy - qy * wx, wx, wy, wz};      // s x W_row, W_row
            const double r = wx * dx + wy * dy + wz * dz;
            corr_row6(icp_weight(a.loss, a.loss_k, r), J, r, acc);
            r2 += r * r;
        }
        acc[27] += r2;
    }
}

template <int MODE>
__global__ void __launch_bounds__(CORR_BS) k_corr_rows(CorrArgs a) {
    constexpr int NV = CorrNV<MODE>::value;
    __shared__ double red[CORR_BS / 16][CORR_NVP];          // one row per 16-lane DPP row
    double o[6] = {0, 0, 0, 0, 0, 0};            // the origins of the moments: the target point of row 0, then its source point
    if (MODE == CORR_P2P) {
        const float *t0 = a.tgt + (size_t)a.corres[1] * 3, *s0 = a.src + (size_t)a.corres[0] * 3;
        o[0] = t0[0]; o[1] = t0[1]; o[2] = t0[2]; o[3] = s0[0]; o[4] = s0[1]; o[5] = s0[2];
    }
    double acc[NV];
#pragma unroll
    for (int k = 0; k < NV; k++) acc[k] = 0.0;
    for (int c = blockIdx.x * CORR_BS + threadIdx.x; c < a.C; c += gridDim.x * CORR_BS) corr_row<MODE>(a, c, o, acc);
    // every lane of the workgroup is here (lanes past the end of the list hold zeros): DPP butterfly inside every 16-lane row, then the rows in order
    const int lane = threadIdx.x & 63, r = lane & 15, row = threadIdx.x >> 4;
    if constexpr (NV == 1) {
        const double s = pcr_row16_sum(acc[0]);
        if (r == 0) red[row][0] = s;
    } else {
        double lo, hi;
        pcr_row16_sum_halving<NV>(acc, lane, &lo, &hi);
        red[row][r] = lo;
        if (16 + r < NV) red[row][16 + r] = hi;
    }
    __syncthreads();
    if ((int)threadIdx.x < NV) {
        double s = red[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < CORR_BS / 16; w++) s += red[w][threadIdx.x];
        a.partials[(size_t)blockIdx.x * CORR_NVP + threadIdx.x] = s;
    }
}

// out: [0..15] the pose, [16] the sum of an RMSE mode, [17] 1 when a fit was made (0: the identity stands in for a system without solution)
template <int MODE>
__global__ void __launch_bounds__(64) k_corr_fit(CorrArgs a, int nb, int with_scaling, double *__restrict__ out) {
    constexpr int NV = CorrNV<MODE>::value;
    __shared__ double S[CORR_NVP], ldl_w[96], rhs[6], sol[8];
    __shared__ int ldl_perm[6];
    if (threadIdx.x < CORR_NVP) {
        double s = 0.0;
        if ((int)threadIdx.x < NV)
            for (int b = 0; b < nb; b++) s += a.partials[(size_t)b * CORR_NVP + threadIdx.x];
        S[threadIdx.x] = s;
    }
    __syncthreads();
    // every lane runs the same scalar work on the same sums; lane 0 writes
    double U[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    double fitted = 0.0;
    if (MODE == CORR_P2P) {
        const float *t0 = a.tgt + (size_t)a.corres[1] * 3, *s0 = a.src + (size_t)a.corres[0] * 3;
        const double org[3] = {t0[0], t0[1], t0[2]}, org_s[3] = {s0[0], s0[1], s0[2]};
        icp_umeyama(S, (double)a.C, org, with_scaling != 0, U, org_s);
        fitted = 1.0;
    } else if (MODE == CORR_P2PL || MODE == CORR_GICP || MODE == CORR_GICP_COV) {
        double nb6[6], x[6];
#pragma unroll
        for (int p = 0; p < 6; p++) nb6[p] = -S[21 + p];
        bool solved = icp_ldlt6_fast(S, nb6, x);
        if (!solved) {                     // indefinite / semi-definite system (uniform: every lane saw the same sums); dynamic indexing stays in LDS
            if (threadIdx.x == 0) {
                for (int p = 0; p < 6; p++) rhs[p] = -S[21 + p];
                sol[6] = icp_ldlt6_pivoted(S, rhs, sol, ldl_w, ldl_perm) ? 1.0 : 0.0;
            }
            __syncthreads();
            solved = sol[6] != 0.0;
#pragma unroll
            for (int p = 0; p < 6; p++) x[p] = sol[p];
        }
        if (solved) {
            const double sa = sin(x[0]), ca = cos(x[0]), sb = sin(x[1]), cb = cos(x[1]), sg = sin(x[2]), cg = cos(x[2]);
            U[0] = cg * cb; U[1] = cg * sb * sa - sg * ca; U[2] = cg * sb * ca + sg * sa; U[3] = x[3];
            U[4] = sg * cb; U[5] = sg * sb * sa + cg * ca; U[6] = sg * sb * ca - cg * sa; U[7] = x[4];
            U[8] = -sb;     U[9] = cb * sa;                U[10] = cb * ca;               U[11] = x[5];
            fitted = 1.0;
        }
    }
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 16; k++) out[k] = U[k];
        out[16] = S[0];
        out[17] = fitted;
    }
}

// ---- host
static int corr_blocks(int64_t C) {
    const int64_t nb = (C + CORR_BS - 1) / CORR_BS;
    return (int)(nb < 1 ? 1 : (nb > CORR_MAX_BLOCKS ? CORR_MAX_BLOCKS : nb));
}
static size_t corr_scratch_bytes() { return (size_t)CORR_MAX_BLOCKS * CORR_NVP * sizeof(double) + 32 * sizeof(double) + 4096; }

// range check of a correspondence list on the device (scratch: one int from the arena the caller has reserved); the count is on the host when it returns
int pcr_corres_check(pcr_context *ctx, const int32_t *corres, int64_t C, int64_t n_src, int64_t n_tgt) {
    if (C <= 0) return PCR_OK;
    ArenaMark mark(ctx);
    int *bad = arena<int>(ctx, 1);
    if (!bad) return PCR_ENOMEM;
    PCR_HIP_CHECK(ctx, hipMemsetAsync(bad, 0, sizeof(int), ctx->stream));
    PCR_LAUNCH(ctx, k_corr_check, dim3(corr_blocks(C)), dim3(CORR_BS), 0, ctx->stream, corres, (int)C, (int)n_src, (int)n_tgt, bad);
    int64_t n_bad = 0;
    PCR_TRY(pcr_read_count(ctx, bad, &n_bad));
    if (n_bad) {
        ctx->err = "correspondence index out of range (" + std::to_string((long long)n_bad) + " of " + std::to_string((long long)C) + " rows; source " +
                   std::to_string((long long)n_src) + ", target " + std::to_string((long long)n_tgt) + " points)";
        return PCR_EINVAL;
    }
    return PCR_OK;
}

template <int MODE>
static int corr_reduce(pcr_context *ctx, const CorrArgs &a, int with_scaling, double *h18) {
    const int nb = corr_blocks(a.C);
    double *out = arena<double>(ctx, 18);
    if (!out) return PCR_ENOMEM;
    PCR_LAUNCH(ctx, k_corr_rows<MODE>, dim3(nb), dim3(CORR_BS), 0, ctx->stream, a);
    PCR_LAUNCH(ctx, k_corr_fit<MODE>, dim3(1), dim3(64), 0, ctx->stream, a, nb, with_scaling, out);
    PCR_HIP_CHECK(ctx, hipMemcpyAsync(h18, out, sizeof(double) * 18, hipMemcpyDeviceToHost, ctx->stream));
    PCR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return PCR_OK;
}

// what both entry points share: argument checks, the range check, the choice of the kernel form.  *mode_out = -1: no launch, the result is the
// identity / 0 (an empty list, a target without normals, clouds without the covariances or normals the GICP rows need)
static int corr_prepare(pcr_context *ctx, const pcr_estimation *e, const float *src_xyz, const float *src_nrm, const float *src_cov6, int64_t n_src,
                        const float *tgt_xyz, const float *tgt_nrm, const float *tgt_cov6, int64_t n_tgt, const int32_t *corres, int64_t C, bool rmse,
                        CorrArgs *a, int *mode_out) {
    *mode_out = -1;
    if (!e) { ctx->err = "missing pcr_estimation"; return PCR_EINVAL; }
    if (e->kind < PCR_EST_POINT_TO_POINT || e->kind > PCR_EST_GENERALIZED_ICP) { ctx->err = "unknown estimator (pcr_estimation_kind)"; return PCR_EINVAL; }
    if (e->kind != PCR_EST_POINT_TO_POINT && (e->loss < PCR_LOSS_L2 || e->loss > PCR_LOSS_GM)) { ctx->err = "unknown robust kernel (pcr_loss_kind)"; return PCR_EINVAL; }
    if (n_src < 0 || n_tgt < 0 || C < 0) { ctx->err = "negative count"; return PCR_EINVAL; }
    if (n_src > INT_MAX / 8 || n_tgt > INT_MAX / 8 || C > INT_MAX / 8) { ctx->err = "cloud or correspondence list too large"; return PCR_EINVAL; }
    if ((n_src > 0 && !src_xyz) || (n_tgt > 0 && !tgt_xyz)) { ctx->err = "missing cloud"; return PCR_EINVAL; }
    if (C == 0) return PCR_OK;
    if (!corres || n_src == 0 || n_tgt == 0) { ctx->err = "correspondences without a list or without points"; return PCR_EINVAL; }
    PCR_TRY(pcr_arena_reserve(ctx, corr_scratch_bytes()));
    PCR_TRY(pcr_corres_check(ctx, corres, C, n_src, n_tgt));
    memset(a, 0, sizeof *a);
    a->src = src_xyz; a->tgt = tgt_xyz; a->src_nrm = src_nrm; a->tgt_nrm = tgt_nrm; a->src_cov6 = src_cov6; a->tgt_cov6 = tgt_cov6;
    a->corres = corres; a->C = (int)C; a->loss = e->loss; a->loss_k = e->loss_k; a->a = 1.0 - e->epsilon;
    a->partials = arena<double>(ctx, (size_t)CORR_MAX_BLOCKS * CORR_NVP);
    if (!a->partials) return PCR_ENOMEM;
    if (e->kind == PCR_EST_POINT_TO_POINT) *mode_out = rmse ? CORR_RMSE_POINT : CORR_P2P;
    else if (e->kind == PCR_EST_POINT_TO_PLANE) *mode_out = !tgt_nrm ? -1 : (rmse ? CORR_RMSE_PLANE : CORR_P2PL);
    else if (rmse) *mode_out = CORR_RMSE_POINT;
    else if (src_cov6 && tgt_cov6) *mode_out = CORR_GICP_COV;
    else if (!src_cov6 && !tgt_cov6 && src_nrm && tgt_nrm) *mode_out = CORR_GICP;
    return PCR_OK;
}

extern "C" int pcr_estimation_compute_transformation(pcr_context *ctx, const pcr_estimation *estimation, const float *src_xyz, const float *src_normals,
                                                     const float *src_cov6, int64_t n_src, const float *tgt_xyz, const float *tgt_normals,
                                                     const float *tgt_cov6, int64_t n_tgt, const int32_t *corres, int64_t n_corres, double *T16) {
    return pcr_api_call(ctx, [&]() -> int {
        if (!T16) return PCR_EINVAL;
        for (int k = 0; k < 16; k++) T16[k] = (k % 5 == 0) ? 1.0 : 0.0;
        CorrArgs a; int mode;
        PCR_TRY(corr_prepare(ctx, estimation, src_xyz, src_normals, src_cov6, n_src, tgt_xyz, tgt_normals, tgt_cov6, n_tgt, corres, n_corres, false, &a, &mode));
        if (mode < 0) return PCR_OK;
        double h[18];
        if (mode == CORR_P2P) PCR_TRY(corr_reduce<CORR_P2P>(ctx, a, estimation->with_scaling, h));
        else if (mode == CORR_P2PL) PCR_TRY(corr_reduce<CORR_P2PL>(ctx, a, 0, h));
        else if (mode == CORR_GICP) PCR_TRY(corr_reduce<CORR_GICP>(ctx, a, 0, h));
        else PCR_TRY(corr_reduce<CORR_GICP_COV>(ctx, a, 0, h));
        memcpy(T16, h, sizeof(double) * 16);
        return PCR_OK;
    });
}

extern "C" int pcr_estimation_compute_rmse(pcr_context *ctx, const pcr_estimation *estimation, const float *src_xyz, const float *src_normals,
                                           const float *src_cov6, int64_t n_src, const float *tgt_xyz, const float *tgt_normals, const float *tgt_cov6,
                                           int64_t n_tgt, const int32_t *corres, int64_t n_corres, double *rmse) {
    return pcr_api_call(ctx, [&]() -> int {
        if (!rmse) return PCR_EINVAL;
        *rmse = 0.0;
        CorrArgs a; int mode;
        PCR_TRY(corr_prepare(ctx, estimation, src_xyz, src_normals, src_cov6, n_src, tgt_xyz, tgt_normals, tgt_cov6, n_tgt, corres, n_corres, true, &a, &mode));
        if (mode < 0) return PCR_OK;
        double h[18];
        if (mode == CORR_RMSE_POINT) PCR_TRY(corr_reduce<CORR_RMSE_POINT>(ctx, a, 0, h));
        else PCR_TRY(corr_reduce<CORR_RMSE_PLANE>(ctx, a, 0, h));
        *rmse = sqrt(h[16] / (double)n_corres);
        return PCR_OK;
    });
}

extern "C" int pcr_correspondences_from_features(pcr_context *ctx, const float *src_feat, int64_t n_src, const float *tgt_feat, int64_t n_tgt, int feature_dim,
                                                 int mutual_filter, double mutual_consistency_ratio, int32_t *corres, int64_t *n_corres) {
    return pcr_api_call(ctx, [&]() -> int {
        if (!n_corres) return PCR_EINVAL;
        *n_corres = 0;
        if (feature_dim != 33) { ctx->err = "correspondences_from_features: the features must be 33-dimensional (FPFH), got " + std::to_string(feature_dim); return PCR_EINVAL; }
        if (n_src < 0 || n_tgt < 0 || n_src > INT_MAX / 8 || n_tgt > INT_MAX / 8) { ctx->err = "correspondences_from_features: feature count out of range"; return PCR_EINVAL; }
        if (!(mutual_consistency_ratio >= 0.0) || !std::isfinite(mutual_consistency_ratio)) { ctx->err = "correspondences_from_features: mutual_consistency_ratio must be finite and >= 0"; return PCR_EINVAL; }
        if (n_src == 0 || n_tgt == 0) return PCR_OK;
        if (!src_feat || !tgt_feat || !corres) { ctx->err = "correspondences_from_features: missing features or output"; return PCR_EINVAL; }
        PCR_TRY(pcr_arena_reserve(ctx, pcr_feature_corres_scratch_bytes(n_src, n_tgt)));
        // Open3D: the mutual rows when there are at least (int)(ratio * n_src) of them, else all rows
        const double need = mutual_consistency_ratio * (double)n_src;
        const int min_rows = need >= (double)INT_MAX ? INT_MAX : (int)need;
        return pcr_feature_corres(ctx, src_feat, (int)n_src, tgt_feat, (int)n_tgt, mutual_filter, min_rows, corres, n_corres);
    });
}
