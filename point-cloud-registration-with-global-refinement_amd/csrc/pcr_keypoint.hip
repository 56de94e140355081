// pcr_keypoint.hip -- ISS keypoint detection (Intrinsic Shape Signatures, Zhong 2009) on gfx950.
// Reference behaviour: Open3D geometry::keypoint::ComputeISSKeypoints (cpp/open3d/geometry/Keypoint.cpp); the reference scripts do not
// call it, Open3D users put it in front of a global registration so that the feature search runs over a few percent of the points.
// The rules (radius membership, the suppression guard G, the default radii) are stated next to the entry point in include/pcr_hip.h.
// Both kernels are fixed-radius walks of the Morton-sorted octree (oct_group_frame / oct_ball_walk, pcr_octree.h).
#include <cmath>
#include "pcr_octree.h"

#define ISS_BS 256
#define ISS_G_FACTOR 1e-11          // suppression guard G = ISS_G_FACTOR x salient_radius^2 (include/pcr_hip.h)

// ============================================================================================ eigenvalues of a symmetric 3x3
// The eigenvalue part of d_fast_eigen3x3 (pcr_eigen3.h;Eberly's non-iterative solver): the matrix scaled by its largest entry, the
// trigonometric closed form of the characteristic cubic, and -- as that solver does for its eigenvectors -- a deflation by the eigenvector
// of the well-separated root.  The closed form alone gives the two roots next to each other (l2 and l3 of a line-like neighbourhood, where
// acos works at 1 - 1e-10) only to 1e-11 of the largest; the eigenvalues of the 2x2 block in the complement of the separated eigenvector
// are good to eps times the largest.  A coordinate axis that decouples exactly (the other two entries of its row are zero: points that
// share one coordinate) is taken out first, so that a flat neighbourhood gives the eigenvalue 0 and not rounding noise of either sign.
// C6 = (xx, xy, xz, yy, yz, zz); ev ascending.  false (and ev = 0): no positive entry, the all-zero covariance of coincident points.
// All in float64, the transcendental calls included.
__device__ static inline void iss_sort3_block(double lone, double a, double b, double d, double *e) {       // lone, and the eigenvalues of [a b; b d]
    const double h = (a + d) * 0.5, k = (a - d) * 0.5, g = sqrt(k * k + b * b);
    const double lo = h - g, hi = h + g;
    e[0] = fmin(lone, lo); e[2] = fmax(lone, hi);
    e[1] = fmax(fmin(lone, hi), lo);
}
__device__ static inline bool iss_eigenvalues3(const double *C6, double *ev) {
    double mc = C6[0];
#pragma unroll
    for (int k = 1; k < 6; k++) mc = fmax(mc, C6[k]);
    ev[0] = ev[1] = ev[2] = 0.0;
    if (!(mc > 0.0)) return false;
    double A[6], e[3];
#pragma unroll
    for (int k = 0; k < 6; k++) A[k] = C6[k] / mc;
    if (A[1] == 0.0 && A[2] == 0.0) iss_sort3_block(A[0], A[3], A[4], A[5], e);
    else if (A[1] == 0.0 && A[4] == 0.0) iss_sort3_block(A[3], A[0], A[2], A[5], e);
    else if (A[2] == 0.0 && A[4] == 0.0) iss_sort3_block(A[5], A[0], A[1], A[3], e);
    else {
        const double norm = A[1] * A[1] + A[2] * A[2] + A[4] * A[4];
        const double q = (A[0] + A[3] + A[5]) / 3.0;
        const double b00 = A[0] - q, b11 = A[3] - q, b22 = A[5] - q;
        const double p = sqrt((b00 * b00 + b11 * b11 + b22 * b22 + norm * 2.0) / 6.0);
        const double c00 = b11 * b22 - A[4] * A[4], c01 = A[1] * b22 - A[4] * A[2], c02 = A[1] * A[4] - b11 * A[2];
        const double det = (b00 * c00 - A[1] * c01 + A[2] * c02) / (p * p * p);
        double hd = det * 0.5; hd = fmin(fmax(hd, -1.0), 1.0);
        const double angle = acos(hd) / 3.0;
        const double two_thirds_pi = 2.09439510239319549;
        const double beta2 = cos(angle) * 2.0, beta0 = cos(angle + two_thirds_pi) * 2.0, beta1 = -(beta0 + beta2);
        e[0] = q + p * beta0; e[1] = q + p * beta1; e[2] = q + p * beta2;
        // the separated root (the largest when hd >= 0, else the smallest) and its eigenvector: the largest cross product of two rows of A - iso I
        const double iso = hd >= 0 ? e[2] : e[0];
        const double r0x = A[0] - iso, r1y = A[3] - iso, r2z = A[5] - iso;
        const double ax = A[1] * A[4] - A[2] * r1y, ay = A[2] * A[1] - r0x * A[4], az = r0x * r1y - A[1] * A[1];           // r0 x r1
        const double bx = A[1] * r2z - A[2] * A[4], by = A[2] * A[2] - r0x * r2z, bz = r0x * A[4] - A[1] * A[2];           // r0 x r2
        const double cx = r1y * r2z - A[4] * A[4], cy = A[4] * A[2] - A[1] * r2z, cz = A[1] * A[4] - r1y * A[2];           // r1 x r2
        const double da = ax * ax + ay * ay + az * az, db = bx * bx + by * by + bz * bz, dc = cx * cx + cy * cy + cz * cz;
        double vx = ax, vy = ay, vz = az, dm = da;
        if (db > dm) { vx = bx; vy = by; vz = bz; dm = db; }
        if (dc > dm) { vx = cx; vy = cy; vz = cz; dm = dc; }
        if (dm > 0.0) {
            const double is = 1.0 / sqrt(dm);
            vx *= is; vy *= is; vz *= is;
            double ux, uy, uz;                                 // U, W = v x U: an orthonormal basis of the complement
            if (fabs(vx) > fabs(vy)) { const double inv = 1.0 / sqrt(vx * vx + vz * vz); ux = -vz * inv; uy = 0.0; uz = vx * inv; }
            else { const double inv = 1.0 / sqrt(vy * vy + vz * vz); ux = 0.0; uy = vz * inv; uz = -vy * inv; }
            const double wx = vy * uz - vz * uy, wy = vz * ux - vx * uz, wz = vx * uy - vy * ux;
            const double aux = A[0] * ux + A[1] * uy + A[2] * uz, auy = A[1] * ux + A[3] * uy + A[4] * uz, auz = A[2] * ux + A[4] * uy + A[5] * uz;
            const double awx = A[0] * wx + A[1] * wy + A[2] * wz, awy = A[1] * wx + A[3] * wy + A[4] * wz, awz = A[2] * wx + A[4] * wy + A[5] * wz;
            iss_sort3_block(iso, ux * aux + uy * auy + uz * auz, ux * awx + uy * awy + uz * awz, wx * awx + wy * awy + wz * awz, e);
        }
    }
    ev[0] = e[0] * mc; ev[1] = e[1] * mc; ev[2] = e[2] * mc;
    return true;
}

// ======================================================================================================== saliency
// The fixed-radius walk at salient_radius, every query to its end (the point itself a member).  The moments are those of (p - q), the
// offset from the QUERY: the covariance does not depend on the origin, the terms are at most r^2 instead of the squares of coordinates
// hundreds of metres from the origin (SURVEY.md hard part 3), and a neighbourhood of coincident points gives exactly zero.  saliency = the smallest eigenvalue when l2 / l1 < gamma_21 and l3 / l2 < gamma_32, else 0;
// 0 too with fewer than min_neighbors members or an all-zero covariance.
struct IssSalArgs {
    OctView t; const uint32_t *perm; float r2f; double r2; double gamma_21, gamma_32; int min_neighbors;
    double *sal_sorted;                       // n, Morton order: what k_iss_nonmax reads next to pts
    double *sal_caller, *eig_caller;          // optional caller rows: saliency (n), eigenvalues descending (n x 3)
};
__global__ void __launch_bounds__(ISS_BS) k_iss_saliency(IssSalArgs a) {
    oct_group_frame<ISS_BS>(a.t, [&](const OctGroupQuery &g) {
    const int qi = g.qi, ol = g.ol; const bool live = g.live; const float4 q = g.q;
    double cu[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    int cnt = 0;
    // active = live: every query walks to its end
    oct_ball_walk(a.t, g, a.r2f, [&]() { return live; }, [&](int idx) {
        const float4 p = a.t.pts[idx];
        if (oct_ball_member<false>(q, p, a.r2f, a.r2)) {
            const double dx = (double)p.x - (double)q.x, dy = (double)p.y - (double)q.y, dz = (double)p.z - (double)q.z;
            cu[0] += dx; cu[1] += dy; cu[2] += dz;
            cu[3] += dx * dx; cu[4] += dx * dy; cu[5] += dx * dz; cu[6] += dy * dy; cu[7] += dy * dz; cu[8] += dz * dz;
            cnt++;
        }
    });
#pragma unroll
    for (int t = 0; t < 9; t++) cu[t] = pcr_octet_sum(cu[t]);
    cnt = pcr_octet_sum_i(cnt);
    if (live && ol == 0) {
        double ev[3] = {0.0, 0.0, 0.0}, sal = 0.0;
        if (cnt >= a.min_neighbors) {
            const double c = (double)cnt;
#pragma unroll
            for (int t = 0; t < 9; t++) cu[t] = cu[t] / c;
            double C6[6];
            C6[0] = cu[3] - cu[0] * cu[0]; C6[1] = cu[4] - cu[0] * cu[1]; C6[2] = cu[5] - cu[0] * cu[2];
            C6[3] = cu[6] - cu[1] * cu[1]; C6[4] = cu[7] - cu[1] * cu[2]; C6[5] = cu[8] - cu[2] * cu[2];
            if (iss_eigenvalues3(C6, ev) && ev[1] / ev[2] < a.gamma_21 && ev[0] / ev[1] < a.gamma_32) sal = ev[0];
        }
        a.sal_sorted[qi] = sal;
        const size_t row = a.perm[qi];
        if (a.sal_caller) a.sal_caller[row] = sal;
        if (a.eig_caller) { a.eig_caller[row * 3] = ev[2]; a.eig_caller[row * 3 + 1] = ev[1]; a.eig_caller[row * 3 + 2] = ev[0]; }
    }
    });
}

// ============================================================================================= non-maximum suppression
// The fixed-radius walk at non_max_radius for the queries with saliency > 0 (a wavefront without one does not walk): count the members,
// and look for one that suppresses the query, s_j > s_i + G.  A query that is suppressed is finished.  The walk opens the nearest cells
// first, so most queries meet a stronger neighbour in their own leaf.  keypoint = saliency > 0, at least min_neighbors members, no
// suppressor; the flag goes to the caller's row of the mask.
struct IssNmsArgs { OctView t; const uint32_t *perm; float r2f; double r2; const double *sal_sorted; double guard; int min_neighbors; uint8_t *keep; };
__global__ void __launch_bounds__(ISS_BS) k_iss_nonmax(IssNmsArgs a) {
    oct_group_frame<ISS_BS>(a.t, [&](const OctGroupQuery &g) {
    const double s = g.live ? a.sal_sorted[g.qi] : 0.0;
    const bool cand = g.live && s > 0.0;                      // octet-uniform
    const double bar = s + a.guard;
    int cnt = 0, hit = 0, total = 0, beaten = 0;              // this lane's count and find; the octet's count and verdict (octet-uniform, refreshed after every range)
    if (__ballot(cand) != 0ull) {
        // active until a suppressor is found: beaten changes in the per-range step only, as active() must
        oct_ball_walk(a.t, g, a.r2f, [&]() { return cand && !beaten; },
                      [&](int idx) { if (oct_ball_member<false>(g.q, a.t.pts[idx], a.r2f, a.r2)) { cnt++; hit |= a.sal_sorted[idx] > bar ? 1 : 0; } },
                      [&]() { total = pcr_octet_sum_i(cnt); beaten = pcr_octet_sum_i(hit) != 0 ? 1 : 0; });
    }
    if (g.live && g.ol == 0) a.keep[a.perm[g.qi]] = (cand && !beaten && total >= a.min_neighbors) ? 1 : 0;
    });
}

// ============================================================================================ default radii (resolution)
// Sum of n float64 values with a fixed tree: wavefront reduction, one slab per workgroup, one launch that adds the slabs in their order
// (the scheme of k_moments_partial / k_moments_final, pcr_query.hip).  The grid depends on n alone: two runs give the same bits.
#define ISS_SUM_MAX_BLOCKS 256
__global__ void __launch_bounds__(ISS_BS) k_iss_sum_partial(const double *__restrict__ v, int n, double *__restrict__ slabs) {
    double s = 0.0;
    for (int i = blockIdx.x * ISS_BS + threadIdx.x; i < n; i += (int)gridDim.x * ISS_BS) s += v[i];
    __shared__ double w[ISS_BS / PCR_WAVE];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const double r = pcr_wave_sum(s);
    if (lane == 0) w[wv] = r;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = w[0];
        for (int k = 1; k < ISS_BS / PCR_WAVE; k++) t += w[k];
        slabs[blockIdx.x] = t;
    }
}
__global__ void k_iss_sum_final(const double *__restrict__ slabs, int nb, double *__restrict__ out) {
    if (threadIdx.x == 0) {
        double t = slabs[0];
        for (int k = 1; k < nb; k++) t += slabs[k];
        *out = t;
    }
}

// resolution = the mean over all points of the distance to the nearest other point (0 for a point without one), on the host; one synchronisation
static int iss_resolution(pcr_context *ctx, const DevCloud *c, const uint32_t *perm, int64_t n, double *resolution) {
    ArenaMark mark(ctx);
    const int nb = (int)((n + ISS_BS - 1) / ISS_BS < ISS_SUM_MAX_BLOCKS ? (n + ISS_BS - 1) / ISS_BS : ISS_SUM_MAX_BLOCKS);
    double *dist = arena<double>(ctx, n), *slabs = arena<double>(ctx, nb), *out = arena<double>(ctx, 1);
    if (!dist || !slabs || !out) return PCR_ENOMEM;
    PCR_TRY(pcr_dev_nn_distance(ctx, c, perm, dist));
    PCR_LAUNCH(ctx, k_iss_sum_partial, dim3(nb), dim3(ISS_BS), 0, ctx->stream, (const double *)dist, (int)n, slabs);
    PCR_LAUNCH(ctx, k_iss_sum_final, dim3(1), dim3(64), 0, ctx->stream, (const double *)slabs, nb, out);
    double sum = 0.0;
    PCR_HIP_CHECK(ctx, hipMemcpyAsync(&sum, out, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    PCR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    *resolution = sum / (double)n;
    return PCR_OK;
}

// ====================================================================================================== C ABI
extern "C" int pcr_iss_keypoints(pcr_context *ctx, const float *xyz, int64_t n, double salient_radius, double non_max_radius,
                                 double gamma_21, double gamma_32, int min_neighbors,
                                 uint8_t *keep_mask, float *out_xyz, int64_t *out_index, int64_t *out_n,
                                 double *saliency, double *eigenvalues3, double *radii_used2) {
    return pcr_api_call(ctx, [&]() -> int {
    if (n < 0 || n > 0x7fffffffLL / 4 || (n > 0 && !xyz)) { ctx->err = "iss_keypoints: bad cloud pointer or size"; return PCR_EINVAL; }
    if (!(salient_radius >= 0.0) || !(non_max_radius >= 0.0) || !std::isfinite(salient_radius) || !std::isfinite(non_max_radius)) {
        ctx->err = "iss_keypoints: salient_radius and non_max_radius must be finite and >= 0"; return PCR_EINVAL;
    }
    if (min_neighbors < 1) { ctx->err = "iss_keypoints: min_neighbors < 1"; return PCR_EINVAL; }
    if (!std::isfinite(gamma_21) || !std::isfinite(gamma_32)) { ctx->err = "iss_keypoints: gamma_21 and gamma_32 must be finite"; return PCR_EINVAL; }
    if (out_n) *out_n = 0;
    if (radii_used2) { radii_used2[0] = salient_radius; radii_used2[1] = non_max_radius; }
    if (n == 0) return PCR_OK;
    PCR_TRY(pcr_arena_reserve(ctx, pcr_scratch_bytes_for(n) + (size_t)n * 64));
    DevCloud c; uint32_t *perm = nullptr;
    PCR_TRY(pcr_import_cloud(ctx, xyz, nullptr, n, &c, &perm, false));       // once per call, whichever radii are given
    if (salient_radius == 0.0 || non_max_radius == 0.0) {                    // Open3D: BOTH are replaced when either is 0
        double resolution = 0.0;
        PCR_TRY(iss_resolution(ctx, &c, perm, n, &resolution));
        salient_radius = 6.0 * resolution; non_max_radius = 4.0 * resolution;
        if (radii_used2) { radii_used2[0] = salient_radius; radii_used2[1] = non_max_radius; }
    }
    double *sal_sorted = arena<double>(ctx, n);
    uint8_t *keep_caller = keep_mask ? keep_mask : arena<uint8_t>(ctx, n);
    if (!sal_sorted || !keep_caller) return PCR_ENOMEM;
    const dim3 grid((unsigned)(((size_t)c.cap * OCT + ISS_BS - 1) / ISS_BS));
    IssSalArgs sa; sa.t = oct_view(&c); sa.perm = perm; sa.r2 = salient_radius * salient_radius; sa.r2f = pcr_wide_r2f(sa.r2);
    sa.gamma_21 = gamma_21; sa.gamma_32 = gamma_32; sa.min_neighbors = min_neighbors; sa.sal_sorted = sal_sorted; sa.sal_caller = saliency; sa.eig_caller = eigenvalues3;
    PCR_LAUNCH(ctx, k_iss_saliency, grid, dim3(ISS_BS), 0, ctx->stream, sa);
    IssNmsArgs na; na.t = sa.t; na.perm = perm; na.r2 = non_max_radius * non_max_radius; na.r2f = pcr_wide_r2f(na.r2);
    na.sal_sorted = sal_sorted; na.guard = ISS_G_FACTOR * sa.r2; na.min_neighbors = min_neighbors; na.keep = keep_caller;
    PCR_LAUNCH(ctx, k_iss_nonmax, grid, dim3(ISS_BS), 0, ctx->stream, na);
    return pcr_emit_kept_rows(ctx, xyz, n, keep_caller, out_xyz, out_index, out_n);      // the keypoints in CALLER order, ascending
    });
}
