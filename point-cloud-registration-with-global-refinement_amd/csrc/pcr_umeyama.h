// pcr_umeyama.h -- what the point-to-point ICP update (pcr_gicp.hip) and the RANSAC hypothesis kernel (pcr_ransac.hip) share: the float64
// Umeyama fit from moments, and the counter-based sampler of the FGR tuple test (pcr_fgr.hip) that RANSAC draws its samples with.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

__host__ __device__ static inline uint64_t pcr_splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// Eigen::umeyama(source, target, with_scaling) (Eigen >= 3.3, what TransformationEstimationPointToPoint returns) from the float64 moments of the
// n pairs (icp_point, P2P modes): M[0..2] = sum u, M[3..5] = sum v, M[6..14] = sum v u^T (row-major), M[15] = sum |u|^2, u = q - os, v = t - o
// (os = o unless the caller took the source's moments about an origin of its own: a source far from the target would otherwise leave var(u)
// and sigma as small differences of large sums).
// sigma = cov(v, u); R = the rotation that maximises tr(R^T sigma), i.e. Umeyama's U S V^T with the reflection fixed, found as Horn's unit
// quaternion: the eigenvector of the largest eigenvalue of the symmetric 4x4 N(sigma), by cyclic Jacobi in float64 with static indexing only
// (registers); for sigma of rank >= 2 the same R.  c = tr(R^T sigma) / var(u) = tr(D S) / var(u) (1 without scaling), t = mean t - c R mean q.
__host__ __device__ static inline void icp_umeyama(const double *M, double n, const double *o, bool scaling, double *U, const double *os = nullptr) {
    const double inv = 1.0 / n;
    const double mu[3] = {M[0] * inv, M[1] * inv, M[2] * inv}, mv[3] = {M[3] * inv, M[4] * inv, M[5] * inv};
    double sg[3][3];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) sg[r][c] = M[6 + 3 * r + c] * inv - mv[r] * mu[c];
    const double var = M[15] * inv - (mu[0] * mu[0] + mu[1] * mu[1] + mu[2] * mu[2]);
    // Horn's S_ab = sum u_a v_b = sigma[b][a]
    const double Sxx = sg[0][0], Sxy = sg[1][0], Sxz = sg[2][0], Syx = sg[0][1], Syy = sg[1][1], Syz = sg[2][1], Szx = sg[0][2], Szy = sg[1][2], Szz = sg[2][2];
    double a[4][4] = {{Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx},
                      {Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz},
                      {Szx - Sxz, Sxy + Syx, Syy - Sxx - Szz, Syz + Szy},
                      {Sxy - Syx, Szx + Sxz, Syz + Szy, Szz - Sxx - Syy}};
    double v[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
    for (int sweep = 0; sweep < 16; sweep++) {
        double off = 0, tot = 0;
#pragma unroll
        for (int p = 0; p < 4; p++) {
            tot += a[p][p] * a[p][p];
#pragma unroll
            for (int q = p + 1; q < 4; q++) off += a[p][q] * a[p][q];
        }
        if (!(off > 1e-36 * tot)) break;
#pragma unroll
        for (int pq = 0; pq < 6; pq++) {
            const int p = pq < 3 ? 0 : (pq < 5 ? 1 : 2), q = pq < 3 ? pq + 1 : (pq < 5 ? pq - 1 : 3);
            const double apq = a[p][q];
            if (apq != 0.0) {
                const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
#pragma unroll
                for (int k = 0; k < 4; k++) { const double akp = a[k][p], akq = a[k][q]; a[k][p] = c * akp - sn * akq; a[k][q] = sn * akp + c * akq; }
#pragma unroll
                for (int k = 0; k < 4; k++) { const double apk = a[p][k], aqk = a[q][k]; a[p][k] = c * apk - sn * aqk; a[q][k] = sn * apk + c * aqk; }
#pragma unroll
                for (int k = 0; k < 4; k++) { const double vkp = v[k][p], vkq = v[k][q]; v[k][p] = c * vkp - sn * vkq; v[k][q] = sn * vkp + c * vkq; }
            }
        }
    }
    double lmax = a[0][0], w = v[0][0], x = v[1][0], y = v[2][0], z = v[3][0];      // largest eigenvalue (ties: the lower column)
#pragma unroll
    for (int k = 1; k < 4; k++)
        if (a[k][k] > lmax) { lmax = a[k][k]; w = v[0][k]; x = v[1][k]; y = v[2][k]; z = v[3][k]; }
    const double qn = 1.0 / sqrt(w * w + x * x + y * y + z * z);
    w *= qn; x *= qn; y *= qn; z *= qn;
    const double R[3][3] = {{w * w + x * x - y * y - z * z, 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)},
                            {2.0 * (x * y + w * z), w * w - x * x + y * y - z * z, 2.0 * (y * z - w * x)},
                            {2.0 * (x * z - w * y), 2.0 * (y * z + w * x), w * w - x * x - y * y + z * z}};
    double c = 1.0;
    if (scaling) {
        double tr = 0;
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int k = 0; k < 3; k++) tr += R[r][k] * sg[r][k];
        c = tr / var;
    }
    if (!os) os = o;
    const double ms[3] = {mu[0] + os[0], mu[1] + os[1], mu[2] + os[2]}, md[3] = {mv[0] + o[0], mv[1] + o[1], mv[2] + o[2]};
#pragma unroll
    for (int r = 0; r < 3; r++) {
        U[r * 4 + 0] = c * R[r][0]; U[r * 4 + 1] = c * R[r][1]; U[r * 4 + 2] = c * R[r][2];
        U[r * 4 + 3] = md[r] - c * (R[r][0] * ms[0] + R[r][1] * ms[1] + R[r][2] * ms[2]);
    }
    U[12] = 0; U[13] = 0; U[14] = 0; U[15] = 1;
}
