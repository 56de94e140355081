// pcr_solve6.h -- what the ICP loop (pcr_gicp.hip) and the one-shot fits over a correspondence list (pcr_corres.hip) share on the device: the robust
// kernels' weights, the inverse square root of a symmetric 3x3 and the 6x6 LDL^T solves of the pose update.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/pcr_hip.h"

__host__ __device__ static inline double icp_weight(int loss, double k, double r) {
    if (loss == PCR_LOSS_L1) return 1.0 / fmax(fabs(r), 1e-300);    // Open3D: 1/|r| (unguarded); guard only against r == 0
    if (loss == PCR_LOSS_GM) { const double d = k + r * r; return k / (d * d); }
    return 1.0;
}

// W = (M^-1)^(1/2), symmetric principal root of an SPD 3x3 (general covariances: no closed form): cyclic Jacobi in
// float64, fully unrolled (static indexing only -> registers)
__host__ __device__ static inline void icp_sym3_inv_sqrt(const double *M6 /*xx,xy,xz,yy,yz,zz*/, double *W) {
    double a[3][3] = {{M6[0], M6[1], M6[2]}, {M6[1], M6[3], M6[4]}, {M6[2], M6[4], M6[5]}};
    double v[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
#pragma unroll
    for (int sweep = 0; sweep < 6; sweep++) {
#pragma unroll
        for (int pq = 0; pq < 3; pq++) {
            const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
            const double apq = a[p][q];
            if (apq != 0.0) {
                const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
#pragma unroll
                for (int k = 0; k < 3; k++) { const double akp = a[k][p], akq = a[k][q]; a[k][p] = c * akp - sn * akq; a[k][q] = sn * akp + c * akq; }
#pragma unroll
                for (int k = 0; k < 3; k++) { const double apk = a[p][k], aqk = a[q][k]; a[p][k] = c * apk - sn * aqk; a[q][k] = sn * apk + c * aqk; }
#pragma unroll
                for (int k = 0; k < 3; k++) { const double vkp = v[k][p], vkq = v[k][q]; v[k][p] = c * vkp - sn * vkq; v[k][q] = sn * vkp + c * vkq; }
            }
        }
    }
    const double l0 = 1.0 / sqrt(a[0][0]), l1 = 1.0 / sqrt(a[1][1]), l2 = 1.0 / sqrt(a[2][2]);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) W[i * 3 + j] = v[i][0] * v[j][0] * l0 + v[i][1] * v[j][1] * l1 + v[i][2] * v[j][2] * l2;
}

// 6x6 symmetric solve on ONE lane.  Fast path: LDL^T without pivoting, fully unrolled so that every array lives in
// registers (no scratch traffic on the critical path of the iteration).  If a pivot is not strictly positive/finite
// (semi-definite or indefinite system) fall back to the diagonally pivoted LDL^T of Eigen::LDLT on LDS arrays.
__host__ __device__ static bool icp_ldlt6_fast(const double *S /*21 upper-triangular sums*/, const double *b /*6*/, double *x) {
    double A[6][6];
    {
        int t = 0;
#pragma unroll
        for (int p = 0; p < 6; p++)
#pragma unroll
            for (int q = p; q < 6; q++) { A[q][p] = S[t]; t++; }      // lower triangle
    }
    double D[6], y[6];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 6; k++) {
        const double d = A[k][k];
        ok = ok && (d > 0.0) && isfinite(d);
        D[k] = d;
        const double inv = 1.0 / d;
        double col[6];
#pragma unroll
        for (int i = k + 1; i < 6; i++) col[i] = A[i][k];            // original column k below the diagonal
#pragma unroll
        for (int i = k + 1; i < 6; i++) {
            const double l = col[i] * inv;
#pragma unroll
            for (int j = k + 1; j <= i; j++) A[i][j] -= l * col[j];
            A[i][k] = l;
        }
    }
#pragma unroll
    for (int i = 0; i < 6; i++) {
        double s = b[i];
#pragma unroll
        for (int j = 0; j < i; j++) s -= A[i][j] * y[j];
        y[i] = s;
    }
#pragma unroll
    for (int i = 0; i < 6; i++) y[i] /= D[i];
#pragma unroll
    for (int i = 5; i >= 0; i--) {
        double s = y[i];
#pragma unroll
        for (int j = i + 1; j < 6; j++) s -= A[j][i] * x[j];
        x[i] = s;
    }
#pragma unroll
    for (int i = 0; i < 6; i++) ok = ok && isfinite(x[i]);
    return ok;
}

// pivoted fallback; w = LDS workspace of >= 36+36+6+6+6 doubles and 6 ints
__host__ __device__ static bool icp_ldlt6_pivoted(const double *S, const double *b6, double *x6, double *w, int *perm) {
    double *A = w, *L = w + 36, *D = w + 72, *y = w + 78, *z = w + 84;
    {
        int t = 0;
        for (int p = 0; p < 6; p++) for (int q = p; q < 6; q++) { A[p * 6 + q] = S[t]; A[q * 6 + p] = S[t]; t++; }
    }
    for (int i = 0; i < 36; i++) L[i] = 0;
    for (int i = 0; i < 6; i++) perm[i] = i;
    for (int k = 0; k < 6; k++) {
        int piv = k; double best = fabs(A[k * 6 + k]);
        for (int i = k + 1; i < 6; i++) if (fabs(A[i * 6 + i]) > best) { best = fabs(A[i * 6 + i]); piv = i; }
        if (piv != k) {
            for (int j = 0; j < 6; j++) { double t = A[k * 6 + j]; A[k * 6 + j] = A[piv * 6 + j]; A[piv * 6 + j] = t; }
            for (int j = 0; j < 6; j++) { double t = A[j * 6 + k]; A[j * 6 + k] = A[j * 6 + piv]; A[j * 6 + piv] = t; }
            for (int j = 0; j < k; j++) { double t = L[k * 6 + j]; L[k * 6 + j] = L[piv * 6 + j]; L[piv * 6 + j] = t; }
            int t = perm[k]; perm[k] = perm[piv]; perm[piv] = t;
        }
        const double d = A[k * 6 + k];
        D[k] = d; L[k * 6 + k] = 1.0;
        if (d == 0.0 || !isfinite(d)) return false;
        for (int i = k + 1; i < 6; i++) L[i * 6 + k] = A[i * 6 + k] / d;
        for (int i = k + 1; i < 6; i++)
            for (int j = k + 1; j < 6; j++) A[i * 6 + j] -= L[i * 6 + k] * d * L[j * 6 + k];
    }
    for (int i = 0; i < 6; i++) { double s = b6[perm[i]]; for (int j = 0; j < i; j++) s -= L[i * 6 + j] * y[j]; y[i] = s; }
    for (int i = 0; i < 6; i++) y[i] /= D[i];
    for (int i = 5; i >= 0; i--) { double s = y[i]; for (int j = i + 1; j < 6; j++) s -= L[j * 6 + i] * z[j]; z[i] = s; }
    bool ok = true;
    for (int i = 0; i < 6; i++) { const double v = z[i]; ok = ok && isfinite(v); w[90 + perm[i]] = v; }
    for (int i = 0; i < 6; i++) x6[i] = w[90 + i];
    return ok;
}
