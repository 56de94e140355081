// pcr_eigen3.h -- the non-iterative symmetric 3x3 eigen solver the normal estimators share (pcr_cloud.hip, pcr_pmap.hip).  A unit includes it under its own
// floating-point contraction setting.
#pragma once
#include <cmath>

// ---- analytic symmetric 3x3 eigenvector of the smallest eigenvalue (Eberly's non-iterative solver)
__device__ static inline void d_cross(const double *a, const double *b, double *c) {
    c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ static inline double d_dot(const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
// A = [a00 a01 a02; a01 a11 a12; a02 a12 a22] passed as 6 values
__device__ static void d_eigvec0(const double *A, double ev, double *out) {
    double r0[3] = {A[0] - ev, A[1], A[2]}, r1[3] = {A[1], A[3] - ev, A[4]}, r2[3] = {A[2], A[4], A[5] - ev};
    double c01[3], c02[3], c12[3];
    d_cross(r0, r1, c01); d_cross(r0, r2, c02); d_cross(r1, r2, c12);
    double d0 = d_dot(c01, c01), d1 = d_dot(c02, c02), d2 = d_dot(c12, c12);
    double dmax = d0; int imax = 0;
    if (d1 > dmax) { dmax = d1; imax = 1; }
    if (d2 > dmax) { imax = 2; }
    double s;
    if (imax == 0) { s = sqrt(d0); out[0] = c01[0] / s; out[1] = c01[1] / s; out[2] = c01[2] / s; }
    else if (imax == 1) { s = sqrt(d1); out[0] = c02[0] / s; out[1] = c02[1] / s; out[2] = c02[2] / s; }
    else { s = sqrt(d2); out[0] = c12[0] / s; out[1] = c12[1] / s; out[2] = c12[2] / s; }
}
__device__ static void d_eigvec1(const double *A, const double *e0, double ev1, double *out) {
    double U[3], V[3];
    if (fabs(e0[0]) > fabs(e0[1])) { double inv = 1.0 / sqrt(e0[0] * e0[0] + e0[2] * e0[2]); U[0] = -e0[2] * inv; U[1] = 0; U[2] = e0[0] * inv; }
    else { double inv = 1.0 / sqrt(e0[1] * e0[1] + e0[2] * e0[2]); U[0] = 0; U[1] = e0[2] * inv; U[2] = -e0[1] * inv; }
    d_cross(e0, U, V);
    double AU[3] = {A[0] * U[0] + A[1] * U[1] + A[2] * U[2], A[1] * U[0] + A[3] * U[1] + A[4] * U[2], A[2] * U[0] + A[4] * U[1] + A[5] * U[2]};
    double AV[3] = {A[0] * V[0] + A[1] * V[1] + A[2] * V[2], A[1] * V[0] + A[3] * V[1] + A[4] * V[2], A[2] * V[0] + A[4] * V[1] + A[5] * V[2]};
    double m00 = d_dot(U, AU) - ev1, m01 = d_dot(U, AV), m11 = d_dot(V, AV) - ev1;
    double a00 = fabs(m00), a01 = fabs(m01), a11 = fabs(m11);
    if (a00 >= a11) {
        if (fmax(a00, a01) > 0) {
            if (a00 >= a01) { m01 /= m00; m00 = 1 / sqrt(1 + m01 * m01); m01 *= m00; }
            else { m00 /= m01; m01 = 1 / sqrt(1 + m00 * m00); m00 *= m01; }
            for (int k = 0; k < 3; k++) out[k] = m01 * U[k] - m00 * V[k];
        } else { out[0] = U[0]; out[1] = U[1]; out[2] = U[2]; }
    } else {
        if (fmax(a11, a01) > 0) {
            if (a11 >= a01) { m01 /= m11; m11 = 1 / sqrt(1 + m01 * m01); m01 *= m11; }
            else { m11 /= m01; m01 = 1 / sqrt(1 + m11 * m11); m11 *= m01; }
            for (int k = 0; k < 3; k++) out[k] = m11 * U[k] - m01 * V[k];
        } else { out[0] = U[0]; out[1] = U[1]; out[2] = U[2]; }
    }
}
__device__ static void d_fast_eigen3x3(const double *C6, double *nv) {
    double A[6];
    double mc = C6[0];
    for (int k = 1; k < 6; k++) mc = fmax(mc, C6[k]);
    if (mc == 0.0) { nv[0] = nv[1] = nv[2] = 0; return; }
    for (int k = 0; k < 6; k++) A[k] = C6[k] / mc;
    const double norm = A[1] * A[1] + A[2] * A[2] + A[4] * A[4];
    if (norm > 0) {
        const double q = (A[0] + A[3] + A[5]) / 3.0;
        const double b00 = A[0] - q, b11 = A[3] - q, b22 = A[5] - q;
        const double p = sqrt((b00 * b00 + b11 * b11 + b22 * b22 + norm * 2.0) / 6.0);
        const double c00 = b11 * b22 - A[4] * A[4], c01 = A[1] * b22 - A[4] * A[2], c02 = A[1] * A[4] - b11 * A[2];
        const double det = (b00 * c00 - A[1] * c01 + A[2] * c02) / (p * p * p);
        double hd = det * 0.5; hd = fmin(fmax(hd, -1.0), 1.0);
        const double angle = acos(hd) / 3.0;
        const double two_thirds_pi = 2.09439510239319549;
        const double beta2 = cos(angle) * 2.0, beta0 = cos(angle + two_thirds_pi) * 2.0, beta1 = -(beta0 + beta2);
        const double ev0 = q + p * beta0, ev1 = q + p * beta1, ev2 = q + p * beta2;
        double e0[3], e1[3], e2[3];
        if (hd >= 0) {
            d_eigvec0(A, ev2, e2);
            if (ev2 < ev0 && ev2 < ev1) { nv[0] = e2[0]; nv[1] = e2[1]; nv[2] = e2[2]; return; }
            d_eigvec1(A, e2, ev1, e1);
            if (ev1 < ev0 && ev1 < ev2) { nv[0] = e1[0]; nv[1] = e1[1]; nv[2] = e1[2]; return; }
            d_cross(e1, e2, e0);
            nv[0] = e0[0]; nv[1] = e0[1]; nv[2] = e0[2];
        } else {
            d_eigvec0(A, ev0, e0);
            if (ev0 < ev1 && ev0 < ev2) { nv[0] = e0[0]; nv[1] = e0[1]; nv[2] = e0[2]; return; }
            d_eigvec1(A, e0, ev1, e1);
            if (ev1 < ev0 && ev1 < ev2) { nv[0] = e1[0]; nv[1] = e1[1]; nv[2] = e1[2]; return; }
            d_cross(e0, e1, e2);
            nv[0] = e2[0]; nv[1] = e2[1]; nv[2] = e2[2];
        }
    } else {
        // diagonal matrix: axis of the smallest diagonal entry, (0,0,1) on ties
        if (A[0] < A[3] && A[0] < A[5]) { nv[0] = 1; nv[1] = 0; nv[2] = 0; }
        else if (A[3] < A[0] && A[3] < A[5]) { nv[0] = 0; nv[1] = 1; nv[2] = 0; }
        else { nv[0] = 0; nv[1] = 0; nv[2] = 1; }
    }
}
