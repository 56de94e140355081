// pcr_plane.h -- the plane arithmetic of segment_plane (pcr_segment.hip), host and device: the point-to-plane distance every kernel decides
// inliers with, the plane through three points, and the moment fit (Open3D's GetPlaneFromPoints) that the hypothesis kernel runs on a sample
// of 4..8 points and the host runs on the reduced moments of the inliers.  Float64 on float32 coordinates, every product, sum, quotient and
// square root rounded on its own (contraction off in every function), in the operation order written out in include/pcr_hip.h: a host
// recomputation in that order gives the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

// |((a x + b y) + c z) + d|
__host__ __device__ static inline double pcr_plane_dist(const double *pl, double x, double y, double z) {
#pragma clang fp contract(off)
    const double ax = pl[0] * x, by = pl[1] * y, cz = pl[2] * z;
    double s = ax + by;
    s = s + cz;
    s = s + pl[3];
    return fabs(s);
}

// (nx, ny, nz) normalised, d = -((a ox + b oy) + c oz) for the point o of the plane; false (and the zero plane): the norm is not > 0 or
// the plane is not finite
__host__ __device__ static inline bool pcr_plane_from_normal(double nx, double ny, double nz, double ox, double oy, double oz, double *pl) {
#pragma clang fp contract(off)
    const double xx = nx * nx, yy = ny * ny, zz = nz * nz;
    double s = xx + yy;
    s = s + zz;
    const double norm = sqrt(s);
    const double a = nx / norm, b = ny / norm, c = nz / norm;
    const double ax = a * ox, by = b * oy, cz = c * oz;
    double t = ax + by;
    t = t + cz;
    const double d = -t;
    const bool ok = norm > 0.0 && __builtin_isfinite(a) && __builtin_isfinite(b) && __builtin_isfinite(c) && __builtin_isfinite(d);
    pl[0] = ok ? a : 0.0; pl[1] = ok ? b : 0.0; pl[2] = ok ? c : 0.0; pl[3] = ok ? d : 0.0;
    return ok;
}

// the plane through p0, p1, p2: normal (p1 - p0) x (p2 - p0), through p0
__host__ __device__ static inline bool pcr_plane_from_3(const double *p0, const double *p1, const double *p2, double *pl) {
#pragma clang fp contract(off)
    const double ux = p1[0] - p0[0], uy = p1[1] - p0[1], uz = p1[2] - p0[2];
    const double vx = p2[0] - p0[0], vy = p2[1] - p0[1], vz = p2[2] - p0[2];
    const double a1 = uy * vz, a2 = uz * vy, b1 = uz * vx, b2 = ux * vz, c1 = ux * vy, c2 = uy * vx;
    return pcr_plane_from_normal(a1 - a2, b1 - b2, c1 - c2, p0[0], p0[1], p0[2], pl);
}

// THE moment fit: centroid c and the six second moments m = (xx, xy, xz, yy, yz, zz) about it (sums, not divided by the count).  The normal is
// the column of the adjugate of the moment matrix that belongs to the largest of its diagonal minors.
__host__ __device__ static inline bool pcr_plane_from_moments(const double *c, const double *m, double *pl) {
#pragma clang fp contract(off)
    const double xx = m[0], xy = m[1], xz = m[2], yy = m[3], yz = m[4], zz = m[5];
    const double yyzz = yy * zz, yzyz = yz * yz, xxzz = xx * zz, xzxz = xz * xz, xxyy = xx * yy, xyxy = xy * xy;
    const double det_x = yyzz - yzyz, det_y = xxzz - xzxz, det_z = xxyy - xyxy;
    const double xzyz = xz * yz, xyzz = xy * zz, xyyz = xy * yz, xzyy = xz * yy, xyxz = xy * xz, yzxx = yz * xx;
    const double p = xzyz - xyzz, q = xyyz - xzyy, r = xyxz - yzxx;
    double nx, ny, nz;
    if (det_x > det_y && det_x > det_z) { nx = det_x; ny = p; nz = q; }
    else if (det_y > det_z) { nx = p; ny = det_y; nz = r; }
    else { nx = q; ny = r; nz = det_z; }
    return pcr_plane_from_normal(nx, ny, nz, c[0], c[1], c[2], pl);
}

// the moment fit of a sample of N float32 points (N in 4..8): sums over k = 0 .. N - 1 in that order, centroid = sum / N, moments about it
template <int N> __host__ __device__ static inline bool pcr_plane_from_sample(const float (*s)[3], double *pl) {
#pragma clang fp contract(off)
    double sum[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < N; k++) { sum[0] = sum[0] + (double)s[k][0]; sum[1] = sum[1] + (double)s[k][1]; sum[2] = sum[2] + (double)s[k][2]; }
    const double c[3] = {sum[0] / (double)N, sum[1] / (double)N, sum[2] / (double)N};
    double m[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < N; k++) {
        const double x = (double)s[k][0] - c[0], y = (double)s[k][1] - c[1], z = (double)s[k][2] - c[2];
        const double xx = x * x, xy = x * y, xz = x * z, yy = y * y, yz = y * z, zz = z * z;
        m[0] = m[0] + xx; m[1] = m[1] + xy; m[2] = m[2] + xz; m[3] = m[3] + yy; m[4] = m[4] + yz; m[5] = m[5] + zz;
    }
    return pcr_plane_from_moments(c, m, pl);
}
