"""Restatement of the plane segmentation rules of include/pcr_hip.h (SAMPLE, FIT, SCORE, BETTER, STOP, RESULT) in numpy / ``math``: the
sequential loop itself, in float64 on the float32 points, every operation rounded on its own and in the order the header writes out -- Python
floats and numpy's element-wise ufuncs do not contract -- so planes, distances and inlier decisions have the bits the device has.  What the
device sums in its own order (the err of a hypothesis, the moments of the refit) is summed with ``math.fsum`` here and compared with a tolerance.

Two CONDITIONS of an exact comparison are counted and are asserted to be 0 by the tests that compare:
  rim   (hypothesis, point) pairs with |dist - thr| <= 1e-9 thr (the decision is made on identical bits anyway; a rim pair would make it fragile)
  near  hypotheses whose count equals the running best's with an rmse within 1e-9 relative of it (err is summed in another order on the device)"""
import math

import numpy as np

M64 = (1 << 64) - 1
ZERO_PLANE = (0.0, 0.0, 0.0, 0.0)


def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def sample_rows(seed, ransac_n, i, n):
    return [splitmix64((seed + ransac_n * i + k) & M64) % n for k in range(ransac_n)]


def plane_from_normal(nx, ny, nz, ox, oy, oz):
    """-> (valid, (a, b, c, d)); the zero plane when the norm is not > 0 or the plane is not finite"""
    norm = math.sqrt((nx * nx + ny * ny) + nz * nz)
    if not norm > 0.0 or not math.isfinite(norm):
        return False, ZERO_PLANE
    a, b, c = nx / norm, ny / norm, nz / norm
    d = -((a * ox + b * oy) + c * oz)
    if not all(math.isfinite(v) for v in (a, b, c, d)):
        return False, ZERO_PLANE
    return True, (a, b, c, d)


def plane_from_3(p0, p1, p2):
    ux, uy, uz = p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]
    vx, vy, vz = p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]
    return plane_from_normal(uy * vz - uz * vy, uz * vx - ux * vz, ux * vy - uy * vx, p0[0], p0[1], p0[2])


def plane_from_moments(c, m):
    """the moment fit: centroid c, second moments m = (xx, xy, xz, yy, yz, zz) about it (sums)"""
    xx, xy, xz, yy, yz, zz = m
    det_x = yy * zz - yz * yz
    det_y = xx * zz - xz * xz
    det_z = xx * yy - xy * xy
    if det_x > det_y and det_x > det_z:
        n = (det_x, xz * yz - xy * zz, xy * yz - xz * yy)
    elif det_y > det_z:
        n = (xz * yz - xy * zz, det_y, xy * xz - yz * xx)
    else:
        n = (xy * yz - xz * yy, xy * xz - yz * xx, det_z)
    return plane_from_normal(n[0], n[1], n[2], c[0], c[1], c[2])


def plane_from_sample(ps):
    """ps: the sampled points (tuples of Python floats) in draw order; 3 points: the cross product, more: the moment fit, sums left to right"""
    if len(ps) == 3:
        return plane_from_3(*ps)
    k = float(len(ps))
    s = [0.0, 0.0, 0.0]
    for p in ps:
        s = [s[0] + p[0], s[1] + p[1], s[2] + p[2]]
    c = (s[0] / k, s[1] / k, s[2] / k)
    m = [0.0] * 6
    for p in ps:
        x, y, z = p[0] - c[0], p[1] - c[1], p[2] - c[2]
        m = [m[0] + x * x, m[1] + x * y, m[2] + x * z, m[3] + y * y, m[4] + y * z, m[5] + z * z]
    return plane_from_moments(c, m)


def plane_dist(plane, X, Y, Z):
    """|((a x + b y) + c z) + d| on float64 arrays (or floats), one rounding per operation"""
    a, b, c, d = plane
    return np.abs(((a * X + b * Y) + c * Z) + d)


def refit_fsum(pts64):
    """the moment fit over the rows of pts64 with exactly rounded sums -> (valid, plane)"""
    k = float(len(pts64))
    c = tuple(math.fsum(pts64[:, j].tolist()) / k for j in range(3))
    q = pts64 - np.array(c)
    m = [math.fsum((q[:, u] * q[:, v]).tolist()) for u, v in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
    return plane_from_moments(c, m)


class _Cloud:
    def __init__(self, pts):
        p = np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 3)
        self.p64 = p.astype(np.float64)
        self.X, self.Y, self.Z = (np.ascontiguousarray(self.p64[:, j]) for j in range(3))
        self.rows = [tuple(float(v) for v in r) for r in self.p64] if len(p) <= 100000 else None
        self.n = len(p)

    def row(self, r):
        return self.rows[r] if self.rows is not None else tuple(float(v) for v in self.p64[r])

    def hypothesis(self, thr, seed, ransac_n, i):
        """-> (valid, plane, count (-1: invalid), err, rim pairs)"""
        ok, plane = plane_from_sample([self.row(r) for r in sample_rows(seed, ransac_n, i, self.n)])
        if not ok:
            return False, ZERO_PLANE, -1, 0.0, 0
        d = plane_dist(plane, self.X, self.Y, self.Z)
        inl = d < thr
        rim = int((np.abs(d - thr) <= 1e-9 * thr).sum())
        return True, plane, int(inl.sum()), math.fsum(d[inl].tolist()), rim


def plane_hypotheses(pts, thr, seed, ransac_n, first, count):
    """what the test hook returns for iterations [first, first + count), no early stop -> dict(valid, plane (count, 4), count, err, rim)"""
    c = _Cloud(pts)
    out = [c.hypothesis(thr, seed, ransac_n, first + h) for h in range(count)]
    return dict(valid=np.array([o[0] for o in out], dtype=np.uint8), plane=np.array([o[1] for o in out], dtype=np.float64).reshape(count, 4),
                count=np.array([o[2] for o in out], dtype=np.int32), err=np.array([o[3] for o in out], dtype=np.float64), rim=sum(o[4] for o in out))


def segment_plane_reference(pts, thr, ransac_n=3, num_iterations=100, probability=0.99999999, seed=0):
    """The sequential loop -> dict(plane (refit with fsum; zeros if none or degenerate), inliers (ascending int64), iterations_run,
    best_iteration, n_valid, count, best_plane, fitness, rmse, rim, near)"""
    c = _Cloud(pts)
    n = c.n
    assert 3 <= ransac_n <= 8 and n >= ransac_n
    est_k, i = num_iterations, 0
    best = dict(count=0, rmse=0.0, err=0.0, it=-1, plane=ZERO_PLANE)
    n_valid = rim = near = 0
    log_fail = math.log(1.0 - probability) if probability < 1.0 else None
    while i < est_k:
        ok, plane, cnt, err, r = c.hypothesis(thr, seed, ransac_n, i)
        rim += r
        if ok:
            n_valid += 1
        if cnt > 0:
            rmse = err / math.sqrt(float(cnt))
            if cnt == best["count"] and abs(rmse - best["rmse"]) <= 1e-9 * best["rmse"]:
                near += 1
            if cnt > best["count"] or (cnt == best["count"] and rmse < best["rmse"]):
                best = dict(count=cnt, rmse=rmse, err=err, it=i, plane=plane)
                if log_fail is not None:
                    if cnt == n:
                        kp = 0.0
                    else:
                        p = 1.0
                        for _ in range(ransac_n):
                            p *= cnt / n
                        den = math.log1p(-p)
                        kp = log_fail / den if den != 0.0 else math.inf
                    if math.isfinite(kp) and 0.0 <= kp < est_k:
                        est_k = int(math.ceil(kp))
        i += 1
    out = dict(iterations_run=i, best_iteration=best["it"], n_valid=n_valid, count=best["count"], best_plane=np.array(best["plane"]),
               fitness=best["count"] / n, rmse=best["rmse"], rim=rim, near=near, plane=np.zeros(4), inliers=np.zeros(0, np.int64))
    if best["it"] >= 0:
        inl = plane_dist(best["plane"], c.X, c.Y, c.Z) < thr
        out["inliers"] = np.nonzero(inl)[0].astype(np.int64)
        out["plane"] = np.array(refit_fsum(c.p64[inl])[1])
    return out


def plane_difference(p, q):
    """(angle between the normals [rad] by the chord, |d_p - d_q|) of two planes with unit normals"""
    p, q = np.asarray(p, float), np.asarray(q, float)
    return float(2.0 * math.asin(min(1.0, 0.5 * float(np.linalg.norm(p[:3] - q[:3]))))), abs(float(p[3] - q[3]))
