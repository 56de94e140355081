"""Numpy restatement of the boundary point rule (include/pcr_hip.h, ``pcr_boundary_points``), written in the rule's own operation order: the
yardstick of the boundary tests.  The rows come from ``neighbor_reference.hybrid`` (the search index's result rule on the cloud itself).

Everything up to the arguments of ``arctan2`` is float64 arithmetic in which numpy rounds every product, sum and difference once, as the rule
asks, so those bits are the device's; ``arctan2`` itself is libm's and differs from the device's by ulps."""
import numpy as np

import neighbor_reference as nref

TWO_PI = 2.0 * np.pi


def threshold(angle_threshold):
    """T of rule 6, evaluated left to right."""
    return float(angle_threshold) * np.pi / 180.0


def _cross(p, q):
    """(p_y q_z - p_z q_y, p_z q_x - p_x q_z, p_x q_y - p_y q_x), every product and difference rounded once."""
    return np.stack([p[:, 1] * q[:, 2] - p[:, 2] * q[:, 1], p[:, 2] * q[:, 0] - p[:, 0] * q[:, 2], p[:, 0] * q[:, 1] - p[:, 1] * q[:, 0]], 1)


def frames(normals):
    """(u, v) of rule 3 for float32 normals (n, 3): e = the axis of the smallest |component| (np.argmin takes the first on a tie: x, y, z)."""
    nrm = np.asarray(normals, np.float32).reshape(-1, 3).astype(np.float64)
    with np.errstate(invalid="ignore"):
        axis = np.argmin(np.abs(nrm), axis=1)
    e = np.zeros_like(nrm)
    e[np.arange(len(nrm)), axis] = 1.0
    with np.errstate(invalid="ignore", over="ignore"):
        v = _cross(nrm, e)
        u = _cross(v, nrm)
    return u, v


def boundary(points, normals, radius, max_nn, angle_threshold, chunk=1000):
    """-> dict(mask (n,) bool, gap (n,) float64 radians, counts (n,) int32, m (n,) angles per row, idx (n, max_nn) the rows, T)."""
    pts = np.asarray(points, np.float32).reshape(-1, 3)
    nrm = np.asarray(normals, np.float32).reshape(-1, 3)
    n = len(pts)
    T = threshold(angle_threshold)
    if n == 0:
        return dict(mask=np.zeros(0, bool), gap=np.zeros(0), counts=np.zeros(0, np.int32), m=np.zeros(0, np.int64), idx=np.zeros((0, max_nn), np.int64), T=T)
    # rule 1
    idx, _, counts = nref.hybrid(pts, pts, radius, max_nn, chunk=chunk)
    p, nn = pts.astype(np.float64), nrm.astype(np.float64)
    # rule 2
    decided = np.isfinite(p).all(1) & np.isfinite(nn).all(1) & ~(nn == 0.0).all(1)
    # rule 3
    u, v = frames(nrm)
    # rule 4
    member = np.arange(max_nn)[None, :] < counts[:, None]
    j = np.where(member, idx, 0)
    with np.errstate(invalid="ignore", over="ignore"):
        d = p[j] - p[:, None, :]
        x = (u[:, None, 0] * d[..., 0] + u[:, None, 1] * d[..., 1]) + u[:, None, 2] * d[..., 2]
        y = (v[:, None, 0] * d[..., 0] + v[:, None, 1] * d[..., 1]) + v[:, None, 2] * d[..., 2]
        used = member & decided[:, None] & ~((x == 0.0) & (y == 0.0))
        ang = np.where(used, np.arctan2(y, x), np.inf)
    # rule 5
    m = used.sum(1)
    a = np.sort(ang, axis=1)
    gap = np.zeros(n)
    if max_nn > 1:
        with np.errstate(invalid="ignore"):
            step = a[:, 1:] - a[:, :-1]
        step = np.where(np.arange(1, max_nn)[None, :] < m[:, None], step, 0.0)
        gap = step.max(1)
    has = m > 0
    last = a[np.arange(n), np.maximum(m - 1, 0)]
    wrap = np.where(has, TWO_PI - (np.where(has, last, 0.0) - np.where(has, a[:, 0], 0.0)), 0.0)
    gap = np.where(has, np.maximum(gap, wrap), 0.0)
    # rule 6
    return dict(mask=has & (gap > T), gap=gap, counts=counts.astype(np.int32), m=m, idx=idx, T=T)


# ---------------------------------------------------------------------------------------------------- analytic shapes
def grid_cloud(side=32):
    """side x side unit grid in z = 0 with normals +z -> (points, normals) float32"""
    g = np.arange(side, dtype=np.float32)
    xx, yy = np.meshgrid(g, g, indexing="ij")
    pts = np.stack([xx.ravel(), yy.ravel(), np.zeros(side * side, np.float32)], 1).astype(np.float32)
    nrm = np.tile(np.array([0.0, 0.0, 1.0], np.float32), (len(pts), 1))
    return pts, nrm


def fibonacci_sphere(n=4096):
    """n points of a Fibonacci lattice on the unit sphere with radial normals -> (points, normals) float32"""
    i = np.arange(n, dtype=np.float64)
    z = 1.0 - (2.0 * i + 1.0) / n
    r = np.sqrt(1.0 - z * z)
    phi = i * (np.pi * (3.0 - np.sqrt(5.0)))
    pts = np.stack([r * np.cos(phi), r * np.sin(phi), z], 1).astype(np.float32)
    return pts, pts.copy()


def cut_sphere(n=4096, z_cut=0.5):
    """the Fibonacci sphere with z > z_cut removed"""
    pts, nrm = fibonacci_sphere(n)
    keep = ~(pts[:, 2] > z_cut)
    return pts[keep], nrm[keep]
