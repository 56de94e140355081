"""Farthest point sampling as include/pcr_hip.h states it (DIST, INIT, STEP, RESULT), restated in numpy: the specification the device is compared
with bit for bit.  numpy rounds every difference, product and sum on its own (no fused multiply-add), which is the DIST rule."""
import numpy as np


def d2_to_row(pts, s):
    """DIST: float64 on the float32 coordinates, differences, squares and sums in the order x, y, z, each rounded once -> (n,) float64"""
    p = np.asarray(pts, dtype=np.float32).astype(np.float64)
    ex, ey, ez = p[:, 0] - p[s, 0], p[:, 1] - p[s, 1], p[:, 2] - p[s, 2]
    d2 = ex * ex
    d2 = d2 + ey * ey
    d2 = d2 + ez * ez
    return d2


def farthest_point_reference(pts, k, start=0):
    """-> dict(sel (k,) int64 in selection order, dist (n,) float64 final running distances (-1 on non-finite rows), maxima (k,) float64 = m after
    every step, tie_steps = the number of steps whose maximum m > 0 is held by more than one row, cover_dist2 = m after the last step)"""
    pts = np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 3)
    n = len(pts)
    assert 0 <= k <= n and (k == 0 or 0 <= start < n)
    finite = np.isfinite(pts).all(axis=1)
    assert k == 0 or finite[start], "start_index names a non-finite row"
    dist = np.where(finite, np.inf, -1.0)
    sel = np.zeros(k, dtype=np.int64)
    maxima = np.zeros(k, dtype=np.float64)
    tie_steps = 0
    cur = int(start)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(k):
            sel[i] = cur
            d2 = d2_to_row(pts, cur)
            upd = finite & (d2 < dist)
            dist = np.where(upd, d2, dist)
            m = 0.0
            if finite.any():
                m = max(0.0, float(dist[finite].max()))
            maxima[i] = m
            if m > 0.0:
                at = np.nonzero(dist == m)[0]
                tie_steps += 1 if len(at) > 1 else 0
                cur = int(at[0])              # the smallest index: an ascending scan with a strict >
    return dict(sel=sel, dist=dist, maxima=maxima, tie_steps=tie_steps, cover_dist2=float(maxima[-1]) if k else 0.0)


def lattice(side=6):
    """the side^3 unit lattice in ``ij`` order: row (a side + b) side + c = (a, b, c)"""
    g = np.arange(side, dtype=np.float32)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
