"""Plain numpy restatement of the Scan Context rule of include/pcr_hip.h (``pcr_scan_context``, ``pcr_scan_context_distance``): the polar
height image of a scan and the shift-minimised mean column cosine distance of two images (Kim and Kim, IROS 2018).  Every sum whose order
matters is an explicit loop in the stated order; the device must give these rows bit for bit.  ``tables`` builds the float64 tables the
library takes as arguments, exactly as the package does (place.scan_context_tables is this function's twin)."""
import math

import numpy as np

DEFAULTS = (20, 60, 80.0, 2.0)          # num_rings, num_sectors, max_range, height_offset


def tables(num_rings, num_sectors, max_range):
    """(ring_bound2[R-1], cos_k[S/4-1], sin_k[S/4-1], L2), float64, elementwise as the header writes them."""
    R, S, L = int(num_rings), int(num_sectors), float(max_range)
    bounds = [float(k) * L / R for k in range(1, R)]
    ring_bound2 = np.array([b * b for b in bounds], dtype=np.float64)
    cos_k = np.array([math.cos(2.0 * math.pi * k / S) for k in range(1, S // 4)], dtype=np.float64)
    sin_k = np.array([math.sin(2.0 * math.pi * k / S) for k in range(1, S // 4)], dtype=np.float64)
    return ring_bound2, cos_k, sin_k, L * L


def descriptor(xyz, num_rings=20, num_sectors=60, max_range=80.0, height_offset=2.0):
    """-> ((R, S) float32 descriptor, dict(used, dropped_nonfinite, dropped_range))."""
    R, S = int(num_rings), int(num_sectors)
    ring_bound2, cos_k, sin_k, L2 = tables(R, S, max_range)
    p = np.ascontiguousarray(np.asarray(xyz, dtype=np.float32).reshape(-1, 3))
    finite = np.isfinite(p).all(axis=1)
    q = p[finite]
    x, y = q[:, 0].astype(np.float64), q[:, 1].astype(np.float64)
    rho2 = x * x + y * y                                   # float32 squares are exact in float64: one rounding, in the sum
    inside = (rho2 < L2) & (rho2 != 0.0)
    x, y, z, rho2 = x[inside], y[inside], q[inside, 2], rho2[inside]
    ring = (rho2[:, None] >= ring_bound2[None, :]).sum(axis=1)
    quad = np.full(len(x), -1)
    quad[(x > 0) & (y >= 0)] = 0
    quad[(x <= 0) & (y > 0)] = 1
    quad[(x < 0) & (y <= 0)] = 2
    quad[(x >= 0) & (y < 0)] = 3
    assert (quad >= 0).all()
    u = np.choose(quad, [x, y, -x, -y])
    v = np.choose(quad, [y, -x, -y, x])
    within = ((v[:, None] * cos_k[None, :]) >= (u[:, None] * sin_k[None, :])).sum(axis=1)
    sector = quad * (S // 4) + within
    value = z.astype(np.float32) + np.float32(height_offset)          # float32 + float32 in float32
    desc = np.full((R, S), -np.inf, dtype=np.float32)
    np.maximum.at(desc, (ring, sector), value)
    desc[np.isneginf(desc)] = np.float32(0.0)                         # a cell without rows
    desc[desc == 0] = np.float32(0.0)                                  # a maximum of -0.0 is stored as +0.0
    info = dict(used=int(inside.sum()), dropped_nonfinite=int((~finite).sum()), dropped_range=int((~inside).sum()))
    return desc, info


def distance(A, B):
    """-> (distance float64, shift int) of the query descriptor A and the candidate descriptor B."""
    A = np.asarray(A, dtype=np.float32).astype(np.float64)
    B = np.asarray(B, dtype=np.float32).astype(np.float64)
    assert A.shape == B.shape and A.ndim == 2
    R, S = A.shape
    nA, nB, G = np.zeros(S), np.zeros(S), np.zeros((S, S))
    for r in range(R):                                      # r ascending; product rounded, then added
        nA = nA + A[r] * A[r]
        nB = nB + B[r] * B[r]
        G = G + A[r][:, None] * B[r][None, :]
    valid = (nA > 0)[:, None] & (nB > 0)[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        Cm = G / (np.sqrt(nA)[:, None] * np.sqrt(nB)[None, :])
    best, best_n = None, 0
    for n in range(S):
        total, m = 0.0, 0
        for j in range(S):                                  # j ascending
            jp = (j - n) % S
            if valid[j, jp]:
                total = total + Cm[j, jp]
                m += 1
        d = 1.0 - total / float(m) if m > 0 else 1.0
        if best is None or d < best:
            best, best_n = d, n
    return np.float64(best), best_n


def distance_block(descs_a, descs_b):
    """-> ((nA, nB) float64, (nA, nB) int32)."""
    dist = np.zeros((len(descs_a), len(descs_b)), dtype=np.float64)
    shift = np.zeros((len(descs_a), len(descs_b)), dtype=np.int32)
    for a, A in enumerate(descs_a):
        for b, B in enumerate(descs_b):
            dist[a, b], shift[a, b] = distance(A, B)
    return dist, shift


def loop_closures(dist, shift, max_distance, exclude_recent=50, top_k=1):
    """The selection of ScanContextDatabase.detect_loop_closures from a full (N, N) matrix: -> (int64 rows (i, j, shift), float64 distances)."""
    rows, ds = [], []
    for i in range(dist.shape[0]):
        cand = [(dist[i, j], j) for j in range(dist.shape[1]) if i - j > exclude_recent and dist[i, j] <= max_distance]
        for d, j in sorted(cand)[:top_k]:
            rows.append((i, j, int(shift[i, j]))); ds.append(d)
    return np.array(rows, dtype=np.int64).reshape(-1, 3), np.array(ds, dtype=np.float64)


def rotate_z(xyz, degrees):
    """The cloud turned about z, computed in float64 and rounded to float32."""
    a = math.radians(degrees)
    c, s = math.cos(a), math.sin(a)
    p = np.asarray(xyz, dtype=np.float64)
    out = np.stack([c * p[:, 0] - s * p[:, 1], s * p[:, 0] + c * p[:, 1], p[:, 2]], axis=1)
    return out.astype(np.float32)
