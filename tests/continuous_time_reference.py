"""Restatement of the continuous-time rule (include/pcr_hip.h, "continuous time") in numpy, on top of tests/point_map_reference.py.  It imports
neither the package nor a device nor the oracle.

  exp3, log3     E(v) and Log(R) of the rule
  alphas         TIMES: alpha_i in float64 on the widened float32
  place          POSE AT alpha: (q, u, alpha) of every source point for a pose pair
  deskew         DESKEW(cloud, D, alpha_ref)
  match_q        the ROW rule of the voxel point map on points that are already placed (float64, not rounded)
  linearize      UPDATE's 12-column sums, with the sum of the magnitudes of every entry's terms (the scale of a comparison)
  step, loop     STEP and LOOP on the host
  skew           the planted input of the tests: p_i = float32(T(alpha_i)^-1 W_i)
  odometry_icp, odometry_ct      the recipes, on the restatement's maps
"""
from dataclasses import dataclass, field

import numpy as np

import point_map_reference as pm
import voxel_reference as vr


# ------------------------------------------------------------------------------------------------------------------ rotations
def exp3(v):
    """E(v) for v of shape (..., 3) -> (..., 3, 3)"""
    v = np.asarray(v, np.float64)
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    xx, yy, zz = x * x, y * y, z * z
    t2 = (xx + yy) + zz
    th = np.sqrt(t2)
    big = th >= 1e-4
    safe_th, safe_t2 = np.where(big, th, 1.0), np.where(big, t2, 1.0)
    A = np.where(big, np.sin(safe_th) / safe_th, 1.0 - t2 / 6.0)
    B = np.where(big, (1.0 - np.cos(safe_th)) / safe_t2, 0.5 - t2 / 24.0)
    xy, xz, yz = x * y, x * z, y * z
    E = np.empty(v.shape[:-1] + (3, 3))
    E[..., 0, 0] = 1.0 - B * (yy + zz); E[..., 0, 1] = B * xy - A * z;       E[..., 0, 2] = B * xz + A * y
    E[..., 1, 0] = B * xy + A * z;       E[..., 1, 1] = 1.0 - B * (xx + zz); E[..., 1, 2] = B * yz - A * x
    E[..., 2, 0] = B * xz - A * y;       E[..., 2, 1] = B * yz + A * x;       E[..., 2, 2] = 1.0 - B * (xx + yy)
    return E


def log3(R):
    """the rotation vector of R, angle in [0, pi]"""
    R = np.asarray(R, np.float64).reshape(3, 3)
    w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) * 0.5
    s = np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
    c = ((R[0, 0] + R[1, 1]) + R[2, 2] - 1.0) * 0.5
    theta = np.arctan2(s, c)
    if s < 1e-8 and c > 0.0:
        return w
    if c > -0.99:
        return w * (theta / s)
    d = np.diag(R)
    k = int(np.argmax(d))
    a = np.zeros(3)
    a[k] = np.sqrt(max((d[k] - c) / (1.0 - c), 0.0))
    for j in range(3):
        if j != k:
            a[j] = (R[k, j] + R[j, k]) * 0.5 / ((1.0 - c) * a[k]) if a[k] > 0.0 else 0.0
    n = np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])
    sign = -1.0 if (a[0] * w[0] + a[1] * w[1]) + a[2] * w[2] < 0.0 else 1.0
    return sign * theta * a / n if n > 0.0 else np.zeros(3)


def _mul3(a, b):
    """a b with every entry (a_i0 b_0j + a_i1 b_1j) + a_i2 b_2j; a (3, 3), b (..., 3, 3)"""
    out = np.empty(b.shape)
    for i in range(3):
        for j in range(3):
            out[..., i, j] = (a[i, 0] * b[..., 0, j] + a[i, 1] * b[..., 1, j]) + a[i, 2] * b[..., 2, j]
    return out


def _rotate(R, p):
    """the rotated point (r0 x + r1 y) + r2 z of every row; R (n, 3, 3) or (3, 3), p (n, 3) float64"""
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([(R[..., r, 0] * x + R[..., r, 1] * y) + R[..., r, 2] * z for r in range(3)], 1)


def _rotate_t(R, w):
    """R^T w entry by entry (r_0d w_0 + r_1d w_1) + r_2d w_2; R (3, 3)"""
    return np.stack([(R[0, d] * w[:, 0] + R[1, d] * w[:, 1]) + R[2, d] * w[:, 2] for d in range(3)], 1)


# ------------------------------------------------------------------------------------------------------------------ times and poses
def span(times, t0=None, t1=None):
    t = np.ascontiguousarray(times, np.float32)
    t0 = float(t.min()) if t0 is None else float(t0)
    t1 = float(t.max()) if t1 is None else float(t1)
    if not (np.isfinite(t0) and np.isfinite(t1) and t1 > t0):
        raise ValueError("t1 must be greater than t0")
    return t0, t1


def alphas(times, t0, t1):
    t = np.ascontiguousarray(times, np.float32)
    if not np.isfinite(t).all():
        raise ValueError("times holds a non-finite value")
    return (t.astype(np.float64) - float(t0)) / (float(t1) - float(t0))


def rotations(Rb, Re, alpha):
    """R(alpha) = R_b E(alpha phi) for every alpha"""
    Rb, Re = np.asarray(Rb, np.float64), np.asarray(Re, np.float64)
    phi = log3(_mul3(Rb.T.copy(), Re))
    return _mul3(Rb, exp3(alpha[:, None] * phi[None, :]))


def place(src, times, T_b, T_e, t0, t1):
    """(q, u, alpha): the placed point, the rotated point and the fraction of every source point"""
    p = np.ascontiguousarray(src, np.float32).astype(np.float64).reshape(-1, 3)
    T_b, T_e = np.asarray(T_b, np.float64).reshape(4, 4), np.asarray(T_e, np.float64).reshape(4, 4)
    a = alphas(times, t0, t1)
    u = _rotate(rotations(T_b[:3, :3], T_e[:3, :3], a), p)
    t = T_b[:3, 3][None, :] + a[:, None] * (T_e[:3, 3] - T_b[:3, 3])[None, :]
    return u + t, u, a


def pose_at(T_b, T_e, alpha):
    """T(alpha) as 4x4 matrices, (n, 4, 4)"""
    T_b, T_e = np.asarray(T_b, np.float64), np.asarray(T_e, np.float64)
    alpha = np.atleast_1d(np.asarray(alpha, np.float64))
    T = np.zeros((len(alpha), 4, 4))
    T[:, :3, :3] = rotations(T_b[:3, :3], T_e[:3, :3], alpha)
    T[:, :3, 3] = T_b[:3, 3][None, :] + alpha[:, None] * (T_e[:3, 3] - T_b[:3, 3])[None, :]
    T[:, 3, 3] = 1.0
    return T


def skew(world, alpha, T_b, T_e):
    """what a sensor that moves from T_b to T_e measures of the world points W: p_i = float32(T(alpha_i)^-1 W_i)"""
    W = np.asarray(world, np.float64).reshape(-1, 3)
    T = pose_at(T_b, T_e, alpha)
    d = W - T[:, :3, 3]
    return np.einsum("nji,nj->ni", T[:, :3, :3], d).astype(np.float32)


def azimuth_alpha(xyz):
    """synthetic times: the azimuth of every point in the sensor frame mapped to [0, 1], float32"""
    p = np.asarray(xyz, np.float64).reshape(-1, 3)
    return ((np.arctan2(p[:, 1], p[:, 0]) + np.pi) / (2.0 * np.pi)).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------ deskew
def deskew(xyz, normals, times, D, alpha_ref=1.0, t0=None, t1=None):
    """(points float32, normals float32 or None) in the sensor frame at alpha_ref"""
    p = np.ascontiguousarray(xyz, np.float32).astype(np.float64).reshape(-1, 3)
    D = np.asarray(D, np.float64).reshape(4, 4)
    t0, t1 = span(times, t0, t1)
    a = alphas(times, t0, t1)
    phi = log3(D[:3, :3])
    R = exp3(a[:, None] * phi[None, :])
    Rr = exp3(float(alpha_ref) * phi)
    tau = D[:3, 3]
    w = (_rotate(R, p) + a[:, None] * tau[None, :]) - (float(alpha_ref) * tau)[None, :]
    out = _rotate_t(Rr, w).astype(np.float32)
    nrm = None
    if normals is not None:
        n = np.ascontiguousarray(normals, np.float32).astype(np.float64).reshape(-1, 3)
        nrm = _rotate_t(Rr, _rotate(R, n)).astype(np.float32)
    return out, nrm


# ------------------------------------------------------------------------------------------------------------------ the rows
def match_q(m, q, neighborhood=27):
    """pm.match for points that are already placed: (row or -1, d^2) by the smallest (d^2, row) over the members of the candidate cells"""
    with np.errstate(invalid="ignore", over="ignore"):
        cell = np.floor((q - m.origin) / m.voxel)
    cell = np.where(np.isfinite(cell), cell, -4.0)
    cell = np.clip(cell, -4.0, float(pm.LIMIT + 4)).astype(np.int64)
    best = np.full(len(q), np.inf)
    row = np.full(len(q), -1, np.int64)
    for off in pm.OFFSETS[neighborhood]:
        c = cell + off
        ok = ((c >= 0) & (c < pm.LIMIT)).all(1)
        key = vr.cell_key(np.where(ok[:, None], c, 0))
        pos = np.searchsorted(m.lex_keys, key).clip(max=len(m.lex_keys) - 1)
        ok &= m.lex_keys[pos] == key
        t = m.lex_cell[pos]
        for j in range(int(m.counts.max())):
            live = np.nonzero(ok & (m.counts[t] > j))[0]
            if len(live) == 0:
                break
            r = m.starts[t[live]] + j
            d2 = pm._d2(q[live], m.points[r])
            better = (d2 < best[live]) | ((d2 == best[live]) & (r < row[live]))
            best[live[better]] = d2[better]
            row[live[better]] = r[better]
    return row, best


def matches_at(m, q, max_distance, neighborhood=27, valid=None, plane=False):
    """(match per source point or -1, d^2): the ROW rule with the distance bound; valid: the validity of an estimated map's rows, read by point to plane"""
    row, d2 = match_q(m, q, neighborhood)
    has = (row >= 0) & (d2 < float(max_distance) * float(max_distance))
    if valid is not None and plane:
        has &= np.asarray(valid, bool)[np.where(row >= 0, row, 0)]
    return np.where(has, row, -1).astype(np.int32), d2


def linearize(m, src, times, T_b, T_e, max_distance, neighborhood=27, kind=pm.POINT_TO_POINT, loss=pm.L2, k=1.0, t0=None, t1=None, valid=None, chunk=None):
    """dict(H (12, 12), g (12,), rows, sum_d2, sum_r2, mag_H, mag_g, matches); residuals and J12 per row too (for the finite differences)"""
    t0, t1 = span(times, t0, t1)
    q, u, a = place(src, times, T_b, T_e, t0, t1)
    plane = kind == pm.POINT_TO_PLANE
    matches, d2 = matches_at(m, q, max_distance, neighborhood, valid, plane)
    i = np.nonzero(matches >= 0)[0]
    r_ = matches[i]
    q, u, a, d2 = q[i], u[i], a[i], d2[i]
    e = q - m.points[r_].astype(np.float64)
    if plane:
        n = m.normals[r_].astype(np.float64)
        r = ((e[:, 0] * n[:, 0] + e[:, 1] * n[:, 1]) + e[:, 2] * n[:, 2])[:, None]
        J = np.concatenate([np.cross(u, n), n], 1)[:, None, :]
        w = pm.weight(loss, k, r[:, 0])[:, None]
        sum_r2 = float(pm._sum(r[:, 0] * r[:, 0], chunk))
    else:
        nn = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
        r = e
        z, o = np.zeros(len(u)), np.ones(len(u))
        J = np.stack([np.stack([z, u[:, 2], -u[:, 1], o, z, z], 1), np.stack([-u[:, 2], z, u[:, 0], z, o, z], 1), np.stack([u[:, 1], -u[:, 0], z, z, z, o], 1)], 1)
        w = np.repeat(pm.weight(loss, k, np.sqrt(nn))[:, None], 3, 1)
        sum_r2 = float(pm._sum(nn, chunk))
    J12 = np.concatenate([(1.0 - a)[:, None, None] * J, a[:, None, None] * J], 2)                    # (rows, 1 or 3, 12)
    tH = (w[:, :, None, None] * J12[:, :, :, None] * J12[:, :, None, :]).sum(1)
    tg = (w[:, :, None] * J12 * r[:, :, None]).sum(1)
    mH = np.abs(w[:, :, None, None] * J12[:, :, :, None] * J12[:, :, None, :]).sum(1)
    mg = np.abs(w[:, :, None] * J12 * r[:, :, None]).sum(1)
    return dict(H=pm._sum(tH, chunk).reshape(12, 12), g=pm._sum(tg, chunk).reshape(12), rows=len(i), sum_d2=float(pm._sum(d2, chunk)), sum_r2=sum_r2,
                mag_H=mH.sum(0).reshape(12, 12), mag_g=mg.sum(0).reshape(12), matches=matches, residuals=r, J12=J12, weights=w)


# ------------------------------------------------------------------------------------------------------------------ step and loop
def step(H, g, rows, T_b, T_e, begin="fixed", prior=None, prior_weight=None):
    """STEP: (T_b, T_e, applied).  prior: the T_begin the call was given; prior_weight: (w_rot, w_trans) or None"""
    T_b, T_e = np.array(T_b, np.float64), np.array(T_e, np.float64)
    H, g = np.array(H, np.float64), np.array(g, np.float64)
    if begin == "free" and prior_weight is not None:
        w_rot, w_trans = float(prior_weight[0]), float(prior_weight[1])
        H[0:3, 0:3] += rows * w_rot * np.eye(3)
        H[3:6, 3:6] += rows * w_trans * np.eye(3)
        g[0:3] += rows * w_rot * log3(T_b[:3, :3] @ np.asarray(prior, np.float64)[:3, :3].T)
        g[3:6] += rows * w_trans * (T_b[:3, 3] - np.asarray(prior, np.float64)[:3, 3])
    lo = 6 if begin == "fixed" else 0
    delta = np.zeros(12)
    try:
        L = np.linalg.cholesky(H[lo:, lo:])
        delta[lo:] = -np.linalg.solve(L.T, np.linalg.solve(L, g[lo:]))
    except np.linalg.LinAlgError:
        return T_b, T_e, False
    if not np.isfinite(delta).all():
        return T_b, T_e, False
    if begin != "fixed":
        T_b[:3, :3] = exp3(delta[0:3]) @ T_b[:3, :3]
        T_b[:3, 3] = T_b[:3, 3] + delta[3:6]
    T_e[:3, :3] = exp3(delta[6:9]) @ T_e[:3, :3]
    T_e[:3, 3] = T_e[:3, 3] + delta[9:12]
    return T_b, T_e, True


@dataclass
class CtResult:
    begin_pose: np.ndarray
    end_pose: np.ndarray
    fitness: float
    inlier_rmse: float
    n_rows: int
    iterations: int
    converged: bool
    matches: np.ndarray = field(repr=False, default=None)
    history: list = field(repr=False, default_factory=list)      # after every update: (begin pose, end pose, fitness, inlier_rmse, rows, matches)

    def after(self, max_it):
        """what the same loop returns under a smaller max_iteration (its trajectory is a prefix of this one)"""
        if self.iterations <= max_it:
            return self
        b, e, fit, rmse, n, matches = self.history[max_it - 1]
        return CtResult(b, e, fit, rmse, n, max_it, False, matches)


def loop(m, src, times, T_b, T_e, max_distance, neighborhood=27, kind=pm.POINT_TO_POINT, loss=pm.L2, k=1.0, max_it=30, rel_fitness=1e-6, rel_rmse=1e-6, begin="fixed",
         prior_weight=None, t0=None, t1=None, valid=None, chunk=None):
    n = len(np.asarray(src).reshape(-1, 3))
    T_b, T_e = np.array(T_b, np.float64).reshape(4, 4), np.array(T_e, np.float64).reshape(4, 4)
    prior = T_b.copy()
    t0, t1 = span(times, t0, t1)

    def lin(T_b, T_e):
        s = linearize(m, src, times, T_b, T_e, max_distance, neighborhood, kind, loss, k, t0, t1, valid, chunk)
        rows = s["rows"]
        return s, (rows / n if n else 0.0), (float(np.sqrt(s["sum_d2"] / rows)) if rows else 0.0)

    s, fit, rmse = lin(T_b, T_e)
    it, converged, history = 0, False, []
    while it < max_it:
        applied = False
        if s["rows"]:
            T_b, T_e, applied = step(s["H"], s["g"], s["rows"], T_b, T_e, begin, prior, prior_weight)
        if not applied:
            break
        before = (fit, rmse)
        s, fit, rmse = lin(T_b, T_e)
        it += 1
        history.append((T_b.copy(), T_e.copy(), fit, rmse, s["rows"], s["matches"]))
        if abs(before[0] - fit) < rel_fitness and abs(before[1] - rmse) < rel_rmse:
            converged = True
            break
    return CtResult(T_b, T_e, fit, rmse, s["rows"], it, converged, s["matches"], history)


# ------------------------------------------------------------------------------------------------------------------ the recipes
def odometry_icp(scans, times, voxel, max_distance, deskewed, grid_min, M=20, neighborhood=27, kind=pm.POINT_TO_POINT, max_it=30):
    """scan_to_map_odometry_icp under "constant_velocity" on scans without normals (point to point) -> (poses, map)"""
    poses = [np.eye(4)]
    m = pm.build_map(scans[0], None, voxel, M, grid_min, np.eye(4))
    for k in range(1, len(scans)):
        start, scan = poses[-1], scans[k]
        if k >= 2:
            start = poses[-1] @ np.linalg.inv(poses[-2]) @ poses[-1]
            if deskewed:
                scan = deskew(scan, None, times[k], np.linalg.inv(poses[-2]) @ poses[-1])[0]
        res = pm.loop(m, scan, start, max_distance, neighborhood, kind, max_it=max_it)
        poses.append(res.transformation)
        m = pm.insert(m, scan, None, poses[-1])
    return poses, m


def odometry_ct(scans, times, voxel, max_distance, grid_min, M=20, neighborhood=27, kind=pm.POINT_TO_POINT, max_it=30, init=np.eye(4)):
    """scan_to_map_odometry_ct with begin = "fixed" -> (begin poses, end poses, map)"""
    init = np.array(init, np.float64)
    begins, ends = [init], [init]
    m = pm.build_map(scans[0], None, voxel, M, grid_min, init)
    for k in range(1, len(scans)):
        T_b = ends[-1]
        T_e = ends[-1] @ np.linalg.inv(begins[-1]) @ ends[-1] if k > 1 else T_b
        res = loop(m, scans[k], times[k], T_b, T_e, max_distance, neighborhood, kind, max_it=max_it)
        begins.append(res.begin_pose); ends.append(res.end_pose)
        d = deskew(scans[k], None, times[k], np.linalg.inv(res.begin_pose) @ res.end_pose)[0]
        m = pm.insert(m, d, None, res.end_pose)
    return begins, ends, m
