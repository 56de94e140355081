"""Restatement of the voxel point map and of scan-to-map ICP on it (the rule: include/pcr_hip.h, "scan-to-map ICP on a voxel point map") in
numpy.  It imports neither the package nor a device nor the oracle.

  build_map      MAP (ON A GRID, AT A POSE): the kept points as rows ordered by (Morton key of the cell, input order), the cell table
  merge, insert, remove_far      the growth rules, on the rows
  sequential     the consequence the header states: every point, in arrival order, joins its cell's list while that list has fewer than M
                 entries -- written as exactly that, a dictionary of lists, so that it shares no code with merge
  rows_at        ROW OF A SOURCE POINT AT T over the candidate cells; brute_force_rows: the nearest of ALL rows (the exactness lemma's other side)
  linearize      UPDATE's sums over the rows, with the sum of the magnitudes of every entry's terms (the scale of a comparison); chunk regroups the sums
  loop           RegistrationICP's loop over rows_at / linearize / solve_update
"""
from dataclasses import dataclass, field

import numpy as np

import voxel_reference as vr

OFFSETS = {
    1: np.array([(0, 0, 0)], np.int64),
    7: np.array([(0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], np.int64),
    27: np.array([(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)], np.int64),
}
LIMIT = vr.MAX_INDEX + 1          # cell indices live in [0, 2^21)
L2, L1, GM = 0, 1, 2
POINT_TO_POINT, POINT_TO_PLANE = 1, 2


class OutsideGrid(ValueError):
    pass


@dataclass
class PointMapRef:
    voxel: float
    grid_min: np.ndarray           # (3,) float64
    max_points: int
    points: np.ndarray             # (rows, 3) float32
    normals: object                # (rows, 3) float32 or None
    row_cell: np.ndarray           # (rows, 3) int64: the cell of every row
    cells: np.ndarray = field(default=None)       # (m, 3) int64 in ascending Morton order
    starts: np.ndarray = field(default=None)      # (m,) first row
    counts: np.ndarray = field(default=None)      # (m,) members, 1 .. M
    lex_keys: np.ndarray = field(default=None, repr=False)      # vr.cell_key of the cells, ascending, and ...
    lex_cell: np.ndarray = field(default=None, repr=False)      # ... the cell-table row of each

    @property
    def origin(self):
        return self.grid_min - self.voxel * 0.5

    def __len__(self):
        return len(self.points)


def transform(src, T):
    """q_r = ((T_r0 x + T_r1 y) + T_r2 z) + T_r3 in float64 on the float32 coordinates, every operation rounded once"""
    p = np.ascontiguousarray(src, np.float32).astype(np.float64).reshape(-1, 3)
    T = np.asarray(T, np.float64).reshape(4, 4)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], 1)


def place(xyz, normals, T):
    """the members at a pose: p' = float32(q), n' = float32(R n) entry by entry; T None: the inputs bit for bit"""
    p = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    n = None if normals is None else np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    if T is None:
        return p, n
    T = np.asarray(T, np.float64).reshape(4, 4)
    q = transform(p, T).astype(np.float32)
    if n is not None:
        a = n.astype(np.float64)
        n = np.stack([(T[r, 0] * a[:, 0] + T[r, 1] * a[:, 1]) + T[r, 2] * a[:, 2] for r in range(3)], 1).astype(np.float32)
    return q, n


def _from_members(voxel, grid_min, M, pts, nrm):
    """the map of members given in arrival order: stable sort by the Morton key of the cell, rank inside the cell, cut at M"""
    grid_min = np.asarray(grid_min, np.float64).reshape(3)
    origin = grid_min - float(voxel) * 0.5
    if not np.isfinite(pts).all():
        raise OutsideGrid("a member is not finite")
    idx = np.floor((pts.astype(np.float64) - origin) / float(voxel))
    if not ((idx >= 0) & (idx < LIMIT)).all():
        raise OutsideGrid("a member lies outside the grid")
    idx = idx.astype(np.int64)
    key = vr.morton3(idx)
    order = np.argsort(key, kind="stable")
    ks = key[order]
    head = np.ones(len(ks), bool); head[1:] = ks[1:] != ks[:-1]
    first = np.nonzero(head)[0]
    rank = np.arange(len(ks)) - first[np.cumsum(head) - 1]
    rows = order[rank < M]
    return _finish(PointMapRef(float(voxel), grid_min, int(M), pts[rows], None if nrm is None else nrm[rows], idx[rows]))


def _finish(m):
    key = vr.morton3(m.row_cell)
    assert (key[1:] >= key[:-1]).all()
    head = np.ones(len(key), bool); head[1:] = key[1:] != key[:-1]
    m.starts = np.nonzero(head)[0].astype(np.int64)
    m.counts = np.diff(np.append(m.starts, len(key))).astype(np.int64)
    m.cells = m.row_cell[m.starts]
    lex = vr.cell_key(m.cells)
    o = np.argsort(lex)
    m.lex_keys, m.lex_cell = lex[o], o
    return m


def build_map(xyz, normals, voxel, M, grid_min=None, T=None):
    p, n = place(xyz, normals, T)
    if grid_min is None:
        assert T is None
        grid_min = p.astype(np.float64).min(0)
    return _from_members(voxel, grid_min, M, p, n)


def merge(a, b):
    """MERGE(a, b): in a shared cell a's members, then b's, cut at M"""
    assert a.voxel == b.voxel and np.array_equal(a.grid_min, b.grid_min) and a.max_points == b.max_points and (a.normals is None) == (b.normals is None)
    nrm = None if a.normals is None else np.concatenate([a.normals, b.normals])
    return _from_members(a.voxel, a.grid_min, a.max_points, np.concatenate([a.points, b.points]), nrm)


def insert(m, xyz, normals, T=None):
    """INSERT(m, cloud, T) = MERGE(m, the map of the cloud at T on m's grid)"""
    return merge(m, build_map(xyz, normals if m.normals is not None else None, m.voxel, m.max_points, m.grid_min, T))


def distance2(points, center):
    d = np.ascontiguousarray(points, np.float32).astype(np.float64) - np.asarray(center, np.float64).reshape(3)
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def remove_far(m, center, r):
    keep = distance2(m.points, center) < float(r) * float(r)
    if not keep.any():
        raise ValueError("would leave the map empty")
    return _finish(PointMapRef(m.voxel, m.grid_min, m.max_points, m.points[keep], None if m.normals is None else m.normals[keep], m.row_cell[keep]))


def sequential(clouds, voxel, M, grid_min):
    """KISS-ICP's rule, literally: `clouds` is a list of (xyz, normals or None, T or None) in arrival order; every point joins the list of its
    cell while the list has fewer than M entries.  Returns (cells in Morton order, {cell: list of (point bits, normal bits)})"""
    origin = np.asarray(grid_min, np.float64) - float(voxel) * 0.5
    lists = {}
    for xyz, nrm, T in clouds:
        p, n = place(xyz, nrm, T)
        idx = np.floor((p.astype(np.float64) - origin) / float(voxel)).astype(np.int64)
        for i in range(len(p)):
            cell = tuple(int(v) for v in idx[i])
            members = lists.setdefault(cell, [])
            if len(members) < M:
                members.append((p[i].tobytes(), None if n is None else n[i].tobytes()))
    cells = np.array(sorted(lists, key=lambda c: int(vr.morton3(np.array([c]))[0])), np.int64).reshape(-1, 3)
    return cells, lists


def equals_sequential(m, cells, lists):
    if not np.array_equal(m.cells, cells):
        return False
    for c, s, k in zip(m.cells, m.starts, m.counts):
        want = lists[tuple(int(v) for v in c)]
        got = [(m.points[r].tobytes(), None if m.normals is None else m.normals[r].tobytes()) for r in range(s, s + k)]
        if got != want:
            return False
    return True


# ------------------------------------------------------------------------------------------------------------------ the rows
def _d2(q, p):
    d = q - p.astype(np.float64)
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def match(m, src, T, neighborhood=27):
    """(row or -1, d^2) of every source point: the smallest (d^2, row) over the members of the candidate cells, whatever the distance"""
    q = transform(src, T)
    with np.errstate(invalid="ignore", over="ignore"):
        cell = np.floor((q - m.origin) / m.voxel)
    cell = np.where(np.isfinite(cell), cell, -4.0)
    cell = np.clip(cell, -4.0, float(LIMIT + 4)).astype(np.int64)
    best = np.full(len(q), np.inf)
    row = np.full(len(q), -1, np.int64)
    for off in OFFSETS[neighborhood]:
        c = cell + off
        ok = ((c >= 0) & (c < LIMIT)).all(1)
        key = vr.cell_key(np.where(ok[:, None], c, 0))
        pos = np.searchsorted(m.lex_keys, key).clip(max=len(m.lex_keys) - 1)
        ok &= m.lex_keys[pos] == key
        t = m.lex_cell[pos]
        for j in range(int(m.counts.max())):
            live = np.nonzero(ok & (m.counts[t] > j))[0]
            if len(live) == 0:
                break
            r = m.starts[t[live]] + j
            d2 = _d2(q[live], m.points[r])
            better = (d2 < best[live]) | ((d2 == best[live]) & (r < row[live]))
            best[live[better]] = d2[better]
            row[live[better]] = r[better]
    return row, best


def rows_at(m, src, T, max_distance, neighborhood=27, with_d2=False):
    """(rows, 2) int32 (i, map row), ordered by i: the match where d^2 < max_distance^2"""
    row, d2 = match(m, src, T, neighborhood)
    has = (row >= 0) & (d2 < float(max_distance) * float(max_distance))
    i = np.nonzero(has)[0]
    out = np.stack([i, row[i]], 1).astype(np.int32)
    return (out, d2[i]) if with_d2 else out


def brute_force_rows(m, src, T, max_distance, block=512):
    """the nearest of ALL map rows by (d^2, row), kept where d^2 < max_distance^2"""
    q = transform(src, T)
    p = m.points.astype(np.float64)
    out = []
    for i0 in range(0, len(q), block):
        d = q[i0:i0 + block, None, :] - p[None, :, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        r = d2.argmin(1)                               # (the first of equal minima: the smallest row)
        best = d2[np.arange(len(r)), r]
        has = best < float(max_distance) * float(max_distance)
        out.append(np.stack([np.nonzero(has)[0] + i0, r[has]], 1))
    return np.concatenate(out).astype(np.int32)


# ------------------------------------------------------------------------------------------------------------------ the update
def weight(loss, k, r):
    if loss == L1:
        return 1.0 / np.maximum(np.abs(r), 1e-300)
    if loss == GM:
        return k / ((k + r * r) * (k + r * r))
    return np.ones_like(r)


def _sum(terms, chunk):
    """sum over axis 0: numpy's own order, or, regrouped, chunk by chunk with the chunk sums added in order"""
    if chunk is None or len(terms) <= chunk:
        return terms.sum(0)
    out = np.zeros(terms.shape[1:])
    for i0 in range(0, len(terms), chunk):
        out = out + terms[i0:i0 + chunk].sum(0)
    return out


def linearize(m, src, T, max_distance, neighborhood=27, kind=POINT_TO_POINT, loss=L2, k=1.0, chunk=None):
    """dict(JTJ (6, 6), JTr (6,), rows, sum_d2, sum_r2, mag_JTJ, mag_JTr, pairs): mag_* = the sums of the absolute values of the terms"""
    pairs, d2 = rows_at(m, src, T, max_distance, neighborhood, with_d2=True)
    s = transform(src, T)[pairs[:, 0]]
    t = m.points[pairs[:, 1]].astype(np.float64)
    e = s - t
    if kind == POINT_TO_PLANE:
        n = m.normals[pairs[:, 1]].astype(np.float64)
        r = ((e[:, 0] * n[:, 0] + e[:, 1] * n[:, 1]) + e[:, 2] * n[:, 2])[:, None]               # (rows, 1)
        J = np.concatenate([np.cross(s, n), n], 1)[:, None, :]                                   # (rows, 1, 6)
        w = weight(loss, k, r[:, 0])[:, None]
        sum_r2 = float(_sum(r[:, 0] * r[:, 0], chunk))
    else:
        nn = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
        r = e                                                                                    # (rows, 3)
        z, o = np.zeros(len(s)), np.ones(len(s))
        J = np.stack([np.stack([z, s[:, 2], -s[:, 1], o, z, z], 1), np.stack([-s[:, 2], z, s[:, 0], z, o, z], 1), np.stack([s[:, 1], -s[:, 0], z, z, z, o], 1)], 1)
        w = np.repeat(weight(loss, k, np.sqrt(nn))[:, None], 3, 1)
        sum_r2 = float(_sum(nn, chunk))
    tJ = (w[:, :, None, None] * J[:, :, :, None] * J[:, :, None, :]).sum(1)                      # per source point, its rows in the order x, y, z
    tr = (w[:, :, None] * J * r[:, :, None]).sum(1)
    mJ = (np.abs(w[:, :, None, None] * J[:, :, :, None] * J[:, :, None, :])).sum(1)
    mr = (np.abs(w[:, :, None] * J * r[:, :, None])).sum(1)
    return dict(JTJ=_sum(tJ, chunk), JTr=_sum(tr, chunk), rows=len(pairs), sum_d2=float(_sum(d2, chunk)), sum_r2=sum_r2, mag_JTJ=mJ.sum(0), mag_JTr=mr.sum(0),
                pairs=pairs)


def solve_update(JTJ, JTr):
    """x = -JTJ^-1 JTr, the pose Rz(x2) Ry(x1) Rx(x0) with the translation x[3:]; the identity when the solve fails"""
    try:
        x = np.linalg.solve(JTJ, -JTr)
    except np.linalg.LinAlgError:
        return np.eye(4)
    if not np.isfinite(x).all():
        return np.eye(4)
    sa, ca, sb, cb, sg, cg = np.sin(x[0]), np.cos(x[0]), np.sin(x[1]), np.cos(x[1]), np.sin(x[2]), np.cos(x[2])
    U = np.eye(4)
    U[:3, :3] = [[cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa], [sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa], [-sb, cb * sa, cb * ca]]
    U[:3, 3] = x[3:]
    return U


@dataclass
class LoopResult:
    transformation: np.ndarray
    fitness: float
    inlier_rmse: float
    n_rows: int
    iterations: int
    converged: bool
    history: list = field(repr=False, default_factory=list)      # after every update: (pose, fitness, inlier_rmse, rows)

    def after(self, max_it):
        """what the same loop returns under a smaller max_iteration (its trajectory is a prefix of this one)"""
        if self.iterations <= max_it:
            return self
        T, fit, rmse, n = self.history[max_it - 1]
        return LoopResult(T, fit, rmse, n, max_it, False)


def loop(m, src, T0, max_distance, neighborhood=27, kind=POINT_TO_POINT, loss=L2, k=1.0, max_it=30, rel_fitness=1e-6, rel_rmse=1e-6, chunk=None):
    n = len(np.asarray(src).reshape(-1, 3))
    T = np.array(T0, np.float64).reshape(4, 4)

    def lin(T):
        s = linearize(m, src, T, max_distance, neighborhood, kind, loss, k, chunk)
        rows = s["rows"]
        return s, (rows / n if n else 0.0), (float(np.sqrt(s["sum_d2"] / rows)) if rows else 0.0)

    s, fit, rmse = lin(T)
    it, converged, history = 0, False, []
    while it < max_it:
        U = solve_update(s["JTJ"], s["JTr"]) if s["rows"] else np.eye(4)
        T = U @ T
        before = (fit, rmse)
        s, fit, rmse = lin(T)
        it += 1
        history.append((T.copy(), fit, rmse, s["rows"]))
        if abs(before[0] - fit) < rel_fitness and abs(before[1] - rmse) < rel_rmse:
            converged = True
            break
    return LoopResult(T, fit, rmse, s["rows"], it, converged, history)


# ------------------------------------------------------------------------------------------------------------------ the adaptive threshold
def model_error(predicted, estimated, max_range):
    D = np.linalg.inv(np.asarray(predicted, np.float64)) @ np.asarray(estimated, np.float64)
    theta = np.arccos(np.clip((np.trace(D[:3, :3]) - 1.0) / 2.0, -1.0, 1.0))
    return float(np.linalg.norm(D[:3, 3]) + 2.0 * max_range * np.sin(theta / 2.0))
