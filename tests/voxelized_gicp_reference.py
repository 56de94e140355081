"""Restatement of voxelized GICP on a voxel covariance map (the rule: include/pcr_hip.h, "voxelized GICP on a voxel covariance map") in
numpy on top of tests/voxel_reference.py (the grid and the ordered sums) and of the CPU oracle (the per-correspondence GICP arithmetic,
the 6x6 solve).  It imports neither the package nor a device.

  build_map   cells, counts, float32 means and float32 mean covariances, rows in Morton order of the cell
  rows_at     the rows (i, v) at a pose, ordered by i and then by the neighbourhood's offset order
  linearize   sum over the rows of N_v x (what the oracle's GICP linearisation gives for (q_i, R C_i R^T, mu_v, C_v)): one oracle call per
              distinct N_v on the virtual target (mu, C) -- the sums are linear in the rows
  loop        RegistrationICP's loop over rows_at / linearize / the oracle's solve_update
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


def _oracle():
    from oracle import oracle as orc
    return orc


def cov6_of(cov33):
    c = np.asarray(cov33).reshape(-1, 3, 3)
    return np.stack([c[:, 0, 0], c[:, 0, 1], c[:, 0, 2], c[:, 1, 1], c[:, 1, 2], c[:, 2, 2]], 1)


def cov33_of(cov6):
    c = np.asarray(cov6, np.float64).reshape(-1, 6)
    return c[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(-1, 3, 3)


def cov6_from_normals(normals, epsilon=1e-3):
    """the member covariance of a cloud that carries normals: the GICP estimator's, in float64 from the float32 normal, rounded to float32"""
    n32 = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    return cov6_of(_oracle().covariances_from_normals(n32.astype(np.float64), epsilon)).astype(np.float32)


@dataclass
class MapRef:
    voxel: float
    origin: np.ndarray             # (3,) float64
    cells: np.ndarray              # (m, 3) int64, in ascending Morton order
    count: np.ndarray              # (m,) int64
    mean: np.ndarray               # (m, 3) float32
    cov6: np.ndarray               # (m, 6) float32
    cell_of_point: np.ndarray      # (n,) map row of every input point
    lex_keys: np.ndarray = field(repr=False, default=None)      # vr.cell_key of the cells, ascending, and ...
    lex_row: np.ndarray = field(repr=False, default=None)       # ... the map row of each


def build_map(xyz, cov6, voxel):
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    cov6 = np.ascontiguousarray(cov6, np.float32).reshape(-1, 6)
    assert len(cov6) == len(xyz)
    ref = vr.voxel_reference(xyz, voxel)
    m = len(ref.keys)
    sums = vr.ordered_sums(cov6, ref.cell_of_point, m)
    c6 = (sums / ref.count[:, None].astype(np.float64)).astype(np.float32)
    order = np.argsort(vr.morton3(ref.cells), kind="stable")          # lexicographic row -> Morton row
    row_of_lex = np.empty(m, np.int64)
    row_of_lex[order] = np.arange(m)
    return MapRef(float(voxel), ref.origin, ref.cells[order], ref.count[order], ref.points[order], c6[order], row_of_lex[ref.cell_of_point],
                  ref.keys, row_of_lex)


def transform(src, T):
    """q_r = ((T_r0 x + T_r1 y) + T_r2 z) + T_r3 in float64 on the float32 coordinates, every operation rounded once"""
    p = np.ascontiguousarray(src, np.float32).astype(np.float64).reshape(-1, 3)
    T = np.asarray(T, np.float64).reshape(4, 4)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], 1)


def candidate_rows(mp, src, T, neighborhood=1, min_points_per_voxel=1):
    """(n, neighbourhood) int64: the map row of every candidate cell of every source point, -1 where the candidate gives no row"""
    q = transform(src, T)
    with np.errstate(invalid="ignore", over="ignore"):
        cell = np.floor((q - mp.origin) / mp.voxel)
    cell = np.where(np.isfinite(cell), cell, -4.0)
    cell = np.clip(cell, -4.0, float(LIMIT + 4)).astype(np.int64)
    out = np.full((len(q), len(OFFSETS[neighborhood])), -1, np.int64)
    for k, off in enumerate(OFFSETS[neighborhood]):
        c = cell + off
        ok = ((c >= 0) & (c < LIMIT)).all(1)
        key = vr.cell_key(np.where(ok[:, None], c, 0))
        pos = np.searchsorted(mp.lex_keys, key).clip(max=len(mp.lex_keys) - 1)
        ok &= mp.lex_keys[pos] == key
        row = mp.lex_row[pos]
        ok &= mp.count[row] >= min_points_per_voxel
        out[:, k] = np.where(ok, row, -1)
    return out


def rows_at(mp, src, T, neighborhood=1, min_points_per_voxel=1):
    """(rows, 2) int32 (i, v), ordered by i, then by offset order"""
    cand = candidate_rows(mp, src, T, neighborhood, min_points_per_voxel)
    i, k = np.nonzero(cand >= 0)                      # row-major: by i, then by k
    return np.stack([i, cand[i, k]], 1).astype(np.int32)


def evaluate(mp, src, T, rows):
    """fitness, inlier_rmse of the rows at T"""
    n = len(np.asarray(src).reshape(-1, 3))
    if len(rows) == 0:
        return 0.0, 0.0
    q = transform(src, T)
    d = q[rows[:, 0]] - mp.mean[rows[:, 1]].astype(np.float64)
    return len(np.unique(rows[:, 0])) / n, float(np.sqrt((d * d).sum() / len(rows)))


def rotate_covariances(R, C):
    """R C_i R^T of every (3, 3) C_i as the oracle rotates a cloud's covariances (transform_cloud: m3_mul, then m3_mul_bt): (R C) R^T, every
    entry (a_0 b_0 + a_1 b_1) + a_2 b_2 in float64 with every operation rounded once -- an order a matrix product of a library does not promise"""
    RC = np.empty_like(C)
    out = np.empty_like(C)
    for i in range(3):
        for j in range(3):
            RC[:, i, j] = (R[i, 0] * C[:, 0, j] + R[i, 1] * C[:, 1, j]) + R[i, 2] * C[:, 2, j]
    for i in range(3):
        for j in range(3):
            out[:, i, j] = (RC[:, i, 0] * R[j, 0] + RC[:, i, 1] * R[j, 1]) + RC[:, i, 2] * R[j, 2]
    return out


def linearize(mp, src, src_cov6, T, rows, loss=0, loss_k=1.0):
    """JTJ (6, 6), JTr (6,) of the update at T over `rows`"""
    orc = _oracle()
    T = np.asarray(T, np.float64).reshape(4, 4)
    q = transform(src, T)
    Cs = rotate_covariances(T[:3, :3], cov33_of(np.ascontiguousarray(src_cov6, np.float32)))
    mu, Cv = mp.mean.astype(np.float64), cov33_of(mp.cov6)
    JTJ, JTr = np.zeros((6, 6)), np.zeros(6)
    nv = mp.count[rows[:, 1]]
    for c in np.unique(nv):
        A, b, _ = orc.gicp_linearize(q, Cs, mu, Cv, rows[nv == c], loss, loss_k)
        JTJ += float(c) * A
        JTr += float(c) * b
    return JTJ, JTr


@dataclass
class LoopResult:
    transformation: np.ndarray
    fitness: float
    inlier_rmse: float
    n_rows: int
    iterations: int
    converged: bool
    rows: np.ndarray = field(repr=False, default=None)
    history: list = field(repr=False, default_factory=list)      # after every update: (pose, fitness, inlier_rmse, rows)
    extra: dict = field(default_factory=dict)

    def after(self, max_it):
        """what the same loop returns under a smaller max_iteration (its trajectory is a prefix of this one)"""
        if self.iterations <= max_it:
            return self
        T, fit, rmse, n = self.history[max_it - 1]
        return LoopResult(T, fit, rmse, n, max_it, False)


def loop(mp, src, src_cov6, T0, neighborhood=1, min_points_per_voxel=1, loss=0, loss_k=1.0, max_it=30, rel_fitness=1e-6, rel_rmse=1e-6):
    orc = _oracle()
    T = np.array(T0, np.float64).reshape(4, 4)
    rows = rows_at(mp, src, T, neighborhood, min_points_per_voxel)
    fit, rmse = evaluate(mp, src, T, rows)
    it, converged, history = 0, False, []
    while it < max_it:
        U = np.eye(4)
        if len(rows):
            JTJ, JTr = linearize(mp, src, src_cov6, T, rows, loss, loss_k)
            U, _ = orc.solve_update(JTJ, JTr)          # (the identity when the solve fails, as Open3D)
        T = U @ T
        before = (fit, rmse)
        rows = rows_at(mp, src, T, neighborhood, min_points_per_voxel)
        fit, rmse = evaluate(mp, src, T, rows)
        it += 1
        history.append((T.copy(), fit, rmse, len(rows)))
        if abs(before[0] - fit) < rel_fitness and abs(before[1] - rmse) < rel_rmse:
            converged = True
            break
    return LoopResult(T, fit, rmse, len(rows), it, converged, rows, history)
