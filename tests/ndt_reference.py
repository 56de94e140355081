"""Restatement of NDT registration on a normal-distributions voxel map (the rule: include/pcr_hip.h, "NDT on a normal-distributions voxel
map") in numpy.  It stands on tests/voxel_reference.py (the grid and the ordered sums) and tests/voxelized_gicp_reference.py (the map of a
six-channel member statistic, the pose expression, the candidate rows, fitness and RMSE) for what they already state, and on the CPU oracle
for the 6x6 solve and the pose update.  It imports neither the package nor a device.

  build_map        cells, counts, float32 means, float32 C_v, float64 information matrices A_v (numpy.linalg.eigh) and the valid flags
  rows_at          the rows (i, v) at a pose: the candidate rows of the voxelized GICP rule that land in a VALID cell
  score_constants  d1, d2 of Magnusson's score from the outlier ratio and the voxel size
  linearize        JTJ, JTr, score, sum_d2, rows, points_with_rows at a pose -- and, per sum, the sum of the magnitudes of its terms
  loop             RegistrationICP's loop over rows_at / linearize / the oracle's solve_update
"""
from dataclasses import dataclass, field

import numpy as np

import voxelized_gicp_reference as vg

OFFSETS, LIMIT, transform, evaluate, LoopResult = vg.OFFSETS, vg.LIMIT, vg.transform, vg.evaluate, vg.LoopResult


@dataclass
class NdtMapRef:
    voxel: float
    origin: np.ndarray             # (3,) float64
    cells: np.ndarray              # (m, 3) int64, in ascending Morton order
    count: np.ndarray              # (m,) int64
    mean: np.ndarray               # (m, 3) float32
    cov6: np.ndarray               # (m, 6) float32: C_v
    info: np.ndarray               # (m, 3, 3) float64: A_v, zero for an invalid cell
    valid: np.ndarray              # (m,) bool
    clamped: np.ndarray            # (m,) eigenvalues raised to eigenvalue_ratio * lambda_max (0 for an invalid cell)
    cell_of_point: np.ndarray      # (n,) map row of every input point
    base: vg.MapRef = field(repr=False, default=None)      # the same rows as a voxelized GICP map (what candidate_rows reads)

    @property
    def info6(self):
        return vg.cov6_of(self.info)


def member_products(xyz, mean_of_point):
    """the six products of d = float64(p) - float64(mu), each rounded once to float64 and then to float32"""
    d = np.ascontiguousarray(xyz, np.float32).astype(np.float64).reshape(-1, 3) - np.ascontiguousarray(mean_of_point, np.float32).astype(np.float64)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    return np.stack([x * x, x * y, x * z, y * y, y * z, z * z], 1).astype(np.float32)


def information(cov6, count, min_points_per_voxel=6, eigenvalue_ratio=0.01):
    """(A_v (m, 3, 3), valid (m,), clamped (m,)) from the float32 C_v and the counts"""
    count = np.asarray(count, np.int64)
    m = len(count)
    info, valid, clamped = np.zeros((m, 3, 3)), np.zeros(m, bool), np.zeros(m, np.int64)
    enough = count >= max(int(min_points_per_voxel), 2)
    if not enough.any():
        return info, valid, clamped
    nv = count[enough].astype(np.float64)
    S = vg.cov33_of(cov6)[enough] * nv[:, None, None] / (nv[:, None, None] - 1.0)
    lam, V = np.linalg.eigh(S)
    lmax = lam.max(1)
    ok = lmax > 0.0
    floor = eigenvalue_ratio * lmax
    lam_c = np.maximum(lam, floor[:, None])
    with np.errstate(divide="ignore", invalid="ignore"):
        A = np.einsum("nik,nk,njk->nij", V, 1.0 / lam_c, V)
    A = 0.5 * (A + A.transpose(0, 2, 1))
    idx = np.nonzero(enough)[0]
    valid[idx] = ok
    info[idx[ok]] = A[ok]
    clamped[idx[ok]] = (lam < floor[:, None]).sum(1)[ok]
    return info, valid, clamped


def build_map(xyz, voxel, min_points_per_voxel=6, eigenvalue_ratio=0.01):
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    means = vg.build_map(xyz, np.zeros((len(xyz), 6), np.float32), voxel)                       # once for the means ...
    base = vg.build_map(xyz, member_products(xyz, means.mean[means.cell_of_point]), voxel)      # ... once with the six channels
    assert np.array_equal(base.cells, means.cells) and np.array_equal(base.cell_of_point, means.cell_of_point)
    info, valid, clamped = information(base.cov6, base.count, min_points_per_voxel, eigenvalue_ratio)
    return NdtMapRef(float(voxel), base.origin, base.cells, base.count, base.mean, base.cov6, info, valid, clamped, base.cell_of_point, base)


def candidate_rows(mp, src, T, neighborhood=7):
    cand = vg.candidate_rows(mp.base, src, T, neighborhood, 1)
    return np.where((cand >= 0) & mp.valid[np.maximum(cand, 0)], cand, -1)


def rows_at(mp, src, T, neighborhood=7):
    """(rows, 2) int32 (i, v), ordered by i, then by offset order"""
    cand = candidate_rows(mp, src, T, neighborhood)
    i, k = np.nonzero(cand >= 0)
    return np.stack([i, cand[i, k]], 1).astype(np.int32)


def score_constants(outlier_ratio=0.55, voxel=1.0):
    p, r = float(outlier_ratio), float(voxel)
    c1 = 10.0 * (1.0 - p)
    c2 = p / (r * r * r)
    d3 = -np.log(c2)
    d1 = -np.log(c1 + c2) - d3
    d2 = -2.0 * np.log((-np.log(c1 * np.exp(-0.5) + c2) - d3) / d1)
    return float(d1), float(d2)


@dataclass
class Linearized:
    JTJ: np.ndarray                # (6, 6)
    JTr: np.ndarray                # (6,)
    score: float
    sum_d2: float
    rows: int
    points_with_rows: int
    mag: dict = field(repr=False, default_factory=dict)      # per sum: the sum of the magnitudes of its terms (one term per row)


def linearize(mp, src, T, rows, outlier_ratio=0.55):
    d1, d2 = score_constants(outlier_ratio, mp.voxel)
    rows = np.asarray(rows).reshape(-1, 2)
    if len(rows) == 0:
        z = dict(JTJ=np.zeros((6, 6)), JTr=np.zeros(6), score=0.0, sum_d2=0.0)
        return Linearized(np.zeros((6, 6)), np.zeros(6), 0.0, 0.0, 0, 0, z)
    q = transform(src, T)[rows[:, 0]]
    delta = q - mp.mean[rows[:, 1]].astype(np.float64)
    A = mp.info[rows[:, 1]]
    Ad = np.einsum("nij,nj->ni", A, delta)
    m = (delta * Ad).sum(1)
    e = np.exp(-d2 * m / 2.0)
    w = -d1 * d2 * e
    J = np.zeros((len(rows), 3, 6))
    x, y, z = q[:, 0], q[:, 1], q[:, 2]
    J[:, 0, 1], J[:, 0, 2], J[:, 1, 0], J[:, 1, 2], J[:, 2, 0], J[:, 2, 1] = z, -y, -z, x, y, -x      # -skew(q)
    J[:, 0, 3] = J[:, 1, 4] = J[:, 2, 5] = 1.0
    H = w[:, None, None] * np.einsum("nki,nkl,nlj->nij", J, A, J)
    g = w[:, None] * np.einsum("nki,nk->ni", J, Ad)
    s = -d1 * e
    dd = (delta * delta).sum(1)
    mag = dict(JTJ=np.abs(H).sum(0), JTr=np.abs(g).sum(0), score=float(np.abs(s).sum()), sum_d2=float(dd.sum()))
    return Linearized(H.sum(0), g.sum(0), float(s.sum()), float(dd.sum()), len(rows), len(np.unique(rows[:, 0])), mag)


def loop(mp, src, T0, neighborhood=7, outlier_ratio=0.55, max_it=30, rel_fitness=1e-6, rel_rmse=1e-6):
    """RegistrationICP's loop; extra["scores"][k] is the score at the pose the k-th update started from"""
    orc = vg._oracle()
    T = np.array(T0, np.float64).reshape(4, 4)
    rows = rows_at(mp, src, T, neighborhood)
    fit, rmse = evaluate(mp, src, T, rows)
    it, converged, history, scores = 0, False, [], []
    while it < max_it:
        U = np.eye(4)
        if len(rows):
            lin = linearize(mp, src, T, rows, outlier_ratio)
            scores.append(lin.score)
            U, _ = orc.solve_update(lin.JTJ, lin.JTr)          # (the identity when the solve fails, as Open3D)
        T = U @ T
        before = (fit, rmse)
        rows = rows_at(mp, src, T, neighborhood)
        fit, rmse = evaluate(mp, src, T, rows)
        it += 1
        history.append((T.copy(), fit, rmse, len(rows)))
        if abs(before[0] - fit) < rel_fitness and abs(before[1] - rmse) < rel_rmse:
            converged = True
            break
    return LoopResult(T, fit, rmse, len(rows), it, converged, rows, history, {"scores": scores})
