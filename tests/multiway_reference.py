"""Numpy float64 restatement of joint multiway registration (include/pcr_hip.h, next to ``pcr_multiway_linearize``): the yardstick of
tests/test_multiway_api.py and tests/test_gpu_multiway.py, and the builder of their fixture.

Rows: q = ((M_r0 x + M_r1 y) + M_r2 z) + M_r3 elementwise (numpy does not fuse), qf = float32(q), the match of qf in the target by the index rule
(tests/neighbor_reference.py: hybrid, max_nn = 1).  Sums: every element of JTJ, JTr and the three statistics together with the sum of the absolute
values of its terms, which is what a comparison of two summation orders is measured against.  The joint system, the gauge, the solve and the loop
are written here on their own (dense, ``np.linalg.solve``), not taken from the package's multiway.py."""
import os

import numpy as np

import neighbor_reference as nr
from pose_solver_reference import vec6_to_pose

P2P, P2PL, GICP = 1, 2, 3              # pcr_estimation_kind
L2, L1, GM = 0, 1, 2                   # pcr_loss_kind
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ------------------------------------------------------------------------------------------------- rows
def transform64(M, pts):
    """q of the rule: float64, every product and sum rounded once, in the stated order."""
    M = np.asarray(M, np.float64)
    p = np.asarray(pts, np.float32).reshape(-1, 3).astype(np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([((M[r, 0] * x + M[r, 1] * y) + M[r, 2] * z) + M[r, 3] for r in range(3)], axis=1)


def matches(M, src, tgt, radius, fast=False):
    """-> (idx (m,) int64, -1 = none; d2 (m,) float64, 0 where none; q (m, 3) float64).  ``fast``: the candidates of a k-d tree, decided by the
    rule's own (d2, index) wherever the candidate list provably holds the answer and by brute force elsewhere -- the same rows (a CPU test
    compares them), for the loops, which search thousands of times."""
    q = transform64(M, src)
    with np.errstate(over="ignore"):
        qf = q.astype(np.float32)
    tgt = np.asarray(tgt, np.float32).reshape(-1, 3)
    if len(qf) == 0 or len(tgt) == 0:
        return np.full(len(qf), -1, np.int64), np.zeros(len(qf)), q
    if not fast:
        idx, d2, _ = nr.hybrid(tgt, qf, radius, 1)
        return idx[:, 0], d2[:, 0], q
    from scipy.spatial import cKDTree
    K = min(4, len(tgt))
    finite = np.isfinite(qf).all(1)
    t64 = tgt.astype(np.float64)
    _, cand = cKDTree(t64).query(np.where(finite[:, None], qf, np.float32(0)).astype(np.float64), k=K)
    cand = cand.reshape(len(qf), K)
    q64 = qf.astype(np.float64)
    d = q64[:, None, 0] - t64[cand, 0]; cd2 = d * d
    d = q64[:, None, 1] - t64[cand, 1]; cd2 += d * d
    d = q64[:, None, 2] - t64[cand, 2]; cd2 += d * d
    order = np.lexsort((cand, cd2), axis=1)
    cand = np.take_along_axis(cand, order, axis=1); cd2 = np.take_along_axis(cd2, order, axis=1)
    idx, d2 = cand[:, 0].astype(np.int64), cd2[:, 0].copy()
    r2 = float(radius) * float(radius)
    # the tree orders by its own d2, a few ulps from the rule's: the list holds the answer when its best is clearly below its last
    sure = (cd2[:, 0] < cd2[:, K - 1] * (1.0 - 1e-9)) if K < len(tgt) else np.ones(len(qf), bool)
    redo = np.nonzero(finite & ~sure)[0]
    if len(redo):
        bi, bd, _ = nr.hybrid(tgt, qf[redo], radius, 1)
        idx[redo], d2[redo] = bi[:, 0], np.where(bi[:, 0] >= 0, bd[:, 0], np.inf)
    none = ~finite | ~(d2 < r2) | (idx < 0)
    idx[none] = -1; d2[none] = 0.0
    return idx, d2, q


def weight(loss, k, r):
    r = np.asarray(r, np.float64)
    if loss == L1:
        return 1.0 / np.maximum(np.abs(r), 1e-300)
    if loss == GM:
        d = k + r * r
        return k / (d * d)
    return np.ones_like(r)


def _unit_or_e1(n):
    n = np.asarray(n, np.float32).astype(np.float64).copy()
    n[n[:, 0] < -0.99] = [1.0, 0.0, 0.0]
    return n / np.sqrt((n * n).sum(1))[:, None]


def _neg_skew(s):
    Z = np.zeros(len(s))
    return np.stack([np.stack([Z, s[:, 2], -s[:, 1]], 1), np.stack([-s[:, 2], Z, s[:, 0]], 1), np.stack([s[:, 1], -s[:, 0], Z], 1)], 1)      # (R, 3, 3) = -skew(s)


def edge_rows(kind, loss, k, eps, M, s, t, src_n, tgt_n):
    """The rows of the matched pairs (s: float64 source points at M, t: float64 target points, the normals of the same pairs as stored):
    (J (R, 6), r (R,), w (R,), pair (R,) = the match a row belongs to)."""
    m = len(s)
    pair = np.arange(m)
    if kind == P2PL:
        n = np.asarray(tgt_n, np.float32).astype(np.float64)
        r = ((s - t) * n).sum(1)
        return np.concatenate([np.cross(s, n), n], axis=1), r, weight(loss, k, r), pair
    if kind == P2P:
        W = np.broadcast_to(np.identity(3), (m, 3, 3))
    else:
        R = np.asarray(M, np.float64)[:3, :3]
        u = _unit_or_e1(src_n) @ R.T
        v = _unit_or_e1(tgt_n)
        a = 1.0 - eps
        C = 2.0 * np.identity(3)[None] - a * (u[:, :, None] * u[:, None, :] + v[:, :, None] * v[:, None, :])      # C_t + R C_s R^T
        lam, V = np.linalg.eigh(C)
        W = np.einsum("nij,nj,nkj->nik", V, 1.0 / np.sqrt(lam), V)
    r = np.einsum("nij,nj->ni", W, s - t)                                    # (m, 3)
    J = np.concatenate([np.einsum("nij,njk->nik", W, _neg_skew(s)), W], axis=2)    # (m, 3, 6)
    w = weight(loss, k, r) if kind == GICP else np.ones_like(r)
    return J.reshape(-1, 6), r.reshape(-1), w.reshape(-1), np.repeat(pair, 3)


def _sum(terms, chunk):
    """sum over axis 0: numpy's own order, or, regrouped, chunk by chunk with the chunk sums added in order"""
    if chunk is None or len(terms) <= chunk:
        return terms.sum(0)
    out = np.zeros(terms.shape[1:])
    for i0 in range(0, len(terms), chunk):
        out = out + terms[i0:i0 + chunk].sum(0)
    return out


def edge_sums(kind, loss, k, eps, M, src, src_n, tgt, tgt_n, radius, chunk=None, fast=False, found=None):
    """One edge at M.  -> dict: JTJ (6, 6), JTr (6,), rows, sum_d2, sum_r2, sum_wr2, match (n_src,), and under "abs" the sums of the absolute
    values of the same terms.  ``found``: what ``matches`` returned for this edge at this M, when the caller already holds it."""
    idx, d2, q = found if found is not None else matches(M, src, tgt, radius, fast)
    has = idx >= 0
    if not has.any():
        zero = dict(JTJ=np.zeros((6, 6)), JTr=np.zeros(6), sum_d2=0.0, sum_r2=0.0, sum_wr2=0.0)
        return dict(zero, rows=0, match=idx, abs=dict(zero))
    s = q[has]
    t = np.asarray(tgt, np.float32).reshape(-1, 3)[idx[has]].astype(np.float64)
    sn = np.asarray(src_n, np.float32).reshape(-1, 3)[has] if src_n is not None else None
    tn = np.asarray(tgt_n, np.float32).reshape(-1, 3)[idx[has]] if tgt_n is not None else None
    J, r, w, _ = edge_rows(kind, loss, k, eps, M, s, t, sn, tn)
    tJ = w[:, None, None] * J[:, :, None] * J[:, None, :]
    tr = (w * r)[:, None] * J
    out = dict(JTJ=_sum(tJ, chunk), JTr=_sum(tr, chunk), rows=int(has.sum()), sum_d2=float(_sum(d2[has], chunk)), sum_r2=float(_sum(r * r, chunk)),
               sum_wr2=float(_sum(w * r * r, chunk)), match=idx)
    out["abs"] = dict(JTJ=np.abs(tJ).sum(0), JTr=np.abs(tr).sum(0), sum_d2=float(d2[has].sum()), sum_r2=float((r * r).sum()), sum_wr2=float((w * r * r).sum()))
    return out


# ------------------------------------------------------------------------------------------------- the joint system
def inv_rigid(T):
    T = np.asarray(T, np.float64)
    out = np.identity(4)
    out[:3, :3] = T[:3, :3].T
    out[:3, 3] = -(T[:3, :3].T @ T[:3, 3])
    return out


def adjoint(T):
    R, t = T[:3, :3], T[:3, 3]
    S = np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])
    return np.block([[R, np.zeros((3, 3))], [S @ R, R]])


def expand(JTJ, JTr, T_b):
    A = adjoint(inv_rigid(T_b))
    return A.T @ JTJ @ A, A.T @ JTr


def free_nodes(n, edges, rows, reference_node):
    """the gauge: the nodes that keep their unknowns"""
    comp = list(range(n))                                      # label = lowest-numbered node of the component, by relabelling until stable
    live = [(int(a), int(b)) for (a, b), r in zip(edges, rows) if r > 0]
    changed = True
    while changed:
        changed = False
        for a, b in live:
            lo = min(comp[a], comp[b])
            if comp[a] != lo or comp[b] != lo:
                comp[a] = comp[b] = lo
                changed = True
    touched = {a for a, _ in live} | {b for _, b in live}
    return [i for i in range(n) if i in touched and i != reference_node and not (comp[i] == i and comp[reference_node] != i)]


def solve_step(poses, edges, sums, reference_node):
    """x (n, 6) of H x = -g, zero rows for the removed nodes; None when the solve fails or is not finite"""
    n = len(poses)
    free = free_nodes(n, edges, [s["rows"] for s in sums], reference_node)
    x = np.zeros((n, 6))
    if not free:
        return x
    H = np.zeros((6 * n, 6 * n)); g = np.zeros(6 * n)
    for (a, b), s in zip(edges, sums):
        if s["rows"] <= 0:
            continue
        a, b = int(a), int(b)
        Hw, gw = expand(s["JTJ"], s["JTr"], poses[b])
        A, B = slice(6 * a, 6 * a + 6), slice(6 * b, 6 * b + 6)
        H[A, A] += Hw; H[B, B] += Hw; H[A, B] -= Hw; H[B, A] -= Hw
        g[A] += gw; g[B] -= gw
    keep = np.concatenate([np.arange(6 * i, 6 * i + 6) for i in free])
    try:
        sol = np.linalg.solve(H[np.ix_(keep, keep)], -g[keep])
    except np.linalg.LinAlgError:
        return None
    if not np.isfinite(sol).all():
        return None
    x.reshape(-1)[keep] = sol
    return x


def linearize(clouds, normals, poses, edges, radius, kind, loss=L2, k=1.0, eps=1e-3, chunk=None, fast=True):
    out = []
    for a, b in edges:
        a, b = int(a), int(b)
        M = inv_rigid(poses[b]) @ poses[a]
        out.append(edge_sums(kind, loss, k, eps, M, clouds[a], normals[a] if normals else None, clouds[b], normals[b] if normals else None, radius, chunk, fast))
    return out


def figures(sums, clouds, edges):
    total = sum(len(clouds[int(a)]) for a, _ in edges)
    rows = sum(s["rows"] for s in sums)
    return (rows / total if total else 0.0), (float(np.sqrt(sum(s["sum_d2"] for s in sums) / rows)) if rows else 0.0)


def loop(clouds, normals, poses, edges, radius, kind, loss=L2, k=1.0, eps=1e-3, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6,
         reference_node=0, chunk=None):
    P = [np.array(T, np.float64) for T in poses]
    sums = linearize(clouds, normals, P, edges, radius, kind, loss, k, eps, chunk)
    fit, rmse = figures(sums, clouds, edges)
    history, iterations, converged = [(fit, rmse)], 0, False
    for _ in range(max_iteration):
        x = solve_step(P, edges, sums, reference_node)
        if x is None:
            break
        P = [vec6_to_pose(x[i]) @ P[i] if x[i].any() else P[i] for i in range(len(P))]
        sums = linearize(clouds, normals, P, edges, radius, kind, loss, k, eps, chunk)
        f2, r2 = figures(sums, clouds, edges)
        iterations += 1
        history.append((f2, r2))
        done = abs(f2 - fit) < relative_fitness and abs(r2 - rmse) < relative_rmse
        fit, rmse = f2, r2
        if done:
            converged = True
            break
    return dict(poses=np.array(P), fitness=fit, inlier_rmse=rmse, iterations=iterations, converged=converged, history=history,
                edge_rows=np.array([s["rows"] for s in sums]))


def pose_distance(A, B):
    """(largest rotation angle [rad], largest translation distance [m]) over two lists of poses"""
    ang = dist = 0.0
    for a, b in zip(A, B):
        ang = max(ang, float(2.0 * np.arcsin(min(1.0, np.linalg.norm(a[:3, :3] - b[:3, :3]) / (2.0 * np.sqrt(2.0))))))
        dist = max(dist, float(np.linalg.norm(a[:3, 3] - b[:3, 3])))
    return ang, dist


# ------------------------------------------------------------------------------------------------- the fixture
def voxel_means(xyz, voxel):
    p = np.asarray(xyz, np.float64)
    cell = np.floor((p - p.min(0)) / voxel).astype(np.int64)
    _, inv, cnt = np.unique(cell, axis=0, return_inverse=True, return_counts=True)
    out = np.zeros((len(cnt), 3))
    np.add.at(out, inv.reshape(-1), p)
    return out / cnt[:, None]


def planted_loop(voxel=0.6, n=4, keep=0.9, noise=0.005, seed=0):
    """n scans of one world (pair 899's target at `voxel`): scan i keeps a random `keep` of the world's points, adds Gaussian noise and is
    expressed in its own frame, planted[i] maps it back.  drifted = the planted chain with an error that grows by the same small motion at
    every step, 2.5e-2 rad / 0.25 m at its far end; node 0 is exact in both.  -> dict(clouds, planted, drifted)."""
    world = voxel_means(np.load(os.path.join(GOLDEN, "nclt_pair_899.npz"))["target"], voxel)
    rng = np.random.default_rng(seed)
    planted, drifted, clouds = [], [], []
    step = vec6_to_pose(np.array([0.3, -0.2, 1.0, 0.0, 0.0, 0.0]) * (2.5e-2 / np.sqrt(1.13) / (n - 1)))
    step[:3, 3] = np.array([0.6, -0.7, 0.4]) * (0.25 / np.sqrt(1.01) / (n - 1))
    D = np.identity(4)
    for i in range(n):
        T = vec6_to_pose(np.array([0.01 * i, -0.015 * i, 0.12 * i, 0.8 * i, -0.5 * i, 0.05 * i]))
        planted.append(T)
        drifted.append(D @ T)
        D = step @ D
        pts = world[rng.random(len(world)) < keep]
        pts = pts + rng.normal(0.0, noise, pts.shape)
        Ti = inv_rigid(T)
        clouds.append((pts @ Ti[:3, :3].T + Ti[:3, 3]).astype(np.float32))
    return dict(clouds=clouds, planted=np.array(planted), drifted=np.array(drifted))


def pca_normals(xyz, k=20):
    """the eigenvector of the smallest eigenvalue of the covariance of the k nearest points (self included), float32; the sign is arbitrary"""
    from scipy.spatial import cKDTree
    p = np.asarray(xyz, np.float64)
    _, nb = cKDTree(p).query(p, k=min(k, len(p)))
    q = p[nb]
    c = q - q.mean(1, keepdims=True)
    _, V = np.linalg.eigh(np.einsum("nki,nkj->nij", c, c))
    return V[:, :, 0].astype(np.float32)
