"""Exact references and exact inputs for the pose solvers' tests (tests/test_gpu_pose_solvers.py, tests/test_pose_solvers_host.py).

``exact_solve6`` solves the 6x6 normal equations of a point-to-plane or GICP update in ``fractions.Fraction``: every input is a float32 or
float64 value, hence a rational number, so the result is THE solution of the system the device only approximates, and its rank is a fact, not
a threshold.  The clouds below are built from small integers and dyadic fractions with axis-aligned normals, so that whole columns of
J = [s x n, n] are exactly zero (or exactly equal) in float64 whatever the order of the sums."""
from fractions import Fraction

import numpy as np


def vec6_to_pose(x):
    """Rz(x2) Ry(x1) Rx(x0) | (x3, x4, x5): the pose of an update vector (oracle/cloud_ops.c:orc_vec6_to_T)."""
    sa, ca, sb, cb, sg, cg = np.sin(x[0]), np.cos(x[0]), np.sin(x[1]), np.cos(x[1]), np.sin(x[2]), np.cos(x[2])
    return np.array([[cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa, x[3]],
                     [sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa, x[4]],
                     [-sb, cb * sa, cb * ca, x[5]],
                     [0.0, 0.0, 0.0, 1.0]])


def exact_solve(A, b):
    """Gauss-Jordan elimination of the square system A x = b in rationals.  Returns (x as a list of Fraction, or None when A is singular; rank)."""
    n = len(b)
    M = [[Fraction(A[i][j]) for j in range(n)] + [Fraction(b[i])] for i in range(n)]
    rank = 0
    for col in range(n):
        piv = next((r for r in range(rank, n) if M[r][col] != 0), None)
        if piv is None:
            continue
        M[rank], M[piv] = M[piv], M[rank]
        p = M[rank][col]
        M[rank] = [v / p for v in M[rank]]
        for r in range(n):
            if r != rank and M[r][col] != 0:
                f = M[r][col]
                M[r] = [v - f * u for v, u in zip(M[r], M[rank])]
        rank += 1
    if rank < n:
        return None, rank
    return [M[i][n] for i in range(n)], rank


def normal_equations(J, w, r):
    """(JTJ, JTr) = (sum w J^T J, sum w J r) in rationals."""
    J = np.asarray(J, np.float64); w = np.asarray(w, np.float64); r = np.asarray(r, np.float64)
    A = [[Fraction(0)] * 6 for _ in range(6)]
    b = [Fraction(0)] * 6
    for row, wi, ri in zip(J.tolist(), w.tolist(), r.tolist()):
        fr = [Fraction(v) for v in row]
        fw = Fraction(wi)
        for p in range(6):
            if fr[p] == 0:
                continue
            wj = fw * fr[p]
            for q in range(p, 6):
                A[p][q] += wj * fr[q]
            b[p] += wj * Fraction(ri)
    for p in range(6):
        for q in range(p):
            A[p][q] = A[q][p]
    return A, b


def exact_solve6(J, w, r):
    """JTJ x = -JTr with JTJ = sum w J^T J and JTr = sum w J r, solved exactly.  Returns (x float64[6] or None, rank, 4x4 pose): the pose is
    Rz Ry Rx | t of the correctly rounded x, the identity when the system is singular."""
    A, b = normal_equations(J, w, r)
    x, rank = exact_solve(A, [-v for v in b])
    if x is None:
        return None, rank, np.eye(4)
    x = np.array([float(v) for v in x])
    return x, rank, vec6_to_pose(x)


def plane_rows(src, tgt, normals, corres):
    """(J, r) of the point-to-plane rows over a list: r = (s - t).n, J = [s x n, n], float64 on the stored values."""
    corres = np.asarray(corres, np.int64).reshape(-1, 2)
    s = np.asarray(src, np.float64)[corres[:, 0]]; t = np.asarray(tgt, np.float64)[corres[:, 1]]; n = np.asarray(normals, np.float64)[corres[:, 1]]
    return np.concatenate([np.cross(s, n), n], axis=1), ((s - t) * n).sum(1)


def exact_update(JTJ, JTr):
    """JTJ x = -JTr of a system given as float64 sums (the GICP system of the oracle's ``gicp_linearize``), solved exactly: (x, rank, pose)."""
    A = np.asarray(JTJ, np.float64).reshape(6, 6)
    x, rank = exact_solve(A.tolist(), [-v for v in np.asarray(JTr, np.float64).tolist()])
    if x is None:
        return None, rank, np.eye(4)
    x = np.array([float(v) for v in x])
    return x, rank, vec6_to_pose(x)


# ---------------------------------------------------------------------------------------------- exact clouds
def identity_rows(n):
    return np.stack([np.arange(n), np.arange(n)], axis=1).astype(np.int32)


def floor(lift=0.25, side=20):
    """side x side integer grid in z = 0, normals (0, 0, 1), the target lifted by `lift`: J = [y, -x, 0, 0, 0, 1], rank 3."""
    g = np.stack(np.meshgrid(np.arange(float(side)), np.arange(float(side)), indexing="ij"), axis=-1).reshape(-1, 2)
    src = np.concatenate([g, np.zeros((len(g), 1))], axis=1)
    nrm = np.tile([0.0, 0.0, 1.0], (len(g), 1))
    return src, src + lift * nrm, nrm


def corridor(lift=0.25):
    """Two 20 x 20 integer grids, in z = 0 (normal e3) and in x = 0 (normal e1), the target moved by `lift` along the normals: the rows
    [y, -x, 0, 0, 0, 1] and [0, z, -y, 1, 0, 0] leave the column of t_y exactly zero, rank 5.  800 points."""
    g = np.stack(np.meshgrid(np.arange(1.0, 21.0), np.arange(1.0, 21.0), indexing="ij"), axis=-1).reshape(-1, 2)
    a = np.concatenate([g, np.zeros((400, 1))], axis=1)                      # (x, y, 0), x, y in 1..20
    b = np.concatenate([np.zeros((400, 1)), g], axis=1)                      # (0, y, z), y, z in 1..20
    src = np.concatenate([a, b])
    nrm = np.concatenate([np.tile([0.0, 0.0, 1.0], (400, 1)), np.tile([1.0, 0.0, 0.0], (400, 1))])
    return src, src + lift * nrm, nrm


def sphere():
    """Every integer point with x^2 + y^2 + z^2 = 81 (102 of them), n = s exactly and t = 1.0078125 s: s x n = 0, J = [0, 0, 0, n], rank 3."""
    r = np.arange(-9, 10)
    g = np.stack(np.meshgrid(r, r, r, indexing="ij"), axis=-1).reshape(-1, 3)
    src = g[(g * g).sum(1) == 81].astype(np.float64)
    return src, 1.0078125 * src, src.copy()


def assert_exact_columns(J, zero=(), equal=()):
    """the property the singular cases rest on, asserted on the test's own float64 rows: the named columns of J are exactly zero, the named
    pairs of columns exactly equal"""
    J = np.asarray(J, np.float64)
    for c in zero:
        assert (J[:, c] == 0.0).all(), c
    for a, b in equal:
        assert (J[:, a] == J[:, b]).all(), (a, b)
