"""Joint multiway registration of a set of scans (Lu and Milios 1997; Borrmann et al., RAS 2008 -- PCL's ``registration::LUM``): all scans of
a graph in one least-squares problem whose correspondences are searched again at the current poses of every iteration, the last stage after
``posegraph.pose_graph_from_odometry`` and ``posegraph.global_optimization``, which only ever see relative poses.  The rule -- the rows of an
edge, its sums, the joint system, the gauge, the loop -- is stated in include/pcr_hip.h next to ``pcr_multiway_linearize``.  The device
(csrc/pcr_multiway.hip) searches, linearises and reduces a whole edge list in one call; the assembly and the solve below are host float64.
Neither Open3D nor the reference has a counterpart (the reference's "LUM", ``refinement.py``, works on poses alone).
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from .geometry import PointCloud, _dev_f32, _ptr, _torch

DENSE_MAX_NODES = 200          # free nodes up to which the joint system is solved dense (1200 unknowns); scipy.sparse beyond


# ------------------------------------------------------------------------------------------------- pose algebra
def vector_to_pose(x) -> np.ndarray:
    """Open3D's ``TransformVector6dToMatrix4d``: ``Rz(x2) Ry(x1) Rx(x0)``, then the translation ``x[3:6]``."""
    sa, ca, sb, cb, sg, cg = math.sin(x[0]), math.cos(x[0]), math.sin(x[1]), math.cos(x[1]), math.sin(x[2]), math.cos(x[2])
    return np.array([[cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa, x[3]],
                     [sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa, x[4]],
                     [-sb, cb * sa, cb * ca, x[5]],
                     [0.0, 0.0, 0.0, 1.0]], dtype=np.float64)


def rigid_inverse(T) -> np.ndarray:
    """``(R^T, -R^T t)`` of a rigid 4x4 pose."""
    T = np.asarray(T, dtype=np.float64)
    out = np.identity(4)
    out[:3, :3] = T[:3, :3].T
    out[:3, 3] = -(T[:3, :3].T @ T[:3, 3])
    return out


def _skew(t):
    return np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])


def adjoint(T) -> np.ndarray:
    """``Ad(T)`` for unknowns ordered (rotation, translation): ``[[R, 0], [skew(t) R, R]]``."""
    R, t = np.asarray(T, np.float64)[:3, :3], np.asarray(T, np.float64)[:3, 3]
    A = np.zeros((6, 6))
    A[:3, :3] = R
    A[3:, 3:] = R
    A[3:, :3] = _skew(t) @ R
    return A


def expand_edge(JTJ, JTr, T_b):
    """An edge's sums, taken in the frame of its target b, as its contribution to the joint system: ``(H_w, g_w) = (A^T JTJ A, A^T JTr)`` with
    ``A = Ad(inv(T_b))``.  ``H_w`` goes to the blocks (a, a) and (b, b) and, negated, to (a, b) and (b, a); ``g_w`` to ``g_a`` and, negated, to
    ``g_b``."""
    A = adjoint(rigid_inverse(T_b))
    return A.T @ np.asarray(JTJ, np.float64).reshape(6, 6) @ A, A.T @ np.asarray(JTr, np.float64).reshape(6)


def circuit_edges(n: int, both_directions: bool = True) -> np.ndarray:
    """The edges of a closed circuit of ``n`` scans: ``(i, (i + 1) % n)`` for every i and, with ``both_directions``, the reverse of each right
    after it.  (E, 2) int32.  Two scans give the one pair, once per direction."""
    if int(n) != n or int(n) < 2:
        raise ValueError(f"circuit_edges: n must be an integer >= 2, got {n!r}")
    n = int(n)
    out = []
    for i in range(n if n > 2 else 1):
        j = (i + 1) % n
        out.append((i, j))
        if both_directions:
            out.append((j, i))
    return np.array(out, dtype=np.int32).reshape(-1, 2)


# ------------------------------------------------------------------------------------------------- argument checks (no device is touched)
def _check_edges(fn: str, edges, n_clouds: int) -> np.ndarray:
    e = np.asarray(edges)
    if e.size == 0:
        return np.zeros((0, 2), np.int32)
    if e.ndim != 2 or e.shape[1] != 2 or not np.issubdtype(e.dtype, np.integer):
        raise ValueError(f"{fn}: edges must be (E, 2) integer rows (source cloud, target cloud), got shape {e.shape} of {e.dtype}")
    if e.min() < 0 or e.max() >= n_clouds:
        raise ValueError(f"{fn}: edges name a cloud outside 0..{n_clouds - 1}")
    if (e[:, 0] == e[:, 1]).any():
        raise ValueError(f"{fn}: edges join a cloud to itself (row {int(np.nonzero(e[:, 0] == e[:, 1])[0][0])})")
    return np.ascontiguousarray(e, dtype=np.int32)


def _check_distance(fn: str, max_correspondence_distance) -> float:
    try:
        r = float(max_correspondence_distance)
    except (TypeError, ValueError):
        raise ValueError(f"{fn}: max_correspondence_distance must be a number, got {max_correspondence_distance!r}") from None
    if not (math.isfinite(r) and r > 0.0):
        raise ValueError(f"{fn}: max_correspondence_distance must be finite and > 0, got {max_correspondence_distance!r}")
    return r


def _check_poses(fn: str, poses, count: int, what: str = "poses") -> np.ndarray:
    try:
        P = np.array([np.asarray(T, dtype=np.float64) for T in poses], dtype=np.float64)
        if P.size == 0:
            P = P.reshape(0, 4, 4)
    except (TypeError, ValueError):
        raise ValueError(f"{fn}: {what} must be {count} matrices of shape (4, 4)") from None
    if P.shape != (count, 4, 4):
        raise ValueError(f"{fn}: {what} must be {count} matrices of shape (4, 4), got shape {P.shape}")
    if not np.isfinite(P).all():
        raise ValueError(f"{fn}: {what} hold a non-finite entry")
    return P


def _check_estimation(fn: str, estimation_method):
    from .registration import (TransformationEstimationForGeneralizedICP, TransformationEstimationPointToPlane, TransformationEstimationPointToPoint)
    if estimation_method is None:
        estimation_method = TransformationEstimationPointToPlane()
    if not isinstance(estimation_method, (TransformationEstimationPointToPoint, TransformationEstimationPointToPlane, TransformationEstimationForGeneralizedICP)):
        raise ValueError(f"{fn}: estimation_method must be a point-to-point, point-to-plane or generalized ICP estimation, got {type(estimation_method).__name__}")
    if getattr(estimation_method, "with_scaling", False):
        raise ValueError(f"{fn}: estimation_method with_scaling has no joint form")
    return estimation_method


def _needs_normals(estimation_method):
    """(source needs normals, target needs normals)"""
    kind = estimation_method._estimation().kind
    return kind == _lib.EST_GENERALIZED_ICP, kind != _lib.EST_POINT_TO_POINT


def _check_reference(fn: str, reference_node, n: int) -> int:
    if int(reference_node) != reference_node or not 0 <= int(reference_node) < n:
        raise ValueError(f"{fn}: reference_node must be a node in 0..{n - 1}, got {reference_node!r}")
    return int(reference_node)


# ------------------------------------------------------------------------------------------------- the problem on the device
class MultiwayProblem:
    """The clouds of a multiway registration on the device: per cloud a search index and, where the cloud carries them, its normals, in device
    memory of the problem's own until ``close()``.  A context manager like ``VoxelCovarianceMap``.  ``clouds`` holds ``PointCloud`` objects (with
    or without normals) or (n, 3) arrays; an empty cloud is valid.

        with MultiwayProblem(scans) as problem:
            lin = problem.linearize(poses, circuit_edges(len(scans)), 0.5)
            result = multiway_registration(problem, poses, circuit_edges(len(scans)), 0.5)
    """

    _handle = None

    def __init__(self, clouds):
        fn = "MultiwayProblem"
        clouds = list(clouds)
        for k, c in enumerate(clouds):
            if not isinstance(c, PointCloud):
                shape = tuple(c.shape) if hasattr(c, "shape") else np.asarray(c).shape
                if len(shape) != 2 or shape[1] != 3:
                    raise ValueError(f"{fn}: cloud {k} must be a PointCloud or an (n, 3) array, got shape {shape}")
        xyz, nrm = [], []
        for c in clouds:
            if isinstance(c, PointCloud):
                xyz.append(c.device_xyz())
                nrm.append(c.device_normals() if c.has_normals() else None)
            else:
                xyz.append(_dev_f32(c, 3))
                nrm.append(None)
        self.sizes = [int(t.shape[0]) for t in xyz]
        self.has_normals = [t is not None for t in nrm]
        m = len(xyz)
        ctx = _lib.Context.current()
        h = C.c_void_p()
        px = (C.c_void_p * max(m, 1))(*[t.data_ptr() if t.shape[0] else None for t in xyz])
        pn = (C.c_void_p * max(m, 1))(*[t.data_ptr() if t is not None else None for t in nrm])
        cnt = (C.c_int64 * max(m, 1))(*self.sizes)
        ctx.check(ctx.lib.pcr_multiway_create(ctx.handle, C.c_int(m), px, pn, cnt, C.byref(h)), fn)
        self._handle = h
        self._lib = ctx.lib

    def __len__(self):
        return len(self.sizes)

    def close(self):
        """Destroy the problem (waits for the device)."""
        h, self._handle = self._handle, None
        if h is not None and h.value:
            self._lib.pcr_multiway_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def _open(self):
        if self._handle is None:
            raise RuntimeError("MultiwayProblem: the problem is closed")
        return self._handle

    def linearize(self, poses_or_M, edges, max_correspondence_distance, estimation_method=None, return_matches: bool = False, per_edge: bool = False):
        """One linearisation of every edge (``pcr_multiway_linearize``).  ``poses_or_M``: the node poses, one 4x4 per cloud -- edge (a, b) is
        then taken at ``M = rigid_inverse(T_b) @ T_a`` --, or, with ``per_edge``, one 4x4 ``M`` per edge as it stands.  Returns a dict of
        float64 / int64 numpy arrays ``JTJ`` (E, 6, 6), ``JTr`` (E, 6), ``rows`` (E,), ``sum_d2``, ``sum_r2``, ``sum_wr2`` (E,) and ``M``
        (E, 4, 4); with ``return_matches`` also ``matches``: per edge an int32 device tensor with, for every point of the source in caller
        order, the matched row of the target or -1."""
        fn = "MultiwayProblem.linearize"
        h = self._open()
        return _linearize(fn, self, h, poses_or_M, edges, max_correspondence_distance, estimation_method, return_matches, per_edge)


def _edge_poses(P, edges):
    M = np.empty((len(edges), 4, 4))
    for k, (a, b) in enumerate(edges):
        M[k] = rigid_inverse(P[b]) @ P[a]
    return M


def _linearize(fn, problem, handle, poses_or_M, edges, max_correspondence_distance, estimation_method, return_matches, per_edge):
    edges = _check_edges(fn, edges, len(problem.sizes))
    r = _check_distance(fn, max_correspondence_distance)
    est = _check_estimation(fn, estimation_method)
    E = len(edges)
    if per_edge:
        M = _check_poses(fn, poses_or_M, E, "the per-edge poses M")
    else:
        M = _edge_poses(_check_poses(fn, poses_or_M, len(problem.sizes)), edges)
    need_s, need_t = _needs_normals(est)
    for k, (a, b) in enumerate(edges):
        for c, need in ((a, need_s), (b, need_t)):
            if need and problem.sizes[c] > 0 and not problem.has_normals[c]:
                raise ValueError(f"{fn}: the estimator needs the normals of cloud {int(c)}, which carries none (edge {k})")
    JTJ, JTr, stats, rows = np.zeros((E, 6, 6)), np.zeros((E, 6)), np.zeros((E, 3)), np.zeros(E, np.int64)
    out = dict(JTJ=JTJ, JTr=JTr, rows=rows, M=M)
    matches = None
    if E:
        torch = _torch()
        counts = [problem.sizes[a] for a, _ in edges]
        flat = torch.empty((max(sum(counts), 1),), dtype=torch.int32, device="cuda") if return_matches else None
        pe = est._estimation()
        Mc = np.ascontiguousarray(M, dtype=np.float64)
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        ctx = _lib.Context.current()
        ctx.check(ctx.lib.pcr_multiway_linearize(ctx.handle, handle, edges.ctypes.data_as(C.c_void_p), C.c_int64(E), dp(Mc), C.c_double(r), C.byref(pe),
                                                 dp(JTJ), dp(JTr), dp(stats), rows.ctypes.data_as(C.POINTER(C.c_int64)), _ptr(flat)), fn)
        if return_matches:
            offs = np.concatenate([[0], np.cumsum(counts)])
            matches = [flat[int(offs[k]):int(offs[k + 1])] for k in range(E)]
    elif return_matches:
        matches = []
    out.update(sum_d2=stats[:, 0].copy(), sum_r2=stats[:, 1].copy(), sum_wr2=stats[:, 2].copy())
    if return_matches:
        out["matches"] = matches
    return out


# ------------------------------------------------------------------------------------------------- the joint system and the loop (host)
class MultiwayResult:
    """``poses`` (n, 4, 4) float64; ``fitness`` = matched source points over all source points of the edges; ``inlier_rmse`` = the root mean
    square of the matches' distances; ``iterations`` = updates made; ``converged``; ``edge_rows`` and ``edge_rmse`` per edge at the end poses;
    ``history`` = (fitness, inlier_rmse) at the given poses and after every update."""

    def __init__(self, poses, fitness, inlier_rmse, iterations, converged, edge_rows, edge_rmse, history):
        self.poses, self.fitness, self.inlier_rmse = poses, float(fitness), float(inlier_rmse)
        self.iterations, self.converged = int(iterations), bool(converged)
        self.edge_rows, self.edge_rmse, self.history = edge_rows, edge_rmse, history

    def __repr__(self):
        return (f"MultiwayResult with {len(self.poses)} poses, fitness={self.fitness:.6e}, inlier_rmse={self.inlier_rmse:.6e}, "
                f"iterations={self.iterations}, converged={self.converged}")


def gauge_nodes(n: int, edges, rows, reference_node: int):
    """The nodes whose unknowns stay in the joint system (ascending), by the three gauge rules: not the reference node, not a node touched by no
    edge with rows > 0, not the lowest-numbered node of a connected component (over those edges) that does not hold the reference node."""
    parent = list(range(n))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i
    touched = [False] * n
    for (a, b), r in zip(edges, rows):
        if r > 0:
            touched[a] = touched[b] = True
            ra, rb = find(int(a)), find(int(b))
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)          # the root of a component is its lowest-numbered node
    ref_root = find(reference_node)
    return [i for i in range(n) if touched[i] and i != reference_node and not (find(i) == i and find(i) != ref_root)]


def joint_step(poses, edges, lin, reference_node: int):
    """Assemble ``H x = -g`` from the edges' sums and solve it: the (n, 6) update vectors, zero for the nodes the gauge removes, or ``None``
    when the solve fails or its result is not finite."""
    n = len(poses)
    free = gauge_nodes(n, edges, lin["rows"], reference_node)
    x = np.zeros((n, 6))
    if not free:
        return x
    slot = {node: k for k, node in enumerate(free)}
    blocks, g = {}, np.zeros(6 * len(free))
    for k, (a, b) in enumerate(edges):
        if lin["rows"][k] <= 0:
            continue
        a, b = int(a), int(b)
        Hw, gw = expand_edge(lin["JTJ"][k], lin["JTr"][k], poses[b])
        for i, j, sgn in ((a, a, 1.0), (b, b, 1.0), (a, b, -1.0), (b, a, -1.0)):
            if i in slot and j in slot:
                key = (slot[i], slot[j])
                blocks[key] = blocks[key] + sgn * Hw if key in blocks else sgn * Hw
        if a in slot:
            g[6 * slot[a]:6 * slot[a] + 6] += gw
        if b in slot:
            g[6 * slot[b]:6 * slot[b] + 6] -= gw
    m = len(free)
    try:
        if m <= DENSE_MAX_NODES:
            H = np.zeros((6 * m, 6 * m))
            for (i, j), B in blocks.items():
                H[6 * i:6 * i + 6, 6 * j:6 * j + 6] = B
            sol = np.linalg.solve(H, -g)
        else:
            import warnings
            import scipy.sparse as sp
            import scipy.sparse.linalg as spl
            keys = list(blocks)
            six = np.arange(6)
            H = sp.coo_matrix((np.concatenate([blocks[k].ravel() for k in keys]),
                               (np.concatenate([np.repeat(six + 6 * k[0], 6) for k in keys]), np.concatenate([np.tile(six + 6 * k[1], 6) for k in keys]))),
                              shape=(6 * m, 6 * m)).tocsc()
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                sol = spl.spsolve(H, -g)
    except (np.linalg.LinAlgError, RuntimeError):
        return None
    if not np.isfinite(sol).all():
        return None
    for node, k in slot.items():
        x[node] = sol[6 * k:6 * k + 6]
    return x


def _figures(lin, sizes, edges):
    total = sum(sizes[int(a)] for a, _ in edges)
    rows = int(np.sum(lin["rows"]))
    fitness = rows / total if total else 0.0
    rmse = math.sqrt(float(np.sum(lin["sum_d2"])) / rows) if rows else 0.0
    return fitness, rmse


def multiway_registration(clouds_or_problem, poses, edges, max_correspondence_distance, estimation_method=None, criteria=None, reference_node: int = 0):
    """Register all clouds jointly: starting from the node ``poses`` (one 4x4 per cloud, cloud -> common frame), every iteration searches the
    correspondences of every edge (source cloud, target cloud) again at the current poses on the device, and one Gauss-Newton step of the joint
    system moves all poses but that of ``reference_node``.  ``clouds_or_problem``: a list of clouds (a ``MultiwayProblem`` is made and closed
    here) or an open ``MultiwayProblem``.  ``estimation_method``: ``TransformationEstimationPointToPlane()`` by default (the targets need
    normals), point-to-point or generalized ICP (both clouds of an edge need normals); ``criteria``: ``ICPConvergenceCriteria()``.  Returns a
    ``MultiwayResult``."""
    from .registration import ICPConvergenceCriteria
    fn = "multiway_registration"
    own = not hasattr(clouds_or_problem, "linearize")
    n = len(clouds_or_problem) if own else len(clouds_or_problem.sizes)
    P = _check_poses(fn, poses, n)
    edges = _check_edges(fn, edges, n)
    _check_distance(fn, max_correspondence_distance)
    est = _check_estimation(fn, estimation_method)
    if n == 0:
        raise ValueError(f"{fn}: no clouds")
    ref = _check_reference(fn, reference_node, n)
    criteria = criteria or ICPConvergenceCriteria()
    problem = MultiwayProblem(clouds_or_problem) if own else clouds_or_problem
    try:
        lin = problem.linearize(P, edges, max_correspondence_distance, est)
        fitness, rmse = _figures(lin, problem.sizes, edges)
        history = [(fitness, rmse)]
        iterations, converged = 0, False
        for _ in range(int(criteria.max_iteration)):
            x = joint_step(P, edges, lin, ref)
            if x is None:
                break
            P = np.array([vector_to_pose(x[i]) @ P[i] if x[i].any() else P[i] for i in range(n)])
            lin = problem.linearize(P, edges, max_correspondence_distance, est)
            f2, r2 = _figures(lin, problem.sizes, edges)
            iterations += 1
            history.append((f2, r2))
            done = abs(f2 - fitness) < criteria.relative_fitness and abs(r2 - rmse) < criteria.relative_rmse
            fitness, rmse = f2, r2
            if done:
                converged = True
                break
    finally:
        if own:
            problem.close()
    rows = np.asarray(lin["rows"], np.int64).copy()
    edge_rmse = np.sqrt(np.divide(lin["sum_d2"], rows, out=np.zeros(len(rows)), where=rows > 0))
    return MultiwayResult(P, fitness, rmse, iterations, converged, rows, edge_rmse, history)
