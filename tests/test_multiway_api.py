"""CPU-side checks of joint multiway registration: the expansion of an edge's sums into the joint system against a finite-difference Jacobian, the
three gauge rules and a failed solve with stubbed linearisations, the helpers, the argument checks of the Python layer, the ABI of the entry
points, and -- with the numpy restatement alone (tests/multiway_reference.py) -- the conditions the GPU comparisons rest on.  Needs no GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import multiway_reference as mr
from conftest import ROOT, pkg
from pose_solver_reference import vec6_to_pose

EDGES8 = [(0, 1), (1, 0), (1, 2), (2, 1), (2, 3), (3, 2), (3, 0), (0, 3)]


@pytest.fixture(scope="module")
def loop4():
    f = mr.planted_loop()
    f["normals"] = [mr.pca_normals(c) for c in f["clouds"]]
    return f


# ------------------------------------------------------------------------------------------------- the expansion
def test_expansion_matches_a_finite_difference_jacobian_in_both_poses():
    """Fixed point-to-plane pairs between two clouds at poses T_a, T_b: the residuals as a function of the updates (x_a, x_b) of
    T <- V(x) T have the Jacobian [J A, -J A] at 0, so H_w = A^T JTJ A and g_w = A^T JTr are what the edge adds to the joint system."""
    P = pkg()
    rng = np.random.default_rng(5)
    pa = rng.uniform(-5, 5, (40, 3)); pb = rng.uniform(-5, 5, (40, 3))
    nb = rng.normal(size=(40, 3)); nb /= np.linalg.norm(nb, axis=1)[:, None]
    Ta = vec6_to_pose(np.array([0.3, -0.2, 0.5, 1.0, -2.0, 0.5])); Tb = vec6_to_pose(np.array([-0.4, 0.1, 1.2, -3.0, 0.7, 2.0]))

    def residuals(xa, xb):
        M = mr.inv_rigid(vec6_to_pose(xb) @ Tb) @ (vec6_to_pose(xa) @ Ta)
        s = pa @ M[:3, :3].T + M[:3, 3]
        return ((s - pb) * nb).sum(1)
    M = mr.inv_rigid(Tb) @ Ta
    s = pa @ M[:3, :3].T + M[:3, 3]
    J = np.concatenate([np.cross(s, nb), nb], axis=1)
    r0 = residuals(np.zeros(6), np.zeros(6))
    h = 1e-6
    Ja = np.stack([(residuals(h * e, np.zeros(6)) - residuals(-h * e, np.zeros(6))) / (2 * h) for e in np.identity(6)], axis=1)
    Jb = np.stack([(residuals(np.zeros(6), h * e) - residuals(np.zeros(6), -h * e)) / (2 * h) for e in np.identity(6)], axis=1)
    for expand in (P.multiway.expand_edge, mr.expand):
        Hw, gw = expand(J.T @ J, J.T @ r0, Tb)
        scale = np.abs(Hw).max()
        assert np.abs(Hw - Ja.T @ Ja).max() < 1e-6 * scale and np.abs(Hw - Jb.T @ Jb).max() < 1e-6 * scale
        assert np.abs(-Hw - Ja.T @ Jb).max() < 1e-6 * scale
        assert np.abs(gw - Ja.T @ r0).max() < 1e-6 * np.abs(gw).max() and np.abs(-gw - Jb.T @ r0).max() < 1e-6 * np.abs(gw).max()
    assert P.expand_edge is P.multiway.expand_edge
    A = P.multiway.adjoint(Tb)
    assert np.allclose(A, mr.adjoint(Tb)) and np.allclose(P.multiway.rigid_inverse(Tb) @ Tb, np.identity(4), atol=1e-14)
    x = np.array([0.1, -0.2, 0.3, 1.0, 2.0, 3.0])
    assert np.array_equal(P.multiway.vector_to_pose(x), vec6_to_pose(x))


# ------------------------------------------------------------------------------------------------- gauge, solve and loop with stubs
class _Stub:
    """a problem in place of the device: every cloud is the same 12 points and point i of the source is matched to point i of the target, so an
    edge's sums are the point-to-point rows of these pairs at M (a true Gauss-Newton problem whose solution is M = identity); `rows[k]` is what
    the stub reports as the edge's row count, 0 = the edge found nothing; `singular` zeroes every JTJ"""
    PTS = np.random.default_rng(11).uniform(-1.0, 1.0, (12, 3))

    def __init__(self, sizes, rows, singular=False):
        self.sizes, self.rows, self.singular, self.calls = list(sizes), rows, singular, 0

    def linearize(self, poses, edges, max_correspondence_distance, estimation_method=None):
        self.calls += 1
        E = len(edges)
        JTJ = np.zeros((E, 6, 6)); JTr = np.zeros((E, 6)); d2 = np.zeros(E)
        for k, (a, b) in enumerate(edges):
            if self.rows[k] <= 0:
                continue
            M = mr.inv_rigid(poses[b]) @ poses[a]
            s = self.PTS @ M[:3, :3].T + M[:3, 3]
            J = np.concatenate([mr._neg_skew(s), np.broadcast_to(np.identity(3), (len(s), 3, 3))], axis=2).reshape(-1, 6)
            r = (s - self.PTS).reshape(-1)
            JTJ[k] = 0.0 if self.singular else J.T @ J
            JTr[k] = J.T @ r
            d2[k] = float(r @ r)
        return dict(JTJ=JTJ, JTr=JTr, rows=np.asarray(self.rows, np.int64), sum_d2=d2, sum_r2=d2.copy(), sum_wr2=d2.copy())


def _shifted(n, amount=0.1):
    out = []
    for i in range(n):
        T = np.identity(4); T[0, 3] = amount * i * i
        out.append(T)
    return out


def test_reference_node_and_untouched_node_keep_their_poses_bit_for_bit():
    P = pkg()
    poses = _shifted(5)
    poses[2] = vec6_to_pose(np.array([0.1, 0.2, 0.3, 0.123456789, 1 / 3, 2 / 3]))
    edges = [(0, 1), (1, 0), (1, 2), (2, 1), (2, 0)]          # node 3 and node 4 have no edge at all
    stub = _Stub([10] * 5, [10, 10, 10, 10, 10])
    for ref in (0, 2):
        res = P.multiway_registration(stub, poses, edges, 1.0, reference_node=ref)
        assert np.array_equal(res.poses[ref].view(np.int64), np.asarray(poses[ref]).view(np.int64))
        for i in (3, 4):
            assert np.array_equal(res.poses[i].view(np.int64), np.asarray(poses[i]).view(np.int64))
        moved = [i for i in range(5) if not np.array_equal(res.poses[i], poses[i])]
        assert moved == [i for i in (0, 1, 2) if i != ref]
        assert res.iterations >= 1 and res.history[-1][1] < 1e-3 * res.history[0][1]
    assert P.multiway.gauge_nodes(5, edges, [10] * 5, 0) == [1, 2] == mr.free_nodes(5, edges, [10] * 5, 0)
    # an edge without rows does not touch its nodes
    assert P.multiway.gauge_nodes(5, edges + [(3, 4)], [10] * 5 + [0], 0) == [1, 2] == mr.free_nodes(5, edges + [(3, 4)], [10] * 5 + [0], 0)


def test_a_component_without_the_reference_node_loses_its_lowest_node():
    P = pkg()
    edges = [(0, 1), (4, 2), (2, 5), (5, 4), (3, 6)]
    rows = [5, 5, 5, 5, 5]
    assert P.multiway.gauge_nodes(7, edges, rows, 0) == [1, 4, 5, 6] == mr.free_nodes(7, edges, rows, 0)
    assert P.multiway.gauge_nodes(7, edges, rows, 5) == [1, 2, 4, 6] == mr.free_nodes(7, edges, rows, 5)
    assert P.multiway.gauge_nodes(7, edges, [5, 5, 0, 0, 5], 0) == [1, 4, 6] == mr.free_nodes(7, edges, [5, 5, 0, 0, 5], 0)
    poses = _shifted(7)
    res = P.multiway_registration(_Stub([10] * 7, rows), poses, edges, 1.0, criteria=P.registration.ICPConvergenceCriteria(1e-13, 1e-13, 30))
    for i in (0, 2, 3):
        assert np.array_equal(res.poses[i].view(np.int64), np.asarray(poses[i]).view(np.int64))
    for i in (1, 4, 5, 6):
        assert not np.array_equal(res.poses[i], poses[i])
    # the components come to rest on their fixed nodes: every edge's residual translation vanishes
    for a, b in edges:
        assert np.abs((np.linalg.inv(res.poses[b]) @ res.poses[a])[:3, 3]).max() < 1e-9


def test_a_failed_solve_ends_the_loop_at_the_last_completed_step():
    P = pkg()
    poses = _shifted(3)
    stub = _Stub([10] * 3, [10, 10], singular=True)
    res = P.multiway_registration(stub, poses, [(0, 1), (1, 2)], 1.0)
    assert res.converged is False and res.iterations == 0 and stub.calls == 1 and len(res.history) == 1
    assert np.array_equal(res.poses, np.array(poses))
    assert P.multiway.joint_step(np.array(poses), [(0, 1), (1, 2)], stub.linearize(poses, [(0, 1), (1, 2)], 1.0), 0) is None
    lin = stub.linearize(poses, [(0, 1), (1, 2)], 1.0)
    lin["JTJ"][:] = np.identity(6); lin["JTr"][0, 0] = np.nan
    assert P.multiway.joint_step(np.array(poses), [(0, 1), (1, 2)], lin, 0) is None
    sums = [dict(JTJ=np.zeros((6, 6)), JTr=np.ones(6), rows=3)] * 2
    assert mr.solve_step(poses, [(0, 1), (1, 2)], sums, 0) is None
    # nothing to solve is a step that changes nothing: the loop converges at once
    res = P.multiway_registration(_Stub([10] * 3, [0, 0]), poses, [(0, 1), (1, 2)], 1.0)
    assert res.converged and res.iterations == 1 and np.array_equal(res.poses, np.array(poses)) and res.fitness == 0.0 and res.inlier_rmse == 0.0


def test_sparse_and_dense_solves_agree(monkeypatch):
    P = pkg()
    n = 12
    poses = _shifted(n, 0.01)
    edges = [(i, (i + 1) % n) for i in range(n)]
    stub = _Stub([10] * n, [10] * n)
    lin = stub.linearize(poses, edges, 1.0)
    dense = P.multiway.joint_step(np.array(poses), edges, lin, 0)
    monkeypatch.setattr(P.multiway, "DENSE_MAX_NODES", 4)
    sparse = P.multiway.joint_step(np.array(poses), edges, lin, 0)
    assert np.abs(dense - sparse).max() < 1e-12 * max(1.0, np.abs(dense).max()) and np.abs(dense).max() > 0


def test_circuit_edges():
    P = pkg()
    e = P.circuit_edges(4)
    assert e.dtype == np.int32 and e.tolist() == [list(x) for x in EDGES8]
    assert P.circuit_edges(4, both_directions=False).tolist() == [[0, 1], [1, 2], [2, 3], [3, 0]]
    assert P.circuit_edges(2).tolist() == [[0, 1], [1, 0]] and P.circuit_edges(2, False).tolist() == [[0, 1]]
    assert P.circuit_edges(3).shape == (6, 2)
    for bad in (1, 0, -3, 2.5):
        with pytest.raises(ValueError, match="circuit_edges"):
            P.circuit_edges(bad)
    assert P.circuit_edges is P.multiway.circuit_edges and P.multiway_registration is P.multiway.multiway_registration
    assert P.MultiwayProblem is P.multiway.MultiwayProblem and P.MultiwayResult is P.multiway.MultiwayResult
    assert P.refine_pose_graph is P.posegraph.refine_pose_graph


# ------------------------------------------------------------------------------------------------- argument checks
class _NoDevice:
    @classmethod
    def current(cls):
        raise AssertionError("a device context was asked for")


def test_bad_arguments_raise_value_error_before_a_device_is_touched(monkeypatch):
    P = pkg()
    monkeypatch.setattr(P._lib, "Context", _NoDevice)
    reg = P.registration
    clouds = [np.zeros((5, 3), np.float32)] * 3
    poses = [np.identity(4)] * 3
    good = dict(poses=poses, edges=[(0, 1), (1, 2)], max_correspondence_distance=0.5)
    bad = [(dict(edges=[(0, 3)]), "edges"), (dict(edges=[(-1, 0)]), "edges"), (dict(edges=[(1, 1)]), "itself"), (dict(edges=[(0, 1, 2)]), "edges"),
           (dict(edges=[(0.5, 1.0)]), "edges"), (dict(max_correspondence_distance=0.0), "max_correspondence_distance"),
           (dict(max_correspondence_distance=-1.0), "max_correspondence_distance"), (dict(max_correspondence_distance=float("inf")), "max_correspondence_distance"),
           (dict(max_correspondence_distance=float("nan")), "max_correspondence_distance"), (dict(max_correspondence_distance="wide"), "max_correspondence_distance"),
           (dict(poses=poses[:2]), "poses"), (dict(poses=[np.identity(3)] * 3), "poses"),
           (dict(poses=[np.identity(4), np.identity(4), np.full((4, 4), np.nan)]), "non-finite"),
           (dict(estimation_method=reg.TransformationEstimationPointToPoint(with_scaling=True)), "with_scaling"),
           (dict(estimation_method=reg.TransformationEstimationForColoredICP()), "estimation_method"), (dict(estimation_method="plane"), "estimation_method"),
           (dict(reference_node=3), "reference_node"), (dict(reference_node=-1), "reference_node"), (dict(reference_node=0.5), "reference_node")]
    for change, word in bad:
        kw = dict(good); kw.update(change)
        with pytest.raises(ValueError, match=word):
            P.multiway_registration(clouds, **kw)
    with pytest.raises(ValueError, match="cloud 1"):
        P.MultiwayProblem([np.zeros((5, 3), np.float32), np.zeros((5, 4), np.float32)])
    g = P.posegraph.PoseGraph()
    g.nodes = [P.posegraph.PoseGraphNode() for _ in range(3)]
    g.edges = [P.posegraph.PoseGraphEdge(0, 1), P.posegraph.PoseGraphEdge(1, 2)]
    with pytest.raises(ValueError, match="refine_pose_graph"):
        P.refine_pose_graph(clouds[:2], g, 0.5)
    g.edges.append(P.posegraph.PoseGraphEdge(2, 2))
    with pytest.raises(ValueError, match="refine_pose_graph"):
        P.refine_pose_graph(clouds, g, 0.5)


def test_missing_normals_are_refused_by_name_before_a_device_is_touched(monkeypatch):
    P = pkg()
    monkeypatch.setattr(P._lib, "Context", _NoDevice)
    prob = P.MultiwayProblem.__new__(P.MultiwayProblem)
    prob.sizes, prob.has_normals, prob._handle = [5, 5, 0], [True, False, False], C.c_void_p(1)
    M = [np.identity(4)] * 3
    with pytest.raises(ValueError, match="normals of cloud 1"):
        prob.linearize(M, [(0, 1)], 0.5)                                                              # point-to-plane: the target's
    with pytest.raises(ValueError, match="normals of cloud 1"):
        prob.linearize(M, [(1, 0)], 0.5, P.registration.TransformationEstimationForGeneralizedICP())   # GICP: the source's too
    with pytest.raises(ValueError, match="per-edge"):
        prob.linearize(M, [(0, 1)], 0.5, P.registration.TransformationEstimationPointToPoint(), per_edge=True)
    prob._handle = None
    with pytest.raises(RuntimeError, match="closed"):
        prob.linearize(M, [(1, 0)], 0.5)


def test_refine_pose_graph_builds_its_edges_from_the_graph():
    P = pkg()
    pg = P.posegraph
    poses = _shifted(4)
    g = pg.PoseGraph()
    g.nodes = [pg.PoseGraphNode(T) for T in poses]
    g.edges = [pg.PoseGraphEdge(0, 1, np.identity(4) * 2, np.identity(6) * 3, uncertain=False), pg.PoseGraphEdge(1, 2), pg.PoseGraphEdge(0, 3, uncertain=True)]
    seen = []

    class Spy(_Stub):
        def linearize(self, poses, edges, *a, **k):
            seen.append(np.asarray(edges).tolist())
            return super().linearize(poses, edges, *a, **k)
    res = pg.refine_pose_graph(Spy([10] * 4, [10] * 6), g, 1.0)
    assert seen[0] == [[0, 1], [1, 0], [1, 2], [2, 1], [0, 3], [3, 0]]
    for nd, T in zip(g.nodes, res.poses):
        assert np.array_equal(nd.pose, T)
    assert np.array_equal(g.nodes[0].pose, poses[0]) and not np.array_equal(g.nodes[3].pose, poses[3])
    assert np.array_equal(g.edges[0].transformation, np.identity(4) * 2) and np.array_equal(g.edges[0].information, np.identity(6) * 3)
    assert [e.uncertain for e in g.edges] == [False, False, True]
    seen.clear()
    pg.refine_pose_graph(Spy([10] * 4, [10] * 3), g, 1.0, symmetric=False, reference_node=1)
    assert seen[0] == [[0, 1], [1, 2], [0, 3]]


# ------------------------------------------------------------------------------------------------- ABI
def test_entry_points_are_declared_exported_and_prototyped():
    P = pkg()
    hdr = open(os.path.join(ROOT, "include", "pcr_hip.h")).read()
    if not os.path.exists(P._lib.SO_PATH):
        P._lib.build()
    lib = P._lib.load()
    want = {"pcr_multiway_create": ["ctx", "n_clouds", "xyz", "normals", "n", "problem"],
            "pcr_multiway_destroy": ["problem"],
            "pcr_multiway_linearize": ["ctx", "problem", "edges2", "E", "M", "max_correspondence_distance", "estimation", "JTJ", "JTr", "stats", "rows", "match"]}
    for name, args in want.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert m, f"{name} is not declared in include/pcr_hip.h"
        assert [p.split()[-1].lstrip("*") for p in m.group(1).split(",")] == args
        assert name in P._lib.EXPORTS and hasattr(lib, name)
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == len(args)
    assert re.search(r"#define\s+PCR_MULTIWAY_TILE\s+256\b", hdr) and P._lib.MULTIWAY_TILE == 256
    doc = hdr[:hdr.index("int pcr_multiway_create(")].rsplit("/* ==", 1)[1]
    for word in ("Borrmann", "registration::LUM", "((M_r0 x + M_r1 y) + M_r2 z) + M_r3", "max_nn = 1", "strict", "non-finite", "1e-300", "[s x n_t, n_t]",
                 "-skew(s)", "R C_s R^T", "sum_d2", "sum_wr2", "without floating-point atomics", "any position of any list", "Rz Ry Rx",
                 "[[R, 0], [skew(t) R, R]]", "H x = -g", "lowest-numbered", "converged = false", "PCR_EINVAL", "with_scaling"):
        assert word in doc, word


def test_unit_is_in_the_build_and_in_the_packed_fp32_scan():
    csrc = os.path.join(ROOT, "point-cloud-registration-with-global-refinement_amd", "csrc")
    assert os.path.exists(os.path.join(csrc, "pcr_multiway.hip"))
    assert re.search(r"^for f in .*\bpcr_multiway\b", open(os.path.join(csrc, "build.sh")).read(), re.M)
    assert '"pcr_multiway"' in open(os.path.join(ROOT, "tools", "pk_trans_scan.py")).read()


# ------------------------------------------------------------------------------------------------- the conditions of the GPU comparisons
def test_the_fixture_is_what_the_gpu_tests_assume(loop4):
    clouds = loop4["clouds"]
    assert len(clouds) == 4 and all(c.dtype == np.float32 and 3000 < len(c) < 3700 for c in clouds)
    a0, d0 = mr.pose_distance(loop4["drifted"], loop4["planted"])
    assert 2.4e-2 < a0 < 2.6e-2 and 0.2 < d0 < 0.26
    assert np.array_equal(loop4["drifted"][0], loop4["planted"][0]) and np.array_equal(loop4["planted"][0], np.identity(4))
    again = mr.planted_loop()
    assert all(np.array_equal(a, b) for a, b in zip(again["clouds"], clouds))


def test_at_least_80_percent_of_the_source_points_have_a_row_at_the_planted_poses(loop4):
    sums = mr.linearize(loop4["clouds"], loop4["normals"], loop4["planted"], EDGES8, 1.2, mr.P2PL, fast=False)
    total = sum(len(loop4["clouds"][a]) for a, _ in EDGES8)
    rows = sum(s["rows"] for s in sums)
    print(f"rows at the planted poses: {rows} of {total}")
    assert rows >= 0.8 * total
    # the k-d tree form of the search the loops use gives the same rows as the brute-force rule
    for (a, b), s in zip(EDGES8[:3], sums):
        M = mr.inv_rigid(loop4["drifted"][b]) @ loop4["drifted"][a]
        i1, d1, _ = mr.matches(M, loop4["clouds"][a], loop4["clouds"][b], 1.2, fast=False)
        i2, d2, _ = mr.matches(M, loop4["clouds"][a], loop4["clouds"][b], 1.2, fast=True)
        assert np.array_equal(i1, i2) and np.array_equal(d1.view(np.int64), d2.view(np.int64)) and (i1 >= 0).sum() > 0.5 * len(i1)


@pytest.mark.parametrize("kind, loss", [(mr.P2PL, mr.L2), (mr.GICP, mr.L1)], ids=["point_to_plane_L2", "gicp_L1"])
def test_the_reference_loop_ends_ten_times_closer_to_the_planted_poses(loop4, kind, loss):
    a0, d0 = mr.pose_distance(loop4["drifted"], loop4["planted"])
    res = mr.loop(loop4["clouds"], loop4["normals"], loop4["drifted"], EDGES8, 1.2, kind, loss)
    a1, d1 = mr.pose_distance(res["poses"], loop4["planted"])
    print(f"reference loop: {a0:.2e} rad / {d0:.2e} m -> {a1:.2e} rad / {d1:.2e} m in {res['iterations']} iterations, converged {res['converged']}")
    assert res["converged"] and a1 * 10 <= a0 and d1 * 10 <= d0
    assert np.array_equal(res["poses"][0], loop4["drifted"][0])
