"""Joint multiway registration on the device (csrc/pcr_multiway.hip, multiway.py) against the numpy restatement of its rule
(tests/multiway_reference.py): matches exactly, sums within the reordering bound of their own terms, the same bits whatever else is in the edge
list, and the loop against the reference loop under the reference's own scatter.  The fixture is `planted_loop` (four scans of pair 899's target
at 0.6 m voxels, about 3.3k points each), with the normals `estimate_normals(KNN 20)` gives on the device."""
import ctypes as C

import numpy as np
import pytest

import multiway_reference as mr
from conftest import TOL_M, TOL_RAD, pkg

pytestmark = pytest.mark.gpu

EDGES8 = [(0, 1), (1, 0), (1, 2), (2, 1), (2, 3), (3, 2), (3, 0), (0, 3)]
CAP = 1.2
FIELDS = ("JTJ", "JTr", "rows", "sum_d2", "sum_r2", "sum_wr2")


def _estimation(P, kind, loss):
    reg = P.registration
    kernel = {mr.L2: reg.L2Loss(), mr.L1: reg.L1Loss(), mr.GM: reg.GMLoss(0.5)}[loss]
    if kind == mr.P2P:
        return reg.TransformationEstimationPointToPoint()          # (its rows carry no weight: the loss is not read)
    return reg.TransformationEstimationPointToPlane(kernel) if kind == mr.P2PL else reg.TransformationEstimationForGeneralizedICP(kernel)


def _edge_M(poses, edges):
    return np.array([mr.inv_rigid(poses[b]) @ poses[a] for a, b in edges])


@pytest.fixture(scope="module")
def loop4():
    P = pkg()
    f = mr.planted_loop()
    pcs = []
    for c in f["clouds"]:
        pc = P.PointCloud(c)
        pc.estimate_normals(P.KDTreeSearchParamKNN(20))
        pcs.append(pc)
    f["pcs"] = pcs
    f["normals"] = [pc.device_normals().cpu().numpy() for pc in pcs]          # float32, as stored
    f["identity"] = np.array([np.identity(4)] * 4)
    f["found"] = {}                                                            # pose set -> the reference's matches per edge, computed once
    with P.MultiwayProblem(pcs) as problem:
        f["problem"] = problem
        yield f


def _found(f, which):
    if which not in f["found"]:
        M = _edge_M(f[which], EDGES8)
        f["found"][which] = (M, [mr.matches(M[k], f["clouds"][a], f["clouds"][b], CAP) for k, (a, b) in enumerate(EDGES8)])
    return f["found"][which]


# ------------------------------------------------------------------------------------------------- matches
@pytest.mark.parametrize("which", ["planted", "drifted", "identity"])
def test_matches_equal_the_reference_exactly(loop4, which):
    P = pkg()
    M, found = _found(loop4, which)
    lin = loop4["problem"].linearize(M, EDGES8, CAP, P.registration.TransformationEstimationPointToPoint(), return_matches=True, per_edge=True)
    total = 0
    for k, (idx, d2, _) in enumerate(found):
        dev = lin["matches"][k].cpu().numpy()
        assert dev.dtype == np.int32 and np.array_equal(dev, idx), (which, k, int((dev != idx).sum()))
        assert lin["rows"][k] == (idx >= 0).sum()
        total += int((idx >= 0).sum())
    print(f"{which}: {total} rows on 8 edges")
    assert total > 0
    # node poses give the same M, hence the same matches
    lin2 = loop4["problem"].linearize(loop4[which], EDGES8, CAP, P.registration.TransformationEstimationPointToPoint(), return_matches=True)
    assert np.array_equal(lin2["M"], M)
    assert all(np.array_equal(a.cpu().numpy(), b.cpu().numpy()) for a, b in zip(lin["matches"], lin2["matches"]))


def test_a_target_exactly_at_the_radius_gives_no_row_and_a_tie_gives_the_lower_index():
    P = pkg()
    est = P.registration.TransformationEstimationPointToPoint()
    src = np.zeros((1, 3), np.float32)
    at_r = np.array([[0.5, 0.0, 0.0]], np.float32)
    ties = np.array([[1.0, 1.0, 1.0], [0.0, 0.25, 0.0], [0.25, 0.0, 0.0], [-0.25, 0.0, 0.0]], np.float32)
    with P.MultiwayProblem([src, at_r, ties]) as prob:
        lin = prob.linearize([np.identity(4)] * 3, [(0, 1), (0, 2), (1, 0)], 0.5, est, return_matches=True)
        assert lin["rows"].tolist() == [0, 1, 0]
        assert [m.cpu().numpy().tolist() for m in lin["matches"]] == [[-1], [1], [-1]]
        assert not lin["JTJ"][0].any() and not lin["JTr"][0].any() and lin["sum_d2"][0] == 0.0
        assert lin["sum_d2"][1] == 0.0625 and lin["sum_r2"][1] == 0.0625 and lin["sum_wr2"][1] == 0.0625
        assert np.array_equal(lin["JTr"][1], [0.0, 0.0, 0.0, 0.0, -0.25, 0.0])
        lin = prob.linearize([np.identity(4)] * 3, [(0, 1)], np.nextafter(0.5, 1.0), est, return_matches=True)       # just inside
        assert lin["rows"].tolist() == [1] and lin["matches"][0].cpu().numpy().tolist() == [0] and lin["sum_d2"][0] == 0.25


# ------------------------------------------------------------------------------------------------- sums
def _assert_sums(dev, k, ref, what):
    assert dev["rows"][k] == ref["rows"], (what, dev["rows"][k], ref["rows"])
    worst = 0.0
    for name in ("JTJ", "JTr", "sum_d2", "sum_r2", "sum_wr2"):
        d, r, a = np.asarray(dev[name][k], np.float64), np.asarray(ref[name], np.float64), np.asarray(ref["abs"][name], np.float64)
        assert np.isfinite(d).all(), (what, name)
        err = np.abs(d - r)
        with np.errstate(divide="ignore", invalid="ignore"):
            worst = max(worst, float(np.nanmax(np.where(a > 0, err / a, np.where(err > 0, np.inf, 0.0)))))
        assert (err <= 1e-9 * a).all(), (what, name, float(err.max()), float(a.max()))
    return worst


@pytest.mark.parametrize("loss", [mr.L2, mr.L1, mr.GM], ids=["L2", "L1", "GM"])
@pytest.mark.parametrize("kind", [mr.P2P, mr.P2PL, mr.GICP], ids=["point_to_point", "point_to_plane", "gicp"])
def test_sums_are_the_reference_sums_within_the_reordering_bound(loop4, kind, loss):
    """|device - reference| <= 1e-9 x the sum of the absolute values of the element's terms.  Any regrouping of at most 3 x 2^20 float64 terms
    stays within 3 x 2^20 x 2^-53 = 3.5e-10 of that sum; the 3x3 inverse square roots of the GICP rows are conditioned at most 1 / epsilon = 1e3."""
    P = pkg()
    M, found = _found(loop4, "drifted")
    lin = loop4["problem"].linearize(M, EDGES8, CAP, _estimation(P, kind, loss), per_edge=True)
    worst = 0.0
    for k, (a, b) in enumerate(EDGES8):
        ref = mr.edge_sums(kind, loss, 0.5, 1e-3, M[k], loop4["clouds"][a], loop4["normals"][a], loop4["clouds"][b], loop4["normals"][b], CAP, found=found[k])
        worst = max(worst, _assert_sums(lin, k, ref, (kind, loss, k)))
        assert np.array_equal(lin["JTJ"][k], lin["JTJ"][k].T)
    print(f"kind {kind} loss {loss}: largest |dev - ref| / sum|terms| = {worst:.2e}")


def _random_cloud(P, rng, n, offset=0.0):
    pc = P.PointCloud((rng.uniform(0.0, 1.0, (n, 3)) + offset).astype(np.float32))
    if n:
        nrm = rng.normal(size=(n, 3))
        pc.normals = (nrm / np.linalg.norm(nrm, axis=1)[:, None]).astype(np.float32)
    return pc


def test_every_source_size_around_the_octet_and_the_tile_against_small_and_large_targets():
    P = pkg()
    TILE = P._lib.MULTIWAY_TILE
    rng = np.random.default_rng(3)
    sizes = [1, 7, 8, 9, TILE - 1, TILE, TILE + 1]
    pcs = [_random_cloud(P, rng, n) for n in sizes] + [_random_cloud(P, rng, 1), _random_cloud(P, rng, 1000), _random_cloud(P, rng, 0), _random_cloud(P, rng, 300, 100.0)]
    T1, T1000, EMPTY, FAR = len(sizes), len(sizes) + 1, len(sizes) + 2, len(sizes) + 3
    edges = [(s, t) for s in range(len(sizes)) for t in (T1, T1000)] + [(0, EMPTY), (EMPTY, T1000), (T1000, EMPTY), (T1000, FAR), (FAR, T1000), (T1000, T1)]
    xyz = [pc.device_xyz().cpu().numpy() for pc in pcs]
    nrm = [pc.device_normals().cpu().numpy() if pc.has_normals() else None for pc in pcs]
    poses = [mr.inv_rigid(np.identity(4)) for _ in pcs]
    poses[3] = np.array([[0.0, -1.0, 0.0, 1.0], [1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.05], [0.0, 0.0, 0.0, 1.0]])          # one source turned about z
    M = _edge_M(poses, edges)
    est = P.registration.TransformationEstimationPointToPlane(P.registration.GMLoss(0.5))
    with P.MultiwayProblem(pcs) as prob:
        assert len(prob) == len(pcs) and prob.sizes == sizes + [1, 1000, 0, 300]
        lin = prob.linearize(M, edges, 0.3, est, return_matches=True, per_edge=True)
        one = [prob.linearize(M[k:k + 1], edges[k:k + 1], 0.3, est, return_matches=True, per_edge=True) for k in (0, 9, len(edges) - 1)]       # E = 1
    matched = 0
    for k, (a, b) in enumerate(edges):
        ref = mr.edge_sums(mr.P2PL, mr.GM, 0.5, 1e-3, M[k], xyz[a], nrm[a], xyz[b], nrm[b], 0.3)
        dev = lin["matches"][k].cpu().numpy()
        assert dev.shape == (len(xyz[a]),) and np.array_equal(dev, ref["match"]), (k, a, b)
        _assert_sums(lin, k, ref, (k, a, b))
        matched += ref["rows"]
    assert matched > 700
    # an edge touching an empty cloud and an edge with no row: zeros, and every source point unmatched
    for k in range(len(sizes) * 2, len(sizes) * 2 + 5):
        assert lin["rows"][k] == 0 and not lin["JTJ"][k].any() and not lin["JTr"][k].any() and lin["sum_d2"][k] == lin["sum_r2"][k] == lin["sum_wr2"][k] == 0.0
        assert (lin["matches"][k].cpu().numpy() == -1).all()
    assert lin["rows"][1] == 1 and lin["rows"][2 * 6 + 1] > 200          # the one-point source and the TILE + 1 source in the large target
    for o, k in zip(one, (0, 9, len(edges) - 1)):
        for name in FIELDS:
            assert np.array_equal(np.asarray(o[name][0]), np.asarray(lin[name][k])), (name, k)
        assert np.array_equal(o["matches"][0].cpu().numpy(), lin["matches"][k].cpu().numpy())
    with P.MultiwayProblem(pcs) as prob:
        none = prob.linearize(np.zeros((0, 4, 4)), [], 0.3, est, return_matches=True, per_edge=True)
        assert none["JTJ"].shape == (0, 6, 6) and none["rows"].shape == (0,) and none["matches"] == []


# ------------------------------------------------------------------------------------------------- bits
def _bits(lin, k):
    return tuple(np.ascontiguousarray(lin[name][k]).tobytes() for name in FIELDS) + (lin["matches"][k].cpu().numpy().tobytes(),)


def test_the_same_edge_gives_the_same_bits_in_any_position_of_any_list(loop4):
    P = pkg()
    est = P.registration.TransformationEstimationForGeneralizedICP(P.registration.L1Loss())
    M = _edge_M(loop4["drifted"], EDGES8)
    prob = loop4["problem"]
    first = prob.linearize(M, EDGES8, CAP, est, return_matches=True, per_edge=True)
    again = prob.linearize(M, EDGES8, CAP, est, return_matches=True, per_edge=True)
    base = [_bits(first, k) for k in range(8)]
    assert [_bits(again, k) for k in range(8)] == base
    assert all(first["rows"][k] > 1000 for k in range(8))
    perm = [5, 2, 7, 0, 3, 6, 1, 4]
    shuffled = prob.linearize(M[perm], [EDGES8[p] for p in perm], CAP, est, return_matches=True, per_edge=True)
    assert [_bits(shuffled, j) for j in range(8)] == [base[p] for p in perm]
    dup = [0, 3, 3, 1, 0, 3]
    doubled = prob.linearize(M[dup], [EDGES8[p] for p in dup], CAP, est, return_matches=True, per_edge=True)
    assert [_bits(doubled, j) for j in range(len(dup))] == [base[p] for p in dup]


# ------------------------------------------------------------------------------------------------- the loop
@pytest.mark.parametrize("kind, loss, max_it", [(mr.P2PL, mr.L2, 30), (mr.GICP, mr.L1, 10)], ids=["point_to_plane_L2", "gicp_L1"])
def test_loop_against_the_reference_loop_and_the_planted_poses(loop4, kind, loss, max_it):
    """The bound of the device-vs-reference comparison is the larger of the north-star tolerance and three times the reference's own spread when its
    float64 sums are regrouped (chunks of 64 / 512 / 4096 terms): the method of conftest.l1_tolerance.  Against the planted poses the device must
    land within twice the error the reference reaches, which is computed here."""
    P = pkg()
    crit = P.registration.ICPConvergenceCriteria(1e-6, 1e-6, max_it)
    res = P.multiway_registration(loop4["problem"], loop4["drifted"], EDGES8, CAP, _estimation(P, kind, loss), crit)
    run = lambda chunk: mr.loop(loop4["clouds"], loop4["normals"], loop4["drifted"], EDGES8, CAP, kind, loss, 0.5, 1e-3, max_it, 1e-6, 1e-6, 0, chunk)
    ref = run(None)
    spread = [mr.pose_distance(run(c)["poses"], ref["poses"]) for c in (64, 512, 4096)]
    sa, sd = max(s[0] for s in spread), max(s[1] for s in spread)
    tol_a, tol_d = max(TOL_RAD, 3.0 * sa), max(TOL_M, 3.0 * sd)
    a, d = mr.pose_distance(res.poses, ref["poses"])
    a0, d0 = mr.pose_distance(loop4["drifted"], loop4["planted"])
    ra, rd = mr.pose_distance(ref["poses"], loop4["planted"])
    da, dd = mr.pose_distance(res.poses, loop4["planted"])
    print(f"device vs reference {a:.2e} rad {d:.2e} m (spread {sa:.2e} / {sd:.2e}, bound {tol_a:.2e} / {tol_d:.2e}); iterations {res.iterations} vs {ref['iterations']}; "
          f"to the planted poses: start {a0:.2e} / {d0:.2e}, reference {ra:.2e} / {rd:.2e}, device {da:.2e} / {dd:.2e}; fitness {res.fitness:.4f} rmse {res.inlier_rmse:.4f}")
    assert a <= tol_a and d <= tol_d
    assert da <= 2.0 * ra and dd <= 2.0 * rd
    assert np.array_equal(res.poses[0], loop4["drifted"][0])
    assert len(res.history) == res.iterations + 1 and res.history[-1] == (res.fitness, res.inlier_rmse)
    assert res.edge_rows.shape == (8,) and res.edge_rmse.shape == (8,) and res.edge_rows.sum() == round(res.fitness * sum(len(loop4["clouds"][a_]) for a_, _ in EDGES8))
    assert abs(res.fitness - ref["fitness"]) < 1e-3 and abs(res.inlier_rmse - ref["inlier_rmse"]) < 1e-4


def test_refine_pose_graph_gives_the_poses_of_multiway_registration_bit_for_bit(loop4):
    P = pkg()
    pg = P.posegraph
    crit = P.registration.ICPConvergenceCriteria(1e-6, 1e-6, 3)
    info = lambda s, t, v, T: np.identity(6) * 7.0
    g = pg.pose_graph_from_odometry(loop4["pcs"], loop4["drifted"], information_fn=info)
    before = [(e.transformation.copy(), e.information.copy(), e.uncertain) for e in g.edges]
    res = pg.refine_pose_graph(loop4["problem"], g, CAP, criteria=crit)
    edges = [(0, 1), (1, 0), (1, 2), (2, 1), (2, 3), (3, 2)]
    want = P.multiway_registration(loop4["problem"], loop4["drifted"], edges, CAP, criteria=crit)
    assert res.iterations == want.iterations >= 1
    for nd, T, W in zip(g.nodes, res.poses, want.poses):
        assert np.array_equal(nd.pose.view(np.int64), W.view(np.int64)) and np.array_equal(T.view(np.int64), W.view(np.int64))
    assert not np.array_equal(g.nodes[3].pose, loop4["drifted"][3])
    for e, (T, I, u) in zip(g.edges, before):
        assert np.array_equal(e.transformation, T) and np.array_equal(e.information, I) and e.uncertain == u
    # from a list of clouds the problem is made and closed inside the call: the same poses
    g2 = pg.pose_graph_from_odometry(loop4["pcs"], loop4["drifted"], information_fn=info)
    pg.refine_pose_graph(loop4["pcs"], g2, CAP, criteria=crit)
    assert all(np.array_equal(a.pose, b.pose) for a, b in zip(g.nodes, g2.nodes))


# ------------------------------------------------------------------------------------------------- refusals
def _raw(P, prob, edges, M, r, est):
    ctx = P._lib.Context.current()
    e = np.ascontiguousarray(np.asarray(edges, np.int32).reshape(-1, 2))
    E = len(e)
    Mc = np.ascontiguousarray(M, np.float64)
    JTJ, JTr, stats, rows = np.full((E, 36), 7.0), np.full((E, 6), 7.0), np.full((E, 3), 7.0), np.full(E, 7, np.int64)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    rc = ctx.lib.pcr_multiway_linearize(ctx.handle, prob._handle, e.ctypes.data_as(C.c_void_p), C.c_int64(E), dp(Mc), C.c_double(r), C.byref(est) if est is not None else None,
                                        dp(JTJ), dp(JTr), dp(stats), rows.ctypes.data_as(C.POINTER(C.c_int64)), None)
    msg = ctx.lib.pcr_last_error(ctx.handle)
    untouched = (JTJ == 7.0).all() and (JTr == 7.0).all() and (stats == 7.0).all() and (rows == 7).all()
    return rc, (msg.decode() if msg else ""), untouched


def test_refusals_name_their_argument():
    P = pkg()
    L = P._lib
    rng = np.random.default_rng(8)
    with_n, bare = _random_cloud(P, rng, 50), P.PointCloud(rng.uniform(0, 1, (40, 3)).astype(np.float32))
    plane = L.PcrEstimation(L.EST_POINT_TO_PLANE, 0, L.LOSS_L2, 1.0, 1e-3)
    point = L.PcrEstimation(L.EST_POINT_TO_POINT, 0, L.LOSS_L2, 1.0, 1e-3)
    gicp = L.PcrEstimation(L.EST_GENERALIZED_ICP, 0, L.LOSS_L1, 1.0, 1e-3)
    I = np.identity(4).reshape(1, 4, 4)
    bad_M = I.copy(); bad_M[0, 1, 3] = np.inf
    with P.MultiwayProblem([with_n, bare, with_n]) as prob:
        cases = [(([(0, 3)], I, 0.5, point), ["edges", "0..2"]), (([(-1, 0)], I, 0.5, point), ["edges"]), (([(2, 2)], I, 0.5, point), ["edges", "itself"]),
                 (([(0, 1)], I, 0.0, point), ["max_correspondence_distance"]), (([(0, 1)], I, -0.5, point), ["max_correspondence_distance"]),
                 (([(0, 1)], I, float("inf"), point), ["max_correspondence_distance"]), (([(0, 1)], I, float("nan"), point), ["max_correspondence_distance"]),
                 (([(0, 1)], bad_M, 0.5, point), ["M", "edge 0"]),
                 (([(0, 1)], I, 0.5, plane), ["normals", "cloud 1"]), (([(0, 2), (1, 0)], np.concatenate([I, I]), 0.5, gicp), ["normals", "cloud 1", "edge 1"]),
                 (([(0, 1)], I, 0.5, L.PcrEstimation(L.EST_POINT_TO_POINT, 1, L.LOSS_L2, 1.0, 1e-3)), ["with_scaling"]),
                 (([(0, 1)], I, 0.5, L.PcrEstimation(7, 0, L.LOSS_L2, 1.0, 1e-3)), ["estimation", "kind"]),
                 (([(0, 2)], I, 0.5, L.PcrEstimation(L.EST_POINT_TO_PLANE, 0, 9, 1.0, 1e-3)), ["estimation", "loss"]),
                 (([(0, 1)], I, 0.5, None), ["estimation"])]
        for args, words in cases:
            rc, msg, untouched = _raw(P, prob, *args)
            assert rc == L.PCR_EINVAL and untouched, (args[0], rc, msg)
            assert msg.startswith("multiway_linearize") and all(w in msg for w in words), (words, msg)
        rc, msg, _ = _raw(P, prob, [(1, 0)], I, 0.5, plane)          # the target carries normals: point-to-plane does not need the source's
        assert rc == L.PCR_OK, msg
        # the Python layer refuses the same things with ValueError (tests/test_multiway_api.py); what reaches the library raises its message
        with pytest.raises(ValueError, match="normals of cloud 1"):
            prob.linearize([np.identity(4)] * 3, [(0, 1)], 0.5)
    with pytest.raises(RuntimeError, match="multiway_create"):
        ctx = L.Context.current()
        h = C.c_void_p()
        ctx.check(ctx.lib.pcr_multiway_create(ctx.handle, 1, (C.c_void_p * 1)(None), None, (C.c_int64 * 1)(5), C.byref(h)), "create")


def test_use_after_close_raises(loop4):
    P = pkg()
    prob = P.MultiwayProblem(loop4["pcs"][:2])
    prob.linearize([np.identity(4)] * 2, [(0, 1)], CAP)
    prob.close()
    prob.close()                                                      # closing twice is harmless
    with pytest.raises(RuntimeError, match="closed"):
        prob.linearize([np.identity(4)] * 2, [(0, 1)], CAP)
    with pytest.raises(RuntimeError, match="closed"):
        P.multiway_registration(prob, [np.identity(4)] * 2, [(0, 1)], CAP)
    with P.MultiwayProblem(loop4["pcs"][:2]) as inside:
        pass
    with pytest.raises(RuntimeError, match="closed"):
        inside.linearize([np.identity(4)] * 2, [(0, 1)], CAP)
