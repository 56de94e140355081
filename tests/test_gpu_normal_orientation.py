"""Normal orientation on the device against the restatement of the rules of include/pcr_hip.h (normal_orientation_reference.py) on the same float32
points and normals.  Under the order (weight, lo, hi) both spanning trees are unique, so every comparison is equality: EMST edges and d^2 bits,
tree edges, flip mask, normals as uint32; there is no tolerance in this file.

Inputs: every second source point of golden pair 899 (8,263 rows, whose k-NN graph falls into 175 / 15 / 3 components at k = 4 / 16 / 30) with
the normals of estimate_normals(KNN 20) and a seeded half of them negated; the 6 x 6 x 6 lattice with normals +-(0, 0, 1), where every weight
is tied and (lo, hi) alone decides both trees; duplicated points; sizes around the wavefront and workgroup widths with k below, at and above
n; two far blobs whose rows have their whole neighbourhood in their own component."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from conftest import GOLDEN, pkg
import normal_orientation_reference as ref

pytestmark = pytest.mark.gpu

OK, EINVAL = 0, -1
NAME = "orient_normals_consistent_tangent_plane"


@pytest.fixture(scope="module")
def P():
    return pkg()


def _signs(seed, n):
    return np.where(np.random.default_rng(seed).random(n) < 0.5, -1, 1).astype(np.float32)[:, None]


def _unit_normals(seed, n):
    v = np.random.default_rng(seed).normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def _emst(P, pts, edges=True, d2=True, info=True, xyz=True, n=None):
    """pcr_euclidean_mst itself -> (status, message, edges (n - 1, 2), d2 (n - 1,), info); a False switch passes a null pointer"""
    import torch
    ctx = P._lib.Context.current()
    pts = np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 3)
    rows = len(pts)
    d = torch.from_numpy(pts).cuda() if rows else torch.zeros((1, 3), dtype=torch.float32, device="cuda")
    e = torch.full((max(rows - 1, 1), 2), -7, dtype=torch.int32, device="cuda")
    w = torch.full((max(rows - 1, 1),), -7.0, dtype=torch.float64, device="cuda")
    inf = P._lib.PcrOrientInfo(-7, -7, -7, -7, -7)
    rc = ctx.lib.pcr_euclidean_mst(ctx.handle, C.c_void_p(d.data_ptr()) if xyz else None, C.c_int64(rows if n is None else n), C.c_void_p(e.data_ptr()) if edges else None,
                                   C.c_void_p(w.data_ptr()) if d2 else None, C.byref(inf) if info else None)
    msg = ctx.lib.pcr_last_error(ctx.handle)
    m = max(rows - 1, 0)
    return rc, (msg.decode() if msg else ""), e.cpu().numpy().astype(np.int64)[:m], w.cpu().numpy()[:m], inf


def _orient(P, pts, nrm, k, flipped=True, tree=True, info=True, xyz=True, normals=True, n=None):
    """pcr_orient_normals_tangent_plane itself -> (status, message, normals after the call, flipped (n,), tree (n - 1, 2), info)"""
    import torch
    ctx = P._lib.Context.current()
    pts = np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 3)
    nrm = np.ascontiguousarray(nrm, dtype=np.float32).reshape(-1, 3)
    rows = len(pts)
    d = torch.from_numpy(pts).cuda() if rows else torch.zeros((1, 3), dtype=torch.float32, device="cuda")
    dn = torch.from_numpy(nrm.copy()).cuda() if rows else torch.zeros((1, 3), dtype=torch.float32, device="cuda")
    f = torch.full((max(rows, 1),), 9, dtype=torch.uint8, device="cuda")
    e = torch.full((max(rows - 1, 1), 2), -7, dtype=torch.int32, device="cuda")
    inf = P._lib.PcrOrientInfo(-7, -7, -7, -7, -7)
    rc = ctx.lib.pcr_orient_normals_tangent_plane(ctx.handle, C.c_void_p(d.data_ptr()) if xyz else None, C.c_void_p(dn.data_ptr()) if normals else None,
                                                  C.c_int64(rows if n is None else n), C.c_int(k), C.c_void_p(f.data_ptr()) if flipped else None,
                                                  C.c_void_p(e.data_ptr()) if tree else None, C.byref(inf) if info else None)
    msg = ctx.lib.pcr_last_error(ctx.handle)
    m = max(rows - 1, 0)
    return rc, (msg.decode() if msg else ""), dn.cpu().numpy()[:rows], f.cpu().numpy()[:rows], e.cpu().numpy().astype(np.int64)[:m], inf


def _assert_orient(P, pts, nrm, k, want, what):
    rc, msg, out, flipped, tree, info = _orient(P, pts, nrm, k)
    assert rc == OK, (what, rc, msg)
    n = len(pts)
    print(f"{what}: n = {n}, k = {k}: {info.emst_rounds} + {info.tree_rounds} rounds, {info.walked_rows} walked rows, {info.n_flipped} flipped, root {info.root}; "
          f"{int((tree != want['tree']).any(1).sum())} other tree edges, {int((flipped.astype(bool) != want['flip']).sum())} other flips")
    assert np.array_equal(tree, want["tree"]), what
    assert set(np.unique(flipped).tolist()) <= {0, 1} and np.array_equal(flipped.astype(bool), want["flip"]), what
    assert np.array_equal(out.view(np.uint32), want["normals"].view(np.uint32)), what          # bit for bit
    assert info.root == want["root"] and info.n_flipped == int(want["flip"].sum()), what
    bound = max(math.ceil(math.log2(n)), 0) if n > 1 else 0
    assert 0 <= info.emst_rounds <= bound and 0 <= info.tree_rounds <= bound, (what, info.emst_rounds, info.tree_rounds)
    return info


# ------------------------------------------------------------------------------------------------------------ 1. the golden cloud
@pytest.fixture(scope="module")
def golden(P):
    pts = np.load(os.path.join(GOLDEN, "nclt_pair_899.npz"))["source"][::2]
    assert pts.shape == (8263, 3)
    pc = P.PointCloud(pts)
    pc.estimate_normals(P.KDTreeSearchParamKNN(20))
    nrm = pc.device_normals().cpu().numpy().astype(np.float32)
    assert np.isfinite(nrm).all()
    return dict(pts=pts, nrm=nrm * _signs(17, len(pts)), plain=nrm, emst=ref.emst_reference(pts), lists=ref.knn_lists(pts, 30))


def test_golden_emst(P, golden):
    rc, msg, edges, d2, info = _emst(P, golden["pts"])
    assert rc == OK, (rc, msg)
    we, wd = golden["emst"]
    print(f"golden EMST: {info.emst_rounds} rounds, {info.walked_rows} walked rows; {int((edges != we).any(1).sum())} other edges, "
          f"{int((d2.view(np.uint64) != wd.view(np.uint64)).sum())} distances with other bits")
    assert np.array_equal(edges, we)
    assert np.array_equal(d2.view(np.uint64), wd.view(np.uint64))
    assert 1 <= info.emst_rounds <= math.ceil(math.log2(len(we) + 1)) and info.walked_rows > 0 and info.root == -1 and info.tree_rounds == 0


@pytest.mark.parametrize("k", [4, 16, 30])
def test_golden_orientation(P, golden, k):
    want = ref.orient_reference(golden["pts"], golden["nrm"], k, emst=golden["emst"], lists=golden["lists"])
    info = _assert_orient(P, golden["pts"], golden["nrm"], k, want, f"golden k = {k}")
    assert info.emst_rounds <= math.ceil(math.log2(len(golden["pts"])))
    if k == 4:
        assert info.walked_rows > 0


# ------------------------------------------------------------------------------------------------------------ 2. the lattice
@pytest.mark.parametrize("k", [0, 7])
def test_lattice_is_decided_by_lo_hi_alone(P, k):
    lat = ref.lattice(6)
    nrm = np.tile(np.float32([0, 0, 1]), (216, 1)) * _signs(4, 216)
    rc, msg, edges, d2, _ = _emst(P, lat)
    assert rc == OK, msg
    we, wd = ref.emst_reference(lat)
    assert np.array_equal(edges, we) and np.array_equal(d2.view(np.uint64), wd.view(np.uint64)) and (d2 == 1.0).all()
    want = ref.orient_reference(lat, nrm, k, emst=(we, wd))
    _assert_orient(P, lat, nrm, k, want, f"lattice k = {k}")
    assert (want["normals"] == np.float32([0, 0, 1])).all()


def test_lattice_k_above_the_limit_is_an_error(P):
    lat = ref.lattice(6)
    nrm = np.tile(np.float32([0, 0, 1]), (216, 1)) * _signs(4, 216)
    rc, msg, out, flipped, tree, info = _orient(P, lat, nrm, 300)
    assert rc == EINVAL and NAME in msg, (rc, msg)
    assert np.array_equal(out.view(np.uint32), nrm.view(np.uint32)) and (flipped == 9).all() and (tree == -7).all()


# ------------------------------------------------------------------------------------------------------------ 3. duplicates
def test_duplicated_points(P):
    two = np.array([[0.5, 1, 2]] * 5 + [[3, 1, 2.5]] * 3, dtype=np.float32)[[0, 5, 1, 2, 6, 3, 7, 4]]
    nrm = _unit_normals(21, 8)
    for k in (0, 2, 8):
        rc, msg, edges, d2, _ = _emst(P, two)
        we, wd = ref.emst_reference(two)
        assert rc == OK and np.array_equal(edges, we) and np.array_equal(d2.view(np.uint64), wd.view(np.uint64)), msg
        assert (np.sort(d2)[:6] == 0.0).all()
        _assert_orient(P, two, nrm, k, ref.orient_reference(two, nrm, k), f"5 + 3 copies, k = {k}")
    one = np.tile(np.float32([[1.25, -2, 0.5]]), (70, 1))
    nrm = _unit_normals(22, 70)
    rc, msg, edges, d2, _ = _emst(P, one)
    we, wd = ref.emst_reference(one)
    assert rc == OK and np.array_equal(edges, we) and (d2 == 0.0).all(), msg
    assert np.array_equal(we, np.stack([np.zeros(69, np.int64), np.arange(1, 70)], 1))          # (lo, hi) alone: a star at row 0
    for k in (3, 9):
        _assert_orient(P, one, nrm, k, ref.orient_reference(one, nrm, k), f"one point 70 times, k = {k}")


# ------------------------------------------------------------------------------------------------------------ 4. sizes
@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 513, 1025])
def test_sizes(P, n):
    rng = np.random.default_rng(100 + n)
    pts = rng.uniform(-4, 4, (n, 3)).astype(np.float32)
    nrm = _unit_normals(200 + n, n)
    emst = ref.emst_reference(pts)
    rc, msg, edges, d2, _ = _emst(P, pts)
    assert rc == OK and np.array_equal(edges, emst[0]) and np.array_equal(d2.view(np.uint64), emst[1].view(np.uint64)), msg
    ks = sorted({min(max(n - 1, 0), 200), min(n, 200), min(n + 3, 200)}) if n <= 65 else [5, 12]      # below, at and above n where the limit of 200 allows it
    lists = ref.knn_lists(pts, max(ks))
    for k in ks:
        _assert_orient(P, pts, nrm, k, ref.orient_reference(pts, nrm, k, emst=emst, lists=lists), f"n = {n}, k = {k}")


# ------------------------------------------------------------------------------------------------------------ 5. two far blobs
@pytest.fixture(scope="module")
def blobs():
    rng = np.random.default_rng(31)
    a = rng.normal(0, 1.0, (700, 3)); b = rng.normal(0, 1.0, (700, 3)) + [100.0, 0, 0]
    pts = np.concatenate([a, b, [[50.0, 40.0, -3.0]]]).astype(np.float32)
    return pts, _unit_normals(32, len(pts)), ref.emst_reference(pts)


def test_two_far_blobs(P, blobs):
    pts, nrm, emst = blobs
    rc, msg, edges, d2, info = _emst(P, pts)
    assert rc == OK and np.array_equal(edges, emst[0]) and np.array_equal(d2.view(np.uint64), emst[1].view(np.uint64)), msg
    assert info.walked_rows > 0 and (d2 > 1000.0).sum() == 2                  # the two edges that cross the gaps
    _assert_orient(P, pts, nrm, 8, ref.orient_reference(pts, nrm, 8, emst=emst), "two blobs and a lone row")


# ------------------------------------------------------------------------------------------------------------ 6., 7. re-run and signs
def test_second_run_flips_nothing(P, blobs):
    pts, nrm, emst = blobs
    rc, _, out, _, tree, _ = _orient(P, pts, nrm, 8)
    assert rc == OK
    rc, _, again, flipped, tree2, info = _orient(P, pts, out, 8)
    assert rc == OK and info.n_flipped == 0 and not flipped.any()
    assert np.array_equal(tree, tree2) and np.array_equal(out.view(np.uint32), again.view(np.uint32))


def test_result_does_not_depend_on_the_input_signs(P, golden):
    outs = [_orient(P, golden["pts"], golden["plain"] * _signs(seed, len(golden["pts"])), 16) for seed in (5, 6)]
    assert outs[0][0] == OK and outs[1][0] == OK
    assert np.array_equal(outs[0][2], outs[1][2]) and np.array_equal(outs[0][4], outs[1][4])       # numerically equal normals, the same tree
    assert not np.array_equal(outs[0][3], outs[1][3])


# ------------------------------------------------------------------------------------------------------------ 8. errors
def test_errors_write_nothing(P):
    rng = np.random.default_rng(41)
    pts = rng.uniform(-1, 1, (100, 3)).astype(np.float32)
    nrm = _unit_normals(42, 100)
    want = ref.orient_reference(pts, nrm, 6)

    def refused(rc, msg, out, flipped, tree, what, word=None):
        assert rc == EINVAL and NAME in msg, (what, rc, msg)
        if word:
            assert word in msg, (what, msg)
        assert np.array_equal(out.view(np.uint32), nrm_in.view(np.uint32)) and (flipped == 9).all() and (tree == -7).all(), what
    for what, bad_pts, bad_nrm in (("coordinate", True, False), ("normal", False, True)):
        for value in (np.nan, np.inf, -np.inf):
            p, nrm_in = pts.copy(), nrm.copy()
            (p if bad_pts else nrm_in)[57, 1] = value
            rc, msg, out, flipped, tree, _ = _orient(P, p, nrm_in, 6)
            assert rc == EINVAL and NAME in msg and "non-finite" in msg, (what, rc, msg)
            assert np.array_equal(out.view(np.uint32), nrm_in.view(np.uint32)) and (flipped == 9).all() and (tree == -7).all(), what
    nrm_in = nrm
    for what, kw in (("null cloud", dict(xyz=False)), ("null normals", dict(normals=False)), ("n = 2^31", dict(n=2 ** 31)), ("n < 0", dict(n=-1))):
        rc, msg, out, flipped, tree, _ = _orient(P, pts, nrm, 6, **kw)
        refused(rc, msg, out, flipped, tree, what)
    rc, msg, out, flipped, tree, _ = _orient(P, pts, nrm, -1)
    refused(rc, msg, out, flipped, tree, "k < 0")
    rc, msg, out, flipped, tree, _ = _orient(P, pts, nrm, 201)
    refused(rc, msg, out, flipped, tree, "k = 201")
    # optional outputs left out: the same normals
    rc, msg, out, flipped, tree, _ = _orient(P, pts, nrm, 6, flipped=False, tree=False, info=False)
    assert rc == OK and np.array_equal(out.view(np.uint32), want["normals"].view(np.uint32)) and (flipped == 9).all() and (tree == -7).all(), msg
    # n = 0: nothing is written
    rc, msg, _, flipped, _, info = _orient(P, np.zeros((0, 3)), np.zeros((0, 3)), 6, xyz=False, normals=False)
    assert rc == OK and info.n_flipped == 0, msg
    # the EMST's own entry point
    rc, msg, _, _, info = _emst(P, np.zeros((0, 3)), xyz=False)
    assert rc == OK and info.emst_rounds == 0, msg
    rc, msg, _, _, info = _emst(P, pts[:1])
    assert rc == OK and info.emst_rounds == 0 and info.walked_rows == 0, msg
    rc, msg, edges, d2, _ = _emst(P, pts, d2=False, info=False)
    assert rc == OK and np.array_equal(edges, want["emst"]) and (d2 == -7.0).all(), msg
    for kw in (dict(xyz=False), dict(edges=False), dict(n=2 ** 31)):
        rc, msg, edges, d2, _ = _emst(P, pts, **kw)
        assert rc == EINVAL and "euclidean_minimum_spanning_tree" in msg and (edges == -7).all() and (d2 == -7.0).all(), (kw, rc, msg)
    p = pts.copy(); p[3, 2] = np.nan
    rc, msg, edges, d2, _ = _emst(P, p)
    assert rc == EINVAL and "non-finite" in msg and (edges == -7).all(), (rc, msg)


# ------------------------------------------------------------------------------------------------------------ 9. element-wise
def _elementwise_inputs():
    rng = np.random.default_rng(51)
    pts = rng.uniform(-5, 5, (300, 3)).astype(np.float32)
    nrm = _unit_normals(52, 300) * rng.uniform(0.2, 3.0, (300, 1)).astype(np.float32)
    nrm[[0, 10, 64]] = 0.0; nrm[11] = [0.0, -0.0, 0.0]          # zero normals
    nrm[20] = [0, 1, 0]; nrm[21] = [0, -2, 0]; nrm[22] = [0.5, 0, 0]          # dot products of exactly 0 with the references below
    pts[10] = [1.5, -2.0, 0.25]; pts[20] = [1.5, 7.0, 0.25]; pts[22] = [1.5, 3.0, 1.0]          # a zero view vector at row 10 and n . v == 0 at row 22 for the first camera below
    return pts, nrm


def test_elementwise_calls_match_their_restatement(P):
    import torch
    ctx = P._lib.Context.current()
    pts, nrm = _elementwise_inputs()
    d = torch.from_numpy(pts).cuda()

    def call(mode, r, xyz=True):
        dn = torch.from_numpy(nrm.copy()).cuda()
        if mode == 2:
            rc = ctx.lib.pcr_normalize_normals(ctx.handle, C.c_void_p(dn.data_ptr()), C.c_int64(len(nrm)))
        else:
            rc = ctx.lib.pcr_orient_normals(ctx.handle, C.c_void_p(d.data_ptr()) if xyz else None, C.c_void_p(dn.data_ptr()), C.c_int64(len(nrm)), C.c_int(mode),
                                            (C.c_double * 3)(*r))
        return rc, dn.cpu().numpy()
    for r in ((1.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0.3, -0.7, 0.1)):
        rc, out = call(0, r, xyz=False)
        assert rc == OK and np.array_equal(out.view(np.uint32), ref.direction_reference(nrm, r).view(np.uint32)), r
    for loc in ((1.5, -2.0, 0.25), (0.0, 0.0, 0.0), (100.0, 3.0, -8.0)):
        rc, out = call(1, loc)
        assert rc == OK and np.array_equal(out.view(np.uint32), ref.camera_reference(pts, nrm, loc).view(np.uint32)), loc
    rc, out = call(2, None)
    want = ref.normalize_reference(nrm)
    assert rc == OK and np.array_equal(out.view(np.uint32), want.view(np.uint32))
    assert (out[[0, 10, 11, 64]] == 0).all() and np.allclose(np.linalg.norm(np.delete(out, [0, 10, 11, 64], 0), axis=1), 1.0, atol=1e-6)
    assert call(1, (0.0, 0.0, 0.0), xyz=False)[0] == EINVAL and call(3, (0.0, 0.0, 1.0))[0] == EINVAL


# ------------------------------------------------------------------------------------------------------------ 10. the Python layer
def test_python_layer(P, golden):
    import torch
    pts = golden["pts"]
    pc = P.PointCloud(pts)
    with pytest.raises(RuntimeError, match="normals"):
        pc.orient_normals_consistent_tangent_plane(8)
    with pytest.raises(RuntimeError, match="normals"):
        pc.orient_normals_towards_camera_location()
    pc.normals = golden["nrm"]
    pc.colors = np.full((len(pts), 3), 0.25, np.float32)
    pc.estimate_covariances(P.KDTreeSearchParamKNN(10))
    for kw in ("lambda_penalty", "cos_alpha_tol"):
        with pytest.raises(ValueError, match=kw):
            pc.orient_normals_consistent_tangent_plane(16, **{kw: 0.5})
    xyz0, col0, cov0, nrm_t = pc.device_xyz().clone(), pc.device_colors().clone(), pc._cov.clone(), pc.device_normals()
    want = ref.orient_reference(pts, golden["nrm"], 16, emst=golden["emst"], lists=golden["lists"])
    assert pc.orient_normals_consistent_tangent_plane(16) is None
    assert pc.device_normals() is nrm_t                                           # the tensor itself was updated
    assert np.array_equal(nrm_t.cpu().numpy().view(np.uint32), want["normals"].view(np.uint32))
    assert torch.equal(pc.device_xyz(), xyz0) and torch.equal(pc.device_colors(), col0) and torch.equal(pc._cov, cov0)
    flipped, info = P.geometry._orient_normals_tangent_plane(pc, 16)
    assert flipped.dtype == torch.bool and flipped.is_cuda and not flipped.any() and info["n_flipped"] == 0 and info["root"] == want["root"]
    assert info["tree_edges"].dtype == torch.int64 and np.array_equal(info["tree_edges"].cpu().numpy(), want["tree"])
    edges, d2 = P.geometry.euclidean_minimum_spanning_tree(pc)
    assert edges.dtype == torch.int64 and d2.dtype == torch.float64 and edges.is_cuda and d2.is_cuda
    assert np.array_equal(edges.cpu().numpy(), golden["emst"][0]) and np.array_equal(d2.cpu().numpy().view(np.uint64), golden["emst"][1].view(np.uint64))
    loc = (3.0, -2.0, 40.0)
    assert pc.orient_normals_towards_camera_location(loc) is None and pc.device_normals() is nrm_t
    out = nrm_t.cpu().numpy()
    assert np.array_equal(out.view(np.uint32), ref.camera_reference(pts, want["normals"], loc).view(np.uint32))
    v = np.asarray(loc)[None, :] - pts.astype(np.float64)
    assert (ref._dot3(out.astype(np.float64), v) >= 0).all()
    assert pc.orient_normals_to_align_with_direction() is None
    assert np.array_equal(nrm_t.cpu().numpy().view(np.uint32), ref.direction_reference(out, (0, 0, 1)).view(np.uint32))
    before = nrm_t.cpu().numpy()
    assert pc.normalize_normals() is pc
    assert np.array_equal(nrm_t.cpu().numpy().view(np.uint32), ref.normalize_reference(before).view(np.uint32))
