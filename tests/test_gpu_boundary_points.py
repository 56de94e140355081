"""Boundary points on the device against the numpy restatement of the rule (tests/boundary_reference.py; the rule: include/pcr_hip.h) on
the same float32 points and normals: row lengths, largest gaps and verdicts on a LiDAR scan, the outputs among each other, shapes whose
boundary is known, the smallest and the degenerate shapes by brute force, the errors, and the Python calls built on the entry point.

Main input: the source of golden pair 899 after ``voxel_down_sample(0.2)`` and ``estimate_normals(Hybrid(1.0, 30))`` (about 9.5k points),
four parameter sets.  Sparse ring LiDAR is mostly rim at these radii, so both classes are large.

Bounds, derived and not measured.  GAP_TOL = 1e-12 rad: everything up to the arguments of atan2 is fixed bit for bit by the rule; the angles
are at most pi in magnitude and atan2 is good to a few ulp of that, 4.4e-16 each; a gap is one difference of two such angles (or 2 pi minus
one), so its error is at most about 3e-15, and 1e-12 leaves more than two orders of margin.  The row lengths are integers of a bit-defined
rule: equal.  The verdict is gap > T: a row with |gap_ref - T| <= RIM = 1e-9 rad is left out of the mask comparison, and at most
RIM_SHARE = 1e-3 of the rows of a case may be left out (the constant of the ISS test)."""
import ctypes as C

import numpy as np
import pytest

import boundary_reference as bref
from conftest import pkg

pytestmark = pytest.mark.gpu

GAP_TOL, RIM, RIM_SHARE = 1e-12, 1e-9, 1e-3
# (radius, max_nn, angle_threshold)
CASES = [(0.6, 30, 90.0), (1.0, 30, 90.0), (1.0, 16, 120.0), (2.0, 200, 60.0)]
OUTPUTS = ("mask", "xyz", "idx", "gap", "counts")


@pytest.fixture(scope="module")
def P():
    return pkg()


def _cloud(P, pts, nrm):
    pc = P.PointCloud(pts)
    pc.normals = nrm
    return pc


def _device(P, pts, nrm, params):
    """the private call -> dict(idx, mask, gap, counts), on the host"""
    idx, mask, gap, counts = P.geometry._boundary_points(_cloud(P, pts, nrm), *params)
    return dict(idx=idx.cpu().numpy(), mask=mask, gap=gap, counts=counts)


def _raw(P, pts, nrm, params, want=OUTPUTS, n=None, null=()):
    """pcr_boundary_points itself with the optional outputs named in `want` -> (status, count, dict of the outputs asked for)"""
    import torch
    ctx = P._lib.Context.current()
    rows = len(pts)
    n = rows if n is None else n
    d = torch.from_numpy(np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 3)).cuda()
    dn = torch.from_numpy(np.ascontiguousarray(nrm, dtype=np.float32).reshape(-1, 3)).cuda()
    buf = dict(mask=torch.full((max(rows, 1),), 7, dtype=torch.uint8, device="cuda"), xyz=torch.zeros((max(rows, 1), 3), dtype=torch.float32, device="cuda"),
               idx=torch.full((max(rows, 1),), -1, dtype=torch.int64, device="cuda"), gap=torch.full((max(rows, 1),), -1.0, dtype=torch.float64, device="cuda"),
               counts=torch.full((max(rows, 1),), -1, dtype=torch.int32, device="cuda"))
    ptr = lambda k: C.c_void_p(buf[k].data_ptr()) if k in want else None
    m = C.c_int64(-1)
    radius, max_nn, angle = params
    rc = ctx.lib.pcr_boundary_points(ctx.handle, None if "xyz" in null else C.c_void_p(d.data_ptr()), None if "normals" in null else C.c_void_p(dn.data_ptr()),
                                     C.c_int64(n), C.c_double(radius), C.c_int(max_nn), C.c_double(angle), ptr("mask"), ptr("xyz"), ptr("idx"), C.byref(m),
                                     ptr("gap"), ptr("counts"))
    msg = ctx.lib.pcr_last_error(ctx.handle)
    kk = max(int(m.value), 0)
    out = {k: buf[k][:kk if k in ("xyz", "idx") else rows].cpu().numpy() for k in want}
    if "mask" in out:
        out["mask"] = out["mask"].astype(bool)
    return rc, int(m.value), out, (msg.decode() if msg else "")


def _compare(dev, ref, what, share=None):
    """row lengths, gaps and verdicts of one device result against the restatement; returns the rows left out of the mask comparison"""
    n = len(ref["gap"])
    err = np.abs(dev["gap"] - ref["gap"])
    rim = np.abs(ref["gap"] - ref["T"]) <= RIM
    print(f"{what}: n = {n}, boundary points: restatement {int(ref['mask'].sum())}, device {int(dev['mask'].sum())}; rows left out {int(rim.sum())}; "
          f"worst gap error {float(err.max()) if n else 0.0:.3e} rad; row lengths {int(ref['counts'].min()) if n else 0}..{int(ref['counts'].max()) if n else 0}")
    assert dev["mask"].shape == (n,) and dev["gap"].shape == (n,) and dev["counts"].shape == (n,)
    assert dev["mask"].dtype == bool and dev["gap"].dtype == np.float64 and dev["counts"].dtype == np.int32
    assert np.array_equal(dev["counts"], ref["counts"]), (what, int((dev["counts"] != ref["counts"]).sum()))
    assert (err <= GAP_TOL).all(), (what, float(err.max()))
    assert np.array_equal(dev["mask"][~rim], ref["mask"][~rim]), (what, int((dev["mask"] != ref["mask"])[~rim].sum()))
    assert np.array_equal(dev["idx"], np.nonzero(dev["mask"])[0]) and dev["idx"].dtype == np.int64
    if share is not None:
        assert rim.sum() <= share * n, (what, int(rim.sum()))
    return int(rim.sum())


# ---------------------------------------------------------------------------------------------------- main input
@pytest.fixture(scope="module")
def cloud(P, small_pair):
    """(source cloud of pair 899 at 0.2 m with Hybrid(1.0, 30) normals and colours, its float32 points, its float32 normals)"""
    pc = P.PointCloud(small_pair["source"]).voxel_down_sample(0.2)
    pc.estimate_normals(P.KDTreeSearchParamHybrid(radius=1.0, max_nn=30))
    pc.colors = np.random.default_rng(3).random((len(pc), 3))
    return pc, pc.points.astype(np.float32), pc.normals.astype(np.float32)


@pytest.fixture(scope="module")
def references(cloud):
    """{case: restatement}, computed once (brute force in chunks of 1000 rows)"""
    return {c: bref.boundary(cloud[1], cloud[2], *c, chunk=1000) for c in CASES}


@pytest.fixture(scope="module")
def devices(P, cloud):
    return {c: _device(P, cloud[1], cloud[2], c) for c in CASES}


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("case", CASES, ids=[f"{c[0]}-{c[1]}-{c[2]}" for c in CASES])
def test_row_lengths_gaps_and_verdicts_against_the_restatement(cloud, references, devices, case):
    ref, dev = references[case], devices[case]
    n = len(cloud[1])
    assert 0.05 * n < ref["mask"].sum() < 0.95 * n                        # both classes are large
    assert ref["counts"].max() == case[1] and ref["counts"].min() < case[1]          # rows cut by max_nn and rows that are not
    _compare(dev, ref, f"case {case}", share=RIM_SHARE)


# ---------------------------------------------------------------------------------------------------------------- 2
def test_outputs_agree_with_each_other(P, cloud, devices):
    pc, pts, nrm = cloud
    case = CASES[1]
    dev = devices[case]
    rc, m, out, _ = _raw(P, pts, nrm, case)
    assert rc == 0 and m == len(out["idx"]) == int(out["mask"].sum())
    assert np.array_equal(out["mask"], dev["mask"]) and out["gap"].tobytes() == dev["gap"].tobytes() and np.array_equal(out["counts"], dev["counts"])
    assert np.array_equal(out["idx"], np.nonzero(out["mask"])[0]) and (np.diff(out["idx"]) > 0).all()
    assert out["xyz"].tobytes() == pts[out["idx"]].tobytes()               # bit for bit
    assert np.array_equal(P.boundary_point_indices(pc, *case), out["idx"]) and P.boundary_point_indices(pc, *case).dtype == np.int64
    # every optional output omitted but one: that output is unchanged
    for k in OUTPUTS:
        rc1, m1, one, _ = _raw(P, pts, nrm, case, want=(k,))
        assert rc1 == 0 and m1 == m and one[k].tobytes() == out[k].tobytes(), k
    # every optional pointer null: accepted, the count alone comes back
    rc0, m0, _, _ = _raw(P, pts, nrm, case, want=())
    assert rc0 == 0 and m0 == m


# ---------------------------------------------------------------------------------------------------------------- 3
def test_two_runs_give_the_same_bits(P, cloud, devices):
    for case in (CASES[0], CASES[3]):
        a, b = devices[case], _device(P, cloud[1], cloud[2], case)
        for k in ("mask", "idx", "gap", "counts"):
            assert a[k].tobytes() == b[k].tobytes(), (case, k)


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.fixture(scope="module")
def grid():
    pts, nrm = bref.grid_cloud(32)
    on_x, on_y = (pts[:, 0] == 0) | (pts[:, 0] == 31), (pts[:, 1] == 0) | (pts[:, 1] == 31)
    return pts, nrm, on_x | on_y, on_x & on_y


def test_grid_perimeter_and_corners(P, grid):
    pts, nrm, perimeter, corner = grid
    assert perimeter.sum() == 124 and corner.sum() == 4
    at90 = _device(P, pts, nrm, (1.5, 30, 90.0))
    _compare(at90, bref.boundary(pts, nrm, 1.5, 30, 90.0), "grid at 90")
    assert np.array_equal(at90["mask"], perimeter)
    at200 = _device(P, pts, nrm, (1.5, 30, 200.0))
    assert np.array_equal(at200["mask"], corner)
    deg = np.degrees(at90["gap"])
    assert np.abs(deg[~perimeter] - 45.0).max() < 1e-9 and np.abs(deg[perimeter & ~corner] - 180.0).max() < 1e-9 and np.abs(deg[corner] - 270.0).max() < 1e-9
    # every normal negated: the same mask, the same gaps
    neg = _device(P, pts, -nrm, (1.5, 30, 90.0))
    assert np.array_equal(neg["mask"], perimeter) and np.abs(neg["gap"] - at90["gap"]).max() <= GAP_TOL
    # the grid turned by a fixed rotation, normals turned with it: the same 124 and 4 points
    ax = np.array([0.3, -0.5, 0.81]); ax /= np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + np.sin(0.7) * K + (1.0 - np.cos(0.7)) * (K @ K)
    rp, rn = (pts.astype(np.float64) @ R.T + np.array([3.0, -2.0, 1.0])).astype(np.float32), (nrm.astype(np.float64) @ R.T).astype(np.float32)
    assert np.array_equal(_device(P, rp, rn, (1.5, 30, 90.0))["mask"], perimeter)
    assert np.array_equal(_device(P, rp, rn, (1.5, 30, 200.0))["mask"], corner)


def test_closed_and_cut_sphere(P):
    pts, nrm = bref.fibonacci_sphere(4096)
    ref = bref.boundary(pts, nrm, 0.12, 30, 90.0)
    dev = _device(P, pts, nrm, (0.12, 30, 90.0))
    assert _compare(dev, ref, "sphere") == 0
    assert not dev["mask"].any() and abs(np.degrees(dev["gap"].max()) - 48.1) < 0.1 and 13 <= dev["counts"].min() and dev["counts"].max() <= 17
    pts, nrm = bref.cut_sphere(4096, 0.5)
    ref = bref.boundary(pts, nrm, 0.12, 30, 90.0)
    dev = _device(P, pts, nrm, (0.12, 30, 90.0))
    assert len(pts) == 3072 and _compare(dev, ref, "cut sphere") == 0
    assert dev["mask"].sum() == 89 and (pts[dev["mask"], 2] > 0.5 - 0.12).all()


# ---------------------------------------------------------------------------------------------------------------- 5
def _random_cloud(n, seed, spread=1.0):
    rng = np.random.default_rng(seed)
    nrm = rng.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return (rng.random((n, 3)) * spread).astype(np.float32), nrm.astype(np.float32)


@pytest.mark.parametrize("n", [1, 2, 3, 9, 65, 257])
def test_small_clouds_by_brute_force(P, n):
    pts, nrm = _random_cloud(n, 300 + n)
    for max_nn in (1, 2, 8):
        ref = bref.boundary(pts, nrm, 0.6, max_nn, 90.0)
        dev = _device(P, pts, nrm, (0.6, max_nn, 90.0))
        _compare(dev, ref, f"n = {n}, max_nn = {max_nn}")
        if max_nn == 1:                                                   # the row holds the point alone
            assert (dev["counts"] == 1).all() and not dev["mask"].any() and (dev["gap"] == 0).all()
        if n >= 65 and max_nn == 8:
            assert (ref["counts"] == 8).any() and 0 < ref["mask"].sum()    # rows cut by max_nn; the comparison is not empty
    if n >= 2:
        full = bref.boundary(pts, nrm, 0.6, 30, 90.0)
        _compare(_device(P, pts, nrm, (0.6, 30, 90.0)), full, f"n = {n}, max_nn = 30")


# ---------------------------------------------------------------------------------------------------------------- 6
def test_full_rows_of_200_members(P):
    rng = np.random.default_rng(41)
    pts = rng.normal(0.0, 0.2, size=(300, 3)).astype(np.float32)
    nrm = rng.normal(size=(300, 3)); nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    ref = bref.boundary(pts, nrm, 5.0, 200, 90.0)
    assert (ref["counts"] == 200).all() and (ref["m"] == 199).all()
    assert 0 < ref["mask"].sum() < 300 and not (np.abs(ref["gap"] - ref["T"]) <= 1e-6).any()
    assert _compare(_device(P, pts, nrm, (5.0, 200, 90.0)), ref, "blob, max_nn = 200") == 0
    ref8 = bref.boundary(pts, nrm, 5.0, 8, 90.0)
    assert (ref8["counts"] == 8).all()
    _compare(_device(P, pts, nrm, (5.0, 8, 90.0)), ref8, "blob, max_nn = 8")


# ---------------------------------------------------------------------------------------------------------------- 7
def test_coincident_points_have_no_boundary(P):
    pts = np.repeat(np.array([[0.25, -1.5, 3.0]], np.float32), 50, axis=0)
    nrm = np.tile(np.array([0.0, 0.6, 0.8], np.float32), (50, 1))
    for max_nn in (8, 30, 200):
        dev = _device(P, pts, nrm, (0.5, max_nn, 90.0))
        assert not dev["mask"].any() and (dev["gap"] == 0).all() and (dev["counts"] == min(50, max_nn)).all() and len(dev["idx"]) == 0


def test_members_on_the_normal_line_are_skipped(P):
    t = np.arange(10, dtype=np.float32) * np.float32(0.125)              # exact in float32
    pts = np.array([0.25, 0.5, 0.75], np.float32) + t[:, None] * np.array([0.0, 0.0, 1.0], np.float32)
    nrm = np.tile(np.array([0.0, 0.0, 1.0], np.float32), (10, 1))
    dev = _device(P, pts, nrm, (5.0, 30, 90.0))
    assert (dev["counts"] == 10).all() and not dev["mask"].any() and (dev["gap"] == 0).all()
    # one point off the line: every row on the line sees one direction, a gap of 2 pi
    pts2 = np.concatenate([pts, np.array([[1.25, 0.5, 0.75]], np.float32)]); nrm2 = np.concatenate([nrm, nrm[:1]])
    ref = bref.boundary(pts2, nrm2, 5.0, 30, 90.0)
    dev = _device(P, pts2, nrm2, (5.0, 30, 90.0))
    _compare(dev, ref, "line and one point")
    assert (dev["gap"][:10] == 2.0 * np.pi).all() and dev["mask"][:10].all()


def test_undecided_rows(P):
    pts, nrm = _random_cloud(65, 77)
    nrm[5] = 0.0
    nrm[17, 1] = np.nan
    pts[40, 2] = np.nan
    ref = bref.boundary(pts, nrm, 0.6, 30, 90.0)
    assert ref["counts"][40] == 0 and not (ref["idx"] == 40).any()         # the NaN point finds nothing and is nobody's neighbour
    assert ref["counts"][5] > 1 and ref["counts"][17] > 1
    dev = _device(P, pts, nrm, (0.6, 30, 90.0))
    for row in (5, 17, 40):
        assert not dev["mask"][row] and dev["gap"][row] == 0.0, row
    _compare(dev, ref, "zero normal, NaN normal, NaN point")               # every other row as well
    # ... and the same rows without the three: the NaN point changed nobody's row
    inf = pts.copy(); inf[40] = [np.inf, 0.0, -np.inf]
    dev_inf = _device(P, inf, nrm, (0.6, 30, 90.0))
    for k in ("mask", "gap", "counts"):
        assert dev_inf[k].tobytes() == dev[k].tobytes(), k


# ---------------------------------------------------------------------------------------------------------------- 8
def test_empty_cloud(P):
    rc, m, out, _ = _raw(P, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), (1.0, 30, 90.0))
    assert rc == 0 and m == 0 and len(out["idx"]) == 0
    rc, m, _, _ = _raw(P, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), (1.0, 30, 90.0), null=("xyz", "normals"))
    assert rc == 0 and m == 0
    idx, mask, gap, counts = P.geometry._boundary_points(P.PointCloud(), 1.0)
    assert len(idx) == 0 and mask.shape == gap.shape == counts.shape == (0,)
    assert P.boundary_point_indices(P.PointCloud(), 1.0).shape == (0,)


def test_bad_arguments_through_the_raw_call(P):
    pts, nrm = _random_cloud(65, 1)
    good = (0.6, 30, 90.0)
    bad = [((0.0, 30, 90.0), {}), ((-1.0, 30, 90.0), {}), ((float("nan"), 30, 90.0), {}), ((float("inf"), 30, 90.0), {}),
           ((0.6, 0, 90.0), {}), ((0.6, 201, 90.0), {}), ((0.6, -1, 90.0), {}),
           ((0.6, 30, float("nan")), {}), ((0.6, 30, float("inf")), {}), ((0.6, 30, -0.5), {}), ((0.6, 30, 360.5), {}),
           (good, dict(n=-1)), (good, dict(n=2 ** 31)), (good, dict(null=("xyz",))), (good, dict(null=("normals",)))]
    for params, kw in bad:
        rc, m, out, msg = _raw(P, pts, nrm, params, **kw)
        assert rc == P._lib.PCR_EINVAL and "boundary_points" in msg, (params, kw, rc, msg)
        assert (out["gap"] == -1.0).all() and (out["counts"] == -1).all() and (out["mask"] == 1).all()          # nothing was written
    # the limits themselves are accepted
    for params in ((0.6, 1, 0.0), (0.6, 200, 360.0)):
        rc, m, out, _ = _raw(P, pts, nrm, params)
        assert rc == 0 and m == int(out["mask"].sum())
    assert not _raw(P, pts, nrm, (0.6, 200, 360.0))[2]["mask"].any()         # no gap exceeds 2 pi
    # the Python calls raise on the host
    for call in (lambda: _cloud(P, pts, nrm).compute_boundary_points(-1.0), lambda: P.remove_boundary_points(_cloud(P, pts, nrm), 1.0, max_nn=0)):
        with pytest.raises(ValueError, match="compute_boundary_points"):
            call()
    with pytest.raises(RuntimeError, match="No normals"):
        P.PointCloud(pts).compute_boundary_points(1.0)


# ---------------------------------------------------------------------------------------------------------------- 9
def test_compute_and_remove_boundary_points(P, cloud, devices):
    import torch
    pc, pts, nrm = cloud
    case = CASES[1]
    dev = devices[case]
    rim, mask = pc.compute_boundary_points(*case)
    assert isinstance(mask, torch.Tensor) and mask.dtype == torch.bool and mask.is_cuda and mask.shape == (len(pc),)
    assert np.array_equal(mask.cpu().numpy(), dev["mask"])
    rest, removed = P.remove_boundary_points(pc, *case)
    assert isinstance(removed, torch.Tensor) and removed.dtype == torch.int64 and removed.is_cuda
    assert np.array_equal(removed.cpu().numpy(), dev["idx"])
    kept = np.nonzero(~dev["mask"])[0]
    assert isinstance(rim, P.PointCloud) and isinstance(rest, P.PointCloud) and len(rim) + len(rest) == len(pc) and len(rim) == len(dev["idx"])
    for part, rows in ((rim, dev["idx"]), (rest, kept)):                   # the two clouds partition the input, attributes bit for bit
        assert part.device_xyz().cpu().numpy().tobytes() == pts[rows].tobytes()
        assert part.has_normals() and part.device_normals().cpu().numpy().tobytes() == nrm[rows].tobytes()
        assert part.has_colors() and np.array_equal(part.colors, pc.colors[rows])
    # default arguments are Open3D's
    assert np.array_equal(pc.compute_boundary_points(1.0)[1].cpu().numpy(), dev["mask"])
    # the recipe: ISS keypoints that are not rim points pick the rows of a full-cloud feature
    iss = P.iss_keypoint_indices(pc, 1.0, 0.8)
    inner = np.setdiff1d(iss, P.boundary_point_indices(pc, *case))
    print(f"ISS keypoints {len(iss)}, of them not on the rim {len(inner)}")
    assert 0 < len(inner) <= len(iss) and not dev["mask"][inner].any()
    reg = P.o3d.pipelines.registration
    full = reg.compute_fpfh_feature(pc, P.KDTreeSearchParamHybrid(radius=1.0, max_nn=30))
    sel = full.select_by_index(inner)
    assert isinstance(sel, reg.Feature) and sel.num() == len(inner) and np.array_equal(sel.data, full.data[:, inner])
    assert sel.num() == len(pc.select_by_index(inner))
