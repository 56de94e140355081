"""CPU-side checks of the voxel point map: the ABI, the Python surface and its refusals before a device is touched, the numpy restatement
(tests/point_map_reference.py) against itself -- sequential arrival, the order of MERGE, the exactness lemma, the adaptive threshold -- and
the conditions the comparisons of tests/test_gpu_point_map.py rest on.  Needs no GPU."""
import inspect
import os
import re

import numpy as np
import pytest

import point_map_reference as pm
import voxel_reference as vr
from conftest import ROOT, pkg

ENTRY_POINTS = ["pcr_point_map_create", "pcr_point_map_create_on_grid", "pcr_point_map_destroy", "pcr_point_map_size", "pcr_point_map_read", "pcr_point_map_grid",
                "pcr_point_map_insert", "pcr_point_map_merge", "pcr_point_map_remove_far", "pcr_point_map_correspondences", "pcr_point_map_linearize",
                "pcr_registration_point_map"]


# ------------------------------------------------------------------------------------------ the boundary
@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_entry_point_is_declared_exported_and_prototyped(name):
    P = pkg()
    hdr = open(os.path.join(ROOT, "include", "pcr_hip.h")).read()
    m = re.search(r"\bint " + name + r"\(([^;]*)\);", hdr)
    assert m, name
    n_args = len([a for a in m.group(1).split(",") if a.strip()])
    assert name in P._lib.EXPORTS and len(P._lib.QUERY_PROTOTYPES[name][0]) == n_args
    assert hasattr(P._lib.load(), name)


def test_header_states_the_rule_and_the_unit_is_built():
    hdr = open(os.path.join(ROOT, "include", "pcr_hip.h")).read()
    sec = hdr[hdr.index("scan-to-map ICP on a voxel point map"):hdr.index("int pcr_registration_point_map(")]
    for word in ("MAP.", "ON A GRID, AT A POSE", "MERGE(A, B)", "MERGE IS NOT COMMUTATIVE", "INSERT(map, cloud, T)", "KISS-ICP's rule", "REMOVE_FAR", "ROW OF A SOURCE POINT AT T",
                 "EXACTNESS", "UPDATE.", "NOT the Umeyama fit", "LOOP.", "SUMS."):
        assert word in sec, word
    csrc = os.path.join(ROOT, "point-cloud-registration-with-global-refinement_amd", "csrc")
    assert os.path.exists(os.path.join(csrc, "pcr_pmap.hip")) and os.path.exists(os.path.join(csrc, "pcr_pmap.h"))
    assert re.search(r"^for f in .*\bpcr_pmap\b", open(os.path.join(csrc, "build.sh")).read(), re.M)
    assert '"pcr_pmap"' in open(os.path.join(ROOT, "tools", "pk_trans_scan.py")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "pcr_pmap.hip" in readme and "Umeyama" in readme and "AdaptiveThreshold" in readme
    assert "voxel point map" in open(os.path.join(ROOT, "DESIGN.md")).read()


def test_python_surface_and_defaults():
    P = pkg()
    R = P.registration
    sig = inspect.signature(R.registration_point_map).parameters
    assert list(sig) == ["source", "target_or_map", "max_correspondence_distance", "voxel_size", "init", "estimation_method", "criteria", "neighborhood",
                         "max_points_per_voxel"]
    assert sig["voxel_size"].default is None and sig["estimation_method"].default is None and sig["neighborhood"].default == 27 and sig["max_points_per_voxel"].default == 20
    sig = inspect.signature(R.scan_to_map_odometry_icp).parameters
    assert list(sig) == ["scans", "voxel_size", "max_correspondence_distance", "init", "estimation_method", "criteria", "neighborhood", "max_points_per_voxel", "motion_model",
                         "max_range", "grid_min", "adaptive_threshold"]
    assert list(inspect.signature(R.VoxelPointMap.__init__).parameters) == ["self", "target", "voxel_size", "max_points_per_voxel"]
    assert list(inspect.signature(R.VoxelPointMap.on_grid).parameters) == ["target", "voxel_size", "max_points_per_voxel", "grid_min", "transformation"]
    assert list(inspect.signature(R.VoxelPointMap.correspondences).parameters) == ["self", "source", "T", "max_correspondence_distance", "neighborhood"]
    assert list(inspect.signature(R.VoxelPointMap.linearize).parameters) == ["self", "source", "T", "max_correspondence_distance", "estimation_method", "neighborhood"]
    assert list(inspect.signature(R.AdaptiveThreshold.__init__).parameters) == ["self", "initial_threshold", "min_motion", "max_range"]
    M = R.VoxelPointMap
    assert M.__bases__ == (R._GrowingVoxelMap,) and M._C == "pcr_point_map" and M._NAME == "VoxelPointMap"
    for name in ("merge", "remove_far", "close", "__enter__", "__exit__", "__len__", "centered_grid_min", "cells", "counts", "points"):      # the frame's own
        assert name not in vars(M) and hasattr(M, name), name
    for name in ("starts", "normals", "grid_min", "origin", "to_point_cloud", "insert", "correspondences", "linearize", "on_grid"):
        assert name in vars(M), name
    assert P.o3d.pipelines.registration.registration_point_map is R.registration_point_map
    # the existing point-to-point estimator is what it was for every other call
    e = R.TransformationEstimationPointToPoint()._estimation()
    assert (e.kind, e.with_scaling, e.loss, e.loss_k) == (P._lib.EST_POINT_TO_POINT, 0, P._lib.LOSS_L2, 1.0)


class _NoDevice:
    """stands in for the context class: any use of a device inside the block fails the test"""

    @classmethod
    def current(cls):
        raise AssertionError("a device context was asked for")


def _host_cloud(P, n=5, normals=False):
    import torch
    pc = P.PointCloud()
    pc._xyz = torch.zeros((n, 3), dtype=torch.float32)
    if normals:
        pc._nrm = torch.zeros((n, 3), dtype=torch.float32)
    return pc


BAD = [dict(neighborhood=0), dict(neighborhood=6), dict(neighborhood=26), dict(max_points_per_voxel=0), dict(max_points_per_voxel=65), dict(max_points_per_voxel=2.5),
       dict(max_correspondence_distance=0.0), dict(max_correspondence_distance=-1.0), dict(max_correspondence_distance=float("nan")),
       dict(max_correspondence_distance=float("inf")), dict(max_correspondence_distance=None), dict(voxel_size=0.0), dict(voxel_size=float("nan")), dict(voxel_size=None)]


@pytest.mark.parametrize("bad", BAD, ids=[f"{k}={v}" for b in BAD for k, v in b.items()])
def test_bad_arguments_raise_value_error_before_a_device_is_touched(monkeypatch, bad):
    P = pkg()
    R = P.registration
    monkeypatch.setattr(P._lib, "Context", _NoDevice)
    args = dict(max_correspondence_distance=1.0, voxel_size=1.0, neighborhood=27, max_points_per_voxel=20)
    args.update(bad)
    with pytest.raises(ValueError, match="registration_point_map"):
        R.registration_point_map(_host_cloud(P), _host_cloud(P), **args)
    if "voxel_size" in bad or "max_points_per_voxel" in bad:
        with pytest.raises(ValueError, match="VoxelPointMap"):
            R.VoxelPointMap(_host_cloud(P), args["voxel_size"], args["max_points_per_voxel"])


def test_other_host_side_refusals(monkeypatch):
    P = pkg()
    R = P.registration
    monkeypatch.setattr(P._lib, "Context", _NoDevice)
    with pytest.raises(ValueError, match="with_scaling"):
        R.registration_point_map(_host_cloud(P), _host_cloud(P), 1.0, 1.0, estimation_method=R.TransformationEstimationPointToPoint(True))
    with pytest.raises(RuntimeError, match="neither TransformationEstimationPointToPoint nor"):
        R.registration_point_map(_host_cloud(P), _host_cloud(P), 1.0, 1.0, estimation_method=R.TransformationEstimationForGeneralizedICP())
    with pytest.raises(TypeError, match="PointCloud or a VoxelPointMap"):
        R.registration_point_map(_host_cloud(P), np.zeros((4, 3)), 1.0, 1.0)
    with pytest.raises(RuntimeError, match="at least one point"):
        R.VoxelPointMap(P.PointCloud(), 1.0)
    with pytest.raises(ValueError, match="needs a grid_min"):
        R.VoxelPointMap.on_grid(_host_cloud(P), 1.0, transformation=np.eye(4))
    scans = [_host_cloud(P), _host_cloud(P)]
    with pytest.raises(ValueError, match="exactly one of max_correspondence_distance and adaptive_threshold"):
        R.scan_to_map_odometry_icp(scans, 1.0)
    with pytest.raises(ValueError, match="exactly one of max_correspondence_distance and adaptive_threshold"):
        R.scan_to_map_odometry_icp(scans, 1.0, 1.0, adaptive_threshold=R.AdaptiveThreshold(2.0, 0.1, 100.0))
    with pytest.raises(TypeError, match="AdaptiveThreshold"):
        R.scan_to_map_odometry_icp(scans, 1.0, adaptive_threshold=2.0)
    with pytest.raises(RuntimeError, match="scan 1 has no normals"):
        R.scan_to_map_odometry_icp([_host_cloud(P, normals=True), _host_cloud(P)], 1.0, 1.0, estimation_method=R.TransformationEstimationPointToPlane())
    for bad in (dict(initial_threshold=0.0), dict(min_motion=-1.0), dict(max_range=float("nan"))):
        with pytest.raises(ValueError, match="AdaptiveThreshold: " + next(iter(bad))):
            R.AdaptiveThreshold(**{**dict(initial_threshold=2.0, min_motion=0.1, max_range=100.0), **bad})
    # good arguments: the next thing either call wants is the device
    with pytest.raises(AssertionError, match="device context"):
        R.VoxelPointMap(_host_cloud(P), 1.0)
    with pytest.raises(AssertionError, match="device context"):
        R.registration_point_map(_host_cloud(P), _host_cloud(P), 1.0, 1.0)
    with pytest.raises(AssertionError, match="device context"):
        R.scan_to_map_odometry_icp(scans, 1.0, 1.0)


# ------------------------------------------------------------------------------------------ the restatement against itself
def _clouds(seed, n=(300, 200, 250), span=4.0, normals=True):
    rng = np.random.default_rng(seed)
    out = []
    for k, m in enumerate(n):
        xyz = rng.uniform(0.0, span, (m, 3)).astype(np.float32)
        nrm = rng.normal(size=(m, 3)).astype(np.float32) if normals else None
        a = 0.1 * k
        T = np.eye(4)
        T[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
        T[:3, 3] = [0.3 * k, -0.2 * k, 0.05]
        out.append((xyz, nrm, T))
    return out


@pytest.mark.parametrize("M", [1, 3, 20])
@pytest.mark.parametrize("normals", [False, True])
def test_sequential_arrival_equals_create_insert_insert(M, normals):
    clouds = _clouds(5, normals=normals)
    g = np.array([-8.0, -8.0, -8.0])
    m = pm.build_map(clouds[0][0], clouds[0][1], 1.0, M, g, clouds[0][2])
    for xyz, nrm, T in clouds[1:]:
        m = pm.insert(m, xyz, nrm, T)
    cells, lists = pm.sequential(clouds, 1.0, M, g)
    assert pm.equals_sequential(m, cells, lists)
    assert m.counts.max() <= M and m.counts.sum() == len(m)
    if M <= 3:
        assert (m.counts == M).sum() > 20 and len(m) < sum(len(c[0]) for c in clouds) - 100                  # many cells were cut
    else:
        assert (m.counts < M).any()
    assert np.array_equal(m.starts, np.concatenate([[0], np.cumsum(m.counts)[:-1]]))
    key = vr.morton3(m.cells)
    assert (key[1:] > key[:-1]).all()


def test_merge_is_not_commutative_where_a_cell_overflows():
    (xa, na, _), (xb, nb, _), _ = _clouds(9)
    g = np.array([-1.0, -1.0, -1.0])
    A, B = pm.build_map(xa, na, 1.0, 4, g), pm.build_map(xb, nb, 1.0, 4, g)
    ab, ba = pm.merge(A, B), pm.merge(B, A)
    assert np.array_equal(ab.cells, ba.cells) and np.array_equal(ab.counts, ba.counts)
    ca = dict(zip(map(tuple, A.cells), A.counts)); cb = dict(zip(map(tuple, B.cells), B.counts))
    differs = same = 0
    for c, s, k in zip(ab.cells, ab.starts, ab.counts):
        na_, nb_ = ca.get(tuple(c), 0), cb.get(tuple(c), 0)
        assert k == min(4, na_ + nb_)
        rows_ab = {ab.points[r].tobytes() for r in range(s, s + k)}
        rows_ba = {ba.points[r].tobytes() for r in range(s, s + k)}
        if na_ + nb_ > 4 and na_ and nb_:
            assert rows_ab != rows_ba                                   # A's members first and B's tail cut, or the other way round
            sa = int(A.starts[[tuple(x) for x in A.cells].index(tuple(c))])
            assert [ab.points[s + j].tobytes() for j in range(na_)] == [A.points[sa + j].tobytes() for j in range(na_)]
            differs += 1
        else:
            assert rows_ab == rows_ba
            same += 1
    assert differs > 10 and same > 10
    # associative: the cut of a prefix is a prefix of the cut
    C = pm.build_map(*_clouds(9)[2][:2], 1.0, 4, g)
    l, r = pm.merge(pm.merge(A, B), C), pm.merge(A, pm.merge(B, C))
    assert vr.bits_equal(l.points, r.points) and vr.bits_equal(l.normals, r.normals) and np.array_equal(l.cells, r.cells)


def test_remove_far_is_per_row():
    xyz, nrm, _ = _clouds(3, n=(400,))[0]
    m = pm.build_map(xyz, nrm, 1.0, 8)
    out = pm.remove_far(m, [2.0, 2.0, 2.0], 1.5)
    keep = pm.distance2(m.points, [2.0, 2.0, 2.0]) < 2.25
    assert vr.bits_equal(out.points, m.points[keep]) and len(out.cells) < len(m.cells)
    thinned = sum(1 for c, k in zip(out.cells, out.counts) if k < dict(zip(map(tuple, m.cells), m.counts))[tuple(c)])
    assert thinned > 5                                                  # cells that lost some rows and kept others
    with pytest.raises(ValueError, match="empty"):
        pm.remove_far(m, [100.0, 0.0, 0.0], 1.0)


@pytest.fixture(scope="module")
def pair899(small_pair):
    src = vr.voxel_reference(small_pair["source"], 0.3).points
    tgt = vr.voxel_reference(small_pair["target"], 0.3).points
    assert (len(src), len(tgt)) == (6897, 7074)
    return src, tgt, small_pair["T_fgr"]


def test_exactness_lemma_against_brute_force(pair899):
    src, tgt, T = pair899
    m = pm.build_map(tgt, None, 1.0, 20)
    for dist in (0.3, 1.0):                                             # <= voxel: the rows of neighbourhood 27 are the exact nearest within the distance
        assert np.array_equal(pm.rows_at(m, src, T, dist, 27), pm.brute_force_rows(m, src, T, dist)), dist
    # neighbourhoods 1 and 7 are approximations, a distance above the voxel is only the rule: both in fact differ from the exact search here
    exact = pm.brute_force_rows(m, src, T, 1.0)
    for nbh in (1, 7):
        got = pm.rows_at(m, src, T, 1.0, nbh)
        assert len(got) <= len(exact) and not np.array_equal(got, exact), nbh
    assert not np.array_equal(pm.rows_at(m, src, T, 2.5, 27), pm.brute_force_rows(m, src, T, 2.5))


def test_conditions_of_the_gpu_comparisons_on_pair_899(pair899):
    """the 1.0 m map of the 0.3 m target: 1853 cells, the largest of 36 members; M = 8 cuts 115 cells and M = 20 cuts 7 (so the cut is in every
    map comparison); at T_fgr with max_correspondence_distance 1.0, 0.88 of the source points have a row (so the sums are over most of the source)"""
    src, tgt, T = pair899
    whole = pm.build_map(tgt, None, 1.0, 64)
    assert len(whole.cells) == 1853 and whole.counts.max() == 36 and len(whole) == len(tgt)
    cut8, cut20 = int((whole.counts > 8).sum()), int((whole.counts > 20).sum())
    print(f"cells cut at M = 8: {cut8}, at M = 20: {cut20}")
    assert cut8 > 100 and cut20 >= 1
    for M, cut in ((8, cut8), (20, cut20)):
        m = pm.build_map(tgt, None, 1.0, M)
        assert np.array_equal(m.cells, whole.cells) and (m.counts == np.minimum(whole.counts, M)).all() and int((m.counts == M).sum()) >= cut
    rows = pm.rows_at(pm.build_map(tgt, None, 1.0, 20), src, T, 1.0, 27)
    print(f"source points with a row at T_fgr, distance 1.0: {len(rows) / len(src):.3f}")
    assert len(rows) >= 0.5 * len(src)


def test_linearize_of_the_restatement():
    """the sums do not depend on their grouping beyond rounding, and a source on its own map has zero residuals"""
    xyz, nrm, _ = _clouds(4, n=(500,))[0]
    m = pm.build_map(xyz, nrm, 1.0, 64)
    s = pm.linearize(m, xyz, np.eye(4), 0.5, 27, pm.POINT_TO_PLANE)
    assert s["rows"] == len(xyz) and s["sum_d2"] == 0.0 and not s["JTr"].any()
    T = np.eye(4); T[:3, 3] = [0.02, -0.01, 0.03]
    for kind in (pm.POINT_TO_POINT, pm.POINT_TO_PLANE):
        for loss in (pm.L2, pm.L1, pm.GM):
            a, b = pm.linearize(m, xyz, T, 0.5, 27, kind, loss, 0.3), pm.linearize(m, xyz, T, 0.5, 27, kind, loss, 0.3, chunk=64)
            assert a["rows"] == b["rows"] > 400
            assert (np.abs(a["JTJ"] - b["JTJ"]) <= 1e-12 * a["mag_JTJ"]).all() and (np.abs(a["JTr"] - b["JTr"]) <= 1e-12 * a["mag_JTr"]).all()
    # point to point, L2, a small translation: one update brings the cloud back but for the few points that matched a neighbour
    s = pm.linearize(m, xyz, T, 0.5, 27, pm.POINT_TO_POINT)
    U = pm.solve_update(s["JTJ"], s["JTr"])
    assert np.abs((U @ T)[:3, 3]).max() < 0.05 * np.abs(T[:3, 3]).max()
    assert pm.linearize(m, xyz, U @ T, 0.5, 27, pm.POINT_TO_POINT)["sum_d2"] < 0.01 * s["sum_d2"]


def test_adaptive_threshold_arithmetic():
    R = pkg().registration
    a = R.AdaptiveThreshold(2.0, 0.1, 100.0)
    assert a.sse == 4.0 and a.samples == 1 and a.sigma == 2.0
    P = np.eye(4); P[:3, 3] = [1.0, 2.0, 3.0]
    E = P.copy(); E[:3, 3] += P[:3, :3] @ np.array([0.3, 0.0, 0.4])      # a pure translation of 0.5 in the predicted frame
    assert abs(a.update(P, E) - 0.5) < 1e-15
    assert abs(a.sse - 4.25) < 1e-15 and a.samples == 2 and abs(a.sigma - np.sqrt(4.25 / 2)) < 1e-15
    th = 0.02                                                            # a pure rotation: e = 2 max_range sin(theta / 2)
    Rz = np.eye(4); Rz[:2, :2] = [[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]
    e = a.update(P, P @ Rz)
    assert abs(e - 200.0 * np.sin(0.01)) < 1e-9 and a.samples == 3 and abs(a.sse - (4.25 + e * e)) < 1e-12
    before = (a.sse, a.samples)
    small = P.copy(); small[:3, 3] += [0.05, 0.0, 0.0]                   # e = 0.05 <= min_motion: not a sample
    assert abs(a.update(P, small) - 0.05) < 1e-12 and (a.sse, a.samples) == before
    assert abs(a.update(P, P)) < 1e-12 and (a.sse, a.samples) == before
    assert abs(pm.model_error(P, P @ Rz, 100.0) - e) < 1e-15
