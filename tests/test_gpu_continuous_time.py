"""Per-point times, deskewing and the continuous-time iteration on the device against the numpy restatement of their rule
(tests/continuous_time_reference.py): the times through the cloud's methods, pcr_deskew coordinate by coordinate, one linearisation entry by entry
with its matches exactly, the rigid code at equal poses, the trajectories of the loop, the planted sweep, the recipes and the refusals.  Pair 899
with both clouds at voxel 0.3 against a 1.0 m map with M = 20 (the clouds of tests/test_gpu_point_map.py), and clouds of tens of points.  What the
comparisons rest on is checked on the CPU in tests/test_continuous_time_api.py."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest

import continuous_time_reference as ct
import point_map_reference as pm
import voxel_reference as vr
from conftest import pkg, pose_error
from test_continuous_time_api import PLANTED_END_M, PLANTED_END_RAD, motion, planted_sweep, skewed_drive

pytestmark = pytest.mark.gpu

MAP_VOXEL = 1.0
LOSS = {"l2": pm.L2, "l1": pm.L1, "gm": pm.GM}
KIND = {"point": pm.POINT_TO_POINT, "plane": pm.POINT_TO_PLANE}
GM_K = 0.5


@pytest.fixture(scope="module")
def P():
    return pkg()


@pytest.fixture(scope="module")
def clouds(P, small_pair):
    """pair 899 at voxel 0.3 with KNN-20 normals (6897 / 7074 points), as tests/test_gpu_point_map.py makes them; the source carries the azimuth of
    its points as times"""
    out = {}
    for key in ("source", "target"):
        pc = P.PointCloud(small_pair[key]).voxel_down_sample(0.3)
        pc.estimate_normals(P.KDTreeSearchParamKNN(knn=20))
        out[key] = pc
        out[key + "_xyz"] = pc._xyz.cpu().numpy()
        out[key + "_nrm"] = pc._nrm.cpu().numpy()
    assert (len(out["source"]), len(out["target"])) == (6897, 7074)
    out["source_t"] = ct.azimuth_alpha(out["source_xyz"])
    out["source"].times = out["source_t"]
    return out


@pytest.fixture(scope="module")
def ref_map(clouds):
    return pm.build_map(clouds["target_xyz"], clouds["target_nrm"], MAP_VOXEL, 20)


@pytest.fixture(scope="module")
def dev_map(P, clouds):
    m = P.registration.VoxelPointMap(clouds["target"], MAP_VOXEL, 20)
    yield m
    m.close()


@pytest.fixture(scope="module")
def pose_pair(small_pair):
    """the begin and end pose of the linearisations: T_fgr and a pose 0.3 m and 2 degrees further"""
    T_b = np.array(small_pair["T_fgr"], np.float64)
    return T_b, T_b @ motion(2.0, [0.3, -0.1, 0.05])


def _cloud(P, xyz, nrm=None, times=None):
    pc = P.PointCloud(np.ascontiguousarray(xyz, np.float32))
    if nrm is not None:
        pc.normals = np.ascontiguousarray(nrm, np.float32)
    if times is not None:
        pc.times = np.ascontiguousarray(times, np.float32)
    return pc


def _estimation(P, kind, loss):
    R = P.registration
    kernel = {"l2": R.L2Loss(), "l1": R.L1Loss(), "gm": R.GMLoss(GM_K)}[loss]
    return R.TransformationEstimationPointToPlane(kernel) if kind == "plane" else R.TransformationEstimationPointToPoint(False, kernel)


def _assert_map_equals(dev, ref):
    """the comparison of tests/test_gpu_point_map.py"""
    assert len(dev) == len(ref)
    assert np.array_equal(dev.cells, ref.cells)
    assert np.array_equal(dev.starts, ref.starts) and np.array_equal(dev.counts, ref.counts)
    assert vr.bits_equal(dev.points, ref.points)
    assert dev.has_normals == (ref.normals is not None)
    if dev.has_normals:
        assert vr.bits_equal(dev.normals, ref.normals)


# ------------------------------------------------------------------------------------------ times
def test_times_setter_getter_and_carriers(P, clouds):
    src = clouds["source"]
    t = clouds["source_t"]
    assert src.has_times() and src.times.dtype == np.float32 and src.times.tobytes() == t.tobytes()
    bare = P.PointCloud(clouds["source_xyz"])
    assert not bare.has_times() and bare.times.shape == (0,)
    for bad in (t[:-1], np.zeros(len(t) + 1, np.float32), np.zeros((2, 2), np.float32)):
        with pytest.raises(ValueError, match="one value per point"):
            bare.times = bad
    assert not bare.has_times()
    c = copy.deepcopy(src)
    assert c.times.tobytes() == t.tobytes() and c._tim.data_ptr() != src._tim.data_ptr()
    idx = np.array([5, 0, 6000, 17, 17], np.int64)
    assert np.array_equal(src.select_by_index(idx).times, t[idx])
    keep = np.ones(len(t), bool); keep[idx] = False
    assert np.array_equal(src.select_by_index(idx, invert=True).times, t[keep])
    assert np.array_equal(src.uniform_down_sample(7).times, t[::7])
    r = src.random_down_sample(0.1, seed=3)
    rows = {p.tobytes(): i for i, p in enumerate(clouds["source_xyz"])}
    assert np.array_equal(r.times, t[[rows[p.tobytes()] for p in r._xyz.cpu().numpy()]])
    f = src.farthest_point_down_sample(50)
    assert np.array_equal(f.times, t[P.geometry.farthest_point_indices(src, 50)])
    moved = copy.deepcopy(src).transform(motion(10.0, [1.0, 2.0, 3.0]))
    assert moved.times.tobytes() == t.tobytes()
    filtered, kept = src.remove_radius_outlier(3, 0.6)
    assert np.array_equal(filtered.times, t[kept])
    # assigning the points clears the times, as it clears the other attributes
    c.points = clouds["source_xyz"]
    assert not c.has_times()


def test_voxel_down_sample_carries_the_mean_time(P, clouds):
    t = clouds["source_t"]
    timed = _cloud(P, clouds["source_xyz"], clouds["source_nrm"], t)
    coloured = _cloud(P, clouds["source_xyz"], clouds["source_nrm"])
    coloured.colors = np.stack([t, t, t], 1)
    a, b = timed.voxel_down_sample(0.7), coloured.voxel_down_sample(0.7)
    assert 100 < len(a) < len(timed) and a.has_times() and not a.has_colors()
    assert vr.bits_equal(a.times, b._col.cpu().numpy()[:, 0].copy())
    assert vr.bits_equal(a._xyz.cpu().numpy(), b._xyz.cpu().numpy()) and vr.bits_equal(a._nrm.cpu().numpy(), b._nrm.cpu().numpy())
    # with colours too, both are carried
    both = _cloud(P, clouds["source_xyz"], None, t)
    both.colors = np.stack([t, 1 - t, t * t], 1)
    d = both.voxel_down_sample(0.7)
    assert vr.bits_equal(d.times, a.times) and d.has_colors()


def test_a_cloud_without_times_gives_the_bytes_it_gave(P, clouds):
    """the same public calls on a cloud whose times were set and taken away again (by assigning the points) and on one that never had any"""
    never = _cloud(P, clouds["source_xyz"], clouds["source_nrm"])
    once = _cloud(P, clouds["source_xyz"], None, clouds["source_t"])
    once.points = clouds["source_xyz"]
    once.normals = clouds["source_nrm"]
    assert once._tim is None
    for call in (lambda pc: pc.voxel_down_sample(0.7), lambda pc: pc.uniform_down_sample(3), lambda pc: pc.select_by_index([4, 2, 9]), lambda pc: copy.deepcopy(pc),
                 lambda pc: pc.farthest_point_down_sample(20), lambda pc: copy.deepcopy(pc).transform(motion(5.0, [1, 0, 0]))):
        a, b = call(never), call(once)
        assert a._tim is None and b._tim is None and not a.has_times()
        assert a._xyz.cpu().numpy().tobytes() == b._xyz.cpu().numpy().tobytes() and a._nrm.cpu().numpy().tobytes() == b._nrm.cpu().numpy().tobytes()


# ------------------------------------------------------------------------------------------ deskew
def _motions():
    pure = np.eye(4); pure[:3, 3] = [0.4, -0.2, 0.1]
    tiny = np.eye(4); tiny[:3, :3] = ct.exp3(np.array([6e-6, -7e-6, 4e-6])); tiny[:3, 3] = [0.1, 0.0, 0.2]      # theta = 1.005e-5: the series branch
    assert 0.9e-5 < np.linalg.norm(ct.log3(tiny[:3, :3])) < 1.1e-5
    rad = np.eye(4); rad[:3, :3] = ct.exp3(np.array([0.6, -0.64, 0.48])); rad[:3, 3] = [1.0, 2.0, -0.5]          # theta = 1 rad
    return {"phi = 0": pure, "theta = 1e-5": tiny, "3 degrees": motion(3.0, [0.5, 0.0, 0.0]), "1 rad": rad}


@pytest.mark.parametrize("n", [1, 255, 256, 257, 7074])
def test_deskew_matches_reference(P, clouds, n):
    """The device's sin / cos are not numpy's, so a float64 value may differ in its last bits and a float32 output by one spacing, where the value
    falls on a rounding boundary: no coordinate differs by more than one spacing, and at most 1 in 1000 differs at all (expected: about 1e-8)"""
    xyz, nrm = clouds["target_xyz"][:n], clouds["target_nrm"][:n]
    t = ct.azimuth_alpha(xyz)
    pc = _cloud(P, xyz, nrm, t)
    pc.colors = np.abs(nrm)
    for name, D in _motions().items():
        for ref in (0.0, 0.5, 1.0):
            want_p, want_n = ct.deskew(xyz, nrm, t, D, ref, 0.0, 1.0)
            got = pc.deskew(D, ref, 0.0, 1.0)
            for what, a, b in (("points", got._xyz.cpu().numpy(), want_p), ("normals", got._nrm.cpu().numpy(), want_n)):
                differ = a != b
                steps = np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.abs(b)).astype(np.float64)
                assert steps.max() <= 1.0, (name, ref, what, float(steps.max()))
                assert differ.sum() <= differ.size / 1000.0, (name, ref, what, int(differ.sum()))
            assert got.times.tobytes() == t.tobytes() and vr.bits_equal(got.colors, pc.colors) and not got.has_covariances()
            assert np.array_equal(pc._xyz.cpu().numpy(), xyz)                      # the input is untouched
    if n > 1:                                                                   # the default span is the cloud's own minimum and maximum
        D = _motions()["3 degrees"]
        want_p, _ = ct.deskew(xyz, nrm, t, D, 1.0)
        a = pc.deskew(D)._xyz.cpu().numpy()
        assert (np.abs(a.astype(np.float64) - want_p) <= np.spacing(np.abs(want_p))).all() and (a != want_p).sum() <= a.size / 1000.0


def test_deskew_identity_covariances_and_refusals(P, clouds):
    pc = _cloud(P, clouds["target_xyz"], clouds["target_nrm"], ct.azimuth_alpha(clouds["target_xyz"]))
    pc.estimate_covariances(P.KDTreeSearchParamKNN(knn=10))
    assert pc.has_covariances()
    for ref in (0.0, 0.5, 1.0):
        same = pc.deskew(np.eye(4), ref)
        assert np.array_equal(same._xyz.cpu().numpy(), clouds["target_xyz"]) and np.array_equal(same._nrm.cpu().numpy(), clouds["target_nrm"])
        assert not same.has_covariances() and same.has_times()
    # the normals are rotated: by R(alpha_ref)^T R(alpha_i), which is the identity only where alpha_i == alpha_ref
    turned = pc.deskew(motion(30.0, [0, 0, 0]), 1.0, 0.0, 1.0)._nrm.cpu().numpy()
    assert np.abs(turned - clouds["target_nrm"]).max() > 0.1
    assert np.allclose(np.linalg.norm(turned, axis=1), np.linalg.norm(clouds["target_nrm"], axis=1), atol=1e-6)
    with pytest.raises(RuntimeError, match="no times"):
        P.PointCloud(clouds["target_xyz"]).deskew(np.eye(4))
    with pytest.raises(ValueError, match="t_end must be greater"):
        pc.deskew(np.eye(4), 1.0, 1.0, 1.0)
    with pytest.raises(ValueError, match="shape"):
        pc.deskew(np.eye(3))


# ------------------------------------------------------------------------------------------ one linearisation
def _compare_sums(got, ref, label):
    assert got.rows == ref["rows"]
    assert np.array_equal(got.matches.cpu().numpy(), ref["matches"])
    for name, a, b, mag in (("H", got.H, ref["H"], ref["mag_H"]), ("g", got.g, ref["g"], ref["mag_g"])):
        err = np.abs(a - b)
        print(f"{label} {name}: largest error / magnitude {float((err / np.maximum(mag, 1e-300)).max()):.1e}")
        assert (err <= 1e-9 * mag).all(), (label, name, float(err.max()))
    assert abs(got.sum_d2 - ref["sum_d2"]) <= 1e-9 * ref["sum_d2"] and abs(got.sum_r2 - ref["sum_r2"]) <= 1e-9 * ref["sum_r2"]
    assert np.array_equal(got.H, got.H.T)


@pytest.mark.parametrize("nbh", [7, 27])
@pytest.mark.parametrize("loss", ["l2", "l1", "gm"])
@pytest.mark.parametrize("kind", ["point", "plane"])
def test_linearize_continuous_matches_reference(P, clouds, dev_map, ref_map, pose_pair, kind, loss, nbh):
    """the bound of test_gpu_point_map.py::test_linearize_matches_reference: every entry within 1e-9 of the sum of the magnitudes of its terms"""
    T_b, T_e = pose_pair
    dist = 1.0 if nbh == 27 else 0.6
    ref = ct.linearize(ref_map, clouds["source_xyz"], clouds["source_t"], T_b, T_e, dist, nbh, KIND[kind], LOSS[loss], GM_K, 0.0, 1.0)
    got = dev_map.linearize_continuous(clouds["source"], T_b, T_e, dist, _estimation(P, kind, loss), nbh, 0.0, 1.0, True)
    assert got.rows > 3000
    _compare_sums(got, ref, f"{kind} {loss} nbh {nbh}")
    again = dev_map.linearize_continuous(clouds["source"], T_b, T_e, dist, _estimation(P, kind, loss), nbh, 0.0, 1.0, True)
    assert got.H.tobytes() == again.H.tobytes() and got.g.tobytes() == again.g.tobytes() and (got.rows, got.sum_d2, got.sum_r2) == (again.rows, again.sum_d2, again.sum_r2)
    assert np.array_equal(got.matches.cpu().numpy(), again.matches.cpu().numpy())
    assert dev_map.linearize_continuous(clouds["source"], T_b, T_e, dist, _estimation(P, kind, loss), nbh, 0.0, 1.0).matches is None


def test_linearize_continuous_default_span_and_extrapolation(P, clouds, dev_map, ref_map, pose_pair):
    """t_begin / t_end default to the cloud's minimum and maximum time; alpha is not clamped (a span inside the times extrapolates)"""
    T_b, T_e = pose_pair
    for span in ((None, None), (0.25, 0.75)):
        ref = ct.linearize(ref_map, clouds["source_xyz"], clouds["source_t"], T_b, T_e, 1.0, 27, pm.POINT_TO_PLANE, t0=span[0], t1=span[1])
        got = dev_map.linearize_continuous(clouds["source"], T_b, T_e, 1.0, _estimation(P, "plane", "l2"), 27, span[0], span[1], True)
        _compare_sums(got, ref, f"span {span}")


@pytest.mark.parametrize("n", [1, 511, 512, 513, 1025])
def test_tile_edges(P, clouds, dev_map, ref_map, pose_pair, n):
    T_b, T_e = pose_pair
    xyz, t = clouds["source_xyz"][3000:3000 + n], clouds["source_t"][3000:3000 + n]
    for kind in ("point", "plane"):
        ref = ct.linearize(ref_map, xyz, t, T_b, T_e, 1.0, 27, KIND[kind], t0=0.0, t1=1.0)
        got = dev_map.linearize_continuous(_cloud(P, xyz, None, t), T_b, T_e, 1.0, _estimation(P, kind, "l2"), 27, 0.0, 1.0, True)
        _compare_sums(got, ref, f"{kind} n {n}")


def test_source_outside_the_grid_has_no_rows(P, clouds, dev_map, pose_pair):
    T_b, T_e = pose_pair
    far = _cloud(P, clouds["source_xyz"][:700] + np.float32(1e4), None, clouds["source_t"][:700])
    for shift in (far, _cloud(P, clouds["source_xyz"][:700] - np.float32(3e7), None, clouds["source_t"][:700])):
        got = dev_map.linearize_continuous(shift, T_b, T_e, 1.0, None, 27, 0.0, 1.0, True)
        assert got.rows == 0 and got.sum_d2 == 0.0 and got.sum_r2 == 0.0 and not got.H.any() and not got.g.any() and (got.matches.cpu().numpy() == -1).all()
    res = P.registration.registration_point_map_continuous(far, dev_map, 1.0, T_b, T_e, t_begin=0.0, t_end=1.0)
    assert res.iterations == 0 and not res.converged and res.fitness == 0.0 and np.array_equal(res.end_pose, T_e) and len(res.correspondence_set) == 0


def test_small_maps_with_cells_of_one_and_of_m_rows(P):
    """maps of tens of points: cells with exactly 1 and exactly M rows, and more arrivals than M"""
    rng = np.random.default_rng(11)
    M = 4
    cell = np.concatenate([np.repeat(np.array([c], np.float64), k, 0) for c, k in (((3, 1, 2), M), ((0, 5, 1), M + 3), ((2, 2, 2), 1), ((7, 0, 0), 1), ((1, 1, 1), M - 1))])
    xyz = (cell + rng.uniform(-0.3, 0.3, cell.shape)).astype(np.float32)
    nrm = rng.normal(size=xyz.shape).astype(np.float32)
    ref = pm.build_map(xyz, nrm, 1.0, M, np.zeros(3))
    assert sorted(ref.counts.tolist()) == [1, 1, M - 1, M, M]
    src = (xyz + rng.normal(scale=0.1, size=xyz.shape)).astype(np.float32)
    t = rng.uniform(0.0, 1.0, len(src)).astype(np.float32)
    T_b, T_e = motion(1.0, [0.02, 0.0, 0.01]), motion(-2.0, [0.0, 0.05, 0.0])
    with P.registration.VoxelPointMap.on_grid(_cloud(P, xyz, nrm), 1.0, M, np.zeros(3)) as dev:
        for kind in ("point", "plane"):
            for nbh in (1, 7, 27):
                want = ct.linearize(ref, src, t, T_b, T_e, 0.8, nbh, KIND[kind], pm.GM, GM_K, 0.0, 1.0)
                got = dev.linearize_continuous(_cloud(P, src, None, t), T_b, T_e, 0.8, _estimation(P, kind, "gm"), nbh, 0.0, 1.0, True)
                assert want["rows"] > 5
                _compare_sums(got, want, f"small {kind} nbh {nbh}")


def test_estimated_map_validity(P, clouds, pose_pair):
    """on a map that estimates its normals a match to a row that is not valid is no row for point to plane, and is a row for point to point"""
    T_b, T_e = pose_pair
    with P.registration.VoxelPointMap(P.PointCloud(clouds["target_xyz"]), MAP_VOXEL, 20) as dev:
        dev.estimate_normals(1.0, 12)
        valid = dev.normal_valid
        ref = pm.build_map(clouds["target_xyz"], None, MAP_VOXEL, 20)
        assert vr.bits_equal(dev.points, ref.points)
        ref.normals = dev.normals
        point = ct.linearize(ref, clouds["source_xyz"], clouds["source_t"], T_b, T_e, 1.0, 27, pm.POINT_TO_POINT, t0=0.0, t1=1.0, valid=valid)
        plane = ct.linearize(ref, clouds["source_xyz"], clouds["source_t"], T_b, T_e, 1.0, 27, pm.POINT_TO_PLANE, t0=0.0, t1=1.0, valid=valid)
        dropped = (point["matches"] >= 0) & (plane["matches"] < 0)
        assert dropped.sum() > 50 and plane["rows"] > 1000 and not valid[point["matches"][dropped]].any() and plane["rows"] + dropped.sum() == point["rows"]
        _compare_sums(dev.linearize_continuous(clouds["source"], T_b, T_e, 1.0, _estimation(P, "point", "l2"), 27, 0.0, 1.0, True), point, "estimated point")
        _compare_sums(dev.linearize_continuous(clouds["source"], T_b, T_e, 1.0, _estimation(P, "plane", "l2"), 27, 0.0, 1.0, True), plane, "estimated plane")


# ------------------------------------------------------------------------------------------ the code that exists
@pytest.mark.parametrize("kind", ["point", "plane"])
def test_equal_poses_agree_with_the_rigid_calls(P, small_pair, clouds, dev_map, kind):
    T = np.array(small_pair["T_fgr"], np.float64)
    est = _estimation(P, kind, "l2")
    got = dev_map.linearize_continuous(clouds["source"], T, T, 1.0, est, 27, 0.0, 1.0, True)
    rows = dev_map.correspondences(clouds["source"], T, 1.0, 27).cpu().numpy()
    rigid = dev_map.linearize(clouds["source"], T, 1.0, est, 27)
    m = got.matches.cpu().numpy()
    i = np.nonzero(m >= 0)[0]
    assert got.rows == rigid.rows == len(rows) and np.array_equal(np.stack([i, m[i]], 1), rows)
    assert abs(got.sum_d2 - rigid.sum_d2) <= 1e-12 * rigid.sum_d2
    if kind == "plane":
        S = got.H[6:9, 6:9] + got.H[0:3, 6:9] + got.H[6:9, 0:3] + got.H[0:3, 0:3]          # the rotation block over u
        assert np.abs(S - S.T).max() <= 1e-12 * np.abs(S).max()
        assert np.linalg.eigvalsh((S + S.T) / 2.0).min() >= -1e-9 * np.abs(S).max()
        tr = got.H[9:12, 9:12] + got.H[3:6, 9:12] + got.H[9:12, 3:6] + got.H[3:6, 3:6]      # the translation block is the rigid one: sum w n n^T
        assert np.allclose(tr, rigid.JTJ[3:6, 3:6], rtol=1e-12, atol=0.0)


# ------------------------------------------------------------------------------------------ the loop
@pytest.fixture(scope="module")
def sweep(P, clouds):
    """the planted sweep of tests/test_continuous_time_api.py on the device's target cloud: the skewed scan, its times, the planted poses"""
    scan, times, T_b, T_e = planted_sweep(clouds["target_xyz"])
    return dict(scan=scan, times=times, T_b=T_b, T_e=T_e, cloud=_cloud(P, scan, None, times))


@pytest.fixture(scope="module")
def reference_loop(sweep, ref_map):
    @functools.lru_cache(maxsize=None)
    def run(kind, loss, begin="fixed", weight=None):
        return ct.loop(ref_map, sweep["scan"], sweep["times"], sweep["T_b"], sweep["T_b"], 1.0, 27, KIND[kind], LOSS[loss], GM_K, 5, begin=begin, prior_weight=weight, t0=0.0, t1=1.0)
    return run


@pytest.mark.parametrize("loss", ["l2", "gm"])
@pytest.mark.parametrize("kind", ["point", "plane"])
def test_trajectory_matches_reference(P, sweep, dev_map, reference_loop, kind, loss):
    """the bands of test_trajectory_matches_reference in tests/test_gpu_point_map.py, for both poses"""
    R = P.registration
    full = reference_loop(kind, loss)
    assert full.iterations > 2, full
    for max_it in (1, 2, 5):
        ref = full.after(max_it)
        res = R.registration_point_map_continuous(sweep["cloud"], dev_map, 1.0, sweep["T_b"], None, None, _estimation(P, kind, loss), R.ICPConvergenceCriteria(1e-6, 1e-6, max_it), 27,
                                                  t_begin=0.0, t_end=1.0)
        (ab, db), (ae, de) = pose_error(res.begin_pose, ref.begin_pose), pose_error(res.end_pose, ref.end_pose)
        print(f"{kind} {loss} max_it {max_it}: end {ae:.2e} rad {de:.2e} m, iterations {res.iterations} / {ref.iterations}, fitness {res.fitness - ref.fitness:+.1e} "
              f"rmse {res.inlier_rmse - ref.inlier_rmse:+.1e}")
        assert ae < 1e-7 and de < 1e-6 and ab < 1e-7 and db < 1e-6, (kind, loss, max_it, ae, de)
        assert res.iterations == ref.iterations and res.converged == ref.converged
        assert abs(res.fitness - ref.fitness) < 1e-12 and abs(res.inlier_rmse - ref.inlier_rmse) < 1e-9
        assert res.begin_pose.tobytes() == np.ascontiguousarray(sweep["T_b"], np.float64).tobytes()      # begin = "fixed": bit for bit
        assert res.transformation is res.end_pose
        i = np.nonzero(ref.matches >= 0)[0]
        assert np.array_equal(res.correspondence_set, np.stack([i, ref.matches[i]], 1))


def test_free_begin_with_and_without_a_prior(P, sweep, dev_map, reference_loop):
    R = P.registration
    for weight in (None, (10.0, 100.0)):
        ref = reference_loop("point", "l2", "free", weight)
        res = R.registration_point_map_continuous(sweep["cloud"], dev_map, 1.0, sweep["T_b"], None, None, None, R.ICPConvergenceCriteria(1e-6, 1e-6, 5), 27, begin="free",
                                                  begin_prior_weight=weight, t_begin=0.0, t_end=1.0)
        (ab, db), (ae, de) = pose_error(res.begin_pose, ref.begin_pose), pose_error(res.end_pose, ref.end_pose)
        print(f"free begin, prior {weight}: begin {ab:.2e} rad {db:.2e} m, end {ae:.2e} rad {de:.2e} m; begin moved {pose_error(res.begin_pose, sweep['T_b'])}")
        assert ae < 1e-7 and de < 1e-6 and ab < 1e-7 and db < 1e-6 and res.iterations == ref.iterations
    loose, held = reference_loop("point", "l2", "free", None), reference_loop("point", "l2", "free", (10.0, 100.0))
    assert pose_error(held.begin_pose, sweep["T_b"])[1] < pose_error(loose.begin_pose, sweep["T_b"])[1]


def test_planted_poses(P, clouds, sweep, dev_map):
    """the device ends within twice the distance from the planted end pose that the restatement's loop ends at (measured on the CPU, the constants of
    tests/test_continuous_time_api.py; the two is for the differing sin / cos and sum orders over the iterations), and with a smaller inlier RMSE
    than the rigid registration of the same skewed scan"""
    R = P.registration
    res = R.registration_point_map_continuous(sweep["cloud"], dev_map, 1.0, sweep["T_b"], t_begin=0.0, t_end=1.0)
    rigid = R.registration_point_map(sweep["cloud"], dev_map, 1.0, None, sweep["T_b"])
    ang, dt = pose_error(res.end_pose, sweep["T_e"])
    print(f"planted: {res.iterations} iterations, end pose {ang:.4e} rad {dt:.4e} m from the planted one, inlier_rmse {res.inlier_rmse:.6f} against the rigid {rigid.inlier_rmse:.6f}")
    assert res.converged and ang <= 2.0 * PLANTED_END_RAD and dt <= 2.0 * PLANTED_END_M
    assert res.inlier_rmse < rigid.inlier_rmse
    # a cloud target builds a temporary map of voxel_size: the same result
    other = R.registration_point_map_continuous(sweep["cloud"], clouds["target"], 1.0, sweep["T_b"], voxel_size=MAP_VOXEL, t_begin=0.0, t_end=1.0)
    assert other.end_pose.tobytes() == res.end_pose.tobytes()


# ------------------------------------------------------------------------------------------ the recipes
@pytest.fixture(scope="module")
def drive(P, clouds):
    truth, scans, times = skewed_drive(clouds["target_xyz"])
    return truth, [_cloud(P, s, None, t) for s, t in zip(scans, times)], scans, times


def test_odometry_with_deskewing_ends_closer_to_the_planted_poses(P, drive):
    R = P.registration
    truth, scans, _, _ = drive
    plain, _, m0 = R.scan_to_map_odometry_icp(scans, MAP_VOXEL, 1.0, max_points_per_voxel=10)
    m0.close()
    desk, results, m1 = R.scan_to_map_odometry_icp_deskew(scans, MAP_VOXEL, 1.0, max_points_per_voxel=10)
    with m1:
        assert len(desk) == len(results) == 4 and results[0] is None and np.array_equal(desk[1], plain[1])
        for k in (2, 3):
            (a0, d0), (a1, d1) = pose_error(plain[k], truth[k]), pose_error(desk[k], truth[k])
            print(f"scan {k}: without deskewing {a0:.3e} rad {d0:.3e} m, with {a1:.3e} rad {d1:.3e} m")
            assert a1 < a0 and d1 < d0
    # "static" takes every scan as it is
    still, _, m2 = R.scan_to_map_odometry_icp_deskew(scans, MAP_VOXEL, 1.0, max_points_per_voxel=10, motion_model="static")
    same, _, m3 = R.scan_to_map_odometry_icp(scans, MAP_VOXEL, 1.0, max_points_per_voxel=10, motion_model="static")
    m2.close(); m3.close()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(still, same))
    bare = [P.PointCloud(s._xyz) for s in scans]
    with pytest.raises(RuntimeError, match="no times"):
        R.scan_to_map_odometry_icp_deskew(bare, MAP_VOXEL, 1.0)


def test_continuous_time_odometry(P, drive):
    R = P.registration
    truth, scans, raw, times = drive
    crit = R.ICPConvergenceCriteria(1e-6, 1e-6, 10)
    begins, ends, results, m = R.scan_to_map_odometry_ct(scans, MAP_VOXEL, 1.0, criteria=crit, max_points_per_voxel=10)
    with m:
        assert len(begins) == len(ends) == len(results) == 4 and results[0] is None and np.array_equal(begins[0], np.eye(4)) and np.array_equal(ends[0], np.eye(4))
        for k in range(1, 4):
            assert begins[k].tobytes() == ends[k - 1].tobytes()
            a, d = pose_error(ends[k], truth[k])
            a0, d0 = pose_error(ends[k - 1], truth[k])
            print(f"scan {k}: end pose {a:.3e} rad {d:.3e} m from the planted one (the pose before: {a0:.3e} rad {d0:.3e} m), {results[k].iterations} iterations")
            assert a < a0 and d < d0
        # the returned map is the restatement's after the same deskewed inserts
        g = R.VoxelPointMap.centered_grid_min(scans[0].get_center(), MAP_VOXEL)
        assert np.array_equal(m.grid_min, g)
        ref = pm.build_map(raw[0], None, MAP_VOXEL, 10, g, np.eye(4))
        for k in range(1, 4):
            d = scans[k].deskew(np.linalg.inv(begins[k]) @ ends[k], reference=1.0)._xyz.cpu().numpy()
            want, _ = ct.deskew(raw[k], None, times[k], np.linalg.inv(begins[k]) @ ends[k], 1.0)
            assert (np.abs(d.astype(np.float64) - want) <= np.spacing(np.abs(want))).all()
            ref = pm.insert(ref, d, None, ends[k])
        _assert_map_equals(m, ref)
    # the calls by hand give the same poses bit for bit
    with R.VoxelPointMap.on_grid(scans[0], MAP_VOXEL, 10, g, np.eye(4)) as hand:
        b, e = [np.eye(4)], [np.eye(4)]
        for k in range(1, 4):
            T_b = e[-1]
            T_e = e[-1] @ np.linalg.inv(b[-1]) @ e[-1] if k > 1 else T_b
            res = R.registration_point_map_continuous(scans[k], hand, 1.0, T_b, T_e, None, None, crit, 27, 10, "fixed", None)
            b.append(res.begin_pose); e.append(res.end_pose)
            hand.insert(scans[k].deskew(np.linalg.inv(res.begin_pose) @ res.end_pose, reference=1.0), res.end_pose)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(b + e, begins + ends))
    with pytest.raises(RuntimeError, match="no times"):
        R.scan_to_map_odometry_ct([scans[0], P.PointCloud(scans[1]._xyz)], MAP_VOXEL, 1.0)


# ------------------------------------------------------------------------------------------ refusals
def _message(ctx):
    return (ctx.lib.pcr_last_error(ctx.handle) or b"").decode()


def test_abi_refusals_name_the_argument(P, clouds, dev_map):
    L = P._lib
    ctx = L.Context.current()
    lib, dp = ctx.lib, C.POINTER(C.c_double)
    torch = P.geometry._torch()
    src, ns, tim = clouds["source"].device_xyz().data_ptr(), len(clouds["source"]), clouds["source"].device_times().data_ptr()
    eye = np.eye(4)
    Tp = eye.ctypes.data_as(dp)
    m = dev_map._open()
    est = L.PcrEstimation(L.EST_POINT_TO_POINT, 0, 0, 1.0, 1e-3)

    def refused(rc, word):
        assert rc == L.PCR_EINVAL and word in _message(ctx), (rc, word, _message(ctx))

    def lin(mp=m, xyz=src, times=tim, n=ns, Tb=Tp, Te=Tp, t0=0.0, t1=1.0, d=1.0, nbh=27, e=est):
        return lib.pcr_point_map_linearize_continuous(ctx.handle, mp, xyz, times, n, Tb, Te, C.c_double(t0), C.c_double(t1), C.c_double(d), nbh,
                                                      C.byref(e) if e is not None else None, None, None, None, None, None, None)

    assert lin() == L.PCR_OK, _message(ctx)                                        # every output is optional
    refused(lin(times=None), "src_times is null")
    bad_t = torch.tensor(clouds["source_t"], device="cuda"); bad_t[17] = float("nan")
    refused(lin(times=bad_t.data_ptr()), "src_times holds a non-finite")
    for t0, t1 in ((1.0, 1.0), (2.0, 1.0)):
        refused(lin(t0=t0, t1=t1), "t1")
    refused(lin(t0=float("nan")), "t0")
    refused(lin(t1=float("inf")), "t1")
    nan_T = eye.copy(); nan_T[1, 2] = np.inf
    refused(lin(Tb=nan_T.ctypes.data_as(dp)), "T_begin16 holds")
    refused(lin(Te=nan_T.ctypes.data_as(dp)), "T_end16 holds")
    refused(lin(Te=None), "T_end16 is null")
    row_T = eye.copy(); row_T[3, 0] = 0.5
    refused(lin(Tb=row_T.ctypes.data_as(dp)), "T_begin16")
    refused(lin(Te=row_T.ctypes.data_as(dp)), "T_end16 is no pose")
    # the refusals of pcr_point_map_linearize
    for nbh in (0, 5, 26):
        refused(lin(nbh=nbh), "neighborhood")
    for d in (0.0, -1.0, float("nan"), float("inf")):
        refused(lin(d=d), "max_correspondence_distance")
    refused(lin(mp=None), "map is null")
    refused(lin(xyz=None), "src_xyz")
    nan_xyz = torch.tensor(clouds["source_xyz"], device="cuda"); nan_xyz[3, 1] = float("nan")
    refused(lin(xyz=nan_xyz.data_ptr()), "src_xyz holds")
    refused(lin(e=None), "estimation is null")
    refused(lin(e=L.PcrEstimation(L.EST_GENERALIZED_ICP, 0, 0, 1.0, 1e-3)), "estimation.kind")
    refused(lin(e=L.PcrEstimation(L.EST_POINT_TO_POINT, 1, 0, 1.0, 1e-3)), "with_scaling")
    refused(lin(e=L.PcrEstimation(L.EST_POINT_TO_PLANE, 0, 7, 1.0, 1e-3)), "estimation.loss")
    with P.registration.VoxelPointMap(P.PointCloud(clouds["target_xyz"]), MAP_VOXEL, 20) as bare:
        refused(lin(mp=bare._open(), e=L.PcrEstimation(L.EST_POINT_TO_PLANE, 0, 0, 1.0, 1e-3)), "normals")

    out = torch.empty((ns, 3), dtype=torch.float32, device="cuda")

    def desk(xyz=src, nrm=None, times=tim, n=ns, D=Tp, t0=0.0, t1=1.0, ref=1.0, o=out.data_ptr(), on=None):
        return lib.pcr_deskew(ctx.handle, xyz, nrm, times, n, D, C.c_double(t0), C.c_double(t1), C.c_double(ref), o, on)

    assert desk() == L.PCR_OK, _message(ctx)
    refused(desk(times=None), "times is null")
    refused(desk(times=bad_t.data_ptr()), "times holds a non-finite")
    refused(desk(xyz=nan_xyz.data_ptr()), "xyz holds a non-finite")
    refused(desk(t0=1.0, t1=1.0), "t1")
    refused(desk(t0=1.0, t1=0.5), "t1")
    refused(desk(ref=float("nan")), "alpha_ref")
    refused(desk(D=None), "motion16 is null")
    refused(desk(D=nan_T.ctypes.data_as(dp)), "motion16 holds")
    refused(desk(D=row_T.ctypes.data_as(dp)), "motion16 is no pose")
    refused(desk(o=None), "out_xyz")
    refused(desk(nrm=clouds["source"].device_normals().data_ptr()), "out_normals")
    refused(desk(on=out.data_ptr()), "out_normals")
