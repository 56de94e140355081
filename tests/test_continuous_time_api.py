"""CPU-side checks of the continuous-time rule (include/pcr_hip.h, "continuous time"): the numpy restatement (tests/continuous_time_reference.py)
against itself -- its Jacobian against finite differences where the rule claims exactness, its loop and its deskewing on a planted sweep, the
condition the odometry comparison of tests/test_gpu_continuous_time.py rests on --, the ABI, the Python surface and the PCD time field.  Needs no GPU."""
import inspect
import os
import re

import numpy as np
import pytest

import continuous_time_reference as ct
import point_map_reference as pm
import voxel_reference as vr
from conftest import ROOT, pkg, pose_error

ENTRY_POINTS = ["pcr_deskew", "pcr_point_map_linearize_continuous"]

# The restatement's loop on the planted sweep of test_planted_poses_restatement_loop (pair 899's target at voxel 0.3 as the world, a 1.0 m map with
# M = 20, point to point, L2, neighbourhood 27, distance 1.0, the begin pose fixed, the end pose started at the begin pose), measured with numpy on
# the CPU by that test: the distance of the returned end pose from the planted one, and the final inlier RMSE of it and of the rigid pm.loop on the
# same skewed scan.  The rest is the first-order rotation columns and the map's own sampling; the GPU test holds the device to twice the distances.
PLANTED_END_RAD, PLANTED_END_M = 1.4234e-05, 1.4060e-03
PLANTED_CT_RMSE, PLANTED_RIGID_RMSE = 0.021283, 0.208088


def motion(deg, t):
    a = np.deg2rad(deg)
    T = np.eye(4)
    T[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
    T[:3, 3] = t
    return T


def planted_sweep(world):
    """(scan, times, T_b, T_e): the world seen by a sensor that moves by 0.5 m and 3 degrees over the sweep, alpha = the azimuth in the begin frame"""
    T_b, T_e = np.eye(4), motion(3.0, [0.5, 0.0, 0.0])
    alpha = ct.azimuth_alpha(world)
    return ct.skew(world, alpha.astype(np.float64), T_b, T_e), alpha, T_b, T_e


def skewed_drive(world):
    """(truth, scans, times): the drive of tests/test_gpu_point_map.py -- four poses that advance by 0.2 m and 1 degree -- with every scan skewed by
    its own step: scan 0 is taken at rest, scan k while the sensor moves from truth[k - 1] to truth[k]; alpha = the azimuth in the end frame"""
    step = motion(1.0, [0.2, 0.0, 0.0])
    truth, scans, times = [np.eye(4)], [], []
    for k in range(4):
        if k:
            truth.append(truth[-1] @ step)
        inv = np.linalg.inv(truth[k])
        a = ct.azimuth_alpha(np.asarray(world, np.float64) @ inv[:3, :3].T + inv[:3, 3])
        scans.append(ct.skew(world, a.astype(np.float64), truth[k - 1] if k else truth[0], truth[k]))
        times.append(a)
    return truth, scans, times


@pytest.fixture(scope="module")
def world(small_pair):
    W = vr.voxel_reference(small_pair["target"], 0.3).points.astype(np.float32)
    assert len(W) == 7074
    return W


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
    sec = hdr[hdr.index("= continuous time"):hdr.index("int pcr_point_map_linearize_continuous(")]
    for word in ("TIMES.", "POSE AT alpha.", "DESKEW(cloud, D, alpha_ref).", "ROW.", "UPDATE.", "LIMITATION.", "SUMS.", "STEP", "LOOP.", "NOBODY HAS COMPARED",
                 "COVARIANCES ARE NOT", "NOT clamped"):
        assert word in sec, word
    csrc = os.path.join(ROOT, "point-cloud-registration-with-global-refinement_amd", "csrc")
    assert os.path.exists(os.path.join(csrc, "pcr_ctime.hip"))
    assert re.search(r"^for f in .*\bpcr_ctime\b", open(os.path.join(csrc, "build.sh")).read(), re.M)
    assert '"pcr_ctime"' in open(os.path.join(ROOT, "tools", "pk_trans_scan.py")).read()
    # the search helpers live once, in the header both units include
    for unit in ("pcr_pmap.hip", "pcr_ctime.hip"):
        text = open(os.path.join(csrc, unit)).read()
        assert "void pm_search(" not in text and "void pm_match_own(" not in text and "double pm_weight(" not in text and '#include "pcr_pmap.h"' in text
    assert open(os.path.join(csrc, "pcr_pmap.h")).read().count("void pm_search(") == 1
    assert "pcr_ctime.hip" in open(os.path.join(ROOT, "README.md")).read()
    assert "4.29" in open(os.path.join(ROOT, "DESIGN.md")).read()


def test_python_surface_and_defaults():
    P = pkg()
    R, G = P.registration, P.geometry
    assert isinstance(vars(G.PointCloud)["times"], property) and callable(G.PointCloud.has_times)
    sig = inspect.signature(G.PointCloud.deskew).parameters
    assert list(sig) == ["self", "motion", "reference", "t_begin", "t_end"] and sig["reference"].default == 1.0
    sig = inspect.signature(R.VoxelPointMap.linearize_continuous).parameters
    assert list(sig) == ["self", "source", "T_begin", "T_end", "max_correspondence_distance", "estimation_method", "neighborhood", "t_begin", "t_end", "return_matches"]
    assert sig["neighborhood"].default == 27 and sig["return_matches"].default is False
    sig = inspect.signature(R.registration_point_map_continuous).parameters
    assert list(sig) == ["source", "target_or_map", "max_correspondence_distance", "T_begin", "T_end", "voxel_size", "estimation_method", "criteria", "neighborhood",
                         "max_points_per_voxel", "begin", "begin_prior_weight", "t_begin", "t_end"]
    assert sig["begin"].default == "fixed" and sig["T_end"].default is None and sig["neighborhood"].default == 27 and sig["max_points_per_voxel"].default == 20
    sig = inspect.signature(R.scan_to_map_odometry_ct).parameters
    assert list(sig) == ["scans", "voxel_size", "max_correspondence_distance", "init", "estimation_method", "criteria", "neighborhood", "max_points_per_voxel", "max_range",
                         "grid_min", "begin", "begin_prior_weight"]
    # the deskewing recipe is a function of its own: the two recipes it extends keep their signatures
    old = inspect.signature(R.scan_to_map_odometry_icp_map_normals).parameters
    sig = inspect.signature(R.scan_to_map_odometry_icp_deskew).parameters
    assert list(sig) == list(inspect.signature(R.scan_to_map_odometry_icp).parameters) + ["map_normals", "map_normal_radius", "map_normal_min_neighbors"]
    assert sig["map_normals"].default is False and sig["map_normal_min_neighbors"].default == old["map_normal_min_neighbors"].default
    for fn in (R.scan_to_map_odometry_ct, R.scan_to_map_odometry_icp_deskew, R.registration_point_map_continuous, G.PointCloud.deskew):
        assert "deskew" in fn.__doc__ or "continuous" in fn.__doc__.lower()
    assert "map.insert(scans[k].deskew(inv(begin_poses[k]) @ end_poses[k], reference=1.0), end_poses[k])" in R.scan_to_map_odometry_ct.__doc__
    for bad in ({"begin": "loose"}, {"begin_prior_weight": (1.0, 1.0)}, {"begin": "free", "begin_prior_weight": (1.0,)}, {"begin": "free", "begin_prior_weight": (-1.0, 0.0)}):
        with pytest.raises(ValueError, match="begin"):
            R.registration_point_map_continuous(None, None, 1.0, np.eye(4), **bad)


def test_pcd_times_round_trip(tmp_path):
    io = pkg("io")
    rng = np.random.default_rng(7)
    xyz = rng.normal(size=(17, 3)).astype(np.float32)
    t = rng.uniform(0.0, 0.1, 17).astype(np.float32)
    path = str(tmp_path / "sweep.pcd")
    io.write_pcd_xyzt(path, xyz, t)
    assert np.array_equal(io.read_pcd_xyz(path), xyz) and io.read_pcd_times(path).tobytes() == t.tobytes()
    assert io.read_pcd_times(path, "time").tobytes() == t.tobytes() and io.read_pcd_times(path, "timestamp") is None
    assert io.read_pcd(path)[1] is None                                # the existing readers see a file without colours
    plain = str(tmp_path / "plain.pcd")
    io.write_pcd_xyz(plain, xyz)
    assert io.read_pcd_times(plain) is None
    with pytest.raises(ValueError, match="one time per point"):
        io.write_pcd_xyzt(path, xyz, t[:5])


# ------------------------------------------------------------------------------------------ the restatement against itself
def test_exp_and_log():
    assert np.array_equal(ct.exp3(np.zeros(3)), np.eye(3))
    rng = np.random.default_rng(1)
    for theta in (1e-9, 1e-5, 0.9e-4, 1.1e-4, 0.05, 1.0, 3.0, np.pi - 1e-3, np.pi - 1e-9):
        v = rng.normal(size=3)
        v *= theta / np.linalg.norm(v)
        E = ct.exp3(v)
        assert np.abs(E @ E.T - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(E) - 1.0) < 1e-14
        back = ct.log3(E)
        assert np.linalg.norm(back - v) < 1e-7 * max(theta, 1e-9) or np.linalg.norm(back - v) < 2e-8, (theta, back, v)
    # both series meet at the threshold: the truncation is below 1e-18
    v = np.array([1e-4, 0.0, 0.0])
    assert np.abs(ct.exp3(v * (1 - 1e-12)) - ct.exp3(v)).max() < 1e-15


@pytest.mark.parametrize("kind", ["point", "plane"])
def test_jacobian_equals_finite_differences_where_the_rotations_agree(kind):
    """phi = 0 (R_b == R_e) and t_b != t_e is where the rule claims exactness: the restatement's 12-column rows against central differences of its
    own residuals under the STEP's own update, to 1e-6 of the largest entry"""
    rng = np.random.default_rng(5)
    pts = rng.uniform(0.0, 6.0, (80, 3)).astype(np.float32)
    nrm = rng.normal(size=(80, 3)); nrm = (nrm / np.linalg.norm(nrm, axis=1)[:, None]).astype(np.float32)
    m = pm.build_map(pts, nrm, 1.0, 20)
    T_b = motion(20.0, [0.3, -0.2, 0.1]); T_e = T_b.copy(); T_e[:3, 3] += [0.4, 0.1, -0.05]
    times = rng.uniform(0.0, 1.0, 80).astype(np.float32)
    alpha = times.astype(np.float64)
    world = pts.astype(np.float64) + rng.normal(scale=0.02, size=(80, 3))
    src = ct.skew(world, alpha, T_b, T_e)
    K = pm.POINT_TO_PLANE if kind == "plane" else pm.POINT_TO_POINT
    base = ct.linearize(m, src, times, T_b, T_e, 1.0, 27, K, t0=0.0, t1=1.0)
    assert base["rows"] == 80
    J = base["J12"].reshape(-1, 12)

    def residuals(x):
        b, e, ok = ct.step(np.eye(12), -x, 1, T_b, T_e, "free")
        assert ok
        s = ct.linearize(m, src, times, b, e, 1.0, 27, K, t0=0.0, t1=1.0)
        assert np.array_equal(s["matches"], base["matches"])
        return s["residuals"].reshape(-1)

    h = 1e-5
    fd = np.stack([(residuals(h * np.eye(12)[c]) - residuals(-h * np.eye(12)[c])) / (2.0 * h) for c in range(12)], 1)
    err = np.abs(fd - J).max() / np.abs(J).max()
    print(f"{kind}: largest |finite difference - J12| / largest |J12| = {err:.2e}")
    assert err <= 1e-6
    # H and g are the sums of these rows
    w = base["weights"].reshape(-1)
    assert np.allclose(base["H"], (w[:, None, None] * J[:, :, None] * J[:, None, :]).sum(0), rtol=1e-12, atol=1e-12)
    assert np.allclose(base["g"], (w[:, None] * J * base["residuals"].reshape(-1)[:, None]).sum(0), rtol=1e-12, atol=1e-12)


def test_equal_poses_give_the_rigid_sums(world):
    """T_begin == T_end: the placed points are the rigid ones bit for bit, the rows those of the rigid rule"""
    T = motion(2.0, [0.1, 0.05, 0.0])
    m = pm.build_map(world, None, 1.0, 20)
    src = world[::7]
    times = ct.azimuth_alpha(src)
    q, u, a = ct.place(src, times, T, T, 0.0, 1.0)
    assert np.array_equal(q, pm.transform(src, T))
    s = ct.linearize(m, src, times, T, T, 1.0, 27, t0=0.0, t1=1.0)
    r = pm.linearize(m, src, T, 1.0, 27)
    assert s["rows"] == r["rows"] and np.array_equal(s["matches"][s["matches"] >= 0], r["pairs"][:, 1]) and s["sum_d2"] == r["sum_d2"]
    # the translation block of the four 6x6 blocks together is the rigid one
    tr = s["H"][3:6, 3:6] + s["H"][3:6, 9:12] + s["H"][9:12, 3:6] + s["H"][9:12, 9:12]
    assert np.allclose(tr, r["JTJ"][3:6, 3:6], rtol=1e-12)


def test_planted_poses_restatement_loop(world):
    scan, times, T_b, T_e = planted_sweep(world)
    m = pm.build_map(world, None, 1.0, 20)
    res = ct.loop(m, scan, times, T_b, T_b, 1.0, 27, t0=0.0, t1=1.0)
    rigid = pm.loop(m, scan, T_b, 1.0, 27)
    ang, dt = pose_error(res.end_pose, T_e)
    a0, d0 = pose_error(T_b, T_e)
    print(f"continuous time: {res.iterations} iterations, end pose {ang:.4e} rad {dt:.4e} m from the planted one (start {a0:.3e} rad {d0:.3e} m), inlier_rmse {res.inlier_rmse:.6f}; "
          f"rigid: {rigid.iterations} iterations, inlier_rmse {rigid.inlier_rmse:.6f}, {pose_error(rigid.transformation, T_e)}")
    assert np.array_equal(res.begin_pose, T_b)
    assert res.inlier_rmse < rigid.inlier_rmse
    assert ang < a0 and dt < d0
    # the recorded figures are these (numpy's last bits may differ between versions: 1 %)
    assert abs(ang - PLANTED_END_RAD) <= 0.01 * PLANTED_END_RAD and abs(dt - PLANTED_END_M) <= 0.01 * PLANTED_END_M
    assert abs(res.inlier_rmse - PLANTED_CT_RMSE) <= 0.01 * PLANTED_CT_RMSE and abs(rigid.inlier_rmse - PLANTED_RIGID_RMSE) <= 0.01 * PLANTED_RIGID_RMSE


def test_deskew_round_trip(world):
    """deskewing the skewed scan with the planted motion gives inv(T_e) W back.  The skewed scan was rounded to float32 at ITS coordinates, so the
    spacing that bounds the error of a coordinate is that of the point's largest coordinate, before or after, not the coordinate's own"""
    scan, times, T_b, T_e = planted_sweep(world)
    back, none = ct.deskew(scan, None, times, np.linalg.inv(T_b) @ T_e, 1.0, 0.0, 1.0)
    assert none is None and back.dtype == np.float32
    inv = np.linalg.inv(T_e)
    want = world.astype(np.float64) @ inv[:3, :3].T + inv[:3, 3]
    spacing = np.spacing(np.maximum(np.abs(scan).max(1), np.abs(back).max(1)).astype(np.float32)).astype(np.float64)
    err = np.abs(back.astype(np.float64) - want) / spacing[:, None]
    print(f"deskew round trip: largest error {err.max():.3f} spacings")
    assert err.max() <= 1.0
    # the identity motion returns the input values, whatever the reference
    for ref in (0.0, 0.5, 1.0):
        same, _ = ct.deskew(scan, None, times, np.eye(4), ref, 0.0, 1.0)
        assert np.array_equal(same, scan)
    # alpha_ref = 0 is the begin frame
    first, _ = ct.deskew(scan, None, times, np.linalg.inv(T_b) @ T_e, 0.0, 0.0, 1.0)
    assert np.abs(first.astype(np.float64) - world.astype(np.float64)).max() < 1e-5


def test_odometry_condition_deskewing_ends_closer(world):
    """what the odometry comparison on the device rests on: on the skewed drive the restatement's recipe with deskewing ends closer to the planted
    end poses than without, at scans 2 and 3 (scans 0 and 1 are taken as they are by both)"""
    truth, scans, times = skewed_drive(world)
    g = np.floor(scans[0].astype(np.float64).mean(0)) - float(1 << 20)
    plain, _ = ct.odometry_icp(scans, times, 1.0, 1.0, False, g, M=10)
    desk, _ = ct.odometry_icp(scans, times, 1.0, 1.0, True, g, M=10)
    assert np.array_equal(plain[1], desk[1])
    for k in (2, 3):
        (a0, d0), (a1, d1) = pose_error(plain[k], truth[k]), pose_error(desk[k], truth[k])
        print(f"scan {k}: without deskewing {a0:.3e} rad {d0:.3e} m, with {a1:.3e} rad {d1:.3e} m")
        assert a1 < a0 and d1 < d0
