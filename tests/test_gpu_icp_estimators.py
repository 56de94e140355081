"""registration_icp with TransformationEstimationPointToPlane / PointToPoint on the device against a float64 restatement of Open3D's
RegistrationICP (oracle correspondences, numpy linearisation / Umeyama, incremental transform of the cloud)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, pkg, pose_error

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    return pkg()


@pytest.fixture(scope="module")
def scale_clouds(P, small_pair):
    """Pair 899 at voxel 0.3, SOR(30, 1), KNN-20 normals: the clouds of tests/test_gpu_gicp.py's loop tests."""
    out = []
    for key in ("source", "target"):
        pc = P.PointCloud(small_pair[key]).voxel_down_sample(0.3)
        pc, _ = pc.remove_statistical_outlier(30, 1.0)
        pc.estimate_normals(P.KDTreeSearchParamKNN(knn=20))
        out.append(pc)
    return out


def _umeyama(src, dst, with_scaling):
    n = src.shape[0]
    ms, md = src.mean(0), dst.mean(0)
    sd, dd = src - ms, dst - md
    sigma = dd.T @ sd / n
    U, D, Vt = np.linalg.svd(sigma)
    S = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2] = -1
    R = U @ np.diag(S) @ Vt
    c = (D @ S) / ((sd ** 2).sum() / n) if with_scaling else 1.0
    T = np.eye(4)
    T[:3, :3] = c * R
    T[:3, 3] = md - c * R @ ms
    return T


def _weights(loss, k, r):
    if loss == "l1":
        return 1.0 / np.abs(r)
    if loss == "gm":
        return k / (k + r * r) ** 2
    return np.ones_like(r)


def reference_icp(oracle, src, tgt, tgt_normals, max_dist, T0, estimation, loss="l2", k=1.0, max_it=30, rel=1e-6):
    """Open3D RegistrationICP in float64: search at init, then update / left-multiply / transform the cloud / search again."""
    tgt = np.asarray(tgt, np.float64)
    n = np.asarray(tgt_normals, np.float64) if tgt_normals is not None else None
    T = np.array(T0, np.float64)
    P = np.asarray(src, np.float64) @ T[:3, :3].T + T[:3, 3]
    corr, fit, rmse = oracle.find_correspondences(P, tgt, max_dist)
    it, converged = 0, False
    while it < max_it:
        U = np.eye(4)
        if len(corr):
            q, t = P[corr[:, 0]], tgt[corr[:, 1]]
            if estimation == "p2pl":
                nn = n[corr[:, 1]]
                r = ((q - t) * nn).sum(1)
                J = np.concatenate([np.cross(q, nn), nn], axis=1)
                w = _weights(loss, k, r)
                U, _ = oracle.solve_update((J * w[:, None]).T @ J, (J * (w * r)[:, None]).sum(0))
            else:
                U = _umeyama(q, t, estimation == "p2ps")
        T = U @ T
        P = P @ U[:3, :3].T + U[:3, 3]
        before = (fit, rmse)
        corr, fit, rmse = oracle.find_correspondences(P, tgt, max_dist)
        it += 1
        if abs(before[0] - fit) < rel and abs(before[1] - rmse) < rel:
            converged = True
            break
    return T, fit, rmse, it, converged, len(corr)


def _est(P, estimation, loss="l2", k=1.0):
    R = P.registration
    if estimation == "p2pl":
        return R.TransformationEstimationPointToPlane({"l2": R.L2Loss(), "l1": R.L1Loss(), "gm": R.GMLoss(k)}[loss])
    return R.TransformationEstimationPointToPoint(estimation == "p2ps")


@pytest.mark.parametrize("estimation", ["p2pl", "p2p", "p2ps"])
def test_trajectory_matches_reference(P, oracle, small_pair, scale_clouds, estimation):
    src, tgt = scale_clouds
    T0 = small_pair["T_fgr"]
    for max_it in (1, 5, 40):
        crit = P.registration.ICPConvergenceCriteria(1e-6, 1e-6, max_it)
        res = P.registration.registration_icp(src, tgt, 0.6, T0, _est(P, estimation), crit)
        T, fit, rmse, it, conv, nc = reference_icp(oracle, src.points, tgt.points, tgt.normals, 0.6, T0, estimation, max_it=max_it)
        ang, dt = pose_error(res.transformation, T)
        assert ang < 1e-7 and dt < 1e-6, (max_it, ang, dt)
        if estimation == "p2ps":
            assert abs(np.cbrt(np.linalg.det(res.transformation[:3, :3])) - np.cbrt(np.linalg.det(T[:3, :3]))) < 1e-7
        assert res.iterations == it and res.converged == conv, (max_it, res.iterations, it, res.converged, conv)
        assert abs(res.fitness - fit) < 1e-12 and abs(res.inlier_rmse - rmse) < 1e-9
        assert len(res.correspondence_set) == nc
        cs = res.correspondence_set
        assert cs.shape == (nc, 2) and len(np.unique(cs[:, 0])) == nc and cs[:, 0].max() < len(src) and cs[:, 1].max() < len(tgt)


@pytest.mark.parametrize("loss", ["l1", "gm"])
def test_point_to_plane_robust_kernels(P, oracle, small_pair, scale_clouds, loss):
    src, tgt = scale_clouds
    T0 = small_pair["T_fgr"]
    crit = P.registration.ICPConvergenceCriteria(1e-6, 1e-6, 3)
    res = P.registration.registration_icp(src, tgt, 0.6, T0, _est(P, "p2pl", loss, 0.5), crit)
    T, *_ = reference_icp(oracle, src.points, tgt.points, tgt.normals, 0.6, T0, "p2pl", loss=loss, k=0.5, max_it=3)
    ang, dt = pose_error(res.transformation, T)
    assert ang < 1e-6 and dt < 1e-5, (loss, ang, dt)
    assert not np.allclose(res.transformation, P.registration.registration_icp(src, tgt, 0.6, T0, _est(P, "p2pl"), crit).transformation, rtol=0, atol=1e-9)


def test_point_to_plane_takes_target_normals_unnormalised(P, oracle, small_pair, scale_clouds):
    """GICP normalises its normals, point-to-plane does not: normals of length 2 double every residual and Jacobian row (the
    update of L2 is the same), while GM weights them by the unscaled kernel: another pose, the one of the reference."""
    src, tgt = scale_clouds
    T0 = small_pair["T_fgr"]
    long = P.PointCloud(tgt.points)
    long.normals = 2.0 * np.asarray(tgt.normals)
    crit = P.registration.ICPConvergenceCriteria(1e-6, 1e-6, 3)
    res = P.registration.registration_icp(src, long, 0.6, T0, _est(P, "p2pl", "gm", 0.5), crit)
    T, *_ = reference_icp(oracle, src.points, tgt.points, long.normals, 0.6, T0, "p2pl", loss="gm", k=0.5, max_it=3)
    ang, dt = pose_error(res.transformation, T)
    assert ang < 1e-6 and dt < 1e-5, (ang, dt)


def test_point_to_point_recovers_a_similarity(P, scale_clouds):
    src = np.asarray(scale_clouds[0].points, np.float64)
    a = np.deg2rad(3.0)
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]) @ np.array(
        [[1, 0, 0], [0, np.cos(a / 2), -np.sin(a / 2)], [0, np.sin(a / 2), np.cos(a / 2)]])
    s, t = 1.05, np.array([0.03, -0.02, 0.01])
    tgt = (s * src @ R.T + t).astype(np.float32)
    T_true = np.eye(4)
    T_true[:3, :3] = s * R
    T_true[:3, 3] = t
    b = np.deg2rad(0.05)
    dR = np.array([[np.cos(b), -np.sin(b), 0], [np.sin(b), np.cos(b), 0], [0, 0, 1]])
    init = T_true.copy()
    init[:3, :3] = s * 1.0005 * dR @ R
    init[:3, 3] += [0.02, 0.01, -0.01]
    crit = P.registration.ICPConvergenceCriteria(1e-6, 1e-6, 50)
    res = P.registration.registration_icp(P.PointCloud(src.astype(np.float32)), P.PointCloud(tgt), 0.6, init,
                                          P.registration.TransformationEstimationPointToPoint(True), crit)
    Tr = res.transformation
    sr = np.cbrt(np.linalg.det(Tr[:3, :3]))
    assert abs(sr - s) < 1e-6, sr
    assert np.abs(Tr[:3, :3] / sr - R).max() < 1e-6 and np.abs(Tr[:3, 3] - t).max() < 1e-6, Tr
    assert res.fitness == 1.0 and res.converged
    assert np.array_equal(Tr[3], [0, 0, 0, 1])
    # without scaling every update is rigid: the pose keeps the scale of the start
    rig = P.registration.registration_icp(P.PointCloud(src.astype(np.float32)), P.PointCloud(tgt), 0.6, init,
                                          P.registration.TransformationEstimationPointToPoint(False), crit)
    assert abs(np.linalg.det(rig.transformation[:3, :3]) / np.linalg.det(init[:3, :3]) - 1.0) < 1e-9


@pytest.mark.parametrize("estimation", ["p2pl", "p2p", "p2ps"])
def test_errors_and_degenerate(P, scale_clouds, estimation):
    src, tgt = scale_clouds
    icp = P.registration.registration_icp
    with pytest.raises(RuntimeError):
        icp(src, tgt, 0.0, np.eye(4), _est(P, estimation))
    far = P.PointCloud(tgt.points + 1000.0)
    far.normals = tgt.normals
    res = icp(src, far, 0.5, np.eye(4), _est(P, estimation))
    assert res.fitness == 0 and res.inlier_rmse == 0 and np.array_equal(res.transformation, np.eye(4))
    assert res.converged and res.iterations == 1 and len(res.correspondence_set) == 0
    empty = P.PointCloud(np.zeros((0, 3)))
    res = icp(empty, tgt, 0.5, np.eye(4), _est(P, estimation))
    assert res.fitness == 0 and np.array_equal(res.transformation, np.eye(4))
    assert res.converged and res.iterations == 1


def test_point_to_plane_needs_target_normals(P, scale_clouds):
    src, tgt = scale_clouds
    bare = P.PointCloud(tgt.points)
    with pytest.raises(RuntimeError, match="normal"):
        P.registration.registration_icp(src, bare, 0.6, np.eye(4), P.registration.TransformationEstimationPointToPlane())
    # point-to-point needs none, on either cloud
    res = P.registration.registration_icp(P.PointCloud(src.points), bare, 0.6, np.eye(4))
    assert res.iterations >= 1


def test_default_estimator_and_gicp_dispatch(P, small_pair, scale_clouds):
    src, tgt = scale_clouds
    T0 = small_pair["T_fgr"]
    R = P.registration
    a = R.registration_icp(src, tgt, 0.6, T0)
    b = R.registration_icp(src, tgt, 0.6, T0, R.TransformationEstimationPointToPoint(False), R.ICPConvergenceCriteria())
    assert a.transformation.tobytes() == b.transformation.tobytes() and a.iterations == b.iterations and a.fitness == b.fitness
    assert np.array_equal(a.correspondence_set, b.correspondence_set)
    est = R.TransformationEstimationForGeneralizedICP(R.L2Loss())
    crit = R.ICPConvergenceCriteria(1e-6, 1e-6, 10)
    g1 = R.registration_icp(src, tgt, 0.6, T0, est, crit)
    g2 = R.registration_generalized_icp(src, tgt, 0.6, T0, est, crit)
    assert g1.transformation.tobytes() == g2.transformation.tobytes() and g1.iterations == g2.iterations
    assert g1.fitness == g2.fitness and g1.inlier_rmse == g2.inlier_rmse


def test_estimators_do_not_share_captured_graphs(P, small_pair, scale_clouds):
    """Point-to-point and point-to-plane problems on the same clouds with the same parameters have byte-identical loop arguments; the
    captured chunk of launches must still be the estimator's own (the estimator is part of the graph cache key)."""
    src, tgt = scale_clouds
    T0 = small_pair["T_fgr"]
    R = P.registration
    crit = R.ICPConvergenceCriteria(1e-6, 1e-6, 30)
    ests = [("gicp", R.TransformationEstimationForGeneralizedICP(R.L2Loss())), ("p2pl", R.TransformationEstimationPointToPlane()),
            ("p2p", R.TransformationEstimationPointToPoint()), ("p2pl", R.TransformationEstimationPointToPlane()),
            ("p2p", R.TransformationEstimationPointToPoint())]
    first = {}
    for name, est in ests:
        r = R.registration_icp(src, tgt, 0.6, T0, est, crit)
        key = (r.transformation.tobytes(), r.iterations, r.fitness, r.inlier_rmse)
        if name in first:
            assert key == first[name], name
        first.setdefault(name, key)
    assert first["p2p"][0] != first["p2pl"][0]


def test_switches_do_not_change_the_result():
    """Skip certificates, cell hash or octree, hipGraph replay: the same arithmetic scheduled another way, the same bits (the switches are
    latched per process: one child process each)."""
    lines = []
    for env in ({}, {"PCR_ICP_SKIP": "0"}, {"PCR_ICP_GRID": "0"}, {"PCR_ICP_GRAPH": "0"}):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "icp_pose.py")], env=dict(os.environ, **env), capture_output=True,
                             text=True, timeout=300)
        assert out.returncode == 0, (env, out.stderr[-2000:])
        got = [l for l in out.stdout.splitlines() if l.split(" ")[0] in ("P2PL", "P2P", "P2PS")]
        assert len(got) == 3, out.stdout[-2000:]
        lines.append((env, got))
    for env, got in lines[1:]:
        assert got == lines[0][1], (env, got, lines[0][1])
