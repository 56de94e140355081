"""GPU checks of the calls on a correspondence list the caller holds (include/pcr_hip.h): the estimators' compute_transformation /
compute_rmse against float64 restatements (tests/correspondence_reference.py), the loop's first update, the list sizes at which the
reduction takes another path, correspondences_from_features against a brute-force matcher, and the list forms of RANSAC and FGR against
their feature forms."""
import ctypes as C

import numpy as np
import pytest

from conftest import pkg, pose_error

import correspondence_reference as ref

pytestmark = pytest.mark.gpu

ROWS_PER_WORKGROUP, MAX_WORKGROUPS = 256, 256          # CORR_BS, CORR_MAX_BLOCKS of csrc/pcr_corres.hip


@pytest.fixture(scope="module")
def P():
    return pkg()


def _cloud(P, points, normals=None):
    pc = P.PointCloud(np.asarray(points, np.float32))
    if normals is not None:
        pc.normals = np.asarray(normals, np.float32)
    return pc


@pytest.fixture(scope="module")
def pair(P, small_pair):
    """Pair 899 at voxel 0.3, SOR(30, 1), KNN-20 normals (the clouds of tests/test_gpu_icp_estimators.py, about 12k points each), the source
    pre-aligned on the host in float64 by the shipped FGR pose and stored as a new float32 cloud; list A = the rows evaluate_registration
    finds at 0.6 m under the identity; list B = 3 n_src rows drawn from A with repeats, in random order."""
    out = []
    for key in ("source", "target"):
        pc = P.PointCloud(small_pair[key]).voxel_down_sample(0.3)
        pc, _ = pc.remove_statistical_outlier(30, 1.0)
        pc.estimate_normals(P.KDTreeSearchParamKNN(knn=20))
        out.append(pc)
    src0, tgt = out
    T = np.asarray(small_pair["T_fgr"], np.float64)
    src = _cloud(P, src0.points @ T[:3, :3].T + T[:3, 3], src0.normals @ T[:3, :3].T)
    A = P.registration.evaluate_registration(src, tgt, 0.6, np.eye(4)).correspondence_set.astype(np.int32)
    assert len(A) > 5000
    rng = np.random.default_rng(20)
    B = A[rng.integers(0, len(A), 3 * len(src))]
    assert len(np.unique(B[:, 0])) < len(B) and len(B) > len(src)
    src_c, tgt_c = _cloud(P, src.points), _cloud(P, tgt.points)
    src_c.estimate_covariances(); tgt_c.estimate_covariances()
    return dict(src=src, tgt=tgt, A=A, B=B, src_c=src_c, tgt_c=tgt_c, sx=src.points, tx=tgt.points, sn=src.normals, tn=tgt.normals)


def _kernel(R, loss, k=0.5):
    return {"l2": R.L2Loss(), "l1": R.L1Loss(), "gm": R.GMLoss(k)}[loss]


def _close(T, T_ref, what, scaled=False):
    ang, dt = pose_error(T, T_ref)
    print(f"{what}: {ang:.2e} rad {dt:.2e} m")
    assert ang < 1e-7 and dt < 1e-6, (what, ang, dt)           # the project's one-update tolerances (test_trajectory_matches_reference)
    if scaled:
        assert abs(np.cbrt(np.linalg.det(T[:3, :3])) - np.cbrt(np.linalg.det(T_ref[:3, :3]))) < 1e-7
    assert np.array_equal(T[3], [0, 0, 0, 1])


# ------------------------------------------------------------------------------------------------ 1. fits against the float64 reference
@pytest.mark.parametrize("which", ["A", "B"])
@pytest.mark.parametrize("scaling", [False, True])
def test_point_to_point_fit(P, pair, which, scaling):
    est = P.registration.TransformationEstimationPointToPoint(scaling)
    T = est.compute_transformation(pair["src"], pair["tgt"], pair[which])
    _close(T, ref.point_to_point(pair["sx"], pair["tx"], pair[which], scaling), f"p2p scaling={scaling} list {which}", scaled=scaling)


@pytest.mark.parametrize("which", ["A", "B"])
@pytest.mark.parametrize("loss", ["l2", "l1", "gm"])
def test_point_to_plane_fit(P, oracle, pair, which, loss):
    est = P.registration.TransformationEstimationPointToPlane(_kernel(P.registration, loss))
    T = est.compute_transformation(pair["src"], pair["tgt"], pair[which])
    _close(T, ref.point_to_plane(oracle, pair["sx"], pair["tx"], pair["tn"], pair[which], loss, 0.5), f"p2pl {loss} list {which}")
    assert not np.array_equal(T, np.eye(4))


@pytest.mark.parametrize("which", ["A", "B"])
@pytest.mark.parametrize("form", ["normals", "covariances"])
def test_generalized_icp_fit(P, oracle, pair, which, form):
    est = P.registration.TransformationEstimationForGeneralizedICP(P.registration.L1Loss())
    if form == "normals":
        T = est.compute_transformation(pair["src"], pair["tgt"], pair[which])
        T_ref = ref.generalized_icp(oracle, pair["sx"], pair["tx"], pair[which], "l1", src_normals=pair["sn"], tgt_normals=pair["tn"])
    else:
        T = est.compute_transformation(pair["src_c"], pair["tgt_c"], pair[which])
        T_ref = ref.generalized_icp(oracle, pair["sx"], pair["tx"], pair[which], "l1", src_cov=pair["src_c"].covariances, tgt_cov=pair["tgt_c"].covariances)
    _close(T, T_ref, f"gicp {form} list {which}")
    assert not np.array_equal(T, np.eye(4))


def test_generalized_icp_without_what_its_rows_need_is_the_identity(P, pair):
    est = P.registration.TransformationEstimationForGeneralizedICP(P.registration.L1Loss())
    bare_s, bare_t = _cloud(P, pair["sx"]), _cloud(P, pair["tx"])
    assert np.array_equal(est.compute_transformation(bare_s, bare_t, pair["A"]), np.eye(4))                  # neither normals nor covariances
    assert np.array_equal(est.compute_transformation(pair["src_c"], bare_t, pair["A"]), np.eye(4))           # covariances on one side only
    assert abs(est.compute_rmse(bare_s, bare_t, pair["A"][:10000]) / ref.rmse_euclidean(pair["sx"], pair["tx"], pair["A"][:10000]) - 1.0) < 1e-12


def test_rmse(P, pair):
    """Relative 1e-12: for C <= 40 000 non-negative float64 terms the relative error of the sum is below C 2^-53 = 4.4e-12 whatever the order,
    and the square root halves it; the lists here hold at most 10 000 rows (1.1e-12 before, 5.6e-13 after the root), so 1e-12 holds with margin."""
    R = P.registration
    for which in ("A", "B"):
        rows = pair[which][:10000]
        assert 5000 < len(rows) <= 10000
        e = ref.rmse_euclidean(pair["sx"], pair["tx"], rows)
        for est in (R.TransformationEstimationPointToPoint(), R.TransformationEstimationPointToPoint(True), R.TransformationEstimationForGeneralizedICP(R.L1Loss())):
            got = est.compute_rmse(pair["src"], pair["tgt"], rows)
            print(f"rmse {type(est).__name__} list {which}: {got!r} reference {e!r}")
            assert abs(got / e - 1.0) < 1e-12
        got = R.TransformationEstimationPointToPlane(R.GMLoss(0.5)).compute_rmse(pair["src"], pair["tgt"], rows)
        e = ref.rmse_plane(pair["sx"], pair["tx"], pair["tn"], rows)
        print(f"rmse point-to-plane list {which}: {got!r} reference {e!r}")
        assert e > 0 and abs(got / e - 1.0) < 1e-12


# ------------------------------------------------------------------------------------------------ 2. the loop's first update is the estimator's
def test_the_loops_first_update_is_the_estimators(P, pair):
    R = P.registration
    src, tgt, A = pair["src"], pair["tgt"], pair["A"]
    one, none = R.ICPConvergenceCriteria(1e-6, 1e-6, 1), R.ICPConvergenceCriteria(1e-6, 1e-6, 0)
    for est in (R.TransformationEstimationPointToPoint(), R.TransformationEstimationPointToPlane(R.GMLoss(0.5))):
        loop = R.registration_icp(src, tgt, 0.6, np.eye(4), est, one)
        assert loop.iterations == 1
        _close(loop.transformation, est.compute_transformation(src, tgt, A), f"loop vs estimator {type(est).__name__}")
    est = R.TransformationEstimationForGeneralizedICP(R.L1Loss())
    loop = R.registration_generalized_icp(src, tgt, 0.6, np.eye(4), est, one)
    assert loop.iterations == 1
    _close(loop.transformation, est.compute_transformation(src, tgt, A), "loop vs estimator GICP")
    # the loop's RMSE at init is Euclidean over the rows of its search: compute_rmse of the point-to-point and GICP estimators on that list
    at_init = R.registration_icp(src, tgt, 0.6, np.eye(4), R.TransformationEstimationPointToPoint(), none)
    assert at_init.iterations == 0 and np.array_equal(at_init.correspondence_set, A)
    assert abs(at_init.inlier_rmse - R.TransformationEstimationPointToPoint().compute_rmse(src, tgt, A)) < 1e-9
    at_init = R.registration_generalized_icp(src, tgt, 0.6, np.eye(4), est, none)
    assert at_init.iterations == 0 and abs(at_init.inlier_rmse - est.compute_rmse(src, tgt, A)) < 1e-9


# ------------------------------------------------------------------------------------------------ 3. list sizes
def _planted(n=300, seed=3, noise=1e-3, scale=1.0):
    """n points in a cube of side 4 about the origin, the first three a triangle of radius 2 about it; target = motion(source) + noise vectors
    drawn uniformly from the ball of radius `noise`.  A fit over the first three rows is then off by at most the mean of three such vectors in
    translation (their centroid is the origin, so the rotation's error has no lever: below `noise`) and by about noise / 2 in rotation."""
    rng = np.random.default_rng(seed)
    src = rng.uniform(-2, 2, (n, 3))
    src[:3] = [[2, 0, 0], [-1, 1.7320508, 0], [-1, -1.7320508, 0]]
    a = np.deg2rad(3.0)
    Rm = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]) @ np.array(
        [[1, 0, 0], [0, np.cos(a / 2), -np.sin(a / 2)], [0, np.sin(a / 2), np.cos(a / 2)]])
    T = np.eye(4); T[:3, :3] = scale * Rm; T[:3, 3] = [0.03, -0.02, 0.01]
    src = src.astype(np.float32).astype(np.float64)
    d = rng.standard_normal((n, 3))
    d *= (noise * np.cbrt(rng.uniform(0, 1, n)) / np.linalg.norm(d, axis=1))[:, None]
    tgt = src @ T[:3, :3].T + T[:3, 3] + d
    return src, tgt.astype(np.float32).astype(np.float64), T


@pytest.mark.parametrize("C_rows", [0, 1, 3, 255, 256, 257, ROWS_PER_WORKGROUP * MAX_WORKGROUPS + 1])
def test_list_sizes(P, oracle, C_rows):
    """0, 1, 3 rows; one below, at and above one workgroup's tile; one row past the tile times the widest grid (the grid-stride loop goes round)."""
    sx, tx, T_true = _planted()
    src, tgt = _cloud(P, sx), _cloud(P, tx)
    rows = np.stack([np.arange(C_rows) % 300, np.arange(C_rows) % 300], axis=1).astype(np.int32)
    est = P.registration.TransformationEstimationPointToPoint()
    T, e = est.compute_transformation(src, tgt, rows), est.compute_rmse(src, tgt, rows)
    T2, e2 = est.compute_transformation(src, tgt, rows), est.compute_rmse(src, tgt, rows)
    assert T.tobytes() == T2.tobytes() and e == e2                       # the same bits when called twice
    if C_rows == 0:
        assert np.array_equal(T, np.eye(4)) and e == 0.0
    elif C_rows == 1:
        assert np.isfinite(T).all() and np.isfinite(e)
    else:
        ang, dt = pose_error(T, T_true)
        print(f"C = {C_rows}: {ang:.2e} rad {dt:.2e} m from the planted motion, rmse {e:.3e}")
        assert ang < 1e-3 and dt < 1e-3, (C_rows, ang, dt)
        _close(T, ref.point_to_point(sx, tx, rows), f"C = {C_rows} against the reference")
        # (C 2^-53 / 2 again: 3.6e-12 for the 65 537 rows of the longest list)
        assert abs(e / ref.rmse_euclidean(sx, tx, rows) - 1.0) < (1e-12 if C_rows <= 10000 else 1e-11)
    # the 6x6 form at the same sizes: the same bits twice; the reference from 255 rows on (fewer rows than unknowns leave a singular system)
    nrm = np.random.default_rng(12).standard_normal((300, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32).astype(np.float64)
    tgt_n = _cloud(P, tx, nrm)
    pl = P.registration.TransformationEstimationPointToPlane()
    Tp = pl.compute_transformation(src, tgt_n, rows)
    assert Tp.tobytes() == pl.compute_transformation(src, tgt_n, rows).tobytes()
    if C_rows == 0:
        assert np.array_equal(Tp, np.eye(4)) and pl.compute_rmse(src, tgt_n, rows) == 0.0
    elif C_rows >= 255:
        _close(Tp, ref.point_to_plane(oracle, sx, tx, nrm, rows), f"point-to-plane, C = {C_rows}")


# ------------------------------------------------------------------------------------------------ 4. a planted similarity
def test_point_to_point_recovers_a_planted_similarity(P, pair):
    src = pair["sx"]
    a = np.deg2rad(3.0)
    Rm = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]) @ np.array(
        [[1, 0, 0], [0, np.cos(a / 2), -np.sin(a / 2)], [0, np.sin(a / 2), np.cos(a / 2)]])
    s, t = 1.05, np.array([0.03, -0.02, 0.01])
    tgt = (s * src @ Rm.T + t).astype(np.float32)
    rows = np.stack([np.arange(len(src)), np.arange(len(src))], axis=1)
    Tr = P.registration.TransformationEstimationPointToPoint(True).compute_transformation(pair["src"], _cloud(P, tgt), rows)
    sr = np.cbrt(np.linalg.det(Tr[:3, :3]))
    assert abs(sr - s) < 1e-6, sr
    assert np.abs(Tr[:3, :3] / sr - Rm).max() < 1e-6 and np.abs(Tr[:3, 3] - t).max() < 1e-6, Tr
    rigid = P.registration.TransformationEstimationPointToPoint(False).compute_transformation(pair["src"], _cloud(P, tgt), rows)
    assert abs(np.linalg.det(rigid[:3, :3]) - 1.0) < 1e-9


# ------------------------------------------------------------------------------------------------ 5. correspondences_from_features
@pytest.fixture(scope="module")
def synthetic_features():
    """1500 x 1200 standard normal float32 rows of 33, with 20 target rows duplicated and 10 all-zero rows on both sides (exact ties)."""
    rng = np.random.default_rng(33)
    fs = rng.standard_normal((1500, 33)).astype(np.float32)
    ft = rng.standard_normal((1200, 33)).astype(np.float32)
    ft[600:620] = ft[100:120]
    fs[40:50] = 0.0
    ft[700:710] = 0.0
    return fs, ft


def _assert_no_near_ties(a, b):
    """the test's own inputs: a row's best and second-best float64 distances are equal (an exact tie, decided by the index) or more than
    1e-9 relative apart, so that no row depends on the order of a float64 sum"""
    _, best, second = ref.nearest_rows(a, b)
    tied = second == best
    assert ((second - best)[~tied] > 1e-9 * second[~tied]).all()
    return int(tied.sum())


def test_correspondences_from_features_on_synthetic_rows(P, synthetic_features):
    import torch
    fs, ft = synthetic_features
    tied_s, tied_t = _assert_no_near_ties(fs, ft), _assert_no_near_ties(ft, fs)
    assert tied_s >= 10 and tied_t >= 10                   # the zero rows (and whatever points at a duplicated target row)
    R = P.registration
    Fs, Ft = R.Feature(torch.from_numpy(fs).cuda()), R.Feature(torch.from_numpy(ft).cuda())
    all_rows, n_mutual = ref.match_features(fs, ft, False)
    assert 0 < n_mutual < int(0.9 * len(fs)) and n_mutual >= int(0.1 * len(fs))
    got = R.correspondences_from_features(Fs, Ft)
    assert got.is_cuda and got.dtype == torch.int32 and tuple(got.shape) == (1500, 2)
    assert np.array_equal(got.cpu().numpy(), all_rows)
    for ratio in (0.0, 0.1, 0.9):
        want, _ = ref.match_features(fs, ft, True, ratio)
        assert len(want) == (len(fs) if ratio == 0.9 else n_mutual)         # 0.9 falls back to all rows
        assert np.array_equal(R.correspondences_from_features(Fs, Ft, True, ratio).cpu().numpy(), want), ratio
        assert np.array_equal(R.correspondences_from_features(Fs, Ft, False, ratio).cpu().numpy(), all_rows)
    # five sources that all point at target row 0: one mutual row.  A ratio of 0 returns it, 0.9 asks for int(0.9 * 5) = 4 and gets all rows
    few_s = R.Feature(torch.from_numpy(np.stack([ft[0] + 0.1 * (k + 1) for k in range(5)]).astype(np.float32)).cuda())
    few_t = R.Feature(torch.from_numpy(ft[:3].copy()).cuda())
    assert R.correspondences_from_features(few_s, few_t, True, 0.0).cpu().numpy().tolist() == [[0, 0]]
    assert R.correspondences_from_features(few_s, few_t, True, 0.9).cpu().numpy().tolist() == [[k, 0] for k in range(5)]
    with pytest.raises(RuntimeError, match="33-dimensional"):
        R.correspondences_from_features(R.Feature(torch.zeros((4, 32), device="cuda")), R.Feature(torch.zeros((4, 32), device="cuda")))
    empty = R.Feature(torch.zeros((0, 33), device="cuda"))
    assert tuple(R.correspondences_from_features(empty, Ft).shape) == (0, 2) and tuple(R.correspondences_from_features(Fs, empty, True).shape) == (0, 2)


@pytest.fixture(scope="module")
def fpfh_pair(P, pair):
    """every third point of the two clouds with their FPFH features, the larger cloud as the source (the feature form of FGR then keeps its
    cross-checked list in source order)"""
    out = []
    for pc in (pair["src"], pair["tgt"]):
        sub = pc.select_by_index(np.arange(0, len(pc), 3))
        out.append((sub, P.registration.compute_fpfh_feature(sub, P.KDTreeSearchParamHybrid(radius=1.5, max_nn=100))))
    out.sort(key=lambda cf: -len(cf[0]))
    (src, fs), (tgt, ft) = out
    assert len(src) >= len(tgt)
    return src, fs, tgt, ft


def test_correspondences_from_features_on_fpfh(P, fpfh_pair):
    src, fs, tgt, ft = fpfh_pair
    a, b = fs._dev.cpu().numpy(), ft._dev.cpu().numpy()
    for mutual in (False, True):
        want, n_mutual = ref.match_features(a, b, mutual, 0.0)
        got = P.registration.correspondences_from_features(fs, ft, mutual, 0.0).cpu().numpy()
        assert got.shape == want.shape and np.array_equal(got, want), (mutual, int((got != want).any(1).sum()) if got.shape == want.shape else None)
    assert n_mutual > 10


# ------------------------------------------------------------------------------------------------ 6. the same answer as the feature forms
def _same(a, b):
    return (a.transformation.tobytes() == b.transformation.tobytes() and a.fitness == b.fitness and a.inlier_rmse == b.inlier_rmse
            and np.array_equal(a.correspondence_set, b.correspondence_set))


def test_ransac_on_the_list_equals_the_feature_form(P, fpfh_pair):
    R = P.registration
    src, fs, tgt, ft = fpfh_pair
    rows = R.correspondences_from_features(fs, ft, True, 0.0)
    assert rows.shape[0] >= 3                               # the feature form keeps the mutual rows when there are at least ransac_n
    kw = dict(ransac_n=3, checkers=[R.CorrespondenceCheckerBasedOnEdgeLength(0.9), R.CorrespondenceCheckerBasedOnDistance(0.5)],
              criteria=R.RANSACConvergenceCriteria(4000, 0.999), seed=11)
    feat = R.registration_ransac_based_on_feature_matching(src, tgt, fs, ft, True, 0.5, **kw)
    lst = R.registration_ransac_based_on_correspondence(src, tgt, rows, 0.5, **kw)
    assert feat.n_corres == rows.shape[0] and feat.iterations == lst.iterations and feat.best_iteration == lst.best_iteration
    assert _same(feat, lst)


def test_fgr_on_the_list_equals_the_feature_form(P, fpfh_pair):
    R = P.registration
    src, fs, tgt, ft = fpfh_pair
    rows = R.correspondences_from_features(fs, ft, True, 0.0)
    opt = R.FastGlobalRegistrationOption(1.4, True, True, 0.6, 64, 0.95, 500, True, seed=77)
    feat = R.registration_fgr_based_on_feature_matching(src, tgt, fs, ft, opt)
    lst = R.registration_fgr_based_on_correspondence(src, tgt, rows, opt)
    assert _same(feat, lst)
    assert not np.array_equal(lst.transformation[:3, :3], np.eye(3))
    assert _same(lst, R.registration_fgr_based_on_correspondence(src, tgt, rows.cpu().numpy(), opt))          # a host list is the same list


def test_fgr_on_a_list_without_the_tuple_test_and_a_larger_target(P):
    """500 exact pairs of a planted motion, a fifth of them with a random target index, a target of 600 points: every row goes to the optimiser
    (the feature form refuses tuple_test=False with the larger target), whose annealed weights switch the wrong rows off."""
    sx, tx, T_true = _planted(500, seed=8, noise=0.0)
    rng = np.random.default_rng(9)
    tx = np.concatenate([tx, rng.uniform(-2, 2, (100, 3))])
    rows = np.stack([np.arange(500), np.arange(500)], axis=1).astype(np.int32)
    wrong = rng.permutation(500)[:100]
    rows[wrong, 1] = rng.integers(0, 600, 100)
    noise = 1e-3          # float32 rounding of the coordinates is 2e-7: the pairs are exact far below this
    opt = P.registration.FastGlobalRegistrationOption(1.4, False, True, noise, 128, 0.95, 1000, False, seed=1)
    res = P.registration.registration_fgr_based_on_correspondence(_cloud(P, sx), _cloud(P, tx), rows, opt)
    ang, dt = pose_error(res.transformation, T_true)
    print(f"fgr on a list, 20 % wrong rows: {ang:.2e} rad {dt:.2e} m, fitness {res.fitness:.3f}")
    assert ang < 1e-3 and dt < 1e-3, (ang, dt)
    # fewer than 10 rows: the identity in the normalised frame = the centroids on each other (as the feature form)
    few = P.registration.registration_fgr_based_on_correspondence(_cloud(P, sx), _cloud(P, tx), rows[:9], opt)
    expect = np.eye(4); expect[:3, 3] = tx.mean(0) - sx.mean(0)
    assert np.allclose(few.transformation, expect, atol=1e-6)


# ------------------------------------------------------------------------------------------------ 7. registro_manual
def test_registro_manual_gives_the_planted_motion(P):
    """five picks; the coordinates are exact up to float32 rounding (2.4e-7 at |x| <= 2), the picks span 2 m and more: 1e-5 holds with margin"""
    sx, tx, T_true = _planted(300, seed=4, noise=0.0)
    rng = np.random.default_rng(6)
    perm = rng.permutation(300)                             # the target in another order: picks are index pairs, not equal indices
    tgt = _cloud(P, tx[perm])
    where = np.argsort(perm)
    picks_s = [0, 1, 2, 17, 230]
    T = P.registro_manual(_cloud(P, sx), tgt, picks_s, [int(where[i]) for i in picks_s])
    assert T.shape == (4, 4) and T.dtype == np.float64
    ang, dt = pose_error(T, T_true)
    assert ang < 1e-5 and dt < 1e-5, (ang, dt)


# ------------------------------------------------------------------------------------------------ 8. error paths
def test_errors_leave_the_context_usable(P, pair):
    import torch
    R = P.registration
    src, tgt, A = pair["src"], pair["tgt"], pair["A"]
    est = R.TransformationEstimationPointToPoint()
    good = est.compute_transformation(src, tgt, A)
    bad = A.copy(); bad[7, 0] = len(src)
    for rows in (bad, torch.from_numpy(bad).cuda()):
        with pytest.raises(RuntimeError, match="out of range"):
            est.compute_transformation(src, tgt, rows)
        with pytest.raises(RuntimeError, match="out of range"):
            R.registration_fgr_based_on_correspondence(src, tgt, rows)
    # the library checks the list itself, on the device (a caller of the C ABI has no Python in front)
    ctx = P._lib.Context.current()
    cd = torch.from_numpy(bad).cuda()
    e = est._estimation()
    T = np.full(16, 7.0)
    args = (C.byref(e), C.c_void_p(src.device_xyz().data_ptr()), None, None, C.c_int64(len(src)), C.c_void_p(tgt.device_xyz().data_ptr()), None, None,
            C.c_int64(len(tgt)), C.c_void_p(cd.data_ptr()), C.c_int64(len(bad)))
    rc = ctx.lib.pcr_estimation_compute_transformation(ctx.handle, *args, T.ctypes.data_as(C.POINTER(C.c_double)))
    assert rc == P._lib.PCR_EINVAL and b"out of range" in ctx.lib.pcr_last_error(ctx.handle)
    assert np.array_equal(T.reshape(4, 4), np.eye(4))
    out = np.full(1, 7.0)
    rc = ctx.lib.pcr_estimation_compute_rmse(ctx.handle, *args, out.ctypes.data_as(C.POINTER(C.c_double)))
    assert rc == P._lib.PCR_EINVAL and out[0] == 0.0
    res, o = P._lib.PcrResult(), R._fgr_option(R.FastGlobalRegistrationOption(seed=1))
    rc = ctx.lib.pcr_registration_fgr_correspondence(ctx.handle, C.c_void_p(src.device_xyz().data_ptr()), C.c_int64(len(src)), C.c_void_p(tgt.device_xyz().data_ptr()),
                                                     C.c_int64(len(tgt)), C.c_void_p(cd.data_ptr()), C.c_int64(len(bad)), C.byref(o), C.byref(res), None)
    assert rc == P._lib.PCR_EINVAL and b"out of range" in ctx.lib.pcr_last_error(ctx.handle)
    # ... and the next call succeeds, with the bits of the call before
    assert est.compute_transformation(src, tgt, A).tobytes() == good.tobytes()
    # point-to-plane without target normals: the identity and 0 (Open3D)
    pl = R.TransformationEstimationPointToPlane()
    bare = _cloud(P, pair["tx"])
    assert np.array_equal(pl.compute_transformation(src, bare, A), np.eye(4)) and pl.compute_rmse(src, bare, A) == 0.0
    # a system without a solution (normals of length zero: JTJ = 0) gives the identity too
    flat = _cloud(P, pair["tx"], np.zeros_like(pair["tx"]))
    assert np.array_equal(pl.compute_transformation(src, flat, A), np.eye(4)) and pl.compute_rmse(src, flat, A) == 0.0
    # an empty list on every estimator
    none = np.zeros((0, 2), np.int32)
    for e_ in (est, pl, R.TransformationEstimationForGeneralizedICP()):
        assert np.array_equal(e_.compute_transformation(src, tgt, none), np.eye(4)) and e_.compute_rmse(src, tgt, none) == 0.0
