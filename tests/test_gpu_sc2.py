"""Spatial-compatibility (SC2) global registration on the device against the numpy restatement of its rule (tests/sc2_reference.py;
include/pcr_hip.h states the rule).  Bits, degrees, scores, seeds and the member rows of K1 and K2 are integers or float64 comparisons made
by the same expression on both sides, so they are compared exactly, on inputs where the restatement finds no pair and no row within 1e-9
relative of a threshold (asserted: a condition on the inputs).  The hypotheses are checked by certificate, as test_gpu_ransac.py checks
RANSAC's: a rotation, a residual over K2 within (1 + 1e-9) of numpy's own fit, and count / err2 equal to the float64 recount under the
device's own pose.  The selection and the refinement are then restated on the device's hypotheses."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import sc2_reference as ref
from conftest import pkg, pose_error

pytestmark = pytest.mark.gpu

TAU = 0.1


@pytest.fixture(scope="module")
def P():
    return pkg()


@functools.lru_cache(maxsize=None)
def planted(n, f, sigma, seed):
    return ref.planted_list(n, f, sigma, seed)


@functools.lru_cache(maxsize=None)
def graph_of(n):
    """A planted list of n rows and its restated graph: (src, tgt, corres, C, rim, deg, score)."""
    src, tgt, corres, _ = planted(n, 0.05, 0.02, 100 + n)
    s, t = ref.list_points(src, tgt, corres)
    Cm, rim = ref.compatibility(s, t, TAU)
    deg, score = ref.degrees_scores(Cm)
    return src, tgt, corres, Cm, rim, deg, score


def check_graph(P, src, tgt, corres, tau, Cm, rim, deg, score):
    assert rim == 0
    n = len(corres)
    g = P.spatial_compatibility(P.PointCloud(src), P.PointCloud(tgt), corres, tau)
    bits = g.bits.cpu().numpy()
    assert bits.shape == (n, (n + 63) // 64) and bits.dtype == np.int64
    if n % 64:
        assert not (bits[:, -1].view(np.uint64) >> np.uint64(n % 64)).any()          # tail bits are zero
    assert np.array_equal(bits, ref.pack_bits(Cm))
    assert g.degrees.dtype.is_floating_point is False and np.array_equal(g.degrees.cpu().numpy(), deg)
    assert np.array_equal(g.scores.cpu().numpy(), score)
    return g


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 130, 1000])
def test_bits_degrees_scores_equal_the_restatement(P, n):
    src, tgt, corres, Cm, rim, deg, score = graph_of(n)
    check_graph(P, src, tgt, corres, TAU, Cm, rim, deg, score)
    if n >= 63:
        assert Cm.any() and score.max() > 0


def test_a_row_repeated_three_times(P):
    src, tgt, corres, *_ = graph_of(130)
    corres = corres.copy()
    corres[70] = corres[5]
    corres[129] = corres[5]
    s, t = ref.list_points(src, tgt, corres)
    Cm, rim = ref.compatibility(s, t, TAU)
    assert Cm[5, 70] and Cm[70, 129] and Cm[129, 5] and not Cm[5, 5]            # repeated rows are compatible with each other, never with themselves
    deg, score = ref.degrees_scores(Cm)
    check_graph(P, src, tgt, corres, TAU, Cm, rim, deg, score)


def test_more_than_one_tile_in_each_direction(P):
    """8192 rows: 128 words per row, 32 row blocks of the bit kernel's grid, rows of the score pass that span several passes of a wavefront."""
    n = 8192
    src, tgt, corres, _ = planted(n, 0.01, 0.02, 7)
    s, t = ref.list_points(src, tgt, corres)
    Cm, rim = ref.compatibility(s, t, TAU)
    deg, score = ref.degrees_scores(Cm)
    check_graph(P, src, tgt, corres, TAU, Cm, rim, deg, score)


# ------------------------------------------------------------------------------------------------------------ seeds and hypotheses
def strip(row):
    return row[row >= 0]


def check_seeds_and_hypotheses(P, src, tgt, corres, tau, **kw):
    """Seeds, K1, K2 against the restatement (exact); every hypothesis by certificate.  Returns (debug dump, restatement, s, t)."""
    R = P.registration
    opt = R.SpatialCompatibilityOption(tau, **kw)
    dbg = R.debug_sc2_seeds(P.PointCloud(src), P.PointCloud(tgt), corres, opt)
    r = ref.register(src, tgt, corres, tau, **kw)
    assert r["rim"] == 0
    s, t = ref.list_points(src, tgt, corres)
    assert np.array_equal(dbg["seeds"], r["seeds"])
    S = len(r["seeds"])
    for k in range(S):
        assert dbg["k1"][k][0] == r["seeds"][k] and dbg["k2"][k][0] == r["seeds"][k]
        assert np.array_equal(strip(dbg["k1"][k]), r["K1"][k]), k
        assert np.array_equal(strip(dbg["k2"][k]), r["K2"][k]), k
    assert np.array_equal(dbg["valid"], r["valid"])
    n_checked = 0
    for k in range(S):
        T = dbg["T"][k]
        if not dbg["valid"][k]:
            assert dbg["count"][k] == -1 and dbg["err2"][k] == 0.0 and len(r["K2"][k]) < 3 and not T[:3].any()
            continue
        Rm = T[:3, :3]
        assert np.abs(Rm.T @ Rm - np.eye(3)).max() < 1e-9 and abs(np.linalg.det(Rm) - 1.0) < 1e-9 and np.array_equal(T[3], [0, 0, 0, 1])
        K2 = r["K2"][k]
        res_dev = float(ref.residual2(T, s[K2], t[K2]).sum())
        res_ref = float(ref.residual2(ref.fit(s[K2], t[K2]), s[K2], t[K2]).sum())
        floor = 1e-24 * len(K2)            # (coordinates of tens of metres rounded to float64: 1e-14 m per residual at the very most)
        assert res_ref * (1 - 1e-9) - floor <= res_dev <= res_ref * (1 + 1e-9) + floor, (k, res_dev, res_ref)
        d2 = ref.residual2(T, s, t)
        inl = d2 < tau * tau
        assert not (np.abs(np.sqrt(d2) - tau) <= ref.RIM * tau).any()
        e = math.fsum(d2[inl].tolist())
        assert dbg["count"][k] == int(inl.sum()), k
        assert abs(dbg["err2"][k] - e) <= 1e-12 * e, (k, dbg["err2"][k], e)
        n_checked += 1
    return dbg, r, s, t, n_checked


def check_result(P, src, tgt, corres, tau, dbg, s, t, **kw):
    """The registration call against the selection and refinement restated on the device's own hypotheses and figures."""
    R = P.registration
    res = R.registration_sc2_based_on_correspondence(P.PointCloud(src), P.PointCloud(tgt), corres, R.SpatialCompatibilityOption(tau, **kw))
    best = ref.select_best(dbg["count"], dbg["err2"])
    n = len(corres)
    assert res.info["n_corres"] == n and res.info["n_seeds"] == len(dbg["seeds"]) and res.info["n_valid"] == int(dbg["valid"].sum())
    assert res.info["best_seed"] == best
    if best < 0:
        assert np.array_equal(res.transformation, np.eye(4)) and res.fitness == 0.0 and res.inlier_rmse == 0.0 and not res.converged
        assert len(res.correspondence_set) == 0 and res.info["best_seed_count"] == 0 and res.info["refine_iterations_run"] == 0
        return res
    assert res.info["best_seed_count"] == dbg["count"][best] and res.converged
    T, inl, c, e, rim = ref.refine(dbg["T"][best], s, t, tau, kw.get("refine_iterations", 20))
    assert rim == 0
    ang, dt = pose_error(res.transformation, T)
    print(f"n={n} {kw}: {len(dbg['seeds'])} seeds, {int(dbg['valid'].sum())} valid, best {best} ({dbg['count'][best]} rows) -> {c} rows after "
          f"{res.info['refine_iterations_run']} passes; device vs restatement {ang:.1e} rad {dt:.1e} m")
    assert ang < 1e-9 and dt < 1e-9, (ang, dt)
    assert np.array_equal(np.asarray(res.correspondence_set), np.asarray(corres)[inl])
    assert res.fitness == c / n and abs(res.inlier_rmse - math.sqrt(e / c)) <= 1e-9 * math.sqrt(e / c)
    assert 0 <= res.info["refine_iterations_run"] <= kw.get("refine_iterations", 20) and res.iterations == res.info["refine_iterations_run"]
    return res


CASES = [dict(), dict(k1=63, k2=63), dict(nms_radius=0.0), dict(nms_radius=1e9), dict(seed_ratio=1.0, max_seeds=7), dict(k1=2, k2=1)]


@pytest.mark.parametrize("kw", CASES, ids=["default", "k63", "nms0", "nms1e9", "ratio1_max7", "k1_2_k2_1"])
def test_seeds_members_hypotheses_and_result(P, kw):
    src, tgt, corres, T_true = planted(1000, 0.05, 0.02, 0)
    dbg, r, s, t, n_checked = check_seeds_and_hypotheses(P, src, tgt, corres, TAU, **kw)
    S = len(dbg["seeds"])
    assert S >= 1
    if kw.get("nms_radius") == 1e9:
        assert S == 1
    if kw.get("max_seeds") == 7:
        assert S == 7
    if kw.get("nms_radius") == 0.0:
        assert S == min(200, int((r["score"] > 0).sum()))
    if kw.get("k1") == 2:
        assert n_checked == 0 and not dbg["valid"].any()          # K2 has at most 2 rows: every seed is invalid, the result empty
    elif kw.get("nms_radius") != 1e9:
        assert n_checked >= 1
    if kw.get("k1") == 63:
        assert max(len(k) for k in r["K1"]) > 31 and max(len(k) for k in r["K2"]) > 21          # more members than the defaults allow
    res = check_result(P, src, tgt, corres, TAU, dbg, s, t, **kw)
    if kw.get("k1") == 2:
        assert not res.converged and res.fitness == 0.0


@pytest.mark.parametrize("n,f,seed", [(n, f, seed) for n, f in ((1000, 0.05), (1000, 0.02), (2000, 0.01)) for seed in (0, 1, 2)])
def test_planted_pose_on_the_device(P, n, f, seed):
    """The planted cases of test_sc2_api.py: within 1e-3 rad and 5e-2 m of the planted pose, and the restatement's count."""
    R = P.registration
    src, tgt, corres, T_true = planted(n, f, 0.02, seed)
    r = ref.register(src, tgt, corres, TAU)
    assert r["rim"] == 0
    res = R.registration_sc2_based_on_correspondence(P.PointCloud(src), P.PointCloud(tgt), corres, R.SpatialCompatibilityOption(TAU))
    ang, dt = ref.pose_error(res.transformation, T_true)
    print(f"planted n={n} f={f} seed={seed}: device {ang:.2e} rad {dt:.2e} m from the planted pose, {len(res.correspondence_set)} rows (restatement {r['n_inliers']})")
    assert ang < 1e-3 and dt < 5e-2, (ang, dt)
    assert len(res.correspondence_set) == r["n_inliers"] and res.fitness == r["n_inliers"] / n


# ------------------------------------------------------------------------------------------------------------ pair 899
@pytest.fixture(scope="module")
def pair899(P, small_pair):
    """Clouds with Hybrid(0.2, 20) normals, their FPFH Hybrid(1.0, 200) features and the mutual list, all from the device."""
    out = []
    for key in ("source", "target"):
        pc = P.PointCloud(small_pair[key])
        pc.estimate_normals(P.KDTreeSearchParamHybrid(radius=0.2, max_nn=20))
        out.append((pc, P.registration.compute_fpfh_feature(pc, P.KDTreeSearchParamHybrid(radius=1.0, max_nn=200))))
    (src, fs), (tgt, ft) = out
    corres = P.registration.correspondences_from_features(fs, ft, True).cpu().numpy()
    return src, fs, tgt, ft, corres


def test_pair_899_mutual_list(P, pair899, small_pair):
    """Bound against T_gicp: 3e-2 rad / 0.25 m, about three times what the CPU prototype measured with oracle features on its mutual list
    (1.07e-2 rad / 7.9e-2 m); the device's list differs slightly."""
    R = P.registration
    src, fs, tgt, ft, corres = pair899
    tau = 0.5
    sx, tx = src.device_xyz().cpu().numpy(), tgt.device_xyz().cpu().numpy()
    assert 3 <= len(corres) <= 65536
    dbg, r, s, t, n_checked = check_seeds_and_hypotheses(P, sx, tx, corres, tau)
    assert n_checked >= 1
    res = check_result(P, sx, tx, corres, tau, dbg, s, t)
    ang, dt = pose_error(res.transformation, small_pair["T_gicp"])
    n_true = int((ref.residual2(np.asarray(small_pair["T_gicp"], float), s, t) < tau * tau).sum())
    print(f"pair 899, mutual list of {len(corres)} rows ({n_true} within {tau} m under T_gicp): {len(res.correspondence_set)} inliers, "
          f"{ang:.3e} rad {dt:.3e} m from T_gicp")
    assert ang < 3e-2 and dt < 0.25, (ang, dt)
    # the feature form is the list form on the list the features give
    rf = R.registration_sc2_based_on_feature_matching(src, tgt, fs, ft, R.SpatialCompatibilityOption(tau))
    assert np.array_equal(rf.transformation, res.transformation) and rf.fitness == res.fitness and rf.inlier_rmse == res.inlier_rmse
    assert np.array_equal(np.asarray(rf.correspondence_set), np.asarray(res.correspondence_set)) and rf.info == res.info


# ------------------------------------------------------------------------------------------------------------ other checks
def test_two_runs_give_the_same_bits(P):
    R = P.registration
    src, tgt, corres, _ = planted(2000, 0.01, 0.02, 1)
    a, b = (R.registration_sc2_based_on_correspondence(P.PointCloud(src), P.PointCloud(tgt), corres, R.SpatialCompatibilityOption(TAU)) for _ in range(2))
    assert a.transformation.tobytes() == b.transformation.tobytes() and a.fitness == b.fitness and a.inlier_rmse == b.inlier_rmse and a.info == b.info
    assert np.array_equal(np.asarray(a.correspondence_set), np.asarray(b.correspondence_set)) and a.converged
    g, h = (R.spatial_compatibility(P.PointCloud(src), P.PointCloud(tgt), corres, TAU) for _ in range(2))
    assert bool((g.bits == h.bits).all()) and bool((g.scores == h.scores).all()) and bool((g.degrees == h.degrees).all())


def _raw_call(P, n_src, n_tgt, corres_dev, tau=0.5):
    import torch
    L = P._lib
    ctx = L.Context.current()
    pts = torch.zeros((max(n_src, n_tgt), 3), dtype=torch.float32, device="cuda")
    opt, res, info = L.PcrSc2Option(tau, tau, 30, 20, 0.2, 2048, 20), L.PcrResult(), L.PcrSc2Info()
    rc = ctx.lib.pcr_registration_sc2_correspondence(ctx.handle, C.c_void_p(pts.data_ptr()), n_src, C.c_void_p(pts.data_ptr()), n_tgt, C.c_void_p(corres_dev.data_ptr()),
                                                     corres_dev.shape[0], C.byref(opt), C.byref(res), None, C.byref(info))
    rc2 = ctx.lib.pcr_spatial_compatibility(ctx.handle, C.c_void_p(pts.data_ptr()), n_src, C.c_void_p(pts.data_ptr()), n_tgt, C.c_void_p(corres_dev.data_ptr()),
                                            corres_dev.shape[0], tau, None, None, None)
    return rc, rc2, (ctx.lib.pcr_last_error(ctx.handle) or b"").decode()


def test_65537_rows_are_refused_before_any_allocation(P):
    import torch
    R = P.registration
    corres = torch.zeros((65537, 2), dtype=torch.int32, device="cuda")
    src = P.PointCloud(np.zeros((4, 3)))
    with pytest.raises(RuntimeError, match="the limit is 65536"):
        R.registration_sc2_based_on_correspondence(src, src, corres, R.SpatialCompatibilityOption(0.5))
    P._lib.Context.current()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    rc, rc2, msg = _raw_call(P, 4, 4, corres)
    free1 = torch.cuda.mem_get_info()[0]
    assert rc == P._lib.PCR_EINVAL and rc2 == P._lib.PCR_EINVAL and "65536" in msg and "mutual filter" in msg and "keypoint subset" in msg
    assert free0 - free1 < (64 << 20), (free0, free1)          # (the bit matrix of 65537 rows alone would take 537 MB)


def test_an_index_out_of_range_is_refused(P):
    import torch
    R = P.registration
    src, tgt, corres, _ = planted(130, 0.05, 0.02, 230)
    bad = corres.copy()
    bad[17, 1] = len(tgt)
    with pytest.raises(RuntimeError, match="out"):
        R.registration_sc2_based_on_correspondence(P.PointCloud(src), P.PointCloud(tgt), bad, R.SpatialCompatibilityOption(TAU))
    with pytest.raises(RuntimeError, match="out"):
        R.spatial_compatibility(P.PointCloud(src), P.PointCloud(tgt), torch.as_tensor(bad, device="cuda"), TAU)
    rc, rc2, msg = _raw_call(P, len(src), len(tgt), torch.as_tensor(bad, device="cuda"))          # the library's own check, under the Python layer's
    assert rc == P._lib.PCR_EINVAL and rc2 == P._lib.PCR_EINVAL and "out of range" in msg


def test_short_lists_give_the_empty_result(P):
    R = P.registration
    src, tgt, corres, _ = planted(130, 0.05, 0.02, 230)
    for n in (0, 1, 2):
        res = R.registration_sc2_based_on_correspondence(P.PointCloud(src), P.PointCloud(tgt), corres[:n].reshape(-1, 2), R.SpatialCompatibilityOption(TAU))
        assert np.array_equal(res.transformation, np.eye(4)) and res.fitness == 0.0 and not res.converged and len(res.correspondence_set) == 0
        assert res.info["n_corres"] == n and res.info["best_seed"] == -1
