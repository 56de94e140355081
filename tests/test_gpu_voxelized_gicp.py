"""Voxelized GICP on the device against the numpy restatement of its rule (tests/voxelized_gicp_reference.py): the map bit for bit, the
rows exactly, the trajectories of the loop, and the edges.  Pair 899 with both clouds at voxel 0.3 against a 1.0 m map (the condition of these
comparisons -- most source points have a row -- is checked on the CPU in tests/test_voxelized_gicp_api.py), and clouds of tens of points."""
import ctypes as C
import functools

import numpy as np
import pytest

import voxel_reference as vr
import voxelized_gicp_reference as vg
from conftest import l1_tolerance, pkg, pose_error

pytestmark = pytest.mark.gpu

MAP_VOXEL = 1.0
LOSS = {"l2": 0, "l1": 1, "gm": 2}


@pytest.fixture(scope="module")
def P():
    return pkg()


@pytest.fixture(scope="module")
def clouds(P, small_pair):
    """pair 899 at voxel 0.3 with KNN-20 normals (6897 / 7074 points); the float32 arrays the device holds are what the reference gets"""
    out = {}
    for key in ("source", "target"):
        pc = P.PointCloud(small_pair[key]).voxel_down_sample(0.3)
        pc.estimate_normals(P.KDTreeSearchParamKNN(knn=20))
        out[key] = pc
        out[key + "_xyz"] = pc._xyz.cpu().numpy()
        out[key + "_cov6"] = vg.cov6_from_normals(pc._nrm.cpu().numpy())
    assert (len(out["source"]), len(out["target"])) == (6897, 7074)
    return out


@pytest.fixture(scope="module")
def ref_map(clouds):
    return vg.build_map(clouds["target_xyz"], clouds["target_cov6"], MAP_VOXEL)


@pytest.fixture(scope="module")
def dev_map(P, clouds):
    m = P.registration.VoxelCovarianceMap(clouds["target"], MAP_VOXEL)
    yield m
    m.close()


def _assert_map_equals(dev, ref):
    assert len(dev) == len(ref.cells)
    assert np.array_equal(dev.cells, ref.cells)                       # the same cells in the same (Morton) order
    assert np.array_equal(dev.counts, ref.count)
    assert vr.bits_equal(dev.points, ref.mean)
    assert vr.bits_equal(dev.covariances, ref.cov6)


# ------------------------------------------------------------------------------------------ the map, bit for bit
def test_map_from_estimated_covariances(P, clouds):
    pc = P.PointCloud(clouds["target_xyz"])
    pc.estimate_covariances(P.KDTreeSearchParamKNN(knn=20))
    cov6 = pc._cov.cpu().numpy()
    ref = vg.build_map(clouds["target_xyz"], cov6, MAP_VOXEL)
    assert len(np.unique(ref.count)) > 10 and ref.count.sum() == len(pc)
    with P.registration.VoxelCovarianceMap(pc, MAP_VOXEL) as dev:
        _assert_map_equals(dev, ref)
        back = dev.to_point_cloud()
        assert vr.bits_equal(back._xyz.cpu().numpy(), ref.mean) and vr.bits_equal(back._cov.cpu().numpy(), ref.cov6)


def test_map_sums_the_six_channels_in_member_order(P):
    """channels whose float64 sums depend on the order of the members (voxel_reference.order_sensitive_attribute, under its condition)"""
    c = vr.case("n4097")
    lo, hi = c.attrs[0], vr.order_sensitive_attribute(c.label, 977)
    for a in (lo, hi):
        vr.assert_condition(vr.order_sensitivity(a, c.label))
    cov6 = np.concatenate([lo, hi], 1)
    ref = vg.build_map(c.xyz, cov6, 1.0)
    assert np.array_equal(ref.cell_of_point, np.argsort(np.argsort(vr.morton3(vr.voxel_reference(c.xyz, 1.0).cells)))[c.label])
    pc = P.PointCloud(c.xyz)
    pc.covariances = cov6
    assert vr.bits_equal(pc._cov.cpu().numpy(), cov6)
    with P.registration.VoxelCovarianceMap(pc, 1.0) as dev:
        _assert_map_equals(dev, ref)


def test_map_from_normals_is_the_map_from_their_covariances(P, clouds, dev_map, ref_map):
    _assert_map_equals(dev_map, ref_map)
    pc = P.PointCloud(clouds["target_xyz"])
    pc.covariances = vg.cov33_of(clouds["target_cov6"])                 # the (n, 3, 3) form of the setter
    with P.registration.VoxelCovarianceMap(pc, MAP_VOXEL) as dev:
        _assert_map_equals(dev, ref_map)


def test_map_refuses_what_the_voxel_stage_refuses(P, clouds):
    pc = P.PointCloud(np.array([[0, 0, 0], [3e6, 0, 0]], np.float32))
    pc.normals = np.array([[0, 0, 1], [0, 0, 1]], np.float32)
    with pytest.raises(RuntimeError, match="voxel_size is too small"):
        P.registration.VoxelCovarianceMap(pc, 1.0)
    bad = P.PointCloud(np.array([[0, 0, 0], [1, np.nan, 0]], np.float32))
    bad.normals = np.array([[0, 0, 1], [0, 0, 1]], np.float32)
    with pytest.raises(RuntimeError, match="xyz holds a non-finite"):
        P.registration.VoxelCovarianceMap(bad, 1.0)
    bad = P.PointCloud(np.array([[0, 0, 0], [1, 0, 0]], np.float32))
    bad.normals = np.array([[0, 0, 1], [0, np.inf, 1]], np.float32)
    with pytest.raises(RuntimeError, match="normals holds a non-finite"):
        P.registration.VoxelCovarianceMap(bad, 1.0)


# ------------------------------------------------------------------------------------------ the rows, exactly
def _poses(small_pair):
    a = np.deg2rad(2.0)
    shift = np.eye(4)
    shift[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
    shift[:3, 3] = [-10.0, -12.0, 0.1]               # an eighth of the source leaves the grid on its low side (negative indices), most of the rest the occupied cells
    return {"identity": np.eye(4), "T_fgr": small_pair["T_fgr"], "shifted": shift @ small_pair["T_fgr"]}


@pytest.mark.parametrize("min_points", [1, 3])
@pytest.mark.parametrize("nbh", [1, 7, 27])
def test_rows_equal_the_reference(P, small_pair, clouds, dev_map, ref_map, nbh, min_points):
    for name, T in _poses(small_pair).items():
        ref = vg.rows_at(ref_map, clouds["source_xyz"], T, nbh, min_points)
        got = dev_map.correspondences(clouds["source"], T, nbh, min_points).cpu().numpy()
        assert len(ref) > 100, (name, len(ref))
        assert got.dtype == np.int32 and np.array_equal(got, ref), (name, nbh, min_points, len(got), len(ref))
    T = _poses(small_pair)["shifted"]
    idx = np.floor((vg.transform(clouds["source_xyz"], T) - ref_map.origin) / MAP_VOXEL)
    assert 0.05 < (idx < 0).any(1).mean() < 0.5                       # the shifted pose: negative indices for part of the source


def _tiny(P):
    """a 5 x 4 x 3 lattice of 60 points with spacing 0.25 on a grid of voxel 1e-6: the indices reach 1.0e6 of the 2^21 = 2.1e6 there are, so a
    source point 2 m above the lattice has an index past 2^21 and one below it a negative index"""
    rng = np.random.default_rng(3)
    g = np.stack(np.meshgrid(np.arange(5), np.arange(4), np.arange(3), indexing="ij"), -1).reshape(-1, 3)
    tgt = (0.25 * g + rng.uniform(-1e-7, 1e-7, g.shape)).astype(np.float32)
    nrm = rng.normal(size=tgt.shape).astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    pc = P.PointCloud(tgt)
    pc.normals = nrm
    src = np.concatenate([tgt[::2], tgt[1::7] + np.float32(2.5), tgt[::9] - np.float32(1.0), tgt[:3] + np.array([3.0, -1.0, 0.0], np.float32),
                          np.array([[1e30, 0, 0], [-1e30, 1e30, 0]], np.float32)]).astype(np.float32)
    return pc, tgt, vg.cov6_from_normals(nrm), src


@pytest.mark.parametrize("nbh", [1, 7, 27])
def test_rows_outside_the_grid_on_both_sides(P, nbh):
    pc, tgt, cov6, src = _tiny(P)
    voxel = 1e-6
    ref_map = vg.build_map(tgt, cov6, voxel)
    q = vg.transform(src, np.eye(4))
    idx = np.floor((q - ref_map.origin) / voxel)
    assert (idx < 0).any() and (idx >= vg.LIMIT).any() and ref_map.cells.max() >= 1000000
    with P.registration.VoxelCovarianceMap(pc, voxel) as dev:
        _assert_map_equals(dev, ref_map)
        ref = vg.rows_at(ref_map, src, np.eye(4), nbh)
        got = dev.correspondences(P.PointCloud(src), np.eye(4), nbh).cpu().numpy()
        assert np.array_equal(got, ref) and len(ref) == len(tgt[::2])


@pytest.mark.parametrize("nbh", [1, 7, 27])
def test_rows_on_a_one_cell_map(P, nbh):
    rng = np.random.default_rng(4)
    tgt = rng.uniform(0.1, 0.9, (37, 3)).astype(np.float32)
    pc = P.PointCloud(tgt)
    pc.covariances = np.tile(np.array([1, 0, 0, 1, 0, 1], np.float32), (37, 1))
    ref_map = vg.build_map(tgt, pc._cov.cpu().numpy(), 4.0)
    assert len(ref_map.cells) == 1 and ref_map.count[0] == 37
    src = rng.uniform(-3.0, 4.5, (90, 3)).astype(np.float32)          # cells -1, 0 and 1 per axis; about one point in seven falls into the cell itself
    with P.registration.VoxelCovarianceMap(pc, 4.0) as dev:
        _assert_map_equals(dev, ref_map)
        for min_points in (1, 37, 38):
            ref = vg.rows_at(ref_map, src, np.eye(4), nbh, min_points)
            got = dev.correspondences(P.PointCloud(src), np.eye(4), nbh, min_points).cpu().numpy()
            assert np.array_equal(got, ref), (nbh, min_points)
            assert (len(ref) > 0) == (min_points <= 37)


# ------------------------------------------------------------------------------------------ the trajectories
def _estimation(P, loss, k=1.0):
    R = P.registration
    return R.TransformationEstimationForGeneralizedICP({"l2": R.L2Loss(), "l1": R.L1Loss(), "gm": R.GMLoss(k)}[loss])


@pytest.fixture(scope="module")
def reference_loop(small_pair, clouds, ref_map):
    @functools.lru_cache(maxsize=None)
    def run(loss, nbh, max_it=40):
        return vg.loop(ref_map, clouds["source_xyz"], clouds["source_cov6"], small_pair["T_fgr"], nbh, 1, LOSS[loss], 1.0, max_it=max_it)
    return run


@pytest.mark.parametrize("nbh", [1, 7])
@pytest.mark.parametrize("loss", ["l2", "gm"])
def test_trajectory_matches_reference(P, small_pair, clouds, dev_map, ref_map, reference_loop, loss, nbh):
    full = reference_loop(loss, nbh)
    assert full.converged and 1 < full.iterations < 40, full
    for max_it in (1, 5, 40):
        ref = full.after(max_it)
        crit = P.registration.ICPConvergenceCriteria(1e-6, 1e-6, max_it)
        res = P.registration.registration_voxelized_gicp(clouds["source"], dev_map, None, small_pair["T_fgr"], _estimation(P, loss), crit, nbh, 1)
        ang, dt = pose_error(res.transformation, ref.transformation)
        print(f"{loss} nbh {nbh} max_it {max_it}: {ang:.2e} rad {dt:.2e} m, iterations {res.iterations} / {ref.iterations}, rows {len(res.correspondence_set)} / {ref.n_rows}, "
              f"fitness {res.fitness - ref.fitness:+.1e} rmse {res.inlier_rmse - ref.inlier_rmse:+.1e}")
        assert ang < 1e-7 and dt < 1e-6, (loss, nbh, max_it, ang, dt)
        assert res.iterations == ref.iterations and res.converged == ref.converged, (max_it, res.iterations, ref.iterations, res.converged, ref.converged)
        assert len(res.correspondence_set) == ref.n_rows
        assert abs(res.fitness - ref.fitness) < 1e-12 and abs(res.inlier_rmse - ref.inlier_rmse) < 1e-9
        # the correspondence set is the rule's rows at the returned pose
        assert np.array_equal(res.correspondence_set, vg.rows_at(ref_map, clouds["source_xyz"], res.transformation, nbh, 1))


@pytest.mark.parametrize("max_it", [1, 5])
@pytest.mark.parametrize("nbh", [1, 7])
def test_l1_trajectory_within_the_reference_spread(P, oracle, small_pair, clouds, dev_map, ref_map, nbh, max_it):
    """L1's 1 / |r| weights make the pose chaotic in the last bits of the sums: the bound is the spread of the reference itself under
    regrouped float64 sums (oracle.l1_spread through conftest.l1_tolerance, as tests/test_gpu_gicp.py bounds its L1 runs): the larger of the
    north-star tolerance (1e-4 rad, 1e-3 m) and three times that spread.

    Why the device holds it.  On the reference alone (CPU, numpy): a change of the summation chunking moves the pose by 1e-16 m after one
    iteration and 100 to 1000 times more after every further one (neighbourhood 7: 2e-14, 2e-12, 2e-9, 2e-6 ... 1e-5 m after 2, 3, 4, 5); changing
    every covariance entry by one unit in its last place -- the size of a per-row rounding, which regrouped SUMS do not sample -- moves it by
    3.4e-4 m (neighbourhood 1) and 3.7e-3 m (neighbourhood 7) after 5 iterations (1e-16 m under L2 and GM).  A kernel whose rows are right to
    1e-16 but rounded differently from the oracle's (fused multiply-adds, six fixed Jacobi sweeps, symmetrised R C R^T: the first form of
    k_icp_iter_vgicp) sat 4.8e-5 m and 1.8e-3 m from the reference after 5 iterations: outside this bound for neighbourhood 7.  So the kernel
    forms a row's W, J and r in the oracle's operation order without contraction, voxelized_gicp_reference.rotate_covariances states R C R^T in
    that order too, and what is left between device and reference is the order of the sums: measured on an MI355X 8e-17 / 6e-17 m after one
    iteration and 1.1e-7 / 6.0e-6 m after five (neighbourhood 1 / 7), the size of the spread itself (1.0e-7 / 5.9e-6 m)."""
    run = lambda: vg.loop(ref_map, clouds["source_xyz"], clouds["source_cov6"], small_pair["T_fgr"], nbh, 1, LOSS["l1"], 1.0, max_it=max_it)      # noqa: E731
    ref, tol_rad, tol_m, spread = l1_tolerance(oracle, run, chunks=(64, 512, 4096))
    res = P.registration.registration_voxelized_gicp(clouds["source"], dev_map, None, small_pair["T_fgr"], _estimation(P, "l1"),
                                                     P.registration.ICPConvergenceCriteria(1e-6, 1e-6, max_it), nbh, 1)
    ang, dt = pose_error(res.transformation, ref.transformation)
    print(f"l1 nbh {nbh}: {ang:.2e} rad {dt:.2e} m (tolerance {tol_rad:.1e} / {tol_m:.1e}, spread {spread[0]:.1e} / {spread[1]:.1e})")
    assert ang <= tol_rad and dt <= tol_m, (ang, dt, spread)
    assert res.iterations == ref.iterations == max_it and not res.converged and not ref.converged


def test_result_is_closer_to_the_shipped_gicp_pose_than_the_start(P, small_pair, clouds, dev_map):
    a0, d0 = pose_error(small_pair["T_fgr"], small_pair["T_gicp"])
    for nbh in (1, 7):
        res = P.registration.registration_voxelized_gicp(clouds["source"], dev_map, init=small_pair["T_fgr"], neighborhood=nbh)
        a, d = pose_error(res.transformation, small_pair["T_gicp"])
        print(f"nbh {nbh}: {np.degrees(a):.3f} deg {d:.3f} m from T_gicp after {res.iterations} iterations (start {np.degrees(a0):.3f} deg {d0:.3f} m)")
        assert res.converged and a < a0 and d < d0, (nbh, a, d, a0, d0)


# ------------------------------------------------------------------------------------------ the edges
def test_source_wholly_outside_the_map(P, clouds, dev_map):
    far = P.PointCloud(clouds["source_xyz"] + np.float32(5000.0))
    far.normals = clouds["source"]._nrm
    init = np.eye(4)
    init[:3, 3] = [0.5, -0.25, 0.125]
    for nbh in (1, 27):
        res = P.registration.registration_voxelized_gicp(far, dev_map, init=init, neighborhood=nbh)
        assert np.array_equal(res.transformation, init) and res.fitness == 0 and res.inlier_rmse == 0
        assert res.converged and res.iterations == 1 and len(res.correspondence_set) == 0


def test_one_source_point(P, clouds, dev_map, ref_map, small_pair):
    i = int(np.nonzero(vg.candidate_rows(ref_map, clouds["source_xyz"], small_pair["T_fgr"], 1)[:, 0] >= 0)[0][0])
    one = clouds["source"].select_by_index([i])
    crit = P.registration.ICPConvergenceCriteria(1e-6, 1e-6, 2)
    res = P.registration.registration_voxelized_gicp(one, dev_map, None, small_pair["T_fgr"], criteria=crit, neighborhood=7)
    # (three rows per map row do not determine six unknowns: what the update is then is the solver's business; the rows and the bookkeeping are the rule's)
    assert 1 <= res.iterations <= 2 and np.isfinite(res.transformation).all()
    rows = vg.rows_at(ref_map, clouds["source_xyz"][i:i + 1], res.transformation, 7, 1)
    assert np.array_equal(res.correspondence_set, rows) and res.fitness == (1.0 if len(rows) else 0.0)
    empty = P.registration.registration_voxelized_gicp(P.PointCloud(np.zeros((0, 3))), dev_map, init=small_pair["T_fgr"])
    assert empty.fitness == 0 and np.array_equal(empty.transformation, small_pair["T_fgr"]) and empty.converged and empty.iterations == 1


def _key(res):
    return (res.transformation.tobytes(), res.fitness, res.inlier_rmse, res.iterations, res.converged, res.correspondence_set.tobytes())


def test_one_map_serves_many_calls(P, small_pair, clouds, dev_map):
    """a map reused for two sources gives what two fresh maps give, bit for bit, and the same on a second run"""
    R = P.registration
    second = clouds["source"].select_by_index(np.arange(0, len(clouds["source"]), 2))
    crit = R.ICPConvergenceCriteria(1e-6, 1e-6, 10)
    runs = []
    for _ in range(2):
        runs.append([_key(R.registration_voxelized_gicp(s, dev_map, None, small_pair["T_fgr"], criteria=crit, neighborhood=7)) for s in (clouds["source"], second)])
    fresh = [_key(R.registration_voxelized_gicp(s, clouds["target"], MAP_VOXEL, small_pair["T_fgr"], criteria=crit, neighborhood=7)) for s in (clouds["source"], second)]
    assert runs[0] == runs[1] == fresh
    assert runs[0][0] != runs[0][1]


def test_use_after_close_raises(P, clouds):
    m = P.registration.VoxelCovarianceMap(clouds["target"], MAP_VOXEL)
    assert len(m) > 1000
    m.close()
    m.close()
    for call in (lambda: len(m), lambda: m.cells, lambda: m.counts, lambda: m.points, lambda: m.covariances, m.to_point_cloud,
                 lambda: m.correspondences(clouds["source"], np.eye(4)), lambda: P.registration.registration_voxelized_gicp(clouds["source"], m)):
        with pytest.raises(RuntimeError, match="closed"):
            call()


def test_call_without_a_correspondence_buffer_gives_the_same_pose(P, small_pair, clouds, dev_map):
    L = P._lib
    ctx = L.Context.current()
    src = clouds["source"]
    T0 = np.ascontiguousarray(small_pair["T_fgr"], np.float64)
    poses = []
    for want in (False, True):
        import torch
        corr = torch.empty((len(src) * 7, 2), dtype=torch.int32, device="cuda") if want else None
        res = L.PcrResult()
        p = L.PcrVgicpParams(0, 1.0, 1e-3, 1e-6, 1e-6, 30, 7, 1)
        ctx.check(ctx.lib.pcr_registration_voxelized_gicp(ctx.handle, src._xyz.data_ptr(), None, src._nrm.data_ptr(), len(src), dev_map._open(),
                                                          T0.ctypes.data_as(C.POINTER(C.c_double)), C.byref(p), C.byref(res), corr.data_ptr() if want else None), "vgicp")
        poses.append((bytes(res.transformation), res.fitness, res.inlier_rmse, res.n_correspondences, res.iterations))
    assert poses[0] == poses[1]


def test_abi_refusals_name_the_argument(P, clouds, dev_map):
    L = P._lib
    ctx = L.Context.current()
    src = clouds["source"]
    T0 = np.eye(4)

    def call(p, cov=None, nrm=src._nrm.data_ptr(), T=T0):
        res = L.PcrResult()
        return ctx.lib.pcr_registration_voxelized_gicp(ctx.handle, src._xyz.data_ptr(), cov, nrm, len(src), dev_map._open(), T.ctypes.data_as(C.POINTER(C.c_double)),
                                                       C.byref(p), C.byref(res), None)
    good = (0, 1.0, 1e-3, 1e-6, 1e-6, 30, 1, 1)
    for p, kw, word in ((L.PcrVgicpParams(*good[:6], 5, 1), {}, "neighborhood"), (L.PcrVgicpParams(*good[:6], 1, 0), {}, "min_points_per_voxel"),
                        (L.PcrVgicpParams(*good), dict(nrm=None), "src_cov6"), (L.PcrVgicpParams(*good), dict(T=np.full((4, 4), np.nan)), "init_T")):
        assert call(p, **kw) == L.PCR_EINVAL
        assert word in ctx.lib.pcr_last_error(ctx.handle).decode(), word
