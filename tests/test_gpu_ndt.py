"""NDT registration on the device against the numpy restatement of its rule (tests/ndt_reference.py): the map bit for bit (the information
matrices to 1e-10 of their norm), the rows exactly, the linearisation to the project's multiway bound, the trajectories of the loop, and the
edges.  Pair 899 with both clouds at voxel 0.3 against a 2.0 m map with min_points_per_voxel 6 (733 cells, 456 valid: the condition of these
comparisons is checked on the CPU in tests/test_ndt_api.py), and hand-made clouds of tens of points."""
import ctypes as C
import functools

import numpy as np
import pytest

import ndt_reference as nd
import voxel_reference as vr
import voxelized_gicp_reference as vg
from conftest import pkg, pose_error

pytestmark = pytest.mark.gpu

MAP_VOXEL = 2.0
MIN_POINTS = 6
LIN_BS = 512          # source points per workgroup of k_icp_iter_ndt / k_ndt_lin (pcr_icp_loop.h)


@pytest.fixture(scope="module")
def P():
    return pkg()


@pytest.fixture(scope="module")
def clouds(P, small_pair):
    """pair 899 at voxel 0.3 (6897 / 7074 points), nothing per point; the float32 arrays the device holds are what the reference gets"""
    out = {}
    for key in ("source", "target"):
        pc = P.PointCloud(small_pair[key]).voxel_down_sample(0.3)
        out[key] = pc
        out[key + "_xyz"] = pc._xyz.cpu().numpy()
    assert (len(out["source"]), len(out["target"])) == (6897, 7074)
    return out


@pytest.fixture(scope="module")
def ref_map(clouds):
    return nd.build_map(clouds["target_xyz"], MAP_VOXEL, MIN_POINTS)


@pytest.fixture(scope="module")
def dev_map(P, clouds):
    m = P.registration.NormalDistributionsMap(clouds["target"], MAP_VOXEL, MIN_POINTS)
    yield m
    m.close()


def _assert_map_equals(dev, ref):
    assert len(dev) == len(ref.cells)
    assert np.array_equal(dev.cells, ref.cells)                       # the same cells in the same (Morton) order
    assert np.array_equal(dev.counts, ref.count)
    assert vr.bits_equal(dev.points, ref.mean)
    assert vr.bits_equal(dev.covariances, ref.cov6)
    valid = dev.valid
    assert valid.dtype == bool and np.array_equal(valid, ref.valid)
    got = vg.cov33_of(dev.information)
    err = np.linalg.norm((got - ref.info).reshape(-1, 9), axis=1)
    norm = np.linalg.norm(ref.info.reshape(-1, 9), axis=1)
    worst = float((err / np.maximum(norm, 1e-300)).max()) if len(err) else 0.0
    print(f"information: worst |dA| / |A|_F = {worst:.2e} over {int(ref.valid.sum())} valid cells of {len(ref.cells)}")
    assert (err <= 1e-10 * norm).all(), worst
    assert (got[~ref.valid] == 0).all()
    assert np.array_equal(dev.origin, ref.origin) and dev.voxel_size == ref.voxel


# ------------------------------------------------------------------------------------------ the map
def test_map_equals_the_reference(P, dev_map, ref_map):
    assert (len(ref_map.cells), int(ref_map.valid.sum())) == (733, 456)
    _assert_map_equals(dev_map, ref_map)
    back = dev_map.to_point_cloud()
    assert vr.bits_equal(back._xyz.cpu().numpy(), ref_map.mean) and vr.bits_equal(back._cov.cpu().numpy(), ref_map.cov6)


def test_map_with_other_thresholds(P, clouds):
    """min_points_per_voxel 2 and eigenvalue_ratio 1 (every eigenvalue raised to the largest: A_v = I / lambda_max) and 0.3"""
    for min_points, ratio in ((2, 1.0), (9, 0.3)):
        ref = nd.build_map(clouds["target_xyz"], MAP_VOXEL, min_points, ratio)
        with P.registration.NormalDistributionsMap(clouds["target"], MAP_VOXEL, min_points, ratio) as dev:
            _assert_map_equals(dev, ref)


def _cell_cloud(kind, n, rng, base=(0.0, 0.0, 0.0)):
    """n points inside the unit cell around `base` (cells of voxel 1.0 on a grid whose origin the anchor point below fixes at -0.5)"""
    b = np.asarray(base, np.float64)
    if kind == "identical":
        p = np.tile(b + [0.25, 0.125, 0.375], (n, 1))
    elif kind == "collinear":
        p = b + [-0.3, -0.2, -0.1] + np.linspace(0.0, 0.5, n)[:, None] * np.array([1.0, 0.5, 0.25])
    else:
        p = b + rng.uniform(-0.4, 0.4, (n, 3))
    return p


def _degenerate(kind, rng):
    anchor = np.zeros((1, 3))          # a lone point at the grid's minimum (every other cell lies above it on every axis): origin = -0.5, its cell is invalid by its count
    if kind == "identical":
        return np.concatenate([anchor, _cell_cloud("identical", 8, rng, (2, 1, 1))]), [False, False], None
    if kind == "collinear":
        return np.concatenate([anchor, _cell_cloud("collinear", 8, rng, (2, 1, 1))]), [False, True], 2
    if kind == "threshold":           # N = min_points_per_voxel - 1 and N = min_points_per_voxel
        return np.concatenate([anchor, _cell_cloud("random", MIN_POINTS - 1, rng, (2, 1, 1)), _cell_cloud("random", MIN_POINTS, rng, (1, 3, 2))]), [False, False, True], None
    raise KeyError(kind)


@pytest.mark.parametrize("kind", ["identical", "collinear", "threshold"])
def test_degenerate_cells(P, kind):
    xyz, want_valid, want_clamped = _degenerate(kind, np.random.default_rng(11))
    xyz = xyz.astype(np.float32)
    ref = nd.build_map(xyz, 1.0, MIN_POINTS)
    order = np.argsort(ref.count, kind="stable") if kind == "threshold" else np.arange(len(ref.cells))
    assert ref.valid[order].tolist() == want_valid, (ref.count, ref.valid)
    if want_clamped is not None:
        assert ref.clamped[ref.valid].tolist() == [want_clamped]
    with P.registration.NormalDistributionsMap(P.PointCloud(xyz), 1.0, MIN_POINTS) as dev:
        _assert_map_equals(dev, ref)
        src = P.PointCloud(xyz)
        for nbh in (1, 7, 27):
            got = dev.correspondences(src, np.eye(4), nbh).cpu().numpy()
            assert np.array_equal(got, nd.rows_at(ref, xyz, np.eye(4), nbh))
        if not ref.valid.any():       # a map with no valid cell: no rows, the pose stays, and that is no error
            init = np.eye(4)
            init[:3, 3] = [0.5, -0.25, 0.125]
            res = P.registration.registration_ndt(src, dev, init=init)
            assert np.array_equal(res.transformation, init) and res.fitness == 0 and res.inlier_rmse == 0 and len(res.correspondence_set) == 0
            assert res.converged and res.iterations == 1
            lin = dev.linearize(src, init)
            assert lin.rows == 0 and lin.points_with_rows == 0 and lin.score == 0 and not lin.JTJ.any() and not lin.JTr.any()


@pytest.mark.parametrize("nbh", [1, 7, 27])
def test_one_cell_map(P, nbh):
    rng = np.random.default_rng(4)
    tgt = rng.uniform(0.1, 0.9, (37, 3)).astype(np.float32)
    ref = nd.build_map(tgt, 4.0, MIN_POINTS)
    assert len(ref.cells) == 1 and ref.count[0] == 37 and ref.valid[0]
    src = rng.uniform(-3.0, 4.5, (90, 3)).astype(np.float32)          # cells -1, 0 and 1 per axis; about one point in seven falls into the cell itself
    with P.registration.NormalDistributionsMap(P.PointCloud(tgt), 4.0, MIN_POINTS) as dev:
        _assert_map_equals(dev, ref)
        rows = nd.rows_at(ref, src, np.eye(4), nbh)
        assert len(rows) > 0
        assert np.array_equal(dev.correspondences(P.PointCloud(src), np.eye(4), nbh).cpu().numpy(), rows)
        _assert_linearization(dev.linearize(P.PointCloud(src), np.eye(4), nbh), nd.linearize(ref, src, np.eye(4), rows))
    with P.registration.NormalDistributionsMap(P.PointCloud(tgt), 4.0, 38) as dev:
        assert not dev.valid.any() and len(dev.correspondences(P.PointCloud(src), np.eye(4), nbh)) == 0


# ------------------------------------------------------------------------------------------ the rows, exactly
def _poses(small_pair, ref_map):
    """T_fgr, T_gicp, and T_fgr turned by 2 degrees and pushed 10 m down the x axis and 12 m up the y axis: part of the source leaves the grid
    on its low side in x (negative indices), another part lies past the last occupied cell in y"""
    a = np.deg2rad(2.0)
    shift = np.eye(4)
    shift[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
    shift[:3, 3] = [-10.0, 12.0, 0.1]
    return {"T_fgr": small_pair["T_fgr"], "T_gicp": small_pair["T_gicp"], "shifted": shift @ small_pair["T_fgr"]}


@pytest.mark.parametrize("nbh", [1, 7, 27])
def test_rows_equal_the_reference(P, small_pair, clouds, dev_map, ref_map, nbh):
    poses = _poses(small_pair, ref_map)
    for name, T in poses.items():
        ref = nd.rows_at(ref_map, clouds["source_xyz"], T, nbh)
        got = dev_map.correspondences(clouds["source"], T, nbh).cpu().numpy()
        assert len(ref) > 100, (name, len(ref))
        assert got.dtype == np.int32 and np.array_equal(got, ref), (name, nbh, len(got), len(ref))
    idx = np.floor((vg.transform(clouds["source_xyz"], poses["shifted"]) - ref_map.origin) / MAP_VOXEL)
    low, high = (idx < 0).any(1).mean(), (idx > ref_map.cells.max(0)).any(1).mean()
    assert low > 0.01 and high > 0.01, (low, high)                     # the shifted pose: part of the source outside on both sides
    # rows that land in an occupied but invalid cell are dropped: the condition is that there are such candidates
    cand = vg.candidate_rows(ref_map.base, clouds["source_xyz"], small_pair["T_fgr"], nbh, 1)
    assert ((cand >= 0) & ~ref_map.valid[np.maximum(cand, 0)]).sum() > 50
    far = P.PointCloud(clouds["source_xyz"] + np.float32(5000.0))
    assert len(dev_map.correspondences(far, small_pair["T_fgr"], nbh)) == 0


@pytest.mark.parametrize("nbh", [1, 7, 27])
def test_rows_outside_the_grid_on_both_sides(P, nbh):
    """a 5 x 4 x 3 lattice of cells 0.25 apart on a grid of voxel 1e-6, seven members each: the indices reach 1.0e6 of the 2^21 = 2.1e6 there
    are, so a source point 2.5 m above the lattice has an index past 2^21 and one below it a negative index"""
    rng = np.random.default_rng(3)
    g = np.stack(np.meshgrid(np.arange(5), np.arange(4), np.arange(3), indexing="ij"), -1).reshape(-1, 3)
    nodes = np.repeat(0.25 * g, 7, axis=0)
    tgt = (nodes + rng.integers(-2, 3, nodes.shape) * 2.0 ** -24).astype(np.float32)        # members a few float32 steps apart
    voxel = 1e-6
    ref = nd.build_map(tgt, voxel, MIN_POINTS)
    assert len(ref.cells) == 60 and (ref.count == 7).all() and ref.valid.sum() > 40 and ref.cells.max() >= 1000000
    src = np.concatenate([tgt[::2], tgt[1::7] + np.float32(2.5), tgt[::9] - np.float32(1.0), tgt[:3] + np.array([3.0, -1.0, 0.0], np.float32),
                          np.array([[1e30, 0, 0], [-1e30, 1e30, 0]], np.float32)]).astype(np.float32)
    idx = np.floor((vg.transform(src, np.eye(4)) - ref.origin) / voxel)
    assert (idx < 0).any() and (idx >= vg.LIMIT).any()
    with P.registration.NormalDistributionsMap(P.PointCloud(tgt), voxel, MIN_POINTS) as dev:
        _assert_map_equals(dev, ref)
        rows = nd.rows_at(ref, src, np.eye(4), nbh)
        got = dev.correspondences(P.PointCloud(src), np.eye(4), nbh).cpu().numpy()
        assert np.array_equal(got, rows) and len(rows) == int(ref.valid[ref.cell_of_point[::2]].sum())


# ------------------------------------------------------------------------------------------ the linearisation
def _assert_linearization(got, ref, what=""):
    """rows and points exactly; every sum within 1e-9 x the sum of the magnitudes of its terms (the bound of tests/test_gpu_multiway.py)"""
    assert (got.rows, got.points_with_rows) == (ref.rows, ref.points_with_rows), what
    worst = 0.0
    for name, g, r in (("JTJ", got.JTJ, ref.JTJ), ("JTr", got.JTr, ref.JTr), ("score", got.score, ref.score), ("sum_d2", got.sum_d2, ref.sum_d2)):
        err, mag = np.abs(np.asarray(g) - np.asarray(r)), np.asarray(ref.mag[name])
        worst = max(worst, float((err / np.maximum(mag, 1e-300)).max()))
        assert (err <= 1e-9 * mag).all(), (what, name, err, mag)
    assert np.array_equal(got.JTJ, got.JTJ.T)
    print(f"linearize {what}: rows {got.rows}, score {got.score:.6f}, worst error / sum of magnitudes {worst:.2e}")


def _lin_key(lin):
    return (lin.JTJ.tobytes(), lin.JTr.tobytes(), lin.score, lin.rows, lin.points_with_rows, lin.sum_d2)


@pytest.mark.parametrize("nbh", [1, 7, 27])
def test_linearize_at_T_fgr(P, small_pair, clouds, dev_map, ref_map, nbh):
    import torch
    T = small_pair["T_fgr"]
    ref = nd.linearize(ref_map, clouds["source_xyz"], T, nd.rows_at(ref_map, clouds["source_xyz"], T, nbh))
    got = dev_map.linearize(clouds["source"], T, nbh)
    _assert_linearization(got, ref, f"nbh {nbh}")
    assert ref.rows > 3000 and ref.score > 0
    assert _lin_key(dev_map.linearize(clouds["source"], T, nbh)) == _lin_key(got)            # two runs: the same bits
    # ... and the same bits wherever the source sits in a larger buffer
    n = len(clouds["source"])
    for lead in (1, 5):
        buf = torch.full((n + 8, 3), 1e30, dtype=torch.float32, device="cuda")
        buf[lead:lead + n] = clouds["source"]._xyz
        moved = P.PointCloud()
        moved._xyz = buf[lead:lead + n]
        assert moved._xyz.data_ptr() == buf.data_ptr() + 12 * lead
        assert _lin_key(dev_map.linearize(moved, T, nbh)) == _lin_key(got), lead
    # another outlier ratio changes the weights, not the rows
    other = dev_map.linearize(clouds["source"], T, nbh, 0.3)
    _assert_linearization(other, nd.linearize(ref_map, clouds["source_xyz"], T, nd.rows_at(ref_map, clouds["source_xyz"], T, nbh), 0.3), f"nbh {nbh} p 0.3")
    assert other.score != got.score


@pytest.mark.parametrize("n", [1, LIN_BS - 1, LIN_BS, LIN_BS + 1])
def test_sizes_around_the_workgroup(P, small_pair, clouds, dev_map, ref_map, n):
    """prefixes of the source (which is in Morton order: a prefix is a corner of the scene, with rows).  One source point leaves the 6x6 system
    of rank 3 (every row of a point has the same J), and what a solver makes of a singular system is its own business: there the rows and the
    bookkeeping are compared, from two points on the pose too."""
    T = small_pair["T_fgr"]
    first = int(np.nonzero(nd.candidate_rows(ref_map, clouds["source_xyz"], T, 7)[:, 0] >= 0)[0][0])
    xyz = clouds["source_xyz"][first:first + n]
    src = P.PointCloud(xyz)
    rows = nd.rows_at(ref_map, xyz, T, 7)
    assert len(rows) >= 1
    _assert_linearization(dev_map.linearize(src, T, 7), nd.linearize(ref_map, xyz, T, rows), f"n {n}")
    ref = nd.loop(ref_map, xyz, T, 7, max_it=1)
    res = P.registration.registration_ndt(src, dev_map, None, T, P.registration.ICPConvergenceCriteria(1e-6, 1e-6, 1), 7)
    assert res.iterations == ref.iterations == 1 and np.isfinite(res.transformation).all()
    assert np.array_equal(res.correspondence_set, nd.rows_at(ref_map, xyz, res.transformation, 7))
    if n > 1:
        ang, dt = pose_error(res.transformation, ref.transformation)
        print(f"n {n}: {ang:.2e} rad {dt:.2e} m, rows {len(res.correspondence_set)} / {ref.n_rows}")
        assert ang < 1e-7 and dt < 1e-6, (n, ang, dt)
        assert res.converged == ref.converged and len(res.correspondence_set) == ref.n_rows
        assert abs(res.fitness - ref.fitness) < 1e-12 and abs(res.inlier_rmse - ref.inlier_rmse) < 1e-9


# ------------------------------------------------------------------------------------------ the trajectories
@pytest.fixture(scope="module")
def reference_loop(small_pair, clouds, ref_map):
    @functools.lru_cache(maxsize=None)
    def run(nbh, max_it=40):
        return nd.loop(ref_map, clouds["source_xyz"], small_pair["T_fgr"], nbh, max_it=max_it)
    return run


@pytest.mark.parametrize("nbh", [1, 7])
def test_trajectory_matches_reference(P, small_pair, clouds, dev_map, ref_map, reference_loop, nbh):
    """The bound is that of the smooth-weight voxelized GICP runs; the loop's sensitivity (a 1e-12 relative change of every A_v moves the end
    pose by 1e-13 m) says the true difference is far below it.  Measured on an MI355X: 4e-18 to 3e-17 rad and 4e-17 to 8e-16 m over the six
    runs, iteration counts 17 and 14 as the restatement's."""
    full = reference_loop(nbh)
    assert full.converged and 1 < full.iterations < 40, full
    for max_it in (1, 5, 40):
        ref = full.after(max_it)
        crit = P.registration.ICPConvergenceCriteria(1e-6, 1e-6, max_it)
        res = P.registration.registration_ndt(clouds["source"], dev_map, None, small_pair["T_fgr"], crit, nbh)
        ang, dt = pose_error(res.transformation, ref.transformation)
        print(f"nbh {nbh} max_it {max_it}: {ang:.2e} rad {dt:.2e} m, iterations {res.iterations} / {ref.iterations}, rows {len(res.correspondence_set)} / {ref.n_rows}, "
              f"fitness {res.fitness - ref.fitness:+.1e} rmse {res.inlier_rmse - ref.inlier_rmse:+.1e}")
        assert ang < 1e-7 and dt < 1e-6, (nbh, max_it, ang, dt)
        assert res.iterations == ref.iterations and res.converged == ref.converged, (max_it, res.iterations, ref.iterations, res.converged, ref.converged)
        assert len(res.correspondence_set) == ref.n_rows
        assert abs(res.fitness - ref.fitness) < 1e-12 and abs(res.inlier_rmse - ref.inlier_rmse) < 1e-9
        # the correspondence set is the rule's rows at the returned pose
        assert np.array_equal(res.correspondence_set, nd.rows_at(ref_map, clouds["source_xyz"], res.transformation, nbh))


def test_result_is_closer_to_the_shipped_gicp_pose_than_the_start(P, small_pair, clouds, dev_map):
    a0, d0 = pose_error(small_pair["T_fgr"], small_pair["T_gicp"])
    for nbh in (1, 7):
        res = P.registration.registration_ndt(clouds["source"], dev_map, init=small_pair["T_fgr"], neighborhood=nbh)
        a, d = pose_error(res.transformation, small_pair["T_gicp"])
        print(f"nbh {nbh}: {np.degrees(a):.3f} deg {d:.3f} m from T_gicp after {res.iterations} iterations (start {np.degrees(a0):.3f} deg {d0:.3f} m)")
        assert res.converged and a < a0 and d < d0, (nbh, a, d, a0, d0)


# ------------------------------------------------------------------------------------------ the plumbing
def _key(res):
    return (res.transformation.tobytes(), res.fitness, res.inlier_rmse, res.iterations, res.converged, res.correspondence_set.tobytes())


def test_one_map_serves_many_calls(P, small_pair, clouds, dev_map):
    """a map reused for two sources gives what two fresh maps give, bit for bit, and the same on a second run"""
    R = P.registration
    second = clouds["source"].select_by_index(np.arange(0, len(clouds["source"]), 2))
    crit = R.ICPConvergenceCriteria(1e-6, 1e-6, 10)
    runs = []
    for _ in range(2):
        runs.append([_key(R.registration_ndt(s, dev_map, None, small_pair["T_fgr"], crit, 7)) for s in (clouds["source"], second)])
    fresh = [_key(R.registration_ndt(s, clouds["target"], MAP_VOXEL, small_pair["T_fgr"], crit, 7, 0.55, MIN_POINTS)) for s in (clouds["source"], second)]
    assert runs[0] == runs[1] == fresh
    assert runs[0][0] != runs[0][1]
    empty = R.registration_ndt(P.PointCloud(np.zeros((0, 3))), dev_map, init=small_pair["T_fgr"])
    assert empty.fitness == 0 and np.array_equal(empty.transformation, small_pair["T_fgr"]) and empty.converged and empty.iterations == 1


def test_use_after_close_raises(P, clouds):
    m = P.registration.NormalDistributionsMap(clouds["target"], MAP_VOXEL)
    assert len(m) == 733
    m.close()
    m.close()
    for call in (lambda: len(m), lambda: m.cells, lambda: m.counts, lambda: m.points, lambda: m.covariances, lambda: m.information, lambda: m.valid,
                 lambda: m.voxel_size, lambda: m.origin, m.to_point_cloud, lambda: m.correspondences(clouds["source"], np.eye(4)),
                 lambda: m.linearize(clouds["source"], np.eye(4)), lambda: P.registration.registration_ndt(clouds["source"], m)):
        with pytest.raises(RuntimeError, match="closed"):
            call()


def _raw_call(L, ctx, src, dev_map, T0, p, corr=None):
    res = L.PcrResult()
    rc = ctx.lib.pcr_registration_ndt(ctx.handle, src._xyz.data_ptr(), len(src), dev_map._open(), T0.ctypes.data_as(C.POINTER(C.c_double)), C.byref(p), C.byref(res),
                                      corr.data_ptr() if corr is not None else None)
    return rc, res


def test_call_without_a_correspondence_buffer_gives_the_same_pose(P, small_pair, clouds, dev_map):
    import torch
    L = P._lib
    ctx = L.Context.current()
    src = clouds["source"]
    T0 = np.ascontiguousarray(small_pair["T_fgr"], np.float64)
    poses = []
    for want in (False, True):
        corr = torch.empty((len(src) * 7, 2), dtype=torch.int32, device="cuda") if want else None
        rc, res = _raw_call(L, ctx, src, dev_map, T0, L.PcrNdtParams(1e-6, 1e-6, 30, 7, 0.55), corr)
        ctx.check(rc, "ndt")
        poses.append((bytes(res.transformation), res.fitness, res.inlier_rmse, res.n_correspondences, res.iterations))
    assert poses[0] == poses[1]


def test_abi_refusals_name_the_argument(P, clouds, dev_map):
    import torch
    L = P._lib
    ctx = L.Context.current()
    src = clouds["source"]
    T0 = np.eye(4)
    err = lambda: ctx.lib.pcr_last_error(ctx.handle).decode()      # noqa: E731
    good = (1e-6, 1e-6, 30, 7, 0.55)
    for p, T, word in ((L.PcrNdtParams(*good[:3], 5, 0.55), T0, "neighborhood"), (L.PcrNdtParams(*good[:4], 0.0), T0, "outlier_ratio"),
                       (L.PcrNdtParams(*good[:4], 1.0), T0, "outlier_ratio"), (L.PcrNdtParams(*good[:4], float("nan")), T0, "outlier_ratio"),
                       (L.PcrNdtParams(1e-6, 1e-6, -1, 7, 0.55), T0, "max_iteration"), (L.PcrNdtParams(*good), np.full((4, 4), np.nan), "init_T")):
        assert _raw_call(L, ctx, src, dev_map, T, p)[0] == L.PCR_EINVAL
        assert word in err(), word
    bad_src = P.PointCloud(np.array([[0, 0, 0], [1, np.inf, 0]], np.float32))
    assert _raw_call(L, ctx, bad_src, dev_map, T0, L.PcrNdtParams(*good))[0] == L.PCR_EINVAL and "src_xyz" in err()
    # the map's own refusals
    xyz = clouds["target"]._xyz
    h = C.c_void_p()
    create = lambda t, voxel, min_points, ratio: ctx.lib.pcr_ndt_map_create(ctx.handle, t.data_ptr(), len(t), voxel, min_points, ratio, C.byref(h))      # noqa: E731
    for args, word in (((xyz, 0.0, 6, 0.01), "voxel_size"), ((xyz, -1.0, 6, 0.01), "voxel_size"), ((xyz, 2.0, 1, 0.01), "min_points_per_voxel"),
                       ((xyz, 2.0, 6, 0.0), "eigenvalue_ratio"), ((xyz, 2.0, 6, 1.5), "eigenvalue_ratio"), ((xyz, 2.0, 6, float("nan")), "eigenvalue_ratio"),
                       ((xyz, 1e-6, 6, 0.01), "voxel_size is too small")):
        assert create(*args) == L.PCR_EINVAL and not h.value
        assert word in err(), word
    nan = torch.tensor([[0, 0, 0], [1, float("nan"), 0]], dtype=torch.float32, device="cuda")
    assert create(nan, 2.0, 6, 0.01) == L.PCR_EINVAL and "xyz holds a non-finite" in err()
    n = C.c_int64(0)
    rows = torch.empty((len(src) * 7, 2), dtype=torch.int32, device="cuda")
    assert ctx.lib.pcr_ndt_map_correspondences(ctx.handle, dev_map._open(), src._xyz.data_ptr(), len(src), T0.ctypes.data_as(C.POINTER(C.c_double)), 3, rows.data_ptr(),
                                               C.byref(n)) == L.PCR_EINVAL and "neighborhood" in err()
    assert ctx.lib.pcr_ndt_linearize(ctx.handle, dev_map._open(), src._xyz.data_ptr(), len(src), T0.ctypes.data_as(C.POINTER(C.c_double)), 7, 1.25, None, None, None, None, None,
                                     None) == L.PCR_EINVAL and "outlier_ratio" in err()
    if torch.cuda.device_count() > 1:          # a map on another device than the context
        with torch.cuda.device(1):
            other = P.registration.NormalDistributionsMap(P.PointCloud(clouds["target_xyz"]), MAP_VOXEL)
        try:
            assert _raw_call(L, ctx, src, other, T0, L.PcrNdtParams(*good))[0] == L.PCR_EINVAL and "another device" in err()
        finally:
            other.close()
