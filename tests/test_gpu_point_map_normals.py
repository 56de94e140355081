"""ESTIMATE on the device -- a VoxelPointMap that computes its normals from its own rows and keeps them current -- against the numpy restatement
(tests/point_map_normals_reference.py): the counts EQUAL (the same float64 arithmetic), every normal explained by its neighbourhood's covariance
(tests/normal_reference.py: no reference eigenvector), the normals as a function of the rows alone however the map was reached, all or nothing,
and point-to-plane ICP over the valid rows: one linearisation, the trajectories of the loop and scan-to-map odometry with scans without normals.
Pair 899 with both clouds at voxel 0.3 against a 1.0 m map with M = 20 and rho = 1.0, a crafted cloud of 128 clusters, and maps of tens of points."""
import ctypes as C
import functools

import numpy as np
import pytest

import normal_reference as nr
import point_map_normals_reference as pn
import point_map_reference as pm
import voxel_reference as vr
from conftest import pkg, pose_error

pytestmark = pytest.mark.gpu

MAP_VOXEL, RHO, K_MIN = 1.0, 1.0, 5
LOSS = {"l2": pm.L2, "l1": pm.L1, "gm": pm.GM}
GM_K = 0.5


@pytest.fixture(scope="module")
def P():
    return pkg()


def _cloud(P, xyz, nrm=None):
    pc = P.PointCloud(np.ascontiguousarray(xyz, np.float32))
    if nrm is not None:
        pc.normals = np.ascontiguousarray(nrm, np.float32)
    return pc


@pytest.fixture(scope="module")
def clouds(P, small_pair):
    """pair 899 at voxel 0.3 WITHOUT normals (6897 / 7074 points): the grid of tests/test_gpu_point_map.py"""
    out = {}
    for key in ("source", "target"):
        pc = P.PointCloud(small_pair[key]).voxel_down_sample(0.3)
        out[key] = pc
        out[key + "_xyz"] = pc._xyz.cpu().numpy()
    assert (len(out["source"]), len(out["target"])) == (6897, 7074)
    return out


@pytest.fixture(scope="module")
def ref_est(clouds):
    """the restatement of the estimated map of pair 899's target, computed once: (map without normals, Neighbours, counts, valid)"""
    ref = pm.build_map(clouds["target_xyz"], None, MAP_VOXEL, 20)
    nb, counts, valid = pn.estimate(ref, RHO, K_MIN)
    return ref, nb, counts, valid


@pytest.fixture(scope="module")
def est_map(P, clouds):
    m = P.registration.VoxelPointMap(clouds["target"], MAP_VOXEL, 20)
    m.estimate_normals(RHO, K_MIN)
    yield m
    m.close()


@pytest.fixture(scope="module")
def ref_map(est_map, ref_est):
    """the restatement's map with the DEVICE's normals (test_pair_899 holds every one of them explained) and the restatement's validity"""
    ref, _, _, valid = ref_est
    assert vr.bits_equal(est_map.points, ref.points)
    return pn.with_normals(ref, est_map.normals), valid


def _check_estimated(dev, ref, radius, k_min, valid_rows, what):
    """counts equal, every row explained, validity and the reported state; returns (Neighbours, counts)"""
    assert vr.bits_equal(dev.points, ref.points)
    nb, counts, valid = pn.estimate(ref, radius, k_min)
    got = dev.normal_counts
    assert got.dtype == np.int32 and np.array_equal(got, counts), (what, np.nonzero(got != counts)[0][:10])
    nr.assert_normals_explained(ref.points, dev.normals, nb, what=what)
    assert dev.normal_valid.dtype == bool and np.array_equal(dev.normal_valid, valid) and valid_rows == int(valid.sum())
    assert dev.has_normals and dev.normals_estimated and dev.normal_radius == radius and dev.normal_min_neighbors == k_min
    back = dev.to_point_cloud()
    assert vr.bits_equal(back._nrm.cpu().numpy(), dev.normals)
    return nb, counts


def _snapshot(m):
    est = m.normals_estimated
    return (m.cells.tobytes(), m.starts.tobytes(), m.counts.tobytes(), m.points.tobytes(), m.has_normals, m.normals.tobytes() if m.has_normals else None, est,
            m.normal_radius, m.normal_min_neighbors, m.normal_counts.tobytes() if est else None)


# ------------------------------------------------------------------------------------------ 1. the crafted cloud
@pytest.mark.parametrize("M", [20, 64])
def test_crafted_cloud(P, M):
    pts, _, names = nr.crafted_cloud()
    ref = pm.build_map(pts, None, 0.5, M)
    assert len(ref) == len(pts)                                          # a cluster has at most 20 points and no cell holds two clusters
    with P.registration.VoxelPointMap(_cloud(P, pts), 0.5, M) as dev:
        assert not dev.has_normals and not dev.normals_estimated and dev.normal_radius is None and dev.normal_min_neighbors is None
        valid_rows = dev.estimate_normals(0.5, 5)
        nb, counts = _check_estimated(dev, ref, 0.5, 5, valid_rows, f"crafted cloud, M = {M}")
        node = np.rint((ref.points.astype(np.float64) - nr.OFFSET) / 10.0).astype(np.int64)
        label = node[:, 0] + 8 * node[:, 1] + 32 * node[:, 2]
        size = np.bincount(label, minlength=128)
        assert np.array_equal(counts, size[label])                       # the neighbours of a row are its own cluster
        assert set(size.tolist()) >= {1, 2, 3, 20} and sum(n.startswith(("grid", "line", "coincident", "cut")) for n in names) > 40
        assert np.array_equal(dev.normal_valid, size[label] >= 5)


# ------------------------------------------------------------------------------------------ 2. the smallest shapes
@pytest.mark.parametrize("M", [1, 2, 64])
def test_forty_points(P, M):
    """rho = the voxel: neighbours come from the adjacent cells, not only from the row's own"""
    xyz = np.random.default_rng(40).uniform(0.0, 2.5, (40, 3)).astype(np.float32)
    ref = pm.build_map(xyz, None, 1.0, M)
    with P.registration.VoxelPointMap(_cloud(P, xyz), 1.0, M) as dev:
        valid_rows = dev.estimate_normals(None, 3)                       # (None: the voxel size)
        _, counts = _check_estimated(dev, ref, 1.0, 3, valid_rows, f"forty points, M = {M}")
        assert np.array_equal(counts, pn.brute_counts(ref.points, 1.0))
        own = np.array([int((ref.row_cell == c).all(1).sum()) for c in ref.row_cell])
        assert (counts > own).sum() > len(ref) // 2                      # most rows have neighbours outside their own cell


def test_first_and_last_cell_of_an_axis(P):
    """cells 0 and 2^21 - 1 are inside; the candidate cells -1 and 2^21 do not exist and are neither wrapped nor probed"""
    top = 2097151.0
    xyz = np.array([[-0.5, 0.0, 0.0], [-0.25, 0.25, 0.0], [0.25, 0.0, 0.25], [0.75, 0.25, 0.0], [0.0, 0.0, top], [0.25, 0.25, top - 0.75], [0.0, 0.5, top + 0.25],
                    [-0.5, 0.0, top], [0.0, -0.5, 1.0], [top, 0.0, 0.0], [top - 0.5, 0.25, 0.25], [top + 0.25, -0.25, 0.0]], np.float32)
    ref = pm.build_map(xyz, None, 1.0, 8, np.zeros(3))
    assert ref.cells.min() == 0 and ref.cells.max() == 2097151 and (ref.cells[:, 2] == 2097151).sum() >= 2 and (ref.cells[:, 0] == 2097151).sum() >= 1
    with P.registration.VoxelPointMap.on_grid(_cloud(P, xyz), 1.0, 8, np.zeros(3)) as dev:
        valid_rows = dev.estimate_normals(1.0, 3)
        _, counts = _check_estimated(dev, ref, 1.0, 3, valid_rows, "first and last cell")
        assert np.array_equal(counts, pn.brute_counts(ref.points, 1.0)) and counts.max() >= 3


def test_block_of_full_cells(P):
    """3 x 3 x 3 cells with 64 rows each: every candidate cell is occupied and full, the counts run into the hundreds"""
    rng = np.random.default_rng(27)
    cell = np.array([(x, y, z) for x in (1, 2, 3) for y in (1, 2, 3) for z in (1, 2, 3)], np.float64)
    xyz = (np.repeat(cell, 64, 0) + rng.uniform(-0.49, 0.49, (27 * 64, 3))).astype(np.float32)
    xyz = xyz[rng.permutation(len(xyz))]
    ref = pm.build_map(xyz, None, 1.0, 64, np.zeros(3))
    assert len(ref.cells) == 27 and (ref.counts == 64).all()
    with P.registration.VoxelPointMap.on_grid(_cloud(P, xyz), 1.0, 64, np.zeros(3)) as dev:
        valid_rows = dev.estimate_normals(1.0, 5)
        _, counts = _check_estimated(dev, ref, 1.0, 5, valid_rows, "27 full cells")
        assert counts.max() > 200 and counts.min() >= 5


# ------------------------------------------------------------------------------------------ 3. pair 899
def test_pair_899(est_map, ref_est):
    ref, nb, counts, valid = ref_est
    nr.assert_ambiguity_cap(nb, "pair 899, radius 1.0")
    assert valid.mean() >= 0.95, (int((~valid).sum()), len(valid))      # from the reference alone
    assert np.array_equal(est_map.normal_counts, counts)
    nr.assert_normals_explained(ref.points, est_map.normals, nb, what="pair 899, 1.0 m map, rho 1.0")
    assert np.array_equal(est_map.normal_valid, valid) and est_map.normals_estimated and est_map.has_normals
    print(f"pair 899: {len(ref)} rows, {int((~valid).sum())} invalid, largest count {int(counts.max())}")


# ------------------------------------------------------------------------------------------ 4. a function of the rows
def _pose(deg, t):
    a = np.deg2rad(deg)
    T = np.eye(4)
    T[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
    T[:3, 3] = t
    return T


def _same_estimate(a, b):
    assert vr.bits_equal(a.points, b.points) and np.array_equal(a.cells, b.cells) and np.array_equal(a.starts, b.starts)
    assert a.normals_estimated and b.normals_estimated
    assert vr.bits_equal(a.normals, b.normals) and np.array_equal(a.normal_counts, b.normal_counts)


def test_three_inserts_equal_one_map_of_all_points(P, clouds):
    M = P.registration.VoxelPointMap
    g = M.centered_grid_min(clouds["target_xyz"].mean(0), MAP_VOXEL)
    arrivals = [(clouds["target_xyz"], None), (clouds["source_xyz"], _pose(2.0, [0.3, -0.2, 0.0])), (clouds["target_xyz"][::3], _pose(-1.0, [-0.1, 0.4, 0.05])),
                (clouds["source_xyz"][::2], None)]
    placed = np.concatenate([pm.place(x, None, T)[0] for x, T in arrivals])
    with M.on_grid(_cloud(P, arrivals[0][0]), MAP_VOXEL, 6, g) as a, M.on_grid(_cloud(P, placed), MAP_VOXEL, 6, g) as b:
        first = a.estimate_normals(RHO, K_MIN)
        n0 = a.normals
        for x, T in arrivals[1:]:
            a.insert(_cloud(P, x), T)
        assert len(a) > len(n0) + 2000 and (a.counts == 6).sum() > 500
        valid_rows = b.estimate_normals(RHO, K_MIN)
        _same_estimate(a, b)
        assert valid_rows == int(a.normal_valid.sum()) > first
        # estimated again with other arguments: the new rule, the same rows
        again = a.estimate_normals(0.5, 8)
        assert (a.normal_radius, a.normal_min_neighbors) == (0.5, 8) and again < valid_rows and vr.bits_equal(a.points, b.points)
        b.estimate_normals(0.5, 8)
        _same_estimate(a, b)


def test_remove_far_equals_a_fresh_map_of_the_remaining_rows(P, clouds):
    M = P.registration.VoxelPointMap
    c = clouds["target_xyz"].astype(np.float64).mean(0)
    g = M.centered_grid_min(c, MAP_VOXEL)
    with M.on_grid(clouds["target"], MAP_VOXEL, 20, g) as a:
        a.estimate_normals(RHO, K_MIN)
        before = a.normal_counts
        removed = a.remove_far(c, 12.0)
        assert removed > 500 and a.normals_estimated and len(a.normal_counts) == len(before) - removed
        with M.on_grid(_cloud(P, a.points), MAP_VOXEL, 20, g) as b:
            b.estimate_normals(RHO, K_MIN)
            _same_estimate(a, b)
        state = _snapshot(a)
        assert a.remove_far(c, 12.0) == 0 and _snapshot(a) == state       # nothing more to drop: the map stays
        with pytest.raises(RuntimeError, match="would leave the map empty"):
            a.remove_far(c + 500.0, 1.0)
        assert _snapshot(a) == state


def test_merge_with_an_estimated_and_with_a_normal_free_other(P, small_pair, clouds):
    M = P.registration.VoxelPointMap
    g = M.centered_grid_min(clouds["target_xyz"].mean(0), MAP_VOXEL)
    T = small_pair["T_fgr"]
    merged = pm.merge(pm.build_map(clouds["target_xyz"], None, MAP_VOXEL, 8, g), pm.build_map(clouds["source_xyz"], None, MAP_VOXEL, 8, g, T))
    with M.on_grid(_cloud(P, merged.points), MAP_VOXEL, 8, g) as want:
        want.estimate_normals(RHO, K_MIN)
        assert vr.bits_equal(want.points, merged.points)
        for other_estimated in (True, False):
            with M.on_grid(clouds["target"], MAP_VOXEL, 8, g) as a, M.on_grid(clouds["source"], MAP_VOXEL, 8, g, T) as b:
                a.estimate_normals(RHO, K_MIN)
                if other_estimated:
                    b.estimate_normals(0.75, 3)                           # (its rule and its normals are derived data: not read)
                before = _snapshot(b)
                a.merge(b)
                _same_estimate(a, want)
                assert (a.normal_radius, a.normal_min_neighbors) == (RHO, K_MIN) and _snapshot(b) == before
        # a map without normals stays without, whatever the other has derived
        with M.on_grid(clouds["target"], MAP_VOXEL, 8, g) as a, M.on_grid(clouds["source"], MAP_VOXEL, 8, g, T) as b:
            b.estimate_normals(RHO, K_MIN)
            a.merge(b)
            assert not a.has_normals and not a.normals_estimated and vr.bits_equal(a.points, merged.points)
            with pytest.raises(RuntimeError, match="no normals"):
                a.normals
            with pytest.raises(RuntimeError, match="estimate"):
                a.normal_counts


# ------------------------------------------------------------------------------------------ 5. all or nothing, and the refusals
def _ctx(P):
    return P._lib.Context.current()


def _message(ctx):
    return (ctx.lib.pcr_last_error(ctx.handle) or b"").decode()


def test_refused_calls_leave_the_map_as_it_was(P, clouds):
    L = P._lib
    M = P.registration.VoxelPointMap
    ctx = _ctx(P)
    lib = ctx.lib
    g = M.centered_grid_min(clouds["target_xyz"].mean(0), MAP_VOXEL)

    def refused(rc, word):
        assert rc == L.PCR_EINVAL and word in _message(ctx), (rc, word, _message(ctx))

    with_normals = _cloud(P, clouds["target_xyz"], np.tile(np.array([[0, 0, 1]], np.float32), (len(clouds["target_xyz"]), 1)))
    with M.on_grid(clouds["target"], MAP_VOXEL, 20, g) as m, M.on_grid(with_normals, MAP_VOXEL, 20, g) as own, M.on_grid(clouds["source"], MAP_VOXEL, 20, g) as bare:
        assert m.estimate_normals(RHO, K_MIN) > 6000
        state = _snapshot(m)
        h, valid = m._open(), C.c_int64(-1)
        far = clouds["source_xyz"].copy()
        far[17] = [0.0, -3.0e6, 0.0]                                     # one point below the grid's first cell
        with pytest.raises(RuntimeError, match="outside the map's grid"):
            m.insert(_cloud(P, far))
        assert _snapshot(m) == state
        for r in (0.0, -1.0, float("nan"), float("inf"), 1.0 + 2.0 ** -40):
            refused(lib.pcr_point_map_estimate_normals(ctx.handle, h, C.c_double(r), 5, C.byref(valid)), "radius")
        for k in (2, 0, -5):
            refused(lib.pcr_point_map_estimate_normals(ctx.handle, h, C.c_double(1.0), k, C.byref(valid)), "min_neighbors")
        refused(lib.pcr_point_map_estimate_normals(ctx.handle, None, C.c_double(1.0), 5, None), "map is null")
        refused(lib.pcr_point_map_estimate_normals(ctx.handle, own._open(), C.c_double(1.0), 5, None), "normals")
        xyz, n = clouds["source"].device_xyz().data_ptr(), len(clouds["source"])
        refused(lib.pcr_point_map_insert(ctx.handle, h, xyz, with_normals.device_normals().data_ptr(), n, None), "normals")
        refused(lib.pcr_point_map_merge(ctx.handle, h, own._open()), "normals")
        refused(lib.pcr_point_map_merge(ctx.handle, own._open(), h), "normals")
        t = P.geometry._torch().empty((len(m),), dtype=P.geometry._torch().int32, device="cuda")
        refused(lib.pcr_point_map_read_normal_counts(ctx.handle, bare._open(), t.data_ptr()), "map does not estimate")
        refused(lib.pcr_point_map_read_normal_counts(ctx.handle, own._open(), t.data_ptr()), "map does not estimate")
        refused(lib.pcr_point_map_read_normal_counts(ctx.handle, h, None), "counts")
        assert _snapshot(m) == state
        # the Python surface
        with pytest.raises(RuntimeError, match="normals of the caller's"):
            own.estimate_normals()
        for bad in (dict(radius=0.0), dict(radius=1.5), dict(radius=float("nan")), dict(radius="wide")):
            with pytest.raises(ValueError, match="radius"):
                m.estimate_normals(**bad)
        for bad in (2, 2.5, None):
            with pytest.raises(ValueError, match="min_neighbors"):
                m.estimate_normals(1.0, bad)
        with pytest.raises(RuntimeError, match="estimate"):
            bare.normal_counts
        est, radius, kmin = C.c_int(-1), C.c_double(-1), C.c_int(-1)
        assert lib.pcr_point_map_normal_rule(own._open(), C.byref(est), C.byref(radius), C.byref(kmin)) == 0 and (est.value, radius.value, kmin.value) == (0, 0.0, 0)
        assert lib.pcr_point_map_normal_rule(h, C.byref(est), C.byref(radius), C.byref(kmin)) == 0 and (est.value, radius.value, kmin.value) == (1, RHO, K_MIN)
        has = C.c_int(-1)
        assert lib.pcr_point_map_grid(h, None, None, None, None, C.byref(has)) == 0 and has.value == 1
        assert _snapshot(m) == state
        # an estimated map takes a cloud with normals and does not read them
        m.insert(with_normals, _pose(1.0, [0.1, 0.0, 0.0]))
        bare_twin = _cloud(P, clouds["target_xyz"])
        with M.on_grid(clouds["target"], MAP_VOXEL, 20, g) as twin:
            twin.estimate_normals(RHO, K_MIN)
            twin.insert(bare_twin, _pose(1.0, [0.1, 0.0, 0.0]))
            _same_estimate(m, twin)


# ------------------------------------------------------------------------------------------ 6. one linearisation
def _plane(P, loss, k=GM_K):
    R = P.registration
    return R.TransformationEstimationPointToPlane({"l2": R.L2Loss(), "l1": R.L1Loss(), "gm": R.GMLoss(k)}[loss])


@pytest.mark.parametrize("loss", ["l2", "l1", "gm"])
def test_linearize_counts_the_valid_rows(P, small_pair, clouds, est_map, ref_map, loss):
    """the band of test_linearize_matches_reference (tests/test_gpu_point_map.py): 1e-9 x the summed magnitudes of an entry's terms"""
    ref_m, valid = ref_map
    T = small_pair["T_fgr"]
    for nbh, dist in ((27, 1.0), (7, 0.6)):
        ref = pn.linearize(ref_m, valid, clouds["source_xyz"], T, dist, nbh, LOSS[loss], GM_K)
        every = len(pm.rows_at(ref_m, clouds["source_xyz"], T, dist, nbh))
        got = est_map.linearize(clouds["source"], T, dist, _plane(P, loss), nbh)
        print(f"plane {loss} nbh {nbh}: {got.rows} rows of {every} matches")
        assert got.rows == ref["rows"] > 3000 and ref["rows"] < every      # (some matches ARE dropped: the filter is exercised)
        for name, a, b, mag in (("JTJ", got.JTJ, ref["JTJ"], ref["mag_JTJ"]), ("JTr", got.JTr, ref["JTr"], ref["mag_JTr"])):
            err = np.abs(a - b)
            print(f"plane {loss} nbh {nbh} {name}: largest error / magnitude {float((err / np.maximum(mag, 1e-300)).max()):.1e}")
            assert (err <= 1e-9 * mag).all(), (name, float(err.max()))
        assert abs(got.sum_d2 - ref["sum_d2"]) <= 1e-9 * ref["sum_d2"] and abs(got.sum_r2 - ref["sum_r2"]) <= 1e-9 * ref["sum_r2"]
        assert np.array_equal(got.JTJ, got.JTJ.T)
        again = est_map.linearize(clouds["source"], T, dist, _plane(P, loss), nbh)
        assert got.JTJ.tobytes() == again.JTJ.tobytes() and got.JTr.tobytes() == again.JTr.tobytes() and (got.rows, got.sum_d2, got.sum_r2) == (again.rows, again.sum_d2, again.sum_r2)


def test_point_to_point_never_reads_validity(P, small_pair, clouds, est_map):
    R = P.registration
    T = small_pair["T_fgr"]
    with R.VoxelPointMap(clouds["target"], MAP_VOXEL, 20) as bare:
        assert not bare.has_normals
        for loss, nbh in (("l2", 27), ("gm", 7), ("l1", 27)):
            est = R.TransformationEstimationPointToPoint(False, {"l2": R.L2Loss(), "l1": R.L1Loss(), "gm": R.GMLoss(GM_K)}[loss])
            a, b = est_map.linearize(clouds["source"], T, 1.0, est, nbh), bare.linearize(clouds["source"], T, 1.0, est, nbh)
            assert a.JTJ.tobytes() == b.JTJ.tobytes() and a.JTr.tobytes() == b.JTr.tobytes() and (a.rows, a.sum_d2, a.sum_r2) == (b.rows, b.sum_d2, b.sum_r2)
        ra = R.registration_point_map(clouds["source"], est_map, 1.0, init=T)
        rb = R.registration_point_map(clouds["source"], bare, 1.0, init=T)
        assert ra.transformation.tobytes() == rb.transformation.tobytes() and np.array_equal(ra.correspondence_set, rb.correspondence_set)
        assert (ra.fitness, ra.inlier_rmse, ra.iterations) == (rb.fitness, rb.inlier_rmse, rb.iterations)
        # the search is purely geometric on either map
        assert np.array_equal(est_map.correspondences(clouds["source"], T, 1.0, 27).cpu().numpy(), bare.correspondences(clouds["source"], T, 1.0, 27).cpu().numpy())


# ------------------------------------------------------------------------------------------ 7. the trajectories
@pytest.fixture(scope="module")
def reference_loop(small_pair, clouds, ref_map):
    ref_m, valid = ref_map

    @functools.lru_cache(maxsize=None)
    def run(loss, nbh):
        return pn.loop(ref_m, valid, clouds["source_xyz"], small_pair["T_fgr"], 1.0, nbh, LOSS[loss], GM_K, 30)
    return run


@pytest.mark.parametrize("nbh", [7, 27])
@pytest.mark.parametrize("loss", ["l2", "gm"])
def test_trajectory_matches_reference(P, small_pair, clouds, est_map, ref_map, reference_loop, loss, nbh):
    """the bands of test_trajectory_matches_reference in tests/test_gpu_point_map.py"""
    R = P.registration
    ref_m, valid = ref_map
    full = reference_loop(loss, nbh)
    assert full.iterations > 2, full
    for max_it in (1, 2, 5, 30):
        ref = full.after(max_it)
        res = R.registration_point_map(clouds["source"], est_map, 1.0, None, small_pair["T_fgr"], _plane(P, loss), R.ICPConvergenceCriteria(1e-6, 1e-6, max_it), nbh)
        ang, dt = pose_error(res.transformation, ref.transformation)
        print(f"plane {loss} nbh {nbh} max_it {max_it}: {ang:.2e} rad {dt:.2e} m, iterations {res.iterations} / {ref.iterations}, rows {len(res.correspondence_set)} / {ref.n_rows}, "
              f"fitness {res.fitness - ref.fitness:+.1e} rmse {res.inlier_rmse - ref.inlier_rmse:+.1e}")
        assert ang < 1e-7 and dt < 1e-6, (loss, nbh, max_it, ang, dt)
        assert res.iterations == ref.iterations and res.converged == ref.converged, (max_it, res.iterations, ref.iterations, res.converged, ref.converged)
        assert abs(res.fitness - ref.fitness) < 1e-12 and abs(res.inlier_rmse - ref.inlier_rmse) < 1e-9
        # the correspondence set is the rule's rows at the returned pose, without the matches to rows that are not valid
        assert np.array_equal(res.correspondence_set, pn.rows_at(ref_m, valid, clouds["source_xyz"], res.transformation, 1.0, nbh))
        assert res.fitness == len(res.correspondence_set) / len(clouds["source"])


# ------------------------------------------------------------------------------------------ 8. odometry
def _step():
    a = np.deg2rad(1.0)
    S = np.eye(4)
    S[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
    S[:3, 3] = [0.2, 0.0, 0.0]
    return S


def test_odometry_on_scans_without_normals(P, clouds):
    """the drive of tests/test_gpu_point_map.py -- four views of the 0.3 m target of pair 899, 0.2 m and 1 degree apart -- with scans that carry no
    normals: under "static" the start of scan k is the pose of scan k - 1, one step from the truth.  First the numpy restatement, then the device."""
    R = P.registration
    truth, arrays = [np.eye(4)], []
    for k in range(4):
        if k:
            truth.append(truth[-1] @ _step())
        inv = np.linalg.inv(truth[k])
        arrays.append((clouds["target_xyz"].astype(np.float64) @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32))
    scans = [P.PointCloud(a) for a in arrays]
    assert not any(s.has_normals() for s in scans)
    g = R.VoxelPointMap.centered_grid_min(scans[0].get_center(), MAP_VOXEL)

    def closer(poses, who):
        for k in range(1, 4):
            a0, d0 = pose_error(poses[k - 1], truth[k])
            a, d = pose_error(poses[k], truth[k])
            print(f"{who} scan {k}: start {a0:.2e} rad {d0:.3f} m -> {a:.2e} rad {d:.4f} m")
            assert a < a0 and d < d0, (who, k, a, d, a0, d0)

    ref_poses, _, _ = pn.odometry(arrays, MAP_VOXEL, 1.0, 10, g, RHO, K_MIN)
    closer(ref_poses, "restatement")
    poses, results, m = R.scan_to_map_odometry_icp_map_normals(scans, MAP_VOXEL, 1.0, estimation_method=R.TransformationEstimationPointToPlane(), motion_model="static",
                                                   max_points_per_voxel=10, map_normal_radius=RHO)
    with m:
        assert len(poses) == len(results) == 4 and results[0] is None and np.array_equal(poses[0], np.eye(4))
        closer(poses, "device")
        assert m.normals_estimated and (m.normal_radius, m.normal_min_neighbors) == (RHO, K_MIN) and np.array_equal(m.grid_min, g)
        # the returned map's normals are those of a fresh estimated map of the same inserts
        with R.VoxelPointMap.on_grid(scans[0], MAP_VOXEL, 10, g, np.eye(4)) as fresh:
            for k in range(1, 4):
                fresh.insert(scans[k], poses[k])
            fresh.estimate_normals(RHO, K_MIN)
            _same_estimate(m, fresh)
    # scans that carry normals give the same poses: their normals are not read
    for s in scans:
        s.normals = np.tile(np.array([[1.0, 0.0, 0.0]], np.float32), (len(s), 1))
    poses2, _, m2 = R.scan_to_map_odometry_icp_map_normals(scans, MAP_VOXEL, 1.0, estimation_method=R.TransformationEstimationPointToPlane(), motion_model="static",
                                               max_points_per_voxel=10, map_normal_radius=RHO)
    m2.close()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(poses, poses2))
