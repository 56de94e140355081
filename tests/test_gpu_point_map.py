"""The voxel point map and scan-to-map ICP on the device against the numpy restatement of their rule (tests/point_map_reference.py): the map
bit for bit, the growth calls, the rows exactly, one linearisation, the trajectories of the loop, the parent's own registration_icp, and the
edges.  Pair 899 with both clouds at voxel 0.3 against a 1.0 m map (the conditions of these comparisons -- cells are in fact cut at M = 8 and
M = 20, most source points have a row -- are checked on the CPU in tests/test_point_map_api.py), and clouds of tens of points."""
import ctypes as C
import functools

import numpy as np
import pytest

import point_map_reference as pm
import voxel_reference as vr
from conftest import pkg, pose_error

pytestmark = pytest.mark.gpu

MAP_VOXEL = 1.0
LOSS = {"l2": pm.L2, "l1": pm.L1, "gm": pm.GM}
KIND = {"point": pm.POINT_TO_POINT, "plane": pm.POINT_TO_PLANE}
GM_K = 0.5
# registration_point_map (point to plane, L2, neighbourhood 27, distance 1.0 = the voxel) against registration_icp on map.to_point_cloud(), pair 899 from
# T_fgr, 30 iterations (both stop after 7 with the same 6081 rows): the pose difference measured on an MI355X, 1.239e-16 rad and 1.268e-15 m (DESIGN.md
# 4.27) -- the last bits of two float64 sums taken in different orders.  The test asserts ten times this.
PARENT_RAD, PARENT_M = 1.239e-16, 1.268e-15


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
        out[key + "_nrm"] = pc._nrm.cpu().numpy()
    assert (len(out["source"]), len(out["target"])) == (6897, 7074)
    return out


def _cloud(P, xyz, nrm=None):
    pc = P.PointCloud(np.ascontiguousarray(xyz, np.float32))
    if nrm is not None:
        pc.normals = np.ascontiguousarray(nrm, np.float32)
    return pc


def _assert_map_equals(dev, ref):
    assert len(dev) == len(ref)
    assert np.array_equal(dev.cells, ref.cells)                       # the same cells in the same (Morton) order
    assert np.array_equal(dev.starts, ref.starts) and np.array_equal(dev.counts, ref.counts)
    assert vr.bits_equal(dev.points, ref.points)
    assert dev.has_normals == (ref.normals is not None)
    if dev.has_normals:
        assert vr.bits_equal(dev.normals, ref.normals)


def _state(m):
    return (m.cells.tobytes(), m.starts.tobytes(), m.counts.tobytes(), m.points.tobytes(), m.normals.tobytes() if m.has_normals else None)


@pytest.fixture(scope="module")
def ref_map(clouds):
    return pm.build_map(clouds["target_xyz"], clouds["target_nrm"], MAP_VOXEL, 20)


@pytest.fixture(scope="module")
def dev_map(P, clouds):
    m = P.registration.VoxelPointMap(clouds["target"], MAP_VOXEL, 20)
    yield m
    m.close()


# ------------------------------------------------------------------------------------------ the map, bit for bit
@pytest.mark.parametrize("M", [8, 20])
def test_map_of_pair_899(P, clouds, M):
    ref = pm.build_map(clouds["target_xyz"], clouds["target_nrm"], MAP_VOXEL, M)
    with P.registration.VoxelPointMap(clouds["target"], MAP_VOXEL, M) as dev:
        _assert_map_equals(dev, ref)
        assert dev.max_points_per_voxel == M and dev.voxel_size == MAP_VOXEL and np.array_equal(dev.grid_min, ref.grid_min) and np.array_equal(dev.origin, ref.origin)
        back = dev.to_point_cloud()
        assert vr.bits_equal(back._xyz.cpu().numpy(), ref.points) and vr.bits_equal(back._nrm.cpu().numpy(), ref.normals)
    bare = P.PointCloud(clouds["target_xyz"])
    with P.registration.VoxelPointMap(bare, MAP_VOXEL, M) as dev:
        _assert_map_equals(dev, pm.build_map(clouds["target_xyz"], None, MAP_VOXEL, M))
        with pytest.raises(RuntimeError, match="no normals"):
            dev.normals


@pytest.mark.parametrize("M", [1, 2, 64])
def test_map_of_forty_points(P, M):
    rng = np.random.default_rng(40)
    xyz = rng.uniform(0.0, 2.5, (40, 3)).astype(np.float32)
    nrm = rng.normal(size=(40, 3)).astype(np.float32)
    ref = pm.build_map(xyz, nrm, 1.0, M)
    assert ref.counts.max() == min(M, ref.counts.max()) and (M > 2 or (ref.counts == M).sum() > 3)
    with P.registration.VoxelPointMap(_cloud(P, xyz, nrm), 1.0, M) as dev:
        _assert_map_equals(dev, ref)


def _cells_cloud(members, seed, jitter=0.3):
    """points of given cells of the voxel-1 grid with grid_min 0 (cell c spans [c - 0.5, c + 0.5)): members = [(cell, count), ...], shuffled"""
    rng = np.random.default_rng(seed)
    cell = np.concatenate([np.repeat(np.array([c], np.float64), k, 0) for c, k in members])
    xyz = (cell + rng.uniform(-jitter, jitter, cell.shape)).astype(np.float32)
    return xyz[rng.permutation(len(xyz))]


def test_cells_with_exactly_m_m_plus_one_and_three_m_members(P):
    M = 4
    xyz = _cells_cloud([((3, 1, 2), M), ((0, 5, 1), M + 1), ((2, 2, 2), 3 * M), ((7, 0, 0), 1), ((1, 1, 1), M - 1)], 1)
    ref = pm.build_map(xyz, None, 1.0, M, np.zeros(3))
    assert sorted(ref.counts.tolist()) == [1, M - 1, M, M, M] and len(ref) == 4 * M
    with P.registration.VoxelPointMap.on_grid(_cloud(P, xyz), 1.0, M, np.zeros(3)) as dev:
        _assert_map_equals(dev, ref)


def test_points_on_a_cell_face(P):
    """coordinates k + 0.5 are exactly the faces of the grid of grid_min 0 and voxel 1: such a point belongs to the upper cell"""
    g = np.stack(np.meshgrid(np.arange(3), np.arange(3), np.arange(2), indexing="ij"), -1).reshape(-1, 3)
    xyz = np.concatenate([g + 0.5, g + np.array([0.5, 0.25, 0.0]), g.astype(np.float64)]).astype(np.float32)
    ref = pm.build_map(xyz, None, 1.0, 3, np.zeros(3))
    assert (np.floor(xyz[:len(g)].astype(np.float64) + 0.5) == g + 1).all() and ref.cells.max() == 3
    with P.registration.VoxelPointMap.on_grid(_cloud(P, xyz), 1.0, 3, np.zeros(3)) as dev:
        _assert_map_equals(dev, ref)


def _pose(deg, t):
    a = np.deg2rad(deg)
    T = np.eye(4)
    T[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
    T[:3, :3] = T[:3, :3] @ np.array([[1, 0, 0], [0, np.cos(0.3 * a), -np.sin(0.3 * a)], [0, np.sin(0.3 * a), np.cos(0.3 * a)]])
    T[:3, 3] = t
    return T


def test_on_grid_at_a_pose_with_normals(P, clouds):
    M = P.registration.VoxelPointMap
    T = _pose(33.0, [4.0, -7.0, 1.5])
    g = M.centered_grid_min(T[:3, :3] @ clouds["target_xyz"].mean(0) + T[:3, 3], MAP_VOXEL)
    ref = pm.build_map(clouds["target_xyz"], clouds["target_nrm"], MAP_VOXEL, 8, g, T)
    assert not vr.bits_equal(ref.normals[:50], pm.build_map(clouds["target_xyz"], clouds["target_nrm"], MAP_VOXEL, 8, g, np.eye(4)).normals[:50])
    with M.on_grid(clouds["target"], MAP_VOXEL, 8, g, T) as dev:
        _assert_map_equals(dev, ref)
    # no pose: the members are the inputs bit for bit, -0 included
    z = np.array([[-0.0, 0.25, 1.0], [0.5, -0.0, 2.0]], np.float32)
    with M.on_grid(_cloud(P, z, z), 1.0, 8, np.array([-4.0, -4.0, -4.0])) as dev:
        assert np.signbit(dev.points).sum() == 2
        _assert_map_equals(dev, pm.build_map(z, z, 1.0, 8, np.array([-4.0, -4.0, -4.0])))


# ------------------------------------------------------------------------------------------ growth
def test_insert_into_a_cell_with_one_place_left(P):
    M = 5
    g = np.zeros(3)
    first = _cells_cloud([((2, 2, 2), M - 1), ((4, 0, 1), 2)], 2)
    more = _cells_cloud([((2, 2, 2), 3), ((4, 0, 1), 1)], 3)
    ref0 = pm.build_map(first, None, 1.0, M, g)
    ref = pm.insert(ref0, more, None)
    row = int(ref.starts[[tuple(c) for c in ref.cells].index((2, 2, 2))])
    new_in_cell = more[(np.floor(more.astype(np.float64) + 0.5) == [2, 2, 2]).all(1)]
    assert len(new_in_cell) == 3 and ref.points[row + M - 1].tobytes() == new_in_cell[0].tobytes() and len(ref) == M + 3
    with P.registration.VoxelPointMap.on_grid(_cloud(P, first), 1.0, M, g) as dev:
        _assert_map_equals(dev, ref0)
        dev.insert(_cloud(P, more))
        _assert_map_equals(dev, ref)


def test_insert_that_adds_only_new_cells(P):
    g = np.zeros(3)
    first, more = _cells_cloud([((1, 1, 1), 3), ((5, 5, 5), 2)], 4), _cells_cloud([((0, 0, 0), 2), ((3, 3, 3), 4), ((9, 1, 1), 1)], 5)
    ref0 = pm.build_map(first, None, 1.0, 3, g)
    ref = pm.insert(ref0, more, None)
    assert len(ref.cells) == 5 and len(ref) == 5 + 2 + 3 + 1
    with P.registration.VoxelPointMap.on_grid(_cloud(P, first), 1.0, 3, g) as dev:
        dev.insert(_cloud(P, more))
        _assert_map_equals(dev, ref)


def test_merge_both_ways(P, small_pair, clouds):
    M = P.registration.VoxelPointMap
    g = M.centered_grid_min(clouds["target_xyz"].mean(0), MAP_VOXEL)
    T = small_pair["T_fgr"]
    ra = pm.build_map(clouds["target_xyz"], clouds["target_nrm"], MAP_VOXEL, 8, g)
    rb = pm.build_map(clouds["source_xyz"], clouds["source_nrm"], MAP_VOXEL, 8, g, T)
    ab, ba = pm.merge(ra, rb), pm.merge(rb, ra)
    assert np.array_equal(ab.cells, ba.cells) and not vr.bits_equal(ab.points, ba.points)      # an overflowing shared cell keeps the first map's members
    with M.on_grid(clouds["target"], MAP_VOXEL, 8, g) as a, M.on_grid(clouds["source"], MAP_VOXEL, 8, g, T) as b:
        before = _state(b)
        a.merge(b)
        _assert_map_equals(a, ab)
        assert _state(b) == before
    with M.on_grid(clouds["target"], MAP_VOXEL, 8, g) as a, M.on_grid(clouds["source"], MAP_VOXEL, 8, g, T) as b:
        b.merge(a)
        _assert_map_equals(b, ba)


def test_remove_far(P, small_pair, clouds):
    M = P.registration.VoxelPointMap
    c = clouds["target_xyz"].astype(np.float64).mean(0)
    g = M.centered_grid_min(c, MAP_VOXEL)
    whole = pm.build_map(clouds["target_xyz"], clouds["target_nrm"], MAP_VOXEL, 20, g)
    with M.on_grid(clouds["target"], MAP_VOXEL, 20, g) as dev:
        ref = pm.remove_far(whole, c, 12.0)
        old = dict(zip(map(tuple, whole.cells), whole.counts))
        assert len(ref.cells) < len(whole.cells) - 50 and sum(1 for cc, k in zip(ref.cells, ref.counts) if k < old[tuple(cc)]) > 10      # cells emptied, cells thinned
        assert dev.remove_far(c, 12.0) == len(whole) - len(ref)
        _assert_map_equals(dev, ref)
        assert dev.remove_far(c, 12.0) == 0                             # nothing more to drop: the map stays
        _assert_map_equals(dev, ref)
        before = _state(dev)
        with pytest.raises(RuntimeError, match="would leave the map empty"):
            dev.remove_far(c + 500.0, 1.0)
        assert _state(dev) == before
        ref2 = pm.insert(ref, clouds["source_xyz"], clouds["source_nrm"], small_pair["T_fgr"])      # a thinned cell has room again
        assert len(ref2) > len(ref) + 1000
        dev.insert(clouds["source"], small_pair["T_fgr"])
        _assert_map_equals(dev, ref2)


def test_outside_the_grid_is_refused_on_both_sides(P):
    M = P.registration.VoxelPointMap
    xyz = np.array([[0, 0, 0], [1, 1, 1], [2, 0, 1]], np.float32)
    with M.on_grid(_cloud(P, xyz), 1.0, 4, np.zeros(3)) as dev:
        before = _state(dev)
        for bad in ([[-0.6, 0, 0]], [[0, 0, 2097151.6]], [[1, 1, 1], [0, -1, 0]]):
            with pytest.raises(RuntimeError, match="outside the map's grid"):
                dev.insert(_cloud(P, np.array(bad, np.float32)))
            with pytest.raises(pm.OutsideGrid):
                pm.insert(pm.build_map(xyz, None, 1.0, 4, np.zeros(3)), np.array(bad, np.float32), None)
        down = np.eye(4); down[0, 3] = -3.0
        with pytest.raises(RuntimeError, match="outside the map's grid"):
            dev.insert(_cloud(P, xyz), down)
        assert _state(dev) == before
        dev.insert(_cloud(P, np.array([[-0.5, 0, 2097151.0]], np.float32)))      # the first and the last cell of an axis are inside
        assert len(dev) == 4 and dev.cells.min() == 0 and dev.cells.max() == 2097151
    with pytest.raises(RuntimeError, match="outside the map's grid"):
        M.on_grid(_cloud(P, xyz), 1.0, 4, np.array([0.6, 0.0, 0.0]))


def test_three_inserts_equal_sequential_arrival(P, clouds):
    M = P.registration.VoxelPointMap
    g = M.centered_grid_min(clouds["target_xyz"].mean(0), MAP_VOXEL)
    arrivals = [(clouds["target_xyz"], clouds["target_nrm"], None), (clouds["source_xyz"], clouds["source_nrm"], _pose(2.0, [0.3, -0.2, 0.0])),
                (clouds["target_xyz"][::3], clouds["target_nrm"][::3], _pose(-1.0, [-0.1, 0.4, 0.05])), (clouds["source_xyz"][::2], clouds["source_nrm"][::2], None)]
    cells, lists = pm.sequential(arrivals, MAP_VOXEL, 6, g)
    with M.on_grid(clouds["target"], MAP_VOXEL, 6, g) as dev:
        dev.insert(clouds["source"], arrivals[1][2])
        dev.insert(_cloud(P, arrivals[2][0], arrivals[2][1]), arrivals[2][2])
        dev.insert(_cloud(P, arrivals[3][0], arrivals[3][1]))
        got = pm._finish(pm.PointMapRef(MAP_VOXEL, g, 6, dev.points, dev.normals, np.repeat(dev.cells.astype(np.int64), dev.counts, 0)))
        assert np.array_equal(got.starts, dev.starts) and pm.equals_sequential(got, cells, lists)
        assert (dev.counts == 6).sum() > 500


# ------------------------------------------------------------------------------------------ the rows, exactly
@pytest.mark.parametrize("nbh", [1, 7, 27])
def test_rows_equal_the_reference(small_pair, clouds, dev_map, ref_map, nbh):
    for dist in (0.3, 1.0, 2.5):
        ref = pm.rows_at(ref_map, clouds["source_xyz"], small_pair["T_fgr"], dist, nbh)
        got = dev_map.correspondences(clouds["source"], small_pair["T_fgr"], dist, nbh).cpu().numpy()
        assert len(ref) > 500, (dist, len(ref))
        assert got.dtype == np.int32 and np.array_equal(got, ref), (nbh, dist, len(got), len(ref))


def test_rows_on_small_maps(P):
    R = P.registration
    # a one-cell map
    cell = np.array([[0.1, 0.2, 0.3], [0.3, 0.1, 0.2], [0.2, 0.3, 0.1]], np.float32)
    src = np.array([[0.1, 0.2, 0.25], [0.9, 0.9, 0.9], [5.0, 5.0, 5.0], [0.0, 0.0, 0.0]], np.float32)
    ref = pm.build_map(cell, None, 1.0, 8)
    with R.VoxelPointMap(_cloud(P, cell), 1.0, 8) as dev:
        assert len(dev.cells) == 1
        for nbh in (1, 7, 27):
            for dist in (0.2, 1.0, 10.0):
                assert np.array_equal(dev.correspondences(_cloud(P, src), np.eye(4), dist, nbh).cpu().numpy(), pm.rows_at(ref, src, np.eye(4), dist, nbh)), (nbh, dist)
        assert len(pm.rows_at(ref, src, np.eye(4), 10.0, 27)) == 3 and len(pm.rows_at(ref, src, np.eye(4), 10.0, 1)) == 2
    # a query equidistant from two rows (all values exact in float32): the smaller row index wins; and a duplicate point in the map
    tgt = np.array([[1.0, 0.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 3.0, 0.0], [0.0, 3.0, 0.0], [0.25, 3.0, 0.0]], np.float32)
    q = np.array([[0.0, 0.0, 0.0], [0.0, 3.0, 0.125], [0.0, 0.25, 0.0]], np.float32)
    ref = pm.build_map(tgt, None, 8.0, 8, np.zeros(3))                 # one cell: [-4, 4) on every axis
    with R.VoxelPointMap.on_grid(_cloud(P, tgt), 8.0, 8, np.zeros(3)) as dev:
        want = pm.rows_at(ref, q, np.eye(4), 2.0, 27)
        assert len(dev.cells) == 1 and vr.bits_equal(dev.points, tgt)
        assert want.tolist() == [[0, 0], [1, 2], [2, 0]]
        for nbh in (1, 7, 27):
            assert np.array_equal(dev.correspondences(_cloud(P, q), np.eye(4), 2.0, nbh).cpu().numpy(), want)


def test_source_wholly_outside_the_grid(P, clouds, dev_map):
    R = P.registration
    far = _cloud(P, clouds["source_xyz"] - np.float32(5000.0))
    init = np.eye(4)
    init[:3, 3] = [0.5, -0.25, 0.125]
    assert len(dev_map.correspondences(far, init, 1.0, 27)) == 0
    for nbh in (1, 27):
        res = R.registration_point_map(far, dev_map, 1.0, init=init, neighborhood=nbh)
        assert np.array_equal(res.transformation, init) and res.fitness == 0 and res.inlier_rmse == 0
        assert res.converged and res.iterations == 1 and len(res.correspondence_set) == 0


def test_one_source_point(P, clouds, dev_map, ref_map, small_pair):
    R = P.registration
    i = int(pm.rows_at(ref_map, clouds["source_xyz"], small_pair["T_fgr"], 0.3, 27)[0, 0])
    one = clouds["source"].select_by_index([i])
    res = R.registration_point_map(one, dev_map, 1.0, None, small_pair["T_fgr"], criteria=R.ICPConvergenceCriteria(1e-6, 1e-6, 2))
    assert 1 <= res.iterations <= 2 and np.isfinite(res.transformation).all()
    rows = pm.rows_at(ref_map, clouds["source_xyz"][i:i + 1], res.transformation, 1.0, 27)
    assert np.array_equal(res.correspondence_set, rows) and res.fitness == (1.0 if len(rows) else 0.0)
    empty = R.registration_point_map(P.PointCloud(np.zeros((0, 3))), dev_map, 1.0, init=small_pair["T_fgr"])
    assert empty.fitness == 0 and np.array_equal(empty.transformation, small_pair["T_fgr"]) and empty.converged and empty.iterations == 1


# ------------------------------------------------------------------------------------------ one linearisation
def _estimation(P, kind, loss, k=GM_K):
    R = P.registration
    kernel = {"l2": R.L2Loss(), "l1": R.L1Loss(), "gm": R.GMLoss(k)}[loss]
    return R.TransformationEstimationPointToPlane(kernel) if kind == "plane" else R.TransformationEstimationPointToPoint(False, kernel)


@pytest.mark.parametrize("loss", ["l2", "l1", "gm"])
@pytest.mark.parametrize("kind", ["point", "plane"])
def test_linearize_matches_reference(P, small_pair, clouds, dev_map, ref_map, kind, loss):
    """|device - reference| <= 1e-9 x the sum of the absolute values of the entry's terms (the bound of tests/test_gpu_multiway.py: a regrouping of
    n float64 terms moves a sum by at most about n 2^-53 of that, 1e-12 here; what is left is room for the rows' own arithmetic)"""
    for nbh, dist in ((27, 1.0), (7, 0.6)):
        ref = pm.linearize(ref_map, clouds["source_xyz"], small_pair["T_fgr"], dist, nbh, KIND[kind], LOSS[loss], GM_K)
        got = dev_map.linearize(clouds["source"], small_pair["T_fgr"], dist, _estimation(P, kind, loss), nbh)
        assert got.rows == ref["rows"] > 3000
        for name, a, b, mag in (("JTJ", got.JTJ, ref["JTJ"], ref["mag_JTJ"]), ("JTr", got.JTr, ref["JTr"], ref["mag_JTr"])):
            err = np.abs(a - b)
            print(f"{kind} {loss} nbh {nbh} {name}: largest error / magnitude {float((err / np.maximum(mag, 1e-300)).max()):.1e}")
            assert (err <= 1e-9 * mag).all(), (name, float(err.max()))
        assert abs(got.sum_d2 - ref["sum_d2"]) <= 1e-9 * ref["sum_d2"] and abs(got.sum_r2 - ref["sum_r2"]) <= 1e-9 * ref["sum_r2"]
        assert np.array_equal(got.JTJ, got.JTJ.T)
        again = dev_map.linearize(clouds["source"], small_pair["T_fgr"], dist, _estimation(P, kind, loss), nbh)
        assert got.JTJ.tobytes() == again.JTJ.tobytes() and got.JTr.tobytes() == again.JTr.tobytes() and (got.rows, got.sum_d2, got.sum_r2) == (again.rows, again.sum_d2, again.sum_r2)


# ------------------------------------------------------------------------------------------ the trajectories
@pytest.fixture(scope="module")
def reference_loop(small_pair, clouds, ref_map):
    @functools.lru_cache(maxsize=None)
    def run(kind, loss, nbh, max_it=30, chunk=None):
        return pm.loop(ref_map, clouds["source_xyz"], small_pair["T_fgr"], 1.0, nbh, KIND[kind], LOSS[loss], GM_K, max_it, chunk=chunk)
    return run


@pytest.mark.parametrize("nbh", [7, 27])
@pytest.mark.parametrize("loss", ["l2", "gm"])
@pytest.mark.parametrize("kind", ["point", "plane"])
def test_trajectory_matches_reference(P, small_pair, clouds, dev_map, ref_map, reference_loop, kind, loss, nbh):
    """the bands of test_trajectory_matches_reference in tests/test_gpu_voxelized_gicp.py"""
    R = P.registration
    full = reference_loop(kind, loss, nbh)
    assert full.iterations > 2, full
    for max_it in (1, 2, 5, 30):
        ref = full.after(max_it)
        res = R.registration_point_map(clouds["source"], dev_map, 1.0, None, small_pair["T_fgr"], _estimation(P, kind, loss), R.ICPConvergenceCriteria(1e-6, 1e-6, max_it), nbh)
        ang, dt = pose_error(res.transformation, ref.transformation)
        print(f"{kind} {loss} nbh {nbh} max_it {max_it}: {ang:.2e} rad {dt:.2e} m, iterations {res.iterations} / {ref.iterations}, rows {len(res.correspondence_set)} / {ref.n_rows}, "
              f"fitness {res.fitness - ref.fitness:+.1e} rmse {res.inlier_rmse - ref.inlier_rmse:+.1e}")
        assert ang < 1e-7 and dt < 1e-6, (kind, loss, nbh, max_it, ang, dt)
        assert res.iterations == ref.iterations and res.converged == ref.converged, (max_it, res.iterations, ref.iterations, res.converged, ref.converged)
        assert abs(res.fitness - ref.fitness) < 1e-12 and abs(res.inlier_rmse - ref.inlier_rmse) < 1e-9
        # the correspondence set is the rule's rows at the returned pose
        assert np.array_equal(res.correspondence_set, pm.rows_at(ref_map, clouds["source_xyz"], res.transformation, 1.0, nbh))


@pytest.mark.parametrize("nbh", [7, 27])
@pytest.mark.parametrize("kind", ["point", "plane"])
def test_l1_trajectory_within_the_reference_spread(P, small_pair, clouds, dev_map, reference_loop, kind, nbh):
    """L1's 1 / |r| weights make the pose sensitive to the last bits of the sums, so the bound is derived on the spot, as conftest.l1_tolerance
    derives it: the restatement is run with three other summation chunkings (nothing else changes), and three times the largest distance of any
    of those end poses from the default one is the bound -- but never less than the band the L2 and GM trajectories are held to (1e-7 rad,
    1e-6 m), which no kernel can be asked to beat."""
    R = P.registration
    for max_it in (1, 2, 5):
        base = reference_loop(kind, "l1", nbh, 5).after(max_it)
        spread = [pose_error(reference_loop(kind, "l1", nbh, 5, chunk).after(max_it).transformation, base.transformation) for chunk in (64, 512, 4096)]
        tol_rad, tol_m = max(1e-7, 3.0 * max(s[0] for s in spread)), max(1e-6, 3.0 * max(s[1] for s in spread))
        res = R.registration_point_map(clouds["source"], dev_map, 1.0, None, small_pair["T_fgr"], _estimation(P, kind, "l1"), R.ICPConvergenceCriteria(1e-6, 1e-6, max_it), nbh)
        ang, dt = pose_error(res.transformation, base.transformation)
        print(f"l1 {kind} nbh {nbh} max_it {max_it}: {ang:.2e} rad {dt:.2e} m (bound {tol_rad:.1e} / {tol_m:.1e}, spread {max(s[0] for s in spread):.1e} / {max(s[1] for s in spread):.1e})")
        assert ang <= tol_rad and dt <= tol_m, (kind, nbh, max_it, ang, dt, spread)
        assert res.iterations == base.iterations


def test_against_registration_icp_on_the_map_cloud(P, small_pair, clouds, dev_map):
    """With a map that has normals, max_correspondence_distance <= voxel_size, neighbourhood 27 and L2 the correspondences are the exact nearest
    rows (the lemma), so point-to-plane registration_point_map and the parent's registration_icp on map.to_point_cloud() run the same rule and
    differ only in where the query is rounded (registration_icp searches with the float32 query) and in the order of the sums."""
    R = P.registration
    est, crit = R.TransformationEstimationPointToPlane(), R.ICPConvergenceCriteria(1e-6, 1e-6, 30)
    a = R.registration_point_map(clouds["source"], dev_map, 1.0, None, small_pair["T_fgr"], est, crit, 27)
    b = R.registration_icp(clouds["source"], dev_map.to_point_cloud(), 1.0, small_pair["T_fgr"], est, crit)
    ang, dt = pose_error(a.transformation, b.transformation)
    print(f"registration_point_map against registration_icp: {ang:.3e} rad {dt:.3e} m; iterations {a.iterations} / {b.iterations}, rows {len(a.correspondence_set)} / "
          f"{len(b.correspondence_set)}, fitness {a.fitness:.6f} / {b.fitness:.6f}, rmse {a.inlier_rmse:.6f} / {b.inlier_rmse:.6f}")
    assert 10 * PARENT_RAD <= 1e-5 and 10 * PARENT_M <= 1e-4
    assert ang <= 10 * PARENT_RAD and dt <= 10 * PARENT_M, (ang, dt)


# ------------------------------------------------------------------------------------------ housekeeping
def _key(res):
    return (res.transformation.tobytes(), res.fitness, res.inlier_rmse, res.iterations, res.converged, res.correspondence_set.tobytes())


def test_one_map_serves_many_calls(P, small_pair, clouds, dev_map):
    R = P.registration
    first = _key(R.registration_point_map(clouds["source"], dev_map, 1.0, init=small_pair["T_fgr"]))
    other = R.registration_point_map(clouds["source"], dev_map, 0.5, init=small_pair["T_fgr"], estimation_method=_estimation(P, "plane", "gm"), neighborhood=7)
    assert _key(other) != first
    assert _key(R.registration_point_map(clouds["source"], dev_map, 1.0, init=small_pair["T_fgr"])) == first
    # a cloud target builds a temporary map of voxel_size: the same result
    assert _key(R.registration_point_map(clouds["source"], clouds["target"], 1.0, MAP_VOXEL, small_pair["T_fgr"])) == first


def _ctx(P):
    return P._lib.Context.current()


def _message(ctx):
    return (ctx.lib.pcr_last_error(ctx.handle) or b"").decode()


def test_call_without_a_correspondence_buffer(P, small_pair, clouds, dev_map):
    R = P.registration
    want = R.registration_point_map(clouds["source"], dev_map, 1.0, init=small_pair["T_fgr"])
    ctx = _ctx(P)
    res = P._lib.PcrResult()
    p = P._lib.PcrPointMapParams(P._lib.PcrEstimation(P._lib.EST_POINT_TO_POINT, 0, 0, 1.0, 1e-3), 1e-6, 1e-6, 30, 27)
    T = np.ascontiguousarray(small_pair["T_fgr"], np.float64)
    rc = ctx.lib.pcr_registration_point_map(ctx.handle, clouds["source"].device_xyz().data_ptr(), len(clouds["source"]), dev_map._open(), C.c_double(1.0),
                                            T.ctypes.data_as(C.POINTER(C.c_double)), C.byref(p), C.byref(res), None)
    assert rc == 0, _message(ctx)
    assert np.array_equal(np.array(res.transformation).reshape(4, 4), want.transformation) and res.n_correspondences == len(want.correspondence_set)


def test_use_after_close_raises(P, clouds):
    M = P.registration.VoxelPointMap
    m = M(clouds["target"], MAP_VOXEL)
    with M(clouds["source"], MAP_VOXEL) as live:
        m.close()
        for call in (lambda: m.insert(clouds["source"]), lambda: m.merge(live), lambda: live.merge(m), lambda: m.remove_far([0, 0, 0], 1.0), lambda: m.grid_min, lambda: m.origin,
                     lambda: len(m), lambda: m.points, lambda: m.correspondences(clouds["source"], np.eye(4), 1.0),
                     lambda: P.registration.registration_point_map(clouds["source"], m, 1.0)):
            with pytest.raises(RuntimeError, match="closed"):
                call()
    m.close()                                                           # twice is allowed


def test_abi_refusals_name_the_argument(P, clouds, dev_map):
    L = P._lib
    ctx = _ctx(P)
    lib, dp = ctx.lib, C.POINTER(C.c_double)
    xyz, n = clouds["target"].device_xyz().data_ptr(), len(clouds["target"])
    eye = np.eye(4)
    Tp = eye.ctypes.data_as(dp)
    g = np.zeros(3)

    def refused(rc, word):
        assert rc == L.PCR_EINVAL and word in _message(ctx), (rc, word, _message(ctx))

    h = C.c_void_p()
    for M in (0, 65, -1):
        refused(lib.pcr_point_map_create(ctx.handle, xyz, None, n, 1.0, M, C.byref(h)), "max_points_per_voxel")
    refused(lib.pcr_point_map_create(ctx.handle, xyz, None, n, 0.0, 8, C.byref(h)), "voxel_size")
    refused(lib.pcr_point_map_create(ctx.handle, xyz, None, 0, 1.0, 8, C.byref(h)), "xyz")
    bad_g = np.array([0.0, np.nan, 0.0])
    refused(lib.pcr_point_map_create_on_grid(ctx.handle, xyz, None, n, 1.0, 8, bad_g.ctypes.data_as(dp), None, C.byref(h)), "grid_min3")
    bad_T = eye.copy(); bad_T[1, 2] = np.inf
    refused(lib.pcr_point_map_create_on_grid(ctx.handle, xyz, None, n, 1.0, 8, g.ctypes.data_as(dp), bad_T.ctypes.data_as(dp), C.byref(h)), "T holds")
    nan_cloud = _cloud(P, np.array([[0, 0, 0], [1, np.nan, 0]], np.float32))
    refused(lib.pcr_point_map_create(ctx.handle, nan_cloud.device_xyz().data_ptr(), None, 2, 1.0, 8, C.byref(h)), "xyz holds a non-finite")
    inf_n = _cloud(P, np.zeros((2, 3), np.float32), np.array([[0, 0, 1], [0, np.inf, 0]], np.float32))
    refused(lib.pcr_point_map_create(ctx.handle, inf_n.device_xyz().data_ptr(), inf_n.device_normals().data_ptr(), 2, 1.0, 8, C.byref(h)), "normals holds a non-finite")
    assert not h.value
    m = dev_map._open()
    src, ns = clouds["source"].device_xyz().data_ptr(), len(clouds["source"])
    rows = P.geometry._torch().empty((ns, 2), dtype=P.geometry._torch().int32, device="cuda")
    cnt = C.c_int64(0)
    for nbh in (0, 5, 26):
        refused(lib.pcr_point_map_correspondences(ctx.handle, m, src, ns, Tp, C.c_double(1.0), nbh, rows.data_ptr(), C.byref(cnt)), "neighborhood")
    for d in (0.0, -1.0, float("nan"), float("inf")):
        refused(lib.pcr_point_map_correspondences(ctx.handle, m, src, ns, Tp, C.c_double(d), 27, rows.data_ptr(), C.byref(cnt)), "max_correspondence_distance")
    refused(lib.pcr_point_map_correspondences(ctx.handle, m, src, ns, bad_T.ctypes.data_as(dp), C.c_double(1.0), 27, rows.data_ptr(), C.byref(cnt)), "T holds")
    refused(lib.pcr_point_map_correspondences(ctx.handle, None, src, ns, Tp, C.c_double(1.0), 27, rows.data_ptr(), C.byref(cnt)), "map is null")
    refused(lib.pcr_point_map_correspondences(ctx.handle, m, nan_cloud.device_xyz().data_ptr(), 2, Tp, C.c_double(1.0), 27, rows.data_ptr(), C.byref(cnt)), "src_xyz holds")
    res = L.PcrResult()
    est = lambda kind, scaling=0, loss=0: L.PcrPointMapParams(L.PcrEstimation(kind, scaling, loss, 1.0, 1e-3), 1e-6, 1e-6, 30, 27)      # noqa: E731
    reg = lambda mp, p: lib.pcr_registration_point_map(ctx.handle, src, ns, mp, C.c_double(1.0), Tp, C.byref(p), C.byref(res), None)      # noqa: E731
    refused(reg(m, est(L.EST_POINT_TO_POINT, 1)), "with_scaling")
    refused(reg(m, est(L.EST_GENERALIZED_ICP)), "estimation.kind")
    refused(reg(m, est(L.EST_POINT_TO_PLANE, 0, 7)), "estimation.loss")
    p = est(L.EST_POINT_TO_POINT); p.max_iteration = -1
    refused(reg(m, p), "max_iteration")
    with P.registration.VoxelPointMap(P.PointCloud(clouds["target_xyz"]), MAP_VOXEL, 20) as bare, P.registration.VoxelPointMap(clouds["target"], MAP_VOXEL, 8) as m8, \
            P.registration.VoxelPointMap(clouds["target"], 0.5, 20) as fine:
        refused(reg(bare._open(), est(L.EST_POINT_TO_PLANE)), "normals")
        refused(lib.pcr_point_map_merge(ctx.handle, m, bare._open()), "normals")
        refused(lib.pcr_point_map_merge(ctx.handle, m, m8._open()), "max_points_per_voxel")
        refused(lib.pcr_point_map_merge(ctx.handle, m, fine._open()), "grid")
        refused(lib.pcr_point_map_merge(ctx.handle, m, m), "itself")
        refused(lib.pcr_point_map_insert(ctx.handle, m, xyz, None, n, None), "normals")
        refused(lib.pcr_point_map_insert(ctx.handle, bare._open(), xyz, clouds["target"].device_normals().data_ptr(), n, None), "normals")
    c3 = np.array([0.0, np.inf, 0.0])
    refused(lib.pcr_point_map_remove_far(ctx.handle, m, c3.ctypes.data_as(dp), C.c_double(5.0), None), "center3")
    refused(lib.pcr_point_map_remove_far(ctx.handle, m, g.ctypes.data_as(dp), C.c_double(-5.0), None), "max_distance")


# ------------------------------------------------------------------------------------------ odometry
def _step():
    a = np.deg2rad(1.0)
    S = np.eye(4)
    S[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
    S[:3, 3] = [0.2, 0.0, 0.0]
    return S


@pytest.fixture(scope="module")
def drive(P, clouds):
    """four scans of the 0.3 m target of pair 899 seen from poses that advance by 0.2 m and 1 degree: scan k = inv(P_k) world, float32 (the
    construction of the odometry test in tests/test_gpu_voxel_map_update.py)"""
    truth, scans = [np.eye(4)], []
    for k in range(4):
        if k:
            truth.append(truth[-1] @ _step())
        inv = np.linalg.inv(truth[k])
        pc = P.PointCloud((clouds["target_xyz"].astype(np.float64) @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32))
        pc.normals = (clouds["target_nrm"].astype(np.float64) @ inv[:3, :3].T).astype(np.float32)
        scans.append(pc)
    return truth, scans


@pytest.mark.parametrize("mode", ["fixed", "adaptive"])
def test_odometry_ends_closer_to_the_planted_poses_than_the_motion_model(P, drive, mode):
    """Under "static" the start of scan k is the pose of scan k - 1, one step (0.2 m, 1 degree) from the truth when that pose is right."""
    R = P.registration
    truth, scans = drive
    if mode == "fixed":
        poses, results, m = R.scan_to_map_odometry_icp(scans, MAP_VOXEL, 1.0, motion_model="static", max_points_per_voxel=10)
    else:
        th = R.AdaptiveThreshold(0.5, 0.01, 10.0)
        poses, results, m = R.scan_to_map_odometry_icp(scans, MAP_VOXEL, motion_model="static", max_points_per_voxel=10, adaptive_threshold=th)
        assert th.samples == 4 and 0.05 < th.sigma < 0.5               # three registrations a step from their prediction: three samples
    with m:
        assert len(poses) == len(results) == 4 and results[0] is None and np.array_equal(poses[0], np.eye(4))
        for k in range(1, 4):
            a0, d0 = pose_error(poses[k - 1], truth[k])
            a, d = pose_error(poses[k], truth[k])
            print(f"{mode} scan {k}: start {np.degrees(a0):.3f} deg {d0:.3f} m -> {np.degrees(a):.4f} deg {d:.4f} m after {results[k].iterations} iterations, fitness {results[k].fitness:.3f}")
            assert a < a0 and d < d0, (k, a, d, a0, d0)
        # the returned map is the restatement's after the same inserts
        g = R.VoxelPointMap.centered_grid_min(scans[0].get_center(), MAP_VOXEL)
        assert np.array_equal(m.grid_min, g)
        ref = pm.build_map(scans[0]._xyz.cpu().numpy(), scans[0]._nrm.cpu().numpy(), MAP_VOXEL, 10, g, np.eye(4))
        for k in range(1, 4):
            ref = pm.insert(ref, scans[k]._xyz.cpu().numpy(), scans[k]._nrm.cpu().numpy(), poses[k])
        _assert_map_equals(m, ref)
