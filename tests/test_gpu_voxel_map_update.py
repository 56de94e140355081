"""The voxel covariance map that grows, on the device against the numpy restatement of its rules (tests/voxel_map_update_reference.py): cells,
counts, means and covariances bit for bit after create-on-a-grid, insert, merge and remove_far; the rows and the registration against a grown
map; the refusals, each leaving the map as it was; and the odometry recipe.  Pair 899 with both clouds at voxel 0.3 on a 1.0 m grid centred on the
target's mean (the condition of these comparisons -- hundreds of cells of each kind -- is checked on the CPU in
tests/test_voxel_map_update_api.py), and maps of a few cells to a few hundred built cell by cell."""
import numpy as np
import pytest

import voxel_map_update_reference as vu
import voxel_reference as vr
import voxelized_gicp_reference as vg
from conftest import pkg, pose_error

pytestmark = pytest.mark.gpu

MAP_VOXEL = 1.0
MID = 1 << 20                        # the cell of the point (0, 0, 0) on the grid centred on it


@pytest.fixture(scope="module")
def P():
    return pkg()


@pytest.fixture(scope="module")
def M(P):
    return P.registration.VoxelCovarianceMap


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
        out[key + "_cov6"] = vg.cov6_from_normals(out[key + "_nrm"])
    assert (len(out["source"]), len(out["target"])) == (6897, 7074)
    out["grid_min"] = vu.centered_grid_min(out["target_xyz"].astype(np.float64).mean(0), MAP_VOXEL)
    return out


@pytest.fixture(scope="module")
def refs(clouds, small_pair):
    """the restatement's maps, computed once and left unchanged"""
    g, T = clouds["grid_min"], small_pair["T_gicp"]
    t = vu.build_map_on_grid(clouds["target_xyz"], clouds["target_cov6"], MAP_VOXEL, g)
    s = vu.build_map_on_grid(clouds["source_xyz"], clouds["source_cov6"], MAP_VOXEL, g, T)
    s_id = vu.build_map_on_grid(clouds["source_xyz"], clouds["source_cov6"], MAP_VOXEL, g)
    return {"target": t, "source": s, "source_id": s_id, "merged": vu.merge(t, s)}


def _assert_map_equals(dev, ref):
    assert len(dev) == len(ref.cells)
    assert np.array_equal(dev.cells, ref.cells)                       # the same cells in the same (Morton) order
    assert np.array_equal(dev.counts, ref.count)
    assert vr.bits_equal(dev.points, ref.mean)
    assert vr.bits_equal(dev.covariances, ref.cov6)


def _state(dev):
    return len(dev), dev.cells.tobytes(), dev.counts.tobytes(), dev.points.tobytes(), dev.covariances.tobytes()


def _grown(M, clouds, small_pair):
    m = M.on_grid(clouds["target"], MAP_VOXEL, grid_min=clouds["grid_min"])
    m.insert(clouds["source"], small_pair["T_gicp"])
    return m


# ------------------------------------------------------------------------------------------ create on a grid
def test_create_on_the_centred_grid(M, clouds, refs):
    with M.on_grid(clouds["target"], MAP_VOXEL, grid_min=clouds["grid_min"]) as dev:
        _assert_map_equals(dev, refs["target"])
        assert np.array_equal(dev.grid_min, clouds["grid_min"]) and np.array_equal(dev.origin, refs["target"].origin) and dev.voxel_size == MAP_VOXEL
        assert dev.cells.min() > MID - 200 and dev.cells.max() < MID + 200          # all 63 key bits are in play


def test_create_on_the_clouds_own_grid_is_todays_map(M, clouds):
    own = clouds["target_xyz"].astype(np.float64).min(0)
    with M(clouds["target"], MAP_VOXEL) as today, M.on_grid(clouds["target"], MAP_VOXEL, grid_min=own) as dev, M.on_grid(clouds["target"], MAP_VOXEL) as plain:
        assert _state(dev) == _state(today) == _state(plain) and len(dev) > 1000
        for m in (dev, plain):
            assert np.array_equal(m.grid_min, today.grid_min) and np.array_equal(m.origin, today.origin)
        assert np.array_equal(today.grid_min, own) and np.array_equal(today.origin, own - 0.5)


def test_create_at_a_pose_from_normals_and_from_covariances(P, M, clouds, refs, small_pair):
    T = small_pair["T_gicp"]
    with M.on_grid(clouds["source"], MAP_VOXEL, grid_min=clouds["grid_min"], transformation=T) as dev:
        _assert_map_equals(dev, refs["source"])
    rng = np.random.default_rng(2)
    a = rng.normal(size=(len(clouds["source"]), 3, 3))
    cov6 = vg.cov6_of(a @ a.transpose(0, 2, 1)).astype(np.float32)          # full covariances: every entry of (R C) R^T has three non-zero terms
    pc = P.PointCloud(clouds["source_xyz"])
    pc.covariances = cov6
    ref = vu.build_map_on_grid(clouds["source_xyz"], cov6, MAP_VOXEL, clouds["grid_min"], T)
    with M.on_grid(pc, MAP_VOXEL, grid_min=clouds["grid_min"], transformation=T) as dev:
        _assert_map_equals(dev, ref)


# ------------------------------------------------------------------------------------------ insert
def test_insert_at_a_pose_and_again(M, clouds, refs, small_pair):
    T = small_pair["T_gicp"]
    with _grown(M, clouds, small_pair) as dev:
        _assert_map_equals(dev, refs["merged"])
        dev.insert(clouds["source"], T)
        twice = vu.insert(refs["merged"], clouds["source_xyz"], clouds["source_cov6"], T)
        _assert_map_equals(dev, twice)
        # the scan's cells: N_t + 2 N_s members now
        rows = twice.lex_row[np.searchsorted(twice.lex_keys, vr.cell_key(refs["source"].cells))]
        before = refs["merged"].lex_row[np.searchsorted(refs["merged"].lex_keys, vr.cell_key(refs["source"].cells))]
        assert np.array_equal(dev.counts[rows], refs["merged"].count[before] + refs["source"].count)


def test_insert_with_the_identity_is_the_merge_of_the_two_maps(M, clouds, refs):
    want = vu.merge(refs["target"], refs["source_id"])
    g = clouds["grid_min"]
    with M.on_grid(clouds["target"], MAP_VOXEL, grid_min=g) as a, M.on_grid(clouds["target"], MAP_VOXEL, grid_min=g) as b, \
            M.on_grid(clouds["source"], MAP_VOXEL, grid_min=g) as s:
        a.insert(clouds["source"])
        b.merge(s)
        _assert_map_equals(a, want)
        _assert_map_equals(b, want)
        _assert_map_equals(s, refs["source_id"])


# ------------------------------------------------------------------------------------------ merge
GRID0 = vu.centered_grid_min([0.0, 0.0, 0.0], 1.0)


def _cell_cloud(cells, seed):
    """one to three float32 points in each of the given cells of the grid centred on (0, 0, 0), with full random covariances"""
    rng = np.random.default_rng(seed)
    cells = np.asarray(cells, np.int64).reshape(-1, 3)
    cop = np.repeat(cells, rng.integers(1, 4, len(cells)), 0)
    cop = cop[rng.permutation(len(cop))]
    xyz = ((cop - MID).astype(np.float64) + rng.uniform(-0.4, 0.4, cop.shape)).astype(np.float32)
    a = rng.normal(size=(len(xyz), 3, 3))
    return xyz, vg.cov6_of(a @ a.transpose(0, 2, 1)).astype(np.float32)


def _block(nx, ny, nz, lo=(MID, MID, MID)):
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 3)
    return g + np.asarray(lo, np.int64)


def _boundary_case(n):
    """n rows on each side; the first and the last cell of the union (in Morton order) are in both, the cells between alternate"""
    pool = _block(9, 8, 8)
    pool = pool[np.argsort(vr.morton3(pool))][:2 * n - 2]
    ends, mid = pool[[0, -1]], pool[1:-1]
    return np.concatenate([ends, mid[0::2]]), np.concatenate([ends, mid[1::2]])


def _interleaved():
    rng = np.random.default_rng(40)
    pool = _block(6, 6, 6, (MID - 3, MID - 3, MID - 3))              # straddles the top key bit on every axis
    pick = rng.random((2, len(pool))) < 0.5
    return pool[pick[0]], pool[pick[1]]


C0 = np.array([[MID + 2, MID + 1, MID + 3]])
MERGE_CASES = {
    "same_cell": lambda: (C0, C0),
    "lower_cell": lambda: (C0, C0 - [1, 0, 0]),
    "higher_cell": lambda: (C0, C0 + [1, 0, 0]),
    "wholly_below": lambda: (_block(4, 3, 3), _block(4, 3, 3, (MID - 4, MID, MID))),      # the top bit of x is clear in every cell of `other`
    "wholly_above": lambda: (_block(4, 3, 3, (MID - 4, MID, MID)), _block(4, 3, 3)),
    "interleaved": _interleaved,
    "rows255": lambda: _boundary_case(255),
    "rows256": lambda: _boundary_case(256),
    "rows257": lambda: _boundary_case(257),
}


@pytest.mark.parametrize("name", list(MERGE_CASES))
def test_merge_in_both_orders(P, M, name):
    ca, cb = MERGE_CASES[name]()
    (xa, va), (xb, vb) = _cell_cloud(ca, 50), _cell_cloud(cb, 51)
    ra, rb = vu.build_map_on_grid(xa, va, 1.0, GRID0), vu.build_map_on_grid(xb, vb, 1.0, GRID0)
    assert np.array_equal(np.unique(vr.cell_key(ra.cells)), np.unique(vr.cell_key(ca))) and np.array_equal(np.unique(vr.cell_key(rb.cells)), np.unique(vr.cell_key(cb)))
    ka, kb = vr.morton3(ra.cells), vr.morton3(rb.cells)
    if name == "wholly_below":
        assert kb.max() < ka.min()
    if name == "wholly_above":
        assert kb.min() > ka.max()
    if name.startswith("rows"):
        n = int(name[4:])
        assert len(ka) == len(kb) == n and ka[0] == kb[0] and ka[-1] == kb[-1] and len(np.intersect1d(ka, kb)) == 2
    if name == "interleaved":
        shared = len(np.intersect1d(ka, kb))
        assert shared > 20 and len(ka) - shared > 20 and len(kb) - shared > 20
    want = vu.merge(ra, rb)

    def dev(xyz, cov6):
        pc = P.PointCloud(xyz)
        pc.covariances = cov6
        return M.on_grid(pc, 1.0, grid_min=GRID0)
    with dev(xa, va) as a, dev(xb, vb) as b, dev(xa, va) as a2, dev(xb, vb) as b2:
        _assert_map_equals(a, ra)
        _assert_map_equals(b, rb)
        other = _state(b)
        a.merge(b)
        _assert_map_equals(a, want)
        assert _state(b) == other                                      # `other` is unchanged
        b2.merge(a2)
        _assert_map_equals(b2, vu.merge(rb, ra))
        assert _state(b2) == _state(a)                                 # commutative bit for bit
        rows = a.correspondences(P.PointCloud(xb), np.eye(4), 1).cpu().numpy()      # the new cell hash finds every cell of `other`
        assert np.array_equal(rows, vg.rows_at(want, xb, np.eye(4), 1)) and len(rows) == len(xb)


# ------------------------------------------------------------------------------------------ remove_far
def test_remove_far(M, clouds, refs, small_pair):
    ref = refs["merged"]
    centre = ref.mean.astype(np.float64).mean(0)
    d2 = np.sort(vu.distance2(ref.mean, centre))
    outside = ref.mean.astype(np.float64).max(0) + 30.0
    d2o = np.sort(vu.distance2(ref.mean, outside))
    cases = {"half": (centre, float(np.sqrt(np.median(d2)))), "centre_outside": (outside, float(np.sqrt(d2o[len(d2o) // 4]))),
             "one_row": (centre, float(np.sqrt(0.5 * (d2[0] + d2[1]))))}
    for name, (c, r) in cases.items():
        want = vu.remove_far(ref, c, r)
        with _grown(M, clouds, small_pair) as dev:
            removed = dev.remove_far(c, r)
            assert removed == len(ref.cells) - len(want.cells) and removed > 0, name
            _assert_map_equals(dev, want)
            rows = dev.correspondences(clouds["target"], np.eye(4), 1).cpu().numpy()
            assert np.array_equal(rows, vg.rows_at(want, clouds["target_xyz"], np.eye(4), 1)), name
    assert 0.4 < len(vu.remove_far(ref, *cases["half"]).cells) / len(ref.cells) < 0.6
    assert 0 < len(vu.remove_far(ref, *cases["centre_outside"]).cells) < len(ref.cells) / 2
    assert len(vu.remove_far(ref, *cases["one_row"]).cells) == 1
    with _grown(M, clouds, small_pair) as dev:                         # a radius that keeps everything changes nothing
        assert dev.remove_far(centre, 1e4) == 0
        _assert_map_equals(dev, ref)


# ------------------------------------------------------------------------------------------ registration against a grown map
def test_rows_and_registration_against_a_grown_map(P, M, clouds, refs, small_pair):
    R = P.registration
    ref, T0 = refs["merged"], small_pair["T_fgr"]
    with _grown(M, clouds, small_pair) as dev:
        for nbh in (1, 7, 27):
            got = dev.correspondences(clouds["source"], T0, nbh).cpu().numpy()
            want = vg.rows_at(ref, clouds["source_xyz"], T0, nbh)
            assert len(want) > 1000 and np.array_equal(got, want), nbh
        loop = vg.loop(ref, clouds["source_xyz"], clouds["source_cov6"], T0, 1, 1, 0, 1.0, max_it=5)
        res = R.registration_voxelized_gicp(clouds["source"], dev, None, T0, R.TransformationEstimationForGeneralizedICP(R.L2Loss()),
                                            R.ICPConvergenceCriteria(1e-6, 1e-6, 5), 1, 1)
        ang, dt = pose_error(res.transformation, loop.transformation)
        print(f"grown map, l2 nbh 1, 5 iterations: {ang:.2e} rad {dt:.2e} m, iterations {res.iterations} / {loop.iterations}, rows {len(res.correspondence_set)} / {loop.n_rows}")
        assert ang < 1e-7 and dt < 1e-6, (ang, dt)                     # the L2 bound of tests/test_gpu_voxelized_gicp.py::test_trajectory_matches_reference
        assert res.iterations == loop.iterations and res.converged == loop.converged
        assert len(res.correspondence_set) == loop.n_rows


# ------------------------------------------------------------------------------------------ refusals
def _refused(dev, call, match):
    before = _state(dev)
    with pytest.raises(RuntimeError, match=match):
        call()
    assert _state(dev) == before


def test_refusals_leave_the_map_as_it_was(P, M, clouds, small_pair):
    T = small_pair["T_gicp"]
    g = clouds["grid_min"]
    with M(clouds["target"], MAP_VOXEL) as own:                       # the target's own grid: the placed source reaches below its origin
        _refused(own, lambda: own.insert(clouds["source"], T), "outside the map's grid")
    with M.on_grid(clouds["target"], MAP_VOXEL, grid_min=g) as dev:
        with M.on_grid(clouds["source"], 2.0, grid_min=g) as other:
            _refused(dev, lambda: dev.merge(other), "not on the map's grid")
        with M.on_grid(clouds["source"], MAP_VOXEL, grid_min=g + [MAP_VOXEL, 0.0, 0.0]) as other:
            _refused(dev, lambda: dev.merge(other), "not on the map's grid")
        _refused(dev, lambda: dev.merge(dev), "itself")
        _refused(dev, lambda: dev.remove_far([1e5, 0.0, 0.0], 1.0), "would leave the map empty")
        bad = np.array(T)
        bad[1, 2] = np.nan
        _refused(dev, lambda: dev.insert(clouds["source"], bad), "T holds a non-finite")
        bad[1, 2] = np.inf
        _refused(dev, lambda: dev.insert(clouds["source"], bad), "T holds a non-finite")
        far = np.eye(4)
        far[0, 3] = 3e6                                                # past the upper end of the grid
        _refused(dev, lambda: dev.insert(clouds["source"], far), "outside the map's grid")
        with pytest.raises(RuntimeError, match="T holds a non-finite"):
            M.on_grid(clouds["source"], MAP_VOXEL, grid_min=g, transformation=bad)
        with pytest.raises(RuntimeError, match="grid_min3 holds a non-finite"):
            M.on_grid(clouds["source"], MAP_VOXEL, grid_min=[0.0, np.nan, 0.0])


def test_counts_past_int32_are_refused(P, M):
    """two one-cell maps merged into each other in turn: the counts run through the Fibonacci numbers, 45 merges to pass 2^31 - 1"""
    pc = P.PointCloud(np.array([[0.25, 0.25, 0.25]], np.float32))
    pc.covariances = np.array([[1, 0, 0, 1, 0, 1]], np.float32)
    with M.on_grid(pc, 1.0, grid_min=GRID0) as x, M.on_grid(pc, 1.0, grid_min=GRID0) as y:
        nx = ny = 1
        merges = 0
        while nx + ny <= vu.COUNT_MAX:
            x.merge(y)
            nx += ny
            x, y, nx, ny = y, x, ny, nx
            merges += 1
        assert merges > 40 and x.counts[0] == nx and y.counts[0] == ny and len(x) == len(y) == 1
        assert vr.bits_equal(x.points, pc._xyz.cpu().numpy())          # (equal means stay what they are: N_a a + N_b a = N a exactly below 2^29, rounded above)
        _refused(x, lambda: x.merge(y), r"2\^31 - 1")
        assert y.counts[0] == ny


def test_use_after_close_raises(M, clouds):
    m = M.on_grid(clouds["target"], MAP_VOXEL, grid_min=clouds["grid_min"])
    with M.on_grid(clouds["source"], MAP_VOXEL, grid_min=clouds["grid_min"]) as live:
        m.close()
        before = _state(live)
        for call in (lambda: m.insert(clouds["source"]), lambda: m.merge(live), lambda: live.merge(m), lambda: m.remove_far([0, 0, 0], 1.0), lambda: m.grid_min,
                     lambda: m.origin):
            with pytest.raises(RuntimeError, match="closed"):
                call()
        assert _state(live) == before


# ------------------------------------------------------------------------------------------ odometry
def _step():
    a = np.deg2rad(1.0)
    S = np.eye(4)
    S[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
    S[:3, 3] = [0.2, 0.0, 0.0]
    return S


@pytest.fixture(scope="module")
def drive(P, clouds):
    """four scans of the 0.3 m target of pair 899 seen from poses that advance by 0.2 m and 1 degree: scan k = inv(P_k) world, float32"""
    truth, scans = [np.eye(4)], []
    for k in range(4):
        if k:
            truth.append(truth[-1] @ _step())
        inv = np.linalg.inv(truth[k])
        pc = P.PointCloud((clouds["target_xyz"].astype(np.float64) @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32))
        pc.normals = (clouds["target_nrm"].astype(np.float64) @ inv[:3, :3].T).astype(np.float32)
        scans.append(pc)
    return truth, scans


@pytest.mark.parametrize("model,max_range", [("constant_velocity", None), ("static", 25.0)])
def test_odometry_is_the_public_calls_by_hand(P, M, drive, model, max_range):
    R = P.registration
    _, scans = drive
    poses, results, m = R.scan_to_map_odometry(scans, MAP_VOXEL, motion_model=model, max_range=max_range)
    with m:
        assert len(poses) == len(results) == 4 and results[0] is None and np.array_equal(poses[0], np.eye(4))
        g = M.centered_grid_min(scans[0].get_center(), MAP_VOXEL)
        assert np.array_equal(m.grid_min, g)
        with M.on_grid(scans[0], MAP_VOXEL, 1e-3, g, np.eye(4)) as hand:
            by_hand = [np.eye(4)]
            for k in range(1, 4):
                start = by_hand[-1]
                if model == "constant_velocity" and k >= 2:
                    start = by_hand[-1] @ np.linalg.inv(by_hand[-2]) @ by_hand[-1]
                res = R.registration_voxelized_gicp(scans[k], hand, None, start)
                by_hand.append(res.transformation)
                hand.insert(scans[k], res.transformation)
                if max_range is not None:
                    hand.remove_far(res.transformation[:3, 3], max_range)
            for k in range(4):
                assert np.array_equal(poses[k], by_hand[k]), k         # bit for bit
            assert _state(hand) == _state(m)
        if max_range is not None:
            d2 = vu.distance2(m.points, poses[-1][:3, 3])
            assert (d2 < max_range * max_range).all() and len(m) > 100
            with M.on_grid(scans[0], MAP_VOXEL, 1e-3, g, np.eye(4)) as whole:
                assert len(m) < len(whole)                              # something was in fact out of range


def test_odometry_poses_are_closer_to_the_truth_than_their_starts(P, drive):
    """Under "static" the start of scan k is the pose of scan k - 1, one step (0.2 m, 1 degree) from the truth when that pose is right.  (Under
    "constant_velocity" with this exactly constant motion the start of scans 2 and 3 is the truth up to the estimator's own error, and the
    comparison would set one such error against another.)"""
    truth, scans = drive
    poses, results, m = P.registration.scan_to_map_odometry(scans, MAP_VOXEL, motion_model="static")
    m.close()
    for k in range(1, 4):
        a0, d0 = pose_error(poses[k - 1], truth[k])
        a, d = pose_error(poses[k], truth[k])
        print(f"scan {k}: start {np.degrees(a0):.3f} deg {d0:.3f} m -> {np.degrees(a):.4f} deg {d:.4f} m after {results[k].iterations} iterations, fitness {results[k].fitness:.3f}")
        assert a < a0 and d < d0, (k, a, d, a0, d0)
