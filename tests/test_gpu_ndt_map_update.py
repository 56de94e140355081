"""The normal-distributions map that grows, on the device against the numpy restatement of its rules (tests/ndt_map_update_reference.py): cells,
counts, means, C_v and validity bit for bit and A_v within 1e-10 of its Frobenius norm (the bound of tests/test_gpu_ndt.py) after
create-on-a-grid, insert, merge and remove_far; the rows, the sums and the registration against a grown map; the refusals, each leaving the map
as it was; and the odometry recipe.  Pair 899 with both clouds at voxel 0.3 on a 2.0 m grid centred on the target's mean, and the hand-made maps
of tests/ndt_map_update_cases.py (the conditions of these comparisons are checked on the CPU in tests/test_ndt_map_update_api.py)."""
import numpy as np
import pytest

import ndt_map_update_cases as cases
import ndt_map_update_reference as nu
import ndt_reference as nd
import voxel_reference as vr
import voxelized_gicp_reference as vg
from conftest import pkg, pose_error

pytestmark = pytest.mark.gpu

MAP_VOXEL = 2.0
MIN_POINTS = 6


@pytest.fixture(scope="module")
def P():
    return pkg()


@pytest.fixture(scope="module")
def M(P):
    return P.registration.NormalDistributionsMap


@pytest.fixture(scope="module")
def clouds(P, small_pair):
    """pair 899 at voxel 0.3 (6897 / 7074 points), nothing per point; the float32 arrays the device holds are what the reference gets"""
    out = {}
    for key in ("source", "target"):
        pc = P.PointCloud(small_pair[key]).voxel_down_sample(0.3)
        out[key] = pc
        out[key + "_xyz"] = pc._xyz.cpu().numpy()
    assert (len(out["source"]), len(out["target"])) == (6897, 7074)
    out["grid_min"] = nu.centered_grid_min(out["target_xyz"].astype(np.float64).mean(0), MAP_VOXEL)
    return out


@pytest.fixture(scope="module")
def refs(clouds, small_pair):
    """the restatement's maps, computed once and left unchanged"""
    g, T = clouds["grid_min"], small_pair["T_gicp"]
    t = nu.build_map_on_grid(clouds["target_xyz"], MAP_VOXEL, g)
    s = nu.build_map_on_grid(clouds["source_xyz"], MAP_VOXEL, g, T)
    s_id = nu.build_map_on_grid(clouds["source_xyz"], MAP_VOXEL, g)
    return {"target": t, "source": s, "source_id": s_id, "merged": nu.merge(t, s)}


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
    assert np.array_equal(dev.origin, ref.origin) and dev.voxel_size == ref.voxel and np.array_equal(dev.grid_min, ref.grid_min)


def _state(dev):
    return len(dev), dev.cells.tobytes(), dev.counts.tobytes(), dev.points.tobytes(), dev.covariances.tobytes(), dev.valid.tobytes(), dev.information.tobytes()


def _grown(M, clouds, small_pair):
    m = M.on_grid(clouds["target"], MAP_VOXEL, grid_min=clouds["grid_min"])
    m.insert(clouds["source"], small_pair["T_gicp"])
    return m


# ------------------------------------------------------------------------------------------ create on a grid
def test_create_on_the_centred_grid(M, clouds, refs):
    with M.on_grid(clouds["target"], MAP_VOXEL, grid_min=clouds["grid_min"]) as dev:
        _assert_map_equals(dev, refs["target"])
        assert dev.cells.min() > cases.MID - 200 and dev.cells.max() < cases.MID + 200          # all 63 key bits are in play
        assert dev.min_points_per_voxel == 6 and dev.eigenvalue_ratio == 0.01


def test_create_on_the_clouds_own_grid_is_todays_map(M, clouds):
    own = clouds["target_xyz"].astype(np.float64).min(0)
    with M(clouds["target"], MAP_VOXEL) as today, M.on_grid(clouds["target"], MAP_VOXEL, grid_min=own) as dev, M.on_grid(clouds["target"], MAP_VOXEL) as plain:
        assert _state(dev) == _state(today) == _state(plain) and len(dev) == 733          # A_v bits included
        for m in (dev, plain):
            assert np.array_equal(m.grid_min, today.grid_min) and np.array_equal(m.origin, today.origin)
        assert np.array_equal(today.grid_min, own) and np.array_equal(today.origin, own - 1.0)
        _assert_map_equals(dev, nu.build_map_on_grid(clouds["target_xyz"], MAP_VOXEL, own))


def test_create_at_a_pose_and_with_other_thresholds(M, clouds, refs, small_pair):
    T = small_pair["T_gicp"]
    with M.on_grid(clouds["source"], MAP_VOXEL, grid_min=clouds["grid_min"], transformation=T) as dev:
        _assert_map_equals(dev, refs["source"])
    ref = nu.build_map_on_grid(clouds["source_xyz"], MAP_VOXEL, clouds["grid_min"], T, 2, 1.0)
    with M.on_grid(clouds["source"], MAP_VOXEL, 2, 1.0, clouds["grid_min"], T) as dev:
        _assert_map_equals(dev, ref)


# ------------------------------------------------------------------------------------------ insert
def test_insert_at_a_pose_and_again(M, clouds, refs, small_pair):
    T = small_pair["T_gicp"]
    with _grown(M, clouds, small_pair) as dev:
        _assert_map_equals(dev, refs["merged"])
        assert refs["merged"].valid.sum() > refs["target"].valid.sum() + 50          # cells become valid through the insert
        dev.insert(clouds["source"], T)
        twice = nu.insert(refs["merged"], clouds["source_xyz"], T)
        _assert_map_equals(dev, twice)
        # the scan's cells: N_t + 2 N_s members now
        rows = twice.base.lex_row[np.searchsorted(twice.base.lex_keys, vr.cell_key(refs["source"].cells))]
        before = refs["merged"].base.lex_row[np.searchsorted(refs["merged"].base.lex_keys, vr.cell_key(refs["source"].cells))]
        assert np.array_equal(dev.counts[rows], refs["merged"].count[before] + refs["source"].count)


def test_insert_with_the_identity_is_the_merge_of_the_two_maps(M, clouds, refs):
    want = nu.merge(refs["target"], refs["source_id"])
    g = clouds["grid_min"]
    with M.on_grid(clouds["target"], MAP_VOXEL, grid_min=g) as a, M.on_grid(clouds["target"], MAP_VOXEL, grid_min=g) as b, \
            M.on_grid(clouds["source"], MAP_VOXEL, grid_min=g) as s, M.on_grid(clouds["target"], MAP_VOXEL, grid_min=g) as c:
        a.insert(clouds["source"])
        b.merge(s)
        c.insert(clouds["source"], np.eye(4))
        _assert_map_equals(a, want)
        _assert_map_equals(s, refs["source_id"])
        assert _state(a) == _state(b) == _state(c)


# ------------------------------------------------------------------------------------------ merge
@pytest.mark.parametrize("name", list(cases.MERGE_CASES))
def test_merge_in_both_orders(P, M, name):
    _, _, xa, xb = cases.merge_case(name)
    ra, rb = (nu.build_map_on_grid(x, 1.0, cases.GRID0, None, MIN_POINTS, 0.01) for x in (xa, xb))
    want = nu.merge(ra, rb)

    def dev(xyz):
        return M.on_grid(P.PointCloud(xyz), 1.0, MIN_POINTS, 0.01, cases.GRID0)
    with dev(xa) as a, dev(xb) as b, dev(xa) as a2, dev(xb) as b2:
        _assert_map_equals(a, ra)
        _assert_map_equals(b, rb)
        other = _state(b)
        a.merge(b)
        _assert_map_equals(a, want)
        assert _state(b) == other                                      # `other` is unchanged
        b2.merge(a2)
        _assert_map_equals(b2, nu.merge(rb, ra))
        assert _state(b2) == _state(a)                                 # commutative bit for bit, A_v included
        # a cell in only one map keeps its row bit for bit, A_v included
        ka, km = vr.cell_key(ra.cells), vr.cell_key(want.cells)
        only_a = ~np.isin(ka, vr.cell_key(rb.cells))
        with dev(xa) as fresh:
            order = np.argsort(km, kind="stable")
            row_of = order[np.searchsorted(km[order], ka[only_a])]
            assert np.array_equal(a.information[row_of], fresh.information[only_a]) and np.array_equal(a.covariances[row_of], fresh.covariances[only_a])
        # the new cell hash finds every cell: each point of either cloud lands in its own cell's row when that cell is valid
        for xyz in (xa, xb):
            rows = a.correspondences(P.PointCloud(xyz), np.eye(4), 1).cpu().numpy()
            assert np.array_equal(rows, nd.rows_at(want, xyz, np.eye(4), 1))
        rows = a.correspondences(P.PointCloud(np.concatenate([xa, xb])), np.eye(4), 27).cpu().numpy()
        assert np.array_equal(rows, nd.rows_at(want, np.concatenate([xa, xb]), np.eye(4), 27))


# ------------------------------------------------------------------------------------------ remove_far
def test_remove_far(M, clouds, refs, small_pair):
    ref = refs["merged"]
    centre = ref.mean.astype(np.float64).mean(0)
    d2 = np.sort(nu.distance2(ref.mean, centre))
    outside = ref.mean.astype(np.float64).max(0) + 30.0
    d2o = np.sort(nu.distance2(ref.mean, outside))
    todo = {"half": (centre, float(np.sqrt(np.median(d2)))), "centre_outside": (outside, float(np.sqrt(d2o[len(d2o) // 4]))),
            "one_row": (centre, float(np.sqrt(0.5 * (d2[0] + d2[1]))))}
    with _grown(M, clouds, small_pair) as whole:
        info = whole.information
    for name, (c, r) in todo.items():
        want = nu.remove_far(ref, c, r)
        with _grown(M, clouds, small_pair) as dev:
            removed = dev.remove_far(c, r)
            assert removed == len(ref.cells) - len(want.cells) and removed > 0, name
            _assert_map_equals(dev, want)
            assert np.array_equal(dev.information, info[nu.distance2(ref.mean, c) < r * r]), name          # kept rows keep all their bits
            rows = dev.correspondences(clouds["target"], np.eye(4), 1).cpu().numpy()
            assert np.array_equal(rows, nd.rows_at(want, clouds["target_xyz"], np.eye(4), 1)), name
    assert 0.4 < len(nu.remove_far(ref, *todo["half"]).cells) / len(ref.cells) < 0.6
    assert 0 < len(nu.remove_far(ref, *todo["centre_outside"]).cells) < len(ref.cells) / 2
    assert len(nu.remove_far(ref, *todo["one_row"]).cells) == 1
    with _grown(M, clouds, small_pair) as dev:                         # a radius that keeps everything changes nothing
        before = _state(dev)
        assert dev.remove_far(centre, 1e4) == 0
        assert _state(dev) == before


# ------------------------------------------------------------------------------------------ rows and sums against a grown map
def _assert_linearization(got, ref, what=""):
    """rows and points exactly; every sum within 1e-9 x the sum of the magnitudes of its terms (the bound of tests/test_gpu_ndt.py)"""
    assert (got.rows, got.points_with_rows) == (ref.rows, ref.points_with_rows), what
    worst = 0.0
    for name, g, r in (("JTJ", got.JTJ, ref.JTJ), ("JTr", got.JTr, ref.JTr), ("score", got.score, ref.score), ("sum_d2", got.sum_d2, ref.sum_d2)):
        err, mag = np.abs(np.asarray(g) - np.asarray(r)), np.asarray(ref.mag[name])
        worst = max(worst, float((err / np.maximum(mag, 1e-300)).max()))
        assert (err <= 1e-9 * mag).all(), (what, name, err, mag)
    print(f"linearize {what}: rows {got.rows}, score {got.score:.6f}, worst error / sum of magnitudes {worst:.2e}")


def test_rows_sums_and_registration_against_a_grown_map(P, M, clouds, refs, small_pair):
    R = P.registration
    ref, T0 = refs["merged"], small_pair["T_fgr"]
    with _grown(M, clouds, small_pair) as dev:
        for nbh in (1, 7, 27):
            got = dev.correspondences(clouds["source"], T0, nbh).cpu().numpy()
            want = nd.rows_at(ref, clouds["source_xyz"], T0, nbh)
            assert len(want) > 1000 and np.array_equal(got, want), nbh
            _assert_linearization(dev.linearize(clouds["source"], T0, nbh), nd.linearize(ref, clouds["source_xyz"], T0, want), f"grown map, nbh {nbh}")
        loop = nd.loop(ref, clouds["source_xyz"], T0, 7, max_it=5)
        res = R.registration_ndt(clouds["source"], dev, None, T0, R.ICPConvergenceCriteria(1e-6, 1e-6, 5), 7)
        ang, dt = pose_error(res.transformation, loop.transformation)
        print(f"grown map, nbh 7, 5 iterations: {ang:.2e} rad {dt:.2e} m, iterations {res.iterations} / {loop.iterations}, rows {len(res.correspondence_set)} / {loop.n_rows}")
        assert ang < 1e-7 and dt < 1e-6, (ang, dt)                     # the bound of tests/test_gpu_ndt.py::test_trajectory_matches_reference
        assert res.iterations == loop.iterations and res.converged == loop.converged
        assert len(res.correspondence_set) == loop.n_rows
        assert np.array_equal(res.correspondence_set, nd.rows_at(ref, clouds["source_xyz"], res.transformation, 7))


# ------------------------------------------------------------------------------------------ refusals
def _refused(dev, call, match):
    before = _state(dev)
    with pytest.raises(RuntimeError, match=match):
        call()
    assert _state(dev) == before


def test_refusals_leave_the_map_as_it_was(P, M, clouds, small_pair):
    T = small_pair["T_gicp"]
    g = clouds["grid_min"]
    with M(clouds["target"], MAP_VOXEL) as own:                       # the target's own grid: a source pushed 10 m down the x axis reaches below its origin
        low = np.array(T)
        low[0, 3] -= 10.0
        assert vg.transform(clouds["source_xyz"], low)[:, 0].min() < own.origin[0] - MAP_VOXEL
        _refused(own, lambda: own.insert(clouds["source"], low), "outside the map's grid")
    with M.on_grid(clouds["target"], MAP_VOXEL, grid_min=g) as dev:
        with M.on_grid(clouds["source"], 4.0, grid_min=g) as other:         # another voxel size (on this grid_min the clouds sit near cell 2^19)
            _refused(dev, lambda: dev.merge(other), "not on the map's grid")
        with M.on_grid(clouds["source"], MAP_VOXEL, grid_min=g + [MAP_VOXEL, 0.0, 0.0]) as other:
            _refused(dev, lambda: dev.merge(other), "not on the map's grid")
        with M.on_grid(clouds["source"], MAP_VOXEL, 5, grid_min=g) as other:
            _refused(dev, lambda: dev.merge(other), "min_points_per_voxel and eigenvalue_ratio")
        with M.on_grid(clouds["source"], MAP_VOXEL, 6, 0.02, grid_min=g) as other:
            _refused(dev, lambda: dev.merge(other), "min_points_per_voxel and eigenvalue_ratio")
        _refused(dev, lambda: dev.merge(dev), "itself")
        _refused(dev, lambda: dev.remove_far([1e5, 0.0, 0.0], 1.0), "would leave the map empty")
        _refused(dev, lambda: dev.remove_far([0.0, np.nan, 0.0], 1.0), "center3 holds a non-finite")
        bad = np.array(T)
        bad[1, 2] = np.nan
        _refused(dev, lambda: dev.insert(clouds["source"], bad), "T holds a non-finite")
        bad[1, 2] = np.inf
        _refused(dev, lambda: dev.insert(clouds["source"], bad), "T holds a non-finite")
        far = np.eye(4)
        far[0, 3] = 5e6                                                # past the upper end of the grid
        _refused(dev, lambda: dev.insert(clouds["source"], far), "outside the map's grid")
        far[0, 3] = -5e6                                               # below its origin
        _refused(dev, lambda: dev.insert(clouds["source"], far), "outside the map's grid")
        with pytest.raises(RuntimeError, match="outside the map's grid"):
            M.on_grid(clouds["source"], MAP_VOXEL, grid_min=g, transformation=far)
        with pytest.raises(RuntimeError, match="T holds a non-finite"):
            M.on_grid(clouds["source"], MAP_VOXEL, grid_min=g, transformation=bad)
        with pytest.raises(RuntimeError, match="grid_min3 holds a non-finite"):
            M.on_grid(clouds["source"], MAP_VOXEL, grid_min=[0.0, np.nan, 0.0])


def test_counts_past_int32_are_refused(P, M):
    """two one-cell maps merged into each other in turn: the counts run through the Fibonacci numbers, 45 merges to pass 2^31 - 1.  The members
    coincide, so the cell stays invalid with C = 0 exactly whatever its count"""
    pc = P.PointCloud(np.array([[0.25, 0.25, 0.25]], np.float32))
    with M.on_grid(pc, 1.0, grid_min=cases.GRID0) as x, M.on_grid(pc, 1.0, grid_min=cases.GRID0) as y:
        nx = ny = 1
        merges = 0
        while nx + ny <= nu.COUNT_MAX:
            x.merge(y)
            nx += ny
            x, y, nx, ny = y, x, ny, nx
            merges += 1
        assert merges > 40 and x.counts[0] == nx and y.counts[0] == ny and len(x) == len(y) == 1
        assert vr.bits_equal(x.points, pc._xyz.cpu().numpy()) and not x.covariances.any() and not x.valid[0] and not x.information.any()
        _refused(x, lambda: x.merge(y), r"2\^31 - 1")
        assert y.counts[0] == ny


def test_use_after_close_raises(M, clouds):
    m = M.on_grid(clouds["target"], MAP_VOXEL, grid_min=clouds["grid_min"])
    with M.on_grid(clouds["source"], MAP_VOXEL, grid_min=clouds["grid_min"]) as live:
        m.close()
        before = _state(live)
        for call in (lambda: m.insert(clouds["source"]), lambda: m.merge(live), lambda: live.merge(m), lambda: m.remove_far([0, 0, 0], 1.0), lambda: m.grid_min,
                     lambda: m.origin, lambda: len(m)):
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
        scans.append(P.PointCloud((clouds["target_xyz"].astype(np.float64) @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)))
    return truth, scans


@pytest.mark.parametrize("model,max_range", [("constant_velocity", None), ("static", 25.0)])
def test_odometry_is_the_public_calls_by_hand(P, M, drive, model, max_range):
    R = P.registration
    _, scans = drive
    poses, results, m = R.scan_to_map_odometry_ndt(scans, MAP_VOXEL, motion_model=model, max_range=max_range)
    with m:
        assert len(poses) == len(results) == 4 and results[0] is None and np.array_equal(poses[0], np.eye(4))
        g = M.centered_grid_min(scans[0].get_center(), MAP_VOXEL)
        assert np.array_equal(m.grid_min, g)
        with M.on_grid(scans[0], MAP_VOXEL, 6, 0.01, g, np.eye(4)) as hand:
            by_hand = [np.eye(4)]
            for k in range(1, 4):
                start = by_hand[-1]
                if model == "constant_velocity" and k >= 2:
                    start = by_hand[-1] @ np.linalg.inv(by_hand[-2]) @ by_hand[-1]
                res = R.registration_ndt(scans[k], hand, None, start)
                by_hand.append(res.transformation)
                hand.insert(scans[k], res.transformation)
                if max_range is not None:
                    hand.remove_far(res.transformation[:3, 3], max_range)
            for k in range(4):
                assert np.array_equal(poses[k], by_hand[k]), k         # bit for bit
            assert _state(hand) == _state(m)
        if max_range is not None:
            d2 = nu.distance2(m.points, poses[-1][:3, 3])
            assert (d2 < max_range * max_range).all() and len(m) > 100
            with M.on_grid(scans[0], MAP_VOXEL, 6, 0.01, g, np.eye(4)) as whole:
                assert len(m) < len(whole)                              # something was in fact out of range


def test_odometry_poses_are_closer_to_the_truth_than_their_starts(P, drive):
    """Under "static" the start of scan k is the pose of scan k - 1, one step (0.2 m, 1 degree) from the truth when that pose is right: condition
    (c) of tests/test_ndt_map_update_api.py, on the device"""
    truth, scans = drive
    poses, results, m = P.registration.scan_to_map_odometry_ndt(scans, MAP_VOXEL, motion_model="static")
    with m:
        valid = int(m.valid.sum())
    for k in range(1, 4):
        a0, d0 = pose_error(poses[k - 1], truth[k])
        a, d = pose_error(poses[k], truth[k])
        print(f"scan {k}: start {np.degrees(a0):.3f} deg {d0:.3f} m -> {np.degrees(a):.4f} deg {d:.4f} m after {results[k].iterations} iterations, fitness {results[k].fitness:.3f}")
        assert results[k].converged and a < a0 and d < d0, (k, a, d, a0, d0)
    assert valid > 458                                                 # (458 of 745 cells are valid after scan 0 alone)
