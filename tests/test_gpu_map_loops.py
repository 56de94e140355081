"""What the three map loops -- registration_voxelized_gicp, registration_ndt, registration_point_map (point to point, and point to plane on a map
that estimates its normals: both forms of its kernel) -- share and what no other test holds them to: the chunk boundaries of the pump, the ragged
last chunk, replay from the graph cache, three loops in one cache, and the shared tail of the correspondence sets.

The inputs are synthetic and seeded: about 600 points on two perpendicular planes with normals, 1.0 m cells, and as the source 513 of them under a
small known motion -- 513 is one more than the 512 source points a workgroup of the iteration kernels owns, so there are two workgroups and the
second holds one live lane -- and a source of one point.  The criteria cannot hold: both relative thresholds are 0 and |x| < 0 is never true, so
every loop runs max_iteration updates and one more launch that sees iteration == max_iteration.  The loops queue their launches in chunks of 8
(PCR_ICP_CHUNK unset) and only a full chunk is replayed as a cached graph: max_iteration + 1 launches for max_iteration in (0, 1, 7, 8, 9, 16,
17) are a lone ragged chunk, a ragged chunk of two, one full chunk, full plus one, full plus two, two full plus one and two full plus two.

Why a call with max_iteration = k must equal k chained calls with max_iteration = 1 bit for bit: every launch linearises all source points at the
float64 pose in the state and nothing else of the state enters the sums or the update; the pose goes out and comes back as the same 16 doubles."""
import os

import numpy as np
import pytest

from conftest import pkg

pytestmark = pytest.mark.gpu

VOXEL = 1.0
MAX_ITS = (0, 1, 7, 8, 9, 16, 17)
LOOPS = ("vgicp", "ndt", "point", "plane")


@pytest.fixture(scope="module")
def P():
    return pkg()


def _motion():
    a = np.deg2rad(0.8)
    axis = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)
    T[:3, 3] = [0.03, -0.02, 0.04]
    return T


@pytest.fixture(scope="module")
def scene(P):
    """the clouds and one map per loop; the maps live as long as the module"""
    R = P.registration
    rng = np.random.default_rng(2024)
    floor = np.column_stack([rng.uniform(0, 4, 300), rng.uniform(0, 4, 300), np.zeros(300)])
    wall = np.column_stack([np.zeros(300), rng.uniform(0, 4, 300), rng.uniform(0, 4, 300)])
    xyz = (np.concatenate([floor, wall]) + rng.normal(0.0, 0.002, (600, 3))).astype(np.float32)
    nrm = np.concatenate([np.tile([0.0, 0.0, 1.0], (300, 1)), np.tile([1.0, 0.0, 0.0], (300, 1))]).astype(np.float32)
    pick = np.sort(rng.permutation(600)[:513])
    inv = np.linalg.inv(_motion())
    src_xyz = (xyz[pick].astype(np.float64) @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)
    src_nrm = (nrm[pick].astype(np.float64) @ inv[:3, :3].T).astype(np.float32)

    def cloud(p, n=None):
        pc = P.PointCloud(np.ascontiguousarray(p))
        if n is not None:
            pc.normals = np.ascontiguousarray(n)
        return pc

    target, bare = cloud(xyz, nrm), cloud(xyz)
    s = {"source": cloud(src_xyz, src_nrm), "one": cloud(src_xyz[256:257], src_nrm[256:257])}
    s["vgicp"] = R.VoxelCovarianceMap(target, VOXEL)
    s["ndt"] = R.NormalDistributionsMap(target, VOXEL)
    s["point"] = R.VoxelPointMap(bare, VOXEL)
    s["plane"] = R.VoxelPointMap(bare, VOXEL)
    assert s["plane"].estimate_normals(VOXEL, 5) > 500 and s["plane"].normals_estimated and not s["point"].has_normals
    yield s
    for name in LOOPS:
        s[name].close()


def _register(P, s, loop, source, init, max_it):
    R = P.registration
    crit = R.ICPConvergenceCriteria(0.0, 0.0, max_it)
    if loop == "vgicp":
        return R.registration_voxelized_gicp(source, s["vgicp"], None, init, None, crit, 7, 1)
    if loop == "ndt":
        return R.registration_ndt(source, s["ndt"], None, init, crit, 7)
    est = R.TransformationEstimationPointToPlane() if loop == "plane" else R.TransformationEstimationPointToPoint()
    return R.registration_point_map(source, s[loop], VOXEL, None, init, est, crit, 27)


def _rows_at(s, loop, source, T):
    """the loop's own correspondences call at the pose T, as the registration counts rows"""
    if loop == "vgicp":
        return s["vgicp"].correspondences(source, T, 7, 1).cpu().numpy()
    if loop == "ndt":
        return s["ndt"].correspondences(source, T, 7).cpu().numpy()
    rows = s[loop].correspondences(source, T, VOXEL, 27).cpu().numpy()
    return rows[s["plane"].normal_valid[rows[:, 1]]] if loop == "plane" else rows      # (a match to a row that is not valid is no row)


def _key(res):
    return (res.transformation.tobytes(), res.fitness, res.inlier_rmse, res.iterations, res.converged, res.correspondence_set.tobytes())


@pytest.fixture(scope="module")
def first(P, scene):
    """every (loop, max_iteration) once, from the identity: what the repeats, the chains and the interleaved orders are compared with"""
    # the library reads its loop switches once per process: the chunk shapes named above are those of the defaults, so the defaults it must be
    assert os.environ.get("PCR_ICP_CHUNK", "8") == "8" and os.environ.get("PCR_ICP_GRAPH", "1") != "0", "run with PCR_ICP_CHUNK and PCR_ICP_GRAPH unset"
    return {(loop, k): _register(P, scene, loop, scene["source"], np.eye(4), k) for loop in LOOPS for k in MAX_ITS}


@pytest.mark.parametrize("loop", LOOPS)
def test_every_chunk_shape_runs_max_iteration_updates(P, scene, first, loop):
    for k in MAX_ITS:
        res = first[loop, k]
        print(f"{loop} max_iteration {k}: iterations {res.iterations}, fitness {res.fitness:.4f}, rmse {res.inlier_rmse:.5f}, rows {len(res.correspondence_set)}")
        assert res.iterations == k and not res.converged, (loop, k, res.iterations, res.converged)
        assert np.isfinite(res.transformation).all() and np.array_equal(res.transformation[3], [0, 0, 0, 1])
        # the shared tail: the correspondence set is the rows of the loop's own correspondences call at the returned pose
        assert np.array_equal(res.correspondence_set, _rows_at(scene, loop, scene["source"], res.transformation)), (loop, k)
        assert _key(_register(P, scene, loop, scene["source"], np.eye(4), k)) == _key(res), (loop, k)      # (a full chunk now replays from the cache)
    assert first[loop, 0].fitness > 0.5                                  # most source points have a row at the start
    assert np.array_equal(first[loop, 0].transformation, np.eye(4))
    assert not np.array_equal(first[loop, 1].transformation, np.eye(4))  # ... and an update moves the pose


@pytest.mark.parametrize("loop", LOOPS)
def test_one_call_equals_chained_calls_of_one_iteration(P, scene, first, loop):
    T = np.eye(4)
    for k in range(1, 18):
        step = _register(P, scene, loop, scene["source"], T, 1)          # (two launches: a ragged chunk, never a graph)
        assert step.iterations == 1
        T = step.transformation
        if k in MAX_ITS:
            want = first[loop, k]
            assert T.tobytes() == want.transformation.tobytes(), (loop, k, float(np.abs(T - want.transformation).max()))
            # the last launch of either call linearised at this pose: the same figures and the same rows
            assert (step.fitness, step.inlier_rmse) == (want.fitness, want.inlier_rmse)
            assert np.array_equal(step.correspondence_set, want.correspondence_set)


@pytest.mark.parametrize("order", [LOOPS, ("plane", "ndt", "point", "vgicp")])
def test_interleaved_loops_share_one_graph_cache(P, scene, first, order):
    for k in (9, 8, 17):
        for loop in order:
            assert _key(_register(P, scene, loop, scene["source"], np.eye(4), k)) == _key(first[loop, k]), (order, loop, k)


@pytest.mark.parametrize("loop", LOOPS)
def test_a_source_of_one_point(P, scene, loop):
    for k in (0, 1, 9):
        res = _register(P, scene, loop, scene["one"], np.eye(4), k)
        assert res.iterations == k and not res.converged and np.isfinite(res.transformation).all(), (loop, k)
        assert np.array_equal(res.correspondence_set, _rows_at(scene, loop, scene["one"], res.transformation))
        assert _key(_register(P, scene, loop, scene["one"], np.eye(4), k)) == _key(res)
    assert len(_register(P, scene, loop, scene["one"], np.eye(4), 0).correspondence_set) >= 1


@pytest.mark.parametrize("loop", ["point", "plane"])
def test_linearize_is_untouched_by_a_registration_on_the_same_map(P, scene, loop):
    R = P.registration
    est = R.TransformationEstimationPointToPlane() if loop == "plane" else R.TransformationEstimationPointToPoint()

    def sums():
        lin = scene[loop].linearize(scene["source"], np.eye(4), VOXEL, est, 27)
        return (lin.JTJ.tobytes(), lin.JTr.tobytes(), lin.rows, lin.sum_d2, lin.sum_r2)

    before = sums()
    assert before[2] > 256
    _register(P, scene, loop, scene["source"], np.eye(4), 9)
    assert sums() == before
