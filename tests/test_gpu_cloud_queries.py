"""The cloud queries on the device against float64 references on the same float32 points: nearest-neighbour distances and cloud-to-cloud
distances against the oracle's k-d tree, the radius outlier filter against an exact numpy count, mean and covariance against numpy, the
two functions built on them, small and degenerate shapes by brute force, and bit-for-bit repeatability.

Main input: the source of golden pair 899 after ``voxel_down_sample(0.2)`` (about 9.5k points, no coincident points, mean
nearest-neighbour distance 0.16 m); the other cloud is the pair's target prepared the same way (cloud-to-cloud distances up to 18.5 m:
the unbounded walk is exercised).

Bounds.  A distance is exact for the neighbour the device chose, and the neighbour is chosen by float32 d^2: a row may differ from the
oracle's by a float32 tie, 2e-6 relative on the distance (half of the 4e-6 on d^2 that test_knn_index_is_exact grants such a tie), and at
least 99.99 % of the rows are the same neighbour in float64 arithmetic, 1e-12 relative.  The radius mask must equal the exact count on
every row without a neighbour on the rim, |d^2 - r^2| <= 1e-9 r^2.  Moments: 1e-10 x the largest raw second moment, a factor 50 over
the float64 summation bound n eps = 2e-12 at n = 1e4."""
import copy
import ctypes as C

import numpy as np
import pytest

from conftest import pkg

pytestmark = pytest.mark.gpu

TIE_RTOL, SAME_RTOL, SAME_SHARE = 2e-6, 1e-12, 0.9999
RIM_RTOL, RIM_SHARE = 1e-9, 1e-3
RADIUS_CASES = [(5, 0.5), (2, 0.3), (30, 1.0)]


@pytest.fixture(scope="module")
def P():
    return pkg()


@pytest.fixture(scope="module")
def clouds(P, small_pair):
    """(source cloud, target cloud, their float32 points) at 0.2 m."""
    src = P.PointCloud(small_pair["source"]).voxel_down_sample(0.2)
    tgt = P.PointCloud(small_pair["target"]).voxel_down_sample(0.2)
    return src, tgt, src.points.astype(np.float32), tgt.points.astype(np.float32)


@pytest.fixture(scope="module")
def nn_reference(oracle, clouds):
    pts = clouds[2]
    return np.sqrt(oracle.knn(pts, pts, 2)[1][:, 1])


@pytest.fixture(scope="module")
def nn_device(clouds):
    return clouds[0].compute_nearest_neighbor_distance()


def _pair_d2(a, b):
    """float64 squared distances of every row of a (float32) to every row of b (float32): an (len(a), len(b)) array."""
    a = a.astype(np.float64); b = b.astype(np.float64)
    d2 = np.zeros((len(a), len(b)))
    for k in range(3):
        d = a[:, k, None] - b[None, :, k]
        d2 += d * d
    return d2


def _radius_reference(pts, cases, chunk=1000):
    """Exact float64 count per case -> {case: (keep mask, rim rows)}: keep = more than nb points (the point itself included) with
    d^2 < r^2; rim = the row has a neighbour with |d^2 - r^2| <= 1e-9 r^2."""
    n = len(pts)
    cnt = {c: np.zeros(n, np.int64) for c in cases}
    rim = {c: np.zeros(n, bool) for c in cases}
    for i0 in range(0, n, chunk):
        d2 = _pair_d2(pts[i0:i0 + chunk], pts)
        for c in cases:
            r2 = float(c[1]) ** 2
            cnt[c][i0:i0 + chunk] = (d2 < r2).sum(1)
            rim[c][i0:i0 + chunk] = (np.abs(d2 - r2) <= RIM_RTOL * r2).any(1)
    return {c: (cnt[c] > c[0], rim[c]) for c in cases}


@pytest.fixture(scope="module")
def radius_reference(clouds):
    return _radius_reference(clouds[2], RADIUS_CASES)


@pytest.fixture(scope="module")
def cloud_with_normals(P, clouds):
    pc = copy.deepcopy(clouds[0])
    pc.estimate_normals(P.KDTreeSearchParamKNN(knn=20))
    return pc


def _assert_distances(dev, ref, what):
    assert dev.dtype == np.float64 and dev.shape == ref.shape, what
    err = np.abs(dev - ref)
    same = err <= SAME_RTOL * ref
    worst = float((err / np.maximum(ref, 1e-300)).max()) if len(ref) else 0.0
    print(f"{what}: {len(ref)} rows, worst relative difference {worst:.3e}, {int((~same).sum())} rows beyond {SAME_RTOL:g}")
    assert (err <= TIE_RTOL * ref).all(), (what, worst)
    assert same.mean() >= SAME_SHARE if len(ref) else True, (what, float(same.mean()))
    return same


def _host_distance(q, t, nearest):
    """the device's rule in numpy float64: differences, squares and sums in the order x, y, z, each rounded once"""
    e = q.astype(np.float64) - t[nearest].astype(np.float64)
    return np.sqrt(e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1] + e[:, 2] * e[:, 2])


def _radius_raw(P, pts, nb_points, radius):
    """pcr_remove_radius_outlier with every output -> (status, mask, indices, compacted points)."""
    import torch
    ctx = P._lib.Context.current()
    n = len(pts)
    d = torch.from_numpy(np.ascontiguousarray(pts, dtype=np.float32)).cuda()
    mask = torch.zeros(max(n, 1), dtype=torch.uint8, device="cuda")
    idx = torch.full((max(n, 1),), -1, dtype=torch.int64, device="cuda")
    out = torch.zeros((max(n, 1), 3), dtype=torch.float32, device="cuda")
    m = C.c_int64(-1)
    rc = ctx.lib.pcr_remove_radius_outlier(ctx.handle, C.c_void_p(d.data_ptr() if n else 0), C.c_int64(n), C.c_int(nb_points), C.c_double(radius),
                                           C.c_void_p(mask.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(idx.data_ptr()), C.byref(m))
    k = max(int(m.value), 0)
    return rc, mask[:n].cpu().numpy().astype(bool), idx[:k].cpu().numpy(), out[:k].cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------- 1
def test_nearest_neighbor_distance_against_the_kd_tree(clouds, nn_reference, nn_device):
    assert (nn_reference > 0).all()                       # no coincident points on this input
    _assert_distances(nn_device, nn_reference, "nearest-neighbour distance")
    print(f"mean nearest-neighbour distance {nn_device.mean():.4f} m")


# ---------------------------------------------------------------------------------------------------------------- 2
def test_point_cloud_distance_against_the_kd_tree(oracle, clouds):
    src, tgt, pts, tpts = clouds
    ridx, rd2, _ = oracle.knn(tpts, pts, 1)
    ref = np.sqrt(rd2[:, 0])
    assert ref.max() > 10.0                               # far queries: the walk is unbounded
    dist, nearest = src._point_cloud_distance(tgt)
    assert np.array_equal(src.compute_point_cloud_distance(tgt), dist)
    same = _assert_distances(dist, ref, "cloud-to-cloud distance")
    assert nearest.dtype == np.int32 and nearest.min() >= 0 and nearest.max() < len(tpts)
    assert np.array_equal(nearest[same], ridx[same, 0])
    assert np.array_equal(_host_distance(pts, tpts, nearest), dist)      # exact for the neighbour returned


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("nb_points,radius", RADIUS_CASES)
def test_radius_outlier_filter_against_an_exact_count(P, clouds, radius_reference, cloud_with_normals, nb_points, radius):
    pts = clouds[2]
    keep, rim = radius_reference[(nb_points, radius)]
    print(f"radius filter ({nb_points}, {radius}): reference keeps {keep.mean():.3f}, {int(rim.sum())} rim rows")
    assert 0.05 < keep.mean() < 0.95                      # neither answer is trivial
    assert rim.mean() <= RIM_SHARE
    rc, mask, idx, out = _radius_raw(P, pts, nb_points, radius)
    assert rc == 0
    assert np.array_equal(mask[~rim], keep[~rim]), int((mask != keep)[~rim].sum())
    assert np.array_equal(idx, np.nonzero(mask)[0])       # ascending, and the mask's rows
    assert np.array_equal(out, pts[idx])
    cloud, index = cloud_with_normals.remove_radius_outlier(nb_points, radius)
    assert isinstance(index, list) and np.array_equal(np.asarray(index, np.int64), idx)
    assert np.array_equal(cloud.points, cloud_with_normals.points[idx])
    assert cloud.has_normals() and np.array_equal(cloud.normals, cloud_with_normals.normals[idx])


# ---------------------------------------------------------------------------------------------------------------- 4
def _moments_reference(pts):
    p = pts.astype(np.float64)
    n = len(p)
    if n == 0:
        return np.zeros(3), np.eye(3), 1.0
    mean = p.mean(0)
    c = p - mean
    return mean, c.T @ c / n, float(np.abs(p.T @ p / n).max())


def _assert_moments(pc, pts, what):
    mean, cov = pc.compute_mean_and_covariance()
    rmean, rcov, m2 = _moments_reference(pts)
    assert mean.dtype == np.float64 and mean.shape == (3,) and cov.dtype == np.float64 and cov.shape == (3, 3)
    print(f"{what}: largest raw second moment {m2:.3f}, mean off by {np.abs(mean - rmean).max():.3e}, covariance by {np.abs(cov - rcov).max():.3e}")
    assert np.abs(cov - rcov).max() <= 1e-10 * m2, what
    assert np.abs(mean - rmean).max() <= 1e-10 * np.sqrt(m2), what       # (the same bound in metres: tighter than 1e-10 m2 here)
    assert np.array_equal(cov, cov.T)
    assert np.array_equal(pc.get_center(), mean)
    return mean, cov


def test_mean_and_covariance_against_numpy(clouds):
    src, _, pts, _ = clouds
    _, cov = _assert_moments(src, pts, "0.2 m cloud")
    assert np.allclose(cov, np.cov(pts.astype(np.float64).T, bias=True), rtol=0, atol=1e-10 * float(np.abs(pts.astype(np.float64).T @ pts.astype(np.float64) / len(pts)).max()))


# ---------------------------------------------------------------------------------------------------------------- 5
def _random_cloud(n, seed):
    return (np.random.default_rng(seed).random((n, 3)) * 4.0).astype(np.float32)


def _cloud(P, pts):
    return P.PointCloud(pts) if len(pts) else P.PointCloud()          # (the constructor wants at least one row to infer N x 3)


def _brute_second(pts):
    """sqrt of the second smallest d^2 of every point to the cloud, itself included; 0 with fewer than two points"""
    if len(pts) < 2:
        return np.zeros(len(pts))
    return np.sqrt(np.sort(_pair_d2(pts, pts), axis=1)[:, 1])


def _assert_radius_small(P, pts, nb_points, radius, what):
    keep, rim = _radius_reference(pts, [(nb_points, radius)])[(nb_points, radius)]
    assert not rim.any(), what                            # (property of the seeded input)
    cloud, index = _cloud(P, pts).remove_radius_outlier(nb_points, radius)
    assert np.array_equal(np.asarray(index, np.int64), np.nonzero(keep)[0]), what
    assert np.array_equal(cloud.points, pts[keep].astype(np.float64)), what
    return keep


@pytest.mark.parametrize("n", [0, 1, 2, 3, 63, 64, 65, 513])
def test_small_clouds_by_brute_force(P, n):
    pts = _random_cloud(n, 100 + n)
    pc = _cloud(P, pts)
    assert len(pc) == n
    # nearest-neighbour distance
    d = pc.compute_nearest_neighbor_distance()
    ref = _brute_second(pts)
    if n < 2:
        assert d.dtype == np.float64 and d.shape == (n,) and (d == 0).all()
    else:
        _assert_distances(d, ref, f"n = {n}")
    # this cloud as the TARGET of 65 queries (n = 0: the empty target, n = 1: the one-point target)
    qpts = _random_cloud(65, 7) + np.float32(1.5)
    dist, nearest = P.PointCloud(qpts)._point_cloud_distance(pc)
    if n == 0:
        assert dist.shape == (65,) and (dist == 0).all() and (nearest == -1).all()
    else:
        d2 = _pair_d2(qpts, pts)
        same = _assert_distances(dist, np.sqrt(d2.min(1)), f"65 queries against n = {n}")
        assert np.array_equal(nearest[same], d2.argmin(1)[same])
        assert np.array_equal(_host_distance(qpts, pts, nearest), dist)
    # ... and as the source: an empty source writes nothing
    back = pc.compute_point_cloud_distance(P.PointCloud(qpts))
    assert back.shape == (n,) and back.dtype == np.float64
    if n:
        _assert_distances(back, np.sqrt(_pair_d2(pts, qpts).min(1)), f"n = {n} queries against 65")
    # radius filter: the count includes the point itself, so nb_points = 1 keeps exactly the points with a neighbour inside the radius
    for nb_points, radius in ((1, 0.45), (3, 0.8)):
        keep = _assert_radius_small(P, pts, nb_points, radius, f"n = {n} ({nb_points}, {radius})")
        if n >= 63:
            assert 0 < keep.sum() < n, (n, nb_points, radius)
    # moments
    mean, cov = _assert_moments(pc, pts, f"n = {n}")
    if n == 0:
        assert np.array_equal(mean, np.zeros(3)) and np.array_equal(cov, np.eye(3))
    if n == 1:
        assert np.array_equal(mean, pts[0].astype(np.float64)) and np.array_equal(cov, np.zeros((3, 3)))
    # uniform_down_sample is an index list
    assert np.array_equal(pc.uniform_down_sample(3).points, pts[::3].astype(np.float64).reshape(-1, 3))


def test_every_point_duplicated(P):
    base = _random_cloud(200, 5)
    pts = np.concatenate([base, base])[np.random.default_rng(6).permutation(400)]
    pc = P.PointCloud(pts)
    d = pc.compute_nearest_neighbor_distance()
    assert d.shape == (400,) and (d == 0).all()
    # the count includes the duplicates: every point counts itself twice, so nb_points = 1 keeps everything and the filter at
    # (3, 0.5) keeps the points with at least one other PAIR inside the radius
    cloud, index = pc.remove_radius_outlier(1, 1e-3)
    assert index == list(range(400))
    keep = _assert_radius_small(P, pts, 3, 0.5, "duplicated cloud")
    single = _radius_reference(base, [(3, 0.5)])[(3, 0.5)][0]
    assert 0 < keep.sum() < 400 and keep.sum() > 2 * single.sum()


def test_bad_arguments_raise(P):
    pc = P.PointCloud(_random_cloud(65, 1))
    for nb_points, radius in ((0, 0.5), (-1, 0.5), (5, 0.0), (5, -1.0)):
        with pytest.raises(RuntimeError, match="Illegal input parameters, number of points and radius must be positive"):
            pc.remove_radius_outlier(nb_points, radius)
        rc, *_ = _radius_raw(P, _random_cloud(65, 1), nb_points, radius)
        assert rc == P._lib.PCR_EINVAL
    ctx = P._lib.Context.current()
    assert b"nb_points" in ctx.lib.pcr_last_error(ctx.handle)
    for k in (0, -2):
        with pytest.raises(RuntimeError):
            pc.uniform_down_sample(k)
    # a missing output pointer is refused, not written through
    import torch
    d = torch.zeros((4, 3), dtype=torch.float32, device="cuda")
    assert ctx.lib.pcr_nearest_neighbor_distance(ctx.handle, C.c_void_p(d.data_ptr()), C.c_int64(4), None) == P._lib.PCR_EINVAL
    assert ctx.lib.pcr_point_cloud_distance(ctx.handle, C.c_void_p(d.data_ptr()), C.c_int64(4), C.c_void_p(d.data_ptr()), C.c_int64(4), None, None) == P._lib.PCR_EINVAL
    assert ctx.lib.pcr_mean_and_covariance(ctx.handle, C.c_void_p(d.data_ptr()), C.c_int64(4), None, None) == P._lib.PCR_EINVAL


# ---------------------------------------------------------------------------------------------------------------- 6
def _eigen_features_restated(pts):
    """ALL_FUNCTIONS.py:1033-1058 in numpy float64; the normalised cloud is rounded to float32 where the stand-in stores it"""
    p = pts.astype(np.float64)
    q = p - p.mean(0)
    q = q / max(np.linalg.norm(q.max(0)), np.linalg.norm(q.min(0)))
    q = q.astype(np.float32).astype(np.float64)
    s = np.linalg.svd(np.cov(q.T, bias=True))[1]
    total = s.sum()
    s = s / np.linalg.norm(s)
    return np.array([(s[0] - s[1]) / s[0], (s[1] - s[2]) / s[0], s[2] / s[0], s[2] / s.sum(), s[0] - s[2] / s[0], (s[0] * s[1] * s[2]) ** (1 / 3), total])


def test_eigen_features_and_knn_distance_table(P, clouds, nn_device):
    src, tgt, pts, _ = clouds
    got = P.extract_eigen_features(src)
    ref = _eigen_features_restated(pts)
    print("eigen features", got, "relative difference", np.abs(got - ref) / np.abs(ref))
    assert got.shape == (7,) and got.dtype == np.float64
    assert np.allclose(got, ref, rtol=1e-9, atol=0.0)
    table = P.knn_distance_table(src, tgt)
    assert [label for _, label in table] == ["Voxel downsampling", "Hybrid downsampling"]
    assert np.array_equal(table[0][0], nn_device)
    assert np.array_equal(table[1][0], tgt.compute_nearest_neighbor_distance()) and len(table[1][0]) == len(tgt)


# ---------------------------------------------------------------------------------------------------------------- 7
def test_two_calls_give_the_same_bits(P, clouds, nn_device):
    src, tgt, pts, _ = clouds
    assert np.array_equal(src.compute_nearest_neighbor_distance(), nn_device)
    a, b = src._point_cloud_distance(tgt), src._point_cloud_distance(tgt)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    r1, r2 = _radius_raw(P, pts, 5, 0.5), _radius_raw(P, pts, 5, 0.5)                 # status, mask, indices, compacted points
    assert r1[0] == r2[0] == 0 and all(np.array_equal(x, y) for x, y in zip(r1[1:], r2[1:]))
    assert src.remove_radius_outlier(5, 0.5)[1] == src.remove_radius_outlier(5, 0.5)[1] == r1[2].tolist()
    assert src.get_center().tobytes() == src.get_center().tobytes()
    m1, m2 = src.compute_mean_and_covariance(), src.compute_mean_and_covariance()
    assert m1[0].tobytes() == m2[0].tobytes() and m1[1].tobytes() == m2[1].tobytes()
