"""ISS keypoints on the device against a float64 numpy restatement of Open3D's ComputeISSKeypoints on the same float32 points: default
radii, eigenvalues, the saliency and keypoint masks, the outputs among each other, the keypoint -> feature-row pipeline, the smallest and
the degenerate shapes by brute force, and the errors.

Main input: the source of golden pair 899 after ``voxel_down_sample(0.2)`` (about 9.5k points), four parameter sets.

The restatement: brute-force float64 d^2 (``_pair_d2`` of test_gpu_cloud_queries.py), membership d^2 < r^2 with the point itself a member,
the covariance centred on the neighbourhood mean and divided by the count, ``np.linalg.eigvalsh``, and the library's suppression rule:
member j suppresses point i iff s_j > s_i + G, G = 1e-11 salient_radius^2 (include/pcr_hip.h; Open3D has G = 0).

Bounds.  Radii: 1e-12 relative, n eps at n = 1e4 (the argument of the moments bound in test_gpu_cloud_queries.py).  Eigenvalues: the moments
are float64 sums of at most n_b terms of magnitude <= r^2 taken about the query, so a mean moment is off by at most n_b eps r^2 = 5e-14 r^2 at
the largest ball of the main input (226 points); the closed-form solver adds O(eps l1) <= 1e-15 r^2; the bound is 1e-12 r^2, a factor 20.
Masks: equal on every row that is not on a rim -- a member of either ball with |d^2 - r^2| <= 1e-9 r^2 (RIM_RTOL; a count that reaches
min_neighbors only through such a member is such a row), a gamma ratio within 1e-9 relative of its threshold, a reference l3 <= G, or
|max_j s_j - s_i - G| <= G / 2; a row whose non-max ball holds a point with an undecided saliency (radius or gamma rim) is left out of the
keypoint comparison too.  On the main input the rows left out are at most RIM_SHARE = 1e-3 of n per case.

Flat rows are NOT left out.  The golden scan has a clipped ground at z = -1.077297 exactly: about 350 rows of the main input have a
neighbourhood whose members share that coordinate, the covariance has an exactly zero row, and l3 is exactly 0 in the restatement.  Such a
row is decided -- saliency 0, no keypoint -- and the device has to give l3 = 0 there too, not rounding noise of either sign (it takes an
axis that decouples exactly out of the matrix before the closed form).  Leaving them out as "l3 <= G" would break the RIM_SHARE cap."""
import ctypes as C

import numpy as np
import pytest

from conftest import pkg

pytestmark = pytest.mark.gpu

RIM_RTOL, RIM_SHARE = 1e-9, 1e-3
EIG_RTOL = 1e-12                     # x salient_radius^2
RADII_RTOL = 1e-12
G_FACTOR = 1e-11                     # x salient_radius^2
# (salient radius, non-max radius, gamma_21, gamma_32, min_neighbors)
CASES = [(0.0, 0.0, 0.975, 0.975, 5), (1.0, 0.8, 0.975, 0.975, 5), (0.6, 0.5, 0.6, 0.6, 8), (0.35, 0.35, 0.975, 0.975, 5)]
SMALL = (0.3, 0.3, 0.975, 0.975, 3)
OFFSET = np.array([300.0, -150.0, 20.0])


@pytest.fixture(scope="module")
def P():
    return pkg()


# ------------------------------------------------------------------------------------------------------ reference
def _pair_d2(a, b):
    """float64 squared distances of every row of a (float32) to every row of b (float32): an (len(a), len(b)) array."""
    a = a.astype(np.float64); b = b.astype(np.float64)
    d2 = np.zeros((len(a), len(b)))
    for k in range(3):
        d = a[:, k, None] - b[None, :, k]
        d2 += d * d
    return d2


def _ball_pairs(pts, radii, chunk=1000):
    """{r: (rows, cols, d2)} of every pair with d^2 <= r^2 (1 + RIM_RTOL), rows ascending; one pass over the d^2 blocks for all radii."""
    out = {r: ([], [], []) for r in radii}
    for i0 in range(0, len(pts), chunk):
        d2 = _pair_d2(pts[i0:i0 + chunk], pts)
        for r in radii:
            rows, cols = np.nonzero(d2 <= r * r * (1.0 + RIM_RTOL))
            out[r][0].append(rows + i0); out[r][1].append(cols); out[r][2].append(d2[rows, cols])
    return {r: tuple(np.concatenate(v) if v else np.zeros(0, np.int64 if k < 2 else np.float64) for k, v in enumerate(out[r])) for r in radii}


def _brute_resolution(pts, chunk=1000):
    """mean over the points of the distance to the nearest other point (the second smallest d^2, the point itself first); 0 below two points"""
    n = len(pts)
    if n < 2:
        return 0.0
    second = np.concatenate([np.partition(_pair_d2(pts[i0:i0 + chunk], pts), 1, axis=1)[:, 1] for i0 in range(0, n, chunk)])
    return float(np.sqrt(second).sum() / n)


def _iss_reference(pts, rs, rn, g21, g32, min_nb, pairs=None):
    """Open3D's ComputeISSKeypoints in float64 numpy with the suppression guard G; returns the decisions and the rim rows."""
    n = len(pts)
    p = pts.astype(np.float64)
    G = G_FACTOR * rs * rs
    pairs = pairs or _ball_pairs(pts, sorted({rs, rn}))
    # ---- saliency
    rows, cols, d2 = pairs[rs]
    rim_s = np.bincount(rows[np.abs(d2 - rs * rs) <= RIM_RTOL * rs * rs], minlength=n) > 0
    ins = d2 < rs * rs
    rows, cols = rows[ins], cols[ins]
    cnt = np.bincount(rows, minlength=n)
    div = np.maximum(cnt, 1).astype(np.float64)
    off = p[cols] - p[rows]                                      # (exact: differences of float32 values; the covariance does not depend on the origin)
    mean = np.stack([np.bincount(rows, off[:, k], minlength=n) for k in range(3)], 1) / div[:, None]
    c = off - mean[rows]                                         # centred on the neighbourhood mean
    cov = np.zeros((n, 3, 3))
    for a in range(3):
        for b in range(a, 3):
            cov[:, a, b] = cov[:, b, a] = np.bincount(rows, c[:, a] * c[:, b], minlength=n) / div
    enough = cnt >= min_nb
    nonzero = enough & (np.abs(cov).reshape(n, 9).max(1) > 0) if n else np.zeros(0, bool)
    ev = np.linalg.eigvalsh(cov)[:, ::-1].copy() if n else np.zeros((0, 3))      # descending
    ev[~nonzero] = 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        r21, r32 = ev[:, 1] / ev[:, 0], ev[:, 2] / ev[:, 1]
        passes = nonzero & (r21 < g21) & (r32 < g32)
        gamma_rim = nonzero & ((np.abs(r21 - g21) <= RIM_RTOL * g21) | (np.abs(r32 - g32) <= RIM_RTOL * g32))
    sal = np.where(passes, ev[:, 2], 0.0)
    flat = nonzero & (cov[:, [0, 1, 2], [0, 1, 2]] == 0).any(1)      # the members share one coordinate exactly: l3 is exactly 0, a decided row
    low = nonzero & (ev[:, 2] <= G) & ~flat
    # ---- non-maximum suppression
    rows, cols, d2 = pairs[rn]
    rim_n = np.bincount(rows[np.abs(d2 - rn * rn) <= RIM_RTOL * rn * rn], minlength=n) > 0
    ins = d2 < rn * rn
    rows, cols = rows[ins], cols[ins]
    cnt_n = np.bincount(rows, minlength=n)
    best = np.full(n, -np.inf)
    np.maximum.at(best, rows, sal[cols])
    cand = sal > 0
    keep = cand & (cnt_n >= min_nb) & ~(best > sal + G)
    supp_rim = cand & (np.abs(best - sal - G) <= G / 2)
    undecided = rim_s | gamma_rim                                # the reference does not decide these rows' saliency ...
    near = np.bincount(rows, undecided[cols].astype(np.float64), minlength=n) > 0      # ... nor what they do to the rows they are members of
    out_sal = rim_s | gamma_rim | low
    return dict(G=G, cnt=cnt, ev=ev, sal=sal, keep=keep, rim_s=rim_s, out_sal=out_sal, out_keep=out_sal | rim_n | supp_rim | near,
                parts=dict(radius=int((rim_s | rim_n).sum()), gamma=int(gamma_rim.sum()), low=int(low.sum()), suppression=int(supp_rim.sum()), flat=int(flat.sum())))


def _cloud(P, pts):
    return P.PointCloud(pts) if len(pts) else P.PointCloud()          # (the constructor wants at least one row to infer N x 3)


def _device(P, pts, params):
    """the private call: -> dict(idx, mask, sal, ev, radii)"""
    idx, mask, sal, ev, radii = P.geometry._iss_keypoints(_cloud(P, pts), *params)
    return dict(idx=idx.cpu().numpy(), mask=mask, sal=sal, ev=ev, radii=radii)


def _raw(P, pts, params, outputs=True):
    """pcr_iss_keypoints itself -> (status, count, mask, indices, compacted points); outputs=False: every optional pointer null."""
    import torch
    ctx = P._lib.Context.current()
    n = len(pts)
    d = torch.from_numpy(np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 3)).cuda()
    mask = torch.zeros(max(n, 1), dtype=torch.uint8, device="cuda")
    idx = torch.full((max(n, 1),), -1, dtype=torch.int64, device="cuda")
    out = torch.zeros((max(n, 1), 3), dtype=torch.float32, device="cuda")
    m = C.c_int64(-1)
    rs, rn, g21, g32, k = params
    ptr = (lambda t: C.c_void_p(t.data_ptr())) if outputs else (lambda t: None)
    rc = ctx.lib.pcr_iss_keypoints(ctx.handle, C.c_void_p(d.data_ptr() if n else 0), C.c_int64(n), C.c_double(rs), C.c_double(rn), C.c_double(g21),
                                   C.c_double(g32), C.c_int(k), ptr(mask), ptr(out), ptr(idx), C.byref(m), None, None, None)
    kk = max(int(m.value), 0)
    return rc, int(m.value), mask[:n].cpu().numpy().astype(bool), idx[:kk].cpu().numpy(), out[:kk].cpu().numpy()


def _assert_against_reference(dev, ref, rs, what, share=None):
    """eigenvalues, saliency mask and keypoint mask of one device result against the reference; returns the rows left out"""
    n = len(ref["sal"])
    ok_e = ~ref["rim_s"]
    err = np.abs(dev["ev"] - ref["ev"])[ok_e]
    worst = float(err.max() / (EIG_RTOL * rs * rs)) if err.size else 0.0
    left = int(ref["out_keep"].sum())
    print(f"{what}: n = {n}, largest ball {int(ref['cnt'].max()) if n else 0}, reference keypoints {int(ref['keep'].sum())}, device {int(dev['mask'].sum())}; "
          f"worst eigenvalue error / bound {worst:.3e}; rows left out {left} {ref['parts']}")
    assert dev["ev"].shape == (n, 3) and dev["sal"].shape == (n,) and dev["mask"].shape == (n,)
    assert (err <= EIG_RTOL * rs * rs).all(), (what, worst)
    assert np.array_equal(dev["sal"], np.where(dev["sal"] != 0, dev["ev"][:, 2], 0.0))          # the saliency is l3 or 0
    ok_s = ~ref["out_sal"]
    assert np.array_equal((dev["sal"] > 0)[ok_s], (ref["sal"] > 0)[ok_s]), (what, int(((dev["sal"] > 0) != (ref["sal"] > 0))[ok_s].sum()))
    ok_k = ~ref["out_keep"]
    assert np.array_equal(dev["mask"][ok_k], ref["keep"][ok_k]), (what, int((dev["mask"] != ref["keep"])[ok_k].sum()))
    assert np.array_equal(dev["idx"], np.nonzero(dev["mask"])[0])                               # ascending, and the mask's rows
    if share is not None:
        assert left <= share * n, (what, left, ref["parts"])
    return left


# ---------------------------------------------------------------------------------------------------- main input
@pytest.fixture(scope="module")
def cloud(P, small_pair):
    """(source cloud of pair 899 at 0.2 m with normals and colours, its float32 points)"""
    pc = P.PointCloud(small_pair["source"]).voxel_down_sample(0.2)
    pc.estimate_normals(P.KDTreeSearchParamKNN(knn=20))
    pc.colors = np.random.default_rng(3).random((len(pc), 3))
    return pc, pc.points.astype(np.float32)


@pytest.fixture(scope="module")
def resolution(cloud):
    return _brute_resolution(cloud[1])


@pytest.fixture(scope="module")
def references(cloud, resolution):
    """{case: reference}, computed once: the d^2 blocks are shared by the radii of the four cases (case one at the reference's own resolution)"""
    pts = cloud[1]
    radii = {c: ((6.0 * resolution, 4.0 * resolution) if c[0] == 0.0 else (c[0], c[1])) for c in CASES}
    pairs = _ball_pairs(pts, sorted({r for rr in radii.values() for r in rr}))
    return {c: (radii[c], _iss_reference(pts, radii[c][0], radii[c][1], c[2], c[3], c[4], pairs)) for c in CASES}


@pytest.fixture(scope="module")
def devices(P, cloud):
    return {c: _device(P, cloud[1], c) for c in CASES}


# ---------------------------------------------------------------------------------------------------------------- 1
def test_default_radii_are_six_and_four_resolutions(P, cloud, devices, resolution):
    pc = cloud[0]
    res = float(pc.compute_nearest_neighbor_distance().mean())
    rs, rn = devices[CASES[0]]["radii"]
    print(f"resolution {res:.6f} m (brute force {resolution:.6f}); radii used {rs:.6f}, {rn:.6f}; relative differences "
          f"{abs(rs - 6 * res) / (6 * res):.3e}, {abs(rn - 4 * res) / (4 * res):.3e}")
    assert abs(rs - 6.0 * res) <= RADII_RTOL * 6.0 * res and abs(rn - 4.0 * res) <= RADII_RTOL * 4.0 * res
    # one radius given, the other 0: both are replaced
    assert _device(P, cloud[1], (0.7, 0.0, 0.975, 0.975, 5))["radii"] == (rs, rn)
    # explicit radii come back as given
    assert devices[CASES[1]]["radii"] == (1.0, 0.8)


# ------------------------------------------------------------------------------------------------------------ 2, 3
@pytest.mark.parametrize("case", CASES, ids=[f"{c[0]}-{c[1]}-{c[2]}-{c[4]}" for c in CASES])
def test_eigenvalues_and_masks_against_the_restatement(cloud, references, devices, case):
    (rs, rn), ref = references[case]
    dev = devices[case]
    assert 20 <= ref["keep"].sum() <= 0.2 * len(cloud[1])                 # neither answer is trivial
    assert (ref["sal"] > 0).sum() > ref["keep"].sum()                     # the suppression has something to do
    _assert_against_reference(dev, ref, rs, f"case {case}", share=RIM_SHARE)


# ---------------------------------------------------------------------------------------------------------------- 4
def test_outputs_agree_with_each_other(P, cloud, devices):
    pc, pts = cloud
    case = CASES[1]
    dev = devices[case]
    rc, m, mask, idx, out = _raw(P, pts, case)
    assert rc == 0 and m == len(idx) == int(mask.sum())
    assert np.array_equal(mask, dev["mask"])
    assert np.array_equal(idx, np.nonzero(mask)[0]) and (np.diff(idx) > 0).all()
    assert np.array_equal(out, pts[idx])                                   # bit for bit
    assert np.array_equal(P.iss_keypoint_indices(pc, *case), idx) and P.iss_keypoint_indices(pc, *case).dtype == np.int64
    kp = P.o3d.geometry.keypoint.compute_iss_keypoints(pc, *case)
    assert isinstance(kp, P.PointCloud) and len(kp) == len(idx)
    assert np.array_equal(kp.points, pc.points[idx])
    assert kp.has_normals() and np.array_equal(kp.normals, pc.normals[idx])
    assert kp.has_colors() and np.array_equal(kp.colors, pc.colors[idx])
    # every optional pointer null: accepted, the count alone comes back
    rc0, m0, *_ = _raw(P, pts, case, outputs=False)
    assert rc0 == 0 and m0 == m


def test_two_runs_give_the_same_bits(P, cloud, devices):
    for case in (CASES[0], CASES[3]):
        a, b = devices[case], _device(P, cloud[1], case)
        assert a["radii"] == b["radii"]
        for k in ("mask", "idx", "sal", "ev"):
            assert a[k].tobytes() == b[k].tobytes(), (case, k)


# ---------------------------------------------------------------------------------------------------------------- 5
def test_keypoint_rows_of_a_full_cloud_feature(P, cloud, devices):
    pc = cloud[0]
    idx = devices[CASES[1]]["idx"]
    reg = P.o3d.pipelines.registration
    full = reg.compute_fpfh_feature(pc, P.KDTreeSearchParamHybrid(radius=1.0, max_nn=100))
    sel = full.select_by_index(idx)
    assert isinstance(sel, reg.Feature) and sel.num() == len(idx) and sel.dimension() == full.dimension() == 33
    assert np.array_equal(sel.data, full.data[:, idx])
    assert np.array_equal(full.select_by_index(idx.tolist()).data, sel.data)
    assert sel.num() == len(pc.select_by_index(idx))                      # the pair that feeds the RANSAC / FGR entry points


# ---------------------------------------------------------------------------------------------------------------- 6
def _random_cloud(n, seed):
    return (np.random.default_rng(seed).random((n, 3)) + OFFSET).astype(np.float32)


def _assert_small(P, pts, what, params=SMALL):
    ref = _iss_reference(pts, *params)
    dev = _device(P, pts, params)
    _assert_against_reference(dev, ref, params[0], what)
    kp = P.compute_iss_keypoints(_cloud(P, pts), *params)
    assert np.array_equal(kp.points, pts[dev["idx"]].astype(np.float64).reshape(-1, 3))
    return dev, ref


@pytest.mark.parametrize("n", [1, 2, 7, 8, 9, 31, 32, 33, 63, 64, 65, 257, 500])
def test_small_clouds_by_brute_force(P, n):
    dev, ref = _assert_small(P, _random_cloud(n, 200 + n), f"n = {n}")
    if n >= 257:
        assert 0 < ref["keep"].sum() < n and (~ref["out_keep"]).sum() > n // 2          # the comparison is not empty
    if n < SMALL[4]:
        assert not dev["mask"].any()


def test_empty_cloud(P):
    kp = P.compute_iss_keypoints(P.PointCloud())
    assert isinstance(kp, P.PointCloud) and len(kp) == 0
    assert P.iss_keypoint_indices(P.PointCloud(), 0.3, 0.3).shape == (0,)
    rc, m, mask, idx, out = _raw(P, np.zeros((0, 3), np.float32), SMALL)
    assert rc == 0 and m == 0 and len(idx) == 0


def test_coincident_points_have_no_keypoints(P):
    pts = np.repeat(_random_cloud(1, 9), 40, axis=0)
    for params in (SMALL, (0.0, 0.0, 0.975, 0.975, 3)):                   # (default radii: the resolution is 0)
        dev = _device(P, pts, params)
        assert not dev["mask"].any() and len(dev["idx"]) == 0
        assert (dev["ev"] == 0).all() and (dev["sal"] == 0).all()          # the covariance is exactly zero
    assert _device(P, pts, (0.0, 0.0, 0.975, 0.975, 3))["radii"] == (0.0, 0.0)


def test_collinear_points_return(P):
    t = np.linspace(0.0, 1.0, 50)[:, None]
    pts = (OFFSET + t * np.array([0.6, 0.3, 0.2])).astype(np.float32)
    dev = _device(P, pts, SMALL)                                          # l2 is rounding noise: the set is not asserted
    assert dev["idx"].dtype == np.int64 and ((dev["idx"] >= 0) & (dev["idx"] < 50)).all()
    assert np.array_equal(dev["idx"], np.nonzero(dev["mask"])[0])
    assert np.isfinite(dev["ev"]).all() and np.isfinite(dev["sal"]).all() and (dev["ev"][:, 0] > 1e-4).any()


def test_structural_ties_keep_every_point_of_a_cluster(P):
    rng = np.random.default_rng(11)
    a = OFFSET + rng.random((6, 3)) * 0.1
    b = OFFSET + np.array([10.0, 0.0, 0.0]) + rng.random((6, 3)) * 0.1
    pts = np.concatenate([a, b])[rng.permutation(12)].astype(np.float32)
    which = pts[:, 0] > OFFSET[0] + 5.0
    dev, ref = _assert_small(P, pts, "two clusters")
    assert not ref["out_keep"].any() and (ref["cnt"] == 6).all()          # all six points of a cluster share one neighbourhood
    for side in (which, ~which):
        assert len(set(dev["mask"][side].tolist())) == 1 and np.array_equal(dev["mask"][side], ref["keep"][side])
    assert dev["mask"].all()                                              # the tie keeps all of them (the strict rule would keep one per cluster)


def test_min_neighbors_above_n(P):
    pts = _random_cloud(64, 5)
    dev = _device(P, pts, (0.3, 0.3, 0.975, 0.975, 65))
    assert not dev["mask"].any() and (dev["sal"] == 0).all() and (dev["ev"] == 0).all()
    assert not _device(P, pts, (5.0, 5.0, 0.975, 0.975, 65))["mask"].any()


# ---------------------------------------------------------------------------------------------------------------- 7
def test_bad_arguments_raise(P):
    pts = _random_cloud(65, 1)
    pc = P.PointCloud(pts)
    ctx = P._lib.Context.current()
    for params in ((-0.5, 0.3, 0.975, 0.975, 5), (0.3, -0.5, 0.975, 0.975, 5), (0.3, 0.3, 0.975, 0.975, 0), (0.3, 0.3, float("nan"), 0.975, 5),
                   (0.3, 0.3, 0.975, float("nan"), 5)):
        with pytest.raises(RuntimeError, match="iss_keypoints"):
            P.compute_iss_keypoints(pc, *params)
        rc, *_ = _raw(P, pts, params)
        assert rc == P._lib.PCR_EINVAL
        assert ctx.lib.pcr_last_error(ctx.handle)
    # a null cloud with n > 0
    assert ctx.lib.pcr_iss_keypoints(ctx.handle, None, C.c_int64(4), C.c_double(0.3), C.c_double(0.3), C.c_double(0.975), C.c_double(0.975), C.c_int(5),
                                     None, None, None, None, None, None, None) == P._lib.PCR_EINVAL
