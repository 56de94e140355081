"""Plane segmentation on the device against the restatement of the rules of include/pcr_hip.h (plane_reference.py) on the same float32 points.

The answer is one sequential loop's, so the comparison is equality: valid flags, planes bit for bit and counts of every hypothesis through the
test hook; iterations run, best iteration, valid count, inlier count and the inlier index list of the call.  Two things are summed in the device's
own fixed order and compared with a tolerance: the err of a hypothesis (1e-12 relative: at most 8 263 float64 addends of one sign) and the moments
of the refit (normal within 1e-12 rad, d within 1e-11 m of the ``math.fsum`` refit: four summation orders of these inlier sets differ by at most
2.4e-16 rad and 1.1e-14 m).  The restatement counts what would make an exact comparison fragile -- ``rim`` pairs with a distance
within 1e-9 relative of the threshold, ``near`` hypotheses tying the running best within 1e-9 -- and every comparing test asserts both are 0.

Main input: every second source point of golden pair 899 (8,263 points).  The round of the device loop is 1024 hypotheses: one case ends in the
second round (1296 iterations run), one has its best hypothesis in the fifth (iteration 4393)."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from conftest import pkg
from plane_reference import (plane_difference, plane_dist, plane_from_sample, plane_hypotheses, sample_rows, segment_plane_reference)

pytestmark = pytest.mark.gpu

EINVAL = -1
OFFSET = np.array([300.0, -150.0, 20.0])
PS_ROUND, PS_TILE, PS_SPLIT_ROWS, PS_MAX_SPLITS = 1024, 512, 1024, 256      # csrc/pcr_segment.hip
TOL_RAD, TOL_D = 1e-12, 1e-11
# (thr, num_iterations, probability, seed, ransac_n) -> (best count, best iteration, iterations run, valid) of the restatement
MAIN = {
    (0.1, 1000, 0.99999999, 1, 3): (1984, 887, 1000, 1000),
    (0.1, 1000, 0.999, 7, 3): (1965, 135, 511, 511),                    # early stop
    (0.2, 2000, 0.99, 11, 3): (2744, 106, 124, 124),
    (0.05, 300, 1.0, 3, 3): (1187, 228, 300, 300),                      # probability 1: no early stop
    (0.1, 5000, 0.99999999, 1, 3): (1997, 1013, 1296, 1296),            # ends past the first round
    (0.02, 5000, 0.999, 9, 3): (702, 902, 5000, 4997),                  # three draws with a repeated row
    (0.1, 1000, 0.999, 5, 4): (1909, 664, 1000, 1000),
    (0.1, 1000, 0.999, 5, 6): (1683, 443, 1000, 1000),
    (0.1, 500, 0.999, 5, 8): (1759, 332, 500, 500),
    (0.1, 5000, 0.99999999, 1, 5): (2065, 4393, 5000, 5000),            # the best in a late round
}
MOVED = {k: MAIN[k] for k in [(0.1, 1000, 0.99999999, 1, 3), (0.1, 1000, 0.999, 7, 3), (0.1, 1000, 0.999, 5, 4)]}
FIRST = {3: (3, 6, 7, 1), 4: (4, 1, 2, 1), 9: (9, 1, 2, 1), 63: (57, 1, 6, 6), 65: (58, 0, 6, 6), 257: (189, 7, 14, 14)}      # at (0.1, 50, 0.999, 2, 3)
HOOK = [(0.1, 1, 3), (0.1, 5, 4), (0.1, 5, 6)]                          # (thr, seed, ransac_n): the first 1 000 iterations


@pytest.fixture(scope="module")
def P():
    return pkg()


def _params(P, case):
    thr, iters, prob, seed, rn = case
    return P._lib.PcrPlaneParams(int(rn), int(iters), float(prob), int(seed))


def _raw(P, pts, case, mask=True, index=True, count=True, info=True, xyz=True, plane=True, n=None, params=True):
    """pcr_segment_plane itself -> (status, plane (4,), mask uint8 (n,), index int64 (capacity n), out_n, info); a False switch passes a null pointer"""
    import torch
    ctx = P._lib.Context.current()
    pts = np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 3)
    rows = len(pts)
    d = torch.from_numpy(pts).cuda()
    m = torch.full((max(rows, 1),), 9, dtype=torch.uint8, device="cuda")
    idx = torch.full((max(rows, 1),), -7, dtype=torch.int64, device="cuda")
    pl = (C.c_double * 4)(7.0, 7.0, 7.0, 7.0)
    k = C.c_int64(-7)
    inf = P._lib.PcrPlaneInfo()
    par = _params(P, case)
    rc = ctx.lib.pcr_segment_plane(ctx.handle, C.c_void_p(d.data_ptr()) if xyz and rows else None, C.c_int64(rows if n is None else n), C.c_double(case[0]),
                                   C.byref(par) if params else None, pl if plane else None, C.c_void_p(m.data_ptr()) if mask else None,
                                   C.c_void_p(idx.data_ptr()) if index else None, C.byref(k) if count else None, C.byref(inf) if info else None)
    return rc, np.array(pl), m[:rows].cpu().numpy(), idx[:rows].cpu().numpy(), int(k.value), inf


def _hook(P, pts, thr, seed, rn, first, count):
    import torch
    ctx = P._lib.Context.current()
    pts = np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 3)
    d = torch.from_numpy(pts).cuda()
    valid = torch.full((count,), 9, dtype=torch.uint8, device="cuda")
    plane = torch.full((count, 4), 7.0, dtype=torch.float64, device="cuda")
    cnt = torch.full((count,), -7, dtype=torch.int32, device="cuda")
    err = torch.full((count,), -7.0, dtype=torch.float64, device="cuda")
    par = P._lib.PcrPlaneParams(int(rn), 100, 0.999, int(seed))
    rc = ctx.lib.pcr_debug_plane_hypotheses(ctx.handle, C.c_void_p(d.data_ptr()), C.c_int64(len(pts)), C.c_double(thr), C.byref(par), C.c_int64(first), C.c_int64(count),
                                            C.c_void_p(valid.data_ptr()), C.c_void_p(plane.data_ptr()), C.c_void_p(cnt.data_ptr()), C.c_void_p(err.data_ptr()))
    assert rc == 0, ctx.lib.pcr_last_error(ctx.handle)
    return valid.cpu().numpy(), plane.cpu().numpy(), cnt.cpu().numpy(), err.cpu().numpy()


def _assert_hypotheses(P, pts, thr, seed, rn, first, count, what, rim_free=True):
    ref = plane_hypotheses(pts, thr, seed, rn, first, count)
    valid, plane, cnt, err = _hook(P, pts, thr, seed, rn, first, count)
    rel = np.abs(err - ref["err"]) / np.maximum(ref["err"], 1e-300)
    print(f"{what}: hypotheses [{first}, {first + count}) at ({thr}, seed {seed}, ransac_n {rn}): {int(ref['valid'].sum())} valid, {ref['rim']} rim pairs; device: "
          f"{int((valid != ref['valid']).sum())} other flags, {int((plane.view(np.uint64) != ref['plane'].view(np.uint64)).any(1).sum())} planes with other bits, "
          f"{int((cnt != ref['count']).sum())} other counts, err off by at most {rel.max():.1e} relative")
    assert ref["rim"] == 0 or not rim_free, what              # a condition of the comparison, not a result
    assert np.array_equal(valid, ref["valid"]), what
    assert np.array_equal(plane.view(np.uint64), ref["plane"].view(np.uint64)), what      # bit for bit
    assert np.array_equal(cnt, ref["count"]), what
    assert (rel <= 1e-12).all(), (what, float(rel.max()))
    return ref


def _assert_call(P, pts, case, what, ref=None, figures=None):
    """the call against the restatement: loop figures, count, index list, mask and the refit plane -> (reference, device plane, info)"""
    ref = ref or segment_plane_reference(pts, case[0], case[4], case[1], case[2], case[3])
    rc, plane, mask, idx, k, info = _raw(P, pts, case)
    ang, dd = plane_difference(plane, ref["plane"])
    print(f"{what} {case}: n = {len(pts)}; reference count {ref['count']} at iteration {ref['best_iteration']} of {ref['iterations_run']} run, {ref['n_valid']} valid, "
          f"{ref['rim']} rim, {ref['near']} near; device count {info.n_inliers} at {info.best_iteration} of {info.iterations_run}, {info.n_valid} valid; "
          f"refit off by {ang:.2e} rad, {dd:.2e} m")
    assert rc == 0
    assert ref["rim"] == 0 and ref["near"] == 0, what         # conditions of the comparison
    if figures is not None:
        assert (ref["count"], ref["best_iteration"], ref["iterations_run"], ref["n_valid"]) == figures, what
    assert (info.iterations_run, info.best_iteration, info.n_valid, info.n_inliers, k) == (ref["iterations_run"], ref["best_iteration"], ref["n_valid"], ref["count"], ref["count"]), what
    assert np.array_equal(idx[:k], ref["inliers"]), what
    assert np.array_equal(np.nonzero(mask)[0], ref["inliers"]) and set(np.unique(mask)) <= {0, 1}, what
    assert info.fitness == ref["count"] / len(pts) and abs(info.inlier_rmse - ref["rmse"]) <= 1e-12 * ref["rmse"], what
    assert ang <= TOL_RAD and dd <= TOL_D, (what, ang, dd)
    return ref, plane, info


# ---------------------------------------------------------------------------------------------------- main input
@pytest.fixture(scope="module")
def points(small_pair):
    pts = np.ascontiguousarray(small_pair["source"][::2], dtype=np.float32)
    assert pts.shape == (8263, 3)
    return pts


@pytest.fixture(scope="module")
def moved(points):
    """the same scan 300 m from the origin (SURVEY.md hard part 3), rounded to float32: other points, compared against THEIR restatement"""
    return (points.astype(np.float64) + OFFSET).astype(np.float32)


@pytest.fixture(scope="module")
def references(points):
    """{case: restatement}, filled on first use and left unchanged"""
    cache = {}

    def get(case):
        if case not in cache:
            cache[case] = segment_plane_reference(points, case[0], case[4], case[1], case[2], case[3])
        return cache[case]
    return get


@pytest.mark.parametrize("thr,seed,rn", HOOK, ids=[f"n{c[2]}" for c in HOOK])
def test_hypotheses_equal_the_restatement(P, points, thr, seed, rn):
    _assert_hypotheses(P, points, thr, seed, rn, 0, 1000, "main input")


@pytest.mark.parametrize("case", list(MAIN), ids=["-".join(str(v) for v in c) for c in MAIN])
def test_call_equals_the_sequential_loop(P, points, references, case):
    _assert_call(P, points, case, "main input", references(case), MAIN[case])


def test_round_constant_is_crossed_by_the_cases():
    run = {c: MAIN[c][2] for c in MAIN}
    best = {c: MAIN[c][1] for c in MAIN}
    assert any(PS_ROUND < r < c[1] for c, r in run.items())              # one loop ends inside a later round than the first
    assert any(b >= PS_ROUND for b in best.values())                      # one best hypothesis lies in a later round


@pytest.mark.parametrize("case", list(MOVED), ids=["-".join(str(v) for v in c) for c in MOVED])
def test_offset_cloud_at_nclt_scale_coordinates(P, moved, case):
    ref, plane, _ = _assert_call(P, moved, case, "offset input", figures=MOVED[case])
    assert abs(plane[3]) > 20.0


@pytest.mark.parametrize("n", list(FIRST))
def test_small_clouds_and_partial_wavefronts(P, points, n):
    """the first n points: with 3 points six draws with a repeated row come first (invalid hypotheses use up iterations); fitness 1 stops at once"""
    _assert_call(P, points[:n], (0.1, 50, 0.999, 2, 3), f"first {n} points", figures=FIRST[n])


def test_two_runs_give_identical_bits(P, points):
    case = (0.1, 1000, 0.999, 7, 3)
    a, b = _raw(P, points, case), _raw(P, points, case)
    assert a[0] == 0 and b[0] == 0 and a[4] == b[4]
    assert np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64)) and np.array_equal(a[2], b[2]) and np.array_equal(a[3][:a[4]], b[3][:b[4]])
    assert bytes(a[5]) == bytes(b[5])


def test_another_seed_gives_another_best_iteration(P, points, references):
    a = _assert_call(P, points, (0.1, 1000, 0.999, 7, 3), "seed 7", references((0.1, 1000, 0.999, 7, 3)))[2]
    b = _assert_call(P, points, (0.1, 1000, 0.999, 8, 3), "seed 8")[2]
    assert a.best_iteration != b.best_iteration


def test_permuted_rows_are_compared_against_their_own_reference(P, points, references):
    order = np.random.default_rng(11).permutation(len(points))
    ref, _, info = _assert_call(P, np.ascontiguousarray(points[order]), (0.1, 1000, 0.999, 7, 3), "permuted rows")
    base = references((0.1, 1000, 0.999, 7, 3))
    assert (ref["best_iteration"], ref["count"]) != (base["best_iteration"], base["count"])       # the sampler draws ROWS: another loop


# ------------------------------------------------------------------------------------------------ constructed inputs
def _lattice(z=2.0, side=16):
    g = np.arange(side, dtype=np.float32)
    xy = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
    return np.concatenate([xy, np.full((len(xy), 1), z, np.float32)], 1).astype(np.float32)


def test_lattice_plane_is_exact_and_stops_after_one_iteration(P):
    pts = _lattice()
    seed = next(s for s in range(100) if plane_from_sample([tuple(map(float, pts[r])) for r in sample_rows(s, 3, 0, len(pts))])[0])
    ref, plane, info = _assert_call(P, pts, (0.01, 100, 0.99999999, seed, 3), "16 x 16 lattice at z = 2")
    assert (info.best_iteration, info.iterations_run, info.n_inliers) == (0, 1, 256)
    assert plane.tolist() in ([0.0, 0.0, 1.0, -2.0], [0.0, 0.0, -1.0, 2.0])


def test_collinear_points_have_no_plane(P):
    t = np.arange(50, dtype=np.float32)[:, None]
    pts = t * np.array([[1.0, 2.0, 3.0]], np.float32)
    rc, plane, mask, idx, k, info = _raw(P, pts, (0.1, 100, 0.999, 3, 3))
    assert rc == 0 and plane.tolist() == [0.0] * 4 and k == 0 and not mask.any()
    assert (info.best_iteration, info.iterations_run, info.n_valid, info.n_inliers, info.fitness, info.inlier_rmse) == (-1, 100, 0, 0, 0.0, 0.0)
    valid, planes, cnt, err = _hook(P, pts, 0.1, 3, 3, 0, 64)
    assert not valid.any() and (cnt == -1).all() and not planes.any() and not err.any()
    rc, plane, mask, idx, k, info = _raw(P, pts, (0.1, 0, 0.999, 3, 3))          # num_iterations == 0: the empty result too
    assert rc == 0 and plane.tolist() == [0.0] * 4 and k == 0 and not mask.any() and (info.best_iteration, info.iterations_run) == (-1, 0)


def test_uniform_points_in_a_cube(P):
    pts = np.random.default_rng(3).uniform(-1, 1, (2000, 3)).astype(np.float32)
    ref, _, _ = _assert_call(P, pts, (0.05, 300, 0.999, 4, 3), "2 000 uniform points")
    assert ref["count"] == 152 and ref["iterations_run"] == 300              # no structure: no early stop


def _slab():
    """a 16 x 16 lattice on z = 0 and, above and below four of its points, points at exactly thr = 0.5 and one float32 ulp inside"""
    base = _lattice(0.0)
    inside = float(np.nextafter(np.float32(0.5), np.float32(0.0)))
    extra = [[x, y, s * z] for (x, y) in ((2, 3), (5, 11), (9, 4), (13, 13)) for s in (1.0, -1.0) for z in (0.5, inside)]
    return np.concatenate([base, np.array(extra, np.float32)]), 0.5


def test_a_point_at_exactly_the_threshold_is_not_an_inlier(P):
    pts, thr = _slab()
    ref = _assert_hypotheses(P, pts, thr, 1, 3, 0, 128, "slab", rim_free=False)
    flat = (np.abs(ref["plane"][:, 2]) == 1.0) & (ref["plane"][:, 3] == 0.0) & (ref["valid"] == 1)      # three lattice points: the plane z = 0 exactly
    assert flat.sum() >= 32 and (ref["count"][flat] == 256 + 8).all()          # the eight points one ulp inside, not the eight at 0.5
    for h in np.nonzero(flat)[0][:2]:
        d = plane_dist(ref["plane"][h], *pts.astype(np.float64).T)
        assert (d[256:] == np.abs(pts[256:, 2].astype(np.float64))).all() and (d == thr).sum() == 8
    case = (thr, 100, 0.999, 1, 3)
    r = segment_plane_reference(pts, *[case[k] for k in (0, 4, 1, 2, 3)])
    rc, plane, mask, idx, k, info = _raw(P, pts, case)
    assert rc == 0 and (info.iterations_run, info.best_iteration, info.n_valid, k) == (r["iterations_run"], r["best_iteration"], r["n_valid"], r["count"])
    assert np.array_equal(idx[:k], r["inliers"])


def _fma_cases(count=8, seed=21):
    """Clouds of four float32 points p0, p1, p2, q with a threshold that separates the two ways of forming dist(q) against the plane of a
    hypothesis that samples three distinct rows of p0, p1, p2: rounded one by one (the rule) and contracted (fma(c, z, fma(b, y, a x)) + d, what a compiler left to
    itself emits), which differ by one ulp there.  thr equals the larger of the two, so the smaller is an inlier and the larger is not.
    -> [(points, thr, iteration, inlier by the rule, inlier if contracted)]; the contracted value is formed in rationals, rounded once per fma."""
    rng = np.random.default_rng(seed)
    it = next(i for i in range(1000) if sorted(sample_rows(5, 3, i, 4)) == [0, 1, 2])       # n = 4 and the seed fix the rows of every iteration
    out = []
    for _ in range(100000):
        tri = rng.uniform(-2.0, 2.0, (3, 3)).astype(np.float32)
        q = rng.uniform(-2.0, 2.0, 3).astype(np.float32)
        pts = np.concatenate([tri, q[None]])
        ok, (a, b, c, d) = plane_from_sample([tuple(map(float, pts[r])) for r in sample_rows(5, 3, it, 4)])
        if not ok:
            continue
        x, y, z = (float(v) for v in q)
        plain = abs(((a * x + b * y) + c * z) + d)
        t = float(Fraction(b) * Fraction(y) + Fraction(a * x))
        t = float(Fraction(c) * Fraction(z) + Fraction(t))
        fused = abs(t + d)
        if plain == fused or min(plain, fused) < 0.05:
            continue
        top = max(plain, fused)
        if sum(1 for o in out if o[3] == (plain < top)) >= count // 2:      # both directions are wanted
            continue
        out.append((pts, top, it, plain < top, fused < top))
        if len(out) == count:
            return out
    raise AssertionError("no such clouds found")


def test_distance_is_formed_without_fused_multiply_add(P):
    cases = _fma_cases()
    assert {(a, b) for _, _, _, a, b in cases} == {(True, False), (False, True)}
    for pts, thr, it, by_rule, contracted in cases:
        ref = _assert_hypotheses(P, pts, thr, 5, 3, it, 1, f"point at the rim, inlier by the rule: {by_rule}", rim_free=False)
        assert ref["valid"][0] == 1 and ref["count"][0] == (4 if by_rule else 3)      # the restatement follows the rule ...
        assert by_rule != contracted                                                   # ... which a contracted sum would not


@pytest.mark.parametrize("n", [PS_TILE - 1, PS_TILE, PS_TILE + 1, PS_SPLIT_ROWS - 1, PS_SPLIT_ROWS, PS_SPLIT_ROWS + 1, 2 * PS_SPLIT_ROWS + 1])
def test_tile_and_split_boundaries(P, points, n):
    """one LDS tile less one row, exactly, plus one; the same around the rows of one split (one row more: a second split), and three splits"""
    _assert_hypotheses(P, points[:n], 0.1, 2, 3, 0, 8, f"first {n} points")
    _assert_call(P, points[:n], (0.1, 50, 0.999, 2, 3), f"first {n} points")


def test_more_rows_than_the_splits_hold(P):
    """from PS_MAX_SPLITS * PS_SPLIT_ROWS points on a lane walks more than PS_SPLIT_ROWS rows, in several tiles: one point more than that"""
    n = PS_MAX_SPLITS * PS_SPLIT_ROWS + 1
    rng = np.random.default_rng(17)
    pts = rng.uniform(-20, 20, (n, 3))
    pts[: n // 2, 2] = 0.02 * pts[: n // 2, 0] - 1.0 + rng.normal(0, 0.02, n // 2)          # half of them on a tilted plane with 2 cm of noise
    pts = pts[rng.permutation(n)].astype(np.float32)
    _assert_hypotheses(P, pts, 0.05, 2, 3, 0, 4, f"{n} points")
    ref, _, _ = _assert_call(P, pts, (0.05, 40, 0.999, 6, 3), f"{n} points")
    assert ref["count"] > n // 3


# ---------------------------------------------------------------------------------------------------- Python layer
def test_python_layer(P, points, references):
    import torch
    case = (0.1, 1000, 0.999, 7, 3)
    ref = references(case)
    pc = P.PointCloud(points)
    plane, inliers = pc.segment_plane(0.1, 3, 1000, 0.999, 7)
    assert isinstance(plane, np.ndarray) and plane.dtype == np.float64 and plane.shape == (4,) and isinstance(inliers, list) and isinstance(inliers[0], int)
    assert inliers == ref["inliers"].tolist()
    plane2, inliers2 = pc.segment_plane(distance_threshold=0.1, ransac_n=3, num_iterations=1000, probability=0.999, seed=7)
    assert np.array_equal(plane, plane2) and inliers == inliers2
    d100 = pc.segment_plane(0.1, seed=1)                                        # defaults: 3 points, 100 iterations, probability 0.99999999
    r100 = segment_plane_reference(points, 0.1, 3, 100, 0.99999999, 1)
    assert d100[1] == r100["inliers"].tolist() and r100["rim"] == 0 and r100["near"] == 0
    pn, inl = pc.segment_plane(0.1)                                             # seed=None: some seed
    assert len(inl) >= 3 and abs(np.linalg.norm(pn[:3]) - 1.0) < 1e-15
    dp, di, info = P.geometry._segment_plane(pc, 0.1, 3, 1000, 0.999, 7)
    assert di.is_cuda and di.dtype == torch.int64 and info["mask"].is_cuda and np.array_equal(dp, plane) and np.array_equal(di.cpu().numpy(), ref["inliers"])
    assert (info["iterations_run"], info["best_iteration"], info["n_valid"], info["n_inliers"]) == (ref["iterations_run"], ref["best_iteration"], ref["n_valid"], ref["count"])
    # remove_plane: the complement, a numpy selection on the REFERENCE inliers
    rest, plane3, removed = P.remove_plane(pc, 0.1, 3, 1000, 0.999, 7)
    keep = np.setdiff1d(np.arange(len(points)), ref["inliers"])
    assert removed.is_cuda and np.array_equal(removed.cpu().numpy(), ref["inliers"]) and np.array_equal(plane3, plane)
    assert np.array_equal(rest.points.astype(np.float32), points[keep])
    before, after = pc.cluster_dbscan(0.5, 10), rest.cluster_dbscan(0.5, 10)
    assert before.shape == (len(points),) and after.shape == (len(keep),)
    for name, lab in (("with the ground", before), ("without it", after)):
        sizes = np.bincount(lab[lab >= 0]) if (lab >= 0).any() else np.zeros(1, int)
        print(f"cluster_dbscan(0.5, 10) {name}: {lab.max() + 1} clusters, the largest of {sizes.max()} points, {int((lab < 0).sum())} noise")


# ----------------------------------------------------------------------------------------------------------- errors
def test_invalid_arguments_return_einval_with_a_message(P, points):
    ctx = P._lib.Context.current()
    pts = points[:50]
    good = (0.1, 50, 0.999, 2, 3)
    bad = [(dict(), (0.1, 50, 0.999, 2, 2)), (dict(), (0.1, 50, 0.999, 2, 9)), (dict(n=2), good), (dict(n=2 ** 31), good), (dict(n=-1), good), (dict(xyz=False), good),
           (dict(plane=False), good), (dict(params=False), good), (dict(), (-0.1, 50, 0.999, 2, 3)), (dict(), (float("nan"), 50, 0.999, 2, 3)),
           (dict(), (float("inf"), 50, 0.999, 2, 3)), (dict(), (0.1, -1, 0.999, 2, 3)), (dict(), (0.1, 50, 0.0, 2, 3)), (dict(), (0.1, 50, 1.5, 2, 3)),
           (dict(), (0.1, 50, float("nan"), 2, 3))]
    for kw, case in bad:
        rc = _raw(P, pts, case, **kw)[0]
        msg = ctx.lib.pcr_last_error(ctx.handle).decode()
        assert rc == EINVAL and "segment_plane" in msg, (kw, case, rc, msg)
    for kw in (dict(ransac_n=2), dict(num_iterations=-1), dict(probability=0.0), dict(distance_threshold=-1.0)):
        args = dict(distance_threshold=0.1, seed=1); args.update(kw)
        with pytest.raises(RuntimeError, match="segment_plane"):
            P.PointCloud(pts).segment_plane(**args)
    with pytest.raises(RuntimeError, match="segment_plane"):
        P.PointCloud(pts[:2]).segment_plane(0.1)
    # a valid call on the same context afterwards; the optional outputs may be null
    ref, plane, _ = _assert_call(P, pts, good, "after the errors")
    rc, plane2, mask, idx, k, info = _raw(P, pts, good, mask=False, index=False, count=False, info=False)
    assert rc == 0 and np.array_equal(plane2.view(np.uint64), plane.view(np.uint64)) and (mask == 9).all() and (idx == -7).all() and k == -7
    rc, plane2, mask, idx, k, info = _raw(P, pts, good, index=False)
    assert rc == 0 and k == ref["count"] and np.array_equal(np.nonzero(mask)[0], ref["inliers"]) and (idx == -7).all()
