"""DBSCAN on the device against the float64 restatement of Open3D's ClusterDBSCAN (dbscan_reference.py) on the same float32 points: the labels
of EVERY row, the core mask and the cluster count.

The six rules (include/pcr_hip.h) fix every label, and the device forms d^2 in the restatement's order without fused multiply-adds, so the
comparison is equality with no row left out.  What could still differ is a pair whose d^2 is within rounding of eps^2 -- there is none: the
restatement counts the pairs with |d^2 - eps^2| <= 1e-9 eps^2 (an exact tie is decided and is not one of them), and the tests assert that the
count is zero on every input they compare (but the integer lattice, which puts d^2 = 1 one ulp below eps^2 on purpose, and the constructed pairs
whose d^2 lands on eps^2 or one ulp below it depending on whether the sums are fused: d^2 has the restatement's bits, so those are decided too).  A rim pair could merge two clusters, so there is no exclusion share.

Main input: every second point of the source of golden pair 899 (8,263 points, no library call in front of it) at four parameter sets:
35 / 557 / 34 / 102 clusters, and 1 / 74 / 30 / 0 border rows within reach of more than one cluster."""
import ctypes as C

import numpy as np
import pytest

from conftest import pkg
from dbscan_reference import dbscan_reference

pytestmark = pytest.mark.gpu

CASES = [(0.5, 10), (0.3, 4), (1.0, 20), (0.8, 3)]          # (eps, min_points)
OFFSET = np.array([300.0, -150.0, 20.0])
EINVAL = -1


@pytest.fixture(scope="module")
def P():
    return pkg()


def _raw(P, pts, eps, min_points, labels=True, core=True, count=True, xyz=True, n=None):
    """pcr_cluster_dbscan itself -> (status, labels int32 (n,), core bool (n,), cluster count); a False switch passes a null pointer"""
    import torch
    ctx = P._lib.Context.current()
    pts = np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 3)
    rows = len(pts)
    d = torch.from_numpy(pts).cuda()
    lab = torch.full((max(rows, 1),), -7, dtype=torch.int32, device="cuda")
    cm = torch.full((max(rows, 1),), 9, dtype=torch.uint8, device="cuda")
    m = C.c_int64(-7)
    rc = ctx.lib.pcr_cluster_dbscan(ctx.handle, C.c_void_p(d.data_ptr()) if xyz and rows else None, C.c_int64(rows if n is None else n), C.c_double(eps),
                                    C.c_int(min_points), C.c_void_p(lab.data_ptr()) if labels else None, C.c_void_p(cm.data_ptr()) if core else None,
                                    C.byref(m) if count else None)
    return rc, lab[:rows].cpu().numpy(), cm[:rows].cpu().numpy(), int(m.value)


def _assert_equal(P, pts, eps, min_points, what, ref=None, rim_free=True):
    """rim_free=False: only where a test PUTS pairs next to eps^2 on purpose (the lattice); d^2 has the restatement's bits, so they are decided too"""
    ref = ref or dbscan_reference(pts, eps, min_points)
    rc, lab, core, m = _raw(P, pts, eps, min_points)
    wrong = int((lab != ref["labels"]).sum())
    print(f"{what} ({eps}, {min_points}): n = {len(ref['labels'])}; reference {ref['n_clusters']} clusters, {int(ref['core'].sum())} core, "
          f"{int((ref['labels'] < 0).sum())} noise, {ref['shared_border']} shared border rows, {ref['rim_pairs']} rim pairs; device {m} clusters, "
          f"{int((core == 1).sum())} core, {wrong} rows with another label")
    assert rc == 0
    assert ref["rim_pairs"] == 0 or not rim_free, what          # a condition of the comparison, not a result
    assert np.array_equal(core, ref["core"].astype(np.uint8)), (what, int((core != ref["core"]).sum()))
    assert m == ref["n_clusters"], what
    assert np.array_equal(lab, ref["labels"]), (what, wrong)   # every row
    return ref, lab


# ---------------------------------------------------------------------------------------------------- main input
@pytest.fixture(scope="module")
def points(small_pair):
    pts = np.ascontiguousarray(small_pair["source"][::2], dtype=np.float32)
    assert pts.shape == (8263, 3)
    return pts


@pytest.fixture(scope="module")
def references(points):
    """{case: restatement}, computed once and left unchanged"""
    return {c: dbscan_reference(points, *c) for c in CASES}


@pytest.mark.parametrize("case", CASES, ids=[f"{c[0]}-{c[1]}" for c in CASES])
def test_labels_core_mask_and_count_equal_the_restatement_on_every_row(P, points, references, case):
    ref, _ = _assert_equal(P, points, case[0], case[1], "main input", references[case])
    assert ref["n_clusters"] >= 30 and (ref["labels"] < 0).any() and (~ref["core"] & (ref["labels"] >= 0)).any()      # clusters, noise and border rows


def test_the_main_input_has_border_rows_in_reach_of_several_clusters(references):
    shared = {c: references[c]["shared_border"] for c in CASES}
    print("border rows with more than one candidate cluster:", shared)
    assert all(references[c]["rim_pairs"] == 0 for c in CASES)
    assert max(shared.values()) >= 1


@pytest.mark.parametrize("case", [(0.5, 10), (0.3, 4)], ids=["0.5-10", "0.3-4"])
def test_offset_cloud_at_nclt_scale_coordinates(P, points, case):
    """the same scan 300 m from the origin (SURVEY.md hard part 3), rounded to float32: other points, compared against THEIR restatement"""
    moved = (points.astype(np.float64) + OFFSET).astype(np.float32)
    _assert_equal(P, moved, case[0], case[1], "offset input")


def test_numbering_follows_caller_rows_not_morton_order(P, points, references):
    order = np.random.default_rng(11).permutation(len(points))
    shuffled = np.ascontiguousarray(points[order])
    ref, lab = _assert_equal(P, shuffled, 0.3, 4, "permuted rows")
    # the same partition as the unpermuted input, renumbered: the clusters' seeds are other rows now
    base = references[(0.3, 4)]["labels"][order]
    assert ref["n_clusters"] == references[(0.3, 4)]["n_clusters"] and not np.array_equal(base, lab)
    core = ref["core"]
    pairs = np.unique(np.stack([base[core], lab[core]], 1), axis=0)
    assert len(pairs) == ref["n_clusters"]                     # one-to-one on the core rows
    seeds = np.array([np.nonzero(core & (lab == k))[0].min() for k in range(ref["n_clusters"])])
    assert (np.diff(seeds) > 0).all()                          # label k's first core row comes before label k + 1's


def test_two_runs_give_identical_labels(P, points):
    a = _raw(P, points, 0.3, 4)
    b = _raw(P, points, 0.3, 4)
    assert a[0] == 0 and b[0] == 0 and a[3] == b[3]
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


# ------------------------------------------------------------------------------------------------------ strictness
def _lattice():
    g = np.arange(4, dtype=np.float32)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)


def test_a_pair_at_exactly_eps_is_not_a_neighbour(P):
    pts = _lattice()
    rc, lab, core, m = _raw(P, pts, 1.0, 2)
    assert rc == 0 and m == 0 and (lab == -1).all() and (core == 0).all()       # d^2 = 1 is not below 1: every point is alone


@pytest.mark.parametrize("min_points", [4, 5, 7])
def test_lattice_just_above_the_spacing(P, min_points):
    """eps one ulp above 1: the six axis neighbours are members.  A corner has 4 members, an edge point 5, a face point 6, an inner point 7."""
    pts = _lattice()
    inner = ((pts > 0) & (pts < 3)).sum(1)                      # 3: inner, 2: face, 1: edge, 0: corner
    ref, lab = _assert_equal(P, pts, float(np.nextafter(1.0, 2.0)), min_points, "4 x 4 x 4 lattice", rim_free=False)
    if min_points == 4:
        assert ref["n_clusters"] == 1 and (lab == 0).all() and ref["core"].all()
    elif min_points == 5:
        assert (lab == 0).all() and np.array_equal(ref["core"], inner > 0)        # the corners are border points
    else:
        assert np.array_equal(ref["core"], inner == 3) and np.array_equal(lab >= 0, inner >= 2)      # face points border, edges and corners noise
        assert ref["n_clusters"] == 1


# ------------------------------------------------------------------------------------------------ no fused multiply-add
def _fma_pairs(count=8, seed=21):
    """`count` pairs of float32 points, each with an eps whose float64 square separates the two ways of forming d^2: rounded one by one
    (dx dx, += dy dy, += dz dz: the rule) and contracted (fma(dz, dz, fma(dy, dy, dx dx)), what a compiler left to itself emits), which differ
    by one ulp there.  eps^2 equals the larger of the two, so the smaller is a member and the larger is not.  -> [(p, q, eps, member by the
    rule, member if contracted)]; the contracted value is formed exactly, in rationals, and rounded once per fma."""
    from fractions import Fraction
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(100000):
        p = rng.uniform(-2.0, 2.0, 3).astype(np.float32)
        q = (p + rng.uniform(-0.4, 0.4, 3)).astype(np.float32)
        dx, dy, dz = (float(v) for v in (p.astype(np.float64) - q.astype(np.float64)))
        plain = dx * dx
        plain += dy * dy
        plain += dz * dz
        fused = float(Fraction(dz) * Fraction(dz) + Fraction(float(Fraction(dy) * Fraction(dy) + Fraction(dx * dx))))
        if plain == fused:
            continue
        top = max(plain, fused)
        eps = next((e for e in (float(np.sqrt(top)), float(np.nextafter(np.sqrt(top), 0.0)), float(np.nextafter(np.sqrt(top), 9.0))) if e * e == top), None)
        if eps is None:
            continue
        # both directions are wanted: the rule says member and a contraction would not, and the other way round
        if sum(1 for o in out if o[3] == (plain < top)) >= count // 2:
            continue
        out.append((p, q, eps, plain < top, fused < top))
        if len(out) == count:
            return out
    raise AssertionError("no such pairs found")


def test_d2_is_formed_without_fused_multiply_add(P):
    """Two points whose d^2 lands on eps^2 or one ulp below it depending on whether the sums are contracted: with min_points = 2 the pair is one
    cluster of two core points or two noise points.  The lattice cannot tell (its products are exact); these coordinates have inexact squares."""
    pairs = _fma_pairs()
    assert {(a, b) for _, _, _, a, b in pairs} == {(True, False), (False, True)}
    for p, q, eps, by_rule, contracted in pairs:
        pts = np.stack([p, q])
        ref, lab = _assert_equal(P, pts, eps, 2, f"pair at the rim, member by the rule: {by_rule}", rim_free=False)
        assert ref["core"].all() == by_rule and (ref["n_clusters"] == 1) == by_rule      # the restatement follows the rule ...
        assert by_rule != contracted                                                  # ... which a contracted sum would not


# ----------------------------------------------------------------------------------------------------------- chain
def _chain(gap_at=None, n=3000, eps=0.5):
    x = np.arange(n, dtype=np.float64) * (0.9 * eps)
    if gap_at is not None:
        x[gap_at:] += (1.01 - 0.9) * eps                        # one gap of 1.01 eps
    pts = np.zeros((n, 3))
    pts[:, 0] = x
    order = np.random.default_rng(5).permutation(n)
    return pts[order].astype(np.float32), order


def test_one_component_across_a_hundred_workgroups(P):
    """3,000 points on a line 0.9 eps apart, rows shuffled, min_points = 3: one cluster of every point; the two ends have two members and are
    border points, not noise.  A query octet per 8 points and 32 octets per workgroup: the component spans 94 workgroups' unions."""
    pts, order = _chain()
    ref, lab = _assert_equal(P, pts, 0.5, 3, "chain")
    assert ref["n_clusters"] == 1 and (lab == 0).all()
    ends = np.isin(order, [0, len(order) - 1])
    assert np.array_equal(~ref["core"], ends)


def test_a_gap_of_1_01_eps_splits_the_chain(P):
    pts, order = _chain(gap_at=1500)
    ref, lab = _assert_equal(P, pts, 0.5, 3, "chain with a gap")
    assert ref["n_clusters"] == 2
    assert np.array_equal(lab == lab[order == 0][0], order < 1500)            # the two halves
    first_core = np.nonzero(ref["core"])[0].min()
    assert lab[first_core] == 0                                               # label 0: the half with the smaller core row
    assert np.array_equal(~ref["core"], np.isin(order, [0, 1499, 1500, 2999]))


# ------------------------------------------------------------------------------------------- shared border by construction
def test_a_point_in_reach_of_two_clusters_takes_the_smaller_label(P):
    """Two rows of ten points 0.1 apart, ending at x = 0 and starting at x = 0.6, and a lone point at x = 0.3; eps = 0.35, min_points = 4: the
    ends at 0 and 0.6 are core (4 members), the lone point has 3 members and is in reach of one core point of each row."""
    a = np.zeros((10, 3)); a[:, 0] = -0.1 * np.arange(10)
    b = np.zeros((10, 3)); b[:, 0] = 0.6 + 0.1 * np.arange(10)
    lone = np.array([[0.3, 0.0, 0.0]])
    for first, second, what in ((a, b, "a first"), (b, a, "b first")):
        pts = np.concatenate([first, second, lone]).astype(np.float32)
        ref, lab = _assert_equal(P, pts, 0.35, 4, f"two rows and a lone point, {what}")
        assert ref["n_clusters"] == 2 and ref["shared_border"] == 1 and not ref["core"][20]
        assert (lab[:10] == 0).all() and (lab[10:20] == 1).all() and lab[20] == 0      # the lone point goes with whichever row comes first


# ------------------------------------------------------------------------------------------ smallest and degenerate shapes
def test_one_point(P):
    one = np.array([[1.5, -2.0, 0.25]], np.float32)
    rc, lab, core, m = _raw(P, one, 0.5, 1)
    assert (rc, lab.tolist(), core.tolist(), m) == (0, [0], [1], 1)
    rc, lab, core, m = _raw(P, one, 0.5, 2)
    assert (rc, lab.tolist(), core.tolist(), m) == (0, [-1], [0], 0)


def test_fewer_points_than_an_octet(P):
    pts = np.random.default_rng(2).random((7, 3)).astype(np.float32)
    for mp in (1, 2, 3):
        _assert_equal(P, pts, 0.5, mp, "7 points")


@pytest.mark.parametrize("n", [9, 63, 65, 257])
def test_partial_octets_wavefronts_and_a_second_workgroup(P, points, n):
    """the first n points of the main input: a partial last octet (9, 63, 65, 257), a partial last wavefront and, at 257, a second workgroup"""
    _assert_equal(P, points[:n], 0.5, 4, f"first {n} points")


def test_coincident_points(P):
    pts = np.tile(np.array([[3.0, 1.0, -2.0]], np.float32), (20, 1))
    rc, lab, core, m = _raw(P, pts, 0.1, 20)
    assert rc == 0 and m == 1 and (lab == 0).all() and (core == 1).all()
    rc, lab, core, m = _raw(P, pts, 0.1, 21)
    assert rc == 0 and m == 0 and (lab == -1).all() and (core == 0).all()


def test_isolated_points_are_numbered_by_row(P):
    pts = (np.random.default_rng(4).permutation(300)[:, None] * np.array([[1.0, 0.0, 0.0]]) + np.array([[0.0, 2.0, 1.0]])).astype(np.float32)
    rc, lab, core, m = _raw(P, pts, 0.9, 1)                     # every point alone and, with min_points = 1, a core point
    assert rc == 0 and m == 300 and (core == 1).all()
    assert np.array_equal(lab, np.arange(300))


def test_empty_cloud(P):
    rc, lab, core, m = _raw(P, np.zeros((0, 3), np.float32), 0.5, 3)
    assert rc == 0 and m == 0
    assert P.PointCloud().cluster_dbscan(0.5, 3).shape == (0,)


# ---------------------------------------------------------------------------------------------------- Python layer
def test_python_layer(P, points, references):
    case = (0.5, 10)
    ref = references[case]
    pc = P.PointCloud(points)
    rc, lab, core, m = _raw(P, points, *case)
    out = pc.cluster_dbscan(*case, print_progress=True)
    assert isinstance(out, np.ndarray) and out.dtype == np.int32 and out.shape == (len(points),)
    assert rc == 0 and np.array_equal(out, lab) and np.array_equal(out, np.asarray(pc.cluster_dbscan(eps=case[0], min_points=case[1])))
    dl, dc, dm = P.geometry._cluster_dbscan(pc, *case)
    assert dl.is_cuda and dc.is_cuda and dm == m and np.array_equal(dl.cpu().numpy(), lab) and np.array_equal(dc.cpu().numpy(), core.astype(bool))
    # remove_small_clusters: a numpy selection on the REFERENCE labels
    for size in (1, 40, 10 ** 6):
        sizes = np.bincount(ref["labels"][ref["labels"] >= 0], minlength=ref["n_clusters"])
        keep = (ref["labels"] >= 0) & (sizes[np.maximum(ref["labels"], 0)] >= size)
        kept, idx = P.remove_small_clusters(pc, case[0], case[1], size)
        idx = idx.cpu().numpy()
        print(f"remove_small_clusters(min_cluster_size = {size}): {len(idx)} of {len(points)} points kept")
        assert np.array_equal(idx, np.nonzero(keep)[0])
        assert np.array_equal(kept.points.astype(np.float32), points[idx])
    assert 0 < int(((ref["labels"] >= 0) & (sizes[np.maximum(ref["labels"], 0)] >= 40)).sum()) < int((ref["labels"] >= 0).sum())      # size 40 drops clusters, keeps others


# ----------------------------------------------------------------------------------------------------------- errors
def test_invalid_arguments_return_einval_with_a_message(P):
    ctx = P._lib.Context.current()
    pts = np.random.default_rng(6).random((50, 3)).astype(np.float32)
    bad = [dict(n=-1), dict(n=2 ** 31), dict(xyz=False), dict(labels=False),
           dict(eps=float("nan")), dict(eps=float("inf")), dict(eps=0.0), dict(eps=-0.5), dict(min_points=0), dict(min_points=-3)]
    for kw in bad:
        eps, mp = kw.pop("eps", 0.3), kw.pop("min_points", 3)
        rc = _raw(P, pts, eps, mp, **kw)[0]
        msg = ctx.lib.pcr_last_error(ctx.handle).decode()
        assert rc == EINVAL and "cluster_dbscan" in msg, (kw, eps, mp, rc, msg)
    with pytest.raises(RuntimeError, match="cluster_dbscan"):
        P.PointCloud(pts).cluster_dbscan(-1.0, 3)
    # a valid call on the same context afterwards; the optional outputs may be null
    _assert_equal(P, pts, 0.3, 3, "after the errors")
    rc, lab, core, m = _raw(P, pts, 0.3, 3, core=False, count=False)
    assert rc == 0 and (core == 9).all() and m == -7 and np.array_equal(lab, dbscan_reference(pts, 0.3, 3)["labels"])
