"""The Hybrid(r, max_nn) neighbour lists behind every FPFH row (k_radius_list and the pieces it hands to the k-best kernel), row by row
against the oracle's k-d tree (``pcr_debug_radius_lists``).

A device row is compared as a SET with the oracle's k + extra nearest, ranked by (float64 d^2, caller index):
  * rim: a point with |d^2 - r^2| <= 2^-20 r^2 may be in or out (the device tests float32 d^2 < float(r^2)); elsewhere the in-ball decision is exact;
  * a row holds min(k, ball) distinct valid indices, up to rim points;
  * overfull ball (more than k points): with D the oracle's k-th d^2, every point below D (1 - 2^-20) is in the row, none above D (1 + 2^-20);
  * exact ties: when every point of that band has d^2 exactly D, the row IS the oracle's row (lowest caller indices win), on every path.
Every case also asserts how many rows each path produced (append: ball <= k; select: ball > k and cnt == k; spill: cnt == -1), so that a
construction that stops reaching its path fails instead of passing by accident."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_fpfh_explained, pkg

EPS = 2.0 ** -20
EXTRA = 128                  # the oracle is asked for k + EXTRA: the ball size past k and the run of distances beyond the k-th place


@pytest.fixture(scope="module")
def P():
    return pkg()


@pytest.fixture
def list_select(P):
    """Sets pcr_set_option "radius_list_select" for the calls of one test (1: threshold selection, the default; 0: every overfull piece to
    the k-best kernel) and puts 1 back afterwards."""
    yield lambda v: P._lib.set_option("radius_list_select", v)
    P._lib.set_option("radius_list_select", 1)


# ------------------------------------------------------------------------------------------------------------ the comparison
def check_rows(pts, rows, idx, cnt, k, radius, ref_idx, ref_d2, ref_cnt):
    """Device rows `idx[rows]`, `cnt[rows]` (caller indices; cnt -1: scan all k slots) of cloud `pts` against the reference's k + extra
    nearest of the same queries (`ref_*`: one row per entry of `rows`, ranked by (float64 d^2, index)).  Returns a dict of counts; the
    list `bad` holds the rows that break a rule (empty when all hold)."""
    pts = np.asarray(pts, np.float32).astype(np.float64)
    rows = np.asarray(rows); n = len(pts); nq = len(rows); K2 = ref_idx.shape[1]
    r2 = float(radius) * float(radius)
    dev = np.asarray(idx)[rows].astype(np.int64)
    c = np.asarray(cnt)[rows]
    slot = np.arange(k)[None, :]
    valid = (dev >= 0) & ((c[:, None] < 0) | (slot < c[:, None]))
    in_range = np.where(valid, (dev >= 0) & (dev < n), True)
    dev = np.where(valid & in_range, dev, -1); valid &= in_range
    d2 = ((pts[np.where(valid, dev, 0)] - pts[rows][:, None, :]) ** 2).sum(-1)
    sd = np.sort(np.where(valid, dev, np.int64(1) << 40), axis=1)
    dup = ((sd[:, 1:] == sd[:, :-1]) & (sd[:, 1:] < (1 << 40))).any(1)
    size = valid.sum(1)
    ball_seen = ref_cnt.astype(np.int64)
    over = ball_seen > k
    rslot = np.arange(K2)[None, :]
    rvalid = rslot < ball_seen[:, None]
    D = np.where(over, ref_d2[:, k - 1], r2)
    rim_ref = rvalid & (np.abs(ref_d2 - r2) <= EPS * r2)
    # must: every reference point below the band (below the rim for a ball that fits)
    must = rvalid & (ref_d2 < D[:, None] * (1.0 - EPS)) & ~rim_ref
    rr = np.broadcast_to(np.arange(nq)[:, None], ref_idx.shape)
    dev_keys = np.arange(nq)[:, None] * (np.int64(n) + 1) + np.where(valid, dev, n)
    missing = must & ~np.isin(rr * (np.int64(n) + 1) + ref_idx, dev_keys[valid])
    # nothing above the band (above the rim for a ball that fits), nothing outside the ball
    hi = np.where(over, D * (1.0 + EPS), r2 * (1.0 + EPS))
    too_far = valid & ((d2 > hi[:, None]) | (d2 >= r2 * (1.0 + EPS)))
    # size: min(k, ball) up to rim points
    n_rim = rim_ref.sum(1)
    lo_size = np.minimum(k, ball_seen - n_rim)
    size_bad = (size < lo_size) | (size > np.minimum(k, ball_seen))
    # exact ties at the k-th place: the band seen in full and all of it at exactly D -> the reference's row itself
    band = rvalid & (np.abs(ref_d2 - D[:, None]) <= EPS * D[:, None])
    band_seen = (ball_seen < K2) | (ref_d2[:, K2 - 1] > D * (1.0 + EPS))
    exact = over & band_seen & (np.where(band, ref_d2 == D[:, None], True)).all(1) & ~(np.abs(D - r2) <= EPS * r2)
    ref_sorted = np.sort(np.where(slot < np.minimum(ball_seen, k)[:, None], ref_idx[:, :k], np.int64(1) << 40), axis=1)
    same = (sd == ref_sorted).all(1)
    tie_bad = exact & ~same
    bad_mask = dup | missing.any(1) | too_far.any(1) | size_bad | tie_bad
    return {"append": int((~over).sum()), "select": int((over & (c == k)).sum()), "spill": int((c == -1).sum()),
            "rows": nq, "differ": int((~same).sum()), "exact_tie_rows": int(exact.sum()),
            "bad": [int(rows[i]) for i in np.nonzero(bad_mask)[0]],
            "why": {"dup": int(dup.sum()), "missing": int(missing.any(1).sum()), "too_far": int(too_far.any(1).sum()),
                    "size": int(size_bad.sum()), "tie": int(tie_bad.sum())}}


def brute_knn(pts, queries, K2, radius):
    """numpy reference of oracle.knn: the K2 nearest with d^2 < r^2 by (float64 d^2, index)."""
    p = np.asarray(pts, np.float32).astype(np.float64); q = np.asarray(queries, np.float32).astype(np.float64)
    d2 = ((p[None, :, :] - q[:, None, :]) ** 2).sum(-1)
    order = np.lexsort((np.broadcast_to(np.arange(len(p)), d2.shape), d2), axis=1)
    sd = np.take_along_axis(d2, order, 1)
    cnt = (d2 < radius * radius).sum(1).clip(max=K2)
    idx = np.full((len(q), K2), -1, np.int64); dd = np.full((len(q), K2), np.inf)
    m = min(K2, len(p))
    idx[:, :m] = order[:, :m]; dd[:, :m] = sd[:, :m]
    slot = np.arange(K2)[None, :]
    idx = np.where(slot < cnt[:, None], idx, -1); dd = np.where(slot < cnt[:, None], dd, np.inf)
    return idx, dd, cnt.astype(np.int32)


def test_row_check_against_brute_force():
    """The comparison itself: rows built from a numpy brute force pass -- in append and in slot layout, shuffled, with exact ties broken by
    index -- and one swapped entry, a tie broken the other way or a duplicate is rejected."""
    rng = np.random.default_rng(3)
    g = np.stack(np.meshgrid(*[np.arange(6)] * 3, indexing="ij"), -1).reshape(-1, 3) * 0.125          # exact ties
    pts = np.concatenate([g, rng.uniform(0, 0.7, (150, 3)), np.repeat(g[:1], 20, 0)]).astype(np.float32)
    pts = pts[rng.permutation(len(pts))]
    n, k, radius = len(pts), 30, 0.2
    ref_idx, ref_d2, ref_cnt = brute_knn(pts, pts, k + EXTRA, radius)
    idx = np.full((n, k), -1, np.int32); cnt = np.zeros(n, np.int32)
    for i in range(n):
        m = min(k, ref_cnt[i])
        row = ref_idx[i, :m].copy(); rng.shuffle(row)
        if m == k and i % 2:
            cnt[i] = -1; idx[i] = row                                           # slot layout
        else:
            cnt[i] = m; idx[i, :m] = row; idx[i, m:] = rng.integers(0, n, k - m)  # append layout, junk past cnt
    rows = np.arange(n)
    ok = check_rows(pts, rows, idx, cnt, k, radius, ref_idx, ref_d2, ref_cnt)
    assert ok["bad"] == [] and ok["differ"] == 0 and ok["exact_tie_rows"] > 10, ok
    assert ok["append"] > 10 and ok["append"] + ok["select"] + ok["spill"] >= n

    def rejects(i, new_row):
        bad = idx.copy(); bad[i] = new_row; c2 = cnt.copy(); c2[i] = -1
        return i in check_rows(pts, rows, bad, c2, k, radius, ref_idx, ref_d2, ref_cnt)["bad"]

    over = np.nonzero(ref_cnt > k)[0]
    i = int(over[0])
    far = ref_idx[i, k + 5] if ref_cnt[i] > k + 5 else int(np.argmax(((pts - pts[i]) ** 2).sum(1)))
    assert rejects(i, np.r_[ref_idx[i, : k - 1], far])                                   # one entry swapped for a farther point
    assert rejects(i, np.r_[ref_idx[i, : k - 1], ref_idx[i, 0]])                         # a duplicate
    # a tie broken by the higher index: a row whose k-th place is an exact tie, the tied point of the next place instead
    tied = [j for j in over if ref_d2[j, k - 1] == ref_d2[j, k]]
    assert tied
    j = int(tied[0])
    assert rejects(j, np.r_[ref_idx[j, : k - 1], ref_idx[j, k]])
    # an append row that misses a point of a ball that fits
    small = int(np.nonzero((ref_cnt < k) & (ref_cnt > 3))[0][0])
    bad = idx.copy(); c2 = cnt.copy(); c2[small] = ref_cnt[small] - 1; bad[small, : c2[small]] = ref_idx[small, 1: ref_cnt[small]]
    assert small in check_rows(pts, rows, bad, c2, k, radius, ref_idx, ref_d2, ref_cnt)["bad"]


# ------------------------------------------------------------------------------------------------------------ device calls
def radius_lists(P, clouds, k, radius):
    """pcr_debug_radius_lists over `clouds` in one call (count = len(clouds)); rows and cnt per cloud, in caller order."""
    import torch
    ctx = P._lib.Context.current()
    m = len(clouds)
    d = [torch.from_numpy(np.ascontiguousarray(p, dtype=np.float32)).cuda() for p in clouds]
    idx = [torch.empty((len(p), k), dtype=torch.int32, device="cuda") for p in clouds]
    cnt = [torch.empty(len(p), dtype=torch.int32, device="cuda") for p in clouds]
    ptr = lambda ts: (C.c_void_p * m)(*[t.data_ptr() for t in ts])
    ctx.check(ctx.lib.pcr_debug_radius_lists(ctx.handle, C.c_int(m), ptr(d), (C.c_int64 * m)(*[len(p) for p in clouds]), C.c_int(k),
                                             C.c_double(radius), ptr(idx), ptr(cnt)), "debug_radius_lists")
    torch.cuda.synchronize()
    return [(i.cpu().numpy(), c.cpu().numpy()) for i, c in zip(idx, cnt)]


def compare(oracle, pts, idx, cnt, k, radius, rows=None, what="", extra=EXTRA):
    pts = np.ascontiguousarray(pts, np.float32)
    rows = np.arange(len(pts)) if rows is None else np.asarray(rows)
    ref_idx, ref_d2, ref_cnt = oracle.knn(pts, pts[rows], k + extra, radius)
    s = check_rows(pts, rows, idx, cnt, k, radius, ref_idx, ref_d2, ref_cnt)
    print(f"{what} k={k} r={radius}: rows {s['rows']}, append {s['append']}, select {s['select']}, spill {s['spill']}, "
          f"exact-tie rows {s['exact_tie_rows']}, differ from the oracle {s['differ']}, broken {len(s['bad'])} {s['why']}")
    assert not s["bad"], (what, k, s["why"], s["bad"][:10])
    return s


def lattice(m=25, h=0.125, seed=5):
    """m^3 grid of spacing h (exact in float32 and float64), caller order shuffled so that it differs from Morton order."""
    g = np.stack(np.meshgrid(*[np.arange(m)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float64) * h
    return g[np.random.default_rng(seed).permutation(len(g))].astype(np.float32)


def overflow_cloud(seed=11):
    """65 600 points in a 0.04 m cube around the origin (one exactly at it), 130 at d^2 in [3.2, 3.8] / 128 and 10 at [5.2, 5.8] / 128:
    one d^2 bin of 128 over r = 1 holds more than 65 535 points."""
    rng = np.random.default_rng(seed)
    cube = rng.uniform(-0.02, 0.02, (65600, 3)); cube[0] = 0.0

    def shell(cnt, lo, hi):
        v = rng.standard_normal((cnt, 3)); v /= np.linalg.norm(v, axis=1, keepdims=True)
        return v * np.sqrt(rng.uniform(lo, hi, cnt) / 128.0)[:, None]
    return np.concatenate([cube, shell(130, 3.2, 3.8), shell(10, 5.2, 5.8)]).astype(np.float32)


def duplicates(seed=13):
    rng = np.random.default_rng(seed)
    return np.concatenate([np.repeat(np.array([[0.3, -0.2, 0.1]]), 300, 0), rng.uniform(-0.6, 0.6, (50, 3))]).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- (a)
@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 20, 32, 33, 64, 65, 200])
def test_pair_raw(P, oracle, small_pair, k):
    pts = small_pair["source"].astype(np.float32)
    (idx, cnt), = radius_lists(P, [pts], k, 1.0)
    s = compare(oracle, pts, idx, cnt, k, 1.0, what="pair 899 raw")
    assert s["select"] >= 100 and s["append"] >= (100 if k >= 20 else 1), s


@pytest.mark.gpu
def test_pair_voxelised(P, oracle, small_pair):
    pts = P.PointCloud(small_pair["source"]).voxel_down_sample(0.1).points.astype(np.float32)
    (idx, cnt), = radius_lists(P, [pts], 200, 1.0)
    s = compare(oracle, pts, idx, cnt, 200, 1.0, what="pair 899 at 0.1")
    assert s["append"] >= 100 and s["select"] >= 10, s


# ---------------------------------------------------------------------------------------------------------------- (b) (c) (h)
@pytest.mark.gpu
@pytest.mark.parametrize("k,path", [(175, "select"), (200, "spill")])
@pytest.mark.parametrize("select", [1, 0])
def test_lattice_exact_ties(P, oracle, list_select, k, path, select):
    """25^3 lattice, r = 1 (8 spacings): for an interior query the 175th place falls in shell i^2+j^2+k^2 = 12 (171 below, 8 in it: no spill),
    the 200th in shell 13 (179 below, 24 in it: the piece spills).  Under select = 0 every overfull piece goes to the k-best kernel."""
    list_select(select)
    pts = lattice()
    (idx, cnt), = radius_lists(P, [pts], k, 1.0)
    s = compare(oracle, pts, idx, cnt, k, 1.0, what=f"lattice select={select}")
    assert s["exact_tie_rows"] >= 2000, s
    if select == 0:
        assert s["select"] == 0 and s["spill"] >= 2000, s
    elif path == "select":
        assert s["select"] >= 2000, s
    else:
        assert s["spill"] >= 2000, s
    assert s["differ"] <= s["rows"] - s["exact_tie_rows"], s


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["pair", "lattice175", "lattice200"])
def test_select_off_gives_the_same_sets(P, small_pair, list_select, case):
    """(h) radius_list_select 0 against 1: the same set on every row."""
    pts, k = {"pair": (small_pair["source"].astype(np.float32), 200), "lattice175": (lattice(), 175), "lattice200": (lattice(), 200)}[case]
    out = []
    for v in (1, 0):
        list_select(v)
        (idx, cnt), = radius_lists(P, [pts], k, 1.0)
        valid = (idx >= 0) & ((cnt[:, None] < 0) | (np.arange(k)[None, :] < cnt[:, None]))
        out.append(np.sort(np.where(valid, idx, np.iinfo(np.int32).max), axis=1))
    diff = (out[0] != out[1]).any(1)
    assert not diff.any(), (int(diff.sum()), np.nonzero(diff)[0][:10])


# ---------------------------------------------------------------------------------------------------------------- (d) (e) (f)
@pytest.mark.gpu
@pytest.mark.parametrize("select", [1, 0])
@pytest.mark.parametrize("k", [20, 200])
def test_duplicates(P, oracle, list_select, k, select):
    """300 copies of one point: every distance at the k-th place ties at 0."""
    list_select(select)
    pts = duplicates()
    (idx, cnt), = radius_lists(P, [pts], k, 1.0)
    s = compare(oracle, pts, idx, cnt, k, 1.0, what=f"duplicates select={select}", extra=len(pts) - k)        # (the whole tie in view)
    assert s["exact_tie_rows"] >= 300 and s["spill"] >= 300, s


@pytest.mark.gpu
def test_bin_counter_overflow(P, oracle):
    """One d^2 bin holding more than 65 535 points: the origin's row is its 200 nearest cube points, not points of the far shells."""
    pts = overflow_cloud()
    (idx, cnt), = radius_lists(P, [pts], 200, 1.0)
    rows = np.r_[0, np.random.default_rng(1).choice(np.arange(1, len(pts)), 2000, replace=False)]
    s = compare(oracle, pts, idx, cnt, 200, 1.0, rows=rows, what="overflow")
    assert s["spill"] >= 2000, s
    row0 = idx[0][idx[0] >= 0]
    assert len(row0) == 200 and (np.abs(pts[row0]).max(1) <= 0.02).all()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 5, 8, 9, 63, 65])
def test_partial_pieces(P, oracle, n):
    pts = lattice(m=5, h=0.125, seed=n)[:n]
    for k in (1, 8, 60):
        (idx, cnt), = radius_lists(P, [pts], k, 0.3)
        compare(oracle, pts, idx, cnt, k, 0.3, what=f"n={n}")


# ---------------------------------------------------------------------------------------------------------------- (g)
@pytest.mark.gpu
def test_batched_equals_single(P, oracle, small_pair):
    clouds = [lattice(m=20, seed=7), P.PointCloud(small_pair["source"]).voxel_down_sample(0.1).points.astype(np.float32), lattice(m=5, seed=2)[:5]]
    k = 200
    both = radius_lists(P, clouds, k, 1.0)
    for c, (pts, (idx, cnt)) in enumerate(zip(clouds, both)):
        (i1, c1), = radius_lists(P, [pts], k, 1.0)
        assert np.array_equal(cnt, c1), c
        valid = (idx >= 0) & ((cnt[:, None] < 0) | (np.arange(k)[None, :] < cnt[:, None]))
        assert np.array_equal(np.where(valid, idx, -1), np.where(valid, i1, -1)), c
        compare(oracle, pts, idx, cnt, k, 1.0, what=f"batched cloud {c}")


# ---------------------------------------------------------------------------------------------------------------- FPFH on the same inputs
@pytest.mark.gpu
@pytest.mark.parametrize("case,k", [("lattice", 175), ("lattice", 200), ("overflow", 200)])
def test_fpfh_on_tie_and_overflow_clouds(P, oracle, case, k):
    """compute_fpfh_feature on the clouds above, with seeded random unit normals (pair features off the bin edges)."""
    pts = lattice() if case == "lattice" else overflow_cloud()
    v = np.random.default_rng(17).standard_normal(pts.shape); v /= np.linalg.norm(v, axis=1, keepdims=True)
    nrm = v.astype(np.float32)
    pc = P.PointCloud(pts); pc.normals = nrm
    dev = P.registration.compute_fpfh_feature(pc, P.KDTreeSearchParamHybrid(radius=1.0, max_nn=k)).data.T
    ref = oracle.compute_fpfh(pts, nrm, oracle.SEARCH_HYBRID, k, 1.0)
    assert_fpfh_explained(dev, ref, what=f"FPFH {case}")
    differ = ~(np.abs(dev - ref) <= 1e-3 * (1.0 + np.abs(ref))).all(1)
    assert differ.mean() <= 1e-3, differ.mean()
