"""The nearest-neighbour search index on the device against the brute-force numpy reference of its result rule (``neighbor_reference``):
every comparison is EQUALITY -- indices exactly, d^2 bit for bit, counts and row splits exactly, padding as specified -- with no exempted
rows.

Main input: the source of golden pair 899 after ``voxel_down_sample(0.2)`` on the device (about 9.5k points) as the dataset, the reference
computed on the float32 points the device returned; queries: every third row of the pair's target at 0.2 m (about 3.2k rows; about 600 of
them have their nearest point beyond 1 m, up to 14 m away, so the unbounded walk is exercised, and at r = 0.3 / 0.5 / 1.0 most, half and a
fifth of the rows are empty).  Ties: the 12 x 12 x 12 integer lattice in shuffled caller order, queried at its points and at its cell
centres (8-way exact ties): everything is exact in float32 and float64, so the caller-index tie-break decides every row.  Duplicates: 300
points, each present three times.  Small and degenerate shapes, non-finite queries, queries far outside the box; the index's lifetime; the two
query-order forms of the kernels."""
import ctypes as C

import numpy as np
import pytest

import neighbor_reference as ref
from conftest import pkg

pytestmark = pytest.mark.gpu

KNN_KS = [1, 8, 9, 30, 32, 33, 64, 65, 200]          # the issue's {1, 30, 33, 65, 200} and both sides of every slot variant (8, 32, 64)
RADIUS_CASES = [(0.3, True), (0.3, False), (1.0, True), (1.0, False)]
HYBRID_CASES = [(0.3, 5), (0.5, 30), (1.0, 200)]


@pytest.fixture(scope="module")
def P():
    return pkg()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _np(t):
    return t.detach().cpu().numpy()


def assert_knn(got, want, what=""):
    (gi, gd), (wi, wd) = got, want
    gi, gd = _np(gi), _np(gd)
    assert gi.dtype == np.int64 and gd.dtype == np.float64
    assert gi.shape == wi.shape and gd.shape == wd.shape, (what, gi.shape, wi.shape)
    bad = np.nonzero((gi != wi).any(1) | (_bits(gd) != _bits(wd)).any(1))[0]
    assert len(bad) == 0, (what, len(bad), bad[:5], gi[bad[:2]], wi[bad[:2]], gd[bad[:2]], wd[bad[:2]])


def assert_radius(got, want, sort, what=""):
    (gi, gd, gs), (wi, wd, ws) = got, want
    gi, gd, gs = _np(gi), _np(gd), _np(gs)
    assert gi.dtype == np.int64 and gd.dtype == np.float64 and gs.dtype == np.int64
    assert (gs == ws).all(), (what, np.nonzero(gs != ws)[0][:5])
    assert gi.shape == wi.shape and gd.shape == wd.shape
    if not sort:                                          # the order inside a row is free: each row compared as a set, sorted on the host
        row = np.repeat(np.arange(len(gs) - 1), np.diff(gs))
        order = np.lexsort((gi, gd, row))
        gi, gd = gi[order], gd[order]
    bad = np.nonzero((gi != wi) | (_bits(gd) != _bits(wd)))[0]
    assert len(bad) == 0, (what, len(bad), bad[:5], gi[bad[:5]], wi[bad[:5]])


def assert_hybrid(got, want, what=""):
    (gi, gd, gc), (wi, wd, wc) = got, want
    gi, gd, gc = _np(gi), _np(gd), _np(gc)
    assert gi.dtype == np.int64 and gd.dtype == np.float64 and gc.dtype == np.int32
    assert (gc == wc).all(), (what, np.nonzero(gc != wc)[0][:5])
    assert gi.shape == wi.shape
    bad = np.nonzero((gi != wi).any(1) | (_bits(gd) != _bits(wd)).any(1))[0]
    assert len(bad) == 0, (what, len(bad), bad[:5], gi[bad[:2]], wi[bad[:2]])


# ------------------------------------------------------------------------------------------------------------ main input
@pytest.fixture(scope="module")
def main(P, small_pair):
    """(index, dataset float32 points, query float32 rows, {name: reference})."""
    cloud = P.PointCloud(small_pair["source"]).voxel_down_sample(0.2)
    pts = cloud.points.astype(np.float32)
    q = np.ascontiguousarray(P.PointCloud(small_pair["target"]).voxel_down_sample(0.2).points.astype(np.float32)[::3])
    assert 9000 < len(pts) < 10000 and 3000 < len(q) < 3500
    refs = {"knn": ref.knn(pts, q, 200)}
    for r in (0.3, 1.0):
        refs["radius", r] = ref.radius(pts, q, r)
    for r, k in HYBRID_CASES:
        refs["hybrid", r, k] = ref.hybrid(pts, q, r, k)
    nns = P.NearestNeighborSearch(cloud)
    yield nns, pts, q, refs
    nns.close()


def test_the_main_input_exercises_what_it_claims(main):
    _, pts, q, refs = main
    d1 = np.sqrt(refs["knn"][1][:, 0])
    assert (d1 > 1.0).sum() > 300 and d1.max() > 10.0          # the unbounded walk
    sizes = np.diff(refs["radius", 1.0][2])
    assert sizes.max() > 200 and (sizes == 0).sum() > 300       # balls larger than every k-best, and empty rows
    for (r, k) in HYBRID_CASES:                                 # both the cut and the padding
        sz = np.diff(ref.radius(pts, q, r)[2]) if r == 0.5 else np.diff(refs["radius", r][2])
        assert (sz > k).any() and (sz < k).any(), (r, k)


@pytest.mark.parametrize("k", KNN_KS)
def test_knn_rows_equal_the_reference(main, k):
    nns, _, q, refs = main
    wi, wd = refs["knn"]
    assert_knn(nns.knn_search(q, k), (wi[:, :k], wd[:, :k]), f"k={k}")


@pytest.mark.parametrize("r,sort", RADIUS_CASES)
def test_radius_rows_equal_the_reference(main, r, sort):
    nns, _, q, refs = main
    assert_radius(nns.fixed_radius_search(q, r, sort=sort), refs["radius", r], sort, f"r={r} sort={sort}")


@pytest.mark.parametrize("r,k", HYBRID_CASES)
def test_hybrid_rows_equal_the_reference(main, r, k):
    nns, _, q, refs = main
    assert_hybrid(nns.hybrid_search(q, r, k), refs["hybrid", r, k], f"r={r} max_knn={k}")


def test_both_query_orders_give_the_same_bits(P, main):
    """The kernels take the queries in the caller's order or in the Morton order of their keys on the index's lattice (by default only
    large batches of searches with k above 8): forced either way, the rows are the same."""
    nns, _, q, refs = main
    try:
        for form in (0, 1):
            P._lib.set_option("search_sort_queries", form)
            wi, wd = refs["knn"]
            assert_knn(nns.knn_search(q, 30), (wi[:, :30], wd[:, :30]), f"form {form}")
            assert_knn(nns.knn_search(q, 1), (wi[:, :1], wd[:, :1]), f"form {form}")
            assert_radius(nns.fixed_radius_search(q, 1.0), refs["radius", 1.0], True, f"form {form}")
            assert_hybrid(nns.hybrid_search(q, 0.5, 30), refs["hybrid", 0.5, 30], f"form {form}")
    finally:
        P._lib.set_option("search_sort_queries", -1)


# ------------------------------------------------------------------------------------------------------------------ ties
@pytest.fixture(scope="module")
def lattice(P):
    g = np.stack(np.meshgrid(*[np.arange(12)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    data = np.ascontiguousarray(g[np.random.default_rng(5).permutation(len(g))])
    q = np.ascontiguousarray(np.concatenate([g, g + np.float32(0.5)]))
    nns = P.NearestNeighborSearch(data)
    yield nns, data, q, len(g)
    nns.close()


@pytest.mark.parametrize("k", [1, 8, 9, 27])
def test_lattice_knn_ties_go_to_the_lower_caller_index(lattice, k):
    nns, data, q, _ = lattice
    want = ref.knn(data, q, k)
    assert_knn(nns.knn_search(q, k), want, f"lattice k={k}")


def test_lattice_radius_and_hybrid(lattice):
    nns, data, q, ng = lattice
    got = nns.fixed_radius_search(q, 1.0)
    assert_radius(got, ref.radius(data, q, 1.0), True, "lattice r=1.0")
    sizes = np.diff(_np(got[2]))
    assert (sizes[:ng] == 1).all()                   # the six neighbours at d^2 = 1 exactly are out, the point itself is in
    assert (_np(got[1])[:ng] == 0.0).all()
    for sort in (True, False):
        assert_radius(nns.fixed_radius_search(q, 1.5, sort=sort), ref.radius(data, q, 1.5), sort, f"lattice r=1.5 sort={sort}")
    assert_hybrid(nns.hybrid_search(q, 1.5, 10), ref.hybrid(data, q, 1.5, 10), "lattice hybrid")


def test_duplicates_come_out_by_caller_index(P):
    rng = np.random.default_rng(11)
    base = rng.uniform(-5, 5, (300, 3)).astype(np.float32)
    data = np.ascontiguousarray(np.repeat(base, 3, axis=0)[rng.permutation(900)])
    nns = P.NearestNeighborSearch(data)
    for k in (2, 3, 4):
        got = nns.knn_search(base, k)
        assert_knn(got, ref.knn(data, base, k), f"duplicates k={k}")
        gi, gd = _np(got[0]), _np(got[1])
        c = min(k, 3)
        assert (gd[:, :c] == 0.0).all() and (np.diff(gi[:, :c], axis=1) > 0).all()
    assert_radius(nns.fixed_radius_search(base, 1e-3), ref.radius(data, base, 1e-3), True, "duplicates radius")
    nns.close()


# ----------------------------------------------------------------------------------------------- small and degenerate
def _small_queries(rng, data, m):
    """m query rows around the data; with m = 9: one 1e3 m outside the box, one with a NaN, one with an inf, next to valid rows."""
    q = rng.uniform(-2, 2, (m, 3)).astype(np.float32)
    if m and len(data):
        q[0] = data[0]                                 # a dataset point itself
    if m == 9:
        q[2] = [1e3, -1e3, 1e3]
        q[4, 1] = np.nan
        q[6, 0] = np.inf
        q[7] = [-1e3, 0.5, 0.25]
    return np.ascontiguousarray(q)


@pytest.mark.parametrize("n", [0, 1, 2, 7, 8, 9, 63, 64, 65])
def test_small_and_degenerate_shapes(P, n):
    rng = np.random.default_rng(100 + n)
    data = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    nns = P.NearestNeighborSearch(data)
    assert len(nns) == n
    for m in (0, 1, 9):
        q = _small_queries(rng, data, m)
        for k in (1, 3, 200):
            gi, gd = nns.knn_search(q, k)
            assert tuple(gi.shape) == (m, min(k, n))
            wi, wd = ref.knn(data, q, k)
            assert_knn((gi, gd), (wi[:, :min(k, n)], wd[:, :min(k, n)]), f"n={n} m={m} k={k}")
        for r in (0.5, 5000.0):                        # 5000: covers the whole cloud from every finite query
            for sort in (True, False):
                assert_radius(nns.fixed_radius_search(q, r, sort=sort), ref.radius(data, q, r), sort, f"n={n} m={m} r={r}")
            assert_hybrid(nns.hybrid_search(q, r, 3), ref.hybrid(data, q, r, 3), f"n={n} m={m} r={r}")
        assert_hybrid(nns.hybrid_search(q, 5000.0, 200), ref.hybrid(data, q, 5000.0, 200), f"n={n} m={m} hybrid 200")
    nns.close()


def test_abi_pads_rows_beyond_the_dataset(P):
    """k > n through the C ABI: the places beyond the dataset's size hold idx = -1 and d2 = +inf (knn) / 0 (hybrid)."""
    import torch
    rng = np.random.default_rng(3)
    for n in (0, 5):
        data = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
        q = _small_queries(rng, data, 9)
        nns = P.NearestNeighborSearch(data)
        ctx = P._lib.Context.current()
        qd = torch.from_numpy(q).cuda()
        idx = torch.full((9, 8), 77, dtype=torch.int32, device="cuda"); d2 = torch.full((9, 8), 77.0, dtype=torch.float64, device="cuda")
        ctx.check(ctx.lib.pcr_index_knn(ctx.handle, nns._handle, C.c_void_p(qd.data_ptr()), C.c_int64(9), C.c_int(8), C.c_void_p(idx.data_ptr()),
                                        C.c_void_p(d2.data_ptr())), "knn")
        wi, wd = ref.knn(data, q, 8)
        assert (_np(idx) == wi).all() and (_bits(_np(d2)) == _bits(wd)).all()
        assert (_np(idx)[:, n:] == -1).all() and np.isposinf(_np(d2)[:, n:]).all()
        cnt = torch.full((9,), 77, dtype=torch.int32, device="cuda")
        ctx.check(ctx.lib.pcr_index_hybrid(ctx.handle, nns._handle, C.c_void_p(qd.data_ptr()), C.c_int64(9), C.c_double(5000.0), C.c_int(8),
                                           C.c_void_p(idx.data_ptr()), C.c_void_p(d2.data_ptr()), C.c_void_p(cnt.data_ptr())), "hybrid")
        wi, wd, wc = ref.hybrid(data, q, 5000.0, 8)
        assert (_np(idx) == wi).all() and (_bits(_np(d2)) == _bits(wd)).all() and (_np(cnt) == wc).all()
        # arguments outside the limits are PCR_EINVAL with a message
        for bad_k in (0, 201):
            assert ctx.lib.pcr_index_knn(ctx.handle, nns._handle, C.c_void_p(qd.data_ptr()), C.c_int64(9), C.c_int(bad_k), C.c_void_p(idx.data_ptr()),
                                         C.c_void_p(d2.data_ptr())) == P._lib.PCR_EINVAL
            assert b"1..200" in ctx.lib.pcr_last_error(ctx.handle)
        assert ctx.lib.pcr_index_radius_count(ctx.handle, nns._handle, C.c_void_p(qd.data_ptr()), C.c_int64(9), C.c_double(0.0),
                                              C.c_void_p(cnt.data_ptr())) == P._lib.PCR_EINVAL
        nns.close()


# ------------------------------------------------------------------------------------------------------------ lifetime
def _three_searches(nns, q):
    a = nns.knn_search(q, 30); b = nns.fixed_radius_search(q, 1.0); c = nns.hybrid_search(q, 0.5, 30)
    return [_np(t) for t in (*a, *b, *c)]


def _same(xs, ys):
    return all(x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(xs, ys))


def test_index_keeps_its_own_copy_and_repeats_bit_for_bit(P, main):
    import torch
    _, pts, q, refs = main
    q = q[:800]
    xyz = torch.from_numpy(pts).cuda()
    nns = P.NearestNeighborSearch(xyz)
    xyz.fill_(123.0)                                    # the dataset tensor is overwritten after the build
    torch.cuda.synchronize()
    first = _three_searches(nns, q)
    wi, wd = refs["knn"]
    assert (first[0] == wi[:800, :30]).all() and (_bits(first[1]) == _bits(wd[:800, :30])).all()
    assert _same(first, _three_searches(nns, q))        # the same calls twice
    fresh = P.NearestNeighborSearch(pts)                # ... and on a fresh index
    assert _same(first, _three_searches(fresh, q))
    fresh.close()
    nns.close()


def test_index_is_searched_from_a_second_context(P, main):
    import torch
    nns, _, q, refs = main
    here = P._lib.Context.current()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        assert P._lib.Context.current() is not here
        got = nns.knn_search(q, 30)
        rad = nns.fixed_radius_search(q, 1.0)
    side.synchronize()
    wi, wd = refs["knn"]
    assert_knn(got, (wi[:, :30], wd[:, :30]), "second context")
    assert_radius(rad, refs["radius", 1.0], True, "second context")


def test_search_after_close_raises(P):
    nns = P.NearestNeighborSearch(np.zeros((4, 3), np.float32))
    nns.knn_search(np.zeros((1, 3), np.float32), 1)
    nns.close()
    nns.close()                                          # closing twice is harmless
    for call in (lambda: nns.knn_search(np.zeros((1, 3), np.float32), 1), lambda: nns.fixed_radius_search(np.zeros((1, 3), np.float32), 1.0),
                 lambda: nns.hybrid_search(np.zeros((1, 3), np.float32), 1.0, 2)):
        with pytest.raises(RuntimeError, match="closed"):
            call()


def test_kdtreeflann_rows_equal_the_batch_rows(P, main):
    nns, pts, q, refs = main
    tree = P.KDTreeFlann(P.PointCloud(pts))
    wi, wd = refs["knn"]
    ri, rd, rs = refs["radius", 1.0]
    hi, hd, hc = refs["hybrid", 0.5, 30]
    rows = [0, 1, 17, int(np.argmax(np.diff(rs))), int(np.argmin(np.diff(rs))), len(q) - 1]
    for i in rows:
        for (c, idx, d2) in (tree.search_knn_vector_3d(q[i].astype(np.float64), 30), tree.search_vector_3d(q[i], P.KDTreeSearchParamKNN(30))):
            assert c == 30 and idx.dtype == np.int32 and d2.dtype == np.float64
            assert (idx == wi[i, :30]).all() and (_bits(d2) == _bits(wd[i, :30])).all()
        for (c, idx, d2) in (tree.search_radius_vector_3d(q[i], 1.0), tree.search_vector_3d(q[i], P.KDTreeSearchParamRadius(1.0))):
            assert c == rs[i + 1] - rs[i] and idx.dtype == np.int32
            assert (idx == ri[rs[i]:rs[i + 1]]).all() and (_bits(d2) == _bits(rd[rs[i]:rs[i + 1]])).all()
        for (c, idx, d2) in (tree.search_hybrid_vector_3d(q[i], 0.5, 30), tree.search_vector_3d(q[i], P.KDTreeSearchParamHybrid(0.5, 30))):
            assert c == hc[i] and len(idx) == c and idx.dtype == np.int32
            assert (idx == hi[i, :c]).all() and (_bits(d2) == _bits(hd[i, :c])).all()
    # the indices feed select_by_index directly
    got = nns.knn_search(q[:5], 3)[0]
    sel = P.PointCloud(pts).select_by_index(got.reshape(-1))
    assert (sel.points.astype(np.float32) == pts[wi[:5, :3].reshape(-1)]).all()
    tree.close()
