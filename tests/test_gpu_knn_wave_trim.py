"""The one-query-per-lane k-NN search (csrc/pcr_knn_wave.h, option knn_wave = 1) on the inputs that steer its scan loops: exact ties with
the bound (pass 2 splits every step on "does any lane tie"), zero distances, lists that a radius cap leaves short, staged batches of
every length modulo 8 (the scans read two steps of four candidates per turn), and wavefronts whose pass-1 log overflows and that walk
the tree a second time.

The independent reference is the octet kernel (knn_wave = 0): counts equal, the sorted distances of every row array_equal, indices
different only inside runs of equal distances, no index twice in a row.  Where every coordinate is a multiple of 0.25 each float32
squared distance is exact whatever the order of the operations, and a numpy brute force is a second reference for the distances."""
import numpy as np
import pytest

from conftest import pkg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    return pkg()


@pytest.fixture
def knn_form(P):
    """Selects the exact k-NN kernel for the calls of one test (0 octet, 1 one query per lane); the default rule and budget come back afterwards."""
    yield lambda form: P._lib.set_option("knn_wave", form)
    P._lib.set_option("knn_wave", -1)
    P._lib.set_option("knnw_budget", 80)


def _debug_knn(P, pts, k, radius=0.0):
    import ctypes as C
    import torch
    n = len(pts)
    ctx = P._lib.Context.current()
    d = torch.from_numpy(np.ascontiguousarray(pts, dtype=np.float32)).cuda()
    idx = torch.empty((n, k), dtype=torch.int32, device="cuda"); d2 = torch.empty((n, k), dtype=torch.float32, device="cuda")
    cnt = torch.empty(n, dtype=torch.int32, device="cuda")
    ctx.check(ctx.lib.pcr_debug_knn(ctx.handle, C.c_void_p(d.data_ptr()), C.c_int64(n), C.c_int(k), C.c_double(radius),
                                    C.c_void_p(idx.data_ptr()), C.c_void_p(d2.data_ptr()), C.c_void_p(cnt.data_ptr())), "debug_knn")
    return idx.cpu().numpy(), d2.cpu().numpy(), cnt.cpu().numpy()


def _by_distance(idx, d2):
    order = np.lexsort((idx, d2), axis=1)                          # device rows are an unordered k-best set (inf, -1: empty slot)
    return np.take_along_axis(idx, order, 1), np.take_along_axis(d2, order, 1)


def _wave_against_octet(P, knn_form, pts, k, radius=0.0):
    """Runs both kernels and asserts the four properties on EVERY row; returns the wavefront kernel's (indices, distances, counts),
    rows sorted by distance."""
    knn_form(1)
    wi, wd, wc = _debug_knn(P, pts, k, radius)
    knn_form(0)
    oi, od, oc = _debug_knn(P, pts, k, radius)
    assert np.array_equal(wc, oc)
    wi, wd = _by_distance(wi, wd)
    oi, od = _by_distance(oi, od)
    assert np.array_equal(wd, od)                                  # same float32 distances, slot for slot (inf = empty)
    assert ((wi >= 0).sum(1) == wc).all() and np.isfinite(wd).sum(1).tolist() == wc.tolist()
    # Indices may differ only inside a run of equal distances.  Inside the row that is a run of equal slots; the run of the row's LAST
    # distance goes on outside the row (the k-th and the (k+1)-th nearest tie, each kernel keeps its pick), so there the two points are
    # measured again: both lie at the slot's distance from the query.
    inrow = np.zeros(wd.shape, bool)
    if k > 1:
        same = wd[:, 1:] == wd[:, :-1]
        inrow[:, 1:] |= same; inrow[:, :-1] |= same
    last = wd[np.arange(len(wd)), np.maximum(wc, 1) - 1]
    differ = wi != oi
    assert (inrow | (wd == last[:, None]))[differ].all()
    r, c = np.nonzero(differ & ~inrow)
    if len(r):
        p64 = pts.astype(np.float64)
        dw = ((p64[wi[r, c]] - p64[r]) ** 2).sum(1); do = ((p64[oi[r, c]] - p64[r]) ** 2).sum(1)
        assert np.allclose(dw, do, rtol=1e-6, atol=0.0) and np.allclose(dw, wd[r, c], rtol=1e-6, atol=0.0)
    cols = np.arange(k, dtype=np.int64)
    s = np.sort(np.where(wi >= 0, wi.astype(np.int64), -1 - cols), axis=1)       # (empty slots: distinct negative numbers)
    assert (np.diff(s, axis=1) != 0).all()                         # no index twice
    assert (wi < len(pts)).all()
    return wi, wd, wc


def _brute_distances(pts, k, r2cap=None):
    """Sorted k smallest squared distances of every row (inf: empty) and their number, in float32: exact where the coordinates are
    multiples of 0.25.  A cap excludes the points AT it."""
    p = pts.astype(np.float32)
    d = p[:, None, :] - p[None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    if r2cap is not None:
        d2 = np.where(d2 < np.float32(r2cap), d2, np.float32(np.inf))
    d2 = np.sort(d2, axis=1)
    if d2.shape[1] < k:
        d2 = np.concatenate([d2, np.full((len(p), k - d2.shape[1]), np.inf, np.float32)], axis=1)
    d2 = d2[:, :k]
    return d2, np.isfinite(d2).sum(1)


def _lattice():
    g = np.stack(np.meshgrid(np.arange(12), np.arange(12), np.arange(3), indexing="ij"), -1).reshape(-1, 3)
    return (g * 0.25).astype(np.float32)                           # 432 points, every coordinate a multiple of 0.25


@pytest.mark.parametrize("k", [30, 20, 7])
def test_ties_at_the_bound(P, knn_form, k):
    """On a lattice almost every row ties at its k-th distance (and lanes of one wavefront tie at different candidates), so the step with
    a tie and the step without one alternate inside a wavefront."""
    pts = _lattice()
    wi, wd, wc = _wave_against_octet(P, knn_form, pts, k)
    ref, rc = _brute_distances(pts, k)
    assert (wc == k).all() and np.array_equal(rc, wc)
    assert np.array_equal(wd, ref)
    kth = np.sort(((pts[:, None] - pts[None]) ** 2).sum(-1), axis=1)
    assert (kth[:, k - 1] == kth[:, k]).mean() > 0.5               # the k-th and the (k+1)-th distance tie in most rows: the case is what it says


def test_zero_distances_triplicated_points(P, knn_form):
    pts = np.repeat(_lattice()[np.linspace(0, 431, 100).astype(int)], 3, axis=0)
    assert len(np.unique(pts, axis=0)) == 100 and len(pts) == 300
    wi, wd, wc = _wave_against_octet(P, knn_form, pts, 30)
    ref, rc = _brute_distances(pts, 30)
    assert (wc == 30).all() and np.array_equal(wd, ref)
    assert (wd[:, :3] == 0).all()


def test_zero_distances_one_point_forty_times(P, knn_form):
    """Every distance is 0: the bound is 0 and all 30 list entries tie with it."""
    pts = np.tile(np.array([[0.75, -1.5, 2.25]], np.float32), (40, 1))
    wi, wd, wc = _wave_against_octet(P, knn_form, pts, 30)
    assert (wc == 30).all() and (wd == 0).all()


def test_list_not_full_under_a_radius_cap(P, knn_form):
    """Radius exactly 0.5 on the 0.25 lattice: at most 27 points lie strictly inside the cap, so no list is full, the bound is the cap
    itself, no tie counts, and the points AT the cap (two lattice steps along an axis) stay out."""
    pts = _lattice()
    wi, wd, wc = _wave_against_octet(P, knn_form, pts, 30, radius=0.5)
    ref, rc = _brute_distances(pts, 30, r2cap=0.25)
    assert np.array_equal(wc, rc) and np.array_equal(wd, ref)
    assert wc.max() < 30 and wd[np.isfinite(wd)].max() < 0.25
    at_cap = (((pts[:, None] - pts[None]) ** 2).sum(-1) == 0.25).sum(1)
    assert (at_cap > 0).all()


@pytest.fixture(scope="module")
def scan_points(P, small_pair):
    return P.PointCloud(small_pair["source"]).voxel_down_sample(0.2).points.astype(np.float32)


@pytest.mark.parametrize("n", [1, 29, 30, 31, 63, 64, 65, 129, 200])
def test_batch_tails(P, knn_form, scan_points, n):
    """Small clouds: the staged batches (after the cull) and the replayed log end at every residue modulo 8."""
    pts = scan_points[:n].copy()
    wi, wd, wc = _wave_against_octet(P, knn_form, pts, 30)
    assert (wc == min(30, n)).all()


def _log_spaced_disc():
    """8192 points of a thin disc whose radii are log-uniform over 1 .. e^6: every scale of spacing at once."""
    rng = np.random.default_rng(20)
    rad = np.exp(rng.uniform(0.0, 6.0, 8192)); ang = rng.uniform(0.0, 2.0 * np.pi, 8192)
    return np.stack([rad * np.cos(ang), rad * np.sin(ang), rng.normal(0.0, 0.02, 8192)], 1).astype(np.float32)


@pytest.fixture(scope="module")
def overflow_points():
    return _log_spaced_disc()


@pytest.mark.parametrize("k", [30, 20])
def test_log_overflow_and_second_walk(P, knn_form, overflow_points, k):
    """Where the spacing of the points grows with the distance from the centre, 64 Morton-consecutive queries span several scales: the
    lanes far out keep wide bounds while the dense part goes by, and the candidates that beat some bound in pass 1 outnumber the 768
    slots of the log in 31 of the 128 wavefronts at k = 30 and in 27 at k = 20 (counted with an instrumented build,
    profiles/knn_wave_trim.md; 4096 points uniform in a cube reach 458 events at the most, a thin shell with points inside it 672).  The debug call hands nothing over, so those
    wavefronts walk the tree a second time."""
    wi, wd, wc = _wave_against_octet(P, knn_form, overflow_points, k)
    assert (wc == k).all()
