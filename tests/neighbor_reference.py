"""Brute-force numpy reference of the search index's result rule (include/pcr_hip.h, "THE RESULT RULE"): the yardstick of the
neighbour-search tests.

For a query q and a dataset point p, both float32: d = q.astype(f64) - p.astype(f64); d2 = d[0]*d[0]; d2 += d[1]*d[1]; d2 += d[2]*d[2]
(every operation rounded once: numpy does not fuse).  The dataset is ordered for a query by (d2, index) ascending: np.lexsort on
(index, d2).  knn = the first k of that order; radius = every point with d2 < float64(radius) * float64(radius), strict; hybrid = the
first max_nn of the radius set.  A query with a non-finite coordinate finds nothing."""
import numpy as np


def pair_d2(queries, dataset):
    """(m, n) float64 squared distances of float32 rows, in the operation order of the rule."""
    q = np.asarray(queries, np.float32).reshape(-1, 3).astype(np.float64)
    p = np.asarray(dataset, np.float32).reshape(-1, 3).astype(np.float64)
    d = q[:, None, 0] - p[None, :, 0]
    d2 = d * d
    d = q[:, None, 1] - p[None, :, 1]
    d2 += d * d
    d = q[:, None, 2] - p[None, :, 2]
    d2 += d * d
    return d2


def _first(d2, k):
    """The first min(k, n) places of the order (d2, index) of every row of d2 (c, n) -> (indices (c, k'), their d2 (c, k')).  np.lexsort on
    (index, d2) -- over the k' + 65 smallest values of a row when that provably holds the answer (the k'-th value is strictly below the
    largest value kept, so every point tied with one of the first k' is among those kept), over the whole row otherwise."""
    c, n = d2.shape
    kk = min(int(k), n)
    if kk == 0:
        return np.zeros((c, 0), np.int64), np.zeros((c, 0))
    ids = np.broadcast_to(np.arange(n, dtype=np.int64), d2.shape)

    def full(rows):
        order = np.lexsort((ids[rows], d2[rows]), axis=1)[:, :kk]
        return order, np.take_along_axis(d2[rows], order, axis=1)
    w = kk + 64
    if n <= w + 1:
        return full(slice(None))
    part = np.argpartition(d2, w, axis=1)[:, :w + 1].astype(np.int64)
    pd2 = np.take_along_axis(d2, part, axis=1)
    local = np.lexsort((part, pd2), axis=1)
    cand = np.take_along_axis(part, local, axis=1); cd2 = np.take_along_axis(pd2, local, axis=1)
    idx, out = cand[:, :kk].copy(), cd2[:, :kk].copy()
    redo = np.nonzero(~(cd2[:, kk - 1] < cd2[:, w]))[0]
    if len(redo):
        idx[redo], out[redo] = full(redo)
    return idx, out


def _chunks(queries, dataset, chunk):
    """Yields (row offset, d2 (c, n), finite (c,) bool) per chunk of queries; the rows of non-finite queries are computed for (0, 0, 0)."""
    queries = np.asarray(queries, np.float32).reshape(-1, 3)
    dataset = np.asarray(dataset, np.float32).reshape(-1, 3)
    for i0 in range(0, len(queries), chunk):
        q = queries[i0:i0 + chunk]
        finite = np.isfinite(q).all(1)
        yield i0, pair_d2(np.where(finite[:, None], q, np.float32(0.0)), dataset), finite


def knn(dataset, queries, k, chunk=512):
    """-> (idx (m, k) int64, d2 (m, k) float64): places beyond the dataset's size, and the rows of non-finite queries, hold -1 / +inf."""
    m = len(np.asarray(queries).reshape(-1, 3))
    idx = np.full((m, k), -1, np.int64); d2 = np.full((m, k), np.inf)
    for i0, pd2, finite in _chunks(queries, dataset, chunk):
        order, sd2 = _first(pd2, k)
        c = order.shape[1]
        rows = slice(i0, i0 + len(order))
        idx[rows, :c] = np.where(finite[:, None], order[:, :c], -1)
        d2[rows, :c] = np.where(finite[:, None], sd2[:, :c], np.inf)
    return idx, d2


def radius(dataset, queries, r, chunk=512):
    """-> (idx (T,) int64, d2 (T,) float64, row_splits (m + 1,) int64), every row in the order of the rule."""
    r2 = float(r) * float(r)
    m = len(np.asarray(queries).reshape(-1, 3))
    rows_i, rows_d, counts = [], [], np.zeros(m, np.int64)
    for i0, pd2, finite in _chunks(queries, dataset, chunk):
        order, sd2 = _first(pd2, int(((pd2 < r2) & finite[:, None]).sum(1).max(initial=0)))
        inside = (sd2 < r2) & finite[:, None]
        counts[i0:i0 + len(order)] = inside.sum(1)
        rows_i.append(order[inside]); rows_d.append(sd2[inside])          # row-major: rows stay in order
    splits = np.zeros(m + 1, np.int64); splits[1:] = np.cumsum(counts)
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)
    return cat(rows_i, np.int64), cat(rows_d, np.float64), splits


def hybrid(dataset, queries, r, max_nn, chunk=512):
    """-> (idx (m, max_nn) int64, d2 (m, max_nn) float64, counts (m,) int32): places beyond the count hold -1 / 0."""
    r2 = float(r) * float(r)
    m = len(np.asarray(queries).reshape(-1, 3))
    idx = np.full((m, max_nn), -1, np.int64); d2 = np.zeros((m, max_nn)); counts = np.zeros(m, np.int32)
    for i0, pd2, finite in _chunks(queries, dataset, chunk):
        order, sd2 = _first(pd2, max_nn)
        c = order.shape[1]
        inside = (sd2[:, :c] < r2) & finite[:, None]
        rows = slice(i0, i0 + len(order))
        idx[rows, :c] = np.where(inside, order[:, :c], -1)
        d2[rows, :c] = np.where(inside, sd2[:, :c], 0.0)
        counts[rows] = inside.sum(1)
    return idx, d2, counts
