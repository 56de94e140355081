"""Numpy float64 restatement of FPFH (Rusu et al. 2009, as Open3D's ComputeFPFHFeature evaluates it): the yardstick of the FPFH row tests.

Inputs are float32 points and normals taken as float64, and the neighbour lists as given (an index array per point, the point itself
excluded, -1 = no entry).  Nothing here is shared with the device code: every pair in float64, no float pass, no packed counters.

THE RULE.  For a point p1 with normal n1 and a neighbour p2 with normal n2: dp = p2 - p1, angle_i = n_i . dp / |dp|.  When
acos|angle1| > acos|angle2| the two points change roles (dp = -dp).  With (a, b) the normals in that order: f2 = a . dp / |dp|, v = dp x a
normalised, w = a x v, f1 = v . b, f0 = atan2(w . b, a . b).  dp == 0 and v == 0 give f0 = f1 = f2 = 0.  The normals are used as given:
with a normal longer than 1 an |angle| can exceed 1, acos is NaN, the comparison false and the roles stay.  The pair votes once in each of
three 11-bin histograms, at floor(11 (f0 + pi) / 2 pi), floor(11 (f1 + 1) / 2), floor(11 (f2 + 1) / 2), each clamped to 0..10; a vote weighs
inc = 100 / (number of neighbours).  That is the point's SPFH (33 numbers).  Its FPFH row: the SPFH rows of its neighbours weighted by
1 / d^2 (d^2 == 0: no weight) and summed, each of the three histograms of the sum scaled to 100, plus the point's own SPFH.  A point without
neighbours has an all-zero row.

WHAT FLOAT64 DOES NOT FIX.  acos and atan2 differ between libm implementations in the last bits, so a pair whose bin hangs on them is
`undecided` (MARGIN, far above any float64 evaluation error): a bin coordinate within MARGIN of an interior bin edge (1..10 for f1 and f2,
0..11 for the angle f0, whose ends wrap); differing normals whose two acos values are within MARGIN of each other, or an |angle| within
MARGIN of 1 (where acos turns NaN); 0 < |v| / (|dp| |a|) <= MARGIN.  Exactly degenerate pairs (dp == 0, v == 0, equal normals, two
|angle| that are the same number, an |angle| > 1, w . b == 0 -- atan2 of an exact zero) are decided.  A row is `touched` when one of its
own pairs, or a pair in the SPFH of one of its neighbours, is undecided.

LISTS.  knn_lists / hybrid_lists build on neighbor_reference (order (d^2, index), float64 d^2): KNN(k) = the k nearest including the point
itself, so at most k - 1 others; Hybrid(r, max_nn) the same inside d^2 < r^2.  The device kernels select by float32 d^2, so a row is
`list_open` -- the device's set need not be this one -- when another point's d^2 lies within the relative band BAND of the cut: the k-th
distance of an overfull list, or r^2.  A row is compared when neither it nor a row its list names is `list_open` (spread) or `touched`."""
import numpy as np

import neighbor_reference as nbr

MARGIN = 1e-9
BAND = 2.0 ** -20


def _dot(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def pair_bins(p1, n1, p2, n2):
    """The three bins (m, 3) int64, each 0..10, and the flag `undecided` (m,) of m pairs; all inputs (m, 3) float64."""
    m = len(p1)
    dp = p2 - p1
    length = np.sqrt(_dot(dp, dp))
    live = length != 0.0
    safe_len = np.where(live, length, 1.0)
    angle1, angle2 = _dot(n1, dp) / safe_len, _dot(n2, dp) / safe_len
    with np.errstate(invalid="ignore"):
        t1, t2 = np.arccos(np.abs(angle1)), np.arccos(np.abs(angle2))       # NaN for |angle| > 1
        swap = live & (t1 > t2)                                             # False where either is NaN
    a = np.where(swap[:, None], n2, n1); b = np.where(swap[:, None], n1, n2)
    dp = np.where(swap[:, None], -dp, dp)
    f2 = np.where(swap, -angle2, angle1)
    v = _cross(dp, a)
    vn = np.sqrt(_dot(v, v))
    live &= vn != 0.0
    v = v / np.where(live, vn, 1.0)[:, None]
    w = _cross(a, v)
    f = np.zeros((m, 3))
    f[:, 2] = np.where(live, f2, 0.0)
    f[:, 1] = np.where(live, _dot(v, b), 0.0)
    y = np.where(live, _dot(w, b), 0.0)
    f[:, 0] = np.where(live, np.arctan2(y, _dot(a, b)), 0.0)
    coord = np.stack([11.0 * (f[:, 0] + np.pi) / (2.0 * np.pi), 11.0 * (f[:, 1] + 1.0) * 0.5, 11.0 * (f[:, 2] + 1.0) * 0.5], axis=1)
    bins = np.clip(np.floor(coord), 0, 10).astype(np.int64)
    # --- what float64 does not fix
    edge = np.rint(coord)
    near = np.abs(coord - edge) <= MARGIN
    # (y == 0 exactly: atan2 is exactly 0 or +-pi by IEEE 754's rules of signs, no matter whose libm -- bin 5, or the bins 0 / 10 at the wrap)
    und = (near[:, 0] & (y != 0.0)) | (near[:, 1] & (edge[:, 1] >= 1) & (edge[:, 1] <= 10)) | (near[:, 2] & (edge[:, 2] >= 1) & (edge[:, 2] <= 10))
    differ = (n1 != n2).any(axis=1) & (length != 0.0)
    with np.errstate(invalid="ignore"):
        # (False where either is NaN: no swap, decided; |angle1| == |angle2| exactly, as of (0, 0, 1) and (0, 0, -1): acos of one number, decided)
        und |= differ & (np.abs(t1 - t2) <= MARGIN) & (np.abs(angle1) != np.abs(angle2))
    und |= differ & ((np.abs(np.abs(angle1) - 1.0) <= MARGIN) | (np.abs(np.abs(angle2) - 1.0) <= MARGIN))
    an = np.sqrt(_dot(a, a))
    with np.errstate(invalid="ignore", divide="ignore"):
        sine = vn / (length * an)
        und |= (vn != 0.0) & (length != 0.0) & (sine <= MARGIN)
    return bins, und


def fpfh(points, normals, idx):
    """points, normals (n, 3) float32; idx (n, K) integer neighbour lists, -1 = no entry, the point itself excluded ->
    dict(counts (n, 33) int64, inc (n,), spfh (n, 33), fpfh (n, 33) float64, m (n,) neighbours per point, undecided (n, K) bool, touched (n,) bool)."""
    p = np.asarray(points, np.float32).reshape(-1, 3).astype(np.float64)
    nr = np.asarray(normals, np.float32).reshape(-1, 3).astype(np.float64)
    idx = np.asarray(idx, np.int64).reshape(len(p), -1)
    n, K = idx.shape
    valid = idx >= 0
    assert not (idx == np.arange(n)[:, None]).any(), "a list names its own point"
    I, S = np.nonzero(valid)
    J = idx[I, S]
    bins, und = pair_bins(p[I], nr[I], p[J], nr[J])
    counts = np.zeros((n, 33), np.int64)
    for h in range(3):
        np.add.at(counts, (I, bins[:, h] + 11 * h), 1)
    m = valid.sum(1)
    inc = np.where(m > 0, 100.0 / np.maximum(m, 1), 0.0)
    spfh = counts * inc[:, None]
    undecided = np.zeros((n, K), bool)
    undecided[I, S] = und
    touched = spread(undecided.any(1), idx)
    # --- the weighted sum, slot by slot
    acc = np.zeros((n, 33))
    for s in range(K):
        j = idx[:, s]
        ok = j >= 0
        jj = np.where(ok, j, 0)
        d = p[jj] - p
        d2 = d[:, 0] * d[:, 0]; d2 += d[:, 1] * d[:, 1]; d2 += d[:, 2] * d[:, 2]
        ok &= d2 != 0.0
        acc += np.where(ok[:, None], spfh[jj] / np.where(ok, d2, 1.0)[:, None], 0.0)
    total = acc.reshape(n, 3, 11).sum(2)
    scale = np.where(total != 0.0, 100.0 / np.where(total != 0.0, total, 1.0), 0.0)
    out = (acc.reshape(n, 3, 11) * scale[:, :, None]).reshape(n, 33) + spfh
    out[m == 0] = 0.0
    return dict(counts=counts, inc=inc, spfh=spfh, fpfh=out, m=m, undecided=undecided, touched=touched)


def _others(idx, n):
    """Drops the point itself from every row of idx (n, k) (order kept, -1 at the end) -> (n, max(k - 1, 0)).  A row that does not hold its own
    point (k or more coincident copies with lower indices come first) loses its last entry: such a row is `list_open` (the cut is at d^2 = 0)."""
    k = idx.shape[1]
    if k == 0:
        return np.zeros((n, 0), np.int64)
    me = idx == np.arange(n)[:, None]
    drop = np.where(me.any(1), me.argmax(1), k - 1)
    keep = np.arange(k)[None, :] != drop[:, None]
    return idx[keep].reshape(n, k - 1)


def _open_at_kth(idx, d2, k):
    """Rows of a (d^2, index)-ordered list of k + 1 places that are overfull (place k taken) and hold another d^2 within BAND of the k-th."""
    over = idx[:, k] >= 0
    D = d2[:, k - 1]
    with np.errstate(invalid="ignore"):                                    # (inf - inf in the rows shorter than k: not overfull)
        near = np.abs(d2[:, k] - D) <= BAND * D
        if k >= 2:
            near |= np.abs(d2[:, k - 2] - D) <= BAND * D
    return over, over & near


def knn_lists(points, k):
    """KDTreeSearchParamKNN(k) -> (idx (n, k - 1) int64 others, list_open (n,) bool)."""
    points = np.asarray(points, np.float32).reshape(-1, 3)
    n = len(points)
    idx, d2 = nbr.knn(points, points, k + 1)
    _, is_open = _open_at_kth(idx, d2, k)
    return _others(idx[:, :k], n), is_open


def hybrid_lists(points, radius, max_nn):
    """KDTreeSearchParamHybrid(radius, max_nn) -> (idx (n, max_nn - 1) int64 others, list_open (n,) bool, overfull (n,) bool: more than max_nn
    points, the point itself among them, inside the ball)."""
    points = np.asarray(points, np.float32).reshape(-1, 3)
    n = len(points)
    r2 = float(radius) * float(radius)
    idx, d2, cnt = nbr.hybrid(points, points, radius, max_nn + 1)
    d2 = np.where(idx >= 0, d2, np.inf)
    over, is_open = _open_at_kth(idx, d2, max_nn)
    for i0 in range(0, n, 512):                                            # the rim of the ball
        is_open[i0:i0 + 512] |= (np.abs(nbr.pair_d2(points[i0:i0 + 512], points) - r2) <= BAND * r2).any(1)
    return _others(idx[:, :max_nn], n), is_open, over


def spread(flag, idx):
    """flag (n,) of a row or of any row its list names: a row's FPFH reads the SPFH -- so the list -- of every neighbour."""
    out = flag.copy()
    i, s = np.nonzero(idx >= 0)
    np.logical_or.at(out, i, flag[idx[i, s]])
    return out


def lists_for(points, spec):
    """spec = ("knn", k) or ("hybrid", radius, max_nn) -> (idx, list_open)."""
    if spec[0] == "knn":
        return knn_lists(points, spec[1])
    idx, is_open, _ = hybrid_lists(points, spec[1], spec[2])
    return idx, is_open
