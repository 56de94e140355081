"""A reference for estimated normals and covariances that shares nothing with the solver under test (plain numpy, float32 inputs taken as exact).

The device (d_fast_eigen3x3) and the CPU oracle (orc_fast_eigen3x3) run the same non-iterative eigen solver branch for branch, and both build the
covariance with the uncentred formula E[x x^T] - mu mu^T in float64.  Comparing their normals can never show an error the two share, and a share of
rows within a dot product of 1 - 1e-5 hides a path that is wrong on every row it serves.  Here every row is checked, and no reference EIGENVECTOR
is needed: a unit vector n is the normal of a neighbourhood iff it is an eigenvector of the neighbourhood's covariance C (residual) that belongs to
the smallest eigenvalue (Rayleigh quotient), and both can be bounded from C alone.

NEIGHBOUR SETS (neighbours).  Brute force in float64, in chunks, rows ordered by (d^2, index); KNN, Hybrid(radius, k) and Radius, with d^2 < r^2
strict as in the oracle.  Every row also gets its first non-member.  A row is AMBIGUOUS when a float32 search may legitimately decide otherwise:
its k-th and (k+1)-th d^2 differ by less than 4e-6 relative (the float32 d^2 resolution test_knn_index_is_exact uses), or a candidate lies within
4e-6 relative of r^2.  An ambiguous row carries a second acceptable set (farthest member swapped for the first non-member; the rim point taken in
or left out).  assert_ambiguity_cap holds the ambiguous rows to 0.1 % of a cloud -- from the reference alone, before a device is consulted.

COVARIANCE (covariance).  Centred, two-pass, in np.longdouble, divided by the count as Open3D does.

THE BOUND E.  Oracle and device evaluate C_ij = S_ij / k - (S_i / k)(S_j / k) with S the float64 sums over the k members.  With u = 2^-53: a sum
of k products carries at most (k - 1) + 1 roundings per term, the division one more, so |fl(S_ij / k) - S_ij / k| <= (k + 1) u E|x_i x_j|; the two
means carry k u |mu_i| each, their product one rounding more: |fl(mu_i mu_j) - mu_i mu_j| <= (2 k + 2) u |mu_i mu_j|; the subtraction rounds once
more at the size of the larger operand.  With E|x_i x_j| <= (E x_i^2 + E x_j^2) / 2 <= |mu|^2 + tr C and |mu_i mu_j| <= |mu|^2 the three add up to
less than (3 k + 5) u (|mu|^2 + tr C) <= E := 4 (k + 3) 2^-53 (|mu|^2 + tr C).  That is what the uncentred formula may lose per entry, whatever the
summation order; on the scan (|mu| ~ 50 m, tr C ~ 0.1 m^2) E ~ 3e-11 m^2.

CHECKS (assert_normals_explained), for every row, none of them a share:
  * unit length: | |n| - 1 | <= 2^-23 (three float32 roundings of a unit vector move its length by at most sqrt(3) 2^-25);
  * eigenvector residual: |C n - (n^T C n) n| <= (2^-23 + E / lmax) lmax -- 2^-23 is twice the float32 rounding of the output (rounding a unit
    eigenvector moves C n - rho n by at most lmax sqrt(3) 2^-25), the factor leaves room for the solver; E / lmax is the covariance's own error;
  * Rayleigh excess: n^T C n - l0 <= the same bound, with l0 = eigvalsh(C)[0]: n belongs to the smallest eigenvalue, not to another one;
  * orientation: with a prior, n . prior >= 0;
  * special rows follow the oracle's literal rule and are compared for EQUALITY (special_rule): fewer than 3 neighbours -> identity covariance
    -> (0, 0, 1); all neighbours coincident -> zero covariance -> the prior itself (not normalised) or (0, 0, 1); a covariance whose three
    off-diagonal entries are exactly zero -> "axis of the strictly smallest diagonal entry, else z"; then flipped iff n . prior < 0 (a row with
    n . prior == 0 is not flipped).  QUIRK, reproduced on purpose: for a line along z the covariance is diag(0, 0, L), no diagonal entry is
    strictly smallest, and the rule returns z -- the line's own direction, the eigenvector of the LARGEST eigenvalue.  A line along x or y, or
    along a diagonal, gets a proper normal.  Open3D's solver does the same.
assert_covariances_explained: every entry of every row, |dev - ref| <= E + 2^-24 |ref| (the float32 rounding of the output).

CRAFTED CLOUD (crafted_cloud): 128 isolated clusters of exactly 20 points (diameter <= 0.1, centres on a 10 m lattice offset by (300, -200, 50)),
so that every 20-NN, Radius 0.5 and Hybrid (0.5, 20) set is the point's own cluster and no neighbour search can be blamed for a wrong normal."""
from dataclasses import dataclass

import numpy as np

U23, U24, U53 = 2.0 ** -23, 2.0 ** -24, 2.0 ** -53
AMBIG_REL = 4e-6
AMBIG_CAP = 1e-3
KNN, RADIUS, HYBRID = 0, 1, 2


@dataclass
class Neighbours:
    mode: int
    k: int                       # list width (KNN / Hybrid: k; Radius: the largest ball)
    radius: float
    idx: np.ndarray              # (n, k) int64, members ordered by (d^2, index), -1 = none
    count: np.ndarray            # (n,) members
    alt: dict                    # row -> int64 array: the second acceptable member set of an ambiguous row
    next_d2: np.ndarray          # (n,) d^2 of the first non-member (inf: none)
    kth_d2: np.ndarray           # (n,) d^2 of the farthest member

    @property
    def ambiguous(self):
        a = np.zeros(len(self.idx), bool)
        a[list(self.alt)] = True
        return a


def neighbours(pts, mode, k=0, radius=0.0, chunk=512, window=True):
    """Neighbour sets of every point of `pts` (float32 rows, taken as exact) among `pts`, self included.  Distances are float64 and exact to
    rounding for every candidate.  For the radius-bounded modes the candidates of a chunk of queries are the points whose x lies within the
    radius (and a margin beyond the rim tolerance) of the chunk's x range -- nothing else can be a member or a rim point -- so next_d2 is then
    the first non-member among THOSE (inf: none that near); window=False compares against every point (the CPU test holds the two equal)."""
    p = np.ascontiguousarray(pts, dtype=np.float32).astype(np.float64)
    n = len(p)
    r2 = radius * radius if mode in (RADIUS, HYBRID) else np.inf
    bounded = mode != KNN and window
    perm = np.argsort(p[:, 0], kind="stable") if bounded else np.arange(n)
    xs = p[perm, 0]
    reach = radius * (1.0 + 1e-5) + 1e-12                                   # beyond it in x, d^2 > r^2 (1 + 4e-6)
    blocks, alt = [], {}
    next_d2 = np.full(n, np.inf); kth_d2 = np.zeros(n); count = np.zeros(n, np.int64)
    for a in range(0, n, chunk):
        rows = perm[a:a + chunk]
        q = p[rows]
        cols = perm[np.searchsorted(xs, xs[a] - reach, "left"):np.searchsorted(xs, xs[a + len(rows) - 1] + reach, "right")] if bounded else perm
        pc = p[cols]; m = len(cols)
        d2 = (q[:, None, 0] - pc[None, :, 0]) ** 2
        for ax in (1, 2):
            d2 += (q[:, None, ax] - pc[None, :, ax]) ** 2
        inside = (d2 < r2).sum(1)
        cnt = np.minimum(inside, k) if mode != RADIUS else inside
        if mode == KNN:
            cnt = np.full(len(q), min(k, n))
        w = min(m, int(cnt.max()) + 2)                                      # the members, the first non-member and one more, in (d^2, index) order
        local = np.argpartition(d2, w - 1, axis=1)[:, :w] if w < m else np.broadcast_to(np.arange(m), d2.shape)
        part = cols[local]; pd = np.take_along_axis(d2, local, 1)
        o = np.lexsort((part, pd), axis=1)
        order = np.take_along_axis(part, o, 1); sd = np.take_along_axis(pd, o, 1)
        sd = np.concatenate([sd, np.full((len(q), 1), np.inf)], 1)          # (no point beyond the last)
        blocks.append((rows, order[:, :int(cnt.max()) + 1], cnt))
        rr = np.arange(len(q))
        kth = np.where(cnt > 0, sd[rr, np.maximum(cnt - 1, 0)], 0.0); nxt = sd[rr, cnt]
        kth_d2[rows] = kth; next_d2[rows] = nxt; count[rows] = cnt
        full = cnt == k if mode != RADIUS else np.zeros(len(q), bool)
        tie = full & (nxt < r2) & (nxt - kth < AMBIG_REL * nxt)
        lo = (mode != KNN) & ~tie & (cnt > 0) & (kth > r2 * (1 - AMBIG_REL)) & ((mode == RADIUS) | (inside <= k))
        hi = (mode != KNN) & ~tie & ~lo & (nxt < r2 * (1 + AMBIG_REL)) & ((mode == RADIUS) | (cnt < k))
        for r in np.nonzero(tie | lo | hi)[0]:
            c = int(cnt[r]); members = order[r, :c]
            if tie[r]:
                alt[int(rows[r])] = np.concatenate([members[:-1], order[r, c:c + 1]])   # farthest member <-> first point outside
            elif lo[r]:
                alt[int(rows[r])] = members[:-1]                                         # the rim point left out
            else:
                alt[int(rows[r])] = order[r, :c + 1]                                     # the rim point taken in
    idx = np.full((n, max(int(count.max()), 1)), -1, np.int64)
    for rows, ri, rc in blocks:
        w = min(ri.shape[1], idx.shape[1])
        blk = ri[:, :w].copy()
        blk[np.arange(w)[None, :] >= rc[:, None]] = -1
        idx[rows, :w] = blk
    return Neighbours(mode, idx.shape[1], float(radius), idx, count, alt, next_d2, kth_d2)


def assert_ambiguity_cap(nb, what=""):
    """At most 0.1 % of the rows may be ambiguous -- asserted from the reference alone."""
    m = len(nb.alt)
    assert m <= AMBIG_CAP * len(nb.idx), (what, m, len(nb.idx))
    return m


def covariance(pts, idx):
    """Centred two-pass covariance in np.longdouble of the member rows `idx` ((n, k), -1 = none), divided by the count.  Returns (C (n, 3, 3), mu (n, 3),
    count (n,)) as longdouble; rows without members get zeros."""
    p = np.ascontiguousarray(pts, dtype=np.float32).astype(np.longdouble)
    idx = np.asarray(idx, np.int64)
    has = idx >= 0
    cnt = has.sum(1)
    x = p[np.where(has, idx, 0)] * has[:, :, None]
    den = np.maximum(cnt, 1).astype(np.longdouble)
    mu = x.sum(1) / den[:, None]
    d = (x - mu[:, None, :]) * has[:, :, None]
    C = np.einsum("nki,nkj->nij", d, d) / den[:, None, None]
    return C, mu, cnt


def error_bound(C, mu, cnt):
    """E = 4 (k + 3) 2^-53 (|mu|^2 + tr C): see the module docstring."""
    C = np.asarray(C, np.float64); mu = np.asarray(mu, np.float64)
    return 4.0 * (np.asarray(cnt, np.float64) + 3.0) * U53 * ((mu ** 2).sum(1) + np.trace(C, axis1=1, axis2=2))


def special_rule(C, cnt, prior=None):
    """(special (n,) bool, expected (n, 3) float64): the rows that follow the oracle's literal rule, and what it returns for them."""
    n = len(C)
    offz = (C[:, 0, 1] == 0) & (C[:, 0, 2] == 0) & (C[:, 1, 2] == 0)
    few = cnt < 3
    special = few | offz
    d = np.stack([C[:, 0, 0], C[:, 1, 1], C[:, 2, 2]], 1).astype(np.float64)
    d[few] = 1.0                                                            # identity covariance
    zero = (d == 0).all(1) & ~few                                           # all neighbours coincident
    exp = np.zeros((n, 3)); exp[:, 2] = 1.0
    ax = (d[:, 0] < d[:, 1]) & (d[:, 0] < d[:, 2])
    ay = ~ax & (d[:, 1] < d[:, 0]) & (d[:, 1] < d[:, 2])
    exp[ax] = (1.0, 0.0, 0.0); exp[ay] = (0.0, 1.0, 0.0)
    if prior is not None:
        pr = np.asarray(prior, np.float64)
        exp[zero] = pr[zero]
        flip = (exp * pr).sum(1) < 0
        exp[flip] = -exp[flip]
    return special, exp


def _row_measures(C, mu, cnt, nrm):
    """(residual, excess, bound, lmax) of unit vectors `nrm` against covariances C (longdouble), row by row."""
    Cd = np.asarray(C, np.float64)
    lam = np.linalg.eigvalsh(Cd)
    lmax = lam[:, 2]
    nl = nrm.astype(np.longdouble)
    Cn = np.einsum("nij,nj->ni", C, nl)
    rho = (nl * Cn).sum(1)
    res = np.sqrt((((Cn - rho[:, None] * nl)) ** 2).sum(1)).astype(np.float64)
    exc = (rho - lam[:, 0].astype(np.longdouble)).astype(np.float64)
    return res, exc, U23 * lmax + error_bound(Cd, mu, cnt), lmax


def measure_normals(pts, normals, nb, prior=None):
    """Every row of `normals` against the reference: dict of per-row arrays (unit, res, exc, bound, lmax, special, expected, ok) -- the best of the
    acceptable sets for an ambiguous row.  assert_normals_explained asserts on it; the CPU test reads the worst figures from it."""
    nrm = np.ascontiguousarray(normals, dtype=np.float64)
    n = len(nrm)
    assert nrm.shape == (n, 3) and len(nb.idx) == n
    pr = None if prior is None else np.ascontiguousarray(prior, dtype=np.float64)

    def one(idx, rows):
        C, mu, cnt = covariance(pts, idx)
        special, exp = special_rule(C, cnt, None if pr is None else pr[rows])
        v = nrm[rows]
        res, exc, bound, lmax = _row_measures(C, mu, cnt, v)
        unit = np.abs(np.sqrt((v ** 2).sum(1)) - 1.0)
        ok = (unit <= U23) & (res <= bound) & (exc <= bound)
        if pr is not None:
            ok &= (v * pr[rows]).sum(1) >= 0
        ok = np.where(special, (v == exp).all(1), ok)
        return dict(unit=unit, res=res, exc=exc, bound=bound, lmax=lmax, special=special, expected=exp, ok=ok)

    m = one(nb.idx, np.arange(n))
    for i, members in nb.alt.items():
        if not m["ok"][i]:
            a = one(members[None, :], np.array([i]))
            if a["ok"][0]:
                for key in m:
                    m[key][i] = a[key][0]
    return m


def assert_normals_explained(pts, normals, nb, prior=None, what="normals"):
    """Every row of `normals` (float32 values) is a unit eigenvector of the smallest eigenvalue of its neighbourhood's covariance, oriented by
    `prior`, or -- a special row -- equals the oracle's literal rule.  Returns the measures (measure_normals)."""
    m = measure_normals(pts, normals, nb, prior)
    g = ~m["special"]
    rel = np.where(g, np.maximum(m["res"], m["exc"]) / np.maximum(m["bound"], 1e-300), 0.0)
    print(f"{what}: {len(normals)} rows, {int(m['special'].sum())} special, {len(nb.alt)} ambiguous; worst |len-1| {m['unit'][g].max() if g.any() else 0:.2e}, "
          f"worst residual / bound {rel.max():.3f}, failing {int((~m['ok']).sum())}")
    bad = np.nonzero(~m["ok"])[0]
    if len(bad):
        i = int(bad[0])
        dot = None if prior is None else float((np.asarray(normals, np.float64)[i] * np.asarray(prior, np.float64)[i]).sum())
        raise AssertionError(f"{what}: {len(bad)} of {len(normals)} rows fail, first row {i}: normal {np.asarray(normals)[i]}, special {bool(m['special'][i])} "
                             f"(expected {m['expected'][i]}), |len-1| {m['unit'][i]:.3e}, residual {m['res'][i]:.3e}, excess {m['exc'][i]:.3e}, bound {m['bound'][i]:.3e}, "
                             f"lmax {m['lmax'][i]:.3e}, n.prior {dot}, members {int(nb.count[i])}, ambiguous {i in nb.alt}; rows {bad[:10].tolist()}")
    return m


def assert_covariances_explained(pts, cov, nb, what="covariances"):
    """Every entry of every row of `cov` ((n, 3, 3), float32 values): |dev - ref| <= E + 2^-24 |ref|; identity for rows of fewer than 3 neighbours."""
    dev = np.ascontiguousarray(cov, dtype=np.float64).reshape(-1, 3, 3)
    n = len(dev)

    def one(idx, rows):
        C, mu, cnt = covariance(pts, idx)
        ref = np.asarray(C, np.float64)
        E = error_bound(ref, mu, cnt)
        few = cnt < 3
        ref[few] = np.eye(3); E[few] = 0.0
        err = np.abs(dev[rows] - ref); tol = E[:, None, None] + U24 * np.abs(ref)
        return (err <= tol).all(axis=(1, 2)), (err / np.maximum(tol, 1e-300)).max(axis=(1, 2))

    ok, rel = one(nb.idx, np.arange(n))
    for i, members in nb.alt.items():
        if not ok[i]:
            o2, r2 = one(members[None, :], np.array([i]))
            if o2[0]:
                ok[i], rel[i] = True, r2[0]
    print(f"{what}: {n} rows, worst error / bound {rel.max():.3f}, failing {int((~ok).sum())}")
    bad = np.nonzero(~ok)[0]
    assert not len(bad), f"{what}: {len(bad)} of {n} rows fail, first row {int(bad[0])}: {dev[bad[0]].ravel()} (error / bound {rel[bad[0]]:.3g}); rows {bad[:10].tolist()}"
    return rel


# ------------------------------------------------------------------------------------------------------------------ crafted cloud
CLUSTER = 20
OFFSET = np.array([300.0, -200.0, 50.0])


def _rotation(rng):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def crafted_shapes():
    """[(name, (m, 3) float64 offsets from the cluster centre, m <= 20, within a ball of radius 0.05)]: 128 shapes."""
    rng = np.random.default_rng(20240607)
    out = []

    def spread(sig, along=None):
        """20 points with standard deviations `sig` along the axes (`along`: fixed, evenly spaced coordinates on the first axis), clipped into the
        ball, no two closer than 2e-3 (a voxel grid of 1e-3 keeps every one of them), under a random rotation."""
        while True:
            x = np.clip(rng.standard_normal((CLUSTER, 3)) * np.asarray(sig), -0.025, 0.025)
            if along is not None:
                x[:, 0] = along
            d = np.linalg.norm(x[:, None, :] - x[None, :, :], axis=2) + np.eye(CLUSTER)
            if d.min() > 2e-3:
                return x @ _rotation(rng).T

    grid = np.array([[i, j, 0] for i in range(5) for j in range(4)], float)
    grid -= grid.mean(0)
    for t in (1e-2, 1e-5, 0.0):                                             # noisy planes: thickness 1e-2, 1e-5 and exactly flat (before rotation)
        for _ in range(10):
            out.append((f"plane{t:g}", spread((0.012, 0.012, t * 0.5))))
    for _ in range(10):                                                     # needles
        out.append(("needle", spread((0.0, 1.2e-5, 1.7e-5), along=np.linspace(-0.024, 0.024, CLUSTER))))
    for _ in range(10):                                                     # discs: regular 20-gons, two equal large eigenvalues
        a = 2 * np.pi * np.arange(CLUSTER) / CLUSTER
        out.append(("disc", np.stack([0.04 * np.cos(a), 0.04 * np.sin(a), np.zeros(CLUSTER)], 1) @ _rotation(rng).T))
    for _ in range(10):                                                     # near-isotropic blobs
        out.append(("blob", spread((0.01, 0.01 * (1 + 1e-3), 0.01 * (1 - 1e-3)))))
    # axis-aligned grids on dyadic coordinates: every moment is exact in float64, the off-diagonal ones vanish exactly -> the diagonal branch
    h = 2.0 ** -7
    for perm in ((0, 1, 2), (1, 2, 0), (2, 0, 1)):                          # 5 x 4 x 1 steps: the flat axis is z, x, y in turn
        for _ in range(6):
            out.append((f"grid{perm[2]}", (grid * h)[:, np.argsort(perm)]))
    box = np.array([[i, j, l] for i in range(5) for j in range(2) for l in range(2)], float); box -= box.mean(0)
    for _ in range(6):                                                      # 5 x 2 x 2: the two small diagonal entries tie -> z
        out.append(("gridtie", box * h))
    for _ in range(6):
        out.append(("gridtie_yx", (box * h)[:, [1, 0, 2]]))                 # ... the long axis is y, x and z tie -> z
    line = (np.arange(CLUSTER) - 9.5)[:, None] * h / 4
    for _ in range(6):                                                      # a line along z: the quirk (z, the line's own direction)
        out.append(("line_z", line * np.array([0.0, 0.0, 1.0])))
    for _ in range(6):
        out.append(("line_x", line * np.array([1.0, 0.0, 0.0])))
    for _ in range(6):                                                      # a line along a diagonal: off-diagonal moments, a proper normal
        out.append(("line_diag", line * np.array([1.0, 1.0, 1.0])))
    for _ in range(4):
        out.append(("coincident", np.zeros((CLUSTER, 3))))
    for m in (1, 2, 3):                                                     # clusters cut to 1, 2 and 3 points
        for _ in range(4):
            out.append((f"cut{m}", spread((0.012, 0.012, 0.012))[:m]))
    while len(out) < 128:
        out.append(("plane0.01", spread((0.012, 0.012, 5e-3))))
    assert len(out) == 128
    return out


def crafted_cloud(with_cut=True):
    """(points float32 (N, 3), cluster id per point, shape name per cluster).  Cluster c sits at lattice node (c % 8, c // 8 % 4, c // 32) x 10 m +
    (300, -200, 50); the order of the points is shuffled with a fixed seed.  with_cut=False leaves out the clusters cut to 1, 2 and 3 points: the
    cloud for plain KNN 20, whose sets would otherwise reach over to the (equidistant) lattice neighbours of a cut cluster."""
    shapes = crafted_shapes()
    pts, lab = [], []
    for c, (nm, x) in enumerate(shapes):
        if nm.startswith("cut") and not with_cut:
            continue
        centre = OFFSET + 10.0 * np.array([c % 8, c // 8 % 4, c // 32], float)
        pts.append(centre + x); lab.append(np.full(len(x), c))
    pts = np.concatenate(pts).astype(np.float32); lab = np.concatenate(lab)
    order = np.random.default_rng(7).permutation(len(pts))
    return pts[order], lab[order], [nm for nm, _ in shapes]


def fixed_prior(n, seed):
    """A fixed-seed random unit field (float32)."""
    v = np.random.default_rng(seed).standard_normal((n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------ scale clouds
def eigh_vectors(pts, idx, which=0):
    """Unit eigenvectors (float32) of the `which`-th smallest eigenvalue of the reference covariance of the member rows, by np.linalg.eigh.  Used
    only to BUILD answers (wrong ones, for the rejection tests); no assertion compares against it."""
    C, _, _ = covariance(pts, idx)
    _, v = np.linalg.eigh(np.asarray(C, np.float64))
    return v[:, :, which].astype(np.float32)


def lexsorted(a):
    """Row order that sorts the rows of `a` lexicographically (x, then y, then z)."""
    return np.lexsort((a[:, 2], a[:, 1], a[:, 0]))


def fallback_rows(vox_pts, keep, sor_k, normal_k):
    """Kept rows of the voxel cloud (as indices into the CLEANED cloud) whose sor_k-nearest list in the un-cleaned cloud holds fewer than normal_k
    survivors: the rows the filter's lists cannot serve, which the product searches again (all kept rows when normal_k > sor_k).  Also returns
    the sor_k-NN sets of the un-cleaned cloud."""
    nb = neighbours(vox_pts, KNN, sor_k)
    surv = (keep[np.maximum(nb.idx, 0)] & (nb.idx >= 0)).sum(1)
    fb = keep & ((surv < normal_k) & (nb.count == sor_k) if normal_k <= sor_k else True)
    pos = np.cumsum(keep) - 1
    return pos[fb], nb


def scale_cloud_reference(oracle, xyz, prior, voxel, sor_k, sor_std):
    """What the reference pipeline makes of one cloud at one scale (voxel grid, outlier filter; float64 oracle), as float32 rows in the oracle's
    order: dict(points, prior (voxel means of `prior` at the kept rows, or None), n_voxel, n_clean, vox_points, keep)."""
    if prior is not None:
        vp, vn = oracle.voxel_down_sample(xyz, voxel, normals=prior)
    else:
        vp, vn = oracle.voxel_down_sample(xyz, voxel), None
    keep = oracle.remove_statistical_outlier(vp, sor_k, sor_std)[0]
    return dict(points=vp[keep].astype(np.float32), prior=None if vn is None else vn[keep].astype(np.float32), n_voxel=len(vp), n_clean=int(keep.sum()),
                vox_points=vp.astype(np.float32), keep=keep)
