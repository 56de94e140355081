"""The numpy normal reference (tests/normal_reference.py) against the CPU oracle, without a device: that its bounds and its ambiguity cap are not
too tight (the oracle passes on every row), that the solver the device shares with the oracle holds the bounds on hard spectra, and that the
reference rejects the wrong answers it was built to catch.

Measured with the oracle on golden pair 899 (source and target at voxel 0.5 and 0.3; float32-rounded normals unless noted):
  * worst eigenvector residual 5.7e-8 lmax and worst Rayleigh excess 5.0e-8 lmax, i.e. at most 0.48 of the bound (2^-23 + E / lmax) lmax -- all of it
    the float32 rounding of the output: the oracle's unrounded float64 normals show 1.0e-12 lmax on KNN rows and 4.1e-10 lmax on the sparse
    Hybrid / Radius rows (residual), 6.5e-12 lmax (excess);
  * worst | |n| - 1 | 4.6e-8 (bound 1.19e-7);
  * covariances: worst error 0.998 of E + 2^-24 |ref| (the float32 rounding alone reaches 1.0 of its half ulp);
  * ambiguous rows per cloud (source 0.5, source 0.3, target 0.5, target 0.3): KNN 20: 0, 1, 0, 0; KNN 65: 3, 1, 1, 0; Hybrid (0.6, 20) and
    Radius 0.6: 0, 0, 0, 2; the cleaned clouds (30, 1.0, 20): 0, 1, 0, 0 (cap: 3 to 7 rows);
  * hard spectra through oracle.fast_eigen3x3 (unrounded float64 output), worst residual: thin plane 4.0e-11 lmax, needle 3.8e-11 lmax, two equal
    largest 3.0e-16, near-isotropic 1.1e-15, plain 2.8e-16 (test_hard_spectra prints them);
  * rejections on the cleaned source at 0.5: middle eigenvector -- residual inside the bound on every row, excess outside on every row; farthest
    member swapped: 3,926 of 3,926 rows caught; un-cleaned neighbours: 15 of 15 fallback rows caught."""
import numpy as np
import pytest

import normal_reference as NR

VOXELS = (0.5, 0.3)
FORMS = [("knn20", NR.KNN, 20, 0.0), ("knn65", NR.KNN, 65, 0.0), ("hybrid", NR.HYBRID, 20, 0.6), ("radius", NR.RADIUS, 0, 0.6)]


def _oracle_mode(oracle, mode):
    return {NR.KNN: oracle.SEARCH_KNN, NR.HYBRID: oracle.SEARCH_HYBRID, NR.RADIUS: oracle.SEARCH_RADIUS}[mode]


def _worst(m):
    g = ~m["special"]
    return float((m["res"][g] / m["lmax"][g]).max()), float((m["exc"][g] / m["lmax"][g]).max())


@pytest.mark.parametrize("voxel", VOXELS)
@pytest.mark.parametrize("which", ["source", "target"])
def test_oracle_passes_on_raw_voxel_clouds(oracle, small_pair, which, voxel):
    pts = oracle.voxel_down_sample(small_pair[which], voxel).astype(np.float32)
    for name, mode, k, r in FORMS:
        nb = NR.neighbours(pts, mode, k, r)
        amb = NR.assert_ambiguity_cap(nb, name)
        nrm = oracle.estimate_normals(pts, _oracle_mode(oracle, mode), max(k, 1), r).astype(np.float32)
        m = NR.assert_normals_explained(pts, nrm, nb, what=f"{which} {voxel} {name}")
        NR.assert_covariances_explained(pts, oracle.estimate_covariances(pts, _oracle_mode(oracle, mode), max(k, 1), r).astype(np.float32), nb, what=f"{which} {voxel} {name}")
        print(f"{which} {voxel} {name}: ambiguous {amb}, worst residual / lmax {_worst(m)[0]:.2e}, worst excess / lmax {_worst(m)[1]:.2e}")
        if mode != NR.KNN:
            assert (nb.count < 3).sum() >= 100                               # sparse rows: the (0, 0, 1) rule is exercised


@pytest.mark.parametrize("voxel", VOXELS)
@pytest.mark.parametrize("which", ["source", "target"])
def test_oracle_passes_on_cleaned_clouds(oracle, small_pair, which, voxel):
    raw = small_pair[which].astype(np.float32)
    field = NR.fixed_prior(len(raw), 5)
    for prior in (None, field):
        sc = NR.scale_cloud_reference(oracle, raw, prior, voxel, 30, 1.0)
        nb = NR.neighbours(sc["points"], NR.KNN, 20)
        NR.assert_ambiguity_cap(nb)
        nrm = oracle.estimate_normals(sc["points"], oracle.SEARCH_KNN, 20, prior=sc["prior"]).astype(np.float32)
        NR.assert_normals_explained(sc["points"], nrm, nb, prior=sc["prior"], what=f"cleaned {which} {voxel} prior {prior is not None}")
        if prior is not None:
            assert 0.05 < np.linalg.norm(sc["prior"], axis=1).mean() < 0.95      # a voxel-mean prior: not a unit field any more


@pytest.mark.parametrize("mode,k,r", [(NR.HYBRID, 20, 0.6), (NR.RADIUS, 0, 0.6)])
def test_windowed_candidates_equal_all_candidates(oracle, small_pair, mode, k, r):
    """The radius-bounded modes compare a chunk of queries with the points near it in x only: same sets, counts, rim rows and alternatives as the
    comparison with every point; the first non-member agrees wherever it is near enough to matter."""
    pts = oracle.voxel_down_sample(small_pair["target"], 0.3).astype(np.float32)
    a, b = NR.neighbours(pts, mode, k, r), NR.neighbours(pts, mode, k, r, window=False)
    assert np.array_equal(a.idx, b.idx) and np.array_equal(a.count, b.count) and np.array_equal(a.kth_d2, b.kth_d2)
    assert sorted(a.alt) == sorted(b.alt) and all(np.array_equal(a.alt[i], b.alt[i]) for i in a.alt) and len(a.alt) >= 1
    near = b.next_d2 < r * r * (1 + 1e-5)
    assert near.any() and np.array_equal(a.next_d2[near], b.next_d2[near]) and (a.next_d2 >= b.next_d2).all()


def _spectrum_cases():
    rng = np.random.default_rng(11)
    spectra = {"thin plane": (0.0, 1e-14, 1e-8), "needle": (1e-6, 2e-6, 1.0), "two equal largest": (0.1, 1.0, 1.0), "near-isotropic": (1 - 2e-6, 1 - 1e-6, 1.0),
               "plain": (0.01, 0.3, 1.0)}
    for name, lam in spectra.items():
        for scale in (1.0, 1e-20, 1e20):
            for _ in range(50):
                R = NR._rotation(rng)
                C = (R * (np.asarray(lam) * scale)) @ R.T
                yield name, scale, (C + C.T) / 2


def test_hard_spectra(oracle):
    """Prescribed spectra under random rotations through the solver the device shares with the oracle: unit length, residual and Rayleigh excess
    within the float32 output's bound, for the float64 output and for its float32 rounding."""
    worst = {}
    for name, scale, C in _spectrum_cases():
        n = oracle.fast_eigen3x3(C)
        Cl = C.astype(np.longdouble)[None]
        for v in (n.astype(np.float32).astype(np.float64), n):
            res, exc, bound, lmax = NR._row_measures(Cl, np.zeros((1, 3)), np.array([20]), v[None])
            assert abs(np.linalg.norm(v) - 1) <= NR.U23, (name, scale, v)
            assert res[0] <= bound[0] and exc[0] <= bound[0], (name, scale, res[0] / lmax[0], exc[0] / lmax[0])
        worst[name] = max(worst.get(name, 0.0), float(res[0] / lmax[0]))      # (of the unrounded float64 output)
    print("worst float64 residual / lmax:", {k: f"{v:.1e}" for k, v in worst.items()})


def test_diagonal_branch_rule_equals_the_oracle(oracle):
    """Axis-aligned permutations, ties, the zero matrix and the identity: special_rule restates the oracle's literal rule."""
    prior = np.array([[0.3, -0.2, -0.9]])
    for d in [(1, 2, 3), (3, 1, 2), (2, 3, 1), (3, 2, 1), (1, 1, 2), (2, 1, 1), (1, 2, 1), (0, 0, 5), (5, 0, 0), (0, 5, 0), (1, 1, 1), (0, 0, 0), (1e-20, 3e-20, 2e-20)]:
        C = np.diag(np.asarray(d, float))
        n = oracle.fast_eigen3x3(C)
        special, exp = NR.special_rule(C[None].astype(np.longdouble), np.array([20]))
        assert special[0]
        if any(d):
            assert np.array_equal(n, exp[0]), (d, n, exp)
        else:
            assert not n.any() and np.array_equal(exp[0], (0, 0, 1))          # the zero vector becomes (0, 0, 1) in estimate_normals ...
            assert np.array_equal(NR.special_rule(C[None].astype(np.longdouble), np.array([20]), prior)[1][0], prior[0])      # ... or the prior itself
    assert np.array_equal(NR.special_rule(np.diag([1.0, 2.0, 3.0])[None], np.array([20]), prior)[1][0], (1, 0, 0))           # n . prior > 0: kept
    assert np.array_equal(NR.special_rule(np.diag([3.0, 2.0, 1.0])[None], np.array([20]), prior)[1][0], (0, 0, -1))          # n . prior < 0: flipped
    assert np.array_equal(NR.special_rule(np.diag([3.0, 2.0, 1.0])[None], np.array([20]), np.array([[1.0, 1.0, 0.0]]))[1][0], (0, 0, 1))     # == 0: not flipped


def test_crafted_cloud_is_what_it_claims_and_the_oracle_passes(oracle):
    for mode, k, r in ((NR.KNN, 20, 0.0), (NR.HYBRID, 20, 0.5), (NR.RADIUS, 0, 0.5)):
        pts, lab, names = NR.crafted_cloud(with_cut=mode != NR.KNN)
        prior = NR.fixed_prior(len(pts), 9)
        nb = NR.neighbours(pts, mode, k, r)
        assert not nb.alt
        assert ((lab[np.maximum(nb.idx, 0)] == lab[:, None]) | (nb.idx < 0)).all() and (nb.count == np.bincount(lab)[lab]).all()      # its own cluster, all of it
        assert (nb.next_d2 > 25.0).all() and (nb.kth_d2 <= 0.01).all()
        om = _oracle_mode(oracle, mode)
        for pr in (None, prior):
            nrm = oracle.estimate_normals(pts, om, max(k, 1), r, prior=pr).astype(np.float32)
            m = NR.assert_normals_explained(pts, nrm, nb, prior=pr, what=f"crafted {mode}")
        NR.assert_covariances_explained(pts, oracle.estimate_covariances(pts, om, max(k, 1), r).astype(np.float32), nb, what=f"crafted {mode}")
    # the shapes meant for the special rows are special, the others are not
    sp = {nm: m["special"][np.isin(lab, [c for c, x in enumerate(names) if x == nm])] for nm in set(names)}
    for nm, v in sp.items():
        assert v.all() == (nm.startswith(("grid", "line_z", "line_x", "coincident", "cut1", "cut2"))), (nm, v.mean())
    z = np.isin(lab, [c for c, x in enumerate(names) if x == "line_z"])
    assert (m["expected"][z][:, :2] == 0).all() and (np.abs(m["expected"][z][:, 2]) == 1).all()          # the quirk: the line's own direction


@pytest.fixture(scope="module")
def scan(oracle, small_pair):
    raw = small_pair["source"].astype(np.float32)
    prior = NR.fixed_prior(len(raw), 5)
    sc = NR.scale_cloud_reference(oracle, raw, prior, 0.5, 30, 1.0)
    nb = NR.neighbours(sc["points"], NR.KNN, 20)
    nrm = oracle.estimate_normals(sc["points"], oracle.SEARCH_KNN, 20, prior=sc["prior"]).astype(np.float32)
    NR.assert_normals_explained(sc["points"], nrm, nb, prior=sc["prior"])
    return sc, nb, nrm


def _rejected(sc, nb, nrm, rows, wrong, prior=True):
    """Rows `rows` replaced by `wrong`: the assertion must raise, and measure_normals says which of the rows it caught."""
    bad = nrm.copy(); bad[rows] = wrong
    with pytest.raises(AssertionError):
        NR.assert_normals_explained(sc["points"], bad, nb, prior=sc["prior"] if prior else None)
    return ~NR.measure_normals(sc["points"], bad, nb, prior=sc["prior"] if prior else None)["ok"][rows]


def test_rejects_the_middle_eigenvector(scan):
    sc, nb, nrm = scan
    rows = np.arange(len(nrm))
    mid = NR.eigh_vectors(sc["points"], nb.idx, 1)
    m = NR.measure_normals(sc["points"], mid, nb)
    assert ((m["res"] <= m["bound"]) & (m["exc"] > m["bound"])).all()            # an eigenvector all right, of the wrong eigenvalue: only the excess says so
    assert _rejected(sc, nb, nrm, rows[:1], mid[:1], prior=False).all()


def test_rejects_a_set_with_the_farthest_member_swapped(scan):
    sc, nb, nrm = scan
    rows = np.array([i for i in range(len(nrm)) if i not in nb.alt])
    p = sc["points"].astype(np.float64)
    d2 = ((p[:, None, :] - p[None, :, :]) ** 2).sum(2)
    order = np.lexsort((np.broadcast_to(np.arange(len(p)), d2.shape), d2), axis=1)
    swapped = np.concatenate([order[:, :19], order[:, 20:21]], 1)
    wrong = NR.eigh_vectors(sc["points"], swapped)
    wrong[(wrong * sc["prior"]).sum(1) < 0] *= -1
    caught = _rejected(sc, nb, nrm, rows, wrong[rows])
    print("swapped farthest member: caught", caught.sum(), "of", len(rows))
    assert caught.mean() > 0.99          # (a swap that moves the normal by less than the float32 output's resolution cannot be seen, nor does it matter)


def test_rejects_uncleaned_neighbours_on_fallback_rows(scan):
    sc, nb, nrm = scan
    fb, nb_vox = NR.fallback_rows(sc["vox_points"], sc["keep"], 30, 20)
    assert len(fb) >= 10
    kept = np.nonzero(sc["keep"])[0]
    wrong = NR.eigh_vectors(sc["vox_points"], nb_vox.idx[kept[fb], :20])         # the 20 nearest of the UN-cleaned cloud, removed points included
    wrong[(wrong * sc["prior"][fb]).sum(1) < 0] *= -1
    caught = _rejected(sc, nb, nrm, fb, wrong)
    print("un-cleaned neighbours on fallback rows: caught", caught.sum(), "of", len(fb))
    assert caught.all()


def test_rejects_a_flipped_normal_and_a_long_one(scan):
    sc, nb, nrm = scan
    assert _rejected(sc, nb, nrm, np.array([17]), -nrm[17:18]).all()
    NR.assert_normals_explained(sc["points"], -nrm, nb)                          # (without a prior either sign is a normal)
    assert _rejected(sc, nb, nrm, np.array([17]), (nrm[17:18].astype(np.float64) * (1 + 1e-6)).astype(np.float32)).all()
