"""The normals the GICP loops consume, and the public normal / covariance estimators, row by row against tests/normal_reference.py.

The scale clouds of pcr_multiscale_gicp, pcr_register_pairs and the lockstep groups (voxel grid, outlier filter, normals of the cleaned cloud from
the filter's k-best lists, fallback search for the rows the lists cannot serve) come back through pcr_debug_scale_clouds, which runs the product's
own preparation code in its three forms.  Every row is checked: counts and points against the CPU oracle, normals as unit eigenvectors of the
smallest eigenvalue of the reference covariance of the row's neighbours IN THE CLEANED CLOUD, oriented by the voxel-mean prior; the three forms
bit for bit against each other.  No tolerance here is a share of rows (see normal_reference.py for the bounds and the one cap, asserted from the
reference before the device is consulted; tests/test_normal_reference.py shows that the CPU oracle passes and that wrong answers do not)."""
import numpy as np
import pytest

import normal_reference as NR
from conftest import pkg

pytestmark = pytest.mark.gpu

VOXELS = (0.5, 0.3)
# (sor_k, std, normal_k): product values (fused lists + piece-list fallback); normal_k == sor_k (many fallback rows); normal_k > sor_k (no
# fusion, every kept row searched with the keep filter); config 5 (forms 1 and 2 decline, form 0 serves it through the wide-slot kernels)
PARAMS = [(30, 1.0, 20), (30, 0.5, 30), (20, 1.0, 30), (30, 1.0, 64)]


@pytest.fixture(scope="module")
def P():
    return pkg()


@pytest.fixture
def knn_form(P):
    yield lambda form, budget=80: (P._lib.set_option("knn_wave", form), P._lib.set_option("knnw_budget", budget))
    P._lib.set_option("knn_wave", -1)
    P._lib.set_option("knnw_budget", 80)


_cache = {}


def _memo(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _raw(small_pair, which):
    return small_pair[which].astype(np.float32)


def _field(small_pair, which):
    return NR.fixed_prior(len(small_pair[which]), 5 if which == "source" else 6)


def _scale_ref(oracle, small_pair, which, with_prior, voxel, params):
    """The reference scale cloud, its neighbour sets (cleaned cloud, normal_k) and its fallback rows -- nothing of it from the device."""
    sor_k, std, normal_k = params
    sc = _memo(("sc", which, with_prior, voxel, sor_k, std),
               lambda: NR.scale_cloud_reference(oracle, _raw(small_pair, which), _field(small_pair, which) if with_prior else None, voxel, sor_k, std))
    nb = _memo(("nb", which, voxel, sor_k, std, normal_k), lambda: NR.neighbours(sc["points"], NR.KNN, normal_k))
    if normal_k > sor_k:
        n_fallback = sc["n_clean"]                                            # no list can serve: every kept row is searched
    else:
        nbv = _memo(("nbv", which, voxel, sor_k), lambda: NR.neighbours(sc["vox_points"], NR.KNN, sor_k))
        keep = sc["keep"]
        surv = (keep[np.maximum(nbv.idx, 0)] & (nbv.idx >= 0)).sum(1)
        n_fallback = int((keep & (surv < normal_k) & (nbv.count == sor_k)).sum())
    return sc, nb, n_fallback


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _check_cloud(dev, sc, nb, what):
    """One device scale cloud (points, normals, n_voxel, untouched) against its reference."""
    pts, nrm, n_voxel, untouched = dev
    assert untouched, what                                                    # nothing past the clean count
    assert n_voxel == sc["n_voxel"] and len(pts) == sc["n_clean"], (what, n_voxel, len(pts), sc["n_voxel"], sc["n_clean"])
    od, orf = NR.lexsorted(pts), NR.lexsorted(sc["points"])
    assert np.array_equal(_bits(pts[od]), _bits(sc["points"][orf])), what      # the float32 rounding of the oracle's rows, as a set
    # the reference's neighbour sets and prior live in the oracle's row order: bring the device's normals there
    back = np.empty(len(od), np.int64); back[orf] = od
    NR.assert_normals_explained(sc["points"], nrm[back], nb, prior=sc["prior"], what=what)


@pytest.mark.parametrize("params", PARAMS, ids=lambda p: "sor%d_%g_k%d" % p)
@pytest.mark.parametrize("with_prior", [False, True], ids=["noprior", "prior"])
def test_scale_clouds_row_by_row(P, oracle, small_pair, with_prior, params):
    """Source (cloud 0, no tree) and target (cloud 1, with its tree) of pair 899 at voxel 0.5 and 0.3 through the three forms of the preparation."""
    sor_k, std, normal_k = params
    refs = {}
    for c, which in enumerate(("source", "target")):
        for s, voxel in enumerate(VOXELS):
            sc, nb, n_fb = _scale_ref(oracle, small_pair, which, with_prior, voxel, params)
            NR.assert_ambiguity_cap(nb, (which, voxel))
            assert n_fb >= 10, (which, voxel, n_fb)                          # the fallback search is exercised -- known from the reference alone
            print(f"{which} {voxel}: {sc['n_voxel']} voxels, {sc['n_clean']} kept, {n_fb} fallback rows, {len(nb.alt)} ambiguous")
            refs[c, s] = (sc, nb)
    clouds = [_raw(small_pair, "source"), _raw(small_pair, "target")]
    priors = [_field(small_pair, "source"), _field(small_pair, "target")] if with_prior else None
    out = [P._lib.debug_scale_clouds(clouds, priors, VOXELS, sor_k, std, normal_k, form) for form in (0, 1, 2)]
    assert out[0] is not None                                                # the scale-by-scale path serves everything
    if normal_k > 32:
        assert out[1] is None and out[2] is None                             # the decline of the batched forms is reported, nothing written
    else:
        assert out[1] is not None and out[2] is not None
    for (c, s), (sc, nb) in refs.items():
        _check_cloud(out[0][c][s], sc, nb, f"form 0 cloud {c} voxel {VOXELS[s]} {params}")
        for form in (1, 2):
            if out[form] is None:
                continue
            # "same per-problem arithmetic ... bit-identical results": the forms agree in every bit
            for what, a, b in (("points", out[form][c][s][0], out[0][c][s][0]), ("normals", out[form][c][s][1], out[0][c][s][1])):
                assert a.shape == b.shape, (form, c, s, what)
                differ = np.nonzero((_bits(a) != _bits(b)).any(1))[0]
                assert not len(differ), f"form {form} against form 0, cloud {c} voxel {VOXELS[s]} {params}: {len(differ)} rows of the {what} differ, first {differ[:5]}: {a[differ[:2]]} / {b[differ[:2]]}"
            assert out[form][c][s][2:] == out[0][c][s][2:]


def test_group_indexing(P, oracle, small_pair):
    """A group of two pairs whose four clouds differ in size, only the first and the last with a prior: the group batch (form 2) gives for every
    cloud the rows of that cloud prepared by itself (form 1 takes the clouds one by one).  Pins the priors[k] / todos[k] / counter indexing."""
    src, tgt = _raw(small_pair, "source"), _raw(small_pair, "target")
    clouds = [src, tgt[:11000], src[2500:14001], tgt]
    priors = [NR.fixed_prior(len(clouds[0]), 21), None, None, NR.fixed_prior(len(clouds[3]), 24)]
    assert len({len(c) for c in clouds}) == 4
    grp = P._lib.debug_scale_clouds(clouds, priors, VOXELS, 30, 1.0, 20, 2)
    one = P._lib.debug_scale_clouds(clouds, priors, VOXELS, 30, 1.0, 20, 1)
    assert grp is not None and one is not None
    for c in range(4):
        alone = P._lib.debug_scale_clouds([clouds[c]] if c % 2 == 0 else [clouds[0][:2000], clouds[c]], None if priors[c] is None else [priors[c]] if c % 2 == 0 else [None, priors[c]],
                                          VOXELS, 30, 1.0, 20, 2)[c % 2]
        for s in range(len(VOXELS)):
            for other, name in ((one[c], "cloud by cloud"), (alone, "alone")):
                assert grp[c][s][2:] == other[s][2:] and grp[c][s][3], (c, s, name)
                assert np.array_equal(_bits(grp[c][s][0]), _bits(other[s][0])), (c, s, name)
                assert np.array_equal(_bits(grp[c][s][1]), _bits(other[s][1])), (c, s, name)
    # the priors reached their own clouds: clouds 0 and 3 are oriented by theirs, and a cloud without one is not
    for c in (0, 3):
        for s, voxel in enumerate(VOXELS):
            sc = NR.scale_cloud_reference(oracle, clouds[c], priors[c], voxel, 30, 1.0)
            pts, nrm = grp[c][s][:2]
            back = np.empty(len(pts), np.int64); back[NR.lexsorted(sc["points"])] = NR.lexsorted(pts)
            assert np.array_equal(_bits(pts[back]), _bits(sc["points"]))
            assert ((nrm[back].astype(np.float64) * sc["prior"]).sum(1) >= 0).all(), (c, s)
    for c, seed in ((1, 21), (2, 24)):
        pts, nrm = grp[c][0][:2]
        assert ((nrm * NR.fixed_prior(len(nrm), seed)).sum(1) < 0).mean() > 0.3        # (no hidden orientation)


def test_declines_are_reported_and_write_nothing(P, oracle, small_pair):
    """Forms 1 and 2 decline where the product falls back to the next path -- one scale, sor_k > 32, normal_k > 32 (test_scale_clouds_row_by_row),
    the merged voxel pass declining (three scales whose index does not fit above 63 Morton bits: tests/voxel_reference.py, case merged63) --
    and leave the caller's buffers alone (debug_scale_clouds checks that); form 0 serves all of them with the oracle's counts and points."""
    import voxel_reference as VR
    src = _raw(small_pair, "source")[:6000]
    for cloud, voxels, sor_k in ((src, (0.5,), 30), (src, (0.5, 0.3), 33), (VR.case("merged63").xyz, (1.0, 2.0, 4.0), 30)):
        assert P._lib.debug_scale_clouds([cloud, cloud], None, voxels, sor_k, 1.0, 20, 1) is None
        assert P._lib.debug_scale_clouds([cloud, cloud], None, voxels, sor_k, 1.0, 20, 2) is None
        out = P._lib.debug_scale_clouds([cloud, cloud], None, voxels, sor_k, 1.0, 20, 0)
        for s, voxel in enumerate(voxels):
            sc = NR.scale_cloud_reference(oracle, cloud, None, voxel, sor_k, 1.0)
            for c in (0, 1):
                pts, nrm, n_voxel, untouched = out[c][s]
                assert untouched and n_voxel == sc["n_voxel"] and len(pts) == sc["n_clean"], (voxels, sor_k, c, s)
                assert np.array_equal(_bits(pts[NR.lexsorted(pts)]), _bits(sc["points"][NR.lexsorted(sc["points"])]))
                assert (np.abs(np.linalg.norm(nrm.astype(np.float64), axis=1) - 1) <= NR.U23).all()
    assert P._lib.debug_scale_clouds([src, src], None, (0.5, 0.3), 30, 1.0, 20, 1) is not None      # (the same cloud is taken when nothing stands in the way)


# ------------------------------------------------------------------------------------------------------------- public entry points
SEARCHES = {"knn20": (NR.KNN, 20, 0.0), "knn64": (NR.KNN, 64, 0.0), "knn65": (NR.KNN, 65, 0.0), "hybrid": (NR.HYBRID, 20, 0.6), "radius": (NR.RADIUS, 0, 0.6)}


def _param(P, mode, k, r):
    return {NR.KNN: lambda: P.KDTreeSearchParamKNN(knn=k), NR.HYBRID: lambda: P.KDTreeSearchParamHybrid(radius=r, max_nn=k), NR.RADIUS: lambda: P.KDTreeSearchParamRadius(radius=r)}[mode]()


def _public_rows(P, knn_form, pts, nb, mode, k, r, prior, what):
    """estimate_normals (without and with `prior`) and estimate_covariances of `pts` through every kernel form that serves the search."""
    waves = (0, 1) if mode != NR.RADIUS and k <= 64 else (0,)                # the one-query-per-lane kernel: k <= 64, not the radius walk
    for wave in waves:
        knn_form(wave, 3)                                                    # budget 3: most wavefronts are handed over to the octet kernel
        for pr in (None, prior):
            pc = P.PointCloud(pts)
            if pr is not None:
                pc.normals = pr
            pc.estimate_normals(_param(P, mode, k, r))
            NR.assert_normals_explained(pts, pc.normals.astype(np.float32), nb, prior=pr, what=f"{what} wave {wave} prior {pr is not None}")
        pc = P.PointCloud(pts)
        pc.estimate_covariances(_param(P, mode, k, r))
        NR.assert_covariances_explained(pts, pc.covariances, nb, what=f"{what} wave {wave}")


@pytest.mark.parametrize("search", ["knn20", "knn64", "knn65", "radius"])
@pytest.mark.parametrize("cloud", [("source", 0.3), ("target", 0.5)], ids=["source0.3", "target0.5"])
def test_public_normals_and_covariances_row_by_row(P, oracle, small_pair, knn_form, cloud, search):
    which, voxel = cloud
    mode, k, r = SEARCHES[search]
    pts = oracle.voxel_down_sample(small_pair[which], voxel).astype(np.float32)
    nb = NR.neighbours(pts, mode, k, r)
    NR.assert_ambiguity_cap(nb, (cloud, search))
    _public_rows(P, knn_form, pts, nb, mode, k, r, NR.fixed_prior(len(pts), 3), f"{which} {voxel} {search}")


def test_public_hybrid_on_the_raw_cloud_row_by_row(P, small_pair, knn_form):
    """Hybrid (0.6, 20) on the raw scan: full rows, rows the radius cuts short, and rows of fewer than 3 neighbours -> (0, 0, 1)."""
    pts = _raw(small_pair, "source")
    mode, k, r = SEARCHES["hybrid"]
    nb = NR.neighbours(pts, mode, k, r)
    NR.assert_ambiguity_cap(nb, "raw hybrid")
    assert (nb.count < 3).sum() >= 10 and ((nb.count >= 3) & (nb.count < k)).sum() >= 100 and (nb.count == k).sum() >= 100
    _public_rows(P, knn_form, pts, nb, mode, k, r, NR.fixed_prior(len(pts), 4), "raw source hybrid")


# ------------------------------------------------------------------------------------------------------------- crafted cloud
@pytest.mark.parametrize("search", ["knn", "hybrid", "radius"])
def test_crafted_clusters_row_by_row(P, knn_form, search):
    """128 isolated clusters whose neighbour sets are the clusters themselves: planes down to thickness 0, needles, discs, blobs, the exact diagonal
    branch in its permutations and ties, lines, coincident points, clusters of 1, 2 and 3 points.  Every row passes the reference; for KNN the 20
    rows of a cluster are equal in bits (same set, and the sums must not depend on the order the search found the members in)."""
    mode, k, r = {"knn": (NR.KNN, 20, 0.0), "hybrid": (NR.HYBRID, 20, 0.5), "radius": (NR.RADIUS, 0, 0.5)}[search]
    pts, lab, names = NR.crafted_cloud(with_cut=mode != NR.KNN)
    nb = NR.neighbours(pts, mode, k, r)
    assert not nb.alt and ((lab[np.maximum(nb.idx, 0)] == lab[:, None]) | (nb.idx < 0)).all() and (nb.count == np.bincount(lab)[lab]).all()
    prior = NR.fixed_prior(len(pts), 9)
    _public_rows(P, knn_form, pts, nb, mode, k, r, prior, f"crafted {search}")
    if mode == NR.KNN:
        for wave in (0, 1):
            knn_form(wave, 3)
            pc = P.PointCloud(pts); pc.estimate_normals(_param(P, mode, k, r))
            pv = P.PointCloud(pts); pv.estimate_covariances(_param(P, mode, k, r))
            nrm, cov = _bits(pc.normals.astype(np.float32)), _bits(pv.covariances.astype(np.float32).reshape(-1, 9))
            for c in np.unique(lab):
                rows = np.nonzero(lab == c)[0]
                assert (nrm[rows] == nrm[rows[0]]).all() and (cov[rows] == cov[rows[0]]).all(), (names[c], wave, pc.normals[rows][:3])


def test_crafted_clusters_as_a_scale_cloud(P, oracle):
    """The crafted cloud through the scale-cloud preparation at voxel sizes that keep every point but the coincident ones (which share a voxel):
    counts, points and every normal, in all three forms."""
    pts, lab, names = NR.crafted_cloud()
    voxels = (1e-3, 5e-4)
    prior = NR.fixed_prior(len(pts), 9)
    # (20, 1.0, 20): the filter removes exactly the clusters of fewer than 20 points (mean distance to 20 neighbours ~9 m against <= 0.1 m), so
    # that the 20 nearest kept points of every kept point are again its own cluster
    out = [P._lib.debug_scale_clouds([pts, pts], [prior, None], voxels, 20, 1.0, 20, form) for form in (0, 1, 2)]
    assert out[0] is not None
    coincident = sum(NR.CLUSTER - 1 for nm in names if nm == "coincident")
    full = sum(NR.CLUSTER for nm in names if not nm.startswith(("cut", "coincident")))
    for c, pr in enumerate((prior, None)):
        for s, voxel in enumerate(voxels):
            sc = NR.scale_cloud_reference(oracle, pts, pr, voxel, 20, 1.0)
            assert sc["n_voxel"] == len(pts) - coincident and sc["n_clean"] == full
            nb = NR.neighbours(sc["points"], NR.KNN, 20)
            assert not nb.alt and (nb.kth_d2 <= 0.01).all() and (nb.next_d2 > 25.0).all()
            _check_cloud(out[0][c][s], sc, nb, f"crafted scale cloud {c} voxel {voxel}")
            for form in (1, 2):
                if out[form] is not None:
                    assert np.array_equal(_bits(out[form][c][s][0]), _bits(out[0][c][s][0])) and np.array_equal(_bits(out[form][c][s][1]), _bits(out[0][c][s][1])), (form, c, s)
