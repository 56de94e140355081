"""The two bodies of the normals-from-lists kernel (pcr_set_option "nfl_form": 0 the octet rounds, 1 one point per lane, the default) give the
same bits.

The kernel turns the outlier filter's k-best lists into the normals of the cleaned cloud: per kept point the survivors of its list, the farthest
of them dropped until normal_k remain, their raw moments in a fixed summation tree, the eigen solver.  The lane form keeps the sets (the drop
order of equal distances included) and the summation tree of the octet form, so for both values of the option and through all three forms of
the preparation (pcr_debug_scale_clouds: 0 scale by scale, 1 a cloud's scales batched, 2 all clouds and scales as one batch) the returned points,
every normal (compared as uint32), n_voxel, the clean counts and the `untouched` flag must be equal.  On the crafted clouds the normals of the
lane form are also held against tests/normal_reference.py, row by row, with the cleaned cloud the device returned as the cloud: agreement of the
two forms is then not agreement on a shared error.

Shapes are the smallest that can still go wrong: the golden pair at the product's (30, 1.0, 20) and at (30, 0.5, 30) (nothing to drop, many
fallback rows); a 12 x 12 unit lattice whose float32 distances are exact and tie eight at a time at the drop threshold; clouds of 1 ... 129 points
around the lane (64) and piece (8) boundaries with lists that are not full; a group of two pairs of four different sizes."""
import numpy as np
import pytest

import normal_reference as NR
from conftest import pkg

pytestmark = pytest.mark.gpu

VOXELS = (0.5, 0.3)
FORMS = (0, 1, 2)


@pytest.fixture(scope="module")
def P():
    return pkg()


@pytest.fixture
def nfl_form(P):
    yield lambda form: P._lib.set_option("nfl_form", form)
    P._lib.set_option("nfl_form", 1)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _all_forms(P, nfl_form, clouds, priors, voxels, params, forms=FORMS):
    """out[nfl][form] of pcr_debug_scale_clouds for nfl_form 0 and 1; every (nfl, form) must serve the inputs."""
    sor_k, std, normal_k = params
    out = {}
    for nfl in (0, 1):
        nfl_form(nfl)
        out[nfl] = {form: P._lib.debug_scale_clouds(clouds, priors, voxels, sor_k, std, normal_k, form) for form in forms}
        assert all(o is not None for o in out[nfl].values()), (nfl, params)
    return out


def _assert_same(out, n_clouds, n_scales, what):
    """Every (nfl_form, preparation form) against (0, first form): points, normals (uint32, every row), n_voxel, clean count, untouched."""
    forms = sorted(out[0])
    base = out[0][forms[0]]
    for nfl in (0, 1):
        for form in forms:
            for c in range(n_clouds):
                for s in range(n_scales):
                    a, b = out[nfl][form][c][s], base[c][s]
                    tag = f"{what}: nfl_form {nfl} form {form} against nfl_form 0 form {forms[0]}, cloud {c} scale {s}"
                    assert a[3] and b[3], tag                                                  # untouched past the clean count
                    assert a[2] == b[2] and len(a[0]) == len(b[0]) and a[1].shape == b[1].shape, (tag, a[2], b[2], len(a[0]), len(b[0]))
                    assert np.array_equal(_bits(a[0]), _bits(b[0])), tag + ": points"
                    differ = np.nonzero((_bits(a[1]) != _bits(b[1])).any(1))[0]
                    assert not len(differ), f"{tag}: {len(differ)} of {len(a[1])} normals differ, first rows {differ[:5]}: {a[1][differ[:2]]} / {b[1][differ[:2]]}"


def _explained(dev, raw, prior, normal_k, what):
    """The normals of one device scale cloud against the reference, with the cleaned cloud the device returned as the cloud (one point per voxel:
    a returned row is a row of `raw`, and its prior is that row's)."""
    pts, nrm = dev[0], dev[1]
    if not len(pts):
        return
    pr = None
    if prior is not None:
        key = {r.tobytes(): i for i, r in enumerate(_bits(raw))}
        pr = prior[[key[r.tobytes()] for r in _bits(pts)]]
    NR.assert_normals_explained(pts, nrm, NR.neighbours(pts, NR.KNN, normal_k), prior=pr, what=what)


# ------------------------------------------------------------------------------------------------------------------------ golden pair
@pytest.mark.parametrize("params", [(30, 1.0, 20), (30, 0.5, 30)], ids=lambda p: "sor%d_%g_k%d" % p)
@pytest.mark.parametrize("with_prior", [False, True], ids=["noprior", "prior"])
def test_golden_pair(P, nfl_form, small_pair, with_prior, params):
    clouds = [small_pair[w].astype(np.float32) for w in ("source", "target")]
    priors = [NR.fixed_prior(len(clouds[0]), 5), NR.fixed_prior(len(clouds[1]), 6)] if with_prior else None
    out = _all_forms(P, nfl_form, clouds, priors, VOXELS, params)
    _assert_same(out, 2, len(VOXELS), f"pair 899 {params} prior {with_prior}")


# ---------------------------------------------------------------------------------------------------------------------------- lattice
LATTICE_PARAMS = (29, 0.5, 20)       # 29: the lists of the inner points end between d^2 = 9 and 10 (1 + 4 + 4 + 4 + 8 + 4 + 4 = 29 points up to 9)
LATTICE_VOXELS = (0.5, 0.25)         # spacing 1.0: every voxel holds one point at both sizes


def _lattice():
    g = np.arange(12, dtype=np.float32)
    plane = np.stack([np.repeat(g, 12), np.tile(g, 12), np.zeros(144, np.float32)], 1)
    rng = np.random.default_rng(11)
    far = np.concatenate([5.5 + rng.standard_normal((6, 2)), rng.uniform(8.0, 15.0, (6, 1)) * rng.choice([-1.0, 1.0], (6, 1))], 1)      # above / below the middle
    pts = np.concatenate([plane, far.astype(np.float32)]).astype(np.float32)
    return pts[np.random.default_rng(12).permutation(len(pts))]


def _lattice_facts(oracle, pts):
    """From numpy and the CPU oracle alone: (rows with more than one survivor at their drop threshold, kept rows whose list holds a removed row)."""
    sor_k, std, normal_k = LATTICE_PARAMS
    keep = np.asarray(oracle.remove_statistical_outlier(pts, sor_k, std)[0], bool)
    p = pts.astype(np.float64)
    d2 = ((p[:, None, :] - p[None, :, :]) ** 2).sum(2)                      # integers and sums of few float32 squares: exact
    o = np.argsort(d2, axis=1, kind="stable")
    sd = np.take_along_axis(d2, o, 1)
    tied, short = 0, 0
    for i in np.nonzero(keep)[0]:
        if sd[i, sor_k - 1] == sd[i, sor_k]:
            continue                                                        # which points the list holds is the search's choice: not used
        members = o[i, :sor_k]
        surv = members[keep[members]]
        short += len(surv) < sor_k
        excess = len(surv) - normal_k
        if excess > 0:
            ds = np.sort(d2[i, surv])[::-1]
            tied += int((ds == ds[excess - 1]).sum() > 1)
    return tied, short, keep


def test_lattice_with_ties(P, nfl_form, oracle):
    pts = _lattice()
    tied, short, keep = _lattice_facts(oracle, pts)
    print(f"lattice: {int(keep.sum())} of {len(pts)} rows kept; {tied} rows tie at their drop threshold, {short} kept rows list a removed row")
    assert tied >= 1 and short >= 1 and not keep.all()
    prior = NR.fixed_prior(len(pts), 13)
    out = _all_forms(P, nfl_form, [pts, pts], [prior, None], LATTICE_VOXELS, LATTICE_PARAMS)
    _assert_same(out, 2, len(LATTICE_VOXELS), "lattice")
    for c, pr in enumerate((prior, None)):
        for s in range(len(LATTICE_VOXELS)):
            _explained(out[1][2][c][s], pts, pr, LATTICE_PARAMS[2], f"lattice cloud {c} scale {s}")


# ------------------------------------------------------------------------------------------------------------------------------ sizes
SIZES = (1, 2, 3, 7, 8, 9, 31, 33, 63, 64, 65, 129)
SIZE_PARAMS = (30, 1.0, 20)


def _separated(n, seed):
    """n random points on distinct cells of a lattice of spacing 1 (jittered by +-0.2: every spacing is above 0.6), float32."""
    rng = np.random.default_rng(seed)
    cells = rng.permutation(8 * 8 * 8)[:n]
    base = np.stack([cells % 8, (cells // 8) % 8, cells // 64], 1).astype(np.float64)
    return (base + rng.uniform(-0.2, 0.2, (n, 3)) + (40.0, -30.0, 5.0)).astype(np.float32)


def test_sizes_around_the_lane_and_piece_boundaries(P, nfl_form):
    voxels = (0.25, 0.125)                                                  # below the smallest spacing: one point per voxel
    clouds = [_separated(n, 100 + n) for n in SIZES]
    for c in clouds:
        d = np.linalg.norm(c[:, None, :].astype(np.float64) - c[None, :, :], axis=2) + np.eye(len(c)) * 9.0
        assert d.min() > 0.55
    priors = [NR.fixed_prior(len(c), 200 + len(c)) if k % 3 else None for k, c in enumerate(clouds)]
    out = _all_forms(P, nfl_form, clouds, priors, voxels, SIZE_PARAMS)
    _assert_same(out, len(clouds), len(voxels), f"sizes {SIZES}")
    for c, cloud in enumerate(clouds):
        for s in range(len(voxels)):
            assert out[1][2][c][s][2] == len(cloud)                         # every point is a voxel
            _explained(out[1][2][c][s], cloud, priors[c], SIZE_PARAMS[2], f"{len(cloud)} points scale {s}")


# -------------------------------------------------------------------------------------------------------------------- two-pair group
def test_two_pair_group(P, nfl_form, small_pair):
    """Four clouds of different sizes as one group batch (form 2) under both bodies, and cloud by cloud (form 1): the per-problem todo_count and
    piece_count reach their own problems."""
    src, tgt = small_pair["source"].astype(np.float32), small_pair["target"].astype(np.float32)
    clouds = [src, tgt[:11000], src[2500:14001], tgt]
    priors = [NR.fixed_prior(len(clouds[0]), 21), None, None, NR.fixed_prior(len(clouds[3]), 24)]
    assert len({len(c) for c in clouds}) == 4
    out = _all_forms(P, nfl_form, clouds, priors, VOXELS, (30, 1.0, 20), forms=(2, 1))
    _assert_same(out, 4, len(VOXELS), "two-pair group")
