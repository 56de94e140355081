"""FPFH rows of the device against the numpy float64 restatement (fpfh_reference.py, itself checked against the oracle on these very inputs in
test_fpfh_reference.py), on the clouds of fpfh_cases.py: both search kinds, max_nn below and above the ball's and the cloud's size, clouds
smaller than a workgroup, the three regimes of the float64 queue, coincident points, normals that are not unit normals.

Every case runs compute_fpfh_feature in four forms of the SPFH pass (option "spfh_float64": 1 = all float64, 4 = float pass + float64 queue,
3 = a 16-entry queue, which overflows, 0 = the product's choice) and asserts
  * between forms: the same bits;
  * against the restatement, on rows where neither the row nor a row of its list is `touched` or `list_open`: every entry within one
    float32 ulp of float32(reference) and at least 99.9 % of the entries equal to it.  (The float64 values differ by less than 1e-12 relative -- sums of at most 200 positive terms,
    no cancellation -- so their float32 roundings differ by at most one ulp, and only where the value lies within 1e-12 relative of a rounding
    boundary: an expected share of 2e-5 of the entries.)
  * rows with neighbours: each of the three histograms sums to 200 within 2e-3 (to 100 where every neighbour is a copy of the point: no
    weighted sum); rows without: exactly zero -- excluded rows included."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fpfh_cases as fc
from conftest import pkg

pytestmark = pytest.mark.gpu

FORMS = (1, 4, 3, 0)


@pytest.fixture(scope="module")
def P():
    return pkg()


def _param(P, spec):
    return P.KDTreeSearchParamKNN(spec[1]) if spec[0] == "knn" else P.KDTreeSearchParamHybrid(spec[1], spec[2])


def _rows(P, pts, nrm, spec, form):
    """(n, 33) float32 of the device under "spfh_float64" = form."""
    from importlib import import_module
    lib = import_module(P.__name__ + "._lib")
    pc = P.PointCloud(pts.copy())                  # (the shared arrays are read-only)
    pc.normals = nrm.copy()
    lib.set_option("spfh_float64", form)
    try:
        return P.registration.compute_fpfh_feature(pc, _param(P, spec))._dev.cpu().numpy().copy()
    finally:
        lib.set_option("spfh_float64", 0)


def _check(P, name, spec, forms=FORMS):
    pts, nrm, idx, ref, excluded, cap = fc.reference(name, spec)
    got = {form: _rows(P, pts, nrm, spec, form) for form in forms}
    first = got[forms[0]]
    assert first.shape == (len(pts), 33) and first.dtype == np.float32
    for form in forms[1:]:
        assert np.array_equal(got[form], first), (name, spec, form, int((got[form] != first).any(1).sum()))
    # every row: the sums, or exactly zero.  (A row all of whose neighbours are copies of its point has no weighted sum: its own SPFH alone, 100.)
    has = ref["m"] > 0
    assert (first[~has] == 0.0).all(), (name, spec)
    blocks = first.astype(np.float64).reshape(-1, 3, 11).sum(2)
    apart = ((idx >= 0) & (pts[np.where(idx >= 0, idx, 0)] != pts[:, None, :]).any(2)).any(1)
    assert np.allclose(blocks[has & apart], 200.0, atol=2e-3), (name, spec, float(np.abs(blocks[has & apart] - 200.0).max(initial=0.0)))
    assert np.allclose(blocks[has & ~apart], 100.0, atol=1e-3), (name, spec)
    # rows the reference fixes
    good = ~excluded
    assert (~good).mean() <= cap, (name, spec, int((~good).sum()))
    want = ref["fpfh"].astype(np.float32)
    ulps = np.abs(first[good].view(np.int32).astype(np.int64) - want[good].view(np.int32).astype(np.int64))
    equal = float((ulps == 0).mean()) if ulps.size else 1.0
    print(f"{name} {spec}: {int(good.sum())} of {len(pts)} rows compared, {int((ulps > 1).sum())} entries off by more than an ulp in {int((ulps > 1).any(1).sum())} rows, "
          f"{equal:.6f} equal")
    assert (ulps <= 1).all(), (name, spec, int((ulps > 1).any(1).sum()), np.nonzero(good)[0][(ulps > 1).any(1)][:8].tolist())
    assert equal >= 0.999, (name, spec, equal)
    return first


@pytest.mark.parametrize("spec", fc.SHEET_SPECS, ids=fc.spec_id)
def test_random_sheet(P, spec):
    """Balls under-full and over-full (Hybrid(r, 50): both kinds of row, asserted in test_fpfh_reference.py), the k nearest of the KNN kernel, lists of
    the point alone (all-zero rows).  The float pass queues a few pairs per workgroup here: the first regime of the queue."""
    rows = _check(P, "sheet", spec)
    if spec[-1] == 1:
        assert (rows == 0.0).all()
    if spec == ("hybrid", fc.SHEET_R, 50):
        m = fc.reference("sheet", spec)[3]["m"]
        assert (m == 49).sum() > 100 and (m < 49).sum() > 100       # lists cut at max_nn, and whole balls


@pytest.mark.parametrize("n", fc.SMALL_SIZES)
def test_small_clouds(P, n):
    """Clouds of less than a workgroup's 32 points, of one more, of a few workgroups with a partial last one; n < k for most: rows shorter than the
    8 slots of a point's lanes, lists padded with -1."""
    for spec in fc.SMALL_SPECS:
        _check(P, f"small{n}", spec)


def test_one_bin_at_capacity(P):
    """All 199 votes of a point in one bin of each histogram: a byte counter holds 199."""
    rows = _check(P, "flat", ("knn", 200), forms=(1, 4))
    assert (rows[:, [5, 16, 27]] > 100.0).all()


@pytest.mark.parametrize("name", ["needle8", "needle10"])
def test_queue_regimes(P, name):
    """Needle clouds (fpfh_cases.needles): inside a stack dp x n is exactly zero, float64 votes in the bins of f = 0 and the float form declines.
    needle8: 7 declined pairs per point, 224 in a full workgroup -- over the 192 places of its LDS list, so entries go straight to the global queue --
    and 7 n in all, under the queue's 8 n.  needle10: 9 n, over it: the queue is dropped and every row redone in float64.
    Measured on an MI355X (tools/fpfh_queue_count.py; asserted in test_needle_clouds_reach_their_regimes):
        needle8   1000 points, 7042 pairs queued, capacity 8000
        needle10  1000 points, 9120 pairs queued, capacity 8000 (over: every row redone)"""
    _check(P, name, fc.NEEDLE_SPEC)


def test_needle_clouds_reach_their_regimes():
    """The counts the float pass prints under PCR_DEBUG_FGR, in a child process: a construction that stops reaching its regime fails here."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "fpfh_queue_count.py"), "sheet", "needle8", "needle10"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    q = {l.split()[1]: tuple(int(v) for v in l.split()[2:]) for l in out.stdout.splitlines() if l.startswith("QUEUE ")}
    print(q)
    n, queued, cap = q["sheet"]
    assert 0 < queued < 192 * (n // 32) and queued <= cap              # a few per workgroup
    n, queued, cap = q["needle8"]
    assert 7 * n <= queued <= cap, q
    n, queued, cap = q["needle10"]
    assert queued >= 9 * n and queued > cap, q


@pytest.mark.parametrize("spec", fc.CASES["copies"][1] + fc.CASES["places"][1], ids=fc.spec_id)
def test_coincident_points(P, spec):
    """Exact duplicates: a pair at distance 0 votes in the bins of f = 0 and has no weight in the sum."""
    _check(P, "copies" if spec in fc.CASES["copies"][1] else "places", spec)


@pytest.mark.parametrize("spec", fc.CASES["overk"][1], ids=fc.spec_id)
def test_more_copies_than_the_list_is_long(P, spec):
    """Six copies of a point under k = 3: whichever copies a list holds -- the point itself among them or not -- all its pairs are at distance 0, and
    the row is 100 in the f = 0 bin of each histogram, as Open3D's (test_fpfh_reference.py::test_copies_over_k_rows)."""
    rows = _check(P, "overk", spec)
    want = np.zeros(33, np.float32); want[[5, 16, 27]] = 100.0
    assert (rows[:6] == want).all(), rows[:6]


@pytest.mark.parametrize("kind", fc.NORMAL_KINDS)
def test_normals_that_are_not_unit_normals(P, kind):
    """pcr_import_cloud does not normalise, Open3D's FPFH neither.  With a normal longer than 1 an |angle| exceeds 1, float64's acos is NaN and the
    frame stays with the first point; the float form must not answer such a pair from fa1 < fa2.  The float64 form matches the restatement (and so
    the oracle), the float pass gives the same bits, and form 2 -- float64 plus a comparison with the float form wherever that answers -- finds no
    pair whose bins differ (it raises if it does)."""
    name = "normals_" + kind
    _check(P, name, fc.NORMALS_SPEC)
    pts, nrm = fc.cloud(name)
    _rows(P, pts, nrm, fc.NORMALS_SPEC, 2)
