"""The yardstick of test_gpu_fpfh_rows.py, checked on the CPU: the numpy float64 restatement of FPFH (fpfh_reference.py) against the C oracle
(oracle/fpfh.c, a kd-tree and a loop per point) on the same inputs -- every test cloud of fpfh_cases.py and a decimated golden cloud, both
search kinds.  On rows that are not excluded (neither they nor a neighbour `touched` or `list_open`) the two agree to 1e-12 relative: float64 sums of at most 200 positive
terms in another order (the oracle adds inc vote by vote, the restatement multiplies the count).  And every input meets its cap on excluded
rows here, by the reference alone, so that a failure on the device is never the input's fault."""
import os

import numpy as np
import pytest

import fpfh_cases as fc
import fpfh_reference as fr
from conftest import GOLDEN


def _oracle_rows(oracle, pts, nrm, spec):
    if spec[0] == "knn":
        return oracle.compute_fpfh(pts, nrm, oracle.SEARCH_KNN, spec[1], 0.0)
    return oracle.compute_fpfh(pts, nrm, oracle.SEARCH_HYBRID, spec[2], spec[1])


def _assert_rows(ref, excluded, rows, what):
    good = ~excluded
    want = ref["fpfh"]
    err = np.abs(rows - want)[good]
    assert (err <= 1e-12 * np.abs(want[good])).all(), (what, float((err / np.maximum(np.abs(want[good]), 1e-300)).max(initial=0.0)))
    assert (rows[ref["m"] == 0] == 0.0).all(), what


@pytest.mark.parametrize("name,spec", fc.case_ids(), ids=fc.spec_id)
def test_restatement_matches_oracle_and_input_meets_its_cap(oracle, name, spec):
    pts, nrm, idx, ref, excluded, cap = fc.reference(name, spec)
    print(f"{name} {spec}: {len(pts)} points, {int(ref['undecided'].sum())} undecided pairs, {int(ref['touched'].sum())} rows touched, {int(excluded.sum())} rows excluded")
    assert excluded.mean() <= cap, (name, spec, int(excluded.sum()), len(pts))
    assert (ref["counts"].reshape(-1, 3, 11).sum(2) == ref["m"][:, None]).all()
    _assert_rows(ref, excluded, _oracle_rows(oracle, pts, nrm, spec), (name, spec))


def test_cases_reach_what_they_are_built_for():
    """Properties of the inputs that the device tests lean on."""
    # Hybrid(r, 50) on the sheet: balls that hold fewer than 50 points and balls that hold more
    _, _, over = fr.hybrid_lists(fc.cloud("sheet")[0], fc.SHEET_R, 50)
    assert over.sum() > 100 and (~over).sum() > 100, (int(over.sum()), int((~over).sum()))
    # KNN(1) and max_nn = 1: the point itself is the whole list
    for spec in (("knn", 1), ("hybrid", fc.SHEET_R, 1)):
        ref = fc.reference("sheet", spec)[3]
        assert (ref["m"] == 0).all() and (ref["fpfh"] == 0.0).all()
    # the flat patch: 199 votes in one bin of each histogram
    ref = fc.reference("flat", ("knn", 200))[3]
    assert (ref["counts"][:, [5, 16, 27]] == 199).all() and (ref["m"] == 199).all()
    # needle clouds: every pair inside a stack is degenerate (dp x n == 0) and decided -- height - 1 such pairs per point, more than the 192 places
    # of a workgroup's list in every full workgroup of 32 points; 7 n in all is under the queue's 8 n, 9 n is over
    for name, height in (("needle8", 8), ("needle10", 10)):
        pts, nrm, idx, ref, excluded, _ = fc.reference(name, fc.NEEDLE_SPEC)
        p = pts.astype(np.float64)
        j = np.where(idx >= 0, idx, 0)
        in_stack = (idx >= 0) & (p[j][:, :, 0] == p[:, None, 0]) & (p[j][:, :, 1] == p[:, None, 1])
        assert (in_stack.sum(1) == height - 1).all()
        assert not ref["undecided"].any() and not excluded.any()
        assert (ref["m"] > height - 1).mean() > 0.9                  # stacks have neighbours: pairs that the float form answers
    assert 32 * 7 > 192 and 7 * 1000 < 8 * 1000 < 9 * 1000
    # the copies: pairs at distance 0 in the lists
    pts, nrm, idx, ref, _, _ = fc.reference("copies", ("knn", 10))
    j = np.where(idx >= 0, idx, 0)
    assert ((idx >= 0) & (pts[j] == pts[:, None, :]).all(2)).sum() == 6
    # long normals: pairs with an |angle| above 1, by the thousand
    for kind, least in (("x1.05", 1000), ("x1.5", 10000), ("x100", 60000), ("mixed", 10000), ("x0.5", 0), ("voxel", 0)):
        pts, nrm, idx, ref, _, _ = fc.reference("normals_" + kind, fc.NORMALS_SPEC)
        i, s = np.nonzero(idx >= 0)
        j = idx[i, s]
        dp = pts[j].astype(np.float64) - pts[i].astype(np.float64)
        length = np.linalg.norm(dp, axis=1)
        over = (np.abs((nrm[i].astype(np.float64) * dp).sum(1)) > length) | (np.abs((nrm[j].astype(np.float64) * dp).sum(1)) > length)
        assert over.sum() >= least and (least > 0 or over.sum() == 0), (kind, int(over.sum()))


def test_copies_over_k_rows():
    """A point with more copies of itself than the list is long: whichever k of them a search lists, every pair is at distance 0 -- votes in the
    bins of f = 0, no weight in the sum -- so its row is 100 in bins 5, 16 and 27 (k >= 2)."""
    for spec in fc.CASES["overk"][1]:
        ref = fc.reference("overk", spec)[3]
        want = np.zeros(33); want[[5, 16, 27]] = 100.0
        assert (ref["fpfh"][:6] == want).all()


@pytest.mark.parametrize("spec", [("knn", 100), ("hybrid", 1.0, 200), ("hybrid", 1.0, 30)], ids=fc.spec_id)
def test_restatement_matches_oracle_on_a_golden_cloud(oracle, spec):
    """Every sixth point of a golden NCLT cloud with the normal it has in the whole cloud (the oracle's, float32 as a PointCloud holds them).  A
    scan of flat ground: hundreds of normals are (0, 0, +-1) to 1e-9 and pairs of them tie in acos|angle| within MARGIN, so many rows are
    `touched` here -- under KNN(100), whose lists reach far on a sparse cloud, three in four; some five hundred rows at least are compared."""
    full = np.load(os.path.join(GOLDEN, "nclt_pair_899.npz"))["source"].astype(np.float32)
    pts, nrm = full[::6].copy(), oracle.estimate_normals(full, oracle.SEARCH_HYBRID, 20, 0.2).astype(np.float32)[::6].copy()
    idx, is_open = fr.lists_for(pts, spec)
    ref = fr.fpfh(pts, nrm, idx)
    excluded = ref["touched"] | fr.spread(is_open, idx)
    print(f"golden {spec}: {len(pts)} points, {int((~excluded).sum())} rows compared")
    assert (~excluded).sum() >= 500
    _assert_rows(ref, excluded, _oracle_rows(oracle, pts, nrm, spec), spec)
