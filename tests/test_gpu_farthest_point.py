"""Farthest point sampling on the device against the restatement of the rule of include/pcr_hip.h (farthest_point_reference.py) on the same
float32 points.  The answer is one sequential loop's, so every comparison is equality: the index list, the final distances as uint64 and the
cover distance; there is no tolerance in this file.  Both forms of the loop are forced through the options ``fps_form`` / ``fps_wgs`` /
``fps_timeout`` and every test restores them.

Inputs: every second source point of golden pair 899 (8,263 points: more than one workgroup's LDS holds, so ``fps_wgs`` 1 also walks rows kept in
global memory); the 6 x 6 x 6 lattice, whose 96 tie steps fall across lanes, wavefronts and workgroups; duplicates; sizes around the wavefront and
workgroup widths; rows with non-finite coordinates."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN, pkg
from farthest_point_reference import farthest_point_reference, lattice

pytestmark = pytest.mark.gpu

OK, EINVAL = 0, -1
STEP, PERSIST = 0, 1


@pytest.fixture(scope="module")
def P():
    return pkg()


@pytest.fixture()
def force(P):
    """force(form, wgs=0, timeout=-1) selects the form of the calls of one test; the defaults come back afterwards"""
    def set_(form, wgs=0, timeout=-1):
        P._lib.set_option("fps_form", form); P._lib.set_option("fps_wgs", wgs); P._lib.set_option("fps_timeout", timeout)
    yield set_
    set_(-1, 0, -1)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "nclt_pair_899.npz"))["source"][::2]


@pytest.fixture(scope="module")
def golden_ref(golden):
    return farthest_point_reference(golden, 512, 0)


def _raw(P, pts, k, start, index=True, dist=True, info=True, xyz=True, n=None):
    """pcr_farthest_point_sample itself -> (status, message, sel (k,), dist (n,), info); a False switch passes a null pointer"""
    import torch
    ctx = P._lib.Context.current()
    pts = np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 3)
    rows = len(pts)
    d = torch.from_numpy(pts).cuda()
    sel = torch.full((max(k, 1),), -7, dtype=torch.int64, device="cuda")
    d2 = torch.full((max(rows, 1),), -7.0, dtype=torch.float64, device="cuda")
    inf = P._lib.PcrFpsInfo(-7, -7, -7, -7.0)
    rc = ctx.lib.pcr_farthest_point_sample(ctx.handle, C.c_void_p(d.data_ptr()) if xyz and rows else None, C.c_int64(rows if n is None else n), C.c_int64(k),
                                           C.c_int64(start), C.c_void_p(sel.data_ptr()) if index else None, C.c_void_p(d2.data_ptr()) if dist else None,
                                           C.byref(inf) if info else None)
    msg = ctx.lib.pcr_last_error(ctx.handle)
    return rc, (msg.decode() if msg else ""), sel[:max(k, 0)].cpu().numpy(), d2[:rows].cpu().numpy(), inf


def _assert_equal(P, pts, k, start, ref, what, form, wgs=None):
    rc, msg, sel, d2, info = _raw(P, pts, k, start)
    assert rc == OK, (what, rc, msg)
    print(f"{what}: n = {len(pts)}, K = {k}, start {start}: form {info.form}, {info.workgroups} workgroups, fell back {info.fell_back}; "
          f"{int((sel != ref['sel']).sum())} other indices, {int((d2.view(np.uint64) != ref['dist'].view(np.uint64)).sum())} distances with other bits, "
          f"cover {info.cover_dist2!r} against {ref['cover_dist2']!r}")
    assert info.form == form and info.fell_back == 0, (what, info.form, info.fell_back)
    if wgs is not None:
        assert info.workgroups == wgs, (what, info.workgroups)
    assert sel.dtype == np.int64 and np.array_equal(sel, ref["sel"]), what
    assert np.array_equal(d2.view(np.uint64), ref["dist"].view(np.uint64)), what          # bit for bit
    assert np.float64(info.cover_dist2).view(np.uint64) == np.float64(ref["cover_dist2"]).view(np.uint64), what
    return info


@pytest.mark.parametrize("form,wgs", [(STEP, 0), (PERSIST, 1), (PERSIST, 2), (PERSIST, 7)])
def test_golden_cloud(P, force, golden, golden_ref, form, wgs):
    force(form, wgs)
    info = _assert_equal(P, golden, 512, 0, golden_ref, f"golden form {form} wgs {wgs}", form, wgs if form == PERSIST else 9)      # step form: 1024 rows per workgroup
    assert np.sqrt(info.cover_dist2) == 1.5150902351744047


@pytest.mark.parametrize("form,wgs", [(PERSIST, 1), (PERSIST, 3), (STEP, 0)])
def test_lattice_ties(P, force, form, wgs):
    """96 of the 100 steps have their maximum on several rows: the smallest index must win among lanes, wavefronts and workgroups"""
    pts = lattice(6)
    ref = farthest_point_reference(pts, 100, 0)
    assert ref["tie_steps"] == 96
    force(form, wgs)
    _assert_equal(P, pts, 100, 0, ref, f"lattice form {form} wgs {wgs}", form)


@pytest.mark.parametrize("form,wgs", [(STEP, 0), (PERSIST, 1), (PERSIST, 3)])
def test_duplicates_repeat_the_last_index(P, force, form, wgs):
    force(form, wgs)
    same = np.full((5, 3), 0.25, np.float32)
    ref = farthest_point_reference(same, 3, 2)
    assert ref["sel"].tolist() == [2, 2, 2]
    _assert_equal(P, same, 3, 2, ref, "five copies", form)
    two = np.array([[0, 0, 0]] * 3 + [[1, 1, 1]] * 3, dtype=np.float32)
    ref = farthest_point_reference(two, 5, 1)
    assert ref["sel"].tolist() == [1, 3, 3, 3, 3]
    _assert_equal(P, two, 5, 1, ref, "two triples", form)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 513, 1025])
def test_sizes(P, force, n):
    pts = np.random.default_rng(100 + n).uniform(-4, 4, (n, 3)).astype(np.float32)
    k, start = min(n, 40), n - 1 - (n // 7)                             # a start index in the last of three slices
    ref = farthest_point_reference(pts, k, start)
    for form, wgs in ((STEP, 0), (PERSIST, 1), (PERSIST, 3)):
        force(form, wgs)
        _assert_equal(P, pts, k, start, ref, f"n {n} form {form} wgs {wgs}", form)


def test_non_finite_rows(P, force):
    pts = np.random.default_rng(9).uniform(-2, 2, (200, 3)).astype(np.float32)
    bad = [0, 77, 199]
    pts[bad] = [[np.nan, 0, 0], [1, np.inf, 0], [0.5, -np.inf, np.nan]]
    ref = farthest_point_reference(pts, 120, 5)
    for form, wgs in ((STEP, 0), (PERSIST, 1), (PERSIST, 3)):
        force(form, wgs)
        rc, msg, sel, d2, info = _raw(P, pts, 120, 5)
        assert rc == OK and info.form == form, (rc, msg)
        assert not np.isin(bad, sel).any() and (d2[bad] == -1.0).all()
        assert np.array_equal(sel, ref["sel"]) and np.array_equal(d2.view(np.uint64), ref["dist"].view(np.uint64))
        assert np.float64(info.cover_dist2).view(np.uint64) == np.float64(ref["cover_dist2"]).view(np.uint64)
        for s in bad:
            rc, msg, *_ = _raw(P, pts, 10, s)
            assert rc == EINVAL and "farthest_point_down_sample" in msg and "non-finite" in msg, (form, s, rc, msg)


def test_fall_back_gives_the_same_answer(P, force, golden):
    """a wait of 0 ticks at the barrier: a workgroup that finds another not yet arrived gives up, every wave reaches an exit, and the host redoes
    the call launch by launch.  Run once; whether the fall-back happens depends on the arrival times, so either outcome must be consistent."""
    ref = farthest_point_reference(golden, 64, 0)
    force(STEP)
    _assert_equal(P, golden, 64, 0, ref, "step form", STEP)
    force(PERSIST, 8, 0)
    rc, msg, sel, d2, info = _raw(P, golden, 64, 0)
    print(f"fall-back: form {info.form}, {info.workgroups} workgroups, fell back {info.fell_back}")
    assert rc == OK, (rc, msg)
    assert (info.form, info.fell_back) in ((STEP, 1), (PERSIST, 0))
    assert info.workgroups == (8 if info.form == PERSIST else 9)
    assert np.array_equal(sel, ref["sel"]) and np.array_equal(d2.view(np.uint64), ref["dist"].view(np.uint64))
    assert np.float64(info.cover_dist2).view(np.uint64) == np.float64(ref["cover_dist2"]).view(np.uint64)


def test_errors_and_edges(P, force, golden):
    pts = golden[:300]
    for form in (STEP, PERSIST):
        force(form)
        # K = 0: nothing is written, whatever else is passed
        for kw in ({}, dict(index=False, dist=False, info=False), dict(start=-5), dict(start=10 ** 6)):
            start = kw.pop("start", 0)
            rc, msg, sel, d2, info = _raw(P, pts, 0, start, **kw)
            assert rc == OK and (d2 == -7.0).all(), (kw, rc, msg)
        rc, msg, sel, d2, info = _raw(P, np.zeros((0, 3), np.float32), 0, 0)          # an empty cloud
        assert rc == OK
        # K = n: every row once, and every distance 0
        ref = farthest_point_reference(pts, 300, 17)
        rc, msg, sel, d2, info = _raw(P, pts, 300, 17)
        assert rc == OK and np.array_equal(sel, ref["sel"]) and sorted(sel.tolist()) == list(range(300)) and (d2 == 0.0).all() and info.cover_dist2 == 0.0
        # optional outputs left out
        ref = farthest_point_reference(pts, 20, 3)
        for kw in (dict(dist=False), dict(info=False), dict(dist=False, info=False)):
            rc, msg, sel, d2, info = _raw(P, pts, 20, 3, **kw)
            assert rc == OK and np.array_equal(sel, ref["sel"]), (kw, rc, msg)
            assert (d2 == -7.0).all() if not kw.get("dist", True) else np.array_equal(d2.view(np.uint64), ref["dist"].view(np.uint64))
        for kw, k, start in ((dict(), 301, 0), (dict(), -1, 0), (dict(), 10, 300), (dict(), 10, -1), (dict(index=False), 10, 0), (dict(xyz=False), 10, 0),
                             (dict(xyz=False, index=False, dist=False, info=False), 10, 0), (dict(n=2 ** 31), 10, 0), (dict(n=-1), 0, 0)):
            rc, msg, sel, d2, info = _raw(P, pts, k, start, **kw)
            assert rc == EINVAL and "farthest_point_down_sample" in msg, (kw, k, start, rc, msg)
            assert (sel == -7).all() and (d2 == -7.0).all()


def test_python_layer(P, golden, golden_ref):
    import torch
    rng = np.random.default_rng(3)
    pc = P.PointCloud(golden)
    pc.normals = rng.normal(size=golden.shape).astype(np.float32)
    pc.colors = rng.uniform(0, 1, golden.shape).astype(np.float32)
    pc.estimate_covariances(P.KDTreeSearchParamKNN(10))
    idx, info = P.geometry._farthest_point_sample(pc, 512)
    assert isinstance(idx, torch.Tensor) and idx.is_cuda and idx.dtype == torch.int64 and np.array_equal(idx.cpu().numpy(), golden_ref["sel"])
    assert info["cover_radius"] == 1.5150902351744047 and info["cover_dist2"] == golden_ref["cover_dist2"] and info["form"] in (STEP, PERSIST)
    assert info["dist2"].is_cuda and np.array_equal(info["dist2"].cpu().numpy().view(np.uint64), golden_ref["dist"].view(np.uint64))
    again = P.farthest_point_indices(pc, 512)
    assert again.dtype == np.int64 and np.array_equal(again, golden_ref["sel"])                     # two runs give the same indices
    down = pc.farthest_point_down_sample(512)
    sel = golden_ref["sel"]
    assert len(down) == 512 and np.array_equal(np.asarray(down.points, np.float32), golden[sel])    # selection order
    for attr in ("normals", "colors", "covariances"):
        assert np.array_equal(np.asarray(getattr(down, attr)), np.asarray(getattr(pc, attr))[sel]), attr
    started = pc.farthest_point_down_sample(num_samples=30, start_index=4000)
    assert np.array_equal(np.asarray(started.points, np.float32), golden[farthest_point_reference(golden, 30, 4000)["sel"]])
    assert len(pc.farthest_point_down_sample(0)) == 0
    whole = pc.farthest_point_down_sample(len(pc), 5)
    assert np.array_equal(np.asarray(whole.points, np.float32), golden) and np.array_equal(np.asarray(whole.normals), np.asarray(pc.normals))
    assert whole._xyz.data_ptr() != pc._xyz.data_ptr()                                               # a copy
    for args in ((len(pc) + 1,), (-1,), (10, len(pc)), (10, -1)):
        with pytest.raises(RuntimeError, match="farthest_point_down_sample"):
            pc.farthest_point_down_sample(*args)
    # the budget of feature rows of a global registration
    small = P.PointCloud(golden[:2000])
    small.estimate_normals(P.KDTreeSearchParamHybrid(1.0, 20))
    feat = P.registration.compute_fpfh_feature(small, P.KDTreeSearchParamHybrid(2.5, 100))
    rows = feat.select_by_index(P.farthest_point_indices(small, 256))
    assert rows.num() == 256 and rows.dimension() == 33
