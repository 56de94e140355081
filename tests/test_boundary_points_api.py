"""CPU-side checks of the boundary point detector: ``pcr_boundary_points`` is declared in the header, exported by the built library and
carries a ctypes prototype that matches the declaration; the Python surface has the calls built on it with Open3D's defaults and refuses bad
arguments on the host; and three facts of the numpy restatement of the rule (tests/boundary_reference.py) on shapes whose boundary is known.
Needs no GPU."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import boundary_reference as bref
from conftest import ROOT, pkg

NAME = "pcr_boundary_points"
_CTYPE = {"int64_t": C.c_int64, "int": C.c_int, "double": C.c_double}
HOST_OUTPUTS = {"out_n": C.c_int64}          # typed pointers; every other pointer is passed as an address


def _declaration(hdr, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
    assert m, f"{name} is not declared in include/pcr_hip.h"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_entry_point_is_declared_exported_and_prototyped():
    P = pkg()
    hdr = open(os.path.join(ROOT, "include", "pcr_hip.h")).read()
    if not os.path.exists(P._lib.SO_PATH):
        P._lib.build()
    lib = P._lib.load()
    params = _declaration(hdr, NAME)
    assert [p.split()[-1].lstrip("*") for p in params] == ["ctx", "xyz", "normals", "n", "radius", "max_nn", "angle_threshold", "boundary_mask", "out_xyz",
                                                           "out_index", "out_n", "max_gap", "counts"]
    assert NAME in P._lib.EXPORTS
    assert hasattr(lib, NAME), f"{NAME} is not exported by libpcr_hip.so"
    fn = getattr(lib, NAME)
    assert fn.restype is C.c_int and fn.argtypes is not None, f"{NAME} has no prototype in _lib"
    assert len(fn.argtypes) == len(params), params
    for at, p in zip(fn.argtypes, params):
        arg = p.split()[-1].lstrip("*")
        if "*" in p:
            if arg in HOST_OUTPUTS:
                assert issubclass(at, C._Pointer) and at._type_ is HOST_OUTPUTS[arg], (p, at)
                assert _CTYPE[p.replace("const", "").split("*")[0].split()[-1]] is at._type_, (p, at)      # ... and the declared pointee
            else:
                assert at is C.c_void_p, (p, at)
        else:
            assert at is _CTYPE[p.split()[-2]], (p, at)
    # the rule and the two deviations are stated next to the entry point
    doc = hdr[:hdr.index("int " + NAME)].rsplit("/*", 1)[1]
    for word in ("ComputeBoundaryPoints", "BoundaryEstimation", "TWO DEVIATIONS", "GetCoordinateSystemOnPlane", "(d^2, caller index)", "atan2", "2.0 * M_PI",
                 "angle_threshold * M_PI / 180.0", "x before y before z", "PCR_EINVAL"):
        assert word in doc, word


def test_python_surface_and_defaults():
    P = pkg()
    g = P.geometry
    defaults = {"max_nn": 30, "angle_threshold": 90.0}
    for fn, first in ((g.PointCloud.compute_boundary_points, "self"), (g._boundary_points, "cloud"), (g.boundary_point_indices, "cloud"),
                      (P.functions.remove_boundary_points, "cloud")):
        sig = inspect.signature(fn).parameters
        assert list(sig)[:2] == [first, "radius"] and sig["radius"].default is inspect.Parameter.empty, fn
        assert {k: sig[k].default for k in list(sig)[2:]} == defaults, fn
    assert P.boundary_point_indices is g.boundary_point_indices and P.remove_boundary_points is P.functions.remove_boundary_points
    import pcr_amd
    assert pcr_amd.boundary_point_indices is g.boundary_point_indices and pcr_amd.remove_boundary_points is P.functions.remove_boundary_points
    assert P.o3d.geometry.PointCloud is g.PointCloud and callable(P.o3d.geometry.PointCloud.compute_boundary_points)


def test_unit_is_in_the_build_and_in_the_packed_fp32_scan():
    csrc = os.path.join(ROOT, "point-cloud-registration-with-global-refinement_amd", "csrc")
    assert os.path.exists(os.path.join(csrc, "pcr_boundary.hip"))
    assert re.search(r"^for f in .*\bpcr_boundary\b", open(os.path.join(csrc, "build.sh")).read(), re.M)
    assert '"pcr_boundary"' in open(os.path.join(ROOT, "tools", "pk_trans_scan.py")).read()


class _NoDevice:
    """stands in for the context class: any use of a device inside the block fails the test"""

    @classmethod
    def current(cls):
        raise AssertionError("a device context was asked for")


def _host_cloud(P, n=5, normals=True):
    """a cloud whose storage is host memory: enough for the checks that must come before any device work"""
    import torch
    pc = P.PointCloud()
    pc._xyz = torch.zeros((n, 3), dtype=torch.float32)
    if normals:
        pc._nrm = torch.zeros((n, 3), dtype=torch.float32)
    return pc


BAD = [dict(radius=0.0), dict(radius=-1.0), dict(radius=float("nan")), dict(radius=float("inf")), dict(max_nn=0), dict(max_nn=201), dict(max_nn=-3),
       dict(angle_threshold=-1.0), dict(angle_threshold=360.5), dict(angle_threshold=float("nan")), dict(angle_threshold=float("inf"))]


@pytest.mark.parametrize("bad", BAD, ids=[f"{k}={v}" for b in BAD for k, v in b.items()])
def test_bad_arguments_raise_value_error_before_a_device_is_touched(monkeypatch, bad):
    P = pkg()
    monkeypatch.setattr(P._lib, "Context", _NoDevice)
    args = dict(radius=1.0, max_nn=30, angle_threshold=90.0)
    args.update(bad)
    for cloud in (_host_cloud(P), _host_cloud(P, normals=False)):          # the arguments are looked at first
        for call in (cloud.compute_boundary_points, lambda **kw: P.geometry._boundary_points(cloud, **kw),
                     lambda **kw: P.boundary_point_indices(cloud, **kw), lambda **kw: P.remove_boundary_points(cloud, **kw)):
            with pytest.raises(ValueError, match="compute_boundary_points"):
                call(**args)


def test_a_cloud_without_normals_raises_before_a_device_is_touched(monkeypatch):
    P = pkg()
    monkeypatch.setattr(P._lib, "Context", _NoDevice)
    cloud = _host_cloud(P, normals=False)
    for call in (lambda: cloud.compute_boundary_points(1.0), lambda: P.geometry._boundary_points(cloud, 1.0), lambda: P.boundary_point_indices(cloud, 1.0),
                 lambda: P.remove_boundary_points(cloud, 1.0)):
        with pytest.raises(RuntimeError, match="No normals"):              # PointCloud._need_normals
            call()
    # good arguments and normals: the next thing the call wants is the device
    with pytest.raises(AssertionError, match="device context"):
        _host_cloud(P).compute_boundary_points(1.0)


# ------------------------------------------------------------------------------------------ facts of the restatement
def test_restatement_on_a_grid():
    pts, nrm = bref.grid_cloud(32)
    at90 = bref.boundary(pts, nrm, 1.5, 30, 90.0)
    x, y = pts[:, 0], pts[:, 1]
    on_x, on_y = (x == 0) | (x == 31), (y == 0) | (y == 31)
    perimeter, corner = on_x | on_y, on_x & on_y
    assert perimeter.sum() == 124 and corner.sum() == 4
    assert np.array_equal(at90["mask"], perimeter)
    at200 = bref.boundary(pts, nrm, 1.5, 30, 200.0)
    assert np.array_equal(at200["mask"], corner)
    deg = np.degrees(at90["gap"])
    assert np.abs(deg[~perimeter] - 45.0).max() < 1e-9                     # 8 neighbours
    assert np.abs(deg[perimeter & ~corner] - 180.0).max() < 1e-9           # 5
    assert np.abs(deg[corner] - 270.0).max() < 1e-9                        # 3
    assert np.array_equal(at90["counts"], np.where(corner, 4, np.where(perimeter, 6, 9)))
    assert np.array_equal(at90["m"], at90["counts"] - 1)                   # the point itself is a member and is skipped


def test_restatement_on_a_closed_sphere():
    pts, nrm = bref.fibonacci_sphere(4096)
    ref = bref.boundary(pts, nrm, 0.12, 30, 90.0)
    assert not ref["mask"].any()
    assert 13 <= ref["counts"].min() and ref["counts"].max() <= 17
    assert abs(np.degrees(ref["gap"].max()) - 48.1) < 0.1


def test_restatement_on_a_cut_sphere():
    pts, nrm = bref.cut_sphere(4096, 0.5)
    assert len(pts) == 3072
    ref = bref.boundary(pts, nrm, 0.12, 30, 90.0)
    assert ref["mask"].sum() == 89
    assert (pts[ref["mask"], 2] > 0.5 - 0.12).all()                        # a point farther from the cut keeps its whole neighbourhood
