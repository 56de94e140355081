"""CPU-side checks of the frame that the two growing voxel maps share: both units include the shared header and instantiate its kernels with
their own row policy; both Python classes derive from one base and leave its lifecycle, merge and remove_far alone; remove_far refuses bad
arguments with the texts it had when each class carried its own copy; and the two odometry recipes issue the documented calls through the one
driver.  Needs no GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, pkg

CSRC = os.path.join(ROOT, "point-cloud-registration-with-global-refinement_amd", "csrc")
MAPS = {"VoxelCovarianceMap": ("pcr_vmap.hip", "VmapRow", "pcr_vgicp.h"), "NormalDistributionsMap": ("pcr_nmap.hip", "NmapRow", "pcr_ndt.h")}


def _src(name):
    return open(os.path.join(CSRC, name)).read()


@pytest.mark.parametrize("cls", list(MAPS))
def test_unit_takes_the_frame_from_the_shared_header(cls):
    unit, policy, home = MAPS[cls]
    text, frame = _src(unit), _src("pcr_mapgrow.h")
    assert '#include "pcr_mapgrow.h"' in text
    assert re.search(r"^#pragma clang fp contract\(off\)", text, re.M)              # contraction stays a matter of the unit
    assert "#pragma clang fp contract" not in re.sub(r"\{.*?^\}", "", frame, flags=re.S | re.M)      # ... never of the header's file scope
    assert f"struct {policy} {{" in _src(home)
    assert f"{policy}::combine(" in text                                             # the one thing that differs is the unit's own
    for host in ("map_merge_into", "map_remove_far"):
        assert f"{host}<{policy}>(" in text, host
    for kernel in ("k_map_merge_mark", "k_map_merge_write", "k_map_far_flags", "k_map_gather"):
        assert re.search(r"template <class Row>\s*__global__ void __launch_bounds__\(MG_BS\) " + kernel + r"\(", frame), kernel
        assert not re.search(r"__global__[^\n]*\bk_[vn]map_" + kernel[len("k_map_"):] + r"\b", text), kernel
    # one builder: the block is carved and hashed in one place for the four callers
    units = [_src(f) for f in ("pcr_vmap.hip", "pcr_nmap.hip", "pcr_vgicp.hip", "pcr_ndt.hip", "pcr_vgicp.h", "pcr_ndt.h", "pcr_mapgrow.h")]
    assert sum(t.count("SideLane own(") for t in units) == 1 and sum(t.count("pcr_dev_build_grid_batch(") for t in units) == 1
    assert "SideLane own(" in frame and "pcr_dev_build_grid_batch(" in frame
    assert "if (is_ndt" not in frame and "Never reserves the arena" in frame
    for f in ("pcr_vgicp.hip", "pcr_ndt.hip"):
        assert "map_build_block<" in _src(f), f
    assert "pcr_mapgrow.h" in open(os.path.join(ROOT, "README.md")).read()
    assert "The frame of the maps that grow" in open(os.path.join(ROOT, "DESIGN.md")).read()


def test_both_classes_derive_from_the_one_base():
    R = pkg().registration
    base = R._GrowingVoxelMap
    shared = ("_refresh", "close", "__del__", "__enter__", "__exit__", "_open", "__len__", "_pose", "centered_grid_min", "merge", "remove_far", "voxel_size", "_read",
              "cells", "counts", "points", "covariances", "to_point_cloud")
    for cls in (R.VoxelCovarianceMap, R.NormalDistributionsMap):
        assert cls.__bases__ == (base,)
        for name in shared:
            assert name in vars(base) and name not in vars(cls), (cls.__name__, name)
        for name in ("__init__", "on_grid", "insert", "grid_min", "origin", "correspondences", "_C", "_NAME", "_COLUMNS"):
            assert name in vars(cls), (cls.__name__, name)
        assert cls._NAME == cls.__name__
    assert R.VoxelCovarianceMap._C == "pcr_voxel_map" and R.NormalDistributionsMap._C == "pcr_ndt_map"
    assert list(R.VoxelCovarianceMap._COLUMNS) == ["cells", "counts", "points", "covariances"]
    assert list(R.NormalDistributionsMap._COLUMNS) == ["cells", "counts", "points", "covariances", "information", "valid"]
    for name in ("linearize", "information", "valid"):
        assert name in vars(R.NormalDistributionsMap) and not hasattr(R.VoxelCovarianceMap, name)
    assert "_cloud_arrays" in vars(R.VoxelCovarianceMap)
    src = open(R.__file__).read()
    maps = src[src.index("class _GrowingVoxelMap"):src.index("def multiscale_gicp")]
    assert maps.count("def remove_far") == 1 and maps.count("def close") == 1 and maps.count("def merge") == 1
    for fn in ("scan_to_map_odometry", "scan_to_map_odometry_ndt"):      # neither odometry function holds the loop
        body = maps[maps.index(f"def {fn}("):]
        body = body[:body.index("\ndef ", 1) if "\ndef " in body[1:] else len(body)]
        assert "_scan_to_map(" in body and "for k in range" not in body and ".insert(" not in body.split('"""')[2], fn


class _NoDevice:
    """stands in for the context class: any use of a device inside the block fails the test"""

    @classmethod
    def current(cls):
        raise AssertionError("a device context was asked for")


def _fake_open_map(cls):
    m = cls.__new__(cls)
    m._handle = C.c_void_p(0)            # (close() does not destroy a null handle)
    m._voxel_size, m._cells = 1.0, 1
    return m


@pytest.mark.parametrize("cls", list(MAPS))
def test_remove_far_refuses_with_the_texts_of_either_class(cls, monkeypatch):
    """the strings are those of the two separate remove_far methods before they became one"""
    P = pkg()
    monkeypatch.setattr(P._lib, "Context", _NoDevice)
    m = _fake_open_map(getattr(P.registration, cls))
    for center in ([0, 0], [0, 0, 0, 0], 1.0):
        with pytest.raises(ValueError) as e:
            m.remove_far(center, 1.0)
        assert str(e.value) == f"{cls}.remove_far: center must hold three numbers, got {center!r}"
    for bad in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError) as e:
            m.remove_far([0, 0, 0], bad)
        assert str(e.value) == f"{cls}.remove_far: max_distance must be a finite number greater than 0, got {bad!r}"
    for bad in (None, "far", [1.0, 2.0]):
        with pytest.raises(ValueError) as e:
            m.remove_far([0, 0, 0], bad)
        assert str(e.value) == f"{cls}.remove_far: max_distance must be a number greater than 0, got {bad!r}"
    with pytest.raises(AssertionError, match="device context"):      # good arguments: the next thing the call wants is the device
        m.remove_far([0, 0, 0], 1.0)
    m._handle = None
    with pytest.raises(RuntimeError) as e:
        m.remove_far([0, 0, 0], 1.0)
    assert str(e.value) == f"{cls}: the map is closed"


# ------------------------------------------------------------------------------------------ the odometry recipes
class _Scan:
    """a scan as the recipes use it before any map call: a length and a centre"""

    def __init__(self, k):
        self.k = k

    def __len__(self):
        return 5

    def get_center(self):
        return np.array([1.0 + self.k, 2.0, 3.0])


class _Result:
    def __init__(self, T):
        self.transformation = T


def _step(k):
    T = np.eye(4)
    T[:3, 3] = [0.5 * k, 0.25, 0.0]
    T[:2, :2] = [[np.cos(0.1 * k), -np.sin(0.1 * k)], [np.sin(0.1 * k), np.cos(0.1 * k)]]
    return T


def _recording(monkeypatch, R, kind, log, fail_at=None):
    """the map class and the registration call of one recipe replaced by stubs that write every call into `log`"""
    class Map:
        @staticmethod
        def _cloud_arrays(fn, cloud, what="cloud"):
            log.append(("check", what))

        @classmethod
        def on_grid(cls, *args):
            log.append(("on_grid",) + args)
            return cls()

        def insert(self, scan, T):
            log.append(("insert", scan, T))

        def remove_far(self, center, r):
            log.append(("remove_far", center, r))

        def close(self):
            log.append(("close",))

    def register(*args):
        log.append(("register",) + args)
        if fail_at is not None and args[0].k == fail_at:
            raise RuntimeError("the registration failed")
        return _Result(_step(args[0].k) @ args[3])

    monkeypatch.setattr(R, {"vgicp": "VoxelCovarianceMap", "ndt": "NormalDistributionsMap"}[kind], Map)
    monkeypatch.setattr(R, {"vgicp": "registration_voxelized_gicp", "ndt": "registration_ndt"}[kind], register)
    monkeypatch.setattr(R, "PointCloud", _Scan)      # (the NDT recipe's per-scan check is an isinstance and a len)
    return Map


@pytest.mark.parametrize("max_range", [None, 40.0])
@pytest.mark.parametrize("model", ["constant_velocity", "static"])
@pytest.mark.parametrize("kind", ["vgicp", "ndt"])
def test_odometry_issues_the_documented_calls(kind, model, max_range, monkeypatch):
    R = pkg().registration
    log = []
    Map = _recording(monkeypatch, R, kind, log)
    scans = [_Scan(k) for k in range(4)]
    init = _step(7)
    crit, est = object(), R.TransformationEstimationForGeneralizedICP(epsilon=2e-3)
    if kind == "vgicp":
        poses, results, m = R.scan_to_map_odometry(iter(scans), 2.0, init, est, crit, 7, 3, model, max_range)
        rule_on_grid, rule_register = (2.0, 2e-3), (est, crit, 7, 3)
    else:
        poses, results, m = R.scan_to_map_odometry_ndt(iter(scans), 2.0, init, crit, 27, 0.4, 5, 0.05, model, max_range)
        rule_on_grid, rule_register = (2.0, 5, 0.05), (crit, 27, 0.4, 5)
    assert isinstance(m, Map) and len(poses) == len(results) == 4 and results[0] is None and np.array_equal(poses[0], init)
    calls = [c for c in log if c[0] != "check"]
    assert [c[1] for c in log if c[0] == "check"] == ([f"scan {k}" for k in range(4)] if kind == "vgicp" else [])
    assert [c[0] for c in calls] == ["on_grid"] + (["register", "insert"] + (["remove_far"] if max_range else [])) * 3
    g = R._GrowingVoxelMap.centered_grid_min(init[:3, :3] @ scans[0].get_center() + init[:3, 3], 2.0)
    on_grid = calls[0]
    assert on_grid[1] is scans[0] and on_grid[2:2 + len(rule_on_grid)] == rule_on_grid and np.array_equal(on_grid[-2], g) and np.array_equal(on_grid[-1], init)
    per = 3 if max_range else 2
    for k in range(1, 4):
        reg, ins = calls[1 + (k - 1) * per], calls[2 + (k - 1) * per]
        start = poses[k - 1] if model == "static" or k < 2 else poses[k - 1] @ np.linalg.inv(poses[k - 2]) @ poses[k - 1]
        assert reg[1] is scans[k] and reg[2] is m and reg[3] is None and np.array_equal(reg[4], start) and reg[5:] == rule_register
        assert np.array_equal(poses[k], results[k].transformation) and np.array_equal(poses[k], _step(k) @ start)
        assert ins[1] is scans[k] and np.array_equal(ins[2], poses[k])
        if max_range:
            far = calls[3 + (k - 1) * per]
            assert np.array_equal(far[1], poses[k][:3, 3]) and far[2] == max_range
    assert ("close",) not in log                                       # the caller owns the returned map


@pytest.mark.parametrize("kind", ["vgicp", "ndt"])
def test_odometry_closes_the_map_when_a_registration_raises(kind, monkeypatch):
    R = pkg().registration
    log = []
    _recording(monkeypatch, R, kind, log, fail_at=2)
    fn = R.scan_to_map_odometry if kind == "vgicp" else R.scan_to_map_odometry_ndt
    with pytest.raises(RuntimeError, match="the registration failed"):
        fn([_Scan(k) for k in range(4)], 2.0, grid_min=np.zeros(3))
    calls = [c[0] for c in log if c[0] != "check"]
    assert calls == ["on_grid", "register", "insert", "register", "close"]
