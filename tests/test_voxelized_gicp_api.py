"""CPU-side checks of voxelized GICP: the six entry points are declared in the header, exported by the built library and carry ctypes
prototypes that match their declarations; the header states the rule; the Python surface has the calls with their defaults and refuses bad
arguments on the host; facts of the numpy restatement of the rule (tests/voxelized_gicp_reference.py) on known shapes; and the condition
of the GPU comparisons on pair 899, checked on the restatement alone.  Needs no GPU."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import voxel_reference as vr
import voxelized_gicp_reference as vg
from conftest import ROOT, pkg

_CTYPE = {"int64_t": C.c_int64, "int": C.c_int, "double": C.c_double}
# typed pointers; every other pointer is passed as an address
TYPED = {"cells": C.c_int64, "n_rows": C.c_int64, "T": C.c_double, "init_T": C.c_double, "out": C.c_void_p, "params": "PcrVgicpParams", "result": "PcrResult"}
ENTRY_POINTS = {
    "pcr_voxel_map_create": ["ctx", "xyz", "cov6", "normals", "n", "voxel_size", "epsilon", "out"],
    "pcr_voxel_map_destroy": ["map"],
    "pcr_voxel_map_size": ["map", "cells"],
    "pcr_voxel_map_read": ["ctx", "map", "cell3", "count", "mean3", "cov6"],
    "pcr_voxel_map_correspondences": ["ctx", "map", "src_xyz", "n_src", "T", "neighborhood", "min_points_per_voxel", "rows2", "n_rows"],
    "pcr_registration_voxelized_gicp": ["ctx", "src_xyz", "src_cov6", "src_normals", "n_src", "map", "init_T", "params", "result", "correspondences"],
}


def _declaration(hdr, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
    assert m, f"{name} is not declared in include/pcr_hip.h"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


@pytest.mark.parametrize("name", list(ENTRY_POINTS))
def test_entry_point_is_declared_exported_and_prototyped(name):
    P = pkg()
    hdr = open(os.path.join(ROOT, "include", "pcr_hip.h")).read()
    if not os.path.exists(P._lib.SO_PATH):
        P._lib.build()
    lib = P._lib.load()
    params = _declaration(hdr, name)
    assert [p.split()[-1].lstrip("*") for p in params] == ENTRY_POINTS[name]
    assert name in P._lib.EXPORTS
    assert hasattr(lib, name), f"{name} is not exported by libpcr_hip.so"
    fn = getattr(lib, name)
    assert fn.restype is C.c_int and fn.argtypes is not None, f"{name} has no prototype in _lib"
    assert len(fn.argtypes) == len(params), params
    for at, p in zip(fn.argtypes, params):
        arg = p.split()[-1].lstrip("*")
        if "*" in p and arg in TYPED:
            want = getattr(P._lib, TYPED[arg]) if isinstance(TYPED[arg], str) else TYPED[arg]
            assert issubclass(at, C._Pointer) and at._type_ is want, (p, at)
        elif "*" in p:
            assert at is C.c_void_p, (p, at)
        else:
            assert at is _CTYPE[p.split()[-2]], (p, at)


def test_params_struct_is_the_gicp_parameters_plus_two():
    P = pkg()
    hdr = open(os.path.join(ROOT, "include", "pcr_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} pcr_vgicp_params;", hdr, re.S).group(1)
    fields = re.findall(r"(\w+)\s*;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    gicp = [f for f, _ in P._lib.PcrGicpParams._fields_]
    assert fields == gicp + ["neighborhood", "min_points_per_voxel"]
    assert [f for f, _ in P._lib.PcrVgicpParams._fields_] == fields
    assert P._lib.PcrVgicpParams._fields_[:len(gicp)] == P._lib.PcrGicpParams._fields_
    assert [t for _, t in P._lib.PcrVgicpParams._fields_[len(gicp):]] == [C.c_int32, C.c_int32]


def test_header_states_the_rule():
    hdr = open(os.path.join(ROOT, "include", "pcr_hip.h")).read()
    doc = hdr[:hdr.index("int pcr_voxel_map_create")]
    doc = doc[doc.rindex("voxelized GICP on a voxel covariance map"):]
    for phrase in ("Koide", "origin = min - voxel_size / 2", "floor((p - origin) / voxel_size)", "21 bits", "in input order", "Morton order", "epsilon",
                   "((T_r0 x + T_r1 y) + T_r2 z) + T_r3", "no fused multiply-add", "(0,0,0), (+1,0,0), (-1,0,0), (0,+1,0), (0,-1,0), (0,0,+1), (0,0,-1)",
                   "lexicographic order, dx slowest", "min_points_per_voxel", "ordered by i, then by offset order", "N_v times",
                   "W = (C_v + R C_i R^T)^(-1/2)", "LDLT, Rz Ry Rx", "No rows: the identity", "(source points with at least one row) / n_src",
                   "n_correspondences = the number of rows", "no\n *   max_correspondence_distance", "PCR_EINVAL"):
        assert phrase in doc, phrase


def test_unit_is_in_the_build_and_in_the_packed_fp32_scan():
    csrc = os.path.join(ROOT, "point-cloud-registration-with-global-refinement_amd", "csrc")
    assert os.path.exists(os.path.join(csrc, "pcr_vgicp.hip"))
    assert re.search(r"^for f in .*\bpcr_vgicp\b", open(os.path.join(csrc, "build.sh")).read(), re.M)
    assert '"pcr_vgicp"' in open(os.path.join(ROOT, "tools", "pk_trans_scan.py")).read()
    assert "pcr_vgicp.hip" in open(os.path.join(ROOT, "README.md")).read()


def test_python_surface_and_defaults():
    P = pkg()
    R = P.registration
    sig = inspect.signature(R.registration_voxelized_gicp).parameters
    assert list(sig) == ["source", "target_or_map", "voxel_size", "init", "estimation_method", "criteria", "neighborhood", "min_points_per_voxel"]
    assert sig["voxel_size"].default is None and sig["estimation_method"].default is None and sig["criteria"].default is None
    assert np.array_equal(sig["init"].default, np.eye(4)) and sig["neighborhood"].default == 1 and sig["min_points_per_voxel"].default == 1
    sig = inspect.signature(R.VoxelCovarianceMap.__init__).parameters
    assert list(sig) == ["self", "target", "voxel_size", "epsilon"] and sig["epsilon"].default == 1e-3
    sig = inspect.signature(R.VoxelCovarianceMap.correspondences).parameters
    assert list(sig) == ["self", "source", "T", "neighborhood", "min_points_per_voxel"]
    assert sig["neighborhood"].default == 1 and sig["min_points_per_voxel"].default == 1
    for name in ("__len__", "cells", "counts", "points", "covariances", "to_point_cloud", "correspondences", "close", "__enter__", "__exit__"):
        assert hasattr(R.VoxelCovarianceMap, name), name
    assert P.o3d.pipelines.registration.registration_voxelized_gicp is R.registration_voxelized_gicp
    assert isinstance(P.PointCloud.covariances, property) and P.PointCloud.covariances.fset is not None


class _NoDevice:
    """stands in for the context class: any use of a device inside the block fails the test"""

    @classmethod
    def current(cls):
        raise AssertionError("a device context was asked for")


def _host_cloud(P, n=5, normals=True, covariances=False):
    """a cloud whose storage is host memory: enough for the checks that must come before any device work"""
    import torch
    pc = P.PointCloud()
    pc._xyz = torch.zeros((n, 3), dtype=torch.float32)
    if normals:
        pc._nrm = torch.zeros((n, 3), dtype=torch.float32)
    if covariances:
        pc._cov = torch.zeros((n, 6), dtype=torch.float32)
    return pc


BAD = [dict(neighborhood=0), dict(neighborhood=6), dict(neighborhood=26), dict(neighborhood=-1), dict(min_points_per_voxel=0), dict(min_points_per_voxel=-2),
       dict(min_points_per_voxel=1.5), dict(voxel_size=0.0), dict(voxel_size=-1.0), dict(voxel_size=float("nan")), dict(voxel_size=float("inf")),
       dict(voxel_size=None)]


@pytest.mark.parametrize("bad", BAD, ids=[f"{k}={v}" for b in BAD for k, v in b.items()])
def test_bad_arguments_raise_value_error_before_a_device_is_touched(monkeypatch, bad):
    P = pkg()
    monkeypatch.setattr(P._lib, "Context", _NoDevice)
    args = dict(voxel_size=1.0, neighborhood=1, min_points_per_voxel=1)
    args.update(bad)
    with pytest.raises(ValueError, match="registration_voxelized_gicp"):
        P.registration.registration_voxelized_gicp(_host_cloud(P), _host_cloud(P), **args)
    if "voxel_size" in bad:
        with pytest.raises(ValueError, match="VoxelCovarianceMap"):
            P.registration.VoxelCovarianceMap(_host_cloud(P), bad["voxel_size"])


def test_other_host_side_refusals(monkeypatch):
    P = pkg()
    R = P.registration
    monkeypatch.setattr(P._lib, "Context", _NoDevice)
    with pytest.raises(RuntimeError, match="neither covariances nor normals"):
        R.VoxelCovarianceMap(_host_cloud(P, normals=False), 1.0)
    with pytest.raises(RuntimeError, match="at least one point"):
        R.VoxelCovarianceMap(P.PointCloud(), 1.0)
    with pytest.raises(RuntimeError, match="TransformationEstimationForGeneralizedICP"):
        R.registration_voxelized_gicp(_host_cloud(P), _host_cloud(P), 1.0, estimation_method=R.TransformationEstimationPointToPlane())
    with pytest.raises(TypeError, match="PointCloud or a VoxelCovarianceMap"):
        R.registration_voxelized_gicp(_host_cloud(P), np.zeros((4, 3)), 1.0)
    with pytest.raises(ValueError, match="covariances must have shape"):
        _host_cloud(P).covariances = np.zeros((5, 4))
    # good arguments: the next thing either call wants is the device
    with pytest.raises(AssertionError, match="device context"):
        R.VoxelCovarianceMap(_host_cloud(P), 1.0)
    with pytest.raises(AssertionError, match="device context"):
        R.registration_voxelized_gicp(_host_cloud(P, covariances=True), _host_cloud(P, covariances=True), 1.0)


# ------------------------------------------------------------------------------------------ facts of the restatement
def _unit_cov6(n):
    return np.tile(np.array([1, 0, 0, 1, 0, 1], np.float32), (n, 1))


def test_a_cloud_against_its_own_map_has_fitness_one():
    rng = np.random.default_rng(5)
    xyz = rng.uniform(-3, 3, (400, 3)).astype(np.float32)
    mp = vg.build_map(xyz, _unit_cov6(len(xyz)), 0.7)
    rows = vg.rows_at(mp, xyz, np.eye(4), 1)
    assert np.array_equal(rows[:, 0], np.arange(len(xyz))) and np.array_equal(rows[:, 1], mp.cell_of_point)
    assert vg.evaluate(mp, xyz, np.eye(4), rows)[0] == 1.0
    assert mp.count.sum() == len(xyz) and (vr.morton3(mp.cells)[1:] > vr.morton3(mp.cells)[:-1]).all()
    # a cell of c members gives its rows only from min_points_per_voxel <= c
    rows3 = vg.rows_at(mp, xyz, np.eye(4), 1, 3)
    assert np.array_equal(rows3[:, 0], np.nonzero(mp.count[mp.cell_of_point] >= 3)[0])


def test_rows_on_a_full_lattice_of_single_point_cells():
    g = np.arange(3)
    xyz = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    mp = vg.build_map(xyz, _unit_cov6(27), 1.0)
    assert len(mp.cells) == 27 and (mp.count == 1).all() and np.array_equal(mp.origin, [-0.5] * 3)
    centre, corner = int(np.nonzero((xyz == 1).all(1))[0][0]), int(np.nonzero((xyz == 0).all(1))[0][0])
    for nbh, n_centre, n_corner in ((1, 1, 1), (7, 7, 4), (27, 27, 8)):
        rows = vg.rows_at(mp, xyz, np.eye(4), nbh)
        assert (rows[:, 0] == centre).sum() == n_centre and (rows[:, 0] == corner).sum() == n_corner, nbh
        assert (np.diff(rows[:, 0]) >= 0).all()
        # the rows of the centre point list the cells in offset order
        got = mp.cells[rows[rows[:, 0] == centre, 1]]
        assert np.array_equal(got, 1 + vg.OFFSETS[nbh]), nbh
    assert len(vg.rows_at(mp, xyz, np.eye(4), 27, 2)) == 0


def test_condition_of_the_gpu_comparisons_on_pair_899(small_pair):
    """At least half of the source points of pair 899 (both clouds at voxel 0.3, a 1.0 m map, at T_fgr) have a row for neighbourhood 1
    (measured when the feature was written: 0.737), so the trajectories of tests/test_gpu_voxelized_gicp.py are driven by thousands of rows."""
    src = vr.voxel_reference(small_pair["source"], 0.3).points
    tgt = vr.voxel_reference(small_pair["target"], 0.3).points
    assert (len(src), len(tgt)) == (6897, 7074)
    mp = vg.build_map(tgt, _unit_cov6(len(tgt)), 1.0)
    rows = vg.rows_at(mp, src, small_pair["T_fgr"], 1)
    fit, rmse = vg.evaluate(mp, src, small_pair["T_fgr"], rows)
    print(f"pair 899: fitness {fit:.4f} with {len(rows)} rows, rmse {rmse:.4f}; neighbourhood 7: {len(vg.rows_at(mp, src, small_pair['T_fgr'], 7))} rows")
    assert fit >= 0.5
