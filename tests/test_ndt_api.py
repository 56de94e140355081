"""CPU-side checks of NDT registration: the entry points are declared in the header, exported by the built library and carry ctypes prototypes
that match their declarations; the header states the rule; the Python surface has the calls with their defaults and refuses bad arguments on the
host; facts of the numpy restatement of the rule (tests/ndt_reference.py) on hand-made shapes; and the condition of the GPU comparisons on pair
899, checked on the restatement alone.  Needs no GPU."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import ndt_reference as nd
import voxel_reference as vr
import voxelized_gicp_reference as vg
from conftest import ROOT, pkg, pose_error

_CTYPE = {"int64_t": C.c_int64, "int": C.c_int, "double": C.c_double}
# typed pointers; every other pointer is passed as an address
TYPED = {"cells": C.c_int64, "n_rows": C.c_int64, "T": C.c_double, "init_T": C.c_double, "out": C.c_void_p, "params": "PcrNdtParams", "result": "PcrResult",
         "origin3": C.c_double, "voxel_size": C.c_double, "JTJ": C.c_double, "JTr": C.c_double, "score": C.c_double, "sum_d2": C.c_double, "rows": C.c_int64,
         "points_with_rows": C.c_int64}
ENTRY_POINTS = {
    "pcr_ndt_map_create": ["ctx", "xyz", "n", "voxel_size", "min_points_per_voxel", "eigenvalue_ratio", "out"],
    "pcr_ndt_map_destroy": ["map"],
    "pcr_ndt_map_size": ["map", "cells"],
    "pcr_ndt_map_read": ["ctx", "map", "cell3", "count", "mean3", "cov6", "info6", "valid"],
    "pcr_ndt_map_grid": ["map", "origin3", "voxel_size"],
    "pcr_ndt_map_correspondences": ["ctx", "map", "src_xyz", "n_src", "T", "neighborhood", "rows2", "n_rows"],
    "pcr_ndt_linearize": ["ctx", "map", "src_xyz", "n_src", "T", "neighborhood", "outlier_ratio", "JTJ", "JTr", "score", "rows", "points_with_rows", "sum_d2"],
    "pcr_registration_ndt": ["ctx", "src_xyz", "n_src", "map", "init_T", "params", "result", "correspondences"],
}


def _header():
    return open(os.path.join(ROOT, "include", "pcr_hip.h")).read()


def _declaration(hdr, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
    assert m, f"{name} is not declared in include/pcr_hip.h"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


@pytest.mark.parametrize("name", list(ENTRY_POINTS))
def test_entry_point_is_declared_exported_and_prototyped(name):
    P = pkg()
    if not os.path.exists(P._lib.SO_PATH):
        P._lib.build()
    lib = P._lib.load()
    params = _declaration(_header(), name)
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


def test_params_struct_matches_the_header():
    P = pkg()
    body = re.search(r"typedef struct \{([^}]*)\} pcr_ndt_params;", _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(\w+)\s+(\w+)\s*;", body)
    assert [f for _, f in fields] == ["relative_fitness", "relative_rmse", "max_iteration", "neighborhood", "outlier_ratio"]
    assert [f for f, _ in P._lib.PcrNdtParams._fields_] == [f for _, f in fields]
    assert [t for _, t in P._lib.PcrNdtParams._fields_] == [{"double": C.c_double, "int32_t": C.c_int32}[t] for t, _ in fields]
    assert C.sizeof(P._lib.PcrNdtParams) == 32


def test_header_states_the_rule():
    hdr = _header()
    doc = hdr[:hdr.index("int pcr_ndt_map_create")]
    doc = doc[doc.rindex("NDT on a normal-distributions voxel map"):]
    for phrase in ("Biber", "Magnusson", "NormalDistributionsTransform", "neither normals nor covariances", "SAMPLE covariance", "min_points_per_voxel >= 2",
                   "eigenvalue_ratio in (0, 1]", "min_covar_eigvalue_mult", "exactly MAP\n *   of the voxelized GICP section", "d = float64(p_i) - float64(mu_v)",
                   "d_x d_x, d_x d_y, d_x d_z, d_y d_y, d_y d_z, d_z d_z", "rounded once to float64 and then to float32", "in input order", "VALID iff N_v >= min_points_per_voxel",
                   "S_v = C_v N_v / (N_v - 1)", "A_v = V diag(1 / max(lambda_k, eigenvalue_ratio lambda_max)) V^T", "kept in float64", "has A_v = 0",
                   "\"valid\" in place of \"N_v >= min_points_per_voxel\"", "c1 = 10 (1 - p), c2 = p / r^3, d3 = -log c2, d1 = -log(c1 + c2) - d3",
                   "d2 = -2 log((-log(c1 e^(-1/2) + c2) - d3) / d1)", "m = delta^T A_v delta", "e = exp(-d2 m / 2)", "w = -d1 d2 e", "J = [-skew(q_i) | I]",
                   "w J^T A_v J", "w J^T A_v delta", "-d1 e to the score", "NOT weighted by N_v", "LDLT, Rz Ry Rx", "No rows: the identity", "Gauss-Newton (IRLS)",
                   "positive semi-definite", "More-Thuente line\n *   search is NOT what runs", "(source points with at least one row) / n_src",
                   "n_correspondences = the number of rows", "PCR_EINVAL"):
        assert phrase in doc, phrase


def test_unit_is_in_the_build_and_in_the_packed_fp32_scan():
    csrc = os.path.join(ROOT, "point-cloud-registration-with-global-refinement_amd", "csrc")
    assert os.path.exists(os.path.join(csrc, "pcr_ndt.hip"))
    assert re.search(r"^for f in .*\bpcr_ndt\b", open(os.path.join(csrc, "build.sh")).read(), re.M)
    assert '"pcr_ndt"' in open(os.path.join(ROOT, "tools", "pk_trans_scan.py")).read()
    assert "pcr_ndt.hip" in open(os.path.join(ROOT, "README.md")).read()
    assert "### 4.22" in open(os.path.join(ROOT, "DESIGN.md")).read()
    # the kernel is plain C++: no inline assembly in the unit
    assert "asm" not in re.sub(r"//[^\n]*", "", open(os.path.join(csrc, "pcr_ndt.hip")).read())


def test_python_surface_and_defaults():
    P = pkg()
    R = P.registration
    sig = inspect.signature(R.registration_ndt).parameters
    assert list(sig) == ["source", "target_or_map", "voxel_size", "init", "criteria", "neighborhood", "outlier_ratio", "min_points_per_voxel"]
    assert sig["voxel_size"].default is None and sig["criteria"].default is None and np.array_equal(sig["init"].default, np.eye(4))
    assert sig["neighborhood"].default == 7 and sig["outlier_ratio"].default == 0.55 and sig["min_points_per_voxel"].default == 6
    sig = inspect.signature(R.NormalDistributionsMap.__init__).parameters
    assert list(sig) == ["self", "target", "voxel_size", "min_points_per_voxel", "eigenvalue_ratio"]
    assert sig["min_points_per_voxel"].default == 6 and sig["eigenvalue_ratio"].default == 0.01
    sig = inspect.signature(R.NormalDistributionsMap.correspondences).parameters
    assert list(sig) == ["self", "source", "T", "neighborhood"]
    sig = inspect.signature(R.NormalDistributionsMap.linearize).parameters
    assert list(sig) == ["self", "source", "T", "neighborhood", "outlier_ratio"] and sig["neighborhood"].default == 7 and sig["outlier_ratio"].default == 0.55
    for name in ("__len__", "cells", "counts", "points", "covariances", "information", "valid", "voxel_size", "origin", "to_point_cloud", "correspondences", "linearize",
                 "close", "__enter__", "__exit__"):
        assert hasattr(R.NormalDistributionsMap, name), name
    for name in ("cells", "counts", "points", "covariances", "information", "valid", "voxel_size", "origin"):
        assert isinstance(getattr(R.NormalDistributionsMap, name), property), name
    assert P.o3d.pipelines.registration.registration_ndt is R.registration_ndt
    assert P.o3d.pipelines.registration.NormalDistributionsMap is R.NormalDistributionsMap
    import pcr_amd
    assert pcr_amd.registration.NormalDistributionsMap is R.NormalDistributionsMap and pcr_amd.registration.registration_ndt is R.registration_ndt
    # the existing map and its registration are as they were
    assert list(inspect.signature(R.VoxelCovarianceMap.__init__).parameters) == ["self", "target", "voxel_size", "epsilon"]


class _NoDevice:
    """stands in for the context class: any use of a device inside the block fails the test"""

    @classmethod
    def current(cls):
        raise AssertionError("a device context was asked for")


def _host_cloud(P, n=5):
    """a cloud whose storage is host memory: enough for the checks that must come before any device work"""
    import torch
    pc = P.PointCloud()
    pc._xyz = torch.zeros((n, 3), dtype=torch.float32)
    return pc


BAD = [dict(neighborhood=0), dict(neighborhood=6), dict(neighborhood=26), dict(neighborhood=-1), dict(min_points_per_voxel=1), dict(min_points_per_voxel=0),
       dict(min_points_per_voxel=6.5), dict(outlier_ratio=0.0), dict(outlier_ratio=1.0), dict(outlier_ratio=-0.1), dict(outlier_ratio=float("nan")),
       dict(outlier_ratio=None), dict(voxel_size=0.0), dict(voxel_size=-1.0), dict(voxel_size=float("nan")), dict(voxel_size=float("inf")), dict(voxel_size=None)]


@pytest.mark.parametrize("bad", BAD, ids=[f"{k}={v}" for b in BAD for k, v in b.items()])
def test_bad_arguments_raise_value_error_before_a_device_is_touched(monkeypatch, bad):
    P = pkg()
    monkeypatch.setattr(P._lib, "Context", _NoDevice)
    args = dict(voxel_size=2.0)
    args.update(bad)
    with pytest.raises(ValueError, match="registration_ndt"):
        P.registration.registration_ndt(_host_cloud(P), _host_cloud(P), **args)
    if "voxel_size" in bad:
        with pytest.raises(ValueError, match="NormalDistributionsMap"):
            P.registration.NormalDistributionsMap(_host_cloud(P), bad["voxel_size"])


def test_other_host_side_refusals(monkeypatch):
    P = pkg()
    R = P.registration
    monkeypatch.setattr(P._lib, "Context", _NoDevice)
    for ratio in (0.0, -0.5, 1.5, float("nan"), None):
        with pytest.raises(ValueError, match="eigenvalue_ratio"):
            R.NormalDistributionsMap(_host_cloud(P), 2.0, 6, ratio)
    with pytest.raises(ValueError, match="min_points_per_voxel"):
        R.NormalDistributionsMap(_host_cloud(P), 2.0, 1)
    with pytest.raises(RuntimeError, match="at least one point"):
        R.NormalDistributionsMap(P.PointCloud(), 2.0)
    with pytest.raises(TypeError, match="PointCloud or a NormalDistributionsMap"):
        R.registration_ndt(_host_cloud(P), np.zeros((4, 3)), 2.0)
    # good arguments (eigenvalue_ratio 1 is allowed): the next thing either call wants is the device
    with pytest.raises(AssertionError, match="device context"):
        R.NormalDistributionsMap(_host_cloud(P), 2.0, 2, 1.0)
    with pytest.raises(AssertionError, match="device context"):
        R.registration_ndt(_host_cloud(P), _host_cloud(P), 2.0)


# ------------------------------------------------------------------------------------------ facts of the restatement
def test_score_constants():
    d1, d2 = nd.score_constants(0.55, 2.0)
    assert d1 == pytest.approx(-4.196518186951408, rel=1e-15) and d2 == pytest.approx(0.24847851012449546, rel=1e-14)
    assert -d1 * d2 > 0                                                 # the weight of a row


def test_cube_corners_in_one_cell_give_the_information_matrix_by_hand():
    """eight points on the corners of a cube of edge 2 h about c: mean c, C_v = h^2 I, S_v = (8 / 7) h^2 I, A_v = 7 / (8 h^2) I; nothing is
    clamped.  With h = 0.25 and c = (1, 1, 1) every number is exact in float32."""
    h, c = 0.25, np.array([1.0, 1.0, 1.0])
    corners = c + h * np.array([(sx, sy, sz) for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float64)
    mp = nd.build_map(corners.astype(np.float32), 4.0, 6)
    assert len(mp.cells) == 1 and mp.count[0] == 8 and mp.valid[0] and mp.clamped[0] == 0
    assert np.array_equal(mp.mean[0], c.astype(np.float32))
    assert np.array_equal(mp.cov6[0], np.array([h * h, 0, 0, h * h, 0, h * h], np.float32))
    assert np.allclose(mp.info[0], np.eye(3) * 7.0 / (8.0 * h * h), rtol=1e-14, atol=1e-14)
    # min_points_per_voxel above the count: the row stays, A_v = 0
    off = nd.build_map(corners.astype(np.float32), 4.0, 9)
    assert not off.valid[0] and not off.info.any() and np.array_equal(off.cov6, mp.cov6) and len(nd.rows_at(off, corners, np.eye(4), 27)) == 0
    # a point at the mean scores -d1 and pulls nowhere; a point off the mean is pulled towards it
    lin = nd.linearize(mp, c[None], np.eye(4), nd.rows_at(mp, c[None], np.eye(4), 1))
    d1, d2 = nd.score_constants(0.55, 4.0)
    assert lin.rows == 1 and lin.score == pytest.approx(-d1) and np.allclose(lin.JTr, 0) and np.allclose(lin.JTJ[3:, 3:], -d1 * d2 * mp.info[0])
    p = (c + [0.1, 0, 0])[None]
    lin = nd.linearize(mp, p, np.eye(4), nd.rows_at(mp, p, np.eye(4), 1))
    assert lin.JTr[3] > 0 and np.linalg.eigvalsh(lin.JTJ).min() > -1e-9 * np.abs(lin.JTJ).max()      # positive semi-definite


def test_planar_and_collinear_cells_get_clamped_eigenvalues():
    rng = np.random.default_rng(2)
    n = 40
    plane = np.stack([rng.uniform(0.2, 1.8, n), rng.uniform(0.2, 1.8, n), np.full(n, 1.0)], 1).astype(np.float32)
    mp = nd.build_map(plane, 4.0, 6, 0.01)
    assert len(mp.cells) == 1 and mp.valid[0] and mp.clamped[0] == 1            # exactly one: the normal direction
    lam = np.linalg.eigvalsh(np.linalg.inv(mp.info[0]))
    assert lam[0] == pytest.approx(0.01 * lam[2], rel=1e-9) and lam[1] > 0.01 * lam[2]
    line = (np.array([0.2, 0.3, 0.4]) + np.linspace(0, 1, n)[:, None] * np.array([1.0, 0.5, 0.25])).astype(np.float32)
    mp = nd.build_map(line, 4.0, 6, 0.01)
    assert mp.valid[0] and mp.clamped[0] == 2 and np.linalg.cond(mp.info[0]) == pytest.approx(100.0, rel=1e-6)
    same = np.tile(np.array([[0.25, 0.5, 0.75]], np.float32), (n, 1))
    mp = nd.build_map(same, 4.0, 6, 0.01)
    assert mp.count[0] == n and not mp.valid[0] and not mp.cov6.any()             # N identical points: invalid
    # eigenvalue_ratio 1: every eigenvalue is raised to the largest, A_v = I / lambda_max
    mp = nd.build_map(plane, 4.0, 6, 1.0)
    assert np.allclose(mp.info[0], np.eye(3) * mp.info[0][0, 0], rtol=1e-12, atol=1e-12 * mp.info[0][0, 0])


def test_member_statistic_is_summed_in_input_order():
    """C_v is build_map's ordered sum over the six products: on channels made order-sensitive the restatement must show the member order"""
    c = vr.case("n4097")
    mp = nd.build_map(c.xyz, 1.0, 2)
    means = vg.build_map(c.xyz, np.zeros((len(c.xyz), 6), np.float32), 1.0)
    prod = nd.member_products(c.xyz, means.mean[means.cell_of_point])
    assert prod.dtype == np.float32 and vr.bits_equal(mp.cov6, vg.build_map(c.xyz, prod, 1.0).cov6)
    d = c.xyz.astype(np.float64) - means.mean[means.cell_of_point].astype(np.float64)
    assert np.array_equal(prod[:, 1], (d[:, 0] * d[:, 1]).astype(np.float32))
    assert np.array_equal(mp.valid, (mp.count >= 2) & (mp.cov6[:, [0, 3, 5]].sum(1) > 0))


@pytest.fixture(scope="module")
def pair899(small_pair):
    src = vr.voxel_reference(small_pair["source"], 0.3).points
    tgt = vr.voxel_reference(small_pair["target"], 0.3).points
    assert (len(src), len(tgt)) == (6897, 7074)
    return src, tgt, nd.build_map(tgt, 2.0, 6)


def test_condition_of_the_gpu_comparisons_on_pair_899(pair899):
    """pair 899 at voxel 0.3 on a 2.0 m map with min_points_per_voxel 6: 733 cells of which 456 are valid; 36 cells hold exactly 5 points and
    45 exactly 6 (the threshold is exercised on both sides); 330 valid cells have a clamped eigenvalue, 96 of them two (234 exactly one)"""
    _, _, mp = pair899
    assert (len(mp.cells), int(mp.valid.sum())) == (733, 456)
    assert (int((mp.count == 5).sum()), int((mp.count == 6).sum())) == (36, 45)
    assert not mp.valid[mp.count < 6].any() and mp.valid[mp.count >= 6].all()
    assert (int((mp.clamped[mp.valid] >= 1).sum()), int((mp.clamped[mp.valid] == 2).sum())) == (330, 96)
    w = np.linalg.eigvalsh(mp.info[mp.valid])
    assert (w > 0).all() and (w[:, 2] / w[:, 0] <= 100.0 * (1 + 1e-9)).all()          # the clamp bounds the condition number by 1 / eigenvalue_ratio


@pytest.mark.parametrize("nbh", [1, 7, 27])
def test_restatement_loop_converges_from_T_fgr(small_pair, pair899, nbh):
    src, _, mp = pair899
    res = nd.loop(mp, src, small_pair["T_fgr"], nbh, max_it=40)
    scores = res.extra["scores"]
    print(f"nbh {nbh}: {res.iterations} iterations, score {scores[0]:.1f} -> {scores[-1]:.1f}, fitness {res.fitness:.4f}, rows {res.n_rows}")
    assert res.converged and 1 < res.iterations < 40
    assert scores[0] <= scores[1] <= scores[2] <= scores[3]                  # the score at the start and after each of the first three iterations
    a0, d0 = pose_error(small_pair["T_fgr"], small_pair["T_gicp"])
    a, d = pose_error(res.transformation, small_pair["T_gicp"])
    assert a < a0 and d < d0
