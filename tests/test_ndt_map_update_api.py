"""CPU-side checks of the normal-distributions map that grows: the five entry points are declared in the header, exported by the built library
and carry ctypes prototypes that match their declarations; the header states RULE OF A MAP / MERGE / INSERT / REMOVE_FAR after
pcr_registration_ndt and no longer calls the map unchangeable; the unit is in the build; the Python surface has the calls with their defaults and
refuses bad arguments on the host; facts of the numpy restatement (tests/ndt_map_update_reference.py); and the conditions of the GPU comparisons,
checked on the restatement alone.  Needs no GPU."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import ndt_map_update_cases as cases
import ndt_map_update_reference as nu
import ndt_reference as nd
import voxel_reference as vr
from conftest import ROOT, pkg, pose_error

_CTYPE = {"int64_t": C.c_int64, "int": C.c_int, "double": C.c_double}
# typed pointers; every other pointer is passed as an address
TYPED = {"grid_min3": C.c_double, "center3": C.c_double, "T": C.c_double, "removed": C.c_int64, "out": C.c_void_p, "min_points_per_voxel": C.c_int,
         "eigenvalue_ratio": C.c_double}
ENTRY_POINTS = {
    "pcr_ndt_map_create_on_grid": ["ctx", "xyz", "n", "voxel_size", "min_points_per_voxel", "eigenvalue_ratio", "grid_min3", "T", "out"],
    "pcr_ndt_map_insert": ["ctx", "map", "xyz", "n", "T"],
    "pcr_ndt_map_merge": ["ctx", "map", "other"],
    "pcr_ndt_map_remove_far": ["ctx", "map", "center3", "max_distance", "removed"],
    "pcr_ndt_map_rule": ["map", "grid_min3", "min_points_per_voxel", "eigenvalue_ratio"],
}
MAP_VOXEL = 2.0


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
            assert issubclass(at, C._Pointer) and at._type_ is TYPED[arg], (p, at)
        elif "*" in p:
            assert at is C.c_void_p, (p, at)
        else:
            assert at is _CTYPE[p.split()[-2]], (p, at)


def test_existing_entry_points_keep_their_signatures():
    P = pkg()
    hdr = _header()
    assert [p.split()[-1].lstrip("*") for p in _declaration(hdr, "pcr_ndt_map_grid")] == ["map", "origin3", "voxel_size"]
    assert [p.split()[-1].lstrip("*") for p in _declaration(hdr, "pcr_ndt_map_create")] == ["ctx", "xyz", "n", "voxel_size", "min_points_per_voxel", "eigenvalue_ratio", "out"]
    assert C.sizeof(P._lib.PcrNdtParams) == 32


def test_header_states_the_rules_after_the_registration_call():
    hdr = _header()
    ndt = hdr[hdr.index("NDT on a normal-distributions voxel map"):]
    assert "is never changed" not in ndt
    doc = ndt[ndt.index("int pcr_registration_ndt"):ndt.index("int pcr_ndt_map_create_on_grid")]
    for phrase in ("A normal-distributions map that grows", "RULE OF A MAP.", "g - voxel_size / 2", "compatible iff all four are equal bit for bit",
                   "pure function of\n *   (N_v, C_v, min_points_per_voxel, eigenvalue_ratio)", "MAP ON A GIVEN GRID, AT A POSE.", "p' = float32(q)",
                   "((T_r0 x + T_r1 y) + T_r2 z) + T_r3", "applied all\n *   the same", "below the origin counts too", "xyz lies outside the map's grid",
                   "row for row and bit for bit", "MERGE(A, B).", "keeps that row bit for bit: count, mean, C_v, A_v, validity", "N = N_a + N_b", "2^31 - 1",
                   "mu = float32((float64(N_a) a + float64(N_b) b) / float64(N))", "parallel-axis term", "d_a = float64(mu_a) - float64(mu)", "the NEW float32 mean",
                   "M_a = float64(C_a[rc]) + d_a[r] d_a[c]", "the product rounded first, then the sum", "C[rc] = float32((float64(N_a) M_a + float64(N_b) M_b) / float64(N))",
                   "those of MAP from (N, C)", "recomputed, never averaged", "commutative bit for bit", "not associative",
                   "INSERT(map, cloud, T) = MERGE(map, the map of the cloud at T on the map's grid with the map's rule)", "REMOVE_FAR(map, center c", "d^2 < r^2",
                   "in the order x, y, z", "A_v included", "would leave the map empty", "all or nothing", "swapped\n * in", "no other call may\n * use the map",
                   "stale afterwards", "no fused\n * multiply-add"):
        assert phrase in doc, phrase
    for name in ENTRY_POINTS:                                          # every declaration comes after pcr_registration_ndt
        assert re.search(r"\bint\s+" + name + r"\s*\(", ndt[ndt.index("int pcr_registration_ndt"):]), name


def test_unit_is_in_the_build_and_in_the_packed_fp32_scan():
    csrc = os.path.join(ROOT, "point-cloud-registration-with-global-refinement_amd", "csrc")
    assert os.path.exists(os.path.join(csrc, "pcr_nmap.hip"))
    assert re.search(r"^for f in .*\bpcr_nmap\b", open(os.path.join(csrc, "build.sh")).read(), re.M)
    assert '"pcr_nmap"' in open(os.path.join(ROOT, "tools", "pk_trans_scan.py")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "pcr_nmap.hip" in readme and "The map does not grow." not in readme
    assert "### 4.24" in open(os.path.join(ROOT, "DESIGN.md")).read()
    # the map's struct and the one function that makes A_v live in the shared header; both kernels call that function
    shared = open(os.path.join(csrc, "pcr_ndt.h")).read()
    ndt, nmap = open(os.path.join(csrc, "pcr_ndt.hip")).read(), open(os.path.join(csrc, "pcr_nmap.hip")).read()
    assert "struct pcr_ndt_map {" in shared and "struct NdtMapView {" in shared and "ndt_block_bytes" in shared
    assert "struct pcr_ndt_map {" not in ndt and "struct pcr_ndt_map {" not in nmap
    assert "ndt_cell_information(" in shared and "ndt_cell_information(" in ndt and "ndt_cell_information(" in nmap
    for text in (shared, nmap):                                        # plain C++: no inline assembly
        assert "asm" not in re.sub(r"//[^\n]*", "", text)


def test_python_surface_and_defaults():
    P = pkg()
    R = P.registration
    M = R.NormalDistributionsMap
    assert list(inspect.signature(M.__init__).parameters) == ["self", "target", "voxel_size", "min_points_per_voxel", "eigenvalue_ratio"]
    sig = inspect.signature(M.on_grid).parameters
    assert list(sig) == ["target", "voxel_size", "min_points_per_voxel", "eigenvalue_ratio", "grid_min", "transformation"]
    assert sig["min_points_per_voxel"].default == 6 and sig["eigenvalue_ratio"].default == 0.01 and sig["grid_min"].default is None and sig["transformation"].default is None
    sig = inspect.signature(M.insert).parameters
    assert list(sig) == ["self", "cloud", "transformation"] and sig["transformation"].default is None
    assert list(inspect.signature(M.merge).parameters) == ["self", "other"]
    assert list(inspect.signature(M.remove_far).parameters) == ["self", "center", "max_distance"]
    for name in ("grid_min", "origin", "voxel_size", "cells", "counts", "points", "covariances", "information", "valid"):
        assert isinstance(getattr(M, name), property), name
    assert isinstance(inspect.getattr_static(M, "centered_grid_min"), staticmethod)
    sig = inspect.signature(R.scan_to_map_odometry_ndt).parameters
    assert list(sig) == ["scans", "voxel_size", "init", "criteria", "neighborhood", "outlier_ratio", "min_points_per_voxel", "eigenvalue_ratio", "motion_model", "max_range",
                         "grid_min"]
    assert np.array_equal(sig["init"].default, np.eye(4)) and sig["criteria"].default is None and sig["neighborhood"].default == 7 and sig["outlier_ratio"].default == 0.55
    assert sig["min_points_per_voxel"].default == 6 and sig["eigenvalue_ratio"].default == 0.01 and sig["motion_model"].default == "constant_velocity"
    assert sig["max_range"].default is None and sig["grid_min"].default is None
    assert P.o3d.pipelines.registration.scan_to_map_odometry_ndt is R.scan_to_map_odometry_ndt
    import pcr_amd
    assert pcr_amd.registration.scan_to_map_odometry_ndt is R.scan_to_map_odometry_ndt
    doc = R.scan_to_map_odometry_ndt.__doc__
    order = [doc.index(w) for w in ("NormalDistributionsMap.on_grid(", "registration_ndt(", "map.insert(", "map.remove_far(")]
    assert order == sorted(order) and "Exactly these public calls, in this order" in doc
    # the voxel covariance recipe is as it was
    assert list(inspect.signature(R.scan_to_map_odometry).parameters) == ["scans", "voxel_size", "init", "estimation_method", "criteria", "neighborhood", "min_points_per_voxel",
                                                                          "motion_model", "max_range", "grid_min"]
    rng = np.random.default_rng(1)
    for p in rng.uniform(-500, 500, (5, 3)):
        assert np.array_equal(M.centered_grid_min(p, 2.0), R.VoxelCovarianceMap.centered_grid_min(p, 2.0))
        assert np.array_equal(M.centered_grid_min(p, 2.0), nu.centered_grid_min(p, 2.0))


class _NoDevice:
    """stands in for the context class: any use of a device inside the block fails the test"""

    @classmethod
    def current(cls):
        raise AssertionError("a device context was asked for")


def _host_cloud(P, n=5):
    import torch
    pc = P.PointCloud()
    pc._xyz = torch.zeros((n, 3), dtype=torch.float32)
    return pc


def _fake_open_map(P):
    """a map object that looks open without a library behind it: enough for the refusals that come before any device work"""
    M = P.registration.NormalDistributionsMap
    m = M.__new__(M)
    m._handle = C.c_void_p(0)            # (close() does not destroy a null handle)
    m._voxel_size, m.min_points_per_voxel, m.eigenvalue_ratio, m._cells = 1.0, 6, 0.01, 1
    return m


def test_host_side_refusals(monkeypatch):
    P = pkg()
    R = P.registration
    M = R.NormalDistributionsMap
    monkeypatch.setattr(P._lib, "Context", _NoDevice)
    g = np.zeros(3)
    with pytest.raises(ValueError, match=r"transformation must have shape \(4, 4\)"):
        M.on_grid(_host_cloud(P), 1.0, grid_min=g, transformation=np.eye(3))
    with pytest.raises(ValueError, match="grid_min must hold three numbers"):
        M.on_grid(_host_cloud(P), 1.0, grid_min=np.zeros(4))
    with pytest.raises(ValueError, match="needs a grid_min"):
        M.on_grid(_host_cloud(P), 1.0, transformation=np.eye(4))
    with pytest.raises(ValueError, match="voxel_size"):
        M.on_grid(_host_cloud(P), -1.0, grid_min=g)
    with pytest.raises(ValueError, match="min_points_per_voxel"):
        M.on_grid(_host_cloud(P), 1.0, 1, grid_min=g)
    with pytest.raises(ValueError, match="eigenvalue_ratio"):
        M.on_grid(_host_cloud(P), 1.0, 6, 1.5, grid_min=g)
    with pytest.raises(RuntimeError, match="at least one point"):
        M.on_grid(P.PointCloud(), 1.0, grid_min=g)
    with pytest.raises(AssertionError, match="device context"):      # good arguments: the next thing the call wants is the device
        M.on_grid(_host_cloud(P), 1.0, grid_min=g, transformation=np.eye(4))
    m = _fake_open_map(P)
    with pytest.raises(ValueError, match=r"insert: transformation must have shape \(4, 4\)"):
        m.insert(_host_cloud(P), np.zeros((3, 4)))
    with pytest.raises(RuntimeError, match="insert: the cloud must be a PointCloud with at least one point"):
        m.insert(P.PointCloud())
    with pytest.raises(TypeError, match="merge: other must be a NormalDistributionsMap"):
        m.merge(np.zeros((3, 3)))
    with pytest.raises(TypeError, match="merge: other must be a NormalDistributionsMap"):
        m.merge(R.VoxelCovarianceMap.__new__(R.VoxelCovarianceMap))
    with pytest.raises(ValueError, match="remove_far: center must hold three numbers"):
        m.remove_far([0, 0], 1.0)
    for bad in (0.0, -1.0, float("nan"), float("inf"), None):
        with pytest.raises(ValueError, match="remove_far: max_distance"):
            m.remove_far([0, 0, 0], bad)
    with pytest.raises(AssertionError, match="device context"):
        m.insert(_host_cloud(P))
    m._handle = None
    closed = M.__new__(M)
    for call in (lambda: closed.insert(_host_cloud(P)), lambda: closed.merge(_fake_open_map(P)), lambda: _fake_open_map(P).merge(closed),
                 lambda: closed.remove_far([0, 0, 0], 1.0), lambda: closed.grid_min, lambda: closed.origin, lambda: len(closed)):
        with pytest.raises(RuntimeError, match="closed"):
            call()
    # the odometry recipe
    fn = R.scan_to_map_odometry_ndt
    with pytest.raises(ValueError, match="motion_model"):
        fn([_host_cloud(P)], 1.0, motion_model="jerk")
    with pytest.raises(ValueError, match="at least one scan"):
        fn([], 1.0)
    with pytest.raises(RuntimeError, match="scan 1 must be a PointCloud with at least one point"):
        fn([_host_cloud(P), P.PointCloud()], 1.0)
    with pytest.raises(ValueError, match="max_range"):
        fn([_host_cloud(P)], 1.0, max_range=0.0)
    with pytest.raises(ValueError, match="neighborhood"):
        fn([_host_cloud(P)], 1.0, neighborhood=5)
    with pytest.raises(ValueError, match="eigenvalue_ratio"):
        fn([_host_cloud(P)], 1.0, eigenvalue_ratio=0.0)
    with pytest.raises(ValueError, match=r"init must have shape \(4, 4\)"):
        fn([_host_cloud(P)], 1.0, init=np.eye(3), grid_min=g)


# ------------------------------------------------------------------------------------------ facts of the restatement
def _equal(a, b):
    return (np.array_equal(a.cells, b.cells) and np.array_equal(a.count, b.count) and vr.bits_equal(a.mean, b.mean) and vr.bits_equal(a.cov6, b.cov6)
            and np.array_equal(a.valid, b.valid) and vr.bits_equal(a.info, b.info))


@pytest.fixture(scope="module")
def pair899(small_pair):
    src = vr.voxel_reference(small_pair["source"], 0.3).points
    tgt = vr.voxel_reference(small_pair["target"], 0.3).points
    assert (len(src), len(tgt)) == (6897, 7074)
    return src, tgt


def test_map_on_its_own_grid_without_a_pose_is_build_map(pair899):
    _, tgt = pair899
    for min_points, ratio in ((6, 0.01), (2, 1.0)):
        want = nd.build_map(tgt, MAP_VOXEL, min_points, ratio)
        got = nu.build_map_on_grid(tgt, MAP_VOXEL, tgt.astype(np.float64).min(0), None, min_points, ratio)
        assert _equal(got, want) and np.array_equal(got.origin, want.origin) and np.array_equal(got.cell_of_point, want.cell_of_point)


def test_merge_commutes_bit_for_bit_and_is_not_associative():
    rng = np.random.default_rng(7)
    cells = cases.block(5, 5, 4)
    maps = [nu.build_map_on_grid(cases.cell_cloud(cells[rng.random(len(cells)) < 0.7], 60 + k), 1.0, cases.GRID0, None, 6, 0.01) for k in range(3)]
    a, b, c = maps
    ab, ba = nu.merge(a, b), nu.merge(b, a)
    assert _equal(ab, ba) and len(np.intersect1d(vr.cell_key(a.cells), vr.cell_key(b.cells))) > 20
    left, right = nu.merge(ab, c), nu.merge(a, nu.merge(b, c))
    assert np.array_equal(left.cells, right.cells) and np.array_equal(left.count, right.count)
    assert not (vr.bits_equal(left.mean, right.mean) and vr.bits_equal(left.cov6, right.cov6))      # the roundings differ ...
    assert np.abs(left.cov6.astype(np.float64) - right.cov6.astype(np.float64)).max() < 1e-6         # ... by a few float32 steps
    # validity and A_v are a pure function of (N, C, rule) in every row of every map
    for m in (a, ab, left, right):
        info, valid, _ = nd.information(m.cov6, m.count, m.min_points, m.ratio)
        assert np.array_equal(valid, m.valid) and vr.bits_equal(info, m.info)
    other = nu.build_map_on_grid(cases.cell_cloud(cells, 70), 1.0, cases.GRID0, None, 5, 0.01)
    with pytest.raises(ValueError, match="not compatible"):
        nu.merge(a, other)


@pytest.mark.parametrize("min_points", [2, 3])
def test_two_one_point_cells(min_points):
    """a one-point cell merged with a one-point cell becomes valid iff min_points_per_voxel == 2 and the points differ; coincident points stay
    invalid with C = 0 exactly"""
    p, q = np.array([[0.25, 0.375, -0.125]], np.float32), np.array([[0.3, 0.1, 0.2]], np.float32)
    mp, mq = (nu.build_map_on_grid(x, 1.0, cases.GRID0, None, min_points, 0.01) for x in (p, q))
    assert not mp.valid[0] and not mq.valid[0] and not mp.cov6.any() and mp.count[0] == 1
    m = nu.merge(mp, mq)
    assert len(m.cells) == 1 and m.count[0] == 2 and bool(m.valid[0]) == (min_points == 2) and m.cov6[0, [0, 3, 5]].min() > 0
    one_shot = nu.build_map_on_grid(np.concatenate([p, q]), 1.0, cases.GRID0, None, min_points, 0.01)
    assert np.abs(m.cov6.astype(np.float64) - one_shot.cov6).max() < 1e-7 and np.array_equal(m.valid, one_shot.valid)
    same = nu.merge(mp, mp)
    assert same.count[0] == 2 and not same.valid[0] and not same.cov6.any() and not same.info.any() and vr.bits_equal(same.mean, mp.mean)
    for k in range(4):                                                 # ... and stay so however often they are merged
        same = nu.merge(same, mp)
    assert same.count[0] == 6 and not same.valid[0] and not same.cov6.any() and vr.bits_equal(same.mean, mp.mean)


def test_remove_far_keeps_bits_and_order():
    m = nu.build_map_on_grid(cases.cell_cloud(cases.block(5, 5, 4), 3), 1.0, cases.GRID0, None, 6, 0.01)
    centre = m.mean.astype(np.float64).mean(0)
    d2 = nu.distance2(m.mean, centre)
    r = float(np.sqrt(np.median(d2)))
    kept = nu.remove_far(m, centre, r)
    keep = d2 < r * r
    assert 0 < keep.sum() < len(keep) and np.array_equal(kept.cells, m.cells[keep]) and vr.bits_equal(kept.info, m.info[keep]) and np.array_equal(kept.valid, m.valid[keep])
    with pytest.raises(ValueError, match="would leave the map empty"):
        nu.remove_far(m, centre + 1e5, 1.0)


# ------------------------------------------------------------------------------------------ the conditions of the GPU comparisons
def test_condition_a_merge_against_a_one_shot_map(small_pair, pair899):
    """(a) two clouds with coordinates within 64 m: merge(map(A), map(B)) against the one-shot map of A u B on the same grid.  Counts and valid are
    equal and max |dC| <= 1e-4 voxel^2; without the parallel-axis term the covariances are off by more than 0.1 voxel^2."""
    src, tgt = pair899
    placed = nu.vu.place(src, np.zeros((len(src), 6), np.float32), small_pair["T_gicp"])[0]
    assert max(np.abs(tgt).max(), np.abs(placed).max()) < 64.0
    g = nu.centered_grid_min(tgt.astype(np.float64).mean(0), MAP_VOXEL)
    a, b = nu.build_map_on_grid(tgt, MAP_VOXEL, g), nu.build_map_on_grid(src, MAP_VOXEL, g, small_pair["T_gicp"])
    one_shot = nu.build_map_on_grid(np.concatenate([tgt, placed]), MAP_VOXEL, g)
    merged = nu.merge(a, b)
    shared = len(np.intersect1d(vr.cell_key(a.cells), vr.cell_key(b.cells)))
    assert shared > 300 and np.array_equal(merged.cells, one_shot.cells) and np.array_equal(merged.count, one_shot.count) and np.array_equal(merged.valid, one_shot.valid)
    err = float(np.abs(merged.cov6.astype(np.float64) - one_shot.cov6.astype(np.float64)).max()) / MAP_VOXEL ** 2
    flat = nu.merge(a, b, parallel_axis=False)
    err_flat = float(np.abs(flat.cov6.astype(np.float64) - one_shot.cov6.astype(np.float64)).max()) / MAP_VOXEL ** 2
    print(f"merge against one shot: {shared} shared cells, max |dC| = {err:.2e} voxel^2 (without the parallel-axis term {err_flat:.3f}); valid {int(a.valid.sum())} + "
          f"{int(b.valid.sum())} -> {int(merged.valid.sum())} of {len(merged.cells)}")
    assert err <= 1e-4 and err_flat >= 0.1
    assert merged.valid.sum() > max(a.valid.sum(), b.valid.sum())                      # cells become valid through the merge


def _gpu_reference_maps(small_pair, pair899):
    """every reference map the GPU tests compare against (tests/test_gpu_ndt_map_update.py builds the same ones)"""
    src, tgt = pair899
    g = nu.centered_grid_min(tgt.astype(np.float64).mean(0), MAP_VOXEL)
    t = nu.build_map_on_grid(tgt, MAP_VOXEL, g)
    grown = nu.insert(t, src, small_pair["T_gicp"])
    out = {"target": t, "grown": grown, "twice": nu.insert(grown, src, small_pair["T_gicp"]), "identity": nu.insert(t, src)}
    for name in cases.MERGE_CASES:
        _, _, xa, xb = cases.merge_case(name)
        ra, rb = (nu.build_map_on_grid(x, 1.0, cases.GRID0, None, cases.MIN_POINTS, 0.01) for x in (xa, xb))
        out[name + "_a"], out[name + "_b"], out[name] = ra, rb, nu.merge(ra, rb)
    return out


def test_condition_b_eigenvalue_gap_and_the_kinds_of_cells(small_pair, pair899):
    """(b) in every reference map a GPU test uses, each cell's lambda_max is exactly 0 or above 1e-12 voxel^2, so `valid` cannot hinge on the
    eigen-solver; and the hand-made merge cases hold every kind of cell the issue names"""
    maps = _gpu_reference_maps(small_pair, pair899)
    for name, m in maps.items():
        lam = nu.lambda_max(m)
        assert ((lam == 0.0) | (lam > 1e-12 * m.voxel ** 2)).all(), name
        assert np.array_equal(m.valid, (m.count >= m.min_points) & (lam > 0)), name
    through_merge = stays_invalid = planar = coincident = 0
    for name in cases.MERGE_CASES:
        ca, cb, xa, xb = cases.merge_case(name)
        ra, rb, m = maps[name + "_a"], maps[name + "_b"], maps[name]
        assert np.array_equal(np.unique(vr.cell_key(ra.cells)), np.unique(vr.cell_key(ca))) and np.array_equal(np.unique(vr.cell_key(rb.cells)), np.unique(vr.cell_key(cb)))
        assert 1 <= ra.count.min() and ra.count.max() <= 8 and rb.count.max() <= 8
        ka, kb, km = vr.cell_key(ra.cells), vr.cell_key(rb.cells), vr.cell_key(m.cells)
        both = np.isin(km, ka) & np.isin(km, kb)
        va = np.isin(km, ka[ra.valid]) | np.isin(km, kb[rb.valid])
        through_merge += int((both & m.valid & ~va).sum())
        stays_invalid += int((both & ~m.valid).sum())
        planar += int((both & m.valid & (m.clamped >= 1)).sum())
        coincident += int((both & (m.count >= cases.MIN_POINTS) & ~m.cov6.any(1)).sum())
        ma, mb = vr.morton3(ra.cells), vr.morton3(rb.cells)
        if name == "wholly_below":
            assert mb.max() < ma.min()
        if name == "wholly_above":
            assert mb.min() > ma.max()
        if name.startswith("rows"):
            n = int(name[4:])
            assert len(ma) == len(mb) == n and ma[0] == mb[0] and ma[-1] == mb[-1] and len(np.intersect1d(ma, mb)) == 2
        if name == "interleaved":
            shared = len(np.intersect1d(ma, mb))
            assert shared > 20 and len(ma) - shared > 20 and len(mb) - shared > 20
    m = maps["same_cell"]
    assert (maps["same_cell_a"].count[0], maps["same_cell_b"].count[0]) == (5, 1) and m.valid[0] and not maps["same_cell_a"].valid[0]      # 5 + 1
    print(f"merge cases: {through_merge} cells valid only through the merge, {stays_invalid} stay invalid, {planar} valid with a clamped eigenvalue, {coincident} of coincident points")
    assert through_merge >= 5 and stays_invalid >= 5 and planar >= 3 and coincident >= 1
    # pair 899: hundreds of cells of each kind
    t, grown = maps["target"], maps["grown"]
    shared = np.isin(vr.cell_key(grown.cells), vr.cell_key(t.cells)).sum()
    assert len(grown.cells) > len(t.cells) and shared == len(t.cells) and grown.valid.sum() > t.valid.sum() + 50
    assert grown.cells.min() > cases.MID - 200 and grown.cells.max() < cases.MID + 200          # all 63 key bits are in play


def _step():
    a = np.deg2rad(1.0)
    S = np.eye(4)
    S[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
    S[:3, 3] = [0.2, 0.0, 0.0]
    return S


@pytest.mark.parametrize("nbh", [7, 1])
def test_condition_c_odometry_on_the_restatement(pair899, nbh):
    """(c) pair 899's 0.3 m target seen from four poses advancing 0.2 m and 1 degree, 2.0 m cells, "static": every pose ends closer to the truth
    than its start, and the map's valid cells grow with every scan"""
    _, tgt = pair899
    truth, scans = [np.eye(4)], []
    for k in range(4):
        if k:
            truth.append(truth[-1] @ _step())
        inv = np.linalg.inv(truth[k])
        scans.append((tgt.astype(np.float64) @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32))
    g = nu.centered_grid_min(scans[0].astype(np.float64).mean(0), MAP_VOXEL)
    m = nu.build_map_on_grid(scans[0], MAP_VOXEL, g, np.eye(4))
    poses, valid = [np.eye(4)], [int(m.valid.sum())]
    for k in range(1, 4):
        res = nd.loop(m, scans[k], poses[-1], nbh)
        a0, d0 = pose_error(poses[-1], truth[k])
        a, d = pose_error(res.transformation, truth[k])
        print(f"nbh {nbh} scan {k}: start {np.degrees(a0):.3f} deg {d0:.3f} m -> {np.degrees(a):.4f} deg {d:.4f} m after {res.iterations} iterations; "
              f"{valid[-1]} of {len(m.cells)} cells valid")
        assert res.converged and a < a0 and d < d0, (k, a, d, a0, d0)
        poses.append(res.transformation)
        m = nu.insert(m, scans[k], poses[-1])
        valid.append(int(m.valid.sum()))
    assert valid[0] < valid[1] < valid[2] <= valid[3] and valid[0] == 458, valid          # (a cell needs 6 members: scan 0 alone leaves 287 of 745 unused)
