"""CPU-side checks of the voxel covariance map that grows: the five entry points are declared in the header, exported by the built library and
carry ctypes prototypes that match their declarations; the header states the GRID / MERGE / INSERT / REMOVE_FAR rules and no longer calls the map
read-only; the Python surface has the calls with their defaults and refuses bad arguments on the host; facts of the numpy restatement
(tests/voxel_map_update_reference.py); and the condition of the GPU comparisons on pair 899, checked on the restatement alone.  Needs no GPU."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import voxel_map_update_reference as vu
import voxel_reference as vr
import voxelized_gicp_reference as vg
from conftest import ROOT, pkg

_CTYPE = {"int64_t": C.c_int64, "int": C.c_int, "double": C.c_double}
# typed pointers; every other pointer is passed as an address
TYPED = {"grid_min3": C.c_double, "origin3": C.c_double, "voxel_size": C.c_double, "center3": C.c_double, "T": C.c_double, "removed": C.c_int64, "out": C.c_void_p}
ENTRY_POINTS = {
    "pcr_voxel_map_create_on_grid": ["ctx", "xyz", "cov6", "normals", "n", "voxel_size", "epsilon", "grid_min3", "T", "out"],
    "pcr_voxel_map_insert": ["ctx", "map", "xyz", "cov6", "normals", "n", "epsilon", "T"],
    "pcr_voxel_map_merge": ["ctx", "map", "other"],
    "pcr_voxel_map_remove_far": ["ctx", "map", "center3", "max_distance", "removed"],
    "pcr_voxel_map_grid": ["map", "grid_min3", "origin3", "voxel_size"],
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
            assert issubclass(at, C._Pointer) and at._type_ is TYPED[arg], (p, at)
        elif "*" in p:
            assert at is C.c_void_p, (p, at)
        else:
            assert at is _CTYPE[p.split()[-2]], (p, at)


def test_header_states_the_rules_and_drops_read_only():
    hdr = open(os.path.join(ROOT, "include", "pcr_hip.h")).read()
    doc = hdr[:hdr.index("int pcr_voxel_map_create")]
    doc = doc[doc.rindex("voxelized GICP on a voxel covariance map"):]
    assert "read-only" not in doc
    for phrase in ("GRID.", "g - voxel_size / 2", "equal bit for bit", "MAP ON A GIVEN GRID, AT A POSE.", "p' = float32(q)", "C' = float32((R C) R^T)",
                   "(a0 b0 + a1 b1) + a2 b2", "below the origin counts too", "outside the map's grid", "MERGE(A, B).", "N = N_a + N_b", "2^31 - 1",
                   "float32((float64(N_a) float64(a) + float64(N_b) float64(b)) / float64(N))", "exact for counts below 2^29", "commutative bit for bit",
                   "not associative", "INSERT(map, cloud, T) = MERGE(map,", "REMOVE_FAR(map, center c", "d^2 < r^2", "in the order x, y, z",
                   "keep their bits and their relative order", "never has zero rows", "would leave the map empty", "all or nothing", "no other call may use the map",
                   "stale afterwards"):
        assert phrase in doc, phrase


def test_unit_is_in_the_build_and_in_the_packed_fp32_scan():
    csrc = os.path.join(ROOT, "point-cloud-registration-with-global-refinement_amd", "csrc")
    assert os.path.exists(os.path.join(csrc, "pcr_vmap.hip"))
    assert re.search(r"^for f in .*\bpcr_vmap\b", open(os.path.join(csrc, "build.sh")).read(), re.M)
    assert '"pcr_vmap"' in open(os.path.join(ROOT, "tools", "pk_trans_scan.py")).read()
    assert "pcr_vmap.hip" in open(os.path.join(ROOT, "README.md")).read()
    # the map's struct lives in the shared header, not in the unit of the iteration kernel
    assert "struct pcr_voxel_map {" in open(os.path.join(csrc, "pcr_vgicp.h")).read()
    assert "struct pcr_voxel_map {" not in open(os.path.join(csrc, "pcr_vgicp.hip")).read()


def test_python_surface_and_defaults():
    P = pkg()
    R = P.registration
    M = R.VoxelCovarianceMap
    sig = inspect.signature(M.on_grid).parameters
    assert list(sig) == ["target", "voxel_size", "epsilon", "grid_min", "transformation"]
    assert sig["epsilon"].default == 1e-3 and sig["grid_min"].default is None and sig["transformation"].default is None
    sig = inspect.signature(M.insert).parameters
    assert list(sig) == ["self", "cloud", "transformation"] and np.array_equal(sig["transformation"].default, np.eye(4))
    assert list(inspect.signature(M.merge).parameters) == ["self", "other"]
    assert list(inspect.signature(M.remove_far).parameters) == ["self", "center", "max_distance"]
    for name in ("grid_min", "origin", "voxel_size"):
        assert isinstance(getattr(M, name), property), name
    assert isinstance(inspect.getattr_static(M, "centered_grid_min"), staticmethod)
    sig = inspect.signature(R.scan_to_map_odometry).parameters
    assert list(sig) == ["scans", "voxel_size", "init", "estimation_method", "criteria", "neighborhood", "min_points_per_voxel", "motion_model", "max_range", "grid_min"]
    assert np.array_equal(sig["init"].default, np.eye(4)) and sig["estimation_method"].default is None and sig["criteria"].default is None
    assert sig["neighborhood"].default == 1 and sig["min_points_per_voxel"].default == 1 and sig["motion_model"].default == "constant_velocity"
    assert sig["max_range"].default is None and sig["grid_min"].default is None
    assert P.o3d.pipelines.registration.scan_to_map_odometry is R.scan_to_map_odometry


def test_centered_grid_min_puts_the_point_in_the_middle():
    M = pkg().registration.VoxelCovarianceMap
    rng = np.random.default_rng(1)
    for voxel in (1.0, 0.3, 2.5):
        for p in rng.uniform(-500, 500, (20, 3)):
            g = M.centered_grid_min(p, voxel)
            assert g.dtype == np.float64 and np.array_equal(g, vu.centered_grid_min(p, voxel))
            assert np.array_equal(g, np.floor(p / voxel) * voxel - 2.0 ** 20 * voxel)
            idx = np.floor((p - vu.grid_origin(g, voxel)) / voxel)
            assert (np.abs(idx - 2 ** 20) <= 1).all(), idx
    with pytest.raises(ValueError, match="centered_grid_min"):
        M.centered_grid_min([0, 0], 1.0)
    with pytest.raises(ValueError, match="centered_grid_min"):
        M.centered_grid_min([0, 0, 0], 0.0)


class _NoDevice:
    """stands in for the context class: any use of a device inside the block fails the test"""

    @classmethod
    def current(cls):
        raise AssertionError("a device context was asked for")


def _host_cloud(P, n=5, normals=True):
    import torch
    pc = P.PointCloud()
    pc._xyz = torch.zeros((n, 3), dtype=torch.float32)
    if normals:
        pc._nrm = torch.zeros((n, 3), dtype=torch.float32)
    return pc


def _fake_open_map(P):
    """a map object that looks open without a library behind it: enough for the refusals that come before any device work"""
    m = P.registration.VoxelCovarianceMap.__new__(P.registration.VoxelCovarianceMap)
    m._handle = C.c_void_p(0)            # (close() does not destroy a null handle)
    m._voxel_size, m.epsilon, m._cells = 1.0, 1e-3, 1
    return m


def test_host_side_refusals(monkeypatch):
    P = pkg()
    R = P.registration
    M = R.VoxelCovarianceMap
    monkeypatch.setattr(P._lib, "Context", _NoDevice)
    g = np.zeros(3)
    with pytest.raises(ValueError, match=r"transformation must have shape \(4, 4\)"):
        M.on_grid(_host_cloud(P), 1.0, grid_min=g, transformation=np.eye(3))
    with pytest.raises(ValueError, match="grid_min must hold three numbers"):
        M.on_grid(_host_cloud(P), 1.0, grid_min=np.zeros(4))
    with pytest.raises(ValueError, match="needs a grid_min"):
        M.on_grid(_host_cloud(P), 1.0, transformation=np.eye(4))
    with pytest.raises(RuntimeError, match="neither covariances nor normals"):
        M.on_grid(_host_cloud(P, normals=False), 1.0, grid_min=g)
    with pytest.raises(ValueError, match="voxel_size"):
        M.on_grid(_host_cloud(P), -1.0, grid_min=g)
    with pytest.raises(AssertionError, match="device context"):      # good arguments: the next thing the call wants is the device
        M.on_grid(_host_cloud(P), 1.0, grid_min=g, transformation=np.eye(4))
    m = _fake_open_map(P)
    with pytest.raises(ValueError, match=r"insert: transformation must have shape \(4, 4\)"):
        m.insert(_host_cloud(P), np.zeros((3, 4)))
    with pytest.raises(RuntimeError, match="insert: the cloud has neither covariances nor normals"):
        m.insert(_host_cloud(P, normals=False))
    with pytest.raises(RuntimeError, match="insert: the cloud must be a PointCloud with at least one point"):
        m.insert(P.PointCloud())
    with pytest.raises(TypeError, match="merge: other must be a VoxelCovarianceMap"):
        m.merge(np.zeros((3, 3)))
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
                 lambda: closed.remove_far([0, 0, 0], 1.0), lambda: closed.grid_min, lambda: closed.origin):
        with pytest.raises(RuntimeError, match="closed"):
            call()
    # the odometry recipe
    with pytest.raises(ValueError, match="motion_model"):
        R.scan_to_map_odometry([_host_cloud(P)], 1.0, motion_model="jerk")
    with pytest.raises(ValueError, match="at least one scan"):
        R.scan_to_map_odometry([], 1.0)
    with pytest.raises(RuntimeError, match="scan 1 has neither covariances nor normals"):
        R.scan_to_map_odometry([_host_cloud(P), _host_cloud(P, normals=False)], 1.0)
    with pytest.raises(ValueError, match="max_range"):
        R.scan_to_map_odometry([_host_cloud(P)], 1.0, max_range=0.0)
    with pytest.raises(ValueError, match=r"init must have shape \(4, 4\)"):
        R.scan_to_map_odometry([_host_cloud(P)], 1.0, init=np.eye(3), grid_min=g)


# ------------------------------------------------------------------------------------------ facts of the restatement
def _unit_cov6(n):
    return np.tile(np.array([1, 0, 0, 1, 0, 1], np.float32), (n, 1))


def _cloud(seed, n=600, lo=-4.0, hi=4.0):
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    a = rng.normal(size=(n, 3, 3))
    cov6 = vg.cov6_of(a @ a.transpose(0, 2, 1)).astype(np.float32)
    return xyz, cov6


def _same(a, b):
    return (np.array_equal(a.cells, b.cells) and np.array_equal(a.count, b.count) and vr.bits_equal(a.mean, b.mean) and vr.bits_equal(a.cov6, b.cov6)
            and np.array_equal(a.lex_keys, b.lex_keys) and np.array_equal(a.lex_row, b.lex_row) and vu.same_grid(a, b))


def test_on_the_clouds_own_grid_without_a_pose_it_is_build_map():
    xyz, cov6 = _cloud(1)
    a = vg.build_map(xyz, cov6, 0.7)
    b = vu.build_map_on_grid(xyz, cov6, 0.7, xyz.astype(np.float64).min(0))
    assert _same(a, b) and np.array_equal(a.cell_of_point, b.cell_of_point) and len(a.cells) > 100


def test_merge_commutes_bit_for_bit_and_is_not_associative_in_general():
    g = vu.centered_grid_min([0, 0, 0], 1.0)
    maps = [vu.build_map_on_grid(*_cloud(s), 1.0, g) for s in (2, 3, 4)]
    ab, ba = vu.merge(maps[0], maps[1]), vu.merge(maps[1], maps[0])
    assert _same(ab, ba)
    shared = len(maps[0].cells) + len(maps[1].cells) - len(ab.cells)
    assert shared > 50 and len(ab.cells) > len(maps[0].cells)
    left, right = vu.merge(ab, maps[2]), vu.merge(maps[0], vu.merge(maps[1], maps[2]))
    assert np.array_equal(left.cells, right.cells) and np.array_equal(left.count, right.count)       # the cells and the counts are associative ...
    assert not vr.bits_equal(left.mean, right.mean)                                                  # ... the rounded channels are not
    assert np.abs(left.mean.astype(np.float64) - right.mean).max() < 1e-5


def test_disjoint_maps_merge_to_their_morton_ordered_union():
    g = vu.centered_grid_min([0, 0, 0], 1.0)
    xa, ca = _cloud(5, lo=-4.0, hi=-0.1)
    xb, cb = _cloud(6, lo=0.1, hi=4.0)
    a, b = vu.build_map_on_grid(xa, ca, 1.0, g), vu.build_map_on_grid(xb, cb, 1.0, g)
    u = vu.merge(a, b)
    assert len(u.cells) == len(a.cells) + len(b.cells)
    mk = vr.morton3(u.cells)
    assert (mk[1:] > mk[:-1]).all()
    for part in (a, b):
        rows = u.lex_row[np.searchsorted(u.lex_keys, vr.cell_key(part.cells))]
        assert np.array_equal(u.cells[rows], part.cells) and np.array_equal(u.count[rows], part.count)
        assert vr.bits_equal(u.mean[rows], part.mean) and vr.bits_equal(u.cov6[rows], part.cov6)


def test_insert_with_the_identity_is_merge_with_the_map_on_the_grid():
    g = vu.centered_grid_min([0, 0, 0], 0.8)
    xa, ca = _cloud(7)
    xb, cb = _cloud(8)
    a = vu.build_map_on_grid(xa, ca, 0.8, g)
    assert _same(vu.insert(a, xb, cb, np.eye(4)), vu.merge(a, vu.build_map_on_grid(xb, cb, 0.8, g)))
    assert _same(vu.insert(a, xb, cb), vu.insert(a, xb, cb, np.eye(4)))
    # the identity leaves the members as they are, bit for bit
    p, c = vu.place(xb, cb, None)
    assert vr.bits_equal(p, xb) and vr.bits_equal(c, cb)


def test_a_merged_mean_stays_in_its_cell():
    g = vu.centered_grid_min([0, 0, 0], 1.0)
    u = vu.merge(vu.build_map_on_grid(*_cloud(9), 1.0, g), vu.build_map_on_grid(*_cloud(10), 1.0, g))
    assert np.array_equal(vr.cell_index(u.mean, u.origin, u.voxel), u.cells)


def test_remove_far_keeps_order_and_bits():
    g = vu.centered_grid_min([0, 0, 0], 1.0)
    m = vu.build_map_on_grid(*_cloud(11), 1.0, g)
    c = np.array([0.5, -0.25, 1.0])
    d2 = vu.distance2(m.mean, c)
    r = float(np.sqrt(np.median(d2)))
    k = vu.remove_far(m, c, r)
    keep = d2 < r * r
    assert 0.3 < keep.mean() < 0.7 and len(k.cells) == keep.sum()
    assert np.array_equal(k.cells, m.cells[keep]) and np.array_equal(k.count, m.count[keep])
    assert vr.bits_equal(k.mean, m.mean[keep]) and vr.bits_equal(k.cov6, m.cov6[keep])
    # strict: a row at exactly r goes
    exact = float(np.sqrt(d2.min()))
    if exact * exact == d2.min():
        with pytest.raises(ValueError, match="empty"):
            vu.remove_far(m, c, exact)
    with pytest.raises(ValueError, match="empty"):
        vu.remove_far(m, [1e4, 0, 0], 1.0)
    rows = vg.rows_at(k, m.mean, np.eye(4), 1)                 # the lookup arrays of the result work
    assert np.array_equal(rows[:, 0], np.nonzero(keep)[0]) and np.array_equal(rows[:, 1], np.arange(keep.sum()))


def test_counts_past_int32_are_refused():
    g = vu.centered_grid_min([0, 0, 0], 1.0)
    one = vu.build_map_on_grid(np.array([[0.2, 0.2, 0.2]], np.float32), _unit_cov6(1), 1.0, g)
    big = one
    for _ in range(30):
        big = vu.merge(big, big)
    assert big.count[0] == 2 ** 30 and vr.bits_equal(big.mean, one.mean)
    with pytest.raises(ValueError, match=r"2\^31 - 1"):
        vu.merge(big, big)
    almost = one
    for k in range(30):                                         # 2^30 - 1 = 1 + 2 + ... + 2^29 copies of the point
        almost = one if k == 0 else vu.merge(vu.merge(almost, almost), one)
    assert almost.count[0] == 2 ** 30 - 1 and vu.merge(big, almost).count[0] == 2 ** 31 - 1


def test_a_point_below_the_origin_is_refused():
    xyz, cov6 = _cloud(12)
    g = xyz.astype(np.float64).min(0)
    T = np.eye(4)
    T[1, 3] = -1.0
    with pytest.raises(vu.OutsideGrid):
        vu.build_map_on_grid(xyz, cov6, 1.0, g, T)
    with pytest.raises(vu.OutsideGrid):
        vu.insert(vu.build_map_on_grid(xyz, cov6, 1.0, g), xyz, cov6, T)


def test_condition_of_the_gpu_comparisons_on_pair_899(small_pair):
    """Pair 899 at voxel 0.3 (6897 / 7074 points), 1.0 m cells on the grid centred on the target's mean, the source placed at T_gicp: at least
    500 cells in both maps, 500 only in the target's and 500 only in the source's (measured when the feature was written: 1226 / 669 / 662 with
    1895 and 1888 rows), so a merge on the device copies, combines and interleaves hundreds of rows of each kind.  On the target's OWN grid
    the same placed source has a negative cell index (measured: -1 on y): the map of pcr_voxel_map_create cannot take it."""
    src = vr.voxel_reference(small_pair["source"], 0.3).points
    tgt = vr.voxel_reference(small_pair["target"], 0.3).points
    assert (len(src), len(tgt)) == (6897, 7074)
    g = vu.centered_grid_min(tgt.astype(np.float64).mean(0), 1.0)
    mt = vu.build_map_on_grid(tgt, _unit_cov6(len(tgt)), 1.0, g)
    ms = vu.build_map_on_grid(src, _unit_cov6(len(src)), 1.0, g, small_pair["T_gicp"])
    kt, ks = vr.cell_key(mt.cells), vr.cell_key(ms.cells)
    both = len(np.intersect1d(kt, ks))
    only_t, only_s = len(kt) - both, len(ks) - both
    print(f"pair 899 on the centred grid: {both} cells in both, {only_t} only in the target's, {only_s} only in the source's; rows {len(kt)} / {len(ks)}, "
          f"distinct counts {len(np.unique(mt.count))} / {len(np.unique(ms.count))}, largest {mt.count.max()} / {ms.count.max()}")
    assert both >= 500 and only_t >= 500 and only_s >= 500
    assert len(vu.merge(mt, ms).cells) == both + only_t + only_s
    assert (mt.cells.min() > 2 ** 20 - 200) and (mt.cells.max() < 2 ** 20 + 200)              # the grid is anchored 2^20 cells from its origin
    placed, _ = vu.place(src, _unit_cov6(len(src)), small_pair["T_gicp"])
    own = vr.cell_index(placed, vr.grid_origin(tgt, 1.0), 1.0)
    print(f"on the target's own grid the placed source spans cells {own.min(0).tolist()} .. {own.max(0).tolist()}")
    assert own.min() < 0
    with pytest.raises(vu.OutsideGrid):
        vu.insert(vg.build_map(tgt, _unit_cov6(len(tgt)), 1.0), src, _unit_cov6(len(src)), small_pair["T_gicp"])
