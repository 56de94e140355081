"""Scan Context on the device against the numpy restatement of the rule (tests/scan_context_reference.py; the rule: include/pcr_hip.h).
Equality throughout, compared as integer views of the bits: descriptors and row counts of LiDAR scans at four parameter sets, of a hand-made
cloud of rows on every bin boundary and of the smallest clouds; distances and shifts of square and rectangular blocks, of the extreme shapes
and of descriptors whose shifts tie; the loop closures and queries of the database against the same selection made from the restatement's
matrix; the errors of the two entry points; and one registration started from a detected closure."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import scan_context_reference as sc
from conftest import GOLDEN, TOL_M, TOL_RAD, golden_pair_files, pkg, pose_error

pytestmark = pytest.mark.gpu

# (num_rings, num_sectors, max_range, height_offset)
PARAMS = [sc.DEFAULTS, (8, 16, 30.0, 0.0), (40, 120, 45.0, 2.0), (1, 4, 80.0, 2.0)]


@pytest.fixture(scope="module")
def P():
    return pkg()


@pytest.fixture(scope="module")
def source_899():
    return np.load(os.path.join(GOLDEN, "nclt_pair_899.npz"))["source"]


@pytest.fixture(scope="module")
def golden_scans():
    clouds = []
    for f in golden_pair_files():
        d = np.load(f)
        clouds += [d["source"], d["target"]]
    return clouds


@pytest.fixture(scope="module")
def golden_reference(golden_scans):
    """descriptors of the 16 scans at the defaults and their full distance block, from the restatement; computed once and left unchanged"""
    descs = np.stack([sc.descriptor(c)[0] for c in golden_scans])
    dist, shift = sc.distance_block(descs, descs)
    for a in (descs, dist, shift):
        a.setflags(write=False)
    return descs, dist, shift


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def assert_same_bits(dev, ref, what=""):
    dev, ref = np.asarray(dev), np.asarray(ref)
    assert dev.dtype == ref.dtype and dev.shape == ref.shape, (what, dev.dtype, ref.dtype, dev.shape, ref.shape)
    bad = bits(dev) != bits(ref)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:5].tolist(), dev[bad][:5], ref[bad][:5])


def device_descriptor(P, cloud, params):
    d, info = P.scan_context(np.asarray(cloud, dtype=np.float32).reshape(-1, 3), *params, return_info=True)
    return d.cpu().numpy(), info


def check_descriptor(P, cloud, params, what=""):
    dev, info = device_descriptor(P, cloud, params)
    ref, ref_info = sc.descriptor(cloud, *params)
    assert_same_bits(dev, ref, what)
    assert info == ref_info, (what, info, ref_info)
    return ref, ref_info


def device_distance(P, A, B):
    dist, shift = P.scan_context_distance(np.asarray(A), np.asarray(B))
    return dist.cpu().numpy(), shift.cpu().numpy()


def check_distance(P, A, B, what=""):
    dist, shift = device_distance(P, A, B)
    rd, rs = sc.distance_block(A, B)
    assert_same_bits(dist, rd, what)
    assert np.array_equal(shift, rs) and shift.dtype == np.int32, (what, shift, rs)
    return rd, rs


# ------------------------------------------------------------------------------------------------- descriptor
@pytest.mark.parametrize("params", PARAMS, ids=lambda p: "R%d-S%d-L%g-h%g" % p)
def test_descriptor_of_a_scan(P, source_899, params):
    ref, info = check_descriptor(P, source_899, params)
    assert info["used"] + info["dropped_range"] == 16526
    if params == PARAMS[1]:
        assert info["dropped_range"] == 1912                         # the 30 m range drops rows (12 % of them)
    assert (ref != 0).any()


def boundary_cloud():
    """rows on every boundary of the rule; z varies so that a row in the wrong cell shows"""
    rows = []
    for r in (0.5, 3.0, 4.0, 7.999, 8.0, 36.0, 76.0, 79.99):                         # the four axes, at ring bounds too
        rows += [(r, 0, 1), (0, r, 2), (-r, 0, 3), (0, -r, 4), (r, -0.0, 5), (-0.0, r, 6)]
    for r in (1.0, 5.0, 30.0):                                                        # 45 degrees: a sector bound at S = 8
        rows += [(r, r, 1.5), (-r, r, 2.5), (-r, -r, 3.5), (r, -r, 4.5)]
    for k in range(1, 21):                                                            # rho exactly 4 k (3-4-5 triangles): ring bounds at L = 80, R = 20
        rows += [(4.0 * k, 0, 0.1 * k), (2.4 * k, 3.2 * k, -0.1 * k), (0, -4.0 * k, 0.2 * k)]
    rows += [(80, 0, 9), (0, 80, 9), (48, 64, 9), (0, 0, 9), (0, 0, -9), (-0.0, 0.0, 1)]     # rho exactly L, the origin
    rows += [(np.nan, 1, 1), (1, np.inf, 1), (1, 1, -np.inf), (np.nan, np.nan, np.nan)]
    rows += [(10, 10, -2.0), (-10, 10, -0.0), (-10, -10, -5.0), (-10, -10.5, -7.0), (10, -10, -2.0), (10.1, -10, -3.0)]   # z = -h, z = -0.0, negative cells
    a = np.array(rows, dtype=np.float32)
    k = np.arange(1, 200, dtype=np.float64)                                           # and rows next to every default sector bound
    ang = 2.0 * math.pi * (k % 60) / 60
    near = np.stack([20 * np.cos(ang), 20 * np.sin(ang), 0.01 * k], axis=1).astype(np.float32)
    return np.concatenate([a, near, np.nextafter(near, np.float32(0)), np.nextafter(near, np.float32(100))])


@pytest.mark.parametrize("params", [sc.DEFAULTS, (20, 8, 80.0, 2.0), (20, 60, 80.0, 0.0), (64, 128, 80.0, -1.0)], ids=lambda p: "R%d-S%d-L%g-h%g" % p)
def test_descriptor_of_boundary_rows(P, params):
    cloud = boundary_cloud()
    ref, info = check_descriptor(P, cloud, params)
    assert info["dropped_nonfinite"] == 4 and info["dropped_range"] >= 6
    assert not np.signbit(ref[ref == 0]).any()                        # -0.0 is never stored
    if params[3] == 0.0:
        assert (ref < 0).any()                                        # cells whose rows are all below the sensor keep their negative maximum


def test_descriptor_of_many_rows_in_one_cell(P):
    rng = np.random.default_rng(5)
    cloud = np.stack([10.0 + 0.5 * rng.random(5000), 0.2 + 0.1 * rng.random(5000), rng.normal(0, 3, 5000)], axis=1).astype(np.float32)
    ref, info = check_descriptor(P, cloud, sc.DEFAULTS)
    assert info["used"] == 5000 and (ref != 0).sum() == 1
    ref, _ = check_descriptor(P, -np.abs(cloud), sc.DEFAULTS)          # every value negative before the offset
    assert (ref != 0).sum() == 1


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_descriptor_of_small_clouds(P, source_899, n):
    ref, info = check_descriptor(P, source_899[:n], sc.DEFAULTS)
    assert info["used"] == n
    if n == 0:
        assert not ref.any()
    dev, _ = device_descriptor(P, source_899[5000:5000 + n], PARAMS[1])
    assert_same_bits(dev, sc.descriptor(source_899[5000:5000 + n], *PARAMS[1])[0])


# ------------------------------------------------------------------------------------------------- distance
def test_distance_block_of_the_golden_scans(P, golden_scans, golden_reference):
    descs, dist, shift = golden_reference
    dev = np.stack([device_descriptor(P, c, sc.DEFAULTS)[0] for c in golden_scans])
    assert_same_bits(dev, descs)
    d, s = device_distance(P, descs, descs)
    assert_same_bits(d, dist)
    assert np.array_equal(s, shift)
    for ra, rb in ((slice(3, 4), slice(0, 16)), (slice(0, 16), slice(7, 8)), (slice(2, 5), slice(9, 14))):      # 1 x 16, 16 x 1, 3 x 5
        d, s = device_distance(P, descs[ra], descs[rb])
        assert_same_bits(d, dist[ra, rb])
        assert np.array_equal(s, shift[ra, rb])
    d2, s2 = device_distance(P, descs, descs)                          # the same bits on every run
    d, s = device_distance(P, descs, descs)
    assert_same_bits(d, d2)
    assert np.array_equal(s, s2)


@pytest.mark.parametrize("params", PARAMS[1:], ids=lambda p: "R%d-S%d" % p[:2])
def test_distance_at_other_shapes(P, golden_scans, params):
    descs = np.stack([sc.descriptor(c, *params)[0] for c in golden_scans[:3]])
    rd, rs = check_distance(P, descs, descs[::-1])
    if params[0] == 1:                                                 # one ring: every cosine is +-1 and, all heights positive, every shift ties
        assert (rs == 0).all()


def test_distance_at_the_largest_shape(P):
    rng = np.random.default_rng(11)
    descs = rng.normal(1.0, 2.0, (3, 64, 128)).astype(np.float32)
    descs[rng.random(descs.shape) < 0.3] = 0
    descs[0][:, 5:9] = 0
    check_distance(P, descs[:2], descs[1:])


def test_distance_of_degenerate_descriptors(P, golden_reference):
    descs = golden_reference[0]
    R, S = descs.shape[1:]
    zero = np.zeros((1, R, S), np.float32)
    d, s = device_distance(P, zero, descs[:5])
    assert (d == 1.0).all() and (s == 0).all()
    d, s = device_distance(P, descs[:5], zero)
    assert (d == 1.0).all() and (s == 0).all()
    check_distance(P, np.concatenate([zero, descs[:2]]), np.concatenate([descs[3:4], zero]))
    sparse = descs[:3].copy()
    sparse[:, :, 10:50] = 0                                            # 40 of 60 columns empty
    check_distance(P, sparse, descs[:4])
    check_distance(P, descs[:4], sparse)
    equal = np.repeat(descs[0][:, 7:8], S, axis=1)[None]              # equal columns: all shifts tie, the smallest wins
    rd, rs = check_distance(P, equal, np.concatenate([equal, descs[:2]]))
    assert rs[0, 0] == 0 and rd[0, 0] == 0.0
    half = np.concatenate([descs[1][:, :S // 2], descs[1][:, :S // 2]], axis=1)[None]   # period S / 2: shifts n and n + S / 2 tie
    rd, rs = check_distance(P, half, np.concatenate([np.roll(half, 7, axis=2), np.roll(half, S // 2 + 3, axis=2), half]))
    assert rs.tolist() == [[S // 2 - 7, S // 2 - 3, 0]] and (rd == 0.0).all()


# ------------------------------------------------------------------------------------------------- database
@pytest.fixture(scope="module")
def database(P, golden_scans):
    db = P.ScanContextDatabase()
    assert db.extend(golden_scans[:10]) == list(range(10))
    assert [db.add(c) for c in golden_scans[10:]] == list(range(10, 16))
    yield db
    db.close()


def test_database_rows(P, database, golden_reference):
    descs, dist, shift = golden_reference
    assert len(database) == 16 and tuple(database.descriptors.shape) == (16, 20, 60)
    assert_same_bits(database.descriptors.cpu().numpy(), descs)
    d, s = database.distances()
    assert_same_bits(d.cpu().numpy(), dist)
    d, s = database.distances(rows_a=[5, 2, 11], rows_b=slice(4, 9))
    assert_same_bits(d.cpu().numpy(), dist[[5, 2, 11], 4:9])
    assert np.array_equal(s.cpu().numpy(), shift[[5, 2, 11], 4:9])


@pytest.mark.parametrize("block_rows", [256, 5])
@pytest.mark.parametrize("max_distance", [0.4, 2.0])
@pytest.mark.parametrize("top_k", [1, 3])
@pytest.mark.parametrize("exclude_recent", [0, 3])
def test_detect_loop_closures(P, database, golden_reference, exclude_recent, top_k, max_distance, block_rows, monkeypatch):
    _, dist, shift = golden_reference
    monkeypatch.setattr(database, "BLOCK_ROWS", block_rows)
    rows, ds = database.detect_loop_closures(max_distance, exclude_recent=exclude_recent, top_k=top_k)
    ref_rows, ref_ds = sc.loop_closures(dist, shift, max_distance, exclude_recent, top_k)
    assert rows.dtype == np.int64 and ds.dtype == np.float64
    assert np.array_equal(rows, ref_rows), (rows, ref_rows)
    assert_same_bits(ds, ref_ds)
    if max_distance == 0.4:
        assert [tuple(r[:2]) for r in rows] == ([(2 * k + 1, 2 * k) for k in range(8)] if exclude_recent == 0 else [])


@pytest.mark.parametrize("top_k", [1, 3, 40])
def test_query(P, database, golden_scans, golden_reference, top_k):
    descs, dist, shift = golden_reference
    for q in (0, 9):
        order = sorted(range(16), key=lambda j: (dist[q, j], j))[:top_k]
        for query in (golden_scans[q], descs[q]):                       # a cloud, and its descriptor
            idx, d, s = database.query(query, top_k=top_k)
            assert idx.tolist() == order
            assert_same_bits(d, dist[q, order])
            assert s.tolist() == shift[q, order].tolist()
    rows = [12, 3, 8, 9]
    order = sorted(rows, key=lambda j: (dist[9, j], j))[:top_k]
    idx, d, s = database.query(descs[9], top_k=top_k, rows=rows)
    assert idx.tolist() == order and s.tolist() == shift[9, order].tolist()
    assert_same_bits(d, dist[9, order])


# ------------------------------------------------------------------------------------------------- errors
def _raw_descriptor(P, n=4, R=20, S=60, L=80.0, h=2.0, L2=None, null=()):
    import torch
    ctx = P._lib.Context.current()
    xyz = torch.ones((max(n, 1), 3), dtype=torch.float32, device="cuda")
    out = torch.full((64 * 128,), -7.0, dtype=torch.float32, device="cuda")
    rb, ck, sk, r2 = sc.tables(min(max(R, 1), 64), min(max(S - S % 4, 4), 128), L if math.isfinite(L) and L > 0 else 1.0)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    params = P._lib.PcrScanContextParams(R, S, L, h)
    tables = P._lib.PcrScanContextTables(None if "ring_bound2" in null else dp(rb), None if "cos_k" in null else dp(ck), None if "sin_k" in null else dp(sk),
                                         r2 if L2 is None else L2)
    rc = ctx.lib.pcr_scan_context(ctx.handle, None if "xyz" in null else C.c_void_p(xyz.data_ptr()), C.c_int64(n), None if "params" in null else C.byref(params),
                                  None if "tables" in null else C.byref(tables), None if "out" in null else C.c_void_p(out.data_ptr()), None)
    torch.cuda.synchronize()
    return rc, (ctx.lib.pcr_last_error(ctx.handle) or b"").decode(), bool((out == -7.0).all().item())


BAD_DESCRIPTOR = [dict(null=("xyz",)), dict(null=("params",)), dict(null=("tables",)), dict(null=("out",)), dict(null=("ring_bound2",)), dict(null=("cos_k",)),
                  dict(null=("sin_k",)), dict(R=0), dict(R=65), dict(S=0), dict(S=132), dict(S=6), dict(S=62), dict(L=0.0), dict(L=-1.0), dict(L=float("inf")),
                  dict(L=float("nan")), dict(L2=0.0), dict(L2=float("nan")), dict(h=float("nan")), dict(h=float("inf")), dict(n=-1)]


@pytest.mark.parametrize("bad", BAD_DESCRIPTOR, ids=[",".join(f"{k}={v}" for k, v in b.items()) for b in BAD_DESCRIPTOR])
def test_descriptor_errors(P, bad):
    rc, msg, untouched = _raw_descriptor(P, **bad)
    assert rc == P._lib.PCR_EINVAL and "scan_context" in msg and untouched, (rc, msg, untouched)


def test_descriptor_accepts_what_is_not_an_error(P):
    assert _raw_descriptor(P)[0] == P._lib.PCR_OK
    rc, _, untouched = _raw_descriptor(P, n=0, null=("xyz",))           # no rows: no cloud needed, the descriptor is zeroed
    assert rc == P._lib.PCR_OK and not untouched
    assert _raw_descriptor(P, R=1, S=4, null=("ring_bound2", "cos_k", "sin_k"))[0] == P._lib.PCR_OK


def _raw_distance(P, nA=2, nB=3, R=20, S=60, null=()):
    import torch
    ctx = P._lib.Context.current()
    A = torch.ones((max(nA, 1) * 64 * 128,), dtype=torch.float32, device="cuda")
    B = torch.ones((max(nB, 1) * 64 * 128,), dtype=torch.float32, device="cuda")
    dist = torch.full((max(nA, 1) * max(nB, 1),), -7.0, dtype=torch.float64, device="cuda")
    shift = torch.full((max(nA, 1) * max(nB, 1),), -7, dtype=torch.int32, device="cuda")
    p = lambda name, t: None if name in null else C.c_void_p(t.data_ptr())
    rc = ctx.lib.pcr_scan_context_distance(ctx.handle, p("A", A), C.c_int64(nA), p("B", B), C.c_int64(nB), C.c_int(R), C.c_int(S), p("dist", dist), p("shift", shift))
    torch.cuda.synchronize()
    return rc, (ctx.lib.pcr_last_error(ctx.handle) or b"").decode(), bool((dist == -7.0).all().item() and (shift == -7).all().item())


BAD_DISTANCE = [dict(null=("A",)), dict(null=("B",)), dict(null=("dist",)), dict(null=("shift",)), dict(R=0), dict(R=65), dict(S=0), dict(S=132), dict(S=6),
                dict(S=62), dict(nA=-1), dict(nB=-1)]


@pytest.mark.parametrize("bad", BAD_DISTANCE, ids=[",".join(f"{k}={v}" for k, v in b.items()) for b in BAD_DISTANCE])
def test_distance_errors(P, bad):
    rc, msg, untouched = _raw_distance(P, **bad)
    assert rc == P._lib.PCR_EINVAL and "scan_context_distance" in msg and untouched, (rc, msg, untouched)


def test_distance_of_empty_blocks_writes_nothing(P):
    for kw in (dict(nA=0), dict(nB=0), dict(nA=0, nB=0, null=("A", "B", "dist", "shift"))):
        rc, _, untouched = _raw_distance(P, **kw)
        assert rc == P._lib.PCR_OK and untouched
    rc, _, untouched = _raw_distance(P)
    assert rc == P._lib.PCR_OK and not untouched
    db = P.ScanContextDatabase()
    d, s = db.distances()
    assert tuple(d.shape) == (0, 0) and tuple(s.shape) == (0, 0)


# ------------------------------------------------------------------------------------------------- end to end
def test_registration_from_a_detected_closure(P, source_899):
    """The target is the source turned by 36 degrees about z (rounded to float32): the database finds the closure with shift 6, and the default
    registration of loop_closure_edges, started at Rz(36 degrees), stays there: only the float32 rounding of the turned points moves it."""
    turned = sc.rotate_z(source_899, 36.0)
    with P.ScanContextDatabase() as db:
        db.extend([source_899, turned])
        closures, dist = db.detect_loop_closures(0.4, exclude_recent=0)
    assert closures.tolist() == [[1, 0, 6]] and dist.tolist() == [0.0]
    clouds = [P.PointCloud(source_899), P.PointCloud(turned)]
    edges = P.loop_closure_edges(clouds, closures, 0.1)
    assert len(edges) == 1
    e = edges[0]
    assert (e.source_node_id, e.target_node_id, e.uncertain) == (0, 1, True)
    truth = P.shift_to_transformation(6, 60)
    ang, dt = pose_error(e.transformation, truth)
    print(f"closure edge against Rz(36 deg): {ang:.2e} rad, {dt:.2e} m")
    assert ang < TOL_RAD and dt < TOL_M, (ang, dt)
    assert e.information.shape == (6, 6) and e.information[5, 5] > 0
    g = P.pose_graph_from_odometry(clouds, [np.identity(4), np.linalg.inv(truth)], closures, voxel_size=0.1)
    assert len(g.nodes) == 2 and [(x.source_node_id, x.target_node_id, x.uncertain) for x in g.edges] == [(0, 1, False), (0, 1, True)]
