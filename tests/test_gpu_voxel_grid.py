"""The voxel grid and the stable radix sort under it (pcr_cloud.hip, pcr_sort.hip) against tests/voxel_reference.py, for EQUALITY of float32
bits and of counts, on inputs whose voxel means depend on the order in which the members are added (order_sensitive_attribute: a sort
whose FIRST pass ranks lanes, rows, wavefronts or tiles in another order is still a sort, passes every comparison on real clouds and changes
these means; in a later pass the same mistake breaks the sorted order itself) and whose grid indices control every key bit (lattice_cloud):
  key widths    2 ... 21 bits per axis = 1 ... 8 radix passes, and 21 x 1 x 1 bits;
  sizes         around one row, one wavefront span and one tile of the sort, and 34 tiles (the second trip of the scan's eight-load loop);
  runs          one cell, two alternating cells, one cell of 5,000 members among singletons;
  the limit     index 2,097,151 is accepted on every axis, 2,097,152 raises "voxel_size is too small";
  colours       pcr_voxel_down_sample_ex with colours, and with normals and colours (two sorts that must agree row for row);
  merged passes pcr_dev_voxel_multi and pcr_dev_voxel_multi_batch against the one-scale pass, through pcr_debug_voxel_grids.
Device rows are matched to reference rows by the cell of the output point (voxel_reference.match_rows, which also asserts the Morton order
of the rows).  The condition that makes a comparison order-sensitive is asserted from the reference alone (voxel_reference.check_case_condition)."""
import ctypes as C

import numpy as np
import pytest

import voxel_reference as VR
from conftest import pkg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    return pkg()


def f32(a):
    return np.ascontiguousarray(a, np.float64).astype(np.float32)        # (PointCloud hands float32 values out as float64)


def down_sample(P, xyz, normals=None, colors=None, voxel=1.0):
    pc = P.PointCloud(xyz)
    if normals is not None:
        pc.normals = normals
    if colors is not None:
        pc.colors = colors
    out = pc.voxel_down_sample(voxel)
    return f32(out.points), (f32(out.normals) if normals is not None else None), (f32(out.colors) if colors is not None else None)


def assert_rows(ref, pts, attrs, what):
    """device rows (points, list of attribute means) == the reference's, bit for bit, row for row"""
    pos = VR.match_rows(ref, pts)
    assert VR.bits_equal(pts, ref.points[pos]), (what, "points")
    for k, a in enumerate(attrs):
        bad = (np.ascontiguousarray(a).view(np.uint32) != ref.attrs[k][pos].view(np.uint32)).any(1)
        assert a.shape == ref.points.shape and not bad.any(), (what, f"attribute {k}: {int(bad.sum())} of {len(bad)} voxel means differ")


def run_case(P, name):
    VR.check_case_condition(name)
    c = VR.case(name)
    pts, nrm, _ = down_sample(P, c.xyz, normals=c.attrs[0])
    assert_rows(VR.reference(name), pts, [nrm], name)


# ------------------------------------------------------------------------------------------------------- widths, sizes, runs
@pytest.mark.parametrize("name", [f"bits{b}" for b in VR.WIDTH_BITS] + ["aniso"])
def test_key_widths(P, name):
    run_case(P, name)


@pytest.mark.parametrize("name", [f"n{n}" for n in VR.SIZES] + ["tiles34"])
def test_sizes(P, name):
    run_case(P, name)


@pytest.mark.parametrize("name", ["one_cell", "two_cells", "big_cell"])
def test_runs_of_equal_keys(P, name):
    run_case(P, name)
    if name == "big_cell":
        assert VR.reference(name).count.max() == 5000 and (VR.reference(name).count == 1).sum() == VR.N_RUNS - 5000


# --------------------------------------------------------------------------------------------------------------- the limit
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_index_limit(P, axis):
    pts = np.zeros((2, 3), np.float32)
    pts[1, axis] = 2097151.0
    out, _, _ = down_sample(P, pts)
    ref = VR.voxel_reference(pts, 1.0)
    assert ref.cells[1, axis] == VR.MAX_INDEX
    assert_rows(ref, out, [], f"axis {axis}")
    assert VR.bits_equal(out, pts)
    pts[1, axis] = 2097152.0
    with pytest.raises(RuntimeError, match="voxel_size is too small"):
        down_sample(P, pts)


# ----------------------------------------------------------------------------------------------------------------- colours
def test_colours(P):
    VR.check_case_condition("colours")
    c = VR.case("colours"); ref = VR.reference("colours")
    nrm, col = c.attrs
    assert not np.array_equal(nrm, col)
    plain, _, _ = down_sample(P, c.xyz)
    only = VR.voxel_reference(c.xyz, 1.0, [col])
    pts, _, dc = down_sample(P, c.xyz, colors=col)
    assert_rows(only, pts, [dc], "colours only")
    assert VR.bits_equal(pts, plain)
    pts, dn, dc = down_sample(P, c.xyz, normals=nrm, colors=col)
    assert_rows(ref, pts, [dn, dc], "normals and colours")
    assert VR.bits_equal(pts, plain)


# ------------------------------------------------------------------------------------------------------------ merged passes
SENTINEL = -7.0


def voxel_grids(P, clouds, attrs, voxels, form):
    """pcr_debug_voxel_grids over `clouds` (one call) -> [cloud][scale] = (points, attribute means), or None when the pass declined
    (the output buffers are then asserted untouched)."""
    import torch
    ctx = P._lib.Context.current()
    m, S = len(clouds), len(voxels)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    dx = [up(p) for p in clouds]; da = [up(a) for a in attrs]
    ox = [torch.full((len(p), 3), SENTINEL, dtype=torch.float32, device="cuda") for p in clouds for _ in range(S)]
    oa = [torch.full((len(p), 3), SENTINEL, dtype=torch.float32, device="cuda") for p in clouds for _ in range(S)]
    ptr = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    out_n = (C.c_int32 * (m * S))(*([-1] * (m * S)))
    taken = C.c_int(-1)
    torch.cuda.synchronize()
    ctx.check(ctx.lib.pcr_debug_voxel_grids(ctx.handle, C.c_int(m), ptr(dx), ptr(da), (C.c_int64 * m)(*[len(p) for p in clouds]),
                                            (C.c_double * S)(*voxels), C.c_int(S), C.c_int(form), ptr(ox), ptr(oa), out_n, C.byref(taken)),
              "debug_voxel_grids")
    torch.cuda.synchronize()
    assert taken.value in (0, 1)
    if not taken.value:
        assert all((t == SENTINEL).all().item() for t in ox + oa) and all(v == -1 for v in out_n)
        return None
    out = []
    for c in range(m):
        row = []
        for s in range(S):
            k = c * S + s
            cnt = out_n[k]
            assert 1 <= cnt <= len(clouds[c])
            assert (ox[k][cnt:] == SENTINEL).all().item() and (oa[k][cnt:] == SENTINEL).all().item()      # nothing past the count
            row.append((ox[k][:cnt].cpu().numpy(), oa[k][:cnt].cpu().numpy()))
        out.append(row)
    return out


def assert_same_grids(a, b, what):
    assert len(a) == len(b)
    for c, (ra, rb) in enumerate(zip(a, b)):
        for s, ((pa, aa), (pb, ab)) in enumerate(zip(ra, rb)):
            assert VR.bits_equal(pa, pb) and VR.bits_equal(aa, ab), (what, "cloud", c, "scale", s, len(pa), len(pb))


def assert_grids_are_reference(names, voxels, got, what):
    for c, name in enumerate(names):
        for s, v in enumerate(voxels):
            assert_rows(VR.reference(name, v), got[c][s][0], [got[c][s][1]], (what, name, v))


@pytest.mark.parametrize("name", ["merged6", "merged11"])
@pytest.mark.parametrize("voxels", [(1.0, 2.0, 4.0), VR.LATTICE10], ids=["1-2-4", "5-4-3-2-1"])
def test_all_scales_of_a_cloud_in_one_pass(P, name, voxels):
    VR.check_case_condition(name)
    c = VR.case(name)
    one = voxel_grids(P, [c.xyz], [c.attrs[0]], voxels, 0)
    multi = voxel_grids(P, [c.xyz], [c.attrs[0]], voxels, 1)
    assert one is not None and multi is not None
    assert_grids_are_reference([name], voxels, one, "one-scale pass")
    assert_grids_are_reference([name], voxels, multi, "merged pass")
    assert_same_grids(multi, one, name)


def test_scale_index_above_63_morton_bits(P):
    """Two scales: shift + 1 = 64 key bits, the pass is taken.  Three scales: the index does not fit, the pass declines and writes nothing."""
    VR.check_case_condition("merged63")
    c = VR.case("merged63")
    assert tuple(VR.reference("merged63").cells.max(0)) == (VR.MAX_INDEX,) * 3
    two = voxel_grids(P, [c.xyz], [c.attrs[0]], (1.0, 2.0), 1)
    assert two is not None
    assert_grids_are_reference(["merged63"], (1.0, 2.0), two, "merged pass, 64 key bits")
    assert voxel_grids(P, [c.xyz], [c.attrs[0]], (1.0, 2.0, 4.0), 1) is None
    assert voxel_grids(P, [c.xyz], [c.attrs[0]], (1.0, 2.0, 4.0), 2) is None
    one = voxel_grids(P, [c.xyz], [c.attrs[0]], (1.0, 2.0, 4.0), 0)
    assert_grids_are_reference(["merged63"], (1.0, 2.0, 4.0), one, "one-scale pass")
    assert_same_grids([two[0][:2]], [one[0][:2]], "merged63")


@pytest.mark.parametrize("count", [2, 8])
def test_all_clouds_of_a_group_in_one_pass(P, count):
    """count = 2: argument structs by value; count = 8: through device memory.  Clouds of different sizes and extents: every cloud has its
    own Morton width (shift) under the group's shared number of sort passes."""
    names = [f"group{k}" for k in range(count)]
    voxels = (1.0, 2.0, 4.0)
    for nm in names:
        VR.check_case_condition(nm)
    clouds = [VR.case(nm).xyz for nm in names]; attrs = [VR.case(nm).attrs[0] for nm in names]
    assert len({len(p) for p in clouds}) == count and max(len(p) for p in clouds) <= VR.N3
    assert len({tuple(VR.case(nm).top) for nm in names}) >= count - 1
    one = voxel_grids(P, clouds, attrs, voxels, 0)
    batch = voxel_grids(P, clouds, attrs, voxels, 2)
    assert one is not None and batch is not None
    assert_grids_are_reference(names, voxels, one, "one-scale pass")
    assert_same_grids(batch, one, f"group of {count}")
    per_cloud = voxel_grids(P, clouds, attrs, voxels, 1)
    assert_same_grids(per_cloud, one, f"cloud by cloud, {count}")


def test_hook_rejects_bad_arguments(P):
    VR.check_case_condition("n64")
    c = VR.case("n64")
    with pytest.raises(RuntimeError):
        voxel_grids(P, [c.xyz], [c.attrs[0]], (1.0,), 3)
    assert voxel_grids(P, [c.xyz], [c.attrs[0]], (1.0,), 1) is None            # a single scale has nothing to merge
    one = voxel_grids(P, [c.xyz], [c.attrs[0]], (1.0,), 0)
    assert_grids_are_reference(["n64"], (1.0,), one, "one scale")
