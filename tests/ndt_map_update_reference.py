"""Restatement of the rules by which a normal-distributions map grows (include/pcr_hip.h: RULE OF A MAP / MAP ON A GIVEN GRID, AT A POSE / MERGE /
INSERT / REMOVE_FAR of the NDT section) in numpy, on top of tests/voxel_map_update_reference.py (the grid, the placed members, the ordered
sums, the far test) and tests/ndt_reference.py (the member products, the information matrices, NdtMapRef).  It imports neither the package nor
a device.

  build_map_on_grid   the map of a cloud placed at a pose on the grid of a given grid_min
  merge               one row per cell of either map; a shared cell gets the counts' sum, the count-weighted mean, the covariances moved to that
                      mean by the parallel-axis term, and validity and A_v anew from (N, C)
  insert              merge(m, the map of the placed cloud on m's grid with m's rule)
  remove_far          the rows with d^2 < r^2, bits and order kept
Every function returns a GrownNdtMapRef, an NdtMapRef that also carries grid_min and the rule, so nd.rows_at, nd.linearize and nd.loop work
on it (cell_of_point is filled by build_map_on_grid only)."""
from dataclasses import dataclass

import numpy as np

import ndt_reference as nd
import voxel_map_update_reference as vu
import voxel_reference as vr

COUNT_MAX = vu.COUNT_MAX
OutsideGrid = vu.OutsideGrid
centered_grid_min = vu.centered_grid_min
distance2 = vu.distance2
CHANNELS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))          # (r, c) of xx, xy, xz, yy, yz, zz


@dataclass
class GrownNdtMapRef(nd.NdtMapRef):
    grid_min: np.ndarray = None    # (3,) float64
    min_points: int = 6
    ratio: float = 0.01


def _wrap(base, info, valid, clamped, grid_min, min_points, ratio):
    return GrownNdtMapRef(base.voxel, base.origin, base.cells, base.count, base.mean, base.cov6, info, valid, clamped, base.cell_of_point, base,
                          np.asarray(grid_min, np.float64).reshape(3).copy(), int(min_points), float(ratio))


def build_map_on_grid(xyz, voxel, grid_min, T=None, min_points=6, ratio=0.01):
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    origin = vu.grid_origin(grid_min, voxel)
    zeros = np.zeros((len(xyz), 6), np.float32)
    means = vu._build(xyz, zeros, voxel, origin, T)                                # the members placed, once for the means ...
    p = vu.place(xyz, zeros, T)[0]
    base = vu._build(p, nd.member_products(p, means.mean[means.cell_of_point]), voxel, origin, None)      # ... once with the six channels (p is placed already)
    assert np.array_equal(base.cells, means.cells) and np.array_equal(base.cell_of_point, means.cell_of_point) and vr.bits_equal(base.mean, means.mean)
    info, valid, clamped = nd.information(base.cov6, base.count, min_points, ratio)
    return _wrap(base, info, valid, clamped, grid_min, min_points, ratio)


def compatible(a, b):
    return (vu.same_grid(a, b) and np.asarray(a.grid_min, np.float64).tobytes() == np.asarray(b.grid_min, np.float64).tobytes()
            and int(a.min_points) == int(b.min_points) and np.float64(a.ratio).tobytes() == np.float64(b.ratio).tobytes())


def merged_cell(na, mean_a, cov_a, nb, mean_b, cov_b, parallel_axis=True):
    """(mean (k, 3) float32, C (k, 6) float32) of k cells held by both maps; parallel_axis=False drops the term (what a channel average would do)"""
    fa, fb = np.asarray(na, np.float64), np.asarray(nb, np.float64)
    fn = (np.asarray(na, np.int64) + np.asarray(nb, np.int64)).astype(np.float64)
    ma, mb = np.asarray(mean_a, np.float32).astype(np.float64), np.asarray(mean_b, np.float32).astype(np.float64)
    mean = ((fa[:, None] * ma + fb[:, None] * mb) / fn[:, None]).astype(np.float32)
    da, db = ma - mean.astype(np.float64), mb - mean.astype(np.float64)
    cov = np.zeros((len(fn), 6), np.float32)
    for t, (r, c) in enumerate(CHANNELS):
        Ma, Mb = np.asarray(cov_a, np.float32)[:, t].astype(np.float64), np.asarray(cov_b, np.float32)[:, t].astype(np.float64)
        if parallel_axis:
            Ma, Mb = Ma + da[:, r] * da[:, c], Mb + db[:, r] * db[:, c]
        cov[:, t] = ((fa * Ma + fb * Mb) / fn).astype(np.float32)
    return mean, cov


def merge(a, b, parallel_axis=True):
    if not compatible(a, b):
        raise ValueError("the maps are not compatible")
    ka, kb = vr.cell_key(a.cells), vr.cell_key(b.cells)
    keys = np.union1d(ka, kb)
    m = len(keys)
    ra, rb = np.full(m, -1, np.int64), np.full(m, -1, np.int64)
    ra[np.searchsorted(keys, ka)] = np.arange(len(ka))
    rb[np.searchsorted(keys, kb)] = np.arange(len(kb))
    both, only_a, only_b = (ra >= 0) & (rb >= 0), (ra >= 0) & (rb < 0), (ra < 0) & (rb >= 0)
    count, mean, cov6 = np.zeros(m, np.int64), np.zeros((m, 3), np.float32), np.zeros((m, 6), np.float32)
    info, valid, clamped = np.zeros((m, 3, 3)), np.zeros(m, bool), np.zeros(m, np.int64)
    for mask, src, rows in ((only_a, a, ra), (only_b, b, rb)):                     # a cell in only one map keeps its row bit for bit
        r = rows[mask]
        count[mask], mean[mask], cov6[mask], info[mask], valid[mask], clamped[mask] = src.count[r], src.mean[r], src.cov6[r], src.info[r], src.valid[r], src.clamped[r]
    na, nb = a.count[ra[both]], b.count[rb[both]]
    if len(na) and (na + nb).max() > COUNT_MAX:
        raise ValueError("the member count of a cell would pass 2^31 - 1")
    count[both] = na + nb
    mean[both], cov6[both] = merged_cell(na, a.mean[ra[both]], a.cov6[ra[both]], nb, b.mean[rb[both]], b.cov6[rb[both]], parallel_axis)
    info[both], valid[both], clamped[both] = nd.information(cov6[both], count[both], a.min_points, a.ratio)
    cells = np.stack([keys >> 42, (keys >> 21) & vr.MAX_INDEX, keys & vr.MAX_INDEX], 1)
    order = np.argsort(vr.morton3(cells), kind="stable")
    base = vu._map(a.voxel, a.origin, cells[order], count[order], mean[order], cov6[order])
    return _wrap(base, info[order], valid[order], clamped[order], a.grid_min, a.min_points, a.ratio)


def insert(m, xyz, T=None):
    return merge(m, build_map_on_grid(xyz, m.voxel, m.grid_min, T, m.min_points, m.ratio))


def remove_far(m, center, r):
    keep = distance2(m.mean, center) < float(r) * float(r)
    if not keep.any():
        raise ValueError("would leave the map empty")
    base = vu._map(m.voxel, m.origin, m.cells[keep], m.count[keep], m.mean[keep], m.cov6[keep])      # (Morton order already: the permutation is the identity)
    return _wrap(base, m.info[keep], m.valid[keep], m.clamped[keep], m.grid_min, m.min_points, m.ratio)


def lambda_max(m):
    """the largest eigenvalue of every cell's float64 S_v = C_v N_v / (N_v - 1) (0 for a cell of one member)"""
    from voxelized_gicp_reference import cov33_of
    n = m.count.astype(np.float64)
    out = np.zeros(len(n))
    big = m.count >= 2
    S = cov33_of(m.cov6)[big] * (n[big] / (n[big] - 1.0))[:, None, None]
    out[big] = np.linalg.eigvalsh(S).max(1)
    return out
