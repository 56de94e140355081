"""Restatement of the rules by which a voxel covariance map grows (include/pcr_hip.h: GRID / MAP ON A GIVEN GRID, AT A POSE / MERGE / INSERT /
REMOVE_FAR) in numpy, on top of tests/voxel_reference.py (cells, ordered sums) and tests/voxelized_gicp_reference.py (the pose expression,
the rotation of covariances, MapRef).  It imports neither the package nor a device.

  build_map_on_grid   the map of a cloud placed at a pose on the grid of a given grid_min
  merge               one row per cell of either map; a shared cell gets the counts' sum and the count-weighted channels
  insert              merge(m, the map of the placed cloud on m's grid)
  remove_far          the rows with d^2 < r^2, bits and order kept
Every function returns a MapRef whose lookup arrays are filled, so vg.rows_at and vg.loop work on it (cell_of_point is filled by
build_map_on_grid only)."""
import numpy as np

import voxel_reference as vr
import voxelized_gicp_reference as vg

COUNT_MAX = (1 << 31) - 1


class OutsideGrid(ValueError):
    """a member's cell index lies outside [0, 2^21) on some axis"""


def grid_origin(grid_min, voxel):
    return np.asarray(grid_min, np.float64).reshape(3) - float(voxel) * 0.5


def centered_grid_min(point, voxel):
    """the grid_min of a grid with `point` in the middle of its 2^21 cells per axis"""
    v = float(voxel)
    return np.floor(np.asarray(point, np.float64).reshape(3) / v) * v - float(1 << 20) * v


def place(xyz, cov6, T=None):
    """(p', C'): float32(T p) by the ROWS expression and float32((R C) R^T); none is the identity, applied all the same"""
    T = np.eye(4) if T is None else np.asarray(T, np.float64).reshape(4, 4)
    p = vg.transform(xyz, T).astype(np.float32)
    c33 = vg.cov33_of(np.ascontiguousarray(cov6, np.float32).reshape(-1, 6))
    return p, vg.cov6_of(vg.rotate_covariances(T[:3, :3], c33)).astype(np.float32)


def _map(voxel, origin, cells, count, mean, cov6, cell_of_point=None):
    """MapRef of rows given in any order: Morton order, lookup arrays filled"""
    cells = np.asarray(cells, np.int64).reshape(-1, 3)
    order = np.argsort(vr.morton3(cells), kind="stable")
    cells, count, mean, cov6 = cells[order], np.asarray(count, np.int64)[order], np.asarray(mean, np.float32)[order], np.asarray(cov6, np.float32)[order]
    lex = vr.cell_key(cells)
    by_lex = np.argsort(lex, kind="stable")
    if cell_of_point is not None:
        new_row = np.empty(len(order), np.int64)
        new_row[order] = np.arange(len(order))
        cell_of_point = new_row[cell_of_point]
    return vg.MapRef(float(voxel), np.asarray(origin, np.float64), cells, count, mean, cov6, cell_of_point, lex[by_lex], by_lex)


def _build(xyz, cov6, voxel, origin, T):
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    cov6 = np.ascontiguousarray(cov6, np.float32).reshape(-1, 6)
    assert len(xyz) == len(cov6) >= 1
    p, c = place(xyz, cov6, T)
    idx = vr.cell_index(p, origin, voxel)
    if idx.min() < 0 or idx.max() > vr.MAX_INDEX:
        raise OutsideGrid(f"cell indices {idx.min(0).tolist()} .. {idx.max(0).tolist()}")
    keys, label = np.unique(vr.cell_key(idx), return_inverse=True)
    label = label.reshape(-1)
    m = len(keys)
    count = np.bincount(label, minlength=m).astype(np.int64)
    cells = np.stack([keys >> 42, (keys >> 21) & vr.MAX_INDEX, keys & vr.MAX_INDEX], 1)
    div = count[:, None].astype(np.float64)
    mean = (vr.ordered_sums(p, label, m) / div).astype(np.float32)
    c6 = (vr.ordered_sums(c, label, m) / div).astype(np.float32)
    return _map(voxel, origin, cells, count, mean, c6, label)


def build_map_on_grid(xyz, cov6, voxel, grid_min, T=None):
    return _build(xyz, cov6, voxel, grid_origin(grid_min, voxel), T)


def same_grid(a, b):
    return np.float64(a.voxel).tobytes() == np.float64(b.voxel).tobytes() and np.asarray(a.origin, np.float64).tobytes() == np.asarray(b.origin, np.float64).tobytes()


def merge(a, b):
    if not same_grid(a, b):
        raise ValueError("the maps are not on the same grid")
    ka, kb = vr.cell_key(a.cells), vr.cell_key(b.cells)
    keys = np.union1d(ka, kb)
    m = len(keys)
    ra, rb = np.full(m, -1, np.int64), np.full(m, -1, np.int64)
    ra[np.searchsorted(keys, ka)] = np.arange(len(ka))
    rb[np.searchsorted(keys, kb)] = np.arange(len(kb))
    both, only_a, only_b = (ra >= 0) & (rb >= 0), (ra >= 0) & (rb < 0), (ra < 0) & (rb >= 0)
    count = np.zeros(m, np.int64)
    chan = np.zeros((m, 9), np.float32)
    ca, cb = np.concatenate([a.mean, a.cov6], 1), np.concatenate([b.mean, b.cov6], 1)
    count[only_a], chan[only_a] = a.count[ra[only_a]], ca[ra[only_a]]
    count[only_b], chan[only_b] = b.count[rb[only_b]], cb[rb[only_b]]
    na, nb = a.count[ra[both]], b.count[rb[both]]
    if len(na) and (na + nb).max() > COUNT_MAX:
        raise ValueError("the member count of a cell would pass 2^31 - 1")
    count[both] = na + nb
    fa, fb = na.astype(np.float64)[:, None], nb.astype(np.float64)[:, None]
    chan[both] = ((fa * ca[ra[both]].astype(np.float64) + fb * cb[rb[both]].astype(np.float64)) / (na + nb).astype(np.float64)[:, None]).astype(np.float32)
    cells = np.stack([keys >> 42, (keys >> 21) & vr.MAX_INDEX, keys & vr.MAX_INDEX], 1)
    return _map(a.voxel, a.origin, cells, count, chan[:, :3], chan[:, 3:])


def insert(m, xyz, cov6, T=None):
    return merge(m, _build(xyz, cov6, m.voxel, m.origin, T))


def distance2(mean, center):
    """d^2 in float64 from the float32 means: differences, squares and sums in the order x, y, z"""
    p = np.ascontiguousarray(mean, np.float32).astype(np.float64)
    c = np.asarray(center, np.float64).reshape(3)
    dx, dy, dz = p[:, 0] - c[0], p[:, 1] - c[1], p[:, 2] - c[2]
    return (dx * dx + dy * dy) + dz * dz


def remove_far(m, center, r):
    keep = distance2(m.mean, center) < float(r) * float(r)
    if not keep.any():
        raise ValueError("would leave the map empty")
    return _map(m.voxel, m.origin, m.cells[keep], m.count[keep], m.mean[keep], m.cov6[keep])
