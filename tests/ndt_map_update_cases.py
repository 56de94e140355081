"""The hand-made maps that tests/test_ndt_map_update_api.py (their condition, on the restatement alone) and tests/test_gpu_ndt_map_update.py (device
against restatement) share: the cell patterns of tests/test_gpu_voxel_map_update.py -- one cell, a neighbour below and above, maps wholly below
and above each other, interleaved maps across the top key bit, and 255 / 256 / 257 rows on each side (the block-size edge of a 256-lane kernel) --
filled with 1 to 8 points per cell of three kinds, so that a merge meets cells that become valid only through it, cells that stay invalid,
planar cells (a clamped eigenvalue) and cells of coincident points.  Voxel 1.0 on the grid centred on (0, 0, 0)."""
import numpy as np

import voxel_map_update_reference as vu
import voxel_reference as vr

MID = 1 << 20                        # the cell of the point (0, 0, 0) on the grid centred on it
GRID0 = vu.centered_grid_min([0.0, 0.0, 0.0], 1.0)
MIN_POINTS = 6


def kind_of(cells):
    """0: every member at one point that depends on the cell alone (so two maps agree on it); 1: members on one plane z = const of the cell; else: anywhere"""
    c = np.asarray(cells, np.int64).reshape(-1, 3)
    return (c[:, 0] + 2 * c[:, 1] + 3 * c[:, 2]) % 5


def cell_cloud(cells, seed, counts=None):
    """float32 points, 1 to 8 (or counts[k]) in each of the given cells, in a shuffled order"""
    rng = np.random.default_rng(seed)
    cells = np.asarray(cells, np.int64).reshape(-1, 3)
    counts = rng.integers(1, 9, len(cells)) if counts is None else np.asarray(counts, np.int64)
    cop = np.repeat(cells, counts, 0)
    kind = kind_of(cop)
    off = rng.uniform(-0.4, 0.4, cop.shape)
    off[kind == 1, 2] = 0.125
    off[kind == 0] = [0.25, 0.125, -0.375]
    xyz = ((cop - MID).astype(np.float64) + off).astype(np.float32)
    return xyz[rng.permutation(len(xyz))]


def block(nx, ny, nz, lo=(MID, MID, MID)):
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 3)
    return g + np.asarray(lo, np.int64)


def _boundary_case(n):
    """n rows on each side; the first and the last cell of the union (in Morton order) are in both, the cells between alternate"""
    pool = block(9, 8, 8)
    pool = pool[np.argsort(vr.morton3(pool))][:2 * n - 2]
    ends, mid = pool[[0, -1]], pool[1:-1]
    return np.concatenate([ends, mid[0::2]]), np.concatenate([ends, mid[1::2]])


def _interleaved():
    rng = np.random.default_rng(40)
    pool = block(6, 6, 6, (MID - 3, MID - 3, MID - 3))              # straddles the top key bit on every axis
    pick = rng.random((2, len(pool))) < 0.5
    return pool[pick[0]], pool[pick[1]]


C0 = np.array([[MID + 2, MID + 1, MID + 3]])                         # a cell whose members lie anywhere in it
assert kind_of(C0)[0] >= 2
MERGE_CASES = {
    "same_cell": lambda: (C0, C0),
    "lower_cell": lambda: (C0, C0 - [1, 0, 0]),
    "higher_cell": lambda: (C0, C0 + [1, 0, 0]),
    "wholly_below": lambda: (block(4, 3, 3), block(4, 3, 3, (MID - 4, MID, MID))),      # the top bit of x is clear in every cell of `other`
    "wholly_above": lambda: (block(4, 3, 3, (MID - 4, MID, MID)), block(4, 3, 3)),
    "interleaved": _interleaved,
    "rows255": lambda: _boundary_case(255),
    "rows256": lambda: _boundary_case(256),
    "rows257": lambda: _boundary_case(257),
}


def merge_case(name):
    """(cells of A, cells of B, points of A, points of B); in "same_cell" A holds 5 points and B 1: valid only through the merge"""
    ca, cb = MERGE_CASES[name]()
    if name == "same_cell":
        return ca, cb, cell_cloud(ca, 50, [MIN_POINTS - 1]), cell_cloud(cb, 51, [1])
    return ca, cb, cell_cloud(ca, 50), cell_cloud(cb, 51)
