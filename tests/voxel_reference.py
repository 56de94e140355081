"""Restatement of the voxel grid rule (DESIGN.md "voxel"; PointCloud.voxel_down_sample) in numpy, the inputs that make its member order
visible, and the table of cases that tests/test_gpu_voxel_grid.py runs and tests/test_voxel_reference.py qualifies on the CPU.

The rule, in float64 on the float32 coordinates:
  origin = min - voxel / 2                 per axis
  index  = floor((p - origin) / voxel)     per axis; a voxel is one (ix, iy, iz)
  mean   = (sum of the members IN INPUT ORDER) / count, then rounded to float32 -- for the points and for every attribute
Rows are keyed by (ix, iy, iz) and listed in lexicographic order of it (the oracle's order).  Nothing here imports the package or the oracle.

Why the inputs are special: a float64 sum of float32 values of similar size is exact in ANY order, so equality with a reference says nothing
about member order on real clouds or on random attributes.  ``order_sensitive_attribute`` deals exactly cancelling pairs +A, -A
(A = (1 + u) 2^e, e in [60, 100)) and small values 1 + u to the members of every voxel: a small value added while the running sum holds an A
is absorbed, so what survives depends on the order.  ``order_sensitivity`` measures that on the reference alone, and ``assert_condition`` is
the CONDITION of every comparison that uses the attribute (not a tolerance: everything compared with the device is compared for equality):
reversing the member order changes the float32 mean (of any channel) in >= 90 % of the voxels with three or more members, and at least half
of the voxels have three or more members."""
import functools
from dataclasses import dataclass, field

import numpy as np

MAX_INDEX = (1 << 21) - 1          # largest voxel index per axis that the device accepts (21 Morton bits per axis)


# ------------------------------------------------------------------------------------------------------------------ the rule
def grid_origin(xyz, voxel):
    p = np.ascontiguousarray(xyz, np.float32).astype(np.float64).reshape(-1, 3)
    return p.min(0) - float(voxel) * 0.5


def cell_index(xyz, origin, voxel):
    """(ix, iy, iz) int64 of every row of `xyz` (float32 values) on the grid (origin, voxel)."""
    p = np.ascontiguousarray(xyz, np.float32).astype(np.float64).reshape(-1, 3)
    return np.floor((p - origin) / float(voxel)).astype(np.int64)


def cell_key(idx):
    """one int64 per cell, ascending = lexicographic in (ix, iy, iz); indices must fit 21 bits"""
    idx = np.asarray(idx, np.int64).reshape(-1, 3)
    assert idx.size == 0 or (idx.min() >= 0 and idx.max() <= MAX_INDEX), (idx.min(), idx.max())
    return (idx[:, 0] << 42) | (idx[:, 1] << 21) | idx[:, 2]


def ordered_sums(values, label, m):
    """sums[v] = float64 sum of values[i] over label[i] == v, added one by one in the order of i (np.add.at is unbuffered and sequential)"""
    s = np.zeros((m, values.shape[1]), np.float64)
    np.add.at(s, label, np.asarray(values, np.float64))
    return s


@dataclass
class VoxelRef:
    voxel: float
    origin: np.ndarray             # (3,) float64
    cells: np.ndarray              # (m, 3) int64, lexicographic
    keys: np.ndarray               # (m,) int64 = cell_key(cells), ascending
    count: np.ndarray              # (m,) int64
    points: np.ndarray             # (m, 3) float32
    attrs: list                    # of (m, 3) float32, one per input attribute
    cell_of_point: np.ndarray      # (n,) row of `cells` of every input point


def voxel_reference(xyz, voxel, attrs=()):
    p32 = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    origin = grid_origin(p32, voxel)
    key = cell_key(cell_index(p32, origin, voxel))
    keys, label = np.unique(key, return_inverse=True)
    label = label.reshape(-1)
    m = len(keys)
    count = np.bincount(label, minlength=m).astype(np.int64)
    cells = np.stack([keys >> 42, (keys >> 21) & MAX_INDEX, keys & MAX_INDEX], 1)
    mean = lambda v: (ordered_sums(np.ascontiguousarray(v, np.float32).reshape(-1, 3), label, m) / count[:, None].astype(np.float64)).astype(np.float32)
    return VoxelRef(float(voxel), origin, cells, keys, count, mean(p32), [mean(a) for a in attrs], label)


def morton3(cells):
    """bit b of ix, iy, iz at bits 3b, 3b + 1, 3b + 2: the order in which the device lists its rows"""
    c = np.asarray(cells, np.int64).reshape(-1, 3).astype(np.uint64)
    out = np.zeros(len(c), np.uint64)
    for b in range(21):
        for d in range(3):
            out |= ((c[:, d] >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b + d)
    return out


def match_rows(ref, out_xyz):
    """Row of `ref` for every device row, by the cell index of the device's OUTPUT POINT on the reference's grid (a float32 mean lies between
    the smallest and the largest member coordinate, and floor((x - origin) / voxel) is monotone in x: a mean never leaves its cell).  Asserts
    that the device rows are the reference's cells, each once, listed in ascending Morton order."""
    out_xyz = np.ascontiguousarray(out_xyz, np.float32).reshape(-1, 3)
    assert len(out_xyz) == len(ref.keys), f"{len(out_xyz)} device rows, {len(ref.keys)} reference voxels"
    assert np.isfinite(out_xyz).all()
    idx = cell_index(out_xyz, ref.origin, ref.voxel)
    assert idx.min() >= 0 and idx.max() <= MAX_INDEX, (idx.min(), idx.max())
    k = cell_key(idx)
    pos = np.searchsorted(ref.keys, k).clip(max=len(ref.keys) - 1)
    wrong = ref.keys[pos] != k
    assert not wrong.any(), f"{int(wrong.sum())} device rows lie in cells the reference does not occupy, first {idx[wrong][:3].tolist()}"
    assert len(np.unique(pos)) == len(pos), "two device rows in one cell"
    mc = morton3(idx)
    assert (mc[1:] > mc[:-1]).all(), "device rows are not in ascending Morton order of their cells"
    return pos


def bits_equal(a, b):
    a = np.ascontiguousarray(a, np.float32); b = np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------ the inputs
def placed_cloud(cells, rng):
    """float32 points at the integer cell centres `cells` (n x 3; smallest index 0 on every axis) plus a jitter in (-0.25, 0.25): in
    (-0.249, -0.19) on an axis where the cell index is 0, in (-0.18, 0.18) elsewhere (at most 0.1875 in size after the float32 rounding of a
    coordinate below 2^21).  So origin = j - v / 2 with j the smallest jitter of all, a point of cell c sits at c + j' with 0 <= j' - j < 0.44,
    and on the voxel-1 grid floor(c + j' - j + 0.5) = c: the grid index IS the cell.  On a grid of v = 2, 3, ... the index is
    floor((c + v / 2 + j' - j) / v) = floor((c + v / 2) / v) for every member of the cell: a coarser voxel is a union of whole cells, and the
    cancelling pairs of order_sensitive_attribute stay together."""
    cells = np.asarray(cells, np.int64).reshape(-1, 3)
    assert cells.min() >= 0 and cells.max() <= MAX_INDEX and (cells.min(0) == 0).all()
    jit = np.where(cells == 0, rng.uniform(-0.249, -0.19, cells.shape), rng.uniform(-0.18, 0.18, cells.shape))
    return (cells.astype(np.float64) + jit).astype(np.float32)


def lattice_cloud(bits, n, cells, seed, axis_bits=None):
    """n float32 points on a voxel-1 lattice whose largest index is 2^bits - 1 (per axis: 2^axis_bits[d] - 1).  `cells` distinct occupied cells
    are drawn uniformly, the corner cells (0, 0, 0) and (max, max, max) among them, every cell gets one point and every other point is dealt
    to a random cell; then the points are shuffled, so the members of a voxel are scattered over the whole input.  Returns (xyz, cell of every point)."""
    rng = np.random.default_rng(seed)
    ab = tuple(int(b) for b in axis_bits) if axis_bits is not None else (int(bits),) * 3
    assert all(0 <= b <= 21 for b in ab)
    space = 1 << sum(ab)
    cells = int(max(1, min(cells, n, space)))
    if cells == 1:
        lin = np.zeros(1, np.uint64)
    else:
        inner = cells - 2
        if space <= 1 << 22:
            cand = rng.permutation(space - 2)[:inner].astype(np.uint64) + np.uint64(1)
        else:
            cand = np.unique(rng.integers(1, space - 1, size=inner + inner // 8 + 16, dtype=np.uint64))
            assert len(cand) >= inner
            cand = rng.permutation(cand)[:inner]
        lin = np.concatenate([np.array([0, space - 1], np.uint64), cand])
    mask = [np.uint64((1 << b) - 1) for b in ab]
    cell = np.stack([(lin >> np.uint64(ab[1] + ab[2])) & mask[0], (lin >> np.uint64(ab[2])) & mask[1], lin & mask[2]], 1).astype(np.int64)
    deal = rng.permutation(np.concatenate([np.arange(cells), rng.integers(0, cells, n - cells)]))
    cop = cell[deal]
    return placed_cloud(cop, rng), cop


def order_sensitive_attribute(cell_of_point, seed):
    """n x 3 float32 whose voxel means reveal the order in which the members were added (module docstring).  Per voxel of m >= 2 members and per
    channel, max(1, (m + 3) // 6) exactly cancelling pairs +A, -A (about a third of the members; A = (1 + u) 2^e, e in [60, 100), u a multiple of
    2^-23) and 1 + u for the rest, dealt to the members in random order, independently per channel.  A voxel of one member gets 1 + u."""
    rng = np.random.default_rng(seed)
    lab = np.asarray(cell_of_point).reshape(-1)
    n = len(lab)
    out = np.empty((n, 3), np.float32)
    pos = np.arange(n)
    for ch in range(3):
        order = np.lexsort((rng.random(n), lab))                 # the members of a voxel side by side, in random order
        sl = lab[order]
        start = np.ones(n, bool); start[1:] = sl[1:] != sl[:-1]
        heads = np.nonzero(start)[0]
        voxel_of = np.cumsum(start) - 1
        rank = pos - heads[voxel_of]
        size = np.diff(np.append(heads, n))[voxel_of]
        pairs = np.where(size >= 2, np.maximum(1, (size + 3) // 6), 0)
        small = 1.0 + rng.integers(0, 1 << 23, n) / float(1 << 23)
        big = (1.0 + rng.integers(0, 1 << 23, n) / float(1 << 23)) * np.exp2(rng.integers(60, 100, n).astype(np.float64))
        in_pair = rank < 2 * pairs
        val = np.where(in_pair, big, small)
        odd = np.nonzero(in_pair & (rank % 2 == 1))[0]
        val[odd] = -val[odd - 1]
        out[order, ch] = val                                     # (every value has 24 significant bits: exact in float32)
    return out


def order_sensitivity(values, cell_of_point):
    """How visible member order is in the float32 voxel means of `values` (n x 3 float32): the reference's means against the means with the
    members of every voxel added in REVERSED order.  Computed from the reference alone."""
    v = np.ascontiguousarray(values, np.float32).reshape(-1, 3)
    lab = np.asarray(cell_of_point).reshape(-1)
    m = int(lab.max()) + 1
    count = np.bincount(lab, minlength=m).astype(np.float64)[:, None]
    fwd = (ordered_sums(v, lab, m) / count).astype(np.float32)
    rev = (ordered_sums(v[::-1], lab[::-1], m) / count).astype(np.float32)
    changed = (fwd.view(np.uint32) != rev.view(np.uint32)).any(1)
    ge3 = count[:, 0] >= 3
    return {"voxels": m, "ge3": int(ge3.sum()), "changed": int(changed.sum()), "changed_ge3": int((changed & ge3).sum())}


def assert_condition(s, half_rule=True):
    assert s["ge3"] >= 1 and s["changed_ge3"] >= 0.9 * s["ge3"], s
    if half_rule:
        assert 2 * s["ge3"] >= s["voxels"], s


# ------------------------------------------------------------------------------------------------------------------ the cases
# Every device comparison of tests/test_gpu_voxel_grid.py takes its input from here, so that tests/test_voxel_reference.py can check, without
# a device, that the case still has the condition above.  `voxels`: the grids the case is used at.  `condition`: "full" (both rules), "order"
# (the 90 % rule only: the case is BUILT with a majority of singletons) or None (fewer than three points: no voxel can show order).
@dataclass
class Case:
    xyz: np.ndarray
    attrs: list
    voxels: tuple = (1.0,)
    condition: object = "full"
    top: object = None             # expected largest (ix, iy, iz) on the voxel-1 grid
    label: np.ndarray = field(default=None, repr=False)


N3 = 3 * 4096 + 1                                   # three full sort tiles plus one key
WIDTH_BITS = (2, 3, 6, 9, 11, 14, 17, 19, 21)       # 1, 2, 3, 4, 5, 6, 7, 8, 8 radix passes (8-bit digits over 3 * bits key bits)
SIZES = (1, 2, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097)
N_RUNS = 2 * 4096 + 1
LATTICE10 = (5.0, 4.0, 3.0, 2.0, 1.0)               # the project's voxel sizes {0.5, 0.4, 0.3, 0.2, 0.1} on a lattice of unit 0.1
GROUP = ((4097, 9), (12289, 14), (1, 11), (65, 3), (2, 11), (1023, 6), (4096, 17), (63, 2))      # (points, bits) of the clouds of a lockstep group


def _labels(cop):
    return np.unique(cell_key(cop), return_inverse=True)[1].reshape(-1)


def _lattice_case(bits, n, seed, axis_bits=None, voxels=(1.0,), n_attrs=1):
    xyz, cop = lattice_cloud(bits, n, max(min(n, 2), n // 4), seed, axis_bits)
    lab = _labels(cop)
    ab = axis_bits if axis_bits is not None else (bits,) * 3
    top = tuple((1 << b) - 1 for b in ab) if n >= 2 else (0, 0, 0)
    return Case(xyz, [order_sensitive_attribute(lab, seed * 7 + 1 + k) for k in range(n_attrs)], tuple(voxels), "full" if n >= 3 else None, top, lab)


def _runs_case(kind):
    rng = np.random.default_rng({"one_cell": 11, "two_cells": 12, "big_cell": 13}[kind])
    n, top = N_RUNS, 2047
    if kind == "one_cell":
        cop = np.zeros((n, 3), np.int64); cond = "full"; top = 0
    elif kind == "two_cells":                       # the two corners of an 11-bit grid, alternating in the input
        cop = np.where((np.arange(n) % 2 == 1)[:, None], top, 0) * np.ones((1, 3), np.int64); cond = "full"
    else:
        # one cell of 5,000 members among singletons: 4,500 of them in one run of the input, from index 1,000 on (whole 64-key rows of one
        # key, and a voxel that straddles the tile boundary at 4,096), 500 scattered; the singletons hold the corners
        _, single = lattice_cloud(11, n - 5000, n - 5000, 14)
        big = np.array([[1000, 37, 1999]], np.int64)
        assert not (single == big).all(1).any()
        rest = rng.permutation(np.concatenate([single, np.repeat(big, 500, 0)]))
        cop = np.concatenate([rest[:1000], np.repeat(big, 4500, 0), rest[1000:]]); cond = "order"
    lab = _labels(cop)
    return Case(placed_cloud(cop, rng), [order_sensitive_attribute(lab, 21)], (1.0,), cond, (top,) * 3, lab)


@functools.lru_cache(maxsize=None)
def case(name):
    if name.startswith("bits"):
        return _lattice_case(int(name[4:]), N3, 100 + int(name[4:]))
    if name == "aniso":
        return _lattice_case(21, N3, 131, axis_bits=(21, 1, 1))
    if name == "tiles34":
        return _lattice_case(11, 33 * 4096 + 5, 132)          # 135,173 keys = 34 tiles: the second trip of the scan's eight-load loop
    if name.startswith("n"):
        return _lattice_case(11, int(name[1:]), 200 + int(name[1:]))
    if name in ("one_cell", "two_cells", "big_cell"):
        return _runs_case(name)
    if name == "colours":
        return _lattice_case(11, N3, 300, n_attrs=2)
    if name in ("merged6", "merged11"):                       # (6 bits: the coarser grids merge cells; 11 bits: they only renumber them)
        return _lattice_case(int(name[6:]), N3, 400 + int(name[6:]), voxels=(1.0, 2.0, 4.0, 5.0, 3.0))         # {1, 2, 4} and LATTICE10
    if name == "merged63":                                    # the finest grid needs 3 * 21 = 63 Morton bits
        return _lattice_case(21, N3, 401, voxels=(1.0, 2.0, 4.0))
    if name.startswith("group"):
        n, bits = GROUP[int(name[5:])]
        return _lattice_case(bits, n, 500 + int(name[5:]), voxels=(1.0, 2.0, 4.0))
    raise KeyError(name)


CASE_NAMES = ([f"bits{b}" for b in WIDTH_BITS] + ["aniso", "tiles34"] + [f"n{n}" for n in SIZES] + ["one_cell", "two_cells", "big_cell", "colours",
              "merged6", "merged11", "merged63"] + [f"group{k}" for k in range(len(GROUP))])


@functools.lru_cache(maxsize=None)
def reference(name, voxel=1.0):
    c = case(name)
    return voxel_reference(c.xyz, voxel, c.attrs)


def check_case_condition(name):
    """The condition of every comparison on this case (every attribute, every grid it is used at); returns the figures."""
    c = case(name)
    out = []
    for voxel in c.voxels:
        ref = reference(name, voxel)
        if voxel == 1.0 and c.top is not None:
            assert tuple(ref.cells.max(0)) == tuple(c.top), (name, ref.cells.max(0), c.top)      # the grid is as wide as the case intends
            assert np.array_equal(ref.cell_of_point, c.label)                                   # ... and its voxels are the cells dealt
        for a in c.attrs:
            s = order_sensitivity(a, ref.cell_of_point)
            if c.condition:
                assert_condition(s, half_rule=c.condition == "full")
            out.append((name, voxel, s))
    return out
