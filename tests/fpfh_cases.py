"""The inputs of the FPFH row tests (test_fpfh_reference.py on the CPU, test_gpu_fpfh_rows.py on the device), a few thousand points at most,
and their cached float64 references.  A case is (points, normals float32, search specs, cap): cap = the largest share of rows that may be
excluded as `touched` or `list_open`, by themselves or by a neighbour (fpfh_reference.py) -- a condition on the INPUT, asserted on the CPU."""
import functools

import numpy as np

import fpfh_reference as fr

SHEET_R = 0.2
SMALL_SIZES = (1, 2, 3, 8, 9, 31, 32, 33, 64, 65, 129, 201)
NORMAL_KINDS = ("x0.5", "voxel", "x1.05", "x1.5", "x100", "mixed")


def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def sheet(n=2000, seed=1):
    """A bumpy surface over [0, 4] x [0, 2], dense at x = 0 (about 300 points in a ball of SHEET_R) and sparse at x = 4 (about 15), with noisy
    unit normals of generic direction."""
    rng = np.random.default_rng(seed)
    x = 4.0 * rng.random(n) ** 2
    y = 2.0 * rng.random(n)
    z = 0.15 * np.sin(3.0 * x) * np.cos(2.0 * y) + rng.normal(0.0, 0.02, n)
    pts = np.stack([x, y, z], axis=1).astype(np.float32)
    g = np.stack([-0.45 * np.cos(3.0 * x) * np.cos(2.0 * y), 0.30 * np.sin(3.0 * x) * np.sin(2.0 * y), np.ones(n)], axis=1)
    nrm = _unit(_unit(g) + rng.normal(0.0, 0.5, (n, 3))).astype(np.float32)
    return pts, nrm


def sheet_with_copies():
    """The sheet with three points at one place, each with a normal of its own: votes in the bins of f = 0, no weight in the sum.  (Few copies: a
    list that is cut between two of them is `list_open`, and so is every row that reads it.)"""
    pts, nrm = sheet()
    for dst, src in ((100, 7), (101, 7)):
        pts[dst] = pts[src]
    return pts, nrm


def small(n):
    """The first n points of one blob of radius 0.5 with random unit normals."""
    rng = np.random.default_rng(7)
    pts = (0.5 * _unit(rng.normal(size=(256, 3))) * rng.random((256, 1)) ** (1.0 / 3.0)).astype(np.float32)
    nrm = _unit(rng.normal(size=(256, 3))).astype(np.float32)
    return pts[:n].copy(), nrm[:n].copy()


def places():
    """Three points at one place, two at another, normals all different: "skip the point itself" and "skip list place 0" must agree."""
    pts = np.array([[0.25, 0.5, 0.125]] * 3 + [[0.75, 0.25, 0.5]] * 2, np.float32)
    nrm = _unit(np.random.default_rng(3).normal(size=(5, 3))).astype(np.float32)
    return pts, nrm


def copies_over_k():
    """Six copies of one point (more than the k = 3 of its specs) and six points elsewhere."""
    rng = np.random.default_rng(9)
    pts = np.concatenate([np.tile(np.array([[0.5, 0.25, 0.75]]), (6, 1)), rng.random((6, 3))]).astype(np.float32)
    nrm = _unit(rng.normal(size=(12, 3))).astype(np.float32)
    return pts, nrm


def flat_patch():
    """225 points of the plane z = 0 with the normal (0, 0, 1): under KNN(200) all 199 votes of a point land in ONE bin of each histogram."""
    rng = np.random.default_rng(5)
    pts = np.concatenate([rng.random((225, 2)), np.zeros((225, 1))], axis=1).astype(np.float32)
    nrm = np.tile(np.array([[0.0, 0.0, 1.0]], np.float32), (225, 1))
    return pts, nrm


def needles(height, stacks, seed=11):
    """`stacks` vertical stacks of `height` points 0.1 apart with exactly equal x and y and the normal (0, 0, 1), at random places of a square in
    which about six other stacks stand within 1.0 of a stack (none nearer than 0.15: no direction between stacks is near the vertical).  Inside
    a stack dp x n is exactly zero: float64 takes the degenerate branch, the float form must decline.  Search: Hybrid(1.0, 200)."""
    rng = np.random.default_rng(seed)
    side = np.sqrt(stacks * np.pi / 7.0)
    xy = np.zeros((0, 2))
    while len(xy) < stacks:
        c = side * rng.random(2)
        if len(xy) == 0 or ((xy - c) ** 2).sum(1).min() > 0.15 ** 2:
            xy = np.concatenate([xy, c[None]])
    z0 = 0.05 * rng.random(stacks)
    pts = np.zeros((stacks, height, 3))
    pts[:, :, :2] = xy[:, None, :]
    pts[:, :, 2] = z0[:, None] + 0.1 * np.arange(height)[None, :]
    pts = pts.reshape(-1, 3).astype(np.float32)
    return pts, np.tile(np.array([[0.0, 0.0, 1.0]], np.float32), (len(pts), 1))


def sheet_normals(kind):
    """The sheet with normals that are not unit normals: all halved; shortened by a factor in [0.7, 1] per point, as the mean of the normals of a
    voxel is; 1.05, 1.5 and 100 times as long; or unit and long ones (x1.5, x3) side by side."""
    pts, nrm = sheet()
    rng = np.random.default_rng(13)
    n = len(pts)
    if kind == "voxel":
        f = 0.7 + 0.3 * rng.random(n)
    elif kind == "mixed":
        f = np.where(rng.random(n) < 0.5, 1.0, np.where(rng.random(n) < 0.5, 1.5, 3.0))
    else:
        f = np.full(n, float(kind[1:]))
    return pts, (nrm.astype(np.float64) * f[:, None]).astype(np.float32)


SHEET_SPECS = (("hybrid", SHEET_R, 50), ("hybrid", SHEET_R, 200), ("knn", 10), ("knn", 100), ("knn", 200), ("knn", 1), ("hybrid", SHEET_R, 1))
SMALL_SPECS = (("knn", 200), ("hybrid", 10.0, 200))
NEEDLE_SPEC = ("hybrid", 1.0, 200)
NORMALS_SPEC = ("hybrid", SHEET_R, 50)

CASES = {"sheet": (sheet, SHEET_SPECS, 0.01),
         "copies": (sheet_with_copies, (("hybrid", SHEET_R, 50), ("knn", 10)), 0.01),
         "places": (places, SMALL_SPECS, 0.0),
         "overk": (copies_over_k, (("knn", 3), ("hybrid", 10.0, 3)), 1.0),      # (every list is cut inside a run of equal distances)
         "flat": (flat_patch, (("knn", 200),), 0.01),
         "needle8": (functools.partial(needles, 8, 125), (NEEDLE_SPEC,), 0.0),
         "needle10": (functools.partial(needles, 10, 100), (NEEDLE_SPEC,), 0.0)}
CASES.update({f"small{n}": (functools.partial(small, n), SMALL_SPECS, 0.0) for n in SMALL_SIZES})
CASES.update({f"normals_{k}": (functools.partial(sheet_normals, k), (NORMALS_SPEC,), 0.01) for k in NORMAL_KINDS})


def case_ids(prefix=None):
    """("name", spec) of every case (of the cases whose name starts with prefix)."""
    return [(name, spec) for name, (_, specs, _) in CASES.items() if prefix is None or name.startswith(prefix) for spec in specs]


def spec_id(v):
    return v if isinstance(v, str) else "-".join(str(x) for x in v)


@functools.lru_cache(maxsize=None)
def cloud(name):
    pts, nrm = CASES[name][0]()
    pts.setflags(write=False); nrm.setflags(write=False)
    return pts, nrm


@functools.lru_cache(maxsize=None)
def reference(name, spec):
    """-> (points, normals, lists idx, the dict of fpfh_reference.fpfh, excluded, cap); computed once per process, shared, read-only.  excluded (n,):
    the row, or a row its list names, is `touched` or `list_open`."""
    pts, nrm = cloud(name)
    idx, is_open = fr.lists_for(pts, spec)
    ref = fr.fpfh(pts, nrm, idx)
    excluded = ref["touched"] | fr.spread(is_open, idx)
    for a in (idx, excluded, *ref.values()):
        a.setflags(write=False)
    return pts, nrm, idx, ref, excluded, CASES[name][2]
