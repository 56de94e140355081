"""numpy restatement of the normal-orientation rules of include/pcr_hip.h (DIST, DOT, ORDER, EMST, KNN, GRAPH, TREE, ROOT, PROPAGATE, RESULT and
the element-wise calls): the yardstick of the normal-orientation tests.  Everything is float64 on the float32 inputs with every operation
rounded once (numpy does not fuse), and every order is the strict total order (weight, lo, hi), so both spanning trees are unique and the
device has to reproduce every row.

EMST: Prim under ORDER, one distance row per step (no n x n matrix).  KNN: neighbor_reference.knn.  TREE: Kruskal over the lexsorted edge list.
PROPAGATE: the parity statement (`flips_by_parity`) and a literal queue-based walk that negates rows as it goes (`flips_by_walk`)."""
from collections import deque

import numpy as np

import neighbor_reference as nr


def lattice(m):
    """the m x m x m unit lattice, row (x m + y) m + z = (x, y, z): every d^2 tied"""
    g = np.arange(m, dtype=np.float32)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)


def d2_row(p64, i):
    """DIST of every row to row i"""
    d = p64[:, 0] - p64[i, 0]
    d2 = d * d
    d = p64[:, 1] - p64[i, 1]
    d2 += d * d
    d = p64[:, 2] - p64[i, 2]
    d2 += d * d
    return d2


def dot_rows(normals, a, b):
    """DOT of the rows a[t] and b[t]"""
    n64 = np.asarray(normals, np.float32).reshape(-1, 3).astype(np.float64)
    c = n64[a, 0] * n64[b, 0]
    c = c + n64[a, 1] * n64[b, 1]
    c = c + n64[a, 2] * n64[b, 2]
    return c


def _sorted_edges(lo, hi, *extra):
    order = np.lexsort((hi, lo))
    edges = np.stack([lo[order], hi[order]], 1).astype(np.int64).reshape(-1, 2)
    return (edges,) + tuple(np.asarray(x)[order] for x in extra)


def emst_reference(points):
    """EMST -> (edges (n - 1, 2) int64, rows (lo, hi) ascending by (lo, hi); d2 (n - 1,) float64 aligned with them).  Prim: the vertex outside the
    tree whose best edge into it is the smallest under ORDER joins next; under a strict total order that is the unique minimum spanning tree."""
    p64 = np.asarray(points, np.float32).reshape(-1, 3).astype(np.float64)
    n = len(p64)
    if n < 2:
        return np.zeros((0, 2), np.int64), np.zeros(0)
    ids = np.arange(n, dtype=np.int64)
    outside = np.ones(n, bool); outside[0] = False
    bd = d2_row(p64, 0)
    blo = np.minimum(ids, 0); bhi = np.maximum(ids, 0)
    lo_out = np.empty(n - 1, np.int64); hi_out = np.empty(n - 1, np.int64); d_out = np.empty(n - 1)
    for step in range(n - 1):
        m = bd[outside].min()
        cand = np.nonzero(outside & (bd == m))[0]
        v = int(cand[0])
        if len(cand) > 1:
            v = int(cand[np.lexsort((bhi[cand], blo[cand]))[0]])
        lo_out[step], hi_out[step], d_out[step] = blo[v], bhi[v], bd[v]
        outside[v] = False
        d = d2_row(p64, v)
        nlo = np.minimum(ids, v); nhi = np.maximum(ids, v)
        better = outside & ((d < bd) | ((d == bd) & ((nlo < blo) | ((nlo == blo) & (nhi < bhi)))))
        bd = np.where(better, d, bd); blo = np.where(better, nlo, blo); bhi = np.where(better, nhi, bhi)
    return _sorted_edges(lo_out, hi_out, d_out)


def knn_lists(points, k):
    """KNN -> (n, k') int64 with -1 beyond the cloud's size: the first k rows of the order (d^2, index), the row itself still in its place"""
    pts = np.asarray(points, np.float32).reshape(-1, 3)
    if k <= 0 or len(pts) == 0:
        return np.zeros((len(pts), 0), np.int64)
    return nr.knn(pts, pts, int(k))[0]


def graph_edges(emst, lists):
    """GRAPH -> unique (lo, hi) rows: the EMST and every (i, j in KNN(i)), the row itself skipped"""
    n, k = lists.shape
    i = np.repeat(np.arange(n, dtype=np.int64), k); j = lists.reshape(-1)
    keep = (j >= 0) & (j != i)
    i, j = i[keep], j[keep]
    e = np.concatenate([np.asarray(emst, np.int64).reshape(-1, 2), np.stack([np.minimum(i, j), np.maximum(i, j)], 1)])
    return np.unique(e, axis=0)


def tree_reference(n, edges, normals):
    """TREE: Kruskal over the edges in the order (w, lo, hi) -> (n - 1, 2) int64 ascending by (lo, hi)"""
    w = 1.0 - np.abs(dot_rows(normals, edges[:, 0], edges[:, 1]))
    order = np.lexsort((edges[:, 1], edges[:, 0], w))
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    lo, hi = [], []
    for a, b in edges[order].tolist():
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[ra] = rb
            lo.append(a); hi.append(b)
            if len(lo) == n - 1:
                break
    assert len(lo) == n - 1, "the graph is not connected"
    return _sorted_edges(np.asarray(lo, np.int64), np.asarray(hi, np.int64))[0]


def root_reference(points):
    """ROOT: the smallest row with the largest z (float32 comparison)"""
    return int(np.argmax(np.asarray(points, np.float32).reshape(-1, 3)[:, 2]))


def _adjacency(n, tree):
    adj = [[] for _ in range(n)]
    for a, b in np.asarray(tree).tolist():
        adj[a].append(b); adj[b].append(a)
    return adj


def flips_by_parity(points, normals, tree):
    """PROPAGATE as stated: flip_v = flip_r XOR the XOR of s(i, j) = (c(i, j) < 0) over the tree path r -> v, s from the INPUT normals"""
    nrm = np.asarray(normals, np.float32).reshape(-1, 3)
    n = len(nrm)
    r = root_reference(points)
    s = {}
    if len(tree):
        neg = dot_rows(nrm, tree[:, 0], tree[:, 1]) < 0.0
        s = {(int(a), int(b)): bool(f) for (a, b), f in zip(tree.tolist(), neg.tolist())}
    adj = _adjacency(n, tree)
    flip = np.zeros(n, bool); seen = np.zeros(n, bool)
    flip[r] = nrm[r, 2] < 0; seen[r] = True
    stack = [r]
    while stack:
        u = stack.pop()
        for v in adj[u]:
            if not seen[v]:
                seen[v] = True
                flip[v] = flip[u] ^ s[(min(u, v), max(u, v))]
                stack.append(v)
    assert seen.all()
    return flip


def flips_by_walk(points, normals, tree):
    """Open3D's breadth-first walk, literally: the root is turned to +z, then a child is negated iff (oriented parent) . child < 0.
    -> (flip mask, the oriented normals float32)"""
    out = np.array(normals, np.float32).reshape(-1, 3).copy()
    n = len(out)
    r = root_reference(points)
    adj = _adjacency(n, tree)
    flip = np.zeros(n, bool); seen = np.zeros(n, bool)
    if out[r, 2] < 0:
        out[r] = -out[r]; flip[r] = True
    seen[r] = True
    queue = deque([r])
    while queue:
        u = queue.popleft()
        for v in adj[u]:
            if not seen[v]:
                seen[v] = True
                if dot_rows(out, np.array([u]), np.array([v]))[0] < 0.0:
                    out[v] = -out[v]; flip[v] = True
                queue.append(v)
    assert seen.all()
    return flip, out


def orient_reference(points, normals, k, emst=None, lists=None):
    """The whole rule -> dict(emst, emst_d2, lists, tree, root, flip, normals).  `emst`: (edges, d2) when already known (it depends on the points only);
    `lists`: knn_lists(points, k') with k' >= k when already known (the first k places of a longer list are the list of k)."""
    pts = np.asarray(points, np.float32).reshape(-1, 3)
    nrm = np.asarray(normals, np.float32).reshape(-1, 3)
    n = len(pts)
    e, d2 = emst if emst is not None else emst_reference(pts)
    lists = knn_lists(pts, k) if lists is None else np.asarray(lists)[:, :max(int(k), 0)]
    tree = tree_reference(n, graph_edges(e, lists), nrm) if n > 1 else np.zeros((0, 2), np.int64)
    flip = flips_by_parity(pts, nrm, tree) if n else np.zeros(0, bool)
    out = nrm.copy()
    out[flip] = -out[flip]
    return dict(emst=e, emst_d2=d2, lists=lists, tree=tree, root=root_reference(pts) if n else -1, flip=flip, normals=out)


# ---- the element-wise calls: float64 on the float32 data, sums in the order x, y, z
def _dot3(a, b):
    d = a[:, 0] * b[:, 0]
    d = d + a[:, 1] * b[:, 1]
    d = d + a[:, 2] * b[:, 2]
    return d


def direction_reference(normals, ref):
    nrm = np.array(normals, np.float32).reshape(-1, 3).copy()
    ref = np.asarray(ref, np.float64).reshape(1, 3)
    zero = (nrm == 0).all(1)
    neg = (_dot3(nrm.astype(np.float64), np.broadcast_to(ref, nrm.shape)) < 0.0) & ~zero
    nrm[neg] = -nrm[neg]
    nrm[zero] = ref.astype(np.float32)
    return nrm


def camera_reference(points, normals, loc):
    pts = np.asarray(points, np.float32).reshape(-1, 3).astype(np.float64)
    nrm = np.array(normals, np.float32).reshape(-1, 3).copy()
    v = np.asarray(loc, np.float64).reshape(1, 3) - pts
    zero = (nrm == 0).all(1)
    neg = (_dot3(nrm.astype(np.float64), v) < 0.0) & ~zero
    nrm[neg] = -nrm[neg]
    length = np.sqrt(_dot3(v, v))
    with np.errstate(invalid="ignore", divide="ignore"):
        unit = np.where(length[:, None] == 0.0, np.array([[0.0, 0.0, 1.0]]), v / length[:, None])
    nrm[zero] = unit[zero].astype(np.float32)
    return nrm


def normalize_reference(normals):
    nrm = np.array(normals, np.float32).reshape(-1, 3).copy()
    n64 = nrm.astype(np.float64)
    length = np.sqrt(_dot3(n64, n64))
    nz = ~(nrm == 0).all(1)
    nrm[nz] = (n64[nz] / length[nz, None]).astype(np.float32)
    return nrm
