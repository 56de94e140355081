"""Float64 numpy / scipy restatement of Open3D's ``PointCloud::ClusterDBSCAN`` on float32 points (a helper of the DBSCAN tests, not a test).

The rules (include/pcr_hip.h, ``pcr_cluster_dbscan``): j is a neighbour of i iff d^2 < eps^2 (strict, the point itself a member); core =
at least ``min_points`` members; clusters = connected components of the core-core pairs, numbered in ascending order of their smallest core
row; a non-core point takes the smallest label among its core neighbours; everything else is -1.

d^2 is formed as ``dx * dx``, ``+= dy * dy``, ``+= dz * dz`` in float64 (the order of ``_pair_d2`` in test_gpu_iss_keypoints.py), brute force
in blocks of ``chunk`` rows; eps^2 is the float64 product ``eps * eps``."""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

RIM_RTOL = 1e-9


def dbscan_reference(pts, eps, min_points, chunk=1000):
    """-> dict(labels int32 (n,), core bool (n,), n_clusters, rim_pairs, shared_border).

    rim_pairs: unordered pairs with |d^2 - eps^2| <= 1e-9 eps^2 and d^2 != eps^2 (an exact tie is decided: not a neighbour).
    shared_border: border rows whose core neighbours belong to more than one cluster."""
    pts = np.asarray(pts, dtype=np.float32).reshape(-1, 3)
    n = len(pts)
    p = pts.astype(np.float64)
    e2 = float(eps) * float(eps)
    rows, cols, rim = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], 0
    for i0 in range(0, n, chunk):
        a = p[i0:i0 + chunk]
        d = a[:, 0, None] - p[None, :, 0]
        d2 = d * d
        d = a[:, 1, None] - p[None, :, 1]
        d2 += d * d
        d = a[:, 2, None] - p[None, :, 2]
        d2 += d * d
        r, c = np.nonzero(d2 < e2)
        rows.append(r + i0); cols.append(c)
        rim += int(((np.abs(d2 - e2) <= RIM_RTOL * e2) & (d2 != e2)).sum())
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    core = np.bincount(rows, minlength=n) >= int(min_points)
    labels = np.full(n, -1, np.int32)
    n_clusters, shared = 0, 0
    if core.any():
        cc = core[rows] & core[cols]
        _, comp = connected_components(coo_matrix((np.ones(int(cc.sum()), np.int8), (rows[cc], cols[cc])), shape=(n, n)).tocsr(), directed=False)
        core_rows = np.nonzero(core)[0]
        first = np.full(comp.max() + 1, n, np.int64)                   # smallest core row of every component (n: a component of one non-core row)
        np.minimum.at(first, comp[core_rows], core_rows)
        order = np.argsort(first, kind="stable")
        n_clusters = int((first < n).sum())
        number = np.empty(len(first), np.int64)
        number[order] = np.arange(len(first))                          # the components with a core row come first, in the order of that row
        labels[core_rows] = number[comp[core_rows]]
        bc = ~core[rows] & core[cols]                                  # (border row, core neighbour)
        lo = np.full(n, n_clusters, np.int64); hi = np.full(n, -1, np.int64)
        np.minimum.at(lo, rows[bc], labels[cols[bc]])
        np.maximum.at(hi, rows[bc], labels[cols[bc]])
        border = hi >= 0
        labels[border] = lo[border]
        shared = int((border & (lo != hi)).sum())
    return dict(labels=labels, core=core, n_clusters=n_clusters, rim_pairs=rim // 2, shared_border=shared)
