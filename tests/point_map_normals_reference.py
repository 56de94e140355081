"""Restatement of ESTIMATE on a voxel point map (the rule: include/pcr_hip.h, "scan-to-map ICP on a voxel point map") and of point-to-plane ICP on
an estimated map, in numpy, built from what the suite has: it imports neither the package nor a device nor the oracle.

  estimate        the neighbour sets of every map row: normal_reference.neighbours(rows, RADIUS, radius=rho), brute force over ALL rows in the float64
                  arithmetic of the rule (differences, squares, (x + y) + z, d^2 < rho^2 strict), so the counts must be EQUAL to the device's, not
                  close; valid = count >= k_min.  The normals themselves need no reference vector: normal_reference.assert_normals_explained
                  bounds every row from its covariance alone
  brute_counts    the same counts written as a literal double loop (the CPU test holds the two equal)
  with_normals    a reference map with given normals (the device's own, once they are explained; or eigh's, to run the restatement alone)
  rows_at         point_map_reference.rows_at filtered by validity: a match whose map row is not valid is no row
  linearize, loop point_map_reference's, over those rows
  odometry        the recipe of scan_to_map_odometry_icp_map_normals, under the "static" motion model
"""
import dataclasses

import numpy as np

import normal_reference as nr
import point_map_reference as pm


def estimate(m, radius, min_neighbors):
    """(Neighbours, counts (rows,) int64, valid (rows,) bool) of the map's rows"""
    assert 0.0 < radius <= m.voxel and min_neighbors >= 3
    nb = nr.neighbours(m.points, nr.RADIUS, radius=float(radius))
    return nb, nb.count, nb.count >= min_neighbors


def brute_counts(points, radius):
    """count_i, literally: every pair, d^2 = ((dx dx + dy dy) + dz dz) in float64 on the widened float32 points, d^2 < radius^2 strict"""
    p = np.ascontiguousarray(points, np.float32).astype(np.float64)
    r2 = float(radius) * float(radius)
    out = np.zeros(len(p), np.int64)
    for i in range(len(p)):
        for j in range(len(p)):
            dx, dy, dz = p[i, 0] - p[j, 0], p[i, 1] - p[j, 1], p[i, 2] - p[j, 2]
            if (dx * dx + dy * dy) + dz * dz < r2:
                out[i] += 1
    return out


def eigh_normals(m, nb):
    """normals by np.linalg.eigh over the reference covariance, with the rule's literal answer on the special rows (fewer than 3 neighbours, a zero or
    a diagonal covariance: normal_reference.special_rule): to run the restatement without a device (no assertion compares a device against them)"""
    v = nr.eigh_vectors(m.points, nb.idx)
    C, _, cnt = nr.covariance(m.points, nb.idx)
    special, exp = nr.special_rule(C, cnt)
    v[special] = exp[special].astype(np.float32)
    return v


def with_normals(m, normals):
    return dataclasses.replace(m, normals=np.ascontiguousarray(normals, np.float32))


def rows_at(m, valid, src, T, max_distance, neighborhood=27, with_d2=False):
    pairs, d2 = pm.rows_at(m, src, T, max_distance, neighborhood, with_d2=True)
    keep = valid[pairs[:, 1]]
    return (pairs[keep], d2[keep]) if with_d2 else pairs[keep]


def linearize(m, valid, src, T, max_distance, neighborhood=27, loss=pm.L2, k=1.0, chunk=None):
    """point_map_reference.linearize for PCR_EST_POINT_TO_PLANE over the valid rows: the same expressions, the same dict"""
    pairs, d2 = rows_at(m, valid, src, T, max_distance, neighborhood, with_d2=True)
    s = pm.transform(src, T)[pairs[:, 0]]
    t = m.points[pairs[:, 1]].astype(np.float64)
    n = m.normals[pairs[:, 1]].astype(np.float64)
    e = s - t
    r = (e[:, 0] * n[:, 0] + e[:, 1] * n[:, 1]) + e[:, 2] * n[:, 2]
    J = np.concatenate([np.cross(s, n), n], 1)
    w = pm.weight(loss, k, r)
    tJ = w[:, None, None] * J[:, :, None] * J[:, None, :]
    tr = w[:, None] * J * r[:, None]
    return dict(JTJ=pm._sum(tJ, chunk), JTr=pm._sum(tr, chunk), rows=len(pairs), sum_d2=float(pm._sum(d2, chunk)), sum_r2=float(pm._sum(r * r, chunk)),
                mag_JTJ=np.abs(tJ).sum(0), mag_JTr=np.abs(tr).sum(0), pairs=pairs)


def loop(m, valid, src, T0, max_distance, neighborhood=27, loss=pm.L2, k=1.0, max_it=30, rel_fitness=1e-6, rel_rmse=1e-6, chunk=None):
    """point_map_reference.loop over linearize above"""
    n = len(np.asarray(src).reshape(-1, 3))
    T = np.array(T0, np.float64).reshape(4, 4)

    def lin(T):
        s = linearize(m, valid, src, T, max_distance, neighborhood, loss, k, chunk)
        rows = s["rows"]
        return s, (rows / n if n else 0.0), (float(np.sqrt(s["sum_d2"] / rows)) if rows else 0.0)

    s, fit, rmse = lin(T)
    it, converged, history = 0, False, []
    while it < max_it:
        U = pm.solve_update(s["JTJ"], s["JTr"]) if s["rows"] else np.eye(4)
        T = U @ T
        before = (fit, rmse)
        s, fit, rmse = lin(T)
        it += 1
        history.append((T.copy(), fit, rmse, s["rows"]))
        if abs(before[0] - fit) < rel_fitness and abs(before[1] - rmse) < rel_rmse:
            converged = True
            break
    return pm.LoopResult(T, fit, rmse, s["rows"], it, converged, history)


def odometry(scans, voxel, max_distance, M, grid_min, radius, min_neighbors, max_it=30):
    """scan_to_map_odometry_icp_map_normals(scans, voxel, max_distance, estimation_method=point to plane (L2), motion_model="static", max_points_per_voxel=M,
    grid_min=grid_min, map_normal_radius=radius, map_normal_min_neighbors=min_neighbors) on float32 arrays -> (poses, final map with eigh normals, valid)"""
    def estimated(m):
        nb, _, valid = estimate(m, radius, min_neighbors)
        return with_normals(m, eigh_normals(m, nb)), valid

    m, valid = estimated(pm.build_map(scans[0], None, voxel, M, grid_min, np.eye(4)))
    poses = [np.eye(4)]
    for k in range(1, len(scans)):
        res = loop(m, valid, scans[k], poses[-1], max_distance, 27, max_it=max_it)
        poses.append(res.transformation)
        m, valid = estimated(pm.insert(dataclasses.replace(m, normals=None), scans[k], None, poses[-1]))
    return poses, m, valid
