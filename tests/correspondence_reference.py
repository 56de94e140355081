"""Float64 restatements, in plain numpy, of what the library computes on a correspondence list the caller holds (include/pcr_hip.h,
pcr_estimation_compute_transformation / pcr_estimation_compute_rmse / pcr_correspondences_from_features): the references of
tests/test_gpu_correspondences.py.  The 6x6 systems are solved by the oracle's ``solve_update`` (Open3D's LDLT and pose), the GICP
system is built by the oracle's ``gicp_linearize`` on the list."""
import numpy as np


def umeyama(src, dst, with_scaling):
    """Eigen::umeyama by SVD (tests/test_gpu_icp_estimators.py::_umeyama)."""
    n = src.shape[0]
    ms, md = src.mean(0), dst.mean(0)
    sd, dd = src - ms, dst - md
    sigma = dd.T @ sd / n
    U, D, Vt = np.linalg.svd(sigma)
    S = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2] = -1
    R = U @ np.diag(S) @ Vt
    c = (D @ S) / ((sd ** 2).sum() / n) if with_scaling else 1.0
    T = np.eye(4)
    T[:3, :3] = c * R
    T[:3, 3] = md - c * R @ ms
    return T


def _pairs(src, tgt, corres):
    corres = np.asarray(corres, np.int64).reshape(-1, 2)
    return np.asarray(src, np.float64)[corres[:, 0]], np.asarray(tgt, np.float64)[corres[:, 1]], corres


def kernel_weights(loss, k, r):
    if loss == "l1":
        return 1.0 / np.abs(r)
    if loss == "gm":
        return k / (k + r * r) ** 2
    return np.ones_like(r)


def point_to_point(src, tgt, corres, with_scaling=False):
    s, t, corres = _pairs(src, tgt, corres)
    return umeyama(s, t, with_scaling) if len(corres) else np.eye(4)


def point_to_plane(oracle, src, tgt, tgt_normals, corres, loss="l2", k=1.0):
    """r = (s - t).n over the normals as stored, J = [s x n, n], the kernel's weights; identity when the system has no solution."""
    s, t, corres = _pairs(src, tgt, corres)
    if not len(corres) or tgt_normals is None:
        return np.eye(4)
    n = np.asarray(tgt_normals, np.float64)[corres[:, 1]]
    r = ((s - t) * n).sum(1)
    J = np.concatenate([np.cross(s, n), n], axis=1)
    w = kernel_weights(loss, k, r)
    T, rc = oracle.solve_update((J * w[:, None]).T @ J, (J * (w * r)[:, None]).sum(0))
    return T if rc == 0 else np.eye(4)


def cov9_from_cov6(cov6):
    c = np.asarray(cov6, np.float64)
    out = np.empty((c.shape[0], 3, 3))
    out[:, 0, 0] = c[:, 0]; out[:, 0, 1] = out[:, 1, 0] = c[:, 1]; out[:, 0, 2] = out[:, 2, 0] = c[:, 2]
    out[:, 1, 1] = c[:, 3]; out[:, 1, 2] = out[:, 2, 1] = c[:, 4]; out[:, 2, 2] = c[:, 5]
    return out


def unit_normals(normals):
    """the normals as the GICP rows take them: e1 where n.x < -0.99, then normalised"""
    n = np.asarray(normals, np.float64).copy()
    n[n[:, 0] < -0.99] = (1.0, 0.0, 0.0)
    return n / np.linalg.norm(n, axis=1, keepdims=True)


def generalized_icp(oracle, src, tgt, corres, loss, k=1.0, src_cov=None, tgt_cov=None, src_normals=None, tgt_normals=None, epsilon=1e-3):
    """Both clouds with covariances (N x 3 x 3): used untouched.  Neither, both with normals: the covariances of the normals.  Else identity."""
    corres = np.asarray(corres, np.int64).reshape(-1, 2)
    if not len(corres):
        return np.eye(4)
    if src_cov is not None and tgt_cov is not None:
        cs, ct = src_cov, tgt_cov
    elif src_cov is None and tgt_cov is None and src_normals is not None and tgt_normals is not None:
        cs, ct = oracle.covariances_from_normals(unit_normals(src_normals), epsilon), oracle.covariances_from_normals(unit_normals(tgt_normals), epsilon)
    else:
        return np.eye(4)
    code = {"l2": oracle.LOSS_L2, "l1": oracle.LOSS_L1, "gm": oracle.LOSS_GM}[loss]
    JTJ, JTr, _ = oracle.gicp_linearize(np.asarray(src, np.float64), cs, np.asarray(tgt, np.float64), ct, corres.astype(np.int32), code, k)
    T, rc = oracle.solve_update(JTJ, JTr)
    return T if rc == 0 else np.eye(4)


def rmse_euclidean(src, tgt, corres):
    """point-to-point and GICP: sqrt(sum |s - t|^2 / C)"""
    s, t, corres = _pairs(src, tgt, corres)
    return float(np.sqrt(((s - t) ** 2).sum() / len(corres))) if len(corres) else 0.0


def rmse_plane(src, tgt, tgt_normals, corres):
    """point-to-plane: sqrt(sum ((s - t).n)^2 / C), 0 without target normals"""
    s, t, corres = _pairs(src, tgt, corres)
    if not len(corres) or tgt_normals is None:
        return 0.0
    r = ((s - t) * np.asarray(tgt_normals, np.float64)[corres[:, 1]]).sum(1)
    return float(np.sqrt((r * r).sum() / len(corres)))


def nearest_rows(a, b, chunk=128):
    """Per row of a, over the rows of b by d = sum_k (a_ik - b_jk)^2 in float64 on the float32 rows: (index of the smallest d, the smaller index
    on a tie; smallest d; second smallest d).  Row blocks at a time: the table is never held whole."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    idx = np.empty(a.shape[0], np.int64); best = np.empty(a.shape[0]); second = np.full(a.shape[0], np.inf)
    for i0 in range(0, a.shape[0], chunk):
        d = a[i0:i0 + chunk, None, :] - b[None, :, :]
        d = (d * d).sum(2)
        idx[i0:i0 + chunk] = d.argmin(1)                      # argmin returns the first minimum: the smaller index on a tie
        if b.shape[0] > 1:
            part = np.partition(d, 1, axis=1)
            best[i0:i0 + chunk], second[i0:i0 + chunk] = part[:, 0], part[:, 1]
        else:
            best[i0:i0 + chunk] = d[:, 0]
    return idx, best, second


def match_features(src_feat, tgt_feat, mutual_filter=False, mutual_consistency_ratio=0.1):
    """Brute force: (i, nearest target row of i) by (float64 distance, smaller index), in source order; with mutual_filter the rows whose
    target row points back when there are at least int(ratio * n_src) of them, else all rows.  Returns (rows, mutual count)."""
    s_to_t = nearest_rows(src_feat, tgt_feat)[0]
    t_to_s = nearest_rows(tgt_feat, src_feat)[0]
    n = len(s_to_t)
    rows = np.stack([np.arange(n), s_to_t], axis=1).astype(np.int32)
    mutual = rows[t_to_s[s_to_t] == np.arange(n)]
    if mutual_filter and len(mutual) >= int(mutual_consistency_ratio * n):
        return mutual, len(mutual)
    return rows, len(mutual)
