"""registration_colored_icp on the device against a float64 restatement of its specification (include/pcr_hip.h): colour means through the
voxel pass, the colour gradients (pcr_color_gradient), the trajectory of the two-row iteration, its lambda = 1 limit (point-to-plane), a planar
patch that only colour can register, errors, graph-cache keys and the scheduling switches.

Colours are a smooth synthetic texture c(p): three channels 0.5 + 0.4 sin(2 pi a.p / L + phi) with periods L = 8, 11 and 15 m along three
different directions, so every value lies in [0.1, 0.9] and nothing clips.  The target carries c(p) at its own points, the source
c(T_gicp p): the colours agree at the golden pose."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, pkg, pose_error

pytestmark = pytest.mark.gpu

F32_ROUND = 2.0 ** -24                    # one float32 rounding, relative
DIRS = np.array([[0.8, 0.6, 0.0], [-0.6, 0.64, 0.48], [0.36, -0.48, 0.8]])
PERIODS = np.array([8.0, 11.0, 15.0])
PHASES = np.array([0.3, 1.7, 4.1])


def texture(p, periods=PERIODS):
    p = np.asarray(p, np.float64)
    return (0.5 + 0.4 * np.sin(2.0 * np.pi * (p @ DIRS.T) / periods + PHASES)).astype(np.float32)


def intensity(colors):
    c = np.asarray(colors, np.float64)
    return (c[:, 0] + c[:, 1] + c[:, 2]) / 3.0


@pytest.fixture(scope="module")
def P():
    return pkg()


@pytest.fixture(scope="module")
def colored_clouds(P, small_pair):
    """Pair 899 at voxel 0.3, SOR(30, 1), KNN-20 normals -- the clouds of tests/test_gpu_icp_estimators.py -- with the texture on top."""
    out = []
    for key in ("source", "target"):
        pc = P.PointCloud(small_pair[key]).voxel_down_sample(0.3)
        pc, _ = pc.remove_statistical_outlier(30, 1.0)
        pc.estimate_normals(P.KDTreeSearchParamKNN(knn=20))
        out.append(pc)
    src, tgt = out
    Tg = np.asarray(small_pair["T_gicp"], np.float64)
    src.colors = texture(np.asarray(src.points) @ Tg[:3, :3].T + Tg[:3, 3])
    tgt.colors = texture(tgt.points)
    return src, tgt


# ------------------------------------------------------------------------------------------ the restatement
def ldlt3(M, b):
    """Rows of x = M^-1 b for symmetric 3x3 M by LDL^T with diagonal pivoting (largest remaining diagonal entry, the earlier one on a tie);
    a zero pivot leaves its component 0."""
    M = np.array(M, np.float64); b = np.array(b, np.float64)
    n = M.shape[0]
    r = np.arange(n)
    perm = np.tile(np.arange(3), (n, 1))
    p0 = np.argmax(np.abs(M[:, [0, 1, 2], [0, 1, 2]]), axis=1)
    order = np.tile(np.arange(3), (n, 1))
    order[r, 0] = p0; order[r, p0] = 0
    M = M[r[:, None, None], order[:, :, None], order[:, None, :]]; b = b[r[:, None], order]; perm = perm[r[:, None], order]
    with np.errstate(divide="ignore", invalid="ignore"):
        i0 = np.where(M[:, 0, 0] != 0, 1.0 / M[:, 0, 0], 0.0)
        l1, l2 = M[:, 0, 1] * i0, M[:, 0, 2] * i0
        s11 = M[:, 1, 1] - l1 * M[:, 0, 1]; s12 = M[:, 1, 2] - l1 * M[:, 0, 2]; s22 = M[:, 2, 2] - l2 * M[:, 0, 2]
        sw = np.abs(s22) > np.abs(s11)
        s11, s22 = np.where(sw, s22, s11), np.where(sw, s11, s22)
        l1, l2 = np.where(sw, l2, l1), np.where(sw, l1, l2)
        b1, b2 = np.where(sw, b[:, 2], b[:, 1]), np.where(sw, b[:, 1], b[:, 2])
        q1, q2 = np.where(sw, perm[:, 2], perm[:, 1]), np.where(sw, perm[:, 1], perm[:, 2])
        i1 = np.where(s11 != 0, 1.0 / s11, 0.0)
        l21 = s12 * i1
        d2 = s22 - l21 * s12
        i2 = np.where(d2 != 0, 1.0 / d2, 0.0)
    y0 = b[:, 0]; y1 = b1 - l1 * y0; y2 = b2 - l2 * y0 - l21 * y1
    x2 = y2 * i2; x1 = y1 * i1 - l21 * x2; x0 = y0 * i0 - l1 * x1 - l2 * x2
    x = np.zeros((n, 3))
    x[r, perm[:, 0]] = x0; x[r, q1] = x1; x[r, q2] = x2
    return x


def gradient_rows(oracle, pts, normals, colors, radius, max_nn):
    """A (N, max_nn, 3), b (N, max_nn), nn (N) and the neighbour index rows of the colour-gradient least squares of every point: the hybrid search's
    neighbours in the k-d tree's order (d^2, index); row k - 1 for neighbour k = 1 .. nn - 1, the last row (nn - 1) n; unused rows are zero."""
    pts = np.asarray(pts, np.float64); nrm = np.asarray(normals, np.float64); I = intensity(colors)
    idx, d2, cnt = oracle.knn(pts, pts, max_nn, radius)
    n = len(pts)
    rows = np.arange(n)[:, None]
    valid = np.arange(max_nn)[None, :] < cnt[:, None]
    d2s = np.where(valid, d2, np.inf); ids = np.where(valid, idx, np.iinfo(np.int64).max)
    order = np.lexsort((ids, d2s), axis=1)
    idx = np.take_along_axis(idx, order, 1); valid = np.take_along_axis(valid, order, 1)
    nb = np.where(valid, idx, 0)
    v = pts[nb] - pts[:, None, :]
    vn = (v * nrm[:, None, :]).sum(2)
    A = v - vn[:, :, None] * nrm[:, None, :]
    b = I[nb] - I[:, None]
    use = valid.copy(); use[:, 0] = False                     # the first neighbour is the point itself
    A = np.where(use[:, :, None], A, 0.0); b = np.where(use, b, 0.0)
    A = np.concatenate([A[:, 1:], np.zeros((n, 1, 3))], axis=1); b = np.concatenate([b[:, 1:], np.zeros((n, 1))], axis=1)
    nn = cnt.astype(np.int64)
    has = nn >= 1
    A[rows[has, 0], nn[has] - 1] = (nn[has] - 1)[:, None] * nrm[has]
    return A, b, nn, np.where(valid, idx, -1)


def reference_gradient(oracle, pts, normals, colors, radius, max_nn):
    """Float64 colour gradients by LDLT of the normal equations (nn < 4: zero), the same rows solved by numpy.linalg.lstsq, nn, neighbour rows."""
    A, b, nn, nbr = gradient_rows(oracle, pts, normals, colors, radius, max_nn)
    M = np.einsum("nki,nkj->nij", A, A); rhs = np.einsum("nki,nk->ni", A, b)
    d = ldlt3(M, rhs)
    d[nn < 4] = 0.0
    d_ls = np.zeros_like(d)
    for i in np.nonzero(nn >= 4)[0]:
        d_ls[i] = np.linalg.lstsq(A[i, : nn[i]], b[i, : nn[i]], rcond=None)[0]
    return d, d_ls, nn, nbr


def _weights(loss, k, r):
    if loss == "l1":
        return 1.0 / np.abs(r)
    if loss == "gm":
        return k / (k + r * r) ** 2
    return np.ones_like(r)


def reference_colored_icp(oracle, src, src_colors, tgt, tgt_normals, tgt_colors, grad, max_dist, T0, lam=0.968, loss="l2", k=1.0, max_it=30, rel=1e-6):
    """RegistrationICP in float64 with the two-row update of TransformationEstimationForColoredICP over the given gradients."""
    tgt = np.asarray(tgt, np.float64); n = np.asarray(tgt_normals, np.float64); d = np.asarray(grad, np.float64)
    Is, It = intensity(src_colors), intensity(tgt_colors)
    sl, sp = np.sqrt(lam), np.sqrt(1.0 - lam)
    T = np.array(T0, np.float64)
    Pts = np.asarray(src, np.float64) @ T[:3, :3].T + T[:3, 3]
    corr, fit, rmse = oracle.find_correspondences(Pts, tgt, max_dist)
    it, converged = 0, False
    while it < max_it:
        U = np.eye(4)
        if len(corr):
            s, t, nn, dd = Pts[corr[:, 0]], tgt[corr[:, 1]], n[corr[:, 1]], d[corr[:, 1]]
            sd = ((s - t) * nn).sum(1)
            rg = sl * sd
            Jg = sl * np.concatenate([np.cross(s, nn), nn], axis=1)
            sproj = s - sd[:, None] * nn
            dm = -dd + (dd * nn).sum(1)[:, None] * nn
            ri = sp * (Is[corr[:, 0]] - ((dd * (sproj - t)).sum(1) + It[corr[:, 1]]))
            Ji = sp * np.concatenate([np.cross(s, dm), dm], axis=1)
            wg, wi = _weights(loss, k, rg), _weights(loss, k, ri)
            JTJ = (Jg * wg[:, None]).T @ Jg + (Ji * wi[:, None]).T @ Ji
            JTr = (Jg * (wg * rg)[:, None]).sum(0) + (Ji * (wi * ri)[:, None]).sum(0)
            U, _ = oracle.solve_update(JTJ, JTr)
        T = U @ T
        Pts = Pts @ U[:3, :3].T + U[:3, 3]
        before = (fit, rmse)
        corr, fit, rmse = oracle.find_correspondences(Pts, tgt, max_dist)
        it += 1
        if abs(before[0] - fit) < rel and abs(before[1] - rmse) < rel:
            converged = True
            break
    return T, fit, rmse, it, converged, len(corr)


def _est(P, lam=0.968, loss="l2", k=1.0):
    R = P.registration
    return R.TransformationEstimationForColoredICP(lam, {"l2": R.L2Loss(), "l1": R.L1Loss(), "gm": R.GMLoss(k)}[loss])


@pytest.fixture(scope="module")
def target_gradients(P, oracle, colored_clouds):
    """Device gradients of the target (float32) and the restatement's on the same float32 points / normals / colours, search (1.2, 30)."""
    _, tgt = colored_clouds
    dev = P.registration.color_gradient(tgt, P.KDTreeSearchParamHybrid(1.2, 30))
    ref, ref_ls, nn, nbr = reference_gradient(oracle, tgt.points, tgt.normals, tgt.colors, 1.2, 30)
    return dev, ref, ref_ls, nn, nbr


@pytest.fixture(scope="module")
def pose_bound(oracle, small_pair, colored_clouds, target_gradients):
    """The method's sensitivity to storing gradients in float32: how far the restatement's end pose (40 iterations from T_fgr) moves when its own
    float64 gradients are rounded to float32 and back; the bound is three times that or the point-to-plane test's 1e-7 rad / 1e-6 m."""
    src, tgt = colored_clouds
    _, ref, _, _, _ = target_gradients
    args = (oracle, src.points, src.colors, tgt.points, tgt.normals, tgt.colors)
    worst = [0.0, 0.0]
    for lam in (0.968, 0.5):
        A = reference_colored_icp(*args, ref, 0.6, small_pair["T_fgr"], lam, max_it=40)[0]
        B = reference_colored_icp(*args, ref.astype(np.float32).astype(np.float64), 0.6, small_pair["T_fgr"], lam, max_it=40)[0]
        ang, dt = pose_error(A, B)
        worst = [max(worst[0], ang), max(worst[1], dt)]
    bound = (max(3.0 * worst[0], 1e-7), max(3.0 * worst[1], 1e-6))
    print(f"colored ICP pose sensitivity to float32 gradients: {worst[0]:.2e} rad {worst[1]:.2e} m -> bound {bound[0]:.2e} rad {bound[1]:.2e} m")
    return bound


# ------------------------------------------------------------------------------------------ 1. voxel colours
def test_voxel_colors_and_carriers(P, small_pair):
    import copy
    xyz = np.asarray(small_pair["target"], np.float32)
    pc = P.PointCloud(xyz)
    pc.estimate_normals(P.KDTreeSearchParamKNN(knn=10))
    nrm = pc.normals
    plain = P.PointCloud(xyz); plain.normals = nrm
    pc.colors = texture(xyz)
    assert pc.has_colors() and not plain.has_colors()
    v, vp = pc.voxel_down_sample(0.3), plain.voxel_down_sample(0.3)
    assert v.has_colors() and v.has_normals() and not vp.has_colors()
    assert v.device_xyz().cpu().numpy().tobytes() == vp.device_xyz().cpu().numpy().tobytes()
    assert v.device_normals().cpu().numpy().tobytes() == vp.device_normals().cpu().numpy().tobytes()
    # Open3D's key rule: floor((p - (min_bound - v / 2)) / v) in float64
    p64 = xyz.astype(np.float64)
    org = p64.min(0) - 0.15
    keys = np.floor((p64 - org) / 0.3).astype(np.int64)
    uniq, inv = np.unique(keys, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    cnt = np.bincount(inv, minlength=len(uniq)).astype(np.float64)
    c64 = pc.colors
    mean = np.stack([np.bincount(inv, weights=c64[:, k], minlength=len(uniq)) for k in range(3)], axis=1) / cnt[:, None]
    okeys = np.floor((np.asarray(v.points) - org) / 0.3).astype(np.int64)
    look = {tuple(k): i for i, k in enumerate(uniq)}
    rows = np.array([look[tuple(k)] for k in okeys])
    assert len(rows) == len(uniq) and len(np.unique(rows)) == len(uniq)
    err = np.abs(v.colors - mean[rows]).max()
    print(f"voxel colour means: {len(uniq)} voxels, max |device - numpy| = {err:.2e}")
    assert err <= 1e-6
    # colours alone (no normals) ride in the attribute slot of the one pass: the same means as from the pass of their own
    bare = P.PointCloud(xyz); bare.colors = texture(xyz)
    vb = bare.voxel_down_sample(0.3)
    assert vb.device_xyz().cpu().numpy().tobytes() == vp.device_xyz().cpu().numpy().tobytes()
    assert vb.device_colors().cpu().numpy().tobytes() == v.device_colors().cpu().numpy().tobytes() and not vb.has_normals()
    # SOR, select_by_index, deepcopy and random_down_sample carry colours row for row; transform leaves them; new points drop them
    kept, index = v.remove_statistical_outlier(30, 1.0)
    assert kept.has_colors() and np.array_equal(kept.colors, v.colors[index]) and np.array_equal(kept.points, v.points[index])
    sel = v.select_by_index([5, 3, 100])
    assert np.array_equal(sel.colors, v.colors[[5, 3, 100]])
    inv_sel = v.select_by_index([0, 1], invert=True)
    assert np.array_equal(inv_sel.colors, v.colors[2:])
    dc = copy.deepcopy(v)
    assert np.array_equal(dc.colors, v.colors) and dc.device_colors().data_ptr() != v.device_colors().data_ptr()
    rs = v.random_down_sample(0.25, seed=3)
    assert rs.has_colors() and len(rs.colors) == len(rs)
    # every sampled row is a (point, colour) row of v
    both = {(tuple(a), tuple(b)) for a, b in zip(v.points.tolist(), v.colors.tolist())}
    assert all((tuple(a), tuple(b)) in both for a, b in zip(rs.points.tolist(), rs.colors.tolist()))
    before = dc.colors
    dc.transform(np.asarray(small_pair["T_fgr"]))
    assert np.array_equal(dc.colors, before)
    dc.points = v.points[:10]
    assert not dc.has_colors() and dc.colors.shape == (0, 3)
    short = P.PointCloud(xyz[:100]); short.colors = texture(xyz[:50])
    assert not short.has_colors()
    assert short.paint_uniform_color([1.0, 0.706, 0.0]) is short and short.has_colors()
    assert np.array_equal(short.colors, np.tile(np.float32([1.0, 0.706, 0.0]).astype(np.float64), (100, 1)))


# ------------------------------------------------------------------------------------------ 2. gradient
def test_color_gradient_matches_restatement(colored_clouds, target_gradients):
    """Device gradients against the restatement on the same float32 inputs; the figures measured on MI355X are in DESIGN.md section 4.7."""
    P_ = pkg()
    _, tgt = colored_clouds
    dev, ref, ref_ls, nn, nbr = target_gradients
    n = len(ref)
    few = nn < 4
    print(f"gradient search (1.2, 30): {few.sum()} of {n} rows with fewer than 4 neighbours ({few.mean():.2%}), median {int(np.median(nn))}")
    assert few.mean() <= 0.01
    assert np.isfinite(dev).all()
    assert (dev[few] == 0).all()
    # rows whose device neighbour set differs from the oracle's (a d^2 tie at the rim or at the 30th place) are left out
    lib = P_._lib
    import ctypes as C
    import torch
    ctx = lib.Context.current()
    didx = torch.empty((n, 30), dtype=torch.int32, device="cuda"); dd2 = torch.empty((n, 30), dtype=torch.float32, device="cuda")
    dcnt = torch.empty(n, dtype=torch.int32, device="cuda")
    ctx.check(ctx.lib.pcr_debug_knn(ctx.handle, C.c_void_p(tgt.device_xyz().data_ptr()), C.c_int64(n), C.c_int(30), C.c_double(1.2),
                                    C.c_void_p(didx.data_ptr()), C.c_void_p(dd2.data_ptr()), C.c_void_p(dcnt.data_ptr())), "pcr_debug_knn")
    torch.cuda.synchronize()
    dsets = np.sort(didx.cpu().numpy().astype(np.int64), axis=1); osets = np.sort(nbr, axis=1)
    same = (dsets == osets).all(axis=1)
    print(f"rows left out for another neighbour set: {(~same).sum()} of {n}")
    assert (~same).mean() <= 0.001
    # the restatement's own sensitivity: the same rows solved by lstsq on A, b against the LDLT of the normal equations
    cmp_ = same & ~few
    scale = 1.0 + np.abs(ref).max(axis=1)
    sens = (np.abs(ref_ls - ref).max(axis=1) / scale)[cmp_].max()
    tol = 3.0 * sens + F32_ROUND
    err = (np.abs(dev.astype(np.float64) - ref).max(axis=1) / scale)[cmp_]
    print(f"gradient: lstsq-vs-LDLT sensitivity {sens:.3e}, tolerance {tol:.3e}, device max error {err.max():.3e} over {cmp_.sum()} rows, max |d| {np.abs(ref).max():.3e}")
    assert err.max() <= tol


# ------------------------------------------------------------------------------------------ 3. trajectory
@pytest.mark.parametrize("lam", [0.968, 0.5])
def test_trajectory_matches_restatement(P, oracle, small_pair, colored_clouds, target_gradients, pose_bound, lam):
    src, tgt = colored_clouds
    dev_grad = target_gradients[0].astype(np.float64)          # the device's float32 gradients: this test isolates the iteration
    T0 = small_pair["T_fgr"]
    for max_it in (1, 5, 40):
        crit = P.registration.ICPConvergenceCriteria(1e-6, 1e-6, max_it)
        res = P.registration.registration_colored_icp(src, tgt, 0.6, T0, _est(P, lam), crit)
        T, fit, rmse, it, conv, nc = reference_colored_icp(oracle, src.points, src.colors, tgt.points, tgt.normals, tgt.colors, dev_grad, 0.6, T0, lam,
                                                           max_it=max_it)
        ang, dt = pose_error(res.transformation, T)
        print(f"lambda {lam} max_it {max_it}: {res.iterations} iterations, pose error {ang:.2e} rad {dt:.2e} m (bound {pose_bound[0]:.2e} / {pose_bound[1]:.2e})")
        assert ang < pose_bound[0] and dt < pose_bound[1], (max_it, ang, dt)
        assert res.iterations == it and res.converged == conv, (max_it, res.iterations, it, res.converged, conv)
        assert abs(res.fitness - fit) < 1e-12 and abs(res.inlier_rmse - rmse) < 1e-9
        cs = res.correspondence_set
        assert len(cs) == nc
        assert cs.shape == (nc, 2) and len(np.unique(cs[:, 0])) == nc and cs[:, 0].max() < len(src) and cs[:, 1].max() < len(tgt)


@pytest.mark.parametrize("loss", ["l1", "gm"])
def test_robust_kernels(P, oracle, small_pair, colored_clouds, target_gradients, loss):
    src, tgt = colored_clouds
    dev_grad = target_gradients[0].astype(np.float64)
    T0 = small_pair["T_fgr"]
    crit = P.registration.ICPConvergenceCriteria(1e-6, 1e-6, 3)
    res = P.registration.registration_colored_icp(src, tgt, 0.6, T0, _est(P, 0.968, loss, 0.5), crit)
    T, *_ = reference_colored_icp(oracle, src.points, src.colors, tgt.points, tgt.normals, tgt.colors, dev_grad, 0.6, T0, 0.968, loss=loss, k=0.5, max_it=3)
    ang, dt = pose_error(res.transformation, T)
    print(f"{loss}: pose error {ang:.2e} rad {dt:.2e} m")
    assert ang < 1e-6 and dt < 1e-5, (loss, ang, dt)
    l2 = P.registration.registration_colored_icp(src, tgt, 0.6, T0, _est(P), crit)
    assert not np.allclose(res.transformation, l2.transformation, rtol=0, atol=1e-9)


# ------------------------------------------------------------------------------------------ 4. lambda = 1 is point-to-plane
def test_lambda_one_is_point_to_plane(P, small_pair, colored_clouds, pose_bound):
    src, tgt = colored_clouds
    R = P.registration
    T0 = small_pair["T_fgr"]
    for max_it in (5, 40):
        crit = R.ICPConvergenceCriteria(1e-6, 1e-6, max_it)
        a = R.registration_colored_icp(src, tgt, 0.6, T0, R.TransformationEstimationForColoredICP(1.0), crit)
        b = R.registration_icp(src, tgt, 0.6, T0, R.TransformationEstimationPointToPlane(), crit)
        ang, dt = pose_error(a.transformation, b.transformation)
        print(f"lambda 1 against point-to-plane, max_it {max_it}: {ang:.2e} rad {dt:.2e} m, {a.iterations} / {b.iterations} iterations")
        assert a.iterations == b.iterations and a.converged == b.converged
        assert ang < pose_bound[0] and dt < pose_bound[1]
    # and registration_icp dispatches to it
    crit = R.ICPConvergenceCriteria(1e-6, 1e-6, 5)
    c = R.registration_icp(src, tgt, 0.6, T0, R.TransformationEstimationForColoredICP(0.9), crit)
    d = R.registration_colored_icp(src, tgt, 0.6, T0, R.TransformationEstimationForColoredICP(0.9), crit)
    assert c.transformation.tobytes() == d.transformation.tobytes() and c.iterations == d.iterations


# ------------------------------------------------------------------------------------------ 5. colour decides what geometry cannot
PATCH_PERIODS = np.array([1.3, 1.9, 2.6])       # m; the 0.058 m offset is 1/22 of the shortest: far inside the texture's linear range
PATCH_DIST = 0.15                               # max_correspondence_distance; gradients over Hybrid(0.3, 30), about 0.15 m of a 0.05 m lattice


def planar_patch():
    """141 x 141 points on a 0.05 m lattice (7 m x 7 m, 19881 points), jittered by up to 0.015 m in the plane, z = 0, normals +z."""
    rng = np.random.default_rng(11)
    g = np.arange(141) * 0.05
    xy = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2) + rng.uniform(-0.015, 0.015, (141 * 141, 2))
    pts = np.concatenate([xy, np.zeros((len(xy), 1))], axis=1).astype(np.float32)
    nrm = np.tile(np.float32([0, 0, 1]), (len(pts), 1))
    return pts, nrm


def test_color_recovers_an_in_plane_shift(P, oracle, pose_bound):
    R = P.registration
    pts, nrm = planar_patch()
    off = np.array([0.05, 0.03, 0.0])
    col = texture(pts, PATCH_PERIODS)
    tgt = P.PointCloud(pts); tgt.normals = nrm; tgt.colors = col
    src = P.PointCloud((pts.astype(np.float64) + off).astype(np.float32)); src.colors = col
    crit = R.ICPConvergenceCriteria(1e-6, 1e-6, 50)
    # geometry alone: nothing in the plane is observable
    pl = R.registration_icp(src, tgt, PATCH_DIST, np.eye(4), R.TransformationEstimationPointToPlane(), crit)
    moved = np.linalg.norm(pl.transformation[:2, 3])
    print(f"point-to-plane: in-plane motion {moved:.2e} m of the {np.linalg.norm(off):.3f} m offset, {pl.iterations} iterations")
    assert moved <= 0.1 * np.linalg.norm(off)
    # the restatement recovers the shift ...
    grad, grad_ls, _, _ = reference_gradient(oracle, tgt.points, tgt.normals, tgt.colors, 2 * PATCH_DIST, 30)
    dev_grad = R.color_gradient(tgt, P.KDTreeSearchParamHybrid(2 * PATCH_DIST, 30)).astype(np.float64)
    # the device's gradients of the patch against the restatement's, by the rule of the gradient test (three times the lstsq-vs-LDLT sensitivity
    # plus one float32 rounding); a row whose 30th neighbour is a d^2 tie may hold another set: at most 0.1 % of the rows may miss the bound
    scale = 1.0 + np.abs(grad).max(axis=1)
    gtol = 3.0 * (np.abs(grad_ls - grad).max(axis=1) / scale).max() + F32_ROUND
    gerr = np.abs(dev_grad - grad).max(axis=1) / scale
    print(f"patch gradients: tolerance {gtol:.3e}, device max error {gerr.max():.3e}, rows over it {(gerr > gtol).sum()} of {len(gerr)}")
    assert (gerr > gtol).mean() <= 0.001
    T, fit, rmse, it, conv, nc = reference_colored_icp(oracle, src.points, src.colors, tgt.points, tgt.normals, tgt.colors, dev_grad, PATCH_DIST, np.eye(4),
                                                       max_it=50)
    left = np.linalg.norm(T[:2, 3] + off[:2])
    print(f"restatement: {it} iterations, in-plane error {left:.2e} m; max |device - restatement gradient| {np.abs(dev_grad - grad).max():.2e}")
    assert left < 0.1 * np.linalg.norm(off)
    # ... and the device ends where the restatement does
    res = R.registration_colored_icp(src, tgt, PATCH_DIST, np.eye(4), R.TransformationEstimationForColoredICP(), crit)
    ang, dt = pose_error(res.transformation, T)
    print(f"device: {res.iterations} iterations, pose error against the restatement {ang:.2e} rad {dt:.2e} m")
    assert ang < pose_bound[0] and dt < pose_bound[1]
    assert res.iterations == it and res.converged == conv


# ------------------------------------------------------------------------------------------ 6. errors and degenerate input
def test_errors_and_degenerate(P, colored_clouds):
    src, tgt = colored_clouds
    R = P.registration
    icp = R.registration_colored_icp
    with pytest.raises(RuntimeError):
        icp(src, tgt, 0.0)
    no_normals = P.PointCloud(tgt.points); no_normals.colors = tgt.colors
    with pytest.raises(RuntimeError, match="normal"):
        icp(src, no_normals, 0.6)
    no_colors = P.PointCloud(tgt.points); no_colors.normals = tgt.normals
    with pytest.raises(RuntimeError, match="colors for target"):
        icp(src, no_colors, 0.6)
    with pytest.raises(RuntimeError, match="colors for source"):
        icp(P.PointCloud(src.points), tgt, 0.6)
    with pytest.raises(RuntimeError):
        icp(src, tgt, 0.6, np.eye(4), R.TransformationEstimationPointToPlane())
    far = P.PointCloud(tgt.points + 1000.0); far.normals = tgt.normals; far.colors = tgt.colors
    res = icp(src, far, 0.5)
    assert res.fitness == 0 and res.inlier_rmse == 0 and np.array_equal(res.transformation, np.eye(4))
    assert res.converged and res.iterations == 1 and len(res.correspondence_set) == 0
    empty = P.PointCloud(np.zeros((0, 3)))
    res = icp(empty, tgt, 0.5)
    assert res.fitness == 0 and np.array_equal(res.transformation, np.eye(4))
    assert res.converged and res.iterations == 1


# ------------------------------------------------------------------------------------------ 7. graphs
def test_lambda_and_estimator_are_part_of_the_graph_key(P, small_pair, colored_clouds):
    src, tgt = colored_clouds
    R = P.registration
    T0 = small_pair["T_fgr"]
    crit = R.ICPConvergenceCriteria(1e-6, 1e-6, 30)
    runs = [("c968", R.TransformationEstimationForColoredICP(0.968)), ("p2pl", R.TransformationEstimationPointToPlane()),
            ("c5", R.TransformationEstimationForColoredICP(0.5)), ("c968", R.TransformationEstimationForColoredICP(0.968)),
            ("p2pl", R.TransformationEstimationPointToPlane()), ("c5", R.TransformationEstimationForColoredICP(0.5)),
            ("c968", R.TransformationEstimationForColoredICP(0.968))]
    first = {}
    for name, est in runs:
        r = R.registration_icp(src, tgt, 0.6, T0, est, crit)
        key = (r.transformation.tobytes(), r.iterations, r.fitness, r.inlier_rmse, r.correspondence_set.tobytes())
        if name in first:
            assert key == first[name], name
        first.setdefault(name, key)
    assert len({first[k][0] for k in first}) == 3


# ------------------------------------------------------------------------------------------ 8. switches
def test_switches_do_not_change_the_result():
    """Skip certificates, cell hash or octree, hipGraph replay: the same arithmetic scheduled another way, the same bits (the switches are
    latched per process: one child process each)."""
    lines = []
    for env in ({}, {"PCR_ICP_SKIP": "0"}, {"PCR_ICP_GRID": "0"}, {"PCR_ICP_GRAPH": "0"}):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "colored_icp_pose.py")], env=dict(os.environ, **env), capture_output=True,
                             text=True, timeout=300)
        assert out.returncode == 0, (env, out.stderr[-2000:])
        got = [l for l in out.stdout.splitlines() if l.split(" ")[0] in ("C968", "C500")]
        assert len(got) == 2, out.stdout[-2000:]
        lines.append((env, got))
    for env, got in lines[1:]:
        assert got == lines[0][1], (env, got, lines[0][1])
