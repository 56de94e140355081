"""GPU checks of RANSAC global registration (registration_ransac_based_on_correspondence / _feature_matching).

Open3D is not installed and the reference never calls RANSAC, so the float64 restatement of the algorithm stated in include/pcr_hip.h
lives here: numpy draws by the splitmix64 formula, the checkers, an SVD Umeyama (Eigen's algorithm), the scores and the sequential
better-than / stop loop.  Hypotheses are compared by CERTIFICATE (a degenerate sample has many minimisers, any of them is legitimate):
the device's T must be a rotation (times a scale) that fits the sample as well as numpy's fit does, and the device's score must be the
float64 recount under the device's own T.  Inputs: golden pair 899 with Hybrid(0.2, 20) normals and FPFH Hybrid(1.0, 200)."""
import ctypes as C
import math
import threading

import numpy as np
import pytest

from conftest import TOL_M, TOL_RAD, pkg, pose_error

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
D_MIXED = 0.5          # max_correspondence_distance of the hypothesis / loop tests (every source point with its nearest target feature)


@pytest.fixture(scope="module")
def P():
    return pkg()


@pytest.fixture(scope="module")
def inputs(P, small_pair):
    """(source, target) clouds with normals, their FPFH features, and the two nearest-feature maps from pcr_debug_feature_nn."""
    import torch
    out = []
    for key in ("source", "target"):
        pc = P.PointCloud(small_pair[key])
        pc.estimate_normals(P.KDTreeSearchParamHybrid(radius=0.2, max_nn=20))
        feat = P.registration.compute_fpfh_feature(pc, P.KDTreeSearchParamHybrid(radius=1.0, max_nn=200))
        out.append((pc, feat))
    (src, fs), (tgt, ft) = out
    s_to_t, t_to_s = _feature_maps(P, fs._dev, ft._dev)
    corres = np.stack([np.arange(len(src), dtype=np.int32), s_to_t.astype(np.int32)], axis=1)
    return dict(src=src, tgt=tgt, fs=fs, ft=ft, s_to_t=s_to_t, t_to_s=t_to_s, corres=corres,
                sx=src.device_xyz().cpu().numpy().astype(np.float64), tx=tgt.device_xyz().cpu().numpy().astype(np.float64),
                sn=src.device_normals().cpu().numpy().astype(np.float64), tn=tgt.device_normals().cpu().numpy().astype(np.float64))


def _feature_maps(P, fs_dev, ft_dev, mode=0):
    """source row -> nearest target row and target row -> nearest source row (both directions in full; mode 0: the production search,
    2: the brute-force one small clouds take)."""
    import torch
    ctx = P._lib.Context.current()
    ns, nt = int(fs_dev.shape[0]), int(ft_dev.shape[0])
    s_to_t = torch.full((ns,), -7, dtype=torch.int32, device="cuda"); t_to_s = torch.full((nt,), -7, dtype=torch.int32, device="cuda")
    ctx.check(ctx.lib.pcr_debug_feature_nn(ctx.handle, C.c_void_p(ft_dev.data_ptr()), C.c_int64(nt), C.c_void_p(fs_dev.data_ptr()), C.c_int64(ns),
                                           C.c_void_p(s_to_t.data_ptr()), C.c_void_p(t_to_s.data_ptr()), C.c_int(mode)), "pcr_debug_feature_nn")
    return s_to_t.cpu().numpy().astype(np.int64), t_to_s.cpu().numpy().astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------- restatement
def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def draw_rows(seed, n, first, count, n_corres):
    return np.array([[splitmix64((seed + n * i + k) & M64) % n_corres for k in range(n)] for i in range(first, first + count)], dtype=np.int64)


def umeyama(S, T, scaling):
    """Eigen::umeyama(src, dst, with_scaling) on n x 3 float64 arrays."""
    n = len(S)
    ms, mt = S.mean(0), T.mean(0)
    Sc, Tc = S - ms, T - mt
    sigma = Tc.T @ Sc / n
    U, D, Vt = np.linalg.svd(sigma)
    sgn = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        sgn[2] = -1.0
    R = U @ np.diag(sgn) @ Vt
    c = 1.0
    if scaling:
        with np.errstate(divide="ignore", invalid="ignore"):
            c = float((D * sgn).sum() / ((Sc * Sc).sum() / n))
    M = np.eye(4)
    M[:3, :3] = c * R
    M[:3, 3] = mt - c * R @ ms
    return M


def residual(T, S, Tt):
    d = S @ T[:3, :3].T + T[:3, 3] - Tt
    return float((d * d).sum())


def restate_hypothesis(S, Tt, scaling, edge_thr, dist_thr):
    """(valid, rim, fit or None): the decision of the checkers with numpy's own fit; rim = a checker quantity within 1e-9 relative of its threshold."""
    rim = False
    n = len(S)
    if edge_thr is not None:
        ok = True
        for a in range(n):
            for b in range(a + 1, n):
                ls, lt = np.linalg.norm(S[a] - S[b]), np.linalg.norm(Tt[a] - Tt[b])
                for x, y in ((ls, lt * edge_thr), (lt, ls * edge_thr)):
                    if x < y:
                        ok = False
                    if abs(x - y) <= 1e-9 * max(x, y) and max(x, y) > 0:
                        rim = True
        if not ok:
            return False, rim, None
    with np.errstate(all="ignore"):
        try:
            fit = umeyama(S, Tt, scaling)
        except np.linalg.LinAlgError:
            return False, rim, None
    if not np.isfinite(fit).all():
        return False, rim, None
    if dist_thr is not None:
        dis = np.linalg.norm(S @ fit[:3, :3].T + fit[:3, 3] - Tt, axis=1)
        if (np.abs(dis - dist_thr) <= 1e-9 * dist_thr).any():
            rim = True
        if (dis > dist_thr).any():
            return False, rim, fit
    return True, rim, fit


def recount(T, ps, pt, d):
    """float64 inlier mask, rim mask and sum of squared inlier distances of one pose over the whole list."""
    dis = np.linalg.norm(ps @ T[:3, :3].T + T[:3, 3] - pt, axis=1)
    rim = np.abs(dis - d) <= 1e-9 * d
    inl = dis < d
    return inl, rim, float(math.fsum((dis[inl & ~rim] ** 2).tolist()))


def rmse_of(count, err2):
    return math.sqrt(err2 / count)


def sequential_loop(valid, count, err2, n_corres, n, max_iteration, confidence):
    """The sequential better-than and stop rule over per-hypothesis (valid, count, err2) -> (best_iteration, iterations_run, n_valid)."""
    est_k, best, bc, be, i, n_valid = max_iteration, -1, 0, 0.0, 0, 0
    while i < est_k:
        if valid[i]:
            n_valid += 1
            c, e = int(count[i]), float(err2[i])
            if c > 0 and (c > bc or (c == bc and rmse_of(c, e) < rmse_of(bc, be))):
                best, bc, be = i, c, e
                rho = c / n_corres
                p = 1.0
                for _ in range(n):
                    p *= rho
                # k' with the denominator as log1p(-p): 1 - p rounds to 1 below p = 1e-16, where k' is huge, not -inf (include/pcr_hip.h)
                with np.errstate(divide="ignore", invalid="ignore"):
                    kp = float(np.log(np.float64(1.0 - confidence)) / np.log1p(np.float64(-p)))
                if p > 0.0 and math.isfinite(kp) and 0.0 <= kp < est_k:
                    est_k = int(math.ceil(kp))
        i += 1
    return best, i, n_valid


# ---------------------------------------------------------------------------------------------------------------- device access
def ransac_params(P, n, scaling, edge, dist, ang, seed, max_iteration=100000, confidence=0.999):
    return P._lib.PcrRansacParams(n, int(scaling), max_iteration, confidence, seed, -1.0 if edge is None else edge, -1.0 if dist is None else dist,
                                  -1.0 if ang is None else ang)


def dump(P, inp, corres, d, params, first, count, normals=False):
    import torch
    ctx = P._lib.Context.current()
    src, tgt = inp["src"], inp["tgt"]
    cd = torch.from_numpy(np.ascontiguousarray(corres.astype(np.int32))).cuda()
    valid = torch.full((count,), 9, dtype=torch.uint8, device="cuda"); T = torch.full((count, 16), float("nan"), dtype=torch.float64, device="cuda")
    inl = torch.full((count,), -9, dtype=torch.int32, device="cuda"); err2 = torch.full((count,), float("nan"), dtype=torch.float64, device="cuda")
    ctx.check(ctx.lib.pcr_debug_ransac_hypotheses(
        ctx.handle, C.c_void_p(src.device_xyz().data_ptr()), C.c_void_p(src.device_normals().data_ptr() if normals else 0), C.c_int64(len(src)),
        C.c_void_p(tgt.device_xyz().data_ptr()), C.c_void_p(tgt.device_normals().data_ptr() if normals else 0), C.c_int64(len(tgt)),
        C.c_void_p(cd.data_ptr()), C.c_int64(len(corres)), C.c_double(d), C.byref(params), C.c_int64(first), C.c_int64(count),
        C.c_void_p(valid.data_ptr()), C.c_void_p(T.data_ptr()), C.c_void_p(inl.data_ptr()), C.c_void_p(err2.data_ptr())), "pcr_debug_ransac_hypotheses")
    return valid.cpu().numpy(), T.cpu().numpy().reshape(count, 4, 4), inl.cpu().numpy(), err2.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------- 1. hypotheses
@pytest.mark.parametrize("checkers", [False, True], ids=["nocheck", "edge+dist"])
@pytest.mark.parametrize("scaling", [False, True], ids=["rigid", "scaled"])
@pytest.mark.parametrize("n", [3, 4])
def test_hypotheses_by_certificate(P, inputs, n, scaling, checkers):
    corres, d = inputs["corres"], D_MIXED
    nc = len(corres)
    ps, pt = inputs["sx"][corres[:, 0]], inputs["tx"][corres[:, 1]]
    seed, first, count = 0xC0FFEE + 17 * n, 1000, 4096
    edge, dist = (0.9, d) if checkers else (None, None)
    valid, T, inl, err2 = dump(P, inputs, corres, d, ransac_params(P, n, scaling, edge, dist, None, seed), first, count)
    assert set(np.unique(valid)) <= {0, 1}
    rows = draw_rows(seed, n, first, count, nc)
    n_rim_flag = n_fit_checked = n_scored = n_scored_clean = 0
    for h in range(count):
        S, Tt = ps[rows[h]], pt[rows[h]]
        ok, rim, fit = restate_hypothesis(S, Tt, scaling, edge, dist)
        # ---- valid flag against the restatement's decision (left out only on the rim of a checker threshold)
        if rim:
            n_rim_flag += 1
        else:
            assert bool(valid[h]) == ok, (h, valid[h], ok)
        assert (inl[h] >= 0) == bool(valid[h]) and (valid[h] or err2[h] == 0.0)
        # ---- transformation: a rotation (times a scale) that fits the sample as well as numpy's minimiser
        if fit is not None and np.isfinite(T[h]).all() and (valid[h] or not rim):
            A = T[h][:3, :3]
            det = np.linalg.det(A)
            if not (scaling and np.cbrt(np.linalg.det(fit[:3, :3])) < 1e-9):      # (every sampled target point the same one: the best scale is 0)
                assert det > 0, (h, det)
                c = np.cbrt(det) if scaling else 1.0
                R = A / c
                assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(R) - 1.0) <= 1e-12, (h, R)
            assert np.array_equal(T[h][3], [0, 0, 0, 1])
            scale2 = float((S * S).sum() + (Tt * Tt).sum())
            assert residual(T[h], S, Tt) <= residual(fit, S, Tt) + 1e-12 * scale2, (h, residual(T[h], S, Tt), residual(fit, S, Tt))
            n_fit_checked += 1
        # ---- score: the float64 recount under the device's own T
        if valid[h]:
            m_in, m_rim, e_ref = recount(T[h], ps, pt, d)
            lo, hi = int((m_in & ~m_rim).sum()), int((m_in | m_rim).sum())
            assert lo <= inl[h] <= hi, (h, inl[h], lo, hi)
            n_scored += 1
            if not m_rim.any():
                assert inl[h] == lo
                assert abs(err2[h] - e_ref) <= 1e-12 * e_ref, (h, err2[h], e_ref)
                n_scored_clean += 1
    print(f"n={n} scaling={scaling} checkers={checkers}: valid {int(valid.sum())} of {count}, rim flags {n_rim_flag}, fits checked {n_fit_checked}, "
          f"scores checked {n_scored} ({n_scored_clean} without a rim row)")
    assert n_rim_flag < 0.001 * count
    assert n_fit_checked > (0 if checkers else 0.99 * count)
    if not checkers:
        assert n_scored > 0.99 * count
    assert n_scored_clean >= 0.99 * n_scored                     # not vacuous: nearly no hypothesis has a row on the rim of d


def test_normal_checker_prunes_by_the_rotated_normals(P, inputs):
    """CorrespondenceCheckerBasedOnNormal alone: the fit does not depend on it (same T bits), and the flag is `every sampled pair has
    (T[:3,:3] n_s) . n_t >= cos(threshold)` under the device's own T (a degenerate sample leaves the rotation about its line free, so numpy's
    fit is no referee here), left out within 1e-9 of the threshold."""
    corres, d, n, seed, count, thr = inputs["corres"], D_MIXED, 3, 4711, 4096, 0.5
    v0, T0, _, _ = dump(P, inputs, corres, d, ransac_params(P, n, False, None, None, None, seed), 0, count, normals=True)
    v1, T1, i1, _ = dump(P, inputs, corres, d, ransac_params(P, n, False, None, None, thr, seed), 0, count, normals=True)
    v2, _, _, _ = dump(P, inputs, corres, d, ransac_params(P, n, False, None, None, thr, seed), 0, count, normals=False)
    assert np.array_equal(T0, T1)
    assert np.array_equal(v2, v0)                              # no normals on the clouds: the checker passes
    rows = draw_rows(seed, n, 0, count, len(corres))
    ns_, nt_ = inputs["sn"][corres[:, 0]], inputs["tn"][corres[:, 1]]
    n_rim = 0
    for h in range(count):
        dots = np.einsum("kj,kj->k", ns_[rows[h]] @ T0[h][:3, :3].T, nt_[rows[h]])
        if (np.abs(dots - math.cos(thr)) <= 1e-9).any():
            n_rim += 1
            continue
        assert bool(v1[h]) == (bool(v0[h]) and bool((dots >= math.cos(thr)).all())), (h, dots)
    assert n_rim < 0.001 * count
    assert 0 < v1.sum() < v0.sum()


RS_TILE, RS_SPLIT_ROWS, RS_MAX_SPLITS = 512, 1024, 64      # csrc/pcr_ransac.hip
BOUNDARY_SEED = 20240607


def lattice_list(rows):
    """A list for the boundary test: source points on a lattice of multiples of 1/8 m; the target of an inlier row is its source point plus
    one translation of multiples of 1/8, every other row is moved at least 4 m further along each axis (by an amount that changes from row to
    row, so that the outliers agree on no second pose).  Every coordinate is exact in float32.  The list pairs source row i with target row
    rows - 1 - i."""
    i = np.arange(rows)
    src = np.stack([i % 37, (i // 37) % 41, i // (37 * 41)], axis=1) / 8.0
    inlier = (i * 7) % 10 < 6
    off = np.stack([32 + i % 7, -(32 + i % 11), 32 + i % 13], axis=1) / 8.0
    tgt = src + np.array([3, -5, 7]) / 8.0 + np.where(inlier[:, None], 0.0, off)
    corres = np.stack([i, rows - 1 - i], axis=1).astype(np.int32)
    return src.astype(np.float32), tgt[::-1].astype(np.float32).copy(), corres


@pytest.mark.parametrize("rows", [RS_TILE - 1, RS_TILE, RS_TILE + 1, RS_SPLIT_ROWS - 1, RS_SPLIT_ROWS, RS_SPLIT_ROWS + 1, 2 * RS_SPLIT_ROWS + 1,
                                  RS_MAX_SPLITS * RS_SPLIT_ROWS + 1])
def test_tile_and_split_boundaries(P, rows):
    """The score at list lengths around a tile, around a split, and one row past RS_MAX_SPLITS * RS_SPLIT_ROWS, from where a lane walks more
    than RS_SPLIT_ROWS rows in several tiles: the count of every valid one of the first 64 hypotheses is numpy's float64 count of
    |T s - t|^2 < d^2 under the device's own T.  No compared row lies within 1e-9 relative of the threshold (asserted; it holds for the
    restatement's fits of these samples too)."""
    d, n, count = 0.1, 3, 64
    src, tgt, corres = lattice_list(rows)
    inp = dict(src=P.PointCloud(src), tgt=P.PointCloud(tgt))
    valid, T, inl, _ = dump(P, inp, corres, d, ransac_params(P, n, False, None, None, None, BOUNDARY_SEED), 0, count)
    ps, pt = src.astype(np.float64)[corres[:, 0]], tgt.astype(np.float64)[corres[:, 1]]
    assert valid.any()
    best = 0
    for h in np.flatnonzero(valid):
        diff = ps @ T[h][:3, :3].T + T[h][:3, 3] - pt
        d2 = (diff * diff).sum(axis=1)
        assert not (np.abs(np.sqrt(d2) - d) <= 1e-9 * d).any(), h
        ref = int((d2 < d * d).sum())
        assert inl[h] == ref, (rows, h, inl[h], ref)
        best = max(best, ref)
    print(f"rows {rows}: {int(valid.sum())} valid of {count}, largest count {best}")
    assert best > 3


# ---------------------------------------------------------------------------------------------------------------- 2. loop
def _check_loop(P, inputs, n, d, checkers, confidence, seed, max_it=20000):
    """Product call against the restated sequential rule run over the device's own per-hypothesis dump (max_it spans more than one round)."""
    R = P.registration
    corres = inputs["corres"]
    nc = len(corres)
    edge, dist = (0.9, d) if checkers else (None, None)
    valid, T, inl, err2 = dump(P, inputs, corres, d, ransac_params(P, n, False, edge, dist, None, seed), 0, max_it)
    best, run, n_valid = sequential_loop(valid, inl, err2, nc, n, max_it, confidence)
    res = R.registration_ransac_based_on_correspondence(
        inputs["src"], inputs["tgt"], corres, d, R.TransformationEstimationPointToPoint(False), n,
        [R.CorrespondenceCheckerBasedOnEdgeLength(0.9), R.CorrespondenceCheckerBasedOnDistance(d)] if checkers else [],
        R.RANSACConvergenceCriteria(max_it, confidence), seed=seed)
    print(f"n={n} d={d} checkers={checkers} confidence={confidence}: restated best {best} run {run} valid {n_valid}; device best {res.best_iteration} "
          f"run {res.iterations} valid {res.n_valid}; fitness {res.fitness:.5f} rmse {res.inlier_rmse:.4f}")
    assert (res.best_iteration, res.iterations, res.n_valid, res.n_corres) == (best, run, n_valid, nc)
    assert best >= 0
    assert np.array_equal(res.transformation, T[best])           # bitwise
    assert res.fitness == inl[best] / nc and res.inlier_rmse == math.sqrt(err2[best] / inl[best])
    ps, pt = inputs["sx"][corres[:, 0]], inputs["tx"][corres[:, 1]]
    m_in, m_rim, _ = recount(T[best], ps, pt, d)
    got = res.correspondence_set
    assert len(got) == inl[best]
    if not m_rim.any():
        assert np.array_equal(got, corres[m_in])                 # the exact row set, in input order
    else:
        keys = set(map(tuple, got.tolist()))
        assert set(map(tuple, corres[m_in & ~m_rim].tolist())) <= keys <= set(map(tuple, corres[m_in | m_rim].tolist()))
        assert np.array_equal(got, np.array(sorted(keys)))
    return run, valid, inl


@pytest.mark.parametrize("confidence", [0.5, 0.999, 1.0])
@pytest.mark.parametrize("checkers", [False, True], ids=["nocheck", "edge+dist"])
def test_loop_is_the_sequential_rule_over_the_device_scores(P, inputs, checkers, confidence):
    run, _, _ = _check_loop(P, inputs, 3, D_MIXED, checkers, confidence, 20240607)
    if confidence == 1.0:
        assert run == 20000
    if confidence == 0.5:
        assert run < 20000                                       # stops early on this pair


@pytest.mark.parametrize("n", [6, 8])
def test_loop_with_a_tiny_inlier_ratio_does_not_stop_on_the_first_inlier(P, inputs, n):
    """ransac_n 6 and 8 at d = 0.05: the first hypothesis with any inlier has a handful of them out of 16526 rows, rho^n is below 1e-16 and
    1 - rho^n rounds to 1.  k' is then astronomically large (log1p), it is not log(1 - conf) / 0: the loop must go on.  With the best inlier
    ratio of the whole dump k' = -log(1 - conf) / rho^n still exceeds max_iteration, so every iteration runs."""
    conf, max_it = 0.999, 20000
    run, valid, inl = _check_loop(P, inputs, n, 0.05, False, conf, 977 + n, max_it)
    nc = len(inputs["corres"])
    first = int(np.nonzero((valid != 0) & (inl > 0))[0][0])
    assert 1.0 - (inl[first] / nc) ** n == 1.0, (first, inl[first])          # the case this test is about
    assert -math.log(1.0 - conf) / (inl.max() / nc) ** n > max_it
    assert run == max_it


# ---------------------------------------------------------------------------------------------------------------- 3. determinism
def _bits(res):
    return (res.transformation.tobytes(), res.fitness, res.inlier_rmse, res.iterations, res.best_iteration, res.correspondence_set.tobytes())


def test_same_seed_same_bits_also_next_to_a_running_fgr(P, inputs, small_pair):
    import torch
    R = P.registration

    def run():
        return _bits(R.registration_ransac_based_on_feature_matching(
            inputs["src"], inputs["tgt"], inputs["fs"], inputs["ft"], True, 0.2, None, 3,
            [R.CorrespondenceCheckerBasedOnEdgeLength(0.9), R.CorrespondenceCheckerBasedOnDistance(0.2)], R.RANSACConvergenceCriteria(40000, 0.999), seed=5))

    quiet = run()
    assert run() == quiet
    stop, errors = threading.Event(), []

    def load():
        try:
            with torch.cuda.stream(torch.cuda.Stream()):
                while not stop.is_set():
                    R.registro_fgr(P.PointCloud(small_pair["source"]), P.PointCloud(small_pair["target"]), 0.1, seed=1)
        except Exception as e:            # noqa: BLE001
            errors.append(e)

    t = threading.Thread(target=load)
    t.start()
    try:
        busy = [run() for _ in range(4)]
    finally:
        stop.set()
        t.join()
    assert not errors, errors
    assert all(b == quiet for b in busy)


# ---------------------------------------------------------------------------------------------------------------- 4. quality
def restated_ransac(ps, pt, n, seed, max_iteration, confidence, edge_thr, dist_thr, d):
    """The whole algorithm on the CPU in float64: (best_iteration, iterations_run, T of the best).  Draws and the edge-length check are
    vectorised (same formulas); the few survivors are fitted, checked and scored one by one."""
    nc = len(ps)
    i = np.arange(max_iteration, dtype=np.uint64)
    rows = np.empty((max_iteration, n), np.int64)
    with np.errstate(over="ignore"):
        for k in range(n):
            x = np.uint64(seed) + np.uint64(n) * i + np.uint64(k) + np.uint64(0x9E3779B97F4A7C15)
            x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
            x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
            rows[:, k] = ((x ^ (x >> np.uint64(31))) % np.uint64(nc)).astype(np.int64)
    assert np.array_equal(rows[:50], draw_rows(seed, n, 0, 50, nc))
    ok = np.ones(max_iteration, bool)
    for a in range(n):
        for b in range(a + 1, n):
            ls = np.linalg.norm(ps[rows[:, a]] - ps[rows[:, b]], axis=1); lt = np.linalg.norm(pt[rows[:, a]] - pt[rows[:, b]], axis=1)
            ok &= ~((ls < lt * edge_thr) | (lt < ls * edge_thr))
    valid = np.zeros(max_iteration, bool); count = np.full(max_iteration, -1, np.int64); err2 = np.zeros(max_iteration); fits = {}
    for h in np.nonzero(ok)[0]:
        v, _, fit = restate_hypothesis(ps[rows[h]], pt[rows[h]], False, None, dist_thr)
        if v:
            m_in, _, _ = recount(fit, ps, pt, d)
            dis2 = ((ps @ fit[:3, :3].T + fit[:3, 3] - pt) ** 2).sum(1)
            valid[h], count[h], err2[h], fits[int(h)] = True, int(m_in.sum()), float(math.fsum(dis2[m_in].tolist())), fit
    best, run, _ = sequential_loop(valid, count, err2, nc, n, max_iteration, confidence)
    return best, run, (fits[best] if best >= 0 else np.eye(4))


def test_registration_quality_after_one_icp_refinement(P, inputs, small_pair):
    """Feature-matching form, mutual filter, EdgeLength(0.9) + Distance(d) checkers, d = 0.2, defaults otherwise, seed 42; then ONE
    registration_icp point-to-point refinement at d (a fixed 100 iterations, relative criteria 0: two starts in one basin must arrive at
    the same fixed point, so the loop may not stop on a small step while still TOL away from it).

    On pair 899 the refined pose does not come within TOL_RAD / TOL_M of the same refinement started from the shipped T_fgr: a RANSAC pose
    is good to about d, and from there a 0.2 m ICP settles in another minimum than from T_fgr.  Whether that is the algorithm on this pair or
    the device is decided as the specification says: the float64 restatement runs on the CPU with the same seed, its figures are printed next
    to the device's, and the device is held to it -- the same best iteration and iteration count, its pose that of numpy's fit of that sample
    to rounding, and its refined pose within TOL_RAD / TOL_M of the refinement of the restatement's pose."""
    R = P.registration
    d, seed = 0.2, 42
    res = R.registration_ransac_based_on_feature_matching(
        inputs["src"], inputs["tgt"], inputs["fs"], inputs["ft"], True, d, R.TransformationEstimationPointToPoint(False), 3,
        [R.CorrespondenceCheckerBasedOnEdgeLength(0.9), R.CorrespondenceCheckerBasedOnDistance(d)], R.RANSACConvergenceCriteria(100000, 0.999), seed=seed)
    crit = R.ICPConvergenceCriteria(0.0, 0.0, 100)

    def refine(T):
        return R.registration_icp(inputs["src"], inputs["tgt"], d, T, R.TransformationEstimationPointToPoint(), crit)

    ref, got = refine(small_pair["T_fgr"]), refine(res.transformation)
    a0, d0 = pose_error(res.transformation, small_pair["T_fgr"])
    a, dm = pose_error(got.transformation, ref.transformation)
    print(f"device RANSAC: {res.n_corres} mutual rows, fitness {res.fitness:.4f} rmse {res.inlier_rmse:.4f}, best {res.best_iteration} of {res.iterations} iterations "
          f"({res.n_valid} valid); to T_fgr {a0:.2e} rad {d0:.2e} m; after ICP against ICP from T_fgr {a:.2e} rad {dm:.2e} m (ICP fitness {got.fitness:.4f} / {ref.fitness:.4f})")
    if a < TOL_RAD and dm < TOL_M:
        return
    s_to_t, t_to_s, corres = inputs["s_to_t"], inputs["t_to_s"], inputs["corres"]
    mutual = corres[t_to_s[s_to_t] == np.arange(len(s_to_t))]
    best, run, T_cpu = restated_ransac(inputs["sx"][mutual[:, 0]], inputs["tx"][mutual[:, 1]], 3, seed, 100000, 0.999, 0.9, d, d)
    cpu = refine(T_cpu)
    ac0, dc0 = pose_error(T_cpu, small_pair["T_fgr"])
    ac, dc = pose_error(cpu.transformation, ref.transformation)
    print(f"CPU restatement, same seed: best {best} of {run} iterations; to T_fgr {ac0:.2e} rad {dc0:.2e} m; after ICP against ICP from T_fgr {ac:.2e} rad {dc:.2e} m")
    assert (res.best_iteration, res.iterations, res.n_corres) == (best, run, len(mutual))
    ar, dr = pose_error(res.transformation, T_cpu)
    assert ar < 1e-9 and dr < 1e-9, (ar, dr)
    ag, dg = pose_error(got.transformation, cpu.transformation)
    print(f"device against restatement: RANSAC pose {ar:.1e} rad {dr:.1e} m, refined pose {ag:.1e} rad {dg:.1e} m")
    assert ag < TOL_RAD and dg < TOL_M, (ag, dg)


# ---------------------------------------------------------------------------------------------------------------- 5. feature form
def test_feature_form_runs_on_the_nearest_feature_list(P, inputs):
    """Huge d, one iteration, no checkers: hypothesis 0 takes every row as an inlier, so correspondence_set IS the list RANSAC ran on."""
    R = P.registration
    s_to_t, t_to_s, corres = inputs["s_to_t"], inputs["t_to_s"], inputs["corres"]
    mutual = corres[t_to_s[s_to_t] == np.arange(len(s_to_t))]
    assert 3 <= len(mutual) < len(corres)
    for flt, want in ((True, mutual), (False, corres)):
        res = R.registration_ransac_based_on_feature_matching(inputs["src"], inputs["tgt"], inputs["fs"], inputs["ft"], flt, 1e6,
                                                              criteria=R.RANSACConvergenceCriteria(1, 0.999), seed=3)
        assert (res.best_iteration, res.iterations, res.n_corres, res.fitness) == (0, 1, len(want), 1.0)
        assert np.array_equal(res.correspondence_set, want)


def test_feature_form_falls_back_when_the_mutual_filter_leaves_too_few(P):
    """Five points a side; every source feature is nearest to target row 0, whose own nearest source row is 0: ONE mutual pair, fewer than
    ransac_n, so the list is all five rows (Open3D: "too few correspondences after mutual filter")."""
    import torch
    R = P.registration
    rng = np.random.default_rng(5)
    src, tgt = P.PointCloud(rng.uniform(-1, 1, (5, 3))), P.PointCloud(rng.uniform(-1, 1, (5, 3)))
    fs = np.zeros((5, 33), np.float32); fs[:, 0] = 0.1 * np.arange(5)
    ft = np.zeros((5, 33), np.float32); ft[1:, 1] = 100.0 * np.arange(1, 5)
    Fs, Ft = R.Feature(torch.as_tensor(fs, device="cuda")), R.Feature(torch.as_tensor(ft, device="cuda"))
    s_to_t, t_to_s = _feature_maps(P, Fs._dev, Ft._dev, mode=2)
    assert np.array_equal(s_to_t, np.zeros(5, np.int64)) and t_to_s[0] == 0
    res = R.registration_ransac_based_on_feature_matching(src, tgt, Fs, Ft, True, 1e6, criteria=R.RANSACConvergenceCriteria(1, 0.999), seed=1)
    assert res.n_corres == 5 and res.iterations == 1
    assert np.array_equal(res.correspondence_set, np.stack([np.arange(5), np.zeros(5, np.int64)], axis=1))


# ---------------------------------------------------------------------------------------------------------------- 6. errors and edges
def _is_empty(res, n_corres):
    return (np.array_equal(res.transformation, np.eye(4)) and res.fitness == 0.0 and res.inlier_rmse == 0.0 and len(res.correspondence_set) == 0
            and res.best_iteration == -1 and res.iterations == 0 and res.n_corres == n_corres)


def test_errors_and_edges(P, inputs):
    import torch
    R = P.registration
    src, tgt, fs, ft, corres = inputs["src"], inputs["tgt"], inputs["fs"], inputs["ft"], inputs["corres"]
    # fewer rows than ransac_n: the empty result, as Open3D
    assert _is_empty(R.registration_ransac_based_on_correspondence(src, tgt, corres[:2], 0.5, seed=1), 2)
    assert _is_empty(R.registration_ransac_based_on_correspondence(src, tgt, corres[:3], 0.5, ransac_n=4, seed=1), 3)
    assert _is_empty(R.registration_ransac_based_on_correspondence(src, tgt, np.zeros((0, 2), np.int32), 0.5, seed=1), 0)
    assert not _is_empty(R.registration_ransac_based_on_correspondence(src, tgt, corres[:3], 1e6, seed=1), 3)
    # no iterations allowed: nothing can be the best
    r0 = R.registration_ransac_based_on_correspondence(src, tgt, corres, 0.5, criteria=R.RANSACConvergenceCriteria(0, 0.999), seed=1)
    assert _is_empty(r0, len(corres))
    # empty clouds
    e = P.PointCloud()
    assert _is_empty(R.registration_ransac_based_on_correspondence(e, e, np.zeros((0, 2), np.int32), 0.5, seed=1), 0)
    ef = R.Feature(torch.zeros((0, 33), dtype=torch.float32, device="cuda"))
    assert _is_empty(R.registration_ransac_based_on_feature_matching(e, e, ef, ef, True, 0.5, seed=1), 0)
    assert _is_empty(R.registration_ransac_based_on_feature_matching(e, tgt, ef, ft, False, 0.5, seed=1), 0)
    assert _is_empty(R.registration_ransac_based_on_feature_matching(src, e, fs, ef, True, 0.5, seed=1), 0)
    # argument errors
    for dd in (0.0, -0.5):
        with pytest.raises(RuntimeError, match="Invalid max_correspondence_distance."):
            R.registration_ransac_based_on_correspondence(src, tgt, corres, dd)
        with pytest.raises(RuntimeError, match="Invalid max_correspondence_distance."):
            R.registration_ransac_based_on_feature_matching(src, tgt, fs, ft, True, dd)
    for n in (2, 9):
        with pytest.raises(RuntimeError, match="ransac_n"):
            R.registration_ransac_based_on_correspondence(src, tgt, corres, 0.5, ransac_n=n)
        with pytest.raises(RuntimeError, match="ransac_n"):
            R.registration_ransac_based_on_feature_matching(src, tgt, fs, ft, True, 0.5, ransac_n=n)
    with pytest.raises(RuntimeError, match="is not implemented on the MI355X path"):
        R.registration_ransac_based_on_correspondence(src, tgt, corres, 0.5, R.TransformationEstimationPointToPlane())
    with pytest.raises(RuntimeError, match="is not implemented on the MI355X path"):
        R.registration_ransac_based_on_feature_matching(src, tgt, fs, ft, True, 0.5, R.TransformationEstimationForGeneralizedICP())
    bad = corres.copy(); bad[7, 1] = len(tgt)
    with pytest.raises(RuntimeError, match="out of range"):
        R.registration_ransac_based_on_correspondence(src, tgt, bad, 0.5, seed=1)
    # the library checks the list itself too (a caller of the C ABI has no Python in front)
    ctx = P._lib.Context.current()
    cd = torch.from_numpy(bad).cuda()
    res, info, p = P._lib.PcrResult(), P._lib.PcrRansacInfo(), ransac_params(P, 3, False, None, None, None, 1, 100)
    rc = ctx.lib.pcr_registration_ransac_correspondence(
        ctx.handle, C.c_void_p(src.device_xyz().data_ptr()), C.c_void_p(0), C.c_int64(len(src)), C.c_void_p(tgt.device_xyz().data_ptr()), C.c_void_p(0),
        C.c_int64(len(tgt)), C.c_void_p(cd.data_ptr()), C.c_int64(len(bad)), C.c_double(0.5), C.byref(p), C.byref(res), C.c_void_p(0), C.byref(info))
    assert rc == P._lib.PCR_EINVAL
    # the Normal checker on clouds without normals passes (Open3D warns and goes on): same bits as without it
    s0, t0 = P.PointCloud(src.device_xyz().cpu().numpy()), P.PointCloud(tgt.device_xyz().cpu().numpy())
    assert not s0.has_normals() and not t0.has_normals()
    crit = R.RANSACConvergenceCriteria(3000, 1.0)
    plain = R.registration_ransac_based_on_correspondence(s0, t0, corres, 0.5, criteria=crit, seed=9)
    withn = R.registration_ransac_based_on_correspondence(s0, t0, corres, 0.5, checkers=[R.CorrespondenceCheckerBasedOnNormal(0.3)], criteria=crit, seed=9)
    half = R.registration_ransac_based_on_correspondence(src, t0, corres, 0.5, checkers=[R.CorrespondenceCheckerBasedOnNormal(0.3)], criteria=crit, seed=9)
    assert _bits(plain) == _bits(withn) == _bits(half) and plain.n_valid == withn.n_valid == half.n_valid == 3000
    pruned = R.registration_ransac_based_on_correspondence(src, tgt, corres, 0.5, checkers=[R.CorrespondenceCheckerBasedOnNormal(0.3)], criteria=crit, seed=9)
    assert 0 < pruned.n_valid < 3000
