"""numpy restatement of the spatial-compatibility (SC2) global registration that include/pcr_hip.h specifies, the rim detector of its exact
tests, and the planted-list generator.  Every count is an integer and every length the float64 expression of the header (differences,
squares and sums in the order x, y, z, each rounded once; IEEE sqrt), so bits, degrees, scores, seeds and member rows are compared exactly.
Poses are compared by tolerance: the fits are made by SVD here, by a quaternion eigenvector on the device."""
import numpy as np

RIM = 1e-9
CHUNK = 512


# ---------------------------------------------------------------------------------------------------------------- lists
def planted_list(n, inlier_fraction, sigma, seed):
    """(source, target, corres, T_true): sources uniform in +-40 x +-40 x +-4 m, a random rotation and a translation in +-10 m; the first
    max(3, floor(f n)) rows are the moved source points plus Gaussian noise sigma, the others random targets (other points of the box, moved);
    everything rounded to float32, then the list and the target rows are permuted."""
    rng = np.random.default_rng(seed)
    box = np.array([40.0, 40.0, 4.0])
    src = rng.uniform(-1.0, 1.0, (n, 3)) * box
    q = rng.standard_normal(4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    t = rng.uniform(-10.0, 10.0, 3)
    k = min(n, max(3, int(np.floor(inlier_fraction * n))))
    tgt = (rng.uniform(-1.0, 1.0, (n, 3)) * box) @ R.T + t
    tgt[:k] = src[:k] @ R.T + t + rng.standard_normal((k, 3)) * sigma
    src = src.astype(np.float32)
    tgt = tgt.astype(np.float32)
    place = rng.permutation(n)              # target row of list row i before the list is permuted
    tgt_out = np.empty_like(tgt)
    tgt_out[place] = tgt
    corres = np.stack([np.arange(n), place], 1)
    corres = corres[rng.permutation(n)].astype(np.int32)
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = t
    return src, tgt_out, corres, T


def pose_error(A, B):
    dR = A[:3, :3].T @ B[:3, :3]
    return float(np.arccos(np.clip((np.trace(dR) - 1.0) / 2.0, -1.0, 1.0))), float(np.linalg.norm(A[:3, 3] - B[:3, 3]))


def list_points(source, target, corres):
    corres = np.asarray(corres).reshape(-1, 2)
    return (np.asarray(source, dtype=np.float32)[corres[:, 0]].astype(np.float64).reshape(-1, 3),
            np.asarray(target, dtype=np.float32)[corres[:, 1]].astype(np.float64).reshape(-1, 3))


def lengths(p, rows=None):
    """ls[r, j] for the given rows (all by default): sqrt of dx*dx + dy*dy + dz*dz, summed in that order."""
    q = p if rows is None else p[rows]
    d = q[:, None, 0] - p[None, :, 0]
    d2 = d * d
    d = q[:, None, 1] - p[None, :, 1]
    d2 = d2 + d * d
    d = q[:, None, 2] - p[None, :, 2]
    d2 = d2 + d * d
    return np.sqrt(d2)


def compatibility(s, t, tau):
    """C (bool N x N) and the number of rim pairs: | |ls - lt| - tau | <= 1e-9 tau, i != j."""
    n = len(s)
    C = np.zeros((n, n), dtype=bool)
    rim = 0
    for r0 in range(0, n, CHUNK):
        rows = np.arange(r0, min(n, r0 + CHUNK))
        diff = np.abs(lengths(s, rows) - lengths(t, rows))
        c = diff < tau
        c[np.arange(len(rows)), rows] = False
        near = np.abs(diff - tau) <= RIM * tau
        near[np.arange(len(rows)), rows] = False
        rim += int(near.sum())
        C[rows] = c
    return C, rim


def pack_bits(C):
    """(N, ceil(N / 64)) int64: bit b of word w of row i is C[i, 64 w + b]."""
    n = C.shape[0]
    W = (n + 63) // 64
    padded = np.zeros((n, W * 64), dtype=np.uint8)
    padded[:, :n] = C
    by = np.packbits(padded.reshape(n, W, 8, 8), axis=-1, bitorder="little").reshape(n, W, 8)      # byte k of a word = bits 8k .. 8k + 7
    words = np.zeros((n, W), dtype=np.uint64)
    for k in range(8):
        words |= by[:, :, k].astype(np.uint64) << np.uint64(8 * k)
    return words.view(np.int64)


def sc2_row(C, i):
    """(rows j with C_ij ascending, SC2_ij for them)."""
    nb = np.flatnonzero(C[i])
    return nb, (C[nb] & C[i]).sum(1).astype(np.int64)


def degrees_scores(C):
    n = C.shape[0]
    deg = C.sum(1).astype(np.int32)
    score = np.zeros(n, dtype=np.int64)
    for i in range(n):
        if deg[i]:
            score[i] = sc2_row(C, i)[1].sum()
    return deg, score


# ---------------------------------------------------------------------------------------------------------------- seeds
def order_of(score):
    return np.lexsort((np.arange(len(score)), -score))


def seed_cap(n, seed_ratio, max_seeds):
    return min(max(1, int(seed_ratio * n)), max_seeds)


def pick_seeds(s, score, nms_radius, seed_ratio, max_seeds):
    """(seed rows in order, rim pairs of the suppression test)."""
    n = len(s)
    order = order_of(score)
    cand = score[order] > 0
    rim = 0
    if nms_radius > 0.0:
        ps = s[order]
        for r0 in range(0, n, CHUNK):
            rows = np.arange(r0, min(n, r0 + CHUNK))
            L = lengths(ps, rows)
            before = np.arange(n)[None, :] < rows[:, None]
            cand[rows] &= ~((L < nms_radius) & before).any(1)
            rim += int(((np.abs(L - nms_radius) <= RIM * nms_radius) & before).sum())
    return order[cand][:seed_cap(n, seed_ratio, max_seeds)], rim


def seed_members(C, m, k1, k2):
    """(K1 rows, K2 rows), the seed first."""
    nb, sc2 = sc2_row(C, m)
    take = np.lexsort((nb, -sc2))[:k1]
    K1 = np.concatenate([[m], nb[take]]).astype(np.int64)
    sub = C[np.ix_(K1, K1)]
    L = np.array([int(sub[0, a]) * int((sub[0] & sub[a]).sum()) for a in range(1, len(K1))], dtype=np.int64)
    first = np.lexsort((np.arange(len(L)), -L))[:k2]
    keep = [a for a in first if 2 * L[a] >= L.max()]
    K2 = np.concatenate([[m], K1[1:][keep]]).astype(np.int64)
    return K1, K2


def fit(s, t):
    """Umeyama without scaling (Kabsch by SVD), 4 x 4."""
    ms, mt = s.mean(0), t.mean(0)
    H = (t - mt).T @ (s - ms)
    U, _, Vt = np.linalg.svd(H)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U) * np.linalg.det(Vt))])
    R = U @ D @ Vt
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = mt - R @ ms
    return T


def residual2(T, s, t):
    """d2 per row under T, the header's expression left to right."""
    x = T[0, 0] * s[:, 0] + T[0, 1] * s[:, 1] + T[0, 2] * s[:, 2] + T[0, 3] - t[:, 0]
    y = T[1, 0] * s[:, 0] + T[1, 1] * s[:, 1] + T[1, 2] * s[:, 2] + T[1, 3] - t[:, 1]
    z = T[2, 0] * s[:, 0] + T[2, 1] * s[:, 1] + T[2, 2] * s[:, 2] + T[2, 3] - t[:, 2]
    return x * x + y * y + z * z


def score_pose(T, s, t, tau):
    """(inlier mask, count, err2, rim rows: | |T s - t| - tau | <= 1e-9 tau)."""
    d2 = residual2(T, s, t)
    inl = d2 < tau * tau
    rim = int((np.abs(np.sqrt(d2) - tau) <= RIM * tau).sum())
    return inl, int(inl.sum()), float(d2[inl].sum()), rim


def select_best(counts, err2):
    """Position of the best hypothesis (counts[k] < 0: invalid), or -1."""
    best = -1
    for k in range(len(counts)):
        if counts[k] <= 0:
            continue
        if best < 0 or counts[k] > counts[best] or (counts[k] == counts[best] and err2[k] < err2[best]):
            best = k
    return best


def refine(T, s, t, tau, iterations):
    """(T, inlier mask, count, err2, rim rows met)."""
    inl, c, e, rim = score_pose(T, s, t, tau)
    for _ in range(iterations):
        if c < 1:
            break
        T2 = fit(s[inl], t[inl])
        if not np.isfinite(T2).all():
            break
        inl2, c2, e2, r2 = score_pose(T2, s, t, tau)
        rim += r2
        if not (c2 > c or (c2 == c and e2 < e)):
            break
        T, inl, c, e = T2, inl2, c2, e2
    return T, inl, c, e, rim


def register(source, target, corres, inlier_threshold, nms_radius=None, k1=30, k2=20, seed_ratio=0.2, max_seeds=2048, refine_iterations=20,
             hypotheses=None):
    """The whole rule.  ``hypotheses`` (array S x 4 x 4, optional) replaces the fits of the valid seeds, e.g. by the device's own.  Returns a dict:
    C, deg, score, seeds, K1, K2 (lists of arrays), valid, T_seed, count, err2, best, T, inliers (mask), n_inliers, err2_final, rim (pairs + rows)."""
    tau = float(inlier_threshold)
    nms = tau if nms_radius is None else float(nms_radius)
    s, t = list_points(source, target, corres)
    n = len(s)
    out = {"n": n, "seeds": np.zeros(0, np.int64), "K1": [], "K2": [], "valid": np.zeros(0, bool), "best": -1, "T": np.eye(4), "inliers": np.zeros(n, bool),
           "n_inliers": 0, "err2_final": 0.0, "rim": 0, "T_seed": np.zeros((0, 4, 4)), "count": np.zeros(0, np.int64), "err2": np.zeros(0)}
    if n < 3:
        return out
    C, rim = compatibility(s, t, tau)
    deg, score = degrees_scores(C)
    seeds, rim_nms = pick_seeds(s, score, nms, seed_ratio, max_seeds)
    rim += rim_nms
    S = len(seeds)
    K1, K2, valid, Ts = [], [], np.zeros(S, bool), np.zeros((S, 4, 4))
    counts, err2 = np.full(S, -1, np.int64), np.zeros(S)
    for k, m in enumerate(seeds):
        a, b = seed_members(C, int(m), k1, k2)
        K1.append(a)
        K2.append(b)
        if len(b) < 3:
            continue
        T = fit(s[b], t[b]) if hypotheses is None else np.asarray(hypotheses[k], dtype=np.float64)
        if not np.isfinite(T).all():
            continue
        valid[k], Ts[k] = True, T
        _, counts[k], err2[k], r = score_pose(T, s, t, tau)
        rim += r
    best = select_best(counts, err2)
    out.update(C=C, deg=deg, score=score, seeds=seeds, K1=K1, K2=K2, valid=valid, T_seed=Ts, count=counts, err2=err2, best=best, rim=rim)
    if best >= 0:
        T, inl, c, e, r = refine(Ts[best], s, t, tau, refine_iterations)
        out.update(T=T, inliers=inl, n_inliers=c, err2_final=e, rim=rim + r)
    return out
