"""GPU checks of the three float64 pose solvers on the inputs the rest of the suite never feeds them: rank-deficient and ill-conditioned
6x6 systems (csrc/pcr_solve6.h: the fast LDL^T, its pivoted fall-back and the identity that stands in when both refuse), degenerate rows for
the Umeyama fit (csrc/pcr_umeyama.h), inverse square roots away from estimated covariances, and the L1 weight at a zero residual -- through
the one-shot fits on a list (csrc/pcr_corres.hip) and, where marked, through the tail of the ICP loop (csrc/pcr_icp_loop.h).

References: ``pose_solver_reference.exact_solve6`` (the normal equations solved in rationals), ``correspondence_reference`` (SVD Umeyama,
the oracle's GICP rows).  The singular clouds are integers and dyadic fractions with axis-aligned normals: their zero pivots are exact zeros
whatever order the device sums in, and every such test asserts that property of its own rows before it calls the device."""
import numpy as np
import pytest

from conftest import pkg, pose_error

import correspondence_reference as ref
import pose_solver_reference as psr
from test_gpu_correspondences import _close, _cloud, _kernel

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
GM_K = 0.5


@pytest.fixture(scope="module")
def P():
    return pkg()


def _f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def _rot(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


def _pose(R, t=(0, 0, 0)):
    T = np.eye(4); T[:3, :3] = R; T[:3, 3] = t
    return T


def _lattice(seed, side=7, jitter=0.2):
    """side^3 points of the unit lattice centred on the origin, each moved by at most `jitter` per axis: no two closer than 1 - 2 jitter, so a
    target moved by less than a quarter of that is found row by row by a nearest-neighbour search"""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(*[np.arange(side) - (side - 1) / 2.0] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    return _f32(g + rng.uniform(-jitter, jitter, g.shape))


SMALL_MOTION = _pose(_rot([1.0, -2.0, 0.5], 0.01), [0.03, -0.02, 0.01])          # moves a point of the lattices here by less than 0.1


def _sorted_rows(rows):
    rows = np.asarray(rows)
    return rows[np.argsort(rows[:, 0], kind="stable")]


def _assert_planted(result, n):
    """the loop's (or the evaluation's) search returned row i for source point i, for every point"""
    assert np.array_equal(_sorted_rows(result.correspondence_set), psr.identity_rows(n))


_WELL_POSED = {}


def _context_still_fits(P, oracle):
    """One well-posed point-to-plane fit (GM weights) on the context a degenerate call has just used: a flag, an LDS row or a state left behind
    by the rare path would show here.  The reference is computed once."""
    if not _WELL_POSED:
        sx = _lattice(5)
        tx = _f32(sx @ SMALL_MOTION[:3, :3].T + SMALL_MOTION[:3, 3] + np.random.default_rng(6).uniform(-1e-3, 1e-3, sx.shape))
        nrm = np.random.default_rng(7).standard_normal(sx.shape)
        nrm = _f32(nrm / np.linalg.norm(nrm, axis=1, keepdims=True))
        rows = psr.identity_rows(len(sx))
        _WELL_POSED.update(sx=sx, tx=tx, nrm=nrm, rows=rows, T_ref=ref.point_to_plane(oracle, sx, tx, nrm, rows, "gm", GM_K))
        assert not np.array_equal(_WELL_POSED["T_ref"], np.eye(4))
    w = _WELL_POSED
    T = P.registration.TransformationEstimationPointToPlane(P.registration.GMLoss(GM_K)).compute_transformation(_cloud(P, w["sx"]), _cloud(P, w["tx"], w["nrm"]), w["rows"])
    _close(T, w["T_ref"], "well-posed fit after the degenerate call")


# ================================================================================================ 1. exact rank deficiency, point-to-plane
QUARTER_TURN = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
SINGULAR = {                # cloud, rank, columns of J that are exactly zero, an exact non-trivial initial pose (entries 0, +-1 and dyadic fractions)
    "floor": (psr.floor, 3, (2, 3, 4), _pose(QUARTER_TURN, [3.0, -2.0, 0.5])),
    "corridor": (psr.corridor, 5, (4,), _pose(QUARTER_TURN, [3.0, -2.0, 0.5])),
    "sphere": (psr.sphere, 3, (0, 1, 2), _pose(QUARTER_TURN)),
    # 36 x 36 = 1296 points: the loop's tail then gathers THREE workgroups' partial rows (512 points each), so the LDS rows the pivoted
    # fall-back borrows for its right-hand side and its result hold live sums when it starts -- up to 1024 points they hold zeros, and a
    # result read before lane 0 wrote it would read "no solution" and pass for the right answer
    "wide floor": (lambda: psr.floor(side=36), 3, (2, 3, 4), _pose(QUARTER_TURN, [3.0, -2.0, 0.5])),
}
_SINGULAR_INPUTS = {}


def _singular(shape, loss):
    """the clouds of a singular case with the properties the case rests on asserted in float64 and in rationals (once per case)"""
    if (shape, loss) not in _SINGULAR_INPUTS:
        make, rank, zero_cols, T0 = SINGULAR[shape]
        sx, tx, nrm = make()
        assert np.array_equal(sx, _f32(sx)) and np.array_equal(tx, _f32(tx)) and np.array_equal(nrm, _f32(nrm))    # float32 holds every value exactly
        rows = psr.identity_rows(len(sx))
        J, r = psr.plane_rows(sx, tx, nrm, rows)
        psr.assert_exact_columns(J, zero=zero_cols)
        assert (r != 0.0).all()                                             # (L1: no residual is exactly zero)
        x, exact_rank, T_exact = psr.exact_solve6(J, ref.kernel_weights(loss, GM_K, r), r)
        assert x is None and exact_rank == rank and np.array_equal(T_exact, np.eye(4))
        _SINGULAR_INPUTS[(shape, loss)] = (sx, tx, nrm, rows, T0)
    return _SINGULAR_INPUTS[(shape, loss)]


@pytest.mark.parametrize("loss", ["l2", "l1", "gm"])
@pytest.mark.parametrize("shape", list(SINGULAR))
def test_rank_deficient_point_to_plane_fit(P, oracle, shape, loss):
    """Branch (k_corr_fit): the fast LDL^T meets an exact zero pivot and refuses, the pivoted form meets the same zero and refuses, the identity
    stands in (out[17] == 0): the 4x4 identity bit for bit, twice, and the RMSE of the rows."""
    R = P.registration
    sx, tx, nrm, rows, _ = _singular(shape, loss)
    src, tgt = _cloud(P, sx), _cloud(P, tx, nrm)
    est = R.TransformationEstimationPointToPlane(_kernel(R, loss, GM_K))
    T = est.compute_transformation(src, tgt, rows)
    assert T.tobytes() == np.eye(4).tobytes(), T
    assert est.compute_transformation(src, tgt, rows).tobytes() == T.tobytes()
    e, e_ref = est.compute_rmse(src, tgt, rows), ref.rmse_plane(sx, tx, nrm, rows)
    assert e_ref > 0 and abs(e / e_ref - 1.0) < 1e-12
    _context_still_fits(P, oracle)


@pytest.mark.parametrize("start", ["identity", "posed"])
@pytest.mark.parametrize("loss", ["l2", "l1", "gm"])
@pytest.mark.parametrize("shape", list(SINGULAR))
def test_rank_deficient_point_to_plane_loop(P, oracle, shape, loss, start):
    """Branch (icp_finish): both LDL^T forms refuse, lane 0 hands "no solution" to the wavefront through LDS, U stays the identity.  The pose
    then stays the initial pose bit for bit, the second launch sees the same fitness and RMSE and the loop stops as converged after one
    "update": what the oracle's loop does when its solve fails (oracle/gicp.c applies the identity), which the test makes it do on the same
    clouds by handing it all-zero covariances.  From the identity and from an exact non-trivial pose, so that "unchanged" is not "identity"."""
    R = P.registration
    sx, tx, nrm, rows, T0 = _singular(shape, loss)
    n = len(sx)
    init = np.eye(4) if start == "identity" else T0
    Ti = np.linalg.inv(init)
    assert np.array_equal(Ti @ init, np.eye(4))
    s0 = sx @ Ti[:3, :3].T + Ti[:3, 3]
    assert np.array_equal(s0 @ init[:3, :3].T + init[:3, 3], sx)           # the initial pose puts the source exactly onto the planted rows
    src0, tgt = _cloud(P, s0), _cloud(P, tx, nrm)
    est = R.TransformationEstimationPointToPlane(_kernel(R, loss, GM_K))
    at_init = R.evaluate_registration(src0, tgt, 0.5, init)
    _assert_planted(at_init, n)
    loop = R.registration_icp(src0, tgt, 0.5, init, est, R.ICPConvergenceCriteria(1e-6, 1e-6, 30))
    _assert_planted(loop, n)
    assert loop.transformation.tobytes() == np.ascontiguousarray(init, np.float64).tobytes(), loop.transformation
    assert loop.fitness == at_init.fitness == 1.0 and loop.inlier_rmse == at_init.inlier_rmse and loop.inlier_rmse > 0
    z = np.zeros((n, 3, 3))
    orc = oracle.registration_gicp(s0, tx, 0.5, init, src_cov=z, tgt_cov=z, loss=oracle.LOSS_L2, rel_fitness=1e-6, rel_rmse=1e-6, max_it=30)
    assert np.array_equal(orc.transformation, init) and orc.fitness == 1.0                # its solve failed too: the identity was applied
    print(f"{shape} {loss} from {start}: loop {loop.iterations} iterations, converged {loop.converged}; oracle {orc.iterations}, {orc.converged}")
    assert (loop.iterations, loop.converged) == (orc.iterations, bool(orc.converged)) == (1, True)
    assert abs(loop.inlier_rmse / orc.inlier_rmse - 1.0) < 1e-12
    _context_still_fits(P, oracle)


# ================================================================================================ 2. conditioning ladder
def _relief_floor(d):
    """the floor with relief d U(-1, 1) in z and normals tilted by d N(0, 1), 400 rows; the target is the source under SMALL_MOTION about the
    floor's centre (every point moves by less than 0.2, a fifth of the spacing)"""
    rng = np.random.default_rng(21)
    sx, _, _ = psr.floor()
    sx = sx - [9.5, 9.5, 0.0]
    sx[:, 2] = d * rng.uniform(-1, 1, 400)
    def normals():
        n = np.array([0.0, 0.0, 1.0]) + d * rng.standard_normal((400, 3))
        return _f32(n / np.linalg.norm(n, axis=1, keepdims=True))
    sn, tn = normals(), normals()
    sx = _f32(sx)
    return sx, _f32(sx @ SMALL_MOTION[:3, :3].T + SMALL_MOTION[:3, 3]), sn, tn


def _ladder_close(T, T_ref, bound, what):
    ang, dt = pose_error(T, T_ref)
    print(f"{what}: error {ang:.2e} rad {dt:.2e} m, rounding bound {bound:.2e}")
    assert ang < max(1e-7, bound) and dt < max(1e-6, bound), (what, ang, dt, bound)
    assert np.array_equal(T[3], [0, 0, 0, 1])


@pytest.mark.parametrize("d", [1.0, 1e-1, 1e-2, 1e-3])
def test_conditioning_ladder(P, oracle, d):
    """Branch: the fast LDL^T (every pivot positive), at condition numbers from about 1e1 to 1e7.  Reference: the exact solution of the same
    normal equations.  bound = 8 n 2^-53 cond |x_exact| is what float64 sums of n rows in any order can move the solution by; for d >= 1e-2
    it stays below a tenth of the project's tolerance (asserted) and the tolerance is the project's; for d = 1e-3 the tolerance is the larger of
    the two."""
    R = P.registration
    sx, tx, sn, tn = _relief_floor(d)
    rows = psr.identity_rows(400)
    src, tgt = _cloud(P, sx, sn), _cloud(P, tx, tn)
    J, r = psr.plane_rows(sx, tx, tn, rows)
    for loss in ("l2", "gm"):
        w = ref.kernel_weights(loss, GM_K, r)
        x, rank, T_ref = psr.exact_solve6(J, w, r)
        assert rank == 6
        cond = np.linalg.cond((J * w[:, None]).T @ J)
        bound = 8.0 * 400 * EPS * cond * np.linalg.norm(x)
        print(f"d = {d:g} point-to-plane {loss}: cond {cond:.2e}, |x| {np.linalg.norm(x):.2e}, bound {bound:.2e}")
        if d >= 1e-2:
            assert bound < 1e-8
        est = R.TransformationEstimationPointToPlane(_kernel(R, loss, GM_K))
        T = est.compute_transformation(src, tgt, rows)
        _ladder_close(T, T_ref, bound, f"d = {d:g} point-to-plane {loss}")
        if d == 1e-2:               # the loop's first update is the same fit (fast path of icp_finish)
            loop = R.registration_icp(src, tgt, 0.45, np.eye(4), est, R.ICPConvergenceCriteria(1e-6, 1e-6, 1))
            _assert_planted(loop, 400)
            assert loop.iterations == 1
            _close(loop.transformation, T, f"d = {d:g} loop against the estimator, point-to-plane {loss}")
    # GICP from normals: the system of the oracle's rows, solved exactly
    cs, ct = oracle.covariances_from_normals(ref.unit_normals(sn), 1e-3), oracle.covariances_from_normals(ref.unit_normals(tn), 1e-3)
    JTJ, JTr, _ = oracle.gicp_linearize(sx, cs, tx, ct, rows, oracle.LOSS_L2, 1.0)
    x, rank, T_ref = psr.exact_update(JTJ, JTr)
    assert rank == 6
    cond = np.linalg.cond(JTJ)
    bound = 8.0 * 1200 * EPS * cond * np.linalg.norm(x)
    print(f"d = {d:g} GICP from normals: cond {cond:.2e}, |x| {np.linalg.norm(x):.2e}, bound {bound:.2e}")
    if d >= 1e-2:
        assert bound < 1e-8
    est = R.TransformationEstimationForGeneralizedICP(R.L2Loss())
    T = est.compute_transformation(src, tgt, rows)
    _ladder_close(T, T_ref, bound, f"d = {d:g} GICP from normals")
    if d == 1e-2:
        loop = R.registration_generalized_icp(src, tgt, 0.45, np.eye(4), est, R.ICPConvergenceCriteria(1e-6, 1e-6, 1))
        _assert_planted(loop, 400)
        assert loop.iterations == 1
        _close(loop.transformation, T, f"d = {d:g} loop against the estimator, GICP")


# ================================================================================================ 3. fewer rows than unknowns, near-dependence
def _tilted_corridor():
    """the corridor with its wall turned about z by 1 rad: the wall's rows have J[3] = cos 1 and J[4] = sin 1 (the same two float32 values in
    every row), the floor's have neither, so the columns of t_x and t_y are dependent in exact arithmetic and a last pivot of the LDL^T is
    whatever rounding leaves of zero"""
    sx, _, nrm = psr.corridor()
    Rz = _rot([0, 0, 1], 1.0)
    sx[400:] = sx[400:] @ Rz.T
    nrm[400:] = nrm[400:] @ Rz.T
    sx, nrm = _f32(sx), _f32(nrm)
    return sx, _f32(sx + 0.25 * nrm), nrm


@pytest.mark.parametrize("case", ["1 row", "3 rows", "5 rows", "tilted corridor"])
def test_underdetermined_and_nearly_dependent_systems(P, oracle, case):
    """Branch: fast refusing or not, pivoted refusing or not -- rounding decides.  With fewer rows than unknowns, or columns that depend on each
    other only in exact arithmetic, a trailing pivot is +1e-17 or -1e-17 or 0 by the order of the sums, so no single pose is right: for a
    positive semi-definite system the success return of icp_ldlt6_pivoted is reached through rounding only.  What CAN be pinned, and is: the
    pose is finite with bottom row (0, 0, 0, 1), a second call gives the same bits, and the context fits a well-posed list afterwards."""
    R = P.registration
    if case == "tilted corridor":
        sx, tx, nrm = _tilted_corridor()
        rows = psr.identity_rows(len(sx))
    else:
        sx = _lattice(31); tx = _f32(sx @ SMALL_MOTION[:3, :3].T + SMALL_MOTION[:3, 3])
        nrm = np.random.default_rng(32).standard_normal(sx.shape)
        nrm = _f32(nrm / np.linalg.norm(nrm, axis=1, keepdims=True))
        rows = psr.identity_rows(len(sx))[[11, 200, 77, 305, 150][: int(case.split()[0])]]
    J, r = psr.plane_rows(sx, tx, nrm, rows)
    assert np.linalg.matrix_rank(J) < 6
    src, tgt = _cloud(P, sx), _cloud(P, tx, nrm)
    for loss in ("l2", "l1", "gm"):
        est = R.TransformationEstimationPointToPlane(_kernel(R, loss, GM_K))
        T = est.compute_transformation(src, tgt, rows)
        print(f"{case} {loss}: identity {np.array_equal(T, np.eye(4))}, |T - I| {np.abs(T - np.eye(4)).max():.3e}")
        assert np.isfinite(T).all() and np.array_equal(T[3], [0, 0, 0, 1])
        assert est.compute_transformation(src, tgt, rows).tobytes() == T.tobytes()
        _context_still_fits(P, oracle)


# ================================================================================================ 4. the L1 weight at a zero residual
@pytest.mark.parametrize("k", [1, 40])
def test_l1_weight_at_zero_residuals(P, oracle, k):
    """k of 343 rows have t = s, so (s - t).n == 0 exactly.  The oracle (Open3D) weights such a row 1 / 0 = inf, its sums turn NaN and its solve
    fails: the identity.  The device weights it 1 / 1e-300 (icp_weight, include/pcr_hip.h): the row enters JTJ with 1e300 J^T J, beside which
    the other rows vanish, and adds nothing to JTr (its r is 0).  JTJ is then k rows' worth of rank at 1e300 plus rounding at 1e284, and what
    the LDL^T makes of it is finite and tiny: on an MI355X |T - I| was 2.0e-281 for k = 1 and 8.7e-300 for k = 40, 1.0e-2 rad and 3.7e-2 m from
    the fit over the remaining rows.  That is neither the identity bit for bit nor that fit, so the number is not pinned (include/pcr_hip.h says
    the same); the test prints it and asserts what holds whatever rounding does: a finite pose, the same bits on a second call, the ordinary fit
    once the zero rows are left out, a usable context."""
    R = P.registration
    sx = _lattice(41); tx = _f32(sx @ SMALL_MOTION[:3, :3].T + SMALL_MOTION[:3, 3])
    nrm = np.random.default_rng(42).standard_normal(sx.shape)
    nrm = _f32(nrm / np.linalg.norm(nrm, axis=1, keepdims=True))
    hit = np.random.default_rng(43).permutation(len(sx))[:k]
    tx[hit] = sx[hit]
    rows = psr.identity_rows(len(sx))
    J, r = psr.plane_rows(sx, tx, nrm, rows)
    assert (r[hit] == 0.0).all() and (np.delete(r, hit) != 0.0).all()
    with np.errstate(divide="ignore", invalid="ignore"):
        T_oracle = ref.point_to_plane(oracle, sx, tx, nrm, rows, "l1")
    assert np.array_equal(T_oracle, np.eye(4))                               # 1 / 0, NaN sums, a failed solve: the identity
    rest = np.delete(rows, hit, axis=0)
    T_rest = ref.point_to_plane(oracle, sx, tx, nrm, rest, "l1")
    est = R.TransformationEstimationPointToPlane(R.L1Loss())
    src, tgt = _cloud(P, sx), _cloud(P, tx, nrm)
    T = est.compute_transformation(src, tgt, rows)
    ang, dt = pose_error(T, T_rest)
    print(f"L1, {k} zero residuals: device identity {np.array_equal(T, np.eye(4))}, |T - I| {np.abs(T - np.eye(4)).max():.3e}; from the fit over the other rows {ang:.2e} rad {dt:.2e} m")
    assert np.isfinite(T).all() and np.array_equal(T[3], [0, 0, 0, 1])
    assert est.compute_transformation(src, tgt, rows).tobytes() == T.tobytes()
    # without the zero rows the same call is the ordinary fit
    _close(est.compute_transformation(src, tgt, rest), T_rest, f"L1 without the {k} zero rows")
    _context_still_fits(P, oracle)


# ================================================================================================ 5. Umeyama on degenerate rows
def _residual(T, s, t):
    return float(np.sqrt((((s @ T[:3, :3].T + T[:3, 3]) - t) ** 2).sum() / len(s)))


def _fit(P, sx, tx, scaling, rows=None):
    rows = psr.identity_rows(len(sx)) if rows is None else rows
    est = P.registration.TransformationEstimationPointToPoint(scaling)
    src, tgt = _cloud(P, sx), _cloud(P, tx)
    T = est.compute_transformation(src, tgt, rows)
    assert est.compute_transformation(src, tgt, rows).tobytes() == T.tobytes()
    return T, ref.point_to_point(sx, tx, rows, scaling)


def _one_p2p_update(P, sx, tx, scaling, max_dist):
    """one point-to-point update of the loop from the identity, its search checked against the planted rows"""
    R = P.registration
    loop = R.registration_icp(_cloud(P, sx), _cloud(P, tx), max_dist, np.eye(4), R.TransformationEstimationPointToPoint(scaling), R.ICPConvergenceCriteria(1e-6, 1e-6, 1))
    _assert_planted(loop, len(sx))
    assert loop.iterations == 1
    return loop.transformation


@pytest.mark.parametrize("scaling", [False, True])
def test_umeyama_coplanar_rows(P, scaling):
    """(a) sigma of rank 2: 400 jittered grid points in the plane z = 0 under a rotation about (1, -2, 0.5) -- list and loop"""
    rng = np.random.default_rng(51)
    sx, _, _ = psr.floor()
    sx = _f32(sx - [9.5, 9.5, 0.0] + np.concatenate([rng.uniform(-0.2, 0.2, (400, 2)), np.zeros((400, 1))], axis=1))
    assert (sx[:, 2] == 0).all()
    tx = _f32(sx @ SMALL_MOTION[:3, :3].T + SMALL_MOTION[:3, 3])
    T, T_ref = _fit(P, sx, tx, scaling)
    _close(T, T_ref, f"coplanar rows, scaling={scaling}", scaled=scaling)
    _close(_one_p2p_update(P, sx, tx, scaling, 0.3), T_ref, f"coplanar rows through the loop, scaling={scaling}", scaled=scaling)


def _thin_column(axis):
    """300 points within 0.06 of the line through the origin along `axis`, one per unit of length: a half turn about the line moves each by less
    than 0.12, so a nearest-neighbour search still returns the planted rows"""
    rng = np.random.default_rng(52)
    p = np.concatenate([rng.uniform(-0.04, 0.04, (300, 2)), (np.arange(300.0) - 149.5)[:, None]], axis=1)
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    if abs(a[2]) < 1.0:
        p = p @ _rot(np.cross([0, 0, 1.0], a), np.arccos(a[2])).T
    return _f32(p)


@pytest.mark.parametrize("scaling", [False, True])
@pytest.mark.parametrize("axis", [(0.0, 0.0, 1.0), (1.0, 2.0, 3.0)])
@pytest.mark.parametrize("short", [0.0, 1e-5])
def test_umeyama_half_turns(P, axis, short, scaling):
    """(b) rotations by exactly pi (Horn's quaternion has w = 0) and by pi - 1e-5, about z and about (1, 2, 3): a generic cloud on a list, and
    a thin column about the axis through the loop"""
    Rm = _rot(axis, np.pi - short)
    sx = _lattice(53)
    tx = _f32(sx @ Rm.T + [0.3, -0.2, 0.1])
    T, T_ref = _fit(P, sx, tx, scaling)
    _close(T, T_ref, f"half turn - {short:g} about {axis}, scaling={scaling}", scaled=scaling)
    Rd = T[:3, :3] / np.cbrt(np.linalg.det(T[:3, :3]))
    assert abs(np.arccos(np.clip((np.trace(Rd) - 1.0) / 2.0, -1.0, 1.0)) - (np.pi - short)) < 1e-3          # (it IS the half turn; arccos near -1 resolves 1e-8 of it)
    col = _thin_column(axis)
    tcol = _f32(col @ Rm.T)
    assert np.linalg.norm(tcol - col, axis=1).max() < 0.125
    T_ref = ref.point_to_point(col, tcol, psr.identity_rows(300), scaling)
    _close(_one_p2p_update(P, col, tcol, scaling, 0.3), T_ref, f"half turn - {short:g} about {axis} through the loop, scaling={scaling}", scaled=scaling)


@pytest.mark.parametrize("scaling", [False, True])
def test_umeyama_mirrored_target(P, scaling):
    """(c) the target is the source mirrored in z: the best ROTATION is wanted (the reflection fix), with the SVD form's residual"""
    sx = _lattice(54)[:300]
    tx = sx * [1.0, 1.0, -1.0]
    T, T_ref = _fit(P, sx, tx, scaling)
    c = np.cbrt(np.linalg.det(T[:3, :3]))
    assert c > 0 and abs(np.linalg.det(T[:3, :3] / c) - 1.0) < 1e-9
    _close(T, T_ref, f"mirrored target, scaling={scaling}", scaled=scaling)
    e, e_ref = _residual(T, sx, tx), _residual(T_ref, sx, tx)
    print(f"mirrored target, scaling={scaling}: residual {e!r}, reference {e_ref!r}")
    assert e_ref > 0.1 and abs(e / e_ref - 1.0) < 1e-9


@pytest.mark.parametrize("scaling", [False, True])
@pytest.mark.parametrize("case", ["collinear", "two rows"])
def test_umeyama_rows_that_leave_a_rotation_free(P, case, scaling):
    """(d) collinear source rows and two rows: the rotation about the line is free, so the poses are compared by certificate -- the device's
    pose fits the rows as well as the SVD form's (residual RMSE equal to 1e-9 relative; the 1e-12 m beside it is for the two scaled rows, which
    both forms fit exactly: coordinates below 8 carry float64 rounding of 1e-15 m), it is finite and its rotation has determinant 1."""
    rng = np.random.default_rng(55)
    if case == "collinear":
        sx = _f32(np.outer(np.arange(40.0) / 8.0 - 2.0, [1.0, -2.0, 0.5]) + [0.5, 0.25, -1.0])
        assert np.linalg.matrix_rank(sx - sx[0]) == 1                       # exactly collinear in float32: multiples of 1/8 along (1, -2, 0.5)
    else:
        sx = _lattice(56)[[3, 300]]
    tx = _f32(sx @ SMALL_MOTION[:3, :3].T + SMALL_MOTION[:3, 3] + rng.uniform(-0.01, 0.01, sx.shape))
    T, T_ref = _fit(P, sx, tx, scaling)
    assert np.isfinite(T).all() and np.array_equal(T[3], [0, 0, 0, 1])
    c = np.cbrt(np.linalg.det(T[:3, :3]))
    assert c > 0 and abs(np.linalg.det(T[:3, :3] / c) - 1.0) < 1e-9
    e, e_ref = _residual(T, sx, tx), _residual(T_ref, sx, tx)
    print(f"{case}, scaling={scaling}: residual {e!r}, reference {e_ref!r}")
    assert abs(e - e_ref) <= 1e-9 * e_ref + 1e-12


@pytest.mark.parametrize("copies", [1, 5])
def test_umeyama_one_row(P, copies):
    """(e) one row, and five copies of it (coordinates with a few bits, so that every product is exact and the source's variance is an exact
    zero).  Without scaling: the rotation is the identity and the translation takes s to t.  With scaling: include/pcr_hip.h documents that the
    fit "divides by a zero variance" -- 0 / 0, the pose is not finite.  Either way the next call on the context is correct."""
    sx = np.array([[1.5, -2.25, 0.75], [4.0, 4.0, 4.0]]); tx = np.array([[-0.5, 3.0, 2.125], [0.0, 1.0, 2.0]])
    rows = np.zeros((copies, 2), np.int32)
    T, _ = _fit(P, sx, tx, False, rows)
    assert np.array_equal(T[:3, :3], np.eye(3)) and np.array_equal(T[:3, 3], tx[0] - sx[0]) and np.array_equal(T[3], [0, 0, 0, 1])
    est = P.registration.TransformationEstimationPointToPoint(True)
    Ts = est.compute_transformation(_cloud(P, sx), _cloud(P, tx), rows)
    print(f"{copies} copies of one row with scaling:\n{Ts}")
    assert not np.isfinite(Ts[:3]).all()
    lat = _lattice(57); tlat = _f32(lat @ SMALL_MOTION[:3, :3].T + SMALL_MOTION[:3, 3])
    for scaling in (False, True):
        T, T_ref = _fit(P, lat, tlat, scaling)
        _close(T, T_ref, f"the call after {copies} copies of one row, scaling={scaling}", scaled=scaling)


@pytest.mark.parametrize("scaling", [False, True])
def test_umeyama_cube_corners(P, scaling):
    """(f) the eight corners of a cube under the identity (Horn's matrix is diagonal with a triple eigenvalue below the largest: no sweep runs)
    and under a quarter turn about z"""
    sx = np.array([[x, y, z] for x in (-1.0, 1.0) for y in (-1.0, 1.0) for z in (-1.0, 1.0)])
    for name, Rm in (("identity", np.eye(3)), ("quarter turn", QUARTER_TURN)):
        T, T_ref = _fit(P, sx, sx @ Rm.T, scaling)
        _close(T, T_ref, f"cube corners, {name}, scaling={scaling}", scaled=scaling)
        _close(T, _pose(Rm), f"cube corners, {name}, against the planted motion")


@pytest.mark.parametrize("scaling", [False, True])
def test_umeyama_far_from_the_origin(P, scaling):
    """(g) both clouds, and the target alone, shifted by 1e2 ... 1e5 m: the target's moments are taken about the target point of row 0 and the
    source's about the source point of row 0, so the centred sums cancel neither against the offset nor against the distance between the
    clouds.  (With ONE origin for both, the scaled fit of the target shifted alone by 1e5 m was 1.25e-7 rad off: the source's variance, 5,
    came out of sums of 1e10.)  The reference works on the float32-rounded coordinates.  (h) row 0 names a target point 1e4 m from everything
    else: that point is the origin the device uses for the target."""
    base = _lattice(58)[:300]
    moved = base @ SMALL_MOTION[:3, :3].T + SMALL_MOTION[:3, 3] + np.random.default_rng(59).uniform(-1e-3, 1e-3, base.shape)
    for off in (1e2, 1e3, 1e4, 1e5):
        shift = off * np.array([1.0, -0.5, 0.25])
        for what, sx in (("both", _f32(base + shift)), ("target only", _f32(base))):
            tx = _f32(moved + shift)
            T, T_ref = _fit(P, sx, tx, scaling)
            _close(T, T_ref, f"{what} shifted by {off:g} m, scaling={scaling}", scaled=scaling)
    sx, tx = _f32(base), _f32(moved)
    tx[0] = [1e4, -5e3, 2.5e3]
    T, T_ref = _fit(P, sx, tx, scaling)
    _close(T, T_ref, f"row 0 names an outlier at 1e4 m, scaling={scaling}", scaled=scaling)


# ================================================================================================ 6. the inverse square root
def _frames(rng, n):
    Q = np.linalg.qr(rng.standard_normal((n, 3, 3)))[0]
    Q[:, :, 0] *= np.sign(np.linalg.det(Q))[:, None]
    return Q


def _prescribed_covariances(case, n=300, seed=61):
    """n pairs of float32 cov6 rows (Cs, Ct) whose sum M has the eigenvalues of `case` in a random orthonormal frame of its own (the frames are
    drawn until n of them leave cond(M) <= 1e6 AFTER the rounding to float32, which moves an eigenvalue of 1e-6 by a few per cent)"""
    rng = np.random.default_rng(seed)
    lam = {"equal": (1, 1, 1), "two equal": (2, 2, 2e-3), "nearly equal": (2, 2 - 1e-6, 2e-3), "spread": (1, 1e-3, 1e-6)}.get(case)
    out = []
    while len(out) < n:
        if lam is not None:
            Q = _frames(rng, n)
            half = np.einsum("nik,k,njk->nij", Q, 0.5 * np.array(lam, np.float64), Q)
        else:
            d = np.stack([rng.uniform(0.5, 2.0, n), rng.uniform(1e-3, 1e-2, n), rng.uniform(1e-5, 1e-4, n)], axis=1)[:, rng.permutation(3)]
            half = np.einsum("ni,ij->nij", 0.5 * d, np.eye(3))
            if case == "nearly diagonal":
                half = half + 0.5e-7 * (1.0 - np.eye(3))
        half = _f32(0.5 * (half + half.transpose(0, 2, 1)))
        keep = np.linalg.cond(2.0 * half) <= 1e6
        out.extend(half[keep])
    return np.array(out[:n])


@pytest.mark.parametrize("case", ["equal", "two equal", "nearly equal", "spread", "diagonal", "nearly diagonal"])
def test_inverse_square_root_through_covariance_gicp(P, oracle, case):
    """Branch: icp_sym3_inv_sqrt (six fixed Jacobi sweeps) inside k_corr_rows<GICP_COV>, then the fast LDL^T.  Reference: the oracle's GICP rows
    on the float32-rounded covariances.  The project's tolerance while cond(M) <= 1e6, which the test asserts of its own inputs."""
    R = P.registration
    sx = _lattice(62)[:300]; tx = _f32(sx @ SMALL_MOTION[:3, :3].T + SMALL_MOTION[:3, 3])
    half = _prescribed_covariances(case)
    cond = np.linalg.cond(half + half)
    assert cond.max() <= 1e6
    if case in ("diagonal", "nearly diagonal"):
        off = half[:, [0, 0, 1], [1, 2, 2]]
        assert (off == 0).all() if case == "diagonal" else (abs(2 * off - 1e-7) < 1e-13).all()
    rows = psr.identity_rows(300)
    src, tgt = _cloud(P, sx), _cloud(P, tx)
    src.covariances = half; tgt.covariances = half
    assert np.array_equal(src.covariances, half)                             # float32 holds them exactly
    est = R.TransformationEstimationForGeneralizedICP(R.L2Loss())
    T = est.compute_transformation(src, tgt, rows)
    T_ref = ref.generalized_icp(oracle, sx, tx, rows, "l2", src_cov=half, tgt_cov=half)
    assert not np.array_equal(T_ref, np.eye(4))
    print(f"{case}: cond(M) {cond.min():.2e} ... {cond.max():.2e}")
    _close(T, T_ref, f"covariance GICP, M {case}")
    if case == "two equal":          # the loop's rows (M = R Cs R^T + Ct at R = identity) give the same first update
        loop = R.registration_generalized_icp(src, tgt, 0.3, np.eye(4), est, R.ICPConvergenceCriteria(1e-6, 1e-6, 1))
        _assert_planted(loop, 300)
        assert loop.iterations == 1
        _close(loop.transformation, T, "covariance GICP loop against the estimator")


def test_singular_covariance_sum(P, oracle):
    """Cs = Ct = diag(1, 1, 0) exactly: M has a zero eigenvalue, its inverse square root none.  Nothing is pinned but that the call returns and
    the context is usable (branch: non-finite sums, both LDL^T forms refuse, the identity stands in -- printed, not asserted)."""
    R = P.registration
    sx = _lattice(63)[:300]; tx = _f32(sx @ SMALL_MOTION[:3, :3].T + SMALL_MOTION[:3, 3])
    src, tgt = _cloud(P, sx), _cloud(P, tx)
    cov = np.tile(np.diag([1.0, 1.0, 0.0]), (300, 1, 1))
    src.covariances = cov; tgt.covariances = cov
    T = R.TransformationEstimationForGeneralizedICP(R.L2Loss()).compute_transformation(src, tgt, psr.identity_rows(300))
    print(f"singular covariance sum: the device gave\n{T}")
    assert T.shape == (4, 4)
    _context_still_fits(P, oracle)


# ================================================================================================ 7. RANSAC draws the Umeyama fit too
def test_ransac_on_collinear_rows(P):
    """200 rows whose source points are collinear, ransac_n = 3, no checkers: every hypothesis fits rows that leave a rotation free (and samples
    with repeated rows leave more).  The best pose is finite and its inlier count is the count recomputed on the host in float64 under that
    pose (no row lies within 1e-9 m of the threshold, so float64 rounding cannot move a row across it)."""
    R = P.registration
    rng = np.random.default_rng(71)
    sx = _f32(np.outer(np.arange(200.0) / 16.0 - 6.0, [1.0, -2.0, 0.5]) + [0.5, 0.25, -1.0])
    assert np.linalg.matrix_rank(sx - sx[0]) == 1
    tx = _f32(sx @ SMALL_MOTION[:3, :3].T + SMALL_MOTION[:3, 3] + rng.uniform(-0.02, 0.02, sx.shape))
    rows = psr.identity_rows(200)
    res = R.registration_ransac_based_on_correspondence(_cloud(P, sx), _cloud(P, tx), rows, 0.02, R.TransformationEstimationPointToPoint(False), 3, [],
                                                        R.RANSACConvergenceCriteria(2000, 0.999), seed=5)
    T = res.transformation
    assert np.isfinite(T).all() and np.array_equal(T[3], [0, 0, 0, 1]) and res.converged
    dis = np.linalg.norm(sx @ T[:3, :3].T + T[:3, 3] - tx, axis=1)
    assert (abs(dis - 0.02) > 1e-9).all()
    inl = dis < 0.02
    print(f"RANSAC on collinear rows: {int(inl.sum())} inliers of 200 after {res.iterations} iterations, fitness {res.fitness}")
    assert 0 < inl.sum() and res.fitness == inl.sum() / 200.0
    assert np.array_equal(res.correspondence_set, rows[inl])
    assert abs(res.inlier_rmse / np.sqrt((dis[inl] ** 2).sum() / inl.sum()) - 1.0) < 1e-9
