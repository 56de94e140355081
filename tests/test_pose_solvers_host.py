"""The four float64 pose solvers (csrc/pcr_solve6.h: icp_ldlt6_fast, icp_ldlt6_pivoted, icp_sym3_inv_sqrt, icp_weight; csrc/pcr_umeyama.h:
icp_umeyama) compiled for the HOST and driven through a stand-alone program (tests/host/pose_solvers_main.cpp): what no cloud can feed them on
the device -- indefinite 6x6 systems -- and 10^4 random positive definite systems across condition numbers 1 ... 1e8.  The program is built
twice, plain and with -fsanitize=address,undefined, and both builds must print the same bits.  No GPU is needed."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import pose_solver_reference as psr

HERE = os.path.dirname(os.path.abspath(__file__))
EPS = 2.0 ** -53


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    out = tmp_path_factory.mktemp("pose_solvers_host")
    base = [cxx, "-std=c++17", "-O2", "-Wno-unknown-pragmas", "-I", os.path.join(HERE, "host"), os.path.join(HERE, "host", "pose_solvers_main.cpp")]
    plain, san = str(out / "solvers"), str(out / "solvers_san")
    subprocess.run(base + ["-o", plain], check=True, capture_output=True, text=True, timeout=300)
    subprocess.run(base + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", san], check=True, capture_output=True, text=True, timeout=300)
    return plain, san


def _run(programs, lines):
    """the answers of both builds (they must be the same text), parsed: one list of floats per line, the tag dropped"""
    text = "\n".join(lines) + "\n"
    outs = []
    for exe in programs:
        r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stderr == "", (exe, r.returncode, r.stderr[-2000:])
        outs.append(r.stdout)
    assert outs[0] == outs[1], "the sanitizer build printed other bits than the plain build"
    rows = [ln.split() for ln in outs[0].splitlines()]
    assert len(rows) == len(lines) and all(row[0] == ln[0] for row, ln in zip(rows, lines))
    return [[float.fromhex(v) for v in row[1:]] for row in rows]


def _hex(values):
    return " ".join(float(v).hex() for v in np.asarray(values, np.float64).reshape(-1))


def _upper(A):
    return [A[p, q] for p in range(A.shape[0]) for q in range(p, A.shape[0])]


def _spd(rng, n, cond):
    """a random symmetric positive definite n x n of 2-norm condition number `cond`: log-uniform eigenvalues between 1 / cond and 1 in a random
    orthonormal frame, symmetrised exactly"""
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    lam = np.exp(rng.uniform(np.log(1.0 / cond), 0.0, n))
    lam[0], lam[1] = 1.0, 1.0 / cond
    A = (Q * lam) @ Q.T
    return 0.5 * (A + A.T)


def _solve_line(A, b):
    return "L " + _hex(_upper(A)) + " " + _hex(b)


# ------------------------------------------------------------------------------------------------ indefinite 6x6 systems
def _indefinite_systems():
    """Symmetric non-singular systems with a leading pivot that is not positive: a well-conditioned positive definite B (condition <= 100) whose
    entry (0, 0) is negated (a negative leading pivot; one negative eigenvalue) or set to zero (a zero leading diagonal entry; e1^T A e1 = 0
    with a non-zero first row makes A indefinite), and the same with the change at entry (k, k), where the unpivoted form meets it later."""
    rng = np.random.default_rng(61)
    out = []
    for trial in range(60):
        B = _spd(rng, 6, 10.0 ** rng.uniform(0, 2))
        b = rng.standard_normal(6)
        for k in (0, 3):
            for value in (-B[k, k], 0.0):
                A = B.copy(); A[k, k] = value
                out.append((A, b, k, value))
    return out


def test_indefinite_systems_are_refused_by_the_fast_form_and_solved_by_the_pivoted_one(programs):
    """icp_ldlt6_fast must say no (its pivots must be positive: the callers then take the pivoted form), icp_ldlt6_pivoted must solve the system
    to within 64 cond 2^-53 |x| of the exact solution (fractions)."""
    systems = _indefinite_systems()
    got = _run(programs, [_solve_line(A, b) for A, b, _, _ in systems])
    worst = 0.0
    for (A, b, k, value), row in zip(systems, got):
        lam = np.linalg.eigvalsh(A)
        assert lam[0] < 0 < lam[-1]                                     # the test's own input: indefinite
        x_exact, rank = psr.exact_solve(A.tolist(), b.tolist())
        assert rank == 6
        x_exact = np.array([float(v) for v in x_exact])
        fast_ok, piv_ok, xp = row[0], row[7], np.array(row[8:14])
        assert fast_ok == 0.0, (k, value)
        assert piv_ok == 1.0, (k, value)
        cond = np.linalg.cond(A)
        err, bound = np.linalg.norm(xp - x_exact), 64.0 * cond * EPS * np.linalg.norm(x_exact)
        worst = max(worst, err / bound)
        assert err <= bound, (k, value, err, bound, cond)
    print(f"indefinite 6x6: {len(systems)} systems, worst error / (64 cond 2^-53 |x|) = {worst:.2e}")


def test_singular_systems_are_refused_by_both_forms(programs):
    """exact zero rows and columns (what a floor, a corridor and a sphere give the device), the zero matrix and a non-finite entry: both forms
    say no -- the callers then let the identity stand in"""
    rng = np.random.default_rng(62)
    lines = []
    for keep in ([0, 1, 5], [0, 1, 2, 3, 5], [3, 4, 5], []):
        B = _spd(rng, 6, 10.0)
        A = np.zeros((6, 6))
        A[np.ix_(keep, keep)] = B[np.ix_(keep, keep)]
        assert np.linalg.matrix_rank(A) == len(keep)
        lines.append(_solve_line(A, rng.standard_normal(6) * np.isin(np.arange(6), keep)))
    for bad in (np.inf, np.nan):
        A = _spd(rng, 6, 10.0); A[2, 2] = bad
        lines.append(_solve_line(A, rng.standard_normal(6)))
    for row in _run(programs, lines):
        assert row[0] == 0.0 and row[7] == 0.0, row


# ------------------------------------------------------------------------------------------------ 10^4 random positive definite systems
def test_random_positive_definite_6x6_systems(programs):
    """5000 systems, condition numbers 1 ... 1e8: both forms solve them, and the residual of each obeys
        |A x - b| <= 64 cond 2^-53 |b|            (the form of the bound on x, carried to the residual: |A| |x| <= cond |b|)
        |A x - b| <= 128 2^-53 |A| |x|            (backward stability of a Cholesky-type solve: (3n + 1) n = 114 roundings for n = 6, Higham 10.4)
    with the residual itself evaluated in extended precision (64-bit mantissa)."""
    rng = np.random.default_rng(63)
    systems = [(_spd(rng, 6, 10.0 ** rng.uniform(0, 8)), rng.standard_normal(6)) for _ in range(5000)]
    got = _run(programs, [_solve_line(A, b) for A, b in systems])
    worst = [0.0, 0.0]
    for n, ((A, b), row) in enumerate(zip(systems, got)):
        assert row[0] == 1.0 and row[7] == 1.0, n
        cond, nA, nb = np.linalg.cond(A), np.linalg.norm(A, 2), np.linalg.norm(b)
        for which, x in enumerate((np.array(row[1:7]), np.array(row[8:14]))):
            res = np.linalg.norm(np.array(A, np.longdouble) @ np.array(x, np.longdouble) - np.array(b, np.longdouble)).astype(np.float64)
            tight = 128.0 * EPS * nA * np.linalg.norm(x)
            worst[which] = max(worst[which], res / tight)
            assert res <= 64.0 * cond * EPS * nb and res <= tight, (n, which, res, tight, cond)
    print(f"positive definite 6x6: worst residual / (128 2^-53 |A| |x|): fast {worst[0]:.2e}, pivoted {worst[1]:.2e}")


def test_random_positive_definite_3x3_inverse_square_roots(programs):
    """5000 matrices, condition numbers 1 ... 1e8 (plus exactly diagonal ones, equal eigenvalues and the identity): |W M W - I| <= 64 cond 2^-53.
    The eigenvalues of the Jacobi iteration carry an absolute error of a few 2^-53 |M|, hence a relative error of that times cond in the
    smallest one, which is what W M W - I sees.  W is symmetric to the last bit (it is assembled from one expression per entry pair)."""
    rng = np.random.default_rng(64)
    mats = [_spd(rng, 3, 10.0 ** rng.uniform(0, 8)) for _ in range(5000)]
    mats += [np.diag([1.0, 1e-3, 1e-6]), np.diag([2.0, 2.0, 2e-3]), np.eye(3), 4.0 * np.eye(3), np.diag([1.0, 1e-3, 1e-6]) + 1e-7 * (1 - np.eye(3))]
    got = _run(programs, ["W " + _hex(_upper(M)) for M in mats])
    worst = 0.0
    for n, (M, row) in enumerate(zip(mats, got)):
        W = np.array(row, np.longdouble).reshape(3, 3)
        assert np.isfinite(np.array(row)).all() and np.array_equal(W, W.T), n
        res = np.linalg.norm((W @ np.array(M, np.longdouble) @ W - np.eye(3)).astype(np.float64), 2)
        bound = 64.0 * np.linalg.cond(M) * EPS
        worst = max(worst, res / bound)
        assert res <= bound, (n, res, bound)
    assert np.array_equal(np.array(got[5002]).reshape(3, 3), np.eye(3))                # the identity: no rotation is made, W = I exactly
    assert np.array_equal(np.array(got[5003]).reshape(3, 3), 0.5 * np.eye(3))
    print(f"inverse square root 3x3: worst |W M W - I| / (64 cond 2^-53) = {worst:.2e}")


# ------------------------------------------------------------------------------------------------ Umeyama from moments
def _moments(src, dst, origin, origin_src):
    u, v = src - origin_src, dst - origin
    return np.concatenate([u.sum(0), v.sum(0), (v[:, :, None] * u[:, None, :]).sum(0).reshape(-1), [(u * u).sum()]])


def _svd_umeyama(src, dst, scaling):
    import correspondence_reference as ref
    return ref.umeyama(src, dst, scaling)


@pytest.mark.parametrize("scaling", [False, True])
def test_umeyama_on_a_mirrored_target_and_half_turns(programs, scaling):
    """the fit from float64 moments against the SVD form: a mirrored target (the reflection fix: det R = +1 and the SVD's pose), rotations by
    exactly pi (the quaternion's w = 0) and the identity"""
    rng = np.random.default_rng(65)
    src = rng.uniform(-2, 2, (300, 3))
    a = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    cases = {"mirror": src * [1, 1, -1], "pi about z": src * [-1, -1, 1], "pi about (1,2,3)": src @ (2.0 * np.outer(a, a) - np.eye(3)).T + [0.1, 0.2, -0.3],
             "identity": src.copy()}
    lines = ["U " + _hex([float(scaling), len(src)]) + " " + _hex(dst[0]) + " " + _hex(src[0]) + " " + _hex(_moments(src, dst, dst[0], src[0])) for dst in cases.values()]
    for (name, dst), row in zip(cases.items(), _run(programs, lines)):
        T, T_ref = np.array(row).reshape(4, 4), _svd_umeyama(src, dst, scaling)
        c = np.cbrt(np.linalg.det(T[:3, :3]))
        assert c > 0 and abs(np.linalg.det(T[:3, :3] / c) - 1.0) < 1e-9, name
        assert np.abs(T - T_ref).max() < 1e-9, (name, np.abs(T - T_ref).max())


def test_l1_weight_at_a_zero_residual(programs):
    """1 / max(|r|, 1e-300): finite at r = 0 (Open3D divides by zero), 1 / |r| everywhere else"""
    rows = _run(programs, ["K " + _hex([1, 1.0, r]) for r in (0.0, -0.0, 1e-310, 0.25, -4.0)] + ["K " + _hex([2, 0.5, 0.5]), "K " + _hex([0, 0.5, 0.5])])
    assert [r[0] for r in rows] == [1.0 / 1e-300, 1.0 / 1e-300, 1.0 / 1e-300, 4.0, 0.25, 0.5 / (0.5 + 0.25) ** 2, 1.0]
