"""CPU: the product's bootstrap mathematics (csrc/bootstrap_math.h) compiled for the host (oracle/bootmath_host.cpp), function by
function against a plain high-precision statement of the operation (numpy longdouble where a residual is formed, numpy.linalg as the
second factorisation), and its two serial pipelines against the oracle's independent restatement (oracle/homography.cpp).
tests/test_gpu_bootstrap_stages.py then holds the device to this host build bit for bit.  PARITY UNPINNED against the reference."""
import numpy as np
import pytest

import boot_cases as bc
import oracle.binding as orc
from test_oracle_bootstrap import _rot

B = orc.BootMath
LD = np.longdouble
EPS = np.finfo(np.float64).eps


def _minimal_matrix(m8):
    """the 2n x 9 (at least 9 x 9) matrix of HomographyFromMatches, jni/HomographyInit.cc:75-116"""
    rows = max(2 * len(m8), 9)
    A = np.zeros((rows, 9))
    for k, (x, y, u, v) in enumerate(m8[:, :4]):
        A[2 * k] = [x, y, 1, 0, 0, 0, -x * u, -y * u, -u]
        A[2 * k + 1] = [0, 0, 0, x, y, 1, -x * v, -y * v, -v]
    return A


def _svd_cases():
    rng = np.random.default_rng(7)
    m8 = bc.tilted(2, 40)
    Q1, Q2 = np.linalg.qr(rng.normal(size=(3, 3)))[0], np.linalg.qr(rng.normal(size=(3, 3)))[0]
    return {"3x3": rng.normal(size=(3, 3)), "9x9 rank 8": _minimal_matrix(m8[:4]), "18x9": _minimal_matrix(m8[:9]),
            "two equal, diagonal": np.diag([3.0, 3.0, 1.0]), "two equal, rotated": Q1 @ np.diag([2.0, 2.0, 0.5]) @ Q2.T, "zero": np.zeros((3, 3))}


def _svd_residuals(A, U, S, V):
    """(|| V^T V - I ||, || A - U diag(S) V^T ||), Frobenius, formed in longdouble"""
    A, U, S, V = (np.asarray(x, LD) for x in (A, U, S, V))
    return float(np.linalg.norm(V.T @ V - np.eye(V.shape[1], dtype=LD))), float(np.linalg.norm(A - (U * S) @ V.T))


@pytest.mark.parametrize("name", list(_svd_cases()))
def test_svd_onesided_against_numpy(name):
    """bm::svd_onesided: singular values against numpy.linalg.svd within 2 max(m, n) eps sigma_max (each factorisation is backward stable to
    about max(m, n) eps ||A||, and a perturbation moves a singular value by at most its norm), decreasing order, and the residuals
    || V^T V - I || and || A - U S V^T || within 16 x the same residual of numpy's factors of the same matrix.
    Measured (ours / numpy's; orthogonality, then reconstruction):  3x3 1.2e-15 / 7.3e-16 and 3.0e-15 / 2.3e-15;  9x9 rank 8 3.6e-15 / 1.9e-15
    and 4.4e-15 / 1.9e-15;  18x9 4.5e-15 / 2.1e-15 and 7.1e-15 / 2.9e-15;  two equal rotated 2.8e-16 / 1.2e-16 and 4.5e-16 / 1.6e-15;  the
    diagonal and the zero matrix 0 / 0 on both sides (no rotation is made, V stays the identity)."""
    A = _svd_cases()[name]
    m, n = A.shape
    AS, V, S, order = B.svd_onesided(A)
    s_sorted = S[order]
    assert np.all(np.diff(s_sorted) <= 0), s_sorted
    un, sn, vtn = np.linalg.svd(A, full_matrices=False)
    assert np.abs(s_sorted - sn).max() <= 2 * max(m, n) * EPS * max(sn[0], 0.0), (s_sorted, sn)
    assert np.array_equal(S, np.sqrt((AS * AS).sum(0))) or np.allclose(S, np.linalg.norm(AS, axis=0), rtol=4 * EPS, atol=0)   # S = the column norms of what the rotations left
    U = np.where(S > 0, AS / np.where(S > 0, S, 1.0), 0.0)
    ours, ref = _svd_residuals(A, U, S, V), _svd_residuals(A, un, sn, vtn.T)
    print("svd %s: V orth %.3g (numpy %.3g), reconstruction %.3g (numpy %.3g)" % (name, ours[0], ref[0], ours[1], ref[1]))
    assert ours[0] <= 16 * ref[0] and ours[1] <= 16 * ref[1], (ours, ref)
    nz = S > 1e-9 * max(sn[0], 1e-300)                                   # the columns of U that carry a direction are orthonormal
    Un = np.asarray(U[:, nz], LD)
    assert float(np.linalg.norm(Un.T @ Un - np.eye(int(nz.sum()), dtype=LD))) <= 16 * max(float(np.linalg.norm(np.asarray(un, LD).T @ np.asarray(un, LD) - np.eye(n, dtype=LD))), EPS)


def _normal_matrix(H, m8, inl):
    """the 9 x 9 system of one RefineHomographyWithInliers step (jni/HomographyInit.cc:133-199): prior 1, Tukey weights, integer-cast errors"""
    H = np.asarray(H, float).reshape(3, 3)
    rows, errs = [], []
    for q in m8[inl]:
        un = np.array([q[0], q[1], 1.0]); s = H @ un
        d = q[2:4] - s[:2] / s[2]
        Jp = q[4:].reshape(2, 2)
        J = np.zeros((2, 9))
        J[0, :3] = un / s[2]; J[0, 6:] = -un * s[0] / s[2] ** 2
        J[1, 3:6] = un / s[2]; J[1, 6:] = -un * s[1] / s[2] ** 2
        rows.append(Jp @ J); errs.append(Jp @ d)
    e2 = np.array([e @ e for e in errs])
    sigma = 4.6851 * 1.4826 * (1 + 5.0 / (len(inl) * 2 - 6)) * np.sqrt(np.sort(e2)[len(inl) // 2])
    Cm, v = np.eye(9), np.zeros(9)
    for PJ, e, es in zip(rows, errs, e2):
        w = 0.0 if es > sigma ** 2 else (1 - es / sigma ** 2) ** 2
        for r in range(2):
            Cm += w * np.outer(PJ[r], PJ[r]); v += float(int(e[r])) * w * PJ[r]
    return Cm, v


def _solve_longdouble(A, b):
    A, b = np.array(A, LD), np.array(b, LD)
    n = len(b)
    for k in range(n):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        A[[k, p]] = A[[p, k]]; b[[k, p]] = b[[p, k]]
        for r in range(k + 1, n):
            f = A[r, k] / A[k, k]
            A[r, k:] -= f * A[k, k:]; b[r] -= f * b[k]
    x = np.zeros(n, LD)
    for k in range(n - 1, -1, -1):
        x[k] = (b[k] - A[k, k + 1:] @ x[k + 1:]) / A[k, k]
    return x


def test_lu_solve_on_the_normal_matrices_of_the_refinement():
    """bm::lu_solve on the 9 x 9 systems RefineHomographyWithInliers forms (noisy matches, so that the integer-cast errors are not all zero)
    against elimination in longdouble: forward error within 8 n eps cond_2(A) ||x||_inf, the first-order bound of partial-pivot elimination
    with its usual small growth.  Measured: cond 7.2e7 .. 8.0e7, error 8.7e-14 .. 4.7e-13 against bounds of 7.2e-9 .. 1.2e-8.  A matrix with a zero column, and one
    with two equal rows, return false."""
    for seed in (1, 2, 3):
        m8, _, _ = bc._planar_matches(seed, n=120, outliers=12, noise=4e-3)
        rec = B.homography_pipeline(m8, seed)
        inl = bc.arr(rec.inliers)[:rec.n_inliers]
        Cm, v = _normal_matrix(rec.H_mlesac, m8, inl)
        assert np.abs(v).max() > 0                                           # a step that moves
        ok, x = B.lu_solve(Cm, v)
        want = _solve_longdouble(Cm, v)
        err, bound = float(np.abs(np.asarray(x, LD) - want).max()), 8 * 9 * EPS * np.linalg.cond(Cm) * float(np.abs(want).max())
        print("lu_solve seed %d: cond %.3g, error %.3g, bound %.3g" % (seed, np.linalg.cond(Cm), err, bound))
        assert ok and err <= bound, (seed, err, bound)
        # ... and the step refine_homography takes is the solution of that system
        H1 = B.refine_homography(rec.H_mlesac, m8, inl)
        assert np.abs((H1 - bc.arr(rec.H_mlesac)) - x).max() <= 64 * EPS * np.abs(x).max() + bound, seed
    Z = np.array(Cm); Z[:, 4] = 0.0
    assert not B.lu_solve(Z, v)[0]
    Z = np.array(Cm); Z[7] = Z[2]
    assert not B.lu_solve(Z, v)[0]
    assert B.lu_solve(np.eye(9), v)[0] and np.array_equal(B.lu_solve(np.eye(9), v)[1], v)


def test_kth_smallest_is_the_order_statistic():
    """bm::kth_smallest against numpy.sort, exactly, for every k: n = 1, 2, random, many ties, all equal"""
    rng = np.random.default_rng(3)
    cases = [np.array([2.5]), np.array([2.0, 1.0]), np.array([1.0, 2.0]), rng.normal(size=37), rng.integers(0, 4, 50).astype(float), np.full(17, 0.25),
             rng.normal(size=270) ** 2]
    for v in cases:
        want = np.sort(v)
        for k in range(len(v)):
            assert B.kth_smallest(v, k) == want[k], (len(v), k)


MOTIONS = [(_rot(1, 0.05) @ _rot(0, -0.03) @ _rot(2, 0.02), [0.2, 0.01, -0.02], [0.1, -0.05, 1.0], 2.0),
           (_rot(0, 0.2) @ _rot(2, -0.1), [0.0, 0.05, -0.4], [0.0, 0.0, 1.0], 1.5),
           (np.eye(3), [0.3, 0.0, 0.0], [0.3, 0.2, 1.0], 3.0)]


@pytest.mark.parametrize("case", range(len(MOTIONS)))
def test_decompose_homography_returns_eight_motions_of_the_homography(case):
    """bm::decompose_homography on H = d R + t n^T of known motions: eight results, every R orthonormal with determinant +1, every
    d R + t n^T the input up to scale (formed in longdouble), the true motion among them.  The bars follow from the conditioning of the
    Faugeras-Lustman construction, which divides by the gaps of H's singular values: 64 eps (d1 / min gap)^2 for the motion, 64 eps
    d1 / d3 for orthonormality and reconstruction.  Measured: orthonormality <= 3.1e-15 and reconstruction <= 7.8e-16 against
    1.6e-14 at the least; the true motion <= 6.9e-15 against 7.3e-12 at the least."""
    R, t, n, d = MOTIONS[case]
    t, n = np.array(t, float), np.array(n, float) / np.linalg.norm(n)
    H = d * R + np.outer(t, n)
    sv = np.linalg.svd(H)[1]
    bar_o, bar_m = 64 * EPS * sv[0] / sv[2], 64 * EPS * (sv[0] / min(sv[0] - sv[1], sv[1] - sv[2])) ** 2
    res = B.decompose_homography(H)
    assert len(res) == 8
    worst_o = worst_h = 0.0
    best = np.inf
    for (Ri, ti, ni, di) in res:
        Rl = np.asarray(Ri, LD)
        worst_o = max(worst_o, float(np.abs(Rl @ Rl.T - np.eye(3, dtype=LD)).max()), abs(float(np.linalg.det(Ri)) - 1.0))
        Hi = np.asarray(di, LD) * Rl + np.outer(np.asarray(ti, LD), np.asarray(ni, LD))
        worst_h = max(worst_h, float(np.abs(bc.normalised_h(np.asarray(Hi, float)) - bc.normalised_h(H)).max()))
        sgn = 1.0 if ni @ n > 0 else -1.0                                  # (t, n) and (-t, -n) are the same motion
        best = min(best, max(np.abs(Ri - R).max(), np.abs(sgn * ti - t).max(), np.abs(sgn * ni - n).max(), abs(di - d)))
    print("decompose %d: orthonormality %.3g (bar %.3g), reconstruction %.3g, true motion %.3g (bar %.3g)" % (case, worst_o, bar_o, worst_h, best, bar_m))
    assert worst_o <= bar_o and worst_h <= bar_o and best <= bar_m, (worst_o, worst_h, best)


def test_decompose_homography_refuses_equal_singular_values():
    assert B.decompose_homography(np.eye(3)) == []                          # d1 == d2 == d3
    assert B.decompose_homography(np.diag([2.0, 2.0, 1.0])) == []           # d1 == d2
    assert len(B.decompose_homography(np.diag([3.0, 2.0, 1.0]))) == 8


def test_sym3_smallest_eigenvector_against_eigh():
    """bm::sym3_smallest_eigenvector against numpy.linalg.eigh, up to sign, within 16 eps ||M|| / gap (Davis-Kahan: a symmetric perturbation E
    turns an eigenvector by at most ||E|| / gap, and each solver is backward stable to a few eps ||M||): a scatter matrix, a diagonal matrix,
    a repeated LARGEST eigenvalue (the smallest stays simple); a zero matrix gives a finite unit vector.  Measured: <= 3.3e-16 against bars >= 4.2e-15."""
    rng = np.random.default_rng(5)
    X = rng.normal(size=(50, 3)) * [1.0, 0.6, 0.01]
    Q = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    cases = {"scatter": (X @ Q.T).T @ (X @ Q.T), "diagonal": np.diag([3.0, 0.5, 2.0]), "repeated largest": Q @ np.diag([2.0, 2.0, 0.3]) @ Q.T}
    for name, M in cases.items():
        M = (M + M.T) / 2
        w, v = np.linalg.eigh(M)
        got = B.sym3_smallest_eigenvector(M)
        want = v[:, 0] if v[:, 0] @ got > 0 else -v[:, 0]
        err, bar = np.abs(got - want).max(), 16 * EPS * np.abs(w).max() / (w[1] - w[0])
        print("sym3 %s: %.3g (bar %.3g)" % (name, err, bar))
        assert err <= bar and abs(np.linalg.norm(got) - 1.0) <= 8 * EPS, (name, err, bar)
    z = B.sym3_smallest_eigenvector(np.zeros((3, 3)))
    assert np.all(np.isfinite(z)) and np.linalg.norm(z) == 1.0


# ---- the serial pipelines against the oracle ------------------------------------------------------------------------------------
def _grid():
    out = []
    for seed in range(1, 13):
        for n in (8, 12, 40, 200, 300):
            out.append(("tilted seed %d n %d" % (seed, n), bc.tilted(seed, n), seed))
    for n in (4, 9, 10, 1000):
        out.append(("tilted n %d" % n, bc.tilted(21, n), 21))
    out.append(("fronto-parallel, x translation", bc.fronto_parallel(3, 200, [0.2, 0.0, 0.0], outliers=10), 3))
    out.append(("fronto-parallel, z translation", bc.fronto_parallel(3, 200, [0.0, 0.0, -0.3], outliers=10), 3))
    out.append(("quantised to 1/500", bc.quantised(bc.tilted(5, 200)), 5))
    out.append(("all outliers", bc.all_outliers(6, 60), 6))
    out.append(("every match three times", np.repeat(bc.tilted(7, 60), 3, axis=0), 7))
    out.append(("2-pixel noise (the refinement moves)", bc._planar_matches(8, n=200, outliers=20, noise=4e-3)[0], 8))
    return out


def test_host_homography_pipeline_against_the_oracle():
    """The serial restatement of boot_homography_stage over the host build against the oracle's HomographyInit (two-sided Jacobi SVD, its own
    elimination) on well-conditioned input: ok, the inlier index list (= the best trial's inlier set) and the branch of ChooseBestDecomposition
    exactly; the MLESAC and the refined homography (unit norm, largest element positive) and every pose element within 16 x the spread of
    the ORACLE's outputs over three seeded +-1 ulp perturbations of every input double, not below 1e-13.
    Measured over the 70 cases: 68 differ from the oracle by less than the 1e-13 floor (largest: pose 1.7e-14 at an oracle spread of 1.6e-14,
    H 8.8e-15 at 1.2e-14).  Two are held by 16 x their own spread: "quantised to 1/500", pose difference 2.3e-13 at a spread of 6.2e-14
    (bar 9.9e-13), and "2-pixel noise", where alone the refinement moves the homography: H_refined 5.4e-14 at a spread of 9.5e-14, pose
    1.6e-13 at 2.2e-13.  69 cases take the unambiguous branch of the choice, the fronto-parallel z translation the ambiguous one."""
    rep = []
    took = {0: 0, 1: 0, 2: 0}
    for tag, m8, seed in _grid():
        rec = B.homography_pipeline(m8, seed, 5.0, bc.WIGGLE)
        bc.check_homography_against_oracle(rec, m8, seed, tag, rep)
        assert rec.best_trial == (bc.first_argmin(rec.scores[:]) if len(m8) >= 10 else -1), tag
        if rec.ok:
            took[rec.choice] += 1
            assert abs(np.linalg.norm(bc.arr(rec.t_scaled)) - bc.WIGGLE) <= 4 * EPS and np.abs(np.cross(bc.arr(rec.t_scaled), bc.arr(rec.t))).max() <= 8 * EPS * np.linalg.norm(bc.arr(rec.t)), tag
    print("homography pipeline: max spread H %.3g pose %.3g; max diff H %.3g pose %.3g; pose diff without the all-outlier case %.3g; branches %r" % (
        max(max(s["H_mlesac"], s["H_refined"]) for _, _, s in rep), max(s["pose"] for _, _, s in rep),
        max(max(d["H_mlesac"], d["H_refined"]) for _, d, _ in rep), max(d["pose"] for _, d, _ in rep),
        max(d["pose"] for t, d, _ in rep if t != "all outliers"), took))
    assert took[0] > 0 and took[1] + took[2] > 0                             # both branches of the choice were compared


@pytest.mark.parametrize("n", [10, 100, 500])
def test_host_plane_pipeline_against_the_oracle(n):
    """boot_plane_stage restated serially against the oracle's CalcPlaneAligner (closed-form eigenvector) on the scene of
    test_plane_aligner_puts_the_dominant_plane_at_z_zero: the RANSAC's mean and normal and the aligner under the rule above.
    Measured: oracle spread <= 1.1e-15, difference 0 for mean and normal (the same expressions) and <= 4.4e-16 for the aligner."""
    pos = bc.plane_cloud(n)
    rec = B.plane_pipeline(pos, 1)
    diff, spread = bc.check_plane_against_oracle(rec, pos, 1, "n %d" % n)
    print("plane pipeline n %d: diff %r spread %r" % (n, diff, spread))
    assert rec.have == 1 and rec.best_trial == int(np.argmin(np.where(np.array(rec.sums[:]) < 0, np.inf, np.array(rec.sums[:]))))
    R = bc.arr(rec.R).reshape(3, 3)
    assert np.abs(R @ R.T - np.eye(3)).max() <= 16 * EPS and R[2, 2] <= 0
    assert B.plane_pipeline(pos[:9], 1).have == 0                         # fewer than ten points (:1107-1110)
