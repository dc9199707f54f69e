"""Reference side of the pose iteration's tail (csrc/dev_math.h: wave_pose_solve, wave_pose_apply) and its test cases.

lu_solve is a line-by-line transcription of lu_solve_n (csrc/dev_math.h; the oracle's orc::lu_solve is the same text): Python floats
are IEEE doubles and Python never fuses a multiply with an addition.  pose_mul transcribes pose_mul the same way."""
import numpy as np


def lu_solve(A, b, n):
    """In place on the lists A (n * n, row-major) and b (n); -> (ok, pivots)."""
    pivots = []
    for k in range(n):
        piv = k
        best = abs(A[k * n + k])
        for r in range(k + 1, n):
            if abs(A[r * n + k]) > best:
                best = abs(A[r * n + k])
                piv = r
        if best == 0.0:
            return False, pivots
        pivots.append(piv)
        if piv != k:
            for c in range(n):
                t = A[k * n + c]
                A[k * n + c] = A[piv * n + c]
                A[piv * n + c] = t
            t = b[k]
            b[k] = b[piv]
            b[piv] = t
        inv = 1.0 / A[k * n + k]
        for r in range(k + 1, n):
            f = A[r * n + k] * inv
            if f == 0.0:
                continue
            for c in range(k + 1, n):
                A[r * n + c] -= f * A[k * n + c]
            b[r] -= f * b[k]
    for k in range(n - 1, -1, -1):
        s = b[k]
        for c in range(k + 1, n):
            s -= A[k * n + c] * b[c]
        b[k] = s / A[k * n + k]
    return True, pivots


def system_from_sums(sums27):
    """myWLS::compute's mirror of the upper triangle (jni/myWLS.h:54-58) -> (C as a list of 36, v as a list of 6)."""
    s = [float(x) for x in sums27]
    C = [0.0] * 36
    q = 0
    for r in range(6):
        for c in range(r, 6):
            C[r * 6 + c] = s[q]
            C[c * 6 + r] = s[q]
            q += 1
    return C, s[21:27]


def sums_from_system(C, v):
    C = np.asarray(C, np.float64).reshape(6, 6)
    assert np.array_equal(C, C.T)
    return np.array([C[r, c] for r in range(6) for c in range(r, 6)] + [float(x) for x in v])


def solve_update(sums27):
    """-> (update [6] (zero when the system is singular), ok, pivots)"""
    C, v = system_from_sums(sums27)
    ok, piv = lu_solve(C, v, 6)
    return np.array(v if ok else [0.0] * 6), ok, piv


def pose_mul(a, b):
    """pose12 * pose12 (R row-major, then t), csrc/dev_math.h pose_mul."""
    a = [float(x) for x in a]
    b = [float(x) for x in b]
    r = [0.0] * 12
    for i in range(3):
        for j in range(3):
            r[i * 3 + j] = a[i * 3 + 0] * b[0 * 3 + j] + a[i * 3 + 1] * b[1 * 3 + j] + a[i * 3 + 2] * b[2 * 3 + j]
    for i in range(3):
        r[9 + i] = a[9 + i] + (a[i * 3 + 0] * b[9] + a[i * 3 + 1] * b[10] + a[i * 3 + 2] * b[11])
    return np.array(r)


def _sym(rng, diag, off):
    C = rng.uniform(-1.0, 1.0, (6, 6)) * off
    C = np.triu(C, 1)
    C = C + C.T
    C[np.diag_indices(6)] = diag
    return C


def _unit_system(v):
    return sums_from_system(np.eye(6), v)          # C = I: the update is v itself


def cases():
    """name -> (sums [27], pose12 [12], what the transcription must report: 'pivots' list / 'singular' / None)"""
    out = {}
    rng = np.random.default_rng(11)
    w = rng.uniform(-0.3, 0.3, 3)
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    R = np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * (K @ K)
    pose = np.concatenate([R.reshape(9), rng.uniform(-2.0, 2.0, 3)])

    J = rng.uniform(-1.0, 1.0, (40, 6)) * np.array([300.0, 300.0, 100.0, 400.0, 400.0, 200.0])
    C = J.T @ J + 100.0 * np.eye(6)
    C = np.triu(C) + np.triu(C, 1).T
    out["spd"] = (sums_from_system(C, C @ rng.uniform(-0.02, 0.02, 6)), pose, None)

    for seed in range(1000):                       # a symmetric system whose elimination changes rows at every column
        r2 = np.random.default_rng(100 + seed)
        C = _sym(r2, np.arange(1, 7) * 1e-3, 1.0) + np.triu(np.ones((6, 6)), 1) + np.tril(np.ones((6, 6)), -1)
        s = sums_from_system(C, C @ r2.uniform(-0.05, 0.05, 6))
        _, ok, piv = solve_update(s)
        if ok and all(piv[k] != k for k in range(5)):
            out["swap_every_step"] = (s, pose, "swaps")
            break

    C = _sym(rng, 7.0, 0.5)
    C[0, 0] = 2.0; C[0, 1] = C[1, 0] = -2.0; C[0, 2] = C[2, 0] = 2.0          # column 0: |2| three times, the lowest row stays
    out["tie_keeps_row"] = (sums_from_system(C, rng.uniform(-0.1, 0.1, 6)), pose, [0])
    C = _sym(rng, 7.0, 0.5)
    C[0, 0] = 1.0; C[0, 1] = C[1, 0] = 3.0; C[0, 2] = C[2, 0] = -3.0; C[0, 4] = C[4, 0] = 3.0   # rows 1, 2, 4 tie: row 1
    out["tie_first_of_equals"] = (sums_from_system(C, rng.uniform(-0.1, 0.1, 6)), pose, [1])

    C = _sym(rng, 5.0, 0.5)
    C[0, :] = 0.0; C[:, 0] = 0.0
    out["zero_column_first"] = (sums_from_system(C, rng.uniform(-0.1, 0.1, 6)), pose, "singular")
    C = np.diag([4.0, 3.0, 2.0, 0.0, 5.0, 6.0])
    out["zero_column_later"] = (sums_from_system(C, rng.uniform(-0.1, 0.1, 6)), pose, "singular")
    out["all_zero"] = (np.zeros(27), pose, "singular")                      # no measurement found

    C = _sym(rng, 9.0, 1.0)
    out["zero_vector"] = (sums_from_system(C, np.zeros(6)), pose, None)

    def rot(theta):
        a = np.array([0.6, -0.48, 0.64])           # unit axis
        return np.concatenate([[0.01, -0.02, 0.03], a * theta])
    out["rotation_1e-9"] = (_unit_system(rot(1e-9)), pose, None)            # theta^2 < 1e-8
    out["rotation_5e-4"] = (_unit_system(rot(5e-4)), pose, None)            # 1e-8 <= theta^2 < 1e-6
    out["rotation_2e-2"] = (_unit_system(rot(2e-2)), pose, None)            # sin / cos
    out["rotation_near_pi"] = (_unit_system(rot(3.14159)), pose, None)
    return out


CASES = cases()
