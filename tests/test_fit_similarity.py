"""CPU test: vslam_fit_similarity (csrc/transform.hip, host code only) through the C ABI: exact synthetic data is recovered, noisy data is
fitted as well as a numpy SVD statement of Umeyama's closed form fits it, mirrored data still gives a proper rotation, and every refusal."""
import ctypes as C

import numpy as np
import pytest

import transform_ref as tr
from visualslam_android_amd import capi

E_INVALID = -1
RECOVER = 1e-10


def truth(rng, s=None):
    R = tr.rotation(rng.normal(size=3), rng.uniform(0.2, 3.0))
    return R, rng.normal(size=3) * 2.0, float(np.exp(rng.uniform(-1.5, 1.5))) if s is None else s


def umeyama(a, b, w=None, fix_scale=False):
    """Umeyama 1991 with numpy's SVD -> (R, t, s, weighted rms)"""
    w = np.ones(len(a)) if w is None else np.asarray(w, np.float64)
    w = w / w.sum()
    ma, mb = w @ a, w @ b
    da, db = a - ma, b - mb
    U, D, Vt = np.linalg.svd((db * w[:, None]).T @ da)
    S = np.diag([1.0, 1.0, np.sign(np.linalg.det(U) * np.linalg.det(Vt))])
    R = U @ S @ Vt
    s = 1.0 if fix_scale else float((D * np.diag(S)).sum() / (w @ (da * da).sum(axis=1)))
    t = mb - s * R @ ma
    return R, t, s, float(np.sqrt(w @ ((b - (s * a @ R.T + t)) ** 2).sum(axis=1)))


def points(rng, n):
    if n == 3:
        return np.array([[0.1, 0.2, 0.3], [1.3, -0.2, 0.5], [0.4, 0.9, -0.6]])
    if n == 4:
        return np.array([[0.0, 0.0, 0.0], [1.0, 0.1, 0.0], [0.2, 1.1, 0.1], [0.3, 0.2, 0.9]])
    return rng.uniform(0, 1, size=(n, 3))


@pytest.mark.parametrize("n", [3, 4, 100])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("fix_scale", [False, True])
def test_exact_data_is_recovered(n, weighted, fix_scale):
    rng = np.random.default_rng(1000 * n + 10 * weighted + fix_scale)
    R, t, s = truth(rng, 1.0 if fix_scale else None)
    a = points(rng, n)
    b = s * a @ R.T + t
    w = rng.uniform(0.2, 3.0, size=n) if weighted else None
    q, sc, rms = capi.fit_similarity(a, b, w, fix_scale)
    err = max(np.abs(q[:9].reshape(3, 3) - R).max(), np.abs(q[9:] - t).max(), abs(sc - s))
    print("n %d weighted %d fix_scale %d: recovery error %.3e, rms %.3e" % (n, weighted, fix_scale, err, rms))
    assert err <= RECOVER and rms <= RECOVER
    assert abs(np.linalg.det(q[:9].reshape(3, 3)) - 1.0) < 1e-12
    if fix_scale:
        assert sc == 1.0


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("fix_scale", [False, True])
def test_noisy_data_is_fitted_as_well_as_numpy_fits_it(weighted, fix_scale):
    rng = np.random.default_rng(77 + 2 * weighted + fix_scale)
    R, t, s = truth(rng)
    a = rng.uniform(-1, 1, size=(60, 3))
    b = s * a @ R.T + t + rng.normal(size=(60, 3)) * 0.02
    w = rng.uniform(0.0, 2.0, size=60) if weighted else None
    if weighted:
        w[5] = 0.0
    q, sc, rms = capi.fit_similarity(a, b, w, fix_scale)
    Rn, tn, sn, rms_n = umeyama(a, b, w, fix_scale)
    print("noisy, weighted %d fix_scale %d: rms %.9e, numpy %.9e" % (weighted, fix_scale, rms, rms_n))
    assert rms <= rms_n * (1 + 1e-9)
    assert np.abs(q[:9].reshape(3, 3) - Rn).max() < 1e-9 and np.abs(q[9:] - tn).max() < 1e-9 and abs(sc - sn) < 1e-9


def test_a_mirrored_set_still_gives_a_proper_rotation():
    rng = np.random.default_rng(5)
    R, t, s = truth(rng)
    a = rng.uniform(-1, 1, size=(40, 3))
    b = s * (a * [1, 1, -1]) @ R.T + t                                # no rotation maps a onto its mirror image
    q, sc, rms = capi.fit_similarity(a, b)
    Rn, tn, sn, rms_n = umeyama(a, b)
    assert abs(np.linalg.det(q[:9].reshape(3, 3)) - 1.0) < 1e-12 and np.abs(q[:9].reshape(3, 3).T @ q[:9].reshape(3, 3) - np.eye(3)).max() < 1e-12
    assert sc > 0 and rms > 0.1 and rms <= rms_n * (1 + 1e-9)
    # a planar set mirrored in its own plane is a rotated set: three points always are
    a3 = points(rng, 3)
    q, sc, rms = capi.fit_similarity(a3, s * a3 @ R.T + t)
    assert abs(np.linalg.det(q[:9].reshape(3, 3)) - 1.0) < 1e-12 and rms < RECOVER


def fit_rc(n, a, b, w=None):
    lib = capi.load_library()
    q, s, rms = np.zeros(12), C.c_double(0.0), C.c_double(0.0)
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    w = None if w is None else np.ascontiguousarray(w, np.float64)
    return lib.vslam_fit_similarity(n, a.ctypes.data, b.ctypes.data, None if w is None else w.ctypes.data, 0, q.ctypes.data, C.byref(s), C.byref(rms))


def test_refusals():
    rng = np.random.default_rng(9)
    a = rng.uniform(-1, 1, size=(6, 3))
    b = a + 1.0
    assert fit_rc(6, a, b) == 0
    assert fit_rc(2, a, b) == E_INVALID and fit_rc(0, a, b) == E_INVALID and fit_rc(-1, a, b) == E_INVALID
    for bad in (np.nan, np.inf, -np.inf):
        x = a.copy(); x[3, 1] = bad
        assert fit_rc(6, x, b) == E_INVALID and fit_rc(6, a, x) == E_INVALID
        w = np.ones(6); w[2] = bad
        assert fit_rc(6, a, b, w) == E_INVALID
    w = np.ones(6); w[4] = -1e-3
    assert fit_rc(6, a, b, w) == E_INVALID
    line = np.outer(np.linspace(-1, 2, 6), [0.3, -0.5, 0.8]) + [4.0, 5.0, 6.0]
    assert fit_rc(6, line, b) == E_INVALID                            # collinear
    assert fit_rc(6, np.tile([1.0, 2.0, 3.0], (6, 1)), b) == E_INVALID   # coincident
    near = line.copy(); near[2] += np.array([0.8, 0.0, -0.3]) * 1e-13
    assert fit_rc(6, near, b) == E_INVALID                            # within 1e-12 of the extent
    off = line.copy(); off[2] += np.array([0.8, 0.0, -0.3]) * 1e-6
    assert fit_rc(6, off, off * 2.0) == 0                             # far outside it: a rotation is determined
    w = np.array([1.0, 1.0, 0.0, 0.0, 0.0, 0.0])
    assert fit_rc(6, a, b, w) == E_INVALID                            # two correspondences carry weight
    assert b"fit_similarity" in capi.load_library().vslam_last_error()
    lib = capi.load_library()
    q = np.zeros(12)
    assert lib.vslam_fit_similarity(6, None, b.ctypes.data, None, 0, q.ctypes.data, None, None) == E_INVALID
    assert lib.vslam_fit_similarity(6, a.ctypes.data, b.ctypes.data, None, 0, None, None, None) == E_INVALID
    assert lib.vslam_fit_similarity(6, a.ctypes.data, b.ctypes.data, None, 0, q.ctypes.data, None, None) == 0   # scale and rms are optional
