"""Inputs, references and comparisons shared by tests/test_bootmath_host.py (CPU) and tests/test_gpu_bootstrap_stages.py (GPU):
synthetic match sets and point clouds for the two bootstrap stages, the bar a comparison with the oracle gets, and the bit-wise
comparison of two stage records.  No GPU is touched here."""
import ctypes as C
import functools

import numpy as np

import oracle.binding as orc
from test_oracle_bootstrap import _planar_matches, _rot

WIGGLE = 0.1                                   # vslam_params.wiggle_scale's default
JAC = [500.0, 0.0, 0.0, 500.0]                 # a pixel Jacobian: 500 pixels per unit of the z = 1 plane
BAR_FACTOR, BAR_FLOOR = 16.0, 1e-13


def matches_of_motion(P, R, t, rng=None, noise=0.0):
    """(n, 8) matches of the 3-D points P (first camera's frame) seen again after x -> R x + t"""
    Q = (R @ P.T).T + t
    first, second = P[:, :2] / P[:, 2:], Q[:, :2] / Q[:, 2:]
    if noise:
        second = second + rng.normal(0, noise, second.shape)
    return np.c_[first, second, np.tile(JAC, (len(P), 1))]


def tilted(seed, n, outliers=None, where="first"):
    """test_oracle_bootstrap._planar_matches (a tilted plane, rotation + sideways translation) with a tenth of gross outliers, at the
    first or the last indices"""
    k = n // 10 if outliers is None else outliers
    m8, R, t = _planar_matches(seed, n=n, outliers=k)
    if where == "last":
        m8 = m8[::-1].copy()
    return m8


def fronto_parallel(seed, n, t, outliers=0, noise=1e-4, depth=2.0):
    """a plane z = depth facing the first camera, pure translation t (+ a small rotation about z): with t along z the visibility votes
    of ChooseBestDecomposition cannot separate the two physical solutions"""
    rng = np.random.default_rng(seed)
    P = np.c_[rng.uniform(-1, 1, n), rng.uniform(-0.8, 0.8, n), np.full(n, depth)]
    m8 = matches_of_motion(P, _rot(2, 0.01), np.asarray(t, float), rng, noise)
    m8[:outliers, 2:4] += rng.uniform(-0.1, 0.1, (outliers, 2))
    return m8


def quantised(m8, q=500.0):
    m = m8.copy()
    m[:, :4] = np.round(m[:, :4] * q) / q
    return m


def all_outliers(seed, n):
    rng = np.random.default_rng(seed)
    return np.c_[rng.uniform(-1, 1, (n, 2)), rng.uniform(-1, 1, (n, 2)), np.tile(JAC, (n, 1))]


def degenerate(kind, seed=1, n=60):
    """match sets HomographyInit has no answer for: their `ok` hangs on the last bits of an SVD, so only device == host is asked of them"""
    rng = np.random.default_rng(seed)
    P = np.c_[rng.uniform(-1, 1, n), rng.uniform(-0.8, 0.8, n), 2.0 + rng.uniform(-0.3, 0.3, n)]
    if kind == "pure_rotation":
        return matches_of_motion(P, _rot(1, 0.05) @ _rot(0, -0.03), np.zeros(3))
    if kind == "identity":
        return matches_of_motion(P, np.eye(3), np.zeros(3))
    if kind == "collinear":
        s = rng.uniform(-1, 1, n)
        P = np.c_[s, 0.5 * s + 0.1, np.full(n, 2.0)]
        return matches_of_motion(P, _rot(1, 0.02), np.array([0.2, 0.0, 0.0]))
    if kind == "identical":
        return np.tile(matches_of_motion(P[:1], _rot(1, 0.02), np.array([0.2, 0.0, 0.0])), (n, 1))
    raise KeyError(kind)


def pixel_scene(seed, n, cam5, w, h, outliers=8):
    """integer pixel pairs (n, 4) of a tilted plane seen by the ATAN camera cam5 (normalised parameters) before and after a sideways move"""
    rng = np.random.default_rng(seed)
    P = np.c_[rng.uniform(-0.9, 0.9, n), rng.uniform(-0.6, 0.6, n), np.zeros(n)]
    P[:, 2] = 2.0 + 0.15 * P[:, 0] - 0.1 * P[:, 1]
    Q = (_rot(1, 0.04) @ _rot(0, -0.02) @ P.T).T + np.array([0.15, 0.01, -0.01])

    def project(X):
        out = np.zeros((len(X), 2))
        for i, x in enumerate(X):
            out[i] = orc.cam_project(cam5, w, h, x[0] / x[2], x[1] / x[2])[0]
        return out
    a, b = project(P), project(Q)
    b[:outliers] += rng.uniform(-30, 30, (outliers, 2))
    px = np.rint(np.c_[a, b]).astype(np.int32)
    keep = (px[:, 0::2] >= 0).all(1) & (px[:, 0::2] < w).all(1) & (px[:, 1::2] >= 0).all(1) & (px[:, 1::2] < h).all(1)
    return px[keep]


def plane_cloud(n, clutter=0.05, seed=1):
    """the scene of test_plane_aligner_puts_the_dominant_plane_at_z_zero: a thin slab, a share of clutter off it, rotated and moved"""
    rng = np.random.default_rng(seed)
    pts = np.c_[rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.normal(0, 0.002, n)]
    k = int(round(n * clutter))
    pts[:k, 2] += rng.uniform(0.2, 0.6, k)
    Rw, tw = _rot(0, 0.4) @ _rot(1, -0.3), np.array([0.3, -0.2, 1.5])
    return (Rw @ pts.T).T + tw


# ---- comparisons ---------------------------------------------------------------------------------------------------------------
def normalised_h(H):
    """sign and scale of a homography are free: unit Frobenius norm, the element of largest magnitude positive"""
    H = np.asarray(H, float).reshape(-1)
    nrm = np.linalg.norm(H)
    if not nrm > 0:
        return H
    H = H / nrm
    return H if H[np.argmax(np.abs(H))] > 0 else -H


def ulp_draws(a, draws=3, seed=0):
    """the array a with every double moved by +1 or -1 ulp, in `draws` seeded draws"""
    a = np.asarray(a, float)
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(draws):
        up = rng.integers(0, 2, a.shape).astype(bool)
        out.append(np.where(up, np.nextafter(a, np.inf), np.nextafter(a, -np.inf)))
    return out


def _spread(vals):
    v = np.array(vals, float)
    return float((v.max(0) - v.min(0)).max()) if v.size else 0.0


def bar_of(spread):
    return max(BAR_FACTOR * spread, BAR_FLOOR)


def oracle_homography(m8, seed, max_err=5.0):
    """the oracle's stages on m8, and the spread of each of its outputs over the input and three +-1 ulp draws of it"""
    base = orc.homography_init_stages(m8, max_err, seed)
    runs = [base] + [orc.homography_init_stages(d, max_err, seed) for d in ulp_draws(m8)]
    spread = {"pose": _spread([r["pose"] for r in runs]),
              "H_mlesac": _spread([normalised_h(r["H_mlesac"]) for r in runs]),
              "H_refined": _spread([normalised_h(r["H_refined"]) for r in runs])}
    return base, spread


def oracle_plane(pos, seed):
    base = orc.calc_plane_aligner_stages(pos, seed)
    runs = [base] + [orc.calc_plane_aligner_stages(d, seed) for d in ulp_draws(pos)]
    spread = {k: _spread([r[k] for r in runs]) for k in ("aligner", "mean", "normal")}
    return base, spread


def arr(x):
    return np.array(x[:])


def check_homography_against_oracle(rec, m8, seed, tag, report=None):
    """a stage record (host build or device) against the oracle's stages: ok, the inlier list and the branch exactly; homographies
    (normalised) and the pose within 16 x the oracle's own +-1 ulp spread, not below 1e-13.  Returns the differences and spreads."""
    o, spread = oracle_homography(m8, seed)
    diff = {"H_mlesac": float(np.abs(normalised_h(rec.H_mlesac) - normalised_h(o["H_mlesac"])).max()),
            "H_refined": float(np.abs(normalised_h(rec.H_refined) - normalised_h(o["H_refined"])).max()),
            "pose": float(np.abs(np.r_[arr(rec.R), arr(rec.t)] - o["pose"]).max()) if o["ok"] else 0.0}
    if report is not None:
        report.append((tag, diff, spread))
    assert bool(rec.ok) == o["ok"], (tag, rec.ok, o["ok"])
    assert np.array_equal(arr(rec.inliers)[:rec.n_inliers], o["inliers"]), tag
    for k in ("H_mlesac", "H_refined", "pose"):
        assert diff[k] <= bar_of(spread[k]), (tag, k, diff[k], spread[k])
    if o["ok"]:
        assert rec.choice == o["choice"], (tag, rec.choice, o["choice"])
    return diff, spread


def check_plane_against_oracle(rec, pos, seed, tag, report=None):
    o, spread = oracle_plane(pos, seed)
    diff = {"mean": float(np.abs(arr(rec.mean) - o["mean"]).max()), "normal": float(np.abs(arr(rec.normal) - o["normal"]).max()),
            "aligner": float(np.abs(np.r_[arr(rec.R), arr(rec.t)] - o["aligner"]).max()) if o["ok"] else 0.0}
    if report is not None:
        report.append((tag, diff, spread))
    assert bool(rec.have) == o["ok"], tag
    for k in ("mean", "normal", "aligner") if rec.n >= 10 else ():          # with fewer than ten points the stage is not reached (:1107-1110)
        assert diff[k] <= bar_of(spread[k]), (tag, k, diff[k], spread[k])
    return diff, spread


def _fields_equal(a, b):
    """every field of two ctypes records: integers exactly; doubles bit for bit (so -0.0 is not 0.0), except that a NaN equals a NaN --
    the sign and payload of a generated NaN are the platform's, not IEEE 754's"""
    bad = []
    for name, ctype in a._fields_:
        x, y = getattr(a, name), getattr(b, name)
        if isinstance(x, C.Array):
            x, y = np.array(x[:]), np.array(y[:])
        else:
            x, y = np.array([x]), np.array([y])
        if x.dtype.kind == "f":
            same = (x.view(np.uint64) == y.view(np.uint64)) | (np.isnan(x) & np.isnan(y))
        else:
            same = x == y
        if not same.all():
            i = int(np.argmin(same))
            bad.append("%s[%d]: %r != %r (%d of %d differ)" % (name, i, x[i], y[i], int((~same).sum()), same.size))
    return bad


def assert_same_bits(dev, host, tag):
    bad = _fields_equal(dev, host)
    assert not bad, (tag, bad)


def first_argmin(scores):
    """the first strict minimum of the 300 scores in trial order, as BestHomographyFromMatches_MLESAC keeps it (-1: no score below its start value)"""
    best, bt = 999999999999999999.9, -1
    for t, e in enumerate(scores):
        if e < best:
            best, bt = e, t
    return bt
