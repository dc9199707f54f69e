"""Hand-built maps for the map-maker's driver kernels (csrc/ba.hip: k_ba_select, k_ba_assemble, k_ba_writeback with handle_bad_points),
shared by tests/test_mapmaker_cases.py (CPU: the oracle alone reaches what every case is named for) and tests/test_gpu_mapmaker_edges.py
(GPU: the device == the oracle on every case).  No GPU is touched here.

The sequence tests put these kernels on feeder-rendered scenes, which never stand where the kernels branch.  The maps here are numpy
only: cameras with chosen centres look along +z at a slab of points, a measurement is the camera model's projection of the true point
(project(), checked against the oracle's camera by the CPU test) plus seeded noise of PIXEL_NOISE pixels of its level, levels 0..3 by
turns, and the stored points (and, unless a case needs exact distances, the stored poses of the keyframes that are not fixed) are
perturbed so that an adjustment accepts steps.  The kernels never read pixels: every keyframe image is constant grey at 64 x 48.  A
gross corruption moves a measurement by CORRUPT_PX pixels at level 0, which the bundle's Tukey weight rejects in its first step: the
outlier list is known in advance.

A Case is a map, the system's capacities (close to the map's counts), a list of jobs ("recent", "all", ("idle", job number)), point
flags that no upload can set (bad, n_in, n_out: the oracle takes them through set_point_flags, the device through a patched snapshot),
and `want`: what the case is named for, derived from its construction and asserted on the oracle's last problem by the CPU test.
idle_iterations = -1 keeps the failure queue and the never-retry sets without running an idle pass after a frame.

Not reached by any case: a failure queue beyond its 8192 entries, and the asynchronous map-maker (ba_delay_frames > 0)."""
import functools

import numpy as np

from visualslam_android_amd import capi
from visualslam_android_amd.ba_scene import CAM

W, H = 64, 48
BA_THREADS = 256                 # chunk of k_ba_assemble's compactions
LDS_OUTLIERS = 2048              # k_ba_writeback keeps the outliers' point ids in LDS up to here
MAX_MEAS = 65536                 # the pool's cap on a problem's measurements (ba_alloc)
SRC_TRACKER, SRC_REFIND, SRC_ROOT, SRC_TRAIL, SRC_EPIPOLAR = range(5)
RETRY_SOURCES = (SRC_TRACKER, SRC_EPIPOLAR)          # an outlier of these goes to the failure queue, of any other to the never-retry set
CORRUPT_PX = 60.0
PIXEL_NOISE, POINT_NOISE, POSE_NOISE = 0.25, 0.005, (0.003, 0.001)     # the perturbations stay below the noise: the residuals are alike at every level
GREY = np.full((H, W), 128, np.uint8)


def project(pose12, X):
    """the camera model (jni/ATANCamera) of the default calibration at W x H, vectorised: pose12 camera-from-world, X [n, 3] -> [n, 2]"""
    R, t = np.asarray(pose12[:9]).reshape(3, 3), np.asarray(pose12[9:])
    c = X @ R.T + t
    x, y = c[:, 0] / c[:, 2], c[:, 1] / c[:, 2]
    r = np.hypot(x, y)
    rs = np.where(r < 0.001, 1.0, r)
    fac = np.where(r < 0.001, 1.0, np.arctan(rs * 2 * np.tan(CAM[4] / 2)) / CAM[4] / rs)
    return np.stack([W * CAM[2] - 0.5 + W * CAM[0] * x * fac, H * CAM[3] - 0.5 + H * CAM[1] * y * fac], 1)


def _rot(w):
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.eye(3) + K if th < 1e-12 else np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K


def make_map(centres, vis, seed, fixed=(0,), exact_poses=False, corrupt=(), sources=None, behind=False, pose_noise=POSE_NOISE):
    """centres [nk, 3]: camera centres (identity rotation with exact_poses: the stored pose is then (I, -centre) exactly, and a dyadic
    centre makes KeyFrameLinearDist exact).  vis [nk, npts] bool: keyframe k measures point i.  corrupt: (kf, pt) measurements moved by
    CORRUPT_PX at level 0.  sources: {(kf, pt): source}, SRC_TRACKER otherwise.  behind: the slab lies behind the cameras.  pose_noise:
    (translation, rotation) perturbation of the stored poses."""
    rng = np.random.default_rng(seed)
    centres = np.asarray(centres, np.float64)
    vis = np.asarray(vis, bool)
    nk, npts = vis.shape
    X = np.stack([rng.uniform(-0.5, 0.5, npts), rng.uniform(-0.35, 0.35, npts), rng.uniform(3.5, 4.5, npts) * (-1 if behind else 1)], 1)
    corrupt, sources = set(corrupt), dict(sources or {})
    kfs, meas = [], []
    for k in range(nk):
        R = np.eye(3) if exact_poses else _rot(rng.normal(0, 0.02, 3))
        true = np.concatenate([R.ravel(), -R @ centres[k]])
        stored = true
        if not exact_poses and k not in fixed:
            dR = _rot(rng.normal(0, pose_noise[1], 3))
            stored = np.concatenate([(dR @ R).ravel(), dR @ true[9:] + rng.normal(0, pose_noise[0], 3)])
        kfs.append({"pose": stored, "fixed": k in fixed, "image": GREY, "depth_mean": 4.0, "depth_sigma": 0.3})
        idx = np.flatnonzero(vis[k])
        uv = project(true, X[idx]) + rng.normal(0, PIXEL_NOISE, (len(idx), 2)) * (1 << ((idx + k) % 4))[:, None]   # a level's pixel is its unit
        for j, i in enumerate(idx):
            level = int((i + k) % 4)
            u, v = uv[j]
            if (k, int(i)) in corrupt:
                level, u, v = 0, u + CORRUPT_PX, v - CORRUPT_PX
            meas.append((k, int(i), level, float(u), float(v), 0, sources.get((k, int(i)), SRC_TRACKER)))
    Xs = X + rng.normal(0, POINT_NOISE, X.shape)
    points = [{"pos": Xs[i], "src_kf": 0, "level": 0, "irx": 20, "iry": 20, "right": (0.02, 0.0, 0.0), "down": (0.0, 0.02, 0.0)} for i in range(npts)]
    return {"keyframes": kfs, "points": points, "meas": meas}


# ---- a plain model of what BundleAdjustRecent / BundleAdjustAll take from a map (jni/MapMaker.cc:776-902), from the construction -----------------
def problem_of(vis, fixed, adjusted=None, bad=()):
    """-> the fixed set, the point set and the measurement count of the problem.  adjusted: the window of a BundleAdjustRecent (its point
    set is what the window measures, its fixed set every other keyframe that measures one of them); None: BundleAdjustAll (every point
    that is not bad, every keyframe)."""
    vis = np.asarray(vis, bool)
    nk, npts = vis.shape
    if adjusted is None:
        adjusted = [k for k in range(nk) if k not in fixed]
        pset = np.array([i not in bad for i in range(npts)])
        fx = [k for k in range(nk) if k in fixed]
    else:
        pset = vis[list(adjusted)].any(0)
        fx = [k for k in range(nk) if k not in adjusted and (vis[k] & pset).any()]
    cams = sorted(adjusted) + fx
    return {"adjusted": sorted(adjusted), "fixed": fx, "points": np.flatnonzero(pset), "n_meas": int(vis[cams][:, pset].sum()) if cams else 0}


class Case:
    """jobs run in order on one loaded map.  flags: {point: (bad, n_in, n_out)} set after the load.  want: what the LAST job's problem must be
    (keys of problem_of plus "n_meas_over", "ret", "n_outliers", "outliers" (set of (kf, pt)), "bad_mid_walk", "never_retry_high" (set of (pt, kf >= 64)),
    "ran": False where the last job builds no problem).  device_refuses: the device answers the last job with ba_accepted = -3 and
    leaves the map alone, where the oracle has no limit; `then` is a job that fits and runs after it.  fast: also run with ba_sum_order = 0."""

    def __init__(self, name, group, build, jobs, pkw, want=None, flags=None, fast=False, device_refuses=False, then=None, then_want=None):
        self.name, self.group, self._build, self.jobs, self.pkw = name, group, build, tuple(jobs), dict(pkw)
        self.want, self.flags, self.fast, self.device_refuses, self.then, self.then_want = dict(want or {}), dict(flags or {}), fast, device_refuses, then, then_want
        self._map = None

    def __repr__(self):
        return self.name

    def map(self):
        if self._map is None and self._build is not None:
            self._map = self._build()
        return self._map

    def params(self, n_streams=1, **kw):
        return capi.default_params(W, H, n_streams, **{**BASE, **self.pkw, **kw})


BASE = dict(idle_iterations=-1, ba_sum_order=1, ba_max_iterations=3, ba_window=3, ba_min_keyframes=3)


def _caps(nk, npts, **kw):
    return dict(max_keyframes=max(nk, 2), max_points=max(npts, 16), **kw)


def _line(xs):
    return np.stack([np.asarray(xs, np.float64), np.zeros(len(xs)), np.zeros(len(xs))], 1)


def _case(name, group, centres, vis, seed, jobs, want, fixed=(0,), exact_poses=False, corrupt=(), sources=None, behind=False, pose_noise=POSE_NOISE, **kw):
    pkw = kw.pop("pkw", {})
    vis = np.asarray(vis, bool)
    return Case(name, group, lambda: make_map(centres, vis, seed, fixed, exact_poses, corrupt, sources, behind, pose_noise), jobs,
                {**_caps(*vis.shape), **pkw}, want, **kw)


# ---- select, Recent --------------------------------------------------------------------------------------------------------------------
def _full(nk, npts):
    return np.ones((nk, npts), bool)


def _recent_want(vis, fixed, adjusted, **kw):
    return {**problem_of(vis, fixed, adjusted), **kw}


def _wide_line(nk, near):
    """nk keyframes on the x axis, the newest at 0; near: {keyframe: dyadic distance}, every other keyframe far away at 0.5 + k / 256"""
    xs = [0.5 + k / 256.0 for k in range(nk)]
    for k, d in near.items():
        xs[k] = d
    xs[nk - 1] = 0.0
    return _line(xs)


@functools.lru_cache(maxsize=None)
def select_recent():
    out = []
    v = _full(3, 24)
    out.append(_case("nk = ba_min_keyframes - 1", "select", _line([0.5, 0.25, 0]), v, 1, ["recent"], {"ran": False, "ret": -2}, pkw=dict(ba_min_keyframes=4), fast=True))
    v = _full(4, 24)      # window 5: four places for three other keyframes
    out.append(_case("nk = ba_min_keyframes, ba_window - 1 > nk - 1", "select", _line([0.75, 0.5, 0.25, 0]), v, 2, ["recent"],
                     _recent_want(v, (0,), [1, 2, 3]), pkw=dict(ba_min_keyframes=4, ba_window=5), fast=True))
    v = _full(6, 24)      # the last place: keyframes 1 and 3 at exactly 0.5 on either side -> the lower index
    out.append(_case("two keyframes tie for the last place", "select", _line([1.0, 0.5, 0.25, -0.5, -1.0, 0]), v, 3, ["recent"],
                     _recent_want(v, (0,), [1, 2, 5], tie=(5, (1, 3))), exact_poses=True, fast=True))
    v = _full(7, 24)      # ... keyframes 1, 2, 3 at exactly 0.5 along y, x and -x
    c = np.array([[2.0, 0, 0], [0, 0.5, 0], [0.5, 0, 0], [-0.5, 0, 0], [0.25, 0, 0], [-2.0, 0, 0], [0, 0, 0]])
    out.append(_case("three keyframes tie for the last place", "select", c, v, 4, ["recent"],
                     _recent_want(v, (0,), [1, 4, 6], tie=(6, (1, 2, 3))), exact_poses=True, fast=True))
    v = _full(6, 24)      # the nearest (2) is fixed: it takes a place of the window and joins as a fixed camera
    out.append(_case("the nearest keyframe is fixed", "select", _line([1.0, 0.75, 0.125, 0.5, 0.25, 0]), v, 5, ["recent"],
                     _recent_want(v, (0, 2), [4, 5]), fixed=(0, 2), fast=True))
    v = _full(5, 24)
    out.append(_case("every keyframe but the newest is fixed", "select", _line([1.0, 0.75, 0.5, 0.25, 0]), v, 6, ["recent"],
                     _recent_want(v, (0, 1, 2, 3), [4]), fixed=(0, 1, 2, 3), fast=True))
    # the two words of the chosen / taken sets: window 7, the six nearest on both sides of keyframes 63 | 64
    w7 = dict(ba_window=7, ba_max_iterations=2)
    v = _full(64, 20)
    out.append(_case("nk = 64, the newest is keyframe 63", "select", _wide_line(64, {0: 0.0625, 31: 0.125, 32: 0.1875, 61: 0.25, 62: 0.03125, 1: 0.3125}), v, 7,
                     ["recent"], _recent_want(v, (0,), [1, 31, 32, 61, 62, 63]), pkw=w7, fast=True))     # keyframe 0 is fixed: five adjusted beside the newest
    v = _full(65, 20)
    out.append(_case("nk = 65, the newest is keyframe 64", "select", _wide_line(65, {2: 0.0625, 62: 0.125, 63: 0.1875, 33: 0.25, 1: 0.03125, 61: 0.3125}), v, 8,
                     ["recent"], _recent_want(v, (0,), [1, 2, 33, 61, 62, 63, 64]), pkw=w7, fast=True))
    v = _full(128, 20)
    out.append(_case("nk = 128, the newest is keyframe 127", "select", _wide_line(128, {63: 0.0625, 64: 0.125, 65: 0.1875, 62: 0.25, 126: 0.03125, 1: 0.3125}), v, 9,
                     ["recent"], _recent_want(v, (0,), [1, 62, 63, 64, 65, 126, 127]), pkw=w7, fast=True))
    return out


# ---- select, All -----------------------------------------------------------------------------------------------------------------------
def _fan(nk):
    return np.stack([np.cos(np.arange(nk) * 0.7) * 0.4, np.sin(np.arange(nk) * 0.7) * 0.3, np.arange(nk) * 0.004], 1)


@functools.lru_cache(maxsize=None)
def select_all():
    out = []
    it = dict(ba_max_iterations=2)
    v = _full(65, 24)
    out.append(_case("64 adjustable + 1 fixed", "select", _fan(65), v, 11, ["all"], {**problem_of(v, (0,))}, pkw=it, fast=True))
    v = _full(66, 24)
    out.append(_case("65 adjustable + 1 fixed", "select", _fan(66), v, 12, ["all"], {**problem_of(v, (0,))}, pkw=it, fast=True, device_refuses=True,
                     then="recent", then_want=_recent_want(v, (0,), _nearest(_fan(66), 65, 2))))
    v = _full(3, 24)
    out.append(_case("no adjustable keyframe", "select", _fan(3), v, 13, ["all"], {**problem_of(v, (0, 1, 2))}, fixed=(0, 1, 2), fast=True))
    return out


def _nearest(centres, newest, n, fixed=(0,)):
    """the window of BundleAdjustRecent by plain sorting of (distance, index)"""
    d = sorted((float(np.linalg.norm(centres[k] - centres[newest])), k) for k in range(len(centres)) if k != newest)
    return sorted([newest] + [k for _d, k in d[:n] if k not in fixed])


# ---- assemble --------------------------------------------------------------------------------------------------------------------------
def _assemble_vis(npts, seed, only=None):
    """five keyframes, window {2, 3, 4}: the window measures the points of a seeded mask (or `only`), keyframes 3 and 4 all of them and keyframe 2
    a seeded half; keyframe 0 (fixed) measures a seeded 70 % of all points, keyframe 1 a seeded half of all points"""
    rng = np.random.default_rng(1000 + seed)
    mask = rng.uniform(size=npts) < 0.5
    if only is not None:
        mask[:] = False
        mask[list(only)] = True
    mask[npts - 1] = True if only is None else mask[npts - 1]
    vis = np.zeros((5, npts), bool)
    vis[3] = vis[4] = mask
    vis[2] = mask & (rng.uniform(size=npts) < 0.5)
    vis[0] = rng.uniform(size=npts) < 0.7
    vis[1] = rng.uniform(size=npts) < 0.5
    if only is not None:                       # a handful of points: every keyframe measures them, so that the problem stays well posed
        vis[:3, list(only)] = True
    return vis


ASSEMBLE_CENTRES = np.array([[1.25, 0, 0], [-1.0, 0, 0], [-0.5, 0.2, 0], [0.5, -0.2, 0], [0, 0, 0]])     # the window of keyframe 4 is {2, 3, 4}


@functools.lru_cache(maxsize=None)
def assemble():
    out = []
    for n in (BA_THREADS - 1, BA_THREADS, BA_THREADS + 1, 2 * BA_THREADS + 1):
        v = _assemble_vis(n, n)
        out.append(_case("n_points = %d, half in the set" % n, "assemble", ASSEMBLE_CENTRES, v, 20 + n, ["recent"], _recent_want(v, (0,), [2, 3, 4]), fast=True))
    only = (63, 64, BA_THREADS - 1, BA_THREADS)
    v = _assemble_vis(300, 5, only=only)
    want = _recent_want(v, (0,), [3, 4])                    # window 2: four points carry two free cameras, not three
    assert want["points"].tolist() == list(only)
    out.append(_case("the set is points 63, 64, 255, 256", "assemble", _line([1.25, -1.0, 0.75, 0.5, 0]), v, 31, ["recent"], want, pkw=dict(ba_window=2), fast=True))
    # the fixed set: keyframe 1 shares exactly the last map point with the window, keyframe 2 measures only points outside the set
    n = 2 * BA_THREADS + 1
    v = np.zeros((6, n), bool)
    rng = np.random.default_rng(32)
    mask = rng.uniform(size=n) < 0.5
    mask[n - 1] = True
    v[3] = v[4] = v[5] = mask
    v[0] = True
    v[1] = ~mask
    v[1, n - 1] = True
    v[2] = ~mask
    want = _recent_want(v, (0,), [3, 4, 5])
    assert want["fixed"] == [0, 1] and int((v[1] & mask).sum()) == 1
    out.append(_case("a fixed-set keyframe through the last point, one that must not join", "assemble",
                     np.array([[1.25, 0, 0], [-1.0, 0, 0], [1.0, 0.3, 0], [-0.5, 0.2, 0], [0.5, -0.2, 0], [0, 0, 0]]), v, 32, ["recent"],
                     want, fast=True))
    # a bad point that still has its measurements: the window's point set takes it, BundleAdjustAll's does not
    v = _full(5, 40)
    flags = {7: (1, 0, 0), 39: (1, 0, 0)}
    recent, every = _recent_want(v, (0,), [2, 3, 4]), problem_of(v, (0,), bad=(7, 39))
    assert len(recent["points"]) == 40 and len(every["points"]) == 38 and not {7, 39} & set(every["points"].tolist())
    out.append(_case("a bad point with measurements, Recent", "assemble", ASSEMBLE_CENTRES, v, 33, ["recent"], recent, flags=flags, fast=True))
    out.append(_case("a bad point with measurements, All", "assemble", ASSEMBLE_CENTRES, v, 33, ["all"], every, flags=flags, fast=True))
    return out


# ---- capacity --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def capacity():
    out = []
    # exactly the cap: 32 x 2048 measurements in a system of 32 x 2100 slots, so that the pool's cap is the truncated one here too
    v = _full(32, MAX_MEAS // 32)
    want = problem_of(v, (0,))
    assert want["n_meas"] == MAX_MEAS and 32 * 2100 > MAX_MEAS
    out.append(_case("BundleAdjustAll with exactly %d measurements" % MAX_MEAS, "capacity", _fan(32), v, 41, ["all"], want, pkw=dict(ba_max_iterations=1, max_points=2100)))
    # more: keyframes 0..26 measure 2440 points (65880); the five newest, the window of the BundleAdjustRecent that follows the refusal, measure
    # 60 points of their own, and so does the fixed keyframe 0
    n_main, n_own = 2440, 60
    v = np.zeros((32, n_main + n_own), bool)
    v[:27, :n_main] = True
    v[27:, n_main:] = True
    v[0, n_main:] = True
    c = _fan(32)
    c[27:] = _line([0.125, 0.0625, 0.03125, 0.015625, 0]) + np.array([0, 0, 0.25])
    out.append(_case("BundleAdjustAll with more than %d measurements" % MAX_MEAS, "capacity", c, v, 42, ["all"], {**problem_of(v, (0,)), "n_meas_over": MAX_MEAS},
                     pkw=dict(ba_max_iterations=1, ba_window=5), device_refuses=True, then="recent", then_want=_recent_want(v, (0,), [27, 28, 29, 30, 31])))
    return out


# ---- write-back ------------------------------------------------------------------------------------------------------------------------
def _pick(vis, n, seed, first_kf=1):
    """n (kf, pt) measurements of a seeded permutation of the map's, none in a keyframe below first_kf; the first n of a longer pick are the same"""
    rng = np.random.default_rng(seed)
    k, i = np.nonzero(np.asarray(vis)[first_kf:])
    order = rng.permutation(len(k))
    return [(int(k[j]) + first_kf, int(i[j])) for j in order[:n]]


def _walk_map():
    """eight keyframes, 40 points, BundleAdjustAll.  The points with outliers (n_meas_kfs -> the walk):
      0  seen by 4, outliers in 2          4 -> 3 -> 2: both erased, not bad
      1  seen by 4, outliers in 3          4 -> 3 -> 2, the third entry finds 2: bad part-way, its measurement stays
      2  seen by 5, outliers in 4          5 -> 4 -> 3 -> 2, the fourth entry: bad part-way
      3  seen by 4, outliers in all 4      the third and the fourth entry find 2: bad part-way, two measurements stay
      4  seen by 2, outlier in 1           bad at once
      5  seen by 8, one SRC_ROOT outlier   bad at once, nothing erased
      6..10  seen by 8, one outlier of source 0..4 in keyframe 2..6: queue, never-retry, bad (SRC_ROOT), never-retry, queue
    Three of the outliers of points 1 and 2 are re-find / trail / epipolar measurements, the rest the tracker's.
    """
    nk, npts = 8, 40
    vis = _full(nk, npts)
    seen = {0: (1, 3, 5, 7), 1: (1, 2, 4, 6), 2: (2, 3, 4, 5, 7), 3: (1, 3, 5, 6), 4: (2, 6)}
    for p, ks in seen.items():
        vis[:, p] = False
        vis[list(ks), p] = True
    out = {0: (1, 5), 1: (1, 2, 4), 2: (2, 3, 4, 5), 3: (1, 3, 5, 6), 4: (6,), 5: (3,)}
    corrupt = [(k, p) for p, ks in out.items() for k in ks]
    sources = {(3, 5): SRC_ROOT}
    for s in range(5):
        corrupt.append((2 + s, 6 + s))
        sources[(2 + s, 6 + s)] = s
    sources[(2, 1)] = SRC_REFIND
    sources[(3, 2)] = SRC_TRAIL
    sources[(5, 2)] = SRC_EPIPOLAR
    return vis, corrupt, sources


def apply_outliers(vis, outliers, sources):
    """the reference's walk (jni/MapMaker.cc:941-959) over an outlier list [(kf, pt)] in order, on the construction alone ->
    {"bad": set, "erased": set of (kf, pt), "queue": sorted list, "never": set of (pt, kf), "bad_mid_walk": int}"""
    nkfs = np.asarray(vis).sum(0).astype(int)
    bad, erased, queue, never, mid = set(), set(), [], set(), 0
    for k, p in outliers:
        src = sources.get((k, p), SRC_TRACKER)
        if nkfs[p] <= 2 or src == SRC_ROOT:
            if p not in bad and any(q == p for _k, q in erased):
                mid += 1
            bad.add(p)
            continue
        (queue.append((k, p)) if src in RETRY_SOURCES else never.add((p, k)))
        erased.add((k, p))
        nkfs[p] -= 1
    return {"bad": bad, "erased": erased, "queue": sorted(queue), "never": never, "bad_mid_walk": mid}


def _kf_major(pairs):
    return sorted(pairs)


@functools.lru_cache(maxsize=None)
def writeback():
    out = []
    c8 = _fan(8)
    v = _full(8, 40)
    out.append(_case("no outlier", "write-back", c8, v, 50, ["all", "all"], {**problem_of(v, (0,)), "outliers": set()}))
    one = [(4, 17)]
    out.append(_case("one outlier", "write-back", c8, v, 51, ["all"], {**problem_of(v, (0,)), "outliers": set(one), "walk": apply_outliers(v, one, {})}, corrupt=one))
    vw, corrupt, sources = _walk_map()
    out.append(_case("points with 2, 3 and 4 outliers, a SRC_ROOT outlier, every source", "write-back", c8, vw, 52, ["all", "recent"],
                     {"outliers_first_job": set(corrupt), "walk": apply_outliers(vw, _kf_major(corrupt), sources), "bad_mid_walk": 3}, corrupt=corrupt, sources=sources))
    # either side of the LDS copy of the list: 12 keyframes x 600 points, a seeded pick of the measurements, sources by turns tracker / re-find
    v = _full(12, 600)
    for n in (LDS_OUTLIERS, LDS_OUTLIERS + 1):
        pick = _pick(v, n, 53)
        src = {kp: (SRC_TRACKER, SRC_REFIND, SRC_EPIPOLAR, SRC_TRAIL)[j % 4] for j, kp in enumerate(pick)}
        out.append(_case("%d outliers" % n, "write-back", _fan(12), v, 53, ["all"],
                         {**problem_of(v, (0,)), "outliers": set(pick), "n_outliers": n, "walk": apply_outliers(v, _kf_major(pick), src)}, corrupt=pick, sources=src))
    # never-retry bits of keyframes 63, 64 and 127: re-find / trail outliers there, in a window of the 128-keyframe map
    v = _full(128, 20)
    pick = [(63, 3), (64, 4), (127, 5), (64, 3), (1, 6)]
    src = {(63, 3): SRC_REFIND, (64, 4): SRC_TRAIL, (127, 5): SRC_REFIND, (64, 3): SRC_REFIND, (1, 6): SRC_EPIPOLAR}
    out.append(_case("never-retry bits of keyframes 63, 64 and 127", "write-back",
                     _wide_line(128, {63: 0.0625, 64: 0.125, 65: 0.1875, 62: 0.25, 126: 0.03125, 1: 0.3125}), v, 54, ["recent"],
                     {**_recent_want(v, (0,), [1, 62, 63, 64, 65, 126, 127]), "outliers": set(pick), "walk": apply_outliers(v, _kf_major(pick), src),
                      "never_retry_high": {(3, 64), (4, 64), (5, 127)}}, corrupt=pick, sources=src, pkw=dict(ba_window=7, ba_max_iterations=2)))
    # results that are not accepted steps
    v = _full(5, 24)
    out.append(_case("every point behind the cameras (Compute fails)", "write-back", ASSEMBLE_CENTRES, v, 55, ["recent", "all"], {"ret": -1}, behind=True))
    out.append(_case("one trial, not accepted", "write-back", ASSEMBLE_CENTRES, v, 90, ["recent", "all"], {"ret_first": 0}, pose_noise=(0.1, 0.1),
                     pkw=dict(ba_max_iterations=1)))
    return out


# ---- bad points ------------------------------------------------------------------------------------------------------------------------
BAD_FLAGS = {3: (0, 5, 20), 4: (0, 5, 21), 5: (0, 21, 21), 6: (0, 30, 21), 7: (0, 20, 20), 8: (0, 0, 255), 9: (0, 30, 20), 39: (0, 20, 21)}   # point: (bad, n_in, n_out)
BAD_EXPECTED = {4, 8, 39}                  # n_out > 20 and n_out > n_in


@functools.lru_cache(maxsize=None)
def bad_points():
    v = _full(5, 40)
    out = []
    for name, jobs in (("Recent", ["recent"]), ("All", ["all"]), ("idle job 0 (no adjustment is due)", [("idle", 0)]), ("idle job 2 (no adjustment is due)", [("idle", 2)])):
        out.append(_case("n_out 20 | 21 against n_in, through " + name, "bad points", ASSEMBLE_CENTRES, v, 60, jobs, {"bad": BAD_EXPECTED}, flags=BAD_FLAGS))
    # the idle jobs with an adjustment due: a Recent that stops after one step leaves both flags down -> idle job 0 runs a Recent
    out.append(_case("idle job 0 runs BundleAdjustRecent", "bad points", ASSEMBLE_CENTRES, v, 61, ["recent", ("idle", 0), ("idle", 2), ("idle", 0)],
                     {"bad": BAD_EXPECTED, "idle": {"ba_recent_idle": 2, "ba_all": 0}}, flags=BAD_FLAGS, pkw=dict(ba_max_iterations=1)))
    # ... one that converges leaves the full flag down alone -> idle job 2 runs a BundleAdjustAll
    out.append(_case("idle job 2 runs BundleAdjustAll", "bad points", ASSEMBLE_CENTRES, v, 62, ["recent", ("idle", 0), ("idle", 2)],
                     {"bad": BAD_EXPECTED, "idle": {"ba_recent_idle": 0, "ba_all": 1}}, flags=BAD_FLAGS, pkw=dict(ba_max_iterations=40)))
    return out


# ---- batch -----------------------------------------------------------------------------------------------------------------------------
BATCH_STREAMS = 65                         # one past k_ba_select's block of 64 lanes
BATCH_JOBS = ("recent", "all", "recent")
BATCH_PKW = dict(max_keyframes=66, max_points=48, ba_max_iterations=2, ba_min_keyframes=4)


@functools.lru_cache(maxsize=None)
def batch_templates():
    """the maps of the batch, by turns: below the minimum, refused (65 adjustable keyframes), a tied window, outliers, no map at all"""
    v = _full(6, 40)
    vw, corrupt, sources = _walk_map()
    t = [_case("batch: below the minimum", "batch", _line([0.5, 0.25, 0]), _full(3, 24), 70, BATCH_JOBS, {}),
         _case("batch: 65 adjustable keyframes", "batch", _fan(66), _full(66, 24), 71, BATCH_JOBS, {}),
         _case("batch: tied window", "batch", _line([1.0, 0.5, 0.25, -0.5, -1.0, 0]), v, 72, BATCH_JOBS, {}, exact_poses=True),
         _case("batch: outliers", "batch", _fan(8), vw, 73, BATCH_JOBS, {}, corrupt=corrupt, sources=sources),
         Case("batch: no map", "batch", None, BATCH_JOBS, {})]
    for c in t:
        c.pkw = dict(BATCH_PKW)
    return t


BATCH_ORACLE_TEMPLATES = (0, 2, 3)         # the templates whose first stream is also checked against the oracle (the refused one has no oracle)


def batch_template_of(stream):
    """by turns, starting so that stream 64 -- the one lane of k_ba_select's second block -- carries the outlier map"""
    return (stream + 4) % 5


GROUPS = ("select", "assemble", "capacity", "write-back", "bad points")


@functools.lru_cache(maxsize=None)
def cases():
    return select_recent() + select_all() + assemble() + capacity() + writeback() + bad_points()


def by_group(group):
    return [c for c in cases() if c.group == group]


# ---- running a case on the oracle ------------------------------------------------------------------------------------------------------
def run_job(x, job, stream=None):
    """one job on the oracle (stream is None) or on the device; -> the oracle's return value where it has one"""
    if job == "recent":
        return x.bundle_adjust_recent()
    if job == "all":
        return x.bundle_adjust_all()
    return x.idle_job(job[1]) if stream is None else x.mapmaker_idle_job(job[1])


def oracle_for(case, **pkw):
    from oracle import binding as orc
    o = orc.OracleSystem(orc.params_from_vslam(case.params(**pkw)))
    if case.map() is not None:
        o.load_map(case.map())
        for pt, (bad, n_in, n_out) in case.flags.items():
            o.set_point_flags(pt, bad, n_in, n_out)
    return o
