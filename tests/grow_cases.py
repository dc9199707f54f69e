"""Map-growth cases with chosen counts, shared by tests/test_grow_cases.py (CPU: the oracle alone reaches every condition) and
tests/test_gpu_grow_counts.py (GPU: the device == the oracle on every case).  No GPU is touched here.

The sequence tests load the feeder's full map, which covers the image: ThinCandidates leaves AddPointEpipolar a few candidates per level,
ReFindInSingleKeyFrame measures almost only at level 0, and the template cache of ReFind_Common is hit a few times in a run.  The cases here
turn cheap levers instead, each checked on the oracle: sparse sub-maps (tracker_cases.sub_map: less is thinned away, one frame gives a
hundred calls), max_patches_per_frame = 100 (the tracker measures 100 points, the re-find gets the rest, at every level), the dense
texture rects = 4000 (re-find windows longer than 64 and 128 list entries, more corners per block of the epipolar filter),
wiggle_scale = 0.02 (every ray ends before it starts: stage 1), a frame rendered at a map keyframe's own pose (every epipolar segment
shorter than 1e-4: stage 2), and max_points just above the sub-map's size (the capacity branch of the ordered commit: stage 7).

A Case is a scene key, a sub-map, parameters, a start pose, an optional own frame and (group D) its targets; groups of cases are the
streams of one System.  Every case runs one tracked frame that becomes a keyframe, the four idle jobs in order, and a second tracked
frame (record()).  Everything is derived from the oracle, nothing from the device.

What stays unreached in every case (test_grow_cases.py asserts the counts are zero, so that a change that reaches one is noticed):
stage 3 (the line outside largest_radius), stage 4 (candidates keep a border of 10 pixels, the template needs P / 2 + 1), an equal-ZMSSD
tie at the strict minimum of the epipolar search, the start-depth clip (v3RayStart_TC[2] <= 0), a stored corner list cut at
16384 / 8192 / 4096 / 2048 entries, and a failure queue beyond its 8192 entries.  No scene is built for any of these."""
import functools

import numpy as np

from helpers import make_oracle, make_scene
from tracker_cases import _zoomed, sub_map
from visualslam_android_amd import capi

W, H = 320, 240
PER_LEVEL, SEED = (120, 50, 20, 8), 77
DENSE_RECTS = 4000
PATCHES_PER_STEP = {8: 8, 11: 4}                            # k_epipolar scores this many survivors of one ballot per step
GROW_WAVES = 4                                              # candidates per chunk of k_epipolar's ordered commit
BASE = (("grow_map", 3), ("idle_iterations", -1), ("ba_sum_order", 1))
MAX_POINTS = 256


def _with(pkw, **kw):
    return tuple(x for x in pkw if x[0] not in kw) + tuple(sorted(kw.items()))


@functools.lru_cache(maxsize=None)
def scene(rects=None):
    return make_scene(W, H, seed=SEED, n_frames=2, per_level=PER_LEVEL, rects=rects)


def _levels(rects=None):
    return np.array([q["level"] for q in scene(rects)[1]["points"]])


class Case:
    """keep: None = the full map, "no map" = nothing loaded, else the indices of the sub-map.  at_kf: the start pose is that map
    keyframe's and both frames are rendered there.  zoom: the start pose is the scene's moved along the optical axis to 1 / zoom of its
    distance from the plane, frames rendered there.  kf_request = False: the tracker has just dropped a keyframe, so it asks for none."""

    def __init__(self, name, keep=None, pkw=BASE, rects=None, at_kf=None, zoom=None, kf_request=True, target=None):
        self.name, self.pkw, self.rects, self.at_kf, self.zoom, self.kf_request, self.target = name, tuple(pkw), rects, at_kf, zoom, kf_request, dict(target or {})
        self.keep = keep if keep is None or isinstance(keep, str) else np.asarray(keep, np.int64)
        self._map, self._frames = None, {}

    @property
    def has_map(self):
        return not isinstance(self.keep, str)

    @property
    def grows(self):
        return self.has_map and self.kf_request

    def map(self):
        if self._map is None:
            m = scene(self.rects)[1]
            self._map = m if self.keep is None else sub_map(m, self.keep)
        return self._map

    def start_pose(self):
        f, m, _frames = scene(self.rects)
        if self.zoom is not None:
            return _zoomed(f.pose(-1), self.zoom)
        return f.pose(-1) if self.at_kf is None else np.asarray(m["keyframes"][self.at_kf]["pose"], np.float64)

    def frame(self, t):
        if self.at_kf is None and self.zoom is None:
            return scene(self.rects)[2][t]
        if t not in self._frames:
            self._frames[t] = scene(self.rects)[0].render_pose(self.start_pose(), key=t)
        return self._frames[t]

    def params(self, n_streams, patch):
        return capi.default_params(W, H, n_streams, patch_size=patch, **dict(self.pkw))

    def oracle(self, patch, **pkw):
        o = make_oracle(capi.default_params(W, H, 1, patch_size=patch, **dict(_with(self.pkw, **pkw))), self.map(), self.start_pose())
        if not self.kf_request:
            o.set_last_keyframe_dropped(0)
        return o

    def load(self, g, s):
        if not self.has_map:
            return
        g.load_map(s, self.map()); g.set_pose(s, self.start_pose())
        if not self.kf_request:
            g.set_last_keyframe_dropped(s, 0)


# ---- what the oracle does on a case ---------------------------------------------------------------------------------------------
class Record:
    """the oracle's run of a case: frame 0, the four idle jobs, frame 1"""

    def per_level(self):
        return [int((self.log[:, 0] == l).sum()) for l in range(4)]

    def stages(self, level=None):
        st = self.log[:, 2] if level is None else self.log[self.log[:, 0] == level, 2]
        return {int(k): int((st == k).sum()) for k in np.unique(st)}

    def chunks(self):
        """the full chunks of GROW_WAVES consecutive candidates of a level: (all accepted, some accepted and some not)"""
        full = mixed = 0
        for l in range(4):
            st = self.log[self.log[:, 0] == l, 2]
            for c in range(0, len(st) - GROW_WAVES + 1, GROW_WAVES):
                acc = int((st[c:c + GROW_WAVES] == 0).sum())
                full += acc == GROW_WAVES
                mixed += 0 < acc < GROW_WAVES
        return full, mixed


@functools.lru_cache(maxsize=None)
def _record(case, patch, pkw):
    o = case.oracle(patch, **dict(pkw))
    r = Record()
    r.n0, r.kf0 = o.state().n_points, o.state().n_keyframes
    o.track_frame(case.frame(0))
    st = o.state()
    r.kf_added, r.n_points, r.n_keyframes, r.quality0 = st.kf_added, st.n_points, st.n_keyframes, st.quality
    r.log, r.detail = o.grow_log(), o.grow_detail()
    for job in range(4):
        o.idle_job(job)
    r.idle = o.idle_stats()
    o.track_frame(case.frame(1))
    st = o.state()
    r.kf_added1, r.n_points1, r.quality1, r.attempted1, r.found1 = st.kf_added, st.n_points, st.quality, list(st.attempted), list(st.found)
    r.refind = o.refind_log()
    o.close()
    return r


def record(case, patch, **pkw):
    return _record(case, patch, tuple(sorted(pkw.items())))


# ---- group A: epipolar counts -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def group_a():
    n, lv = len(_levels()), _levels()
    nd = len(_levels(DENSE_RECTS))
    return [Case("full map"),
            Case("every 2nd point", np.arange(0, n, 2)), Case("every 4th point", np.arange(0, n, 4)),
            Case("every 8th point", np.arange(0, n, 8)), Case("every 16th point", np.arange(0, n, 16)),
            Case("level-0 points only", np.flatnonzero(lv == 0)), Case("levels 1-3 only", np.flatnonzero(lv > 0)),
            Case("first 200 points", np.arange(200)),
            Case("dense texture, every 8th point", np.arange(0, nd, 8), rects=DENSE_RECTS),
            Case("no keyframe request", np.arange(0, n, 8), kf_request=False),
            Case("no map", "no map")]


# ---- group B: re-find ---------------------------------------------------------------------------------------------------------------
B_PKW = _with(BASE, max_patches_per_frame=100)


BAD_SCALE_ZOOM = 2.0


@functools.lru_cache(maxsize=None)
def group_b():
    """The fourth stream is there for the cached verdict.  A template that MakeTemplateCoarseCont regenerates is bad when the warp samples
    outside the source image, which the 10-pixel border of candidates and map points rules out here; a kept template says what the last
    generation said unless the scale is bad (determinant of the warp below 0.25, or above 3 at level 3).  So a cache hit is bad only by
    a bad scale: the new keyframe seen from twice as close, whose new level-0 points the map's keyframes see at less than half the size."""
    n = len(_levels())
    return [Case("full map, 100 patches", None, B_PKW), Case("every 2nd point, 100 patches", np.arange(0, n, 2), B_PKW),
            Case("dense texture, full map, 100 patches", None, B_PKW, rects=DENSE_RECTS),
            Case("every 8th point, %.0fx closer, 100 patches" % BAD_SCALE_ZOOM, np.arange(0, n, 8), B_PKW, zoom=BAD_SCALE_ZOOM)]


# ---- group C: whole-level rejections ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def group_c(which):
    n = len(_levels())
    if which == "stage 1":
        return [Case("wiggle_scale = 0.02", np.arange(0, n, 8), _with(BASE, wiggle_scale=0.02), target=dict(stage=1))]
    return [Case("at the pose of map keyframe 0", np.arange(0, n, 8), _with(BASE, max_kf_dist_wiggle_mult=0.0), at_kf=0, target=dict(stage=2))]


# ---- group D: map capacity ----------------------------------------------------------------------------------------------------------
D_PKW = _with(BASE, max_points=MAX_POINTS)
EXACT_FIT_STRIDES = ((27, 1), (15, 2)) + tuple((st, off) for st in range(9, 40) for off in range(3))     # (stride, first point) tried for n + points added == MAX_POINTS
MID_CHUNK_SIZES = tuple(range(201, 230))                   # first-n sub-maps tried for a first stage-7 call inside a chunk


def first_full(rec):
    """(level, index among the level's candidates) of the first stage-7 call, or None"""
    for i in np.flatnonzero(rec.log[:, 2] == 7)[:1]:
        l = int(rec.log[i, 0])
        return l, int((rec.log[:i, 0] == l).sum())
    return None


@functools.lru_cache(maxsize=None)
def exact_fit_case(patch):
    """the first strided sub-map of EXACT_FIT_STRIDES whose growth, by the oracle's own count without a limit, ends on exactly MAX_POINTS
    points: with max_points = MAX_POINTS the last accepted candidate takes the last slot and no call meets a full map"""
    n_all = len(_levels())
    for st, off in EXACT_FIT_STRIDES:
        c = Case("every %dth point from %d (exact fit)" % (st, off), np.arange(off, n_all, st), D_PKW, target=dict(full_level=None))
        if record(c, patch, max_points=0).n_points == MAX_POINTS:
            return c
    raise AssertionError("no sub-map of EXACT_FIT_STRIDES grows to exactly %d points" % MAX_POINTS)


@functools.lru_cache(maxsize=None)
def mid_chunk_case(patch):
    """the first-n sub-map whose first stage-7 call is not the first wavefront of its chunk"""
    for n in MID_CHUNK_SIZES:
        c = Case("first %d points (full inside a chunk)" % n, np.arange(n), D_PKW, target=dict(full_level=0, mid_chunk=True))
        ff = first_full(record(c, patch))
        if ff is not None and ff[1] % GROW_WAVES:
            return c
    raise AssertionError("no first-n sub-map of MID_CHUNK_SIZES fills the map inside a chunk")


def fill_level(rec):
    """the level of the call that adds the last point"""
    return int(rec.log[np.flatnonzero(rec.log[:, 2] == 0)[-1], 0])


def _fills_during(patch, name, keep, level):
    """the sub-map, with as many of the map's first points outside it added as it takes for the map to fill during `level` (none at 8x8; at 11x11 the
    every-8th sub-map accepts one candidate fewer at level 0 and needs one point more)"""
    extra = np.setdiff1d(np.arange(len(_levels())), keep)
    for k in range(5):
        c = Case(name + (", %d more" % k if k else "") + ", %d slots" % MAX_POINTS, np.sort(np.r_[keep, extra[:k]]), D_PKW, target=dict(full_level=level))
        if fill_level(record(c, patch)) == level:
            return c
    raise AssertionError("%s does not fill the map during level %d" % (name, level))


@functools.lru_cache(maxsize=None)
def group_d(patch):
    n = len(_levels())
    return [_fills_during(patch, "every 8th point", np.arange(0, n, 8), 0), _fills_during(patch, "every 16th point", np.arange(0, n, 16), 1),
            _fills_during(patch, "first 200 points", np.arange(200), 0), exact_fit_case(patch), mid_chunk_case(patch)]


GROUP_NAMES = ("a: epipolar counts", "b: re-find", "c: stage 1", "c: stage 2", "d: map capacity")


def groups(patch):
    return {"a: epipolar counts": group_a(), "b: re-find": group_b(), "c: stage 1": group_c("stage 1"), "c: stage 2": group_c("stage 2"),
            "d: map capacity": group_d(patch)}
