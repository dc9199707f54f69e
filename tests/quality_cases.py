"""Cases at the thresholds of the tracker's frame tail (the end of k_pose's fine stage and k_plan's velocity gate, csrc/track.hip;
jni/Tracker.cc:781-878, jni/MapMaker.cc:737-773, 1098-1101), shared by tests/test_quality_cases.py (CPU: the oracle reaches every target
exactly) and tests/test_gpu_frame_tail.py (GPU: the device == the oracle on every case).  No GPU is touched here.

The cases are sub-maps of tracker_cases.A_SCENE, chosen from one oracle frame on the full map (tracker_cases.fine_flags): with the coarse
stage off a patch's search depends on the point, the predicted pose and the frame alone, so a sub-map of f found and u unfound points of
a level gives exactly these counts.

(a) QUALITY_TABLE: per-level found / unfound counts that put AssessTrackingQuality's dTotal, la and dLarge on, just above and just below
    their cut-offs.  The exact-equality case lf / la == 13 / 100 needs 87 searched-and-unfound points at levels 2 and 3; neither A_SCENE
    (59 with 8x8 patches, 58 with 11x11) nor FULL_SCENE (82, 82) holds them, so this case alone tracks a frame whose columns from PAINT_X
    on are a flat grey: the points that project there are attempted and not found.  Its flags come from an oracle frame on that image.
(b) bracket(): a parameter that enters one comparison, bisected on the oracle over the bit patterns of the doubles until two ADJACENT
    doubles give different decisions: wiggle_scale (IsDistanceToNearestKeyFrameExcessive: quality 0 | 1), max_kf_dist_wiggle_mult
    (NeedNewKeyFrame: kf_added 1 | 0) and coarse_min_vel (k_plan: did_coarse 1 | 0).  The device agrees on both sides only if its closest,
    closest * (1.0 / depth_mean) and msd_vel carry the oracle's bits.
(c) gate_case(): min_frames_between_kf = 3 and max_kf_dist_wiggle_mult = 0, free-running: a keyframe every 4 frames.
(d) LOSS_SEQUENCES: blank frames for one or two frames, then real ones again: lost_frames counts up and is reset.  The last sequence
    holds a DODGY frame between two BAD ones: a real frame painted grey from column x on, x scanned on the oracle (dodgy_column) until
    the frame's quality is 1."""
import functools

import numpy as np

import tracker_cases as tc
from helpers import make_oracle

GREY = 128
PAINT_X = 160
BLANK = "blank"


def edited(frame, e):
    """a frame as a sequence feeds it: e = None (as rendered), BLANK (zeros) or a column x (the columns from x on a flat grey)"""
    if e is None:
        return frame
    if isinstance(e, str):
        assert e == BLANK
        return np.zeros_like(frame)
    out = frame.copy()
    out[:, int(e):] = GREY
    return out


@functools.lru_cache(maxsize=None)
def scene_frame(skey, t):
    """frame t of the scene's path; past the frames tracker_cases.scene holds, rendered by the scene's feeder"""
    f, _m, frames = tc.scene(*skey)
    return frames[t] if t < len(frames) else f.render(t, 1)[0]


class QCase(tc.Case):
    """a tracker_cases.Case whose frame t is edited by edits[t] (see edited)"""

    def __init__(self, name, skey, keep, pkw, target, edits=None, **kw):
        tc.Case.__init__(self, name, skey, keep, pkw, target, **kw)
        self.edits = dict(edits or {})

    def frame(self, t):
        return edited(scene_frame(self.skey, t), self.edits.get(t))

    def variant(self, name=None, target=None, edits=None, **params):
        """the same map, start and frames with other parameters"""
        c = QCase(name or self.name, self.skey, self.keep, tc._with(self.pkw, **params), self.target if target is None else target,
                  self.edits if edits is None else edits, start=self.start, vel=self.vel, pose=self.pose)
        c._map = self._map
        return c


@functools.lru_cache(maxsize=None)
def flags(skey, patch, paint_x=None):
    """tracker_cases.fine_flags on the scene's frame 0 painted grey from column paint_x on"""
    if paint_x is None:
        return tc.fine_flags(skey, patch)
    f, m, frames = tc.scene(*skey)
    o = make_oracle(tc._params(skey[0], skey[1], 1, patch, tc.ALL_SELECTED), m, f.pose(-1))
    o.frame_begin(edited(frames[0], paint_x)); o.search_stage(0); o.pose_stage(0); o.search_stage(1)
    t = o.point_tracks()
    o.close()
    return {"level": t["level"], "searched": t["searched"], "found": t["found"]}


def level_counts(fl):
    """(found, searched and not found) per level"""
    ok = fl["searched"] == 1
    return ([int((ok & (fl["found"] == 1) & (fl["level"] == l)).sum()) for l in range(4)],
            [int((ok & (fl["found"] == 0) & (fl["level"] == l)).sum()) for l in range(4)])


def choose_per_level(fl, found, unfound, seed=0):
    """found[l] points whose patch the oracle finds at level l and unfound[l] it searches there and does not find"""
    parts = []
    for l in range(4):
        ok = (fl["searched"] == 1) & (fl["level"] == l)
        F, U = np.flatnonzero(ok & (fl["found"] == 1)), np.flatnonzero(ok & (fl["found"] == 0))
        assert len(F) >= found[l] and len(U) >= unfound[l], (l, len(F), found[l], len(U), unfound[l])
        parts += [tc._shuffled(F, seed + l)[:found[l]], tc._shuffled(U, seed + 10 + l)[:unfound[l]]]
    return np.sort(np.concatenate(parts))


def assess(attempted, found):
    """AssessTrackingQuality's thresholds on the per-level counts (jni/Tracker.cc:832-878), before the excessive-distance demotion"""
    ta, tf, la, lf = sum(attempted), sum(found), sum(attempted[2:]), sum(found[2:])
    if tf == 0 or ta == 0:
        return 0
    d_total = tf / ta
    d_large = lf / la if la > 10 else d_total
    return 2 if d_total > 0.3 else 0 if d_large < 0.13 else 1


# ---- (a) the quality cut-offs -------------------------------------------------------------------------------------------------
# name, found per level, searched-and-unfound per level, expected quality, painted frame
QUALITY_TABLE = (
    ("dTotal == 3/10, la = 4", (1, 1, 1, 0), (2, 2, 2, 1), 1, None),
    ("dTotal == 30/100, lf/la = 3/20", (14, 13, 2, 1), (27, 26, 12, 5), 1, None),
    ("dTotal == 4/13", (2, 1, 1, 0), (4, 3, 1, 1), 2, None),
    ("la == 10, lf = 1, 8/40", (4, 3, 1, 0), (12, 11, 6, 3), 1, None),
    ("la == 11, lf = 1, 8/40", (4, 3, 1, 0), (11, 11, 7, 3), 0, None),
    ("lf/la == 2/15", (3, 3, 1, 1), (10, 10, 9, 4), 1, None),
    ("lf/la == 2/16", (3, 3, 1, 1), (10, 10, 10, 4), 0, None),
    ("tf == 0, ta = 12", (0, 0, 0, 0), (4, 4, 3, 1), 0, None),
    ("level 3 only, 1/1", (0, 0, 0, 1), (0, 0, 0, 0), 2, None),
    ("lf/la == 13/100", (2, 2, 11, 2), (8, 8, 75, 12), 1, PAINT_X),
)
DODGY_NAME = "dTotal == 3/10, la = 4"                         # the DODGY case the wiggle_scale bracket is taken on


@functools.lru_cache(maxsize=None)
def quality_cases(patch):
    out = []
    for k, (name, found, unfound, q, paint) in enumerate(QUALITY_TABLE):
        assert assess([f + u for f, u in zip(found, unfound)], found) == q, name        # the table states what the rule gives
        keep = choose_per_level(flags(tc.A_SCENE, patch, paint), found, unfound, seed=100 + k)
        target = dict(n_points=len(keep), attempted=[f + u for f, u in zip(found, unfound)], found=list(found), quality=q, did_coarse=0)
        out.append(QCase(name, tc.A_SCENE, keep, tc.NO_COARSE, target, edits={} if paint is None else {0: paint}))
    return out


def frame0(case, patch):
    """the oracle's state after the case's first frame"""
    o = case.oracle(patch)
    o.track_frame(case.frame(0))
    s = o.state()
    o.close()
    return s


# ---- (b) thresholds taken to one ulp ------------------------------------------------------------------------------------------
def _bits(x):
    return int(np.array(x, np.float64).view(np.int64))


def _double(b):
    return float(np.array(b, np.int64).view(np.float64))


def bisect_flip(decide, lo, hi):
    """decide(x) differs at 0 <= lo < hi: two adjacent doubles (a, b), lo <= a < b <= hi, with decide(a) == decide(lo) and
    decide(b) == decide(hi), and both decisions.  Non-negative doubles are ordered like their bit patterns, so halving the distance in
    bit patterns ends after at most 63 runs."""
    assert 0.0 <= lo < hi
    at_lo, at_hi = decide(lo), decide(hi)
    assert at_lo != at_hi, (lo, hi, at_lo)
    a, b = _bits(lo), _bits(hi)
    runs = 2
    while b - a > 1:
        mid = (a + b) // 2
        runs += 1
        if decide(_double(mid)) == at_lo:
            a = mid
        else:
            b = mid
    return _double(a), _double(b), at_lo, at_hi, runs


KF_BASE = tc._with(tc.NO_COARSE, min_frames_between_kf=0, ba_sum_order=1)
BRACKETS = {       # parameter: (what the oracle's state is asked, low end, high end, decisions at the low and the high end)
    "wiggle_scale": ("quality", 1e-6, 0.1, 0, 1),
    "max_kf_dist_wiggle_mult": ("kf_added", 0.0, 10.0, 1, 0),
    "coarse_min_vel": ("did_coarse", 0.0, 1.0, 1, 0),
}


@functools.lru_cache(maxsize=None)
def good_case(patch):
    """60 found and 4 unfound points: quality 2"""
    keep = tc.choose_found(tc.fine_flags(tc.A_SCENE, patch), 60, 4, seed=1)
    return QCase("60 found + 4 unfound", tc.A_SCENE, keep, tc.NO_COARSE, dict(n_points=64, quality=2, did_coarse=0))


@functools.lru_cache(maxsize=None)
def bracket_base(param, patch):
    if param == "wiggle_scale":
        return [c for c in quality_cases(patch) if c.name == DODGY_NAME][0]
    if param == "max_kf_dist_wiggle_mult":
        return good_case(patch).variant(**dict(KF_BASE))
    e = tc._e_case("fast start", patch, (10, 10, 30, tc.COARSE_MAX), tc.E_COARSE)      # n3 == coarse_max of tracker_cases.coarse_edge_cases
    return QCase(e.name, e.skey, e.keep, e.pkw, {}, start=e.start, vel=e.vel)


@functools.lru_cache(maxsize=None)
def bracket(param, patch):
    """(a, b, decision at a, decision at b, oracle runs): the adjacent doubles of `param` between which the oracle's decision flips"""
    key, lo, hi, _at_lo, _at_hi = BRACKETS[param]
    base = bracket_base(param, patch)
    return bisect_flip(lambda x: getattr(frame0(base.variant(**{param: x}), patch), key), lo, hi)


@functools.lru_cache(maxsize=None)
def bracket_pair(param, patch):
    """the base case at both ends of its bracket; the targets hold the decision (and n_keyframes for the keyframe request)"""
    a, b, at_a, at_b, _runs = bracket(param, patch)
    key = BRACKETS[param][0]
    base = bracket_base(param, patch)
    n_kf = len(base.map()["keyframes"])
    out = []
    for x, d in ((a, at_a), (b, at_b)):
        target = {key: d}
        if key == "kf_added":
            target["n_keyframes"] = n_kf + d
        out.append(base.variant(name="%s = %r" % (param, x), target=target, **{param: x}))
    return out


# ---- (c) the keyframe gate in frames --------------------------------------------------------------------------------------------
GATE_FRAMES = 9
GATE_MIN_FRAMES = 3
GATE = dict(min_frames_between_kf=GATE_MIN_FRAMES, max_kf_dist_wiggle_mult=0.0, ba_sum_order=1)


def gate_case(patch, **params):
    """the GOOD sub-map free-running with a keyframe wanted on every frame: frame - last > 3 grants every fourth"""
    kw = dict(GATE); kw.update(params)
    return good_case(patch).variant(name="keyframe gate", target={}, **kw)


def keyframe_frames(case, patch, n_frames=GATE_FRAMES):
    """the frames on which the free-running oracle adds a keyframe, and its n_keyframes after every frame"""
    o = case.oracle(patch)
    added, n_kf = [], []
    for t in range(n_frames):
        o.track_frame(case.frame(t))
        s = o.state()
        assert s.quality == 2, (t, s.quality)
        if s.kf_added:
            added.append(t)
        n_kf.append(s.n_keyframes)
    o.close()
    return added, n_kf


# ---- (d) loss and return ----------------------------------------------------------------------------------------------------
LOSS_FRAMES = 7
LOSS_SEQUENCES = (      # name, blank frames, lost_frames per frame
    ("two lost, back", (1, 2), [0, 1, 2, 0, 0, 0, 0]),
    ("one lost twice", (1, 3), [0, 1, 0, 1, 0, 0, 0]),
    ("two lost twice", (1, 2, 4, 5), [0, 1, 2, 0, 1, 2, 0]),
)
DODGY_SEQUENCE = ("DODGY between two BAD", (1, 3), 2, [2, 0, 1, 0, 2, 2, 2], [0, 1, 0, 1, 0, 0, 0])     # name, blank frames, painted frame, qualities, lost_frames
DODGY_SEEDS = (1, 2, 3, 4, 5, 6)
DODGY_COLUMNS = tuple(range(4, tc.W, 4))


def sequence(case, patch):
    """(quality, lost_frames) of every frame of the case in the free-running oracle"""
    o = case.oracle(patch)
    out = []
    for t in range(LOSS_FRAMES):
        o.track_frame(case.frame(t))
        s = o.state()
        out.append((s.quality, s.lost_frames))
    o.close()
    return out


def _loss_base(patch, seed=1):
    keep = tc.choose_found(tc.fine_flags(tc.A_SCENE, patch), 60, 4, seed=seed)
    return QCase("60 + 4", tc.A_SCENE, keep, tc.NO_KF, {})


@functools.lru_cache(maxsize=None)
def dodgy_column(patch):
    """(choose_found seed, column x): frame 2 painted grey from x on, between two blank frames, is DODGY in the oracle and the sequence is
    the one DODGY_SEQUENCE states; None when no seed of DODGY_SEEDS and no column of DODGY_COLUMNS gives it"""
    _name, blanks, painted, quality, lost = DODGY_SEQUENCE
    for seed in DODGY_SEEDS:
        base = _loss_base(patch, seed)
        for x in DODGY_COLUMNS:
            edits = {t: BLANK for t in blanks}
            edits[painted] = x
            if sequence(base.variant(edits=edits), patch) == list(zip(quality, lost)):
                return seed, x
    return None


@functools.lru_cache(maxsize=None)
def loss_cases(patch):
    """the sequences of LOSS_SEQUENCES on the 60 + 4 sub-map and, where dodgy_column finds one, DODGY_SEQUENCE; targets: quality and
    lost_frames per frame"""
    out = []
    for name, blanks, lost in LOSS_SEQUENCES:
        quality = [0 if t in blanks else 2 for t in range(LOSS_FRAMES)]
        out.append(_loss_base(patch).variant(name=name, target=dict(quality=quality, lost_frames=lost), edits={t: BLANK for t in blanks}))
    found = dodgy_column(patch)
    if found is not None:
        seed, x = found
        name, blanks, painted, quality, lost = DODGY_SEQUENCE
        edits = {t: BLANK for t in blanks}
        edits[painted] = x
        out.append(_loss_base(patch, seed).variant(name="%s (x = %d)" % (name, x), target=dict(quality=quality, lost_frames=lost), edits=edits))
    return out


def undisturbed(case):
    """the case with real frames throughout"""
    return case.variant(name=case.name + ", undisturbed", target={}, edits={})
