"""Trail-tracking and MiniPatch cases with chosen counts, shared by tests/test_trail_cases.py (CPU: the oracle alone reaches every
condition) and tests/test_gpu_trail_counts.py (GPU: the device == the oracle on every case).  No GPU is touched here.

The feeder sequences of tests/test_gpu_bootstrap.py keep about 200 trails in windows of about 60 corners: one trail per thread of
k_trail_advance's compaction, at most two chunks of 64 in mp_find, never a tie, never a reset.  The frames here are cheap instead: windows
of one seeded conftest.synth_image shifted by a few pixels per frame (crops), windows of a random p x p byte tile repeated over the plane
(period 7, 9, 13: every patch has exact copies 7, 9, 13 pixels away, so the searches meet equal SSDs and the candidates equal Shi-Tomasi
scores), a flat frame (no corner at all), a crop with a rectangle painted flat (the trails inside it find an empty box: the lever
for `good`), and a crop with one half brighter in one frame and darker in the next (the backward search misses on SSD).  Sizes: 96x64 and 157x101 (the front end's band form; at 157 the row pitch of the device's level 0 is not the width), 160x120
and 320x240 (the strip form).

A Case is a list of frames and the frame indices of its spacebar presses; the cases of a group are the streams of one System.  Only first
presses: a press always meets a stream whose stage is 0 (run() asserts it), InitFromStereo has tests/test_gpu_bootstrap*.py.

start_ref / advance_ref restate TrailTracking_Start / TrailTracking_Advance (jni/Tracker.cc:290-346) from orc.fast10, orc.fast_score,
orc.nonmax, orc.candidates, orc.minipatch_sample, orc.minipatch_find and numpy, keep every trail's 81-byte patch, and say of every search
what csrc/boot.hip's mp_find meets on it (Search).  run(case) drives them through the case's frames; test_trail_cases.py holds every
frame of it to the oracle System's trails() and init_info().  Everything is derived from the oracle, nothing from the device.

Every target of TARGETS is reached by a case, so UNREACHED is empty.  A target that a later change of the cases can no longer reach goes
there (at most three, none of BARRED); test_trail_cases.py asserts that the count of a listed target is zero, so that a change that reaches
it again is noticed."""
import functools

import numpy as np

import oracle.binding as orc
from conftest import synth_image
from visualslam_android_amd import capi

MAX_TRAILS = 1000                        # MaxInitialTrails, jni/Tracker.cc:305 (BOOT_MAX_TRAILS)
MAX_SSD = 100000                         # MiniPatchMaxSSD, jni/Tracker.cc:249
RANGE = 10
HALF = 4                                 # MiniPatch::mnHalfPatchSize
CHUNK, STEP = 64, 8                      # mp_find: list entries per ballot, corners scored per step
THREADS = 256                            # k_trail_advance's compaction: thread i owns trails [i * per, (i + 1) * per)
MIN_GOOD = 10                            # jni/Tracker.cc:266
MARGIN = 32                              # the crops' room to move inside their source image
SIZES = ((96, 64), (157, 101), (160, 120), (320, 240))
UNREACHED = ()                           # names of TARGETS no case reaches


# ---- frame builders -----------------------------------------------------------------------------------------------------------------
def _crops(big, w, h, offsets):
    out = []
    for dx, dy in offsets:
        assert abs(dx) <= MARGIN and abs(dy) <= MARGIN
        out.append(np.ascontiguousarray(big[MARGIN + dy:MARGIN + dy + h, MARGIN + dx:MARGIN + dx + w]))
    return out


@functools.lru_cache(maxsize=None)
def _synth_big(seed, w, h):
    return synth_image(seed, w + 2 * MARGIN, h + 2 * MARGIN)


def synth_crops(seed, w, h, offsets):
    """windows of one synth_image at the given (dx, dy) offsets: the scene moves by the differences"""
    return _crops(_synth_big(seed, w, h), w, h, offsets)


def tiled_crops(period, seed, w, h, offsets):
    """windows of a random period x period byte tile repeated over the plane"""
    tile = np.random.default_rng(seed).integers(0, 256, size=(period, period), dtype=np.uint8)
    big = np.tile(tile, ((h + 2 * MARGIN) // period + 1, (w + 2 * MARGIN) // period + 1))[:h + 2 * MARGIN, :w + 2 * MARGIN]
    return _crops(big, w, h, offsets)


def flat_frame(w, h, value=100):
    return np.full((h, w), value, np.uint8)


def with_flat_rect(frame, x0, y0, x1, y1, value=100):
    out = frame.copy()
    out[y0:y1, x0:x1] = value
    return out


def steps(n, dx=1, dy=0, start=(0, 0)):
    """n offsets moving by (dx, dy) per frame"""
    return [(start[0] + t * dx, start[1] + t * dy) for t in range(n)]


class Case:
    def __init__(self, name, frames, presses):
        self.name, self.frames, self.presses = name, [np.ascontiguousarray(f, np.uint8) for f in frames], tuple(sorted(presses))
        self.h, self.w = self.frames[0].shape
        assert all(f.shape == (self.h, self.w) for f in self.frames) and all(0 <= t < len(self.frames) for t in self.presses)

    def params(self, n_streams, **kw):
        return capi.default_params(self.w, self.h, n_streams, grow_map=3, **kw)

    def oracle(self):
        return orc.OracleSystem(orc.params_from_vslam(self.params(1)))


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
class Frame:
    """level 0 of a frame as the trail code sees it: the image and its FAST corners in raster order with their row table"""

    def __init__(self, img, thr=10):
        self.img = np.ascontiguousarray(img, np.uint8)
        self.h, self.w = self.img.shape
        self.corners = orc.fast10(self.img, thr)
        self.cx, self.cy = (self.corners & 0xFFFF).astype(np.int64), (self.corners >> 16).astype(np.int64)
        self.n = len(self.corners)
        self.lut = np.searchsorted(self.cy, np.arange(self.h + 1))          # lut[y] = first corner of row >= y; lut[h] = n
        self.win = np.lib.stride_tricks.sliding_window_view(self.img, (9, 9))
        self.inside = (self.cx >= HALF) & (self.cy >= HALF) & (self.cx < self.w - HALF) & (self.cy < self.h - HALF)


class Search:
    """One FindPatch call (jni/MiniPatch.cc:35-68) as csrc/boot.hip's mp_find walks it: the row window [lut[T], lut[B + 1]) in chunks of 64
    list entries, the in-box corners of a chunk in steps of eight, the first strict minimum in list order.
      found, x, y   the oracle's answer (orc.minipatch_find)
      win_len       entries of the row window
      box           in-box corners per chunk (one entry per chunk of the window, none for an empty window)
      near_border   in-box corners closer than 4 px to a border (SSDAtPoint answers max_ssd + 1)
      best          the minimal SSD over the in-box corners with a whole patch (None: there is none)
      win_chunk, win_step   chunk of the window and step of eight of that chunk in which the first minimum is scored
      n_tied        in-box corners that share the minimal SSD (1: no tie)
      tie           None, "same step", "steps" (different steps of one chunk) or "chunks": the widest separation among the tied corners
      edges         subset of "tblr": the image edges the box crosses"""

    def __init__(self, patch, fr, x, y, rng=RANGE, max_ssd=MAX_SSD):
        self.found, self.x, self.y = orc.minipatch_find(patch, fr.img, fr.corners, x, y, rng, max_ssd)
        L, R, T, B = x - rng, x + rng, y - rng, y + rng
        i0, i1 = int(fr.lut[min(max(T, 0), fr.h)]), int(fr.lut[min(max(B + 1, 0), fr.h)])
        i1 = max(i1, i0)
        self.win_len = i1 - i0
        self.edges = "".join(e for e, c in zip("tblr", (T < 0, B > fr.h - 1, L < 0, R > fr.w - 1)) if c)
        idx = i0 + np.flatnonzero((fr.cx[i0:i1] >= L) & (fr.cx[i0:i1] <= R))
        chunk = (idx - i0) // CHUNK
        nchunks = (self.win_len + CHUNK - 1) // CHUNK
        self.box = np.bincount(chunk, minlength=nchunks).astype(int).tolist() if nchunks else []
        ins = fr.inside[idx]
        self.near_border = int((~ins).sum())
        self.best, self.win_chunk, self.win_step, self.n_tied, self.tie = None, None, None, 0, None
        if ins.any():
            k = np.flatnonzero(ins)
            d = fr.win[fr.cy[idx[k]] - HALF, fr.cx[idx[k]] - HALF].astype(np.int64) - np.asarray(patch, np.int64).reshape(9, 9)
            ssd = (d * d).reshape(len(k), -1).sum(1)
            self.best = int(ssd.min())
            tied = k[ssd == self.best]                                       # positions among the in-box corners, list order
            step = np.array([int((chunk[:j] == chunk[j]).sum()) // STEP for j in tied])
            self.win_chunk, self.win_step, self.n_tied = int(chunk[tied[0]]), int(step[0]), len(tied)
            if len(tied) > 1:
                self.tie = "chunks" if len(set(chunk[tied])) > 1 else "steps" if len(set(step)) > 1 else "same step"
            # the numpy restatement and the oracle agree on the winner
            assert self.found == (self.best < max_ssd) and (not self.found or (self.x, self.y) == (int(fr.cx[idx[tied[0]]]), int(fr.cy[idx[tied[0]]])))
        else:
            assert not self.found
        self.miss = None if self.found else ("empty" if len(idx) == 0 else "ssd")


class Trail:
    __slots__ = ("init", "cur", "patch")

    def __init__(self, init, cur, patch):
        self.init, self.cur, self.patch = init, cur, patch


class StartRecord:
    """TrailTracking_Start: n_cand level-0 candidates inside MiniPatch's border, n_scores distinct Shi-Tomasi scores among them, cut_in_tie:
    ranks 999 and 1000 (from 0) share a score, so candidate order alone decides which of the two becomes a trail"""


def level0_candidates(fr, vp):
    sc = orc.fast_score(fr.img, fr.corners, vp.nonmax_barrier)
    keep = orc.nonmax(fr.corners, sc, quirk=bool(vp.quirks & capi.Q_NONMAX_RIGHT_NEIGHBOUR))
    return orc.candidates(fr.img, keep, 70.0, 10)


def start_ref(fr, vp):
    """-> (trails, StartRecord): the at most 1000 in-border candidates of lowest Shi-Tomasi score, equal scores in candidate order"""
    pos, score = level0_candidates(fr, vp)
    x, y = (pos & 0xFFFF).astype(int), (pos >> 16).astype(int)
    inb = (x >= HALF) & (y >= HALF) & (x < fr.w - HALF) & (y < fr.h - HALF)
    x, y, score = x[inb], y[inb], score[inb]
    order = np.argsort(score, kind="stable")
    r = StartRecord()
    r.n_cand, r.n_scores = len(order), len(np.unique(score))
    r.cut_in_tie = bool(len(order) > MAX_TRAILS and score[order[MAX_TRAILS - 1]] == score[order[MAX_TRAILS]])
    trails = []
    for i in order[:MAX_TRAILS]:
        p = (int(x[i]), int(y[i]))
        trails.append(Trail(p, p, orc.minipatch_sample(fr.img, *p)))
    return trails, r


class TrailRecord:
    """one trail in one TrailTracking_Advance: fwd / back (Search, back None after a forward miss), d2 (squared distance of the backward
    answer from the start, None without one), kept"""


def advance_ref(trails, cur, prev):
    """-> (surviving trails in order, good, [TrailRecord]): forward search at cur's corners, backward search from there at prev's, kept when
    the backward answer is within sqrt(2) px of where the trail stood; good counts the forward finds"""
    keep, recs, good = [], [], 0
    for t in trails:
        r = TrailRecord()
        r.fwd, r.back, r.d2 = Search(t.patch, cur, *t.cur), None, None
        found = r.fwd.found
        if found:
            end = (r.fwd.x, r.fwd.y)
            r.back = Search(orc.minipatch_sample(cur.img, *end), prev, *end)
            found = r.back.found
            if found:
                r.d2 = (r.back.x - t.cur[0]) ** 2 + (r.back.y - t.cur[1]) ** 2
                found = r.d2 <= 2
            good += 1
            if found:
                keep.append(Trail(t.init, end, t.patch))
        r.kept = found
        recs.append(r)
    return keep, good, recs


class FrameRecord:
    """one frame of run(): stage before and after, what happened ("idle", "start", "advance", "reset": an advance that ended in Reset),
    n (trails entering an advance), good, start (StartRecord), trails (TrailRecord list), the (n, 4) array trails() must show after it"""


def run(case, shift_patches_after=None):
    """the case's frames through start_ref / advance_ref -> [FrameRecord].  shift_patches_after = t: after frame t's compaction every kept
    trail carries the patch of its successor in the list (what a compaction that copies patches one slot off would leave)"""
    vp = case.params(1)
    stage, trails, prev, out = 0, [], None, []
    for t, img in enumerate(case.frames):
        fr = Frame(img, vp.fast_threshold[0])
        r = FrameRecord()
        r.stage_before, r.what, r.n, r.good, r.start, r.trails = stage, "idle", None, None, None, []
        if t in case.presses:
            assert stage == 0, "%s: the press of frame %d would be a second press" % (case.name, t)
            trails, r.start = start_ref(fr, vp)
            stage, r.what = 1, "start"
        elif stage == 1:
            r.n = len(trails)
            trails, r.good, r.trails = advance_ref(trails, fr, prev)
            r.what = "advance"
            if r.good < MIN_GOOD:
                trails, stage, r.what = [], 0, "reset"
            elif shift_patches_after == t and len(trails) > 1:
                trails = [Trail(a.init, a.cur, b.patch) for a, b in zip(trails, trails[1:] + trails[:1])]
        prev = fr
        r.stage = stage
        r.positions = np.array([t_.init + t_.cur for t_ in trails], np.int32).reshape(-1, 4)
        out.append(r)
    return out


@functools.lru_cache(maxsize=None)
def record(case):
    return run(case)


# ---- the conditions at which the kernels split, counted on the records --------------------------------------------------------------
START_TARGETS = ("start: 0 candidates", "start: 1-255 candidates", "start: 257-999 candidates", "start: > 1000 candidates, all scores distinct",
                 "start: > 1000 candidates, one score", "start: ranks 999 and 1000 share a score")
N_TARGETS = ("n = 0", "n = 1", "n not a multiple of 4", "n in 1-256 (per = 1)", "n in 257-512 (per = 2)", "n in 769-999 (per = 4)", "n = 1000 (per = 4)",
             "per = 2: survivors after a thread's range with drops", "per = 4: survivors after a thread's range with drops")
WINDOW_TARGETS = ("window 0", "window 1-64", "window 65-128", "window 129-192", "window > 256", "a chunk without a box corner before one with",
                  "chunk with 1-7 box corners", "chunk with 8, 16, ... box corners", "chunk with > 8 box corners, no multiple of 8",
                  "winner outside the first chunk", "winner outside the first step of eight")
TIE_CLASSES = ("same step", "steps", "chunks")
TIE_TARGETS = tuple("tie: %s" % c for c in TIE_CLASSES) + tuple("tie: %s, forward, trail kept" % c for c in TIE_CLASSES)
EDGE_TARGETS = ("box over the top edge", "box over the bottom edge", "box over the left edge", "box over the right edge", "box corner within 4 px of a border")
OUTCOME_TARGETS = ("forward miss, empty box", "forward miss on SSD", "backward miss", "distance^2 0 kept", "distance^2 1 kept", "distance^2 2 kept",
                   "distance^2 >= 4 dropped", "good >= 10 with 1-9 survivors", "good >= 10 with no survivor", "good = 10 (continues)", "good = 9 (resets)", "reset")
SEQUENCE_TARGETS = ("first press after a reset",)
TARGETS = START_TARGETS + N_TARGETS + WINDOW_TARGETS + TIE_TARGETS + EDGE_TARGETS + OUTCOME_TARGETS + SEQUENCE_TARGETS
# never to be listed in UNREACHED: each of these has been reached on the oracle alone
BARRED = START_TARGETS + N_TARGETS[3:7] + WINDOW_TARGETS[:4] + ("tie: same step", "tie: chunks", "good >= 10 with no survivor", "reset")


def per_thread(n):
    return (n + THREADS - 1) // THREADS


def crosses_a_range(kept, per):
    """k_trail_advance's compaction: some thread's range [i * per, (i + 1) * per) holds a dropped trail and a later range a kept one, so
    the kept one's slot is the scan over the ranges before it and not its own index"""
    kept = np.asarray(kept, bool)
    drops = np.flatnonzero(~kept)
    return bool(len(drops) and kept[(drops[0] // per + 1) * per:].any())


def tally(recs):
    """-> {target: count} over the FrameRecords of one case"""
    c = dict.fromkeys(TARGETS, 0)
    reset_seen = False
    for r in recs:
        if r.start is not None:
            s = r.start
            c["start: 0 candidates"] += s.n_cand == 0
            c["start: 1-255 candidates"] += 1 <= s.n_cand <= 255
            c["start: 257-999 candidates"] += 257 <= s.n_cand <= 999
            c["start: > 1000 candidates, all scores distinct"] += s.n_cand > MAX_TRAILS and s.n_scores == s.n_cand
            c["start: > 1000 candidates, one score"] += s.n_cand > MAX_TRAILS and s.n_scores == 1
            c["start: ranks 999 and 1000 share a score"] += s.cut_in_tie
            c["first press after a reset"] += reset_seen
        if r.what not in ("advance", "reset"):
            continue
        n, per, kept = r.n, per_thread(r.n), [x.kept for x in r.trails]
        left = sum(kept)
        c["n = 0"] += n == 0; c["n = 1"] += n == 1; c["n not a multiple of 4"] += n % 4 != 0
        c["n in 1-256 (per = 1)"] += 1 <= n <= 256; c["n in 257-512 (per = 2)"] += 257 <= n <= 512
        c["n in 769-999 (per = 4)"] += 769 <= n <= 999; c["n = 1000 (per = 4)"] += n == 1000
        if per in (2, 4) and crosses_a_range(kept, per):
            c["per = %d: survivors after a thread's range with drops" % per] += 1
        c["good >= 10 with 1-9 survivors"] += r.good >= MIN_GOOD and 1 <= left <= 9
        c["good >= 10 with no survivor"] += r.good >= MIN_GOOD and left == 0
        c["good = 10 (continues)"] += r.good == MIN_GOOD; c["good = 9 (resets)"] += r.good == MIN_GOOD - 1
        if r.what == "reset":
            c["reset"] += 1
            reset_seen = True
        for x in r.trails:
            for s in (x.fwd, x.back):
                if s is None:
                    continue
                L = s.win_len
                c["window 0"] += L == 0; c["window 1-64"] += 1 <= L <= 64; c["window 65-128"] += 65 <= L <= 128
                c["window 129-192"] += 129 <= L <= 192; c["window > 256"] += L > 256
                nz = [k for k, b in enumerate(s.box) if b]
                c["a chunk without a box corner before one with"] += bool(nz) and any(b == 0 for b in s.box[:nz[-1]])
                c["chunk with 1-7 box corners"] += any(1 <= b <= 7 for b in s.box)
                c["chunk with 8, 16, ... box corners"] += any(b and b % STEP == 0 for b in s.box)
                c["chunk with > 8 box corners, no multiple of 8"] += any(b > STEP and b % STEP for b in s.box)
                if s.best is not None:
                    c["winner outside the first chunk"] += s.win_chunk > 0
                    c["winner outside the first step of eight"] += s.win_step > 0
                if s.tie:
                    c["tie: %s" % s.tie] += 1
                for e, name in zip("tblr", ("top", "bottom", "left", "right")):
                    c["box over the %s edge" % name] += e in s.edges
                c["box corner within 4 px of a border"] += s.near_border > 0
            if x.fwd.tie and x.kept:
                c["tie: %s, forward, trail kept" % x.fwd.tie] += 1
            c["forward miss, empty box"] += x.fwd.miss == "empty"; c["forward miss on SSD"] += x.fwd.miss == "ssd"
            c["backward miss"] += x.back is not None and not x.back.found
            if x.d2 is not None:
                if x.d2 <= 2:
                    c["distance^2 %d kept" % x.d2] += 1
                c["distance^2 >= 4 dropped"] += x.d2 >= 4
    return {k: int(v) for k, v in c.items()}


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
def brightness_steps(frame, x1, deltas):
    """the frame with its columns [0, x1) brighter by each delta (clipped): FAST sees the same corners away from the seam, a MiniPatch SSD
    grows by 81 * delta^2.  +20 then -20: both forward searches stay below MiniPatchMaxSSD (32,400), the backward search of the second
    frame compares the two shifted frames (129,600) and misses"""
    out = []
    for d in deltas:
        f = frame.astype(np.int32)
        f[:, :x1] += d
        out.append(np.clip(f, 0, 255).astype(np.uint8))
    return out


JUMP = [(0, 0), (1, 1), (2, 2), (3, 3), (15, 8), (16, 9), (17, 10), (18, 11)]          # three small moves, one of (12, 5), three small moves
IDLE = steps(8, 1, 0)


@functools.lru_cache(maxsize=None)
def good_edge_case(w, h, want):
    """A synth crop whose second frame has its columns [0, x) painted flat: the trails there find an empty box.  The first (seed, x), x moved
    one column at a time, at which TrailTracking_Advance counts exactly `want` forward finds."""
    vp = capi.default_params(w, h, 1, grow_map=3)
    for seed in range(3, 12):
        f = synth_crops(seed, w, h, steps(8, 1, 0))
        f0 = Frame(f[0], vp.fast_threshold[0])
        trails, _r = start_ref(f0, vp)
        for x in range(0, w):
            cur = Frame(with_flat_rect(f[1], 0, 0, x, h), vp.fast_threshold[0])
            good = sum(orc.minipatch_find(t.patch, cur.img, cur.corners, *t.cur)[0] for t in trails)      # advance_ref's count, without its records
            if good == want:
                return Case("synth %d, columns [0, %d) of frame 1 flat: good = %d" % (seed, x, want), [f[0], with_flat_rect(f[1], 0, 0, x, h)] + f[2:], [0])
            if good < want:
                break
    raise AssertionError("no flat rectangle leaves good = %d at %dx%d" % (want, w, h))


def single_candidate_case(w, h):
    """a flat frame with one brighter rectangle in its top left corner: the rectangle's one corner away from the borders is the only level-0
    candidate (three FAST corners, one maximal).  One trail, which the next frame's advance meets as n = 1 and finds: good = 1"""
    return Case("one rectangle corner", [with_flat_rect(flat_frame(w, h), 0, 0, 40 + t, 30, 200) for t in range(8)], [1])


def flat_case(w, h, n, press):
    return Case("flat frames", [flat_frame(w, h)] * n, [press])


@functools.lru_cache(maxsize=None)
def group(size):
    """the streams of one System of the given (w, h), 8 frames each"""
    w, h = size
    if size == (96, 64):
        b = synth_crops(4, w, h, steps(6, 1, 0))
        return [Case("synth 3, a move of (12, 5)", synth_crops(3, w, h, JUMP), [0]),
                good_edge_case(w, h, MIN_GOOD), good_edge_case(w, h, MIN_GOOD - 1), single_candidate_case(w, h),
                Case("synth 4, the left half brighter by 20, then darker by 20", b[:2] + brightness_steps(b[2], w // 2, (20, -20, -20)) + b[3:], [1]),
                Case("synth 5 then flat frames", synth_crops(5, w, h, steps(3, 1, 0)) + [flat_frame(w, h)] * 5, [0]),
                flat_case(w, h, 8, 2)]
    if size == (157, 101):
        return [Case("synth 3, a move of (12, 5)", synth_crops(3, w, h, JUMP), [0]),
                Case("tile 7", tiled_crops(7, 1, w, h, IDLE), [1, 5]),
                Case("tile 13, moves of (3, 0) and (0, 3)", tiled_crops(13, 1, w, h, [(0, 0), (1, 0), (4, 0), (5, 0), (5, 3), (6, 3), (7, 3), (8, 3)]), [0]),
                Case("synth 6, moves of (-2, -1)", synth_crops(6, w, h, steps(8, -2, -1)), [0]),
                Case("synth 7, never pressed", synth_crops(7, w, h, IDLE), [])]
    if size == (160, 120):
        # frame 3: "tile 9" consumes its first press, "tile 13" advances, "flat frames" resets, "never pressed" has never been pressed
        return [Case("synth 1, a move of (12, 5)", synth_crops(1, w, h, JUMP), [0]),
                Case("tile 7, pressed again after its reset", tiled_crops(7, 1, w, h, IDLE), [1, 5]),
                Case("tile 9", tiled_crops(9, 1, w, h, IDLE), [3]),
                Case("tile 13, moves of (3, 0) and (0, 3)", tiled_crops(13, 1, w, h, [(0, 0), (1, 0), (4, 0), (5, 0), (5, 3), (6, 3), (7, 3), (8, 3)]), [0]),
                flat_case(w, h, 8, 2),
                Case("synth 2, never pressed", synth_crops(2, w, h, IDLE), [])]
    assert size == (320, 240)
    return [Case("synth 3, a move of (12, 5)", synth_crops(3, w, h, JUMP), [0]),
            Case("synth 3, moves of (7, 4)", synth_crops(3, w, h, [(0, 0), (0, 0), (1, 0), (8, 4), (9, 4), (16, 8), (17, 8), (18, 8)]), [1]),
            Case("synth 8, pressed late", synth_crops(8, w, h, IDLE), [5]),
            Case("synth 9, never pressed", synth_crops(9, w, h, IDLE), [])]


# per stream of a group the frames in which the stage goes from 1 back to 0 (Reset, jni/Tracker.cc:266-269): asserted of the oracle on the
# CPU and of the device on the GPU
RESETS = {(96, 64): [[4], [], [1], [2], [], [3], [3]], (157, 101): [[6], [3, 7], [5], [], []],
          (160, 120): [[], [3, 7], [5], [5], [3], []], (320, 240): [[], [], [], []]}


def resets(stages):
    """frames in which the stage goes from 1 back to 0, of the list of stages after each frame"""
    return [t for t in range(1, len(stages)) if (stages[t - 1], stages[t]) == (1, 0)]


def joint_frame(cases):
    """the first frame in which one stream consumes a first press, one advances, one resets and one has never been pressed (None: none)"""
    recs = [record(c) for c in cases]
    for t in range(len(cases[0].frames)):
        what = [r[t].what for r in recs]
        never = [not c.presses or min(c.presses) > t for c in cases]
        if "start" in what and "advance" in what and "reset" in what and any(never):
            return t
    return None


# ---- the two primitives (csrc/minipatch.hip) ------------------------------------------------------------------------------------------
class Primitive:
    """one vslam_minipatch_find call: the frame searched, (n, 9, 9) templates, (n, 2) positions, range, max_ssd"""

    def __init__(self, name, frame, patches, pos, rng, max_ssd):
        self.name, self.frame, self.rng, self.max_ssd = name, frame, int(rng), int(max_ssd)
        self.patches, self.pos = np.ascontiguousarray(patches, np.uint8).reshape(-1, 9, 9), np.ascontiguousarray(pos, np.int32).reshape(-1, 2)
        assert len(self.patches) == len(self.pos) >= 1

    def expected(self, fr=None):
        """-> (found (n), pos (n, 2): unchanged where nothing is found), by orc.minipatch_find"""
        fr = fr or Frame(self.frame)
        found, pos = np.zeros(len(self.pos), np.int32), self.pos.copy()
        for i, (x, y) in enumerate(self.pos):
            ok, nx, ny = orc.minipatch_find(self.patches[i], fr.img, fr.corners, int(x), int(y), self.rng, self.max_ssd)
            found[i] = ok
            if ok:
                pos[i] = (nx, ny)
        return found, pos


PRIM_RANGES = (0, 3, 10, 400)            # 400: larger than every image here


def sample_positions(fr, seed, n_corners=60, n_other=40):
    """corners of the frame, random positions (some closer than 4 px to a border), the four image corners, and one position 25 rows below
    the image and one 25 rows above it (k_minipatch_find's row-window clamps: both ends at ncorners, both at the list's start)"""
    rng = np.random.default_rng(seed)
    pick = fr.corners[rng.choice(fr.n, size=min(n_corners, fr.n), replace=False)] if fr.n else np.zeros(0, np.uint32)
    pos = [((int(c) & 0xFFFF), int(c) >> 16) for c in pick]
    pos += [(int(rng.integers(0, fr.w)), int(rng.integers(0, fr.h))) for _ in range(n_other)]
    pos += [(0, 0), (fr.w - 1, 0), (0, fr.h - 1), (fr.w - 1, fr.h - 1), (fr.w // 2, fr.h + 25), (fr.w // 2, -25)]
    return np.array(pos, np.int32)


def _patches_at(fr, pos, seed):
    """the oracle's samples; a random template where the position has no whole patch"""
    rng = np.random.default_rng(seed)
    out = np.zeros((len(pos), 9, 9), np.uint8)
    for i, (x, y) in enumerate(pos):
        p = orc.minipatch_sample(fr.img, int(x), int(y))
        out[i] = p if p is not None else rng.integers(0, 256, size=(9, 9), dtype=np.uint8)
    return out


@functools.lru_cache(maxsize=None)
def primitives(size):
    """-> (frames to sample from: [(name, frame, positions)], [Primitive])"""
    w, h = size
    a, b = synth_crops(3, w, h, [(0, 0), (2, 1)])
    fa, fb = Frame(a), Frame(b)
    pos = sample_positions(fa, 1)
    patches = _patches_at(fa, pos, 2)
    prims = [Primitive("synth, range %d" % r, b, patches, pos, r, MAX_SSD) for r in PRIM_RANGES]
    # max_ssd at, one above and far below the best SSD of a trail: strict <
    n_thr = 0
    for i in range(len(pos)):
        s = Search(patches[i], fb, int(pos[i][0]), int(pos[i][1]))
        if s.best is not None and 0 < s.best < MAX_SSD and n_thr < 6:
            n_thr += 1
            prims += [Primitive("synth, trail %d, max_ssd = %s" % (i, name), b, patches[i:i + 1], pos[i:i + 1], RANGE, m)
                      for name, m in (("best SSD", s.best), ("best SSD + 1", s.best + 1), ("0", 0))]
    assert n_thr == 6
    rnd = np.random.default_rng(3).integers(0, 256, size=(len(pos), 9, 9), dtype=np.uint8)
    prims.append(Primitive("random templates, max_ssd = 500", b, rnd, pos, RANGE, 500))
    ta, tb = tiled_crops(7, 1, w, h, [(0, 0), (1, 0)])
    fta = Frame(ta)
    tpos = np.stack([fta.cx, fta.cy], 1)[np.random.default_rng(4).choice(fta.n, size=1000, replace=False)].astype(np.int32)
    prims.append(Primitive("tile 7, 1000 corners", tb, _patches_at(fta, tpos, 5), tpos, RANGE, MAX_SSD))
    prims.append(Primitive("tile 7, range 400", tb, _patches_at(fta, tpos[:8], 5), tpos[:8], 400, MAX_SSD))
    ua, ub = tiled_crops(13, 1, w, h, [(0, 0), (3, 0)])                # copies 13 px apart in a row: ties inside one chunk
    fua = Frame(ua)
    upos = np.stack([fua.cx, fua.cy], 1)[np.random.default_rng(6).choice(fua.n, size=300, replace=False)].astype(np.int32)
    prims.append(Primitive("tile 13, 300 corners", ub, _patches_at(fua, upos, 7), upos, RANGE, MAX_SSD))
    prims.append(Primitive("a frame without corners", flat_frame(w, h), patches, pos, RANGE, MAX_SSD))
    return [("synth", a, pos), ("tile 7", ta, np.vstack([tpos, pos[-6:]])), ("flat", flat_frame(w, h), pos)], prims
