"""Patch-search cases with chosen trip counts, shared by tests/test_search_trip_cases.py (CPU: every case reaches its target in the oracle)
and tests/test_gpu_search_trips.py (GPU: the device == the oracle on every case).  No GPU is touched here.

k_searchN (csrc/track.hip) filters the corners of a patch's row-LUT window N_CORNERS at a time and scores the survivors K_FLIGHT at a time.
What a single patch meets there depends on the frame, the predicted position and the level alone (tracker_cases.py: one oracle frame on
the full map tells it for every point), so a case is a sub-map that holds one chosen point, a few found points around it so that the pose
update has something to work on, and a target: the number of corners in the chosen point's window, the number that survive the x-window
and circle tests, a survivor too close to a border in the middle of a trip, two candidates of equal best ZMSSD in one trip or in two.
search_windows() recomputes coarse_window, the row-LUT range and the survivors from the oracle's corner lists and positions; nothing comes
from the device.  The points come from two scenes of the feeder, its own texture and one three times as dense (windows of 2 N + 1 corners).
Three kinds of case edit their first frame: the texture faded out around one corner (a window of one corner), a band of rows faded out (a
window of none beside windows of 2 N + 1 in one wavefront), a block of texture repeated inside the window (two corners with identical
neighbourhoods: equal ZMSSD, beside each other in raster order or a trip apart).  The empty window (coarse_window's `empty`) needs a level
whose last row is cut: 131x77 and a coarse range of 0, where a level-3 point projected below row 9 * 8 has a window that starts past
the level's 9 rows."""
import functools

import numpy as np

import oracle.binding as orc
import tracker_cases as tc
from helpers import make_oracle, make_scene
from tracker_cases import Case

N_CORNERS = 128                                         # SEARCH_N: window corners a lane group filters per trip
K_FLIGHT = 4                                            # SEARCH_K: survivors scored per trip
WINDOW_TARGETS = (0, 1, N_CORNERS - 1, N_CORNERS, N_CORNERS + 1, 2 * N_CORNERS, 2 * N_CORNERS + 1)
SURVIVOR_TARGETS = (0, 1, K_FLIGHT - 1, K_FLIGHT, K_FLIGHT + 1, 2 * K_FLIGHT + 1)
SCENE = tc.A_SCENE                                      # the feeder's texture: windows of up to some 150 corners at level 0
DENSE_SCENE = tc.A_SCENE + (8, 3000)                    # 3000 rectangles instead of 1000: windows of more than 2 N corners
SCENES = (SCENE, DENSE_SCENE)
PKW = tc.ALL_SELECTED                                   # no coarse stage, every point of the PVS searched once: the fine range is 10
FINE_RANGE = 10
N_FILLER = 7
PATCHES_PER_WAVE = tc.PATCHES_PER_WAVE
EMPTY_SIZE = (131, 77)
EMPTY_PKW = tc._with(tc.E_COARSE, coarse_range=0, coarse_min=1)


@functools.lru_cache(maxsize=None)
def scene(w, h, seed, per_level, n_keyframes=8, rects=None):
    """tracker_cases.scene with the feeder's number of rectangles as a sixth key"""
    if rects is None:
        return tc.scene(w, h, seed, per_level, n_keyframes)
    return make_scene(w, h, seed=seed, n_frames=tc.LOSS_FRAMES, n_keyframes=n_keyframes, per_level=per_level, rects=rects)


# ---- FindPatchCoarse's window, recomputed (jni/PatchFinder.cc:170-235) ---------------------------------------------------------------
def coarse_window(irx, iry, range_l0, level, rows):
    scale = 1 << level
    rng = (range_l0 + scale - 1) // scale
    top, bpo = int(iry - rng), int(iry + rng + 1)        # int() truncates toward zero, like the cast
    left, right = int(irx - rng), int(irx + rng)
    top = max(top, 0)
    return dict(range=rng, top=top, bottom_plus_one=bpo, left=left, right=right, empty=top >= rows or bpo <= 0)


def window_of(kf, level, image, range_l0, patch):
    """one patch's search: the window, its span [i0, i1) of the level's corner list, the survivors in raster order as (list index, x, y)
    and whether each keeps the patch's border"""
    img, corners, lut = kf[level]
    rows, cols = img.shape
    scale = 1 << level
    irx, iry = float(image[0]) / scale, float(image[1]) / scale
    cw = coarse_window(irx, iry, range_l0, level, rows)
    out = dict(level=level, empty=cw["empty"], i0=0, i1=0, survivors=[], inside=[])
    if cw["empty"]:
        return out
    i0 = int(lut[cw["top"]])
    i1 = len(corners) if cw["bottom_plus_one"] >= rows else int(lut[cw["bottom_plus_one"]])
    half = patch // 2
    r2 = float(cw["range"] * cw["range"])
    for ci in range(i0, i1):
        cx, cy = int(corners[ci] & 0xFFFF), int(corners[ci] >> 16)
        if cx < cw["left"] or cx > cw["right"]:
            continue
        dx, dy = irx - cx, iry - cy
        if dx * dx + dy * dy > r2:
            continue
        out["survivors"].append((ci, cx, cy))
        out["inside"].append(cx >= half and cy >= half and cx < cols - half and cy < rows - half)
    out["i0"], out["i1"] = i0, i1
    return out


def trip_of(w, k):
    """(filter trip, ZMSSD trip within it) of survivor k of window w"""
    f = (w["survivors"][k][0] - w["i0"]) // N_CORNERS
    first = next(j for j, sv in enumerate(w["survivors"]) if (sv[0] - w["i0"]) // N_CORNERS == f)
    return f, (k - first) // K_FLIGHT


def search_windows(tracks, frame, patch, thr, range_l0):
    """window_of for every searched point of `tracks` (an oracle's point_tracks after a search stage that did not re-project)"""
    kf = orc.make_keyframe_lite(frame, thr)
    return {int(i): window_of(kf, int(tracks["level"][i]), tracks["image"][i], range_l0, patch) for i in np.flatnonzero(tracks["searched"] == 1)}


def _thr(skey, patch, pkw):
    return tuple(tc._params(skey[0], skey[1], 1, patch, pkw).fast_threshold[:])


@functools.lru_cache(maxsize=None)
def full_windows(patch, skey=SCENE):
    """one oracle frame on the scene's full map (tracker_cases.full_frame): the flags and the windows of every searched point"""
    f, m, frames = scene(*skey)
    o = make_oracle(tc._params(skey[0], skey[1], 1, patch, PKW), m, f.pose(-1))
    o.frame_begin(frames[0]); o.search_stage(0); o.pose_stage(0); o.search_stage(1)
    fl = o.point_tracks()
    o.close()
    return fl, search_windows(fl, frames[0], patch, _thr(skey, patch, PKW), FINE_RANGE)


# ---- cases ------------------------------------------------------------------------------------------------------------------------
class TripCase(Case):
    """a Case whose first frame may be edited; `chosen` are the sub-map indices of the points the target speaks of"""
    def __init__(self, name, keep, chosen_points, target, edit=None, skey=SCENE, pkw=PKW, **kw):
        Case.__init__(self, name, skey, keep, pkw, target, **kw)
        keep = [] if self.keep is None else [int(i) for i in self.keep]
        self.chosen = [keep.index(int(p)) for p in chosen_points]
        self.edit = edit
        self._first = None

    def map(self):
        if self._map is None:
            m = scene(*self.skey)[1]
            self._map = m if self.keep is None else tc.sub_map(m, self.keep)
        return self._map

    def start_pose(self):
        return scene(*self.skey)[0].pose(self.start) if self.pose is None else np.asarray(self.pose, np.float64)

    def frame(self, t):
        if self.own_frames:
            if t not in self._frames:
                self._frames[t] = scene(*self.skey)[0].render_pose(self.start_pose(), key=t)
            return self._frames[t]
        fr = scene(*self.skey)[2][t]
        if t == 0 and self.edit is not None:
            if self._first is None:
                self._first = self.edit(fr)
            return self._first
        return fr


def case_windows(case, patch, stage=1, range_l0=FINE_RANGE):
    """the oracle on the case's own sub-map and first frame, up to search stage `stage`: tracks, windows, the oracle (left open for the
    caller, who closes it)"""
    o = case.oracle(patch)
    o.frame_begin(case.frame(0)); o.search_stage(0)
    if stage == 1:
        o.pose_stage(0); o.search_stage(1)
    tr = o.point_tracks()
    return o, tr, search_windows(tr, case.frame(0), patch, _thr(case.skey, patch, case.pkw), range_l0)


def _fillers(fl, avoid, seed):
    """found level-0 points spread over the map: what the pose update works on beside the chosen point"""
    F = np.flatnonzero((fl["searched"] == 1) & (fl["found"] == 1) & (fl["level"] == 0))
    F = F[~np.isin(F, avoid)]
    return tc._shuffled(F, seed)[:N_FILLER]


def _case(name, fl, points, target, seed, **kw):
    points = [int(p) for p in points]
    keep = np.sort(np.r_[np.array(points, np.int64), _fillers(fl, points, seed)])
    return TripCase(name, keep, points, target, **kw)


def _pick(patch, pred, what):
    """the first point, over the scenes, whose window satisfies pred: (scene key, flags, point)"""
    for skey in SCENES:
        fl, wins = full_windows(patch, skey)
        for i in sorted(wins):
            if pred(wins[i]):
                return skey, fl, i
    raise AssertionError("no point of the full maps has " + what)


@functools.lru_cache(maxsize=None)
def window_count_cases(patch):
    out = []
    for k, n in enumerate(WINDOW_TARGETS):
        if n == 1:
            out.append(one_corner_case(patch)); continue
        skey, fl, i = _pick(patch, lambda w: not w["empty"] and w["i1"] - w["i0"] == n, "a window of %d corners" % n)
        out.append(_case("window of %d corners" % n, fl, [i], dict(window=n), seed=100 + k, skey=skey))
    return out


@functools.lru_cache(maxsize=None)
def survivor_count_cases(patch):
    out = []
    for k, n in enumerate(SURVIVOR_TARGETS):
        skey, fl, i = _pick(patch, lambda w: len(w["survivors"]) == n and (n > 0 or w["i1"] > w["i0"]), "%d survivors" % n)
        out.append(_case("%d survivors" % n, fl, [i], dict(survivors=n), seed=200 + k, skey=skey))
    return out


def border_in_mid_trip(w):
    """the survivors of w that fail in_image_with_border with a survivor before and one after them in their ZMSSD trip"""
    hit = []
    for k, ok in enumerate(w["inside"]):
        if not ok and 0 < k < len(w["inside"]) - 1 and trip_of(w, k - 1) == trip_of(w, k) == trip_of(w, k + 1):
            hit.append(k)
    return hit


@functools.lru_cache(maxsize=None)
def border_case(patch):
    skey, fl, i = _pick(patch, lambda w: len(border_in_mid_trip(w)) > 0, "a survivor at the border in the middle of a trip")
    return _case("border survivor in mid trip", fl, [i], dict(border_mid_trip=True), seed=300, skey=skey)


# ---- edited frames ------------------------------------------------------------------------------------------------------------------
def fade_around(frame, cx, cy, r_in, r_out):
    """the frame's texture kept within r_in of (cx, cy) and faded to the mean grey at r_out: no edge, so no corner, is made"""
    h, w = frame.shape
    yy, xx = np.mgrid[0:h, 0:w]
    d = np.sqrt((xx - cx) ** 2.0 + (yy - cy) ** 2.0)
    wgt = np.clip((r_out - d) / float(r_out - r_in), 0.0, 1.0)
    mean = float(frame.mean())
    return np.clip(np.rint(mean + (frame.astype(np.float64) - mean) * wgt), 0, 255).astype(np.uint8)


def repeat_block(frame, cx, cy, half_lo, half_hi, ox, oy):
    """the block [c - half_lo, c + half_hi] around (cx, cy) -- a patch and the FAST ring inside it -- copied to (cx + ox, cy + oy)"""
    out = frame.copy()
    out[cy + oy - half_lo:cy + oy + half_hi + 1, cx + ox - half_lo:cx + ox + half_hi + 1] = frame[cy - half_lo:cy + half_hi + 1, cx - half_lo:cx + half_hi + 1]
    return out


def _found_corner(fl, i):
    """the level-0 corner the oracle found for point i (vfound is the corner's position, no sub-pixel step at level 0)"""
    return int(round(fl["vfound"][i][0])), int(round(fl["vfound"][i][1]))


@functools.lru_cache(maxsize=None)
def one_corner_case(patch):
    """a level-0 point whose frame keeps the texture around its corner only: the first radius at which its window holds one corner"""
    fl, wins = full_windows(patch)
    thr = _thr(SCENE, patch, PKW)
    frame0 = scene(*SCENE)[2][0]
    cand = [i for i in sorted(wins) if fl["level"][i] == 0 and fl["found"][i] == 1 and 40 < fl["image"][i][0] < 280 and 40 < fl["image"][i][1] < 200]
    for i in cand[:40]:
        cx, cy = _found_corner(fl, i)
        for r_in in (5, 6, 7, 8, 9, 10):
            edit = functools.partial(fade_around, cx=cx, cy=cy, r_in=r_in, r_out=r_in + 14)
            kf = orc.make_keyframe_lite(edit(frame0), thr)
            w = window_of(kf, 0, fl["image"][i], FINE_RANGE, patch)
            if w["i1"] - w["i0"] == 1:
                keep = np.array([i], np.int64)               # the faded frame shows no other point: the sub-map is the point alone
                return TripCase("window of 1 corner", keep, [i], dict(window=1), edit=edit)
    raise AssertionError("no faded frame leaves one corner in a window")


def equal_best(case, patch):
    """of the case's chosen point: the survivors whose ZMSSD equals the smallest (the oracle's template and frame), as ranks in raster order,
    their trips, and whether the oracle found the first of them"""
    o, tr, wins = case_windows(case, patch)
    p = case.chosen[0]
    w = wins[p]
    tmpl = o.template(p)["tmpl"]
    o.close()
    img = orc.make_keyframe_lite(case.frame(0), _thr(case.skey, patch, case.pkw))[w["level"]][0]
    ssd = [orc.zmssd(tmpl, img, x, y) if ok else None for (_ci, x, y), ok in zip(w["survivors"], w["inside"])]
    best = min(s for s in ssd if s is not None)
    ranks = [k for k, s in enumerate(ssd) if s == best]
    first = w["survivors"][ranks[0]]
    won = tr["found"][p] == 1 and (float(first[1]), float(first[2])) == tuple(tr["vfound"][p])
    return ranks, [trip_of(w, k) for k in ranks], bool(won), best


@functools.lru_cache(maxsize=None)
def tie_case(patch, same_trip):
    """a block of texture repeated inside a level-0 window: the found corner and its copy score the same.  Offsets along the row put the
    copy next to the original in raster order, offsets down the image put other survivors, and a trip's end, between them."""
    fl, wins = full_windows(patch)
    lo, hi = patch // 2, (patch - 1) // 2                    # a patch spans [c - PS / 2, c + (PS - 1) / 2]; the FAST ring (radius 3) lies inside
    hi = max(hi, 3)
    step = lo + hi + 1
    offsets = [(s * d, 0) for d in (step, step + 1, step + 2) for s in (1, -1)] if same_trip else [(0, s * d) for d in (step, step + 1, step + 2, step + 3) for s in (1, -1)]
    cand = [i for i in sorted(wins) if fl["level"][i] == 0 and fl["found"][i] == 1 and len(wins[i]["survivors"]) >= (2 if same_trip else K_FLIGHT + 2)
            and 40 < fl["image"][i][0] < 280 and 40 < fl["image"][i][1] < 200]
    for i in cand[:60]:
        cx, cy = _found_corner(fl, i)
        for ox, oy in offsets:
            edit = functools.partial(repeat_block, cx=cx, cy=cy, half_lo=lo, half_hi=hi, ox=ox, oy=oy)
            c = _case("equal best ZMSSD in %s" % ("one trip" if same_trip else "two trips"), fl, [i], dict(tie="same" if same_trip else "other"), seed=400 + i, edit=edit)
            try:
                ranks, trips, won, _best = equal_best(c, patch)
            except (ValueError, KeyError):
                continue
            if len(ranks) == 2 and won and (trips[0] == trips[1]) == same_trip:
                return c
    raise AssertionError("no repeated block gives two equal best candidates in %s" % ("one trip" if same_trip else "two trips"))


def fade_rows(frame, y0, y1, ramp=8):
    """rows [y0, y1] of the frame faded to the mean grey, over `ramp` rows on either side: a band without corners"""
    h = frame.shape[0]
    yy = np.arange(h, dtype=np.float64)
    wgt = np.clip(np.maximum(y0 - yy, yy - y1) / float(ramp), 0.0, 1.0)[:, None]
    mean = float(frame.mean())
    return np.clip(np.rint(mean + (frame.astype(np.float64) - mean) * wgt), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def mixed_wave_case(patch):
    """one wavefront's patches (8, or 4 at 11x11) at the extremes, all at level 0 so that they follow each other in the search list: windows
    of 2 N + 1 corners or more, a window of none (the point given twice at 8x8, its rows of the frame faded out; the others lie clear of
    the band), no survivor in a window that holds corners, 2 K + 1 survivors or more"""
    fl, wins = full_windows(patch, DENSE_SCENE)
    ppw = PATCHES_PER_WAVE[patch]
    lv0 = [i for i in sorted(wins) if fl["level"][i] == 0]
    big = [i for i in lv0 if wins[i]["i1"] - wins[i]["i0"] >= 2 * N_CORNERS + 1]
    crowded = [i for i in lv0 if len(wins[i]["survivors"]) >= 2 * K_FLIGHT + 1 and wins[i]["i1"] - wins[i]["i0"] <= N_CORNERS]
    none = [i for i in lv0 if not wins[i]["survivors"] and wins[i]["i1"] > wins[i]["i0"]]
    assert len(big) >= 2 and len(crowded) >= 2 and len(none) >= 2, (len(big), len(crowded), len(none))
    others = [big[0], none[0], crowded[0], big[-1], none[-1], crowded[-1]]
    clear = 2 * FINE_RANGE + 14                               # a window's rows, the ramp and a patch
    hollow = next(i for i in lv0 if 30 < fl["image"][i][1] < 210 and all(abs(fl["image"][i][1] - fl["image"][j][1]) > clear for j in others))
    y = int(fl["image"][hollow][1])
    edit = functools.partial(fade_rows, y0=y - FINE_RANGE - 1, y1=y + FINE_RANGE + 2)
    pts = ([hollow] + others[:3] + [hollow] + others[3:])[:ppw]
    c = TripCase("a wavefront of extremes", np.sort(np.array(pts, np.int64)), [], dict(mixed=True, n_search=len(pts)), edit=edit, skey=DENSE_SCENE)
    c.chosen = list(range(len(pts)))
    return c


# ---- the empty window ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def empty_window_case(patch):
    """131x77 with a coarse range of 0: level 3 has 9 rows, a level-3 point projected at y >= 72 has top = int(y / 8) = 9 = rows.  The map
    seen from closer puts points at level 3; the first zoom at which the coarse stage searches such a point is taken."""
    skey = EMPTY_SIZE + (1234, tc.SPARSE)
    for z in (4.0, 4.5, 5.0, 5.5, 6.0, 7.0, 3.6, 3.2):
        c = TripCase("empty window", None, [], dict(empty=True), skey=skey, pkw=EMPTY_PKW, pose=tc._zoomed(scene(*skey)[0].pose(-1), z), own_frames=True)
        o, tr, wins = case_windows(c, patch, stage=0, range_l0=0)
        o.close()
        hit = [i for i in sorted(wins) if wins[i]["empty"]]
        if hit:
            c.chosen = hit
            return c
    raise AssertionError("no zoom puts a searched level-3 point below the last full row")


# ---- the groups: each is the streams of one System ----------------------------------------------------------------------------------
GROUP_NAMES = ("17 streams", "9 streams", "1 stream: a wavefront of extremes", "1 stream: the empty window")


def groups(patch):
    w, s = window_count_cases(patch), survivor_count_cases(patch)
    ties = [tie_case(patch, True), tie_case(patch, False)]
    all17 = w + s + [border_case(patch)] + ties + [mixed_wave_case(patch)]
    assert len(all17) == 17
    nine = [w[6], s[5], ties[1], w[1], s[0], border_case(patch), w[3], ties[0], w[4]]          # the streams in another order, nine of them
    return {"17 streams": all17, "9 streams": nine, "1 stream: a wavefront of extremes": [mixed_wave_case(patch)],
            "1 stream: the empty window": [empty_window_case(patch)]}
