"""Warped-template cases at the level, cache and source-border edges, shared by tests/test_template_cases.py (CPU: the oracle alone reaches
every target) and tests/test_gpu_template_edges.py (GPU: the device == the oracle on every case).  No GPU is touched here.

Every patch search starts from the template that csrc/patch_dev.h makes (search_level_and_warp, template_warp_matrix, warp_moved,
template_warp and its steps, warp_sample).  Its decisions come from jni/PatchFinder.cc:31-125 and jni/vision/ImageHandler.cpp:12-113: the
search level (det > 3 per level, the cap at level 3, det < 0.25), the refresh limit of 0.07 on a column of the warp, nOutside != 0, and the
verdict a kept template carries forward.  The groups here put a chosen point on each side of each decision:

a  level thresholds.  For each of the five decisions (level 0->1, 1->2, 2->3, 3->bad, bad->0) and chosen points, two camera distances that
   are adjacent doubles of tracker_cases._zoomed's z, found by bisection on the oracle, at which the point's verdict differs.  The rounded
   pose leaves the determinant some ulps apart between the two, so the streams take, of the poses within NUDGE ulps of the bisected one,
   the two whose determinants (read from the oracle's warp) stand closest to the threshold on either side; each side is a stream.
   Plain and with the camera tilted TILT_DEG degrees, so that the off-diagonal terms of the warp take part in det.
b  the refresh limit.  Two frames with the pose set before each: frame 0 makes the templates at Z0, frame 1 is zoomed (or rolled about the
   optical axis, or swung about the spot the camera looks at, which moves the first column of the warp most) by an amount bisected so that the oracle keeps the template on one side and makes it again on the other, then moved by
   up to NUDGE ulps so that the squared column move (worked out from the oracle's warp) stands closest to 0.07 squared.  Three more
   streams hold, at one level and in search-list order, kept and re-made templates in turn, kept ones only and re-made ones only.
c  the source border.  Maps built with patch_border = patch // 2 - 1 .. patch // 2 + 2, cut down to the points nearer than 10 level pixels
   to a border of their source image, seen at zooms 0.6, 0.8, 1.0 and 2.0 and tilted: templates with samples outside the source (zeros,
   bad verdict).  A second frame at the same pose (the kept verdict) and a third zoomed in by NEAR (made again, many of them good).
d  the sticky bad scale.  z0, 0.99 z0, z0 with z0 = 0.50 .. 0.54: points good, then out by a bad scale, then back in the potentially visible
   set with a kept template that is still bad (mbTemplateBad is only cleared where the template is made again); a fourth frame zoomed in
   by NEAR makes them again.

A case is a tracker_cases.Case with one pose per frame (SeqCase); the pose is set, with a zero velocity, before every frame.  Everything is
derived from the oracle, nothing from the device."""
import functools
import itertools

import numpy as np

import oracle.binding as orc
import tracker_cases as tc
from helpers import make_oracle, make_scene

W, H = tc.W, tc.H
SMALL = (131, 77)                                           # levels of 65x38, 32x19 and 16x9
SEED = 1234
PKW = tc.ALL_SELECTED
ZERO_VEL = (0.0,) * 6
PPW = tc.PATCHES_PER_WAVE
TILT_DEG = 25.0

# (a)
TRANSITIONS = ((0, 1), (1, 2), (2, 3), (3, -1), (-1, 0))   # verdicts of search_level_and_warp on the far and on the near side, -1 = bad scale
ZOOM_GRID = np.linspace(0.4, 2.0, 81)
POINTS_PER_THRESHOLD = 2
N_FILLERS = 6
NUDGE = 3                                                   # ulps each way on the entries of the translation, around the bisected pose
# (b)
Z0 = 1.2                                                    # no level threshold of the scene's points lies between 1.0 and 1.7
Z_FAR, Z_MAX, ROLL_MAX = 1.0, 1.5, np.radians(12.0)
REFRESH_KINDS = (("zoom", 4), ("roll", 2), ("swing", 2))    # (what the camera does between the frames, points)
SWING_MAX = np.radians(40.0)
MIX_ZOOMS = tuple(np.linspace(1.28, 1.36, 17))
# (c)
VIEWS = (("zoom 0.6", 0.6, 0.0), ("zoom 0.8", 0.8, 0.0), ("zoom 1.0", 1.0, 0.0), ("zoom 2.0", 2.0, 0.0), ("zoom 1.0, tilted", 1.0, TILT_DEG))
NEAR = 1.5                                                  # the zoom-in of the last frame of groups c and d: every column of the warp moves by more than 0.07
RING = 10                                                   # feeder.build_map's default border: points nearer than this to a side are the border points
CLEAR = 12                                                  # a point this far from the other three sides can leave its source only through the one it is near
MAX_BORDER_POINTS = 160
SIDES = ("left", "top", "right", "bottom")
# (d)
STICKY_ZOOMS = (0.50, 0.52, 0.54)
STICKY_MIN = 8


@functools.lru_cache(maxsize=None)
def scene(w, h, border=RING):
    return make_scene(w, h, seed=SEED, n_frames=1, per_level=tc.SPARSE, patch_border=border)


def base_pose(w, h, tilt=0.0):
    p = scene(w, h)[0].pose(-1)
    return tc._tilted(p, np.radians(tilt)) if tilt else p


def view_pose(w, h, z, tilt=0.0):
    return tc._zoomed(base_pose(w, h, tilt), z)


def rolled(pose12, angle):
    """the camera turned by `angle` about its optical axis"""
    c, s = np.cos(angle), np.sin(angle)
    Rz = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
    R, t = np.asarray(pose12[:9]).reshape(3, 3), np.asarray(pose12[9:])
    return np.r_[(Rz @ R).ravel(), Rz @ t]


def swung(pose12, angle):
    """the camera swung by `angle` about the vertical axis through the spot of the plane z = 0 it looks at: the same spot from the same
    distance, seen from the side, so the scene is foreshortened across and the first column of the warp moves"""
    c, s = np.cos(angle), np.sin(angle)
    Ry = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    R, t = np.asarray(pose12[:9]).reshape(3, 3), np.asarray(pose12[9:])
    spot = np.array([0.0, 0.0, (R.T @ t)[2] / R[2, 2]])          # in the camera's frame: along the optical axis to the plane
    return np.r_[(Ry @ R).ravel(), Ry @ (t - spot) + spot]


def with_made_point(m, f, kf, level, x, y):
    """the map with one more point: the scene's surface at pixel (x, y) of level `level` of keyframe kf, with the pixel vectors the
    feeder gives it (Feeder.make_point) and its source measurement"""
    made = f.make_point(m["keyframes"][kf]["pose"], level, x, y)
    assert made is not None, (kf, level, x, y)
    pos, right, down = made
    s = 1 << level
    q = {"pos": pos, "src_kf": kf, "level": level, "irx": int(x), "iry": int(y), "right": right, "down": down}
    return {"keyframes": m["keyframes"], "points": list(m["points"]) + [q],
            "meas": list(m["meas"]) + [(kf, len(m["points"]), level, (x + 0.5) * s - 0.5, (y + 0.5) * s - 0.5, 1, 2)]}


class SeqCase(tc.Case):
    """a sub-map of scene(w, h, border) and one camera pose per frame, each frame rendered at its pose"""

    def __init__(self, name, size, keep, poses, target=None, border=RING, made=()):
        """made: (keyframe, level, x, y) of points to add behind the sub-map's, made by the feeder at those pixels of the keyframe's level"""
        super().__init__(name, tuple(size) + (SEED, tc.SPARSE), keep, PKW, target or {}, pose=poses[0], own_frames=True)
        self.border, self.poses, self.made = border, [np.asarray(p, np.float64) for p in poses], tuple(made)

    def _scene(self):
        return scene(self.size[0], self.size[1], self.border)

    def map(self):
        if self._map is None:
            m = self._scene()[1]
            self._map = m if self.keep is None else tc.sub_map(m, self.keep)
            for kf, level, x, y in self.made:
                self._map = with_made_point(self._map, self._scene()[0], kf, level, x, y)
        return self._map

    def frame(self, t):
        if t not in self._frames:
            self._frames[t] = self._scene()[0].render_pose(self.poses[t], key=t)
        return self._frames[t]

    def begin(self, t, o=None, g=None, s=None):
        """the pose of frame t and a zero velocity, on the oracle and on stream s of the System"""
        if o is not None:
            o.set_pose(self.poses[t]); o.set_velocity(ZERO_VEL)
        if g is not None:
            g.set_pose(s, self.poses[t]); g.set_velocity(s, ZERO_VEL)


def run(case, patch):
    """the oracle alone on the case: per frame the levels after the first search stage with the template flags there (a fresh template
    state shows a bad scale as bad without have) and the warp of the first point (after the frame: the warp its template was made with),
    the tracks and the templates after the fine search, and the counters"""
    o = case.oracle(patch)
    recs = []
    for t in range(len(case.poses)):
        case.begin(t, o)
        o.frame_begin(case.frame(t)); o.search_stage(0)
        pvs_level, pvs_tm, warp0 = o.point_tracks()["level"].copy(), o.templates(), o.warp(0)[0]
        o.pose_stage(0); o.search_stage(1)
        tr, tm, st = o.point_tracks(), o.templates(), o.state()
        o.pose_stage(1); o.frame_end()
        recs.append(dict(pvs_level=pvs_level, pvs_bad=pvs_tm["bad"], pvs_have=pvs_tm["have"], warp0=warp0, last_warp0=o.warp(0)[1], tracks=tr, tmpl=tm, attempted=list(st.attempted), n_zmssd=st.n_zmssd,
                         nf=int(((tr["level"] >= 0) & (tr["found"] == 1)).sum()), quality=o.state().quality))
    o.close()
    return recs


def in_view(size, pose12, pos):
    """the point projects into the image (tracker_cases.row_kinds' 13-double row)"""
    w, h = size
    cam5 = list(tc._params(w, h, 1, 8, PKW).cam[:])
    lr = orc.cam_project(cam5, w, h, 0.0, 0.0)[3]
    p = np.asarray(pose12, np.float64)
    c = p[:9].reshape(3, 3) @ np.asarray(pos, np.float64) + p[9:]
    if c[2] < 0.001 or (c[0] / c[2]) ** 2 + (c[1] / c[2]) ** 2 > lr * lr:
        return False
    im, _d, inv, _lr = orc.cam_project(cam5, w, h, c[0] / c[2], c[1] / c[2])
    return not (inv or im[0] < 0 or im[1] < 0 or im[0] > w or im[1] > h)


class Probe:
    """One oracle on a map, stepped through poses on blank frames: the potentially visible set and the templates depend on the pose and the
    map, not on the frame, and with a zero velocity the predicted pose is the one set.  Cheap enough to bisect with.  What is found
    this way is only a choice: test_template_cases.py checks every case again on a fresh oracle with the frames the device gets."""

    def __init__(self, size, m, patch=8):
        self.o = make_oracle(tc._params(size[0], size[1], 1, patch, PKW), m, base_pose(*size))
        self.blank = np.zeros((size[1], size[0]), np.uint8)

    def levels(self, pose12):
        self.o.set_pose(pose12); self.o.frame_begin(self.blank); self.o.search_stage(0)
        return self.o.point_tracks()["level"].copy()

    def search(self, pose12):
        self.levels(pose12); self.o.pose_stage(0); self.o.search_stage(1)
        return self.o.point_tracks(), self.o.templates()

    def kept(self, pose0, pose1, far):
        """per point: the template made at pose0 is the one held after pose1.  The step to `far` first moves every warp by more than the
        limit, so that pose0 makes its templates whatever the probe did before."""
        self.search(far)
        tr0, t0 = self.search(pose0)
        tr1, t1 = self.search(pose1)
        same = (t0["tmpl"] == t1["tmpl"]).all((1, 2))
        ok = (tr0["level"] >= 0) & (tr0["searched"] == 1) & (tr1["searched"] == 1) & (tr1["level"] == tr0["level"])
        return same, ok, tr0["level"]

    def close(self):
        self.o.close()


def _spread(idx, k, seed):
    idx = np.asarray(idx)
    return np.sort(tc._shuffled(idx, seed)[:k]) if len(idx) > k else idx


# ---- (a) level thresholds ---------------------------------------------------------------------------------------------------------
def _bisect(verdict, lo, hi, v_lo, v_hi):
    """lo < hi with verdict(lo) == v_lo != v_hi == verdict(hi) -> the same with no double between them"""
    while True:
        mid = lo + (hi - lo) / 2
        if not lo < mid < hi:
            return lo, hi
        v = verdict(mid)
        assert v in (v_lo, v_hi), (lo, mid, hi, v, v_lo, v_hi)
        if v == v_lo:
            lo = mid
        else:
            hi = mid


def level_value(warp_inv, a):
    """what search_level_and_warp compares at the decision that ends verdict a: the determinant of the warp after the level loop's
    multiplications by 0.25 (jni/PatchFinder.cc:50-63), in the reference's association; against 3 for a >= 0, against 0.25 for a == -1"""
    det = float(warp_inv[0]) * float(warp_inv[3]) - float(warp_inv[1]) * float(warp_inv[2])
    for _ in range(max(a, 0)):
        det *= 0.25
    return det


def threshold(a):
    return 3.0 if a >= 0 else 0.25


def _nudged(pose12, n3):
    """the pose with the three entries of its translation moved by n3 ulps"""
    q = np.array(pose12, np.float64)
    for ax, n in enumerate(n3):
        for _ in range(abs(n)):
            q[9 + ax] = np.nextafter(q[9 + ax], np.inf if n > 0 else -np.inf)
    return q


def _tightest(pr, pose12, a, b):
    """Two adjacent zooms leave the determinant several ulps apart: the pose's entries are rounded.  Among the poses within NUDGE ulps of
    pose12 in each entry of the translation, the one with verdict a and the one with verdict b whose determinants stand closest to the
    threshold: ((pose, value) of a, (pose, value) of b).  pr probes a map of the point alone."""
    far = near = None
    for n3 in itertools.product(range(-NUDGE, NUDGE + 1), repeat=3):
        q = _nudged(pose12, n3)
        v, val = int(pr.levels(q)[0]), level_value(pr.o.warp(0)[0], a)
        if v == a and (far is None or abs(val - threshold(a)) < abs(far[1] - threshold(a))):
            far = (q, val)
        if v == b and (near is None or abs(val - threshold(a)) < abs(near[1] - threshold(a))):
            near = (q, val)
    return far, near


@functools.lru_cache(maxsize=None)
def straddles(tilt):
    """per transition up to POINTS_PER_THRESHOLD (point, z_lo, z_hi, far, near, fillers): the point's verdict is the transition's first at
    z_lo and its second at z_hi, adjacent doubles; far and near are (pose, value) with those verdicts, within NUDGE ulps of the pose of
    z_lo, whose determinants stand closest to the threshold (_tightest).  The point is in the image, so a verdict of -1 is the scale's;
    the fillers are points in the potentially visible set on both sides."""
    size = (W, H)
    m = scene(W, H)[1]
    base = base_pose(W, H, tilt)
    pr = Probe(size, m)
    L = np.array([pr.levels(tc._zoomed(base, z)) for z in ZOOM_GRID])
    out = {}
    for a, b in TRANSITIONS:
        found = []
        for k in range(len(ZOOM_GRID) - 1):
            for i in np.flatnonzero((L[k] == a) & (L[k + 1] == b)):
                pos = m["points"][i]["pos"]
                if all(i != j for j, *_ in found) and in_view(size, tc._zoomed(base, ZOOM_GRID[k]), pos) and in_view(size, tc._zoomed(base, ZOOM_GRID[k + 1]), pos):
                    found.append((int(i), k))
        pick = [found[0], found[-1]] if len(found) > POINTS_PER_THRESHOLD else found        # the first and the last in zoom: different source levels where the scene has them
        rows = []
        for i, k in pick[:POINTS_PER_THRESHOLD]:
            lo, hi = _bisect(lambda z: int(pr.levels(tc._zoomed(base, z))[i]), float(ZOOM_GRID[k]), float(ZOOM_GRID[k + 1]), a, b)
            one = Probe(size, tc.sub_map(m, [i]))
            far, near = _tightest(one, tc._zoomed(base, lo), a, b)
            one.close()
            both = np.flatnonzero((L[k] >= 0) & (L[k + 1] >= 0))
            rows.append((i, lo, hi, far, near, tuple(int(j) for j in _spread(both[both != i], N_FILLERS, i))))
        out[(a, b)] = rows
    pr.close()
    return out


@functools.lru_cache(maxsize=None)
def level_cases(tilt):
    """two streams per straddle: the point (first in the sub-map) and its fillers at the far and at the near pose, two frames at the same pose"""
    out = []
    for (a, b), rows in straddles(tilt).items():
        for i, lo, hi, far, near, fillers in rows:
            for (p, val), v in ((far, a), (near, b)):
                out.append(SeqCase("level %d->%d, point %d, z = %r%s, det %s" % (a, b, i, lo, ", tilted" if tilt else "", "below" if v == a else "above"), (W, H), (i,) + fillers, [p, p],
                                   dict(point=i, transition=(a, b), verdict=v, value=val, pair=(lo, hi))))
    return out


# ---- (b) the refresh limit --------------------------------------------------------------------------------------------------------
def _moved(kind, x):
    p0 = view_pose(W, H, Z0)
    return tc._zoomed(base_pose(W, H), x) if kind == "zoom" else rolled(p0, x) if kind == "roll" else swung(p0, x)


REFRESH_LIMIT2 = 0.07 * 0.07


def column_moves(warp_inv, level, last_warp):
    """what warp_moved compares with 0.07 squared, per column: the squared move of mm2WarpInverse.inverse() * LevelScale against the warp
    the template was made with (jni/PatchFinder.cc:82, 96-101), in the reference's association"""
    w = [float(x) for x in warp_inv]
    inv_det = 1.0 / (w[0] * w[3] - w[1] * w[2])
    sc = float(1 << level)
    m2 = [w[3] * inv_det * sc, -w[1] * inv_det * sc, -w[2] * inv_det * sc, w[0] * inv_det * sc]
    out = []
    for i in range(2):
        dx, dy = m2[i] - float(last_warp[i]), m2[2 + i] - float(last_warp[2 + i])
        out.append(dx * dx + dy * dy)
    return out


def _tightest_move(pr, j, pose1):
    """of the poses within NUDGE ulps of pose1 in each entry of the translation: the one whose larger column move is the largest that
    keeps the template of the probe's last search, and the one whose is the smallest that makes it again: ((pose, moves), (pose, moves))"""
    last = pr.o.warp(j)[1]
    far = near = None
    for n3 in itertools.product(range(-NUDGE, NUDGE + 1), repeat=3):
        q = _nudged(pose1, n3)
        lv = int(pr.levels(q)[j])                                  # the first search stage alone: no template is made, the last warp stays
        mv = column_moves(pr.o.warp(j)[0], lv, last)
        if max(mv) > REFRESH_LIMIT2:
            if near is None or max(mv) < max(near[1]):
                near = (q, mv)
        elif far is None or max(mv) > max(far[1]):
            far = (q, mv)
    return far, near


@functools.lru_cache(maxsize=None)
def refresh_straddles(kind, n_points):
    """n_points (point, x_lo, x_hi, kept, made): frame 0 at Z0, frame 1 zoomed to x (kind "zoom"), rolled by x about the optical axis (kind "roll") or swung by x about the spot it looks at (kind "swing"); the
    oracle keeps the point's template at x_lo and makes it again at x_hi, adjacent doubles; kept and made are (pose, column moves) within
    NUDGE ulps of the pose of x_lo whose larger move stands closest to the limit on either side (_tightest_move)"""
    m = scene(W, H)[1]
    p0, far = view_pose(W, H, Z0), view_pose(W, H, Z_FAR)
    x0, x1 = {"zoom": (Z0, Z_MAX), "roll": (0.0, ROLL_MAX), "swing": (0.0, SWING_MAX)}[kind]
    pr = Probe((W, H), m)
    same, ok, _lv = pr.kept(p0, _moved(kind, x1), far)
    cand = _spread(np.flatnonzero(ok & ~same), n_points, 3 + len(kind))
    pr.close()
    pr = Probe((W, H), tc.sub_map(m, cand))
    out = []
    for j, i in enumerate(cand):
        lo, hi = _bisect(lambda x: bool(pr.kept(p0, _moved(kind, x), far)[0][j]), x0, x1, True, False)
        pr.search(far); pr.search(p0)
        kept, made = _tightest_move(pr, j, _moved(kind, lo))
        out.append((int(i), float(lo), float(hi), kept, made))
    pr.close()
    return out


@functools.lru_cache(maxsize=None)
def mixed_wave_picks():
    """(z1, kept points, re-made points): level-0 points searched at Z0 and at z1, the z1 of MIX_ZOOMS at which the two kinds are most even"""
    m = scene(W, H)[1]
    pr = Probe((W, H), m)
    best = None
    for z1 in MIX_ZOOMS:
        same, ok, lv = pr.kept(view_pose(W, H, Z0), view_pose(W, H, z1), view_pose(W, H, Z_FAR))
        K, R = np.flatnonzero(ok & (lv == 0) & same), np.flatnonzero(ok & (lv == 0) & ~same)
        if best is None or min(len(K), len(R)) > min(len(best[1]), len(best[2])):
            best = (float(z1), K, R)
    pr.close()
    return best


@functools.lru_cache(maxsize=None)
def refresh_cases(patch):
    p0 = view_pose(W, H, Z0)
    out = []
    for kind, n_points in REFRESH_KINDS:
        for i, lo, hi, kept, made in refresh_straddles(kind, n_points):
            for (p1, moves), k in ((kept, True), (made, False)):
                out.append(SeqCase("refresh, %s, point %d, %s = %r, %s" % (kind, i, "z1" if kind == "zoom" else "angle", lo, "kept" if k else "made again"), (W, H), (i,), [p0, p1],
                                   dict(point=i, kept=[k], pair=(lo, hi), kind=kind, moves=moves)))
    z1, K, R = mixed_wave_picks()
    n = PPW[patch]
    assert len(K) >= 8 + n and len(R) >= 8 + n, (len(K), len(R))
    p1 = view_pose(W, H, z1)
    mixed = np.stack([K[:8], R[:8]], 1).ravel()                 # the sub-map's order is the search list's: one level, no coarse stage, no shuffle
    out.append(SeqCase("kept and re-made in turn, z1 = %r" % z1, (W, H), mixed, [p0, p1], dict(kept=[True, False] * 8)))
    out.append(SeqCase("one wavefront, all kept", (W, H), K[8:8 + n], [p0, p1], dict(kept=[True] * n)))
    out.append(SeqCase("one wavefront, all re-made", (W, H), R[8:8 + n], [p0, p1], dict(kept=[False] * n)))
    return out


# ---- (c) the source border --------------------------------------------------------------------------------------------------------
def borders(patch):
    return tuple(range(patch // 2 - 1, patch // 2 + 3))


def side_distances(size, q):
    """the distances of a point's patch centre from the left, top, right and bottom border of its source level"""
    lw, lh = size[0] >> q["level"], size[1] >> q["level"]
    return np.array([q["irx"], q["iry"], lw - 1 - q["irx"], lh - 1 - q["iry"]])


def only_side(size, q):
    """the side the point is nearer than RING to, if it keeps CLEAR from the other three (its template can then leave the source through that
    side only), else None"""
    d = side_distances(size, q)
    near = np.flatnonzero(d < RING)
    return SIDES[near[0]] if len(near) == 1 and (np.delete(d, near[0]) >= CLEAR).all() else None


def bottom_points(size, b, kf):
    """build_map keeps the first per_level cells in raster order, which at 320x240 end above the bottom rows: points made at chosen
    pixels b and b + 3 rows above the bottom border of levels 0 and 1 of keyframe kf"""
    out = []
    for level in (0, 1):
        lw, lh = size[0] >> level, size[1] >> level
        for x in np.linspace(CLEAR + 2, lw - 3 - CLEAR, 6).astype(int):
            out += [(kf, level, int(x), lh - 1 - b), (kf, level, int(x), lh - 1 - b - 3)]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def border_cases(patch, size):
    """per border width and view a stream: the map's points nearer than RING to a border of their source level (at most MAX_BORDER_POINTS)
    and a few others; frames at the view, at the view again, and NEAR times closer"""
    w, h = size
    out = []
    for b in borders(patch):
        m = scene(w, h, b)[1]
        ring = np.flatnonzero([side_distances(size, q).min() < RING for q in m["points"]])
        rest = np.setdiff1d(np.arange(len(m["points"])), ring)
        made = bottom_points(size, b, len(m["keyframes"]) - 1) if size == (W, H) else ()
        for name, z, tilt in VIEWS:
            keep = np.sort(np.r_[_spread(ring, MAX_BORDER_POINTS, b), _spread(rest, 8, b)])
            p = view_pose(w, h, z, tilt)
            out.append(SeqCase("%dx%d, border %d, %s" % (w, h, b, name), size, keep, [p, p, view_pose(w, h, z * NEAR, tilt)], dict(zoom=z, tilt=tilt), border=b, made=made))
    return out


def border_counts(case, rec0):
    """{(source level, side): [templates made good, templates made bad]} of the case's one-sided border points in frame 0.  A template that
    the frame made (have) and called bad has samples outside its source: a bad scale keeps a point out of the search list."""
    n = {}
    tm = rec0["tmpl"]
    for j, q in enumerate(case.map()["points"]):
        side = only_side(case.size, q)
        if side is not None and tm["have"][j]:
            n.setdefault((q["level"], side), [0, 0])[int(tm["bad"][j])] += 1
    return n


# ---- (d) the sticky bad scale -----------------------------------------------------------------------------------------------------
def sticky_points(recs):
    """points searched with a good template in frame 0, out by a bad scale in frame 1, back in the potentially visible set in frame 2 with the
    template of frame 0, still bad and not searched, and made again, good and searched, in frame 3"""
    r0, r1, r2, r3 = recs
    t0, t2, t3 = r0["tmpl"], r2["tmpl"], r3["tmpl"]
    ok = (r0["tracks"]["level"] >= 0) & (r0["tracks"]["searched"] == 1) & (t0["have"] == 1) & (t0["bad"] == 0)
    ok &= (r1["pvs_level"] == -1) & (r1["pvs_bad"] == 1)
    ok &= (r2["tracks"]["level"] >= 0) & (r2["tracks"]["searched"] == 0) & (t2["bad"] == 1) & (t2["tmpl"] == t0["tmpl"]).all((1, 2))
    ok &= (r3["tracks"]["level"] >= 0) & (r3["tracks"]["searched"] == 1) & (t3["bad"] == 0) & ~(t3["tmpl"] == t0["tmpl"]).all((1, 2))
    return np.flatnonzero(ok)


def _sticky_poses(z0):
    return [view_pose(W, H, z) for z in (z0, 0.99 * z0, z0, NEAR * z0)]


@functools.lru_cache(maxsize=None)
def sticky_cases(patch):
    """per z0 a stream: up to 24 of the points the out-and-back sequence leaves with a kept bad template, and 8 others"""
    out = []
    n_all = len(scene(W, H)[1]["points"])
    for z0 in STICKY_ZOOMS:
        full = SeqCase("sticky, full map", (W, H), None, _sticky_poses(z0))
        st = sticky_points(run(full, patch))
        keep = np.sort(np.r_[_spread(st, 24, 1), _spread(np.setdiff1d(np.arange(n_all), st), 8, 2)])
        out.append(SeqCase("sticky bad scale, z0 = %.2f" % z0, (W, H), keep, _sticky_poses(z0), dict(n_sticky=min(len(st), 24))))
    return out


# ---- the groups: each is the streams of one System --------------------------------------------------------------------------------
GROUP_NAMES = ("a: level thresholds", "a: level thresholds, tilted", "b: refresh limit", "c: source border, %dx%d" % (W, H), "c: source border, %dx%d" % SMALL,
               "d: sticky bad scale")


def groups(patch):
    return {"a: level thresholds": level_cases(0.0), "a: level thresholds, tilted": level_cases(TILT_DEG), "b: refresh limit": refresh_cases(patch),
            "c: source border, %dx%d" % (W, H): border_cases(patch, (W, H)), "c: source border, %dx%d" % SMALL: border_cases(patch, SMALL),
            "d: sticky bad scale": sticky_cases(patch)}
