"""Tracker cases with chosen counts, shared by tests/test_tracker_cases.py (CPU: every case reaches its target in the oracle) and
tests/test_gpu_tracker_counts.py (GPU: the device == the oracle on every case).  No GPU is touched here.

How a count is chosen.  A patch's search depends on the predicted pose, the frame and the point itself, not on the other points of the
map -- as long as the point is selected: no coarse stage, max_patches_per_frame not reached.  ONE oracle frame on a full feeder map
(full_frame) therefore tells, per point, whether it is in the potentially visible set, at which level, and whether its patch is found.
sub_map() cuts a map down to chosen points; the choose_* functions pick them from those flags, so that the sub-map reaches a wanted
n_points, number of searched patches, per-level PVS count or number of found patches nf.  Everything is derived from the oracle,
nothing from the device, and test_tracker_cases.py asserts that the oracle, run on the sub-map alone, reaches every target exactly.

A Case carries its scene, sub-map, parameters, start state and targets; groups of cases are the streams of one System."""
import functools

import numpy as np

import oracle.binding as orc
from helpers import make_oracle, make_scene
from visualslam_android_amd import capi

W, H = 320, 240
SPARSE, DENSE = (120, 50, 20, 8), (330, 110, 40, 15)
NO_KF = (("min_frames_between_kf", 1000),)              # no keyframe, so no bundle adjustment moves a map between the two frames
FAST_VEL = (0.01, 0.012, 0.0, 0.0, 0.0, 0.0)            # the velocity prior of test_coarse_stage_and_pose_recovery (start pose 6 frames behind)
N_FRAMES = 2                                            # frame 2 takes the cached-template path
NF_TARGETS = (0, 1, 2, 3, 7, 8, 9, 20, 21, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 255, 256, 257, 511, 512, 513)
PATCHES_PER_WAVE = {8: 8, 11: 4}
N_SEARCH_TARGETS = {8: (1, 16, 10, 19, 28, 37, 46, 55), 11: (1, 8, 6, 7, 12, 13, 18, 23)}     # every residue modulo the patches per wavefront
N_POINTS_TARGETS = (1, 255, 256, 257, 513)
LOSS_STREAMS, LOSS_FRAMES = 17, 7
LOSS_IDLE = {7: "no map", 8: "lost", 16: "lost"}


@functools.lru_cache(maxsize=None)
def scene(w, h, seed, per_level, n_keyframes=8):
    return make_scene(w, h, seed=seed, n_frames=LOSS_FRAMES, n_keyframes=n_keyframes, per_level=per_level)


def sub_map(m, keep):
    """The map m cut down to the points keep (indices in map order; an index given k times makes k copies of the point, each with the
    point's measurements): all keyframes, the chosen points in their order, the measurements of the others dropped, point indices
    renumbered.  A plain dict of the form System.load_map and the oracle's load_map take."""
    keep = [int(i) for i in keep]
    new_of = {}
    for j, i in enumerate(keep):
        new_of.setdefault(i, []).append(j)
    pts = m["points"]
    meas = [(kf, j, lv, rx, ry, sp, src) for (kf, pt, lv, rx, ry, sp, src) in m["meas"] for j in new_of.get(pt, ())]
    return {"keyframes": m["keyframes"], "points": [dict(pts[i]) for i in keep], "meas": meas}


def _params(w, h, n_streams, patch, pkw):
    return capi.default_params(w, h, n_streams, patch_size=patch, **dict(pkw))


class Case:
    def __init__(self, name, skey, keep, pkw, target, start=-1, vel=None, pose=None, blank_from=None, own_frames=False):
        self.name, self.skey, self.keep, self.pkw, self.target = name, skey, None if keep is None else np.asarray(keep, np.int64), tuple(pkw), dict(target)
        self.start, self.vel, self.pose, self.blank_from = start, vel, pose, blank_from
        self.own_frames = own_frames                        # the frames are rendered at the case's start pose, not taken from the scene's path
        self._map, self._frames = None, {}

    @property
    def size(self):
        return self.skey[0], self.skey[1]

    def map(self):
        if self._map is None:
            m = scene(*self.skey)[1]
            self._map = m if self.keep is None else sub_map(m, self.keep)
        return self._map

    def start_pose(self):
        return scene(*self.skey)[0].pose(self.start) if self.pose is None else np.asarray(self.pose, np.float64)

    def frame(self, t):
        if self.own_frames:
            if t not in self._frames:
                self._frames[t] = scene(*self.skey)[0].render_pose(self.start_pose(), key=t)
            return self._frames[t]
        fr = scene(*self.skey)[2]
        return np.zeros_like(fr[0]) if self.blank_from is not None and t >= self.blank_from else fr[t]

    def params(self, n_streams, patch):
        return _params(self.size[0], self.size[1], n_streams, patch, self.pkw)

    def oracle(self, patch):
        o = make_oracle(self.params(1, patch), self.map(), self.start_pose())
        if self.vel is not None:
            o.set_velocity(self.vel)
        return o

    def load(self, g, s):
        g.load_map(s, self.map()); g.set_pose(s, self.start_pose())
        if self.vel is not None:
            g.set_velocity(s, self.vel)


# ---- one oracle frame on the full map: the flags the choices are made from ------------------------------------------------------
@functools.lru_cache(maxsize=None)
def full_frame(skey, patch, pkw, start=-1, vel=None):
    """level (-1: not in the PVS), searched, found of every point after the coarse search (c_*) and entering the fine pose stage, the
    positions the errors are made of, and the per-level counts of both search stages"""
    f, m, frames = scene(*skey)
    o = make_oracle(_params(skey[0], skey[1], 1, patch, pkw), m, f.pose(start))
    if vel is not None:
        o.set_velocity(vel)
    o.frame_begin(frames[0]); o.search_stage(0)
    c = o.point_tracks()
    o.pose_stage(0); o.search_stage(1)
    t = o.point_tracks()
    o.close()
    return {"level": t["level"], "searched": t["searched"], "found": t["found"], "vfound": t["vfound"], "image": t["image"],
            "c_searched": c["searched"], "c_found": c["found"]}


ALL_SELECTED = (("coarse_disabled", 1), ("max_patches_per_frame", 100000)) + NO_KF     # every PVS point is searched, none twice


def fine_flags(skey, patch):
    return full_frame(skey, patch, ALL_SELECTED)


def _shuffled(idx, seed):
    return np.random.default_rng(seed).permutation(idx)


def choose_found(fl, nf, n_unfound, seed=0):
    """nf points whose patch the oracle finds and n_unfound it searches and does not find, spread over the map"""
    ok = fl["searched"] == 1
    F, U = np.flatnonzero(ok & (fl["found"] == 1)), np.flatnonzero(ok & (fl["found"] == 0))
    assert len(F) >= nf and len(U) >= n_unfound, (len(F), nf, len(U), n_unfound)
    return np.sort(np.r_[_shuffled(F, seed)[:nf], _shuffled(U, seed + 1)[:n_unfound]])


def choose_levels(fl, per_level, n_outside=0, seed=0, first=False):
    """per_level[l] searched points of the PVS at level l and n_outside points outside the PVS (first: the first in map order)"""
    parts = []
    for l, k in enumerate(per_level):
        idx = np.flatnonzero((fl["searched"] == 1) & (fl["level"] == l))
        assert len(idx) >= k, (l, len(idx), k)
        parts.append((idx if first else _shuffled(idx, seed + l))[:k])
    out = np.flatnonzero(fl["level"] < 0)
    assert len(out) >= n_outside
    parts.append(_shuffled(out, seed + 9)[:n_outside])
    return np.sort(np.concatenate(parts))


def choose_searched(fl, n_search, n_outside, seed=0):
    idx, out = np.flatnonzero(fl["searched"] == 1), np.flatnonzero(fl["level"] < 0)
    assert len(idx) >= n_search and len(out) >= n_outside
    return np.sort(np.r_[_shuffled(idx, seed)[:n_search], _shuffled(out, seed + 1)[:n_outside]])


def squared_errors(tr):
    """the squared errors entering FindSigmaSquared in the first fine iteration, of the found points in map order (jni/Tracker.cc:707)"""
    f = (tr["level"] >= 0) & (tr["found"] == 1)
    e = (tr["vfound"][f] - tr["image"][f]) * (1.0 / (1 << tr["level"][f]))[:, None]
    return e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]


# ---- (a) nf sweep, (b) median ties ----------------------------------------------------------------------------------------------
A_SCENE = (W, H, 1234, DENSE)
NO_COARSE = (("coarse_disabled", 1),) + NO_KF


@functools.lru_cache(maxsize=None)
def nf_cases(patch):
    fl = fine_flags(A_SCENE, patch)
    out = []
    for k, nf in enumerate(NF_TARGETS):
        nu = 12 if nf == 0 else 2 + nf // 16                     # nf == 0: every point is searched and none is found (not an empty map)
        keep = choose_found(fl, nf, nu, seed=k)
        out.append(Case("nf=%d" % nf, A_SCENE, keep, NO_COARSE, dict(n_points=nf + nu, nf=nf, did_coarse=0, attempted_sum=nf + nu)))
    return out


@functools.lru_cache(maxsize=None)
def tie_case(patch, n_base=41):
    """n_base = 41: nf = 43; n_base = 301: nf = 303, more than one pass of block_radix_select's 256 threads.  Squared errors are doubles made of a projection: two points never have the same one.  A point given three times does -- the copies
    are searched independently and end on the same corner with the same bits -- so the sub-map holds the point at the median rank
    three times: level-0 patches at integer corner positions, equal values at ranks nf/2 - 1, nf/2, nf/2 + 1."""
    fl = fine_flags(A_SCENE, patch)
    F0 = _shuffled(np.flatnonzero((fl["searched"] == 1) & (fl["found"] == 1) & (fl["level"] == 0)), 5)[:n_base]
    e = (fl["vfound"][F0] - fl["image"][F0])
    mid = F0[np.argsort((e * e).sum(1), kind="stable")[n_base // 2]]
    keep = np.sort(np.r_[F0, mid, mid])
    return Case("median tie, nf=%d" % (n_base + 2), A_SCENE, keep, NO_COARSE, dict(n_points=n_base + 2, nf=n_base + 2, did_coarse=0, attempted=[n_base + 2, 0, 0, 0]))


TIE_BASES = (41, 301)


def tie_run(e2):
    """how many values of e2 equal the one at rank n / 2, and whether the run covers the ranks on both sides of it"""
    s = np.sort(e2)
    r = len(s) // 2
    return int((s == s[r]).sum()), bool(r >= 1 and r + 1 < len(s) and s[r - 1] == s[r] == s[r + 1])


# ---- (c) n_points / n_search --------------------------------------------------------------------------------------------------
C_SCENE = (W, H, 77, SPARSE)
FULL_SCENE = (W, H, 1234, DENSE, 14)                       # 14 source keyframes: more than 4096 points


@functools.lru_cache(maxsize=None)
def n_search_cases(patch):
    fl = fine_flags(C_SCENE, patch)
    return [Case("n_search=%d" % n, C_SCENE, choose_searched(fl, n, 3, seed=k), NO_COARSE, dict(n_points=n + 3, attempted_sum=n, did_coarse=0))
            for k, n in enumerate(N_SEARCH_TARGETS[patch])]


def _tilted(pose12, angle):
    """the camera turned by `angle` about its own x axis"""
    c, s = np.cos(angle), np.sin(angle)
    Rx = np.array([[1, 0, 0], [0, c, -s], [0, s, c]])
    R, t = np.asarray(pose12[:9]).reshape(3, 3), np.asarray(pose12[9:])
    return np.r_[(Rx @ R).ravel(), Rx @ t]


def row_kinds(case, patch):
    """what k_pvs writes per point of the case's first frame: 3 doubles (behind the camera or beyond the largest radius), 5 (projected,
    outside the image) or 13 (in the image), from the start pose (no velocity) and the oracle's camera"""
    w, h = case.size
    vp = case.params(1, patch)
    cam5 = list(vp.cam[:])
    lr = orc.cam_project(cam5, w, h, 0.0, 0.0)[3]
    p = case.start_pose()
    R, t = p[:9].reshape(3, 3), p[9:]
    kinds = []
    for q in case.map()["points"]:
        c = R @ q["pos"] + t
        if c[2] < 0.001 or (c[0] / c[2]) ** 2 + (c[1] / c[2]) ** 2 > lr * lr:
            kinds.append(3); continue
        im, _d, inv, _lr = orc.cam_project(cam5, w, h, c[0] / c[2], c[1] / c[2])
        kinds.append(5 if inv or im[0] < 0 or im[1] < 0 or im[0] > w or im[1] > h else 13)
    return np.array(kinds)


@functools.lru_cache(maxsize=None)
def mixed_block_case(patch, n=200):
    """the first n points of the map seen from a start pose turned until part of the map is behind the camera, part projects outside the
    image and part is in view: 3-, 5- and 13-double rows in one LDS block of k_pvs"""
    f = scene(*C_SCENE)[0]
    best = None
    for deg in range(20, 85, 5):
        c = Case("mixed block", C_SCENE, np.arange(n), NO_COARSE, {}, pose=_tilted(f.pose(-1), np.radians(deg)))
        k = row_kinds(c, patch)
        score = min((k == 3).sum(), (k == 5).sum(), (k == 13).sum())
        if best is None or score > best[0]:
            best = (score, c, k)
    _score, c, k = best
    c.target = dict(n_points=n, did_coarse=0, rows=[int((k == v).sum()) for v in (3, 5, 13)])
    return c


@functools.lru_cache(maxsize=None)
def n_points_cases(patch):
    fl = fine_flags(C_SCENE, patch)
    n_all = len(fl["level"])
    out = []
    for k, n in enumerate(N_POINTS_TARGETS):
        keep = choose_searched(fl, 1, 0) if n == 1 else np.sort(_shuffled(np.arange(n_all), 20 + k)[:n])
        out.append(Case("n_points=%d" % n, C_SCENE, keep, NO_COARSE, dict(n_points=n, did_coarse=0, attempted_sum=int((fl["searched"][keep] == 1).sum()))))
    per = [20, 0, 10, 4]
    out.append(Case("empty level 1", C_SCENE, choose_levels(fl, per, 5), NO_COARSE, dict(n_points=sum(per) + 5, attempted=per, did_coarse=0)))
    out.append(mixed_block_case(patch))
    return out


@functools.lru_cache(maxsize=None)
def full_capacity_case(patch):
    return Case("n_points=4096", FULL_SCENE, np.arange(4096), NO_KF, dict(n_points=4096, did_coarse=0))


# ---- (d) a 17-stream batch with idle streams ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def loss_batch(patch):
    """17 streams: None = no map, a case with blank_from = a stream that loses tracking, the rest small mapped streams"""
    fl = fine_flags(C_SCENE, patch)
    out = []
    for s in range(LOSS_STREAMS):
        kind = LOSS_IDLE.get(s)
        if kind == "no map":
            out.append(None); continue
        keep = choose_found(fl, 60 + s, 4, seed=40 + s)
        out.append(Case("stream %d%s" % (s, " (lost)" if kind else ""), C_SCENE, keep, NO_KF, dict(n_points=64 + s), blank_from=2 if kind else None))
    return out


# ---- (e) selection edges of k_plan -------------------------------------------------------------------------------------------
E_SCENE = FULL_SCENE
COARSE_MIN, COARSE_MAX, FINE_MAX = 4, 12, 40
E_COARSE = (("coarse_min", COARSE_MIN), ("coarse_max", COARSE_MAX), ("coarse_min_vel", 0.0)) + NO_KF
E_FINE = E_COARSE + (("max_patches_per_frame", FINE_MAX),)


def plan(n, coarse_min=COARSE_MIN, coarse_max=COARSE_MAX, max_patches=1000):
    """jni/Tracker.cc:437-461, 493-535 on the PVS counts n[level]: (coarse level 3, coarse level 2, fine level 3, fine others)"""
    n0, n1, n2, n3 = n
    c3 = c2 = h3 = h2 = 0
    if n3 + n2 > coarse_min:
        h3 = c3 = min(n3, coarse_max)
        if c3 < coarse_max:
            more = coarse_max - c3
            if n2 <= more:
                c3, c2, h2 = 0, n2, n2                      # :454-456 replaces the level-3 selection
            else:
                c2 = h2 = more
    f3 = n3 - h3
    fine = max(0, max_patches - (c3 + c2 + f3))
    return c3, c2, f3, min(fine, (n2 - h2) + n1 + n0)


def _with(pkw, **kw):
    return tuple(x for x in pkw if x[0] not in kw) + tuple(sorted(kw.items()))


def _e_flags(patch):
    """the levels at the fast-moving start, and the coarse search's verdict on every level-2 point (coarse_max so large that the kept
    bug selects level 2 alone) and on every level-3 point (coarse_max = n3 + 1: all of level 3 and one level-2 point)"""
    lv = full_frame(E_SCENE, patch, E_COARSE, start=-6, vel=FAST_VEL)
    c2 = full_frame(E_SCENE, patch, _with(E_COARSE, coarse_max=100000), start=-6, vel=FAST_VEL)
    c3 = full_frame(E_SCENE, patch, _with(E_COARSE, coarse_max=int((lv["level"] == 3).sum()) + 1), start=-6, vel=FAST_VEL)
    return lv, c2, c3


def _e_case(name, patch, n, pkw, extra=None, unfound2=0):
    lv, c2, c3 = _e_flags(patch)
    parts = []
    for l, k in enumerate(n):                                  # levels 2 and 3: the points the coarse search finds first, so that the coarse
        idx = np.flatnonzero((lv["searched"] == 1) & (lv["level"] == l))      # pose stage has its coarse_min patches; then map order
        if l >= 2:
            cf = (c2 if l == 2 else c3)
            idx = idx[np.argsort(~((cf["c_searched"][idx] == 1) & (cf["c_found"][idx] == 1)), kind="stable")]
        assert len(idx) >= k, (l, len(idx), k)
        parts.append(idx[:k])
    keep = np.concatenate(parts)                               # not sorted: the sub-map's order, which the selection follows, is found first
    if unfound2:                                               # the level-2 points are ones the coarse search does not find
        idx2 = np.flatnonzero((lv["level"] == 2) & (c2["c_searched"] == 1))
        U, F = idx2[c2["c_found"][idx2] == 0], idx2[c2["c_found"][idx2] == 1]
        assert len(U) >= unfound2 and len(F) >= n[2] - unfound2, (len(U), len(F))
        keep = np.r_[keep[lv["level"][keep] != 2], U[:unfound2], F[:n[2] - unfound2]]
    mp = dict(pkw).get("max_patches_per_frame", 1000)
    c3, c2n, f3, fo = plan(n, max_patches=mp)
    t = dict(n_points=sum(n), coarse_attempted=[0, 0, c2n, c3], attempted_sum=c3 + c2n + f3 + fo, plan=(c3, c2n, f3, fo))
    t.update(extra or {})
    return Case(name, E_SCENE, keep, pkw, t, start=-6, vel=FAST_VEL)


@functools.lru_cache(maxsize=None)
def coarse_edge_cases(patch):
    M, X = COARSE_MIN, COARSE_MAX
    return [
        _e_case("n3+n2 == coarse_min", patch, (10, 10, 2, M - 2), E_COARSE, dict(did_coarse=0)),
        _e_case("n3+n2 == coarse_min+1", patch, (10, 10, M + 1, 0), E_COARSE, dict(did_coarse=1)),      # n2 <= more: level 2 alone, so it holds the coarse_min found
        _e_case("n3 == coarse_max-1", patch, (10, 10, 30, X - 1), E_COARSE, dict(did_coarse=1)),
        _e_case("n3 == coarse_max", patch, (10, 10, 30, X), E_COARSE, dict(did_coarse=1)),
        _e_case("n3 == coarse_max+1", patch, (10, 10, 30, X + 1), E_COARSE, dict(did_coarse=1)),
        _e_case("n2 == more (level 2 only)", patch, (10, 10, X - 5, 5), E_COARSE, dict(did_coarse=1)),
        _e_case("n2 == more+1", patch, (10, 10, X - 5 + 1, 5), E_COARSE, dict(did_coarse=1)),
        _e_case("coarse found < coarse_min", patch, (10, 10, 6, 2), E_COARSE, dict(did_coarse=0), unfound2=3),
    ]


@functools.lru_cache(maxsize=None)
def fine_edge_cases(patch):
    X, F = COARSE_MAX, FINE_MAX
    return [
        _e_case("nit+n3 > max_patches", patch, (10, 10, 10, F + 1), E_FINE, dict(did_coarse=1)),
        _e_case("nit+n3 == max_patches", patch, (10, 10, 10, F), E_FINE, dict(did_coarse=1)),
        _e_case("nother == nFine+1", patch, (7, 7, 7, X + 8), E_FINE, dict(did_coarse=1)),
        _e_case("nother == nFine-1", patch, (7, 6, 6, X + 8), E_FINE, dict(did_coarse=1)),
    ]


# ---- (f) search-window and sub-pixel edges --------------------------------------------------------------------------------------
F_COARSE_MAX = 140                                          # more coarse patches than one k_subpixN pass covers (16 workgroups x 8)
F_MANY = _with(E_COARSE, coarse_max=F_COARSE_MAX)
SMALL_SIZES = ((48, 48), (131, 77))
WINDOW_EDGES = {(48, 48): ("bottom", "border"), (131, 77): ("bottom", "empty", "border")}     # what window_edges must count at each size


SUBPIX_GRID_BLOCKS = 16                                     # k_subpixN's grid per stream: one pass covers 16 x PATCHES_PER_WAVE entries
LEVEL3_ZOOMS = (4.0, 7.5)                                   # 48x48: level-1 and level-0 source points seen this much closer are searched at level 3
EXIT_SIZE = (163, 117)                                      # level 3 is 20x14: the rows a patch fits in are mostly rows the sub-pixel border excludes
EXIT_ZOOMS = (3.6, 4.0, 4.5, 5.0, 5.5, 6.0, 3.2)


@functools.lru_cache(maxsize=None)
def many_coarse_case(patch):
    return Case("n_coarse > 128", A_SCENE, None, F_MANY, dict(n_coarse_min=129, did_coarse=1), start=-6, vel=FAST_VEL)


def second_pass_refined(coarse_tracks, patch):
    """how many coarse patches beyond k_subpixN's first pass are found and sub-pixel refined.  The coarse list is the level-3 selection
    followed by the level-2 one, each in map order (jni/Tracker.cc:441-461); a point whose template is bad holds an entry without being
    searched, so the rank among the searched points is a lower bound of the entry number."""
    tr = coarse_tracks
    idx = np.flatnonzero(tr["searched"] == 1)
    order = idx[np.argsort(-tr["level"][idx], kind="stable")]
    late = order[SUBPIX_GRID_BLOCKS * PATCHES_PER_WAVE[patch]:]
    return int(((tr["found"][late] == 1) & (tr["subpix"][late] == 1)).sum())


def _zoomed(pose12, z):
    """the camera moved along its optical axis to 1 / z of its distance from the plane z = 0 of the feeder's scene"""
    R, t = np.asarray(pose12[:9]).reshape(3, 3), np.asarray(pose12[9:])
    C, d = -R.T @ t, R[2]
    C2 = C + (1.0 - 1.0 / z) * (-C[2] / d[2]) * d
    return np.r_[R.ravel(), -R @ C2]


@functools.lru_cache(maxsize=None)
def level3_cases(patch, w=48, h=48):
    """48x48 seen from closer, so that the warp puts map points at level 3 (6x6 pixels): the patches are attempted there, no 8x8 or 11x11
    patch fits, none is found.  attempted is what the oracle gives at this pose; test_tracker_cases.py asserts attempted[3] > 0 = found[3]."""
    skey = (w, h, 1234, SPARSE)
    out = []
    for z in LEVEL3_ZOOMS:
        c = Case("%dx%d, %.1fx closer" % (w, h, z), skey, None, NO_COARSE, dict(did_coarse=0, level3_unfound=True),
                 pose=_zoomed(scene(*skey)[0].pose(-1), z), own_frames=True)
        out.append(c)
    return out


def subpix_exits(case, patch):
    """the points of the case's first frame that the search finds and the sub-pixel refinement un-finds: found with a sub-pixel budget of 0
    (the oracle then reports the corner), searched and not found with the budget.  Returns their indices and, of these, the ones whose
    corner lies half a patch from a border of its level -- ZMSSDAtPoint takes it (jni/PatchFinder.cc:356), IterateSubPix's border is
    one pixel wider (:300) and the first iteration leaves the image."""
    def tracks(c):
        o = c.oracle(patch)
        o.frame_begin(c.frame(0)); o.search_stage(0); o.pose_stage(0); o.search_stage(1)
        tr = o.point_tracks()
        o.close()
        return tr
    plain = Case(case.name, case.skey, case.keep, _with(case.pkw, fine_subpix_its=0, coarse_subpix_its=0), {}, start=case.start, vel=case.vel, pose=case.pose, own_frames=case.own_frames)
    a, b = tracks(plain), tracks(case)
    gone = np.flatnonzero((a["found"] == 1) & (a["level"] >= 0) & (b["level"] == a["level"]) & (b["searched"] == 1) & (b["subpix"] == 1) & (b["found"] == 0))
    w, h = case.size
    at_border = []
    for i in gone:
        l = int(a["level"][i]); sc = 1 << l
        cx, cy = (a["vfound"][i] + 0.5) / sc - 0.5                 # LevelNPos of the corner
        bd = patch // 2 + 1
        if not (cx >= bd and cy >= bd and cx < (w >> l) - bd and cy < (h >> l) - bd):
            at_border.append(int(i))
    return gone, np.array(at_border, np.int64)


@functools.lru_cache(maxsize=None)
def subpix_exit_case(patch):
    """a 163x117 frame seen from closer (the first zoom of EXIT_ZOOMS at which the oracle un-finds a patch at a border): level-3 patches
    next to the border, with the fine stage's sub-pixel iterations"""
    skey = EXIT_SIZE + (1234, SPARSE)
    for z in EXIT_ZOOMS:
        c = Case("%dx%d, %.1fx closer" % (EXIT_SIZE + (z,)), skey, None, NO_COARSE, dict(did_coarse=0),
                 pose=_zoomed(scene(*skey)[0].pose(-1), z), own_frames=True)
        gone, at_border = subpix_exits(c, patch)
        if len(at_border):
            c.target["n_exits"] = len(at_border)
            return c
    raise AssertionError("no zoom of EXIT_ZOOMS gives a refinement that leaves the image")


@functools.lru_cache(maxsize=None)
def small_size_case(patch, w, h):
    return Case("%dx%d" % (w, h), (w, h, 1234, SPARSE), None, NO_COARSE, dict(did_coarse=0))


def window_edges(case, patch):
    """of the searches of the case's first frame, counted by the oracle inside FindPatchCoarse (jni/PatchFinder.cc:170-235): the windows
    that reach the bottom row of their level, that hold no corner that passes the range test, and that hold a candidate closer than
    half a patch to an image border"""
    o = case.oracle(patch)
    o.frame_begin(case.frame(0)); o.search_stage(0); o.pose_stage(0); o.search_stage(1)
    n = o.window_counts()
    o.close()
    return n


# ---- the groups: each is the streams of one System ------------------------------------------------------------------------------
def groups(patch):
    a = nf_cases(patch)
    g = {"a: nf sweep, 9 streams": a[:9], "a: nf sweep, 17 streams": a[9:26], "a+b: nf=513 and the median tie": [a[26]] + [tie_case(patch, n) for n in TIE_BASES],
         "c: n_search sweep, 8 streams": n_search_cases(patch), "c: n_points sweep, 7 streams": n_points_cases(patch),
         "c: full capacity": [full_capacity_case(patch)],
         "e: coarse selection": coarse_edge_cases(patch), "e: fine selection": fine_edge_cases(patch),
         "f: two sub-pixel passes": [many_coarse_case(patch)], "f: sub-pixel exit": [subpix_exit_case(patch)]}
    for w, h in SMALL_SIZES:
        g["f: %dx%d" % (w, h)] = [small_size_case(patch, w, h)] + (level3_cases(patch) if (w, h) == (48, 48) else [])
    return g


GROUP_NAMES = ("a: nf sweep, 9 streams", "a: nf sweep, 17 streams", "a+b: nf=513 and the median tie", "c: n_search sweep, 8 streams", "c: n_points sweep, 7 streams",
               "c: full capacity", "e: coarse selection", "e: fine selection", "f: two sub-pixel passes", "f: sub-pixel exit") + tuple("f: %dx%d" % s for s in SMALL_SIZES)


def stage_record(o):
    """what a case's targets are checked against, from an oracle that has just run a search or pose stage"""
    st, tr = o.state(), o.point_tracks()
    return {"n_points": st.n_points, "attempted": list(st.attempted), "found_counts": list(st.found), "did_coarse": st.did_coarse,
            "nf": int(((tr["level"] >= 0) & (tr["found"] == 1)).sum()), "tracks": tr}
