"""InitFromStereo cases with chosen exits and counts, shared by tests/test_stereo_cases.py (CPU: the oracle alone, in shared-stage mode,
reaches every named condition) and tests/test_gpu_init_from_stereo.py (GPU: the device == that oracle on every case, bit for bit).  No GPU
is touched here and nothing comes from the device.

MapMaker::InitFromStereo (jni/MapMaker.cc:204-376) past the homography: the point loop (csrc/boot.hip k_boot_points, BOOT_WAVES = 4 matches
per round of the workgroup), the five + until-converged adjustments, the scene depths, AddSomeMapPoints, CalcPlaneAligner +
ApplyGlobalTransformationToMap.  The feeder sequences of tests/test_gpu_bootstrap.py lead about 200 matches through it of which one or two
fail the sub-pixel step: no template at a border, no point behind the camera, no failed initialisation, never fewer than ten points.

A case is two frames, a match list, the three frames that follow and the boot seed.  The starting point is the feeder at 160 x 120 (320 x 240
for one case) and the oracle's own trails after twelve frames; the cases cut and extend that list and, where stated, edit the frames:

  A  residues        the list cut to 4k, 4k + 1, 4k + 2, 4k + 3 entries; and 4k + 1 where the last round's only live match fails
  B  template border first positions at half, half + 1, half + 2 from each border of the first image (half = patch / 2), at the start, in
                     the middle and at the end of the list; the second positions follow the flow of the nearest trail
  C  sub-pixel       (flat) the second positions of some matches lie in a rectangle of the second frame painted flat: ten iterations, no
                     convergence; (border) second positions inside the sub-pixel border of the second image: the first iteration leaves
  D  behind          a block of the first frame pasted into the second, displaced against the flow: the triangulation gives z < 0
  E  return false    (i) 0, 3 and 9 matches; (ii) the second image is the first and every match is (x, y, x, y)
  F  under ten       both frames faded out except in discs around a dozen matches, half of which lose their disc in the second frame
  G  a mixed batch   five streams through the spacebar path (mixed_batch())

run(case, shared) gives the oracle after the call."""
import functools

import numpy as np

import oracle.binding as orc
from helpers import make_scene
from visualslam_android_amd import capi, feeder

WAVES = 4                                # BOOT_WAVES: matches per round of k_boot_points
PATCHES = (8, 11)
SIZE = (160, 120)
BIG = (320, 240)
N_TRAIL_FRAMES = 12
N_FOLLOW = 3
BOOT_SEED = 3
BIG_SEED = 4                             # (at seed 3 ChooseBestDecomposition keeps the mirrored pose: the second 320 x 240 case)
DEVICE_KW = dict(bootstrap=1, ba_sum_order=1)
CODE_POINT, CODE_BORDER, CODE_SUBPIX, CODE_BEHIND = range(4)
EXIT_NONE, EXIT_HOMOGRAPHY, EXIT_ZERO_TRANSLATION, EXIT_HOST_NOT_OK = range(4)


def half(patch):
    return patch // 2


def params(w, h, patch, n_streams=1, **kw):
    return capi.default_params(w, h, n_streams, patch_size=patch, grow_map=3, **kw)


@functools.lru_cache(maxsize=None)
def base(patch, size=SIZE, seed=5):
    """-> (frames of the feeder, the oracle's trails between frame 0 and frame N_TRAIL_FRAMES - 1 as (n, 4) int32)"""
    w, h = size
    frames = feeder.Feeder(w, h, seed=seed, noise=2).render(0, N_TRAIL_FRAMES + N_FOLLOW)
    o = orc.OracleSystem(orc.params_from_vslam(params(w, h, patch)))
    o.press_spacebar()
    for t in range(N_TRAIL_FRAMES):
        o.track_frame(frames[t])
    m = o.trails().copy()
    o.close()
    assert len(m) > 100
    return frames, m


class Case:
    def __init__(self, name, patch, first, second, matches, follow, seed=BOOT_SEED, **want):
        self.name, self.patch, self.seed = name, patch, seed
        self.first, self.second = np.ascontiguousarray(first, np.uint8), np.ascontiguousarray(second, np.uint8)
        self.matches = np.ascontiguousarray(matches, np.int32).reshape(-1, 4)
        self.follow = [np.ascontiguousarray(f, np.uint8) for f in follow]
        self.h, self.w = self.first.shape
        self.want = want                 # what tests/test_stereo_cases.py asserts of the oracle on this case
        assert len(self.matches) <= 1000 and self.second.shape == self.first.shape

    def params(self, **kw):
        return params(self.w, self.h, self.patch, **kw)

    def oracle(self, shared=True):
        o = orc.OracleSystem(orc.params_from_vslam(self.params()))
        o.set_boot_seed(self.seed)
        o.set_shared_stages(shared)
        return o


def run(case, shared=True):
    """-> (the oracle after InitFromStereo on the case, its return value)"""
    o = case.oracle(shared)
    ok, _ = o.init_from_stereo(case.first, case.second, case.matches)
    return o, ok


def _case(name, patch, matches, second=None, first=None, size=SIZE, seed=BOOT_SEED, **want):
    frames, _ = base(patch, size)
    return Case(name, patch, frames[0] if first is None else first, frames[N_TRAIL_FRAMES - 1] if second is None else second, matches,
                frames[N_TRAIL_FRAMES:N_TRAIL_FRAMES + N_FOLLOW], seed=seed, **want)


def flow_at(m, x, y):
    """the displacement of the match whose first position is nearest to (x, y)"""
    i = int(np.argmin((m[:, 0] - x) ** 2 + (m[:, 1] - y) ** 2))
    return int(m[i, 2] - m[i, 0]), int(m[i, 3] - m[i, 1])


# ---- A ------------------------------------------------------------------------------------------------------------------------------
def border_match(patch, m, w, h):
    """a match whose template does not keep the border: the first position `half` from the left border"""
    y = h // 2
    dx, dy = flow_at(m, half(patch), y)
    return [half(patch), y, half(patch) + dx, y + dy]


def residue_cases(patch):
    _, m = base(patch)
    k = 10
    out = [_case("A: %d matches" % (WAVES * k + r), patch, m[:WAVES * k + r], n=WAVES * k + r) for r in range(WAVES)]
    # the last round's only live match fails, after a round whose first wavefront made a point: its result slot has to be cleared
    lone = np.r_[m[:WAVES * k], [border_match(patch, m, *SIZE)]]
    out.append(_case("A: %d matches, the last alone and failing" % len(lone), patch, lone, n=WAVES * k + 1, lone_failure=True))
    return out


# ---- B ------------------------------------------------------------------------------------------------------------------------------
def border_matches(patch, m, w, h):
    """-> [(match, distance from its border - half)]: three distances from each of the four borders, left, top, right, bottom"""
    out = []
    for side in range(4):
        for d in (0, 1, 2):
            q = half(patch) + d
            x, y = ((q, h // 2 + 7 * d), (w // 2 + 7 * d, q), (w - 1 - q, h // 2 - 7 * d), (w // 2 - 7 * d, h - 1 - q))[side]
            dx, dy = flow_at(m, x, y)
            out.append(([x, y, x + dx, y + dy], d))
    return out


def border_case(patch):
    _, m = base(patch)
    m = m[:61]                                                         # 61 + 12 = 73 matches: a last round of one
    bm = border_matches(patch, m, *SIZE)
    rows = [q for q, _ in bm]
    at = {0: rows[0:4], len(m) // 2: rows[4:8], len(m): rows[8:12]}     # before the first, in the middle, behind the last
    out, where = [], []
    for i in range(len(m) + 1):
        for q in at.get(i, ()):
            where.append(len(out)); out.append(q)                      # (in bm's order)
        if i < len(m):
            out.append(list(m[i]))
    return _case("B: template border", patch, out, border_rows=where, border_dist=[d for _, d in bm])


# ---- C ------------------------------------------------------------------------------------------------------------------------------
FLAT = (52, 36, 108, 84)                 # x0, y0, x1, y1 of the rectangle of the second frame painted flat


def subpix_cases(patch):
    frames, m = base(patch)
    second = frames[N_TRAIL_FRAMES - 1].copy()
    x0, y0, x1, y1 = FLAT
    second[y0:y1, x0:x1] = 100
    b = half(patch) + 1 + patch                                        # room for ten updates of the sub-pixel position
    inside = (m[:, 2] >= x0 + b) & (m[:, 2] < x1 - b) & (m[:, 3] >= y0 + b) & (m[:, 3] < y1 - b)
    flat = _case("C: second positions in flat image", patch, m, second=second, flat_rows=np.flatnonzero(inside).tolist())
    # inside the sub-pixel border of the second image (half + 1 wide), the template still good: left, top, right, bottom
    w, h = SIZE
    hb = half(patch)
    edge = [[hb + 1, h // 2, hb, h // 2], [w // 2, hb + 1, w // 2, hb], [w - hb - 2, h // 2, w - hb - 1, h // 2], [w // 2, h - hb - 2, w // 2, h - hb - 1]]
    mm = np.r_[edge[:2], m[:70], edge[2:]]
    border = _case("C: second positions in the sub-pixel border", patch, mm, edge_rows=[0, 1, len(mm) - 2, len(mm) - 1])
    return [flat, border]


# ---- D ------------------------------------------------------------------------------------------------------------------------------
DISPLACEMENTS = (-2.0, -3.0, -4.0, -6.0, 2.0, 3.0)                     # multiples of the local flow tried, in this order
BLOCK = 12                               # half the side of the pasted block


def behind_candidates(patch):
    """the pasted-block cases for every displacement of DISPLACEMENTS; the CPU test keeps the first that reaches code 3"""
    frames, m = base(patch)
    w, h = SIZE
    i = int(np.argmin((m[:, 0] - w // 2) ** 2 + (m[:, 1] - h // 2) ** 2))   # the trail nearest to the centre
    cx, cy = int(m[i, 0]), int(m[i, 1])
    dx, dy = int(m[i, 2]) - cx, int(m[i, 3]) - cy
    out = []
    for k in DISPLACEMENTS:
        ex, ey = cx + int(round(k * dx)), cy + int(round(k * dy))
        if not (BLOCK <= ex < w - BLOCK and BLOCK <= ey < h - BLOCK and BLOCK <= cx < w - BLOCK and BLOCK <= cy < h - BLOCK):
            continue
        second = frames[N_TRAIL_FRAMES - 1].copy()
        second[ey - BLOCK:ey + BLOCK + 1, ex - BLOCK:ex + BLOCK + 1] = frames[0][cy - BLOCK:cy + BLOCK + 1, cx - BLOCK:cx + BLOCK + 1]
        far = (np.abs(m[:, 2] - ex) > BLOCK + patch) | (np.abs(m[:, 3] - ey) > BLOCK + patch)      # the trails the block does not cover
        mm = np.r_[m[far][:50], [[cx, cy, ex, ey]], m[far][50:]]
        out.append(_case("D: block displaced by %g x the flow" % k, patch, mm, second=second, behind_row=50))
    return out


@functools.lru_cache(maxsize=None)
def behind_case(patch):
    """the first displacement whose match is triangulated behind the camera (None if the set holds none: the CPU test fails then)"""
    for c in behind_candidates(patch):
        o, ok = run(c)
        code = o.boot_log()["code"]
        o.close()
        if ok and code[c.want["behind_row"]] == CODE_BEHIND:
            return c
    return None


# ---- E ------------------------------------------------------------------------------------------------------------------------------
STILL_SEED_FAILS, STILL_SEED_PASSES = 1, 3


def failing_cases(patch):
    frames, m = base(patch)
    out = [_case("E-i: %d matches" % n, patch, m[:n], few=n) for n in (0, 3, 9)]
    still = np.c_[m[:, :2], m[:, :2]]
    # The homography of a zero baseline is the identity up to rounding: whether its three singular values come out distinct (:286-296) hangs
    # on the last bits, so on the draws.  STILL_SEED_FAILS is a seed at which the host pipeline says ok = 0, STILL_SEED_PASSES one at which
    # it decomposes the rounding (the call goes through, with points behind the camera and adjustments that do not converge in fifty).
    out.append(_case("E-ii: zero baseline", patch, still, second=frames[0], seed=STILL_SEED_FAILS, zero_baseline=True))
    out.append(_case("E-ii: zero baseline, a seed at which the rounding decomposes", patch, still, second=frames[0], seed=STILL_SEED_PASSES, zero_baseline_passes=True))
    return out


# ---- F ------------------------------------------------------------------------------------------------------------------------------
N_DISCS, N_KEPT, RADIUS = 12, 6, 6
CONTRAST = 0.15                          # of the texture inside the discs


RAMP = 5                                 # pixels over which a disc's texture fades into the flat image (a hard edge would be a ring of corners)


def faded(img, centres, radius, grey=110, contrast=1.0):
    """the image flat except inside the discs, where the texture keeps `contrast` of its amplitude"""
    h, w = img.shape
    yy, xx = np.mgrid[0:h, 0:w]
    alpha = np.zeros((h, w))
    for x, y in centres:
        alpha = np.maximum(alpha, np.clip((radius + RAMP - np.sqrt((xx - x) ** 2 + (yy - y) ** 2)) / RAMP, 0.0, 1.0))
    return np.round(grey + (img.astype(np.float64) - grey) * alpha * contrast).astype(np.uint8)


def few_points_case(patch):
    frames, m = base(patch)
    w, h = SIZE
    rng = np.random.RandomState(11)
    r = RADIUS + half(patch) + RAMP                                    # the discs' radius and a pixel between them
    pool = [i for i in rng.permutation(len(m)) if r <= m[i, 0] < w - r and r <= m[i, 1] < h - r and r <= m[i, 2] < w - r and r <= m[i, 3] < h - r]
    pick = []
    for i in pool:                                                     # apart, so that a match that loses its disc is not inside a neighbour's
        if all((m[i, 0] - m[j, 0]) ** 2 + (m[i, 1] - m[j, 1]) ** 2 > (2 * RADIUS + patch) ** 2 for j in pick):
            pick.append(i)
        if len(pick) == N_DISCS:
            break
    assert len(pick) == N_DISCS
    pick = sorted(pick)
    kept = pick[::2][:N_KEPT]                                          # every other match keeps its disc in the second frame
    first = faded(frames[0], [(m[i, 0], m[i, 1]) for i in pick], RADIUS + half(patch), contrast=CONTRAST)
    second = faded(frames[N_TRAIL_FRAMES - 1], [(m[i, 2], m[i, 3]) for i in kept], RADIUS + half(patch), contrast=CONTRAST)
    return _case("F: fewer than ten points", patch, m[pick], first=first, second=second, under_ten=True)


def one_stream_cases(patch):
    """every case that goes through vslam_init_from_stereo, D by the displacement behind_case() found"""
    _, m = base(patch)
    out = [_case("baseline", patch, m, baseline=True)]
    out += residue_cases(patch) + [border_case(patch)] + subpix_cases(patch)
    d = behind_case(patch)
    if d is not None:
        out.append(d)
    out += failing_cases(patch) + [few_points_case(patch)]
    if patch == 8:
        out.append(_case("baseline at 320 x 240", patch, base(patch, BIG)[1], size=BIG, seed=BIG_SEED, baseline=True))
        out.append(_case("D: 320 x 240, the mirrored decomposition", patch, base(patch, BIG)[1], size=BIG, seed=3, many_behind=True))
    return out


# ---- G ------------------------------------------------------------------------------------------------------------------------------
G_PER_LEVEL = (60, 25, 10, 4)
G_FRAMES = N_TRAIL_FRAMES + N_FOLLOW     # frames of the batch; the second presses are consumed in frame N_TRAIL_FRAMES - 1
G_FAIL_SEED = 2
G_ROLES = ("loaded map", "second press succeeds", "second press fails", "first press", "never pressed")


@functools.lru_cache(maxsize=None)
def mixed_scene():
    w, h = SIZE
    return make_scene(w, h, seed=501, n_frames=G_FRAMES, per_level=G_PER_LEVEL)


def mixed_batch(patch):
    """-> list of (role, frames, presses, map scene or None, boot seed) for the five streams.  A press at frame t is made before frame t is
    tracked.  The failing stream sees the same image in every frame up to the second press: its trails do not move, the baseline is zero
    (E-ii), and G_FAIL_SEED is a seed at which the host pipeline says ok = 0 for them."""
    frames, _ = base(patch)
    other = feeder.Feeder(SIZE[0], SIZE[1], seed=9, noise=2).render(0, G_FRAMES)
    t2 = N_TRAIL_FRAMES - 1
    still = [frames[0]] * (t2 + 1) + list(frames[t2 + 1:G_FRAMES])
    sc = mixed_scene()
    return [(G_ROLES[0], list(sc[2][:G_FRAMES]), (), sc, BOOT_SEED),
            (G_ROLES[1], list(frames[:G_FRAMES]), (0, t2), None, BOOT_SEED),
            (G_ROLES[2], still, (0, t2), None, G_FAIL_SEED),
            (G_ROLES[3], list(other), (t2,), None, BOOT_SEED),
            (G_ROLES[4], list(other[::-1]), (), None, BOOT_SEED)]


def mixed_oracle(patch, stream):
    """the oracle of one stream of the batch, in shared-stage mode, before its first frame"""
    from helpers import make_oracle
    role, frames, presses, scene, seed = stream
    vp = params(SIZE[0], SIZE[1], patch)
    o = make_oracle(vp, scene[1], scene[0].pose(-1)) if scene is not None else orc.OracleSystem(orc.params_from_vslam(vp))
    o.set_boot_seed(seed)
    o.set_shared_stages(True)
    return o
