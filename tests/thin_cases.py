"""MapMaker::ThinCandidates (jni/MapMaker.cc:381-422; k_thin_candidates, csrc/frontend.hip) at its edges, shared by
tests/test_thin_cases.py (CPU: the expected survivors, from the oracle and from a plain statement of the rule) and
tests/test_gpu_frame_tail.py (GPU: the device's lists == the oracle's).  No GPU is touched here.

One 320x240 feeder frame (2000 rectangles of texture, so that level 0 holds more than 256 candidates) supplies the Shi-Tomasi
candidates of every level.  A scenario is a map built by hand -- one keyframe whose measurement row is placed relative to chosen
candidates -- and every scenario is one stream of a System that sees the same frame.  A measurement of level m at the level-0 position
root is a busy position rounded(root / 2**l) for the candidates of the levels l = m and l = m - 1; a candidate closer than 10
level-pixels (dx*dx + dy*dy < 100) to a busy position goes.

The targets of the distance and rounding scenarios are ISOLATED by ISOLATION = 12 level-pixels: no other candidate of their level lies
that close to the measurement placed for them, and no two targets of a level are closer than APART = 32, so at its own level a
measurement decides its target alone and a target's fate is its own measurement's doing (test_thin_cases.py re-derives both).  20
level-pixels cannot be had: a 320x240 frame dense enough for 256 level-0 candidates has no candidate that far from all others, and
levels 1 to 3 have none at any density.  The level filter's and the chunk scenarios' targets are not isolated: a measurement on top of a
candidate takes the candidate's neighbours with it, and a measurement of level m also thins level m - 1 around root / 2**(m - 1).
Which candidates go is in the expected lists (both references compute every level), and test_thin_cases.py prints how many."""
import functools

import numpy as np

import oracle.binding as orc
from helpers import make_scene

W, H = 320, 240
ISOLATION = 12
APART = 32                                                   # two targets of a level: no measurement reaches the other's target
CHUNK = 256                                                  # candidates per pass of k_thin_candidates' compaction
MIN_SCORE, BORDER = 70.0, 10
LEVEL_FILTER = ((1, 2, False), (1, 0, True), (1, 3, True), (0, 1, False), (2, 3, False), (2, 1, True))     # candidate's level, measurement's, survives
SCENARIOS = ("distance", "rounding at level 0", "rounding at level 1") + tuple("level filter: candidate of level %d, measurement of level %d" % f[:2] for f in LEVEL_FILTER) + \
            ("every candidate of level 2", "first chunk only", "last chunk only", "every chunk")


@functools.lru_cache(maxsize=None)
def _scene():
    return make_scene(W, H, seed=77, n_frames=1, n_keyframes=2, per_level=(8, 4, 2, 1), rects=2000)


def frame():
    return _scene()[2][0]


@functools.lru_cache(maxsize=None)
def level_candidates():
    """[(packed positions, Shi-Tomasi scores)] per level of the frame, as MakeKeyFrame_Rest leaves them"""
    out = []
    for img, corners, _lut in orc.make_keyframe_lite(frame()):
        keep = orc.nonmax(corners, orc.fast_score(img, corners, 10))
        out.append(orc.candidates(img, keep, MIN_SCORE, BORDER))
    return out


def xy(pos):
    return np.stack([pos & 0xFFFF, pos >> 16], 1).astype(np.int64)


def rule_keep(pos, level, root, mlev):
    """the rule in numpy: the mask of the candidates `pos` of `level` that survive the measurements (root [n, 2], mlev [n])"""
    sel = (mlev == level) | (mlev == level + 1)
    v = root[sel] / (1 << level)
    busy = np.trunc(np.where(v > 0.0, v + 0.5, v - 0.5)).astype(np.int64)                  # rounded(): half away from zero
    d = xy(pos)[:, None, :] - busy[None, :, :]
    return ~((d * d).sum(2) < 100).any(1)


def isolated(level, offset, taken, n, radius=ISOLATION):
    """n candidates of `level` (indices) such that no other candidate of the level lies within `radius` level-pixels of candidate + offset,
    none of them in `taken`, and no two closer than APART"""
    c = xy(level_candidates()[level][0])
    out = []
    for i in range(len(c)):
        m = c[i] + np.asarray(offset)
        d = c - m
        near = np.flatnonzero((d * d).sum(1) < radius * radius)
        if set(near) <= {i} and i not in taken and all(((c[i] - c[j]) ** 2).sum() >= APART * APART for j in list(taken) + out):
            out.append(i)
            if len(out) == n:
                return out
    raise AssertionError("level %d holds %d isolated candidates, %d wanted" % (level, len(out), n))


def _on(level, i, dx=0.0, dy=0.0, mlev=None):
    """a measurement of level mlev (default: the candidate's) whose busy position at `level` is candidate i + (dx, dy)"""
    c = xy(level_candidates()[level][0])[i]
    s = 1 << level
    return (level if mlev is None else mlev, (c[0] + dx) * s, (c[1] + dy) * s)


DISTANCE = (((6, 8), True), ((7, 7), False), ((10, 0), True), ((9, 0), False), ((-8, -6), True), ((0, -9), False))       # offset, survives
ROUNDING = ((9.5, True), (9.49, False))                       # rounds to 10: d2 = 100 stays; to 9: goes


def _in_chunks(chunks):
    """level-0 candidates to put a measurement on so that every candidate it removes lies in the same chunk of 256, two per chunk"""
    pos = level_candidates()[0][0]
    c = xy(pos)
    out = []
    for k in chunks:
        got = 0
        for i in range(k * CHUNK, min((k + 1) * CHUNK, len(c))):
            gone = np.flatnonzero(((c - c[i]) ** 2).sum(1) < 100)
            if gone.min() >= k * CHUNK and gone.max() < (k + 1) * CHUNK:
                out.append(i); got += 1
                if got == 2:
                    break
        assert got >= 1, k
    return out


@functools.lru_cache(maxsize=None)
def scenario(name):
    """-> (measurements [(level, root x, root y)], targets [(level, candidate index, survives)])"""
    meas, targets = [], []
    n0 = len(level_candidates()[0][0])
    n_chunks = (n0 + CHUNK - 1) // CHUNK
    if name == "distance":
        taken = []
        for off, stays in DISTANCE:
            i = isolated(0, off, taken, 1)[0]
            taken.append(i)
            meas.append(_on(0, i, *off)); targets.append((0, i, stays))
    elif name.startswith("rounding"):
        level = int(name[-1])
        taken = []
        for dx, stays in ROUNDING:
            i = isolated(level, (round(dx), 0), taken, 1)[0]
            taken.append(i)
            m = _on(level, i, dx)
            if level == 1 and dx == 9.5:
                assert m[1] == int(m[1]) and int(m[1]) % 2 == 1       # root / 2 of an odd integer
            meas.append(m); targets.append((level, i, stays))
    elif name.startswith("level filter"):
        # one measurement on top of one candidate, a scenario each: a measurement of another level thins that level's neighbourhood too,
        # which must not reach a target.  Not isolated (levels 1 and 2 hold too few such candidates): what counts here is WHICH levels a
        # measurement thins; the neighbours that go with a target are in the expected lists
        level, mlev, stays = [f for f in LEVEL_FILTER if name.endswith("level %d, measurement of level %d" % f[:2])][0]
        i = len(level_candidates()[level][0]) // 2
        meas.append(_on(level, i, mlev=mlev)); targets.append((level, i, stays))
    elif name == "every candidate of level 2":
        n2 = len(level_candidates()[2][0])
        meas = [_on(2, i) for i in range(n2)]
        targets = [(2, i, False) for i in range(n2)]
    else:
        chunks = {"first chunk only": [0], "last chunk only": [n_chunks - 1], "every chunk": list(range(n_chunks))}[name]
        for i in _in_chunks(chunks):
            meas.append(_on(0, i)); targets.append((0, i, False))
    return meas, targets


def scenario_map(name):
    """the scenario as a map of the form System.load_map takes: keyframe 0 of the feeder's map, one map point per measurement"""
    m = _scene()[1]
    meas, _targets = scenario(name)
    _kf, _pt, _lv, _rx, _ry, sp, src = m["meas"][0]
    return {"keyframes": m["keyframes"][:1], "points": [dict(m["points"][0], src_kf=0) for _ in meas],
            "meas": [(0, j, lv, float(rx), float(ry), sp, src) for j, (lv, rx, ry) in enumerate(meas)]}


def expected(name):
    """the oracle's thinned lists of every level: [(positions, scores)]"""
    meas, _targets = scenario(name)
    root, mlev = np.array([[rx, ry] for _l, rx, ry in meas], np.float64), np.array([l for l, _x, _y in meas], np.int32)
    return [orc.thin_candidates(p, sc, l, root, mlev) for l, (p, sc) in enumerate(level_candidates())]
