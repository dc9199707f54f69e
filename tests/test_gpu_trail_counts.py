"""GPU parity of the first half of the map bootstrap at the counts where its kernels split: k_trail_start's cut at rank 1000 with equal
scores in candidate order, k_trail_advance's compaction at one, two and four trails per thread and its Reset tail, mp_find's walk over
row windows of nought to sixteen chunks of 64 with ties inside a step of eight, between steps and between chunks (csrc/boot.hip), and the two
C-ABI primitives k_minipatch_sample / k_minipatch_find (csrc/minipatch.hip), which are separate code.  The cases come from
tests/trail_cases.py; tests/test_trail_cases.py asserts on the CPU that the oracle reaches every condition on them.

Here the cases of a size are the streams of one System (bootstrap = 1, grow_map = 3, default corner capacity), each beside its own oracle
System, every stream with its own spacebar presses.  After every frame and for every stream: init_info on all six fields, and while the
stage is 1 the trails -- order, initial and current positions -- with ==.  The trails' patches cannot be read back; the frame after a
compaction searches with them (test_trail_cases.py shows that a patch one slot off changes that frame).  Everything is an integer: no
tolerance anywhere."""
import numpy as np
import pytest

import trail_cases as tc
from visualslam_android_amd import capi

pytestmark = pytest.mark.gpu


def explain(case, t, want, got):
    """which trail of the frame's record (trail_cases.run, made only now) the first differing row belongs to, and what its searches met"""
    rec = tc.record(case)[t]
    kept = [i for i, x in enumerate(rec.trails) if x.kept]
    n = min(len(want), len(got))
    diff = np.flatnonzero((want[:n] != got[:n]).any(1))
    row = int(diff[0]) if len(diff) else n
    msg = "%s of n = %s: %d trails against the oracle's %d, first difference in row %d" % (rec.what, rec.n, len(got), len(want), row)
    if row < len(want) and row < len(kept):
        x = rec.trails[kept[row]]
        msg += ": trail %d, oracle %s" % (kept[row], want[row].tolist())
        if row < len(got):
            msg += ", device %s" % got[row].tolist()
        msg += "; forward search: window %d, box corners per chunk %s, tie class %s (%d corners share the minimum), winner in chunk %s step %s" % (
            x.fwd.win_len, x.fwd.box, x.fwd.tie, x.fwd.n_tied, x.fwd.win_chunk, x.fwd.win_step)
        if x.back is not None:
            msg += "; backward search: window %d, tie class %s, distance^2 %s" % (x.back.win_len, x.back.tie, x.d2)
    ties = {c: sum(1 for x in rec.trails for s in (x.fwd, x.back) if s is not None and s.tie == c) for c in tc.TIE_CLASSES}
    return msg + "; ties in this frame %s" % ties


def run_group(size):
    """-> per stream the stages after each frame"""
    cases = tc.group(size)
    S, T = len(cases), len(cases[0].frames)
    g = capi.System(cases[0].params(S, bootstrap=1))
    assert list(g.params.max_corners)[0] == (size[0] * size[1]) // 2
    oracles = [c.oracle() for c in cases]
    stages = [[] for _ in cases]
    for t in range(T):
        for s, c in enumerate(cases):
            if t in c.presses:
                g.press_spacebar(s); oracles[s].press_spacebar()
        g.track_frame(np.stack([c.frames[t] for c in cases]))
        for s, (c, o) in enumerate(zip(cases, oracles)):
            o.track_frame(c.frames[t])
            io, ig = o.init_info(), g.init_info(s)
            tag = "%dx%d stream %d (%s) frame %d" % (size + (s, c.name, t))
            want, got = o.trails(), g.trails(s)
            assert len(want) == io["trails"] and (io["stage"] == 1 or len(want) == 0), tag
            if io["stage"] == 1 and not np.array_equal(want, got):        # first, so that the message can name the trail and its tie class
                raise AssertionError("%s: %s" % (tag, explain(c, t, want, got)))
            assert io == ig, "%s: oracle %s, device %s" % (tag, io, ig)
            assert len(got) == ig["trails"], tag
            stages[s].append(io["stage"])
    for o in oracles:
        o.close()
    g.close()
    return stages


def test_trails_96x64():
    """Seven streams of the band form: 48 trails in windows of 23 to 102 corners; the flat rectangle that leaves good = 10 (continues with
    ten trails) and, one column further, good = 9 (Reset); a single candidate (n = 1); a brightness step that makes 19 backward searches
    miss; flat frames after a start (every window empty, good = 0); a press on a flat frame (no candidate, n = 0, Reset)."""
    st = run_group((96, 64))
    assert [tc.resets(x) for x in st] == tc.RESETS[(96, 64)], st


def test_trails_157x101():
    """Five streams, odd width and height, the device's row pitch is not the width: a move of (12, 5) that leaves 30 of 138 trails, then 6,
    then Reset; the 7-tile (1000 of 1605 candidates with one score, every search tied, no survivor, Reset, pressed again); the 13-tile with
    ties inside a step, between steps and between chunks whose trails survive; moves to the left and up (boxes over the right and bottom
    edges); a stream never pressed."""
    st = run_group((157, 101))
    assert [tc.resets(x) for x in st] == tc.RESETS[(157, 101)], st


def test_trails_160x120():
    """Six streams of the strip form; in frame 3 one consumes its first press, two advance, two reset and one has never been pressed.  275
    trails (two per thread of the compaction) of which a move of (12, 5) keeps 60; the 7-tile (4268 corners, 2000 candidates of one score) and
    its second first press after the Reset; the 9-tile (ranks 999 and 1000 inside an equal-score group, 1000 -> 1 trail -> Reset); the 13-tile."""
    st = run_group((160, 120))
    assert [tc.resets(x) for x in st] == tc.RESETS[(160, 120)], st
    assert [x[2:4] for x in st] == [[1, 1], [1, 0], [0, 1], [1, 1], [1, 0], [0, 0]], st      # frame 3: advance, reset, start, advance, reset, idle


def test_trails_320x240():
    """Four streams: 1160 candidates with distinct scores cut at 1000; four trails per thread; a move of (12, 5) that keeps 273 of 1000,
    then 74; moves of (7, 4) that keep 994, 988, 962, 959 (drops in the middle of full ranges); windows of 126 to 390 corners."""
    st = run_group((320, 240))
    assert [tc.resets(x) for x in st] == tc.RESETS[(320, 240)], st


@pytest.mark.parametrize("size", [(160, 120), (157, 101)], ids=lambda s: "%dx%d" % s)
def test_minipatch_primitives(size):
    """vslam_minipatch_sample / vslam_minipatch_find against orc.minipatch_*: corners, other positions, the image's four corners, positions
    above and below the image; ranges 0, 3, 10 and 400; max_ssd at a trail's best SSD (not found: strict <), one above (found) and 0;
    random templates; tiled frames whose searches tie inside a step, between steps and between chunks; a frame without corners; n = 1 and
    n = 1000.  found and the positions with ==, the position unchanged where nothing is found."""
    w, h = size
    samples, prims = tc.primitives(size)
    g = capi.System(capi.default_params(w, h, 1))
    for name, frame, pos in samples:
        g.make_keyframe_lite(frame[None])
        patches, ok = g.minipatch_sample(0, pos)
        for i, (x, y) in enumerate(pos):
            want = tc.orc.minipatch_sample(frame, int(x), int(y))
            assert bool(ok[i]) == (want is not None), (name, i, x, y)
            if want is not None:
                assert np.array_equal(patches[i], want), (name, i, x, y)
    loaded, fr = None, None
    for p in prims:
        if loaded is not p.frame:
            g.make_keyframe_lite(p.frame[None])
            loaded, fr = p.frame, tc.Frame(p.frame)
        found, pos = g.minipatch_find(0, p.patches, p.pos, p.rng, p.max_ssd)
        want_found, want_pos = p.expected(fr)
        bad = np.flatnonzero((found != want_found) | (pos != want_pos).any(1))
        assert len(bad) == 0, (p.name, [(int(i), p.pos[i].tolist(), int(found[i]), pos[i].tolist(), int(want_found[i]), want_pos[i].tolist()) for i in bad[:5]])
    g.close()
