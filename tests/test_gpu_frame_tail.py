"""GPU parity of the tracker's frame tail at its thresholds (the end of k_pose's fine stage and k_plan's velocity gate, csrc/track.hip) and of
k_thin_candidates at its edges (csrc/frontend.hip).  The cases come from tests/quality_cases.py and tests/thin_cases.py, built from the
oracle alone; tests/test_quality_cases.py and tests/test_thin_cases.py assert on the CPU that the oracle reaches every target.  Here the
device is held to the oracle with ==, and to the case's target, which ties the run to the case the CPU test vouched for:

  quality cut-offs      dTotal on 0.3 and above, la on 10 and 11, dLarge on 0.13 and on both sides, tf == 0, one level only
  brackets              wiggle_scale, max_kf_dist_wiggle_mult and coarse_min_vel at two ADJACENT doubles with different decisions
  keyframe gate         min_frames_between_kf = 3: a keyframe every fourth frame; a full map without keyframe_retire asks for none
  loss and return       lost_frames counts up over blank frames and is reset, a DODGY frame between two BAD ones
  ThinCandidates        d2 == 100 and below, rounding of .5, the level filter, untouched and emptied levels, removals per chunk of 256"""
import numpy as np
import pytest

import quality_cases as qc
import thin_cases as th
from helpers import assert_map_exact, assert_tracker_exact, check_and_resync, pose_err
from stagewise import run_group
from visualslam_android_amd import capi

pytestmark = pytest.mark.gpu

FIRST_FRAME_KEYS = ("attempted", "found", "quality", "kf_added", "n_keyframes", "did_coarse")


def first_frame_targets(cases):
    """run_group's per-frame hook: after frame 0 the device's state == the case's target; after a keyframe the map == the oracle's"""
    def check(o, g, s, tag):
        sg = g.state(s)
        if sg.frame == 1:
            for key in FIRST_FRAME_KEYS:
                if key in cases[s].target:
                    got = getattr(sg, key)
                    assert (list(got) if key in ("attempted", "found") else got) == cases[s].target[key], (tag, key)
        if o.state().kf_added:
            assert_map_exact(o, g, s, tag)
    return check


@pytest.mark.parametrize("patch", [8, 11])
def test_quality_at_its_cut_offs(patch):
    """AssessTrackingQuality (jni/Tracker.cc:832-878) on per-level counts that sit on dTotal == 0.3 (3/10, 30/100) and just above (4/13),
    la == 10 and 11, dLarge == 2/15, 13/100 and 2/16 around 0.13, tf == 0 and a single level-3 patch: quality 1 (DODGY) on six of the ten
    streams, and lost_frames after one frame"""
    cases = qc.quality_cases(patch)
    assert sorted({c.target["quality"] for c in cases}) == [0, 1, 2]
    run_group(cases, patch, first_frame_targets(cases))


@pytest.mark.parametrize("patch", [8, 11])
@pytest.mark.parametrize("param", sorted(qc.BRACKETS))
def test_decision_flips_between_adjacent_doubles(param, patch):
    """one System on each side of the oracle's bracket: wiggle_scale (a DODGY frame is demoted to BAD when closest > wiggle_scale * 10),
    max_kf_dist_wiggle_mult (closest * (1.0 / depth_mean) > mult * wiggle_depth_norm asks for a keyframe; n_keyframes and the adjusted
    map are compared too), coarse_min_vel (msd_vel < coarse_min_vel switches the coarse stage off; did_coarse is 1 AT equality)"""
    pair = qc.bracket_pair(param, patch)
    key = qc.BRACKETS[param][0]
    assert pair[0].target[key] != pair[1].target[key]
    for c in pair:
        run_group([c], patch, first_frame_targets([c]))


def run_free(case, patch, n_frames, oracle_case=None, **params):
    """two streams of the case frame by frame against one oracle (of oracle_case, default the case), re-synchronised after every frame ->
    (kf_added, n_keyframes) of the device per frame"""
    dev = case.variant(**params) if params else case
    g = capi.System(dev.params(2, patch))
    for s in range(2):
        dev.load(g, s)
    o = (oracle_case or case).oracle(patch)
    out = []
    for t in range(n_frames):
        g.track_frame(np.stack([dev.frame(t)] * 2))
        o.track_frame(dev.frame(t))
        for s in range(2):
            tag = "%s, %dx%d patches, frame %d, stream %d" % (dev.name, patch, patch, t, s)
            assert_tracker_exact(o, g, s, tag)
            if o.state().kf_added:
                assert_map_exact(o, g, s, tag)                   # ba_sum_order = 1: the adjusted map bit for bit
            check_and_resync(o, g, s, tag)
        assert g.state(0).quality == 2
        out.append((g.state(0).kf_added, g.state(0).n_keyframes))
    o.close()
    g.close()
    return out


@pytest.mark.parametrize("patch", [8, 11])
def test_keyframe_gate_in_frames(patch):
    """min_frames_between_kf = 3 with a keyframe wanted on every frame (max_kf_dist_wiggle_mult = 0): frame - last_kf_dropped > 3 grants
    frames 0, 4, 8 of 9"""
    out = run_free(qc.gate_case(patch), patch, qc.GATE_FRAMES)
    added = [t for t, (kf, _n) in enumerate(out) if kf]
    assert len(added) >= 2 and all(b - a == qc.GATE_MIN_FRAMES + 1 for a, b in zip(added, added[1:])), added
    assert [n for _kf, n in out] == [8 + sum(t >= a for a in added) for t in range(qc.GATE_FRAMES)]


@pytest.mark.parametrize("patch", [8, 11])
def test_full_map_without_retirement_asks_for_no_keyframe(patch):
    """the same run on a map that fills max_keyframes = 8, keyframe_retire = 0: no request on any frame, and the tracker == an oracle that
    never wants a keyframe (the oracle has no capacity).  With max_keyframes = 9 exactly one keyframe is added, on the frame the
    unbounded oracle adds its first, and until the oracle's second the two stay =="""
    case = qc.gate_case(patch)
    assert len(case.map()["keyframes"]) == 8
    never = qc.gate_case(patch, min_frames_between_kf=1000)
    out = run_free(case, patch, qc.GATE_FRAMES, oracle_case=never, max_keyframes=8, keyframe_retire=0)
    assert out == [(0, 8)] * qc.GATE_FRAMES
    first, second = 0, qc.GATE_MIN_FRAMES + 1                        # test_quality_cases.py: the unbounded oracle adds on frames 0, 4, 8
    out = run_free(case, patch, second, max_keyframes=9, keyframe_retire=0)
    assert out == [(int(t == first), 9) for t in range(second)]
    dev = case.variant(max_keyframes=9, keyframe_retire=0)
    g = capi.System(dev.params(1, patch))
    dev.load(g, 0)
    for t in range(qc.GATE_FRAMES):
        g.track_frame(dev.frame(t)[None])
        sg = g.state(0)
        assert (sg.quality, sg.kf_added, sg.n_keyframes) == (2, int(t == first), 9), t
    g.close()


@pytest.mark.parametrize("patch", [8, 11])
def test_loss_and_return(patch):
    """blank frames at {1, 2}, {1, 3} and {1, 2, 4, 5} of 7, and a DODGY frame (painted grey from a column on) between two blank ones: each
    sequence beside an undisturbed copy in one System, free-running.  On every frame quality, lost_frames, the per-level counts, the pose
    and the velocity == the oracle's (a blank frame's update is zero on both sides; the velocity it decays is what the next real frame
    starts from); on real frames everything assert_tracker_exact compares."""
    cases = qc.loss_cases(patch)
    streams = [c2 for c in cases for c2 in (c, qc.undisturbed(c))]
    assert len(cases) == 4 and len(streams) <= 17 and all(c.pkw == streams[0].pkw for c in streams)
    g = capi.System(streams[0].params(len(streams), patch))
    oracles = []
    for s, c in enumerate(streams):
        c.load(g, s)
        oracles.append(c.oracle(patch))
    for t in range(qc.LOSS_FRAMES):
        g.track_frame(np.stack([c.frame(t) for c in streams]))
        for s, (o, c) in enumerate(zip(oracles, streams)):
            o.track_frame(c.frame(t))
            tag = "%s, %dx%d patches, frame %d" % (c.name, patch, patch, t)
            so, sg = o.state(), g.state(s)
            assert (so.quality, so.lost_frames, so.frame, so.n_keyframes) == (sg.quality, sg.lost_frames, sg.frame, sg.n_keyframes), (tag, so.quality, sg.quality, so.lost_frames, sg.lost_frames)
            assert list(so.attempted) == list(sg.attempted) and list(so.found) == list(sg.found), tag
            assert np.array_equal(np.array(so.pose[:]), np.array(sg.pose[:])), (tag, pose_err(so.pose, sg.pose))
            assert np.array_equal(np.array(so.velocity[:]), np.array(sg.velocity[:])), tag
            if c.edits.get(t) != qc.BLANK:
                assert_tracker_exact(o, g, s, tag)
            if c.target:
                assert (sg.quality, sg.lost_frames) == (c.target["quality"][t], c.target["lost_frames"][t]), tag
            else:
                assert (sg.quality, sg.lost_frames) == (2, 0), tag
    for o in oracles:
        o.close()
    g.close()


def test_thin_candidates_at_the_edges():
    """MapMaker::ThinCandidates against a stored keyframe's measurements (jni/MapMaker.cc:381-422), one hand-built map per stream, all on
    the same frame: the surviving positions and scores of every level == the oracle's"""
    S = len(th.SCENARIOS)
    g = capi.System(capi.default_params(th.W, th.H, S))
    for s, name in enumerate(th.SCENARIOS):
        g.load_map(s, th.scenario_map(name))
    g.make_keyframe_lite(np.stack([th.frame()] * S))
    g.make_keyframe_rest(th.MIN_SCORE)
    for s in range(S):
        for l, (pos, sc) in enumerate(th.level_candidates()):
            got, gsc = g.read_candidates(s, l)
            assert np.array_equal(got, pos) and np.array_equal(gsc, sc), ("before thinning", s, l)
    g.thin_candidates(0)
    for s, name in enumerate(th.SCENARIOS):
        want = th.expected(name)
        _meas, targets = th.scenario(name)
        for l in range(4):
            got, gsc = g.read_candidates(s, l)
            assert np.array_equal(got, want[l][0]) and np.array_equal(gsc, want[l][1]), (name, l, len(got), len(want[l][0]))
        for level, i, stays in targets:                              # the target itself, by name
            p = th.level_candidates()[level][0][i]
            assert (p in g.read_candidates(s, level)[0]) == stays, (name, level, i)
    g.close()
