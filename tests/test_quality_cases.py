"""CPU check of tests/quality_cases.py: the oracle alone reaches every case's target EXACTLY -- the per-level attempted and found counts
and the quality of the cut-off cases, two adjacent doubles with different decisions for each bracketed parameter, a keyframe every
fourth frame under min_frames_between_kf = 3, and the lost_frames sequences of the loss-and-return cases.  A case that misses is a broken
case: the selection has to change, not the target.  Run with -s to see every case's counts, the three brackets and the column of the
DODGY frame."""
import numpy as np
import pytest

import quality_cases as qc
import tracker_cases as tc


@pytest.mark.parametrize("patch", [8, 11])
def test_quality_cases_reach_their_counts_and_quality(patch):
    cases = qc.quality_cases(patch)
    assert len(cases) == len(qc.QUALITY_TABLE) <= 17
    print("\n[quality cut-offs, %dx%d patches] found / unfound per level: %s plain, %s painted from column %d"
          % (patch, patch, qc.level_counts(qc.flags(tc.A_SCENE, patch)), qc.level_counts(qc.flags(tc.A_SCENE, patch, qc.PAINT_X)), qc.PAINT_X))
    for c in cases:
        s = qc.frame0(c, patch)
        print("  %s: attempted %s, found %s, quality %d" % (c.name, list(s.attempted), list(s.found), s.quality))
        assert s.n_points == c.target["n_points"] <= 130
        assert (list(s.attempted), list(s.found), s.quality) == (c.target["attempted"], c.target["found"], c.target["quality"]), c.name
        assert s.did_coarse == 0 and s.lost_frames == (1 if s.quality == 0 else 0) and s.kf_added == 0


def test_quality_table_sits_on_the_cut_offs():
    """what the table is for, in the counts themselves: dTotal on 0.3 and just above, la on 10 and 11, dLarge on 0.13 and on both sides"""
    rows = {name: ([f + u for f, u in zip(found, unfound)], found, q) for name, found, unfound, q, _paint in qc.QUALITY_TABLE}
    ratio = lambda a, f: (sum(f) / sum(a), sum(a[2:]), sum(f[2:]))
    assert [ratio(*rows[n][:2])[0] for n in ("dTotal == 3/10, la = 4", "dTotal == 30/100, lf/la = 3/20")] == [0.3, 0.3]
    assert ratio(*rows["dTotal == 30/100, lf/la = 3/20"][:2])[1:] == (20, 3)
    assert ratio(*rows["dTotal == 4/13"][:2])[0] == 4 / 13 > 0.3
    assert ratio(*rows["la == 10, lf = 1, 8/40"][:2]) == (0.2, 10, 1) and ratio(*rows["la == 11, lf = 1, 8/40"][:2]) == (0.2, 11, 1)
    for name, la, lf in (("lf/la == 2/15", 15, 2), ("lf/la == 2/16", 16, 2), ("lf/la == 13/100", 100, 13)):
        d, a, f = ratio(*rows[name][:2])
        assert (a, f) == (la, lf) and d <= 0.3, name
    assert 2 / 16 < 0.13 == 13 / 100 < 2 / 15                        # 13.0 / 100 rounds to the double the literal 0.13 is
    assert sum(rows["tf == 0, ta = 12"][0]) == 12 and rows["level 3 only, 1/1"][0] == [0, 0, 0, 1]
    assert sorted({q for _a, _f, q in rows.values()}) == [0, 1, 2]


@pytest.mark.parametrize("patch", [8, 11])
@pytest.mark.parametrize("param", sorted(qc.BRACKETS))
def test_brackets_are_adjacent_doubles_with_different_decisions(param, patch):
    key, lo, hi, at_lo, at_hi = qc.BRACKETS[param]
    a, b, at_a, at_b, runs = qc.bracket(param, patch)
    print("\n[%s, %dx%d patches] %s is %d at %r and %d at %r (%d oracle runs)" % (param, patch, patch, key, at_a, a, at_b, b, runs))
    assert lo <= a < b <= hi and np.nextafter(a, b) == b and (at_a, at_b) == (at_lo, at_hi)
    base = qc.bracket_base(param, patch)
    assert len(base.map()["points"]) <= 100
    pair = qc.bracket_pair(param, patch)
    states = [qc.frame0(c, patch) for c in pair]
    for c, s in zip(pair, states):                                   # the pair's cases, run afresh, stand on the two sides
        for k, v in c.target.items():
            assert getattr(s, k) == v, (c.name, k)
    assert states[0].pose[:] == states[1].pose[:] or param == "coarse_min_vel"       # the parameter enters the decision alone
    if param == "wiggle_scale":
        assert list(states[0].attempted) == list(states[1].attempted) and list(states[0].found) == list(states[1].found)
        assert qc.assess(list(states[0].attempted), list(states[0].found)) == 1      # DODGY by the counts: the demotion decides
        # a * 10 < closest <= b * 10, and the two products are adjacent doubles: closest == wiggle_scale * 10 at b, where the frame stays DODGY
        assert np.nextafter(a * 10.0, 1.0) == b * 10.0
    if param == "max_kf_dist_wiggle_mult":
        assert [s.quality for s in states] == [2, 2] and [s.n_keyframes for s in states] == [len(base.map()["keyframes"]) + 1, len(base.map()["keyframes"])]
    if param == "coarse_min_vel":
        o = pair[0].oracle(patch)
        assert o.state().msd_velocity == a                            # did_coarse is 1 AT msd_vel == coarse_min_vel (msd_vel < coarse_min_vel is false)
        o.close()
        n23 = sum(qc.frame0(pair[0].variant(coarse_min_vel=0.0), patch).attempted[2:])
        assert n23 >= tc.COARSE_MIN + 1


@pytest.mark.parametrize("patch", [8, 11])
def test_keyframe_gate_grants_every_fourth_frame(patch):
    f, _m, frames = tc.scene(*tc.A_SCENE)
    assert qc.GATE_FRAMES > len(frames) and np.array_equal(f.render(3, 1)[0], frames[3])           # the later frames continue the same path
    added, n_kf = qc.keyframe_frames(qc.gate_case(patch), patch)
    print("\n[keyframe gate, %dx%d patches] keyframes added on frames %s, n_keyframes %s" % (patch, patch, added, n_kf))
    assert len(added) >= 2 and all(b - a == qc.GATE_MIN_FRAMES + 1 for a, b in zip(added, added[1:])), added
    assert added[0] == 0                                               # test_gpu_frame_tail.py's full-map test counts from here
    never, n_never = qc.keyframe_frames(qc.gate_case(patch, min_frames_between_kf=1000), patch)      # the oracle the full map is held to
    assert never == [] and set(n_never) == {8}


@pytest.mark.parametrize("patch", [8, 11])
def test_loss_sequences_count_up_and_reset(patch):
    cases = qc.loss_cases(patch)
    found = qc.dodgy_column(patch)
    print("\n[loss and return, %dx%d patches] DODGY frame: %s" % (patch, patch, "none found" if found is None else "choose_found seed %d, grey from column x = %d" % found))
    assert found is not None and len(cases) == len(qc.LOSS_SEQUENCES) + 1
    for c in cases:
        seq = qc.sequence(c, patch)
        print("  %s: quality %s, lost_frames %s" % (c.name, [q for q, _l in seq], [l for _q, l in seq]))
        assert [q for q, _l in seq] == c.target["quality"] and [l for _q, l in seq] == c.target["lost_frames"], c.name
        assert max(c.target["lost_frames"]) < 3                      # never handed to the relocaliser
        ok = qc.sequence(qc.undisturbed(c), patch)
        assert ok == [(2, 0)] * qc.LOSS_FRAMES, c.name
    assert [c.target["lost_frames"] for c in cases[:3]] == [[0, 1, 2, 0, 0, 0, 0], [0, 1, 0, 1, 0, 0, 0], [0, 1, 2, 0, 1, 2, 0]]
    assert cases[3].target["quality"][:5] == [2, 0, 1, 0, 2] and cases[3].target["lost_frames"][:5] == [0, 1, 0, 1, 0]
