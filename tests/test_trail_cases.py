"""CPU check of tests/trail_cases.py: the oracle alone, run on every case of tests/test_gpu_trail_counts.py, reaches the counts at which
k_trail_start, k_trail_advance and mp_find (csrc/boot.hip) and k_minipatch_find (csrc/minipatch.hip) split.  A case that misses a condition
is a broken case: the frames have to change, not the condition.  Run with -s to see the counts per target and the case that reaches each.

1. start_ref / advance_ref, driven by trail_cases.run, reproduce the oracle System's trails() and init_info() in every frame of every case:
   the records the counts are taken from describe what the oracle did.
2. Every target of trail_cases.TARGETS is reached by at least one case (none is listed in trail_cases.UNREACHED; one listed there would be
   asserted to stay at zero).
3. The trails' patches cannot be read back from the device: what checks their compaction is the NEXT frame's positions.  A compaction that
   leaves every kept trail its successor's patch gives other trails in the following frame (test_next_frame_depends_on_the_compacted_patches).
4. Every case that drops trails from the middle of the list runs at least two more frames.

The counts test_every_target_is_reached printed when the cases were written (searches or frames that meet the condition, over all cases;
the first case that reaches it); none is unreached:

       2  start: 0 candidates                                        96x64 flat frames
       8  start: 1-255 candidates                                    96x64 synth 3, a move of (12, 5)
       1  start: 257-999 candidates                                  160x120 synth 1, a move of (12, 5)
       3  start: > 1000 candidates, all scores distinct              320x240 synth 3, a move of (12, 5)
       4  start: > 1000 candidates, one score                        157x101 tile 7
       7  start: ranks 999 and 1000 share a score                    157x101 tile 7
       6  n = 0                                                      96x64 flat frames
       2  n = 1                                                      96x64 one rectangle corner
      44  n not a multiple of 4                                      96x64 synth 3, columns [0, 72) of frame 1 flat: good = 10
      47  n in 1-256 (per = 1)                                       96x64 synth 3, a move of (12, 5)
       5  n in 257-512 (per = 2)                                     160x120 synth 1, a move of (12, 5)
       4  n in 769-999 (per = 4)                                     320x240 synth 3, moves of (7, 4)
      17  n = 1000 (per = 4)                                         157x101 tile 7
       2  per = 2: survivors after a thread's range with drops       160x120 synth 1, a move of (12, 5)
       9  per = 4: survivors after a thread's range with drops       157x101 tile 13, moves of (3, 0) and (0, 3)
      54  window 0                                                   96x64 synth 5 then flat frames
     570  window 1-64                                                96x64 synth 3, a move of (12, 5)
    2698  window 65-128                                              96x64 synth 3, a move of (12, 5)
    2424  window 129-192                                             157x101 synth 3, a move of (12, 5)
   40342  window > 256                                               157x101 tile 7
   12451  a chunk without a box corner before one with               157x101 synth 3, a move of (12, 5)
   46744  chunk with 1-7 box corners                                 96x64 synth 3, a move of (12, 5)
   19747  chunk with 8, 16, ... box corners                          96x64 synth 3, a move of (12, 5)
   40137  chunk with > 8 box corners, no multiple of 8               96x64 synth 3, a move of (12, 5)
   42974  winner outside the first chunk                             96x64 synth 3, a move of (12, 5)
    6376  winner outside the first step of eight                     96x64 synth 3, a move of (12, 5)
    2355  tie: same step                                             157x101 tile 13, moves of (3, 0) and (0, 3)
    1200  tie: steps                                                 157x101 tile 13, moves of (3, 0) and (0, 3)
   10497  tie: chunks                                                157x101 tile 7
      28  tie: same step, forward, trail kept                        157x101 tile 13, moves of (3, 0) and (0, 3)
      90  tie: steps, forward, trail kept                            157x101 tile 13, moves of (3, 0) and (0, 3)
      12  tie: chunks, forward, trail kept                           157x101 tile 13, moves of (3, 0) and (0, 3)
     992  box over the top edge                                      96x64 synth 3, a move of (12, 5)
     116  box over the bottom edge                                   157x101 synth 3, a move of (12, 5)
     870  box over the left edge                                     96x64 synth 3, a move of (12, 5)
      88  box over the right edge                                    157x101 synth 6, moves of (-2, -1)
    5542  box corner within 4 px of a border                         96x64 synth 3, a move of (12, 5)
     138  forward miss, empty box                                    96x64 synth 3, a move of (12, 5)
     663  forward miss on SSD                                        96x64 synth 3, a move of (12, 5)
      19  backward miss                                              96x64 synth 4, the left half brighter by 20, then darker by 20
   16718  distance^2 0 kept                                          96x64 synth 3, a move of (12, 5)
      48  distance^2 1 kept                                          96x64 synth 3, a move of (12, 5)
       8  distance^2 2 kept                                          320x240 synth 3, a move of (12, 5)
    7741  distance^2 >= 4 dropped                                    96x64 synth 3, a move of (12, 5)
       4  good >= 10 with 1-9 survivors                              157x101 synth 3, a move of (12, 5)
       4  good >= 10 with no survivor                                157x101 tile 7
       7  good = 10 (continues)                                      96x64 synth 3, columns [0, 72) of frame 1 flat: good = 10
       1  good = 9 (resets)                                          96x64 synth 3, columns [0, 73) of frame 1 flat: good = 9
      14  reset                                                      96x64 synth 3, a move of (12, 5)
       2  first press after a reset                                  157x101 tile 7
"""
import numpy as np
import pytest

import trail_cases as tc

_TALLY = {}


def tallies(size):
    if size not in _TALLY:
        _TALLY[size] = [(c, tc.tally(tc.record(c))) for c in tc.group(size)]
    return _TALLY[size]


@pytest.mark.parametrize("size", tc.SIZES, ids=lambda s: "%dx%d" % s)
def test_restatement_reproduces_the_oracle_in_every_frame(size):
    cases = tc.group(size)
    assert len({len(c.frames) for c in cases}) == 1 and all((c.w, c.h) == size for c in cases)
    print("\n[%dx%d] %d streams" % (size + (len(cases),)))
    cap = list(cases[0].params(1).max_corners)
    for c in cases:
        recs, o = tc.record(c), c.oracle()
        for t, r in enumerate(recs):
            n_corners = [len(lv[1]) for lv in tc.orc.make_keyframe_lite(c.frames[t], list(c.params(1).fast_threshold))]
            assert all(n <= m for n, m in zip(n_corners, cap)), (c.name, t, n_corners, cap)   # the device's default corner lists hold every corner
            if t in c.presses:
                o.press_spacebar()
            o.track_frame(c.frames[t])
            io = o.init_info()
            assert io == dict(stage=r.stage, trails=len(r.positions), init_ok=0, hom_inliers=0, stereo_points=0, map_good=0), (c.name, t, io)
            assert np.array_equal(o.trails(), r.positions), (c.name, t)
        o.close()
        assert tc.resets([r.stage for r in recs]) == tc.RESETS[size][cases.index(c)], c.name
        print("  %s: %s" % (c.name, " ".join("%s%s" % (r.what, "" if r.n is None else "(n %d, good %d -> %d)" % (r.n, r.good, len(r.positions))) for r in recs)))


def test_one_frame_holds_a_start_an_advance_a_reset_and_an_unpressed_stream():
    t = tc.joint_frame(tc.group((160, 120)))
    assert t is not None
    print("\nframe %d of the 160x120 group: %s" % (t, [tc.record(c)[t].what for c in tc.group((160, 120))]))


def test_every_target_is_reached():
    total, where = dict.fromkeys(tc.TARGETS, 0), {}
    for size in tc.SIZES:
        for c, ta in tallies(size):
            for k, v in ta.items():
                total[k] += v
                if v and k not in where:
                    where[k] = "%dx%d %s" % (size + (c.name,))
    print()
    for k in tc.TARGETS:
        print("%8d  %-58s %s" % (total[k], k, where.get(k, "-- unreached")))
    assert len(tc.UNREACHED) <= 3 and not set(tc.UNREACHED) & set(tc.BARRED) and set(tc.UNREACHED) <= set(tc.TARGETS)
    for k in tc.TARGETS:
        if k in tc.UNREACHED:
            assert total[k] == 0, (k, total[k], "reached now: take it out of trail_cases.UNREACHED")
        else:
            assert total[k] > 0, k


def test_per_of_one_two_and_four_each_compact_visibly():
    """for every trails-per-thread count of k_trail_advance's compaction, a frame that drops trails before kept ones and whose survivors
    the next frame advances (so that their patches are used)"""
    seen = set()
    for size in tc.SIZES:
        for c in tc.group(size):
            recs = tc.record(c)
            for t, r in enumerate(recs[:-1]):
                if r.what == "advance" and recs[t + 1].what == "advance" and len(recs[t + 1].positions) > 0:
                    kept = np.array([x.kept for x in r.trails], bool)
                    drops = np.flatnonzero(~kept)
                    if len(drops) and kept[drops[0]:].any():
                        seen.add(tc.per_thread(r.n))
    assert {1, 2, 4} <= seen, seen


def test_cases_that_drop_from_the_middle_run_two_more_frames():
    n = 0
    for size in tc.SIZES:
        for c in tc.group(size):
            for t, r in enumerate(tc.record(c)):
                kept = np.array([x.kept for x in r.trails], bool)
                drops = np.flatnonzero(~kept)
                if len(drops) and kept[drops[0]:].any():                      # a kept trail behind a dropped one
                    assert t + 2 < len(c.frames), (c.name, t)
                    n += 1
                    break
    assert n >= 8, n


def test_next_frame_depends_on_the_compacted_patches():
    case = tc.group((160, 120))[0]
    recs = tc.record(case)
    t = next(t for t, r in enumerate(recs) if r.what == "advance" and 0 < len(r.positions) < r.n)
    assert recs[t + 1].what == "advance" and len(recs[t + 1].positions) > 0
    off = tc.run(case, shift_patches_after=t)
    for u in range(t + 1):
        assert np.array_equal(off[u].positions, recs[u].positions)             # the shift changes no position by itself
    assert not np.array_equal(off[t + 1].positions, recs[t + 1].positions)
    print("\n%s: frame %d keeps %d of %d trails; with the patches one slot off frame %d keeps %d trails, not %d" % (
        case.name, t, len(recs[t].positions), recs[t].n, t + 1, len(off[t + 1].positions), len(recs[t + 1].positions)))


@pytest.mark.parametrize("size", [(160, 120), (157, 101)], ids=lambda s: "%dx%d" % s)
def test_primitive_cases_reach_their_conditions(size):
    samples, prims = tc.primitives(size)
    by = {p.name: p for p in prims}
    assert len(by) == len(prims)
    n_inside = 0
    for _name, frame, pos in samples:
        ok = [tc.orc.minipatch_sample(frame, int(x), int(y)) is not None for x, y in pos]
        n_inside += sum(ok)
        assert not all(ok)                                                    # positions without a whole patch in every sample call
    assert n_inside > 1000
    assert {p.rng for p in prims} == set(tc.PRIM_RANGES) and {len(p.pos) for p in prims} >= {1, 1000}
    w, h = size
    pos = by["synth, range 10"].pos
    assert any(y - 400 < 0 and y + 400 >= h for _x, y in pos) and any(y - 10 >= h for _x, y in pos) and any(y + 10 + 1 < 0 for _x, y in pos)
    for r in tc.PRIM_RANGES:
        f, q = by["synth, range %d" % r].expected()
        assert 0 < f.sum() < len(f) and np.array_equal(q[f == 0], pos[f == 0])
        assert not f[-2:].any() or r == 400                                  # above and below the image: nothing within range
    best = [p for p in prims if p.name.endswith("max_ssd = best SSD")]
    assert len(best) == 6
    for p in best:
        stem = p.name[:-len("best SSD")]
        assert p.expected()[0].tolist() == [0] and by[stem + "best SSD + 1"].expected()[0].tolist() == [1] and by[stem + "0"].expected()[0].tolist() == [0]
        assert by[stem + "best SSD + 1"].max_ssd == p.max_ssd + 1
    assert by["random templates, max_ssd = 500"].expected()[0].sum() == 0
    assert by["a frame without corners"].expected()[0].sum() == 0 and tc.Frame(by["a frame without corners"].frame).n == 0
    ties = []
    for tile in (by["tile 7, 1000 corners"], by["tile 13, 300 corners"]):
        ft = tc.Frame(tile.frame)
        ties += [tc.Search(tile.patches[i], ft, int(x), int(y)).tie for i, (x, y) in enumerate(tile.pos[:300])]
    count = {k: ties.count(k) for k in tc.TIE_CLASSES}
    print("\n%dx%d: ties among 600 tile searches: %s" % (w, h, count))
    assert all(v >= 10 for v in count.values()), count
