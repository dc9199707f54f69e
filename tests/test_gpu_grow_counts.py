"""GPU parity of map growth at the counts where its kernels split (csrc/mapgrow.hip with grow_dev.h): k_target_implane, k_epipolar's ballot /
rank / sel[] batches of 8 (8x8 patches) or 4 (11x11) survivors and its ordered commit over the four wavefronts of a chunk with the
map-capacity branch, refind_common's loop over windows longer than 64 list entries by the row table (k_refind) and by the binary search
(k_refind_idle), the template RefindCache carries across the keyframes of one point with its kept verdict, and k_idle_gate.  The cases come
from tests/grow_cases.py -- sparse sub-maps, a capped tracker, the dense texture, whole-level rejections, a map that fills;
tests/test_grow_cases.py asserts on the CPU that the oracle reaches the counts on them.  Here the cases of a group are the streams of one
System, each beside its own oracle, both started from the same bits, bundle adjustment in reference order (ba_sum_order = 1): one tracked
frame that becomes a keyframe, the four idle jobs, a second tracked frame, everything compared with == and nothing re-synchronised, so a
first difference is a finding."""
import numpy as np
import pytest

import grow_cases as gc
import retire_ref as rr
from helpers import assert_map_exact, assert_tracker_exact
from visualslam_android_amd import capi

pytestmark = pytest.mark.gpu


def assert_tables_exact(o, g, s, tag):
    """every keyframe's measurement table: points, levels, sources and root positions"""
    for k in range(o.state().n_keyframes):
        mo, mg = o.keyframe_meas(k), g.keyframe_meas(s, k)
        assert np.array_equal(mo["pt"], mg["pt"]) and np.array_equal(mo["level"], mg["level"]) and np.array_equal(mo["source"], mg["source"]), (tag, k)
        assert np.array_equal(mo["root"], mg["root"]), (tag, k, np.abs(mo["root"] - mg["root"]).max())


def assert_candidates_exact(o, g, s, tag, vouched):
    """per level the candidates ThinCandidates left, in order, and what AddPointEpipolar did with each: a negative score is the stage that
    turned the candidate away (vslam_read_candidates), against the oracle's log of this keyframe -- which is the log the CPU test looked at"""
    log = o.grow_log()
    assert np.array_equal(log, vouched), tag
    for l in range(4):
        rows = log[log[:, 0] == l]
        pos, sc = g.read_candidates(s, l)
        assert np.array_equal(pos, rows[:, 1].astype(np.uint32)), (tag, l, len(pos), len(rows))
        stage = np.where(sc < 0, -sc, 0).astype(np.int32)
        assert np.array_equal(stage, rows[:, 2]), (tag, l, [(int(i), int(a), int(b)) for i, (a, b) in enumerate(zip(stage, rows[:, 2])) if a != b][:8])


def assert_never_retry_exact(o, g, s, tag):
    """sNeverRetryKFs of every point: the oracle's sets against the device's 128-bit words, read from a snapshot of the stream.  The
    measurement tables alone show a wrong bit only if a later job happens to retry the pair."""
    _h, secs = rr.sections(g.snapshot(s))
    dev = secs[rr.NEVER_RETRY].view(np.uint64).reshape(-1, 2)
    want = o.point_mapmaker_data()["never_retry"]
    assert dev.shape == want.shape and np.array_equal(dev, want), (tag, dev.shape, want.shape, np.flatnonzero((dev != want).any(1))[:8].tolist() if dev.shape == want.shape else None)
    return int(np.sum([bin(int(v)).count("1") for v in want.ravel()]))


def run_group(cases, patch, never_retry=False):
    """never_retry: also compare the never-retry sets after the keyframe and after each idle job -> the bits set at the end, per stream"""
    bits = {}
    S = len(cases)
    assert all(c.pkw == cases[0].pkw for c in cases)                                      # the parameters are system-wide
    g = capi.System(cases[0].params(S, patch))
    oracles = []
    for s, c in enumerate(cases):
        c.load(g, s)
        oracles.append(c.oracle(patch) if c.has_map else None)
    start = [(g.state(s).n_points, g.state(s).n_keyframes, g.idle_stats(s)) for s in range(S)]

    def untouched(s, tag):
        sg = g.state(s)
        assert (sg.n_points, sg.n_keyframes, g.idle_stats(s)) == start[s], (tag, sg.n_points, sg.n_keyframes, g.idle_stats(s), start[s])

    def tags(what):
        return [(s, c, o, "%s, %dx%d patches, %s" % (c.name, patch, patch, what)) for s, (c, o) in enumerate(zip(cases, oracles))]

    g.track_frame(np.stack([c.frame(0) for c in cases]))
    for s, c, o, tag in tags("frame 0"):
        if o is None:
            untouched(s, tag); continue
        o.track_frame(c.frame(0))
        so, sg = o.state(), g.state(s)
        assert (so.kf_added, so.n_keyframes, so.n_points) == (sg.kf_added, sg.n_keyframes, sg.n_points) and so.kf_added == int(c.grows), (tag, so.n_points, sg.n_points)
        if c.grows:
            assert_candidates_exact(o, g, s, tag, gc.record(c, patch).log)
        else:
            untouched(s, tag)
        assert_tables_exact(o, g, s, tag)
        assert_map_exact(o, g, s, tag)
        assert_tracker_exact(o, g, s, tag)
        if never_retry:
            assert_never_retry_exact(o, g, s, tag)
    for job in range(4):
        g.mapmaker_idle_job(job)
        for s, c, o, tag in tags("idle job %d" % job):
            if o is None or not c.grows:
                untouched(s, tag)
            if o is None:
                continue
            o.idle_job(job)
            assert g.idle_stats(s) == o.idle_stats(), (tag, g.idle_stats(s), o.idle_stats())
            assert_tables_exact(o, g, s, tag)
            assert_map_exact(o, g, s, tag)
            if never_retry:
                bits[s] = assert_never_retry_exact(o, g, s, tag)
    g.track_frame(np.stack([c.frame(1) for c in cases]))
    for s, c, o, tag in tags("frame 1"):
        if o is None:
            untouched(s, tag); continue
        o.track_frame(c.frame(1))
        assert_tracker_exact(o, g, s, tag)                                                # templates included: the new points' pixel vectors and source patches
        assert o.state().kf_added == 0                                                    # no second keyframe inside the frames run (test_grow_cases.py)
        assert g.idle_stats(s) == o.idle_stats(), tag
        assert_tables_exact(o, g, s, tag)
        assert_map_exact(o, g, s, tag)
        o.close()
    g.close()
    return bits


@pytest.mark.parametrize("patch", [8, 11])
def test_epipolar_search_at_every_candidate_count(patch):
    """11 streams: the full map, every 2nd / 4th / 8th / 16th point, the level-0 points alone, levels 1-3 alone, the first 200 points, every 8th
    point of the dense texture, a stream whose tracker asks for no keyframe and one without a map.  Per-level candidate counts 0, 1, 2, 3,
    multiples of 4 and every residue modulo the four wavefronts of a chunk; up to 11 candidates and a new point at level 3, the first level
    processed; stages 0, 5 and 6; up to 27 survivors of the line filter in one ballot (four steps of 8, seven of 4) and survivors in
    several blocks of the target's corner list; chunks accepted whole and in part; then ReFindNewlyMade with thousands of kept
    templates.  The two idle streams stay untouched."""
    run_group(gc.groups(patch)["a: epipolar counts"], patch)


@pytest.mark.parametrize("patch", [8, 11])
def test_refind_at_every_level_and_window_length(patch):
    """max_patches_per_frame = 100 on the full map, every 2nd point and the dense texture's full map: ReFindInSingleKeyFrame measures
    hundreds of points at levels 0 to 2 and a few at level 3 (the sub-pixel iterations whose result nobody checks), in windows of up to 161
    list entries (three passes of refind_common's loop) found through the row table, and ReFindNewlyMade in windows of up to 130 found by
    the binary search.  The fourth stream sees every 8th point from twice as close: its new level-0 points have a bad scale in the map's
    keyframes, so the kept template of ReFindNewlyMade answers bad (RefindCache's bad_scale ? true : prev_bad) dozens of times.  The
    never-retry sets are compared after the keyframe and after every idle job: the returns of refind_common before the template (outside
    largest_radius, outside the image) set a bit and nothing else, so only the sets show them."""
    bits = run_group(gc.groups(patch)["b: re-find"], patch, never_retry=True)
    assert len(bits) == 4 and min(bits.values()) >= 100, bits                            # the sets compared are not empty


@pytest.mark.parametrize("patch", [8, 11])
@pytest.mark.parametrize("which", ["c: stage 1", "c: stage 2"])
def test_levels_rejected_whole(which, patch):
    """wiggle_scale = 0.02: every ray ends before it starts, 121 calls at four levels leave at stage 1.  A frame rendered at the pose of map
    keyframe 0 with max_kf_dist_wiggle_mult = 0: the keyframe is requested all the same and all 200 epipolar segments are shorter than
    1e-4, stage 2.  No point is added; the codes, the tables and the map still == the oracle's."""
    run_group(gc.groups(patch)[which], patch)


@pytest.mark.parametrize("patch", [8, 11])
def test_map_that_fills_during_growth(patch):
    """max_points = 256, five streams: sub-maps that fill the map during level 0 and during level 1, one whose last accepted candidate takes
    the last slot (no stage 7 at all), one whose first call on a full map is not the first wavefront of its chunk.  Every later candidate that
    passes all stages is marked -7 and adds nothing; every stream ends on 256 points, and the second frame tracks the full map.  No second
    keyframe falls inside the two frames."""
    cases = gc.groups(patch)["d: map capacity"]
    assert cases[0].params(1, patch).max_points == gc.MAX_POINTS
    run_group(cases, patch)


@pytest.mark.parametrize("patch", [8, 11])
def test_epipolar_exits_and_refind_behind(patch):
    """Group e, ten streams.  Two whose target keyframe is the camera of frame 0 turned 20 and -30 degrees about its vertical axis:
    dozens of candidates at levels 0 to 2 leave at stage 3 (the line passes outside largest_radius; with +20 degrees dNormDist has one sign,
    with -30 the other) beside accepted candidates in the same chunks, and the codes, the new points and the tables == the oracle's.  One
    with three map points behind the new keyframe: refind_common's first early return, which writes a never-retry bit and nothing else.
    Five with a block of texture repeated in the target keyframe's image, so that an accepted candidate meets two corners of equal ZMSSD at
    its minimum -- in one step of k_epipolar's ballot (the first step at both patch sizes, the second at 11x11), in two steps, in two
    ballots: the first in list order must win, and the new point's position and its measurement in the target keyframe (compared bit for
    bit) are the twin's otherwise.  Two that reach the start-depth clip inside k_epipolar: a camera zoomed out and tilted 35 degrees, with
    hundreds of clipped lines of which a few are matched and accepted, and a tilted camera whose target is turned 80 degrees and stands
    0.04 ahead of it (dirn[2] of a few hundredths in the re-start's division).
    The never-retry sets are compared after the keyframe and after every idle job."""
    cases = gc.groups(patch)["e: epipolar exits"]
    bits = run_group(cases, patch, never_retry=True)
    assert len(bits) == len(cases) == 5 + len(gc.TIES) and min(bits.values()) >= gc.BEHIND, bits


@pytest.mark.parametrize("patch", [8, 11])
def test_refind_templates_that_leave_their_source_image(patch):
    """Group f, five streams on a map whose points keep patch // 2 level pixels from the borders of their source images.  Three (the full
    map at zooms 1.0, 0.8 and 0.6, the tracker capped at 100 patches): dozens of templates that refind_common makes anew sample outside
    the source -- warp_sample gives 0 and counts, one pixel per lane, the template is bad, the pair gets its never-retry bit and no
    measurement.  Two (every 4th point, two map keyframes that see the new keyframe from 78 or 75 degrees to the side, a fraction of a
    degree apart): new points whose template leaves the new keyframe's image in the first of the two and is kept, with its verdict, by
    the second (RefindCache::prev_bad from nOutside, where group b's comes from the scale).  A verdict taken the other way shows as a
    measurement row or a missing never-retry bit: both are compared after the keyframe and after every idle job, and the second frame's
    tracker state after that."""
    cases = gc.groups(patch)["f: border map"]
    bits = run_group(cases, patch, never_retry=True)
    assert len(bits) == len(cases) == 5 and min(bits.values()) >= 100, bits
