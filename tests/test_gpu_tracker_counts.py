"""GPU parity of the tracker at the counts where its kernels split (csrc/track.hip): k_pvs's LDS blocks, k_plan's passes and selection
edges, k_searchN's patches per wavefront, xcd_stream_block's groups of eight streams, k_subpixN's strided grid, and k_pose's batches,
chunks and read-ahead.  The cases come from tests/tracker_cases.py -- sub-maps chosen from the oracle so that each reaches a wanted
n_points, number of searched patches, per-level count or number of found patches; tests/test_tracker_cases.py asserts on the CPU that
they do.  Here every case is a stream of one System beside its own oracle (stagewise.run_group), both started from the same bits, and everything is compared
with ==: after each search and pose stage (so a difference is attributed to one of them), and after the frame through
helpers.assert_tracker_exact, templates included.  Two frames per case, re-synchronised in between; the second takes the
cached-template path."""
import numpy as np
import pytest

import tracker_cases as tc
from helpers import check_and_resync, pose_err
from stagewise import run_group
from visualslam_android_amd import capi

pytestmark = pytest.mark.gpu


def outlier_marks_equal(o, g, s, tag):
    """the outlier marks of iteration 9 (jni/Tracker.cc:749-756), which assert_tracker_exact does not look at"""
    po, pg = o.points(), g.points(s)
    assert np.array_equal(po["n_in"], pg["n_in"]) and np.array_equal(po["n_out"], pg["n_out"]), tag


@pytest.mark.parametrize("patch", [8, 11])
@pytest.mark.parametrize("group", ["a: nf sweep, 9 streams", "a: nf sweep, 17 streams"])
def test_pose_update_at_every_found_count(group, patch):
    """k_pose at nf = 0, 1, 2, 3, 7..9, 20, 21, 31..33, 63..65, 95..97, 127..129, 255..257, 511, 512 (513 below): chunks of 32 measurements
    with nchunks = 0, 1, 2 mod 3, every residue of the chain's groups of eight calls, the read-ahead past a one-group chunk, both gather
    and iteration batch sizes, the depth update's threshold, and the zero update of a map whose points are all searched and none found;
    batches of 9 and 17 streams (xcd_stream_block's second and third group of eight)."""
    run_group(tc.groups(patch)[group], patch, outlier_marks_equal)


@pytest.mark.parametrize("patch", [8, 11])
def test_median_ties_and_outlier_marks(patch):
    """nf = 513, and two sub-maps (nf = 43 and nf = 303, below and above block_radix_select's 256 threads) whose squared errors hold three
    equal values around rank nf / 2 (block_radix_select against sort + [n / 2]); the outlier marks of the last iteration are compared
    as well.  Two distinct points never give the same error bits, so the tie is made by loading the point at the median rank three
    times (tracker_cases.sub_map takes an index more than once): the copies are searched independently and end on the same corner."""
    run_group(tc.groups(patch)["a+b: nf=513 and the median tie"], patch, outlier_marks_equal)


@pytest.mark.parametrize("patch", [8, 11])
def test_search_at_every_residue_of_patches_per_wavefront(patch):
    """k_searchN with n_search = 1 and every residue modulo 8 (8x8) or 4 (11x11) patches per wavefront: the idle groups of the last wave
    pass through the same ballots and shuffles; 8 streams."""
    run_group(tc.groups(patch)["c: n_search sweep, 8 streams"], patch)


@pytest.mark.parametrize("patch", [8, 11])
def test_pvs_blocks_and_levels_at_their_seams(patch):
    """k_pvs / k_plan with n_points = 1, 255, 256, 257, 513 (full, short and single-point last blocks of 256), a level without any PVS
    entry, and a block that mixes points behind the camera, outside the image and in view (rows of 3, 5 and 13 doubles): points outside
    the PVS report level -1 on both sides (assert_stage_exact compares the PVS membership of every point); 7 streams."""
    cases = tc.groups(patch)["c: n_points sweep, 7 streams"]
    assert len(cases) == 7
    run_group(cases, patch)


@pytest.mark.parametrize("patch", [8, 11])
def test_map_that_fills_max_points(patch):
    """n_points == max_points == 4096 == k_plan's one pass of 16 x 256 points and k_pose's SORT_CAP: the feeder map of 14 source
    keyframes supplies more than 4096 distinct points and is cut to the first 4096; max_points is left at its default."""
    case = tc.full_capacity_case(patch)
    assert case.params(1, patch).max_points == 4096 == len(case.map()["points"])
    run_group([case], patch)


@pytest.mark.parametrize("patch", [8, 11])
@pytest.mark.parametrize("group", ["e: coarse selection", "e: fine selection"])
def test_selection_edges_of_the_plan(group, patch):
    """k_plan's coarse selection (n3 + n2 == coarse_min and + 1; n3 == coarse_max - 1, coarse_max, coarse_max + 1; n2 == more, where the kept
    bug takes level 2 alone, and more + 1; the coarse stage tried with fewer than coarse_min found) and fine selection (nit + n3 above and
    at max_patches_per_frame, the others chopped by one and not chopped), with coarse_min = 4, coarse_max = 12, max_patches_per_frame = 40
    and the fast-moving start of test_coarse_stage_and_pose_recovery.  did_coarse, attempted and found per level and the found sets are
    compared after every stage."""
    run_group(tc.groups(patch)[group], patch)


@pytest.mark.parametrize("patch", [8, 11])
def test_more_coarse_patches_than_one_subpixel_pass(patch):
    """coarse_max = 140: 140 coarse patches carry a sub-pixel budget, k_subpixN's 16 workgroups cover 128 (8x8) or 64 (11x11) per pass"""
    run_group(tc.groups(patch)["f: two sub-pixel passes"], patch)


@pytest.mark.parametrize("patch", [8, 11])
def test_refinement_that_leaves_the_image(patch):
    """163x117 seen from closer: level-3 patches the search finds on corners half a patch from a border, which the first sub-pixel
    iteration un-finds (test_tracker_cases.py counts them in the oracle): k_subpixN clears the found flag and the per-level count"""
    run_group(tc.groups(patch)["f: sub-pixel exit"], patch)


@pytest.mark.parametrize("patch", [8, 11])
@pytest.mark.parametrize("size", tc.SMALL_SIZES)
def test_small_images_and_window_edges(size, patch):
    """48x48 and 131x77 (odd, levels 2 and 3 a few patches wide): search windows that reach the bottom row, windows without a corner in
    range, candidates closer than half a patch to a border (counted on the CPU by test_tracker_cases.py).  The 48x48 batch also holds
    two streams seen from 4x and 7.5x closer, whose points are attempted at level 3 (6x6 pixels, no patch fits) and none found."""
    run_group(tc.groups(patch)["f: %dx%d" % size], patch)


@pytest.mark.parametrize("patch", [8, 11])
def test_idle_streams_at_the_group_boundaries_of_a_17_stream_batch(patch):
    """a stream without a map at position 7, streams that lose tracking (blank frames until lost_frames == 3) at 8 and 16: the 14 mapped
    streams stay == their oracles in every frame, the unmapped stream is only counted, the lost ones follow their oracles and stand still"""
    batch = tc.loss_batch(patch)
    live = [c for c in batch if c is not None]
    w, h = live[0].size
    g = capi.System(live[0].params(len(batch), patch))
    oracles = {}
    for s, c in enumerate(batch):
        if c is not None:
            c.load(g, s)
            oracles[s] = c.oracle(patch)
    blank = np.zeros((h, w), np.uint8)
    frozen = {}
    for t in range(tc.LOSS_FRAMES):
        g.track_frame(np.stack([blank if c is None else c.frame(t) for c in batch]))
        for s, c in enumerate(batch):
            tag = "stream %d frame %d" % (s, t)
            sg = g.state(s)
            if c is None:
                assert (sg.frame, sg.n_keyframes, sg.n_points, sum(sg.attempted), sum(sg.found)) == (t + 1, 0, 0, 0, 0), tag
                continue
            o = oracles[s]
            o.track_frame(c.frame(t))
            so = o.state()
            if c.blank_from is None or t < c.blank_from:
                check_and_resync(o, g, s, tag)
                continue
            assert (so.quality, so.lost_frames, so.frame, so.n_keyframes) == (sg.quality, sg.lost_frames, sg.frame, sg.n_keyframes), tag
            assert list(so.attempted) == list(sg.attempted) and list(so.found) == list(sg.found), tag
            assert np.array_equal(np.array(so.pose[:]), np.array(sg.pose[:])), (tag, pose_err(so.pose, sg.pose))
            if so.lost_frames == 3:                                                       # no tracking any more: nothing of the stream moves
                now = (tuple(sg.pose[:]), tuple(sg.velocity[:]), tuple(sg.attempted[:]), tuple(sg.found[:]), g.points(s)["pos"].tobytes())
                assert frozen.setdefault(s, now) == now, tag
    assert sorted(frozen) == [s for s, k in tc.LOSS_IDLE.items() if k == "lost"] and all(g.state(s).lost_frames == 3 for s in frozen)
    g.close()
