"""GPU parity of the warped template at its own decisions (csrc/patch_dev.h: search_level_and_warp, template_warp_matrix, warp_moved,
template_warp with warp_row_step and warp_pixel_step, warp_sample; called by k_pvs and k_searchN in csrc/track.hip): the search level
within an ulp or two of the determinant of every threshold, the refresh limit of 0.07 within a rounding step of the zoom, roll or swing
that reaches it,
wavefronts of k_searchN that hold kept and re-made templates side by side, templates that sample outside their source image at each of
its four borders, and the bad verdict that a kept template carries on.  The cases come from tests/template_cases.py, built from the oracle
alone; tests/test_template_cases.py asserts on the CPU that the oracle takes each decision both ways on them.  Here the cases of a group
are the streams of one System, each beside its own oracle (stagewise.run_group), the pose of every frame set on both sides with a zero
velocity, and everything is compared with == after each search and pose stage and after the frame: levels (-1 included), searched and
found sets, counters and n_zmssd, and -- through helpers.assert_templates_exact -- the bad and have flags of EVERY point of the map and
the bytes and sums of every template there is, the bad ones that the search skips included."""
import numpy as np
import pytest

import template_cases as tpl
from helpers import assert_templates_exact
from stagewise import run_group

pytestmark = pytest.mark.gpu


def set_pose(o, g, s, case, t):
    case.begin(t, o, g, s)


def templates_and_counts(o, g, s, tag):
    """every point's template state, and no bad template among the attempted patches: attempted counts the points marked searched"""
    assert_templates_exact(o, g, s, tag)
    if ", search " in tag:
        tg, sg = g.point_tracks(s), g.state(s)
        n = int(((tg["level"] >= 0) & (tg["searched"] == 1)).sum())
        assert (sum(sg.attempted) == n) if tag.endswith("search 1") else (sum(sg.attempted) <= n), (tag, list(sg.attempted), n)


def run(cases, patch):
    n_frames = len(cases[0].poses)
    assert all(len(c.poses) == n_frames for c in cases)
    run_group(cases, patch, after_fine_pose=templates_and_counts, n_frames=n_frames, before_frame=set_pose, after_stage=templates_and_counts)


@pytest.mark.parametrize("patch", [8, 11])
@pytest.mark.parametrize("group", ["a: level thresholds", "a: level thresholds, tilted"])
def test_search_level_on_both_sides_of_every_threshold(group, patch):
    """20 streams: for level 0->1, 1->2, 2->3, 3->bad (det > 3 at the cap) and bad->0 (det < 0.25) two points each, on either side of the
    threshold: poses within a few ulps of each other, chosen around two adjacent doubles of the camera distance so that the oracle's
    determinant is the threshold itself (3.0, 0.25: the side `>` and `<` leave alone) in most pairs and one or two ulps past it in the
    partner; plain, and tilted 25 degrees so that the off-diagonal terms of the warp take part.  A product of det contracted into an FMA
    moves it by an ulp and flips the level of the stream at 3 + 1 ulp (run on an oracle so changed: the level of point 27 at det
    3.0000000000000004 is 0 where it was 1, and point 376's, tilted, 2 where it was 3); `>=` for `>` flips every stream at 3.0."""
    run(tpl.groups(patch)[group], patch)


@pytest.mark.parametrize("patch", [8, 11])
def test_refresh_limit_and_mixed_wavefronts(patch):
    """19 streams, two frames.  Sixteen hold one point whose warp, between the frames, moves a column by 0.07 to within a step of the
    pose's rounding: the camera zooms, rolls about the optical axis (the loop of warp_moved leaves at column 1) or swings about the spot
    it looks at (it leaves at column 0); kept on one side -- in five streams at a squared move of exactly 0.07 * 0.07 -- and made again
    on the other, one to seventeen ulps above, and the bytes of the two differ.  Three hold level-0 points in search-list order whose
    templates are kept and re-made in turn (every wavefront of k_searchN takes the refresh branch with half of its lane groups idle in
    it), kept only and re-made only.  A wrong decision leaves the other template's bytes and sums in the cache, which
    assert_templates_exact reads (with dx * dx + dy * dy contracted into an FMA the oracle keeps the template of point 523, rolled, that
    it made again)."""
    run(tpl.groups(patch)["b: refresh limit"], patch)


@pytest.mark.parametrize("patch", [8, 11])
@pytest.mark.parametrize("size", [(tpl.W, tpl.H), tpl.SMALL])
def test_templates_that_leave_their_source_image(size, patch):
    """20 streams, three frames: maps whose points keep patch // 2 - 1 .. patch // 2 + 2 level pixels from the borders of their source
    images, cut down to the points near a border, at zooms 0.6, 0.8, 1.0, 2.0 and tilted.  Hundreds of templates sample outside the
    source at its left, top, right and bottom border: warp_sample returns 0 there and counts, the template is bad, the point is not
    searched and not counted in attempted -- and its flag, its bytes with the zeros and its sums == the oracle's.  The second frame keeps
    the template and its verdict, the third (1.5 times closer) makes it again, for many points with every sample inside.  A comparison of
    warp_sample taken the other way reads a pixel where the oracle writes 0 (or the reverse) and flips the verdict."""
    run(tpl.groups(patch)["c: source border, %dx%d" % size], patch)


@pytest.mark.parametrize("patch", [8, 11])
def test_bad_scale_sticks_to_a_kept_template(patch):
    """3 streams, four frames: z0, 0.99 z0, z0, 1.5 z0 with z0 = 0.50, 0.52, 0.54.  Points searched in frame 0 fall below det = 0.25 in
    frame 1 (k_pvs sets the bad flag), are back in the potentially visible set in frame 2 with a warp that has not moved by 0.07 -- the
    kept template keeps the verdict, the point is not searched -- and are made again and searched in frame 3.  A k_pvs that did not set
    the flag, or a k_searchN that cleared it without making the template, would search them in frame 2."""
    run(tpl.groups(patch)["d: sticky bad scale"], patch)
