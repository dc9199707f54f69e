"""CPU check of tests/tracker_cases.py: the oracle alone, run on every case of tests/test_gpu_tracker_counts.py with the stage calls,
reaches the case's targets EXACTLY -- n_points, the found count entering the fine pose stage, the per-level attempted counts, did_coarse,
the number of searched patches.  A case that misses is a broken case: the selection or the scene has to change, not the target.
Run with -s to see, per group, the targets and the sub-map sizes that reached them."""
import numpy as np
import pytest

import tracker_cases as tc


def run_stages(case, patch):
    """the oracle's first frame on the case, cut at the stages: the records after the coarse search and entering the fine pose stage"""
    o = case.oracle(patch)
    o.frame_begin(case.frame(0))
    o.search_stage(0)
    coarse = tc.stage_record(o)
    o.pose_stage(0); o.search_stage(1)
    fine = tc.stage_record(o)
    o.pose_stage(1); o.frame_end()
    o.close()
    return coarse, fine


def check_targets(case, patch):
    coarse, fine = run_stages(case, patch)
    t = case.target
    assert fine["n_points"] == len(case.map()["points"])
    for key in ("n_points", "nf", "attempted", "did_coarse"):
        if key in t:
            assert fine[key] == t[key], (case.name, key, fine[key], t[key])
    if "attempted_sum" in t:
        assert sum(fine["attempted"]) == t["attempted_sum"], (case.name, fine["attempted"], t["attempted_sum"])
    if "coarse_attempted" in t:
        assert coarse["attempted"] == t["coarse_attempted"], (case.name, coarse["attempted"], t["coarse_attempted"])
    if "n_coarse_min" in t:
        assert sum(coarse["attempted"]) >= t["n_coarse_min"], (case.name, coarse["attempted"])
        late = tc.second_pass_refined(coarse["tracks"], patch)
        print("  coarse patches beyond k_subpixN's first pass, found and sub-pixel refined: %d" % late)
        assert late >= 1, case.name
    if t.get("level3_unfound"):
        assert fine["attempted"][3] > 0 and fine["found_counts"][3] == 0, (case.name, fine["attempted"], fine["found_counts"])
    return "%s: n_points %d, attempted %s (coarse %s), nf %d, did_coarse %d" % (case.name, fine["n_points"], fine["attempted"], coarse["attempted"], fine["nf"], fine["did_coarse"])


@pytest.mark.parametrize("patch", [8, 11])
@pytest.mark.parametrize("group", tc.GROUP_NAMES)
def test_every_case_reaches_its_targets_in_the_oracle(group, patch):
    cases = tc.groups(patch)[group]
    assert 1 <= len(cases) <= 17
    print("\n[%s, %dx%d patches] %d streams" % (group, patch, patch, len(cases)))
    for c in cases:
        print("  " + check_targets(c, patch))


@pytest.mark.parametrize("patch", [8, 11])
def test_sweeps_hold_every_listed_target(patch):
    assert tuple(c.target["nf"] for c in tc.nf_cases(patch)) == tc.NF_TARGETS
    ppw = tc.PATCHES_PER_WAVE[patch]
    ns = [c.target["attempted_sum"] for c in tc.n_search_cases(patch)]
    assert {n % ppw for n in ns} == set(range(ppw)) and 1 in ns
    assert [c.target["n_points"] for c in tc.n_points_cases(patch)[:len(tc.N_POINTS_TARGETS)]] == list(tc.N_POINTS_TARGETS)
    assert {len(g) for g in tc.groups(patch).values()} >= {7, 8, 9, 17}
    assert len(tc.loss_batch(patch)) == 17


@pytest.mark.parametrize("patch", [8, 11])
@pytest.mark.parametrize("n_base", tc.TIE_BASES)
def test_median_tie_case_has_equal_errors_around_the_rank(n_base, patch):
    """the oracle's squared errors entering FindSigmaSquared (recomputed from point_tracks) hold at least three equal values that
    straddle rank nf / 2"""
    case = tc.tie_case(patch, n_base)
    _coarse, fine = run_stages(case, patch)
    e2 = tc.squared_errors(fine["tracks"])
    assert len(e2) == case.target["nf"]
    n_equal, straddles = tc.tie_run(e2)
    print("\nmedian tie, %dx%d: nf %d, %d equal values at rank %d" % (patch, patch, len(e2), n_equal, len(e2) // 2))
    assert n_equal >= 3 and straddles


@pytest.mark.parametrize("patch", [8, 11])
def test_mixed_block_holds_all_three_row_kinds(patch):
    """one k_pvs block with points behind the camera or beyond the largest radius (3 doubles), projected outside the image (5) and in the
    image (13); the oracle's PVS is a subset of the last"""
    case = tc.mixed_block_case(patch)
    rows = case.target["rows"]
    print("\nmixed block, %dx%d: %d points, rows of 3 / 5 / 13 doubles: %s" % (patch, patch, case.target["n_points"], rows))
    assert case.target["n_points"] <= 256 and min(rows) >= 5, rows
    _coarse, fine = run_stages(case, patch)
    kinds = tc.row_kinds(case, patch)
    lv = fine["tracks"]["level"]
    assert (lv[kinds != 13] == -1).all() and (lv >= 0).sum() > 0


@pytest.mark.parametrize("patch", [8, 11])
def test_loss_batch_streams_lose_tracking_on_the_expected_frame(patch):
    batch = tc.loss_batch(patch)
    assert [s for s, c in enumerate(batch) if c is None or c.blank_from is not None] == sorted(tc.LOSS_IDLE)
    for s, kind in tc.LOSS_IDLE.items():
        if kind != "lost":
            continue
        o = batch[s].oracle(patch)
        lost = []
        for t in range(tc.LOSS_FRAMES):
            o.track_frame(batch[s].frame(t))
            lost.append(o.state().lost_frames)
        assert lost == [0, 0, 1, 2, 3, 3, 3], (s, lost)
        o.close()


@pytest.mark.parametrize("patch", [8, 11])
@pytest.mark.parametrize("size", tc.SMALL_SIZES)
def test_small_sizes_visit_the_search_window_edges(size, patch):
    """the oracle's search meets windows that reach the bottom row of their level and candidate corners closer than half a patch to a border
    at both sizes; at 131x77 one map and pose also hold windows without a corner in range (48x48 is too crowded for one)"""
    n = tc.window_edges(tc.small_size_case(patch, *size), patch)
    print("\n%dx%d, %dx%d patches: windows at the bottom row %d, without a corner %d, with a border candidate %d" % (size + (patch, patch, n["bottom"], n["empty"], n["border"])))
    assert all(n[k] > 0 for k in tc.WINDOW_EDGES[size]), n


@pytest.mark.parametrize("patch", [8, 11])
def test_subpixel_exit_case_unfinds_a_patch_at_a_border(patch):
    """the search finds the patch (found == 1 with a sub-pixel budget of 0), the refinement un-finds it (found == 0 with the budget), and its
    corner lies where the first sub-pixel iteration is outside IterateSubPix's border: the refinement left the image"""
    case = tc.subpix_exit_case(patch)
    gone, at_border = tc.subpix_exits(case, patch)
    print("\n%s, %dx%d patches: found by the search and un-found by sub-pixel %d, of these at a border %d" % (case.name, patch, patch, len(gone), len(at_border)))
    assert len(at_border) == case.target["n_exits"] >= 1 and set(at_border) <= set(gone)
