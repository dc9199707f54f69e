"""CPU check of tests/grow_cases.py: the oracle alone, run on every case of tests/test_gpu_grow_counts.py (one tracked frame that becomes a
keyframe, the four idle jobs, a second tracked frame), reaches the counts at which csrc/mapgrow.hip forks.  A case that misses a condition
is a broken case: the sub-map has to change, not the condition.  Run with -s to see the counts per stream.

Reached: per-level candidate counts 0, 1, 2, 3, multiples of 4 and every residue modulo the four wavefronts of a chunk; level 3 (the first
level grow_on_keyframe processes) with candidates and a new point; the reject stages 0, 1, 2, 5, 6, 7; ballots with more survivors than
one step of k_epipolar scores, up to four steps (the winner in the second step at 8x8, in every step at 11x11); survivors in several blocks of 64; chunks accepted whole and in part; re-finds of the new
keyframe measured at every level; search windows longer than 64 and 128 list entries; hundreds of kept templates in ReFindNewlyMade, some
with a bad verdict.

Group e: stage 3 beside accepted calls at levels 0 to 2 (a target keyframe turned about its vertical axis, both ways); an equal-ZMSSD tie
at the minimum of an accepted call, the two rivals in one step of the ballot (the first step at both patch sizes, a later one at 11x11),
in two steps and in two ballots (a block of texture repeated inside the target keyframe's image); the start-depth clip, on hundreds of
calls of which a few are accepted (a camera zoomed out and tilted) and with a small dirn[2] (a tilted camera, the target turned 80
degrees and ahead of it); ReFind_Common's return "behind".  Its returns "outside radius" and "outside image" are reached by group b, in the new keyframe and in the
map's keyframes (the oracle's re-find log records the calls that return before the template as outcomes of their own).

Group f: templates that sample outside their source image (nOutside != 0), made anew in ReFindInSingleKeyFrame on a map whose points keep
half a patch from the borders of their source images, and kept with that verdict in ReFindNewlyMade by map keyframes that see the new
keyframe from far to the side.

Not reached: at 8x8 a winner scored in the third or fourth step of its ballot (test_group_a prints the steps).  Not reached, and asserted to be
absent so that a change that reaches one is noticed: stage 3, an equal-ZMSSD tie at the minimum and the start-depth clip outside group e,
stage 4; of ReFind_Common's returns, the invalid projection and a search window outside the rows of its level (the module docstring of
grow_cases.py gives the reason for each; test_refind_window_never_lies_outside_its_level runs the oracle's FindPatchCoarse at the
image's edges for the last one); a kept template
in ReFindFromFailureQueue (the queue is sorted by keyframe first, neighbours are different points) and one kept across two jobs."""
import numpy as np
import pytest

import grow_cases as gc
import oracle.binding as orc

OUTCOME = {name: i for i, name in enumerate(orc.OracleSystem.REFIND_OUTCOMES)}
JOB = {name: i for i, name in enumerate(orc.OracleSystem.REFIND_JOBS)}
EARLY = orc.OracleSystem.REFIND_EARLY                            # outcomes from here on returned before the template


def template_calls(rf):
    """the records of the calls that reached the template"""
    m = rf["outcome"] < EARLY
    return {k: v[m] for k, v in rf.items()}


def describe(case, r, patch):
    d, rf = r.detail, r.refind
    npw = gc.PATCHES_PER_STEP[patch]
    line = "  %s: points %d -> %d, candidates per level %s, stages %s" % (case.name, r.n0, r.n_points, r.per_level(), r.stages())
    if len(r.log):
        line += "; survivors in one block: > %d in %d calls, most %d; in >= 2 blocks %d calls; chunks whole / mixed %s" % (
            npw, int((d["block_max"] > npw).sum()), int(d["block_max"].max()), int((d["blocks"] >= 2).sum()), r.chunks())
    for job, name in enumerate(orc.OracleSystem.REFIND_JOBS):
        jm = rf["job"] == job
        if jm.any():
            line += "\n      %s: early returns %s" % (name, {k: int((jm & (rf["outcome"] == v)).sum()) for k, v in OUTCOME.items() if v >= EARLY})
        jm = jm & (rf["outcome"] < EARLY)
        if jm.any():
            line += "\n      %s: %d template calls, measured per level %s, outcomes %s, kept templates %d (bad %d), longest window %d" % (
                name, int(jm.sum()), [int((jm & (rf["outcome"] == 0) & (rf["level"] == l)).sum()) for l in range(4)],
                {k: int((jm & (rf["outcome"] == v)).sum()) for k, v in OUTCOME.items() if v < EARLY}, int((jm & (rf["hit"] == 1)).sum()),
                int((jm & (rf["hit"] == 1) & (rf["outcome"] == OUTCOME["template bad"])).sum()), int(rf["span"][jm].max()))
    return line + "\n      idle: %s; second frame: quality %d, found %s" % (r.idle, r.quality1, r.found1)


def records(group, patch, verbose=True):
    cases = gc.groups(patch)[group]
    assert 1 <= len(cases) <= 11
    out = [(c, gc.record(c, patch)) for c in cases if c.has_map]
    if verbose:
        print("\n[%s, %dx%d patches] %d streams" % (group, patch, patch, len(cases)))
        for c, r in out:
            print(describe(c, r, patch))
    for c, r in out:                                             # every stream with a map tracks both frames; the growing ones add one keyframe
        assert (r.kf_added, r.kf_added1, r.n_keyframes - r.kf0) == (int(c.grows), 0, int(c.grows)), c.name
        assert r.quality0 == r.quality1 == 2 and r.n_points1 == r.n_points, c.name
        if c.border is not None and r.idle["ba_all"] == 0:
            # group f at 8x8 and zoom 0.8: the recent bundle adjustment ends its job unconverged, so the full one and both re-find jobs find
            # their gate shut (MapMaker::run, jni/MapMaker.cc:97-112) and the new points wait in their queue: the gate's other answer
            assert r.idle["ba_recent_idle"] == 1 and r.idle["refound_new"] == r.idle["refound_failed"] == 0 and r.idle["new_queue"] == r.n_points - r.n0, (c.name, r.idle)
        else:
            assert r.idle["new_queue"] == 0 and r.idle["failure_queue"] <= 8192, (c.name, r.idle)
        for k in (3, 4):                                         # the unreached stages stay unreached (stage 3: outside group e's turned targets)
            if not (k == 3 and c.turned_kf is not None):
                assert r.stages().get(k, 0) == 0, (c.name, r.stages())
        assert (r.detail["tie"].sum() == 0 or c.repeat is not None) and (r.detail["clipped"].sum() == 0 or "clip_stages" in c.target), c.name
        assert (r.refind["outcome"] != OUTCOME["window outside"]).all() and (r.refind["outcome"] != OUTCOME["invalid projection"]).all(), c.name
        if not c.behind:
            assert (r.refind["outcome"] != OUTCOME["behind"]).all(), c.name
    return out


@pytest.mark.parametrize("patch", [8, 11])
def test_group_a_reaches_the_epipolar_counts(patch):
    recs = records("a: epipolar counts", patch)
    assert [c.name for c in gc.group_a() if not c.grows] == ["no keyframe request", "no map"]
    for c, r in recs:
        if not c.grows:
            assert len(r.log) == 0 and r.n_points == r.n0 and len(r.refind["job"]) == 0 and not any(r.idle.values()), c.name
    counts = [n for _c, r in recs if _c.grows for n in r.per_level()]
    assert {0, 1, 2, 3} <= set(counts), counts
    assert any(n >= 4 and n % gc.GROW_WAVES == 0 for n in counts), counts
    assert {n % gc.GROW_WAVES for n in counts if n > 4} == set(range(gc.GROW_WAVES)), counts
    assert max(r.per_level()[3] for _c, r in recs) >= 4
    assert any(((r.log[:, 0] == 3) & (r.log[:, 2] == 0)).any() for _c, r in recs if len(r.log))                  # a level-3 point is added
    stages = set().union(*[set(r.stages()) for _c, r in recs])
    assert stages == {0, 5, 6}, stages
    npw = gc.PATCHES_PER_STEP[patch]
    block_max = np.concatenate([r.detail["block_max"] for _c, r in recs])
    blocks = np.concatenate([r.detail["blocks"] for _c, r in recs])
    assert (block_max > npw).sum() >= 10 and (block_max > 2 * npw).sum() >= 1 and (blocks >= 2).sum() >= 10
    # the step of its ballot in which the winning corner is scored: at 11x11 the third and fourth steps hold winners; at 8x8 no sub-map, stride
    # or texture tried puts one beyond the second step (the winner is among the first 16 survivors of its block), so there the later steps
    # only ever score losers -- the count is printed, and asserted where it is reached
    won = np.concatenate([r.detail["best_rank"][np.isin(r.log[:, 2], (0, 6, 7))] for _c, r in recs]) // npw
    print("  step of the ballot that scores the winner: %s" % {int(k): int((won == k).sum()) for k in np.unique(won)})
    assert (won >= 1).sum() >= 10 and (patch == 8 or (won >= 2).sum() >= 10)
    whole, mixed = (sum(x) for x in zip(*[r.chunks() for _c, r in recs]))
    assert whole >= 1 and mixed >= 1
    print("  over the group: %d calls; calls with > %d survivors in a block %d, needing >= 3 steps %d, with survivors in >= 2 blocks %d; chunks whole %d, mixed %d"
          % (len(block_max), npw, int((block_max > npw).sum()), int((block_max > 2 * npw).sum()), int((blocks >= 2).sum()), whole, mixed))


def _cat(recs, key):
    return np.concatenate([r.refind[key] for _c, r in recs])


def cross_job_hits(rf):
    """kept templates whose previous template call belonged to another run of a job"""
    rf = template_calls(rf)
    h = np.flatnonzero(rf["hit"] == 1)
    assert (h > 0).all() and (rf["pt"][h] == rf["pt"][h - 1]).all()              # a kept template follows a call for the same point
    return int((rf["run"][h] != rf["run"][h - 1]).sum())


@pytest.mark.parametrize("patch", [8, 11])
def test_group_b_reaches_the_refind_counts(patch):
    recs = records("b: re-find", patch)
    job, level, outcome, span, hit = (_cat(recs, k) for k in ("job", "level", "outcome", "span", "hit"))
    new_kf = job == JOB["single keyframe"]
    for l in range(4):                                                             # re-finds of the new keyframe measured at every level
        assert (new_kf & (outcome == OUTCOME["measured"]) & (level == l)).sum() >= 1, l
    assert (span > 64).sum() >= 1 and (span > 128).sum() >= 1
    assert (new_kf & (span > 128)).sum() >= 1 and ((job == JOB["newly made"]) & (span > 128)).sum() >= 1     # by the row table and by the binary search
    for name in ("measured", "template bad", "not found"):                         # every early return the scene reaches ("window outside": none)
        assert (outcome == OUTCOME[name]).sum() >= 1, name
    # the returns before the template: the radius and the image border in the new keyframe and in the map's keyframes; no point lies behind a
    # keyframe (group e), and the radius test leaves nothing for the invalid projection (module docstring of grow_cases.py)
    for name in ("outside radius", "outside image"):
        assert (new_kf & (outcome == OUTCOME[name])).sum() >= 10 and ((job == JOB["newly made"]) & (outcome == OUTCOME[name])).sum() >= 1, name
    assert (outcome == OUTCOME["behind"]).sum() == 0 and (outcome == OUTCOME["invalid projection"]).sum() == 0
    assert ((level == -1) == (outcome >= EARLY)).all() and (hit[outcome >= EARLY] == 0).all() and (span[outcome >= EARLY] == -1).all()
    both = recs + records("a: epipolar counts", patch, verbose=False)
    job, outcome, hit = (_cat(both, k) for k in ("job", "outcome", "hit"))
    newly = job == JOB["newly made"]
    n_hits, n_bad = int((newly & (hit == 1)).sum()), int((newly & (hit == 1) & (outcome == OUTCOME["template bad"])).sum())
    fq_hits = int(((job == JOB["failure queue"]) & (hit == 1)).sum())
    cross = sum(cross_job_hits(r.refind) for _c, r in both)
    print("  groups a and b: kept templates in ReFindNewlyMade %d (bad verdict %d), in ReFindFromFailureQueue %d, kept across two jobs %d" % (n_hits, n_bad, fq_hits, cross))
    assert n_hits >= 100 and n_bad >= 1
    assert (new_kf_hits := int(((job == JOB["single keyframe"]) & (hit == 1)).sum())) == 0, new_kf_hits      # k_refind's comment: never the same point twice in a row
    assert fq_hits == 0 and cross == 0           # RefindCache starts empty per point and per queue entry: a hit here would be one the device cannot have


@pytest.mark.parametrize("patch", [8, 11])
@pytest.mark.parametrize("which", ["c: stage 1", "c: stage 2"])
def test_group_c_rejects_every_call_at_one_stage(which, patch):
    (c, r), = records(which, patch)
    assert len(r.log) >= 100 and (r.log[:, 2] == c.target["stage"]).all(), r.stages()
    assert r.n_points == r.n0 and sum(n > 0 for n in r.per_level()) == 4


@pytest.mark.parametrize("patch", [8, 11])
def test_group_d_fills_the_map(patch):
    recs = records("d: map capacity", patch)
    assert [c.target["full_level"] for c, _r in recs] == [0, 1, 0, None, 0]
    for c, r in recs:
        assert r.n0 < gc.MAX_POINTS == r.n_points == r.n_points1, (c.name, r.n0, r.n_points)
        assert sum(r.attempted1) > 0 and r.quality1 == 2, c.name                   # the second frame tracks the full map
        ff, st = gc.first_full(r), r.log[:, 2]
        if c.target["full_level"] is None:                                         # the last accepted candidate takes the last slot
            assert ff is None and (st == 0).sum() == gc.MAX_POINTS - r.n0, c.name
            continue
        last, fill = int(np.flatnonzero(st == 0)[-1]), gc.fill_level(r)            # the call that takes the last slot
        assert ff is not None and fill == c.target["full_level"], (c.name, fill, ff)
        assert (st[:last + 1] != 7).all() and (st[:last + 1] == 0).sum() == gc.MAX_POINTS - r.n0 and (st[last + 1:] != 0).all(), c.name
        # up to the end of the level that fills the map the candidates are those of the run without a limit (the later levels are thinned by
        # fewer new points): there stage 7 is exactly what that run accepts
        u = gc.record(c, patch, max_points=0).log
        end = last + 1 + int((r.log[last + 1:, 0] == fill).sum())
        assert np.array_equal(u[:end, :2], r.log[:end, :2]) and np.array_equal(np.where(st[:end] == 7, 0, st[:end]), u[:end, 2]), c.name
        assert (st == 7).sum() >= 1 and (r.log[st == 7, 0] == ff[0]).any(), c.name
        if c.target.get("mid_chunk"):
            assert ff[1] % gc.GROW_WAVES != 0, (c.name, ff)
        print("      the map fills during level %d; first call on a full map: level %d, candidate %d of the level (wavefront %d of its chunk); levels with stage 7: %s" % (fill, ff[0], ff[1], ff[1] % gc.GROW_WAVES, sorted(set(r.log[st == 7, 0].tolist()))))


@pytest.mark.parametrize("patch", [8, 11])
def test_group_e_reaches_stage_3_and_the_early_return_behind(patch):
    recs = records("e: epipolar exits", patch)
    steps = []
    for c, r in recs:
        print("      %s: stages per level %s, ties %d, clips %d" % (c.name, {l: r.stages(l) for l in range(4)}, int(r.detail["tie"].sum()), int(r.detail["clipped"].sum())))
        outcome = r.refind["outcome"]
        if "stage3_levels" in c.target:
            for l in c.target["stage3_levels"]:                                    # stage 3 and an accepted call in the same level
                st = r.stages(l)
                assert st.get(3, 0) >= 1 and st.get(0, 0) >= 1, (c.name, l, st)
            assert r.stages().get(3, 0) >= 10 and r.n_points > r.n0, (c.name, r.stages())
            # the far side is one half of the image: stage 3 on one side of the candidates' mean x, accepted calls on the other
            x = (r.log[:, 1] & 0xFFFF) * (1 << r.log[:, 0])
            far, near = x[r.log[:, 2] == 3], x[r.log[:, 2] == 0]
            assert (far.mean() - near.mean()) * c.turned_kf[0] > 0, (c.name, far.mean(), near.mean())
        elif c.turned_kf is None:
            assert r.stages().get(3, 0) == 0, (c.name, r.stages())
        if c.repeat is not None:                                                   # an equal minimum on an accepted call, the rivals where TIES says
            t = np.flatnonzero((r.detail["tie"] == 1) & (r.log[:, 2] == 0))
            assert len(t) == 1 and int(r.detail["tie"].sum()) == 1, (c.name, t)
            got = tuple(int(r.detail[k][t[0]]) for k in ("best_rank", "rival_rank", "rival_same_block"))
            assert got == c.target["tie"][patch], (c.name, got)
            steps.append((got[0] // gc.PATCHES_PER_STEP[patch], got[1] // gc.PATCHES_PER_STEP[patch], got[2]))
            base = gc.record(gc.group_e()[2], patch)                                # without the block the call has no rival (the behind stream: same sub-map and parameters)
            i = np.flatnonzero((base.log[:, :2] == r.log[t[0], :2]).all(1))
            assert len(i) == 1 and base.log[i[0], 2] == 0 and base.detail["tie"][i[0]] == 0, c.name
        if "clip_stages" in c.target:                                              # clipped lines, and what became of them
            cl = r.detail["clipped"] == 1
            for st in c.target["clip_stages"]:
                assert (cl & (r.log[:, 2] == st)).sum() >= 1, (c.name, st, np.bincount(r.log[cl, 2]).tolist())
            assert (~cl & (r.log[:, 2] != 1)).sum() >= 1 or c.zoom is not None, c.name
        if c.behind:
            m = outcome == OUTCOME["behind"]
            assert m.sum() == c.target["behind"] and (r.refind["job"][m] == JOB["single keyframe"]).all(), (c.name, int(m.sum()))
            assert sorted(r.refind["pt"][m].tolist()) == list(range(r.n0 - c.behind, r.n0)), c.name
    assert sum("stage3_levels" in c.target for c, _r in recs) == 2 and sum("clip_stages" in c.target for c, _r in recs) == 2 and sum(c.behind > 0 for c, _r in recs) == 1
    # the rivals of a tie: in two steps of one ballot, in two ballots, and (8x8) in one step
    assert any(a != b and same for a, b, same in steps) and any(not same for _a, _b, same in steps), steps
    assert any(a == b == 0 and same for a, b, same in steps) and (patch == 8 or any(a == b == 1 and same for a, b, same in steps)), steps   # one step: the first, and (11x11) a later one


@pytest.mark.parametrize("patch", [8, 11])
def test_group_f_makes_and_keeps_templates_that_leave_their_source(patch):
    """the border map: templates made anew (hit == 0) that end "template bad" -- the verdict of nOutside alone, a template made anew
    replaces what the scale said (jni/PatchFinder.cc:105-117) -- and kept templates (hit == 1) whose bad verdict is the one nOutside gave
    when the template was made"""
    recs = records("f: border map", patch)
    assert len(recs) == len(gc.F_ZOOMS) + len(gc.F_OBLIQUE) and all(c.border == patch // 2 and c.pkw == gc.B_PKW for c, _r in recs)
    bad = OUTCOME["template bad"]
    made, kept, total = {}, {}, [0, 0]
    for c, r in recs:
        rf = r.refind
        made[c.name] = {name: int(((rf["job"] == j) & (rf["hit"] == 0) & (rf["outcome"] == bad)).sum()) for name, j in JOB.items()}
        kept[c.name] = gc.kept_outside_verdicts(rf, bad)
        total[0] += sum(made[c.name].values()); total[1] += kept[c.name]
        print("      %s: templates made bad per job %s; kept with the bad verdict of nOutside %d (kept and bad in all %d)" % (
            c.name, made[c.name], kept[c.name], int(((rf["hit"] == 1) & (rf["outcome"] == bad)).sum())))
    assert total[0] >= 8 and total[1] >= 1, total
    assert all(sum(made[c.name].values()) >= 8 for c, _r in recs[:len(gc.F_ZOOMS)]), made      # every zoom of the full border map on its own
    assert all(kept[c.name] >= 1 for c, _r in recs[len(gc.F_ZOOMS):]), kept                   # both streams with the keyframes to the side
    # without the narrow border the same streams never leave the source in ReFindInSingleKeyFrame: the branch is the border's
    plain = gc.record(gc.Case("border 10", None, gc.B_PKW, zoom=gc.F_ZOOMS[0]), patch).refind
    assert ((plain["job"] == JOB["single keyframe"]) & (plain["outcome"] == bad)).sum() < made[recs[0][0].name]["single keyframe"]


def test_refind_window_never_lies_outside_its_level():
    """the argument of grow_cases' docstring, on the code that runs: once :996 has bounded the projection by the image, the oracle's
    FindPatchCoarse (range 4, as ReFind_Common calls it) finds its window inside the level at every level -- a span, never -1 -- at
    320x240 and at the odd size of search_trip_cases.py; one step outside the image in y the window does leave the small levels, so the
    -1 is not out of this call's reach"""
    rng = np.random.RandomState(3)
    for w0, h0 in ((gc.W, gc.H), (131, 77)):
        img = rng.randint(0, 256, (h0, w0)).astype(np.uint8)
        for l in range(4):
            for im_y in (0.0, 0.5, h0 / 2.0, np.nextafter(float(h0), 0.0), float(h0)):     # :996 lets 0 <= im_y <= h0 through
                for im_x in (0.0, w0 / 2.0, float(w0)):
                    assert orc.find_coarse_span(img, l, im_x, im_y) >= 0, (w0, h0, l, im_x, im_y)
        assert orc.find_coarse_span(img, 3, w0 / 2.0, h0 + 16.0) == -1 and orc.find_coarse_span(img, 0, w0 / 2.0, h0 + 5.0) == -1
