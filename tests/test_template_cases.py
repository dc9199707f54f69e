"""CPU check of tests/template_cases.py: the oracle alone, run on every case of tests/test_gpu_template_edges.py with the stage calls and the
frames the device gets, takes the decision each case was built for -- the search level on both sides of every straddle, the kept and the
re-made template on both sides of the refresh limit, templates with samples outside their source at every border of it, the bad scale
that outlives its cause.  A case that misses is a broken case: the choice has to change, not the target.  Run with -s to see the straddles
with their two distances, the per-side counts of the border group, the wavefronts of the refresh group and the sticky counts."""
import numpy as np
import pytest

import template_cases as tpl


def adjacent(lo, hi):
    return lo < hi and np.nextafter(lo, np.inf) == hi


@pytest.mark.parametrize("patch", [8, 11])
@pytest.mark.parametrize("group", ["a: level thresholds", "a: level thresholds, tilted"])
def test_every_level_threshold_is_straddled_by_adjacent_distances(group, patch):
    """per decision of search_level_and_warp at least one point (two where the scene has them) whose verdict differs between two adjacent
    doubles of the zoom; a verdict of -1 is the scale's: the point projects into the image and its finder says bad before any template"""
    cases = tpl.groups(patch)[group]
    assert len(cases) % 2 == 0 and 2 * len(tpl.TRANSITIONS) <= len(cases) <= 40
    seen, ulps = {}, []
    print("\n[%s, %dx%d patches] %d streams" % (group, patch, patch, len(cases)))
    for far, near in zip(cases[0::2], cases[1::2]):
        t = far.target
        a, b = t["transition"]
        thr = tpl.threshold(a)
        assert near.target["transition"] == (a, b) and near.target["point"] == t["point"] and t["pair"] == near.target["pair"]
        assert adjacent(*t["pair"]), t["pair"]
        got = []
        for c in (far, near):
            r = tpl.run(c, patch)[0]
            got.append(int(r["pvs_level"][0]))
            assert tpl.level_value(r["warp0"], a) == c.target["value"], c.name        # the determinant the choice was made on is this run's
            assert r["pvs_have"][0] == 0                               # a first frame: nothing kept
            assert int(r["pvs_bad"][0]) == int(got[-1] == -1), (c.name, got)
            assert tpl.in_view(c.size, c.poses[0], c.map()["points"][0]["pos"]), c.name
            # (near det = 0.25 a template covers twice its size in the source: an 11x11 one can leave it past the map's 10-pixel border)
            assert (r["tracks"]["searched"][0] == 1) == (got[-1] >= 0 and r["tmpl"]["bad"][0] == 0) and sum(r["attempted"]) == int((r["tracks"]["searched"] == 1).sum()), c.name
        assert got == [a, b] == [far.target["verdict"], near.target["verdict"]], (far.name, got)
        vf, vn = far.target["value"], near.target["value"]
        assert (vf <= thr < vn) if a >= 0 else (vf < thr <= vn), (far.name, vf, vn)      # det > 3 leaves the level, det < 0.25 is bad
        assert np.abs(far.poses[0] - near.poses[0]).max() <= 2 * tpl.NUDGE * np.spacing(np.abs(far.poses[0]).max())
        ulps.append(((vf - thr) / np.spacing(thr), (vn - thr) / np.spacing(thr)))
        seen[(a, b)] = seen.get((a, b), 0) + 1
        print("  %d -> %d: point %d (source level %d) between z = %r and %r; streams with det = %r (%+.1f ulp of %g) and %r (%+.1f ulp)" % (
            a, b, t["point"], far.map()["points"][0]["level"], t["pair"][0], t["pair"][1], vf, ulps[-1][0], thr, vn, ulps[-1][1]))
    assert set(seen) == set(tpl.TRANSITIONS) and min(seen.values()) >= 1, seen
    assert sum(seen.values()) >= 2 * len(tpl.TRANSITIONS) - 2, seen
    # the two streams of a pair stand a few ulps of the determinant apart, and at least half of the pairs hold the threshold itself on one side
    assert max(n - f for f, n in ulps) <= 8 and sum(f == 0 or n == 0 for f, n in ulps) >= len(ulps) // 2, ulps


def _first_frame_template(case, patch):
    """what a fresh oracle makes at the pose of the case's second frame"""
    c = tpl.SeqCase(case.name, case.size, case.keep, case.poses[1:2], border=case.border)
    return tpl.run(c, patch)[0]["tmpl"]["tmpl"]


@pytest.mark.parametrize("patch", [8, 11])
def test_refresh_limit_is_straddled_and_the_wavefronts_mix(patch):
    """frame 1 keeps the template of frame 0 on one side of each pair and holds the one a fresh oracle makes at its pose on the other; the
    two differ in bytes, so a wrong decision shows.  The three wavefront streams hold what their names say, at one level."""
    cases = tpl.groups(patch)["b: refresh limit"]
    assert len(cases) == 2 * sum(n for _k, n in tpl.REFRESH_KINDS) + 3
    print("\n[b: refresh limit, %dx%d patches] %d streams" % (patch, patch, len(cases)))
    n_pairs, columns, ulps = {k: 0 for k, _n in tpl.REFRESH_KINDS}, set(), []
    for c in cases:
        r0, r1 = tpl.run(c, patch)
        t0, t1, fresh = r0["tmpl"]["tmpl"], r1["tmpl"]["tmpl"], _first_frame_template(c, patch)
        kept = (t0 == t1).all((1, 2))
        assert kept.tolist() == c.target["kept"], (c.name, kept.tolist())
        assert not (t0 == fresh).all((1, 2)).any(), c.name               # keeping and making again never give the same bytes here
        assert (t1[~kept] == fresh[~kept]).all(), c.name
        for r in (r0, r1):
            assert (r["tracks"]["searched"] == 1).all() and (r["tmpl"]["bad"] == 0).all() and (r["tmpl"]["have"] == 1).all(), c.name
        assert np.array_equal(r0["tracks"]["level"], r1["tracks"]["level"]), c.name
        if "pair" in c.target:
            assert adjacent(*c.target["pair"]), c.target["pair"]
            n_pairs[c.target["kind"]] += 1
            mv = tpl.column_moves(r1["warp0"], int(r1["tracks"]["level"][0]), r0["last_warp0"])
            assert mv == c.target["moves"] and (max(mv) > tpl.REFRESH_LIMIT2) == (not kept[0]), (c.name, mv)     # the moves the choice was made on are this run's
            first = next((i for i in range(2) if mv[i] > tpl.REFRESH_LIMIT2), None)
            columns.add((c.target["kind"], first))
            ulps.append((max(mv) - tpl.REFRESH_LIMIT2) / np.spacing(tpl.REFRESH_LIMIT2))
            print("  %s: point %d between %r and %r; %s with column moves %r (%+.1f ulp of 0.07^2)%s" % (c.target["kind"], c.target["point"], c.target["pair"][0], c.target["pair"][1],
                  "kept" if kept[0] else "made again", mv, ulps[-1], "" if first is None else ", the loop leaves at column %d" % first))
        else:
            assert len(set(r1["tracks"]["level"].tolist())) == 1 and len(kept) % tpl.PPW[patch] == 0, c.name
            waves = kept.reshape(-1, tpl.PPW[patch])
            print("  %s: %d wavefronts of %d patches at level %d, kept per wavefront %s" % (c.name, len(waves), tpl.PPW[patch], r1["tracks"]["level"][0], waves.sum(1).tolist()))
    assert n_pairs == {k: 2 * n for k, n in tpl.REFRESH_KINDS}
    # every stream within one step of the limit: an ulp of a warp entry (below 2) moves a squared move of 0.07^2 by up to 2 * 0.07 * 2^-52
    assert max(np.abs(ulps)) <= 2 * 0.07 * np.spacing(1.0) / np.spacing(tpl.REFRESH_LIMIT2), ulps
    print("  (kind, column at which the loop leaves): %s" % sorted(columns, key=str))
    assert {f for _k, f in columns} >= {None, 0} and len(columns) >= 3
    mixed, all_kept, all_made = (np.array(c.target["kept"]).reshape(-1, tpl.PPW[patch]) for c in cases[-3:])
    assert len(mixed) >= 2 and (mixed.sum(1) == tpl.PPW[patch] // 2).all() and all_kept.all() and len(all_kept) == 1 and not all_made.any() and len(all_made) == 1


@pytest.mark.parametrize("patch", [8, 11])
@pytest.mark.parametrize("size", [(tpl.W, tpl.H), tpl.SMALL])
def test_border_group_makes_good_and_bad_templates_at_every_side(size, patch):
    """per source level and side of the source image: the border points whose template the oracle makes good and those it makes bad by
    nOutside (both outcomes of each of warp_sample's four comparisons); bad templates hold zeros, are not counted in attempted, keep their
    verdict in the second frame and, some of them, lose it in the third"""
    cases = tpl.groups(patch)["c: source border, %dx%d" % size]
    assert len(cases) == len(tpl.borders(patch)) * len(tpl.VIEWS) <= 24
    assert tpl.borders(patch) == tuple(range(patch // 2 - 1, patch // 2 + 3))
    total, n_bad, n_stay, n_flip = {}, 0, 0, 0
    for c in cases:
        assert len(c.map()["points"]) <= tpl.MAX_BORDER_POINTS + 8 + 24
        r0, r1, r2 = tpl.run(c, patch)
        for k, v in tpl.border_counts(c, r0).items():
            a = total.setdefault(k, [0, 0]); a[0] += v[0]; a[1] += v[1]
        t0, t1, t2 = r0["tmpl"], r1["tmpl"], r2["tmpl"]
        bad = (t0["have"] == 1) & (t0["bad"] == 1)
        assert (r0["pvs_have"] == 0).all() and (r0["tracks"]["level"][bad] >= 0).all() and (r0["tracks"]["searched"][bad] == 0).all(), c.name
        assert ((t0["tmpl"][bad] == 0).sum((1, 2)) >= 1).all(), c.name              # a sample outside the source is written as 0
        for r in (r0, r1, r2):
            assert sum(r["attempted"]) == int(((r["tracks"]["level"] >= 0) & (r["tracks"]["searched"] == 1)).sum()), c.name
        stay = bad & (r1["tracks"]["level"] >= 0)
        assert (t1["bad"][stay] == 1).all() and (r1["tracks"]["searched"][stay] == 0).all() and (t1["tmpl"][stay] == t0["tmpl"][stay]).all(), c.name
        flip = bad & (r2["tracks"]["level"] >= 0) & (t2["bad"] == 0) & (r2["tracks"]["searched"] == 1)
        n_bad, n_stay, n_flip = n_bad + int(bad.sum()), n_stay + int(stay.sum()), n_flip + int(flip.sum())
    print("\n[c: source border, %dx%d, %dx%d patches] %d streams; templates made bad %d, kept bad in frame 1 %d, made again and good in frame 2 %d" % (size + (patch, patch, len(cases), n_bad, n_stay, n_flip)))
    for side in tpl.SIDES:
        per_level = {l: total[(l, side)] for l in range(4) if (l, side) in total}
        print("  %-6s [good, bad] per source level: %s" % (side, per_level))
        assert sum(v[0] for v in per_level.values()) >= 1 and sum(v[1] for v in per_level.values()) >= 1, (side, per_level)
    assert n_bad >= 50 and n_stay >= 50 and n_flip >= 10


@pytest.mark.parametrize("patch", [8, 11])
def test_bad_scale_outlives_its_cause_until_the_template_is_made_again(patch):
    cases = tpl.groups(patch)["d: sticky bad scale"]
    assert len(cases) == len(tpl.STICKY_ZOOMS)
    print()
    for c in cases:
        recs = tpl.run(c, patch)
        st = tpl.sticky_points(recs)
        print("[d, %dx%d patches] %s: %d points, good / bad by scale / kept bad and not searched / made again: %d" % (patch, patch, c.name, len(c.map()["points"]), len(st)))
        assert len(st) == c.target["n_sticky"] >= tpl.STICKY_MIN, (c.name, len(st))
        assert all(r["quality"] == 2 for r in recs), c.name
