"""CPU check of tests/search_trip_cases.py: the oracle alone, run on every case of tests/test_gpu_search_trips.py, meets the counts the
case is named for -- recomputed here from the oracle's corner lists, levels and predicted positions (coarse_window, the row-LUT range,
the x-window and circle tests), and checked against the oracle's own count of ZMSSD evaluations.  A case that misses is a broken
case.  Run with -s to see what each case reaches."""
import pytest

import search_trip_cases as sc

N, K = sc.N_CORNERS, sc.K_FLIGHT


def reached(case, patch):
    """the windows of the case's chosen points in the oracle's first frame, after checking the recomputation against the oracle:
    the survivors of all searched points are the ZMSSD evaluations it counted"""
    empty = bool(case.target.get("empty"))
    o, tr, wins = sc.case_windows(case, patch, stage=0 if empty else 1, range_l0=0 if empty else sc.FINE_RANGE)
    st = o.state()
    o.close()
    assert sum(len(w["survivors"]) for w in wins.values()) == st.n_zmssd, (case.name, st.n_zmssd)
    assert all(p in wins for p in case.chosen), case.name                       # the chosen points are searched
    return tr, [wins[p] for p in case.chosen]


def check_target(case, patch):
    t = case.target
    tr, ws = reached(case, patch)
    counts = [(w["i1"] - w["i0"], len(w["survivors"])) for w in ws]
    if "window" in t:
        assert not ws[0]["empty"] and counts[0][0] == t["window"], (case.name, counts)
    if "survivors" in t:
        assert counts[0][1] == t["survivors"] and (t["survivors"] > 0 or counts[0][0] > 0), (case.name, counts)
    if t.get("border_mid_trip"):
        assert sc.border_in_mid_trip(ws[0]), case.name
    if "tie" in t:
        ranks, trips, won, best = sc.equal_best(case, patch)
        assert len(ranks) == 2 and ranks[0] < ranks[1] and won, (case.name, ranks, won)   # the earlier in raster order is the one found
        assert (trips[0] == trips[1]) == (t["tie"] == "same"), (case.name, trips)
        counts.append(("equal best ZMSSD %d at survivors" % best, ranks, "trips", trips))
    if t.get("mixed"):
        assert len(ws) == t["n_search"] == sc.PATCHES_PER_WAVE[patch] and all(w["level"] == 0 for w in ws), case.name
        assert int((tr["searched"] == 1).sum()) == t["n_search"], case.name
        assert any(c[0] == 0 for c in counts) and any(c[0] >= 2 * N + 1 for c in counts), (case.name, counts)
        assert any(c[0] > 0 and c[1] == 0 for c in counts) and any(c[1] >= 2 * K + 1 for c in counts), (case.name, counts)
    if t.get("empty"):
        assert ws and all(w["empty"] for w in ws) and all(tr["found"][p] == 0 for p in case.chosen), case.name
        counts = ["cw.empty at level %d" % w["level"] for w in ws]
    return "%s: (window corners, survivors) of the chosen patches %s" % (case.name, counts), ws


@pytest.mark.parametrize("patch", [8, 11])
@pytest.mark.parametrize("group", sc.GROUP_NAMES)
def test_every_case_reaches_its_target_in_the_oracle(group, patch):
    cases = sc.groups(patch)[group]
    print("\n[%s, %dx%d patches]" % (group, patch, patch))
    for c in cases:
        print("  " + check_target(c, patch)[0])


@pytest.mark.parametrize("patch", [8, 11])
def test_every_named_count_is_reached(patch):
    """window corners 0, 1, N - 1, N, N + 1, 2 N, 2 N + 1 and survivors 0, 1, K - 1, K, K + 1, 2 K + 1 with N, K as k_searchN is built; an empty
    window, a border survivor in mid trip, both ties, the wavefront of extremes; batches of 1, 9 and 17 streams"""
    g = sc.groups(patch)
    assert {len(v) for v in g.values()} == {1, 9, 17} and tuple(g) == sc.GROUP_NAMES
    windows, survivors, kinds = set(), set(), set()
    for c in g["17 streams"] + g["1 stream: the empty window"]:
        _line, ws = check_target(c, patch)
        t = c.target
        if "window" in t:
            windows.add(ws[0]["i1"] - ws[0]["i0"])
        if "survivors" in t:
            survivors.add(len(ws[0]["survivors"]))
        kinds |= {k if k != "tie" else "tie " + t[k] for k in t if k in ("border_mid_trip", "tie", "mixed", "empty")}
    assert (N, K) == (128, 4)                                                   # SEARCH_N, SEARCH_K of csrc/track.hip
    assert windows == set(sc.WINDOW_TARGETS) == {0, 1, N - 1, N, N + 1, 2 * N, 2 * N + 1}, windows
    assert survivors == set(sc.SURVIVOR_TARGETS) == {0, 1, K - 1, K, K + 1, 2 * K + 1}, survivors
    assert kinds == {"border_mid_trip", "tie same", "tie other", "mixed", "empty"}, kinds
    assert all(c in g["17 streams"] for c in g["9 streams"])
