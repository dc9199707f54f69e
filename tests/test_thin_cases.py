"""CPU check of tests/thin_cases.py: in every scenario the oracle's ThinCandidates (orc.thin_candidates, jni/MapMaker.cc:381-422) and a
plain numpy statement of the rule leave the same candidates, every target candidate stays or goes as the scenario states, and the
scenarios reach what they are for: d2 == 100 and below, rounding of .5 and .49 at levels 0 and 1, the level filter, untouched and
emptied levels, removals confined to one chunk of 256.  Run with -s to see, per scenario, the counts per level before and after."""
import numpy as np
import pytest

import thin_cases as th


def survivors(name):
    meas, targets = th.scenario(name)
    root, mlev = np.array([[rx, ry] for _l, rx, ry in meas], np.float64), np.array([l for l, _x, _y in meas], np.int32)
    want = th.expected(name)
    keep = []
    for l, (pos, sc) in enumerate(th.level_candidates()):
        k = th.rule_keep(pos, l, root, mlev)
        assert np.array_equal(want[l][0], pos[k]) and np.array_equal(want[l][1], sc[k]), (name, l)       # oracle == rule, order kept
        keep.append(k)
    return meas, targets, keep


def test_frame_has_more_than_one_chunk_of_level_0_candidates():
    n = [len(p) for p, _sc in th.level_candidates()]
    print("\ncandidates per level: %s" % n)
    assert n[0] > th.CHUNK and min(n) > 0
    assert all(((th.xy(p) >= th.BORDER).all() for p, _sc in th.level_candidates()))


@pytest.mark.parametrize("name", th.SCENARIOS)
def test_scenario_removes_what_it_states(name):
    meas, targets, keep = survivors(name)
    n = [len(k) for k in keep]
    left = [int(k.sum()) for k in keep]
    print("\n[%s] %d measurements, candidates per level %s -> %s" % (name, len(meas), n, left))
    root, mlev = np.array([[rx, ry] for _l, rx, ry in meas], np.float64), np.array([l for l, _x, _y in meas], np.int32)
    for j, (level, i, stays) in enumerate(targets):
        assert bool(keep[level][i]) == stays, (name, level, i, stays)
        if not stays and name != "every candidate of level 2":     # ... and it is its own measurement that removes it
            rest = np.arange(len(meas)) != j
            assert th.rule_keep(th.level_candidates()[level][0], level, root[rest], mlev[rest])[i], (name, level, i)
    gone = {l: set(np.flatnonzero(~k)) for l, k in enumerate(keep)}
    aimed = {l: {i for tl, i, stays in targets if tl == l and not stays} for l in range(4)}
    others = {l: sorted(gone[l] - aimed[l]) for l in range(4) if gone[l] - aimed[l]}
    print("  candidates that go beside the targets (a measurement of level m also thins level m - 1): %s" % ({l: len(v) for l, v in others.items()} or "none"))
    if name in ("distance", "rounding at level 0"):
        assert not others and left[1:] == n[1:]                    # levels without a busy position: unchanged
        assert left[0] == n[0] - sum(not s for _l, _i, s in targets)
    if name == "rounding at level 1":
        assert set(others) <= {0} and left[1] == n[1] - 1 and left[2:] == n[2:]
    if name.startswith("level filter"):
        (mlev1, _x, _y), (level, _i, stays) = meas[0], targets[0]
        assert len(meas) == 1 and stays == (mlev1 - level not in (0, 1))
        thinned = {l for l in range(4) if left[l] < n[l]}
        assert thinned <= {mlev1 - 1, mlev1} and (level in thinned) == (not stays)
    if name == "every candidate of level 2":
        assert n[2] > 0 and left[2] == 0 and left[3] == n[3]
    if name.endswith("chunk only") or name == "every chunk":
        n_chunks = (n[0] + th.CHUNK - 1) // th.CHUNK
        hit = sorted({int(i) // th.CHUNK for i in gone[0]})
        want = {"first chunk only": [0], "last chunk only": [n_chunks - 1], "every chunk": list(range(n_chunks))}[name]
        assert n_chunks >= 2 and hit == want, (hit, want)
        assert left[1:] == n[1:]


def test_level_filter_covers_both_sides():
    assert sorted({m - l for l, m, _s in th.LEVEL_FILTER}) == [-1, 1, 2] and all(s == (m - l not in (0, 1)) for l, m, s in th.LEVEL_FILTER)
    assert len(th.SCENARIOS) <= 17


def test_distance_and_rounding_stand_on_the_threshold():
    """the busy positions the scenarios make, as the rule rounds them: d2 == 100 keeps, 98 and 81 go; 9.5 rounds to 10, 9.49 to 9"""
    for name in ("distance", "rounding at level 0", "rounding at level 1"):
        meas, targets = th.scenario(name)
        for (mlev, rx, ry), (level, i, stays) in zip(meas, targets):
            v = np.array([rx, ry]) / (1 << level)
            busy = np.trunc(np.where(v > 0.0, v + 0.5, v - 0.5)).astype(np.int64)
            d2 = int(((busy - th.xy(th.level_candidates()[level][0])[i]) ** 2).sum())
            assert mlev == level and (d2 >= 100) == stays and d2 in (100, 98, 81), (name, d2)
    assert [(dx * dx + dy * dy, stays) for (dx, dy), stays in th.DISTANCE] == [(100, True), (98, False), (100, True), (81, False), (100, True), (81, False)]
