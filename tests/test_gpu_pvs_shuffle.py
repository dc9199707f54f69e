"""GPU tests of the seeded shuffle of the potentially visible set (vslam_params.pvs_shuffle_seed; csrc/pvs_perm.h, k_plan<true> in
csrc/track.hip; jni/Tracker.cc:396-397, 525): the device sort against the host form and the NumPy restatement, k_plan's ordered plans
against the restated selection of tests/pvs_perm_ref.py on the branches of :437-461 and :520-527, a whole frame against the unchanged
(identity) oracle run on a map re-ordered by the permutation, coverage of the map over frames, and determinism / independence of the
stream's slot.  The maps are sub-maps of the feeder's 320x240 test scene with a few dozen points per level (tests/tracker_cases.py)."""
import numpy as np
import pytest

import pvs_perm_ref as ref
import tracker_cases as tc
from pvs_cases import GROUPS, PATCH, SEED, cpu_levels, expected, plan_cases
from helpers import assert_tracker_exact, make_oracle, make_scene
from visualslam_android_amd import capi

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 2, 63, 64, 65, 255, 256, 257, 1000, 2049, 4095, 4096)      # 65, 257, 2049: one more than half the padded length
TRIPLES = ((1, 0, 0), (0xC0FFEE, 7, 4), (0xFFFFFFFF, 123456, 3))


# ---- 1. the device routine ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("triple", TRIPLES)
def test_device_sort_equals_host_form_and_restatement(triple):
    seed, frame, lst = triple
    for n in LENGTHS:
        dev = capi.pvs_permutation(seed, frame, lst, n)
        assert np.array_equal(dev, capi.pvs_permutation(seed, frame, lst, n, on_host=True)), (triple, n)
        assert np.array_equal(dev, ref.permutation(seed, frame, lst, n)), (triple, n)


@pytest.mark.parametrize("n", [2, 65, 257, 1000, 2049, 4096])
def test_device_sort_keeps_ties_in_identity_order(n):
    same = np.full(n, 0xFFFFFFFF, np.uint32)                                 # the largest key: next to the padding of the network
    assert np.array_equal(capi.pvs_permutation(1, 1, 0, n, keys=same), np.arange(n))
    two = np.where(np.random.default_rng(n).random(n) < 0.5, 9, 4).astype(np.uint32)
    assert np.array_equal(capi.pvs_permutation(1, 1, 0, n, keys=two), np.r_[np.flatnonzero(two == 4), np.flatnonzero(two == 9)])


# ---- 2. the plan (the cases and what the restatement expects of them: tests/pvs_cases.py) ----------------------------------------------
def run_plans(names, seed):
    """the cases as the streams of one System, stage by stage -> per case (coarse plan, full plan, counts, searched flags, state)"""
    cases = [plan_cases()[k][0] for k in names]
    vp = cases[0].params(len(cases), PATCH)
    vp.pvs_shuffle_seed = seed
    g = capi.System(vp)
    for s, c in enumerate(cases):
        c.load(g, s)
    g.make_keyframe_lite(np.stack([c.frame(0) for c in cases]))
    g.patch_search(0)
    first = [g.search_plan(s) for s in range(len(cases))]
    g.pose_update(0)
    g.patch_search(1)
    out = []
    for s in range(len(cases)):
        plan, counts = g.search_plan(s)
        out.append({"coarse": first[s][0], "coarse_counts": first[s][1], "plan": plan, "counts": counts, "tracks": g.point_tracks(s),
                    "state": g.state(s), "bad": g.templates(s)["bad"]})
    g.pose_update(1)
    g.finish_frame()
    for s in range(len(cases)):
        out[s]["final_plan"] = g.search_plan(s)[0]
        out[s]["final_state"] = g.state(s)
    g.close()
    return out


@pytest.mark.parametrize("group", range(len(GROUPS)))
def test_plan_equals_the_restated_selection(group):
    names = GROUPS[group]
    got, ident = run_plans(names, SEED), run_plans(names, 0)
    differs = 0
    for k, r, r0 in zip(names, got, ident):
        e, lv = expected(k, SEED), cpu_levels(k)
        assert r["state"].frame == 1
        assert np.array_equal(r["coarse"], e["coarse"]), (k, r["coarse"], e["coarse"])
        assert r["coarse_counts"] == {"coarse": len(e["coarse"]), "level3": 0, "other": 0, "total": len(e["coarse"])}, k
        assert np.array_equal(r["plan"], e["all"]), (k, r["plan"], e["all"])
        assert np.array_equal(r["final_plan"], e["all"]), k
        assert r["counts"] == {"coarse": len(e["coarse"]), "level3": len(e["level3"]), "other": len(e["other"]), "total": len(e["all"])}, k
        tr = r["tracks"]
        assert np.array_equal(tr["level"], lv), k
        srch = np.flatnonzero(tr["searched"] == 1)
        assert set(srch.tolist()) <= set(e["all"].tolist()), k
        skipped = np.setdiff1d(e["all"], srch)                               # planned and not searched: only a point whose template is bad (:637-640)
        assert (r["bad"][skipped] == 1).all(), (k, skipped)
        assert list(r["state"].attempted) == [int((lv[srch] == l).sum()) for l in range(4)], k
        assert np.array_equal(r0["plan"], expected(k, 0)["all"]), k          # the identity run takes map order
        differs += set(srch.tolist()) != set(np.flatnonzero(r0["tracks"]["searched"] == 1).tolist())
    if group == 0:
        assert differs >= 1                                                  # the chop keeps other points than the head of the lists


# ---- 3. a whole frame against the identity oracle on the re-ordered map ---------------------------------------------------------------
class Reordered:
    """a System's read-backs of one stream with the map points in another order: entry j is the device's point order[j]"""
    def __init__(self, g, order):
        self.g, self.order = g, order

    def state(self, s):
        return self.g.state(s)

    def point_tracks(self, s):
        return {k: v[self.order] for k, v in self.g.point_tracks(s).items()}

    def templates(self, s, n):
        return {k: v[self.order] for k, v in self.g.templates(s, n).items()}


@pytest.mark.parametrize("name", ["b: level 3 longer than coarse_max", "e: gate closed, cap not reached"])
def test_frame_equals_identity_oracle_on_the_reordered_map(name):
    c = plan_cases()[name][0]
    lv = cpu_levels(name)
    assert not expected(name, SEED)["chopped"]                               # no second shuffle: the order is the levels' alone
    order = np.arange(len(lv))
    for l in range(4):                                                       # the slots of a level's points take them in shuffled order
        idx = np.flatnonzero(lv == l)
        order[idx] = ref.shuffled(idx, SEED, 1, l)
    assert not np.array_equal(order, np.arange(len(lv)))
    c2 = tc.Case(c.name + " re-ordered", c.skey, c.keep[order], c.pkw, {}, start=c.start, vel=c.vel)
    o = c2.oracle(PATCH)
    vp = c.params(1, PATCH)
    vp.pvs_shuffle_seed = SEED
    g = capi.System(vp)
    c.load(g, 0)
    o.track_frame(c.frame(0))
    g.track_frame(c.frame(0)[None])
    assert np.array_equal(order[ref.iteration_set(o.point_tracks()["level"], *[dict(c.pkw).get(k, d) for k, d in (("coarse_min", 20), ("coarse_max", 60), ("max_patches_per_frame", 1000))],
                                                  plan_cases()[name][1], 0, 1)["all"]], g.search_plan(0)[0])
    assert_tracker_exact(o, Reordered(g, order), 0, name)
    o.close(); g.close()


# ---- 4. coverage over frames -----------------------------------------------------------------------------------------------------------
def test_shuffle_covers_the_map_and_finds_as_well():
    n_frames = 12
    f, m, frames = make_scene(tc.W, tc.H, seed=77, n_frames=n_frames, per_level=tc.SPARSE)
    base = dict(tc.NO_KF)
    o = make_oracle(capi.default_params(tc.W, tc.H, 1, patch_size=PATCH, **base), m, f.pose(-1))
    o.frame_begin(frames[0]); o.search_stage(0)
    lv = o.point_tracks()["level"]
    o.close()
    n0 = int((lv == 0).sum())
    cap = int((lv >= 0).sum()) - n0 // 2                                     # the identity order never reaches the second half of level 0
    assert n0 >= 100 and cap > 0
    runs = {}
    for seed in (0, SEED):
        vp = capi.default_params(tc.W, tc.H, 1, patch_size=PATCH, max_patches_per_frame=cap, pvs_shuffle_seed=seed, **base)
        g = capi.System(vp)
        g.load_map(0, m); g.set_pose(0, f.pose(-1))
        seen = np.zeros(len(lv), bool)
        att, fnd = np.zeros(4, np.int64), np.zeros(4, np.int64)
        for t in range(n_frames):
            g.track_frame(frames[t][None])
            st = g.state(0)
            assert st.quality == 2, (seed, t, st.quality)
            seen |= g.point_tracks(0)["searched"] == 1
            att += np.array(st.attempted[:]); fnd += np.array(st.found[:])
        g.close()
        runs[seed] = (seen, att, fnd)
    print("searched over %d frames: identity %d, shuffled %d of %d points" % (n_frames, runs[0][0].sum(), runs[SEED][0].sum(), len(lv)))
    assert runs[SEED][0].sum() > runs[0][0].sum()
    for l in range(4):
        (_, a0, f0), (_, a1, f1) = runs[0], runs[SEED]
        if a0[l] == 0 or a1[l] == 0:
            continue
        p, q = f0[l] / a0[l], f1[l] / a1[l]
        print("level %d: found / attempted identity %.4f (%d), shuffled %.4f (%d)" % (l, p, a0[l], q, a1[l]))
        assert q >= p - 3.0 * np.sqrt(p * (1.0 - p) / a1[l]), (l, p, q)


# ---- 5. determinism and independence ---------------------------------------------------------------------------------------------------
def run_stream(S, slot, seed, frames=2, stream_seed=None, reset_first=False):
    """case a in `slot` of an S-stream system -> per frame (plan, pose, velocity, found counts)"""
    c = plan_cases()["a: gate closed, chopped"][0]
    vp = c.params(S, PATCH)
    vp.pvs_shuffle_seed = seed
    g = capi.System(vp)
    blank = np.zeros((S,) + c.frame(0).shape, np.uint8)

    def play():
        c.load(g, slot)
        out = []
        for t in range(frames):
            fr = blank.copy(); fr[slot] = c.frame(t)
            g.track_frame(fr)
            st = g.state(slot)
            out.append((g.search_plan(slot)[0].tolist(), tuple(st.pose[:]), tuple(st.velocity[:]), tuple(st.found[:]), st.frame))
        return out
    if reset_first:                                                          # a first life with another seed, then Reset and the map again
        g.set_pvs_seed(slot, seed + 1)
        first = play()
        g.reset([slot])
        again = play()
        g.close()
        return first, again
    if stream_seed is not None:
        g.set_pvs_seed(slot, stream_seed)
    out = play()
    g.close()
    return out


def test_same_seed_same_bits_whatever_the_slot():
    a = run_stream(1, 0, SEED)
    assert a == run_stream(1, 0, SEED)
    assert a == run_stream(8, 5, SEED)
    assert a[0][0] != a[1][0]                                                # the frame number enters


def test_per_stream_seeds_and_reset():
    a, ident = run_stream(1, 0, SEED), run_stream(1, 0, 0)
    other = run_stream(1, 0, SEED, stream_seed=SEED + 1)
    assert other[0][0] != a[0][0] and other[0][0] != ident[0][0] and sorted(other[0][0]) != sorted(ident[0][0])
    assert run_stream(2, 1, SEED, stream_seed=0) == ident                    # seed 0 on a stream: the identity kernel's bits
    first, again = run_stream(2, 1, SEED, reset_first=True)
    assert first == other and again == a                                     # Reset puts the seed back to the params value
    vp = capi.default_params(tc.W, tc.H, 1)
    g = capi.System(vp)
    assert g.lib.vslam_set_pvs_seed(g.h, 0, 5) == -4                          # VSLAM_E_STATE: created with the identity kernel
    g.close()
