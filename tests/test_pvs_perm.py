"""CPU test of the PVS shuffle's permutation (csrc/pvs_perm.h): the library's host form (vslam_pvs_permutation, on_host = 1) against the NumPy
restatement of tests/pvs_perm_ref.py, at the lengths where the device network changes shape (one wavefront, one pass of 256 threads, the
padded powers of two) and at the capacity."""
import numpy as np
import pytest

import pvs_perm_ref as ref
import tracker_cases as tc
from pvs_cases import CAP, SEED, cpu_levels, expected, plan_cases
from visualslam_android_amd import capi

LENGTHS = (0, 1, 2, 63, 64, 65, 255, 256, 257, 1000, 4095, 4096)
TRIPLES = ((1, 0, 0), (0xC0FFEE, 7, 4), (0xFFFFFFFF, 123456, 3))       # (seed, frame, list): frame 0, list 4, the largest seed


@pytest.mark.parametrize("triple", TRIPLES)
def test_host_form_equals_the_restatement(triple):
    seed, frame, lst = triple
    for n in LENGTHS:
        got = capi.pvs_permutation(seed, frame, lst, n, on_host=True)
        assert np.array_equal(got, ref.permutation(seed, frame, lst, n)), (triple, n)
        assert np.array_equal(np.sort(got), np.arange(n)), (triple, n)                    # a permutation


def test_frames_and_lists_give_different_permutations():
    n = 257
    base = capi.pvs_permutation(5, 3, 0, n, on_host=True)
    assert not np.array_equal(base, np.arange(n))
    assert not np.array_equal(base, capi.pvs_permutation(5, 4, 0, n, on_host=True))        # another frame
    assert not np.array_equal(base, capi.pvs_permutation(5, 3, 4, n, on_host=True))        # another list
    assert not np.array_equal(base, capi.pvs_permutation(6, 3, 0, n, on_host=True))        # another seed
    assert np.array_equal(base, capi.pvs_permutation(5, 3, 0, n, on_host=True))


@pytest.mark.parametrize("n", [2, 65, 1000, 4096])
def test_ties_keep_identity_order(n):
    same = np.full(n, 77, np.uint32)
    assert np.array_equal(capi.pvs_permutation(1, 1, 0, n, keys=same, on_host=True), np.arange(n))
    two = np.where(np.random.default_rng(n).random(n) < 0.5, 9, 4).astype(np.uint32)       # two distinct values: the stable partition
    want = np.r_[np.flatnonzero(two == 4), np.flatnonzero(two == 9)]
    assert np.array_equal(capi.pvs_permutation(1, 1, 0, n, keys=two, on_host=True), want)
    assert np.array_equal(ref.permutation(1, 1, 0, n, two), want)


def test_length_past_the_capacity_is_refused_and_the_default_is_identity():
    lib = capi.load_library()
    out = np.zeros(4097, np.int32)
    for on_host in (1, 0):                                                                 # refused before any device is looked for
        assert lib.vslam_pvs_permutation(1, 1, 0, 4097, None, out.ctypes.data, on_host) == -1
    assert lib.vslam_pvs_permutation(1, 1, 0, -1, None, out.ctypes.data, 1) == -1
    assert capi.default_params(320, 240, 1).pvs_shuffle_seed == 0


def test_restated_selection_in_identity_mode_is_the_plan_of_the_tracker_cases():
    """pvs_perm_ref.iteration_set at seed 0 against tracker_cases.plan (the counts the oracle is held to in test_tracker_cases.py)"""
    import tracker_cases as tc
    rng = np.random.default_rng(3)
    for n in ((10, 10, 2, 2), (10, 10, 5, 0), (10, 10, 30, 11), (10, 10, 30, 13), (10, 10, 7, 5), (10, 10, 8, 5), (7, 7, 7, 20), (10, 10, 10, 41)):
        level = rng.permutation(np.repeat([0, 1, 2, 3, -1], list(n) + [6]))
        for mp in (40, 1000):
            it = ref.iteration_set(level, tc.COARSE_MIN, tc.COARSE_MAX, mp, True, 0, 1)
            c3, c2, f3, fo = tc.plan(n, max_patches=mp)
            assert (int((level[it["coarse"]] == 3).sum()), int((level[it["coarse"]] == 2).sum()), len(it["level3"]), len(it["other"])) == (c3, c2, f3, fo), (n, mp)
            assert len(set(it["all"].tolist())) == len(it["all"])


def test_cases_reach_their_branches_on_the_cpu():
    X = tc.COARSE_MAX
    e = {k: expected(k, SEED) for k in plan_cases()}
    lv = {k: cpu_levels(k) for k in plan_cases()}
    a = e["a: gate closed, chopped"]
    assert len(a["coarse"]) == 0 and a["chopped"] and len(a["all"]) == CAP
    assert not e["e: gate closed, cap not reached"]["chopped"] and len(e["e: gate closed, cap not reached"]["coarse"]) == 0
    b = e["b: level 3 longer than coarse_max"]
    assert len(b["coarse"]) == X and (lv["b: level 3 longer than coarse_max"][b["coarse"]] == 3).all() and len(b["level3"]) == 8 and not b["chopped"]
    c = e["c: level 3 short, level 2 longer than the remainder"]
    lc = lv["c: level 3 short, level 2 longer than the remainder"][c["coarse"]]
    assert (lc == 3).sum() == 5 and (lc == 2).sum() == X - 5 and len(c["level3"]) == 0
    d = e["d: level 2 replaces level 3"]
    assert (lv["d: level 2 replaces level 3"][d["coarse"]] == 2).all() and len(d["coarse"]) == X - 5 and len(d["level3"]) == 0
    for k in plan_cases():                                                   # and the seed changes the order in every case
        assert not np.array_equal(e[k]["all"], expected(k, 0)["all"]), k
