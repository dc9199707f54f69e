"""The plan cases of the PVS shuffle, shared by tests/test_pvs_perm.py (CPU: each case reaches its branch of jni/Tracker.cc:437-461 /
:520-527 in the restated selection) and tests/test_gpu_pvs_shuffle.py (GPU: k_plan's plans == the restatement's).  Sub-maps of the feeder's
320x240 scene with chosen per-level counts (tracker_cases._e_case); the levels come from the oracle, nothing from the device."""
import functools

import numpy as np

import pvs_perm_ref as ref
import tracker_cases as tc

PATCH = 8
SEED = 0x5EED
CAP = 25
GATE_CLOSED = tc._with(tc.E_COARSE, coarse_disabled=1, max_patches_per_frame=CAP)


@functools.lru_cache(maxsize=None)
def plan_cases():
    """name -> (case, bTryCoarse).  Two parameter sets: the coarse gate closed with max_patches_per_frame = 25, and coarse_min = 4,
    coarse_max = 12 with the gate open (coarse_min_vel = 0) and the cap out of reach."""
    M, X = tc.COARSE_MIN, tc.COARSE_MAX
    return {
        "a: gate closed, chopped": (tc._e_case("a", PATCH, (20, 10, 10, 5), GATE_CLOSED), False),
        "e: gate closed, cap not reached": (tc._e_case("e", PATCH, (5, 5, 5, 3), GATE_CLOSED), False),
        "b: level 3 longer than coarse_max": (tc._e_case("b", PATCH, (10, 10, 10, X + 8), tc.E_COARSE), True),
        "c: level 3 short, level 2 longer than the remainder": (tc._e_case("c", PATCH, (10, 10, 30, 5), tc.E_COARSE), True),
        "d: level 2 replaces level 3": (tc._e_case("d", PATCH, (10, 10, X - 5, 5), tc.E_COARSE), True),
    }


GROUPS = (("a: gate closed, chopped", "e: gate closed, cap not reached"),
          ("b: level 3 longer than coarse_max", "c: level 3 short, level 2 longer than the remainder", "d: level 2 replaces level 3"))


@functools.lru_cache(maxsize=None)
def cpu_levels(name):
    """the search level of every point of the case in its first frame, from the oracle (the levels do not depend on the order)"""
    c = plan_cases()[name][0]
    o = c.oracle(PATCH)
    o.frame_begin(c.frame(0)); o.search_stage(0)
    lv = o.point_tracks()["level"].copy()
    o.close()
    return lv


def expected(name, seed, frame=1):
    c, try_coarse = plan_cases()[name]
    p = dict(c.pkw)
    return ref.iteration_set(cpu_levels(name), p.get("coarse_min", 20), p.get("coarse_max", 60), p.get("max_patches_per_frame", 1000), try_coarse, seed, frame)
