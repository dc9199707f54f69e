"""GPU parity of the paths one Levenberg-Marquardt step of the device Bundle::Compute can take (ba_device.h: ba_lm, ba_step_sweep,
the commit of an accepted trial, the erase of a step's outliers), on small stand-alone problems built with ba_scene (the one with
66 fixed cameras with ba_paths_scene's ring of cameras: ba_scene's cameras walk through the points when there are that many).

Every case states with the oracle what makes it the case it claims to be (a rejected trial, a step that erases nothing before one
that does, ...), so it cannot pass empty.  Then, per summation mode:
  ba_sum_order = 1   cameras, points, accepted, trials and the outlier lists are the oracle's, bit for bit (check_exact)
  ba_sum_order = 0   they agree with the oracle within the fast mode's bars (check(), 1e-8 on cameras and 1e-7 on points with two
                     fixed cameras, as in test_gpu_bundle_paths.py), and they are bit-equal to tests/golden/ba_step_paths_fast.npz.
The fixture holds what the fast mode gave before the step's commit and sweep were reworked: those changes move no
floating-point expression and no sum's order, so the bits must stay.  It is written by this file run as a program
(python tests/test_gpu_ba_step_paths.py OUT.npz, VSLAM_LIB naming the library to record from).

  rejected_trial          more LM trials than accepted steps: the committed state survives a rejected trial
  erase_skip_then_erase   a step that marks no outlier (its erase finds nothing) before a step that marks some
  first_step_outliers     gross outliers erased in the first step
  nfree_1 5 6 10 11       the edges of BA_MFMA_FREE and BA_FAST_FREE: the sweep's two unrolled U / epsilon_a forms and the form without
  multi_trip_point        every point has 66 measurements in fixed cameras: a chunk of two trips, the point's sums carried across
  chunk_64 65 258         M = 64, 65 and just above 4 x 64 slots: one full trip, one slot over, more chunks than wavefronts"""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:                     # (run as a program to record the fixture; under pytest conftest.py has done it)
    sys.path.insert(0, ROOT)

from ba_paths_scene import paths_scene
from ba_scene import CAM, ba_scene
from oracle import binding as orc
from test_gpu_bundle import check, check_exact, load
from visualslam_android_amd import capi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ba_step_paths_fast.npz")
ROUGH = (0.4, 20 * np.pi / 180, 0.8)         # a start far from the truth: trials get rejected


def truncated(sc, M):
    """The first M measurements of the scene's list put point-major, so that every camera keeps some."""
    assert len(sc["meas"]) >= M
    sc["meas"] = sorted(sc["meas"], key=lambda m: (m[1], m[0]))[:M]
    return sc


# case -> (scene, LM iterations)
CASES = {
    "rejected_trial": (lambda: ba_scene(n_cams=4, n_pts=40, n_fixed=2, seed=0, init_noise=ROUGH), 8),
    "erase_skip_then_erase": (lambda: ba_scene(n_cams=4, n_pts=40, n_fixed=2, seed=2), 8),
    "first_step_outliers": (lambda: ba_scene(n_cams=4, n_pts=40, n_fixed=2, seed=0), 5),
    "nfree_1": (lambda: ba_scene(n_cams=3, n_pts=40, n_fixed=2, visibility=0.8, seed=31), 5),
    "nfree_5": (lambda: ba_scene(n_cams=7, n_pts=40, n_fixed=2, visibility=0.8, seed=35), 5),
    "nfree_6": (lambda: ba_scene(n_cams=8, n_pts=40, n_fixed=2, visibility=0.8, seed=36), 5),
    "nfree_10": (lambda: ba_scene(n_cams=12, n_pts=40, n_fixed=2, visibility=0.8, seed=40), 5),
    "nfree_11": (lambda: ba_scene(n_cams=13, n_pts=40, n_fixed=2, visibility=0.8, seed=41), 5),
    "multi_trip_point": (lambda: paths_scene(69, 12, fixed=tuple(range(66)), visibility=1.0, outlier_frac=0.02, seed=50), 4),
    "chunk_64": (lambda: truncated(ba_scene(n_cams=4, n_pts=24, n_fixed=2, seed=60), 64), 4),
    "chunk_65": (lambda: truncated(ba_scene(n_cams=4, n_pts=24, n_fixed=2, seed=60), 65), 4),
    "chunk_258": (lambda: truncated(ba_scene(n_cams=5, n_pts=64, n_fixed=2, seed=61), 258), 4),
}


@functools.lru_cache(maxsize=None)
def scene(case):
    return CASES[case][0]()


class OracleRun:
    """One oracle Compute of a scene, kept: the surface check() / check_exact() read (their compute() returns the kept value)."""

    def __init__(self, sc, max_it):
        o = orc.OracleBundle(CAM, 640, 480, max_iterations=max_it)
        load(o, sc)
        self._acc = o.compute()
        self._stats, self._conv = o.stats(), o.converged()
        self._cams, self._pts, self._om, self._op = o.cameras(), o.points(), o.outlier_meas().copy(), o.outlier_points().copy()
        o.close()

    def compute(self): return self._acc
    def stats(self): return self._stats
    def converged(self): return self._conv
    def cameras(self): return self._cams
    def points(self): return self._pts
    def outlier_meas(self): return self._om
    def outlier_points(self): return self._op


@functools.lru_cache(maxsize=None)
def oracle_run(case, max_it=None):
    return OracleRun(scene(case), CASES[case][1] if max_it is None else max_it)


def n_free(sc):
    return sum(1 for f in sc["fixed"] if not f)


def precondition(case):
    """What the oracle says about the case (CPU only)."""
    sc, o = scene(case), oracle_run(case)
    acc, trials = o.compute(), o.stats()[2]
    assert acc > 0
    if case == "rejected_trial":
        assert trials > acc
    elif case == "erase_skip_then_erase":
        # every trial of this run is accepted, so k iterations are k steps: the outliers after k steps, step by step
        n = [0]
        for k in range(1, CASES[case][1] + 1):
            ok = oracle_run(case, k)
            assert ok.compute() == k and ok.stats()[2] == k
            n.append(len(ok.outlier_meas()))
        inc = np.diff(n)
        assert any(inc[k] == 0 and inc[k + 1:].max(initial=0) > 0 for k in range(len(inc)))
    elif case == "first_step_outliers":
        assert len(oracle_run(case, 1).outlier_meas()) > 0
    elif case.startswith("nfree_"):
        assert n_free(sc) == int(case[6:])
    elif case == "multi_trip_point":
        per_point = np.zeros(len(sc["pts_init"]), int)
        for (c, p, _, _) in sc["meas"]:
            per_point[p] += bool(sc["fixed"][c])
        assert per_point.max() > 64
    elif case.startswith("chunk_"):
        assert len(sc["meas"]) == int(case[6:])


def device_run(case, mode):
    sc, max_it = scene(case), CASES[case][1]
    vp = capi.default_params(640, 480, 1, ba_max_iterations=max_it, ba_sum_order=mode)
    g = capi.Bundle(vp, 1, len(sc["cams_init"]), len(sc["pts_init"]), len(sc["meas"]))
    load(g, sc)
    g.compute()
    return g


def outcome(g):
    """The fixture's arrays of one problem, all float64."""
    r = g.result(0)
    return {"res": np.array([r["accepted"], r["trials"], r["converged"], r["sigma2"], r["lambda"]], np.float64),
            "cams": g.cameras(0), "pts": g.points(0), "outl": g.outlier_meas(0).astype(np.float64).reshape(-1, 2)}


@pytest.mark.parametrize("case", list(CASES))
def test_case_is_what_it_claims(case):
    """(needs no GPU: the oracle alone)"""
    precondition(case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_reference_order_equals_the_oracle(case):
    precondition(case)
    g = device_run(case, 1)
    check_exact(oracle_run(case), g, 0)
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_fast_mode_within_its_bars_and_bit_equal_to_the_fixture(case):
    precondition(case)
    g = device_run(case, 0)
    got = outcome(g)
    check(oracle_run(case), g, 0, tol=1e-8)
    g.close()
    with np.load(GOLDEN) as z:
        for k, x in got.items():
            want = z[case + "." + k]
            assert x.shape == want.shape and np.array_equal(x, want), (case, k, np.abs(x - want).max() if x.shape == want.shape else (x.shape, want.shape))


if __name__ == "__main__":                                              # record the fixture: python tests/test_gpu_ba_step_paths.py OUT.npz
    if os.environ.get("VSLAM_LIB"):
        capi.load_library(os.environ["VSLAM_LIB"])
    out = {}
    for case in CASES:
        g = device_run(case, 0)
        for k, x in outcome(g).items():
            out[case + "." + k] = x
        g.close()
    np.savez_compressed(sys.argv[1], **out)
    print("recorded", len(CASES), "cases to", sys.argv[1])
