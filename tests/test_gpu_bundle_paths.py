"""GPU parity of every code path of the device Bundle::Compute (ba_device.h / ba_ordered.h) against the oracle's Bundle, in both
summation modes: vslam_params.ba_sum_order = 1 must give the oracle's bits (check_exact), the fast mode (0) its results within
the fixed bars of check() where two cameras fix the gauge, and -- for one Levenberg-Marquardt trial -- no further from an
extended-precision solve of the full normal equations (tests/ba_hp.py) than the oracle's sequential fp64 sums are.

The problem shape picks the path: adjustable cameras (1-5 one matrix-core group + register solve, 6-10 two groups + LDS solve,
11-64 wave-per-block reduced system + global solve, > 64 refused), measurements (<= 4096 vs more: the two radix selects of the
Tukey median), measurements of one point in one region (> 64: a chunk of several trips), fixed cameras anywhere in the list.

Which test reaches which branch (every one in both modes):
  one matrix-core group + register solve (1-5 adjustable)      test_nfree_sweep[1..5], test_one_trial_against_extended_precision[1, 5]
  two groups + LDS solve (6-10, 10 = BA_FAST_FREE)              test_nfree_sweep[6..10], test_one_trial_...[6, 10]
  wave-per-block S, global solve, storeAll (11-64)              test_nfree_sweep[11..64], test_one_trial_...[11, 32],
                                                                test_bundle_adjust_all_sixteen_keyframes (through k_ba_assemble)
  refusal, accepted = -1 (> 64)                                 test_more_than_64_adjustable_cameras_are_refused
  radix select <8> / <16> at M = 4095 / 4096 / 4097 / 65536     test_median_select_edges (ties: groups of identical points)
  multi-trip chunk with carry (> 64 slots of one point)         test_long_tracks_in_the_fixed_region (65 and 100 fixed cameras)
  fixed cameras not first (SL_FORD ordinals)                    test_fixed_camera_placement
  shuffled AddMeas order                                        test_shuffled_measurement_order
  duplicated (camera, point) measurement: refused               test_duplicate_measurements_are_refused
  vslam_bundle_set_problem                                      test_set_problem_equals_add_calls
  capacity 128 / 4096 / 65536 and one over                      test_full_capacity_problem, test_capacity_limits_are_enforced
  problems of every path in one launch                          test_heterogeneous_launch_matches_problems_alone"""
import numpy as np
import pytest

import ba_hp
from ba_paths_scene import CAM, HP_NFREE, arrays, hp_scene, paths_scene
from oracle import binding as orc
from test_gpu_bundle import check, check_exact, load
from visualslam_android_amd import capi

pytestmark = pytest.mark.gpu

MODES = (0, 1)


def caps(sc):
    return max(len(sc["cams_init"]), 1), max(len(sc["pts_init"]), 1), max(len(sc["meas"]), 1)


def oracle_for(sc, max_it):
    o = orc.OracleBundle(CAM, 640, 480, max_iterations=max_it)
    load(o, sc)
    return o


def run(sc, mode, max_it=6, tol=1e-8, capacity=None):
    """sc on the device alone and in the oracle; the mode's check.  -> the device Bundle (closed by the caller)"""
    vp = capi.default_params(640, 480, 1, ba_max_iterations=max_it, ba_sum_order=mode)
    g = capi.Bundle(vp, 1, *(capacity or caps(sc)))
    load(g, sc)
    g.compute()
    o = oracle_for(sc, max_it)
    if mode:
        check_exact(o, g, 0)
    else:
        check(o, g, 0, tol=tol)
    o.close()
    return g


def n_free(sc):
    return sum(1 for f in sc["fixed"] if not f)


# ---- adjustable cameras: every form of the reduced camera system ------------------------------------------------------------
NFREE_SWEEP = tuple(range(1, 13)) + (16, 24, 32, 48, 64)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nfree", NFREE_SWEEP)
def test_nfree_sweep(nfree, mode):
    # two fixed cameras fix the gauge (scale included): the fast mode's bar is check()'s 1e-8 on cameras, 1e-7 on points
    sc = paths_scene(nfree + 2, 48 if nfree > 24 else 64, fixed=(0, 1), visibility=0.6, outlier_frac=0.03, seed=200 + nfree)
    assert n_free(sc) == nfree
    g = run(sc, mode, max_it=5)
    assert g.result(0)["accepted"] > 0
    g.close()


@pytest.mark.parametrize("mode", MODES)
def test_more_than_64_adjustable_cameras_are_refused(mode):
    """The documented limit (vslam_c.h, vslam_bundle_create): 65 adjustable cameras -> accepted = -1, nothing moves."""
    sc = paths_scene(66, 40, fixed=(0,), visibility=0.5, seed=265)
    vp = capi.default_params(640, 480, 1, ba_max_iterations=5, ba_sum_order=mode)
    g = capi.Bundle(vp, 1, *caps(sc))
    load(g, sc)
    g.compute()
    r = g.result(0)
    assert r["accepted"] == -1 and r["trials"] == 0 and not r["converged"]
    assert np.array_equal(g.cameras(0), np.asarray(sc["cams_init"])) and np.array_equal(g.points(0), np.asarray(sc["pts_init"]))
    assert len(g.outlier_meas(0)) == 0
    g.close()


# ---- where the fixed cameras sit in the list (SL_FORD ordinals, start rows) --------------------------------------------------
def placement(nfree, kind):
    if kind == "first":
        n, fixed = nfree + 2, (0, 1)
    elif kind == "last":
        n, fixed = nfree + 2, (nfree, nfree + 1)
    elif kind == "alternating":
        n, fixed = 2 * nfree + 1, tuple(range(0, 2 * nfree + 1, 2))
    else:                                                            # "unmeasured": a fixed camera in the middle that nothing sees
        n, fixed = nfree + 3, (0, nfree // 2 + 1, nfree + 2)
    sc = paths_scene(n, 48, fixed=fixed, visibility=0.6, outlier_frac=0.03, seed=300 + nfree + 7 * len(kind))
    if kind == "unmeasured":
        dead = nfree // 2 + 1
        sc["meas"] = [m for m in sc["meas"] if m[0] != dead]
    assert n_free(sc) == nfree
    return sc


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", ["first", "last", "alternating", "unmeasured"])
@pytest.mark.parametrize("nfree", [3, 8, 20])
def test_fixed_camera_placement(nfree, kind, mode):
    g = run(placement(nfree, kind), mode, max_it=5)
    assert g.result(0)["accepted"] > 0
    g.close()


# ---- degenerate points and long tracks in one region (the multi-trip chunk of the step sweep) --------------------------------
def long_track_scene():
    """100 fixed + 28 adjustable cameras (fixed ones interleaved).  Point 0: seen once (adjustable camera); 1: only by fixed
    cameras (3); 2 / 3 / 4: by exactly 64 / 65 / 100 fixed cameras (region X: one chunk of 64 slots, then two trips, two trips);
    5: by all 128 (100 in X, 28 in F); 6: 33 adjustable + 32 fixed = 65 slots over both regions (no multi-trip chunk)."""
    n = 128
    adj = list(range(2, 128, 4)) + [127]                           # 32 + 1 - 5 = 28 adjustable cameras, spread over the list
    adj = sorted(set(adj[:28]))
    fixed = [j for j in range(n) if j not in adj]
    tracks = {0: [adj[3]], 1: fixed[:3], 2: fixed[:64], 3: fixed[:65], 4: fixed[:100], 5: list(range(n)),
              6: sorted(adj[:28] + fixed[:37])}
    sc = paths_scene(n, 40, fixed=fixed, tracks=tracks, visibility=0.3, outlier_frac=0.02, seed=400)
    cnt = {}
    for (c, p, _, _) in sc["meas"]:
        cnt[p] = cnt.get(p, 0) + 1
    assert [cnt[p] for p in range(7)] == [1, 3, 64, 65, 100, 128, 65] and n_free(sc) == 28
    return sc


def long_track_f_scene():
    """64 adjustable cameras (the most a problem adjusts) and 2 fixed: point 0 is seen by all 64 adjustable ones (region F: one
    full chunk) and one fixed camera, point 1 by all 66."""
    n = 66
    tracks = {0: list(range(1, 65)) + [0], 1: list(range(n))}
    sc = paths_scene(n, 40, fixed=(0, 65), tracks=tracks, visibility=0.4, outlier_frac=0.02, seed=401)
    return sc


@pytest.mark.parametrize("mode", MODES)
def test_long_tracks_in_the_fixed_region(mode):
    g = run(long_track_scene(), mode, max_it=5)
    assert g.result(0)["accepted"] > 0
    g.close()


@pytest.mark.parametrize("mode", MODES)
def test_long_tracks_in_the_adjustable_region(mode):
    g = run(long_track_f_scene(), mode, max_it=4)
    assert g.result(0)["accepted"] > 0
    g.close()


# ---- the Tukey median: radix select <8> (M <= 4096) and <16> (M > 4096) ---------------------------------------------------
def median_scene(M, ties=False):
    if M == 65536:
        return full_scene()
    if ties:   # groups of 8 identical points, observations exact projections rounded to whole pixels: the squared errors tie
        sc = paths_scene(8, 800, fixed=(0, 1), visibility=1.0, pixel_noise=0.0, quantize=True, tie_group=8, seed=500 + M)
    else:
        sc = paths_scene(10, 520, fixed=(0, 1), visibility=1.0, outlier_frac=0.03, seed=510 + M % 97)
    assert len(sc["meas"]) >= M
    sc["meas"] = sc["meas"][:M]
    return sc


MEDIAN_CASES = [(4095, False), (4096, False), (4097, False), (4096, True), (4097, True), (65536, False)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("M,ties", MEDIAN_CASES)
def test_median_select_edges(M, ties, mode):
    sc = median_scene(M, ties)
    if ties:
        e2 = first_step_squared_errors(sc)
        assert len(e2) - len(np.unique(e2)) > M // 2                   # most squared errors tie with another one
    # one step: sigma^2 comes from the start state, which both sides project with the same expressions -> equal bits in BOTH
    # modes (selection does not depend on summation order)
    vp = capi.default_params(640, 480, 1, ba_max_iterations=1, ba_sum_order=mode)
    g = capi.Bundle(vp, 1, *caps(sc))
    load(g, sc)
    g.compute()
    o = oracle_for(sc, 1)
    o.compute()
    assert g.result(0)["sigma2"] == o.stats()[0]
    assert len(g.outlier_meas(0)) == len(o.outlier_meas())
    g.close(); o.close()
    if M < 65536:                                                      # (the full run of the 65536 problem: test_full_capacity_problem)
        run(sc, mode, max_it=4).close()


def first_step_squared_errors(sc):
    """The squared errors pass 1 of Do_LM_Step computes at the start state (numpy, fp64; for counting ties only)."""
    from ba_scene import project
    out = []
    for (c, p, xy, s2) in sc["meas"]:
        im, z = project(sc["cams_init"][c], sc["pts_init"][p])
        out.append(float(((xy - im) ** 2).sum() / s2))
    return np.array(out)


# ---- measurement order and duplicates --------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nfree", [3, 8, 20])
def test_shuffled_measurement_order(nfree, mode):
    sc = paths_scene(nfree + 2, 60, fixed=(1, nfree), visibility=0.6, outlier_frac=0.04, shuffle=True, seed=600 + nfree)
    g = run(sc, mode, max_it=5)
    assert g.result(0)["accepted"] > 0 and len(g.outlier_meas(0)) > 0
    g.close()


@pytest.mark.parametrize("mode", MODES)
def test_duplicate_measurements_are_refused(mode):
    """vslam_c.h: at most one measurement per (camera, point); add_meas and set_problem refuse a second with VSLAM_E_INVALID and
    leave the problem as it was -- the result is then the oracle's on the list without the duplicate."""
    sc = paths_scene(7, 50, fixed=(0, 4), visibility=0.7, outlier_frac=0.03, seed=700)
    dup = paths_scene(7, 50, fixed=(0, 4), visibility=0.7, outlier_frac=0.03, seed=700, duplicates=1)
    assert len(dup["meas"]) == len(sc["meas"]) + 1
    vp = capi.default_params(640, 480, 1, ba_max_iterations=5, ba_sum_order=mode)
    g = capi.Bundle(vp, 2, *caps(dup))
    load(g, sc)
    c, p, xy, s2 = dup["meas"][-1]
    with pytest.raises(capi.VslamError, match="error -1:"):
        g.add_meas(c, p, xy, s2)
    g.set_problem(1, *arrays(sc))
    with pytest.raises(capi.VslamError, match="error -1:"):
        g.set_problem(1, *arrays(dup))
    g.compute()
    for n in range(2):
        o = oracle_for(sc, 5)
        (check_exact(o, g, n) if mode else check(o, g, n))
        o.close()
    g.close()


# ---- capacity ---------------------------------------------------------------------------------------------------------------
def full_scene():
    """A problem at every capacity limit: 128 cameras (64 adjustable, 64 fixed, alternating), 4096 points, 65536 measurements."""
    sc = paths_scene(128, 4096, fixed=tuple(range(0, 128, 2)), visibility=0.135, outlier_frac=0.02, seed=800)
    assert len(sc["meas"]) >= 65536
    sc["meas"] = sc["meas"][:65536]
    return sc


@pytest.mark.parametrize("mode", MODES)
def test_full_capacity_problem(mode):
    sc = full_scene()
    assert n_free(sc) == 64
    g = run(sc, mode, max_it=3, capacity=(128, 4096, 65536))
    assert g.result(0)["accepted"] > 0
    g.close()


def test_capacity_limits_are_enforced():
    vp = capi.default_params(640, 480, 1)
    for over in ((129, 16, 16), (4, 4097, 16), (4, 16, 65537), (0, 16, 16), (4, 0, 16), (4, 16, 0)):
        with pytest.raises(capi.VslamError, match="error -1:"):
            capi.Bundle(vp, 1, *over)
    g = capi.Bundle(vp, 1, 128, 4096, 65536)
    pose = np.r_[np.eye(3).ravel(), 0, 0, 1.0]
    for j in range(128):
        g.add_camera(pose, j % 2 == 0)
    with pytest.raises(capi.VslamError, match="error -3:"):
        g.add_camera(pose, False)
    g.set_problem(0, np.tile(pose, (17, 1)), [1] + [0] * 16, np.zeros((4096, 3)), np.repeat(np.arange(16), 4096), np.tile(np.arange(4096), 16),
                  np.full((65536, 2), 320.0), np.ones(65536))
    with pytest.raises(capi.VslamError, match="error -3:"):
        g.add_point([0.0, 0.0, 0.0])
    with pytest.raises(capi.VslamError, match="error -3:"):
        g.add_meas(16, 0, [320.0, 240.0], 1.0)                     # a new (camera, point) pair, one past the measurement capacity
    for bad in ((129, 4096, 1), (2, 4097, 1), (2, 4096, 65537)):
        nc, npt, nm = bad
        with pytest.raises(capi.VslamError, match="error -3:"):
            g.set_problem(0, np.tile(pose, (nc, 1)), [1] * nc, np.zeros((npt, 3)), [0] * nm, [0] * nm, np.full((nm, 2), 320.0), np.ones(nm))
    g.close()


# ---- bulk upload -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_set_problem_equals_add_calls(mode):
    scs = [paths_scene(10, 80, fixed=(3, 7), visibility=0.6, outlier_frac=0.03, shuffle=True, seed=900),
           paths_scene(22, 60, fixed=(0, 21), visibility=0.5, outlier_frac=0.03, seed=901)]
    vp = capi.default_params(640, 480, 1, ba_max_iterations=5, ba_sum_order=mode)
    g = capi.Bundle(vp, 4, 22, 80, 2048)
    for k, sc in enumerate(scs):
        load(g, sc, problem=2 * k)
        g.set_problem(2 * k + 1, *arrays(sc))
    g.compute()
    for k, sc in enumerate(scs):
        a, b = 2 * k, 2 * k + 1
        assert g.result(a) == g.result(b)
        assert np.array_equal(g.cameras(a), g.cameras(b)) and np.array_equal(g.points(a), g.points(b))
        assert np.array_equal(g.outlier_meas(a), g.outlier_meas(b)) and np.array_equal(g.outlier_points(a), g.outlier_points(b))
        o = oracle_for(sc, 5)
        (check_exact(o, g, b) if mode else check(o, g, b))
        o.close()
    g.close()


# ---- one heterogeneous launch -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_heterogeneous_launch_matches_problems_alone(mode):
    """nfree 3, 8, 20 and 64, an empty problem and a refused one (65 adjustable cameras) in one launch: each gives the bits it
    gives alone (nothing leaks between problems), and the oracle's result."""
    scs = [paths_scene(5, 60, fixed=(0, 4), visibility=0.7, outlier_frac=0.03, seed=1000),
           paths_scene(10, 60, fixed=(2, 9), visibility=0.6, outlier_frac=0.03, seed=1001),
           paths_scene(22, 50, fixed=(0, 11), visibility=0.5, outlier_frac=0.03, seed=1002),
           paths_scene(66, 40, fixed=(0, 33), visibility=0.4, outlier_frac=0.03, seed=1003),
           None,
           paths_scene(66, 30, fixed=(0,), visibility=0.4, seed=1004)]
    cap = (66, 60, max(len(s["meas"]) for s in scs if s))
    vp = capi.default_params(640, 480, 1, ba_max_iterations=4, ba_sum_order=mode)

    def outcome(g, n):
        return g.result(n), g.cameras(n), g.points(n), g.outlier_meas(n), g.outlier_points(n)

    alone = []
    for sc in scs:
        g = capi.Bundle(vp, 1, *cap)
        if sc:
            load(g, sc)
        g.compute()
        alone.append(outcome(g, 0))
        g.close()
    g = capi.Bundle(vp, len(scs), *cap)
    for n, sc in enumerate(scs):
        if sc:
            load(g, sc, problem=n)
    g.compute()
    for n, sc in enumerate(scs):
        got = outcome(g, n)
        assert got[0] == alone[n][0], n
        for x, y in zip(got[1:], alone[n][1:]):
            assert np.array_equal(x, y), n
        if sc is None:
            continue
        if n == 5:
            assert got[0]["accepted"] == -1 and np.array_equal(got[1], np.asarray(sc["cams_init"]))
            continue
        o = oracle_for(sc, 4)
        (check_exact(o, g, n) if mode else check(o, g, n))
        o.close()
    g.close()


# ---- one trial against the extended-precision solve of the full normal equations ---------------------------------------------
@pytest.mark.parametrize("key", [str(n) for n in HP_NFREE] + ["config3"])
def test_one_trial_against_extended_precision(key):
    """Fast mode: max|gpu - hp| <= 8 max|oracle - hp| + 16 eps max|hp| (cameras and points), i.e. no worse than a sequential fp64
    sum; ordered mode: the oracle's bits."""
    sc = hp_scene(key)
    hp = ba_hp.first_trial(CAM, 640, 480, sc["cams_init"], sc["fixed"], sc["pts_init"], sc["meas"])
    assert hp["new_err"] < hp["cur_err"]
    for mode in MODES:
        vp = capi.default_params(640, 480, 1, ba_max_iterations=1, ba_sum_order=mode)
        g = capi.Bundle(vp, 1, *caps(sc))
        load(g, sc)
        g.compute()
        o = oracle_for(sc, 1)
        if mode:
            check_exact(o, g, 0)
        else:
            assert o.compute() == 1 and g.result(0)["accepted"] == 1 and g.result(0)["trials"] == 1
            assert g.result(0)["sigma2"] == o.stats()[0]
            for got, want, ref in ((g.cameras(0), hp["cams"], o.cameras()), (g.points(0), hp["pts"], o.points())):
                dg, allowed, do = ba_hp.bar(got, ref, want)
                assert dg <= allowed, (key, dg, allowed, do)
            assert np.array_equal(o.outlier_meas(), g.outlier_meas(0))
        o.close(); g.close()


# ---- the system path: BundleAdjustAll over 16 keyframes (k_ba_assemble -> the wave-per-block reduced system) -----------------
@pytest.mark.parametrize("mode", MODES)
def test_bundle_adjust_all_sixteen_keyframes(mode):
    from helpers import make_oracle, make_scene, pose_err
    w, h = 320, 240
    f, m, frames = make_scene(w, h, seed=23, n_frames=2, n_keyframes=16, per_level=(120, 50, 20, 8), point_noise=0.004,
                              pose_noise=(0.003, 0.002))
    vp = capi.default_params(w, h, 1, ba_sum_order=mode)
    o = make_oracle(vp, m, f.pose(-1))
    g = capi.System(vp)
    g.load_map(0, m)
    g.set_pose(0, f.pose(-1))
    acc = o.bundle_adjust_all()
    g.bundle_adjust_all()
    sg = g.state(0)
    assert sg.n_keyframes == 16
    assert sg.ba_accepted == acc and acc > 0 and sg.n_ba_trials == o.state().n_ba_trials
    po, pg = o.points(), g.points(0)
    assert np.array_equal(po["bad"], pg["bad"])
    if mode:
        for k in range(sg.n_keyframes):
            assert np.array_equal(np.asarray(o.keyframe_pose(k)), np.asarray(g.keyframe_pose(0, k))), k
        assert np.array_equal(po["pos"], pg["pos"])
    else:
        for k in range(sg.n_keyframes):
            assert pose_err(o.keyframe_pose(k), g.keyframe_pose(0, k)) < 1e-8
        assert np.abs(po["pos"] - pg["pos"]).max() < 1e-8
    g.close()
