"""GPU: the two mathematical stages of the map bootstrap, observed directly.

vslam_probe_homography_init / vslam_probe_plane_aligner run the device functions InitFromStereo runs (csrc/boot.hip: boot_homography_stage,
boot_plane_stage -- the product kernels call them and nothing else for this part) and return a record of every stage: the matches, the
300 MLESAC scores, the best trial, the MLESAC homography, the inlier list, the refined homography, the chosen decomposition, the scaled
translation; the 100 RANSAC sums, the best plane, the aligner.

The first assertion is everywhere the same: the device's record == the record of the host build of the same header
(oracle/bootmath_host.cpp, the stages restated serially), every integer and every double bit for bit -- what csrc/bootstrap_math.h
promises, and it needs no tolerance.  (A NaN equals a NaN: the sign of a generated NaN is the platform's.)  Well-conditioned cases are
additionally held to the oracle's independent mathematics under the bar of tests/test_bootmath_host.py (16 x the oracle's own +-1 ulp
spread, not below 1e-13); degenerate input is not, because there the oracle's `ok` hangs on the last bits of a different SVD.

The systems are tiny (frames are never uploaded); one has three streams and is probed on stream 2, so the per-stream offsets into
boot_match / boot_inl / boot_ws count.  PARITY UNPINNED against the reference."""
import numpy as np
import pytest

import boot_cases as bc
import oracle.binding as orc
from visualslam_android_amd import capi

pytestmark = pytest.mark.gpu
B = orc.BootMath
P_SMALL, P_VGA = 300, 512                      # 3 * max_points below / above BOOT_MAX_TRAILS: both strides of the boot_ws slices


@pytest.fixture(scope="module")
def small():
    g = capi.System(capi.default_params(64, 48, 3, grow_map=3, bootstrap=1, max_points=P_SMALL))
    yield g
    g.close()


@pytest.fixture(scope="module")
def vga():
    g = capi.System(capi.default_params(640, 480, 1, grow_map=3, bootstrap=1, max_points=P_VGA))
    yield g
    g.close()


def _probe_h(g, stream, m8, seed, tag):
    """device record == host record; returns both"""
    dev = g.probe_homography_init(stream, seed, m8=m8)
    host = B.homography_pipeline(m8, seed, 5.0, g.params.wiggle_scale)
    bc.assert_same_bits(dev, host, tag)
    assert dev.best_trial == (bc.first_argmin(dev.scores[:]) if len(m8) >= 10 else -1), tag
    return dev, host


HOM_CASES = {   # name -> (matches, seed, expected branch of the choice or None)
    "n 4": lambda: (bc.tilted(21, 4), 21), "n 9": lambda: (bc.tilted(21, 9), 21),                   # the direct fit on lane 0
    "n 10": lambda: (bc.tilted(21, 10), 21), "n 11": lambda: (bc.tilted(22, 11), 22),               # the first MLESAC sizes
    "n 255": lambda: (bc.tilted(23, 255), 23), "n 256": lambda: (bc.tilted(24, 256), 24),           # one full compaction pass ...
    "n 257": lambda: (bc.tilted(25, 257), 25),                                                      # ... and one lane of a second
    "n 1000": lambda: (bc.tilted(26, 1000), 26),                                                    # BOOT_MAX_TRAILS
    "outliers in the first 50": lambda: (bc.tilted(27, 300, outliers=50, where="first"), 27),
    "outliers in the last 50": lambda: (bc.tilted(27, 300, outliers=50, where="last"), 27),
    "seed 1": lambda: (bc.tilted(1, 300), 1), "seed 4": lambda: (bc.tilted(4, 300), 4), "seed 11": lambda: (bc.tilted(11, 300), 11),
    "fronto-parallel, z translation": lambda: (bc.fronto_parallel(3, 200, [0.0, 0.0, -0.3], outliers=10), 3),
    "fronto-parallel, x translation": lambda: (bc.fronto_parallel(3, 200, [0.2, 0.0, 0.0], outliers=10), 3),
    "2-pixel noise": lambda: (bc._planar_matches(8, n=200, outliers=20, noise=4e-3)[0], 8),      # the refinement moves the homography
    "quantised to 1/500": lambda: (bc.quantised(bc.tilted(5, 200)), 5),
    "all outliers": lambda: (bc.all_outliers(6, 60), 6),                                            # nearly every trial scores n * 25
    "every match three times": lambda: (np.repeat(bc.tilted(7, 60), 3, axis=0), 7),
}


@pytest.mark.parametrize("name", list(HOM_CASES))
def test_homography_stage_bits_and_oracle(small, name):
    """Well-conditioned match sets at the sizes where boot_homography_stage changes path (see HOM_CASES): device == host bits, then the
    device against the oracle's stages."""
    m8, seed = HOM_CASES[name]()
    dev, host = _probe_h(small, 2, m8, seed, name)
    assert dev.ok == 1 and 4 <= dev.n_inliers <= len(m8), name
    bc.check_homography_against_oracle(dev, m8, seed, name)
    inl = bc.arr(dev.inliers)[:dev.n_inliers]
    assert np.all(np.diff(inl) > 0), name                                 # match order
    if name.startswith("outliers in the"):
        lo, hi = (50, 300) if "first" in name else (0, 250)
        assert np.array_equal(inl[(inl >= lo) & (inl < hi)], np.arange(lo, hi)) and dev.n_inliers < 275, name   # the clean 250 are all in, in order, across both passes
    # which branch of ChooseBestDecomposition this case takes is a property of the scene, read off the HOST record
    if name == "fronto-parallel, z translation":
        assert host.choice in (1, 2), name                                # the visibility votes tie: the Sampson scores decide
    if name in ("seed 1", "seed 4", "seed 11", "fronto-parallel, x translation", "n 1000"):
        assert host.choice == 0, name                                     # the tilted plane / a sideways move: no ambiguity


def test_homography_stage_trial_scan_conditions(small):
    """The first-minimum scan over 300 trials spread on 256 threads: trials 256..299 are the second pass of threads 0..43.  Seeds chosen on
    the CPU so that the best trial is a second-pass one (seed 1: 269), one of threads 0..43's first (seed 11: 12), neither (seed 4: 132), and
    so that some thread's second trial beats its first without being the global best; each condition is asserted from the host's scores."""
    seen_second_better = False
    for seed, want in ((1, 269), (4, 132), (11, 12)):
        m8 = bc.tilted(seed, 300)
        dev, host = _probe_h(small, 2, m8, seed, "seed %d" % seed)
        sc = np.array(host.scores[:])
        assert host.best_trial == want == int(np.argmin(sc)), (seed, host.best_trial)
        second_better = [t for t in range(44) if sc[t + 256] < sc[t] and host.best_trial != t + 256]
        seen_second_better |= len(second_better) > 0
    assert seen_second_better
    assert (269 >= 256) and (12 < 44) and not (132 < 44 or 132 >= 256)


def test_homography_stage_tied_minimum_keeps_the_first_trial(small):
    """Six matches, each ten times over: two trials that draw copies of the same four matches in the same order have the same score to the
    bit.  With these seeds (found on the CPU, asserted here) the MINIMUM is such a pair, on different threads and, for the second, with
    other trials between them: the scan has to keep the first."""
    for under, seed, pair in ((6, 2, (24, 142)), (8, 9, (151, 229))):
        m8 = np.tile(bc.tilted(seed, under, outliers=1), (10, 1))
        dev, host = _probe_h(small, 2, m8, seed, "tied minimum, seed %d" % seed)
        sc = np.array(host.scores[:])
        assert tuple(np.flatnonzero(sc == sc.min())) == pair and dev.best_trial == pair[0] and dev.ok == 1, (seed, np.flatnonzero(sc == sc.min()))


def test_homography_stage_too_few_matches(small):
    for n in (0, 3):
        m8 = bc.tilted(21, 8)[:n]
        dev, host = _probe_h(small, 2, m8, 1, "n %d" % n)
        assert dev.ok == 0 and dev.n_inliers == 0 and dev.best_trial == -1 and not np.any(bc.arr(dev.H_mlesac)), n


@pytest.mark.parametrize("kind", ["pure_rotation", "identity", "collinear", "identical"])
def test_homography_stage_degenerate_input_same_bits(small, kind):
    """Input HomographyInit has no answer for: the device and the host build still agree on every bit, `ok` included, and where `ok` is 1
    every output is finite.  Not compared with the oracle (its `ok` differs from this header's in three of six such cases on the CPU)."""
    for seed in (1, 2, 3):
        m8 = bc.degenerate(kind, seed)
        dev, _ = _probe_h(small, 2, m8, seed, "%s seed %d" % (kind, seed))
        if dev.ok:
            for f in ("H_mlesac", "H_refined", "R", "t", "normal", "t_scaled"):
                assert np.all(np.isfinite(bc.arr(getattr(dev, f)))), (kind, seed, f)
            assert np.isfinite(dev.d) and np.all(np.isfinite(bc.arr(dev.scores)))


def test_homography_stage_streams_keep_their_own_slices(small, vga):
    """The same probe on every stream of the batch with different matches: each record is its own host record (a stream that read or
    wrote another stream's slice of boot_match / boot_inl / boot_ws would return that stream's), also on the one-stream system."""
    sets = [(bc.tilted(31 + s, 120 + 40 * s), 31 + s) for s in range(3)]
    for s in (2, 0, 1):
        _probe_h(small, s, sets[s][0], sets[s][1], "stream %d" % s)
    for s in (0, 1, 2):                                                    # again, after every other stream's slices were written
        _probe_h(small, s, sets[s][0], sets[s][1], "stream %d again" % s)
    _probe_h(vga, 0, sets[1][0], sets[1][1], "one-stream system")


def test_homography_stage_from_integer_pixels(vga):
    """The product's input: integer pixel pairs through the kernel's own UnProject + GetProjectionDerivs (unproject_with_derivs).  A tilted
    plane projected through default_params(640, 480)'s camera and rounded to pixels: the device's Match array == the oracle's
    (both evaluate vslam_libm.h), the rest of the record == the host build fed with those matches, the pose within the bar of the oracle."""
    vp = vga.params
    px = bc.pixel_scene(41, 220, list(vp.cam), vp.width, vp.height)
    assert len(px) > 150
    dev = vga.probe_homography_init(0, 5, matches_xyxy=px)
    m8 = orc.boot_matches(list(vp.cam), vp.width, vp.height, px)
    got = bc.arr(dev.matches)[:8 * len(px)].reshape(-1, 8)
    assert np.array_equal(got.view(np.uint64), m8.view(np.uint64)), np.abs(got - m8).max()
    assert np.abs(m8[:, 5]).max() > 0 and np.abs(m8[:, 4] - m8[:, 7]).max() > 0            # the radial model's derivatives are not a scaled identity
    host = B.homography_pipeline(m8, 5, 5.0, vp.wiggle_scale)
    bc.assert_same_bits(dev, host, "integer pixels")
    assert dev.ok == 1 and dev.n_inliers >= len(px) - 12
    bc.check_homography_against_oracle(dev, m8, 5, "integer pixels")


# ---- the plane aligner -----------------------------------------------------------------------------------------------------------
def _probe_p(g, stream, pos, seed, tag):
    dev = g.probe_plane_aligner(stream, seed, pos)
    host = B.plane_pipeline(pos, seed)
    bc.assert_same_bits(dev, host, tag)
    return dev, host


@pytest.mark.parametrize("n", [9, 10, 100, P_SMALL])
def test_plane_stage_bits_and_oracle(small, n):
    """The slab with 5 % clutter at n = 9 (no aligner), the smallest size that has one, 100 and max_points: device == host bits, the device
    against the oracle's stages, R orthonormal with its third row (the plane normal) pointing back to the camera."""
    pos = bc.plane_cloud(n)
    dev, _ = _probe_p(small, 2, pos, 2, "n %d" % n)
    bc.check_plane_against_oracle(dev, pos, 2, "n %d" % n)
    assert dev.have == (1 if n >= 10 else 0)
    if dev.have:
        R = bc.arr(dev.R).reshape(3, 3)
        assert np.abs(R @ R.T - np.eye(3)).max() <= 16 * np.finfo(float).eps and R[2, 2] <= 0
        Z = (R @ pos.T).T + bc.arr(dev.t)
        assert abs(np.median(Z[:, 2])) < 1e-2                              # the slab went to z = 0


def test_plane_stage_max_points_of_the_other_stride(vga):
    pos = bc.plane_cloud(P_VGA)
    dev, _ = _probe_p(vga, 0, pos, 3, "n %d" % P_VGA)
    bc.check_plane_against_oracle(dev, pos, 3, "n %d" % P_VGA)
    with pytest.raises(capi.VslamError):
        vga.probe_plane_aligner(0, 3, np.r_[pos, pos[:1]])                 # more than max_points


def test_plane_stage_skipped_trials_and_defaults(small):
    """Trials the RANSAC skips and points it skips, device == host bits throughout: forty copies of one point (some trials draw three of them:
    collinear, the negative marker); a point exactly at a trial's mean (the zero-distance skip); all points on one line (every trial is
    skipped, the defaults mean 0, normal (0, 0, 1) go into the aligner); an isotropic cloud."""
    rng = np.random.default_rng(9)
    pos = bc.plane_cloud(100)
    pos[:40] = pos[0]
    dev, host = _probe_p(small, 2, pos, 2, "forty copies")
    sums = np.array(host.sums[:])
    assert (sums < 0).any() and (sums >= 0).any() and dev.have == 1 and sums[dev.best_trial] == sums[sums >= 0].min()

    pos = bc.plane_cloud(60)
    _, mean0, _ = B.plane_trial(pos, 2, 0)
    for j in range(60):                                                    # put a point on trial 0's mean without touching its three points
        q = pos.copy(); q[j] = mean0
        if np.array_equal(B.plane_trial(q, 2, 0)[1], mean0):
            break
    assert np.array_equal(B.plane_trial(q, 2, 0)[1], q[j])
    _probe_p(small, 2, q, 2, "a point at a trial's mean")

    s = rng.uniform(-1, 1, 50)
    line = np.c_[s, np.full(50, 0.5), np.full(50, 0.01)]
    dev, host = _probe_p(small, 2, line, 2, "one line")
    assert (np.array(host.sums[:]) < 0).all() and dev.best_trial == -1 and not np.any(bc.arr(dev.mean)) and list(dev.normal) == [0.0, 0.0, 1.0]
    assert dev.have == 1 and np.all(np.isfinite(bc.arr(dev.R)))          # the line lies within 0.05 of the default plane

    _probe_p(small, 2, rng.normal(0, 0.5, (200, 3)) + [0, 0, 2.0], 2, "isotropic")


def test_plane_stage_streams_keep_their_own_slices(small):
    clouds = [bc.plane_cloud(80 + 60 * s, seed=50 + s) for s in range(3)]
    for s in (1, 2, 0, 2, 1, 0):
        _probe_p(small, s, clouds[s], 7 + s, "stream %d" % s)


def test_probes_are_refused_while_an_initialisation_is_in_progress():
    """VSLAM_E_STATE for the stream whose trails are running (its slices are the initialisation's), for a system without the bootstrap, and
    for more matches than MaxInitialTrails; the other streams are still served."""
    g = capi.System(capi.default_params(64, 48, 2, grow_map=3, bootstrap=1, max_points=P_SMALL))
    m8 = bc.tilted(1, 40)
    frame = np.full((2, 48, 64), 128, np.uint8)                          # no corner, no trail: the press still starts the stage (jni/Tracker.cc:255-258)
    g.press_spacebar(1)
    g.track_frame(frame)
    assert g.init_info(1)["stage"] == 1 and g.init_info(0)["stage"] == 0
    with pytest.raises(capi.VslamError):
        g.probe_homography_init(1, 1, m8=m8)
    with pytest.raises(capi.VslamError):
        g.probe_plane_aligner(1, 1, bc.plane_cloud(20))
    bc.assert_same_bits(g.probe_homography_init(0, 1, m8=m8), B.homography_pipeline(m8, 1, 5.0, g.params.wiggle_scale), "the other stream")
    with pytest.raises(capi.VslamError):
        g.probe_homography_init(0, 1, m8=np.zeros((1001, 8)))
    g.close()
    g = capi.System(capi.default_params(64, 48, 1))
    with pytest.raises(capi.VslamError):
        g.probe_homography_init(0, 1, m8=m8)
    g.close()
