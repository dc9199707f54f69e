"""GPU: a handle gives back what it holds on the device -- vslam_destroy, a vslam_create that fails after most of its allocations,
vslam_bundle_destroy.  Free device memory (torch.cuda.mem_get_info after a torch.cuda.synchronize) must not drift downwards over
create/use/destroy cycles: the first cycle is the warm-up, the next four are compared with it.

A guard, not a proof: it sees a leaked handle (gigabytes here), not a leaked 64-byte event, not the few megabytes of a bundle of the
size used below, not the host-side bundle-adjustment workspace, and not a leak on a path where a HIP call itself fails (such a failure
cannot be provoked on a shared machine and must not be).  For those the argument is the code's structure: every acquisition goes
through DevOwner (csrc/vslam_internal.h) and there is one release path.

SLACK, the drift that is allowed, was measured, not chosen: this file was run three times (three processes) against the library built
from the commit before DevOwner, whose code shows no device-memory leak on these paths.  All three runs gave the same figures: no drift
in any case but the first of the process, and there SLACK_MEASURED_DRIFT bytes from the second cycle on, the same in cycles two to
five.  That is the runtime's, not a handle's: scratch memory belongs to a hardware queue, a process has four, a handle's two streams
take the next two in turn, so the second handle of a process is the first to launch on the other pair.  (When the whole suite runs in
one process, every queue has seen every kernel before this file starts and the figure is zero.)  SLACK is twice the measured drift,
because one three-run sample understates the spread, and the handles of the first test are sized so that one of them is more than ten
times SLACK."""
import numpy as np
import pytest
import torch

from ba_scene import ba_scene
from conftest import synth_image
from visualslam_android_amd import capi

pytestmark = pytest.mark.gpu

W, H = 320, 240
S = 4096                                    # streams of a handle of the first test: its footprint must exceed 10 * SLACK (measured: see the test)
S_SMALL = 8
SMALL = dict(max_points=256, max_keyframes=4)
E_INVALID = -1
CYCLES = 4                                  # after the warm-up cycle, where the runtime's own lazy allocations (code objects, scratch) land

SLACK_MEASURED_DRIFT = 436207616            # bytes: largest drift in three runs at the parent commit (416 MiB)
SLACK = 2 * SLACK_MEASURED_DRIFT


def frames(s, n):
    """n frames of s streams [n][s][H][W]: eight different images per frame, repeated over the streams"""
    return np.stack([np.tile(np.stack([synth_image(100 * t + i, W, H) for i in range(8)]), (s // 8, 1, 1)) for t in range(n)])


@pytest.fixture(scope="module")
def device_frames():
    """three frames of S streams in device memory, uploaded once (the allocation is torch's and outlives every measurement below)"""
    fr = torch.from_numpy(frames(8, 3)).cuda().repeat(1, S // 8, 1, 1).contiguous()
    torch.cuda.synchronize()
    return fr


def free_bytes():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def assert_no_drift(cycle, tag):
    """cycle() once as the warm-up, then CYCLES times: free memory never falls more than SLACK below its value after the warm-up"""
    cycle()
    base = free_bytes()
    drift = []
    for _ in range(CYCLES):
        cycle()
        drift.append(base - free_bytes())
    print("%s: free after warm-up %d, drift per cycle %s, slack %d" % (tag, base, drift, SLACK))
    assert max(drift) <= SLACK, (tag, drift)


CONFIGS = {
    "defaults": {},
    # the map-maker's stream ring, ev_asm, ev_ba, ev_reset_ba, the ordered pool
    "async_mapmaker": dict(ba_delay_frames=2, ba_batch_frames=2, use_sbi=1, relocalise=1, grow_map=3, ba_sum_order=1),
    # bootstrap and the idle jobs (both need ba_delay_frames = 0)
    "bootstrap_idle": dict(bootstrap=1, grow_map=3, idle_iterations=1, use_sbi=1, relocalise=1),
}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_destroyed_system_gives_its_device_memory_back(name, device_frames):
    vp = capi.default_params(W, H, S, **SMALL, **CONFIGS[name])
    footprint = []

    def cycle():
        before = free_bytes()
        g = capi.System(vp)
        footprint.append(before - free_bytes())
        g.profile_begin(4)
        for t in range(2):
            g.track_frame_device(device_frames[t].data_ptr(), W, H * W)
        g.profile_end()
        g.reset([3])
        g.track_frame_device(device_frames[2].data_ptr(), W, H * W)
        assert g.state(3).frame == 1 and g.state(0).frame == 3
        g.close()

    assert_no_drift(cycle, name)
    print("%s: footprint of a handle per cycle %s" % (name, footprint))
    assert min(footprint[1:]) > 10 * SLACK, footprint          # a leaked handle would be unmistakable


def test_failed_create_gives_everything_back():
    """ba_alloc refuses max_keyframes = 129 after trk_alloc has allocated the whole map; reloc_alloc refuses a 128 x 64 small image
    (2048 x 1024 frames) after every other *_alloc has run.  What one refused create has allocated by then, from trk_alloc's keyframe
    images alone (streams x keyframes x 1.3 x width x height): 256 x 129 x 102 kB = 3.4 GB, and 1 x 128 x 2.8 MB = 0.36 GB -- so four
    leaked ones are 15 and 1.7 times SLACK."""
    late = [(capi.default_params(W, H, 256, max_points=256, max_keyframes=129), "max_keyframes 129 exceeds 128"),
            (capi.default_params(2048, 1024, 1, max_keyframes=128, relocalise=1), "relocalise: small image of 8192 pixels exceeds 4096")]
    for vp, msg in late:
        def cycle():
            with pytest.raises(capi.VslamError) as e:
                capi.System(vp)
            assert str(e.value) == "vslam error %d: %s" % (E_INVALID, msg), str(e.value)

        base = free_bytes()
        cycle()                                                  # the warm-up
        warm = free_bytes()
        drift = []
        for _ in range(CYCLES):
            cycle()
            drift.append(warm - free_bytes())
        print("%s: free before %d, after warm-up %d, drift per failed create %s, slack %d" % (msg, base, warm, drift, SLACK))
        assert max(drift) <= SLACK, (msg, drift)
    g = capi.System(capi.default_params(W, H, S_SMALL, **SMALL))   # a valid create still succeeds and tracks a frame
    g.track_frame(frames(S_SMALL, 1)[0])
    assert g.state(0).frame == 1
    g.close()


def test_destroyed_bundle_gives_its_device_memory_back():
    n_prob, n_cams, n_pts = 4, 3, 16
    scs = [ba_scene(n_cams=n_cams, n_pts=n_pts, pixel_noise=0.3, outlier_frac=0.0, seed=60 + n) for n in range(n_prob)]
    vp = capi.default_params(640, 480, 1, ba_max_iterations=5)

    def cycle():
        b = capi.Bundle(vp, n_prob, n_cams, n_pts, n_cams * n_pts)
        for n, sc in enumerate(scs):
            for pose, fixed in zip(sc["cams_init"], sc["fixed"]):
                b.add_camera(pose, fixed, problem=n)
            for p in sc["pts_init"]:
                b.add_point(p, problem=n)
            for (c, p, xy, s2) in sc["meas"]:
                b.add_meas(c, p, xy, s2, problem=n)
        out = []
        for _ in range(2):                                       # the second compute starts again from the caller's values
            b.compute()
            out.append([(b.result(n), b.cameras(n).tobytes(), b.points(n).tobytes()) for n in range(n_prob)])
        assert out[0] == out[1]
        b.close()

    assert_no_drift(cycle, "bundle")
