"""The two combinations of map-maker jobs that no other test reaches, as a characterisation of the map-maker's host driver
(csrc/ba.hip): a host-driven AddKeyFrame beside the asynchronous map-maker, and a BundleAdjustAll that first has to collect an
adjustment still in flight.  In both, a system with ba_delay_frames = 3 must leave the same bits as one with ba_delay_frames = 0:
the kernels read the same map, only the stream they run on and the moment of the write-back differ.
The driver's kernels themselves (k_ba_select, k_ba_assemble, k_ba_writeback) are held to the oracle where they branch by
tests/test_gpu_mapmaker_edges.py, on the hand-built maps of tests/mapmaker_cases.py."""
import numpy as np
import pytest

from helpers import make_scene
from visualslam_android_amd import capi

pytestmark = pytest.mark.gpu

W, H = 320, 240
_scene = []


def scene():
    if not _scene:
        _scene.append(make_scene(W, H, seed=1234, n_frames=2, per_level=(120, 50, 20, 8)))
    return _scene[0]


def system(delay):
    f, m, _frames = scene()
    g = capi.System(capi.default_params(W, H, 1, ba_delay_frames=delay))
    g.load_map(0, m)
    g.set_pose(0, f.pose(-1))
    return g


def read_back(g):
    st = g.state(0)
    return {"n_keyframes": st.n_keyframes, "ba_accepted": st.ba_accepted, "n_ba_trials": st.n_ba_trials, "pose": np.array(st.pose[:]),
            "kf_poses": np.stack([g.keyframe_pose(0, k) for k in range(st.n_keyframes)]), "points": g.points(0)}


def assert_same_bits(a, b):
    for key in ("n_keyframes", "ba_accepted", "n_ba_trials"):
        assert a[key] == b[key], (key, a[key], b[key])
    assert np.array_equal(a["pose"], b["pose"])
    assert np.array_equal(a["kf_poses"], b["kf_poses"]), np.abs(a["kf_poses"] - b["kf_poses"]).max()
    assert np.array_equal(a["points"]["pos"], b["points"]["pos"]), np.abs(a["points"]["pos"] - b["points"]["pos"]).max()
    assert np.array_equal(a["points"]["bad"], b["points"]["bad"])


def test_host_driven_add_keyframe_beside_the_asynchronous_mapmaker():
    """vslam_add_keyframe is adjusted at once even where the tracker's own keyframes go to the map-maker streams."""
    _f, m, frames = scene()
    out = []
    for delay in (0, 3):
        g = system(delay)
        g.set_last_keyframe_dropped(0, 0)                   # the tracker asks for no keyframe of its own
        g.track_frame(frames[0][None])
        assert g.state(0).n_keyframes == len(m["keyframes"]) and not g.state(0).kf_added
        g.add_keyframe_now(0)
        out.append(read_back(g))
        g.close()
    assert out[0]["n_keyframes"] == len(m["keyframes"]) + 1 and out[0]["n_ba_trials"] > 0
    assert_same_bits(out[0], out[1])


def test_bundle_adjust_all_with_an_adjustment_in_flight():
    """Frame 0 adds a keyframe; BundleAdjustAll right after it first drains that keyframe's pending BundleAdjustRecent."""
    _f, m, frames = scene()
    out = []
    for delay in (0, 3):
        g = system(delay)
        g.track_frame(frames[0][None])
        st = g.state(0)
        assert st.kf_added and st.n_keyframes == len(m["keyframes"]) + 1
        trials_after_frame = st.n_ba_trials                 # delay 3: the keyframe's adjustment has not been written back yet
        g.bundle_adjust_all()
        out.append(read_back(g))
        assert out[-1]["n_ba_trials"] > trials_after_frame
        g.close()
    assert_same_bits(out[0], out[1])
