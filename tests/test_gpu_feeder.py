"""The feeder's device renderer (vslam_feeder_render_device, bench.py's set-up) against the host feeder: the same bytes."""
import numpy as np
import pytest
import torch

from visualslam_android_amd import feeder

pytestmark = pytest.mark.gpu


def test_render_device_is_byte_identical_to_the_host_feeder():
    W, H, T = 640, 480, 3
    fs = [feeder.Feeder(W, H, seed=1234 + s) for s in range(3)]
    times = [-160, -20, 0, 1, 2]
    poses = np.array([[f.pose(t) for t in times] for f in fs])
    keys = np.array([[1000, 1007, 100000, 100001, 100002]] * len(fs), np.uint64)
    out = torch.full((len(fs) + 1, len(times), H, W), 7, dtype=torch.uint8, device="cuda")   # one feeder's worth of guard
    feeder.render_device(fs, poses, keys, out.data_ptr(), len(times) * H * W, H * W)
    got = out.cpu().numpy()
    for i, f in enumerate(fs):
        for j, t in enumerate(times):
            assert np.array_equal(got[i, j], f.render_pose(poses[i, j], key=int(keys[i, j]))), (i, t)
        assert np.array_equal(got[i, 2:], f.render(0, T))                          # render()'s frames: pose(t), key t + 100000
    assert (got[len(fs)] == 7).all()                                                  # nothing written past the last feeder
    ring = torch.full((len(fs) + 1, 4, H, W), 7, dtype=torch.uint8, device="cuda")
    feeder.render_device(fs, None, None, ring.data_ptr(), 4 * H * W, H * W, first=5, count=3)   # frames 5 .. 7 of render()
    got = ring.cpu().numpy()
    for i, f in enumerate(fs):
        assert np.array_equal(got[i, :3], f.render(5, 3))
    assert (got[:, 3] == 7).all() and (got[len(fs)] == 7).all()                      # count frames per feeder, nothing more
    for f in fs:
        f.close()
