"""GPU test: the tail of a pose iteration as k_pose's chain wavefront runs it (vslam_eval_pose_tail: the 6 x 6 solve in lanes, then
exp(update) * pose) returns the bits of the serial statement -- the Python transcription of lu_solve_n (tests/pose_tail_ref.py, held
to the oracle's solve by tests/test_pose_tail_ref.py), the oracle's se3_exp and pose_mul's product."""
import numpy as np
import pytest

import pose_tail_ref as ref
from visualslam_android_amd import capi


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(ref.CASES))
def test_pose_tail_returns_the_serial_bits(oracle, name):
    sums, pose, what = ref.CASES[name]
    up_ref, ok, _piv = ref.solve_update(sums)
    pose_ref = ref.pose_mul(oracle.se3_exp(up_ref), pose)
    up, out = capi.eval_pose_tail(sums, pose)
    print(name, "update", up, "max |pose - ref|", np.abs(out - pose_ref).max())
    assert np.array_equal(bits(up), bits(up_ref)), (name, up, up_ref)
    assert np.array_equal(bits(out), bits(pose_ref)), (name, out, pose_ref)
    if what == "singular":
        assert not ok and not up.any() and np.array_equal(out, pose)          # a zero update leaves the pose as it is
