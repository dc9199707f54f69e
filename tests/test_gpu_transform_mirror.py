"""GPU test: MapMaker::ApplyGlobalScaleToMap and ApplyGlobalTransformationToMap of the C++ drop-in classes (include/vslam/ptam.h)
against the C call they mirror, through examples/transform_mirror.cpp."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_two_members_give_the_read_backs_of_the_c_call():
    """Two sets of drop-in objects on the same map and frames: one moved by the two members (scale, then rigid transform), one by a single
    vslam_transform_maps.  Pose, velocity, depths, every keyframe pose and every point are equal double for double, the accumulated
    similarity of vslam_get_transform_info is the same after two transforms as after one, and the next tracked frame is equal too."""
    exe = os.path.join(ROOT, "examples", "_build", "transform_mirror")
    assert os.path.exists(exe), "examples/_build/transform_mirror not built (run __graft_entry__.build())"
    out = subprocess.run([exe, "3"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.search(r"members: 2 transforms, C call: 1; (\d+) doubles read back, (\d+) moved, 0 differ; accumulated scale 1\.75\b", out.stdout)
    assert m and int(m.group(1)) > 300 and int(m.group(2)) > 300, out.stdout
    assert "next frame: equal" in out.stdout and "quality good" in out.stdout and "mirror ok" in out.stdout
