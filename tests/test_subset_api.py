"""CPU test: the subset-step entry points exist in every layer -- include/vslam_c.h declares them, capi.py binds them with the
header's argument lists, and the built library exports them."""
import ctypes
import os
import re

from visualslam_android_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vslam_make_keyframe_lite_subset", "vslam_track_frame_subset", "vslam_get_step_streams")


def test_subset_entry_points_are_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "vslam_c.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(capi.LIB_PATH)
    for name in NEW:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, "include/vslam_c.h does not declare %s" % name
        n_args = len(m.group(1).split(","))
        assert name in capi.SYMBOLS, "capi.py does not bind %s" % name
        res, args = capi.SYMBOLS[name]
        assert res is ctypes.c_int and len(args) == n_args, (name, n_args, args)
        assert hasattr(lib, name), "libvslam_hip.so does not export %s" % name
    # the two step calls take the list before the image arguments of vslam_track_frame
    assert len(capi.SYMBOLS["vslam_track_frame_subset"][1]) == len(capi.SYMBOLS["vslam_track_frame"][1]) + 2
    for meth in ("track_frame_subset", "make_keyframe_lite_subset", "step_streams"):
        assert callable(getattr(capi.System, meth))
