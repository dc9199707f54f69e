"""CPU: the overlay renderer's surface -- include/vslam_c.h declares it, libvslam_hip.so exports it, capi binds it, and the new
parameter defaults to off.  No GPU."""
import ctypes
import os
import re

from visualslam_android_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ("vslam_render_overlay", "vslam_get_overlay_info", "vslam_get_render_timing", "vslam_eval_overlay")
FLAGS = {"VSLAM_DRAW_POINTS": 1, "VSLAM_DRAW_TRAILS": 2, "VSLAM_DRAW_FAST": 4, "VSLAM_DRAW_IN_PLACE": 8, "VSLAM_DRAW_ALPHA0": 16}


def header():
    return open(os.path.join(ROOT, "include", "vslam_c.h")).read()


def test_header_declares_the_four_functions_and_five_flags():
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for f in FUNCTIONS:
        assert re.search(r"\bint\s+%s\s*\(" % f, text), f
    for name, value in FLAGS.items():
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), text), name
    body = text[text.index("typedef struct vslam_params"):text.index("} vslam_params;")]
    assert re.search(r"\bint\s+overlay\s*;", body), "overlay is a member of vslam_params"


def test_library_exports_and_capi_binds_them():
    lib = ctypes.CDLL(capi.LIB_PATH)
    for f in FUNCTIONS:
        assert hasattr(lib, f), f
        assert f in capi.SYMBOLS, f
    assert len(capi.SYMBOLS["vslam_render_overlay"][1]) == 8 and len(capi.SYMBOLS["vslam_eval_overlay"][1]) == 13
    assert (capi.DRAW_POINTS, capi.DRAW_TRAILS, capi.DRAW_FAST, capi.DRAW_IN_PLACE, capi.DRAW_ALPHA0) == tuple(FLAGS.values())
    for m in ("render_overlay", "render_overlay_device", "overlay_info", "render_timing"):
        assert callable(getattr(capi.System, m)), m
    assert callable(capi.eval_overlay)


def test_overlay_defaults_to_off_and_the_mirror_lists_the_fields_in_the_headers_order():
    p = capi.default_params(640, 480, 2)
    assert p.overlay == 0
    names = [f[0] for f in capi.Params._fields_]
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    body = text[text.index("typedef struct vslam_params"):text.index("} vslam_params;")]
    declared = re.findall(r"(\w+)\s*(?:\[[^\]]*\])?\s*[;,]", body)
    assert "overlay" in names and [n for n in declared if n in names] == names
    assert capi.default_params(640, 480, 2, overlay=1).overlay == 1


def test_the_hook_validates_its_arguments_before_it_looks_for_a_device():
    import numpy as np
    import pytest
    g = np.zeros((48, 48), np.uint8)
    with pytest.raises(capi.VslamError, match="error -1"):
        capi.eval_overlay(g, flags=capi.DRAW_POINTS)                      # only IN_PLACE and ALPHA0 mean something to the hook
    with pytest.raises(capi.VslamError, match="error -1"):
        capi.eval_overlay(g, discs=[(1, 1, 4)])                           # a level outside 0..3
    with pytest.raises(capi.VslamError, match="error -1"):
        capi.eval_overlay(g, lines=[(0, 0, 40000, 3)])                    # a coordinate beyond +-32767
    with pytest.raises(capi.VslamError, match="error -1"):
        capi.eval_overlay(g, row_stride=4 * 48 - 1)
