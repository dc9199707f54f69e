"""CPU test: the map merge is declared, exported and bound alike; it adds no member to vslam_params; bad arguments are refused before
anything needs a device."""
import ctypes
import os
import re
import subprocess

from visualslam_android_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vslam_merge_maps", "vslam_get_merge_info", "vslam_get_merge_timing")
E_INVALID = -1


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vslam_c.h")).read(), flags=re.S)


def test_header_library_and_binding_agree_on_the_merge_symbols():
    text = header()
    lib = ctypes.CDLL(capi.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(\s*vslam_system\s*\*" % name, text), name
        assert hasattr(lib, name), "libvslam_hip.so does not export %s" % name
        assert name in capi.SYMBOLS
    assert re.search(r"vslam_merge_maps\s*\(\s*vslam_system\s*\*\s*sys\s*,\s*const\s+int\s*\*\s*dst\s*,\s*const\s+int\s*\*\s*src\s*,\s*int\s+n\s*\)", text)
    assert re.search(r"vslam_get_merge_info\s*\(\s*vslam_system\s*\*\s*sys\s*,\s*int\s+stream\s*,\s*int\s+out\[6\]\s*\)", text)
    assert re.search(r"vslam_get_merge_timing\s*\(\s*vslam_system\s*\*\s*sys\s*,\s*double\s*\*\s*ms\s*\)", text)
    assert text.index("vslam_fit_similarity") < text.index("vslam_merge_maps")          # a block of its own behind the similarity transform's
    assert len(capi.SYMBOLS["vslam_merge_maps"][1]) == 4 and len(capi.SYMBOLS["vslam_get_merge_info"][1]) == 3
    assert callable(capi.System.merge_maps) and callable(capi.System.merge_info) and callable(capi.System.merge_timing)


def test_bad_arguments_are_refused_without_a_system():
    lib = capi.load_library()
    one = (ctypes.c_int * 1)(0)
    out = (ctypes.c_int * 6)()
    ms = ctypes.c_double(0.0)
    assert lib.vslam_merge_maps(None, one, one, 1) == E_INVALID
    assert b"merge" in lib.vslam_last_error()
    assert lib.vslam_merge_maps(None, one, one, -1) == E_INVALID
    assert lib.vslam_merge_maps(None, None, None, 0) == E_INVALID
    assert lib.vslam_get_merge_info(None, 0, out) == E_INVALID
    assert b"merge" in lib.vslam_last_error()
    assert lib.vslam_get_merge_timing(None, ctypes.byref(ms)) == E_INVALID
    assert b"merge" in lib.vslam_last_error()


def test_vslam_params_is_unchanged_and_keyframe_retire_is_still_last(tmp_path):
    body = header()
    body = body[body.index("typedef struct vslam_params"):body.index("} vslam_params;")]
    assert re.search(r"int\s+keyframe_retire\s*;\s*$", body) and "merge" not in body
    assert capi.Params._fields_[-1][0] == "keyframe_retire" and not [f for f, _ in capi.Params._fields_ if "merge" in f]
    src = '#include <stdio.h>\n#include "%s"\nint main() { printf("%%zu", sizeof(vslam_params)); return 0; }\n' % os.path.join(ROOT, "include", "vslam_c.h")
    c = tmp_path / "size.c"
    c.write_text(src)
    subprocess.check_call(["gcc", str(c), "-o", str(tmp_path / "size")])
    assert int(subprocess.check_output([str(tmp_path / "size")])) == ctypes.sizeof(capi.Params)


def test_the_cxx_mirror_gains_nothing():
    """include/vslam/ptam.h mirrors one stream per MapMaker: a merge of two streams has no place in it"""
    assert "vslam_merge_maps" not in open(os.path.join(ROOT, "include", "vslam", "ptam.h")).read()
