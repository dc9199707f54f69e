"""CPU test: keyframe retirement is declared, exported and bound alike; keyframe_retire is off by default; bad arguments are refused
before anything needs a device."""
import ctypes
import os
import re
import subprocess

from visualslam_android_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vslam_retire_keyframes", "vslam_get_retire_info", "vslam_get_retire_timing")
E_INVALID = -1


def test_header_library_and_binding_agree_on_the_retire_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vslam_c.h")).read(), flags=re.S)
    lib = ctypes.CDLL(capi.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(\s*vslam_system\s*\*" % name, text), name
        assert hasattr(lib, name), "libvslam_hip.so does not export %s" % name
        assert name in capi.SYMBOLS
    assert re.search(r"vslam_retire_keyframes\s*\(\s*vslam_system\s*\*\s*sys\s*,\s*const\s+int\s*\*\s*streams\s*,\s*const\s+int\s*\*\s*keyframes\s*,\s*int\s+n\s*\)", text)
    assert re.search(r"vslam_get_retire_info\s*\(\s*vslam_system\s*\*\s*sys\s*,\s*int\s+stream\s*,\s*int\s+out\[6\]\s*\)", text)
    assert re.search(r"vslam_get_retire_timing\s*\(\s*vslam_system\s*\*\s*sys\s*,\s*double\s*\*\s*ms\s*\)", text)
    assert len(capi.SYMBOLS["vslam_retire_keyframes"][1]) == 4 and len(capi.SYMBOLS["vslam_get_retire_info"][1]) == 3
    assert callable(capi.System.retire_keyframes) and callable(capi.System.retire_info) and callable(capi.System.retire_timing)


def test_keyframe_retire_is_the_last_field_and_off_by_default():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vslam_c.h")).read(), flags=re.S)
    body = text[text.index("typedef struct vslam_params"):text.index("} vslam_params;")]
    assert re.search(r"int\s+keyframe_retire\s*;\s*$", body)
    assert capi.Params._fields_[-1][0] == "keyframe_retire"
    p = capi.default_params(640, 480, 3)
    assert p.keyframe_retire == 0 and (p.max_keyframes, p.max_points) == (32, 4096)
    # the C struct and the ctypes mirror agree on the size, so the new field is where the library reads it
    src = '#include <stdio.h>\n#include "%s"\nint main() { printf("%%zu", sizeof(vslam_params)); return 0; }\n' % os.path.join(ROOT, "include", "vslam_c.h")
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "size.c")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", c, "-o", os.path.join(d, "size")])
        assert int(subprocess.check_output([os.path.join(d, "size")])) == ctypes.sizeof(capi.Params)


def test_bad_arguments_are_refused_without_a_system():
    lib = capi.load_library()
    one = (ctypes.c_int * 1)(0)
    out = (ctypes.c_int * 6)()
    ms = ctypes.c_double(0.0)
    assert lib.vslam_retire_keyframes(None, one, one, 1) == E_INVALID
    assert lib.vslam_retire_keyframes(None, one, one, -1) == E_INVALID
    assert lib.vslam_retire_keyframes(None, None, None, 0) == E_INVALID
    assert lib.vslam_get_retire_info(None, 0, out) == E_INVALID
    assert lib.vslam_get_retire_timing(None, ctypes.byref(ms)) == E_INVALID
    assert b"retire" in lib.vslam_last_error()


def test_the_cxx_mirror_reaches_the_retirement(tmp_path):
    """include/vslam/ptam.h: MapMaker::RetireKeyFrame calls vslam_retire_keyframes, and the Tracker's constructor sets keyframe_retire"""
    hdr = os.path.join(ROOT, "include", "vslam", "ptam.h")
    tu = tmp_path / "mirror.cpp"
    tu.write_text('#include "%s"\nvoid f(MapMaker& m) { m.RetireKeyFrame(); m.RetireKeyFrame(2); }\n' % hdr)
    obj = str(tmp_path / "mirror.o")
    subprocess.check_call(["g++", "-std=c++17", "-c", str(tu), "-o", obj])
    assert "vslam_retire_keyframes" in subprocess.check_output(["nm", "-u", obj], text=True)
    assert re.search(r"p\.keyframe_retire\s*=", open(hdr).read())


def test_create_refuses_keyframe_retire_on_a_map_of_two():
    """a map keeps at least two keyframes, so a system of max_keyframes = 2 could never retire: refused before any device is touched"""
    import pytest
    with pytest.raises(capi.VslamError, match="keyframe_retire"):
        capi.System(capi.default_params(640, 480, 1, keyframe_retire=1, max_keyframes=2))
