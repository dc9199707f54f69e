"""CPU test: the similarity transform is declared, exported and bound alike; the refusals that need no device; the C++ mirror reaches it."""
import ctypes
import os
import re
import subprocess

import numpy as np

from visualslam_android_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vslam_transform_maps", "vslam_get_transform_info", "vslam_get_transform_timing")
E_INVALID = -1


def test_header_library_and_binding_agree_on_the_transform_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vslam_c.h")).read(), flags=re.S)
    lib = ctypes.CDLL(capi.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(\s*vslam_system\s*\*" % name, text), name
        assert hasattr(lib, name), "libvslam_hip.so does not export %s" % name
        assert name in capi.SYMBOLS
    assert re.search(r"vslam_transform_maps\s*\(\s*vslam_system\s*\*\s*sys\s*,\s*const\s+int\s*\*\s*streams\s*,\s*int\s+n\s*,\s*const\s+double\s*\*\s*new_from_old12\s*,\s*const\s+double\s*\*\s*scale\s*\)", text)
    assert re.search(r"vslam_get_transform_info\s*\(\s*vslam_system\s*\*\s*sys\s*,\s*int\s+stream\s*,\s*int\s+out_i\[2\]\s*,\s*double\s+out_d\[13\]\s*\)", text)
    assert re.search(r"vslam_get_transform_timing\s*\(\s*vslam_system\s*\*\s*sys\s*,\s*double\s*\*\s*ms\s*\)", text)
    assert re.search(r"vslam_fit_similarity\s*\(\s*int\s+n\s*,\s*const\s+double\s*\*\s*from3\s*,\s*const\s+double\s*\*\s*to3\s*,\s*const\s+double\s*\*\s*weights\s*,\s*int\s+fix_scale\s*,", text)
    assert hasattr(lib, "vslam_fit_similarity") and len(capi.SYMBOLS["vslam_fit_similarity"][1]) == 8
    assert len(capi.SYMBOLS["vslam_transform_maps"][1]) == 5 and len(capi.SYMBOLS["vslam_get_transform_info"][1]) == 4
    assert callable(capi.System.transform_maps) and callable(capi.System.transform_info) and callable(capi.System.transform_timing) and callable(capi.fit_similarity)


def test_bad_arguments_are_refused_without_a_system():
    lib = capi.load_library()
    one = (ctypes.c_int * 1)(0)
    T = np.r_[np.eye(3).reshape(-1), np.zeros(3)]
    oi, od = (ctypes.c_int * 2)(), (ctypes.c_double * 13)()
    ms = ctypes.c_double(0.0)
    assert lib.vslam_transform_maps(None, one, 1, T.ctypes.data, None) == E_INVALID
    assert lib.vslam_transform_maps(None, None, 0, None, None) == E_INVALID
    assert lib.vslam_get_transform_info(None, 0, oi, od) == E_INVALID
    assert lib.vslam_get_transform_timing(None, ctypes.byref(ms)) == E_INVALID
    assert b"transform" in lib.vslam_last_error()


def test_the_cxx_mirror_reaches_the_transform(tmp_path):
    """include/vslam/ptam.h: MapMaker::ApplyGlobalTransformationToMap(mySE3) and ApplyGlobalScaleToMap(double) are public and call
    vslam_transform_maps"""
    hdr = os.path.join(ROOT, "include", "vslam", "ptam.h")
    tu = tmp_path / "mirror.cpp"
    tu.write_text('#include "%s"\nvoid f(MapMaker& m, mySE3 T) { m.ApplyGlobalTransformationToMap(T); m.ApplyGlobalScaleToMap(2.0); }\n' % hdr)
    obj = str(tmp_path / "mirror.o")
    subprocess.check_call(["g++", "-std=c++17", "-c", str(tu), "-o", obj])
    assert "vslam_transform_maps" in subprocess.check_output(["nm", "-u", obj], text=True)
