"""CPU: vslam_snapshot_info, the host-only validator of a stream snapshot (csrc/snapshot_format.h).  It needs no GPU and no system:
a well-formed blob head is described, and an empty buffer, a wrong magic, a wrong version, a header cut one byte short and a total size
that disagrees with the number of bytes are refused with VSLAM_E_INVALID.  The header here is written by hand from the layout the
format header documents, so the test also pins that layout (a change of it is a new SNAP_VERSION)."""
import struct

import numpy as np
import pytest

from visualslam_android_amd import capi

E_INVALID = -1
N_SECTIONS = 26
HEADER_BYTES = 8 + 4 + 4 + 8 + 16 + 40 + 16 + 16 + 16 * N_SECTIONS
MAGIC = b"VSLMSNAP"
CAM = (0.841906, 1.10893, 0.505171, 0.470265, -0.0133843)


def align16(x):
    return (x + 15) & ~15


def section_sizes(w, h, n_kf, n_pts, n_iter):
    """bytes of every section of a blob without optional parts, in order (snapshot_format.h: SnapSection)"""
    img = [n_kf * (w >> l) * (h >> l) for l in range(4)]
    return [624, n_pts * 24, n_pts * 80, n_pts * 168, n_pts * 128, n_pts * 4, n_pts * 4, n_pts * 24, n_kf * n_pts * 24, n_kf * 96, n_kf * 4,
            n_kf * 16] + img + [n_iter * 4] + [0] * 9


def make_header(w=640, h=480, n_kf=3, n_pts=65, n_iter=40, patch=11, quirks=0, frame=12, map_good=1, magic=MAGIC, version=1, total=None):
    sizes = section_sizes(w, h, n_kf, n_pts, n_iter)
    assert len(sizes) == N_SECTIONS
    off, table = HEADER_BYTES, []
    for b in sizes:
        table.append((off, b))
        off = align16(off + b)
    total_true = off
    head = struct.pack("<8sIIQ4i5d4i2i2I", magic, version, HEADER_BYTES, total_true if total is None else total, w, h, patch, quirks, *CAM,
                       n_kf, n_pts, frame, map_good, n_iter, 0, 0, 0)
    head += b"".join(struct.pack("<QQ", o, b) for o, b in table)
    assert len(head) == HEADER_BYTES and HEADER_BYTES % 16 == 0
    return head, total_true, table


def info(head, nbytes):
    """vslam_snapshot_info on `head`, told that the blob is nbytes long (it reads no more than a header)"""
    a = np.frombuffer(head, np.uint8)
    out = capi.SnapshotInfo()
    rc = capi.load_library().vslam_snapshot_info(a.ctypes.data if len(a) else None, nbytes, out)
    return rc, out


def test_a_well_formed_header_is_described():
    head, total, table = make_header()
    rc, o = info(head, total)
    assert rc == 0, capi.load_library().vslam_last_error()
    assert (o.version, o.width, o.height, o.patch_size, o.quirks) == (1, 640, 480, 11, 0) and tuple(o.cam) == CAM
    assert (o.n_keyframes, o.n_points, o.frame, o.map_good) == (3, 65, 12, 1)
    assert (o.has_idle_state, o.has_sbi, o.has_reloc_state) == (0, 0, 0) and o.total_bytes == total
    assert o.point_pos_offset == table[1][0] and o.keyframe_pose_offset == table[9][0]
    for l in range(4):
        assert o.image_offset[l] == table[12 + l][0] and o.image_row_stride[l] == 640 >> l and o.image_stride[l] == (640 >> l) * (480 >> l)
    assert capi.snapshot_info(head + bytes(total - len(head))).n_points == 65          # the Python wrapper, on a whole (zero-filled) blob


def test_an_empty_buffer_is_refused():
    assert info(b"", 0)[0] == E_INVALID
    with pytest.raises(capi.VslamError):
        capi.snapshot_info(b"")


def test_a_wrong_magic_is_refused():
    head, total, _ = make_header(magic=b"VSLMSNAQ")
    assert info(head, total)[0] == E_INVALID
    assert b"magic" in capi.load_library().vslam_last_error()


def test_a_wrong_version_is_refused():
    for v in (0, 2, 0xFFFFFFFF):
        head, total, _ = make_header(version=v)
        assert info(head, total)[0] == E_INVALID, v


def test_a_header_cut_one_byte_short_is_refused():
    head, total, _ = make_header()
    assert info(head[:-1], len(head) - 1)[0] == E_INVALID


def test_a_total_size_that_disagrees_with_the_bytes_is_refused():
    head, total, _ = make_header()
    for n in (total - 1, total + 1, total + 16, len(head)):
        assert info(head, n)[0] == E_INVALID, n
    head, total, _ = make_header(total=10 ** 9)                                            # the field itself disagrees with the counts
    assert info(head, total)[0] == E_INVALID and info(head, 10 ** 9)[0] == E_INVALID
