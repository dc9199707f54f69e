"""GPU: the overlay renderer (csrc/overlay.hip) against tests/overlay_ref.py, byte for byte throughout.

The hook (vslam_eval_overlay) runs the render kernel over given primitives at the sizes where its paths split: 48x48 and 128x56 (every
output row 16-byte aligned), 50x49 and 157x101 (rows that start 4, 8 or 12 bytes past a 16-byte boundary: single pixels at head and
tail; gray rows that are not dword aligned), 4096x48 (the widest image: 4 rows per band, the whole 64 KB key plane), in place with a row
stride of 4 W + 3 (rows of every alignment modulo 4: the byte stores).  More than one band everywhere (16 rows per band up to 1024 wide).
vslam_render_overlay is held to the reference built from the existing read-backs on tracked, lost, unmapped, reset, retired, held and
bootstrapping streams."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import overlay_ref as ov
import tracker_cases as tc
import trail_cases as trc
from visualslam_android_amd import capi, feeder

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_STATE = -1, -4
POINTS, TRAILS, FAST, IN_PLACE, ALPHA0 = capi.DRAW_POINTS, capi.DRAW_TRAILS, capi.DRAW_FAST, capi.DRAW_IN_PLACE, capi.DRAW_ALPHA0
ALL = POINTS | TRAILS | FAST
HOOK_SIZES = ((48, 48), (50, 49), (157, 101), (128, 56), (4096, 48))
HOOK_SETS = ("structured", "random, no disc", "random, 1 disc", "random, 1000 discs")


def structured(w, h):
    """a disc centred on every row, centres at x = w and y = h included; lines across the whole image in all octants and along the axes
    and diagonals, both ways round, so that every band edge is crossed; marks on the borders"""
    discs = [(7 * y % w, y, y % 4) for y in range(h + 1)] + [(w, y, 1) for y in range(0, h + 1, 5)] + [(x, h, 2) for x in range(0, w + 1, 9)]
    cx, cy, m = w // 2, h // 2, min(w, h) - 1
    lines = [(0, 0, w - 1, h - 1), (w - 1, h - 1, 0, 0), (0, h - 1, w - 1, 0), (w - 1, 0, 0, h - 1),
             (cx, 0, cx, h - 1), (cx + 1, h - 1, cx + 1, 0), (0, cy, w - 1, cy), (w - 1, cy + 1, 0, cy + 1),
             (0, 0, m, m), (m, 0, 0, m), (w - 1, h - 1, w - 1 - m, h - 1 - m), (-5, -7, w + 4, h + 9), (w + 3, -2, -4, h + 1)]
    for ex, ey in ((w - 1, cy - h // 4), (w - 1, cy + h // 4), (0, cy - h // 4), (0, cy + h // 4),
                   (cx - m // 4, 0), (cx + m // 4, 0), (cx - m // 4, h - 1), (cx + m // 4, h - 1), (cx + 3, 0), (cx - 3, h - 1)):
        lines += [(cx, cy, ex, ey)]
    marks = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w, 5), (-1, 7), (9, -1), (11, h), (cx, cy), (cx + 1, cy)]
    return marks, lines, discs


def random_set(w, h, n_discs, seed):
    rng = np.random.default_rng(seed)
    def xy(n):
        return np.stack([rng.integers(-8, w + 8, size=n), rng.integers(-8, h + 8, size=n)], 1)
    marks = xy(5000)
    lines = np.concatenate([xy(1000), xy(1000)], 1)
    discs = np.concatenate([xy(n_discs), rng.integers(0, 4, size=(n_discs, 1))], 1)
    return marks, lines, discs


@pytest.mark.parametrize("which", HOOK_SETS)
@pytest.mark.parametrize("size", HOOK_SIZES, ids=lambda s: "%dx%d" % s)
def test_hook_equals_the_reference(size, which):
    w, h = size
    k = HOOK_SETS.index(which)
    marks, lines, discs = structured(w, h) if k == 0 else random_set(w, h, (0, 1, 1000)[k - 1], seed=100 * k + w)
    rng = np.random.default_rng(7 + w + h)
    gray = rng.integers(0, 256, size=(h, w), dtype=np.uint8)
    for flags in (0, ALPHA0):
        got = capi.eval_overlay(gray, marks, lines, discs, flags)
        want = ov.render(w, h, gray, marks, lines, discs, flags)
        assert np.array_equal(got, want), (size, which, flags, int((got != want).any(-1).sum()))
    # in place over random bytes, rows 4 w + 3 bytes apart: the bytes between the rows and every undrawn pixel stay
    stride = 4 * w + 3
    buf = rng.integers(0, 256, size=stride * (h - 1) + 4 * w, dtype=np.uint8)
    rows = np.stack([buf[y * stride:y * stride + 4 * w] for y in range(h)]).reshape(h, w, 4)
    want = buf.copy()
    ref = ov.render(w, h, rows, marks, lines, discs, IN_PLACE)
    for y in range(h):
        want[y * stride:y * stride + 4 * w] = ref[y].reshape(-1)
    got = capi.eval_overlay(gray, marks, lines, discs, IN_PLACE, rgba=buf, row_stride=stride)
    assert np.array_equal(got, want), (size, which, "in place", int((got != want).sum()))
    assert k == 1 or (ref != rows).any()


def test_hook_with_nothing_to_draw_is_the_gray_base():
    gray = np.random.default_rng(3).integers(0, 256, size=(49, 50), dtype=np.uint8)
    got = capi.eval_overlay(gray)
    assert np.array_equal(got[..., 0], gray) and np.array_equal(got[..., 1], gray) and np.array_equal(got[..., 2], gray) and (got[..., 3] == 255).all()


# ---- vslam_render_overlay -------------------------------------------------------------------------------------------------------------
W, H = tc.W, tc.H
SCENES = (tc.A_SCENE, tc.C_SCENE)


def tracking_system(n_frames=2, **kw):
    """two streams on the scenes of tracker_cases, n_frames tracked -> (system, per stream the frames)"""
    pkw = dict(tc.NO_KF, overlay=1)
    pkw.update(kw)
    g = capi.System(capi.default_params(W, H, len(SCENES), **pkw))
    frames = []
    for s, key in enumerate(SCENES):
        f, m, fr = tc.scene(*key)
        g.load_map(s, m); g.set_pose(s, f.pose(-1))
        frames.append(fr)
    for t in range(n_frames):
        g.track_frame(np.stack([fr[t] for fr in frames]))
    return g, frames


def render_rc(g, streams, out, row_stride, stream_stride, on_device, flags, n=None):
    a = None if streams is None else np.ascontiguousarray(streams, np.int32)
    ptr = out if isinstance(out, int) or out is None else out.ctypes.data
    return g.lib.vslam_render_overlay(g.h, None if a is None else a.ctypes.data, len(a) if n is None and a is not None else (n or 0), ptr, row_stride, stream_stride,
                                      int(on_device), int(flags))


def check_stream_images(g, streams, flags, tag):
    """host output of the listed streams == the reference from read-backs, and the counts of overlay_info -> the counts per stream"""
    got = g.render_overlay(streams, flags)
    counts = []
    for i, s in enumerate(range(g.S) if streams is None else streams):
        want, n = ov.render_stream(g, s, flags)
        assert np.array_equal(got[i], want), (tag, s, int((got[i] != want).any(-1).sum()))
        info = g.overlay_info(s)
        assert (info["discs"], info["lines"], info["marks"]) == n, (tag, s, info, n)
        counts.append(n)
    return counts


def test_tracking_device_and_host_output():
    g, _frames = tracking_system(2)
    flags = ALL
    want = [ov.render_stream(g, s, flags) for s in range(2)]
    assert all(n[0] > 50 and n[2] > 100 for _img, n in want), [n for _img, n in want]
    levels = set(ov.primitives_from_readbacks(g, 0, flags)[2][:, 2].tolist())
    assert len(levels) >= 3, levels
    # device memory, rows 16 bytes and images 4096 + 64 bytes further apart than they need to be: the padding stays
    row_stride, stream_stride = 4 * W + 16, (4 * W + 16) * H + 4160
    dev = torch.full((2 * stream_stride,), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    g.render_overlay_device(None, dev.data_ptr(), row_stride, stream_stride, flags)
    g.synchronize()
    assert g.render_timing() > 0.0
    out = dev.cpu().numpy()
    mask = np.zeros(out.size, bool)
    for s in range(2):
        rows = np.stack([out[s * stream_stride + y * row_stride:s * stream_stride + y * row_stride + 4 * W] for y in range(H)]).reshape(H, W, 4)
        assert np.array_equal(rows, want[s][0]), ("device", s, int((rows != want[s][0]).any(-1).sum()))
        for y in range(H):
            mask[s * stream_stride + y * row_stride:s * stream_stride + y * row_stride + 4 * W] = True
    assert (out[~mask] == 0x5A).all()
    for s in range(2):
        info = g.overlay_info(s)
        assert (info["discs"], info["lines"], info["marks"]) == want[s][1] and info["track_map_frame"] == g.state(s).frame == 2
    # host memory, every stream and a list in another order; in place over a pattern; points alone
    check_stream_images(g, None, flags, "host")
    check_stream_images(g, [1, 0], POINTS, "host, listed")
    base = np.random.default_rng(5).integers(0, 256, size=(1, H, W, 4), dtype=np.uint8)
    got = g.render_overlay([1], POINTS | IN_PLACE | ALPHA0, rgba=base)
    want1, _n = ov.render_stream(g, 1, POINTS | IN_PLACE | ALPHA0, base=base[0])
    assert np.array_equal(got[0], want1) and (got[0] != base[0]).any()
    g.close()


def test_arguments_and_states():
    g, frames = tracking_system(1)
    buf = np.full((2, H, W, 4), 7, np.uint8)
    ok = dict(row_stride=4 * W, stream_stride=4 * W * H, on_device=0, flags=POINTS)
    assert g.lib.vslam_render_overlay(None, None, 0, buf.ctypes.data, 4 * W, 4 * W * H, 0, POINTS) == E_INVALID
    assert render_rc(g, [0, 1], buf, n=-1, **ok) == E_INVALID and render_rc(g, [0, 1, 0], buf, **ok) == E_INVALID      # n < 0, n > n_streams
    assert render_rc(g, [0, 2], buf, **ok) == E_INVALID and render_rc(g, [-1], buf, **ok) == E_INVALID                  # outside the batch
    assert render_rc(g, [1, 1], buf, **ok) == E_INVALID                                                                  # a duplicate
    assert render_rc(g, [0], None, **ok) == E_INVALID and render_rc(g, None, None, **ok) == E_INVALID                    # NULL rgba
    assert render_rc(g, [0], buf, **dict(ok, row_stride=4 * W - 1)) == E_INVALID
    assert render_rc(g, [0, 1], buf, **dict(ok, stream_stride=4 * W * H - 1)) == E_INVALID
    assert render_rc(g, [0], buf, **dict(ok, stream_stride=0)) == 0                                                      # one image: the stride is not read
    buf[:] = 7
    assert render_rc(g, [0], buf, **dict(ok, flags=32)) == E_INVALID and render_rc(g, [0], buf, **dict(ok, flags=POINTS | 64)) == E_INVALID
    assert render_rc(g, [], buf, n=0, **ok) == 0
    # a stage-wise frame: refused until vslam_pose_update(sys, 1) has been enqueued, then what the read-backs give
    g.make_keyframe_lite(np.stack([fr[1] for fr in frames]))
    g.patch_search(0)
    assert render_rc(g, None, buf, **ok) == E_STATE
    g.pose_update(0); g.patch_search(1)
    assert render_rc(g, None, buf, **ok) == E_STATE
    assert (buf == 7).all(), "a refused call writes nothing"
    g.pose_update(1)
    n = check_stream_images(g, None, ALL, "open frame")
    assert all(c[0] > 50 for c in n)
    g.finish_frame()
    assert check_stream_images(g, None, ALL, "closed frame") == n
    g.close()


def test_streams_without_discs():
    """a mapped stream, the stream without a map and a stream that loses tracking (tracker_cases.LOSS_IDLE): once TrackMap no longer
    runs the record goes stale, the discs stop and the base is intact"""
    batch = tc.loss_batch(11)
    pick = [6, 7, 8]
    assert [tc.LOSS_IDLE.get(s) for s in pick] == [None, "no map", "lost"]
    cases = [batch[s] for s in pick]
    vp = cases[0].params(len(cases), 11)
    vp.overlay = 1
    g = capi.System(vp)
    for s, c in enumerate(cases):
        if c is not None:
            c.load(g, s)
    blank = np.zeros((H, W), np.uint8)
    stale_by = []
    for t in range(tc.LOSS_FRAMES):
        g.track_frame(np.stack([blank if c is None else c.frame(t) for c in cases]))
        n = check_stream_images(g, None, POINTS | TRAILS, "frame %d" % t)
        ran = [g.overlay_info(s)["track_map_frame"] for s in range(3)]
        assert ran[0] == t + 1 and n[0][0] > 30
        assert ran[1] == -1 and n[1] == (0, 0, 0)
        st = g.state(2)
        if st.lost_frames == 3 and ran[2] != st.frame:
            stale_by.append(st.frame - ran[2])
            assert n[2] == (0, 0, 0)
            img = g.render_overlay([2], POINTS | TRAILS)[0]
            assert (img[..., :3] == blank[..., None]).all() and (img[..., 3] == 255).all()
    assert stale_by and stale_by[0] == 1, stale_by
    g.close()


@pytest.mark.parametrize("size", ((96, 64), (157, 101)), ids=lambda s: "%dx%d" % s)
def test_trails(size):
    """the crops of trail_cases: the frame that starts the trails (single pixels) and two advances"""
    cases = trc.group(size)
    g = capi.System(cases[0].params(len(cases), bootstrap=1, overlay=1))
    drew = 0
    for t in range(3):
        for s, c in enumerate(cases):
            if t in c.presses:
                g.press_spacebar(s)
        g.track_frame(np.stack([c.frames[t] for c in cases]))
        n = check_stream_images(g, None, ALL, "%dx%d frame %d" % (size + (t,)))
        for s, c in enumerate(cases):
            want = len(g.trails(s)) if g.init_info(s)["stage"] == 1 else 0
            assert n[s][1] == want and n[s][0] == 0
        drew += n[0][1]
        assert n[0][1] > 10, n[0]
    no_trails = g.render_overlay([0], POINTS | FAST)
    assert np.array_equal(no_trails[0], ov.render_stream(g, 0, POINTS | FAST)[0]) and g.overlay_info(0)["lines"] == 0
    g.close()


def test_lines_stop_and_discs_begin_after_the_second_spacebar():
    w, h = 640, 480
    f = feeder.Feeder(w, h, seed=1234, noise=2)
    frames = f.render(0, 15)
    g = capi.System(capi.default_params(w, h, 1, grow_map=3, bootstrap=1, overlay=1))
    seen = {}
    for t in range(15):
        if t in (0, 12):
            g.press_spacebar(0)
        g.track_frame(frames[t][None])
        if t in (0, 11, 12, 13, 14):
            seen[t] = check_stream_images(g, [0], POINTS | TRAILS, "frame %d" % t)[0]
    assert g.init_info(0)["map_good"] == 1
    assert seen[0][1] > 100 and seen[0][0] == 0 and seen[11][1] > 50 and seen[11][0] == 0
    assert seen[12][:2] == (0, 0)                      # the frame InitFromStereo ran in: no trails any more, TrackMap has not run yet
    assert seen[13][0] > 50 and seen[13][1] == 0 and seen[14][0] > 50
    g.close()


def test_subset_step_held_stream_is_refused():
    g, frames = tracking_system(2)
    g.track_frame_subset([1], frames[1][2][None])
    buf = np.full((2, H, W, 4), 9, np.uint8)
    ok = dict(row_stride=4 * W, stream_stride=4 * W * H, on_device=0, flags=ALL)
    assert render_rc(g, [0], buf, **ok) == E_STATE and render_rc(g, None, buf, **ok) == E_STATE and render_rc(g, [1, 0], buf, **ok) == E_STATE
    assert (buf == 9).all()
    n = check_stream_images(g, [1], ALL, "the stream of the step")
    assert n[0][0] > 50 and g.overlay_info(1)["track_map_frame"] == 3 and g.overlay_info(0)["track_map_frame"] == 2
    g.track_frame(np.stack([frames[0][2], frames[1][3]]))
    check_stream_images(g, None, ALL, "the next full step")
    g.close()


def test_reset_retire_and_overlay_off():
    g, frames = tracking_system(2)
    assert check_stream_images(g, None, POINTS, "before")[0][0] > 50
    g.retire_keyframes([1])
    g.reset([0])
    n = check_stream_images(g, None, POINTS, "after reset and retire")
    assert n[0][0] == 0 and n[1][0] == 0
    assert g.overlay_info(0)["track_map_frame"] == -1 and g.overlay_info(1)["track_map_frame"] == -1
    g.track_frame(np.stack([frames[0][2], frames[1][2]]))
    n = check_stream_images(g, None, POINTS, "the frame after")
    assert n[0][0] == 0 and n[1][0] > 50                # the reset stream has no map; the other one tracks on with one keyframe fewer
    g.close()
    # overlay = 0: no renderer, and the same bits in every other read-back
    kw = dict(min_frames_between_kf=2, ba_sum_order=1)
    on, _ = tracking_system(0, **kw)
    off, _ = tracking_system(0, **dict(kw, overlay=0))
    for t in range(5):
        for x in (on, off):
            x.track_frame(np.stack([fr[t] for fr in frames]))
        on.render_overlay(None, ALL)
        a, b = (b"".join(bytes(st) for st in x.states()) for x in (on, off))
        assert a == b, t
        for s in range(2):
            ta, tb = on.point_tracks(s), off.point_tracks(s)
            assert all(np.array_equal(ta[k], tb[k]) for k in ta), (t, s)
            assert np.array_equal(on.search_plan(s)[0], off.search_plan(s)[0])
    buf = np.zeros((2, H, W, 4), np.uint8)
    assert render_rc(off, None, buf, 4 * W, 4 * W * H, 0, POINTS) == E_STATE and not buf.any()
    o4 = np.zeros(4, np.int32)
    assert off.lib.vslam_get_overlay_info(off.h, 0, o4.ctypes.data) == E_STATE
    ms = C.c_double(0)
    assert off.lib.vslam_get_render_timing(off.h, C.byref(ms)) == E_STATE
    on.close(); off.close()


def test_drop_in_example_draws_on_its_colour_frame(tmp_path):
    exe = os.path.join(ROOT, "examples", "_build", "system_ptam")
    assert os.path.exists(exe), "examples/_build/system_ptam not built (run __graft_entry__.build())"
    path = str(tmp_path / "rgb.raw")
    out = subprocess.run([exe, "20", "draw", path], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    img = np.fromfile(path, np.uint8).reshape(480, 640, 4)
    drawn = img.any(-1)
    assert drawn.sum() > 21 * 20
    colours = set(map(tuple, img[drawn].tolist()))
    assert colours <= {c + (255,) for c in ov.PALETTE}, colours
    assert len(colours & {c + (255,) for c in ov.LEVEL_COLOURS}) >= 2, colours
