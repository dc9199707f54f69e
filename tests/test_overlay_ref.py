"""CPU: the raster rules of the overlay as tests/overlay_ref.py restates them, and the scene of the GPU tracking case seen through the
oracle, so that tests/test_gpu_overlay.py cannot pass on a scene that draws nothing worth checking."""
import functools

import numpy as np

import overlay_ref as ov
import tracker_cases as tc
from helpers import make_oracle
from visualslam_android_amd import capi


def iterator_pixels(xa, ya, xb, yb):
    """the error recurrence of OpenCV's 8-connected LineIterator with left_to_right, pixel by pixel"""
    dx, dy = xb - xa, yb - ya
    if dx < 0:
        xa, ya, dx, dy = xb, yb, -dx, -dy
    sy = -1 if dy < 0 else 1
    dy = abs(dy)
    ymajor = dy > dx
    a, b = (dy, dx) if ymajor else (dx, dy)
    err, plus, minus = a - 2 * b, 2 * a, -2 * b
    x, y, out = xa, ya, []
    for _ in range(a + 1):
        out.append((x, y))
        step = err < 0
        err += minus + (plus if step else 0)
        if ymajor:
            y += sy; x += 1 if step else 0
        else:
            x += 1; y += sy if step else 0
    return np.array(out, np.int64)


def test_closed_form_line_is_the_iterator_in_all_octants():
    for dx in range(-40, 41):
        for dy in range(-40, 41):
            got, want = ov.line_pixels(5, -3, 5 + dx, -3 + dy), iterator_pixels(5, -3, 5 + dx, -3 + dy)
            assert np.array_equal(got, want), (dx, dy)


def test_line_ends_on_its_end_point_and_is_symmetric():
    rng = np.random.default_rng(1)
    for xa, ya, xb, yb in rng.integers(-50, 200, size=(300, 4)):
        p = ov.line_pixels(xa, ya, xb, yb)
        ends = {tuple(p[0]), tuple(p[-1])}
        assert ends == {(xa, ya), (xb, yb)}, (xa, ya, xb, yb)
        assert tuple(p[0]) == ((xa, ya) if xa <= xb else (xb, yb))
        q = ov.line_pixels(xb, yb, xa, ya)
        assert set(map(tuple, p)) == set(map(tuple, q)), (xa, ya, xb, yb)
        assert len(p) == max(abs(xb - xa), abs(yb - ya)) + 1
        assert np.abs(np.diff(p, axis=0)).max(initial=0) <= 1                    # 8-connected


def test_degenerate_line_is_one_pixel():
    assert ov.line_pixels(7, 9, 7, 9).tolist() == [[7, 9]]


def test_disc_and_mark_shapes():
    d = ov.disc_pixels(10, 20)
    assert len(d) == 21 and len(set(map(tuple, d))) == 21
    assert all((x - 10) ** 2 + (y - 20) ** 2 <= 6 for x, y in d) and (12, 21) in set(map(tuple, d)) and (12, 22) not in set(map(tuple, d))
    assert sorted(map(tuple, ov.mark_pixels(3, 4))) == [(2, 4), (3, 3), (3, 5), (4, 4)]


def test_disc_is_clipped_in_all_four_corners():
    w, h = 9, 7
    g = np.zeros((h, w), np.uint8)
    for (x, y), n in (((0, 0), 8), ((w - 1, 0), 8), ((0, h - 1), 8), ((w - 1, h - 1), 8), ((w, h), 3), ((-3, 2), 0), ((w + 1, 1), 3), ((4, 3), 21)):
        img = ov.render(w, h, g, [], [], [(x, y, 2)])
        drawn = (img[..., :3] == ov.LEVEL_COLOURS[2]).all(-1)
        want = {(px, py) for px, py in ov.disc_pixels(x, y).tolist() if 0 <= px < w and 0 <= py < h}
        assert drawn.sum() == len(want) == n, ((x, y), drawn.sum(), len(want), n)
        assert {(px, py) for py, px in np.argwhere(drawn).tolist()} == want, (x, y)


def test_drawing_order():
    w, h = 24, 16
    g = np.full((h, w), 50, np.uint8)
    # a later line is over an earlier one: same colour, so tell them apart in place over a marker image through ALPHA0 and 255
    a = ov.render(w, h, g, [(8, 8)], [(0, 8, 23, 8)], [(8, 8, 1), (9, 8, 2)])
    assert tuple(a[8, 8]) == ov.LEVEL_COLOURS[1] + (255,)                    # the first disc of the list is on top
    assert tuple(a[8, 11]) == ov.LEVEL_COLOURS[2] + (255,)                   # ... where only the second reaches
    assert tuple(a[8, 20]) == ov.TRAIL_COLOUR + (255,) and tuple(a[8, 0]) == ov.TRAIL_COLOUR + (255,)
    b = ov.render(w, h, g, [(15, 8), (15, 3)], [(0, 8, 23, 8)], [])
    assert tuple(b[8, 14]) == ov.TRAIL_COLOUR + (255,) and tuple(b[7, 15]) == ov.MARK_COLOUR + (255,)     # lines over marks
    assert tuple(b[3, 15]) == (50, 50, 50, 255)                              # a mark's centre is not drawn
    c = ov.render(w, h, g, [(9, 8)], [], [(11, 8, 3)])
    assert tuple(c[8, 10]) == ov.LEVEL_COLOURS[3] + (255,) and tuple(c[8, 8]) == ov.MARK_COLOUR + (255,)   # discs over marks
    # two crossing lines: the pixel they share belongs to the later one -- painted with different alphas to tell them apart
    first = ov.render(w, h, g, [], [(0, 0, 14, 14)], [], capi.DRAW_ALPHA0)
    both = ov.render(w, h, first, [], [(0, 14, 14, 0)], [], capi.DRAW_IN_PLACE)
    shared = set(map(tuple, ov.line_pixels(0, 0, 14, 14))) & set(map(tuple, ov.line_pixels(0, 14, 14, 0)))
    assert shared and all(both[y, x, 3] == 255 for x, y in shared) and both[0, 0, 3] == 0


def test_in_place_leaves_every_undrawn_byte_alone_and_alpha0():
    w, h = 31, 17
    rng = np.random.default_rng(2)
    base = rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8)
    marks, lines, discs = [(4, 4), (30, 16)], [(2, 1, 28, 15)], [(15, 8, 0), (0, 0, 3)]
    out = ov.render(w, h, base, marks, lines, discs, capi.DRAW_IN_PLACE | capi.DRAW_ALPHA0)
    full = ov.render(w, h, np.zeros((h, w), np.uint8), marks, lines, discs, capi.DRAW_ALPHA0)
    drawn = full[..., 3] == 0                                               # the base of a full render has alpha 255
    assert drawn.sum() > 40
    assert np.array_equal(out[~drawn], base[~drawn]) and np.array_equal(out[drawn], full[drawn])
    assert set(map(tuple, out[drawn][:, :3])) <= set(ov.PALETTE) and (out[drawn][:, 3] == 0).all()
    assert (ov.render(w, h, base, marks, lines, discs, capi.DRAW_IN_PLACE)[drawn][:, 3] == 255).all()


TRACK_SCENE = tc.A_SCENE                     # the scene of test_gpu_overlay.py's tracking case (stream 0)
TRACK_PKW = tc.NO_KF


@functools.lru_cache(maxsize=None)
def oracle_discs():
    f, m, frames = tc.scene(*TRACK_SCENE)
    w, h = TRACK_SCENE[:2]
    o = make_oracle(capi.default_params(w, h, 1, **dict(TRACK_PKW)), m, f.pose(-1))
    o.track_frame(frames[0])
    tr = o.point_tracks()
    o.close()
    return ov.discs_from_tracks(np.flatnonzero(tr["level"] >= 0), tr)


def test_the_tracking_scene_draws_three_levels_and_overlapping_discs_of_different_colour():
    d = oracle_discs()
    assert len(set(d[:, 2].tolist())) >= 3, np.bincount(d[:, 2], minlength=4)
    covered = {}
    for x, y, level in d:
        for p in map(tuple, ov.disc_pixels(x, y)):
            covered.setdefault(p, set()).add(int(level))
    assert any(len(v) > 1 for v in covered.values()), "no two discs of different colour overlap"
