"""The overlay's raster rules (csrc/overlay_dev.h) and what is drawn for a stream (include/vslam_c.h, vslam_render_overlay), restated
in numpy.  The device renders through a rank plane; here the primitives are painted one after the other in drawing order, so the two share
the rules and nothing of their construction.  No GPU is touched by the raster functions; primitives_from_readbacks reads a System."""
import numpy as np

from visualslam_android_amd import capi

LEVEL_COLOURS = ((255, 0, 0), (255, 255, 0), (0, 255, 0), (0, 0, 178))      # gavLevelColors * 255; 178.5 rounds half to even
TRAIL_COLOUR = (255, 0, 0)
MARK_COLOUR = (255, 0, 255)
PALETTE = tuple(sorted(set(LEVEL_COLOURS + (TRAIL_COLOUR, MARK_COLOUR))))


def line_pixels(xa, ya, xb, yb):
    """-> (n, 2) x, y of the 8-connected line, from the endpoint with the smaller x (the first given on a tie): pixel i = 0 .. a lies i
    steps along the major axis and (2 b i + a - 1) // (2 a) steps along the minor one"""
    if xb < xa:
        xa, ya, xb, yb = xb, yb, xa, ya
    dx, dy = xb - xa, yb - ya
    a, b = max(dx, abs(dy)), min(dx, abs(dy))
    i = np.arange(a + 1, dtype=np.int64)
    m = (2 * b * i + a - 1) // (2 * a) if a else np.zeros(1, np.int64)
    sy = -1 if dy < 0 else 1
    if abs(dy) > dx:
        return np.stack([xa + m, ya + sy * i], 1)
    return np.stack([xa + i, ya + sy * m], 1)


_DISC = np.array([(dx, dy) for dy in range(-2, 3) for dx in range(-2, 3) if dx * dx + dy * dy <= 6], np.int64)
_MARK = np.array([(-1, 0), (1, 0), (0, -1), (0, 1)], np.int64)


def disc_pixels(x, y):
    """the 21 pixels with dx^2 + dy^2 <= 6"""
    return _DISC + np.array([x, y], np.int64)


def mark_pixels(x, y):
    """the four neighbours, not the centre"""
    return _MARK + np.array([x, y], np.int64)


def _paint(img, pix, rgba):
    h, w = img.shape[:2]
    ok = (pix[:, 0] >= 0) & (pix[:, 0] < w) & (pix[:, 1] >= 0) & (pix[:, 1] < h)
    img[pix[ok, 1], pix[ok, 0]] = rgba


def render(w, h, base, marks, lines, discs, flags=0):
    """-> uint8 (h, w, 4).  base: the gray image (h, w), or with DRAW_IN_PLACE the RGBA image (h, w, 4) drawn on.  marks (n, 2), lines
    (n, 4), discs (n, 3: x, y, level) in list order.  Lowest first: marks, lines, discs in reverse list order."""
    if flags & capi.DRAW_IN_PLACE:
        img = np.array(base, np.uint8).reshape(h, w, 4).copy()
    else:
        g = np.asarray(base, np.uint8).reshape(h, w)
        img = np.stack([g, g, g, np.full_like(g, 255)], 2)
    alpha = 0 if flags & capi.DRAW_ALPHA0 else 255
    for x, y in np.asarray(marks, np.int64).reshape(-1, 2):
        _paint(img, mark_pixels(x, y), MARK_COLOUR + (alpha,))
    for xa, ya, xb, yb in np.asarray(lines, np.int64).reshape(-1, 4):
        _paint(img, line_pixels(int(xa), int(ya), int(xb), int(yb)), TRAIL_COLOUR + (alpha,))
    for x, y, level in np.asarray(discs, np.int64).reshape(-1, 3)[::-1]:
        _paint(img, disc_pixels(x, y), LEVEL_COLOURS[int(level)] + (alpha,))
    return img


def discs_from_tracks(order, tracks):
    """the entries of `order` (map-point indices) whose point is found -> (n, 3) x, y, level; the centre is v2Image truncated"""
    order = np.asarray(order, np.int64)
    f = order[tracks["found"][order] == 1]
    xy = np.trunc(tracks["image"][f]).astype(np.int64)
    return np.concatenate([xy.reshape(-1, 2), tracks["level"][f].astype(np.int64).reshape(-1, 1)], 1)


def primitives_from_readbacks(sys, stream, flags):
    """-> (marks, lines, discs) of what vslam_render_overlay draws for the stream now, from the existing read-backs and overlay_info"""
    marks, lines, discs = np.zeros((0, 2), np.int64), np.zeros((0, 4), np.int64), np.zeros((0, 3), np.int64)
    if flags & capi.DRAW_FAST:
        c = sys.read_corners(stream, 0)
        marks = np.stack([c & 0xFFFF, c >> 16], 1).astype(np.int64)
    if flags & capi.DRAW_TRAILS and sys.params.bootstrap and sys.init_info(stream)["stage"] == 1:
        lines = sys.trails(stream).astype(np.int64)
    if flags & capi.DRAW_POINTS:
        ran = sys.overlay_info(stream)["track_map_frame"]
        if ran >= 0 and ran == sys.state(stream).frame:
            order, _counts = sys.search_plan(stream)
            discs = discs_from_tracks(order, sys.point_tracks(stream))
    return marks, lines, discs


def render_stream(sys, stream, flags, base=None):
    """the reference image of one stream; base: the RGBA image drawn on, with DRAW_IN_PLACE"""
    w, h = sys.params.width, sys.params.height
    marks, lines, discs = primitives_from_readbacks(sys, stream, flags)
    img = render(w, h, base if flags & capi.DRAW_IN_PLACE else sys.read_level_image(stream, 0), marks, lines, discs, flags)
    return img, (len(discs), len(lines), len(marks))
