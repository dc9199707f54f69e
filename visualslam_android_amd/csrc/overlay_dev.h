// The overlay's raster rules, stated once: what Tracker::TrackFrame draws on its colour frame (jni/Tracker.cc:580-588 the found patches
// as discs, :322-336 the bootstrap trails as lines, :148-155 drawFast's corner marks).  The reference draws with cv::circle and
// cv::line, which are third-party arithmetic the project neither vendors nor can run (like cv::resize): the rules
// below are this build's own definitions, parity unpinned.  Integer only; the render kernel (overlay.hip), the library's host code and
// host-side checks include this one header.  tests/overlay_ref.py restates it in numpy.
//
// Pixel format: 4 bytes R, G, B, A in memory order (CV_8UC4); cv::Scalar(v0, v1, v2) writes v0 to byte 0.  A drawn pixel's alpha is
// 255, or 0 with VSLAM_DRAW_ALPHA0 (what cv::Scalar's unset fourth value writes).
// Clipping: a pixel outside the image is skipped; nothing is clipped beforehand, so a line's phase does not depend on the border.
// Order, lowest first: marks in corner-list order, lines in trail-list order, discs in REVERSE list order (:581 iterates the set
// backwards, so its first entry ends on top); a later primitive overwrites an earlier one.  ov_rank() turns that order into one
// number per primitive, 0 = the base image, so that "the largest rank wins" is the order whatever order the pixels are produced in.
//
// Two differences from the reference in what is drawn for a stream: a trail that died in this frame has left the list, so its
// one-frame (0, 255, 255) line (:333) is not drawn; and on the frame that starts the trails each trail is a single pixel, where the
// reference draws nothing.
#pragma once
#include <stdint.h>

#ifndef HDFN
#if defined(__HIPCC__) || defined(__CUDACC__)
#define HDFN __host__ __device__ __forceinline__
#else
#define HDFN inline
#endif
#endif

#define OV_COORD_MAX 32767   // a primitive with a coordinate beyond +-OV_COORD_MAX is not drawn (an image is at most 4096 wide)

// ---- colours ------------------------------------------------------------------------------------------------------------------
// Level colours gavLevelColors * 255 (jni/KeyFrame.cc:122-125): level 3 is 0.7 * 255 = 178.5, which saturate_cast rounds half to even.
enum OvClass : int { OV_LEVEL0 = 0, OV_LEVEL1 = 1, OV_LEVEL2 = 2, OV_LEVEL3 = 3, OV_TRAIL = 4, OV_MARK = 5 };
// the pixel as a little-endian dword: byte 0 = R
HDFN uint32_t ov_colour(int cls, bool alpha0) {
  const uint32_t rgb = cls == OV_LEVEL0 ? 0x0000FFu      // (255,   0,   0)
                     : cls == OV_LEVEL1 ? 0x00FFFFu      // (255, 255,   0)
                     : cls == OV_LEVEL2 ? 0x00FF00u      // (  0, 255,   0)
                     : cls == OV_LEVEL3 ? 0xB20000u      // (  0,   0, 178)
                     : cls == OV_TRAIL  ? 0x0000FFu      // (255,   0,   0)  jni/Tracker.cc:330
                     :                    0xFF00FFu;     // (255,   0, 255)  jni/Tracker.cc:153
  return alpha0 ? rgb : rgb | 0xFF000000u;
}
HDFN uint32_t ov_gray(uint32_t g) { return g * 0x010101u | 0xFF000000u; }   // the base: R = G = B = gray, A = 255

// ---- rank ---------------------------------------------------------------------------------------------------------------------
// marks 1 .. nm, lines nm + 1 .. nm + nl, disc j of nd (list order) nm + nl + nd - j: unique per primitive
HDFN uint32_t ov_rank_mark(int i) { return 1u + (uint32_t)i; }
HDFN uint32_t ov_rank_line(int nm, int i) { return 1u + (uint32_t)nm + (uint32_t)i; }
HDFN uint32_t ov_rank_disc(int nm, int nl, int nd, int j) { return (uint32_t)nm + (uint32_t)nl + (uint32_t)(nd - j); }
// ... and back: 0 a mark, 1 a line, 2 a disc, *idx its list position
HDFN int ov_rank_kind(uint32_t rank, int nm, int nl, int nd, int* idx) {
  if (rank <= (uint32_t)nm) { *idx = (int)rank - 1; return 0; }
  if (rank <= (uint32_t)nm + (uint32_t)nl) { *idx = (int)(rank - 1u - (uint32_t)nm); return 1; }
  *idx = nd - (int)(rank - (uint32_t)nm - (uint32_t)nl); return 2;
}

HDFN bool ov_coord_ok(int v) { return v >= -OV_COORD_MAX && v <= OV_COORD_MAX; }

// ---- disc: cv::circle(centre, 1, colour, 3), the 21 pixels with dx^2 + dy^2 <= 6 -------------------------------------------------
#define OV_DISC_R 2
#define OV_DISC_PIXELS 21
HDFN bool ov_disc_covers(int dx, int dy) { return dx * dx + dy * dy <= 6; }
// row dy of the disc spans dx = -h .. h
HDFN int ov_disc_half_width(int dy) { return (dy == 2 || dy == -2) ? 1 : 2; }

// ---- mark: cv::circle(centre, 1, colour, 1), OpenCV's midpoint circle at radius 1: the four neighbours, not the centre -------------
#define OV_MARK_PIXELS 4
HDFN void ov_mark_pixel(int k, int* dx, int* dy) { *dx = k == 0 ? -1 : k == 1 ? 1 : 0; *dy = k == 2 ? -1 : k == 3 ? 1 : 0; }

// ---- line: thickness 1, 8-connected, the form of OpenCV's LineIterator with left_to_right ------------------------------------------
// It starts at the endpoint with the smaller x (the first given on a tie).  a = max(|dx|, |dy|), b = the smaller; the major axis is y
// only if |dy| > |dx|.  Pixel i = 0 .. a lies i steps along the major axis and (2 b i + a - 1) / (2 a) steps (0 when a = 0) along the
// minor axis, towards the end point: the iterator's error recurrence in closed form, so any pixel is had without carried state.
struct OvLine { int x0, y0, a, b, sy, ymajor; };   // sy: the direction of y from the start (+1 / -1); x never decreases
HDFN OvLine ov_line_setup(int xa, int ya, int xb, int yb) {
  if (xb < xa) { int t = xa; xa = xb; xb = t; t = ya; ya = yb; yb = t; }
  const int dx = xb - xa, dy = yb - ya, ady = dy < 0 ? -dy : dy;
  OvLine L;
  L.x0 = xa; L.y0 = ya; L.sy = dy < 0 ? -1 : 1; L.ymajor = ady > dx ? 1 : 0;
  L.a = L.ymajor ? ady : dx; L.b = L.ymajor ? dx : ady;
  return L;
}
HDFN int ov_line_minor(const OvLine& L, int i) { return L.a ? (int)((2ll * L.b * i + L.a - 1) / (2ll * L.a)) : 0; }
HDFN void ov_line_pixel(const OvLine& L, int i, int* x, int* y) {
  const int m = ov_line_minor(L, i);
  if (L.ymajor) { *x = L.x0 + m; *y = L.y0 + L.sy * i; }
  else { *x = L.x0 + i; *y = L.y0 + L.sy * m; }
}
