// PatchFinder (jni/PatchFinder.cc) and the MapPoint pieces around it, stated once for every kernel that needs them: the tracker
// (k_pvs, k_searchN, k_subpixN in track.hip), the map maker (k_epipolar, ReFind_Common in mapgrow.hip) and the stereo bootstrap
// (k_boot_points in boot.hip).  What each lane computes per pixel or per candidate is here; how pixels and candidates are dealt
// to lanes stays with the kernels.  Nothing may be contracted into FMAs, and every expression keeps the reference's association.
#pragma once
#include "vslam_internal.h"

// ---- packed rows: row r of a PS x PS patch as dwords, unused bytes zero (operands of v_dot4_u32_u8) ------------------------------
template <int PS> struct PRow { unsigned w[(PS + 3) / 4]; };
template <int PS> DEVFN PRow<PS> zero_row() {
  PRow<PS> r;
#pragma unroll
  for (int k = 0; k < (PS + 3) / 4; k++) r.w[k] = 0u;
  return r;
}
template <int PS> DEVFN PRow<PS> load_row(const uint8_t* p) {
  PRow<PS> r = zero_row<PS>();
  __builtin_memcpy(&r, p, PS);
  return r;
}
template <int PS> DEVFN PRow<PS> load_row_lds(const uint8_t* p) {         // a row out of LDS (byte reads: 8-byte rows of an 11-byte pitch are unaligned)
  PRow<PS> r = zero_row<PS>();
#pragma unroll
  for (int x = 0; x < PS; x++) r.w[x >> 2] |= (unsigned)p[x] << (8 * (x & 3));
  return r;
}
template <int PS> DEVFN int row_byte(const PRow<PS>& r, int x) { return (int)((r.w[x >> 2] >> (8 * (x & 3))) & 255u); }
DEVFN unsigned udot4(unsigned a, unsigned b, unsigned c) { return __builtin_amdgcn_udot4(a, b, c, false); }

// ---- PatchFinder::ZMSSDAtPoint, jni/PatchFinder.cc:352-380 -----------------------------------------------------------------------
// the score from the template's sums (MakeTemplateSums :152-164) and the image patch's sum, sum of squares and cross sum
template <int NPIX> DEVFN int zmssd_score(int tsum, int tsumsq, int sA, int sQ, int sX) {
  const int SA = tsum, SB = sA;
  return ((2 * SA * SB - SA * SA - SB * SB) / NPIX + sQ + tsumsq - 2 * sX);
}
// G lanes per patch (8 for 8x8 -> 8 patches per wavefront, 16 for 11x11 -> 4): lane r < PS holds row r of the image patch and of the
// template (the other lanes zero rows); the three sums are dot products reduced over the group
template <int PS, int G> DEVFN void grp_zmssd_sums(const PRow<PS>& row, const PRow<PS>& trow, int& sA, int& sQ, int& sX) {
  unsigned a = 0, q = 0, x = 0;
#pragma unroll
  for (int k = 0; k < (PS + 3) / 4; k++) {
    a = udot4(row.w[k], 0x01010101u, a);
    q = udot4(row.w[k], row.w[k], q);
    x = udot4(row.w[k], trow.w[k], x);
  }
  sA = (int)grp_sum<G>(a); sQ = (int)grp_sum<G>(q); sX = (int)grp_sum<G>(x);
}
// one patch per wavefront, one pixel per lane and step; the template lies in LDS
template <int PS>
DEVFN int wave_zmssd(const uint8_t* tmpl, const uint8_t* img, int ip, int wl, int hl, int cx, int cy, int tsum, int tsumsq, int max_ssd, int lane) {
  constexpr int NPIX = PS * PS, HALF = PS / 2;
  if (!(cx >= HALF && cy >= HALF && cx < wl - HALF && cy < hl - HALF)) return max_ssd + 1;
  int sA = 0, sQ = 0, sX = 0;
  for (int q = lane; q < NPIX; q += 64) {
    const int y = q / PS, x = q - y * PS;
    const int n = img[(size_t)(cy - HALF + y) * ip + (cx - HALF + x)], t = tmpl[q];
    sA += n; sQ += n * n; sX += n * t;
  }
  sA = wave_sum(sA); sQ = wave_sum(sQ); sX = wave_sum(sX);
  return zmssd_score<NPIX>(tsum, tsumsq, sA, sQ, sX);
}

// ---- PatchFinder::CalcSearchLevelAndWarpMatrix, jni/PatchFinder.cc:31-68 ---------------------------------------------------------
// cam = the point in the camera frame, derivs = m2CamDerivs there, right / down = the point's pixel vectors in the world.  Fills
// warp_inv (mm2WarpInverse, row-major) and search_level (mnSearchLevel, which MakeTemplateCoarseCont reads whatever the verdict);
// returns the level, or -1 for a bad scale (mbTemplateBad = true, :62-65).
DEVFN int search_level_and_warp(const Pose& pose, const double cam[3], const double d[4], const double right[3], const double down[3],
                                double warp_inv[4], int& search_level) {
  const double ooz = 1.0 / cam[2];
  double mr[3], md[3];
  pose_rot(pose, right, mr);
  pose_rot(pose, down, md);
  const double r0 = mr[0] - cam[0] * mr[2] * ooz, r1 = mr[1] - cam[1] * mr[2] * ooz;
  const double d0 = md[0] - cam[0] * md[2] * ooz, d1 = md[1] - cam[1] * md[2] * ooz;
  warp_inv[0] = (d[0] * r0 + d[1] * r1) * ooz; warp_inv[2] = (d[2] * r0 + d[3] * r1) * ooz;
  warp_inv[1] = (d[0] * d0 + d[1] * d1) * ooz; warp_inv[3] = (d[2] * d0 + d[3] * d1) * ooz;
  double det = warp_inv[0] * warp_inv[3] - warp_inv[1] * warp_inv[2];
  int lv = 0;
  while (det > 3 && lv < NLEV - 1) { lv++; det *= 0.25; }
  search_level = lv;
  return (det > 3 || det < 0.25) ? -1 : lv;
}

// ---- PatchFinder::MakeTemplateCoarseCont, jni/PatchFinder.cc:79-125 --------------------------------------------------------------
DEVFN void template_warp_matrix(const double warp_inv[4], int scale, double m2[4]) {   // m2 = mm2WarpInverse.inverse() * LevelScale, :83-84
  double inv[4];
  inv2(warp_inv, inv);
  m2[0] = inv[0] * scale; m2[1] = inv[1] * scale; m2[2] = inv[2] * scale; m2[3] = inv[3] * scale;
}
// :88-92: a column of the warp moved by more than 0.07 since the template was last made
DEVFN bool warp_moved(const double m2[4], const double last_warp[4]) {
  for (int i = 0; i < 2; i++) {
    const double dx = m2[i] - last_warp[i], dy = m2[2 + i] - last_warp[2 + i];
    if (dx * dx + dy * dy > 0.07 * 0.07) return true;
  }
  return false;
}
// transform_image (jni/vision/ImageHandler.cpp:21-113) walks ONE accumulated sample position over the template: a step `across`
// per pixel, the carriage return `cr` after the PS steps of a row.  A lane reaches its pixel by making exactly those additions.
struct TemplateWarp {
  double across[2], down[2], cr[2], x0, y0;   // x0, y0: the sample position of template pixel (0, 0)
  float x_bound, y_bound;                     // sample() reads (x .. x + 1, y .. y + 1) of a iw x ih source image
};
template <int PS> DEVFN TemplateWarp template_warp(const double m2[4], int irx, int iry, int iw, int ih) {
  constexpr int HALF = PS / 2;
  TemplateWarp w;
  w.across[0] = m2[0]; w.across[1] = m2[2]; w.down[0] = m2[1]; w.down[1] = m2[3];
  w.x0 = (double)irx - (m2[0] * HALF + m2[1] * HALF); w.y0 = (double)iry - (m2[2] * HALF + m2[3] * HALF);
  w.cr[0] = w.down[0] - PS * w.across[0]; w.cr[1] = w.down[1] - PS * w.across[1];
  w.x_bound = (float)(iw - 1); w.y_bound = (float)(ih - 1);
  return w;
}
DEVFN void warp_pixel_step(const TemplateWarp& w, double& x, double& y) { x += w.across[0]; y += w.across[1]; }
template <int PS> DEVFN void warp_row_step(const TemplateWarp& w, double& x, double& y) {   // a whole row and its carriage return
#pragma unroll
  for (int j = 0; j < PS; j++) warp_pixel_step(w, x, y);
  x += w.cr[0]; y += w.cr[1];
}
// sample(), ImageHandler.cpp:12-19: truncated bilinear read; a position outside the source gives 0 and counts
DEVFN int warp_sample(const TemplateWarp& w, const uint8_t* src, int sp, double x, double y, int& nOutside) {
  if (0 <= x && 0 <= y && x < w.x_bound && y < w.y_bound) {
    const int lx = (int)x, ly = (int)y;
    x -= lx; y -= ly;
    const uint8_t* q0 = src + (size_t)ly * sp + lx;
    return (uint8_t)((1 - y) * ((1 - x) * q0[0] + x * q0[1]) + y * ((1 - x) * q0[sp] + x * q0[sp + 1]));
  }
  nOutside++;
  return 0;
}

// ---- PatchFinder::FindPatchCoarse, jni/PatchFinder.cc:170-235: the search window around (irx, iry) at the search level ------------
struct CoarseWindow {
  unsigned range;                              // nRange
  int top, bottom_plus_one, left, right;       // rows [top, bottom_plus_one) of the corner list, columns [left, right]
  bool empty;                                  // no row of the level's `rows` lies in the window (:189-192)
};
DEVFN CoarseWindow coarse_window(double irx, double iry, int range_l0, int scale, int rows) {
  CoarseWindow cw;
  cw.range = ((unsigned)range_l0 + scale - 1) / scale;
  cw.top = (int)(iry - cw.range);
  cw.bottom_plus_one = (int)(iry + cw.range + 1);
  cw.left = (int)(irx - cw.range); cw.right = (int)(irx + cw.range);
  if (cw.top < 0) cw.top = 0;
  cw.empty = cw.top >= rows || cw.bottom_plus_one <= 0;
  return cw;
}

// ---- PatchFinder::MakeTemplateCoarseNoWarp (jni/PatchFinder.cc:130-142) + MakeTemplateSums by one wavefront ----------------------
// copies the PS x PS patch around (cx, cy) into tmpl; false (nothing written) when the patch does not keep the border
template <int PS>
DEVFN bool template_no_warp(const uint8_t* img, int pitch, int w, int h, int cx, int cy, uint8_t* tmpl, int lane, int& sum, int& sumsq) {
  constexpr int NPIX = PS * PS, HALF = PS / 2, bord = HALF + 1;
  if (!(cx >= bord && cy >= bord && cx < w - bord && cy < h - bord)) return false;
  int sa = 0, sq = 0;
  for (int q = lane; q < NPIX; q += 64) {
    const int y = q / PS, x = q - y * PS;
    const int v = img[(size_t)(cy - HALF + y) * pitch + (cx - HALF + x)];
    tmpl[q] = (uint8_t)v; sa += v; sq += v * v;
  }
  sum = wave_sum(sa); sumsq = wave_sum(sq);
  return true;
}

// ---- MapPoint::RefreshPixelVectors, jni/MapPoint.cc:4-29, in the source keyframe's frame (patch normal (0, 0, -1)) ----------------
// cen, rgt, dwn: unit rays through the patch centre and its neighbours; depth: the point's z in that frame
DEVFN void refresh_pixel_vectors(const double cen[3], const double rgt[3], const double dwn[3], double depth, double right_out[3], double down_out[3]) {
  const double hgt = fabs(-depth), rc = fabs(-cen[2]), rr = fabs(-rgt[2]), rd = fabs(-dwn[2]);
  for (int i = 0; i < 3; i++) { const double cop = cen[i] * hgt / rc; right_out[i] = rgt[i] * hgt / rr - cop; down_out[i] = dwn[i] * hgt / rd - cop; }
}

// ---- a new map point --------------------------------------------------------------------------------------------------------------
HDFN TrackData fresh_track_data() {
  TrackData td = {};
  td.last_warp[0] = 9999.9; td.last_warp[3] = 9999.9;   // jni/PatchFinder.cc:23
  return td;
}
// mMap.vpPoints.push_back: everything of point `pid` of stream s except its measurements and the stream's point count
DEVFN void append_point(const MapDev& m, const TrackParams& tp, int s, int pid, const MapPointDev& mp) {
  const size_t gi = (size_t)s * tp.max_points + pid;
  m.pts[gi] = mp;
  m.td[gi] = fresh_track_data();
  m.pt_level[gi] = -1; m.pt_flags[gi] = 0;
  m.cur_meas[gi].valid = 0;
}
