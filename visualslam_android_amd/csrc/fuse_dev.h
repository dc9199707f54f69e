// Point fusion (vslam_fuse_points, fuse.hip): the rule by which two map points of one stream are one surface feature, stated once for
// gfx950 and for the host, like merge_dev.h and similarity_dev.h.  The kernels, the library's host code and the host-side check
// (tests/fuse_rules_check.cpp, built with sanitizers) include this one header; tests/fuse_ref.py restates it in numpy and does not
// read it.
//
// One stream, nk keyframes, np points, the caller's radius (level pixels) and min_views.  A point is live if !bad; cell (k, i) is
// kf_meas[k][i], valid if its valid byte is non-zero.  For live q < p and keyframe k:
//   shared(k)     both cells valid
//   agree(k)      shared(k), equal level bytes, and d2 <= lim2 with dx = root_p[0] - root_q[0], dy = root_p[1] - root_q[1],
//                 d2 = dx*dx + dy*dy, lim = radius * (double)(1 << level), lim2 = lim*lim -- in that order, no contraction (the
//                 library is built with -ffp-contract=off).  A NaN compares false: no agreement.  A level byte outside 0..FUSE_MAX_LEVEL
//                 names no pyramid level and cannot be shifted by: no agreement either                                  (fuse_relation)
//   conflict(k)   shared(k) and not agree(k)
//   dup(p, q)     agreements over k < nk >= min_views and no conflict                                                        (fuse_dup)
//   partner(p)    the lowest live q < p with dup(p, q), else -1
//   p is dropped into q = partner(p) iff q >= 0 and partner(q) < 0: one level per call, a chain's tail waits for the next (fuse_dropped)
// A kept q, keyframe k < nk: a valid cell stays; an empty cell whose keyframe is in q's never-retry set stays empty
// (fuse_never_retry_bit); an empty cell otherwise takes the 24 bytes of cell (k, p) of the lowest p dropped into q whose cell (k, p) is
// valid, with SRC_ROOT turned into SRC_REFIND (fuse_source): a point has one root, its own.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define FUSE_FN __host__ __device__ inline
#else
#define FUSE_FN inline
#endif

#define FUSE_MAX_LEVEL 30        // 1 << level is an int
#define FUSE_SET_BITS 128        // keyframes a never-retry set can name (= BA_MAX_KF)
#define FUSE_SRC_ROOT 2          // MeasDev::source of the measurement a point was made from (mapgrow.hip, boot.hip; read at ba.hip, k_ba_writeback)
#define FUSE_SRC_REFIND 1        // ... of one that ReFind_Common added (mapgrow.hip)

enum FuseRelation : int { FUSE_NONE = 0, FUSE_AGREE = 1, FUSE_CONFLICT = 2 };

// lim2 of a level byte that names a level
FUSE_FN double fuse_lim2(double radius, int level) {
  const double lim = radius * (double)(1 << level);
  return lim * lim;
}
FUSE_FN bool fuse_level_ok(int level) { return level >= 0 && level <= FUSE_MAX_LEVEL; }
// d2 <= lim2, false for a NaN on either side
FUSE_FN bool fuse_within(double px, double py, double qx, double qy, double lim2) {
  const double dx = px - qx, dy = py - qy;
  const double d2 = dx * dx + dy * dy;
  return d2 <= lim2;
}
// cells (k, p) and (k, q) of one keyframe
FUSE_FN int fuse_relation(int valid_p, int level_p, double px, double py, int valid_q, int level_q, double qx, double qy, double radius) {
  if (!valid_p || !valid_q) return FUSE_NONE;
  if (level_p != level_q || !fuse_level_ok(level_p)) return FUSE_CONFLICT;
  return fuse_within(px, py, qx, qy, fuse_lim2(radius, level_p)) ? FUSE_AGREE : FUSE_CONFLICT;
}
FUSE_FN bool fuse_dup(int n_agree, int n_conflict, int min_views) { return n_agree >= min_views && n_conflict == 0; }
// partner_p = partner(p), partner_of_partner = partner(partner(p)) where partner_p >= 0 (not read otherwise)
FUSE_FN bool fuse_dropped(int partner_p, int partner_of_partner) { return partner_p >= 0 && partner_of_partner < 0; }
// bit k of the 128-bit set (w0 low word, w1 high word); no shift by a count outside 0..63
FUSE_FN bool fuse_never_retry_bit(uint64_t w0, uint64_t w1, int k) {
  if (k < 0 || k >= FUSE_SET_BITS) return false;
  return k < 64 ? ((w0 >> k) & 1ull) != 0 : ((w1 >> (k - 64)) & 1ull) != 0;
}
// an empty cell (k, q) of a kept point takes a valid cell of a point dropped into it
FUSE_FN bool fuse_takes(int valid_q, bool never_retry_k) { return !valid_q && !never_retry_k; }
// the source byte of a cell taken
FUSE_FN int fuse_source(int source) { return source == FUSE_SRC_ROOT ? FUSE_SRC_REFIND : source; }
