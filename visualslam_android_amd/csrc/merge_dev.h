// Map merge (vslam_merge_maps, merge.hip): the index rules of appending the map of a source stream s (nk_s keyframes, np_s points)
// to the map of a destination stream d (nk_d, np_d), stated once for gfx950 and for the host, like similarity_dev.h and pvs_perm.h.
// The kernel, the library's host code and the host-side check (tests/merge_rules_check.cpp, built with sanitizers) include this one
// header; tests/merge_ref.py restates it in numpy and does not read it.
//
//   keyframe k of s        becomes keyframe nk_d + k of d        (merge_keyframe)
//   point p of s           becomes point np_d + p of d           (merge_point)
//   pt_flags               keep TDF_TMPL_BAD | TDF_HAVE_LAST: the template cache comes along, the per-frame bits (IN_IMAGE, FOUND,
//                          SEARCHED, SUBPIX) belong to s's last frame and d's read-backs must not show them            (merge_flags)
//   never-retry set        s's 128-bit set over its keyframes, masked to its low nk_s bits (nothing above the count comes along),
//                          then shifted up by nk_d across the two words.  Every count from 0 to 128 is legal on both sides: a shift
//                          by 64 or more of a 64-bit word is undefined in C++, so no shift below is by a count outside 1..63
//                                                                                                                (merge_never_retry)
//   failure queue          entry j of s's stored entries (k, p) lands as (nk_d + k, np_d + p) at position stored_d + j while that is
//                          below the queue's capacity; the count becomes stored_d + stored_s and may pass the capacity, as
//                          k_ba_writeback lets it (the readers clamp)                                    (merge_queue_entry, _slot)
//   measurement (k, p)     of s lands in d's table at row nk_d + k, column np_d + p; the row stride is max_points       (merge_meas_cell)
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define MERGE_FN __host__ __device__ inline
#else
#define MERGE_FN inline
#endif

#define MERGE_KEEP_FLAGS (16 | 32)   // TDF_TMPL_BAD | TDF_HAVE_LAST (merge.hip asserts it against vslam_internal.h)
#define MERGE_SET_BITS 128           // keyframes a never-retry set can name (= BA_MAX_KF)

MERGE_FN int merge_keyframe(int k, int nk_d) { return nk_d + k; }
MERGE_FN int merge_point(int p, int np_d) { return np_d + p; }
MERGE_FN int merge_flags(int flags_s) { return flags_s & MERGE_KEEP_FLAGS; }

// the low n bits of a 64-bit word, n in 0..64
MERGE_FN uint64_t merge_low_bits(int n) { return n <= 0 ? 0ull : (n >= 64 ? ~0ull : ((1ull << n) - 1ull)); }

// (w0 low word, w1 high word) of s -> the set d holds for the appended point
MERGE_FN void merge_never_retry(uint64_t w0, uint64_t w1, int nk_s, int nk_d, uint64_t* o0, uint64_t* o1) {
  w0 &= merge_low_bits(nk_s);
  w1 &= merge_low_bits(nk_s - 64);
  if (nk_d <= 0) { *o0 = w0; *o1 = w1; }
  else if (nk_d < 64) { *o0 = w0 << nk_d; *o1 = (w1 << nk_d) | (w0 >> (64 - nk_d)); }
  else if (nk_d == 64) { *o0 = 0ull; *o1 = w0; }
  else if (nk_d < MERGE_SET_BITS) { *o0 = 0ull; *o1 = w0 << (nk_d - 64); }
  else { *o0 = 0ull; *o1 = 0ull; }
}

MERGE_FN void merge_queue_entry(int k, int p, int nk_d, int np_d, int* ok, int* op) { *ok = merge_keyframe(k, nk_d); *op = merge_point(p, np_d); }
// where entry j of s's stored entries lands in d's queue, -1: past the capacity, not stored (it is still counted)
MERGE_FN int merge_queue_slot(int stored_d, int j, int fq_cap) { const long q = (long)stored_d + j; return q < fq_cap ? (int)q : -1; }
// entries of a queue whose counter says fq_n (it may count past the capacity)
MERGE_FN int merge_queue_stored(int fq_n, int fq_cap) { return fq_n < 0 ? 0 : (fq_n < fq_cap ? fq_n : fq_cap); }

// cell index of s's measurement (k, p) in d's table [max_keyframes][max_points]
MERGE_FN size_t merge_meas_cell(int k, int p, int nk_d, int np_d, int max_points) {
  return (size_t)merge_keyframe(k, nk_d) * (size_t)max_points + (size_t)merge_point(p, np_d);
}
