// The quick reject of the FAST-10 strip kernel (k_fast_slide, frontend.hip), stated once and computed two pixels per instruction.
//
// Predicate (cvfast.cpp:6088-9241 as a filter): ten contiguous ring pixels contain two ADJACENT compass pixels (0, 4, 8, 12), so a
// corner has such a pair both above c + t or both below c - t:
//     max(min(max(p0, p8), max(p4, p12)) - c,  c - max(min(p0, p8), min(p4, p12)))  >  t
// p0 / p8 are the pixels 3 rows below / above the centre c, p4 / p12 the pixels 3 to the right / left.
//
// Packed form: a dword of four pixels is unpacked into two registers of two 16-bit lanes each, pixels (0, 2) and pixels (1, 3), one
// v_perm_b32 with zero-filling selectors per register; the predicate's ten operations (v_pk_max_u16, v_pk_min_u16, v_pk_sub_i16,
// v_pk_max_i16) then serve two pixels each.  Pixel values are 0..255 and t is below 256, so every intermediate lies in
// [-255, 510] and fits a signed 16-bit lane: no lane ever carries into its neighbour.  The answer of a lane is the SIGN of t - v.
//
// Static cost in k_fast_slide (rows unpacked where they are used, the centre row's unpacked dwords shared by its neighbours), per
// lane and row of 16 pixels: 34 v_perm_b32 + 80 packed operations + 20 to gather the sign bits (8 v_lshrrev, 8 v_and, 4 v_or3) + 2 to
// order them = 136 instructions, 8.5 per pixel (the 32-bit form with byte selects it replaces: 11.5; profiles/r09_frontend_isa.txt).
// fast_reject4() alone, with nothing shared: 10 v_perm_b32 + 20 packed + 7 = 37 per four pixels.
//
// Integer only; the strip kernel and host-side checks (tests/fast_reject_check.cpp) include this one header.  Outside device
// compilation the packed lanes are a plain struct and v_perm_b32 a byte loop.
#pragma once
#include <stdint.h>

#ifndef HDFN
#if defined(__HIPCC__) || defined(__CUDACC__)
#define HDFN __host__ __device__ __forceinline__
#else
#define HDFN inline
#endif
#endif

// v_perm_b32 selectors (byte k of the result <- selector byte k: 0..3 a byte of the low operand, 4..7 of the high one, 0x0c zero)
#define FR_SEL_EVEN 0x0c020c00u    // pixels 0, 2 of the low operand
#define FR_SEL_ODD 0x0c030c01u     // pixels 1, 3 of the low operand
#define FR_SEL_L3_ODD 0x0c040c02u  // (lo = the dword to the left, hi = centre dword): the pixels 3 to the left of pixels 1, 3
#define FR_SEL_R3_EVEN 0x0c050c03u // (lo = centre dword, hi = the dword to the right): the pixels 3 to the right of pixels 0, 2

#if defined(__HIP_DEVICE_COMPILE__)
typedef unsigned short fr_u2 __attribute__((ext_vector_type(2)));
typedef short fr_i2 __attribute__((ext_vector_type(2)));
HDFN unsigned fr_perm(unsigned hi, unsigned lo, unsigned sel) { return __builtin_amdgcn_perm(hi, lo, sel); }
HDFN fr_u2 fr_lanes(unsigned w) { return __builtin_bit_cast(fr_u2, w); }
HDFN fr_u2 fr_maxu(fr_u2 a, fr_u2 b) { return __builtin_elementwise_max(a, b); }
HDFN fr_u2 fr_minu(fr_u2 a, fr_u2 b) { return __builtin_elementwise_min(a, b); }
HDFN fr_i2 fr_subi(fr_u2 a, fr_u2 b) { return __builtin_bit_cast(fr_i2, a) - __builtin_bit_cast(fr_i2, b); }
HDFN fr_i2 fr_maxi(fr_i2 a, fr_i2 b) { return __builtin_elementwise_max(a, b); }
HDFN unsigned fr_signs(fr_u2 t, fr_i2 v) { return __builtin_bit_cast(unsigned, __builtin_bit_cast(fr_i2, t) - v); }
#else
struct fr_u2 { uint16_t x, y; };
struct fr_i2 { int16_t x, y; };
HDFN unsigned fr_perm(unsigned hi, unsigned lo, unsigned sel) {
  const uint64_t src = ((uint64_t)hi << 32) | lo;
  unsigned r = 0;
  for (int k = 0; k < 4; k++) {
    const unsigned s = (sel >> (8 * k)) & 255u;
    const unsigned b = s < 8 ? (unsigned)((src >> (8 * s)) & 255u) : 0u;   // the selectors above use 0..7 and 0x0c only
    r |= b << (8 * k);
  }
  return r;
}
HDFN fr_u2 fr_lanes(unsigned w) { return fr_u2{(uint16_t)(w & 0xFFFFu), (uint16_t)(w >> 16)}; }
HDFN fr_u2 fr_maxu(fr_u2 a, fr_u2 b) { return fr_u2{a.x > b.x ? a.x : b.x, a.y > b.y ? a.y : b.y}; }
HDFN fr_u2 fr_minu(fr_u2 a, fr_u2 b) { return fr_u2{a.x < b.x ? a.x : b.x, a.y < b.y ? a.y : b.y}; }
HDFN int16_t fr_wrap16(int v) { return (int16_t)(uint16_t)((unsigned)v & 0xFFFFu); }
HDFN fr_i2 fr_subi(fr_u2 a, fr_u2 b) { return fr_i2{fr_wrap16((int)a.x - (int)b.x), fr_wrap16((int)a.y - (int)b.y)}; }
HDFN fr_i2 fr_maxi(fr_i2 a, fr_i2 b) { return fr_i2{a.x > b.x ? a.x : b.x, a.y > b.y ? a.y : b.y}; }
HDFN unsigned fr_signs(fr_u2 t, fr_i2 v) {
  const unsigned lo = (unsigned)((int)t.x - (int)v.x) & 0xFFFFu, hi = (unsigned)((int)t.y - (int)v.y) & 0xFFFFu;
  return lo | (hi << 16);
}
#endif

// two pixels of one dword, zero-extended into the 16-bit lanes
HDFN fr_u2 fr_even(unsigned w) { return fr_lanes(fr_perm(0u, w, FR_SEL_EVEN)); }
HDFN fr_u2 fr_odd(unsigned w) { return fr_lanes(fr_perm(0u, w, FR_SEL_ODD)); }
// the threshold in both lanes
HDFN fr_u2 fr_thr2(int t) { return fr_lanes((unsigned)t * 0x00010001u); }

// The predicate on two pixels at once.  Bit 15 and bit 31 of the result are the pass bits of the low and the high lane's pixel (the
// sign of t - v); the other bits are the difference's and mean nothing.
HDFN unsigned fr_pass2(fr_u2 c, fr_u2 p0, fr_u2 p8, fr_u2 p4, fr_u2 p12, fr_u2 t2) {
  const fr_u2 bm = fr_minu(fr_maxu(p0, p8), fr_maxu(p4, p12));
  const fr_u2 dm = fr_maxu(fr_minu(p0, p8), fr_minu(p4, p12));
  return fr_signs(t2, fr_maxi(fr_subi(bm, c), fr_subi(c, dm)));
}

// The quick reject of the four pixels of a dword: cw the centres, uw / dw the same columns 3 rows below / above, p4w / p12w the centre
// row shifted by 3 pixels (the pixels to the right / left of each centre).  Bit j of the result: pixel j passes.
HDFN unsigned fast_reject4(unsigned cw, unsigned uw, unsigned dw, unsigned p4w, unsigned p12w, int t) {
  const fr_u2 t2 = fr_thr2(t);
  const unsigned e = fr_pass2(fr_even(cw), fr_even(uw), fr_even(dw), fr_even(p4w), fr_even(p12w), t2);
  const unsigned o = fr_pass2(fr_odd(cw), fr_odd(uw), fr_odd(dw), fr_odd(p4w), fr_odd(p12w), t2);
  return ((e >> 15) & 1u) | ((o >> 14) & 2u) | ((e >> 29) & 4u) | ((o >> 28) & 8u);
}

// The same for the four dwords of a strip's row, as the strip kernel holds it: c[0..5], u[0..5], d[0..5] are a row's six dwords (left
// neighbour, the lane's own four, right neighbour) of the centre row and of the rows 3 below / above; only [1..4] of u and d are read.
// The shifted rows are never formed: the pixels 3 to the left of pixels (0, 2) are pixels (1, 3) of the dword to the left, those 3 to
// the right of pixels (1, 3) are pixels (0, 2) of the dword to the right, and the other two pairs take one v_perm_b32 each.
// Bit 4 * q + j of the result: pixel j of dword q passes (bit = column of the strip, the order the survivors' compaction reads).
HDFN unsigned fast_reject16(const unsigned* c, const unsigned* u, const unsigned* d, int t) {
  const fr_u2 t2 = fr_thr2(t);
  unsigned acc = 0;
  fr_u2 left_odd = fr_odd(c[0]), ce = fr_even(c[1]);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int q = 0; q < 4; q++) {
    const unsigned cw = c[1 + q];
    const fr_u2 co = fr_odd(cw), right_even = fr_even(c[2 + q]);
    const fr_u2 p12o = fr_lanes(fr_perm(cw, c[q], FR_SEL_L3_ODD)), p4e = fr_lanes(fr_perm(c[2 + q], cw, FR_SEL_R3_EVEN));
    const unsigned e = fr_pass2(ce, fr_even(u[1 + q]), fr_even(d[1 + q]), p4e, left_odd, t2);
    const unsigned o = fr_pass2(co, fr_odd(u[1 + q]), fr_odd(d[1 + q]), right_even, p12o, t2);
    // pixels 0, 1 of the dword to bits 4q, 4q + 1; pixels 2, 3 to the same bits of the upper half
    acc |= (e >> (15 - 4 * q)) & (0x00010001u << (4 * q));
    acc |= (o >> (14 - 4 * q)) & (0x00020002u << (4 * q));
    left_odd = co; ce = right_even;
  }
  return (acc | (acc >> 14)) & 0xFFFFu;   // the upper half's bits 4q, 4q + 1 are pixels 2, 3: two places up
}
