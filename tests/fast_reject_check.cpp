// Host-side check of csrc/fast_reject_dev.h (tests/test_fast_reject_host.py compiles and runs it, plain and with sanitizers): the packed
// quick reject against the predicate in plain integers, written out here.
//   fast_reject4   every centre 0..255 x t in {1, 10, 15, 127, 255} x each compass pixel from {0, 1, c-t-1, c-t, c-t+1, c, c+t-1, c+t,
//                  c+t+1, 254, 255} clipped to 0..255: 256 * 5 * 11^4 = 18,739,200 dwords.  Byte j of a dword holds the case whose centre
//                  is c + 64 j and whose value indices are advanced by (j, 2j, 3j, 4j) mod 11 -- a bijection of the case set per byte
//                  position, so every case is met at all four byte positions, always beside three different cases.
//   fast_reject16  seeded rows of six dwords drawn from the same edge values, against the predicate with the neighbours taken from the
//                  bytes of the row: the shifted pairs that the strip kernel never forms as dwords.
// Prints "R4 <dwords> <passes>", "R16 <rows> <passes>" and "ok"; exit status 1 with the first disagreement otherwise.
#include <stdio.h>
#include "../visualslam_android_amd/csrc/fast_reject_dev.h"

// the predicate twice: as the strip kernel states it, and as the segment test's necessary condition it stands for
static bool pass_formula(int c, int p0, int p8, int p4, int p12, int t) {
  const int max08 = p0 > p8 ? p0 : p8, max412 = p4 > p12 ? p4 : p12, min08 = p0 < p8 ? p0 : p8, min412 = p4 < p12 ? p4 : p12;
  const int bm = max08 < max412 ? max08 : max412, dm = min08 > min412 ? min08 : min412;
  const int a = bm - c, b = c - dm;
  return (a > b ? a : b) > t;
}
static bool pass_pairs(int c, int p0, int p8, int p4, int p12, int t) {
  const int cb = c + t, c_b = c - t;
  const int p[4] = {p0, p4, p8, p12};
  for (int k = 0; k < 4; k++) {
    const int a = p[k], b = p[(k + 1) & 3];
    if ((a > cb && b > cb) || (a < c_b && b < c_b)) return true;
  }
  return false;
}
static int clip(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
static void edge_values(int c, int t, int* v) {
  const int e[11] = {0, 1, c - t - 1, c - t, c - t + 1, c, c + t - 1, c + t, c + t + 1, 254, 255};
  for (int k = 0; k < 11; k++) v[k] = clip(e[k]);
}

int main() {
  static const int thr[5] = {1, 10, 15, 127, 255};
  unsigned long long n4 = 0, pass4 = 0;
  for (int ti = 0; ti < 5; ti++) {
    const int t = thr[ti];
    for (int c0 = 0; c0 < 256; c0++) {
      int cj[4], ev[4][11];
      for (int j = 0; j < 4; j++) { cj[j] = (c0 + 64 * j) & 255; edge_values(cj[j], t, ev[j]); }
      for (int i0 = 0; i0 < 11; i0++)
        for (int i8 = 0; i8 < 11; i8++)
          for (int i4 = 0; i4 < 11; i4++)
            for (int i12 = 0; i12 < 11; i12++) {
              unsigned cw = 0, uw = 0, dw = 0, p4w = 0, p12w = 0;
              int P0[4], P8[4], P4[4], P12[4];
              for (int j = 0; j < 4; j++) {
                P0[j] = ev[j][(i0 + j) % 11]; P8[j] = ev[j][(i8 + 2 * j) % 11]; P4[j] = ev[j][(i4 + 3 * j) % 11]; P12[j] = ev[j][(i12 + 4 * j) % 11];
                cw |= (unsigned)cj[j] << (8 * j); uw |= (unsigned)P0[j] << (8 * j); dw |= (unsigned)P8[j] << (8 * j);
                p4w |= (unsigned)P4[j] << (8 * j); p12w |= (unsigned)P12[j] << (8 * j);
              }
              const unsigned got = fast_reject4(cw, uw, dw, p4w, p12w, t);
              for (int j = 0; j < 4; j++) {
                const bool want = pass_formula(cj[j], P0[j], P8[j], P4[j], P12[j], t);
                if (want != pass_pairs(cj[j], P0[j], P8[j], P4[j], P12[j], t)) { printf("the two plain forms disagree: c %d p0 %d p8 %d p4 %d p12 %d t %d\n", cj[j], P0[j], P8[j], P4[j], P12[j], t); return 1; }
                if ((((got >> j) & 1u) != 0) != want) { printf("fast_reject4: byte %d c %d p0 %d p8 %d p4 %d p12 %d t %d: packed %u plain %d\n", j, cj[j], P0[j], P8[j], P4[j], P12[j], t, (got >> j) & 1u, (int)want); return 1; }
                pass4 += want;
              }
              if (got >> 4) { printf("fast_reject4 sets bits above the dword's four: %08x\n", got); return 1; }
              n4++;
            }
    }
  }
  printf("R4 %llu %llu\n", n4, pass4);

  unsigned long long n16 = 0, pass16 = 0;
  uint32_t rng = 12345u;
  for (int ti = 0; ti < 5; ti++) {
    const int t = thr[ti];
    for (int it = 0; it < 40000; it++) {
      uint8_t rows[3][24];                                            // centre, 3 below, 3 above: six dwords each
      int ev[11];
      rng = rng * 1664525u + 1013904223u;
      edge_values((int)(rng >> 24), t, ev);
      for (int r = 0; r < 3; r++)
        for (int x = 0; x < 24; x++) {
          rng = rng * 1664525u + 1013904223u;
          rows[r][x] = (it & 1) ? (uint8_t)(rng >> 24) : (uint8_t)ev[(rng >> 20) % 11u];
        }
      unsigned c[6], u[6], d[6];
      for (int q = 0; q < 6; q++) {
        c[q] = u[q] = d[q] = 0;
        for (int j = 0; j < 4; j++) { c[q] |= (unsigned)rows[0][4 * q + j] << (8 * j); u[q] |= (unsigned)rows[1][4 * q + j] << (8 * j); d[q] |= (unsigned)rows[2][4 * q + j] << (8 * j); }
      }
      const unsigned got = fast_reject16(c, u, d, t);
      for (int x = 0; x < 16; x++) {
        const bool want = pass_formula(rows[0][4 + x], rows[1][4 + x], rows[2][4 + x], rows[0][4 + x + 3], rows[0][4 + x - 3], t);
        if ((((got >> x) & 1u) != 0) != want) { printf("fast_reject16: row %d t %d column %d: packed %u plain %d\n", it, t, x, (got >> x) & 1u, (int)want); return 1; }
        pass16 += want;
      }
      if (got >> 16) { printf("fast_reject16 sets bits above the row's sixteen: %08x\n", got); return 1; }
      n16++;
    }
  }
  printf("R16 %llu %llu\n", n16, pass16);
  printf("ok\n");
  return 0;
}
