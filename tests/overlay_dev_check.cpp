// Host-side check of csrc/overlay_dev.h (tests/test_overlay_ref.py compiles and runs it, with sanitizers): the header's lines, disc,
// mark, ranks and colours as plain C++, printed for the numpy restatement to compare.
//   L dx dy n hash     the line from (5, -3) to (5 + dx, -3 + dy): pixel count and a hash over its pixels in order
//   D n ...            the disc's offsets (dx dy pairs, row by row)
//   M ...              the mark's offsets
//   C cls rgba rgba0   a class's colour bytes (R G B A), with and without VSLAM_DRAW_ALPHA0
//   R ok               ranks are unique, ordered marks < lines < discs (first disc highest) and ov_rank_kind inverts them
#include <stdio.h>
#include "../visualslam_android_amd/csrc/overlay_dev.h"

int main() {
  for (int dx = -40; dx <= 40; dx++)
    for (int dy = -40; dy <= 40; dy++) {
      const OvLine L = ov_line_setup(5, -3, 5 + dx, -3 + dy);
      unsigned long long h = 0;
      for (int i = 0; i <= L.a; i++) {
        int x, y;
        ov_line_pixel(L, i, &x, &y);
        h = h * 1000003ull + (unsigned long long)(x + 100) * 65537ull + (unsigned long long)(y + 100);
      }
      printf("L %d %d %d %llu\n", dx, dy, L.a + 1, h);
    }
  int n = 0;
  for (int dy = -OV_DISC_R; dy <= OV_DISC_R; dy++) n += 2 * ov_disc_half_width(dy) + 1;
  printf("D %d", n);
  for (int dy = -OV_DISC_R; dy <= OV_DISC_R; dy++)
    for (int dx = -ov_disc_half_width(dy); dx <= ov_disc_half_width(dy); dx++) printf(" %d %d", dx, dy);
  printf("\n");
  for (int dy = -3; dy <= 3; dy++)
    for (int dx = -3; dx <= 3; dx++) {
      const int h = (dy >= -OV_DISC_R && dy <= OV_DISC_R) ? ov_disc_half_width(dy) : -1;
      if (ov_disc_covers(dx, dy) != (dx >= -h && dx <= h)) { printf("disc rows and ov_disc_covers disagree at %d %d\n", dx, dy); return 1; }
    }
  printf("M");
  for (int k = 0; k < OV_MARK_PIXELS; k++) { int dx, dy; ov_mark_pixel(k, &dx, &dy); printf(" %d %d", dx, dy); }
  printf("\n");
  for (int cls = OV_LEVEL0; cls <= OV_MARK; cls++) {
    const uint32_t a = ov_colour(cls, false), b = ov_colour(cls, true);
    printf("C %d %u %u %u %u %u %u %u %u\n", cls, a & 255, (a >> 8) & 255, (a >> 16) & 255, a >> 24, b & 255, (b >> 8) & 255, (b >> 16) & 255, b >> 24);
  }
  const int nm = 5, nl = 3, nd = 4;
  uint32_t prev = 0;
  bool ok = true;
  for (int i = 0; i < nm; i++) { const uint32_t r = ov_rank_mark(i); int idx; ok = ok && r > prev && ov_rank_kind(r, nm, nl, nd, &idx) == 0 && idx == i; prev = r; }
  for (int i = 0; i < nl; i++) { const uint32_t r = ov_rank_line(nm, i); int idx; ok = ok && r > prev && ov_rank_kind(r, nm, nl, nd, &idx) == 1 && idx == i; prev = r; }
  for (int j = nd - 1; j >= 0; j--) { const uint32_t r = ov_rank_disc(nm, nl, nd, j); int idx; ok = ok && r > prev && ov_rank_kind(r, nm, nl, nd, &idx) == 2 && idx == j; prev = r; }
  ok = ok && ov_gray(0x7Fu) == 0xFF7F7F7Fu && ov_coord_ok(OV_COORD_MAX) && !ov_coord_ok(OV_COORD_MAX + 1) && !ov_coord_ok(-OV_COORD_MAX - 1);
  printf("R %s\n", ok ? "ok" : "bad");
  return ok ? 0 : 1;
}
