// Stand-alone host build of csrc/fuse_dev.h (tests/test_fuse_rules_header.py).  Reads cases from stdin.  A case is a line
// "nk np min_views radius_bits", then nk * np lines "valid level source rootx_bits rooty_bits" (keyframe-major; doubles as the decimal
// value of their 64 bits), then np lines "bad w0 w1" (the never-retry words).  Per case it prints one line: "P" and partner(p) of every
// point, "D" and what every point is dropped into (-1: it stays), "T" and a quadruple "k q p source" per cell taken, keyframe-major,
// then "N" and the valid cells of dropped points not taken.  The loops around the header's functions are the plainest possible (every
// q for every p); the comparison with the numpy model is the test's.
#include <inttypes.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../visualslam_android_amd/csrc/fuse_dev.h"

struct Cell { int valid, level, source; double x, y; };

static double from_bits(unsigned long long b) { double d; memcpy(&d, &b, sizeof(d)); return d; }

int main() {
  int nk, np, min_views;
  unsigned long long rb;
  size_t n_cases = 0;
  while (scanf("%d %d %d %llu", &nk, &np, &min_views, &rb) == 4) {
    const double radius = from_bits(rb);
    std::vector<Cell> c((size_t)nk * np);
    for (Cell& e : c) {
      unsigned long long bx, by;
      if (scanf("%d %d %d %llu %llu", &e.valid, &e.level, &e.source, &bx, &by) != 5) return 2;
      e.x = from_bits(bx); e.y = from_bits(by);
    }
    std::vector<int> bad((size_t)np), partner((size_t)np, -1), into((size_t)np, -1);
    std::vector<uint64_t> w0((size_t)np), w1((size_t)np);
    for (int i = 0; i < np; i++) {
      unsigned long long a, b;
      if (scanf("%d %llu %llu", &bad[i], &a, &b) != 3) return 2;
      w0[i] = a; w1[i] = b;
    }
    for (int p = 0; p < np; p++) {
      if (bad[p]) continue;
      for (int q = 0; q < p && partner[p] < 0; q++) {
        if (bad[q]) continue;
        int agree = 0, conflict = 0;
        for (int k = 0; k < nk; k++) {
          const Cell& a = c[(size_t)k * np + p]; const Cell& b = c[(size_t)k * np + q];
          const int r = fuse_relation(a.valid, a.level, a.x, a.y, b.valid, b.level, b.x, b.y, radius);
          agree += r == FUSE_AGREE; conflict += r == FUSE_CONFLICT;
        }
        if (fuse_dup(agree, conflict, min_views)) partner[p] = q;
      }
    }
    for (int p = 0; p < np; p++) if (fuse_dropped(partner[p], partner[p] >= 0 ? partner[partner[p]] : 0)) into[p] = partner[p];
    printf("P");
    for (int p = 0; p < np; p++) printf(" %d", partner[p]);
    printf(" D");
    for (int p = 0; p < np; p++) printf(" %d", into[p]);
    printf(" T");
    int not_taken = 0;
    for (int k = 0; k < nk; k++)
      for (int q = 0; q < np; q++) {
        int first = -1;
        for (int p = q + 1; p < np; p++)
          if (into[p] == q && c[(size_t)k * np + p].valid) { if (first < 0) first = p; else not_taken++; }
        if (first < 0) continue;
        if (fuse_takes(c[(size_t)k * np + q].valid, fuse_never_retry_bit(w0[q], w1[q], k))) printf(" %d %d %d %d", k, q, first, fuse_source(c[(size_t)k * np + first].source));
        else not_taken++;
      }
    printf(" N %d\n", not_taken);
    n_cases++;
  }
  printf("cases %zu\n", n_cases);
  return 0;
}
