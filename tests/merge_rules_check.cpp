// Stand-alone host build of csrc/merge_dev.h (tests/test_merge_rules_header.py).  Reads cases from stdin, one per line, as 13 decimal
// numbers -- w0 w1 nk_s nk_d flags k p np_d stored_d j fq_cap fq_n max_points -- and prints per case one line of 8:
// merge_never_retry's two words, merge_flags, merge_queue_entry's keyframe and point, merge_queue_slot, merge_queue_stored,
// merge_meas_cell.  Nothing else: the comparison with the numpy model is the test's.
#include <inttypes.h>
#include <stdio.h>
#include "../visualslam_android_amd/csrc/merge_dev.h"

int main() {
  unsigned long long w0, w1;
  int nk_s, nk_d, flags, k, p, np_d, stored_d, j, cap, fq_n, maxp;
  size_t n = 0;
  while (scanf("%llu %llu %d %d %d %d %d %d %d %d %d %d %d", &w0, &w1, &nk_s, &nk_d, &flags, &k, &p, &np_d, &stored_d, &j, &cap, &fq_n, &maxp) == 13) {
    uint64_t o0 = 0, o1 = 0;
    merge_never_retry((uint64_t)w0, (uint64_t)w1, nk_s, nk_d, &o0, &o1);
    int ok = 0, op = 0;
    merge_queue_entry(k, p, nk_d, np_d, &ok, &op);
    printf("%" PRIu64 " %" PRIu64 " %d %d %d %d %d %zu\n", o0, o1, merge_flags(flags), ok, op, merge_queue_slot(stored_d, j, cap), merge_queue_stored(fq_n, cap),
           merge_meas_cell(k, p, nk_d, np_d, maxp));
    n++;
  }
  printf("cases %zu\n", n);
  return 0;
}
