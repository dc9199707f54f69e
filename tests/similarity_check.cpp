// Stand-alone host build of csrc/similarity_dev.h (tests/test_similarity_header.py): reads cases of 31 doubles -- T (pose12), s, a
// point, a vector, a pose (pose12) -- from the file argv[1] and writes, per case, 44 doubles to argv[2]: pose_inverse(T), sim_point,
// sim_vector, sim_pose, sim_length of the point's first component, and sim_compose of (T, s) behind the case's pose taken as an
// accumulated transform of scale |vector[0]| + 0.5 (pose12, scale).  Nothing else: the comparison with the numpy model is the test's.
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../visualslam_android_amd/csrc/similarity_dev.h"

#define CASE_IN 31
#define CASE_OUT 44

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: similarity_check cases.bin out.bin\n"); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  std::vector<double> in;
  double buf[CASE_IN];
  while (fread(buf, sizeof(double), CASE_IN, f) == CASE_IN) in.insert(in.end(), buf, buf + CASE_IN);
  fclose(f);
  const size_t n = in.size() / CASE_IN;
  std::vector<double> out(n * CASE_OUT);
  for (size_t i = 0; i < n; i++) {
    const double* c = &in[i * CASE_IN];
    double* o = &out[i * CASE_OUT];
    Pose T, C;
    for (int k = 0; k < 9; k++) { T.R[k] = c[k]; C.R[k] = c[19 + k]; }
    for (int k = 0; k < 3; k++) { T.t[k] = c[9 + k]; C.t[k] = c[28 + k]; }
    const double s = c[12];
    const Similarity g = sim_make(T, s);
    for (int k = 0; k < 9; k++) o[k] = g.Tinv.R[k];
    for (int k = 0; k < 3; k++) o[9 + k] = g.Tinv.t[k];
    sim_point(g, c + 13, o + 12);
    sim_vector(g, c + 16, o + 15);
    const Pose D = sim_pose(g, C);
    for (int k = 0; k < 9; k++) o[18 + k] = D.R[k];
    for (int k = 0; k < 3; k++) o[27 + k] = D.t[k];
    o[30] = sim_length(g, c[13]);
    Pose acc = C;
    double accs = (c[16] < 0 ? -c[16] : c[16]) + 0.5;
    sim_compose(T, s, acc, accs);
    for (int k = 0; k < 9; k++) o[31 + k] = acc.R[k];
    for (int k = 0; k < 3; k++) o[40 + k] = acc.t[k];
    o[43] = accs;
  }
  f = fopen(argv[2], "wb");
  if (!f) { perror(argv[2]); return 2; }
  if (fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) { fclose(f); return 3; }
  fclose(f);
  printf("cases %zu\n", n);
  return 0;
}
