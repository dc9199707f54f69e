// MapMaker::ApplyGlobalScaleToMap and ApplyGlobalTransformationToMap of include/vslam/ptam.h (jni/MapMaker.cc:440-464) against the
// C call they mirror.  Two SystemPTAM-style sets of drop-in objects get the same uploaded map and the same frames; one is moved by the
// two members (the scale, then the rigid transform), the other by one vslam_transform_maps with both; every read-back that the move
// touches must then be equal, double for double, and stay equal over one more tracked frame.
// Usage: transform_mirror [n_frames]   (needs an MI355X; prints "mirror ok" and returns 0 when everything is equal)
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../include/vslam/ptam.h"
#include "../include/vslam_feeder.h"

struct Objects {   // jni/jni_part.cpp:20-46
  ATANCamera cam; Map map; MapMaker mm; Tracker tracker;
  Objects(int w, int h) : cam("Camera"), mm(map, cam), tracker(w, h, cam, map, mm) {}
};

static int upload(vslam_system* dev, vslam_feeder* f, int W, int H) {   // one source keyframe, every third maximal corner (examples/system_ptam.cpp)
  double kfpose[12];
  vslam_feeder_pose(f, -20, kfpose);
  std::vector<uint8_t> img((size_t)W * H);
  vslam_feeder_render_pose(f, kfpose, 1, img.data(), W);
  if (vslam_map_add_keyframe(dev, 0, kfpose, 1, img.data(), W, 1.0, 0.1) < 0) return -1;
  vslam_make_keyframe_lite(dev, img.data(), W, 0, 0);
  vslam_fast_nonmax(dev);
  int npts = 0;
  for (int l = 0; l < 4; l++) {
    std::vector<uint32_t> c(100000); int nc = 0;
    vslam_read_max_corners(dev, 0, l, c.data(), nullptr, (int)c.size(), &nc);
    for (int i = 0; i < nc; i += 3) {
      const int x = c[i] & 0xFFFF, y = c[i] >> 16;
      if (x < 10 || y < 10 || x >= (W >> l) - 10 || y >= (H >> l) - 10) continue;
      double pos[3], r[3], d[3];
      if (vslam_feeder_make_point(f, kfpose, l, x, y, pos, r, d)) continue;
      const int p = vslam_map_add_point(dev, 0, pos, 0, l, x, y, r, d);
      if (p < 0) break;
      const double root[2] = {(x + 0.5) * (1 << l) - 0.5, (y + 0.5) * (1 << l) - 0.5};
      vslam_map_add_measurement(dev, 0, 0, p, l, root, 1, 2);
      npts++;
    }
  }
  vslam_map_set_good(dev, 0);
  double start[12];
  vslam_feeder_pose(f, -1, start);
  vslam_set_pose(dev, 0, start);
  return npts;
}

// every double the move touches that the C ABI reads back
static std::vector<double> readback(vslam_system* dev) {
  std::vector<double> out;
  vslam_track_state st;
  vslam_get_state(dev, 0, &st);
  out.insert(out.end(), st.pose, st.pose + 12);
  out.insert(out.end(), st.velocity, st.velocity + 6);
  out.push_back(st.depth_mean); out.push_back(st.depth_sigma); out.push_back(st.msd_velocity);
  for (int k = 0; k < st.n_keyframes; k++) { double q[12]; vslam_get_keyframe_pose(dev, 0, k, q); out.insert(out.end(), q, q + 12); }
  std::vector<double> pos((size_t)3 * (st.n_points > 0 ? st.n_points : 1));
  vslam_get_points(dev, 0, pos.data(), nullptr, nullptr, nullptr, st.n_points);
  out.insert(out.end(), pos.begin(), pos.begin() + (size_t)3 * st.n_points);
  return out;
}

int main(int argc, char** argv) {
  const int W = 640, H = 480, n = argc > 1 ? atoi(argv[1]) : 3;
  const double cam[5] = {0.841906, 1.10893, 0.505171, 0.470265, -0.0133843};
  vslam_feeder* f = nullptr;
  if (vslam_feeder_create(W, H, cam, 1234, 2, &f)) return 2;
  Objects a(W, H), b(W, H);
  const int na = upload(a.map.sys, f, W, H), nb = upload(b.map.sys, f, W, H);
  if (na <= 0 || na != nb) { fprintf(stderr, "upload: %d, %d points: %s\n", na, nb, vslam_last_error()); return 1; }
  cv::Mat bw(H, W, CV_8UC1), rgb(H, W, CV_8UC4);
  auto frame = [&](int t) {
    double p[12];
    vslam_feeder_pose(f, t, p);
    vslam_feeder_render_pose(f, p, 100 + t, bw.data, bw.step);
    a.tracker.TrackFrame(bw, rgb, false); b.tracker.TrackFrame(bw, rgb, false);
  };
  for (int t = 0; t < n; t++) frame(t);
  const std::vector<double> before = readback(a.map.sys);
  bool ok = before == readback(b.map.sys);
  mySE3 T;                                                           // a quarter turn about z and a shift, exactly representable
  const double R[9] = {0, -1, 0, 1, 0, 0, 0, 0, 1}, t3[3] = {0.5, -2.0, 1.25}, s = 1.75;
  for (int i = 0; i < 9; i++) T.R[i] = R[i];
  for (int i = 0; i < 3; i++) T.t[i] = t3[i];
  a.mm.ApplyGlobalScaleToMap(s);
  a.mm.ApplyGlobalTransformationToMap(T);
  double q[12];
  for (int i = 0; i < 9; i++) q[i] = R[i];
  for (int i = 0; i < 3; i++) q[9 + i] = t3[i];
  const int s0 = 0;
  if (vslam_transform_maps(b.map.sys, &s0, 1, q, &s) != VSLAM_OK) { fprintf(stderr, "%s\n", vslam_last_error()); return 1; }
  const std::vector<double> ra = readback(a.map.sys), rb = readback(b.map.sys);
  size_t differ = 0, moved = 0;
  for (size_t i = 0; i < ra.size() && i < rb.size(); i++) { differ += ra[i] != rb[i]; moved += ra[i] != before[i]; }
  ok = ok && ra.size() == rb.size() && differ == 0 && moved > (size_t)na;
  int ia[2], ib[2]; double da[13], db[13];
  vslam_get_transform_info(a.map.sys, 0, ia, da); vslam_get_transform_info(b.map.sys, 0, ib, db);
  bool same_acc = true;
  for (int i = 0; i < 13; i++) same_acc = same_acc && da[i] == db[i];
  ok = ok && ia[0] == 2 && ib[0] == 1 && ia[1] == ib[1] && same_acc;
  printf("members: %d transforms, C call: %d; %zu doubles read back, %zu moved, %zu differ; accumulated scale %.17g\n", ia[0], ib[0], ra.size(), moved, differ, da[12]);
  frame(n);
  const bool after = readback(a.map.sys) == readback(b.map.sys);
  printf("next frame: %s | %s\n", after ? "equal" : "DIFFERENT", a.tracker.GetMessageForUser().c_str());
  ok = ok && after && a.tracker.GetMessageForUser().find("quality good") != std::string::npos;
  vslam_feeder_destroy(f);
  if (ok) printf("mirror ok\n");
  return ok ? 0 : 1;
}
