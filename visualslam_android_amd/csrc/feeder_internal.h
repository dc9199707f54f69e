// Synthetic frame feeder internals shared by the host feeder (feeder.cpp) and its device renderer (feeder_dev.hip).
#ifndef VSLAM_FEEDER_INTERNAL_H
#define VSLAM_FEEDER_INTERNAL_H
#include <cmath>
#include <mutex>
#include <stdint.h>
#include <vector>

namespace feeder_detail {

struct Rng {  // xorshift64*
  uint64_t s;
  explicit Rng(uint64_t seed) : s(seed * 0x9E3779B97F4A7C15ull + 0x1234567ull) { if (!s) s = 1; }
  uint64_t next() { s ^= s >> 12; s ^= s << 25; s ^= s >> 27; return s * 0x2545F4914F6CDD1Dull; }
  double uni() { return (next() >> 11) * (1.0 / 9007199254740992.0); }
  int range(int lo, int hi) { return lo + (int)(uni() * (hi - lo)); }
};

#if defined(__HIPCC__)
__host__ __device__
#endif
inline uint32_t hash32(uint64_t x) {
  x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33;
  return (uint32_t)x;
}

constexpr int TEX = 4096;          // texels per side
constexpr double TEX_M = 4.0;      // metres per side: plane patch [-2,2]^2
constexpr double PPM = TEX / TEX_M;
constexpr int LAT = 64;            // coarse lattice of the texture's value noise

}  // namespace feeder_detail

struct vslam_feeder {
  int w, h, noise;
  uint64_t seed;
  double focal[2], center[2], inv_focal[2], ww, winv, two_tan, one_over_2tan;
  std::vector<float> lat;    // (LAT + 1)^2 value-noise lattice
  std::vector<int> rects;    // x0, y0, w, h, grey of every rectangle, in painting order
  std::vector<uint8_t> tex;  // TEX x TEX, made from lat + rects on first host render (feeder_texture)
  std::once_flag tex_once;
  std::vector<float> rays;   // per pixel: z = 1 plane coordinates of the (distorted) pixel
  // trajectory parameters
  double radius, height, dtheta, phase, wob_a, wob_b;

  // ATAN/FOV camera (jni/ATANCamera.cc:133-164, ATANCamera.h:136-150)
  void unproject(double ix, double iy, double out[2]) const {
    const double dx = (ix - center[0]) * inv_focal[0], dy = (iy - center[1]) * inv_focal[1];
    const double dr = std::sqrt(dx * dx + dy * dy);
    const double r = ww == 0.0 ? dr : std::tan(dr * ww) * one_over_2tan;
    const double f = dr > 0.01 ? r / dr : 1.0;
    out[0] = dx * f; out[1] = dy * f;
  }
  void project(double cx, double cy, double im[2]) const {
    const double r = std::sqrt(cx * cx + cy * cy);
    const double fac = (r < 0.001 || ww == 0.0) ? 1.0 : winv * std::atan(r * two_tan) / r;
    im[0] = center[0] + focal[0] * (cx * fac); im[1] = center[1] + focal[1] * (cy * fac);
  }
};

// ground-truth pose at frame t (feeder.cpp; vslam_feeder_pose)
void pose_at(const vslam_feeder* f, double t, double P[12]);

#endif
