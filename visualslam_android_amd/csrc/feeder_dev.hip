// Synthetic frame feeder on the device (vslam_feeder_render_device): the texture and the frames of many feeders at once, the
// same arithmetic as the host feeder (feeder.cpp: feeder_texture, render_one) evaluated per texel / pixel, so that the bytes
// are the host's (no contraction: -ffp-contract=off; IEEE double + - * / are correctly rounded on both sides).
#include <hip/hip_runtime.h>
#include <cstring>
#include <vector>
#include "../../include/vslam_feeder.h"
#include "feeder_internal.h"
#include "vslam_internal.h"   // DevTemp

using namespace feeder_detail;

namespace {

// value noise of every texel of feeder blockIdx.y (feeder_texture's first loop)
__global__ void k_feeder_noise(const float* __restrict__ lat, uint8_t* __restrict__ tex) {
  const int f = blockIdx.y;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)TEX * TEX) return;
  const int G = LAT;
  const float* l = lat + (size_t)f * (G + 1) * (G + 1);
  const int x = (int)(i % TEX), y = (int)(i / TEX);
  const double gx = (double)x * G / TEX, gy = (double)y * G / TEX;
  const int ix = (int)gx, iy = (int)gy;
  const double fx = gx - ix, fy = gy - iy;
  const double n = (1 - fy) * ((1 - fx) * l[iy * (G + 1) + ix] + fx * l[iy * (G + 1) + ix + 1]) +
                   fy * ((1 - fx) * l[(iy + 1) * (G + 1) + ix] + fx * l[(iy + 1) * (G + 1) + ix + 1]);
  tex[(size_t)f * TEX * TEX + i] = (uint8_t)(128 + 18 * n);
}

// the rectangles of feeder blockIdx.x painted in their order (one workgroup per feeder, a barrier between rectangles)
__global__ void k_feeder_rects(const int* __restrict__ rects, int nrect, uint8_t* __restrict__ tex) {
  const int* r = rects + (size_t)blockIdx.x * nrect * 5;
  uint8_t* t = tex + (size_t)blockIdx.x * TEX * TEX;
  for (int k = 0; k < nrect; k++) {
    const int x0 = r[5 * k], y0 = r[5 * k + 1], rw = r[5 * k + 2], rh = r[5 * k + 3];
    const uint8_t g = (uint8_t)r[5 * k + 4];
    for (int p = threadIdx.x; p < rw * rh; p += blockDim.x) t[(size_t)(y0 + p / rw) * TEX + x0 + p % rw] = g;
    __syncthreads();
  }
}

// one pixel of frame blockIdx.y of feeder blockIdx.z (render_one)
__global__ void k_feeder_render(const uint8_t* __restrict__ tex, const float* __restrict__ rays, const double* __restrict__ poses,
                                const uint64_t* __restrict__ keys, int w, int h, int noise, int count, uint8_t* out,
                                size_t feeder_stride, size_t frame_stride) {
  const int f = blockIdx.z, j = blockIdx.y;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= w * h) return;
  const int x = i % w, y = i / w;
  const double* P = poses + ((size_t)f * count + j) * 12;
  const uint64_t noise_key = keys[(size_t)f * count + j];
  const uint8_t* T = tex + (size_t)f * TEX * TEX;
  const double* R = P; const double* t = P + 9;
  const double C[3] = {-(R[0] * t[0] + R[3] * t[1] + R[6] * t[2]), -(R[1] * t[0] + R[4] * t[1] + R[7] * t[2]), -(R[2] * t[0] + R[5] * t[1] + R[8] * t[2])};
  const float* ry = &rays[2 * ((size_t)y * w + x)];
  const double cx = ry[0], cy = ry[1];
  const double dx = R[0] * cx + R[3] * cy + R[6], dy = R[1] * cx + R[4] * cy + R[7], dz = R[2] * cx + R[5] * cy + R[8];
  int v = 128;
  if (dz > 1e-6) {
    const double s = -C[2] / dz;
    const double u = (C[0] + s * dx + TEX_M / 2) * PPM - 0.5, vv = (C[1] + s * dy + TEX_M / 2) * PPM - 0.5;
    if (u >= 0 && vv >= 0 && u < TEX - 1 && vv < TEX - 1) {
      const int iu = (int)u, iv = (int)vv;
      const double fu = u - iu, fv = vv - iv;
      const uint8_t* p = &T[(size_t)iv * TEX + iu];
      v = (int)((1 - fv) * ((1 - fu) * p[0] + fu * p[1]) + fv * ((1 - fu) * p[TEX] + fu * p[TEX + 1]) + 0.5);
    }
  }
  if (noise) v += (int)(hash32(noise_key * 0x100000001B3ull + (uint64_t)y * w + x) % (2 * noise + 1)) - noise;
  out[(size_t)f * feeder_stride + (size_t)j * frame_stride + (size_t)y * w + x] = (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}

bool same_camera(const vslam_feeder* a, const vslam_feeder* b) {
  return a->w == b->w && a->h == b->h && a->noise == b->noise && a->rects.size() == b->rects.size() &&
         a->focal[0] == b->focal[0] && a->focal[1] == b->focal[1] && a->center[0] == b->center[0] && a->center[1] == b->center[1] &&
         a->ww == b->ww;
}

}  // namespace

extern "C" int vslam_feeder_render_device(const vslam_feeder* const* feeders, int n, int first, int count, const double* poses,
                                          const uint64_t* keys, uint8_t* out, size_t feeder_stride, size_t frame_stride, int device) {
  if (!feeders || n <= 0 || count <= 0 || !out || (!poses) != (!keys)) return -1;
  const vslam_feeder* f0 = feeders[0];
  for (int i = 0; i < n; i++)
    if (!feeders[i] || !same_camera(f0, feeders[i])) return -1;
  const int w = f0->w, h = f0->h, nrect = (int)(f0->rects.size() / 5);
  if (frame_stride < (size_t)w * h || (n > 1 && feeder_stride < (size_t)count * frame_stride)) return -1;
  const size_t nlat = (size_t)(LAT + 1) * (LAT + 1);
  std::vector<float> lat(nlat * n);
  std::vector<int> rects((size_t)nrect * 5 * n + 5);
  std::vector<uint64_t> k((size_t)n * count);
  std::vector<double> P;
  if (!poses) {                        // vslam_feeder_render's frames first .. first + count - 1: pose_at(first + j), key first + j + 100000
    P.resize((size_t)n * count * 12);
    for (int i = 0; i < n; i++)
      for (int j = 0; j < count; j++) pose_at(feeders[i], first + j, &P[((size_t)i * count + j) * 12]);
    poses = P.data();
  }
  for (int i = 0; i < n; i++) {
    memcpy(&lat[nlat * i], feeders[i]->lat.data(), nlat * sizeof(float));
    if (nrect) memcpy(&rects[(size_t)nrect * 5 * i], feeders[i]->rects.data(), (size_t)nrect * 5 * sizeof(int));
    for (int j = 0; j < count; j++)                                                                                   // render_pose's key
      k[(size_t)i * count + j] = (keys ? keys[(size_t)i * count + j] : (uint64_t)(first + j + 100000)) ^ (feeders[i]->seed << 20);
  }
  if (hipSetDevice(device) != hipSuccess) return -2;
  DevTemp<float> d_lat, d_rays; DevTemp<int> d_rects; DevTemp<double> d_poses; DevTemp<uint64_t> d_keys; DevTemp<uint8_t> d_tex;
  int rc = 0;
  if (d_lat.get(lat.size()) != hipSuccess || d_rects.get(rects.size()) != hipSuccess || d_rays.get(f0->rays.size()) != hipSuccess ||
      d_poses.get((size_t)n * count * 12) != hipSuccess || d_keys.get(k.size()) != hipSuccess || d_tex.get((size_t)n * TEX * TEX) != hipSuccess) {
    rc = -3;
  } else if (hipMemcpy(d_lat.p, lat.data(), lat.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
             hipMemcpy(d_rects.p, rects.data(), rects.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess ||
             hipMemcpy(d_rays.p, f0->rays.data(), f0->rays.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
             hipMemcpy(d_poses.p, poses, (size_t)n * count * 12 * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
             hipMemcpy(d_keys.p, k.data(), k.size() * sizeof(uint64_t), hipMemcpyHostToDevice) != hipSuccess) {
    rc = -4;
  } else {
    hipLaunchKernelGGL(k_feeder_noise, dim3((unsigned)(((size_t)TEX * TEX + 255) / 256), n), dim3(256), 0, 0, d_lat.p, d_tex.p);
    hipLaunchKernelGGL(k_feeder_rects, dim3(n), dim3(1024), 0, 0, d_rects.p, nrect, d_tex.p);
    hipLaunchKernelGGL(k_feeder_render, dim3((unsigned)((w * h + 255) / 256), count, n), dim3(256), 0, 0, d_tex.p, d_rays.p, d_poses.p, d_keys.p,
                       w, h, f0->noise, count, out, feeder_stride, frame_stride);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) rc = -4;
  }
  return rc;
}
