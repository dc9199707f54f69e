// Wavefront-level pieces of the map maker's point making shared by mapgrow.hip (AddPointEpipolar, ReFind_Common) and boot.hip
// (InitFromStereo): the sub-pixel iterations, triangulation, unit rays.  The patch finder proper is in patch_dev.h.
#pragma once
#include "patch_dev.h"

// MakeSubPixTemplate (jni/PatchFinder.cc:242-271) + IterateSubPixToConvergence (:273-350) by one wavefront, starting from
// the level-zero position in sub0/sub1; these are left wherever the iteration stopped (ReFind_Common reads them regardless)
template <int PS>
DEVFN bool wave_subpix(const uint8_t* tmpl, const uint8_t* img, int ip, int wl, int hl, int nLevel, int max_its, int lane, double& sub0, double& sub1, double* slab /* LDS [3][Q*Q] of this wavefront */) {
  constexpr int HALF = PS / 2, Q = PS - 2, NQL = (Q * Q + 63) / 64;
  const int nLevelScale = 1 << nLevel;
  double gx[NQL], gy[NQL];
  double h00 = 0, h01 = 0, h02 = 0, h11 = 0, h12 = 0, h22 = 0;
  for (int q = 0; q < NQL; q++) {
    const int k = q * 64 + lane;
    gx[q] = 0; gy[q] = 0;
    if (k < Q * Q) {
      const int x = k / Q + 1, y = k % Q + 1;
      gx[q] = 0.5 * (tmpl[y * PS + x + 1] - tmpl[y * PS + x - 1]);
      gy[q] = 0.5 * (tmpl[(y + 1) * PS + x] - tmpl[(y - 1) * PS + x]);
      h00 += gx[q] * gx[q]; h01 += gx[q] * gy[q]; h02 += gx[q]; h11 += gy[q] * gy[q]; h12 += gy[q]; h22 += 1.0;
    }
  }
  h00 = wave_sum(h00); h01 = wave_sum(h01); h02 = wave_sum(h02); h11 = wave_sum(h11); h12 = wave_sum(h12); h22 = wave_sum(h22);
  const double H[9] = {h00, h01, h02, h01, h11, h12, h02, h12, h22};
  double Hinv[9];
  inv3(H, Hinv);
  double meanDiff = 0.0;
  for (int it = 0; it < max_its; it++) {
    const double cx = level_n_pos(sub0, nLevel), cy = level_n_pos(sub1, nLevel);
    const int xb = (int)(cx > 0.0 ? cx + 0.5 : cx - 0.5), yb = (int)(cy > 0.0 ? cy + 0.5 : cy - 0.5);
    const int b = HALF + 1;
    if (!(xb >= b && yb >= b && xb < wl - b && yb < hl - b)) return false;
    const double bx = cx - HALF, by = cy - HALF;
    const double dX = bx - floor(bx), dY = by - floor(by);
    const float fTL = (float)((1.0 - dX) * (1.0 - dY)), fTR = (float)((dX) * (1.0 - dY));
    const float fBL = (float)((1.0 - dX) * (dY)), fBR = (float)((dX) * (dY));
    // v3Accum in the reference's pixel order, y outer / x inner (:316-340): the per-pixel products go to LDS in that order
    // and lanes 0..2 walk one sum each (a butterfly over the lanes would round differently)
    for (int q = 0; q < NQL; q++) {
      const int k = q * 64 + lane;
      if (k < Q * Q) {
        const int x = k / Q + 1, y = k % Q + 1;
        const uint8_t* tl = img + (size_t)((int)by + y) * ip + (int)bx + x;
        const float fPixel = fTL * tl[0] + fTR * tl[1] + fBL * tl[ip] + fBR * tl[ip + 1];
        const double dDiff = (fPixel - (float)tmpl[y * PS + x]) + meanDiff;
        const int o = (y - 1) * Q + (x - 1);
        slab[o] = dDiff * gx[q]; slab[Q * Q + o] = dDiff * gy[q]; slab[2 * Q * Q + o] = dDiff;
      }
    }
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_wave_barrier();
    double acc = 0.0;
    if (lane < 3) {
      const double* sp = slab + lane * Q * Q;
      _Pragma("unroll") for (int o = 0; o < Q * Q; o++) acc += sp[o];
    }
    const double a0 = __shfl(acc, 0), a1 = __shfl(acc, 1), a2 = __shfl(acc, 2);
    __builtin_amdgcn_wave_barrier();
    const double u0 = Hinv[0] * a0 + Hinv[1] * a1 + Hinv[2] * a2;
    const double u1 = Hinv[3] * a0 + Hinv[4] * a1 + Hinv[5] * a2;
    const double u2 = Hinv[6] * a0 + Hinv[7] * a1 + Hinv[8] * a2;
    sub0 -= u0 * nLevelScale; sub1 -= u1 * nLevelScale; meanDiff -= u2;
    if (u0 * u0 + u1 * u1 < 0.03 * 0.03) return true;
  }
  return false;
}

// Eigen::JacobiSVD of the square 4x4 triangulation matrix (jni/MapMaker.cc:191-192): two-sided Jacobi on A itself as
// published for Eigen 3.0-3.1 -- sweeps over the pairs (p, q), q < p; a pair is rotated while max(|m_pq|, |m_qp|) >
// 2 eps max(|m_pp|, |m_qq|); the 2x2 step symmetrises the block with a left rotation, then diagonalises it with the Jacobi
// rotation of the symmetric block; V collects the right rotations; the column of V of the smallest |m_ii| is
// matrixV().col(3).  Statement for statement what oracle/mapgrow.cpp evaluates on the host (one lane, same order: same
// bits).  Third-party arithmetic, version unpinned: parity unpinned against the reference.
DEVFN void svd4_smallest_right_vector(const double Ain[16], double out[4]) {
  double M[16], V[16];
  for (int i = 0; i < 16; i++) { M[i] = Ain[i]; V[i] = (i % 5 == 0) ? 1.0 : 0.0; }
  const double precision = 2.0 * 2.220446049250313e-16;
  _Pragma("unroll 1") for (int sweep = 0; sweep < 64; sweep++) {
    bool finished = true;
    _Pragma("unroll") for (int p = 1; p < 4; p++)
      _Pragma("unroll") for (int q = 0; q < p; q++) {
        const double apq = fabs(M[p * 4 + q]), aqp = fabs(M[q * 4 + p]), off = apq > aqp ? apq : aqp;
        const double app = fabs(M[p * 4 + p]), aqq = fabs(M[q * 4 + q]), dia = app > aqq ? app : aqq;
        if (!(off > dia * precision)) continue;
        finished = false;
        const double m00 = M[p * 4 + p], m01 = M[p * 4 + q], m10 = M[q * 4 + p], m11 = M[q * 4 + q];
        double c1, s1;
        const double t = m00 + m11, d = m10 - m01;
        if (t == 0.0) { c1 = 0.0; s1 = d > 0.0 ? 1.0 : -1.0; }
        else { const double u = d / t; c1 = 1.0 / sqrt(1.0 + u * u); s1 = c1 * u; }
        const double x = c1 * m00 + s1 * m10, y = c1 * m01 + s1 * m11, z = -s1 * m01 + c1 * m11;
        double c2, s2;
        if (y == 0.0) { c2 = 1.0; s2 = 0.0; }
        else {
          const double tau = (x - z) / (2.0 * fabs(y)), w = sqrt(tau * tau + 1.0);
          const double tt = tau > 0.0 ? 1.0 / (tau + w) : 1.0 / (tau - w);
          const double sign_t = tt > 0.0 ? 1.0 : -1.0, n = 1.0 / sqrt(tt * tt + 1.0);
          s2 = -sign_t * (y / fabs(y)) * fabs(tt) * n; c2 = n;
        }
        const double cl = c1 * c2 + s1 * s2, sl = s1 * c2 - c1 * s2;
        _Pragma("unroll") for (int k = 0; k < 4; k++) { const double a = M[p * 4 + k], b = M[q * 4 + k]; M[p * 4 + k] = cl * a + sl * b; M[q * 4 + k] = -sl * a + cl * b; }
        _Pragma("unroll") for (int k = 0; k < 4; k++) { const double a = M[k * 4 + p], b = M[k * 4 + q]; M[k * 4 + p] = c2 * a - s2 * b; M[k * 4 + q] = s2 * a + c2 * b; }
        _Pragma("unroll") for (int k = 0; k < 4; k++) { const double a = V[k * 4 + p], b = V[k * 4 + q]; V[k * 4 + p] = c2 * a - s2 * b; V[k * 4 + q] = s2 * a + c2 * b; }
      }
    if (finished) break;
  }
  // the column of the smallest |m_ii| without a dynamically indexed register array (selects)
  double bestv = fabs(M[0]);
  out[0] = V[0]; out[1] = V[4]; out[2] = V[8]; out[3] = V[12];
  _Pragma("unroll") for (int i = 1; i < 4; i++) {
    const double a = fabs(M[i * 4 + i]);
    if (a < bestv) { bestv = a; out[0] = V[i]; out[1] = V[4 + i]; out[2] = V[8 + i]; out[3] = V[12 + i]; }
  }
}

// MapMaker::ReprojectPoint, jni/MapMaker.cc:174-200: the homogeneous vector as the SVD hands it over (:176-192) ...
DEVFN void reproject_vector(const Pose& AfromB, const double v2A[2], const double v2B[2], double v[4]) {
  double PD[12];
  for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) PD[r * 4 + c] = AfromB.R[r * 3 + c]; PD[r * 4 + 3] = AfromB.t[r]; }
  double A[16] = {-1.0, 0.0, v2B[0], 0.0, 0.0, -1.0, v2B[1], 0.0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int c = 0; c < 4; c++) { A[8 + c] = v2A[0] * PD[8 + c] - PD[0 + c]; A[12 + c] = v2A[1] * PD[8 + c] - PD[4 + c]; }
  svd4_smallest_right_vector(A, v);
}
// ... and the point (:194-199)
DEVFN void reproject_point(const Pose& AfromB, const double v2A[2], const double v2B[2], double out[3]) {
  double v[4];
  reproject_vector(AfromB, v2A, v2B, v);
  if (v[3] == 0.0) v[3] = 0.00001;
  out[0] = v[0] / v[3]; out[1] = v[1] / v[3]; out[2] = v[2] / v[3];
}

DEVFN void unit_ray(const CamModel& cam, double ix, double iy, double out[3]) {   // myUnproject + normalize()
  double u[2];
  cam_unproject(cam, ix, iy, u);
  const double n = sqrt(u[0] * u[0] + u[1] * u[1] + 1.0);
  out[0] = u[0] / n; out[1] = u[1] / n; out[2] = 1.0 / n;
}
DEVFN void rot_inv(const Pose& T, const double p[3], double o[3]) {             // R^T p
  o[0] = T.R[0] * p[0] + T.R[3] * p[1] + T.R[6] * p[2];
  o[1] = T.R[1] * p[0] + T.R[4] * p[1] + T.R[7] * p[2];
  o[2] = T.R[2] * p[0] + T.R[5] * p[1] + T.R[8] * p[2];
}

// The geometry of AddPointEpipolar's search line, jni/MapMaker.cc:544-591: the candidate at level position (irx, iry) of level
// nLevel in the source keyframe, its ray between the depths the scene allows, seen in the target keyframe's z = 1 plane.
// why: 0 the line stands, 1 the ray ends before it starts or behind the target (:559-563), 2 a segment shorter than 1e-4
// (:575-576), 3 the line passes outside largest_radius (:582-583).  clipped: the start of the ray lay behind the target's image
// plane and was moved to 0.001 in front of it (:565-568).  startZ, endZ, alongSq: what the first three tests look at
// (v3RayStart_TC[2] before the clip, v3RayEnd_TC[2], the squared length), for the probe; k_epipolar reads none of
// them.  A field an exit does not reach stays 0 (along holds the
// un-normalised difference at exit 2).  k_epipolar and vslam_eval_epipolar run this; oracle/mapgrow.cpp epipolar_line states
// it for the host, statement for statement.
struct EpiLine { int why, clipped; double root[2], along[2], normal[2], dNormDist, dMinLen, dMaxLen, startZ, endZ, alongSq; };

DEVFN EpiLine epipolar_line(const Pose& Tsrc, const Pose& Ttgt, const CamModel& cam, double irx, double iry, int nLevel, double dMean, double dSigma,
                            double wiggle_scale) {
  EpiLine e;
  e.why = 0; e.clipped = 0; e.along[0] = 0; e.along[1] = 0; e.normal[0] = 0; e.normal[1] = 0; e.dNormDist = 0; e.dMinLen = 0; e.dMaxLen = 0; e.alongSq = 0;
  e.root[0] = level_zero_pos(irx, nLevel); e.root[1] = level_zero_pos(iry, nLevel);
  double ray[3], tmp[3], dirn[3];
  unit_ray(cam, e.root[0], e.root[1], ray);
  rot_inv(Tsrc, ray, tmp);
  pose_rot(Ttgt, tmp, dirn);
  const double dStartDepth = wiggle_scale > dMean - dSigma ? wiggle_scale : dMean - dSigma;
  const double dEndDepth = 40 * wiggle_scale < dMean + dSigma ? 40 * wiggle_scale : dMean + dSigma;
  const Pose srcInv = pose_inverse(Tsrc);
  double centre[3];
  pose_xform(Ttgt, srcInv.t, centre);
  double rs[3], re[3];
  for (int i = 0; i < 3; i++) { rs[i] = centre[i] + dStartDepth * dirn[i]; re[i] = centre[i] + dEndDepth * dirn[i]; }
  e.startZ = rs[2]; e.endZ = re[2];
  if (re[2] <= rs[2]) { e.why = 1; return e; }
  if (re[2] <= 0.0) { e.why = 1; return e; }
  if (rs[2] <= 0.0) { e.clipped = 1; const double f = 0.001 - rs[2] / dirn[2]; for (int i = 0; i < 3; i++) rs[i] += dirn[i] * f; }
  const double v2A[2] = {rs[0] / rs[2], rs[1] / rs[2]}, v2B[2] = {re[0] / re[2], re[1] / re[2]};
  e.along[0] = v2A[0] - v2B[0]; e.along[1] = v2A[1] - v2B[1];
  e.alongSq = e.along[0] * e.along[0] + e.along[1] * e.along[1];
  if (e.along[0] * e.along[0] + e.along[1] * e.along[1] < 0.00000001) { e.why = 2; return e; }
  const double n = sqrt(e.along[0] * e.along[0] + e.along[1] * e.along[1]);
  e.along[0] /= n; e.along[1] /= n;
  e.normal[0] = e.along[1]; e.normal[1] = -e.along[0];
  e.dNormDist = v2A[0] * e.normal[0] + v2A[1] * e.normal[1];
  if (fabs(e.dNormDist) > cam.largest_radius) { e.why = 3; return e; }
  const double la = e.along[0] * v2A[0] + e.along[1] * v2A[1], lb = e.along[0] * v2B[0] + e.along[1] * v2B[1];
  e.dMinLen = (la < lb ? la : lb) - 0.05; e.dMaxLen = (la > lb ? la : lb) + 0.05;
  if (e.dMinLen < -2.0) e.dMinLen = -2.0;
  if (e.dMaxLen < -2.0) e.dMaxLen = -2.0;
  if (e.dMinLen > 2.0) e.dMinLen = 2.0;
  if (e.dMaxLen > 2.0) e.dMaxLen = 2.0;
  return e;
}

