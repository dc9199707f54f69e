// Similarity transform of a stream's map, the rule stated once: MapMaker::ApplyGlobalScaleToMap(s) followed by
// MapMaker::ApplyGlobalTransformationToMap(T) (jni/MapMaker.cc:440-464), x' = R (s x) + t with T = (R, t) mapping the old world frame
// to the new one and s > 0.  Host and device code: the kernel (transform.hip), the library's host code and host-side checks include
// this one header; tests/transform_ref.py restates it in numpy.  It builds only on pose_xform, pose_rot, pose_mul and pose_inverse of
// dev_math.h: their expression order is the contract (the library is built with -ffp-contract=off, so no multiply and add fuse).
//
//   MapPointDev::pos                        q = pos * s per component, then pose_xform(T, q)
//   MapPointDev::right, down                q = v * s, then pose_rot(T, q)
//   kf_pose[k], TrackerState::pose_final / start_pose / pose_cur, RelocInfo::best_pose
//                                           C.t *= s, then pose_mul(C, Tinv), Tinv = pose_inverse(T) once per stream
//   TrackerState::velocity[0..2]            *= s (the motion is in the camera frame: T does not enter; the rotational half stays)
//   TrackerState::depth_mean, depth_sigma, kf_depth[k][0..1], TrackData::cam[0..2]     *= s
//   everything else                         untouched, bit for bit
// TrackData::cam is the only per-point tracker field that holds a length: image, vfound and the derivatives are pixels and pixels per
// unit of the z = 1 plane, the warp matrices are ratios of pixel vectors to depth, the rest is counts and sums of grey values.
// wiggle_depth_norm and msd_vel are normalised by the scene depth and so carry no scale.
//
// Two choices are deliberate.  The pixel vectors are rotated and scaled, not remade by RefreshPixelVectors: for vectors that function
// made the result is the same up to rounding (it commutes with a similarity), and a map uploaded through vslam_map_add_point(s)
// carries the caller's own vectors, which remaking would change.  The depths are multiplied, not recomputed by RefreshSceneDepth:
// with s == 1.0 every `*= s` is exact, so a pure rigid move leaves velocity, depths and TrackData::cam bitwise alone.
//
// Two things in the reference read wiggle_scale as an absolute length: IsDistanceToNearestKeyFrameExcessive (jni/MapMaker.cc:1098-1101)
// and the start depth of AddPointEpipolar.  They do not follow a rescale; that is the reference's own behaviour and nothing here
// compensates for it.  Two more constants are absolute lengths in the same way, with a smaller effect: Bundle::Compute ends when the
// squared length of its update falls below ba_convergence_limit (so a rescaled map may be adjusted in a different number of trials), and
// the tracker's pose update adds wls_prior to the translational diagonal as well (a difference of 1e-10 in the pose at s = 2.5).
#pragma once
#include "dev_math.h"

struct Similarity { Pose T, Tinv; double s; };     // what one stream's call carries

HDFN Similarity sim_make(const Pose& T, double s) { Similarity g; g.T = T; g.Tinv = pose_inverse(T); g.s = s; return g; }

HDFN void sim_point(const Similarity& g, const double p[3], double o[3]) {          // a world position
  const double q[3] = {p[0] * g.s, p[1] * g.s, p[2] * g.s};
  pose_xform(g.T, q, o);
}
HDFN void sim_vector(const Similarity& g, const double v[3], double o[3]) {         // a world direction that carries a length
  const double q[3] = {v[0] * g.s, v[1] * g.s, v[2] * g.s};
  pose_rot(g.T, q, o);
}
HDFN Pose sim_pose(const Similarity& g, const Pose& C) {                            // a camera-from-world pose
  Pose c = C;
  c.t[0] *= g.s; c.t[1] *= g.s; c.t[2] *= g.s;
  return pose_mul(c, g.Tinv);
}
HDFN double sim_length(const Similarity& g, double x) { return x * g.s; }           // a length in a camera frame

// The accumulated similarity from a stream's original gauge (vslam_get_transform_info): `next` applied after `acc`,
// R' = R R_acc, t' = s R t_acc + t, s' = s s_acc.
HDFN void sim_compose(const Pose& T, double s, Pose& accT, double& accs) {
  Pose a = accT;
  a.t[0] *= s; a.t[1] *= s; a.t[2] *= s;
  accT = pose_mul(T, a);
  accs = s * accs;
}

// The host's gate on a caller's rotation: max |R^T R - I| and det R
HDFN void sim_rotation_defect(const double R[9], double& ortho, double& det) {
  ortho = 0.0;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      const double d = (R[0 * 3 + i] * R[0 * 3 + j] + R[1 * 3 + i] * R[1 * 3 + j] + R[2 * 3 + i] * R[2 * 3 + j]) - (i == j ? 1.0 : 0.0);
      const double a = d < 0 ? -d : d;
      ortho = a > ortho ? a : ortho;
    }
  det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
}
#define SIM_ROTATION_TOL 1e-9
