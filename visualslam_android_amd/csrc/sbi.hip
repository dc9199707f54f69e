// SmallBlurryImage and the rotation prior of the motion model, one workgroup per stream on the
// front-end stream, one frame ahead of the tracker:
//   SmallBlurryImage::MakeFromKF (jni/SmallBlurryImage.cc:20-55)  level 3 -> half size, zero mean, 9x9 Gaussian sigma 0.75
//   MakeJacs (:58-79)                                              central differences of the template
//   IteratePosRelToTarget (:98-222)                                6 ESM iterations aligning this frame's SBI to the last one's
//   SE3fromSE2 (:249-333) + Tracker::CalcSBIRotation (jni/Tracker.cc:885-893)   -> mv6SBIRot, read by k_motion (ApplyMotionModel)
// cv::resize / cv::GaussianBlur / Eigen's 4x4 inverse are third-party arithmetic, restated exactly as in oracle/sbi.cpp
// (same float expressions in the same order).  The whole stage is bit-exact with the oracle: the sample positions of
// transform_image are accumulated pixel by pixel by two lanes, and the fifteen ESM sums are taken in the reference's
// column-major order by fifteen lanes of wave 0 from per-pixel records the other threads stage in LDS.
#include "sbi_dev.h"

struct SbiArgs {
  const uint8_t* l3; size_t l3_sstride; int l3_pitch, w3, h3;
  uint8_t* small; float* tmpl; float* jacs; double* rot;          // this frame
  const float* last_tmpl; const float* last_jacs;                 // previous frame (== this frame's on the very first frame)
  SbiBlur blur;                                                   // cv::getGaussianKernel(9, 0.75, CV_32F)
  CamModel cam;                                                   // the camera at the small image's size (SE3fromSE2 :254)
  const int* list;                                                // subset step: workgroup -> stream (null: the identity)
  const unsigned char* held;                                      // subset step: the step's mask (null: a full step)
};

// The stages themselves are the device functions of sbi_dev.h, which the relocaliser (reloc.hip) runs on other images.
// RESTART: only the streams flagged in `restart` (vslam_reset_streams), which then lose their flag.
template <bool RESTART>
DEVFN void sbi_frame(const SbiArgs& a, unsigned char* restart) {
  extern __shared__ double sbi_dyn[];
  __shared__ SbiShared sh;
  const int s = (!RESTART && a.list) ? a.list[blockIdx.x] : (int)blockIdx.x, tid = threadIdx.x;
  if (RESTART && (!restart[s] || !trk_in_step(a.held, s))) return;   // a held stream keeps its flag for its own next frame
  const int W = a.w3 / 2, H = a.h3 / 2, N = W * H;
  float* t0 = (float*)sbi_dyn;           // zero-mean small image, later the warped template
  float* t1 = t0 + N;                    // row pass, later this frame's template
  double* wk = sbi_dyn + (2 * N + 1) / 2;   // sample positions [N][2], then the records [2][SBI_CHUNK][SBI_REC]
  const uint8_t* l3 = a.l3 + (size_t)s * a.l3_sstride;
  float* jacs = a.jacs + (size_t)s * N * 2;
  sbi_make_from_l3<4>(l3, a.l3_pitch, W, H, a.blur.k, t0, t1, a.small + (size_t)s * N, a.tmpl + (size_t)s * N, sh);
  sbi_make_jacs(t1, W, H, jacs);          // of this frame's template (it is the "last frame" of the next call)
  // on the first frame "last" is this frame itself (jni/Tracker.cc:90-92): wait for our own stores
  __threadfence();
  __syncthreads();
  Se2 CtoC; double final_score;
  sbi_iterate_pos_rel_to_target(t0, t1, wk, a.last_tmpl + (size_t)s * N, a.last_jacs + (size_t)s * N * 2, W, H, sh, CtoC, final_score);
  if (tid != 0) return;
  const Pose so3 = sbi_se3_from_se2(CtoC, a.cam, W, H);              // + ln: Tracker::CalcSBIRotation
  double out6[6];
  se3_ln(so3, out6);
  double* rot = a.rot + (size_t)s * 8;
  for (int i = 0; i < 6; i++) rot[i] = out6[i];
  rot[6] = final_score; rot[7] = 0.0;
  if (RESTART) restart[s] = 0;
}
__global__ __launch_bounds__(SBI_THREADS) void k_sbi(SbiArgs a) { sbi_frame<false>(a, nullptr); }
// A stream vslam_reset_streams has reset starts a new video: its next frame is a first frame, both SmallBlurryImages made from it
// (jni/Tracker.cc:90-92).  Launched behind k_sbi in that one frame only, for those streams only.
__global__ __launch_bounds__(SBI_THREADS) void k_sbi_restart(SbiArgs a, unsigned char* restart) { sbi_frame<true>(a, restart); }

// Subset step: the SmallBlurryImage products live in the frame's buffer, and the next frame of a stream aligns to "the other buffer".
// A held stream's products therefore move along, from the last step's buffer into this one, so that its rotation prior aligns to its
// own last frame whenever it resumes (and vslam_read_sbi and a snapshot keep finding them).  One workgroup per stream.
struct SbiCarryArgs {
  const uint8_t* small0; const float* tmpl0; const float* jacs0; const double* rot0;   // the last step's buffer
  uint8_t* small1; float* tmpl1; float* jacs1; double* rot1;                           // this step's
  const unsigned char* held; int N;
};
__global__ __launch_bounds__(SBI_THREADS) void k_sbi_carry(SbiCarryArgs a) {
  const int s = blockIdx.x;
  if (!a.held[s]) return;
  const size_t o = (size_t)s * a.N;
  for (int i = threadIdx.x; i < a.N; i += SBI_THREADS) {
    a.small1[o + i] = a.small0[o + i];
    a.tmpl1[o + i] = a.tmpl0[o + i];
    a.jacs1[2 * (o + i)] = a.jacs0[2 * (o + i)]; a.jacs1[2 * (o + i) + 1] = a.jacs0[2 * (o + i) + 1];
  }
  if (threadIdx.x < 8) a.rot1[(size_t)s * 8 + threadIdx.x] = a.rot0[(size_t)s * 8 + threadIdx.x];
}

static int sbi_args(vslam_system* sys, const FrameDev& last, SbiArgs& a, size_t& lds) {
  const LevelGeom& g3 = sys->geom[3];
  const int W = g3.w / 2, H = g3.h / 2;
  if (W * H > SBI_MAX_PIX || H > SBI_THREADS) { vslam_set_error("use_sbi: small image %d x %d exceeds %d pixels", W, H, SBI_MAX_PIX); return VSLAM_E_INVALID; }
  a.l3 = sys->fr.img[3]; a.l3_sstride = sys->fr.img_sstride[3]; a.l3_pitch = sys->fr.img_pitch[3]; a.w3 = g3.w; a.h3 = g3.h;
  a.small = sys->fr.sbi_small; a.tmpl = sys->fr.sbi_tmpl; a.jacs = sys->fr.sbi_jacs; a.rot = sys->fr.sbi_rot;
  a.last_tmpl = last.sbi_tmpl; a.last_jacs = last.sbi_jacs;
  sbi_blur_fill(a.blur, 0.75);                                       // gvdSBIBlur, jni/Tracker.cc:87
  cam_fill(a.cam, sys->p.cam, W, H, sys->p.quirks);
  lds = sbi_lds_bytes(W * H);
  a.list = nullptr; a.held = sys->fe_held;
  return VSLAM_OK;
}

int fe_sbi(vslam_system* sys, const FrameDev& last, const int* list, int n) {
  SbiArgs a; size_t lds;
  int r = sbi_args(sys, last, a, lds); if (r) return r;
  a.list = list;
  if (lds > 48 * 1024) HIPCHK(hipFuncSetAttribute((const void*)k_sbi, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(k_sbi, dim3(n), dim3(SBI_THREADS), lds, sys->fe_stream, a);
  HIPCHK(hipGetLastError());
  return VSLAM_OK;
}

int fe_sbi_carry(vslam_system* sys, const FrameDev& last) {
  SbiCarryArgs a;
  a.small0 = last.sbi_small; a.tmpl0 = last.sbi_tmpl; a.jacs0 = last.sbi_jacs; a.rot0 = last.sbi_rot;
  a.small1 = sys->fr.sbi_small; a.tmpl1 = sys->fr.sbi_tmpl; a.jacs1 = sys->fr.sbi_jacs; a.rot1 = sys->fr.sbi_rot;
  a.held = sys->fr.held; a.N = (sys->geom[3].w / 2) * (sys->geom[3].h / 2);
  hipLaunchKernelGGL(k_sbi_carry, dim3(sys->S), dim3(SBI_THREADS), 0, sys->fe_stream, a);
  HIPCHK(hipGetLastError());
  return VSLAM_OK;
}

int fe_sbi_restart(vslam_system* sys) {
  SbiArgs a; size_t lds;
  int r = sbi_args(sys, sys->fr, a, lds); if (r) return r;
  if (lds > 48 * 1024) HIPCHK(hipFuncSetAttribute((const void*)k_sbi_restart, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(k_sbi_restart, dim3(sys->S), dim3(SBI_THREADS), lds, sys->fe_stream, a, sys->sbi_restart);
  HIPCHK(hipGetLastError());
  return VSLAM_OK;
}
