// The relocaliser (vslam_params.relocalise): a stream that has lost tracking finds its way back into its map from the
// SmallBlurryImages of the map's keyframes.
//   KeyFrame::MakeKeyFrame_Rest (jni/KeyFrame.cc:97-100)     every keyframe gets a SmallBlurryImage and its gradient image: k_kf_sbi
//   Relocaliser::AttemptRecovery (jni/Relocaliser.cc:17-42)  k_recover, one workgroup per stream, lost streams only:
//     kCurrent.pSBI->MakeFromKF(kCurrent)                    the frame's SBI at reloc_blur (the default 2.5 takes the 17 x 17 branch)
//     ScoreKFs (:46-58)                                      ZMSSD (jni/SmallBlurryImage.cc:82-94) against every keyframe, first strict minimum
//     IteratePosRelToTarget(best, 6), SE3fromSE2             mse3Best = SE3fromSE2(mse2) * se3CfromW(best)
//   Tracker::AttemptRecovery (jni/Tracker.cc:163-175)        score < 9e6: pose = start pose = mse3Best, velocity 0, mbJustRecoveredSoUseCoarse
// The image arithmetic is that of sbi_dev.h, shared with the tracker's frame SBI (k_sbi); a ZMSSD is summed by one lane in the
// reference's order (columns outer, rows inner), four keyframes at a time from templates staged in LDS.
#include "sbi_dev.h"

#define RELOC_MAX_SCORE 9e6        // jni/Relocaliser.cc:37
#define RELOC_KF_PER_ROUND 4       // keyframe templates staged per round: 4 N floats fit the 2 N doubles of the ESM's working area

struct KfSbiArgs {
  const uint8_t* kf_l3; size_t kf_stride; int kf_pitch, w3, h3;     // MapDev::kf_img[3]
  int K;                                                            // max_keyframes
  int stream, first;                                                // stream < 0: every stream with kf_pending, its slot n_kf; else keyframe first + blockIdx.x of `stream`
  SbiBlur blur;
  RelocDev r;
};

// SmallBlurryImage(kf) + MakeJacs of a stored keyframe, from the keyframe slot's level-3 image
__global__ __launch_bounds__(SBI_THREADS) void k_kf_sbi(MapDev m, KfSbiArgs a) {
  extern __shared__ double sbi_dyn[];
  __shared__ SbiShared sh;
  int s = a.stream, k = a.first + blockIdx.x;
  if (s < 0) {
    s = blockIdx.x;
    const TrackerState* st = &m.st[s];
    if (!trk_kf_pending(m.held, s, st)) return;
    k = st->n_kf;                                                   // the slot k_add_keyframe has just filled (n_kf advances in k_ba_select)
  }
  if (k < 0 || k >= a.K) return;
  const int W = a.w3 / 2, H = a.h3 / 2, N = W * H;
  float* t0 = (float*)sbi_dyn;
  float* t1 = t0 + N;
  const size_t slot = (size_t)s * a.K + k;
  sbi_make_from_l3(a.blur, a.kf_l3 + slot * a.kf_stride, a.kf_pitch, W, H, t0, t1, nullptr, a.r.kf_tmpl + slot * N, sh);
  sbi_make_jacs(t1, W, H, a.r.kf_jacs + slot * N * 2);
}

struct RecoverArgs {
  const uint8_t* l3; size_t l3_sstride; int l3_pitch, w3, h3;       // the current frame's level 3
  int K;
  SbiBlur blur;
  CamModel cam;                                                     // the camera at the small image's size (SE3fromSE2 :254)
  RelocDev r;
};

__global__ __launch_bounds__(SBI_THREADS) void k_recover(MapDev m, RecoverArgs a) {
  extern __shared__ double sbi_dyn[];
  __shared__ SbiShared sh;
  __shared__ int sh_best;
  const int s = blockIdx.x, tid = threadIdx.x;
  if (!trk_in_step(m.held, s)) return;                              // a held stream makes no attempt and keeps recovered_now
  TrackerState* st = &m.st[s];
  const bool lost = st->map_good && st->lost_frames >= 3;           // jni/Tracker.cc:103-104, 133
  const int nk = min(st->n_kf, a.K);
  if (tid == 0) st->recovered_now = 0;
  if (!lost || nk < 1) return;
  const int W = a.w3 / 2, H = a.h3 / 2, N = W * H;
  float* t0 = (float*)sbi_dyn;
  float* t1 = t0 + N;                                               // kCurrent.pSBI->mimTemplate
  double* wk = sbi_dyn + (2 * N + 1) / 2;
  RelocInfo* ri = a.r.info + s;
  double* scores = a.r.scores + (size_t)s * a.K;
  sbi_make_from_l3(a.blur, a.l3 + (size_t)s * a.l3_sstride, a.l3_pitch, W, H, t0, t1, nullptr, a.r.cur_tmpl + (size_t)s * N, sh);
  // ---- ScoreKFs: the keyframe templates come in once, coalesced, and are laid down in the order the sum walks them ----
  float* stage = (float*)wk;                                        // [RELOC_KF_PER_ROUND][N], column-major
  for (int k0 = 0; k0 < nk; k0 += RELOC_KF_PER_ROUND) {
    const int nr = min(RELOC_KF_PER_ROUND, nk - k0);
    for (int g = 0; g < nr; g++) {
      const float* kt = a.r.kf_tmpl + ((size_t)s * a.K + k0 + g) * N;
      for (int i = tid; i < N; i += SBI_THREADS) { const int y = i / W, x = i - y * W; stage[g * N + x * H + y] = kt[i]; }
    }
    __syncthreads();
    if (tid < nr) {                                                 // SmallBlurryImage::ZMSSD: the difference in float, squared and summed in double
      const float* kt = stage + tid * N;
      double dSSD = 0.0;
      int q = 0;
      for (int x = 0; x < W; x++)
        for (int y = 0; y < H; y++, q++) {
          const double dDiff = t1[y * W + x] - kt[q];
          dSSD += dDiff * dDiff;
        }
      scores[k0 + tid] = dSSD;
    }
    __syncthreads();
  }
  __threadfence();
  __syncthreads();
  if (tid == 0) {
    double best_score = 99999999999999.9;                           // jni/Relocaliser.cc:48-57
    int best = -1;
    for (int k = 0; k < nk; k++) { const double d = scores[k]; if (d < best_score) { best_score = d; best = k; } }
    sh_best = best;
    ri->attempts++; ri->best = best; ri->frame = st->frame + 1;     // mnFrame++ comes before the attempt (jni/Tracker.cc:100)
    ri->best_zmssd = best_score;
  }
  __syncthreads();
  const int best = sh_best;
  if (best < 0) return;                                             // no keyframe scored under the initial bound: nothing to align to
  Se2 CtoC; double score;
  const size_t slot = (size_t)s * a.K + best;
  sbi_iterate_pos_rel_to_target(t0, t1, wk, a.r.kf_tmpl + slot * N, a.r.kf_jacs + slot * N * 2, W, H, sh, CtoC, score);
  if (tid != 0) return;
  const Pose adj = sbi_se3_from_se2(CtoC, a.cam, W, H);
  const Pose best_pose = pose_mul(adj, m.kf_pose[slot]);            // :33-34
  se3_ln(adj, ri->ln_adj);
  ri->score = score; ri->best_pose = best_pose;
  if (score < RELOC_MAX_SCORE) {                                    // :37-41, then Tracker::AttemptRecovery, jni/Tracker.cc:169-174
    ri->successes++;
    st->pose_final = best_pose; st->pose_cur = best_pose; st->start_pose = best_pose;
    for (int i = 0; i < 6; i++) st->velocity[i] = 0.0;
    st->just_recovered = 1;
    st->recovered_now = 1;
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------
static size_t small_pixels(const vslam_system* sys) { return (size_t)(sys->geom[3].w / 2) * (sys->geom[3].h / 2); }

int reloc_alloc(vslam_system* sys) {
  if (!sys->p.relocalise) return VSLAM_OK;
  const size_t S = sys->S, K = sys->p.max_keyframes, N = small_pixels(sys);
  if (N > SBI_MAX_PIX) { vslam_set_error("relocalise: small image of %d pixels exceeds %d", (int)N, SBI_MAX_PIX); return VSLAM_E_INVALID; }
  DevOwner& own = sys->own; hipStream_t q = sys->stream;
  VCHK(own.alloc(&sys->reloc.kf_tmpl, S * K * N, q)); VCHK(own.alloc(&sys->reloc.kf_jacs, S * K * N * 2, q));
  VCHK(own.alloc(&sys->reloc.cur_tmpl, S * N, q)); VCHK(own.alloc(&sys->reloc.scores, S * K, q)); VCHK(own.alloc(&sys->reloc.info, S, q));
  return VSLAM_OK;
}

static int launch_kf_sbi(vslam_system* sys, int s, int first, int n) {
  const LevelGeom& g3 = sys->geom[3];
  KfSbiArgs a;
  a.kf_l3 = sys->map.kf_img[3]; a.kf_stride = (size_t)g3.pitch * g3.h; a.kf_pitch = g3.pitch; a.w3 = g3.w; a.h3 = g3.h;
  a.K = sys->p.max_keyframes; a.stream = s; a.first = first;
  sbi_blur_fill(a.blur, sys->p.reloc_blur);
  a.r = sys->reloc;
  const size_t lds = (small_pixels(sys) * 2 * sizeof(float) + 7) & ~(size_t)7;
  hipLaunchKernelGGL(k_kf_sbi, dim3(n), dim3(SBI_THREADS), lds, sys->stream, sys->map, a);
  HIPCHK(hipGetLastError());
  return VSLAM_OK;
}

int reloc_keyframe_sbi_pending(vslam_system* sys) { return sys->p.relocalise ? launch_kf_sbi(sys, -1, 0, sys->S) : VSLAM_OK; }
int reloc_keyframe_sbi(vslam_system* sys, int s, int first, int n) { return sys->p.relocalise && n > 0 ? launch_kf_sbi(sys, s, first, n) : VSLAM_OK; }

int reloc_attempt_recovery(vslam_system* sys) {
  if (!sys->p.relocalise) return VSLAM_OK;
  const LevelGeom& g3 = sys->geom[3];
  const int W = g3.w / 2, H = g3.h / 2;
  RecoverArgs a;
  a.l3 = sys->fr.img[3]; a.l3_sstride = sys->fr.img_sstride[3]; a.l3_pitch = sys->fr.img_pitch[3]; a.w3 = g3.w; a.h3 = g3.h;
  a.K = sys->p.max_keyframes;
  sbi_blur_fill(a.blur, sys->p.reloc_blur);
  cam_fill(a.cam, sys->p.cam, W, H, sys->p.quirks);
  a.r = sys->reloc;
  const size_t lds = sbi_lds_bytes(W * H);
  if (lds > 48 * 1024) HIPCHK(hipFuncSetAttribute((const void*)k_recover, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(k_recover, dim3(sys->S), dim3(SBI_THREADS), lds, sys->stream, sys->map, a);
  HIPCHK(hipGetLastError());
  return VSLAM_OK;
}

// ---- C ABI ----------------------------------------------------------------------------------------------------------
extern "C" int vslam_attempt_recovery(vslam_system* sys) {
  if (!sys) { vslam_set_error("attempt_recovery: null system"); return VSLAM_E_INVALID; }
  if (!sys->p.relocalise) return VSLAM_OK;
  if (!sys->have_frame) { vslam_set_error("attempt_recovery: no current frame (vslam_make_keyframe_lite first)"); return VSLAM_E_STATE; }
  if (sys->frame_open) { vslam_set_error("attempt_recovery: the frame's tracking has started (call it before vslam_patch_search(sys, 0))"); return VSLAM_E_STATE; }
  return reloc_attempt_recovery(sys);
}

static int reloc_check(vslam_system* sys, int stream, const char* who) {
  if (!sys || stream < 0 || stream >= sys->S) { vslam_set_error("%s: bad system/stream", who); return VSLAM_E_INVALID; }
  if (!sys->p.relocalise) { vslam_set_error("%s: created with relocalise = 0", who); return VSLAM_E_STATE; }
  return VSLAM_OK;
}

extern "C" int vslam_read_keyframe_sbi(vslam_system* sys, int stream, int keyframe, float* tmpl, float* jacs) {
  int r = reloc_check(sys, stream, "read_keyframe_sbi"); if (r) return r;
  int nk = 0;
  HostCopy c(sys->stream);
  VCHK(c.get(&nk, &sys->map.st[stream].n_kf)); VCHK(c.wait());
  if (keyframe < 0 || keyframe >= nk) { vslam_set_error("read_keyframe_sbi: keyframe %d of %d", keyframe, nk); return VSLAM_E_INVALID; }
  const size_t N = small_pixels(sys), slot = (size_t)stream * sys->p.max_keyframes + keyframe;
  if (tmpl) VCHK(c.get(tmpl, sys->reloc.kf_tmpl + slot * N, N));
  if (jacs) VCHK(c.get(jacs, sys->reloc.kf_jacs + slot * N * 2, N * 2));
  return c.wait();
}

extern "C" int vslam_get_reloc_info(vslam_system* sys, int stream, int out_i[4], double out_d[24]) {
  int r = reloc_check(sys, stream, "get_reloc_info"); if (r) return r;
  RelocInfo ri;
  VCHK(host_get(sys->stream, &ri, sys->reloc.info + stream));
  if (out_i) { out_i[0] = ri.attempts; out_i[1] = ri.successes; out_i[2] = ri.best; out_i[3] = ri.frame; }
  if (out_d) {
    out_d[0] = ri.best_zmssd; out_d[1] = ri.score;
    for (int i = 0; i < 6; i++) out_d[2 + i] = ri.ln_adj[i];
    pose_to12(ri.best_pose, out_d + 8);
    for (int i = 20; i < 24; i++) out_d[i] = 0.0;
  }
  return VSLAM_OK;
}

extern "C" int vslam_read_reloc_attempt(vslam_system* sys, int stream, float* cur_tmpl, double* zmssd, int cap) {
  int r = reloc_check(sys, stream, "read_reloc_attempt"); if (r) return r;
  RelocInfo ri;
  int nk = 0;
  HostCopy c(sys->stream);
  VCHK(c.get(&ri, sys->reloc.info + stream)); VCHK(c.get(&nk, &sys->map.st[stream].n_kf)); VCHK(c.wait());
  if (ri.attempts < 1) { vslam_set_error("read_reloc_attempt: the stream has not attempted a recovery"); return VSLAM_E_STATE; }
  const size_t N = small_pixels(sys);
  if (cur_tmpl) VCHK(c.get(cur_tmpl, sys->reloc.cur_tmpl + (size_t)stream * N, N));
  VCHK(c.take(zmssd, sys->reloc.scores + (size_t)stream * sys->p.max_keyframes, nk, cap)); VCHK(c.wait());
  return nk;
}
