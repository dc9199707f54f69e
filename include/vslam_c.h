/*
 * vslam_c.h -- C ABI of libvslam_hip.so: the MI355X (gfx950) implementation of the PTAM
 * tracking + local bundle-adjustment hot path of ahcorde/visualSLAM_Android.
 *
 * The only C ABI the reference has is its JNI surface (jni/jni_part.cpp:84-145):
 *   native_createTest / native_disposeTest / native_touchScreen / native_update(gray, rgba).
 * vslam_create / vslam_destroy / vslam_touch / vslam_update replace those one for one
 * (INTEGRATION.md shows the JNI stub that binds them).  The remaining entry points expose the
 * stages behind Tracker::TrackFrame (jni/Tracker.cc:76-146) and MapMaker::AddKeyFrame
 * (jni/MapMaker.cc:470-478) individually for parity tests and benchmarks; each cites the
 * reference function it replaces.
 *
 * Conventions: plain pointers and sizes only; every call returns 0 on success or a negative
 * VSLAM_E_* code (never aborts; the reference has no error convention, jni_part.cpp:144
 * returns constant 0).  One vslam_system holds n_streams independent sequences that are
 * processed in lock-step by batched kernels on one HIP stream; calls on one system must be
 * serialised by the caller, different systems are independent.  Inputs are borrowed for the
 * duration of the call; outputs go to caller-provided buffers.
 */
#ifndef VSLAM_C_H
#define VSLAM_C_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VSLAM_LEVELS 4 /* jni/KeyFrame.h:33 */

#define VSLAM_OK 0
#define VSLAM_E_INVALID (-1)  /* bad argument */
#define VSLAM_E_HIP (-2)      /* HIP runtime error, see vslam_last_error() */
#define VSLAM_E_CAPACITY (-3) /* a fixed-capacity device buffer overflowed */
#define VSLAM_E_STATE (-4)    /* call not valid in the current state */

/* reference-quirk switches. Default 0 = PTAM-intended semantics. */
#define VSLAM_Q_CAM_INT_RADIUS 1         /* jni/ATANCamera.cc:70-82  */
#define VSLAM_Q_POSE_INT_RESIDUAL 2      /* jni/Tracker.cc:766-767   */
#define VSLAM_Q_NONMAX_RIGHT_NEIGHBOUR 4 /* jni/vision/cvfast.cpp:9282-9285 */

typedef struct vslam_system vslam_system;

/* Every tunable the reference hard-codes on the hot path. */
typedef struct vslam_params {
  int width, height;               /* jni/jni_part.cpp:41 (800x480 there); 48..4096 each, any value, odd ones included */
  int n_streams;                   /* independent sequences batched on this GPU */
  int fast_threshold[VSLAM_LEVELS];/* jni/KeyFrame.cc:32-39: 10,15,15,10 */
  int nonmax_barrier;              /* jni/KeyFrame.cc:63: 10 */
  int patch_size;                  /* jni/PatchFinder.h:48: 11 (BASELINE configs: 8) */
  int max_corners[VSLAM_LEVELS];   /* device capacity per stream and level */
  int max_points;                  /* map-point capacity per stream */
  int max_keyframes;               /* keyframe capacity per stream */
  int max_patches_per_frame;       /* jni/Tracker.cc:518: 1000 */
  int coarse_min, coarse_max;      /* jni/Tracker.cc:405-406: 20, 60 */
  int coarse_range;                /* jni/Tracker.cc:407: 30 */
  int coarse_subpix_its;           /* jni/Tracker.cc:408: 8 */
  int coarse_disabled;             /* jni/Tracker.cc:409: 0 */
  double coarse_min_vel;           /* jni/Tracker.cc:410: 0.006 */
  int fine_subpix_its;             /* jni/Tracker.cc:505: 8 (level 3 only) */
  double wls_prior;                /* jni/Tracker.cc:734: 100 */
  int use_sbi;                     /* jni/Tracker.cc:88 gvnUseSBI (reference 1): SmallBlurryImage rotation prior in the motion model; default 0 */
  int min_frames_between_kf;       /* jni/Tracker.cc:128: 20 */
  double max_kf_dist_wiggle_mult;  /* jni/MapMaker.cc:768: 0.2 */
  double wiggle_scale;             /* jni/MapMaker.cc:57: 0.1 */
  int ba_max_iterations;           /* jni/Bundle.cc:65: 20 */
  double ba_convergence_limit;     /* jni/Bundle.cc:66: 1e-6 */
  double ba_min_tukey_sigma;       /* jni/Bundle.cc:224: 0.4 */
  int ba_window;                   /* jni/MapMaker.cc:812-820: newest + 4 nearest = 5 */
  int ba_min_keyframes;            /* jni/MapMaker.cc:803: 8 */
  double cam[5];                   /* jni/ATANCamera.cc:20-24 normalised fx fy cx cy w */
  int quirks;                      /* VSLAM_Q_* bit set */
  int device;                      /* HIP device ordinal */
  int ba_delay_frames;             /* 0: a keyframe's bundle adjustment is finished before the next frame (synchronous
                                      map-maker); D > 0: it runs on its own HIP stream beside the next frames and its results
                                      are applied at the start of the D-th following frame (the reference's map-maker is a
                                      second thread whose results also arrive "a few frames later", jni/MapMaker.cc:80-123) */
  int grow_map;                    /* bit flags, the rest of MapMaker::AddKeyFrameFromTopOfQueue (jni/MapMaker.cc:481-506) on every new keyframe:
                                      1: MakeKeyFrame_Rest's candidates, ThinCandidates and AddSomeMapPoints (epipolar search +
                                         triangulation, :498-501, 525-703), so the map gains points;
                                      2: ReFindInSingleKeyFrame (:497, 967-1056), so the keyframe also gains measurements of points the
                                         tracker did not measure in it;
                                      3: both, the reference's behaviour; 0 (default): only the tracker's measurements are stored */
  int ba_batch_frames;             /* asynchronous map-maker only (ba_delay_frames > 0): Bundle::Compute of the keyframes of this many consecutive
                                      frames is launched together (1 .. ba_delay_frames; 0 = 1).  Independent sequences ask for keyframes in
                                      different frames; one launch per frame would carry only a few problems.  Does not change any result: a
                                      keyframe's adjustment is still applied ba_delay_frames frames after the keyframe */
  int idle_iterations;             /* MapMaker::run's idle jobs (jni/MapMaker.cc:94-117) after every frame, this many passes: BundleAdjustRecent until it
                                      has converged, ReFindNewlyMade (:1061-1081), BundleAdjustAll until it has converged (:776-798), every 20th pass
                                      ReFindFromFailureQueue (:1083-1096; the reference draws rand() % 20), HandleBadPoints.  0 (default): one
                                      BundleAdjustRecent per keyframe only.  -1: none after a frame, but the failure queue and never-retry sets are kept so that
                                      vslam_mapmaker_idle_job can run the jobs on request.  Needs the synchronous map-maker (ba_delay_frames = 0) */
  int bootstrap;                   /* 1: a stream without a map runs Tracker::TrackForInitialMap (jni/Tracker.cc:247-288): vslam_press_spacebar starts the
                                      trails on the next frame, a second press runs MapMaker::InitFromStereo (HomographyInit, the stereo points,
                                      AddSomeMapPoints, BundleAdjustAll, CalcPlaneAligner) on the frame that consumes it.  Needs grow_map != 0
                                      (keyframe corner lists) and the synchronous map-maker for the streams being initialised.  0 (default): maps are uploaded */
  int ba_sum_order;                /* 0 (default): Bundle::Compute sums U, V, the reduced camera system and the objectives as parallel partial sums and
                                      matrix-core products (results within ~1e-10 of the reference's loops).  1: every sum in the order of the
                                      reference's loops (jni/Bundle.cc:241-321, 362-470, 537-561) -- same results as the reference's sequential
                                      code bit for bit, several times slower: the parity mode */
  int relocalise;                  /* 1: the relocaliser (jni/Relocaliser.cc, jni/Tracker.cc:133-139, 163-175): every keyframe keeps a SmallBlurryImage
                                      (jni/KeyFrame.cc:97-100; 12 * (width/16) * (height/16) bytes each, max_keyframes per stream) and a stream that has
                                      been lost for three frames attempts a recovery in every frame (vslam_attempt_recovery).  0 (default): a lost stream
                                      stays lost, no kernel is launched and nothing is allocated for it */
  double reloc_blur;               /* jni/SmallBlurryImage.h:19-20 dBlur of the relocaliser's images: 2.5.  <= 2: 9 x 9 Gaussian, > 2: 17 x 17
                                      (jni/SmallBlurryImage.cc:51-54) */
  unsigned pvs_shuffle_seed;       /* jni/Tracker.cc:396-397,525: TrackMap shuffles every level's list of the potentially visible set before the coarse
                                      selection, and the list of the remaining points before it cuts it to max_patches_per_frame, so that a map
                                      larger than the cap is measured all over and not at the head of its lists.  The reference draws from rand();
                                      here the order is the seeded permutation of csrc/pvs_perm.h, a function of (seed, frame, list, length).
                                      0 (default): the identity order, map order.  Non-zero: every stream starts with this seed
                                      (vslam_set_pvs_seed changes one stream's) */
  int overlay;                     /* 1: the system can draw what Tracker::TrackFrame draws on its colour frame (vslam_render_overlay below).  It keeps
                                      one int per stream, the mnFrame at which TrackMap last ran for it, written by one 64-lane launch in front of the
                                      motion model; every other read-back gives the bits it gives with 0.  0 (default): nothing is allocated, nothing
                                      is launched, vslam_render_overlay returns VSLAM_E_STATE.
                                      (It stands in front of keyframe_retire, which stays the struct's last member.) */
  int keyframe_retire;             /* What a stream does whose map holds max_keyframes keyframes when its tracker wants another one (NeedNewKeyFrame,
                                      jni/MapMaker.cc:761-773).  0 (default): nothing, the map stops growing (the reference's map has no limit,
                                      jni/Map.h:21-34).  1: it asks for the keyframe after all, and vslam_finish_frame / vslam_add_keyframe first
                                      retire one keyframe by policy (vslam_retire_keyframes below) into whose place the others move, so the new
                                      keyframe takes the last slot.  While an adjustment of the asynchronous map-maker is pending for the stream the
                                      request waits for a later frame.  No host synchronisation.  Needs max_keyframes >= 3 */
} vslam_params;

const char* vslam_last_error(void);
int vslam_default_params(vslam_params* p, int width, int height, int n_streams);

/* native_createTest / native_disposeTest (jni/jni_part.cpp:109-118) */
int vslam_create(const vslam_params* p, vslam_system** out);
int vslam_destroy(vslam_system* sys);
int vslam_synchronize(vslam_system* sys);
/* Self-test hook: the library's own transcendentals (csrc/vslam_libm.h -- the camera model's atan / tan, jni/ATANCamera.h:136-150,
 * and the sin / cos / asin / acos of SE3 exp and ln, jni/RT.h:134-214, 318-383) over n arguments, on the device or
 * (on_host != 0) as compiled for the host.  fn: 0 sin, 1 cos, 2 tan, 3 atan, 4 asin, 5 acos, 6 sqrt, 7 reciprocal.  Both sides
 * must return the same bits: one ulp of difference in a projection flips template pixels (jni/vision/ImageHandler.cpp:12-19). */
int vslam_eval_transcendental(int fn, int n, const double* x, double* y, int on_host);
/* Self-test hooks for two pieces of the tracker's pose iterations and the bundle adjustment, each run in one workgroup of the
 * size its kernel uses.
 * vslam_eval_select: the k-th smallest (0-based) of n non-negative doubles, as the Tukey median takes it (jni/MEstimator.h:67-77).
 *   form 0: the tracker's workgroup, values in on-chip memory (n <= 4096); form 1: the bundle adjustment's, values in device memory.
 *   +inf marks an entry that is not part of the median (k counts the others).
 * vslam_eval_pose_tail: the end of one pose iteration (jni/Tracker.cc:487 / :573) from the 27 sums of the normal equations (upper
 *   triangle of C row by row, then v): the solve of myWLS::compute (jni/myWLS.h:54-62; a singular C gives a zero update) and
 *   pose12_out = exp(update6) * pose12. */
int vslam_eval_select(int form, int n, const double* v, int k, double* out);
int vslam_eval_pose_tail(const double* sums27, const double* pose12, double* update6, double* pose12_out);
/* Self-test hook: the ATAN camera's arithmetic on its own (jni/ATANCamera.cc:31-91, 133-164, 198-231), as every projecting kernel reads
 * it, for the calibration cam5 (as vslam_params.cam) of a width x height image.  xy: n image-plane points (x, y).  out17 receives
 * 17 doubles per point: Project (im[2], r, factor, invalid as 0 / 1), GetProjectionDerivs [4] (row-major as stored: d00 d01 d10 d11),
 * UnProject(im) [2], and the bootstrap's UnProject + GetProjectionDerivs at im (position [2], derivatives [4]).  derived5 receives
 * what SetImageSize / RefreshParams / OnePixelDist derive: two_tan, winv, largest_radius, max_r, one_pixel_dist.  The points are
 * evaluated by one 64-lane workgroup on the device or (on_host != 0) by the same functions compiled for the host; both must return
 * the same bits. */
int vslam_eval_camera(const double* cam5, int width, int height, int quirks, int n, const double* xy, double* out17, double* derived5, int on_host);
/* Self-test hook: the line geometry of MapMaker::AddPointEpipolar (jni/MapMaker.cc:544-591) and the triangulation of
 * MapMaker::ReprojectPoint (:174-200) on their own, by the device functions the map-growth kernel runs, with the handle's camera
 * (vslam_params.cam, width, height, quirks) and on the handle's queue; one launch, one lane per case.
 * lines30: n_lines cases of 30 doubles -- the source keyframe's pose [12] (R row-major, then t), the target keyframe's [12], the
 *   candidate's level position x, y, its level (0..3), the source keyframe's scene depth mean and sigma, wiggle_scale.
 *   line_flags2 receives per case (why, clipped): why = 0 the line stands, 1 the ray ends before it starts or behind the target, 2 a
 *   segment shorter than 1e-4, 3 the line passes outside largest_radius; clipped = 1 if the start of the ray was moved in front of
 *   the target's image plane.  line_out12 receives root [2], along [2], normal [2], dNormDist, dMinLen, dMaxLen, and what the first
 *   three tests compare: the depth of the ray's start in the target before the clip, of its end, the squared length of the segment; a
 *   field an exit does not reach is 0 (along is the un-normalised difference at why = 2).
 * tri16: n_tri cases of 16 doubles -- AfromB [12], v2A [2], v2B [2].  tri_out7 receives the homogeneous vector of the smallest
 *   singular value [4] as the SVD returns it, and the point [3].
 * The oracle states both for the host (orc_eval_epipolar, orc_eval_triangulation); the two must return the same bits. */
int vslam_eval_epipolar(vslam_system* sys, int n_lines, const double* lines30, int* line_flags2, double* line_out12, int n_tri, const double* tri16, double* tri_out7);

/* ---- frame front-end ------------------------------------------------------------------- */

/* KeyFrame::MakeKeyFrame_Lite (jni/KeyFrame.cc:5-51) for all n_streams frames at once:
 * 4-level pyramid, FAST-10 per level, raster-ordered corner lists and row LUTs, all on device.
 * gray: n_streams images, image s at gray + s*stream_stride, rows row_stride bytes apart;
 * on_device != 0 means gray is device memory (borrowed until the next front-end call; with vslam_params.bootstrap until the
 * frame AFTER the next has been enqueued and this one's work has finished: the trail tracker reads the previous frame's level 0
 * in place, jni/Tracker.cc:294-346).  Asynchronous on the system's stream.
 * Any size vslam_create accepts and any alignment of gray, row_stride and stream_stride give the same bits; a width that is a multiple
 * of 32 (and at least 128, with a height of at least 56) read from 16-B aligned memory takes the faster of the two forms of the kernels. */
int vslam_make_keyframe_lite(vslam_system* sys, const uint8_t* gray, size_t row_stride,
                             size_t stream_stride, int on_device);

/* fast_nonmax (jni/vision/cvfast.cpp:9395-9400) on the current frame of every stream, all
 * levels: compute_fast_score_old + nonmax_suppression -> vMaxCorners. */
int vslam_fast_nonmax(vslam_system* sys);

/* read-back of the current frame (synchronises) */
int vslam_read_level_image(vslam_system* sys, int stream, int level, uint8_t* dst, size_t dst_stride);
int vslam_read_corners(vslam_system* sys, int stream, int level, uint32_t* corners /* x | y<<16 */,
                       int cap, int* n);
int vslam_read_row_lut(vslam_system* sys, int stream, int level, int* lut /* height>>level ints */);
int vslam_read_max_corners(vslam_system* sys, int stream, int level, uint32_t* corners, int* scores,
                           int cap, int* n);

/* KeyFrame::MakeKeyFrame_Rest (jni/KeyFrame.cc:53-95) for the current frame of every stream: fast_nonmax on the four levels,
 * then the candidate list -- maximal corners inside the 10-px border whose Shi-Tomasi score (half-window 3,
 * jni/vision/ImageHandler.cpp:124-155) exceeds min_shi_tomasi_score (reference: 70, :57).  The SmallBlurryImage part of the
 * function (:97-100) belongs to the relocaliser: with vslam_params.relocalise it is made when a frame becomes a keyframe
 * (vslam_read_keyframe_sbi), not here. */
int vslam_make_keyframe_rest(vslam_system* sys, double min_shi_tomasi_score);
/* MapMaker::ThinCandidates (jni/MapMaker.cc:393-422) on all four levels of the current candidate lists, against the
 * measurements of `keyframe` of each stream (keyframe < 0: the tracker's measurements of the current frame, i.e. what
 * MapMaker::AddKeyFrame copies into the new keyframe). */
int vslam_thin_candidates(vslam_system* sys, int keyframe);
/* Candidate::irLevelPos (packed x | y<<16) and dSTScore of one level, raster order; *n = count (may exceed cap).
 * After a keyframe with grow_map bit 0 the list is what ThinCandidates left, and a candidate AddPointEpipolar (jni/MapMaker.cc:525-703)
 * turned away has its score replaced by the negated stage at which it gave up: -1 the ray ends before it starts or behind the target
 * camera, -2 the epipolar line segment is shorter than 1e-4, -3 the line lies outside the camera's largest radius, -4 the template touches
 * the source level's border, -5 no target corner on the line scores below the limit, -6 the sub-pixel iterations did not converge,
 * -7 the map already holds max_points points (a limit of this build, not of PTAM; the remaining candidates are still looked at).  A
 * candidate that became a map point keeps its Shi-Tomasi score (> 0). */
int vslam_read_candidates(vslam_system* sys, int stream, int level, uint32_t* pos, double* score, int cap, int* n);
/* grow_map = 1: Level::vCorners (packed x | y << 16, raster order) of a stored keyframe -- the epipolar search's target list.
 * At most 16384 / 8192 / 4096 / 2048 corners per level are kept (a longer list is cut in raster order); *n = stored count. */
int vslam_get_keyframe_corners(vslam_system* sys, int stream, int keyframe, int level, uint32_t* corners, int cap, int* n);
/* use_sbi = 1: the SmallBlurryImage of the current frame (jni/SmallBlurryImage.cc:20-55: (w/16) x (h/16) u8 image and its
 * zero-mean blurred fp32 template) and rot8 = { mv6SBIRot[6] (jni/Tracker.cc:885-893), final ESM score, 0 }. */
int vslam_read_sbi(vslam_system* sys, int stream, uint8_t* small_img, float* tmpl, double rot8[8]);
/* relocalise = 1: KeyFrame::pSBI of a keyframe of the map (jni/KeyFrame.cc:97-100, jni/SmallBlurryImage.cc:20-79): mimTemplate
 * ((w/16) x (h/16) floats) and mimImageJacs (two floats per pixel).  Either pointer may be NULL.  VSLAM_E_STATE with relocalise = 0. */
int vslam_read_keyframe_sbi(vslam_system* sys, int stream, int keyframe, float* tmpl, float* jacs);
/* relocalise = 1: the relocaliser's members (jni/Relocaliser.h) for a stream.  out_i = AttemptRecovery calls so far, those that returned
 * true, mnBest and the frame number of the last call; out_d = mdBestScore (jni/Relocaliser.cc:46-58), the final score of
 * IteratePosRelToTarget (:29-31), ln of SE3fromSE2's result (6; the quantity vslam_read_sbi reports as rot8), mse3Best (:34) as R row-major
 * (9) + t (3), four zeros.  VSLAM_E_STATE with relocalise = 0. */
int vslam_get_reloc_info(vslam_system* sys, int stream, int out_i[4], double out_d[24]);
/* relocalise = 1: the images of the stream's last AttemptRecovery: kCurrent.pSBI->mimTemplate (jni/Relocaliser.cc:20-23) and the ZMSSD of
 * every keyframe ScoreKFs computed (:51-57; the first `cap`).  Returns the number of keyframes scored.  Either pointer may be NULL.
 * VSLAM_E_STATE with relocalise = 0 or before the first attempt. */
int vslam_read_reloc_attempt(vslam_system* sys, int stream, float* cur_tmpl, double* zmssd, int cap);

/* ---- MiniPatch (jni/MiniPatch.cc), the primitives of the reference's trail tracking ------------- */
/* MiniPatch::SampleFromImage (:71-83): 9x9 patches around n integer positions of the current frame's level 0
 * of `stream`; ok[i] = 0 where the patch would leave the image (the reference asserts). Synchronous. */
int vslam_minipatch_sample(vslam_system* sys, int stream, int n, const int* pos_xy, uint8_t* patches /* n*81 */, int* ok);
/* MiniPatch::FindPatch (:35-68): for each patch, best raw SSD at the FAST corners inside the +-range box around
 * pos_xy[i]; on success pos_xy[i] is replaced by the corner and found[i] = 1 (SSD < max_ssd, jni/Tracker.cc:226). */
int vslam_minipatch_find(vslam_system* sys, int stream, int n, const uint8_t* patches, int* pos_xy, int range, int max_ssd,
                         int* found);

/* ---- map (jni/Map.h:21-34) ---------------------------------------------------------------- */
/* The reference fills its map through InitFromStereo / AddPointEpipolar (bootstrap and map growth: out of
 * scope / "next" rows); the feeder supplies a ground-truth map through these instead. */

/* KeyFrame (jni/KeyFrame.h:73-97): pose12 = R row-major (9) + t (3), camera-from-world; gray is host memory.
 * Builds the keyframe's pyramid on device.  Returns the keyframe index (>= 0) or a negative error. */
int vslam_map_add_keyframe(vslam_system* sys, int stream, const double pose12[12], int fixed, const uint8_t* gray,
                           size_t row_stride, double depth_mean, double depth_sigma);
/* the same for n keyframes of the stream at once: pose12 n x 12, fixed n, gray n images image_stride bytes apart, depth_mean_sigma n x 2.
 * Returns the index of the first one. */
int vslam_map_add_keyframes(vslam_system* sys, int stream, int n, const double* pose12, const int* fixed, const uint8_t* gray, size_t row_stride,
                            size_t image_stride, const double* depth_mean_sigma);
/* MapPoint (jni/MapPoint.h:22-69). Returns the point index or a negative error. */
int vslam_map_add_point(vslam_system* sys, int stream, const double pos[3], int src_keyframe, int src_level,
                        int ir_x, int ir_y, const double pixel_right_w[3], const double pixel_down_w[3]);
/* the same for n points at once (pos, pixel_right_w, pixel_down_w: 3n doubles; ir_xy: 2n ints). Returns the new point count. */
int vslam_map_add_points(vslam_system* sys, int stream, int n, const double* pos, const int* src_keyframe, const int* src_level,
                         const int* ir_xy, const double* pixel_right_w, const double* pixel_down_w);
/* Measurement (jni/KeyFrame.h:46-51): source 0 TRACKER 1 REFIND 2 ROOT 3 TRAIL 4 EPIPOLAR */
int vslam_map_add_measurement(vslam_system* sys, int stream, int keyframe, int point, int level,
                              const double root_pos[2], int subpix, int source);
/* the same for n measurements at once (arrays of n; root_pos 2n doubles) */
int vslam_map_add_measurements(vslam_system* sys, int stream, int n, const int* keyframe, const int* point,
                               const int* level, const double* root_pos, const int* subpix, const int* source);
int vslam_map_set_good(vslam_system* sys, int stream);           /* Map::bGood (jni/Map.h:33) */
/* map editing after the upload (a host-side map-maker, a loaded map, tests that re-synchronise the map to a reference):
 * MapPoint::v3WorldPos of the points [first, first + n) (pos3: 3n doubles) and KeyFrame::se3CfromW of one keyframe */
int vslam_map_set_point_positions(vslam_system* sys, int stream, int first, int n, const double* pos3);
int vslam_map_set_keyframe_pose(vslam_system* sys, int stream, int keyframe, const double pose12[12]);
int vslam_set_pose(vslam_system* sys, int stream, const double pose12[12]);
int vslam_set_velocity(vslam_system* sys, int stream, const double v6[6]);
/* Tracker::mnLastKeyFrameDropped (jni/Tracker.h:118; -20 after Reset, jni/Tracker.cc:59): frame number of the stream's last keyframe;
 * the tracker asks for the next one more than min_frames_between_kf frames later (jni/Tracker.cc:128) */
int vslam_set_last_keyframe_dropped(vslam_system* sys, int stream, int frame);

/* Tracker::Reset (jni/Tracker.cc:45-70) with MapMaker::RequestReset / Reset (jni/MapMaker.cc:60-74, 127-136) and Map::Reset (jni/Map.cc:8-14)
 * for n streams of a live batch (streams == NULL: every stream): the map is dropped and the tracker returns to its constructed state --
 * quality GOOD, frame 0, no velocity, scene depth 1 / 1, mnLastKeyFrameDropped -20, mnInitialStage TRAIL_TRACKING_NOT_STARTED, no trails,
 * no pending spacebar, mbBundleConverged_Full / _Recent true, empty failure and new queues, every per-stream counter zero, the boot seed 1.
 * Afterwards each of these streams is a stream of a newly created system: every read-back, and every frame tracked after a new map has
 * been uploaded (vslam_map_add_*) or bootstrapped, gives the bits a new system gives; with use_sbi its next frame makes both
 * SmallBlurryImages from itself (jni/Tracker.cc:90-92).  An adjustment of the asynchronous map-maker that is pending for the stream is
 * abandoned (mbBundleAbortRequested, CHECK_RESET jni/MapMaker.cc:76-78): its result never reaches the map.  The other streams are not
 * touched.  Between frames only: VSLAM_E_STATE while a stage-wise frame is open; VSLAM_E_INVALID for an index outside the batch, and then
 * no stream is reset.  Ordered on the system's stream, asynchronous (MapMaker::ResetDone, jni/MapMaker.cc:133-136, has nothing to wait for). */
int vslam_reset_streams(vslam_system* sys, const int* streams, int n);
/* out[0..3] = Reset calls the stream has seen, mnFrame (jni/Tracker.h:116) at the last one, and the keyframes and map points
 * (jni/Map.h:29-30) that call dropped. */
int vslam_get_reset_info(vslam_system* sys, int stream, int out[4]);
/* HIP-event milliseconds of the last vslam_reset_streams on the system's stream: the flag copy, the wait for the map-maker streams
 * (asynchronous map-maker) and the reset kernels.  Synchronises.  VSLAM_E_STATE before the first call. */
int vslam_get_reset_timing(vslam_system* sys, double* ms);

/* ---- keyframe retirement ---------------------------------------------------------------------
 * One keyframe of each listed stream leaves its map, on the device and in place.  The reference has no such operation (its Map grows on
 * the heap, jni/Map.h:21-34, and nothing leaves vpKeyFrames): like max_points this is the build's own, for a stream that runs
 * indefinitely in bounded memory.  With keyframe r of stream streams[i] (keyframes[i]; < 0: by policy, the keyframe whose camera centre
 * is farthest from the stream's current pose, KeyFrameLinearDist jni/MapMaker.cc:705-712, lowest index on ties):
 *   - keyframe r leaves; the later keyframes move down one and keep their order of creation (the newest is still n_keyframes - 1);
 *   - the map points whose patch source it was (MapPoint::pPatchSourceKF, jni/MapPoint.h:36) leave with it, and so does every bad point;
 *     the survivors keep their relative order and are renumbered, in every per-point array, measurement row, never-retry set, the
 *     failure queue and the last frame's iteration set; pPatchSourceKF and the measurement-keyframe count of a survivor follow;
 *   - if r was the map's only fixed keyframe the oldest survivor becomes fixed (BundleAdjustAll keeps its gauge, jni/MapMaker.cc:776-798);
 *   - Relocaliser::mnBest (jni/Relocaliser.h) follows, -1 if it was r.
 * Between frames, on any system whatever its keyframe_retire.  Stream indices must be distinct.  The call waits once for the device to
 * read the listed streams' states; everything is decided before anything changes, and a refused call changes nothing for any stream.
 * VSLAM_E_INVALID: NULL system, n < 0, an index outside the batch, a duplicate stream, keyframes[i] >= the stream's keyframes.
 * VSLAM_E_STATE: a stage-wise frame is open; a listed stream has no good map, fewer than 3 keyframes (a map keeps at least two), its
 * trails running, or an adjustment of the asynchronous map-maker pending.  All listed streams go in one set of three launches. */
int vslam_retire_keyframes(vslam_system* sys, const int* streams, const int* keyframes, int n);
/* out[0..5] = retirements of the stream so far (explicit and automatic); of the last one: the index the keyframe had before it left, the
 * points dropped because it was their source, the bad points reclaimed, the failure-queue entries dropped, and mnFrame
 * (jni/Tracker.h:116) at that time.  vslam_reset_streams and vslam_restore_stream zero the record. */
int vslam_get_retire_info(vslam_system* sys, int stream, int out[6]);
/* HIP-event milliseconds of the last vslam_retire_keyframes that retired, its three launches on the system's stream.  Waits for them.
 * VSLAM_E_STATE before the first such call. */
int vslam_get_retire_timing(vslam_system* sys, double* ms);

/* ---- similarity transform of a map (re-anchor and rescale) -------------------------------------
 * MapMaker::ApplyGlobalScaleToMap + ApplyGlobalTransformationToMap (jni/MapMaker.cc:440-464) for n streams of a live batch, on the
 * device and in place: a monocular map has no gauge of its own, and this puts it into the caller's -- a site frame, a metric scale.
 * x' = R (s x) + t, with new_from_old12 = (R, t) (pose12: R row-major, then t) mapping the old world frame to the new one and s > 0
 * (scale == NULL: all 1).  Transform i belongs to streams[i]; streams == NULL: every stream, transform s for stream s (n > 0 is then not
 * read further).  n == 0 succeeds and does nothing.  What changes, and in which order of operations, is stated once in
 * csrc/similarity_dev.h: the map points and their pixel vectors, the keyframe poses and scene depths, the tracker's poses, the
 * translational half of its velocity, its scene depth, the camera-frame positions of its per-point data, and the relocaliser's pose;
 * everything else keeps every bit.  The pixel vectors are rotated and scaled, not remade (a map uploaded with the caller's own vectors
 * keeps them), and the depths are multiplied, not recomputed: with s == 1 a rigid move leaves velocity and depths bitwise alone.  The
 * tracker's next frame continues in the new gauge.  Two things read vslam_params.wiggle_scale as an absolute length
 * (IsDistanceToNearestKeyFrameExcessive, jni/MapMaker.cc:1098-1101, and the start depth of AddPointEpipolar) and do not follow a rescale,
 * and ba_convergence_limit and wls_prior are absolute in the same way (csrc/similarity_dev.h): that is the reference's behaviour,
 * nothing compensates for it.
 * Between frames or between subset steps; a stream held in the last step is not special.  The call waits once for the device to read the
 * listed streams' states; everything is decided before anything changes, and a refused call changes nothing for any stream.  All listed
 * streams go in one launch on the system's stream; nothing is allocated per call.
 * VSLAM_E_INVALID: NULL system, n < 0 or n > n_streams, an index outside the batch, a duplicate stream, NULL transforms with n > 0, a
 * non-finite entry, s <= 0, R not a rotation (max |R^T R - I| > 1e-9, or det R < 0).
 * VSLAM_E_STATE: a stage-wise frame is open; a listed stream has no good map, its trails running, or an adjustment of the asynchronous
 * map-maker pending (its result would land in the old gauge; the call succeeds once it has landed). */
int vslam_transform_maps(vslam_system* sys, const int* streams, int n, const double* new_from_old12 /* n x pose12 */, const double* scale /* n, or NULL: all 1 */);
/* out_i[0..1] = transforms of the stream since its creation, reset or restore, and mnFrame (jni/Tracker.h:116) at the last one;
 * out_d[0..12] = the accumulated similarity from the original gauge to the current one, pose12 then scale (a transform (R, t, s) applied
 * after (R_acc, t_acc, s_acc) gives R R_acc, s R t_acc + t, s s_acc).  Kept on the host: no wait.  vslam_reset_streams and
 * vslam_restore_stream put it back to zero and the identity; a snapshot does not carry it. */
int vslam_get_transform_info(vslam_system* sys, int stream, int out_i[2], double out_d[13]);
/* HIP-event milliseconds around the last vslam_transform_maps's launch on the system's stream.  Waits for it.  VSLAM_E_STATE before the
 * first call that transformed. */
int vslam_get_transform_timing(vslam_system* sys, double* ms);
/* Least-squares similarity to3 ~ s R from3 + t over n >= 3 correspondences (weights NULL = 1), Horn / Umeyama closed form; host only, no
 * GPU and no system.  fix_scale != 0: s = 1, only R and t are fitted.  The result goes straight into vslam_transform_maps: read the
 * keyframe centres with vslam_get_keyframe_pose, fit them to their known positions, apply.  R is always a proper rotation (det > 0), for
 * mirrored data too.  scale and rms (the weighted root mean square residual) may be NULL.
 * VSLAM_E_INVALID: n < 3, a non-finite entry, a negative weight, or points (from3, or to3) that are collinear or coincident within 1e-12
 * of their extent -- the rotation is then not determined. */
int vslam_fit_similarity(int n, const double* from3, const double* to3, const double* weights, int fix_scale,
                         double new_from_old12[12], double* scale, double* rms);

/* ---- map merge: append one live stream's map to another's ---------------------------------------
 * Pair i appends the map of stream src[i] to the map of stream dst[i], both in this system, on the device and in place; afterwards the
 * destination's tracker and map-maker work on the union.  A map from another system comes in through vslam_restore_stream into a spare
 * slot first.  The reference has no such operation (its Map is a single heap object, jni/Map.h:21-34): like retirement this is the
 * build's own, and a system that never calls it allocates nothing for it and launches nothing.
 * With nk_d keyframes and np_d points in the destination: the source's keyframe k becomes keyframe nk_d + k, its point p becomes point
 * np_d + p, order kept; measurements, templates and their source images, the tracker's per-point data, never-retry sets and the failure
 * queue come along renumbered (csrc/merge_dev.h states the index rules, csrc/merge.hip what every array holds afterwards).  The
 * appended keyframes are not fixed (the destination keeps its one gauge), the appended points carry none of the source's per-frame
 * flags, and both "bundle adjustment has converged" flags of the destination are cleared.  The source is read only and keeps every bit:
 * the caller resets it or lets it run on.  Nothing of the destination below its old counts changes.
 * Points that both maps hold of the same surface feature are two points afterwards; vslam_fuse_points (below) makes them one once they
 * have been measured at the same corners.  No registration: bringing both maps into one
 * frame and scale first is the caller's job (vslam_fit_similarity + vslam_transform_maps); nothing in this call can check it.  The parts
 * become one adjustable map as keyframes added afterwards measure points of both, and, with idle_iterations, as ReFindNewlyMade looks for
 * the appended points in the destination's keyframes: they all count as newly made (mqNewQueue keeps its head).
 * Between frames only.  The call waits once for the device to read the 2n states; everything is decided before anything changes, and a
 * refused call changes nothing for any stream.  All pairs go in one set of two launches; n == 0 succeeds and does nothing.
 * VSLAM_E_INVALID: NULL system, n < 0, NULL lists with n > 0, an index outside the batch, dst[i] == src[i], a stream that appears twice
 * among the 2n entries in either role (so the pairs of one call are independent).
 * VSLAM_E_STATE: a stage-wise frame is open; a stream of a pair has no good map, its trails running, or an adjustment of the
 * asynchronous map-maker pending.
 * VSLAM_E_CAPACITY: the keyframes of a pair exceed max_keyframes or its points max_points; the message names the pair, the counts and
 * the capacity.  vslam_retire_keyframes makes room. */
int vslam_merge_maps(vslam_system* sys, const int* dst, const int* src, int n);
/* out[0] = merges into this stream so far; of the last one: out[1] the source stream's index, out[2] keyframes appended, out[3] points
 * appended, out[4] failure-queue entries appended, out[5] the destination's mnFrame (jni/Tracker.h:116) at that time.  All zeros for a
 * stream that was never a destination.  vslam_reset_streams and vslam_restore_stream zero the record. */
int vslam_get_merge_info(vslam_system* sys, int stream, int out[6]);
/* HIP-event milliseconds around the last vslam_merge_maps's launches on the system's stream.  Waits for them.  VSLAM_E_STATE before the
 * first call that merged. */
int vslam_get_merge_timing(vslam_system* sys, double* ms);

/* ---- point fusion: coincident measurements make two map points one --------------------------------
 * After a merge of two maps of overlapping ground every shared surface feature is in the destination twice, and with idle_iterations
 * ReFindNewlyMade finds the appended twin in the destination's keyframes at the very corner where the destination's own point is
 * measured.  This call reads that and nothing else: two live (not bad) points q < p of a stream are duplicates if in at least min_views
 * keyframes both are measured at the same pyramid level with |root_p - root_q| <= radius * 2^level (radius in level pixels), and in no
 * keyframe both are measured otherwise (csrc/fuse_dev.h states the rule and its order of operations).  Nothing is projected and no
 * registration is trusted.  The partner of p is the lowest such q; p is dropped into it unless that q has a partner of its own -- one
 * level per call, all decisions on the state before the call: the tail of a chain stays, is counted, and a later call takes it.
 * The lower index is kept (after a merge: the destination's own point) with its position, template and tracker data; the next bundle
 * adjustment moves it.  Of a kept q an empty measurement cell (k, q) whose keyframe is not in q's never-retry set takes the measurement
 * (k, p) of the lowest p dropped into q that has one, no longer marked as a point's root measurement, and q's measurement-keyframe count
 * grows by one per cell taken.  A dropped p becomes bad and the valid bytes of its measurements are cleared; nothing else of it changes
 * (the tracker and the map-maker skip bad points; vslam_retire_keyframes reclaims their slots).  If anything was dropped both "bundle
 * adjustment has converged" flags are cleared.  Every other byte of the stream keeps its value.
 * streams == NULL: every stream, whatever n > 0 is (it is only checked against n_streams; n == 0 still does nothing).  Between frames or
 * between subset steps.  The call waits once for the device to read the listed streams'
 * states; everything is decided before anything changes, and a refused call changes nothing for any stream.  All listed streams go in one
 * set of four launches on the system's stream; n == 0 succeeds and does nothing.  The scratch (12 bytes per point of every stream's
 * capacity) is allocated by the first call.
 * VSLAM_E_INVALID: NULL system, n < 0 or n > n_streams, an index outside the batch, a duplicate stream, radius not finite or <= 0,
 * min_views < 1.
 * VSLAM_E_STATE: a stage-wise frame is open; a listed stream has no good map, its trails running, or an adjustment of the asynchronous
 * map-maker pending (its result would write outlier bookkeeping for points that no longer exist). */
int vslam_fuse_points(vslam_system* sys, const int* streams, int n, double radius, int min_views);
/* out[0] = calls that dropped something for this stream so far; of the last call that listed it: out[1] points dropped, out[2] cells
 * taken, out[3] valid cells of dropped points that were not taken, out[4] points left because their partner was itself a duplicate,
 * out[5] mnFrame (jni/Tracker.h:116) at that call.  All zeros before the first call.  vslam_reset_streams and vslam_restore_stream zero
 * the record. */
int vslam_get_fuse_info(vslam_system* sys, int stream, int out[6]);
/* The (dropped, kept) point indices of the last call that listed the stream, ascending by dropped: a caller that holds point indices
 * (anchors) follows them.  *n = the number of pairs; VSLAM_E_CAPACITY if cap is short (then *n is still the count and nothing is
 * written).  VSLAM_E_STATE for a stream no call has listed since its creation, reset or restore. */
int vslam_get_fuse_pairs(vslam_system* sys, int stream, int* dropped, int* kept, int cap, int* n);
/* HIP-event milliseconds around the last vslam_fuse_points's launches on the system's stream.  Waits for them.  VSLAM_E_STATE before the
 * first call that launched. */
int vslam_get_fuse_timing(vslam_system* sys, double* ms);

/* ---- overlay: the tracker's points and trails drawn into RGBA (vslam_params.overlay) -------------
 * What Tracker::TrackFrame draws on imageColor (jni/Tracker.cc:580-588 the patches TrackMap found, as discs coloured by pyramid level, the
 * `if(mbDraw)` guard commented out; :322-336 the bootstrap trails, as lines) and native_update hands back to the Java view
 * (jni/jni_part.cpp:59-71, 132-145).  The raster rules -- pixel format R, G, B, A; colours; the 21-pixel disc; the 4-pixel corner mark; the
 * closed form of the 8-connected line; clipping; drawing order -- are this build's own (OpenCV's cv::circle / cv::line are third-party
 * arithmetic, parity unpinned) and are stated once, in csrc/overlay_dev.h.  What is drawn for a stream is a pure function of read-backs
 * taken at the time of the call:
 *   base                 level 0 of the stream's current frame (vslam_read_level_image) as R = G = B = gray, A = 255; with
 *                        VSLAM_DRAW_IN_PLACE the caller's image, of which only drawn pixels are written (the reference's behaviour);
 *   VSLAM_DRAW_POINTS    a disc for every entry of the iteration set (vslam_get_search_plan) whose point has `found` set, centre = `image`
 *                        truncated, colour by `level` (vslam_get_point_tracks); the first entry ends on top.  Only if TrackMap ran for the
 *                        stream in its latest frame: a lost stream, a stream without a map and one just reset, restored or retired from
 *                        get no discs;
 *   VSLAM_DRAW_TRAILS    a line per trail (vslam_get_trails), initial -> current position, while init_stage == 1;
 *   VSLAM_DRAW_FAST      a mark at every level-0 corner of the current frame (vslam_read_corners; Tracker::drawFast, :148-155);
 *   VSLAM_DRAW_ALPHA0    a drawn pixel's alpha is 0 (what cv::Scalar's unset fourth value writes), not 255.
 * Marks lie under lines under discs. */
#define VSLAM_DRAW_POINTS 1
#define VSLAM_DRAW_TRAILS 2
#define VSLAM_DRAW_FAST 4
#define VSLAM_DRAW_IN_PLACE 8
#define VSLAM_DRAW_ALPHA0 16
/* image i (rgba + i*stream_stride, rows row_stride bytes apart, any alignment) belongs to streams[i]; streams == NULL: every stream, image s =
 * stream s (n is not read).  Between frames, and in a stage-wise frame after vslam_pose_update(sys, 1); earlier in an open frame
 * VSLAM_E_STATE.  on_device != 0: rgba is device memory and is written directly, asynchronously on the system's stream (a call with a stream
 * list waits once, for the list's upload).  Host memory: the call synchronises; in place the images go up, are drawn on and come down.
 * VSLAM_E_INVALID: NULL system, n < 0 or n > n_streams, an index outside the batch or a duplicate, NULL rgba with n > 0, row_stride <
 * 4 * width, stream_stride < row_stride * height with more than one image, unknown flag bits.  VSLAM_E_STATE: overlay = 0, no current
 * frame, or a listed stream was held in the last step (it has no front-end products).  A refused call writes nothing. */
int vslam_render_overlay(vslam_system* sys, const int* streams, int n, uint8_t* rgba, size_t row_stride, size_t stream_stride, int on_device, int flags);
/* out[0..3] = mnFrame at which TrackMap last ran (-1 none); discs, lines, marks of the stream's last render */
int vslam_get_overlay_info(vslam_system* sys, int stream, int out[4]);
int vslam_get_render_timing(vslam_system* sys, double* ms);   /* HIP events around the last render's launches; waits for them */
/* self-test hook, no system: the same device raster routines over primitives given by the caller, one image, host memory, synchronous.
 * width, height 1..4096; coordinates within +-32767; flags: VSLAM_DRAW_IN_PLACE (gray is not read) and VSLAM_DRAW_ALPHA0 */
int vslam_eval_overlay(int width, int height, const uint8_t* gray, size_t gray_stride, int n_marks, const int* marks_xy, int n_lines, const int* lines_xyxy,
                       int n_discs, const int* discs_xy_level /* 3 ints each, list order = iteration-set order */, uint8_t* rgba, size_t row_stride, int flags);

/* ---- stream snapshots ------------------------------------------------------------------------
 * One stream taken out of a live batch whole, and put back bit for bit into any slot of any compatible system.  The reference's only
 * persistence is MapMaker::GUICommandHandler("SaveMap") (jni/MapMaker.cc:1254-1286, vslam_save_map below: positions and poses at six
 * digits); what a snapshot carries is the Map itself (jni/Map.h:21-34: vpPoints, vpKeyFrames, bGood) with everything of the Tracker and
 * the MapMaker that a later frame or a per-stream read-back depends on: the tracker state, the map points with their PatchFinder state
 * and cached templates, the measurement tables, keyframe poses, depths and pyramids, the last frame's iteration set, and where the source
 * keeps them the never-retry sets and the failure queue (idle jobs), the last frame's SmallBlurryImage (use_sbi) and the relocaliser's
 * record (relocalise).  Keyframe corner lists and keyframe SmallBlurryImages are not carried: the restore remakes them from the stored
 * pyramids exactly as the map upload does, so a blob of a system without grow_map / relocalise restores into one with it.  Not carried: the
 * frame's own front-end products, vslam_get_reset_info, profiles and timings, and the bundle-adjustment pool record (vslam_get_bundle_stats
 * is a new stream's until the next adjustment).  From its next frame on the restored stream produces the bits the source stream produces
 * had it gone on.  The blob is compact (the counts in use, dense image rows), independent of the source's capacities, stream count and
 * slot, and has no checksum; csrc/snapshot_format.h states its layout.
 *
 * Refused with VSLAM_E_STATE: while a stage-wise frame is open; while the stream's trails are running (mnInitialStage
 * TRAIL_TRACKING_STARTED: the trail tracker reads the previous frame in place); while an adjustment of the asynchronous map-maker is
 * pending for the stream (the call succeeds once it has landed). */
/* (the struct cannot share the function's name: typedef names and functions live in one C name space) */
typedef struct vslam_snapshot_desc {
  int version, width, height, patch_size;
  double cam[5];
  int quirks;
  int n_keyframes, n_points, frame, map_good;
  int has_idle_state, has_sbi, has_reloc_state;          /* the optional parts */
  unsigned long long total_bytes;
  /* keyframe k's level-l image starts at image_offset[l] + k * image_stride[l]; its rows are image_row_stride[l] (= width >> l) bytes apart */
  unsigned long long image_offset[VSLAM_LEVELS], image_row_stride[VSLAM_LEVELS], image_stride[VSLAM_LEVELS];
  unsigned long long point_pos_offset;                   /* n_points x 3 doubles, MapPoint::v3WorldPos */
  unsigned long long keyframe_pose_offset;               /* n_keyframes x 12 doubles, pose12 layout */
} vslam_snapshot_desc;
/* *bytes = the size of the blob the stream's present state packs to.  Synchronises. */
int vslam_snapshot_size(vslam_system* sys, int stream, size_t* bytes);
/* Packs the stream on the device, then makes one copy to dst (host memory, or device memory with dst_on_device != 0).  Synchronises.
 * *bytes (may be NULL) is set to the blob's size whenever the stream can be packed, that is on success and on VSLAM_E_CAPACITY (cap too
 * small; dst is not written); a call refused with VSLAM_E_STATE or VSLAM_E_INVALID leaves it alone.  The failure queue travels sorted by
 * (keyframe, point) -- its order in memory is no part of the state -- and at most its capacity's entries of it. */
int vslam_snapshot_stream(vslam_system* sys, int stream, void* dst, size_t cap, int dst_on_device, size_t* bytes);
/* The slot first becomes what vslam_reset_streams makes it (a pending adjustment of the asynchronous map-maker is abandoned, and
 * vslam_get_reset_info counts the call), then receives the blob.  Ordered on the system's stream; a host blob is consumed before the call
 * returns.  Not asynchronous: the blob's header is read on the host first, and with keyframe corner lists (grow_map, idle jobs) the host
 * waits once per keyframe while they are remade, as in the map upload.  The blob's width, height, patch size, cam[5] and quirks must equal the system's, and the bytes must be a well-formed snapshot:
 * otherwise VSLAM_E_INVALID.  More keyframes or points (or failure-queue entries) than the system's capacities: VSLAM_E_CAPACITY.  A
 * refused call changes nothing.  The other streams are not touched. */
int vslam_restore_stream(vslam_system* sys, int stream, const void* blob, size_t bytes, int on_device);
/* Pure host code, no GPU and no system: validates magic, version, total size and every section of a blob in host memory against `bytes`
 * (VSLAM_E_INVALID otherwise) and describes it. */
int vslam_snapshot_info(const void* blob, size_t bytes, vslam_snapshot_desc* out);
/* The blob to and from a file. */
int vslam_save_stream(vslam_system* sys, int stream, const char* path);
int vslam_load_stream(vslam_system* sys, int stream, const char* path);
/* ms[0], ms[1] = HIP-event milliseconds of the last pack (the kernel) and of the last unpack (the reset, the kernel and the remaking of
 * the derived keyframe data) on the system's stream; 0 for one that has not run.  Synchronises. */
int vslam_get_snapshot_timing(vslam_system* sys, double ms[2]);

/* ---- tracking ------------------------------------------------------------------------------ */

typedef struct vslam_track_state {
  double pose[12];                 /* Tracker::GetCurrentPose, jni/Tracker.h:58 */
  double velocity[6];              /* mv6CameraVelocity */
  double msd_velocity, depth_mean, depth_sigma;
  int attempted[VSLAM_LEVELS], found[VSLAM_LEVELS];   /* manMeasAttempted / manMeasFound */
  int quality;                     /* 0 BAD, 1 DODGY, 2 GOOD (jni/Tracker.h:123) */
  int lost_frames, frame, did_coarse;
  int kf_added, n_keyframes, n_points, ba_accepted;
  long long n_zmssd, n_ba_trials;  /* counters: ZMSSD evaluations, LM trials */
} vslam_track_state;

/* Tracker::TrackFrame (jni/Tracker.cc:76-146) for one frame of every stream: MakeKeyFrame_Lite, motion
 * model, TrackMap, quality assessment, and -- when the tracker asks for a keyframe -- MapMaker::AddKeyFrame
 * (jni/MapMaker.cc:470-506) followed by one BundleAdjustRecent (jni/MapMaker.cc:801-851), all on device.
 * Same image arguments as vslam_make_keyframe_lite.  Asynchronous. */
int vslam_track_frame(vslam_system* sys, const uint8_t* gray, size_t row_stride, size_t stream_stride,
                      int on_device);
/* Tracker::TrackFrame stage by stage (per-kernel entry points for parity tests and benchmarks).  After
 * vslam_make_keyframe_lite, on the current frame of every stream:
 *   vslam_patch_search(sys, 0)  Tracker::ApplyMotionModel (jni/Tracker.cc:781-798), the potentially visible set with
 *                               TrackerData::Project / PatchFinder::CalcSearchLevelAndWarpMatrix (:369-392), the coarse selection
 *                               (:399-461) and Tracker::SearchForPoints (:629-674: MakeTemplateCoarseCont, FindPatchCoarse,
 *                               sub-pixel iterations) of the coarse set;
 *   vslam_pose_update(sys, 0)   the ten coarse Gauss-Newton iterations (:463-490): CalcJacobian, Tracker::CalcPoseUpdate (:683-774);
 *   vslam_patch_search(sys, 1)  the fine selection (:493-535) and SearchForPoints of the level-3 points and of the rest;
 *   vslam_pose_update(sys, 1)   the ten fine iterations (:543-577), measurement export and scene depth (:594-625),
 *                               UpdateMotionModel (:802-820), AssessTrackingQuality (:832-878), the keyframe decision (:128-132);
 *   vslam_finish_frame(sys)     MapMaker::AddKeyFrame + BundleAdjustRecent for the streams whose tracker asked for a keyframe.
 * vslam_track_frame is exactly this sequence.  All asynchronous; the tracker state between two stages is read with
 * vslam_get_state / vslam_get_point_tracks / vslam_get_template (pose = the tracker's current estimate) .
 * With vslam_params.relocalise, vslam_attempt_recovery comes between vslam_make_keyframe_lite and vslam_patch_search(sys, 0). */
int vslam_patch_search(vslam_system* sys, int stage);
int vslam_pose_update(vslam_system* sys, int stage);
int vslam_finish_frame(vslam_system* sys);
/* Tracker::AttemptRecovery (jni/Tracker.cc:163-175) with Relocaliser::AttemptRecovery (jni/Relocaliser.cc:17-58) for the streams that have a
 * map and have been lost for three frames (jni/Tracker.cc:133-139), on the current frame, before vslam_patch_search(sys, 0): the frame's
 * SmallBlurryImage at reloc_blur, ScoreKFs (ZMSSD against every keyframe's, jni/SmallBlurryImage.cc:82-94), IteratePosRelToTarget(best, 6),
 * SE3fromSE2.  A final score below 9e6 sets the pose to mse3Best, the velocity to zero and mbJustRecoveredSoUseCoarse; that frame then runs
 * TrackMap and AssessTrackingQuality only (no motion model, no keyframe).  The other streams are not touched.  Does nothing with
 * vslam_params.relocalise = 0.  vslam_track_frame calls it.  Asynchronous. */
int vslam_attempt_recovery(vslam_system* sys);
/* ---- subset steps: only the streams that have a new frame ----
 * One step for the n streams listed (distinct indices, any order); image i, at gray + i*stream_stride, belongs to streams[i].
 * The other streams of the batch are HELD: this step does not exist for them.  Every read-back of a held stream's tracker and map
 * returns the bytes it returned before the step (vslam_get_state with frame, kf_added, attempted / found and n_zmssd,
 * vslam_get_point_tracks, vslam_get_points, keyframe poses and measurements, templates, vslam_get_search_plan, vslam_get_idle_stats,
 * vslam_get_reloc_info, vslam_read_sbi, vslam_get_init_info); it makes no keyframe, runs no bundle adjustment and no idle pass, makes
 * no recovery attempt and no trail step; a pending spacebar stays pending, its shuffle seed and boot seed stay.  With the asynchronous
 * map-maker ba_delay_frames counts the stream's own frames: a pending result lands at the start of its D-th own frame after the
 * keyframe.  With use_sbi the rotation prior of its next frame aligns to its own last frame.
 * vslam_track_frame_subset is exactly vslam_make_keyframe_lite_subset, vslam_attempt_recovery, vslam_patch_search(0), vslam_pose_update(0),
 * vslam_patch_search(1), vslam_pose_update(1), vslam_finish_frame: after vslam_make_keyframe_lite_subset the stage-wise calls act on the
 * subset until the frame is finished.  n == 0 is a valid step in which nothing moves (streams and gray may then be NULL).
 * Every image is copied into the system's own level-0 storage, from the host (on_device = 0) or from device memory.
 * The step's front-end products of a held stream do not exist: vslam_read_level_image, vslam_read_corners, vslam_read_row_lut,
 * vslam_read_max_corners, vslam_read_candidates, vslam_minipatch_sample, vslam_minipatch_find and vslam_add_keyframe(stream) return
 * VSLAM_E_STATE for it; vslam_fast_nonmax, vslam_make_keyframe_rest, vslam_thin_candidates(keyframe < 0) and vslam_add_keyframe(-1) act
 * on the streams of the step.  Between steps nothing is special about a held stream.
 * VSLAM_E_INVALID: n < 0, n > n_streams, an index outside the batch, a duplicate index, NULL gray with n > 0.  VSLAM_E_STATE: a
 * stage-wise frame is open; or the step would hold a stream whose bootstrap trails are running (init_stage 1: it reads the previous
 * frame's level 0 in place, so its frames must be consecutive steps).  On systems created with bootstrap = 1 the call synchronises
 * once to read the stages; other systems do not synchronise.  A refused call changes nothing.  Asynchronous otherwise. */
int vslam_make_keyframe_lite_subset(vslam_system* sys, const int* streams, int n, const uint8_t* gray, size_t row_stride,
                                    size_t stream_stride, int on_device);
int vslam_track_frame_subset(vslam_system* sys, const int* streams, int n, const uint8_t* gray, size_t row_stride,
                             size_t stream_stride, int on_device);
/* in_step[n_streams] = 1 for the streams of the current / last step (all ones after a full step) */
int vslam_get_step_streams(vslam_system* sys, unsigned char* in_step);
/* the JNI-equivalent per-frame entry: native_update (jni/jni_part.cpp:132-145): host gray image of stream 0..n-1,
 * synchronous; native_touchScreen (:120-124) = the spacebar of every stream: with vslam_params.bootstrap it starts the trails / runs
 * InitFromStereo on the next frame of the streams that have no map, otherwise (and once a map exists) it has no effect. */
int vslam_update(vslam_system* sys, const uint8_t* gray, size_t row_stride, size_t stream_stride);
int vslam_touch(vslam_system* sys);

int vslam_get_state(vslam_system* sys, int stream, vslam_track_state* out);
/* the same for the streams [first, first + n): out[n], one device-to-host copy */
int vslam_get_states(vslam_system* sys, int first, int n, vslam_track_state* out);
/* MapMaker::NeedNewKeyFrame (jni/MapMaker.cc:761-773: distance to the closest keyframe, scaled by the scene depth, against
 * max_kf_dist_wiggle_mult * mdWiggleScaleDepthNormalized) and MapMaker::IsDistanceToNearestKeyFrameExcessive (:1098-1101: > 10 * wiggle
 * scale) for the stream's current pose.  The tracker takes both decisions on device; these are the reference's public members. */
int vslam_need_new_keyframe(vslam_system* sys, int stream, int* need);
int vslam_distance_to_nearest_keyframe_excessive(vslam_system* sys, int stream, int* excessive);
/* Tracker::GetMessageForUser (jni/Tracker.cc:880-883): "Tracking Map, quality good. Found: a/b ... Map: nP, nKF" */
int vslam_get_message(vslam_system* sys, int stream, char* buf, size_t cap);
/* per map point of a stream (arrays of n_points): TrackerData::bFound/bSearched/nSearchLevel/bDidSubPix,
 * v2Found (L0), v2Image.  Any pointer may be NULL. Returns n_points. */
int vslam_get_point_tracks(vslam_system* sys, int stream, int* found, int* searched, int* level, int* subpix,
                           double* vfound, double* image, int cap);
int vslam_get_points(vslam_system* sys, int stream, double* pos3, int* bad, int* n_inlier, int* n_outlier, int cap);
int vslam_get_keyframe_pose(vslam_system* sys, int stream, int keyframe, double pose12[12]);
/* The reference's only on-disk format, MapMaker::GUICommandHandler("SaveMap") (jni/MapMaker.cc:1254-1286): writes
 * <dir>/map.dump -- per map point (bad ones are in the reference's trash list and not written) v3WorldPos the way Eigen
 * streams a Vector3d (one coefficient per line, right-aligned to a common width, 6 significant digits) followed by two
 * blanks and nSourceLevel -- and <dir>/keyframes/<i>.info -- se3CfromW the way jni/RT.h:303-312 streams it (three lines
 * "r0 r1 r2 t") plus the blank line of the trailing endl.  The directories must exist.  Returns the number of points written. */
int vslam_save_map(vslam_system* sys, int stream, const char* dir);
int vslam_get_keyframe_measurements(vslam_system* sys, int stream, int keyframe, int* point, int* level,
                                    double* root_pos, int* source, int cap);
int vslam_get_template(vslam_system* sys, int stream, int point, uint8_t* tmpl /* P*P */, int* sum, int* sumsq,
                       int* bad);
/* the same for the points [first, first + n): tmpl n * P * P bytes; sum, sumsq, bad, have n ints each (any may be NULL) */
int vslam_get_templates(vslam_system* sys, int stream, int first, int n, uint8_t* tmpl, int* sum, int* sumsq, int* bad, int* have);
/* Size of the last bundle-adjustment problem MapMaker::BundleAdjust (jni/MapMaker.cc:854-960) assembled for the stream:
 * out[0..5] = cameras, adjustable cameras, points, measurements added, LM trials (mnCounter), accepted steps. */
int vslam_get_bundle_stats(vslam_system* sys, int stream, int out[6]);
/* Counters of the map-maker's idle jobs (vslam_params.idle_iterations, MapMaker::run jni/MapMaker.cc:94-117): out[0..5] = measurements
 * added by ReFindNewlyMade, by ReFindFromFailureQueue, BundleAdjustAll calls, idle BundleAdjustRecent calls, failure-queue length,
 * new-queue length. */
int vslam_get_idle_stats(vslam_system* sys, int stream, int out[6]);
/* One idle job of MapMaker::run (jni/MapMaker.cc:94-117) for every stream, between frames: 0 BundleAdjustRecent if not converged
 * (:97-98), 1 ReFindNewlyMade (:102-103), 2 BundleAdjustAll if not converged (:107-108), 3 every 20th call
 * ReFindFromFailureQueue (:112-113); each followed by HandleBadPoints (:117).  Needs idle_iterations != 0 at creation. */
int vslam_mapmaker_idle_job(vslam_system* sys, int job);

/* ---- map bootstrap (vslam_params.bootstrap) ----
 * Tracker::mbUserPressedSpacebar (jni/Tracker.h:138) of one stream, or of every stream (stream < 0): consumed by the next frame. */
int vslam_press_spacebar(vslam_system* sys, int stream);
/* MapMaker::InitFromStereo(KeyFrame&, KeyFrame&, vector<pair<ImageRef, ImageRef>>&, mySE3&) (jni/MapMaker.h:38, jni/MapMaker.cc:204-376) for a caller that
 * owns the two frames and the matches: host gray images of the first and the second keyframe, n matches as (x, y in the first, x, y in the second)
 * at level 0.  The first image becomes the first keyframe, the matches take the place of the trails, the second image is the frame the map is made
 * in.  Returns 1 and the tracker's pose (pose12_out may be NULL) when the map is good, 0 when InitFromStereo gave up (then a new attempt may
 * follow), a negative error otherwise.  One-stream systems created with bootstrap = 1 that have no map yet.  Synchronous. */
int vslam_init_from_stereo(vslam_system* sys, const uint8_t* gray_first, const uint8_t* gray_second, size_t row_stride, int n_matches,
                           const int* matches_xyxy, double pose12_out[12]);
/* the seed that stands in for the reference's rand() state in HomographyInit's MLESAC and CalcPlaneAligner's RANSAC (default 1) */
int vslam_set_boot_seed(vslam_system* sys, int stream, unsigned seed);

/* ---- the shuffle of the potentially visible set (vslam_params.pvs_shuffle_seed; jni/Tracker.cc:396-397, 525) ----
 * The seed of one stream, or of every stream (stream < 0), from its next frame on; 0 gives that stream the identity order.  VSLAM_E_STATE on a
 * system created with pvs_shuffle_seed = 0: it runs the planning kernel that has no shuffle.  vslam_reset_streams puts a stream's seed back
 * to the value of vslam_params. */
int vslam_set_pvs_seed(vslam_system* sys, int stream, unsigned seed);
/* vIterationSet of the stream's current frame, in order, as far as it is planned: after vslam_patch_search(sys, 0) the coarse set, after
 * vslam_patch_search(sys, 1) and after the frame also the level-3 points and the rest (jni/Tracker.cc:465, 507, 536-539).  iter_idx receives
 * map-point indices, at most cap; counts (may be NULL) = coarse entries, level-3 fine entries, other fine entries, total.  Returns the total.
 * Synchronises. */
int vslam_get_search_plan(vslam_system* sys, int stream, int* iter_idx, int cap, int counts[4]);
/* The permutation of csrc/pvs_perm.h on its own: out[j] = the position of the identity order that lands at j, for a list of n entries
 * (0..4096, else VSLAM_E_INVALID) with list = 0..3 for a level and 4 for the remaining points.  keys_or_null (n values) takes the place
 * of the generated keys: equal keys keep the identity order.  on_host != 0: the header's host form, no GPU needed; otherwise the device
 * routine the planning kernel calls, on one workgroup.  Both must return the same list. */
int vslam_pvs_permutation(unsigned seed, int frame, int list, int n, const unsigned* keys_or_null, int* out, int on_host);

/* out[0..5] = mnInitialStage (0 not started, 1 trails running, 2 complete), trails alive, InitFromStereo succeeded, homography inliers,
 * map points made from the stereo pair, map good */
int vslam_get_init_info(vslam_system* sys, int stream, int out[6]);
/* the trails (jni/Tracker.h Trail): irInitialPos x, y, irCurrentPos x, y per trail, in list order */
int vslam_get_trails(vslam_system* sys, int stream, int* out4, int cap, int* n);
/* ---- the two mathematical stages of the bootstrap on their own: test and diagnosis entry points ----
 * Both run the device functions InitFromStereo runs (csrc/boot.hip: boot_homography_stage, boot_plane_stage) in the work slices of one
 * stream and write a record; no tracker, keyframe or map field is read or written.  Systems created with bootstrap = 1; VSLAM_E_STATE while
 * the stream has an initialisation in progress (its trails are running) or a stage-wise frame is open.  Synchronous.  What a stage does not
 * reach stays zero in the record (best_trial: -1). */
#define VSLAM_PROBE_MAX_MATCHES 1000   /* MaxInitialTrails, jni/Tracker.cc:305 */
typedef struct vslam_homography_probe {
  int ok;                  /* HomographyInit::Compute succeeded and the translation has a length (InitFromStereo goes on) */
  int n;                   /* matches given */
  int best_trial;          /* first minimum of scores[] in trial order; -1 with fewer than ten matches (one direct fit, no trials) */
  int n_inliers;
  int choice;              /* ChooseBestDecomposition: 0 the visibility votes left no ambiguity, 1 / 2 the first / second of the ambiguous pair */
  int reserved;
  double scores[300];      /* the MLESAC score of every trial */
  double H_mlesac[9];      /* the best trial's homography (row-major; sign and scale are free) */
  double H_refined[9];     /* after the five refinements over the inliers */
  double R[9], t[3], normal[3], d;   /* the chosen decomposition */
  double t_scaled[3];      /* t at the length vslam_params.wiggle_scale: the second camera's translation */
  int inliers[VSLAM_PROBE_MAX_MATCHES];        /* indices of the inliers of H_mlesac, in match order (n_inliers of them) */
  double matches[VSLAM_PROBE_MAX_MATCHES * 8]; /* the HomographyMatch array the stage worked on: first xy, second xy, 2x2 pixel Jacobian at the second */
} vslam_homography_probe;
/* HomographyInit::Compute(vMatches, max_pixel_error, se3) and the scale of InitFromStereo (jni/MapMaker.cc:233-250) with `seed` in the place of the
 * stream's boot seed.  The n <= VSLAM_PROBE_MAX_MATCHES matches are given either as level-0 pixel pairs (matches_xyxy, 4 ints each: they go through
 * the kernel's own UnProject / GetProjectionDerivs as in InitFromStereo) or as ready HomographyMatch records (m8, 8 doubles each, laid out as
 * vslam_homography_probe.matches); the other pointer is NULL. */
int vslam_probe_homography_init(vslam_system* sys, int stream, int n, const int* matches_xyxy, const double* m8, unsigned seed, double max_pixel_error,
                                vslam_homography_probe* out);
typedef struct vslam_plane_probe {
  int have;                /* an aligner was made (ten points or more, and the best plane has an inlier) */
  int n;
  int best_trial;          /* first minimum among the trials that were not skipped; -1: none, mean / normal hold the defaults 0 / (0, 0, 1) */
  int reserved;
  double sums[100];        /* the summed truncated distance of every RANSAC trial; negative: the three points were collinear, trial skipped */
  double mean[3], normal[3];   /* of the best trial */
  double R[9], t[3];       /* the aligner (new-from-old), R row-major */
} vslam_plane_probe;
/* MapMaker::CalcPlaneAligner (jni/MapMaker.cc:1104-1231) over n <= max_points positions (3 doubles each).  seed is the RANSAC's own: InitFromStereo
 * runs it with the stream's boot seed + 1. */
int vslam_probe_plane_aligner(vslam_system* sys, int stream, int n, const double* pos3, unsigned seed, vslam_plane_probe* out);
/* Reads the directory vslam_save_map wrote (MapMaker "SaveMap", jni/MapMaker.cc:1254-1286: map.dump, keyframes/<i>.info) back: point
 * positions + source levels, keyframe poses as R (9, row-major) then t (3).  Arrays may be null to count only. */
/* Writes the state such a dump holds (positions of the good points, keyframe poses; 6 significant digits) back into the map it was
 * saved from: same keyframes and points, checked by count and source level.  Images, templates and measurements are not part of the
 * reference's format, so this restores an estimate, it does not build a map. */
int vslam_load_map(vslam_system* sys, int stream, const char* dir);
int vslam_read_map_dump(const char* dir, double* pos3, int* level, int point_cap, int* n_points, double* pose12, int kf_cap, int* n_keyframes);

/* ---- measurement: HIP-event time per stage of vslam_track_frame, on the system's own stream ---- */
#define VSLAM_N_STAGES 14
/* stages: 0 pyr_fast0, 1 fast_lvl, 2 compact, 3 pvs, 4 plan_coarse, 5 search_coarse, 6 pose_coarse, 7 plan_fine,
 * 8 search_fine, 9 pose_fine, 10 add_keyframe, 11 ba_assemble, 12 ba_compute, 13 ba_writeback */
const char* vslam_stage_name(int stage);
int vslam_profile_begin(vslam_system* sys, int max_frames);
/* synchronises; stage_ms[VSLAM_N_STAGES] = summed milliseconds over the recorded frames */
int vslam_profile_end(vslam_system* sys, double* stage_ms, int* n_frames);
/* launches[VSLAM_N_STAGES] = how many launches of each stage the last vslam_profile_begin/end pair recorded (every frame for all stages
 * but ba_compute with the asynchronous map-maker, which is launched once per batch of frames) */
int vslam_profile_launches(vslam_system* sys, int* launches);
/* What the Bundle::Compute launches (k_ba_compute) of the last vslam_profile_begin/end window actually ran, counted on the device by
 * the launches themselves: stats[0] problems, [1] LM trials (Do_LM_Step's inner trials, jni/Bundle.cc:327-501), and the
 * trial-weighted sums SURVEY.md 8(d)'s formulas need -- [2] trials x measurements, [3] trials x cameras, [4] trials x points,
 * [5] trials x points x C(adjustable cameras, 2), [6] trials x (6 x adjustable cameras)^3 -- [7] launches.  After vslam_profile_end. */
int vslam_profile_ba_stats(vslam_system* sys, unsigned long long stats[8]);
/* the same counters over every Bundle::Compute launch of the system since its creation (the last 1024); stats[7] = launches that ran a problem */
int vslam_get_ba_launch_totals(vslam_system* sys, unsigned long long stats[8]);
/* HIP-event time of the last host-driven vslam_bundle_adjust_recent / vslam_bundle_adjust_all on the system's stream:
 * ms[0] selection + assembly (k_ba_select, k_ba_assemble), ms[1] Bundle::Compute (k_ba_compute, one workgroup per stream's
 * problem), ms[2] write-back + HandleBadPoints; stats (may be NULL): the launch's counters as vslam_profile_ba_stats. Synchronises. */
int vslam_get_mapmaker_timing(vslam_system* sys, double ms[3], unsigned long long stats[8]);

/* ---- mapping ------------------------------------------------------------------------------- */
/* MapMaker::BundleAdjustRecent / BundleAdjustAll (jni/MapMaker.cc:801-851, 776-798) on every stream, followed by
 * HandleBadPoints (:140-164); what the reference's map-maker thread loop (:80-123) would run next. */
int vslam_bundle_adjust_recent(vslam_system* sys);
int vslam_bundle_adjust_all(vslam_system* sys);
/* MapMaker::AddKeyFrame (jni/MapMaker.cc:470-478) called from the host: the current frame of `stream` (all streams
 * if stream < 0) becomes a keyframe now, followed by the same BundleAdjustRecent + HandleBadPoints as the
 * tracker-driven path -- on the system's own stream, finished before the next frame, also with the asynchronous map-maker
 * (whose adjustments in flight are collected first).  Timed like vslam_bundle_adjust_recent (vslam_get_mapmaker_timing).
 * Needs a tracked current frame. */
int vslam_add_keyframe(vslam_system* sys, int stream);

/* ---- stand-alone Bundle (jni/Bundle.h:111-121), batched: n_problems independent problems ----
 * Capacity per problem: 1..128 cameras, 1..4096 points, 1..65536 measurements (vslam_bundle_create refuses more with
 * VSLAM_E_INVALID; an add_* or set_problem call past the problem's capacity returns VSLAM_E_CAPACITY and changes nothing).
 * At most 64 of a problem's cameras may be adjustable: a problem with more is not adjusted -- vslam_bundle_get_result reports
 * accepted = -1 and its cameras and points stay as added.
 * Duplicates: a problem holds at most one measurement per (camera, point) pair.  The reference accepts a second one (both enter
 * the U / V sums, GenerateMeasLUTs keeps the last for the reduced system); here vslam_bundle_add_meas and
 * vslam_bundle_set_problem refuse it with VSLAM_E_INVALID and the problem stays as it was. */
typedef struct vslam_bundle vslam_bundle;
int vslam_bundle_create(const vslam_params* p, int n_problems, int max_cameras, int max_points, int max_meas,
                        vslam_bundle** out);
int vslam_bundle_destroy(vslam_bundle* b);
int vslam_bundle_add_camera(vslam_bundle* b, int problem, const double pose12[12], int fixed);   /* Bundle::AddCamera */
int vslam_bundle_add_point(vslam_bundle* b, int problem, const double pos[3]);                   /* Bundle::AddPoint  */
int vslam_bundle_add_meas(vslam_bundle* b, int problem, int cam, int point, const double pos[2],
                          double sigma_squared);                                                  /* Bundle::AddMeas   */
/* Bundle::AddCamera / AddPoint / AddMeas for a whole problem at once, replacing what it held: pose12 n_cams x 12, fixed n_cams,
 * pos3 n_pts x 3; cam, point, sigma_squared n_meas and xy n_meas x 2 in AddMeas order. */
int vslam_bundle_set_problem(vslam_bundle* b, int problem, int n_cams, const double* pose12, const int* fixed, int n_pts, const double* pos3,
                             int n_meas, const int* cam, const int* point, const double* xy, const double* sigma_squared);
/* HIP-event milliseconds of the last vslam_bundle_compute launch (its inputs were resident before the first event) and the counters
 * the launch kept on the device (stats[8] as vslam_profile_ba_stats; may be NULL).  Synchronises. */
int vslam_bundle_get_timing(vslam_bundle* b, double* ms, unsigned long long stats[8]);
/* Bundle::Compute for every problem (one launch), each from the cameras / points / measurements the caller added -- a second call
 * starts again from those, not from the first call's result; asynchronous. accepted[problem] read by _get_result. */
int vslam_bundle_compute(vslam_bundle* b);
int vslam_bundle_synchronize(vslam_bundle* b);
int vslam_bundle_get_result(vslam_bundle* b, int problem, int* accepted, int* converged, double* sigma_squared,
                            double* lambda, long long* trials);
int vslam_bundle_get_camera(vslam_bundle* b, int problem, int n, double pose12[12]);             /* Bundle::GetCamera */
int vslam_bundle_get_point(vslam_bundle* b, int problem, int n, double pos[3]);                  /* Bundle::GetPoint  */
int vslam_bundle_get_outlier_meas(vslam_bundle* b, int problem, int* pc_pairs, int cap);         /* GetOutlierMeasurements */
int vslam_bundle_get_outlier_points(vslam_bundle* b, int problem, int* idx, int cap);            /* GetOutliers */

#ifdef __cplusplus
}
#endif
#endif
