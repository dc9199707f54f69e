// Similarity transform of a live stream's map: MapMaker::ApplyGlobalScaleToMap + ApplyGlobalTransformationToMap
// (jni/MapMaker.cc:440-464) for n streams of a live batch, on the device and in place (vslam_transform_maps), and the closed-form fit
// that gives such a transform from correspondences (vslam_fit_similarity, host only).  The rule -- which state changes and in which
// order of operations -- is csrc/similarity_dev.h; nothing of it is restated here.
//
// One launch, blockIdx.y = the ordinal in the call's list, blockIdx.x = a block of TRANSFORM_THREADS of that stream's points; the last
// block of a row is the tail: the keyframe poses and depths, the tracker's poses, velocity and depths, the relocaliser's pose.  Every
// element is read and written by one lane only, and no lane reads what another writes (the counts n_points and n_kf, which every
// block reads, are not written), so there is no ordering inside the launch.  The call's arguments (stream, T, T^-1, s per ordinal)
// travel through pinned memory into a device array sized for every stream at creation, in the batch that reads the listed streams'
// states: nothing is allocated per call.
#include "vslam_internal.h"
#include "similarity_dev.h"
#include "bootstrap_math.h"
#include <math.h>
#include <string.h>

#define TRANSFORM_THREADS 256

struct TransformArg { Similarity g; int stream; int pad; };
static TransformRecord transform_record_identity() {
  TransformRecord r = {};
  for (int i = 0; i < 9; i += 4) r.T.R[i] = 1.0;
  r.s = 1.0;
  return r;
}

__global__ __launch_bounds__(TRANSFORM_THREADS) void k_transform(MapDev m, TrackParams tp, const TransformArg* args, RelocInfo* reloc) {
  const TransformArg& a = args[blockIdx.y];
  const Similarity g = a.g;
  const int s = a.stream;
  TrackerState* st = &m.st[s];
  const int P = tp.max_points, K = tp.max_keyframes;
  const int np = st->n_points < 0 ? 0 : (st->n_points < P ? st->n_points : P);
  const int nk = st->n_kf < 0 ? 0 : (st->n_kf < K ? st->n_kf : K);
  if (blockIdx.x + 1 < gridDim.x) {                                  // ---- the points ----
    const int i = blockIdx.x * TRANSFORM_THREADS + threadIdx.x;
    if (i >= np) return;
    MapPointDev* p = m.pts + (size_t)s * P + i;
    const double pos[3] = {p->pos[0], p->pos[1], p->pos[2]}, right[3] = {p->right[0], p->right[1], p->right[2]}, down[3] = {p->down[0], p->down[1], p->down[2]};
    TrackData* td = m.td + (size_t)s * P + i;
    const double c0 = td->cam[0], c1 = td->cam[1], c2 = td->cam[2];
    double o[3];
    sim_point(g, pos, o);
    p->pos[0] = o[0]; p->pos[1] = o[1]; p->pos[2] = o[2];
    sim_vector(g, right, o);
    p->right[0] = o[0]; p->right[1] = o[1]; p->right[2] = o[2];
    sim_vector(g, down, o);
    p->down[0] = o[0]; p->down[1] = o[1]; p->down[2] = o[2];
    td->cam[0] = sim_length(g, c0); td->cam[1] = sim_length(g, c1); td->cam[2] = sim_length(g, c2);
    return;
  }
  // ---- the tail: keyframes from lane 0 up, the tracker's own state from the last lane down ----
  for (int k = threadIdx.x; k < nk; k += TRANSFORM_THREADS) {
    Pose* kp = m.kf_pose + (size_t)s * K + k;
    *kp = sim_pose(g, *kp);
    double* d = m.kf_depth + ((size_t)s * K + k) * 2;
    d[0] = sim_length(g, d[0]); d[1] = sim_length(g, d[1]);
  }
  switch (TRANSFORM_THREADS - 1 - (int)threadIdx.x) {
    case 0: st->pose_final = sim_pose(g, st->pose_final); break;
    case 1: st->start_pose = sim_pose(g, st->start_pose); break;
    case 2: st->pose_cur = sim_pose(g, st->pose_cur); break;
    case 3: if (reloc) reloc[s].best_pose = sim_pose(g, reloc[s].best_pose); break;
    case 4:
      for (int k = 0; k < 3; k++) st->velocity[k] = sim_length(g, st->velocity[k]);
      st->depth_mean = sim_length(g, st->depth_mean); st->depth_sigma = sim_length(g, st->depth_sigma);
      break;
    default: break;
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------
int transform_alloc(vslam_system* sys) {
  DevOwner& own = sys->own;
  const size_t S = (size_t)sys->S;
  TransformArg* d = nullptr;
  VCHK(own.alloc(&d, S, sys->stream));
  sys->transform_args = d;
  { void* pin = nullptr; VCHK(own.pinned(&pin, S * sizeof(TransformArg))); sys->transform_stage = pin; }
  for (int k = 0; k < 2; k++) VCHK(own.event(&sys->ev_transform_t[k], true));
  sys->transform_rec.assign(S, transform_record_identity());
  sys->transform_states.resize(S);
  return VSLAM_OK;
}

void transform_forget(vslam_system* sys, int s) { sys->transform_rec[(size_t)s] = transform_record_identity(); }

static const char* transform_bad_entry(const double* T12, double s) {
  for (int k = 0; k < 12; k++) if (!isfinite(T12[k])) return "has a non-finite entry";
  if (!isfinite(s)) return "has a non-finite scale";
  if (!(s > 0.0)) return "has a scale that is not positive";
  double ortho, det;
  sim_rotation_defect(T12, ortho, det);
  if (ortho > SIM_ROTATION_TOL || det < 0.0) return "is not a rotation (max |R^T R - I| > 1e-9, or a reflection)";
  return nullptr;
}

extern "C" int vslam_transform_maps(vslam_system* sys, const int* streams, int n, const double* new_from_old12, const double* scale) {
  if (!sys || n < 0 || n > sys->S) { vslam_set_error("transform_maps: bad argument"); return VSLAM_E_INVALID; }
  if (n == 0) return VSLAM_OK;
  if (!new_from_old12) { vslam_set_error("transform_maps: null transforms"); return VSLAM_E_INVALID; }
  const int S = sys->S, cnt = streams ? n : S;
  std::vector<unsigned char> seen;
  if (streams) {
    seen.assign((size_t)S, 0);
    for (int i = 0; i < n; i++) {
      if (streams[i] < 0 || streams[i] >= S) { vslam_set_error("transform_maps: stream %d of %d (entry %d); nothing was changed", streams[i], S, i); return VSLAM_E_INVALID; }
      if (seen[(size_t)streams[i]]) { vslam_set_error("transform_maps: stream %d is listed twice; nothing was changed", streams[i]); return VSLAM_E_INVALID; }
      seen[(size_t)streams[i]] = 1;
    }
  }
  for (int i = 0; i < cnt; i++) {
    const char* why = transform_bad_entry(new_from_old12 + 12 * (size_t)i, scale ? scale[i] : 1.0);
    if (why) { vslam_set_error("transform_maps: transform %d (stream %d) %s; nothing was changed", i, streams ? streams[i] : i, why); return VSLAM_E_INVALID; }
  }
  if (sys->frame_open) { vslam_set_error("transform_maps: a frame is open (vslam_finish_frame first)"); return VSLAM_E_STATE; }
  // One wait: the call's arguments go up and the listed streams' states come down in one batch; everything is decided before anything is
  // launched.  (The wait also means that the copy out of the pinned arguments has finished before the next call fills them again; a
  // refused call leaves a stale argument array behind, which nothing reads.)
  TransformArg* arg = (TransformArg*)sys->transform_stage;
  for (int i = 0; i < cnt; i++) {
    arg[i].g = sim_make(pose_from12(new_from_old12 + 12 * (size_t)i), scale ? scale[i] : 1.0);
    arg[i].stream = streams ? streams[i] : i; arg[i].pad = 0;
  }
  TrackerState* st = sys->transform_states.data();
  {
    HostCopy c(sys->stream);
    VCHK(c.put((TransformArg*)sys->transform_args, arg, (size_t)cnt));
    if (cnt == S) VCHK(c.get(st, sys->map.st, (size_t)S));
    else for (int i = 0; i < cnt; i++) VCHK(c.get(st + streams[i], sys->map.st + streams[i]));
    VCHK(c.wait());
  }
  for (int i = 0; i < cnt; i++) {
    const int s = arg[i].stream;
    const TrackerState& t = st[s];
    const char* why = !t.map_good ? "has no good map" : t.init_stage == 1 ? "has its trails running"
                    : (sys->tp.ba_delay > 0 && t.ba_countdown > 0) ? "has an adjustment pending" : nullptr;
    if (why) { vslam_set_error("transform_maps: stream %d %s; nothing was changed", s, why); return VSLAM_E_STATE; }
    if (t.n_kf < 0 || t.n_kf > sys->p.max_keyframes || t.n_points < 0 || t.n_points > sys->p.max_points) { vslam_set_error("transform_maps: stream %d holds counts beyond the system's capacities", s); return VSLAM_E_STATE; }
  }
  TransformRecord* rec = sys->transform_rec.data();
  for (int i = 0; i < cnt; i++) {
    const int s = arg[i].stream;
    rec[s].count++; rec[s].frame = st[s].frame;
    sim_compose(arg[i].g.T, arg[i].g.s, rec[s].T, rec[s].s);
  }
  HIPCHK(hipEventRecord(sys->ev_transform_t[0], sys->stream));
  const int blocks = (sys->p.max_points + TRANSFORM_THREADS - 1) / TRANSFORM_THREADS + 1;
  hipLaunchKernelGGL(k_transform, dim3(blocks, cnt), dim3(TRANSFORM_THREADS), 0, sys->stream, sys->map, sys->tp, (const TransformArg*)sys->transform_args, sys->reloc.info);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(sys->ev_transform_t[1], sys->stream));
  sys->transform_calls++;
  return VSLAM_OK;
}

extern "C" int vslam_get_transform_info(vslam_system* sys, int stream, int out_i[2], double out_d[13]) {
  if (!sys || stream < 0 || stream >= sys->S || !out_i || !out_d) { vslam_set_error("get_transform_info: bad argument"); return VSLAM_E_INVALID; }
  const TransformRecord& r = sys->transform_rec[(size_t)stream];
  out_i[0] = r.count; out_i[1] = r.frame;
  pose_to12(r.T, out_d); out_d[12] = r.s;
  return VSLAM_OK;
}

extern "C" int vslam_get_transform_timing(vslam_system* sys, double* ms) {
  if (!sys || !ms) { vslam_set_error("get_transform_timing: bad argument"); return VSLAM_E_INVALID; }
  if (sys->transform_calls == 0) { vslam_set_error("get_transform_timing: no vslam_transform_maps call that transformed yet"); return VSLAM_E_STATE; }
  HIPCHK(hipEventSynchronize(sys->ev_transform_t[1]));
  float t = 0.f;
  HIPCHK(hipEventElapsedTime(&t, sys->ev_transform_t[0], sys->ev_transform_t[1]));
  *ms = t;
  return VSLAM_OK;
}

// ---- the fit: Horn / Umeyama closed form, host only ------------------------------------------------------------------------
// to ~ s R from + t minimising sum w |to - (s R from + t)|^2.  With the weighted means mf, mt and the cross-covariance
// C = sum w (to - mt)(from - mf)^T = U D V^T (singular values decreasing): R = U diag(1, 1, det U det V) V^T, formed here as
// u0 v0^T + u1 v1^T + (u0 x u1)(v0 x v1)^T, which is that matrix whatever the signs the decomposition chose and needs only the two
// largest singular directions (three points are always coplanar: the third singular value is then zero and its u undefined).
// s = trace(R^T C) / sum w |from - mf|^2, t = mt - s R mf.
static void cross3(const double a[3], const double b[3], double o[3]) {
  o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}

// collinear or coincident within 1e-12 of the extent around the mean m, over the correspondences that carry weight
static bool fit_collinear(int n, const double* p3, const double* weights, const double m[3]) {
  double extent = 0.0, far[3] = {0, 0, 0};
  int counted = 0;
  for (int i = 0; i < n; i++) {
    if (weights && weights[i] == 0.0) continue;
    counted++;
    const double d[3] = {p3[3 * i] - m[0], p3[3 * i + 1] - m[1], p3[3 * i + 2] - m[2]};
    const double r = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    if (r > extent) { extent = r; far[0] = d[0] / r; far[1] = d[1] / r; far[2] = d[2] / r; }
  }
  if (counted < 3 || !(extent > 0.0)) return true;
  double off_line = 0.0;
  for (int i = 0; i < n; i++) {
    if (weights && weights[i] == 0.0) continue;
    const double d[3] = {p3[3 * i] - m[0], p3[3 * i + 1] - m[1], p3[3 * i + 2] - m[2]};
    double c[3];
    cross3(d, far, c);
    const double r = sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
    off_line = r > off_line ? r : off_line;
  }
  return off_line <= 1e-12 * extent;
}

extern "C" int vslam_fit_similarity(int n, const double* from3, const double* to3, const double* weights, int fix_scale,
                                    double new_from_old12[12], double* scale, double* rms) {
  if (n < 3 || !from3 || !to3 || !new_from_old12) { vslam_set_error("fit_similarity: needs n >= 3 correspondences and non-null arrays"); return VSLAM_E_INVALID; }
  double W = 0.0;
  for (int i = 0; i < n; i++) {
    for (int k = 0; k < 3; k++) if (!isfinite(from3[3 * i + k]) || !isfinite(to3[3 * i + k])) { vslam_set_error("fit_similarity: correspondence %d is not finite", i); return VSLAM_E_INVALID; }
    const double w = weights ? weights[i] : 1.0;
    if (!isfinite(w) || w < 0.0) { vslam_set_error("fit_similarity: weight %d is negative or not finite", i); return VSLAM_E_INVALID; }
    W += w;
  }
  if (!(W > 0.0)) { vslam_set_error("fit_similarity: the weights sum to zero"); return VSLAM_E_INVALID; }
  double mf[3] = {0, 0, 0}, mt[3] = {0, 0, 0};
  for (int i = 0; i < n; i++) {
    const double w = weights ? weights[i] : 1.0;
    for (int k = 0; k < 3; k++) { mf[k] += w * from3[3 * i + k]; mt[k] += w * to3[3 * i + k]; }
  }
  for (int k = 0; k < 3; k++) { mf[k] /= W; mt[k] /= W; }
  if (fit_collinear(n, from3, weights, mf)) { vslam_set_error("fit_similarity: the from points are collinear or coincident: no rotation is determined"); return VSLAM_E_INVALID; }
  if (fit_collinear(n, to3, weights, mt)) { vslam_set_error("fit_similarity: the to points are collinear or coincident: no rotation is determined"); return VSLAM_E_INVALID; }
  double Cm[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, var_f = 0.0;
  for (int i = 0; i < n; i++) {
    const double w = (weights ? weights[i] : 1.0) / W;
    double df[3], dt[3];
    for (int k = 0; k < 3; k++) { df[k] = from3[3 * i + k] - mf[k]; dt[k] = to3[3 * i + k] - mt[k]; }
    for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) Cm[3 * r + c] += w * dt[r] * df[c];
    var_f += w * (df[0] * df[0] + df[1] * df[1] + df[2] * df[2]);
  }
  double A[9], V[9], Sv[3];
  int order[3];
  memcpy(A, Cm, sizeof(A));
  bm::svd_onesided(A, 3, 3, V, Sv, order);                           // A = U diag(S) column by column
  if (!(Sv[order[1]] > 0.0)) { vslam_set_error("fit_similarity: the correspondences determine no rotation"); return VSLAM_E_INVALID; }
  double u[3][3], v[3][3];
  for (int j = 0; j < 2; j++) for (int k = 0; k < 3; k++) { u[j][k] = A[3 * k + order[j]] / Sv[order[j]]; v[j][k] = V[3 * k + order[j]]; }
  {                                                                  // u1 orthogonal to u0 to the last bit that matters, then the third of each hand
    const double d = u[0][0] * u[1][0] + u[0][1] * u[1][1] + u[0][2] * u[1][2];
    for (int k = 0; k < 3; k++) u[1][k] -= d * u[0][k];
    const double l = sqrt(u[1][0] * u[1][0] + u[1][1] * u[1][1] + u[1][2] * u[1][2]);
    for (int k = 0; k < 3; k++) u[1][k] /= l;
  }
  cross3(u[0], u[1], u[2]);
  cross3(v[0], v[1], v[2]);
  Pose T;
  for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) T.R[3 * r + c] = u[0][r] * v[0][c] + u[1][r] * v[1][c] + u[2][r] * v[2][c];
  double s = 1.0;
  if (!fix_scale) {
    double tr = 0.0;
    for (int k = 0; k < 9; k++) tr += T.R[k] * Cm[k];
    s = tr / var_f;
    if (!(s > 0.0) || !isfinite(s)) { vslam_set_error("fit_similarity: the fitted scale %g is not positive", s); return VSLAM_E_INVALID; }
  }
  double rmf[3];
  pose_rot(T, mf, rmf);
  for (int k = 0; k < 3; k++) T.t[k] = mt[k] - s * rmf[k];
  pose_to12(T, new_from_old12);
  if (scale) *scale = s;
  if (rms) {
    double e2 = 0.0;
    for (int i = 0; i < n; i++) {
      const double q[3] = {from3[3 * i] * s, from3[3 * i + 1] * s, from3[3 * i + 2] * s};
      double o[3];
      pose_xform(T, q, o);
      const double w = weights ? weights[i] : 1.0;
      for (int k = 0; k < 3; k++) e2 += w * (to3[3 * i + k] - o[k]) * (to3[3 * i + k] - o[k]);
    }
    *rms = sqrt(e2 / W);
  }
  return VSLAM_OK;
}
