// Point fusion: two live map points of one stream that were measured at the same place, at the same level, in several keyframes, and
// nowhere at different places, become one (vslam_fuse_points), on the device and in place, for any number of streams in one call.  It
// completes the map merge (merge.hip): after a merge of two maps of overlapping ground every shared feature is in the destination
// twice, and ReFindNewlyMade finds the appended twin in the destination's keyframes at the very corner where the destination's own
// point is measured.  That coincidence is appearance-verified (the patch finder located the template there) and is all the rule reads.
// The reference has no such operation; like retirement, transform and merge it is the build's own and opt-in by being called: a system
// that never calls it allocates nothing here and launches nothing.
//
// What it is not.  No registration and no geometry: nothing is projected, no world-space radius is read, so a sloppy similarity fit
// cannot fuse what merely lies close together.  No re-triangulation: the kept point keeps its position, the next bundle adjustment
// moves it.  One level per call: a point whose partner is itself a duplicate stays, is counted, and a later call takes it.
//
// The rule is csrc/fuse_dev.h.  The lower index q is kept (after a merge: the destination's own point), so its tracker data, template
// and PVS state do not move.  What changes, all decided on the state before the call:
//   kf_meas[k][q], k < nk   valid: stays.  Empty with bit k of never_retry[q] set: stays empty.  Empty otherwise: takes the 24 bytes of
//                           cell (k, p) of the lowest p dropped into q whose cell (k, p) is valid, SRC_ROOT turned into SRC_REFIND (a point
//                           has one root, its own: k_ba_writeback turns a point bad over an outlier at its root)
//   pts[q].n_meas_kfs       + 1 per cell taken
//   kf_meas[k][p], k < nk   the valid byte of a dropped p becomes 0 -- that byte alone, which is what handle_bad_points (ba.hip) leaves
//   pts[p].bad              1.  Nothing else of p: n_meas_kfs, pt_flags, queue entries and newq_head stay; every reader skips a bad
//                           point (k_pvs, k_ba_assemble's point set, k_refind, ReFindNewlyMade) or undoes what it added
//                           (handle_bad_points after ReFindFromFailureQueue); vslam_retire_keyframes reclaims the slot
//   TrackerState            ba_converged_recent = ba_converged_full = 0 if anything was dropped; every other byte stays
// Every other byte of the stream keeps its value.
//
// Four launches on the system's stream, every listed stream in each (blockIdx.y or blockIdx.x = ordinal), no host wait in between:
//   k_fuse_find     a workgroup takes a tile of FUSE_TILE candidate points p and walks the keyframes.  Per keyframe the row's cells for
//                   q below the tile's end come in through LDS in chunks of FUSE_CHUNK cells: consecutive lanes read consecutive
//                   16-byte words of the row (a cell is 24 bytes, a row starts on a multiple of 8: the chunk is read from the 16-byte
//                   word that holds its first byte), then the valid cells are compacted -- root as two doubles, (level, index) -- by
//                   wave ballot and one LDS counter.  The row is read once per tile, not once per p.  Each lane tests its own cell
//                   against the compacted ones (a broadcast read) and keeps the q that agree with it somewhere, at most FUSE_CAND of
//                   them, in LDS; the candidates are then verified in ascending order over all nk cells for the agree and conflict
//                   counts, and the first that passes is the partner.  A lane with more candidates than that verifies every q < p
//                   instead.  partner[p] is written for p < np.
//   k_fuse_resolve  one workgroup per stream: dropped = partner >= 0 && partner[partner] < 0; the (dropped, kept) pairs, compacted in
//                   ascending order of p by a block scan; the counts of the record; the two convergence flags.
//   k_fuse_take     a workgroup per pair, a lane per keyframe.  The workgroup lists the lower points dropped into the same q (the pairs
//                   are sorted by p; up to FUSE_SIB in LDS, beyond that every lane scans the pairs itself); a lane whose cell (k, p) is
//                   valid is the lowest for (k, q) if none of them has a valid cell (k, p'), and only the lowest goes on to read cell
//                   (k, q) and the never-retry bit and to write the cell.
//   k_fuse_drop     a lane per (pair, keyframe) clears the valid byte of cell (k, p); one per pair sets bad.
// Hazards.  Find only reads the map and writes partner, which resolve reads in the next launch.  In k_fuse_take a lane reads valid
// bytes of cells of dropped points, which no lane of that launch writes, and cell (k, q) of a kept point, which only the one lane that
// is lowest for (k, q) reads or writes: a kept point is never a dropped one (partner(q) < 0), so no cell is both.  n_meas_kfs and the
// record's counts are integer atomic adds.  k_fuse_drop writes what k_fuse_take read, hence the launch of its own.  Find and apply do
// not overlap: they are successive launches on one stream.
#include "vslam_internal.h"
#include "fuse_dev.h"
#include <limits.h>
#include <math.h>
#include <string.h>

#define FUSE_THREADS 256
#define FUSE_TILE FUSE_THREADS   // candidate points p of a workgroup, one per lane
#define FUSE_CHUNK 512           // cells of a row staged at a time
#define FUSE_CAND 16             // candidate partners a lane keeps before it falls back to verifying every q < p
#define FUSE_SIB 64              // lower points dropped into the same q that k_fuse_take lists in LDS before it falls back to scanning per lane
#define FUSE_APPLY_THREADS 128   // lanes across the keyframes of a pair (= FUSE_SET_BITS)
#define FUSE_APPLY_BLOCKS 32     // workgroups per stream that share the pairs
#define FUSE_RAW_WORDS ((FUSE_CHUNK * 24 + 15) / 16 + 1)

// the record of a stream: [0..5] are vslam_get_fuse_info's
enum FuseInfo : int { FI_CALLS = 0, FI_DROPPED, FI_TAKEN, FI_NOT_TAKEN, FI_CHAINED, FI_FRAME, FI_LISTED, FUSE_INFO_N = 8 };

static_assert(sizeof(MeasDev) == 24 && offsetof(MeasDev, valid) == 16 && offsetof(MeasDev, level) == 17, "the staging reads a cell as root[2] and the word behind it");

struct FuseArgs { const int* list; int* partner; int2* pairs; int* info; double radius; int min_views; };

DEVFN int fuse_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// dup(p, q) over the keyframes of the stream; q < p, p live
DEVFN bool fuse_pair_dup(const MeasDev* kfm, const MapPointDev* pts, int P, int nk, int p, int q, double radius, int min_views) {
  if (pts[q].bad) return false;
  int n_agree = 0;
  for (int k = 0; k < nk; k++) {
    const MeasDev cp = kfm[(size_t)k * P + p], cq = kfm[(size_t)k * P + q];
    const int r = fuse_relation(cp.valid, cp.level, cp.root[0], cp.root[1], cq.valid, cq.level, cq.root[0], cq.root[1], radius);
    if (r == FUSE_CONFLICT) return false;
    n_agree += r == FUSE_AGREE;
  }
  return fuse_dup(n_agree, 0, min_views);
}

// blockIdx.y = ordinal of the listed stream, blockIdx.x = tile of candidate points
__global__ __launch_bounds__(FUSE_THREADS) void k_fuse_find(MapDev m, TrackParams tp, FuseArgs a) {
  __shared__ uint4 s_raw[FUSE_RAW_WORDS];
  __shared__ double2 s_root[FUSE_CHUNK];
  __shared__ int2 s_meta[FUSE_CHUNK];            // (level, point index)
  __shared__ int s_cand[FUSE_CAND][FUSE_THREADS];
  __shared__ int s_n;
  const int s = a.list[blockIdx.y];
  const TrackerState* st = &m.st[s];
  const int P = tp.max_points, K = tp.max_keyframes;
  const int np = fuse_clamp(st->n_points, P), nk = fuse_clamp(st->n_kf, K);
  const int t = threadIdx.x, lane = t & 63;
  if (blockIdx.x == 0 && t == 0) {
    int* o = a.info + FUSE_INFO_N * (size_t)s;
    o[FI_DROPPED] = 0; o[FI_TAKEN] = 0; o[FI_NOT_TAKEN] = 0; o[FI_CHAINED] = 0; o[FI_FRAME] = st->frame; o[FI_LISTED] = 1;
  }
  const int p0 = blockIdx.x * FUSE_TILE;
  if (p0 >= np) return;
  const int pe = p0 + FUSE_TILE < np ? p0 + FUSE_TILE : np;          // the tile is [p0, pe)
  const int qe = pe - 1;                                             // the partners in question are [0, qe)
  const MapPointDev* pts = m.pts + (size_t)s * P;
  const MeasDev* kfm = m.kf_meas + (size_t)s * K * P;
  const int p = p0 + t;
  const bool live = p < np && !pts[p].bad;
  int ncand = 0;
  bool overflow = false;
  for (int k = 0; k < nk; k++) {
    const MeasDev* row = kfm + (size_t)k * P;
    bool mine = false; int lvl = 0; double px = 0.0, py = 0.0, lim2 = 0.0;
    if (live) {
      const MeasDev c = row[p];
      mine = c.valid != 0 && fuse_level_ok(c.level);                // a cell whose level names none agrees with nothing
      if (mine) { lvl = c.level; px = c.root[0]; py = c.root[1]; lim2 = fuse_lim2(a.radius, lvl); }
    }
    for (int c0 = 0; c0 < qe; c0 += FUSE_CHUNK) {
      const int cnt = qe - c0 < FUSE_CHUNK ? qe - c0 : FUSE_CHUNK;
      __syncthreads();                                               // the previous chunk has been tested
      if (t == 0) s_n = 0;
      // the chunk's bytes, from the 16-byte word that holds the first: at most 8 bytes of the cell (or row) before it and 15 of the
      // cell behind it come along, and c0 + cnt < np says that cell is still this row's
      const uintptr_t b0 = (uintptr_t)(row + c0);
      const int shift = (int)(b0 & 15);
      const uint4* src = (const uint4*)(b0 - (uintptr_t)shift);
      const int words = (shift + cnt * 24 + 15) / 16;
      for (int i = t; i < words; i += FUSE_THREADS) s_raw[i] = src[i];
      __syncthreads();
      const unsigned char* raw = (const unsigned char*)s_raw + shift;
      for (int j0 = 0; j0 < cnt; j0 += FUSE_THREADS) {
        const int j = j0 + t;
        int meta = 0;
        if (j < cnt) meta = *(const int*)(raw + (size_t)j * 24 + 16);
        const bool v = j < cnt && (meta & 0xff) != 0;
        const unsigned long long bm = __ballot(v);
        int base = 0;
        if (lane == 0 && bm) base = atomicAdd(&s_n, __popcll(bm));
        base = __shfl(base, 0);
        if (v) {
          const int pos = base + __popcll(bm & ((1ull << lane) - 1ull));
          const double* r = (const double*)(raw + (size_t)j * 24);
          s_root[pos] = make_double2(r[0], r[1]);
          s_meta[pos] = make_int2((int)(signed char)((meta >> 8) & 0xff), c0 + j);
        }
      }
      __syncthreads();
      if (mine) {
        const int n = s_n;
        for (int i = 0; i < n; i++) {
          const int2 e = s_meta[i];
          if (e.y >= p || e.x != lvl) continue;
          const double2 r = s_root[i];
          if (!fuse_within(px, py, r.x, r.y, lim2)) continue;
          bool have = false;
          for (int c = 0; c < ncand; c++) have = have || s_cand[c][t] == e.y;
          if (have) continue;
          if (ncand < FUSE_CAND) s_cand[ncand++][t] = e.y;
          else overflow = true;
        }
      }
    }
  }
  if (p >= np) return;
  int best = -1;
  if (live) {
    if (!overflow) {                                                 // ascending: the first candidate that passes is the partner
      int last = -1;
      for (int v = 0; v < ncand && best < 0; v++) {
        int q = INT_MAX;
        for (int c = 0; c < ncand; c++) { const int e = s_cand[c][t]; if (e > last && e < q) q = e; }
        if (fuse_pair_dup(kfm, pts, P, nk, p, q, a.radius, a.min_views)) best = q;
        last = q;
      }
    } else {
      for (int q = 0; q < p && best < 0; q++) if (fuse_pair_dup(kfm, pts, P, nk, p, q, a.radius, a.min_views)) best = q;
    }
  }
  a.partner[(size_t)s * P + p] = best;
}

// blockIdx.x = ordinal of the listed stream
__global__ __launch_bounds__(FUSE_THREADS) void k_fuse_resolve(MapDev m, TrackParams tp, FuseArgs a) {
  __shared__ int s_d[FUSE_THREADS / 64], s_c[FUSE_THREADS / 64];
  const int s = a.list[blockIdx.x];
  TrackerState* st = &m.st[s];
  const int P = tp.max_points;
  const int np = fuse_clamp(st->n_points, P);
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int* partner = a.partner + (size_t)s * P;
  int2* pairs = a.pairs + (size_t)s * P;
  int total = 0, chained = 0;
  for (int base = 0; base < np; base += FUSE_THREADS) {
    const int p = base + t;
    const int q = p < np ? partner[p] : -1;
    const bool d = q >= 0 && fuse_dropped(q, partner[q]);
    const bool ch = q >= 0 && !d;
    const unsigned long long bd = __ballot(d), bc = __ballot(ch);
    if (lane == 0) { s_d[wave] = __popcll(bd); s_c[wave] = __popcll(bc); }
    __syncthreads();
    int off = total;
    for (int w = 0; w < FUSE_THREADS / 64; w++) { if (w < wave) off += s_d[w]; total += s_d[w]; chained += s_c[w]; }
    if (d) pairs[off + __popcll(bd & ((1ull << lane) - 1ull))] = make_int2(p, q);
    __syncthreads();
  }
  if (t != 0) return;
  int* o = a.info + FUSE_INFO_N * (size_t)s;
  o[FI_DROPPED] = total; o[FI_CHAINED] = chained;
  if (total > 0) { o[FI_CALLS]++; st->ba_converged_recent = 0; st->ba_converged_full = 0; }
}

// blockIdx.y = ordinal of the listed stream, blockIdx.x shares the pairs; a lane per keyframe
__global__ __launch_bounds__(FUSE_APPLY_THREADS) void k_fuse_take(MapDev m, TrackParams tp, FuseArgs a) {
  const int s = a.list[blockIdx.y];
  const TrackerState* st = &m.st[s];
  const int P = tp.max_points, K = tp.max_keyframes;
  const int nk = fuse_clamp(st->n_kf, K);
  int* o = a.info + FUSE_INFO_N * (size_t)s;
  const int npairs = fuse_clamp(o[FI_DROPPED], P);
  const int2* pairs = a.pairs + (size_t)s * P;
  MapPointDev* pts = m.pts + (size_t)s * P;
  MeasDev* kfm = m.kf_meas + (size_t)s * K * P;
  __shared__ int s_sib[FUSE_SIB];
  __shared__ int s_nsib;
  int taken = 0, not_taken = 0;
  for (int j = blockIdx.x; j < npairs; j += gridDim.x) {
    const int2 pq = pairs[j];
    __syncthreads();                                                 // the previous pair's list has been read
    if (threadIdx.x == 0) s_nsib = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < j; i += FUSE_APPLY_THREADS) {      // the lower points dropped into the same q, in any order
      const int2 o2 = pairs[i];
      if (o2.y == pq.y) { const int n = atomicAdd(&s_nsib, 1); if (n < FUSE_SIB) s_sib[n] = o2.x; }
    }
    __syncthreads();
    const int nsib = s_nsib;
    for (int k = threadIdx.x; k < nk; k += FUSE_APPLY_THREADS) {
      MeasDev* row = kfm + (size_t)k * P;
      if (!row[pq.x].valid) continue;
      bool lowest = true;
      if (nsib <= FUSE_SIB) { for (int i = 0; i < nsib && lowest; i++) if (row[s_sib[i]].valid) lowest = false; }
      else for (int i = 0; i < j && lowest; i++) { const int2 o2 = pairs[i]; if (o2.y == pq.y && row[o2.x].valid) lowest = false; }
      bool take = false;
      if (lowest) {
        bool nr = false;
        if (m.never_retry) { const unsigned long long* w = m.never_retry + 2 * ((size_t)s * P + pq.y); nr = fuse_never_retry_bit(w[0], w[1], k); }
        take = fuse_takes(row[pq.y].valid, nr);
      }
      if (take) {
        MeasDev c = row[pq.x];
        c.source = (signed char)fuse_source(c.source);
        row[pq.y] = c;
        atomicAdd(&pts[pq.y].n_meas_kfs, 1);
        taken++;
      } else not_taken++;
    }
  }
  if (taken) atomicAdd(&o[FI_TAKEN], taken);
  if (not_taken) atomicAdd(&o[FI_NOT_TAKEN], not_taken);
}

__global__ __launch_bounds__(FUSE_APPLY_THREADS) void k_fuse_drop(MapDev m, TrackParams tp, FuseArgs a) {
  const int s = a.list[blockIdx.y];
  const TrackerState* st = &m.st[s];
  const int P = tp.max_points, K = tp.max_keyframes;
  const int nk = fuse_clamp(st->n_kf, K);
  const int npairs = fuse_clamp(a.info[FUSE_INFO_N * (size_t)s + FI_DROPPED], P);
  const int2* pairs = a.pairs + (size_t)s * P;
  MapPointDev* pts = m.pts + (size_t)s * P;
  MeasDev* kfm = m.kf_meas + (size_t)s * K * P;
  for (int j = blockIdx.x; j < npairs; j += gridDim.x) {
    const int p = pairs[j].x;
    for (int k = threadIdx.x; k < nk; k += FUSE_APPLY_THREADS) kfm[(size_t)k * P + p].valid = 0;
    if (threadIdx.x == 0) pts[p].bad = 1;
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------
static int fuse_alloc(vslam_system* sys) {
  if (sys->fuse_partner) return VSLAM_OK;
  DevOwner& own = sys->own;
  const size_t S = (size_t)sys->S, P = (size_t)sys->p.max_points;
  VCHK(own.alloc(&sys->fuse_info, S * FUSE_INFO_N, sys->stream));
  VCHK(own.alloc(&sys->fuse_list, S, sys->stream));
  VCHK(own.alloc(&sys->fuse_pairs, S * P, sys->stream));
  { void* pin = nullptr; VCHK(own.pinned(&pin, S * sizeof(int))); sys->fuse_list_stage = (int*)pin; }
  for (int k = 0; k < 2; k++) VCHK(own.event(&sys->ev_fuse_t[k], true));
  VCHK(own.alloc(&sys->fuse_partner, S * P, sys->stream));           // last: the sign that the scratch is whole
  return VSLAM_OK;
}

extern "C" int vslam_fuse_points(vslam_system* sys, const int* streams, int n, double radius, int min_views) {
  if (!sys || n < 0 || n > sys->S) { vslam_set_error("fuse_points: bad argument"); return VSLAM_E_INVALID; }
  if (!isfinite(radius) || !(radius > 0.0)) { vslam_set_error("fuse_points: the radius must be finite and positive; nothing was fused"); return VSLAM_E_INVALID; }
  if (min_views < 1) { vslam_set_error("fuse_points: min_views %d, at least 1 is needed; nothing was fused", min_views); return VSLAM_E_INVALID; }
  const int S = sys->S, cnt = streams ? n : S;
  if (streams) {
    std::vector<unsigned char> seen((size_t)S, 0);
    for (int i = 0; i < n; i++) {
      if (streams[i] < 0 || streams[i] >= S) { vslam_set_error("fuse_points: stream %d of %d (entry %d); nothing was fused", streams[i], S, i); return VSLAM_E_INVALID; }
      if (seen[(size_t)streams[i]]) { vslam_set_error("fuse_points: stream %d is listed twice; nothing was fused", streams[i]); return VSLAM_E_INVALID; }
      seen[(size_t)streams[i]] = 1;
    }
  }
  if (n == 0) return VSLAM_OK;
  if (sys->frame_open) { vslam_set_error("fuse_points: a frame is open (vslam_finish_frame first); nothing was fused"); return VSLAM_E_STATE; }
  VCHK(fuse_alloc(sys));
  // One wait: the list goes up and the listed streams' states come down in one batch; everything is decided before anything is
  // launched.  (The wait also means the previous call's copy out of the pinned list has long finished.)
  int* list = sys->fuse_list_stage;
  for (int i = 0; i < cnt; i++) list[i] = streams ? streams[i] : i;
  std::vector<TrackerState> st((size_t)cnt);
  {
    HostCopy c(sys->stream);
    VCHK(c.put(sys->fuse_list, list, (size_t)cnt));
    if (cnt == S) VCHK(c.get(st.data(), sys->map.st, (size_t)S));
    else for (int i = 0; i < cnt; i++) VCHK(c.get(&st[(size_t)i], sys->map.st + list[i]));
    VCHK(c.wait());
  }
  const int K = sys->p.max_keyframes, P = sys->p.max_points;
  for (int i = 0; i < cnt; i++) {
    const TrackerState& t = st[(size_t)i];
    const char* why = !t.map_good ? "has no good map" : t.init_stage == 1 ? "has its trails running"
                    : (sys->tp.ba_delay > 0 && t.ba_countdown > 0) ? "has an adjustment pending" : nullptr;
    if (why) { vslam_set_error("fuse_points: stream %d %s; nothing was fused", list[i], why); return VSLAM_E_STATE; }
    if (t.n_kf < 0 || t.n_kf > K || t.n_kf > FUSE_SET_BITS || t.n_points < 0 || t.n_points > P) { vslam_set_error("fuse_points: stream %d holds counts beyond the system's capacities", list[i]); return VSLAM_E_STATE; }
  }
  FuseArgs a = {sys->fuse_list, sys->fuse_partner, sys->fuse_pairs, sys->fuse_info, radius, min_views};
  HIPCHK(hipEventRecord(sys->ev_fuse_t[0], sys->stream));
  hipLaunchKernelGGL(k_fuse_find, dim3((P + FUSE_TILE - 1) / FUSE_TILE, cnt), dim3(FUSE_THREADS), 0, sys->stream, sys->map, sys->tp, a);
  hipLaunchKernelGGL(k_fuse_resolve, dim3(cnt), dim3(FUSE_THREADS), 0, sys->stream, sys->map, sys->tp, a);
  hipLaunchKernelGGL(k_fuse_take, dim3(FUSE_APPLY_BLOCKS, cnt), dim3(FUSE_APPLY_THREADS), 0, sys->stream, sys->map, sys->tp, a);
  hipLaunchKernelGGL(k_fuse_drop, dim3(FUSE_APPLY_BLOCKS, cnt), dim3(FUSE_APPLY_THREADS), 0, sys->stream, sys->map, sys->tp, a);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(sys->ev_fuse_t[1], sys->stream));
  sys->fuse_calls++;
  return VSLAM_OK;
}

extern "C" int vslam_get_fuse_info(vslam_system* sys, int stream, int out[6]) {
  if (!sys || stream < 0 || stream >= sys->S || !out) { vslam_set_error("get_fuse_info: bad argument"); return VSLAM_E_INVALID; }
  if (!sys->fuse_info) { for (int k = 0; k < 6; k++) out[k] = 0; return VSLAM_OK; }   // nothing has ever been fused here
  return host_get(sys->stream, out, sys->fuse_info + FUSE_INFO_N * (size_t)stream, 6);
}

extern "C" int vslam_get_fuse_pairs(vslam_system* sys, int stream, int* dropped, int* kept, int cap, int* n) {
  if (!sys || stream < 0 || stream >= sys->S || !n || cap < 0 || (cap > 0 && (!dropped || !kept))) { vslam_set_error("get_fuse_pairs: bad argument"); return VSLAM_E_INVALID; }
  int rec[FUSE_INFO_N] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (sys->fuse_info) VCHK(host_get(sys->stream, rec, sys->fuse_info + FUSE_INFO_N * (size_t)stream, (size_t)FUSE_INFO_N));
  if (!rec[FI_LISTED]) { vslam_set_error("get_fuse_pairs: stream %d has been in no vslam_fuse_points call (since its reset or restore)", stream); return VSLAM_E_STATE; }
  const int cnt = rec[FI_DROPPED] < 0 ? 0 : (rec[FI_DROPPED] > sys->p.max_points ? sys->p.max_points : rec[FI_DROPPED]);
  *n = cnt;
  if (cnt > cap) { vslam_set_error("get_fuse_pairs: stream %d has %d pairs, the arrays hold %d", stream, cnt, cap); return VSLAM_E_CAPACITY; }
  if (cnt == 0) return VSLAM_OK;
  std::vector<int2> pq((size_t)cnt);
  VCHK(host_get(sys->stream, pq.data(), sys->fuse_pairs + (size_t)stream * (size_t)sys->p.max_points, (size_t)cnt));
  for (int i = 0; i < cnt; i++) { dropped[i] = pq[(size_t)i].x; kept[i] = pq[(size_t)i].y; }
  return VSLAM_OK;
}

extern "C" int vslam_get_fuse_timing(vslam_system* sys, double* ms) {
  if (!sys || !ms) { vslam_set_error("get_fuse_timing: bad argument"); return VSLAM_E_INVALID; }
  if (sys->fuse_calls == 0) { vslam_set_error("get_fuse_timing: no vslam_fuse_points call that launched yet"); return VSLAM_E_STATE; }
  HIPCHK(hipEventSynchronize(sys->ev_fuse_t[1]));
  float t = 0.f;
  HIPCHK(hipEventElapsedTime(&t, sys->ev_fuse_t[0], sys->ev_fuse_t[1]));
  *ms = t;
  return VSLAM_OK;
}
