// vsg_mappoints.hip -- the local map's MapPoints resident on the device (include/vsg_orb.h: vsg_mappoints), and the two
// Frame entry points that read them: Frame::isInFrustum (Frame.cc:656-719) as a kernel and Tracking::SearchLocalPoints
// (Tracking.cc:3423-3495) as one enqueue and one wait.
//
// The local map changes slowly (a few hundred points per new keyframe) and the pose changes every frame: positions,
// normals, distance bounds and descriptors stay on the device, a call sends the pose (88 bytes, a kernel argument), the
// slot list and the skip flags.  k_frustum runs vsg::frustum_point one lane per map point and, for a search, writes the
// point's WinQuery and copies its descriptor into the calling thread's device arena, where k_window_search (enqueued
// right behind it on the same stream) finds both through WindowCall::launch's q_dev / qdesc_dev.  The descriptors are
// GATHERED by k_frustum rather than read by the window kernel through the slot index: the window kernel is the one
// every search routine shares and stays as it is, a wavefront of it reads its query's 32 bytes once either way, and
// only the points that are searched (in view, not far) are copied -- 13-19 % of a local map.
//
// k_project_points does the same for the two other searches of Tracking that project map points through a Frame's
// pose (vsg_project.h): SearchByProjection(CurrentFrame, LastFrame) with the last frame resident (its octaves are read
// on the device) and SearchByProjection(CurrentFrame, pKF, sAlreadyFound) for relocalisation; and for the back end's
// routines that project into ONE KeyFrame: the two Fuse and SearchByProjection(pKF, Scw, ...), whose Sim3 the caller
// has decomposed into a pose as the routines themselves do on entry.
#include <cstring>
#include <mutex>
#include <vector>

#include "vsg_frame_int.h"
#include "vsg_frustum.h"
#include "vsg_obs_args.h"
#include "vsg_observations.h"
#include "vsg_project.h"
#include "vsg_track_int.h"

using namespace vsg;

struct vsg_mappoints {
  int device = 0, capacity = 0;
  uint8_t *d_block = nullptr;  // one allocation behind the arrays below
  float *d_pos = nullptr, *d_normal = nullptr;  // [3 * capacity]
  float *d_min = nullptr, *d_max = nullptr;     // [capacity]
  uint8_t *d_desc = nullptr;                    // [32 * capacity]
  uint8_t *d_observed = nullptr;                // [capacity]
  std::mutex mutex;                             // update's duplicate stamps
  std::vector<uint32_t> stamp;                  // [capacity]: the update call that last listed the slot
  uint32_t epoch = 0;
};

bool vsg::store_view(const vsg_mappoints *mp, StoreView *v) {
  if (!mp || !mp->d_block) return false;
  *v = {mp->d_pos, mp->device, mp->capacity};
  return true;
}

bool vsg::store_fields(vsg_mappoints *mp, StoreFields *v) {
  if (!mp || !mp->d_block) return false;
  *v = {mp->d_pos, mp->d_normal, mp->d_min, mp->d_max, mp->d_desc, mp->d_observed, mp->device, mp->capacity};
  return true;
}

namespace {

struct StoreDev {
  float *pos, *normal, *min_dist, *max_dist;
  uint8_t *desc, *observed;
};
StoreDev store_dev(const vsg_mappoints *mp) {
  return {mp->d_pos, mp->d_normal, mp->d_min, mp->d_max, mp->d_desc, mp->d_observed};
}

// The fields of an update / a read, packed in the pinned arena; nullptr = field not part of the call.  Const pointers
// for an update (the arena is the source), plain ones for a read.
template <class F, class B>
struct FieldsDev {
  const int32_t *slots;  // -1: entry superseded by a later one of the same call
  F *pos, *normal, *min_dist, *max_dist;
  B *desc, *observed;
};
typedef FieldsDev<const float, const uint8_t> FieldsIn;
typedef FieldsDev<float, uint8_t> FieldsOut;

__device__ __forceinline__ void copy3(float *dst, const float *src) { dst[0] = src[0], dst[1] = src[1], dst[2] = src[2]; }
__device__ __forceinline__ void copy_desc(uint8_t *dst, const uint8_t *src) {  // 32 bytes, 32-byte aligned on both sides
  const uint4 lo = ((const uint4 *)src)[0], hi = ((const uint4 *)src)[1];
  ((uint4 *)dst)[0] = lo, ((uint4 *)dst)[1] = hi;
}

// vsg_mappoints_update: entry i of the arena -> slot slots[i].  One lane per entry.
__global__ __launch_bounds__(256) void k_mappoints_scatter(StoreDev S, FieldsIn A, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int s = A.slots[i];
  if (s < 0) return;
  if (A.pos) copy3(S.pos + 3 * (size_t)s, A.pos + 3 * (size_t)i);
  if (A.normal) copy3(S.normal + 3 * (size_t)s, A.normal + 3 * (size_t)i);
  if (A.min_dist) S.min_dist[s] = A.min_dist[i];
  if (A.max_dist) S.max_dist[s] = A.max_dist[i];
  if (A.desc) copy_desc(S.desc + 32 * (size_t)s, A.desc + 32 * (size_t)i);
  if (A.observed) S.observed[s] = A.observed[i];
}

// vsg_mappoints_read: slot slots[i] -> entry i of the arena
__global__ __launch_bounds__(256) void k_mappoints_gather(StoreDev S, FieldsOut A, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int s = A.slots[i];
  if (A.pos) copy3(A.pos + 3 * (size_t)i, S.pos + 3 * (size_t)s);
  if (A.normal) copy3(A.normal + 3 * (size_t)i, S.normal + 3 * (size_t)s);
  if (A.min_dist) A.min_dist[i] = S.min_dist[s];
  if (A.max_dist) A.max_dist[i] = S.max_dist[s];
  if (A.desc) copy_desc(A.desc + 32 * (size_t)i, S.desc + 32 * (size_t)s);
  if (A.observed) A.observed[i] = S.observed[s];
}

// What both projection kernels are launched with: the pose, the image bounds and a search's th and scale table, then the
// few scalars that one form reads.
struct PointArgs {
  vsg_frame_pose cam;
  ImageBounds bounds;  // the Frame's; the into-KeyFrame form: keyframe_bounds() of them
  int n;
  float th;
  float scale_factors[16];
  float viewing_cos_limit;   // k_frustum
  int b_factor, far_points;  // k_frustum's search half (Q != nullptr)
  float th_far_points;
  int direction;  // last-frame form: 0 neither, 1 bForward, 2 bBackward
};

// The per-point results of both kernels, one array per field; nullptr = the call does not want the field.
struct PointOut {
  uint8_t *valid;     // mbTrackInView / the point reaches GetFeaturesInArea
  float *x, *y;       // mTrackProjX / Y, uv
  float *xr, *depth;  // mTrackProjXR, uv(0) - mbf * invzc; mTrackDepth
  int32_t *level;     // mnTrackScaleLevel / nPredictedLevel
  float *view_cos;    // mTrackViewCos
  uint8_t *observed;  // Observations() > 0 of point i, for the ordered host pass
};
// valid, x and y are part of every call; a call names the others it wants with these bits
enum { kXr = 1, kDepth = 2, kLevel = 4, kViewCos = 8, kObserved = 16, kEveryCall = 32 };
// f(member, its bit) for every field of PointOut, in the order of the blocks in the arena
template <class Fn>
void point_fields(Fn f) {
  f(&PointOut::valid, kEveryCall), f(&PointOut::x, kEveryCall), f(&PointOut::y, kEveryCall), f(&PointOut::xr, kXr);
  f(&PointOut::depth, kDepth), f(&PointOut::level, kLevel), f(&PointOut::view_cos, kViewCos);
  f(&PointOut::observed, kObserved);
}

// Frame::isInFrustum, one lane per map point i = slot slots[i] (nullptr: slot i).  skip[i]: never projected (in_view 0,
// proj -1).  With Q: the window of SearchByProjection(F, vpMapPoints) (ORBmatcher.cc:59-70) as a WinQuery and the
// point's descriptor at qdesc[32 i]; a point that is not searched gets the inactive flag and no descriptor.
// k_window_search loads qdesc[32 q] of every query before it looks at the flag, so for those points it reads 32 bytes of the
// arena that this call never wrote: in bounds (n * 32 bytes are reserved), and the value is never used -- an inactive
// query has no candidates to compare it with.  Not a value to rely on, and not a read for a checker to flag.
// 64 lanes per workgroup: 4000 points are 63 workgroups on 63 CUs, each running the fp64 logf once.
__global__ __launch_bounds__(64) void k_frustum(StoreDev S, const int32_t *__restrict__ slots,
                                                const uint8_t *__restrict__ skip, PointArgs A, PointOut O,
                                                WinQuery *__restrict__ Q, uint8_t *__restrict__ qdesc) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= A.n) return;
  const int s = slots ? slots[i] : i;
  FrustumOut o = {0, -1.0f, -1.0f, 0.0f, 0.0f, 0, 0.0f};
  if (!(skip && skip[i])) {
    const float *P = S.pos + 3 * (size_t)s, *N = S.normal + 3 * (size_t)s;
    o = frustum_point(A.cam, A.bounds.minX, A.bounds.maxX, A.bounds.minY, A.bounds.maxY, A.viewing_cos_limit, P[0], P[1],
                      P[2], N[0], N[1], N[2], S.min_dist[s], S.max_dist[s]);
  }
  O.valid[i] = (uint8_t)o.in_view;
  O.x[i] = o.proj_x, O.y[i] = o.proj_y;
  if (O.xr) O.xr[i] = o.proj_xr;
  if (O.depth) O.depth[i] = o.depth;
  if (O.level) O.level[i] = o.scale_level;
  if (O.view_cos) O.view_cos[i] = o.view_cos;
  if (O.observed) O.observed[i] = S.observed[s];
  if (Q) {
    WinQuery w = win_inactive(false);
    // :50-54: !mbTrackInView -> continue; bFarPoints && mTrackDepth > thFarPoints -> continue
    if (o.in_view && !(A.far_points && o.depth > A.th_far_points)) {
      w = win_local(o.proj_x, o.proj_y, o.proj_xr, o.scale_level, o.view_cos, A.th, A.b_factor, A.scale_factors);
      copy_desc(qdesc + 32 * (size_t)i, S.desc + 32 * (size_t)s);
    }
    Q[i] = w;
  }
}

// The projection loops of SearchByProjection(CurrentFrame, LastFrame) (kLast, ORBmatcher.cc:1686-1724) and of
// SearchByProjection(CurrentFrame, pKF, sAlreadyFound) (ORBmatcher.cc:1895-1930), one lane per query, 64 lanes per
// workgroup like k_frustum.  kProjLast: query i = feature i of the resident last frame, slots[i] < 0 = no map point or an
// outlier, the octave is the last frame's own.  kProjReloc: query i = slot slots[i], skip[i] = isBad() or
// in sAlreadyFound.  kProjKeyFrame: the loop of Fuse x2 and SearchByProjection(pKF, Scw, ...) (ORBmatcher.cc:1194-1241,
// :1360-1395, :452-486), query i = slot slots[i], skip[i] = isBad(), IsInKeyFrame(pKF) or in spAlreadyFound; A.bounds
// are the KeyFrame's truncated ones.  A query that is not searched gets the inactive flag and no descriptor (see k_frustum).
// Of O it can fill valid, x, y, xr (last-frame and into-KeyFrame form), level (the two KeyFrame forms) and observed.
enum { kProjLast = 0, kProjReloc = 1, kProjKeyFrame = 2 };
template <int kForm>
__global__ __launch_bounds__(64) void k_project_points(StoreDev S, const int32_t *__restrict__ slots,
                                                       const uint8_t *__restrict__ skip,
                                                       const KeyPointPOD *__restrict__ last_kps, PointArgs A,
                                                       PointOut O, WinQuery *__restrict__ Q,
                                                       uint8_t *__restrict__ qdesc) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= A.n) return;
  const int s = slots[i];
  ProjectOut o = {0, 0.0f, 0.0f, 0.0f, 0};
  WinQuery w = win_inactive(false);
  uint8_t observed = 0;
  if (s >= 0 && !(skip && skip[i])) {
    const float *P = S.pos + 3 * (size_t)s;
    if (kForm == kProjLast) {
      const int oct = last_kps[i].octave;  // nLastOctave (:1711); the host refused octaves outside the pyramid
      o = project_last_point(A.cam, A.bounds, P);
      if ((unsigned)oct >= 16u) o.valid = 0;
      if (o.valid) w = win_last(o.u, o.v, o.ur, oct, A.th, A.direction, A.scale_factors);
      observed = S.observed[s];
    } else if (kForm == kProjReloc) {
      o = project_kf_point(A.cam, A.bounds, P, S.min_dist[s], S.max_dist[s]);
      if (o.valid) w = win_kf(o.u, o.v, fmul(A.th, A.scale_factors[o.level]), o.level);  // radius: :1928
    } else {
      o = project_keyframe_point(A.cam, A.bounds, P, S.normal + 3 * (size_t)s, S.min_dist[s], S.max_dist[s]);
      // radius: :1241 / :1395 / :486; the level window [l - 1, l] and Fuse's ur ride in the query
      if (o.valid) w = win_keyframe_area(o.u, o.v, fmul(A.th, A.scale_factors[o.level]), o.level, o.ur, false);
    }
    if (o.valid) copy_desc(qdesc + 32 * (size_t)i, S.desc + 32 * (size_t)s);
  }
  O.valid[i] = (uint8_t)o.valid;
  O.x[i] = o.u, O.y[i] = o.v;
  if (O.xr) O.xr[i] = o.ur;
  if (O.level) O.level[i] = o.level;
  if (O.observed) O.observed[i] = observed;
  Q[i] = w;
}

// ---- vsg_mappoints_refresh_from_observations: MapPoint::ComputeDistinctiveDescriptors (MapPoint.cc:340-417) and
// MapPoint::UpdateNormalAndDepth (:440-513) of many map points from their observation lists, written into the slots.
// One entry of the keyframe table per keyframe: where its descriptors and keypoints live on the device (read from the
// vsg_frame handles by the call itself) and its camera centre.
struct KfEntry {
  const uint8_t *desc;
  const KeyPointPOD *kps;
  float Ow[3];
  int32_t pad;
};
struct RefreshArgs {
  const KfEntry *table;
  const int32_t *order;  // point indices: the launch handles order[first .. first + count)
  const int32_t *slots, *off, *kf, *idx;
  const uint8_t *bad;  // nullptr: no observation is bad
  const int32_t *ref_pos;
  int first, count, what, nlevels;
  float scale_factors[16];
  int32_t *best;  // the outs, by point index, in the pinned arena
  float *normal, *min_dist, *max_dist;
};

__device__ __forceinline__ int hamming_u4(const uint4 a0, const uint4 a1, const uint4 b0, const uint4 b1) {
  return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) +
         __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}

// A group of kLanes lanes (one wavefront, or a workgroup of two) per map point, kPts groups per workgroup: real
// observation counts are 3 to 20, and one workgroup per point would leave most of the chip idle.  The host sends a point
// to the form whose kLanes holds its observations that are not bad (obs_check: at most 128); every index the kernel forms
// is one obs_check has bounded.  Every barrier is reached by every lane: nothing returns early.
//   1. 64 observations at a time: lane j reads observation j's bad flag and computes its unit vector; the ballot of the
//      flags gives the list positions of the good observations in order (s_good), and the unit vectors are added SERIALLY
//      in list order (every lane adds the same values: float addition does not associate, vsg_observations.h).
//   2. lane j fetches good observation j's 32 bytes through the table into the LDS tile; every later pass reads LDS.
//   3. lane i computes row i of the distance matrix into its own LDS column and finds the element of rank
//      (int)(0.5 * (N - 1)) by bisection on the VALUE (9 bits: 9 counting passes, not N): the least v with
//      #{x <= v} > rank.
//   4. the least (median << 16 | i) over the group: the first row with the least median (strict '<', :406); that row
//      goes from the tile into the slot as two uint4 stores.
template <int kLanes, int kPts>
__global__ __launch_bounds__(kLanes *kPts) void k_refresh(StoreDev S, RefreshArgs A) {
  constexpr int kWaves = kLanes / 64;
  __shared__ uint4 s_desc[kPts][kLanes][2];
  __shared__ uint16_t s_D[kPts][kLanes * kLanes];  // [j][i]: lane i's column, written and read by lane i alone
  __shared__ int32_t s_good[kPts][kLanes];
  __shared__ uint32_t s_key[kPts][kWaves];
  const int g = threadIdx.x / kLanes, t = threadIdx.x % kLanes, lane = threadIdx.x & 63, gw = t >> 6;
  const int q = blockIdx.x * kPts + g;
  const bool active = q < A.count;
  int p = 0, s = 0, o = 0, m = 0;
  float P[3] = {0.0f, 0.0f, 0.0f};
  if (active) {
    p = A.order[A.first + q], s = A.slots[p], o = A.off[p], m = A.off[p + 1] - o;
    copy3(P, S.pos + 3 * (size_t)s);
  }
  const bool do_normal = (A.what & VSG_REFRESH_NORMAL) && gw == 0;
  int ngood = 0;
  float sum[3] = {0.0f, 0.0f, 0.0f};
  for (int c = 0; c < m; c += 64) {
    const int j = c + lane;
    bool good = false;
    float u[3] = {0.0f, 0.0f, 0.0f};
    if (j < m) {
      good = !(A.bad && A.bad[o + j]);  // pKF->isBad() (:363); UpdateNormalAndDepth has no such test
      if (do_normal) observation_unit(P, A.table[A.kf[o + j]].Ow, u);
    }
    const unsigned long long mask = __ballot(good);
    const int pos = ngood + __popcll(mask & ((1ull << lane) - 1ull));
    if (good && gw == 0 && pos < kLanes) s_good[g][pos] = j;
    ngood += __popcll(mask);
    if (do_normal) {
      const int cnt = min(64, m - c);
      for (int k = 0; k < cnt; k++) {
        const float uk[3] = {__shfl(u[0], k), __shfl(u[1], k), __shfl(u[2], k)};
        observation_add(sum, uk);
      }
    }
  }
  ngood = min(ngood, kLanes);
  if (active && t == 0) {
    float nrm[3], mn = S.min_dist[s], mx = S.max_dist[s];
    copy3(nrm, S.normal + 3 * (size_t)s);
    if (do_normal && m > 0) {  // :455: no observation, no change
      const int r = o + A.ref_pos[p];
      const KfEntry e = A.table[A.kf[r]];
      const int level = e.kps[A.idx[r]].octave & 15;  // :492; obs_check saw it below nlevels
      observation_depth(P, e.Ow, A.scale_factors, level, A.nlevels, &mn, &mx);
      observation_mean(sum, m, nrm);
      copy3(S.normal + 3 * (size_t)s, nrm);
      S.min_dist[s] = mn, S.max_dist[s] = mx;
    }
    copy3(A.normal + 3 * (size_t)p, nrm);
    A.min_dist[p] = mn, A.max_dist[p] = mx;
  }
  const bool do_desc = active && (A.what & VSG_REFRESH_DESC) && ngood > 0;  // :354, :379
  __syncthreads();
  uint4 d0 = {0, 0, 0, 0}, d1 = {0, 0, 0, 0};
  if (do_desc && t < ngood) {
    const int j = o + s_good[g][t];
    const uint4 *src = (const uint4 *)(A.table[A.kf[j]].desc + 32 * (size_t)A.idx[j]);
    d0 = src[0], d1 = src[1];
    s_desc[g][t][0] = d0, s_desc[g][t][1] = d1;
  }
  __syncthreads();
  uint32_t key = 0xFFFFFFFFu;
  if (do_desc && t < ngood) {
    uint16_t *D = s_D[g] + t;
    for (int j = 0; j < ngood; j++) D[j * kLanes] = (uint16_t)hamming_u4(d0, d1, s_desc[g][j][0], s_desc[g][j][1]);
    const int rank = (ngood - 1) >> 1;  // vDists[0.5 * (N - 1)] (:404)
    int lo = 0, hi = 256;
    for (int it = 0; it < 9; it++) {  // [0, 256] holds 257 values: 9 halvings
      const int mid = (lo + hi) >> 1;
      int le = 0;
      for (int j = 0; j < ngood; j++) le += D[j * kLanes] <= mid;
      if (le > rank)
        hi = mid;
      else
        lo = mid + 1;
    }
    key = ((uint32_t)lo << 16) | (uint32_t)t;
  }
  for (int d = 32; d > 0; d >>= 1) key = min(key, (uint32_t)__shfl_xor((int)key, d));
  if (lane == 0) s_key[g][gw] = key;
  __syncthreads();
  if (do_desc) {
    uint32_t b = s_key[g][0];
    for (int w = 1; w < kWaves; w++) b = min(b, s_key[g][w]);
    const int win = (int)(b & 0xFFFFu);
    if (t < 2) ((uint4 *)(S.desc + 32 * (size_t)s))[t] = s_desc[g][win][t];
    if (t == 0) A.best[p] = s_good[g][win];
  } else if (active && t == 0) {
    A.best[p] = -1;
  }
}

int store_check(const vsg_mappoints *mp) { return mp && mp->d_block ? VSG_OK : VSG_ERR_INVALID; }

// Does every slot of a caller's list lie inside the store (nullptr list: the kernel uses slot i)?  Every entry point asks
// BEFORE anything is enqueued: an error return leaves no kernel behind.
bool slots_in_store(const vsg_mappoints *mp, int n, const int32_t *slots) {
  if (!slots) return n <= mp->capacity;
  for (int i = 0; i < n; i++)
    if (slots[i] < 0 || slots[i] >= mp->capacity) return false;
  return true;
}

// What the seven entry points on resident points check first, in this order (the codes differ): the handles and the
// pose are there; no second camera; one device, a pyramid, n, the entry's own required arrays (entry_ok); and for a
// search (levels) its scale table against the pose.  An entry adds its slot list's test and what only it knows.
int resident_check(const vsg_frame *F, const vsg_mappoints *mp, const vsg_frame_pose *pose, int n, bool entry_ok,
                   bool levels, const float *scale_factors, int nlevels) {
  if (!F || !F->d_block || store_check(mp) != VSG_OK || !pose) return VSG_ERR_INVALID;
  // isInFrustumChecks with KannalaBrandt8 (Frame.cc:721-800), bRight / mpCamera2 (ORBmatcher.cc:1154-1159)
  if (F->nleft != -1) return VSG_ERR_UNSUPPORTED;
  if (F->device != mp->device || pose->n_levels < 1 || n < 0 || !entry_ok) return VSG_ERR_INVALID;
  if (levels && (!scale_factors || nlevels < 1 || nlevels > 16 || pose->n_levels > nlevels)) return VSG_ERR_INVALID;
  return VSG_OK;
}

// The kernels' arguments for F's camera at `pose`; a search adds its th and scale table.  kKeyFrameBounds: the bounds are
// KeyFrame::mnMinX .. mnMaxY, the Frame's truncated to int.  The scalars of one form are the caller's to set by name.
enum BoundsForm { kFrameBounds, kKeyFrameBounds };
PointArgs point_args(const vsg_frame *F, const vsg_frame_pose *pose, int n, BoundsForm form = kFrameBounds, float th = 0.0f,
                     const float *scale_factors = nullptr, int nlevels = 0) {
  PointArgs A;
  memset(&A, 0, sizeof(A));
  A.cam = *pose;
  A.bounds = {F->minX, F->maxX, F->minY, F->maxY};
  if (form == kKeyFrameBounds) A.bounds = keyframe_bounds(A.bounds);
  A.n = n, A.th = th;
  for (int l = 0; l < nlevels; l++) A.scale_factors[l] = scale_factors[l];
  return A;
}

// update and read share the staging: slots + the fields that are part of the call, one kernel, one wait
struct CopyLayout {
  size_t oS, oP, oN, oMin, oMax, oD, oO, total;
  CopyLayout(size_t N, bool pos, bool normal, bool mind, bool maxd, bool desc, bool obs) {
    Stage st;
    oS = st.add(N * 4), oP = st.add(pos ? N * 12 : 0), oN = st.add(normal ? N * 12 : 0), oMin = st.add(mind ? N * 4 : 0);
    oMax = st.add(maxd ? N * 4 : 0), oD = st.add(desc ? N * 32 : 0), oO = st.add(obs ? N : 0);
    total = st.total;
  }
};

// arguments every update / read checks BEFORE anything is staged or enqueued; the thread's context with the arena reserved
int copy_begin(vsg_mappoints *mp, int n, const int32_t *slots, const CopyLayout &L, ThreadCtx **c) {
  if (!slots_in_store(mp, n, slots)) return VSG_ERR_INVALID;
  int rc = VSG_OK;
  *c = thread_ctx(mp->device, &rc);
  if (!*c) return rc;
  return ctx_reserve(*c, L.total, 0);
}

// The wait is part of both contracts: the arena is free for the thread's next call, and another thread's search that starts
// after an update returns reads the new values (its stream is not ordered against this one).
int copy_end(ThreadCtx *c) {
  const hipError_t e1 = hipGetLastError(), e2 = hipStreamSynchronize(c->stream);
  return e1 == hipSuccess && e2 == hipSuccess ? VSG_OK : VSG_ERR_HIP;
}

// The pinned-arena blocks of one call on resident points, [slots? | skip? | the fields of PointOut the call wants]:
// lay_out() says how many bytes to reserve, bind() (after the reserve: it may move the arena) copies the caller's slots
// and skip flags in and takes both sides' pointers, copy_out() hands the caller the fields it gave an array for.
struct PointStage {
  size_t N = 0, oSlots = 0, oSkip = 0, off[8] = {}, total = 0;
  unsigned want = 0;
  const int32_t *src_slots = nullptr, *slots = nullptr;  // the caller's, and where the kernel reads them (nullptr: slot i)
  const uint8_t *src_skip = nullptr, *skip = nullptr;
  PointOut host = {}, dev = {};

  void lay_out(int n, const int32_t *slots_, const uint8_t *skip_, unsigned want_) {
    N = (size_t)n, src_slots = slots_, src_skip = skip_, want = want_ | kEveryCall;
    Stage st;
    oSlots = st.add(src_slots ? N * 4 : 0), oSkip = st.add(src_skip ? N : 0);
    int k = 0;
    point_fields([&](auto m, unsigned bit) { off[k++] = st.add(want & bit ? N * sizeof(*(host.*m)) : 0); });
    total = st.total;
  }
  template <class T>
  static void at(T *&p, uint8_t *block) { p = (T *)block; }
  void bind(uint8_t *hp, uint8_t *dp) {
    if (src_slots) memcpy(hp + oSlots, src_slots, N * 4), slots = (const int32_t *)(dp + oSlots);
    if (src_skip) memcpy(hp + oSkip, src_skip, N), skip = dp + oSkip;
    int k = 0;
    point_fields([&](auto m, unsigned bit) {
      if (want & bit) at(host.*m, hp + off[k]), at(dev.*m, dp + off[k]);
      k++;
    });
  }
  // dst names the caller's arrays (nullptr: not asked for); only a field the call wanted may be asked for
  void copy_out(const PointOut &dst) const {
    point_fields([&](auto m, unsigned) {
      if (dst.*m) memcpy(dst.*m, host.*m, N * sizeof(*(dst.*m)));
    });
  }
};

// What a projection kernel is launched with besides its arguments: the device side of a PointStage, where the search's
// queries and descriptors go (nullptr: isInFrustum alone), and the stream.
struct ResidentDev {
  const int32_t *slots;
  const uint8_t *skip;
  PointOut out;
  WinQuery *Q;
  uint8_t *qdesc;
  hipStream_t stream;
};
void launch_frustum(const ResidentDev &R, const vsg_mappoints *mp, const PointArgs &A) {
  hipLaunchKernelGGL(k_frustum, dim3((A.n + 63) / 64), dim3(64), 0, R.stream, store_dev(mp), R.slots, R.skip, A, R.out, R.Q,
                     R.qdesc);
}
template <int kForm>
void launch_project(const ResidentDev &R, const vsg_mappoints *mp, const vsg_frame *last, const PointArgs &A) {
  const bool kLast = kForm == kProjLast;
  hipLaunchKernelGGL(k_project_points<kForm>, dim3((A.n + 63) / 64), dim3(64), 0, R.stream, store_dev(mp), R.slots,
                     R.skip, kLast ? (const KeyPointPOD *)last->d_kps : (const KeyPointPOD *)nullptr, A, R.out, R.Q, R.qdesc);
}

// How the window kernel behind the projection runs: candidate lists for an ordered host pass, or the best candidate per
// query (Fuse) with its scan's start value and, for the chi-square gate, pKF->mvInvLevelSigma2.
struct ResidentMode {
  int mode, gate_mode, best_init;
  const float *inv_sigma2;
  int nlevels;
};
ResidentMode resident_lists(int gate_mode) { return {kWinList, gate_mode, 256, nullptr, 0}; }

// What the six searches on resident map points share: a projection kernel that writes every point's WinQuery and
// gathers its descriptor, k_window_search right behind it on the same stream, one wait.  The call's PointStage sits
// behind the window call's blocks in the pinned arena, [WinQuery | descriptors] in the device arena.
struct ResidentCall {
  WindowCall wc;
  PointStage st;

  // want: the optional fields of PointOut the projection kernel is to write; launch(ResidentDev) enqueues it.
  // enqueue(): both kernels on the thread's stream, no wait.  dev_lists (the chain calls, vsg_track_int.h): {start, length}
  // and the candidate array go to the device arena behind the queries and descriptors, where a kernel behind these two
  // reads them, and the pinned arena holds none of the three; *lists = where they are.  pin_extra / dev_extra: room for
  // the caller's own blocks behind this call's in both arenas; dev_used = where the device one starts.  n == 0 enqueues
  // nothing.
  size_t dev_used = 0;
  struct DevLists {
    int *off, *cnt;
    uint32_t *ent;
    size_t entries;
  };
  template <class Launch>
  int enqueue(const vsg_frame *F, int n, const int32_t *slots, const uint8_t *skip, unsigned want, const ResidentMode &M,
              Launch launch, bool dev_lists = false, size_t pin_extra = 0, size_t dev_extra = 0, DevLists *lists = nullptr) {
    st.lay_out(n, slots, skip, want);
    wc.dev_lists = dev_lists;
    int rc = wc.begin(F->device, n, M.mode, false, 0, st.total + pin_extra);
    if (rc != VSG_OK) return rc;
    ThreadCtx *c = wc.c;
    const size_t Q = (size_t)(n > 0 ? n : 1), entries = Q * kWinInline + (size_t)wc.cap;
    Stage sd;
    const size_t dQ = sd.add(Q * sizeof(WinQuery)), dD = sd.add(Q * 32);
    const size_t dOff = sd.add(dev_lists ? Q * 4 : 0), dCnt = sd.add(dev_lists ? Q * 4 : 0),
                 dOut = sd.add(dev_lists ? entries * 4 : 0);
    dev_used = sd.total;
    rc = ctx_reserve(c, 0, sd.total + dev_extra);
    if (rc != VSG_OK) return rc;
    // both reserves first, pointers after: either reserve may move its arena
    st.bind(c->h_pin + wc.bytes(), c->d_pin + wc.bytes());
    if (dev_lists) {
      wc.x_off = (int *)(c->d_buf + dOff), wc.x_cnt = (int *)(c->d_buf + dCnt), wc.x_out = (uint32_t *)(c->d_buf + dOut);
      if (lists) *lists = {wc.x_off, wc.x_cnt, wc.x_out, entries};
    }
    if (n == 0) return VSG_OK;
    const ResidentDev R = {st.slots, st.skip, st.dev, (WinQuery *)(c->d_buf + dQ), c->d_buf + dD, c->stream};
    launch(R);
    rc = hipGetLastError() == hipSuccess ? VSG_OK : VSG_ERR_HIP;
    if (rc == VSG_OK) rc = wc.launch(F, M.gate_mode, M.best_init, M.inv_sigma2, M.nlevels, R.qdesc, R.Q);
    if (rc != VSG_OK) hipStreamSynchronize(c->stream);  // nothing of this call may still write the arena when the next one fills it
    return rc;
  }
  // enqueue() and the wait.  VSG_RETRY: the lists overflowed, the whole call runs again
  template <class Launch>
  int run(const vsg_frame *F, int n, const int32_t *slots, const uint8_t *skip, unsigned want, const ResidentMode &M,
          Launch launch) {
    const int rc = enqueue(F, n, slots, skip, want, M, launch);
    return rc != VSG_OK ? rc : wc.finish();
  }
};

// SearchLocalPoints' second loop and its search as vsg_frame_search_local_points and the chain call
// (track_local_enqueue) both enqueue them: one definition of the arguments, of the fields k_frustum writes and of the gate.
PointArgs local_point_args(const vsg_frame *F, const vsg_frame_pose *pose, int n, float viewing_cos_limit, float th,
                           int far_points, float th_far_points, const float *scale_factors, int nlevels) {
  PointArgs A = point_args(F, pose, n, kFrameBounds, th, scale_factors, nlevels);
  A.viewing_cos_limit = viewing_cos_limit;
  A.b_factor = th != 1.0;  // ORBmatcher.cc:46
  A.far_points = far_points ? 1 : 0, A.th_far_points = th_far_points;
  return A;
}
int local_enqueue(ResidentCall &call, const vsg_frame *F, const vsg_mappoints *mp, int n, const int32_t *slots,
                  const uint8_t *skip, const PointArgs &A, bool dev_lists = false, size_t pin_extra = 0,
                  size_t dev_extra = 0, ResidentCall::DevLists *lists = nullptr) {
  // the stereo gate of :97-102 applies to frames with mvuRight (Nleft == -1 here)
  return call.enqueue(F, n, slots, skip, kObserved, resident_lists(F->has_uright ? kGateUr : kGateNone),
                      [&](const ResidentDev &R) { launch_frustum(R, mp, A); }, dev_lists, pin_extra, dev_extra, lists);
}

// The caller's arrays of the three routines that project into one KeyFrame, by name (ur: Fuse's pose form alone)
PointOut keyframe_outs(uint8_t *projected, float *u, float *v, float *ur, int32_t *predicted_level) {
  PointOut dst = {};
  dst.valid = projected, dst.x = u, dst.y = v, dst.xr = ur, dst.level = predicted_level;
  return dst;
}

// What those three check BEFORE anything is enqueued, resident_check first.  VSG_OK with *go == false: n == 0, the entry
// returns 0.
int keyframe_check(const vsg_frame *kf, const vsg_mappoints *mp, int n, const int32_t *slots, const vsg_frame_pose *pose,
                   const float *scale_factors, int nlevels, bool entry_ok, bool *go) {
  *go = false;
  const int rc = resident_check(kf, mp, pose, n, entry_ok, true, scale_factors, nlevels);
  if (rc != VSG_OK || n == 0) return rc;
  if (!slots || !slots_in_store(mp, n, slots)) return VSG_ERR_INVALID;
  *go = true;
  return VSG_OK;
}

// Fuse's search on resident points: the projection kernel, then k_window_search in best mode; one wait
int fuse_points(vsg_frame *kf, vsg_mappoints *mp, int n, const int32_t *slots, const uint8_t *skip,
                const vsg_frame_pose *pose, float th, const float *scale_factors, int nlevels, const ResidentMode &M,
                int32_t *best_idx, int32_t *best_dist, const PointOut &dst) {
  const PointArgs A = point_args(kf, pose, n, kKeyFrameBounds, th, scale_factors, nlevels);
  ResidentCall call;
  const int rc = call.run(kf, n, slots, skip, kXr | kLevel, M,
                          [&](const ResidentDev &R) { launch_project<kProjKeyFrame>(R, mp, nullptr, A); });
  if (rc != VSG_OK) return rc;
  call.st.copy_out(dst);
  return call.wc.best_out(M.best_init, best_idx, best_dist);
}

}  // namespace

namespace vsg {

const uint8_t *store_observed_dev(const vsg_mappoints *mp) { return mp->d_observed; }

int track_last_check(const vsg_frame *cur, const vsg_frame *last, const vsg_mappoints *mp, const int32_t *last_slots,
                     const vsg_frame_pose *cur_pose, const vsg_frame_pose *last_pose, float mb, int mono,
                     const float *scale_factors, int nlevels, int *dir) {
  if (!last || !last->d_block || !last_pose || !last_slots) return VSG_ERR_INVALID;
  const int n = last->n;
  const int rc = resident_check(cur, mp, cur_pose, n, true, true, scale_factors, nlevels);
  if (rc != VSG_OK) return rc;
  if (last->nleft != -1) return VSG_ERR_UNSUPPORTED;  // the right-camera block (ORBmatcher.cc:1785-1853)
  if (last->device != cur->device) return VSG_ERR_INVALID;
  const vsg_keypoint *lk = last->h_kps.data();
  for (int i = 0; i < n; i++) {
    if (last_slots[i] >= mp->capacity) return VSG_ERR_INVALID;
    if (last_slots[i] >= 0 && (lk[i].octave < 0 || lk[i].octave >= nlevels)) return VSG_ERR_INVALID;
  }
  *dir = motion_direction(*cur_pose, *last_pose, mb, mono ? 1 : 0);  // :1677-1684
  return VSG_OK;
}

int track_last_enqueue(TrackSearch *T, const vsg_frame *cur, const vsg_frame *last, const vsg_mappoints *mp,
                       const int32_t *last_slots, const vsg_frame_pose *cur_pose, float th, int dir,
                       const float *scale_factors, int nlevels, size_t pin_extra_bytes, size_t dev_extra_bytes) {
  PointArgs A = point_args(cur, cur_pose, last->n, kFrameBounds, th, scale_factors, nlevels);
  A.direction = dir;
  // the stereo gate of :1742-1748 applies to frames with mvuRight (Nleft == -1 here)
  ResidentCall call;
  ResidentCall::DevLists lists = {};
  const int rc = call.enqueue(cur, last->n, last_slots, nullptr, kXr | kObserved,
                              resident_lists(cur->has_uright ? kGateUr : kGateNone),
                              [&](const ResidentDev &R) { launch_project<kProjLast>(R, mp, last, A); }, true,
                              pin_extra_bytes, dev_extra_bytes, &lists);
  if (rc != VSG_OK) return rc;
  // what the entry point needs after this frame is gone: the window call (its counter accounting) and plain pointers
  T->wc = call.wc;
  call.wc.range_open = false;  // T->wc pops the range now
  T->c = T->wc.c, T->nq = last->n, T->list_total = (int)lists.entries;
  T->pin_extra = T->wc.bytes() + call.st.total, T->dev_extra = call.dev_used;
  T->d_observed = call.st.dev.observed, T->d_slots = call.st.slots;
  T->d_off = lists.off, T->d_cnt = lists.cnt, T->d_ent = lists.ent;
  return VSG_OK;
}

int track_local_check(const vsg_frame *F, const vsg_mappoints *mp, int n, const int32_t *slots, const vsg_frame_pose *pose,
                      const float *scale_factors, int nlevels) {
  const int rc = resident_check(F, mp, pose, n, true, true, scale_factors, nlevels);
  if (rc != VSG_OK) return rc;
  return n == 0 || slots_in_store(mp, n, slots) ? VSG_OK : VSG_ERR_INVALID;
}

int track_local_enqueue(TrackSearch *T, const vsg_frame *F, const vsg_mappoints *mp, int n, const int32_t *slots,
                        const uint8_t *skip, const vsg_frame_pose *pose, float viewing_cos_limit, float th, int far_points,
                        float th_far_points, const float *scale_factors, int nlevels, size_t pin_extra_bytes,
                        size_t dev_extra_bytes) {
  const PointArgs A = local_point_args(F, pose, n, viewing_cos_limit, th, far_points, th_far_points, scale_factors, nlevels);
  ResidentCall call;
  ResidentCall::DevLists lists = {};
  const int rc = local_enqueue(call, F, mp, n, slots, skip, A, true, pin_extra_bytes, dev_extra_bytes, &lists);
  if (rc != VSG_OK) return rc;
  T->wc = call.wc;
  call.wc.range_open = false;  // T->wc pops the range now
  T->c = T->wc.c, T->nq = n, T->list_total = (int)lists.entries;
  T->pin_extra = T->wc.bytes() + call.st.total, T->dev_extra = call.dev_used;
  T->d_observed = call.st.dev.observed, T->d_slots = call.st.slots;
  T->d_off = lists.off, T->d_cnt = lists.cnt, T->d_ent = lists.ent;
  T->d_valid = call.st.dev.valid, T->h_valid = call.st.host.valid, T->h_x = call.st.host.x, T->h_y = call.st.host.y;
  return VSG_OK;
}

}  // namespace vsg

extern "C" {

int vsg_mappoints_create(int device, int capacity, vsg_mappoints **out) {
  if (!out || capacity < 1 || capacity > (1 << 24)) return VSG_ERR_INVALID;
  *out = nullptr;
  int rc = VSG_OK;
  ThreadCtx *c = thread_ctx(device, &rc);
  if (!c) return rc;
  vsg_mappoints *mp = new vsg_mappoints();
  mp->device = device, mp->capacity = capacity;
  const size_t C = (size_t)capacity;
  Stage st;
  const size_t oD = st.add(C * 32), oP = st.add(C * 12), oN = st.add(C * 12), oMin = st.add(C * 4), oMax = st.add(C * 4),
               oO = st.add(C);
  // zeroed on the calling thread's own stream and waited for (see vsg_frame_create)
  if (hipMalloc((void **)&mp->d_block, st.total) != hipSuccess ||
      hipMemsetAsync(mp->d_block, 0, st.total, c->stream) != hipSuccess ||
      hipStreamSynchronize(c->stream) != hipSuccess) {
    if (mp->d_block) hipFree(mp->d_block);
    delete mp;
    return VSG_ERR_HIP;
  }
  mp->d_desc = mp->d_block + oD;
  mp->d_pos = (float *)(mp->d_block + oP), mp->d_normal = (float *)(mp->d_block + oN);
  mp->d_min = (float *)(mp->d_block + oMin), mp->d_max = (float *)(mp->d_block + oMax);
  mp->d_observed = mp->d_block + oO;
  mp->stamp.assign(C, 0u);
  *out = mp;
  return VSG_OK;
}

void vsg_mappoints_destroy(vsg_mappoints *mp) {
  if (!mp) return;
  hipSetDevice(mp->device);
  hipFree(mp->d_block);
  delete mp;
}

int vsg_mappoints_capacity(const vsg_mappoints *mp) { return mp ? mp->capacity : VSG_ERR_INVALID; }

int vsg_mappoints_update(vsg_mappoints *mp, int n, const int32_t *slots, const float *world_pos, const float *normal,
                         const float *min_dist, const float *max_dist, const uint8_t *desc, const uint8_t *observed) {
  if (store_check(mp) != VSG_OK || n < 0) return VSG_ERR_INVALID;
  if (n == 0) return VSG_OK;
  if (!slots) return VSG_ERR_INVALID;
  const size_t N = (size_t)n;
  const CopyLayout L(N, world_pos, normal, min_dist, max_dist, desc, observed);
  ThreadCtx *c = nullptr;
  int rc = copy_begin(mp, n, slots, L, &c);
  if (rc != VSG_OK) return rc;
  uint8_t *hp = c->h_pin, *dp = c->d_pin;
  int32_t *hs = (int32_t *)(hp + L.oS);
  memcpy(hs, slots, N * 4);
  {
    // a slot listed twice takes its last entry: earlier ones are dropped here (two lanes storing to one slot would race)
    std::lock_guard<std::mutex> lock(mp->mutex);
    if (++mp->epoch == 0) std::fill(mp->stamp.begin(), mp->stamp.end(), 0u), mp->epoch = 1;
    for (int i = n - 1; i >= 0; i--) {
      if (mp->stamp[hs[i]] == mp->epoch)
        hs[i] = -1;
      else
        mp->stamp[hs[i]] = mp->epoch;
    }
  }
  if (world_pos) memcpy(hp + L.oP, world_pos, N * 12);
  if (normal) memcpy(hp + L.oN, normal, N * 12);
  if (min_dist) memcpy(hp + L.oMin, min_dist, N * 4);
  if (max_dist) memcpy(hp + L.oMax, max_dist, N * 4);
  if (desc) memcpy(hp + L.oD, desc, N * 32);
  if (observed) memcpy(hp + L.oO, observed, N);
  const FieldsIn A = {(const int32_t *)(dp + L.oS),
                      world_pos ? (const float *)(dp + L.oP) : nullptr,
                      normal ? (const float *)(dp + L.oN) : nullptr,
                      min_dist ? (const float *)(dp + L.oMin) : nullptr,
                      max_dist ? (const float *)(dp + L.oMax) : nullptr,
                      desc ? dp + L.oD : nullptr,
                      observed ? dp + L.oO : nullptr};
  hipLaunchKernelGGL(k_mappoints_scatter, dim3((n + 255) / 256), dim3(256), 0, c->stream, store_dev(mp), A, n);
  return copy_end(c);
}

int vsg_mappoints_read(vsg_mappoints *mp, int n, const int32_t *slots, float *world_pos, float *normal, float *min_dist,
                       float *max_dist, uint8_t *desc, uint8_t *observed) {
  if (store_check(mp) != VSG_OK || n < 0) return VSG_ERR_INVALID;
  if (n == 0) return VSG_OK;
  if (!slots) return VSG_ERR_INVALID;
  const size_t N = (size_t)n;
  const CopyLayout L(N, world_pos, normal, min_dist, max_dist, desc, observed);
  ThreadCtx *c = nullptr;
  int rc = copy_begin(mp, n, slots, L, &c);
  if (rc != VSG_OK) return rc;
  uint8_t *hp = c->h_pin, *dp = c->d_pin;
  memcpy(hp + L.oS, slots, N * 4);
  const FieldsOut A = {(const int32_t *)(dp + L.oS),
                       world_pos ? (float *)(dp + L.oP) : nullptr,
                       normal ? (float *)(dp + L.oN) : nullptr,
                       min_dist ? (float *)(dp + L.oMin) : nullptr,
                       max_dist ? (float *)(dp + L.oMax) : nullptr,
                       desc ? dp + L.oD : nullptr,
                       observed ? dp + L.oO : nullptr};
  hipLaunchKernelGGL(k_mappoints_gather, dim3((n + 255) / 256), dim3(256), 0, c->stream, store_dev(mp), A, n);
  rc = copy_end(c);
  if (rc != VSG_OK) return rc;
  if (world_pos) memcpy(world_pos, hp + L.oP, N * 12);
  if (normal) memcpy(normal, hp + L.oN, N * 12);
  if (min_dist) memcpy(min_dist, hp + L.oMin, N * 4);
  if (max_dist) memcpy(max_dist, hp + L.oMax, N * 4);
  if (desc) memcpy(desc, hp + L.oD, N * 32);
  if (observed) memcpy(observed, hp + L.oO, N);
  return VSG_OK;
}

int vsg_mappoints_refresh_from_observations(vsg_mappoints *mp, int n, const int32_t *slots, const int32_t *obs_off,
                                            const int32_t *obs_kf, const int32_t *obs_idx, const uint8_t *obs_bad,
                                            const int32_t *ref_pos, int n_kf, vsg_frame *const *kfs, const float *kf_Ow,
                                            const float *scale_factors, int nlevels, int what, int32_t *best,
                                            float *normal, float *min_dist, float *max_dist) {
  if (store_check(mp) != VSG_OK || n < 0 || n_kf < 0 || !scale_factors) return VSG_ERR_INVALID;
  if (what < 1 || what > (VSG_REFRESH_DESC | VSG_REFRESH_NORMAL)) return VSG_ERR_INVALID;
  if (n_kf > 0 && (!kfs || !kf_Ow)) return VSG_ERR_INVALID;
  for (int k = 0; k < n_kf; k++)
    if (frame_check(kfs[k]) != VSG_OK || kfs[k]->device != mp->device) return VSG_ERR_INVALID;
  for (int k = 0; k < n_kf; k++)  // GetRightCameraCenter, mvKeysRight (:475-481, :494-501)
    if (kfs[k]->nleft != -1) return VSG_ERR_UNSUPPORTED;
  std::vector<int32_t> kf_n((size_t)n_kf), good;
  std::vector<const vsg_keypoint *> kf_kps((size_t)n_kf);
  for (int k = 0; k < n_kf; k++) {
    const size_t have = kfs[k]->h_kps.size();
    kf_n[(size_t)k] = (int32_t)((size_t)kfs[k]->n < have ? (size_t)kfs[k]->n : have);
    kf_kps[(size_t)k] = kfs[k]->h_kps.data();
  }
  const ObsView view = {n,    slots,       obs_off,       obs_kf,       obs_idx, obs_bad, ref_pos,
                        n_kf, kf_n.data(), kf_kps.data(), mp->capacity, nlevels};
  int rc = obs_check(view, &good);
  if (rc != VSG_OK || n == 0) return rc;
  // everything the kernels index has been bounded; nothing has been enqueued
  ThreadCtx *c = thread_ctx(mp->device, &rc);
  if (!c) return rc;
  const size_t N = (size_t)n, T = (size_t)obs_off[n], K = (size_t)n_kf;
  Stage st;
  const size_t oTab = st.add(K * sizeof(KfEntry)), oS = st.add(N * 4), oOff = st.add((N + 1) * 4), oKf = st.add(T * 4),
               oIdx = st.add(T * 4), oBad = st.add(obs_bad ? T : 0), oRef = st.add(N * 4), oOrd = st.add(N * 4);
  const size_t in_bytes = st.total;
  const size_t oBest = st.add(N * 4), oNrm = st.add(N * 12), oMin = st.add(N * 4), oMax = st.add(N * 4);
  rc = ctx_reserve(c, st.total, in_bytes);
  if (rc != VSG_OK) return rc;
  uint8_t *hp = c->h_pin, *dv = c->d_buf, *dp = c->d_pin;
  KfEntry *tab = (KfEntry *)(hp + oTab);
  for (size_t k = 0; k < K; k++) {  // the frames' pointers as they are NOW
    tab[k].desc = kfs[k]->d_desc, tab[k].kps = kfs[k]->d_kps, tab[k].pad = 0;
    tab[k].Ow[0] = kf_Ow[3 * k], tab[k].Ow[1] = kf_Ow[3 * k + 1], tab[k].Ow[2] = kf_Ow[3 * k + 2];
  }
  memcpy(hp + oS, slots, N * 4);
  memcpy(hp + oOff, obs_off, (N + 1) * 4);
  if (T) memcpy(hp + oKf, obs_kf, T * 4), memcpy(hp + oIdx, obs_idx, T * 4);
  if (T && obs_bad) memcpy(hp + oBad, obs_bad, T);
  if (ref_pos)
    memcpy(hp + oRef, ref_pos, N * 4);
  else
    memset(hp + oRef, 0, N * 4);
  // points of at most 64 candidates first (one wavefront each), then those of 65 .. 128 (one workgroup each)
  static_assert(kObsMaxCandidates == 128, "k_refresh<128, 1> holds the longest list obs_check accepts");
  int32_t *ord = (int32_t *)(hp + oOrd);
  int n_small = 0;
  for (int i = 0; i < n; i++)
    if (good[(size_t)i] <= 64) ord[n_small++] = i;
  int n_all = n_small;
  for (int i = 0; i < n; i++)
    if (good[(size_t)i] > 64) ord[n_all++] = i;
  TRY_HIP(hipMemcpyAsync(dv, hp, in_bytes, hipMemcpyHostToDevice, c->stream));
  RefreshArgs A;
  memset(&A, 0, sizeof(A));
  A.table = (const KfEntry *)(dv + oTab), A.order = (const int32_t *)(dv + oOrd), A.slots = (const int32_t *)(dv + oS);
  A.off = (const int32_t *)(dv + oOff), A.kf = (const int32_t *)(dv + oKf), A.idx = (const int32_t *)(dv + oIdx);
  A.bad = obs_bad ? dv + oBad : nullptr, A.ref_pos = (const int32_t *)(dv + oRef);
  A.what = what, A.nlevels = nlevels;
  for (int l = 0; l < nlevels; l++) A.scale_factors[l] = scale_factors[l];
  A.best = (int32_t *)(dp + oBest), A.normal = (float *)(dp + oNrm);
  A.min_dist = (float *)(dp + oMin), A.max_dist = (float *)(dp + oMax);
  if (n_small > 0) {
    A.first = 0, A.count = n_small;
    hipLaunchKernelGGL((k_refresh<64, 4>), dim3((n_small + 3) / 4), dim3(256), 0, c->stream, store_dev(mp), A);
  }
  if (n_all > n_small) {
    A.first = n_small, A.count = n_all - n_small;
    hipLaunchKernelGGL((k_refresh<128, 1>), dim3(n_all - n_small), dim3(128), 0, c->stream, store_dev(mp), A);
  }
  rc = copy_end(c);
  if (rc != VSG_OK) return rc;
  if (best) memcpy(best, hp + oBest, N * 4);
  if (normal) memcpy(normal, hp + oNrm, N * 12);
  if (min_dist) memcpy(min_dist, hp + oMin, N * 4);
  if (max_dist) memcpy(max_dist, hp + oMax, N * 4);
  return VSG_OK;
}

int vsg_frame_is_in_frustum(vsg_frame *F, vsg_mappoints *mp, int n, const int32_t *slots, const vsg_frame_pose *pose,
                            float viewing_cos_limit, uint8_t *in_view, float *proj_x, float *proj_y, float *proj_xr,
                            float *depth, int32_t *scale_level, float *view_cos) {
  int rc = resident_check(F, mp, pose, n, true, false, nullptr, 0);
  if (rc != VSG_OK || n == 0) return rc;
  ThreadCtx *c = thread_ctx(F->device, &rc);
  if (!c) return rc;
  PointStage st;
  st.lay_out(n, slots, nullptr, kXr | kDepth | kLevel | kViewCos);
  rc = ctx_reserve(c, st.total, 0);
  if (rc != VSG_OK) return rc;
  if (!slots_in_store(mp, n, slots)) return VSG_ERR_INVALID;
  st.bind(c->h_pin, c->d_pin);
  PointArgs A = point_args(F, pose, n);
  A.viewing_cos_limit = viewing_cos_limit;
  launch_frustum({st.slots, st.skip, st.dev, nullptr, nullptr, c->stream}, mp, A);
  const hipError_t e1 = hipGetLastError(), e2 = hipStreamSynchronize(c->stream);
  if (e1 != hipSuccess || e2 != hipSuccess) return VSG_ERR_HIP;
  PointOut dst = {};
  dst.valid = in_view, dst.x = proj_x, dst.y = proj_y, dst.xr = proj_xr, dst.depth = depth;
  dst.level = scale_level, dst.view_cos = view_cos;
  st.copy_out(dst);
  return VSG_OK;
}

int vsg_frame_search_local_points(vsg_frame *F, vsg_mappoints *mp, int n, const int32_t *slots, const uint8_t *skip,
                                  const vsg_frame_pose *pose, float viewing_cos_limit, float th, float nnratio,
                                  int far_points, float th_far_points, const float *scale_factors, int nlevels,
                                  uint8_t *train_blocked, int32_t *train_match, uint8_t *in_view, float *proj_x,
                                  float *proj_y, int *n_to_match) {
  int rc = resident_check(F, mp, pose, n, train_blocked && train_match, true, scale_factors, nlevels);
  if (rc != VSG_OK) return rc;
  if (n_to_match) *n_to_match = 0;
  if (n == 0) return 0;
  if (!slots_in_store(mp, n, slots)) return VSG_ERR_INVALID;
  const PointArgs A = local_point_args(F, pose, n, viewing_cos_limit, th, far_points, th_far_points, scale_factors, nlevels);
  PointOut dst = {};
  dst.valid = in_view, dst.x = proj_x, dst.y = proj_y;
  return with_retry([&]() -> int {
    ResidentCall call;
    rc = local_enqueue(call, F, mp, n, slots, skip, A);
    if (rc == VSG_OK) rc = call.wc.finish();
    if (rc != VSG_OK) return rc;
    const PointOut &h = call.st.host;
    int to_match = 0;
    for (int i = 0; i < n; i++) to_match += h.valid[i];
    if (n_to_match) *n_to_match = to_match;
    call.st.copy_out(dst);
    // a point that is in view but too far has an empty list: the pass does nothing for it, as :53-54
    return walk::search_local(call.wc.lists(), n, -1, h.valid, nullptr, nullptr, h.observed, nnratio, nullptr, nullptr,
                              train_blocked, train_match);
  });
}

int vsg_frame_search_last_frame(vsg_frame *cur, vsg_frame *last, vsg_mappoints *mp, const int32_t *last_slots,
                                const vsg_frame_pose *cur_pose, const vsg_frame_pose *last_pose, float mb, int mono,
                                float th, const float *scale_factors, int nlevels, int check_orientation,
                                uint8_t *train_blocked, int32_t *train_match, int *direction, uint8_t *projected, float *u,
                                float *v, float *ur) {
  if (!last || !last->d_block || !last_pose || !last_slots) return VSG_ERR_INVALID;
  const int n = last->n;
  int rc = resident_check(cur, mp, cur_pose, n, train_blocked && train_match, true, scale_factors, nlevels);
  if (rc != VSG_OK) return rc;
  if (last->nleft != -1) return VSG_ERR_UNSUPPORTED;  // the right-camera block (ORBmatcher.cc:1785-1853)
  if (last->device != cur->device) return VSG_ERR_INVALID;
  const int dir = motion_direction(*cur_pose, *last_pose, mb, mono ? 1 : 0);  // :1677-1684
  const vsg_keypoint *lk = last->h_kps.data();
  for (int i = 0; i < n; i++) {  // before the first enqueue
    if (last_slots[i] >= mp->capacity) return VSG_ERR_INVALID;
    if (last_slots[i] >= 0 && (lk[i].octave < 0 || lk[i].octave >= nlevels)) return VSG_ERR_INVALID;
  }
  if (direction) *direction = dir;  // after the checks: an invalid call writes nothing
  if (n == 0) return 0;
  PointArgs A = point_args(cur, cur_pose, n, kFrameBounds, th, scale_factors, nlevels);
  A.direction = dir;
  PointOut dst = {};
  dst.valid = projected, dst.x = u, dst.y = v, dst.xr = ur;
  std::vector<float> last_angle;  // kpLF.angle (:1768)
  if (check_orientation) {
    last_angle.resize((size_t)n);
    for (int i = 0; i < n; i++) last_angle[i] = lk[i].angle;
  }
  return with_retry([&]() -> int {
    ResidentCall call;
    // the stereo gate of :1742-1748 applies to frames with mvuRight (Nleft == -1 here)
    rc = call.run(cur, n, last_slots, nullptr, kXr | kObserved, resident_lists(cur->has_uright ? kGateUr : kGateNone),
                  [&](const ResidentDev &R) { launch_project<kProjLast>(R, mp, last, A); });
    if (rc != VSG_OK) return rc;
    call.st.copy_out(dst);
    const vsg_keypoint *hk = cur->h_kps.data();
    // a feature without a map point, an outlier and a point that does not project have empty lists: the pass does nothing
    // for them, as the `continue`s of :1689-1709
    return walk::search_last(call.wc.lists(), n, -1, last_angle.data(), call.st.host.observed,
                             [&](int i) { return hk[i].angle; }, walk::TH_HIGH, check_orientation != 0, train_blocked,
                             train_match);
  });
}

int vsg_frame_search_keyframe_points(vsg_frame *cur, vsg_mappoints *mp, int n, const int32_t *slots, const uint8_t *skip,
                                     const vsg_frame_pose *pose, float th, int orb_dist, const float *scale_factors,
                                     int nlevels, int check_orientation, const float *kf_angle, uint8_t *occupied,
                                     int32_t *train_match, uint8_t *projected, float *u, float *v,
                                     int32_t *predicted_level) {
  int rc = resident_check(cur, mp, pose, n, occupied && train_match && !(check_orientation && n > 0 && !kf_angle), true,
                          scale_factors, nlevels);
  if (rc != VSG_OK || n == 0) return rc;
  if (!slots || !slots_in_store(mp, n, slots)) return VSG_ERR_INVALID;
  const PointArgs A = point_args(cur, pose, n, kFrameBounds, th, scale_factors, nlevels);
  const PointOut dst = keyframe_outs(projected, u, v, nullptr, predicted_level);
  return with_retry([&]() -> int {
    ResidentCall call;  // (this search has no stereo gate)
    rc = call.run(cur, n, slots, skip, kLevel, resident_lists(kGateNone),
                  [&](const ResidentDev &R) { launch_project<kProjReloc>(R, mp, nullptr, A); });
    if (rc != VSG_OK) return rc;
    call.st.copy_out(dst);
    const vsg_keypoint *hk = cur->h_kps.data();
    return walk::search_kf_projection(call.wc.lists(), n, kf_angle, [&](int i) { return hk[i].angle; }, orb_dist,
                                      check_orientation != 0, occupied, train_match);
  });
}

int vsg_frame_fuse_points(vsg_frame *kf, vsg_mappoints *mp, int n, const int32_t *slots, const uint8_t *skip,
                          const vsg_frame_pose *pose, float th, const float *scale_factors,
                          const float *inv_level_sigma2, int nlevels, int32_t *best_idx, int32_t *best_dist,
                          uint8_t *projected, float *u, float *v, float *ur, int32_t *predicted_level) {
  bool go;
  const int rc = keyframe_check(kf, mp, n, slots, pose, scale_factors, nlevels,
                                best_idx && best_dist && inv_level_sigma2, &go);
  if (rc != VSG_OK || !go) return rc;
  // the chi-square gate of :1269-1293 reads mvuRight where the KeyFrame has it; bestDist starts at 256 (:1255)
  return fuse_points(kf, mp, n, slots, skip, pose, th, scale_factors, nlevels,
                     {kWinBest, kGateChi2, 256, inv_level_sigma2, nlevels}, best_idx, best_dist,
                     keyframe_outs(projected, u, v, ur, predicted_level));
}

int vsg_frame_fuse_points_sim3(vsg_frame *kf, vsg_mappoints *mp, int n, const int32_t *slots, const uint8_t *skip,
                               const vsg_frame_pose *pose, float th, const float *scale_factors, int nlevels,
                               int32_t *best_idx, int32_t *best_dist, uint8_t *projected, float *u, float *v,
                               int32_t *predicted_level) {
  bool go;
  const int rc = keyframe_check(kf, mp, n, slots, pose, scale_factors, nlevels, best_idx && best_dist, &go);
  if (rc != VSG_OK || !go) return rc;
  // no gate; bestDist starts at INT_MAX (:1406)
  return fuse_points(kf, mp, n, slots, skip, pose, th, scale_factors, nlevels,
                     {kWinBest, kGateNone, 0x7FFFFFFF, nullptr, 0}, best_idx, best_dist,
                     keyframe_outs(projected, u, v, nullptr, predicted_level));
}

int vsg_frame_search_sim3_points(vsg_frame *kf, vsg_mappoints *mp, int n, const int32_t *slots, const uint8_t *skip,
                                 const vsg_frame_pose *pose, float th, float ratio_hamming, const float *scale_factors,
                                 int nlevels, int32_t *matched, uint8_t *projected, float *u, float *v,
                                 int32_t *predicted_level) {
  bool go;
  int rc = keyframe_check(kf, mp, n, slots, pose, scale_factors, nlevels, matched != nullptr, &go);
  if (rc != VSG_OK || !go) return rc;
  const PointArgs A = point_args(kf, pose, n, kKeyFrameBounds, th, scale_factors, nlevels);
  const PointOut dst = keyframe_outs(projected, u, v, nullptr, predicted_level);
  return with_retry([&]() -> int {
    ResidentCall call;
    rc = call.run(kf, n, slots, skip, kXr | kLevel, resident_lists(kGateNone),
                  [&](const ResidentDev &R) { launch_project<kProjKeyFrame>(R, mp, nullptr, A); });
    if (rc != VSG_OK) return rc;
    call.st.copy_out(dst);
    // a point that does not pass :446-483 has an empty list: the pass does nothing for it (:490-491)
    return walk::search_sim3_projection(call.wc.lists(), n, ratio_hamming, matched);
  });
}

}  // extern "C"
