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
#include "vsg_project.h"

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

struct FrustumArgs {
  vsg_frame_pose cam;
  float minX, maxX, minY, maxY, viewing_cos_limit;
  int n;
  // the search half (Q == nullptr: isInFrustum alone)
  int b_factor, far_points;
  float th, th_far_points;
  float scale_factors[16];
};

struct FrustumOutDev {
  uint8_t *in_view;
  float *proj_x, *proj_y, *proj_xr, *depth;  // proj_xr, depth, scale_level, view_cos: nullptr when not wanted
  int32_t *scale_level;
  float *view_cos;
  uint8_t *observed;  // Observations() > 0 of point i, for the ordered host pass (nullptr when not wanted)
};

// Frame::isInFrustum, one lane per map point i = slot slots[i] (nullptr: slot i).  skip[i]: never projected (in_view 0,
// proj -1).  With Q: the window of SearchByProjection(F, vpMapPoints) (ORBmatcher.cc:59-70) as a WinQuery and the
// point's descriptor at qdesc[32 i]; a point that is not searched gets the inactive flag and no descriptor.
// k_window_search loads qdesc[32 q] of every query before it looks at the flag, so for those points it reads 32 bytes of the
// arena that this call never wrote: in bounds (n * 32 bytes are reserved), and the value is never used -- an inactive
// query has no candidates to compare it with.  Not a value to rely on, and not a read for a checker to flag.
// 64 lanes per workgroup: 4000 points are 63 workgroups on 63 CUs, each running the fp64 logf once.
__global__ __launch_bounds__(64) void k_frustum(StoreDev S, const int32_t *__restrict__ slots,
                                                const uint8_t *__restrict__ skip, FrustumArgs A, FrustumOutDev O,
                                                WinQuery *__restrict__ Q, uint8_t *__restrict__ qdesc) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= A.n) return;
  const int s = slots ? slots[i] : i;
  FrustumOut o = {0, -1.0f, -1.0f, 0.0f, 0.0f, 0, 0.0f};
  if (!(skip && skip[i])) {
    const float *P = S.pos + 3 * (size_t)s, *N = S.normal + 3 * (size_t)s;
    o = frustum_point(A.cam, A.minX, A.maxX, A.minY, A.maxY, A.viewing_cos_limit, P[0], P[1], P[2], N[0], N[1], N[2],
                      S.min_dist[s], S.max_dist[s]);
  }
  O.in_view[i] = (uint8_t)o.in_view;
  O.proj_x[i] = o.proj_x, O.proj_y[i] = o.proj_y;
  if (O.proj_xr) O.proj_xr[i] = o.proj_xr;
  if (O.depth) O.depth[i] = o.depth;
  if (O.scale_level) O.scale_level[i] = o.scale_level;
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

struct ProjectArgs {
  vsg_frame_pose cam;
  ImageBounds bounds;
  int n;
  float th;
  int direction;  // last-frame form: 0 neither, 1 bForward, 2 bBackward
  float scale_factors[16];
};

struct ProjectOutDev {
  uint8_t *valid;     // the point reaches GetFeaturesInArea
  float *u, *v;
  float *ur;          // last-frame form, into-KeyFrame form
  int32_t *level;     // relocalisation form, into-KeyFrame form
  uint8_t *observed;  // last-frame form: Observations() > 0 of query i's point, for the ordered host pass
};

// The projection loops of SearchByProjection(CurrentFrame, LastFrame) (kLast, ORBmatcher.cc:1686-1724) and of
// SearchByProjection(CurrentFrame, pKF, sAlreadyFound) (ORBmatcher.cc:1895-1930), one lane per query, 64 lanes per
// workgroup like k_frustum.  kProjLast: query i = feature i of the resident last frame, slots[i] < 0 = no map point or an
// outlier, the octave is the last frame's own.  kProjReloc: query i = slot slots[i], skip[i] = isBad() or
// in sAlreadyFound.  kProjKeyFrame: the loop of Fuse x2 and SearchByProjection(pKF, Scw, ...) (ORBmatcher.cc:1194-1241,
// :1360-1395, :452-486), query i = slot slots[i], skip[i] = isBad(), IsInKeyFrame(pKF) or in spAlreadyFound; A.bounds
// are the KeyFrame's truncated ones.  A query that is not searched gets the inactive flag and no descriptor (see k_frustum).
enum { kProjLast = 0, kProjReloc = 1, kProjKeyFrame = 2 };
template <int kForm>
__global__ __launch_bounds__(64) void k_project_points(StoreDev S, const int32_t *__restrict__ slots,
                                                       const uint8_t *__restrict__ skip,
                                                       const KeyPointPOD *__restrict__ last_kps, ProjectArgs A,
                                                       ProjectOutDev O, WinQuery *__restrict__ Q,
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
  O.u[i] = o.u, O.v[i] = o.v;
  if (O.ur) O.ur[i] = o.ur;
  if (O.level) O.level[i] = o.level;
  if (O.observed) O.observed[i] = observed;
  Q[i] = w;
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

int pose_check(const vsg_frame *F, const vsg_mappoints *mp, const vsg_frame_pose *pose) {
  if (!F || !F->d_block || store_check(mp) != VSG_OK || !pose) return VSG_ERR_INVALID;
  if (F->nleft != -1) return VSG_ERR_UNSUPPORTED;  // isInFrustumChecks with KannalaBrandt8 (Frame.cc:721-800)
  if (F->device != mp->device || pose->n_levels < 1) return VSG_ERR_INVALID;
  return VSG_OK;
}

FrustumArgs frustum_args(const vsg_frame *F, const vsg_frame_pose *pose, float viewing_cos_limit, int n) {
  FrustumArgs A;
  memset(&A, 0, sizeof(A));
  A.cam = *pose;
  A.minX = F->minX, A.maxX = F->maxX, A.minY = F->minY, A.maxY = F->maxY;
  A.viewing_cos_limit = viewing_cos_limit;
  A.n = n;
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

// What the six searches on resident map points share: a projection kernel that writes every point's WinQuery and
// gathers its descriptor, k_window_search right behind it on the same stream, one wait.  The call's own blocks
// [slots? | skip? | valid | observed? | x | y | aux? | aux2?] sit behind the window call's in the pinned arena,
// [WinQuery | descriptors] in the device arena.
struct ResidentDev {  // what the projection kernel is launched with: the device side of those blocks and the stream
  const int32_t *slots;
  const uint8_t *skip;
  uint8_t *valid, *observed;
  float *x, *y;
  void *aux;   // one more 4-byte value per point: ur (last-frame form, into-KeyFrame form) / level (relocalisation form)
  void *aux2;  // and another: level (into-KeyFrame form)
  WinQuery *Q;
  uint8_t *qdesc;
  hipStream_t stream;
};
// How the window kernel behind the projection runs: candidate lists for an ordered host pass, or the best candidate per
// query (Fuse) with its scan's start value and, for the chi-square gate, pKF->mvInvLevelSigma2.
struct ResidentMode {
  int mode, gate_mode, best_init;
  const float *inv_sigma2;
  int nlevels;
};
ResidentMode resident_lists(int gate_mode) { return {kWinList, gate_mode, 256, nullptr, 0}; }
struct ResidentCall {
  WindowCall wc;
  size_t oS = 0, oK = 0, oV = 0, oO = 0, oX = 0, oY = 0, oA = 0, oA2 = 0;
  uint8_t *hp = nullptr;  // the call's blocks, host side

  // launch(ResidentDev) enqueues the projection kernel.  VSG_RETRY: the lists overflowed, the whole call runs again
  template <class Launch>
  int run(const vsg_frame *F, int n, const int32_t *slots, const uint8_t *skip, bool observed, bool aux, bool aux2,
          const ResidentMode &M, Launch launch) {
    const size_t N = (size_t)n;
    Stage st, sd;
    oS = st.add(slots ? N * 4 : 0), oK = st.add(skip ? N : 0), oV = st.add(N), oO = st.add(observed ? N : 0);
    oX = st.add(N * 4), oY = st.add(N * 4), oA = st.add(aux ? N * 4 : 0), oA2 = st.add(aux2 ? N * 4 : 0);
    const size_t dQ = sd.add(N * sizeof(WinQuery)), dD = sd.add(N * 32);
    int rc = wc.begin(F->device, n, M.mode, false, 0, st.total);
    if (rc != VSG_OK) return rc;
    ThreadCtx *c = wc.c;
    rc = ctx_reserve(c, 0, sd.total);
    if (rc != VSG_OK) return rc;
    // both reserves first, pointers after: either reserve may move its arena
    hp = c->h_pin + wc.bytes();
    uint8_t *dp = c->d_pin + wc.bytes();
    if (slots) memcpy(hp + oS, slots, N * 4);
    if (skip) memcpy(hp + oK, skip, N);
    const ResidentDev R = {slots ? (const int32_t *)(dp + oS) : nullptr, skip ? dp + oK : nullptr, dp + oV,
                           observed ? dp + oO : nullptr, (float *)(dp + oX), (float *)(dp + oY),
                           aux ? dp + oA : nullptr, aux2 ? dp + oA2 : nullptr, (WinQuery *)(c->d_buf + dQ),
                           c->d_buf + dD, c->stream};
    launch(R);
    rc = hipGetLastError() == hipSuccess ? VSG_OK : VSG_ERR_HIP;
    if (rc == VSG_OK) rc = wc.launch(F, M.gate_mode, M.best_init, M.inv_sigma2, M.nlevels, R.qdesc, R.Q);
    if (rc != VSG_OK) {
      hipStreamSynchronize(c->stream);  // nothing of this call may still write the arena when the next one fills it
      return rc;
    }
    return wc.finish();
  }
  // copy-out of the per-point results the caller asked for
  void outs(int n, uint8_t *valid, float *x, float *y, void *aux, void *aux2 = nullptr) const {
    const size_t N = (size_t)n;
    if (valid) memcpy(valid, hp + oV, N);
    if (x) memcpy(x, hp + oX, N * 4);
    if (y) memcpy(y, hp + oY, N * 4);
    if (aux) memcpy(aux, hp + oA, N * 4);
    if (aux2) memcpy(aux2, hp + oA2, N * 4);
  }
};

template <int kForm>
void launch_project(const ResidentDev &R, const vsg_mappoints *mp, const vsg_frame *last, const ProjectArgs &A) {
  const bool kLast = kForm == kProjLast;
  const ProjectOutDev O = {R.valid, R.x, R.y, kForm != kProjReloc ? (float *)R.aux : nullptr,
                           (int32_t *)(kForm == kProjReloc ? R.aux : kForm == kProjKeyFrame ? R.aux2 : nullptr), R.observed};
  hipLaunchKernelGGL(k_project_points<kForm>, dim3((A.n + 63) / 64), dim3(64), 0, R.stream, store_dev(mp), R.slots,
                     R.skip, kLast ? (const KeyPointPOD *)last->d_kps : (const KeyPointPOD *)nullptr, A, O, R.Q, R.qdesc);
}

// the checks the two projection searches share, in the order of pose_check
int project_check(const vsg_frame *cur, const vsg_mappoints *mp, const vsg_frame_pose *pose, const float *scale_factors,
                  int nlevels, const uint8_t *blocked, const int32_t *train_match) {
  const int rc = pose_check(cur, mp, pose);
  if (rc != VSG_OK) return rc;
  if (!scale_factors || !blocked || !train_match || nlevels < 1 || nlevels > 16 || pose->n_levels > nlevels)
    return VSG_ERR_INVALID;
  return VSG_OK;
}

ProjectArgs project_args(const vsg_frame *cur, const vsg_frame_pose *pose, int n, float th, const float *scale_factors,
                         int nlevels) {
  ProjectArgs A;
  memset(&A, 0, sizeof(A));
  A.cam = *pose;
  A.bounds = {cur->minX, cur->maxX, cur->minY, cur->maxY};
  A.n = n, A.th = th;
  for (int l = 0; l < nlevels; l++) A.scale_factors[l] = scale_factors[l];
  return A;
}

// What the three routines that project into one KeyFrame check, in the order of project_check, BEFORE anything is
// enqueued; outs_ok: the entry's own required arrays are there.  VSG_OK with *go == false: n == 0, the entry returns 0.
int keyframe_check(const vsg_frame *kf, const vsg_mappoints *mp, int n, const int32_t *slots, const vsg_frame_pose *pose,
                   const float *scale_factors, int nlevels, bool outs_ok, bool *go) {
  *go = false;
  const int rc = pose_check(kf, mp, pose);  // Nleft != -1: bRight / mpCamera2 (ORBmatcher.cc:1154-1159)
  if (rc != VSG_OK) return rc;
  if (!scale_factors || !outs_ok || nlevels < 1 || nlevels > 16 || pose->n_levels > nlevels || n < 0)
    return VSG_ERR_INVALID;
  if (n == 0) return VSG_OK;
  if (!slots || !slots_in_store(mp, n, slots)) return VSG_ERR_INVALID;
  *go = true;
  return VSG_OK;
}

// ... and their projection arguments: the bounds are KeyFrame::mnMinX .. mnMaxY, the Frame's truncated to int
ProjectArgs keyframe_args(const vsg_frame *kf, const vsg_frame_pose *pose, int n, float th, const float *scale_factors,
                          int nlevels) {
  ProjectArgs A = project_args(kf, pose, n, th, scale_factors, nlevels);
  A.bounds = keyframe_bounds(A.bounds);
  return A;
}

// Fuse's search on resident points: the projection kernel, then k_window_search in best mode; one wait
int fuse_points(vsg_frame *kf, vsg_mappoints *mp, int n, const int32_t *slots, const uint8_t *skip,
                const vsg_frame_pose *pose, float th, const float *scale_factors, int nlevels, const ResidentMode &M,
                int32_t *best_idx, int32_t *best_dist, uint8_t *projected, float *u, float *v, float *ur,
                int32_t *predicted_level) {
  const ProjectArgs A = keyframe_args(kf, pose, n, th, scale_factors, nlevels);
  ResidentCall call;
  const int rc = call.run(kf, n, slots, skip, false, true, true, M,
                          [&](const ResidentDev &R) { launch_project<kProjKeyFrame>(R, mp, nullptr, A); });
  if (rc != VSG_OK) return rc;
  call.outs(n, projected, u, v, ur, predicted_level);
  const int32_t *b = call.wc.best();
  int nfused = 0;
  for (int k = 0; k < n; k++) {
    best_idx[k] = b[2 * k];
    best_dist[k] = b[2 * k] >= 0 ? b[2 * k + 1] : M.best_init;
    if (b[2 * k] >= 0 && b[2 * k + 1] <= walk::TH_LOW) nfused++;  // :1310 / :1428
  }
  return nfused;
}

}  // namespace

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

int vsg_frame_is_in_frustum(vsg_frame *F, vsg_mappoints *mp, int n, const int32_t *slots, const vsg_frame_pose *pose,
                            float viewing_cos_limit, uint8_t *in_view, float *proj_x, float *proj_y, float *proj_xr,
                            float *depth, int32_t *scale_level, float *view_cos) {
  int rc = pose_check(F, mp, pose);
  if (rc != VSG_OK) return rc;
  if (n < 0) return VSG_ERR_INVALID;
  if (n == 0) return VSG_OK;
  ThreadCtx *c = thread_ctx(F->device, &rc);
  if (!c) return rc;
  const size_t N = (size_t)n;
  Stage st;
  const size_t oS = st.add(slots ? N * 4 : 0), oV = st.add(N), oX = st.add(N * 4), oY = st.add(N * 4),
               oXR = st.add(N * 4), oDp = st.add(N * 4), oL = st.add(N * 4), oC = st.add(N * 4);
  rc = ctx_reserve(c, st.total, 0);
  if (rc != VSG_OK) return rc;
  uint8_t *hp = c->h_pin, *dp = c->d_pin;
  if (!slots_in_store(mp, n, slots)) return VSG_ERR_INVALID;
  if (slots) memcpy(hp + oS, slots, N * 4);
  const FrustumOutDev O = {dp + oV,
                           (float *)(dp + oX),
                           (float *)(dp + oY),
                           (float *)(dp + oXR),
                           (float *)(dp + oDp),
                           (int32_t *)(dp + oL),
                           (float *)(dp + oC),
                           nullptr};
  hipLaunchKernelGGL(k_frustum, dim3((n + 63) / 64), dim3(64), 0, c->stream, store_dev(mp),
                     slots ? (const int32_t *)(dp + oS) : (const int32_t *)nullptr, (const uint8_t *)nullptr,
                     frustum_args(F, pose, viewing_cos_limit, n), O, (WinQuery *)nullptr, (uint8_t *)nullptr);
  const hipError_t e1 = hipGetLastError(), e2 = hipStreamSynchronize(c->stream);
  if (e1 != hipSuccess || e2 != hipSuccess) return VSG_ERR_HIP;
  if (in_view) memcpy(in_view, hp + oV, N);
  if (proj_x) memcpy(proj_x, hp + oX, N * 4);
  if (proj_y) memcpy(proj_y, hp + oY, N * 4);
  if (proj_xr) memcpy(proj_xr, hp + oXR, N * 4);
  if (depth) memcpy(depth, hp + oDp, N * 4);
  if (scale_level) memcpy(scale_level, hp + oL, N * 4);
  if (view_cos) memcpy(view_cos, hp + oC, N * 4);
  return VSG_OK;
}

int vsg_frame_search_local_points(vsg_frame *F, vsg_mappoints *mp, int n, const int32_t *slots, const uint8_t *skip,
                                  const vsg_frame_pose *pose, float viewing_cos_limit, float th, float nnratio,
                                  int far_points, float th_far_points, const float *scale_factors, int nlevels,
                                  uint8_t *train_blocked, int32_t *train_match, uint8_t *in_view, float *proj_x,
                                  float *proj_y, int *n_to_match) {
  int rc = pose_check(F, mp, pose);
  if (rc != VSG_OK) return rc;
  if (n < 0 || !train_blocked || !train_match || !scale_factors || nlevels < 1 || nlevels > 16 ||
      pose->n_levels > nlevels)
    return VSG_ERR_INVALID;
  if (n_to_match) *n_to_match = 0;
  if (n == 0) return 0;
  if (!slots_in_store(mp, n, slots)) return VSG_ERR_INVALID;
  FrustumArgs A = frustum_args(F, pose, viewing_cos_limit, n);
  A.b_factor = th != 1.0;  // ORBmatcher.cc:46
  A.th = th, A.far_points = far_points ? 1 : 0, A.th_far_points = th_far_points;
  for (int l = 0; l < nlevels; l++) A.scale_factors[l] = scale_factors[l];
  return with_retry([&]() -> int {
    ResidentCall call;
    // the stereo gate of :97-102 applies to frames with mvuRight (Nleft == -1 here)
    rc = call.run(F, n, slots, skip, true, false, false, resident_lists(F->has_uright ? kGateUr : kGateNone),
                  [&](const ResidentDev &R) {
                    const FrustumOutDev O = {R.valid, R.x, R.y, nullptr, nullptr, nullptr, nullptr, R.observed};
                    hipLaunchKernelGGL(k_frustum, dim3((n + 63) / 64), dim3(64), 0, R.stream, store_dev(mp), R.slots,
                                       R.skip, A, O, R.Q, R.qdesc);
                  });
    if (rc != VSG_OK) return rc;
    const uint8_t *hv = call.hp + call.oV;
    int to_match = 0;
    for (int i = 0; i < n; i++) to_match += hv[i];
    if (n_to_match) *n_to_match = to_match;
    call.outs(n, in_view, proj_x, proj_y, nullptr);
    // a point that is in view but too far has an empty list: the pass does nothing for it, as :53-54
    return walk::search_local(call.wc.lists(), n, -1, hv, nullptr, nullptr, call.hp + call.oO, nnratio, nullptr, nullptr,
                              train_blocked, train_match);
  });
}

int vsg_frame_search_last_frame(vsg_frame *cur, vsg_frame *last, vsg_mappoints *mp, const int32_t *last_slots,
                                const vsg_frame_pose *cur_pose, const vsg_frame_pose *last_pose, float mb, int mono,
                                float th, const float *scale_factors, int nlevels, int check_orientation,
                                uint8_t *train_blocked, int32_t *train_match, int *direction, uint8_t *projected, float *u,
                                float *v, float *ur) {
  if (!last || !last->d_block || !last_pose || !last_slots) return VSG_ERR_INVALID;
  int rc = project_check(cur, mp, cur_pose, scale_factors, nlevels, train_blocked, train_match);
  if (rc != VSG_OK) return rc;
  if (last->nleft != -1) return VSG_ERR_UNSUPPORTED;  // the right-camera block (ORBmatcher.cc:1785-1853)
  if (last->device != cur->device) return VSG_ERR_INVALID;
  const int dir = motion_direction(*cur_pose, *last_pose, mb, mono ? 1 : 0);  // :1677-1684
  const int n = last->n;
  const vsg_keypoint *lk = last->h_kps.data();
  for (int i = 0; i < n; i++) {  // before the first enqueue
    if (last_slots[i] >= mp->capacity) return VSG_ERR_INVALID;
    if (last_slots[i] >= 0 && (lk[i].octave < 0 || lk[i].octave >= nlevels)) return VSG_ERR_INVALID;
  }
  if (direction) *direction = dir;  // after the checks: an invalid call writes nothing
  if (n == 0) return 0;
  ProjectArgs A = project_args(cur, cur_pose, n, th, scale_factors, nlevels);
  A.direction = dir;
  std::vector<float> last_angle;  // kpLF.angle (:1768)
  if (check_orientation) {
    last_angle.resize((size_t)n);
    for (int i = 0; i < n; i++) last_angle[i] = lk[i].angle;
  }
  return with_retry([&]() -> int {
    ResidentCall call;
    // the stereo gate of :1742-1748 applies to frames with mvuRight (Nleft == -1 here)
    rc = call.run(cur, n, last_slots, nullptr, true, true, false, resident_lists(cur->has_uright ? kGateUr : kGateNone),
                  [&](const ResidentDev &R) { launch_project<kProjLast>(R, mp, last, A); });
    if (rc != VSG_OK) return rc;
    call.outs(n, projected, u, v, ur);
    const vsg_keypoint *hk = cur->h_kps.data();
    // a feature without a map point, an outlier and a point that does not project have empty lists: the pass does nothing
    // for them, as the `continue`s of :1689-1709
    return walk::search_last(call.wc.lists(), n, -1, last_angle.data(), call.hp + call.oO,
                             [&](int i) { return hk[i].angle; }, walk::TH_HIGH, check_orientation != 0, train_blocked,
                             train_match);
  });
}

int vsg_frame_search_keyframe_points(vsg_frame *cur, vsg_mappoints *mp, int n, const int32_t *slots, const uint8_t *skip,
                                     const vsg_frame_pose *pose, float th, int orb_dist, const float *scale_factors,
                                     int nlevels, int check_orientation, const float *kf_angle, uint8_t *occupied,
                                     int32_t *train_match, uint8_t *projected, float *u, float *v,
                                     int32_t *predicted_level) {
  int rc = project_check(cur, mp, pose, scale_factors, nlevels, occupied, train_match);
  if (rc != VSG_OK) return rc;
  if (n < 0 || (check_orientation && n > 0 && !kf_angle)) return VSG_ERR_INVALID;
  if (n == 0) return 0;
  if (!slots || !slots_in_store(mp, n, slots)) return VSG_ERR_INVALID;
  const ProjectArgs A = project_args(cur, pose, n, th, scale_factors, nlevels);
  return with_retry([&]() -> int {
    ResidentCall call;  // (this search has no stereo gate)
    rc = call.run(cur, n, slots, skip, false, true, false, resident_lists(kGateNone),
                  [&](const ResidentDev &R) { launch_project<kProjReloc>(R, mp, nullptr, A); });
    if (rc != VSG_OK) return rc;
    call.outs(n, projected, u, v, predicted_level);
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
  if (rc != VSG_OK) return rc;
  if (!go) return 0;
  // the chi-square gate of :1269-1293 reads mvuRight where the KeyFrame has it; bestDist starts at 256 (:1255)
  return fuse_points(kf, mp, n, slots, skip, pose, th, scale_factors, nlevels,
                     {kWinBest, kGateChi2, 256, inv_level_sigma2, nlevels}, best_idx, best_dist, projected, u, v, ur,
                     predicted_level);
}

int vsg_frame_fuse_points_sim3(vsg_frame *kf, vsg_mappoints *mp, int n, const int32_t *slots, const uint8_t *skip,
                               const vsg_frame_pose *pose, float th, const float *scale_factors, int nlevels,
                               int32_t *best_idx, int32_t *best_dist, uint8_t *projected, float *u, float *v,
                               int32_t *predicted_level) {
  bool go;
  const int rc = keyframe_check(kf, mp, n, slots, pose, scale_factors, nlevels, best_idx && best_dist, &go);
  if (rc != VSG_OK) return rc;
  if (!go) return 0;
  // no gate; bestDist starts at INT_MAX (:1406)
  return fuse_points(kf, mp, n, slots, skip, pose, th, scale_factors, nlevels,
                     {kWinBest, kGateNone, 0x7FFFFFFF, nullptr, 0}, best_idx, best_dist, projected, u, v, nullptr,
                     predicted_level);
}

int vsg_frame_search_sim3_points(vsg_frame *kf, vsg_mappoints *mp, int n, const int32_t *slots, const uint8_t *skip,
                                 const vsg_frame_pose *pose, float th, float ratio_hamming, const float *scale_factors,
                                 int nlevels, int32_t *matched, uint8_t *projected, float *u, float *v,
                                 int32_t *predicted_level) {
  bool go;
  int rc = keyframe_check(kf, mp, n, slots, pose, scale_factors, nlevels, matched != nullptr, &go);
  if (rc != VSG_OK) return rc;
  if (!go) return 0;
  const ProjectArgs A = keyframe_args(kf, pose, n, th, scale_factors, nlevels);
  return with_retry([&]() -> int {
    ResidentCall call;
    rc = call.run(kf, n, slots, skip, false, true, true, resident_lists(kGateNone),
                  [&](const ResidentDev &R) { launch_project<kProjKeyFrame>(R, mp, nullptr, A); });
    if (rc != VSG_OK) return rc;
    call.outs(n, projected, u, v, nullptr, predicted_level);
    // a point that does not pass :446-483 has an empty list: the pass does nothing for it (:490-491)
    return walk::search_sim3_projection(call.wc.lists(), n, ratio_hamming, matched);
  });
}

}  // extern "C"
