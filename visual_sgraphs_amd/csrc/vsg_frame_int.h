// vsg_frame_int.h -- internal layout of a device-resident Frame / KeyFrame feature set (include/vsg_orb.h: vsg_frame)
// and the window-search launcher (vsg_window.hip), shared by vsg_frame.hip, vsg_window.hip, vsg_mappoints.hip,
// vsg_match.hip, vsg_bow.hip and vsg_orb.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/vsg_orb.h"
#include "vsg_common.h"
#include "vsg_ctx.h"
#include "vsg_walks.h"
#include "vsg_windows.h"

enum { kGridCols = 64, kGridRows = 48, kGridCells = kGridCols * kGridRows };  // FRAME_GRID_COLS / ROWS (Frame.h:49-50)
enum { kGridLdsMax = 4096 };  // keypoints per frame up to which k_frame_grid_build orders the cells in LDS

namespace vsg {
// One entry of a grid cell's vector (mGrid[ix][iy][j], Frame.h:290) with the keypoint fields GetFeaturesInArea tests
// stored inline: a window walk reads cell_start -> entries and never chases the keypoint array.
struct GridEnt {
  float x, y;   // kpUn.pt
  uint32_t io;  // feature index (grid-local) | octave << 16
};
}  // namespace vsg

// What the searches read of one Frame (Frame.h:280-290) or KeyFrame, resident on the device.
struct vsg_frame {
  int device = 0, capacity = 0;
  int n = 0, nleft = -1;  // N, Nleft (right-camera features are [nleft, n))
  bool has_uright = false;
  float minX = 0, minY = 0, maxX = 0, maxY = 0, invW = 0, invH = 0;  // mnMinX.., mfGridElementWidthInv / HeightInv
  uint8_t *d_block = nullptr;  // one allocation behind all of the pointers below
  vsg::KeyPointPOD *d_kps = nullptr;
  uint8_t *d_desc = nullptr;
  float *d_uright = nullptr;
  int *d_cell_start[2] = {nullptr, nullptr};  // [0] mGrid, [1] mGridRight: CSR over cells ix * 48 + iy
  vsg::GridEnt *d_ent[2] = {nullptr, nullptr};
  std::vector<vsg_keypoint> h_kps;  // host mirror (angle / octave for the ordered host passes)
  // Frame::mFeatVec (Frame.h:196), resident since round 6: written by the assembly kernel of ComputeBoW (vsg_bow.hip), or for
  // frames of more than kAsmMax features copied up after the host assembly; joined with another frame's by the SearchByBoW
  // kernels without a host round trip.  hdr = {nodes, features listed}
  int *d_fv_hdr = nullptr, *d_fv_node = nullptr, *d_fv_off = nullptr, *d_fv_idx = nullptr;
  bool fv_valid = false;  // a ComputeBoW of the CURRENT features has been enqueued on the owning thread's stream
  bool fv_empty = false;  // ... and it left no node (no features, or an empty() vocabulary): the device copy is not written
  int fv_bound = 0;       // upper bound of the FeatureVector's node count (what the join kernels launch for)
  // Optimizer::PoseOptimization (vsg_pose.hip): the compacted edges, their last errors, the estimate and the flags of a
  // call, allocated on first use.  pose_held: a call stopped after round 2's optimize and the CURRENT features are still
  // the ones its edges were gathered from; pose_feat[e] = the feature of edge e.
  uint8_t *d_pose = nullptr;
  bool pose_held = false;
  std::vector<int32_t> pose_feat;
  // CreateNewMapPoints (vsg_triangulate.hip): any_stereo = some mvuRight of the CURRENT features may be >= 0 (known for an
  // uploaded array, assumed for one the device computed); d_stereo = {x3Dc, cos parallax} per feature, allocated by the
  // first vsg_frame_set_stereo_points; stereo_attached: it holds the current features' values (every upload drops it)
  bool any_stereo = false, stereo_attached = false;
  float4 *d_stereo = nullptr;
};

namespace vsg {

// device view of a frame, passed to kernels by value
struct FrameDev {
  const KeyPointPOD *kps;
  const uint8_t *desc;
  const float *uright;  // nullptr: every mvuRight is -1
  const int *cell_start[2];
  const GridEnt *ent[2];
  int n, nleft;
  float minX, minY, invW, invH;
};
FrameDev frame_dev(const vsg_frame *f);
// the frame's resident FeatureVector as the node-search kernels take it (vsg_match.hip): hdr = {nodes, features listed}
struct FvDev {
  const int *hdr, *node, *off, *idx;
};
inline FvDev fv_dev(const vsg_frame *f) { return FvDev{f->d_fv_hdr, f->d_fv_node, f->d_fv_off, f->d_fv_idx}; }
// what another translation unit may read of a vsg_mappoints store (vsg_mappoints.hip): false = no store
struct StoreView {
  const float *pos;  // GetWorldPos(), [3 * capacity]
  int device, capacity;
};
bool store_view(const vsg_mappoints *mp, StoreView *v);
// every field of a store, for the one kernel outside vsg_mappoints.hip that WRITES points (k_new_points)
struct StoreFields {
  float *pos, *normal, *min_dist, *max_dist;
  uint8_t *desc, *observed;
  int device, capacity;
};
bool store_fields(vsg_mappoints *mp, StoreFields *v);
inline int frame_check(const vsg_frame *f) { return f && f->d_block ? VSG_OK : VSG_ERR_INVALID; }
// a vsg_grid (include/vsg_orb.h) is a vsg_frame behind an opaque name
inline vsg_frame *grid_frame(vsg_grid *g) { return (vsg_frame *)g; }

// inclusive prefix sum over the 64 lanes of a wavefront (k_frame_grid_build, k_window_search)
__device__ __forceinline__ int wave_incl_scan(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, true);   // row_shr:1
  v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, true);   // row_shr:2
  v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, true);   // row_shr:4
  v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, true);   // row_shr:8
  v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, false);  // row_bcast:15 -> rows 1, 3
  v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, false);  // row_bcast:31 -> rows 2, 3
  return v;
}

enum { kWinList = 0, kWinBest = 1 };
enum { kWinInline = 16 };  // entries of a query's inline slot in list mode (vsg_window.hip)
enum { VSG_RETRY = -100 };  // internal: candidate lists overflowed the compact array; the entry point runs again
enum { kGateNone = 0, kGateUr = 1, kGateChi2 = 2 };

// One window-search call on the calling thread's stream: begin() lays the pinned arena out and returns host pointers
// for the caller to fill (queries, descriptors); launch() enqueues the kernel; finish() waits for the stream and, when
// the lists overflowed the compact array, raises the thread's capacity hint and returns VSG_RETRY: the entry point's
// body runs again from begin() (with_retry below).
struct WindowCall {
  ThreadCtx *c = nullptr;
  int nq = 0, mode = kWinList, cap = 0;  // cap: entries the compact candidate array holds (list mode)
  size_t oQ = 0, oD = 0, oOff = 0, oCnt = 0, oOut = 0;
  bool with_desc = true;
  size_t base = 0;  // offset of this call's blocks inside the arena (several calls can share one arena)
  bool range_open = false;  // a roctx range pushed by begin() and not yet popped (every exit path pops exactly once)
  // The chain calls (vsg_track.hip): {start, length} per query and the candidate array at these DEVICE addresses instead of
  // the pinned arena's blocks, for a kernel behind this one to read (nullptr: the pinned arena).  Such a call ends with
  // account(), not finish(): the kernel behind it sums what the waves took from the counter.
  // dev_lists (set before begin()): the pinned arena holds none of the three blocks.
  int *x_off = nullptr, *x_cnt = nullptr;
  uint32_t *x_out = nullptr;
  bool dev_lists = false;
  ~WindowCall();

  int begin(int device, int nq, int mode, bool with_desc, size_t arena_base = 0, size_t arena_extra = 0);
  WinQuery *queries() const { return (WinQuery *)(c->h_pin + base + oQ); }
  uint8_t *desc() const { return c->h_pin + base + oD; }
  int launch(const vsg_frame *f, int gate_mode, int best_init, const float *inv_sigma2, int nlevels,
             const uint8_t *qdesc_dev = nullptr,   // qdesc_dev: query descriptors already on the device
             const WinQuery *q_dev = nullptr);     // q_dev: queries a kernel in front of this one wrote on the device
  int finish();  // waits for the stream; VSG_RETRY when the lists overflowed (list mode)
  // the second half of finish() alone: `total` entries went to the overflow area; VSG_RETRY when that is more than cap
  int account(long long total);
  // launch() then finish(): what an entry point with ONE window kernel does between its fill and its host pass
  int run(const vsg_frame *f, int gate_mode, int best_init = 256, const float *inv_sigma2 = nullptr, int nlevels = 0,
          const uint8_t *qdesc_dev = nullptr) {
    const int rc = launch(f, gate_mode, best_init, inv_sigma2, nlevels, qdesc_dev);
    return rc != VSG_OK ? rc : finish();
  }
  size_t bytes() const;
  size_t out_bytes() const;
  walk::CandView lists() const;
  const int32_t *best() const { return (const int32_t *)(c->h_pin + base + oOut); }  // pairs {idx, dist}
  // Fuse's copy-out of best mode: bestIdx / bestDist per query (no candidate: -1 / the scan's start value); returns
  // how many are within TH_LOW (ORBmatcher.cc:1310 / :1428)
  int best_out(int best_init, int32_t *best_idx, int32_t *best_dist) const {
    const int32_t *b = best();
    int nfused = 0;
    for (int k = 0; k < nq; k++) {
      best_idx[k] = b[2 * k];
      best_dist[k] = b[2 * k] >= 0 ? b[2 * k + 1] : best_init;
      if (b[2 * k] >= 0 && b[2 * k + 1] <= walk::TH_LOW) nfused++;
    }
    return nfused;
  }
};

// Retry loop around a window-search entry point body: a body whose WindowCall::finish() returned VSG_RETRY runs again
// with the larger stride finish() left behind.  window_call_done() closes the thread's call profile
// (vsg_debug_call_profile: the whole entry point's wall time).
void window_call_done();
template <class Body>
int with_retry(Body body) {
  for (int attempt = 0; attempt < 8; attempt++) {
    const int rc = body();
    if (rc != VSG_RETRY) {
      window_call_done();
      return rc;
    }
  }
  return VSG_ERR_CAPACITY;
}

// One ComputeBoW in flight on a thread's arena (vsg_bow.hip): enqueue -> [other work of the same Frame] -> ONE wait -> finish
struct BowCall {
  vsg_vocab *voc = nullptr;
  ThreadCtx *c = nullptr;
  vsg_frame *resident = nullptr;  // the frame whose FeatureVector this call writes (nullptr: none)
  int n = 0, fv_bound = 0;
  bool active = false, device_assembly = false;
  bool uploaded = false;  // finish() enqueued copies of a host-assembled FeatureVector: wait for the stream before the arena is reused
  size_t pin_base = 0, oW = 0, oWord = 0, oNode = 0, oHdr = 0, oBowId = 0, oBowVal = 0, oFvNode = 0, oFvOff = 0, oFvIdx = 0;
};
void bow_sizes(int n, bool host_desc, size_t *pin_bytes, size_t *dev_bytes);
int bow_enqueue(BowCall *b, vsg_vocab *voc, const uint8_t *desc, const uint8_t *d_desc, int n, int levelsup,
                vsg_frame *resident, ThreadCtx *c, size_t pin_base, size_t dev_base);
int bow_finish(BowCall *b, int32_t *bow_ids, double *bow_vals, int bow_cap, int *n_bow, int32_t *fv_node, int32_t *fv_off,
               int32_t *fv_idx, int fv_cap, int *n_fv, int32_t *word_of, int32_t *node_of, double *weight_of);
int vocab_device(const vsg_vocab *v);

// One SearchByBoW on two frames with resident FeatureVectors (vsg_match.hip), in the same two halves
struct BowSearchCall {
  ThreadCtx *c = nullptr;
  vsg_frame *A = nullptr, *B = nullptr;
  int mode = 0, nOut = 0;
  bool active = false;
  size_t pin_base = 0, oOut = 0;
};
void bow_search_sizes(int nA, int nB, int mode, size_t *pin_bytes, size_t *dev_bytes);
int bow_search_enqueue(BowSearchCall *s, int mode, vsg_frame *A, const uint8_t *validA, vsg_frame *B, const uint8_t *validB,
                       float nnratio, ThreadCtx *c, size_t pin_base, size_t dev_base);
int bow_search_finish(BowSearchCall *s, int check_orientation, int32_t *out);

// vsg_frame_search_for_triangulation_epipolar in two halves (vsg_match.hip): the check, then layout + launch on the calling
// thread's arena with room for the caller's own blocks behind the search's
struct EpiSearchArgs {
  vsg_frame *kf1;
  const uint8_t *no_mp1;
  const int32_t *node_id1, *off1, *idx1;
  int nodes1;
  vsg_frame *kf2;
  const uint8_t *no_mp2;
  const int32_t *node_id2, *off2, *idx2;
  int nodes2;
  const float *F12, *ep, *scale_factors2, *level_sigma2_2;
  int nlevels, only_stereo, coarse;
};
struct EpiSearch {
  ThreadCtx *c = nullptr;
  int n1 = 0;
  bool launched = false;      // false: no walk was needed, every match is -1
  size_t oM = 0, oExtra = 0;  // the matches / the caller's block, offsets into the pinned arena
};
int epipolar_search_check(const EpiSearchArgs &a, const int32_t *matches12);
int epipolar_search_enqueue(EpiSearch *s, const EpiSearchArgs &a, size_t extra_bytes);

// view of the handle's outputs of the last extract call (vsg_orb.hip)
struct OrbOutputView {
  const KeyPointPOD *d_kps = nullptr;  // frame `index`
  const uint8_t *d_desc = nullptr;
  const int *d_counts = nullptr;       // {n, monoIndex}
  hipEvent_t done = nullptr;           // recorded after the last kernel of that call
  int device = 0;
};

}  // namespace vsg

int vsg_orb_output_view(vsg_orb *h, int index, vsg::OrbOutputView *v);
int vsg_orb_device_of(const vsg_orb *h);  // the device the handle lives on
// May the device read [p, p + bytes) of caller host memory in place on behalf of h?  The image path's fail-closed
// classification (vsg_orb.hip, "caller host memory the device may touch IN PLACE"); *dev_alias = the device address.
bool vsg_orb_host_direct(const vsg_orb *h, const void *p, size_t bytes, void **dev_alias);
// Work a blocking extract call enqueues on the handle's stream BEHIND its stage chain and in front of the completion event
// the call waits for (vsg_orb_extract_to_frame: the resident frame's grid launch rides in operator()'s one wait).  The
// hook is consumed by the next submit; `v` = frame 0 of that call's outputs.
typedef int (*vsg_post_chain_fn)(void *ctx, hipStream_t stream, const vsg::OrbOutputView &v);
void vsg_orb_set_post_chain(vsg_orb *h, vsg_post_chain_fn fn, void *ctx);
