// vsg_track_int.h -- the halves of a chain call (vsg_track.hip: vsg_frame_track_with_motion_model,
// vsg_frame_track_local_map)
// that live beside the kernels they enqueue: the projection + window search (vsg_mappoints.hip) with its candidate lists
// left in the DEVICE arena, and the pose optimisation (vsg_pose.hip) taking its edges from the walk kernel's buffer.
// Nothing here waits: the entry point owns the one wait of the call.
#pragma once
#include "vsg_frame_int.h"

namespace vsg {

// What the search half leaves behind.  Pinned arena: [the window call's blocks | the per-query fields | the caller's
// block at pin_extra].  Device arena: [queries | descriptors | off | cnt | candidates | the caller's block at dev_extra].
struct TrackSearch {
  ThreadCtx *c = nullptr;
  WindowCall wc;
  int nq = 0, list_total = 0;
  size_t pin_extra = 0, dev_extra = 0;
  const uint8_t *d_observed = nullptr;  // per query, as the projection kernel wrote it into the pinned arena (device alias)
  const int32_t *d_slots = nullptr;  // the caller's slot list in the pinned arena (device alias; nullptr: slot i)
  const int32_t *d_off = nullptr, *d_cnt = nullptr;  // the lists, device arena
  const uint32_t *d_ent = nullptr;
  // the local-map form: mbTrackInView per query for the walk (device alias), and the host side of the fields the caller
  // may ask for after the wait
  const uint8_t *d_valid = nullptr, *h_valid = nullptr;
  const float *h_x = nullptr, *h_y = nullptr;
};

// vsg_frame_search_last_frame's checks in its order and with its codes; *dir = bForward / bBackward
int track_last_check(const vsg_frame *cur, const vsg_frame *last, const vsg_mappoints *mp, const int32_t *last_slots,
                     const vsg_frame_pose *cur_pose, const vsg_frame_pose *last_pose, float mb, int mono,
                     const float *scale_factors, int nlevels, int *dir);
// k_project_points<kProjLast> and k_window_search on the calling thread's stream
int track_last_enqueue(TrackSearch *T, const vsg_frame *cur, const vsg_frame *last, const vsg_mappoints *mp,
                       const int32_t *last_slots, const vsg_frame_pose *cur_pose, float th, int dir,
                       const float *scale_factors, int nlevels, size_t pin_extra_bytes, size_t dev_extra_bytes);
// vsg_frame_search_local_points' checks in its order and with its codes (its own output arrays apart)
int track_local_check(const vsg_frame *F, const vsg_mappoints *mp, int n, const int32_t *slots, const vsg_frame_pose *pose,
                      const float *scale_factors, int nlevels);
// k_frustum and k_window_search on the calling thread's stream, as vsg_frame_search_local_points launches them.  slots must
// not be nullptr (the walk reads the queries' slots from the staged list); n == 0 enqueues nothing.
int track_local_enqueue(TrackSearch *T, const vsg_frame *F, const vsg_mappoints *mp, int n, const int32_t *slots,
                        const uint8_t *skip, const vsg_frame_pose *pose, float viewing_cos_limit, float th, int far_points,
                        float th_far_points, const float *scale_factors, int nlevels, size_t pin_extra_bytes,
                        size_t dev_extra_bytes);
const uint8_t *store_observed_dev(const vsg_mappoints *mp);  // Observations() > 0 per slot, on the device

// The solve half.  Pinned block of pose_chain_bytes(nf) at pin_base: [flags | chi2 | result header].
size_t pose_chain_bytes(int nf);
// k_pose_optimize behind the walk kernel: n_edges, (feat, slot) and the status word come from the walk's device buffer
// (status[1] = n_edges, status[2] != 0: the kernel writes its header and returns).
int pose_chain_enqueue(vsg_frame *F, ThreadCtx *c, const StoreView &S, const int32_t *d_edge_feat,
                       const int32_t *d_edge_slot, const int32_t *d_status, const vsg_pose_se3 *Tcw,
                       const vsg_frame_pose *cam, const float *inv_level_sigma2, int nlevels, int hold_round,
                       size_t pin_base);
// after the wait: F->pose_feat from the edge list read back, outlier / chi2 per feature, res; returns n_initial - n_bad
// (0 when held)
int pose_chain_finish(vsg_frame *F, ThreadCtx *c, size_t pin_base, const int32_t *h_edge_feat, int n_edges,
                      uint8_t *outlier, float *chi2, vsg_pose_result *res);
// what vsg_frame_pose_optimization returns without enqueueing anything (fewer than 3 edges, :1251)
void pose_result_input(const vsg_pose_se3 *Tcw, int n_edges, vsg_pose_result *res);

}  // namespace vsg
