/* vsg_orb_debug.h -- test and measurement hooks of libvsg_orb.so.  NOT part of the drop-in boundary: nothing a maintainer
 * of the reference binds (INTEGRATION.md does not mention this header); the tests and tools/abi_latency.cpp include it.
 * The symbols are exported by the same library so that the tests exercise the shipped code object. */
#ifndef VSG_ORB_DEBUG_H
#define VSG_ORB_DEBUG_H
#include "vsg_orb.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Test hook: sorts items[0..n) (n <= 2048) by their upper 32 bits with the device code DistributeOctTree uses for
 * `std::sort(vSizeAndPointerToNode...)` (ORBextractor.cc:707): a replay of libstdc++'s introsort whose result --
 * including the order of equal keys -- must equal std::sort's.  Lets tests compare the two directly. */
int vsg_debug_device_sort(int device, uint64_t *items, int n);

/* Measurement hook: wall time in microseconds of the calling thread's last vsg_frame_* window search -- {filling the
 * pinned arena, the launch call, the stream synchronisation (kernel + PCIe), the whole entry point} */
int vsg_debug_call_profile(float us[4]);

/* The five launch forms of the extractor's octree stage (vsg_launch_forms.octree_kernel) */
enum {
  VSG_OCT_BLUR_MEMBATCH = 1,       /* k_octree_blur<kOctMemBatch>: blur fused, few frames, workspace too big for 5 per CU */
  VSG_OCT_BLUR_MEMBATCH_FUSED = 2, /* k_octree_blur<kOctMemBatchFused>: blur fused, every other fused launch */
  VSG_OCT_FEW_MEMBATCH = 3,        /* k_octree_few<kOctMemBatch>: blur on its own stream, few frames per call */
  VSG_OCT_FEW_MEMBATCH_FUSED = 4,  /* k_octree_few<kOctMemBatchFused>: more frames, five workspaces fit a CU's LDS */
  VSG_OCT_STANDALONE = 5           /* k_octree: more frames, workspace too big for five per CU (5 waves, batched sweeps) */
};

/* What the host code chose for the handle's most recent enqueue */
typedef struct vsg_launch_forms {
  int latency_chain;      /* 1: the blocking small-batch path (ingest kernel, records mirrored to pinned memory) */
  int pyramid_tiling;     /* -1: one k_resize launch per level; 0 / 1 / 2: k_pyramid with that tiling */
  int fast_cells_per_wg;  /* k_fast_cells: FAST cells per workgroup */
  int fast_tile_pitch;    /* k_fast_cells: bytes per tile row of the tile class (52 / 68 / 84) */
  int cand_segmented;     /* 1: FAST candidates in per-cell segments; 0: one list per level (a level has > 4096 cells) */
  int fused_blur;         /* the blur's workgroups ride in the octree's launch (k_octree_blur); 0: two streams */
  int octree_kernel;      /* VSG_OCT_* */
  int octree_hist_big;    /* the octree workspace holds the big histogram */
  int octree_label_bytes; /* LDS node-label area of an octree workgroup (0: labels of overflowing levels in global memory) */
  int octree_lead;        /* rows the octree's workgroups run ahead of the blur's in k_octree_blur */
  int self_slots;         /* k_slots not launched: k_orient_desc derives the output slots itself */
  int orient_mirror;      /* k_orient_desc also writes the records into pinned host memory */
  int cus;                /* compute units the FAST cells-per-workgroup gate used */
  int total_cells;        /* FAST cells per frame of the geometry (the gate's other input) */
  int nframes;            /* frames of the batch described */
  int fast_specialised;   /* 1: k_fast_cells<kSeg, kPlain> (no sliver / unfetched-tile staging, no per-level list); 0: general */
} vsg_launch_forms;

/* Test hook: the launch forms of the handle's most recent enqueue (any entry point).  VSG_ERR_INVALID before the first
 * enqueue. */
int vsg_debug_last_launch_forms(vsg_orb *h, vsg_launch_forms *out);

/* Test hook, read-only: the six KeyFrame members the database's queries read and write, as the device holds them for
 * keyframe `kf_id` after everything enqueued so far: query = {mnRelocQuery, mnPlaceRecognitionQuery}, words =
 * {mnRelocWords, mnPlaceRecognitionWords}, score = {mRelocScore, mPlaceRecognitionScore}.  VSG_ERR_INVALID for an id the
 * database never saw (never added, mapped or named as a neighbour); the outputs are then left alone. */
int vsg_debug_kfdb_state(vsg_kfdb *db, uint64_t kf_id, uint64_t query[2], int32_t words[2], float score[2]);

/* Words of the `status` vsg_debug_track_walk hands back: walkdev::Status of csrc/vsg_walks_dev.h as int32 */
enum {
  VSG_WALK_ST_NMATCHES = 0,
  VSG_WALK_ST_N_EDGES = 1,
  VSG_WALK_ST_FLAGS = 2, /* 1: the lists overflowed (nothing else was written), 2: nmatches < min_matches, 4: < 3 edges */
  VSG_WALK_ST_ROUNDS = 3,
  VSG_WALK_ST_OVERFLOW_SUM = 4,
  VSG_WALK_ST_BINS = 5, /* 30 words: claims per rotation bin before the filter */
  VSG_WALK_ST_WORDS = 36
};

/* Test hook: the ordered walk of the two chain calls (k_track_walk: vsg_frame_track_with_motion_model's and
 * vsg_frame_track_local_map's pass between the window search and the pose solve) ALONE, on candidate lists the caller
 * wrote: one launch of the kernel through the chain calls' own launch function on the calling thread's stream and arenas,
 * one wait, then the copies out.
 *   form: 0 the last-frame walk, 1 the local one.  Lists as the window search lays them out: list q is ent[off[q] ..
 *   off[q] + cnt[q]) of n_ent entries in all, a list longer than 16 lies in the overflow area of `cap` entries; off and cnt
 *   are NOT validated here (the kernel does that: a list outside the array ends the call as an overflow).  q_valid,
 *   observed [nq], blocked_in [nf], q_slot [nq], slots_in [nf] and slot_observed [n_slots] may be NULL with the meaning
 *   walkdev::Args gives that; q_angle [nq] and t_angle [nf] are plain float arrays.
 *   Outputs, [nf] each: what the kernel does not write comes back as the caller passed it (edge_feat / edge_slot behind
 *   n_edges; feat_observed without slot_observed; everything but `status` after an overflow).  status: VSG_WALK_ST_WORDS
 *   int32.
 * Before a device is touched, with nothing written: VSG_ERR_INVALID for a NULL among ent, off, cnt, q_angle, t_angle, the
 * outputs and status, a negative count, nf > 32768 (an entry's index field has 15 bits), form outside {0, 1}, and, with
 * slot_observed, a q_slot or slots_in entry outside [-1, n_slots); VSG_ERR_CAPACITY for a shape whose LDS the chain
 * calls refuse.  nq == 0 and nf == 0 are launched. */
int vsg_debug_track_walk(int form, int nq, int nf, int n_ent, const uint32_t *ent, const int32_t *off, const int32_t *cnt,
                         int cap, const uint8_t *q_valid, const uint8_t *observed, const uint8_t *blocked_in,
                         const float *q_angle, const float *t_angle, const int32_t *q_slot, const int32_t *slots_in,
                         const uint8_t *slot_observed, int n_slots, int check_orientation, int min_matches, float nnratio,
                         int32_t *train_match, uint8_t *train_blocked, int32_t *feat_slots, uint8_t *feat_observed,
                         int32_t *edge_feat, int32_t *edge_slot, int32_t *status);

#ifdef __cplusplus
}
#endif
#endif
