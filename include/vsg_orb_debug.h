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

#ifdef __cplusplus
}
#endif
#endif
