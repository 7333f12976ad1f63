/*
 * vsg_orb.h -- C ABI of the MI355X-native ORB front-end (libvsg_orb.so).
 *
 * Drop-in boundary for the per-frame hot path of snt-arg/visual_sgraphs (vS-Graphs on
 * ORB-SLAM3).  Each entry point names the reference interface it replaces (paths relative to
 * the reference tree).  Plain pointers and sizes only; nothing throws across this boundary;
 * every function returns a negative VSG_ERR_* code on failure.  There is NO CPU fallback:
 * without a HIP device every compute entry point fails with VSG_ERR_NO_DEVICE.
 *
 * Threading: a handle is not re-entrant (like one ORBextractor instance, which mutates
 * mvImagePyramid); distinct handles may be used concurrently from different host threads,
 * on the same or different GPUs (the stereo Frame ctor does exactly that, Frame.cc:129-132).
 * Matcher entry points are stateless and thread-safe.
 */
#ifndef VSG_ORB_H
#define VSG_ORB_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VSG_OK 0
#define VSG_ERR_EMPTY_IMAGE (-1)   /* operator() returns -1 on an empty image (ORBextractor.cc:1087-1088) */
#define VSG_ERR_CAPACITY (-2)      /* caller's keypoint/descriptor capacity is too small */
#define VSG_ERR_UNSUPPORTED (-3)   /* parameters/image size the reference itself cannot process, or over a limit */
#define VSG_ERR_NO_DEVICE (-4)     /* no usable HIP device / HIP runtime error at start-up */
#define VSG_ERR_HIP (-5)           /* a HIP call failed; see vsg_last_error() */
#define VSG_ERR_INVALID (-6)       /* bad argument */
#define VSG_ERR_BUSY (-7)          /* submitted batches are still un-waited: vsg_orb_wait them, then retry (nothing to grow) */

/* cv::KeyPoint-compatible record: pt.x pt.y size angle response octave class_id (28 bytes),
 * so a C++ adaptor can memcpy into std::vector<cv::KeyPoint>. */
typedef struct vsg_keypoint {
  float x, y, size, angle, response;
  int32_t octave, class_id;
} vsg_keypoint;

typedef struct vsg_orb vsg_orb; /* one ORBextractor instance + its device buffers and streams */

const char *vsg_last_error(void);   /* thread-local description of the last failure */
int vsg_device_count(void);         /* number of HIP devices, or VSG_ERR_NO_DEVICE */

/* ---- ORBextractor ------------------------------------------------------------------------- */

/* ORBextractor::ORBextractor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST)
 * (ORBextractor.h:51-52, ORBextractor.cc:411-470).  `device` = HIP device ordinal;
 * `max_batch` = frames processed per launch by the batch entry points (>= 1). */
int vsg_orb_create(int nfeatures, float scale_factor, int nlevels, int ini_th_fast, int min_th_fast, int device,
                   int max_batch, vsg_orb **out);
void vsg_orb_destroy(vsg_orb *h);

/* GetLevels/GetScaleFactors/GetInverseScaleFactors/GetScaleSigmaSquares/GetInverseScaleSigmaSquares
 * (ORBextractor.h:63-91) plus mnFeaturesPerLevel and umax[16]; any pointer may be NULL.
 * Returns nlevels.  No device needed. */
int vsg_orb_get_tables(const vsg_orb *h, float *scale, float *inv_scale, float *sigma2, float *inv_sigma2,
                       int *features_per_level, int *umax16);

/* The 7 taps of cv::GaussianBlur(7x7, sigma 2)'s 8.8 fixed-point kernel (ORBextractor.cc:1130).
 * Default {18,34,49,55,49,34,18} (OpenCV 4.2.0 independent rounding); OpenCV >= 4.3 normalises to
 * {18,34,48,56,48,34,18}.  Version-sensitive, hence data. */
int vsg_orb_set_blur_taps(vsg_orb *h, const uint16_t taps[7]);

/* Launch form of ComputePyramid (ORBextractor.cc:1171-1195): -1 (default) = the fused chain kernel with the tiling the
 * handle picks (the one it timed faster for its image size; 16-pixel top tiles for calls of one or two frames),
 * 0 / 1 / 2 = the fused kernel with the 32- / 36- / 16-pixel top-level tiling, 3 = one launch per level.  Every form
 * produces the same bytes (tests/test_gpu_switches.py runs all five against the oracle); the setter exists so that each
 * form stays a tested path instead of an environment switch. */
int vsg_orb_set_pyramid_tiling(vsg_orb *h, int which);

/* Launch form of the per-cell FAST kernel (k_fast_cells): -1 (default) = automatic, the form compiled without the paths
 * that the handle's geometry rules out (sliver cells, tiles beyond the prefetch registers, one candidate list per level)
 * where it applies; 0 = the general form, which handles every geometry.  Both produce the same bytes
 * (tests/test_gpu_fast_forms.py); the setter serves tests and in-process A/B.  vsg_launch_forms.fast_specialised
 * (include/vsg_orb_debug.h) reports which one a launch took. */
int vsg_orb_set_fast_form(vsg_orb *h, int which);

/* Keypoint capacity a caller must provide per frame for images of this size (>= nfeatures + 3*nlevels,
 * ORBextractor.cc:692,753-754), or a VSG_ERR_* code. */
int vsg_orb_capacity(vsg_orb *h, int rows, int cols);

/* int ORBextractor::operator()(image, mask, keypoints, descriptors, vLappingArea)
 * (ORBextractor.h:59-61, ORBextractor.cc:1083-1169).  gray: CV_8UC1 host image, `stride` bytes per row.
 * lap0/lap1 = vLappingArea.  kps[capacity], desc[capacity*32] are host buffers owned by the caller.
 * Returns monoIndex (>= 0) like the reference, VSG_ERR_EMPTY_IMAGE (-1) for an empty image, or another
 * VSG_ERR_*.  *n = number of keypoints (rows of the descriptor Mat; 0 => the reference release()s it). */
int vsg_orb_extract(vsg_orb *h, const uint8_t *gray, int rows, int cols, int stride, int lap0, int lap1,
                    vsg_keypoint *kps, uint8_t *desc, int capacity, int *n);

/* Batched operator(): nframes (<= max_batch) images of equal size at gray + i*frame_stride.
 * Outputs are [nframes][capacity] records; n[i], mono_index[i] per frame.  Host pointers. */
int vsg_orb_extract_batch(vsg_orb *h, const uint8_t *gray, int nframes, size_t frame_stride, int rows, int cols,
                          int stride, int lap0, int lap1, vsg_keypoint *kps, uint8_t *desc, int capacity, int *n,
                          int *mono_index);

/* Device-resident batched operator() for throughput pipelines and multi-GPU sharding:
 * d_gray, d_kps ([nframes][capacity]), d_desc ([nframes][capacity][32]) and d_counts ([nframes][2] =
 * {n, monoIndex}) are DEVICE pointers on the handle's device.  Work is enqueued asynchronously behind
 * `stream` (a hipStream_t) and completes in stream order.  stream == NULL means the caller's NULL stream: the chain is
 * ordered behind everything the NULL stream holds at entry and the NULL stream waits for it at exit, so
 * producer -> extract -> vsg_hamming_block_best2_device(stream = NULL) sequences are ordered.  Level 0 is read in
 * place: d_gray must stay alive until the work has completed (and for image_pyramid(0) / stereo read-back after it).
 * Descriptors stay resident for the matcher entry points. */
int vsg_orb_extract_batch_device(vsg_orb *h, const uint8_t *d_gray, int nframes, size_t frame_stride, int rows,
                                 int cols, int stride, int lap0, int lap1, vsg_keypoint *d_kps, uint8_t *d_desc,
                                 int *d_counts, int capacity, void *stream);

/* Colour input: Tracking::GrabImage{Monocular,Stereo,RGBD} converts with cv::cvtColor(...,
 * COLOR_{RGB,BGR,RGBA,BGRA}2GRAY) before building the Frame (Tracking.cc:1526-1551, 1595-1608, 1643-1656).  This
 * entry takes the interleaved 8-bit colour frames (channels = 3 or 4; rgb_order != 0 for RGB(A), 0 for BGR(A) =
 * Tracking::mbRGB) on the device and fuses the conversion into the level-0 staging.  Coefficients are data
 * (default = OpenCV 4.2: R2Y 4899, G2Y 9617, B2Y 1868, shift 14); they must sum to 1 << shift, 1 <= shift <= 20.
 * vsg_orb_set_gray_coeffs stores the table in the handle: it applies to every later call of both colour entries on that
 * handle, image-size changes included, until it is set again; a refused table (VSG_ERR_INVALID) leaves the previous one
 * in force.
 * Layout: frame i starts at img + i*frame_stride, a row is `stride` bytes apart from the next and holds cols * channels
 * bytes.  stride < cols * channels is refused with VSG_ERR_INVALID before any copy or launch; apart from that, base,
 * stride and frame_stride need no alignment (pad bytes are never read). */
int vsg_orb_set_gray_coeffs(vsg_orb *h, const int coeffs[3], int shift);
int vsg_orb_extract_batch_device_color(vsg_orb *h, const uint8_t *d_img, int channels, int rgb_order, int nframes,
                                       size_t frame_stride, int rows, int cols, int stride, int lap0, int lap1,
                                       vsg_keypoint *d_kps, uint8_t *d_desc, int *d_counts, int capacity,
                                       void *stream);
/* same with host pointers (colour cv::Mat frames in, keypoints/descriptors out) */
int vsg_orb_extract_batch_color(vsg_orb *h, const uint8_t *img, int channels, int rgb_order, int nframes,
                                size_t frame_stride, int rows, int cols, int stride, int lap0, int lap1,
                                vsg_keypoint *kps, uint8_t *desc, int capacity, int *n, int *mono_index);

/* mvImagePyramid[level] (public member, ORBextractor.h:93; read by Frame::ComputeStereoMatches,
 * Frame.cc:964,1054-1069) of frame `frame` of the last call.  with_border != 0 copies the
 * (w+38)x(h+38) buffer including the 19 px BORDER_REFLECT_101 frame (ORBextractor.cc:1186-1192). */
int vsg_orb_level_size(vsg_orb *h, int level, int *w, int *ht);
int vsg_orb_copy_pyramid_level(vsg_orb *h, int frame, int level, int with_border, uint8_t *dst, int dst_stride);

/* All levels of mvImagePyramid of frame `frame` of the last call in ONE device-to-host copy, each WITH its 19 px
 * border, packed back to back: level l starts at offsets[l] (nlevels entries) with a row stride of width + 38.  With
 * dst == NULL (or dst_bytes too small) nothing is written and the byte count needed is returned; otherwise the bytes
 * written.  This is what the adaptor's DownloadPyramid() uses. */
int vsg_orb_copy_pyramid(vsg_orb *h, int frame, uint8_t *dst, size_t dst_bytes, size_t *offsets);

/* Stage read-back of the last call, for stage-by-stage parity tests: the blurred level
 * (ORBextractor.cc:1129-1130), the FAST candidates (vToDistributeKeys, :868-873; unordered,
 * packed x | y<<12 | response<<24 relative to (16,16)) and the octree selection in list order. */
int vsg_orb_copy_blurred_level(vsg_orb *h, int frame, int level, uint8_t *dst, int dst_stride);
int vsg_orb_copy_candidates(vsg_orb *h, int frame, int level, uint32_t *dst, int cap);
int vsg_orb_copy_selected(vsg_orb *h, int frame, int level, uint32_t *dst, int cap);

/* Average device time per stage of the last N timed calls (HIP events on the handle's streams).
 * names: "pyramid","fast","octree","blur","slots","orient_desc","total".  Returns number of stages.
 * vsg_orb_enable_timing: 0 = off; 1 = events around every stage (the blur then runs as its own launch on its own stream
 * instead of riding in the octree's launch, so the chain is a few % slower than an untimed call); 2 = events around the
 * FAST launch only, everything else exactly as in an untimed call (only "fast" is filled in). */
/* Tracing: VSG_ROCTX=1 in the environment wraps the stage chain and the entry points in roctx ranges for
 * rocprofv3 --marker-trace.  vsg_orb_time_stats is the REGISTER_TIMES analogue (Settings.h:23): mean / std in ms of
 * the host wall time of the blocking operator() calls so far ("ORB Extraction" in Tracking::PrintTimeStats,
 * Tracking.cc:291-330; Frame::mTimeORB_Ext, Frame.cc:126-137).  Returns the number of calls; reset != 0 clears. */
int vsg_orb_time_stats(vsg_orb *h, double *mean_ms, double *std_ms, int reset);
int vsg_orb_enable_timing(vsg_orb *h, int enable);
/* serialize != 0: enqueue every kernel on one stream (no blur overlap), so that stage timings and rocprof kernel
 * durations are free of interference from concurrent kernels.  Results are identical either way. */
int vsg_orb_set_serialize(vsg_orb *h, int serialize);
int vsg_orb_get_timing(vsg_orb *h, float *ms_out, int cap);

/* void Frame::ComputeStereoMatches() (Frame.cc:957-1127) for a rectified pair.  hl/hr = the
 * extractors that just processed the left/right image (their mvImagePyramid is read on the device; one handle
 * with a 2-frame batch works too: frame_l/frame_r index the batch).  kps/desc = the operator() outputs (host).
 * u_right[n_l], depth[n_l] receive mvuRight / mvDepth (-1 where no match); mb, mbf as in Frame.  Returns the
 * number of stereo matches kept. */
int vsg_stereo_matches(vsg_orb *hl, int frame_l, vsg_orb *hr, int frame_r, const vsg_keypoint *kps_l,
                       const uint8_t *desc_l, int n_l, const vsg_keypoint *kps_r, const uint8_t *desc_r, int n_r,
                       float mb, float mbf, float *u_right, float *depth);

/* ---- ORBmatcher (flattened POD views; pointer-graph walking and geometry stay in the C++ adaptor) ---- */

/* static int ORBmatcher::DescriptorDistance(a, b) (ORBmatcher.h:40, ORBmatcher.cc:2047-2063)
 * for npairs row pairs: dist[i] = hamming(a[ia[i]], b[ib[i]]).  Host pointers. */
int vsg_hamming_pairs(int device, const uint8_t *a, int na, const uint8_t *b, int nb, const int32_t *ia,
                      const int32_t *ib, int npairs, int32_t *dist);

/* Brute-force best / second-best of every row of A against all rows of B: the inner loop of
 * SearchByBoW (ORBmatcher.cc:276-299, 810-841) for one vocabulary node without greedy state.
 * Ties resolve to the lowest B index (strict '<' scan).  Host pointers. */
int vsg_hamming_block_best2(int device, const uint8_t *a, int na, const uint8_t *b, int nb, int32_t *best,
                            int32_t *second, int32_t *argbest);
/* Same on device pointers, batched over `nblocks` independent (A_i, B_i) blocks laid out with fixed strides: block i has
 * its rows at d_a + i * block_stride_bytes and d_b + i * block_stride_bytes (0: every block reads the same rows; d_a == d_b
 * and d_b = d_a - block_stride_bytes, "block i against block i - 1", are fine: nothing is written there).  Rows need 4-byte
 * alignment: d_a, d_b and block_stride_bytes are multiples of 4.
 * Counts: na[i] = d_counts_a[i * count_stride], nb[i] = d_counts_b[i * count_stride] (int32 on the device, read when the
 * kernel runs), each clamped to [0, max_rows]: a negative count is an empty side, a count above max_rows is max_rows.  A NULL
 * count pointer means max_rows rows on that side in every block.  Rows at or past the clamped count are never read as
 * data, whatever they hold (stale descriptors of an earlier, larger frame do not take part); each block must still have
 * its row 0 readable on both sides, also where its count is 0.
 * Outputs are [nblocks][max_rows] int32: row q < na[i] of block i goes to index i * max_rows + q; rows at or past the clamped
 * na[i] are NOT written and keep what they held.  Ties go to the lowest B index, `second` counts duplicates (two rows at
 * the best distance: second == best), and a query with no train row (nb[i] == 0, or every row at distance 256) gets
 * best = second = 256, argbest = -1.
 * Refused before anything is enqueued: a NULL d_a, d_b or output, nblocks < 1, max_rows < 1 (VSG_ERR_INVALID);
 * max_rows > 2^20 (the row index has 20 bits of the packed key) or nblocks > 65535 (VSG_ERR_UNSUPPORTED).
 * Asynchronous on `stream` (NULL: the NULL stream): the call returns once the kernel is enqueued; the inputs, the counts
 * and the outputs belong to it until the caller has synchronised with `stream`. */
int vsg_hamming_block_best2_device(int device, const uint8_t *d_a, const uint8_t *d_b, size_t block_stride_bytes,
                                   const int32_t *d_counts_a, const int32_t *d_counts_b, int count_stride,
                                   int nblocks, int max_rows, int32_t *d_best, int32_t *d_second,
                                   int32_t *d_argbest, void *stream);

/* int ORBmatcher::SearchByBoW(KeyFrame *pKF, Frame &F, vpMapPointMatches) (ORBmatcher.h:64,
 * ORBmatcher.cc:226-428), F.Nleft == -1.  FeatureVectors (DBoW2 std::map<NodeId, vector<unsigned>>)
 * are CSR: node ids ascending, offsets[nodes+1], indices.  kf_valid[i] = (pMP && !pMP->isBad()).
 * match_f[i] = KF feature index whose MapPoint F feature i received, or -1.  Returns nmatches.
 * Checked before anything is enqueued, in this and in every other call that takes FeatureVectors as host arrays
 * (vsg_search_by_bow_*, vsg_search_for_triangulation and their vsg_frame_* forms): a NULL output; NULL descriptors, angles
 * or flags of a side with n > 0; and per FeatureVector with nodes > 0 a NULL array, node ids that do not strictly ascend,
 * offsets that do not ascend from 0 or an idx outside [0, n): VSG_ERR_INVALID, and the output is not written.  These checks
 * come before the device is looked at: on a machine without a device a bad argument reports VSG_ERR_INVALID, not
 * VSG_ERR_NO_DEVICE.  A feature listed under two nodes is NOT detected and stays the caller's contract (a DBoW2
 * FeatureVector cannot hold one). */
int vsg_search_by_bow_kf_f(int device, const uint8_t *kf_desc, const float *kf_angle, const uint8_t *kf_valid,
                           int n_kf, const int32_t *kf_node_id, const int32_t *kf_off, const int32_t *kf_idx,
                           int kf_nodes, const uint8_t *f_desc, const float *f_angle, int n_f,
                           const int32_t *f_node_id, const int32_t *f_off, const int32_t *f_idx, int f_nodes,
                           float nnratio, int check_orientation, int32_t *match_f);

/* The same for a fisheye-stereo Frame (F.Nleft != -1, ORBmatcher.cc:277-326, 362-389): features [0, f_nleft) come
 * from the left camera, [f_nleft, n_f) from the right (descriptors vconcat'ed, Frame.cc:296).  Left and right
 * candidates keep separate best / second-best pairs; the right best is accepted at dist <= TH_LOW without a ratio
 * test, but only when the left best also is <= TH_LOW (the reference nests the block).  f_nleft = -1 is the call
 * above.  Checked before anything is enqueued: as above, and f_nleft outside [-1, n_f]: VSG_ERR_INVALID. */
int vsg_search_by_bow_kf_f_stereo(int device, const uint8_t *kf_desc, const float *kf_angle, const uint8_t *kf_valid,
                                  int n_kf, const int32_t *kf_node_id, const int32_t *kf_off, const int32_t *kf_idx,
                                  int kf_nodes, const uint8_t *f_desc, const float *f_angle, int n_f, int f_nleft,
                                  const int32_t *f_node_id, const int32_t *f_off, const int32_t *f_idx, int f_nodes,
                                  float nnratio, int check_orientation, int32_t *match_f);

/* int ORBmatcher::SearchByBoW(KeyFrame *pKF1, KeyFrame *pKF2, vpMatches12) (ORBmatcher.h:65,
 * ORBmatcher.cc:758-900), NLeft == -1.  matches12[idx1] = idx2 or -1.  Checked before anything is enqueued: as for
 * vsg_search_by_bow_kf_f, with the flags of both sides: VSG_ERR_INVALID. */
int vsg_search_by_bow_kf_kf(int device, const uint8_t *desc1, const float *angle1, const uint8_t *valid1, int n1,
                            const int32_t *node_id1, const int32_t *off1, const int32_t *idx1, int nodes1,
                            const uint8_t *desc2, const float *angle2, const uint8_t *valid2, int n2,
                            const int32_t *node_id2, const int32_t *off2, const int32_t *idx2, int nodes2,
                            float nnratio, int check_orientation, int32_t *matches12);

/* int ORBmatcher::SearchForTriangulation(KeyFrame *pKF1, KeyFrame *pKF2, vMatchedPairs, bOnlyStereo, bCoarse)
 * (ORBmatcher.h:72, ORBmatcher.cc:902-1146), NLeft == -1.  eligible1[i] = !pKF1->GetMapPoint(i) && (!bOnlyStereo ||
 * stereo(i)) (:969-979), eligible2 likewise (:998-1005; the reference never sets vbMatched2).  The geometric
 * predicate of :1031-1071 (epipole distance gate, then bCoarse || epipolarConstrain) is a pure function of the pair
 * and stays with the adaptor: for the s-th SHARED vocabulary node (ascending node id = merge-join order), bit
 * pair_off[s] + i1 * n2(s) + i2 of pair_ok says whether (node list position i1 of KF1, i2 of KF2) passes;
 * pair_off has (shared nodes + 1) entries; pair_ok == NULL means every pair passes.  Among the passing candidates
 * with dist <= TH_LOW the smallest distance wins, the LATER one on ties (`dist > bestDist` skips, :1015).
 * matches12[idx1] = idx2 or -1 (vMatchedPairs = the non-negative entries in index order).  Returns nmatches after
 * the rotation-histogram filter.  Checked before anything is enqueued: as for vsg_search_by_bow_kf_kf, and pair_ok without
 * pair_off, pair_off[0] < 0, or a shared node s whose range pair_off[s + 1] - pair_off[s] holds fewer than n1(s) * n2(s)
 * bits (so a node whose bit count does not fit the int32 offsets): VSG_ERR_INVALID.  pair_ok is read up to word
 * (pair_off[shared nodes] + 31) / 32, exclusive. */
int vsg_search_for_triangulation(int device, const uint8_t *desc1, const float *angle1, const uint8_t *eligible1,
                                 int n1, const int32_t *node_id1, const int32_t *off1, const int32_t *idx1, int nodes1,
                                 const uint8_t *desc2, const float *angle2, const uint8_t *eligible2, int n2,
                                 const int32_t *node_id2, const int32_t *off2, const int32_t *idx2, int nodes2,
                                 const uint32_t *pair_ok, const int32_t *pair_off, int check_orientation,
                                 int32_t *matches12);

/* int ORBmatcher::SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, th, bMono)
 * (ORBmatcher.h:50, ORBmatcher.cc:1667-1878), Nleft == -1.  The adaptor projects the map points and
 * runs Frame::GetFeaturesInArea; query q brings its descriptor, keypoint angle and candidate list
 * cand_idx[cand_off[q] .. cand_off[q+1]) in GetFeaturesInArea order.  train_blocked[i] =
 * (CurrentFrame.mvpMapPoints[i] && Observations() > 0) on entry, updated in place; query_blocks[q] =
 * (pMP_q->Observations() > 0).  train_match[i] = q or left untouched (caller initialises to -1).
 * th_high = TH_HIGH (100).  Returns nmatches. */
int vsg_search_by_projection_last(int device, const uint8_t *q_desc, const float *q_angle,
                                  const uint8_t *query_blocks, int n_q, const int32_t *cand_off,
                                  const int32_t *cand_idx, const uint8_t *t_desc, const float *t_angle,
                                  uint8_t *train_blocked, int n_t, int th_high, int check_orientation,
                                  int32_t *train_match);

/* int ORBmatcher::SearchByProjection(Frame &F, const vector<MapPoint*> &, th, ...) (ORBmatcher.h:46,
 * ORBmatcher.cc:42-216), left block, Nleft == -1: best + second best with octave-aware ratio test. */
int vsg_search_by_projection_local(int device, const uint8_t *q_desc, const uint8_t *query_blocks, int n_q,
                                   const int32_t *cand_off, const int32_t *cand_idx, const uint8_t *t_desc,
                                   const int32_t *t_octave, uint8_t *train_blocked, int n_t, float nnratio,
                                   int32_t *train_match);

/* Common core of the searches that keep only the best candidate per projected MapPoint:
 *   SearchByProjection(KeyFrame*, Sim3, vpPoints, vpMatched, th, ratioHamming)   (ORBmatcher.h:58, .cc:430-528)
 *   SearchByProjection(KeyFrame*, Sim3, vpPoints, vpPointsKFs, ...)             (ORBmatcher.h:62, .cc:530-641)
 *   SearchByProjection(Frame&, KeyFrame*, sAlreadyFound, th, ORBdist)           (ORBmatcher.h:54, .cc:1880-2000; the
 *                                                  rotation check is vsg_search_by_projection_last's check_orientation)
 *   SearchBySim3's two directional passes (.cc:1500-1640) and Fuse's candidate loops (.cc:1148-1446), whose
 *   geometric predicates (level window, chi2 of the reprojection) filter the candidate lists in the adaptor.
 * For each query in order: best (strict '<', earliest wins) over the non-blocked candidates; q_best_idx/q_best_dist per
 * query (-1 / 256 if none); if dist <= th_high the match is accepted: train_match[best] = q, train_blocked[best] =
 * query_blocks[q] (NULL: never blocks).  train_blocked / train_match may be NULL.  Returns the number accepted. */
int vsg_search_window(int device, const uint8_t *q_desc, const uint8_t *query_blocks, int n_q,
                      const int32_t *cand_off, const int32_t *cand_idx, const uint8_t *t_desc, uint8_t *train_blocked,
                      int n_t, int th_high, int32_t *q_best_idx, int32_t *q_best_dist, int32_t *train_match);

/* void MapPoint::ComputeDistinctiveDescriptors() (MapPoint.cc:340-415) for ngroups map points at once:
 * group g = descriptor rows off[g] .. off[g+1]-1 (the observations' descriptors in the order the reference pushes
 * them); best[g] = index inside the group of the descriptor with the least median distance to the rest (first one
 * on ties), -1 for an empty group.  Groups of more than 128 descriptors return VSG_ERR_UNSUPPORTED. */
int vsg_distinctive_descriptors(int device, const uint8_t *desc, const int32_t *off, int ngroups, int32_t *best);

/* ---- Frame grid: Frame::AssignFeaturesToGrid / PosInGrid (Frame.cc:521-553, 870-880) and
 * Frame::GetFeaturesInArea / KeyFrame::GetFeaturesInArea (Frame.cc:802-868, KeyFrame.cc:834-874) on the device.
 * 64 x 48 cells (Frame.h:49-50).  kps = the (undistorted) keypoints the reference indexes (host pointer).
 * A vsg_grid is the left grid of a resident frame (vsg_frame, below) without descriptors, mvuRight or FeatureVector:
 * the same upload builds it and the same kernel answers vsg_grid_query and vsg_frame_features_in_area.  n <= 32767
 * (VSG_ERR_INVALID above); n == 0 builds a grid whose every query is empty.  Octaves are compared whole and may be
 * anything an int16 holds (a resident frame's: 0..15); outside of that: VSG_ERR_UNSUPPORTED.  Device memory per grid:
 * one allocation of 12 bytes per keypoint (the grid entry: x, y, index | octave -- the keypoint records themselves stay
 * on the host) + two cell tables of 12 KB (the right-camera one is empty). */
typedef struct vsg_grid vsg_grid;
int vsg_grid_build(int device, const vsg_keypoint *kps, int n, float min_x, float min_y, float max_x, float max_y,
                   vsg_grid **out);
void vsg_grid_destroy(vsg_grid *g);
/* nq queries (x, y, r, minLevel, maxLevel) -> CSR candidate lists in the reference's order (cells ix outer, iy
 * inner, insertion order inside a cell): cand_off[nq+1], cand_idx[cap].  min_level/max_level may be NULL (= -1,
 * KeyFrame::GetFeaturesInArea has no level filter).  Returns the total number of candidates (which may exceed
 * cap: nothing beyond cap is written) or a VSG_ERR_* code. */
int vsg_grid_query(vsg_grid *g, const float *x, const float *y, const float *r, const int32_t *min_level,
                   const int32_t *max_level, int nq, int32_t *cand_off, int32_t *cand_idx, int cap);

/* ---- DBoW2 vocabulary: ORBVocabulary::loadFromBinFile (TemplatedVocabulary.h:1478-1552, called at
 * System.cc:105-112) from an in-memory image of the .bin file, and transform(features, BowVector, FeatureVector,
 * levelsup) (TemplatedVocabulary.h:1139-1212) as called by Frame::ComputeBoW / KeyFrame::ComputeBoW with
 * levelsup = 4 (Frame.cc:882-889).  BowVector: ascending (word id, value) pairs; FeatureVector: CSR with ascending
 * node ids (the form vsg_search_by_bow_* takes); fv_idx must hold n entries, fv_off fv_cap+1.  word_of / node_of /
 * weight_of (optional) are the per-feature leaf word, node at level L - levelsup and word weight. */
typedef struct vsg_vocab vsg_vocab;
int vsg_vocab_load(int device, const uint8_t *blob, size_t size, vsg_vocab **out);
void vsg_vocab_destroy(vsg_vocab *v);
int vsg_vocab_info(const vsg_vocab *v, int *k, int *L, int *scoring, int *weighting, int *nnodes, int *nwords);
int vsg_bow_transform(vsg_vocab *voc, const uint8_t *desc, int n, int levelsup, int32_t *bow_ids, double *bow_vals,
                      int bow_cap, int *n_bow, int32_t *fv_node, int32_t *fv_off, int32_t *fv_idx, int fv_cap,
                      int *n_fv, int32_t *word_of, int32_t *node_of, double *weight_of);

/* ---- TemplatedVocabulary::score (TemplatedVocabulary.h:1214-1219, ScoringObject.cpp:21-314) with the vocabulary's
 * scoring type: one query BowVector (ids, vals, n) against m BowVectors in CSR form (vector c = m_ids / m_vals
 * [off[c], off[c+1])); out[c] = score(query, vector c), bit-identical doubles.  Every BowVector has strictly ascending
 * word ids < the vocabulary's word count.  Each pair is summed as ONE chain in ascending shared word id, as the merge
 * loop does; L2 keeps its score >= 1 clamp.  KL scoring (log) returns VSG_ERR_UNSUPPORTED: the device cannot reproduce
 * the host's log bit for bit.  Query BowVectors of more than 12288 words: VSG_ERR_UNSUPPORTED. */
int vsg_vocab_score(vsg_vocab *voc, const int32_t *ids, const double *vals, int n, const int32_t *off,
                    const int32_t *m_ids, const double *m_vals, int m, double *out);

/* ---- KeyFrameDatabase (KeyFrameDatabase.h, KeyFrameDatabase.cc:31-96, 592-830) resident on the device.  Keyframes are
 * the caller's uint64 ids (KeyFrame::mnId), maps int32 ids (KeyFrame::GetMap(); a keyframe no call has given a map has
 * map -1).  Every keyframe's BowVector and the inverted file stay on the device; posting lists keep the reference's
 * order: add appends to each word's list, erase removes the keyframe's FIRST entry in each list of its BowVector (the
 * BowVector of its last add), clear / clear_map drop entries.  Adding an id twice without an erase gives two entries.
 * The database keeps, per keyframe id, the KeyFrame members the queries use (mnRelocQuery, mnRelocWords, mRelocScore,
 * mnPlaceRecognitionQuery, mnPlaceRecognitionWords, mPlaceRecognitionScore), across queries, erase, re-add and clear;
 * all start at 0 (mRelocScore, uninitialised in the reference, is defined as 0).  There is no bad flag: callers erase a
 * keyframe when it turns bad, as KeyFrame::SetBadFlag does (KeyFrame.cc:809).  Thread-safe: every call takes the
 * database's lock (mMutex); a query runs on the calling thread's stream, one enqueue and one wait.  KL scoring: the
 * queries return VSG_ERR_UNSUPPORTED; so do query BowVectors of more than 12288 words. */
typedef struct vsg_kfdb vsg_kfdb;
/* KeyFrameDatabase(const ORBVocabulary &voc) (:31-34) */
int vsg_kfdb_create(vsg_vocab *voc, vsg_kfdb **out);
void vsg_kfdb_destroy(vsg_kfdb *db);
/* add(pKF) (:36-42): pKF->mBowVec as ascending (bow_ids, bow_vals); map_id = pKF->GetMap() */
int vsg_kfdb_add(vsg_kfdb *db, uint64_t kf_id, int32_t map_id, const int32_t *bow_ids, const double *bow_vals, int n);
/* erase(pKF) (:44-62), clear() (:64-68), clearMap(pMap) (:70-96) */
int vsg_kfdb_erase(vsg_kfdb *db, uint64_t kf_id);
int vsg_kfdb_clear(vsg_kfdb *db);
int vsg_kfdb_clear_map(vsg_kfdb *db, int32_t map_id);
/* KeyFrame::GetMap() changes when maps merge (KeyFrame::UpdateMap): the new map of each keyframe id */
int vsg_kfdb_set_map(vsg_kfdb *db, const uint64_t *kf_ids, const int32_t *map_ids, int n);
/* GetBestCovisibilityKeyFrames(10) of n keyframes: neighbours of kf_ids[j] are neigh_ids[offsets[j] .. offsets[j+1]) in
 * the reference's order (only the first 10 are kept); a neighbour need not be in the database */
int vsg_kfdb_set_covisibility(vsg_kfdb *db, const uint64_t *kf_ids, const int32_t *offsets, const uint64_t *neigh_ids,
                              int n);
/* DetectRelocalizationCandidates(F, pMap) (:719-830): query_id = F->mnId, (bow_ids, bow_vals, n) = F->mBowVec.  The
 * candidates in the reference's order; more than cap: VSG_ERR_CAPACITY with *n_out = the number needed. */
int vsg_kfdb_detect_relocalization_candidates(vsg_kfdb *db, uint64_t query_id, const int32_t *bow_ids,
                                              const double *bow_vals, int n, int32_t map_id, uint64_t *out_ids, int cap,
                                              int *n_out);
/* DetectNBestCandidates(pKF, vpLoopCand, vpMergeCand, nNumCandidates) (:592-717): query_kf_id = pKF->mnId, the BowVector
 * pKF->mBowVec, connected_ids = pKF->GetConnectedKeyFrames(), map_id = pKF->GetMap(), bad_map_ids = the maps whose
 * IsBad() is true.  loop_out / merge_out hold nNumCandidates ids each. */
int vsg_kfdb_detect_n_best_candidates(vsg_kfdb *db, uint64_t query_kf_id, const int32_t *bow_ids,
                                      const double *bow_vals, int n, const uint64_t *connected_ids, int n_conn,
                                      int32_t map_id, const int32_t *bad_map_ids, int n_bad, int nNumCandidates,
                                      uint64_t *loop_out, int *n_loop, uint64_t *merge_out, int *n_merge);

/* int ORBmatcher::SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize)
 * (ORBmatcher.h:68, ORBmatcher.cc:643-756); candidate lists from F2.GetFeaturesInArea per F1 keypoint. */
int vsg_search_for_initialization(int device, const uint8_t *desc1, const float *angle1, const int32_t *octave1,
                                  int n1, const int32_t *cand_off, const int32_t *cand_idx, const uint8_t *desc2,
                                  const float *angle2, int n2, float nnratio, int check_orientation,
                                  int32_t *matches12);


/* ---- Threads, streams, staging ("re-entrant, thread-safe, stream per calling thread") ----------------
 * Every matcher / grid / BoW / stereo / frame entry point runs on the CALLING THREAD's own non-blocking HIP stream and
 * stages through that thread's pinned + device arenas, which only grow: no hipMalloc / hipFree / NULL-stream launch
 * in steady state (a hipFree in LoopClosing's thread would otherwise stall Tracking's extractor streams).
 * vsg_thread_release() frees the calling thread's streams and arenas (optional; call before the thread exits).
 * vsg_thread_arena_growths(device) = number of arena (re)allocations so far on this thread (constant in steady state). */
int vsg_thread_release(void);
int vsg_thread_arena_growths(int device);
/* hipMemcpyAsync(dst, src, bytes, DeviceToDevice, stream) on `device`, for hosts that hold raw device pointers (the
 * records of vsg_shard_record) and should not bind a second copy of the HIP runtime for one copy. */
int vsg_copy_d2d_async(int device, void *dst, const void *src, size_t bytes, void *stream);

/* ---- Pinned caller memory (the buffers behind cv::Mat::data of a reused frame, Frame::mvKeys / mDescriptors rings;
 * the reference hands operator() plain heap memory: ORBextractor.h:59-61, Frame.cc:555-563) ---------------------------
 * vsg_host_alloc / vsg_host_free: pinned host memory from the runtime's own allocator (hipHostMalloc), what the handle's
 * staging slots use themselves.  Memory from vsg_host_alloc is the memory the device reads and writes IN PLACE
 * (vsg_orb_submit_batch / vsg_orb_wait, the blocking entry points): no staging copy on either side.  So is hipHostMalloc
 * memory the caller obtained elsewhere.  vsg_host_free releases ONLY pointers vsg_host_alloc returned (VSG_ERR_INVALID for
 * anything else, also for hipHostMalloc memory of another owner: since round 5 the library keeps a registry of its own blocks and
 * does not forward foreign pointers to hipHostFree).
 * vsg_host_register / vsg_host_unregister: pin ordinary heap memory after the fact (hipHostRegister).  Such memory is a
 * user-pointer mapping of heap pages; on the round-4 test pool a page of a live, registered, in-use range lost its
 * device mapping under heap churn (a fatal `Memory access fault by GPU`; profiles/r04_q_open_issue_gpu_fault.txt,
 * tools/repro_hostregister.cpp).  By DEFAULT the library therefore treats registered memory like pageable memory: it is
 * staged through the slot's own pinned buffers by the calling thread and the device never touches it.
 * vsg_orb_set_direct_registered(h, 1) opts a handle in to in-place access of registered memory as well (hosts that
 * register page-aligned, long-lived, mlock-ed arenas and have qualified their kernel / driver).
 * vsg_host_kind(ptr, bytes): how the library classifies the WHOLE range [ptr, ptr + bytes) -- both ends must be pinned
 * the same way under one contiguous device alias, otherwise the range counts as pageable. */
#define VSG_HOST_PAGEABLE 0      /* staged through the slot's pinned buffers */
#define VSG_HOST_LIB_ALLOC 1     /* inside one vsg_host_alloc range: in place */
#define VSG_HOST_HIPHOSTMALLOC 2 /* somebody else's hipHostMalloc memory: in place */
#define VSG_HOST_REGISTERED 3    /* hipHostRegister-ed heap memory: staged unless vsg_orb_set_direct_registered(h, 1) */
int vsg_host_register(void *ptr, size_t bytes);
int vsg_host_unregister(void *ptr);
int vsg_host_alloc(size_t bytes, void **out);
int vsg_host_free(void *ptr);
int vsg_host_kind(const void *ptr, size_t bytes);
int vsg_orb_set_direct_registered(vsg_orb *h, int enable);

/* ---- Asynchronous operator() batches (caller: Frame::ExtractORB, Frame.cc:555-563, in a throughput pipeline) -----
 * vsg_orb_submit_batch enqueues H2D + the stage chain + the output export of one batch into one of the handle's
 * vsg_orb_slots() (= 3) pipeline slots and returns at once with a ticket (>= 0); VSG_ERR_BUSY when every slot
 * holds a batch that has not been waited for, and when the image size differs from the handle's current one while any
 * ticket is still un-waited (a new size rebuilds the slots those tickets live in).  H2D of batch k+1 runs beside the kernels of batch k and the export of
 * batch k-1 (three streams).  kps / desc ([nframes][capacity] records, host memory) must stay valid until the wait
 * returns; if they are memory the device may touch in place (vsg_host_alloc / hipHostMalloc memory, see "Pinned caller
 * memory" above) the device writes the n[i] records of every frame straight into them, otherwise they are filled from
 * the slot's pinned staging inside vsg_orb_wait -- either way only n[i] records per frame cross PCIe, not `capacity`.
 * `gray` must stay valid until the wait returns if it is such memory; any other
 * input is copied before submit returns (batches of 16 frames and more: by the calling thread and three helper
 * threads the handle keeps asleep between batches).  vsg_orb_wait(ticket) blocks until that batch is complete and delivers n[]
 * and mono_index[] (nframes entries each).  Tickets are waited for in submission order. */
int vsg_orb_slots(const vsg_orb *h);
/* Latency path of the BLOCKING entry points (vsg_orb_extract, vsg_orb_extract_batch with <= 8 frames; the reference
 * calls operator() once per frame: System::TrackRGBD -> Frame::ExtractORB, System.cc:359, Frame.cc:555-563): the pinned
 * image is read by a kernel instead of a copy-engine transfer and k_orient_desc writes the records into the pinned
 * destination itself (no export launch, no DMA).  Results are identical on either path. */
int vsg_orb_submit_batch(vsg_orb *h, const uint8_t *gray, int nframes, size_t frame_stride, int rows, int cols,
                         int stride, int lap0, int lap1, vsg_keypoint *kps, uint8_t *desc, int capacity);
int vsg_orb_wait(vsg_orb *h, int ticket, int *n, int *mono_index);

/* ---- Device-resident Frame / KeyFrame features (SURVEY 8b last row; Frame.h:280,290) ---------------------------
 * A vsg_frame keeps what the searches read of one Frame or KeyFrame on the device between calls: the keypoints the
 * grid indexes (mvKeysUn; mvKeys || mvKeysRight when Nleft != -1), mDescriptors, mvuRight and the 64 x 48 mGrid (+
 * mGridRight) as CSR -- so that a search uploads only the projected positions and the map points' descriptors.
 * A small host mirror of the keypoints serves the ordered host-side passes (rotation histogram, level ratio test).
 * Frames are immutable after upload and may be searched concurrently from several threads.  The one thing that may be
 * added to an uploaded frame is the per-keyframe stereo attachment of vsg_frame_set_stereo_points (below, at
 * vsg_frame_triangulate_matches): it is set once per keyframe, before the first call that reads it and not while another
 * thread's call does, and the next vsg_frame_upload / vsg_frame_from_extractor* / vsg_orb_extract_to_frame* into the
 * frame drops it. */
typedef struct vsg_frame vsg_frame;
/* Limits (the packed candidate entries are index : 15 | distance : 9 | octave : 4 bits): capacity <= 32767 features per
 * frame (vsg_frame_create returns VSG_ERR_INVALID beyond, the host-candidate forms vsg_search_* return
 * VSG_ERR_UNSUPPORTED for n_t > 32767) and keypoint octaves 0..15 (vsg_frame_upload: VSG_ERR_UNSUPPORTED; the
 * extractor itself is limited to 16 levels).  The reference's settings use 1000-2000 features and 8 levels.  A frame
 * that was created but never uploaded is empty: every search on it finds nothing. */
int vsg_frame_create(int device, int capacity, vsg_frame **out);
void vsg_frame_destroy(vsg_frame *f);
/* Frame::Frame(...) after ExtractORB + UndistortKeyPoints: keys = mvKeysUn (Nleft == -1) or mvKeys followed by
 * mvKeysRight (nleft = Nleft, Frame.cc:296); u_right = mvuRight (NULL: all -1); grid bounds mnMinX.. (Frame.cc:378).
 * Builds mGrid / mGridRight exactly like AssignFeaturesToGrid (Frame.cc:521-553). */
int vsg_frame_upload(vsg_frame *f, const vsg_keypoint *keys, const uint8_t *desc, const float *u_right, int n,
                     int nleft, float min_x, float min_y, float max_x, float max_y);
/* The same straight out of the extractor, device to device, for frame `index` of the handle's last
 * vsg_orb_extract / _batch / _submit_batch call (no distortion: mvKeysUn = mvKeys, Frame.cc UndistortKeyPoints with
 * mDistCoef == 0); the grid is built by a kernel.  The host mirror is filled from kps_host (the records the extract
 * call delivered) -- nothing is downloaded. */
int vsg_frame_from_extractor(vsg_frame *f, vsg_orb *h, int index, const vsg_keypoint *kps_host, int n, float min_x,
                             float min_y, float max_x, float max_y);
/* Frame::ComputeImageBounds (Frame.cc:924-955) for a pinhole camera: K4 = {fx, fy, cx, cy} (the floats of mK), dist = the
 * 4 or 5 floats of mDistCoef (k1, k2, p1, p2[, k3]; Tracking.cc:742-787); out = {mnMinX, mnMinY, mnMaxX, mnMaxY} -- the
 * image rectangle when mDistCoef(0) == 0, otherwise the four corners through cv::undistortPoints(.., K, D, Mat(), K)
 * ([OCV 4.2]: five fixed iterations in double).  Four points, once per camera (mbInitialComputations, Frame.cc:373-392):
 * host arithmetic, no device needed. */
int vsg_camera_image_bounds(int cols, int rows, const float K4[4], const float *dist, int ndist, float out[4]);
/* vsg_frame_from_extractor for a DISTORTED camera (mDistCoef(0) != 0: config/RGB-D/TUM1.yaml, config/RGB-D-Inertial/
 * RealSense_D435i.yaml -- BASELINE configs C1 and C5): Frame::UndistortKeyPoints (Frame.cc:891-921) runs on the device,
 * in double, inside the launch that builds the grid -- the frame's keypoints are mvKeysUn, the grid indexes them with
 * the bounds of vsg_camera_image_bounds, and keys_un_out (n records, may be NULL) receives mvKeysUn for the host's own
 * use (Tracking, the optimizer).  The frame stays resident: no D2H -> cv::undistortPoints -> H2D hop.  With
 * mDistCoef(0) == 0 this is vsg_frame_from_extractor (keys_un_out = kps_host). */
int vsg_frame_from_extractor_undistort(vsg_frame *f, vsg_orb *h, int index, const vsg_keypoint *kps_host, int n,
                                       const float K4[4], const float *dist, int ndist, float min_x, float min_y,
                                       float max_x, float max_y, vsg_keypoint *keys_un_out);
/* The Frame constructor's front end in ONE call and ONE wait (Frame.cc:344-358: ExtractORB -> UndistortKeyPoints ->
 * AssignFeaturesToGrid): vsg_orb_extract + vsg_frame_from_extractor_undistort, with the grid launch enqueued on the
 * extractor's stream right behind its stage chain (it reads the keypoint count on the device), so the blocking call's
 * single wait covers both.  Arguments as the two calls'; K4 == NULL: no distortion.  Returns monoIndex like
 * vsg_orb_extract, *n = the keypoint count; VSG_ERR_CAPACITY when the frame's capacity is below *n. */
int vsg_orb_extract_to_frame(vsg_orb *h, const uint8_t *gray, int rows, int cols, int stride, int lap0, int lap1,
                             vsg_keypoint *kps, uint8_t *desc, int capacity, int *n, vsg_frame *f, const float K4[4],
                             const float *dist, int ndist, float min_x, float min_y, float max_x, float max_y,
                             vsg_keypoint *keys_un_out);
/* RGB-D Frame (Frame.cc:344-358 with the step between UndistortKeyPoints and AssignFeaturesToGrid):
 * vsg_orb_extract_to_frame + Tracking::GrabImageRGBD's depth conversion (Tracking.cc:1610-1611) +
 * Frame::ComputeStereoFromRGBD (Frame.cc:1129-1150), in ONE enqueue and ONE wait.  depth: the depth plane (rows x cols of
 * the gray image, `depth_stride` bytes per row) as VSG_DEPTH_U16 (TUM PNG, RealSense) or VSG_DEPTH_F32; depth_scale =
 * Tracking::mDepthMapFactor (vsg_depth_map_scale), converted as convertTo(CV_32F, depth_scale) unless the plane is F32
 * and |depth_scale - 1| <= 1e-5; mbf = Frame::mbf.  d = depth at ((int)mvKeys[i].y, (int)mvKeys[i].x); d > 0:
 * mvDepth[i] = d, mvuRight[i] = mvKeysUn[i].x - mbf / d, otherwise both -1 (so are keypoints whose truncated pixel lies
 * outside the plane, or NaN coordinates: undefined behaviour in the reference).  The resident frame has mvuRight
 * (the stereo gates of SearchByProjection / Fuse apply); u_right / depth_out (capacity entries each, may be NULL)
 * receive mvuRight / mvDepth.  Pinned depth (vsg_host_alloc, hipHostMalloc) is read in place, any other memory is
 * staged behind the extractor's enqueue.  Sizes other than rows x cols: VSG_ERR_INVALID; other types:
 * VSG_ERR_UNSUPPORTED.  Returns as vsg_orb_extract_to_frame; on failure the frame is empty. */
#define VSG_DEPTH_U16 0
#define VSG_DEPTH_F32 1
int vsg_orb_extract_to_frame_rgbd(vsg_orb *h, const uint8_t *gray, int rows, int cols, int stride, int lap0, int lap1,
                                  vsg_keypoint *kps, uint8_t *desc, int capacity, int *n, vsg_frame *f,
                                  const float K4[4], const float *dist, int ndist, float min_x, float min_y, float max_x,
                                  float max_y, vsg_keypoint *keys_un_out, const void *depth, int depth_type,
                                  size_t depth_stride, int depth_rows, int depth_cols, float depth_scale, float mbf,
                                  float *u_right, float *depth_out);
/* Tracking's mDepthMapFactor from the settings' RGBD.DepthMapFactor (Tracking.cc:638-642): 1 when |yaml| < 1e-5,
 * otherwise 1.0f / yaml.  Host arithmetic. */
float vsg_depth_map_scale(float yaml_value);
/* Throughput form of the depth step for the outputs of vsg_orb_extract_batch_device(_color): d_kps [nframes][capacity]
 * (mvKeys), d_counts [nframes][2] and nframes depth planes at d_depth + f * frame_stride (rows x cols, depth_stride
 * bytes per row) on `device`.  Each record is undistorted as vsg_frame_from_extractor_undistort does (K4 / dist / ndist;
 * ndist = 0 or dist[0] == 0: none) and sampled as vsg_orb_extract_to_frame_rgbd; d_u_right / d_depth_out
 * [nframes][capacity] receive mvuRight / mvDepth, -1 past each frame's count.  One launch, asynchronous on `stream`
 * (NULL = the caller's NULL stream). */
int vsg_rgbd_depth_batch_device(int device, const void *d_depth, int depth_type, int nframes, size_t frame_stride,
                                size_t depth_stride, int rows, int cols, float depth_scale, float mbf, const float K4[4],
                                const float *dist, int ndist, const vsg_keypoint *d_kps, const int *d_counts,
                                int capacity, float *d_u_right, float *d_depth_out, void *stream);
int vsg_frame_size(const vsg_frame *f);
/* test / debug read-back of the device copy: grid CSR (cell_start[64*48+1], entries[n]) of the left (0) or right (1) grid */
int vsg_frame_copy_grid(vsg_frame *f, int right, int32_t *cell_start, int32_t *entries);

/* Frame::GetFeaturesInArea(x, y, r, minLevel, maxLevel, bRight) (Frame.cc:802-868) / KeyFrame::GetFeaturesInArea
 * (KeyFrame.cc:834-874; pass min_level = max_level = NULL) for nq windows on the resident grid; CSR out, return value
 * and cap as vsg_grid_query, which is this call on a grid's frame with right = 0.  Indices are grid-local (right grid:
 * i - Nleft), exactly what the reference's vectors hold. */
int vsg_frame_features_in_area(vsg_frame *f, const float *x, const float *y, const float *r, const int32_t *min_level,
                               const int32_t *max_level, int right, int nq, int32_t *cand_off, int32_t *cand_idx,
                               int cap);

/* int ORBmatcher::SearchByProjection(Frame &F, const vector<MapPoint*> &vpMapPoints, th, bFarPoints, thFarPoints)
 * (ORBmatcher.h:46, ORBmatcher.cc:42-216), BOTH blocks (left :59-143, right camera :146-214 when F.Nleft != -1).
 * One entry per map point that survives the caller-side tests (:50-57: in view, far points, isBad):
 *   in_view / proj_x / proj_y / proj_xr / scale_level / view_cos   = mbTrackInView, mTrackProjX/Y, mTrackProjXR,
 *   mnTrackScaleLevel, mTrackViewCos;  the *_r arrays (NULL when Nleft == -1) = the ...R members of the right camera;
 *   mp_desc = pMP->GetDescriptor(); mp_observed = pMP->Observations() > 0.
 * scale_factors = F.mvScaleFactors.  left_to_right / right_to_left = F.mvLeftToRightMatch / mvRightToLeftMatch
 * (Nleft != -1).  train_blocked[i] = (F.mvpMapPoints[i] && Observations() > 0) on entry, updated in place;
 * train_match[i] = index of the map point assigned to feature i (caller initialises to -1).  Returns nmatches. */
int vsg_frame_search_by_projection(vsg_frame *F, int n_mp, const uint8_t *mp_desc, const uint8_t *mp_observed,
                                   const uint8_t *in_view, const float *proj_x, const float *proj_y,
                                   const float *proj_xr, const int32_t *scale_level, const float *view_cos,
                                   const uint8_t *in_view_r, const float *proj_x_r, const float *proj_y_r,
                                   const int32_t *scale_level_r, const float *view_cos_r, float th, float nnratio,
                                   const float *scale_factors, int nlevels, const int32_t *left_to_right,
                                   const int32_t *right_to_left, uint8_t *train_blocked, int32_t *train_match);

/* ---- The local map's MapPoints, resident on the device: what Frame::isInFrustum (Frame.cc:656-719) and
 * SearchByProjection(F, vpMapPoints) (ORBmatcher.cc:42-216) read of a MapPoint.  Slots 0 .. capacity-1 are the caller's
 * own index of a MapPoint*.  Per slot: world_pos[3] = GetWorldPos(), normal[3] = GetNormal(), min_dist / max_dist = the
 * MEMBERS mfMinDistance / mfMaxDistance (MapPoint.h; set at MapPoint.cc:106-107, 509-510), not the scaled values of
 * GetMinDistanceInvariance() / GetMaxDistanceInvariance(): isInFrustum compares with 0.8f * mfMinDistance and
 * 1.2f * mfMaxDistance (the library applies the getters' factors, MapPoint.cc:521-531) but PredictScale divides the
 * unscaled mfMaxDistance (MapPoint.cc:555), and 1.2f * x cannot be undone exactly.  desc[32] = GetDescriptor(),
 * observed = Observations() > 0.  A new store is
 * all zeros.  update and read run on the calling thread's stream and return when the device copy is written / read, so
 * a search that another thread starts afterwards sees the update; an update must not run WHILE another thread's call
 * reads the same store (the reference holds mMutexPos / mMutexFeatures for that). */
typedef struct vsg_mappoints vsg_mappoints;
int vsg_mappoints_create(int device, int capacity, vsg_mappoints **out);
void vsg_mappoints_destroy(vsg_mappoints *mp);
int vsg_mappoints_capacity(const vsg_mappoints *mp);
/* SetWorldPos / AddObservation / ComputeDistinctiveDescriptors / UpdateNormalAndDepth of n slots (MapPoint.cc:116,
 * 141, 340, 440): entry i of every non-NULL field array goes to slot slots[i]; a NULL field keeps what the slots
 * hold.  A slot listed more than once takes its LAST entry.  A slot outside [0, capacity): VSG_ERR_INVALID and nothing
 * is written.  One scatter kernel, no copy per field.  desc, normal, min_dist and max_dist are DERIVED from a point's
 * observations in keyframes: the caller either computes them and sends them here, or sends the observation lists to
 * vsg_mappoints_refresh_from_observations below, which computes and writes them on the device. */
int vsg_mappoints_update(vsg_mappoints *mp, int n, const int32_t *slots, const float *world_pos, const float *normal,
                         const float *min_dist, const float *max_dist, const uint8_t *desc, const uint8_t *observed);
/* test / debug read-back of n slots (any out pointer may be NULL) */
int vsg_mappoints_read(vsg_mappoints *mp, int n, const int32_t *slots, float *world_pos, float *normal, float *min_dist,
                       float *max_dist, uint8_t *desc, uint8_t *observed);

/* void MapPoint::ComputeDistinctiveDescriptors() (MapPoint.cc:340-417) and void MapPoint::UpdateNormalAndDepth()
 * (MapPoint.cc:440-513) of n map points from their observations in resident keyframes, written into the slots on the
 * device: the caller sends a few integers per observation instead of gathering descriptors, computing and uploading.
 * Point i = slot slots[i]; its observations (mObservations in the std::map's order, one per keyframe: its leftIndex)
 * are entries [obs_off[i], obs_off[i + 1]) of obs_kf (index into kfs), obs_idx (leftIndex in that keyframe) and obs_bad
 * (pKF->isBad(); NULL: none); ref_pos[i] = the position of mpRefKF's observation inside that list.  kfs[k] holds
 * keyframe k's mDescriptors and mvKeysUn, kf_Ow[3 k] = its GetCameraCenter().  scale_factors = mvScaleFactors,
 * nlevels = mnScaleLevels, in [1, 16].  what = the fields to refresh; fields it does not name stay byte-identical.
 *   - A bad keyframe's observation is left out of the descriptor candidates (:363); it is still summed into the normal
 *     (:461-482 has no such test) and may be the reference observation (:484-492).
 *   - A point with an empty list keeps all four fields (:354, :455); its best is -1, its outs are what the slot holds.
 *   - A point whose candidates are all bad keeps its descriptor (:379), best -1; its normal and depth are updated.
 *   - best[i] = the position inside point i's list of the chosen observation: the first row with the least median
 *     wins (strict '<', :406); the caller copies that row of its own mDescriptors into mDescriptor (:415).  -1 when
 *     what does not name VSG_REFRESH_DESC.
 *   - normal / min_dist / max_dist (outs) = mNormalVector, mfMinDistance, mfMaxDistance as the slot holds them after
 *     the call (:509-511).  Float arithmetic in a fixed order, one rounding per operation, the sum serial in list order
 *     (csrc/vsg_observations.h).  Pos == a camera centre gives NaN, as in the reference.
 *   - world_pos is read from the store: the caller has sent SetWorldPos before (vsg_mappoints_update).
 * Any out may be NULL.  Checked before anything is enqueued (an error leaves no kernel behind and writes nothing):
 * offsets that do not ascend from 0, an observation outside [0, n_kf) x [0, N of that keyframe), a slot outside
 * [0, capacity) or listed twice, a ref_pos outside a non-empty list, a reference keypoint whose octave is >= nlevels,
 * nlevels outside [1, 16], what outside 1 .. 3, a keyframe on another device than the store: VSG_ERR_INVALID; a keyframe
 * with Nleft != -1 (:475-481, :494-501), or a point with more than 128 observations that are not bad (the cap of
 * vsg_distinctive_descriptors): VSG_ERR_UNSUPPORTED.  n == 0: VSG_OK, nothing is touched.  One enqueue on the calling
 * thread's stream and one wait: the call returns when the store is written, as vsg_mappoints_update. */
#define VSG_REFRESH_DESC 1   /* ComputeDistinctiveDescriptors -> desc */
#define VSG_REFRESH_NORMAL 2 /* UpdateNormalAndDepth -> normal, min_dist, max_dist */
int vsg_mappoints_refresh_from_observations(vsg_mappoints *mp, int n, const int32_t *slots, const int32_t *obs_off,
                                            const int32_t *obs_kf, const int32_t *obs_idx, const uint8_t *obs_bad,
                                            const int32_t *ref_pos, int n_kf, vsg_frame *const *kfs, const float *kf_Ow,
                                            const float *scale_factors, int nlevels, int what, int32_t *best,
                                            float *normal, float *min_dist, float *max_dist);

/* The camera of one Frame as isInFrustum uses it (Frame.h:203-204, 316-318; set by Frame::UpdatePoseMatrices,
 * Frame.cc:612-619): Rcw = mRcw row-major, tcw = mtcw, Ow = mOw (passed, not derived: the reference stores it),
 * fx, fy, cx, cy = Pinhole::mvParameters, mbf, log_scale_factor = mfLogScaleFactor, n_levels = mnScaleLevels.  The image
 * bounds mnMinX .. mnMaxY are the vsg_frame's own. */
typedef struct vsg_frame_pose {
  float Rcw[9], tcw[3], Ow[3];
  float fx, fy, cx, cy, mbf, log_scale_factor;
  int32_t n_levels;
} vsg_frame_pose;

/* bool Frame::isInFrustum(MapPoint *pMP, float viewingCosLimit) (Frame.h:130, Frame.cc:656-719: the Nleft == -1 branch
 * with Pinhole::project, Pinhole.cpp:46-53, and MapPoint::PredictScale, MapPoint.cc:550-565) for the n map points in
 * slots[i] (slots == NULL: slots 0 .. n-1).  Outs (any may be NULL): in_view = the return value = mbTrackInView,
 * proj_x / proj_y = mTrackProjX / Y (-1 for a point rejected before Frame.cc:684, u / v after), and for in-view points
 * proj_xr = mTrackProjXR, depth = mTrackDepth, scale_level = mnTrackScaleLevel, view_cos = mTrackViewCos (unspecified
 * for the others).  Float arithmetic in a fixed order, one rounding per operation, glibc's logf.
 * A frame with Nleft != -1 (isInFrustumChecks on a KannalaBrandt8 pair, Frame.cc:721-800): VSG_ERR_UNSUPPORTED. */
int vsg_frame_is_in_frustum(vsg_frame *F, vsg_mappoints *mp, int n, const int32_t *slots, const vsg_frame_pose *pose,
                            float viewing_cos_limit, uint8_t *in_view, float *proj_x, float *proj_y, float *proj_xr,
                            float *depth, int32_t *scale_level, float *view_cos);

/* void Tracking::SearchLocalPoints() (Tracking.cc:3423-3495), its second loop (:3446-3466) and the
 * SearchByProjection(mCurrentFrame, mvpLocalMapPoints, th, bFarPoints, thFarPoints) it ends with (ORBmatcher.cc:42-143),
 * in one enqueue and one wait.  Map point i = slot slots[i] (NULL: slot i).  skip[i] != 0 (NULL: none) = the point
 * is never projected (mnLastFrameSeen == mCurrentFrame.mnId || isBad(), :3450-3453); its mbTrackInView is false.
 * viewing_cos_limit = 0.5 at :3455.  th, nnratio, scale_factors, nlevels, train_blocked, train_match and the return
 * value are those of vsg_frame_search_by_projection; far_points / th_far_points = bFarPoints / thFarPoints
 * (ORBmatcher.cc:53-54: an in-view point with mTrackDepth > thFarPoints is not searched).  pose->n_levels <= nlevels <= 16.
 * Optional outs: in_view[i], proj_x[i], proj_y[i] as above (what mmProjectPoints takes, :3462-3465), *n_to_match =
 * nToMatch (:3460).  The reference searches only when nToMatch > 0; with none in view nothing matches here either.
 * Nleft != -1: VSG_ERR_UNSUPPORTED. */
int vsg_frame_search_local_points(vsg_frame *F, vsg_mappoints *mp, int n, const int32_t *slots, const uint8_t *skip,
                                  const vsg_frame_pose *pose, float viewing_cos_limit, float th, float nnratio,
                                  int far_points, float th_far_points, const float *scale_factors, int nlevels,
                                  uint8_t *train_blocked, int32_t *train_match, uint8_t *in_view, float *proj_x,
                                  float *proj_y, int *n_to_match);

/* int ORBmatcher::SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, th, bMono) (ORBmatcher.h:50,
 * ORBmatcher.cc:1667-1878), both blocks (right camera :1786-1853 when CurrentFrame.Nleft != -1).  One entry per
 * LastFrame map point that projects into the image (:1690-1711):  u, v = uv;  ur = uv(0) - mbf * invzc (stereo gate
 * :1741-1747, used when Nleft == -1);  u_r, v_r = projection through Trl (:1788-1789; NULL when Nleft == -1);
 * last_octave = nLastOctave;  last_angle = kpLF.angle;  mp_desc / mp_observed as above.  direction: 0 = neither,
 * 1 = bForward, 2 = bBackward (:1683-1684) selects the level window of GetFeaturesInArea.  Returns nmatches after
 * the rotation-consistency filter; a match dropped by it also loses its blocked flag (mvpMapPoints[i] = NULL, :1869). */
int vsg_frame_search_by_projection_last(vsg_frame *cur, int n_q, const uint8_t *mp_desc, const uint8_t *mp_observed,
                                        const float *u, const float *v, const float *ur, const float *u_r,
                                        const float *v_r, const int32_t *last_octave, const float *last_angle,
                                        float th, int direction, const float *scale_factors, int nlevels,
                                        int check_orientation, uint8_t *train_blocked, int32_t *train_match);

/* int ORBmatcher::SearchByProjection(KeyFrame *pKF, Sim3f &Scw, vpPoints, vpMatched, th, ratioHamming)
 * (ORBmatcher.h:58, ORBmatcher.cc:430-528) and its twin that also records the source KeyFrame (ORBmatcher.h:62,
 * .cc:530-641: the adaptor sets vpMatchedKF[i] = vpPointsKFs[matched[i]]).  One entry per point that passes the
 * geometry (:446-487): u, v, radius = th * mvScaleFactors[nPredictedLevel], predicted_level.  matched[i] != -1 on
 * entry = vpMatched[i] already set (skipped as a candidate, :501); on return matched[i] = query index for the new
 * assignments (old entries keep their value).  Accept rule: bestDist <= TH_LOW * ratioHamming (:520).  Returns nmatches. */
int vsg_frame_search_by_projection_sim3(vsg_frame *kf, int n_q, const uint8_t *mp_desc, const float *u, const float *v,
                                        const float *radius, const int32_t *predicted_level, float ratio_hamming,
                                        int32_t *matched);

/* int ORBmatcher::SearchByProjection(Frame &CurrentFrame, KeyFrame *pKF, const set<MapPoint*> &sAlreadyFound, th,
 * ORBdist) (ORBmatcher.h:54, ORBmatcher.cc:1880-2000).  One entry per KeyFrame map point that is not bad, not in
 * sAlreadyFound and projects into the frame (:1905-1932): u, v, radius, predicted_level (window levels
 * [level-1, level+1], :1934), kf_angle = pKF->mvKeysUn[i].angle.  occupied[i] = (CurrentFrame.mvpMapPoints[i] != NULL)
 * on entry (:1946), updated in place incl. the rotation filter's reset (:1990); train_match as above. */
int vsg_frame_search_by_projection_kf(vsg_frame *cur, int n_q, const uint8_t *mp_desc, const float *u, const float *v,
                                      const float *radius, const int32_t *predicted_level, const float *kf_angle,
                                      int orb_dist, int check_orientation, uint8_t *occupied, int32_t *train_match);

/* The two searches above with their geometry on the device: the map points are those of a vsg_mappoints store, the
 * projection loop runs as a kernel in front of the window search (one enqueue, one wait), and only poses and slot lists
 * cross to the device.  Float arithmetic in a fixed order, one rounding per operation.  Frames with
 * Nleft != -1: VSG_ERR_UNSUPPORTED.  pose->n_levels <= nlevels <= 16.
 *
 * int ORBmatcher::SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, th, bMono) (ORBmatcher.cc:1667-1878)
 * as Tracking::TrackWithMotionModel calls it (Tracking.cc:2945-2965).  last = the resident LastFrame (its octaves are read
 * on the device, its angles from the host mirror); last_slots[i], one entry per feature of last, = the slot of
 * LastFrame.mvpMapPoints[i], or < 0 for "no map point, or mvbOutlier[i]" (:1688-1691).  cur_pose / last_pose =
 * CurrentFrame / LastFrame.GetPose() with the current camera's intrinsics; mb = CurrentFrame.mb, mono = bMono: bForward /
 * bBackward (:1677-1684) are derived here.  The invzc < 0 test, Pinhole::project, the bounds (:1699-1709), the radius
 * th * mvScaleFactors[nLastOctave] (:1715), the level window (:1719-1724) and ur = uv(0) - mbf * invzc (:1744) follow.
 * Return value, train_blocked and the rotation filter are those of vsg_frame_search_by_projection_last given the
 * projected points in order; train_match[i2] = index of the LAST-FRAME FEATURE whose map point feature i2 takes.
 * Optional outs: *direction (0 neither, 1 bForward, 2 bBackward); per last-frame feature projected[i] (reached
 * GetFeaturesInArea), u[i], v[i], ur[i] (0 where not projected).  A retry with 2 * th (Tracking.cc:2956-2961) is the
 * same call with another th: nothing else is sent again.  A slot >= capacity, last_slots == NULL, or a feature with a
 * slot whose octave lies outside [0, nlevels): VSG_ERR_INVALID, before anything is enqueued. */
int vsg_frame_search_last_frame(vsg_frame *cur, vsg_frame *last, vsg_mappoints *mp, const int32_t *last_slots,
                                const vsg_frame_pose *cur_pose, const vsg_frame_pose *last_pose, float mb, int mono,
                                float th, const float *scale_factors, int nlevels, int check_orientation,
                                uint8_t *train_blocked, int32_t *train_match, int *direction, uint8_t *projected, float *u,
                                float *v, float *ur);

/* int ORBmatcher::SearchByProjection(Frame &CurrentFrame, KeyFrame *pKF, const set<MapPoint*> &sAlreadyFound, th,
 * ORBdist) (ORBmatcher.cc:1880-2000) as Tracking::Relocalization calls it (Tracking.cc:3805, :3819).  Query i = slot
 * slots[i] = pKF->GetMapPointMatches()[i] for the n entries that hold a map point; skip[i] != 0 (NULL:
 * none) = isBad() || sAlreadyFound.count(pMP) (:1901).  Projection WITHOUT a sign test on the depth, the bounds, the band
 * 0.8f * mfMinDistance .. 1.2f * mfMaxDistance, PredictScale and radius = th * mvScaleFactors[nPredictedLevel]
 * (:1904-1930) follow.  kf_angle[i] = pKF->mvKeysUn[i].angle of query i (may be NULL when check_orientation == 0).
 * Return value, occupied and train_match (= query index) are those of vsg_frame_search_by_projection_kf given the
 * projected points in order.  Optional outs per query: projected[i], u[i], v[i], predicted_level[i] (0 where not
 * projected).  slots == NULL or a slot outside [0, capacity): VSG_ERR_INVALID, before anything is enqueued. */
int vsg_frame_search_keyframe_points(vsg_frame *cur, vsg_mappoints *mp, int n, const int32_t *slots, const uint8_t *skip,
                                     const vsg_frame_pose *pose, float th, int orb_dist, const float *scale_factors,
                                     int nlevels, int check_orientation, const float *kf_angle, uint8_t *occupied,
                                     int32_t *train_match, uint8_t *projected, float *u, float *v,
                                     int32_t *predicted_level);

/* The back end's routines that project map points into ONE KeyFrame, with their geometry on the device: the points are
 * those of a vsg_mappoints store, the per-point loop runs as a kernel in front of the window search (one enqueue, one
 * wait), and only the pose, the slot list and the skip flags cross to the device.  The four loops (ORBmatcher.cc:452-486,
 * :559-595, :1194-1241, :1360-1395) are one: p3Dc = Tcw * p3Dw, p3Dc(2) < 0 rejects, Pinhole::project,
 * KeyFrame::IsInImage (KeyFrame.cc:880-883: maximum exclusive, a NaN rejected) on the KeyFrame's `const int` bounds
 * (KeyFrame.h:419-422, the resident frame's own truncated toward zero as at KeyFrame.cc:52), the band 0.8f * mfMinDistance ..
 * 1.2f * mfMaxDistance, PO.dot(Pn) < 0.5 * dist3D rejects, PredictScale, radius = th * mvScaleFactors[nPredictedLevel].
 * Float arithmetic in a fixed order, one rounding per operation.  Query i = slot slots[i];
 * skip[i] != 0 (NULL: none) = the routine `continue`s before GetWorldPos().  pose = Tcw / Ow with the KeyFrame's
 * intrinsics: pKF->GetPose() / GetCameraCenter(), or for the Sim3 routines the caller's decomposition
 * Tcw = SE3f(Scw.rotationMatrix(), Scw.translation() / Scw.scale()), Ow = Tcw.inverse().translation() (:433-434,
 * :1340-1341).  pose->n_levels <= nlevels <= 16.  Optional outs per query: projected[i] (reached GetFeaturesInArea), u[i],
 * v[i], ur[i], predicted_level[i] (0 where not projected).  Checked before anything is enqueued: NULL handles, frame and
 * store on different devices, nlevels outside 1..16, pose->n_levels > nlevels, n < 0, slots == NULL or a slot outside
 * [0, capacity): VSG_ERR_INVALID; a KeyFrame with Nleft != -1 (bRight, mpCamera2: :1154-1159): VSG_ERR_UNSUPPORTED; n == 0
 * returns 0.  One target KeyFrame per call, as in the reference.
 *
 * int ORBmatcher::Fuse(KeyFrame *pKF, const vector<MapPoint*> &vpMapPoints, th, false) (ORBmatcher.cc:1148-1335) as
 * LocalMapping::SearchInNeighbors calls it for every neighbour (LocalMapping.cc:770, :800): the search.  skip[i] =
 * !pMP || isBad() || IsInKeyFrame(pKF) (:1177-1192).  Chi-square gate with inv_level_sigma2 = pKF->mvInvLevelSigma2
 * (:1269-1293), scan from 256.  best_idx / best_dist per QUERY, -1 / 256 when nothing qualifies; returns the count with
 * bestDist <= TH_LOW (:1310).  Results are those of vsg_frame_fuse given the projected points in order; the replace / add
 * walk stays vsg_fuse_decide. */
int vsg_frame_fuse_points(vsg_frame *kf, vsg_mappoints *mp, int n, const int32_t *slots, const uint8_t *skip,
                          const vsg_frame_pose *pose, float th, const float *scale_factors,
                          const float *inv_level_sigma2, int nlevels, int32_t *best_idx, int32_t *best_dist,
                          uint8_t *projected, float *u, float *v, float *ur, int32_t *predicted_level);
/* int ORBmatcher::Fuse(KeyFrame *pKF, Sim3f &Scw, vpPoints, th, vpReplacePoint) (ORBmatcher.cc:1337-1446) as
 * LoopClosing::SearchAndFuse calls it (LoopClosing.cc:2012, :2054).  skip[i] = isBad() || spAlreadyFound.count(pMP)
 * (:1356; the set is pKF->GetMapPoints(), :1344).  No gate, scan from INT_MAX (:1406): best_dist is INT_MAX when nothing
 * qualifies.  Results are those of vsg_frame_fuse_sim3 given the projected points in order. */
int vsg_frame_fuse_points_sim3(vsg_frame *kf, vsg_mappoints *mp, int n, const int32_t *slots, const uint8_t *skip,
                               const vsg_frame_pose *pose, float th, const float *scale_factors, int nlevels,
                               int32_t *best_idx, int32_t *best_dist, uint8_t *projected, float *u, float *v,
                               int32_t *predicted_level);
/* int ORBmatcher::SearchByProjection(KeyFrame *pKF, Sim3f &Scw, vpPoints, vpMatched, th, ratioHamming)
 * (ORBmatcher.cc:430-528) as LoopClosing calls it (LoopClosing.cc:735, :757, :944); the twin with vpPointsKFs (:530-641)
 * goes through the adaptor as for vsg_frame_search_by_projection_sim3.  skip[i] = isBad() || spAlreadyFound.count(pMP)
 * (:448).  matched (one entry per KeyFrame feature, -1 = vpMatched[i] not set, in / out), the accept rule
 * bestDist <= TH_LOW * ratioHamming (:520) and the return value are those of vsg_frame_search_by_projection_sim3 given the
 * projected points in order; a new entry holds the QUERY index. */
int vsg_frame_search_sim3_points(vsg_frame *kf, vsg_mappoints *mp, int n, const int32_t *slots, const uint8_t *skip,
                                 const vsg_frame_pose *pose, float th, float ratio_hamming, const float *scale_factors,
                                 int nlevels, int32_t *matched, uint8_t *projected, float *u, float *v,
                                 int32_t *predicted_level);

/* int Optimizer::PoseOptimization(Frame *pFrame) (Optimizer.h, Optimizer.cc:1063-1452: the !mpCamera2 branches
 * :1115-1180, the round loop :1254-1442, the pose recovery :1444-1451) on a resident frame and resident map points: the
 * link between the resident searches above, which project through the pose this routine produces.  One persistent
 * workgroup runs all four rounds (g2o's OptimizationAlgorithmLevenberg::solve, optimization_algorithm_levenberg.cpp:
 * 61-194, ten iterations of at most ten trials each; EdgeSE3ProjectXYZOnlyPose, OptimizableTypes.cpp:47-62, and
 * EdgeStereoSE3ProjectXYZOnlyPose, types_six_dof_expmap.cpp:365-437; Huber, robust_kernel_impl.cpp:78) in double, in one
 * enqueue and one wait; only the slot of each feature and a pose cross to the device.  The arithmetic is
 * csrc/vsg_pose_opt.h, which a host build reproduces bit for bit.
 *   - feat_slots[i], one per feature of F, = the slot of pFrame->mvpMapPoints[i], or < 0 for none.  A feature is stereo
 *     when the frame's u_right[i] >= 0 (:1118); a frame without u_right is all monocular.
 *   - Tcw = pFrame->GetPose(): unit_quaternion() as x y z w, translation().  EVERY round starts from it (:1263).
 *   - fx .. bf = the Frame's floats; inv_level_sigma2 = mvInvLevelSigma2, nlevels entries, nlevels in [1, 16].
 *   - Returns nInitialCorrespondences - nBad (:1451).  outlier = the storage of mvbOutlier: entry i is written ONLY for
 *     features with a slot (:1121, :1149, :1361-1367), the others keep their bytes.  chi2 (may be NULL): the float that
 *     was compared at the last classification that compared feature i (:1357).  res->q / t = vSE3_recov->estimate()
 *     (:1446; the caller narrows it to the Sophus::SE3f of :1447), n_initial, n_bad, rounds_run.
 *   - Fewer than 3 features with a slot (:1251): their outlier flags are cleared, res holds the input pose, returns 0,
 *     nothing is enqueued.  Fewer than 10 edges end the loop after one round (:1440).
 *   - hold_round = -1 runs everything.  hold_round = 2 runs rounds 0 and 1, then round 2's optimize(), and returns 0
 *     with res->held = 1, res->q / t = the estimate the host's plane step reads (:1296-1298) and outlier as after round
 *     1: the vS-Graphs refine_map_points step (:1270-1335) runs on the host HERE, and
 *     vsg_frame_pose_optimization_resume(F, removed, ...) finishes round 2's classification and round 3, with
 *     removed[i] != 0 (NULL: none) for the features whose map point that step dropped (mvpMapPoints[j] = NULL,
 *     mvbOutlier[j] = true): they stay flagged and are counted in nBad in both rounds (:1348-1353), and they leave
 *     optimizer.edges() (:1440).  If the loop ended before round 2, held = 0 and the call is complete.  The held state
 *     lives in a device buffer of the frame.  _resume with nothing held, after a call that rewrote the frame's features
 *     (vsg_frame_upload, vsg_frame_from_extractor*, vsg_orb_extract_to_frame*), or a second time: VSG_ERR_INVALID.
 * Checked before anything is enqueued (an error leaves no kernel behind and writes nothing): a NULL F, mp, feat_slots,
 * Tcw, inv_level_sigma2, outlier or res, a slot >= capacity, nlevels outside [1, 16], a feature with a slot whose octave
 * is >= nlevels, a hold_round other than -1 or 2, store and frame on different devices: VSG_ERR_INVALID; Nleft != -1
 * (EdgeSE3ProjectXYZOnlyPoseToBody :1182-1246, KannalaBrandt8): VSG_ERR_UNSUPPORTED.
 * vsg_frame_track_with_motion_model below runs a search and this routine in one enqueue. */
typedef struct vsg_pose_se3 {
  float q[4]; /* Tcw.unit_quaternion() as x y z w */
  float t[3]; /* Tcw.translation() */
} vsg_pose_se3;
typedef struct vsg_pose_result {
  double q[4], t[3];
  int32_t n_initial, n_bad, rounds_run, held;
} vsg_pose_result;
int vsg_frame_pose_optimization(vsg_frame *F, vsg_mappoints *mp, const int32_t *feat_slots, const vsg_pose_se3 *Tcw,
                                float fx, float fy, float cx, float cy, float bf, const float *inv_level_sigma2,
                                int nlevels, int hold_round, uint8_t *outlier, float *chi2, vsg_pose_result *res);
int vsg_frame_pose_optimization_resume(vsg_frame *F, const uint8_t *removed, uint8_t *outlier, float *chi2,
                                       vsg_pose_result *res);

/* Tracking's motion-model step on resident data as ONE enqueue and ONE wait: the projection kernel, the window search,
 * the ordered walk of the search (csrc/vsg_walks_dev.h: on the device what vsg_frame_search_last_frame does on the host
 * after its wait) and vsg_frame_pose_optimization, whose edges are the walk's matches in ascending feature order
 * (Optimizer.cc:1109-1180) and never leave the device in between.  Every call that is accepted gives, bit for bit, what
 * the two existing calls give with the caller's loops between them; the checks are stricter in one place (below).
 * Frames with Nleft != -1: VSG_ERR_UNSUPPORTED.  The intrinsics of the
 * solve are cur_pose's fx, fy, cx, cy, mbf; Tcw is the same pose as the caller's quaternion (both paths get the same
 * bits); inv_level_sigma2, nlevels (shared with the search, 1..16) and hold_round as in vsg_frame_pose_optimization.
 * Checked before anything is enqueued, with the codes of the two calls: everything vsg_frame_search_last_frame and
 * vsg_frame_pose_optimization check; here EVERY feature of cur must have its octave in [0, nlevels) (any of them may
 * end with a slot).
 * 2 * features + queries above about 16000 (the walk's state is one workgroup's LDS, kept to 64 KB by choice):
 * VSG_ERR_CAPACITY, also before anything is enqueued.  An error after an enqueue waits for the stream before it returns.
 * No error writes *res or an output array, or drops a hold that is pending on cur.
 *
 * bool Tracking::TrackWithMotionModel() (Tracking.cc:2945-3005): fill(mvpMapPoints, NULL) and SearchByProjection(
 * mCurrentFrame, mLastFrame, th, bMono) (:2945-2956); if nmatches < 20 the same once more with 2 * th from all-free
 * features (:2958-2963, a second enqueue and wait, in this rare case only); still below 20: return (:2967), here with
 * res->optimized = 0, the input pose, the wide search's matches and no outlier writes.  Then PoseOptimization (:2978) and
 * the discard loop (:2980-3005): a matched feature flagged outlier loses its slot and its flag is cleared.
 *   - cur .. check_orientation: as vsg_frame_search_last_frame (every feature of cur starts free).
 *   - feat_slots_out[i], one per feature of cur: the slot of mvpMapPoints[i] after the discard, or -1.  train_match (may
 *     be NULL): as vsg_frame_search_last_frame defines it, for the search whose matches were used.  outlier, chi2 (may be
 *     NULL): as vsg_frame_pose_optimization, entries of features with a match only; after the discard every written flag
 *     is 0.
 *   - res: pose = the solve's result (the input pose when it did not run); n_search = nmatches of the first search;
 *     wide = 1 when the 2 * th search ran; n_matches_searched = nmatches of the search that was used; optimized = 0 when
 *     both searches stayed below 20; n_matches = nmatches after the discard's decrements; n_matches_map = nmatchesMap,
 *     the survivors whose point has `observed` set in the store; direction as vsg_frame_search_last_frame.
 *   - hold_round = 2 is passed through: with res->pose.held = 1 the discard is NOT applied, feat_slots_out and outlier
 *     are as after round 1 and n_matches = n_matches_searched; the caller runs the plane step, calls
 *     vsg_frame_pose_optimization_resume(cur, ...) and discards itself.
 * Returns res->n_matches, or an error code. */
typedef struct vsg_track_result {
  vsg_pose_result pose;
  int32_t n_search, wide, n_matches_searched, optimized, n_matches, n_matches_map, direction, pad;
} vsg_track_result;
int vsg_frame_track_with_motion_model(vsg_frame *cur, vsg_frame *last, vsg_mappoints *mp, const int32_t *last_slots,
                                      const vsg_frame_pose *cur_pose, const vsg_frame_pose *last_pose, float mb, int mono,
                                      float th, const float *scale_factors, int nlevels, int check_orientation,
                                      const vsg_pose_se3 *Tcw, const float *inv_level_sigma2, int hold_round,
                                      int32_t *feat_slots_out, int32_t *train_match, uint8_t *outlier, float *chi2,
                                      vsg_track_result *res);

/* Tracking's local-map step on resident data as ONE enqueue and ONE wait: k_frustum and the window search exactly as
 * vsg_frame_search_local_points enqueues them, the ordered walk of that search on the device (csrc/vsg_walks_dev.h in its
 * local form: what vsg_frame_search_local_points does on the host after its wait) and vsg_frame_pose_optimization on the
 * walk's edges.  Every call that is accepted gives, bit for bit, what the two existing calls give with the caller's loops
 * between them.
 *
 * bool Tracking::TrackLocalMap() (Tracking.cc:3019-3131; pinhole, Nleft == -1, no IMU): the second loop of
 * SearchLocalPoints (:3446-3466, isInFrustum(pMP, 0.5)), SearchByProjection(mCurrentFrame, mvpLocalMapPoints, th,
 * bFarPoints, thFarPoints) (ORBmatcher.cc:42-143), Optimizer::PoseOptimization(&mCurrentFrame) (:3041,
 * Optimizer.cc:1063-1452) and the statistics loop (:3074-3095).
 * WHAT STAYS WITH THE CALLER: UpdateLocalMap (:3026); the first loop of SearchLocalPoints (:3426-3443: a bad point of the
 * frame becomes slot -1 in feat_slots_in, mnLastFrameSeen == mnId becomes skip[i]); IncreaseVisible (in_view) and
 * IncreaseFound (a feature that ends with a slot and no outlier flag); the choice of th (:3471-3491); the threshold on
 * mnMatchesInliers (:3100-3130).
 *   - F .. nlevels: as vsg_frame_search_local_points.
 *   - feat_slots_in[i], one per feature of F: the slot of mvpMapPoints[i] on entry, < 0 for none (what
 *     vsg_frame_track_with_motion_model returned).  No train_blocked array is sent: a feature is blocked on entry iff it
 *     has a slot whose point is `observed` in the store (ORBmatcher.cc:86-88), which the walk kernel derives on the device.
 *     A feature that holds an unobserved point can be taken by a local point (:130); after the walk a feature holds its
 *     claimant's slot, or else its entry slot.  There is no rotation filter in this routine.
 *   - Tcw, inv_level_sigma2, hold_round: as vsg_frame_pose_optimization; the intrinsics of the solve are pose's fx, fy, cx,
 *     cy, mbf.  The solve runs whatever the search found; fewer than 3 features with a slot (Optimizer.cc:1251): their
 *     outlier flags are cleared and res->pose holds the input pose.
 *   - only_tracking = mbOnlyTracking (:3084); drop_outliers = (mSensor == System::STEREO) (:3092).
 *   - feat_slots_out[i]: the slot of mvpMapPoints[i] after the walk; with drop_outliers (and no hold) an outlier's slot is -1
 *     (:3093) and its outlier flag STAYS set (unlike the motion-model discard).  train_match (may be NULL): as
 *     vsg_frame_search_local_points from all -1, an index into the n queried points.  outlier, chi2 (may be NULL): as
 *     vsg_frame_pose_optimization, written only for features that end the walk with a slot.  in_view, proj_x, proj_y (n
 *     entries each, any may be NULL): as vsg_frame_search_local_points, for IncreaseVisible and mmProjectPoints.
 *   - res: pose = the solve's result; n_to_match = nToMatch (:3460); n_matches_searched = the search's return value;
 *     n_matches_inliers = mnMatchesInliers: the features with a slot that are no outlier and, with only_tracking == 0, whose
 *     point is `observed`; walk_rounds = rounds the walk kernel took to its fixed point.
 *   - hold_round = 2 is passed through: with res->pose.held = 1 neither the statistics nor the drop are applied
 *     (n_matches_inliers = 0, the call returns 0), feat_slots_out and outlier are as after round 1; the caller runs the plane
 *     step, vsg_frame_pose_optimization_resume(F, ...) and both loops itself.
 *   - n == 0, every point skipped or nothing in view: exactly vsg_frame_pose_optimization on feat_slots_in, then the
 *     statistics.  A frame without features: returns 0 with the input pose, nothing is enqueued, no array is written.
 * Checked before anything is enqueued, with the codes of the calls it joins: everything vsg_frame_search_local_points and
 * vsg_frame_pose_optimization check (Nleft != -1: VSG_ERR_UNSUPPORTED); feat_slots_in == NULL or a slot >= capacity:
 * VSG_ERR_INVALID.  DEVIATIONS: EVERY feature of F must have its octave in [0, nlevels) (any of them may end with a slot),
 * else VSG_ERR_INVALID; 2 * features + n above about 16000 (the walk's state is one workgroup's LDS, kept to 64 KB by
 * choice): VSG_ERR_CAPACITY -- take the two-call path for such a local map.  Candidate lists that overflow are retried
 * as in vsg_frame_track_with_motion_model.  An error after an enqueue waits for the stream before it returns.  No error
 * writes *res or an output array, or drops a hold that is pending on F.
 * Returns res->n_matches_inliers, or an error code. */
typedef struct vsg_track_local_result {
  vsg_pose_result pose;
  int32_t n_to_match, n_matches_searched, n_matches_inliers, walk_rounds;
} vsg_track_local_result;
int vsg_frame_track_local_map(vsg_frame *F, vsg_mappoints *mp, int n, const int32_t *slots, const uint8_t *skip,
                              const vsg_frame_pose *pose, float viewing_cos_limit, float th, float nnratio, int far_points,
                              float th_far_points, const float *scale_factors, int nlevels, const int32_t *feat_slots_in,
                              const vsg_pose_se3 *Tcw, const float *inv_level_sigma2, int hold_round, int only_tracking,
                              int drop_outliers, int32_t *feat_slots_out, int32_t *train_match, uint8_t *outlier,
                              float *chi2, uint8_t *in_view, float *proj_x, float *proj_y, vsg_track_local_result *res);

/* int ORBmatcher::SearchBySim3(KeyFrame *pKF1, KeyFrame *pKF2, vpMatches12, S12, th) (ORBmatcher.h:76,
 * ORBmatcher.cc:1448-1665).  Direction 1 (:1489-1565): for each KF1 feature i1 with a usable, not yet matched map
 * point that projects into KF2: idx1[k] = i1, its descriptor, (u, v, radius, predicted level) in KF2; direction 2
 * (:1568-1643) likewise from KF2 into KF1.  best-only scans from INT_MAX, accept <= TH_HIGH, then the agreement pass
 * (:1646-1662): matches12[i1] = i2 where both directions agree, else -1.  n1 / n2 = feature counts of the two
 * KeyFrames (matches12 has n1 entries).  Returns nFound. */
int vsg_frame_search_by_sim3(vsg_frame *kf1, vsg_frame *kf2, int nq1, const int32_t *idx1, const uint8_t *desc1,
                             const float *u1, const float *v1, const float *radius1, const int32_t *level1, int nq2,
                             const int32_t *idx2, const uint8_t *desc2, const float *u2, const float *v2,
                             const float *radius2, const int32_t *level2, int32_t *matches12);

/* int ORBmatcher::Fuse(KeyFrame *pKF, const vector<MapPoint*> &vpMapPoints, th, bRight) (ORBmatcher.h:84,
 * ORBmatcher.cc:1148-1329): the search.  One entry per map point that passes :1176-1236: u, v, ur = u - bf * invz,
 * radius, predicted_level.  Candidates: GetFeaturesInArea(u, v, radius, bRight), level window, then the chi-square
 * gate on the reprojection error (:1267-1292: 7.8 with mvuRight >= 0, 5.99 without) with inv_level_sigma2 =
 * pKF->mvInvLevelSigma2.  best_idx[k] (index into mDescriptors, i.e. + NLeft for bRight) / best_dist[k]; -1 / 256 when
 * nothing qualifies.  A match is bestDist <= TH_LOW (:1308); the replace-vs-add decision on the MapPoint graph
 * (:1310-1324) is vsg_fuse_decide below. Returns the number of entries with bestDist <= TH_LOW. */
int vsg_frame_fuse(vsg_frame *kf, int n_q, const uint8_t *mp_desc, const float *u, const float *v, const float *ur,
                   const float *radius, const int32_t *predicted_level, int right, const float *inv_level_sigma2,
                   int nlevels, int32_t *best_idx, int32_t *best_dist);
/* int ORBmatcher::Fuse(KeyFrame *pKF, Sim3f &Scw, vpPoints, th, vpReplacePoint) (ORBmatcher.h:87,
 * ORBmatcher.cc:1331-1446): the search (scan from INT_MAX, level window only, no chi-square gate). */
int vsg_frame_fuse_sim3(vsg_frame *kf, int n_q, const uint8_t *mp_desc, const float *u, const float *v,
                        const float *radius, const int32_t *predicted_level, int32_t *best_idx, int32_t *best_dist);
/* The ordered decision pass of both Fuse overloads on flattened state, for callers that keep map points as ids:
 * slot_mp[i] = id of the map point in pKF->GetMapPoint(i) or -1 (updated in place as AddMapPoint /
 * ReplaceMapPointMatch would); mp_obs[id] = Observations(), mp_bad[id] = isBad() (updated by Replace as
 * MapPoint::Replace does for THIS keyframe: the survivor takes over the slot and the loser's observation count, the
 * loser turns bad).  query_mp[k] = id of the k-th query's map point.  action[k]: 0 none (bestDist > TH_LOW),
 * 1 AddObservation + AddMapPoint (:1321-1322), 2 pMP->Replace(pMPinKF) (:1315), 3 pMPinKF->Replace(pMP) (:1317),
 * 4 counted but nothing done (pMPinKF is bad), 5 (sim3 form) vpReplacePoint[k] = pMPinKF (:1436).  sim3_form selects
 * :1429-1444.  Returns nFused. */
int vsg_fuse_decide(int n_q, const int32_t *query_mp, const int32_t *best_idx, const int32_t *best_dist, int sim3_form,
                    int32_t *slot_mp, int n_slots, int32_t *mp_obs, uint8_t *mp_bad, int n_mp, int32_t *action,
                    int32_t *other_mp);

/* int ORBmatcher::SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize) (ORBmatcher.h:68,
 * ORBmatcher.cc:643-756) with both frames resident: only vbPrevMatched (x, y per F1 keypoint) goes up;
 * F2.GetFeaturesInArea(x, y, windowSize, 0, 0) (:663) runs on F2's resident grid for the level-0 keypoints of F1. */
int vsg_frame_search_for_initialization(vsg_frame *f1, vsg_frame *f2, const float *prev_x, const float *prev_y,
                                        int window_size, float nnratio, int check_orientation, int32_t *matches12);

/* SearchByBoW(KeyFrame*, Frame&) / (KeyFrame*, KeyFrame*) (ORBmatcher.cc:226-428, 758-900) on resident descriptors:
 * only the FeatureVectors and the validity flags go up.  Same outputs as vsg_search_by_bow_kf_f_stereo / _kf_kf.
 * With ALL FeatureVector arrays NULL the FeatureVectors both frames keep resident since their vsg_frame_bow_transform
 * (Frame::mFeatVec, any number of features) are joined on the device and only the flags go up.  An empty frame, or a
 * ComputeBoW with an empty vocabulary, gives 0 matches and every output -1, as in the reference; otherwise
 * VSG_ERR_INVALID when either frame never had its ComputeBoW since its features were last written (nothing is left
 * running on the calling thread's stream when this or any other error is returned).  The flag and match arrays of an empty
 * frame may be NULL.  Checked before anything is enqueued: NULL handles, inputs or outputs, frames on different devices, only
 * SOME of the FeatureVector arrays NULL, and in the host-FeatureVector form what vsg_search_by_bow_kf_f checks of a
 * FeatureVector (node ids that do not strictly ascend, offsets that do not ascend from 0, an idx outside [0, n)):
 * VSG_ERR_INVALID. */
int vsg_frame_search_by_bow_kf_f(vsg_frame *kf, const uint8_t *kf_valid, const int32_t *kf_node_id,
                                 const int32_t *kf_off, const int32_t *kf_idx, int kf_nodes, vsg_frame *f,
                                 const int32_t *f_node_id, const int32_t *f_off, const int32_t *f_idx, int f_nodes,
                                 float nnratio, int check_orientation, int32_t *match_f);
int vsg_frame_search_by_bow_kf_kf(vsg_frame *kf1, const uint8_t *valid1, const int32_t *node_id1, const int32_t *off1,
                                  const int32_t *idx1, int nodes1, vsg_frame *kf2, const uint8_t *valid2,
                                  const int32_t *node_id2, const int32_t *off2, const int32_t *idx2, int nodes2,
                                  float nnratio, int check_orientation, int32_t *matches12);
/* SearchForTriangulation(KeyFrame*, KeyFrame*, ...) (ORBmatcher.cc:902-1146) with both KeyFrames resident (LocalMapping::
 * CreateNewMapPoints calls it for the current keyframe against each of its 10-20 best covisible neighbours,
 * LocalMapping.cc:389: the current keyframe's descriptors go up once, not once per neighbour).  Arguments and result as
 * vsg_search_for_triangulation; angles come from the frames' host mirrors.  Checked before anything is enqueued: NULL
 * handles, flags or output, frames on different devices, and what vsg_search_for_triangulation checks of the FeatureVectors
 * and of pair_ok / pair_off: VSG_ERR_INVALID. */
int vsg_frame_search_for_triangulation(vsg_frame *kf1, const uint8_t *eligible1, const int32_t *node_id1,
                                       const int32_t *off1, const int32_t *idx1, int nodes1, vsg_frame *kf2,
                                       const uint8_t *eligible2, const int32_t *node_id2, const int32_t *off2,
                                       const int32_t *idx2, int nodes2, const uint32_t *pair_ok, const int32_t *pair_off,
                                       int check_orientation, int32_t *matches12);
/* SearchForTriangulation(KeyFrame*, KeyFrame*, ...) (ORBmatcher.cc:902-1146) on two resident KeyFrames with the geometric
 * predicate evaluated on the device too: no caller-side loop over the pairs and no bitmask.  LocalMapping::
 * CreateNewMapPoints calls it for the new keyframe against each of its best covisible neighbours (LocalMapping.cc:389-460);
 * one neighbour per call, as in the reference.  no_mpX[i] = !pKFX->GetMapPoint(i) (:969-973, :1001-1002) is the only
 * per-feature state that goes up; everything else the predicate reads per keypoint is resident (mvKeysUn x, y, octave,
 * mvuRight: a frame uploaded without mvuRight counts as all -1).  Per pair, in float, a fixed order and one rounding per
 * operation (csrc/vsg_epipolar.h):
 *   bOnlyStereo with a mono keypoint on either side: no candidate (:976-980, :1004-1008);
 *   both keypoints mono: distex = ep[0] - x2, distey = ep[1] - y2, distex * distex + distey * distey <
 *     100 * scale_factors2[octave2] rejects (:1023-1031; also under bCoarse);
 *   unless bCoarse, Pinhole::epipolarConstrain (Pinhole.cpp:118-141): a = x1 * F12(0,0) + y1 * F12(1,0) + F12(2,0), b and c
 *     with columns 1 and 2, num = a * x2 + b * y2 + c, den = a * a + b * b, den == 0 rejects, dsqr = num * num / den, accept
 *     iff (double)dsqr < 3.84 * (double)level_sigma2_2[octave2] (a double comparison, as in the reference).
 * F12 (row-major) = K1.transpose().inverse() * hat(t12) * R12 * K2.inverse() (Pinhole.cpp:121-124) and ep =
 * pKF2->mpCamera->project(T2w * Cw) (:913-915) depend on the two keyframes only: the caller computes them once per call with
 * the reference's own expressions.  scale_factors2 / level_sigma2_2 = pKF2->mvScaleFactors / mvLevelSigma2, nlevels entries.
 * With ALL six FeatureVector arrays NULL the FeatureVectors both frames keep resident since their vsg_frame_bow_transform are
 * joined on the device, under the rules of vsg_frame_search_by_bow_kf_kf: an empty frame or an empty vocabulary gives 0
 * matches, a frame that never had its ComputeBoW VSG_ERR_INVALID.  matches12 and the return value (nmatches after the
 * rotation-histogram filter) are those of vsg_frame_search_for_triangulation given eligible = no_mp (&& stereo under
 * bOnlyStereo) and the bitmask of this predicate.  Checked before anything is enqueued: NULL handles, inputs or outputs,
 * frames on different devices, nlevels outside 1..16, a keypoint of kf2 whose octave lies outside [0, nlevels), only SOME of
 * the FeatureVector arrays NULL, and in the host-FeatureVector form node ids that do not strictly ascend, offsets that do not
 * ascend from 0 or an idx outside [0, n): VSG_ERR_INVALID; a frame with Nleft != -1 (mpCamera2: :929-937, :1033-1071): VSG_ERR_UNSUPPORTED.  An error after
 * the enqueue waits for the stream before it returns. */
int vsg_frame_search_for_triangulation_epipolar(vsg_frame *kf1, const uint8_t *no_mp1, const int32_t *node_id1,
                                                const int32_t *off1, const int32_t *idx1, int nodes1, vsg_frame *kf2,
                                                const uint8_t *no_mp2, const int32_t *node_id2, const int32_t *off2,
                                                const int32_t *idx2, int nodes2, const float F12[9], const float ep[2],
                                                const float *scale_factors2, const float *level_sigma2_2, int nlevels,
                                                int only_stereo, int coarse, int check_orientation, int32_t *matches12);
/* ---- LocalMapping::CreateNewMapPoints on resident keyframes (LocalMapping.cc:382-710) -------------------------------
 * The loop over one neighbour's matches (:475-708): per matched pair (idx1 of mpCurrentKeyFrame = kf1, idx2 of pKF2 = kf2)
 * the parallax test, GeometricTools::Triangulate (GeometricTools.cc:47-66) or KeyFrame::UnprojectStereo (KeyFrame.cc:
 * 885-902), the two depth signs, the two reprojection gates, the scale-consistency gate, and for an accepted pair the new
 * MapPoint written straight into a resident store: SetWorldPos, ComputeDistinctiveDescriptors and UpdateNormalAndDepth of a
 * point with exactly two observations.  Both keyframes have Nleft == -1 and the Pinhole camera.  One source for host and
 * device (csrc/vsg_triangulate.h): float arithmetic in the reference's order, one rounding per
 * operation, comparisons as the reference writes them (a NaN takes the reference's branch), with these quirks kept:
 *   - cosParallaxStereo2 is taken only when kf1's keypoint is mono (the `else if (bStereo2)` of :570);
 *   - the float cosParallaxRays is compared with the DOUBLE literals 0.9996 (inertial) / 0.9998 (:582), the squared
 *     reprojection errors with 5.991 * sigma2 / 7.8 * sigma2 in double (:632, :643), invz = (float)(1.0 / z) (:624);
 *   - kf2's u2_r uses the CURRENT keyframe's mbf (:663): kf1.mbf is read, kf2.mbf never;
 *   - Triangulate's right singular vector comes from a one-sided Jacobi in DOUBLE (6 sweeps) on the float A of :50-53, not
 *     from Eigen's float JacobiSVD: a deviation of arithmetic class, recorded in DESIGN.md beside the pose solve's LDL^T.
 * Reason codes (uint8 per feature of kf1) and source codes (what countStereo counts, :693): */
#define VSG_TRI_ACCEPTED 0
#define VSG_TRI_LOW_PARALLAX 1  /* :600-603 */
#define VSG_TRI_W_ZERO 2        /* GeometricTools.cc:59 */
#define VSG_TRI_STEREO_DEPTH 3  /* KeyFrame.cc:888: mvDepth <= 0 */
#define VSG_TRI_Z1 4            /* :613 */
#define VSG_TRI_Z2 5            /* :617 */
#define VSG_TRI_REPROJ1 6       /* :632 / :643 */
#define VSG_TRI_REPROJ2 7       /* :657 / :668 */
#define VSG_TRI_DIST_ZERO 8     /* :679 */
#define VSG_TRI_FAR 9           /* :682 */
#define VSG_TRI_SCALE_RATIO 10  /* :688 */
#define VSG_TRI_NO_FREE_SLOT 11 /* accepted by every gate, but free_slots was used up: nothing is written for it */
#define VSG_TRI_NO_MATCH 255    /* matches12[idx1] < 0 */
#define VSG_TRI_FROM_TRIANGULATE 0
#define VSG_TRI_FROM_STEREO1 1 /* mpCurrentKeyFrame->UnprojectStereo(idx1) (:592) */
#define VSG_TRI_FROM_STEREO2 2 /* pKF2->UnprojectStereo(idx2) (:598) */
/* kf1 / kf2 = the two cameras (Rcw, tcw, Ow, fx, fy, cx, cy and kf1's mbf are read; log_scale_factor and n_levels are not);
 * ratio_factor = 1.5f * mpCurrentKeyFrame->mfScaleFactor (:422); inertial = mbInertial; far_points / th_far_points =
 * mbFarPoints / mThFarPoints; kf2_first = std::less<KeyFrame *>()(pKF2, mpCurrentKeyFrame): the new point's
 * mObservations is a std::map<KeyFrame *, ...>, with two observations both rows of ComputeDistinctiveDescriptors have
 * median 0 and the FIRST in the map's order wins (MapPoint.cc:406), and UpdateNormalAndDepth sums in that order. */
typedef struct vsg_triangulation_params {
  vsg_frame_pose kf1, kf2;
  float ratio_factor, th_far_points;
  int32_t inertial, far_points, kf2_first;
} vsg_triangulation_params;
/* The per-keyframe inputs of the stereo branches, attached to a resident frame once per keyframe: xyz_c[3 i ..] = x3Dc of
 * KeyFrame::UnprojectStereo(i) (KeyFrame.cc:887-894: z = mvDepth[i], x = (mvKeys[i].pt.x - cx) * z * invfx, y likewise --
 * mvKeys, the RAW keypoints, which the frame does not hold), cos_parallax[i] = cos(2 * atan2(mb / 2, mvDepth[i])) (:569),
 * both computed by the caller with the reference's own expressions (as F12 and the epipole of the search).  Entries of
 * features with mvuRight < 0 are never read.  The two calls below return VSG_ERR_INVALID before they enqueue anything when
 * a frame that was given an mvuRight with any entry >= 0 (or filled by vsg_orb_extract_to_frame_rgbd) has nothing
 * attached; a frame without mvuRight needs nothing.  Dropped by the next upload into the frame.  NULL frame or array, or
 * a frame never uploaded: VSG_ERR_INVALID.  One copy on the calling thread's stream, waited for. */
int vsg_frame_set_stereo_points(vsg_frame *f, const float *xyz_c, const float *cos_parallax);
/* The loop :475-708 for a match list the caller holds: matches12[n1] as the searches return it (-1: none), walked in
 * ascending idx1 as the reference walks vMatchedIndices.  scale_factorsX / level_sigma2_X = mvScaleFactors / mvLevelSigma2
 * of kfX, nlevels entries each (nlevels = mnScaleLevels in 1..16).  Outputs, each n1 entries (x3d 3 n1), all required:
 * reason / source as above (a feature without a match: 255 / 0), x3d = x3D as far as the reference assigned it (zeros
 * before), new_slot = the slot of the point the pair created or -1, *n_created = how many.
 *   mp == NULL: geometry only; free_slots / n_free are not read, nothing is created, an accepted pair has reason 0.
 *   mp != NULL: the k-th accepted pair in ascending idx1 takes free_slots[k]; the device writes that slot's world_pos = x3D,
 *     desc (row idx1 of kf1, or row idx2 of kf2 under kf2_first), normal, min_dist, max_dist (UpdateNormalAndDepth with
 *     mpRefKF = mpCurrentKeyFrame: csrc/vsg_observations.h on the two-entry list) and observed = 1.  Accepted pairs beyond
 *     n_free get VSG_TRI_NO_FREE_SLOT and write nothing.  Slots that are not assigned stay byte-identical.
 * Checked before anything is enqueued (outputs untouched): NULL handles, params, tables or outputs, frames and store on
 * different devices, nlevels outside 1..16, a keypoint of EITHER frame whose octave lies outside [0, nlevels), a match
 * outside [0, n2), n_free < 0, a free_slots entry outside [0, capacity) or listed twice, a frame with stereo keypoints and
 * no attachment: VSG_ERR_INVALID; Nleft != -1 on either frame (:482-554): VSG_ERR_UNSUPPORTED.  One enqueue on the
 * calling thread's stream and one wait; an error after the enqueue waits for the stream before it returns.  The caller
 * clears no_mp1[idx1] / no_mp2[idx2] for created points between neighbours (:699-700). */
int vsg_frame_triangulate_matches(vsg_frame *kf1, vsg_frame *kf2, const int32_t *matches12,
                                  const vsg_triangulation_params *params, const float *scale_factors1,
                                  const float *level_sigma2_1, const float *scale_factors2, const float *level_sigma2_2,
                                  int nlevels, vsg_mappoints *mp, const int32_t *free_slots, int n_free, uint8_t *reason,
                                  uint8_t *source, float *x3d, int32_t *new_slot, int32_t *n_created);
/* One neighbour of CreateNewMapPoints (:456-708) in ONE enqueue and ONE wait: vsg_frame_search_for_triangulation_epipolar
 * (its arguments, both FeatureVector forms, and its checks), the rotation-consistency filter (ORBmatcher.cc:1100-1118:
 * rot_bin per match, the 30-bin count and ComputeThreeMaxima, here on the device), then vsg_frame_triangulate_matches on
 * the filtered matches.  matches12 is the list AFTER the filter and the return value its count; the other outputs, the
 * store writes and the checks are those of the two calls.  An all-neighbours call is deliberately not offered: the
 * reference leaves the loop between neighbours (CheckNewKeyFrames, :430) and the caller updates no_mp1 there. */
int vsg_frame_create_new_map_points(vsg_frame *kf1, const uint8_t *no_mp1, const int32_t *node_id1, const int32_t *off1,
                                    const int32_t *idx1, int nodes1, vsg_frame *kf2, const uint8_t *no_mp2,
                                    const int32_t *node_id2, const int32_t *off2, const int32_t *idx2, int nodes2,
                                    const float F12[9], const float ep[2], int only_stereo, int coarse,
                                    int check_orientation, const vsg_triangulation_params *params,
                                    const float *scale_factors1, const float *level_sigma2_1, const float *scale_factors2,
                                    const float *level_sigma2_2, int nlevels, vsg_mappoints *mp, const int32_t *free_slots,
                                    int n_free, int32_t *matches12, uint8_t *reason, uint8_t *source, float *x3d,
                                    int32_t *new_slot, int32_t *n_created);
/* Sim3Solver (Sim3Solver.cc; LoopClosing.cc:678-690) on resident map points: EVERY RANSAC hypothesis in one call.
 * Hypothesis k depends on its three sampled correspondences alone and iterate's stopping rule (:215-291, called until
 * bConverge || bNoMore) is a function of the hypotheses' inlier counts c[k]: converged at the FIRST k with
 * c[k] > min_inliers (mnIterations = k + 1), otherwise bNoMore with the members holding the LAST k that reaches the
 * maximum.  So the call computes all n_hyp hypotheses side by side and selects.
 *   Correspondence i (mvpMapPoints1[i], mvpMapPoints2[i]) = slot slots1[i] of mp1 and slot slots2[i] of mp2 (mp2 may be
 * mp1; a merge candidate lives in another map).  kf1 / kf2 = pKF1 / pKF2: Rcw, tcw, fx, fy, cx, cy are read, nothing else;
 * X3Dc2 goes through kf2's pose also for a point matched through another keyframe pKFm (:107) -- only the sigma is pKFm's.
 * max_err1 / max_err2 = mvnMaxError1 / 2 AS THE COMPARISON SEES THEM: 9.210 * sigmaSquare is a double stored into a
 * std::vector<size_t> (Sim3Solver.h:72-73), so the threshold is truncated toward zero and `err < mvnMaxError[i]` compares
 * with that integer as a float: pass (float)(size_t)(9.210 * sigma2).  fix_scale = mbFixScale, min_inliers =
 * mRansacMinInliers, n_hyp = mRansacMaxIts after SetRansacParameters (vsg_sim3_ransac_iterations), samples[3 k .. 3 k + 2] =
 * the three correspondence indices of hypothesis k in the order they fill columns 0..2 (vsg_sim3_draw_samples).
 *   Outputs: inlier[i] = mvbInliersi of the returned hypothesis (the caller scatters it to vbInliers[mvnIndices1[i]]);
 * res as below; hyp_inliers[k] / hyp_T12[16 k ..] (either may be NULL) = mnInliersi / mT12i of every hypothesis.
 * n < min_inliers (:222-226): no_more = 1, the identity, best_hypothesis -1, flags cleared, nothing is enqueued.
 *   Arithmetic (csrc/vsg_sim3.h, host and device from one source): float in the reference's order;
 * the eigenvector of N comes from a double Jacobi instead of Eigen's float EigenSolver and the rotation from the quaternion
 * directly instead of atan2 + SO3f::exp, both deviations by rounding; a zero imaginary part gives the reference's NaN
 * rotation and no inlier.  NaNs in res and hyp_T12 are canonical.
 *   Checked before anything is enqueued (an error writes nothing and leaves no kernel behind), VSG_ERR_INVALID: NULL
 * handles, poses, res, samples, or (n > 0) arrays; stores on different devices; n < 0; a slot outside [0, capacity) of its
 * store; n_hyp outside [1, 1024]; min_inliers < 0; and when n >= min_inliers: n < 3, a sample outside [0, n), two equal
 * samples in one triple.  One enqueue (three kernels) on the calling thread's stream and one wait; only the indices, the
 * thresholds, two poses and the samples cross to the device. */
typedef struct vsg_sim3_result {
  float R12[9], t12[3], s12, T12[16]; /* mBestRotation (row-major), mBestTranslation, mBestScale, mBestT12 (row-major) */
  int32_t converged, no_more, n_inliers, best_hypothesis, iterations; /* bConverge, bNoMore, mnBestInliers, k, mnIterations */
} vsg_sim3_result;
int vsg_mappoints_sim3_ransac(vsg_mappoints *mp1, vsg_mappoints *mp2, int n, const int32_t *slots1, const int32_t *slots2,
                              const float *max_err1, const float *max_err2, const vsg_frame_pose *kf1,
                              const vsg_frame_pose *kf2, int fix_scale, int min_inliers, int n_hyp, const int32_t *samples,
                              uint8_t *inlier, vsg_sim3_result *res, int32_t *hyp_inliers, float *hyp_T12);
/* Sim3Solver::SetRansacParameters (:120-144): mRansacMaxIts for n correspondences, with the float epsilon and
 * max(1, min(nIterations, max_iterations)).  Host only.  n < 0 or min_inliers < 0: VSG_ERR_INVALID. */
int vsg_sim3_ransac_iterations(double probability, int min_inliers, int max_iterations, int n);
/* The draw of :242-256 for n_hyp hypotheses: per hypothesis a copy of mvAllIndices (0 .. n-1), then three times
 * randi = random_int(0, size - 1, ctx), the element is taken, back() moves into its place, pop_back().  random_int == NULL:
 * DUtils::Random::RandomInt's formula over rand() (Random.cpp:47-50).  Host only.  n < 3, n_hyp < 0, NULL samples, or a
 * random_int result outside its range: VSG_ERR_INVALID. */
int vsg_sim3_draw_samples(int n, int n_hyp, int (*random_int)(int lo, int hi, void *ctx), void *ctx, int32_t *samples);
/* int Optimizer::OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale, mAcumHessian, bAllPoints) (Optimizer.h,
 * Optimizer.cc:3261-3529; called at LoopClosing.cc:538 and :747) on two resident keyframes and resident map points: the
 * link between vsg_mappoints_sim3_ransac above and vsg_frame_search_sim3_points, which projects through the g2oS12 this
 * routine refines.  One persistent workgroup gathers the pairs (:3313-3450), runs optimize(5), the first check on the
 * errors AS THE LAST computeActiveErrors LEFT THEM (:3452-3486), the `< 10` gate, optimize(5 or 10) without the kernel and
 * the second check on fresh errors (:3488-3522), in double, in one enqueue and one wait; only the slots and indices of the
 * pairs, two poses and g2oS12 cross to the device.  The Jacobian is g2o's NUMERIC one (base_binary_edge.hpp:131-205,
 * central differences with delta = 1e-9 through VertexSim3Expmap::oplusImpl, OptimizableTypes.h:172-181): neither edge
 * defines linearizeOplus.  The arithmetic is csrc/vsg_sim3_opt.h, which a host build reproduces bit for bit (DESIGN.md
 * section 8).
 *   - Entry i, one per feature of kf1 (vpMatches1.size() = N): slots1[i] = the slot of vpMapPoints1[i] in mp1, slots2[i]
 *     = the slot of vpMatches1[i] in mp2 (mp2 may be mp1), either < 0 for a missing OR BAD point: every such branch of
 *     :3315-3373 adds no edge and leaves the match alone.  idx2[i] = get<0>(pMP2->GetIndexInKeyFrame(pKF2)) or < 0;
 *     level2[i] = pMP2->mnTrackScaleLevel, read only when idx2[i] < 0.
 *   - pose1 / pose2 = the keyframes' GetRotation(), GetTranslation() (Rcw, tcw) and Pinhole parameters (fx, fy, cx, cy);
 *     nothing else of them is read.  inv_level_sigma2_1 / _2 = mvInvLevelSigma2 of pKF1 / pKF2, nlevels entries each.
 *   - S12 = g2oS12 taken as it is (not normalised); th2, fix_scale = bFixScale, all_points = bAllPoints.
 *   - state[i], written for ALL i: 0 = no edge, match untouched; 1 = inlier; 2 = vpMatches1[i] nulled at the first check;
 *     3 = nulled at the second; 4 = skipped for P3D2c.z < 0 (:3381); 5 = skipped for i2 < 0 && !bAllPoints (:3375).  A
 *     skipped entry keeps its match.  chi2[2 i], chi2[2 i + 1] (chi2 may be NULL) = the two doubles last compared for pair
 *     i (e12, e21), NaN canonical; entries without an edge keep their bytes.
 *   - Returns nIn (:3528), or 0 when nCorrespondences - nBad < 10 (:3494): the bad matches are nulled by then and g2oS12
 *     is NOT updated (res->updated = 0, res->S12 = the input, byte for byte).  res->more_iterations = nMoreIterations.
 *     mAcumHessian is only set to zero by the reference (:3502): the caller does that.
 *   - No entry with both slots: nothing is enqueued, res holds the input S12, returns 0.
 * Checked before anything is enqueued (an error writes nothing and leaves no kernel behind), VSG_ERR_INVALID: a NULL kf1,
 * kf2, mp1, mp2, slots1, slots2, idx2, level2, pose1, pose2, either sigma table, S12, state or res; stores or frames on
 * different devices; a slot >= its store's capacity; on an entry with both slots: idx2[i] >= kf2's feature count, and --
 * unless it is skipped for i2 < 0 && !all_points -- an octave of kf1's feature i, of kf2's feature idx2[i], or a level2[i]
 * (idx2[i] < 0) outside [0, nlevels); nlevels outside [1, 16]; th2 not finite or <= 0.  Nleft != -1 on either keyframe
 * (KannalaBrandt8 pairs): VSG_ERR_UNSUPPORTED, as in vsg_frame_pose_optimization.  The scratch lives in the calling
 * thread's arena, so two threads may optimise on the same stores and keyframes at the same time. */
typedef struct vsg_sim3d { double q[4], t[3], s; } vsg_sim3d;             /* g2o::Sim3: r as x y z w, t, s */
typedef struct vsg_sim3_opt_result {
  vsg_sim3d S12;                 /* g2oS12 on return: the input when the call returned before :3526 */
  int32_t n_correspondences, n_bad, n_in, n_in_kf2, n_out_kf2, more_iterations, updated;
} vsg_sim3_opt_result;
int vsg_frame_optimize_sim3(vsg_frame *kf1, vsg_frame *kf2, vsg_mappoints *mp1, vsg_mappoints *mp2,
                            const int32_t *slots1, const int32_t *slots2, const int32_t *idx2, const int32_t *level2,
                            const vsg_frame_pose *pose1, const vsg_frame_pose *pose2,
                            const float *inv_level_sigma2_1, const float *inv_level_sigma2_2, int nlevels,
                            const vsg_sim3d *S12, float th2, int fix_scale, int all_points,
                            uint8_t *state, double *chi2, vsg_sim3_opt_result *res);
/* Frame::ComputeBoW (Frame.cc:882-889) on the resident descriptors; outputs as vsg_bow_transform. */
int vsg_frame_bow_transform(vsg_vocab *voc, vsg_frame *f, int levelsup, int32_t *bow_ids, double *bow_vals,
                            int bow_cap, int *n_bow, int32_t *fv_node, int32_t *fv_off, int32_t *fv_idx, int fv_cap,
                            int *n_fv, int32_t *word_of, int32_t *node_of, double *weight_of);
/* Frame::ComputeStereoMatches (Frame.cc:957-1127) on two resident feature sets (left / right eye of one stereo
 * Frame, straight out of the two extractors): nothing but mvuRight / mvDepth crosses PCIe. */
int vsg_frame_stereo_matches(vsg_orb *hl, int frame_l, vsg_orb *hr, int frame_r, vsg_frame *fl, vsg_frame *fr,
                             float mb, float mbf, float *u_right, float *depth);

/* Frame::ComputeStereoMatches (Frame.cc:957-1127) + Frame::ComputeBoW (Frame.cc:882-889) + ORBmatcher::SearchByBoW(KeyFrame*,
 * Frame&, ...) (ORBmatcher.cc:226-428) of one stereo Frame in ONE enqueue and ONE wait: what depends only on two resident
 * frames shares a stream round trip instead of paying three.  Arguments as vsg_frame_stereo_matches (fl / fr = the resident
 * left / right eye; *n_stereo = matches kept by the median cut), vsg_frame_bow_transform (of fl; its FeatureVector also
 * stays resident in fl) and vsg_frame_search_by_bow_kf_f with NULL FeatureVector arrays (kf = a frame whose own ComputeBoW
 * ran earlier; kf == NULL: no search, match_f / n_match are not touched).  Results are those of the three blocking calls.
 * A kf with features that never had its ComputeBoW is refused (VSG_ERR_INVALID) before anything is enqueued; an error after
 * the first enqueue waits for the stream before it returns.  An fl of more than 2048 features has its FeatureVector
 * assembled on the host after the wait and the search follows behind a second wait; smaller frames take exactly one. */
int vsg_frame_stereo_bow_search(vsg_orb *hl, int frame_l, vsg_orb *hr, int frame_r, vsg_frame *fl, vsg_frame *fr, float mb,
                                float mbf, float *u_right, float *depth, int *n_stereo, vsg_vocab *voc, int levelsup,
                                int32_t *bow_ids, double *bow_vals, int bow_cap, int *n_bow, int32_t *fv_node,
                                int32_t *fv_off, int32_t *fv_idx, int fv_cap, int *n_fv, vsg_frame *kf,
                                const uint8_t *kf_valid, float nnratio, int check_orientation, int32_t *match_f,
                                int *n_match);

/* ---- Frame sharding over the GPUs of one node (one process per GPU) -------------------------------
 * The reference has no distributed layer.  Extraction shards by frame (or camera stream) with no collective; the
 * neighbour's features that matching frame t against t-1 needs travel as fixed-capacity per-frame records
 *   { int32 n, int32 monoIndex, uint32 flags, pad to 16 | KeyPoint[cap] (padded to 16) | uint8 desc[cap][32] | pad to 64 }
 * (flags bit 0 = VSG_SHARD_FLAG_TRUNCATED: the frame held more keypoints than the record's capacity; n and monoIndex
 * are clamped to it.  Slots of a partial batch -- nframes < frames_per_rank -- are sent with n = 0.)
 * in ONE ncclAllGather (RCCL over xGMI) per batch, enqueued on the caller's stream.  RCCL is loaded on first use
 * (dlopen); VSG_ERR_UNSUPPORTED when it is not available.
 *   vsg_shard_unique_id   rank 0 creates the 128-byte ncclUniqueId; the caller hands it to every rank (MPI, a file,
 *                         torch.distributed.broadcast, ...)
 *   vsg_shard_create      ncclCommInitRank + the send / receive record buffers for `frames_per_rank` frames per batch
 *   vsg_shard_all_gather  packs this rank's batch (the device outputs of vsg_orb_extract_batch_device: d_counts
 *                         [nframes][2], d_kps / d_desc [nframes][src_capacity]) and all-gathers; asynchronous on `stream`
 *   vsg_shard_record      device pointers of frame `frame` of rank `rank` in the gathered block: they can be passed
 *                         straight to vsg_hamming_block_best2_device / vsg_frame_* (valid until the next all-gather)
 *   vsg_shard_frame_owner / vsg_shard_stream_owner   the partition: frame f -> rank f mod world; camera stream s of
 *                         n_streams -> rank s (world <= n_streams: s mod world), a stream's frames round-robin over the
 *                         ranks {s, s + n_streams, ...} when there are more ranks than streams (4 cameras on 8 GPUs) */
typedef struct vsg_shard vsg_shard;
#define VSG_SHARD_FLAG_TRUNCATED 1u
const char *vsg_shard_last_error(void);
size_t vsg_shard_record_bytes(int capacity);
size_t vsg_shard_record_desc_offset(int capacity);
int vsg_shard_frame_owner(int frame, int world);
int vsg_shard_stream_owner(int stream, int n_streams, int world, int frame);
int vsg_shard_unique_id(uint8_t id[128]);
int vsg_shard_create(int device, int rank, int world, const uint8_t id[128], int capacity, int frames_per_rank,
                     vsg_shard **out);
void vsg_shard_destroy(vsg_shard *s);
int vsg_shard_all_gather(vsg_shard *s, const int *d_counts, const vsg_keypoint *d_kps, const uint8_t *d_desc,
                         int src_capacity, int nframes, void *stream);
int vsg_shard_record(vsg_shard *s, int rank, int frame, const int **d_counts, const vsg_keypoint **d_kps,
                     const uint8_t **d_desc);
/* Size of the communicator and this process's rank in it AS RCCL REPORTS THEM (ncclCommCount / ncclCommUserRank on the
 * live communicator -- not an echo of what vsg_shard_create was given); VSG_ERR_UNSUPPORTED if the loaded RCCL lacks them. */
int vsg_shard_world(const vsg_shard *s);
int vsg_shard_rank(const vsg_shard *s);
/* Neighbour-only exchange for chunk-partitioned sequences (rank r owns frames [r B, (r + 1) B) of a step): matching
 * needs ONE remote record per rank and step, the predecessor rank's last frame.  Packs frame `frame` of this rank's
 * batch and sends it to rank + 1 while receiving the record of rank - 1 (cyclic): one ncclSend / ncclRecv pair on the
 * caller's stream instead of an all-gather of every record.  vsg_shard_boundary_record: device pointers of the
 * received record (valid until the next exchange). */
int vsg_shard_send_recv_boundary(vsg_shard *s, const int *d_counts, const vsg_keypoint *d_kps, const uint8_t *d_desc,
                                 int src_capacity, int frame, void *stream);
int vsg_shard_boundary_record(vsg_shard *s, const int **d_counts, const vsg_keypoint **d_kps, const uint8_t **d_desc);

/* The visual part of void Optimizer::LocalBundleAdjustment(pKF, pbStopFlag, pMap, ...) (Optimizer.cc:1454-2454) on
 * resident keyframes and resident map points: the keyframe vertices (:1762-1793), the point vertices and their monocular
 * and stereo edges (:1850-1948), optimize(iterations) (:2288), the classification (:2296-2340) and the recovery
 * (:2398-2414), in double, with the arithmetic of csrc/vsg_local_ba.h, which a host build reproduces bit for bit (DESIGN.md
 * section 8).  The marker, plane, room and door vertices and their edges (:1995-2274, :2342-2369, :2416-2452) are NOT
 * part of it: a caller whose local lists of planes and rooms are not empty calls
 * vsg_mappoints_local_bundle_adjustment_sgraph below instead.
 *   - Point i = slot slots[i] of mp, with the observations [obs_off[i], obs_off[i + 1]) of obs_kf (index into kfs) and
 *     obs_idx (leftIndex in that keyframe), as vsg_mappoints_refresh_from_observations takes them: the observations that
 *     pass !pKFi->isBad() && GetMap() == pCurrentMap (:1881), in mObservations' order.  The edges are these entries in this
 *     order (g2o's insertion order); edge e is stereo when that keyframe's u_right[idx] >= 0 (:1886, :1913), else mono.
 *   - kfs = the local keyframes AND the fixed ones, resident with mvKeysUn and mvuRight, in ascending mnId; kf_Tcw[k] =
 *     GetPose(); kf_fixed[k] != 0 for lFixedCameras and for the map's initial keyframe (:1772, :1789); kf_cam[k] = that
 *     keyframe's fx, fy, cx, cy, mbf.  inv_level_sigma2 = mvInvLevelSigma2, nlevels entries.  iterations = 10 at :2288.
 *   - stop_flag (may be NULL) = pbStopFlag: read before optimising (:2283) and each time the host looks at the solver's
 *     state between iterations; a set flag then ends the run with stop_reason 3.  The kernels never read it.
 *   - kf_Tcw_out[k]: an optimised keyframe with at least one edge gets vSE3->estimate(); every other keyframe (fixed, or
 *     without an edge: g2o drops such a vertex) gets its input, widened.  world_pos_out[3 i] (may be NULL) = the float
 *     position of point i, ALSO written into the slot's world_pos on the device (SetWorldPos, :2412); a point with an
 *     empty list is no vertex: its slot keeps its bytes and its out is what the slot holds.  The other fields of the slots
 *     are untouched: follow with vsg_mappoints_refresh_from_observations(VSG_REFRESH_NORMAL) (:2413).
 *   - erase[e] = whether (keyframe, point) of observation e goes into vToErase; chi2[e] (may be NULL) = the double
 *     compared, NaN canonical: e->chi2() as the LAST computeActiveErrors left it (after a rejected last trial that is the
 *     rejected state's), compared with > 5.991 / > 7.815; isDepthPositive() on the restored estimates.
 *   - res->ran = 0: the reference returned before optimize -- no fixed keyframe (:1734), no edge (:2277), the stop flag
 *     (:2283) -- or n_points == 0; nothing is enqueued and no out but res is written.  stop_reason: 0 = the iterations
 *     are done, 1 = Terminate (qmax == 10 || rho == 0), 2 = _nBad >= 3, 3 = the stop flag.
 * Checked before anything is enqueued (an error writes nothing and leaves no kernel behind), VSG_ERR_INVALID: a NULL mp,
 * slots, obs_off, kfs, a keyframe, kf_Tcw, kf_fixed, kf_cam, inv_level_sigma2, kf_Tcw_out, erase or res; obs_kf / obs_idx
 * NULL with observations; offsets that do not ascend from 0; an observation outside [0, n_kf) x [0, N of that keyframe); a
 * slot outside [0, capacity) or listed twice; nlevels outside [1, 16]; an observed keypoint's octave >= nlevels;
 * iterations outside [1, 100]; a keyframe on another device than the store.  VSG_ERR_UNSUPPORTED: a keyframe with
 * Nleft != -1 (EdgeSE3ProjectXYZToBody, KannalaBrandt8: :1950-1989), edges but no optimised keyframe with one, more than
 * 128 optimised keyframes with edges (the reduced system's one code path holds 768 rows).
 * The scratch lives in the calling thread's arena: two threads may solve on the same store at the same time ONLY when
 * their point sets are disjoint (each writes its points' world_pos).  The call waits for its stream before it returns,
 * on an error too. */
typedef struct vsg_pose_se3d { double q[4], t[3]; } vsg_pose_se3d;
typedef struct vsg_ba_camera { float fx, fy, cx, cy, bf; } vsg_ba_camera;
typedef struct vsg_local_ba_result {
  int32_t ran;              /* 0: returned before optimize (:1734 no fixed keyframe, :2277 no edge, :2283 stop flag) */
  int32_t n_opt_kf, n_fixed_kf, n_points, n_edges, n_mono, n_stereo, n_erase;
  int32_t iterations_run, trials_run, stop_reason;   /* iterations done | Terminate | nBad >= 3 */
  double lambda, chi2_initial, chi2_final;
} vsg_local_ba_result;
int vsg_mappoints_local_bundle_adjustment(
    vsg_mappoints *mp, int n_points, const int32_t *slots,
    const int32_t *obs_off, const int32_t *obs_kf, const int32_t *obs_idx,   /* as vsg_mappoints_refresh_from_observations */
    int n_kf, vsg_frame *const *kfs, const vsg_pose_se3 *kf_Tcw, const uint8_t *kf_fixed, const vsg_ba_camera *kf_cam,
    const float *inv_level_sigma2, int nlevels, int iterations, const volatile uint8_t *stop_flag,
    vsg_pose_se3d *kf_Tcw_out, float *world_pos_out, uint8_t *erase, double *chi2, vsg_local_ba_result *res);

/* Optimizer::LocalBundleAdjustment WITH its planes and rooms: the visual part above, and behind it the plane vertices with
 * their keyframe edges (Optimizer.cc:2018-2130), the room vertices with their wall edges (:2155-2214), their classification
 * (:2342-2369) and recovery (:2426-2441), with the arithmetic of csrc/vsg_sgraph_ba.h, which a host build reproduces bit
 * for bit (DESIGN.md sections 7 and 8).  The planes and rooms are rows of the reduced system behind the keyframes; the
 * Jacobians of their edges are g2o's numeric ones.  The arguments up to chi2 are the visual call's; then:
 *   - plane_eq[4 i] = localPlaneList's getGlobalEquation().coeffs(), taken as held (setEstimate does not renormalise).
 *     Plane i has the observations [pl_obs_off[i], pl_obs_off[i + 1]) of pl_obs_kf (index into kfs): the entries of
 *     getObservations() that pass :2070-2083, in the map's order.  Per observation: pl_obs_local[4] = obs.localPlane's
 *     coefficients, pl_obs_G[16] = obs.Gij row-major, w_plane_kf = obs.confidence * plane_kf.information_gain or 0 when
 *     that edge is not added (plane_kf disabled), w_plane_point = obs.confidence * plane_point.information_gain or 0 when
 *     not added (plane_point disabled, or getClassIdFromPlaneType == -1).
 *   - the rooms that get a vertex (walls.size() >= 2, :2163): room_center[3 r] = getRoomCenter(), room_n_walls[r] = 2
 *     (getIsCorridor()) or 4, room_wall[4 r + k] = wall k as an index into the planes.  The reference's :2198 tests walls[2]
 *     twice and would dereference a missing walls[3]; here all four must exist.
 *   - plane_eq_out[4 i] = vPlane->estimate() (:2431); a plane without an edge gets its input bytes (g2o drops the vertex).
 *     room_center_out[3 r] = the room vertex's translation (:2441).  erase_plane[o] = whether (keyframe, plane) of
 *     observation o goes into vToErasePlane: chi2 > 7.815 of its plane-keyframe edge, chi2 > 3.841 of its point-to-plane
 *     edge, or !isDistanceCorrect() of either on the restored estimates; the std::find of :2352 / :2366 is this one flag.
 *     chi2_plane_kf[o] / chi2_plane_point[o] (may be NULL) = the doubles compared, NaN canonical, NaN where the edge does
 *     not exist.  A keyframe whose only edges are plane edges is optimised too.
 *   - res->local is the visual call's result; n_edges counts the visual edges.  ran = 0 as there, where "no edge" (:2277)
 *     counts the visual and the plane edges but NOT the room edges: the reference never increments nEdges for them.
 *   - the edge order of every sum: the visual edges, then per plane and observation the plane-keyframe edge before the
 *     point-to-plane edge, then the rooms.  With n_planes == 0 and n_rooms == 0 every out the two calls share is
 *     byte-equal to vsg_mappoints_local_bundle_adjustment's.
 * NOT part of it (the caller keeps the reference routine): marginalize_planes = true and the plane_map_point factor
 * (:2026, :2037); the plane / room section of Optimizer::BundleAdjustment (:289-498).  Markers have no edge in this version
 * of the reference (g2o drops them, their recovery returns the input) and doors are commented out: neither is an argument.
 * Checked before anything is enqueued, VSG_ERR_INVALID: everything the visual call lists; a NULL new array with a non-zero
 * count (plane_eq_out, room_center_out, erase_plane among them); plane offsets that do not ascend from 0; an observation
 * keyframe outside [0, n_kf) or listed twice for one plane; a negative or NaN weight; a non-finite plane or one with a zero
 * normal; room_n_walls outside {2, 4}; a wall outside [0, n_planes) or listed twice in a room.  VSG_ERR_UNSUPPORTED: what
 * the visual call lists, and 6 optimised keyframes + 3 planes with an edge + 6 rooms > 768 rows. */
typedef struct vsg_sgraph_local_ba_result {
  vsg_local_ba_result local;
  int32_t n_planes_active, n_rooms_active;          /* vertices with an edge */
  int32_t n_plane_kf, n_plane_point, n_room_edges;  /* edges of each kind */
  int32_t n_rows, n_erase_plane, reserved;          /* rows of the reduced system; erase_plane flags set */
} vsg_sgraph_local_ba_result;
int vsg_mappoints_local_bundle_adjustment_sgraph(
    vsg_mappoints *mp, int n_points, const int32_t *slots,
    const int32_t *obs_off, const int32_t *obs_kf, const int32_t *obs_idx,
    int n_kf, vsg_frame *const *kfs, const vsg_pose_se3 *kf_Tcw, const uint8_t *kf_fixed, const vsg_ba_camera *kf_cam,
    const float *inv_level_sigma2, int nlevels, int iterations, const volatile uint8_t *stop_flag,
    vsg_pose_se3d *kf_Tcw_out, float *world_pos_out, uint8_t *erase, double *chi2,
    int n_planes, const double *plane_eq, const int32_t *pl_obs_off, const int32_t *pl_obs_kf, const double *pl_obs_local,
    const double *pl_obs_G, const double *w_plane_kf, const double *w_plane_point,
    int n_rooms, const double *room_center, const int32_t *room_n_walls, const int32_t *room_wall,
    double *plane_eq_out, double *room_center_out, uint8_t *erase_plane, double *chi2_plane_kf, double *chi2_plane_point,
    vsg_sgraph_local_ba_result *res);

/* The visual part of void Optimizer::BundleAdjustment(vpKFs, vpMP, ..., nIterations, pbStopFlag, nLoopKF, bRobust, ...)
 * (Optimizer.cc:60-287, :500-610) as Optimizer::GlobalBundleAdjustemnt calls it (:45-58) on resident keyframes and resident
 * map points: from Tracking::CreateInitialMapMonocular (Tracking.cc:2652: 20 iterations, bRobust = true, nLoopKF = 0) and from
 * LoopClosing::RunGlobalBundleAdjustment (LoopClosing.cc:2157: 10 iterations, bRobust = false).  The keyframe vertices
 * (:117-130), the point vertices with their monocular and stereo edges (:143-287), optimize(nIterations) and the write-back
 * (:500-610), in double, with the arithmetic of csrc/vsg_local_ba.h and csrc/vsg_global_ba.h, which a host build reproduces
 * bit for bit.  The marker, plane, room and door vertices and their edges (:289-498, :612-640) are NOT
 * part of it: a caller whose lists of those are not empty keeps the reference routine; at the monocular
 * initialisation they are always empty.  The arguments are those of vsg_mappoints_local_bundle_adjustment except:
 *   - kfs = EVERY keyframe of the map with !isBad() (:120), in ascending mnId; kf_fixed[k] != 0 for mnId ==
 *     pMap->GetInitKFid() (:126).  No fixed keyframe is NO reason to return: the reference has no such check here.
 *   - the lists hold the observations that pass :166-169, in mObservations' order; edge e is stereo when that keyframe's
 *     u_right[idx] >= 0 (:204), else mono (:174).
 *   - robust (:189, :221): 1 = RobustKernelHuber with the float deltas sqrt(5.99) / sqrt(7.815) of :133-134 (5.99, not the
 *     5.991 of the local call); 0 = no kernel, rho = chi2 and weight 1.  iterations = nIterations, within [1, 100].
 *   - nothing is classified: there is no erase out, and no recovery beyond g2o's own pop.  The counts of :529-584 are read
 *     by nothing and are left out.  chi2[e] (may be NULL) = e->chi2() as the LAST computeActiveErrors left it, NaN canonical.
 *   - write_store (:516, :600): 1 = the case nLoopKF == pMap->GetOriginKF()->mnId: the float position of every included
 *     point is written into its slot's world_pos (SetWorldPos); follow with
 *     vsg_mappoints_refresh_from_observations(VSG_REFRESH_NORMAL) (UpdateNormalAndDepth).  0 = the store's bytes are
 *     untouched and the positions come back in world_pos_out alone (mPosGBA, mnBAGlobalForKF stay with the caller), which
 *     must then be non-NULL.
 *   - kf_Tcw_out[k]: an optimised keyframe with at least one edge gets vSE3->estimate(), every other keyframe its input,
 *     widened; the float casts of :518 / :522 stay with the caller.  included[i] = 0 for a point with an empty list
 *     (vbNotIncludedMP, :278-286): its out is what its slot holds and the slot is not written.
 *   - res->ran = 0: no edge, the stop flag set on entry, or n_points == 0: nothing is enqueued and only res and included
 *     are written.  stop_reason as in the local call.
 * Checked before anything is enqueued (an error writes nothing and leaves no kernel behind; so does a failed reservation of
 * the arenas: included, the first out written, is filled behind it.  Only VSG_ERR_HIP from a launch or the stream's wait can
 * leave included written), VSG_ERR_INVALID: everything the
 * local call lists (with included in the place of erase), and: robust or write_store outside {0, 1}; write_store == 0 with
 * a NULL world_pos_out; a NULL included.  VSG_ERR_UNSUPPORTED: a keyframe with Nleft != -1 (EdgeSE3ProjectXYZToBody, :241-275),
 * edges but no optimised keyframe with one, more than 512 optimised keyframes with edges.  At that cap the reduced system has
 * 3072 rows and is a matrix of 75.5 MB; with the lists and the per-edge blocks of a map of 60000 points and 500000
 * observations (664 bytes of blocks per observation) the calling thread's device arena then holds about 450 MB.
 * The reduced system is solved by a chain of kernels over the whole chip whatever its size.  Two threads
 * may solve on the same store at the same time ONLY when their point sets are disjoint.  The call waits for its stream
 * before it returns, on an error too. */
typedef struct vsg_global_ba_result {
  int32_t ran;              /* 0: returned before optimize (no edge, the stop flag, no point) */
  int32_t n_opt_kf, n_fixed_kf, n_points, n_edges, n_mono, n_stereo;
  int32_t iterations_run, trials_run, stop_reason;   /* iterations done | Terminate | nBad >= 3 | the stop flag */
  double lambda, chi2_initial, chi2_final;
} vsg_global_ba_result;
int vsg_mappoints_global_bundle_adjustment(
    vsg_mappoints *mp, int n_points, const int32_t *slots,
    const int32_t *obs_off, const int32_t *obs_kf, const int32_t *obs_idx,
    int n_kf, vsg_frame *const *kfs, const vsg_pose_se3 *kf_Tcw, const uint8_t *kf_fixed, const vsg_ba_camera *kf_cam,
    const float *inv_level_sigma2, int nlevels, int iterations, int robust, int write_store,
    const volatile uint8_t *stop_flag,
    vsg_pose_se3d *kf_Tcw_out, float *world_pos_out, uint8_t *included, double *chi2, vsg_global_ba_result *res);

/* void Optimizer::OptimizeEssentialGraph(pMap, pLoopKF, pCurKF, NonCorrectedSim3, CorrectedSim3, LoopConnections, bFixScale)
 * (Optimizer.cc:2456-2734, the first overload; LoopClosing::CorrectLoop, LoopClosing.cc:1150) on resident map points: the
 * Sim3 vertices (:2490-2525), the EdgeSim3 edges with the 7 x 7 identity as information, g2o's Levenberg loop with
 * setUserLambdaInit(1e-16) and optimize(iterations) (:2469, :2684), and the correction of every listed map point through
 * its reference keyframe (:2704-2731), in double, with the arithmetic of csrc/vsg_essential_graph.h, which a host build
 * reproduces bit for bit.  The merge overload (:2736 ff.), OptimizeEssentialGraph4DoF and the inertial
 * edges (:2662-2679) are NOT part of it: a caller with bImu keyframes keeps the reference routine.
 *   - kf_Scw[k] = vScw of keyframe k (:2502-2511): CorrectedSim3's entry where the keyframe has one, else (GetPose(), 1.0);
 *     the keyframes are those with !isBad() in ascending mnId.  kf_has_non_corrected[k] != 0: kf_non_corrected[k] is the
 *     keyframe's entry of NonCorrectedSim3.  kf_fixed[k] != 0 for mnId == pMap->GetInitKFid() (:2514).
 *   - edge e joins vertex 0 = edge_i[e] and vertex 1 = edge_j[e] (setVertex(0, nIDi), setVertex(1, nIDj)), in g2o's
 *     insertion order; vsg::essential_graph_edges (vsg_orb_adaptor.hpp) builds the list with the reference's filters.
 *     edge_loop[e] != 0: a "Set Loop edges" edge (:2529-2560), both sides of Sji = Sjw * Swi from vScw; 0: a "Set normal
 *     edges" edge (:2563-2660), each side from NonCorrectedSim3 where the keyframe has an entry, else from vScw.  Two edges
 *     between one pair of keyframes are legal and both count.
 *   - fix_scale = bFixScale (VertexSim3Expmap::_fix_scale); iterations = 20 at :2684, within [1, 100].
 *   - slots[i] = the store slot of map point i, point_ref[i] = nIDr of :2712-2721 as an index into the keyframes.  Each
 *     listed slot's world_pos becomes float(correctedSwr.map(Srw.map(double(pos)))) (:2723-2728), also written to
 *     world_pos_out[3 i ..] when that is not NULL; no other slot is touched.  mp may be NULL when n_points == 0: the pose
 *     graph alone, on the calling thread's current device.  Follow with
 *     vsg_mappoints_refresh_from_observations(VSG_REFRESH_NORMAL) for UpdateNormalAndDepth (:2730).
 *   - kf_Scw_out[k] = VSim3->estimate() (:2696): a keyframe that is not fixed and has at least one edge gets its optimised
 *     estimate, NaN canonical, every other keyframe its input's bytes (g2o drops a vertex without an edge).  The SE3 recovery
 *     of :2700 (t / s, the float casts) stays with the caller.  chi2[e] (may be NULL) = the edge's chi2() after the
 *     computeActiveErrors of :2685.
 *   - res->ran = 0: no edge, or no edge at a keyframe that is not fixed: nothing is enqueued, kf_Scw_out holds the inputs,
 *     and the store, world_pos_out and chi2 are untouched (the reference maps every point through Srw and its own inverse
 *     there: a rounding of the float position at most).  stop_reason: 0 the iterations are done, 1 Terminate (ten rejected
 *     trials, or rho == 0), 2 _nBad >= 3; there is no stop flag in this routine.
 * Checked before anything is enqueued (an error writes nothing and leaves no kernel behind), VSG_ERR_INVALID: a negative
 * count; a NULL kf_Scw_out or res; with n_kf > 0 a NULL kf_Scw, kf_has_non_corrected or kf_fixed, or a NULL
 * kf_non_corrected with an entry flagged; with n_edges > 0 a NULL edge_i, edge_j or edge_loop; with n_points > 0 a NULL mp,
 * slots or point_ref; fix_scale outside {0, 1}; iterations outside [1, 100]; an edge index outside [0, n_kf), or
 * edge_i[e] == edge_j[e]; a slot outside [0, capacity), or listed twice; a point_ref outside [0, n_kf); an input Sim3 (an
 * entry of kf_Scw, or a flagged entry of kf_non_corrected) that is not finite or whose scale is <= 0.  VSG_ERR_UNSUPPORTED:
 * more than 438 keyframes that are not fixed and have an edge.  THE CAP: g2o solves this system sparsely; here it is a dense
 * LDL^T of 7 rows per such keyframe through the chain of kernels the global BA's reduced solve uses, tested up to 3072
 * rows (7 x 438 = 3066, a matrix of 75 MB in the calling thread's device arena).  Real maps exceed that: their callers keep
 * the reference routine until a sparse solve exists.  The call waits for its stream before it
 * returns, on an error too. */
typedef struct vsg_essential_graph_result {
  int32_t ran;              /* 0: nothing to optimise */
  int32_t n_opt_kf, n_fixed_kf, n_kf, n_edges, n_points;
  int32_t iterations_run, trials_run, stop_reason;
  int32_t pad;
  double lambda, chi2_initial, chi2_final;
} vsg_essential_graph_result;
int vsg_mappoints_optimize_essential_graph(
    vsg_mappoints *mp,
    int n_kf, const vsg_sim3d *kf_Scw,
    const vsg_sim3d *kf_non_corrected, const uint8_t *kf_has_non_corrected, const uint8_t *kf_fixed,
    int n_edges, const int32_t *edge_i, const int32_t *edge_j, const uint8_t *edge_loop,
    int fix_scale, int iterations,
    int n_points, const int32_t *slots, const int32_t *point_ref,
    vsg_sim3d *kf_Scw_out, float *world_pos_out, double *chi2,
    vsg_essential_graph_result *res);

/* The point correction of LoopClosing::CorrectLoop (LoopClosing.cc:1060-1064: eigCorrectedP3Dw =
 * g2oCorrectedSwi.map(g2oSiw.map(P3Dw))) and of Optimizer::OptimizeEssentialGraph (Optimizer.cc:2723-2728) on resident map
 * points: one kernel, two callers.  The world_pos of slot slots[i] becomes float(S_to_inverse[r].map(S_from[r].map(
 * double(pos)))) with r = point_ref[i], also written to world_pos_out[3 i ..] when that is not NULL; no other slot is
 * touched.  In CorrectLoop S_from[r] = g2oSiw of connected keyframe r (NonCorrectedSim3) and S_to_inverse[r] =
 * g2oCorrectedSiw.inverse(); mnCorrectedByKF / mnCorrectedReference stay with the caller.  Follow with
 * vsg_mappoints_refresh_from_observations(VSG_REFRESH_NORMAL) (UpdateNormalAndDepth, :1067).  n_points == 0 returns VSG_OK
 * and enqueues nothing.  Checked before anything is enqueued (an error writes nothing), VSG_ERR_INVALID: a NULL mp; a negative
 * count; with n_points > 0 a NULL slots, point_ref, S_from or S_to_inverse; a slot outside [0, capacity), or listed twice;
 * a point_ref outside [0, n_ref); an entry of S_from or S_to_inverse that is not finite or whose scale is <= 0. */
int vsg_mappoints_correct_sim3(
    vsg_mappoints *mp, int n_points, const int32_t *slots, const int32_t *point_ref,
    int n_ref, const vsg_sim3d *S_from, const vsg_sim3d *S_to_inverse, float *world_pos_out);

/* bool TwoViewReconstruction::Reconstruct(vKeys1, vKeys2, vMatches12, T21, vP3D, vbTriangulated)
 * (TwoViewReconstruction.cc:40-129; Tracking::MonocularInitialization, Tracking.cc:2568, through
 * Pinhole::ReconstructWithTwoViews, Pinhole.cpp:91-101): the monocular initialisation behind
 * vsg_frame_search_for_initialization.  Hypothesis `it` of either model depends on mvSets[it] alone, each loop keeps the
 * first `it` whose score is strictly greater than every earlier one (:172, :222), the two model searches are independent
 * (:104-109) and so are the 4 (F) or 8 (H) motion hypotheses of CheckRT: all of it runs in ONE enqueue and ONE wait.
 *   f1 / f2 = the reference and the current frame, resident with mvKeysUn; matches12[i] (f1's N entries) = vMatches12, -1
 * or a feature of f2; K = mK row-major; sets = mvSets, n_iter rows of 8 indices into the COMPACTED matches (:51-63: the
 * entries >= 0 in ascending i; vsg_two_view_draw_sets draws them as :82-97); n_iter = mMaxIterations (200).  params: sigma
 * = mSigma; rh_threshold = the 0.50 of :119, min_parallax and min_triangulated = the 1.0 and 50 of :116-127.
 *   res: ok = the return value; reason = 0 success, 1 SH + SF == 0 (:112), 2 the singular-value gate of ReconstructH (:598),
 * 3 no clear winner or too few points (:518, :724), 4 the parallax gate; model = 0 H / 1 F; SH, SF, best_it_h / best_it_f
 * (-1: no hypothesis scored above 0; the matrix is then zeros) and H21 / F21 (row-major) = what the two searches return;
 * R21 (row-major) / t21 = T21 (zeros unless ok); n_good[k] = nGood of motion hypothesis k in the order of :498-501 / :702
 * (4 or 8 entries, the rest 0); parallax = that of the chosen hypothesis (0 where the routine returned before it);
 * n_inliers = N of :476 / :575.
 *   triangulated[i] (f1's N entries) = vbTriangulated and x3d[3 i] = vP3D are written ONLY when ok, and x3d ONLY on the F
 * path: ReconstructH never assigns vP3D (:724-730), so after an H success the caller's x3d holds what it held before --
 * kept as the reference has it.  Both are then written whole (zero where CheckRT wrote nothing).  A point with
 * cosParallax >= 0.99998 has its position written but is not flagged (:879-884).  inlier_h / inlier_f (one byte per
 * COMPACTED match) and score_h / score_f (n_iter floats) may each be NULL: vbMatchesInliersH / F of the two winners and
 * every hypothesis's score.
 *   Arithmetic (csrc/vsg_two_view.h, host and device from one source): float in the reference's order,
 * the scores summed in float in the reference's order; every singular vector comes from a double one-sided Jacobi rounded
 * once instead of Eigen's float JacobiSVD, a deviation by rounding -- the sign of a singular pair only permutes the motion
 * hypotheses (n_good's order).  Triangulate's x3Dh(3) == 0, where the reference reads an unset vector, counts as not
 * finite.  acos runs on the host behind the wait.  NaNs in the outputs are canonical.
 *   Checked before anything is enqueued (an error writes nothing and leaves no kernel behind), VSG_ERR_INVALID: a NULL
 * frame, matches12, K, params, sets, res, triangulated or x3d; frames on different devices; a match outside [-1, N of f2);
 * fewer than 8 matches (the reference would index an empty vector); n_iter outside [1, 1024]; a set entry outside [0,
 * matches); two equal entries in one set; sigma or a K entry not finite; sigma <= 0.  Only the matches, the sets and a
 * few scalars go up; the scratch lives in the calling thread's arena, so two threads may initialise on the same frames
 * at the same time. */
#define VSG_TWO_VIEW_H 0
#define VSG_TWO_VIEW_F 1
typedef struct vsg_two_view_params {
  float sigma, rh_threshold, min_parallax;
  int32_t min_triangulated;
} vsg_two_view_params;
typedef struct vsg_two_view_result {
  int32_t ok, reason, model;
  float SH, SF;
  int32_t best_it_h, best_it_f;
  float H21[9], F21[9], R21[9], t21[3];
  int32_t n_good[8];
  float parallax;
  int32_t n_inliers;
} vsg_two_view_result;
/* sigma 1.0, rh_threshold 0.50, min_parallax 1.0, min_triangulated 50 (Pinhole.cpp:97, TwoViewReconstruction.cc:116-127) */
void vsg_two_view_default_params(vsg_two_view_params *params);
int vsg_frame_two_view_reconstruct(vsg_frame *f1, vsg_frame *f2, const int32_t *matches12, const float K[9],
                                   const vsg_two_view_params *params, int n_iter, const int32_t *sets,
                                   vsg_two_view_result *res, uint8_t *triangulated, float *x3d, uint8_t *inlier_h,
                                   uint8_t *inlier_f, float *score_h, float *score_f);
/* The same on keypoints the caller holds: xy1 / xy2 = {x, y} of the n1 / n2 undistorted keypoints of the two frames --
 * what KannalaBrandt8::ReconstructWithTwoViews (KannalaBrandt8.cpp:181-211) has after it undistorted on its own.  One
 * implementation behind both forms; here the matched coordinates go up as well.  Also refused: a NULL xy1 / xy2, n1 or n2
 * below 1. */
int vsg_two_view_reconstruct(int device, const float *xy1, int n1, const float *xy2, int n2, const int32_t *matches12,
                             const float K[9], const vsg_two_view_params *params, int n_iter, const int32_t *sets,
                             vsg_two_view_result *res, uint8_t *triangulated, float *x3d, uint8_t *inlier_h,
                             uint8_t *inlier_f, float *score_h, float *score_f);
/* The draw of :82-97 for n_iter sets over n matches: per set a copy of vAllIndices (0 .. n-1), then eight times randi =
 * random_int(0, size - 1, ctx), the element is taken, back() moves into its place, pop_back().  random_int == NULL:
 * DUtils::Random::RandomInt's formula over rand() (Random.cpp:47-50); SeedRandOnce(0) (:80) stays with the caller.  Host
 * only.  n < 8, n_iter < 0, NULL sets, or a random_int result outside its range: VSG_ERR_INVALID. */
int vsg_two_view_draw_sets(int n, int n_iter, int (*random_int)(int lo, int hi, void *ctx), void *ctx, int32_t *sets);

/* MLPnPsolver (MLPnPsolver.cpp; constructed at Tracking.cc:3735, iterated at :3762) on a resident frame and resident map
 * points: one call of iterate(n_iterations, ...) entered at mnIterations == first, EVERY hypothesis side by side.
 * Hypothesis k depends on its six sampled correspondences alone, and what iterate returns is a selection over the
 * hypotheses' inlier counts c[k].  Refine() (:303-362) solves over the best set into a local variable and never installs
 * that pose: its CheckInliers counts hypothesis k's inliers again, so it succeeds iff c[k] > min_inliers and hands back
 * hypothesis k's pose and flags; the solve changes nothing a caller can see and is not run here.  The loop (:120) walks
 * k = first .. end - 1 with end = max(max_its, first + n_iterations): a k with c[k] >= min_inliers replaces the best on a
 * strict maximum, and when c[k] > min_inliers the call returns hypothesis k (found = 1, refined = 1, no_more = 0,
 * iterations = k + 1; the best may be an earlier hypothesis of a call before); past the loop, iterations >= max_its gives
 * no_more = 1 and the best hypothesis when there is one (refined = 0).  The state between the reference's
 * calls is (mnIterations, best), both functions of the sets and of first: a resumed call is this call with
 * first = res->iterations of the call before, and the library keeps nothing.
 *   slots[i] (one per feature of f) = the slot of vpMapPointMatches[i] in mp, < 0 for none or a bad one; correspondence
 * index = rank among the entries >= 0.  fx, fy, cx, cy = the Pinhole parameters; level_sigma2 = mvLevelSigma2 (nlevels
 * entries); th2 as SetRansacParameters takes it; min_inliers / max_its = mRansacMinInliers / mRansacMaxIts AFTER
 * SetRansacParameters (vsg_mlpnp_ransac_parameters); sets[6 k .. 6 k + 5] = the six correspondence indices of hypothesis k
 * in drawing order (vsg_mlpnp_draw_sets).
 *   Outputs: inlier[i] (one per feature) = vbInliers; res as below; hyp_inliers[k] / hyp_T[12 k ..] (either may be NULL) =
 * mnInliersi and [R | t] (3 x 4, row-major, double) of every hypothesis.  n < min_inliers (:111): no_more = 1, found = 0,
 * the identity, flags cleared, nothing is enqueued.
 *   Arithmetic (csrc/vsg_mlpnp.h, host and device from one source): double where the reference is,
 * CheckInliers in its mixed double / float order with no positive-depth test; the nullspace of a bearing comes from a
 * Householder reflection, the null vector of A^T A and the nearest rotation from a one-sided Jacobi, the 6 x 6 solve is
 * an LDL^T without pivoting, acos / cbrt / sin / cos are written out -- deviations by rounding; the Jacobian is analytic
 * and takes its limit at w = 0.  NaNs in res and hyp_T are canonical.
 *   Checked before anything is enqueued (an error writes nothing and leaves no kernel behind), VSG_ERR_INVALID: a NULL
 * handle, slots, level_sigma2, sets, inlier or res; frame and store on different devices; a slot >= capacity; nlevels
 * outside [1, 16]; an octave of a used feature outside [0, nlevels); th2 not finite or <= 0; min_inliers < 6; max_its < 1;
 * first < 0; n_iterations < 0; n_hyp outside [1, 1024]; max(max_its, first + n_iterations) > n_hyp; and when
 * n >= min_inliers: a sample outside [0, n), two equal samples in one set.  Nleft != -1 (a KannalaBrandt8 pair):
 * VSG_ERR_UNSUPPORTED, as in vsg_frame_pose_optimization.  One enqueue (three kernels) on the calling thread's stream and
 * one wait; only the slots, the sets and a few scalars cross to the device. */
typedef struct vsg_mlpnp_result {
  float Tcw[16];           /* Tout, row-major */
  int32_t found, no_more;  /* iterate's return value, bNoMore */
  int32_t n_inliers;       /* nInliers */
  int32_t refined;         /* 1 = returned through Refine(): hypothesis iterations - 1; 0 = the best at the loop's end (or nothing) */
  int32_t best_hypothesis; /* b, or -1 */
  int32_t iterations;      /* mnIterations on return */
  int32_t n_correspondences; /* N */
  int32_t n_records;         /* how often the best set was replaced up to the return, calls before included */
} vsg_mlpnp_result;
int vsg_frame_mlpnp_ransac(vsg_frame *f, vsg_mappoints *mp, const int32_t *slots, float fx, float fy, float cx, float cy,
                           const float *level_sigma2, int nlevels, float th2, int min_inliers, int max_its, int first,
                           int n_iterations, int n_hyp, const int32_t *sets, uint8_t *inlier, vsg_mlpnp_result *res,
                           int32_t *hyp_inliers, double *hyp_T);
/* MLPnPsolver::SetRansacParameters (:231-267) for n correspondences: the float N * epsilon truncated, the raise to
 * min_inliers and min_set, the epsilon raise, ceil(log(1 - p) / log(1 - pow(epsilon, 3))) -- the exponent is 3 although
 * the minimal set is 6 -- and max(1, min(nIterations, max_iterations)).  Host only.  n < 0, a NULL output: VSG_ERR_INVALID. */
int vsg_mlpnp_ransac_parameters(double probability, int min_inliers, int max_iterations, int min_set, float epsilon, int n,
                                int *min_inliers_out, int *max_its_out);
/* The draw of :125-145 for n_hyp hypotheses over n correspondences, six per hypothesis, with the semantics of
 * vsg_sim3_draw_samples.  Host only.  n < 6, n_hyp < 0, NULL sets, or a random_int result outside its range:
 * VSG_ERR_INVALID. */
int vsg_mlpnp_draw_sets(int n, int n_hyp, int (*random_int)(int lo, int hi, void *ctx), void *ctx, int32_t *sets);

#ifdef __cplusplus
}
#endif
#endif /* VSG_ORB_H */
