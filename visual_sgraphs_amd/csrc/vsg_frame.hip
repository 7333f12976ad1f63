// vsg_frame.hip -- building a device-resident Frame / KeyFrame feature set (the searches on it: vsg_window.hip).
//
//   Frame::AssignFeaturesToGrid / PosInGrid                          orb_slam3/src/Frame.cc:521-553, 870-880
//   Frame::UndistortKeyPoints / ComputeImageBounds                   orb_slam3/src/Frame.cc:891-921, 924-955
//   Frame::ComputeStereoFromRGBD                                     orb_slam3/src/Frame.cc:1129-1150
//
// A frame becomes resident by an upload of host arrays (the grid is built on the host, one DMA) or straight out of the
// extractor: k_frame_grid_build copies the records, undistorts them, samples an RGB-D depth plane and builds the CSR
// grid in ONE launch, which can ride behind the extractor's own chain (vsg_orb_extract_to_frame).  The stand-alone
// Frame grid (vsg_grid_build / vsg_grid_destroy) is a frame block with the left grid alone, filled by
// the upload path (host_grid is the one host build of the CSR).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "vsg_frame_int.h"
#include "vsg_math.h"
#include "vsg_undistort.h"

using namespace vsg;

namespace {

// ---- Tracking::GrabImageRGBD's depth conversion (Tracking.cc:1610-1611) + Frame::ComputeStereoFromRGBD (Frame.cc:1129-1150)
// A depth plane as the device reads it.  base == nullptr: no RGB-D step.
struct DepthPlane {
  const uint8_t *base;
  size_t stride;        // bytes per row
  int type, rows, cols;  // VSG_DEPTH_U16 / VSG_DEPTH_F32
  int convert;          // fabs(mDepthMapFactor - 1.0f) > 1e-5 || type != CV_32F: convertTo(CV_32F, scale)
  float scale, mbf;
};

// d = imDepth.at<float>((int)kp.pt.y, (int)kp.pt.x) (kp = mvKeys[i], the DISTORTED keypoint); d > 0: {d, kpU.x - mbf / d},
// otherwise {-1, -1}.  A truncated pixel outside the plane, or a NaN coordinate, is {-1, -1} (the reference reads out of
// bounds there).  Float arithmetic, correctly rounded division, no contraction: convertTo's cvt_32f is x * scale + 0.
__device__ __forceinline__ void rgbd_depth(const DepthPlane &P, float kx, float ky, float kux, float *depth, float *ur) {
  float d = -1.0f, u = -1.0f;
  if (kx > -1.0f && ky > -1.0f && kx < (float)P.cols && ky < (float)P.rows) {  // (NaN fails every comparison)
    const uint8_t *row = P.base + (size_t)(int)ky * P.stride;
    const int col = (int)kx;
    float z = P.type == VSG_DEPTH_U16 ? (float)((const uint16_t *)row)[col] : ((const float *)row)[col];
    if (P.convert) z = fmul(z, P.scale);
    if (z > 0) d = z, u = fsub(kux, fdiv(P.mbf, z));
  }
  *depth = d, *ur = u;
}

// Batched form (vsg_rgbd_depth_batch_device): one thread per [frame][record] of the extractor's device outputs -- read the
// record, undistort it (the source k_frame_grid_build runs), sample, write.  Writes are coalesced [nframes][capacity].
__global__ __launch_bounds__(256) void k_rgbd_batch(const KeyPointPOD *__restrict__ kps, const int *__restrict__ counts,
                                                    int capacity, int nframes, size_t frame_stride, DepthPlane P,
                                                    CamModel cam, float *__restrict__ u_right,
                                                    float *__restrict__ depth_out) {
  const size_t r = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= (size_t)nframes * capacity) return;
  const int f = (int)(r / (size_t)capacity), i = (int)(r - (size_t)f * capacity);
  float d = -1.0f, u = -1.0f;
  if (i < counts[2 * f]) {
    const KeyPointPOD kp = kps[r];
    float ux = kp.x, uy;
    if (cam.distorted) undistort_point(cam, kp.x, kp.y, &ux, &uy);
    DepthPlane Pf = P;
    Pf.base = P.base + (size_t)f * frame_stride;
    rgbd_depth(Pf, kp.x, kp.y, ux, &d, &u);
  }
  u_right[r] = u;
  depth_out[r] = d;
}

// ---- Frame::AssignFeaturesToGrid (Frame.cc:521-553) for keypoints [i0, i0 + n) -> CSR (cell_start, ent) with the
// entries of every cell in ascending keypoint order (= the push_back order of the reference), index = i - i0.
// One workgroup: per-cell counts by LDS atomics, one block scan, an unordered atomic append, then every cell's
// (handful of) entries are put in index order by the thread that owns the cell.
__global__ __launch_bounds__(1024) void k_frame_grid_build(const KeyPointPOD *__restrict__ kps, int i0, int n,
                                                            float minX, float minY, float invW, float invH,
                                                            int *__restrict__ cell_start, GridEnt *__restrict__ ent,
                                                            KeyPointPOD *__restrict__ kps_copy,
                                                            const uint8_t *__restrict__ desc_src,
                                                            uint8_t *__restrict__ desc_copy,
                                                            int *__restrict__ zero_cells, CamModel cam,
                                                            KeyPointPOD *__restrict__ kps_un_host,
                                                            const int *__restrict__ n_dev, int n_cap, DepthPlane dp,
                                                            float *__restrict__ uright, float *__restrict__ uright_host,
                                                            float *__restrict__ depth_host) {
  // n_dev: the keypoint count where the extractor's chain left it ({n, monoIndex} of the frame) -- the launch that rides
  // behind operator()'s chain (vsg_orb_extract_to_frame) is enqueued before the host knows it
  if (n_dev) n = min(*n_dev, n_cap);
  __shared__ int s_cnt[kGridCells + 1];
  __shared__ int s_fill[kGridCells];
  __shared__ int s_wtot[16];
  const int tid = threadIdx.x;
  // making a frame resident straight out of the extractor is ONE launch: the keypoint / descriptor records are copied
  // into the frame's block and the (absent) right-camera grid is emptied by the threads that build the grid
  // Frame::UndistortKeyPoints (Frame.cc:891-921) on the way: with a distorted camera the frame's keypoints are mvKeysUn
  // -- every pt through cv::undistortPoints' five double-precision iterations (vsg_undistort.h) -- and the grid below is
  // built from THEM; the host's copy of mvKeysUn is written to pinned memory by the same threads
  // An RGB-D frame (dp.base) samples its depth plane in the same loop: Frame::ComputeStereoFromRGBD (Frame.cc:1129-1150)
  // reads the depth at mvKeys[i] and subtracts from mvKeysUn[i].x -- both are in hand here
  const bool undist = kps_copy && cam.distorted;
  if (undist || dp.base) {
    for (int i = tid; i < n; i += 1024) {
      KeyPointPOD kp = kps[i0 + i];
      const float kx = kp.x, ky = kp.y;
      if (undist) {
        undistort_point(cam, kp.x, kp.y, &kp.x, &kp.y);
        kps_copy[i] = kp;
        if (kps_un_host) kps_un_host[i] = kp;
      }
      if (dp.base) {
        float d, u;
        rgbd_depth(dp, kx, ky, kp.x, &d, &u);
        uright[i] = u;
        if (uright_host) uright_host[i] = u;
        if (depth_host) depth_host[i] = d;
      }
    }
  }
  if (!undist && kps_copy) {
    for (int i = tid; i < n * 7; i += 1024) ((uint32_t *)kps_copy)[i] = ((const uint32_t *)(kps + i0))[i];
  }
  if (desc_copy)
    for (int i = tid; i < n * 8; i += 1024) ((uint32_t *)desc_copy)[i] = ((const uint32_t *)desc_src)[i];
  if (zero_cells)
    for (int c = tid; c <= kGridCells; c += 1024) zero_cells[c] = 0;
  for (int c = tid; c <= kGridCells; c += 1024) s_cnt[c] = 0;
  __syncthreads();  // (also: the undistorted records above are visible to the whole workgroup)
  const KeyPointPOD *gsrc = undist ? kps_copy : kps + i0;  // the keypoints the grid indexes (mvKeysUn)
  // PosInGrid (Frame.cc:870-880): round() = half away from zero
  auto cell_of = [&](const KeyPointPOD &kp) -> int {
    const int px = cvt_int_x86(roundf(fmul(fsub(kp.x, minX), invW)));
    const int py = cvt_int_x86(roundf(fmul(fsub(kp.y, minY), invH)));
    return (px < 0 || px >= kGridCols || py < 0 || py >= kGridRows) ? -1 : px * kGridRows + py;
  };
  for (int i = tid; i < n; i += 1024) {
    const int c = cell_of(gsrc[i]);
    if (c >= 0) atomicAdd(&s_cnt[c], 1);
  }
  __syncthreads();
  {  // exclusive scan of the 3072 counts: 3 cells per thread
    const int c0 = tid * 3;
    const int a = s_cnt[c0], b = s_cnt[c0 + 1], c = s_cnt[c0 + 2];
    const int s = a + b + c;
    const int incl = wave_incl_scan(s);
    if ((tid & 63) == 63) s_wtot[tid >> 6] = incl;
    __syncthreads();
    int base = 0;
    for (int w = 0; w < (tid >> 6); w++) base += s_wtot[w];
    const int start = base + incl - s;
    __syncthreads();
    s_cnt[c0] = start, s_cnt[c0 + 1] = start + a, s_cnt[c0 + 2] = start + a + b;
    s_fill[c0] = start, s_fill[c0 + 1] = start + a, s_fill[c0 + 2] = start + a + b;
    if (tid == 1023) s_cnt[kGridCells] = start + s;
  }
  __syncthreads();
  for (int c = tid; c <= kGridCells; c += 1024) cell_start[c] = s_cnt[c];
  // The reference's cells list their features in index order (mGrid[i][j].push_back in AssignFeaturesToGrid's loop,
  // Frame.cc:521-533): the scatter's atomics do not, so every cell is put in order afterwards.  Up to kGridLdsMax
  // keypoints that happens in LDS on the 4-byte (index | octave) words alone and the 12-byte entries are written once,
  // coalesced, from the sorted words (sorting the entries where they lie -- global memory, a dependent round trip per
  // comparison -- was a third of this launch's 18 us at 1250 keypoints).
  __shared__ uint32_t s_io[kGridLdsMax];
  if (n <= kGridLdsMax) {
    for (int i = tid; i < n; i += 1024) {
      const KeyPointPOD kp = gsrc[i];
      const int c = cell_of(kp);
      if (c < 0) continue;
      s_io[atomicAdd(&s_fill[c], 1)] = (uint32_t)i | ((uint32_t)(kp.octave & 0xFFFF) << 16);
    }
    __syncthreads();
    for (int c = tid; c < kGridCells; c += 1024) {  // insertion sort by index: cells hold a few entries
      const int e0 = s_cnt[c], e1 = s_cnt[c + 1];
      for (int a = e0 + 1; a < e1; a++) {
        const uint32_t v = s_io[a];
        int b = a - 1;
        while (b >= e0 && (s_io[b] & 0xFFFFu) > (v & 0xFFFFu)) {
          s_io[b + 1] = s_io[b];
          b--;
        }
        s_io[b + 1] = v;
      }
    }
    __syncthreads();
    const int nin = s_cnt[kGridCells];
    for (int e = tid; e < nin; e += 1024) {
      const uint32_t io = s_io[e];
      const KeyPointPOD kp = gsrc[io & 0xFFFFu];
      ent[e] = {kp.x, kp.y, io};
    }
    return;
  }
  for (int i = tid; i < n; i += 1024) {
    const KeyPointPOD kp = gsrc[i];
    const int c = cell_of(kp);
    if (c < 0) continue;
    const int slot = atomicAdd(&s_fill[c], 1);
    ent[slot] = {kp.x, kp.y, (uint32_t)i | ((uint32_t)(kp.octave & 0xFFFF) << 16)};
  }
  __threadfence_block();
  __syncthreads();
  for (int c = tid; c < kGridCells; c += 1024) {  // insertion sort by index: cells hold a few entries
    const int e0 = s_cnt[c], e1 = s_cnt[c + 1];
    for (int a = e0 + 1; a < e1; a++) {
      const GridEnt v = ent[a];
      int b = a - 1;
      while (b >= e0 && (ent[b].io & 0xFFFFu) > (v.io & 0xFFFFu)) {
        ent[b + 1] = ent[b];
        b--;
      }
      ent[b + 1] = v;
    }
  }
}

// device layout of a frame for `cap` features.  grid_only: the block behind a vsg_grid -- the left grid and an (empty)
// right cell table, which is all a list-mode window search without descriptors reads (GridEnt carries the keypoint
// fields it tests); the blocks a grid never has are zero bytes long
struct FrameLayout {
  size_t oK, oD, oU, oCS0, oE0, oCS1, oE1, oFvH, oFvN, oFvO, oFvI, total;
  bool grid_only;
  explicit FrameLayout(int cap, bool grid_only_ = false) : grid_only(grid_only_) {
    Stage st;
    const size_t C = (size_t)cap + 1, X = grid_only ? 0 : C;
    oK = st.add(X * sizeof(KeyPointPOD));
    oD = st.add(X * 32);
    oU = st.add(X * 4);
    oCS0 = st.add((kGridCells + 1) * 4);
    oE0 = st.add(C * sizeof(GridEnt));
    oCS1 = st.add((kGridCells + 1) * 4);
    oE1 = st.add(X * sizeof(GridEnt));
    oFvH = st.add(X ? 64 : 0), oFvN = st.add(X * 4), oFvO = st.add(X ? (C + 1) * 4 : 0), oFvI = st.add(X * 4);  // Frame::mFeatVec
    total = st.total;
  }
};

// Frame::AssignFeaturesToGrid (Frame.cc:521-553) on the host for keys [i0, i0 + n): stable bucket fill with the
// reference's float operations (PosInGrid, Frame.cc:870-880; libm round = half away from zero)
void host_grid(const vsg_keypoint *kps, int i0, int n, float minX, float minY, float invW, float invH, int *cell_start,
               GridEnt *ent) {
  std::vector<int16_t> cell_of((size_t)n + 1);
  std::vector<int> cnt(kGridCells, 0);
  for (int i = 0; i < n; i++) {
    const int px = cvt_int_x86(roundf(fmul(fsub(kps[i0 + i].x, minX), invW)));
    const int py = cvt_int_x86(roundf(fmul(fsub(kps[i0 + i].y, minY), invH)));
    const bool in = !(px < 0 || px >= kGridCols || py < 0 || py >= kGridRows);
    cell_of[i] = in ? (int16_t)(px * kGridRows + py) : (int16_t)-1;
    if (in) cnt[px * kGridRows + py]++;
  }
  int run = 0;
  for (int c = 0; c < kGridCells; c++) {
    cell_start[c] = run;
    run += cnt[c];
    cnt[c] = cell_start[c];
  }
  cell_start[kGridCells] = run;
  for (int i = 0; i < n; i++)
    if (cell_of[i] >= 0) {  // insertion order == ascending keypoint index
      const vsg_keypoint &k = kps[i0 + i];
      ent[cnt[cell_of[i]]++] = {k.x, k.y, (uint32_t)i | ((uint32_t)(k.octave & 0xFFFF) << 16)};
    }
}

void set_bounds(vsg_frame *f, float min_x, float min_y, float max_x, float max_y) {
  f->minX = min_x, f->minY = min_y, f->maxX = max_x, f->maxY = max_y;
  // mfGridElementWidthInv = FRAME_GRID_COLS / (mnMaxX - mnMinX)   (Frame.cc:378-379)
  f->invW = (float)kGridCols / (max_x - min_x);
  f->invH = (float)kGridRows / (max_y - min_y);
}

// The device block of a frame for `capacity` features on `device`.  zero_fill: a frame that was created but never
// uploaded has n = 0 AND all-zero cell_start arrays, so a search on it walks empty [0, 0) entry ranges instead of whatever
// the allocation held.  The fill runs on the calling thread's own stream and is WAITED for: uploads and searches use
// non-blocking streams, which the NULL stream's hipMemset is not ordered against (it could land after an upload and wipe
// it).  A grid is uploaded by the call that creates it and skips the fill.  *ctx = the calling thread's context.
int frame_alloc(int device, int capacity, const FrameLayout &L, bool zero_fill, vsg_frame *f, ThreadCtx **ctx) {
  // (thread_ctx below checks the device again, but reports a failed hipSetDevice as VSG_ERR_NO_DEVICE; creating a
  // frame or a grid has always answered VSG_ERR_HIP there, hence the check of its own)
  const int drc = use_device(device);
  if (drc != VSG_OK) return drc;
  f->device = device;
  f->capacity = capacity;
  int rc = VSG_OK;
  ThreadCtx *c = *ctx = thread_ctx(device, &rc);
  if (!c) return rc;
  if (hipMalloc((void **)&f->d_block, L.total) != hipSuccess) return VSG_ERR_HIP;
  if (zero_fill &&
      (hipMemsetAsync(f->d_block, 0, L.total, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess)) {
    hipFree(f->d_block);
    f->d_block = nullptr;
    return VSG_ERR_HIP;
  }
  f->d_kps = (KeyPointPOD *)(f->d_block + L.oK);
  f->d_desc = f->d_block + L.oD;
  f->d_uright = (float *)(f->d_block + L.oU);
  f->d_cell_start[0] = (int *)(f->d_block + L.oCS0);
  f->d_ent[0] = (GridEnt *)(f->d_block + L.oE0);
  f->d_cell_start[1] = (int *)(f->d_block + L.oCS1);
  f->d_ent[1] = (GridEnt *)(f->d_block + L.oE1);
  f->d_fv_hdr = (int *)(f->d_block + L.oFvH), f->d_fv_node = (int *)(f->d_block + L.oFvN);
  f->d_fv_off = (int *)(f->d_block + L.oFvO), f->d_fv_idx = (int *)(f->d_block + L.oFvI);
  return VSG_OK;
}

// What vsg_frame_upload and vsg_grid_build share: bounds and grid(s) [, keypoints, descriptors, mvuRight] of a frame
// laid out as L.  The whole device image is assembled in the calling thread's pinned arena and goes up in ONE DMA.
int frame_put(vsg_frame *f, ThreadCtx *c, const FrameLayout &L, const vsg_keypoint *keys, const uint8_t *desc,
              const float *u_right, int n, int nleft, float min_x, float min_y, float max_x, float max_y) {
  const int rc = ctx_reserve(c, L.total, 0);
  if (rc != VSG_OK) return rc;
  set_bounds(f, min_x, min_y, max_x, max_y);
  f->n = n, f->nleft = nleft, f->has_uright = u_right != nullptr, f->fv_valid = false, f->pose_held = false;
  f->stereo_attached = f->any_stereo = false;
  for (int i = 0; u_right && i < n; i++) f->any_stereo |= u_right[i] >= 0;
  uint8_t *h = c->h_pin;
  if (n && !L.grid_only) memcpy(h + L.oK, keys, (size_t)n * sizeof(vsg_keypoint));
  if (desc && n) memcpy(h + L.oD, desc, (size_t)n * 32);
  if (u_right && n) memcpy(h + L.oU, u_right, (size_t)n * 4);
  const int nl = nleft == -1 ? n : nleft;
  host_grid(keys, 0, nl, f->minX, f->minY, f->invW, f->invH, (int *)(h + L.oCS0), (GridEnt *)(h + L.oE0));
  if (nleft != -1)
    host_grid(keys, nleft, n - nleft, f->minX, f->minY, f->invW, f->invH, (int *)(h + L.oCS1), (GridEnt *)(h + L.oE1));
  else
    memset(h + L.oCS1, 0, (kGridCells + 1) * 4);
  // only the used part of every block travels: [keys | desc | uright | grid] are contiguous up to the right grid
  const size_t used = nleft != -1 ? L.oE1 + (size_t)(n - nleft + 1) * sizeof(GridEnt) : L.oCS1 + (kGridCells + 1) * 4;
  TRY_HIP(hipMemcpyAsync(f->d_block, h, used, hipMemcpyHostToDevice, c->stream));
  TRY_HIP(hipStreamSynchronize(c->stream));  // the frame may be searched from any thread from now on
  return VSG_OK;
}

}  // namespace

extern "C" {

int vsg_frame_create(int device, int capacity, vsg_frame **out) {
  if (!out || capacity < 1 || capacity > 32767) return VSG_ERR_INVALID;
  *out = nullptr;
  vsg_frame *f = new vsg_frame();
  ThreadCtx *c = nullptr;
  const int rc = frame_alloc(device, capacity, FrameLayout(capacity), true, f, &c);
  if (rc != VSG_OK) {
    delete f;
    return rc;
  }
  *out = f;
  return VSG_OK;
}

void vsg_frame_destroy(vsg_frame *f) {
  if (!f) return;
  hipSetDevice(f->device);
  hipFree(f->d_block);
  hipFree(f->d_pose);
  hipFree(f->d_stereo);
  delete f;
}

int vsg_frame_size(const vsg_frame *f) { return f ? f->n : VSG_ERR_INVALID; }

int vsg_frame_upload(vsg_frame *f, const vsg_keypoint *keys, const uint8_t *desc, const float *u_right, int n,
                     int nleft, float min_x, float min_y, float max_x, float max_y) {
  if (frame_check(f) != VSG_OK || n < 0 || n > f->capacity || (n > 0 && (!keys || !desc)) || nleft < -1 || nleft > n)
    return VSG_ERR_INVALID;
  // packed candidate entries carry the octave in 4 bits (index : 15 | distance : 9 | octave : 4, vsg_walks.h)
  for (int i = 0; i < n; i++)
    if (keys[i].octave < 0 || keys[i].octave > 15) return VSG_ERR_UNSUPPORTED;
  int rc = VSG_OK;
  ThreadCtx *c = thread_ctx(f->device, &rc);
  if (!c) return rc;
  rc = frame_put(f, c, FrameLayout(f->capacity), keys, desc, u_right, n, nleft, min_x, min_y, max_x, max_y);
  if (rc == VSG_OK) f->h_kps.assign(keys, keys + n);
  return rc;
}

// ---- the stand-alone Frame grid (include/vsg_orb.h: vsg_grid): a frame block that holds the left grid alone, built by
// the upload path and searched by the list mode of k_window_search
void vsg_grid_destroy(vsg_grid *g) { vsg_frame_destroy(grid_frame(g)); }

int vsg_grid_build(int device, const vsg_keypoint *kps, int n, float min_x, float min_y, float max_x, float max_y,
                   vsg_grid **out) {
  if (!out || n < 0 || (n > 0 && !kps) || n > 32767) return VSG_ERR_INVALID;
  *out = nullptr;
  // GridEnt carries the level in 16 bits; the queries compare it whole, so (unlike a frame's) it need not fit 0..15
  for (int i = 0; i < n; i++)
    if (kps[i].octave < INT16_MIN || kps[i].octave > INT16_MAX) return VSG_ERR_UNSUPPORTED;
  const int cap = n > 0 ? n : 1;
  const FrameLayout L(cap, true);
  vsg_frame *g = new vsg_frame();
  ThreadCtx *c = nullptr;
  // no zero fill: the upload below writes everything a search reads (both cell tables and the entries they index),
  // and the fill is a memset and a second stream wait inside a call whose whole cost is one small DMA and one wait
  int rc = frame_alloc(device, cap, L, false, g, &c);
  if (rc == VSG_OK) rc = frame_put(g, c, L, kps, nullptr, nullptr, n, -1, min_x, min_y, max_x, max_y);
  if (rc != VSG_OK) {
    vsg_frame_destroy(g);
    return rc;
  }
  *out = (vsg_grid *)g;
  return VSG_OK;
}

// one launch: [undistortion +] grid from the keypoints where they already are (the extractor's output) + the two record
// copies + an empty right-camera grid
static int frame_from_extractor(vsg_frame *f, vsg_orb *h, int index, const vsg_keypoint *kps_host, int n,
                                const CamModel &cam, float min_x, float min_y, float max_x, float max_y,
                                vsg_keypoint *keys_un_out) {
  OrbOutputView v;
  int rc = vsg_orb_output_view(h, index, &v);
  if (rc != VSG_OK) return rc;
  if (v.device != f->device) return VSG_ERR_INVALID;
  ThreadCtx *c = thread_ctx(f->device, &rc);
  if (!c) return rc;
  KeyPointPOD *un_pin = nullptr, *un_dev = nullptr;
  if (cam.distorted) {  // mvKeysUn comes back through the calling thread's pinned arena (written by the kernel itself)
    rc = ctx_reserve(c, (size_t)(n + 1) * sizeof(KeyPointPOD), 0);
    if (rc != VSG_OK) return rc;
    un_pin = (KeyPointPOD *)c->h_pin, un_dev = (KeyPointPOD *)c->d_pin;
  }
  set_bounds(f, min_x, min_y, max_x, max_y);
  f->n = n, f->nleft = -1, f->has_uright = false, f->fv_valid = false, f->pose_held = false;
  f->stereo_attached = f->any_stereo = false;
  if (v.done) TRY_HIP(hipStreamWaitEvent(c->stream, v.done, 0));
  hipLaunchKernelGGL(k_frame_grid_build, dim3(1), dim3(1024), 0, c->stream, v.d_kps, 0, n, f->minX, f->minY, f->invW,
                     f->invH, f->d_cell_start[0], f->d_ent[0], f->d_kps, v.d_desc, f->d_desc, f->d_cell_start[1], cam,
                     un_dev, (const int *)nullptr, 0, DepthPlane(), (float *)nullptr, (float *)nullptr,
                     (float *)nullptr);
  TRY_HIP(hipGetLastError());
  if (!cam.distorted) f->h_kps.assign(kps_host, kps_host + n);  // beside the kernel
  TRY_HIP(hipStreamSynchronize(c->stream));
  if (cam.distorted) {
    f->h_kps.assign((const vsg_keypoint *)un_pin, (const vsg_keypoint *)un_pin + n);
    if (keys_un_out && n) memcpy(keys_un_out, un_pin, (size_t)n * sizeof(vsg_keypoint));
  } else if (keys_un_out && n && keys_un_out != kps_host) {
    memcpy(keys_un_out, kps_host, (size_t)n * sizeof(vsg_keypoint));  // mvKeysUn = mvKeys (Frame.cc:893-897)
  }
  return VSG_OK;
}

int vsg_frame_from_extractor(vsg_frame *f, vsg_orb *h, int index, const vsg_keypoint *kps_host, int n, float min_x,
                             float min_y, float max_x, float max_y) {
  if (frame_check(f) != VSG_OK || !h || n < 0 || n > f->capacity || (n > 0 && !kps_host)) return VSG_ERR_INVALID;
  CamModel cam = {};
  return frame_from_extractor(f, h, index, kps_host, n, cam, min_x, min_y, max_x, max_y, nullptr);
}

// ---- Frame::Frame(...) in ONE call and ONE wait: ExtractORB (operator()) -> UndistortKeyPoints -> AssignFeaturesToGrid
// (Frame.cc:344-358 for RGB-D).  The grid launch is enqueued on the extractor's stream right behind its stage chain -- it
// reads the keypoint count from the device -- so the blocking call's single wait covers both, instead of
// operator() [wait] -> vsg_frame_from_extractor* [launch, wait].
namespace {
// the depth plane of an RGB-D call as the caller passed it, and where the hook puts it when it has to be staged
struct RgbdIn {
  const uint8_t *src;
  size_t stride, row_bytes;
  DepthPlane plane;        // base = the device alias of pinned caller memory, or of the staging area
  uint8_t *stage_host;     // non-null: copy the plane here (packed rows) before the launch
  float *ur_dev, *ur_pin, *depth_pin;
};
struct ToFrameHook {
  vsg_frame *f;
  CamModel cam;
  KeyPointPOD *un_dev;
  const RgbdIn *rgbd;  // nullptr: gray only
};
int to_frame_hook(void *ctx, hipStream_t s, const OrbOutputView &v) {
  const ToFrameHook *H = (const ToFrameHook *)ctx;
  vsg_frame *f = H->f;
  DepthPlane dp = DepthPlane();
  float *ur = nullptr, *ur_pin = nullptr, *depth_pin = nullptr;
  if (const RgbdIn *R = H->rgbd) {
    // pageable (or registered) depth is copied into the pinned arena HERE: the extractor's chain is already enqueued, so
    // this copy runs while the device works through it instead of in front of it
    if (R->stage_host)
      for (int y = 0; y < R->plane.rows; y++)
        memcpy(R->stage_host + (size_t)y * R->plane.stride, R->src + (size_t)y * R->stride, R->row_bytes);
    dp = R->plane, ur = R->ur_dev, ur_pin = R->ur_pin, depth_pin = R->depth_pin;
  }
  hipLaunchKernelGGL(k_frame_grid_build, dim3(1), dim3(1024), 0, s, v.d_kps, 0, 0, f->minX, f->minY, f->invW, f->invH,
                     f->d_cell_start[0], f->d_ent[0], f->d_kps, v.d_desc, f->d_desc, f->d_cell_start[1], H->cam, H->un_dev,
                     v.d_counts, f->capacity, dp, ur, ur_pin, depth_pin);
  return hipGetLastError() == hipSuccess ? VSG_OK : VSG_ERR_HIP;
}

void frame_clear(vsg_frame *f) {
  f->n = 0, f->nleft = -1, f->has_uright = false, f->fv_valid = false, f->pose_held = false;
  f->stereo_attached = f->any_stereo = false;
  f->h_kps.clear();
}

// the depth arguments of vsg_orb_extract_to_frame_rgbd / vsg_rgbd_depth_batch_device -> a DepthPlane without its base
int depth_plane(int type, size_t stride, int rows, int cols, float scale, float mbf, DepthPlane *P) {
  if (type != VSG_DEPTH_U16 && type != VSG_DEPTH_F32) return VSG_ERR_UNSUPPORTED;
  const size_t elem = type == VSG_DEPTH_U16 ? 2 : 4;
  if (rows < 1 || cols < 1 || stride < (size_t)cols * elem || stride % elem) return VSG_ERR_INVALID;
  P->base = nullptr, P->stride = stride, P->type = type, P->rows = rows, P->cols = cols;
  // if((fabs(mDepthMapFactor-1.0f)>1e-5) || imDepth.type()!=CV_32F)  (Tracking.cc:1610): float difference, double compare
  P->convert = ((double)fabsf(scale - 1.0f) > 1e-5 || type != VSG_DEPTH_F32) ? 1 : 0;
  P->scale = scale, P->mbf = mbf;
  return VSG_OK;
}

struct RgbdArgs {
  const void *depth;
  int type;
  size_t stride;
  int rows, cols;
  float scale, mbf;
  float *u_right, *depth_out;
};

int extract_to_frame(vsg_orb *h, const uint8_t *gray, int rows, int cols, int stride, int lap0, int lap1,
                     vsg_keypoint *kps, uint8_t *desc, int capacity, int *n, vsg_frame *f, const float K4[4],
                     const float *dist, int ndist, float min_x, float min_y, float max_x, float max_y,
                     vsg_keypoint *keys_un_out, const RgbdArgs *A) {
  if (n) *n = 0;
  if (frame_check(f) != VSG_OK || !h || !kps || !desc || !n) return VSG_ERR_INVALID;
  // the hook launches on the extractor's stream with the frame's device pointers: one device for both
  if (vsg_orb_device_of(h) != f->device) return VSG_ERR_INVALID;
  ToFrameHook H;
  H.f = f, H.un_dev = nullptr, H.rgbd = nullptr;
  H.cam = CamModel();
  if (K4 && !make_cam_model(K4, dist, ndist, &H.cam)) return VSG_ERR_INVALID;
  RgbdIn R = {};
  if (!gray || rows <= 0 || cols <= 0) A = nullptr;  // operator() returns -1 for an empty image: nothing to sample
  if (A) {
    int rc = depth_plane(A->type, A->stride, A->rows, A->cols, A->scale, A->mbf, &R.plane);
    if (rc == VSG_OK && (!A->depth || A->rows != rows || A->cols != cols || (uintptr_t)A->depth % (A->type == VSG_DEPTH_U16 ? 2 : 4)))
      rc = VSG_ERR_INVALID;
    if (rc != VSG_OK) {
      frame_clear(f);
      return rc;
    }
  }
  int rc = VSG_OK;
  ThreadCtx *c = thread_ctx(f->device, &rc);
  if (!c) return rc;
  // the calling thread's pinned arena: [mvKeysUn | mvuRight | mvDepth | staged depth plane]
  Stage st;
  const size_t C1 = (size_t)f->capacity + 1;
  const size_t oUn = st.add(H.cam.distorted ? C1 * sizeof(KeyPointPOD) : 0);
  const size_t oUr = st.add(A ? C1 * 4 : 0), oDp = st.add(A ? C1 * 4 : 0);
  void *alias = nullptr;
  const size_t row_bytes = A ? (size_t)A->cols * (A->type == VSG_DEPTH_U16 ? 2 : 4) : 0;
  const size_t span = A ? (size_t)(A->rows - 1) * A->stride + row_bytes : 0;
  const bool direct = A && vsg_orb_host_direct(h, A->depth, span, &alias);
  const size_t oPl = st.add(A && !direct ? (size_t)A->rows * row_bytes : 0);
  if (st.total) {
    rc = ctx_reserve(c, st.total, 0);
    if (rc != VSG_OK) return rc;
  }
  KeyPointPOD *un_pin = nullptr;
  if (H.cam.distorted) un_pin = (KeyPointPOD *)(c->h_pin + oUn), H.un_dev = (KeyPointPOD *)(c->d_pin + oUn);
  if (A) {
    R.src = (const uint8_t *)A->depth, R.stride = A->stride, R.row_bytes = row_bytes;
    if (direct) {
      R.plane.base = (const uint8_t *)alias;
    } else {
      R.stage_host = c->h_pin + oPl, R.plane.base = c->d_pin + oPl, R.plane.stride = row_bytes;
    }
    R.ur_dev = f->d_uright, R.ur_pin = (float *)(c->d_pin + oUr), R.depth_pin = (float *)(c->d_pin + oDp);
    H.rgbd = &R;
  }
  set_bounds(f, min_x, min_y, max_x, max_y);
  vsg_orb_set_post_chain(h, to_frame_hook, &H);
  const int mono = vsg_orb_extract(h, gray, rows, cols, stride, lap0, lap1, kps, desc, capacity, n);
  vsg_orb_set_post_chain(h, nullptr, nullptr);  // (a call that failed before its submit leaves the hook unconsumed)
  if (mono < 0 || *n > f->capacity) {
    // the bounds are already the new ones and the hook may have rewritten the device arrays: the frame holds nothing
    // searchable any more, and says so
    frame_clear(f);
    return mono < 0 ? mono : VSG_ERR_CAPACITY;
  }
  f->n = *n, f->nleft = -1, f->has_uright = A != nullptr, f->fv_valid = false, f->pose_held = false;
  f->stereo_attached = false, f->any_stereo = f->has_uright;  // mvuRight is computed on the device: assume some are >= 0
  if (H.cam.distorted) {
    f->h_kps.assign((const vsg_keypoint *)un_pin, (const vsg_keypoint *)un_pin + *n);
    if (keys_un_out && *n) memcpy(keys_un_out, un_pin, (size_t)*n * sizeof(vsg_keypoint));
  } else {
    f->h_kps.assign(kps, kps + *n);
    if (keys_un_out && *n && keys_un_out != kps) memcpy(keys_un_out, kps, (size_t)*n * sizeof(vsg_keypoint));
  }
  if (A && A->u_right && *n) memcpy(A->u_right, c->h_pin + oUr, (size_t)*n * 4);
  if (A && A->depth_out && *n) memcpy(A->depth_out, c->h_pin + oDp, (size_t)*n * 4);
  return mono;
}
}  // namespace

int vsg_orb_extract_to_frame(vsg_orb *h, const uint8_t *gray, int rows, int cols, int stride, int lap0, int lap1,
                             vsg_keypoint *kps, uint8_t *desc, int capacity, int *n, vsg_frame *f, const float K4[4],
                             const float *dist, int ndist, float min_x, float min_y, float max_x, float max_y,
                             vsg_keypoint *keys_un_out) {
  return extract_to_frame(h, gray, rows, cols, stride, lap0, lap1, kps, desc, capacity, n, f, K4, dist, ndist, min_x,
                          min_y, max_x, max_y, keys_un_out, nullptr);
}

int vsg_orb_extract_to_frame_rgbd(vsg_orb *h, const uint8_t *gray, int rows, int cols, int stride, int lap0, int lap1,
                                  vsg_keypoint *kps, uint8_t *desc, int capacity, int *n, vsg_frame *f,
                                  const float K4[4], const float *dist, int ndist, float min_x, float min_y, float max_x,
                                  float max_y, vsg_keypoint *keys_un_out, const void *depth, int depth_type,
                                  size_t depth_stride, int depth_rows, int depth_cols, float depth_scale, float mbf,
                                  float *u_right, float *depth_out) {
  const RgbdArgs A = {depth, depth_type, depth_stride, depth_rows, depth_cols, depth_scale, mbf, u_right, depth_out};
  return extract_to_frame(h, gray, rows, cols, stride, lap0, lap1, kps, desc, capacity, n, f, K4, dist, ndist, min_x,
                          min_y, max_x, max_y, keys_un_out, &A);
}

float vsg_depth_map_scale(float yaml_value) {
  // mDepthMapFactor = fSettings["RGBD.DepthMapFactor"]; if(fabs(mDepthMapFactor)<1e-5) mDepthMapFactor=1;
  // else mDepthMapFactor = 1.0f/mDepthMapFactor;  (Tracking.cc:638-642)
  if ((double)fabsf(yaml_value) < 1e-5) return 1.0f;
  return 1.0f / yaml_value;
}

int vsg_rgbd_depth_batch_device(int device, const void *d_depth, int depth_type, int nframes, size_t frame_stride,
                                size_t depth_stride, int rows, int cols, float depth_scale, float mbf, const float K4[4],
                                const float *dist, int ndist, const vsg_keypoint *d_kps, const int *d_counts,
                                int capacity, float *d_u_right, float *d_depth_out, void *stream) {
  DepthPlane P;
  const int rc = depth_plane(depth_type, depth_stride, rows, cols, depth_scale, mbf, &P);
  if (rc != VSG_OK) return rc;
  const size_t elem = depth_type == VSG_DEPTH_U16 ? 2 : 4;
  if (!d_depth || !d_kps || !d_counts || !d_u_right || !d_depth_out || nframes < 1 || capacity < 1 ||
      (nframes > 1 && frame_stride < (size_t)(rows - 1) * depth_stride + (size_t)cols * elem) ||
      frame_stride % elem || (uintptr_t)d_depth % elem)
    return VSG_ERR_INVALID;
  CamModel cam;
  if (!make_cam_model(K4, dist, ndist, &cam)) return VSG_ERR_INVALID;
  const int drc = use_device(device);
  if (drc != VSG_OK) return drc;
  P.base = (const uint8_t *)d_depth;
  const size_t recs = (size_t)nframes * capacity;
  // stream == NULL is the caller's NULL stream: the launch is ordered on both sides of it
  hipLaunchKernelGGL(k_rgbd_batch, dim3((unsigned)((recs + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (const KeyPointPOD *)d_kps, d_counts, capacity, nframes, frame_stride, P, cam, d_u_right,
                     d_depth_out);
  TRY_HIP(hipGetLastError());
  return VSG_OK;
}

int vsg_camera_image_bounds(int cols, int rows, const float K4[4], const float *dist, int ndist, float out[4]) {
  CamModel cam;
  if (!out || cols < 1 || rows < 1 || !make_cam_model(K4, dist, ndist, &cam)) return VSG_ERR_INVALID;
  if (!cam.distorted) {  // Frame.cc:948-954
    out[0] = 0.0f, out[1] = 0.0f, out[2] = (float)cols, out[3] = (float)rows;
    return VSG_OK;
  }
  // the four corners through cv::undistortPoints (Frame.cc:928-946): four points, once per camera -- host arithmetic,
  // the same source the device runs per keypoint
  float x[4], y[4];
  const float cx[4] = {0.f, (float)cols, 0.f, (float)cols}, cy[4] = {0.f, 0.f, (float)rows, (float)rows};
  for (int i = 0; i < 4; i++) undistort_point(cam, cx[i], cy[i], &x[i], &y[i]);
  out[0] = std::min(x[0], x[2]);  // mnMinX = min(mat(0,0), mat(2,0))
  out[2] = std::max(x[1], x[3]);  // mnMaxX = max(mat(1,0), mat(3,0))
  out[1] = std::min(y[0], y[1]);  // mnMinY = min(mat(0,1), mat(1,1))
  out[3] = std::max(y[2], y[3]);  // mnMaxY = max(mat(2,1), mat(3,1))
  return VSG_OK;
}

int vsg_frame_from_extractor_undistort(vsg_frame *f, vsg_orb *h, int index, const vsg_keypoint *kps_host, int n,
                                       const float K4[4], const float *dist, int ndist, float min_x, float min_y,
                                       float max_x, float max_y, vsg_keypoint *keys_un_out) {
  if (frame_check(f) != VSG_OK || !h || n < 0 || n > f->capacity || (n > 0 && !kps_host)) return VSG_ERR_INVALID;
  CamModel cam;
  if (!make_cam_model(K4, dist, ndist, &cam)) return VSG_ERR_INVALID;
  return frame_from_extractor(f, h, index, kps_host, n, cam, min_x, min_y, max_x, max_y, keys_un_out);
}

int vsg_frame_copy_grid(vsg_frame *f, int right, int32_t *cell_start, int32_t *entries) {
  if (frame_check(f) != VSG_OK || !cell_start || !entries || right < 0 || right > 1) return VSG_ERR_INVALID;
  int rc = VSG_OK;
  ThreadCtx *c = thread_ctx(f->device, &rc);
  if (!c) return rc;
  rc = ctx_reserve(c, (kGridCells + 1) * 4 + (size_t)(f->capacity + 1) * sizeof(GridEnt) + 128, 0);
  if (rc != VSG_OK) return rc;
  int *hcs = (int *)c->h_pin;
  GridEnt *he = (GridEnt *)(c->h_pin + (((kGridCells + 1) * 4 + 63) & ~63));
  TRY_HIP(hipMemcpyAsync(hcs, f->d_cell_start[right], (kGridCells + 1) * 4, hipMemcpyDeviceToHost, c->stream));
  TRY_HIP(hipMemcpyAsync(he, f->d_ent[right], (size_t)f->capacity * sizeof(GridEnt), hipMemcpyDeviceToHost, c->stream));
  TRY_HIP(hipStreamSynchronize(c->stream));
  memcpy(cell_start, hcs, (kGridCells + 1) * 4);
  const int ne = hcs[kGridCells];
  if (ne < 0 || ne > f->capacity) return VSG_ERR_HIP;
  for (int i = 0; i < ne; i++) entries[i] = (int)(he[i].io & 0xFFFFu);
  return ne;
}

}  // extern "C"
