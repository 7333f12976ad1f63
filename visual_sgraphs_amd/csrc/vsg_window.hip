// vsg_window.hip -- the windowed ORBmatcher searches on device-resident Frame / KeyFrame features (vsg_frame.hip).
//
//   Frame::GetFeaturesInArea                                         orb_slam3/src/Frame.cc:802-868
//   KeyFrame::GetFeaturesInArea                                      orb_slam3/src/KeyFrame.cc:834-874
//   ORBmatcher::SearchByProjection x5, SearchBySim3, Fuse x2,
//   SearchForInitialization                                          orb_slam3/src/ORBmatcher.cc (lines: below, vsg_windows.h)
//
// One kernel, k_window_search, does everything that is data-parallel in those routines for ALL queries of a call:
// wave = one projected map point: the GetFeaturesInArea window on the resident CSR grid (lanes over the window's
// cells, candidates kept in the reference's order: cells ix outer / iy inner, insertion order inside a cell), the
// level / stereo / chi-square gates, and the Hamming distance to every surviving candidate (query descriptor in
// SGPRs, v_xor + v_bcnt).  Inputs are read from, and results written to, the calling thread's pinned arena straight
// over PCIe: a call is  fill -> ONE launch -> sync -> ordered host pass (vsg_walks.h).  Nothing is allocated and
// nothing runs on the NULL stream.  vsg_grid_query searches a stand-alone Frame grid with the same kernel in list mode.
#include <time.h>

#include <cstring>
#include <vector>

#include "vsg_frame_int.h"

using namespace vsg;

namespace {

struct WinLaunch {
  int nq, mode, gate_mode, best_init, cap;
  uint32_t counter_base;
  float inv_sigma2[16];
};

// ---- the window search (see the file header).  4 queries per 256-thread workgroup, one per wavefront.
// List mode: every query owns an inline slot of kInline entries (one 64-byte line) in the output array, so that the
// host's ordered pass streams through memory; a window with more candidates reserves a segment of the overflow area
// behind the slots with ONE atomic on a never-reset device counter (the host knows its value) and writes its whole
// list there.  {start, length} per query say where the list is.  Best mode: first minimum over the candidates.
// Completion is the stream's: a variant whose last workgroup stamped a pinned flag for the host to spin on needed a
// system-scope fence per wave and took 32 us instead of 13 (MI355X, 1004 queries).
enum { kInline = kWinInline };

__global__ __launch_bounds__(256) void k_window_search(FrameDev F, const WinQuery *__restrict__ Q,
                                                       const uint8_t *__restrict__ qdesc, WinLaunch W,
                                                       int *__restrict__ off, int *__restrict__ cnt,
                                                       uint32_t *__restrict__ out, int *__restrict__ best,
                                                       uint32_t *__restrict__ counter) {
  const int lane = threadIdx.x & 63;
  const int q = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
  if (q < W.nq) {
    const WinQuery wq = Q[q];
    uint32_t qd[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (qdesc) {
      const uint32_t *p = (const uint32_t *)(qdesc + (size_t)q * 32);
#pragma unroll
      for (int k = 0; k < 8; k++) qd[k] = p[k];
    }
    const int right = wq.flags & 1;
    const int *cs = F.cell_start[right];
    const GridEnt *en = F.ent[right];
    const int koff = right ? F.nleft : 0;
    const float x = wq.x, y = wq.y, r = wq.r;
    // (int)floor((x - mnMinX - factorX) * mfGridElementWidthInv) etc. (Frame.cc:810-832): float arithmetic
    // (the int conversions behave like the reference's x86 build for NaN / out-of-range values: cvt_int_x86)
    const int nMinCellX = max(0, cvt_int_x86(floorf(fmul(fsub(fsub(x, F.minX), r), F.invW))));
    const int nMaxCellX = min(kGridCols - 1, cvt_int_x86(ceilf(fmul(fadd(fsub(x, F.minX), r), F.invW))));
    const int nMinCellY = max(0, cvt_int_x86(floorf(fmul(fsub(fsub(y, F.minY), r), F.invH))));
    const int nMaxCellY = min(kGridRows - 1, cvt_int_x86(ceilf(fmul(fadd(fsub(y, F.minY), r), F.invH))));
    const bool active = !(wq.flags & 2) && nMinCellX < kGridCols && nMaxCellX >= 0 && nMinCellY < kGridRows &&
                        nMaxCellY >= 0 && nMaxCellX >= nMinCellX && nMaxCellY >= nMinCellY;
    const int ncy = active ? nMaxCellY - nMinCellY + 1 : 1, ncell = active ? (nMaxCellX - nMinCellX + 1) * ncy : 0;
    const bool bCheckLevels = (wq.minL > 0) || (wq.maxL >= 0);
    // does this grid entry survive GetFeaturesInArea and the routine's static gates?
    auto pass = [&](const GridEnt &g) -> bool {
      const int oct = (int)(int16_t)(g.io >> 16);
      if (bCheckLevels) {
        if (oct < wq.minL) return false;
        if (wq.maxL >= 0 && oct > wq.maxL) return false;
      }
      const float distx = fsub(g.x, x), disty = fsub(g.y, y);
      if (!(fabsf(distx) < r && fabsf(disty) < r)) return false;
      if (wq.hi >= 0 && (oct < wq.lo || oct > wq.hi)) return false;
      if (W.gate_mode == kGateUr) {
        // F.Nleft == -1 && F.mvuRight[idx] > 0: er = fabs(ur - mvuRight[idx]); er > gate -> skip
        // (ORBmatcher.cc:97-102, 1741-1747)
        if (F.uright && F.nleft == -1) {
          const float uR = F.uright[g.io & 0xFFFFu];
          if (uR > 0 && fabsf(fsub(wq.ur, uR)) > wq.gate) return false;
        }
      } else if (W.gate_mode == kGateChi2) {
        // Fuse (ORBmatcher.cc:1267-1292): reprojection error against the keypoint, chi-square at the keypoint's level
        const float uR = F.uright ? F.uright[g.io & 0xFFFFu] : -1.0f;
        const float ex = fsub(x, g.x), ey = fsub(y, g.y);
        const float inv = W.inv_sigma2[oct & 15];
        if (uR >= 0) {
          const float er = fsub(wq.ur, uR);
          const float e2 = fadd(fadd(fmul(ex, ex), fmul(ey, ey)), fmul(er, er));
          if ((double)fmul(e2, inv) > 7.8) return false;
        } else {
          const float e2 = fadd(fmul(ex, ex), fmul(ey, ey));
          if ((double)fmul(e2, inv) > 5.99) return false;
        }
      }
      return true;
    };
    uint32_t bestKey = 0xFFFFFFFFu;
    int bestIdx = -1;
    // One walk over the window in the reference's candidate order (cells ix outer / iy inner = ascending lane, entries
    // in cell order).  `emit(pos, i, dist, oct)` receives every surviving candidate with its list position.
    auto walk_window = [&](auto emit) -> int {
      int count = 0;
      for (int c0 = 0; c0 < ncell; c0 += 64) {
        const int c = c0 + lane;
        int e0 = 0, e1 = 0;
        if (c < ncell) {
          const int cx = c / ncy, cy = c - cx * ncy;
          const int cell = (nMinCellX + cx) * kGridRows + nMinCellY + cy;
          e0 = cs[cell];
          e1 = cs[cell + 1];
        }
        // the filter runs once per entry: survivors are remembered as a bit mask (cells hold a handful of entries;
        // a chunk with a cell of more than 32 falls back to filtering twice)
        const bool big = __ballot(e1 - e0 > 32) != 0;
        uint32_t mask = 0;
        int mine = 0;
        if (!big) {
          for (int e = e0; e < e1; e++)
            if (pass(en[e])) mask |= 1u << (e - e0);
          mine = __popc(mask);
        } else {
          for (int e = e0; e < e1; e++) mine += pass(en[e]) ? 1 : 0;
        }
        const int incl = wave_incl_scan(mine);
        const int tot = __builtin_amdgcn_readlane(incl, 63);
        if (tot == 0) continue;
        int pos = count + incl - mine;
        auto one = [&](int e) {
          const GridEnt g = en[e];
          const int i = (int)(g.io & 0xFFFFu);
          int dist = 0;
          if (qdesc) {
            const uint4 *d = (const uint4 *)(F.desc + (size_t)(i + koff) * 32);
            const uint4 b0 = d[0], b1 = d[1];
            dist = __popc(qd[0] ^ b0.x) + __popc(qd[1] ^ b0.y) + __popc(qd[2] ^ b0.z) + __popc(qd[3] ^ b0.w) +
                   __popc(qd[4] ^ b1.x) + __popc(qd[5] ^ b1.y) + __popc(qd[6] ^ b1.z) + __popc(qd[7] ^ b1.w);
          }
          emit(pos, i, dist, (int)((g.io >> 16) & 15u));
          pos++;
        };
        if (!big) {
          while (mask) {
            one(e0 + __builtin_ctz(mask));
            mask &= mask - 1;
          }
        } else {
          for (int e = e0; e < e1; e++)
            if (pass(en[e])) one(e);
        }
        count += tot;
      }
      return count;
    };
    if (W.mode == kWinList) {
      uint32_t *slot = out + (size_t)q * kInline;
      const int total = walk_window([&](int pos, int i, int dist, int oct) {
        if (pos < kInline) slot[pos] = (uint32_t)i | ((uint32_t)dist << 15) | ((uint32_t)oct << 24);
      });
      int start = q * kInline;
      if (total > kInline) {  // the whole list goes to the overflow area
        int base = 0;
        if (lane == 0) base = (int)(atomicAdd(counter, (uint32_t)total) - W.counter_base);
        base = __builtin_amdgcn_readfirstlane(base);
        start = W.nq * kInline + base;
        uint32_t *seg = out + start;
        const int room = W.cap - base;
        walk_window([&](int pos, int i, int dist, int oct) {
          if (pos < room) seg[pos] = (uint32_t)i | ((uint32_t)dist << 15) | ((uint32_t)oct << 24);
        });
      }
      if (lane == 0) {
        off[q] = start;
        cnt[q] = total;
      }
    } else {
      walk_window([&](int pos, int i, int dist, int) {
        if (dist < W.best_init) {
          const uint32_t key = ((uint32_t)dist << 16) | (uint32_t)pos;  // first minimum in candidate order
          if (key < bestKey) {
            bestKey = key;
            bestIdx = i;
          }
        }
      });
      uint32_t k = bestKey;
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) k = min(k, __shfl_xor(k, d));
      const uint64_t owner = __ballot(bestKey == k && bestIdx >= 0);
      int idx = -1, dist = W.best_init;
      if (k != 0xFFFFFFFFu && owner) {
        idx = __builtin_amdgcn_readlane(bestIdx, __builtin_ctzll(owner));
        dist = (int)(k >> 16);
      }
      if (lane == 0) {
        best[2 * q] = idx < 0 ? -1 : idx + koff;  // index into mDescriptors (ORBmatcher.cc:1294-1295: idx += NLeft)
        best[2 * q + 1] = dist;
      }
    }
  }
}

thread_local int t_cap_hint = 0;  // entries per query the compact candidate array is sized for (sticky, grows)

// where the last window call of this thread spent its wall time (vsg_debug_call_profile): a handful of clock reads
struct CallProf {
  double t0 = 0, fill = 0, launch = 0, sync = 0, total = 0;
};
thread_local CallProf t_prof;
inline double now_us() {
  timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return ts.tv_sec * 1e6 + ts.tv_nsec * 1e-3;
}

}  // namespace

namespace vsg {

FrameDev frame_dev(const vsg_frame *f) {
  FrameDev d;
  d.kps = f->d_kps;
  d.desc = f->d_desc;
  d.uright = f->has_uright ? f->d_uright : nullptr;
  for (int g = 0; g < 2; g++) {
    d.cell_start[g] = f->d_cell_start[g];
    d.ent[g] = f->d_ent[g];
  }
  d.n = f->n;
  d.nleft = f->nleft;
  d.minX = f->minX, d.minY = f->minY, d.invW = f->invW, d.invH = f->invH;
  return d;
}

int WindowCall::begin(int device, int nq_, int mode_, bool with_desc_, size_t arena_base, size_t arena_extra) {
  int rc = VSG_OK;
  if (range_open) range_pop();  // a retry re-enters begin()
  range_push("ORBmatcher window search");
  range_open = true;
  if (arena_base == 0) t_prof.t0 = now_us();
  c = thread_ctx(device, &rc);
  if (!c) return rc;
  nq = nq_, mode = mode_, with_desc = with_desc_, base = arena_base;
  const size_t Q = (size_t)(nq > 0 ? nq : 1);
  if (t_cap_hint < 4) t_cap_hint = 4;
  cap = mode == kWinList ? (int)(Q * (size_t)t_cap_hint) : 0;  // entries of the overflow area behind the inline slots
  Stage st;
  oQ = st.add(Q * sizeof(WinQuery));
  oD = st.add(with_desc ? Q * 32 : 0);
  const bool lists_here = mode == kWinList && !dev_lists;
  oOff = st.add(lists_here ? Q * 4 : 0);
  oCnt = st.add(lists_here ? Q * 4 : 0);
  oOut = st.add(out_bytes());
  return ctx_reserve(c, base + st.total + arena_extra, 0);
}

WindowCall::~WindowCall() {
  if (range_open) range_pop();  // an error return between begin() and finish()
}

// bytes of the candidate array (list mode; none with dev_lists) or of the {idx, dist} pairs (best mode) in the pinned arena
size_t WindowCall::out_bytes() const {
  const size_t Q = (size_t)(nq > 0 ? nq : 1);
  return mode == kWinList ? (dev_lists ? 0 : (Q * kInline + (size_t)cap) * 4) : Q * 8;
}

size_t WindowCall::bytes() const { return oOut + ((out_bytes() + 63) & ~(size_t)63); }

int WindowCall::launch(const vsg_frame *f, int gate_mode, int best_init, const float *inv_sigma2, int nlevels,
                       const uint8_t *qdesc_dev, const WinQuery *q_dev) {
  const double tl = now_us();
  if (base == 0) t_prof.fill = tl - t_prof.t0;
  if (nq <= 0) return VSG_OK;
  WinLaunch W;
  W.nq = nq, W.mode = mode, W.gate_mode = gate_mode, W.best_init = best_init, W.cap = cap;
  W.counter_base = c->counter_base;
  for (int l = 0; l < 16; l++) W.inv_sigma2[l] = (inv_sigma2 && l < nlevels) ? inv_sigma2[l] : 0.f;
  uint8_t *d = c->d_pin + base;
  hipLaunchKernelGGL(k_window_search, dim3((nq + 3) / 4), dim3(256), 0, c->stream, frame_dev(f),
                     q_dev ? q_dev : (const WinQuery *)(d + oQ),
                     qdesc_dev ? qdesc_dev : with_desc ? (const uint8_t *)(d + oD) : (const uint8_t *)nullptr, W,
                     x_out ? x_off : (int *)(d + oOff), x_out ? x_cnt : (int *)(d + oCnt),
                     x_out ? x_out : (uint32_t *)(d + oOut), (int *)(d + oOut), c->d_counter);
  t_prof.launch = now_us() - tl;
  return hipGetLastError() == hipSuccess ? VSG_OK : VSG_ERR_HIP;
}

int WindowCall::finish() {
  const double ts = now_us();
  if (nq > 0 && hipStreamSynchronize(c->stream) != hipSuccess) return VSG_ERR_HIP;
  t_prof.sync = now_us() - ts;
  if (range_open) range_pop(), range_open = false;
  if (mode != kWinList) return VSG_OK;
  const int32_t *cn = (const int32_t *)(c->h_pin + base + oCnt);
  long long total = 0;  // entries of the lists that went to the overflow area = what the waves added to the counter
  for (int q = 0; q < nq; q++) total += cn[q] > kInline ? cn[q] : 0;
  return account(total);
}

int WindowCall::account(long long total) {
  if (range_open) range_pop(), range_open = false;
  c->counter_base += (uint32_t)total;
  if (total <= cap) return VSG_OK;
  const long long per = (2 * total + nq - 1) / (nq > 0 ? nq : 1);
  t_cap_hint = (int)(per > t_cap_hint ? per : 2 * t_cap_hint);  // sticky: room for windows like these from now on
  return VSG_RETRY;
}

void window_call_done() { t_prof.total = now_us() - t_prof.t0; }

walk::CandView WindowCall::lists() const {
  walk::CandView cv;
  cv.ent = (const uint32_t *)(c->h_pin + base + oOut);
  cv.off = (const int32_t *)(c->h_pin + base + oOff);
  cv.cnt = (const int32_t *)(c->h_pin + base + oCnt);
  return cv;
}

}  // namespace vsg

// queries and descriptors of the routines that search a KeyFrame's area (win_keyframe_area; ur == nullptr: 0)
static void fill_keyframe_area(const WindowCall &wc, int nq, const uint8_t *desc, const float *u, const float *v,
                               const float *ur, const float *radius, const int32_t *level, bool right) {
  WinQuery *Q = wc.queries();
  for (int i = 0; i < nq; i++) Q[i] = win_keyframe_area(u[i], v[i], radius[i], level[i], ur ? ur[i] : 0.f, right);
  if (nq) memcpy(wc.desc(), desc, (size_t)nq * 32);
}

extern "C" {

// debug: wall time (microseconds) of the calling thread's last windowed search: filling the pinned arena, the kernel
// launch call, the wait for completion (= kernel + PCIe), and the whole entry point (the rest is the ordered host pass)
int vsg_debug_call_profile(float us[4]) {
  if (!us) return VSG_ERR_INVALID;
  us[0] = (float)t_prof.fill, us[1] = (float)t_prof.launch, us[2] = (float)t_prof.sync, us[3] = (float)t_prof.total;
  return VSG_OK;
}

int vsg_grid_query(vsg_grid *g, const float *x, const float *y, const float *r, const int32_t *min_level,
                   const int32_t *max_level, int nq, int32_t *cand_off, int32_t *cand_idx, int cap) {
  // A grid's block has no keypoint, descriptor or mvuRight arrays (FrameLayout's grid_only: those pointers alias the
  // cell table).  This call never reads them: list mode, no query descriptors, kGateNone, left grid.  A search that
  // does must not be pointed at a grid.
  return vsg_frame_features_in_area(grid_frame(g), x, y, r, min_level, max_level, 0, nq, cand_off, cand_idx, cap);
}

int vsg_frame_features_in_area(vsg_frame *f, const float *x, const float *y, const float *r, const int32_t *min_level,
                               const int32_t *max_level, int right, int nq, int32_t *cand_off, int32_t *cand_idx,
                               int cap) {
  if (frame_check(f) != VSG_OK || !x || !y || !r || !cand_off || nq < 0 || cap < 0) return VSG_ERR_INVALID;
  cand_off[0] = 0;
  if (nq == 0) return 0;
  return with_retry([&]() -> int {
    WindowCall wc;
    int rc = wc.begin(f->device, nq, kWinList, false);
    if (rc != VSG_OK) return rc;
    WinQuery *Q = wc.queries();
    for (int q = 0; q < nq; q++)
      Q[q] = win_area(x[q], y[q], r[q], min_level ? min_level[q] : -1, max_level ? max_level[q] : -1, right != 0);
    rc = wc.run(f, kGateNone);
    if (rc != VSG_OK) return rc;
    const walk::CandView cv = wc.lists();
    int total = 0;
    for (int q = 0; q < nq; q++) {
      const int n = cv.size(q);
      const uint32_t *e = cv.begin(q);
      for (int k = 0; k < n; k++, total++)
        if (cand_idx && total < cap) cand_idx[total] = walk::ent_idx(e[k]);
      cand_off[q + 1] = total;
    }
    return total;
  });
}

int vsg_frame_search_by_projection(vsg_frame *F, int n_mp, const uint8_t *mp_desc, const uint8_t *mp_observed,
                                   const uint8_t *in_view, const float *proj_x, const float *proj_y,
                                   const float *proj_xr, const int32_t *scale_level, const float *view_cos,
                                   const uint8_t *in_view_r, const float *proj_x_r, const float *proj_y_r,
                                   const int32_t *scale_level_r, const float *view_cos_r, float th, float nnratio,
                                   const float *scale_factors, int nlevels, const int32_t *left_to_right,
                                   const int32_t *right_to_left, uint8_t *train_blocked, int32_t *train_match) {
  if (frame_check(F) != VSG_OK || n_mp < 0 || !train_blocked || !train_match || !scale_factors || nlevels < 1)
    return VSG_ERR_INVALID;
  if (n_mp == 0) return 0;
  if (!mp_desc || !in_view || !proj_x || !proj_y || !scale_level || !view_cos) return VSG_ERR_INVALID;
  const bool stereo2 = F->nleft != -1;
  if (stereo2 && in_view_r && (!proj_x_r || !proj_y_r || !scale_level_r || !view_cos_r)) return VSG_ERR_INVALID;
  const bool bFactor = th != 1.0;  // :46
  return with_retry([&]() -> int {
    const int nq = stereo2 ? 2 * n_mp : n_mp;
    WindowCall wc;
    int rc = wc.begin(F->device, nq, kWinList, true);
    if (rc != VSG_OK) return rc;
    WinQuery *Q = wc.queries();
    uint8_t *D = wc.desc();
    for (int i = 0; i < n_mp; i++) {
      WinQuery w = win_inactive(false);
      if (in_view[i]) {
        const int lvl = scale_level[i];
        if (lvl < 0 || lvl >= nlevels) return VSG_ERR_INVALID;
        w = win_local(proj_x[i], proj_y[i], proj_xr ? proj_xr[i] : 0.f, lvl, view_cos[i], th, bFactor, scale_factors);
      }
      Q[i] = w;
      memcpy(D + (size_t)i * 32, mp_desc + (size_t)i * 32, 32);
      if (stereo2) {
        WinQuery wr = win_inactive(true);
        if (in_view_r && in_view_r[i] && scale_level_r[i] != -1) {
          const int lvl = scale_level_r[i];
          if (lvl < 0 || lvl >= nlevels) return VSG_ERR_INVALID;
          wr = win_local_right(proj_x_r[i], proj_y_r[i], lvl, view_cos_r[i], scale_factors);
        }
        Q[n_mp + i] = wr;
        memcpy(D + (size_t)(n_mp + i) * 32, mp_desc + (size_t)i * 32, 32);
      }
    }
    // the stereo gate of :97-102 applies to F.Nleft == -1 frames with mvuRight
    rc = wc.run(F, (!stereo2 && F->has_uright && proj_xr) ? kGateUr : kGateNone);
    if (rc != VSG_OK) return rc;
    return walk::search_local(wc.lists(), n_mp, F->nleft, in_view, in_view_r, scale_level_r, mp_observed, nnratio,
                              left_to_right, right_to_left, train_blocked, train_match);
  });
}

int vsg_frame_search_by_projection_last(vsg_frame *cur, int n_q, const uint8_t *mp_desc, const uint8_t *mp_observed,
                                        const float *u, const float *v, const float *ur, const float *u_r,
                                        const float *v_r, const int32_t *last_octave, const float *last_angle,
                                        float th, int direction, const float *scale_factors, int nlevels,
                                        int check_orientation, uint8_t *train_blocked, int32_t *train_match) {
  if (frame_check(cur) != VSG_OK || n_q < 0 || !train_blocked || !train_match || !scale_factors || nlevels < 1 ||
      direction < 0 || direction > 2)
    return VSG_ERR_INVALID;
  if (n_q == 0) return 0;
  if (!mp_desc || !u || !v || !last_octave || (check_orientation && !last_angle)) return VSG_ERR_INVALID;
  const bool stereo2 = cur->nleft != -1;
  if (stereo2 && (!u_r || !v_r)) return VSG_ERR_INVALID;
  return with_retry([&]() -> int {
    const int nq = stereo2 ? 2 * n_q : n_q;
    WindowCall wc;
    int rc = wc.begin(cur->device, nq, kWinList, true);
    if (rc != VSG_OK) return rc;
    WinQuery *Q = wc.queries();
    uint8_t *D = wc.desc();
    for (int i = 0; i < n_q; i++) {
      const int oct = last_octave[i];
      if (oct < 0 || oct >= nlevels) return VSG_ERR_INVALID;
      Q[i] = win_last(u[i], v[i], ur ? ur[i] : 0.f, oct, th, direction, scale_factors);
      memcpy(D + (size_t)i * 32, mp_desc + (size_t)i * 32, 32);
      if (stereo2) {
        Q[n_q + i] = win_last_area(u_r[i], v_r[i], oct, th, direction, scale_factors, true);
        memcpy(D + (size_t)(n_q + i) * 32, mp_desc + (size_t)i * 32, 32);
      }
    }
    rc = wc.run(cur, (!stereo2 && cur->has_uright && ur) ? kGateUr : kGateNone);
    if (rc != VSG_OK) return rc;
    const vsg_keypoint *hk = cur->h_kps.data();
    return walk::search_last(wc.lists(), n_q, cur->nleft, last_angle, mp_observed, [&](int i) { return hk[i].angle; },
                             walk::TH_HIGH, check_orientation != 0, train_blocked, train_match);
  });
}

int vsg_frame_search_by_projection_sim3(vsg_frame *kf, int n_q, const uint8_t *mp_desc, const float *u, const float *v,
                                        const float *radius, const int32_t *predicted_level, float ratio_hamming,
                                        int32_t *matched) {
  if (frame_check(kf) != VSG_OK || n_q < 0 || !matched) return VSG_ERR_INVALID;
  if (n_q == 0) return 0;
  if (!mp_desc || !u || !v || !radius || !predicted_level) return VSG_ERR_INVALID;
  return with_retry([&]() -> int {
    WindowCall wc;
    int rc = wc.begin(kf->device, n_q, kWinList, true);
    if (rc != VSG_OK) return rc;
    fill_keyframe_area(wc, n_q, mp_desc, u, v, nullptr, radius, predicted_level, false);
    rc = wc.run(kf, kGateNone);
    if (rc != VSG_OK) return rc;
    return walk::search_sim3_projection(wc.lists(), n_q, ratio_hamming, matched);
  });
}

int vsg_frame_search_by_projection_kf(vsg_frame *cur, int n_q, const uint8_t *mp_desc, const float *u, const float *v,
                                      const float *radius, const int32_t *predicted_level, const float *kf_angle,
                                      int orb_dist, int check_orientation, uint8_t *occupied, int32_t *train_match) {
  if (frame_check(cur) != VSG_OK || n_q < 0 || !occupied || !train_match) return VSG_ERR_INVALID;
  if (n_q == 0) return 0;
  if (!mp_desc || !u || !v || !radius || !predicted_level || (check_orientation && !kf_angle)) return VSG_ERR_INVALID;
  return with_retry([&]() -> int {
    WindowCall wc;
    int rc = wc.begin(cur->device, n_q, kWinList, true);
    if (rc != VSG_OK) return rc;
    WinQuery *Q = wc.queries();
    for (int i = 0; i < n_q; i++) Q[i] = win_kf(u[i], v[i], radius[i], predicted_level[i]);
    memcpy(wc.desc(), mp_desc, (size_t)n_q * 32);
    rc = wc.run(cur, kGateNone);
    if (rc != VSG_OK) return rc;
    const vsg_keypoint *hk = cur->h_kps.data();
    return walk::search_kf_projection(wc.lists(), n_q, kf_angle, [&](int i) { return hk[i].angle; }, orb_dist,
                                      check_orientation != 0, occupied, train_match);
  });
}

int vsg_frame_search_by_sim3(vsg_frame *kf1, vsg_frame *kf2, int nq1, const int32_t *idx1, const uint8_t *desc1,
                             const float *u1, const float *v1, const float *radius1, const int32_t *level1, int nq2,
                             const int32_t *idx2, const uint8_t *desc2, const float *u2, const float *v2,
                             const float *radius2, const int32_t *level2, int32_t *matches12) {
  if (frame_check(kf1) != VSG_OK || frame_check(kf2) != VSG_OK || kf1->device != kf2->device || nq1 < 0 || nq2 < 0 ||
      !matches12)
    return VSG_ERR_INVALID;
  if ((nq1 > 0 && (!idx1 || !desc1 || !u1 || !v1 || !radius1 || !level1)) ||
      (nq2 > 0 && (!idx2 || !desc2 || !u2 || !v2 || !radius2 || !level2)))
    return VSG_ERR_INVALID;
  const int N1 = kf1->n, N2 = kf2->n;
  for (int i = 0; i < N1; i++) matches12[i] = -1;
  // both directions in one arena, two launches, one sync
  WindowCall a, b;
  int rc = a.begin(kf1->device, nq1, kWinBest, true, 0, 0);
  if (rc != VSG_OK) return rc;
  const size_t abytes = a.bytes();
  rc = b.begin(kf1->device, nq2, kWinBest, true, abytes, 0);
  if (rc != VSG_OK) return rc;
  a.c = b.c;  // b.begin may have grown (= re-allocated) the arena: a has not written anything yet
  fill_keyframe_area(a, nq1, desc1, u1, v1, nullptr, radius1, level1, false);  // KF1's points searched in KF2
  fill_keyframe_area(b, nq2, desc2, u2, v2, nullptr, radius2, level2, false);  // KF2's points searched in KF1
  rc = a.launch(kf2, kGateNone, 0x7FFFFFFF, nullptr, 0);
  if (rc == VSG_OK) rc = b.launch(kf1, kGateNone, 0x7FFFFFFF, nullptr, 0);
  if (rc != VSG_OK) return rc;
  rc = a.finish();  // one of the two directions may be empty: each waits for the stream it launched on
  if (rc == VSG_OK) rc = b.finish();
  if (rc != VSG_OK) return rc;
  std::vector<int> vnMatch1((size_t)N1, -1), vnMatch2((size_t)N2, -1);
  const int32_t *ba = a.best(), *bb = b.best();
  for (int k = 0; k < nq1; k++) {
    if (idx1[k] < 0 || idx1[k] >= N1) return VSG_ERR_INVALID;
    if (ba[2 * k] >= 0 && ba[2 * k + 1] <= walk::TH_HIGH) vnMatch1[idx1[k]] = ba[2 * k];  // :1562-1565
  }
  for (int k = 0; k < nq2; k++) {
    if (idx2[k] < 0 || idx2[k] >= N2) return VSG_ERR_INVALID;
    if (bb[2 * k] >= 0 && bb[2 * k + 1] <= walk::TH_HIGH) vnMatch2[idx2[k]] = bb[2 * k];  // :1640-1643
  }
  int nFound = 0;  // agreement (:1646-1662)
  for (int i1 = 0; i1 < N1; i1++) {
    const int i2 = vnMatch1[i1];
    if (i2 >= 0 && i2 < N2 && vnMatch2[i2] == i1) {
      matches12[i1] = i2;
      nFound++;
    }
  }
  return nFound;
}

static int fuse_search(vsg_frame *kf, int n_q, const uint8_t *mp_desc, const float *u, const float *v, const float *ur,
                       const float *radius, const int32_t *predicted_level, int right, int gate, int init,
                       const float *inv_level_sigma2, int nlevels, int32_t *best_idx, int32_t *best_dist) {
  if (frame_check(kf) != VSG_OK || n_q < 0 || !best_idx || !best_dist) return VSG_ERR_INVALID;
  if (n_q == 0) return 0;
  if (!mp_desc || !u || !v || !radius || !predicted_level) return VSG_ERR_INVALID;
  if (gate == kGateChi2 && (!ur || !inv_level_sigma2 || nlevels < 1 || nlevels > 16)) return VSG_ERR_INVALID;
  if (right && kf->nleft == -1) return VSG_ERR_INVALID;
  WindowCall wc;
  int rc = wc.begin(kf->device, n_q, kWinBest, true);
  if (rc != VSG_OK) return rc;
  fill_keyframe_area(wc, n_q, mp_desc, u, v, ur, radius, predicted_level, right != 0);
  rc = wc.run(kf, gate, init, inv_level_sigma2, nlevels);
  return rc != VSG_OK ? rc : wc.best_out(init, best_idx, best_dist);
}

int vsg_frame_fuse(vsg_frame *kf, int n_q, const uint8_t *mp_desc, const float *u, const float *v, const float *ur,
                   const float *radius, const int32_t *predicted_level, int right, const float *inv_level_sigma2,
                   int nlevels, int32_t *best_idx, int32_t *best_dist) {
  return fuse_search(kf, n_q, mp_desc, u, v, ur, radius, predicted_level, right, kGateChi2, 256, inv_level_sigma2,
                     nlevels, best_idx, best_dist);
}

int vsg_frame_fuse_sim3(vsg_frame *kf, int n_q, const uint8_t *mp_desc, const float *u, const float *v,
                        const float *radius, const int32_t *predicted_level, int32_t *best_idx, int32_t *best_dist) {
  return fuse_search(kf, n_q, mp_desc, u, v, nullptr, radius, predicted_level, 0, kGateNone, 0x7FFFFFFF, nullptr, 0,
                     best_idx, best_dist);
}

int vsg_fuse_decide(int n_q, const int32_t *query_mp, const int32_t *best_idx, const int32_t *best_dist, int sim3_form,
                    int32_t *slot_mp, int n_slots, int32_t *mp_obs, uint8_t *mp_bad, int n_mp, int32_t *action,
                    int32_t *other_mp) {
  if (n_q < 0 || !query_mp || !best_idx || !best_dist || !slot_mp || !mp_obs || !mp_bad || !action) return VSG_ERR_INVALID;
  int nFused = 0;
  for (int k = 0; k < n_q; k++) {
    action[k] = 0;
    if (other_mp) other_mp[k] = -1;
    const int idx = best_idx[k], pMP = query_mp[k];
    if (idx < 0 || best_dist[k] > walk::TH_LOW) continue;  // :1308 / :1429
    if (idx >= n_slots || pMP < 0 || pMP >= n_mp) return VSG_ERR_INVALID;
    const int pMPinKF = slot_mp[idx];  // pKF->GetMapPoint(bestIdx)
    if (pMPinKF >= 0) {
      if (pMPinKF >= n_mp) return VSG_ERR_INVALID;
      if (other_mp) other_mp[k] = pMPinKF;
      if (!mp_bad[pMPinKF]) {
        if (sim3_form) {
          action[k] = 5;  // vpReplacePoint[iMP] = pMPinKF (:1436)
        } else if (mp_obs[pMPinKF] > mp_obs[pMP]) {
          action[k] = 2;  // pMP->Replace(pMPinKF) (:1315): pMP turns bad, its observations move over
          mp_obs[pMPinKF] += mp_obs[pMP];
          mp_bad[pMP] = 1;
        } else {
          action[k] = 3;  // pMPinKF->Replace(pMP) (:1317): the slot now holds pMP
          mp_obs[pMP] += mp_obs[pMPinKF];
          mp_bad[pMPinKF] = 1;
          slot_mp[idx] = pMP;
        }
      } else {
        action[k] = 4;
      }
    } else {
      action[k] = 1;  // pMP->AddObservation(pKF, bestIdx); pKF->AddMapPoint(pMP, bestIdx) (:1321-1322 / :1440-1441)
      slot_mp[idx] = pMP;
      mp_obs[pMP] += 1;
    }
    nFused++;
  }
  return nFused;
}

int vsg_frame_search_for_initialization(vsg_frame *f1, vsg_frame *f2, const float *prev_x, const float *prev_y,
                                        int window_size, float nnratio, int check_orientation, int32_t *matches12) {
  if (frame_check(f1) != VSG_OK || frame_check(f2) != VSG_OK || f1->device != f2->device || !matches12 || !prev_x ||
      !prev_y)
    return VSG_ERR_INVALID;
  const int n1 = f1->n, n2 = f2->n;
  for (int i = 0; i < n1; i++) matches12[i] = -1;
  if (n1 == 0 || n2 == 0) return 0;
  return with_retry([&]() -> int {
    WindowCall wc;
    int rc = wc.begin(f1->device, n1, kWinList, false);
    if (rc != VSG_OK) return rc;
    WinQuery *Q = wc.queries();
    const vsg_keypoint *k1 = f1->h_kps.data(), *k2 = f2->h_kps.data();
    for (int i = 0; i < n1; i++) {
      // level1 > 0 -> continue (:659-661); F2.GetFeaturesInArea(vbPrevMatched[i1].x, .y, windowSize, level1, level1) (:663)
      const int level1 = k1[i].octave;
      Q[i] = win_area(prev_x[i], prev_y[i], (float)window_size, level1, level1, false, level1 > 0);
    }
    // F1's descriptors are resident: the kernel reads the query descriptors where they are
    rc = wc.run(f2, kGateNone, 256, nullptr, 0, f1->d_desc);
    if (rc != VSG_OK) return rc;
    return walk::search_initialization(wc.lists(), n1, n2, nullptr, [&](int i) { return k1[i].angle; },
                                       [&](int i) { return k2[i].angle; }, nnratio, check_orientation != 0, matches12);
  });
}

}  // extern "C"
