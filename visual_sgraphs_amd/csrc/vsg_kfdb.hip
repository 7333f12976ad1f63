// vsg_kfdb.hip -- TemplatedVocabulary::score and a device-resident KeyFrameDatabase (after N2).
//   orb_slam3/Thirdparty/DBoW2/DBoW2/ScoringObject.cpp  L1 / L2 / ChiSquare / KL / Bhattacharyya / DotProduct
//   orb_slam3/Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1214-1219  score()
//   orb_slam3/src/KeyFrameDatabase.cc:31-96 (add / erase / clear / clearMap), :592-717 (DetectNBestCandidates),
//   :719-830 (DetectRelocalizationCandidates)
//
// Storage: a SLOT STORE.  Every add() appends one slot = the keyframe's BowVector (ascending word ids, values) to two
// device arrays that only grow (amortised 1.5x); its position in the store is the add sequence.  A word's posting list in
// the reference is "the live entries of that word, in add order", so the store IS the inverted file read sideways: a live
// entry of word w in slot s is the entry (kf of s, position = rank of s among the live slots holding w).  erase() removes
// the first live entry of the keyframe in each list of its BowVector (a per-entry tombstone: bit 31 of the word id), a
// slot whose entries are all gone is flagged dead, clear() / clearMap() drop slots.
//
// Query = one enqueue, ONE wait:
//   k_kfdb_count   dense scan of the live slots, one wavefront per slot: each entry's word is looked up in the query
//                  (LDS, binary search); per keyframe a word count (atomicAdd) and a 64-bit first-encounter key
//                  (rank of the query word << 32 | add sequence, atomicMin) -- the order of lKFsSharingWords
//   k_kfdb_words   the per-keyframe query state (mnRelocQuery / mnRelocWords, mnPlaceRecognition*) exactly as the walk
//                  leaves it; maxCommonWords by atomicMax over the keyframes that enter the list
//   k_kfdb_select  keyframes with more than (int)(maxCommonWords * 0.8f) words, compacted (unordered: see below)
//   k_kfdb_score   one wavefront per candidate: the merge-join of the two BowVectors, every shared word's term computed
//                  on its own lane, the sum ONE chain in ascending word id on lane 0 (no tree: that changes the bits);
//                  (float) si stored as mRelocScore / mPlaceRecognitionScore
//   k_kfdb_covis   one thread per candidate: accScore over GetBestCovisibilityKeyFrames(10) in neighbour order (float),
//                  best keyframe by strict '>' -- written straight to pinned host memory
// Host, after the wait: the candidates are sorted by their unique first-encounter keys (= the reference's list order:
// a few hundred keys, microseconds), then the short tail (0.75 * bestAccScore filter + map filter + dedupe, or the stable
// sort by accScore and the loop / merge split).  The state of every keyframe id ever seen persists across queries,
// erase, re-add and clear, as the KeyFrame members do.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "../../include/vsg_orb.h"
#include "../../include/vsg_orb_debug.h"
#include "vsg_ctx.h"
#include "vsg_frame_int.h"

namespace {
enum { kCov = 10, kMaxQueryWords = 12288 };  // GetBestCovisibilityKeyFrames(10); query ids in LDS (48 KB)
constexpr int kTomb = (int)0x80000000u;      // tombstone bit of an entry's word id

// the six KeyFrame members the queries read and write (KeyFrame.h; mRelocScore is never initialised in the reference: 0)
struct KfState {
  unsigned long long rq, pq;  // mnRelocQuery, mnPlaceRecognitionQuery
  int rw, pw;                 // mnRelocWords, mnPlaceRecognitionWords
  float rs, ps;               // mRelocScore, mPlaceRecognitionScore
};
static_assert(sizeof(KfState) == 32, "KfState layout");

struct CandRec {  // one entry of lAccScoreAndMatch, with the key that orders it
  unsigned long long key;
  float acc;
  int best;
};
static_assert(sizeof(CandRec) == 16, "CandRec layout");

// position of w in the ascending q[0..n), or -1
__device__ __forceinline__ int find_rank(const int *q, int n, int w) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (q[mid] < w) lo = mid + 1;
    else hi = mid;
  }
  return (lo < n && q[lo] == w) ? lo : -1;
}

__device__ __forceinline__ void load_query(int *q, const int *__restrict__ g, int n) {
  for (int i = threadIdx.x; i < n; i += blockDim.x) q[i] = g[i];
  __syncthreads();
}

// ScoringObject.cpp: score(v1 = query, v2 = the other BowVector) for one wavefront.  The merge loop visits the shared word
// ids in ascending order and adds one term each; the terms are independent, so each lane computes the term of its own
// entry, the terms of a 64-entry chunk are compacted in order into `buf` and lane 0 adds them to the running sum one
// after the other -- the reference's single chain of double additions (-ffp-contract=off: no FMA).  Result on lane 0.
__device__ double score_chain(const int *q, const double *__restrict__ qv, int nq, const int *__restrict__ wid,
                              const double *__restrict__ wv, int len, int scoring, double *buf) {
  const int lane = threadIdx.x & 63;
  double s = 0.0;
  for (int base = 0; base < len; base += 64) {
    const int j = base + lane;
    bool has = false;
    double t = 0.0;
    if (j < len) {
      const int r = find_rank(q, nq, wid[j] & ~kTomb);  // the BowVector itself: tombstones do not matter here
      if (r >= 0) {
        const double vi = qv[r], wi = wv[j];
        if (scoring == 0) {  // L1
          t = fabs(vi - wi) - fabs(vi) - fabs(wi), has = true;
        } else if (scoring == 1 || scoring == 5) {  // L2, DotProduct
          t = vi * wi, has = true;
        } else if (scoring == 2) {  // ChiSquare
          has = vi + wi != 0.0;
          if (has) t = vi * wi / (vi + wi);
        } else if (scoring == 4) {  // Bhattacharyya
          t = sqrt(vi * wi), has = true;
        }
      }
    }
    const unsigned long long m = __ballot(has);
    if (has) buf[__popcll(m & ((1ull << lane) - 1))] = t;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) {
      const int nm = __popcll(m);
      for (int k = 0; k < nm; k++) s += buf[k];
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  if (scoring == 0) s = -s / 2.0;
  else if (scoring == 1) s = s >= 1 ? 1.0 : 1.0 - sqrt(1.0 - s);  // the clamp of ScoringObject.cpp:114-117
  else if (scoring == 2) s = 2. * s;
  return s;
}

// vsg_vocab_score: item c = entries [off[c], off[c+1]) of (ids, vals)
__global__ __launch_bounds__(256) void k_vocab_score(const int *__restrict__ q_ids, const double *__restrict__ q_vals,
                                                     int nq, int scoring, const int *__restrict__ off,
                                                     const int *__restrict__ ids, const double *__restrict__ vals, int m,
                                                     double *__restrict__ out) {
  extern __shared__ int q[];
  __shared__ double buf[4][64];
  load_query(q, q_ids, nq);
  const int w = threadIdx.x >> 6;
  for (int c = blockIdx.x * 4 + w; c < m; c += gridDim.x * 4) {
    const int a = off[c];
    const double s = score_chain(q, q_vals, nq, ids + a, vals + a, off[c + 1] - a, scoring, buf[w]);
    if ((threadIdx.x & 63) == 0) out[c] = s;
  }
}

__global__ __launch_bounds__(256) void k_kfdb_count(const int *__restrict__ q_ids, int nq,
                                                    const uint32_t *__restrict__ slot_off, const int *__restrict__ slot_len,
                                                    const int *__restrict__ slot_kf, const uint8_t *__restrict__ slot_dead,
                                                    int n_slots, const int *__restrict__ ent_word, int *__restrict__ cnt,
                                                    unsigned long long *__restrict__ key) {
  extern __shared__ int q[];
  load_query(q, q_ids, nq);
  const int lane = threadIdx.x & 63;
  for (int s = blockIdx.x * 4 + (threadIdx.x >> 6); s < n_slots; s += gridDim.x * 4) {
    if (slot_dead[s]) continue;  // wave-uniform
    const uint32_t off = slot_off[s];
    const int len = slot_len[s];
    int c = 0, rmin = 0x7FFFFFFF;
    for (int j = lane; j < len; j += 64) {
      const int w = ent_word[off + j];
      if (w < 0) continue;  // tombstone: erased from this word's list
      const int r = find_rank(q, nq, w);
      if (r >= 0) c++, rmin = min(rmin, r);
    }
#pragma unroll
    for (int d = 32; d; d >>= 1) c += __shfl_xor(c, d), rmin = min(rmin, __shfl_xor(rmin, d));
    if (lane == 0 && c) {
      const int kf = slot_kf[s];
      atomicAdd(&cnt[kf], c);
      atomicMin(&key[kf], ((unsigned long long)rmin << 32) | (uint32_t)s);
    }
  }
}

// The state the walk of :607-627 / :728-742 leaves behind, per keyframe that shares words (cnt > 0).  Relocalisation:
// a keyframe enters lKFsSharingWords iff mnRelocQuery != query id; then its words restart from 0.  N-best: a connected
// keyframe has its words reset at every visit but never takes the query id (words end at 1).  Keyframes that do not
// enter the list get key = ~0.
__global__ __launch_bounds__(256) void k_kfdb_words(int nidx, int kind, unsigned long long qid,
                                                    const int *__restrict__ conn, int nconn, const int *__restrict__ cnt,
                                                    unsigned long long *__restrict__ key, KfState *__restrict__ st,
                                                    int *__restrict__ ctrl) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nidx) return;
  const int c = cnt[i];
  if (!c) return;
  KfState s = st[i];
  bool in_list;
  if (kind == 0) {
    in_list = s.rq != qid;
    s.rw = in_list ? c : s.rw + c;
    s.rq = qid;
  } else {
    bool connected = false;
    for (int j = 0; j < nconn; j++) connected |= conn[j] == i;
    if (s.pq != qid) {
      in_list = !connected;
      s.pw = connected ? 1 : c;
      if (!connected) s.pq = qid;
    } else {
      in_list = false;
      s.pw += c;
    }
  }
  st[i] = s;
  if (in_list) atomicMax(&ctrl[0], c);
  else key[i] = ~0ull;
}

__global__ __launch_bounds__(256) void k_kfdb_select(int nidx, const int *__restrict__ cnt,
                                                     const unsigned long long *__restrict__ key, int *__restrict__ ctrl,
                                                     int *__restrict__ cand) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nidx) return;
  const int c = cnt[i];
  if (!c || key[i] == ~0ull) return;
  const int minw = (int)((float)ctrl[0] * 0.8f);  // int minCommonWords = maxCommonWords * 0.8f
  if (c > minw) cand[atomicAdd(&ctrl[1], 1)] = i;
}

__global__ __launch_bounds__(256) void k_kfdb_score(const int *__restrict__ q_ids, const double *__restrict__ q_vals,
                                                    int nq, int scoring, int kind, const int *__restrict__ ctrl,
                                                    const int *__restrict__ cand, const int *__restrict__ kf_bow,
                                                    const uint32_t *__restrict__ slot_off, const int *__restrict__ slot_len,
                                                    const int *__restrict__ ent_word, const double *__restrict__ ent_val,
                                                    KfState *__restrict__ st) {
  extern __shared__ int q[];
  __shared__ double buf[4][64];
  load_query(q, q_ids, nq);
  const int w = threadIdx.x >> 6, ncand = ctrl[1];
  for (int c = blockIdx.x * 4 + w; c < ncand; c += gridDim.x * 4) {
    const int i = cand[c], slot = kf_bow[i];
    const uint32_t off = slot_off[slot];
    const double s = score_chain(q, q_vals, nq, ent_word + off, ent_val + off, slot_len[slot], scoring, buf[w]);
    if ((threadIdx.x & 63) == 0) {
      if (kind == 0) st[i].rs = (float)s;
      else st[i].ps = (float)s;
    }
  }
}

__global__ __launch_bounds__(256) void k_kfdb_covis(int kind, unsigned long long qid, const int *__restrict__ ctrl,
                                                    const int *__restrict__ cand, const unsigned long long *__restrict__ key,
                                                    const int *__restrict__ cov, const KfState *__restrict__ st,
                                                    int *__restrict__ out_hdr, CandRec *__restrict__ out) {
  const int c = blockIdx.x * 256 + threadIdx.x, ncand = ctrl[1];
  if (c == 0) out_hdr[0] = ncand;
  if (c >= ncand) return;
  const int i = cand[c];
  const float si = kind == 0 ? st[i].rs : st[i].ps;
  float acc = si, bs = si;
  int best = i;
  for (int k = 0; k < kCov; k++) {
    const int nb = cov[i * kCov + k];
    if (nb < 0) break;
    const KfState t = st[nb];
    if ((kind == 0 ? t.rq : t.pq) != qid) continue;
    const float sc = kind == 0 ? t.rs : t.ps;
    acc += sc;
    if (sc > bs) best = nb, bs = sc;
  }
  CandRec r;
  r.key = key[i], r.acc = acc, r.best = best;
  out[c] = r;
}

__global__ __launch_bounds__(256) void k_kfdb_new_slot(uint32_t *slot_off, int *slot_len, int *slot_kf,
                                                       uint8_t *slot_dead, int *kf_bow, int slot, uint32_t off, int len,
                                                       int kf) {
  if (threadIdx.x == 0) slot_off[slot] = off, slot_len[slot] = len, slot_kf[slot] = kf, slot_dead[slot] = 0, kf_bow[kf] = slot;
}

__global__ __launch_bounds__(256) void k_kfdb_mark(const uint32_t *__restrict__ tomb, int nt, int *__restrict__ ent_word,
                                                   const int *__restrict__ dead, int nd, uint8_t *__restrict__ slot_dead) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < nt) ent_word[tomb[i]] |= kTomb;
  if (i < nd) slot_dead[dead[i]] = 1;
}

// rows of 1 + kCov ints: keyframe index, then its neighbours (-1 padded)
__global__ __launch_bounds__(256) void k_kfdb_set_cov(const int *__restrict__ rows, int n, int *__restrict__ cov) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int *r = rows + (size_t)i * (kCov + 1);
  for (int k = 0; k < kCov; k++) cov[r[0] * kCov + k] = r[1 + k];
}

int grid_for(long items_per_block_4waves, long cap) {
  const long g = (items_per_block_4waves + 3) / 4;
  return (int)std::max(1L, std::min(g, cap));
}

// a device array that grows by 1.5x: the first `used` elements are kept, the new tail is filled with `fill` bytes
template <class T>
int grow(T **p, size_t *cap, size_t need, size_t used, int fill, hipStream_t st) {
  if (need <= *cap) return VSG_OK;
  size_t nc = std::max(need, std::max(*cap + *cap / 2, (size_t)1024));
  T *np = nullptr;
  TRY_HIP(hipMalloc((void **)&np, nc * sizeof(T)));
  hipError_t e = hipSuccess;
  if (used) e = hipMemcpyAsync(np, *p, used * sizeof(T), hipMemcpyDeviceToDevice, st);
  if (e == hipSuccess) e = hipMemsetAsync(np + used, fill, (nc - used) * sizeof(T), st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) {
    hipFree(np);
    return VSG_ERR_HIP;
  }
  if (*p) hipFree(*p);
  *p = np, *cap = nc;
  return VSG_OK;
}

bool ascending_words(const int32_t *ids, int n, int nwords) {
  for (int i = 0; i < n; i++)
    if (ids[i] < 0 || ids[i] >= nwords || (i && ids[i] <= ids[i - 1])) return false;
  return true;
}

int vocab_params(vsg_vocab *voc, int *device, int *scoring, int *nwords) {
  if (!voc) return VSG_ERR_INVALID;
  *device = vsg::vocab_device(voc);
  return vsg_vocab_info(voc, nullptr, nullptr, scoring, nullptr, nullptr, nwords);
}
}  // namespace

struct vsg_kfdb {
  int device = 0, scoring = 0, nwords = 0;
  std::mutex mu;  // KeyFrameDatabase::mMutex, held for every call (a query holds it from enqueue to its tail)
  // every keyframe id the database has seen (added, mapped, or named as a neighbour): index -> id, map, live slots
  std::unordered_map<uint64_t, int> index;
  std::vector<uint64_t> id_of;
  std::vector<int32_t> map_of;
  std::vector<std::vector<int>> live_slots;  // ascending add sequence
  std::vector<int> bow_slot;                 // slot of the last add (KeyFrame::mBowVec), -1: none since the last clear()
  struct Slot {
    int kf;
    uint32_t off;
    int live;
    std::vector<int32_t> ids;    // host copy of the word ids (erase() finds its entries here)
    std::vector<uint8_t> alive;  // per entry
  };
  std::vector<Slot> slots;
  size_t n_ent = 0;
  // device
  KfState *d_st = nullptr;
  int *d_kf_bow = nullptr, *d_cov = nullptr;
  size_t kf_cap = 0, cov_cap = 0, bow_cap = 0;
  uint32_t *d_slot_off = nullptr;
  int *d_slot_len = nullptr, *d_slot_kf = nullptr;
  uint8_t *d_slot_dead = nullptr;
  size_t so_cap = 0, sl_cap = 0, sk_cap = 0, sd_cap = 0;
  int *d_ent_word = nullptr;
  double *d_ent_val = nullptr;
  size_t ew_cap = 0, ev_cap = 0;

  // index of `id`, created (with its device rows) on first sight; -1 on a HIP failure
  int kf_index(uint64_t id, hipStream_t st) {
    auto it = index.find(id);
    if (it != index.end()) return it->second;
    const int i = (int)id_of.size();
    const size_t n = (size_t)i + 1;
    if (grow(&d_st, &kf_cap, n, (size_t)i, 0, st) != VSG_OK || grow(&d_kf_bow, &bow_cap, n, (size_t)i, 0xFF, st) != VSG_OK ||
        grow(&d_cov, &cov_cap, n * kCov, (size_t)i * kCov, 0xFF, st) != VSG_OK)
      return -1;
    index.emplace(id, i);
    id_of.push_back(id), map_of.push_back(-1), live_slots.emplace_back(), bow_slot.push_back(-1);
    return i;
  }

  // tombstone entries / flag slots dead on the device (pinned lists, read in place)
  int mark(vsg::ThreadCtx *c, const std::vector<uint32_t> &tomb, const std::vector<int> &dead) {
    if (tomb.empty() && dead.empty()) return VSG_OK;
    vsg::Stage p;
    const size_t oT = p.add(4 * tomb.size()), oD = p.add(4 * dead.size());
    int rc = vsg::ctx_reserve(c, p.total, 0);
    if (rc != VSG_OK) return rc;
    memcpy(c->h_pin + oT, tomb.data(), 4 * tomb.size());
    memcpy(c->h_pin + oD, dead.data(), 4 * dead.size());
    const int n = (int)std::max(tomb.size(), dead.size());
    hipLaunchKernelGGL(k_kfdb_mark, dim3((n + 255) / 256), dim3(256), 0, c->stream, (const uint32_t *)(c->d_pin + oT),
                       (int)tomb.size(), d_ent_word, (const int *)(c->d_pin + oD), (int)dead.size(), d_slot_dead);
    TRY_HIP(hipGetLastError());
    TRY_HIP(hipStreamSynchronize(c->stream));
    return VSG_OK;
  }

  // drop every live slot of keyframe index i (clearMap); entries of dead slots need no tombstones
  void kill_all(int i, std::vector<int> &dead) {
    for (int s : live_slots[i]) {
      slots[s].live = 0;
      dead.push_back(s);
      if (s != bow_slot[i]) release(s);
    }
    live_slots[i].clear();
  }
  void release(int s) {
    std::vector<int32_t>().swap(slots[s].ids);
    std::vector<uint8_t>().swap(slots[s].alive);
  }
};

// ---- one query: the device part (count -> words -> select -> score -> covis, ONE wait), then the candidates in the
// order of lKFsSharingWords
static int kfdb_query(vsg_kfdb *db, int kind, uint64_t qid, const int32_t *ids, const double *vals, int n,
                      const uint64_t *conn_ids, int n_conn, std::vector<CandRec> &out) {
  out.clear();
  if (db->slots.empty() || n == 0) return VSG_OK;  // no posting can be walked: nothing changes
  int rc = VSG_OK;
  vsg::ThreadCtx *c = vsg::thread_ctx(db->device, &rc);
  if (!c) return rc;
  std::vector<int> conn;
  for (int j = 0; j < n_conn; j++) {  // connected keyframes the database never saw share no words
    auto it = db->index.find(conn_ids[j]);
    if (it != db->index.end()) conn.push_back(it->second);
  }
  const int nidx = (int)db->id_of.size(), n_slots = (int)db->slots.size();
  const size_t N = (size_t)n, NI = (size_t)nidx;
  vsg::Stage p, d;
  const size_t pQ = p.add(4 * N), pV = p.add(8 * N), pC = p.add(4 * conn.size()), pH = p.add(64), pO = p.add(16 * NI);
  const size_t dQ = d.add(4 * N), dV = d.add(8 * N), dC = d.add(4 * conn.size()), dCnt = d.add(4 * NI), dKey = d.add(8 * NI),
               dCand = d.add(4 * NI), dCtrl = d.add(64);
  rc = vsg::ctx_reserve(c, p.total, d.total);
  if (rc != VSG_OK) return rc;
  uint8_t *hp = c->h_pin, *dp = c->d_pin, *dv = c->d_buf;
  memcpy(hp + pQ, ids, 4 * N), memcpy(hp + pV, vals, 8 * N);
  if (!conn.empty()) memcpy(hp + pC, conn.data(), 4 * conn.size());
  int *q = (int *)(dv + dQ), *cn = (int *)(dv + dC), *cnt = (int *)(dv + dCnt), *cand = (int *)(dv + dCand),
      *ctrl = (int *)(dv + dCtrl);
  double *qv = (double *)(dv + dV);
  unsigned long long *key = (unsigned long long *)(dv + dKey);
  hipStream_t st = c->stream;
  TRY_HIP(hipMemcpyAsync(q, hp + pQ, 4 * N, hipMemcpyHostToDevice, st));
  TRY_HIP(hipMemcpyAsync(qv, hp + pV, 8 * N, hipMemcpyHostToDevice, st));
  if (!conn.empty()) TRY_HIP(hipMemcpyAsync(cn, hp + pC, 4 * conn.size(), hipMemcpyHostToDevice, st));
  TRY_HIP(hipMemsetAsync(cnt, 0, 4 * NI, st));
  TRY_HIP(hipMemsetAsync(key, 0xFF, 8 * NI, st));
  TRY_HIP(hipMemsetAsync(ctrl, 0, 64, st));
  const size_t lds = 4 * N;
  const int gi = (nidx + 255) / 256;
  hipLaunchKernelGGL(k_kfdb_count, dim3(grid_for(n_slots, 2048)), dim3(256), lds, st, q, n, db->d_slot_off,
                     db->d_slot_len, db->d_slot_kf, db->d_slot_dead, n_slots, db->d_ent_word, cnt, key);
  TRY_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_kfdb_words, dim3(gi), dim3(256), 0, st, nidx, kind, (unsigned long long)qid, cn, (int)conn.size(),
                     cnt, key, db->d_st, ctrl);
  TRY_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_kfdb_select, dim3(gi), dim3(256), 0, st, nidx, cnt, key, ctrl, cand);
  TRY_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_kfdb_score, dim3(grid_for(nidx, 1024)), dim3(256), lds, st, q, qv, n, db->scoring, kind, ctrl, cand,
                     db->d_kf_bow, db->d_slot_off, db->d_slot_len, db->d_ent_word, db->d_ent_val, db->d_st);
  TRY_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_kfdb_covis, dim3(gi), dim3(256), 0, st, kind, (unsigned long long)qid, ctrl, cand, key, db->d_cov,
                     db->d_st, (int *)(dp + pH), (CandRec *)(dp + pO));
  TRY_HIP(hipGetLastError());
  TRY_HIP(hipStreamSynchronize(st));
  const int nc = *(const int *)(hp + pH);
  if (nc < 0 || nc > nidx) return VSG_ERR_HIP;
  const CandRec *r = (const CandRec *)(hp + pO);
  out.assign(r, r + nc);
  std::sort(out.begin(), out.end(), [](const CandRec &a, const CandRec &b) { return a.key < b.key; });
  return VSG_OK;
}

static int check_query(vsg_kfdb *db, const int32_t *ids, const double *vals, int n) {
  if (!db || n < 0 || (n > 0 && (!ids || !vals))) return VSG_ERR_INVALID;
  if (db->scoring == 3) return VSG_ERR_UNSUPPORTED;  // KL: log() is not reproducible bit for bit on the device
  if (n > kMaxQueryWords) return VSG_ERR_UNSUPPORTED;
  if (!ascending_words(ids, n, db->nwords)) return VSG_ERR_INVALID;
  return VSG_OK;
}

extern "C" {

int vsg_vocab_score(vsg_vocab *voc, const int32_t *ids, const double *vals, int n, const int32_t *off,
                    const int32_t *m_ids, const double *m_vals, int m, double *out) {
  int device = 0, scoring = 0, nwords = 0;
  int rc = vocab_params(voc, &device, &scoring, &nwords);
  if (rc != VSG_OK) return rc;
  if (n < 0 || m < 0 || (n > 0 && (!ids || !vals)) || (m > 0 && (!off || !out))) return VSG_ERR_INVALID;
  if (scoring == 3) return VSG_ERR_UNSUPPORTED;
  if (scoring < 0 || scoring > 5 || n > kMaxQueryWords) return VSG_ERR_UNSUPPORTED;
  if (m == 0) return VSG_OK;
  if (off[0] != 0) return VSG_ERR_INVALID;
  for (int c = 0; c < m; c++)
    if (off[c + 1] < off[c]) return VSG_ERR_INVALID;
  const size_t E = (size_t)off[m];
  if (E > 0 && (!m_ids || !m_vals)) return VSG_ERR_INVALID;
  if (!ascending_words(ids, n, nwords)) return VSG_ERR_INVALID;
  for (int c = 0; c < m; c++)
    if (!ascending_words(m_ids + off[c], off[c + 1] - off[c], nwords)) return VSG_ERR_INVALID;
  vsg::ThreadCtx *c = vsg::thread_ctx(device, &rc);
  if (!c) return rc;
  const size_t N = (size_t)n, M = (size_t)m;
  vsg::Stage p, d;
  const size_t pQ = p.add(4 * N), pV = p.add(8 * N), pOff = p.add(4 * (M + 1)), pI = p.add(4 * E), pW = p.add(8 * E),
               pOut = p.add(8 * M);
  const size_t dQ = d.add(4 * N), dV = d.add(8 * N), dOff = d.add(4 * (M + 1)), dI = d.add(4 * E), dW = d.add(8 * E);
  rc = vsg::ctx_reserve(c, p.total, d.total);
  if (rc != VSG_OK) return rc;
  uint8_t *hp = c->h_pin, *dv = c->d_buf;
  memcpy(hp + pQ, ids, 4 * N), memcpy(hp + pV, vals, 8 * N), memcpy(hp + pOff, off, 4 * (M + 1));
  memcpy(hp + pI, m_ids, 4 * E), memcpy(hp + pW, m_vals, 8 * E);
  // one copy of the whole staged block (the device layout mirrors the pinned one up to the output)
  TRY_HIP(hipMemcpyAsync(dv, hp, pOut, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_vocab_score, dim3(grid_for(m, 1024)), dim3(256), 4 * N, c->stream, (const int *)(dv + dQ),
                     (const double *)(dv + dV), n, scoring, (const int *)(dv + dOff), (const int *)(dv + dI),
                     (const double *)(dv + dW), m, (double *)(c->d_pin + pOut));
  TRY_HIP(hipGetLastError());
  TRY_HIP(hipStreamSynchronize(c->stream));
  memcpy(out, hp + pOut, 8 * M);
  return VSG_OK;
}

int vsg_kfdb_create(vsg_vocab *voc, vsg_kfdb **out) {
  if (!out) return VSG_ERR_INVALID;
  *out = nullptr;
  int device = 0, scoring = 0, nwords = 0;
  const int rc = vocab_params(voc, &device, &scoring, &nwords);
  if (rc != VSG_OK) return rc;
  vsg_kfdb *db = new vsg_kfdb();
  db->device = device, db->scoring = scoring, db->nwords = nwords;
  *out = db;
  return VSG_OK;
}

void vsg_kfdb_destroy(vsg_kfdb *db) {
  if (!db) return;
  hipSetDevice(db->device);
  hipFree(db->d_st), hipFree(db->d_kf_bow), hipFree(db->d_cov), hipFree(db->d_slot_off), hipFree(db->d_slot_len);
  hipFree(db->d_slot_kf), hipFree(db->d_slot_dead), hipFree(db->d_ent_word), hipFree(db->d_ent_val);
  delete db;
}

int vsg_kfdb_add(vsg_kfdb *db, uint64_t kf_id, int32_t map_id, const int32_t *bow_ids, const double *bow_vals, int n) {
  if (!db || n < 0 || (n > 0 && (!bow_ids || !bow_vals))) return VSG_ERR_INVALID;
  if (!ascending_words(bow_ids, n, db->nwords)) return VSG_ERR_INVALID;
  std::lock_guard<std::mutex> lock(db->mu);
  if (db->n_ent + (size_t)n >= (size_t)INT32_MAX || db->slots.size() >= (size_t)INT32_MAX) return VSG_ERR_CAPACITY;
  int rc = VSG_OK;
  vsg::ThreadCtx *c = vsg::thread_ctx(db->device, &rc);
  if (!c) return rc;
  hipStream_t st = c->stream;
  const int i = db->kf_index(kf_id, st);
  if (i < 0) return VSG_ERR_HIP;
  const size_t s = db->slots.size(), ne = db->n_ent, N = (size_t)n;
  if ((rc = grow(&db->d_slot_off, &db->so_cap, s + 1, s, 0, st)) != VSG_OK ||
      (rc = grow(&db->d_slot_len, &db->sl_cap, s + 1, s, 0, st)) != VSG_OK ||
      (rc = grow(&db->d_slot_kf, &db->sk_cap, s + 1, s, 0, st)) != VSG_OK ||
      (rc = grow(&db->d_slot_dead, &db->sd_cap, s + 1, s, 1, st)) != VSG_OK ||
      (rc = grow(&db->d_ent_word, &db->ew_cap, ne + N, ne, 0, st)) != VSG_OK ||
      (rc = grow(&db->d_ent_val, &db->ev_cap, ne + N, ne, 0, st)) != VSG_OK)
    return rc;
  vsg::Stage p;
  const size_t pI = p.add(4 * N), pV = p.add(8 * N);
  if ((rc = vsg::ctx_reserve(c, p.total, 0)) != VSG_OK) return rc;
  if (n > 0) {
    memcpy(c->h_pin + pI, bow_ids, 4 * N), memcpy(c->h_pin + pV, bow_vals, 8 * N);
    TRY_HIP(hipMemcpyAsync(db->d_ent_word + ne, c->h_pin + pI, 4 * N, hipMemcpyHostToDevice, st));
    TRY_HIP(hipMemcpyAsync(db->d_ent_val + ne, c->h_pin + pV, 8 * N, hipMemcpyHostToDevice, st));
  }
  hipLaunchKernelGGL(k_kfdb_new_slot, dim3(1), dim3(64), 0, st, db->d_slot_off, db->d_slot_len, db->d_slot_kf,
                     db->d_slot_dead, db->d_kf_bow, (int)s, (uint32_t)ne, n, i);
  TRY_HIP(hipGetLastError());
  TRY_HIP(hipStreamSynchronize(st));
  vsg_kfdb::Slot sl;
  sl.kf = i, sl.off = (uint32_t)ne, sl.live = n;
  sl.ids.assign(bow_ids, bow_ids + n), sl.alive.assign(N, 1);
  const int prev = db->bow_slot[i];
  db->slots.push_back(std::move(sl));
  db->n_ent += N;
  if (n > 0) db->live_slots[i].push_back((int)s);
  if (prev >= 0 && db->slots[prev].live == 0) db->release(prev);  // no longer the BowVector, no live entry
  db->bow_slot[i] = (int)s;
  db->map_of[i] = map_id;
  return VSG_OK;
}

int vsg_kfdb_erase(vsg_kfdb *db, uint64_t kf_id) {
  if (!db) return VSG_ERR_INVALID;
  std::lock_guard<std::mutex> lock(db->mu);
  auto it = db->index.find(kf_id);
  if (it == db->index.end()) return VSG_OK;
  const int i = it->second;
  std::vector<int> &live = db->live_slots[i];
  if (live.empty()) return VSG_OK;
  int rc = VSG_OK;
  vsg::ThreadCtx *c = vsg::thread_ctx(db->device, &rc);
  if (!c) return rc;
  // for each word of the keyframe's BowVector: the first entry of the keyframe in that word's list = its oldest live slot
  // holding the word
  std::vector<std::pair<int, uint32_t>> hit;  // (slot, entry)
  const std::vector<int32_t> bow = db->slots[db->bow_slot[i]].ids;
  for (int32_t w : bow) {
    for (int s : live) {
      vsg_kfdb::Slot &S = db->slots[s];
      auto p = std::lower_bound(S.ids.begin(), S.ids.end(), w);
      if (p == S.ids.end() || *p != w) continue;
      const size_t j = (size_t)(p - S.ids.begin());
      if (!S.alive[j]) continue;
      S.alive[j] = 0, S.live--;
      hit.emplace_back(s, S.off + (uint32_t)j);
      break;
    }
  }
  std::vector<int> dead;
  std::vector<int> still;
  for (int s : live) {
    if (db->slots[s].live == 0) dead.push_back(s);
    else still.push_back(s);
  }
  std::vector<uint32_t> tomb;
  for (auto &h : hit)
    if (db->slots[h.first].live > 0) tomb.push_back(h.second);
  live.swap(still);
  for (int s : dead)
    if (s != db->bow_slot[i]) db->release(s);
  return db->mark(c, tomb, dead);
}

int vsg_kfdb_clear(vsg_kfdb *db) {
  if (!db) return VSG_ERR_INVALID;
  std::lock_guard<std::mutex> lock(db->mu);
  // every list is emptied; the store restarts (kf_bow rows on the device go stale, but a keyframe is only ever scored
  // while it has a live entry, i.e. after its next add)
  db->slots.clear();
  db->n_ent = 0;
  for (auto &l : db->live_slots) l.clear();
  std::fill(db->bow_slot.begin(), db->bow_slot.end(), -1);
  return VSG_OK;
}

int vsg_kfdb_clear_map(vsg_kfdb *db, int32_t map_id) {
  if (!db) return VSG_ERR_INVALID;
  std::lock_guard<std::mutex> lock(db->mu);
  std::vector<int> dead;
  for (size_t i = 0; i < db->id_of.size(); i++)
    if (db->map_of[i] == map_id && !db->live_slots[i].empty()) db->kill_all((int)i, dead);
  if (dead.empty()) return VSG_OK;
  int rc = VSG_OK;
  vsg::ThreadCtx *c = vsg::thread_ctx(db->device, &rc);
  if (!c) return rc;
  return db->mark(c, std::vector<uint32_t>(), dead);
}

int vsg_kfdb_set_map(vsg_kfdb *db, const uint64_t *kf_ids, const int32_t *map_ids, int n) {
  if (!db || n < 0 || (n > 0 && (!kf_ids || !map_ids))) return VSG_ERR_INVALID;
  std::lock_guard<std::mutex> lock(db->mu);
  int rc = VSG_OK;
  vsg::ThreadCtx *c = vsg::thread_ctx(db->device, &rc);
  if (!c) return rc;
  for (int j = 0; j < n; j++) {
    const int i = db->kf_index(kf_ids[j], c->stream);
    if (i < 0) return VSG_ERR_HIP;
    db->map_of[i] = map_ids[j];
  }
  return VSG_OK;
}

int vsg_kfdb_set_covisibility(vsg_kfdb *db, const uint64_t *kf_ids, const int32_t *offsets, const uint64_t *neigh_ids,
                              int n) {
  if (!db || n < 0 || (n > 0 && (!kf_ids || !offsets))) return VSG_ERR_INVALID;
  for (int j = 0; j < n; j++)
    if (offsets[j + 1] < offsets[j] || offsets[0] < 0) return VSG_ERR_INVALID;
  if (n > 0 && offsets[n] > 0 && !neigh_ids) return VSG_ERR_INVALID;
  if (n == 0) return VSG_OK;
  std::lock_guard<std::mutex> lock(db->mu);
  int rc = VSG_OK;
  vsg::ThreadCtx *c = vsg::thread_ctx(db->device, &rc);
  if (!c) return rc;
  std::vector<int> rows((size_t)n * (kCov + 1), -1);
  for (int j = 0; j < n; j++) {
    int *r = &rows[(size_t)j * (kCov + 1)];
    if ((r[0] = db->kf_index(kf_ids[j], c->stream)) < 0) return VSG_ERR_HIP;
    const int cnt = std::min(offsets[j + 1] - offsets[j], (int)kCov);  // GetBestCovisibilityKeyFrames(10)
    for (int k = 0; k < cnt; k++)
      if ((r[1 + k] = db->kf_index(neigh_ids[offsets[j] + k], c->stream)) < 0) return VSG_ERR_HIP;
  }
  vsg::Stage p;
  const size_t oR = p.add(4 * rows.size());
  if ((rc = vsg::ctx_reserve(c, p.total, 0)) != VSG_OK) return rc;
  memcpy(c->h_pin + oR, rows.data(), 4 * rows.size());
  hipLaunchKernelGGL(k_kfdb_set_cov, dim3((n + 255) / 256), dim3(256), 0, c->stream, (const int *)(c->d_pin + oR), n,
                     db->d_cov);
  TRY_HIP(hipGetLastError());
  TRY_HIP(hipStreamSynchronize(c->stream));
  return VSG_OK;
}

int vsg_kfdb_detect_relocalization_candidates(vsg_kfdb *db, uint64_t query_id, const int32_t *bow_ids,
                                              const double *bow_vals, int n, int32_t map_id, uint64_t *out_ids, int cap,
                                              int *n_out) {
  int rc = check_query(db, bow_ids, bow_vals, n);
  if (rc != VSG_OK) return rc;
  if (!n_out || cap < 0 || (cap > 0 && !out_ids)) return VSG_ERR_INVALID;
  *n_out = 0;
  std::lock_guard<std::mutex> lock(db->mu);
  std::vector<CandRec> acc;
  if ((rc = kfdb_query(db, 0, query_id, bow_ids, bow_vals, n, nullptr, 0, acc)) != VSG_OK) return rc;
  // :803-827
  float bestAccScore = 0;
  for (const CandRec &r : acc)
    if (r.acc > bestAccScore) bestAccScore = r.acc;
  const float minScoreToRetain = 0.75f * bestAccScore;
  std::unordered_set<int> added;
  int k = 0;
  for (const CandRec &r : acc) {
    if (!(r.acc > minScoreToRetain)) continue;
    if (db->map_of[r.best] != map_id) continue;
    if (added.insert(r.best).second) {
      if (k < cap) out_ids[k] = db->id_of[r.best];
      k++;
    }
  }
  *n_out = k;
  return k > cap ? VSG_ERR_CAPACITY : VSG_OK;
}

int vsg_kfdb_detect_n_best_candidates(vsg_kfdb *db, uint64_t query_kf_id, const int32_t *bow_ids,
                                      const double *bow_vals, int n, const uint64_t *connected_ids, int n_conn,
                                      int32_t map_id, const int32_t *bad_map_ids, int n_bad, int nNumCandidates,
                                      uint64_t *loop_out, int *n_loop, uint64_t *merge_out, int *n_merge) {
  int rc = check_query(db, bow_ids, bow_vals, n);
  if (rc != VSG_OK) return rc;
  if (n_conn < 0 || (n_conn > 0 && !connected_ids) || n_bad < 0 || (n_bad > 0 && !bad_map_ids) || nNumCandidates < 0 ||
      !n_loop || !n_merge || (nNumCandidates > 0 && (!loop_out || !merge_out)))
    return VSG_ERR_INVALID;
  *n_loop = *n_merge = 0;
  std::lock_guard<std::mutex> lock(db->mu);
  std::vector<CandRec> acc;
  if ((rc = kfdb_query(db, 1, query_kf_id, bow_ids, bow_vals, n, connected_ids, n_conn, acc)) != VSG_OK) return rc;
  // :687-716: lAccScoreAndMatch.sort(compFirst) is a stable sort, descending accScore
  std::stable_sort(acc.begin(), acc.end(), [](const CandRec &a, const CandRec &b) { return a.acc > b.acc; });
  const std::unordered_set<int32_t> bad(bad_map_ids, bad_map_ids + n_bad);
  const size_t N = (size_t)nNumCandidates;
  size_t nl = 0, nm = 0;
  std::unordered_set<int> added;
  for (size_t i = 0; i < acc.size() && (nl < N || nm < N); i++) {
    const int b = acc[i].best;
    if (added.count(b)) continue;
    const int32_t m = db->map_of[b];
    if (map_id == m && nl < N) loop_out[nl++] = db->id_of[b];
    else if (map_id != m && nm < N && !bad.count(m)) merge_out[nm++] = db->id_of[b];
    added.insert(b);
  }
  *n_loop = (int)nl, *n_merge = (int)nm;
  return VSG_OK;
}

// test hook (include/vsg_orb_debug.h): the KfState row of one keyframe, read back after everything enqueued
int vsg_debug_kfdb_state(vsg_kfdb *db, uint64_t kf_id, uint64_t query[2], int32_t words[2], float score[2]) {
  if (!db || !query || !words || !score) return VSG_ERR_INVALID;
  std::lock_guard<std::mutex> lock(db->mu);
  auto it = db->index.find(kf_id);
  if (it == db->index.end()) return VSG_ERR_INVALID;
  int rc = VSG_OK;
  vsg::ThreadCtx *c = vsg::thread_ctx(db->device, &rc);
  if (!c) return rc;
  TRY_HIP(hipStreamSynchronize(c->stream));
  KfState s;
  TRY_HIP(hipMemcpy(&s, db->d_st + it->second, sizeof s, hipMemcpyDeviceToHost));
  query[0] = s.rq, query[1] = s.pq;
  words[0] = s.rw, words[1] = s.pw;
  score[0] = s.rs, score[1] = s.ps;
  return VSG_OK;
}

}  // extern "C"
