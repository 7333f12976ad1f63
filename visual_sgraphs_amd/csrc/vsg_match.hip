// vsg_match.hip -- Hamming searches of ORBmatcher (orb_slam3/src/ORBmatcher.cc) on flattened POD views.
//
// Integer XOR + popcount work (v_xor_b32 / v_bcnt_u32_b32); the brute-force best / second-best scan alone runs on the
// matrix cores (k_block_best2_mfma).
//   * The vocabulary-node searches: nodes are independent (a feature belongs to one node), so a WORKGROUP takes one node both
//     FeatureVectors have, joined on the host (vsg_fv.h, after its checks) or, for two resident ones, in the kernel
//     (block_node).  k_search_by_bow keeps the reference's greedy "already matched" order inside a node as a fixed point over
//     an LDS distance matrix; k_triangulation_walk has no greedy state and walks a node in LDS tiles, its pair predicate a
//     template parameter (the epipolar test of vsg_epipolar.h computed in place, or bits the caller made).
//   * The searches on candidate lists the CALLER made: every candidate's distance in one data-parallel pass (k_cand_dist),
//     the ordered walk over the queries on the host (vsg_walks.h).  On resident frames: vsg_window.hip.
// best / second-best follow the reference's strict '<' scan: packed keys (dist << 20 | scan position) make
// "earliest candidate wins ties" a plain integer minimum (the triangulation walk inverts the position: later wins there).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

#include "../../include/vsg_orb.h"
#include "../../include/vsg_orb_debug_epipolar.h"
#include "vsg_ctx.h"
#include "vsg_epipolar.h"
#include "vsg_frame_int.h"
#include "vsg_fv.h"
#include "vsg_math.h"
#include "vsg_walks.h"

namespace {

const int TH_HIGH = 100;      // ORBmatcher.cc:34
const int TH_LOW = 50;        // ORBmatcher.cc:35
const int HISTO_LENGTH = 30;  // ORBmatcher.cc:36
const uint32_t KEY_NONE = (256u << 20) | 0xFFFFFu;
// The reference's scans start from bestDist = 256 and update on a strict '<', so a candidate at distance 256 (every
// bit different) is never selected: any key whose distance field is 256 means "no best".
__device__ __forceinline__ bool key_is_none(uint32_t k) { return (k >> 20) >= 256u; }

__device__ __forceinline__ int hamming256(const uint4 a0, const uint4 a1, const uint4 b0, const uint4 b1) {
  return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) +
         __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}
__device__ __forceinline__ void load_desc(const uint8_t *base, int row, uint4 &lo, uint4 &hi) {
  const uint4 *p = (const uint4 *)(base + (size_t)row * 32);
  lo = p[0];
  hi = p[1];
}

// two smallest of {k1,k2} U {o1,o2}, each pair already ordered
__device__ __forceinline__ void merge2(uint32_t &k1, uint32_t &k2, uint32_t o1, uint32_t o2) {
  if (o1 < k1) {
    k2 = min(k1, o2);
    k1 = o1;
  } else {
    k2 = min(k2, o1);
  }
}
__device__ __forceinline__ void wave_best2(uint32_t &k1, uint32_t &k2) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const uint32_t o1 = __shfl_xor(k1, d), o2 = __shfl_xor(k2, d);
    merge2(k1, k2, o1, o2);
  }
}
__device__ __forceinline__ uint32_t wave_min(uint32_t k) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) k = min(k, __shfl_xor(k, d));
  return k;
}

// ---- DescriptorDistance over index pairs
__global__ void k_hamming_pairs(const uint8_t *a, const uint8_t *b, const int *ia, const int *ib, int n, int *dist) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint4 a0, a1, b0, b1;
  load_desc(a, ia[i], a0, a1);
  load_desc(b, ib[i], b0, b1);
  dist[i] = hamming256(a0, a1, b0, b1);
}

// ---- brute-force best / second best.  Packed keys (dist << 20 | index) are unique and keep the reference's strict-'<'
// scan semantics: the smallest key is the first minimum, the second smallest is "bestDist2".  With k1 <= k2 the update is
// k2 = median(k1, k2, key), k1 = min(k1, key): one v_med3_u32 and one v_min_u32 per pair.
__device__ __forceinline__ uint32_t umed3(uint32_t a, uint32_t b, uint32_t c) {
  return min(max(a, b), max(min(a, b), c));  // folded to v_med3_u32
}
enum { kMatchQW = 2, kBest2Rows = 128 * kMatchQW };  // query sets of 32 per wave; A rows per workgroup

// ---- the best / second-best scan on the matrix cores.  A Hamming distance matrix is a GEMM over +-1 vectors:
// with s(x) = 2*bit - 1, sum_k s(a_k) * s(b_k) = 256 - 2 * dist.  The train rows are expanded with their bits
// INVERTED (so each product is negated), hence
//     D[i][j] = sum_k (-s(train_i,k)) * s(query_j,k) = 2 * dist(train_i, query_j) - 256
// The operands are FP4 (e2m1: +1 = 0x2, -1 = 0xA; block scales 2^0) for `v_mfma_scale_f32_32x32x64_f8f6f4`: K = 64 per
// instruction at the 32 cycles of the i8 form's K = 32 (tools/ubench.hip), so a 32 x 32 tile of 256-bit distances is FOUR
// instructions (round 4; rounds 1-3: eight v_mfma_i32_32x32x32_i8 -- 0.148 -> 0.111 ms per 512 x 1006^2 pairs, + 2.2 %
// frames/s in the same run), a descriptor dword expands into ONE 16-byte operand through a byte -> 8-nibble table and a
// tile of train rows is 4 KB of LDS.  Sums of +-1 products are exact in fp32.  A wave owns 32 queries (the MFMA's columns,
// kept expanded in 16 VGPRs for the whole scan); the workgroup expands each tile of 32 train rows once into LDS for its
// four waves.  C/D layout: lane = column + 32 * h, register g holds row (g & 3) + 8 * (g >> 2) + 4 * h, so a lane
// folds its 16 rows into a best/second pair of FLOAT keys 32 * acc + row offset (exact, lexicographic in (acc, row)) with
// v_fma_f32 + v_min_f32 + v_med3_f32 per pair, turns the two survivors into the packed integer keys
// (2 * dist << 19 | index == dist << 20 | index) and the two lanes of a column merge at the end: tie handling follows the
// packed-key rule above (an xor + popcount form of this scan measured 0.182 ms per 256 x 1006^2 pairs against 0.088 ms
// for the i8 form: DESIGN 8, round 1).
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

__global__ __launch_bounds__(256) void k_block_best2_mfma(const uint8_t *a_base, const uint8_t *b_base,
                                                          size_t block_stride, const int *counts_a, const int *counts_b,
                                                          int count_stride, int fixed_na, int fixed_nb, int max_rows,
                                                          int *best, int *second, int *argbest) {
  constexpr int TR = 1;  // 32-row train tiles per iteration (independent MFMA chains, one barrier)
  __shared__ i32x4 tiles[2][TR][8 * 32];  // double buffer of [tile][descriptor dword d = 2 * k-step + half][train row r]
  __shared__ uint32_t lut[256];           // byte -> its 8 bits as FP4 nibbles
  {
    uint32_t m = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) m |= ((threadIdx.x >> i) & 1u) << (4 * i + 3);
    lut[threadIdx.x] = 0xAAAAAAAAu ^ m;  // bit set -> 0x2 (+1), bit clear -> 0xA (-1)
  }
  const int blk = blockIdx.y;
  // counts clamp to [0, max_rows].  A negative na has to become 0 HERE: the early return below compares unsigned, so a
  // block with na = -1 would not leave and would scan all of B for rows it never writes
  const int na = counts_a ? min(max(counts_a[blk * count_stride], 0), max_rows) : fixed_na;
  const int nb = counts_b ? min(max(counts_b[blk * count_stride], 0), max_rows) : fixed_nb;
  const uint8_t *A = a_base + (size_t)blk * block_stride, *B = b_base + (size_t)blk * block_stride;
  if (blockIdx.x * kBest2Rows >= na) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  // A wave owns QW sets of 32 queries (round 6: two): the train operand read from LDS feeds QW matrix instructions, whose
  // accumulator chains are independent, and the workgroup's tile expansion serves twice the queries.  Per 1024 x 1006^2 pairs:
  // QW 1 / 2 / 3 / 4 = 0.204 / 0.186 / 0.199 / 0.221 ms at 78 / 114 / 154 / 186 VGPRs (6 / 4 / 3 / 2 waves per SIMD); two sets forced
  // into 96 registers spill and take 0.50 ms (profiles/r06_f_*)
  constexpr int QW = kMatchQW;
  const int q0 = blockIdx.x * kBest2Rows + wave * 32 * QW + r;  // this lane's query (column) of set 0; set u: + 32 u
  const bool wave_active = blockIdx.x * kBest2Rows + wave * 32 * QW < na;
  // queries: dword 2 s + h of the descriptor is the lane's 32 K-values of k-step s (expanded below, once the table is there)
  uint32_t qraw[QW][4];
#pragma unroll
  for (int u = 0; u < QW; u++) {
    const int q = q0 + 32 * u;
    const uint32_t *qd = (const uint32_t *)(A + (size_t)(q < na ? q : 0) * 32);
#pragma unroll
    for (int s = 0; s < 4; s++) qraw[u][s] = qd[2 * s + h];
  }
  uint32_t k1[QW], k2[QW];
#pragma unroll
  for (int u = 0; u < QW; u++) k1[u] = KEY_NONE, k2[u] = KEY_NONE;
  // tile expansion: thread = (train row, dword); the row runs along the lanes so that a wave's 16-byte LDS stores
  // are contiguous (the dword-fastest mapping put 8 lanes on the same banks: an 8-way conflict on every store)
  const int erow = tid & 31, es = tid >> 5;
  auto fetch = [&](int row0) {  // one dword of a train row, inverted (negated products); past the end: any valid row
    const int tr = row0 + erow;
    return ~((const uint32_t *)(B + (size_t)(tr < nb ? tr : 0) * 32))[es];
  };
  // The train dwords are prefetched a GROUP of kPf tiles ahead (register double bank): an iteration is ~600 cycles, a global
  // round trip several thousand, so a one-iteration prefetch left every iteration waiting on memory.  With two query sets per
  // wave: groups of 4 / 6 / 8 / 10 tiles = 0.185 / 0.200 / 0.181 / 0.188 ms per 1024 x 1006^2 pairs (122 VGPRs at 8: still 4 waves
  // per SIMD; profiles/r06_f_*)
  constexpr int kPf = 8;
  uint32_t wa[kPf], wn[kPf];
#pragma unroll
  for (int j = 0; j < kPf; j++) wa[j] = fetch(32 * j), wn[j] = 0u;
  __syncthreads();  // lut
  const f32x16 zerof = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  auto expand4 = [&](uint32_t w) {
    return (i32x8){(int)lut[w & 255], (int)lut[(w >> 8) & 255], (int)lut[(w >> 16) & 255], (int)lut[w >> 24], 0, 0, 0, 0};
  };
  i32x8 Q[QW][4];
#pragma unroll
  for (int u = 0; u < QW; u++)
#pragma unroll
    for (int s = 0; s < 4; s++) Q[u][s] = expand4(qraw[u][s]);
  const int kScale = 0x7F7F7F7F;  // e8m0 block scales: 2^0
  int buf = 0;
  for (int tg = 0; tg < nb; tg += 32 * kPf) {
    if (tg + 32 * kPf < nb) {
#pragma unroll
      for (int j = 0; j < kPf; j++) wn[j] = fetch(tg + 32 * (kPf + j));
    }
#pragma unroll
    for (int j = 0; j < kPf; j += TR) {
      const int t0 = tg + 32 * j;
      if (t0 >= nb) break;
#pragma unroll
      for (int t = 0; t < TR; t++) {
        i32x4 *tile = tiles[buf][t];
        const uint32_t ww = wa[j + t];
        tile[es * 32 + erow] = (i32x4){(int)lut[ww & 255], (int)lut[(ww >> 8) & 255], (int)lut[(ww >> 16) & 255], (int)lut[ww >> 24]};
      }
      // one barrier per iteration: nobody can overwrite this buffer before every wave has passed the NEXT
      // barrier, i.e. finished reading it
      __syncthreads();
      if (wave_active) {
        // acc = sum of negated products = 2 * dist - 256 (C operand: inline 0)
        f32x16 acc[QW][TR];
        auto opA = [&](int t, int s) {
          const i32x4 v = tiles[buf][t][(s * 2 + h) * 32 + r];
          return (i32x8){v.x, v.y, v.z, v.w, 0, 0, 0, 0};
        };
#pragma unroll
        for (int s = 0; s < 4; s++)
#pragma unroll
          for (int t = 0; t < TR; t++) {
            const i32x8 a = opA(t, s);  // ONE operand read for the QW instructions of this k-step
#pragma unroll
            for (int u = 0; u < QW; u++)
              acc[u][t] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, Q[u][s], s == 0 ? zerof : acc[u][t], 4, 4, 0, kScale, 0,
                                                                          kScale);
          }
#pragma unroll
        for (int t = 0; t < TR; t++) {
          const int tb = t0 + 32 * t + 4 * h;  // row of register 0 of this lane
          if (tb - 4 * h + 32 <= nb) {
            // full tile: the best two of the lane's 16 rows on FLOAT keys 32 * acc + row offset (exact: |32 acc + 27| < 2^14;
            // the offset < 32 keeps (acc, row) in lexicographic order): one v_fma_f32, one v_min_f32, one v_med3_f32 per
            // pair; the two survivors become the integer keys (dist << 20 | row) the rest of the kernel works on
#pragma unroll
            for (int u = 0; u < QW; u++) {
              float f1 = __builtin_inff(), f2 = __builtin_inff();
#pragma unroll
              for (int g = 0; g < 16; g++) {
                const float kf = __builtin_fmaf(acc[u][t][g], 32.0f, (float)((g & 3) + 8 * (g >> 2)));
                f2 = __builtin_amdgcn_fmed3f(f1, f2, kf);
                f1 = __builtin_fminf(f1, kf);
              }
              const int i1 = (int)f1, i2 = (int)f2;  // 32 acc + offset: acc = i >> 5 (floor), offset = i & 31
              const uint32_t l1 = ((uint32_t)((i1 >> 5) + 256) << 19) + (uint32_t)((i1 & 31) + tb);
              const uint32_t l2 = ((uint32_t)((i2 >> 5) + 256) << 19) + (uint32_t)((i2 & 31) + tb);
              k2[u] = min(max(k1[u], l1), min(k2[u], l2));
              k1[u] = min(k1[u], l1);
            }
          } else {
#pragma unroll
            for (int u = 0; u < QW; u++)
#pragma unroll
              for (int g = 0; g < 16; g++) {
                const int row = tb + (g & 3) + 8 * (g >> 2);
                uint32_t key = ((uint32_t)((int)acc[u][t][g] + 256) << 19) | (uint32_t)row;
                if (row >= nb) key = KEY_NONE;
                k2[u] = umed3(k1[u], k2[u], key);
                k1[u] = min(k1[u], key);
              }
          }
        }
      }
      buf ^= 1;
    }
#pragma unroll
    for (int j = 0; j < kPf; j++) wa[j] = wn[j];
  }
#pragma unroll
  for (int u = 0; u < QW; u++) {
    const uint32_t o1 = __shfl_xor(k1[u], 32), o2 = __shfl_xor(k2[u], 32);
    merge2(k1[u], k2[u], o1, o2);
    const int q = q0 + 32 * u;
    if (h == 0 && q < na) {
      const size_t o = (size_t)blk * max_rows + q;
      best[o] = (int)(k1[u] >> 20);
      second[o] = (int)(k2[u] >> 20);
      argbest[o] = key_is_none(k1[u]) ? -1 : (int)(k1[u] & 0xFFFFF);
    }
  }
}

// ---- the vocabulary-node searches: one WORKGROUP per node both FeatureVectors have.
using vsg::FvDev;  // a FeatureVector resident on the device (vsg_frame_int.h: Frame::mFeatVec written by k_bow_assemble)
using vsg::NodePair;

// The node of this block, block-uniform; false: the block has none.  Joined on the host (pairs: block b takes pairs[b]), or
// -- pairs == nullptr -- BOTH FeatureVectors are resident and the join of ORBmatcher.cc:247-405 happens here: block b takes
// node b of A and looks the same id up in B's node list (a node is shared or it is not: the merge-join's lower_bound jumps
// and this lookup name the same pairs; nodes are independent, their order is irrelevant).  idxA / idxB then become the
// resident lists.
__device__ __forceinline__ bool block_node(const NodePair *pairs, int npairs, const FvDev &fa, const FvDev &fb, NodePair &np,
                                           const int *&idxA, const int *&idxB) {
  const int node = blockIdx.x, tid = threadIdx.x;
  if (pairs) {
    if (node >= npairs) return false;
    np = pairs[node];
    return true;
  }
  // everything the join needs is requested at once (B's node list 256 entries at a time, whatever the headers say: the
  // arrays hold capacity + 1 entries): ONE memory round trip in front of the offsets instead of a bisection's eight
  __shared__ int s_pos;
  const int nA_nodes = fa.hdr[0], nB_nodes = fb.hdr[0];
  const int id = node < nA_nodes ? fa.node[node] : -1;
  if (tid == 0) s_pos = -1;
  __syncthreads();
  for (int base = 0; base < nB_nodes; base += 256)  // block-uniform; one pass for the reference's ~100 nodes
    if (base + tid < nB_nodes && fb.node[base + tid] == id) s_pos = base + tid;  // ids are unique: at most one writer
  __syncthreads();
  const int lo = s_pos;
  if (node >= nA_nodes || lo < 0) return false;
  np.a_begin = fa.off[node], np.a_end = fa.off[node + 1], np.b_begin = fb.off[lo], np.b_end = fb.off[lo + 1];
  idxA = fa.idx, idxB = fb.idx;
  return true;
}

// ---- SearchByBoW
// mode 0: KF -> Frame  (ORBmatcher.cc:254-392): skip F features already in match_f; accept bestDist1 <= TH_LOW
// mode 1: KF -> KF     (ORBmatcher.cc:790-864): skip vbMatched2 / invalid; accept bestDist1 <  TH_LOW
enum { kBowNodeSide = 128 };  // nodes up to this many features a side are matched on a distance matrix in LDS

//   * The node's descriptors go to LDS once (na + nb rows, not na x nb row pairs), every distance of the node is computed
//     from there in one sweep of all 256 lanes.
//   * The ordered, greedy walk (a KeyFrame feature sees the claims of the ones BEFORE it) as a fixed point, one lane per
//     KeyFrame feature: in round t every feature decides on the claims that the features before it made in round t - 1.
//     By induction feature i is final from round i + 1 on, and a round that changes no decision is the walk's result
//     (feature 0 never depended on anyone, feature 1 is consistent with feature 0's final claim, ...).  Conflicts between
//     neighbours are rare, so a node settles in 2-4 rounds of ~nb LDS reads per lane instead of na dependent reductions.
// `match` is WRITE-ONLY (pre-filled with -1 by whoever owns it: it may be pinned host memory); every feature belongs to
// exactly one node, so a node's block is the only writer and the only reader of its claims.
__global__ __launch_bounds__(256) void k_search_by_bow(const NodePair *pairs, int npairs, FvDev fa, FvDev fb,
                                                       const uint8_t *descA,
                                                       const uint8_t *validA, const int *idxA, const uint8_t *descB,
                                                       const uint8_t *validB, const int *idxB, float nnratio, int mode,
                                                       int nleftB /*mode0: F.Nleft or -1*/,
                                                       int *match /*mode0: match_f [nB], mode1: matches12 [nA]*/,
                                                       int *claimB /*device scratch [nB]: large nodes only*/) {
  const int tid = threadIdx.x, lane = tid & 63;
  NodePair np;
  if (!block_node(pairs, npairs, fa, fb, np, idxA, idxB)) return;
  const int nb = np.b_end - np.b_begin, na = np.a_end - np.a_begin;
  __shared__ uint4 s_da[kBowNodeSide][2], s_db[kBowNodeSide][2];
  __shared__ uint16_t s_dist[kBowNodeSide * kBowNodeSide];
  __shared__ int s_rb[kBowNodeSide], s_ra[kBowNodeSide], s_by0[kBowNodeSide], s_by[kBowNodeSide];
  __shared__ int s_changed[2];  // by round parity: a flag is cleared a whole round before it is written again
  if (na <= kBowNodeSide && nb <= kBowNodeSide) {
    const int kFree = 0x7FFFFFFF;
    {  // rows of both sides: thread = (row, half)
      const int r = tid >> 1, h = tid & 1;
      if (r < na) {
        const int ra = idxA[np.a_begin + r];
        s_da[r][h] = ((const uint4 *)(descA + (size_t)ra * 32))[h];
        if (h == 0) s_ra[r] = validA[ra] ? ra : -1;  // !pMP || pMP->isBad()
      }
      if (tid < 2) s_changed[tid] = 0;
      if (r < nb) {
        const int rb = idxB[np.b_begin + r];
        s_db[r][h] = ((const uint4 *)(descB + (size_t)rb * 32))[h];
        if (h == 0) s_rb[r] = rb, s_by0[r] = s_by[r] = (mode == 1 && !validB[rb]) ? -1 : kFree;  // -1: never a candidate
      }
    }
    __syncthreads();
    const float inv_nb = 1.0f / (float)nb;
    for (int p = tid; p < na * nb; p += 256) {
      const int i = min((int)(((float)p + 0.5f) * inv_nb), na - 1), j = p - i * nb;
      s_dist[p] = (uint16_t)hamming256(s_da[i][0], s_da[i][1], s_db[j][0], s_db[j][1]);
    }
    __syncthreads();
    const int i = tid;
    const int ra = i < na ? s_ra[i] : -1;
    const bool active = ra >= 0;
    int decL = -1, decR = -1;
    for (int round = 0; round <= na; round++) {  // block-uniform
      int newL = -1, newR = -1;
      if (active) {
        uint32_t k1 = KEY_NONE, k2 = KEY_NONE, r1 = KEY_NONE;
        const uint16_t *row = s_dist + i * nb;
        // branch-free, so that the LDS reads of several candidates are in flight together (a taken candidate -- by a feature
        // before this one, or not a candidate at all -- contributes the neutral key)
        if (nleftB < 0) {
#pragma unroll 4
          for (int j = 0; j < nb; j++) {
            const uint32_t key = s_by[j] < i ? KEY_NONE : ((uint32_t)row[j] << 20) | (uint32_t)j;
            k2 = umed3(k1, k2, key), k1 = min(k1, key);
          }
        } else {
#pragma unroll 4
          for (int j = 0; j < nb; j++) {
            const uint32_t key = s_by[j] < i ? KEY_NONE : ((uint32_t)row[j] << 20) | (uint32_t)j;
            const bool isleft = s_rb[j] < nleftB;
            const uint32_t kl = isleft ? key : KEY_NONE, kr = isleft ? KEY_NONE : key;
            k2 = umed3(k1, k2, kl), k1 = min(k1, kl);
            r1 = min(r1, kr);
          }
        }
        const int bestDist1 = (int)(k1 >> 20), bestDist2 = (int)(k2 >> 20);
        // right block, nested in the left test, no ratio test (:362-389)
        if (nleftB >= 0 && bestDist1 <= TH_LOW && (int)(r1 >> 20) <= TH_LOW) newR = (int)(r1 & 0xFFFFF);
        const bool pass = mode == 0 ? bestDist1 <= TH_LOW : bestDist1 < TH_LOW;
        if (pass && (float)bestDist1 < nnratio * (float)bestDist2) newL = (int)(k1 & 0xFFFFF);  // :335-337 / :843-845
      }
      const bool changed = newL != decL || newR != decR;
      decL = newL, decR = newR;
      __syncthreads();  // every lane has read the claims of the previous round (and that round's flag)
      if (tid < nb) s_by[tid] = s_by0[tid];
      if (tid == 0) s_changed[(round + 1) & 1] = 0;
      __syncthreads();
      if (newL >= 0) atomicMin(&s_by[newL], i);
      if (newR >= 0) atomicMin(&s_by[newR], i);
      if (changed) s_changed[round & 1] = 1;
      __syncthreads();
      if (!s_changed[round & 1]) break;
    }
    if (active) {
      if (mode == 0) {
        if (decL >= 0) match[s_rb[decL]] = ra;  // vpMapPointMatches[bestIdxF] = pMP
        if (decR >= 0) match[s_rb[decR]] = ra;
      } else if (decL >= 0) {
        match[ra] = s_rb[decL];                 // vpMatches12[idx1] = vpMapPoints2[bestIdx2]
      }
    }
    return;
  }
  if (tid >= 64) return;
  // ---- large nodes: one scan of the node's Frame features per KeyFrame feature; the claims in device scratch, set up here
  for (int j = lane; j < nb; j += 64) {
    const int rb = idxB[np.b_begin + j];
    claimB[rb] = mode == 1 ? (int)(!validB[rb]) : 0;
  }
  __threadfence_block();
  for (int ia = np.a_begin; ia < np.a_end; ia++) {
    const int ra = idxA[ia];
    if (!validA[ra]) continue;  // !pMP || pMP->isBad()
    uint4 a0, a1;
    load_desc(descA, ra, a0, a1);
    uint32_t k1 = KEY_NONE, k2 = KEY_NONE, r1 = KEY_NONE, r2 = KEY_NONE;  // left / right-camera (fisheye) candidates
    for (int j = lane; j < nb; j += 64) {
      const int rb = idxB[np.b_begin + j];
      if (__hip_atomic_load(&claimB[rb], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) continue;
      uint4 b0, b1;
      load_desc(descB, rb, b0, b1);
      const uint32_t key = ((uint32_t)hamming256(a0, a1, b0, b1) << 20) | (uint32_t)j;
      if (nleftB < 0 || rb < nleftB)
        merge2(k1, k2, key, KEY_NONE);
      else
        merge2(r1, r2, key, KEY_NONE);
    }
    wave_best2(k1, k2);
    const int bestDist1 = (int)(k1 >> 20), bestDist2 = (int)(k2 >> 20);
    if (nleftB >= 0 && bestDist1 <= TH_LOW) {  // right block, nested in the left test, no ratio test (:362-389)
      r1 = wave_min(r1);
      if ((int)(r1 >> 20) <= TH_LOW) {
        const int rb = idxB[np.b_begin + (int)(r1 & 0xFFFFF)];
        if (lane == 0) match[rb] = ra, claimB[rb] = 1;
        __threadfence_block();  // later KF features of this node must see the claim
      }
    }
    const bool pass = mode == 0 ? bestDist1 <= TH_LOW : bestDist1 < TH_LOW;
    if (pass && (float)bestDist1 < nnratio * (float)bestDist2) {  // :335-337 / :843-845
      const int rb = idxB[np.b_begin + (int)(k1 & 0xFFFFF)];
      if (lane == 0) {
        if (mode == 0)
          match[rb] = ra;  // vpMapPointMatches[bestIdxF] = pMP
        else
          match[ra] = rb;  // vpMatches12[idx1] = vpMapPoints2[bestIdx2]
        claimB[rb] = 1;     // (mode 1: vbMatched2[bestIdx2] = true)
      }
      __threadfence_block();
    }
  }
}

// ---- SearchForTriangulation (ORBmatcher.cc:902-1146).  For every KF1 feature of the node that is walked: the best KF2
// feature of the node with dist <= TH_LOW whose pair passes the geometric predicate of :976-1073.  The reference's
// `dist > bestDist -> continue` lets a LATER equal distance win, so keys are (dist << 20) | (0xFFFFF - j), j = the position in
// the node's KF2 list ACROSS tiles, and the walk takes their minimum.  The predicate is a pure function of the pair and the
// reference never sets vbMatched2, so KF1 features are independent.  ONE walk; the predicate is the template parameter:
//   * EpipolarPred: evaluated HERE (vsg_epipolar.h).  (a, b, c, den) of the row's epipolar line are wave-uniform; a KF2 row
//     brings x, y, the level's gate radius and chi-square bound (two 16-entry tables made by the host with the header's own
//     functions) and the flags (stereo; has a map point), in LDS arrays only this instantiation keeps;
//   * CallerBitsPred: one bit per pair made by the caller, bit pair_off[s] + i * nb + j for positions (i, j) of the s-th
//     shared node's lists (pair_bits_check of vsg_fv.h saw the layout: the sum fits an int); bits == nullptr: every pair
//     passes.  A row of either side needs its eligible flag.
// The node's KF2 side goes to LDS once per tile of kEpiTile rows.  Waves take the KF1 rows round-robin; the lanes stride the
// tile's KF2 rows, run the predicate first and the Hamming distance for the survivors; wave_min over the keys.  KF1 rows are
// taken kEpiRows at a time, staged the same way (one round of loads instead of a dependent chain per row); a row's running
// minimum over the tiles lives in LDS (s_key), owned by the wave that walks the row.  A node of any size on either side is
// walked with the same 14 KB of LDS; a node whose KF2 side fits one tile (every node of a real FeatureVector) is staged once.
// matches12 is WRITE-ONLY (pre-filled with -1 by the host: it may be pinned memory); a KF1 feature belongs to one node.
struct EpiParams {
  float F12[9], ep[2];
  float gate[16];    // epipole_gate_radius(mvScaleFactors2[level]); 0 above nlevels
  double bound[16];  // chi_square_bound(mvLevelSigma2_2[level])
  int only_stereo, coarse;
};
struct EpiFrame {
  const vsg::KeyPointPOD *kps;
  const uint8_t *desc;
  const float *uright;   // nullptr: every mvuRight is -1
  const uint8_t *no_mp;  // !pKF->GetMapPoint(i)
};
struct EpipolarPred {
  EpiFrame A, B;
  EpiParams P;
};
struct CallerBitsPred {
  const uint8_t *desc1, *eligible1, *desc2, *eligible2;
  const uint32_t *bits;
  const int *pair_off;
};
enum { kEpiTile = 128, kEpiRows = 128, kEpiStereo = 1, kEpiHasMp = 2 };

template <class Pred>
__global__ __launch_bounds__(256) void k_triangulation_walk(const NodePair *pairs, int npairs, FvDev fa, FvDev fb,
                                                            const int *idxA, const int *idxB, Pred q, int *matches12) {
  constexpr bool kEpi = std::is_same<Pred, EpipolarPred>::value;
  const uint8_t *descA, *descB;
  if constexpr (kEpi)
    descA = q.A.desc, descB = q.B.desc;
  else
    descA = q.desc1, descB = q.desc2;
  const int node = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  NodePair np;
  if (!block_node(pairs, npairs, fa, fb, np, idxA, idxB)) return;
  const int na = np.a_end - np.a_begin, nb = np.b_end - np.b_begin;
  __shared__ uint4 s_d[kEpiTile][2], s_da[kEpiRows][2];
  __shared__ double s_bound[kEpiTile];  // this line and the next: read by the epipolar form alone, gone from the other
  __shared__ float s_x[kEpiTile], s_y[kEpiTile], s_gate[kEpiTile], s_ax[kEpiRows], s_ay[kEpiRows];
  __shared__ int s_flag[kEpiTile], s_ra[kEpiRows], s_aflag[kEpiRows];
  __shared__ uint32_t s_key[kEpiRows];
  const int sr = tid >> 1, sh = tid & 1;  // staging: thread = (row, descriptor half)
  int staged = -1;                        // first KF2 row of the tile in LDS (block-uniform)
  for (int a0 = 0; a0 < na; a0 += kEpiRows) {
    const int rows = min(kEpiRows, na - a0);
    __syncthreads();  // every wave is done with the chunk before
    if (sr < rows) {  // the chunk's KF1 side in one round of loads
      const int ra = idxA[np.a_begin + a0 + sr];
      s_da[sr][sh] = ((const uint4 *)(descA + (size_t)ra * 32))[sh];
      if (sh == 0) {
        s_ra[sr] = ra, s_key[sr] = KEY_NONE;
        if constexpr (kEpi) {
          const vsg::KeyPointPOD kp = q.A.kps[ra];
          const bool stereo1 = q.A.uright && q.A.uright[ra] >= 0;
          s_ax[sr] = kp.x, s_ay[sr] = kp.y;
          // -1: has a map point (:969-973), or mono under bOnlyStereo (:976-980): the row is not walked
          s_aflag[sr] = (!q.A.no_mp[ra] || (q.P.only_stereo && !stereo1)) ? -1 : (stereo1 ? kEpiStereo : 0);
        } else {
          s_aflag[sr] = q.eligible1[ra] ? 0 : -1;
        }
      }
    }
    __syncthreads();
    for (int t0 = 0; t0 < nb; t0 += kEpiTile) {
      const int nt = min(kEpiTile, nb - t0);
      if (staged != t0) {
        if (staged >= 0) __syncthreads();  // every wave is done with the tile before
        if (sr < nt) {
          const int rb = idxB[np.b_begin + t0 + sr];
          s_d[sr][sh] = ((const uint4 *)(descB + (size_t)rb * 32))[sh];
          if (sh == 0) {
            if constexpr (kEpi) {
              const vsg::KeyPointPOD kp = q.B.kps[rb];
              const int lv = kp.octave & 15;  // the host checked [0, nlevels) on its mirror; the tables have 16 entries
              s_x[sr] = kp.x, s_y[sr] = kp.y, s_gate[sr] = q.P.gate[lv], s_bound[sr] = q.P.bound[lv];
              s_flag[sr] = ((q.B.uright && q.B.uright[rb] >= 0) ? kEpiStereo : 0) | (q.B.no_mp[rb] ? 0 : kEpiHasMp);
            } else {
              s_flag[sr] = q.eligible2[rb];
            }
          }
        }
        staged = t0;
        __syncthreads();
      }
      for (int r = wave; r < rows; r += 4) {  // wave-uniform; row r belongs to wave r & 3
        const int af = s_aflag[r];
        if (af < 0) continue;
        vsg::EpipolarLine line = {0.0f, 0.0f, 0.0f, 0.0f};
        int bit0 = 0;  // the row's first bit
        if constexpr (kEpi) {
          if (!q.P.coarse) line = vsg::epipolar_line(q.P.F12, s_ax[r], s_ay[r]);
        } else if (q.bits) {
          bit0 = q.pair_off[node] + (a0 + r) * nb + t0;
        }
        const uint4 d0 = s_da[r][0], d1 = s_da[r][1];
        uint32_t k = KEY_NONE;
        for (int j = lane; j < nt; j += 64) {
          const int fl = s_flag[j];
          if constexpr (kEpi) {
            if (fl & kEpiHasMp) continue;  // :1001-1002
            if (vsg::epipolar_reason(line, af != 0, s_x[j], s_y[j], (fl & kEpiStereo) != 0, q.P.ep[0], q.P.ep[1], s_gate[j],
                                     s_bound[j], q.P.only_stereo, q.P.coarse) != vsg::kEpiPass)
              continue;
          } else {
            if (!fl) continue;
            if (q.bits && !((q.bits[(bit0 + j) >> 5] >> ((bit0 + j) & 31)) & 1u)) continue;
          }
          const int dist = hamming256(d0, d1, s_d[j][0], s_d[j][1]);
          if (dist > TH_LOW) continue;  // :1014
          k = min(k, ((uint32_t)dist << 20) | (0xFFFFFu - (uint32_t)(t0 + j)));
        }
        k = wave_min(k);
        if (lane == 0) s_key[r] = min(s_key[r], k);  // the owner wave's own entry: no other wave reads or writes it
      }
    }
    // the chunk's matches: a wave writes the rows it owns (what its lane 0 left in s_key: same wave, program order)
    for (int r = wave + 4 * lane; r < rows; r += 256) {
      const uint32_t k = s_key[r];
      if (k != KEY_NONE) matches12[s_ra[r]] = idxB[np.b_begin + (int)(0xFFFFFu - (k & 0xFFFFFu))];
    }
  }
}

// test hook (vsg_debug_epipolar_pairs): the device predicate on listed pairs, one lane per pair
__global__ __launch_bounds__(256) void k_epipolar_pairs(int n, const int *i1, const int *i2, EpiFrame A, EpiFrame B,
                                                        EpiParams P, uint8_t *reason) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const int ra = i1[p], rb = i2[p];
  const vsg::KeyPointPOD k1 = A.kps[ra], k2 = B.kps[rb];
  vsg::EpipolarLine line = {0.0f, 0.0f, 0.0f, 0.0f};
  if (!P.coarse) line = vsg::epipolar_line(P.F12, k1.x, k1.y);
  const int lv = k2.octave & 15;
  reason[p] = (uint8_t)vsg::epipolar_reason(line, A.uright && A.uright[ra] >= 0, k2.x, k2.y, B.uright && B.uright[rb] >= 0,
                                            P.ep[0], P.ep[1], P.gate[lv], P.bound[lv], P.only_stereo, P.coarse);
}

// ---- windowed searches on HOST candidate lists (the caller ran GetFeaturesInArea itself): every candidate entry's
// Hamming distance in ONE data-parallel pass, written as the packed entry the ordered host passes read
// (vsg_walks.h: index | distance << 15 | octave << 24).  The walk over the queries that follows is inherently
// sequential (a claimed feature blocks later queries) and touches a dozen candidates per query: it runs on the host
// over these entries, like the reference's own loop -- the first version walked the queries with a single wavefront
// on the device and took 1.3 ms for 1000 queries, 25x the CPU.  (Resident frames: k_window_search, vsg_window.hip.)
__global__ __launch_bounds__(256) void k_cand_dist(const uint8_t *qDesc, const int *qOf, const int *candIdx,
                                                   const uint8_t *tDesc, const uint8_t *tOct, int ncand,
                                                   uint32_t *ent) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncand) return;
  uint4 a0, a1, b0, b1;
  const int i = candIdx[c];
  load_desc(qDesc, qOf[c], a0, a1);
  load_desc(tDesc, i, b0, b1);
  ent[c] = (uint32_t)i | ((uint32_t)hamming256(a0, a1, b0, b1) << 15) | ((uint32_t)(tOct ? tOct[i] & 15 : 0) << 24);
}

// ---- MapPoint::ComputeDistinctiveDescriptors (MapPoint.cc:380-415): one workgroup per map point.  The N x N
// distance matrix lives in LDS; thread i finds the element of rank floor(0.5*(N-1)) of row i by counting (no
// sort needed: the median VALUE does not depend on how ties are ordered); the first row with the least median
// wins (strict '<').
enum { kDistinctMaxN = 128 };
__global__ __launch_bounds__(128) void k_distinctive(const uint8_t *desc, const int *off, int *best) {
  __shared__ uint16_t D[kDistinctMaxN * kDistinctMaxN];
  __shared__ uint32_t s_key[kDistinctMaxN];
  const int g = blockIdx.x, tid = threadIdx.x;
  const int o = off[g], N = off[g + 1] - o;
  if (N <= 0) {
    if (tid == 0) best[g] = -1;
    return;
  }
  for (int i = tid; i < N; i += 128) {
    uint4 a0, a1;
    load_desc(desc, o + i, a0, a1);
    for (int j = 0; j < N; j++) {
      uint4 b0, b1;
      load_desc(desc, o + j, b0, b1);
      D[i * N + j] = (uint16_t)hamming256(a0, a1, b0, b1);
    }
  }
  __syncthreads();
  const int k = (int)(0.5 * (N - 1));
  for (int i = tid; i < N; i += 128) {
    int median = 0;
    for (int j = 0; j < N; j++) {
      const int v = D[i * N + j];
      int less = 0, le = 0;
      for (int t = 0; t < N; t++) {
        const int x = D[i * N + t];
        less += x < v;
        le += x <= v;
      }
      if (less <= k && k < le) median = v;
    }
    s_key[i] = ((uint32_t)median << 16) | (uint32_t)i;  // smallest key = least median, first index
  }
  __syncthreads();
  if (tid == 0) {
    uint32_t b = 0xFFFFFFFFu;
    for (int i = 0; i < N; i++) b = min(b, s_key[i]);
    best[g] = (int)(b & 0xFFFF);
  }
}

// ------------------------------------------------------------------------------------------------ host side
// Every entry point runs on the calling thread's stream and stages through its arenas (vsg_ctx.h): inputs are laid
// out in the pinned arena and go up in ONE DMA into the device arena (they are read many times by the kernels),
// results come back through the pinned arena.  No allocation, no NULL-stream launch in steady state.

using vsg::ThreadCtx;
using vsg::Stage;
namespace walk = vsg::walk;

// Packed candidate entries (vsg_walks.h) for host-provided CSR candidate lists.  On return *ent points into the
// calling thread's pinned arena (valid until its next call).
static int candidate_entries(int device, const uint8_t *q_desc, int n_q, const int32_t *cand_off,
                             const int32_t *cand_idx, const uint8_t *t_desc, const int32_t *t_octave, int n_t,
                             const uint32_t **ent) {
  int rc = VSG_OK;
  ThreadCtx *c = vsg::thread_ctx(device, &rc);
  if (!c) return rc;
  const int ncand = cand_off[n_q];
  *ent = nullptr;
  if (ncand == 0) return VSG_OK;
  if (n_t > 32767) return VSG_ERR_UNSUPPORTED;
  for (int k = 0; k < ncand; k++)
    if (cand_idx[k] < 0 || cand_idx[k] >= n_t) return VSG_ERR_INVALID;
  Stage st;
  const size_t oQ = st.add((size_t)n_q * 32), oT = st.add((size_t)n_t * 32), oOct = st.add(t_octave ? (size_t)n_t : 0),
               oOf = st.add((size_t)ncand * 4), oIdx = st.add((size_t)ncand * 4);
  const size_t in_bytes = st.total;
  const size_t oEnt = st.add((size_t)ncand * 4);
  rc = vsg::ctx_reserve(c, st.total, in_bytes);
  if (rc != VSG_OK) return rc;
  uint8_t *h = c->h_pin;
  memcpy(h + oQ, q_desc, (size_t)n_q * 32);
  memcpy(h + oT, t_desc, (size_t)n_t * 32);
  if (t_octave)
    for (int i = 0; i < n_t; i++) h[oOct + i] = (uint8_t)t_octave[i];
  int32_t *qof = (int32_t *)(h + oOf);
  for (int q = 0; q < n_q; q++)
    for (int k = cand_off[q]; k < cand_off[q + 1]; k++) qof[k] = q;
  memcpy(h + oIdx, cand_idx, (size_t)ncand * 4);
  TRY_HIP(hipMemcpyAsync(c->d_buf, h, in_bytes, hipMemcpyHostToDevice, c->stream));
  const uint8_t *d = c->d_buf;
  hipLaunchKernelGGL(k_cand_dist, dim3((ncand + 255) / 256), dim3(256), 0, c->stream, d + oQ, (const int *)(d + oOf),
                     (const int *)(d + oIdx), d + oT, t_octave ? d + oOct : (const uint8_t *)nullptr, ncand,
                     (uint32_t *)(c->d_pin + oEnt));
  TRY_HIP(hipGetLastError());
  TRY_HIP(hipStreamSynchronize(c->stream));
  *ent = (const uint32_t *)(h + oEnt);
  return VSG_OK;
}

static walk::CandView csr_view(const uint32_t *ent, const int32_t *cand_off) {
  walk::CandView cv;
  cv.ent = ent;
  cv.off = cand_off;
  return cv;
}

// rotation-consistency filter of the BoW / triangulation searches: every match sits in exactly one bin
template <class AngleA, class AngleB>
static int bow_rotation_filter(int *out, int nOut, int mode, AngleA angleA, AngleB angleB, bool checkOri) {
  int nmatches = 0;
  std::vector<int> rotHist[HISTO_LENGTH];
  for (int i = 0; i < nOut; i++) {
    if (out[i] < 0) continue;
    nmatches++;
    if (checkOri) {
      const int bin = mode == 0 ? walk::rot_bin(angleA(out[i]), angleB(i)) : walk::rot_bin(angleA(i), angleB(out[i]));
      rotHist[bin].push_back(i);
    }
  }
  if (checkOri)
    walk::filter_rotation(rotHist, [&](int i) {
      out[i] = -1;
      nmatches--;
    });
  return nmatches;
}

// The buffers of one call in an arena: each is named ONCE, so the size it is laid out with is the size it is copied with
struct Upload {
  enum { kMax = 10 };
  Stage st;
  const void *src[kMax];
  size_t bytes[kMax], at[kMax];
  int n = 0;
  size_t add(const void *s, size_t b) {  // s == nullptr: laid out and left to the caller
    if (n == kMax) abort();
    src[n] = s, bytes[n] = b;
    return at[n++] = st.add(b);
  }
  void fill(uint8_t *base) const {
    for (int i = 0; i < n; i++)
      if (src[i] && bytes[i]) memcpy(base + at[i], src[i], bytes[i]);
  }
};

// ---- the node searches on FeatureVectors given as HOST arrays.  One side of such a call: its descriptors and angles are
// host arrays (the descriptors are staged) or those of a resident frame (d_desc, and the angles of its host mirror)
struct HostSide {
  int n;
  const uint8_t *desc, *d_desc;
  const float *angle;
  const vsg_keypoint *kps;
  const uint8_t *flags;  // valid / eligible per feature; nullptr: the side has none (the Frame of KF -> F)
  vsg::FvView fv;
  float angle_of(int i) const { return angle ? angle[i] : kps[i].angle; }
};
static HostSide frame_side(const vsg_frame *f, const uint8_t *flags, const int32_t *node_id, const int32_t *off,
                           const int32_t *idx, int nodes) {
  return HostSide{f->n, nullptr, f->d_desc, nullptr, f->h_kps.data(), flags, {node_id, off, idx, nodes}};
}

// One such search from the checks to the rotation filter.  mode 0 / 1: SearchByBoW KF -> F (the output is per feature of B:
// match_f) / KF -> KF (per feature of A: matches12); mode 2: SearchForTriangulation (matches12; pair_ok / pair_off).
// Everything that can be refused is refused FIRST, with VSG_ERR_INVALID: before thread_ctx is called, before anything is
// enqueued and before the output is written.  The kernels index the frames with idx and the bits with pair_off: what
// vsg_fv.h refuses never reaches the device.
static int node_search(int device, int mode, int nleftB, float nnratio, const HostSide &A, const HostSide &B,
                       const uint32_t *pair_ok, const int32_t *pair_off, int check_orientation, int32_t *out) {
  for (const HostSide *s : {&A, &B})
    if (s->n < 0 || (s->n > 0 && ((!s->desc && !s->d_desc) || (!s->angle && !s->kps))) || !vsg::fv_check(s->fv, s->n))
      return VSG_ERR_INVALID;
  if ((A.n > 0 && !A.flags) || (mode != 0 && B.n > 0 && !B.flags) || (pair_ok && !pair_off)) return VSG_ERR_INVALID;
  std::vector<NodePair> pairs;
  vsg::join_nodes(A.fv.node_id, A.fv.off, A.fv.nodes, B.fv.node_id, B.fv.off, B.fv.nodes, pairs);
  if (pair_ok && !vsg::pair_bits_check(pairs, pair_off)) return VSG_ERR_INVALID;
  int rc = VSG_OK;
  ThreadCtx *c = vsg::thread_ctx(device, &rc);
  if (!c) return rc;
  const int nOut = mode == 0 ? B.n : A.n, npairs = (int)pairs.size();
  for (int i = 0; i < nOut; i++) out[i] = -1;
  if (pairs.empty() || A.n == 0 || B.n == 0) return 0;
  // The join's pairs, both sides' flags and lists, host descriptors and the predicate bits (the last node's end at
  // pair_off[npairs]) go up in ONE DMA: the kernels read them many times.  Behind them the output and BoW's claim scratch.
  Upload up;
  const size_t oP = up.add(pairs.data(), pairs.size() * sizeof(NodePair)), oFA = up.add(A.flags, (size_t)A.n),
               oIA = up.add(A.fv.idx, (size_t)A.fv.off[A.fv.nodes] * 4), oFB = up.add(B.flags, B.flags ? (size_t)B.n : 0),
               oIB = up.add(B.fv.idx, (size_t)B.fv.off[B.fv.nodes] * 4), oDA = up.add(A.desc, A.d_desc ? 0 : (size_t)A.n * 32),
               oDB = up.add(B.desc, B.d_desc ? 0 : (size_t)B.n * 32),
               oOk = up.add(pair_ok, pair_ok ? ((size_t)pair_off[npairs] + 31) / 32 * 4 : 0),
               oOff = up.add(pair_ok ? pair_off : nullptr, pair_ok ? (size_t)(npairs + 1) * 4 : 0);
  const size_t in_bytes = up.st.total, oOut = up.st.add((size_t)nOut * 4), pin_bytes = up.st.total;
  const size_t oClaim = up.st.add(mode == 2 ? 0 : (size_t)B.n * 4);
  rc = vsg::ctx_reserve(c, pin_bytes, up.st.total);
  if (rc != VSG_OK) return rc;
  uint8_t *h = c->h_pin, *d = c->d_buf;
  up.fill(h);
  TRY_HIP(hipMemcpyAsync(d, h, in_bytes, hipMemcpyHostToDevice, c->stream));
  TRY_HIP(hipMemsetAsync(d + oOut, 0xFF, (size_t)nOut * 4, c->stream));  // -1: the kernels only write matches
  const uint8_t *dA = A.d_desc ? A.d_desc : d + oDA, *dB = B.d_desc ? B.d_desc : d + oDB;
  if (mode == 2)
    hipLaunchKernelGGL(k_triangulation_walk<CallerBitsPred>, dim3(npairs), dim3(256), 0, c->stream, (const NodePair *)(d + oP),
                       npairs, FvDev{}, FvDev{}, (const int *)(d + oIA), (const int *)(d + oIB),
                       CallerBitsPred{dA, d + oFA, dB, d + oFB, pair_ok ? (const uint32_t *)(d + oOk) : nullptr,
                                      (const int *)(d + oOff)},
                       (int *)(d + oOut));
  else
    hipLaunchKernelGGL(k_search_by_bow, dim3(npairs), dim3(256), 0, c->stream, (const NodePair *)(d + oP), npairs, FvDev{},
                       FvDev{}, dA, d + oFA, (const int *)(d + oIA), dB, d + oFB, (const int *)(d + oIB), nnratio, mode, nleftB,
                       (int *)(d + oOut), (int *)(d + oClaim));
  TRY_HIP(hipGetLastError());
  TRY_HIP(hipMemcpyAsync(h + oOut, d + oOut, (size_t)nOut * 4, hipMemcpyDeviceToHost, c->stream));
  TRY_HIP(hipStreamSynchronize(c->stream));
  memcpy(out, h + oOut, (size_t)nOut * 4);
  // rotation consistency (:407-425 / :879-897)
  return bow_rotation_filter(out, nOut, mode == 0 ? 0 : 1, [&](int i) { return A.angle_of(i); },
                             [&](int i) { return B.angle_of(i); }, check_orientation != 0);
}

// ---- SearchByBoW on two frames whose descriptors AND FeatureVectors are resident (round 6): nothing but the KeyFrame's
// "has a map point" flags goes up, the join runs in the kernel, and the call comes in two halves so that it can share one
// wait with the ComputeStereoMatches / ComputeBoW of the same Frame (vsg_chain.hip).
}  // namespace (reopened below: the two halves are called from vsg_chain.hip)
namespace vsg {

void bow_search_sizes(int nA, int nB, int mode, size_t *pin_bytes, size_t *dev_bytes) {
  Stage p, d;
  p.add((size_t)nA), p.add(mode == 1 ? (size_t)nB : 0), p.add(4 * (size_t)(mode == 0 ? nB : nA) + 64);
  d.add(4 * (size_t)nB + 64);
  *pin_bytes = p.total, *dev_bytes = d.total;
}

// ONE launch and nothing else on the stream: the flags are read and the matches written where they lie in the pinned arena
// (a few hundred scattered bytes each way over PCIe, in parallel over the node waves) -- the DMA of the flags, the fill of the
// match array and its copy back cost 4.4 us of stream time EACH (rocprofv3: __amd_rocclr_copyBuffer / fillBufferAligned).
int bow_search_enqueue(BowSearchCall *s, int mode, vsg_frame *A, const uint8_t *validA, vsg_frame *B, const uint8_t *validB,
                       float nnratio, ThreadCtx *c, size_t pin_base, size_t dev_base) {
  s->c = c, s->mode = mode, s->A = A, s->B = B, s->active = false, s->pin_base = pin_base;
  s->nOut = mode == 0 ? B->n : A->n;
  // an empty frame has an empty FeatureVector whatever ComputeBoW left: no shared node, 0 matches (ORBmatcher.cc:247)
  if (A->n == 0 || B->n == 0) return VSG_OK;
  if (!A->fv_valid || !B->fv_valid) return VSG_ERR_INVALID;  // ComputeBoW first (Frame.cc:882-889)
  if (A->fv_empty || B->fv_empty) return VSG_OK;             // ComputeBoW with an empty() vocabulary left no node
  const int nA = A->n, nB = B->n;
  Upload p;  // the layout of bow_search_sizes
  const size_t oVA = p.add(validA, (size_t)nA), oVB = p.add(mode == 1 ? validB : nullptr, mode == 1 ? (size_t)nB : 0);
  s->oOut = p.add(nullptr, 4 * (size_t)s->nOut + 64);
  uint8_t *hp = c->h_pin + pin_base, *dp = c->d_pin + pin_base;
  p.fill(hp);
  memset(hp + s->oOut, 0xFF, 4 * (size_t)s->nOut);  // -1: the kernel only writes matches
  const int blocks = A->fv_bound > 0 ? A->fv_bound : 1;
  hipLaunchKernelGGL(k_search_by_bow, dim3(blocks), dim3(256), 0, c->stream, (const NodePair *)nullptr, 0, vsg::fv_dev(A),
                     vsg::fv_dev(B), A->d_desc, dp + oVA, (const int *)nullptr, B->d_desc, dp + oVB, (const int *)nullptr,
                     nnratio, mode, mode == 0 ? B->nleft : -1, (int *)(dp + s->oOut), (int *)(c->d_buf + dev_base));
  TRY_HIP(hipGetLastError());
  s->active = true;
  return VSG_OK;
}

// after the stream has been waited for: the matches + the rotation-consistency filter (:407-425 / :879-897)
int bow_search_finish(BowSearchCall *s, int check_orientation, int32_t *out) {
  for (int i = 0; i < s->nOut; i++) out[i] = -1;
  if (!s->active) return 0;
  memcpy(out, s->c->h_pin + s->pin_base + s->oOut, 4 * (size_t)s->nOut);
  const vsg_keypoint *ka = s->A->h_kps.data(), *kb = s->B->h_kps.data();
  return bow_rotation_filter(out, s->nOut, s->mode, [&](int i) { return ka[i].angle; }, [&](int i) { return kb[i].angle; },
                             check_orientation != 0);
}

}  // namespace vsg
namespace {

static int search_by_bow_resident(int mode, vsg_frame *A, const uint8_t *validA, vsg_frame *B, const uint8_t *validB,
                                  float nnratio, int check_orientation, int32_t *out) {
  int rc = VSG_OK;
  ThreadCtx *c = vsg::thread_ctx(A->device, &rc);
  if (!c) return rc;
  size_t pin = 0, dev = 0;
  vsg::bow_search_sizes(A->n, B->n, mode, &pin, &dev);
  rc = vsg::ctx_reserve(c, pin, dev);
  if (rc != VSG_OK) return rc;
  vsg::BowSearchCall s;
  rc = vsg::bow_search_enqueue(&s, mode, A, validA, B, validB, nnratio, c, 0, 0);
  if (rc != VSG_OK) {
    hipStreamSynchronize(c->stream);  // nothing this call launched outlives it (the next call rewrites the arena)
    return rc;
  }
  if (s.active) TRY_HIP(hipStreamSynchronize(c->stream));
  return vsg::bow_search_finish(&s, check_orientation, out);
}

// the per-call constants of the epipolar predicate: F12, ep and the two per-level tables of pKF2 (vsg_epipolar.h)
static EpiParams epi_params(const float *F12, const float *ep, const float *scale_factors2, const float *level_sigma2_2,
                            int nlevels, int only_stereo, int coarse) {
  EpiParams P;
  memset(&P, 0, sizeof P);
  memcpy(P.F12, F12, sizeof P.F12);
  P.ep[0] = ep[0], P.ep[1] = ep[1];
  for (int l = 0; l < nlevels; l++)
    P.gate[l] = vsg::epipole_gate_radius(scale_factors2[l]), P.bound[l] = vsg::chi_square_bound(level_sigma2_2[l]);
  P.only_stereo = only_stereo != 0, P.coarse = coarse != 0;
  return P;
}
static bool octaves_within(const vsg_frame *f, int nlevels) {
  for (const vsg_keypoint &k : f->h_kps)
    if (k.octave < 0 || k.octave >= nlevels) return false;
  return true;
}
static EpiFrame epi_frame(const vsg_frame *f, const uint8_t *no_mp) {
  return EpiFrame{f->d_kps, f->d_desc, f->has_uright ? f->d_uright : (const float *)nullptr, no_mp};
}

}  // namespace

// ---- the epipolar search in two halves (vsg_frame_int.h), shared by vsg_frame_search_for_triangulation_epipolar and
// vsg_frame_create_new_map_points (vsg_triangulate.hip)
namespace vsg {

// everything that can be refused is refused here, before anything is enqueued
int epipolar_search_check(const EpiSearchArgs &a, const int32_t *matches12) {
  vsg_frame *kf1 = a.kf1, *kf2 = a.kf2;
  if (vsg::frame_check(kf1) != VSG_OK || vsg::frame_check(kf2) != VSG_OK || kf1->device != kf2->device || !a.F12 || !a.ep ||
      !a.scale_factors2 || !a.level_sigma2_2 || a.nlevels < 1 || a.nlevels > 16 || (!matches12 && kf1->n > 0) ||
      (!a.no_mp1 && kf1->n > 0) || (!a.no_mp2 && kf2->n > 0))
    return VSG_ERR_INVALID;
  if (kf1->nleft != -1 || kf2->nleft != -1) return VSG_ERR_UNSUPPORTED;  // mpCamera2 (:929-937, :1033-1071)
  if (!octaves_within(kf2, a.nlevels)) return VSG_ERR_INVALID;
  const bool resident_fv = !a.node_id1 && !a.off1 && !a.idx1 && !a.node_id2 && !a.off2 && !a.idx2;
  if (!resident_fv) {
    if (!a.node_id1 || !a.off1 || !a.idx1 || !a.node_id2 || !a.off2 || !a.idx2) return VSG_ERR_INVALID;
    // the kernel indexes the frames with these: an index outside a frame never reaches the device
    const vsg::FvView v1{a.node_id1, a.off1, a.idx1, a.nodes1}, v2{a.node_id2, a.off2, a.idx2, a.nodes2};
    if (!vsg::fv_check(v1, kf1->n) || !vsg::fv_check(v2, kf2->n)) return VSG_ERR_INVALID;
  }
  // ComputeBoW first (Frame.cc:882-889); an empty frame has an empty FeatureVector whatever ComputeBoW left
  if (resident_fv && kf1->n > 0 && kf2->n > 0 && (!kf1->fv_valid || !kf2->fv_valid)) return VSG_ERR_INVALID;
  return VSG_OK;
}

// After the check: lays the call out in the calling thread's pinned arena with `extra_bytes` for the caller behind it (at
// s->oExtra) and enqueues the walk.  s->launched == false: no launch was needed, every match is -1 (and when
// extra_bytes != 0 the arena still holds the caller's block).  The caller looks at hipGetLastError and waits.
int epipolar_search_enqueue(EpiSearch *s, const EpiSearchArgs &a, size_t extra_bytes) {
  vsg_frame *kf1 = a.kf1, *kf2 = a.kf2;
  const int n1 = kf1->n, n2 = kf2->n;
  s->n1 = n1, s->launched = false;
  const bool resident_fv = !a.node_id1;
  std::vector<NodePair> pairs;
  bool empty = n1 == 0 || n2 == 0;  // no shared node, 0 matches (ORBmatcher.cc:961)
  if (!empty) {
    if (resident_fv) {
      empty = kf1->fv_empty || kf2->fv_empty;  // ComputeBoW with an empty() vocabulary left no node
    } else {
      vsg::join_nodes(a.node_id1, a.off1, a.nodes1, a.node_id2, a.off2, a.nodes2, pairs);
      empty = pairs.empty();
    }
  }
  if (empty && !extra_bytes) return VSG_OK;
  int rc = VSG_OK;
  ThreadCtx *c = s->c = vsg::thread_ctx(kf1->device, &rc);
  if (!c) return rc;
  // ONE launch and nothing else on the stream (as bow_search_enqueue): the flags and lists are read and the matches written
  // where they lie in the pinned arena
  const int npairs = (int)pairs.size();
  Upload up;
  const size_t oF1 = up.add(a.no_mp1, (size_t)n1), oF2 = up.add(a.no_mp2, (size_t)n2),
               oP = up.add(pairs.data(), pairs.size() * sizeof(NodePair)),
               oI1 = up.add(a.idx1, resident_fv ? 0 : (size_t)a.off1[a.nodes1] * 4),
               oI2 = up.add(a.idx2, resident_fv ? 0 : (size_t)a.off2[a.nodes2] * 4), oM = up.add(nullptr, (size_t)n1 * 4);
  s->oM = oM, s->oExtra = up.st.add(extra_bytes);
  rc = vsg::ctx_reserve(c, up.st.total, 0);
  if (rc != VSG_OK) return rc;
  uint8_t *h = c->h_pin, *d = c->d_pin;
  up.fill(h);
  memset(h + oM, 0xFF, (size_t)n1 * 4);  // -1: the kernel only writes matches
  if (empty) return VSG_OK;
  const EpipolarPred pred{epi_frame(kf1, d + oF1), epi_frame(kf2, d + oF2),
                          epi_params(a.F12, a.ep, a.scale_factors2, a.level_sigma2_2, a.nlevels, a.only_stereo, a.coarse)};
  const int blocks = resident_fv ? (kf1->fv_bound > 0 ? kf1->fv_bound : 1) : npairs;
  hipLaunchKernelGGL(k_triangulation_walk<EpipolarPred>, dim3(blocks), dim3(256), 0, c->stream,
                     resident_fv ? (const NodePair *)nullptr : (const NodePair *)(d + oP), npairs,
                     resident_fv ? vsg::fv_dev(kf1) : FvDev{}, resident_fv ? vsg::fv_dev(kf2) : FvDev{},
                     (const int *)(d + oI1), (const int *)(d + oI2), pred, (int *)(d + oM));
  s->launched = true;
  return VSG_OK;
}

}  // namespace vsg

extern "C" {

int vsg_frame_search_for_triangulation_epipolar(vsg_frame *kf1, const uint8_t *no_mp1, const int32_t *node_id1,
                                                const int32_t *off1, const int32_t *idx1, int nodes1, vsg_frame *kf2,
                                                const uint8_t *no_mp2, const int32_t *node_id2, const int32_t *off2,
                                                const int32_t *idx2, int nodes2, const float F12[9], const float ep[2],
                                                const float *scale_factors2, const float *level_sigma2_2, int nlevels,
                                                int only_stereo, int coarse, int check_orientation, int32_t *matches12) {
  const vsg::EpiSearchArgs a{kf1, no_mp1, node_id1, off1, idx1, nodes1, kf2, no_mp2, node_id2, off2, idx2, nodes2, F12, ep,
                             scale_factors2, level_sigma2_2, nlevels, only_stereo, coarse};
  int rc = vsg::epipolar_search_check(a, matches12);
  if (rc != VSG_OK) return rc;
  const int n1 = kf1->n;
  for (int i = 0; i < n1; i++) matches12[i] = -1;  // no output is touched before the last refusal
  vsg::EpiSearch s;
  rc = vsg::epipolar_search_enqueue(&s, a, 0);
  if (rc != VSG_OK) return rc;
  if (!s.launched) return 0;
  const hipError_t launched = hipGetLastError(), waited = hipStreamSynchronize(s.c->stream);  // an error still waits
  if (launched != hipSuccess || waited != hipSuccess) return VSG_ERR_HIP;
  memcpy(matches12, s.c->h_pin + s.oM, (size_t)n1 * 4);
  const vsg_keypoint *ka = kf1->h_kps.data(), *kb = kf2->h_kps.data();
  return bow_rotation_filter(matches12, n1, 1, [&](int i) { return ka[i].angle; }, [&](int i) { return kb[i].angle; },
                             check_orientation != 0);
}

int vsg_debug_epipolar_pairs(vsg_frame *kf1, vsg_frame *kf2, int n, const int32_t *i1, const int32_t *i2,
                             const float F12[9], const float ep[2], const float *scale_factors2,
                             const float *level_sigma2_2, int nlevels, int only_stereo, int coarse, uint8_t *reason) {
  if (vsg::frame_check(kf1) != VSG_OK || vsg::frame_check(kf2) != VSG_OK || kf1->device != kf2->device || n < 0 ||
      (n > 0 && (!i1 || !i2 || !reason)) || !F12 || !ep || !scale_factors2 || !level_sigma2_2 || nlevels < 1 || nlevels > 16)
    return VSG_ERR_INVALID;
  if (kf1->nleft != -1 || kf2->nleft != -1) return VSG_ERR_UNSUPPORTED;
  if (!octaves_within(kf2, nlevels)) return VSG_ERR_INVALID;
  for (int p = 0; p < n; p++)
    if (i1[p] < 0 || i1[p] >= kf1->n || i2[p] < 0 || i2[p] >= kf2->n) return VSG_ERR_INVALID;
  if (n == 0) return VSG_OK;
  int rc = VSG_OK;
  ThreadCtx *c = vsg::thread_ctx(kf1->device, &rc);
  if (!c) return rc;
  Stage st;
  const size_t o1 = st.add((size_t)n * 4), o2 = st.add((size_t)n * 4), oR = st.add((size_t)n);
  rc = vsg::ctx_reserve(c, st.total, 0);
  if (rc != VSG_OK) return rc;
  uint8_t *h = c->h_pin, *d = c->d_pin;
  memcpy(h + o1, i1, (size_t)n * 4);
  memcpy(h + o2, i2, (size_t)n * 4);
  const EpiParams P = epi_params(F12, ep, scale_factors2, level_sigma2_2, nlevels, only_stereo, coarse);
  hipLaunchKernelGGL(k_epipolar_pairs, dim3((n + 255) / 256), dim3(256), 0, c->stream, n, (const int *)(d + o1),
                     (const int *)(d + o2), epi_frame(kf1, nullptr), epi_frame(kf2, nullptr), P, d + oR);
  const hipError_t launched = hipGetLastError(), waited = hipStreamSynchronize(c->stream);
  if (launched != hipSuccess || waited != hipSuccess) return VSG_ERR_HIP;
  memcpy(reason, h + oR, (size_t)n);
  return VSG_OK;
}

int vsg_hamming_pairs(int device, const uint8_t *a, int na, const uint8_t *b, int nb, const int32_t *ia,
                      const int32_t *ib, int npairs, int32_t *dist) {
  if (!a || !b || !ia || !ib || !dist || npairs < 0 || na < 0 || nb < 0) return VSG_ERR_INVALID;
  int rc = VSG_OK;
  ThreadCtx *c = vsg::thread_ctx(device, &rc);
  if (!c) return rc;
  if (npairs == 0) return VSG_OK;
  Stage st;
  const size_t oA = st.add((size_t)na * 32), oB = st.add((size_t)nb * 32), oIA = st.add((size_t)npairs * 4),
               oIB = st.add((size_t)npairs * 4);
  const size_t in_bytes = st.total;
  const size_t oD = st.add((size_t)npairs * 4);
  rc = vsg::ctx_reserve(c, st.total, in_bytes);
  if (rc != VSG_OK) return rc;
  uint8_t *h = c->h_pin;
  memcpy(h + oA, a, (size_t)na * 32);
  memcpy(h + oB, b, (size_t)nb * 32);
  memcpy(h + oIA, ia, (size_t)npairs * 4);
  memcpy(h + oIB, ib, (size_t)npairs * 4);
  TRY_HIP(hipMemcpyAsync(c->d_buf, h, in_bytes, hipMemcpyHostToDevice, c->stream));
  const uint8_t *d = c->d_buf;
  hipLaunchKernelGGL(k_hamming_pairs, dim3((npairs + 255) / 256), dim3(256), 0, c->stream, d + oA, d + oB,
                     (const int *)(d + oIA), (const int *)(d + oIB), npairs, (int *)(c->d_pin + oD));
  TRY_HIP(hipGetLastError());
  TRY_HIP(hipStreamSynchronize(c->stream));
  memcpy(dist, h + oD, (size_t)npairs * 4);
  return VSG_OK;
}

int vsg_hamming_block_best2_device(int device, const uint8_t *d_a, const uint8_t *d_b, size_t block_stride_bytes,
                                   const int32_t *d_counts_a, const int32_t *d_counts_b, int count_stride,
                                   int nblocks, int max_rows, int32_t *d_best, int32_t *d_second,
                                   int32_t *d_argbest, void *stream) {
  if (!d_a || !d_b || !d_best || !d_second || !d_argbest || nblocks < 1 || max_rows < 1) return VSG_ERR_INVALID;
  // the packed key has 20 bits for the train row, gridDim.y carries the block
  if (max_rows > (1 << 20) || nblocks > 65535) return VSG_ERR_UNSUPPORTED;
  if (vsg::use_device(device) != VSG_OK) return VSG_ERR_NO_DEVICE;
  dim3 grid((max_rows + kBest2Rows - 1) / kBest2Rows, nblocks);
  // stream == NULL is the caller's NULL stream (see vsg_orb_extract_batch_device for how the extractor orders itself
  // against it)
  hipLaunchKernelGGL(k_block_best2_mfma, grid, dim3(256), 0, (hipStream_t)stream, d_a, d_b, block_stride_bytes,
                     d_counts_a, d_counts_b, count_stride, max_rows, max_rows, max_rows, d_best, d_second, d_argbest);
  TRY_HIP(hipGetLastError());
  return VSG_OK;
}

int vsg_hamming_block_best2(int device, const uint8_t *a, int na, const uint8_t *b, int nb, int32_t *best,
                            int32_t *second, int32_t *argbest) {
  if (!a || !b || !best || !second || !argbest || na < 0 || nb < 0) return VSG_ERR_INVALID;
  int rc = VSG_OK;
  ThreadCtx *c = vsg::thread_ctx(device, &rc);
  if (!c) return rc;
  if (na == 0) return VSG_OK;
  Stage st;
  const size_t oA = st.add((size_t)na * 32), oB = st.add((size_t)(nb > 0 ? nb : 1) * 32);
  const size_t in_bytes = st.total;
  const size_t o1 = st.add((size_t)na * 4), o2 = st.add((size_t)na * 4), o3 = st.add((size_t)na * 4);
  rc = vsg::ctx_reserve(c, st.total, in_bytes);
  if (rc != VSG_OK) return rc;
  uint8_t *h = c->h_pin;
  memcpy(h + oA, a, (size_t)na * 32);
  if (nb) memcpy(h + oB, b, (size_t)nb * 32);
  TRY_HIP(hipMemcpyAsync(c->d_buf, h, in_bytes, hipMemcpyHostToDevice, c->stream));
  const uint8_t *d = c->d_buf;
  int *d1 = (int *)(c->d_pin + o1), *d2 = (int *)(c->d_pin + o2), *d3 = (int *)(c->d_pin + o3);
  const dim3 grid((na + kBest2Rows - 1) / kBest2Rows, 1);
  hipLaunchKernelGGL(k_block_best2_mfma, grid, dim3(256), 0, c->stream, d + oA, d + oB, (size_t)0,
                     (const int *)nullptr, (const int *)nullptr, 0, na, nb, na, d1, d2, d3);
  TRY_HIP(hipGetLastError());
  TRY_HIP(hipStreamSynchronize(c->stream));
  memcpy(best, h + o1, (size_t)na * 4);
  memcpy(second, h + o2, (size_t)na * 4);
  memcpy(argbest, h + o3, (size_t)na * 4);
  return VSG_OK;
}

int vsg_search_for_triangulation(int device, const uint8_t *desc1, const float *angle1, const uint8_t *eligible1,
                                 int n1, const int32_t *node_id1, const int32_t *off1, const int32_t *idx1, int nodes1,
                                 const uint8_t *desc2, const float *angle2, const uint8_t *eligible2, int n2,
                                 const int32_t *node_id2, const int32_t *off2, const int32_t *idx2, int nodes2,
                                 const uint32_t *pair_ok, const int32_t *pair_off, int check_orientation,
                                 int32_t *matches12) {
  if (!matches12) return VSG_ERR_INVALID;
  return node_search(device, 2, -1, 0.0f, HostSide{n1, desc1, nullptr, angle1, nullptr, eligible1, {node_id1, off1, idx1, nodes1}},
                     HostSide{n2, desc2, nullptr, angle2, nullptr, eligible2, {node_id2, off2, idx2, nodes2}}, pair_ok, pair_off,
                     check_orientation, matches12);
}

// both KeyFrames resident (vsg_frame): only the FeatureVectors, the eligibility flags and the predicate bits go up
int vsg_frame_search_for_triangulation(vsg_frame *kf1, const uint8_t *eligible1, const int32_t *node_id1,
                                       const int32_t *off1, const int32_t *idx1, int nodes1, vsg_frame *kf2,
                                       const uint8_t *eligible2, const int32_t *node_id2, const int32_t *off2,
                                       const int32_t *idx2, int nodes2, const uint32_t *pair_ok, const int32_t *pair_off,
                                       int check_orientation, int32_t *matches12) {
  if (vsg::frame_check(kf1) != VSG_OK || vsg::frame_check(kf2) != VSG_OK || !matches12 || kf1->device != kf2->device ||
      !eligible1 || !eligible2)
    return VSG_ERR_INVALID;
  return node_search(kf1->device, 2, -1, 0.0f, frame_side(kf1, eligible1, node_id1, off1, idx1, nodes1),
                     frame_side(kf2, eligible2, node_id2, off2, idx2, nodes2), pair_ok, pair_off, check_orientation, matches12);
}

int vsg_search_by_bow_kf_f(int device, const uint8_t *kf_desc, const float *kf_angle, const uint8_t *kf_valid,
                           int n_kf, const int32_t *kf_node_id, const int32_t *kf_off, const int32_t *kf_idx,
                           int kf_nodes, const uint8_t *f_desc, const float *f_angle, int n_f,
                           const int32_t *f_node_id, const int32_t *f_off, const int32_t *f_idx, int f_nodes,
                           float nnratio, int check_orientation, int32_t *match_f) {
  return vsg_search_by_bow_kf_f_stereo(device, kf_desc, kf_angle, kf_valid, n_kf, kf_node_id, kf_off, kf_idx, kf_nodes,
                                       f_desc, f_angle, n_f, -1, f_node_id, f_off, f_idx, f_nodes, nnratio,
                                       check_orientation, match_f);
}

int vsg_search_by_bow_kf_f_stereo(int device, const uint8_t *kf_desc, const float *kf_angle, const uint8_t *kf_valid,
                                  int n_kf, const int32_t *kf_node_id, const int32_t *kf_off, const int32_t *kf_idx,
                                  int kf_nodes, const uint8_t *f_desc, const float *f_angle, int n_f, int f_nleft,
                                  const int32_t *f_node_id, const int32_t *f_off, const int32_t *f_idx, int f_nodes,
                                  float nnratio, int check_orientation, int32_t *match_f) {
  if (!match_f || f_nleft < -1 || f_nleft > n_f) return VSG_ERR_INVALID;
  return node_search(device, 0, f_nleft, nnratio,
                     HostSide{n_kf, kf_desc, nullptr, kf_angle, nullptr, kf_valid, {kf_node_id, kf_off, kf_idx, kf_nodes}},
                     HostSide{n_f, f_desc, nullptr, f_angle, nullptr, nullptr, {f_node_id, f_off, f_idx, f_nodes}}, nullptr, nullptr,
                     check_orientation, match_f);
}

int vsg_search_by_bow_kf_kf(int device, const uint8_t *desc1, const float *angle1, const uint8_t *valid1, int n1,
                            const int32_t *node_id1, const int32_t *off1, const int32_t *idx1, int nodes1,
                            const uint8_t *desc2, const float *angle2, const uint8_t *valid2, int n2,
                            const int32_t *node_id2, const int32_t *off2, const int32_t *idx2, int nodes2,
                            float nnratio, int check_orientation, int32_t *matches12) {
  if (!matches12) return VSG_ERR_INVALID;
  return node_search(device, 1, -1, nnratio, HostSide{n1, desc1, nullptr, angle1, nullptr, valid1, {node_id1, off1, idx1, nodes1}},
                     HostSide{n2, desc2, nullptr, angle2, nullptr, valid2, {node_id2, off2, idx2, nodes2}}, nullptr, nullptr,
                     check_orientation, matches12);
}

// the same two searches with both descriptor sets resident (vsg_frame): only FeatureVectors + flags go up
int vsg_frame_search_by_bow_kf_f(vsg_frame *kf, const uint8_t *kf_valid, const int32_t *kf_node_id,
                                 const int32_t *kf_off, const int32_t *kf_idx, int kf_nodes, vsg_frame *f,
                                 const int32_t *f_node_id, const int32_t *f_off, const int32_t *f_idx, int f_nodes,
                                 float nnratio, int check_orientation, int32_t *match_f) {
  // an empty frame's arrays may be NULL (std::vector::data() of an empty vector)
  if (vsg::frame_check(kf) != VSG_OK || vsg::frame_check(f) != VSG_OK || (!match_f && f->n > 0) || kf->device != f->device ||
      (!kf_valid && kf->n > 0))
    return VSG_ERR_INVALID;
  if (!kf_node_id && !f_node_id)  // both FeatureVectors resident (ComputeBoW ran on both frames): nothing goes up but the flags
    return search_by_bow_resident(0, kf, kf_valid, f, nullptr, nnratio, check_orientation, match_f);
  if (!kf_node_id || !f_node_id || !kf_off || !f_off || !kf_idx || !f_idx) return VSG_ERR_INVALID;  // only SOME of them
  return node_search(kf->device, 0, f->nleft, nnratio, frame_side(kf, kf_valid, kf_node_id, kf_off, kf_idx, kf_nodes),
                     frame_side(f, nullptr, f_node_id, f_off, f_idx, f_nodes), nullptr, nullptr, check_orientation, match_f);
}

int vsg_frame_search_by_bow_kf_kf(vsg_frame *kf1, const uint8_t *valid1, const int32_t *node_id1, const int32_t *off1,
                                  const int32_t *idx1, int nodes1, vsg_frame *kf2, const uint8_t *valid2,
                                  const int32_t *node_id2, const int32_t *off2, const int32_t *idx2, int nodes2,
                                  float nnratio, int check_orientation, int32_t *matches12) {
  if (vsg::frame_check(kf1) != VSG_OK || vsg::frame_check(kf2) != VSG_OK || (!matches12 && kf1->n > 0) ||
      kf1->device != kf2->device || (!valid1 && kf1->n > 0) || (!valid2 && kf2->n > 0))
    return VSG_ERR_INVALID;
  if (!node_id1 && !node_id2) return search_by_bow_resident(1, kf1, valid1, kf2, valid2, nnratio, check_orientation, matches12);
  if (!node_id1 || !node_id2 || !off1 || !off2 || !idx1 || !idx2) return VSG_ERR_INVALID;  // only SOME of them
  return node_search(kf1->device, 1, -1, nnratio, frame_side(kf1, valid1, node_id1, off1, idx1, nodes1),
                     frame_side(kf2, valid2, node_id2, off2, idx2, nodes2), nullptr, nullptr, check_orientation, matches12);
}

int vsg_search_by_projection_last(int device, const uint8_t *q_desc, const float *q_angle,
                                  const uint8_t *query_blocks, int n_q, const int32_t *cand_off,
                                  const int32_t *cand_idx, const uint8_t *t_desc, const float *t_angle,
                                  uint8_t *train_blocked, int n_t, int th_high, int check_orientation,
                                  int32_t *train_match) {
  if (!cand_off || !train_blocked || !train_match || n_q < 0 || n_t < 0) return VSG_ERR_INVALID;
  if (n_q == 0 || n_t == 0) return vsg::use_device(device) == VSG_OK ? 0 : VSG_ERR_NO_DEVICE;
  const uint32_t *ent = nullptr;
  int rc = candidate_entries(device, q_desc, n_q, cand_off, cand_idx, t_desc, nullptr, n_t, &ent);
  if (rc != VSG_OK) return rc;
  // ORBmatcher.cc:1686-1784 (left / mono block) + the rotation filter :1855-1875
  return walk::search_last(csr_view(ent, cand_off), n_q, -1, q_angle, query_blocks, [&](int i) { return t_angle[i]; },
                           th_high, check_orientation != 0, train_blocked, train_match);
}

int vsg_search_by_projection_local(int device, const uint8_t *q_desc, const uint8_t *query_blocks, int n_q,
                                   const int32_t *cand_off, const int32_t *cand_idx, const uint8_t *t_desc,
                                   const int32_t *t_octave, uint8_t *train_blocked, int n_t, float nnratio,
                                   int32_t *train_match) {
  if (!cand_off || !train_blocked || !train_match || !t_octave || n_q < 0 || n_t < 0) return VSG_ERR_INVALID;
  if (n_q == 0 || n_t == 0) return vsg::use_device(device) == VSG_OK ? 0 : VSG_ERR_NO_DEVICE;
  const uint32_t *ent = nullptr;
  int rc = candidate_entries(device, q_desc, n_q, cand_off, cand_idx, t_desc, t_octave, n_t, &ent);
  if (rc != VSG_OK) return rc;
  // ORBmatcher.cc:48-144 (left block): every query is "in view"
  std::vector<uint8_t> in_view((size_t)n_q, 1);
  return walk::search_local(csr_view(ent, cand_off), n_q, -1, in_view.data(), nullptr, nullptr, query_blocks, nnratio,
                            nullptr, nullptr, train_blocked, train_match);
}

int vsg_distinctive_descriptors(int device, const uint8_t *desc, const int32_t *off, int ngroups, int32_t *best) {
  if (!off || !best || ngroups < 0) return VSG_ERR_INVALID;
  int rc = VSG_OK;
  ThreadCtx *c = vsg::thread_ctx(device, &rc);
  if (!c) return rc;
  if (ngroups == 0) return VSG_OK;
  for (int g = 0; g < ngroups; g++)
    if (off[g + 1] - off[g] > kDistinctMaxN) return VSG_ERR_UNSUPPORTED;
  const int n = off[ngroups];
  Stage st;
  const size_t oD = st.add((size_t)n * 32), oOff = st.add((size_t)(ngroups + 1) * 4);
  const size_t in_bytes = st.total;
  const size_t oB = st.add((size_t)ngroups * 4);
  rc = vsg::ctx_reserve(c, st.total, in_bytes);
  if (rc != VSG_OK) return rc;
  uint8_t *h = c->h_pin;
  if (n) memcpy(h + oD, desc, (size_t)n * 32);
  memcpy(h + oOff, off, (size_t)(ngroups + 1) * 4);
  TRY_HIP(hipMemcpyAsync(c->d_buf, h, in_bytes, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_distinctive, dim3(ngroups), dim3(128), 0, c->stream, c->d_buf + oD, (const int *)(c->d_buf + oOff),
                     (int *)(c->d_pin + oB));
  TRY_HIP(hipGetLastError());
  TRY_HIP(hipStreamSynchronize(c->stream));
  memcpy(best, h + oB, (size_t)ngroups * 4);
  return VSG_OK;
}

int vsg_search_window(int device, const uint8_t *q_desc, const uint8_t *query_blocks, int n_q,
                      const int32_t *cand_off, const int32_t *cand_idx, const uint8_t *t_desc, uint8_t *train_blocked,
                      int n_t, int th_high, int32_t *q_best_idx, int32_t *q_best_dist, int32_t *train_match) {
  if (!cand_off || !q_best_idx || !q_best_dist || n_q < 0 || n_t < 0) return VSG_ERR_INVALID;
  for (int q = 0; q < n_q; q++) q_best_idx[q] = -1, q_best_dist[q] = 256;
  if (n_q == 0 || n_t == 0) return vsg::use_device(device) == VSG_OK ? 0 : VSG_ERR_NO_DEVICE;
  const uint32_t *ent = nullptr;
  int rc = candidate_entries(device, q_desc, n_q, cand_off, cand_idx, t_desc, nullptr, n_t, &ent);
  if (rc != VSG_OK) return rc;
  const walk::CandView cv = csr_view(ent, cand_off);
  int nmatches = 0;
  for (int q = 0; q < n_q; q++) {
    int bestDist, bestIdx;
    walk::scan_best(cv.begin(q), cv.size(q), [&](int idx) { return train_blocked && train_blocked[idx]; }, 256, bestDist,
                    bestIdx);
    q_best_idx[q] = bestIdx;
    q_best_dist[q] = bestDist;
    if (bestIdx >= 0 && bestDist <= th_high) {
      if (train_match) train_match[bestIdx] = q;
      if (train_blocked) train_blocked[bestIdx] = query_blocks ? query_blocks[q] : 0;
      nmatches++;
    }
  }
  return nmatches;
}

int vsg_search_for_initialization(int device, const uint8_t *desc1, const float *angle1, const int32_t *octave1,
                                  int n1, const int32_t *cand_off, const int32_t *cand_idx, const uint8_t *desc2,
                                  const float *angle2, int n2, float nnratio, int check_orientation,
                                  int32_t *matches12) {
  if (!cand_off || !matches12 || !octave1 || n1 < 0 || n2 < 0) return VSG_ERR_INVALID;
  for (int i = 0; i < n1; i++) matches12[i] = -1;
  if (n1 == 0 || n2 == 0) return vsg::use_device(device) == VSG_OK ? 0 : VSG_ERR_NO_DEVICE;
  const uint32_t *ent = nullptr;
  int rc = candidate_entries(device, desc1, n1, cand_off, cand_idx, desc2, nullptr, n2, &ent);
  if (rc != VSG_OK) return rc;
  // ORBmatcher.cc:643-756
  return walk::search_initialization(csr_view(ent, cand_off), n1, n2, octave1, [&](int i) { return angle1[i]; },
                                     [&](int i) { return angle2[i]; }, nnratio, check_orientation != 0, matches12);
}

}  // extern "C"
