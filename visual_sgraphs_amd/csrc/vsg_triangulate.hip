// vsg_triangulate.hip -- LocalMapping::CreateNewMapPoints on resident keyframes (LocalMapping.cc:382-710), one neighbour
// per call: vsg_frame_set_stereo_points, vsg_frame_triangulate_matches, vsg_frame_create_new_map_points.
//
// k_new_points is ONE persistent workgroup that runs behind the epipolar walk (k_triangulation_walk<EpipolarPred>,
// vsg_match.hip) on the calling thread's stream, or on its own for a match list the caller holds:
//   1. (fused call with check_orientation) the 30-bin rotation histogram of the matches in LDS -- integer counts, so the
//      order of the LDS atomics does not matter -- and ComputeThreeMaxima by one lane (vsg_walks.h, the host passes' source);
//   2. in chunks of kTriThreads features of kf1, one lane per feature: a match outside the three bins is removed; a lane
//      with a match runs the pair's arithmetic (vsg_triangulate.h: float gates, the 4 x 4 Hestenes Jacobi in double);
//   3. a workgroup-wide exclusive scan of the accepted flags (DPP scan per wave, the waves' totals through LDS, the
//      chunks' running base in LDS) ranks the accepted pairs in ascending idx1;
//   4. the pair of rank k takes free_slots[k] and writes the slot (position, descriptor row, normal and depth range through
//      vsg_observations.h, observed) and the per-feature outputs, all with plain vector stores.
// Every loop is bounded by an argument (n1) or a compile-time constant; nothing spins on data.
#include <string.h>

#include <vector>

#include "vsg_frame_int.h"
#include "vsg_triangulate.h"

using namespace vsg;

namespace {

enum { kTriThreads = 512, kTriWaves = kTriThreads / 64 };

struct TriFrameDev {
  const KeyPointPOD *kps;
  const uint8_t *desc;
  const float *uright;   // nullptr: every mvuRight is -1
  const float4 *stereo;  // {x3Dc, cos parallax}; nullptr: no stereo keypoint
};

struct TriTables {
  float scale_factors[16], level_sigma2[16];
};

struct NewPointsArgs {
  TriFrameDev A, B;
  int n1, nlevels;
  int filter;               // run the rotation-consistency filter on matches_in first
  const int *matches_in;    // [n1], -1 = none
  int *matches_out;         // the list after the filter (fused call; may alias matches_in: lane i reads, then writes, entry i)
  vsg_triangulation_params P;
  TriTables T1, T2;
  StoreFields S;            // pos == nullptr: geometry only
  const int *free_slots;
  int n_free;
  uint8_t *reason, *source;
  float *x3d;
  int *new_slot;
  int *counts;              // {n_created, matches after the filter}
};

__device__ __forceinline__ TriFeature tri_feature(const TriFrameDev &F, const TriTables &T, int i, int *octave) {
  const KeyPointPOD kp = F.kps[i];
  const int lv = kp.octave & 15;  // the host checked [0, nlevels) on its mirror; the tables have 16 entries
  TriFeature f;
  f.x = kp.x, f.y = kp.y, f.uright = F.uright ? F.uright[i] : -1.0f;
  f.scale_factor = T.scale_factors[lv], f.level_sigma2 = T.level_sigma2[lv];
  f.cos_stereo = 0.0f, f.xyz_c[0] = f.xyz_c[1] = f.xyz_c[2] = 0.0f;
  if (f.uright >= 0 && F.stereo) {  // (the host refused a frame with stereo keypoints and nothing attached)
    const float4 s = F.stereo[i];
    f.xyz_c[0] = s.x, f.xyz_c[1] = s.y, f.xyz_c[2] = s.z, f.cos_stereo = s.w;
  }
  *octave = lv;
  return f;
}

__global__ __launch_bounds__(kTriThreads) void k_new_points(NewPointsArgs a) {
  __shared__ int s_hist[walk::HISTO_LENGTH];
  __shared__ int s_ind[3];
  __shared__ int s_wsum[kTriWaves];
  __shared__ int s_base, s_nmatch;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid < walk::HISTO_LENGTH) s_hist[tid] = 0;
  if (tid == 0) s_base = 0, s_nmatch = 0, s_ind[0] = s_ind[1] = s_ind[2] = -1;
  __syncthreads();
  if (a.filter) {  // ORBmatcher.cc:1083-1118
    for (int i = tid; i < a.n1; i += kTriThreads) {
      const int m = a.matches_in[i];
      if (m < 0) continue;
      const int bin = walk::rot_bin(a.A.kps[i].angle, a.B.kps[m].angle);
      if ((unsigned)bin < (unsigned)walk::HISTO_LENGTH) atomicAdd(&s_hist[bin], 1);
    }
    __syncthreads();
    if (tid == 0) {
      int ind1 = -1, ind2 = -1, ind3 = -1;
      walk::three_maxima_of([&](int i) { return s_hist[i]; }, (int)walk::HISTO_LENGTH, ind1, ind2, ind3);
      s_ind[0] = ind1, s_ind[1] = ind2, s_ind[2] = ind3;
    }
    __syncthreads();
  }
  const int ind1 = s_ind[0], ind2 = s_ind[1], ind3 = s_ind[2];
  const bool with_store = a.S.pos != nullptr;
  for (int base = 0; base < a.n1; base += kTriThreads) {  // block-uniform: every lane reaches the barriers below
    const int i = base + tid;
    int m = i < a.n1 ? a.matches_in[i] : -1;
    if (a.filter && m >= 0) {
      const int bin = walk::rot_bin(a.A.kps[i].angle, a.B.kps[m].angle);
      if (bin != ind1 && bin != ind2 && bin != ind3) m = -1;
    }
    TriOut o = {kTriNoMatch, kTriFromTriangulate, {0.0f, 0.0f, 0.0f}};
    int octave1 = 0;
    if (m >= 0) {
      int octave2;
      const TriFeature f1 = tri_feature(a.A, a.T1, i, &octave1), f2 = tri_feature(a.B, a.T2, m, &octave2);
      o = triangulate_pair(a.P, f1, f2);
    }
    const int accepted = o.reason == kTriAccepted ? 1 : 0;
    const int incl = wave_incl_scan(accepted);
    const unsigned long long has = __ballot(m >= 0);
    if (lane == 63) s_wsum[wave] = incl;
    if (lane == 0 && has) atomicAdd(&s_nmatch, __popcll(has));
    __syncthreads();
    int rank = s_base + incl - accepted, total = 0;
    for (int w = 0; w < kTriWaves; w++) {
      const int ws = s_wsum[w];
      if (w < wave) rank += ws;
      total += ws;
    }
    __syncthreads();  // everyone has read s_base and s_wsum
    if (tid == 0) s_base += total;
    int slot = -1;
    if (accepted && with_store) {
      if (rank < a.n_free) {
        slot = a.free_slots[rank];  // inside [0, capacity) and listed once: the host checked
        const size_t s = (size_t)slot;
        a.S.pos[3 * s] = o.x3D[0], a.S.pos[3 * s + 1] = o.x3D[1], a.S.pos[3 * s + 2] = o.x3D[2];
        // ComputeDistinctiveDescriptors of two observations: both medians are 0, the first in the map's order wins
        const uint4 *src = (const uint4 *)(a.P.kf2_first ? a.B.desc + 32 * (size_t)m : a.A.desc + 32 * (size_t)i);
        const uint4 d0 = src[0], d1 = src[1];
        ((uint4 *)(a.S.desc + 32 * s))[0] = d0, ((uint4 *)(a.S.desc + 32 * s))[1] = d1;
        float nrm[3], mn, mx;
        new_point_normal_and_depth(a.P, o.x3D, octave1, a.T1.scale_factors, a.nlevels, nrm, &mn, &mx);
        a.S.normal[3 * s] = nrm[0], a.S.normal[3 * s + 1] = nrm[1], a.S.normal[3 * s + 2] = nrm[2];
        a.S.min_dist[s] = mn, a.S.max_dist[s] = mx;
        a.S.observed[s] = 1;
      } else {
        o.reason = kTriNoFreeSlot;
      }
    }
    if (i < a.n1) {
      if (a.matches_out) a.matches_out[i] = m;
      a.reason[i] = (uint8_t)o.reason, a.source[i] = (uint8_t)o.source;
      a.x3d[3 * (size_t)i] = o.x3D[0], a.x3d[3 * (size_t)i + 1] = o.x3D[1], a.x3d[3 * (size_t)i + 2] = o.x3D[2];
      a.new_slot[i] = slot;
    }
  }
  __syncthreads();
  if (tid == 0) {
    a.counts[0] = with_store ? min(s_base, a.n_free) : 0;
    a.counts[1] = s_nmatch;
  }
}

TriFrameDev tri_frame(const vsg_frame *f) {
  return TriFrameDev{f->d_kps, f->d_desc, f->has_uright ? f->d_uright : (const float *)nullptr,
                     f->stereo_attached ? f->d_stereo : (const float4 *)nullptr};
}

struct TriCallArgs {
  vsg_frame *kf1, *kf2;
  const vsg_triangulation_params *params;
  const float *sf1, *sigma1, *sf2, *sigma2;
  int nlevels;
  vsg_mappoints *mp;
  const int32_t *free_slots;
  int n_free;
  uint8_t *reason, *source;
  float *x3d;
  int32_t *new_slot, *n_created;
};

// What both entry points refuse before anything is enqueued (the match list and the search have checks of their own)
int tri_check(const TriCallArgs &t, StoreFields *S) {
  if (frame_check(t.kf1) != VSG_OK || frame_check(t.kf2) != VSG_OK || t.kf1->device != t.kf2->device || !t.params || !t.sf1 ||
      !t.sigma1 || !t.sf2 || !t.sigma2 || t.nlevels < 1 || t.nlevels > 16 || !t.n_created ||
      (t.kf1->n > 0 && (!t.reason || !t.source || !t.x3d || !t.new_slot)))
    return VSG_ERR_INVALID;
  if (t.kf1->nleft != -1 || t.kf2->nleft != -1) return VSG_ERR_UNSUPPORTED;  // mpCamera2 (:482-554)
  for (const vsg_frame *f : {t.kf1, t.kf2}) {
    if (!tri_octaves_ok((int)f->h_kps.size(), [&](int i) { return f->h_kps[(size_t)i].octave; }, t.nlevels)) return VSG_ERR_INVALID;
    if (f->any_stereo && !f->stereo_attached) return VSG_ERR_INVALID;  // vsg_frame_set_stereo_points first
  }
  memset(S, 0, sizeof *S);
  if (t.mp) {
    if (!store_fields(t.mp, S) || S->device != t.kf1->device) return VSG_ERR_INVALID;
    std::vector<uint8_t> seen((size_t)S->capacity, 0);
    if (!tri_free_slots_ok(S->capacity, t.free_slots, t.n_free, seen.data())) return VSG_ERR_INVALID;
  }
  return VSG_OK;
}

// the outputs of a call that needs no launch: no feature has a match
void tri_no_matches(const TriCallArgs &t) {
  const int n1 = t.kf1->n;
  for (int i = 0; i < n1; i++) {
    t.reason[i] = kTriNoMatch, t.source[i] = kTriFromTriangulate, t.new_slot[i] = -1;
    t.x3d[3 * i] = t.x3d[3 * i + 1] = t.x3d[3 * i + 2] = 0.0f;
  }
  *t.n_created = 0;
}

// the blocks of k_new_points behind `base` in the pinned arena
struct TriLayout {
  size_t oFree, oReason, oSource, oX, oSlot, oCounts, total;
  TriLayout(size_t base, size_t n1, size_t n_free) {
    Stage st;
    st.total = base;
    oFree = st.add(n_free * 4), oReason = st.add(n1), oSource = st.add(n1), oX = st.add(n1 * 12), oSlot = st.add(n1 * 4);
    oCounts = st.add(8);
    total = st.total;
  }
};

// fills the free-slot list, enqueues k_new_points on c's stream.  matches = offset of the match list in the arena.
void tri_enqueue(ThreadCtx *c, const TriCallArgs &t, const StoreFields &S, const TriLayout &L, size_t oMatches, bool filter,
                 bool write_matches) {
  uint8_t *h = c->h_pin, *d = c->d_pin;
  const int n_free = t.mp ? t.n_free : 0;
  if (n_free) memcpy(h + L.oFree, t.free_slots, (size_t)n_free * 4);
  NewPointsArgs a;
  memset(&a, 0, sizeof a);
  a.A = tri_frame(t.kf1), a.B = tri_frame(t.kf2);
  a.n1 = t.kf1->n, a.nlevels = t.nlevels, a.filter = filter ? 1 : 0;
  a.matches_in = (const int *)(d + oMatches), a.matches_out = write_matches ? (int *)(d + oMatches) : nullptr;
  a.P = *t.params;
  for (int l = 0; l < 16; l++) {  // entries above nlevels are never indexed (the octaves were checked)
    const int k = l < t.nlevels ? l : t.nlevels - 1;
    a.T1.scale_factors[l] = t.sf1[k], a.T1.level_sigma2[l] = t.sigma1[k];
    a.T2.scale_factors[l] = t.sf2[k], a.T2.level_sigma2[l] = t.sigma2[k];
  }
  a.S = S;
  a.free_slots = (const int *)(d + L.oFree), a.n_free = n_free;
  a.reason = d + L.oReason, a.source = d + L.oSource, a.x3d = (float *)(d + L.oX), a.new_slot = (int *)(d + L.oSlot);
  a.counts = (int *)(d + L.oCounts);
  hipLaunchKernelGGL(k_new_points, dim3(1), dim3(kTriThreads), 0, c->stream, a);
}

void tri_copy_out(ThreadCtx *c, const TriCallArgs &t, const TriLayout &L, int *n_after_filter) {
  const uint8_t *h = c->h_pin;
  const size_t n1 = (size_t)t.kf1->n;
  memcpy(t.reason, h + L.oReason, n1), memcpy(t.source, h + L.oSource, n1);
  memcpy(t.x3d, h + L.oX, n1 * 12), memcpy(t.new_slot, h + L.oSlot, n1 * 4);
  const int *counts = (const int *)(h + L.oCounts);
  *t.n_created = counts[0];
  if (n_after_filter) *n_after_filter = counts[1];
}

}  // namespace

extern "C" {

int vsg_frame_set_stereo_points(vsg_frame *f, const float *xyz_c, const float *cos_parallax) {
  if (frame_check(f) != VSG_OK || !xyz_c || !cos_parallax) return VSG_ERR_INVALID;
  int rc = VSG_OK;
  ThreadCtx *c = thread_ctx(f->device, &rc);
  if (!c) return rc;
  if (!f->d_stereo) TRY_HIP(hipMalloc((void **)&f->d_stereo, (size_t)f->capacity * sizeof(float4)));  // freed with the frame
  const size_t n = (size_t)f->n;
  if (n) {
    rc = ctx_reserve(c, n * sizeof(float4), 0);
    if (rc != VSG_OK) return rc;
    float4 *h = (float4 *)c->h_pin;
    for (size_t i = 0; i < n; i++) h[i] = make_float4(xyz_c[3 * i], xyz_c[3 * i + 1], xyz_c[3 * i + 2], cos_parallax[i]);
    TRY_HIP(hipMemcpyAsync(f->d_stereo, h, n * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    TRY_HIP(hipStreamSynchronize(c->stream));
  }
  f->stereo_attached = true;
  return VSG_OK;
}

int vsg_frame_triangulate_matches(vsg_frame *kf1, vsg_frame *kf2, const int32_t *matches12,
                                  const vsg_triangulation_params *params, const float *scale_factors1,
                                  const float *level_sigma2_1, const float *scale_factors2, const float *level_sigma2_2,
                                  int nlevels, vsg_mappoints *mp, const int32_t *free_slots, int n_free, uint8_t *reason,
                                  uint8_t *source, float *x3d, int32_t *new_slot, int32_t *n_created) {
  const TriCallArgs t{kf1,     kf2,        params, scale_factors1, level_sigma2_1, scale_factors2, level_sigma2_2, nlevels, mp,
                      free_slots, n_free, reason, source,         x3d,            new_slot,       n_created};
  StoreFields S;
  int rc = tri_check(t, &S);
  if (rc != VSG_OK) return rc;
  const int n1 = kf1->n, n2 = kf2->n;
  if (n1 > 0 && (!matches12 || !tri_matches_ok(n1, n2, matches12))) return VSG_ERR_INVALID;
  bool any = false;
  for (int i = 0; i < n1; i++) any |= matches12[i] >= 0;
  // ---- nothing is refused from here on
  if (!any) {
    tri_no_matches(t);
    return VSG_OK;
  }
  ThreadCtx *c = thread_ctx(kf1->device, &rc);
  if (!c) return rc;
  Stage st;
  const size_t oM = st.add((size_t)n1 * 4);
  const TriLayout L(st.total, (size_t)n1, (size_t)(mp ? n_free : 0));
  rc = ctx_reserve(c, L.total, 0);
  if (rc != VSG_OK) return rc;
  memcpy(c->h_pin + oM, matches12, (size_t)n1 * 4);
  tri_enqueue(c, t, S, L, oM, false, false);
  const hipError_t launched = hipGetLastError(), waited = hipStreamSynchronize(c->stream);  // an error still waits
  if (launched != hipSuccess || waited != hipSuccess) return VSG_ERR_HIP;
  tri_copy_out(c, t, L, nullptr);
  return VSG_OK;
}

int vsg_frame_create_new_map_points(vsg_frame *kf1, const uint8_t *no_mp1, const int32_t *node_id1, const int32_t *off1,
                                    const int32_t *idx1, int nodes1, vsg_frame *kf2, const uint8_t *no_mp2,
                                    const int32_t *node_id2, const int32_t *off2, const int32_t *idx2, int nodes2,
                                    const float F12[9], const float ep[2], int only_stereo, int coarse,
                                    int check_orientation, const vsg_triangulation_params *params,
                                    const float *scale_factors1, const float *level_sigma2_1, const float *scale_factors2,
                                    const float *level_sigma2_2, int nlevels, vsg_mappoints *mp, const int32_t *free_slots,
                                    int n_free, int32_t *matches12, uint8_t *reason, uint8_t *source, float *x3d,
                                    int32_t *new_slot, int32_t *n_created) {
  const TriCallArgs t{kf1,     kf2,        params, scale_factors1, level_sigma2_1, scale_factors2, level_sigma2_2, nlevels, mp,
                      free_slots, n_free, reason, source,         x3d,            new_slot,       n_created};
  StoreFields S;
  int rc = tri_check(t, &S);
  if (rc != VSG_OK) return rc;
  const EpiSearchArgs e{kf1, no_mp1, node_id1, off1, idx1, nodes1, kf2, no_mp2, node_id2, off2, idx2, nodes2, F12, ep,
                        scale_factors2, level_sigma2_2, nlevels, only_stereo, coarse};
  rc = epipolar_search_check(e, matches12);
  if (rc != VSG_OK) return rc;
  if (check_orientation)  // rot_bin's bins lie in [0, 30) for angles of [0, 360] (the extractor's range); nothing else is binned
    for (const vsg_frame *f : {kf1, kf2})
      for (const vsg_keypoint &k : f->h_kps)
        if (!(k.angle >= 0.0f && k.angle <= 360.0f)) return VSG_ERR_INVALID;
  // ---- nothing is refused from here on
  const int n1 = kf1->n;
  for (int i = 0; i < n1; i++) matches12[i] = -1;
  const TriLayout L0(0, (size_t)n1, (size_t)(mp ? n_free : 0));
  EpiSearch s;
  rc = epipolar_search_enqueue(&s, e, L0.total);
  if (rc != VSG_OK) return rc;
  if (!s.launched) {  // no shared node: no match, no point
    tri_no_matches(t);
    return 0;
  }
  hipError_t launched = hipGetLastError();
  const TriLayout L(s.oExtra, (size_t)n1, (size_t)(mp ? n_free : 0));
  if (launched == hipSuccess) {
    tri_enqueue(s.c, t, S, L, s.oM, check_orientation != 0, true);
    launched = hipGetLastError();
  }
  const hipError_t waited = hipStreamSynchronize(s.c->stream);  // an error still waits
  if (launched != hipSuccess || waited != hipSuccess) return VSG_ERR_HIP;
  memcpy(matches12, s.c->h_pin + s.oM, (size_t)n1 * 4);
  int nmatches = 0;
  tri_copy_out(s.c, t, L, &nmatches);
  return nmatches;
}

}  // extern "C"
