// vsg_sgraph_ba.hip -- Optimizer::LocalBundleAdjustment with its planes and rooms (Optimizer.cc:1454-2454) on resident
// keyframes and resident map points: vsg_mappoints_local_bundle_adjustment_sgraph (include/vsg_orb.h).  The arithmetic is
// csrc/vsg_local_ba.h (the visual part) and csrc/vsg_sgraph_ba.h (planes and rooms), shared with the host build bit for
// bit; this file adds the semantic kernels and the entry point.  The enqueue policy is csrc/vsg_lm_driver.h.
//
// KERNEL BOUNDARIES ON THE CALLING THREAD'S STREAM ARE THE ONLY SYNCHRONISATION BETWEEN WORKGROUPS, as in vsg_local_ba.hip:
// no grid-wide barrier, no cooperative launch, no flag between workgroups, nothing spins.  The Levenberg controller
// (lba::State) lives in device memory, is written by the one-lane steps k_begin and k_decide alone, and is read first by
// every phase kernel.  The visual phases are the kernels of vsg_ba_kernels.inc, launched with lba::Prob as the visual call
// fills it except for the reduced system (n rows with the planes and rooms behind the keyframes); k_begin and k_decide get
// the same record with the semantic partials counted in (Prob::Ge, Prob::Gp).
//
// Per iteration: k_linearise, k_sg_linearise (ONE WAVE PER SEMANTIC EDGE: lanes 0-18 / 0-24 / 0-36 each take one
// evaluation of the numeric Jacobian -- (column, sign), the last one the error itself -- then the 64 lanes split the
// entries of the edge's blocks; errors and Jacobians go through LDS), k_gather, k_sg_gather (the semantic chi2 tree, b and
// the diagonal per semantic row, the keyframes' semantic blocks into Hpp / bp), k_begin.  Per trial: k_trial_edges, k_schur,
// k_sg_assemble (the blocks behind the keyframes' Schur complement, one lane per entry, and bs), k_solve (ONE workgroup),
// k_backsub, k_sg_oplus (planes, rooms, computeScale's terms), k_error, k_sg_error, k_decide.  Then k_sg_final.
// k_solve and k_backsub are the local call's, in vsg_ba_kernels.inc with the other visual phases.  All stores are plain
// vector stores; the two visual edge counts are integer atomics.
#include <cstring>

#include "vsg_block_tree.h"
#include "vsg_frame_int.h"
#include "vsg_lm_driver.h"
#include "vsg_sgraph_ba.h"

using namespace vsg;

namespace {

#include "vsg_ba_kernels.inc"

static_assert(sgba::kMaxRows == kSolveRows, "k_solve's LDS arrays hold every row this call admits");

// erase and chi2 stand before wb, unlike in the other two calls' structs: k_sg_final allocates 62 SGPRs with this order and 60
// with wb first, the same occupancy either way
struct FinalArgs {
  uint8_t *erase;
  double *chi2;
  WriteBack wb;
  uint8_t *erase_plane;
  double *chi2_kf, *chi2_pp, *plane_out, *room_out;
};

// one wave per semantic edge, kEdgesPerGroup edges per workgroup
__global__ __launch_bounds__(lba::kThreads) void k_sg_linearise(lba::Prob p, sgba::Sem s, int it) {
  __shared__ double err[sgba::kEdgesPerGroup][sgba::kMaxSlots][3], J[sgba::kEdgesPerGroup][3 * sgba::kMaxCols], rho[sgba::kEdgesPerGroup];
  if (!lba::run_iteration(*p.S, it)) return;
  const int lane = threadIdx.x & (pose::kWave - 1), wave = threadIdx.x / pose::kWave, e = blockIdx.x * sgba::kEdgesPerGroup + wave;
  const bool live = e < s.Es;
  sgba::EdgeInfo I = {};
  if (live) {
    I = sgba::edge_info(s, e);
    if (sgba::slot_live(I, lane)) {
      double r[3];
      sgba::slot_error(p, s, e, I, lane, p.S->cur, r);
      err[wave][lane][0] = r[0], err[wave][lane][1] = r[1], err[wave][lane][2] = r[2];
    }
  }
  __syncthreads();
  if (live) {
    if (lane < 3 * sgba::kMaxCols) {
      const int r = lane / sgba::kMaxCols, c = lane % sgba::kMaxCols;
      J[wave][lane] = c < I.cols && sgba::slot_live(I, 2 * c) ? sgba::jacobian_entry(err[wave][2 * c][r], err[wave][2 * c + 1][r]) : 0.0;
    }
    if (lane == 0) {
      const double c2 = sgba::edge_chi2(err[wave][2 * I.cols], I.dim, I.w);
      double rho0, rho1;
      pose::huber(c2, I.delta, &rho0, &rho1);
      s.chi2[e] = c2, s.cost[e] = rho0, rho[wave] = rho1;
    }
  }
  __syncthreads();
  if (live) {
    const double rho1 = rho[wave];
    for (int x = lane; x < sgba::kBlock; x += pose::kWave)
      if (sgba::block_entry_live(I, x)) s.blocks[(size_t)e * sgba::kBlock + x] = sgba::block_entry(J[wave], err[wave][2 * I.cols], I, rho1, x);
  }
}

// workgroups [0, Gse): the semantic edges' robust chi2 through the tree; [Gse, Gse + Gsr): one lane per semantic row;
// then one lane per optimised keyframe
__global__ __launch_bounds__(lba::kThreads) void k_sg_gather(lba::Prob p, sgba::Sem s, int it) {
  __shared__ double lds[pose::kWaves];
  if (!lba::run_iteration(*p.S, it)) return;
  const int g = blockIdx.x, tid = threadIdx.x;
  if (g < s.Gse) {
    const int e = g * lba::kThreads + tid;
    double v = e < s.Es ? s.cost[e] : 0.0;
    block_tree<1, false>(&v, lds);
    if (tid == 0) p.chiPart[s.Ge0 + g] = v;
    return;
  }
  if (g < s.Gse + s.Gsr) {
    const int r = (g - s.Gse) * lba::kThreads + tid;
    double m = r < s.nsr ? sgba::gather_row(s, r, 6 * p.Ko) : 0.0;
    block_tree<1, true>(&m, lds);
    if (tid == 0) p.maxPart[s.Gp0 + (g - s.Gse)] = m;
    return;
  }
  const int i = (g - s.Gse - s.Gsr) * lba::kThreads + tid;
  if (i < p.Ko) sgba::gather_kf(p, s, i);
}

// workgroups [0, Gb): kBlocksPerGroup blocks each, one lane per entry; [Gb, Gb + Gsr): bs of the semantic rows
__global__ __launch_bounds__(lba::kThreads) void k_sg_assemble(lba::Prob p, sgba::Sem s, int it, int q, int Gb) {
  if (!lba::run_trial(*p.S, it, q)) return;
  const int g = blockIdx.x, tid = threadIdx.x;
  if (g < Gb) {
    const int blk = g * sgba::kBlocksPerGroup + tid / 36;
    if (tid < sgba::kBlocksPerGroup * 36 && blk < s.nbs) sgba::assemble_entry(p, s, blk, tid % 36, p.S->lambda);
    return;
  }
  const int r = (g - Gb) * lba::kThreads + tid;
  if (r < s.nsr) p.bs[6 * p.Ko + r] = s.bsem[r];
}

// one lane per semantic row: computeScale's term through the tree; the lane of a vertex's first row makes its oplus
__global__ __launch_bounds__(lba::kThreads) void k_sg_oplus(lba::Prob p, sgba::Sem s, int it, int q) {
  __shared__ double lds[pose::kWaves];
  if (!lba::run_trial(*p.S, it, q)) return;
  const int g = blockIdx.x, r = g * lba::kThreads + threadIdx.x;
  double v = 0.0;
  if (r < s.nsr) {
    const int sv = s.row_sv[r];
    if (s.sv_row[sv] == 6 * p.Ko + r) sgba::oplus_vertex(p, s, sv, p.S->cur);
    v = sgba::scale_row(p, s, r, p.S->lambda);
  }
  block_tree<1, false>(&v, lds);
  if (threadIdx.x == 0) p.scalePart[s.Gp0 + g] = v;
}

__global__ __launch_bounds__(lba::kThreads) void k_sg_error(lba::Prob p, sgba::Sem s, int it, int q) {
  __shared__ double lds[pose::kWaves];
  if (!lba::run_trial(*p.S, it, q)) return;
  const int e = blockIdx.x * lba::kThreads + threadIdx.x;
  double v = 0.0;
  if (e < s.Es) {
    double err[3], rho1;
    v = sgba::edge_cost(p, s, e, p.S->cur ^ 1, err, &rho1);
  }
  block_tree<1, false>(&v, lds);
  if (threadIdx.x == 0) p.chiPart[s.Ge0 + blockIdx.x] = v;
}

// the classification (:2296-2369) and the recovery (:2398-2441)
__global__ __launch_bounds__(lba::kThreads) void k_sg_final(lba::Prob p, sgba::Sem s, FinalArgs A) {
  const int i = blockIdx.x * lba::kThreads + threadIdx.x, cur = p.S->cur;
  if (i < p.E) lba::classify_edge(p, i, cur, A.erase, A.chi2);
  write_back(p, A.wb, i, cur, true);
  if (i < s.n_obs) sgba::classify_obs(p, s, i, cur, A.erase_plane, A.chi2_kf, A.chi2_pp);
  if (i < s.Pl && s.pl_act[i] >= 0)
    for (int k = 0; k < 4; k++) A.plane_out[4 * (size_t)i + k] = pose::canon(sgba::planes_of(s, cur)[4 * (size_t)i + k]);
  if (i < s.R)
    for (int k = 0; k < 3; k++) A.room_out[3 * (size_t)i + k] = pose::canon(sgba::rooms_of(s, cur)[i].t[k]);
}

// the semantic lists and start values in one block (copied to the device once), the scratch behind them
struct SemLayout {
  Stage in, dev;
  size_t oKind, oV0, oObs, oFix0, oPl, oW, oLocal, oG, oOkf, oOpl, oOpk, oOpp, oAct, oSvRow, oSvItem, oRowSv, oVoff, oVedge, oVcol,
      oKsOff, oKsEdge, oSbS, oSbT, oSbOff, oSbEdge, oSbCa, oSbCb, oPl0, oPl1, oRm0, oRm1;
  size_t dBlocks, dChi2, dCost, dBsem, dM, dBs, dXp, dChiPart, dMaxPart, dScalePart;
  template <class T>
  size_t vec(const std::vector<T> &v) { return in.add(v.size() * sizeof(T)); }
  SemLayout(const sgba::SemTopology &S, const sgba::Sem &s) {
    oKind = vec(S.e_kind), oV0 = vec(S.e_v0), oObs = vec(S.e_obs), oFix0 = vec(S.e_fix0), oPl = vec(S.e_pl), oW = vec(S.e_w);
    oLocal = in.add((size_t)S.n_obs * 32), oG = in.add((size_t)S.n_obs * 128);
    oOkf = vec(S.o_kf), oOpl = vec(S.o_pl), oOpk = vec(S.o_pk), oOpp = vec(S.o_pp), oAct = vec(S.pl_act), oSvRow = vec(S.sv_row);
    oSvItem = vec(S.sv_item), oRowSv = vec(S.row_sv), oVoff = vec(S.v_off), oVedge = vec(S.v_edge), oVcol = vec(S.v_col);
    oKsOff = vec(S.ks_off), oKsEdge = vec(S.ks_edge), oSbS = vec(S.sb_s), oSbT = vec(S.sb_t), oSbOff = vec(S.sb_off);
    oSbEdge = vec(S.sb_edge), oSbCa = vec(S.sb_ca), oSbCb = vec(S.sb_cb);
    oPl0 = in.add((size_t)S.Pl * 32), oPl1 = in.add((size_t)S.Pl * 32), oRm0 = in.add((size_t)S.R * sizeof(pose::Est));
    oRm1 = in.add((size_t)S.R * sizeof(pose::Est));
    dev = in;
    const size_t n = (size_t)S.n, Es = (size_t)S.Es;
    dBlocks = dev.add(Es * 8 * sgba::kBlock), dChi2 = dev.add(Es * 8), dCost = dev.add(Es * 8), dBsem = dev.add((size_t)S.nsr * 8);
    dM = dev.add(n * n * 8), dBs = dev.add(n * 8), dXp = dev.add(n * 8), dChiPart = dev.add((size_t)(s.Ge0 + s.Gse) * 8);
    dMaxPart = dev.add((size_t)(s.Gp0 + s.Gsr) * 8), dScalePart = dev.add((size_t)(s.Gp0 + s.Gsr) * 8);
  }
};

}  // namespace

extern "C" {

int vsg_mappoints_local_bundle_adjustment_sgraph(
    vsg_mappoints *mp, int n_points, const int32_t *slots, const int32_t *obs_off, const int32_t *obs_kf, const int32_t *obs_idx,
    int n_kf, vsg_frame *const *kfs, const vsg_pose_se3 *kf_Tcw, const uint8_t *kf_fixed, const vsg_ba_camera *kf_cam,
    const float *inv_level_sigma2, int nlevels, int iterations, const volatile uint8_t *stop_flag, vsg_pose_se3d *kf_Tcw_out,
    float *world_pos_out, uint8_t *erase, double *chi2, int n_planes, const double *plane_eq, const int32_t *pl_obs_off,
    const int32_t *pl_obs_kf, const double *pl_obs_local, const double *pl_obs_G, const double *w_plane_kf,
    const double *w_plane_point, int n_rooms, const double *room_center, const int32_t *room_n_walls, const int32_t *room_wall,
    double *plane_eq_out, double *room_center_out, uint8_t *erase_plane, double *chi2_plane_kf, double *chi2_plane_point,
    vsg_sgraph_local_ba_result *res) {
  StoreFields F;
  KfLists KL;
  int rc = ba_prologue(mp, n_kf, kfs, kf_Tcw, kf_fixed, kf_cam, inv_level_sigma2, kf_Tcw_out && erase && res, &F, &KL);
  if (rc != VSG_OK) return rc;
  if ((n_planes > 0 && !plane_eq_out) || (n_rooms > 0 && !room_center_out)) return VSG_ERR_INVALID;
  if (n_planes > 0 && pl_obs_off && pl_obs_off[0] == 0 && pl_obs_off[n_planes] > 0 && !erase_plane) return VSG_ERR_INVALID;
  const sgba::SemIn in = {n_planes, plane_eq, pl_obs_off, pl_obs_kf, pl_obs_local, pl_obs_G, w_plane_kf, w_plane_point,
                          n_rooms,  room_center, room_n_walls, room_wall};
  lba::Topology T;
  sgba::SemTopology ST;
  int ran = 0;
  rc = sgba::check_and_build(n_points, slots, obs_off, obs_kf, obs_idx, n_kf, KL.kf_n.data(), KL.nleft.data(), KL.octave(), kf_fixed,
                             F.capacity, nlevels, iterations, stop_flag, in, &T, &ST, &ran);
  if (rc != VSG_OK) return rc;
  if (!ran) {
    if (n_points == 0) T.n_fixed = T.n_opt = 0;
    sgba::fill_result(res, T, nullptr, nullptr);
    return VSG_OK;
  }
  // everything the kernels index has been bounded; nothing has been enqueued
  ThreadCtx *c = thread_ctx(F.device, &rc);
  if (!c) return rc;
  const size_t E = (size_t)T.E, P = (size_t)T.P, K = (size_t)T.K, Ko = (size_t)T.Ko, NO = (size_t)ST.n_obs, Pl = (size_t)ST.Pl,
               R = (size_t)ST.R;
  sgba::Sem s;
  sgba::point_lists(&s, ST, in, (int)((E + lba::kThreads - 1) / lba::kThreads), (int)((P + lba::kThreads - 1) / lba::kThreads));
  SemLayout L(ST, s);
  // the pinned arena behind the visual lists: the visual outs, then the semantic outs and the semantic lists as one block
  Stage so;
  const size_t sPos = so.add(P * 12), sErase = so.add(NO), sChiK = so.add(NO * 8), sChiP = so.add(NO * 8), sPlane = so.add(Pl * 32),
               sRoom = so.add(R * 24), sIn = so.add(L.in.total);
  const size_t outs[4] = {E, E * 8, K * sizeof(vsg_pose_se3d), so.total}, devs[1] = {L.dev.total};
  Staged G;
  rc = stage_problem(c, F, T, slots, kfs, kf_Tcw, kf_cam, inv_level_sigma2, nlevels, iterations, outs, 4, devs, 1, &G);
  if (rc != VSG_OK) return rc;
  uint8_t *hp = G.hp, *dp = G.dp, *dv = G.dv;
  const size_t in_bytes = G.in_bytes, Ge = G.Ge, Gp = G.Gp, oErase = G.out_off[0], oChi2 = G.out_off[1], oKfOut = G.out_off[2],
               oSem = G.out_off[3];
  uint8_t *hs = hp + oSem + sIn, *ds = dv + G.dev_off[0];  // the semantic block: staged here, read there
  put(hs, L.oKind, ST.e_kind), put(hs, L.oV0, ST.e_v0), put(hs, L.oObs, ST.e_obs), put(hs, L.oFix0, ST.e_fix0), put(hs, L.oPl, ST.e_pl);
  put(hs, L.oW, ST.e_w), put(hs, L.oOkf, ST.o_kf), put(hs, L.oOpl, ST.o_pl), put(hs, L.oOpk, ST.o_pk), put(hs, L.oOpp, ST.o_pp);
  put(hs, L.oAct, ST.pl_act), put(hs, L.oSvRow, ST.sv_row), put(hs, L.oSvItem, ST.sv_item), put(hs, L.oRowSv, ST.row_sv);
  put(hs, L.oVoff, ST.v_off), put(hs, L.oVedge, ST.v_edge), put(hs, L.oVcol, ST.v_col), put(hs, L.oKsOff, ST.ks_off);
  put(hs, L.oKsEdge, ST.ks_edge), put(hs, L.oSbS, ST.sb_s), put(hs, L.oSbT, ST.sb_t), put(hs, L.oSbOff, ST.sb_off);
  put(hs, L.oSbEdge, ST.sb_edge), put(hs, L.oSbCa, ST.sb_ca), put(hs, L.oSbCb, ST.sb_cb);
  if (NO) memcpy(hs + L.oLocal, pl_obs_local, NO * 32), memcpy(hs + L.oG, pl_obs_G, NO * 128);
  sgba::start_values(in, (double *)(hs + L.oPl0), (double *)(hs + L.oPl1), (pose::Est *)(hs + L.oRm0), (pose::Est *)(hs + L.oRm1));
  auto I32 = [&](size_t o) { return (const int32_t *)(ds + o); };
  s.e_kind = I32(L.oKind), s.e_v0 = I32(L.oV0), s.e_obs = I32(L.oObs), s.e_fix0 = I32(L.oFix0), s.e_pl = I32(L.oPl);
  s.e_w = (const double *)(ds + L.oW), s.obs_local = (const double *)(ds + L.oLocal), s.obs_G = (const double *)(ds + L.oG);
  s.o_kf = I32(L.oOkf), s.o_pl = I32(L.oOpl), s.o_pk = I32(L.oOpk), s.o_pp = I32(L.oOpp), s.pl_act = I32(L.oAct);
  s.sv_row = I32(L.oSvRow), s.sv_item = I32(L.oSvItem), s.row_sv = I32(L.oRowSv), s.v_off = I32(L.oVoff), s.v_edge = I32(L.oVedge);
  s.v_col = I32(L.oVcol), s.ks_off = I32(L.oKsOff), s.ks_edge = I32(L.oKsEdge), s.sb_s = I32(L.oSbS), s.sb_t = I32(L.oSbT);
  s.sb_off = I32(L.oSbOff), s.sb_edge = I32(L.oSbEdge), s.sb_ca = I32(L.oSbCa), s.sb_cb = I32(L.oSbCb);
  s.pl[0] = (double *)(ds + L.oPl0), s.pl[1] = (double *)(ds + L.oPl1), s.rm[0] = (pose::Est *)(ds + L.oRm0), s.rm[1] = (pose::Est *)(ds + L.oRm1);
  s.blocks = (double *)(ds + L.dBlocks), s.chi2 = (double *)(ds + L.dChi2), s.cost = (double *)(ds + L.dCost), s.bsem = (double *)(ds + L.dBsem);
  // the reduced system and the controller's partials with the planes and rooms in
  lba::Prob p = G.p;
  p.n = ST.n, p.M = (double *)(ds + L.dM), p.bs = (double *)(ds + L.dBs), p.xp = (double *)(ds + L.dXp);
  p.chiPart = (double *)(ds + L.dChiPart), p.maxPart = (double *)(ds + L.dMaxPart), p.scalePart = (double *)(ds + L.dScalePart);
  lba::Prob pc = p;
  pc.Ge = s.Ge0 + s.Gse, pc.Gp = s.Gp0 + s.Gsr;
  lba::State *mirror_dev = G.mirror_dev;
  uint8_t *dso = dp + oSem;
  FinalArgs FA;
  FA.wb = G.wb, FA.wb.kf_out = (vsg_pose_se3d *)(dp + oKfOut), FA.wb.pos_out = (float *)(dso + sPos);
  FA.erase = dp + oErase, FA.chi2 = (double *)(dp + oChi2);
  FA.erase_plane = dso + sErase, FA.chi2_kf = (double *)(dso + sChiK), FA.chi2_pp = (double *)(dso + sChiP);
  FA.plane_out = (double *)(dso + sPlane), FA.room_out = (double *)(dso + sRoom);

  TRY_HIP(hipMemcpyAsync(dv, hp, in_bytes, hipMemcpyHostToDevice, c->stream));
  hipStream_t st = c->stream;
  if (L.in.total > 0 && hipMemcpyAsync(ds, hs, L.in.total, hipMemcpyHostToDevice, st) != hipSuccess) {
    (void)hipStreamSynchronize(st);  // the first copy reads the pinned arena, which belongs to the next call
    return VSG_ERR_HIP;
  }
  const dim3 B(lba::kThreads);
  const unsigned gLin = (unsigned)((ST.Es + sgba::kEdgesPerGroup - 1) / sgba::kEdgesPerGroup),
                 gGather = (unsigned)(s.Gse + s.Gsr) + (unsigned)((Ko + lba::kThreads - 1) / lba::kThreads);
  const int Gs = G.Gs, Gb = (ST.nbs + sgba::kBlocksPerGroup - 1) / sgba::kBlocksPerGroup;
  const bool sem = ST.Es > 0;  // no semantic edge: no semantic vertex, no semantic row
  hipLaunchKernelGGL(k_setup, dim3(G.gAll), B, 0, st, p, G.SA);
  lba::State Sfin;
  const bool done = lm::run(
      st, G.mirror, iterations, lm::kTrialSlots, stop_flag,
      [&](int it) {
        if (Ge) hipLaunchKernelGGL(k_linearise<lba::HuberLocal>, dim3((unsigned)Ge), B, 0, st, p, it, lba::HuberLocal());
        if (sem) hipLaunchKernelGGL(k_sg_linearise, dim3(gLin), B, 0, st, p, s, it);
        hipLaunchKernelGGL(k_gather, dim3((unsigned)(Gp + Ko)), B, 0, st, p, it);
        if (sem) hipLaunchKernelGGL(k_sg_gather, dim3(gGather), B, 0, st, p, s, it);
        hipLaunchKernelGGL(k_begin, dim3(1), dim3(1), 0, st, pc, it, mirror_dev);
      },
      [&](int it, int q) {
        if (Ge) hipLaunchKernelGGL(k_trial_edges, dim3((unsigned)Ge), B, 0, st, p, it, q);
        hipLaunchKernelGGL(k_schur, dim3((unsigned)(Gs + (int)Ko)), B, 0, st, p, it, q, Gs);
        if (sem) hipLaunchKernelGGL(k_sg_assemble, dim3((unsigned)(Gb + s.Gsr)), B, 0, st, p, s, it, q, Gb);
        hipLaunchKernelGGL(k_solve<kSolveRows>, dim3(1), dim3(lba::kSolveThreads), 0, st, p, it, q);
        hipLaunchKernelGGL(k_backsub, dim3((unsigned)(Gp + 1)), B, 0, st, p, it, q);
        if (sem) hipLaunchKernelGGL(k_sg_oplus, dim3((unsigned)s.Gsr), B, 0, st, p, s, it, q);
        if (Ge) hipLaunchKernelGGL(k_error<lba::HuberLocal>, dim3((unsigned)Ge), B, 0, st, p, it, q, lba::HuberLocal());
        if (sem) hipLaunchKernelGGL(k_sg_error, dim3((unsigned)s.Gse), B, 0, st, p, s, it, q);
        hipLaunchKernelGGL(k_decide, dim3(1), dim3(1), 0, st, pc, it, q, mirror_dev);
      },
      [&] {
        size_t most = E > P ? E : P;
        most = most > K ? most : K, most = most > NO ? most : NO, most = most > Pl ? most : Pl, most = most > R ? most : R;
        hipLaunchKernelGGL(k_sg_final, dim3((unsigned)((most + lba::kThreads - 1) / lba::kThreads)), B, 0, st, p, s, FA);
      },
      &Sfin);
  if (!done) return VSG_ERR_HIP;
  sgba::fill_result(res, T, &ST, &Sfin);
  const uint8_t *he = hp + oErase, *hso = hp + oSem;
  int n_erase = 0, n_erase_plane = 0;
  for (size_t e = 0; e < E; e++) n_erase += he[e] != 0;
  for (size_t o = 0; o < NO; o++) n_erase_plane += hso[sErase + o] != 0;
  res->local.n_erase = n_erase, res->n_erase_plane = n_erase_plane;
  memcpy(erase, he, E);
  if (chi2) memcpy(chi2, hp + oChi2, E * 8);
  memcpy(kf_Tcw_out, hp + oKfOut, K * sizeof(vsg_pose_se3d));
  if (world_pos_out) memcpy(world_pos_out, hso + sPos, P * 12);
  if (NO) memcpy(erase_plane, hso + sErase, NO);
  if (chi2_plane_kf && NO) memcpy(chi2_plane_kf, hso + sChiK, NO * 8);
  if (chi2_plane_point && NO) memcpy(chi2_plane_point, hso + sChiP, NO * 8);
  for (size_t i = 0; i < Pl; i++)  // a plane without an edge is no vertex: its input bytes
    memcpy(plane_eq_out + 4 * i, ST.pl_act[i] >= 0 ? (const double *)(hso + sPlane) + 4 * i : plane_eq + 4 * i, 32);
  if (R) memcpy(room_center_out, hso + sRoom, R * 24);
  return VSG_OK;
}

}  // extern "C"
