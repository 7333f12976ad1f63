// vsg_ba_kernels.inc -- the kernels and helpers vsg_local_ba.hip, vsg_sgraph_ba.hip and vsg_global_ba.hip have in common,
// ONE copy: the set-up, the phases around the per-item functions of vsg_local_ba.h, the one-workgroup reduced solve of the
// two local calls (k_solve; the global call has vsg_ldl_chain.inc), k_backsub, and the visual write-back their final
// kernels share.  Included inside each file's anonymous namespace (after vsg_frame_int.h, vsg_local_ba.h, vsg_block_tree.h
// and vsg_lm_driver.h), so each library object gets its own internal instances of the kernels it launches.  k_linearise and
// k_error take the robust kernel as a type: lba::HuberLocal for the local calls (an empty object: the operations they always
// had), gba::Kernel for the global.  At the end, the host's side: ba_prologue checks the store and the keyframes of a call,
// stage_problem lays its lists, start values and scratch out in the calling thread's arenas.

struct KfTab {
  const KeyPointPOD *kps;
  const float *ur;  // nullptr: every mvuRight is -1
};

struct SetupArgs {
  const KfTab *tab;
  const int32_t *e_idx, *slots;
  const float *pos;  // the store's GetWorldPos()
  float sig[16];
};

// Optimizer.cc:1850-1948 (local) / :143-287 (global) for the listed observations: the measurement, the information and the
// kind of every edge; the points' estimates from the store into both buffers
__global__ __launch_bounds__(lba::kThreads) void k_setup(lba::Prob p, SetupArgs A) {
  const int i = blockIdx.x * lba::kThreads + threadIdx.x;
  bool mono = false, stereo = false;
  if (i < p.E) {
    const KfTab t = A.tab[p.e_kf[i]];
    const int idx = A.e_idx[i];
    const KeyPointPOD kp = t.kps[idx];
    const float ur = t.ur ? t.ur[idx] : -1.0f;
    stereo = ur >= 0, mono = !stereo;
    const size_t E = (size_t)p.E;
    p.obs[i] = (double)kp.x, p.obs[E + i] = (double)kp.y, p.obs[2 * E + i] = stereo ? (double)ur : 0.0;
    const int o = kp.octave & 15;
    p.w[i] = (double)A.sig[o];
    p.flag[i] = stereo ? lba::kStereo : 0;
    p.chi2[i] = 0.0;
  }
  // the two edge counts: one integer atomic per wavefront and kind
  const unsigned long long ms = __ballot(stereo), mm = __ballot(mono);
  if ((threadIdx.x & (pose::kWave - 1)) == 0) {
    if (ms) atomicAdd(&p.S->n_stereo, __popcll(ms));
    if (mm) atomicAdd(&p.S->n_mono, __popcll(mm));
  }
  if (i < p.P) {
    const size_t s = (size_t)A.slots[i];
    for (int d = 0; d < 3; d++) p.X[0][3 * (size_t)i + d] = p.X[1][3 * (size_t)i + d] = (double)A.pos[3 * s + d];
  }
  if (i < p.K) p.est[1][i] = p.est[0][i];
}

template <class Kernel>
__global__ __launch_bounds__(lba::kThreads) void k_linearise(lba::Prob p, int it, Kernel kernel) {
  __shared__ double lds[pose::kWaves];
  if (!lba::run_iteration(*p.S, it)) return;
  const int e = blockIdx.x * lba::kThreads + threadIdx.x;
  double v = e < p.E ? lba::linearise_edge(p, e, p.S->cur, kernel) : 0.0;
  block_tree<1, false>(&v, lds);
  if (threadIdx.x == 0) p.chiPart[blockIdx.x] = v;
}

// workgroups [0, Gp): one lane per point; [Gp, Gp + Ko): one workgroup per optimised keyframe
__global__ __launch_bounds__(lba::kThreads) void k_gather(lba::Prob p, int it) {
  __shared__ double lds[pose::kWaves * lba::kHppC];
  if (!lba::run_iteration(*p.S, it)) return;
  const int g = blockIdx.x, tid = threadIdx.x;
  if (g < p.Gp) {
    const int pt = g * lba::kThreads + tid;
    double m = pt < p.P ? lba::gather_point(p, pt) : 0.0;
    block_tree<1, true>(&m, lds);
    if (tid == 0) p.maxPart[g] = m;
    return;
  }
  double acc[lba::kHppC];
  lba::gather_kf_partial(p, g - p.Gp, tid, acc);
  block_tree<lba::kHppC, false>(acc, lds);
  if (tid == 0) lba::gather_kf_store(p, g - p.Gp, acc);
}

__global__ void k_begin(lba::Prob p, int it, lba::State *mirror) {
  if (!lba::run_iteration(*p.S, it)) return;
  lba::begin_iteration(p, it);
  *mirror = *p.S;
}

__global__ __launch_bounds__(lba::kThreads) void k_trial_edges(lba::Prob p, int it, int q) {
  if (!lba::run_trial(*p.S, it, q)) return;
  const int e = blockIdx.x * lba::kThreads + threadIdx.x;
  if (e < p.E) lba::trial_edge(p, e, p.S->lambda);
}

enum { kBlocksPerGroup = lba::kThreads / 36 };  // Schur blocks per workgroup, one lane per entry

// workgroups [0, Gs): kBlocksPerGroup Schur blocks each; [Gs, Gs + Ko): bschur of one optimised keyframe
__global__ __launch_bounds__(lba::kThreads) void k_schur(lba::Prob p, int it, int q, int Gs) {
  __shared__ double lds[pose::kWaves * lba::kC];
  if (!lba::run_trial(*p.S, it, q)) return;
  const int g = blockIdx.x, tid = threadIdx.x;
  if (g < Gs) {
    const int blk = g * kBlocksPerGroup + tid / 36, ent = tid % 36;
    if (tid < kBlocksPerGroup * 36 && blk < p.nb) lba::schur_entry(p, blk, ent / 6, ent % 6, p.S->lambda);
    return;
  }
  double acc[lba::kC];
  lba::bschur_partial(p, g - Gs, tid, acc);
  block_tree<lba::kC, false>(acc, lds);
  if (tid == 0) lba::bschur_store(p, g - Gs, acc);
}

// The reduced system in ONE workgroup: a right-looking LDL^T sweep over the lower triangle in global memory (6 x 128
// keyframes are 768 rows, 4.7 MB of doubles: past LDS, inside L2), column k's multipliers staged in LDS, then the forward
// and backward substitutions with the right-hand side in LDS.  Element (i, j) takes -(L_ik L_jk) D_k in ascending k, which
// is what lba::solve_reduced_host's left-looking loops give it.  One code path for every n <= kN = kSolveRows; a template
// so that only a file that launches it gets an instance (vsg_global_ba.hip does not).
enum { kSolveRows = 6 * lba::kMaxOptKf };
template <int kN>
__global__ __launch_bounds__(lba::kSolveThreads) void k_solve(lba::Prob p, int it, int q) {
  enum { T = lba::kSolveThreads, W = lba::kSolveTile };
  __shared__ double l[kN], D[kN], y[kN];
  __shared__ int bad;
  if (!lba::run_trial(*p.S, it, q)) return;
  const int n = p.n, tid = threadIdx.x, tx = tid % W, ty = tid / W;
  double *M = p.M;
  if (tid == 0) bad = 0;
  for (int k = 0; k < n; k++) {
    __syncthreads();  // step k - 1's updates are visible; its readers are done with l
    const double d = M[(size_t)k * n + k];
    if (tid == 0) {
      D[k] = d;
      if (d <= 0.0) bad = 1;
    }
    for (int i = k + 1 + tid; i < n; i += T) {
      const double v = M[(size_t)i * n + k] / d;
      M[(size_t)i * n + k] = v, l[i] = v;
    }
    __syncthreads();
    for (int i = k + 1 + ty; i < n; i += T / W) {
      const double li = l[i];
      for (int j = k + 1 + tx; j <= i; j += W) M[(size_t)i * n + j] = M[(size_t)i * n + j] - (li * l[j]) * d;
    }
  }
  for (int i = tid; i < n; i += T) y[i] = p.bs[i];
  for (int k = 0; k < n; k++) {
    __syncthreads();
    const double yk = y[k];
    for (int i = k + 1 + tid; i < n; i += T) y[i] = y[i] - M[(size_t)i * n + k] * yk;
  }
  __syncthreads();
  for (int i = tid; i < n; i += T) y[i] = y[i] / D[i];
  for (int k = n - 1; k >= 0; k--) {
    __syncthreads();
    const double xk = y[k];
    for (int i = tid; i < k; i += T) y[i] = y[i] - M[(size_t)k * n + i] * xk;
  }
  __syncthreads();
  for (int i = tid; i < n; i += T) p.xp[i] = y[i];
  if (tid == 0) *p.ok2 = bad ? 0 : 1;
}

// workgroups [0, Gp): one lane per point; [Gp, ...): the optimised keyframes' oplus, one lane per keyframe.  The local
// calls launch ONE such workgroup (Ko <= lba::kMaxOptKf < lba::kThreads), the global call as many as its keyframes need.
__global__ __launch_bounds__(lba::kThreads) void k_backsub(lba::Prob p, int it, int q) {
  __shared__ double lds[pose::kWaves];
  if (!lba::run_trial(*p.S, it, q)) return;
  const int g = blockIdx.x, tid = threadIdx.x, cur = p.S->cur;
  if (g >= p.Gp) {
    const int i = (g - p.Gp) * lba::kThreads + tid;
    if (i < p.Ko) lba::oplus_kf(p, i, cur);
    return;
  }
  const int pt = g * lba::kThreads + tid;
  double v = pt < p.P ? lba::backsub_point(p, pt, cur, p.S->lambda) : 0.0;
  block_tree<1, false>(&v, lds);
  if (tid == 0) p.scalePart[g] = v;
}
static_assert(lba::kMaxOptKf <= lba::kThreads, "one workgroup of k_backsub takes the local calls' keyframes");

template <class Kernel>
__global__ __launch_bounds__(lba::kThreads) void k_error(lba::Prob p, int it, int q, Kernel kernel) {
  __shared__ double lds[pose::kWaves];
  if (!lba::run_trial(*p.S, it, q)) return;
  const int e = blockIdx.x * lba::kThreads + threadIdx.x;
  double v = 0.0;
  if (e < p.E) {
    double err[3], Xc[3], rho1;
    v = lba::edge_cost(p, e, p.S->cur ^ 1, err, Xc, &rho1, kernel);
  }
  block_tree<1, false>(&v, lds);
  if (threadIdx.x == 0) p.chiPart[blockIdx.x] = v;
}

__global__ void k_decide(lba::Prob p, int it, int q, lba::State *mirror) {
  if (!lba::run_trial(*p.S, it, q)) return;
  lba::decide(p);
  *mirror = *p.S;
}

// what the final kernels' visual write-back writes and reads: the caller's two outs, then what stage_problem fills
struct WriteBack {
  vsg_pose_se3d *kf_out;
  float *pos_out;
  const int32_t *slots;
  float *pos;  // the store's, written when write_store
  const vsg_pose_se3 *Tcw;
  const int32_t *opt_of;
};

// Lane i of a final kernel: keyframe i's pose (a vertex's estimate, else its input, widened) and point i's position (a
// vertex's estimate, else what the store holds), which goes back into the store when write_store
__device__ __forceinline__ void write_back(const lba::Prob &p, const WriteBack &A, int i, int cur, bool write_store) {
  if (i < p.K) A.kf_out[i] = A.opt_of[i] >= 0 ? lba::pose_out(p.est[cur][i]) : lba::pose_widened(A.Tcw[i]);
  if (i < p.P) {
    const size_t s = (size_t)A.slots[i];
    const bool vertex = p.p_off[i] != p.p_off[i + 1];
    for (int d = 0; d < 3; d++) {
      const float v = vertex ? pose::canonf((float)p.X[cur][3 * (size_t)i + d]) : A.pos[3 * s + d];
      A.pos_out[3 * (size_t)i + d] = v;
      if (vertex && write_store) A.pos[3 * s + d] = v;
    }
  }
}

// What the three entry points check before their topology: the store, the keyframes (resident, on the store's device) and
// the pointers every one of them needs, with outs_ok the caller's own.  Then, per keyframe, what check_and_build asks for:
// kf_n = the features whose octave the host can see, nleft, and the octave itself.
struct KfLists {
  vsg_frame *const *kfs;
  std::vector<int32_t> kf_n, nleft;
  auto octave() const {
    vsg_frame *const *f = kfs;
    return [f](int k, int i) { return (int)f[k]->h_kps[(size_t)i].octave; };
  }
};

int ba_prologue(vsg_mappoints *mp, int n_kf, vsg_frame *const *kfs, const vsg_pose_se3 *kf_Tcw, const uint8_t *kf_fixed,
                const vsg_ba_camera *kf_cam, const float *inv_level_sigma2, bool outs_ok, StoreFields *F, KfLists *L) {
  if (!store_fields(mp, F) || n_kf < 0 || !inv_level_sigma2 || !outs_ok) return VSG_ERR_INVALID;
  if (n_kf > 0 && (!kfs || !kf_Tcw || !kf_fixed || !kf_cam)) return VSG_ERR_INVALID;
  for (int k = 0; k < n_kf; k++)
    if (frame_check(kfs[k]) != VSG_OK || kfs[k]->device != F->device) return VSG_ERR_INVALID;
  L->kfs = kfs, L->kf_n.resize((size_t)n_kf), L->nleft.resize((size_t)n_kf);
  for (int k = 0; k < n_kf; k++) {
    const size_t have = kfs[k]->h_kps.size();
    L->kf_n[(size_t)k] = (int32_t)((size_t)kfs[k]->n < have ? (size_t)kfs[k]->n : have);
    L->nleft[(size_t)k] = kfs[k]->nleft;
  }
  return VSG_OK;
}

// One call's problem in the CALLING THREAD's arenas.  The pinned arena holds the lists and start values (copied to the device
// arena once: in_bytes), then the controller's mirror and the caller's out blocks; the device arena holds the copy of the
// inputs, then the scratch and the caller's further blocks.
struct Staged {
  lba::Prob p;
  SetupArgs SA;
  size_t in_bytes, Ge, Gp, out_off[4], dev_off[4];
  uint8_t *hp, *dp, *dv;            // pinned arena (host address, device alias), device arena
  lba::State *mirror, *mirror_dev;  // the controller's record for the host's look
  WriteBack wb;                     // the final kernel's: slots, the store, the input poses, opt_of; the caller sets the outs
  unsigned gAll;                    // workgroups that cover edges, points and keyframes
  int Gs;                           // workgroups of Schur blocks
};

// Reserves and fills.  out_bytes / dev_bytes: the sizes of the caller's n_out (<= 4) out blocks behind the mirror and n_dev
// (<= 4) device blocks behind the scratch; their offsets come back in out_off / dev_off.  VSG_OK, or what ctx_reserve
// returned: nothing has been written or enqueued then.
int stage_problem(ThreadCtx *c, const StoreFields &F, const lba::Topology &T, const int32_t *slots, vsg_frame *const *kfs,
                  const vsg_pose_se3 *kf_Tcw, const vsg_ba_camera *kf_cam, const float *inv_level_sigma2, int nlevels,
                  int iterations, const size_t *out_bytes, int n_out, const size_t *dev_bytes, int n_dev, Staged *G) {
  const size_t E = (size_t)T.E, P = (size_t)T.P, K = (size_t)T.K, Ko = (size_t)T.Ko, n = 6 * Ko, nb = T.b_i.size(),
               NP = T.pair_a.size(), Ge = (E + lba::kThreads - 1) / lba::kThreads, Gp = (P + lba::kThreads - 1) / lba::kThreads;
  Stage in;
  const size_t oEkf = in.add(E * 4), oEpt = in.add(E * 4), oEopt = in.add(E * 4), oEidx = in.add(E * 4), oPoff = in.add((P + 1) * 4),
               oSlots = in.add(P * 4), oKoff = in.add((Ko + 1) * 4), oKedge = in.add(T.k_edge.size() * 4), oBi = in.add(nb * 4),
               oBj = in.add(nb * 4), oBoff = in.add((nb + 1) * 4), oPa = in.add(NP * 4), oPb = in.add(NP * 4), oOptKf = in.add(Ko * 4),
               oOptOf = in.add(K * 4), oCam = in.add(K * sizeof(lba::Cam)), oEst0 = in.add(K * sizeof(lba::Est)),
               oTab = in.add(K * sizeof(KfTab)), oTcw = in.add(K * sizeof(vsg_pose_se3)), oState = in.add(sizeof(lba::State)),
               oOk2 = in.add(4);
  G->in_bytes = in.total;
  Stage out = in;
  const size_t oMirror = out.add(sizeof(lba::State));
  for (int k = 0; k < n_out; k++) G->out_off[k] = out.add(out_bytes[k]);
  Stage dev = in;  // the device arena: the copy of the inputs, then the scratch
  const size_t dEst1 = dev.add(K * sizeof(lba::Est)), dX0 = dev.add(P * 24), dX1 = dev.add(P * 24), dObs = dev.add(E * 24),
               dW = dev.add(E * 8), dFlag = dev.add(E), dChi = dev.add(E * 8), dHpl = dev.add(E * 8 * lba::kHpl),
               dHppC = dev.add(E * 8 * lba::kHppC), dHllC = dev.add(E * 8 * lba::kHllC), dBD = dev.add(E * 8 * lba::kHpl),
               dC = dev.add(E * 8 * lba::kC), dHpp = dev.add(Ko * 8 * lba::kHppC), dHll = dev.add(P * 8 * lba::kHllC),
               dM = dev.add(n * n * 8), dBs = dev.add(n * 8), dXp = dev.add(n * 8), dChiPart = dev.add(Ge * 8),
               dMaxPart = dev.add(Gp * 8), dMaxKf = dev.add(Ko * 8), dScale = dev.add(Gp * 8);
  for (int k = 0; k < n_dev; k++) G->dev_off[k] = dev.add(dev_bytes[k]);
  const int rc = ctx_reserve(c, out.total, dev.total);
  if (rc != VSG_OK) return rc;
  uint8_t *hp = G->hp = c->h_pin, *dv = G->dv = c->d_buf;
  G->dp = c->d_pin;
  put(hp, oEkf, T.e_kf), put(hp, oEpt, T.e_pt), put(hp, oEopt, T.e_opt), put(hp, oEidx, T.e_idx), put(hp, oPoff, T.p_off);
  memcpy(hp + oSlots, slots, P * 4);
  put(hp, oKoff, T.k_off), put(hp, oKedge, T.k_edge), put(hp, oBi, T.b_i), put(hp, oBj, T.b_j), put(hp, oBoff, T.b_off);
  put(hp, oPa, T.pair_a), put(hp, oPb, T.pair_b), put(hp, oOptKf, T.opt_kf), put(hp, oOptOf, T.opt_of);
  lba::Cam *cam = (lba::Cam *)(hp + oCam);
  lba::Est *est0 = (lba::Est *)(hp + oEst0);
  KfTab *tab = (KfTab *)(hp + oTab);
  for (size_t k = 0; k < K; k++) {
    cam[k] = lba::Cam{(double)kf_cam[k].fx, (double)kf_cam[k].fy, (double)kf_cam[k].cx, (double)kf_cam[k].cy, (double)kf_cam[k].bf};
    est0[k] = pose::est_from_pose(kf_Tcw[k].q, kf_Tcw[k].t);  // Optimizer.cc:1766, :1783 (local), :124 (global)
    tab[k].kps = kfs[k]->d_kps, tab[k].ur = kfs[k]->has_uright ? kfs[k]->d_uright : nullptr;  // the pointers as they are NOW
  }
  memcpy(hp + oTcw, kf_Tcw, K * sizeof(vsg_pose_se3));
  memset(hp + oState, 0, sizeof(lba::State));
  *(int32_t *)(hp + oOk2) = 1;
  G->mirror = (lba::State *)(hp + oMirror), G->mirror_dev = (lba::State *)(G->dp + oMirror);
  memset(G->mirror, 0, sizeof(*G->mirror));

  lba::Prob &p = G->p;
  memset(&p, 0, sizeof(p));
  p.K = T.K, p.Ko = T.Ko, p.P = T.P, p.E = T.E, p.n = (int)n, p.nb = (int)nb, p.Ge = (int)Ge, p.Gp = (int)Gp, p.iterations = iterations;
  p.e_kf = (const int32_t *)(dv + oEkf), p.e_pt = (const int32_t *)(dv + oEpt), p.e_opt = (const int32_t *)(dv + oEopt);
  p.p_off = (const int32_t *)(dv + oPoff), p.k_off = (const int32_t *)(dv + oKoff), p.k_edge = (const int32_t *)(dv + oKedge);
  p.b_i = (const int32_t *)(dv + oBi), p.b_j = (const int32_t *)(dv + oBj), p.b_off = (const int32_t *)(dv + oBoff);
  p.pair_a = (const int32_t *)(dv + oPa), p.pair_b = (const int32_t *)(dv + oPb), p.opt_kf = (const int32_t *)(dv + oOptKf);
  p.cam = (const lba::Cam *)(dv + oCam), p.obs = (double *)(dv + dObs), p.w = (double *)(dv + dW), p.flag = dv + dFlag;
  p.est[0] = (lba::Est *)(dv + oEst0), p.est[1] = (lba::Est *)(dv + dEst1), p.X[0] = (double *)(dv + dX0), p.X[1] = (double *)(dv + dX1);
  p.chi2 = (double *)(dv + dChi), p.Hpl = (double *)(dv + dHpl), p.HppC = (double *)(dv + dHppC), p.HllC = (double *)(dv + dHllC);
  p.BDinv = (double *)(dv + dBD), p.c = (double *)(dv + dC), p.Hpp = (double *)(dv + dHpp), p.Hll = (double *)(dv + dHll);
  p.M = (double *)(dv + dM), p.bs = (double *)(dv + dBs), p.xp = (double *)(dv + dXp), p.chiPart = (double *)(dv + dChiPart);
  p.maxPart = (double *)(dv + dMaxPart), p.maxKf = (double *)(dv + dMaxKf), p.scalePart = (double *)(dv + dScale);
  p.ok2 = (int32_t *)(dv + oOk2), p.S = (lba::State *)(dv + oState);
  SetupArgs &SA = G->SA;
  memset(&SA, 0, sizeof(SA));
  SA.tab = (const KfTab *)(dv + oTab), SA.e_idx = (const int32_t *)(dv + oEidx), SA.slots = (const int32_t *)(dv + oSlots), SA.pos = F.pos;
  for (int l = 0; l < 16; l++) SA.sig[l] = inv_level_sigma2[l < nlevels ? l : nlevels - 1];
  memset(&G->wb, 0, sizeof(G->wb));
  G->wb.slots = SA.slots, G->wb.pos = F.pos, G->wb.Tcw = (const vsg_pose_se3 *)(dv + oTcw), G->wb.opt_of = (const int32_t *)(dv + oOptOf);
  const size_t most = E > P ? (E > K ? E : K) : (P > K ? P : K);
  G->gAll = (unsigned)((most + lba::kThreads - 1) / lba::kThreads);
  G->Gs = (int)((nb + kBlocksPerGroup - 1) / kBlocksPerGroup);
  G->Ge = Ge, G->Gp = Gp;
  return VSG_OK;
}
