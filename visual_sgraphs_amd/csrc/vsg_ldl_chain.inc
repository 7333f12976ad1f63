// vsg_ldl_chain.inc -- the dense blocked LDL^T solve over the whole chip that vsg_global_ba.hip (the reduced system of the
// Schur complement) and vsg_essential_graph.hip (the 7-row pose-graph system) have in common, ONE copy: the schedule of
// csrc/vsg_global_ba.h (gba::solve_reduced_blocked_host is its host form), gated by lba::run_trial on an lba::State.
// Included inside each file's anonymous namespace, after vsg_global_ba.h and an
//   enum { kThreads = lba::kThreads, W = gba::kPanel, TS = gba::kTile, WP = W + 1 };
// so each library object gets its own internal instances.  (The two local bundle adjustments solve in one workgroup:
// k_solve of vsg_ba_kernels.inc.)

static_assert(W % 6 == 0 && W <= kThreads && TS == 64 && kThreads == 256, "the solver's thread maps assume these");

// what the reduced solve's kernels index: the system, the pivots, the two work vectors, the controller
struct Solve {
  int n;
  double *M;         // [n n] row-major, the lower triangle
  const double *bs;  // [n]
  double *xp, *D, *y, *acc;  // [n] each
  int32_t *ok2;
  const lba::State *S;
};

// ---- the reduced solve.  c0 = the panel's first column, w = min(W, n - c0) its width; every index below is < n.

// step 1, ONE workgroup: the diagonal block [c0, c0 + w)^2 in LDS, column by column; its pivots go to D, a pivot <= 0
// clears ok2 (the first panel sets it) and the sweep goes on
__global__ __launch_bounds__(kThreads) void k_ldl_diag(Solve s, int it, int q, int c0) {
  __shared__ double A[W][WP];
  if (!lba::run_trial(*s.S, it, q)) return;
  const int n = s.n, tid = threadIdx.x, w = n - c0 < W ? n - c0 : W;
  for (int x = tid; x < w * w; x += kThreads) {
    const int i = x / w, j = x % w;
    if (j <= i) A[i][j] = s.M[(size_t)(c0 + i) * n + (c0 + j)];
  }
  bool bad = false;
  for (int k = 0; k < w; k++) {
    __syncthreads();  // column k has every update of the columns before it
    const double d = A[k][k];
    if (tid == 0) {
      s.D[c0 + k] = d;
      if (d <= 0.0) bad = true;
    }
    const int r = k + 1 + tid;
    if (r < w) A[r][k] = A[r][k] / d;
    __syncthreads();
    for (int x = tid; x < w * w; x += kThreads) {
      const int i = x / w, j = x % w;
      if (j > k && j <= i) A[i][j] = A[i][j] - (A[i][k] * A[j][k]) * d;
    }
  }
  __syncthreads();
  for (int x = tid; x < w * w; x += kThreads) {
    const int i = x / w, j = x % w;
    if (j < i) s.M[(size_t)(c0 + i) * n + (c0 + j)] = A[i][j];
  }
  if (tid == 0) {
    if (c0 == 0)
      *s.ok2 = bad ? 0 : 1;
    else if (bad)
      *s.ok2 = 0;
  }
}

// step 2, one workgroup per TS rows below the block: row r's entries of the panel's columns become its multipliers, left
// to right: a[k] / D_k, then a[j] -= (l_k L_jk) D_k for the columns j > k.  Lane = row, the four waves share the columns.
__global__ __launch_bounds__(kThreads) void k_ldl_panel(Solve s, int it, int q, int c0) {
  __shared__ double Ld[W][WP], a[TS][WP], Dk[W];
  if (!lba::run_trial(*s.S, it, q)) return;
  const int n = s.n, tid = threadIdx.x, w = n - c0 < W ? n - c0 : W, R0 = c0 + w + blockIdx.x * TS;
  for (int x = tid; x < w * w; x += kThreads) {
    const int j = x / w, k = x % w;
    Ld[j][k] = s.M[(size_t)(c0 + j) * n + (c0 + k)];
  }
  for (int x = tid; x < TS * w; x += kThreads) {
    const int r = x / w, k = x % w;
    a[r][k] = R0 + r < n ? s.M[(size_t)(R0 + r) * n + (c0 + k)] : 0.0;
  }
  if (tid < w) Dk[tid] = s.D[c0 + tid];
  __syncthreads();
  const int r = tid & (TS - 1), part = tid / TS;
  for (int k = 0; k < w; k++) {
    const double d = Dk[k];
    if (part == 0) a[r][k] = a[r][k] / d;
    __syncthreads();
    const double l = a[r][k];
    for (int j = k + 1 + part; j < w; j += kThreads / TS) a[r][j] = a[r][j] - (l * Ld[j][k]) * d;
    __syncthreads();
  }
  for (int x = tid; x < TS * w; x += kThreads) {
    const int rr = x / w, k = x % w;
    if (R0 + rr < n) s.M[(size_t)(R0 + rr) * n + (c0 + k)] = a[rr][k];
  }
}

// step 3, one workgroup per tile (I >= J) of the trailing lower triangle: the panel's L rows of both tiles and its D through
// LDS, a 4 x 4 micro-tile per lane in registers, every element its w updates in ascending k
__global__ __launch_bounds__(kThreads) void k_ldl_trail(Solve s, int it, int q, int c0) {
  __shared__ double Li[TS][WP], Lj[TS][WP], Dk[W];
  if (!lba::run_trial(*s.S, it, q)) return;
  if (blockIdx.x > blockIdx.y) return;  // the upper triangle's tiles
  const int n = s.n, tid = threadIdx.x, w = n - c0 < W ? n - c0 : W, r0 = c0 + w;
  const int I0 = r0 + blockIdx.y * TS, J0 = r0 + blockIdx.x * TS;
  for (int x = tid; x < TS * w; x += kThreads) {
    const int r = x / w, k = x % w;
    Li[r][k] = I0 + r < n ? s.M[(size_t)(I0 + r) * n + (c0 + k)] : 0.0;
    Lj[r][k] = J0 + r < n ? s.M[(size_t)(J0 + r) * n + (c0 + k)] : 0.0;
  }
  if (tid < w) Dk[tid] = s.D[c0 + tid];
  __syncthreads();
  const int tx = tid & 15, ty = tid >> 4;
  double a[4][4];
#pragma unroll
  for (int u = 0; u < 4; u++)
#pragma unroll
    for (int v = 0; v < 4; v++) {
      const int i = I0 + ty + 16 * u, j = J0 + tx + 16 * v;
      a[u][v] = (i < n && j <= i) ? s.M[(size_t)i * n + j] : 0.0;
    }
  for (int k = 0; k < w; k++) {
    const double d = Dk[k];
    double li[4], lj[4];
#pragma unroll
    for (int u = 0; u < 4; u++) li[u] = Li[ty + 16 * u][k], lj[u] = Lj[tx + 16 * u][k];
#pragma unroll
    for (int u = 0; u < 4; u++)
#pragma unroll
      for (int v = 0; v < 4; v++) a[u][v] = a[u][v] - (li[u] * lj[v]) * d;
  }
#pragma unroll
  for (int u = 0; u < 4; u++)
#pragma unroll
    for (int v = 0; v < 4; v++) {
      const int i = I0 + ty + 16 * u, j = J0 + tx + 16 * v;
      if (i < n && j <= i) s.M[(size_t)i * n + j] = a[u][v];
    }
}

// forward, one launch per panel left to right: every workgroup solves the panel's triangle for the panel's y in LDS, then
// lane = row below the panel: y_i -= L_ik y_k, k ascending.  The first panel reads bs.  Workgroup 0 writes the panel's
// y_k / D_k to acc, which no lane of this launch reads.
__global__ __launch_bounds__(kThreads) void k_fwd(Solve s, int it, int q, int c0) {
  __shared__ double Ld[W][WP], ys[W];
  if (!lba::run_trial(*s.S, it, q)) return;
  const int n = s.n, tid = threadIdx.x, w = n - c0 < W ? n - c0 : W;
  const double *src = c0 == 0 ? s.bs : s.y;
  for (int x = tid; x < w * w; x += kThreads) {
    const int j = x / w, k = x % w;
    Ld[j][k] = s.M[(size_t)(c0 + j) * n + (c0 + k)];
  }
  if (tid < w) ys[tid] = src[c0 + tid];
  for (int k = 0; k < w; k++) {
    __syncthreads();
    if (tid > k && tid < w) ys[tid] = ys[tid] - Ld[tid][k] * ys[k];
  }
  __syncthreads();
  const int i = c0 + w + blockIdx.x * kThreads + tid;
  if (i < n) {
    double v = src[i];
    const double *row = s.M + (size_t)i * n + c0;
    for (int k = 0; k < w; k++) v = v - row[k] * ys[k];
    s.y[i] = v;
  }
  if (blockIdx.x == 0 && tid < w) s.acc[c0 + tid] = ys[tid] / s.D[c0 + tid];
}

// backward, one launch per panel right to left: every workgroup solves the panel's transposed triangle for the panel's x in
// LDS, then lane = row before the panel: acc_i -= L_ki x_k, k descending.  Workgroup 0 writes the panel's x to xp.
__global__ __launch_bounds__(kThreads) void k_bwd(Solve s, int it, int q, int c0) {
  __shared__ double Ld[W][WP], xs[W];
  if (!lba::run_trial(*s.S, it, q)) return;
  const int n = s.n, tid = threadIdx.x, w = n - c0 < W ? n - c0 : W;
  for (int x = tid; x < w * w; x += kThreads) {
    const int j = x / w, k = x % w;
    Ld[j][k] = s.M[(size_t)(c0 + j) * n + (c0 + k)];
  }
  if (tid < w) xs[tid] = s.acc[c0 + tid];
  for (int k = w - 1; k > 0; k--) {
    __syncthreads();
    if (tid < k) xs[tid] = xs[tid] - Ld[k][tid] * xs[k];
  }
  __syncthreads();
  const int i = blockIdx.x * kThreads + tid;
  if (i < c0) {
    double v = s.acc[i];
    for (int k = w - 1; k >= 0; k--) v = v - s.M[(size_t)(c0 + k) * n + i] * xs[k];
    s.acc[i] = v;
  }
  if (blockIdx.x == 0 && tid < w) s.xp[c0 + tid] = xs[tid];
}

// the chain: 3 launches per panel (1 for the last), then one per panel forward and one per panel backward
void enqueue_solve(hipStream_t st, const Solve &s, int it, int q) {
  const int n = s.n;
  const dim3 B(kThreads);
  for (int c0 = 0; c0 < n; c0 += W) {
    const int w = n - c0 < W ? n - c0 : W, rows = n - c0 - w;
    hipLaunchKernelGGL(k_ldl_diag, dim3(1), B, 0, st, s, it, q, c0);
    if (rows <= 0) continue;
    const unsigned nt = (unsigned)((rows + TS - 1) / TS);
    hipLaunchKernelGGL(k_ldl_panel, dim3(nt), B, 0, st, s, it, q, c0);
    hipLaunchKernelGGL(k_ldl_trail, dim3(nt, nt), B, 0, st, s, it, q, c0);
  }
  for (int c0 = 0; c0 < n; c0 += W) {
    const int w = n - c0 < W ? n - c0 : W, rows = n - c0 - w;
    hipLaunchKernelGGL(k_fwd, dim3((unsigned)(rows > 0 ? (rows + kThreads - 1) / kThreads : 1)), B, 0, st, s, it, q, c0);
  }
  for (int c0 = (n - 1) / W * W; c0 >= 0; c0 -= W)
    hipLaunchKernelGGL(k_bwd, dim3((unsigned)(c0 > 0 ? (c0 + kThreads - 1) / kThreads : 1)), B, 0, st, s, it, q, c0);
}
