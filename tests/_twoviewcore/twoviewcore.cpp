// Host build of TwoViewReconstruction's arithmetic (vsg_two_view.h), for tests/two_view_hostcore.py: the same source the
// kernels of vsg_two_view.hip compile, against the NumPy restatement and against the device.
#include "vsg_two_view.h"

#include <vector>

using namespace vsg;

// the null vector (double, before any rounding) of n row-major float systems of `rows` x 9 (rows = 16 or 8), with
// `sweeps` sweeps when that is one of 1 .. 12 (the sweep-count trial), the header's count otherwise
template <int M, int SW>
static void null_of(const float *A, double *v) {
  JacobiRegs<M, 9> s;
  for (int r = 0; r < M; r++)
    for (int c = 0; c < 9; c++) s.at(r, c) = (double)A[9 * r + c];
  for (int r = M; r < M + 9; r++) jacobi_identity_row<M, 9>(s, r);
  jacobi_sweeps<M, 9, SW>(s);
  jacobi_null_vector<M, 9>(s, v);
}
template <int M>
static void null_sw(const float *A, double *v, int sweeps) {
  switch (sweeps) {
    case 1: return null_of<M, 1>(A, v);
    case 2: return null_of<M, 2>(A, v);
    case 3: return null_of<M, 3>(A, v);
    case 4: return null_of<M, 4>(A, v);
    case 5: return null_of<M, 5>(A, v);
    case 6: return null_of<M, 6>(A, v);
    case 7: return null_of<M, 7>(A, v);
    case 8: return null_of<M, 8>(A, v);
    case 9: return null_of<M, 9>(A, v);
    case 10: return null_of<M, 10>(A, v);
    case 11: return null_of<M, 11>(A, v);
    case 12: return null_of<M, 12>(A, v);
    default: return null_of<M, two_view::kSweeps9>(A, v);
  }
}
extern "C" {

int tv_sizes(int *match, int *result, int *params, int *sweeps3) {
  *match = (int)sizeof(two_view::Match), *result = (int)sizeof(vsg_two_view_result), *params = (int)sizeof(vsg_two_view_params);
  *sweeps3 = two_view::kSweeps3;
  return two_view::kSweeps9;
}

// Normalize of n keypoints {x, y}: out = {mean_x, mean_y, sx, sy}, T = the 3 x 3 matrix
void tv_normalize(int n, const float *xy, float *out, float *T) {
  const two_view::Norm nm = two_view::normalize(n, [&](int i, float *x, float *y) { *x = xy[2 * (size_t)i], *y = xy[2 * (size_t)i + 1]; });
  out[0] = nm.mean_x, out[1] = nm.mean_y, out[2] = nm.sx, out[3] = nm.sy;
  two_view::norm_matrix(nm, T);
}

void tv_null_vectors(int n, int rows, const float *A, int sweeps, double *v) {
  for (int i = 0; i < n; i++) {
    if (rows == 16)
      null_sw<16>(A + 144 * (size_t)i, v + 9 * (size_t)i, sweeps);
    else
      null_sw<8>(A + 72 * (size_t)i, v + 9 * (size_t)i, sweeps);
  }
}

// U, w, V of n float 3 x 3 matrices
void tv_svd3(int n, const float *A, float *U, float *w, float *V) {
  for (int i = 0; i < n; i++) two_view::svd3(A + 9 * (size_t)i, U + 9 * (size_t)i, w + 3 * (size_t)i, V + 9 * (size_t)i);
}

// every hypothesis of one model on N matches m (N x 8 floats: two_view::Match; nm1 / nm2 = tv_normalize's out): model[it] = H21 | H12 (18 floats) or F21
// (9 floats, the rest 0), terms[it][i] = {t1, t2}, flags[it][i], scores[it] (raw)
void tv_hypotheses(int model, int N, const float *m, int n_iter, const int32_t *sets, const float *nm1, const float *nm2,
                   float sigma, float *models, float *terms, uint8_t *flags, float *scores) {
  const two_view::Match *M = (const two_view::Match *)m;
  const two_view::Norm a = {nm1[0], nm1[1], nm1[2], nm1[3]}, b = {nm2[0], nm2[1], nm2[2], nm2[3]};
  float T1[9], T2[9], T2x[9];  // T2x = T2.inverse() for H, T2.transpose() for F, as the header's callers form them
  two_view::norm_matrix(a, T1), two_view::norm_matrix(b, T2);
  if (model == two_view::kModelH)
    two_view::inverse3(T2, T2x);
  else
    two_view::transpose3(T2, T2x);
  const float inv_s2 = two_view::inv_sigma_square(sigma);
  for (int it = 0; it < n_iter; it++) {
    const int32_t *set = sets + 8 * (size_t)it;
    auto pt = [&](int j, float *p) {
      const two_view::Match &q = M[set[j]];
      p[0] = q.x1, p[1] = q.y1, p[2] = q.x2, p[3] = q.y2;
    };
    float *mo = models + 18 * (size_t)it;
    for (int k = 0; k < 18; k++) mo[k] = 0.0f;
    if (model == two_view::kModelH) {
      JacobiRegs<16, 9> s;
      two_view::hypothesis_h(s, pt, T1, T2x, mo, mo + 9);
    } else {
      JacobiRegs<8, 9> s;
      two_view::hypothesis_f(s, pt, T1, T2x, mo);
    }
    float score = 0.0f;
    for (int i = 0; i < N; i++) {
      float t1, t2;
      const bool in = model == two_view::kModelH ? two_view::score_h(mo, mo + 9, M[i], inv_s2, &t1, &t2)
                                                 : two_view::score_f(mo, M[i], inv_s2, &t1, &t2);
      terms[2 * ((size_t)it * N + i)] = t1, terms[2 * ((size_t)it * N + i) + 1] = t2, flags[(size_t)it * N + i] = in ? 1 : 0;
      score = fadd(fadd(score, t1), t2);
    }
    scores[it] = score;
  }
}

int tv_first_maximum(const float *scores, int n_iter) { return two_view::first_maximum(scores, n_iter); }

// the motion hypotheses of a model: 8 x 12 floats (R row-major, t); returns how many (0: the singular-value gate)
int tv_motions(int model, const float *M21, const float *K, float *out) {
  two_view::Motion mo[8];
  for (int k = 0; k < 96; k++) out[k] = 0.0f;
  int n = 4;
  if (model == two_view::kModelH)
    n = two_view::motions_h(M21, K, mo) ? 8 : 0;
  else
    two_view::motions_f(M21, K, mo);
  for (int h = 0; h < n; h++) {
    for (int k = 0; k < 9; k++) out[12 * h + k] = mo[h].R[k];
    for (int k = 0; k < 3; k++) out[12 * h + 9 + k] = mo[h].t[k];
  }
  return n;
}

// CheckRT of one motion hypothesis over N matches with inlier flags: state, cos, pos per match; returns nGood, *cosine =
// the ranked cosine
int tv_check_rt(const float *Rt, const float *K, float sigma, int N, const float *m, const uint8_t *inlier, uint8_t *state,
                float *cosv, float *pos, float *cosine) {
  two_view::Motion mo;
  for (int k = 0; k < 9; k++) mo.R[k] = Rt[k];
  for (int k = 0; k < 3; k++) mo.t[k] = Rt[9 + k];
  const two_view::RtSetup c = two_view::rt_setup(mo, K, sigma);
  const two_view::Match *M = (const two_view::Match *)m;
  int n_good = 0;
  for (int i = 0; i < N; i++) {
    state[i] = 0, cosv[i] = 0.0f;
    if (!inlier[i]) continue;
    state[i] = (uint8_t)two_view::check_rt_match(c, M[i], pos + 3 * (size_t)i, cosv + i);
    n_good += state[i] != two_view::kRtSkipped ? 1 : 0;
  }
  *cosine = two_view::ranked_cosine(cosv, state, N, n_good);
  return n_good;
}

float tv_ranked_cosine(const float *cosv, const uint8_t *state, int n, int n_good) {
  return two_view::ranked_cosine(cosv, state, n, n_good);
}

// out = {k, reason}
void tv_choose(int model, const int32_t *n_good, int N, int min_triangulated, int32_t *out) {
  const two_view::Choice ch = model == two_view::kModelH ? two_view::choose_h(n_good, N, min_triangulated)
                                                         : two_view::choose_f(n_good, N, min_triangulated);
  out[0] = ch.k, out[1] = ch.reason;
}

// what vsg_two_view_reconstruct refuses before it enqueues: the number of matches (>= 8) when the arguments pass, else -1
int tv_args_ok(const float *xy1, int n1, const float *xy2, int n2, const int32_t *matches12, const float *K,
               const vsg_two_view_params *params, int n_iter, const int32_t *sets) {
  if (!xy1 || !xy2 || !matches12 || !sets || n1 < 1 || n2 < 1 || !two_view::params_ok(K, params, n_iter)) return -1;
  std::vector<int32_t> pairs(2 * (size_t)n1);
  const int N = two_view::compact_matches(n1, n2, matches12, pairs.data());
  return N >= 8 && two_view::sets_ok(N, n_iter, sets) ? N : -1;
}

// the whole call on arrays the caller holds (two_view::reconstruct_host); the optional outputs may be NULL
void tv_reconstruct(const float *xy1, int n1, const float *xy2, int n2, const int32_t *matches12, const float *K,
                    const vsg_two_view_params *params, int n_iter, const int32_t *sets, int two_threads, vsg_two_view_result *res,
                    uint8_t *triangulated, float *x3d, uint8_t *inlier_h, uint8_t *inlier_f, float *score_h, float *score_f) {
  two_view::HostScratch W;
  two_view::reconstruct_host(xy1, n1, xy2, n2, matches12, K, *params, n_iter, sets, two_threads != 0, W, res, triangulated, x3d,
                             inlier_h, inlier_f, score_h, score_f);
}
}
