// vsg_jacobi.h -- the one-sided (Hestenes) Jacobi on the columns of a small M x N matrix, in double, host and device from
// one source.  GeometricTools::Triangulate's 4 x 4 system (vsg_triangulate.h), the 16 x 9 / 8 x 9 systems of ComputeH21 /
// ComputeF21 and the 3 x 3 decompositions of TwoViewReconstruction (vsg_two_view.h) all take a singular vector from
// Eigen's float JacobiSVD, which cannot be restated bit for bit without Eigen; all of them run THIS routine instead and
// round its double result to float once.
//
// The work matrix W has M + N rows of N doubles: rows [0, M) start as A and end as U * Sigma, rows [M, M + N) start as the
// identity and end as V.  A sweep visits the column pairs (p, q), p < q, in lexicographic order and rotates the pair to
// orthogonality (gamma == 0: already orthogonal, skipped); the number of sweeps is a compile-time constant.  Every
// operation is one vsg::d* call = one rounding and the sums run over the rows in ascending order, so the result does not
// depend on WHO applies a rotation to which row.  That is what the storage policy S decides:
//   JacobiRegs<M, N>   the matrix in registers (or on the host's stack), every row by the caller itself: loops are
//                      compile-time bounded and every index is a constant after unrolling;
//   a policy of the caller's (k_tv_hypotheses: the matrix in LDS, row r rotated by lane r, a barrier between the pairs).
// A policy provides  double &at(int row, int col),  template <class F> void rows(F f)  (f(r) for every row r, by someone)
// and  void sync()  (what rows() wrote is visible to every at() behind it).
#pragma once
#include "vsg_math.h"

#if defined(__HIPCC__)
#define VSG_JAC_UNROLL _Pragma("unroll")
#define VSG_JAC_ROLLED _Pragma("unroll 1")
#else
#define VSG_JAC_UNROLL
#define VSG_JAC_ROLLED
#endif

namespace vsg {

template <int M, int N>
struct JacobiRegs {
  static constexpr bool kUnrolled = true;
  double w[M + N][N];
  VSG_HD double &at(int r, int c) { return w[r][c]; }
  template <class F>
  VSG_HD void rows(F f) {
    VSG_JAC_UNROLL
    for (int r = 0; r < M + N; r++) f(r);
  }
  VSG_HD void sync() {}
};

// rows [M, M + N) = the identity (rows [0, M) are the caller's to fill, through rows() as well)
template <int M, int N, class S>
VSG_HD void jacobi_identity_row(S &s, int r) {
  VSG_JAC_UNROLL
  for (int c = 0; c < N; c++) s.at(r, c) = r - M == c ? 1.0 : 0.0;
}

// one column pair: rotate columns p and q of W to orthogonality
template <int M, int N, class S>
VSG_HD void jacobi_pair(S &s, int p, int q) {
  double alpha = 0.0, beta = 0.0, gamma = 0.0;
  VSG_JAC_UNROLL
  for (int k = 0; k < M; k++) {
    const double up = s.at(k, p), uq = s.at(k, q);
    alpha = dadd(alpha, dmul(up, up));
    beta = dadd(beta, dmul(uq, uq));
    gamma = dadd(gamma, dmul(up, uq));
  }
  if (gamma == 0.0) return;  // the same value for everyone who reads the matrix
  const double zeta = ddiv(dsub(beta, alpha), dmul(2.0, gamma));
  const double az = zeta < 0.0 ? -zeta : zeta;
  const double ta = ddiv(1.0, dadd(az, dsqrt(dadd(1.0, dmul(zeta, zeta)))));
  const double t = zeta < 0.0 ? -ta : ta;
  const double cs = ddiv(1.0, dsqrt(dadd(1.0, dmul(t, t)))), sn = dmul(cs, t);
  s.sync();  // every sum above is taken before a row changes
  s.rows([&](int k) {
    const double wp = s.at(k, p), wq = s.at(k, q);
    s.at(k, p) = dsub(dmul(cs, wp), dmul(sn, wq)), s.at(k, q) = dadd(dmul(sn, wp), dmul(cs, wq));
  });
  s.sync();
}

// S::kUnrolled: the pair loops unrolled, so that p and q are constants (a matrix in registers needs that); otherwise
// they stay loops (a matrix in memory: 36 pairs of a 9-column system times the sweeps would be half a megabyte of code)
template <int M, int N, int SWEEPS, class S>
VSG_HD void jacobi_sweeps(S &s) {
  if constexpr (S::kUnrolled) {
    VSG_JAC_UNROLL
    for (int sweep = 0; sweep < SWEEPS; sweep++) {
      VSG_JAC_UNROLL
      for (int p = 0; p < N - 1; p++) {
        VSG_JAC_UNROLL
        for (int q = p + 1; q < N; q++) jacobi_pair<M, N>(s, p, q);
      }
    }
  } else {
    VSG_JAC_ROLLED
    for (int sweep = 0; sweep < SWEEPS; sweep++) {
      VSG_JAC_ROLLED
      for (int p = 0; p < N - 1; p++) {
        VSG_JAC_ROLLED
        for (int q = p + 1; q < N; q++) jacobi_pair<M, N>(s, p, q);
      }
    }
  }
}

// squared norm of column c of U * Sigma
template <int M, int N, class S>
VSG_HD double jacobi_column_norm2(S &s, int c) {
  double nrm = 0.0;
  VSG_JAC_UNROLL
  for (int k = 0; k < M; k++) nrm = dadd(nrm, dmul(s.at(k, c), s.at(k, c)));
  return nrm;
}

// the right singular vector of the least singular value: the column of V whose column of U * Sigma has the least squared
// norm, the lowest index on a tie
template <int M, int N, class S>
VSG_HD void jacobi_null_vector(S &s, double *v) {
  double best = 0.0;
  VSG_JAC_UNROLL
  for (int c = 0; c < N; c++) {
    const double nrm = jacobi_column_norm2<M, N>(s, c);
    if (c == 0 || nrm < best) {
      best = nrm;
      VSG_JAC_UNROLL
      for (int k = 0; k < N; k++) v[k] = s.at(M + k, c);
    }
  }
}

}  // namespace vsg
