// symeig.hpp -- eigenvalues and eigenvectors of a symmetric 2x2 or 3x3 matrix by cyclic Jacobi rotations, the solve of
// vcp_cluster_moments (cluster_moments.hip).  Host and device: same code, same rounding (vcp_selftest_sym_eig runs it on
// the host).  Internal linkage, like horn.hpp.
//
// All arithmetic is binary64, every operation rounded on its own (the library is built with -ffp-contract=off), sqrt and
// / correctly rounded.  The operation sequence, which tests/cluster_moments_ref.py replays (D = 2 or 3):
//
//   in     s = the upper triangle row by row: (xx, xy, yy) or (xx, xy, xz, yy, yz, zz).  A = the symmetric matrix, V = I.
//   0.     An entry of s that is NaN or +-inf: every entry of eval and evec is NaN (0x7FF8000000000000), sweeps = 0.
//   1.     g = the largest |entry| of s; (., e) = frexp(g) (e = 0 for g = 0); A = ldexp(A, -e).  Exact: the largest entry
//          now lies in [0.5, 1), so no sum of two entries overflows and the angle below is formed without overflow.
//   2.     for sweep = 0 .. SYMEIG_SWEEPS - 1:  stop when a01 == 0 (&& a02 == 0 && a12 == 0 for D = 3), each exactly;
//          else rotate (0,1), then (0,2), then (1,2) (D = 2: (0,1) alone: one rotation solves it) and count the sweep.
//          rotate (p,q), with r the third index; skipped when a_pq == 0:
//              theta = (a_qq - a_pp) / (2.0 * a_pq)
//              t     = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0))
//              c     = 1.0 / sqrt(t * t + 1.0);   s = t * c;   h = t * a_pq
//              a_pp  = a_pp - h;   a_qq = a_qq + h;   a_pq = 0.0   (set, not computed)
//              D = 3:  x = a_rp, y = a_rq;   a_rp = c * x - s * y;   a_rq = s * x + c * y
//              for k = 0 .. D-1:  x = V[k][p], y = V[k][q];   V[k][p] = c * x - s * y;   V[k][q] = s * x + c * y
//          Rutishauser's form: t is the root of smaller magnitude of t^2 + 2 theta t - 1.  A theta or theta^2 that
//          overflows (|a_pq| below about 1e-154 of the diagonal gap) needs no branch: theta * theta + 1.0 is +inf, its
//          sqrt and the denominator are +inf, t = +-0, c = 1, s = +-0, h = +-0: the rotation only sets a_pq to 0.
//          Off-diagonal entries shrink at least quadratically per sweep once they are small, down to products that
//          round to 0: the stop at exact zeros is reached (at most 6 sweeps on everything tests/test_cluster_moments.py
//          draws); the cap only bounds the loop, and what is on the diagonal then is reported all the same.
//   3.     lam_i = ldexp(a_ii, e) + 0.0  (one rounding when the result is subnormal, +inf when it overflows; -0 -> +0).
//          A negative lam (rounding, a rank-deficient matrix) is reported as computed.
//   4.     order: descending lam, equal values in the order of their diagonal position i (a stable sort of 0..D-1).
//   5.     eval[j] = lam of the j-th in that order; evec[j*D .. j*D+D) = ROW j = column order[j] of V, negated (exact)
//          when its component of largest magnitude, the first such on a tie, is negative.
//   out    the rows of evec are orthonormal to rounding; the sign rule fixes each row on its own, so det(evec) may be
//          -1: evec is an orthonormal basis, not always a rotation.  The all-zero matrix gives lam = +0 and evec = I.
//
// Every index is a compile-time constant, so on the device A and V live in registers (see horn.hpp).
#pragma once
#include <cmath>

#define SYMEIG_SWEEPS 32

namespace {

template <int D, int P, int Q>
__host__ __device__ inline void symeig_rot(double (&A)[3][3], double (&V)[3][3]) {
  const double apq = A[P][Q];
  if (apq == 0.0) return;
  const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
  const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c, h = t * apq;
  A[P][P] = A[P][P] - h;
  A[Q][Q] = A[Q][Q] + h;
  A[P][Q] = 0.0;
  A[Q][P] = 0.0;
  if constexpr (D == 3) {
    constexpr int R = 3 - P - Q;
    const double x = A[R][P], y = A[R][Q];
    A[R][P] = A[P][R] = c * x - s * y;
    A[R][Q] = A[Q][R] = s * x + c * y;
  }
#pragma unroll
  for (int k = 0; k < D; k++) {
    const double x = V[k][P], y = V[k][Q];
    V[k][P] = c * x - s * y;
    V[k][Q] = s * x + c * y;
  }
}

// s [D (D + 1) / 2] -> eval [D], evec [D * D]; returns the sweeps made
template <int D>
__host__ __device__ inline int sym_eig(const double* s, double* eval, double* evec) {
  static_assert(D == 2 || D == 3, "2x2 or 3x3");
  double A[3][3], V[3][3];
  bool finite = true;
  double g = 0.0;
#pragma unroll
  for (int r = 0; r < D; r++)
#pragma unroll
    for (int c = r; c < D; c++) {
      const double x = s[r * D - r * (r - 1) / 2 + (c - r)];
      const double a = fabs(x);
      finite = finite && (a <= 1.7976931348623157e308);  // false for NaN
      g = a > g ? a : g;
      A[r][c] = A[c][r] = x;
    }
  if (!finite) {
#ifdef __HIP_DEVICE_COMPILE__
    const double nan = __longlong_as_double(0x7FF8000000000000LL);
#else
    const double nan = __builtin_nan("");
#endif
#pragma unroll
    for (int j = 0; j < D; j++) eval[j] = nan;
#pragma unroll
    for (int j = 0; j < D * D; j++) evec[j] = nan;
    return 0;
  }
  int e;
  (void)frexp(g, &e);
#pragma unroll
  for (int r = 0; r < D; r++)
#pragma unroll
    for (int c = 0; c < D; c++) {
      A[r][c] = ldexp(A[r][c], -e);
      V[r][c] = r == c ? 1.0 : 0.0;
    }
  int sweeps = 0;
  for (; sweeps < SYMEIG_SWEEPS; sweeps++) {
    if (D == 2 ? A[0][1] == 0.0 : (A[0][1] == 0.0 && A[0][2] == 0.0 && A[1][2] == 0.0)) break;
    symeig_rot<D, 0, 1>(A, V);
    if constexpr (D == 3) {
      symeig_rot<D, 0, 2>(A, V);
      symeig_rot<D, 1, 2>(A, V);
    }
  }
  double lam[3];
#pragma unroll
  for (int i = 0; i < D; i++) lam[i] = ldexp(A[i][i], e) + 0.0;
  // the rank of every diagonal position in (descending lam, ascending position): no dynamic index
#pragma unroll
  for (int i = 0; i < D; i++) {
    int rank = 0;
#pragma unroll
    for (int k = 0; k < D; k++) rank += (lam[k] > lam[i] || (lam[k] == lam[i] && k < i)) ? 1 : 0;
    double v[3];
#pragma unroll
    for (int k = 0; k < D; k++) v[k] = V[k][i];
    double big = fabs(v[0]);
    bool neg = v[0] < 0.0;
#pragma unroll
    for (int k = 1; k < D; k++)
      if (fabs(v[k]) > big) {
        big = fabs(v[k]);
        neg = v[k] < 0.0;
      }
    // selects, not stores under a branch: for D = 2 the compiler folds `if (rank == j) eval[j] = ...` over j = 0, 1 into
    // eval[rank] = ..., a dynamic index, and the caller's arrays go to scratch.  Every rank is taken exactly once, so
    // every entry is written; the first pass reads nothing (i == 0 selects against a constant).
#pragma unroll
    for (int j = 0; j < D; j++) {
      const bool here = rank == j;
      eval[j] = here ? lam[i] : (i == 0 ? 0.0 : eval[j]);
#pragma unroll
      for (int k = 0; k < D; k++) evec[j * D + k] = here ? (neg ? -v[k] : v[k]) : (i == 0 ? 0.0 : evec[j * D + k]);
    }
  }
  return sweeps;
}

// shape [4] of vcp_cluster_moments from eval / evec (vcp.h): (sigma_max, sigma_min_inplane, flatness, tilt); all NaN when
// the eigenvalues are NaN
template <int D>
__host__ __device__ inline void sym_eig_shape(const double* eval, const double* evec, double* shape) {
  if (eval[0] != eval[0]) {
    shape[0] = shape[1] = shape[2] = shape[3] = eval[0];
    return;
  }
  shape[0] = sqrt(eval[0] > 0.0 ? eval[0] : 0.0);
  shape[1] = sqrt(eval[1] > 0.0 ? eval[1] : 0.0);
  if constexpr (D == 3) {
    const double sum = (eval[0] + eval[1]) + eval[2];
    shape[2] = sum == 0.0 ? 0.0 : eval[2] / sum;
    shape[3] = fabs(evec[8]);
  } else {
    shape[2] = 0.0;
    shape[3] = 1.0;
  }
}

}  // namespace
