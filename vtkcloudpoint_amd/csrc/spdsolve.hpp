// spdsolve.hpp -- solve A x = b for a symmetric positive-definite 2x2 or 3x3 matrix by the square-root-free Cholesky
// factorisation A = L D L^T, the solve of vcp_cluster_spheres (cluster_spheres.hip).  Host and device: same code, same
// rounding (vcp_selftest_spd_solve runs it on the host).  Internal linkage, like symeig.hpp.
//
// All arithmetic is binary64, every operation rounded on its own (the library is built with -ffp-contract=off), / correctly
// rounded.  The operation sequence, which tests/cluster_spheres_ref.py replays (D = 2 or 3):
//
//   in     s = the upper triangle row by row: (a00, a01, a11) or (a00, a01, a02, a11, a12, a22); b [D].
//   1.     p0  = a00
//          l10 = a01 / p0
//          p1  = a11 - l10 * a01
//          D = 3:  l20 = a02 / p0;   t = a12 - l20 * a01;   l21 = t / p1;   p2 = (a22 - l20 * a02) - l21 * t
//   2.     ok  = every pivot p_i is finite and > 0 (a NaN pivot fails both).  Not ok: every x_i = NaN
//          (0x7FF8000000000000), return 0.  Nothing is scaled: no square of an entry is formed, so normal entries up to
//          about DBL_MAX / 4 factor as they stand; subnormal entries have lost their bits and may leave a pivot of 0.
//   3.     y0 = b0;   y1 = b1 - l10 * y0;   D = 3:  y2 = (b2 - l20 * y0) - l21 * y1
//   4.     z_i = y_i / p_i
//   5.     D = 2:  x1 = z1;   x0 = z0 - l10 * x1
//          D = 3:  x2 = z2;   x1 = z1 - l21 * x2;   x0 = (z0 - l10 * x1) - l20 * x2
//   out    return 1.  b is not looked at by the test of step 2: a non-finite b gives non-finite x with ok = 1, which the
//          caller's own finiteness check catches.
//
// The pivots are the Schur complements in the order of the rows.  A semi-definite matrix whose entries and quotients are
// exact (coincident, collinear or coplanar members on a dyadic grid) gives a pivot of exactly 0 and fails; one that rounds
// may leave a tiny positive pivot, and then the caller's results are huge rather than NaN.
#pragma once
#include <cmath>

namespace {

__host__ __device__ inline bool spd_pivot_ok(double p) { return p > 0.0 && p <= 1.7976931348623157e308; }

// s [D (D + 1) / 2], b [D] -> x [D]; returns 1, or 0 (and x = NaN) when a pivot is not finite and > 0
template <int D>
__host__ __device__ inline int spd_solve(const double* s, const double* b, double* x) {
  static_assert(D == 2 || D == 3, "2x2 or 3x3");
#ifdef __HIP_DEVICE_COMPILE__
  const double nan = __longlong_as_double(0x7FF8000000000000LL);
#else
  const double nan = __builtin_nan("");
#endif
  if constexpr (D == 2) {
    const double a00 = s[0], a01 = s[1], a11 = s[2];
    const double p0 = a00, l10 = a01 / p0, p1 = a11 - l10 * a01;
    if (!(spd_pivot_ok(p0) && spd_pivot_ok(p1))) {
      x[0] = x[1] = nan;
      return 0;
    }
    const double y0 = b[0], y1 = b[1] - l10 * y0;
    const double z0 = y0 / p0, z1 = y1 / p1;
    x[1] = z1;
    x[0] = z0 - l10 * z1;
  } else {
    const double a00 = s[0], a01 = s[1], a02 = s[2], a11 = s[3], a12 = s[4], a22 = s[5];
    const double p0 = a00, l10 = a01 / p0, l20 = a02 / p0;
    const double p1 = a11 - l10 * a01, t = a12 - l20 * a01, l21 = t / p1;
    const double p2 = (a22 - l20 * a02) - l21 * t;
    if (!(spd_pivot_ok(p0) && spd_pivot_ok(p1) && spd_pivot_ok(p2))) {
      x[0] = x[1] = x[2] = nan;
      return 0;
    }
    const double y0 = b[0], y1 = b[1] - l10 * y0, y2 = (b[2] - l20 * y0) - l21 * y1;
    const double z0 = y0 / p0, z1 = y1 / p1, z2 = y2 / p2;
    const double x2 = z2, x1 = z1 - l21 * x2;
    x[2] = x2;
    x[1] = x1;
    x[0] = (z0 - l10 * x1) - l20 * x2;
  }
  return 1;
}

}  // namespace
