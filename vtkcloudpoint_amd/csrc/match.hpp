// match.hpp -- the per-centroid arithmetic of vcp_match (MainForm.calMatchedCoords + RecorrectMatchingPtsByDistance,
// FrmMain.cs:3572-3618), shared by k_match (match.hip) and the inlier score of vcp_icp_multistart (icp.hip), so that a
// score is vcp_match's count_matched by construction.
#pragma once
#include "nngrid.hpp"

#if defined(__HIPCC__)
namespace mtc {

// matched = M * (c, 1) for a row-major 4x4 M: row by row, left to right, no FMA (the library is built with
// -ffp-contract=off), FrmMain.cs:3572-3587
__device__ __forceinline__ void transform(const double* M, double c0, double c1, double c2, double m[3]) {
#pragma unroll
  for (int r = 0; r < 3; r++) m[r] = c0 * M[4 * r] + c1 * M[4 * r + 1] + c2 * M[4 * r + 2] + M[4 * r + 3];
}

// nearest truth of m by sqrt(dx^2 + dy^2 + dz^2) (binary64, correctly rounded sqrt, getDisP :829-835), strict `<` so the
// lowest index wins ties (:3588-3618).  Returns that distance; `best` receives the index.  GRID: the truths are binned
// (nngrid.hpp) and nng::NNG consecutive lanes (sub = 0..NNG-1) work one m together.
template <bool GRID>
__device__ __forceinline__ double nearest(const double* __restrict__ truths, int T, const NNGrid& ng, const double* m,
                                          int sub, int& best) {
  best = 0;
  double bd;
  if (GRID) {
    nng::query<true>(ng, m, sub, best, bd);
    // the distance the C# holds for the winner (NaN / infinity included: the query only orders finite values)
    double dx = truths[3 * best] - m[0], dy = truths[3 * best + 1] - m[1], dz = truths[3 * best + 2] - m[2];
    bd = sqrt(dx * dx + dy * dy + dz * dz);
  } else {
    {
      double dx = truths[0] - m[0], dy = truths[1] - m[1], dz = truths[2] - m[2];
      bd = sqrt(dx * dx + dy * dy + dz * dz);
    }
    for (int i = 1; i < T; i++) {
      double dx = truths[3 * i] - m[0], dy = truths[3 * i + 1] - m[1], dz = truths[3 * i + 2] - m[2];
      double d = sqrt(dx * dx + dy * dy + dz * dz);
      if (d < bd) {
        bd = d;
        best = i;
      }
    }
  }
  return bd;
}

}  // namespace mtc
#endif
