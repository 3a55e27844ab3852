// bounds.hpp -- bounding box and robust range of a cloud (bounds.hip): what the DBSCAN engine's grid, the k-distance
// lattice, the nearest-neighbour grid and the block partition start from.
#pragma once
#include <functional>

#include "vcp_ctx.hpp"

// The points a pass reads: n points of `stride` doubles, the first gd (2 or 3) of which count; with `group` set only the
// points whose group is in [glo, ghi).
struct BoundsSrc {
  const double* c;
  int64_t n;
  int gd, stride;
  const int32_t* group = nullptr;
  int glo = 0, ghi = 0;
};

// Workgroups of the bounds pass: d_part holds vcp_bounds_parts(n) * 8 doubles.
int vcp_bounds_parts(int64_t n);
// Bounding box, left on the device: d_out[0..3) = min and d_out[3..6) = max per axis over the FINITE coordinates (+inf /
// -inf where an axis has none, axes >= gd included), d_out[6] = number of points with a non-finite coordinate among
// their first gd.  Two launches, no synchronisation.
int vcp_bounds_dev(vcp_ctx* ctx, const BoundsSrc& s, double* d_part, double* d_out);
// The same, read back into h[7]: a slot of ctx->pinned (vcp_ctx.hpp lists who uses which).
int vcp_bounds(vcp_ctx* ctx, const BoundsSrc& s, double* d_part, double* d_out, double* h);

// Robust range.  Up to 8 rounds, per axis a < gd: the mean and sigma of the values inside [lo[a], hi[a]], then
// [lo[a], hi[a]] narrowed to mean +- (8 sigma + pad(lo[a], hi[a])) where that leaves a non-empty range.  Stops early when
// a round moves nothing or when done(lo, hi) holds before a round.  `part` is the per-workgroup workspace of the moments
// pass.  A handful of far outliers then fall outside the range instead of stretching it for the whole cloud.
int vcp_robust_range(vcp_ctx* ctx, const BoundsSrc& s, DevBuf& part, double* lo, double* hi,
                     const std::function<double(double lo, double hi)>& pad,
                     const std::function<bool(const double* lo, const double* hi)>& done);
