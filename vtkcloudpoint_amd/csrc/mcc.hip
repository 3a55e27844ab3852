// mcc.hip -- Tools.getCircles / Geometry.FindMinimalBoundingCircle on MI355X (the step
// right after centroid extraction, FrmMain.cs:1539-1540).
//
// Reference: BaseClass/Tools.cs:394-409 (one circle per cluster with more than 3 points) and
// BaseClass/Geometry.cs:247-319 (MakeConvexHull :122-208 = gift wrapping on the pseudo-angle of AngleValue
// :220-246; then the smallest circle through 2 or 3 hull points that encloses the hull, first found on ties;
// FindCircle :340-372 via FindIntersection :373-432).  HullCull (:83-120) culls nothing but NaN points: the
// Rectangle2D it compares against never gets Left/Right/Top/Bottom assigned (DataModel.cs:191-208).
//
// The hull builder and the circle search are csrc/hull.hpp (shared with shapes.hip, which adds the rectangle).
#include <cstring>

#include "hull.hpp"
#include "sort.hpp"

extern "C" int vcp_mcc(vcp_ctx* ctx, const double* xy, const int32_t* labels, const int64_t* order, int64_t m, int64_t n,
                       int32_t K, double* centers, double* radius, uint8_t* valid, int32_t* hull_n) {
  if (!ctx) return VCP_ERR_ARG;
  if (m < 0 || n < 0 || K < 0 || (m > 0 && (!xy || !labels))) return vcp_fail(ctx, VCP_ERR_ARG, "bad argument");
  if (K == 0) return VCP_OK;
  if (!centers || !radius || !valid) return vcp_fail(ctx, VCP_ERR_ARG, "null output");
  if (n >= 0x7FFFFFF0LL || m >= 0x7FFFFFF0LL) return vcp_fail(ctx, VCP_ERR_TOO_LARGE, "n beyond 32-bit indexing");
  VCP_TRY(vcp_bind(ctx));
  hipStream_t st = ctx->stream;
  const size_t nn = (size_t)(n > 0 ? n : 1), mm = (size_t)(m > 0 ? m : 1), kk = (size_t)K;
  VCP_TRY(vcp_ensure(ctx, ctx->b_in0, nn * 16));
  VCP_TRY(vcp_ensure(ctx, ctx->b_in3, nn * 4));
  VCP_TRY(vcp_ensure(ctx, ctx->b_in2, mm * 8));
  VCP_TRY(vcp_ensure(ctx, ctx->b_aux0, (kk + 4) * 4 * 2 + 64));
  VCP_TRY(vcp_ensure(ctx, ctx->b_aux4, mm * 16));
  VCP_TRY(vcp_ensure(ctx, ctx->b_aux5, mm));
  VCP_TRY(vcp_ensure(ctx, ctx->b_out0, kk * 16));
  VCP_TRY(vcp_ensure(ctx, ctx->b_out1, kk));
  VCP_TRY(vcp_ensure(ctx, ctx->b_out2, kk * 8));
  VCP_TRY(vcp_ensure(ctx, ctx->b_out3, kk * 4));
  if (m > 0) {
    VCP_HIP(ctx, hipMemcpyAsync(ctx->b_in0.p, xy, (size_t)n * 16, hipMemcpyHostToDevice, st));
    VCP_HIP(ctx, hipMemcpyAsync(ctx->b_in3.p, labels, (size_t)n * 4, hipMemcpyHostToDevice, st));
    if (order) VCP_HIP(ctx, hipMemcpyAsync(ctx->b_in2.p, order, (size_t)m * 8, hipMemcpyHostToDevice, st));
  }
  uint32_t* counts = ctx->b_aux0.as<uint32_t>();   // [K+2], label 0 included
  uint32_t* segstart = counts + (K + 4);
  uint32_t* bad = segstart + (K + 4);
  VCP_HIP(ctx, hipMemsetAsync(counts, 0, (kk + 4) * 4 * 2 + 64, st));
  const uint32_t* sorted = nullptr;
  VCP_TRY(vcp_group_by_label(ctx, ctx->b_in3.as<int32_t>(), order ? ctx->b_in2.as<int64_t>() : nullptr, m, K, ctx->b_aux1,
                             ctx->b_aux2, ctx->b_aux3, segstart, counts, bad, &sorted));
  if (m > 0)
    VCP_LAUNCH(ctx, k_mcc_gather, dim3(vcp_blocks(m, MT)), dim3(MT), 0, st, ctx->b_in0.as<double>(), sorted, m,
                    ctx->b_aux4.as<double>());
  VCP_LAUNCH(ctx, k_mcc, dim3(K), dim3(MT), 0, st, ctx->b_aux4.as<double>(), segstart, counts, ctx->b_aux5.as<uint8_t>(),
                  ctx->b_out0.as<double>(), ctx->b_out2.as<double>(), ctx->b_out1.as<uint8_t>(), ctx->b_out3.as<int32_t>());
  uint32_t* hp = reinterpret_cast<uint32_t*>(ctx->pinned);
  VCP_HIP(ctx, hipMemcpyAsync(hp, bad, 4, hipMemcpyDeviceToHost, st));
  VCP_HIP(ctx, hipMemcpyAsync(centers, ctx->b_out0.p, kk * 16, hipMemcpyDeviceToHost, st));
  VCP_HIP(ctx, hipMemcpyAsync(radius, ctx->b_out2.p, kk * 8, hipMemcpyDeviceToHost, st));
  VCP_HIP(ctx, hipMemcpyAsync(valid, ctx->b_out1.p, kk, hipMemcpyDeviceToHost, st));
  if (hull_n) VCP_HIP(ctx, hipMemcpyAsync(hull_n, ctx->b_out3.p, kk * 4, hipMemcpyDeviceToHost, st));
  VCP_HIP(ctx, hipStreamSynchronize(st));
  if (hp[0] != 0) return vcp_fail(ctx, VCP_ERR_INDEX, "%u labels outside 0..K (clusList[clusterId-1])", hp[0]);
  for (int32_t k = 0; k < K; k++) {
    if (valid[k] == 2) return vcp_fail(ctx, VCP_ERR_TOO_LARGE, "cluster %d: convex hull beyond %d points", k + 1, HMAX);
    if (valid[k] == 3) return vcp_fail(ctx, VCP_ERR_EMPTY, "cluster %d: no finite point", k + 1);
  }
  return VCP_OK;
}
