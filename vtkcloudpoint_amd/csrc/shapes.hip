// shapes.hip -- per-cluster shapes and the radius / aspect filter (include/vcp.h, "cluster shapes"; DESIGN.md
// section 12): vcp_cluster_shapes[_dev] = convex hull, minimal bounding circle and minimum-area bounding rectangle of
// every cluster in one pass (csrc/hull.hpp: the hull is built once per workgroup and feeds all three);
// vcp_cluster_filter[_dev] = MainForm.FilterClustersByRadius (FrmMain.cs:1905-1920) with the README's length / width
// criterion beside it, and the stable removal of Tools.removeFilterPointFromClustering (BaseClass/Tools.cs:70-74).
#include <cstring>
#include <vector>

#include "hull.hpp"
#include "sort.hpp"
#include "wave.hpp"

namespace {
constexpr int FT = 256;

__global__ __launch_bounds__(MT) void k_shapes(const double* __restrict__ cxy, const uint32_t* __restrict__ segstart,
                                              const uint32_t* __restrict__ counts, uint8_t* __restrict__ removed,
                                              double* __restrict__ centers, double* __restrict__ radius,
                                              uint8_t* __restrict__ valid, int32_t* __restrict__ hull_n, ShapeOut so) {
  cluster_fit<true>(cxy, segstart, counts, removed, centers, radius, valid, hull_n, so);
}

// hull of cluster k: from its member slots (hull_pt at segstart[k]) to its place in the packed list
__global__ __launch_bounds__(64) void k_hull_export(const uint32_t* __restrict__ hull_pt, const uint32_t* __restrict__ segstart,
                                                   const int32_t* __restrict__ hull_n, const uint8_t* __restrict__ valid,
                                                   const int32_t* __restrict__ hull_off, int32_t* __restrict__ hull_idx) {
  const int k = blockIdx.x + 1;
  if (valid[k - 1] != 1) return;
  const int h = hull_n[k - 1];
  const uint32_t* src = hull_pt + segstart[k];
  int32_t* dst = hull_idx + hull_off[k - 1];
  for (int j = threadIdx.x; j < h; j += 64) dst[j] = (int32_t)src[j];
}

// filtered[k] by plain comparisons: a NaN or +inf threshold switches its criterion off
__global__ __launch_bounds__(FT) void k_filter_clusters(const double* __restrict__ radius, const uint8_t* __restrict__ valid,
                                                       const double* __restrict__ rect_len,
                                                       const uint8_t* __restrict__ rect_valid, int32_t K, double max_radius,
                                                       double max_aspect, uint8_t* __restrict__ filtered,
                                                       uint32_t* __restrict__ n_filtered) {
  const int k = blockIdx.x * FT + threadIdx.x;
  bool f = false;
  if (k < K) {
    f = valid[k] == 1 && radius[k] > max_radius;
    if (valid[k] == 1 && rect_len && rect_valid && rect_valid[k] == 1) {
      const double a = rect_len[2 * k], b = rect_len[2 * k + 1];
      f = f || (a > b ? a : b) > max_aspect * (a > b ? b : a);
    }
    filtered[k] = f ? 1 : 0;
  }
  const uint32_t c = wave_count(f);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(n_filtered, c);
}

// keep[i] and its 32-bit twin for the scan; counters: [1] kept points, [2] labels outside 0..K
__global__ __launch_bounds__(FT) void k_filter_points(const int32_t* __restrict__ labels, int64_t n, int32_t K,
                                                     const uint8_t* __restrict__ filtered, uint8_t* __restrict__ keep,
                                                     uint32_t* __restrict__ flag, uint32_t* __restrict__ counters) {
  const int64_t i = (int64_t)blockIdx.x * FT + threadIdx.x;
  bool kp = false, bad = false;
  if (i < n) {
    const int32_t l = labels[i];
    bad = l < 0 || l > K;
    kp = !(l >= 1 && l <= K && filtered[l - 1]);
    if (keep) keep[i] = kp ? 1 : 0;
    if (flag) flag[i] = kp ? 1u : 0u;
  }
  __shared__ uint32_t wc[2 * FT / 64];
  uint32_t a, b;
  if (block_count<FT>(kp, bad, wc, a, b)) {
    if (a) atomicAdd(counters + 1, a);
    if (b) atomicAdd(counters + 2, b);
  }
}

// pos = exclusive scan of the keep flags, pos[n] = their total: point i is kept where the scan steps
__global__ __launch_bounds__(FT) void k_filter_compact(const uint32_t* __restrict__ pos, int64_t n,
                                                      int32_t* __restrict__ kept_idx) {
  const int64_t i = (int64_t)blockIdx.x * FT + threadIdx.x;
  if (i >= n) return;
  const uint32_t p = pos[i];
  if (pos[i + 1] != p) kept_idx[p] = (int32_t)i;
}

size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }
}  // namespace

extern "C" {

int vcp_cluster_shapes_dev(vcp_ctx* ctx, const double* d_xy, const int32_t* d_labels, const int64_t* d_order, int64_t m,
                           int64_t n, int32_t K, double* d_centers, double* d_radius, uint8_t* d_valid, int32_t* d_hull_n,
                           double* d_rect_xy, double* d_rect_len, int32_t* d_rect_edge, uint8_t* d_rect_valid,
                           int32_t* d_hull_off, int32_t* d_hull_idx) {
  if (!ctx) return VCP_ERR_ARG;
  if (m < 0 || n < 0 || K < 0 || (m > 0 && (!d_xy || !d_labels))) return vcp_fail(ctx, VCP_ERR_ARG, "bad argument");
  if (K == 0) return VCP_OK;
  if (!d_centers || !d_radius || !d_valid) return vcp_fail(ctx, VCP_ERR_ARG, "null output");
  if ((d_hull_off == nullptr) != (d_hull_idx == nullptr)) return vcp_fail(ctx, VCP_ERR_ARG, "hull_off without hull_idx");
  if (n >= 0x7FFFFFF0LL || m >= 0x7FFFFFF0LL) return vcp_fail(ctx, VCP_ERR_TOO_LARGE, "n beyond 32-bit indexing");
  VCP_TRY(vcp_bind(ctx));
  vcp_phase_reset(ctx);
  hipStream_t st = ctx->stream;
  const size_t mm = (size_t)(m > 0 ? m : 1), kk = (size_t)K;
  const bool shapes = d_rect_xy || d_rect_len || d_rect_edge || d_rect_valid || d_hull_idx;
  VCP_TRY(vcp_ensure(ctx, ctx->b_aux0, (kk + 4) * 4 * 2 + 64));
  VCP_TRY(vcp_ensure(ctx, ctx->b_aux4, mm * 16));
  VCP_TRY(vcp_ensure(ctx, ctx->b_aux5, mm));
  if (d_hull_idx) VCP_TRY(vcp_ensure(ctx, ctx->b_sh_hull, mm * 4));
  if (!d_hull_n && shapes) {  // the hull export and the error check read it
    VCP_TRY(vcp_ensure(ctx, ctx->b_sh_flag, kk * 4));
    d_hull_n = ctx->b_sh_flag.as<int32_t>();
  }
  vcp_phase(ctx, "shapes_group");
  uint32_t* counts = ctx->b_aux0.as<uint32_t>();  // [K+2], label 0 included
  uint32_t* segstart = counts + (K + 4);
  uint32_t* bad = segstart + (K + 4);
  VCP_HIP(ctx, hipMemsetAsync(counts, 0, (kk + 4) * 4 * 2 + 64, st));
  const uint32_t* sorted = nullptr;
  VCP_TRY(vcp_group_by_label(ctx, d_labels, d_order, m, K, ctx->b_aux1, ctx->b_aux2, ctx->b_aux3, segstart, counts, bad,
                             &sorted));
  if (m > 0)
    VCP_LAUNCH(ctx, k_mcc_gather, dim3(vcp_blocks(m, MT)), dim3(MT), 0, st, d_xy, sorted, m, ctx->b_aux4.as<double>());
  vcp_phase(ctx, "shapes_fit");
  if (shapes) {
    const ShapeOut so{sorted, d_hull_idx ? ctx->b_sh_hull.as<uint32_t>() : nullptr, d_rect_xy, d_rect_len, d_rect_edge,
                      d_rect_valid};
    VCP_LAUNCH(ctx, k_shapes, dim3(K), dim3(MT), 0, st, ctx->b_aux4.as<double>(), segstart, counts,
               ctx->b_aux5.as<uint8_t>(), d_centers, d_radius, d_valid, d_hull_n, so);
  } else {
    VCP_LAUNCH(ctx, k_mcc, dim3(K), dim3(MT), 0, st, ctx->b_aux4.as<double>(), segstart, counts,
               ctx->b_aux5.as<uint8_t>(), d_centers, d_radius, d_valid, d_hull_n);
  }
  if (d_hull_idx) {
    vcp_phase(ctx, "shapes_hull");
    // a cluster that is skipped or in error has hull_n 0 (an overflowing hull: HMAX, and the call fails below)
    VCP_TRY(vcp_exclusive_scan_u32(ctx, reinterpret_cast<const uint32_t*>(d_hull_n), reinterpret_cast<uint32_t*>(d_hull_off),
                                   K, reinterpret_cast<uint32_t*>(d_hull_off) + K));
    VCP_LAUNCH(ctx, k_hull_export, dim3(K), dim3(64), 0, st, ctx->b_sh_hull.as<uint32_t>(), segstart, d_hull_n, d_valid,
               d_hull_off, d_hull_idx);
  }
  VCP_TRY(vcp_phase_finish(ctx));
  uint32_t* hp = reinterpret_cast<uint32_t*>(ctx->pinned);
  std::vector<uint8_t> hv(kk);
  VCP_HIP(ctx, hipMemcpyAsync(hp, bad, 4, hipMemcpyDeviceToHost, st));
  VCP_HIP(ctx, hipMemcpyAsync(hv.data(), d_valid, kk, hipMemcpyDeviceToHost, st));
  VCP_HIP(ctx, hipStreamSynchronize(st));
  if (hp[0] != 0) return vcp_fail(ctx, VCP_ERR_INDEX, "%u labels outside 0..K (clusList[clusterId-1])", hp[0]);
  for (int32_t k = 0; k < K; k++) {
    if (hv[k] == 2) return vcp_fail(ctx, VCP_ERR_TOO_LARGE, "cluster %d: convex hull beyond %d points", k + 1, HMAX);
    if (hv[k] == 3) return vcp_fail(ctx, VCP_ERR_EMPTY, "cluster %d: no finite point", k + 1);
  }
  return VCP_OK;
}

int vcp_cluster_shapes(vcp_ctx* ctx, const double* xy, const int32_t* labels, const int64_t* order, int64_t m, int64_t n,
                       int32_t K, double* centers, double* radius, uint8_t* valid, int32_t* hull_n, double* rect_xy,
                       double* rect_len, int32_t* rect_edge, uint8_t* rect_valid, int32_t* hull_off, int32_t* hull_idx) {
  if (!ctx) return VCP_ERR_ARG;
  if (m < 0 || n < 0 || K < 0 || (m > 0 && (!xy || !labels))) return vcp_fail(ctx, VCP_ERR_ARG, "bad argument");
  if (K == 0) return VCP_OK;
  if (!centers || !radius || !valid) return vcp_fail(ctx, VCP_ERR_ARG, "null output");
  if ((hull_off == nullptr) != (hull_idx == nullptr)) return vcp_fail(ctx, VCP_ERR_ARG, "hull_off without hull_idx");
  if (n >= 0x7FFFFFF0LL || m >= 0x7FFFFFF0LL) return vcp_fail(ctx, VCP_ERR_TOO_LARGE, "n beyond 32-bit indexing");
  VCP_TRY(vcp_bind(ctx));
  hipStream_t st = ctx->stream;
  const size_t nn = (size_t)(n > 0 ? n : 1), mm = (size_t)(m > 0 ? m : 1), kk = (size_t)K;
  VCP_TRY(vcp_ensure(ctx, ctx->b_in0, nn * 16));
  VCP_TRY(vcp_ensure(ctx, ctx->b_in3, nn * 4));
  VCP_TRY(vcp_ensure(ctx, ctx->b_in2, mm * 8));
  VCP_TRY(vcp_ensure(ctx, ctx->b_out0, kk * 16));
  VCP_TRY(vcp_ensure(ctx, ctx->b_out1, kk));
  VCP_TRY(vcp_ensure(ctx, ctx->b_out2, kk * 8));
  VCP_TRY(vcp_ensure(ctx, ctx->b_out3, kk * 4));
  // rectangle and hull outputs: one buffer, every part on a 16-byte boundary
  const size_t o_xy = 0, o_len = o_xy + kk * 64, o_edge = o_len + kk * 16, o_rv = o_edge + up16(kk * 4),
               o_off = o_rv + up16(kk), o_idx = o_off + up16((kk + 1) * 4), o_end = o_idx + mm * 4;
  VCP_TRY(vcp_ensure(ctx, ctx->b_sh_out, o_end));
  char* so = ctx->b_sh_out.as<char>();
  if (m > 0) {
    VCP_HIP(ctx, hipMemcpyAsync(ctx->b_in0.p, xy, (size_t)n * 16, hipMemcpyHostToDevice, st));
    VCP_HIP(ctx, hipMemcpyAsync(ctx->b_in3.p, labels, (size_t)n * 4, hipMemcpyHostToDevice, st));
    if (order) VCP_HIP(ctx, hipMemcpyAsync(ctx->b_in2.p, order, (size_t)m * 8, hipMemcpyHostToDevice, st));
  }
  const int rc = vcp_cluster_shapes_dev(
      ctx, ctx->b_in0.as<double>(), ctx->b_in3.as<int32_t>(), order ? ctx->b_in2.as<int64_t>() : nullptr, m, n, K,
      ctx->b_out0.as<double>(), ctx->b_out2.as<double>(), ctx->b_out1.as<uint8_t>(), ctx->b_out3.as<int32_t>(),
      rect_xy ? reinterpret_cast<double*>(so + o_xy) : nullptr, rect_len ? reinterpret_cast<double*>(so + o_len) : nullptr,
      rect_edge ? reinterpret_cast<int32_t*>(so + o_edge) : nullptr, rect_valid ? reinterpret_cast<uint8_t*>(so + o_rv) : nullptr,
      hull_idx ? reinterpret_cast<int32_t*>(so + o_off) : nullptr, hull_idx ? reinterpret_cast<int32_t*>(so + o_idx) : nullptr);
  // like vcp_mcc, the circle outputs come back whatever the status (valid tells which cluster failed)
  VCP_HIP(ctx, hipMemcpyAsync(centers, ctx->b_out0.p, kk * 16, hipMemcpyDeviceToHost, st));
  VCP_HIP(ctx, hipMemcpyAsync(radius, ctx->b_out2.p, kk * 8, hipMemcpyDeviceToHost, st));
  VCP_HIP(ctx, hipMemcpyAsync(valid, ctx->b_out1.p, kk, hipMemcpyDeviceToHost, st));
  if (hull_n) VCP_HIP(ctx, hipMemcpyAsync(hull_n, ctx->b_out3.p, kk * 4, hipMemcpyDeviceToHost, st));
  if (rc == VCP_OK) {
    if (rect_xy) VCP_HIP(ctx, hipMemcpyAsync(rect_xy, so + o_xy, kk * 64, hipMemcpyDeviceToHost, st));
    if (rect_len) VCP_HIP(ctx, hipMemcpyAsync(rect_len, so + o_len, kk * 16, hipMemcpyDeviceToHost, st));
    if (rect_edge) VCP_HIP(ctx, hipMemcpyAsync(rect_edge, so + o_edge, kk * 4, hipMemcpyDeviceToHost, st));
    if (rect_valid) VCP_HIP(ctx, hipMemcpyAsync(rect_valid, so + o_rv, kk, hipMemcpyDeviceToHost, st));
    if (hull_idx) {
      VCP_HIP(ctx, hipMemcpyAsync(hull_off, so + o_off, (kk + 1) * 4, hipMemcpyDeviceToHost, st));
      VCP_HIP(ctx, hipStreamSynchronize(st));
      if (hull_off[K] > 0)
        VCP_HIP(ctx, hipMemcpyAsync(hull_idx, so + o_idx, (size_t)hull_off[K] * 4, hipMemcpyDeviceToHost, st));
    }
  }
  VCP_HIP(ctx, hipStreamSynchronize(st));
  return rc;
}

int vcp_cluster_filter_dev(vcp_ctx* ctx, const int32_t* d_labels, int64_t n, int32_t K, const double* d_radius,
                           const uint8_t* d_valid, const double* d_rect_len, const uint8_t* d_rect_valid,
                           double max_radius, double max_aspect, uint8_t* d_filtered, uint8_t* d_keep,
                           int32_t* d_kept_idx, int32_t* n_filtered, int64_t* n_kept) {
  if (!ctx) return VCP_ERR_ARG;
  if (n < 0 || K < 0 || (n > 0 && !d_labels) || (K > 0 && (!d_radius || !d_valid || !d_filtered)))
    return vcp_fail(ctx, VCP_ERR_ARG, "bad argument");
  if (n >= 0x7FFFFFF0LL) return vcp_fail(ctx, VCP_ERR_TOO_LARGE, "n beyond 32-bit indexing");
  VCP_TRY(vcp_bind(ctx));
  vcp_phase_reset(ctx);
  hipStream_t st = ctx->stream;
  // [0, 16) bytes: the counters (filtered clusters, kept points, labels outside 0..K); then the flags [n + 1]
  VCP_TRY(vcp_ensure(ctx, ctx->b_sh_flag, 16 + (d_kept_idx ? ((size_t)n + 1) * 4 : 0)));
  uint32_t* counters = ctx->b_sh_flag.as<uint32_t>();
  uint32_t* flag = d_kept_idx ? counters + 4 : nullptr;
  vcp_phase(ctx, "filter");
  VCP_HIP(ctx, hipMemsetAsync(counters, 0, 16, st));
  if (K > 0)
    VCP_LAUNCH(ctx, k_filter_clusters, dim3(vcp_blocks(K, FT)), dim3(FT), 0, st, d_radius, d_valid, d_rect_len, d_rect_valid,
               K, max_radius, max_aspect, d_filtered, counters);
  if (n > 0) {
    VCP_LAUNCH(ctx, k_filter_points, dim3(vcp_blocks(n, FT)), dim3(FT), 0, st, d_labels, n, K, d_filtered, d_keep, flag,
               counters);
    if (d_kept_idx) {
      VCP_TRY(vcp_exclusive_scan_u32(ctx, flag, flag, n, flag + n));
      VCP_LAUNCH(ctx, k_filter_compact, dim3(vcp_blocks(n, FT)), dim3(FT), 0, st, flag, n, d_kept_idx);
    }
  }
  VCP_TRY(vcp_phase_finish(ctx));
  uint32_t* hp = reinterpret_cast<uint32_t*>(ctx->pinned);
  VCP_HIP(ctx, hipMemcpyAsync(hp, counters, 16, hipMemcpyDeviceToHost, st));
  VCP_HIP(ctx, hipStreamSynchronize(st));
  if (hp[2] != 0) return vcp_fail(ctx, VCP_ERR_INDEX, "%u labels outside 0..K (clusList[clusterId-1])", hp[2]);
  if (n_filtered) *n_filtered = (int32_t)hp[0];
  if (n_kept) *n_kept = (int64_t)hp[1];
  return VCP_OK;
}

int vcp_cluster_filter(vcp_ctx* ctx, const int32_t* labels, int64_t n, int32_t K, const double* radius,
                       const uint8_t* valid, const double* rect_len, const uint8_t* rect_valid, double max_radius,
                       double max_aspect, uint8_t* filtered, uint8_t* keep, int32_t* kept_idx, int32_t* n_filtered,
                       int64_t* n_kept) {
  if (!ctx) return VCP_ERR_ARG;
  if (n < 0 || K < 0 || (n > 0 && !labels) || (K > 0 && (!radius || !valid || !filtered)))
    return vcp_fail(ctx, VCP_ERR_ARG, "bad argument");
  if (n >= 0x7FFFFFF0LL) return vcp_fail(ctx, VCP_ERR_TOO_LARGE, "n beyond 32-bit indexing");
  VCP_TRY(vcp_bind(ctx));
  hipStream_t st = ctx->stream;
  const size_t nn = (size_t)(n > 0 ? n : 1), kk = (size_t)(K > 0 ? K : 1);
  const bool rect = rect_len && rect_valid;
  VCP_TRY(vcp_ensure(ctx, ctx->b_in3, nn * 4));
  const size_t i_rad = 0, i_len = i_rad + kk * 8, i_val = i_len + kk * 16, i_rv = i_val + up16(kk), i_end = i_rv + up16(kk);
  VCP_TRY(vcp_ensure(ctx, ctx->b_in0, i_end));
  VCP_TRY(vcp_ensure(ctx, ctx->b_out1, kk));
  VCP_TRY(vcp_ensure(ctx, ctx->b_out0, nn));
  VCP_TRY(vcp_ensure(ctx, ctx->b_sh_out, nn * 4));
  char* in = ctx->b_in0.as<char>();
  if (n > 0) VCP_HIP(ctx, hipMemcpyAsync(ctx->b_in3.p, labels, (size_t)n * 4, hipMemcpyHostToDevice, st));
  if (K > 0) {
    VCP_HIP(ctx, hipMemcpyAsync(in + i_rad, radius, (size_t)K * 8, hipMemcpyHostToDevice, st));
    VCP_HIP(ctx, hipMemcpyAsync(in + i_val, valid, (size_t)K, hipMemcpyHostToDevice, st));
    if (rect) {
      VCP_HIP(ctx, hipMemcpyAsync(in + i_len, rect_len, (size_t)K * 16, hipMemcpyHostToDevice, st));
      VCP_HIP(ctx, hipMemcpyAsync(in + i_rv, rect_valid, (size_t)K, hipMemcpyHostToDevice, st));
    }
  }
  int64_t nk = 0;
  VCP_TRY(vcp_cluster_filter_dev(ctx, ctx->b_in3.as<int32_t>(), n, K, reinterpret_cast<const double*>(in + i_rad),
                                 reinterpret_cast<const uint8_t*>(in + i_val),
                                 rect ? reinterpret_cast<const double*>(in + i_len) : nullptr,
                                 rect ? reinterpret_cast<const uint8_t*>(in + i_rv) : nullptr, max_radius, max_aspect,
                                 ctx->b_out1.as<uint8_t>(), keep ? ctx->b_out0.as<uint8_t>() : nullptr,
                                 kept_idx ? ctx->b_sh_out.as<int32_t>() : nullptr, n_filtered, &nk));
  if (n_kept) *n_kept = nk;
  if (K > 0) VCP_HIP(ctx, hipMemcpyAsync(filtered, ctx->b_out1.p, (size_t)K, hipMemcpyDeviceToHost, st));
  if (keep && n > 0) VCP_HIP(ctx, hipMemcpyAsync(keep, ctx->b_out0.p, (size_t)n, hipMemcpyDeviceToHost, st));
  if (kept_idx && nk > 0) VCP_HIP(ctx, hipMemcpyAsync(kept_idx, ctx->b_sh_out.p, (size_t)nk * 4, hipMemcpyDeviceToHost, st));
  VCP_HIP(ctx, hipStreamSynchronize(st));
  return VCP_OK;
}

}  // extern "C"
