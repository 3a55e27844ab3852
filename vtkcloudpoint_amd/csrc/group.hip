// group.hip -- list entries grouped by cluster label (sort.hpp: vcp_group_by_label), for the per-cluster passes of
// centroids.hip and mcc.hip.
#include "sort.hpp"

namespace {
constexpr int GT = 256;

__global__ __launch_bounds__(GT) void k_label_keys(const int32_t* __restrict__ labels, const int64_t* __restrict__ order,
                                                   int64_t m, int32_t K, uint32_t* __restrict__ keys,
                                                   uint32_t* __restrict__ vals, uint32_t* __restrict__ bad) {
  const int64_t t = (int64_t)blockIdx.x * GT + threadIdx.x;
  if (t >= m) return;
  const int64_t i = order ? order[t] : t;
  int32_t l = labels[i];
  if (l < 0 || l > K) {  // clusList[p.clusterId - 1] out of range (Tools.cs:185)
    atomicAdd(bad, 1u);
    l = 0;
  }
  keys[t] = (uint32_t)l;
  vals[t] = (uint32_t)i;
}

// Segment bounds from the SORTED labels, no per-point atomics (global atomics run at the memory side here: 5 M adds into
// 27 k counters cost more than the sort): mark[l] = (last slot of label l) + 1; the exclusive max-scan of the marks is
// the first slot of every label; counts are the differences.
__global__ __launch_bounds__(GT) void k_label_marks(const uint32_t* __restrict__ skey, int64_t m, uint32_t* __restrict__ mark) {
  const int64_t t = (int64_t)blockIdx.x * GT + threadIdx.x;
  if (t >= m) return;
  const uint32_t k = skey[t];
  if (t == m - 1 || skey[t + 1] != k) mark[k] = (uint32_t)t + 1u;
}

__global__ __launch_bounds__(GT) void k_label_counts(const uint32_t* __restrict__ segstart, int32_t K,
                                                     uint32_t* __restrict__ counts) {
  const int k = blockIdx.x * GT + threadIdx.x;
  if (k <= K) counts[k] = segstart[k + 1] - segstart[k];
}
}  // namespace

int vcp_group_by_label(vcp_ctx* ctx, const int32_t* d_labels, const int64_t* d_order, int64_t m, int32_t K,
                       DevBuf& keys, DevBuf& vals, DevBuf& tmp, uint32_t* segstart, uint32_t* counts, uint32_t* bad,
                       const uint32_t** sorted) {
  hipStream_t st = ctx->stream;
  VCP_TRY(vcp_ensure(ctx, keys, (size_t)(m + 1) * 4 * 2));
  VCP_TRY(vcp_ensure(ctx, vals, (size_t)(m + 1) * 4 * 2));
  uint32_t* keys_in = keys.as<uint32_t>();
  uint32_t* keys_out = keys_in + (m + 1);
  uint32_t* vals_in = vals.as<uint32_t>();
  uint32_t* vals_out = vals_in + (m + 1);
  if (m > 0) {
    VCP_LAUNCH(ctx, k_label_keys, dim3(vcp_blocks(m, GT)), dim3(GT), 0, st, d_labels, d_order, m, K, keys_in, vals_in,
                    bad);
    VCP_TRY(vcp_sort_pairs(ctx, tmp, keys_in, keys_out, vals_in, vals_out, (size_t)m, vcp_bits_for((uint64_t)K)));
    VCP_LAUNCH(ctx, k_label_marks, dim3(vcp_blocks(m, GT)), dim3(GT), 0, st, keys_out, m, segstart);
  }
  VCP_TRY(vcp_exclusive_max_scan_u32(ctx, segstart, segstart, (int64_t)K + 2, nullptr));  // segstart[K + 1] = m
  VCP_LAUNCH(ctx, k_label_counts, dim3(vcp_blocks((int64_t)K + 1, GT)), dim3(GT), 0, st, segstart, K, counts);
  *sorted = vals_out;
  return VCP_OK;
}
