// cluster_seg.hpp -- what the per-cluster sums of vcp_cluster_moments (cluster_moments.hip) and vcp_cluster_spheres
// (cluster_spheres.hip) share: the rows in (label, index) order cut into chunks of CH members, the argument and weight
// check, and pass 1 (total weight and mean).  Both entry points state that their W and mean are the same bits; they are,
// because both compile this source.  Internal linkage, like symeig.hpp.
//
// Every sum runs through the fixed tree of centroids.hip: chunks of CH consecutive members -> one workgroup each
// (thread-strided partial sums from +0.0, the wave shuffle tree, 4 waves in order), then the chunk partials of a cluster in
// chunk order from 0.0.  Every cluster takes the same road whatever its size -- chunk partials, then one thread per
// cluster -- so there is no second road whose bits could differ.
#pragma once
#include <cmath>
#include <cstring>

#include "reduce.hpp"
#include "sort.hpp"
#include "vcp_ctx.hpp"

namespace {
constexpr int CT = 256;
constexpr int CH = 16384;  // members per chunk: vcp_centroids' tree
constexpr int FT = 64;     // threads per workgroup of the per-cluster kernels (one cluster per thread)

__device__ __forceinline__ double cm_nan() { return __longlong_as_double(0x7FF8000000000000LL); }
__device__ __forceinline__ double cm_canon(double v) { return v != v ? cm_nan() : v; }
__device__ __forceinline__ bool cm_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }  // false for NaN

// rows whose weight is negative
__global__ __launch_bounds__(CT) void k_cm_check_w(const int32_t* __restrict__ weights, int64_t n,
                                                   uint32_t* __restrict__ bad) {
  uint32_t c = 0;
  for (int64_t i = (int64_t)blockIdx.x * CT + threadIdx.x; i < n; i += (int64_t)gridDim.x * CT) c += weights[i] < 0 ? 1u : 0u;
  if (c) atomicAdd(bad, c);
}

// nch[k] = chunks of cluster k (k = 0: the rows in no cluster, 0 chunks)
__global__ __launch_bounds__(CT) void k_cm_nchunks(const uint32_t* __restrict__ counts, int32_t K,
                                                   uint32_t* __restrict__ nch) {
  const int k = blockIdx.x * CT + threadIdx.x;
  if (k > K) return;
  nch[k] = k == 0 ? 0u : (counts[k] + CH - 1) / CH;
}

struct CmSeg {
  const uint32_t* sorted;      // the rows in (label, index) order
  const uint32_t* segstart;    // [K + 2]
  const uint32_t* counts;      // [K + 1] members (rows, not weight)
  const uint32_t* chunkstart;  // [K + 2]: first chunk of cluster k
  int32_t K;
  const double* pts;
  int64_t ld;
  const int32_t* weights;      // or NULL
};

// chunk c -> its cluster k and its slots [beg, end) of `sorted`
__device__ __forceinline__ int cm_chunk(const CmSeg& a, uint32_t c, uint32_t& beg, uint32_t& end) {
  int lo = 1, hi = a.K;  // the largest k in [1, K] with chunkstart[k] <= c
  while (lo < hi) {
    const int mid = (int)(((int64_t)lo + hi + 1) >> 1);
    if (a.chunkstart[mid] <= c) lo = mid; else hi = mid - 1;
  }
  const uint32_t within = (c - a.chunkstart[lo]) * (uint32_t)CH, cnt = a.counts[lo];
  beg = a.segstart[lo] + within;
  end = a.segstart[lo] + (within + CH < cnt ? within + CH : cnt);
  return lo;
}

// pass 1, one workgroup per chunk: psum[c * D + a] = the chunk's sum of fl(w x_a), pw[c] = its sum of w (integers: exact
// in any order)
template <int D>
__global__ __launch_bounds__(CT) void k_cm_chunk_mean(CmSeg a, double* __restrict__ psum,
                                                      unsigned long long* __restrict__ pw) {
  __shared__ unsigned long long sw[CT / 64];
  const uint32_t c = blockIdx.x;
  uint32_t beg, end;
  (void)cm_chunk(a, c, beg, end);
  double s[D];
#pragma unroll
  for (int j = 0; j < D; j++) s[j] = 0.0;
  unsigned long long wsum = 0;
  for (uint32_t t = beg + threadIdx.x; t < end; t += CT) {
    const uint32_t i = a.sorted[t];
    const int32_t wi = a.weights ? a.weights[i] : 1;
    const double w = (double)wi;
    const double* p = a.pts + (int64_t)i * a.ld;
#pragma unroll
    for (int j = 0; j < D; j++) s[j] += w * p[j];
    wsum += (unsigned long long)wi;
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) wsum += __shfl_down(wsum, d, 64);
  if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = wsum;
  block_fold<CT>(s, FoldSum(), psum + (size_t)c * D);  // its barrier also publishes sw
  if (threadIdx.x == 0) {
    unsigned long long r = sw[0];
#pragma unroll
    for (int j = 1; j < CT / 64; j++) r += sw[j];
    pw[c] = r;
  }
}

// per cluster: W and the mean
template <int D>
__global__ __launch_bounds__(FT) void k_cm_mean(const double* __restrict__ psum, const unsigned long long* __restrict__ pw,
                                                const uint32_t* __restrict__ chunkstart, int32_t K,
                                                double* __restrict__ wmean, unsigned long long* __restrict__ wtot) {
  const int k = blockIdx.x * FT + threadIdx.x + 1;
  if (k > K) return;
  double s[D];
#pragma unroll
  for (int j = 0; j < D; j++) s[j] = 0.0;
  unsigned long long W = 0;
  for (uint32_t c = chunkstart[k]; c < chunkstart[k + 1]; c++) {
#pragma unroll
    for (int j = 0; j < D; j++) s[j] += psum[(size_t)c * D + j];
    W += pw[c];
  }
  const double Wd = (double)W;
#pragma unroll
  for (int j = 0; j < D; j++) wmean[(size_t)(k - 1) * D + j] = s[j] / Wd;  // W == 0: 0 / 0 = NaN
  wtot[k - 1] = W;
}

int cm_check(vcp_ctx* ctx, const void* pts, int64_t ld, int dim, const void* labels, int64_t n, int32_t K) {
  if (n < 0 || K < 0) return vcp_fail(ctx, VCP_ERR_ARG, "n < 0 or K < 0");
  if (dim != 2 && dim != 3) return vcp_fail(ctx, VCP_ERR_ARG, "dim %d is neither 2 nor 3", dim);
  if (ld < dim) return vcp_fail(ctx, VCP_ERR_ARG, "ld %lld below dim %d", (long long)ld, dim);
  if (n > 0 && (!pts || !labels)) return vcp_fail(ctx, VCP_ERR_ARG, "null pts or labels");
  if (n >= 0x7FFFFFF0LL) return vcp_fail(ctx, VCP_ERR_TOO_LARGE, "n beyond 32-bit indexing");
  return VCP_OK;
}

// doubles of the caller's array that n rows of dim at ld span
size_t cm_span(int64_t n, int64_t ld, int dim) { return n > 0 ? (size_t)(n - 1) * (size_t)ld + (size_t)dim : 0; }

// The tables of one call, in `misc`: [counts | chunkstart | segstart] (kk words each) | 8 counter words (0 bad labels,
// 1 negative weights, 4 chunks) | wtot [K] 64-bit | wmean [K * 3] doubles | `extra` doubles of the caller's
struct CmTables {
  uint32_t *counts, *chunkstart, *segstart;
  const uint32_t* sorted;
  unsigned long long* wtot;
  double *wmean, *extra;
  uint32_t nchunks;
};

// Groups the rows by label, checks labels and weights, counts the chunks: everything up to the call's one synchronisation.
// The label and weight errors are returned from here, before any output is touched.
int cm_group(vcp_ctx* ctx, DevBuf& misc, size_t extra_doubles, const int32_t* d_labels, const int32_t* d_weights, int64_t n,
             int32_t K, CmTables& t) {
  hipStream_t st = ctx->stream;
  const size_t kk = ((size_t)K + 5) & ~(size_t)1;  // even: the 64-bit words behind the arrays stay aligned
  const size_t words = 3 * kk + 8;
  VCP_TRY(vcp_ensure(ctx, misc, words * 4 + (size_t)K * 8 * 4 + extra_doubles * 8));
  t.counts = misc.as<uint32_t>();
  t.chunkstart = t.counts + kk;
  t.segstart = t.chunkstart + kk;
  uint32_t* ctr = t.segstart + kk;
  t.wtot = reinterpret_cast<unsigned long long*>(t.counts + words);
  t.wmean = reinterpret_cast<double*>(t.wtot + K);
  t.extra = t.wmean + (size_t)K * 3;
  VCP_HIP(ctx, hipMemsetAsync(t.counts, 0, words * 4, st));
  t.sorted = nullptr;
  VCP_TRY(vcp_group_by_label(ctx, d_labels, nullptr, n, K, ctx->b_aux1, ctx->b_aux2, ctx->b_aux3, t.segstart, t.counts, ctr,
                             &t.sorted));
  if (d_weights && n > 0) {
    const unsigned walk = (unsigned)(ctx->prop.multiProcessorCount > 0 ? ctx->prop.multiProcessorCount : 256) * 8u;
    VCP_LAUNCH(ctx, k_cm_check_w, dim3(vcp_blocks(n, CT, (int)walk)), dim3(CT), 0, st, d_weights, n, ctr + 1);
  }
  VCP_LAUNCH(ctx, k_cm_nchunks, dim3(vcp_blocks((int64_t)K + 1, CT)), dim3(CT), 0, st, t.counts, K, t.chunkstart);
  VCP_TRY(vcp_exclusive_scan_u32(ctx, t.chunkstart, t.chunkstart, (int64_t)K + 2, ctr + 4));
  uint32_t* hp = reinterpret_cast<uint32_t*>(ctx->pinned);  // [0, 32) of the pinned scratch
  VCP_HIP(ctx, hipMemcpyAsync(hp, ctr, 8 * 4, hipMemcpyDeviceToHost, st));
  VCP_HIP(ctx, hipStreamSynchronize(st));
  if (hp[0] != 0) return vcp_fail(ctx, VCP_ERR_INDEX, "%u labels outside 0..K", hp[0]);
  if (hp[1] != 0) return vcp_fail(ctx, VCP_ERR_ARG, "%u negative weights", hp[1]);
  t.nchunks = hp[4];
  return VCP_OK;
}
}  // namespace
