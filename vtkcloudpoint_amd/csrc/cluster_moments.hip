// cluster_moments.hip -- second central moments per cluster: vcp_cluster_moments (include/vcp.h).
//
// The reference rejects clusters by the circumscribed circle and rectangle (vcp_cluster_shapes): extreme values, which
// one stray return moves by its full distance, and which exist for the (X, Y) view only.  Here every cluster gets its
// mean, its population covariance, the principal axes and eigenvalues of that (symeig.hpp) and four numbers derived
// from them; weights are the `count` of a deduplicated import.
//
// The rows are put in (label, index) order by vcp_group_by_label and every sum runs through the fixed tree of
// centroids.hip: chunks of CH consecutive members -> one workgroup each (thread-strided partial sums from +0.0, the wave
// shuffle tree, 4 waves in order), then the chunk partials of a cluster in chunk order from 0.0, then ONE division.  Two
// passes, centred on purpose: the second pass sums fl(fl(w d_a) d_b) with d = fl(x - mean), so a cloud far from the
// origin keeps its digits (a raw-moment covariance loses all of them).  Every cluster takes the
// same road whatever its size -- chunk partials, then one thread per cluster -- so there is no second road whose bits
// could differ.  Algorithmic bytes per point: 4 (label) + 4 (index) + 2 * 8 * dim (the coordinates, gathered once per
// pass), + 2 * 4 with weights.
#include <cmath>
#include <cstring>

#include "reduce.hpp"
#include "sort.hpp"
#include "symeig.hpp"
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

// pass 2, one workgroup per chunk: pcov[c * NP + ab] = the chunk's sum of fl(fl(w d_a) d_b), a <= b, d = fl(x - mean)
template <int D>
__global__ __launch_bounds__(CT) void k_cm_chunk_cov(CmSeg a, const double* __restrict__ wmean, double* __restrict__ pcov) {
  constexpr int NP = D * (D + 1) / 2;
  const uint32_t c = blockIdx.x;
  uint32_t beg, end;
  const int k = cm_chunk(a, c, beg, end);
  double m[D], s[NP];
#pragma unroll
  for (int j = 0; j < D; j++) m[j] = wmean[(size_t)(k - 1) * D + j];
#pragma unroll
  for (int j = 0; j < NP; j++) s[j] = 0.0;
  for (uint32_t t = beg + threadIdx.x; t < end; t += CT) {
    const uint32_t i = a.sorted[t];
    const double w = a.weights ? (double)a.weights[i] : 1.0;
    const double* p = a.pts + (int64_t)i * a.ld;
    double d[D];
#pragma unroll
    for (int j = 0; j < D; j++) d[j] = p[j] - m[j];
    int ab = 0;
#pragma unroll
    for (int r = 0; r < D; r++) {
      const double wd = w * d[r];
#pragma unroll
      for (int q = r; q < D; q++, ab++) s[ab] += wd * d[q];
    }
  }
  block_fold<CT>(s, FoldSum(), pcov + (size_t)c * NP);
}

struct CmOut {
  double *mean, *cov, *eval, *evec, *shape;
  uint8_t* valid;
  int64_t* counts;
};

// per cluster: the covariance, its eigen-solve, the derived numbers; every output that is not NULL
template <int D>
__global__ __launch_bounds__(FT) void k_cm_final(const double* __restrict__ pcov, const uint32_t* __restrict__ chunkstart,
                                                 int32_t K, const double* __restrict__ wmean,
                                                 const unsigned long long* __restrict__ wtot, CmOut o) {
  constexpr int NP = D * (D + 1) / 2;
  const int k = blockIdx.x * FT + threadIdx.x + 1;
  if (k > K) return;
  double s[NP];
#pragma unroll
  for (int j = 0; j < NP; j++) s[j] = 0.0;
  for (uint32_t c = chunkstart[k]; c < chunkstart[k + 1]; c++)
#pragma unroll
    for (int j = 0; j < NP; j++) s[j] += pcov[(size_t)c * NP + j];
  const unsigned long long W = wtot[k - 1];
  const double Wd = (double)W;
  bool fin = true;
  double cov[NP], m[D], eval[D], evec[D * D], shape[4];
#pragma unroll
  for (int j = 0; j < NP; j++) {
    cov[j] = s[j] / Wd;
    fin = fin && cm_finite(cov[j]);
  }
#pragma unroll
  for (int j = 0; j < D; j++) {
    m[j] = wmean[(size_t)(k - 1) * D + j];
    fin = fin && cm_finite(m[j]);
  }
  (void)sym_eig<D>(cov, eval, evec);
  sym_eig_shape<D>(eval, evec, shape);
  const size_t z = (size_t)(k - 1);
  if (o.mean)
#pragma unroll
    for (int j = 0; j < D; j++) o.mean[z * D + j] = cm_canon(m[j]);
  if (o.cov)
#pragma unroll
    for (int j = 0; j < NP; j++) o.cov[z * NP + j] = cm_canon(cov[j]);
  if (o.eval)
#pragma unroll
    for (int j = 0; j < D; j++) o.eval[z * D + j] = eval[j];
  if (o.evec)
#pragma unroll
    for (int j = 0; j < D * D; j++) o.evec[z * D * D + j] = evec[j];
  if (o.shape)
#pragma unroll
    for (int j = 0; j < 4; j++) o.shape[z * 4 + j] = shape[j];
  if (o.valid) o.valid[z] = (W >= 2 && fin) ? 1 : 0;
  if (o.counts) o.counts[z] = (int64_t)W;
}

int cm_check(vcp_ctx* ctx, const void* pts, int64_t ld, int dim, const void* labels, int64_t n, int32_t K) {
  if (n < 0 || K < 0) return vcp_fail(ctx, VCP_ERR_ARG, "n < 0 or K < 0");
  if (dim != 2 && dim != 3) return vcp_fail(ctx, VCP_ERR_ARG, "dim %d is neither 2 nor 3", dim);
  if (ld < dim) return vcp_fail(ctx, VCP_ERR_ARG, "ld %lld below dim %d", (long long)ld, dim);
  if (n > 0 && (!pts || !labels)) return vcp_fail(ctx, VCP_ERR_ARG, "null pts or labels");
  if (n >= 0x7FFFFFF0LL) return vcp_fail(ctx, VCP_ERR_TOO_LARGE, "n beyond 32-bit indexing");
  return VCP_OK;
}

template <int D>
int cm_run(vcp_ctx* ctx, const CmSeg& a, uint32_t nchunks, double* psum, unsigned long long* pw, double* pcov,
           double* wmean, unsigned long long* wtot, const CmOut& o) {
  hipStream_t st = ctx->stream;
  vcp_phase(ctx, "moments_mean");
  if (nchunks > 0) VCP_LAUNCH(ctx, k_cm_chunk_mean<D>, dim3(nchunks), dim3(CT), 0, st, a, psum, pw);
  VCP_LAUNCH(ctx, k_cm_mean<D>, dim3(vcp_blocks(a.K, FT)), dim3(FT), 0, st, psum, pw, a.chunkstart, a.K, wmean, wtot);
  vcp_phase(ctx, "moments_cov");
  if (nchunks > 0) VCP_LAUNCH(ctx, k_cm_chunk_cov<D>, dim3(nchunks), dim3(CT), 0, st, a, wmean, pcov);
  VCP_LAUNCH(ctx, k_cm_final<D>, dim3(vcp_blocks(a.K, FT)), dim3(FT), 0, st, pcov, a.chunkstart, a.K, wmean, wtot, o);
  return VCP_OK;
}

// doubles of the caller's array that n rows of dim at ld span
size_t cm_span(int64_t n, int64_t ld, int dim) { return n > 0 ? (size_t)(n - 1) * (size_t)ld + (size_t)dim : 0; }
}  // namespace

extern "C" {

int vcp_cluster_moments_dev(vcp_ctx* ctx, const double* d_pts, int64_t ld, int dim, const int32_t* d_labels,
                            const int32_t* d_weights, int64_t n, int32_t K, double* d_mean, double* d_cov,
                            double* d_eval, double* d_evec, double* d_shape, uint8_t* d_valid, int64_t* d_counts) {
  if (!ctx) return VCP_ERR_ARG;
  VCP_TRY(cm_check(ctx, d_pts, ld, dim, d_labels, n, K));
  VCP_TRY(vcp_bind(ctx));
  vcp_phase_reset(ctx);
  hipStream_t st = ctx->stream;
  vcp_phase(ctx, "moments_group");
  // b_cm_misc: [counts | chunkstart | segstart] (kk words each) | 8 counter words (0 bad labels, 1 negative weights,
  // 4 chunks) | wtot [K] 64-bit | wmean [K * 3] doubles
  const size_t kk = ((size_t)K + 5) & ~(size_t)1;  // even: the 64-bit words behind the arrays stay aligned
  const size_t words = 3 * kk + 8;
  VCP_TRY(vcp_ensure(ctx, ctx->b_cm_misc, words * 4 + (size_t)K * 8 * 4));
  uint32_t* counts = ctx->b_cm_misc.as<uint32_t>();
  uint32_t* chunkstart = counts + kk;
  uint32_t* segstart = chunkstart + kk;
  uint32_t* ctr = segstart + kk;
  unsigned long long* wtot = reinterpret_cast<unsigned long long*>(counts + words);
  double* wmean = reinterpret_cast<double*>(wtot + K);
  VCP_HIP(ctx, hipMemsetAsync(counts, 0, words * 4, st));
  const uint32_t* sorted = nullptr;
  VCP_TRY(vcp_group_by_label(ctx, d_labels, nullptr, n, K, ctx->b_aux1, ctx->b_aux2, ctx->b_aux3, segstart, counts, ctr,
                             &sorted));
  if (d_weights && n > 0) {
    const unsigned walk = (unsigned)(ctx->prop.multiProcessorCount > 0 ? ctx->prop.multiProcessorCount : 256) * 8u;
    VCP_LAUNCH(ctx, k_cm_check_w, dim3(vcp_blocks(n, CT, (int)walk)), dim3(CT), 0, st, d_weights, n, ctr + 1);
  }
  VCP_LAUNCH(ctx, k_cm_nchunks, dim3(vcp_blocks((int64_t)K + 1, CT)), dim3(CT), 0, st, counts, K, chunkstart);
  VCP_TRY(vcp_exclusive_scan_u32(ctx, chunkstart, chunkstart, (int64_t)K + 2, ctr + 4));
  uint32_t* hp = reinterpret_cast<uint32_t*>(ctx->pinned);  // [0, 32) of the pinned scratch
  VCP_HIP(ctx, hipMemcpyAsync(hp, ctr, 8 * 4, hipMemcpyDeviceToHost, st));
  VCP_HIP(ctx, hipStreamSynchronize(st));
  if (hp[0] != 0) return vcp_fail(ctx, VCP_ERR_INDEX, "%u labels outside 0..K", hp[0]);
  if (hp[1] != 0) return vcp_fail(ctx, VCP_ERR_ARG, "%u negative weights", hp[1]);
  if (K == 0) return vcp_phase_finish(ctx);
  const uint32_t nchunks = hp[4];
  // b_aux4: psum [nchunks * 3] | pcov [nchunks * 6] | pw [nchunks]
  VCP_TRY(vcp_ensure(ctx, ctx->b_aux4, ((size_t)nchunks + 1) * 10 * 8));
  double* psum = ctx->b_aux4.as<double>();
  double* pcov = psum + (size_t)nchunks * 3;
  unsigned long long* pw = reinterpret_cast<unsigned long long*>(pcov + (size_t)nchunks * 6);
  const CmSeg a{sorted, segstart, counts, chunkstart, K, d_pts, ld, d_weights};
  const CmOut o{d_mean, d_cov, d_eval, d_evec, d_shape, d_valid, d_counts};
  if (dim == 2)
    VCP_TRY(cm_run<2>(ctx, a, nchunks, psum, pw, pcov, wmean, wtot, o));
  else
    VCP_TRY(cm_run<3>(ctx, a, nchunks, psum, pw, pcov, wmean, wtot, o));
  VCP_TRY(vcp_phase_finish(ctx));
  VCP_HIP(ctx, hipStreamSynchronize(st));
  return VCP_OK;
}

int vcp_cluster_moments(vcp_ctx* ctx, const double* pts, int64_t ld, int dim, const int32_t* labels,
                        const int32_t* weights, int64_t n, int32_t K, double* mean, double* cov, double* eval,
                        double* evec, double* shape, uint8_t* valid, int64_t* counts) {
  if (!ctx) return VCP_ERR_ARG;
  VCP_TRY(cm_check(ctx, pts, ld, dim, labels, n, K));
  VCP_TRY(vcp_bind(ctx));
  hipStream_t st = ctx->stream;
  // in: [pts span * 8 | labels n * 4 | weights n * 4]; out: the doubles [mean | cov | eval | evec | shape], counts, valid
  const size_t span = cm_span(n, ld, dim), k = (size_t)K, np = (size_t)dim * (dim + 1) / 2, d = (size_t)dim;
  VCP_TRY(vcp_ensure(ctx, ctx->b_cm_in, span * 8 + (size_t)n * 8));
  const size_t nd = k * (d + np + d + d * d + 4);
  VCP_TRY(vcp_ensure(ctx, ctx->b_cm_out, nd * 8 + k * 8 + k));
  char* din = ctx->b_cm_in.as<char>();
  const int32_t* dl = reinterpret_cast<const int32_t*>(din + span * 8);
  const int32_t* dw = weights ? dl + n : nullptr;
  if (n > 0) {
    VCP_HIP(ctx, hipMemcpyAsync(din, pts, span * 8, hipMemcpyHostToDevice, st));
    VCP_HIP(ctx, hipMemcpyAsync(din + span * 8, labels, (size_t)n * 4, hipMemcpyHostToDevice, st));
    if (weights) VCP_HIP(ctx, hipMemcpyAsync(din + span * 8 + (size_t)n * 4, weights, (size_t)n * 4, hipMemcpyHostToDevice, st));
  }
  double* o_mean = ctx->b_cm_out.as<double>();
  double* o_cov = o_mean + k * d;
  double* o_eval = o_cov + k * np;
  double* o_evec = o_eval + k * d;
  double* o_shape = o_evec + k * d * d;
  int64_t* o_counts = reinterpret_cast<int64_t*>(o_shape + k * 4);
  uint8_t* o_valid = reinterpret_cast<uint8_t*>(o_counts + k);
  VCP_TRY(vcp_cluster_moments_dev(ctx, reinterpret_cast<const double*>(din), ld, dim, dl, dw, n, K, mean ? o_mean : nullptr,
                                  cov ? o_cov : nullptr, eval ? o_eval : nullptr, evec ? o_evec : nullptr,
                                  shape ? o_shape : nullptr, valid ? o_valid : nullptr, counts ? o_counts : nullptr));
  if (K > 0) {
    if (mean) VCP_HIP(ctx, hipMemcpyAsync(mean, o_mean, k * d * 8, hipMemcpyDeviceToHost, st));
    if (cov) VCP_HIP(ctx, hipMemcpyAsync(cov, o_cov, k * np * 8, hipMemcpyDeviceToHost, st));
    if (eval) VCP_HIP(ctx, hipMemcpyAsync(eval, o_eval, k * d * 8, hipMemcpyDeviceToHost, st));
    if (evec) VCP_HIP(ctx, hipMemcpyAsync(evec, o_evec, k * d * d * 8, hipMemcpyDeviceToHost, st));
    if (shape) VCP_HIP(ctx, hipMemcpyAsync(shape, o_shape, k * 4 * 8, hipMemcpyDeviceToHost, st));
    if (counts) VCP_HIP(ctx, hipMemcpyAsync(counts, o_counts, k * 8, hipMemcpyDeviceToHost, st));
    if (valid) VCP_HIP(ctx, hipMemcpyAsync(valid, o_valid, k, hipMemcpyDeviceToHost, st));
    VCP_HIP(ctx, hipStreamSynchronize(st));
  }
  return VCP_OK;
}

int vcp_selftest_sym_eig(int dim, const double* s_packed, double* eval, double* evec, int* sweeps) {
  if (!s_packed || !eval || !evec || (dim != 2 && dim != 3)) return VCP_ERR_ARG;
  const int n = dim == 2 ? sym_eig<2>(s_packed, eval, evec) : sym_eig<3>(s_packed, eval, evec);
  if (sweeps) *sweeps = n;
  return 1;
}

}  // extern "C"
