// cluster_moments.hip -- second central moments per cluster: vcp_cluster_moments (include/vcp.h).
//
// The reference rejects clusters by the circumscribed circle and rectangle (vcp_cluster_shapes): extreme values, which
// one stray return moves by its full distance, and which exist for the (X, Y) view only.  Here every cluster gets its
// mean, its population covariance, the principal axes and eigenvalues of that (symeig.hpp) and four numbers derived
// from them; weights are the `count` of a deduplicated import.
//
// The rows are put in (label, index) order by vcp_group_by_label and every sum runs through the fixed tree of
// centroids.hip: chunks of CH consecutive members -> one workgroup each (thread-strided partial sums from +0.0, the wave
// shuffle tree, 4 waves in order), then the chunk partials of a cluster in chunk order from 0.0, then ONE division (the
// grouping and pass 1 are in cluster_seg.hpp, shared with cluster_spheres.hip).  Two
// passes, centred on purpose: the second pass sums fl(fl(w d_a) d_b) with d = fl(x - mean), so a cloud far from the
// origin keeps its digits (a raw-moment covariance loses all of them).  Every cluster takes the
// same road whatever its size -- chunk partials, then one thread per cluster -- so there is no second road whose bits
// could differ.  Algorithmic bytes per point: 4 (label) + 4 (index) + 2 * 8 * dim (the coordinates, gathered once per
// pass), + 2 * 4 with weights.
#include "cluster_seg.hpp"
#include "symeig.hpp"

namespace {
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
  CmTables t;  // in b_cm_misc (cluster_seg.hpp)
  VCP_TRY(cm_group(ctx, ctx->b_cm_misc, 0, d_labels, d_weights, n, K, t));
  if (K == 0) return vcp_phase_finish(ctx);
  const uint32_t nchunks = t.nchunks;
  // b_aux4: psum [nchunks * 3] | pcov [nchunks * 6] | pw [nchunks]
  VCP_TRY(vcp_ensure(ctx, ctx->b_aux4, ((size_t)nchunks + 1) * 10 * 8));
  double* psum = ctx->b_aux4.as<double>();
  double* pcov = psum + (size_t)nchunks * 3;
  unsigned long long* pw = reinterpret_cast<unsigned long long*>(pcov + (size_t)nchunks * 6);
  const CmSeg a{t.sorted, t.segstart, t.counts, t.chunkstart, K, d_pts, ld, d_weights};
  const CmOut o{d_mean, d_cov, d_eval, d_evec, d_shape, d_valid, d_counts};
  if (dim == 2)
    VCP_TRY(cm_run<2>(ctx, a, nchunks, psum, pw, pcov, t.wmean, t.wtot, o));
  else
    VCP_TRY(cm_run<3>(ctx, a, nchunks, psum, pw, pcov, t.wmean, t.wtot, o));
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
