// cluster_spheres.hip -- least-squares sphere (3-D) or circle (2-D) per cluster: vcp_cluster_spheres (include/vcp.h,
// DESIGN.md section 34).
//
// The instrument stands at the origin, so a target is seen from one side and the mean of its returns lies 2R/3 in front of
// its centre; the fit recovers the centre the returns lie around.  Per cluster: W and the mean (cluster_seg.hpp, the bits of
// vcp_cluster_moments), the algebraic (Kasa) start in the centred frame, `rounds` Gauss-Newton rounds on rho_i - r with the
// radius free (eliminated) or fixed, one closing pass.  The small solves are spdsolve.hpp.
//
// Every sum runs through the fixed tree of centroids.hip, and every cluster takes the same road whatever its size: one
// workgroup per chunk of CH members, then one thread per cluster over the chunk partials, which also solves and moves the
// centre.  The start pass gathers the rows through sorted[] once and writes d = fl(x - mean) -- and the weight, where
// there are weights -- in (label, index) order, one plane per coordinate, and each chunk's cluster and slots into a table;
// every later pass is a contiguous stream of that and finds its chunk with one load.  The folds are block_fold_sum_sparse:
// a wave past the end of its chunk skips its shuffles, which on clusters of a few members is three waves in four.
// Algorithmic bytes per member: start 4 + 8 dim read (+ 4), 8 dim written (+ 4); each round and the closing pass 8 dim
// (+ 4) read.
#include "cluster_seg.hpp"
#include "spdsolve.hpp"

namespace {
constexpr int ST = 10;  // per-cluster state, doubles: u [3] | r_ref | alg [4] | step | ok (1.0 or 0.0)

// (a0 a0 + a1 a1) + a2 a2: the association of every dot product of the definition
template <int D>
__device__ __forceinline__ double cs_dot(const double (&a)[D]) {
  double r = a[0] * a[0] + a[1] * a[1];
  if constexpr (D == 3) r = r + a[2] * a[2];
  return r;
}

// the d planes and the weights in (label, index) order, and what the start pass found for every chunk: a round reads its
// chunk's entry instead of searching chunkstart[] again
struct CsStream {
  double* d;     // plane a at d + a * n
  int32_t* w;    // or NULL
  size_t n;
  uint4* chunk;  // [nchunks]: (cluster k, first slot, end slot, 0)
};

// start, one workgroup per chunk: writes d and w of its members and the chunk's table entry; part[c * NS + .] = the chunk's
// sums of p_ab = fl(fl(w d_a) d_b) (a <= b), then of fl(fl(w q) d_a), q = d . d
template <int D>
__global__ __launch_bounds__(CT) void k_cs_chunk_start(CmSeg a, const double* __restrict__ wmean, CsStream ws,
                                                       double* __restrict__ part) {
  constexpr int NP = D * (D + 1) / 2, NS = NP + D;
  const uint32_t c = blockIdx.x;
  uint32_t beg, end;
  const int k = cm_chunk(a, c, beg, end);
  if (threadIdx.x == 0) ws.chunk[c] = make_uint4((uint32_t)k, beg, end, 0u);
  double m[D], s[NS];
#pragma unroll
  for (int j = 0; j < D; j++) m[j] = wmean[(size_t)(k - 1) * D + j];
#pragma unroll
  for (int j = 0; j < NS; j++) s[j] = 0.0;
  for (uint32_t t = beg + threadIdx.x; t < end; t += CT) {
    const uint32_t i = a.sorted[t];
    const int32_t wi = a.weights ? a.weights[i] : 1;
    const double w = (double)wi;
    const double* p = a.pts + (int64_t)i * a.ld;
    double d[D];
#pragma unroll
    for (int j = 0; j < D; j++) {
      d[j] = p[j] - m[j];
      ws.d[(size_t)j * ws.n + t] = d[j];
    }
    if (ws.w) ws.w[t] = wi;
    int ab = 0;
#pragma unroll
    for (int r = 0; r < D; r++) {
      const double wd = w * d[r];
#pragma unroll
      for (int q = r; q < D; q++, ab++) s[ab] += wd * d[q];
    }
    const double wq = w * cs_dot<D>(d);
#pragma unroll
    for (int j = 0; j < D; j++) s[NP + j] += wq * d[j];
  }
  block_fold_sum_sparse<CT>(s, beg + (threadIdx.x & ~63u) < end, part + (size_t)c * NS);
}

// start, per cluster: S u0 = T / 2, r0, the state
template <int D>
__global__ __launch_bounds__(FT) void k_cs_start(const double* __restrict__ part, const uint32_t* __restrict__ chunkstart,
                                                 int32_t K, const double* __restrict__ wmean,
                                                 const unsigned long long* __restrict__ wtot, double fixed_radius,
                                                 double* __restrict__ state) {
  constexpr int NP = D * (D + 1) / 2, NS = NP + D;
  const int k = blockIdx.x * FT + threadIdx.x + 1;
  if (k > K) return;
  double s[NS];
#pragma unroll
  for (int j = 0; j < NS; j++) s[j] = 0.0;
  for (uint32_t c = chunkstart[k]; c < chunkstart[k + 1]; c++)
#pragma unroll
    for (int j = 0; j < NS; j++) s[j] += part[(size_t)c * NS + j];
  const double Wd = (double)wtot[k - 1];
  double h[D], u[D];
#pragma unroll
  for (int j = 0; j < D; j++) h[j] = s[NP + j] * 0.5;
  const int ok = spd_solve<D>(s, h, u);
  double tr = s[0] + s[D];  // the diagonal of the packed triangle: 0, D, (2 D - 1)
  if constexpr (D == 3) tr = tr + s[5];
  const double r0 = sqrt(cs_dot<D>(u) + tr / Wd);
  double* st = state + (size_t)(k - 1) * ST;
#pragma unroll
  for (int j = 0; j < D; j++) {
    st[j] = u[j];
    st[4 + j] = wmean[(size_t)(k - 1) * D + j] + u[j];
  }
  st[3] = fixed_radius > 0.0 ? fixed_radius : r0;
  st[4 + D] = r0;
  st[8] = 0.0;
  st[9] = ok ? 1.0 : 0.0;
}

// e = fl(d - u), rho = sqrt(e . e), nu = e / rho; a member on the centre (rho == 0) has no direction: nu = 0
template <int D>
__device__ __forceinline__ void cs_member(const CsStream& ws, uint32_t t, const double (&u)[D], double& w, double& rho,
                                          double (&nu)[D]) {
  w = ws.w ? (double)ws.w[t] : 1.0;
  double e[D];
#pragma unroll
  for (int j = 0; j < D; j++) e[j] = ws.d[(size_t)j * ws.n + t] - u[j];
  rho = sqrt(cs_dot<D>(e));
#pragma unroll
  for (int j = 0; j < D; j++) nu[j] = rho == 0.0 ? 0.0 : e[j] / rho;
}

// a round, one workgroup per chunk: the sums of fl(fl(w nu_a) nu_b) (a <= b) | fl(w nu_a) | fl(w rho) | fl(fl(w rho) nu_a)
template <int D>
__global__ __launch_bounds__(CT) void k_cs_chunk_round(CsStream ws, const double* __restrict__ state,
                                                       double* __restrict__ part) {
  constexpr int NP = D * (D + 1) / 2, NS = NP + 2 * D + 1;
  const uint32_t c = blockIdx.x;
  const uint4 ce = ws.chunk[c];
  const uint32_t k = ce.x, beg = ce.y, end = ce.z;
  double u[D], s[NS];
#pragma unroll
  for (int j = 0; j < D; j++) u[j] = state[(size_t)(k - 1) * ST + j];
#pragma unroll
  for (int j = 0; j < NS; j++) s[j] = 0.0;
  for (uint32_t t = beg + threadIdx.x; t < end; t += CT) {
    double w, rho, nu[D];
    cs_member<D>(ws, t, u, w, rho, nu);
    int ab = 0;
#pragma unroll
    for (int r = 0; r < D; r++) {
      const double wn = w * nu[r];
#pragma unroll
      for (int q = r; q < D; q++, ab++) s[ab] += wn * nu[q];
      s[NP + r] += wn;
    }
    const double wr = w * rho;
    s[NP + D] += wr;
#pragma unroll
    for (int j = 0; j < D; j++) s[NP + D + 1 + j] += wr * nu[j];
  }
  block_fold_sum_sparse<CT>(s, beg + (threadIdx.x & ~63u) < end, part + (size_t)c * NS);
}

// a round, per cluster: the Gauss-Newton step with r eliminated (free) or known (fixed); u <- u + delta in place
template <int D>
__global__ __launch_bounds__(FT) void k_cs_round(const double* __restrict__ part, const uint32_t* __restrict__ chunkstart,
                                                 int32_t K, const unsigned long long* __restrict__ wtot, double fixed_radius,
                                                 double* __restrict__ state) {
  constexpr int NP = D * (D + 1) / 2, NS = NP + 2 * D + 1;
  const int k = blockIdx.x * FT + threadIdx.x + 1;
  if (k > K) return;
  double s[NS];
#pragma unroll
  for (int j = 0; j < NS; j++) s[j] = 0.0;
  for (uint32_t c = chunkstart[k]; c < chunkstart[k + 1]; c++)
#pragma unroll
    for (int j = 0; j < NS; j++) s[j] += part[(size_t)c * NS + j];
  const double Wd = (double)wtot[k - 1];
  double* st = state + (size_t)(k - 1) * ST;
  double M[NP], g[D], dl[D];
  if (fixed_radius > 0.0) {
#pragma unroll
    for (int j = 0; j < NP; j++) M[j] = s[j];
#pragma unroll
    for (int j = 0; j < D; j++) g[j] = s[NP + D + 1 + j] - fixed_radius * s[NP + j];
  } else {
    int ab = 0;
#pragma unroll
    for (int r = 0; r < D; r++)
#pragma unroll
      for (int q = r; q < D; q++, ab++) M[ab] = s[ab] - (s[NP + r] * s[NP + q]) / Wd;
#pragma unroll
    for (int j = 0; j < D; j++) g[j] = s[NP + D + 1 + j] - (s[NP + D] * s[NP + j]) / Wd;
    st[3] = s[NP + D] / Wd;  // the radius at the centre this pass saw: the closing pass centres rho on it
  }
  const int ok = spd_solve<D>(M, g, dl);
#pragma unroll
  for (int j = 0; j < D; j++) st[j] = st[j] + dl[j];
  st[8] = sqrt(cs_dot<D>(dl));
  if (!ok) st[9] = 0.0;
}

// closing, one workgroup per chunk: the sums of fl(w nu_a) | fl(w c) | fl(fl(w c) c), c = fl(rho - r_ref)
template <int D>
__global__ __launch_bounds__(CT) void k_cs_chunk_close(CsStream ws, const double* __restrict__ state,
                                                       double* __restrict__ part) {
  constexpr int NS = D + 2;
  const uint32_t c = blockIdx.x;
  const uint4 ce = ws.chunk[c];
  const uint32_t k = ce.x, beg = ce.y, end = ce.z;
  double u[D], s[NS];
#pragma unroll
  for (int j = 0; j < D; j++) u[j] = state[(size_t)(k - 1) * ST + j];
  const double rref = state[(size_t)(k - 1) * ST + 3];
#pragma unroll
  for (int j = 0; j < NS; j++) s[j] = 0.0;
  for (uint32_t t = beg + threadIdx.x; t < end; t += CT) {
    double w, rho, nu[D];
    cs_member<D>(ws, t, u, w, rho, nu);
#pragma unroll
    for (int j = 0; j < D; j++) s[j] += w * nu[j];
    const double cc = rho - rref, wc = w * cc;
    s[D] += wc;
    s[D + 1] += wc * cc;
  }
  block_fold_sum_sparse<CT>(s, beg + (threadIdx.x & ~63u) < end, part + (size_t)c * NS);
}

struct CsOut {
  double *centre, *radius, *rms, *cap, *step, *alg;
  uint8_t* valid;
  int64_t* counts;
};

// closing, per cluster: radius, rms, cap, the validity; every output that is not NULL
template <int D>
__global__ __launch_bounds__(FT) void k_cs_final(const double* __restrict__ part, const uint32_t* __restrict__ chunkstart,
                                                 int32_t K, const double* __restrict__ wmean,
                                                 const unsigned long long* __restrict__ wtot, double fixed_radius,
                                                 const double* __restrict__ state, CsOut o) {
  constexpr int NS = D + 2;
  const int k = blockIdx.x * FT + threadIdx.x + 1;
  if (k > K) return;
  double s[NS];
#pragma unroll
  for (int j = 0; j < NS; j++) s[j] = 0.0;
  for (uint32_t c = chunkstart[k]; c < chunkstart[k + 1]; c++)
#pragma unroll
    for (int j = 0; j < NS; j++) s[j] += part[(size_t)c * NS + j];
  const unsigned long long W = wtot[k - 1];
  const double Wd = (double)W;
  const double* st = state + (size_t)(k - 1) * ST;
  double b[D], centre[D], alg[D + 1], radius, rms;
#pragma unroll
  for (int j = 0; j < D; j++) {
    b[j] = s[j];
    centre[j] = wmean[(size_t)(k - 1) * D + j] + st[j];
  }
#pragma unroll
  for (int j = 0; j <= D; j++) alg[j] = st[4 + j];
  if (fixed_radius > 0.0) {
    radius = fixed_radius;
    rms = sqrt(s[D + 1] / Wd);
  } else {
    const double cb = s[D] / Wd;
    radius = st[3] + cb;
    double v = s[D + 1] / Wd - cb * cb;
    v = v < 0.0 ? 0.0 : v;  // a NaN stays
    rms = sqrt(v);
  }
  const double cap = sqrt(cs_dot<D>(b)) / Wd, step = st[8];
  bool good = W >= (unsigned long long)(fixed_radius > 0.0 ? D : D + 1) && st[9] != 0.0 && cm_finite(radius) &&
              cm_finite(rms) && cm_finite(cap) && cm_finite(step);
#pragma unroll
  for (int j = 0; j < D; j++) good = good && cm_finite(centre[j]);
#pragma unroll
  for (int j = 0; j <= D; j++) good = good && cm_finite(alg[j]);
  const double nan = cm_nan();
  const size_t z = (size_t)(k - 1);
  if (o.centre)
#pragma unroll
    for (int j = 0; j < D; j++) o.centre[z * D + j] = good ? centre[j] : nan;
  if (o.radius) o.radius[z] = good ? radius : nan;
  if (o.rms) o.rms[z] = good ? rms : nan;
  if (o.cap) o.cap[z] = good ? cap : nan;
  if (o.step) o.step[z] = good ? step : nan;
  if (o.alg)
#pragma unroll
    for (int j = 0; j <= D; j++) o.alg[z * (D + 1) + j] = good ? alg[j] : nan;
  if (o.valid) o.valid[z] = good ? 1 : 0;
  if (o.counts) o.counts[z] = (int64_t)W;
}

template <int D>
int cs_run(vcp_ctx* ctx, const CmSeg& a, const CmTables& t, const CsStream& ws, double* psum, unsigned long long* pw,
           double* part, double fixed_radius, int rounds, const CsOut& o) {
  hipStream_t st = ctx->stream;
  const dim3 gc(t.nchunks), gk(vcp_blocks(a.K, FT));
  double* state = t.extra;
  vcp_phase(ctx, "spheres_start");
  if (t.nchunks > 0) VCP_LAUNCH(ctx, k_cm_chunk_mean<D>, gc, dim3(CT), 0, st, a, psum, pw);
  VCP_LAUNCH(ctx, k_cm_mean<D>, gk, dim3(FT), 0, st, psum, pw, a.chunkstart, a.K, t.wmean, t.wtot);
  if (t.nchunks > 0) VCP_LAUNCH(ctx, k_cs_chunk_start<D>, gc, dim3(CT), 0, st, a, t.wmean, ws, part);
  VCP_LAUNCH(ctx, k_cs_start<D>, gk, dim3(FT), 0, st, part, a.chunkstart, a.K, t.wmean, t.wtot, fixed_radius, state);
  vcp_phase(ctx, "spheres_rounds");
  for (int r = 0; r < rounds; r++) {
    if (t.nchunks > 0) VCP_LAUNCH(ctx, k_cs_chunk_round<D>, gc, dim3(CT), 0, st, ws, state, part);
    VCP_LAUNCH(ctx, k_cs_round<D>, gk, dim3(FT), 0, st, part, a.chunkstart, a.K, t.wtot, fixed_radius, state);
  }
  if (t.nchunks > 0) VCP_LAUNCH(ctx, k_cs_chunk_close<D>, gc, dim3(CT), 0, st, ws, state, part);
  VCP_LAUNCH(ctx, k_cs_final<D>, gk, dim3(FT), 0, st, part, a.chunkstart, a.K, t.wmean, t.wtot, fixed_radius, state, o);
  return VCP_OK;
}

int cs_check(vcp_ctx* ctx, const void* pts, int64_t ld, int dim, const void* labels, int64_t n, int32_t K,
             double fixed_radius, int rounds) {
  VCP_TRY(cm_check(ctx, pts, ld, dim, labels, n, K));
  if (!(fixed_radius == 0.0 || (fixed_radius > 0.0 && fixed_radius <= 1.7976931348623157e308)))
    return vcp_fail(ctx, VCP_ERR_ARG, "fixed_radius %g is neither 0 nor finite and > 0", fixed_radius);
  if (rounds < 0 || rounds > 64) return vcp_fail(ctx, VCP_ERR_ARG, "rounds %d outside 0..64", rounds);
  return VCP_OK;
}
}  // namespace

extern "C" {

int vcp_cluster_spheres_dev(vcp_ctx* ctx, const double* d_pts, int64_t ld, int dim, const int32_t* d_labels,
                            const int32_t* d_weights, int64_t n, int32_t K, double fixed_radius, int rounds,
                            double* d_centre, double* d_radius, double* d_rms, double* d_cap, double* d_step, double* d_alg,
                            uint8_t* d_valid, int64_t* d_counts) {
  if (!ctx) return VCP_ERR_ARG;
  VCP_TRY(cs_check(ctx, d_pts, ld, dim, d_labels, n, K, fixed_radius, rounds));
  VCP_TRY(vcp_bind(ctx));
  vcp_phase_reset(ctx);
  hipStream_t st = ctx->stream;
  vcp_phase(ctx, "spheres_group");
  CmTables t;  // in b_cs_misc (cluster_seg.hpp), with the per-cluster state behind it
  VCP_TRY(cm_group(ctx, ctx->b_cs_misc, (size_t)K * ST, d_labels, d_weights, n, K, t));
  if (K == 0) return vcp_phase_finish(ctx);
  // b_cs_d: d [dim planes of n] | w [n] int32 (with weights).  b_aux4: the chunk table [nchunks] of 16 bytes | psum
  // [nchunks * 3] | part [nchunks * 13] | pw [nchunks]
  const size_t nn = (size_t)n, nc = t.nchunks;
  VCP_TRY(vcp_ensure(ctx, ctx->b_cs_d, nn * dim * 8 + nn * 4 + 64));
  VCP_TRY(vcp_ensure(ctx, ctx->b_aux4, (nc + 1) * 19 * 8));
  double* psum = reinterpret_cast<double*>(ctx->b_aux4.as<uint4>() + nc);
  double* part = psum + nc * 3;
  unsigned long long* pw = reinterpret_cast<unsigned long long*>(part + nc * 13);
  const CsStream ws{ctx->b_cs_d.as<double>(), d_weights ? reinterpret_cast<int32_t*>(ctx->b_cs_d.as<double>() + nn * dim) : nullptr,
                    nn, ctx->b_aux4.as<uint4>()};
  const CmSeg a{t.sorted, t.segstart, t.counts, t.chunkstart, K, d_pts, ld, d_weights};
  const CsOut o{d_centre, d_radius, d_rms, d_cap, d_step, d_alg, d_valid, d_counts};
  if (dim == 2)
    VCP_TRY(cs_run<2>(ctx, a, t, ws, psum, pw, part, fixed_radius, rounds, o));
  else
    VCP_TRY(cs_run<3>(ctx, a, t, ws, psum, pw, part, fixed_radius, rounds, o));
  VCP_TRY(vcp_phase_finish(ctx));
  VCP_HIP(ctx, hipStreamSynchronize(st));
  return VCP_OK;
}

int vcp_cluster_spheres(vcp_ctx* ctx, const double* pts, int64_t ld, int dim, const int32_t* labels, const int32_t* weights,
                        int64_t n, int32_t K, double fixed_radius, int rounds, double* centre, double* radius, double* rms,
                        double* cap, double* step, double* alg, uint8_t* valid, int64_t* counts) {
  if (!ctx) return VCP_ERR_ARG;
  VCP_TRY(cs_check(ctx, pts, ld, dim, labels, n, K, fixed_radius, rounds));
  VCP_TRY(vcp_bind(ctx));
  hipStream_t st = ctx->stream;
  // in: [pts span * 8 | labels n * 4 | weights n * 4]; out: the doubles [centre | radius | rms | cap | step | alg], counts,
  // valid
  const size_t span = cm_span(n, ld, dim), k = (size_t)K, d = (size_t)dim;
  VCP_TRY(vcp_ensure(ctx, ctx->b_cs_in, span * 8 + (size_t)n * 8));
  VCP_TRY(vcp_ensure(ctx, ctx->b_cs_out, k * (2 * d + 5) * 8 + k * 8 + k));
  char* din = ctx->b_cs_in.as<char>();
  const int32_t* dl = reinterpret_cast<const int32_t*>(din + span * 8);
  const int32_t* dw = weights ? dl + n : nullptr;
  if (n > 0) {
    VCP_HIP(ctx, hipMemcpyAsync(din, pts, span * 8, hipMemcpyHostToDevice, st));
    VCP_HIP(ctx, hipMemcpyAsync(din + span * 8, labels, (size_t)n * 4, hipMemcpyHostToDevice, st));
    if (weights) VCP_HIP(ctx, hipMemcpyAsync(din + span * 8 + (size_t)n * 4, weights, (size_t)n * 4, hipMemcpyHostToDevice, st));
  }
  double* o_centre = ctx->b_cs_out.as<double>();
  double* o_radius = o_centre + k * d;
  double* o_rms = o_radius + k;
  double* o_cap = o_rms + k;
  double* o_step = o_cap + k;
  double* o_alg = o_step + k;
  int64_t* o_counts = reinterpret_cast<int64_t*>(o_alg + k * (d + 1));
  uint8_t* o_valid = reinterpret_cast<uint8_t*>(o_counts + k);
  VCP_TRY(vcp_cluster_spheres_dev(ctx, reinterpret_cast<const double*>(din), ld, dim, dl, dw, n, K, fixed_radius, rounds,
                                  centre ? o_centre : nullptr, radius ? o_radius : nullptr, rms ? o_rms : nullptr,
                                  cap ? o_cap : nullptr, step ? o_step : nullptr, alg ? o_alg : nullptr,
                                  valid ? o_valid : nullptr, counts ? o_counts : nullptr));
  if (K > 0) {
    if (centre) VCP_HIP(ctx, hipMemcpyAsync(centre, o_centre, k * d * 8, hipMemcpyDeviceToHost, st));
    if (radius) VCP_HIP(ctx, hipMemcpyAsync(radius, o_radius, k * 8, hipMemcpyDeviceToHost, st));
    if (rms) VCP_HIP(ctx, hipMemcpyAsync(rms, o_rms, k * 8, hipMemcpyDeviceToHost, st));
    if (cap) VCP_HIP(ctx, hipMemcpyAsync(cap, o_cap, k * 8, hipMemcpyDeviceToHost, st));
    if (step) VCP_HIP(ctx, hipMemcpyAsync(step, o_step, k * 8, hipMemcpyDeviceToHost, st));
    if (alg) VCP_HIP(ctx, hipMemcpyAsync(alg, o_alg, k * (d + 1) * 8, hipMemcpyDeviceToHost, st));
    if (counts) VCP_HIP(ctx, hipMemcpyAsync(counts, o_counts, k * 8, hipMemcpyDeviceToHost, st));
    if (valid) VCP_HIP(ctx, hipMemcpyAsync(valid, o_valid, k, hipMemcpyDeviceToHost, st));
    VCP_HIP(ctx, hipStreamSynchronize(st));
  }
  return VCP_OK;
}

int vcp_selftest_spd_solve(int dim, const double* s_packed, const double* b, double* x, int* ok) {
  if (!s_packed || !b || !x || (dim != 2 && dim != 3)) return VCP_ERR_ARG;
  const int r = dim == 2 ? spd_solve<2>(s_packed, b, x) : spd_solve<3>(s_packed, b, x);
  if (ok) *ok = r;
  return 1;
}

}  // extern "C"
