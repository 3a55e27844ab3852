// point_features.hip -- the local surface at every return: vcp_point_features (include/vcp_features.h, which holds the
// definition).
//
// Every other entry point describes a cluster, a neighbourhood's size or the few largest planes.  This one reads the k
// neighbour rows the caller has (vcp_kdist's knn: ascending (distance, index), a pinned order) and gives per row the
// covariance of the neighbourhood through symeig.hpp -- the normal, the eigenvalues, the surface variation -- and the
// mean distance to the neighbours.  The order of a row's slots is the order of every sum, so the result is a function of
// the input alone and tests/point_features_ref.py restates it in numpy for equality.
//
// One kernel family, k_pf_rows<D, KC>: one lane per row, consecutive lanes consecutive rows, KC the smallest of
// 8 / 16 / 32 / 64 that is >= k.  A workgroup takes PF_T rows per trip; their neighbour indices are one contiguous span of
// PF_T * k words, which the workgroup reads with coalesced loads (256 bytes per wave instruction) into LDS at a row
// stride of KC + 1 words: odd, so that the lanes' reads of their own slot s fall into 64 different banks.  Pass 1 (the
// sums of the coordinates, and the distances to p_i, which need nothing else) and pass 2 (the centred products) walk
// the slots in order:
//   KC <= 16   every gathered row stays in registers between the passes (48 doubles for D = 3; compile-time indices
//              only, as symeig.hpp needs); the loads of a row's whole list are issued before the first sum;
//   KC >  16   PF_G gathers in flight per lane in both passes; the second pass reads what the first has just read.
// A slot that is no member loads the row i itself (an address that is always valid) and is left out of every sum by a
// select, so there is no branch around a load.  No atomics, no workspace: the _dev form owns nothing on the device.
//
// Workspace of the host form (FeaturesWs, owned by the context through vcp_ctx::features; both buffers are listed in
// vcp_ctx::bufs):
//   b_pf_in    the rows, then the neighbour rows
//   b_pf_out   normal, eval, variation, mean_dist, then count, then valid: the ones the caller asked for are copied back
#include <cmath>
#include <new>

#include "vcp_ctx.hpp"
#include "vcp_features.h"
#include "symeig.hpp"

struct FeaturesWs {
  DevBuf b_pf_in, b_pf_out;
};

extern "C" void vcp_features_ws_free(vcp_ctx* ctx) {
  delete ctx->features;  // the buffers were freed through ctx->bufs
  ctx->features = nullptr;
}

namespace {
constexpr int PF_T = 128;          // threads per workgroup = rows per trip: 33 KB of LDS at KC = 64
constexpr int PF_G = 4;            // gathers in flight per lane on the re-gather road
constexpr int PF_KREG = 16;        // the largest KC whose rows stay in registers between the passes
constexpr int PF_WG_PER_CU = 8;    // the grid's cap
constexpr int PF_MAX_K = 64;

__device__ __forceinline__ double pf_nan() { return __longlong_as_double(0x7FF8000000000000LL); }
__device__ __forceinline__ double pf_canon(double v) { return v != v ? pf_nan() : v; }
__device__ __forceinline__ bool pf_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }  // false for NaN

struct PfArgs {
  const double* pts;
  int64_t ld, n;
  const int32_t* nbr;
  int32_t k, has_vp;
  double vp0, vp1, vp2;  // the viewpoint (has_vp), by value
  double *normal, *eval, *variation, *mean_dist;
  int32_t* count;
  uint8_t* valid;
};

template <int D>
__device__ __forceinline__ void pf_load(const double* __restrict__ pts, int64_t ld, int64_t j, double (&x)[D]) {
  const double* p = pts + j * ld;
#pragma unroll
  for (int a = 0; a < D; a++) x[a] = p[a];
}

// pass 1, one slot: the coordinate sums over the members, the distance sum over the members that are not the row itself
template <int D>
struct PfSum {
  double s[D], sd;
  int m, q;
};
template <int D>
__device__ __forceinline__ void pf_pass1(PfSum<D>& acc, const double (&x)[D], const double (&p)[D], bool mem, bool other) {
  double e2 = 0.0;
#pragma unroll
  for (int a = 0; a < D; a++) {
    const double e = x[a] - p[a];
    const double t = e * e;
    e2 = a == 0 ? t : e2 + t;
    acc.s[a] = mem ? acc.s[a] + x[a] : acc.s[a];
  }
  const double dist = sqrt(e2);
  acc.sd = other ? acc.sd + dist : acc.sd;
  acc.m += mem ? 1 : 0;
  acc.q += other ? 1 : 0;
}

// pass 2, one slot: S_ab += fl(d_a d_b), d = fl(x - mean)
template <int D>
__device__ __forceinline__ void pf_pass2(double (&S)[D * (D + 1) / 2], const double (&x)[D], const double (&mean)[D], bool mem) {
  double d[D];
#pragma unroll
  for (int a = 0; a < D; a++) d[a] = x[a] - mean[a];
  int ab = 0;
#pragma unroll
  for (int r = 0; r < D; r++)
#pragma unroll
    for (int c = r; c < D; c++, ab++) S[ab] = mem ? S[ab] + d[r] * d[c] : S[ab];
}

// Workgroup b takes the trips b, b + gridDim.x, ... of PF_T rows each.
template <int D, int KC>
__global__ __launch_bounds__(PF_T) void k_pf_rows(PfArgs a, uint32_t ntrips) {
  constexpr int NP = D * (D + 1) / 2;
  constexpr int KS = KC + 1;                      // the LDS row stride in words: odd
  __shared__ int32_t s_nbr[PF_T * KS + PF_G];     // + PF_G: the last row's reads of the slots k .. k + PF_G - 1 stay inside
  const int k = a.k;
  const int64_t n = a.n;
  for (uint32_t trip = blockIdx.x; trip < ntrips; trip += gridDim.x) {  // workgroup-uniform
    const int64_t row0 = (int64_t)trip * PF_T;
    const int rows = n - row0 < PF_T ? (int)(n - row0) : PF_T;
    const int words = rows * k;
    const int32_t* __restrict__ src = a.nbr + row0 * k;
    __syncthreads();  // the last trip's reads of s_nbr are done
    {
      // word w of the span is slot w % k of row w / k: one division, then steps of PF_T words
      int w = threadIdx.x, r = w / k, s = w - r * k;
      const int dr = PF_T / k, ds = PF_T - dr * k;
      for (; w < words; w += PF_T) {
        s_nbr[r * KS + s] = src[w];
        r += dr;
        s += ds;
        if (s >= k) {
          s -= k;
          r++;
        }
      }
    }
    __syncthreads();
    const int64_t i = row0 + threadIdx.x;
    if (i >= n) continue;  // the barriers above are reached by every thread: trip and ntrips are uniform
    const int32_t* nb = s_nbr + threadIdx.x * KS;
    double p[D];
    pf_load<D>(a.pts, a.ld, i, p);
    PfSum<D> acc;
#pragma unroll
    for (int c = 0; c < D; c++) acc.s[c] = 0.0;
    acc.sd = 0.0;
    acc.m = acc.q = 0;
    double mean[D], S[NP];
#pragma unroll
    for (int c = 0; c < NP; c++) S[c] = 0.0;
    if constexpr (KC <= PF_KREG) {
      double x[KC][D];
      uint32_t memmask = 0, othermask = 0;
#pragma unroll
      for (int s = 0; s < KC; s++) {
        const int32_t j = s < k ? nb[s] : -1;
        const bool mem = (uint32_t)j < (uint32_t)n;  // n < 2^31
        memmask |= mem ? 1u << s : 0u;
        othermask |= (mem && j != i) ? 1u << s : 0u;
        pf_load<D>(a.pts, a.ld, mem ? (int64_t)j : i, x[s]);
      }
#pragma unroll
      for (int s = 0; s < KC; s++) pf_pass1<D>(acc, x[s], p, (memmask >> s) & 1u, (othermask >> s) & 1u);
#pragma unroll
      for (int c = 0; c < D; c++) mean[c] = acc.s[c] / (double)acc.m;
#pragma unroll
      for (int s = 0; s < KC; s++) pf_pass2<D>(S, x[s], mean, (memmask >> s) & 1u);
    } else {
      for (int s0 = 0; s0 < k; s0 += PF_G) {
        double x[PF_G][D];
        bool mem[PF_G], other[PF_G];
#pragma unroll
        for (int u = 0; u < PF_G; u++) {
          const int32_t j = s0 + u < k ? nb[s0 + u] : -1;
          mem[u] = (uint32_t)j < (uint32_t)n;
          other[u] = mem[u] && j != i;
          pf_load<D>(a.pts, a.ld, mem[u] ? (int64_t)j : i, x[u]);
        }
#pragma unroll
        for (int u = 0; u < PF_G; u++) pf_pass1<D>(acc, x[u], p, mem[u], other[u]);
      }
#pragma unroll
      for (int c = 0; c < D; c++) mean[c] = acc.s[c] / (double)acc.m;
      for (int s0 = 0; s0 < k; s0 += PF_G) {
        double x[PF_G][D];
        bool mem[PF_G];
#pragma unroll
        for (int u = 0; u < PF_G; u++) {
          const int32_t j = s0 + u < k ? nb[s0 + u] : -1;
          mem[u] = (uint32_t)j < (uint32_t)n;
          pf_load<D>(a.pts, a.ld, mem[u] ? (int64_t)j : i, x[u]);
        }
#pragma unroll
        for (int u = 0; u < PF_G; u++) pf_pass2<D>(S, x[u], mean, mem[u]);
      }
    }
    // the covariance, its eigen-solve, the derived numbers
    const double md = (double)acc.m;
    double cov[NP], eval[D], evec[D * D];
    bool fin = true;
#pragma unroll
    for (int c = 0; c < NP; c++) {
      cov[c] = S[c] / md;
      fin = fin && pf_finite(cov[c]);
    }
#pragma unroll
    for (int c = 0; c < D; c++) fin = fin && pf_finite(mean[c]);
    (void)sym_eig<D>(cov, eval, evec);
    double nv[D];
#pragma unroll
    for (int c = 0; c < D; c++) nv[c] = evec[(D - 1) * D + c];
    if (a.has_vp) {
      double sgn = nv[0] * (a.vp0 - p[0]) + nv[1] * (a.vp1 - p[1]);
      if constexpr (D == 3) sgn = sgn + nv[2] * (a.vp2 - p[2]);
      if (sgn < 0.0)
#pragma unroll
        for (int c = 0; c < D; c++) nv[c] = -nv[c];
    }
    double sum = eval[0];
#pragma unroll
    for (int c = 1; c < D; c++) sum = sum + eval[c];
    const double var = sum == 0.0 ? 0.0 : eval[D - 1] / sum;
    const double mdist = acc.sd / (double)acc.q;
    if (a.normal)
#pragma unroll
      for (int c = 0; c < D; c++) a.normal[i * D + c] = pf_canon(nv[c]);
    if (a.eval)
#pragma unroll
      for (int c = 0; c < D; c++) a.eval[i * D + c] = pf_canon(eval[c]);
    if (a.variation) a.variation[i] = pf_canon(var);
    if (a.mean_dist) a.mean_dist[i] = pf_canon(mdist);
    if (a.count) a.count[i] = acc.m;
    if (a.valid) a.valid[i] = (acc.m >= D && fin) ? 1 : 0;
  }
}

// ---- host side --------------------------------------------------------------------------------------------------------
unsigned pf_grid_cap(vcp_ctx* ctx) {
  return (unsigned)(ctx->prop.multiProcessorCount > 0 ? ctx->prop.multiProcessorCount : 256) * (unsigned)PF_WG_PER_CU;
}

int pf_check(vcp_ctx* ctx, const void* pts, int64_t ld, int dim, int64_t n, const void* nbr, int k) {
  if (n < 0) return vcp_fail(ctx, VCP_ERR_ARG, "n < 0");
  if (dim != 2 && dim != 3) return vcp_fail(ctx, VCP_ERR_ARG, "dim %d is not 2 or 3", dim);
  if (ld < dim) return vcp_fail(ctx, VCP_ERR_ARG, "ld %lld below dim %d", (long long)ld, dim);
  if (k < 1) return vcp_fail(ctx, VCP_ERR_ARG, "k %d below 1", k);
  if (n > 0 && (!pts || !nbr)) return vcp_fail(ctx, VCP_ERR_ARG, "null pts or nbr");
  if (k > PF_MAX_K) return vcp_fail(ctx, VCP_ERR_UNSUPPORTED, "k %d above %d", k, PF_MAX_K);
  if (n >= 0x7FFFFFF0LL) return vcp_fail(ctx, VCP_ERR_TOO_LARGE, "n beyond 32-bit indexing");
  return VCP_OK;
}

template <int D, int KC>
int pf_launch(vcp_ctx* ctx, const PfArgs& a) {
  const int64_t ntrips = (a.n + PF_T - 1) / PF_T;
  VCP_LAUNCH(ctx, (k_pf_rows<D, KC>), dim3(vcp_blocks(ntrips, 1, (int)pf_grid_cap(ctx))), dim3(PF_T), 0, ctx->stream, a,
             (uint32_t)ntrips);
  return VCP_OK;
}

template <int D>
int pf_run(vcp_ctx* ctx, const PfArgs& a) {
  if (a.k <= 8) return pf_launch<D, 8>(ctx, a);
  if (a.k <= 16) return pf_launch<D, 16>(ctx, a);
  if (a.k <= 32) return pf_launch<D, 32>(ctx, a);
  return pf_launch<D, 64>(ctx, a);
}

int pf_ws(vcp_ctx* ctx, FeaturesWs*& ws) {
  if (!ctx->features) ctx->features = new (std::nothrow) FeaturesWs();
  if (!ctx->features) return vcp_fail(ctx, VCP_ERR_NOMEM, "the features workspace");
  ws = ctx->features;
  return VCP_OK;
}

size_t pf_span(int64_t n, int64_t ld, int dim) { return n > 0 ? (size_t)(n - 1) * (size_t)ld + (size_t)dim : 0; }
}  // namespace

extern "C" {

int vcp_point_features_shape(vcp_ctx* ctx, int32_t shape[6]) {
  if (!ctx) return VCP_ERR_ARG;
  if (!shape) return vcp_fail(ctx, VCP_ERR_ARG, "null shape");
  shape[0] = PF_T;
  shape[1] = (int32_t)pf_grid_cap(ctx);
  shape[2] = 8;
  shape[3] = 16;
  shape[4] = 32;
  shape[5] = 64;
  static_assert(PF_KREG == 16 && PF_MAX_K == 64, "the classes pf_run chooses among");
  return VCP_OK;
}

int vcp_point_features_dev(vcp_ctx* ctx, const double* d_pts, int64_t ld, int dim, int64_t n, const int32_t* d_nbr, int k,
                           const double* viewpoint, double* d_normal, double* d_eval, double* d_variation,
                           double* d_mean_dist, int32_t* d_count, uint8_t* d_valid) {
  if (!ctx) return VCP_ERR_ARG;
  VCP_TRY(pf_check(ctx, d_pts, ld, dim, n, d_nbr, k));
  if (n == 0 || (!d_normal && !d_eval && !d_variation && !d_mean_dist && !d_count && !d_valid)) return VCP_OK;
  VCP_TRY(vcp_bind(ctx));
  const PfArgs a{d_pts, ld, n, d_nbr, k, viewpoint ? 1 : 0, viewpoint ? viewpoint[0] : 0.0, viewpoint ? viewpoint[1] : 0.0,
                 viewpoint && dim == 3 ? viewpoint[2] : 0.0, d_normal, d_eval, d_variation, d_mean_dist, d_count, d_valid};
  vcp_phase_reset(ctx);
  vcp_phase(ctx, "features_rows");
  VCP_TRY(dim == 2 ? pf_run<2>(ctx, a) : pf_run<3>(ctx, a));
  VCP_TRY(vcp_phase_finish(ctx));
  VCP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return VCP_OK;
}

int vcp_point_features(vcp_ctx* ctx, const double* pts, int64_t ld, int dim, int64_t n, const int32_t* nbr, int k,
                       const double* viewpoint, double* normal, double* eval, double* variation, double* mean_dist,
                       int32_t* count, uint8_t* valid) {
  if (!ctx) return VCP_ERR_ARG;
  VCP_TRY(pf_check(ctx, pts, ld, dim, n, nbr, k));
  if (n == 0 || (!normal && !eval && !variation && !mean_dist && !count && !valid)) return VCP_OK;
  VCP_TRY(vcp_bind(ctx));
  FeaturesWs* ws;
  VCP_TRY(pf_ws(ctx, ws));
  hipStream_t st = ctx->stream;
  // in: [pts span * 8 | nbr n * k * 4]; out: the doubles [normal | eval | variation | mean_dist], count, valid
  const size_t span = pf_span(n, ld, dim), nn = (size_t)n, d = (size_t)dim;
  VCP_TRY(vcp_ensure(ctx, ws->b_pf_in, span * 8 + nn * (size_t)k * 4));
  VCP_TRY(vcp_ensure(ctx, ws->b_pf_out, nn * (2 * d + 2) * 8 + nn * 4 + nn));
  char* din = ws->b_pf_in.as<char>();
  const int32_t* dnbr = reinterpret_cast<const int32_t*>(din + span * 8);
  VCP_HIP(ctx, hipMemcpyAsync(din, pts, span * 8, hipMemcpyHostToDevice, st));
  VCP_HIP(ctx, hipMemcpyAsync(din + span * 8, nbr, nn * (size_t)k * 4, hipMemcpyHostToDevice, st));
  double* o_normal = ws->b_pf_out.as<double>();
  double* o_eval = o_normal + nn * d;
  double* o_var = o_eval + nn * d;
  double* o_md = o_var + nn;
  int32_t* o_count = reinterpret_cast<int32_t*>(o_md + nn);
  uint8_t* o_valid = reinterpret_cast<uint8_t*>(o_count + nn);
  VCP_TRY(vcp_point_features_dev(ctx, reinterpret_cast<const double*>(din), ld, dim, n, dnbr, k, viewpoint,
                                 normal ? o_normal : nullptr, eval ? o_eval : nullptr, variation ? o_var : nullptr,
                                 mean_dist ? o_md : nullptr, count ? o_count : nullptr, valid ? o_valid : nullptr));
  if (normal) VCP_HIP(ctx, hipMemcpyAsync(normal, o_normal, nn * d * 8, hipMemcpyDeviceToHost, st));
  if (eval) VCP_HIP(ctx, hipMemcpyAsync(eval, o_eval, nn * d * 8, hipMemcpyDeviceToHost, st));
  if (variation) VCP_HIP(ctx, hipMemcpyAsync(variation, o_var, nn * 8, hipMemcpyDeviceToHost, st));
  if (mean_dist) VCP_HIP(ctx, hipMemcpyAsync(mean_dist, o_md, nn * 8, hipMemcpyDeviceToHost, st));
  if (count) VCP_HIP(ctx, hipMemcpyAsync(count, o_count, nn * 4, hipMemcpyDeviceToHost, st));
  if (valid) VCP_HIP(ctx, hipMemcpyAsync(valid, o_valid, nn, hipMemcpyDeviceToHost, st));
  VCP_HIP(ctx, hipStreamSynchronize(st));
  return VCP_OK;
}

}  // extern "C"
