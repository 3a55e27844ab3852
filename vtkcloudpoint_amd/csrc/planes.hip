// planes.hip -- plane extraction by consensus: vcp_plane_ransac and its building blocks (include/vcp_planes.h, DESIGN.md
// section 36).
//
// Everything else in the library looks at a cluster or at a neighbourhood; this looks at the whole cloud before it is
// clustered.  Most returns that are not targets lie on a few large planes: RANSAC finds them (H triples per round, each
// triple's plane scored against every active row, the best one refitted by least squares and its rows removed) and
// vcp_dbscan gets the rest.
//
// The score is the hot path and the one kernel here that arithmetic bounds: n * H residuals of 3 multiplies, 3 adds and a
// compare over one read of the cloud per PL_CHUNK hypotheses.  A lane keeps PL_P rows in registers, every plane is read
// wave-uniformly (through the scalar cache; PL_PLANES_IN_LDS), the inliers of a wave are counted with __ballot / __popcll into
// a per-workgroup counter array in LDS and leave it as one global integer add per (workgroup, hypothesis).  Integer
// counts: the result does not depend on the order of anything, which is what lets tests/plane_ref.py restate it in numpy
// and compare for equality.  Sampling is a counter-based hash (splitmix64), so a hypothesis is a function of (seed, round,
// h) and of the active list alone.  The refit is vcp_cluster_moments_dev with K = 1 as it stands.
//
// Workspace (PlanesWs, owned by the context through vcp_ctx::planes; every buffer is listed in vcp_ctx::bufs):
//   b_pl_in    the host forms' inputs on the device: the rows, then the planes (vcp_plane_score) or nothing, then active
//   b_pl_out   the host forms' outputs: the counts (vcp_plane_score) or the labels (vcp_plane_ransac)
//   b_pl_act   vcp_plane_ransac: the working active flags [n] uint8 (the caller's are read only), then at the next
//              multiple of 16 bytes the refit's labels [n] int32
//   b_pl_list  vcp_plane_ransac: the flags' scan [n] uint32, then the active list [n] uint32 (rows in ascending index)
//   b_pl_hyp   the planes [H * 4] doubles, the counts [H] 64-bit, the PlRec of the call (256 bytes), the triples [H * 3]
//              int32; vcp_plane_label_dev uses the PlRec alone
// The refit's vcp_cluster_moments_dev uses b_cm_misc, b_aux1 .. b_aux4, the scan's descriptors and [0, 32) of the pinned
// scratch: none of them holds anything of a round across that call.
#include <cmath>
#include <cstring>
#include <new>

#include "vcp_ctx.hpp"
#include "vcp_planes.h"
#include "wave.hpp"

struct PlanesWs {
  DevBuf b_pl_in, b_pl_out, b_pl_act, b_pl_list, b_pl_hyp;
};

extern "C" void vcp_planes_ws_free(vcp_ctx* ctx) {
  delete ctx->planes;  // the buffers were freed through ctx->bufs
  ctx->planes = nullptr;
}

// Where the score kernel's inner loop reads a hypothesis from: 0 = global memory at a wave-uniform address, through the
// scalar cache (one s_load_dwordx8 per hypothesis; the planes reach the multiplies as SGPR operands); 1 = the chunk staged in
// LDS, one broadcast read per hypothesis.  Both were timed at 10 M rows (profiles/planes_bench.txt): the scalar read took
// 12 to 14 % less time at H = 256, 1024 and 4096, so it is the build.
#ifndef PL_PLANES_IN_LDS
#define PL_PLANES_IN_LDS 0
#endif

namespace {
constexpr int PL_T = 256;            // threads per workgroup
constexpr int PL_P = 4;              // rows per lane: 24 VGPRs of coordinates
constexpr int PL_TILE = PL_T * PL_P;  // rows a workgroup takes per trip
constexpr int PL_CHUNK = 1024;       // hypotheses per pass over the cloud: 4 KB of counters in LDS (+ 32 KB of planes when staged)
constexpr int PL_WG_PER_CU = PL_PLANES_IN_LDS ? 4 : 8;  // the grid's cap: 8 workgroups, 32 waves per CU (4 x 36 KB of LDS with the planes staged)
constexpr int PL_MAX_H = 65536;
constexpr int PL_MAX_PLANES = 64;
constexpr size_t PL_PINNED = 4096;   // the call's words in the pinned scratch (vcp_ctx.hpp)

__device__ __forceinline__ double pl_nan() { return __longlong_as_double(0x7FF8000000000000LL); }
__device__ __forceinline__ bool pl_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }  // false for NaN

struct PlPlane {
  double a, b, c, d;
};

// r = fl(fl(fl(fl(a x) + fl(b y)) + fl(c z)) + d); -ffp-contract=off keeps every rounding
__device__ __forceinline__ bool pl_inlier(const PlPlane& p, double x, double y, double z, double thr) {
  const double r = ((p.a * x + p.b * y) + p.c * z) + p.d;
  return fabs(r) <= thr;
}

// what comes back to the host in a round, in b_pl_hyp
struct PlRec {
  long long win_count;  // the winner's count
  int32_t win_h, pad0;
  double win_plane[4];
  double refit_plane[4];
  unsigned long long refit_count;
  unsigned long long n_labelled;
  uint32_t m, pad1;     // active rows (the scan's total)
  double mean[3], evec[9];  // of the refit's vcp_cluster_moments_dev
  uint8_t refit_valid, pad2[7];
};
static_assert(sizeof(PlRec) <= 256, "PlRec fits its slot");

// ---- the score --------------------------------------------------------------------------------------------------------
// counts[h] += the active rows of this workgroup's tiles that are inliers of plane h.  Workgroup b takes the tiles b,
// b + gridDim.x, ...; per chunk of PL_CHUNK hypotheses one pass over them.  A row that is inactive or beyond n is held as
// NaN, which is an inlier of nothing: the inner loop has no mask.
__global__ __launch_bounds__(PL_T) void k_pl_score(const double* __restrict__ pts, int64_t ld, int64_t n,
                                                   const uint8_t* __restrict__ active, const double* __restrict__ planes,
                                                   int32_t H, double thr, unsigned long long* __restrict__ counts,
                                                   uint32_t ntiles) {
#if PL_PLANES_IN_LDS
  __shared__ __attribute__((aligned(32))) double s_pl[PL_CHUNK * 4];
#endif
  __shared__ uint32_t s_cnt[PL_CHUNK];
  const int lane = threadIdx.x & 63;
  for (int32_t h0 = 0; h0 < H; h0 += PL_CHUNK) {
    const int hc = H - h0 < PL_CHUNK ? H - h0 : PL_CHUNK;
#if PL_PLANES_IN_LDS
    for (int j = threadIdx.x; j < hc * 4; j += PL_T) s_pl[j] = planes[(size_t)h0 * 4 + j];
#else
    const double* __restrict__ g_pl = planes + (size_t)h0 * 4;  // a wave-uniform address: read through the scalar cache
#endif
    for (int j = threadIdx.x; j < hc; j += PL_T) s_cnt[j] = 0u;
    __syncthreads();
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
      double x[PL_P], y[PL_P], z[PL_P];
#pragma unroll
      for (int k = 0; k < PL_P; k++) {
        const int64_t i = (int64_t)tile * PL_TILE + k * PL_T + threadIdx.x;
        x[k] = y[k] = z[k] = pl_nan();
        if (i < n && (!active || active[i])) {
          const double* p = pts + i * ld;
          x[k] = p[0];
          y[k] = p[1];
          z[k] = p[2];
        }
      }
      for (int h = 0; h < hc; h++) {
#if PL_PLANES_IN_LDS
        const PlPlane pl{s_pl[h * 4 + 0], s_pl[h * 4 + 1], s_pl[h * 4 + 2], s_pl[h * 4 + 3]};  // one address: a broadcast read
#else
        const PlPlane pl{g_pl[h * 4 + 0], g_pl[h * 4 + 1], g_pl[h * 4 + 2], g_pl[h * 4 + 3]};
#endif
        uint32_t c = 0;
#pragma unroll
        for (int k = 0; k < PL_P; k++) c += wave_count(pl_inlier(pl, x[k], y[k], z[k], thr));
        if (lane == 0 && c) atomicAdd(&s_cnt[h], c);
      }
    }
    __syncthreads();
    for (int j = threadIdx.x; j < hc; j += PL_T)
      if (s_cnt[j]) atomicAdd(&counts[h0 + j], (unsigned long long)s_cnt[j]);
    __syncthreads();
  }
}

// ---- hypotheses -------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t pl_mix(uint64_t seed, uint64_t c) {
  uint64_t z = seed + 0x9E3779B97F4A7C15ULL * (c + 1);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}

// tri[h * 3 + j] = list[(mix(seed, (r H + h) 3 + j) m) >> 64]
__global__ __launch_bounds__(PL_T) void k_pl_sample(const uint32_t* __restrict__ list, uint32_t m, uint64_t seed,
                                                    uint64_t c0, int32_t H, int32_t* __restrict__ tri) {
  const int t = blockIdx.x * PL_T + threadIdx.x;
  if (t >= H * 3) return;
  const uint64_t slot = __umul64hi(pl_mix(seed, c0 + (uint64_t)t), (uint64_t)m);
  tri[t] = (int32_t)list[slot];
}

__global__ __launch_bounds__(PL_T) void k_pl_from_tri(const double* __restrict__ pts, int64_t ld, int64_t n,
                                                      const int32_t* __restrict__ tri, int32_t H,
                                                      double* __restrict__ planes, uint8_t* __restrict__ valid) {
  const int h = blockIdx.x * PL_T + threadIdx.x;
  if (h >= H) return;
  const int64_t i0 = tri[h * 3 + 0], i1 = tri[h * 3 + 1], i2 = tri[h * 3 + 2];
  bool ok = i0 >= 0 && i0 < n && i1 >= 0 && i1 < n && i2 >= 0 && i2 < n;
  double a = pl_nan(), b = pl_nan(), c = pl_nan(), d = pl_nan();
  if (ok) {
    const double *p0 = pts + i0 * ld, *p1 = pts + i1 * ld, *p2 = pts + i2 * ld;
    const double p0x = p0[0], p0y = p0[1], p0z = p0[2];
    const double ux = p1[0] - p0x, uy = p1[1] - p0y, uz = p1[2] - p0z;
    const double vx = p2[0] - p0x, vy = p2[1] - p0y, vz = p2[2] - p0z;
    const double cx = uy * vz - uz * vy, cy = uz * vx - ux * vz, cz = ux * vy - uy * vx;
    const double nrm = sqrt((cx * cx + cy * cy) + cz * cz);
    a = cx / nrm;
    b = cy / nrm;
    c = cz / nrm;
    d = -((a * p0x + b * p0y) + c * p0z);
    ok = pl_finite(nrm) && nrm > 0.0 && pl_finite(a) && pl_finite(b) && pl_finite(c) && pl_finite(d);
  }
  if (!ok) a = b = c = d = pl_nan();
  planes[(size_t)h * 4 + 0] = a;
  planes[(size_t)h * 4 + 1] = b;
  planes[(size_t)h * 4 + 2] = c;
  planes[(size_t)h * 4 + 3] = d;
  if (valid) valid[h] = ok ? 1 : 0;
}

// The largest count, on a tie the lowest h: the maximum of count << 16 | (65535 - h) (count < 2^31, h < 65536).  One
// workgroup.
__global__ __launch_bounds__(PL_T) void k_pl_winner(const unsigned long long* __restrict__ counts,
                                                    const double* __restrict__ planes, int32_t H, PlRec* __restrict__ rec) {
  __shared__ unsigned long long s_best[PL_T / 64];
  unsigned long long best = 0;
  for (int h = threadIdx.x; h < H; h += PL_T) best = max(best, (counts[h] << 16) | (unsigned long long)(65535 - h));
  best = wave_all<WaveMax>(best);
  if ((threadIdx.x & 63) == 0) s_best[threadIdx.x >> 6] = best;
  __syncthreads();
  if (threadIdx.x != 0) return;
  for (int w = 1; w < PL_T / 64; w++) best = max(best, s_best[w]);
  const int h = 65535 - (int)(best & 0xFFFFu);
  rec->win_count = (long long)(best >> 16);
  rec->win_h = h;
#pragma unroll
  for (int j = 0; j < 4; j++) rec->win_plane[j] = planes[(size_t)h * 4 + j];
}

// the refit plane from the moments of the winner's inliers: the axis of the smallest eigenvalue through the mean
__global__ void k_pl_refit_plane(PlRec* __restrict__ rec) {
  const double a = rec->evec[6], b = rec->evec[7], c = rec->evec[8];
  rec->refit_plane[0] = a;
  rec->refit_plane[1] = b;
  rec->refit_plane[2] = c;
  rec->refit_plane[3] = -((a * rec->mean[0] + b * rec->mean[1]) + c * rec->mean[2]);
}

// ---- the active set ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PL_T) void k_pl_act_init(const uint8_t* __restrict__ active, int64_t n, uint8_t* __restrict__ act) {
  for (int64_t i = (int64_t)blockIdx.x * PL_T + threadIdx.x; i < n; i += (int64_t)gridDim.x * PL_T)
    act[i] = active[i] ? 1 : 0;
}

__global__ __launch_bounds__(PL_T) void k_pl_flag(const uint8_t* __restrict__ act, int64_t n, uint32_t* __restrict__ flag) {
  for (int64_t i = (int64_t)blockIdx.x * PL_T + threadIdx.x; i < n; i += (int64_t)gridDim.x * PL_T) flag[i] = act[i] ? 1u : 0u;
}

// list[pos[i]] = i for the active rows: ascending index, because pos is the exclusive scan of the flags
__global__ __launch_bounds__(PL_T) void k_pl_scatter(const uint8_t* __restrict__ act, const uint32_t* __restrict__ pos,
                                                     int64_t n, uint32_t* __restrict__ list) {
  for (int64_t i = (int64_t)blockIdx.x * PL_T + threadIdx.x; i < n; i += (int64_t)gridDim.x * PL_T)
    if (act[i]) list[pos[i]] = (uint32_t)i;
}

// lab1[i] = 1 for the active inliers of the plane, 0 for every other row: the refit's labels
__global__ __launch_bounds__(PL_T) void k_pl_mark(const double* __restrict__ pts, int64_t ld, int64_t n,
                                                  const uint8_t* __restrict__ act, const PlRec* __restrict__ rec, double thr,
                                                  int32_t* __restrict__ lab1) {
  const PlPlane pl{rec->win_plane[0], rec->win_plane[1], rec->win_plane[2], rec->win_plane[3]};
  for (int64_t i = (int64_t)blockIdx.x * PL_T + threadIdx.x; i < n; i += (int64_t)gridDim.x * PL_T) {
    const double* p = pts + i * ld;
    lab1[i] = act[i] && pl_inlier(pl, p[0], p[1], p[2], thr) ? 1 : 0;
  }
}

// the active inliers: labels[i] = id, active[i] = 0; one add of the wave's count per wave
__global__ __launch_bounds__(PL_T) void k_pl_label(const double* __restrict__ pts, int64_t ld, int64_t n,
                                                   uint8_t* __restrict__ active, PlPlane pl, double thr, int32_t id,
                                                   int32_t* __restrict__ labels, unsigned long long* __restrict__ n_labelled) {
  uint32_t c = 0;
  for (int64_t base = (int64_t)blockIdx.x * PL_T; base < n; base += (int64_t)gridDim.x * PL_T) {  // workgroup-uniform
    const int64_t i = base + threadIdx.x;
    bool in = false;
    if (i < n && (!active || active[i])) {
      const double* p = pts + i * ld;
      in = pl_inlier(pl, p[0], p[1], p[2], thr);
    }
    if (in) {
      labels[i] = id;
      if (active) active[i] = 0;
    }
    c += wave_count(in);
  }
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(n_labelled, (unsigned long long)c);
}

// ---- host side --------------------------------------------------------------------------------------------------------
unsigned pl_walk(vcp_ctx* ctx, int per_cu) {
  return (unsigned)(ctx->prop.multiProcessorCount > 0 ? ctx->prop.multiProcessorCount : 256) * (unsigned)per_cu;
}

int pl_check_rows(vcp_ctx* ctx, const void* pts, int64_t ld, int64_t n) {
  if (n < 0) return vcp_fail(ctx, VCP_ERR_ARG, "n < 0");
  if (ld < 3) return vcp_fail(ctx, VCP_ERR_ARG, "ld %lld below 3", (long long)ld);
  if (n > 0 && !pts) return vcp_fail(ctx, VCP_ERR_ARG, "null pts");
  if (n >= 0x7FFFFFF0LL) return vcp_fail(ctx, VCP_ERR_TOO_LARGE, "n beyond 32-bit indexing");
  return VCP_OK;
}
int pl_check_h(vcp_ctx* ctx, int32_t H) {
  if (H < 1 || H > PL_MAX_H) return vcp_fail(ctx, VCP_ERR_ARG, "H %d outside 1..%d", H, PL_MAX_H);
  return VCP_OK;
}
int pl_check_thr(vcp_ctx* ctx, double thr) {
  if (!(thr >= 0.0)) return vcp_fail(ctx, VCP_ERR_ARG, "thr is negative or NaN");
  return VCP_OK;
}

int pl_ws(vcp_ctx* ctx, PlanesWs*& ws) {
  if (!ctx->planes) ctx->planes = new (std::nothrow) PlanesWs();
  if (!ctx->planes) return vcp_fail(ctx, VCP_ERR_NOMEM, "the planes workspace");
  ws = ctx->planes;
  return VCP_OK;
}

// b_pl_hyp of a call with H hypotheses
struct PlHyp {
  double* planes;
  unsigned long long* counts;
  PlRec* rec;
  int32_t* tri;
};
int pl_hyp(vcp_ctx* ctx, PlanesWs* ws, int32_t H, PlHyp& y) {
  const size_t h = (size_t)H;
  VCP_TRY(vcp_ensure(ctx, ws->b_pl_hyp, h * 32 + h * 8 + 256 + h * 12));
  y.planes = ws->b_pl_hyp.as<double>();
  y.counts = reinterpret_cast<unsigned long long*>(y.planes + h * 4);
  y.rec = reinterpret_cast<PlRec*>(y.counts + h);
  y.tri = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(y.rec) + 256);
  return VCP_OK;
}

PlRec* pl_pinned(vcp_ctx* ctx) { return reinterpret_cast<PlRec*>(static_cast<char*>(ctx->pinned) + PL_PINNED); }

// the PlRec to the host; returns when it is there
int pl_fetch(vcp_ctx* ctx, const PlRec* d_rec) {
  VCP_HIP(ctx, hipMemcpyAsync(pl_pinned(ctx), d_rec, sizeof(PlRec), hipMemcpyDeviceToHost, ctx->stream));
  VCP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return VCP_OK;
}

// counts[0 .. H) = the scores, from zero
int pl_score(vcp_ctx* ctx, const double* d_pts, int64_t ld, int64_t n, const uint8_t* d_active, const double* d_planes,
             int32_t H, double thr, unsigned long long* d_counts) {
  hipStream_t st = ctx->stream;
  VCP_HIP(ctx, hipMemsetAsync(d_counts, 0, (size_t)H * 8, st));
  const int64_t ntiles = (n + PL_TILE - 1) / PL_TILE;
  if (ntiles == 0) return VCP_OK;
  VCP_LAUNCH(ctx, k_pl_score, dim3(vcp_blocks(ntiles, 1, (int)pl_walk(ctx, PL_WG_PER_CU))), dim3(PL_T), 0, st, d_pts, ld, n,
             d_active, d_planes, H, thr, d_counts, (uint32_t)ntiles);
  return VCP_OK;
}

int pl_from_tri(vcp_ctx* ctx, const double* d_pts, int64_t ld, int64_t n, const int32_t* d_tri, int32_t H, double* d_planes,
                uint8_t* d_valid) {
  VCP_LAUNCH(ctx, k_pl_from_tri, dim3(vcp_blocks(H, PL_T)), dim3(PL_T), 0, ctx->stream, d_pts, ld, n, d_tri, H, d_planes,
             d_valid);
  return VCP_OK;
}

// labels the active inliers; the count is in rec->n_labelled on the stream (not yet fetched)
int pl_label(vcp_ctx* ctx, const double* d_pts, int64_t ld, int64_t n, uint8_t* d_active, const PlPlane& pl, double thr,
             int32_t id, int32_t* d_labels, PlRec* rec) {
  hipStream_t st = ctx->stream;
  VCP_HIP(ctx, hipMemsetAsync(&rec->n_labelled, 0, 8, st));
  if (n > 0)
    VCP_LAUNCH(ctx, k_pl_label, dim3(vcp_blocks(n, PL_T, (int)pl_walk(ctx, 8))), dim3(PL_T), 0, st, d_pts, ld, n, d_active, pl,
               thr, id, d_labels, &rec->n_labelled);
  return VCP_OK;
}

// vcp_cluster_moments_dev resets and closes the context's timing phases as an entry point of its own: run it with the
// timing off and put the phases of this call back (no event is taken from the pool meanwhile)
int pl_moments(vcp_ctx* ctx, const double* d_pts, int64_t ld, int64_t n, const int32_t* d_lab1, PlRec* rec) {
  const bool timing = ctx->timing;
  const std::vector<Phase> phases = ctx->phases;
  const size_t used = ctx->ev_used;
  ctx->timing = false;
  const int rc = vcp_cluster_moments_dev(ctx, d_pts, ld, 3, d_lab1, nullptr, n, 1, rec->mean, nullptr, nullptr, rec->evec,
                                         nullptr, &rec->refit_valid, nullptr);
  ctx->timing = timing;
  ctx->phases = phases;
  ctx->ev_used = used;
  return rc;
}

size_t pl_span(int64_t n, int64_t ld) { return n > 0 ? (size_t)(n - 1) * (size_t)ld + 3 : 0; }

int pl_check_ransac(vcp_ctx* ctx, const void* pts, int64_t ld, int64_t n, double thr, int32_t H, int32_t max_planes,
                    int64_t min_inliers, const void* labels, const void* planes, const void* counts, const void* hyp_counts,
                    const void* n_planes) {
  if (n < 0) return vcp_fail(ctx, VCP_ERR_ARG, "n < 0");
  if (ld < 3) return vcp_fail(ctx, VCP_ERR_ARG, "ld %lld below 3", (long long)ld);
  VCP_TRY(pl_check_h(ctx, H));
  if (max_planes < 0 || max_planes > PL_MAX_PLANES)
    return vcp_fail(ctx, VCP_ERR_ARG, "max_planes %d outside 0..%d", max_planes, PL_MAX_PLANES);
  if (min_inliers < 0) return vcp_fail(ctx, VCP_ERR_ARG, "min_inliers < 0");
  VCP_TRY(pl_check_thr(ctx, thr));
  if (!n_planes) return vcp_fail(ctx, VCP_ERR_ARG, "null n_planes");
  if (n > 0 && (!pts || !labels)) return vcp_fail(ctx, VCP_ERR_ARG, "null pts or labels");
  if (max_planes > 0 && (!planes || !counts || !hyp_counts)) return vcp_fail(ctx, VCP_ERR_ARG, "null planes, counts or hyp_counts");
  if (n >= 0x7FFFFFF0LL) return vcp_fail(ctx, VCP_ERR_TOO_LARGE, "n beyond 32-bit indexing");
  return VCP_OK;
}
}  // namespace

extern "C" {

int vcp_plane_score_shape(vcp_ctx* ctx, int32_t shape[3]) {
  if (!ctx) return VCP_ERR_ARG;
  if (!shape) return vcp_fail(ctx, VCP_ERR_ARG, "null shape");
  shape[0] = PL_TILE;
  shape[1] = PL_CHUNK;
  shape[2] = (int32_t)pl_walk(ctx, PL_WG_PER_CU);
  return VCP_OK;
}

int vcp_plane_score_dev(vcp_ctx* ctx, const double* d_pts, int64_t ld, int64_t n, const uint8_t* d_active,
                        const double* d_planes, int32_t H, double thr, int64_t* d_counts) {
  if (!ctx) return VCP_ERR_ARG;
  VCP_TRY(pl_check_rows(ctx, d_pts, ld, n));
  VCP_TRY(pl_check_h(ctx, H));
  VCP_TRY(pl_check_thr(ctx, thr));
  if (!d_planes || !d_counts) return vcp_fail(ctx, VCP_ERR_ARG, "null planes or counts");
  VCP_TRY(vcp_bind(ctx));
  vcp_phase_reset(ctx);
  vcp_phase(ctx, "planes_score");
  VCP_TRY(pl_score(ctx, d_pts, ld, n, d_active, d_planes, H, thr, reinterpret_cast<unsigned long long*>(d_counts)));
  VCP_TRY(vcp_phase_finish(ctx));
  VCP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return VCP_OK;
}

int vcp_plane_score(vcp_ctx* ctx, const double* pts, int64_t ld, int64_t n, const uint8_t* active, const double* planes,
                    int32_t H, double thr, int64_t* counts) {
  if (!ctx) return VCP_ERR_ARG;
  VCP_TRY(pl_check_rows(ctx, pts, ld, n));
  VCP_TRY(pl_check_h(ctx, H));
  VCP_TRY(pl_check_thr(ctx, thr));
  if (!planes || !counts) return vcp_fail(ctx, VCP_ERR_ARG, "null planes or counts");
  VCP_TRY(vcp_bind(ctx));
  PlanesWs* ws;
  VCP_TRY(pl_ws(ctx, ws));
  hipStream_t st = ctx->stream;
  // in: [pts span * 8 | planes H * 32 | active n]; out: counts H * 8
  const size_t span = pl_span(n, ld), h = (size_t)H;
  VCP_TRY(vcp_ensure(ctx, ws->b_pl_in, span * 8 + h * 32 + (size_t)n));
  VCP_TRY(vcp_ensure(ctx, ws->b_pl_out, h * 8));
  char* din = ws->b_pl_in.as<char>();
  double* dpl = reinterpret_cast<double*>(din + span * 8);
  uint8_t* dact = reinterpret_cast<uint8_t*>(dpl + h * 4);
  if (n > 0) VCP_HIP(ctx, hipMemcpyAsync(din, pts, span * 8, hipMemcpyHostToDevice, st));
  VCP_HIP(ctx, hipMemcpyAsync(dpl, planes, h * 32, hipMemcpyHostToDevice, st));
  if (n > 0 && active) VCP_HIP(ctx, hipMemcpyAsync(dact, active, (size_t)n, hipMemcpyHostToDevice, st));
  VCP_TRY(vcp_plane_score_dev(ctx, reinterpret_cast<const double*>(din), ld, n, active ? dact : nullptr, dpl, H, thr,
                              ws->b_pl_out.as<int64_t>()));
  VCP_HIP(ctx, hipMemcpyAsync(counts, ws->b_pl_out.p, h * 8, hipMemcpyDeviceToHost, st));
  VCP_HIP(ctx, hipStreamSynchronize(st));
  return VCP_OK;
}

int vcp_planes_from_triples_dev(vcp_ctx* ctx, const double* d_pts, int64_t ld, int64_t n, const int32_t* d_tri, int32_t H,
                                double* d_planes, uint8_t* d_valid) {
  if (!ctx) return VCP_ERR_ARG;
  VCP_TRY(pl_check_rows(ctx, d_pts, ld, n));
  VCP_TRY(pl_check_h(ctx, H));
  if (!d_tri || !d_planes) return vcp_fail(ctx, VCP_ERR_ARG, "null tri or planes");
  VCP_TRY(vcp_bind(ctx));
  vcp_phase_reset(ctx);
  vcp_phase(ctx, "planes_sample");
  VCP_TRY(pl_from_tri(ctx, d_pts, ld, n, d_tri, H, d_planes, d_valid));
  VCP_TRY(vcp_phase_finish(ctx));
  VCP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return VCP_OK;
}

int vcp_plane_label_dev(vcp_ctx* ctx, const double* d_pts, int64_t ld, int64_t n, uint8_t* d_active, const double plane[4],
                        double thr, int32_t id, int32_t* d_labels, int64_t* n_labelled) {
  if (!ctx) return VCP_ERR_ARG;
  VCP_TRY(pl_check_rows(ctx, d_pts, ld, n));
  VCP_TRY(pl_check_thr(ctx, thr));
  if (!plane || !n_labelled) return vcp_fail(ctx, VCP_ERR_ARG, "null plane or n_labelled");
  if (n > 0 && !d_labels) return vcp_fail(ctx, VCP_ERR_ARG, "null labels");
  VCP_TRY(vcp_bind(ctx));
  PlanesWs* ws;
  VCP_TRY(pl_ws(ctx, ws));
  PlHyp y;
  VCP_TRY(pl_hyp(ctx, ws, 1, y));
  vcp_phase_reset(ctx);
  vcp_phase(ctx, "planes_label");
  VCP_TRY(pl_label(ctx, d_pts, ld, n, d_active, PlPlane{plane[0], plane[1], plane[2], plane[3]}, thr, id, d_labels, y.rec));
  VCP_TRY(vcp_phase_finish(ctx));
  VCP_TRY(pl_fetch(ctx, y.rec));
  *n_labelled = (int64_t)pl_pinned(ctx)->n_labelled;
  return VCP_OK;
}

int vcp_plane_ransac_dev(vcp_ctx* ctx, const double* d_pts, int64_t ld, int64_t n, const uint8_t* d_active, double thr,
                         int32_t H, int32_t max_planes, int64_t min_inliers, uint64_t seed, int32_t refit, int32_t* d_labels,
                         double* planes, int64_t* counts, int64_t* hyp_counts, int32_t* n_planes) {
  if (!ctx) return VCP_ERR_ARG;
  VCP_TRY(pl_check_ransac(ctx, d_pts, ld, n, thr, H, max_planes, min_inliers, d_labels, planes, counts, hyp_counts, n_planes));
  VCP_TRY(vcp_bind(ctx));
  hipStream_t st = ctx->stream;
  vcp_phase_reset(ctx);
  // the results of the rounds, handed over at the end
  double r_planes[PL_MAX_PLANES * 4];
  int64_t r_counts[PL_MAX_PLANES], r_hyp[PL_MAX_PLANES];
  int32_t np = 0;
  if (n > 0) VCP_HIP(ctx, hipMemsetAsync(d_labels, 0, (size_t)n * 4, st));
  if (n > 0 && max_planes > 0) {
    PlanesWs* ws;
    VCP_TRY(pl_ws(ctx, ws));
    PlHyp y;
    VCP_TRY(pl_hyp(ctx, ws, H, y));
    const size_t lab_off = ((size_t)n + 15) & ~(size_t)15;
    VCP_TRY(vcp_ensure(ctx, ws->b_pl_act, lab_off + (size_t)n * 4));
    VCP_TRY(vcp_ensure(ctx, ws->b_pl_list, (size_t)n * 8));
    uint8_t* act = ws->b_pl_act.as<uint8_t>();
    int32_t* lab1 = reinterpret_cast<int32_t*>(act + lab_off);
    uint32_t* pos = ws->b_pl_list.as<uint32_t>();
    uint32_t* list = pos + n;
    const dim3 walk(vcp_blocks(n, PL_T, (int)pl_walk(ctx, 8)));
    if (d_active)
      VCP_LAUNCH(ctx, k_pl_act_init, walk, dim3(PL_T), 0, st, d_active, n, act);
    else
      VCP_HIP(ctx, hipMemsetAsync(act, 1, (size_t)n, st));
    const PlRec* hp = pl_pinned(ctx);
    const int64_t need = min_inliers > 3 ? min_inliers : 3;
    for (int32_t r = 0; r < max_planes; r++) {
      // the active list, the triples, their planes
      vcp_phase(ctx, "planes_sample");
      VCP_LAUNCH(ctx, k_pl_flag, walk, dim3(PL_T), 0, st, act, n, pos);
      VCP_TRY(vcp_exclusive_scan_u32(ctx, pos, pos, n, &y.rec->m));
      VCP_LAUNCH(ctx, k_pl_scatter, walk, dim3(PL_T), 0, st, act, pos, n, list);
      VCP_TRY(pl_fetch(ctx, y.rec));
      const uint32_t m = hp->m;
      if (m < 3) break;
      VCP_LAUNCH(ctx, k_pl_sample, dim3(vcp_blocks((int64_t)H * 3, PL_T)), dim3(PL_T), 0, st, list, m, seed,
                 (uint64_t)r * (uint64_t)H * 3u, H, y.tri);
      VCP_TRY(pl_from_tri(ctx, d_pts, ld, n, y.tri, H, y.planes, nullptr));
      // the counts and the winner
      vcp_phase(ctx, "planes_score");
      VCP_TRY(pl_score(ctx, d_pts, ld, n, act, y.planes, H, thr, y.counts));
      VCP_LAUNCH(ctx, k_pl_winner, dim3(1), dim3(PL_T), 0, st, y.counts, y.planes, H, y.rec);
      VCP_TRY(pl_fetch(ctx, y.rec));
      const int64_t win = hp->win_count;
      if (win < need) break;
      PlPlane acc{hp->win_plane[0], hp->win_plane[1], hp->win_plane[2], hp->win_plane[3]};
      if (refit) {
        vcp_phase(ctx, "planes_refit");
        VCP_LAUNCH(ctx, k_pl_mark, walk, dim3(PL_T), 0, st, d_pts, ld, n, act, y.rec, thr, lab1);
        VCP_TRY(pl_moments(ctx, d_pts, ld, n, lab1, y.rec));
        VCP_LAUNCH(ctx, k_pl_refit_plane, dim3(1), dim3(1), 0, st, y.rec);
        VCP_TRY(pl_score(ctx, d_pts, ld, n, act, y.rec->refit_plane, 1, thr, &y.rec->refit_count));
        VCP_TRY(pl_fetch(ctx, y.rec));
        if (hp->refit_valid == 1 && (int64_t)hp->refit_count >= win)
          acc = PlPlane{hp->refit_plane[0], hp->refit_plane[1], hp->refit_plane[2], hp->refit_plane[3]};
      }
      vcp_phase(ctx, "planes_label");
      VCP_TRY(pl_label(ctx, d_pts, ld, n, act, acc, thr, r + 1, d_labels, y.rec));
      VCP_TRY(pl_fetch(ctx, y.rec));
      r_planes[np * 4 + 0] = acc.a;
      r_planes[np * 4 + 1] = acc.b;
      r_planes[np * 4 + 2] = acc.c;
      r_planes[np * 4 + 3] = acc.d;
      r_counts[np] = (int64_t)hp->n_labelled;
      r_hyp[np] = win;
      np++;
    }
  }
  VCP_TRY(vcp_phase_finish(ctx));
  VCP_HIP(ctx, hipStreamSynchronize(st));
  const uint64_t nan_bits = 0x7FF8000000000000ULL;
  for (int32_t r = 0; r < max_planes; r++) {
    for (int j = 0; j < 4; j++) {
      if (r < np)
        planes[r * 4 + j] = r_planes[r * 4 + j];
      else
        memcpy(&planes[r * 4 + j], &nan_bits, 8);
    }
    counts[r] = r < np ? r_counts[r] : 0;
    hyp_counts[r] = r < np ? r_hyp[r] : 0;
  }
  *n_planes = np;
  return VCP_OK;
}

int vcp_plane_ransac(vcp_ctx* ctx, const double* pts, int64_t ld, int64_t n, const uint8_t* active, double thr, int32_t H,
                     int32_t max_planes, int64_t min_inliers, uint64_t seed, int32_t refit, int32_t* labels, double* planes,
                     int64_t* counts, int64_t* hyp_counts, int32_t* n_planes) {
  if (!ctx) return VCP_ERR_ARG;
  VCP_TRY(pl_check_ransac(ctx, pts, ld, n, thr, H, max_planes, min_inliers, labels, planes, counts, hyp_counts, n_planes));
  VCP_TRY(vcp_bind(ctx));
  PlanesWs* ws;
  VCP_TRY(pl_ws(ctx, ws));
  hipStream_t st = ctx->stream;
  // in: [pts span * 8 | active n]; out: labels n * 4
  const size_t span = pl_span(n, ld);
  VCP_TRY(vcp_ensure(ctx, ws->b_pl_in, span * 8 + (size_t)n));
  VCP_TRY(vcp_ensure(ctx, ws->b_pl_out, (size_t)n * 4));
  char* din = ws->b_pl_in.as<char>();
  uint8_t* dact = reinterpret_cast<uint8_t*>(din + span * 8);
  if (n > 0) {
    VCP_HIP(ctx, hipMemcpyAsync(din, pts, span * 8, hipMemcpyHostToDevice, st));
    if (active) VCP_HIP(ctx, hipMemcpyAsync(dact, active, (size_t)n, hipMemcpyHostToDevice, st));
  }
  VCP_TRY(vcp_plane_ransac_dev(ctx, reinterpret_cast<const double*>(din), ld, n, active ? dact : nullptr, thr, H, max_planes,
                               min_inliers, seed, refit, ws->b_pl_out.as<int32_t>(), planes, counts, hyp_counts, n_planes));
  if (n > 0) {
    VCP_HIP(ctx, hipMemcpyAsync(labels, ws->b_pl_out.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    VCP_HIP(ctx, hipStreamSynchronize(st));
  }
  return VCP_OK;
}

}  // extern "C"
