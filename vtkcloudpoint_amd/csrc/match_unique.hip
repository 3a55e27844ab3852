// match_unique.hip -- vcp_match_unique: a one-to-one pairing of centroids and truths (include/vcp.h).
//
// Definition: the greedy walk over the candidate pairs { (j, i) : d(j, i) < max_dist } in ascending order of the key
// (d, j, i), a pair being accepted when neither end is taken.  d is vcp_match's expression (match.hpp's transform, then
// sqrt(dx*dx + dy*dy + dz*dz) in binary64).  The device reaches the same pairing by rounds of locally dominant pairs: in
// a round every pair that is the minimum-key candidate of BOTH its ends, among the points still free, is accepted at
// once.  The key order is strict and total, so the smallest remaining key is always such a pair (the rounds end) and a
// locally dominant pair is one the walk accepts (no smaller key touches either end).
//
// Candidates come from epsgrid.hpp's grid over the finite truths for max_dist: a centroid meets the truths of the
// 3 x 3 x 3 cells around it.
//
// A round is three kernels over the list of centroids that are still free and still have a free candidate:
//   k_mu_best    every listed centroid scans its candidates among the free truths, keeps its own minimum (d, i) and
//                lowers the truth's word tmin[i] to d's bit pattern (a non-negative double orders like its bits)
//   k_mu_name    the same scan; on an edge whose d equals tmin[i] it lowers tj[i] to j
//   k_mu_accept  a centroid whose own best truth names it back is paired; one without a free candidate leaves the list
//                for good (a taken truth never comes back); the others are compacted into the next round's list
// Only integer min-atomics decide anything, so the outcome does not depend on scheduling (the ORDER of the compacted
// list does, and nothing reads it as an order).  tmin / tj exist twice: round r works on set r & 1 and k_mu_best clears
// the other set's words of every truth it meets, which are exactly the words the next round can touch.
// Rounds are enqueued BATCH at a time behind device-side counters; the host reads them once per batch.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "epsgrid.hpp"
#include "match.hpp"
#include "vcp_ctx.hpp"
#include "wave.hpp"

namespace {
constexpr int MT = 128;
constexpr int BATCH = 8;  // rounds per host synchronisation (even: the two lists swap back)
constexpr unsigned long long NOKEY = ~0ull;

struct M16 {
  double m[16];
};

__global__ __launch_bounds__(MT) void k_mu_init(const double* __restrict__ centers, int K, int T, M16 M,
                                                double* __restrict__ mx, double* __restrict__ mxyz,
                                                int32_t* __restrict__ truth_of, int32_t* __restrict__ center_of,
                                                double* __restrict__ pair_dist, int32_t* __restrict__ list,
                                                unsigned long long* __restrict__ tmin, uint32_t* __restrict__ tj) {
  const int64_t t = (int64_t)blockIdx.x * MT + threadIdx.x;
  if (t < K) {
    const int j = (int)t;
    double m[3];
    mtc::transform(M.m, centers[3 * j], centers[3 * j + 1], centers[3 * j + 2], m);
#pragma unroll
    for (int a = 0; a < 3; a++) {
      mx[3 * j + a] = m[a];
      if (mxyz) mxyz[3 * j + a] = m[a];
    }
    truth_of[j] = -1;
    if (pair_dist) pair_dist[j] = INFINITY;
    list[j] = j;
  }
  if (t < T) {
    center_of[t] = -1;
    tmin[t] = NOKEY;
    tmin[(size_t)T + t] = NOKEY;
    tj[t] = 0xFFFFFFFFu;
    tj[(size_t)T + t] = 0xFFFFFFFFu;
  }
}

struct MUScan {
  EpsGrid g;
  const uint32_t* cellstart;
  const double* sxyz;
  const int32_t* sidx;
  const int32_t* center_of;
  double max_dist;
};

// f(i, bits of d) for every candidate edge of m to a free truth
template <class F>
__device__ __forceinline__ void mu_candidates(const MUScan& q, const double* m, F&& f) {
  eg_query_rows(q.g, q.cellstart, m, [&](uint32_t s0, uint32_t s1) {
    for (uint32_t s = s0; s < s1; s++) {
      const int i = q.sidx[s];
      if (q.center_of[i] >= 0) continue;
      const double dx = q.sxyz[3 * (size_t)s] - m[0], dy = q.sxyz[3 * (size_t)s + 1] - m[1],
                   dz = q.sxyz[3 * (size_t)s + 2] - m[2];
      const double d = sqrt(dx * dx + dy * dy + dz * dz);
      if (d < q.max_dist && d < INFINITY) f(i, (unsigned long long)__double_as_longlong(d));
    }
  });
}

// ctr[0] = centroids in `list`, ctr[1] = pairs this round accepts, ctr[2] = centroids in the next list
__global__ __launch_bounds__(MT) void k_mu_best(const int32_t* __restrict__ list, const uint32_t* __restrict__ ctr,
                                                const double* __restrict__ mx, MUScan q,
                                                unsigned long long* __restrict__ tmin_cur,
                                                unsigned long long* __restrict__ tmin_nxt, uint32_t* __restrict__ tj_nxt,
                                                unsigned long long* __restrict__ bestd, int32_t* __restrict__ besti) {
  const uint32_t t = blockIdx.x * MT + threadIdx.x;
  if (t >= ctr[0]) return;
  const int j = list[t];
  const double m[3] = {mx[3 * j], mx[3 * j + 1], mx[3 * j + 2]};
  unsigned long long bd = NOKEY;
  int bi = -1;
  mu_candidates(q, m, [&](int i, unsigned long long bits) {
    if (bits < bd || (bits == bd && i < bi)) {
      bd = bits;
      bi = i;
    }
    if (bits < __hip_atomic_load(&tmin_cur[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&tmin_cur[i], bits);
    tmin_nxt[i] = NOKEY;
    tj_nxt[i] = 0xFFFFFFFFu;
  });
  bestd[t] = bd;
  besti[t] = bi;
}

__global__ __launch_bounds__(MT) void k_mu_name(const int32_t* __restrict__ list, const uint32_t* __restrict__ ctr,
                                                const double* __restrict__ mx, MUScan q,
                                                const unsigned long long* __restrict__ tmin_cur,
                                                uint32_t* __restrict__ tj_cur, const int32_t* __restrict__ besti) {
  const uint32_t t = blockIdx.x * MT + threadIdx.x;
  if (t >= ctr[0] || besti[t] < 0) return;
  const int j = list[t];
  const double m[3] = {mx[3 * j], mx[3 * j + 1], mx[3 * j + 2]};
  mu_candidates(q, m, [&](int i, unsigned long long bits) {
    if (bits == tmin_cur[i] && (uint32_t)j < __hip_atomic_load(&tj_cur[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
      atomicMin(&tj_cur[i], (uint32_t)j);
  });
}

__global__ __launch_bounds__(MT) void k_mu_accept(const int32_t* __restrict__ list, uint32_t* __restrict__ ctr,
                                                  const uint32_t* __restrict__ tj_cur,
                                                  const unsigned long long* __restrict__ bestd,
                                                  const int32_t* __restrict__ besti, int32_t* __restrict__ truth_of,
                                                  int32_t* __restrict__ center_of, double* __restrict__ pair_dist,
                                                  int32_t* __restrict__ list_nxt) {
  const uint32_t t = blockIdx.x * MT + threadIdx.x;
  const int lane = threadIdx.x & 63;
  bool keep = false, acc = false;
  int j = 0;
  if (t < ctr[0]) {
    j = list[t];
    const int bi = besti[t];
    if (bi >= 0) {
      if (tj_cur[bi] == (uint32_t)j) {
        acc = true;
        truth_of[j] = bi;
        center_of[bi] = j;
        if (pair_dist) pair_dist[j] = __longlong_as_double((long long)bestd[t]);
      } else {
        keep = true;
      }
    }
  }
  const uint32_t slot = wave_append(keep, &ctr[2]), na = wave_count(acc);
  if (keep) list_nxt[slot] = j;
  if (na && lane == 0) atomicAdd(&ctr[1], na);
}

// the counters of one batch: (BATCH + 1) pairs of words, all zero but the first list's length
__global__ __launch_bounds__(64) void k_mu_batch(uint32_t* __restrict__ ctr, uint32_t nact) {
  if (threadIdx.x < 2 * (BATCH + 1)) ctr[threadIdx.x] = threadIdx.x == 0 ? nact : 0u;
}
}  // namespace

extern "C" {

int vcp_match_unique_dev(vcp_ctx* ctx, const double* d_centers, int32_t K, const double* d_truths, int32_t T,
                         const double M[16], double max_dist, double* d_matched_xyz, int32_t* d_truth_of,
                         int32_t* d_center_of, double* d_pair_dist, int32_t* count_pairs, int32_t* rounds) {
  if (!ctx) return VCP_ERR_ARG;
  if (K < 0 || T < 0 || !M || !d_truth_of || !d_center_of) return vcp_fail(ctx, VCP_ERR_ARG, "bad argument");
  if (count_pairs) *count_pairs = 0;
  if (rounds) *rounds = 0;
  if (K == 0) {
    if (T > 0) {
      VCP_TRY(vcp_bind(ctx));
      VCP_HIP(ctx, hipMemsetAsync(d_center_of, 0xFF, (size_t)T * 4, ctx->stream));
      VCP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return VCP_OK;
  }
  if (T == 0) return vcp_fail(ctx, VCP_ERR_EMPTY, "no truth points (truePointCloud.GetPoint(0), FrmMain.cs:3598)");
  if (!d_centers || !d_truths) return vcp_fail(ctx, VCP_ERR_ARG, "null buffer");
  VCP_TRY(vcp_bind(ctx));
  vcp_phase_reset(ctx);
  hipStream_t st = ctx->stream;
  const size_t kk = (size_t)K, tt = (size_t)T;
  // per centroid: [mx K*24 | bestd K*8 | list A K*4 | list B K*4 | besti K*4]
  const size_t c_mx = 0, c_bd = kk * 24, c_la = c_bd + kk * 8, c_lb = c_la + kk * 4, c_bi = c_lb + kk * 4;
  VCP_TRY(vcp_ensure(ctx, ctx->b_mu_cent, c_bi + kk * 4));
  // per truth: [tmin 2*T*8 | sxyz T*24 | tj 2*T*4 | sidx T*4 | cellof T*4]
  const size_t t_min = 0, t_xyz = tt * 16, t_j = t_xyz + tt * 24, t_idx = t_j + tt * 8, t_cell = t_idx + tt * 4;
  VCP_TRY(vcp_ensure(ctx, ctx->b_mu_truth, t_cell + tt * 4));
  const int rb = vcp_bounds_parts(T);
  // [round counters 128 | bounds 64 | bounds partials]
  VCP_TRY(vcp_ensure(ctx, ctx->b_mu_misc, 192 + (size_t)rb * 64));
  char* dc = ctx->b_mu_cent.as<char>();
  char* dt = ctx->b_mu_truth.as<char>();
  double* mx = reinterpret_cast<double*>(dc + c_mx);
  unsigned long long* bestd = reinterpret_cast<unsigned long long*>(dc + c_bd);
  int32_t* lists[2] = {reinterpret_cast<int32_t*>(dc + c_la), reinterpret_cast<int32_t*>(dc + c_lb)};
  int32_t* besti = reinterpret_cast<int32_t*>(dc + c_bi);
  unsigned long long* tmin = reinterpret_cast<unsigned long long*>(dt + t_min);
  double* sxyz = reinterpret_cast<double*>(dt + t_xyz);
  uint32_t* tj = reinterpret_cast<uint32_t*>(dt + t_j);
  int32_t* sidx = reinterpret_cast<int32_t*>(dt + t_idx);
  uint32_t* cellof = reinterpret_cast<uint32_t*>(dt + t_cell);
  uint32_t* ctr = ctx->b_mu_misc.as<uint32_t>();
  double* d_box = reinterpret_cast<double*>(ctx->b_mu_misc.as<char>() + 128);
  double* d_part = reinterpret_cast<double*>(ctx->b_mu_misc.as<char>() + 192);

  vcp_phase(ctx, "matchu_grid");
  M16 m;
  for (int i = 0; i < 16; i++) m.m[i] = M[i];
  VCP_LAUNCH(ctx, k_mu_init, dim3(vcp_blocks(std::max(K, T), MT)), dim3(MT), 0, st, d_centers, K, T, m, mx, d_matched_xyz,
             d_truth_of, d_center_of, d_pair_dist, lists[0], tmin, tj);
  bool have_grid = false;
  MUScan q{};
  {
    EpsGrid g{};
    const uint32_t* cellstart = nullptr;
    VCP_TRY(eg_build_truths<MT>(ctx, d_truths, T, max_dist,
                                TruthGridWork{cellof, sxyz, sidx, d_box, d_part, &ctx->b_mu_cell}, &g, &cellstart, &have_grid));
    if (have_grid) q = MUScan{g, cellstart, sxyz, sidx, d_center_of, max_dist};
  }

  vcp_phase(ctx, "matchu_rounds");
  uint32_t nact = have_grid ? (uint32_t)K : 0u;
  int64_t pairs = 0, nrounds = 0;
  uint32_t r_abs = 0;
  uint32_t* hp = reinterpret_cast<uint32_t*>(static_cast<char*>(ctx->pinned) + 1024);
  while (nact > 0) {
    VCP_LAUNCH(ctx, k_mu_batch, dim3(1), dim3(64), 0, st, ctr, nact);
    const dim3 grid(vcp_blocks(nact, MT));
    for (int r = 0; r < BATCH; r++, r_abs++) {
      const size_t cur_set = (r_abs & 1u) * tt, nxt_set = ((r_abs + 1u) & 1u) * tt;
      const int32_t* la = lists[r_abs & 1u];
      int32_t* lb = lists[(r_abs + 1u) & 1u];
      VCP_LAUNCH(ctx, k_mu_best, grid, dim3(MT), 0, st, la, ctr + 2 * r, mx, q, tmin + cur_set, tmin + nxt_set,
                 tj + nxt_set, bestd, besti);
      VCP_LAUNCH(ctx, k_mu_name, grid, dim3(MT), 0, st, la, ctr + 2 * r, mx, q, tmin + cur_set, tj + cur_set, besti);
      VCP_LAUNCH(ctx, k_mu_accept, grid, dim3(MT), 0, st, la, ctr + 2 * r, tj + cur_set, bestd, besti, d_truth_of,
                 d_center_of, d_pair_dist, lb);
    }
    VCP_HIP(ctx, hipMemcpyAsync(hp, ctr, 2 * (BATCH + 1) * 4, hipMemcpyDeviceToHost, st));
    VCP_HIP(ctx, hipStreamSynchronize(st));
    uint32_t got = 0;
    for (int r = 0; r < BATCH; r++) {
      if (hp[2 * r + 1] > 0) nrounds++;
      got += hp[2 * r + 1];
    }
    pairs += got;
    nact = hp[2 * BATCH];
    // a free centroid with a free candidate implies a smallest remaining key, and that pair is accepted
    if (got == 0 && nact > 0) return vcp_fail(ctx, VCP_ERR_HIP, "vcp_match_unique: a round left %u centroids and accepted nothing", nact);
  }
  VCP_TRY(vcp_phase_finish(ctx));
  VCP_HIP(ctx, hipStreamSynchronize(st));
  if (count_pairs) *count_pairs = (int32_t)pairs;
  if (rounds) *rounds = (int32_t)nrounds;
  return VCP_OK;
}

int vcp_match_unique(vcp_ctx* ctx, const double* centers, int32_t K, const double* truths, int32_t T, const double M[16],
                     double max_dist, double* matched_xyz, int32_t* truth_of, int32_t* center_of, double* pair_dist,
                     int32_t* count_pairs, int32_t* rounds) {
  if (!ctx) return VCP_ERR_ARG;
  if (K < 0 || T < 0 || !M || !truth_of || !center_of) return vcp_fail(ctx, VCP_ERR_ARG, "bad argument");
  if (count_pairs) *count_pairs = 0;
  if (rounds) *rounds = 0;
  if (K == 0) {
    for (int32_t i = 0; i < T; i++) center_of[i] = -1;
    return VCP_OK;
  }
  if (T == 0) return vcp_fail(ctx, VCP_ERR_EMPTY, "no truth points (truePointCloud.GetPoint(0), FrmMain.cs:3598)");
  if (!centers || !truths) return vcp_fail(ctx, VCP_ERR_ARG, "null buffer");
  VCP_TRY(vcp_bind(ctx));
  hipStream_t st = ctx->stream;
  // device layout as in vcp_match: [centers K*24 | truths T*24] in b_in0, [xyz K*24 | dist K*8 | truth_of K*4 |
  // center_of T*4] in b_out0, one copy each way through the pinned stage
  const size_t kk = (size_t)K, tt = (size_t)T;
  const size_t in_t = kk * 24, in_bytes = in_t + tt * 24;
  const size_t o_dist = kk * 24, o_to = o_dist + kk * 8, o_co = o_to + kk * 4, out_bytes = o_co + tt * 4;
  VCP_TRY(vcp_ensure(ctx, ctx->b_in0, in_bytes));
  VCP_TRY(vcp_ensure(ctx, ctx->b_out0, out_bytes));
  char* din = ctx->b_in0.as<char>();
  char* dout = ctx->b_out0.as<char>();
  char* stage = static_cast<char*>(vcp_stage(ctx, std::max(in_bytes, out_bytes)));
  if (stage) {
    std::memcpy(stage, centers, kk * 24);
    std::memcpy(stage + in_t, truths, tt * 24);
    VCP_HIP(ctx, hipMemcpyAsync(din, stage, in_bytes, hipMemcpyHostToDevice, st));
  } else {
    VCP_HIP(ctx, hipMemcpyAsync(din, centers, kk * 24, hipMemcpyHostToDevice, st));
    VCP_HIP(ctx, hipMemcpyAsync(din + in_t, truths, tt * 24, hipMemcpyHostToDevice, st));
  }
  VCP_TRY(vcp_match_unique_dev(ctx, reinterpret_cast<const double*>(din), K, reinterpret_cast<const double*>(din + in_t), T,
                               M, max_dist, reinterpret_cast<double*>(dout), reinterpret_cast<int32_t*>(dout + o_to),
                               reinterpret_cast<int32_t*>(dout + o_co), reinterpret_cast<double*>(dout + o_dist),
                               count_pairs, rounds));
  if (stage) {
    VCP_HIP(ctx, hipMemcpyAsync(stage, dout, out_bytes, hipMemcpyDeviceToHost, st));
    VCP_HIP(ctx, hipStreamSynchronize(st));
    if (matched_xyz) std::memcpy(matched_xyz, stage, kk * 24);
    if (pair_dist) std::memcpy(pair_dist, stage + o_dist, kk * 8);
    std::memcpy(truth_of, stage + o_to, kk * 4);
    std::memcpy(center_of, stage + o_co, tt * 4);
  } else {
    if (matched_xyz) VCP_HIP(ctx, hipMemcpyAsync(matched_xyz, dout, kk * 24, hipMemcpyDeviceToHost, st));
    if (pair_dist) VCP_HIP(ctx, hipMemcpyAsync(pair_dist, dout + o_dist, kk * 8, hipMemcpyDeviceToHost, st));
    VCP_HIP(ctx, hipMemcpyAsync(truth_of, dout + o_to, kk * 4, hipMemcpyDeviceToHost, st));
    VCP_HIP(ctx, hipMemcpyAsync(center_of, dout + o_co, tt * 4, hipMemcpyDeviceToHost, st));
    VCP_HIP(ctx, hipStreamSynchronize(st));
  }
  return VCP_OK;
}

}  // extern "C"
