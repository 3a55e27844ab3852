// eps_tree.hip -- vcp_eps_tree: what DBSCAN(min_pts = k) decides at EVERY eps <= eps_max, in one call (include/vcp.h,
// DESIGN.md section 17).
//
// Definition.  kdist is vcp_kdist's.  P = { i : kdist[i] <= eps_max }, E = { (i, j) : i < j, both in P, d(i, j) <= eps_max },
// w(i, j) = max(kdist[i], kdist[j], d(i, j)) (a selection), edges ordered by the key (w, i, j).  The result is the minimum
// spanning forest of (P, E) under that strict total order: the edges a Kruskal walk in ascending key order accepts
// (tests/eps_tree_ref.py restates the walk; results are compared bit for bit).  reach[i] = min over j in P with
// d(i, j) <= eps_max of max(kdist[j], d(i, j)).
//
// The device reaches the forest by Boruvka rounds over a component array.  Under a strict total order the minimum edge
// leaving a component belongs to the forest (cut property), so every round only adds forest edges, and the only cycle the
// picks of a round can close is two components picking the SAME edge, which is emitted once.
//
// Candidates come from epsgrid.hpp's grid over the finite points for eps_max: all of E lies in the 3^dim cells around a
// point.  The points are put in cell order as records (x, y, z or 0, kdist) plus the original index; all per-vertex
// state is indexed by that slot.  Every reader takes a minimum over a cell, whatever the order inside it.
//
// A round, over the slots of P that are not yet interior:
//   k_et_best   the slot scans its cells for the minimum key (w, lo, hi) among edges to another component, keeps it and
//               lowers its component's word cw to the bits of w (a non-negative double orders like its bits).  A slot
//               without such an edge is INTERIOR for good (components only grow) and never scans again; one whose
//               best edge of the round before still leaves its component keeps it without a scan
//   k_et_name   a slot whose w equals its component's word lowers the component's second word ce to lo << 32 | hi
//   k_et_hook   the one slot per component that holds (cw, ce) hooks its component onto the other end's -- unless the
//               other component picked the same edge and has the larger root: then only that one hooks -- and emits
//   k_et_flat   every slot follows the hooks to its new root (compressing the path) and clears its words
// The slots of a cell whose 3^dim cells hold more than HEAVY points are left to k_et_best_heavy / k_et_reach_heavy: a wave
// per chunk of 64 slots of the cell, which share their candidate rows, or a wave per slot where the chunk is small.
// Only integer min-atomics decide anything.  One counter read-back per round; the rounds stop when the forest is
// spanning or a round emits nothing.  The emitted edges are sorted by (lo, hi), then stably by w.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "bounds.hpp"
#include "epsgrid.hpp"
#include "sort.hpp"
#include "vcp_ctx.hpp"
#include "wave.hpp"

namespace {
constexpr int ET = 256;  // threads per workgroup
constexpr unsigned long long NOKEY = ~0ull;
constexpr uint8_t F_P = 1, F_INTERIOR = 2, F_HEAVY = 4;
enum { C_EMIT = 0, C_P = 1, C_HEAVY = 2, C_ERR = 3, C_WORDS = 4 };

// the finite points: records (x, y, z or 0, kdist) and the original index; a non-finite point gets its reach here
template <int GD>
struct ETSrc {
  const double* c;
  int stride;
  const double* kdist;
  double* reach;  // may be null
  double4* rec;
  int32_t* sidx;
  __device__ void load(int64_t i, double* q) const { load_pt<GD>(c, i, stride, q); }
  __device__ bool in_grid(int64_t, const double* q) const { return eg_finite(q); }
  __device__ void outside(int64_t i) const {
    if (reach) reach[i] = NAN;
  }
  __device__ void store(uint32_t s, int64_t i, const double* q) const {
    rec[s] = make_double4(q[0], q[1], q[2], kdist[i]);
    sidx[s] = (int32_t)i;
  }
};

struct ETArgs : EpsCells {  // rec: [nf] records
  const int32_t* sidx;  // [nf] original index of a slot
  double eps_max;
  uint32_t nf;
  uint8_t* flags;       // [nf] F_P | F_INTERIOR | F_HEAVY
  uint32_t* comp;       // [nf] root slot of the slot's component (flat between rounds)
  uint32_t* par;        // [nf] hooks: par[root] = the root it was hooked onto
  unsigned long long* bw;  // [nf] the slot's best w (bits), NOKEY = none
  unsigned long long* be;  // [nf] its lo << 32 | hi
  uint32_t* bt;            // [nf] the slot at the other end
  unsigned long long* cw;  // [nf] per root: least w leaving the component
  unsigned long long* ce;  // [nf] per root: least lo << 32 | hi among the edges with that w
  uint32_t* heavy;         // [nf] first slot of every heavy chunk
  uint32_t* ctr;           // C_WORDS counters
  unsigned long long* ew;  // [cap] emitted edges
  unsigned long long* ee;
  uint32_t cap;
};

// components, words and flags of every slot; |P| and the list of heavy chunks (<= 64 consecutive slots of one heavy cell)
__global__ __launch_bounds__(ET) void k_et_init(ETArgs a) {
  const uint32_t s = blockIdx.x * ET + threadIdx.x;
  const int lane = threadIdx.x & 63;
  bool inp = false, hv = false;
  if (s < a.nf) {
    const double4 q = a.rec[s];
    inp = q.w <= a.eps_max;
    const bool heavy_cell = eg_heavy_cell(a, q);
    a.flags[s] = (uint8_t)((inp ? F_P : 0) | (heavy_cell ? F_HEAVY : 0));
    hv = heavy_cell && eg_chunk_first(a, q, s);
    a.comp[s] = s;
    a.par[s] = s;
    a.bw[s] = NOKEY;
    a.cw[s] = NOKEY;
    a.ce[s] = NOKEY;
  }
  const uint32_t np = wave_count(inp);
  if (np && lane == 0) atomicAdd(&a.ctr[C_P], np);
  eg_list_chunks(hv, s, a.heavy, &a.ctr[C_HEAVY]);
}

struct Best {
  unsigned long long w, e;
  uint32_t t;
};

// the minimum key among the edges of slot s that leave its component; lane `off` of `step` takes every step-th candidate
template <int METRIC>
__device__ __forceinline__ Best et_best(const ETArgs& a, uint32_t s, const double4& q, uint32_t off, uint32_t step) {
  Best b{NOKEY, NOKEY, 0u};
  const uint32_t cs = a.comp[s];
  const uint32_t qi = (uint32_t)a.sidx[s];
  eg_walk(
      a, q, off, step, [&](uint32_t t) { return a.comp[t] != cs; },  // 4 bytes decide it for most candidates of the later rounds
      [&](uint32_t t, const double4& r) {
        if (!(r.w <= a.eps_max)) return;
        const double d = dist<METRIC>(q, r);
        if (!(d <= a.eps_max)) return;
        const unsigned long long w = (unsigned long long)__double_as_longlong(fmax(fmax(q.w, r.w), d));
        if (w > b.w) return;
        const uint32_t j = (uint32_t)a.sidx[t];
        const unsigned long long e = ((unsigned long long)min(qi, j) << 32) | max(qi, j);
        if (w < b.w || e < b.e) b = Best{w, e, t};
      });
  return b;
}

// The candidates of a slot only ever shrink (components grow, E is fixed), so last round's best edge is still the best as
// long as it still leaves the component: only a slot whose best neighbour has joined it scans again.
__device__ __forceinline__ bool et_still_best(const ETArgs& a, uint32_t s) {
  return a.bw[s] != NOKEY && a.comp[a.bt[s]] != a.comp[s];
}

__device__ __forceinline__ void et_keep(const ETArgs& a, uint32_t s, const Best& b) {
  a.bw[s] = b.w;
  if (b.w == NOKEY) {
    a.flags[s] |= F_INTERIOR;
    return;
  }
  a.be[s] = b.e;
  a.bt[s] = b.t;
  unsigned long long* word = &a.cw[a.comp[s]];
  if (b.w < __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(word, b.w);
}

template <int METRIC>
__global__ __launch_bounds__(ET) void k_et_best(ETArgs a) {
  const uint32_t s = blockIdx.x * ET + threadIdx.x;
  if (s >= a.nf || a.flags[s] != F_P) return;  // not in P, interior or heavy
  if (et_still_best(a, s))
    et_keep(a, s, Best{a.bw[s], a.be[s], a.bt[s]});
  else
    et_keep(a, s, et_best<METRIC>(a, s, a.rec[s], 0u, 1u));
}

template <int METRIC>
__global__ __launch_bounds__(64) void k_et_best_heavy(ETArgs a, uint32_t nheavy) {
  eg_heavy(
      a, a.heavy, nheavy,
      [&](uint32_t s) {
        if (a.flags[s] != (F_P | F_HEAVY)) return;
        if (et_still_best(a, s))
          et_keep(a, s, Best{a.bw[s], a.be[s], a.bt[s]});
        else
          et_keep(a, s, et_best<METRIC>(a, s, a.rec[s], 0u, 1u));
      },
      [&](uint32_t s, uint32_t lane) {
        if (a.flags[s] != (F_P | F_HEAVY)) return;  // wave-uniform
        if (et_still_best(a, s)) {
          if (lane == 0) et_keep(a, s, Best{a.bw[s], a.be[s], a.bt[s]});
          return;
        }
        Best b = et_best<METRIC>(a, s, a.rec[s], lane, 64u);
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
          const unsigned long long ow = __shfl_xor(b.w, d, 64), oe = __shfl_xor(b.e, d, 64);
          const uint32_t ot = (uint32_t)__shfl_xor((int)b.t, d, 64);
          if (ow < b.w || (ow == b.w && oe < b.e)) b = Best{ow, oe, ot};
        }
        if (lane == 0) et_keep(a, s, b);
      });
}

__global__ __launch_bounds__(ET) void k_et_name(ETArgs a) {
  const uint32_t s = blockIdx.x * ET + threadIdx.x;
  if (s >= a.nf || (a.flags[s] & (F_P | F_INTERIOR)) != F_P) return;
  const unsigned long long w = a.bw[s];
  const uint32_t cs = a.comp[s];
  if (w != a.cw[cs]) return;
  const unsigned long long e = a.be[s];
  if (e < __hip_atomic_load(&a.ce[cs], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&a.ce[cs], e);
}

__global__ __launch_bounds__(ET) void k_et_hook(ETArgs a) {
  const uint32_t s = blockIdx.x * ET + threadIdx.x;
  if (s >= a.nf || (a.flags[s] & (F_P | F_INTERIOR)) != F_P) return;
  const unsigned long long w = a.bw[s], e = a.be[s];
  const uint32_t cs = a.comp[s];
  if (w != a.cw[cs] || e != a.ce[cs]) return;  // one slot per component gets past this: the edge's end inside it
  const uint32_t co = a.comp[a.bt[s]];
  if (a.cw[co] == w && a.ce[co] == e && cs < co) return;  // the same edge from both sides: the larger root hooks
  a.par[cs] = co;
  const uint32_t at = atomicAdd(&a.ctr[C_EMIT], 1u);
  if (at < a.cap) {
    a.ew[at] = w;
    a.ee[at] = e;
  } else {
    a.ctr[C_ERR] = 1u;
  }
}

__global__ __launch_bounds__(ET) void k_et_flat(ETArgs a) {
  const uint32_t s = blockIdx.x * ET + threadIdx.x;
  if (s >= a.nf || !(a.flags[s] & F_P)) return;
  const uint32_t first = a.comp[s];
  uint32_t root = first, steps = 0;
  for (uint32_t p; (p = a.par[root]) != root; root = p)
    if (++steps > a.nf) {  // no chain of hooks is longer than the number of components
      a.ctr[C_ERR] = 2u;
      break;
    }
  // path compression: whatever another slot writes here at the same time is an ancestor too
  for (uint32_t x = first, i = 1; i < steps && x != root; i++) {
    const uint32_t nx = a.par[x];
    a.par[x] = root;
    x = nx;
  }
  a.comp[s] = root;
  a.cw[s] = NOKEY;
  a.ce[s] = NOKEY;
}

template <int METRIC>
__device__ __forceinline__ double et_reach(const ETArgs& a, const double4& q, uint32_t off, uint32_t step) {
  double best = INFINITY;
  eg_walk(
      a, q, off, step, [](uint32_t) { return true; },
      [&](uint32_t, const double4& r) {
        if (!(r.w <= a.eps_max)) return;
        const double d = dist<METRIC>(q, r);
        if (!(d <= a.eps_max)) return;
        best = fmin(best, fmax(r.w, d));
      });
  return best;
}

template <int METRIC>
__global__ __launch_bounds__(ET) void k_et_reach(ETArgs a, double* __restrict__ reach) {
  const uint32_t s = blockIdx.x * ET + threadIdx.x;
  if (s >= a.nf || (a.flags[s] & F_HEAVY)) return;
  reach[a.sidx[s]] = et_reach<METRIC>(a, a.rec[s], 0u, 1u);
}

template <int METRIC>
__global__ __launch_bounds__(64) void k_et_reach_heavy(ETArgs a, uint32_t nheavy, double* __restrict__ reach) {
  eg_heavy(
      a, a.heavy, nheavy, [&](uint32_t s) { reach[a.sidx[s]] = et_reach<METRIC>(a, a.rec[s], 0u, 1u); },
      [&](uint32_t s, uint32_t lane) {
        double b = et_reach<METRIC>(a, a.rec[s], lane, 64u);
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) b = fmin(b, __shfl_xor(b, d, 64));
        if (lane == 0) reach[a.sidx[s]] = b;
      });
}

// the sorted edges into the caller's arrays
__global__ __launch_bounds__(ET) void k_et_out(const unsigned long long* __restrict__ w,
                                               const unsigned long long* __restrict__ e, uint32_t m,
                                               double* __restrict__ merge_w, int32_t* __restrict__ merge_a,
                                               int32_t* __restrict__ merge_b) {
  const uint32_t t = blockIdx.x * ET + threadIdx.x;
  if (t >= m) return;
  merge_w[t] = __longlong_as_double((long long)w[t]);
  if (merge_a) {
    merge_a[t] = (int32_t)(e[t] >> 32);
    merge_b[t] = (int32_t)(e[t] & 0xFFFFFFFFull);
  }
}

template <int METRIC>
int run_rounds(vcp_ctx* ctx, const ETArgs& a, uint32_t np, uint32_t nheavy, uint32_t* hp, uint32_t* emitted,
               int32_t* nrounds) {
  hipStream_t st = ctx->stream;
  const dim3 grid(vcp_blocks(a.nf, ET));
  const dim3 hgrid(vcp_blocks(nheavy, 1, 65536));
  uint32_t have = 0;
  int32_t rounds = 0;
  // a tree that accepts an edge in round r has at least 2^(r-1) vertices: 32 rounds cover every n < 2^31
  for (int r = 0; r < 33 && np >= 2 && have + 1 < np; r++) {
    VCP_LAUNCH(ctx, (k_et_best<METRIC>), grid, dim3(ET), 0, st, a);
    if (nheavy) VCP_LAUNCH(ctx, (k_et_best_heavy<METRIC>), hgrid, dim3(64), 0, st, a, nheavy);
    VCP_LAUNCH(ctx, k_et_name, grid, dim3(ET), 0, st, a);
    VCP_LAUNCH(ctx, k_et_hook, grid, dim3(ET), 0, st, a);
    VCP_LAUNCH(ctx, k_et_flat, grid, dim3(ET), 0, st, a);
    VCP_HIP(ctx, hipMemcpyAsync(hp, a.ctr, C_WORDS * 4, hipMemcpyDeviceToHost, st));
    VCP_HIP(ctx, hipStreamSynchronize(st));
    if (hp[C_ERR]) return vcp_fail(ctx, VCP_ERR_HIP, "vcp_eps_tree: the forest is inconsistent (code %u)", hp[C_ERR]);
    if (hp[C_EMIT] == have) break;
    have = hp[C_EMIT];
    rounds++;
  }
  *emitted = have;
  *nrounds = rounds;
  return VCP_OK;
}

template <int GD, int METRIC>
int run_eps_tree(vcp_ctx* ctx, const double* d_coords, int64_t n, int stride, double eps_max, const double* d_kd,
                 double* d_reach, int64_t* n_merge, double* d_merge_w, int32_t* d_merge_a, int32_t* d_merge_b,
                 int32_t* rounds_out) {
  hipStream_t st = ctx->stream;

  // 1. the grid over the finite points and the records in cell order
  vcp_phase(ctx, "epst_grid");
  const int rb = vcp_bounds_parts(n);
  // [counters 64 | bounds 64 | bounds partials]
  VCP_TRY(vcp_ensure(ctx, ctx->b_et_misc, 128 + (size_t)rb * 64));
  uint32_t* ctr = ctx->b_et_misc.as<uint32_t>();
  double* d_box = reinterpret_cast<double*>(ctx->b_et_misc.as<char>() + 64);
  double* d_part = reinterpret_cast<double*>(ctx->b_et_misc.as<char>() + 128);
  double* hb = reinterpret_cast<double*>(ctx->pinned);
  VCP_TRY(vcp_bounds(ctx, BoundsSrc{d_coords, n, GD, stride}, d_part, d_box, hb));
  double lo[3] = {hb[0], hb[1], hb[2]}, hi[3] = {hb[3], hb[4], hb[5]};
  const uint32_t nf = (uint32_t)(n - (int64_t)hb[6]);
  for (int t = GD; t < 3; t++) lo[t] = hi[t] = 0.0;
  if (nf == 0) lo[0] = lo[1] = lo[2] = hi[0] = hi[1] = hi[2] = 0.0;
  for (int t = 0; t < GD; t++)
    if (!std::isfinite(hi[t] - lo[t]))
      return vcp_fail(ctx, VCP_ERR_UNSUPPORTED, "the cloud's extent overflows binary64 (coordinate differences are infinite)");
  // per point: [rec 32 | bw 8 | be 8 | cw 8 | ce 8 | cellof 4 | sidx 4 | comp 4 | par 4 | bt 4 | heavy 4 | flags 1]
  const size_t nn = (size_t)n;
  const size_t o_bw = nn * 32, o_be = o_bw + nn * 8, o_cw = o_be + nn * 8, o_ce = o_cw + nn * 8, o_cell = o_ce + nn * 8,
               o_sidx = o_cell + nn * 4, o_comp = o_sidx + nn * 4, o_par = o_comp + nn * 4, o_bt = o_par + nn * 4,
               o_heavy = o_bt + nn * 4, o_flags = o_heavy + nn * 4;
  VCP_TRY(vcp_ensure(ctx, ctx->b_et_work, o_flags + nn));
  char* dw = ctx->b_et_work.as<char>();
  // the emitted edges and the sort's second set: 4 x [cap] words
  const size_t cap = nn > 1 ? nn - 1 : 1;
  VCP_TRY(vcp_ensure(ctx, ctx->b_et_edge, cap * 32));
  unsigned long long* ed = ctx->b_et_edge.as<unsigned long long>();
  uint32_t* cellof = reinterpret_cast<uint32_t*>(dw + o_cell);
  double4* rec = reinterpret_cast<double4*>(dw);
  int32_t* sidx = reinterpret_cast<int32_t*>(dw + o_sidx);

  VCP_HIP(ctx, hipMemsetAsync(ctr, 0, 64, st));
  const EpsGrid g = eg_plan(lo, hi, eps_max);
  const uint32_t* cellstart = nullptr;
  VCP_TRY(eg_bin<ET>(ctx, ETSrc<GD>{d_coords, stride, d_kd, d_reach, rec, sidx}, n, g, cellof, ctx->b_et_cell, &cellstart));

  ETArgs a{};
  a.g = g;
  a.cellstart = cellstart;
  a.rec = rec;
  a.sidx = sidx;
  a.eps_max = eps_max;
  a.nf = nf;
  a.flags = reinterpret_cast<uint8_t*>(dw + o_flags);
  a.comp = reinterpret_cast<uint32_t*>(dw + o_comp);
  a.par = reinterpret_cast<uint32_t*>(dw + o_par);
  a.bw = reinterpret_cast<unsigned long long*>(dw + o_bw);
  a.be = reinterpret_cast<unsigned long long*>(dw + o_be);
  a.bt = reinterpret_cast<uint32_t*>(dw + o_bt);
  a.cw = reinterpret_cast<unsigned long long*>(dw + o_cw);
  a.ce = reinterpret_cast<unsigned long long*>(dw + o_ce);
  a.heavy = reinterpret_cast<uint32_t*>(dw + o_heavy);
  a.ctr = ctr;
  a.ew = ed;
  a.ee = ed + cap;
  a.cap = (uint32_t)cap;
  uint32_t* hp = reinterpret_cast<uint32_t*>(static_cast<char*>(ctx->pinned) + 1024);
  uint32_t np = 0, nheavy = 0;
  if (nf > 0) {
    VCP_LAUNCH(ctx, k_et_init, dim3(vcp_blocks(nf, ET)), dim3(ET), 0, st, a);
    VCP_HIP(ctx, hipMemcpyAsync(hp, ctr, C_WORDS * 4, hipMemcpyDeviceToHost, st));
    VCP_HIP(ctx, hipStreamSynchronize(st));
    np = hp[C_P];
    nheavy = hp[C_HEAVY];
  }

  // 2. the forest
  vcp_phase(ctx, "epst_rounds");
  uint32_t m = 0;
  int32_t rounds = 0;
  VCP_TRY(run_rounds<METRIC>(ctx, a, np, nheavy, hp, &m, &rounds));

  // 3. reach
  vcp_phase(ctx, "epst_reach");
  if (d_reach && nf > 0) {
    VCP_LAUNCH(ctx, (k_et_reach<METRIC>), dim3(vcp_blocks(nf, ET)), dim3(ET), 0, st, a, d_reach);
    if (nheavy)
      VCP_LAUNCH(ctx, (k_et_reach_heavy<METRIC>), dim3(vcp_blocks(nheavy, 1, 65536)), dim3(64), 0, st, a, nheavy, d_reach);
  }

  // 4. the edges in key order: by lo << 32 | hi, then stably by w
  vcp_phase(ctx, "epst_sort");
  if (m > 0) {
    unsigned long long* w2 = ed + 2 * cap;
    unsigned long long* e2 = ed + 3 * cap;
    VCP_TRY(vcp_sort_pairs(ctx, ctx->b_et_tmp, a.ee, e2, a.ew, w2, (size_t)m, 64));
    VCP_TRY(vcp_sort_pairs(ctx, ctx->b_et_tmp, w2, a.ew, e2, a.ee, (size_t)m, 64));
    VCP_LAUNCH(ctx, k_et_out, dim3(vcp_blocks(m, ET)), dim3(ET), 0, st, a.ew, a.ee, m, d_merge_w, d_merge_a, d_merge_b);
  }
  VCP_TRY(vcp_phase_finish(ctx));
  VCP_HIP(ctx, hipStreamSynchronize(st));
  *n_merge = (int64_t)m;
  if (rounds_out) *rounds_out = rounds;
  return VCP_OK;
}

// the argument errors of both forms (pointers apart); VCP_OK when the call can go on
int check_args(vcp_ctx* ctx, int64_t n, int dim, int metric, int k, double eps_max) {
  if (n < 0) return vcp_fail(ctx, VCP_ERR_ARG, "n < 0");
  if (dim != 2 && dim != 3) return vcp_fail(ctx, VCP_ERR_ARG, "dim must be 2 or 3");
  if (metric != VCP_L1_2D && metric != VCP_L2_2D && metric != VCP_L2_3D)
    return vcp_fail(ctx, VCP_ERR_ARG, "vcp_eps_tree takes VCP_L1_2D, VCP_L2_2D or VCP_L2_3D (metric %d)", metric);
  if (metric == VCP_L2_3D && dim != 3) return vcp_fail(ctx, VCP_ERR_ARG, "VCP_L2_3D needs dim 3");
  if (k < 1) return vcp_fail(ctx, VCP_ERR_ARG, "k < 1");
  if (!(eps_max > 0.0) || !std::isfinite(eps_max)) return vcp_fail(ctx, VCP_ERR_ARG, "eps_max must be finite and > 0");
  if (k > 64) return vcp_fail(ctx, VCP_ERR_UNSUPPORTED, "k > 64");
  if (n >= ((int64_t)1 << 31)) return vcp_fail(ctx, VCP_ERR_TOO_LARGE, "n beyond int32 indices");
  return VCP_OK;
}
}  // namespace

extern "C" {

int vcp_eps_tree_dev(vcp_ctx* ctx, const double* d_coords, int64_t n, int dim, int metric, int k, double eps_max,
                     int kdist_given, double* d_kdist, double* d_reach, int64_t* n_merge, double* d_merge_w,
                     int32_t* d_merge_a, int32_t* d_merge_b, int32_t* rounds) {
  if (!ctx) return VCP_ERR_ARG;
  if (!n_merge || !d_merge_w || (!d_merge_a) != (!d_merge_b) || (kdist_given && !d_kdist))
    return vcp_fail(ctx, VCP_ERR_ARG, "bad argument");
  VCP_TRY(check_args(ctx, n, dim, metric, k, eps_max));
  if (n > 0 && !d_coords) return vcp_fail(ctx, VCP_ERR_ARG, "null buffer");
  VCP_TRY(vcp_bind(ctx));
  vcp_phase_reset(ctx);
  if (n == 0) {
    ctx->last_timing.clear();
    *n_merge = 0;
    if (rounds) *rounds = 0;
    return VCP_OK;
  }
  float kd_ms = 0.f;
  if (!kdist_given) {
    if (!d_kdist) {
      VCP_TRY(vcp_ensure(ctx, ctx->b_et_kd, (size_t)n * 8));
      d_kdist = ctx->b_et_kd.as<double>();
    }
    VCP_TRY(vcp_kdist_dev(ctx, d_coords, n, dim, metric, k, d_kdist, nullptr));
    for (const auto& p : ctx->last_timing) kd_ms += p.second;
    vcp_phase_reset(ctx);
  }
  int rc;
  if (metric == VCP_L1_2D)
    rc = run_eps_tree<2, VCP_L1_2D>(ctx, d_coords, n, dim, eps_max, d_kdist, d_reach, n_merge, d_merge_w, d_merge_a,
                                    d_merge_b, rounds);
  else if (metric == VCP_L2_2D)
    rc = run_eps_tree<2, VCP_L2_2D>(ctx, d_coords, n, dim, eps_max, d_kdist, d_reach, n_merge, d_merge_w, d_merge_a,
                                    d_merge_b, rounds);
  else
    rc = run_eps_tree<3, VCP_L2_3D>(ctx, d_coords, n, dim, eps_max, d_kdist, d_reach, n_merge, d_merge_w, d_merge_a,
                                    d_merge_b, rounds);
  if (rc == VCP_OK && ctx->timing && !kdist_given) ctx->last_timing.insert(ctx->last_timing.begin(), {"epst_kdist", kd_ms});
  return rc;
}

int vcp_eps_tree(vcp_ctx* ctx, const double* coords, int64_t n, int dim, int metric, int k, double eps_max,
                 int kdist_given, double* kdist, double* reach, int64_t* n_merge, double* merge_w, int32_t* merge_a,
                 int32_t* merge_b, int32_t* rounds) {
  if (!ctx) return VCP_ERR_ARG;
  if (!n_merge || !merge_w || (!merge_a) != (!merge_b) || (kdist_given && !kdist))
    return vcp_fail(ctx, VCP_ERR_ARG, "bad argument");
  VCP_TRY(check_args(ctx, n, dim, metric, k, eps_max));
  if (n > 0 && !coords) return vcp_fail(ctx, VCP_ERR_ARG, "null buffer");
  if (n == 0)  // no copies: the device form's answer
    return vcp_eps_tree_dev(ctx, nullptr, 0, dim, metric, k, eps_max, 0, nullptr, nullptr, n_merge, merge_w, nullptr,
                            nullptr, rounds);
  VCP_TRY(vcp_bind(ctx));
  hipStream_t st = ctx->stream;
  // in: [coords n*dim*8 | kdist n*8]; out: [reach n*8 | merge_w cap*8 | merge_a cap*4 | merge_b cap*4]
  const size_t nn = (size_t)n, cap = nn - 1;
  const size_t i_kd = nn * dim * 8;
  const size_t o_w = nn * 8, o_a = o_w + cap * 8, o_b = o_a + cap * 4;
  VCP_TRY(vcp_ensure(ctx, ctx->b_et_in, i_kd + nn * 8));
  VCP_TRY(vcp_ensure(ctx, ctx->b_et_out, o_b + cap * 4 + 16));
  char* din = ctx->b_et_in.as<char>();
  char* dout = ctx->b_et_out.as<char>();
  double* dkd = reinterpret_cast<double*>(din + i_kd);
  VCP_HIP(ctx, hipMemcpyAsync(din, coords, i_kd, hipMemcpyHostToDevice, st));
  if (kdist_given) VCP_HIP(ctx, hipMemcpyAsync(dkd, kdist, nn * 8, hipMemcpyHostToDevice, st));
  int64_t m = 0;
  int32_t r = 0;
  VCP_TRY(vcp_eps_tree_dev(ctx, reinterpret_cast<const double*>(din), n, dim, metric, k, eps_max, kdist_given, dkd,
                           reach ? reinterpret_cast<double*>(dout) : nullptr, &m, reinterpret_cast<double*>(dout + o_w),
                           merge_a ? reinterpret_cast<int32_t*>(dout + o_a) : nullptr,
                           merge_a ? reinterpret_cast<int32_t*>(dout + o_b) : nullptr, &r));
  if (kdist && !kdist_given) VCP_HIP(ctx, hipMemcpyAsync(kdist, dkd, nn * 8, hipMemcpyDeviceToHost, st));
  if (reach) VCP_HIP(ctx, hipMemcpyAsync(reach, dout, nn * 8, hipMemcpyDeviceToHost, st));
  if (m > 0) {
    VCP_HIP(ctx, hipMemcpyAsync(merge_w, dout + o_w, (size_t)m * 8, hipMemcpyDeviceToHost, st));
    if (merge_a) {
      VCP_HIP(ctx, hipMemcpyAsync(merge_a, dout + o_a, (size_t)m * 4, hipMemcpyDeviceToHost, st));
      VCP_HIP(ctx, hipMemcpyAsync(merge_b, dout + o_b, (size_t)m * 4, hipMemcpyDeviceToHost, st));
    }
  }
  VCP_HIP(ctx, hipStreamSynchronize(st));
  *n_merge = m;
  if (rounds) *rounds = r;
  return VCP_OK;
}

}  // extern "C"
