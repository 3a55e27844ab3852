// gdbscan.hip -- vcp_gdbscan: DBSCAN with point weights and a range gate (include/vcp.h).
//
// Definition.  d(i, j) is vcp_kdist's.  N(i) = { j : d(i, j) <= eps and |aux[i] - aux[j]| <= gate } (the second test only
// when aux is given; j = i included; a row with a non-finite coordinate or aux has an empty N and is in nobody's),
// W(i) = sum of w[j] over N(i) in int64, core[i] <=> W(i) >= min_weight.  Clusters are the connected components of the core
// points under j in N(i), numbered cf_in + 1, ... by increasing smallest member index; a non-core point takes the LARGEST
// id among the core points of its N, else 0.  tests/gdbscan_ref.py restates this in numpy; results are compared for
// equality.
//
// The DBSCAN engine (dbscan.hip) is specialised to a count of rows with an early exit at min_pts and is not touched: this
// is a translation unit of its own, in the manner of kdist.hip and eps_tree.hip, and it walks the neighbourhood three times
// (count, union, border) where the engine walks once and keeps lists.
//
// Candidates come from epsgrid.hpp's grid over the finite points for eps, ON THE COORDINATES ONLY (aux is a filter, not an
// axis): all of N(i) lies in the 3^dim cells around i.  The points are put in cell order as 32-byte records (x, y, z or
// 0, aux or 0) plus (weight, original index); all per-point state is indexed by that slot.  Nothing below depends on the
// order inside a cell: W is an integer sum, the components are sets, they are numbered by their smallest ORIGINAL index
// and a border point takes a maximum.
//
//   k_gd_weights   any weight < 0 raises a counter word, read back with the bounds: nothing else has run by then
//   eg_bin (k_eg_cell, scan, k_eg_fill), k_gd_init   the grid, the records, the per-slot state, the list of heavy chunks
//   k_gd_count     W and the core flag of every slot (stops at min_weight when the caller does not want W)
//   k_gd_union     every core slot hooks itself to the core slots of its N with a smaller slot number: the larger root
//                  under the smaller by compare-and-swap, so par[x] <= x always and no cycle can form.  par is read with
//                  agent-scope atomic loads inside this launch: a plain load may be served from this CU's L1, which
//                  another workgroup's store never refreshes, and a retry loop on a stale word would not end
//   k_gd_flat      (a launch of its own: par is final) root of every core slot; the root's smallest original index by
//                  integer min-atomic
//   k_gd_first     a flag at that index; one exclusive scan over the n + 1 flags ranks the clusters
//   k_gd_label     id = rank + cf_in + 1 for the core slots; the rows outside the grid (0, or a cluster each when
//                  min_weight <= 0, as the literal C# does)
//   k_gd_border    the largest id among the core slots of N for every non-core slot
// The slots of a cell whose 3^dim cells hold more than HEAVY points are left to the *_heavy form of the three walks: a wave
// per chunk of 64 slots of the cell, which share their candidate rows, or a wave per slot where the chunk is small; a lane
// never walks a blob's rows alone.  The heavy kernels read the number of chunks on the device, so the call reads back
// twice: the bounds with the weight check, and the cluster count.  Only integer atomics decide anything.
#include <climits>
#include <cmath>
#include <cstring>

#include "bounds.hpp"
#include "epsgrid.hpp"
#include "vcp_ctx.hpp"
#include "wave.hpp"

namespace {
constexpr int GT = 256;  // threads per workgroup
constexpr uint32_t NOIDX = 0xFFFFFFFFu;
constexpr uint8_t F_CORE = 1, F_HEAVY = 2;
enum { C_NEG = 0, C_HEAVY = 1 };  // counter words (64 bytes of them)

// a weight < 0 anywhere raises the counter word
__global__ __launch_bounds__(GT) void k_gd_weights(const int32_t* __restrict__ w, int64_t n, uint32_t* __restrict__ ctr) {
  const int64_t i = (int64_t)blockIdx.x * GT + threadIdx.x;
  const bool neg = i < n && w[i] < 0;
  if (__ballot(neg) && (threadIdx.x & 63) == 0) atomicOr(&ctr[C_NEG], 1u);
}

// the rows with finite coordinates and aux: records (x, y, z or 0, aux or 0) and (weight or 1, original index); with
// min_weight <= 0 a row outside the grid is a cluster of its own: its flag for the ranking
template <int GD>
struct GDSrc {
  const double* c;
  int stride;
  const double* aux;  // may be null
  const int32_t* w;   // may be null
  int alone;
  uint32_t* rank;
  double4* rec;
  int2* wi;
  __device__ void load(int64_t i, double* q) const { load_pt<GD>(c, i, stride, q); }
  __device__ bool in_grid(int64_t i, const double* q) const { return eg_finite(q) && (!aux || isfinite(aux[i])); }
  __device__ void outside(int64_t i) const {
    if (alone) rank[i] = 1u;
  }
  __device__ void store(uint32_t s, int64_t i, const double* q) const {
    rec[s] = make_double4(q[0], q[1], q[2], aux ? aux[i] : 0.0);
    wi[s] = make_int2(w ? w[i] : 1, (int)i);
  }
};

struct GDArgs : EpsCells {     // cellstart: [nc + 1], cellstart[nc] = the number of slots nf; rec: [nf]
  const int2* wi;             // [nf] (weight, original index) of a slot
  double eps, gate;           // gate 0 without aux: the records' fourth word is 0 then
  int64_t min_weight;
  uint32_t nc;
  int none;                   // eps NaN or < 0: every N is empty
  int weighted;               // 0: every weight is 1
  int exact;                  // the caller wants W: no early exit
  int32_t cf_in;
  uint8_t* flags;             // [nf] F_CORE | F_HEAVY
  uint32_t* par;              // [nf] hooks: par[x] <= x
  uint32_t* comp;             // [nf] root of a core slot
  uint32_t* minidx;           // [nf] per root: smallest original index of the component
  uint32_t* cid;              // [nf] cluster id of a core slot
  uint32_t* heavy;            // [nf] first slot of every heavy chunk
  uint32_t* ctr;
  uint32_t* rank;             // [n + 1] first-member flags, then their exclusive scan
  int32_t* labels;            // the caller's, by original index
  uint8_t* is_core;           // may be null
  long long* wsum;            // may be null
};

__device__ __forceinline__ uint32_t gd_nf(const GDArgs& a) { return a.cellstart[a.nc]; }

template <int METRIC>
__device__ __forceinline__ bool near(const GDArgs& a, const double4& q, const double4& r) {
  return dist<METRIC>(q, r) <= a.eps && fabs(q.w - r.w) <= a.gate;
}

// eg_walk; eps NaN or < 0 (a.none): nobody has a candidate
template <class Want, class Use>
__device__ __forceinline__ void gd_walk(const GDArgs& a, const double4& q, uint32_t off, uint32_t step, Want&& want,
                                        Use&& use) {
  if (!a.none) eg_walk(a, q, off, step, want, use);
}

// hooks and flags of every slot; the list of heavy chunks (<= 64 consecutive slots of one heavy cell)
__global__ __launch_bounds__(GT) void k_gd_init(GDArgs a) {
  const uint32_t s = blockIdx.x * GT + threadIdx.x;
  bool hv = false;
  if (s < gd_nf(a)) {
    const double4 q = a.rec[s];
    const bool heavy_cell = !a.none && eg_heavy_cell(a, q);
    a.flags[s] = heavy_cell ? F_HEAVY : 0;
    hv = heavy_cell && eg_chunk_first(a, q, s);
    a.par[s] = s;
    a.minidx[s] = NOIDX;
  }
  eg_list_chunks(hv, s, a.heavy, &a.ctr[C_HEAVY]);
}

// ---- count ------------------------------------------------------------------------------------------------------------
template <int METRIC>
__device__ __forceinline__ long long gd_count(const GDArgs& a, const double4& q, uint32_t off, uint32_t step, bool early) {
  long long W = 0;
  gd_walk(
      a, q, off, step, [](uint32_t) { return true; },
      [&](uint32_t t, const double4& r) {
        if (near<METRIC>(a, q, r)) W += a.weighted ? (long long)a.wi[t].x : 1ll;
        return early && W >= a.min_weight;
      });
  return W;
}

__device__ __forceinline__ void gd_keep(const GDArgs& a, uint32_t s, long long W) {
  const bool core = W >= a.min_weight;
  if (core) a.flags[s] |= F_CORE;
  const int i = a.wi[s].y;
  if (a.is_core) a.is_core[i] = core;
  if (a.wsum) a.wsum[i] = W;
}

template <int METRIC>
__global__ __launch_bounds__(GT) void k_gd_count(GDArgs a) {
  const uint32_t s = blockIdx.x * GT + threadIdx.x;
  if (s >= gd_nf(a) || (a.flags[s] & F_HEAVY)) return;
  gd_keep(a, s, gd_count<METRIC>(a, a.rec[s], 0u, 1u, !a.exact));
}

template <int METRIC>
__global__ __launch_bounds__(64) void k_gd_count_heavy(GDArgs a) {
  eg_heavy(
      a, a.heavy, a.ctr[C_HEAVY], [&](uint32_t s) { gd_keep(a, s, gd_count<METRIC>(a, a.rec[s], 0u, 1u, !a.exact)); },
      [&](uint32_t s, uint32_t lane) {
        const long long W = wave_all<WaveAdd>(gd_count<METRIC>(a, a.rec[s], lane, 64u, false));
        if (lane == 0) gd_keep(a, s, W);
      });
}

// ---- union ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t par_load(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root of x, halving the path on the way: a non-root only ever gets an ancestor stored, which is smaller than itself,
// so every chain descends and ends.
__device__ __forceinline__ uint32_t gd_find(uint32_t* par, uint32_t x) {
  uint32_t p = par_load(par + x);
  while (p != x) {
    const uint32_t gp = par_load(par + p);
    if (gp == p) return p;
    __hip_atomic_store(par + x, gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    x = p;
    p = gp;
  }
  return x;
}

// Hooks the larger root under the smaller.  Only a root is ever swapped (par[r] == r is the expected value), a failed swap
// returns an ancestor of r, and both roots only descend: the loop ends.
__device__ __forceinline__ void gd_unite(uint32_t* par, uint32_t x, uint32_t y) {
  uint32_t rx = gd_find(par, x), ry = gd_find(par, y);
  while (rx != ry) {
    if (rx < ry) {
      const uint32_t t = rx;
      rx = ry;
      ry = t;
    }
    const uint32_t old = atomicCAS(par + rx, rx, ry);
    if (old == rx) return;
    rx = gd_find(par, old);
    ry = gd_find(par, ry);
  }
}

// the symmetric relation is seen from both ends: the end with the larger slot number hooks
template <int METRIC>
__device__ __forceinline__ void gd_union(const GDArgs& a, uint32_t s, uint32_t off, uint32_t step) {
  const double4 q = a.rec[s];
  gd_walk(
      a, q, off, step, [&](uint32_t t) { return t < s && (a.flags[t] & F_CORE); },
      [&](uint32_t t, const double4& r) {
        if (near<METRIC>(a, q, r)) gd_unite(a.par, s, t);
        return false;
      });
}

template <int METRIC>
__global__ __launch_bounds__(GT) void k_gd_union(GDArgs a) {
  const uint32_t s = blockIdx.x * GT + threadIdx.x;
  if (s >= gd_nf(a) || a.flags[s] != F_CORE) return;  // not core, or heavy
  gd_union<METRIC>(a, s, 0u, 1u);
}

template <int METRIC>
__global__ __launch_bounds__(64) void k_gd_union_heavy(GDArgs a) {
  eg_heavy(
      a, a.heavy, a.ctr[C_HEAVY],
      [&](uint32_t s) {
        if (a.flags[s] & F_CORE) gd_union<METRIC>(a, s, 0u, 1u);
      },
      [&](uint32_t s, uint32_t lane) {
        if (a.flags[s] & F_CORE) gd_union<METRIC>(a, s, lane, 64u);
      });
}

// ---- numbering --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GT) void k_gd_flat(GDArgs a) {
  const uint32_t s = blockIdx.x * GT + threadIdx.x;
  if (s >= gd_nf(a) || !(a.flags[s] & F_CORE)) return;
  uint32_t root = s;
  for (uint32_t p; (p = a.par[root]) != root; root = p) {}  // par[x] < x off a root
  a.comp[s] = root;
  atomicMin(&a.minidx[root], (uint32_t)a.wi[s].y);
}

__global__ __launch_bounds__(GT) void k_gd_first(GDArgs a) {
  const uint32_t s = blockIdx.x * GT + threadIdx.x;
  if (s >= gd_nf(a) || !(a.flags[s] & F_CORE) || a.comp[s] != s) return;
  a.rank[a.minidx[s]] = 1u;
}

// thread t: the id of core slot t; the outputs of row t when it is outside the grid
__global__ __launch_bounds__(GT) void k_gd_label(GDArgs a, const uint32_t* __restrict__ cellof, int64_t n) {
  const int64_t t = (int64_t)blockIdx.x * GT + threadIdx.x;
  if (t < (int64_t)gd_nf(a) && (a.flags[t] & F_CORE)) {
    const uint32_t id = a.rank[a.minidx[a.comp[t]]] + (uint32_t)a.cf_in + 1u;
    a.cid[t] = id;
    a.labels[a.wi[t].y] = (int32_t)id;
  }
  if (t < n && cellof[t] == NOCELL) {
    const bool core = 0 >= a.min_weight;  // W = 0
    a.labels[t] = core ? (int32_t)(a.rank[t] + (uint32_t)a.cf_in + 1u) : 0;
    if (a.is_core) a.is_core[t] = core;
    if (a.wsum) a.wsum[t] = 0;
  }
}

// ---- border -----------------------------------------------------------------------------------------------------------
constexpr long long NOID = LLONG_MIN;

// the largest id among the core slots of q's N as a 64-bit key, NOID when there is none (an id is any int32)
template <int METRIC>
__device__ __forceinline__ long long gd_border(const GDArgs& a, const double4& q, uint32_t off, uint32_t step) {
  long long best = NOID;
  gd_walk(
      a, q, off, step, [&](uint32_t t) { return (a.flags[t] & F_CORE) != 0; },
      [&](uint32_t t, const double4& r) {
        if (near<METRIC>(a, q, r)) best = max(best, (long long)(int32_t)a.cid[t]);
        return false;
      });
  return best;
}

__device__ __forceinline__ void gd_border_keep(const GDArgs& a, uint32_t s, long long key) {
  a.labels[a.wi[s].y] = key == NOID ? 0 : (int32_t)key;
}

template <int METRIC>
__global__ __launch_bounds__(GT) void k_gd_border(GDArgs a) {
  const uint32_t s = blockIdx.x * GT + threadIdx.x;
  if (s >= gd_nf(a) || a.flags[s] != 0) return;  // core, or heavy
  gd_border_keep(a, s, gd_border<METRIC>(a, a.rec[s], 0u, 1u));
}

template <int METRIC>
__global__ __launch_bounds__(64) void k_gd_border_heavy(GDArgs a) {
  eg_heavy(
      a, a.heavy, a.ctr[C_HEAVY],
      [&](uint32_t s) {
        if (!(a.flags[s] & F_CORE)) gd_border_keep(a, s, gd_border<METRIC>(a, a.rec[s], 0u, 1u));
      },
      [&](uint32_t s, uint32_t lane) {
        if (a.flags[s] & F_CORE) return;  // wave-uniform
        const long long key = wave_all<WaveMax>(gd_border<METRIC>(a, a.rec[s], lane, 64u));
        if (lane == 0) gd_border_keep(a, s, key);
      });
}

template <int GD, int METRIC>
int run_gdbscan(vcp_ctx* ctx, const double* d_coords, int64_t n, int stride, double eps, const double* d_aux, double gate,
                const int32_t* d_w, int64_t min_weight, int32_t cf_in, int32_t* d_labels, uint8_t* d_is_core,
                int64_t* d_wsum, int32_t* cf_out) {
  hipStream_t st = ctx->stream;
  const unsigned nb = vcp_blocks(n, GT);
  const dim3 hgrid(vcp_blocks(n, 64, 16384));

  // 1. the weight check and the bounds: one read-back of [counters 64 | bounds 64]
  vcp_phase(ctx, "gdb_bounds");
  const int rb = vcp_bounds_parts(n);
  VCP_TRY(vcp_ensure(ctx, ctx->b_gd_misc, 128 + (size_t)rb * 64));
  uint32_t* ctr = ctx->b_gd_misc.as<uint32_t>();
  double* d_box = reinterpret_cast<double*>(ctx->b_gd_misc.as<char>() + 64);
  double* d_part = reinterpret_cast<double*>(ctx->b_gd_misc.as<char>() + 128);
  VCP_HIP(ctx, hipMemsetAsync(ctr, 0, 64, st));
  if (d_w) VCP_LAUNCH(ctx, k_gd_weights, dim3(nb), dim3(GT), 0, st, d_w, n, ctr);
  VCP_TRY(vcp_bounds_dev(ctx, BoundsSrc{d_coords, n, GD, stride}, d_part, d_box));
  char* hp = static_cast<char*>(ctx->pinned);
  VCP_HIP(ctx, hipMemcpyAsync(hp, ctr, 128, hipMemcpyDeviceToHost, st));
  VCP_HIP(ctx, hipStreamSynchronize(st));
  if (reinterpret_cast<const uint32_t*>(hp)[C_NEG]) return vcp_fail(ctx, VCP_ERR_ARG, "a weight is negative");
  const double* hb = reinterpret_cast<const double*>(hp + 64);
  double lo[3] = {hb[0], hb[1], hb[2]}, hi[3] = {hb[3], hb[4], hb[5]};
  for (int t = GD; t < 3; t++) lo[t] = hi[t] = 0.0;
  if ((int64_t)hb[6] == n) lo[0] = lo[1] = lo[2] = hi[0] = hi[1] = hi[2] = 0.0;
  for (int t = 0; t < GD; t++)
    if (!std::isfinite(hi[t] - lo[t]))
      return vcp_fail(ctx, VCP_ERR_UNSUPPORTED, "the cloud's extent overflows binary64 (coordinate differences are infinite)");

  // 2. the grid over the finite rows and the records in cell order
  vcp_phase(ctx, "gdb_grid");
  const EpsGrid g = eg_plan(lo, hi, eps);
  // per row: [rec 32 | wi 8 | cellof 4 | par 4 | comp 4 | minidx 4 | cid 4 | heavy 4], then [rank (n + 1) * 4 | flags n]
  const size_t nn = (size_t)n;
  const size_t o_wi = nn * 32, o_cell = o_wi + nn * 8, o_par = o_cell + nn * 4, o_comp = o_par + nn * 4,
               o_min = o_comp + nn * 4, o_cid = o_min + nn * 4, o_heavy = o_cid + nn * 4, o_rank = o_heavy + nn * 4,
               o_flags = o_rank + (nn + 1) * 4;
  VCP_TRY(vcp_ensure(ctx, ctx->b_gd_work, o_flags + nn));
  char* dw = ctx->b_gd_work.as<char>();
  uint32_t* cellof = reinterpret_cast<uint32_t*>(dw + o_cell);

  double4* rec = reinterpret_cast<double4*>(dw);
  int2* wi = reinterpret_cast<int2*>(dw + o_wi);

  GDArgs a{};
  a.g = g;
  a.rec = rec;
  a.wi = wi;
  a.eps = eps;
  a.gate = d_aux ? gate : 0.0;
  a.min_weight = min_weight;
  a.nc = (uint32_t)((size_t)g.Dx * g.Dy * g.Dz);
  a.none = !(eps >= 0.0);
  a.weighted = d_w != nullptr;
  a.exact = d_wsum != nullptr;
  a.cf_in = cf_in;
  a.flags = reinterpret_cast<uint8_t*>(dw + o_flags);
  a.par = reinterpret_cast<uint32_t*>(dw + o_par);
  a.comp = reinterpret_cast<uint32_t*>(dw + o_comp);
  a.minidx = reinterpret_cast<uint32_t*>(dw + o_min);
  a.cid = reinterpret_cast<uint32_t*>(dw + o_cid);
  a.heavy = reinterpret_cast<uint32_t*>(dw + o_heavy);
  a.ctr = ctr;
  a.rank = reinterpret_cast<uint32_t*>(dw + o_rank);
  a.labels = d_labels;
  a.is_core = d_is_core;
  a.wsum = reinterpret_cast<long long*>(d_wsum);

  VCP_HIP(ctx, hipMemsetAsync(a.rank, 0, (nn + 1) * 4, st));
  VCP_TRY(eg_bin<GT>(ctx, GDSrc<GD>{d_coords, stride, d_aux, d_w, (int)(min_weight <= 0), a.rank, rec, wi}, n, g, cellof,
                     ctx->b_gd_cell, &a.cellstart));
  VCP_LAUNCH(ctx, k_gd_init, dim3(nb), dim3(GT), 0, st, a);

  // 3. W and the core flags
  vcp_phase(ctx, "gdb_count");
  VCP_LAUNCH(ctx, (k_gd_count<METRIC>), dim3(nb), dim3(GT), 0, st, a);
  VCP_LAUNCH(ctx, (k_gd_count_heavy<METRIC>), hgrid, dim3(64), 0, st, a);

  // 4. the components of the core slots and their ranks
  vcp_phase(ctx, "gdb_union");
  VCP_LAUNCH(ctx, (k_gd_union<METRIC>), dim3(nb), dim3(GT), 0, st, a);
  VCP_LAUNCH(ctx, (k_gd_union_heavy<METRIC>), hgrid, dim3(64), 0, st, a);
  VCP_LAUNCH(ctx, k_gd_flat, dim3(nb), dim3(GT), 0, st, a);
  VCP_LAUNCH(ctx, k_gd_first, dim3(nb), dim3(GT), 0, st, a);
  VCP_TRY(vcp_exclusive_scan_u32(ctx, a.rank, a.rank, n + 1, nullptr));

  // 5. ids, the rows outside the grid, the border rows
  vcp_phase(ctx, "gdb_label");
  VCP_LAUNCH(ctx, k_gd_label, dim3(nb), dim3(GT), 0, st, a, cellof, n);
  VCP_LAUNCH(ctx, (k_gd_border<METRIC>), dim3(nb), dim3(GT), 0, st, a);
  VCP_LAUNCH(ctx, (k_gd_border_heavy<METRIC>), hgrid, dim3(64), 0, st, a);
  uint32_t* hk = reinterpret_cast<uint32_t*>(hp + 1024);
  VCP_HIP(ctx, hipMemcpyAsync(hk, a.rank + nn, 4, hipMemcpyDeviceToHost, st));
  VCP_TRY(vcp_phase_finish(ctx));
  VCP_HIP(ctx, hipStreamSynchronize(st));
  *cf_out = (int32_t)((uint32_t)cf_in + *hk);
  return VCP_OK;
}

// the argument errors of both forms; VCP_OK when the call can go on
int check_args(vcp_ctx* ctx, const void* coords, int64_t n, int dim, int metric, const void* aux, double gate,
               const void* labels, const void* cf_out) {
  if (n < 0) return vcp_fail(ctx, VCP_ERR_ARG, "n < 0");
  if (dim != 2 && dim != 3) return vcp_fail(ctx, VCP_ERR_ARG, "dim must be 2 or 3");
  if (metric != VCP_L1_2D && metric != VCP_L2_2D && metric != VCP_L2_3D)
    return vcp_fail(ctx, VCP_ERR_ARG, "vcp_gdbscan takes VCP_L1_2D, VCP_L2_2D or VCP_L2_3D (metric %d)", metric);
  if (metric == VCP_L2_3D && dim != 3) return vcp_fail(ctx, VCP_ERR_ARG, "VCP_L2_3D needs dim 3");
  if (aux && !(gate >= 0.0)) return vcp_fail(ctx, VCP_ERR_ARG, "gate must be >= 0 (+inf allowed)");
  if (!cf_out || (n > 0 && (!coords || !labels))) return vcp_fail(ctx, VCP_ERR_ARG, "null buffer");
  if (n >= ((int64_t)1 << 31)) return vcp_fail(ctx, VCP_ERR_TOO_LARGE, "n beyond int32 indices");
  return VCP_OK;
}
}  // namespace

extern "C" {

int vcp_gdbscan_dev(vcp_ctx* ctx, const double* d_coords, int64_t n, int dim, int metric, double eps, const double* d_aux,
                    double gate, const int32_t* d_weights, int64_t min_weight, int32_t cf_in, int32_t* d_labels,
                    uint8_t* d_is_core, int64_t* d_wsum, int32_t* cf_out) {
  if (!ctx) return VCP_ERR_ARG;
  VCP_TRY(check_args(ctx, d_coords, n, dim, metric, d_aux, gate, d_labels, cf_out));
  VCP_TRY(vcp_bind(ctx));
  vcp_phase_reset(ctx);
  if (n == 0) {
    ctx->last_timing.clear();
    *cf_out = cf_in;
    return VCP_OK;
  }
  if (metric == VCP_L1_2D)
    return run_gdbscan<2, VCP_L1_2D>(ctx, d_coords, n, dim, eps, d_aux, gate, d_weights, min_weight, cf_in, d_labels,
                                     d_is_core, d_wsum, cf_out);
  if (metric == VCP_L2_2D)
    return run_gdbscan<2, VCP_L2_2D>(ctx, d_coords, n, dim, eps, d_aux, gate, d_weights, min_weight, cf_in, d_labels,
                                     d_is_core, d_wsum, cf_out);
  return run_gdbscan<3, VCP_L2_3D>(ctx, d_coords, n, dim, eps, d_aux, gate, d_weights, min_weight, cf_in, d_labels,
                                   d_is_core, d_wsum, cf_out);
}

int vcp_gdbscan(vcp_ctx* ctx, const double* coords, int64_t n, int dim, int metric, double eps, const double* aux,
                double gate, const int32_t* weights, int64_t min_weight, int32_t cf_in, int32_t* labels, uint8_t* is_core,
                int64_t* wsum, int32_t* cf_out) {
  if (!ctx) return VCP_ERR_ARG;
  VCP_TRY(check_args(ctx, coords, n, dim, metric, aux, gate, labels, cf_out));
  if (n == 0)  // no copies: the device form's answer
    return vcp_gdbscan_dev(ctx, nullptr, 0, dim, metric, eps, nullptr, gate, nullptr, min_weight, cf_in, nullptr, nullptr,
                           nullptr, cf_out);
  VCP_TRY(vcp_bind(ctx));
  hipStream_t st = ctx->stream;
  // in: [coords n*dim*8 | aux n*8 | weights n*4]; out: [wsum n*8 | labels n*4 | is_core n]
  const size_t nn = (size_t)n;
  const size_t i_aux = nn * dim * 8, i_w = i_aux + nn * 8;
  const size_t o_lab = nn * 8, o_core = o_lab + nn * 4;
  VCP_TRY(vcp_ensure(ctx, ctx->b_gd_in, i_w + nn * 4));
  VCP_TRY(vcp_ensure(ctx, ctx->b_gd_out, o_core + nn));
  char* din = ctx->b_gd_in.as<char>();
  char* dout = ctx->b_gd_out.as<char>();
  VCP_HIP(ctx, hipMemcpyAsync(din, coords, i_aux, hipMemcpyHostToDevice, st));
  if (aux) VCP_HIP(ctx, hipMemcpyAsync(din + i_aux, aux, nn * 8, hipMemcpyHostToDevice, st));
  if (weights) VCP_HIP(ctx, hipMemcpyAsync(din + i_w, weights, nn * 4, hipMemcpyHostToDevice, st));
  int32_t cf = 0;
  VCP_TRY(vcp_gdbscan_dev(ctx, reinterpret_cast<const double*>(din), n, dim, metric, eps,
                          aux ? reinterpret_cast<const double*>(din + i_aux) : nullptr, gate,
                          weights ? reinterpret_cast<const int32_t*>(din + i_w) : nullptr, min_weight, cf_in,
                          reinterpret_cast<int32_t*>(dout + o_lab),
                          is_core ? reinterpret_cast<uint8_t*>(dout + o_core) : nullptr,
                          wsum ? reinterpret_cast<int64_t*>(dout) : nullptr, &cf));
  VCP_HIP(ctx, hipMemcpyAsync(labels, dout + o_lab, nn * 4, hipMemcpyDeviceToHost, st));
  if (is_core) VCP_HIP(ctx, hipMemcpyAsync(is_core, dout + o_core, nn, hipMemcpyDeviceToHost, st));
  if (wsum) VCP_HIP(ctx, hipMemcpyAsync(wsum, dout, nn * 8, hipMemcpyDeviceToHost, st));
  VCP_HIP(ctx, hipStreamSynchronize(st));
  *cf_out = cf;
  return VCP_OK;
}

}  // extern "C"
