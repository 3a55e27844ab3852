// kdist.hip -- exact k-distance / k nearest neighbours (vcp_kdist, vcp_kdist_dev) on MI355X (gfx950).
//
// kdist_k[i] = k-th smallest d(i, j) over ALL j (j = i included), d = the binary64 expression vcp_dbscan tests
// (|dx| + |dy|, or the correctly rounded sqrt of dx*dx + dy*dy [+ dz*dz], summed left to right, no FMA contraction).
// knn row i = the k smallest (d, j) pairs in lexicographic order.  So vcp_dbscan(eps, min_pts = k).is_core[i] ==
// (kdist_k[i] <= eps) for every finite eps.
//
// Passes:
//   bounds  bounding box of the finite coordinates and the non-finite point count (bounds.hip); then the lattice box is
//           trimmed to mean +- 8 sigma of the values inside it, repeatedly (vcp_robust_range, as for dbscan.hip's grid): a
//           few far outliers land in the EDGE codes of the lattice instead of stretching it for everybody.
//   order   per point a 60-bit Morton key of its lattice codes (2^30 codes per axis in 2-D, 2^20 in 3-D, cubic cells;
//           code 0 / 2^L - 1 = everything below / above the box on that axis; non-finite points get a key after every
//           finite one), one rocPRIM radix sort of (key, index), a gather of the coordinates into key order, and a dense
//           table of the first position of every cell of level G (2^(G dim) <= 2n cells: marks + the library's
//           exclusive max-scan).  In key order every cell of every level l (2^l cells per axis) is ONE contiguous range:
//           level <= G from the table, finer levels by binary search inside the range of the level-G ancestor.
//   search  one lane per query, queries in key order (a wave's queries share their cells).  Start level = the finest
//           level whose own cell holds >= k points (read off the sorted keys: the common prefix of a window of k
//           consecutive keys around the query).  Scan the 3^dim block of cells around the query's cell; keep the top k
//           (value, index) pairs in registers (template K = 8 / 16 / 32 / 64, compile-time indices only: the K - k
//           unused slots are pre-filled with (-inf, -1), which nothing displaces); stop when the k-th value is
//           STRICTLY below a rounding-safe lower bound of the distance to anything outside the block, else go one level
//           coarser and scan again.  A block of more than HEAVY points is left to the heavy pass.
//   heavy   one wave per such query (dense duplicates, far outliers): the block's points dealt over the 64 lanes, each
//           lane keeps its own top K, the 64 sorted lists are merged in LDS by k rounds of a wave-wide arg-min.
//
// The stop bound.  u = (x - lo) * s is the lattice coordinate (code m <=> u in [m - 1, m), edge codes unbounded).  The
// block of level l covers the codes [C0, C1) on an axis; every point outside it has, on some axis, u <= C0 - 1 or
// u >= C1 - 1.  Each computed u is within |u| 2^-51 of the exact value, so the gap (in codes) between the query and any
// outside point is at least min_a (u_q - (C0 - 1), (C1 - 1) - u_q) - (2^-16 + |u_q| 2^-40), and in coordinates that
// gap times w = 1 / s (1 - 2^-30).  Both metrics are >= the largest |coordinate difference| up to one rounding
// (monotone roundings; the sqrt is correctly rounded), so an outside point's d exceeds the bound times (1 - 2^-50).
// kth < bound therefore proves no outside point can enter the top k, ties by index included.
#include <climits>
#include <cmath>

#include "bounds.hpp"
#include "sort.hpp"
#include "vcp_ctx.hpp"

namespace {
constexpr int KT = 256;            // threads per workgroup of the streaming passes and the search
constexpr int KEYBITS = 60;        // Morton key bits (2-D: 2 x 30, 3-D: 3 x 20)
constexpr uint64_t SENT = 1ull << KEYBITS;  // key of a non-finite point: sorts after every finite key
constexpr uint32_t HEAVY = 8192;   // a block with more points goes to the wave-per-query pass
constexpr int NO_ID = INT_MAX;     // an empty slot: (+inf, NO_ID) sorts after every real (d, j); written out as -1

template <int GD>
struct Lat {
  static constexpr int L = KEYBITS / GD;  // levels: 30 (2-D), 20 (3-D)
};

struct KArgs {
  const double4* rec;      // [nf] key order: (x, y, z, original index in the low word of w)
  const uint64_t* keys;    // [nf] sorted keys
  const uint32_t* start;   // [2^(G dim) + 1] first position of every level-G cell
  double lo[3];            // lattice origin (the trimmed box)
  double s, w;             // codes per unit and its inverse
  int G;
  int k;
  uint32_t nf;
  double* kdist;           // [n] by original index
  int32_t* knn;            // [n * k] or null
  uint32_t* heavy;         // [nf] sorted positions left to the heavy pass
  uint32_t* heavy_cnt;
};

__host__ __device__ __forceinline__ uint64_t spread2(uint64_t x) {  // 30 bits -> every 2nd bit
  x &= 0x3FFFFFFFull;
  x = (x | (x << 16)) & 0x0000FFFF0000FFFFull;
  x = (x | (x << 8)) & 0x00FF00FF00FF00FFull;
  x = (x | (x << 4)) & 0x0F0F0F0F0F0F0F0Full;
  x = (x | (x << 2)) & 0x3333333333333333ull;
  x = (x | (x << 1)) & 0x5555555555555555ull;
  return x;
}
__host__ __device__ __forceinline__ uint64_t spread3(uint64_t x) {  // 21 bits -> every 3rd bit
  x &= 0x1FFFFFull;
  x = (x | (x << 32)) & 0x1F00000000FFFFull;
  x = (x | (x << 16)) & 0x1F0000FF0000FFull;
  x = (x | (x << 8)) & 0x100F00F00F00F00Full;
  x = (x | (x << 4)) & 0x10C30C30C30C30C3ull;
  x = (x | (x << 2)) & 0x1249249249249249ull;
  return x;
}
template <int GD>
__host__ __device__ __forceinline__ uint64_t morton(const uint32_t* c) {
  if (GD == 2) return spread2(c[0]) | (spread2(c[1]) << 1);
  return spread3(c[0]) | (spread3(c[1]) << 1) | (spread3(c[2]) << 2);
}

// lattice coordinate and code of one axis
__device__ __forceinline__ double lat_u(double x, double lo, double s) { return (x - lo) * s; }
template <int GD>
__device__ __forceinline__ uint32_t lat_code(double u) {
  constexpr uint32_t top = (1u << Lat<GD>::L) - 1;
  if (!(u >= 0.0)) return 0;
  if (u >= (double)(top - 1)) return top;
  return (uint32_t)u + 1u;
}

template <int GD>
__device__ __forceinline__ bool finite_pt(const double* q) {
  bool f = true;
#pragma unroll
  for (int a = 0; a < GD; a++) f = f && isfinite(q[a]);
  return f;
}

template <int GD>
__device__ __forceinline__ void load_pt(const double* __restrict__ c, int64_t i, int stride, double* q) {
#pragma unroll
  for (int a = 0; a < GD; a++) q[a] = c[i * stride + a];
  if (GD == 2) q[2] = 0.0;
}

// the distance expression of vcp_dbscan (binary64, left to right, -ffp-contract=off)
template <int METRIC>
__device__ __forceinline__ double dist(const double* q, const double4& r) {
  const double dx = q[0] - r.x, dy = q[1] - r.y;
  if (METRIC == VCP_L1_2D) return fabs(dx) + fabs(dy);
  if (METRIC == VCP_L2_2D) return sqrt(dx * dx + dy * dy);
  const double dz = q[2] - r.z;
  return sqrt(dx * dx + dy * dy + dz * dz);
}

__device__ __forceinline__ bool lt(double a, int i, double b, int j) { return a < b || (a == b && i < j); }

// ---- order -------------------------------------------------------------------------------------------------------
template <int GD>
__global__ __launch_bounds__(KT) void k_kd_keys(const double* __restrict__ c, int64_t n, int stride, KArgs a,
                                               uint64_t* __restrict__ key, uint32_t* __restrict__ val) {
  const int64_t i = (int64_t)blockIdx.x * KT + threadIdx.x;
  if (i >= n) return;
  double q[3];
  load_pt<GD>(c, i, stride, q);
  uint64_t kk = SENT;
  if (finite_pt<GD>(q)) {
    uint32_t cc[3];
#pragma unroll
    for (int t = 0; t < GD; t++) cc[t] = lat_code<GD>(lat_u(q[t], a.lo[t], a.s));
    kk = morton<GD>(cc);
  }
  key[i] = kk;
  val[i] = (uint32_t)i;
}

// coordinates into key order; the non-finite points (positions >= nf) get their answer here: NaN and a row of -1
template <int GD>
__global__ __launch_bounds__(KT) void k_kd_gather(const double* __restrict__ c, int64_t n, int stride,
                                                 const uint32_t* __restrict__ sval, KArgs a, double4* __restrict__ rec) {
  const int64_t p = (int64_t)blockIdx.x * KT + threadIdx.x;
  if (p >= n) return;
  const uint32_t i = sval[p];
  if (p >= (int64_t)a.nf) {
    a.kdist[i] = NAN;
    if (a.knn)
      for (int t = 0; t < a.k; t++) a.knn[(size_t)i * a.k + t] = -1;
    return;
  }
  double q[3];
  load_pt<GD>(c, i, stride, q);
  rec[p] = make_double4(q[0], q[1], q[2], __hiloint2double(0, (int)i));
}

// mark[cell + 0] = end position of every non-empty level-G cell (its exclusive max-scan is the start table)
template <int GD>
__global__ __launch_bounds__(KT) void k_kd_marks(const uint64_t* __restrict__ keys, uint32_t nf, int G,
                                                uint32_t* __restrict__ mark) {
  const uint32_t p = blockIdx.x * KT + threadIdx.x;
  if (p >= nf) return;
  const int sh = (Lat<GD>::L - G) * GD;
  const uint64_t c = keys[p] >> sh;
  if (p + 1 == nf || (keys[p + 1] >> sh) != c) mark[c] = p + 1;
}

// ---- search --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t lower_bound(const uint64_t* __restrict__ keys, uint32_t s, uint32_t e, uint64_t v) {
  while (s < e) {
    const uint32_t m = s + ((e - s) >> 1);
    if (keys[m] < v) s = m + 1; else e = m;
  }
  return s;
}

// point range [s, e) of the level-l cell with per-axis cell coordinates c
template <int GD>
__device__ __forceinline__ void cell_range(const KArgs& a, int l, const uint32_t* c, uint32_t& s, uint32_t& e) {
  constexpr int L = Lat<GD>::L;
  if (l == 0) {
    s = 0;
    e = a.nf;
    return;
  }
  uint32_t f[3];
#pragma unroll
  for (int t = 0; t < GD; t++) f[t] = c[t] << (L - l);
  const uint64_t full = morton<GD>(f);
  const int shG = (L - a.G) * GD;
  if (l <= a.G) {
    const uint64_t g = full >> shG;
    s = a.start[g];
    e = a.start[g + (1ull << ((a.G - l) * GD))];
    return;
  }
  const uint64_t g = full >> shG;
  const uint32_t s0 = a.start[g], e0 = a.start[g + 1];
  s = lower_bound(a.keys, s0, e0, full);
  e = lower_bound(a.keys, s, e0, full + (1ull << ((L - l) * GD)));
}

// block of level l around the query: per-axis cell range [b0, b1] and the lower bound of the distance to anything
// outside (see the file header)
template <int GD>
__device__ __forceinline__ double block_of(const KArgs& a, int l, const uint32_t* code, const double* u, uint32_t* b0,
                                           uint32_t* b1, bool& whole) {
  constexpr int L = Lat<GD>::L;
  constexpr uint64_t top = 1ull << L;
  double gap = INFINITY;
#pragma unroll
  for (int t = 0; t < GD; t++) {
    const uint32_t c = code[t] >> (L - l);
    const uint32_t cmax = (1u << l) - 1u;
    b0[t] = c > 0 ? c - 1 : 0;
    b1[t] = c < cmax ? c + 1 : cmax;
    const uint64_t C0 = (uint64_t)b0[t] << (L - l), C1 = ((uint64_t)b1[t] + 1) << (L - l);
    const double marg = 1.52587890625e-05 + fabs(u[t]) * 9.094947017729282e-13;  // 2^-16 + |u| 2^-40
    if (C0 > 0) gap = fmin(gap, u[t] - (double)(C0 - 1) - marg);
    if (C1 < top) gap = fmin(gap, (double)(C1 - 1) - u[t] - marg);
  }
  whole = gap == INFINITY;  // the block is the whole lattice
  if (whole) return INFINITY;
  if (!(gap > 0.0)) return 0.0;
  return gap * a.w * (1.0 - 9.313225746154785e-10);  // (1 - 2^-30)
}

template <int GD>
__device__ __forceinline__ int start_level(const KArgs& a, uint32_t p) {
  constexpr int L = Lat<GD>::L;
  const uint32_t k = (uint32_t)a.k;
  if (a.nf < k) return 0;
  int best = 0;
  for (uint32_t t = 0; t < k; t++) {  // windows [w0, w0 + k) that hold p
    if (t > p) break;
    const uint32_t w0 = p - t;
    if (w0 + k > a.nf) continue;
    const uint64_t x = a.keys[w0] ^ a.keys[w0 + k - 1];
    const int lev = x == 0 ? L : (__clzll((long long)x) - (64 - KEYBITS)) / GD;
    best = max(best, lev);
  }
  return best;
}

template <int GD>
__device__ __forceinline__ void query_setup(const KArgs& a, uint32_t p, double* q, int& qi, uint32_t* code, double* u) {
  const double4 me = a.rec[p];
  q[0] = me.x;
  q[1] = me.y;
  q[2] = me.z;
  qi = __double2loint(me.w);
#pragma unroll
  for (int t = 0; t < GD; t++) {
    u[t] = lat_u(q[t], a.lo[t], a.s);
    code[t] = lat_code<GD>(u[t]);
  }
}

template <int K>
struct TopK {
  double v[K];
  int id[K];
  __device__ __forceinline__ void reset(int k) {
#pragma unroll
    for (int t = 0; t < K; t++) {
      const bool pad = t < K - k;
      v[t] = pad ? -INFINITY : INFINITY;
      id[t] = pad ? -1 : NO_ID;
    }
  }
  __device__ __forceinline__ void insert(double d, int j) {
    if (!lt(d, j, v[K - 1], id[K - 1])) return;
    double cd = d;
    int cj = j;
#pragma unroll
    for (int t = 0; t < K; t++) {
      if (lt(cd, cj, v[t], id[t])) {
        const double td = v[t];
        const int tj = id[t];
        v[t] = cd;
        id[t] = cj;
        cd = td;
        cj = tj;
      }
    }
  }
};

template <int GD>
__device__ __forceinline__ void cell_coords(int t, const uint32_t* b0, uint32_t* c) {
  c[0] = b0[0] + (uint32_t)(t % 3);
  c[1] = b0[1] + (uint32_t)((t / 3) % 3);
  if (GD == 3) c[2] = b0[2] + (uint32_t)(t / 9);
}

template <int GD, int METRIC, int K>
__global__ __launch_bounds__(KT) void k_kd_search(KArgs a) {
  constexpr int NC = GD == 2 ? 9 : 27;
  const uint32_t p = blockIdx.x * KT + threadIdx.x;
  if (p >= a.nf) return;
  double q[3], u[3];
  uint32_t code[3];
  int qi;
  query_setup<GD>(a, p, q, qi, code, u);
  TopK<K> top;
  for (int l = start_level<GD>(a, p);; l--) {
    uint32_t b0[3], b1[3];
    bool whole;
    const double bound = block_of<GD>(a, l, code, u, b0, b1, whole);
    uint32_t total = 0;
    for (int t = 0; t < NC; t++) {
      uint32_t c[3];
      cell_coords<GD>(t, b0, c);
      if (c[0] > b1[0] || c[1] > b1[1] || (GD == 3 && c[2] > b1[2])) continue;
      uint32_t s, e;
      cell_range<GD>(a, l, c, s, e);
      total += e - s;
    }
    if (total > HEAVY) {
      a.heavy[atomicAdd(a.heavy_cnt, 1u)] = p;
      return;
    }
    top.reset(a.k);
    for (int t = 0; t < NC; t++) {
      uint32_t c[3];
      cell_coords<GD>(t, b0, c);
      if (c[0] > b1[0] || c[1] > b1[1] || (GD == 3 && c[2] > b1[2])) continue;
      uint32_t s, e;
      cell_range<GD>(a, l, c, s, e);
      for (uint32_t j = s; j < e; j++) {
        const double4 r = a.rec[j];
        top.insert(dist<METRIC>(q, r), __double2loint(r.w));
      }
    }
    if (top.v[K - 1] < bound || whole) break;
  }
  a.kdist[qi] = top.v[K - 1];
  if (a.knn) {
#pragma unroll
    for (int t = 0; t < K; t++)
      if (t >= K - a.k) a.knn[(size_t)qi * a.k + (t - (K - a.k))] = top.id[t] == NO_ID ? -1 : top.id[t];
  }
}

// one wave per heavy query.  Every lane keeps its own sorted top K in LDS (slot t of lane l at t * 64 + l: no bank
// conflicts; runtime indices are fine there), pre-filled like TopK; the 64 lists are then merged by k rounds of a
// wave-wide arg-min over their heads.
template <int GD, int METRIC, int K>
__global__ __launch_bounds__(64) void k_kd_heavy(KArgs a) {
  constexpr int NC = GD == 2 ? 9 : 27;
  __shared__ double lv[64 * K];
  __shared__ int li[64 * K];
  __shared__ double rv[K];
  __shared__ int ri[K];
  const int lane = threadIdx.x;
  const uint32_t cnt = *a.heavy_cnt;
  for (uint32_t h = blockIdx.x; h < cnt; h += gridDim.x) {
    const uint32_t p = a.heavy[h];
    double q[3], u[3];
    uint32_t code[3];
    int qi;
    query_setup<GD>(a, p, q, qi, code, u);
    for (int l = start_level<GD>(a, p);; l--) {
      uint32_t b0[3], b1[3];
      bool whole;
      const double bound = block_of<GD>(a, l, code, u, b0, b1, whole);
      for (int t = 0; t < K; t++) {
        const bool pad = t < K - a.k;
        lv[t * 64 + lane] = pad ? -INFINITY : INFINITY;
        li[t * 64 + lane] = pad ? -1 : NO_ID;
      }
      double worst = INFINITY;
      int worst_id = NO_ID;
      for (int t = 0; t < NC; t++) {
        uint32_t c[3];
        cell_coords<GD>(t, b0, c);
        if (c[0] > b1[0] || c[1] > b1[1] || (GD == 3 && c[2] > b1[2])) continue;
        uint32_t s, e;
        cell_range<GD>(a, l, c, s, e);
        for (uint32_t j = s + lane; j < e; j += 64) {
          const double4 r = a.rec[j];
          const double d = dist<METRIC>(q, r);
          const int jd = __double2loint(r.w);
          if (!lt(d, jd, worst, worst_id)) continue;
          int t2 = K - 1;  // insertion: the (-inf, -1) pads (or slot 0) stop the walk
          while (t2 > 0 && lt(d, jd, lv[(t2 - 1) * 64 + lane], li[(t2 - 1) * 64 + lane])) {
            lv[t2 * 64 + lane] = lv[(t2 - 1) * 64 + lane];
            li[t2 * 64 + lane] = li[(t2 - 1) * 64 + lane];
            t2--;
          }
          lv[t2 * 64 + lane] = d;
          li[t2 * 64 + lane] = jd;
          worst = lv[(K - 1) * 64 + lane];
          worst_id = li[(K - 1) * 64 + lane];
        }
      }
      // merge the 64 sorted lists: k rounds of a wave-wide arg-min over the list heads
      int ptr = K - a.k;
      for (int r = 0; r < a.k; r++) {
        double hv = ptr < K ? lv[ptr * 64 + lane] : INFINITY;
        int hi = ptr < K ? li[ptr * 64 + lane] : NO_ID;
        int hl = lane;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
          const double ov = __shfl_xor(hv, d, 64);
          const int oi = __shfl_xor(hi, d, 64);
          const int ol = __shfl_xor(hl, d, 64);
          if (lt(ov, oi, hv, hi) || (ov == hv && oi == hi && ol < hl)) {
            hv = ov;
            hi = oi;
            hl = ol;
          }
        }
        if (hl == lane) ptr++;
        if (lane == 0) {
          rv[r] = hv;
          ri[r] = hi;
        }
      }
      __syncthreads();
      const double kth = rv[a.k - 1];
      if (kth < bound || whole) break;
    }
    if (lane == 0) a.kdist[qi] = rv[a.k - 1];
    if (a.knn)
      for (int t = lane; t < a.k; t += 64) a.knn[(size_t)qi * a.k + t] = ri[t] == NO_ID ? -1 : ri[t];
    __syncthreads();
  }
}
template <int GD, int METRIC, int K>
int launch_search(vcp_ctx* ctx, const KArgs& a) {
  VCP_LAUNCH(ctx, (k_kd_search<GD, METRIC, K>), dim3(vcp_blocks(a.nf, KT)), dim3(KT), 0, ctx->stream, a);
  vcp_phase(ctx, "kdist_heavy");
  VCP_LAUNCH(ctx, (k_kd_heavy<GD, METRIC, K>), dim3(8192), dim3(64), 0, ctx->stream, a);  // persistent over the list
  return VCP_OK;
}

template <int GD, int METRIC>
int launch_k(vcp_ctx* ctx, const KArgs& a) {
  if (a.k <= 8) return launch_search<GD, METRIC, 8>(ctx, a);
  if (a.k <= 16) return launch_search<GD, METRIC, 16>(ctx, a);
  if (a.k <= 32) return launch_search<GD, METRIC, 32>(ctx, a);
  return launch_search<GD, METRIC, 64>(ctx, a);
}

template <int GD>
int run_kdist(vcp_ctx* ctx, const double* d_coords, int64_t n, int stride, int metric, int k, double* d_kdist,
              int32_t* d_knn) {
  constexpr int L = Lat<GD>::L;
  hipStream_t st = ctx->stream;
  const unsigned nb = vcp_blocks(n, KT);

  // 1. bounds and the trimmed lattice box
  vcp_phase(ctx, "kdist_bounds");
  const int rb = vcp_bounds_parts(n);
  VCP_TRY(vcp_ensure(ctx, ctx->b_kd_part, (size_t)(rb * 8 + 8) * sizeof(double)));
  double* d_part = ctx->b_kd_part.as<double>();
  double* h = reinterpret_cast<double*>(ctx->pinned);
  const BoundsSrc src{d_coords, n, GD, stride};
  VCP_TRY(vcp_bounds(ctx, src, d_part, d_part + (size_t)rb * 8, h));
  double lo[3] = {h[0], h[1], h[2]}, hi[3] = {h[3], h[4], h[5]};
  const uint32_t nf = (uint32_t)(n - (int64_t)h[6]);
  for (int t = GD; t < 3; t++) lo[t] = hi[t] = 0.0;
  if (nf > 0)
    for (int t = 0; t < GD; t++)
      if (!std::isfinite(hi[t] - lo[t]))
        return vcp_fail(ctx, VCP_ERR_UNSUPPORTED, "the cloud's extent overflows binary64 (coordinate differences are infinite)");
  if (nf == 0) lo[0] = lo[1] = lo[2] = hi[0] = hi[1] = hi[2] = 0.0;
  // robust range: mean +- 8 sigma of the points inside, repeated while it shrinks
  if (nf > 1)
    VCP_TRY(vcp_robust_range(
        ctx, src, ctx->b_kd_part, lo, hi, [](double l, double u) { return 1e-9 * (u - l); },
        [](const double*, const double*) { return false; }));
  double ext = 0.0;
  for (int t = 0; t < GD; t++) ext = std::fmax(ext, hi[t] - lo[t]);
  double s = (double)((1u << L) - 2) / ext;
  if (!(ext > 0.0) || !std::isfinite(s)) s = 1.0;

  KArgs a;
  for (int t = 0; t < 3; t++) a.lo[t] = lo[t];
  a.s = s;
  a.w = 1.0 / s;
  a.k = k;
  a.nf = nf;
  a.kdist = d_kdist;
  a.knn = d_knn;
  int G = 1;
  while (G < L && ((int64_t)1 << ((G + 1) * GD)) <= 2 * (int64_t)nf) G++;
  a.G = G;

  // 2. Morton order
  vcp_phase(ctx, "kdist_order");
  const size_t cells = ((size_t)1 << (G * GD)) + 1;
  VCP_TRY(vcp_ensure(ctx, ctx->b_kd_key, (size_t)n * 16));
  VCP_TRY(vcp_ensure(ctx, ctx->b_kd_val, (size_t)n * 8));
  VCP_TRY(vcp_ensure(ctx, ctx->b_kd_rec, (size_t)n * sizeof(double4)));
  VCP_TRY(vcp_ensure(ctx, ctx->b_kd_start, cells * 4 + 64));
  VCP_TRY(vcp_ensure(ctx, ctx->b_kd_heavy, (size_t)n * 4 + 64));
  uint64_t* kin = ctx->b_kd_key.as<uint64_t>();
  uint64_t* kout = kin + n;
  uint32_t* vin = ctx->b_kd_val.as<uint32_t>();
  uint32_t* vout = vin + n;
  uint32_t* start = ctx->b_kd_start.as<uint32_t>();
  uint32_t* heavy_cnt = start + cells;
  a.heavy = ctx->b_kd_heavy.as<uint32_t>();
  a.heavy_cnt = heavy_cnt;
  VCP_LAUNCH(ctx, (k_kd_keys<GD>), dim3(nb), dim3(KT), 0, st, d_coords, n, stride, a, kin, vin);
  VCP_TRY(vcp_sort_pairs(ctx, ctx->b_kd_tmp, kin, kout, vin, vout, (size_t)n, KEYBITS + 1));
  double4* rec = ctx->b_kd_rec.as<double4>();
  VCP_LAUNCH(ctx, (k_kd_gather<GD>), dim3(nb), dim3(KT), 0, st, d_coords, n, stride, vout, a, rec);
  VCP_HIP(ctx, hipMemsetAsync(start, 0, cells * 4 + 4, st));  // the marks and the heavy counter
  if (nf > 0) {
    VCP_LAUNCH(ctx, (k_kd_marks<GD>), dim3(vcp_blocks(nf, KT)), dim3(KT), 0, st, kout, nf, G, start);
    VCP_TRY(vcp_exclusive_max_scan_u32(ctx, start, start, (int64_t)cells, nullptr));
  }
  a.rec = rec;
  a.keys = kout;
  a.start = start;

  // 3. search
  if (nf > 0) {
    vcp_phase(ctx, "kdist_search");
    if constexpr (GD == 2) {
      if (metric == VCP_L1_2D) VCP_TRY((launch_k<2, VCP_L1_2D>(ctx, a)));
      else VCP_TRY((launch_k<2, VCP_L2_2D>(ctx, a)));
    } else {
      VCP_TRY((launch_k<3, VCP_L2_3D>(ctx, a)));
    }
  }
  VCP_TRY(vcp_phase_finish(ctx));
  VCP_HIP(ctx, hipStreamSynchronize(st));
  return VCP_OK;
}

}  // namespace

extern "C" {

int vcp_kdist_dev(vcp_ctx* ctx, const double* d_coords, int64_t n, int dim, int metric, int k, double* d_kdist,
                  int32_t* d_knn) {
  if (!ctx) return VCP_ERR_ARG;
  if (n < 0) return vcp_fail(ctx, VCP_ERR_ARG, "n < 0");
  if (dim != 2 && dim != 3) return vcp_fail(ctx, VCP_ERR_ARG, "dim must be 2 or 3");
  if (metric != VCP_L1_2D && metric != VCP_L2_2D && metric != VCP_L2_3D)
    return vcp_fail(ctx, VCP_ERR_ARG, "vcp_kdist takes VCP_L1_2D, VCP_L2_2D or VCP_L2_3D (metric %d)", metric);
  if (metric == VCP_L2_3D && dim != 3) return vcp_fail(ctx, VCP_ERR_ARG, "VCP_L2_3D needs dim 3");
  if (k < 1) return vcp_fail(ctx, VCP_ERR_ARG, "k < 1");
  if (k > 64) return vcp_fail(ctx, VCP_ERR_UNSUPPORTED, "k > 64");
  if (n >= ((int64_t)1 << 31)) return vcp_fail(ctx, VCP_ERR_TOO_LARGE, "n beyond int32 indices");
  if (n > 0 && (!d_coords || !d_kdist)) return vcp_fail(ctx, VCP_ERR_ARG, "null buffer");
  VCP_TRY(vcp_bind(ctx));
  vcp_phase_reset(ctx);
  if (n == 0) {
    ctx->last_timing.clear();
    return VCP_OK;
  }
  if (metric == VCP_L2_3D) return run_kdist<3>(ctx, d_coords, n, dim, metric, k, d_kdist, d_knn);
  return run_kdist<2>(ctx, d_coords, n, dim, metric, k, d_kdist, d_knn);
}

int vcp_kdist(vcp_ctx* ctx, const double* coords, int64_t n, int dim, int metric, int k, double* kdist,
              int32_t* knn) {
  if (!ctx) return VCP_ERR_ARG;
  if (n < 0) return vcp_fail(ctx, VCP_ERR_ARG, "n < 0");
  if (dim != 2 && dim != 3) return vcp_fail(ctx, VCP_ERR_ARG, "dim must be 2 or 3");
  if (n > 0 && (!coords || !kdist)) return vcp_fail(ctx, VCP_ERR_ARG, "null buffer");
  if (k < 1 || k > 64 || n == 0 || n >= ((int64_t)1 << 31))  // the argument errors of the device form, no copies
    return vcp_kdist_dev(ctx, nullptr, n, dim, metric, k, nullptr, nullptr);
  VCP_TRY(vcp_bind(ctx));
  hipStream_t st = ctx->stream;
  VCP_TRY(vcp_ensure(ctx, ctx->b_kd_in, (size_t)n * dim * 8));
  VCP_TRY(vcp_ensure(ctx, ctx->b_kd_out, (size_t)n * 8));
  if (knn) VCP_TRY(vcp_ensure(ctx, ctx->b_kd_outk, (size_t)n * k * 4));
  VCP_HIP(ctx, hipMemcpyAsync(ctx->b_kd_in.p, coords, (size_t)n * dim * 8, hipMemcpyHostToDevice, st));
  VCP_TRY(vcp_kdist_dev(ctx, ctx->b_kd_in.as<double>(), n, dim, metric, k, ctx->b_kd_out.as<double>(),
                        knn ? ctx->b_kd_outk.as<int32_t>() : nullptr));
  VCP_HIP(ctx, hipMemcpyAsync(kdist, ctx->b_kd_out.p, (size_t)n * 8, hipMemcpyDeviceToHost, st));
  if (knn) VCP_HIP(ctx, hipMemcpyAsync(knn, ctx->b_kd_outk.p, (size_t)n * k * 4, hipMemcpyDeviceToHost, st));
  VCP_HIP(ctx, hipStreamSynchronize(st));
  return VCP_OK;
}

}  // extern "C"
