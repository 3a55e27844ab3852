// cluster_quant.hip -- order statistics per cluster or group: vcp_cluster_quantiles and vcp_cluster_mad (include/vcp.h,
// DESIGN.md section 29).
//
// The reference has no order statistic but a global one: Tools.GetGroupingManOrMin (BaseClass/Tools.cs:468-497) takes the
// min / max of Distance over all files to seed the one band of SureDistanceFilter.cs:26-61, which
// Tools.FilterByDistance_FixedPoint (:438-461) applies to every file alike.  Here every group gets its own ranks, and a
// band of its own from the median absolute deviation.
//
// The rows are put in (group, row) order by vcp_group_by_label, their values are gathered in that order as 64-bit keys
// whose unsigned order is the numeric order (cq_key), and every segment is selected from by the class of its size:
//   up to CQ_WAVE_MAX keys   one wave: a key per lane, its rank counted over shuffles (k_cq_select_wave)
//   up to CQ_WG_MAX keys     one workgroup: the keys in LDS, an 8-bit MSD radix select per rank (k_cq_select_wg)
//   beyond                   per digit one histogram launch over all the large segments' chunks and one pick launch
//                            (k_cq_hist, k_cq_pick): 16 launches whatever the number of large segments
// Only integer compares and integer atomics decide which key is returned, and the key IS the value: no class can give
// another answer than the next.  All grids are sized to the device and walk their segments or chunks.
#include <cmath>
#include <cstring>

#include "radix_pick.hpp"
#include "sort.hpp"
#include "vcp_ctx.hpp"

namespace {
constexpr int QT = 256;
constexpr int CQ_WAVE_MAX = VCP_CQ_WAVE_MAX;  // 64: one key per lane
constexpr int CQ_WG_MAX = VCP_CQ_WG_MAX;      // 4096: 32 KB of keys in LDS
constexpr int CQ_NQ_MAX = VCP_CQ_NQ_MAX;      // 16 ranks per call: 16 KB of histograms in LDS (k_cq_hist)
constexpr int CQ_HIST_KEYS = 4096;            // keys per chunk of a large segment
constexpr int CQ_DIGITS = 8;
static_assert(QT == 256, "one thread per histogram bin");
static_assert(CQ_WAVE_MAX == 64 && CQ_WG_MAX > CQ_WAVE_MAX && CQ_WG_MAX * 8 <= 32 * 1024, "class limits");

constexpr unsigned long long CQ_NAN_KEY = 0xFFFFFFFFFFFFFFFFull;
constexpr unsigned long long CQ_NAN_BITS = 0x7FF8000000000000ull;

__host__ __device__ __forceinline__ unsigned long long cq_bits(double v) {
#ifdef __HIP_DEVICE_COMPILE__
  return (unsigned long long)__double_as_longlong(v);
#else
  unsigned long long u;
  memcpy(&u, &v, 8);
  return u;
#endif
}
__host__ __device__ __forceinline__ double cq_from_bits(unsigned long long u) {
#ifdef __HIP_DEVICE_COMPILE__
  return __longlong_as_double((long long)u);
#else
  double v;
  memcpy(&v, &u, 8);
  return v;
#endif
}
// the key of the header: unsigned order = numeric order, -0 before +0, every NaN last
__host__ __device__ __forceinline__ unsigned long long cq_key(double v) {
  if (v != v) return CQ_NAN_KEY;
  const unsigned long long u = cq_bits(v);
  return (u >> 63) ? ~u : u ^ 0x8000000000000000ull;
}
// the value of a key; no number has the NaN key (0x7FFFFFFFFFFFFFFF is a NaN's pattern)
__host__ __device__ __forceinline__ double cq_unkey(unsigned long long k) {
  if (k == CQ_NAN_KEY) return cq_from_bits(CQ_NAN_BITS);
  return cq_from_bits((k >> 63) ? k ^ 0x8000000000000000ull : ~k);
}
// 0-based rank of q in a group of c >= 1 rows: one multiplication
__host__ __device__ __forceinline__ int64_t cq_rank(double q, int64_t c) { return (int64_t)floor(q * (double)(c - 1)); }

__device__ __forceinline__ uint32_t cq_digit(unsigned long long k, int d) { return (uint32_t)(k >> (56 - 8 * d)) & 255u; }
// whether k agrees with prefix p in its first d digits
__device__ __forceinline__ bool cq_match(unsigned long long k, unsigned long long p, int d) {
  return d == 0 || ((k ^ p) >> (64 - 8 * d)) == 0;
}

// skey[t] = the key of the t-th row in (group, row) order; the rows in no group (the slots before segstart[1]) have none
__global__ __launch_bounds__(QT) void k_cq_gather(const double* __restrict__ values, int64_t stride,
                                                  const uint32_t* __restrict__ sorted,
                                                  const uint32_t* __restrict__ segstart, int64_t m,
                                                  unsigned long long* __restrict__ skey) {
  for (int64_t t = (int64_t)segstart[1] + (int64_t)blockIdx.x * QT + threadIdx.x; t < m; t += (int64_t)gridDim.x * QT)
    skey[t] = cq_key(values[(int64_t)sorted[t] * stride]);
}

// per segment 1..K: its chunks and whether it is large (0 for the others and for segment 0), to be scanned
__global__ __launch_bounds__(QT) void k_cq_classify(const uint32_t* __restrict__ counts, int32_t K,
                                                    uint32_t* __restrict__ nch, uint32_t* __restrict__ isl) {
  for (int64_t k = (int64_t)blockIdx.x * QT + threadIdx.x; k <= K; k += (int64_t)gridDim.x * QT) {
    const uint32_t c = counts[k];
    const bool large = k >= 1 && c > (uint32_t)CQ_WG_MAX;
    nch[k] = large ? (c + CQ_HIST_KEYS - 1) / CQ_HIST_KEYS : 0u;
    isl[k] = large ? 1u : 0u;
  }
}

struct CqSel {
  const unsigned long long* skey;
  const uint32_t* segstart;  // [K + 2]
  const uint32_t* counts;    // [K + 1], segment 0 = the rows in no group
  const double* q;           // [nq], device
  int32_t K, nq;
  double* out;               // [K * nq]
  int64_t* out_counts;       // [K] or NULL
};

// One wave per segment of up to CQ_WAVE_MAX keys; also the counts of every segment and the NaN of the empty ones.
__global__ __launch_bounds__(QT) void k_cq_select_wave(CqSel a) {
  const uint32_t lane = threadIdx.x & 63;
  const int64_t nw = (int64_t)gridDim.x * (QT / 64);
  for (int64_t k = (int64_t)blockIdx.x * (QT / 64) + (threadIdx.x >> 6) + 1; k <= a.K; k += nw) {
    const uint32_t c = a.counts[k];  // wave-uniform
    if (lane == 0 && a.out_counts) a.out_counts[k - 1] = (int64_t)c;
    if (c > (uint32_t)CQ_WAVE_MAX) continue;
    double* o = a.out + (size_t)(k - 1) * a.nq;
    if (c == 0) {
      for (int j = lane; j < a.nq; j += 64) o[j] = cq_from_bits(CQ_NAN_BITS);
      continue;
    }
    const unsigned long long key = lane < c ? a.skey[a.segstart[k] + lane] : CQ_NAN_KEY;
    uint32_t below = 0;  // keys before this lane's in (key, lane) order
    for (uint32_t j = 0; j < c; j++) {
      const unsigned long long kj = __shfl(key, (int)j, 64);
      below += (kj < key || (kj == key && j < lane)) ? 1u : 0u;
    }
    for (int j = 0; j < a.nq; j++)
      if (lane < c && (int64_t)below == cq_rank(a.q[j], (int64_t)c)) o[j] = cq_unkey(key);
  }
}

// One workgroup per segment of CQ_WAVE_MAX + 1 .. CQ_WG_MAX keys: the keys in LDS, eight digits per rank.
__global__ __launch_bounds__(QT) void k_cq_select_wg(CqSel a) {
  __shared__ unsigned long long sk[CQ_WG_MAX];
  __shared__ uint32_t hist[QT], sh[8];
  for (int64_t k = (int64_t)blockIdx.x + 1; k <= a.K; k += gridDim.x) {
    const uint32_t c = a.counts[k];  // uniform over the workgroup
    if (c <= (uint32_t)CQ_WAVE_MAX || c > (uint32_t)CQ_WG_MAX) continue;
    __syncthreads();  // the previous segment's keys are read
    const unsigned long long* key = a.skey + a.segstart[k];
    for (uint32_t i = threadIdx.x; i < c; i += QT) sk[i] = key[i];
    for (int j = 0; j < a.nq; j++) {
      unsigned long long p = 0;
      uint32_t r = (uint32_t)cq_rank(a.q[j], (int64_t)c) + 1u;
      for (int d = 0; d < CQ_DIGITS; d++) {
        hist[threadIdx.x] = 0;
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < c; i += QT) {
          const unsigned long long x = sk[i];
          if (cq_match(x, p, d)) atomicAdd(&hist[cq_digit(x, d)], 1u);
        }
        __syncthreads();
        uint32_t g, left;
        vcp_radix_pick(hist[threadIdx.x], r, sh, g, left);
        p |= (unsigned long long)g << (56 - 8 * d);
        r = left;
      }
      if (threadIdx.x == 0) a.out[(size_t)(k - 1) * a.nq + j] = cq_unkey(p);
    }
  }
}

// ---- the large segments: all of them in the same launches ----------------------------------------------------------------
struct CqState {
  unsigned long long prefix;  // the digits chosen so far, the others zero
  uint32_t rank;              // 1-based rank left among the keys that agree with them
  uint32_t seg;               // the segment, 1..K
};
struct CqLarge {
  const uint32_t* chunkstart;  // [K + 2]: first chunk of segment k (the segments that are not large have none)
  const uint32_t* slotof;      // [K + 2]: the large segments before segment k
  uint32_t nchunks, nlarge;
  CqState* state;              // [nlarge * nq]
  uint32_t* ghist;             // [nlarge * nq * 256], zero between the launches of a digit
};

__global__ __launch_bounds__(QT) void k_cq_large_init(CqSel a, CqLarge l) {
  for (int64_t k = (int64_t)blockIdx.x * QT + threadIdx.x + 1; k <= a.K; k += (int64_t)gridDim.x * QT) {
    const uint32_t c = a.counts[k];
    if (c <= (uint32_t)CQ_WG_MAX) continue;
    CqState* s = l.state + (size_t)l.slotof[k] * a.nq;
    for (int j = 0; j < a.nq; j++) s[j] = CqState{0ull, (uint32_t)cq_rank(a.q[j], (int64_t)c) + 1u, (uint32_t)k};
  }
}

// digit d: per chunk the histograms of the keys that agree with each rank's prefix, added to the segment's
__global__ __launch_bounds__(QT) void k_cq_hist(CqSel a, CqLarge l, int d) {
  __shared__ uint32_t hist[CQ_NQ_MAX][QT];
  __shared__ unsigned long long pre[CQ_NQ_MAX];
  for (uint32_t ch = blockIdx.x; ch < l.nchunks; ch += gridDim.x) {
    int lo = 1, hi = a.K;  // the largest k with chunkstart[k] <= ch
    while (lo < hi) {
      const int mid = (int)(((int64_t)lo + hi + 1) >> 1);
      if (l.chunkstart[mid] <= ch) lo = mid; else hi = mid - 1;
    }
    const int k = lo;
    const uint32_t slot = l.slotof[k], c = a.counts[k];
    const uint32_t beg = (ch - l.chunkstart[k]) * (uint32_t)CQ_HIST_KEYS;
    const uint32_t end = beg + CQ_HIST_KEYS < c ? beg + CQ_HIST_KEYS : c;
    __syncthreads();  // the previous chunk's histograms are flushed
    for (int j = 0; j < a.nq; j++) hist[j][threadIdx.x] = 0;
    if ((int)threadIdx.x < a.nq) pre[threadIdx.x] = l.state[(size_t)slot * a.nq + threadIdx.x].prefix;
    __syncthreads();
    const unsigned long long* key = a.skey + a.segstart[k];
    for (uint32_t i = beg + threadIdx.x; i < end; i += QT) {
      const unsigned long long x = key[i];
      const uint32_t g = cq_digit(x, d);
      for (int j = 0; j < a.nq; j++)
        if (cq_match(x, pre[j], d)) atomicAdd(&hist[j][g], 1u);
    }
    __syncthreads();
    for (int j = 0; j < a.nq; j++) {
      const uint32_t v = hist[j][threadIdx.x];
      if (v) atomicAdd(&l.ghist[((size_t)slot * a.nq + j) * QT + threadIdx.x], v);
    }
  }
}

// digit d: per (large segment, rank) the bin the rank falls into; the histogram zero again; after the last digit the value
__global__ __launch_bounds__(QT) void k_cq_pick(CqSel a, CqLarge l, int d) {
  __shared__ uint32_t sh[8];
  const int64_t np = (int64_t)l.nlarge * a.nq;
  for (int64_t p = blockIdx.x; p < np; p += gridDim.x) {
    uint32_t* h = l.ghist + (size_t)p * QT;
    const uint32_t v = h[threadIdx.x];
    h[threadIdx.x] = 0;
    CqState s = l.state[p];
    uint32_t g, left;
    vcp_radix_pick(v, s.rank, sh, g, left);  // ends on a barrier: every thread has read the state
    if (threadIdx.x == 0) {
      s.prefix |= (unsigned long long)g << (56 - 8 * d);
      s.rank = left;
      l.state[p] = s;
      if (d == CQ_DIGITS - 1) a.out[(size_t)(s.seg - 1) * a.nq + (size_t)(p % a.nq)] = cq_unkey(s.prefix);
    }
  }
}

// ---- the MAD chain ---------------------------------------------------------------------------------------------------------
// the keys of a group's rows become the keys of their deviations from the group's median, in place (the key of a number
// gives its bits back; a NaN row's deviation is NaN whichever NaN it was)
__global__ __launch_bounds__(QT) void k_cq_dev(unsigned long long* __restrict__ skey, const uint32_t* __restrict__ sorted,
                                               const uint32_t* __restrict__ segstart,
                                               const int32_t* __restrict__ group, int64_t m,
                                               const double* __restrict__ med) {
  for (int64_t t = (int64_t)segstart[1] + (int64_t)blockIdx.x * QT + threadIdx.x; t < m; t += (int64_t)gridDim.x * QT) {
    const int32_t g = group[sorted[t]];  // within 1..K: the call has checked the labels by now, and group 0 lies before
    if (g >= 1) skey[t] = cq_key(fabs(cq_unkey(skey[t]) - med[g - 1]));
  }
}

__global__ __launch_bounds__(QT) void k_cq_thr(const double* __restrict__ mad, int32_t K, double c_mad, double floor_,
                                               double* __restrict__ thr) {
  for (int64_t k = (int64_t)blockIdx.x * QT + threadIdx.x; k < K; k += (int64_t)gridDim.x * QT) {
    const double band = c_mad * mad[k];
    thr[k] = band > floor_ ? band : floor_;  // a NaN band gives the floor
  }
}

// reject per row in row order; rej[k] = rejected rows of group k + 1, *total = all of them.  A workgroup takes a contiguous
// span of rows, and a wave adds to a group's counter when the group of its rejected rows changes, not per row: the rows
// of a file are consecutive, and 64 adds per wave on one of twenty words would take longer than the selects.
__global__ __launch_bounds__(QT) void k_cq_flag(const double* __restrict__ values, int64_t stride,
                                                const int32_t* __restrict__ group, int64_t n,
                                                const double* __restrict__ med, const double* __restrict__ thr,
                                                uint8_t* __restrict__ reject, uint32_t* __restrict__ rej,
                                                unsigned long long* __restrict__ total) {
  __shared__ uint32_t cnt;
  if (threadIdx.x == 0) cnt = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int64_t span = ((n + gridDim.x - 1) / gridDim.x + QT - 1) / QT * QT;
  const int64_t beg = (int64_t)blockIdx.x * span, end = beg + span < n ? beg + span : n;
  int32_t cur_g = 0;  // wave-uniform: the group whose count is pending, and the count
  uint32_t cur_c = 0, all = 0;
  for (int64_t base = beg; base < end; base += QT) {  // uniform over the block
    const int64_t i = base + threadIdx.x;
    const int32_t g = i < end ? group[i] : 0;
    bool r = false;
    if (g >= 1) r = !(fabs(values[i * stride] - med[g - 1]) <= thr[g - 1]);
    if (i < end) reject[i] = r ? 1 : 0;
    unsigned long long todo = __ballot(r);
    while (todo) {  // wave-uniform
      const int32_t gl = __shfl(g, __ffsll((long long)todo) - 1, 64);
      const unsigned long long same = __ballot(r && g == gl);
      if (gl != cur_g) {
        if (cur_c && lane == 0) atomicAdd(&rej[cur_g - 1], cur_c);
        cur_g = gl;
        cur_c = 0;
      }
      cur_c += (uint32_t)__popcll(same);
      all += (uint32_t)__popcll(same);
      todo &= ~same;
    }
  }
  if (cur_c && lane == 0) atomicAdd(&rej[cur_g - 1], cur_c);
  if (all && lane == 0) atomicAdd(&cnt, all);
  __syncthreads();
  if (threadIdx.x == 0 && cnt) atomicAdd(total, (unsigned long long)cnt);
}

__global__ __launch_bounds__(QT) void k_cq_kept(const uint32_t* __restrict__ counts, const uint32_t* __restrict__ rej,
                                                int32_t K, int64_t* __restrict__ kept) {
  for (int64_t k = (int64_t)blockIdx.x * QT + threadIdx.x; k < K; k += (int64_t)gridDim.x * QT)
    kept[k] = (int64_t)counts[k + 1] - (int64_t)rej[k];
}

// ---- host drivers ------------------------------------------------------------------------------------------------------------
// The grouped rows of a call.  b_cq_misc: [counts | segstart | chunkstart | slotof | rej] (K + 4 or K + 5 words each), 16 counter
// words (0 bad labels, 4 chunks, 5 large segments, 8-9 the rejected rows), 32 doubles (the caller's q, then 0.5).
struct CqWork {
  uint32_t *counts, *segstart, *chunkstart, *slotof, *rej, *ctr;
  double* dq;
  const uint32_t* sorted;
  unsigned long long* skey;
  uint32_t nchunks, nlarge;
  unsigned walk;  // workgroups of a grid that walks: eight per compute unit
};

unsigned cq_grid(const CqWork& w, int64_t items, int per_block) { return vcp_blocks(items, per_block, (int)w.walk); }

// Phase cq_group: the rows in (group, row) order, their keys, the large segments' chunks; the one read-back of the call
// before any output is touched (bad labels, chunks, large segments).  q [nq] host, already checked.
int cq_group(vcp_ctx* ctx, const double* d_values, int64_t stride, const int32_t* d_group, int64_t n, int32_t K,
             const double* q, int nq, CqWork& w) {
  hipStream_t st = ctx->stream;
  vcp_phase(ctx, "cq_group");
  const size_t kk = ((size_t)K + 5) & ~(size_t)1;  // even: the 64-bit words behind the arrays stay aligned
  const size_t words = 5 * kk + 16;
  VCP_TRY(vcp_ensure(ctx, ctx->b_cq_misc, words * 4 + 32 * 8));
  VCP_TRY(vcp_ensure(ctx, ctx->b_aux4, (size_t)(n > 0 ? n : 1) * 8));
  w.counts = ctx->b_cq_misc.as<uint32_t>();
  w.segstart = w.counts + kk;
  w.chunkstart = w.segstart + kk;
  w.slotof = w.chunkstart + kk;
  w.rej = w.slotof + kk;
  w.ctr = w.rej + kk;
  w.dq = reinterpret_cast<double*>(w.counts + words);
  w.skey = ctx->b_aux4.as<unsigned long long>();
  w.walk = (unsigned)(ctx->prop.multiProcessorCount > 0 ? ctx->prop.multiProcessorCount : 256) * 8u;
  VCP_HIP(ctx, hipMemsetAsync(w.counts, 0, words * 4, st));
  char* hp = static_cast<char*>(ctx->pinned);
  double* hq = reinterpret_cast<double*>(hp + 128);  // [128, 392) of the pinned scratch: q on its way to the device
  for (int j = 0; j < CQ_NQ_MAX; j++) hq[j] = j < nq ? q[j] : 0.0;
  hq[CQ_NQ_MAX] = 0.5;
  VCP_HIP(ctx, hipMemcpyAsync(w.dq, hq, (CQ_NQ_MAX + 1) * 8, hipMemcpyHostToDevice, st));
  VCP_TRY(vcp_group_by_label(ctx, d_group, nullptr, n, K, ctx->b_aux1, ctx->b_aux2, ctx->b_aux3, w.segstart, w.counts,
                             w.ctr, &w.sorted));
  if (n > 0)
    VCP_LAUNCH(ctx, k_cq_gather, dim3(cq_grid(w, n, QT)), dim3(QT), 0, st, d_values, stride, w.sorted, w.segstart, n,
               w.skey);
  VCP_LAUNCH(ctx, k_cq_classify, dim3(cq_grid(w, (int64_t)K + 1, QT)), dim3(QT), 0, st, w.counts, K, w.chunkstart,
             w.slotof);
  VCP_TRY(vcp_exclusive_scan_u32(ctx, w.chunkstart, w.chunkstart, (int64_t)K + 2, w.ctr + 4));
  VCP_TRY(vcp_exclusive_scan_u32(ctx, w.slotof, w.slotof, (int64_t)K + 2, w.ctr + 5));
  uint32_t* hc = reinterpret_cast<uint32_t*>(hp);
  VCP_HIP(ctx, hipMemcpyAsync(hc, w.ctr, 8 * 4, hipMemcpyDeviceToHost, st));
  VCP_HIP(ctx, hipStreamSynchronize(st));
  if (hc[0] != 0) return vcp_fail(ctx, VCP_ERR_INDEX, "%u labels outside 0..K", hc[0]);
  w.nchunks = hc[4];
  w.nlarge = hc[5];
  return VCP_OK;
}

// every segment's nq ranks into d_out [K * nq]; d_counts [K] may be NULL
int cq_select(vcp_ctx* ctx, const CqWork& w, int32_t K, const double* dq, int nq, double* d_out, int64_t* d_counts) {
  if (K == 0) return VCP_OK;
  hipStream_t st = ctx->stream;
  const CqSel a{w.skey, w.segstart, w.counts, dq, K, nq, d_out, d_counts};
  VCP_LAUNCH(ctx, k_cq_select_wave, dim3(cq_grid(w, K, QT / 64)), dim3(QT), 0, st, a);
  VCP_LAUNCH(ctx, k_cq_select_wg, dim3(cq_grid(w, K, 1)), dim3(QT), 0, st, a);
  if (w.nlarge == 0) return VCP_OK;
  const size_t np = (size_t)w.nlarge * nq;
  VCP_TRY(vcp_ensure(ctx, ctx->b_cq_large, np * sizeof(CqState) + np * QT * 4));
  const CqLarge l{w.chunkstart, w.slotof, w.nchunks, w.nlarge, ctx->b_cq_large.as<CqState>(),
                  reinterpret_cast<uint32_t*>(ctx->b_cq_large.as<CqState>() + np)};
  VCP_HIP(ctx, hipMemsetAsync(l.ghist, 0, np * QT * 4, st));
  VCP_LAUNCH(ctx, k_cq_large_init, dim3(cq_grid(w, K, QT)), dim3(QT), 0, st, a, l);
  for (int d = 0; d < CQ_DIGITS; d++) {
    VCP_LAUNCH(ctx, k_cq_hist, dim3(cq_grid(w, w.nchunks, 1)), dim3(QT), 0, st, a, l, d);
    VCP_LAUNCH(ctx, k_cq_pick, dim3(cq_grid(w, (int64_t)np, 1)), dim3(QT), 0, st, a, l, d);
  }
  return VCP_OK;
}

bool cq_bad_q(double q) { return !(q >= 0.0 && q <= 1.0); }

int cq_check(vcp_ctx* ctx, const void* values, int64_t stride, const void* group, int64_t n, int32_t K) {
  if (n < 0 || K < 0 || stride < 1) return vcp_fail(ctx, VCP_ERR_ARG, "n < 0, K < 0 or stride < 1");
  if (n > 0 && (!values || !group)) return vcp_fail(ctx, VCP_ERR_ARG, "null values or group");
  return VCP_OK;
}
int cq_check_q(vcp_ctx* ctx, const double* q, int32_t nq, const void* out, int32_t K) {
  if (!q || nq < 1 || (K > 0 && !out)) return vcp_fail(ctx, VCP_ERR_ARG, "null q or out, or nq < 1");
  if (nq > CQ_NQ_MAX) return vcp_fail(ctx, VCP_ERR_UNSUPPORTED, "nq %d beyond %d", nq, CQ_NQ_MAX);
  for (int j = 0; j < nq; j++)
    if (cq_bad_q(q[j])) return vcp_fail(ctx, VCP_ERR_ARG, "q[%d] is NaN or outside [0, 1]", j);
  return VCP_OK;
}
int cq_check_mad(vcp_ctx* ctx, double c_mad, double floor_, const void* med, const void* mad, const void* thr,
                 const void* reject, const void* kept, const void* n_rejected, int64_t n, int32_t K) {
  if (!(c_mad >= 0.0) || !(floor_ >= 0.0)) return vcp_fail(ctx, VCP_ERR_ARG, "c_mad or floor is NaN or < 0");
  if (!n_rejected || (n > 0 && !reject) || (K > 0 && (!med || !mad || !thr || !kept)))
    return vcp_fail(ctx, VCP_ERR_ARG, "null output");
  return VCP_OK;
}
int cq_check_n(vcp_ctx* ctx, int64_t n) {
  if (n >= ((int64_t)1 << 31)) return vcp_fail(ctx, VCP_ERR_TOO_LARGE, "n beyond int32 indices");
  return VCP_OK;
}

// doubles of the caller's array that n rows at `stride` span
size_t cq_span(int64_t n, int64_t stride) { return n > 0 ? (size_t)(n - 1) * (size_t)stride + 1 : 0; }
}  // namespace

extern "C" {

int vcp_cluster_quantiles_dev(vcp_ctx* ctx, const double* d_values, int64_t stride, const int32_t* d_group, int64_t n,
                              int32_t K, const double* q, int32_t nq, double* d_out, int64_t* d_counts) {
  if (!ctx) return VCP_ERR_ARG;
  VCP_TRY(cq_check(ctx, d_values, stride, d_group, n, K));
  VCP_TRY(cq_check_q(ctx, q, nq, d_out, K));
  VCP_TRY(cq_check_n(ctx, n));
  VCP_TRY(vcp_bind(ctx));
  vcp_phase_reset(ctx);
  CqWork w{};
  VCP_TRY(cq_group(ctx, d_values, stride, d_group, n, K, q, nq, w));
  vcp_phase(ctx, "cq_select");
  VCP_TRY(cq_select(ctx, w, K, w.dq, nq, d_out, d_counts));
  VCP_TRY(vcp_phase_finish(ctx));
  VCP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return VCP_OK;
}

int vcp_cluster_quantiles(vcp_ctx* ctx, const double* values, int64_t stride, const int32_t* group, int64_t n, int32_t K,
                          const double* q, int32_t nq, double* out, int64_t* counts) {
  if (!ctx) return VCP_ERR_ARG;
  VCP_TRY(cq_check(ctx, values, stride, group, n, K));
  VCP_TRY(cq_check_q(ctx, q, nq, out, K));
  VCP_TRY(cq_check_n(ctx, n));
  VCP_TRY(vcp_bind(ctx));
  hipStream_t st = ctx->stream;
  // in: [values span * 8 | group n * 4]; out: [out K * nq * 8 | counts K * 8]
  const size_t span = cq_span(n, stride), kq = (size_t)K * nq;
  VCP_TRY(vcp_ensure(ctx, ctx->b_cq_in, span * 8 + (size_t)n * 4));
  VCP_TRY(vcp_ensure(ctx, ctx->b_cq_out, kq * 8 + (size_t)K * 8));
  char* din = ctx->b_cq_in.as<char>();
  char* dout = ctx->b_cq_out.as<char>();
  if (n > 0) {
    VCP_HIP(ctx, hipMemcpyAsync(din, values, span * 8, hipMemcpyHostToDevice, st));
    VCP_HIP(ctx, hipMemcpyAsync(din + span * 8, group, (size_t)n * 4, hipMemcpyHostToDevice, st));
  }
  VCP_TRY(vcp_cluster_quantiles_dev(ctx, reinterpret_cast<const double*>(din), stride,
                                    reinterpret_cast<const int32_t*>(din + span * 8), n, K, q, nq,
                                    reinterpret_cast<double*>(dout), reinterpret_cast<int64_t*>(dout + kq * 8)));
  if (K > 0) {
    VCP_HIP(ctx, hipMemcpyAsync(out, dout, kq * 8, hipMemcpyDeviceToHost, st));
    if (counts) VCP_HIP(ctx, hipMemcpyAsync(counts, dout + kq * 8, (size_t)K * 8, hipMemcpyDeviceToHost, st));
    VCP_HIP(ctx, hipStreamSynchronize(st));
  }
  return VCP_OK;
}

int vcp_cluster_mad_dev(vcp_ctx* ctx, const double* d_values, int64_t stride, const int32_t* d_group, int64_t n,
                        int32_t K, double c_mad, double floor, double* d_med, double* d_mad, double* d_thr,
                        uint8_t* d_reject, int64_t* d_kept, int64_t* n_rejected) {
  if (!ctx) return VCP_ERR_ARG;
  VCP_TRY(cq_check(ctx, d_values, stride, d_group, n, K));
  VCP_TRY(cq_check_mad(ctx, c_mad, floor, d_med, d_mad, d_thr, d_reject, d_kept, n_rejected, n, K));
  VCP_TRY(cq_check_n(ctx, n));
  VCP_TRY(vcp_bind(ctx));
  vcp_phase_reset(ctx);
  hipStream_t st = ctx->stream;
  CqWork w{};
  const double half = 0.5;
  VCP_TRY(cq_group(ctx, d_values, stride, d_group, n, K, &half, 1, w));
  vcp_phase(ctx, "cq_select");
  VCP_TRY(cq_select(ctx, w, K, w.dq + CQ_NQ_MAX, 1, d_med, nullptr));
  if (n > 0 && K > 0)
    VCP_LAUNCH(ctx, k_cq_dev, dim3(cq_grid(w, n, QT)), dim3(QT), 0, st, w.skey, w.sorted, w.segstart, d_group, n,
               d_med);
  VCP_TRY(cq_select(ctx, w, K, w.dq + CQ_NQ_MAX, 1, d_mad, nullptr));
  vcp_phase(ctx, "cq_flag");
  unsigned long long* total = reinterpret_cast<unsigned long long*>(w.ctr + 8);
  if (K > 0) VCP_LAUNCH(ctx, k_cq_thr, dim3(cq_grid(w, K, QT)), dim3(QT), 0, st, d_mad, K, c_mad, floor, d_thr);
  if (n > 0)
    VCP_LAUNCH(ctx, k_cq_flag, dim3(cq_grid(w, n, QT)), dim3(QT), 0, st, d_values, stride, d_group, n, d_med, d_thr,
               d_reject, w.rej, total);
  if (K > 0) VCP_LAUNCH(ctx, k_cq_kept, dim3(cq_grid(w, K, QT)), dim3(QT), 0, st, w.counts, w.rej, K, d_kept);
  unsigned long long* ht = reinterpret_cast<unsigned long long*>(static_cast<char*>(ctx->pinned) + 64);
  VCP_HIP(ctx, hipMemcpyAsync(ht, total, 8, hipMemcpyDeviceToHost, st));
  VCP_TRY(vcp_phase_finish(ctx));
  VCP_HIP(ctx, hipStreamSynchronize(st));
  *n_rejected = (int64_t)*ht;
  return VCP_OK;
}

int vcp_cluster_mad(vcp_ctx* ctx, const double* values, int64_t stride, const int32_t* group, int64_t n, int32_t K,
                    double c_mad, double floor, double* med, double* mad, double* thr, uint8_t* reject, int64_t* kept,
                    int64_t* n_rejected) {
  if (!ctx) return VCP_ERR_ARG;
  VCP_TRY(cq_check(ctx, values, stride, group, n, K));
  VCP_TRY(cq_check_mad(ctx, c_mad, floor, med, mad, thr, reject, kept, n_rejected, n, K));
  VCP_TRY(cq_check_n(ctx, n));
  VCP_TRY(vcp_bind(ctx));
  hipStream_t st = ctx->stream;
  // in: [values span * 8 | group n * 4]; out: [med | mad | thr | kept (K * 8 each) | reject n]
  const size_t span = cq_span(n, stride), k8 = (size_t)K * 8;
  VCP_TRY(vcp_ensure(ctx, ctx->b_cq_in, span * 8 + (size_t)n * 4));
  VCP_TRY(vcp_ensure(ctx, ctx->b_cq_out, 4 * k8 + (size_t)n));
  char* din = ctx->b_cq_in.as<char>();
  char* dout = ctx->b_cq_out.as<char>();
  if (n > 0) {
    VCP_HIP(ctx, hipMemcpyAsync(din, values, span * 8, hipMemcpyHostToDevice, st));
    VCP_HIP(ctx, hipMemcpyAsync(din + span * 8, group, (size_t)n * 4, hipMemcpyHostToDevice, st));
  }
  int64_t nr = 0;
  VCP_TRY(vcp_cluster_mad_dev(ctx, reinterpret_cast<const double*>(din), stride,
                              reinterpret_cast<const int32_t*>(din + span * 8), n, K, c_mad, floor,
                              reinterpret_cast<double*>(dout), reinterpret_cast<double*>(dout + k8),
                              reinterpret_cast<double*>(dout + 2 * k8), reinterpret_cast<uint8_t*>(dout + 4 * k8),
                              reinterpret_cast<int64_t*>(dout + 3 * k8), &nr));
  if (K > 0) {
    VCP_HIP(ctx, hipMemcpyAsync(med, dout, k8, hipMemcpyDeviceToHost, st));
    VCP_HIP(ctx, hipMemcpyAsync(mad, dout + k8, k8, hipMemcpyDeviceToHost, st));
    VCP_HIP(ctx, hipMemcpyAsync(thr, dout + 2 * k8, k8, hipMemcpyDeviceToHost, st));
    VCP_HIP(ctx, hipMemcpyAsync(kept, dout + 3 * k8, k8, hipMemcpyDeviceToHost, st));
  }
  if (n > 0) VCP_HIP(ctx, hipMemcpyAsync(reject, dout + 4 * k8, (size_t)n, hipMemcpyDeviceToHost, st));
  VCP_HIP(ctx, hipStreamSynchronize(st));
  *n_rejected = nr;
  return VCP_OK;
}

int vcp_selftest_rank_key(double v, double q, int64_t c, uint64_t* key, int64_t* rank) {
  if (!key || !rank || c < 1 || cq_bad_q(q)) return VCP_ERR_ARG;
  *key = (uint64_t)cq_key(v);
  *rank = cq_rank(q, c);
  return 1;
}

}  // extern "C"
