// scanfmt.hip -- vcp_format_rows: resident columns in, the bytes of an export file out (`[id<TAB>]a<TAB>b<TAB>c<EOL>`, "F<bit>":
// BC/Tools.cs:233, 295, 341, 374); the inverse of scantext.hip.  The bytes are those of vtkcloudpoint_amd.io's writers.
//
//   k_fmt_len     one lane per output line: gathers through `order`, rounds its three numbers (scanfmt.hpp) and takes the
//                 line's exact length from the rounded values; lowers one 64-bit minimum for an entry of `order` outside
//                 [0, n) and one for an unsupported value; one total per workgroup
//   k_fmt_sum     the 64-bit sum of the workgroup totals: the byte count, exact (the 32-bit scan below wraps beyond 2^32)
//   (the context's scan over the totals places every workgroup's span)
//   k_fmt_write   one workgroup per 256 lines, whose span of the text is contiguous: the lanes round their numbers again
//                 and scan their lengths; STAGE: the lines are written into LDS at the span's alignment and the workgroup
//                 copies the span out with aligned 16-byte stores (head and tail bytes one by one); otherwise every lane
//                 stores its own bytes to global memory
// include/vcp.h holds the contract; DESIGN.md section 31 the measurements.
#include <cstdlib>
#include <cstring>
#include <vector>

#include "scanfmt.hpp"
#include "vcp_ctx.hpp"
#include "wave.hpp"

static_assert(sfx::LINE_BYTES_MAX == VCP_FMT_LINE_MAX, "include/vcp.h: VCP_FMT_LINE_MAX");

namespace {
constexpr int TT = 256;
constexpr unsigned long long NONE = ~0ull;
constexpr bool STAGE_DEFAULT = true;  // staged against direct

struct Cols {
  const int32_t* id;
  const double *a, *b, *c;
  int64_t sa, sb, sc;
  const int64_t* order;
  int64_t n, m;
  int bit, eol;
};

// Line j of the output: 0 = its id and rounded numbers are in place, 1 = order[j] is outside [0, n), 2 + k = column k is
// the first one that holds an unsupported value.
__device__ __forceinline__ int load_line(const Cols& q, int64_t j, int32_t* id, sfx::Field f[3]) {
  const int64_t r = q.order ? q.order[j] : j;
  if (r < 0 || r >= q.n) return 1;
  *id = q.id ? q.id[r] : 0;
  if (!sfx::split(q.a[r * q.sa], q.bit, &f[0])) return 2;
  if (!sfx::split(q.b[r * q.sb], q.bit, &f[1])) return 3;
  if (!sfx::split(q.c[r * q.sc], q.bit, &f[2])) return 4;
  return 0;
}

// counters[0]: the first j whose order[j] is out of range; counters[1]: the minimum of (j << 2 | column) over the
// unsupported values
__global__ __launch_bounds__(TT) void k_fmt_len(const Cols q, uint32_t* __restrict__ wg_total,
                                               unsigned long long* __restrict__ counters) {
  const int64_t j = (int64_t)blockIdx.x * TT + threadIdx.x;
  unsigned len = 0;
  if (j < q.m) {
    int32_t id;
    sfx::Field f[3];
    const int st = load_line(q, j, &id, f);
    if (st == 0) len = (unsigned)sfx::line_len(q.id != nullptr, id, f, q.bit, q.eol);
    else if (st == 1) atomicMin(&counters[0], (unsigned long long)j);
    else atomicMin(&counters[1], (unsigned long long)j << 2 | (unsigned)(st - 2));
  }
  len = wave_all<WaveAdd>(len);
  __shared__ unsigned wt[TT / 64];
  if ((threadIdx.x & 63) == 0) wt[threadIdx.x >> 6] = len;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned s = 0;
    for (int k = 0; k < TT / 64; k++) s += wt[k];
    wg_total[blockIdx.x] = s;
  }
}

// one workgroup: *total = the sum of nb words in 64 bits
__global__ __launch_bounds__(TT) void k_fmt_sum(const uint32_t* __restrict__ wg_total, int64_t nb,
                                               unsigned long long* __restrict__ total) {
  unsigned long long s = 0;
  for (int64_t i = threadIdx.x; i < nb; i += TT) s += wg_total[i];
  s = wave_all<WaveAdd>(s);
  __shared__ unsigned long long wt[TT / 64];
  if ((threadIdx.x & 63) == 0) wt[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long t = 0;
    for (int k = 0; k < TT / 64; k++) t += wt[k];
    *total = t;
  }
}

// wg_off = the exclusive scan of wg_total (the text is below 2^32 bytes).  text has room for the whole output.
constexpr int STAGE_BYTES = TT * sfx::LINE_BYTES_MAX + 16;  // the longest span, placed at the span's offset within 16 bytes
static_assert(STAGE_BYTES % 16 == 0 && STAGE_BYTES <= 32768, "k_fmt_write's LDS");
template <bool STAGE>
__global__ __launch_bounds__(TT) void k_fmt_write(const Cols q, const uint32_t* __restrict__ wg_off,
                                                 char* __restrict__ text) {
  __shared__ uint4 sbuf[STAGE ? STAGE_BYTES / 16 : 1];
  __shared__ unsigned wt[TT / 64];
  const int64_t j = (int64_t)blockIdx.x * TT + threadIdx.x;
  unsigned len = 0;
  int32_t id = 0;
  sfx::Field f[3];
  bool live = false;
  if (j < q.m) {
    live = load_line(q, j, &id, f) == 0;  // k_fmt_len found every line of this call good
    if (live) len = (unsigned)sfx::line_len(q.id != nullptr, id, f, q.bit, q.eol);
  }
  uint32_t tot;
  const uint32_t before = block_excl<TT>(len, wt, tot);
  const uint32_t base = wg_off[blockIdx.x];
  if (STAGE) {
    const unsigned mis = base & 15u;
    if (mis + tot <= (unsigned)STAGE_BYTES) {  // the same for every lane; true by the bound on a line
      char* sb = reinterpret_cast<char*>(sbuf) + mis;
      if (live) sfx::put_line(sb + before, q.id != nullptr, id, f, q.bit, q.eol);
      __syncthreads();
      char* g = text + base;
      const unsigned to_align = (16u - mis) & 15u, head = to_align < tot ? to_align : tot;
      if (threadIdx.x < head) g[threadIdx.x] = sb[threadIdx.x];
      const unsigned nvec = (tot - head) >> 4;  // sb + head and g + head are both 16-byte aligned
      uint4* gv = reinterpret_cast<uint4*>(g + head);
      const uint4* sv = reinterpret_cast<const uint4*>(sb + head);
      for (unsigned v = threadIdx.x; v < nvec; v += TT) gv[v] = sv[v];
      const unsigned t0 = head + (nvec << 4) + threadIdx.x;  // fewer than 16 bytes are left
      if (t0 < tot) g[t0] = sb[t0];
      return;
    }
  }
  if (live) sfx::put_line(text + base + before, q.id != nullptr, id, f, q.bit, q.eol);
}

// VCP_FMT_DIRECT (developer switch for tools/bench_format_text.py and the tests, read at every call): 1 takes the kernel
// without the LDS staging, 0 the staged one; unset or empty, the default
bool use_stage() {
  const char* sw = getenv("VCP_FMT_DIRECT");
  if (!sw || sw[0] == '\0') return STAGE_DEFAULT;
  return sw[0] == '0' && sw[1] == '\0';
}

// both forms.  dev: id, a, b, c and order are device pointers; otherwise host pointers, packed and uploaded
int fmt_impl(vcp_ctx* ctx, const int32_t* id, const double* a, int64_t sa, const double* b, int64_t sb, const double* c,
             int64_t sc, const int64_t* order, int64_t n, int64_t m, int bit, int eol, char* text, uint64_t cap,
             uint64_t* nbytes, int64_t* err, bool dev) {
  if (!ctx) return VCP_ERR_ARG;
  if (!nbytes || n < 0 || m < 0 || sa < 1 || sb < 1 || sc < 1 || bit < 0 || bit > sfx::BIT_MAX || eol < 0 || eol > 1 ||
      (!order && m != n) || (m > 0 && (!a || !b || !c)))
    return vcp_fail(ctx, VCP_ERR_ARG, "bad argument");
  if (m >= ((int64_t)1 << 31))
    return vcp_fail(ctx, VCP_ERR_TOO_LARGE, "%lld lines: the text would reach 2^32 bytes", (long long)m);
  int64_t err_local[2];
  if (!err) err = err_local;
  err[0] = err[1] = 0;
  VCP_TRY(vcp_bind(ctx));
  vcp_phase_reset(ctx);
  if (m == 0) {
    ctx->last_timing.clear();
    *nbytes = 0;
    return VCP_OK;
  }
  hipStream_t st = ctx->stream;
  Cols q{id, a, b, c, sa, sb, sc, order, n, m, bit, eol};
  vcp_phase(ctx, "fmt_len");
  std::vector<double> pack;  // the host form's columns, side by side
  if (!dev) {
    const size_t o_id = (size_t)n * 24, o_order = (o_id + (id ? (size_t)n * 4 : 0) + 7) / 8 * 8;
    VCP_TRY(vcp_ensure(ctx, ctx->b_fm_in, o_order + (order ? (size_t)m * 8 : 0) + 8));
    char* in = ctx->b_fm_in.as<char>();
    if (n > 0) {
      pack.resize((size_t)n * 3);
      for (int64_t i = 0; i < n; i++) {
        pack[(size_t)i] = a[i * sa];
        pack[(size_t)(n + i)] = b[i * sb];
        pack[(size_t)(2 * n + i)] = c[i * sc];
      }
      VCP_HIP(ctx, hipMemcpyAsync(in, pack.data(), (size_t)n * 24, hipMemcpyHostToDevice, st));
      if (id) VCP_HIP(ctx, hipMemcpyAsync(in + o_id, id, (size_t)n * 4, hipMemcpyHostToDevice, st));
    }
    if (order) VCP_HIP(ctx, hipMemcpyAsync(in + o_order, order, (size_t)m * 8, hipMemcpyHostToDevice, st));
    VCP_HIP(ctx, hipStreamSynchronize(st));  // `pack` and the caller's arrays have been read
    q.a = reinterpret_cast<const double*>(in);
    q.b = q.a + n;
    q.c = q.a + 2 * n;
    q.sa = q.sb = q.sc = 1;
    q.id = id ? reinterpret_cast<const int32_t*>(in + o_id) : nullptr;
    q.order = order ? reinterpret_cast<const int64_t*>(in + o_order) : nullptr;
  }
  const unsigned nb = vcp_blocks(m, TT);
  VCP_TRY(vcp_ensure(ctx, ctx->b_fm_wg, (size_t)nb * 4));
  VCP_TRY(vcp_ensure(ctx, ctx->b_fm_misc, 64));
  uint32_t* d_wg = ctx->b_fm_wg.as<uint32_t>();
  // misc: [0, 8) the first bad entry of order, [8, 16) the first unsupported value, [16, 24) the byte count,
  // [24, 32) the entry of order that [0, 8) names, [32, 36) the scan's (wrapping) total
  unsigned long long* d_counters = ctx->b_fm_misc.as<unsigned long long>();
  VCP_HIP(ctx, hipMemsetAsync(d_counters, 0xFF, 16, st));
  VCP_LAUNCH(ctx, k_fmt_len, dim3(nb), dim3(TT), 0, st, q, d_wg, d_counters);
  VCP_LAUNCH(ctx, k_fmt_sum, dim3(1), dim3(TT), 0, st, d_wg, (int64_t)nb, d_counters + 2);
  VCP_TRY(vcp_exclusive_scan_u32(ctx, d_wg, d_wg, nb, reinterpret_cast<uint32_t*>(d_counters + 4)));
  unsigned long long* hp = reinterpret_cast<unsigned long long*>(ctx->pinned);  // [0, 32): a copy of the head of misc
  VCP_HIP(ctx, hipMemcpyAsync(hp, d_counters, 24, hipMemcpyDeviceToHost, st));
  VCP_HIP(ctx, hipStreamSynchronize(st));
  if (hp[0] != NONE) {
    const int64_t j = (int64_t)hp[0];
    VCP_HIP(ctx, hipMemcpyAsync(hp + 3, q.order + j, 8, hipMemcpyDeviceToHost, st));  // order != NULL: r = j is in range
    VCP_HIP(ctx, hipStreamSynchronize(st));
    err[0] = j;
    err[1] = (int64_t)hp[3];
    return vcp_fail(ctx, VCP_ERR_INDEX, "order[%lld] = %lld is outside [0, %lld)", (long long)j, (long long)err[1],
                    (long long)n);
  }
  if (hp[1] != NONE) {
    err[0] = (int64_t)(hp[1] >> 2);
    err[1] = (int64_t)(hp[1] & 3u);
    return vcp_fail(ctx, VCP_ERR_UNSUPPORTED, "line %lld column %lld: the device formatter takes finite values below 1e15 in "
                    "magnitude", (long long)err[0], (long long)err[1]);
  }
  const uint64_t total = hp[2];
  if (total >= ((uint64_t)1 << 32))
    return vcp_fail(ctx, VCP_ERR_TOO_LARGE, "text of %llu bytes: offsets are 32 bits", (unsigned long long)total);
  *nbytes = total;
  if (!text) return vcp_phase_finish(ctx);
  if (total > cap)
    return vcp_fail(ctx, VCP_ERR_INDEX, "%llu bytes for a capacity of %llu", (unsigned long long)total,
                    (unsigned long long)cap);
  vcp_phase(ctx, "fmt_write");
  VCP_TRY(vcp_ensure(ctx, ctx->b_fm_text, (size_t)total + 16));
  char* d_text = ctx->b_fm_text.as<char>();
  if (use_stage()) VCP_LAUNCH(ctx, k_fmt_write<true>, dim3(nb), dim3(TT), 0, st, q, d_wg, d_text);
  else VCP_LAUNCH(ctx, k_fmt_write<false>, dim3(nb), dim3(TT), 0, st, q, d_wg, d_text);
  vcp_phase(ctx, "fmt_download");
  VCP_HIP(ctx, hipMemcpyAsync(text, d_text, (size_t)total, hipMemcpyDeviceToHost, st));
  VCP_TRY(vcp_phase_finish(ctx));
  VCP_HIP(ctx, hipStreamSynchronize(st));
  return VCP_OK;
}
}  // namespace

extern "C" int vcp_format_rows(vcp_ctx* ctx, const int32_t* id, const double* a, int64_t stride_a, const double* b,
                               int64_t stride_b, const double* c, int64_t stride_c, const int64_t* order, int64_t n,
                               int64_t m, int bit, int eol, char* text, uint64_t cap, uint64_t* nbytes, int64_t err[2]) {
  return fmt_impl(ctx, id, a, stride_a, b, stride_b, c, stride_c, order, n, m, bit, eol, text, cap, nbytes, err, false);
}

extern "C" int vcp_format_rows_dev(vcp_ctx* ctx, const int32_t* d_id, const double* d_a, int64_t stride_a,
                                   const double* d_b, int64_t stride_b, const double* d_c, int64_t stride_c,
                                   const int64_t* d_order, int64_t n, int64_t m, int bit, int eol, char* text, uint64_t cap,
                                   uint64_t* nbytes, int64_t err[2]) {
  return fmt_impl(ctx, d_id, d_a, stride_a, d_b, stride_b, d_c, stride_c, d_order, n, m, bit, eol, text, cap, nbytes, err,
                  true);
}

extern "C" int vcp_selftest_format_field(double v, int bit, char* out, int64_t cap, int64_t* len) {
  if (!out || !len || bit < 0 || bit > sfx::BIT_MAX) return VCP_ERR_ARG;
  sfx::Field f;
  if (!sfx::split(v, bit, &f)) return 0;
  *len = sfx::field_len(f, bit);
  if (cap < *len) return VCP_ERR_ARG;
  sfx::put_field(out, f, bit);
  return 1;
}

extern "C" int vcp_selftest_format_total_dev(vcp_ctx* ctx, const uint32_t* d_totals, int64_t n, uint64_t* total) {
  if (!ctx) return VCP_ERR_ARG;
  if (!total || n < 0 || (n > 0 && !d_totals)) return vcp_fail(ctx, VCP_ERR_ARG, "bad argument");
  VCP_TRY(vcp_bind(ctx));
  VCP_TRY(vcp_ensure(ctx, ctx->b_fm_misc, 64));
  unsigned long long* d_counters = ctx->b_fm_misc.as<unsigned long long>();
  VCP_LAUNCH(ctx, k_fmt_sum, dim3(1), dim3(TT), 0, ctx->stream, d_totals, n, d_counters + 2);
  unsigned long long* hp = reinterpret_cast<unsigned long long*>(ctx->pinned);
  VCP_HIP(ctx, hipMemcpyAsync(hp, d_counters + 2, 8, hipMemcpyDeviceToHost, ctx->stream));
  VCP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  *total = hp[0];
  return VCP_OK;
}
