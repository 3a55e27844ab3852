// scantext.hip -- vcp_parse_scan_text: the bytes of scan files (`motor_x<TAB>motor_y<TAB>Distance`, one point per line:
// FileMap.ReadFile + FrmMain.cs:1005-1009, written back by Tools.cs:233) in, rows [n, 3] and the file number of every row
// out, in HBM, in the layout vcp_import_compact_dev takes (the other half of the import row).
//
//   k_txt_count   one workgroup per VCP_TXT_CHUNK bytes: line terminators per chunk, the first unsupported byte
//   (the context's scan over the chunk counts; the host reads n and the bad-byte offset: the only sizes it needs)
//   k_txt_index   line_start [n + 1] (uint32; nbytes < 2^32)
//   k_txt_seg     first line of every segment (a lower bound of seg_off in line_start)
//   k_txt_parse   one lane per line: three fields through scantext.hpp, group[j] by a binary search of seg_off; a line
//                 with a class-3 field appends (j, start) to a list, a bad line lowers one 64-bit minimum
//   k_txt_patch   the values the host parsed for the listed lines (sorted first), scattered into rows
// include/vcp.h holds the contract; DESIGN.md section 30 the measurements.
#include <locale.h>

#include <algorithm>
#include <charconv>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "scantext.hpp"
#include "vcp_ctx.hpp"
#include "wave.hpp"

namespace {
constexpr int TT = 256;
constexpr int CHUNK = VCP_TXT_CHUNK;
constexpr int PER = CHUNK / TT;  // bytes per lane of the two indexing kernels: four 16-byte loads
static_assert(PER == 64, "one 64-bit terminator mask per lane");
constexpr uint32_t NOBAD = 0xFFFFFFFFu;

// The 64 bytes at i0 < nbytes (i0 a multiple of 64; the copy of the text is zero-padded to a multiple of 64 plus 64):
// bit b of the result is set when byte i0 + b ends a line -- a '\n', or a '\r' that no '\n' follows.  *bad is lowered to
// the offset of the first byte below nbytes that the contract does not support.
__device__ __forceinline__ uint64_t term_mask(const unsigned char* __restrict__ text, uint32_t nbytes, uint64_t i0,
                                              uint32_t* bad) {
  uint32_t w[PER / 4 + 1];
  const uint4* src = reinterpret_cast<const uint4*>(text + i0);
#pragma unroll
  for (int k = 0; k < PER / 16; k++) {
    const uint4 q = src[k];
    w[4 * k] = q.x;
    w[4 * k + 1] = q.y;
    w[4 * k + 2] = q.z;
    w[4 * k + 3] = q.w;
  }
  w[PER / 4] = text[i0 + PER];  // the byte past the lane's span (past the chunk for the last lane): zero beyond the text
  uint64_t m = 0;
  uint32_t first_bad = NOBAD;
#pragma unroll
  for (int b = PER - 1; b >= 0; b--) {
    const unsigned c = (w[b >> 2] >> (8 * (b & 3))) & 0xFFu, nx = (w[(b + 1) >> 2] >> (8 * ((b + 1) & 3))) & 0xFFu;
    if (c == '\n' || (c == '\r' && nx != '\n')) m |= (uint64_t)1 << b;
    if (!stx::supported_byte(c) && i0 + b < nbytes) first_bad = (uint32_t)(i0 + b);  // descending b: the first one stays
  }
  if (first_bad < *bad) *bad = first_bad;
  return m;
}

__global__ __launch_bounds__(TT) void k_txt_count(const unsigned char* __restrict__ text, uint32_t nbytes,
                                                 uint32_t* __restrict__ chunk_count, uint32_t* __restrict__ bad) {
  const uint64_t i0 = (uint64_t)blockIdx.x * CHUNK + (uint64_t)threadIdx.x * PER;
  uint32_t b = NOBAD;
  unsigned c = 0;
  if (i0 < nbytes) c = (unsigned)__popcll(term_mask(text, nbytes, i0, &b));
  c = wave_all<WaveAdd>(c);
  b = wave_all<WaveMin>(b);
  __shared__ unsigned wc[TT / 64], wb[TT / 64];
  if ((threadIdx.x & 63) == 0) {
    wc[threadIdx.x >> 6] = c;
    wb[threadIdx.x >> 6] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned s = 0;
    uint32_t mb = NOBAD;
    for (int k = 0; k < TT / 64; k++) {
      s += wc[k];
      mb = min(mb, wb[k]);
    }
    chunk_count[blockIdx.x] = s;
    if (mb != NOBAD) atomicMin(bad, mb);
  }
}

// chunk_base = the exclusive scan of chunk_count.  Lane order is byte order, so a lane's lines follow those of the lanes
// before it: line_start[k + 1] = the offset past the k-th terminator, line_start[0] = 0.
__global__ __launch_bounds__(TT) void k_txt_index(const unsigned char* __restrict__ text, uint32_t nbytes,
                                                 const uint32_t* __restrict__ chunk_base,
                                                 uint32_t* __restrict__ line_start) {
  const uint64_t i0 = (uint64_t)blockIdx.x * CHUNK + (uint64_t)threadIdx.x * PER;
  uint32_t b = NOBAD;
  uint64_t m = 0;
  if (i0 < nbytes) m = term_mask(text, nbytes, i0, &b);
  const unsigned c = (unsigned)__popcll(m);
  __shared__ uint32_t wt[TT / 64];
  uint32_t pos = block_excl(c, wt, chunk_base[blockIdx.x]) + 1u;
  while (m) {
    const int bit = __ffsll((long long)m) - 1;
    m &= m - 1;
    line_start[pos++] = (uint32_t)(i0 + bit + 1);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) line_start[0] = 0u;
}

// seg_first[k] = the first line that starts at or after seg_off[k], k = 0..nseg (line_start[n] = nbytes = seg_off[nseg])
__global__ __launch_bounds__(TT) void k_txt_seg(const uint32_t* __restrict__ line_start, int64_t n,
                                               const uint64_t* __restrict__ seg_off, int32_t nseg,
                                               int64_t* __restrict__ seg_first) {
  const int64_t k = (int64_t)blockIdx.x * TT + threadIdx.x;
  if (k > nseg) return;
  const uint64_t target = seg_off[k];
  int64_t lo = 0, hi = n;  // the answer is in [0, n]
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (line_start[mid] < target) lo = mid + 1;
    else hi = mid;
  }
  seg_first[k] = lo;
}

// counters[0]: entries of the host list; counters[1]: the minimum of (line << 2 | kind) over the bad lines.
// STAGE: the workgroup's lines are one contiguous span of the text; when the span (from the 16-byte boundary below it)
// fits STAGE_BYTES it is copied to LDS with 16-byte loads and the lanes walk their lines there; a longer span is read from
// global memory, as every span is without STAGE.
constexpr int STAGE_BYTES = 32768;
template <bool STAGE>
__global__ __launch_bounds__(TT) void k_txt_parse(const unsigned char* __restrict__ text,
                                                 const uint32_t* __restrict__ line_start, int64_t n,
                                                 const uint64_t* __restrict__ seg_off, int32_t nseg,
                                                 double* __restrict__ rows, int32_t* __restrict__ group,
                                                 unsigned long long* __restrict__ hostlist,
                                                 unsigned long long* __restrict__ counters) {
  __shared__ uint4 sbuf[STAGE ? STAGE_BYTES / 16 : 1];
  const int64_t j0 = (int64_t)blockIdx.x * TT, j = j0 + threadIdx.x;
  bool staged = false;
  uint32_t a0 = 0;
  if (STAGE) {
    const int64_t j1 = j0 + TT < n ? j0 + TT : n;
    a0 = line_start[j0] & ~15u;
    const uint64_t span = (uint64_t)line_start[j1] - a0;  // the same for every lane
    staged = span <= (uint64_t)STAGE_BYTES;
    if (staged) {
      const uint4* src = reinterpret_cast<const uint4*>(text + a0);  // the copy of the text is padded past the last line
      for (uint32_t q = threadIdx.x; q < (uint32_t)((span + 15) / 16); q += TT) sbuf[q] = src[q];
      __syncthreads();
    }
  }
  if (j >= n) return;
  const uint32_t s = line_start[j], e = line_start[j + 1];
  const unsigned char* p = staged ? reinterpret_cast<const unsigned char*>(sbuf) + (s - a0) : text + s;
  int64_t len = (int64_t)e - s;  // >= 1: every line ends with its terminator
  if (p[len - 1] == '\n') len--;
  if (len > 0 && p[len - 1] == '\r') len--;
  double v[3];
  int64_t f[6];
  const int st = stx::parse_line(p, len, v, f);
  if (st == stx::LINE_OK) {
    rows[3 * j] = v[0];
    rows[3 * j + 1] = v[1];
    rows[3 * j + 2] = v[2];
  } else if (st == stx::LINE_HOST) {
    const unsigned long long at = atomicAdd(&counters[0], 1ull);
    hostlist[at] = (unsigned long long)j << 32 | s;
  } else {
    atomicMin(&counters[1], (unsigned long long)j << 2 | (unsigned)st);
  }
  if (group) {  // the last segment that starts at or before s: of several that start there, the one that is not empty
    int32_t lo = 0, hi = nseg;
    while (hi - lo > 1) {
      const int32_t mid = lo + ((hi - lo) >> 1);
      if (seg_off[mid] <= s) lo = mid;
      else hi = mid;
    }
    group[j] = lo;
  }
}

__global__ __launch_bounds__(TT) void k_txt_patch(const double* __restrict__ vals, const uint32_t* __restrict__ idx,
                                                 int64_t m, double* __restrict__ rows) {
  const int64_t i = (int64_t)blockIdx.x * TT + threadIdx.x;
  if (i >= m) return;
  const size_t j = idx[i];
  rows[3 * j] = vals[3 * i];
  rows[3 * j + 1] = vals[3 * i + 1];
  rows[3 * j + 2] = vals[3 * i + 2];
}

// ---- the host's share: class-3 fields ---------------------------------------------------------------------------------
// A field the scanner accepted and neither device class settles: correctly rounded and independent of the locale.
// std::from_chars reads the digits; where it reports a result out of range it leaves the value alone (an overflow, or in
// some library versions any result below the normal range), and strtod_l in the "C" locale gives the rounded result.
double host_class3(const unsigned char* s, int64_t len) {
  stx::Scan r;
  if (!stx::scan_field(s, len, &r)) return 0.0;  // not reached: the caller saw class 3
  if (r.name == 1) return stx::from_bits(((uint64_t)r.neg << 63) | 0x7FF0000000000000ull);
  if (r.name == 2) return stx::from_bits(((uint64_t)r.neg << 63) | 0x7FF8000000000000ull);
  int64_t a = 0, b = len;
  while (s[a] == ' ') a++;
  while (s[b - 1] == ' ') b--;
  if (s[a] == '+' || s[a] == '-') a++;
  const char* first = reinterpret_cast<const char*>(s) + a;
  const char* last = reinterpret_cast<const char*>(s) + b;
  double x = 0.0;
  const std::from_chars_result fc = std::from_chars(first, last, x, std::chars_format::general);
  if (fc.ec != std::errc() || fc.ptr != last) {
    static const locale_t c_locale = newlocale(LC_ALL_MASK, "C", (locale_t)0);
    const std::string z(first, last);
    x = strtod_l(z.c_str(), nullptr, c_locale);
  }
  return r.neg ? -x : x;
}

// one listed line on the host: the three values, the class-3 ones through host_class3
void host_line(const unsigned char* text, uint64_t nbytes, uint64_t s, double v[3]) {
  uint64_t e = s;
  while (e < nbytes && text[e] != '\n' && text[e] != '\r') e++;
  int64_t f[6];
  double t[3];
  stx::parse_line(text + s, (int64_t)(e - s), t, f);
  for (int k = 0; k < 3; k++) {
    const unsigned char* p = text + s + f[2 * k];
    v[k] = stx::parse_field(p, f[2 * k + 1], &t[k]) == 3 ? host_class3(p, f[2 * k + 1]) : t[k];
  }
}

// both forms.  dev: rows / group are device pointers; otherwise host pointers filled from the context's workspace
int txt_impl(vcp_ctx* ctx, const char* text_c, uint64_t nbytes, const uint64_t* seg_off, int32_t nseg, int64_t cap,
             double* rows, int32_t* group, bool dev, int64_t* seg_first, int64_t* n_out, int64_t* n_host,
             int64_t* err) {
  if (!ctx) return VCP_ERR_ARG;
  if (!n_out || (nbytes > 0 && !text_c) || (seg_off && nseg < 1) || cap < 0)
    return vcp_fail(ctx, VCP_ERR_ARG, "bad argument");
  if (nbytes >= ((uint64_t)1 << 32)) return vcp_fail(ctx, VCP_ERR_TOO_LARGE, "text of %llu bytes: offsets are 32 bits",
                                                    (unsigned long long)nbytes);
  const unsigned char* text = reinterpret_cast<const unsigned char*>(text_c);
  const uint64_t one[2] = {0, nbytes};
  if (!seg_off) {
    seg_off = one;
    nseg = 1;
  }
  if (seg_off[0] != 0 || seg_off[nseg] != nbytes) return vcp_fail(ctx, VCP_ERR_ARG, "seg_off must run from 0 to nbytes");
  for (int32_t k = 0; k < nseg; k++) {
    if (seg_off[k] > seg_off[k + 1] || seg_off[k + 1] > nbytes)
      return vcp_fail(ctx, VCP_ERR_ARG, "seg_off must ascend (segment %d)", k);
    if (seg_off[k + 1] > seg_off[k] && text[seg_off[k + 1] - 1] != '\n')
      return vcp_fail(ctx, VCP_ERR_ARG, "segment %d does not end with a line feed", k);
  }
  int64_t err_local[3];
  if (!err) err = err_local;
  err[0] = err[1] = err[2] = 0;
  VCP_TRY(vcp_bind(ctx));
  vcp_phase_reset(ctx);
  if (nbytes == 0) {
    ctx->last_timing.clear();
    *n_out = 0;
    if (n_host) *n_host = 0;
    if (seg_first) std::fill(seg_first, seg_first + nseg + 1, (int64_t)0);
    return VCP_OK;
  }
  hipStream_t st = ctx->stream;
  const size_t padded = ((size_t)nbytes + 63) / 64 * 64 + 64;
  const unsigned nchunks = vcp_blocks((int64_t)nbytes, CHUNK);
  const size_t o_seg = 64, o_first = o_seg + (size_t)(nseg + 1) * 8;
  VCP_TRY(vcp_ensure(ctx, ctx->b_tx_text, padded));
  VCP_TRY(vcp_ensure(ctx, ctx->b_tx_chunk, (size_t)nchunks * 4));
  VCP_TRY(vcp_ensure(ctx, ctx->b_tx_misc, o_first + (size_t)(nseg + 1) * 8));
  unsigned char* d_text = ctx->b_tx_text.as<unsigned char>();
  uint32_t* d_chunk = ctx->b_tx_chunk.as<uint32_t>();
  char* misc = ctx->b_tx_misc.as<char>();
  // misc: [0, 8) host-list entries, [8, 16) the bad-line minimum, [16, 20) the bad-byte minimum, [20, 24) n
  unsigned long long* d_counters = reinterpret_cast<unsigned long long*>(misc);
  uint32_t* d_bad = reinterpret_cast<uint32_t*>(misc + 16);
  uint32_t* d_total = reinterpret_cast<uint32_t*>(misc + 20);
  uint64_t* d_seg = reinterpret_cast<uint64_t*>(misc + o_seg);
  int64_t* d_first = reinterpret_cast<int64_t*>(misc + o_first);

  vcp_phase(ctx, "txt_upload");
  VCP_HIP(ctx, hipMemcpyAsync(d_text, text, nbytes, hipMemcpyHostToDevice, st));
  VCP_HIP(ctx, hipMemsetAsync(d_text + nbytes, 0, padded - nbytes, st));
  VCP_HIP(ctx, hipMemcpyAsync(d_seg, seg_off, (size_t)(nseg + 1) * 8, hipMemcpyHostToDevice, st));
  VCP_HIP(ctx, hipMemsetAsync(misc, 0xFF, 24, st));
  VCP_HIP(ctx, hipMemsetAsync(misc, 0, 8, st));

  vcp_phase(ctx, "txt_index");
  VCP_LAUNCH(ctx, k_txt_count, dim3(nchunks), dim3(TT), 0, st, d_text, (uint32_t)nbytes, d_chunk, d_bad);
  VCP_TRY(vcp_exclusive_scan_u32(ctx, d_chunk, d_chunk, nchunks, d_total));
  uint32_t* hp = reinterpret_cast<uint32_t*>(ctx->pinned);  // [0, 24): a copy of the head of misc
  VCP_HIP(ctx, hipMemcpyAsync(hp, misc, 24, hipMemcpyDeviceToHost, st));
  VCP_HIP(ctx, hipStreamSynchronize(st));
  if (hp[4] != NOBAD) {
    err[0] = (int64_t)hp[4];
    return vcp_fail(ctx, VCP_ERR_UNSUPPORTED, "byte 0x%02X at offset %u: the device reader takes \\t \\n \\r and 0x20..0x7E "
                    "without '_'", (unsigned)text[hp[4]], hp[4]);
  }
  const int64_t n = (int64_t)hp[5];
  if (n >= 0x7FFFFFF0LL) return vcp_fail(ctx, VCP_ERR_TOO_LARGE, "%lld lines: beyond 32-bit indexing", (long long)n);
  const bool count_only = rows == nullptr;
  if (!count_only && n > cap) {
    *n_out = n;
    return vcp_fail(ctx, VCP_ERR_INDEX, "%lld lines for a capacity of %lld", (long long)n, (long long)cap);
  }
  if (count_only && !seg_first) {
    *n_out = n;
    if (n_host) *n_host = 0;
    return vcp_phase_finish(ctx);
  }
  const size_t o_list = ((size_t)(n + 1) * 4 + 7) / 8 * 8;
  VCP_TRY(vcp_ensure(ctx, ctx->b_tx_line, o_list + (count_only ? 0 : (size_t)n * 8)));
  uint32_t* d_line = ctx->b_tx_line.as<uint32_t>();
  unsigned long long* d_list = reinterpret_cast<unsigned long long*>(ctx->b_tx_line.as<char>() + o_list);
  VCP_LAUNCH(ctx, k_txt_index, dim3(nchunks), dim3(TT), 0, st, d_text, (uint32_t)nbytes, d_chunk, d_line);
  VCP_LAUNCH(ctx, k_txt_seg, dim3(vcp_blocks(nseg + 1, TT)), dim3(TT), 0, st, d_line, n, d_seg, nseg, d_first);
  std::vector<int64_t> first((size_t)nseg + 1);
  VCP_HIP(ctx, hipMemcpyAsync(first.data(), d_first, first.size() * 8, hipMemcpyDeviceToHost, st));

  double* d_rows = rows;
  int32_t* d_group = group;
  if (!count_only) {
    vcp_phase(ctx, "txt_parse");
    if (!dev) {
      const size_t o_group = (size_t)n * 24;
      VCP_TRY(vcp_ensure(ctx, ctx->b_tx_out, o_group + (size_t)n * 4));
      d_rows = ctx->b_tx_out.as<double>();
      d_group = group ? reinterpret_cast<int32_t*>(ctx->b_tx_out.as<char>() + o_group) : nullptr;
    }
    // developer switch for tools/bench_parse_text.py (read at every call): VCP_TXT_DIRECT=1 takes the kernel without the
    // LDS staging
    const char* sw = getenv("VCP_TXT_DIRECT");
    if (sw && sw[0] != '\0' && !(sw[0] == '0' && sw[1] == '\0'))
      VCP_LAUNCH(ctx, k_txt_parse<false>, dim3(vcp_blocks(n, TT)), dim3(TT), 0, st, d_text, d_line, n, d_seg, nseg, d_rows,
                 d_group, d_list, d_counters);
    else
      VCP_LAUNCH(ctx, k_txt_parse<true>, dim3(vcp_blocks(n, TT)), dim3(TT), 0, st, d_text, d_line, n, d_seg, nseg, d_rows,
                 d_group, d_list, d_counters);
    VCP_HIP(ctx, hipMemcpyAsync(hp, misc, 24, hipMemcpyDeviceToHost, st));
  }
  VCP_HIP(ctx, hipStreamSynchronize(st));
  if (seg_first) std::copy(first.begin(), first.end(), seg_first);
  if (count_only) {
    *n_out = n;
    if (n_host) *n_host = 0;
    return vcp_phase_finish(ctx);
  }
  const unsigned long long* hc = reinterpret_cast<const unsigned long long*>(hp);
  if (hc[1] != ~0ull) {  // the first bad line, in input order
    const int64_t line = (int64_t)(hc[1] >> 2);
    const int64_t k = (std::upper_bound(first.begin(), first.end(), line) - first.begin()) - 1;
    err[0] = line - first[(size_t)k] + 1;
    err[1] = k;
    err[2] = (int64_t)(hc[1] & 3u);
    return vcp_fail(ctx, VCP_ERR_ARG, "segment %lld line %lld: %s", (long long)k, (long long)err[0],
                    err[2] == stx::LINE_FEW ? "fewer than three fields" : "not a number");
  }
  const size_t m = (size_t)hc[0];
  vcp_phase(ctx, "txt_patch");
  if (m > 0) {
    std::vector<unsigned long long> list(m);
    VCP_HIP(ctx, hipMemcpyAsync(list.data(), d_list, m * 8, hipMemcpyDeviceToHost, st));
    VCP_HIP(ctx, hipStreamSynchronize(st));
    std::sort(list.begin(), list.end());
    // one upload: [vals m * 24 | idx m * 4]
    std::vector<double> up(m * 3 + (m + 1) / 2);
    uint32_t* idx = reinterpret_cast<uint32_t*>(up.data() + m * 3);
    for (size_t i = 0; i < m; i++) {
      idx[i] = (uint32_t)(list[i] >> 32);
      host_line(text, nbytes, (uint32_t)list[i], &up[3 * i]);
    }
    VCP_TRY(vcp_ensure(ctx, ctx->b_tx_patch, up.size() * 8));
    VCP_HIP(ctx, hipMemcpyAsync(ctx->b_tx_patch.p, up.data(), up.size() * 8, hipMemcpyHostToDevice, st));
    VCP_LAUNCH(ctx, k_txt_patch, dim3(vcp_blocks((int64_t)m, TT)), dim3(TT), 0, st, ctx->b_tx_patch.as<double>(),
               reinterpret_cast<const uint32_t*>(ctx->b_tx_patch.as<double>() + m * 3), (int64_t)m, d_rows);
    VCP_HIP(ctx, hipStreamSynchronize(st));  // `up` goes out of scope
  }
  if (!dev && n > 0) {
    VCP_HIP(ctx, hipMemcpyAsync(rows, d_rows, (size_t)n * 24, hipMemcpyDeviceToHost, st));
    if (group) VCP_HIP(ctx, hipMemcpyAsync(group, d_group, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  }
  VCP_TRY(vcp_phase_finish(ctx));
  VCP_HIP(ctx, hipStreamSynchronize(st));
  *n_out = n;
  if (n_host) *n_host = (int64_t)m;
  return VCP_OK;
}
}  // namespace

extern "C" int vcp_parse_scan_text(vcp_ctx* ctx, const char* text, uint64_t nbytes, const uint64_t* seg_off, int32_t nseg,
                                   int64_t cap, double* rows, int32_t* group, int64_t* seg_first, int64_t* n,
                                   int64_t* n_host, int64_t err[3]) {
  return txt_impl(ctx, text, nbytes, seg_off, nseg, cap, rows, group, false, seg_first, n, n_host, err);
}

extern "C" int vcp_parse_scan_text_dev(vcp_ctx* ctx, const char* text, uint64_t nbytes, const uint64_t* seg_off,
                                       int32_t nseg, int64_t cap, double* d_rows, int32_t* d_group, int64_t* seg_first,
                                       int64_t* n, int64_t* n_host, int64_t err[3]) {
  return txt_impl(ctx, text, nbytes, seg_off, nseg, cap, d_rows, d_group, true, seg_first, n, n_host, err);
}

extern "C" int vcp_selftest_parse_field(const char* s, int64_t len, double* v) {
  if (!v || len < 0 || (len > 0 && !s)) return VCP_ERR_ARG;
  const unsigned char* u = reinterpret_cast<const unsigned char*>(s);
  const int c = stx::parse_field(u, len, v);
  if (c == 3) *v = host_class3(u, len);
  return c;
}
