// wave_selftest.hip -- vcp_selftest_wave_dev: every shape of wave.hpp run by ONE workgroup on words and flags of the
// caller's, one row of the output per helper (include/vcp.h holds the layout; tests/test_wave_gpu.py the references).
#include "vcp_ctx.hpp"
#include "wave.hpp"

namespace {
constexpr uint32_t NOSLOT = 0xFFFFFFFFu;

// thread t: word v = words[t], predicate p = flags[t] != 0 (0 and false from t = n on); out [VCP_WAVE_ROWS][TB]
template <int TB>
__global__ __launch_bounds__(TB) void k_wave_selftest(const uint32_t* __restrict__ words, const uint8_t* __restrict__ flags,
                                                      uint32_t n, uint32_t* __restrict__ counter,
                                                      uint32_t* __restrict__ out) {
  __shared__ uint32_t w_excl[TB / 64], w_exclt[TB / 64], w_cnt[TB / 64], w_cnt2[2 * TB / 64], w_rank[TB / 64],
      w_rankt[TB / 64];
  const uint32_t t = threadIdx.x;
  const int lane = t & 63;
  const uint32_t v = t < n ? words[t] : 0u;
  const bool p = t < n && flags[t] != 0;
  uint32_t total = 0, cnt = NOSLOT, ca = NOSLOT, cb = NOSLOT, nrank = 0;
  out[0 * TB + t] = block_excl(v, w_excl, 7u) - 7u;
  out[1 * TB + t] = block_excl<TB>(v, w_exclt, total);
  out[2 * TB + t] = total;
  out[3 * TB + t] = wave_all<WaveAdd>(v);
  out[4 * TB + t] = wave_all<WaveMin>(v);
  out[5 * TB + t] = wave_all<WaveMax>(v);
  out[6 * TB + t] = (uint32_t)(wave_all<WaveOr>((unsigned long long)v << 16) >> 16);
  out[7 * TB + t] = wave_count(p);
  if (!block_count<TB>(p, w_cnt, cnt)) cnt = NOSLOT;  // thread 0 alone gets the count
  out[8 * TB + t] = cnt;
  if (!block_count<TB>(p, v & 1u, w_cnt2, ca, cb)) ca = cb = NOSLOT;
  out[9 * TB + t] = ca;
  out[10 * TB + t] = cb;
  out[11 * TB + t] = block_rank(p, w_rank);
  out[12 * TB + t] = block_rank<TB>(p, w_rankt, nrank);
  out[13 * TB + t] = nrank;
  const uint32_t slot = wave_append(p, counter);
  out[14 * TB + t] = p ? slot : NOSLOT;
  out[15 * TB + t] = wave_incl<WaveMax>(v, lane);
  out[16 * TB + t] = wave_incl<WaveAdd, 32>(v, lane & 31);
  out[17 * TB + t] = wave_prev(v);
  // the signed 64-bit forms: s = v - 2^31 stretched over 64 bits, so that sums leave 32 bits and maxima differ in sign
  const long long s = ((long long)v - (1ll << 31)) * (1ll << 20);
  const long long sa = wave_all<WaveAdd>(s), sm = wave_all<WaveMax>(s), sn = wave_all<WaveMin>(s);
  out[18 * TB + t] = (uint32_t)sa;
  out[19 * TB + t] = (uint32_t)((unsigned long long)sa >> 32);
  out[20 * TB + t] = (uint32_t)sm;
  out[21 * TB + t] = (uint32_t)((unsigned long long)sm >> 32);
  out[22 * TB + t] = (uint32_t)sn;
  out[23 * TB + t] = (uint32_t)((unsigned long long)sn >> 32);
}
}  // namespace

extern "C" int vcp_selftest_wave_dev(vcp_ctx* ctx, const uint32_t* d_words, const uint8_t* d_flags, int64_t n, int tb,
                                     uint32_t* d_counter, uint32_t* d_out) {
  if (!ctx) return VCP_ERR_ARG;
  if ((tb != 64 && tb != 256 && tb != 512 && tb != 1024) || n < 0 || n > tb || !d_counter || !d_out ||
      (n > 0 && (!d_words || !d_flags)))
    return vcp_fail(ctx, VCP_ERR_ARG, "bad argument");
  VCP_TRY(vcp_bind(ctx));
  hipStream_t st = ctx->stream;
  const uint32_t m = (uint32_t)n;
  switch (tb) {
    case 64: VCP_LAUNCH(ctx, k_wave_selftest<64>, dim3(1), dim3(64), 0, st, d_words, d_flags, m, d_counter, d_out); break;
    case 256: VCP_LAUNCH(ctx, k_wave_selftest<256>, dim3(1), dim3(256), 0, st, d_words, d_flags, m, d_counter, d_out); break;
    case 512: VCP_LAUNCH(ctx, k_wave_selftest<512>, dim3(1), dim3(512), 0, st, d_words, d_flags, m, d_counter, d_out); break;
    default: VCP_LAUNCH(ctx, k_wave_selftest<1024>, dim3(1), dim3(1024), 0, st, d_words, d_flags, m, d_counter, d_out); break;
  }
  VCP_HIP(ctx, hipStreamSynchronize(st));
  return VCP_OK;
}
