// scanfmt.hpp -- one number and one line of an export file (`[id<TAB>]a<TAB>b<TAB>c<EOL>`, BC/Tools.cs:233, 295, 341, 374),
// __host__ __device__: the kernels of scanfmt.hip and vcp_selftest_format_field compile this source.  For a binary64 v and
// 0 <= bit <= 15 the bytes are those of Python's '%.*f' % (bit, v): the exact binary value rounded to `bit` decimals, ties
// to even.  include/vcp.h (vcp_format_rows) states the contract; the arithmetic, all in integers:
//   |v| = mant * 2^ex, mant < 2^53.  I = floor(|v|) and f = |v| - I = mf * 2^-k (mf < 2^k, mf < 2^53) are exact
//   mf * 10^bit < 2^53 * 10^15 < 2^103 is an exact 128-bit product P; q = P >> k, rem = P mod 2^k
//   k >= 104: P < 2^(k-1), so q = 0 and the remainder is below one half: the fraction rounds to 0
//   round up when rem > 2^(k-1), or rem == 2^(k-1) and the WHOLE number I * 10^bit + q is odd: q's parity for bit >= 1
//   (10^bit is even), I's for bit == 0 (q is 0 there)
//   F = q + up; F == 10^bit carries into I.  I <= 10^15 and F < 10^15; their digits come from one 64-bit division by
//   10^8 each and 32-bit divisions by 10
// Supported: v finite and |v| < 1e15.  Nothing here rounds in floating point, reads a locale or depends on -ffp-contract.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SFX_HD __host__ __device__ __forceinline__
#else
#define SFX_HD inline
#endif

namespace sfx {

constexpr int BIT_MAX = 15;
// The longest field.  An integer part of 16 digits can only be 10^15, reached by a carry out of 999 999 999 999 999.f with
// f >= 1 - 10^-bit / 2.  That integer part is above 2^49, where binary64 fractions are multiples of 1/8: f <= 0.875.  With
// a decimal point (bit >= 1) the carry needs f >= 0.95 and does not happen: at most 15 digits, and '-' + 15 + '.' + 15 =
// 32 bytes at bit 15.  Without one (bit 0) 999999999999999.875 = nextafter(1e15, 0) does round to 10^15: 17 bytes.  (The
// count that ignores this, '-' + 16 + '.' + 15 = 33 per field and 115 per line, is a bound too, and is never reached.)
constexpr int FIELD_BYTES_MAX = 1 + 15 + 1 + BIT_MAX;
constexpr int ID_BYTES_MAX = 11;  // -2147483648
// id TAB a TAB b TAB c CR LF
constexpr int LINE_BYTES_MAX = ID_BYTES_MAX + 1 + 3 * FIELD_BYTES_MAX + 2 + 2;
static_assert(FIELD_BYTES_MAX == 32 && LINE_BYTES_MAX == 112, "include/vcp.h: VCP_FMT_LINE_MAX");

// one number, rounded: sign, integer part, the fraction's `bit` digits as an integer
struct Field {
  uint64_t I, F;
  uint32_t neg;
};

SFX_HD uint64_t bits_of(double v) {
  union {
    double d;
    uint64_t u;
  } x;
  x.d = v;
  return x.u;
}

SFX_HD uint64_t pow10(int k) {  // k in 0..15 (a function, not a table object: see scantext.hpp)
  constexpr uint64_t T[16] = {1ull,
                              10ull,
                              100ull,
                              1000ull,
                              10000ull,
                              100000ull,
                              1000000ull,
                              10000000ull,
                              100000000ull,
                              1000000000ull,
                              10000000000ull,
                              100000000000ull,
                              1000000000000ull,
                              10000000000000ull,
                              100000000000000ull,
                              1000000000000000ull};
  return T[k];
}

// false: v is not supported (NaN, an infinity, |v| >= 1e15); *out is then untouched
SFX_HD bool split(double v, int bit, Field* out) {
  const uint64_t u = bits_of(v), a = u & 0x7FFFFFFFFFFFFFFFull;
  if (a >= 0x430C6BF526340000ull) return false;  // the bits of 1e15: larger magnitudes, the infinities and every NaN
  const int e = (int)(a >> 52);
  const uint64_t mant = e ? (a & 0xFFFFFFFFFFFFFull) | (1ull << 52) : a;
  const int ex = e ? e - 1075 : -1074;  // |v| = mant * 2^ex; ex <= -3 here, as |v| < 2^50
  const int k = -ex;                    // 3..1074
  uint64_t I = 0, mf = mant;
  if (k < 64) {
    I = mant >> k;
    mf = mant & ((1ull << k) - 1);
  }
  uint64_t F = 0;
  if (k < 104 && mf != 0) {
    const uint64_t p10 = pow10(bit);
    const unsigned __int128 P = (unsigned __int128)mf * p10;
    const unsigned __int128 rem = P & (((unsigned __int128)1 << k) - 1), half = (unsigned __int128)1 << (k - 1);
    const uint64_t q = (uint64_t)(P >> k);  // < 10^bit
    const uint64_t odd = (bit ? q : I) & 1u;
    F = q + ((rem > half || (rem == half && odd)) ? 1u : 0u);
    if (F == p10) {
      F = 0;
      I++;
    }
  }
  out->I = I;
  out->F = F;
  out->neg = (uint32_t)(u >> 63);
  return true;
}

SFX_HD int digits_u32(uint32_t x) {  // 1..10
  int d = 1;
  if (x >= 10u) d = 2;
  if (x >= 100u) d = 3;
  if (x >= 1000u) d = 4;
  if (x >= 10000u) d = 5;
  if (x >= 100000u) d = 6;
  if (x >= 1000000u) d = 7;
  if (x >= 10000000u) d = 8;
  if (x >= 100000000u) d = 9;
  if (x >= 1000000000u) d = 10;
  return d;
}

SFX_HD int digits_u64(uint64_t x) {  // x <= 10^15: 1..16
  if (x < 100000000ull) return digits_u32((uint32_t)x);
  return 8 + digits_u32((uint32_t)(x / 100000000ull));
}

SFX_HD int field_len(const Field& f, int bit) { return (int)f.neg + digits_u64(f.I) + (bit ? 1 + bit : 0); }

// exactly nd digits of x (x < 10^nd), zero-padded on the left
template <class P>
SFX_HD void put_u32(P p, uint32_t x, int nd) {
  for (int i = nd - 1; i >= 0; i--) {
    p[i] = (char)('0' + x % 10u);
    x /= 10u;
  }
}

// x <= 10^16 - 1 as nd digits (nd >= its number of digits)
template <class P>
SFX_HD void put_u64(P p, uint64_t x, int nd) {
  if (nd > 8) {
    put_u32(p, (uint32_t)(x / 100000000ull), nd - 8);
    put_u32(p + (nd - 8), (uint32_t)(x % 100000000ull), 8);
  } else {
    put_u32(p, (uint32_t)x, nd);
  }
}

// the bytes of one field at p; returns their number (= field_len)
template <class P>
SFX_HD int put_field(P p, const Field& f, int bit) {
  int o = 0;
  if (f.neg) p[o++] = '-';
  const int nd = digits_u64(f.I);
  put_u64(p + o, f.I, nd);
  o += nd;
  if (bit) {
    p[o++] = '.';
    put_u64(p + o, f.F, bit);
    o += bit;
  }
  return o;
}

// an int32 as Python's '%d'
SFX_HD int id_len(int32_t x) {
  const uint32_t mag = x < 0 ? 0u - (uint32_t)x : (uint32_t)x;
  return (x < 0) + digits_u32(mag);
}
template <class P>
SFX_HD int put_id(P p, int32_t x) {
  const uint32_t mag = x < 0 ? 0u - (uint32_t)x : (uint32_t)x;
  int o = 0;
  if (x < 0) p[o++] = '-';
  const int nd = digits_u32(mag);
  put_u32(p + o, mag, nd);
  return o + nd;
}

// One line `[id TAB] a TAB b TAB c EOL` (eol 0: "\n", 1: "\r\n").
SFX_HD int line_len(bool has_id, int32_t id, const Field f[3], int bit, int eol) {
  return (has_id ? id_len(id) + 1 : 0) + field_len(f[0], bit) + field_len(f[1], bit) + field_len(f[2], bit) + 3 + eol;
}
template <class P>
SFX_HD int put_line(P p, bool has_id, int32_t id, const Field f[3], int bit, int eol) {
  int o = 0;
  if (has_id) {
    o += put_id(p, id);
    p[o++] = '\t';
  }
  o += put_field(p + o, f[0], bit);
  p[o++] = '\t';
  o += put_field(p + o, f[1], bit);
  p[o++] = '\t';
  o += put_field(p + o, f[2], bit);
  if (eol) p[o++] = '\r';
  p[o++] = '\n';
  return o;
}

}  // namespace sfx
