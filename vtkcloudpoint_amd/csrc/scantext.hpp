// scantext.hpp -- one field and one line of a scan file (`motor_x<TAB>motor_y<TAB>Distance`), __host__ __device__: the
// kernels of scantext.hip, the host's patch of the lines the device hands back, and vcp_selftest_parse_field all compile
// this source.  include/vcp.h (vcp_parse_scan_text) states the grammar and the class rule; in short
//   class 1   w == 0, or w <= 2^53 and |e10| <= 22: (double)w times or over an exact power of ten, ONE rounding
//   class 2   else nd <= 19 and |e10| <= 19: w * 10^e10 in integers (an exact 128-bit product, or a 128-by-64-bit long
//             division with a sticky bit), rounded to nearest-even by hand
//   class 3   any other number (more digits, larger exponents, inf / infinity / nan): left to the host
//   class 0   not a number
// with w the mantissa's digits as an integer (leading zeros stripped), nd their count and e10 the exponent minus the
// number of fraction digits.  Nothing here reads a locale, and nothing depends on -ffp-contract.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define STX_HD __host__ __device__ __forceinline__
#else
#define STX_HD inline
#endif

namespace stx {

// what the scanner found in one field (classes 1..3; the sign is applied by the caller of the evaluations)
struct Scan {
  uint64_t w;   // the first 19 significant digits (all of them when nd <= 19)
  int64_t e10;  // exponent minus fraction digits, counted for all nd digits
  int32_t nd;   // significant digits, saturating at 1 << 30
  bool neg;
  int name;  // 0: a decimal number; 1: inf / infinity; 2: nan
};

STX_HD bool is_digit(unsigned c) { return c - (unsigned)'0' < 10u; }

// the bytes vcp_parse_scan_text accepts: \t \n \r and 0x20..0x7E without '_'
STX_HD bool supported_byte(unsigned c) {
  return c == 9u || c == 10u || c == 13u || (c >= 0x20u && c <= 0x7Eu && c != (unsigned)'_');
}

// 1e0 .. 1e22 are exact in binary64; 10^0 .. 10^19 fit 64 bits.  Functions, not tables, so that the device build needs no
// constant-memory object shared between translation units; the switch compiles to a table either way.
STX_HD double pow10_f64(int k) {
  constexpr double T[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                            1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
  return T[k];
}
STX_HD uint64_t pow10_u64(int k) {
  constexpr uint64_t T[20] = {1ull,
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
                              1000000000000000ull,
                              10000000000000000ull,
                              100000000000000000ull,
                              1000000000000000000ull,
                              10000000000000000000ull};
  return T[k];
}

STX_HD double from_bits(uint64_t u) {
  union {
    uint64_t u;
    double d;
  } x;
  x.u = u;
  return x.d;
}

STX_HD int clz64(uint64_t x) {  // x != 0
#if defined(__HIP_DEVICE_COMPILE__)
  return __clzll((long long)x);
#else
  return __builtin_clzll(x);
#endif
}

// Scans s[0, len): sp* [+-]? (D+ ('.' D*)? | '.' D+) ([eE] [+-]? D+)? sp*, or sp* [+-]? (inf | infinity | nan) sp* in any
// letter case.  Returns false when the field is neither.
STX_HD bool scan_field(const unsigned char* s, int64_t len, Scan* out) {
  int64_t i = 0, end = len;
  while (i < end && s[i] == ' ') i++;
  while (end > i && s[end - 1] == ' ') end--;
  Scan r{0, 0, 0, false, 0};
  if (i < end && (s[i] == '+' || s[i] == '-')) {
    r.neg = s[i] == '-';
    i++;
  }
  if (i >= end) return false;
  if (!is_digit(s[i]) && s[i] != '.') {
    // the names, case-insensitive: compare (c | 0x20) with the lower-case letters
    const char nm[3][9] = {"inf", "infinity", "nan"};
    const int nl[3] = {3, 8, 3}, kind[3] = {1, 1, 2};
    for (int k = 0; k < 3; k++) {
      if (end - i != nl[k]) continue;
      bool ok = true;
      for (int j = 0; j < nl[k]; j++) ok = ok && (unsigned char)(s[i + j] | 0x20) == (unsigned char)nm[k][j];
      if (ok) {
        r.name = kind[k];
        *out = r;
        return true;
      }
    }
    return false;
  }
  int64_t nfrac = 0;
  bool any = false;
  for (; i < end && is_digit(s[i]); i++) {  // integer part
    any = true;
    const unsigned d = s[i] - (unsigned)'0';
    if (r.nd == 0 && d == 0) continue;  // a leading zero
    if (r.nd < 19) r.w = r.w * 10u + d;
    else r.e10++;  // a digit beyond the 19 kept: it scales what is kept (class 3; the host reads the text itself)
    if (r.nd < (1 << 30)) r.nd++;
  }
  if (i < end && s[i] == '.') {
    i++;
    for (; i < end && is_digit(s[i]); i++) {
      any = true;
      nfrac++;
      const unsigned d = s[i] - (unsigned)'0';
      if (r.nd == 0 && d == 0) continue;
      if (r.nd < 19) r.w = r.w * 10u + d;
      else r.e10++;
      if (r.nd < (1 << 30)) r.nd++;
    }
  }
  if (!any) return false;
  int64_t ex = 0;
  if (i < end && (s[i] == 'e' || s[i] == 'E')) {
    i++;
    bool eneg = false;
    if (i < end && (s[i] == '+' || s[i] == '-')) {
      eneg = s[i] == '-';
      i++;
    }
    if (i >= end || !is_digit(s[i])) return false;
    for (; i < end && is_digit(s[i]); i++)
      if (ex < (int64_t)1 << 40) ex = ex * 10 + (int64_t)(s[i] - (unsigned)'0');  // saturates far beyond any class
    if (eneg) ex = -ex;
  }
  if (i != end) return false;
  r.e10 += ex - nfrac;  // for nd <= 19 this is the contract's e10; beyond, e10 of the 19 digits kept
  *out = r;
  return true;
}

// the class of a scanned field (1, 2 or 3)
STX_HD int classify(const Scan& r) {
  if (r.name) return 3;
  if (r.w == 0 && r.nd == 0) return 1;
  if (r.nd > 19) return 3;
  if (r.w <= ((uint64_t)1 << 53) && r.e10 >= -22 && r.e10 <= 22) return 1;
  if (r.e10 >= -19 && r.e10 <= 19) return 2;
  return 3;
}

// class 1: Clinger's fast path.  w and the power are exact, so the one multiplication or division is the one rounding.
STX_HD double eval_class1(uint64_t w, int e10) {
  if (w == 0) return 0.0;
  const double x = (double)w;
  return e10 >= 0 ? x * pow10_f64(e10) : x / pow10_f64(-e10);
}

// RNE of (m + a fraction in (0, 1) when sticky) * 2^e2 for m != 0, where the result is a normal binary64
STX_HD double round_u128(unsigned __int128 m, bool sticky, int e2) {
  const uint64_t hi = (uint64_t)(m >> 64), lo = (uint64_t)m;
  const int p = hi ? 127 - clz64(hi) : 63 - clz64(lo);  // the top bit
  uint64_t mant;
  int ex = p;
  if (p <= 52) {
    mant = lo << (52 - p);  // exact (sticky cannot be set here: the callers give at least 64 bits when it is)
  } else {
    const int sh = p - 52;
    mant = (uint64_t)(m >> sh);
    const unsigned __int128 rem = m & (((unsigned __int128)1 << sh) - 1), half = (unsigned __int128)1 << (sh - 1);
    if (rem > half || (rem == half && (sticky || (mant & 1u)))) mant++;
    if (mant >> 53) {
      mant >>= 1;
      ex++;
    }
  }
  return from_bits(((uint64_t)(ex + e2 + 1023) << 52) | (mant & (((uint64_t)1 << 52) - 1)));
}

// class 2: 1 <= w < 10^19, |e10| <= 19
STX_HD double eval_class2(uint64_t w, int e10) {
  if (e10 >= 0) return round_u128((unsigned __int128)w * pow10_u64(e10), false, 0);  // < 10^38 < 2^127: exact
  // w / d: the dividend is w, shifted so that its top bit is bit 63, times 2^64; the quotient then has 64 bits or more.
  // The high half divides in 64 bits; the low half is a restoring division, one quotient bit per step (128-bit division
  // has no device runtime support).
  const uint64_t d = pow10_u64(-e10);
  const int lz = clz64(w);
  const uint64_t wn = w << lz;
  const uint64_t qh = wn / d;
  uint64_t r = wn % d, ql = 0;
  for (int k = 0; k < 64; k++) {
    const bool carry = r >> 63;
    r <<= 1;
    ql <<= 1;
    if (carry || r >= d) {  // with the carry the true remainder is r + 2^64 >= d, and r - d wraps to the right value
      r -= d;
      ql |= 1u;
    }
  }
  return round_u128(((unsigned __int128)qh << 64) | ql, r != 0, -64 - lz);
}

// One field: the class, and for classes 1 and 2 the value with its sign.  For class 3 *v is not written.
STX_HD int parse_field(const unsigned char* s, int64_t len, double* v) {
  Scan r;
  if (!scan_field(s, len, &r)) return 0;
  const int c = classify(r);
  if (c == 3) return 3;
  const double x = c == 1 ? eval_class1(r.w, (int)r.e10) : eval_class2(r.w, (int)r.e10);
  *v = r.neg ? -x : x;
  return c;
}

// One line without its terminator.  Returns 0 (v[0..2] written), 1 (fewer than three fields), 2 (one of the first three
// fields is not a number) or 3 (three numbers, at least one of class 3: the values of the others are in v).  `f` receives
// the offset and the length of the three fields when the count is right.
constexpr int LINE_OK = 0, LINE_FEW = 1, LINE_NAN = 2, LINE_HOST = 3;
STX_HD int parse_line(const unsigned char* s, int64_t len, double v[3], int64_t f[6]) {
  int64_t a = 0;
  int k = 0;
  for (int64_t i = 0; i <= len && k < 3; i++) {
    if (i == len || s[i] == '\t') {
      f[2 * k] = a;
      f[2 * k + 1] = i - a;
      k++;
      a = i + 1;
    }
  }
  if (k < 3) return LINE_FEW;
  int st = LINE_OK;
  for (k = 0; k < 3; k++) {
    const int c = parse_field(s + f[2 * k], f[2 * k + 1], &v[k]);
    if (c == 0) return LINE_NAN;
    if (c == 3) st = LINE_HOST;
  }
  return st;
}

}  // namespace stx
