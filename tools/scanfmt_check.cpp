// scanfmt_check.cpp -- csrc/scanfmt.hpp stand-alone, against the C library's "%.*f" (glibc's is correctly rounded) on N
// seeded (v, bit) pairs; meant to be built with sanitizers on:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan
//       -Ivtkcloudpoint_amd/csrc tools/scanfmt_check.cpp -o scanfmt_check && ./scanfmt_check 5000000
// Every field is written into a heap buffer of exactly field_len bytes, so that a byte too many is a report.  Prints one
// summary line; exit status 1 on the first difference.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "scanfmt.hpp"

static uint64_t state = 0x9E3779B97F4A7C15ull;
static uint64_t next() {  // xorshift64*
  state ^= state >> 12;
  state ^= state << 25;
  state ^= state >> 27;
  return state * 0x2545F4914F6CDD1Dull;
}

int main(int argc, char** argv) {
  const long n = argc > 1 ? atol(argv[1]) : 1000000;
  long supported = 0, unsupported = 0, ties = 0;
  int longest = 0;
  for (long t = 0; t < n; t++) {
    const int bit = (int)(next() % 16);
    double v;
    switch (t % 5) {
      case 0:  // uniform in +-1000
        v = ((double)(next() >> 11) / 9007199254740992.0 - 0.5) * 2000.0;
        break;
      case 1:  // any bit pattern: every exponent, NaNs and infinities among them
      {
        const uint64_t u = next();
        memcpy(&v, &u, 8);
        break;
      }
      case 2:  // 53 random bits with a binary exponent in -1100..50
        v = std::ldexp((double)(next() >> 11), (int)(next() % 1151) - 1100);
        if (next() & 1) v = -v;
        break;
      case 3:  // an exact tie at this bit
        v = (double)(2 * (next() % (1u << 24)) + 1) / std::ldexp(1.0, bit + 1);
        if (next() & 1) v = -v;
        ties++;
        break;
      default: {  // six decimals read back
        char s[64];
        snprintf(s, sizeof s, "%.6f", ((double)(next() >> 11) / 9007199254740992.0 - 0.5) * 2.0e6);
        v = strtod(s, nullptr);
      }
    }
    sfx::Field f;
    const bool ok = sfx::split(v, bit, &f);
    const bool want_ok = std::isfinite(v) && std::fabs(v) < 1e15;
    if (ok != want_ok) {
      printf("FAIL support of %a at bit %d: %d\n", v, bit, (int)ok);
      return 1;
    }
    if (!ok) {
      unsupported++;
      continue;
    }
    supported++;
    const int len = sfx::field_len(f, bit);
    std::unique_ptr<char[]> got(new char[len]);
    const int put = sfx::put_field(got.get(), f, bit);
    char want[400];
    const int wl = snprintf(want, sizeof want, "%.*f", bit, v);
    if (put != len || wl != len || memcmp(want, got.get(), (size_t)len) != 0 || len > sfx::FIELD_BYTES_MAX) {
      printf("FAIL %a at bit %d: wanted %s, got %.*s (len %d, put %d)\n", v, bit, want, put, got.get(), len, put);
      return 1;
    }
    if (len > longest) longest = len;
  }
  // the ids
  const int32_t ids[] = {0, 1, -1, 9, 10, 99, 100, 2147483647, -2147483647 - 1, 1000000000, -999999999};
  for (int32_t x : ids) {
    const int len = sfx::id_len(x);
    std::unique_ptr<char[]> got(new char[len]);
    char want[32];
    const int wl = snprintf(want, sizeof want, "%d", x);
    if (sfx::put_id(got.get(), x) != len || wl != len || memcmp(want, got.get(), (size_t)len) != 0 ||
        len > sfx::ID_BYTES_MAX) {
      printf("FAIL id %d\n", x);
      return 1;
    }
  }
  printf("ok: %ld pairs, %ld supported (%ld exact ties), %ld unsupported, longest field %d bytes\n", n, supported, ties,
         unsupported, longest);
  return 0;
}
