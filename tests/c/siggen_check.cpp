// tests/c/siggen_check.cpp -- TEST INFRASTRUCTURE: a stand-alone caller of ka9q-radio_amd/csrc/chz_siggen.h (the host arithmetic of the
// device-side sig_gen front end).  tests/test_siggen_host_sanitized.py builds it with -fsanitize=address,undefined and runs `selftest`;
// tests/test_siggen_host.py builds it plain and reads `phase` (the header's carrier phase, for its comparison in rational arithmetic).
//   siggen_check selftest            jump-ahead against sequential stepping, additivity, the kernel's row tables, the phase bound
//   siggen_check phase A N [A N ..]  prints siggen_phase(A, N) as a hex float, one per line (A a hex float, N decimal)
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include "chz_siggen.h"

using namespace chz;

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { failures++; fprintf(stderr, "FAILED %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

static bool same(const uint64_t a[4], const uint64_t b[4]) { return a[0] == b[0] && a[1] == b[1] && a[2] == b[2] && a[3] == b[3]; }

// frac(a n) exactly in integers, handed back as a long double (64-bit mantissa: good to 2^-64)
static long double exact_phase(double a, uint64_t n) {
  if (a == 0.0 || n == 0) return 0.0L;
  int e;
  const double m = frexp(fabs(a), &e);                       // |a| = m 2^e, m in [0.5, 1)
  const unsigned __int128 M = (unsigned __int128)(uint64_t)ldexp(m, 53);   // |a| = M 2^(e - 53)
  const int sh = 53 - e;                                     // |a| n = M n / 2^sh
  unsigned __int128 P = M * n;                               // < 2^106
  long double f;
  if (sh <= 0) return 0.0L;                                  // an integer
  if (sh < 128) { P &= (((unsigned __int128)1) << sh) - 1; }
  f = ldexpl((long double)P, -sh);
  if (a < 0 && f != 0.0L) f = 1.0L - f;
  return f;
}

static int selftest() {
  const uint64_t seeds[4] = {1, 0, 0x123456789abcdefULL, ~0ull};
  // against sequential stepping
  const uint64_t counts[] = {0, 1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 1000007};
  for (uint64_t sd : seeds) {
    uint64_t s0[4], seq[4];
    siggen_seed(sd, s0);
    memcpy(seq, s0, sizeof seq);
    uint64_t done = 0;
    for (uint64_t d : counts) {
      for (; done < d; done++) (void)siggen_next(seq);
      uint64_t j[4];
      memcpy(j, s0, sizeof j);
      siggen_jump(j, d, 0);
      EXPECT(same(j, seq), "jump(%" PRIu64 ") from seed %" PRIu64, d, sd);
    }
  }
  // additivity, with carries into the high word
  uint64_t r[4];
  siggen_seed(99, r);
  for (int i = 0; i < 16; i++) {
    const uint64_t a = siggen_next(r) | (1ull << 63), b = siggen_next(r) | (1ull << 63), ah = siggen_next(r) >> 2, bh = siggen_next(r) >> 2;
    uint64_t x[4], y[4];
    siggen_seed((uint64_t)i, x);
    memcpy(y, x, sizeof y);
    siggen_jump(x, a, ah); siggen_jump(x, b, bh);
    const uint64_t lo = a + b, hi = ah + bh + (lo < a ? 1 : 0);
    siggen_jump(y, lo, hi);
    EXPECT(same(x, y), "jump(a) jump(b) != jump(a + b), case %d", i);
  }
  // the row tables hold the same matrix as the columns
  {
    std::vector<uint64_t> rows(1024);
    siggen_rows(6, rows.data());
    uint64_t v[4], want[4], got[4] = {0, 0, 0, 0};
    siggen_seed(7, v);
    memcpy(want, v, sizeof want);
    siggen_jump(want, 64, 0);
    for (int c = 0; c < 4; c++)
      for (int t = 0; t < 64; t++) {
        const uint64_t* row = &rows[(size_t)(c * 64 + t) * 4];
        const uint64_t p = (row[0] & v[0]) ^ (row[1] & v[1]) ^ (row[2] & v[2]) ^ (row[3] & v[3]);
        got[c] |= (uint64_t)(__builtin_popcountll(p) & 1) << t;
      }
    EXPECT(same(got, want), "rows of T^64 against its columns");
  }
  // the phase: within 2^-52 of frac(a n), as angles
  const double as[] = {10.00002e6 / 129.6e6, 10e6 / 129.6e6, 0.123456789, 1e-4, 0.4999, -0.2371, 0.25, 0.0, -0.5, 0x1p-60};
  const uint64_t ns[] = {0, 1, (1ull << 20) + 3, (1ull << 40) + 12345, (1ull << 53) - 1};
  for (double a : as)
    for (uint64_t n : ns) {
      const double phi = siggen_phase(a, n);
      long double d = fabsl((long double)phi - exact_phase(a, n));
      if (d > 0.5L) d = 1.0L - d;
      EXPECT(phi >= 0.0 && phi <= 1.0 && d <= 0x1p-52L, "phase(%a, %" PRIu64 ") = %a, off by %Lg", a, n, phi, d);
    }
  if (failures) return 1;
  printf("siggen_check: ok\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 2 && !strcmp(argv[1], "selftest")) return selftest();
  if (argc >= 4 && !strcmp(argv[1], "phase") && argc % 2 == 0) {
    for (int i = 2; i + 1 < argc; i += 2) printf("%a\n", siggen_phase(strtod(argv[i], nullptr), strtoull(argv[i + 1], nullptr, 10)));
    return 0;
  }
  fprintf(stderr, "usage: siggen_check selftest | phase A N [A N ...]\n");
  return 2;
}
