// chz_siggen.h -- the arithmetic of sig_gen's sample stream (src/sig_gen.c:291-296, 321-326), as a function of the sample index.
//
// The reference steps an oscillator (src/osc.c:28-70) and a xoshiro256** generator (src/gauss.c:47-61) once per sample.  Both have
// closed forms: the carrier's phase after n steps is frac(a n) with a the angle of the step phasor (osc_step_cycles, chz_finetune.h),
// and the generator's state update is linear over GF(2) -- a 256 x 256 bit matrix T -- so that the state after d draws is T^d state(0),
// popcount(d) matrix-vector products with the matrices T^(2^j).  Everything here is host arithmetic in plain C++ (the engine, the
// kernel siggen_fill in chz_siggen.inc -- which shares siggen_phase and siggen_next -- and a stand-alone check include it); nothing
// touches a device.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <deque>
#include <mutex>
#include <vector>

#if defined(__HIPCC__) || defined(HIPEMU)
#define CHZ_SG_HD __host__ __device__
#else
#define CHZ_SG_HD
#endif

namespace chz {

#define CHZ_SIGGEN_RUN_LOG2 6
#ifndef CHZ_SIGGEN_RUN
#define CHZ_SIGGEN_RUN 64                               // ring floats (= draws) one lane of siggen_fill produces (chz_engine.h says the same)
#endif
static_assert(CHZ_SIGGEN_RUN == 1 << CHZ_SIGGEN_RUN_LOG2, "the run length is a power of two: T^R is one of the squared matrices");
#define CHZ_SIGGEN_MAX_POS (1ull << 53)                 // sample indices are exact doubles

// xoshiro256**: one draw (src/gauss.c:47-61)
CHZ_SG_HD static inline uint64_t siggen_rotl(uint64_t x, int k) { return (x << k) | (x >> (64 - k)); }
CHZ_SG_HD static inline uint64_t siggen_next(uint64_t s[4]) {
  const uint64_t out = siggen_rotl(s[1] * 5, 7) * 9;
  const uint64_t t = s[1] << 17;
  s[2] ^= s[0]; s[3] ^= s[1]; s[1] ^= s[2]; s[0] ^= s[3];
  s[2] ^= t;
  s[3] = siggen_rotl(s[3], 45);
  return out;
}
// the integer part of the popcount Gaussian (src/gauss.c:102-111): x = popc(u K1) + popc(u K2) - 64, then x += (int64)u 2^-63, then
// x *= 0.1765469659009499 -- the callers finish it in double, in that order
#define CHZ_SIGGEN_K1 0x2c1b3c6dULL
#define CHZ_SIGGEN_K2 0x297a2d39ULL
#define CHZ_SIGGEN_SIGMA 0.1765469659009499

// splitmix64 expansion of the seed (src/gauss.c:25-45)
static inline void siggen_seed(uint64_t seed, uint64_t s[4]) {
  uint64_t x = seed;
  for (int i = 0; i < 4; i++) {
    uint64_t z = (x += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    s[i] = z ^ (z >> 31);
  }
  if ((s[0] | s[1] | s[2] | s[3]) == 0) s[0] = 1;
}

// The carrier's phase at sample n, in cycles in [0, 1]: frac(a n) with the product taken exactly (hi + fma remainder, as fine_state_at
// does).  n < 2^53 is an exact double; hi - rint(hi) is exact; the one rounding left is the sum, at most 2^-53.  (A sum that rounds up
// to 1.0 is the same angle as 0.)
CHZ_SG_HD static inline double siggen_phase(double a, uint64_t n) {
  const double g = (double)n;
  double hi = g * a;
  const double lo = fma(g, a, -hi);
  hi -= rint(hi);
  const double x = hi + lo;
  return x - floor(x);
}

// ---- jump-ahead ---------------------------------------------------------------------------------------------------------------------
// Column k of a matrix is its image of unit vector k (bit k % 64 of word k / 64): 4 words.
struct SigGenMat { uint64_t col[256][4]; };

static inline void siggen_matvec(const SigGenMat& m, const uint64_t v[4], uint64_t out[4]) {
  uint64_t r0 = 0, r1 = 0, r2 = 0, r3 = 0;
  for (int w = 0; w < 4; w++) {
    uint64_t bits = v[w];
    while (bits) {
      const int k = 64 * w + __builtin_ctzll(bits);
      bits &= bits - 1;
      r0 ^= m.col[k][0]; r1 ^= m.col[k][1]; r2 ^= m.col[k][2]; r3 ^= m.col[k][3];
    }
  }
  out[0] = r0; out[1] = r1; out[2] = r2; out[3] = r3;
}

// T^(2^j), j = 0 .. 127, made by repeated squaring when first asked for and kept for the life of the process
static inline const SigGenMat& siggen_power(int j) {
  static std::mutex mu;
  static std::deque<SigGenMat> pow2;              // a deque's elements stay where they are when it grows
  std::lock_guard<std::mutex> lk(mu);
  while ((int)pow2.size() <= j) {
    const SigGenMat* prev = pow2.empty() ? nullptr : &pow2.back();
    pow2.emplace_back();
    SigGenMat* m = &pow2.back();
    if (!prev) {
      for (int k = 0; k < 256; k++) {
        uint64_t s[4] = {0, 0, 0, 0};
        s[k >> 6] = 1ull << (k & 63);
        (void)siggen_next(s);
        memcpy(m->col[k], s, sizeof s);
      }
    } else {
      for (int k = 0; k < 256; k++) siggen_matvec(*prev, prev->col[k], m->col[k]);
    }
  }
  return pow2[(size_t)j];
}

// state <- T^draws state, draws = draws_hi 2^64 + draws_lo
static inline void siggen_jump(uint64_t s[4], uint64_t draws_lo, uint64_t draws_hi) {
  for (int j = 0; j < 128; j++) {
    const uint64_t word = j < 64 ? draws_lo : draws_hi;
    if (!((word >> (j & 63)) & 1)) continue;
    uint64_t r[4];
    siggen_matvec(siggen_power(j), s, r);
    memcpy(s, r, sizeof r);
  }
}

// What the kernel reads: the ROWS of T^(2^j) -- bit k of row i is bit i of column k -- so that lane t of a wavefront computes bit t of
// each of the product's four words as a parity and a ballot assembles the word.  Layout: [word c][lane t][4 words of row 64 c + t].
static inline void siggen_rows(int j, uint64_t out[1024]) {
  const SigGenMat& m = siggen_power(j);
  memset(out, 0, sizeof(uint64_t) * 1024);
  for (int k = 0; k < 256; k++)
    for (int c = 0; c < 4; c++) {
      uint64_t bits = m.col[k][c];
      while (bits) {
        const int t = __builtin_ctzll(bits);
        bits &= bits - 1;
        out[(c * 64 + t) * 4 + (k >> 6)] |= 1ull << (k & 63);
      }
    }
}

}  // namespace chz
