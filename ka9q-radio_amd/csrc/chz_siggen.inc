// chz_siggen.inc -- sig_gen's carrier and noise generated on the device, straight into the input ring (part of chz_engine.hip's
// translation unit).
//
// sig_gen (src/sig_gen.c:291-296 REAL, :321-326 COMPLEX) makes each sample from an oscillator step (src/osc.c:28-70) and one or two
// draws of the popcount Gaussian over xoshiro256** (src/gauss.c:47-61,95-111): about 10 ns a sample on one core, more than the
// 7.7 ns a sample lasts at 129.6 MS/s.  Every sample depends only on the stream's parameters and its index (chz_siggen.h), so
// chz_input_generate writes any stretch of the stream into the float ring with one launch of siggen_fill: no samples cross the link,
// the input never repeats, and every device of a sharded run can produce the identical stream by itself.
//
// In ring floats the stream is one draw per float (REAL: a sample is a float; COMPLEX: re then im, one draw each, complex_gauss of
// src/misc.h:399-403), so kernel and host count in floats = draws.
//
// siggen_fill: one wavefront per workgroup, a tile of 64 lanes x R = CHZ_SIGGEN_RUN floats per workgroup.
//   Lane states.  The host passes ONE state, that of the launch's first draw.  The workgroup's first state is T^(64 R w) of it, w the
//   workgroup's number: one matrix-vector product per set bit of w with the tables T^(64 R 2^j).  From there T^R is applied 63 times
//   in a chain, lane k keeping the k-th link.  A product is made by the whole wavefront: lane t holds rows t, 64 + t, 128 + t, 192 + t
//   of the matrix (32 registers, loaded once for the chain), takes the parity of row AND vector, and a ballot assembles each word of
//   the result -- wave-uniform, which is what the next product wants as its input.  No reduction, no LDS, about 80 instructions a
//   product against the about 4600 of a lane doing a product alone (256 columns x 4 words, select and xor); a lane-private product
//   would cost each lane popcount(lane number) of those, so that variant was not built.
//   Carrier.  One sincospi in double per lane at its first sample, from the exact phase (siggen_phase), then a rotation by the step
//   phasor over the lane's at most R samples: at most R 2^-52 away from the closed form, where the reference's own recurrence
//   wanders 8.5e-11 from it within 2^18 samples.
//   Rounding.  The products amplitude * carrier and noise * gauss, their sum and the energy's squares are rounded one by one
//   (CHZ_ROUNDED_F64), as the reference's x86-64 build without FMA rounds them.
//   Stores.  The lanes' runs are transposed through LDS (row stride 65: no bank conflicts while generating) and leave in ring order,
//   a float4 per lane wherever four floats lie inside the write, start 16-byte aligned in the ring and do not straddle its end;
//   scalar stores with the wrap elsewhere (head, tail, the four floats around the ring's end, everything behind the wrap of a ring
//   whose length is no multiple of 4).
//   Energy.  Each lane sums samp^2 (re^2 + im^2) of its valid samples in double, before `scale`, as in_energy is in the reference;
//   the wavefront adds the lanes by xor shuffles, lane 0 stores the workgroup's partial with a plain store, the host adds the partials
//   in index order (chz_input_generate_stats): the same bits every run.
#include "chz_siggen.h"

// A/B builds for scripts/siggen_probe.py only (make ../libchz_hip_sgp1.so | _sgp2.so, loaded through CHZ_LIB; their streams are WRONG):
// 1 derives the lane states and generates nothing, 2 generates every lane's run from the launch's state and derives nothing.
#ifndef CHZ_SIGGEN_PROBE
#define CHZ_SIGGEN_PROBE 0
#endif

namespace chz {

#define SIGGEN_TILE (64 * CHZ_SIGGEN_RUN)
struct SigGenParams {
  float* ring;                 // [ring_len]
  long ring_len, wpos, nf;     // floats: the ring, where the first one goes (< ring_len), how many (<= ring_len)
  const uint64_t* tab;         // [1 + nlev][1024]: rows of T^R, then of T^(64 R 2^j) (siggen_rows)
  int nlev;
  uint64_t s[4];               // the generator's state in front of the launch's first draw
  uint64_t n0;                 // the launch's first sample
  double a;                    // carrier step, cycles per sample (osc_step_cycles)
  double amplitude, noise, scale;
  double* part;                // [gridDim.x] this launch's energy partials
};

// y <- M x for a wave-uniform x; r: this lane's four rows of M
__device__ __forceinline__ void siggen_wave_matvec(const uint64_t r[4][4], uint64_t x[4]) {
  uint64_t y[4];
#pragma unroll
  for (int c = 0; c < 4; c++) {
    const uint64_t v = (r[c][0] & x[0]) ^ (r[c][1] & x[1]) ^ (r[c][2] & x[2]) ^ (r[c][3] & x[3]);
    y[c] = (uint64_t)__ballot(__popcll(v) & 1);
  }
#pragma unroll
  for (int c = 0; c < 4; c++) x[c] = y[c];
}
__device__ __forceinline__ void siggen_load_rows(const uint64_t* __restrict__ level, int lane, uint64_t r[4][4]) {
#pragma unroll
  for (int c = 0; c < 4; c++)
#pragma unroll
    for (int w = 0; w < 4; w++) r[c][w] = level[(c * 64 + lane) * 4 + w];
}
// noise * gauss for one draw, rounded as the reference rounds it
__device__ __forceinline__ double siggen_noise(uint64_t s[4], double noise) {
  const uint64_t u = siggen_next(s);
  double x = (double)((int)__popcll(u * CHZ_SIGGEN_K1) + (int)__popcll(u * CHZ_SIGGEN_K2) - 64);      // (the device's __popcll is unsigned)
  x += (double)(long long)u * (1.0 / 9223372036854775808.0);       // the product is exact
  x *= CHZ_SIGGEN_SIGMA;
  CHZ_ROUNDED_F64(x);
  double t = noise * x;
  CHZ_ROUNDED_F64(t);
  return t;
}

template <bool CPLX>
__global__ void __launch_bounds__(64) siggen_fill(SigGenParams p) {
  constexpr int R = CHZ_SIGGEN_RUN, PER = CPLX ? 2 : 1, STRIDE = R + 1;
  __shared__ float tile[64 * STRIDE];
  const int lane = (int)threadIdx.x;
  const unsigned w = blockIdx.x;
  // ---- lane states
  uint64_t x[4] = {p.s[0], p.s[1], p.s[2], p.s[3]};
  uint64_t s[4] = {x[0], x[1], x[2], x[3]};
#if CHZ_SIGGEN_PROBE != 2
  uint64_t r[4][4];
  for (int j = 0; j < p.nlev; j++) {
    if (!((w >> j) & 1u)) continue;
    siggen_load_rows(p.tab + (size_t)(1 + j) * 1024, lane, r);
    siggen_wave_matvec(r, x);
  }
  s[0] = x[0]; s[1] = x[1]; s[2] = x[2]; s[3] = x[3];
  siggen_load_rows(p.tab, lane, r);
  for (int k = 1; k < 64; k++) {
    siggen_wave_matvec(r, x);
    if (lane == k) { s[0] = x[0]; s[1] = x[1]; s[2] = x[2]; s[3] = x[3]; }
  }
#endif
  // ---- this lane's run
  const long q0 = ((long)w * 64 + lane) * R;          // counted from the launch's first float
  double energy = 0.0;
#if CHZ_SIGGEN_PROBE == 1
  for (int i = 0; i < R; i++) tile[lane * STRIDE + i] = (float)(unsigned)(s[i & 3] >> 40);
  if (false) {
#else
  if (q0 < p.nf) {
#endif
    double sn, cs, ss, cc;
    sincospi(2.0 * siggen_phase(p.a, p.n0 + (uint64_t)(q0 / PER)), &sn, &cs);
    sincospi(2.0 * p.a, &ss, &cc);
    float* __restrict__ row = tile + lane * STRIDE;
#pragma unroll 4
    for (int i = 0; i < R; i += PER) {
      double tr = p.amplitude * cs;
      CHZ_ROUNDED_F64(tr);
      double re = tr + siggen_noise(s, p.noise);
      CHZ_ROUNDED_F64(re);
      row[i] = (float)(re * p.scale);
      double sq = re * re;
      CHZ_ROUNDED_F64(sq);
      if constexpr (CPLX) {
        double ti = p.amplitude * sn;
        CHZ_ROUNDED_F64(ti);
        double im = ti + siggen_noise(s, p.noise);
        CHZ_ROUNDED_F64(im);
        row[i + 1] = (float)(im * p.scale);
        double sq2 = im * im;
        CHZ_ROUNDED_F64(sq2);
        sq += sq2;
      }
      if (q0 + i < p.nf) energy += sq;
      const double c2 = cs * cc - sn * ss, s2 = cs * ss + sn * cc;
      cs = c2; sn = s2;
    }
  }
  __syncthreads();
  // ---- the tile leaves in ring order
  const long base = (long)w * SIGGEN_TILE;            // the tile's first float, counted from the launch's first
  const int mis = (int)(p.wpos & 3);                  // tile float f goes to ring float wpos + base + f: groups of 4 start at f = 4 h - mis
  for (int h = lane; h <= SIGGEN_TILE / 4; h += 64) {
    const int f0 = 4 * h - mis;
    if (f0 >= SIGGEN_TILE) break;
    long pos0 = p.wpos + base + f0;
    if (pos0 >= p.ring_len) pos0 -= p.ring_len;
    if (f0 >= 0 && f0 + 3 < SIGGEN_TILE && base + f0 + 3 < p.nf && pos0 + 4 <= p.ring_len && (pos0 & 3) == 0) {
      float v[4];
#pragma unroll
      for (int k = 0; k < 4; k++) { const int f = f0 + k; v[k] = tile[(f / R) * STRIDE + (f % R)]; }
      *reinterpret_cast<float4*>(p.ring + pos0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int f = f0 + k;
        if (f < 0 || f >= SIGGEN_TILE || base + f >= p.nf) continue;
        long pos = p.wpos + base + f;
        if (pos >= p.ring_len) pos -= p.ring_len;
        p.ring[pos] = tile[(f / R) * STRIDE + (f % R)];
      }
    }
  }
  // ---- energy
  for (int d = 32; d > 0; d >>= 1) energy += __shfl_xor(energy, d);
  if (lane == 0) p.part[w] = energy;
}

inline int siggen_grid(long nf) { return (int)((nf + SIGGEN_TILE - 1) / SIGGEN_TILE); }
inline void launch_siggen_fill(bool cplx, hipStream_t s, const SigGenParams& p, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr) {
  const int grid = siggen_grid(p.nf);
  if (cplx) CHZ_LAUNCH(siggen_fill<true>, grid, 64, 0, s, e0, e1, p);
  else CHZ_LAUNCH(siggen_fill<false>, grid, 64, 0, s, e0, e1, p);
}

}  // namespace chz

// the stream an engine generates, and where it stands
struct SigGenState {
  chz_siggen_params prm{};
  double a = 0.0;                      // osc_step_cycles(prm.freq)
  uint64_t seeded[4] = {}, cur[4] = {};   // the generator in front of draw 0 / in front of the next draw
  unsigned long long pos = 0;          // the next sample
  uint64_t* tab = nullptr; int nlev = 0;
  double* part = nullptr; int max_grid = 0;    // [CHZ_RAW_TICKETS][max_grid]
  unsigned tickets = 0; int grid[CHZ_RAW_TICKETS] = {};
};

static void siggen_free(chz_engine* e) {
  if (!e->siggen) return;
  hipFree(e->siggen->tab); hipFree(e->siggen->part);
  delete e->siggen;
  e->siggen = nullptr;
}

extern "C" {

int chz_siggen_check(int in_type, const chz_siggen_params* p) {
  if (!p) return fail(-1, "null argument");
  if (in_type != CHZ_REAL && in_type != CHZ_COMPLEX) return fail(-1, "unknown input type %d", in_type);
  if (!std::isfinite(p->freq) || !std::isfinite(p->amplitude) || !std::isfinite(p->noise) || !std::isfinite(p->scale))
    return fail(-1, "sig_gen parameters must be finite (freq %g, amplitude %g, noise %g, scale %g)", p->freq, p->amplitude, p->noise, p->scale);
  return 0;
}
int chz_siggen_seed(unsigned long long seed, unsigned long long state[4]) {
  if (!state) return fail(-1, "null argument");
  uint64_t s[4];
  siggen_seed(seed, s);
  for (int i = 0; i < 4; i++) state[i] = s[i];
  return 0;
}
int chz_siggen_jump(unsigned long long state[4], unsigned long long draws_lo, unsigned long long draws_hi) {
  if (!state) return fail(-1, "null argument");
  uint64_t s[4] = {state[0], state[1], state[2], state[3]};
  siggen_jump(s, draws_lo, draws_hi);
  for (int i = 0; i < 4; i++) state[i] = s[i];
  return 0;
}

int chz_input_siggen_set(chz_engine* e, const chz_siggen_params* p) {
  if (!e) return fail(-1, "null engine");
  { int r = chz_siggen_check(e->in_type, p); if (r) return r; }
  if (e->ring16) return fail(-1, "int16 input and generated input cannot be mixed on one engine");
  HIPOK(hipSetDevice(e->device));
  if (!e->siggen) {
    SigGenState* g = new SigGenState();
    struct Guard { SigGenState* g; ~Guard() { if (g) { hipFree(g->tab); hipFree(g->part); delete g; } } } guard{g};
    g->max_grid = siggen_grid(e->ring_len);
    while ((1l << g->nlev) < (long)g->max_grid) g->nlev++;
    std::vector<uint64_t> tab((size_t)(1 + g->nlev) * 1024);
    siggen_rows(CHZ_SIGGEN_RUN_LOG2, tab.data());
    for (int j = 0; j < g->nlev; j++) siggen_rows(CHZ_SIGGEN_RUN_LOG2 + 6 + j, tab.data() + (size_t)(1 + j) * 1024);
    HIPOK(hipMalloc((void**)&g->tab, sizeof(uint64_t) * tab.size()));
    HIPOK(hipMemcpy(g->tab, tab.data(), sizeof(uint64_t) * tab.size(), hipMemcpyHostToDevice));
    HIPOK(hipMalloc((void**)&g->part, sizeof(double) * (size_t)CHZ_RAW_TICKETS * g->max_grid));
    e->siggen = g;
    guard.g = nullptr;
  }
  SigGenState* g = e->siggen;
  g->prm = *p;
  g->a = osc_step_cycles(p->freq);
  siggen_seed(p->seed, g->seeded);
  memcpy(g->cur, g->seeded, sizeof g->cur);
  g->pos = 0;
  return 0;
}
int chz_input_siggen_seek(chz_engine* e, unsigned long long sample) {
  if (!e) return fail(-1, "null engine");
  if (!e->siggen) return fail(-1, "no stream has been described (chz_input_siggen_set)");
  if (sample > CHZ_SIGGEN_MAX_POS) return fail(-1, "sample %llu lies beyond 2^53", sample);
  SigGenState* g = e->siggen;
  memcpy(g->cur, g->seeded, sizeof g->cur);
  siggen_jump(g->cur, sample * (unsigned long long)e->per, 0);       // < 2^54 draws
  g->pos = sample;
  return 0;
}
int chz_input_siggen_tell(chz_engine* e, unsigned long long* sample) {
  if (!e || !sample) return fail(-1, "null argument");
  if (!e->siggen) return fail(-1, "no stream has been described (chz_input_siggen_set)");
  *sample = e->siggen->pos;
  return 0;
}

int chz_input_generate(chz_engine* e, long n, unsigned* ticket) {
  if (!e) return fail(-1, "null engine");
  if (e->ring16) return fail(-1, "int16 input and generated input cannot be mixed on one engine");
  SigGenState* g = e->siggen;
  if (!g) return fail(-1, "no stream has been described (chz_input_siggen_set)");
  if (n < 0) return fail(-1, "generate of %ld samples", n);
  if (n > e->ring_len / e->per) return fail(-1, "generate of %ld samples does not fit the ring", n);
  if ((unsigned long long)n > CHZ_SIGGEN_MAX_POS - g->pos) return fail(-1, "generating %ld samples from sample %llu would pass 2^53", n, g->pos);
  const long nf = n * e->per;
  HIPOK(hipSetDevice(e->device));
  const int slot = (int)(g->tickets % CHZ_RAW_TICKETS);      // still the slot of a readable ticket until this launch has been issued
  int grid = 0;
  if (nf > 0) {
    { int r = welch_guard(e, e->wpos / e->per, n); if (r) return r; }
    SigGenParams p{};
    p.ring = e->ring; p.ring_len = e->ring_len; p.wpos = e->wpos; p.nf = nf;
    p.tab = g->tab; p.nlev = g->nlev;
    memcpy(p.s, g->cur, sizeof p.s);
    p.n0 = g->pos; p.a = g->a;
    p.amplitude = g->prm.amplitude; p.noise = g->prm.noise; p.scale = g->prm.scale;
    p.part = g->part + (size_t)slot * g->max_grid;
    grid = siggen_grid(nf);
    launch_siggen_fill(e->in_type == CHZ_COMPLEX, e->stream, p);
    HIPOK(hipGetLastError());
    e->wpos = (e->wpos + nf) % e->ring_len;
    siggen_jump(g->cur, (uint64_t)nf, 0);
    g->pos += (unsigned long long)n;
    if (e->nlanes > 1) { HIPOK(hipEventRecord(e->input_ready, e->stream)); e->input_pending = true; }
  }
  g->grid[slot] = grid;
  if (ticket) *ticket = g->tickets;
  g->tickets++;
  return 0;
}
int chz_input_generate_stats(chz_engine* e, unsigned ticket, double* energy) {
  if (!e) return fail(-1, "null engine");
  SigGenState* g = e->siggen;
  if (!g || ticket >= g->tickets) return fail(-1, "generate %u has not been issued (%u so far)", ticket, g ? g->tickets : 0u);
  if (g->tickets - ticket > CHZ_RAW_TICKETS) return fail(-1, "the statistics of generate %u are gone: the last %d of %u are kept", ticket, CHZ_RAW_TICKETS, g->tickets);
  HIPOK(hipSetDevice(e->device));
  const int slot = (int)(ticket % CHZ_RAW_TICKETS);
  std::vector<double> part((size_t)g->grid[slot]);
  if (!part.empty()) {
    HIPOK(hipMemcpyAsync(part.data(), g->part + (size_t)slot * g->max_grid, sizeof(double) * part.size(), hipMemcpyDeviceToHost, e->stream));
    HIPOK(hipStreamSynchronize(e->stream));
  }
  double sum = 0.0;
  for (double q : part) sum += q;
  if (energy) *energy = sum;
  return 0;
}

}  // extern "C"
