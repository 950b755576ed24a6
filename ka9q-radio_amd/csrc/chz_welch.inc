// chz_welch.inc -- Welch power spectra of the raw input (part of chz_engine.hip's translation unit).
//
// radiod's wideband spectrum analyser (wideband_poll(), src/spectrum.c:308-522) reads the raw A/D ring on the host, windows
// fft_avg overlapping segments of fft_n samples, transforms each and sums |X|^2 of the requested bins -- per poll and per client
// (ka9q-web opens one analyser per client).  The same samples already lie in the engine's HBM ring: a WelchBank holds every
// analyser of one fft_n, and ONE launch pair (welch_seg + welch_sum, chz_kernels.h) serves all that are due.
// Polls run on a stream of their own, ordered behind the input writes issued before them; the one dependency the other way --
// a later input write overwriting samples an unfinished poll still reads -- is one event (welch_guard in chz_engine.hip).
struct WelchBank {
  int fft_n = 0, cap = 0, max_bins = 0, max_avg = 0;
  bool live = false;
  ChanGeom g;
  float2* tw = nullptr;            // g.tw_any
  // real front end, even fft_n, option welch_packed: the transform runs over fft_n/2 packed points (gh, tw_h) and welch_seg splits
  // the bins it reads with the fft_n-point table `tw`
  bool packed = false;
  ChanGeom gh;
  float2* tw_h = nullptr;
  float* window = nullptr;         // [cap][fft_n]
  float* part = nullptr;           // [cap][max_avg][max_bins] |X|^2 per segment
  float* bins = nullptr;           // [cap][max_bins]
  double* minmax = nullptr;        // [cap][2]
  WelchSlot* slot = nullptr;       // [cap]
  int* list = nullptr;             // [cap] the analysers of the latest poll
  float2* scratch = nullptr; int scratch_wgs = 0;      // transform buffers beyond the LDS (welch_seg<true>)
  std::vector<WelchSlot> slot_h;
  std::vector<double> overlap_h;
  std::vector<int> list_h;         // what `list` holds
};

static void welch_free(WelchBank& b) {
  hipFree(b.tw); hipFree(b.tw_h); b.tw_h = nullptr; hipFree(b.window); hipFree(b.part); hipFree(b.bins); hipFree(b.minmax); hipFree(b.slot); hipFree(b.list); hipFree(b.scratch);
  b.tw = nullptr; b.window = nullptr; b.part = nullptr; b.bins = nullptr; b.minmax = nullptr; b.slot = nullptr; b.list = nullptr; b.scratch = nullptr;
  b.slot_h.clear(); b.overlap_h.clear(); b.list_h.clear(); b.live = false; b.cap = 0;
}
static void welch_free_all(chz_engine* e) {
  for (WelchBank* b : e->welch) { welch_free(*b); delete b; }
  e->welch.clear();
}

#define WELCH_CHECK(e, bank, s0, n) \
  if (!(e) || (bank) < 0 || (bank) >= (int)(e)->welch.size() || !(e)->welch[(size_t)(bank)]->live) return fail(-1, "bad welch bank"); \
  if ((s0) < 0 || (n) < 0 || (s0) + (n) > (e)->welch[(size_t)(bank)]->cap) return fail(-1, "analyser range out of bank capacity")

extern "C" {

int chz_welch_create(chz_engine* e, int fft_n, int capacity, int max_bins, int max_avg) {
  if (!e) return fail(-1, "null engine");
  if (capacity < 1 || max_bins < 1 || max_avg < 1) return fail(-1, "bad welch bank geometry");
  const long long R = e->ring_len / e->per;
  WelchBank* b = new WelchBank();
  struct Guard { WelchBank* b; ~Guard() { if (b) { welch_free(*b); delete b; } } } guard{b};
  if (!build_any_geom(fft_n, b->g))
    return fail(-3, "no transform for fft_n=%d: 8 to %d points, and for a length with a prime factor above 13 the chirp-z length 2^k >= 2 fft_n - 1 must fit too", fft_n, CHZ_ANY_MAX_P);
  if ((long long)fft_n > R) return fail(-3, "fft_n=%d is longer than the input ring (%lld samples)", fft_n, R);
  if ((size_t)capacity * max_avg * (size_t)max_bins > ((size_t)1 << 32)) return fail(-2, "%d analysers x %d segments x %d bins is more than the bank can hold", capacity, max_avg, max_bins);
  HIPOK(hipSetDevice(e->device));
  if (options().welch_packed && e->in_type == CHZ_REAL && !(fft_n & 1) && !b->g.blue_M && build_any_geom(fft_n / 2, b->gh) && !b->gh.blue_M) b->packed = true;
  const ChanGeom& tg = b->packed ? b->gh : b->g;       // the transform that is executed
  if (!tg.big && welch_prepare()) return fail(-3, "the runtime refuses %zu bytes of LDS per workgroup (fft_n=%d)", b->g.lds, fft_n);
  b->fft_n = fft_n; b->cap = capacity; b->max_bins = max_bins; b->max_avg = max_avg;
  if (!e->welch_s) {
    HIPOK(stream_create_masked(&e->welch_s, true));          // a hardware queue of its own, like the demodulator stream
    HIPOK(hipEventCreateWithFlags(&e->welch_in, hipEventDisableTiming));
    HIPOK(hipEventCreateWithFlags(&e->welch_done, hipEventDisableTiming));
  }
  int r = upload(&b->tw, b->g.tw_any);
  if (r) return r;
  if (b->packed && (r = upload(&b->tw_h, b->gh.tw_any))) return r;
  HIPOK(hipMalloc((void**)&b->window, sizeof(float) * (size_t)capacity * fft_n));
  HIPOK(hipMemset(b->window, 0, sizeof(float) * (size_t)capacity * fft_n));
  HIPOK(hipMalloc((void**)&b->part, sizeof(float) * (size_t)capacity * max_avg * max_bins));
  HIPOK(hipMalloc((void**)&b->bins, sizeof(float) * (size_t)capacity * max_bins));
  HIPOK(hipMemset(b->bins, 0, sizeof(float) * (size_t)capacity * max_bins));
  HIPOK(hipMalloc((void**)&b->minmax, sizeof(double) * 2 * (size_t)capacity));
  HIPOK(hipMemset(b->minmax, 0, sizeof(double) * 2 * (size_t)capacity));
  b->slot_h.assign((size_t)capacity, WelchSlot{0, 0, 0, 0, 0, 0.0});
  b->overlap_h.assign((size_t)capacity, 0.0);
  HIPOK(hipMalloc((void**)&b->slot, sizeof(WelchSlot) * (size_t)capacity));
  HIPOK(hipMemset(b->slot, 0, sizeof(WelchSlot) * (size_t)capacity));
  HIPOK(hipMalloc((void**)&b->list, sizeof(int) * (size_t)capacity));
  HIPOK(hipMemset(b->list, 0, sizeof(int) * (size_t)capacity));
  if (tg.big) {
    // one pair of buffers per workgroup in flight, not per work item: welch_seg walks its items with a grid stride
    const size_t per = sizeof(float2) * 2 * (size_t)tg.lb;
    long wgs = (long)capacity * max_avg; if (wgs > 256) wgs = 256;
    while (wgs > 1 && per * (size_t)wgs > ((size_t)4 << 30)) wgs /= 2;
    b->scratch_wgs = (int)wgs;
    HIPOK(hipMalloc((void**)&b->scratch, per * (size_t)wgs));
  }
  HIPOK(hipDeviceSynchronize());       // null-stream memsets vs the engine's non-blocking streams
  b->live = true;
  guard.b = nullptr;
  e->welch.push_back(b);
  return (int)e->welch.size() - 1;
}

int chz_welch_destroy(chz_engine* e, int bank) {
  if (e) { chz_exit::Scope _xd; if (_xd.ok) (void)hipSetDevice(e->device); }
  WELCH_CHECK(e, bank, 0, 0);
  if (e->welch_s) { HIPOK(hipStreamSynchronize(e->welch_s)); e->welch_busy = false; }
  welch_free(*e->welch[(size_t)bank]);         // (the id stays reserved, like a channel bank's)
  return 0;
}

int chz_welch_set_window(chz_engine* e, int bank, int slot, const float* window) {
  if (e) { chz_exit::Scope _xd; if (_xd.ok) (void)hipSetDevice(e->device); }
  WELCH_CHECK(e, bank, slot, 1);
  if (!window) return fail(-1, "null window");
  WelchBank& b = *e->welch[(size_t)bank];
  // in the polls' own stream: a poll already enqueued keeps the window it was issued with
  HIPOK(hipMemcpyAsync(b.window + (size_t)slot * b.fft_n, window, sizeof(float) * (size_t)b.fft_n, hipMemcpyHostToDevice, e->welch_s));
  HIPOK(hipStreamSynchronize(e->welch_s));     // the caller's buffer may be pageable / reused
  return 0;
}

int chz_welch_configure(chz_engine* e, int bank, int slot, int shift, int bin_count, int fft_avg, double overlap) {
  if (e) { chz_exit::Scope _xd; if (_xd.ok) (void)hipSetDevice(e->device); }
  WELCH_CHECK(e, bank, slot, 1);
  WelchBank& b = *e->welch[(size_t)bank];
  if (bin_count < 1 || bin_count > b.max_bins) return fail(-1, "bin_count %d outside 1..%d", bin_count, b.max_bins);
  if (fft_avg < 1) return fail(-1, "fft_avg must be at least 1");
  if (!(overlap >= 0.0 && overlap < 1.0)) return fail(-1, "overlap must be in [0, 1)");
  // Limit averaging to the data on hand (src/spectrum.c:359-361,417-419), with the DEVICE ring's length in samples
  const long long R = e->ring_len / e->per;
  const double avg_limit = std::floor(1 + (double)(R / b.fft_n - 1) / (1 - overlap));
  if ((double)fft_avg > avg_limit) fft_avg = (int)avg_limit;
  if (fft_avg > b.max_avg) return fail(-1, "fft_avg %d is more than the bank's max_avg %d", fft_avg, b.max_avg);
  const bool real = e->in_type == CHZ_REAL;
  WelchSlot s{};
  s.shift = shift; s.bin_count = bin_count; s.fft_avg = fft_avg;
  s.hop = (int)std::lrint(b.fft_n * (1. - overlap));                                     // :407,:491
  s.adjust = (long long)std::lrint(b.fft_n * (1 + (fft_avg - 1) * (1 - overlap)));       // :364,:422
  s.gain = (real ? 2. : 1.) / (double)((long long)fft_avg * b.fft_n * b.fft_n);          // :373,:431
  b.slot_h[(size_t)slot] = s; b.overlap_h[(size_t)slot] = overlap;
  HIPOK(hipMemcpyAsync(b.slot + slot, &b.slot_h[(size_t)slot], sizeof(WelchSlot), hipMemcpyHostToDevice, e->welch_s));
  HIPOK(hipStreamSynchronize(e->welch_s));
  return fft_avg;
}

int chz_welch_poll(chz_engine* e, int bank, int nslots, const int* slots, long long end_sample) {
  if (e) { chz_exit::Scope _xd; if (_xd.ok) (void)hipSetDevice(e->device); }
  WELCH_CHECK(e, bank, 0, nslots);
  if (nslots < 1) return 0;
  WelchBank& b = *e->welch[(size_t)bank];
  const long long R = e->ring_len / e->per;
  std::vector<int> list((size_t)nslots);
  for (int i = 0; i < nslots; i++) {
    const int s = slots ? slots[i] : i;
    if (s < 0 || s >= b.cap) return fail(-1, "analyser %d out of bank capacity", s);
    list[(size_t)i] = s;
  }
  if (list.size() > b.list_h.size() || !std::equal(list.begin(), list.end(), b.list_h.begin())) {
    HIPOK(hipStreamSynchronize(e->welch_s));          // earlier polls still read the list they were issued with
    HIPOK(hipMemcpyAsync(b.list, list.data(), sizeof(int) * list.size(), hipMemcpyHostToDevice, e->welch_s));
    HIPOK(hipStreamSynchronize(e->welch_s));
    b.list_h = list;
  }
  const bool cplx = e->in_type == CHZ_COMPLEX;
  int segs = 0; long long back = 0, fwd = 0;
  for (int s : list) {
    const WelchSlot& d = b.slot_h[(size_t)s];
    if (d.fft_avg > segs) segs = d.fft_avg;
    const long long span = (long long)(d.fft_avg - 1) * d.hop;
    const long long bk = cplx ? d.adjust + span : d.adjust;                       // how far in front of `end` the oldest sample lies
    const long long fw = (cplx ? 0 : span) + b.fft_n - d.adjust;                  // how far past it the newest one (rounding of adjust / hop)
    if (bk > back) back = bk;
    if (fw > fwd) fwd = fw;
  }
  const long long end = end_sample < 0 ? (long long)(e->wpos / e->per) : end_sample % R;
  // behind every input write issued so far
  HIPOK(hipEventRecord(e->welch_in, e->stream));
  HIPOK(hipStreamWaitEvent(e->welch_s, e->welch_in, 0));
  WelchParams q{};
  q.ring = e->ring; q.ring16 = e->ring16; q.scale16 = e->scale16; q.derand = e->derand;
  q.ring_samples = R; q.end = end; q.complex_in = cplx ? 1 : 0;
  q.slot = b.slot; q.list = b.list; q.nslots = nslots; q.segs = segs;
  q.window = b.window; q.part = b.part; q.bins = b.bins; q.minmax = b.minmax;
  q.max_bins = b.max_bins; q.max_avg = b.max_avg; q.fft_n = b.fft_n; q.scratch = b.scratch;
  q.packed = b.packed ? 1 : 0; q.tw_split = b.tw;
  if (launch_welch(b.packed ? b.gh : b.g, q, b.packed ? b.tw_h : b.tw, b.scratch_wgs, e->welch_s)) return fail(-3, "welch launch refused (fft_n=%d)", b.fft_n);
  HIPOK(hipGetLastError());
  // the ring samples this poll reads, for the input writes that follow (welch_guard); an earlier poll that may still be
  // running has a region of its own: together they are, conservatively, the whole ring
  bool earlier = false;
  if (e->welch_busy) { earlier = hipEventQuery(e->welch_done) != hipSuccess; (void)hipGetLastError(); }
  HIPOK(hipEventRecord(e->welch_done, e->welch_s));
  long long len = back + fwd;
  if (earlier || len >= R) { e->welch_lo = 0; e->welch_len = R; }
  else { e->welch_lo = ((end - back) % R + R) % R; e->welch_len = len; }
  e->welch_busy = true;
  return 0;
}

static int welch_read(chz_engine* e, int bank, int slot0, int n, float* bins, double* minmax, bool wait) {
  if (e) { chz_exit::Scope _xd; if (_xd.ok) (void)hipSetDevice(e->device); }
  WELCH_CHECK(e, bank, slot0, n);
  WelchBank& b = *e->welch[(size_t)bank];
  if (n == 0) return 0;
  if (bins) HIPOK(hipMemcpyAsync(bins, b.bins + (size_t)slot0 * b.max_bins, sizeof(float) * (size_t)n * b.max_bins, hipMemcpyDeviceToHost, e->welch_s));
  if (minmax) HIPOK(hipMemcpyAsync(minmax, b.minmax + 2 * (size_t)slot0, sizeof(double) * 2 * (size_t)n, hipMemcpyDeviceToHost, e->welch_s));
  if (wait) HIPOK(hipStreamSynchronize(e->welch_s));
  return 0;
}
int chz_welch_read(chz_engine* e, int bank, int slot0, int n, float* bins, double* minmax) { return welch_read(e, bank, slot0, n, bins, minmax, true); }
int chz_welch_read_async(chz_engine* e, int bank, int slot0, int n, float* bins, double* minmax) { return welch_read(e, bank, slot0, n, bins, minmax, false); }

}  // extern "C"
