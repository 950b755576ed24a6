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
  // The narrowband analyser (narrowband_poll(), src/spectrum.c:206-306; chz_bank_welch_*): src_bank >= 0 makes this a bank of analysers
  // of channel bank src_bank's baseband.  Each attached analyser owns a ring of ring_len float2 that bb_ring_append fills behind every
  // block's channel kernel; welch_seg reads it instead of the input ring.  Window, welch_sum, reads and the polls' stream are shared.
  int src_bank = -1;
  bool src_gone = false;           // the channel bank was destroyed
  long long ring_len = 0;          // max_avg * fft_n + (CHZ_ND + 1) * olen
  float2* rings = nullptr;         // [cap][ring_len]
  BbRing* src = nullptr;           // [cap] device copy of src_h
  std::vector<BbRing> src_h;       // [cap] ch < 0: not attached
};

static void welch_free(WelchBank& b) {
  hipFree(b.tw); hipFree(b.tw_h); b.tw_h = nullptr; hipFree(b.window); hipFree(b.part); hipFree(b.bins); hipFree(b.minmax); hipFree(b.slot); hipFree(b.list); hipFree(b.scratch);
  hipFree(b.rings); hipFree(b.src); b.rings = nullptr; b.src = nullptr; b.src_h.clear();
  b.tw = nullptr; b.window = nullptr; b.part = nullptr; b.bins = nullptr; b.minmax = nullptr; b.slot = nullptr; b.list = nullptr; b.scratch = nullptr;
  b.slot_h.clear(); b.overlap_h.clear(); b.list_h.clear(); b.live = false; b.cap = 0;
}
// chz_bank_destroy on a drained engine: the analysers of that bank's channels are detached, their welch banks stay (and refuse polls)
static void welch_bank_gone(chz_engine* e, int bank) {
  for (WelchBank* w : e->welch)
    if (w->live && w->src_bank == bank) { w->src_gone = true; for (BbRing& a : w->src_h) a.ch = -1; }
}
static void welch_free_all(chz_engine* e) {
  for (WelchBank* b : e->welch) { welch_free(*b); delete b; }
  e->welch.clear();
}

#define WELCH_CHECK(e, bank, s0, n) \
  if (!(e) || (bank) < 0 || (bank) >= (int)(e)->welch.size() || !(e)->welch[(size_t)(bank)]->live) return fail(-1, "bad welch bank"); \
  if ((s0) < 0 || (n) < 0 || (s0) + (n) > (e)->welch[(size_t)(bank)]->cap) return fail(-1, "analyser range out of bank capacity")

// narrowband_poll()'s segment walk: the hop the reference takes between two segments -- fft_n forwards while it copies (:259-264), then
// lrint(fft_n overlap) back (:278); NOT lrint(fft_n (1 - overlap)), which differs for odd fft_n -- and where the first one starts (:247)
static void nb_steps(int fft_n, int fft_avg, double overlap, int* hop, long long* adjust) {
  *hop = fft_n - (int)std::lrint(fft_n * overlap);
  *adjust = (long long)std::lrint(fft_n * (1 + (fft_avg - 1) * (1 - overlap)));
}

extern "C" {

#define WELCH_KIND(e, bank, baseband) \
  if (((e)->welch[(size_t)(bank)]->src_bank >= 0) != (baseband)) \
    return fail(-1, (baseband) ? "this call serves banks of chz_bank_welch_create (the narrowband analyser); the bank reads the input ring" \
                               : "this call serves banks of chz_welch_create (the wideband analyser); the bank reads a channel bank's baseband")

// src_bank < 0: the wideband kind, reading the input ring; else the narrowband kind on channel bank src_bank's outputs
static int welch_create(chz_engine* e, int fft_n, int capacity, int max_bins, int max_avg, int src_bank) {
  if (!e) return fail(-1, "null engine");
  if (capacity < 1 || max_bins < 1 || max_avg < 1) return fail(-1, "bad welch bank geometry");
  const bool bb = src_bank >= 0;
  const long long R = bb ? (long long)max_avg * fft_n + (long long)(CHZ_ND + 1) * e->banks[(size_t)src_bank].olen : e->ring_len / e->per;
  WelchBank* b = new WelchBank();
  struct Guard { WelchBank* b; ~Guard() { if (b) { welch_free(*b); delete b; } } } guard{b};
  if (!build_any_geom(fft_n, b->g))
    return fail(-3, "no transform for fft_n=%d: 8 to %d points, and for a length with a prime factor above 13 the chirp-z length 2^k >= 2 fft_n - 1 must fit too", fft_n, CHZ_ANY_MAX_P);
  if (!bb && (long long)fft_n > R) return fail(-3, "fft_n=%d is longer than the input ring (%lld samples)", fft_n, R);
  if (bb && max_bins > fft_n) return fail(-1, "max_bins %d is more than fft_n=%d", max_bins, fft_n);
  if (bb && (size_t)capacity * (size_t)R * sizeof(float2) > ((size_t)16 << 30))
    return fail(-2, "%d baseband rings of %lld samples are more than the bank can hold", capacity, R);
  if ((size_t)capacity * max_avg * (size_t)max_bins > ((size_t)1 << 32)) return fail(-2, "%d analysers x %d segments x %d bins is more than the bank can hold", capacity, max_avg, max_bins);
  HIPOK(hipSetDevice(e->device));
  if (!bb && options().welch_packed && e->in_type == CHZ_REAL && !(fft_n & 1) && !b->g.blue_M && build_any_geom(fft_n / 2, b->gh) && !b->gh.blue_M) b->packed = true;
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
  if (bb) {
    b->src_bank = src_bank; b->ring_len = R;
    HIPOK(hipMalloc((void**)&b->rings, sizeof(float2) * (size_t)capacity * (size_t)R));
    b->src_h.assign((size_t)capacity, BbRing{nullptr, R, 0u, -1});
    for (int i = 0; i < capacity; i++) b->src_h[(size_t)i].ring = b->rings + (size_t)i * (size_t)R;
    HIPOK(hipMalloc((void**)&b->src, sizeof(BbRing) * (size_t)capacity));
    HIPOK(hipMemcpy(b->src, b->src_h.data(), sizeof(BbRing) * (size_t)capacity, hipMemcpyHostToDevice));
  }
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
int chz_welch_create(chz_engine* e, int fft_n, int capacity, int max_bins, int max_avg) { return welch_create(e, fft_n, capacity, max_bins, max_avg, -1); }

// the channel bank's list of attached analysers (Bank::bb), rebuilt from every welch bank that reads it; the engine is drained
static int bb_rebuild(chz_engine* e, int bank) {
  Bank& cb = e->banks[(size_t)bank];
  cb.bb_h.clear();
  for (const WelchBank* w : e->welch)
    if (w->live && w->src_bank == bank && !w->src_gone)
      for (const BbRing& a : w->src_h) if (a.ch >= 0) cb.bb_h.push_back(a);
  std::stable_sort(cb.bb_h.begin(), cb.bb_h.end(), [](const BbRing& a, const BbRing& b) { return a.ch < b.ch; });
  hipFree(cb.bb); cb.bb = nullptr;
  const int n = (int)cb.bb_h.size();
  if (n > 0) {
    HIPOK(hipMalloc((void**)&cb.bb, sizeof(BbRing) * (size_t)n));
    HIPOK(hipMemcpy(cb.bb, cb.bb_h.data(), sizeof(BbRing) * (size_t)n, hipMemcpyHostToDevice));
    if (!cb.bb_done) HIPOK(hipEventCreateWithFlags(&cb.bb_done, hipEventDisableTiming));
    for (int s = 0; s < CHZ_ND; s++) if (!cb.ev_bb[s]) HIPOK(hipEventCreateWithFlags(&cb.ev_bb[s], hipEventDisableTiming));
  }
  cb.bb_n = n;
  return 0;
}
// attach / detach: analyser `slot` of the bank gets channel ch (< 0: none) from block job0 on, on a drained engine
static int bb_set(chz_engine* e, WelchBank& b, int slot, int ch, unsigned job0) {
  { int r = sync_all(e); if (r) return r; }
  drop_graph(e);
  Bank& cb = e->banks[(size_t)b.src_bank];
  BbRing& a = b.src_h[(size_t)slot];
  if (ch >= 0) {
    HIPOK(hipMemset(a.ring, 0, sizeof(float2) * (size_t)b.ring_len));      // the reference's fresh ring is zeros (src/spectrum.c:142-144)
    if (cb.bb_n == 0) { cb.bb_newest = job0 - 1u; for (int s = 0; s < CHZ_ND; s++) cb.bb_rec[s] = false; }
  }
  a.ch = ch; a.job0 = job0;
  HIPOK(hipMemcpy(b.src + slot, &a, sizeof(BbRing), hipMemcpyHostToDevice));
  HIPOK(hipDeviceSynchronize());
  return bb_rebuild(e, b.src_bank);
}

int chz_bank_welch_steps(int fft_n, int fft_avg, double overlap, unsigned job, unsigned job0, int olen, long long ring_len, long long out3[3]) {
  if (fft_n < 1 || fft_avg < 1 || olen < 1 || ring_len < 1 || !out3) return fail(-1, "bad argument");
  int hop; long long adjust; bool before;
  nb_steps(fft_n, fft_avg, overlap, &hop, &adjust);
  out3[0] = hop; out3[1] = adjust;
  out3[2] = bb_ring_pos(job, job0, olen, ring_len, &before);
  if (before) out3[2] = -1;
  return 0;
}
int chz_bank_welch_create(chz_engine* e, int bank, int fft_n, int capacity, int max_bins, int max_avg) {
  if (e) { chz_exit::Scope _xd; if (_xd.ok) (void)hipSetDevice(e->device); }
  BANK_CHECK(e, bank, 0, 0);
  if (!e->banks[(size_t)bank].resp) return fail(-1, "the channel bank has been destroyed");
  if (e->banks[(size_t)bank].out_real) return fail(-1, "the narrowband analyser reads complex baseband: REAL-output banks have none");
  return welch_create(e, fft_n, capacity, max_bins, max_avg, bank);
}
int chz_bank_welch_attach(chz_engine* e, int welch, int slot, int channel, unsigned job0) {
  if (e) { chz_exit::Scope _xd; if (_xd.ok) (void)hipSetDevice(e->device); }
  WELCH_CHECK(e, welch, slot, 1);
  WELCH_KIND(e, welch, true);
  WelchBank& b = *e->welch[(size_t)welch];
  if (b.src_gone) return fail(-1, "the channel bank of this analyser bank has been destroyed");
  if (channel < 0 || channel >= e->banks[(size_t)b.src_bank].cap) return fail(-1, "channel %d outside the bank (capacity %d)", channel, e->banks[(size_t)b.src_bank].cap);
  return bb_set(e, b, slot, channel, job0);
}
int chz_bank_welch_detach(chz_engine* e, int welch, int slot) {
  if (e) { chz_exit::Scope _xd; if (_xd.ok) (void)hipSetDevice(e->device); }
  WELCH_CHECK(e, welch, slot, 1);
  WELCH_KIND(e, welch, true);
  WelchBank& b = *e->welch[(size_t)welch];
  if (b.src_gone || b.src_h[(size_t)slot].ch < 0) return 0;
  return bb_set(e, b, slot, -1, 0u);
}
int chz_bank_welch_configure(chz_engine* e, int welch, int slot, int bin_count, int fft_avg, double overlap) {
  if (e) { chz_exit::Scope _xd; if (_xd.ok) (void)hipSetDevice(e->device); }
  WELCH_CHECK(e, welch, slot, 1);
  WELCH_KIND(e, welch, true);
  WelchBank& b = *e->welch[(size_t)welch];
  if (bin_count < 1 || bin_count > b.max_bins) return fail(-1, "bin_count %d outside 1..%d", bin_count, b.max_bins);
  if (bin_count > b.fft_n) return fail(-1, "bin_count %d is more than fft_n=%d", bin_count, b.fft_n);
  if (fft_avg < 1) return fail(-1, "fft_avg must be at least 1");
  if (!(overlap >= 0.0 && overlap < 1.0)) return fail(-1, "overlap must be in [0, 1)");
  // no clamp to the data on hand: the reference sizes its ring as fft_avg * fft_n, so its limit never binds (:242-246)
  if (fft_avg > b.max_avg) return fail(-1, "fft_avg %d is more than the bank's max_avg %d", fft_avg, b.max_avg);
  drop_graph(e);
  WelchSlot s{};
  s.shift = 0; s.bin_count = bin_count; s.fft_avg = fft_avg;
  nb_steps(b.fft_n, fft_avg, overlap, &s.hop, &s.adjust);
  s.gain = 1.0 / ((double)b.fft_n * b.fft_n * fft_avg);                                  // :255
  b.slot_h[(size_t)slot] = s; b.overlap_h[(size_t)slot] = overlap;
  HIPOK(hipMemcpyAsync(b.slot + slot, &b.slot_h[(size_t)slot], sizeof(WelchSlot), hipMemcpyHostToDevice, e->welch_s));
  HIPOK(hipStreamSynchronize(e->welch_s));
  return fft_avg;
}
int chz_bank_welch_poll(chz_engine* e, int welch, int nslots, const int* slots, unsigned job) {
  if (e) { chz_exit::Scope _xd; if (_xd.ok) (void)hipSetDevice(e->device); }
  WELCH_CHECK(e, welch, 0, nslots);
  WELCH_KIND(e, welch, true);
  if (nslots < 1) return 0;
  WelchBank& b = *e->welch[(size_t)welch];
  if (b.src_gone) return fail(-1, "the channel bank of this analyser bank has been destroyed");
  Bank& cb = e->banks[(size_t)b.src_bank];
  const unsigned newest = __atomic_load_n(&cb.bb_newest, __ATOMIC_RELAXED);
  if ((int)(job - newest) > 0) return fail(-1, "block %u has not been issued yet (the newest is %u)", job, newest);
  if (newest - job > (unsigned)CHZ_ND) return fail(-1, "block %u is older than the rings hold: %u blocks have been issued since, the slack is %d", job, newest - job, CHZ_ND);
  std::vector<int> list((size_t)nslots);
  int segs = 0;
  for (int i = 0; i < nslots; i++) {
    const int s = slots ? slots[i] : i;
    if (s < 0 || s >= b.cap) return fail(-1, "analyser %d out of bank capacity", s);
    const BbRing& a = b.src_h[(size_t)s];
    if (a.ch < 0) return fail(-1, "analyser %d is not attached to a channel", s);
    if ((int)(job - a.job0) < 0) return fail(-1, "block %u lies before analyser %d was attached (block %u)", job, s, a.job0);
    if (b.slot_h[(size_t)s].fft_avg > segs) segs = b.slot_h[(size_t)s].fft_avg;
    list[(size_t)i] = s;
  }
  if (list.size() > b.list_h.size() || !std::equal(list.begin(), list.end(), b.list_h.begin())) {
    HIPOK(hipStreamSynchronize(e->welch_s));          // earlier polls still read the list they were issued with
    HIPOK(hipMemcpyAsync(b.list, list.data(), sizeof(int) * list.size(), hipMemcpyHostToDevice, e->welch_s));
    HIPOK(hipStreamSynchronize(e->welch_s));
    b.list_h = list;
  }
  // behind the appends of every block issued so far, one event per slot
  for (int s = 0; s < CHZ_ND; s++) if (cb.bb_rec[s]) HIPOK(hipStreamWaitEvent(e->welch_s, cb.ev_bb[s], 0));
  WelchParams q{};
  q.ring_samples = 1; q.complex_in = 1;
  q.slot = b.slot; q.list = b.list; q.nslots = nslots; q.segs = segs;
  q.window = b.window; q.part = b.part; q.bins = b.bins; q.minmax = b.minmax;
  q.max_bins = b.max_bins; q.max_avg = b.max_avg; q.fft_n = b.fft_n; q.scratch = b.scratch;
  q.bb = b.src; q.bb_job = job; q.bb_olen = cb.olen;
  if (launch_welch(b.g, q, b.tw, b.scratch_wgs, e->welch_s)) return fail(-3, "welch launch refused (fft_n=%d)", b.fft_n);
  HIPOK(hipGetLastError());
  // The window reaches at most max_avg * fft_n samples back from the end of block `job`, and the ring is (CHZ_ND + 1) blocks longer:
  // the appends of blocks up to job + CHZ_ND + 1 leave it alone, a later one waits for this poll (enqueue_bb_append).  With an earlier poll
  // still running, the older of the two limits stands (the event, re-recorded on the same stream, covers both).
  bool earlier = false;
  if (cb.bb_busy) { earlier = hipEventQuery(cb.bb_done) != hipSuccess; (void)hipGetLastError(); }
  HIPOK(hipEventRecord(cb.bb_done, e->welch_s));
  const unsigned guard = job + (unsigned)CHZ_ND + 1u;
  if (!earlier || (int)(guard - cb.bb_guard) < 0) cb.bb_guard = guard;
  __atomic_store_n(&cb.bb_busy, 1, __ATOMIC_RELEASE);
  return 0;
}

int chz_welch_destroy(chz_engine* e, int bank) {
  if (e) { chz_exit::Scope _xd; if (_xd.ok) (void)hipSetDevice(e->device); }
  WELCH_CHECK(e, bank, 0, 0);
  WelchBank& b = *e->welch[(size_t)bank];
  if (b.src_bank >= 0 && !b.src_gone) {        // the channel bank stops filling this bank's rings
    int r = sync_all(e);
    if (r) return r;
    drop_graph(e);
    for (BbRing& a : b.src_h) a.ch = -1;
    if ((r = bb_rebuild(e, b.src_bank))) return r;
  }
  if (e->welch_s) { HIPOK(hipStreamSynchronize(e->welch_s)); e->welch_busy = false; }
  welch_free(b);         // (the id stays reserved, like a channel bank's)
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
  WELCH_KIND(e, bank, false);
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
  WELCH_KIND(e, bank, false);
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
