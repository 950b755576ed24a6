// chz_filter2.inc -- a bank's filter2 stage, resident on the device (part of chz_engine.hip's translation unit).
//
// radiod puts a channel's private second filter between the fine-tuning rotator and the bb_power sum of downconvert()
// (src/radio.c:1503-1513; created at :1572-1594; share/presets.conf:204,223,297: cwu / cwl with filter2 = 4, isb with 1).
// chz_mini_* serves callers that keep the overlap themselves; here the overlap lives on the device and the stage runs in
// the block pipeline: enqueue_bank() launches f2_ovs (chz_kernels.h) behind every whole-bank channel launch, in block order
// on the demodulator stream, directly in front of the bank's demodulators, which read its output image.  Nothing goes to
// the host in between.  The geometry and its refusals are f2_check_geom's (chz_plan.h); ONE phase per bank: block job0 is
// the first of a cycle of `blocking` blocks, the last block of a cycle fires.
//
// Hazards.  The windows, the responses, the ISB flags and f2_last are only ever touched on the demodulator stream (kernel,
// edits and resets alike), so stream order is block order (chz_run_blocks hands that stream's launches from block to block
// across its issuing threads).  The stage reads the slot's output image behind ev_bank[slot]; the slot's next channel launch,
// four blocks on, waits for ev_tail[slot], recorded behind the stage and the demodulators.  An output image belongs to one
// slot and is rewritten by that slot's next firing block only, on the same stream as its readers.

// a small edit rides the demodulator stream through a pinned staging buffer: effective from the next block enqueued, no drain
static int f2_push(chz_engine* e, Bank& b, void* dst, const void* src, size_t bytes) {
  if (bytes == 0) return 0;
  if (bytes > ((size_t)8 << 20)) {                       // a whole bank being set up: drain once, copy directly
    { int r = sync_all(e); if (r) return r; }
    HIPOK(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    return 0;
  }
  if (b.f2_stage_busy) { HIPOK(hipEventSynchronize(b.f2_stage_ev)); b.f2_stage_busy = false; }      // the edit before this one has left the buffer
  if (bytes > b.f2_stage_bytes) {
    if (b.f2_stage) (void)hipHostFree(b.f2_stage);
    b.f2_stage = nullptr; b.f2_stage_bytes = 0;
    HIPOK(hipHostMalloc((void**)&b.f2_stage, bytes, hipHostMallocDefault));
    b.f2_stage_bytes = bytes;
  }
  if (!b.f2_stage_ev) HIPOK(hipEventCreateWithFlags(&b.f2_stage_ev, hipEventDisableTiming));
  memcpy(b.f2_stage, src, bytes);
  HIPOK(hipMemcpyAsync(dst, b.f2_stage, bytes, hipMemcpyHostToDevice, e->tail));
  HIPOK(hipEventRecord(b.f2_stage_ev, e->tail));
  b.f2_stage_busy = true;
  return 0;
}

static_assert(CHZ_FLAG_PENDING == CHZ_FLAG_PENDING_BIT, "the kernel's flag byte and the header's must agree");

extern "C" {

int chz_bank_filter2_check(int olen, int blocking, int M2) {
  char why[200];
  const int rc = f2_check_geom(olen, blocking, M2, nullptr, why, sizeof why);
  return rc ? fail(rc, "%s", why) : 0;
}

#define F2_BANK(e, bank, ch0, n) \
  BANK_CHECK(e, bank, ch0, n); \
  if (!(e)->banks[(size_t)(bank)].f2_B) return fail(-1, "bank has no filter2: call chz_bank_set_filter2 first")

int chz_bank_set_filter2(chz_engine* e, int bank, unsigned job0, int blocking, int M2) {
  BANK_CHECK(e, bank, 0, 0);
  Bank& b = e->banks[(size_t)bank];
  if (b.out_real) return fail(-1, "filter2 follows COMPLEX-output channels");
  if (!b.fine || !b.power) return fail(-1, "filter2 sits behind the fine-tuning rotator: call chz_bank_set_tuning first");
  if (b.dm_chan) return fail(-1, "filter2 changes the demodulators' block length: call chz_bank_set_filter2 before chz_bank_set_demod");
  if (b.pcm_stride) return fail(-1, "filter2 changes the range of the PCM row size: call chz_bank_set_filter2 before chz_bank_set_pcm_stride");
  if (b.f2_B) return fail(-1, "the bank already has filter2 (blocking %d)", b.f2_B);
  int g3[3]; char why[200];
  { const int rc = f2_check_geom(b.olen, blocking, M2, g3, why, sizeof why); if (rc) return fail(rc, "%s", why); }
  const int L2 = g3[0], N2 = g3[2];
  HIPOK(hipSetDevice(e->device));
  if (f2_prepare(N2)) return fail(-3, "the runtime refuses %zu bytes of LDS per workgroup (N2=%d)", f2_lds_bytes(N2), N2);
  { int r = sync_all(e); if (r) return r; }        // one-time switch
  if (!e->tail) HIPOK(stream_create_masked(&e->tail, true));
  { int r = bank_tail_events(b); if (r) return r; }
  int nimg = 0, img[CHZ_ND];
  for (int s = 0; s < CHZ_ND; s++) {                // slots a firing block can land on: ND / gcd(B, ND) of them
    bool fires = false;
    for (int k = 0; k < CHZ_ND && !fires; k++) fires = (unsigned)(job0 + (unsigned)blocking * (unsigned)(k + 1) - 1u) % CHZ_ND == (unsigned)s;
    img[s] = fires ? nimg++ : -1;
  }
  const size_t cap = (size_t)b.cap;
  struct Undo { Bank* b; ~Undo() { if (b) { hipFree(b->f2_win); hipFree(b->f2_resp); hipFree(b->f2_out); hipFree(b->f2_tw); hipFree(b->f2_isb); hipFree(b->f2_last);
                                            b->f2_win = b->f2_resp = b->f2_out = b->f2_tw = nullptr; b->f2_isb = nullptr; b->f2_last = nullptr; } } } undo{&b};
  HIPOK(hipMalloc((void**)&b.f2_win, sizeof(float2) * cap * N2)); HIPOK(hipMemset(b.f2_win, 0, sizeof(float2) * cap * N2));      // create_filter_input's zeros
  HIPOK(hipMalloc((void**)&b.f2_resp, sizeof(float2) * cap * N2)); HIPOK(hipMemset(b.f2_resp, 0, sizeof(float2) * cap * N2));
  HIPOK(hipMalloc((void**)&b.f2_out, sizeof(float2) * (size_t)nimg * cap * L2)); HIPOK(hipMemset(b.f2_out, 0, sizeof(float2) * (size_t)nimg * cap * L2));
  HIPOK(hipMalloc((void**)&b.f2_isb, cap)); HIPOK(hipMemset(b.f2_isb, 0, cap));
  HIPOK(hipMalloc((void**)&b.f2_last, sizeof(double) * cap)); HIPOK(hipMemset(b.f2_last, 0, sizeof(double) * cap));
  std::vector<f2> tw((size_t)N2);
  for (int k = 0; k < N2; k++) tw[(size_t)k] = root_of_unity(k, N2, -1);
  { int r = upload(&b.f2_tw, tw); if (r) return r; }
  HIPOK(hipDeviceSynchronize());
  undo.b = nullptr;
  b.f2_m = MiniParams{};
  b.f2_m.tw = b.f2_tw; b.f2_m.N = N2; b.f2_m.olen = L2;
  (void)mini_factor(N2, b.f2_m.radix, &b.f2_m.nstages);
  const ChanDescH h = make_chan_desc(CHZ_COMPLEX, N2, N2, 0);      // execute_filter_output(&chan->filter2.out, 0), src/radio.c:1511
  b.f2_d = ChanDesc{h.t0, h.cnt, h.src0, h.dir, h.conj, h.wrap, 0, 0};
  for (int s = 0; s < CHZ_ND; s++) { b.f2_img[s] = img[s]; b.f2_fired[s] = false; }
  b.f2_nimg = nimg; b.f2_L = L2; b.f2_M = g3[1]; b.f2_N = N2; b.f2_job0 = job0; b.f2_seen = false; b.f2_newest = 0;
  b.f2_B = blocking;
  drop_graph(e);
  return 0;
}

int chz_bank_filter2_geometry(chz_engine* e, int bank, int out3[3]) {
  F2_BANK(e, bank, 0, 0);
  if (!out3) return fail(-1, "null argument");
  const Bank& b = e->banks[(size_t)bank];
  out3[0] = b.f2_L; out3[1] = b.f2_M; out3[2] = b.f2_N;
  return 0;
}

// response[N2] complex per channel as set_filter leaves it (src/radio.c:1591-1594); zeros until set
int chz_bank_set_filter2_responses(chz_engine* e, int bank, int ch0, int n, const float* resp) {
  F2_BANK(e, bank, ch0, n);
  if (!resp) return fail(-1, "null argument");
  Bank& b = e->banks[(size_t)bank];
  HIPOK(hipSetDevice(e->device));
  return f2_push(e, b, b.f2_resp + (size_t)ch0 * b.f2_N, resp, sizeof(float2) * (size_t)n * b.f2_N);
}

// chan->filter2.out.isb (src/radio.c:1569,1586)
int chz_bank_set_filter2_isb(chz_engine* e, int bank, int ch0, int n, const unsigned char* flags) {
  F2_BANK(e, bank, ch0, n);
  if (!flags) return fail(-1, "null argument");
  Bank& b = e->banks[(size_t)bank];
  HIPOK(hipSetDevice(e->device));
  std::vector<unsigned char> f((size_t)n);
  for (int i = 0; i < n; i++) f[(size_t)i] = flags[i] ? 1 : 0;
  return f2_push(e, b, b.f2_isb + ch0, f.data(), (size_t)n);
}

// set_channel_filter()'s delete_filter_input + create_filter_input (src/radio.c:1570-1583): the channels' windows are zeros
// again from block `job` on -- the next block to be enqueued, and the first of a cycle (the bank has one phase)
int chz_bank_filter2_reset(chz_engine* e, int bank, unsigned job, int ch0, int n) {
  F2_BANK(e, bank, ch0, n);
  Bank& b = e->banks[(size_t)bank];
  if (f2_phase(job, b.f2_job0, b.f2_B) != 0)
    return fail(-1, "block %u is number %d of its filter2 cycle of %d: a reset starts a cycle", job, f2_phase(job, b.f2_job0, b.f2_B), b.f2_B);
  if (b.f2_seen ? job != b.f2_newest + 1u : job != b.f2_job0)
    return fail(-1, "a filter2 reset takes effect at the next block to be enqueued (%u), not at block %u", b.f2_seen ? b.f2_newest + 1u : b.f2_job0, job);
  if (n == 0) return 0;
  HIPOK(hipSetDevice(e->device));
  HIPOK(hipMemsetAsync(b.f2_win + (size_t)ch0 * b.f2_N, 0, sizeof(float2) * (size_t)n * b.f2_N, e->tail));
  return 0;
}

static int f2_read(chz_engine* e, int bank, int slot, int ch0, int n, float* host, bool wait) {
  F2_BANK(e, bank, ch0, n);
  if (slot < 0 || slot >= CHZ_ND || !host) return fail(-1, "bad argument");
  Bank& b = e->banks[(size_t)bank];
  if (b.f2_img[slot] < 0 || !b.f2_fired[slot]) return fail(-1, "slot %d's last block was pending: filter2 did not fire on it", slot);
  if (n == 0) return 0;
  const float2* src = b.f2_out + ((size_t)b.f2_img[slot] * b.cap + ch0) * b.f2_L;
  HIPOK(hipMemcpyAsync(host, src, sizeof(float2) * (size_t)n * b.f2_L, hipMemcpyDeviceToHost, e->tail));
  if (wait) HIPOK(hipStreamSynchronize(e->tail));
  return 0;
}
int chz_bank_filter2_read(chz_engine* e, int bank, int slot, int ch0, int n, float* host) {
  if (e) { chz_exit::Scope _xd; if (_xd.ok) (void)hipSetDevice(e->device); }
  return f2_read(e, bank, slot, ch0, n, host, true);
}
int chz_bank_filter2_read_async(chz_engine* e, int bank, int slot, int ch0, int n, float* host) {
  if (e) { chz_exit::Scope _xd; if (_xd.ok) (void)hipSetDevice(e->device); }
  return f2_read(e, bank, slot, ch0, n, host, false);
}

}  // extern "C"
