// chz_mpx.inc -- pools of FM-multiplex decoders: stereod's and rdsd's decode() loops (part of chz_engine.hip's translation unit).
//
// stereod (src/stereod.c:373-408, :460-513) and rdsd (src/rdsd.c:385-413, :465-500) keep, per session, a REAL master of L = 384 kHz x
// Blocktime samples of the FM multiplex, M = L + 1, with three (mono, the 19 kHz pilot, L-R around 38 kHz) or two (the pilot, RDS around
// 57 kHz) decimating slaves of olen = L / 8 samples, and behind them a per-sample loop: stereod's stereo matrix with two de-emphasis
// recurrences and the 16-bit packer, rdsd's packer alone.  A pool holds the responses and the state of all sessions of one geometry --
// (block time, kind, input byte order) --; ONE launch of mpx_ovs (chz_kernels.h) serves every session that is due, one workgroup per
// request, from the samples to the packed PCM.  The decoder is a recurrence over blocks: the filter's history, the two de-emphasis states
// and the parameters live on the device, per instance.  What crosses the link is 2 L bytes and a request record down, a 24-byte status
// record and 4 olen bytes of PCM up, plus the 2 olen floats the packer was fed for a chunk in which a request asks for them.  `capacity`
// is the number of requests one launch serves; the instances' storage starts at as many and doubles when chz_mpx_add finds it full.
struct chz_mpx {
  int L = 0, M = 0, N = 0, olen = 0, P = 0, pilot_shift = 0, subc_shift = 0, kind = 0, nslaves = 0, big_endian = 0, cap = 0, ninst = 0, device = 0;
  double blocktime = 0;
  MpxParams kp{};                                  // everything that does not change from launch to launch
  size_t lds = 0; int threads = 0;
  hipStream_t s = nullptr;
  float2* resp = nullptr;        // [ninst][nslaves][P]
  float2* tw = nullptr;          // forward [N/2], split [N/2 + 1], slaves [P]
  MpxState* state = nullptr;     // [ninst]
  float* hist = nullptr;         // [ninst][L]
  // staging for one chunk of k <= cap requests, device and pinned: the k request records, then the samples of those that bring them from
  // the host (ONE copy carries both); back: the k status records and the k PCM rows behind them (ONE copy), and the k rows of floats when a
  // request of the chunk wants its own
  unsigned char *d_stage = nullptr, *h_stage = nullptr, *d_out = nullptr, *h_out = nullptr;
  float *d_audio = nullptr, *h_audio = nullptr;
  std::vector<int> free_inst;
  std::vector<unsigned char> used, seen;
  std::mutex mu;
};
static_assert(sizeof(MpxStatusK) == sizeof(chz_mpx_status), "mpx_ovs writes chz_mpx_status records");
static_assert(sizeof(MpxState) == 2 * sizeof(double) + sizeof(chz_mpx_params), "chz_mpx_set_params writes the tail of an MpxState");
static_assert(CHZ_MPX_STEREO == CHZ_MPX_KIND_STEREO && CHZ_MPX_RDS == CHZ_MPX_KIND_RDS && CHZ_MPX_STEREO == CHZ_MPX_STEREO_K && CHZ_MPX_RDS == CHZ_MPX_RDS_K,
              "the header, the checker and the kernel name the kinds alike");
static_assert(CHZ_MPX_RED == CHZ_MPX_RED_DOUBLES, "the checker sizes the kernel's scratch");

// what a fresh decode() thread starts from: zero states, stereod's own Deemph_rate = exp(-1 / (Deemph_tc * Audio_samprate)) with Deemph_tc =
// 75 us, and Deemph_gain = 4 (src/stereod.c:68,213-214)
static MpxState mpx_fresh_state() { return MpxState{0.0, 0.0, exp(-1.0 / (75.0e-6 * CHZ_MPX_AUDIO_RATE)), 4.0}; }

// storage for n instances (n > m->ninst): new arrays, the old contents copied over, the new instances' state and history zero
static int mpx_grow(chz_mpx* m, int n) {
  float2* resp = nullptr; MpxState* state = nullptr; float* hist = nullptr;
  const size_t PS = (size_t)m->nslaves * m->P, L = (size_t)m->L, old = (size_t)m->ninst;
  struct Guard { float2*& r; MpxState*& s; float*& h; ~Guard() { hipFree(r); hipFree(s); hipFree(h); } } guard{resp, state, hist};
  HIPOK(hipMalloc((void**)&resp, sizeof(float2) * PS * n));
  HIPOK(hipMalloc((void**)&state, sizeof(MpxState) * (size_t)n));
  HIPOK(hipMalloc((void**)&hist, sizeof(float) * L * n));
  HIPOK(hipMemsetAsync(resp, 0, sizeof(float2) * PS * n, m->s));
  HIPOK(hipMemsetAsync(state, 0, sizeof(MpxState) * (size_t)n, m->s));
  HIPOK(hipMemsetAsync(hist, 0, sizeof(float) * L * n, m->s));
  if (old) {
    HIPOK(hipMemcpyAsync(resp, m->resp, sizeof(float2) * PS * old, hipMemcpyDeviceToDevice, m->s));
    HIPOK(hipMemcpyAsync(state, m->state, sizeof(MpxState) * old, hipMemcpyDeviceToDevice, m->s));
    HIPOK(hipMemcpyAsync(hist, m->hist, sizeof(float) * L * old, hipMemcpyDeviceToDevice, m->s));
  }
  HIPOK(hipStreamSynchronize(m->s));
  std::swap(resp, m->resp); std::swap(state, m->state); std::swap(hist, m->hist);      // (the guard frees the old arrays)
  m->kp.state = m->state; m->kp.hist = m->hist;
  for (int s = 0; s < m->nslaves; s++) m->kp.s[s].m.resp = m->resp + (size_t)s * m->P;   // row nslaves x inst of slave s: instance inst
  m->used.resize((size_t)n, 0); m->seen.resize((size_t)n, 0);
  for (int i = n - 1; i >= m->ninst; i--) m->free_inst.push_back(i);
  m->ninst = n;
  return 0;
}

extern "C" {

void chz_mpx_destroy(chz_mpx* m) {
  if (!m) return;
  hipSetDevice(m->device);
  if (m->s) hipStreamSynchronize(m->s);
  hipFree(m->resp); hipFree(m->tw); hipFree(m->state); hipFree(m->hist); hipFree(m->d_stage); hipFree(m->d_out); hipFree(m->d_audio);
  if (m->h_stage) (void)hipHostFree(m->h_stage);
  if (m->h_out) (void)hipHostFree(m->h_out);
  if (m->h_audio) (void)hipHostFree(m->h_audio);
  if (m->s) hipStreamDestroy(m->s);
  delete m;
}

// would chz_mpx_create take this?  0, or < 0 with the reason in chz_last_error(); touches no device
int chz_mpx_check(double blocktime, int kind, int byte_order) {
  char why[240];
  const int rc = mpx_check_geom(blocktime, kind, byte_order, nullptr, why, sizeof why);
  return rc ? fail(rc, "%s", why) : 0;
}

int chz_mpx_create(chz_mpx** out, double blocktime, int kind, int byte_order, int capacity, int device) {
  if (!out) return fail(-1, "null out pointer");
  *out = nullptr;
  if (capacity < 1) return fail(-1, "bad FM-multiplex decoder pool capacity");
  int g[7] = {};
  { char why[240]; const int rc = mpx_check_geom(blocktime, kind, byte_order, g, why, sizeof why); if (rc) return fail(rc, "%s", why); }
  chz_mpx* m = new chz_mpx();
  struct Guard { chz_mpx* m; ~Guard() { if (m) chz_mpx_destroy(m); } } guard{m};
  const int L = g[0], N = g[2], olen = g[3], P = g[4], H = N / 2, bins = H + 1;
  const bool stereo = kind == CHZ_MPX_STEREO;
  m->L = L; m->M = g[1]; m->N = N; m->olen = olen; m->P = P; m->pilot_shift = g[5]; m->subc_shift = g[6]; m->kind = kind;
  m->nslaves = stereo ? 3 : 2; m->big_endian = byte_order == CHZ_MPX_BE; m->cap = capacity; m->device = device; m->blocktime = blocktime;
  MpxParams& kp = m->kp;
  kp.N = N; kp.olen = olen; kp.kind = kind; kp.big_endian = m->big_endian; kp.nslaves = m->nslaves; kp.fwd.N = H;
  kp.deemph_lanes = options().mpx_deemph_lanes;
  mini_factor(H, kp.fwd.radix, &kp.fwd.nstages);
  const int shifts[3] = {stereo ? 0 : m->pilot_shift, stereo ? m->pilot_shift : m->subc_shift, m->subc_shift};
  for (int s = 0; s < m->nslaves; s++) {
    RminiSlave& sl = kp.s[s];
    sl.m.N = P; sl.m.olen = olen;
    mini_factor(P, sl.m.radix, &sl.m.nstages);
    sl.real_out = stereo && s == 0; sl.out_off = 0;
    const ChanDescH h = make_chan_desc(CHZ_REAL, bins, P, shifts[s]);
    kp.d[s] = ChanDesc{h.t0, h.cnt, h.src0, h.dir, h.conj, h.wrap, 0, shifts[s]};
  }
  mpx_launch_geom(N, P, olen, kind, &kp.out_off, &kp.red_off, &m->lds, &m->threads);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(-2, "no HIP device: there is no CPU fallback");
  if (device < 0 || device >= ndev) return fail(-2, "device %d out of range (%d devices)", device, ndev);
  HIPOK(hipSetDevice(device));
  if (m->lds > 64 * 1024 && big_lds_prepare(reinterpret_cast<const void*>(mpx_ovs)))
    return fail(-3, "the runtime refuses %zu bytes of LDS per workgroup (N=%d)", m->lds, N);
  HIPOK(hipStreamCreateWithFlags(&m->s, hipStreamNonBlocking));
  std::vector<f2> tw((size_t)H + (size_t)H + 1 + (size_t)P);
  size_t at = 0;
  for (int k = 0; k < H; k++) tw[at++] = root_of_unity(k, H, -1);
  for (int k = 0; k <= H; k++) tw[at++] = root_of_unity(k, N, -1);
  for (int k = 0; k < P; k++) tw[at++] = root_of_unity(k, P, -1);
  int r = upload(&m->tw, tw);
  if (r) return r;
  kp.fwd.tw = m->tw; kp.tw_split = m->tw + H;
  for (int s = 0; s < m->nslaves; s++) kp.s[s].m.tw = m->tw + (size_t)H + (size_t)H + 1;
  r = mpx_grow(m, capacity);
  if (r) return r;
  static_assert(sizeof(MpxReq) % 8 == 0 && sizeof(MpxStatusK) % 8 == 0, "the samples follow the request records, the PCM rows the status records");
  const size_t stage = (sizeof(MpxReq) + sizeof(short) * (size_t)L) * (size_t)capacity;
  const size_t outb = (sizeof(MpxStatusK) + 4 * (size_t)olen) * (size_t)capacity;
  const size_t arow = sizeof(float) * 2 * (size_t)olen;
  HIPOK(hipMalloc((void**)&m->d_stage, stage));
  HIPOK(hipMalloc((void**)&m->d_out, outb));
  HIPOK(hipMalloc((void**)&m->d_audio, arow * (size_t)capacity));
  HIPOK(hipHostMalloc((void**)&m->h_stage, stage, hipHostMallocDefault));
  HIPOK(hipHostMalloc((void**)&m->h_out, outb, hipHostMallocDefault));
  HIPOK(hipHostMalloc((void**)&m->h_audio, arow * (size_t)capacity, hipHostMallocDefault));
  kp.status = reinterpret_cast<MpxStatusK*>(m->d_out);                      // (pcm: per launch, behind the chunk's status records)
  HIPOK(hipDeviceSynchronize());
  guard.m = nullptr;
  *out = m;
  return 0;
}

int chz_mpx_capacity(const chz_mpx* m) { return m ? m->cap : -1; }

int chz_mpx_geometry(const chz_mpx* m, int out7[7]) {
  if (!m || !out7) return fail(-1, "bad argument");
  out7[0] = m->L; out7[1] = m->M; out7[2] = m->N; out7[3] = m->olen; out7[4] = m->P; out7[5] = m->pilot_shift; out7[6] = m->subc_shift;
  return 0;
}

// one instance = one session's decoder, history and states zero and the parameters stereod's own, as a fresh decode() thread; returns its index
int chz_mpx_add(chz_mpx* m) {
  if (!m) return fail(-1, "null pool");
  std::lock_guard<std::mutex> lk(m->mu);
  HIPOK(hipSetDevice(m->device));
  if (m->free_inst.empty()) { const int r = mpx_grow(m, 2 * m->ninst); if (r) return r; }
  const int i = m->free_inst.back();
  const MpxState fresh = mpx_fresh_state();
  HIPOK(hipMemcpyAsync(m->state + i, &fresh, sizeof fresh, hipMemcpyHostToDevice, m->s));
  HIPOK(hipMemsetAsync(m->hist + (size_t)i * m->L, 0, sizeof(float) * (size_t)m->L, m->s));
  HIPOK(hipStreamSynchronize(m->s));
  m->free_inst.pop_back();
  m->used[(size_t)i] = 1;
  return i;
}
int chz_mpx_release(chz_mpx* m, int inst) {
  if (!m) return fail(-1, "null pool");
  std::lock_guard<std::mutex> lk(m->mu);
  if (inst < 0 || inst >= m->ninst) return fail(-1, "bad instance");
  if (!m->used[(size_t)inst]) return fail(-1, "instance %d is not in use", inst);
  m->used[(size_t)inst] = 0;
  m->free_inst.push_back(inst);
  return 0;
}
// Deemph_rate and Deemph_gain of one instance; they take effect with the next chz_mpx_execute, the states carry over
int chz_mpx_set_params(chz_mpx* m, int inst, const chz_mpx_params* p) {
  if (!m || !p) return fail(-1, "bad argument");
  if (!std::isfinite(p->deemph_rate) || !std::isfinite(p->deemph_gain) || p->deemph_rate < 0 || !(p->deemph_rate < 1))
    return fail(-1, "de-emphasis rate %g (0 <= rate < 1) or gain %g is out of range", p->deemph_rate, p->deemph_gain);
  std::lock_guard<std::mutex> lk(m->mu);
  if (inst < 0 || inst >= m->ninst) return fail(-1, "bad instance");
  if (!m->used[(size_t)inst]) return fail(-1, "instance %d is not in use", inst);
  HIPOK(hipSetDevice(m->device));
  HIPOK(hipMemcpyAsync(&m->state[inst].rate, p, sizeof *p, hipMemcpyHostToDevice, m->s));
  HIPOK(hipStreamSynchronize(m->s));
  return 0;
}
// response of one slave of one instance (STEREO: 0 mono, 1 pilot, 2 L-R; RDS: 0 pilot, 1 rds): P complex values as set_filter leaves
// them (src/filter.c:968-1045; a REAL slave's P/2 + 1 bins come first, the rest is not read)
int chz_mpx_set_response(chz_mpx* m, int inst, int slave, const float* resp) {
  if (!m || !resp) return fail(-1, "bad argument");
  if (slave < 0 || slave >= m->nslaves) return fail(-1, "bad slave index %d: this pool's instances have %d slaves", slave, m->nslaves);
  std::lock_guard<std::mutex> lk(m->mu);
  if (inst < 0 || inst >= m->ninst) return fail(-1, "bad instance");
  if (!m->used[(size_t)inst]) return fail(-1, "instance %d is not in use", inst);
  HIPOK(hipSetDevice(m->device));
  const size_t P = (size_t)m->P;
  HIPOK(hipMemcpyAsync(m->resp + ((size_t)inst * m->nslaves + (size_t)slave) * P, resp, sizeof(float2) * P, hipMemcpyHostToDevice, m->s));
  HIPOK(hipStreamSynchronize(m->s));
  return 0;
}
// Run one block of n decoders, ONE launch per chunk of `capacity`.  Request i: instance inst[i] takes the L 16-bit samples at samples[i]
// (the pool's byte order) -- on the host (samples_on_device = 0: staged with the request records) or on the device (1: read in place; the
// caller has made them complete) --; pcm[i] receives the block's 4 olen bytes, status[i] its record and audio[i], where audio and audio[i]
// are not NULL, the 2 olen floats the packer was fed.  The state is a recurrence: an instance may appear once in a call.  Every request is
// checked before the first launch: a refused call has written nothing and advanced no state.  Synchronous; thread-safe (callers are
// serialised).
int chz_mpx_execute(chz_mpx* m, int n, const int* inst, const void* const* samples, int samples_on_device, void* const* pcm, float* const* audio,
                    chz_mpx_status* status) {
  if (!m || n < 0 || (n > 0 && (!inst || !samples || !pcm || !status))) return fail(-1, "bad argument");
  if (n == 0) return 0;
  std::lock_guard<std::mutex> lk(m->mu);
  HIPOK(hipSetDevice(m->device));
  std::fill(m->seen.begin(), m->seen.end(), 0);
  for (int r = 0; r < n; r++) {
    if (inst[r] < 0 || inst[r] >= m->ninst || !samples[r] || !pcm[r]) return fail(-1, "bad request %d", r);
    if (!m->used[(size_t)inst[r]]) return fail(-1, "request %d: instance %d is not in use", r, inst[r]);
    if (m->seen[(size_t)inst[r]]) return fail(-1, "request %d: instance %d is listed twice (its state is a recurrence over blocks)", r, inst[r]);
    m->seen[(size_t)inst[r]] = 1;
    if (samples_on_device && (reinterpret_cast<uintptr_t>(samples[r]) & 1)) return fail(-1, "request %d: 16-bit samples on the device at an odd address", r);
  }
  const size_t L = (size_t)m->L, row = 4 * (size_t)m->olen, arow = 2 * (size_t)m->olen;
  for (int done = 0; done < n; done += m->cap) {
    const int k = n - done < m->cap ? n - done : m->cap;
    MpxReq* const h_req = reinterpret_cast<MpxReq*>(m->h_stage);
    unsigned short* const h_s = reinterpret_cast<unsigned short*>(m->h_stage + sizeof(MpxReq) * (size_t)k);
    const unsigned short* const d_s = reinterpret_cast<const unsigned short*>(m->d_stage + sizeof(MpxReq) * (size_t)k);
    bool want = false;
    for (int i = 0; i < k; i++) {
      const int r = done + i;
      if (!samples_on_device) memcpy(h_s + (size_t)i * L, samples[r], sizeof(short) * L);
      h_req[i] = MpxReq{samples_on_device ? reinterpret_cast<const unsigned short*>(samples[r]) : d_s + (size_t)i * L, inst[r], 0};
      want = want || (audio && audio[r]);
    }
    HIPOK(hipMemcpyAsync(m->d_stage, m->h_stage, sizeof(MpxReq) * (size_t)k + (samples_on_device ? 0 : sizeof(short) * L * (size_t)k), hipMemcpyHostToDevice, m->s));
    MpxParams kp = m->kp;
    kp.req = reinterpret_cast<const MpxReq*>(m->d_stage);
    const size_t st_bytes = sizeof(MpxStatusK) * (size_t)k;
    kp.pcm = m->d_out + st_bytes;
    kp.audio = want ? m->d_audio : nullptr;
    hipLaunchKernelGGL(mpx_ovs, dim3(k), dim3(m->threads), m->lds, m->s, kp);
    HIPOK(hipGetLastError());
    HIPOK(hipMemcpyAsync(m->h_out, m->d_out, st_bytes + row * (size_t)k, hipMemcpyDeviceToHost, m->s));       // the k status records and the k rows behind them
    if (want) HIPOK(hipMemcpyAsync(m->h_audio, m->d_audio, sizeof(float) * arow * (size_t)k, hipMemcpyDeviceToHost, m->s));
    HIPOK(hipStreamSynchronize(m->s));
    for (int i = 0; i < k; i++) {
      const int r = done + i;
      memcpy(&status[r], m->h_out + sizeof(MpxStatusK) * (size_t)i, sizeof(chz_mpx_status));
      memcpy(pcm[r], m->h_out + st_bytes + row * (size_t)i, row);
      if (audio && audio[r]) memcpy(audio[r], m->h_audio + arow * (size_t)i, sizeof(float) * arow);
    }
  }
  return 0;
}

}  // extern "C"
