// chz_wfm.inc -- pools of stereo broadcast-FM decoders (part of chz_engine.hip's translation unit).
//
// demod_wfm() (src/wfm.c) keeps, per channel, a discriminator, a REAL composite master of L = 384 kHz x blocktime samples with three
// decimating slaves (mono, the 19 kHz pilot, L-R around 38 kHz) and a stereo decoder with de-emphasis.  A pool holds the responses
// and the state of all instances of one block time; ONE launch of wfm_ovs (chz_kernels.h) serves every instance that is due, one
// workgroup per request, from the channel's baseband to its packed PCM.  Unlike chz_rmini_* the decoder is a recurrence over blocks:
// phase_memory, the squelch sequencer, the smoothed statistics, the de-emphasis filters and the composite filter's history live on
// the device, per instance.  `capacity` is the number of requests one launch serves (the staging buffers' size); the instances'
// storage starts at as many and doubles when chz_wfm_add finds it full.
struct chz_wfm {
  int L = 0, N = 0, olen = 0, P = 0, pilot_shift = 0, subc_shift = 0, cap = 0, ninst = 0, device = 0;
  double blocktime = 0;
  WfmParams kp{};                                  // everything that does not change from launch to launch
  size_t lds = 0; int threads = 0, pcm_stride = 0;   // pcm_stride: the largest PCM row (stereo F32), what the output staging is sized by
  hipStream_t s = nullptr;
  float2* resp = nullptr;        // [ninst][3][P]
  float2* tw = nullptr;          // forward [N/2], split [N/2 + 1], slaves [P]
  WfmState* state = nullptr;     // [ninst]
  float* hist = nullptr;         // [ninst][L]
  // staging for one chunk of k <= cap requests, device and pinned: the k request records, then the baseband of those that bring it from
  // the host (ONE copy carries both); back: the k status records, then the k PCM rows packed at the size their instance can fill (ONE copy)
  unsigned char *d_stage = nullptr, *h_stage = nullptr, *d_out = nullptr, *h_out = nullptr;
  std::vector<chz_wfm_params> par;
  std::vector<int> free_inst;
  std::vector<unsigned char> used, seen;
  std::mutex mu;
};
static_assert(sizeof(WfmStatusK) == sizeof(chz_wfm_status), "wfm_ovs writes chz_wfm_status records");
static_assert(sizeof(WfmReq) % 8 == 0, "the baseband follows the request records and is read as float2");

// storage for n instances (n > m->ninst): new arrays, the old contents copied over, the new instances' state and history zero
static int wfm_grow(chz_wfm* m, int n) {
  float2* resp = nullptr; WfmState* state = nullptr; float* hist = nullptr;
  const size_t P3 = (size_t)3 * m->P, L = (size_t)m->L, old = (size_t)m->ninst;
  struct Guard { float2*& r; WfmState*& s; float*& h; ~Guard() { hipFree(r); hipFree(s); hipFree(h); } } guard{resp, state, hist};
  HIPOK(hipMalloc((void**)&resp, sizeof(float2) * P3 * n));
  HIPOK(hipMalloc((void**)&state, sizeof(WfmState) * (size_t)n));
  HIPOK(hipMalloc((void**)&hist, sizeof(float) * L * n));
  HIPOK(hipMemsetAsync(resp, 0, sizeof(float2) * P3 * n, m->s));
  HIPOK(hipMemsetAsync(state, 0, sizeof(WfmState) * (size_t)n, m->s));
  HIPOK(hipMemsetAsync(hist, 0, sizeof(float) * L * n, m->s));
  if (old) {
    HIPOK(hipMemcpyAsync(resp, m->resp, sizeof(float2) * P3 * old, hipMemcpyDeviceToDevice, m->s));
    HIPOK(hipMemcpyAsync(state, m->state, sizeof(WfmState) * old, hipMemcpyDeviceToDevice, m->s));
    HIPOK(hipMemcpyAsync(hist, m->hist, sizeof(float) * L * old, hipMemcpyDeviceToDevice, m->s));
  }
  HIPOK(hipStreamSynchronize(m->s));
  std::swap(resp, m->resp); std::swap(state, m->state); std::swap(hist, m->hist);      // (the guard frees the old arrays)
  m->kp.state = m->state; m->kp.hist = m->hist;
  for (int s = 0; s < 3; s++) m->kp.s[s].m.resp = m->resp + (size_t)s * m->P;            // row 3 inst of slave s: instance inst
  m->used.resize((size_t)n, 0); m->seen.resize((size_t)n, 0); m->par.resize((size_t)n, chz_wfm_params{});
  for (int i = n - 1; i >= m->ninst; i--) m->free_inst.push_back(i);
  m->ninst = n;
  return 0;
}

extern "C" {

void chz_wfm_destroy(chz_wfm* m) {
  if (!m) return;
  hipSetDevice(m->device);
  if (m->s) hipStreamSynchronize(m->s);
  hipFree(m->resp); hipFree(m->tw); hipFree(m->state); hipFree(m->hist); hipFree(m->d_stage); hipFree(m->d_out);
  if (m->h_stage) (void)hipHostFree(m->h_stage);
  if (m->h_out) (void)hipHostFree(m->h_out);
  if (m->s) hipStreamDestroy(m->s);
  delete m;
}

// would chz_wfm_create take this block time?  0, or < 0 with the reason in chz_last_error(); touches no device
int chz_wfm_check(double blocktime) {
  char why[240];
  const int rc = wfm_check_geom(blocktime, nullptr, why, sizeof why);
  return rc ? fail(rc, "%s", why) : 0;
}

int chz_wfm_create(chz_wfm** out, double blocktime, int capacity, int device) {
  if (!out) return fail(-1, "null out pointer");
  *out = nullptr;
  if (capacity < 1) return fail(-1, "bad WFM decoder pool capacity");
  int g[6] = {};
  { char why[240]; const int rc = wfm_check_geom(blocktime, g, why, sizeof why); if (rc) return fail(rc, "%s", why); }
  chz_wfm* m = new chz_wfm();
  struct Guard { chz_wfm* m; ~Guard() { if (m) chz_wfm_destroy(m); } } guard{m};
  const int L = g[0], N = g[1], olen = g[2], P = g[3], H = N / 2, bins = H + 1;
  m->L = L; m->N = N; m->olen = olen; m->P = P; m->pilot_shift = g[4]; m->subc_shift = g[5]; m->cap = capacity; m->device = device;
  m->blocktime = blocktime;
  m->pcm_stride = olen * 2 * (int)sizeof(float);                           // the largest frame: stereo F32
  WfmParams& kp = m->kp;
  kp.N = N; kp.olen = olen; kp.fwd.N = H;
  kp.alpha = -expm1(-blocktime * 1.0);                                     // src/wfm.c:103: 1 s time constant
  kp.deemph_lanes = options().wfm_deemph_lanes;
  mini_factor(H, kp.fwd.radix, &kp.fwd.nstages);
  const int shifts[3] = {0, m->pilot_shift, m->subc_shift};
  for (int s = 0; s < 3; s++) {
    RminiSlave& sl = kp.s[s];
    sl.m.N = P; sl.m.olen = olen;
    mini_factor(P, sl.m.radix, &sl.m.nstages);
    sl.real_out = s == 0; sl.out_off = 0;
    const ChanDescH h = make_chan_desc(CHZ_REAL, bins, P, shifts[s]);
    kp.d[s] = ChanDesc{h.t0, h.cnt, h.src0, h.dir, h.conj, h.wrap, 0, shifts[s]};
  }
  wfm_launch_geom(N, P, olen, &kp.out_off, &kp.red_off, &m->lds, &m->threads);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(-2, "no HIP device: there is no CPU fallback");
  if (device < 0 || device >= ndev) return fail(-2, "device %d out of range (%d devices)", device, ndev);
  HIPOK(hipSetDevice(device));
  if (m->lds > 64 * 1024 && big_lds_prepare(reinterpret_cast<const void*>(wfm_ovs)))
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
  for (int s = 0; s < 3; s++) kp.s[s].m.tw = m->tw + (size_t)H + (size_t)H + 1;
  r = wfm_grow(m, capacity);
  if (r) return r;
  const size_t stage = (sizeof(WfmReq) + sizeof(float2) * (size_t)L) * (size_t)capacity;
  const size_t outb = ((size_t)m->pcm_stride + sizeof(WfmStatusK)) * (size_t)capacity;
  HIPOK(hipMalloc((void**)&m->d_stage, stage));
  HIPOK(hipMalloc((void**)&m->d_out, outb));
  HIPOK(hipHostMalloc((void**)&m->h_stage, stage, hipHostMallocDefault));
  HIPOK(hipHostMalloc((void**)&m->h_out, outb, hipHostMallocDefault));
  kp.status = reinterpret_cast<WfmStatusK*>(m->d_out);                      // (pcm: per launch, behind the chunk's status records)
  HIPOK(hipDeviceSynchronize());
  guard.m = nullptr;
  *out = m;
  return 0;
}

int chz_wfm_capacity(const chz_wfm* m) { return m ? m->cap : -1; }

int chz_wfm_geometry(const chz_wfm* m, int out6[6]) {
  if (!m || !out6) return fail(-1, "bad argument");
  out6[0] = m->L; out6[1] = m->N; out6[2] = m->olen; out6[3] = m->P; out6[4] = m->pilot_shift; out6[5] = m->subc_shift;
  return 0;
}

// one instance = one channel's decoder, its state and history zero; returns its index
int chz_wfm_add(chz_wfm* m) {
  if (!m) return fail(-1, "null pool");
  std::lock_guard<std::mutex> lk(m->mu);
  HIPOK(hipSetDevice(m->device));
  if (m->free_inst.empty()) { const int r = wfm_grow(m, 2 * m->ninst); if (r) return r; }
  const int i = m->free_inst.back();
  HIPOK(hipMemsetAsync(m->state + i, 0, sizeof(WfmState), m->s));
  HIPOK(hipMemsetAsync(m->hist + (size_t)i * m->L, 0, sizeof(float) * (size_t)m->L, m->s));
  HIPOK(hipStreamSynchronize(m->s));
  m->free_inst.pop_back();
  m->used[(size_t)i] = 1;
  m->par[(size_t)i] = chz_wfm_params{};
  return i;
}
int chz_wfm_release(chz_wfm* m, int inst) {
  if (!m) return fail(-1, "null pool");
  std::lock_guard<std::mutex> lk(m->mu);
  if (inst < 0 || inst >= m->ninst) return fail(-1, "bad instance");
  if (!m->used[(size_t)inst]) return fail(-1, "instance %d is not in use", inst);
  m->used[(size_t)inst] = 0;
  m->free_inst.push_back(inst);
  return 0;
}
// the chan_t members demod_wfm() reads every block; they take effect with the next chz_wfm_execute
int chz_wfm_set_params(chz_wfm* m, int inst, const chz_wfm_params* p) {
  if (!m || !p) return fail(-1, "bad argument");
  if (p->encoding < CHZ_PCM_S16BE_K || p->encoding > CHZ_PCM_F16BE_K) return fail(-1, "encoding %d is not one of CHZ_PCM_*", p->encoding);
  if (!(fabs(p->bandwidth) > 0)) return fail(-1, "bandwidth must not be zero");
  std::lock_guard<std::mutex> lk(m->mu);
  if (inst < 0 || inst >= m->ninst) return fail(-1, "bad instance");
  if (!m->used[(size_t)inst]) return fail(-1, "instance %d is not in use", inst);
  m->par[(size_t)inst] = *p;
  return 0;
}
// response of one slave of one instance (0 mono, 1 pilot, 2 L-R): P complex values as set_filter leaves them (src/filter.c:968-1045;
// the REAL mono slave's P/2 + 1 bins come first, the rest is not read)
int chz_wfm_set_response(chz_wfm* m, int inst, int slave, const float* resp) {
  if (!m || !resp || slave < 0 || slave >= 3) return fail(-1, "bad argument");
  std::lock_guard<std::mutex> lk(m->mu);
  if (inst < 0 || inst >= m->ninst) return fail(-1, "bad instance");
  if (!m->used[(size_t)inst]) return fail(-1, "instance %d is not in use", inst);
  HIPOK(hipSetDevice(m->device));
  const size_t P = (size_t)m->P;
  HIPOK(hipMemcpyAsync(m->resp + ((size_t)inst * 3 + (size_t)slave) * P, resp, sizeof(float2) * P, hipMemcpyHostToDevice, m->s));
  HIPOK(hipStreamSynchronize(m->s));
  return 0;
}
// Run one block of n decoders, ONE launch per chunk of `capacity`.  Request i: instance inst[i] takes the L complex baseband samples
// at bb[i] -- on the host (bb_on_device = 0: staged with the request records) or on the device (1: read in place; the caller has
// made them complete, e.g. a row of chz_bank_output_device() after chz_slot_sync) --, the channel's bb_power[i] and noise density
// n0[i]; pcm[i] receives olen * status[i].channels samples of the instance's encoding and stays untouched on a "no samples" block
// (status[i].frame = 1).  The state is a recurrence: an instance may appear once in a call.  Every request is checked before the
// first launch: a refused call has written nothing and advanced no state.  Synchronous; thread-safe (callers are serialised).
int chz_wfm_execute(chz_wfm* m, int n, const int* inst, const float* const* bb, int bb_on_device, const double* bb_power, const double* n0,
                    void* const* pcm, chz_wfm_status* status) {
  if (!m || n < 0 || (n > 0 && (!inst || !bb || !bb_power || !n0 || !pcm || !status))) return fail(-1, "bad argument");
  if (n == 0) return 0;
  std::lock_guard<std::mutex> lk(m->mu);
  HIPOK(hipSetDevice(m->device));
  std::fill(m->seen.begin(), m->seen.end(), 0);
  for (int r = 0; r < n; r++) {
    if (inst[r] < 0 || inst[r] >= m->ninst || !bb[r] || !pcm[r]) return fail(-1, "bad request %d", r);
    if (!m->used[(size_t)inst[r]]) return fail(-1, "request %d: instance %d is not in use", r, inst[r]);
    if (m->seen[(size_t)inst[r]]) return fail(-1, "request %d: instance %d is listed twice (its state is a recurrence over blocks)", r, inst[r]);
    m->seen[(size_t)inst[r]] = 1;
    if (!(fabs(m->par[(size_t)inst[r]].bandwidth) > 0)) return fail(-1, "request %d: instance %d has no parameters yet", r, inst[r]);
  }
  const size_t L = (size_t)m->L;
  for (int done = 0; done < n; done += m->cap) {
    const int k = n - done < m->cap ? n - done : m->cap;
    WfmReq* const h_req = reinterpret_cast<WfmReq*>(m->h_stage);
    float2* const h_bb = reinterpret_cast<float2*>(m->h_stage + sizeof(WfmReq) * (size_t)k);
    const float2* const d_bb = reinterpret_cast<const float2*>(m->d_stage + sizeof(WfmReq) * (size_t)k);
    const auto sample_bytes = [](int enc) -> size_t {
      return (enc == CHZ_PCM_MULAW_K || enc == CHZ_PCM_ALAW_K) ? 1 : (enc == CHZ_PCM_F32LE_K || enc == CHZ_PCM_F32BE_K) ? 4 : 2;
    };
    size_t rows = 0;                                                       // the chunk's PCM rows, each as large as its instance can fill
    for (int i = 0; i < k; i++) {
      const int r = done + i;
      const chz_wfm_params& p = m->par[(size_t)inst[r]];
      if (!bb_on_device) memcpy(h_bb + (size_t)i * L, bb[r], sizeof(float2) * L);
      h_req[i] = WfmReq{bb_on_device ? reinterpret_cast<const float2*>(bb[r]) : d_bb + (size_t)i * L, bb_power[r], n0[r],
                        p.squelch_open, p.squelch_close, p.bandwidth, p.headroom, p.deemph_rate, p.deemph_gain,
                        inst[r], p.stereo_enable != 0, p.encoding, p.squelch_tail, (int)rows, 0};
      rows += (sample_bytes(p.encoding) * (size_t)m->olen * (p.stereo_enable ? 2 : 1) + 3) / 4 * 4;
    }
    HIPOK(hipMemcpyAsync(m->d_stage, m->h_stage, sizeof(WfmReq) * (size_t)k + (bb_on_device ? 0 : sizeof(float2) * L * (size_t)k), hipMemcpyHostToDevice, m->s));
    WfmParams kp = m->kp;
    kp.req = reinterpret_cast<const WfmReq*>(m->d_stage);
    const size_t st_bytes = sizeof(WfmStatusK) * (size_t)k;
    kp.pcm = m->d_out + st_bytes;
    hipLaunchKernelGGL(wfm_ovs, dim3(k), dim3(m->threads), m->lds, m->s, kp);
    HIPOK(hipGetLastError());
    HIPOK(hipMemcpyAsync(m->h_out, m->d_out, st_bytes + rows, hipMemcpyDeviceToHost, m->s));      // the k status records and the k rows behind them
    HIPOK(hipStreamSynchronize(m->s));
    for (int i = 0; i < k; i++) {
      const int r = done + i;
      memcpy(&status[r], m->h_out + sizeof(WfmStatusK) * (size_t)i, sizeof(chz_wfm_status));
      if (status[r].frame != 0) continue;
      memcpy(pcm[r], m->h_out + st_bytes + (size_t)h_req[i].pcm_off, sample_bytes(h_req[i].encoding) * (size_t)m->olen * (size_t)status[r].channels);
    }
  }
  return 0;
}

}  // extern "C"
