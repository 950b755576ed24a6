// chz_ctcss.inc -- pools of CTCSS / PL tone decoders (part of chz_engine.hip's translation unit).
//
// ctcss (src/ctcss.c:268-309, process_pl() :392-419) keeps, per session, a REAL master of L = 0.2 s of audio, M = L + 1 with one COMPLEX
// slave of 100 samples (50 .. 300 Hz spun down by 150 Hz to 500 Hz), and behind it one correlator per tone of its table; every 200 ms it
// names the strongest tone above a fixed threshold.  A pool holds the responses and the state of all sessions of one geometry -- (samprate,
// input byte order, tone table) --; ONE launch of ctcss_ovs (chz_kernels.h) serves every session that is due, one workgroup per request,
// from the samples to the decision.  The decoder is a recurrence over blocks: the filter's history, the oscillators' phasors with their
// step counts and the sticky current tone live on the device, per instance.  What crosses the link is 2 L bytes and a request record
// down and a 16-byte status record up, plus the ntones energies of the requests that ask for them.  `capacity` is the number of requests
// one launch serves; the instances' storage starts at as many and doubles when chz_ctcss_add finds it full.
struct chz_ctcss {
  int L = 0, M = 0, N = 0, olen = 0, P = 0, shift = 0, ntones = 0, big_endian = 0, cap = 0, ninst = 0, device = 0;
  double samprate = 0;
  CtcssParams kp{};                                // everything that does not change from launch to launch
  size_t lds = 0; int threads = 0;
  hipStream_t s = nullptr;
  float2* resp = nullptr;        // [ninst][P]
  float2* tw = nullptr;          // forward [N/2], split [N/2 + 1], slave [P]
  double* tone_step = nullptr;   // [ntones][2]
  CtcssState* state = nullptr;   // [ninst]
  float* hist = nullptr;         // [ninst][M - 1]
  // staging for one chunk of k <= cap requests, device and pinned: the k request records, then the samples of those that bring them from
  // the host (ONE copy carries both); back: the k status records (ONE copy), and the k rows of energies when a request of the chunk wants its own
  unsigned char *d_stage = nullptr, *h_stage = nullptr, *d_out = nullptr, *h_out = nullptr;
  double *d_energies = nullptr, *h_energies = nullptr;
  std::vector<int> free_inst;
  std::vector<unsigned char> used, seen;
  std::mutex mu;
};
static_assert(sizeof(CtcssStatusK) == sizeof(chz_ctcss_status), "ctcss_ovs writes chz_ctcss_status records");
static_assert(CHZ_CTCSS_MAX_TONES == CHZ_CTCSS_TONES_MAX && CHZ_CTCSS_MAX_TONES == CHZ_CTCSS_TABLE_MAX, "the header and the checker state the kernel's limit");

// the table a pool searches when the caller brings none: the 55 standard sub-audible tones in ascending order, 150.0 Hz among them, as
// src/ctcss.c:62-69 lists them (tones == NULL: ntones is not looked at)
static const double ctcss_pl_tones[CHZ_CTCSS_STANDARD_TONES] = {
   67.0,  69.3,  71.9,  74.4,  77.0,  79.7,  82.5,  85.4,  88.5,  91.5,  94.8,  97.4, 100.0, 103.5, 107.2, 110.9, 114.8, 118.8, 123.0,
  127.3, 131.8, 136.5, 141.3, 146.2, 150.0, 151.4, 156.7, 159.8, 162.2, 165.5, 167.9, 171.3, 173.8, 177.3, 179.9, 183.5, 186.2, 189.9,
  192.8, 196.6, 199.5, 203.5, 206.5, 210.7, 213.8, 218.1, 221.3, 225.7, 229.1, 233.6, 237.1, 241.8, 245.5, 250.3, 254.1};

// storage for n instances (n > m->ninst): new arrays, the old contents copied over, the new instances' state and history zero
static int ctcss_grow(chz_ctcss* m, int n) {
  float2* resp = nullptr; CtcssState* state = nullptr; float* hist = nullptr;
  const size_t P = (size_t)m->P, Hs = (size_t)(m->M - 1), old = (size_t)m->ninst;
  struct Guard { float2*& r; CtcssState*& s; float*& h; ~Guard() { hipFree(r); hipFree(s); hipFree(h); } } guard{resp, state, hist};
  HIPOK(hipMalloc((void**)&resp, sizeof(float2) * P * n));
  HIPOK(hipMalloc((void**)&state, sizeof(CtcssState) * (size_t)n));
  HIPOK(hipMalloc((void**)&hist, sizeof(float) * Hs * n));
  HIPOK(hipMemsetAsync(resp, 0, sizeof(float2) * P * n, m->s));
  HIPOK(hipMemsetAsync(state, 0, sizeof(CtcssState) * (size_t)n, m->s));
  HIPOK(hipMemsetAsync(hist, 0, sizeof(float) * Hs * n, m->s));
  if (old) {
    HIPOK(hipMemcpyAsync(resp, m->resp, sizeof(float2) * P * old, hipMemcpyDeviceToDevice, m->s));
    HIPOK(hipMemcpyAsync(state, m->state, sizeof(CtcssState) * old, hipMemcpyDeviceToDevice, m->s));
    HIPOK(hipMemcpyAsync(hist, m->hist, sizeof(float) * Hs * old, hipMemcpyDeviceToDevice, m->s));
  }
  HIPOK(hipStreamSynchronize(m->s));
  std::swap(resp, m->resp); std::swap(state, m->state); std::swap(hist, m->hist);      // (the guard frees the old arrays)
  m->kp.state = m->state; m->kp.hist = m->hist; m->kp.sl.m.resp = m->resp;
  m->used.resize((size_t)n, 0); m->seen.resize((size_t)n, 0);
  for (int i = n - 1; i >= m->ninst; i--) m->free_inst.push_back(i);
  m->ninst = n;
  return 0;
}

extern "C" {

void chz_ctcss_destroy(chz_ctcss* m) {
  if (!m) return;
  hipSetDevice(m->device);
  if (m->s) hipStreamSynchronize(m->s);
  hipFree(m->resp); hipFree(m->tw); hipFree(m->tone_step); hipFree(m->state); hipFree(m->hist); hipFree(m->d_stage); hipFree(m->d_out); hipFree(m->d_energies);
  if (m->h_stage) (void)hipHostFree(m->h_stage);
  if (m->h_out) (void)hipHostFree(m->h_out);
  if (m->h_energies) (void)hipHostFree(m->h_energies);
  if (m->s) hipStreamDestroy(m->s);
  delete m;
}

// would chz_ctcss_create take this?  0, or < 0 with the reason in chz_last_error(); touches no device
int chz_ctcss_check(double samprate, int byte_order, int ntones, const double* tones) {
  char why[240];
  if (byte_order != CHZ_CTCSS_BE && byte_order != CHZ_CTCSS_LE) return fail(-1, "byte order %d is neither CHZ_CTCSS_BE nor CHZ_CTCSS_LE", byte_order);
  if (!tones) { tones = ctcss_pl_tones; ntones = CHZ_CTCSS_STANDARD_TONES; }
  const int rc = ctcss_check_geom(samprate, ntones, tones, nullptr, why, sizeof why);
  return rc ? fail(rc, "%s", why) : 0;
}

int chz_ctcss_create(chz_ctcss** out, double samprate, int byte_order, int ntones, const double* tones, int capacity, int device) {
  if (!out) return fail(-1, "null out pointer");
  *out = nullptr;
  if (capacity < 1) return fail(-1, "bad CTCSS decoder pool capacity");
  if (byte_order != CHZ_CTCSS_BE && byte_order != CHZ_CTCSS_LE) return fail(-1, "byte order %d is neither CHZ_CTCSS_BE nor CHZ_CTCSS_LE", byte_order);
  if (!tones) { tones = ctcss_pl_tones; ntones = CHZ_CTCSS_STANDARD_TONES; }
  int g[7] = {};
  { char why[240]; const int rc = ctcss_check_geom(samprate, ntones, tones, g, why, sizeof why); if (rc) return fail(rc, "%s", why); }
  chz_ctcss* m = new chz_ctcss();
  struct Guard { chz_ctcss* m; ~Guard() { if (m) chz_ctcss_destroy(m); } } guard{m};
  const int L = g[0], N = g[2], olen = g[3], P = g[4], H = N / 2, bins = H + 1;
  m->L = L; m->M = g[1]; m->N = N; m->olen = olen; m->P = P; m->shift = g[5]; m->ntones = ntones;
  m->big_endian = byte_order == CHZ_CTCSS_BE; m->cap = capacity; m->device = device; m->samprate = samprate;
  CtcssParams& kp = m->kp;
  kp.N = N; kp.L = L; kp.ntones = ntones; kp.big_endian = m->big_endian; kp.fwd.N = H;
  kp.threshold = 0.005 * olen;                                             // pl_blocksize = lrint(PL_samprate / PL_blockrate) = olen (:272,404)
  // set_osc(&pl_osc[n], (PL_tones[n] - PL_Shift) / PL_samprate, 0): phasor_step = cispi(2 f), and 1 where f equals the zeroed freq (:276;
  // src/osc.c:37-39) -- cos / sin of 2 pi f as chz_afsk.inc has them, which are exactly 1 and 0 there too
  std::vector<double> step(2 * (size_t)ntones);
  for (int t = 0; t < ntones; t++) {
    const double f = (tones[t] - CHZ_CTCSS_PL_SHIFT) / CHZ_CTCSS_PL_SAMPRATE;
    step[2 * (size_t)t] = cos(2 * M_PI * f); step[2 * (size_t)t + 1] = sin(2 * M_PI * f);
    if (tones[t] > 0) kp.positive |= 1ull << t;
  }
  mini_factor(H, kp.fwd.radix, &kp.fwd.nstages);
  RminiSlave& sl = kp.sl;
  sl.m.N = P; sl.m.olen = olen;
  mini_factor(P, sl.m.radix, &sl.m.nstages);
  sl.real_out = 0; sl.out_off = 0;
  const ChanDescH h = make_chan_desc(CHZ_REAL, bins, P, m->shift);
  kp.d = ChanDesc{h.t0, h.cnt, h.src0, h.dir, h.conj, h.wrap, 0, m->shift};
  rmini_launch_geom(N, P, &m->lds, &m->threads);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(-2, "no HIP device: there is no CPU fallback");
  if (device < 0 || device >= ndev) return fail(-2, "device %d out of range (%d devices)", device, ndev);
  HIPOK(hipSetDevice(device));
  if (m->lds > 64 * 1024 && big_lds_prepare(reinterpret_cast<const void*>(ctcss_ovs)))
    return fail(-3, "the runtime refuses %zu bytes of LDS per workgroup (N=%d)", m->lds, N);
  HIPOK(hipStreamCreateWithFlags(&m->s, hipStreamNonBlocking));
  std::vector<f2> tw((size_t)H + (size_t)H + 1 + (size_t)P);
  size_t at = 0;
  for (int k = 0; k < H; k++) tw[at++] = root_of_unity(k, H, -1);
  for (int k = 0; k <= H; k++) tw[at++] = root_of_unity(k, N, -1);
  for (int k = 0; k < P; k++) tw[at++] = root_of_unity(k, P, -1);
  int r = upload(&m->tw, tw);
  if (r) return r;
  kp.fwd.tw = m->tw; kp.tw_split = m->tw + H; sl.m.tw = m->tw + (size_t)H + (size_t)H + 1;
  HIPOK(hipMalloc((void**)&m->tone_step, sizeof(double) * step.size()));
  HIPOK(hipMemcpy(m->tone_step, step.data(), sizeof(double) * step.size(), hipMemcpyHostToDevice));
  kp.tone_step = m->tone_step;
  r = ctcss_grow(m, capacity);
  if (r) return r;
  static_assert(sizeof(CtcssReq) % 8 == 0, "the samples follow the request records");
  const size_t stage = (sizeof(CtcssReq) + sizeof(short) * (size_t)L) * (size_t)capacity;
  const size_t erow = sizeof(double) * CHZ_CTCSS_MAX_TONES;
  HIPOK(hipMalloc((void**)&m->d_stage, stage));
  HIPOK(hipMalloc((void**)&m->d_out, sizeof(CtcssStatusK) * (size_t)capacity));
  HIPOK(hipMalloc((void**)&m->d_energies, erow * (size_t)capacity));
  HIPOK(hipHostMalloc((void**)&m->h_stage, stage, hipHostMallocDefault));
  HIPOK(hipHostMalloc((void**)&m->h_out, sizeof(CtcssStatusK) * (size_t)capacity, hipHostMallocDefault));
  HIPOK(hipHostMalloc((void**)&m->h_energies, erow * (size_t)capacity, hipHostMallocDefault));
  kp.status = reinterpret_cast<CtcssStatusK*>(m->d_out); kp.energies = m->d_energies;
  HIPOK(hipDeviceSynchronize());
  guard.m = nullptr;
  *out = m;
  return 0;
}

int chz_ctcss_capacity(const chz_ctcss* m) { return m ? m->cap : -1; }

int chz_ctcss_geometry(const chz_ctcss* m, int out7[7]) {
  if (!m || !out7) return fail(-1, "bad argument");
  out7[0] = m->L; out7[1] = m->M; out7[2] = m->N; out7[3] = m->olen; out7[4] = m->P; out7[5] = m->shift; out7[6] = m->ntones;
  return 0;
}

// one instance = one session's decoder, everything zero as in a fresh session (create_session()'s calloc); returns its index
int chz_ctcss_add(chz_ctcss* m) {
  if (!m) return fail(-1, "null pool");
  std::lock_guard<std::mutex> lk(m->mu);
  HIPOK(hipSetDevice(m->device));
  if (m->free_inst.empty()) { const int r = ctcss_grow(m, 2 * m->ninst); if (r) return r; }
  const int i = m->free_inst.back();
  HIPOK(hipMemsetAsync(m->state + i, 0, sizeof(CtcssState), m->s));
  HIPOK(hipMemsetAsync(m->hist + (size_t)i * (m->M - 1), 0, sizeof(float) * (size_t)(m->M - 1), m->s));
  HIPOK(hipStreamSynchronize(m->s));
  m->free_inst.pop_back();
  m->used[(size_t)i] = 1;
  return i;
}
int chz_ctcss_release(chz_ctcss* m, int inst) {
  if (!m) return fail(-1, "null pool");
  std::lock_guard<std::mutex> lk(m->mu);
  if (inst < 0 || inst >= m->ninst) return fail(-1, "bad instance");
  if (!m->used[(size_t)inst]) return fail(-1, "instance %d is not in use", inst);
  m->used[(size_t)inst] = 0;
  m->free_inst.push_back(inst);
  return 0;
}
// response of an instance's slave: P complex values as set_filter leaves them (src/filter.c:968-1045), as chz_rmini_set_response takes them
int chz_ctcss_set_response(chz_ctcss* m, int inst, const float* resp) {
  if (!m || !resp) return fail(-1, "bad argument");
  std::lock_guard<std::mutex> lk(m->mu);
  if (inst < 0 || inst >= m->ninst) return fail(-1, "bad instance");
  if (!m->used[(size_t)inst]) return fail(-1, "instance %d is not in use", inst);
  HIPOK(hipSetDevice(m->device));
  const size_t P = (size_t)m->P;
  HIPOK(hipMemcpyAsync(m->resp + (size_t)inst * P, resp, sizeof(float2) * P, hipMemcpyHostToDevice, m->s));
  HIPOK(hipStreamSynchronize(m->s));
  return 0;
}
// Run one block of n decoders, ONE launch per chunk of `capacity`.  Request i: instance inst[i] takes the L 16-bit samples at samples[i]
// (the pool's byte order) -- on the host (samples_on_device = 0: staged with the request records) or on the device (1: read in place; the
// caller has made them complete) --; status[i] receives the block's record and energies[i], where energies and energies[i] are not NULL,
// the ntones energies the decision was taken on.  The state is a recurrence: an instance may appear once in a call.  Every request is
// checked before the first launch: a refused call has written nothing and advanced no state.  Synchronous; thread-safe (callers are
// serialised).
int chz_ctcss_execute(chz_ctcss* m, int n, const int* inst, const void* const* samples, int samples_on_device, chz_ctcss_status* status,
                      double* const* energies) {
  if (!m || n < 0 || (n > 0 && (!inst || !samples || !status))) return fail(-1, "bad argument");
  if (n == 0) return 0;
  std::lock_guard<std::mutex> lk(m->mu);
  HIPOK(hipSetDevice(m->device));
  std::fill(m->seen.begin(), m->seen.end(), 0);
  for (int r = 0; r < n; r++) {
    if (inst[r] < 0 || inst[r] >= m->ninst || !samples[r]) return fail(-1, "bad request %d", r);
    if (!m->used[(size_t)inst[r]]) return fail(-1, "request %d: instance %d is not in use", r, inst[r]);
    if (m->seen[(size_t)inst[r]]) return fail(-1, "request %d: instance %d is listed twice (its state is a recurrence over blocks)", r, inst[r]);
    m->seen[(size_t)inst[r]] = 1;
    if (samples_on_device && (reinterpret_cast<uintptr_t>(samples[r]) & 1)) return fail(-1, "request %d: 16-bit samples on the device at an odd address", r);
  }
  const size_t L = (size_t)m->L, nt = (size_t)m->ntones;
  for (int done = 0; done < n; done += m->cap) {
    const int k = n - done < m->cap ? n - done : m->cap;
    CtcssReq* const h_req = reinterpret_cast<CtcssReq*>(m->h_stage);
    unsigned short* const h_s = reinterpret_cast<unsigned short*>(m->h_stage + sizeof(CtcssReq) * (size_t)k);
    const unsigned short* const d_s = reinterpret_cast<const unsigned short*>(m->d_stage + sizeof(CtcssReq) * (size_t)k);
    bool want = false;
    for (int i = 0; i < k; i++) {
      const int r = done + i;
      if (!samples_on_device) memcpy(h_s + (size_t)i * L, samples[r], sizeof(short) * L);
      h_req[i] = CtcssReq{samples_on_device ? reinterpret_cast<const unsigned short*>(samples[r]) : d_s + (size_t)i * L, inst[r], 0};
      want = want || (energies && energies[r]);
    }
    HIPOK(hipMemcpyAsync(m->d_stage, m->h_stage, sizeof(CtcssReq) * (size_t)k + (samples_on_device ? 0 : sizeof(short) * L * (size_t)k), hipMemcpyHostToDevice, m->s));
    CtcssParams kp = m->kp;
    kp.req = reinterpret_cast<const CtcssReq*>(m->d_stage);
    hipLaunchKernelGGL(ctcss_ovs, dim3(k), dim3(m->threads), m->lds, m->s, kp);
    HIPOK(hipGetLastError());
    HIPOK(hipMemcpyAsync(m->h_out, m->d_out, sizeof(CtcssStatusK) * (size_t)k, hipMemcpyDeviceToHost, m->s));
    if (want) HIPOK(hipMemcpyAsync(m->h_energies, m->d_energies, sizeof(double) * CHZ_CTCSS_MAX_TONES * (size_t)k, hipMemcpyDeviceToHost, m->s));
    HIPOK(hipStreamSynchronize(m->s));
    const chz_ctcss_status* st = reinterpret_cast<const chz_ctcss_status*>(m->h_out);
    for (int i = 0; i < k; i++) {
      const int r = done + i;
      status[r] = st[i];
      if (energies && energies[r]) memcpy(energies[r], m->h_energies + (size_t)CHZ_CTCSS_MAX_TONES * (size_t)i, sizeof(double) * nt);
    }
  }
  return 0;
}

}  // extern "C"
