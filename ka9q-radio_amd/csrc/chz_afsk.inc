// chz_afsk.inc -- pools of AFSK / AX.25 packet decoders (part of chz_engine.hip's translation unit).
//
// packetd's decode_task() (src/packetd.c:485-629) keeps, per session, a REAL master of L 960, M 961 with one COMPLEX slave that makes the
// 16-bit audio analytic, correlators on the two tones, a Gardner bit clock, NRZI and HDLC with the frame buffer.  A pool holds the
// responses and the state of all sessions of one geometry -- (L, M, samprate, bitrate, mark, space, input byte order) --; ONE launch of
// afsk_ovs (chz_kernels.h) serves every session that is due, one workgroup per request, from the samples to the frames.  Like the WFM
// pool the decoder is a recurrence over blocks: the filter's history, the oscillators, integrators, clock and the HDLC state with its
// 16 KB frame buffer live on the device, per instance.  What crosses the link is 2 L bytes and a request record down, a status record
// up, and the bytes of the frames that completed.  `capacity` is the number of requests one launch serves; the instances' storage starts
// at as many and doubles when chz_afsk_add finds it full.
struct chz_afsk {
  int L = 0, M = 0, N = 0, samppbit = 0, big_endian = 0, cap = 0, ninst = 0, device = 0;
  double samprate = 0, bitrate = 0, mark = 0, space = 0;
  AfskParams kp{};                                 // everything that does not change from launch to launch
  size_t lds = 0; int threads = 0;
  hipStream_t s = nullptr;
  float2* resp = nullptr;        // [ninst][N]
  float2* tw = nullptr;          // forward [N/2], split [N/2 + 1], slave [N]
  AfskState* state = nullptr;    // [ninst]
  float* hist = nullptr;         // [ninst][M - 1]
  unsigned char* frame = nullptr;   // [ninst][CHZ_AFSK_FRAME_PITCH]
  // staging for one chunk of k <= cap requests, device and pinned: the k request records, then the samples of those that bring them from
  // the host (ONE copy carries both); back: the k status records (ONE copy), then what the completed frames fill of the requests' output areas
  unsigned char *d_stage = nullptr, *h_stage = nullptr, *d_out = nullptr, *h_out = nullptr, *d_frames = nullptr, *h_frames = nullptr;
  std::vector<int> free_inst;
  std::vector<unsigned char> used, seen;
  std::mutex mu;
};
static_assert(sizeof(AfskStatusK) == sizeof(chz_afsk_status), "afsk_ovs writes chz_afsk_status records");
static_assert(CHZ_AFSK_MAX_FRAMES == CHZ_AFSK_STATUS_FRAMES && CHZ_AFSK_FRAME_BYTES == CHZ_AFSK_FRAME_MAX, "the header states the kernel's limits");
static_assert(CHZ_AFSK_MAX_DECISIONS / 32 == CHZ_AFSK_MAX_FRAMES, "a frame and its flag take at least 32 decisions");

// storage for n instances (n > m->ninst): new arrays, the old contents copied over, the new instances' state, history and frame buffer zero
static int afsk_grow(chz_afsk* m, int n) {
  float2* resp = nullptr; AfskState* state = nullptr; float* hist = nullptr; unsigned char* frame = nullptr;
  const size_t N = (size_t)m->N, Hs = (size_t)(m->M - 1), F = CHZ_AFSK_FRAME_PITCH, old = (size_t)m->ninst;
  struct Guard { float2*& r; AfskState*& s; float*& h; unsigned char*& f; ~Guard() { hipFree(r); hipFree(s); hipFree(h); hipFree(f); } } guard{resp, state, hist, frame};
  HIPOK(hipMalloc((void**)&resp, sizeof(float2) * N * n));
  HIPOK(hipMalloc((void**)&state, sizeof(AfskState) * (size_t)n));
  HIPOK(hipMalloc((void**)&hist, sizeof(float) * (Hs ? Hs : 1) * n));
  HIPOK(hipMalloc((void**)&frame, F * n));
  HIPOK(hipMemsetAsync(resp, 0, sizeof(float2) * N * n, m->s));
  HIPOK(hipMemsetAsync(state, 0, sizeof(AfskState) * (size_t)n, m->s));
  HIPOK(hipMemsetAsync(hist, 0, sizeof(float) * (Hs ? Hs : 1) * n, m->s));
  HIPOK(hipMemsetAsync(frame, 0, F * n, m->s));
  if (old) {
    HIPOK(hipMemcpyAsync(resp, m->resp, sizeof(float2) * N * old, hipMemcpyDeviceToDevice, m->s));
    HIPOK(hipMemcpyAsync(state, m->state, sizeof(AfskState) * old, hipMemcpyDeviceToDevice, m->s));
    if (Hs) HIPOK(hipMemcpyAsync(hist, m->hist, sizeof(float) * Hs * old, hipMemcpyDeviceToDevice, m->s));
    HIPOK(hipMemcpyAsync(frame, m->frame, F * old, hipMemcpyDeviceToDevice, m->s));
  }
  HIPOK(hipStreamSynchronize(m->s));
  std::swap(resp, m->resp); std::swap(state, m->state); std::swap(hist, m->hist); std::swap(frame, m->frame);      // (the guard frees the old arrays)
  m->kp.state = m->state; m->kp.hist = m->hist; m->kp.frame = m->frame; m->kp.sl.m.resp = m->resp;
  m->used.resize((size_t)n, 0); m->seen.resize((size_t)n, 0);
  for (int i = n - 1; i >= m->ninst; i--) m->free_inst.push_back(i);
  m->ninst = n;
  return 0;
}

extern "C" {

void chz_afsk_destroy(chz_afsk* m) {
  if (!m) return;
  hipSetDevice(m->device);
  if (m->s) hipStreamSynchronize(m->s);
  hipFree(m->resp); hipFree(m->tw); hipFree(m->state); hipFree(m->hist); hipFree(m->frame); hipFree(m->d_stage); hipFree(m->d_out); hipFree(m->d_frames);
  if (m->h_stage) (void)hipHostFree(m->h_stage);
  if (m->h_out) (void)hipHostFree(m->h_out);
  if (m->h_frames) (void)hipHostFree(m->h_frames);
  if (m->s) hipStreamDestroy(m->s);
  delete m;
}

// would chz_afsk_create take this geometry?  0, or < 0 with the reason in chz_last_error(); touches no device
int chz_afsk_check(int L, int M, double samprate, double bitrate, double mark, double space, int byte_order) {
  char why[240];
  if (byte_order != CHZ_AFSK_BE && byte_order != CHZ_AFSK_LE) return fail(-1, "byte order %d is neither CHZ_AFSK_BE nor CHZ_AFSK_LE", byte_order);
  const int rc = afsk_check_geom(L, M, samprate, bitrate, mark, space, nullptr, why, sizeof why);
  return rc ? fail(rc, "%s", why) : 0;
}

int chz_afsk_create(chz_afsk** out, int L, int M, double samprate, double bitrate, double mark, double space, int byte_order, int capacity, int device) {
  if (!out) return fail(-1, "null out pointer");
  *out = nullptr;
  if (capacity < 1) return fail(-1, "bad AFSK decoder pool capacity");
  if (byte_order != CHZ_AFSK_BE && byte_order != CHZ_AFSK_LE) return fail(-1, "byte order %d is neither CHZ_AFSK_BE nor CHZ_AFSK_LE", byte_order);
  int g[4] = {};
  { char why[240]; const int rc = afsk_check_geom(L, M, samprate, bitrate, mark, space, g, why, sizeof why); if (rc) return fail(rc, "%s", why); }
  chz_afsk* m = new chz_afsk();
  struct Guard { chz_afsk* m; ~Guard() { if (m) chz_afsk_destroy(m); } } guard{m};
  const int N = g[2], H = N / 2, bins = H + 1;
  m->L = L; m->M = M; m->N = N; m->samppbit = g[3]; m->big_endian = byte_order == CHZ_AFSK_BE; m->cap = capacity; m->device = device;
  m->samprate = samprate; m->bitrate = bitrate; m->mark = mark; m->space = space;
  AfskParams& kp = m->kp;
  kp.N = N; kp.L = L; kp.samppbit = g[3]; kp.big_endian = m->big_endian; kp.fwd.N = H;
  kp.twist = mark / space;                                                 // src/packetd.c:486
  // set_osc(&mark, -mark_tone / samprate, 0): phasor_step = cispi(2 f) (:503,507; src/osc.c:39).  cos / sin of 2 pi f here, the reference's own
  // sincospi there: the step may differ from the reference's in its last bit, a phase error of 1e-16 per sample that the renormalisation does not
  // touch -- far inside the decisions' margins, and what pins the decoder to the reference is its frames (tests/test_afsk_reference.py)
  kp.mark_step[0] = cos(2 * M_PI * (-mark / samprate)); kp.mark_step[1] = sin(2 * M_PI * (-mark / samprate));
  kp.space_step[0] = cos(2 * M_PI * (-space / samprate)); kp.space_step[1] = sin(2 * M_PI * (-space / samprate));
  mini_factor(H, kp.fwd.radix, &kp.fwd.nstages);
  RminiSlave& sl = kp.sl;
  sl.m.N = N; sl.m.olen = L;
  mini_factor(N, sl.m.radix, &sl.m.nstages);
  sl.real_out = 0; sl.out_off = 0;
  const ChanDescH h = make_chan_desc(CHZ_REAL, bins, N, 0);
  kp.d = ChanDesc{h.t0, h.cnt, h.src0, h.dir, h.conj, h.wrap, 0, 0};
  rmini_launch_geom(N, N, &m->lds, &m->threads);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(-2, "no HIP device: there is no CPU fallback");
  if (device < 0 || device >= ndev) return fail(-2, "device %d out of range (%d devices)", device, ndev);
  HIPOK(hipSetDevice(device));
  if (m->lds > 64 * 1024 && big_lds_prepare(reinterpret_cast<const void*>(afsk_ovs)))
    return fail(-3, "the runtime refuses %zu bytes of LDS per workgroup (N=%d)", m->lds, N);
  HIPOK(hipStreamCreateWithFlags(&m->s, hipStreamNonBlocking));
  std::vector<f2> tw((size_t)H + (size_t)H + 1 + (size_t)N);
  size_t at = 0;
  for (int k = 0; k < H; k++) tw[at++] = root_of_unity(k, H, -1);
  for (int k = 0; k <= H; k++) tw[at++] = root_of_unity(k, N, -1);
  for (int k = 0; k < N; k++) tw[at++] = root_of_unity(k, N, -1);
  int r = upload(&m->tw, tw);
  if (r) return r;
  kp.fwd.tw = m->tw; kp.tw_split = m->tw + H; sl.m.tw = m->tw + (size_t)H + (size_t)H + 1;
  r = afsk_grow(m, capacity);
  if (r) return r;
  static_assert(sizeof(AfskReq) % 8 == 0, "the samples follow the request records");
  const size_t stage = (sizeof(AfskReq) + sizeof(short) * (size_t)L) * (size_t)capacity;
  HIPOK(hipMalloc((void**)&m->d_stage, stage));
  HIPOK(hipMalloc((void**)&m->d_out, sizeof(AfskStatusK) * (size_t)capacity));
  HIPOK(hipMalloc((void**)&m->d_frames, (size_t)CHZ_AFSK_OUT_PITCH * (size_t)capacity));
  HIPOK(hipHostMalloc((void**)&m->h_stage, stage, hipHostMallocDefault));
  HIPOK(hipHostMalloc((void**)&m->h_out, sizeof(AfskStatusK) * (size_t)capacity, hipHostMallocDefault));
  HIPOK(hipHostMalloc((void**)&m->h_frames, (size_t)CHZ_AFSK_OUT_PITCH * (size_t)capacity, hipHostMallocDefault));
  kp.status = reinterpret_cast<AfskStatusK*>(m->d_out); kp.out = m->d_frames;
  HIPOK(hipDeviceSynchronize());
  guard.m = nullptr;
  *out = m;
  return 0;
}

int chz_afsk_capacity(const chz_afsk* m) { return m ? m->cap : -1; }

int chz_afsk_geometry(const chz_afsk* m, int out4[4]) {
  if (!m || !out4) return fail(-1, "bad argument");
  out4[0] = m->L; out4[1] = m->M; out4[2] = m->N; out4[3] = m->samppbit;
  return 0;
}

// one instance = one session's decoder, everything zero as in a fresh decode_task; returns its index
int chz_afsk_add(chz_afsk* m) {
  if (!m) return fail(-1, "null pool");
  std::lock_guard<std::mutex> lk(m->mu);
  HIPOK(hipSetDevice(m->device));
  if (m->free_inst.empty()) { const int r = afsk_grow(m, 2 * m->ninst); if (r) return r; }
  const int i = m->free_inst.back();
  HIPOK(hipMemsetAsync(m->state + i, 0, sizeof(AfskState), m->s));
  if (m->M > 1) HIPOK(hipMemsetAsync(m->hist + (size_t)i * (m->M - 1), 0, sizeof(float) * (size_t)(m->M - 1), m->s));
  HIPOK(hipMemsetAsync(m->frame + (size_t)i * CHZ_AFSK_FRAME_PITCH, 0, CHZ_AFSK_FRAME_PITCH, m->s));
  HIPOK(hipStreamSynchronize(m->s));
  m->free_inst.pop_back();
  m->used[(size_t)i] = 1;
  return i;
}
int chz_afsk_release(chz_afsk* m, int inst) {
  if (!m) return fail(-1, "null pool");
  std::lock_guard<std::mutex> lk(m->mu);
  if (inst < 0 || inst >= m->ninst) return fail(-1, "bad instance");
  if (!m->used[(size_t)inst]) return fail(-1, "instance %d is not in use", inst);
  m->used[(size_t)inst] = 0;
  m->free_inst.push_back(inst);
  return 0;
}
// response of an instance's slave: N complex values as set_filter leaves them (src/filter.c:968-1045), as chz_rmini_set_response takes them
int chz_afsk_set_response(chz_afsk* m, int inst, const float* resp) {
  if (!m || !resp) return fail(-1, "bad argument");
  std::lock_guard<std::mutex> lk(m->mu);
  if (inst < 0 || inst >= m->ninst) return fail(-1, "bad instance");
  if (!m->used[(size_t)inst]) return fail(-1, "instance %d is not in use", inst);
  HIPOK(hipSetDevice(m->device));
  const size_t N = (size_t)m->N;
  HIPOK(hipMemcpyAsync(m->resp + (size_t)inst * N, resp, sizeof(float2) * N, hipMemcpyHostToDevice, m->s));
  HIPOK(hipStreamSynchronize(m->s));
  return 0;
}
// Run one block of n decoders, ONE launch per chunk of `capacity`.  Request i: instance inst[i] takes the L 16-bit samples at samples[i]
// (the pool's byte order) -- on the host (samples_on_device = 0: staged with the request records) or on the device (1: read in place; the
// caller has made them complete) --; status[i] receives the block's record; frame j < status[i].nframes is copied to
// frames[i] + j * frame_stride, at most frame_stride bytes of it (status[i].frame_len[j] is its whole length, CRC included); the rest of
// frames[i] stays untouched.  The state is a recurrence: an instance may appear once in a call.  Every request is checked before the
// first launch: a refused call has written nothing and advanced no state.  Synchronous; thread-safe (callers are serialised).
int chz_afsk_execute(chz_afsk* m, int n, const int* inst, const void* const* samples, int samples_on_device, chz_afsk_status* status,
                     unsigned char* const* frames, int frame_stride) {
  if (!m || n < 0 || (n > 0 && (!inst || !samples || !status || !frames)) || frame_stride < 1) return fail(-1, "bad argument");
  if (n == 0) return 0;
  std::lock_guard<std::mutex> lk(m->mu);
  HIPOK(hipSetDevice(m->device));
  std::fill(m->seen.begin(), m->seen.end(), 0);
  for (int r = 0; r < n; r++) {
    if (inst[r] < 0 || inst[r] >= m->ninst || !samples[r] || !frames[r]) return fail(-1, "bad request %d", r);
    if (!m->used[(size_t)inst[r]]) return fail(-1, "request %d: instance %d is not in use", r, inst[r]);
    if (m->seen[(size_t)inst[r]]) return fail(-1, "request %d: instance %d is listed twice (its state is a recurrence over blocks)", r, inst[r]);
    m->seen[(size_t)inst[r]] = 1;
    if (samples_on_device && (reinterpret_cast<uintptr_t>(samples[r]) & 1)) return fail(-1, "request %d: 16-bit samples on the device at an odd address", r);
  }
  const size_t L = (size_t)m->L;
  for (int done = 0; done < n; done += m->cap) {
    const int k = n - done < m->cap ? n - done : m->cap;
    AfskReq* const h_req = reinterpret_cast<AfskReq*>(m->h_stage);
    unsigned short* const h_s = reinterpret_cast<unsigned short*>(m->h_stage + sizeof(AfskReq) * (size_t)k);
    const unsigned short* const d_s = reinterpret_cast<const unsigned short*>(m->d_stage + sizeof(AfskReq) * (size_t)k);
    for (int i = 0; i < k; i++) {
      const int r = done + i;
      if (!samples_on_device) memcpy(h_s + (size_t)i * L, samples[r], sizeof(short) * L);
      h_req[i] = AfskReq{samples_on_device ? reinterpret_cast<const unsigned short*>(samples[r]) : d_s + (size_t)i * L, inst[r], 0};
    }
    HIPOK(hipMemcpyAsync(m->d_stage, m->h_stage, sizeof(AfskReq) * (size_t)k + (samples_on_device ? 0 : sizeof(short) * L * (size_t)k), hipMemcpyHostToDevice, m->s));
    AfskParams kp = m->kp;
    kp.req = reinterpret_cast<const AfskReq*>(m->d_stage);
    hipLaunchKernelGGL(afsk_ovs, dim3(k), dim3(m->threads), m->lds, m->s, kp);
    HIPOK(hipGetLastError());
    HIPOK(hipMemcpyAsync(m->h_out, m->d_out, sizeof(AfskStatusK) * (size_t)k, hipMemcpyDeviceToHost, m->s));
    HIPOK(hipStreamSynchronize(m->s));
    // the frames: from the first request that completed one to the last, what they fill of their output areas -- nothing on most blocks,
    // one request's few hundred bytes otherwise (several requests completing in one chunk: one copy per request, one wait)
    const chz_afsk_status* st = reinterpret_cast<const chz_afsk_status*>(m->h_out);
    int copies = 0;
    for (int i = 0; i < k; i++) {
      if (st[i].nframes <= 0) continue;
      size_t bytes = 0;
      for (int j = 0; j < st[i].nframes; j++) bytes = (j ? (bytes + 7) / 8 * 8 : 0) + (size_t)st[i].frame_len[j];
      const size_t at = (size_t)CHZ_AFSK_OUT_PITCH * (size_t)i;
      HIPOK(hipMemcpyAsync(m->h_frames + at, m->d_frames + at, bytes, hipMemcpyDeviceToHost, m->s));
      copies++;
    }
    if (copies) HIPOK(hipStreamSynchronize(m->s));
    for (int i = 0; i < k; i++) {
      const int r = done + i;
      status[r] = st[i];
      size_t at = (size_t)CHZ_AFSK_OUT_PITCH * (size_t)i;
      for (int j = 0; j < st[i].nframes; j++) {
        const size_t len = (size_t)st[i].frame_len[j];
        memcpy(frames[r] + (size_t)j * (size_t)frame_stride, m->h_frames + at, len < (size_t)frame_stride ? len : (size_t)frame_stride);
        at += (len + 7) / 8 * 8;
      }
    }
  }
  return 0;
}

}  // extern "C"
