// chz_rmini.inc -- pools of small REAL inline masters with decimating slaves (part of chz_engine.hip's translation unit).
//
// wfm (src/wfm.c:70-89), stereod (src/stereod.c:383-401), rdsd (src/rdsd.c:395-406), packetd (src/packetd.c:493-495) and ctcss
// (src/ctcss.c:269-281) keep a REAL master of a few thousand points per channel or session, hang one to three slaves of other
// lengths and types on it and run it inline.  As with the COMPLEX minis (chz_mini.inc) a pool holds the responses of all
// instances of one geometry -- (L, M, the slave list of (olen, out_type)) -- and ONE launch of rmini_ovs (chz_kernels.h) serves
// every instance that is due: one workgroup per request, forward transform, every selected slave's gather, backward transform
// and tail, all in LDS.  Stateless on the device: a request brings its whole N-sample window.
struct chz_rmini {
  int L = 0, M = 0, N = 0, cap = 0, device = 0, ns = 0;
  int olen[CHZ_RMINI_MAX_SLAVES] = {}, otype[CHZ_RMINI_MAX_SLAVES] = {}, P[CHZ_RMINI_MAX_SLAVES] = {};
  int out_off[CHZ_RMINI_MAX_SLAVES] = {}, out_stride = 0;
  size_t resp_off[CHZ_RMINI_MAX_SLAVES] = {};      // first response of slave s in `resp` (complex values); its rows are P[s] long
  RminiParams kp{};                                // everything that does not change from launch to launch
  size_t lds = 0; int threads = 0;
  hipStream_t s = nullptr;
  float2* resp = nullptr;        // [ns][cap][P_s]
  float2* tw = nullptr;          // forward [N/2], split [N/2 + 1], then [P_s] per slave
  // staging for one chunk of k <= cap requests, device and pinned: the k request records, then the k windows, packed so that ONE copy
  // carries both (sizeof(RminiReq) is a multiple of 8, the windows stay float2-aligned); outputs [cap][out_stride]
  unsigned char *d_stage = nullptr, *h_stage = nullptr;
  float *d_out = nullptr, *h_out = nullptr;
  std::vector<int> free_inst;
  std::vector<unsigned char> used;
  std::mutex mu;
};

extern "C" {

void chz_rmini_destroy(chz_rmini* m) {
  if (!m) return;
  hipSetDevice(m->device);
  if (m->s) hipStreamSynchronize(m->s);
  hipFree(m->resp); hipFree(m->tw); hipFree(m->d_stage); hipFree(m->d_out);
  if (m->h_stage) (void)hipHostFree(m->h_stage);
  if (m->h_out) (void)hipHostFree(m->h_out);
  if (m->s) hipStreamDestroy(m->s);
  delete m;
}

int chz_rmini_create(chz_rmini** out, int L, int M, int nslaves, const int* olen, const int* out_type, int capacity, int device) {
  if (!out) return fail(-1, "null out pointer");
  *out = nullptr;
  if (capacity < 1) return fail(-1, "bad REAL mini-master pool capacity");
  int Ps[CHZ_RMINI_MAX_SLAVES] = {};
  { char why[200]; const int rc = rmini_check_geom(L, M, nslaves, olen, out_type, Ps, why, sizeof why); if (rc) return fail(rc, "%s", why); }
  const int N = L + M - 1, H = N / 2;
  chz_rmini* m = new chz_rmini();
  struct Guard { chz_rmini* m; ~Guard() { if (m) chz_rmini_destroy(m); } } guard{m};
  m->L = L; m->M = M; m->N = N; m->cap = capacity; m->device = device; m->ns = nslaves;
  RminiParams& kp = m->kp;
  kp.N = N; kp.nslaves = nslaves; kp.fwd.N = H;
  mini_factor(H, kp.fwd.radix, &kp.fwd.nstages);
  int maxP = 0, off = 0;
  size_t roff = 0, twn = (size_t)H + (size_t)H + 1;
  for (int s = 0; s < nslaves; s++) {
    const int P = Ps[s];
    RminiSlave& sl = kp.s[s];
    sl.m.N = P; sl.m.olen = olen[s];
    mini_factor(P, sl.m.radix, &sl.m.nstages);
    sl.real_out = out_type[s] == CHZ_REAL;
    sl.out_off = off;
    off += sl.real_out ? (olen[s] + 1) / 2 * 2 : 2 * olen[s];           // complex rows start on an even float
    m->olen[s] = olen[s]; m->otype[s] = out_type[s]; m->P[s] = P; m->out_off[s] = sl.out_off;
    m->resp_off[s] = roff; roff += (size_t)capacity * P;
    twn += (size_t)P;
    if (P > maxP) maxP = P;
  }
  m->out_stride = kp.out_stride = off;
  rmini_launch_geom(N, maxP, &m->lds, &m->threads);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(-2, "no HIP device: there is no CPU fallback");
  if (device < 0 || device >= ndev) return fail(-2, "device %d out of range (%d devices)", device, ndev);
  HIPOK(hipSetDevice(device));
  if (m->lds > 64 * 1024 && big_lds_prepare(reinterpret_cast<const void*>(rmini_ovs)))
    return fail(-3, "the runtime refuses %zu bytes of LDS per workgroup (N=%d)", m->lds, N);
  HIPOK(hipStreamCreateWithFlags(&m->s, hipStreamNonBlocking));
  HIPOK(hipMalloc((void**)&m->resp, sizeof(float2) * roff));
  HIPOK(hipMemset(m->resp, 0, sizeof(float2) * roff));
  std::vector<f2> tw(twn);
  size_t at = 0;
  for (int k = 0; k < H; k++) tw[at++] = root_of_unity(k, H, -1);
  for (int k = 0; k <= H; k++) tw[at++] = root_of_unity(k, N, -1);
  for (int s = 0; s < nslaves; s++)
    for (int k = 0; k < m->P[s]; k++) tw[at++] = root_of_unity(k, m->P[s], -1);
  int r = upload(&m->tw, tw);
  if (r) return r;
  kp.fwd.tw = m->tw; kp.tw_split = m->tw + H;
  at = (size_t)H + (size_t)H + 1;
  for (int s = 0; s < nslaves; s++) { kp.s[s].m.tw = m->tw + at; at += (size_t)m->P[s]; kp.s[s].m.resp = m->resp + m->resp_off[s]; }
  static_assert(sizeof(RminiReq) % 8 == 0, "the windows follow the request records and are read as float2");
  const size_t stage = (sizeof(RminiReq) + sizeof(float) * (size_t)N) * (size_t)capacity;
  HIPOK(hipMalloc((void**)&m->d_stage, stage));
  HIPOK(hipMalloc((void**)&m->d_out, sizeof(float) * (size_t)capacity * m->out_stride));
  HIPOK(hipHostMalloc((void**)&m->h_stage, stage, hipHostMallocDefault));
  HIPOK(hipHostMalloc((void**)&m->h_out, sizeof(float) * (size_t)capacity * m->out_stride, hipHostMallocDefault));
  kp.out = m->d_out;                                              // (in / req: per launch, they depend on the chunk's size)
  HIPOK(hipDeviceSynchronize());
  m->used.assign((size_t)capacity, 0);
  for (int i = capacity - 1; i >= 0; i--) m->free_inst.push_back(i);
  guard.m = nullptr;
  *out = m;
  return 0;
}

int chz_rmini_capacity(const chz_rmini* m) { return m ? m->cap : -1; }

// would chz_rmini_create take this geometry?  0, or < 0 with the reason in chz_last_error(); touches no device
int chz_rmini_check(int L, int M, int nslaves, const int* olen, const int* out_type) {
  char why[200];
  const int rc = rmini_check_geom(L, M, nslaves, olen, out_type, nullptr, why, sizeof why);
  return rc ? fail(rc, "%s", why) : 0;
}

// one instance = one master with all its slaves; returns its index, or < 0 when the pool is full
int chz_rmini_add(chz_rmini* m) {
  if (!m) return fail(-1, "null pool");
  std::lock_guard<std::mutex> lk(m->mu);
  if (m->free_inst.empty()) return fail(-7, "REAL mini-master pool is full (%d instances)", m->cap);
  const int i = m->free_inst.back(); m->free_inst.pop_back();
  m->used[(size_t)i] = 1;
  return i;
}
int chz_rmini_release(chz_rmini* m, int inst) {
  if (!m || inst < 0 || inst >= m->cap) return fail(-1, "bad instance");
  std::lock_guard<std::mutex> lk(m->mu);
  if (!m->used[(size_t)inst]) return fail(-1, "instance %d is not in use", inst);
  m->used[(size_t)inst] = 0;
  m->free_inst.push_back(inst);
  return 0;
}
// response of one slave of one instance: P_s complex values as set_filter leaves them (src/filter.c:968-1045; a REAL slave's
// P_s/2 + 1 bins come first, the rest is not read)
int chz_rmini_set_response(chz_rmini* m, int inst, int slave, const float* resp) {
  if (!m || !resp || inst < 0 || inst >= m->cap || slave < 0 || slave >= m->ns) return fail(-1, "bad argument");
  std::lock_guard<std::mutex> lk(m->mu);
  if (!m->used[(size_t)inst]) return fail(-1, "instance %d is not in use", inst);
  HIPOK(hipSetDevice(m->device));
  const size_t P = (size_t)m->P[slave];
  HIPOK(hipMemcpyAsync(m->resp + m->resp_off[slave] + (size_t)inst * P, resp, sizeof(float2) * P, hipMemcpyHostToDevice, m->s));
  HIPOK(hipStreamSynchronize(m->s));
  return 0;
}
// Run n requests, ONE launch per chunk of `capacity`.  Request i: instance inst[i] transforms the window win[i] (N floats on the
// host: the M-1 old and L new samples of its block) and runs every slave s that mask[i] selects (NULL: all) with bin shift
// shift[i*nslaves+s] (execute_filter_output's argument; NULL: 0) and ISB flag isb[i*nslaves+s] (NULL: off); the slave's olen_s
// complex or float samples go to out[i*nslaves+s], which may be NULL.  Rows of slaves left out stay untouched.  Synchronous;
// thread-safe (requests of concurrent callers are serialised -- the drop-in batches them first).
int chz_rmini_execute(chz_rmini* m, int n, const int* inst, const float* const* win, const int* shift, const unsigned char* mask,
                      const unsigned char* isb, float* const* out) {
  if (!m || n < 0 || (n > 0 && (!inst || !win || !out))) return fail(-1, "bad argument");
  if (n == 0) return 0;
  std::lock_guard<std::mutex> lk(m->mu);
  HIPOK(hipSetDevice(m->device));
  const int ns = m->ns, bins = m->N / 2 + 1;
  const unsigned all = (1u << ns) - 1u;
  for (int r = 0; r < n; r++) {                                   // all of them before the first launch: a refused call has written nothing
    if (inst[r] < 0 || inst[r] >= m->cap || !win[r]) return fail(-1, "bad request %d", r);
    if (!m->used[(size_t)inst[r]]) return fail(-1, "request %d: instance %d is not in use", r, inst[r]);
  }
  for (int done = 0; done < n; done += m->cap) {
    const int k = n - done < m->cap ? n - done : m->cap;
    RminiReq* const h_req = reinterpret_cast<RminiReq*>(m->h_stage);
    float* const h_in = reinterpret_cast<float*>(m->h_stage + sizeof(RminiReq) * (size_t)k);
    for (int i = 0; i < k; i++) {
      const int r = done + i;
      memcpy(h_in + (size_t)i * m->N, win[r], sizeof(float) * (size_t)m->N);
      RminiReq& q = h_req[i];
      q.mask = (int)((mask ? mask[r] : all) & all); q.pad[0] = q.pad[1] = q.pad[2] = 0;
      for (int s = 0; s < CHZ_RMINI_MAX_SLAVES; s++) {
        const int sh = (s < ns && shift) ? shift[(size_t)r * ns + s] : 0;
        ChanDescH h = s < ns ? make_chan_desc(CHZ_REAL, bins, m->P[s], sh) : ChanDescH{0, 0, 0, 1, 0, 0};
        q.d[s] = ChanDesc{h.t0, h.cnt, h.src0, h.dir, h.conj, h.wrap, inst[r], sh};
        q.isb[s] = (s < ns && isb) ? (isb[(size_t)r * ns + s] != 0) : 0;
      }
    }
    HIPOK(hipMemcpyAsync(m->d_stage, m->h_stage, (sizeof(RminiReq) + sizeof(float) * (size_t)m->N) * (size_t)k, hipMemcpyHostToDevice, m->s));
    RminiParams kp = m->kp;
    kp.req = reinterpret_cast<const RminiReq*>(m->d_stage);
    kp.in = reinterpret_cast<const float*>(m->d_stage + sizeof(RminiReq) * (size_t)k);
    hipLaunchKernelGGL(rmini_ovs, dim3(k), dim3(m->threads), m->lds, m->s, kp);
    HIPOK(hipGetLastError());
    HIPOK(hipMemcpyAsync(m->h_out, m->d_out, sizeof(float) * (size_t)k * m->out_stride, hipMemcpyDeviceToHost, m->s));
    HIPOK(hipStreamSynchronize(m->s));
    for (int i = 0; i < k; i++) {
      const int r = done + i;
      for (int s = 0; s < ns; s++) {
        float* o = out[(size_t)r * ns + s];
        if (!o || !((h_req[i].mask >> s) & 1)) continue;
        memcpy(o, m->h_out + (size_t)i * m->out_stride + m->out_off[s],
               sizeof(float) * (size_t)m->olen[s] * (m->otype[s] == CHZ_REAL ? 1 : 2));
      }
    }
  }
  return 0;
}

}  // extern "C"
