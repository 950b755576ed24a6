// chz_mini.inc -- pools of small inline masters (part of chz_engine.hip's translation unit).
//
// radiod gives every channel that asks for it (filter2 = 1..., share/presets.conf:204,223,297) a private
// COMPLEX master of N = round2(2 * blocksize) points with one same-size slave (src/radio.c:1572-1594) and
// runs it inline in the channel thread.  On the GPU thousands of 512..4096-point masters must not be
// thousands of engines: a pool holds the responses of all instances of one geometry, and ONE launch of
// mini_ovs (chz_kernels.h) serves every instance that is due, one workgroup each, entirely in LDS.
// Stateless on the device: each request brings its whole N-sample window (history + new samples, as the
// caller's mirrored ring holds them contiguously), so overlap bookkeeping stays where the reference keeps it.
struct chz_mini {
  int L = 0, M = 0, N = 0, cap = 0, device = 0;
  int nstages = 0, radix[CHZ_MINI_MAX_STAGES] = {};
  hipStream_t s = nullptr;
  float2* resp = nullptr;        // [cap][N]
  float2* tw = nullptr;          // [N]
  float2 *d_in = nullptr, *d_out = nullptr; MiniReq* d_req = nullptr;      // device staging [cap]
  float2 *h_in = nullptr, *h_out = nullptr; MiniReq* h_req = nullptr;      // pinned staging [cap]
  std::vector<int> free_inst;
  std::vector<unsigned char> used;
  std::mutex mu;
};

extern "C" {

void chz_mini_destroy(chz_mini* m) {
  if (!m) return;
  hipSetDevice(m->device);
  if (m->s) hipStreamSynchronize(m->s);
  hipFree(m->resp); hipFree(m->tw); hipFree(m->d_in); hipFree(m->d_out); hipFree(m->d_req);
  if (m->h_in) (void)hipHostFree(m->h_in);
  if (m->h_out) (void)hipHostFree(m->h_out);
  if (m->h_req) (void)hipHostFree(m->h_req);
  if (m->s) hipStreamDestroy(m->s);
  delete m;
}

int chz_mini_create(chz_mini** out, int L, int M, int capacity, int device) {
  if (!out) return fail(-1, "null out pointer");
  *out = nullptr;
  if (capacity < 1) return fail(-1, "bad mini-master geometry");
  { char why[200]; const int rc = mini_check_geom(L, M, why, sizeof why); if (rc) return fail(rc, "%s", why); }
  const int N = L + M - 1;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(-2, "no HIP device: there is no CPU fallback");
  if (device < 0 || device >= ndev) return fail(-2, "device %d out of range (%d devices)", device, ndev);
  HIPOK(hipSetDevice(device));
  chz_mini* m = new chz_mini();
  struct Guard { chz_mini* m; ~Guard() { if (m) chz_mini_destroy(m); } } guard{m};
  m->L = L; m->M = M; m->N = N; m->cap = capacity; m->device = device;
  (void)mini_factor(N, m->radix, &m->nstages);
  // two N-point buffers in LDS: beyond 4096 points that is more than the 64 KB a kernel gets without asking
  if (sizeof(float2) * 2 * (size_t)N > 64 * 1024 && big_lds_prepare(reinterpret_cast<const void*>(mini_ovs)))
    return fail(-3, "the runtime refuses %zu bytes of LDS per workgroup (N=%d)", sizeof(float2) * 2 * (size_t)N, N);
  HIPOK(hipStreamCreateWithFlags(&m->s, hipStreamNonBlocking));
  HIPOK(hipMalloc((void**)&m->resp, sizeof(float2) * (size_t)capacity * N));
  HIPOK(hipMemset(m->resp, 0, sizeof(float2) * (size_t)capacity * N));
  std::vector<f2> tw((size_t)N);
  for (int k = 0; k < N; k++) tw[(size_t)k] = root_of_unity(k, N, -1);
  int r = upload(&m->tw, tw);
  if (r) return r;
  HIPOK(hipMalloc((void**)&m->d_in, sizeof(float2) * (size_t)capacity * N));
  HIPOK(hipMalloc((void**)&m->d_out, sizeof(float2) * (size_t)capacity * L));
  HIPOK(hipMalloc((void**)&m->d_req, sizeof(MiniReq) * (size_t)capacity));
  HIPOK(hipHostMalloc((void**)&m->h_in, sizeof(float2) * (size_t)capacity * N, hipHostMallocDefault));
  HIPOK(hipHostMalloc((void**)&m->h_out, sizeof(float2) * (size_t)capacity * L, hipHostMallocDefault));
  HIPOK(hipHostMalloc((void**)&m->h_req, sizeof(MiniReq) * (size_t)capacity, hipHostMallocDefault));
  HIPOK(hipDeviceSynchronize());
  m->used.assign((size_t)capacity, 0);
  for (int i = capacity - 1; i >= 0; i--) m->free_inst.push_back(i);
  guard.m = nullptr;
  *out = m;
  return 0;
}

int chz_mini_capacity(const chz_mini* m) { return m ? m->cap : -1; }

// one instance = one (master, slave) pair of the pool's geometry; returns its index, or < 0 when the pool is full
int chz_mini_add(chz_mini* m) {
  if (!m) return fail(-1, "null pool");
  std::lock_guard<std::mutex> lk(m->mu);
  if (m->free_inst.empty()) return fail(-7, "mini-master pool is full (%d instances)", m->cap);
  const int i = m->free_inst.back(); m->free_inst.pop_back();
  m->used[(size_t)i] = 1;
  return i;
}
int chz_mini_release(chz_mini* m, int inst) {
  if (!m || inst < 0 || inst >= m->cap) return fail(-1, "bad instance");
  std::lock_guard<std::mutex> lk(m->mu);
  if (!m->used[(size_t)inst]) return fail(-1, "instance %d is not in use", inst);
  m->used[(size_t)inst] = 0;
  m->free_inst.push_back(inst);
  return 0;
}
// response[N] complex as set_filter leaves it (src/filter.c:968-1045)
int chz_mini_set_response(chz_mini* m, int inst, const float* resp) {
  if (!m || !resp || inst < 0 || inst >= m->cap) return fail(-1, "bad argument");
  std::lock_guard<std::mutex> lk(m->mu);
  HIPOK(hipSetDevice(m->device));
  HIPOK(hipMemcpyAsync(m->resp + (size_t)inst * m->N, resp, sizeof(float2) * (size_t)m->N, hipMemcpyHostToDevice, m->s));
  HIPOK(hipStreamSynchronize(m->s));
  return 0;
}
// Run n requests in ONE launch.  Request i: instance inst[i] filters the window win[i] (N complex samples on the
// host: the M-1 old and L new samples of its block) with bin shift shift[i] (execute_filter_output's argument) and
// ISB flag isb[i]; its L output samples go to out[i].  Synchronous; thread-safe (requests of concurrent callers are
// serialised -- the drop-in batches them first).
int chz_mini_execute(chz_mini* m, int n, const int* inst, const float* const* win, const int* shift, const unsigned char* isb,
                     float* const* out) {
  if (!m || n < 0 || (n > 0 && (!inst || !win || !out))) return fail(-1, "bad argument");
  if (n == 0) return 0;
  std::lock_guard<std::mutex> lk(m->mu);
  HIPOK(hipSetDevice(m->device));
  for (int done = 0; done < n; done += m->cap) {
    const int k = n - done < m->cap ? n - done : m->cap;
    for (int i = 0; i < k; i++) {
      const int r = done + i;
      if (inst[r] < 0 || inst[r] >= m->cap || !win[r] || !out[r]) return fail(-1, "bad request %d", r);
      memcpy(m->h_in + (size_t)i * m->N, win[r], sizeof(float2) * (size_t)m->N);
      ChanDescH h = make_chan_desc(CHZ_COMPLEX, m->N, m->N, shift ? shift[r] : 0);
      m->h_req[i].d = ChanDesc{h.t0, h.cnt, h.src0, h.dir, h.conj, h.wrap, inst[r], shift ? shift[r] : 0};
      m->h_req[i].isb = isb ? (isb[r] != 0) : 0; m->h_req[i].pad = 0;
    }
    HIPOK(hipMemcpyAsync(m->d_in, m->h_in, sizeof(float2) * (size_t)k * m->N, hipMemcpyHostToDevice, m->s));
    HIPOK(hipMemcpyAsync(m->d_req, m->h_req, sizeof(MiniReq) * (size_t)k, hipMemcpyHostToDevice, m->s));
    MiniParams p{};
    p.in = m->d_in; p.out = m->d_out; p.req = m->d_req; p.resp = m->resp; p.tw = m->tw;
    p.N = m->N; p.olen = m->L; p.nstages = m->nstages;
    for (int s = 0; s < m->nstages; s++) p.radix[s] = m->radix[s];
    const int threads = m->N / 4 >= 256 ? 256 : (m->N / 4 >= 64 ? (m->N / 4 + 63) / 64 * 64 : 64);
    hipLaunchKernelGGL(mini_ovs, dim3(k), dim3(threads), sizeof(float2) * 2 * (size_t)m->N, m->s, p);
    HIPOK(hipGetLastError());
    HIPOK(hipMemcpyAsync(m->h_out, m->d_out, sizeof(float2) * (size_t)k * m->L, hipMemcpyDeviceToHost, m->s));
    HIPOK(hipStreamSynchronize(m->s));
    for (int i = 0; i < k; i++) memcpy(out[done + i], m->h_out + (size_t)i * m->L, sizeof(float2) * (size_t)m->L);
  }
  return 0;
}

}  // extern "C"
