// scripts/micro/rmini_kernel.hip -- rmini_ovs (chz_kernels.h) timed with HIP events, outside the engine.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=fast -I ka9q-radio_amd/csrc -I include scripts/micro/rmini_kernel.hip -o scripts/micro/rmini_kernel.bin
//   rmini_kernel.bin [L M nreq]         default: wfm's composite master, 7680 7681, REAL + COMPLEX + COMPLEX slaves of olen L/8, 256 requests
// Prints the median and the shortest of 50 launches after 5 warm-up launches.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <algorithm>
#include "chz_engine.h"
#include "chz_launch.h"
using namespace chz;
#define OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

int main(int argc, char** argv) {
  const int L = argc > 1 ? atoi(argv[1]) : 7680, M = argc > 2 ? atoi(argv[2]) : 7681, nreq = argc > 3 ? atoi(argv[3]) : 256;
  const int N = L + M - 1, H = N / 2, ns = 3, olen = L / 8, P = (int)((long long)N * olen / L);
  if ((N & 1) || (long long)N * olen % L || P < 8) { fprintf(stderr, "bad geometry\n"); return 2; }
  RminiParams kp{};
  kp.N = N; kp.nslaves = ns; kp.fwd.N = H;
  if (!mini_factor(H, kp.fwd.radix, &kp.fwd.nstages)) return 2;
  std::vector<f2> tw;
  for (int k = 0; k < H; k++) tw.push_back(root_of_unity(k, H, -1));
  for (int k = 0; k <= H; k++) tw.push_back(root_of_unity(k, N, -1));
  for (int k = 0; k < P; k++) tw.push_back(root_of_unity(k, P, -1));
  float2 *d_tw, *d_resp; float *d_in, *d_out; RminiReq* d_req;
  const int stride = 2 * olen * ns;
  OK(hipMalloc((void**)&d_tw, sizeof(float2) * tw.size()));
  OK(hipMemcpy(d_tw, tw.data(), sizeof(float2) * tw.size(), hipMemcpyHostToDevice));
  OK(hipMalloc((void**)&d_resp, sizeof(float2) * (size_t)nreq * P));
  std::vector<float2> resp((size_t)nreq * P, make_float2(1.f / N, 0.f));
  OK(hipMemcpy(d_resp, resp.data(), sizeof(float2) * resp.size(), hipMemcpyHostToDevice));
  std::vector<float> in((size_t)nreq * N);
  for (size_t i = 0; i < in.size(); i++) in[i] = (float)((i * 2654435761u) >> 8 & 0xffff) / 65536.f - 0.5f;
  OK(hipMalloc((void**)&d_in, sizeof(float) * in.size()));
  OK(hipMemcpy(d_in, in.data(), sizeof(float) * in.size(), hipMemcpyHostToDevice));
  OK(hipMalloc((void**)&d_out, sizeof(float) * (size_t)nreq * stride));
  std::vector<RminiReq> req((size_t)nreq);
  // the three slaves of wfm (src/wfm.c:188-223): mono at 0, the 19 kHz pilot and the 38 kHz subcarrier of a 384 kHz composite, in bins of fs / N
  const int shifts[3] = {0, (int)(19000.0 / 384000.0 * N), (int)(38000.0 / 384000.0 * N)};
  for (int i = 0; i < nreq; i++) {
    memset(&req[(size_t)i], 0, sizeof(RminiReq));
    req[(size_t)i].mask = 7;
    for (int s = 0; s < ns; s++) {
      ChanDescH h = make_chan_desc(CHZ_REAL, H + 1, P, shifts[s]);
      req[(size_t)i].d[s] = ChanDesc{h.t0, h.cnt, h.src0, h.dir, h.conj, h.wrap, i, shifts[s]};
    }
  }
  OK(hipMalloc((void**)&d_req, sizeof(RminiReq) * req.size()));
  OK(hipMemcpy(d_req, req.data(), sizeof(RminiReq) * req.size(), hipMemcpyHostToDevice));
  kp.in = d_in; kp.out = d_out; kp.req = d_req; kp.out_stride = stride;
  kp.fwd.tw = d_tw; kp.tw_split = d_tw + H;
  for (int s = 0; s < ns; s++) {
    RminiSlave& sl = kp.s[s];
    sl.m.N = P; sl.m.olen = olen; sl.m.tw = d_tw + H + H + 1; sl.m.resp = d_resp;
    mini_factor(P, sl.m.radix, &sl.m.nstages);
    sl.real_out = s == 0; sl.out_off = 2 * olen * s;
  }
  size_t lds = 0; int threads = 0;
  rmini_launch_geom(N, P, &lds, &threads);                 // the engine's own choice (chz_plan.h)
  if (lds > CHZ_RMINI_LDS_MAX) { fprintf(stderr, "LDS %zu beyond 160 KB\n", lds); return 2; }
  if (lds > 64 * 1024 && big_lds_prepare(reinterpret_cast<const void*>(rmini_ovs))) return 3;
  hipStream_t st; OK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  hipEvent_t e0, e1; OK(hipEventCreate(&e0)); OK(hipEventCreate(&e1));
  std::vector<float> us;
  for (int it = 0; it < 55; it++) {
    OK(hipEventRecord(e0, st));
    hipLaunchKernelGGL(rmini_ovs, dim3(nreq), dim3(threads), lds, st, kp);
    OK(hipGetLastError());
    OK(hipEventRecord(e1, st));
    OK(hipStreamSynchronize(st));
    float ms = 0; OK(hipEventElapsedTime(&ms, e0, e1));
    if (it >= 5) us.push_back(ms * 1e3f);
  }
  std::sort(us.begin(), us.end());
  printf("rmini_ovs L %d M %d N %d P %d slaves R+C+C requests %d threads %d lds %zu: median %.1f us, min %.1f us per launch (%.2f us per request at the median)\n",
         L, M, N, P, nreq, threads, lds, us[us.size() / 2], us[0], us[us.size() / 2] / nreq);
  return 0;
}
