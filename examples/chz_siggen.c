/* examples/chz_siggen.c -- the synthetic front end on the device, from plain C: sig_gen's carrier generated straight into the
 * input ring by chz_input_generate, no sample crossing the link.
 *
 * One 129.6 MS/s real master (L = 2,592,000, M = 648,001), one 12 kHz channel (P = 300, olen = 240) tuned to a bin-centred
 * carrier of amplitude a with no noise, scaled as sig_gen scales a real front end (scale = 10^(3/20)).  Known answer (SURVEY 8c,
 * analytic test 1): with a response whose DC bin is sqrt(2)/N every output sample of a block has magnitude a scale / sqrt(2).
 *
 *   gcc -O2 -I include examples/chz_siggen.c -L ka9q-radio_amd -lchz_hip -Wl,-rpath,$PWD/ka9q-radio_amd -lm -o chz_siggen
 */
#include <stdio.h>
#include <stdlib.h>
#include <math.h>
#include "chz_engine.h"

#define CHECK(call) do { if ((call) < 0) { fprintf(stderr, "%s: %s\n", #call, chz_last_error()); return 1; } } while (0)

int main(void) {
  const int L = 2592000, M = 648001, N = L + M - 1, P = 300, olen = 240;
  const int k0 = 250000;                       /* 10.000 MHz: bin-centred (40 Hz bins) */
  chz_siggen_params sg = {(double)k0 / N, 0.1, 0.0, pow(10.0, 3.0 / 20.0), 1};
  const double want = sg.amplitude * sg.scale / sqrt(2.0);
  chz_engine *e = NULL;
  CHECK(chz_siggen_check(CHZ_REAL, &sg));
  CHECK(chz_engine_create(&e, L, M, CHZ_REAL, 0, NULL, 8));

  int bank = chz_bank_create(e, P, olen, 1);
  if (bank < 0) { fprintf(stderr, "%s\n", chz_last_error()); return 1; }
  /* a flat response over the whole channel with set_filter's gain: H[k] = sqrt(2)/N */
  float *resp = calloc((size_t)2 * P, sizeof *resp);
  for (int k = 0; k < P; k++) resp[2 * k] = (float)(sqrt(2.0) / N);
  CHECK(chz_bank_set_responses(e, bank, 0, 1, resp));
  CHECK(chz_bank_set_shifts(e, bank, 0, 1, &k0));
  CHECK(chz_bank_set_active(e, bank, 1));

  CHECK(chz_input_siggen_set(e, &sg));
  float *out = malloc(sizeof *out * 2 * (size_t)olen);
  double worst = 0, mag = 0, energy = 0;
  for (unsigned job = 0; job < 3; job++) {
    unsigned ticket = 0;
    CHECK(chz_input_generate(e, L, &ticket));  /* the block's L new samples, made where they are used */
    CHECK(chz_step(e, job));                   /* forward transform + every bank */
    CHECK(chz_bank_read(e, bank, 0, 1, out));
    CHECK(chz_input_generate_stats(e, ticket, &energy));
    if (job == 0) continue;                    /* the first window starts with M-1 zeros: not a steady tone yet */
    for (int n = 0; n < olen; n++) {
      mag = hypot(out[2 * n], out[2 * n + 1]);
      const double err = fabs(mag - want) / want;
      if (err > worst) worst = err;
    }
  }
  unsigned long long pos = 0;
  CHECK(chz_input_siggen_tell(e, &pos));
  printf("generated %llu samples on the device; input power %.6f (a^2/2 = %.6f)\n", pos, energy / L, sg.amplitude * sg.amplitude / 2);
  printf("bin-centred carrier: |y| = %.7f, a scale / sqrt(2) = %.7f, within %.2e (relative)\n", mag, want, worst);
  chz_engine_destroy(e);
  free(resp); free(out);
  return worst < 1e-4 ? 0 : 2;
}
