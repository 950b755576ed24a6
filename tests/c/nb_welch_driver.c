/* tests/c/nb_welch_driver.c -- TEST INFRASTRUCTURE.  The threading of the narrowband analyser's host side for the ThreadSanitizer run of
 * tests/test_welch_narrow_emulated.py: blocks pipelined over 4 lanes from 1, 2 or 4 issuing threads (CHZ_ENQ_THREADS) with analysers of
 * two fft_n attached to a plain and to a tuned bank -- the ring appends, their per-slot events and the hand-over that keeps them in
 * block order -- polls between and right behind the runs, a partial re-run, detach / attach between runs.  Nothing numeric is checked
 * here (tests/test_gpu_welch_narrow.py does that); every call must succeed and the race detector stay silent. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "chz_engine.h"

#define OK(call) do { if ((call) < 0) { fprintf(stderr, "%s: %s\n", #call, chz_last_error()); exit(2); } } while (0)

int main(void) {
  chz_engine *e = NULL;
  int const L = 25920, M = 6481, P = 300, olen = 240, nch = 8;
  if (getenv("CHZ_ENQ_THREADS")) OK(chz_set_option("enq_threads", getenv("CHZ_ENQ_THREADS")));
  OK(chz_engine_create(&e, L, M, CHZ_REAL, 0, NULL, 8));
  int const plain = chz_bank_create(e, P, olen, nch), tuned = chz_bank_create(e, P, olen, nch);
  if (plain < 0 || tuned < 0) { fprintf(stderr, "bank: %s\n", chz_last_error()); return 2; }
  float *resp = calloc((size_t)nch * P * 2, sizeof(float));
  for (int i = 0; i < nch * P; i++) resp[2 * i] = 1.0f / P;
  int *shifts = calloc((size_t)nch, sizeof(int)); double *freq = calloc((size_t)nch, sizeof(double));
  for (int i = 0; i < nch; i++) { shifts[i] = 100 + 37 * i; freq[i] = -3.3 / 12000.0; }
  OK(chz_bank_set_responses(e, plain, 0, nch, resp)); OK(chz_bank_set_shifts(e, plain, 0, nch, shifts)); OK(chz_bank_set_active(e, plain, nch));
  OK(chz_bank_set_responses(e, tuned, 0, nch, resp)); OK(chz_bank_set_tuning(e, tuned, 0, 0, nch, shifts, freq, NULL)); OK(chz_bank_set_active(e, tuned, nch));
  int nb[2] = {5, 0}; OK(chz_set_notches(e, nb, 2, 0.01));
  float *x = calloc((size_t)8 * L, sizeof(float));
  for (long i = 0; i < 8L * L; i++) x[i] = ((float)((i * 2654435761u) % 2001) / 1000.0f - 1.0f) * 0.05f;
  OK(chz_input_write(e, x, 8L * L - (M - 1))); OK(chz_input_write(e, x + (8L * L - (M - 1)), M - 1));

  int const wa = chz_bank_welch_create(e, plain, 64, 4, 64, 8), wb = chz_bank_welch_create(e, plain, 300, 2, 300, 3),
            wt = chz_bank_welch_create(e, tuned, 75, 2, 74, 8);
  if (wa < 0 || wb < 0 || wt < 0) { fprintf(stderr, "welch: %s\n", chz_last_error()); return 2; }
  float win[300]; for (int i = 0; i < 300; i++) win[i] = 1.0f;
  float bins[4 * 300]; double mm[8];
  chz_timing t;
  unsigned job = 0;
  for (int s = 0; s < 4; s++) { OK(chz_bank_welch_attach(e, wa, s, 2 * s, job)); OK(chz_welch_set_window(e, wa, s, win)); OK(chz_bank_welch_configure(e, wa, s, 64, 1 + 2 * s, 0.5)); }
  for (int s = 0; s < 2; s++) { OK(chz_bank_welch_attach(e, wb, s, 2, job)); OK(chz_welch_set_window(e, wb, s, win)); OK(chz_bank_welch_configure(e, wb, s, 300, 3, 0.75)); }
  for (int s = 0; s < 2; s++) { OK(chz_bank_welch_attach(e, wt, s, 7 - s, job)); OK(chz_welch_set_window(e, wt, s, win)); OK(chz_bank_welch_configure(e, wt, s, 74, 8, 0.5)); }
  for (int it = 0; it < 4; it++) {
    OK(chz_run_blocks(e, job, 8, 0, it == 3, &t));
    job += 8;
    OK(chz_bank_welch_poll(e, wa, 4, NULL, job - 1)); OK(chz_bank_welch_poll(e, wb, 2, NULL, job - 2)); OK(chz_bank_welch_poll(e, wt, 2, NULL, job - 1));
    OK(chz_bank_execute_range(e, plain, job - 1, 2, 3));
    OK(chz_step(e, job)); job++;                                   /* a block behind unfinished polls */
    OK(chz_welch_read(e, wa, 0, 4, bins, mm)); OK(chz_welch_read(e, wb, 0, 2, bins, mm)); OK(chz_welch_read(e, wt, 0, 2, bins, mm));
    OK(chz_bank_welch_detach(e, wa, it)); OK(chz_bank_welch_attach(e, wa, it, (it + 1) % nch, job));
    OK(chz_bank_set_shifts(e, plain, 0, 1, shifts));
    OK(chz_engine_check(e));
  }
  OK(chz_welch_destroy(e, wb));
  OK(chz_run_blocks(e, job, 8, 0, 0, &t)); job += 8;
  OK(chz_bank_destroy(e, tuned));
  OK(chz_run_blocks(e, job, 8, 0, 0, &t)); job += 8;
  OK(chz_bank_welch_poll(e, wa, 4, NULL, job - 1)); OK(chz_welch_read(e, wa, 0, 4, bins, mm));
  printf("driver ok blocks %u\n", job);
  chz_engine_destroy(e);
  free(resp); free(shifts); free(freq); free(x);
  return 0;
}
