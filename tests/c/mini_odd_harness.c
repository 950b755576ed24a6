/* tests/c/mini_odd_harness.c -- one small COMPLEX inline master with a same-size COMPLEX slave through filter.h, the way radiod
 * builds a channel's filter2 (src/radio.c:1572-1594), at a geometry of the caller's choice (TEST CODE).
 *
 *   mini_odd_harness <dir> L M nblocks isb low high beta shift_0 .. shift_{nblocks-1}
 *
 * <dir>/in.bin holds nblocks * L complex samples; block b goes in with write_cfilter and comes out of execute_filter_output(shift_b)
 * into <dir>/out.bin.  stdout: "engines <n> inline <0|1> points <N> bins <slave bins>" -- a pooled inline master creates no engine.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <complex.h>
#include "ka9q_filter_abi.h"
#include "ka9q_filter_hip_ext.h"

int main(int argc, char **argv) {
  if (argc < 9) { fprintf(stderr, "usage: %s dir L M nblocks isb low high beta shifts...\n", argv[0]); return 1; }
  int const L = atoi(argv[2]), M = atoi(argv[3]), nblocks = atoi(argv[4]), isb = atoi(argv[5]);
  double const low = atof(argv[6]), high = atof(argv[7]), beta = atof(argv[8]);
  if (L < 1 || M < 1 || nblocks < 1 || argc != 9 + nblocks) { fprintf(stderr, "bad arguments\n"); return 1; }
  char path[512];
  float complex *x = malloc(sizeof *x * (size_t)nblocks * L), *y = malloc(sizeof *y * (size_t)nblocks * L);
  snprintf(path, sizeof path, "%s/in.bin", argv[1]);
  FILE *f = fopen(path, "rb");
  if (!x || !y || !f || fread(x, sizeof *x, (size_t)nblocks * L, f) != (size_t)nblocks * L) { perror("input"); return 1; }
  fclose(f);
  struct filter_in in; struct filter_out out;
  memset(&in, 0, sizeof in); memset(&out, 0, sizeof out);
  if (create_filter_input(&in, L, M, COMPLEX) != 0) { fprintf(stderr, "create_filter_input failed\n"); return 2; }
  in.perform_inline = true;
  if (create_filter_output(&out, &in, L, COMPLEX) != 0) { fprintf(stderr, "create_filter_output failed\n"); return 2; }
  out.isb = isb != 0;                                            /* set by the caller after create (src/radio.c:1586) */
  if (set_filter(&out, low, high, beta) != 0) { fprintf(stderr, "set_filter failed\n"); return 2; }
  for (int b = 0; b < nblocks; b++) {
    if (write_cfilter(&in, x + (size_t)b * L, L) != 1) { fprintf(stderr, "write_cfilter did not complete block %d\n", b); return 3; }
    if (execute_filter_output(&out, atoi(argv[9 + b])) != 0) { fprintf(stderr, "execute_filter_output failed\n"); return 3; }
    memcpy(y + (size_t)b * L, out.output.c, sizeof *y * (size_t)L);
  }
  printf("engines %d inline %d points %d bins %d\n", ka9q_hip_engines_created(), (int)in.perform_inline, in.points, out.bins);
  snprintf(path, sizeof path, "%s/out.bin", argv[1]);
  f = fopen(path, "wb");
  if (!f || fwrite(y, sizeof *y, (size_t)nblocks * L, f) != (size_t)nblocks * L) { perror("output"); return 1; }
  fclose(f);
  delete_filter_output(&out);
  delete_filter_input(&in);
  free(x); free(y);
  return 0;
}
