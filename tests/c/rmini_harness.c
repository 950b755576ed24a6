/* tests/c/rmini_harness.c -- small REAL inline masters driven the way wfm, stereod and packetd drive theirs (TEST CODE).
 *
 *   rmini_harness <dir> <pool 0|1> <n_stereod> <n_packetd> <nblocks> [bench | <rounds>]
 *
 * Every thread owns one REAL master (perform_inline) and its slaves and loops, per block,
 *     write_rfilter(&master, samples, L);  execute_filter_output(&slave[s], shift[s]) for every slave, in creation order
 * (src/wfm.c:183-223, src/packetd.c:493-560).  Threads 0 .. n_stereod-1 are stereod-shaped (L 1920, M 1921; a REAL and two COMPLEX
 * slaves of olen 240), the next n_packetd packetd-shaped (L 960, M 961; one COMPLEX slave of olen 960), and ONE more stereod-shaped
 * master gets a fourth slave the pool cannot serve (olen 17: P = 34 = 2 * 17) before its first block.  Thread t with t % 3 == 0 moves
 * its second slave to another shift from block 2 on.  Odd threads delete their master BEFORE its slaves (src/wfm.c:290-293).
 * Input: <dir>/in.bin, [threads][nblocks * L] float32 (with `bench`: noise made here).  Output: <dir>/out<pool>.bin, per thread, per slave, per block, olen samples.
 * With <rounds> the whole life -- create, run, delete -- is lived that many times in one process (the last round's output is written):
 * the instances a round's masters held in their pools must be free again for the next.
 * stdout: "pooling <ka9q_hip_pool_real_masters()> engines <ka9q_hip_engines_created(), last round> masters <n>
 * pools <ka9q_hip_real_master_pools()> in_use_running <instances taken after the last block> in_use_end <after the last delete>";
 * with `bench` the threads run in lock step
 * and creation time, device memory and the per-block wall times are printed too (no fourth-slave master then).
 */
#define _GNU_SOURCE 1
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <pthread.h>
#include <complex.h>
#include <time.h>
#include <stdint.h>
#include "ka9q_filter_abi.h"
#include "ka9q_filter_hip_ext.h"

extern int hipMemGetInfo(size_t *, size_t *) __attribute__((weak));     /* the runtime the engine library brings along, if it is a device build */

struct shape { int L, M, nsl, olen[4], type[4], shift[4]; double lo[4], hi[4]; };
static const struct shape Stereod = {1920, 1921, 3, {240, 240, 240, 17}, {REAL, COMPLEX, COMPLEX, COMPLEX}, {0, 152, 304, 40},
                                     {0.002, -0.01, -0.3, -0.4}, {0.3, 0.01, 0.3, 0.4}};
static const struct shape Packetd = {960, 961, 1, {960}, {COMPLEX}, {340}, {-0.2}, {0.25}};

struct thr {
  int idx; struct shape sh; const float *in; float *out; size_t out_floats;
  struct filter_in master; struct filter_out slave[4];
  int rc;
};
static int Nblocks, Bench;
static pthread_barrier_t Bar;
static double *Block_ms;

static double now_ms(void) { struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return t.tv_sec * 1e3 + t.tv_nsec / 1e6; }

static int setup(struct thr *t) {
  struct shape const *s = &t->sh;
  if (create_filter_input(&t->master, s->L, s->M, REAL) != 0) return -1;
  t->master.perform_inline = true;
  for (int k = 0; k < s->nsl; k++) {
    if (create_filter_output(&t->slave[k], &t->master, s->olen[k], (enum filtertype)s->type[k]) != 0) return -2;
    if (set_filter(&t->slave[k], s->lo[k], s->hi[k], 5.0 + k) != 0) return -3;
  }
  return 0;
}
static int one_block(struct thr *t, int b) {
  struct shape const *s = &t->sh;
  if (write_rfilter(&t->master, t->in + (size_t)b * s->L, s->L) != 1) return -4;
  size_t at = 0;
  for (int k = 0; k < s->nsl; k++) {
    int const shift = s->shift[k] + 4 * (t->idx % 5) + ((k == 1 && t->idx % 3 == 0 && b >= 2) ? 8 : 0);
    if (execute_filter_output(&t->slave[k], shift) != 0) return -5;
    size_t const n = (size_t)s->olen[k] * (s->type[k] == REAL ? 1 : 2);
    float *dst = t->out + at * (size_t)Nblocks + (size_t)b * n;
    memcpy(dst, s->type[k] == REAL ? (const void *)t->slave[k].output.r : (const void *)t->slave[k].output.c, n * sizeof(float));
    at += n;
  }
  return 0;
}
static void teardown(struct thr *t) {
  if (t->idx & 1) delete_filter_input(&t->master);
  for (int k = 0; k < t->sh.nsl; k++) delete_filter_output(&t->slave[k]);
  if (!(t->idx & 1)) delete_filter_input(&t->master);
}
static void *run(void *arg) {
  struct thr *t = arg;
  for (int b = 0; b < Nblocks && t->rc == 0; b++) {
    if (Bench) pthread_barrier_wait(&Bar);
    double const t0 = now_ms();
    t->rc = one_block(t, b);
    if (Bench) { pthread_barrier_wait(&Bar); if (t->idx == 0) Block_ms[b] = now_ms() - t0; }
  }
  return NULL;
}
static int cmp(const void *a, const void *b) { double x = *(const double *)a, y = *(const double *)b; return x < y ? -1 : x > y; }

int main(int argc, char **argv) {
  if (argc < 6) { fprintf(stderr, "usage: rmini_harness dir pool n_stereod n_packetd nblocks [bench]\n"); return 2; }
  const char *dir = argv[1];
  int const pool = atoi(argv[2]), ns = atoi(argv[3]), np = atoi(argv[4]);
  Nblocks = atoi(argv[5]); Bench = argc > 6 && strcmp(argv[6], "bench") == 0;
  int const rounds = (argc > 6 && !Bench && atoi(argv[6]) > 0) ? atoi(argv[6]) : 1;
  int const T = ns + np + (Bench ? 0 : 1);
  int const pooling = ka9q_hip_pool_real_masters(pool);
  struct thr *th = calloc((size_t)T, sizeof *th);
  size_t in_floats = 0, out_floats = 0;
  for (int i = 0; i < T; i++) {
    th[i].idx = i; th[i].sh = i < ns ? Stereod : i < ns + np ? Packetd : Stereod;
    if (i == ns + np) th[i].sh.nsl = 4;
    for (int k = 0; k < th[i].sh.nsl; k++) th[i].out_floats += (size_t)th[i].sh.olen[k] * (th[i].sh.type[k] == REAL ? 1 : 2);
    in_floats += (size_t)Nblocks * th[i].sh.L; out_floats += th[i].out_floats * (size_t)Nblocks;
  }
  float *in = malloc(in_floats * sizeof(float)), *out = calloc(out_floats, sizeof(float));
  char path[4096];
  snprintf(path, sizeof path, "%s/in.bin", dir);
  FILE *f = NULL;
  if (!in || !out) return 2;
  if (Bench) {                                                     /* timing only: uniform noise made here */
    uint32_t z = 12345u;
    for (size_t i = 0; i < in_floats; i++) { z = z * 1664525u + 1013904223u; in[i] = (float)(z >> 8) / 8388608.0f - 1.0f; }
  } else {
    f = fopen(path, "rb");
    if (!f || fread(in, sizeof(float), in_floats, f) != in_floats) { fprintf(stderr, "rmini_harness: cannot read %s\n", path); return 2; }
    fclose(f);
  }
  { size_t a = 0, o = 0; for (int i = 0; i < T; i++) { th[i].in = in + a; th[i].out = out + o; a += (size_t)Nblocks * th[i].sh.L; o += th[i].out_floats * (size_t)Nblocks; } }
  size_t free0 = 0, free1 = 0, total = 0;
  if (Bench && hipMemGetInfo) { struct filter_in w = {0}; if (create_filter_input(&w, 25920, 6481, REAL) == 0) delete_filter_input(&w); hipMemGetInfo(&free0, &total); }
  int engines = 0, in_use_running = 0, bad = 0;
  double create_ms = 0;
  pthread_t *tid = calloc((size_t)T, sizeof *tid);
  for (int round = 0; round < rounds; round++) {
  int const eng0 = ka9q_hip_engines_created();
  double const c0 = now_ms();
  for (int i = 0; i < T; i++) if ((th[i].rc = setup(&th[i])) != 0) { fprintf(stderr, "rmini_harness: setup of master %d failed (%d)\n", i, th[i].rc); return 1; }
  create_ms = now_ms() - c0;
  if (Bench) { pthread_barrier_init(&Bar, NULL, (unsigned)T); Block_ms = calloc((size_t)Nblocks, sizeof(double)); }
  for (int i = 0; i < T; i++) pthread_create(&tid[i], NULL, run, &th[i]);
  for (int i = 0; i < T; i++) pthread_join(tid[i], NULL);
  if (Bench && hipMemGetInfo) hipMemGetInfo(&free1, &total);
  engines = ka9q_hip_engines_created() - eng0;
  (void)ka9q_hip_real_master_pools(&in_use_running);
  for (int i = 0; i < T; i++) if (th[i].rc != 0) { fprintf(stderr, "rmini_harness: master %d failed (%d)\n", i, th[i].rc); bad = 1; }
  for (int i = 0; i < T; i++) teardown(&th[i]);
  }
  int in_use_end = 0;
  int const pools = ka9q_hip_real_master_pools(&in_use_end);
  snprintf(path, sizeof path, "%s/out%d.bin", dir, pool);
  f = fopen(path, "wb");
  if (!f || fwrite(out, sizeof(float), out_floats, f) != out_floats) { fprintf(stderr, "rmini_harness: cannot write %s\n", path); return 2; }
  fclose(f);
  printf("pooling %d engines %d masters %d pools %d in_use_running %d in_use_end %d\n", pooling, engines, T, pools, in_use_running, in_use_end);
  if (Bench) {
    double first = Block_ms[0], worst = 0;
    for (int b = 1; b < Nblocks; b++) if (Block_ms[b] > worst) worst = Block_ms[b];
    qsort(Block_ms + 1, (size_t)Nblocks - 1, sizeof(double), cmp);
    printf("bench masters %d pool %d create_ms %.1f device_bytes %lld first_block_ms %.3f median_block_ms %.3f worst_block_ms %.3f\n", T, pool, create_ms,
           (long long)free0 - (long long)free1, first, Block_ms[1 + (Nblocks - 1) / 2], worst);
  }
  free(in); free(out); free(th); free(tid); free(Block_ms);
  return bad;
}
