// ref_rdsd_wrap.c -- TEST INFRASTRUCTURE: the reference's rdsd.c, included unmodified where it lies (never copied), wrapped as
// tests/c/ref_stereod_wrap.c wraps stereod.c: main renamed (and never called), the one sendto() redirected to a recorder,
// pthread_cond_timedwait() answering ETIMEDOUT, pthread_detach() a no-op; a session with the whole input queued as RTP packets of 384
// samples; decode() on a thread whose stack is fresh zero pages (it declares its struct filter_outs uninitialised).  rdsd's Blocktime is a
// constant, 5 ms.  tests/test_mpx_reference.py builds this as a program in its tmp_path.
//   ref_rdsd <samples.s16be> <f32: 0 | 1> <pcm out>
// pcm out: every packet's payload, one behind the other.  The time decode() took per block, from the first packet sent to the last, goes
// to stdout.
#include <sys/types.h>
#include <sys/socket.h>
#include <sys/mman.h>
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <unistd.h>

static ssize_t refmpx_record(const void *buf, size_t len);

// the reference's own headers first (they are guarded), so that the macros below meet rdsd.c's statements only
#include "misc.h"
#include "multicast.h"
#include "rtp.h"
#include "status.h"
#include "filter.h"
#include "iir.h"
#include "avahi.h"
#include <assert.h>
#include <errno.h>
#include <complex.h>
#include <math.h>
#include <limits.h>
#include <netdb.h>
#include <locale.h>
#include <sys/time.h>
#include <sys/resource.h>
#include <signal.h>
#include <getopt.h>
#include <sysexits.h>

#define main refmpx_rdsd_main
#define sendto(fd, buf, len, flags, to, tolen) refmpx_record((buf), (len))
#define pthread_cond_timedwait(cond, mutex, abstime) (ETIMEDOUT)
#define pthread_detach(thread) (0)
#include "rdsd.c"
#undef pthread_detach
#undef pthread_cond_timedwait
#undef sendto
#undef main

void oracle_fft_set_precision(int f32);

static FILE *Pcm;
static struct session *Sess;
static long Blocks;
static struct timespec First, Last;

// the session's packet as decode() sends it: an RTP header without extensions (12 bytes), then audio_L pairs of big-endian samples
static ssize_t refmpx_record(const void *buf, size_t len) {
  if (len <= RTP_MIN_SIZE) return -1;
  fwrite((const uint8_t *)buf + RTP_MIN_SIZE, 1, len - RTP_MIN_SIZE, Pcm);
  clock_gettime(CLOCK_MONOTONIC, &Last);
  if (Blocks++ == 0) First = Last;
  return (ssize_t)len;
}

int main(int argc, char *argv[]) {
  if (argc != 4) return 2;
  FILE *in = fopen(argv[1], "rb");
  oracle_fft_set_precision(atoi(argv[2]));
  Pcm = fopen(argv[3], "wb");
  if (!in || !Pcm) return 2;
  // the reference's FFT runs in the caller's thread: with filter.c's worker thread the first block of a master is gathered without waiting for
  // its transform (tests/c/ref_packetd_wrap.c has the details)
  N_worker_threads = 0;
  const int type = pt_from_info(In_samprate, 1, S16BE);
  if (type < 0) return 2;
  Sess = create_session();
  Sess->rtp_state_out.ssrc = Sess->rtp_state_in.ssrc = 4711;
  enum { PER_PACKET = 384 };
  uint16_t seq = 0;
  uint32_t timestamp = 0;
  struct packet **tail = &Sess->queue;
  for (;;) {
    struct packet *pkt = malloc(sizeof *pkt);
    if (!pkt) return 3;
    if (fread(pkt->content, sizeof(int16_t), PER_PACKET, in) != PER_PACKET) { free(pkt); break; }
    memset(&pkt->rtp, 0, sizeof pkt->rtp);
    pkt->rtp.version = RTP_VERS; pkt->rtp.type = (uint8_t)type; pkt->rtp.seq = seq++; pkt->rtp.timestamp = timestamp; pkt->rtp.ssrc = 4711;
    timestamp += PER_PACKET;
    pkt->data = pkt->content; pkt->len = PER_PACKET * sizeof(int16_t); pkt->next = NULL;
    *tail = pkt; tail = &pkt->next;
  }
  fclose(in);
  const size_t stack = 8u << 20;
  void *mem = mmap(NULL, stack, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
  if (mem == MAP_FAILED) return 3;
  pthread_attr_t attr;
  pthread_attr_init(&attr);
  pthread_attr_setstack(&attr, mem, stack);
  pthread_t thr;
  if (pthread_create(&thr, &attr, decode, Sess) != 0) return 4;
  pthread_join(thr, NULL);                                                // (decode() has closed and freed the session)
  pthread_attr_destroy(&attr);
  munmap(mem, stack);
  fclose(Pcm);
  if (Blocks > 1)                                                         // from the first packet sent to the last: filter set-up stays out
    printf("%ld blocks, %.2f us a block\n", Blocks, ((Last.tv_sec - First.tv_sec) * 1e6 + (Last.tv_nsec - First.tv_nsec) * 1e-3) / (Blocks - 1));
  return 0;
}
