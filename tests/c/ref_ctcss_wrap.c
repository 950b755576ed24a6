// ref_ctcss_wrap.c -- TEST INFRASTRUCTURE: the reference's ctcss.c, included unmodified where it lies (never copied).  ctcss's processing is
// the body of its main(), so main is renamed and the three calls that reach the network -- setup_mcast_in(), select() and recvfrom() -- are
// redirected to a feeder that makes RTP packets from a file of samples; after every block's last packet (ten a block, or as many as the caller names:
// the packet size must divide L = lrint(0.2 samprate), and ten does not divide 2205) the feeder records what the
// session holds, and when the file ends it leaves through exit().  tests/test_ctcss_reference.py builds this as a program in its tmp_path
// together with the reference's filter.c ... rtp.c and the oracle's FFT provider.
//   ref_ctcss <samples.s16be> <samprate> <f32: 0 | 1> <records.txt> [packets per block, default 10]
#include <sys/types.h>
#include <sys/socket.h>
#include <sys/select.h>
#include <stdbool.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

static int refctcss_select(fd_set *readfds);
static ssize_t refctcss_recvfrom(void *buf, size_t len, struct sockaddr *from, socklen_t *fromlen);
#define REFCTCSS_FD 3

// the reference's own headers first (they are guarded), so that the macros below meet ctcss.c's statements only
#include "filter.h"
#include "misc.h"
#include "multicast.h"
#include "rtp.h"
#include "osc.h"
#include <assert.h>
#include <errno.h>
#include <complex.h>
#include <math.h>
#include <limits.h>
#include <locale.h>
#include <signal.h>
#include <getopt.h>
#include <sysexits.h>

#define main refctcss_main
#define setup_mcast_in(source, source_sock, target, sock, offset, tries) (REFCTCSS_FD)
#define select(nfds, readfds, writefds, exceptfds, timeout) refctcss_select((readfds))
#define recvfrom(fd, buf, len, flags, from, fromlen) refctcss_recvfrom((buf), (len), (from), (fromlen))
#include "ctcss.c"
#undef recvfrom
#undef select
#undef setup_mcast_in
#undef main

// what ctcss.c takes from multicast.c
char const *Default_mcast_iface;
char const *formatsock(void const *s, bool full) { (void)s; (void)full; return "feeder"; }
int address_match(void const *a, void const *b) { (void)a; (void)b; return 1; }

void oracle_fft_set_precision(int f32);

static FILE *In, *Out;
static int Samprate, Per_packet, Type, Per_block = 10;
static long Packets;
static uint16_t Seq;
static uint32_t Timestamp;

// before every packet: after each block's last one the session has just finished a block (put_rfilter() completed on the packet's last sample)
static int refctcss_select(fd_set *readfds) {
  if (Packets > 0 && Packets % Per_block == 0 && Sessions)
    fprintf(Out, "%d %.17g %.17g\n", Sessions->strongest_tone_index, Sessions->strongest_tone_energy, Sessions->current_pl_tone);
  if (Packets % Per_block == 0) {                          // leave at a block edge when less than a whole block is left
    const long at = ftell(In);
    fseek(In, 0, SEEK_END);
    const long left = ftell(In) - at;
    fseek(In, at, SEEK_SET);
    if (left < (long)Per_block * Per_packet * (long)sizeof(int16_t)) { fclose(Out); exit(0); }
  }
  FD_ZERO(readfds);
  FD_SET(REFCTCSS_FD, readfds);
  return 1;
}
static ssize_t refctcss_recvfrom(void *buf, size_t len, struct sockaddr *from, socklen_t *fromlen) {
  struct rtp_header rtp;
  memset(&rtp, 0, sizeof rtp);
  rtp.version = 2; rtp.type = (uint8_t)Type; rtp.seq = Seq++; rtp.timestamp = Timestamp; rtp.ssrc = 4711;
  uint8_t *dp = hton_rtp(buf, &rtp);
  const size_t bytes = (size_t)Per_packet * sizeof(int16_t);
  if ((size_t)(dp - (uint8_t *)buf) + bytes > len || fread(dp, 1, bytes, In) != bytes) { fclose(Out); exit(3); }
  Timestamp += (uint32_t)Per_packet;
  Packets++;
  memset(from, 0, sizeof *from);
  from->sa_family = AF_INET;
  *fromlen = sizeof *from;
  return (ssize_t)((dp - (uint8_t *)buf) + bytes);
}

int main(int argc, char *argv[]) {
  if (argc != 5 && argc != 6) return 2;
  In = fopen(argv[1], "rb");
  Samprate = atoi(argv[2]);
  oracle_fft_set_precision(atoi(argv[3]));
  Out = fopen(argv[4], "w");
  if (!In || !Out || Samprate <= 0) return 2;
  if (argc == 6) Per_block = atoi(argv[5]);
  const int block = (int)lrint(Filter_time * Samprate);
  if (Per_block < 1 || block % Per_block) return 2;
  Per_packet = block / Per_block;                                // a tenth of a block by default: 480 samples at 24 kHz, as a 20 ms packet carries
  Type = pt_from_info(Samprate, 1, S16BE);
  if (Type < 0) return 2;
  // the reference's FFT runs in the caller's thread: with filter.c's worker thread the first block of a master is gathered without waiting for
  // its transform (tests/c/ref_packetd_wrap.c has the details)
  N_worker_threads = 0;
  char *args[] = {"ctcss", "feeder", NULL};
  return refctcss_main(2, args);
}
