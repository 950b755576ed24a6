// ref_packetd_wrap.c -- TEST INFRASTRUCTURE: the reference's packetd.c, included unmodified where it lies (never copied), with its main()
// renamed and its one send() redirected into a capture buffer, so that decode_task() can be run over a file of samples
// (tests/test_afsk_reference.py builds this into its tmp_path together with the reference's filter.c ... ax25.c and the oracle's FFT provider).
#include <sys/types.h>
#include <sys/socket.h>
#include <sys/mman.h>
#include <fcntl.h>
#include <pthread.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

static unsigned char *Cap_buf;
static size_t Cap_size, Cap_used;
static int *Cap_lens, Cap_max, Cap_n;
static ssize_t refpkt_capture(const void *buf, size_t len) {
  if (Cap_n < Cap_max && Cap_used + len <= Cap_size) {
    memcpy(Cap_buf + Cap_used, buf, len);
    Cap_lens[Cap_n] = (int)len;
    Cap_used += len;
  }
  Cap_n++;
  return (ssize_t)len;
}

// the reference's own headers first (they are guarded), so that the macros below meet packetd.c's statements only
#include "osc.h"
#include "filter.h"
#include "misc.h"
#include "multicast.h"
#include "rtp.h"
#include "ax25.h"
#include "status.h"
#include "avahi.h"
#include <getopt.h>
#include <netdb.h>
#include <locale.h>
#include <sysexits.h>
#include <assert.h>
#include <errno.h>
#include <stdio.h>

#define main refpkt_packetd_main
#define send(fd, buf, len, flags) refpkt_capture((buf), (len))
#include "packetd.c"
#undef send
#undef main

// Bitrate is a plain file static of packetd.c (:54, 1200 unless main() parsed another): set it before a task starts.  samppbit and the filter's
// edges follow it (:496-497,509); the tones are const (:481-482).
__attribute__((visibility("default"))) void refpkt_set_bitrate(double bitrate) { Bitrate = bitrate; }

// decode_task() over the file `path` (big-endian 16-bit samples, as ntohs() at :551 reads them) for a session of `samprate`: the packets it
// "sends" (RTP header and frame) land in out[0, out_size) one behind the other, their lengths in lens[0, max_packets); returns their number.
// decode_task declares its struct filter_out uninitialised and create_filter_output() reads `init` from it, so the task runs on a thread
// whose stack is fresh zero pages (mapped here: a cached stack of an earlier thread would not be).
__attribute__((visibility("default"))) int refpkt_run(const char *path, int samprate, unsigned char *out, long out_size, int *lens, int max_packets) {
  Cap_buf = out; Cap_size = (size_t)out_size; Cap_used = 0; Cap_lens = lens; Cap_max = max_packets; Cap_n = 0;
  Verbose = 0;
  // The reference's FFT runs in this thread, not in filter.c's worker thread.  create_filter_input() names its caller the master's `owner`
  // (src/filter.c:224), and execute_filter_output() does not wait for a master that its own thread "wrote" (:681-683): with a worker thread the
  // first block of a task is gathered while -- on a busy machine, before -- the worker transforms it, from a buffer that lmalloc() did not clear.
  // With no worker threads (perform_inline, :205,562-600) the same statements run in order; the arithmetic is the same.
  N_worker_threads = 0;
  struct session *sp = calloc(1, sizeof(*sp));
  if (!sp) return -1;
  sp->samprate = samprate;
  sp->read_fd = open(path, O_RDONLY);
  if (sp->read_fd < 0) { free(sp); return -2; }
  const size_t stack = 8u << 20;
  void *mem = mmap(NULL, stack, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
  if (mem == MAP_FAILED) { close(sp->read_fd); free(sp); return -3; }
  pthread_attr_t attr;
  pthread_attr_init(&attr);
  pthread_attr_setstack(&attr, mem, stack);
  pthread_t thr;
  int rc = pthread_create(&thr, &attr, decode_task, sp);
  if (rc == 0) pthread_join(thr, NULL);                  // (decode_task closes the file at its end)
  pthread_attr_destroy(&attr);
  munmap(mem, stack);
  free(sp);
  return rc ? -4 : Cap_n;
}
