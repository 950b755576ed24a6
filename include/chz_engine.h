/* chz_engine.h -- C ABI of the MI355X overlap-save channelizer engine
 * (libchz_hip.so, built from ka9q-radio_amd/csrc/chz_engine.hip).
 *
 * Plain pointers and sizes only; no torch, no C++ types.  This is the layer a
 * foreign host (C, ctypes, cgo ...) binds.  Each entry point states which piece
 * of the reference's filter.c it replaces; the struct-compatible drop-in for the
 * reference's own filter.h (create_filter_input & co.) is layered on top of it in
 * ka9q-radio_amd/csrc/filter_hip.c and declared in include/ka9q_filter_abi.h.
 *
 * All functions return 0 on success and a negative value on error (the message
 * is available from chz_last_error()); there is NO CPU fallback: without a HIP
 * device chz_engine_create() fails.
 *
 * Sample/stream conventions are the reference's: blocks of L new samples, impulse
 * length M, N = L+M-1 point transform, window k = stream[kL-(M-1), kL+L) with
 * zeros before time 0 (src/filter.c:196,244,259); unnormalised transforms both ways
 * with all gain folded into the per-channel response (src/filter.c:1020-1028);
 * ND = 4 spectrum slots indexed job % 4 (src/filter.h:48).
 */
#ifndef CHZ_ENGINE_H
#define CHZ_ENGINE_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define CHZ_COMPLEX 1   /* enum filtertype COMPLEX, src/filter.h:31 */
#define CHZ_REAL    2   /* enum filtertype REAL,    src/filter.h:32 */
#define CHZ_ND      4   /* spectrum slots,          src/filter.h:48 */

typedef struct chz_engine chz_engine;

typedef struct chz_info {
  int L, M, N, in_type, bins;
  int ring_blocks;          /* device input ring holds ring_blocks*L samples */
  int Na, Nb, Nc;           /* axis lengths of the forward transform */
  int n_banks;
  int lanes;                /* HIP streams blocks are pipelined over */
  /* device storage order of a spectrum slot: bin k at [(k / spec_na) * spec_pitch + spec_off + k % spec_na];
   * natural order when spec_pitch == spec_na and spec_off == 0.  chz_spectrum_read returns natural
   * order; code that touches the device buffer directly (chz_spectrum_device / _attach, e.g. an RCCL
   * broadcast) must treat it as spec_elems opaque complex values. */
  long spec_elems;
  int spec_na, spec_pitch, spec_off;
  char plan[320];           /* human-readable plan description */
} chz_info;

typedef struct chz_timing {
  double total_ms;          /* HIP-event time of the whole run on the engine's stream */
  int blocks;
  /* per-kernel HIP-event time, accumulated over the run (only when instrumented) */
  double first_ms, cols_ms, rows_ms, notch_ms, chan_ms;   /* notch_ms/notch_n: the noise-estimate kernel (the spur notch is fused into fwd_rows) */
  int first_n, cols_n, rows_n, notch_n, chan_n;
  double enqueue_ms;        /* host wall time spent issuing the launches (close to total_ms = host-bound) */
  double fix_ms; int fix_n; /* the spur-notch kernel (notch_fix) */
  double demod_ms; int demod_n; /* the linear demodulator kernel */
} chz_timing;

const char *chz_last_error(void);
/* 1 once the process has begun to exit (exit() called: radiod's closedown(), src/main.c): the library has stopped issuing work to the HIP runtime, whose own exit
 * handlers are about to tear it down, and every call reports -98 from then on -- not a device failure, nothing to recover (round 6) */
int chz_process_exiting(void);
/* Options (round 6): dispatch thresholds and test hooks, process-wide, read when an engine / communicator is CREATED.  The shipped
 * library reads only the operator's environment variables; everything a test or an A/B script used to set
 * through CHZ_* variables is set here instead.  value NULL or "" = back to the default.  Names: chan_stage, noise_energy, demod_wave
 * (-1 auto / 0 / 1), enq_threads (1|2|4), graph_blocks, notch_fold (0|1), noise_hint (0|1), pll_lane0 (0|1), notch_wait_ms,
 * fault_ticket_skew + allow_fault_injection (recovery-path tests), launch_id (chz_comm_create_file).  < 0: unknown name. */
int chz_set_option(const char *name, const char *value);
int chz_device_count(void);

/* replaces create_filter_input (src/filter.c:186-269): allocates the device input
 * ring (zeroed, write position M-1 ahead of the read position), the ND spectrum
 * slots and the transform plan ("" / NULL = automatic, or "NaxNbxNc[:T1,T2,Ta]"). */
int chz_engine_create(chz_engine **out, int L, int M, int in_type, int device,
                      const char *plan_spec, int ring_blocks);
/* replaces delete_filter_input (src/filter.c:930-942) */
void chz_engine_destroy(chz_engine *e);
int chz_engine_info(const chz_engine *e, chz_info *info);
/* run all engine work on a caller-owned hipStream_t (e.g. torch's current stream) */
int chz_engine_set_stream(chz_engine *e, void *hip_stream);
int chz_sync(chz_engine *e);
/* non-blocking health check: < 0 (and chz_last_error) once a device-side consistency check has failed -- today that is
 * the spur-notch ticket (see chz_set_notches_alpha); chz_sync and chz_run_blocks report the same condition */
int chz_engine_check(const chz_engine *e);

/* replaces the sample hand-over of write_rfilter/write_cfilter
 * (src/filter.c:1093-1134): append n samples (floats; re,im pairs for COMPLEX) from
 * host memory at the ring's write position. */
int chz_input_write(chz_engine *e, const float *host_samples, long n);
/* same, but the samples already live in device memory */
int chz_input_write_device(chz_engine *e, const float *dev_samples, long n);
/* SURVEY 8(f) rank 3 -- raw A/D samples: replaces rx888.c's convert() + write_rfilter(.., NULL, n)
 * (src/rx888.c:753-767,800-829).  The int16 samples go to HBM as they are (half the PCIe bytes, half the
 * first pass's reads); x -> (float)x * scale, the LTC2208 de-randomiser (randomize != 0: if bit 0 is set,
 * flip bits 1..15, src/rx888.c:711-716) and the per-block statistics happen where the first transform
 * pass loads the samples.  REAL masters only; an engine takes either float or int16 input, not both. */
int chz_input_write_i16(chz_engine *e, const short *host_samples, long n, float scale, int randomize);
int chz_input_write_i16_device(chz_engine *e, const short *dev_samples, long n, float scale, int randomize);
/* sum of x*x and count of |x| > 32766 over the L new samples of the block last transformed into `slot`
 * (what rx_callback accumulates into frontend->if_power / overranges, src/rx888.c:780-795); synchronous */
int chz_input_stats(chz_engine *e, int slot, unsigned long long *energy, unsigned *clips);
/* The other front ends' raw A/D formats: replaces the per-sample conversion loops of airspy.c:412-427 + airspy-unpack.c, the switch of
 * hydrasdr.c:660-833 and rtlsdr.c:323-339.  The raw bytes cross the link (1.5 bytes a sample PACKED12, 2 a complex sample 8-bit I/Q) into
 * a device staging buffer -- allocated by an engine's first raw write, freed with the engine -- and the raw_unpack kernel converts them
 * into the FLOAT input ring at the write position, so everything behind the ring is what it is for chz_input_write, and the two may
 * alternate on one engine.  (An engine in int16 mode, chz_input_write_i16, refuses raw writes, and the other way round.)
 *   n        samples; complex samples for the I/Q formats.  PACKED12: a multiple of 8
 *   bits     CHZ_RAW_U16 only, 2..16: frontend->bitspersample
 *   scale    sdr->scale.  x -> (float)(scale * x), the product in double; PACKED12 -> (float)scale * (float)x, the product in float, as
 *            airspy_unpack() does, which is handed (float)sdr->scale
 *   ticket   out (may be NULL): this write's number, counted per engine from 0; the statistics of the last CHZ_RAW_TICKETS writes can be read
 * chz_input_raw_stats: the exact sum of x*x (x*x + y*y) over the write, the samples the reference counts into frontend->overranges (PACKED12
 * x == 2047 || x <= -2047; U16 x >= offset-1 || x <= -offset; 16-bit >= 32767 || <= -32768; 8-bit >= 127 || <= -128; an I/Q sample once if
 * either component clips) and the clipped components one by one (what rtlsdr.c:324-334 adds up; == clipped_samples for REAL formats).
 * Synchronous on the engine's stream, like chz_input_stats.  Any of the three pointers may be NULL.
 * The _device form reads the caller's device buffer in place: 16-byte aligned, and readable up to the next 16-byte boundary behind the
 * last sample (the kernel loads whole 8- or 16-byte groups and masks what lies beyond n). */
#define CHZ_RAW_PACKED12 0   /* REAL: 8 samples in 3 little-endian 32-bit words, offset 2048 (airspy-unpack.c; hydrasdr RAW) */
#define CHZ_RAW_U16      1   /* REAL: uint16, offset 1 << (bits-1)      (hydrasdr.c:681-698) */
#define CHZ_RAW_S16      2   /* REAL: int16                             (:700-715) */
#define CHZ_RAW_U8       3   /* REAL: uint8, offset 128                 (:759-774) */
#define CHZ_RAW_S8       4   /* REAL: int8                              (:776-791) */
#define CHZ_RAW_S16_IQ   5   /* COMPLEX: int16 I,Q                      (:729-746) */
#define CHZ_RAW_U8_IQ    6   /* COMPLEX: uint8 I,Q, offset 128          (:793-810; rtlsdr.c:323-339) */
#define CHZ_RAW_S8_IQ    7   /* COMPLEX: int8 I,Q                       (:812-829) */
#define CHZ_RAW_TICKETS  8   /* the statistics of this many latest raw writes stay readable */
int chz_input_raw_check(int in_type, int format, int bits, long n);   /* 0, or < 0 and chz_last_error(); touches no device */
int chz_input_write_raw(chz_engine *e, int format, int bits, const void *host_samples, long n, double scale, unsigned *ticket);
int chz_input_write_raw_device(chz_engine *e, int format, int bits, const void *dev_samples, long n, double scale, unsigned *ticket);
int chz_input_raw_stats(chz_engine *e, unsigned ticket, unsigned long long *energy, unsigned *clipped_samples, unsigned *clipped_components);
/* The synthetic front end: sig_gen's sample law (src/sig_gen.c:291-296 REAL, :321-326 COMPLEX; oscillator src/osc.c:28-70, popcount
 * Gaussian over xoshiro256** src/gauss.c:47-61,95-111) generated on the device straight into the FLOAT ring, so that no samples cross
 * the link, the input never repeats and every device of a sharded run can make the identical stream by itself.  Sample n of the stream
 * (0 <= n < 2^53) depends only on the parameters and n:
 *   REAL     (float)((amplitude cos(2 pi phi_n) + noise g_n) scale)
 *   COMPLEX  two draws a sample, the real part's first, added to amplitude cis(2 pi phi_n); the ring holds re, im
 *   phi_n    frac(a n), a the angle of the reference's step phasor for set_osc's argument freq (cycles/sample), the product exact
 *   g_j      the popcount Gaussian of the generator's j-th output; the generator is seeded as xoshiro256ss_seed seeds it (the
 *            reference always uses seed 1)
 * The noise term is the reference's bit for bit.  The carrier is the closed form, evaluated in double at the first sample of every run of
 * CHZ_SIGGEN_RUN ring floats and rotated from there: the reference's recurrence rounds differently, by up to 1e-10 of the amplitude within
 * 2^18 samples (a float sample differs by one unit in the last place now and then).
 * chz_input_siggen_set describes the whole stream and puts the position at sample 0 (set on a running stream restarts it: a change of
 * parameters with phase continuity is not offered, as sig_gen_tune is not in the reference); _seek / _tell move and read the position.
 * chz_input_generate appends the next n samples at the ring's write position: a ring write like chz_input_write, with which (and with
 * chz_input_write_raw) it may alternate on one engine; per call the host advances the generator by one O(1) jump, everything per sample
 * and per lane happens in the kernel (siggen_fill).  n == 0 is a valid, empty generate.  Refused (-1, nothing enqueued, nothing advanced):
 * no stream described, an engine in int16 mode, n < 0, n beyond the ring, a position that would pass 2^53, non-finite parameters.
 *   ticket   out (may be NULL): this generate's number, counted per engine from 0
 * chz_input_generate_stats: the sum of samp^2 (re^2 + im^2) over the generate, samp the value BEFORE scale (in_energy of sig_gen.c), added
 * in double in a fixed order (two runs give the same bits); the last CHZ_RAW_TICKETS generates' can be read.  Synchronous on the
 * engine's stream.
 * chz_siggen_check / _seed / _jump touch no device: would these parameters be taken; the seeded generator state; state <- T^draws state
 * for draws = draws_hi 2^64 + draws_lo (T the generator's update, which is linear over GF(2)). */
#define CHZ_SIGGEN_RUN 64    /* ring floats one lane of the kernel produces from its own generator state */
typedef struct { double freq, amplitude, noise, scale; unsigned long long seed; } chz_siggen_params;
int chz_siggen_check(int in_type, const chz_siggen_params *p);
int chz_siggen_jump(unsigned long long state[4], unsigned long long draws_lo, unsigned long long draws_hi);
int chz_siggen_seed(unsigned long long seed, unsigned long long state[4]);
int chz_input_siggen_set(chz_engine *e, const chz_siggen_params *p);
int chz_input_siggen_seek(chz_engine *e, unsigned long long sample);
int chz_input_siggen_tell(chz_engine *e, unsigned long long *sample);
int chz_input_generate(chz_engine *e, long n, unsigned *ticket);
int chz_input_generate_stats(chz_engine *e, unsigned ticket, double *energy);
/* direct access to the device ring for HBM-resident benchmarks */
int chz_input_ring(chz_engine *e, float **dev_ring, long *ring_len_floats);
/* Re-seat the input ring in front of block `job`: the next L samples written are that block's new samples and `history`
 * (M-1 samples from host memory; NULL = zeros, the state create_filter_input leaves, src/filter.c:244,259) is what came
 * before them.  A freshly created engine sits in front of job 0; a host that REPLACES an engine in mid-stream (the drop-in's
 * recovery from a failed device-side check: the reference exits and lets systemd restart it, src/radio.c:398, src/main.c:202)
 * continues its job numbering and its overlap history with this.  Drains the engine.  Float input only. */
int chz_input_seek(chz_engine *e, unsigned job, const float *history);
/* Fences for a producer that does not wait for blocks (the drop-in's KA9Q_HIP_INPUT_FULL=drop): chz_input_mark(e, k) records
 * marker k (0..7) behind everything chz_input_write has enqueued so far, chz_input_mark_wait(e, k) blocks until the copies in
 * front of marker k have read their host source (so that the host ring region may be overwritten); a marker never recorded
 * is complete. */
int chz_input_mark(chz_engine *e, int k);
int chz_input_mark_wait(chz_engine *e, int k);
/* by_event != 0: order the spur-notch recurrence by HIP events between the streams instead of the device ticket (what env
 * CHZ_NOTCH_ORDER=event selects at creation): no device-side wait that could run out.  Drains the engine. */
int chz_engine_notch_order(chz_engine *e, int by_event);

/* replaces the body of execute_filter_input / run_fft (src/filter.c:485-651):
 * forward transform of the window of job `job` (window start = job*L in ring
 * coordinates) into slot job % 4, then the spur notches. */
int chz_forward(chz_engine *e, unsigned job);
/* notch list as radio.c builds it (src/radio.c:601-620): last entry is bin 0;
 * replaces apply_notch_filters' state (src/filter.c:464-474).  n = 0 clears. */
int chz_set_notches(chz_engine *e, const int *bins, int n, double alpha);
/* the same with one averager gain per entry, as struct notch_state carries it (src/filter.h:42-46, src/filter.c:468);
 * an entry with alpha = 0 is the reference's no-op.  The recurrence over blocks is ordered by a ticket the tiny notch
 * kernels take in block order (bounded wait, loud failure, never a wrong state: chz_engine_check), or -- env
 * CHZ_NOTCH_ORDER=event, and always inside captured graphs -- by HIP events between the engine's streams. */
int chz_set_notches_alpha(chz_engine *e, const int *bins, const double *alpha, int n);
int chz_spectrum_read(chz_engine *e, int slot, float *host);     /* 2*bins floats, synchronous */
int chz_spectrum_device(chz_engine *e, int slot, float **dev);
/* the hipStream_t everything addressed by `slot` is enqueued on; lets a caller order foreign work
 * (an RCCL collective on the slot's spectrum) between chz_forward(job) and chz_bank_execute(.., slot) */
int chz_slot_stream(chz_engine *e, int slot, void **hip_stream);
/* point a slot at caller-owned device memory (2*spec_elems floats, see chz_info), e.g. a torch
 * tensor that RCCL broadcasts into */
int chz_spectrum_attach(chz_engine *e, int slot, float *dev);

/* A bank = all channels sharing one (P, olen); replaces create_filter_output's
 * allocations (src/filter.c:298-415) for COMPLEX output channels. */
int chz_bank_create(chz_engine *e, int P, int olen, int capacity);          /* returns bank id */
/* the same for REAL-output slaves (create_filter_output(.., REAL), src/filter.c:372-395; gather :794-809, c2r :914):
 * responses are still P complex values per channel (set_filter's array, of which bins 0..P/2 are used), outputs are
 * olen floats per channel; P must be even */
int chz_bank_create_real(chz_engine *e, int P, int olen, int capacity);
/* Channels with the same filter sharing its response: `nrows` response rows in the bank, every channel names the row it reads
 * (chz_bank_set_rows: takes effect like a retune, in stream order, no drain), rows are written by chz_bank_set_row_responses (between
 * blocks: drains).  The reference keeps one copy per slave (src/filter.c:1039-1043); the values are the same, the HBM traffic per
 * channel and block drops from 8P + 8*olen to 8*olen bytes.  chz_bank_set_responses is refused on such a bank. */
int chz_bank_create_shared(chz_engine *e, int P, int olen, int capacity, int nrows);
int chz_bank_set_rows(chz_engine *e, int bank, int ch0, int n, const int *rows);
int chz_bank_set_row_responses(chz_engine *e, int bank, int row0, int n, const float *resp);
/* None of the per-channel setters below waits for blocks in flight: shifts, tuning, ISB flags and beam weights live in
 * small descriptors kept once per spectrum slot and refreshed in stream order when the next block of that slot is
 * enqueued (blocks already enqueued keep what they were launched with); a response is written to a spare row and the
 * channel re-pointed, the old row being recycled once everything enqueued before the swap has drained.  Only edits of
 * more than 8192 channels at once (a bank being set up) and the first use of a feature that switches the kernel
 * variant (tuning, ISB, beam, noise) drain the engine. */
/* response[P] complex as set_filter leaves it (src/filter.c:968-1045) */
int chz_bank_set_responses(chz_engine *e, int bank, int ch0, int n, const float *resp);
/* `shift` of execute_filter_output(slave, shift) (src/filter.c:663).  A channel has NO gather descriptor until this (or
 * chz_bank_set_tuning) has been called for it -- shift 0 included -- and produces zeros until then. */
int chz_bank_set_shifts(chz_engine *e, int bank, int ch0, int n, const int *shifts);
/* slave->isb (src/filter.c:895-909, filter2 of the linear demodulator in ISB mode): LSB and USB are unpacked to I and Q
 * after the gather.  One flag byte per channel, non-zero = on.  COMPLEX-output banks only. */
int chz_bank_set_isb(chz_engine *e, int bank, int ch0, int n, const unsigned char *flags);
/* slave->beam (src/filter.c:756-775; set by radio.c:938-940): two antennas on I and Q of a COMPLEX master are selected or
 * combined with the weights set_filter_weights left in slave->alpha / ->beta.  ab = 4 doubles per channel (Re alpha,
 * Im alpha, Re beta, Im beta), on = one flag byte per channel.  Bins past the end of the master walk are zero (the
 * reference leaves them unwritten). */
int chz_bank_set_beam(chz_engine *e, int bank, int ch0, int n, const double *ab, const unsigned char *on);
int chz_bank_set_active(chz_engine *e, int bank, int n);                    /* channels [0,n) run */
/* replaces execute_filter_output's gather x response + backward transform
 * (src/filter.c:728-914) for every active channel of the bank at once */
/* the bank runs on the spectrum of block `job` (slot job % 4); for a bank without tuning only the slot
 * matters, so passing a slot number 0..3 is equivalent */
int chz_bank_execute(chz_engine *e, int bank, unsigned job);
/* the same for channels [ch0, ch0+n) only: the slow path of one retuned channel.  ALWAYS a partial re-run of a block the bank has
 * already seen -- whatever the range, including a bank of exactly one channel: the bank's demodulators are not stepped and the
 * block's PCM is left alone (only chz_bank_execute / chz_step / chz_run_blocks are "the block") */
int chz_bank_execute_range(chz_engine *e, int bank, unsigned job, int ch0, int n);

/* SURVEY 8(f) rank 1 -- the tail of radiod's downconvert() fused into the channel kernel's epilogue
 * (src/radio.c:1476-1520): every output sample is multiplied by the channel's fine-tuning rotator
 * (set_osc/step_osc, src/osc.c:28-70) including the per-block phase_adjust for bin shifts that are not a
 * multiple of the overlap factor V = 1 + L/(M-1) and the one-time phase kick on a shift change, and the
 * block's mean |sample|^2 (chan->sig.bb_power) is left in a per-slot array.
 *   shifts[i]  as for chz_bank_set_shifts (this call replaces it for tuned channels)
 *   freq[i]    cycles per OUTPUT sample, = -remainder / output samprate   (first argument of set_osc)
 *   rate[i]    cycles per sample^2,       = doppler_rate / samprate^2     (second argument; NULL = 0)
 * The update takes effect at block `job`, which must not have been enqueued yet; call it when shift,
 * remainder or sweep rate change (it does not wait for the engine), not every block.  The rotation is a closed
 * form in the block number, so tuned banks run eagerly (chz_run_blocks mode 0), any number in flight. */
int chz_bank_set_tuning(chz_engine *e, int bank, unsigned job, int ch0, int n, const int *shifts,
                        const double *freq, const double *rate);
int chz_bank_read_power(chz_engine *e, int bank, int slot, int ch0, int n, double *host);        /* synchronous */
int chz_bank_read_power_async(chz_engine *e, int bank, int slot, int ch0, int n, double *host);

/* SURVEY 8(f) rank 2 -- estimate_noise() (src/radio.c:1783-1866) on the device, run for every channel of
 * the bank right after its channel kernel: energies of max(P, 1000) master bins around |shift|, their 0.10
 * quantile, the mean of the energies below 1.5 x that, bias correction, per Hz.  It is the one reader of
 * the whole block spectrum outside filter.c (src/radio.c:1787-1836): with it on the device the 13 MB
 * spectrum no longer has to travel to the host every block.  samprate = front-end sample rate (Hz), 0 = off.
 * The exponential smoothing of chan->sig.n0 (src/radio.c:1466-1473) stays with the caller. */
int chz_bank_enable_noise(chz_engine *e, int bank, double samprate);
int chz_bank_read_noise(chz_engine *e, int bank, int slot, int ch0, int n, double *host);        /* synchronous */
int chz_bank_read_noise_async(chz_engine *e, int bank, int slot, int ch0, int n, double *host);
int chz_bank_destroy(chz_engine *e, int bank);                              /* frees the bank's device arrays */
int chz_bank_read(chz_engine *e, int bank, int ch0, int n, float *host);    /* n*olen complex (REAL banks: n*olen floats) of the most recent execute, synchronous */
/* Blocks are pipelined over 1, 2 or 4 HIP streams ("lanes", env CHZ_STREAMS, default 4): block j
 * runs on lane j % lanes with its own intermediate buffer, so block j+1's forward transform overlaps
 * block j's tail.  Bank outputs exist once per spectrum slot.  Everything addressed by `slot` below is
 * enqueued on the lane that owns that slot, in call order.
 * Asynchronous device-to-host copies (host memory should come from chz_host_alloc); completion is
 * observed through chz_host_callback or chz_sync */
int chz_bank_read_async(chz_engine *e, int bank, int slot, int ch0, int n, float *host);
int chz_spectrum_read_async(chz_engine *e, int slot, float *host);
/* run fn(arg) on a runtime thread once everything enqueued so far on `slot`'s lane has finished: replaces
 * run_fft's completion broadcast (src/filter.c:522-539) */
int chz_host_callback(chz_engine *e, int slot, void (*fn)(void *), void *arg);
/* wait for everything enqueued on `slot`'s lane only (the other lanes keep running) */
int chz_slot_sync(chz_engine *e, int slot);
/* page-locked host memory for the buffers the device copies into */
int chz_host_alloc(void **p, size_t bytes);
void chz_host_free(void *p);
/* page-lock memory the caller already owns (the mirrored host input ring) so chz_input_write DMAs
 * straight out of it; failure is not fatal, copies then go through the runtime's staging buffer */
int chz_host_register(void *p, size_t bytes);
void chz_host_unregister(void *p);
int chz_bank_output_device(chz_engine *e, int bank, int slot, float **dev);

/* one whole block: chz_forward(job) then every bank on slot job % 4 */
int chz_step(chz_engine *e, unsigned job);

/* Run `nblocks` consecutive blocks starting at `job0` and time them with HIP
 * events on the engine's stream.
 *   mode 0: eager launches          mode 1: one hipGraph per ring cycle, replayed
 *   instrument != 0 (eager only): HIP events around every kernel -> per-kernel ms */
int chz_run_blocks(chz_engine *e, unsigned job0, int nblocks, int mode, int instrument,
                   chz_timing *timing);

/* ---- multi-GPU (north_star: "the forward spectrum is RCCL-broadcast over xGMI and each GPU owns a disjoint
 * channel subset, overlapped with the next block's forward FFT on a second HIP stream").  One process per GPU and one
 * communicator per process; the reference has no counterpart (thread per channel in one process).  RCCL is bound at
 * run time.  Rank 0 obtains an id and ships its CHZ_COMM_ID_BYTES bytes to the peers by any means (or all ranks meet
 * through a file with chz_comm_create_file). */
#define CHZ_COMM_ID_BYTES 128
typedef struct chz_comm chz_comm;
int chz_comm_unique_id(void *id128);
int chz_comm_create(chz_comm **out, int rank, int world, const void *id128, int device);
int chz_comm_create_file(chz_comm **out, int rank, int world, const char *path, int device, double timeout_s);
/* ONE process, several devices (the filter.h drop-in's KA9Q_HIP_DEVICES with KA9Q_HIP_EXCHANGE=broadcast): a clique of n communicators
 * (ncclCommInitAll), out[i] on devices[i]; every device at most once.  chz_spectrum_broadcast_local sends slot `slot` of engines[root]
 * into the same slot of the other engines -- engines[i] created on devices[i], comms from one chz_comm_create_local call -- as one
 * grouped call, each part on its engine's slot stream.  Each communicator is released with chz_comm_destroy. */
int chz_comm_create_local(chz_comm **out, int n, const int *devices);
int chz_spectrum_broadcast_local(chz_engine *const *engines, chz_comm *const *comms, int n, int slot, int root);
void chz_comm_destroy(chz_comm *c);
int chz_comm_rank(const chz_comm *c);
int chz_comm_world(const chz_comm *c);
int chz_comm_barrier(chz_comm *c);
int chz_comm_allreduce_max(chz_comm *c, double *v, int n);           /* n <= 64, blocking: control plane only */
/* ncclBroadcast of spectrum slot `slot` (all spec_elems complex values) from `root`, enqueued on the slot's stream:
 * behind chz_forward(job) on the root, in front of chz_bank_execute(.., job) everywhere */
int chz_spectrum_broadcast(chz_engine *e, chz_comm *c, int slot, int root);
/* sub-band variant: rank r receives only spectrum rows [row_lo[r], row_hi[r]) (row = spec_pitch complex values),
 * one grouped ncclSend/ncclRecv */
int chz_spectrum_exchange_rows(chz_engine *e, chz_comm *c, int slot, int root, const int *row_lo, const int *row_hi);
/* BASELINE config 4 from a C host: per block the root transforms, the spectrum travels (mode 0 broadcast, 1 rows),
 * every rank runs its own banks; timed like chz_run_blocks.  mode 2 (SURVEY 8e's alternative): the block's L new samples
 * travel from the root's input ring into every rank's ring (ncclBroadcast on the communicator's own stream: 10.4 MB instead of
 * the 13.8 MB slot at 129.6 MS/s) and every rank runs the forward transform itself -- nobody waits for the root's transform; with the
 * run's first block the M-1 samples of overlap history in front of it travel too, so every rank's spectra (and notch states) equal the root's */
int chz_run_blocks_sharded(chz_engine *e, chz_comm *c, int root, int mode, const int *row_lo, const int *row_hi,
                           unsigned job0, int nblocks, chz_timing *timing);

/* ---- SURVEY 8(f) rank 4 -- the linear and FM demodulators behind the fine-tuned channel outputs (demod_linear,
 * src/linear.c:56-375; demod_fm, src/fm.c:19-345): the PLL of the coherent modes with its lock detector, noise smoothing
 * (src/radio.c:1466-1473), post-detection shift oscillator, block AGC, the final demodulation pass with its per-sample gain
 * ramp, the squelch sequencers; FM's SNR estimators, discriminator or PLL demodulator, PL-tone squelch, de-emphasis; and PCM
 * packing (src/import.h:88-118 and G.711, src/rtp.c:459-533, via send_output, src/audio.c:117-133).  Runs for every channel of a COMPLEX-output bank that has tuning (chz_bank_set_tuning:
 * bb_power) and the noise estimate (chz_bank_enable_noise) switched on, in block order on a stream of its own behind the
 * bank's channel kernel.  What leaves the device per channel and block is packed PCM plus a status record instead of the
 * complex baseband -- for a 12 kHz mono S16 channel 480 B instead of 1920 B.  RTP framing and the sockets stay with the host.
 * The fields are the chan_t members src/linear.c reads (linear amplitudes / power ratios, not dB). */
#define CHZ_PCM_S16BE 0
#define CHZ_PCM_S16LE 1
#define CHZ_PCM_F32LE 2
#define CHZ_PCM_F32BE 3
#define CHZ_PCM_MULAW 4   /* G.711 mu-law, one byte per sample (float_to_mulaw, src/rtp.c:459-483) */
#define CHZ_PCM_ALAW 5    /* G.711 A-law (float_to_alaw, src/rtp.c:500-533) */
#define CHZ_PCM_F16LE 6   /* IEEE binary16, round to nearest even (export_f16_le / _be, src/import.h:140-157,207-212; src/audio.c:135-139) */
#define CHZ_PCM_F16BE 7
typedef struct chz_demod_params {
  int channels;         /* chan->output.channels: 1 mono, 2 stereo; 0 switches the channel's demodulator off */
  int env;              /* chan->linear.env: envelope (AM) detection */
  int agc;              /* chan->linear.agc */
  int encoding;         /* CHZ_PCM_* (chan->output.encoding) */
  int snr_squelch;      /* chan->squelch.snr_enable */
  int squelch_tail;     /* chan->squelch.tail */
  int tuned;            /* chan->tune.freq != 0 */
  int kind;             /* CHZ_DEMOD_LINEAR (demod_linear, src/linear.c) or CHZ_DEMOD_FM (demod_fm, src/fm.c:19-345: both SNR
                           estimators, squelch sequencer, discriminator with threshold extension or PLL demodulator, offset /
                           deviation statistics, PM carrier removal, PL-tone squelch, de-emphasis, gain) */
  double samprate;      /* chan->output.samprate */
  double headroom;      /* chan->output.headroom */
  double threshold, recovery_rate, hangtime, dc_alpha;   /* chan->linear.* */
  double bandwidth;     /* |chan->filter.min_IF - chan->filter.max_IF| */
  double shift;         /* chan->tune.shift, Hz */
  double squelch_open, squelch_close;                     /* chan->squelch.open / .close, power ratios */
  double gain;          /* chan->output.gain when the demodulator starts (the AGC owns it afterwards) */
  double deemph_rate, deemph_gain;   /* FM: chan->fm.rate (0 = flat FM), chan->fm.gain */
  double threshold_extend;           /* FM: chan->fm.threshold, 0 or 1 */
  int pll_enable;       /* chan->pll.enable: linear -- carrier-tracking PLL in front of the detector, lock detector, PLL squelch
                           (src/linear.c:83-153); FM -- PLL demodulator instead of the discriminator (src/fm.c:176-203) */
  int pll_square;       /* chan->pll.square (linear): squaring loop for suppressed-carrier signals */
  double pll_loop_bw;   /* chan->pll.loop_bw, Hz (linear; the FM loop is 500 Hz wide, src/fm.c:181) */
  double tone_freq;     /* FM: chan->fm.tone_freq, Hz; non-zero = PL / CTCSS tone squelch (src/fm.c:264-311) */
} chz_demod_params;
#define CHZ_DEMOD_LINEAR 0
#define CHZ_DEMOD_FM 1
typedef struct chz_demod_status {
  int frame;            /* 0: PCM present (send_output(chan, samples, N, mute)); 1: no samples (send_output(chan, NULL, N, mute)); 2: a filter2 bank's pending block (send_output is not called) */
  int mute;
  int squelch_state;
  int pll_lock;         /* chan->pll.lock (linear) */
  double output_power;  /* chan->output.power */
  double gain;          /* chan->output.gain after the block */
  double n0;            /* chan->sig.n0 (smoothed) */
  double snr;           /* linear: the squelch's SNR (the SNR squelch's, else the PLL's); FM: chan->fm.snr */
  double foffset;       /* chan->sig.foffset (FM; linear with the PLL on) */
  double pdeviation;    /* FM: chan->fm.pdeviation */
  double pll_snr;       /* chan->pll.snr (linear) */
  double pll_cphase;    /* chan->pll.cphase, radians (linear) */
  double tone_deviation;/* FM: chan->fm.tone_deviation, Hz */
  int pll_rotations;    /* chan->pll.rotations (linear) */
  int tone_mute;        /* FM: 1 while the tone squelch keeps the channel muted */
} chz_demod_status;
/* parameters of channels [ch0, ch0+n) from block `job` on (it must not have been enqueued yet); blocktime = radiod's Blocktime.
 * Waits for the demodulator stream only, never for the transform lanes.  A call that is refused has changed nothing.
 * On a bank that has demodulated blocks already, per channel:
 *  - the same kind on a channel that is on: decode_radio_commands() writing into the running channel.  Every member is read afresh
 *    from block `job` on; the demodulator's state goes on.  The AGC owns the gain (`gain` is ignored), the shift oscillator keeps its
 *    phase when the frequency changes (set_osc, src/osc.c:28-47), a linear PLL that comes on after blocks that ran without it starts
 *    from lock = 0, lock_count = -limit, rotations = 0 (src/linear.c:150-154) with the loop's state kept, and with the PLL off the status
 *    keeps pll_snr / pll_cphase / foffset of its last block.  tone_freq is read by the reference once, when demod_fm() starts
 *    (src/fm.c:50-53), and radiod has no command that changes it live: here a new tone_freq restarts the tone detector as a start leaves
 *    it (cleared, muted until the new tone has been seen, tone_deviation 0) and everything else goes on.
 *  - the other kind on a channel that is on: demod_thread() (src/radio.c:907-978) starting the other demodulator on the same chan_t.
 *    The function locals start over (src/linear.c:41-47, src/fm.c:36-62: init_pll(), am_dc, squelch sequencer and hysteresis,
 *    phase_memory, de-emphasis state, tone detector muted).  The chan_t members survive: sig.n0, output.gain (after demod_fm(): its
 *    fixed gain), linear.hangcount, pll.lock / .lock_count / .rotations / .snr / .cphase / .was_on, sig.foffset (one member for the
 *    linear PLL and demod_fm()), fm.pdeviation, and the shift oscillator, whose phase stands still while demod_fm() runs.  What a
 *    linear demodulator without its PLL writes every block (lock = 0, lock_count = -limit, rotations = 0) is what the next PLL life
 *    finds, with or without an FM stretch in between.
 *  - channels = 0 ends the channel: its status in every slot becomes frame 1 / mute 1 (flags NO_SAMPLES | MUTE), the open read
 *    does not count it, its PCM rows are left alone.  The reference has no such thing as a re-used channel index; here whoever
 *    switches the index on again -- in the same call sequence or blocks later -- gets a NEW channel and inherits nothing: n0 restarts at
 *    the first estimate, the gain at `gain`, PLL and tone records as init_pll() / a start leave them, the shift oscillator at phase 0.
 *    Channels beyond the old active count (chz_bank_set_active + this call) are new channels in the same sense. */
int chz_bank_set_demod(chz_engine *e, int bank, unsigned job, int ch0, int n, const chz_demod_params *p, double blocktime);
/* Demodulating blocks the caller supplies (radiod puts a channel's private second filter, filter2 -- chz_mini_* -- between the
 * channelizer and the demodulator, src/radio.c:1572-1594): chz_bank_write_block stores n channels' olen complex samples
 * (+ bb_power, noise estimates; NULL leaves what is there) into `slot`'s output image, chz_bank_demod runs the bank's
 * demodulators over the slot as block `job` on the demodulator stream (results: chz_bank_read_pcm). */
int chz_bank_write_block(chz_engine *e, int bank, int slot, int ch0, int n, const float *samples, const double *bb_power, const double *n0);
int chz_bank_demod(chz_engine *e, int bank, unsigned job, int slot);
/* on = 0: the bank's demodulators run only when chz_bank_demod says so (its channels pass through filter2 on the way);
 * on = 1 (default): behind every whole-bank channel launch */
int chz_bank_demod_auto(chz_engine *e, int bank, int on);
/* bytes between two channels' PCM rows = the stride of chz_bank_read_pcm's buffer.  Default olen*8 (stereo float32 fits);
 * chz_bank_set_pcm_stride, before the first chz_bank_set_demod, shrinks the rows to what the bank's encodings need (olen*2 for
 * mono S16), so that a block's PCM is one contiguous device-to-host copy of only the bytes that matter */
int chz_bank_pcm_stride(chz_engine *e, int bank);
int chz_bank_set_pcm_stride(chz_engine *e, int bank, int bytes);
/* PCM (pcm_stride bytes per channel, the encoding's N*channels samples first) and status of the block last demodulated
 * on `slot`; synchronous / asynchronous on the demodulator stream (completion: chz_sync) */
int chz_bank_read_pcm(chz_engine *e, int bank, int slot, int ch0, int n, void *pcm, chz_demod_status *status);
int chz_bank_read_pcm_async(chz_engine *e, int bank, int slot, int ch0, int n, void *pcm, chz_demod_status *status);
/* the same with one byte per channel instead of the 96-byte record: what the caller of send_output() needs every block */
#define CHZ_FLAG_NO_SAMPLES 1   /* send_output(chan, NULL, N, mute) */
#define CHZ_FLAG_MUTE 2
#define CHZ_FLAG_PLL_LOCK 4
#define CHZ_FLAG_TONE_MUTE 8
#define CHZ_FLAG_PENDING 16     /* a filter2 bank's block that did not fire (chz_bank_set_filter2): no frame, the byte holds nothing else */
int chz_bank_read_pcm_flags_async(chz_engine *e, int bank, int slot, int ch0, int n, void *pcm, unsigned char *flags);
/* returns once everything chz_bank_read_pcm_async / _flags_async has enqueued for `slot` so far has landed in the host buffers --
   without waiting for later blocks already handed to the demodulator stream (a double-buffered host loop waits for block j-1
   here while block j runs) */
int chz_bank_pcm_wait(chz_engine *e, int bank, int slot);
/* ---- only the rows somebody will send.  A channel is OPEN on a slot when its demodulator is on and its flag byte has none of
 * CHZ_FLAG_NO_SAMPLES, CHZ_FLAG_MUTE and CHZ_FLAG_PENDING: send_output() is handed samples for these and for no others.  The device
 * gathers their rows (kernels pcm_open_count / pcm_open_rows), so that n flag bytes + count * (pcm_stride + 4) bytes cross the link.
 * The dense buffers (4 * capacity * (pcm_stride + 5) bytes of device memory and two small tables) are allocated by the bank's first
 * open read and freed with the bank; a bank that never calls these runs and allocates exactly what it did without them. */
/* rows of the open channels of [ch0, ch0+n) of the block last demodulated on `slot`, dense and in ascending channel order:
   pcm   max_rows * pcm_stride bytes, index   max_rows ints (absolute channel numbers), flags   n bytes (every channel's, as
   chz_bank_read_pcm_flags_async gives them; may be NULL).  Host buffers must stay valid until the wait below.  max_rows = 0 asks
   for count and flags only.  Refused (-1, nothing enqueued): a slot whose last open read has not been waited for. */
int chz_bank_read_pcm_open_async(chz_engine *e, int bank, int slot, int ch0, int n, void *pcm, int *index, unsigned char *flags, int max_rows);
/* returns once they have landed; *count = open channels found (may exceed max_rows: then the first max_rows are delivered and
   the slot's image is intact for chz_bank_read_pcm_flags_async).  Refused (-1): no open read outstanding on the slot.
   Nothing reaches the host buffers before this call: chz_bank_pcm_wait on the slot only waits for the open read's kernels. */
int chz_bank_pcm_open_wait(chz_engine *e, int bank, int slot, int *count);
/* the two kernels' own times (ms, from the dispatch packets) of the slot's latest open read, after its wait.  Off until asked for:
   the first call on a bank turns the timing of its later open reads on; that call, and a call on a slot not timed yet, return 1 */
int chz_bank_pcm_open_times(chz_engine *e, int bank, int slot, double *count_ms, double *rows_ms);

/* ---- filter2 resident on the device: the channel's private second filter of downconvert() (src/radio.c:1503-1513, created at
 * :1572-1594; presets cwu / cwl with filter2 = 4, isb with filter2 = 1, share/presets.conf:204,223,297) as a stage of the block pipeline.
 * For a COMPLEX-output bank with tuning the engine runs a second overlap-save filter per channel behind every whole-bank channel
 * launch (chz_bank_execute, chz_step, chz_run_blocks), in block order on the demodulator stream, directly in front of the bank's
 * demodulators (kernel f2_ovs, one workgroup per channel, the transforms and gather rules of chz_mini_*).  It reads what the channel
 * kernel left in the slot's output image -- the samples behind the fine-tuning rotator (:1499-1501) --, the demodulators read ITS output,
 * and the slot's bb_power (chz_bank_read_power) is that of its output (:1515-1520).  Nothing travels to the host in between.
 *   blocking = chan->filter2.blocking >= 1; L2 = blocking * olen; M2 as given, 0 = radiod's own round2(2 L2) - L2 + 1 (:1578-1579);
 *   N2 = L2 + M2 - 1.  Refused, here and by chz_bank_filter2_check and nowhere else, is what chz_mini_create refuses: N2 outside
 *   8..8192 or with a prime factor above 13.
 * ONE phase per bank: block job0 is the first of a cycle and block j FIRES when (j - job0 + 1) % blocking == 0; a caller that needs
 * another phase uses another bank (no per-channel phase).  There is no drop-in entry point: filter.h callers create filter2
 * themselves and keep going through chz_mini_*.
 *   every block   the channel's olen new samples join its window (device memory, [capacity][N2]; zeros at first, as
 *                 create_filter_input leaves them, src/filter.c:244,259)
 *   firing block  transform of the N2-sample window (M2 - 1 old samples, L2 new ones), gather with shift 0 x response (:1511), ISB
 *                 unpacking where the channel's flag is set, zeroed Nyquist bin, backward transform, the last L2 samples to the
 *                 slot's filter2 image; bb_power = mean |y|^2 (float products, double sum); the demodulators then run on L2 samples
 *                 with the bank's unchanged block time (demod_linear / demod_fm see sampcount = L2 with the global Blocktime)
 *   pending block the reference's `continue` (:1509-1510): no demodulator launch; bb_power repeats the last firing block's value
 *                 (0 before the first); for channels with a demodulator the n0 smoother of :1468-1474, which sits in front of the
 *                 `continue`, takes its step; the slot's flag byte is CHZ_FLAG_PENDING, its status record has frame = 2 (send_output
 *                 is not called) and the smoothed n0, the PCM is left alone
 * A filter2 image exists per spectrum slot that can fire: CHZ_ND / gcd(blocking, CHZ_ND) of them.  Only whole-bank launches step the
 * stage: chz_bank_execute_range never touches a window.  Narrowband analysers attached to the bank keep reading the first filter's
 * output.  The demodulators' block length becomes L2 everywhere: the 10240-sample limit, chz_bank_set_pcm_stride's range (L2 .. 8 L2)
 * and default, the PCM fit check; chz_bank_set_demod's `job` counts as the cycle it falls in (name the first block of a cycle).  Hence chz_bank_set_filter2 is
 * refused once the bank has demodulators or a fixed PCM row size, and on REAL-output banks and banks without tuning;
 * chz_bank_write_block / chz_bank_demod are refused on such a bank, chz_run_blocks mode 1 too (-5).  The channel kernel's AGC-peak
 * epilogue is off; the demodulator takes its own first look at the block. */
int chz_bank_filter2_check(int olen, int blocking, int M2);      /* would chz_bank_set_filter2 take this geometry? 0, or < 0 and chz_last_error(); touches no device */
/* job0 has not been enqueued yet.  Drains the engine once, like other feature switches. */
int chz_bank_set_filter2(chz_engine *e, int bank, unsigned job0, int blocking, int M2);
int chz_bank_filter2_geometry(chz_engine *e, int bank, int out3[3]);                       /* L2, M2, N2 */
/* N2 complex per channel, as set_filter leaves it (:1591-1594); zeros until set.  In stream order from the next block enqueued; edits
 * of up to 8 MB do not drain */
int chz_bank_set_filter2_responses(chz_engine *e, int bank, int ch0, int n, const float *resp);
/* chan->filter2.out.isb (:1569,1586): one byte per channel, non-zero = on; in stream order like the responses */
int chz_bank_set_filter2_isb(chz_engine *e, int bank, int ch0, int n, const unsigned char *flags);
/* what set_channel_filter's delete and re-create do (:1570-1583): the channels' windows are zeros from block `job` on, which must be
 * the next block to be enqueued and the first of a cycle (the bank has one phase), else the call is refused */
int chz_bank_filter2_reset(chz_engine *e, int bank, unsigned job, int ch0, int n);
/* L2 complex per channel of the block that fired on `slot`; an error if that slot's last block was pending.  Synchronous /
 * asynchronous on the demodulator stream (completion: chz_sync) */
int chz_bank_filter2_read(chz_engine *e, int bank, int slot, int ch0, int n, float *host);
int chz_bank_filter2_read_async(chz_engine *e, int bank, int slot, int ch0, int n, float *host);

/* ---- small inline masters: radiod's filter2 (src/radio.c:1572-1594: a private COMPLEX master of N = round2(2*blocksize)
 * points with one same-size COMPLEX slave, run inline by the channel thread; share/presets.conf:204,223,297).  A pool holds
 * every instance of one geometry (8 <= N = L+M-1 <= 8192, no prime factor above 13); ONE kernel launch serves all instances that are
 * due (one workgroup each: forward transform, gather x response with the slave's shift, ISB unpacking, backward transform,
 * all in LDS).  The device keeps no overlap state: a request carries its whole N-sample window, exactly what the
 * reference's mirrored ring holds at input_read_pointer (src/filter.c:626-636). */
typedef struct chz_mini chz_mini;
int chz_mini_create(chz_mini **out, int L, int M, int capacity, int device);     /* replaces create_filter_input + _output */
void chz_mini_destroy(chz_mini *m);
int chz_mini_capacity(const chz_mini *m);
int chz_mini_add(chz_mini *m);                                                  /* -> instance index */
int chz_mini_release(chz_mini *m, int inst);
int chz_mini_set_response(chz_mini *m, int inst, const float *resp);            /* N complex, as set_filter leaves it */
/* n requests in one launch: instance inst[i], window win[i] (N complex on the host), shift[i] (NULL = 0), isb[i] (NULL = off),
 * L output samples to out[i]; synchronous, thread-safe */
int chz_mini_execute(chz_mini *m, int n, const int *inst, const float *const *win, const int *shift, const unsigned char *isb,
                     float *const *out);

/* ---- pools of small REAL inline masters with decimating slaves: wfm's composite master (src/wfm.c:70-89: L 7680, M 7681, a REAL
 * and two COMPLEX slaves of olen 960), stereod (src/stereod.c:383-401), rdsd (src/rdsd.c:395-406), packetd (src/packetd.c:493-495),
 * ctcss (src/ctcss.c:269-281).  A pool holds every instance of ONE geometry: (L, M, the slave list of (olen, out_type)); an instance
 * is one master with all its slaves.  One launch serves every request that is due, one workgroup each, everything in LDS: the N real
 * samples as an N/2-point packed transform and a Hermitian split, then per selected slave the gather x response of
 * src/filter.c:803-911 (negative shifts, bins outside the master, ISB, the zeroed Nyquist bin), a P_s-point backward transform
 * (P_s = N olen_s / L) and the last olen_s samples.  Stateless like chz_mini_*: a request carries its whole N-sample window.
 * Limits, refused at chz_rmini_create and nowhere else: N even, 16 <= N <= 16384, N/2 without a prime factor above 13; 1 to 4
 * slaves, each with P_s an integer, 8 <= P_s <= N, no prime factor above 13, even for a REAL slave; and
 * 8 * max(N, N/2 + 1 + 2 max P_s) bytes of LDS within the 160 KB of a workgroup. */
typedef struct chz_rmini chz_rmini;
int chz_rmini_create(chz_rmini **out, int L, int M, int nslaves, const int *olen, const int *out_type, int capacity, int device);
void chz_rmini_destroy(chz_rmini *m);
int chz_rmini_check(int L, int M, int nslaves, const int *olen, const int *out_type);   /* would chz_rmini_create take this geometry? 0, or < 0 and chz_last_error(); touches no device */
int chz_rmini_capacity(const chz_rmini *m);
int chz_rmini_add(chz_rmini *m);                                                /* -> instance index */
int chz_rmini_release(chz_rmini *m, int inst);
int chz_rmini_set_response(chz_rmini *m, int inst, int slave, const float *resp);   /* P_s complex, as set_filter leaves it (a REAL slave's P_s/2 + 1 bins first) */
/* n requests, one H2D, ONE launch and one D2H per chunk of `capacity`: instance inst[i], window win[i] (N floats on the host), per
 * slave s the shift shift[i*nslaves+s] (NULL = 0) and ISB flag isb[i*nslaves+s] (NULL = off); mask[i] selects the slaves to run
 * (bit s; NULL = all); out[i*nslaves+s] receives olen_s complex or float samples, may be NULL, and stays untouched for a slave the
 * mask leaves out.  An instance may appear several times.  Synchronous, thread-safe. */
int chz_rmini_execute(chz_rmini *m, int n, const int *inst, const float *const *win, const int *shift, const unsigned char *mask,
                      const unsigned char *isb, float *const *out);

/* ---- Pooled stereo broadcast-FM decoders: demod_wfm() (src/wfm.c:134-281) from a 384 kHz channel's baseband to its 48 kHz PCM ------
 * One launch serves every instance that is due, one workgroup per request: squelch, discriminator, statistics, the composite filter
 * (a REAL master of L = 384 kHz x blocktime samples, M = L + 1, with its mono, pilot and L-R slaves -- chz_rmini_*'s transform and
 * gather rules), pilot detector, stereo matrix, de-emphasis and PCM packing.  The decoder is a recurrence over blocks: phase_memory,
 * the squelch sequencer, foffset / pdeviation, the de-emphasis states and the composite filter's history live on the device, per
 * instance, all zero after chz_wfm_add.  Limits, refused at chz_wfm_create / chz_wfm_check and nowhere else: what chz_rmini_create
 * refuses for that master, and a 19 or 38 kHz bin shift that is no multiple of 4 or leaves a remainder (src/wfm.c:96,101) -- 10 ms
 * and 20 ms blocks remain.
 * Option wfm_deemph_lanes (chz_set_option, read by chz_wfm_create): how many lanes share a block's de-emphasis recurrence, 64 (default)
 * = runs of consecutive samples reduced to affine maps and replayed, 1 = one lane walks the block (a measurement switch). */
typedef struct chz_wfm chz_wfm;
typedef struct chz_wfm_params {
  int stereo_enable;    /* chan->fm.stereo_enable: look for the pilot */
  int encoding;         /* CHZ_PCM_* */
  int squelch_tail;     /* chan->squelch.tail, blocks */
  double squelch_open, squelch_close;   /* power ratios */
  double bandwidth;     /* |max_IF - min_IF|, Hz */
  double headroom;      /* amplitude ratio */
  double deemph_rate, deemph_gain;      /* chan->fm.rate (0: no de-emphasis), chan->fm.gain */
} chz_wfm_params;
typedef struct chz_wfm_status {
  int frame;            /* 0: PCM present; 1: no samples (squelch closed: mute, pcm untouched) */
  int mute, squelch_state;
  int channels;         /* 2 with the pilot present, else 1: pcm holds olen * channels samples */
  int pilot_present;
  double snr;           /* chan->fm.snr */
  double foffset, pdeviation, output_power;
  double gain;          /* chan->output.gain = 2 headroom 384000 / bandwidth */
  double subc_amp;      /* mean |pilot|^2 (chan->tp1); 0 where the pilot filter did not run */
} chz_wfm_status;
int chz_wfm_check(double blocktime);                                            /* would chz_wfm_create take this block time? 0, or < 0 and chz_last_error(); touches no device */
int chz_wfm_create(chz_wfm **out, double blocktime, int capacity, int device);
void chz_wfm_destroy(chz_wfm *m);
int chz_wfm_capacity(const chz_wfm *m);
int chz_wfm_geometry(const chz_wfm *m, int out6[6]);                            /* L, N, olen, P, pilot_shift, subc_shift */
int chz_wfm_add(chz_wfm *m);                                                    /* -> instance index */
int chz_wfm_release(chz_wfm *m, int inst);
int chz_wfm_set_params(chz_wfm *m, int inst, const chz_wfm_params *p);
int chz_wfm_set_response(chz_wfm *m, int inst, int slave, const float *resp);   /* slave 0 mono, 1 pilot, 2 L-R; P complex, as chz_rmini_set_response */
/* One block of n decoders, one H2D, ONE launch and one D2H per chunk of `capacity`: instance inst[i] (at most once in a call) takes the
 * L complex samples at bb[i] -- host memory (bb_on_device = 0), or device memory that is complete before the call (1: e.g. a row of
 * chz_bank_output_device() after chz_slot_sync; read in place) --, the channel's bb_power[i] (chz_bank_read_power) and the host's
 * smoothed noise density n0[i]; pcm[i] receives olen * status[i].channels samples of the instance's encoding and stays untouched when
 * status[i].frame = 1.  What comes back per request is its status record and one PCM row as large as the instance can fill (olen samples,
 * twice as many with stereo_enable).  Every request is checked before the first launch: a refused call has written nothing and advanced no state.
 * Synchronous, thread-safe. */
int chz_wfm_execute(chz_wfm *m, int n, const int *inst, const float *const *bb, int bb_on_device, const double *bb_power, const double *n0,
                    void *const *pcm, chz_wfm_status *status);

/* ---- Pooled AFSK / AX.25 packet decoders: packetd's decode_task() (src/packetd.c:485-629, hdlc_process() :634-682, crc_good()
 * src/ax25.c:139-155) from a session's 16-bit audio to its frames ------
 * A pool is one geometry: (L, M, samprate, bitrate, mark, space, input byte order); packetd's own is L 960, M 961, bitrate 1200, mark 1200,
 * space 2200 at the stream's sample rate, samppbit = (int)(samprate / bitrate).  One launch serves every session that is due, one
 * workgroup per request: the L samples are converted (:551-552) and appended to the session's M - 1 old ones, the REAL master and its one
 * COMPLEX slave (olen L, shift 0; chz_rmini_*'s transform and gather rules, the response from the host) make them analytic, and one lane
 * walks the block as the reference does: two tone oscillators (src/osc.c, renormalised every 16384 steps), on-time and offset
 * integrators, the Gardner clock, NRZI, HDLC and the CRC, all in double.  The decoder is a recurrence over blocks: the filter's history,
 * oscillators, integrators, symphase / last_val / mid_val and the HDLC state with its 16384-byte frame buffer live on the device, per
 * instance, all zero after chz_afsk_add.  What stays with the caller: RTP, the reference's input feeder (five blocks of zeros after a
 * block that ends in 100 zero samples, :540-546) and whatever parses the frames (APRS).
 * Limits, refused at chz_afsk_create / chz_afsk_check and nowhere else: what chz_rmini_create refuses for that master and slave;
 * samppbit < 4; a tone at or above samprate / 2; a block that can hold more than 64 decisions, ceil(L / (samppbit - 1)) > 64 (they are
 * reported as one 64-bit word).  A frame and its closing flag take at least 32 decisions, so at most CHZ_AFSK_STATUS_FRAMES = 64 / 32 = 2
 * frames complete in one block. */
#define CHZ_AFSK_BE 0                 /* samples as RTP carries them (ntohs at :551) */
#define CHZ_AFSK_LE 1
#define CHZ_AFSK_STATUS_FRAMES 2
#define CHZ_AFSK_FRAME_MAX 16384      /* sizeof(hdlc.frame): no frame is longer */
typedef struct chz_afsk chz_afsk;
typedef struct chz_afsk_status {
  int ndecisions;               /* bit decisions taken in this block */
  int symphase;                 /* at the end of the block */
  unsigned long long bits;      /* decision i in bit i: 1 = no transition (an NRZI one) */
  double last_val, mid_val;     /* at the end of the block */
  int flag_seen, frame_bits;    /* hdlc state at the end of the block */
  int crc_failures;             /* frames of this block whose CRC failed: counted, not delivered */
  int nframes;                  /* frames completed in this block, 0 .. CHZ_AFSK_STATUS_FRAMES */
  int frame_len[CHZ_AFSK_STATUS_FRAMES];   /* their lengths in bytes, the two CRC bytes included */
} chz_afsk_status;
int chz_afsk_check(int L, int M, double samprate, double bitrate, double mark, double space, int byte_order);   /* would chz_afsk_create take this? 0, or < 0 and chz_last_error(); touches no device */
int chz_afsk_create(chz_afsk **out, int L, int M, double samprate, double bitrate, double mark, double space, int byte_order, int capacity, int device);
void chz_afsk_destroy(chz_afsk *m);
int chz_afsk_capacity(const chz_afsk *m);
int chz_afsk_geometry(const chz_afsk *m, int out4[4]);                          /* L, M, N, samppbit */
int chz_afsk_add(chz_afsk *m);                                                  /* -> instance index; all state zero, as a fresh decode_task */
int chz_afsk_release(chz_afsk *m, int inst);
int chz_afsk_set_response(chz_afsk *m, int inst, const float *resp);            /* N complex, as chz_rmini_set_response (packetd: set_filter(900 / samprate, 2500 / samprate, 3.0)) */
/* One block of n decoders, one H2D, ONE launch and one D2H of status records per chunk of `capacity`: instance inst[i] (at most once in
 * a call) takes the L 16-bit samples at samples[i] in the pool's byte order -- host memory (samples_on_device = 0), or device memory that
 * is complete before the call (1; read in place, 2-byte aligned).  Frame j < status[i].nframes lands at frames[i] + j * frame_stride, at
 * most frame_stride bytes of its status[i].frame_len[j]; the rest of frames[i] stays untouched.  Only the bytes of frames that completed
 * cross the link, in a second copy sized by their lengths (one per request that completed a frame, one wait); a block without a frame
 * returns status only.  Every request is checked before the first launch: a refused call has written nothing and advanced no state.
 * Synchronous, thread-safe. */
int chz_afsk_execute(chz_afsk *m, int n, const int *inst, const void *const *samples, int samples_on_device, chz_afsk_status *status,
                     unsigned char *const *frames, int frame_stride);

/* ---- Pooled CTCSS / PL tone decoders: ctcss's tone search (src/ctcss.c:268-309, process_pl() :392-419, the oscillators of src/osc.c:28-70)
 * from a session's 16-bit audio to the index of the tone it carries ------
 * A pool is one geometry: (samprate, input byte order, tone table).  The sample rate alone fixes the rest as ctcss does: blocks of
 * L = lrint(0.2 samprate) samples, M = L + 1, N = 2 L, one COMPLEX slave of olen = 100 samples at 500 Hz (P = 200), rotated by
 * shift = 60 bins (150 Hz), and one decision per block (pl_blocksize = 100 = olen).  One launch serves every session that is due, one
 * workgroup per request: the L samples are converted (:294) and appended to the session's M - 1 old ones, the REAL master and its slave
 * (chz_rmini_*'s transform and gather rules, the response from the host) leave 100 complex samples, lane t of one wavefront correlates
 * them with tone t's oscillator in double, in the reference's order (step_osc(), renormalised every 16384 steps; integrator +=
 * conj(samp) * phasor), and one lane compares the energies |integrator|^2 in ascending tone order with the reference's strict >,
 * starting from the threshold 0.005 * 100.  The decoder is a recurrence over blocks: the filter's history, the oscillators and the
 * sticky current tone live on the device, per instance, all zero after chz_ctcss_add (the integrators are zero again after every block).
 * What stays with the caller: RTP and collecting a stream's packets into rows of L samples.
 * Limits, refused at chz_ctcss_create / chz_ctcss_check and nowhere else: what chz_rmini_create refuses for that master and slave
 * (48 kHz gives N = 19200 > 16384; the largest L is 8192, 40960 Hz); a sample rate that is not finite and positive; a byte order that
 * is neither; a table of fewer than 1 or more than CHZ_CTCSS_TABLE_MAX = 64 tones (one wavefront); a tone that is not finite. */
#define CHZ_CTCSS_BE 0                /* samples as RTP carries them (ntohs at :294) */
#define CHZ_CTCSS_LE 1
#define CHZ_CTCSS_TABLE_MAX 64
#define CHZ_CTCSS_STANDARD_TONES 55   /* the table searched when chz_ctcss_create is given none: ctcss's own PL_tones[], 67.0 .. 254.1 Hz */
typedef struct chz_ctcss chz_ctcss;
typedef struct chz_ctcss_status {
  int tone_index;               /* the strongest tone above the threshold in this block, -1: none (strongest_tone_index) */
  int current_index;            /* the last tone found so far (the index of current_pl_tone), -1 before the first detection */
  double energy;                /* strongest_tone_energy as the block leaves it: the tone's, or the threshold itself when none is found */
} chz_ctcss_status;
/* tones: ntones frequencies in Hz, or NULL for the standard table (ntones is then not looked at).  A tone of 0 Hz or below is searched
 * like any other but never becomes the current one (the reference tests pl_tone > 0, :303). */
int chz_ctcss_check(double samprate, int byte_order, int ntones, const double *tones);   /* would chz_ctcss_create take this? 0, or < 0 and chz_last_error(); touches no device */
int chz_ctcss_create(chz_ctcss **out, double samprate, int byte_order, int ntones, const double *tones, int capacity, int device);
void chz_ctcss_destroy(chz_ctcss *m);
int chz_ctcss_capacity(const chz_ctcss *m);
int chz_ctcss_geometry(const chz_ctcss *m, int out7[7]);                         /* L, M, N, olen, P, shift, ntones */
int chz_ctcss_add(chz_ctcss *m);                                                 /* -> instance index; all state zero, as a fresh session */
int chz_ctcss_release(chz_ctcss *m, int inst);
int chz_ctcss_set_response(chz_ctcss *m, int inst, const float *resp);           /* P complex, as chz_rmini_set_response (ctcss: set_filter(-100 / 500, 150 / 500, 11)) */
/* One block of n decoders, one H2D, ONE launch and one D2H of status records per chunk of `capacity`: instance inst[i] (at most once in
 * a call) takes the L 16-bit samples at samples[i] in the pool's byte order -- host memory (samples_on_device = 0), or device memory that
 * is complete before the call (1; read in place, 2-byte aligned).  energies may be NULL; energies[i], where not NULL, receives the
 * request's ntones energies in table order (a second D2H, made only for a chunk in which a request asks).  Every request is checked
 * before the first launch: a refused call has written nothing and advanced no state.  Synchronous, thread-safe. */
int chz_ctcss_execute(chz_ctcss *m, int n, const int *inst, const void *const *samples, int samples_on_device, chz_ctcss_status *status,
                      double *const *energies);

/* ---- Pooled FM-multiplex decoders: stereod's and rdsd's decode() loops (src/stereod.c:373-408 and :460-513, src/rdsd.c:385-413 and
 * :465-500) from a session's 16-bit FM multiplex at 384 kHz -- a discriminator's output -- to its 16-bit output at 48 kHz ------
 * A pool is one geometry: (block time, kind, input byte order).  The block time alone fixes the rest as both programs do:
 * L = lrint(384000 blocktime), M = L + 1, N = 2 L, slaves of olen = L / 8 samples (P = 2 olen), rotated by quantum * lrint(f / (hzperbin
 * * quantum)) bins with quantum = 2 and the integer hzperbin = 384000 / N.  One launch serves every session that is due, one workgroup
 * per request: the L samples are converted and appended to the session's L old ones, the REAL master and its slaves (chz_rmini_*'s
 * transform and gather rules, the responses from the host) decimate, and the per-sample loop runs behind them.
 *   CHZ_MPX_STEREO: samples as (float)((1. / 32767) * s); a REAL mono slave at shift 0, COMPLEX pilot and L-R slaves at 19 and 38 kHz; per
 *   output sample, in double, the pilot squared and normalised (where its magnitude is > 0, else L-R counts as 0 and the sample is
 *   counted in zero_pilot), 2 Im(conj(subc) stereo), left = mono + that and right = mono - that, each side through
 *   state = state * rate + gain * (1 - rate) * x and, as a float, through scaleclip() (src/misc.h:252-254); big-endian, L R interleaved.
 *   CHZ_MPX_RDS: samples as ldexp(s, -15); COMPLEX slaves for the pilot and at 57 kHz; the output is scaleclip() of the 57 kHz slave's
 *   re and im, big-endian -- all rdsd does today; nothing reads the pilot slave, so the device does not compute it.
 * The decoder is a recurrence over blocks: the filter's history, the two de-emphasis states and the parameters live on the device, per
 * instance; chz_mpx_add leaves history and states zero and the parameters stereod's own.
 * What stays with the caller: RTP (both ways) and collecting a stream's packets into rows of L samples.
 * Limits, refused at chz_mpx_create / chz_mpx_check and nowhere else: what chz_rmini_create refuses for that master and its slaves
 * (25 ms gives N = 19200 > 16384); 384000 % N != 0 (3 ms: the reference would truncate hzperbin silently); a shift that does not land
 * on its frequency (2.5 ms: 19 kHz falls between even bins of 200 Hz); a kind or byte order that is neither value; a block time that is
 * not finite and positive.  1, 2, 5 (both programs' own), 10 and 20 ms pass.
 * Option mpx_deemph_lanes (chz_set_option, read by chz_mpx_create): how many lanes share a block's de-emphasis recurrences, 64 (default)
 * down to 1 (one lane walks the block in the reference's order). */
#define CHZ_MPX_STEREO 0
#define CHZ_MPX_RDS    1
#define CHZ_MPX_BE 0   /* samples as RTP carries them */
#define CHZ_MPX_LE 1
typedef struct chz_mpx chz_mpx;
typedef struct chz_mpx_params { double deemph_rate, deemph_gain; } chz_mpx_params;   /* after chz_mpx_add: stereod's own, exp(-1 / (75e-6 * 48000)) and 4; rate 0 = no memory.  RDS ignores them */
typedef struct chz_mpx_status {
  int zero_pilot;                    /* STEREO: samples of this block whose squared pilot had magnitude 0 (the reference's a > 0 test failed); RDS: 0 */
  int pad;
  double deemph_left, deemph_right;  /* the states as the block leaves them; RDS: 0 */
} chz_mpx_status;
int  chz_mpx_check(double blocktime, int kind, int byte_order);            /* would chz_mpx_create take this? 0, or < 0 and chz_last_error(); touches no device */
int  chz_mpx_create(chz_mpx **out, double blocktime, int kind, int byte_order, int capacity, int device);
void chz_mpx_destroy(chz_mpx *m);
int  chz_mpx_capacity(const chz_mpx *m);
int  chz_mpx_geometry(const chz_mpx *m, int out7[7]);                      /* L, M, N, olen, P, pilot_shift, subc_shift */
int  chz_mpx_add(chz_mpx *m);                                              /* -> instance index; all state zero, as a fresh decode() thread */
int  chz_mpx_release(chz_mpx *m, int inst);
int  chz_mpx_set_params(chz_mpx *m, int inst, const chz_mpx_params *p);    /* 0 <= rate < 1, both finite; in effect from the next block, the states carry over */
int  chz_mpx_set_response(chz_mpx *m, int inst, int slave, const float *resp);   /* STEREO: 0 mono, 1 pilot, 2 L-R; RDS: 0 pilot, 1 rds; P complex, as chz_rmini_set_response */
/* One block of n decoders, one H2D, ONE launch and one D2H of status records and PCM per chunk of `capacity`: instance inst[i] (at most
 * once in a call) takes the L 16-bit samples at samples[i] in the pool's byte order -- host memory (samples_on_device = 0), or device
 * memory that is complete before the call (1; read in place, 2-byte aligned).  pcm[i] receives 4 olen bytes.  audio may be NULL;
 * audio[i], where not NULL, receives the 2 olen floats the packer was fed -- (float)left, (float)right interleaved, or the 57 kHz
 * slave's re / im pairs -- (a second D2H, made only for a chunk in which a request asks).  Every request is checked before the first
 * launch: a refused call has written nothing and advanced no state.  Synchronous, thread-safe. */
int  chz_mpx_execute(chz_mpx *m, int n, const int *inst, const void *const *samples, int samples_on_device,
                     void *const *pcm, float *const *audio, chz_mpx_status *status);

/* ---- Welch power spectra of the raw input: radiod's wideband spectrum analyser (wideband_poll(), src/spectrum.c:308-522) on the
 * samples the engine's input ring holds (float REAL, float COMPLEX or the int16 of chz_input_write_i16).  A bank holds `capacity`
 * analysers sharing one fft_n (= lrint(samprate / rbw): any length from 8 to 2^20 points; one with a prime factor above 13 runs as
 * chirp-z and needs 2^k >= 2 fft_n - 1 to fit as well), each with its own window, bin shift, bin count, averaging count and
 * overlap.  Per analyser and poll: fft_avg segments of fft_n samples, hop = lrint(fft_n (1 - overlap)), the first one starting
 * adjust = lrint(fft_n (1 + (fft_avg - 1)(1 - overlap))) samples in front of the end of the window -- a REAL master's segments
 * then walk forwards, a COMPLEX master's backwards, as the reference's two branches do (:366,:407 / :424,:491) -- each times the
 * window, transformed, and gain |X[binp]|^2 added bin by bin in iteration order in the reference's types (float bins, double
 * sums; gain = 2 or 1 / (fft_avg fft_n^2), :373,:431).  The bin walks are :396-406 (real: DC and the positive frequencies, then
 * the wrap to the negative output half; a negative shift inverts the spectrum by the sign flip of :381-391) and :477-488
 * (complex: signed offsets).  Bins outside the front end's coverage stay zero.  The same input gives the same bits, whatever else
 * is polled in the same call.  Byte encoding and window generation stay with the caller. */
/* returns a bank id; refuses (with a message) an fft_n no transform covers or longer than the input ring */
int chz_welch_create(chz_engine *e, int fft_n, int capacity, int max_bins, int max_avg);
int chz_welch_destroy(chz_engine *e, int bank);
/* fft_n floats, as generate_window() leaves them in chan->spectrum.window (zeros until set) */
int chz_welch_set_window(chz_engine *e, int bank, int slot, const float *window);
/* shift = chan->filter.bin_shift scaled to fft_n (:347).  fft_avg is limited to the data on hand by the reference's formula with
 * the DEVICE ring's length: floor(1 + (ring_samples / fft_n - 1) / (1 - overlap)), integer quotient (:359-361); the effective
 * value is returned (< 0: error -- a value that is still above the bank's max_avg among them). */
int chz_welch_configure(chz_engine *e, int bank, int slot, int shift, int bin_count, int fft_avg, double overlap);
/* one launch pair for analysers slots[0..nslots) (NULL: 0..nslots-1), on a stream of the polls' own: ordered behind every
 * chz_input_write* issued before it, in no lane's chain.  end_sample is the ring position (samples; job * L is where block job's
 * new samples start, as for chz_forward; taken modulo the ring length) just past the newest sample of the window; < 0 = the
 * write position, i.e. everything written so far.  A later chz_input_write* that would overwrite samples an unfinished poll
 * still reads waits for that poll; other writes do not.  Both orderings cover chz_input_write* only: a run of
 * chz_run_blocks_sharded in mode 2 fills the ring of every rank on the communicator's stream, outside them -- poll such an engine
 * between those runs (after chz_sync), with an explicit end_sample on the ranks other than the root, whose write position does not move.
 * Option welch_packed (chz_set_option, read by chz_welch_create): 1 (default) = a REAL master's even fft_n runs as a half-length packed
 * transform with a Hermitian split where the bins are read, 0 = as a full-length complex transform. */
int chz_welch_poll(chz_engine *e, int bank, int nslots, const int *slots, long long end_sample);
/* bins: n rows of max_bins floats (the first bin_count of a row are the analyser's bin_data, FFT order as the reference leaves
 * them); minmax: n pairs (min_power, max_power) over those bins as :498-507 leave them, from which the caller derives base and step
 * (:508-520).  Either may be NULL.  Synchronous / asynchronous in the polls' stream: completion of the latter is observed through
 * chz_host_callback(e, CHZ_SLOT_WELCH, ..) or chz_slot_sync(e, CHZ_SLOT_WELCH) (or chz_sync). */
#define CHZ_SLOT_WELCH (-2)
int chz_welch_read(chz_engine *e, int bank, int slot0, int n, float *bins, double *minmax);
int chz_welch_read_async(chz_engine *e, int bank, int slot0, int n, float *bins, double *minmax);

/* ---- Welch power spectra of a channel's baseband: radiod's narrowband spectrum analyser (narrowband_poll(), src/spectrum.c:206-306, fed by
 * demod_spectrum(), :123-155) on the output rows a COMPLEX-output channel bank leaves in HBM.  chz_bank_welch_create makes a bank of
 * `capacity` analysers sharing one fft_n (any length chz_welch_create takes), in the id space of chz_welch_create: chz_welch_set_window,
 * chz_welch_read, chz_welch_read_async (CHZ_SLOT_WELCH) and chz_welch_destroy serve both kinds; chz_welch_configure / _poll refuse a bank
 * of this kind with a message, and the calls below refuse a bank of chz_welch_create.  REAL-output banks are refused.
 * Each attached analyser owns a device ring of max_avg * fft_n + (CHZ_ND + 1) * olen complex samples, zeros at attach like the
 * reference's fresh ring (:142-144).  From then on every execution of the bank (chz_step, chz_run_blocks, chz_bank_execute[_range]) copies
 * the analyser's channel row of block `job` to ring position ((job - job0) * olen) mod ring length, right behind the channel kernel on
 * the block's own stream (kernel bb_ring_append): a closed form in the block number, so a re-run of a block (chz_bank_execute_range)
 * rewrites the samples it wrote before, and blocks before job0 write nothing.  A bank without attached analysers pays nothing.  With
 * chz_bank_set_tuning the rows carry downconvert()'s fine rotation, as chan->baseband does.
 * Per analyser and poll, narrowband_poll()'s arithmetic: fft_avg segments walking FORWARDS from end - lrint(fft_n (1 + (fft_avg - 1)
 * (1 - overlap))) (:247) with hop = fft_n - lrint(fft_n overlap) (:278), each times the window, transformed, and gain |X[fr]|^2 added
 * bin by bin in iteration order in the reference's types, gain = 1 / (fft_n^2 fft_avg) (:255, no factor 2), fr = i for
 * i < bin_count / 2, then fft_n - bin_count / 2 + (i - bin_count / 2) (:267-276, no shift); min and max as :284-293.  Where the two
 * roundings carry the last segment past the end of the window, the reference's ring of fft_avg * fft_n samples wraps onto its oldest
 * samples; the device reads those same samples (fft_avg * fft_n further back).  For an ODD bin_count the reference's last bin would
 * read X[fft_n], which its own assert (:271) forbids: the device leaves that bin zero.  bin_count > fft_n and fft_avg > max_avg are
 * refused; fft_avg is not clamped (the reference's limit never binds, :242-246).  A configuration that needs a longer ring
 * (max_avg, fft_n) takes a new bank: rings start as zeros.
 * Graph replay: chz_run_blocks(mode 1) is REFUSED with a message while any bank has attached analysers (the block number is baked into
 * captured launches); attach, detach, configure and destroy drop a captured graph like every configuration change. */
int chz_bank_welch_create(chz_engine *e, int bank, int fft_n, int capacity, int max_bins, int max_avg);
/* analyser `slot` follows channel `channel` of the bank from block job0 on (the next block to be executed, or -- with a
 * chz_bank_execute_range of it afterwards -- the one just executed).  Drains the engine.  Detach stops the copies. */
int chz_bank_welch_attach(chz_engine *e, int welch, int slot, int channel, unsigned job0);
int chz_bank_welch_detach(chz_engine *e, int welch, int slot);
/* returns the effective fft_avg (= fft_avg), < 0: error */
int chz_bank_welch_configure(chz_engine *e, int welch, int slot, int bin_count, int fft_avg, double overlap);
/* one launch pair for analysers slots[0..nslots) (NULL: 0..nslots-1) on the polls' stream; the window ends just past block `job`'s
 * samples.  Ordered behind the ring appends of every block issued so far (one event per slot); blocks job+1 .. job+CHZ_ND may be in
 * flight or issued meanwhile -- the ring's slack keeps them out of the window -- and the append of a later block that would overwrite
 * samples an unfinished poll still reads waits for that poll (one event; the whole ring is taken as one); other appends do not wait.
 * Refused: a job not issued yet, one from before an analyser's attach, and one more than CHZ_ND blocks behind the newest issued. */
int chz_bank_welch_poll(chz_engine *e, int welch, int nslots, const int *slots, unsigned job);

/* host-side helper exposed for tests: out3 = {hop, adjust} of chz_bank_welch_configure(fft_n, fft_avg, overlap) and the ring position of
 * block job's first sample for an analyser attached at job0 (-1: the block lies before the attach) */
int chz_bank_welch_steps(int fft_n, int fft_avg, double overlap, unsigned job, unsigned job0, int olen, long long ring_len, long long out3[3]);

/* host-side helper exposed for tests: the closed-form gather descriptor
 * {t0,cnt,src0,dir,conj,wrap} that restates src/filter.c:728-911 */
int chz_gather_descriptor(int in_type, int master_bins, int P, int shift, int out6[6]);

#ifdef __cplusplus
}
#endif
#endif
