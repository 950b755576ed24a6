/* ka9q_filter_hip_ext.h -- what libka9q_filter_hip.so offers BEYOND ka9q-radio's filter.h (optional; a caller that only
 * knows filter.h never needs it).
 *
 * estimate_noise() (/root/reference/src/radio.c:1783-1866) reads master->fdomain[] on the host for every channel and
 * block; it is the only reader of the block spectrum outside filter.c, and the reason the drop-in copies 13 MB per
 * block back over PCIe by default (KA9Q_HIP_FDOMAIN=1).  The device runs the same function (kernel noise_est, pinned to
 * radio.c's own code to 1e-12): a radiod built with the three-line patch of INTEGRATION.md section 1 takes the estimate
 * from filter_hip_noise() and sets KA9Q_HIP_FDOMAIN=0.
 */
#ifndef KA9Q_FILTER_HIP_EXT_H
#define KA9Q_FILTER_HIP_EXT_H
#ifdef __cplusplus
extern "C" {
#endif
struct filter_in;
struct filter_out;
/* switch the device-side noise estimate on for every channel of `master` (samprate = Frontend.samprate, Hz; 0 = off).
   Returns 0, 1 if some channel sizes have no noise kernel (their slaves report NaN), -1 on bad arguments.
   Env KA9Q_HIP_NOISE_SAMPRATE=<Hz> does the same at create_filter_input time. */
int filter_hip_enable_noise(struct filter_in *master, double samprate);
/* N0 of the block the slave's last execute_filter_output() delivered (NaN: not available) */
double filter_hip_noise(struct filter_out const *slave);
/* returns once the device has finished every block handed to it so far */
int filter_hip_drain(struct filter_in *master);
/* blocks skipped by the front end because the device was ND blocks behind (only with KA9Q_HIP_INPUT_FULL=drop) */
unsigned long filter_hip_skipped_blocks(struct filter_in const *master);
/* Failure policy.  A failed device-side check or a HIP error while a block is being enqueued makes the drop-in replace its engine
   ONCE (every registered slave's response, shift, ISB / beam state, the notch list and the overlap history are carried over; the
   blocks lost on the way are zeros + block_drops for every slave, like a lapped block, /root/reference/src/filter.c:690-701); a second
   failure within 500 blocks, or a re-creation that fails, ends the process with EX_SOFTWARE so that the supervisor restarts it, which
   is what the reference does on a fatal error (/root/reference/src/radio.c:398, src/main.c:202).  Returns the number of recoveries so far. */
unsigned filter_hip_recoveries(struct filter_in const *master, unsigned *blocks_lost);
/* Sharding behind filter.h.  Env KA9Q_HIP_DEVICES="0,1,..." at create_filter_input time spreads the slaves of the master over the
   listed devices (one engine each; every device takes the block's samples from the same pinned host ring and transforms them
   itself; slaves are assigned in creation order, KA9Q_HIP_SHARD_CHANNELS -- default 1024 -- per device before the next one is
   used; a block is complete when every device has delivered).  The reference runs a thread per channel inside one process against
   one shared master (/root/reference/src/radio.c:996, src/filter.c:704-712); callers of filter.h see no difference.  Returns the
   number of devices; counts (may be NULL) receives the slaves living on each. */
int filter_hip_devices(struct filter_in const *master, int *counts, int max);
/* round 6: what the process must still do before the drop-in ends it for the supervisor (a second device failure, a re-creation that
 * fails, a device that completes nothing for KA9Q_HIP_WEDGED_MS).  The reference's fatal path shuts the front end down first
 * (src/main.c:197-201: Frontend.shutdown -- bias tee off, streaming stopped); radiod registers the equivalent here, e.g.
 *     static void hw_off(void) { if (Frontend.shutdown) Frontend.shutdown(&Frontend); }   ...   filter_hip_set_exit_hook(hw_off);
 * Called once, from the failing thread, before stdio is flushed and _exit(EX_SOFTWARE).  NULL removes it. */
void filter_hip_set_exit_hook(void (*hook)(void));
/* The wideband spectrum analyser on the device: what wideband_poll() (src/spectrum.c:308-522) computes from the raw A/D ring on the
 * host -- fft_avg overlapping windowed segments of fft_n samples, transformed, |X|^2 of bin_count bins around `shift` summed into
 * bin_data[] in the reference's bin order -- computed from the newest samples the master's DEVICE ring holds (with KA9Q_HIP_DEVICES: the
 * first device's).  window = chan->spectrum.window (fft_n floats); minmax (may be NULL) receives min_power / max_power of :498-507.
 * Synchronous.  Returns the effective fft_avg (limited to the data on hand as :359-361 limit it), -1 when the master has no device ring
 * (a small inline master) or on bad arguments.  (Named outside this header's other prefix on purpose: the set of names carrying that
 * prefix is pinned by the exported-symbol test.) */
int ka9q_hip_spectrum(struct filter_in *master, int fft_n, const float *window, int shift, int bin_count, int fft_avg, double overlap,
                      float *bin_data, double minmax[2]);
/* The narrowband spectrum analyser on the device: what narrowband_poll() (src/spectrum.c:206-306, fed by demod_spectrum(), :123-155)
 * computes on the host from a ring of the channel's baseband -- fft_avg windowed segments of fft_n samples walking forwards, transformed,
 * 1 / (fft_n^2 fft_avg) |X|^2 summed into bin_data[] in its bin order (no shift; an odd bin_count leaves the last bin zero, where the
 * reference's own assert :271 would fail) -- computed from the rows a COMPLEX slave's channel leaves on the device, ending with the block
 * the slave's last execute_filter_output() delivered.  The first call for a (slave, fft_n) attaches the analyser: it follows the channel
 * from the NEXT block the master issues, history before that is zeros like the reference's fresh ring (:142-144), and that first call
 * therefore reports zeros.  A larger fft_avg, a moved or re-created bank start a fresh ring of zeros too.  window = fft_n floats, cached
 * by content.  LIMIT: the drop-in's banks are untuned, so this is the spectrum BEFORE downconvert()'s fine rotation; it is
 * narrowband_poll()'s only where chan->filter.remainder is zero.  Synchronous.  Returns fft_avg; -1 for a slave of an inline (small)
 * master, a REAL slave, a slave more than four blocks behind its master, bin_count > fft_n or other bad arguments, or an engine
 * library without the analyser. */
int ka9q_hip_spectrum_narrow(struct filter_out *slave, int fft_n, const float *window, int bin_count, int fft_avg, double overlap,
                             float *bin_data, double minmax[2]);
/* Pools of small REAL inline masters (default off; process-wide; affects masters created afterwards).  wfm's composite master
 * (src/wfm.c:70-89), stereod, rdsd, packetd and ctcss keep a REAL master of a few thousand points per channel or session with one to
 * three decimating slaves and run it inline; each is a full engine by default.  With the option on, a REAL master with an even
 * N = L + M - 1 <= 16384 starts as host state only, its COMPLEX / REAL slaves register as they are created, and at the first
 * execute_filter_output() it joins a pool shared by every master of its geometry (chz_rmini_*, include/chz_engine.h): one kernel
 * launch serves every thread that is due, and one request computes all slaves of its master, so that the siblings' calls for the
 * same block and shift are served from the host.  All slaves must exist before the master's first block; one the pool cannot serve (a
 * fifth slave, a block size with a prime factor above 13), or a first block with no slave at all, makes the master an engine in
 * place.  A pooled master is run INLINE whatever N_worker_threads says (master->perform_inline is set to true, as wfm, stereod, rdsd,
 * packetd and ctcss set it themselves): execute_filter_input() only book-keeps and the work is done in the slaves' calls; a process
 * that needs such a master's forward transform to run asynchronously leaves the option off.
 * Returns 1 if such masters will be pooled from now on, 0 if not (switched off, or an engine library without the pools). */
int ka9q_hip_pool_real_masters(int on);
/* engines the drop-in has created in this process so far (one per master and device; pooled inline masters create none) */
int ka9q_hip_engines_created(void);
/* pools of REAL inline masters that exist in this process; instances (may be NULL) receives how many of their instances are taken
   right now -- one per pooled master that still has its master or a slave alive */
int ka9q_hip_real_master_pools(int *instances);
#ifdef __cplusplus
}
#endif
#endif
