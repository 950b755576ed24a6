"""ctypes binding of include/chz_engine.h (libchz_hip.so).

There is deliberately no CPU fallback here: if the HIP library is missing or no
MI355X is visible, loading / engine creation raises.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CHZ_LIB") or os.path.join(HERE, "libchz_hip.so")   # CHZ_LIB: A/B builds only

COMPLEX, REAL = 1, 2
ND = 4

_vp, _i, _u, _d, _l = C.c_void_p, C.c_int, C.c_uint, C.c_double, C.c_long


class ChzInfo(C.Structure):
    _fields_ = [("L", _i), ("M", _i), ("N", _i), ("in_type", _i), ("bins", _i), ("ring_blocks", _i),
                ("Na", _i), ("Nb", _i), ("Nc", _i), ("n_banks", _i), ("lanes", _i), ("spec_elems", _l),
                ("spec_na", _i), ("spec_pitch", _i), ("spec_off", _i), ("plan", C.c_char * 320)]


class ChzTiming(C.Structure):
    _fields_ = [("total_ms", _d), ("blocks", _i),
                ("first_ms", _d), ("cols_ms", _d), ("rows_ms", _d), ("notch_ms", _d), ("chan_ms", _d),
                ("first_n", _i), ("cols_n", _i), ("rows_n", _i), ("notch_n", _i), ("chan_n", _i), ("enqueue_ms", _d),
                ("fix_ms", _d), ("fix_n", _i), ("demod_ms", _d), ("demod_n", _i)]


class DemodParams(C.Structure):
    """chz_demod_params: the chan_t members src/linear.c reads (linear amplitudes / power ratios)."""
    _fields_ = [("channels", _i), ("env", _i), ("agc", _i), ("encoding", _i), ("snr_squelch", _i), ("squelch_tail", _i),
                ("tuned", _i), ("kind", _i),
                ("samprate", _d), ("headroom", _d), ("threshold", _d), ("recovery_rate", _d), ("hangtime", _d), ("dc_alpha", _d),
                ("bandwidth", _d), ("shift", _d), ("squelch_open", _d), ("squelch_close", _d), ("gain", _d),
                ("deemph_rate", _d), ("deemph_gain", _d), ("threshold_extend", _d),
                ("pll_enable", _i), ("pll_square", _i), ("pll_loop_bw", _d), ("tone_freq", _d)]


class DemodStatus(C.Structure):
    _fields_ = [("frame", _i), ("mute", _i), ("squelch_state", _i), ("pll_lock", _i),
                ("output_power", _d), ("gain", _d), ("n0", _d), ("snr", _d), ("foffset", _d), ("pdeviation", _d),
                ("pll_snr", _d), ("pll_cphase", _d), ("tone_deviation", _d), ("pll_rotations", _i), ("tone_mute", _i)]


class WfmParams(C.Structure):
    """chz_wfm_params: the chan_t members src/wfm.c reads every block (linear amplitudes / power ratios)."""
    _fields_ = [("stereo_enable", _i), ("encoding", _i), ("squelch_tail", _i),
                ("squelch_open", _d), ("squelch_close", _d), ("bandwidth", _d), ("headroom", _d), ("deemph_rate", _d), ("deemph_gain", _d)]


class WfmStatus(C.Structure):
    _fields_ = [("frame", _i), ("mute", _i), ("squelch_state", _i), ("channels", _i), ("pilot_present", _i),
                ("snr", _d), ("foffset", _d), ("pdeviation", _d), ("output_power", _d), ("gain", _d), ("subc_amp", _d)]


class AfskStatus(C.Structure):
    """chz_afsk_status: one block of one packet decoder (bits: decision i in bit i, 1 = no transition)."""
    _fields_ = [("ndecisions", _i), ("symphase", _i), ("bits", C.c_ulonglong), ("last_val", _d), ("mid_val", _d),
                ("flag_seen", _i), ("frame_bits", _i), ("crc_failures", _i), ("nframes", _i), ("frame_len", _i * 2)]


class CtcssStatus(C.Structure):
    """chz_ctcss_status: one block of one PL tone decoder (indices into the pool's tone table, -1: none)."""
    _fields_ = [("tone_index", _i), ("current_index", _i), ("energy", _d)]


class MpxParams(C.Structure):
    """chz_mpx_params: stereod's Deemph_rate and Deemph_gain (an RDS pool ignores them)."""
    _fields_ = [("deemph_rate", _d), ("deemph_gain", _d)]


class MpxStatus(C.Structure):
    """chz_mpx_status: one block of one FM-multiplex decoder."""
    _fields_ = [("zero_pilot", _i), ("pad", _i), ("deemph_left", _d), ("deemph_right", _d)]


AFSK_BE, AFSK_LE = 0, 1
MPX_STEREO, MPX_RDS = 0, 1
MPX_BE, MPX_LE = 0, 1
CTCSS_BE, CTCSS_LE = 0, 1
CTCSS_TABLE_MAX = 64
# the table a CtcssPool searches when it is given none: ctcss's own (src/ctcss.c:62-69)
CTCSS_TONES = (67.0, 69.3, 71.9, 74.4, 77.0, 79.7, 82.5, 85.4, 88.5, 91.5, 94.8, 97.4, 100.0, 103.5, 107.2, 110.9, 114.8, 118.8, 123.0, 127.3,
               131.8, 136.5, 141.3, 146.2, 150.0, 151.4, 156.7, 159.8, 162.2, 165.5, 167.9, 171.3, 173.8, 177.3, 179.9, 183.5, 186.2, 189.9, 192.8,
               196.6, 199.5, 203.5, 206.5, 210.7, 213.8, 218.1, 221.3, 225.7, 229.1, 233.6, 237.1, 241.8, 245.5, 250.3, 254.1)
AFSK_FRAME_MAX = 16384
# chz_input_write_raw: CHZ_RAW_*, and the bytes a sample takes as (bytes, samples)
RAW_PACKED12, RAW_U16, RAW_S16, RAW_U8, RAW_S8, RAW_S16_IQ, RAW_U8_IQ, RAW_S8_IQ = range(8)
RAW_BYTES = {RAW_PACKED12: (12, 8), RAW_U16: (2, 1), RAW_S16: (2, 1), RAW_U8: (1, 1), RAW_S8: (1, 1), RAW_S16_IQ: (4, 1), RAW_U8_IQ: (2, 1), RAW_S8_IQ: (2, 1)}
SIGGEN_RUN = 64          # CHZ_SIGGEN_RUN: ring floats one lane of the generating kernel produces
PCM_S16BE, PCM_S16LE, PCM_F32LE, PCM_F32BE, PCM_MULAW, PCM_ALAW, PCM_F16LE, PCM_F16BE = 0, 1, 2, 3, 4, 5, 6, 7
FLAG_NO_SAMPLES, FLAG_MUTE, FLAG_PLL_LOCK, FLAG_TONE_MUTE, FLAG_PENDING = 1, 2, 4, 8, 16
FRAME_PENDING = 2        # DemodStatus.frame of a filter2 bank's pending block


class SigGenParams(C.Structure):
    """chz_siggen_params: sig_gen's stream (freq in cycles/sample, the argument of set_osc)"""
    _fields_ = [("freq", C.c_double), ("amplitude", C.c_double), ("noise", C.c_double), ("scale", C.c_double), ("seed", C.c_ulonglong)]


# every symbol include/chz_engine.h declares (checked by tests/test_host_logic.py and __graft_entry__.build())
SYMBOLS = [
    "chz_last_error", "chz_process_exiting", "chz_device_count", "chz_engine_create", "chz_engine_destroy", "chz_engine_info",
    "chz_engine_set_stream", "chz_sync", "chz_input_write", "chz_input_write_device", "chz_input_ring",
    "chz_forward", "chz_slot_stream", "chz_set_notches", "chz_spectrum_read", "chz_spectrum_device", "chz_spectrum_attach",
    "chz_bank_create", "chz_bank_create_shared", "chz_bank_set_rows", "chz_bank_set_row_responses", "chz_bank_set_responses", "chz_bank_set_shifts", "chz_bank_set_active",
    "chz_bank_execute", "chz_bank_execute_range", "chz_bank_destroy", "chz_bank_read", "chz_bank_read_async",
    "chz_spectrum_read_async", "chz_host_callback", "chz_host_alloc", "chz_host_free", "chz_host_register", "chz_host_unregister",
    "chz_bank_output_device", "chz_bank_write_block", "chz_bank_demod", "chz_bank_demod_auto", "chz_bank_read_pcm_flags_async", "chz_bank_pcm_wait",
    "chz_bank_read_pcm_open_async", "chz_bank_pcm_open_wait", "chz_bank_pcm_open_times", "chz_step", "chz_run_blocks", "chz_gather_descriptor",
    "chz_bank_set_tuning", "chz_bank_read_power", "chz_bank_read_power_async",
    "chz_input_write_i16", "chz_input_write_i16_device", "chz_input_stats",
    "chz_input_raw_check", "chz_input_write_raw", "chz_input_write_raw_device", "chz_input_raw_stats",
    "chz_siggen_check", "chz_siggen_jump", "chz_siggen_seed", "chz_input_siggen_set", "chz_input_siggen_seek", "chz_input_siggen_tell",
    "chz_input_generate", "chz_input_generate_stats",
    "chz_bank_enable_noise", "chz_bank_read_noise", "chz_bank_read_noise_async", "chz_bank_create_real", "chz_bank_set_isb", "chz_bank_set_beam",
    "chz_set_notches_alpha", "chz_slot_sync", "chz_engine_check", "chz_input_seek", "chz_input_mark", "chz_input_mark_wait", "chz_engine_notch_order",
    "chz_bank_set_demod", "chz_bank_pcm_stride", "chz_bank_set_pcm_stride", "chz_bank_read_pcm", "chz_bank_read_pcm_async",
    "chz_comm_unique_id", "chz_comm_create", "chz_comm_create_file", "chz_comm_destroy", "chz_comm_rank", "chz_comm_world",
    "chz_mini_create", "chz_mini_destroy", "chz_mini_capacity", "chz_mini_add", "chz_mini_release", "chz_mini_set_response", "chz_mini_execute",
    "chz_rmini_create", "chz_rmini_destroy", "chz_rmini_check", "chz_rmini_capacity", "chz_rmini_add", "chz_rmini_release", "chz_rmini_set_response", "chz_rmini_execute",
    "chz_wfm_check", "chz_wfm_create", "chz_wfm_destroy", "chz_wfm_capacity", "chz_wfm_geometry", "chz_wfm_add", "chz_wfm_release", "chz_wfm_set_params",
    "chz_wfm_set_response", "chz_wfm_execute",
    "chz_afsk_check", "chz_afsk_create", "chz_afsk_destroy", "chz_afsk_capacity", "chz_afsk_geometry", "chz_afsk_add", "chz_afsk_release",
    "chz_afsk_set_response", "chz_afsk_execute",
    "chz_ctcss_check", "chz_ctcss_create", "chz_ctcss_destroy", "chz_ctcss_capacity", "chz_ctcss_geometry", "chz_ctcss_add", "chz_ctcss_release",
    "chz_ctcss_set_response", "chz_ctcss_execute",
    "chz_mpx_check", "chz_mpx_create", "chz_mpx_destroy", "chz_mpx_capacity", "chz_mpx_geometry", "chz_mpx_add", "chz_mpx_release", "chz_mpx_set_params",
    "chz_mpx_set_response", "chz_mpx_execute",
    "chz_comm_barrier", "chz_comm_allreduce_max", "chz_spectrum_broadcast", "chz_spectrum_exchange_rows", "chz_run_blocks_sharded",
    "chz_comm_create_local", "chz_spectrum_broadcast_local", "chz_set_option",
    "chz_welch_create", "chz_welch_destroy", "chz_welch_set_window", "chz_welch_configure", "chz_welch_poll", "chz_welch_read", "chz_welch_read_async",
    "chz_bank_filter2_check", "chz_bank_set_filter2", "chz_bank_filter2_geometry", "chz_bank_set_filter2_responses", "chz_bank_set_filter2_isb",
    "chz_bank_filter2_reset", "chz_bank_filter2_read", "chz_bank_filter2_read_async",
    "chz_bank_welch_create", "chz_bank_welch_attach", "chz_bank_welch_detach", "chz_bank_welch_configure", "chz_bank_welch_poll", "chz_bank_welch_steps",
]

# the CHZ_* variables tests and scripts have always used to force a code path or arm a test hook: the shipped library does not read
# them (its options are set through chz_set_option, include/chz_engine.h) -- this mirror translates them whenever an engine, a pool
# or a communicator is created, so that a variable set by a test (monkeypatch.setenv) means what it always meant
ENV_OPTIONS = {"CHZ_CHAN_STAGE": "chan_stage", "CHZ_NOISE_ENERGY": "noise_energy", "CHZ_DEMOD_WAVE": "demod_wave", "CHZ_ENQ_THREADS": "enq_threads",
               "CHZ_GRAPH_BLOCKS": "graph_blocks", "CHZ_NOTCH_FOLD": "notch_fold", "CHZ_NOISE_HINT": "noise_hint", "CHZ_PLL_LANE0": "pll_lane0",
               "CHZ_NOTCH_WAIT_MS": "notch_wait_ms", "CHZ_FAULT_TICKET_SKEW": "fault_ticket_skew", "CHZ_ALLOW_FAULT_INJECTION": "allow_fault_injection",
               "CHZ_LAUNCH_ID": "launch_id"}


def apply_env_options():
    L = lib()
    for env, opt in ENV_OPTIONS.items():
        v = os.environ.get(env)
        _check(L.chz_set_option(opt.encode(), v.encode() if v is not None else None))

_lib = None


def lib():
    """Load libchz_hip.so (raises if it has not been built: run __graft_entry__.build())."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libchz_hip.so is missing: build it with `make -C ka9q-radio_amd/csrc` "
                               "(there is no CPU fallback)")
        L = C.CDLL(LIB_PATH)
        # tests/hipemu can build the engine's HOST code for the CPU (kernels on a fiber emulator) so that its orchestration is
        # testable without a GPU; such a library carries this symbol, and nothing but a test that says so may load it
        if hasattr(L, "chz_emulated_build") and os.environ.get("CHZ_ALLOW_EMULATED_ENGINE") != "1":
            raise RuntimeError("%s is a CPU-emulated TEST build of the engine: refusing to use it as the product "
                               "(there is no CPU fallback)" % LIB_PATH)
        L.chz_last_error.restype = C.c_char_p
        L.chz_set_option.argtypes = [C.c_char_p, C.c_char_p]
        L.chz_device_count.restype = _i
        L.chz_engine_create.argtypes = [C.POINTER(_vp), _i, _i, _i, _i, C.c_char_p, _i]
        L.chz_engine_destroy.argtypes = [_vp]; L.chz_engine_destroy.restype = None
        L.chz_engine_info.argtypes = [_vp, C.POINTER(ChzInfo)]
        L.chz_engine_set_stream.argtypes = [_vp, _vp]
        L.chz_sync.argtypes = [_vp]
        L.chz_input_write.argtypes = [_vp, _vp, _l]
        L.chz_input_write_device.argtypes = [_vp, _vp, _l]
        L.chz_input_ring.argtypes = [_vp, C.POINTER(_vp), C.POINTER(_l)]
        L.chz_input_write_i16.argtypes = [_vp, _vp, _l, C.c_float, _i]
        L.chz_input_write_i16_device.argtypes = [_vp, _vp, _l, C.c_float, _i]
        L.chz_input_stats.argtypes = [_vp, _i, C.POINTER(C.c_ulonglong), C.POINTER(C.c_uint)]
        L.chz_input_raw_check.argtypes = [_i, _i, _i, _l]
        L.chz_input_write_raw.argtypes = [_vp, _i, _i, _vp, _l, _d, C.POINTER(_u)]
        L.chz_input_write_raw_device.argtypes = [_vp, _i, _i, _vp, _l, _d, C.POINTER(_u)]
        L.chz_input_raw_stats.argtypes = [_vp, _u, C.POINTER(C.c_ulonglong), C.POINTER(_u), C.POINTER(_u)]
        L.chz_siggen_check.argtypes = [_i, C.POINTER(SigGenParams)]
        L.chz_siggen_jump.argtypes = [C.POINTER(C.c_ulonglong * 4), C.c_ulonglong, C.c_ulonglong]
        L.chz_siggen_seed.argtypes = [C.c_ulonglong, C.POINTER(C.c_ulonglong * 4)]
        L.chz_input_siggen_set.argtypes = [_vp, C.POINTER(SigGenParams)]
        L.chz_input_siggen_seek.argtypes = [_vp, C.c_ulonglong]
        L.chz_input_siggen_tell.argtypes = [_vp, C.POINTER(C.c_ulonglong)]
        L.chz_input_generate.argtypes = [_vp, _l, C.POINTER(_u)]
        L.chz_input_generate_stats.argtypes = [_vp, _u, C.POINTER(_d)]
        L.chz_forward.argtypes = [_vp, _u]
        L.chz_set_notches.argtypes = [_vp, _vp, _i, _d]
        L.chz_set_notches_alpha.argtypes = [_vp, _vp, _vp, _i]
        L.chz_slot_sync.argtypes = [_vp, _i]
        L.chz_engine_check.argtypes = [_vp]
        L.chz_bank_set_demod.argtypes = [_vp, _i, _u, _i, _i, _vp, _d]
        L.chz_bank_pcm_stride.argtypes = [_vp, _i]
        L.chz_bank_set_pcm_stride.argtypes = [_vp, _i, _i]
        L.chz_bank_read_pcm.argtypes = [_vp, _i, _i, _i, _i, _vp, _vp]
        L.chz_bank_read_pcm_async.argtypes = [_vp, _i, _i, _i, _i, _vp, _vp]
        L.chz_mini_create.argtypes = [C.POINTER(_vp), _i, _i, _i, _i]
        L.chz_mini_destroy.argtypes = [_vp]; L.chz_mini_destroy.restype = None
        L.chz_mini_capacity.argtypes = [_vp]
        L.chz_mini_add.argtypes = [_vp]
        L.chz_mini_release.argtypes = [_vp, _i]
        L.chz_mini_set_response.argtypes = [_vp, _i, _vp]
        L.chz_mini_execute.argtypes = [_vp, _i, _vp, _vp, _vp, _vp, _vp]
        L.chz_rmini_create.argtypes = [C.POINTER(_vp), _i, _i, _i, _vp, _vp, _i, _i]
        L.chz_rmini_destroy.argtypes = [_vp]; L.chz_rmini_destroy.restype = None
        L.chz_rmini_check.argtypes = [_i, _i, _i, _vp, _vp]
        L.chz_rmini_capacity.argtypes = [_vp]
        L.chz_rmini_add.argtypes = [_vp]
        L.chz_rmini_release.argtypes = [_vp, _i]
        L.chz_rmini_set_response.argtypes = [_vp, _i, _i, _vp]
        L.chz_rmini_execute.argtypes = [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp]
        L.chz_wfm_check.argtypes = [_d]
        L.chz_wfm_create.argtypes = [C.POINTER(_vp), _d, _i, _i]
        L.chz_wfm_destroy.argtypes = [_vp]; L.chz_wfm_destroy.restype = None
        L.chz_wfm_capacity.argtypes = [_vp]
        L.chz_wfm_geometry.argtypes = [_vp, C.POINTER(_i * 6)]
        L.chz_wfm_add.argtypes = [_vp]
        L.chz_wfm_release.argtypes = [_vp, _i]
        L.chz_wfm_set_params.argtypes = [_vp, _i, C.POINTER(WfmParams)]
        L.chz_wfm_set_response.argtypes = [_vp, _i, _i, _vp]
        L.chz_wfm_execute.argtypes = [_vp, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp]
        L.chz_afsk_check.argtypes = [_i, _i, _d, _d, _d, _d, _i]
        L.chz_afsk_create.argtypes = [C.POINTER(_vp), _i, _i, _d, _d, _d, _d, _i, _i, _i]
        L.chz_afsk_destroy.argtypes = [_vp]; L.chz_afsk_destroy.restype = None
        L.chz_afsk_capacity.argtypes = [_vp]
        L.chz_afsk_geometry.argtypes = [_vp, C.POINTER(_i * 4)]
        L.chz_afsk_add.argtypes = [_vp]
        L.chz_afsk_release.argtypes = [_vp, _i]
        L.chz_afsk_set_response.argtypes = [_vp, _i, _vp]
        L.chz_afsk_execute.argtypes = [_vp, _i, _vp, _vp, _i, _vp, _vp, _i]
        L.chz_ctcss_check.argtypes = [_d, _i, _i, _vp]
        L.chz_ctcss_create.argtypes = [C.POINTER(_vp), _d, _i, _i, _vp, _i, _i]
        L.chz_ctcss_destroy.argtypes = [_vp]; L.chz_ctcss_destroy.restype = None
        L.chz_ctcss_capacity.argtypes = [_vp]
        L.chz_ctcss_geometry.argtypes = [_vp, C.POINTER(_i * 7)]
        L.chz_ctcss_add.argtypes = [_vp]
        L.chz_ctcss_release.argtypes = [_vp, _i]
        L.chz_ctcss_set_response.argtypes = [_vp, _i, _vp]
        L.chz_ctcss_execute.argtypes = [_vp, _i, _vp, _vp, _i, _vp, _vp]
        L.chz_mpx_check.argtypes = [_d, _i, _i]
        L.chz_mpx_create.argtypes = [C.POINTER(_vp), _d, _i, _i, _i, _i]
        L.chz_mpx_destroy.argtypes = [_vp]; L.chz_mpx_destroy.restype = None
        L.chz_mpx_capacity.argtypes = [_vp]
        L.chz_mpx_geometry.argtypes = [_vp, C.POINTER(_i * 7)]
        L.chz_mpx_add.argtypes = [_vp]
        L.chz_mpx_release.argtypes = [_vp, _i]
        L.chz_mpx_set_params.argtypes = [_vp, _i, C.POINTER(MpxParams)]
        L.chz_mpx_set_response.argtypes = [_vp, _i, _i, _vp]
        L.chz_mpx_execute.argtypes = [_vp, _i, _vp, _vp, _i, _vp, _vp, _vp]
        L.chz_comm_unique_id.argtypes = [_vp]
        L.chz_comm_create.argtypes = [C.POINTER(_vp), _i, _i, _vp, _i]
        L.chz_comm_create_file.argtypes = [C.POINTER(_vp), _i, _i, C.c_char_p, _i, _d]
        L.chz_comm_destroy.argtypes = [_vp]; L.chz_comm_destroy.restype = None
        L.chz_comm_rank.argtypes = [_vp]
        L.chz_comm_world.argtypes = [_vp]
        L.chz_comm_barrier.argtypes = [_vp]
        L.chz_comm_allreduce_max.argtypes = [_vp, _vp, _i]
        L.chz_spectrum_broadcast.argtypes = [_vp, _vp, _i, _i]
        L.chz_spectrum_exchange_rows.argtypes = [_vp, _vp, _i, _i, _vp, _vp]
        L.chz_run_blocks_sharded.argtypes = [_vp, _vp, _i, _i, _vp, _vp, _u, _i, C.POINTER(ChzTiming)]
        L.chz_spectrum_read.argtypes = [_vp, _i, _vp]
        L.chz_spectrum_device.argtypes = [_vp, _i, C.POINTER(_vp)]
        L.chz_slot_stream.argtypes = [_vp, _i, C.POINTER(_vp)]
        L.chz_spectrum_attach.argtypes = [_vp, _i, _vp]
        L.chz_bank_create.argtypes = [_vp, _i, _i, _i]
        L.chz_bank_create_real.argtypes = [_vp, _i, _i, _i]
        L.chz_bank_set_isb.argtypes = [_vp, _i, _i, _i, _vp]
        L.chz_bank_set_beam.argtypes = [_vp, _i, _i, _i, _vp, _vp]
        L.chz_bank_set_responses.argtypes = [_vp, _i, _i, _i, _vp]
        L.chz_bank_set_shifts.argtypes = [_vp, _i, _i, _i, _vp]
        L.chz_bank_set_active.argtypes = [_vp, _i, _i]
        L.chz_bank_execute.argtypes = [_vp, _i, _u]
        L.chz_bank_read.argtypes = [_vp, _i, _i, _i, _vp]
        L.chz_bank_execute_range.argtypes = [_vp, _i, _u, _i, _i]
        L.chz_bank_set_tuning.argtypes = [_vp, _i, _u, _i, _i, _vp, _vp, _vp]
        L.chz_bank_read_power.argtypes = [_vp, _i, _i, _i, _i, _vp]
        L.chz_bank_read_power_async.argtypes = [_vp, _i, _i, _i, _i, _vp]
        L.chz_bank_enable_noise.argtypes = [_vp, _i, _d]
        L.chz_bank_read_noise.argtypes = [_vp, _i, _i, _i, _i, _vp]
        L.chz_bank_read_noise_async.argtypes = [_vp, _i, _i, _i, _i, _vp]
        L.chz_bank_destroy.argtypes = [_vp, _i]
        L.chz_bank_read_async.argtypes = [_vp, _i, _i, _i, _i, _vp]
        L.chz_bank_output_device.argtypes = [_vp, _i, _i, C.POINTER(_vp)]
        L.chz_step.argtypes = [_vp, _u]
        L.chz_run_blocks.argtypes = [_vp, _u, _i, _i, _i, C.POINTER(ChzTiming)]
        L.chz_gather_descriptor.argtypes = [_i, _i, _i, _i, C.POINTER(_i * 6)]
        L.chz_welch_create.argtypes = [_vp, _i, _i, _i, _i]
        L.chz_welch_destroy.argtypes = [_vp, _i]
        L.chz_welch_set_window.argtypes = [_vp, _i, _i, _vp]
        L.chz_welch_configure.argtypes = [_vp, _i, _i, _i, _i, _i, _d]
        L.chz_welch_poll.argtypes = [_vp, _i, _i, _vp, C.c_longlong]
        L.chz_welch_read.argtypes = [_vp, _i, _i, _i, _vp, _vp]
        L.chz_welch_read_async.argtypes = [_vp, _i, _i, _i, _vp, _vp]
        L.chz_bank_filter2_check.argtypes = [_i, _i, _i]
        L.chz_bank_set_filter2.argtypes = [_vp, _i, _u, _i, _i]
        L.chz_bank_filter2_geometry.argtypes = [_vp, _i, C.POINTER(_i * 3)]
        L.chz_bank_set_filter2_responses.argtypes = [_vp, _i, _i, _i, _vp]
        L.chz_bank_set_filter2_isb.argtypes = [_vp, _i, _i, _i, _vp]
        L.chz_bank_filter2_reset.argtypes = [_vp, _i, _u, _i, _i]
        L.chz_bank_filter2_read.argtypes = [_vp, _i, _i, _i, _i, _vp]
        L.chz_bank_filter2_read_async.argtypes = [_vp, _i, _i, _i, _i, _vp]
        L.chz_bank_welch_create.argtypes = [_vp, _i, _i, _i, _i, _i]
        L.chz_bank_welch_attach.argtypes = [_vp, _i, _i, _i, _u]
        L.chz_bank_welch_detach.argtypes = [_vp, _i, _i]
        L.chz_bank_welch_configure.argtypes = [_vp, _i, _i, _i, _i, _d]
        L.chz_bank_welch_poll.argtypes = [_vp, _i, _i, _vp, _u]
        L.chz_bank_welch_steps.argtypes = [_i, _i, _d, _u, _u, _i, C.c_longlong, C.POINTER(C.c_longlong * 3)]
        _lib = L
    return _lib


class ChzError(RuntimeError):
    pass


def _check(r):
    if r < 0:
        raise ChzError(lib().chz_last_error().decode())
    return r


def siggen_seed(seed=1):
    """The generator state sig_gen's stream starts from (xoshiro256ss_seed, src/gauss.c:32-45): four 64-bit words."""
    st = (C.c_ulonglong * 4)()
    _check(lib().chz_siggen_seed(int(seed) & 0xFFFFFFFFFFFFFFFF, C.byref(st)))
    return tuple(st)


def siggen_jump(state, draws):
    """The generator state `draws` (< 2^128) outputs after `state`; O(1), touches no device."""
    draws = int(draws)
    if not 0 <= draws < 1 << 128:
        raise ValueError("draws out of range")
    st = (C.c_ulonglong * 4)(*[int(w) for w in state])
    _check(lib().chz_siggen_jump(C.byref(st), draws & 0xFFFFFFFFFFFFFFFF, draws >> 64))
    return tuple(st)


def gather_descriptor(in_type, master_bins, P, shift):
    out = (_i * 6)()
    lib().chz_gather_descriptor(in_type, master_bins, P, int(shift), C.byref(out))
    return tuple(out)


class Engine:
    """One master (input half) on one GPU."""

    def __init__(self, L, M, in_type, device=0, plan="", ring_blocks=0):
        self._h = _vp()
        apply_env_options()
        _check(lib().chz_engine_create(C.byref(self._h), L, M, in_type, device,
                                       plan.encode() if plan else None, ring_blocks))
        info = ChzInfo()
        _check(lib().chz_engine_info(self._h, C.byref(info)))
        self.L, self.M, self.N, self.in_type, self.bins = info.L, info.M, info.N, info.in_type, info.bins
        self.ring_blocks = info.ring_blocks
        self.plan = info.plan.decode()
        self.axes = (info.Na, info.Nb, info.Nc)
        self.lanes = info.lanes
        self.spec_elems = info.spec_elems
        self.spec_layout = (info.spec_na, info.spec_pitch, info.spec_off)
        self.banks = []

    def close(self):
        if self._h:
            lib().chz_engine_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- input ---------------------------------------------------------------
    def write(self, samples):
        dt = np.float32 if self.in_type == REAL else np.complex64
        samples = np.ascontiguousarray(samples, dt)
        _check(lib().chz_input_write(self._h, samples.ctypes.data, samples.shape[0]))
        _check(lib().chz_sync(self._h))   # numpy buffer may be freed by the caller

    def write_i16(self, samples, scale, randomize=False):
        """Raw A/D samples (rx888.c's convert() + write_rfilter): int16, scaled on the device."""
        s = np.ascontiguousarray(samples, np.int16).reshape(-1)
        _check(lib().chz_input_write_i16(self._h, s.ctypes.data, s.size, float(scale), 1 if randomize else 0))
        self.sync()       # the caller's buffer may be pageable / reused

    def input_stats(self, slot):
        """(sum x^2, clipped samples) over the new samples of the block last transformed into `slot`."""
        en, cl = C.c_ulonglong(0), C.c_uint(0)
        _check(lib().chz_input_stats(self._h, slot, C.byref(en), C.byref(cl)))
        return en.value, cl.value

    def write_raw(self, samples, fmt, scale, bits=12, n=None):
        """Raw A/D samples of one of the RAW_* formats (airspy-unpack.c, hydrasdr.c's and rtlsdr.c's conversion loops), converted on the
        device into the float ring.  `samples`: an array of the format's own integers (uint32 words for RAW_PACKED12, I and Q interleaved
        for the I/Q formats) or its bytes; n: the sample count, where it is not all of them.  Returns the write's ticket (raw_stats)."""
        s = np.ascontiguousarray(samples).reshape(-1).view(np.uint8)
        num, den = RAW_BYTES.get(fmt, (1, 1))
        if n is None:
            n = s.size * den // num
        elif n > 0 and (n * num + den - 1) // den > s.size:
            raise ValueError("%d samples of format %d need more than the %d bytes given" % (n, fmt, s.size))
        t = _u(0)
        _check(lib().chz_input_write_raw(self._h, fmt, bits, s.ctypes.data, n, float(scale), C.byref(t)))
        self.sync()       # the caller's buffer may be pageable / reused
        return t.value

    def write_raw_device(self, dev_ptr, n, fmt, scale, bits=12):
        t = _u(0)
        _check(lib().chz_input_write_raw_device(self._h, fmt, bits, dev_ptr, n, float(scale), C.byref(t)))
        return t.value

    def raw_stats(self, ticket):
        """(sum of x^2, clipped samples, clipped components) of raw write `ticket`; the last 8 writes' can be read."""
        en, cs, cc = C.c_ulonglong(0), _u(0), _u(0)
        _check(lib().chz_input_raw_stats(self._h, ticket, C.byref(en), C.byref(cs), C.byref(cc)))
        return en.value, cs.value, cc.value

    def write_device(self, dev_ptr, n):
        _check(lib().chz_input_write_device(self._h, dev_ptr, n))

    def siggen(self, freq, amplitude, noise, scale, seed=1):
        """Describe sig_gen's stream (carrier of `freq` cycles/sample and `amplitude`, Gaussian noise of deviation `noise`, all times
        `scale`); the position goes to sample 0.  generate() then writes it into the ring on the device."""
        p = SigGenParams(float(freq), float(amplitude), float(noise), float(scale), int(seed) & 0xFFFFFFFFFFFFFFFF)
        _check(lib().chz_input_siggen_set(self._h, C.byref(p)))

    def siggen_seek(self, sample):
        if not 0 <= int(sample) < 1 << 64:
            raise ValueError("sample out of range")
        _check(lib().chz_input_siggen_seek(self._h, int(sample)))

    def siggen_tell(self):
        n = C.c_ulonglong(0)
        _check(lib().chz_input_siggen_tell(self._h, C.byref(n)))
        return n.value

    def generate(self, n):
        """Append the stream's next n samples at the ring's write position (asynchronous); returns the generate's ticket."""
        t = _u(0)
        _check(lib().chz_input_generate(self._h, int(n), C.byref(t)))
        return t.value

    def generate_energy(self, ticket):
        """Sum of samp^2 over generate `ticket`, samp before `scale`; the last 8 generates' can be read."""
        en = _d(0.0)
        _check(lib().chz_input_generate_stats(self._h, ticket, C.byref(en)))
        return en.value

    def ring(self):
        p, n = _vp(), _l()
        _check(lib().chz_input_ring(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def set_stream(self, hip_stream):
        _check(lib().chz_engine_set_stream(self._h, hip_stream))
        info = ChzInfo()
        _check(lib().chz_engine_info(self._h, C.byref(info)))
        self.lanes = info.lanes

    # -- forward ---------------------------------------------------------------
    def forward(self, job):
        _check(lib().chz_forward(self._h, job & 0xFFFFFFFF))

    def set_notches(self, bins, alpha=0.01):
        """alpha: one gain for the whole list, or one per entry (struct notch_state, src/filter.h:42-46)."""
        bins = np.ascontiguousarray(bins, np.int32)
        if np.ndim(alpha) == 0:
            _check(lib().chz_set_notches(self._h, bins.ctypes.data if len(bins) else None, len(bins), float(alpha)))
        else:
            al = np.ascontiguousarray(alpha, np.float64).reshape(-1)
            assert al.shape[0] == bins.shape[0]
            _check(lib().chz_set_notches_alpha(self._h, bins.ctypes.data if len(bins) else None,
                                               al.ctypes.data if len(bins) else None, len(bins)))

    def check(self):
        """Raises once a device-side consistency check (the notch ticket) has failed."""
        _check(lib().chz_engine_check(self._h))

    def slot_sync(self, slot):
        _check(lib().chz_slot_sync(self._h, slot))

    def run_blocks_sharded(self, comm, job0, nblocks, root=0, rows=None, samples=False):
        """BASELINE config 4: the root transforms, the spectrum travels over RCCL (whole slot, or the row ranges
        rows = (lo[world], hi[world])), every rank runs its own banks.  samples=True: the block's new samples travel
        instead and every rank transforms them itself (SURVEY 8e's alternative)."""
        t = ChzTiming()
        if samples:
            _check(lib().chz_run_blocks_sharded(self._h, comm._h, root, 2, None, None, job0 & 0xFFFFFFFF, nblocks, C.byref(t)))
        elif rows is None:
            _check(lib().chz_run_blocks_sharded(self._h, comm._h, root, 0, None, None, job0 & 0xFFFFFFFF, nblocks, C.byref(t)))
        else:
            lo = np.ascontiguousarray(rows[0], np.int32); hi = np.ascontiguousarray(rows[1], np.int32)
            _check(lib().chz_run_blocks_sharded(self._h, comm._h, root, 1, lo.ctypes.data, hi.ctypes.data,
                                                job0 & 0xFFFFFFFF, nblocks, C.byref(t)))
        return t

    def spectrum(self, slot):
        out = np.zeros(self.bins, np.complex64)
        _check(lib().chz_spectrum_read(self._h, slot, out.ctypes.data))
        return out

    def spectrum_ptr(self, slot):
        p = _vp()
        _check(lib().chz_spectrum_device(self._h, slot, C.byref(p)))
        return p.value

    def slot_stream(self, slot):
        p = _vp()
        _check(lib().chz_slot_stream(self._h, slot, C.byref(p)))
        return p.value or 0

    def attach_spectrum(self, slot, dev_ptr):
        _check(lib().chz_spectrum_attach(self._h, slot, dev_ptr))

    # -- banks -----------------------------------------------------------------
    def bank(self, P, olen, capacity, real=False, shared_rows=0):
        b = Bank(self, P, olen, capacity, real, shared_rows)
        self.banks.append(b)
        return b

    def welch(self, fft_n, capacity, max_bins, max_avg, packed=None):
        """A bank of wideband spectrum analysers (wideband_poll(), src/spectrum.c:308-522) on the samples of the input ring.
        packed: None = the library's default; True / False = option welch_packed for this bank (real front end, even fft_n:
        half-length packed transform with a Hermitian split instead of the full-length complex transform)."""
        if packed is not None:
            _check(lib().chz_set_option(b"welch_packed", b"1" if packed else b"0"))
        try:
            return Welch(self, fft_n, capacity, max_bins, max_avg)
        finally:
            if packed is not None:
                _check(lib().chz_set_option(b"welch_packed", None))

    def step(self, job):
        _check(lib().chz_step(self._h, job & 0xFFFFFFFF))

    def sync(self):
        _check(lib().chz_sync(self._h))

    def run_blocks(self, job0, nblocks, graph=False, instrument=False):
        t = ChzTiming()
        _check(lib().chz_run_blocks(self._h, job0 & 0xFFFFFFFF, nblocks, 1 if graph else 0,
                                    1 if instrument else 0, C.byref(t)))
        return t


class Bank:
    def __init__(self, eng, P, olen, capacity, real=False, shared_rows=0):
        self.eng, self.P, self.olen, self.capacity, self.real = eng, P, olen, capacity, bool(real)
        L = lib()
        if shared_rows:                                                            # channels name one of `shared_rows` response rows
            L.chz_bank_create_shared.argtypes = [_vp, _i, _i, _i, _i]
            L.chz_bank_set_rows.argtypes = [_vp, _i, _i, _i, _vp]
            L.chz_bank_set_row_responses.argtypes = [_vp, _i, _i, _i, _vp]
            self.id = _check(L.chz_bank_create_shared(eng._h, P, olen, capacity, shared_rows))
        else:
            make = L.chz_bank_create_real if real else L.chz_bank_create          # REAL- or COMPLEX-output slaves
            self.id = _check(make(eng._h, P, olen, capacity))
        self._dtype = np.float32 if real else np.complex64
        self.active = 0

    def destroy(self):
        """Free the bank's device arrays (the id stays reserved)."""
        if self.id is not None and self.eng._h:
            _check(lib().chz_bank_destroy(self.eng._h, self.id))
        self.id = None

    def set_rows(self, ch0, rows):
        r = np.ascontiguousarray(rows, np.int32)
        _check(lib().chz_bank_set_rows(self.eng._h, self.id, ch0, r.shape[0], r.ctypes.data))

    def set_row_responses(self, row0, resp):
        r = np.ascontiguousarray(resp, np.complex64)
        assert r.ndim == 2 and r.shape[1] == self.P
        _check(lib().chz_bank_set_row_responses(self.eng._h, self.id, row0, r.shape[0], r.ctypes.data))

    def set_responses(self, ch0, resp):
        resp = np.ascontiguousarray(resp, np.complex64).reshape(-1, self.P)
        _check(lib().chz_bank_set_responses(self.eng._h, self.id, ch0, resp.shape[0], resp.ctypes.data))

    def set_shifts(self, ch0, shifts):
        shifts = np.ascontiguousarray(shifts, np.int32).reshape(-1)
        _check(lib().chz_bank_set_shifts(self.eng._h, self.id, ch0, shifts.shape[0], shifts.ctypes.data))

    def set_isb(self, ch0, flags):
        """slave->isb per channel (src/filter.c:895-909)."""
        f = np.ascontiguousarray(flags, np.uint8).reshape(-1)
        _check(lib().chz_bank_set_isb(self.eng._h, self.id, ch0, f.shape[0], f.ctypes.data))

    def set_beam(self, ch0, alpha, beta, on):
        """slave->beam with slave->alpha / ->beta per channel (src/filter.c:756-775)."""
        alpha = np.asarray(alpha, np.complex128).reshape(-1); beta = np.asarray(beta, np.complex128).reshape(-1)
        ab = np.ascontiguousarray(np.stack([alpha.real, alpha.imag, beta.real, beta.imag], axis=1), np.float64)
        f = np.ascontiguousarray(on, np.uint8).reshape(-1)
        assert ab.shape[0] == f.shape[0]
        _check(lib().chz_bank_set_beam(self.eng._h, self.id, ch0, f.shape[0], ab.ctypes.data, f.ctypes.data))

    def set_active(self, n):
        _check(lib().chz_bank_set_active(self.eng._h, self.id, n))
        self.active = n

    def execute(self, job):
        """Run the bank on the spectrum of block `job` (slot job % 4; a bare slot number is fine for an untuned bank)."""
        _check(lib().chz_bank_execute(self.eng._h, self.id, job & 0xFFFFFFFF))

    def execute_range(self, job, ch0, n):
        """The same for channels [ch0, ch0+n) only (the slow path of one retuned channel)."""
        _check(lib().chz_bank_execute_range(self.eng._h, self.id, job & 0xFFFFFFFF, ch0, n))

    def set_tuning(self, job, ch0, shifts, freq, rate=None):
        """downconvert()'s tuning update (src/radio.c:1479-1497) taking effect at block `job`:
        shifts[i] bins, freq[i] = -remainder/samprate cycles/sample, rate[i] = doppler_rate/samprate^2."""
        shifts = np.ascontiguousarray(shifts, np.int32).reshape(-1)
        freq = np.ascontiguousarray(freq, np.float64).reshape(-1)
        assert freq.shape == shifts.shape
        rp = None
        if rate is not None:
            rate = np.ascontiguousarray(rate, np.float64).reshape(-1)
            assert rate.shape == shifts.shape
            rp = rate.ctypes.data
        _check(lib().chz_bank_set_tuning(self.eng._h, self.id, job & 0xFFFFFFFF, ch0, shifts.shape[0],
                                         shifts.ctypes.data, freq.ctypes.data, rp))

    def set_demod(self, job, ch0, params, blocktime=0.02):
        """demod_linear()'s per-block work (src/linear.c) for channels ch0.. from block `job`; params: list of DemodParams."""
        arr = (DemodParams * len(params))(*params)
        _check(lib().chz_bank_set_demod(self.eng._h, self.id, job & 0xFFFFFFFF, ch0, len(params), arr, float(blocktime)))

    def set_pcm_stride(self, nbytes):
        _check(lib().chz_bank_set_pcm_stride(self.eng._h, self.id, int(nbytes)))

    def read_pcm(self, slot, ch0=0, n=None):
        """(pcm uint8[n][stride], status DemodStatus[n]) of the block last demodulated on `slot`."""
        if n is None:
            n = self.active - ch0
        stride = _check(lib().chz_bank_pcm_stride(self.eng._h, self.id))
        pcm = np.zeros((n, stride), np.uint8)
        st = (DemodStatus * n)()
        _check(lib().chz_bank_read_pcm(self.eng._h, self.id, slot, ch0, n, pcm.ctypes.data, st))
        return pcm, st

    def inject(self, slot, samples, bb_power=None, n0=None, ch0=0):
        """chz_bank_write_block: complex64[n][olen] (+ float64[n] bb_power, noise estimates) into the slot's output image."""
        x = np.ascontiguousarray(samples, np.complex64)
        pw = None if bb_power is None else np.ascontiguousarray(bb_power, np.float64)
        ne = None if n0 is None else np.ascontiguousarray(n0, np.float64)
        L = lib()
        L.chz_bank_write_block.argtypes = [_vp, _i, _i, _i, _i, _vp, _vp, _vp]
        _check(L.chz_bank_write_block(self.eng._h, self.id, slot, ch0, x.shape[0], x.ctypes.data,
                                      None if pw is None else pw.ctypes.data, None if ne is None else ne.ctypes.data))

    def demod_auto(self, on):
        L = lib()
        L.chz_bank_demod_auto.argtypes = [_vp, _i, _i]
        _check(L.chz_bank_demod_auto(self.eng._h, self.id, 1 if on else 0))

    def demod_only(self, job, slot=None):
        """chz_bank_demod: the demodulator stage alone over what `slot` (default job % 4) holds."""
        L = lib()
        L.chz_bank_demod.argtypes = [_vp, _i, C.c_uint, _i]
        _check(L.chz_bank_demod(self.eng._h, self.id, job, job % 4 if slot is None else slot))

    def read_pcm_flags(self, slot, ch0=0, n=None):
        """(pcm uint8[n][stride], flags uint8[n]): chz_bank_read_pcm_flags_async + chz_sync of the demodulator stream."""
        if n is None:
            n = self.active - ch0
        stride = _check(lib().chz_bank_pcm_stride(self.eng._h, self.id))
        pcm = np.zeros((n, stride), np.uint8); fl = np.zeros(n, np.uint8)
        L = lib()
        L.chz_bank_read_pcm_flags_async.argtypes = [_vp, _i, _i, _i, _i, _vp, _vp]
        _check(L.chz_bank_read_pcm_flags_async(self.eng._h, self.id, slot, ch0, n, pcm.ctypes.data, fl.ctypes.data))
        self.eng.sync()
        return pcm, fl

    def read_pcm_open(self, slot, ch0=0, n=None, max_rows=None):
        """(count, index int32[k], pcm uint8[k][stride], flags uint8[n]), k = min(count, max_rows): the rows of the open channels of
        [ch0, ch0+n) only -- demodulator on, flag byte without NO_SAMPLES, MUTE and PENDING -- dense and in ascending channel order
        (chz_bank_read_pcm_open_async + chz_bank_pcm_open_wait).  max_rows defaults to n."""
        if n is None:
            n = self.active - ch0
        if max_rows is None:
            max_rows = n
        stride = _check(lib().chz_bank_pcm_stride(self.eng._h, self.id))
        pcm = np.zeros((max(max_rows, 0), stride), np.uint8); idx = np.zeros(max(max_rows, 0), np.int32); fl = np.zeros(max(n, 0), np.uint8)
        cnt = C.c_int(0)
        L = lib()
        L.chz_bank_read_pcm_open_async.argtypes = [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _i]
        L.chz_bank_pcm_open_wait.argtypes = [_vp, _i, _i, C.POINTER(C.c_int)]
        _check(L.chz_bank_read_pcm_open_async(self.eng._h, self.id, slot, ch0, n, pcm.ctypes.data, idx.ctypes.data, fl.ctypes.data, max_rows))
        _check(L.chz_bank_pcm_open_wait(self.eng._h, self.id, slot, C.byref(cnt)))
        k = min(cnt.value, max_rows)
        return cnt.value, idx[:k], pcm[:k], fl

    def enable_noise(self, samprate):
        """estimate_noise() (src/radio.c:1783-1866) on the device after every block; samprate = front-end rate in Hz."""
        _check(lib().chz_bank_enable_noise(self.eng._h, self.id, float(samprate)))

    def read_noise(self, slot, ch0=0, n=None):
        if n is None:
            n = self.active - ch0
        out = np.zeros(n, np.float64)
        _check(lib().chz_bank_read_noise(self.eng._h, self.id, slot, ch0, n, out.ctypes.data))
        return out

    def read_power(self, slot, ch0=0, n=None):
        """chan->sig.bb_power of the block last executed on `slot` (src/radio.c:1516-1520)."""
        if n is None:
            n = self.active - ch0
        out = np.zeros(n, np.float64)
        _check(lib().chz_bank_read_power(self.eng._h, self.id, slot, ch0, n, out.ctypes.data))
        return out

    def read(self, ch0=0, n=None):
        if n is None:
            n = self.active - ch0
        out = np.zeros((n, self.olen), self._dtype)
        _check(lib().chz_bank_read(self.eng._h, self.id, ch0, n, out.ctypes.data))
        return out

    def read_slot(self, slot, ch0=0, n=None):
        """Outputs of the block last executed on spectrum slot `slot` (every slot keeps its own image)."""
        if n is None:
            n = self.active - ch0
        out = np.zeros((n, self.olen), self._dtype)
        _check(lib().chz_bank_read_async(self.eng._h, self.id, slot, ch0, n, out.ctypes.data))
        self.eng.sync()
        return out

    # ---- filter2 resident on the device (chz_bank_set_filter2 & co., include/chz_engine.h)
    @staticmethod
    def filter2_check(olen, blocking, M2=0):
        """Would set_filter2 take this geometry?  Raises ChzError with the reason if not; touches no device."""
        _check(lib().chz_bank_filter2_check(int(olen), int(blocking), int(M2)))

    def set_filter2(self, job0, blocking, M2=0):
        """The channels' private second filter (src/radio.c:1503-1513) as a stage of the block pipeline: cycles of `blocking` blocks
        from block job0 on, M2 = 0 for radiod's own impulse length.  Returns (L2, M2, N2)."""
        _check(lib().chz_bank_set_filter2(self.eng._h, self.id, job0 & 0xFFFFFFFF, int(blocking), int(M2)))
        return self.filter2_geometry()

    def filter2_geometry(self):
        out = (_i * 3)()
        _check(lib().chz_bank_filter2_geometry(self.eng._h, self.id, C.byref(out)))
        return tuple(out)

    def set_filter2_responses(self, ch0, resp):
        """complex64[n][N2] as set_filter leaves them; in stream order from the next block enqueued."""
        r = np.ascontiguousarray(resp, np.complex64).reshape(-1, self.filter2_geometry()[2])
        _check(lib().chz_bank_set_filter2_responses(self.eng._h, self.id, ch0, r.shape[0], r.ctypes.data))

    def set_filter2_isb(self, ch0, flags):
        f = np.ascontiguousarray(flags, np.uint8).reshape(-1)
        _check(lib().chz_bank_set_filter2_isb(self.eng._h, self.id, ch0, f.shape[0], f.ctypes.data))

    def filter2_reset(self, job, ch0=0, n=None):
        """Zero the windows of channels [ch0, ch0+n) from block `job` on: the next block, and the first of a cycle."""
        if n is None:
            n = self.active - ch0
        _check(lib().chz_bank_filter2_reset(self.eng._h, self.id, job & 0xFFFFFFFF, ch0, n))

    def read_filter2(self, slot, ch0=0, n=None):
        """complex64[n][L2]: filter2's output of the block that fired on `slot` (ChzError if the slot's last block was pending)."""
        if n is None:
            n = self.active - ch0
        out = np.zeros((n, self.filter2_geometry()[0]), np.complex64)
        _check(lib().chz_bank_filter2_read(self.eng._h, self.id, slot, ch0, n, out.ctypes.data))
        return out

    def output_ptr(self, slot=0):
        p = _vp()
        _check(lib().chz_bank_output_device(self.eng._h, self.id, slot, C.byref(p)))
        return p.value

    def spectrum(self, fft_n, capacity, max_bins, max_avg):
        """A bank of narrowband spectrum analysers (narrowband_poll(), src/spectrum.c:206-306) on the baseband of this bank's channels."""
        return BankSpectrum(self, fft_n, capacity, max_bins, max_avg)


class Welch:
    """chz_welch_*: `capacity` analysers sharing one fft_n; one poll serves any number of them."""

    def __init__(self, eng, fft_n, capacity, max_bins, max_avg):
        self._setup(eng, fft_n, capacity, max_bins, max_avg, lib().chz_welch_create(eng._h, fft_n, capacity, max_bins, max_avg))

    def _setup(self, eng, fft_n, capacity, max_bins, max_avg, bank_id):
        """the state both kinds of bank share (read, set_window and close use nothing else)"""
        self.eng, self.fft_n, self.capacity, self.max_bins, self.max_avg = eng, fft_n, capacity, max_bins, max_avg
        self.id = _check(bank_id)
        self.bin_count = [0] * capacity
        self.fft_avg = [0] * capacity
        self._polled = []

    def set_window(self, slot, window):
        w = np.ascontiguousarray(window, np.float32).reshape(-1)
        assert w.shape[0] == self.fft_n
        _check(lib().chz_welch_set_window(self.eng._h, self.id, slot, w.ctypes.data))

    def configure(self, slot, shift, bin_count, fft_avg, overlap):
        """Returns the effective fft_avg (limited to the data the device ring holds, src/spectrum.c:359-361)."""
        eff = _check(lib().chz_welch_configure(self.eng._h, self.id, slot, int(shift), int(bin_count), int(fft_avg), float(overlap)))
        self.bin_count[slot], self.fft_avg[slot] = int(bin_count), eff
        return eff

    def poll(self, slots=None, end=None):
        """slots: analysers to serve (default: every configured one); end: ring position just past the newest sample of the
        window (default: everything written so far).  Asynchronous; read() waits."""
        if slots is None:
            slots = [s for s in range(self.capacity) if self.fft_avg[s] > 0]
        sl = np.ascontiguousarray(slots, np.int32).reshape(-1)
        self._polled = [int(s) for s in sl]
        if sl.shape[0]:
            _check(lib().chz_welch_poll(self.eng._h, self.id, sl.shape[0], sl.ctypes.data, -1 if end is None else int(end)))

    def read(self, slots=None):
        """(bins, minmax): per analyser of the latest poll (or of `slots`) its bin_count float32 bins in the reference's FFT order
        and float64 (min_power, max_power)."""
        if slots is None:
            slots = getattr(self, "_polled", [])
        rows = np.zeros((self.capacity, self.max_bins), np.float32)
        mm = np.zeros((self.capacity, 2), np.float64)
        _check(lib().chz_welch_read(self.eng._h, self.id, 0, self.capacity, rows.ctypes.data, mm.ctypes.data))
        return [rows[s, :self.bin_count[s]].copy() for s in slots], [mm[s].copy() for s in slots]

    def close(self):
        if self.id is not None and self.eng._h:
            _check(lib().chz_welch_destroy(self.eng._h, self.id))
        self.id = None


class BankSpectrum(Welch):
    """chz_bank_welch_*: `capacity` analysers sharing one fft_n, each attached to one channel of a COMPLEX-output bank whose rows
    the device keeps in a ring per analyser; set_window, read and close are Welch's."""

    def __init__(self, bank, fft_n, capacity, max_bins, max_avg):
        self.bank = bank
        self._setup(bank.eng, fft_n, capacity, max_bins, max_avg, lib().chz_bank_welch_create(bank.eng._h, bank.id, fft_n, capacity, max_bins, max_avg))

    def attach(self, slot, channel, job0):
        """Analyser `slot` follows `channel` from block job0 on; its history starts as zeros."""
        _check(lib().chz_bank_welch_attach(self.eng._h, self.id, slot, channel, job0 & 0xFFFFFFFF))

    def detach(self, slot):
        _check(lib().chz_bank_welch_detach(self.eng._h, self.id, slot))

    def configure(self, slot, bin_count, fft_avg, overlap):
        eff = _check(lib().chz_bank_welch_configure(self.eng._h, self.id, slot, int(bin_count), int(fft_avg), float(overlap)))
        self.bin_count[slot], self.fft_avg[slot] = int(bin_count), eff
        return eff

    def poll(self, slots=None, job=0):
        """slots: analysers to serve (default: every configured one); the window ends just past block `job`.  Asynchronous; read() waits."""
        if slots is None:
            slots = [s for s in range(self.capacity) if self.fft_avg[s] > 0]
        sl = np.ascontiguousarray(slots, np.int32).reshape(-1)
        self._polled = [int(s) for s in sl]
        if sl.shape[0]:
            _check(lib().chz_bank_welch_poll(self.eng._h, self.id, sl.shape[0], sl.ctypes.data, job & 0xFFFFFFFF))


COMM_ID_BYTES = 128


def comm_unique_id():
    """Rank 0: the 128-byte id every rank passes to Comm()."""
    buf = (C.c_ubyte * COMM_ID_BYTES)()
    _check(lib().chz_comm_unique_id(buf))
    return bytes(buf)


class Comm:
    """One RCCL communicator per process (one process per GPU), behind the engine's C ABI."""

    def __init__(self, rank, world, uid=None, device=0, path=None, timeout_s=120.0):
        self._h = _vp()
        if path is not None:
            apply_env_options()
            _check(lib().chz_comm_create_file(C.byref(self._h), rank, world, path.encode(), device, float(timeout_s)))
        else:
            buf = (C.c_ubyte * COMM_ID_BYTES).from_buffer_copy(uid)
            _check(lib().chz_comm_create(C.byref(self._h), rank, world, buf, device))
        self.rank, self.world = rank, world

    def barrier(self):
        _check(lib().chz_comm_barrier(self._h))

    def allreduce_max(self, values):
        v = np.ascontiguousarray(values, np.float64).reshape(-1).copy()
        _check(lib().chz_comm_allreduce_max(self._h, v.ctypes.data, v.shape[0]))
        return v

    def broadcast_spectrum(self, eng, slot, root=0):
        _check(lib().chz_spectrum_broadcast(eng._h, self._h, slot, root))

    def exchange_rows(self, eng, slot, lo, hi, root=0):
        lo = np.ascontiguousarray(lo, np.int32); hi = np.ascontiguousarray(hi, np.int32)
        _check(lib().chz_spectrum_exchange_rows(eng._h, self._h, slot, root, lo.ctypes.data, hi.ctypes.data))

    def close(self):
        if self._h:
            lib().chz_comm_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MiniPool:
    """Pool of small inline masters of one geometry (radiod's filter2, src/radio.c:1572-1594)."""

    def __init__(self, L, M, capacity, device=0):
        self._h = _vp()
        _check(lib().chz_mini_create(C.byref(self._h), L, M, capacity, device))
        self.L, self.M, self.N, self.capacity = L, M, L + M - 1, capacity

    def add(self):
        return _check(lib().chz_mini_add(self._h))

    def release(self, inst):
        _check(lib().chz_mini_release(self._h, inst))

    def set_response(self, inst, resp):
        r = np.ascontiguousarray(resp, np.complex64).reshape(-1)
        assert r.shape[0] == self.N
        _check(lib().chz_mini_set_response(self._h, inst, r.ctypes.data))

    def execute(self, insts, windows, shifts=None, isb=None):
        """windows: [n][N] complex64 (M-1 old + L new samples each) -> [n][L] complex64."""
        insts = np.ascontiguousarray(insts, np.int32)
        n = insts.shape[0]
        win = np.ascontiguousarray(windows, np.complex64).reshape(n, self.N)
        out = np.zeros((n, self.L), np.complex64)
        wp = (_vp * n)(*[win[i].ctypes.data for i in range(n)])
        op = (_vp * n)(*[out[i].ctypes.data for i in range(n)])
        sh = np.ascontiguousarray(shifts, np.int32) if shifts is not None else None
        fl = np.ascontiguousarray(isb, np.uint8) if isb is not None else None
        _check(lib().chz_mini_execute(self._h, n, insts.ctypes.data, wp, sh.ctypes.data if sh is not None else None,
                                      fl.ctypes.data if fl is not None else None, op))
        return out

    def close(self):
        if self._h:
            lib().chz_mini_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RealMiniPool:
    """Pool of small REAL inline masters of one geometry with their decimating slaves (wfm, stereod, rdsd, packetd, ctcss).

    slaves: list of (olen, out_type) with out_type 1 = COMPLEX, 2 = REAL."""

    def __init__(self, L, M, slaves, capacity, device=0):
        self._h = _vp()
        ol = np.ascontiguousarray([s[0] for s in slaves], np.int32)
        ot = np.ascontiguousarray([s[1] for s in slaves], np.int32)
        _check(lib().chz_rmini_create(C.byref(self._h), L, M, len(slaves), ol.ctypes.data, ot.ctypes.data, capacity, device))
        self.L, self.M, self.N, self.capacity = L, M, L + M - 1, capacity
        self.slaves = [(int(a), int(b)) for a, b in slaves]
        self.P = [self.N * a // L for a, _ in self.slaves]

    @staticmethod
    def check(L, M, slaves):
        """Would a pool of this geometry be created?  Raises ChzError with the reason if not; touches no device."""
        ol = np.ascontiguousarray([s[0] for s in slaves], np.int32)
        ot = np.ascontiguousarray([s[1] for s in slaves], np.int32)
        _check(lib().chz_rmini_check(L, M, len(slaves), ol.ctypes.data, ot.ctypes.data))

    def add(self):
        return _check(lib().chz_rmini_add(self._h))

    def release(self, inst):
        _check(lib().chz_rmini_release(self._h, inst))

    def set_response(self, inst, slave, resp):
        r = np.ascontiguousarray(resp, np.complex64).reshape(-1)
        assert r.shape[0] == self.P[slave]
        _check(lib().chz_rmini_set_response(self._h, inst, slave, r.ctypes.data))

    def execute(self, insts, windows, shifts=None, mask=None, isb=None, out=None):
        """windows: [n][N] float32 (M-1 old + L new samples each); shifts, isb: [n][nslaves]; mask: [n] bit s = run slave s.
        Returns one array per slave, [n][olen_s] complex64 or float32; rows of slaves the mask leaves out keep what `out` held."""
        insts = np.ascontiguousarray(insts, np.int32)
        n, ns = insts.shape[0], len(self.slaves)
        win = np.ascontiguousarray(windows, np.float32).reshape(n, self.N)
        if out is None:
            out = [np.zeros((n, a), np.complex64 if t == 1 else np.float32) for a, t in self.slaves]
        wp = (_vp * n)(*[win[i].ctypes.data for i in range(n)])
        op = (_vp * (n * ns))(*[out[s][i].ctypes.data for i in range(n) for s in range(ns)])
        sh = np.ascontiguousarray(shifts, np.int32).reshape(n, ns) if shifts is not None else None
        mk = np.ascontiguousarray(mask, np.uint8).reshape(n) if mask is not None else None
        fl = np.ascontiguousarray(isb, np.uint8).reshape(n, ns) if isb is not None else None
        _check(lib().chz_rmini_execute(self._h, n, insts.ctypes.data, wp, sh.ctypes.data if sh is not None else None,
                                       mk.ctypes.data if mk is not None else None, fl.ctypes.data if fl is not None else None, op))
        return out

    def close(self):
        if self._h:
            lib().chz_rmini_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


PCM_SAMPLE_BYTES = {PCM_S16BE: 2, PCM_S16LE: 2, PCM_F32LE: 4, PCM_F32BE: 4, PCM_MULAW: 1, PCM_ALAW: 1, PCM_F16LE: 2, PCM_F16BE: 2}


class WfmPool:
    """Pool of stereo broadcast-FM decoders of one block time (demod_wfm(), src/wfm.c): baseband in, packed PCM and a status record out."""

    def __init__(self, blocktime, capacity, device=0):
        self._h = _vp()
        _check(lib().chz_wfm_create(C.byref(self._h), float(blocktime), capacity, device))
        g = (_i * 6)()
        _check(lib().chz_wfm_geometry(self._h, C.byref(g)))
        self.geometry = dict(zip(("L", "N", "olen", "P", "pilot_shift", "subc_shift"), (int(v) for v in g)))
        self.L, self.N, self.olen, self.P = (self.geometry[k] for k in ("L", "N", "olen", "P"))
        self.blocktime, self.capacity = float(blocktime), capacity
        self._enc = {}

    @staticmethod
    def check(blocktime):
        """Would a pool of this block time be created?  Raises ChzError with the reason if not; touches no device."""
        _check(lib().chz_wfm_check(float(blocktime)))

    def add(self):
        return _check(lib().chz_wfm_add(self._h))

    def release(self, inst):
        _check(lib().chz_wfm_release(self._h, inst))
        self._enc.pop(inst, None)

    def set_params(self, inst, params):
        _check(lib().chz_wfm_set_params(self._h, inst, C.byref(params)))
        self._enc[inst] = int(params.encoding)

    def set_response(self, inst, slave, resp):
        r = np.ascontiguousarray(resp, np.complex64).reshape(-1)
        assert r.shape[0] == self.P
        _check(lib().chz_wfm_set_response(self._h, inst, slave, r.ctypes.data))

    def execute(self, insts, bb, bb_power, n0, on_device=False, fill=0):
        """bb: [n][L] complex64 on the host (an array, or a list of n rows of which one may be None: a null row, which the call refuses),
        or (on_device) n device addresses of L complex samples each, complete before the call.
        -> (list of n PCM byte arrays, olen * channels samples each, empty for a "no samples" block; WfmStatus array).
        fill: what the PCM buffers hold before the call (the part of a buffer the block did not write is returned in `self.last_raw`)."""
        insts = np.ascontiguousarray(insts, np.int32)
        n = insts.shape[0]
        if on_device:
            bp = (_vp * n)(*[int(a) if a else None for a in bb])
        elif isinstance(bb, (list, tuple)):
            bb = [None if r is None else np.ascontiguousarray(r, np.complex64).reshape(self.L) for r in bb]
            bp = (_vp * n)(*[None if r is None else r.ctypes.data for r in bb])
        else:
            bb = np.ascontiguousarray(bb, np.complex64).reshape(n, self.L)
            bp = (_vp * n)(*[bb[i].ctypes.data for i in range(n)])
        pw = np.ascontiguousarray(bb_power, np.float64).reshape(n)
        nz = np.ascontiguousarray(n0, np.float64).reshape(n)
        raw = np.full((n, self.olen * 2 * 4), fill, np.uint8)
        pp = (_vp * n)(*[raw[i].ctypes.data for i in range(n)])
        status = (WfmStatus * n)()
        self.last_raw = raw
        _check(lib().chz_wfm_execute(self._h, n, insts.ctypes.data, bp, int(bool(on_device)), pw.ctypes.data, nz.ctypes.data, pp, status))
        pcm = []
        for i in range(n):
            nb = 0 if status[i].frame else self.olen * status[i].channels * PCM_SAMPLE_BYTES[self._enc.get(int(insts[i]), PCM_F32LE)]
            pcm.append(raw[i, :nb].copy())
        return pcm, status

    def close(self):
        if self._h:
            lib().chz_wfm_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class AfskPool:
    """Pool of AFSK / AX.25 packet decoders of one geometry (packetd's decode_task(), src/packetd.c): 16-bit audio in, a status record per
    block and the frames that completed (CRC included) out.  RTP, the reference's zero-flush feeder and APRS parsing stay with the caller."""

    def __init__(self, L, M, samprate, capacity, bitrate=1200.0, mark=1200.0, space=2200.0, byte_order=AFSK_BE, device=0, frame_stride=AFSK_FRAME_MAX):
        self._h = _vp()
        _check(lib().chz_afsk_create(C.byref(self._h), L, M, float(samprate), float(bitrate), float(mark), float(space), byte_order, capacity, device))
        g = (_i * 4)()
        _check(lib().chz_afsk_geometry(self._h, C.byref(g)))
        self.geometry = dict(zip(("L", "M", "N", "samppbit"), (int(v) for v in g)))
        self.L, self.M, self.N, self.samppbit = (self.geometry[k] for k in ("L", "M", "N", "samppbit"))
        self.samprate, self.capacity, self.byte_order, self.frame_stride = float(samprate), capacity, byte_order, int(frame_stride)

    @staticmethod
    def check(L, M, samprate, bitrate=1200.0, mark=1200.0, space=2200.0, byte_order=AFSK_BE):
        """Would a pool of this geometry be created?  Raises ChzError with the reason if not; touches no device."""
        _check(lib().chz_afsk_check(L, M, float(samprate), float(bitrate), float(mark), float(space), byte_order))

    def add(self):
        return _check(lib().chz_afsk_add(self._h))

    def release(self, inst):
        _check(lib().chz_afsk_release(self._h, inst))

    def set_response(self, inst, resp):
        r = np.ascontiguousarray(resp, np.complex64).reshape(-1)
        assert r.shape[0] == self.N
        _check(lib().chz_afsk_set_response(self._h, inst, r.ctypes.data))

    def execute(self, insts, samples, on_device=False, frames_buf=None, status_buf=None):
        """samples: [n][L] 16-bit words in the pool's byte order as they lie in memory (an int16 / uint16 array or a list of n rows, of which
        one may be None: a null row, which the call refuses), or (on_device) n device addresses of L such words each, complete before the call.
        frames_buf, status_buf: the caller's own uint8 buffers [n][2 * frame_stride] and [n][sizeof(AfskStatus)] (a caller that runs every block
        keeps them; without them each call makes its own).  -> (AfskStatus array, list of n lists of frames as bytes)."""
        insts = np.ascontiguousarray(insts, np.int32)
        n = insts.shape[0]
        if on_device:
            sp = (_vp * n)(*[int(a) if a else None for a in samples])
        else:
            rows = [None if r is None else np.ascontiguousarray(r).view(np.uint16).reshape(self.L) for r in samples]
            sp = (_vp * n)(*[None if r is None else r.ctypes.data for r in rows])
        raw = np.empty((n, 2 * self.frame_stride), np.uint8) if frames_buf is None else frames_buf
        sraw = np.empty((n, C.sizeof(AfskStatus)), np.uint8) if status_buf is None else status_buf
        assert raw.dtype == np.uint8 and raw.flags.c_contiguous and raw.shape == (n, 2 * self.frame_stride)
        assert sraw.dtype == np.uint8 and sraw.flags.c_contiguous and sraw.shape == (n, C.sizeof(AfskStatus))
        fp = (_vp * n)(*[raw[i].ctypes.data for i in range(n)])
        _check(lib().chz_afsk_execute(self._h, n, insts.ctypes.data, sp, int(bool(on_device)), sraw.ctypes.data, fp, self.frame_stride))
        status = (AfskStatus * n).from_buffer(sraw)
        frames = [[raw[i, j * self.frame_stride:j * self.frame_stride + min(status[i].frame_len[j], self.frame_stride)].tobytes()
                   for j in range(status[i].nframes)] for i in range(n)]
        return status, frames

    def close(self):
        if self._h:
            lib().chz_afsk_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class CtcssPool:
    """Pool of CTCSS / PL tone decoders of one sample rate, byte order and tone table (ctcss's tone search, src/ctcss.c): 16-bit audio in
    rows of L = 0.2 s, one status record per block out -- the strongest tone above the threshold, the last tone found, its energy -- and, on
    request, the energies of all tones.  RTP and collecting packets into rows stay with the caller."""

    def __init__(self, samprate, capacity, byte_order=CTCSS_BE, tones=None, device=0):
        self._h = _vp()
        n, t = self._table(tones)
        _check(lib().chz_ctcss_create(C.byref(self._h), float(samprate), byte_order, n, t, capacity, device))
        g = (_i * 7)()
        _check(lib().chz_ctcss_geometry(self._h, C.byref(g)))
        self.geometry = dict(zip(("L", "M", "N", "olen", "P", "shift", "ntones"), (int(v) for v in g)))
        self.L, self.M, self.N, self.olen, self.P, self.shift, self.ntones = (int(v) for v in g)
        self.tones = tuple(CTCSS_TONES if tones is None else (float(f) for f in tones))
        self.samprate, self.capacity, self.byte_order = float(samprate), capacity, byte_order

    @staticmethod
    def _table(tones):
        if tones is None:
            return 0, None
        tones = [float(f) for f in tones]
        return len(tones), (_d * max(len(tones), 1))(*tones)

    @staticmethod
    def check(samprate, byte_order=CTCSS_BE, tones=None):
        """Would a pool of this geometry be created?  Raises ChzError with the reason if not; touches no device."""
        n, t = CtcssPool._table(tones)
        _check(lib().chz_ctcss_check(float(samprate), byte_order, n, t))

    def add(self):
        return _check(lib().chz_ctcss_add(self._h))

    def release(self, inst):
        _check(lib().chz_ctcss_release(self._h, inst))

    def set_response(self, inst, resp):
        r = np.ascontiguousarray(resp, np.complex64).reshape(-1)
        assert r.shape[0] == self.P
        _check(lib().chz_ctcss_set_response(self._h, inst, r.ctypes.data))

    def execute(self, insts, samples, on_device=False, status_buf=None, energies=None):
        """samples: [n][L] 16-bit words in the pool's byte order as they lie in memory (an int16 / uint16 array or a list of n rows, of which
        one may be None: a null row, which the call refuses), or (on_device) n device addresses of L such words each, complete before the call.
        status_buf: the caller's own uint8 buffer [n][sizeof(CtcssStatus)] (a caller that runs every block keeps it; without it each call makes
        its own).  energies: None, or a float64 array [n][ntones] that receives every request's energies.  -> CtcssStatus array."""
        insts = np.ascontiguousarray(insts, np.int32)
        n = insts.shape[0]
        if on_device:
            sp = (_vp * n)(*[int(a) if a else None for a in samples])
        else:
            rows = [None if r is None else np.ascontiguousarray(r).view(np.uint16).reshape(self.L) for r in samples]
            sp = (_vp * n)(*[None if r is None else r.ctypes.data for r in rows])
        sraw = np.empty((n, C.sizeof(CtcssStatus)), np.uint8) if status_buf is None else status_buf
        assert sraw.dtype == np.uint8 and sraw.flags.c_contiguous and sraw.shape == (n, C.sizeof(CtcssStatus))
        ep = None
        if energies is not None:
            assert energies.dtype == np.float64 and energies.flags.c_contiguous and energies.shape == (n, self.ntones)
            ep = (_vp * n)(*[energies[i].ctypes.data for i in range(n)])
        _check(lib().chz_ctcss_execute(self._h, n, insts.ctypes.data, sp, int(bool(on_device)), sraw.ctypes.data, ep))
        return (CtcssStatus * n).from_buffer(sraw)

    def close(self):
        if self._h:
            lib().chz_ctcss_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MpxPool:
    """Pool of FM-multiplex decoders of one block time, kind and byte order (stereod's and rdsd's decode() loops, src/stereod.c, src/rdsd.c):
    the 16-bit multiplex at 384 kHz in rows of L samples in, 4 olen bytes of big-endian 16-bit PCM (L R interleaved, or the 57 kHz
    subcarrier's re im) and a status record per block out.  RTP and collecting packets into rows stay with the caller."""

    def __init__(self, blocktime, capacity, kind=MPX_STEREO, byte_order=MPX_BE, device=0):
        self._h = _vp()
        _check(lib().chz_mpx_create(C.byref(self._h), float(blocktime), kind, byte_order, capacity, device))
        g = (_i * 7)()
        _check(lib().chz_mpx_geometry(self._h, C.byref(g)))
        self.geometry = dict(zip(("L", "M", "N", "olen", "P", "pilot_shift", "subc_shift"), (int(v) for v in g)))
        self.L, self.M, self.N, self.olen, self.P = (self.geometry[k] for k in ("L", "M", "N", "olen", "P"))
        self.blocktime, self.capacity, self.kind, self.byte_order = float(blocktime), capacity, kind, byte_order
        self.nslaves = 3 if kind == MPX_STEREO else 2
        self.last_raw = None

    @staticmethod
    def check(blocktime, kind=MPX_STEREO, byte_order=MPX_BE):
        """Would a pool of this geometry be created?  Raises ChzError with the reason if not; touches no device."""
        _check(lib().chz_mpx_check(float(blocktime), kind, byte_order))

    def add(self):
        return _check(lib().chz_mpx_add(self._h))

    def release(self, inst):
        _check(lib().chz_mpx_release(self._h, inst))

    def set_params(self, inst, params):
        _check(lib().chz_mpx_set_params(self._h, inst, C.byref(params)))

    def set_response(self, inst, slave, resp):
        r = np.ascontiguousarray(resp, np.complex64).reshape(-1)
        assert r.shape[0] == self.P
        _check(lib().chz_mpx_set_response(self._h, inst, slave, r.ctypes.data))

    def execute(self, insts, samples, audio=False, on_device=False, fill=None):
        """samples: [n][L] 16-bit words in the pool's byte order as they lie in memory (an int16 / uint16 array or a list of n rows, of which
        one may be None: a null row, which the call refuses), or (on_device) n device addresses of L such words each, complete before the call.
        audio: also return the 2 olen floats per request that the packer was fed.  fill: what the PCM (and float) buffers hold before the call;
        the PCM buffers are 16 bytes longer than a row and kept whole in `self.last_raw`, the float buffers in `self.last_raw_audio`.
        -> (list of n PCM byte arrays of 4 olen bytes, list of n float32 arrays of 2 olen or None, MpxStatus array)."""
        insts = np.ascontiguousarray(insts, np.int32)
        n = insts.shape[0]
        if on_device:
            sp = (_vp * n)(*[int(a) if a else None for a in samples])
        else:
            rows = [None if r is None else np.ascontiguousarray(r).view(np.uint16).reshape(self.L) for r in samples]
            sp = (_vp * n)(*[None if r is None else r.ctypes.data for r in rows])
        nb = 4 * self.olen
        raw = np.empty((n, nb + 16), np.uint8) if fill is None else np.full((n, nb + 16), fill, np.uint8)
        pp = (_vp * n)(*[raw[i].ctypes.data for i in range(n)])
        fraw, ap = None, None
        if audio:
            fraw = np.empty((n, 2 * self.olen + 4), np.float32)
            if fill is not None:
                fraw.view(np.uint8)[:] = fill
            ap = (_vp * n)(*[fraw[i].ctypes.data for i in range(n)])
        status = (MpxStatus * n)()
        self.last_raw, self.last_raw_audio = raw, fraw
        _check(lib().chz_mpx_execute(self._h, n, insts.ctypes.data, sp, int(bool(on_device)), pp, ap, status))
        pcm = [raw[i, :nb].copy() for i in range(n)]
        return pcm, ([fraw[i, :2 * self.olen].copy() for i in range(n)] if audio else None), status

    def close(self):
        if self._h:
            lib().chz_mpx_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
