"""What the PCM packer tests share (tests/test_oracle_vs_reference.py pins the restated packers to the reference's rtp.c / import.h at
these values; tests/test_gpu_pcm_edges.py hands the same values to the device's packers, and tests/test_engine_emulated.py to the
emulator's): the floats at which a float -> S16 / G.711 / binary16 conversion can go wrong, how they are laid out as blocks of
baseband, and the input that drives the FM demodulator into the clip.

A linear channel with agc=False, gain_db=0, no envelope, no shift and the squelch off hands every sample to the packer bit for bit
(s = 1.0 * (double)x; out = (float)s), .x for mono and .x / .y for stereo: a row of rows() is one channel's block."""
import numpy as np


def _both_sides(x):
    x = x.astype(np.float32)
    return np.concatenate([x, np.nextafter(x, np.float32(-np.inf)), np.nextafter(x, np.float32(np.inf))])


def f16_values():
    """Every finite non-negative binary16 value, the exact midpoint of every neighbouring pair with the float32
    just below and just above it, the overflow threshold (65520 rounds to infinity, 65519.99 does not), the subnormal threshold (2^-25
    is the tie between 0 and the smallest subnormal 2^-24), an f32 subnormal -- and all of them negated, so that -0.0 is in."""
    halfs = np.arange(0x7c00, dtype=np.uint16).view(np.float16).astype(np.float32)
    mids = ((halfs[:-1].astype(np.float64) + halfs[1:].astype(np.float64)) / 2).astype(np.float32)     # 12 significant bits: exact
    assert np.array_equal(mids.astype(np.float64) * 2, halfs[:-1].astype(np.float64) + halfs[1:].astype(np.float64))
    special = np.array([65519.99, 65520.0, 70000.0, 3.4e38, np.inf, 2.0 ** -24, 2.0 ** -25, np.nextafter(np.float32(2.0 ** -25), np.float32(1)),
                        2.0 ** -26, 1e-8, 1e-40], np.float32)
    pos = np.concatenate([halfs, _both_sides(mids), special])
    return np.concatenate([pos, -pos])


def i16_values():
    """k / 32768 for k = -32769 .. 32769 (every 16-bit level, both clip points and one beyond), the ties
    (k + 0.5) / 32768 with the float32 on either side, and values far beyond the clip.  G.711's segment edges and its clip at 32635 are
    levels of this set; -0.0 is in."""
    k = np.arange(-32769, 32770, dtype=np.float64)
    levels = (k / 32768).astype(np.float32)
    ties = ((k + 0.5) / 32768).astype(np.float32)                     # 17 significant bits: exact
    assert np.array_equal(ties.astype(np.float64) * 32768, k + 0.5)
    special = np.array([1.5, -1.5, np.inf, -np.inf, 1e-40, -1e-40, 3e38, -3e38, -0.0], np.float32)
    return np.concatenate([levels, _both_sides(ties), special])


F16_VALUES = f16_values()
I16_VALUES = i16_values()
# quiet NaNs of both signs, for the F16 and F32 encodings only (lrintf(NaN) of the S16 and G.711 packers is undefined C): the output
# must be a NaN of the same sign, the payload is not compared
QUIET_NANS = np.array([0x7fc00000, 0xffc00000, 0x7fc00001, 0xffe12345, 0x7fffffff], np.uint32).view(np.float32)


def rows(values, channels, N):
    """complex64[nrows][N] holding `values` in order as the packer of a `channels`-channel linear demodulator meets them (mono: the real
    parts, the imaginary parts are +0; stereo: real, imaginary, real, ...); the last row is padded with +0.  Signs and bit patterns
    are kept (no arithmetic touches the values)."""
    values = np.ascontiguousarray(values, np.float32)
    per_row = N * channels
    nrows = -(-values.size // per_row)
    flat = np.zeros(nrows * N * 2, np.float32)
    if channels == 1:
        flat[0:2 * values.size:2] = values
    else:
        flat[:values.size] = values
    return flat.view(np.complex64).reshape(nrows, N)


def packer_input(row, channels):
    """float32[N * channels]: what the packer sees of one row of rows()."""
    f = np.ascontiguousarray(row, np.complex64).view(np.float32)
    return f[0::2].copy() if channels == 1 else f.copy()


def unit_gain_params(ol, channels, encoding, samprate=12000.0):
    """The linear channel that passes its input to the packer unchanged."""
    return ol.lin_params(channels=channels, agc=False, gain_db=0.0, encoding=encoding, samprate=samprate)


def pack(ol, encoding, floats):
    """chzo_pcm_pack (oracle/chz_oracle.c) of float32[n]: uint8 bytes."""
    import ctypes as C
    lib = ol.oracle()
    lib.chzo_pcm_pack.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p]; lib.chzo_pcm_pack.restype = None
    x = np.ascontiguousarray(floats, np.float32)
    out = np.zeros(ol.pcm_bytes(encoding, x.size), np.uint8)
    lib.chzo_pcm_pack(encoding, x.ctypes.data, x.size, out.ctypes.data)
    return out


# ---- FM at the clip ---------------------------------------------------------------------------------------------------
FM_CLIP_N, FM_CLIP_FS, FM_CLIP_BT, FM_CLIP_BLOCKS = 240, 24000.0, 0.01, 10
# (fm_params keywords): +6 dB of headroom with the default de-emphasis, 0 dB without one: about half of the samples clip in both
FM_CLIP_KW = [dict(headroom_db=6.0), dict(deemph_tc=0, headroom_db=0.0)]


def fm_clip_case(seed):
    """(baseband complex64[10][240], bb_power[10], noise estimates[10]): a 3 kHz tone at 7 kHz of deviation, amplitude 0.1, in noise of
    sigma 0.003 a component, 24 kHz."""
    r = np.random.default_rng(seed)
    n = FM_CLIP_N * FM_CLIP_BLOCKS
    t = np.arange(n)
    phase = -(7000.0 / 3000.0) * np.cos(2 * np.pi * 3000.0 * t / FM_CLIP_FS)
    x = 0.1 * np.exp(1j * phase) + 0.003 * (r.standard_normal(n) + 1j * r.standard_normal(n))
    bb = x.astype(np.complex64).reshape(FM_CLIP_BLOCKS, FM_CLIP_N)
    power = np.array([np.mean(np.abs(b.astype(np.complex128)) ** 2) for b in bb])
    n0 = np.full(FM_CLIP_BLOCKS, 2 * 0.003 ** 2 / FM_CLIP_FS)
    return bb, power, n0


def clipped_fraction(ol, encoding, pcm):
    """The share of a frame's samples that sit at the packer's clip: +-32767 for S16, the end codes of G.711 (magnitude 32635 and
    beyond); None for the float encodings, which do not clip."""
    pcm = np.ascontiguousarray(pcm, np.uint8)
    if encoding in (ol.PCM_S16BE, ol.PCM_S16LE):
        v = pcm.view(">i2" if encoding == ol.PCM_S16BE else "<i2").astype(np.int32)
        return float(np.mean(np.abs(v) == 32767))
    if encoding in (ol.PCM_MULAW, ol.PCM_ALAW):
        ends = pack(ol, encoding, np.array([1.0, -1.0], np.float32))
        return float(np.mean((pcm == ends[0]) | (pcm == ends[1])))
    return None
