"""numpy restatement of the reference's raw A/D conversion loops -- the checker of chz_input_write_raw (tests/test_gpu_raw_input.py),
pinned to the reference's own code by tests/test_raw_input_reference.py.

  PACKED12   airspy_unpack(), src/airspy-unpack.c: 8 samples in 3 little-endian 32-bit words, offset 2048; float product with (float)scale
  U16 .. S8_IQ   the switch of rx_callback(), src/hydrasdr.c:660-833 (U8_IQ is src/rtlsdr.c:323-339 too): (float)(scale * x), product in double

convert(fmt, raw_bytes, n, scale, bits) -> (float32 array [n] or [2n] I,Q interleaved, energy, clipped_samples, clipped_components)
energy is the exact integer sum of x^2 (x^2 + y^2); clipped_samples what the reference adds to frontend->overranges (an I/Q sample once if
either component clips); clipped_components every clipped component (rtlsdr.c:324-334)."""
import numpy as np

PACKED12, U16, S16, U8, S8, S16_IQ, U8_IQ, S8_IQ = range(8)
NAMES = {PACKED12: "packed12", U16: "u16", S16: "s16", U8: "u8", S8: "s8", S16_IQ: "s16_iq", U8_IQ: "u8_iq", S8_IQ: "s8_iq"}
REAL_FORMATS = (PACKED12, U16, S16, U8, S8)
IQ_FORMATS = (S16_IQ, U8_IQ, S8_IQ)
# (bytes, samples) a sample takes
BYTES = {PACKED12: (12, 8), U16: (2, 1), S16: (2, 1), U8: (1, 1), S8: (1, 1), S16_IQ: (4, 1), U8_IQ: (2, 1), S8_IQ: (2, 1)}
_DTYPE = {U16: "<u2", S16: "<i2", U8: "u1", S8: "i1", S16_IQ: "<i2", U8_IQ: "u1", S8_IQ: "i1"}


def is_iq(fmt):
    return fmt in IQ_FORMATS


def nbytes(fmt, n):
    num, den = BYTES[fmt]
    return n * num // den


def unpack12(words):
    """[3g] uint32 -> [8g] codes 0..4095"""
    w = np.asarray(words, np.uint32).reshape(-1, 3)
    w0, w1, w2 = w[:, 0], w[:, 1], w[:, 2]
    s = np.stack([w0 >> 20, w0 >> 8, (w0 << 4) | (w1 >> 28), w1 >> 16, w1 >> 4, (w1 << 8) | (w2 >> 24), w2 >> 12, w2], axis=1)
    return (s & np.uint32(0xfff)).astype(np.int64).reshape(-1)


def pack12(codes):
    """[8g] codes 0..4095 -> [3g] uint32: the inverse of unpack12"""
    s = np.asarray(codes, np.uint32).reshape(-1, 8)
    w0 = (s[:, 0] << 20) | (s[:, 1] << 8) | (s[:, 2] >> 4)
    w1 = ((s[:, 2] & 0xf) << 28) | (s[:, 3] << 16) | (s[:, 4] << 4) | (s[:, 5] >> 8)
    w2 = ((s[:, 5] & 0xff) << 24) | (s[:, 6] << 12) | s[:, 7]
    return np.stack([w0, w1, w2], axis=1).astype("<u4").reshape(-1)


def integers(fmt, raw_bytes, n, bits=12):
    """the samples' integer values with the format's offset removed: [n], or [2n] I,Q interleaved"""
    raw = np.frombuffer(np.ascontiguousarray(raw_bytes).reshape(-1).view(np.uint8)[:nbytes(fmt, n)].tobytes(), np.uint8)
    if fmt == PACKED12:
        assert n % 8 == 0
        return unpack12(raw.view("<u4")) - 2048
    x = raw.view(_DTYPE[fmt]).astype(np.int64)
    if fmt == U16:
        x = x - (1 << (bits - 1))
    elif fmt in (U8, U8_IQ):
        x = x - 128
    return x


def clipped(fmt, x, bits=12):
    if fmt == PACKED12:
        return (x == 2047) | (x <= -2047)
    if fmt == U16:
        offset = 1 << (bits - 1)
        return (x >= offset - 1) | (x <= -offset)
    if fmt in (S16, S16_IQ):
        return (x >= 32767) | (x <= -32768)
    return (x >= 127) | (x <= -128)


def scale_double(x, scale):
    """(float)(scale * x), the product in double"""
    return (np.float64(scale) * x.astype(np.float64)).astype(np.float32)


def scale_float(x, scale):
    """(float)scale * (float)x, the product in float"""
    return np.float32(scale) * x.astype(np.float32)


def convert(fmt, raw_bytes, n, scale, bits=12):
    x = integers(fmt, raw_bytes, n, bits)
    out = scale_float(x, scale) if fmt == PACKED12 else scale_double(x, scale)
    assert out.dtype == np.float32
    energy = int((x * x).sum(dtype=np.int64))          # |x| < 2^16: exact for any write a ring holds
    c = clipped(fmt, x, bits)
    comps = int(c.sum())
    samples = int((c[0::2] | c[1::2]).sum()) if is_iq(fmt) else comps
    return out, energy, samples, comps
