"""stereod's and rdsd's decode() loops (src/stereod.c:373-408 and :460-513, src/rdsd.c:385-413 and :465-500) restated in float64 Python /
numpy: the checker of chz_mpx_* (tests/test_gpu_mpx.py), itself pinned to the reference's stereod.c and rdsd.c by
tests/test_mpx_reference.py.

One Decoder is one session: blocks of L = lrint(384000 blocktime) 16-bit samples in, per block the values the packer is fed (float64:
left, right interleaved, or the 57 kHz slave's re, im), the record that chz_mpx_status carries and the packed PCM out.  The filter is
the oracle's (ol.Stream, ol.channel, wfm_oracle.real_channel_f64: a REAL master of L, M = L + 1 with slaves of olen = L / 8, P = 2 olen),
its outputs rounded to float32 as the reference stores them; everything behind it is double in the reference and float64 here, in the
reference's order: the pilot squared with every product rounded, cabs() as hypot, the a > 0 test, 2 Im(conj(subc) stereo), the two
de-emphasis recurrences state = state * rate + (gain * (1 - rate)) * x sample by sample.

f32=True runs the same statements on the oracle's float32 transforms: the "f32 twin", which stands for how far the reference moves when
its own arithmetic rounds differently.

Also here: geometry(), the responses both programs set (Kaiser beta 3.5 pi), scaleclip() (src/misc.h:252-254: the float product 32767 x,
truncated toward zero) and the signal generator of tests/test_gpu_mpx.py."""
import numpy as np

import oracle_lib as ol
from wfm_oracle import real_channel_f64

STEREO, RDS = 0, 1
COMPOSITE_RATE, AUDIO_RATE = 384000, 48000                # Composite_samprate / In_samprate, Audio_samprate / Out_samprate
BETA = 3.5 * np.pi                                        # Kaiser_beta
GAIN = 4.0                                                # Deemph_gain (src/stereod.c:213)


def rate_of(tc):
    """Deemph_rate = exp(-1.0 / (Deemph_tc * Audio_samprate)) (src/stereod.c:214); tc 0: no memory"""
    return float(np.exp(-1.0 / (tc * AUDIO_RATE))) if tc else 0.0


RATE75 = rate_of(75e-6)


def geometry(blocktime, kind=STEREO):
    """src/stereod.c:373-379,405-408 / src/rdsd.c:385-391,410-413: hzperbin in integer division, as the reference writes it"""
    L = int(np.rint(COMPOSITE_RATE * blocktime)); M = L + 1; N = L + M - 1
    olen = (L * AUDIO_RATE) // COMPOSITE_RATE
    hzperbin = COMPOSITE_RATE // N
    quantum = N // (M - 1)
    rot = lambda f: quantum * int(np.rint(f / (hzperbin * quantum)))
    return {"L": L, "M": M, "N": N, "olen": olen, "P": N * olen // L, "pilot_shift": rot(19000.0), "subc_shift": rot(38000.0 if kind == STEREO else 57000.0)}


def responses(blocktime, kind=STEREO):
    """STEREO: mono 50 Hz - 15 kHz (REAL), pilot +-100 Hz, L-R +-15 kHz (src/stereod.c:389,395,401); RDS: pilot +-100 Hz, rds +-2 kHz (src/rdsd.c:401,406)"""
    g = geometry(blocktime, kind)
    P, olen, N = g["P"], g["olen"], g["N"]
    f = lambda lo, hi, t: ol.set_filter(P, olen, N, True, lo / AUDIO_RATE, hi / AUDIO_RATE, BETA, t)
    if kind == STEREO:
        return [f(50.0, 15000.0, ol.REAL), f(-100.0, 100.0, ol.COMPLEX), f(-15000.0, 15000.0, ol.COMPLEX)]
    return [f(-100.0, 100.0, ol.COMPLEX), f(-2000.0, 2000.0, ol.COMPLEX)]


def scaleclip(x):
    """scaleclip() on float32 values -> int16: x >= 1 -> 32767, x <= -1 -> -32767, else (int16_t)(INT16_MAX * x) with the product in float"""
    x = np.asarray(x, np.float32)
    prod = np.float32(32767.0) * x
    assert prod.dtype == np.float32
    v = np.trunc(np.where(np.abs(x) < 1, prod, np.float32(0)))
    return np.where(x >= 1, 32767, np.where(x <= -1, -32767, v)).astype(np.int16)


def pack(x):
    """the bytes both programs send: htons(scaleclip(x)) of every value"""
    return scaleclip(x).astype(">i2").tobytes()


def to_float(s16, kind):
    """src/stereod.c:461-462: (float)(SCALE * s) with SCALE = 1. / INT16_MAX a double; src/rdsd.c:466: ldexp(s, -15), handed to put_rfilter's float"""
    s = np.asarray(s16, np.int16).astype(np.float64)
    return ((1.0 / 32767) * s).astype(np.float32) if kind == STEREO else np.ldexp(s, -15).astype(np.float32)


class Decoder:
    def __init__(self, blocktime, kind=STEREO, resp=None, rate=RATE75, gain=GAIN, f32=False):
        g = geometry(blocktime, kind)
        self.g, self.kind, self.f32 = g, kind, f32
        self.resp = [np.ascontiguousarray(r, np.complex64) for r in (responses(blocktime, kind) if resp is None else resp)]
        self.stream = ol.Stream(g["L"], g["M"], ol.REAL)
        self.rate, self.gain = float(rate), float(gain)
        self.left = self.right = 0.0

    def block(self, s16):
        g = self.g
        P, olen = g["P"], g["olen"]
        x = to_float(s16, self.kind)
        spec = self.stream.push(x, f64=not self.f32)
        cplx = lambda shift, r: ol.channel(spec, ol.REAL, P, olen, shift, r).astype(np.complex64).astype(np.complex128)
        if self.kind == RDS:
            y = cplx(g["subc_shift"], self.resp[1])
            audio = np.ascontiguousarray(y).view(np.float64).copy()
            return {"audio": audio, "zero_pilot": 0, "deemph_left": 0.0, "deemph_right": 0.0, "pcm": pack(audio.astype(np.float32))}
        if self.f32:
            mono = ol.channel(spec, ol.REAL, P, olen, 0, self.resp[0], out_type=ol.REAL).astype(np.float64)
        else:
            mono = real_channel_f64(spec, P, olen, 0, self.resp[0]).astype(np.float32).astype(np.float64)
        pilot, stereo = cplx(g["pilot_shift"], self.resp[1]), cplx(g["subc_shift"], self.resp[2])
        pr, pi = pilot.real, pilot.imag
        sr, si = pr * pr - pi * pi, pr * pi + pi * pr                      # subc_phasor *= subc_phasor
        a = np.hypot(sr, si)                                               # cabs()
        ok = a > 0
        safe = np.where(ok, a, 1.0)
        cr, ci = sr / safe, si / safe
        lmr = np.where(ok, 2.0 * (cr * stereo.imag - ci * stereo.real), 0.0)
        left, right = mono + lmr, mono - lmr
        rate, g1 = self.rate, self.gain * (1 - self.rate)
        out = np.empty(2 * olen)
        yl, yr = self.left, self.right
        for n, (l, r) in enumerate(zip(left.tolist(), right.tolist())):
            yl = yl * rate + g1 * l
            yr = yr * rate + g1 * r
            out[2 * n] = yl; out[2 * n + 1] = yr
        self.left, self.right = yl, yr
        return {"audio": out, "zero_pilot": int(olen - ok.sum()), "deemph_left": yl, "deemph_right": yr, "pcm": pack(out.astype(np.float32))}


def run(blocks, blocktime, kind=STEREO, rate=RATE75, gain=GAIN, f32=False, resp=None):
    """a fresh Decoder over int16 blocks -> the list of block records"""
    d = Decoder(blocktime, kind, resp=resp, rate=rate, gain=gain, f32=f32)
    return [d.block(b) for b in blocks]


# ---- the signal ---------------------------------------------------------------------------------------------------------------------
def signal(nblocks, blocktime, seed, amplitude, script=None, rds=False):
    """int16 [nblocks][L] at 384 kHz: A (0.45 (l + r) + 0.45 (l - r) sin(2 pi 38000 t) + 0.09 sin(2 pi 19000 t) + 1e-3 gaussian), l = sin(2 pi
    1000 t + seed), r = 0.6 sin(2 pi 2600 t + 0.5); rds adds 0.05 b(t) cos(2 pi 57000 t) inside the bracket, b a +-1 sequence at 1187.5 baud.
    script: per block a factor on the whole signal.  Rounded to the nearest 16-bit value."""
    L = geometry(blocktime)["L"]
    n = nblocks * L
    t = np.arange(n) / COMPOSITE_RATE
    rng = np.random.default_rng(seed)
    l, r = np.sin(2 * np.pi * 1000.0 * t + seed), 0.6 * np.sin(2 * np.pi * 2600.0 * t + 0.5)
    x = 0.45 * (l + r) + 0.45 * (l - r) * np.sin(2 * np.pi * 38000.0 * t) + 0.09 * np.sin(2 * np.pi * 19000.0 * t) + 1e-3 * rng.standard_normal(n)
    if rds:
        bits = 2.0 * rng.integers(0, 2, int(n * 1187.5 / COMPOSITE_RATE) + 2) - 1.0
        x = x + 0.05 * bits[np.floor(t * 1187.5).astype(np.int64)] * np.cos(2 * np.pi * 57000.0 * t)
    x = amplitude * x
    if script is not None:
        x = x * np.repeat(np.asarray(script, np.float64), L)
    return np.clip(np.rint(32767.0 * x), -32768, 32767).astype(np.int16).reshape(nblocks, L)
