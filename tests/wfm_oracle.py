"""demod_wfm() (src/wfm.c:134-281) restated in float64 numpy: the checker of chz_wfm_* (tests/test_gpu_wfm.py), itself pinned to the
reference's wfm.c by tests/test_wfm_reference.py.

One Decoder is one channel: float32 baseband, bb_power, n0, the three float32 responses and the parameters in; per block the status
members, the float PCM the reference would hand to send_output() and the margins of the block's decisions out.  The composite
filter is rebuilt from ol.Stream, ol.channel and real_channel_f64 (tests/test_gpu_rmini.py).  The composite block is rounded to
float32 as the reference stores it; everything behind the filter is double in the reference and float64 here.

f32=True runs the same statements with a float32 arctan2 and float32 transforms: the "f32 twin", which stands for how far the
reference moves when its own arithmetic rounds differently."""
import numpy as np

import oracle_lib as ol

COMPOSITE_RATE, AUDIO_RATE = 384000.0, 48000.0          # src/wfm.c:22-23
PILOT_THRESHOLD = 1e-6                                  # :208
CONTINUOUS = ("snr", "foffset", "pdeviation", "subc_amp", "output_power")
DISCRETE = ("frame", "mute", "squelch_state", "channels", "pilot_present")


def geometry(blocktime):
    """L, N, olen, P, pilot_shift, subc_shift (src/wfm.c:51-56,93-101; compute_tuning, src/radio.c:1175-1199)"""
    L = int(np.rint(COMPOSITE_RATE * blocktime)); M = L + 1; N = L + M - 1
    olen = int(np.rint(AUDIO_RATE * blocktime))
    hzperbin = COMPOSITE_RATE / N
    return L, N, olen, N * olen // L, int(np.rint(19000.0 / hzperbin)), int(np.rint(38000.0 / hzperbin))


def responses(blocktime, beta=11.0):
    """the three filters of src/wfm.c:75-89 as set_filter() leaves them: mono 50 Hz - 15 kHz (REAL), pilot +-100 Hz, L-R +-15 kHz"""
    L, N, olen, P, _, _ = geometry(blocktime)
    return [ol.set_filter(P, olen, N, True, 50.0 / AUDIO_RATE, 15000.0 / AUDIO_RATE, beta, ol.REAL),
            ol.set_filter(P, olen, N, True, -100.0 / AUDIO_RATE, 100.0 / AUDIO_RATE, beta, ol.COMPLEX),
            ol.set_filter(P, olen, N, True, -15000.0 / AUDIO_RATE, 15000.0 / AUDIO_RATE, beta, ol.COMPLEX)]


def real_channel_f64(spec, P, olen, shift, resp):
    """a REAL slave of a REAL master on the float64 spectrum (src/filter.c:803-809,911), as tests/test_gpu_rmini.py states it"""
    sb = P // 2 + 1
    mi = np.arange(sb) + shift
    ok = (mi >= 0) & (mi < spec.shape[0])
    fd = np.zeros(sb, np.complex128)
    fd[ok] = spec[mi[ok]] * resp[:sb][ok].astype(np.complex128)
    fd[(sb + 1) // 2] = 0
    return (np.fft.irfft(fd, P) * P)[P - olen:]


class Decoder:
    def __init__(self, blocktime, resp, stereo_enable=True, squelch_open=10.0, squelch_close=6.3, squelch_tail=2, bandwidth=220000.0,
                 headroom=10 ** (-15 / 20), deemph_rate=0.0, deemph_gain=1.0, f32=False):
        self.blocktime, self.f32 = blocktime, f32
        self.L, self.N, self.olen, self.P, self.pilot_shift, self.subc_shift = geometry(blocktime)
        self.resp = [np.ascontiguousarray(r, np.complex64) for r in resp]
        self.stereo_enable, self.open, self.close, self.tail = bool(stereo_enable), squelch_open, squelch_close, squelch_tail
        self.bandwidth, self.headroom, self.rate, self.dgain = bandwidth, headroom, deemph_rate, deemph_gain
        self.stream = ol.Stream(self.L, self.L + 1, ol.REAL)
        self.alpha = -np.expm1(-blocktime * 1.0)                  # :103
        self.phase_memory = 0.0
        self.squelch_state = 0
        self.foffset = self.pdeviation = 0.0
        self.stereo_deemph = 0j
        self.mono_deemph = 0.0
        self.channels = 2 if stereo_enable else 1               # :43-45

    def _slaves(self, composite, want_pilot):
        """mono, pilot (or None), and a function that runs the L-R slave"""
        P, olen = self.P, self.olen
        if self.f32:
            spec = self.stream.push(composite)
            mono = ol.channel(spec, ol.REAL, P, olen, 0, self.resp[0], out_type=ol.REAL).astype(np.float64)
        else:
            spec = self.stream.push(composite, f64=True)
            mono = real_channel_f64(spec, P, olen, 0, self.resp[0])
        cplx = lambda shift, r: ol.channel(spec, ol.REAL, P, olen, shift, r).astype(np.complex128)
        pilot = cplx(self.pilot_shift, self.resp[1]) if want_pilot else None
        return mono, pilot, lambda: cplx(self.subc_shift, self.resp[2])

    def block(self, bb, bb_power, n0):
        bb = np.ascontiguousarray(bb, np.complex64)
        L, olen = self.L, self.olen
        bw = abs(self.bandwidth)
        snr = bb_power / (n0 * bw) - 1                                               # :134
        fm_snr = max(0.0, snr)
        gain = (2 * self.headroom * COMPOSITE_RATE) / bw                             # :193 (a function of the parameters alone: reported on every block)
        out = {"snr": fm_snr, "gain": gain, "pilot_present": 0, "subc_amp": 0.0, "pcm": None, "wrap_margin": np.inf,
               "snr_margin": min(abs(fm_snr / self.open - 1), abs(snr / self.close - 1))}
        smax = self.tail + 1
        if fm_snr >= self.open or (self.squelch_state > 0 and snr >= self.close):    # :139-151
            self.squelch_state = smax
        else:
            self.squelch_state -= 1
            if self.squelch_state <= 0:
                self.squelch_state = 0
                self.phase_memory = 0.0
                out.update(frame=1, mute=1, squelch_state=0, channels=self.channels, output_power=0.0, foffset=self.foffset, pdeviation=self.pdeviation)
                return out
        # :153-161
        if self.f32:
            arg = np.arctan2(bb.imag.astype(np.float32), bb.real.astype(np.float32)).astype(np.float32)
        else:
            arg = np.arctan2(bb.imag.astype(np.float64), bb.real.astype(np.float64)).astype(np.float32)      # cargf(), correctly rounded
        ph = (1.0 / np.pi) * arg.astype(np.float64)
        x = ph - np.concatenate([[self.phase_memory], ph[:-1]])
        self.phase_memory = float(ph[-1])
        out["wrap_margin"] = float(np.min(np.abs(np.abs(x) - 1)))
        x = np.where(x > 1, x - 2, np.where(x < -1, x + 2, x))
        composite = x.astype(np.float32)
        if self.squelch_state == smax:                                               # :162-185
            c = composite.astype(np.float64)
            fo = c.sum() * (COMPOSITE_RATE * 0.5 / L)
            self.foffset += self.alpha * (fo - self.foffset)
            pp = max(0.0, c.max()) * (COMPOSITE_RATE * 0.5) - self.foffset
            pn = min(0.0, c.min()) * (COMPOSITE_RATE * 0.5) - self.foffset
            self.pdeviation = max(pp, -pn)
        mono, pilot, lmr_fn = self._slaves(composite, self.stereo_enable)            # :187-199
        present = False
        if self.stereo_enable:                                                       # :196-210
            p32 = pilot.astype(np.complex64)
            out["subc_amp"] = float((p32.real * p32.real + p32.imag * p32.imag).astype(np.float64).sum() / olen)
            present = out["subc_amp"] > PILOT_THRESHOLD
        if present:                                                                  # :211-249
            self.channels = 2
            lmr = lmr_fn()
            subc = pilot * pilot / (pilot.real ** 2 + pilot.imag ** 2)
            info = 2.0 * (np.conj(subc) * lmr).imag
            s = (mono + info) + 1j * (mono - info)
            if self.rate != 0:
                y = self.stereo_deemph
                for n in range(olen):
                    y += self.rate * (self.dgain * s[n] - y)
                    s[n] = y
                self.stereo_deemph = y
            buf = (s * gain).astype(np.complex64)
            power = float((buf.real * buf.real + buf.imag * buf.imag).astype(np.float64).sum() / (2 * olen))
            pcm = np.ascontiguousarray(buf).view(np.float32).copy()
        else:                                                                        # :250-284
            self.channels = 1
            s = mono.copy()
            if self.rate != 0:
                y = self.mono_deemph
                for n in range(olen):
                    y += self.rate * (self.dgain * s[n] - y)
                    s[n] = y
                self.mono_deemph = y
            s = s * gain
            power = float((s * s).sum() / olen)
            pcm = s.astype(np.float32)
        out.update(frame=0, mute=0, squelch_state=self.squelch_state, channels=self.channels, pilot_present=int(present), output_power=power,
                   foffset=self.foffset, pdeviation=self.pdeviation, pcm=pcm)
        return out


def synthesise(nblocks, blocktime, seed, stereo=None, carrier=0.05, noise=1e-4):
    """complex64 [nblocks][L] at 384 kHz as mini_radiod_lib.synthesise() makes a broadcast signal: L + R, a 19 kHz pilot at 9 %, L - R on the
    suppressed 38 kHz subcarrier, 75 kHz deviation, in complex noise of `noise` a component.  stereo: per block the strength of pilot
    and L - R (None: 1 throughout); carrier 0 leaves the noise alone."""
    L = geometry(blocktime)[0]
    n = nblocks * L
    t = np.arange(n) / COMPOSITE_RATE
    rng = np.random.default_rng(seed)
    st = np.ones(n) if stereo is None else np.repeat(np.asarray(stereo, np.float64), L)
    left, right = np.sin(2 * np.pi * 1000.0 * t), 0.6 * np.sin(2 * np.pi * 2600.0 * t + 0.5)
    mpx = 0.45 * (left + right) + 0.45 * (left - right) * np.sin(2 * np.pi * 38000.0 * t) * st + 0.09 * np.sin(2 * np.pi * 19000.0 * t) * st
    x = carrier * np.exp(1j * (2 * np.pi * 75000.0 * np.cumsum(mpx) / COMPOSITE_RATE + 0.3 * seed))
    x = x + noise * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return x.astype(np.complex64).reshape(nblocks, L)
