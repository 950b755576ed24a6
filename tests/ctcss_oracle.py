"""ctcss's PL tone search (src/ctcss.c:268-309, process_pl() :392-419, the oscillators of src/osc.c:28-70) restated in float64 Python /
numpy: the checker of chz_ctcss_* (tests/test_gpu_ctcss.py), itself pinned to the reference's ctcss.c by tests/test_ctcss_reference.py.

One Decoder is one session: blocks of L = lrint(0.2 samprate) float samples in (16-bit values scaled by 2^-15, :294), per block the
record that chz_ctcss_status carries and the energies of all tones out.  The filter is the oracle's (ol.Stream, ol.channel: a REAL master
of L, M = L + 1 with one COMPLEX slave of olen 100, P = 200, shift 60), its output rounded to float32 as the reference stores it;
everything behind it is double in the reference and float64 here, in the reference's order: every tone's oscillator (afsk_oracle.Osc,
stepped as a Bank) steps sample by sample and is renormalised every 16384 steps, the integrators add conj(samp) * phasor sample by sample from the left
(np.cumsum is a sequential sum), the decision compares the energies in ascending tone order with a strict >.

f32=True runs the same statements on the oracle's float32 transform: the "f32 twin", which stands for how far the reference moves when
its own arithmetic rounds differently.

Also here: the tone generator (segments of simultaneous tones, phase continuous from segment to segment, seeded white noise)."""
import numpy as np

import afsk_oracle as ao
import oracle_lib as ol

TONES = (67.0, 69.3, 71.9, 74.4, 77.0, 79.7, 82.5, 85.4, 88.5, 91.5, 94.8, 97.4, 100.0, 103.5, 107.2, 110.9, 114.8, 118.8, 123.0, 127.3,
         131.8, 136.5, 141.3, 146.2, 150.0, 151.4, 156.7, 159.8, 162.2, 165.5, 167.9, 171.3, 173.8, 177.3, 179.9, 183.5, 186.2, 189.9, 192.8,
         196.6, 199.5, 203.5, 206.5, 210.7, 213.8, 218.1, 221.3, 225.7, 229.1, 233.6, 237.1, 241.8, 245.5, 250.3, 254.1)      # PL_tones[], :62-69
PL_SAMPRATE, PL_SHIFT, FILTER_TIME = 500.0, 150.0, 0.2
OLEN = int(round(PL_SAMPRATE * FILTER_TIME))            # 100: the slave's block and pl_blocksize (:272,280)
P = 2 * OLEN
SHIFT = int(round(2 * (PL_SHIFT * FILTER_TIME)))        # 60 (:298)
THRESHOLD = 0.005 * OLEN                                # :404


def geometry(samprate, ntones=len(TONES)):
    L = int(round(FILTER_TIME * samprate))              # lrint(): ties to even, as round()
    return {"L": L, "M": L + 1, "N": 2 * L, "olen": OLEN, "P": P, "shift": SHIFT, "ntones": ntones}


def response(samprate):
    """set_filter(&pl_filter_out, (50 - 150) / 500, (300 - 150) / 500, 11) (:284)"""
    N = 2 * int(round(FILTER_TIME * samprate))
    return ol.set_filter(P, OLEN, N, True, (50.0 - PL_SHIFT) / PL_SAMPRATE, (300.0 - PL_SHIFT) / PL_SAMPRATE, 11.0, ol.COMPLEX)


class Bank:
    """One afsk_oracle.Osc per tone, stepped together: the same statements as Osc.run() on arrays over the tones (all of a session's
    oscillators count their steps alike, so they renormalise at the same sample).  Real and imaginary parts are kept apart so that every
    product and sum is rounded by itself, as Python's complex arithmetic rounds them in Osc.run(); tests/test_ctcss_reference.py holds the
    two to equal bits across the first renormalisation."""

    def __init__(self, tones):
        osc = [ao.Osc((f - PL_SHIFT) / PL_SAMPRATE) for f in tones]
        for f, o in zip(tones, osc):
            if f == PL_SHIFT:
                assert o.step == 1 + 0j                # the frequency equals the zeroed freq: phasor_step stays 1 (src/osc.c:34,37)
        self.re, self.im = np.array([o.phasor.real for o in osc]), np.array([o.phasor.imag for o in osc])
        self.sr, self.si = np.array([o.step.real for o in osc]), np.array([o.step.imag for o in osc])
        self.steps = osc[0].steps

    def run(self, n):
        out = np.empty((self.re.shape[0], n), np.complex128)
        re, im, sr, si = self.re, self.im, self.sr, self.si
        for i in range(n):
            self.steps -= 1
            if self.steps <= 0:
                self.steps = ao.RENORM
                a = np.hypot(re, im)
                re, im = re / a, im / a
            out[:, i] = re + 1j * im
            re, im = re * sr - im * si, re * si + im * sr
        self.re, self.im = re, im
        return out


# A session's oscillators start from set_osc() on zeroed memory and nothing ever steers them: block b holds the same phasors in every
# session of one tone table.  They are stepped once and shared.
_banks = {}


def phasors(tones, block):
    """[ntones][OLEN]: the phasors step_osc() returns during block `block` of a session"""
    bank, got = _banks.setdefault(tones, (Bank(tones), []))
    while len(got) <= block:
        got.append(bank.run(OLEN))
    return got[block]


class Decoder:
    def __init__(self, samprate, resp=None, tones=TONES, f32=False):
        g = geometry(samprate, len(tones))
        self.L, self.N, self.f32, self.tones = g["L"], g["N"], f32, tuple(float(f) for f in tones)
        self.resp = np.ascontiguousarray(response(samprate) if resp is None else resp, np.complex64)
        self.stream = ol.Stream(self.L, self.L + 1, ol.REAL)
        self.nblock, self.current = 0, -1

    def block(self, samples):
        x = np.ascontiguousarray(samples, np.float32)
        spec = self.stream.push(x, f64=not self.f32)
        y = ol.channel(spec, ol.REAL, P, OLEN, SHIFT, self.resp).astype(np.complex64).astype(np.complex128)
        ph = phasors(self.tones, self.nblock)
        acc = np.cumsum(np.conj(y)[None, :] * ph, axis=1)[:, -1]                  # integrator += conj(samp) * step_osc(), n = 0 .. 99 in order
        energies = acc.real * acc.real + acc.imag * acc.imag                      # cnrm()
        strongest, index = THRESHOLD, -1
        for n, e in enumerate(energies.tolist()):
            if e > strongest:
                strongest, index = e, n
        if index >= 0 and self.tones[index] > 0:                                  # pl_tone > 0 (:303)
            self.current = index
        self.nblock += 1
        return {"tone_index": index, "current_index": self.current, "energy": strongest, "energies": energies}


def run(blocks, samprate, f32=False, tones=TONES):
    """a fresh Decoder over int16 blocks -> the list of block records"""
    d = Decoder(samprate, tones=tones, f32=f32)
    return [d.block(ao.to_float(b)) for b in blocks]


# ---- the signal ---------------------------------------------------------------------------------------------------------------------
def generate(samprate, segments, seed=None):
    """segments: (nblocks, [(freq Hz, amplitude), ...], noise rms) each; the k-th tone of a segment starts at the phase at which the k-th
    tone of the segment before it ended (continuous phase, whatever the two frequencies).  Samples are rint(32767 x), clipped to the 16-bit range.  -> int16 [nblocks total][L]"""
    L = int(round(FILTER_TIME * samprate))
    rng = np.random.default_rng(seed)
    out, phase = [], {}
    for nblocks, tones, noise in segments:
        n = nblocks * L
        x = np.zeros(n)
        nxt = {}
        for slot, (f, a) in enumerate(tones):
            ph0 = phase.get(slot, 0.0)
            x += a * np.sin(ph0 + 2 * np.pi * f * np.arange(n) / samprate)
            nxt[slot] = (ph0 + 2 * np.pi * f * n / samprate) % (2 * np.pi)
        phase = nxt
        if noise:
            x += noise * rng.standard_normal(n)
        out.append(np.clip(np.rint(32767.0 * x), -32768, 32767).astype(np.int16))
    return np.concatenate(out).reshape(-1, L)


def instance0(samprate):
    """the 55 tones in table order, three blocks each, phase continuous, amplitude 0.05 + 0.01 (k mod 7); 2 blocks of zeros; 100 Hz at 0.005
    (below the threshold, which is amplitude 0.01) for 2 blocks and at 0.012 for 2; 1 block of zeros; 203.5 Hz at 0.9 for 3: 175 blocks, the
    16384th oscillator step (the first renormalisation) in block 163"""
    seg = [(3, [(f, 0.05 + 0.01 * (k % 7))], 0.0) for k, f in enumerate(TONES)]
    seg += [(2, [], 0.0), (2, [(100.0, 0.005)], 0.0), (2, [(100.0, 0.012)], 0.0), (1, [], 0.0), (3, [(203.5, 0.9)], 0.0)]
    return generate(samprate, seg)
