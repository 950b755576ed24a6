"""TEST INFRASTRUCTURE: what the tests of the device-side sig_gen front end (chz_input_generate) share.

The checker of the stream is oracle_lib.SigGen (chzo_siggen_*, which tests/test_oracle_vs_reference.py pins to the reference's own loop).  It
hands out floats only, and only from sample 0 on, so two things are restated here in numpy and pinned to it by tests/test_siggen_host.py:
the generator with the popcount Gaussian in double (for the energy sums, and for the stream at a position 2^40 samples in, which nothing
sequential reaches), and the exact carrier phase in rational arithmetic."""
import fractions
import functools

import numpy as np

import oracle_lib as ol

MASK = (1 << 64) - 1
K1, K2 = 0x2c1b3c6d, 0x297a2d39
SIGMA = 0.1765469659009499
# the issue's parameters
SCALE = {True: ol.scale_ad(True, 1), False: 1.0}            # chzo_scale_ad: 1.41254 REAL, 1.0 COMPLEX
FREQS = (10.00002e6 / 129.6e6, 10e6 / 129.6e6, 0.123456789, 1e-4, 0.4999, -0.2371, 0.25)
IRRATIONAL = (0, 2, 3)                                      # of FREQS: the ones that do not land on ties and zeros


def rotl(x, k):
    return ((x << k) | (x >> (64 - k))) & MASK


def seed(s):
    """xoshiro256ss_seed (src/gauss.c:25-45)"""
    x, out = s & MASK, []
    for _ in range(4):
        x = (x + 0x9E3779B97F4A7C15) & MASK
        z = x
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
        out.append(z ^ (z >> 31))
    if not any(out):
        out[0] = 1
    return tuple(out)


def draws(state, n):
    """(the next n outputs as uint64, the state after them): xoshiro256ss_next (src/gauss.c:47-61)"""
    s0, s1, s2, s3 = state
    out = np.empty(n, np.uint64)
    for i in range(n):
        out[i] = (rotl((s1 * 5) & MASK, 7) * 9) & MASK
        t = (s1 << 17) & MASK
        s2 ^= s0; s3 ^= s1; s1 ^= s2; s0 ^= s3
        s2 ^= t
        s3 = rotl(s3, 45)
    return out, (s0, s1, s2, s3)


def popcount(a):
    return np.unpackbits(np.ascontiguousarray(a).view(np.uint8).reshape(-1, 8), axis=1).sum(axis=1).astype(np.int64)


def gauss(u):
    """real_gauss (src/gauss.c:103-111) of each output, in double and in the reference's order"""
    u = np.ascontiguousarray(u, np.uint64)
    x = (popcount(u * np.uint64(K1)) + popcount(u * np.uint64(K2)) - 64).astype(np.float64)
    x = x + u.view(np.int64).astype(np.float64) * 2.0 ** -63
    return x * SIGMA


def samples_f0(state, n, amplitude, noise, isreal):
    """samp (BEFORE scale, in double) of n samples of a stream whose carrier stands still (freq 0: the phasor is exactly 1), the generator
    starting at `state`: float64[n] or complex128[n]"""
    per = 1 if isreal else 2
    g = gauss(draws(state, n * per)[0])
    if isreal:
        return amplitude * 1.0 + noise * g
    return (amplitude * 1.0 + noise * g[0::2]) + 1j * (amplitude * 0.0 + noise * g[1::2])


def to_ring(samp, scale):
    """(float)(samp * scale), as float32[n] or complex64[n]"""
    if np.iscomplexobj(samp):
        return ((samp.real * scale).astype(np.float32) + 1j * (samp.imag * scale).astype(np.float32)).astype(np.complex64)
    return (samp * scale).astype(np.float32)


def energy(samp):
    """the sequential double sum of samp^2 (re^2 + im^2)"""
    sq = samp.real * samp.real + samp.imag * samp.imag if np.iscomplexobj(samp) else samp * samp
    total = 0.0
    for v in sq.tolist():
        total += v
    return total


def step_cycles(x):
    """osc_step_cycles (chz_finetune.h): the angle of the reference's step phasor after sincospi's reduction of 2x, as a double"""
    y = 2.0 * x
    y -= np.floor(y * 0.5) * 2.0
    if y < 0:
        y += 2.0
    if y >= 2.0:
        y -= 2.0
    return float(0.5 * (y - 2.0 if y >= 1.0 else y))


def exact_phase(a, n):
    """frac(a n) for the double a, exactly"""
    p = fractions.Fraction(a) * n
    return p - (p.numerator // p.denominator)


@functools.lru_cache(maxsize=None)
def reference_stream(freq, amplitude, noise, isreal, n):
    """the checker's first n samples (computed once per parameter set and shared: do not modify)"""
    out = ol.SigGen(freq, amplitude, noise, SCALE[isreal], isreal, seed=1).generate(n)
    out.setflags(write=False)
    return out
