"""Welch power spectra of the raw input on the device (chz_welch_*, kernels welch_seg / welch_sum): radiod's wideband spectrum
analyser, wideband_poll() (src/spectrum.c:308-522), on the samples the engine's input ring holds.

The checker is a float64 numpy restatement of wideband_poll()'s two branches (welch_ref below, every step with the reference's
line), including the float accumulation order.  Every
poll names its window (end_sample) on an idle engine.  Tolerance: relative L2 over the bin vector <= 1e-5 (the project's figure,
BASELINE.md) and every bin within 1e-5 x the strongest bin.

Worst figures measured on the MI355X (all cases of this file): relative L2 1.3e-6, worst bin 7.5e-6 of the strongest."""
import numpy as np
import pytest

import oracle_lib as ol
from conftest import load_pkg

pytestmark = pytest.mark.gpu

TOL = 1e-5
# name: (L, M, in_type, int16 ring)
GEOMETRIES = {"small": (25920, 6481, ol.REAL, False),          # the N = 32,400 real master of the parity tests
              "small_i16": (25920, 6481, ol.REAL, True),
              "small_complex": (11520, 2881, ol.COMPLEX, False),
              "config3": (2592000, 648001, ol.REAL, False)}     # 129.6 MS/s
RING_BLOCKS = 8
SCALE16 = np.float32(1.0 / 32768.0)


@pytest.fixture(scope="module")
def pkg():
    p = load_pkg()
    if p.engine.lib().chz_device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests cannot run (there is no CPU fallback)")
    return p


# ---- the reference, restated ----------------------------------------------------------------------------------------------------
def avg_limit(ring_samples, fft_n, overlap):
    """src/spectrum.c:359 / :417 -- input_buffer_size / (sizeof sample * fft_n) is an integer quotient"""
    return int(np.floor(1 + (ring_samples // fft_n - 1) / (1 - overlap)))


def welch_ref(ring, end, real, fft_n, window, shift, bin_count, fft_avg, overlap):
    """wideband_poll() from :354 on.  ring: the input ring as it stands (float32 / complex64, as the A/D conversion left it),
    end: index just past the newest sample (frontend->in.input_write_pointer).  Returns (bin_data float32, min_power, max_power,
    effective fft_avg)."""
    R = ring.shape[0]
    fft_avg = min(fft_avg, avg_limit(R, fft_n, overlap))                              # :359-362 / :417-420
    window = np.asarray(window, np.float32)
    adjust = int(np.rint(fft_n * (1 + (fft_avg - 1) * (1 - overlap))))                # :364 / :422
    hop = int(np.rint(fft_n * (1. - overlap)))                                        # :407 / :491
    bins = np.zeros(bin_count, np.float32)                                            # :338
    pos = (end - adjust) % R                                                          # :366-368 / :424-426
    idx = np.arange(fft_n)
    if real:
        gain = 2. / (fft_avg * fft_n * fft_n)                                         # :373
        for _ in range(fft_avg):
            x = window * ring[(pos + idx) % R]                                        # :379 (float products)
            if shift < 0:                                                             # :385-390
                x = x.copy(); x[1::2] = -x[1::2]
                if fft_n & 1:
                    x[fft_n - 1] = 0
            X = np.fft.rfft(x.astype(np.float64))                                     # :392
            binp = shift if shift >= 0 else fft_n // 2 + shift                        # :396
            i = 0
            while i < bin_count and binp < fft_n // 2 + 1:                            # :398
                if i == bin_count // 2:
                    binp -= bin_count                                                 # :400
                if binp >= 0:                                                         # (the reference would read in front of its array)
                    p = X[binp].real ** 2 + X[binp].imag ** 2                         # :402
                    if np.isfinite(p):
                        bins[i] = np.float32(np.float64(bins[i]) + gain * p)          # :405
                i += 1; binp += 1
            pos = (pos + hop) % R                                                     # :407-409
    else:
        gain = 1. / (fft_avg * fft_n * fft_n)                                         # :431
        for _ in range(fft_avg):
            x = window * ring[(pos + idx) % R]                                        # :435
            X = np.fft.fft(x.astype(np.complex128))                                   # :437
            for i in range(bin_count):                                                # :477-488
                offset = i if i < bin_count // 2 else i - bin_count
                b = shift + offset
                if b < -(fft_n // 2) or b >= (fft_n + 1) // 2:
                    continue
                binp = b if b >= 0 else b + fft_n
                p = X[binp].real ** 2 + X[binp].imag ** 2
                if np.isfinite(p):
                    bins[i] = np.float32(np.float64(bins[i]) + gain * p)
            pos = (pos - hop) % R                                                     # :491-493
    mn, mx = np.inf, 0.0                                                              # :498-507
    for v in bins:
        mn = min(mn, float(v)); mx = max(mx, float(v))
    return bins, mn, mx, fft_avg


def kaiser_window(fft_n, beta):
    """generate_window(): fft_n + 1 points of which the first fft_n are used, normalised to a sum of fft_n (src/spectrum.c:560,596)"""
    w = np.kaiser(fft_n + 1, beta)[:fft_n]
    return (w * (fft_n / w.sum())).astype(np.float32)


def derandomise(a):
    a = a.astype(np.int32)
    a = np.where(a & 1, a ^ 0xfffe, a)                                                # src/rx888.c:711-716
    return a.astype(np.uint16).astype(np.int16)


# ---- a filled engine and the host's image of its ring ----------------------------------------------------------------------------
class Fed:
    def __init__(self, pkg, geom, seed=1, blocks=RING_BLOCKS + 3):
        L, M, in_type, i16 = GEOMETRIES[geom]
        self.real, self.L, self.M = in_type == ol.REAL, L, M
        self.eng = pkg.engine.Engine(L, M, in_type, ring_blocks=RING_BLOCKS)
        self.R = RING_BLOCKS * L
        self.ring = np.zeros(self.R, np.float32 if self.real else np.complex64)
        self.pos = M - 1                                                              # src/filter.c:244,259
        self.i16 = i16
        self.rng = np.random.default_rng(seed)
        for _ in range(blocks):                                                       # more than the ring holds: the write position has wrapped
            self.feed(L)

    def feed(self, n, sync=True):
        t = self.pos + np.arange(n)
        if self.real:
            x = 0.2 * np.cos(2 * np.pi * (0.11 * t + 1e-9 * t * t)) + 0.05 * np.cos(2 * np.pi * 0.3127 * t) + 0.02 * self.rng.standard_normal(n)
        else:
            x = (0.2 * np.exp(2j * np.pi * 0.21 * t) + 0.05 * np.exp(-2j * np.pi * 0.3127 * t)
                 + 0.02 * (self.rng.standard_normal(n) + 1j * self.rng.standard_normal(n)))
        if self.i16:
            raw = np.clip(np.rint(x * 20000), -32768, 32767).astype(np.int16)
            x = derandomise(raw).astype(np.float32) * SCALE16                         # convert(), src/rx888.c:753-767
            assert sync
            self.eng.write_i16(raw, SCALE16, randomize=True)
        else:
            x = x.astype(self.ring.dtype)
            if sync:
                self.eng.write(x)
            else:
                self.keep = np.ascontiguousarray(x)                                   # stays alive until the caller has synchronised
                lib = self.eng_lib
                assert lib.chz_input_write(self.eng._h, self.keep.ctypes.data, n) == 0
        self.ring[(self.pos + np.arange(n)) % self.R] = x
        self.pos = (self.pos + n) % self.R


_fed = {}


@pytest.fixture(scope="module")
def fed(pkg):
    def get(geom):
        if geom not in _fed:
            _fed[geom] = Fed(pkg, geom)
            _fed[geom].eng_lib = pkg.engine.lib()
        return _fed[geom]
    yield get
    for f in _fed.values():
        f.eng.close()
    _fed.clear()


def compare(got, want, what):
    got = np.asarray(got, np.float64); want = np.asarray(want, np.float64)
    top = np.abs(want).max()
    assert top > 0, what
    l2 = np.linalg.norm(got - want) / np.linalg.norm(want)
    worst = np.abs(got - want).max() / top
    print("WELCH %s: rel L2 %.3g, worst bin %.3g of the strongest" % (what, l2, worst))
    assert l2 <= TOL and worst <= TOL, (what, l2, worst)
    return l2, worst


def run_case(f, fft_n, shift, bin_count, fft_avg, overlap, end, beta=7.0, max_avg=None, packed=None):
    w = f.eng.welch(fft_n, 2, bin_count, max_avg or fft_avg, packed=packed)
    try:
        win = kaiser_window(fft_n, beta)
        w.set_window(1, win)
        eff = w.configure(1, shift, bin_count, fft_avg, overlap)
        w.poll([1], end=end)
        (bins,), (mm,) = w.read()
    finally:
        w.close()
    want, mn, mx, eff_ref = welch_ref(f.ring, end, f.real, fft_n, win, shift, bin_count, fft_avg, overlap)
    assert eff == eff_ref
    assert bins.shape == want.shape
    assert mm[0] == bins.min() and mm[1] == bins.max()
    return bins, want


# (geometry, fft_n, shift, bin_count, fft_avg, overlap, where the window ends: "newest" or "wrap")
#   648, 6480, 6075 (odd): two buffers in LDS; 12960, 129600: global scratch; 18514 = 2 x 9257 (prime): Bluestein over 65536 points
CASES = [
    ("small", 648, 37, 200, 8, 0.5, "newest"),
    ("small", 648, -100, 201, 3, 0.0, "wrap"),
    ("small", 648, 300, 100, 8, 0.75, "newest"),          # the walk runs off the top of the front end's coverage (:398)
    ("small", 648, 10, 100, 1, 0.5, "wrap"),              # the negative output half reads in front of bin 0: zeros
    ("small", 6480, 1000, 1620, 3, 0.5, "wrap"),
    ("small", 6480, -2000, 1621, 8, 0.75, "newest"),
    ("small", 6075, 500, 301, 3, 0.5, "newest"),
    ("small", 6075, -700, 300, 3, 0.5, "wrap"),           # odd fft_n, inverted: the last sample is dropped (:389)
    ("small", 12960, 2000, 1620, 3, 0.5, "wrap"),
    ("small", 12960, -3000, 1621, 8, 0.75, "newest"),
    ("small", 18514, 3000, 1000, 3, 0.5, "wrap"),
    ("small", 18514, -4000, 1001, 1, 0.0, "newest"),
    ("small", 129600, 20000, 1620, 8, 0.5, "newest"),     # fft_avg above what the ring holds: 1
    ("small_i16", 6480, 1000, 1620, 3, 0.5, "wrap"),
    ("small_i16", 648, -50, 201, 8, 0.75, "newest"),
    ("small_i16", 12960, 2000, 1621, 3, 0.0, "newest"),
    ("small_complex", 648, 300, 200, 3, 0.5, "newest"),   # off the upper band edge
    ("small_complex", 648, -310, 201, 8, 0.0, "wrap"),    # off the lower band edge
    ("small_complex", 6480, 100, 1620, 8, 0.75, "wrap"),
    ("small_complex", 6075, -1000, 301, 3, 0.5, "newest"),
    ("small_complex", 12960, 6000, 1620, 3, 0.5, "wrap"),
    ("small_complex", 18514, -9000, 1001, 3, 0.5, "newest"),
    ("config3", 6480, 1000, 1620, 8, 0.5, "newest"),
    ("config3", 6480, -2000, 1621, 3, 0.75, "wrap"),
    ("config3", 129600, 30000, 1620, 4, 0.5, "wrap"),
    ("config3", 129600, -40000, 1621, 3, 0.75, "newest"),
    ("config3", 129600, 100, 1620, 8, 0.0, "newest"),
]


def test_the_large_prime_size_is_what_it_claims():
    assert 18514 == 2 * 9257 and all(9257 % d for d in range(2, 97))                  # 97^2 > 9257: 9257 is prime


@pytest.mark.parametrize("geom,fft_n,shift,bin_count,fft_avg,overlap,where", CASES,
                         ids=["%s-n%d-s%d-b%d-a%d-o%g-%s" % c for c in CASES])
def test_bins_match_the_restated_reference(fed, geom, fft_n, shift, bin_count, fft_avg, overlap, where):
    f = fed(geom)
    end = f.pos if where == "newest" else fft_n // 3                                  # "wrap": the window starts near the ring's end
    lim = avg_limit(f.R, fft_n, overlap)
    bins, want = run_case(f, fft_n, shift, bin_count, fft_avg, overlap, end, max_avg=min(fft_avg, lim))
    compare(bins, want, "%s fft_n=%d shift=%d bins=%d avg=%d overlap=%g %s" % (geom, fft_n, shift, bin_count, fft_avg, overlap, where))
    if geom != "small_complex" and shift >= 0 and shift + bin_count // 2 > fft_n // 2 + 1:
        assert not bins[fft_n // 2 + 1 - shift:].any()                                # beyond the coverage: untouched zeros


PACKED_CASES = [c for c in CASES if c[0] != "small_complex" and c[1] % 2 == 0 and c[1] != 18514]


@pytest.mark.parametrize("geom,fft_n,shift,bin_count,fft_avg,overlap,where", PACKED_CASES,
                         ids=["%s-n%d-s%d-b%d-a%d-o%g-%s" % c for c in PACKED_CASES])
def test_packed_real_transform_matches_the_restated_reference(fed, geom, fft_n, shift, bin_count, fft_avg, overlap, where):
    """option welch_packed: a real front end's even fft_n as an fft_n/2-point transform of sample pairs with the Hermitian split where
    the bins are read -- the same cases, the same bound"""
    f = fed(geom)
    end = f.pos if where == "newest" else fft_n // 3
    lim = avg_limit(f.R, fft_n, overlap)
    bins, want = run_case(f, fft_n, shift, bin_count, fft_avg, overlap, end, max_avg=min(fft_avg, lim), packed=True)
    compare(bins, want, "packed %s fft_n=%d shift=%d bins=%d avg=%d overlap=%g %s" % (geom, fft_n, shift, bin_count, fft_avg, overlap, where))
    full, _ = run_case(f, fft_n, shift, bin_count, fft_avg, overlap, end, max_avg=min(fft_avg, lim), packed=False)
    assert np.array_equal(full == 0, bins == 0)                                       # the same bins lie outside the coverage


@pytest.mark.parametrize("geom", ["small", "small_complex"])
def test_fft_avg_is_clamped_by_the_ring_as_the_reference_clamps(fed, geom):
    f = fed(geom)
    for fft_n, overlap in ((12960, 0.0), (6480, 0.5), (12960, 0.75)):
        lim = avg_limit(f.R, fft_n, overlap)
        w = f.eng.welch(fft_n, 1, 16, lim)
        try:
            assert w.configure(0, 0, 16, 10 * lim + 3, overlap) == lim
            assert w.configure(0, 0, 16, lim, overlap) == lim
            assert w.configure(0, 0, 16, max(1, lim - 1), overlap) == max(1, lim - 1)
        finally:
            w.close()
    bins, want = run_case(f, 12960, 700, 64, 1000, 0.0, f.pos, max_avg=avg_limit(f.R, 12960, 0.0))
    compare(bins, want, "%s clamped fft_avg" % geom)


def test_refusals(fed, pkg):
    f = fed("small")
    for fft_n in (4, (1 << 20) + 2, 600011):                                          # too short, too long, 600011 is prime: 2^21 points of chirp-z
        with pytest.raises(pkg.engine.ChzError):
            f.eng.welch(fft_n, 1, 16, 1)
    with pytest.raises(pkg.engine.ChzError):
        f.eng.welch(f.R + 6, 1, 16, 1)                                                # longer than the ring


# ---- pins that use no transform on the checking side -------------------------------------------------------------------------------
def tone_ring(f, fft_n, k0, amp):
    """overwrite the whole ring with a cosine on bin k0 of an fft_n-point transform (same phase origin for every segment start)"""
    n = np.arange(f.R)
    x = amp * np.cos(2 * np.pi * k0 * n / fft_n + 0.3)
    return x


@pytest.mark.parametrize("fft_n,k0", [(6480, 1234), (648, 100), (12960, 4001)])
def test_bin_centred_cosine_in_closed_form(pkg, fft_n, k0):
    L, M = 25920, 6481
    eng = pkg.engine.Engine(L, M, ol.REAL, ring_blocks=RING_BLOCKS)
    R, amp = RING_BLOCKS * L, 0.37
    try:
        # R is a multiple of fft_n for these sizes: the tone is continuous across the ring's wrap
        assert R % fft_n == 0
        x = tone_ring(type("F", (), {"R": R}), fft_n, k0, amp).astype(np.float32)
        x = np.roll(x, -(M - 1))                                                       # the first sample written lands on ring index M - 1
        for b in range(RING_BLOCKS):
            eng.write(x[b * L:(b + 1) * L])
        w = eng.welch(fft_n, 2, 9, 4)
        # rectangular window: a^2/2 on the tone's bin, the float floor next to it
        w.set_window(0, np.ones(fft_n, np.float32))
        w.configure(0, k0, 9, 4, 0.5)
        # normalised Kaiser window (sum = fft_n): the neighbours follow from the window's own sums
        win = kaiser_window(fft_n, 7.0)
        w.set_window(1, win)
        w.configure(1, k0, 9, 4, 0.5)
        w.poll([0, 1], end=1000)
        (rect, kais), _ = w.read()
        # output bins 0..3 are k0..k0+3, bins 4..8 are k0-5..k0-1 (the wrap at i == bin_count/2, :399-400)
        assert abs(rect[0] / (amp * amp / 2) - 1) <= TOL
        assert np.abs(np.delete(rect, 0)).max() <= 1e-10 * amp * amp                   # float32 products: ~(6e-8)^2 of the tone, spread
        n = np.arange(fft_n)
        w64 = win.astype(np.float64)
        adjust, hop = int(np.rint(fft_n * 2.5)), fft_n // 2                            # :364, :407 with fft_avg 4, overlap 0.5
        for i, d in ((0, 0), (1, 1), (2, 2), (8, -1), (7, -2)):
            S = np.sum(w64 * np.exp(-2j * np.pi * d * n / fft_n))                      # the window's own spectrum at offset d ...
            S2 = np.sum(w64 * np.exp(-2j * np.pi * (2 * k0 + d) * n / fft_n))          # ... and at the image of the negative-frequency half
            want = 0.0
            for seg in range(4):
                ph = 0.3 + 2 * np.pi * k0 * ((1000 - adjust + seg * hop) % fft_n) / fft_n     # the tone's phase where the segment starts
                want += 2. / (4 * fft_n ** 2) * abs(amp / 2 * (np.exp(1j * ph) * S + np.exp(-1j * ph) * S2)) ** 2
            assert abs(kais[i] - want) <= TOL * amp * amp / 2, (i, d, kais[i], want)
        assert abs(kais[0] / (amp * amp / 2) - 1) <= 1e-4                              # coherent gain 1
    finally:
        eng.close()


# ---- determinism, batching, ordering -------------------------------------------------------------------------------------------------
def test_polls_repeat_bit_for_bit_and_a_batch_equals_single_polls(fed):
    f = fed("small")
    fft_n, nslots, bin_count = 648, 64, 200
    w = f.eng.welch(fft_n, nslots, bin_count, 8)
    try:
        rng = np.random.default_rng(5)
        for s in range(nslots):
            w.set_window(s, kaiser_window(fft_n, 3.0 + 0.1 * s))
            w.configure(s, int(rng.integers(-300, 300)), bin_count - (s & 1), 1 + s % 8, (0.0, 0.5, 0.75)[s % 3])
        w.poll(end=f.pos)
        a, amm = w.read()
        w.poll(end=f.pos)
        b, bmm = w.read()
        assert len(a) == nslots
        for s in range(nslots):
            assert np.array_equal(a[s], b[s]) and np.array_equal(amm[s], bmm[s])
        for s in range(nslots):
            w.poll([s], end=f.pos)
            (one,), (mm,) = w.read()
            assert np.array_equal(one, a[s]) and np.array_equal(mm, amm[s]), s
    finally:
        w.close()


def test_a_poll_sees_the_write_issued_just_before_it(pkg):
    f = Fed(pkg, "small", seed=9, blocks=2)
    f.eng_lib = pkg.engine.lib()
    try:
        fft_n = 6480
        w = f.eng.welch(fft_n, 1, 1620, 3)
        win = kaiser_window(fft_n, 7.0)
        w.set_window(0, win)
        w.configure(0, 500, 1620, 3, 0.5)
        f.eng.sync()
        f.feed(f.L, sync=False)                                                        # no synchronisation between the write ...
        w.poll([0])                                                                    # ... and the poll of "everything written so far"
        (bins,), _ = w.read()
        f.eng.sync()
        want = welch_ref(f.ring, f.pos, True, fft_n, win, 500, 1620, 3, 0.5)[0]
        compare(bins, want, "poll right behind a write")
        old = welch_ref(f.ring, (f.pos - f.L) % f.R, True, fft_n, win, 500, 1620, 3, 0.5)[0]
        assert np.linalg.norm(bins - old) > 1e-3 * np.linalg.norm(want)               # (the window before the write reads differently)
        w.close()
    finally:
        f.eng.close()


def test_a_write_over_samples_a_poll_still_reads_waits_for_the_poll(pkg):
    """A long poll (64 analysers x 16 segments of 12,960 points, transformed in global scratch) reading the whole ring, then -- with no
    synchronisation -- eight blocks written over the whole ring: the poll's result is that of the ring as it stood when the poll
    was issued; a second poll then sees the new samples."""
    f = Fed(pkg, "small", seed=11, blocks=RING_BLOCKS)
    f.eng_lib = pkg.engine.lib()
    try:
        fft_n, nslots, bins = 12960, 64, 800
        w = f.eng.welch(fft_n, nslots, bins, 16)
        win = kaiser_window(fft_n, 7.0)
        for s in range(nslots):
            w.set_window(s, win)
            assert w.configure(s, 100 * s, bins, 16, 0.0) == 16                       # 16 x 12,960 = the whole ring
        f.eng.sync()
        before, end = f.ring.copy(), f.pos
        w.poll(end=end)
        kept = []
        for _ in range(RING_BLOCKS):                                                  # every sample the poll reads is overwritten
            f.feed(f.L, sync=False); kept.append(f.keep)
        got, _ = w.read()
        f.eng.sync()
        for s in (0, 17, 63):
            compare(got[s], welch_ref(before, end, True, fft_n, win, 100 * s, bins, 16, 0.0)[0], "poll against later writes, analyser %d" % s)
        w.poll([5], end=f.pos)
        (after,), _ = w.read()
        compare(after, welch_ref(f.ring, f.pos, True, fft_n, win, 500, bins, 16, 0.0)[0], "poll after those writes")
        assert np.linalg.norm(after - got[5]) > 1e-3 * np.linalg.norm(after)
        w.close()
    finally:
        f.eng.close()


def test_async_read_completes_through_the_host_callback(fed, pkg):
    import ctypes as C
    f = fed("small")
    lib = pkg.engine.lib()
    w = f.eng.welch(648, 2, 100, 2)
    try:
        for s in range(2):
            w.set_window(s, kaiser_window(648, 5.0))
            w.configure(s, 20 * s, 100, 2, 0.5)
        w.poll(end=f.pos)
        want, wmm = w.read()
        w.poll(end=f.pos)
        rows = np.zeros((2, 100), np.float32); mm = np.zeros((2, 2), np.float64)
        assert lib.chz_welch_read_async(f.eng._h, w.id, 0, 2, rows.ctypes.data, mm.ctypes.data) == 0
        fired = []
        CB = C.CFUNCTYPE(None, C.c_void_p)
        cb = CB(lambda arg: fired.append(1))
        lib.chz_host_callback.argtypes = [C.c_void_p, C.c_int, CB, C.c_void_p]
        assert lib.chz_host_callback(f.eng._h, -2, cb, None) == 0                      # CHZ_SLOT_WELCH
        lib.chz_slot_sync.argtypes = [C.c_void_p, C.c_int]
        assert lib.chz_slot_sync(f.eng._h, -2) == 0
        assert fired == [1]
        assert np.array_equal(rows[0], want[0]) and np.array_equal(rows[1], want[1]) and np.array_equal(mm[1], wmm[1])
    finally:
        w.close()
