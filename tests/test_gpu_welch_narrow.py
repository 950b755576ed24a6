"""Welch power spectra of a channel's baseband on the device (chz_bank_welch_*, Bank.spectrum; kernels bb_ring_append, welch_seg with a
baseband source, welch_sum): radiod's narrowband spectrum analyser, narrowband_poll() (src/spectrum.c:206-306) on the ring that
demod_spectrum() (:123-155) keeps of chan->baseband.

The checker is a float64 numpy restatement of those lines (nb_ref below, every step with the reference's line), applied to the
concatenation of the bank's OWN outputs read back block by block (Bank.read_slot), float32 as the device left them: it judges the
device's ring and the analysis, not the channelizer.  Tolerance: the project's figure (TOL and compare() of
tests/test_gpu_welch.py): relative L2 over the bin vector <= 1e-5 and every bin within 1e-5 x the strongest bin.

Worst figures over all cases of this file, measured on an MI355X (compare() prints every case's, pytest -s): relative L2 1.9e-7, worst bin
2.7e-7 of the strongest.  On the emulated engine (the same kernels compiled for the CPU, tests/test_welch_narrow_emulated.py): 9.6e-8 and 1.1e-7."""
import numpy as np
import pytest

import oracle_lib as ol
from conftest import load_pkg
from test_gpu_welch import Fed, GEOMETRIES, RING_BLOCKS, TOL, compare, kaiser_window

pytestmark = pytest.mark.gpu

NCH = 6
ND = 4                                                                                # CHZ_ND: blocks in flight, output images per bank
# the register-tiled menu / chan_any (one workgroup per channel); P = olen N / L for both masters (N / L = 1.25)
SHAPES = {"tiled": (300, 240), "any": (60, 48)}


@pytest.fixture(scope="module")
def pkg():
    p = load_pkg()
    if p.engine.lib().chz_device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests cannot run (there is no CPU fallback)")
    return p


# ---- the reference, restated ----------------------------------------------------------------------------------------------------
def nb_steps(fft_n, fft_avg, overlap):
    """(hop, adjust): the reference copies fft_n samples forwards (:259-264) and steps lrint(fft_n overlap) back (:278); the first
    segment starts lrint(fft_n (1 + (fft_avg - 1)(1 - overlap))) in front of the write index (:247)"""
    return fft_n - int(np.rint(fft_n * overlap)), int(np.rint(fft_n * (1 + (fft_avg - 1) * (1 - overlap))))


def nb_ref(hist, fft_n, window, bin_count, fft_avg, overlap):
    """demod_spectrum()'s ring followed by narrowband_poll().  hist: every baseband sample of the channel since the analyser was
    created (complex64), the newest last.  Returns (bin_data float32, min_power, max_power)."""
    ring_size = fft_avg * fft_n                                                       # :131
    ring = np.zeros(ring_size, np.complex64)                                          # :144 (a fresh ring is zeros)
    tail = hist[-ring_size:]
    first = len(hist) - len(tail)
    ring[(first + np.arange(len(tail))) % ring_size] = tail                           # :147-151
    ring_idx = len(hist) % ring_size
    window = np.asarray(window, np.float32)
    rp = ring_idx - int(np.rint(fft_n * (1 + (fft_avg - 1) * (1 - overlap))))         # :247
    if rp < 0:
        rp += ring_size                                                               # :248-249
    gain = 1.0 / (float(fft_n) * fft_n * fft_avg)                                     # :255
    bins = np.zeros(bin_count, np.float32)                                            # :219
    fr = np.arange(bin_count)                                                         # :267-276
    fr[bin_count // 2:] = fft_n - bin_count // 2 + np.arange(bin_count - bin_count // 2)
    ok = fr < fft_n                                                                   # (the reference's assert, :271: an odd bin_count's last bin)
    for _ in range(fft_avg):
        x = ring[(rp + np.arange(fft_n)) % ring_size] * window                        # :261 (float products)
        rp = (rp + fft_n) % ring_size                                                 # :262-263
        X = np.fft.fft(x.astype(np.complex128))                                       # :265
        p = np.zeros(bin_count)
        p[ok] = X[fr[ok]].real ** 2 + X[fr[ok]].imag ** 2                             # :272
        p[~np.isfinite(p)] = 0                                                        # :274
        bins[ok] = (bins[ok].astype(np.float64) + gain * p[ok]).astype(np.float32)    # :275 (float += double)
        rp -= int(np.rint(fft_n * overlap))                                           # :278
        if rp < 0:
            rp += ring_size
    mn, mx = np.inf, 0.0                                                              # :284-293
    for v in bins:
        mn = min(mn, float(v)); mx = max(mx, float(v))
    return bins, mn, mx


# ---- an engine with its ring filled once (Fed.feed's tones plus noise), one bank, every block's rows read back ------------------
class Run:
    def __init__(self, pkg, geom, shape, tuned=False, seed=1):
        self.fed = Fed(pkg, geom, seed=seed, blocks=RING_BLOCKS)                      # the whole ring written: any block number can be stepped
        self.eng = self.fed.eng
        L, M, in_type, _ = GEOMETRIES[geom]
        N = L + M - 1
        self.P, self.olen = SHAPES[shape]
        self.bank = self.eng.bank(self.P, self.olen, NCH)
        rng = np.random.default_rng(7)
        resp = (rng.standard_normal((NCH, self.P)) + 1j * rng.standard_normal((NCH, self.P))) / self.P
        self.bank.set_responses(0, resp.astype(np.complex64))
        tone = int(round((0.11 if in_type == ol.REAL else 0.21) * N))                 # Fed.feed's strong tone
        self.shifts = np.array([tone - 20, tone - 5, tone, tone + 7, tone + 25, tone + 1000], np.int32)
        if tuned:                                                                     # downconvert()'s fine rotation: a fraction of an output bin
            self.bank.set_tuning(0, 0, self.shifts, np.full(NCH, 0.37 / 300.0))
        else:
            self.bank.set_shifts(0, self.shifts)
        self.bank.set_active(NCH)
        self.rows = {}
        self.next = 0

    def step(self, n=1):
        for _ in range(n):
            self.eng.step(self.next)
            self.rows[self.next] = self.bank.read_slot(self.next % ND)
            self.next += 1
        return self.next - 1

    def hist(self, ch, job0, job):
        return np.concatenate([self.rows[j][ch] for j in range(job0, job + 1)])

    def close(self):
        self.eng.close()


_runs = {}


@pytest.fixture(scope="module")
def run(pkg):
    def get(geom, shape):
        if (geom, shape) not in _runs:
            _runs[(geom, shape)] = Run(pkg, geom, shape)
        return _runs[(geom, shape)]
    yield get
    for r in _runs.values():
        r.close()
    _runs.clear()


def blocks_for(olen, fft_n, fft_avg):
    return -(-fft_avg * fft_n // olen) + 2                                            # the reference's whole ring, and a little more


# (geometry, shape, fft_n, bin_count, fft_avg, overlap)
#   64: several segments inside one block; 75 with overlap 0.5: hop 37, not 38; 300, 1000: the window spans more than four blocks and
#   fft_n does not divide the ring; 1031: prime, chirp-z over 4096 points; 10368: transformed in global scratch
CASES = [
    ("small_complex", "tiled", 64, 64, 1, 0.0),
    ("small_complex", "any", 8, 8, 50, 0.9),              # hop 1, adjust 47: the last segments START past the end of the window
    ("small_complex", "any", 64, 32, 3, 0.5),
    ("small", "tiled", 64, 64, 8, 0.75),
    ("small_complex", "tiled", 75, 74, 3, 0.5),
    ("small", "any", 75, 40, 8, 0.5),
    ("small_complex", "any", 75, 74, 8, 0.75),
    ("small", "tiled", 75, 20, 1, 0.5),
    ("small_complex", "tiled", 300, 300, 8, 0.0),
    ("small", "any", 300, 128, 3, 0.5),
    ("small", "tiled", 300, 300, 8, 0.75),
    ("small_complex", "any", 300, 200, 1, 0.0),
    ("small_complex", "tiled", 1000, 1000, 3, 0.5),
    ("small", "tiled", 1000, 400, 8, 0.75),
    ("small_complex", "any", 1000, 1000, 1, 0.0),
    ("small", "any", 1000, 500, 3, 0.0),
    ("small_complex", "tiled", 1031, 1030, 3, 0.5),
    ("small", "any", 1031, 512, 1, 0.0),
    ("small", "tiled", 1031, 600, 8, 0.75),
    ("small_complex", "tiled", 10368, 2000, 3, 0.5),
    ("small", "tiled", 10368, 10368, 1, 0.0),
]


def test_the_prime_size_is_what_it_claims():
    assert all(1031 % d for d in range(2, 33))                                        # 33^2 > 1031


@pytest.mark.parametrize("geom,shape,fft_n,bin_count,fft_avg,overlap", CASES, ids=["%s-%s-n%d-b%d-a%d-o%g" % c for c in CASES])
def test_bins_match_the_restated_reference(run, geom, shape, fft_n, bin_count, fft_avg, overlap):
    r = run(geom, shape)
    sp = r.bank.spectrum(fft_n, 2, bin_count, fft_avg)
    try:
        win = kaiser_window(fft_n, 7.0)
        ch, job0 = 2, r.next
        sp.attach(1, ch, job0)
        sp.set_window(1, win)
        assert sp.configure(1, bin_count, fft_avg, overlap) == fft_avg
        job = r.step(blocks_for(r.olen, fft_n, fft_avg))
        sp.poll([1], job)
        (bins,), (mm,) = sp.read()
    finally:
        sp.close()
    want, mn, mx = nb_ref(r.hist(ch, job0, job), fft_n, win, bin_count, fft_avg, overlap)
    assert bins.shape == want.shape
    assert mm[0] == bins.min() and mm[1] == bins.max()
    compare(bins, want, "%s %s fft_n=%d bins=%d avg=%d overlap=%g" % (geom, shape, fft_n, bin_count, fft_avg, overlap))


def test_an_odd_bin_count_leaves_its_last_bin_zero(run):
    r = run("small_complex", "tiled")
    fft_n, bc = 300, 101
    sp = r.bank.spectrum(fft_n, 1, bc, 3)
    try:
        win = kaiser_window(fft_n, 7.0)
        job0 = r.next
        sp.attach(0, 1, job0); sp.set_window(0, win); sp.configure(0, bc, 3, 0.5)
        job = r.step(blocks_for(r.olen, fft_n, 3))
        sp.poll([0], job)
        (bins,), (mm,) = sp.read()
    finally:
        sp.close()
    want = nb_ref(r.hist(1, job0, job), fft_n, win, bc, 3, 0.5)[0]
    assert bins[-1] == 0 and want[-1] == 0 and mm[0] == 0
    compare(bins[:-1], want[:-1], "odd bin_count, the bins in front of the last")


@pytest.mark.parametrize("shape", ["tiled", "any"])
def test_a_poll_before_the_ring_has_filled_sees_leading_zeros(run, shape):
    r = run("small_complex", shape)
    fft_n, avg = 1000, 3
    sp = r.bank.spectrum(fft_n, 1, fft_n, avg)
    try:
        win = kaiser_window(fft_n, 7.0)
        r.step(3)                                                                     # blocks from before the attach must not show
        job0 = r.next
        sp.attach(0, 3, job0); sp.set_window(0, win); sp.configure(0, fft_n, avg, 0.5)
        job = r.step(2)                                                               # 480 or 96 samples of a window of 2000
        sp.poll([0], job)
        (bins,), _ = sp.read()
    finally:
        sp.close()
    hist = r.hist(3, job0, job)
    assert len(hist) < fft_n
    compare(bins, nb_ref(hist, fft_n, win, fft_n, avg, 0.5)[0], "%s: two blocks into an empty ring" % shape)


def test_a_poll_after_the_ring_has_wrapped_twice(run):
    r = run("small", "tiled")
    fft_n, avg = 64, 8
    sp = r.bank.spectrum(fft_n, 1, 64, avg)
    try:
        ring_len = avg * fft_n + (ND + 1) * r.olen                                    # 1712 samples: 7.13 blocks
        win = kaiser_window(fft_n, 5.0)
        job0 = r.next
        sp.attach(0, 0, job0); sp.set_window(0, win); sp.configure(0, 64, avg, 0.0)
        got = []
        for _ in range(3):                                                            # at three different phases of the ring
            job = r.step(8)
            sp.poll([0], job)
            got.append((job, sp.read()[0][0]))
        assert (job - job0 + 1) * r.olen > 3 * ring_len
    finally:
        sp.close()
    for job, bins in got:
        compare(bins, nb_ref(r.hist(0, job0, job), fft_n, win, 64, avg, 0.0)[0], "ring wrapped, block %d" % (job - job0))


# ---- ordering and identity -------------------------------------------------------------------------------------------------------
def test_polls_repeat_bit_for_bit_and_a_batch_equals_single_polls(run):
    r = run("small_complex", "tiled")
    fft_n, nslots = 300, 12
    sp = r.bank.spectrum(fft_n, nslots, fft_n, 8)
    try:
        job0 = r.next
        for s in range(nslots):
            sp.attach(s, s % NCH, job0)
            sp.set_window(s, kaiser_window(fft_n, 3.0 + 0.3 * s))
            sp.configure(s, fft_n - 2 * s, 1 + s % 8, (0.0, 0.5, 0.75)[s % 3])
        job = r.step(blocks_for(r.olen, fft_n, 8))
        sp.poll(job=job)
        a, amm = sp.read()
        sp.poll(job=job)
        b, bmm = sp.read()
        assert len(a) == nslots
        for s in range(nslots):
            assert np.array_equal(a[s], b[s]) and np.array_equal(amm[s], bmm[s])
            sp.poll([s], job)
            (one,), (mm,) = sp.read()
            assert np.array_equal(one, a[s]) and np.array_equal(mm, amm[s]), s
        for s in (0, 5, 11):
            want = nb_ref(r.hist(s % NCH, job0, job), fft_n, kaiser_window(fft_n, 3.0 + 0.3 * s), fft_n - 2 * s, 1 + s % 8, (0.0, 0.5, 0.75)[s % 3])[0]
            compare(a[s], want, "batch, analyser %d" % s)
    finally:
        sp.close()


def _spectra(pkg, shape, drive):
    """a fresh engine, two analysers (fft_n 300), blocks 5 .. 5 + 23 driven by `drive(run, first, n)`, polled at the last one"""
    r = Run(pkg, "small_complex", shape)
    try:
        fft_n, j0, n = 300, 5, 24
        sp = r.bank.spectrum(fft_n, 2, fft_n, 8)
        for s, ch in ((0, 2), (1, 4)):
            sp.attach(s, ch, j0); sp.set_window(s, kaiser_window(fft_n, 6.0)); sp.configure(s, fft_n, 8, 0.5)
        r.next = j0
        drive(r, j0, n)
        sp.poll([0, 1], j0 + n - 1)
        bins, mm = sp.read()
        r.eng.sync()
        if r.rows:                                                                    # (read back block by block: the restatement applies)
            for s, ch in ((0, 2), (1, 4)):
                compare(bins[s], nb_ref(r.hist(ch, j0, j0 + n - 1), fft_n, kaiser_window(fft_n, 6.0), fft_n, 8, 0.5)[0], "stepped, analyser %d" % s)
        return bins, mm, r.bank.read_slot((j0 + n - 1) % ND)
    finally:
        r.close()


@pytest.mark.parametrize("shape", ["tiled", "any"])
def test_blocks_in_flight_equal_blocks_stepped_one_at_a_time(pkg, shape):
    """run_blocks keeps four blocks in flight over four lanes and two issuing threads (from an engine's second long call on);
    stepping runs one block at a time: the rings, and so the spectra, are the same bits"""
    def stepped(r, j0, n):
        r.step(n)

    def in_flight(r, j0, n):
        r.eng.run_blocks(j0, 8)                                                       # (starts the issuing threads)
        r.eng.run_blocks(j0 + 8, n - 8)

    want, wmm, wrows = _spectra(pkg, shape, stepped)
    got, gmm, grows = _spectra(pkg, shape, in_flight)
    assert np.array_equal(grows, wrows)
    for s in range(2):
        assert want[s].max() > 0
        assert np.array_equal(got[s], want[s]) and np.array_equal(gmm[s], wmm[s]), s


def test_a_rerun_of_a_block_rewrites_the_same_ring_samples(run):
    r = run("small_complex", "any")
    fft_n = 300
    sp = r.bank.spectrum(fft_n, 2, fft_n, 3)
    try:
        job0 = r.next
        for s, ch in ((0, 1), (1, 4)):
            sp.attach(s, ch, job0); sp.set_window(s, kaiser_window(fft_n, 6.0)); sp.configure(s, fft_n, 3, 0.5)
        job = r.step(blocks_for(r.olen, fft_n, 3))
        sp.poll([0, 1], job)
        a, _ = sp.read()
        r.bank.execute_range(job, 1, 1)                                               # the drop-in's miss path: channel 1 of the newest block ...
        r.bank.execute_range(job - 2, 4, 1)                                           # ... and channel 4 of an older one, still held by its slot
        sp.poll([0, 1], job)
        b, _ = sp.read()
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        compare(b[0], nb_ref(r.hist(1, job0, job), fft_n, kaiser_window(fft_n, 6.0), fft_n, 3, 0.5)[0], "after the re-run")
    finally:
        sp.close()


def test_two_banks_of_different_fft_n_on_one_channel(run):
    r = run("small", "tiled")
    spa, spb = r.bank.spectrum(64, 1, 64, 8), r.bank.spectrum(300, 1, 300, 3)
    try:
        job0 = r.next
        wa, wb = kaiser_window(64, 4.0), kaiser_window(300, 7.0)
        spa.attach(0, 2, job0); spa.set_window(0, wa); spa.configure(0, 64, 8, 0.5)
        spb.attach(0, 2, job0); spb.set_window(0, wb); spb.configure(0, 300, 3, 0.75)
        job = r.step(6)
        spa.poll([0], job); spb.poll([0], job)
        (a,), _ = spa.read()
        (b,), _ = spb.read()
    finally:
        spa.close(); spb.close()
    h = r.hist(2, job0, job)
    compare(a, nb_ref(h, 64, wa, 64, 8, 0.5)[0], "fft_n 64 beside 300")
    compare(b, nb_ref(h, 300, wb, 300, 3, 0.75)[0], "fft_n 300 beside 64")
    r.step(2)                                                                         # both gone: the bank runs on without its appends


def test_a_poll_with_later_blocks_enqueued_equals_the_poll_on_an_idle_engine(run):
    r = run("small_complex", "tiled")
    fft_n = 1000
    sp = r.bank.spectrum(fft_n, 1, fft_n, 3)
    try:
        win = kaiser_window(fft_n, 7.0)
        job0 = r.next
        sp.attach(0, 2, job0); sp.set_window(0, win); sp.configure(0, fft_n, 3, 0.5)
        job = r.step(blocks_for(r.olen, fft_n, 3))
        sp.poll([0], job)
        (idle,), _ = sp.read()
        r.eng.sync()
        for j in range(job + 1, job + 4):                                             # no synchronisation: three more blocks, then the poll
            r.eng.step(j)
        sp.poll([0], job)
        (busy,), _ = sp.read()
        r.eng.sync()
        for j in range(job + 1, job + 4):
            r.rows[j] = r.bank.read_slot(j % ND)
        r.next = job + 4
        assert np.array_equal(idle, busy)
        compare(idle, nb_ref(r.hist(2, job0, job), fft_n, win, fft_n, 3, 0.5)[0], "poll at an older block")
        sp.poll([0], job + 3)                                                         # (and the newest block is there as well)
        compare(sp.read()[0][0], nb_ref(r.hist(2, job0, job + 3), fft_n, win, fft_n, 3, 0.5)[0], "poll at the newest block")
    finally:
        sp.close()


def test_a_tuned_bank_is_analysed_with_its_fine_rotation(pkg):
    r = Run(pkg, "small_complex", "tiled", tuned=True)
    plain = Run(pkg, "small_complex", "tiled")
    try:
        fft_n = 300
        win = kaiser_window(fft_n, 9.0)
        res = []
        for q in (r, plain):
            sp = q.bank.spectrum(fft_n, 1, fft_n, 3)
            sp.attach(0, 2, 0); sp.set_window(0, win); sp.configure(0, fft_n, 3, 0.5)
            job = q.step(blocks_for(q.olen, fft_n, 3))
            sp.poll([0], job)
            res.append(sp.read()[0][0])
            compare(res[-1], nb_ref(q.hist(2, 0, job), fft_n, win, fft_n, 3, 0.5)[0], "tuned" if q is r else "untuned")
        assert np.linalg.norm(res[0] - res[1]) > 1e-2 * np.linalg.norm(res[1])        # 0.37 of a bin moves the tone's skirt
    finally:
        r.close(); plain.close()


# ---- a pin that needs no restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,fft_n,k0", [("tiled", 300, 37), ("any", 60, -11)])
def test_a_bin_centred_tone_through_the_channelizer(pkg, shape, fft_n, k0):
    """chz_bank_write_block's rows would be overwritten by the channel kernel that the append follows, so the tone goes through the
    channelizer: a complex exponential (shift + k0) master bins up lands on bin k0 of an fft_n = P point analysis of the channel
    (L / olen input samples per output sample).  Rectangular window, every bin, one segment: the peak is bin k0 (FFT order, no
    shift) and the bins add up to sum |x|^2 / fft_n of the very samples analysed (Parseval) -- gain and bin order without a
    restatement."""
    L, M, in_type, _ = GEOMETRIES["small_complex"]
    N = L + M - 1
    P, olen = SHAPES[shape]
    assert fft_n == P
    eng = pkg.engine.Engine(L, M, in_type, ring_blocks=RING_BLOCKS)
    try:
        shift, amp = 2000 - k0 % 5, 0.37                                              # (shift + k0) 8 L / N is a whole number
        # the ring repeats every 8 L samples: a frequency of an integer number of cycles per ring is continuous across the wrap
        cycles = (shift + k0) * RING_BLOCKS * L // N
        assert cycles * N == (shift + k0) * RING_BLOCKS * L
        x = (amp * np.exp(2j * np.pi * cycles * np.arange(RING_BLOCKS * L) / (RING_BLOCKS * L))).astype(np.complex64)
        x = np.roll(x, -(M - 1))
        for b in range(RING_BLOCKS):
            eng.write(x[b * L:(b + 1) * L])
        bank = eng.bank(P, olen, 2)
        bank.set_responses(0, np.ones((2, P), np.complex64) / P); bank.set_shifts(0, [shift, shift]); bank.set_active(2)
        sp = bank.spectrum(fft_n, 1, fft_n, 1)
        sp.attach(0, 1, 0); sp.set_window(0, np.ones(fft_n, np.float32)); sp.configure(0, fft_n, 1, 0.0)
        rows = []
        for j in range(8):
            eng.step(j); rows.append(bank.read_slot(j % ND)[1])
        sp.poll([0], 7)
        (bins,), (mm,) = sp.read()
        seg = np.concatenate(rows)[-fft_n:].astype(np.complex128)
        total = np.sum(np.abs(seg) ** 2) / fft_n
        assert total > 0                                                              # the tone came through
        assert int(np.argmax(bins)) == k0 % fft_n
        assert abs(bins.astype(np.float64).sum() / total - 1) <= TOL
        assert mm[1] == bins.max()
    finally:
        eng.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals(run, pkg):
    r = run("small_complex", "tiled")
    Err = pkg.engine.ChzError
    real = r.eng.bank(300, 240, 2, real=True)
    with pytest.raises(Err, match="REAL"):
        real.spectrum(64, 1, 64, 1)
    real.destroy()
    with pytest.raises(Err):
        r.bank.spectrum(4, 1, 4, 1)                                                   # no transform that short
    sp = r.bank.spectrum(64, 2, 64, 3)
    wide = r.eng.welch(648, 1, 16, 1)
    try:
        with pytest.raises(Err, match="channel"):
            sp.attach(0, NCH, r.next)
        with pytest.raises(Err, match="channel"):
            sp.attach(0, -1, r.next)
        sp.attach(0, 0, r.next)
        sp.set_window(0, np.ones(64, np.float32))
        with pytest.raises(Err, match="bin_count"):
            sp.configure(0, 65, 1, 0.0)
        with pytest.raises(Err, match="max_avg"):
            sp.configure(0, 64, 4, 0.0)
        with pytest.raises(Err):
            r.bank.spectrum(64, 1, 66, 1)                                             # more bins than fft_n
        sp.configure(0, 64, 3, 0.5)
        lib = pkg.engine.lib()
        # the wideband calls on a baseband bank, and the reverse
        for rc in (lib.chz_welch_configure(r.eng._h, sp.id, 0, 0, 16, 1, 0.0), lib.chz_welch_poll(r.eng._h, sp.id, 1, None, -1)):
            with pytest.raises(Err, match="wideband"):
                pkg.engine._check(rc)
        for rc in (lib.chz_bank_welch_configure(r.eng._h, wide.id, 0, 16, 1, 0.0), lib.chz_bank_welch_attach(r.eng._h, wide.id, 0, 0, 0),
                   lib.chz_bank_welch_poll(r.eng._h, wide.id, 1, None, 0)):
            with pytest.raises(Err, match="narrowband"):
                pkg.engine._check(rc)
        first = r.next
        with pytest.raises(Err, match="not been issued"):
            sp.poll([0], first)                                                       # nothing executed since the attach
        job = r.step(ND + 2)
        with pytest.raises(Err, match="not attached"):
            sp.poll([1], job)
        sp.poll([0], job - ND)                                                        # the oldest block the rings still answer for
        sp.read()
        with pytest.raises(Err, match="older"):
            sp.poll([0], job - ND - 1)
        with pytest.raises(Err, match="graph"):
            r.eng.run_blocks(r.next, 8, graph=True)                                   # refused, never silently wrong
    finally:
        sp.close(); wide.close()
    r.step(1)
