"""sig_gen's carrier and noise generated on the device straight into the input ring (chz_input_generate, kernel siggen_fill) -- against
oracle_lib.SigGen (chzo_siggen_*), the restatement of the reference's loop that tests/test_oracle_vs_reference.py pins to the reference's own.

Golden geometry (L 11520, M 2881; REAL and COMPLEX) on the smallest ring the engine makes (3 blocks), as tests/test_gpu_raw_input.py sets
it up.  After every call the float ring itself is read back and compared with a numpy model of it; regions never written stay zero.
  noise only, and a carrier that stands still: float bits EQUAL (the law is integer up to two exact double products)
  a turning carrier: |dev - ref| <= max(spacing(|ref|), amplitude scale 1e-9) per float -- the reference's recurrence wanders at most 8.5e-11
    from the closed form within 2^18 samples at these frequencies -- and, for the frequencies that do not land on ties, at most 2e-3 of a
    2^18-sample run may differ at all (the closed form itself measured 4.1e-4, 3.0e-4, 2.0e-4)
  continuity, seek / tell, the energy sums and their tickets, one block through the transform and a bank of channels, every refusal.
The checker hands out floats only: the energies' double sums, and the stream 2^40 samples in, come from tests/siggen_oracle.py's restatement
of the Gaussian, which tests/test_siggen_host.py pins to the checker and which is compared with it again where it is used here.
tests/test_siggen_emulated.py runs this file on the CPU build."""
import numpy as np
import pytest

import oracle_lib as ol
import siggen_oracle as so
from conftest import load_pkg
from test_gpu_raw_input import L, M, RING_BLOCKS, same_bits
from test_gpu_raw_input import read_ring as read_ring_now

pytestmark = pytest.mark.gpu

R = 64                                 # CHZ_SIGGEN_RUN (asserted below)
SIZES = (1, 3, 7, 8, 9, 63, 64, 65, 511, 512, 513, R - 1, R, R + 1, 64 * R - 1, 64 * R, 64 * R + 1, L)
ROUNDS = 3
AMPLITUDE, NOISE = 0.1, 0.01
LONG = 1 << 18
TYPES = pytest.mark.parametrize("isreal", [True, False], ids=["real", "complex"])


def read_ring(eng):
    """the float ring once everything issued has run (a generate is asynchronous, and the read-back does not wait for the engine's streams)"""
    eng.sync()
    return read_ring_now(eng)


def in_type(isreal):
    return ol.REAL if isreal else ol.COMPLEX


def engine(pkg, isreal):
    return pkg.engine.Engine(L, M, in_type(isreal), ring_blocks=RING_BLOCKS)


class Model:
    """what the float ring must hold"""

    def __init__(self, isreal):
        self.per = 1 if isreal else 2
        self.ring = np.zeros(RING_BLOCKS * L * self.per, np.float32)
        self.wpos = (M - 1) * self.per
        self.offsets, self.straddles = set(), 0

    def write(self, samples, generated=True):
        floats = np.ascontiguousarray(samples).view(np.float32).reshape(-1)
        if generated and floats.size:
            self.offsets.add(self.wpos % 4)
            self.straddles += self.wpos + floats.size > self.ring.size
        idx = (self.wpos + np.arange(floats.size)) % self.ring.size
        self.ring[idx] = floats
        self.wpos = int((self.wpos + floats.size) % self.ring.size)

    def last(self, n):
        """the n samples written last, as floats"""
        return self.ring[(self.wpos - n * self.per + np.arange(n * self.per)) % self.ring.size]


def differing(ring, model):
    return np.flatnonzero(ring.view(np.uint32) != model.ring.view(np.uint32))[:8]


def test_the_binding_s_run_length_is_the_header_s():
    assert load_pkg().engine.SIGGEN_RUN == R


@TYPES
def test_noise_only_streams_equal_the_checker_s_bit_for_bit(isreal):
    """three rounds of the size list, each begun one size further on (the start offsets pass through all residues mod 4, the third block
    wraps), a one-sample chz_input_write in front of every third call"""
    pkg = load_pkg()
    ops = [n for rnd in range(ROUNDS) for n in SIZES[rnd:] + SIZES[:rnd]]
    ref = so.reference_stream(0.3, 0.0, NOISE, isreal, sum(ops))
    filler = (np.arange(1, len(ops) + 1) * 1e-3).astype(np.float32)
    eng = engine(pkg, isreal)
    try:
        eng.siggen(0.3, 0.0, NOISE, so.SCALE[isreal])
        model, used = Model(isreal), 0
        assert eng.ring()[1] == model.ring.size
        for k, n in enumerate(ops):
            if k % 3 == 0:
                x = filler[k:k + 1] if isreal else (filler[k:k + 1] * (1 + 2j)).astype(np.complex64)
                eng.write(x)
                model.write(x, generated=False)
            assert eng.generate(n) == k
            model.write(ref[used:used + n])
            used += n
            ring = read_ring(eng)
            assert same_bits(ring, model.ring), (k, n, differing(ring, model))
            assert eng.siggen_tell() == used
        assert model.straddles >= 2, "no generate straddled the ring end"
        assert model.offsets == ({0, 1, 2, 3} if isreal else {0, 2}), model.offsets
    finally:
        eng.close()


@TYPES
def test_a_carrier_that_stands_still_with_noise_equals_the_checker_s_bits(isreal):
    """freq 0: the step phasor is exactly 1"""
    pkg = load_pkg()
    ops = SIZES[3:] + SIZES[:3]
    ref = so.reference_stream(0.0, AMPLITUDE, NOISE, isreal, sum(ops))
    eng = engine(pkg, isreal)
    try:
        eng.siggen(0.0, AMPLITUDE, NOISE, so.SCALE[isreal])
        model, used = Model(isreal), 0
        for k, n in enumerate(ops):
            eng.generate(n)
            model.write(ref[used:used + n])
            used += n
            ring = read_ring(eng)
            assert same_bits(ring, model.ring), (k, n, differing(ring, model))
    finally:
        eng.close()


def within_tolerance(dev, ref, isreal):
    """per float: |dev - ref| <= max(spacing(|ref|), amplitude scale 1e-9); returns the worst excess ratio"""
    d = np.abs(dev.astype(np.float64) - ref.astype(np.float64))
    bound = np.maximum(np.spacing(np.abs(ref)).astype(np.float64), AMPLITUDE * so.SCALE[isreal] * 1e-9)
    return float((d / bound).max())


@TYPES
@pytest.mark.parametrize("noise", [NOISE, 0.0], ids=["noise", "clean"])
@pytest.mark.parametrize("fi", range(len(so.FREQS)), ids=["f%d" % i for i in range(len(so.FREQS))])
def test_a_turning_carrier_stays_within_the_reference_s_own_wander(fi, noise, isreal):
    """the first 2 L + 4097 samples in three generates whose ends are no multiples of the run length, the ring checked after each"""
    pkg = load_pkg()
    freq = so.FREQS[fi]
    ops = (4097, L, L)
    ref = so.reference_stream(freq, AMPLITUDE, noise, isreal, LONG)
    eng = engine(pkg, isreal)
    try:
        eng.siggen(freq, AMPLITUDE, noise, so.SCALE[isreal])
        model, used = Model(isreal), 0
        for n in ops:
            eng.generate(n)
            model.write(ref[used:used + n])
            used += n
            ring = read_ring(eng)
            worst = within_tolerance(ring, model.ring, isreal)
            print("freq %r noise %g %s: after %d samples the worst |dev - ref| is %.3f of its bound" % (freq, noise, "REAL" if isreal else "COMPLEX", used, worst))
            assert worst <= 1.0, (freq, noise, used, worst)
            model.ring[:] = ring                    # what the device wrote stays; the next call is judged on its own samples (and on leaving these alone)
    finally:
        eng.close()


@TYPES
@pytest.mark.parametrize("noise", [NOISE, 0.0], ids=["noise", "clean"])
@pytest.mark.parametrize("fi", so.IRRATIONAL, ids=["f%d" % i for i in so.IRRATIONAL])
def test_few_samples_of_a_long_run_differ_from_the_reference_at_all(fi, noise, isreal):
    """2^18 samples from the start, a ring's worth a call: the tolerance on every float, and at most 2e-3 of the samples not bit-equal.
    A COMPLEX sample counts if either part differs.  Measured on the MI355X (noise / clean): REAL 133 / 104, 164 / 74, 1 / 52 samples,
    COMPLEX 192 / 187, 340 / 516, 6 / 104 (the CPU build: 117 / 107, 171 / 78, 1 / 52 and 200 / 178, 335 / 516, 6 / 104) -- 516 of 262144 is
    1.97e-3, and it is the reference's own wander: the closed form evaluated in extended precision differs from the reference in 516
    samples of that stream too (178 and 104 of the other two; 107, 78, 52 REAL)."""
    pkg = load_pkg()
    freq = so.FREQS[fi]
    ref = so.reference_stream(freq, AMPLITUDE, noise, isreal, LONG)
    per = 1 if isreal else 2
    eng = engine(pkg, isreal)
    try:
        eng.siggen(freq, AMPLITUDE, noise, so.SCALE[isreal])
        model, used, differ, worst = Model(isreal), 0, 0, 0.0
        while used < LONG:
            n = min(RING_BLOCKS * L, LONG - used)
            eng.generate(n)
            model.write(ref[used:used + n])
            used += n
            ring = read_ring(eng)
            got, want = model_last(ring, model, n), model.last(n)
            worst = max(worst, within_tolerance(got, want, isreal))
            neq = got.view(np.uint32) != want.view(np.uint32)
            differ += int((neq.reshape(-1, per).any(axis=1)).sum())
        assert eng.siggen_tell() == LONG
        print("freq %r noise %g %s: %d of %d samples differ (%.2e), worst |dev - ref| %.3f of its bound" % (freq, noise, "REAL" if isreal else "COMPLEX", differ, LONG, differ / LONG, worst))
        assert worst <= 1.0, (freq, noise, worst)
        assert differ <= 2e-3 * LONG, (freq, noise, differ)
    finally:
        eng.close()


def model_last(ring, model, n):
    return ring[(model.wpos - n * model.per + np.arange(n * model.per)) % ring.size]


@TYPES
def test_two_generates_leave_what_one_generate_of_their_sum_leaves(isreal):
    """generate(a); generate(b) against generate(a + b) on a twin, a and b neighbours in the size list; a carrier that stands still plus noise,
    where every sample is exact whatever run of the kernel it falls into"""
    pkg = load_pkg()
    ea, eb = engine(pkg, isreal), engine(pkg, isreal)
    try:
        for e in (ea, eb):
            e.siggen(0.0, AMPLITUDE, NOISE, so.SCALE[isreal])
        sizes = SIZES + SIZES[:1]
        for a, b in zip(sizes[:-1], sizes[1:]):
            ea.generate(a); ea.generate(b)
            eb.generate(a + b)
            ra, rb = read_ring(ea), read_ring(eb)
            assert same_bits(ra, rb), (a, b, np.flatnonzero(ra.view(np.uint32) != rb.view(np.uint32))[:8])
            assert ea.siggen_tell() == eb.siggen_tell()
    finally:
        ea.close(); eb.close()


@TYPES
def test_seek_gives_the_samples_a_twin_reaches_without_seeking(isreal):
    """carrier and noise; the twin generates the k samples in front in one call, so both engines make the range in the same launch"""
    pkg = load_pkg()
    m = 64 * R + 1
    freq = so.FREQS[0]
    for k in (0, 1, R - 1, R, 64 * R + 5, 3 * L - 7):
        es, et = engine(pkg, isreal), engine(pkg, isreal)
        try:
            for e in (es, et):
                e.siggen(freq, AMPLITUDE, NOISE, so.SCALE[isreal])
            es.generate(5)                               # somewhere else first
            es.siggen_seek(k)
            assert es.siggen_tell() == k
            es.generate(m)
            et.generate(k); et.generate(m)
            ms, mt = Model(isreal), Model(isreal)
            ms.write(np.zeros(5 + m, np.float32 if isreal else np.complex64))
            mt.write(np.zeros(k + m, np.float32 if isreal else np.complex64))
            assert same_bits(model_last(read_ring(es), ms, m), model_last(read_ring(et), mt, m)), k
            assert es.siggen_tell() == et.siggen_tell() == k + m
        finally:
            es.close(); et.close()


@TYPES
def test_seek_0_after_three_blocks_repeats_block_0(isreal):
    pkg = load_pkg()
    eng = engine(pkg, isreal)
    try:
        eng.siggen(so.FREQS[0], AMPLITUDE, NOISE, so.SCALE[isreal])
        eng.generate(L)
        block0 = read_ring(eng)
        eng.generate(L); eng.generate(L)
        assert not same_bits(read_ring(eng), block0)
        eng.siggen_seek(0)
        eng.generate(L)                                  # the ring is three blocks long: block 3 lies where block 0 lay
        ring = read_ring(eng)
        per = 1 if isreal else 2
        where = ((M - 1) * per + np.arange(L * per)) % ring.size
        assert same_bits(ring[where], block0[where])
        assert np.abs(block0[where]).max() > 0
    finally:
        eng.close()


@TYPES
def test_seek_far_into_the_stream_gives_the_restated_gaussian_from_the_jumped_state(isreal):
    pkg = load_pkg()
    E = pkg.engine
    k, m, per = (1 << 40) + 12345, 64 * R + 1, 1 if isreal else 2
    eng = engine(pkg, isreal)
    try:
        eng.siggen(0.3, 0.0, NOISE, so.SCALE[isreal])
        eng.siggen_seek(k)
        assert eng.siggen_tell() == k
        eng.generate(m)
        assert eng.siggen_tell() == k + m
        state = E.siggen_jump(E.siggen_seed(1), k * per)
        g = so.gauss(so.draws(state, m * per)[0])
        want = ((0.0 * 1.0 + NOISE * g) * so.SCALE[isreal]).astype(np.float32)
        model = Model(isreal)
        model.write(want)
        ring = read_ring(eng)
        assert same_bits(ring, model.ring), differing(ring, model)
    finally:
        eng.close()


@TYPES
def test_the_energy_sums_are_the_sequential_double_sums_to_the_reordering_bound(isreal):
    """n in {1, 65, L} one after the other; a carrier that stands still plus noise, whose samp the restatement gives in double (and whose floats
    are the checker's); eight tickets stay readable, the ninth-oldest is refused; a second engine gives the same bits"""
    pkg = load_pkg()
    E = pkg.engine
    per = 1 if isreal else 2
    sizes = (1, 65, L)
    ref = so.reference_stream(0.0, AMPLITUDE, NOISE, isreal, sum(SIZES[3:] + SIZES[:3]))
    runs = []
    for _ in range(2):
        eng = engine(pkg, isreal)
        try:
            eng.siggen(0.0, AMPLITUDE, NOISE, so.SCALE[isreal])
            got, pos = [], 0
            for t, n in enumerate(sizes):
                assert eng.generate(n) == t
                samp = so.samples_f0(E.siggen_jump(E.siggen_seed(1), pos * per), n, AMPLITUDE, NOISE, isreal)
                assert same_bits(so.to_ring(samp, so.SCALE[isreal]), ref[pos:pos + n])       # the restatement is the checker here
                want = so.energy(samp)
                en = eng.generate_energy(t)
                print("n %d %s: energy %r, sequential sum %r, relative difference %.3g (bound %.3g)" % (n, "REAL" if isreal else "COMPLEX", en, want, abs(en - want) / want, 2 * n * 2.0 ** -53))
                assert abs(en - want) <= 2 * n * 2.0 ** -53 * want, (n, en, want)
                got.append(en)
                pos += n
            with pytest.raises(E.ChzError):
                eng.generate_energy(len(sizes))                                              # not yet issued
            for t in range(len(sizes), 9):
                assert eng.generate(0 if t == 5 else 3) == t
            assert eng.generate_energy(5) == 0.0                                             # an empty generate has a ticket and no energy
            assert eng.generate_energy(1) == got[1] and eng.generate_energy(8) > 0
            with pytest.raises(E.ChzError, match="are gone"):
                eng.generate_energy(0)
            runs.append(got)
        finally:
            eng.close()
    assert runs[0] == runs[1]


@TYPES
def test_a_generated_block_goes_through_the_transform_as_the_checker_s_floats_do(isreal):
    pkg = load_pkg()
    ref = so.reference_stream(0.3, 0.0, NOISE, isreal, sum(SIZES) * ROUNDS)
    eg, ew = engine(pkg, isreal), engine(pkg, isreal)
    try:
        eg.siggen(0.3, 0.0, NOISE, so.SCALE[isreal])
        eg.generate(L)
        ew.write(ref[:L])
        eg.forward(0); ew.forward(0)
        sg, sw = eg.spectrum(0), ew.spectrum(0)
        assert same_bits(sg, sw) and np.abs(sg).max() > 0
        # one bank of four 12 kHz channels (20 ms blocks: 240 samples out, 300-point slaves)
        P, olen, outs = 300, 240, []
        resp = ol.set_filter(P, olen, L + M - 1, isreal, -5000.0 / 12000, 5000.0 / 12000, 11.0)
        for e in (eg, ew):
            bank = pkg.engine.Bank(e, P, olen, 4)
            bank.set_responses(0, np.stack([resp] * 4))
            bank.set_shifts(0, [250, 1000, 2500 if isreal else -2500, 6000 if isreal else -1000])
            bank.set_active(4)
            bank.execute(0)
            outs.append(bank.read())
        assert same_bits(outs[0], outs[1]) and np.abs(outs[0]).max() > 0
    finally:
        eg.close(); ew.close()


@TYPES
def test_refusals_enqueue_nothing_and_advance_nothing(isreal):
    pkg = load_pkg()
    E = pkg.engine
    scale = so.SCALE[isreal]
    eng = engine(pkg, isreal)
    try:
        zero = read_ring(eng)
        for call in (lambda: eng.generate(8), lambda: eng.siggen_seek(0), eng.siggen_tell):
            with pytest.raises(E.ChzError, match="no stream"):
                call()
        bad = float("nan"), float("inf"), -float("inf")
        for v in bad:
            for i in range(4):
                args = [0.1, AMPLITUDE, NOISE, scale]
                args[i] = v
                p = E.SigGenParams(*args, 1)
                assert E.lib().chz_siggen_check(in_type(isreal), p) < 0 and "finite" in E.lib().chz_last_error().decode()
                with pytest.raises(E.ChzError, match="finite"):
                    eng.siggen(*args)
        assert E.lib().chz_siggen_check(in_type(isreal), E.SigGenParams(0.1, AMPLITUDE, NOISE, scale, 1)) == 0
        assert E.lib().chz_siggen_check(7, E.SigGenParams(0.1, AMPLITUDE, NOISE, scale, 1)) < 0
        with pytest.raises(E.ChzError, match="no stream"):
            eng.generate(8)                              # a refused description describes nothing
        assert same_bits(read_ring(eng), zero)
        eng.siggen(0.0, AMPLITUDE, NOISE, scale)
        eng.generate(100)
        ring = read_ring(eng)
        for n, says in ((-1, "samples"), (RING_BLOCKS * L + 1, "does not fit")):
            with pytest.raises(E.ChzError, match=says):
                eng.generate(n)
            assert eng.siggen_tell() == 100 and same_bits(read_ring(eng), ring)
        with pytest.raises(E.ChzError, match="finite"):
            eng.siggen(0.0, float("nan"), NOISE, scale)  # refused: the running stream stays as it is
        assert eng.siggen_tell() == 100
        with pytest.raises(E.ChzError, match="2\\^53"):
            eng.siggen_seek((1 << 53) + 1)
        assert eng.siggen_tell() == 100
        eng.siggen_seek((1 << 53) - 5)
        with pytest.raises(E.ChzError, match="2\\^53"):
            eng.generate(6)
        assert eng.siggen_tell() == (1 << 53) - 5 and same_bits(read_ring(eng), ring)
        t = eng.generate(5)                              # up to the last sample is fine, and took the next ticket: refusals took none
        assert t == 1 and eng.siggen_tell() == 1 << 53
        assert eng.generate(0) == 2
        with pytest.raises(E.ChzError, match="2\\^53"):
            eng.generate(1)
        # the write position moved by 105 samples in all: a float write lands behind them
        model = Model(isreal)
        model.write(np.zeros(105, np.float32 if isreal else np.complex64))
        one = np.ones(1, np.float32 if isreal else np.complex64)
        eng.write(one)
        model.write(one)
        after = read_ring(eng)
        assert model_last(after, model, 1)[0] == 1.0
    finally:
        eng.close()
    if isreal:
        e16 = engine(pkg, True)
        try:
            x16 = np.arange(L, dtype=np.int16)
            e16.write_i16(x16, 1e-4)
            with pytest.raises(E.ChzError, match="cannot be mixed"):
                e16.siggen(0.0, AMPLITUDE, NOISE, scale)
            with pytest.raises(E.ChzError):
                e16.generate(8)
        finally:
            e16.close()
        eg = engine(pkg, True)
        try:
            eg.siggen(0.0, AMPLITUDE, NOISE, scale)
            eg.generate(8)
            with pytest.raises(E.ChzError, match="cannot be mixed"):
                eg.write_i16(np.arange(8, dtype=np.int16), 1e-4)      # and the other way round
            assert eg.generate(8) == 1
        finally:
            eg.close()
