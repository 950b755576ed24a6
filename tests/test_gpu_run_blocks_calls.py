"""chz_run_blocks call by call: the eager path starts every lane at once and joins them on the host (no device-side fork or join),
issues short calls from the caller alone and long ones from two threads.  None of that may change a bit of what a call leaves
behind: every comparison here is numpy.array_equal against the same blocks issued one chz_step + chz_sync at a time on a fresh
engine with the same input.

Geometries: BASELINE config 3 (129.6 MS/s real, N = 3,240,000) with a small bank, and the N = 32,400 master of the parity tests
(the one the CPU tier runs on the emulated engine, tests/test_run_blocks_calls_emulated.py).  The DC notch is set in both: its
recurrence over blocks is what the hand-over between issuing threads has to keep in block order.
"""
import time

import numpy as np
import pytest

import oracle_lib as ol
from conftest import load_pkg

pytestmark = pytest.mark.gpu

GEOMETRIES = {"small": (25920, 6481, 1.296e6), "config3": (2592000, 648001, 129.6e6)}
NCH = 48
J0 = 5              # first block of a call: not a multiple of the lane count, so the call does not start on lane 0


@pytest.fixture(scope="module")
def pkg():
    p = load_pkg()
    if p.engine.lib().chz_device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests cannot run (there is no CPU fallback)")
    return p


def ring_of(L):
    return (np.random.default_rng(L).standard_normal(8 * L) * 0.1 + 0.05).astype(np.float32)


def make_engine(pkg, geom, demod=False, nch=NCH):
    """A fresh engine with the ring filled once, the DC notch and one bank; with demod=True the bank carries fine tuning, the noise
    estimate and a linear demodulator with S16BE PCM behind every channel (the parameters of bench.py's next_rows leg)."""
    L, M, fs = GEOMETRIES[geom]
    N = L + M - 1
    eng = pkg.engine.Engine(L, M, ol.REAL, ring_blocks=8)
    x = ring_of(L)
    eng.write(x[:8 * L - (M - 1)]); eng.write(x[8 * L - (M - 1):])
    eng.set_notches([0], 0.01)
    P, olen = 300, 240
    bank = eng.bank(P, olen, nch)
    rng = np.random.default_rng(3)
    hz = fs / N
    shifts = np.array([int(round((fs / 130.0 + (i % 1040) * fs / 2200.0 + (i % 40)) / hz)) for i in range(nch)], np.int32)
    if demod:
        kinds = [(50 / 12000, 3000 / 12000), (-200 / 12000, 200 / 12000), (-5000 / 12000, 5000 / 12000)]
        rows = np.stack([pkg.filterapi.design_response(P, olen, N, True, lo, hi, 11.0) for lo, hi in kinds])
        bank.set_responses(0, np.ascontiguousarray(rows[np.arange(nch) % 3]))
        bank.set_tuning(0, 0, shifts, np.full(nch, -3.3 / 12000.0))
        bank.enable_noise(fs)
        bank.set_pcm_stride(2 * olen)
        v = lambda db: 10 ** (db / 20.0)
        one = pkg.engine.DemodParams(channels=1, env=0, agc=1, encoding=pkg.engine.PCM_S16BE, snr_squelch=0, squelch_tail=1, tuned=1, kind=0,
                                     samprate=12000.0, headroom=v(-15.0), threshold=v(-15.0), recovery_rate=v(20.0), hangtime=1.1, dc_alpha=0.0,
                                     bandwidth=2950.0, shift=0.0, squelch_open=10 ** 0.8, squelch_close=10 ** 0.7, gain=v(50.0))
        bank.set_demod(0, 0, [one] * nch, 0.02)
    else:
        bank.set_responses(0, ((rng.standard_normal((nch, P)) + 1j * rng.standard_normal((nch, P))) / P).astype(np.complex64))
        bank.set_shifts(0, shifts)
    bank.set_active(nch)
    return eng, bank


def slots_of(job0, k):
    """(job, slot) of every block of a k-block call that is still held by a slot afterwards."""
    return [(j, j % 4) for j in range(max(job0, job0 + k - 4), job0 + k)]


def snapshot(eng, bank, jobs):
    return {j: (eng.spectrum(s), bank.read_slot(s)) for j, s in jobs}


def stepped(pkg, geom, job0, k, **kw):
    """The reference: the same blocks, one chz_step + chz_sync at a time, on a fresh engine."""
    eng, bank = make_engine(pkg, geom, **kw)
    try:
        for j in range(job0, job0 + k):
            eng.step(j); eng.sync()
        return snapshot(eng, bank, slots_of(job0, k)), (bank.read_pcm((job0 + k - 1) % 4) if kw.get("demod") else None)
    finally:
        eng.close()


def assert_same(got, want, what):
    assert got.keys() == want.keys()
    for j in got:
        assert np.array_equal(got[j][0], want[j][0]), "%s: spectrum of block %d differs" % (what, j)
        assert np.array_equal(got[j][1], want[j][1]), "%s: channel outputs of block %d differ" % (what, j)


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 8, 9, 20])
@pytest.mark.parametrize("geom", ["small", "config3"])
def test_one_call_equals_the_blocks_stepped_one_at_a_time(pkg, geom, k):
    """K = 1 .. 5 stay with the caller and leave lanes unused (1 .. 3); 8, 9 and 20 are split over the issuing threads once those
    are up -- the second call of an engine is, the first one (which starts them) usually is not: both are checked."""
    want, _ = stepped(pkg, geom, J0, k)
    eng, bank = make_engine(pkg, geom)
    try:
        t = eng.run_blocks(J0, k)
        assert t.blocks == k
        assert_same(snapshot(eng, bank, slots_of(J0, k)), want, "first call, K=%d" % k)
        eng.check()
    finally:
        eng.close()
    # the same call as an engine's SECOND long call: the issuing threads exist by then
    want2, _ = stepped(pkg, geom, J0, 8 + k)
    eng, bank = make_engine(pkg, geom)
    try:
        eng.run_blocks(J0, 8)
        time.sleep(0.05)                       # (the issuing thread sleeps by now: the hand-over has to wake it)
        eng.run_blocks(J0 + 8, k)
        assert_same(snapshot(eng, bank, slots_of(J0 + 8, k)), {j: want2[j] for j, _ in slots_of(J0 + 8, k)}, "second call, K=%d" % k)
        eng.check()
    finally:
        eng.close()


@pytest.mark.parametrize("geom", ["small", "config3"])
def test_fifty_one_block_calls_then_a_long_one(pkg, geom):
    """The entry path with nothing to wait for, fifty times over, then twenty blocks in one call: the last block as stepped."""
    n1, k = 50, 20
    want, _ = stepped(pkg, geom, J0, n1 + k)
    eng, bank = make_engine(pkg, geom)
    try:
        for j in range(J0, J0 + n1):
            assert eng.run_blocks(j, 1).blocks == 1
        eng.run_blocks(J0 + n1, k)
        last = J0 + n1 + k - 1
        got = snapshot(eng, bank, [(last, last % 4)])
        assert_same(got, {last: want[last]}, "50 x 1 + 20")
        eng.check()
    finally:
        eng.close()


@pytest.mark.parametrize("k", [1, 9])
@pytest.mark.parametrize("geom", ["small", "config3"])
def test_demodulated_bank_keeps_the_wait_for_its_stream(pkg, geom, k):
    """A demodulator behind every channel (its kernels run on a stream of their own, in block order): the call returns after the
    last block's demodulator, and the PCM of that block is what the stepped run packs."""
    nch = 300
    want, want_pcm = stepped(pkg, geom, J0, 4 + k, demod=True, nch=nch)
    eng, bank = make_engine(pkg, geom, demod=True, nch=nch)
    try:
        eng.run_blocks(J0, 4)
        t = eng.run_blocks(J0 + 4, k)
        assert t.blocks == k and t.total_ms > 0
        last = J0 + 4 + k - 1
        pcm, st = bank.read_pcm(last % 4)
        assert np.array_equal(pcm, want_pcm[0])
        assert [s.frame for s in st] == [s.frame for s in want_pcm[1]]
        assert_same(snapshot(eng, bank, [(last, last % 4)]), {last: want[last]}, "demodulated, K=%d" % k)
        eng.check()
    finally:
        eng.close()


@pytest.mark.parametrize("demod", [False, True])
@pytest.mark.parametrize("k", [1, 3, 4, 20])
@pytest.mark.parametrize("geom", ["small", "config3"])
def test_timing_of_a_call(pkg, geom, k, demod):
    """timing.total_ms is the device's time from the first kernel's start to the last kernel's end of THIS call: positive, and
    never more than the host saw pass around the call."""
    eng, bank = make_engine(pkg, geom, demod=demod, nch=300 if demod else NCH)
    try:
        eng.run_blocks(J0, 8)
        for rep in range(3):
            job = J0 + 8 + rep * k
            h0 = time.perf_counter()
            t = eng.run_blocks(job, k)
            wall_ms = (time.perf_counter() - h0) * 1e3
            print("geom %s K=%d demod=%d: total_ms %.4f enqueue_ms %.4f wall_ms %.4f" % (geom, k, demod, t.total_ms, t.enqueue_ms, wall_ms))
            assert t.blocks == k
            assert 0 < t.total_ms <= wall_ms
            assert 0 < t.enqueue_ms <= wall_ms
    finally:
        eng.close()
