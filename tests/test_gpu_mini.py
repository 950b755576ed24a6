"""Pools of small COMPLEX inline masters (chz_mini_*, kernel mini_ovs) away from radiod's own lengths, against the float64 oracle.

The pool is meant to take any length 8 <= N <= 8192 without a prime factor above 13 that the reference's FFTW would plan.  Every size
here runs ONE chz_mini_execute of 12 requests against a pool of capacity 5: three launches (5 + 5 + 2), instances listed twice inside
one launch and across launches, a bin shift per request -- zero, +-1, both Nyquist seams, a quarter and a third of the circle, more than
a whole turn -- and ISB on four of them.  An odd N = 2h + 1 is where the ISB unpack can go wrong: the reference loops p < s_bins/2
(src/filter.c:899) and leaves the pair (h, h + 1) as gathered.  The sizes walk the radices (2, 3, 4, 5, 7, 11, 13), the smallest
lengths, and both sides of the 64 KB of LDS a kernel gets without asking (two N-point buffers: N = 4096 is the last size within).

Expected: ol.channel() on numpy's float64 transform of the very window the request carried, per-channel bounds of
tests/test_gpu_parity.py (check_channel, floor 0: white noise).  Where the expected row is all zero -- a shift that moves the whole
slave outside the master, or a negative shift on an odd master, where the reference's gather ends after one bin -- the device's row
must be exactly zero (check_channel asserts that)."""
import numpy as np
import pytest

import oracle_lib as ol
from conftest import load_pkg
from test_gpu_parity import check_channel

pytestmark = pytest.mark.gpu

CAP = 5
REQ = [0, 1, 2, 3, 4, 2, 0, 4, 4, 1, 3, 3]
ISB = [r in (1, 4, 7, 10) for r in range(len(REQ))]
SIZES = [(5, 4), (6, 4), (20, 13), (99, 27), (135, 109), (140, 106), (572, 430), (1001, 1002), (2048, 2049), (2100, 2101), (3281, 3281)]


def shift_list(N):
    return [0, 1, -1, N // 2 - 1, -(N // 2), N // 4, -(N // 3), N // 2, N, -N - 3, 3, 7]


@pytest.fixture(scope="module")
def pkg():
    p = load_pkg()
    if p.engine.lib().chz_device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests cannot run (there is no CPU fallback)")
    ol.build()
    return p


def cnoise(rng, *shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)


def filled_pool(pkg, L, M, rng):
    pool = pkg.engine.MiniPool(L, M, CAP)
    insts = [pool.add() for _ in range(CAP)]
    assert sorted(insts) == list(range(CAP))
    resp = cnoise(rng, CAP, L + M - 1)
    for i in insts:
        pool.set_response(i, resp[i])
    return pool, insts, resp


@pytest.mark.parametrize("L,M", SIZES, ids=["N%d" % (L + M - 1) for L, M in SIZES])
def test_twelve_requests_in_three_launches_match_the_oracle(pkg, L, M):
    N = L + M - 1
    rng = np.random.default_rng(1000 * L + M)
    pool, insts, resp = filled_pool(pkg, L, M, rng)
    try:
        shifts = shift_list(N)
        win = cnoise(rng, len(REQ), N)                               # a random history in front of the L new samples
        got = pool.execute([insts[i] for i in REQ], win, np.array(shifts, np.int32), np.array(ISB, np.uint8))
        spec = np.fft.fft(win.astype(np.complex128), axis=1)
        want = [ol.channel(spec[r], ol.COMPLEX, N, L, shifts[r], resp[REQ[r]], isb=ISB[r]) for r in range(len(REQ))]
        live = [bool(w.any()) for w in want]
        assert sum(live) >= 9 and all(live[r] for r in range(len(REQ)) if ISB[r]), live
        worst = 0.0
        for r in range(len(REQ)):
            e = check_channel(got[r], want[r])
            print("N %d request %2d inst %d shift %6d isb %d: rel-L2 %.3g%s" % (N, r, REQ[r], shifts[r], ISB[r], e, "" if live[r] else "  (all zero)"))
            worst = max(worst, e)
        print("N %d: worst rel-L2 %.3g, %.3g of the bound" % (N, worst, worst / 1e-5))
    finally:
        pool.close()


@pytest.mark.parametrize("L,M", [(6, 4), (135, 109), (2100, 2101)], ids=["N9", "N243", "N4200"])
def test_second_block_carries_the_history(pkg, L, M):
    """Two blocks of a stream per instance, the window of the second holding the last M - 1 samples of the first, against the oracle's
    own overlap-save master (ol.Stream) fed the same blocks."""
    N = L + M - 1
    rng = np.random.default_rng(N)
    pool, insts, resp = filled_pool(pkg, L, M, rng)
    try:
        streams = [ol.Stream(L, M, ol.COMPLEX) for _ in insts]
        win = np.zeros((CAP, N), np.complex64)
        shifts = np.array([0, 1, 3, 0, N // 4], np.int32)
        isb = np.array([0, 1, 0, 1, 1], np.uint8)
        for blk in range(2):
            x = cnoise(rng, CAP, L)
            win = np.concatenate([win[:, L:], x], axis=1)
            got = pool.execute(insts, win, shifts, isb)
            for i in range(CAP):
                spec = streams[i].push(x[i], f64=True)
                want = ol.channel(spec, ol.COMPLEX, N, L, int(shifts[i]), resp[i], isb=bool(isb[i]))
                assert want.any()
                check_channel(got[i], want)
    finally:
        pool.close()


def test_release_and_add_give_the_index_back(pkg):
    L, M = 6, 4
    rng = np.random.default_rng(3)
    pool, insts, resp = filled_pool(pkg, L, M, rng)
    try:
        with pytest.raises(pkg.engine.ChzError) as e:
            pool.add()
        assert "full" in str(e.value)
        pool.release(insts[3])
        with pytest.raises(pkg.engine.ChzError) as e:
            pool.release(insts[3])
        assert "not in use" in str(e.value)
        assert pool.add() == insts[3]
        new = cnoise(rng, L + M - 1)
        pool.set_response(insts[3], new)                             # the row is the instance's again
        win = cnoise(rng, 1, L + M - 1)
        got = pool.execute([insts[3]], win, isb=[1])
        check_channel(got[0], ol.channel(np.fft.fft(win[0].astype(np.complex128)), ol.COMPLEX, L + M - 1, L, 0, new, isb=True))
    finally:
        pool.close()


def test_refusals(pkg):
    with pytest.raises(pkg.engine.ChzError) as e:
        pkg.engine.MiniPool(2049, 2049, 4)                           # N = 4097 = 17 * 241
    assert "above 13" in str(e.value)
    with pytest.raises(pkg.engine.ChzError) as e:
        pkg.engine.MiniPool(4, 4, 4)                                 # N = 7
    assert "8 <= N" in str(e.value)
    pool = pkg.engine.MiniPool(6, 4, 2)
    try:
        a, b = pool.add(), pool.add()
        with pytest.raises(pkg.engine.ChzError) as e:
            pool.add()
        assert "full" in str(e.value)
        win = np.ones((2, 9), np.complex64)
        for bad in (2, -1):
            with pytest.raises(pkg.engine.ChzError) as e:
                pool.execute([a, bad], win)
            assert "bad request 1" in str(e.value)
        with pytest.raises(pkg.engine.ChzError):
            pool.release(2)
        pool.execute([a, b], win)
    finally:
        pool.close()
