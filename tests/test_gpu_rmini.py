"""Pools of small REAL inline masters with decimating slaves (chz_rmini_*, kernel rmini_ovs) against the float64 oracle and,
where it is built, the reference's own filter.c.

Every geometry runs three blocks of 37 instances (plus one instance listed a second time with other shifts) in ONE
chz_rmini_execute call per block: 38 requests against a pool of capacity 37 (two launches), and again against a pool of
capacity 16 (three), which must give the same bits.  Each instance has its own
input stream and its window carries the M-1 samples of the block before.  COMPLEX slaves are compared with
ol.channel() on the float64 spectrum of ol.Stream; the float64 oracle has no REAL-output channel, so a REAL slave's answer is
the same rule (src/filter.c:803-809,911: bin si reads master bin si + shift, zero outside the master, the Nyquist bin zeroed)
applied to that float64 spectrum in numpy, followed by numpy's float64 c2r.  Bounds: check_channel and the constants of
tests/test_gpu_parity.py, floor 0 for white noise; the one case with a strong line uses noise_floor().
"""
import numpy as np
import pytest

import oracle_lib as ol
from conftest import load_pkg
from test_gpu_parity import check_channel, noise_floor

pytestmark = pytest.mark.gpu

C, R = ol.COMPLEX, ol.REAL
NINST, CAP, NBLOCKS = 37, 16, 3
NREF = 5            # instances also run through the reference's filter.c (each is a master with all its slaves there)

GEOMS = {
    "smallest": (8, 9, [(8, C), (4, C), (4, R)]),
    "radix5": (300, 101, [(75, C), (75, R)]),                    # M != L + 1
    "radix357": (1050, 1051, [(150, C)]),
    "packetd": (960, 961, [(960, C)]),                           # P = N
    "stereod": (1920, 1921, [(240, R), (240, C), (240, C)]),
    "wfm": (7680, 7681, [(960, R), (960, C), (960, C)]),         # LDS beyond 64 KB
    "oddP": (8, 19, [(4, C)]),                                   # N = 26, P = 13: ISB on an odd P leaves the innermost pair alone (src/filter.c:899)
}
FILTERS = {C: [(-0.3, 0.3, 5.0), (-0.45, 0.1, 3.0), (0.05, 0.4, 8.0)], R: [(0.02, 0.4, 5.0), (0.0, 0.25, 3.0), (0.1, 0.45, 8.0)]}


@pytest.fixture(scope="module")
def pkg():
    p = load_pkg()
    if p.engine.lib().chz_device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests cannot run (there is no CPU fallback)")
    ol.build()
    return p


def real_channel_f64(spec, P, olen, shift, resp):
    sb = P // 2 + 1
    mi = np.arange(sb) + shift
    ok = (mi >= 0) & (mi < spec.shape[0])
    fd = np.zeros(sb, np.complex128)
    fd[ok] = spec[mi[ok]] * resp[:sb][ok].astype(np.complex128)
    fd[(sb + 1) // 2] = 0
    return (np.fft.irfft(fd, P) * P)[P - olen:]


def want_f64(spec, P, olen, typ, shift, resp, isb):
    if typ == R:
        return real_channel_f64(spec, P, olen, shift, resp)
    return ol.channel(spec, ol.REAL, P, olen, shift, resp, isb=isb)


def shift_menu(bins, P):
    """0, +-multiples of 4, one that is no multiple of the overlap factor, and two that push part of the passband outside the master."""
    big = 4 * max(1, bins // 8)
    return [0, 4, -4, big, -big, 3, bins - P // 4, -(bins - P // 4), 4 * max(1, bins // 16)]


def responses(L, M, slaves):
    N = L + M - 1
    out = []
    for olen, typ in slaves:
        P = N * olen // L
        out.append([ol.set_filter(P, olen, N, True, lo, hi, beta, typ) for lo, hi, beta in FILTERS[typ]])
    return out


def rsel(i):
    return (i % CAP) % 3


@pytest.mark.parametrize("name", list(GEOMS))
def test_pooled_real_masters_match_the_oracle(pkg, name):
    L, M, slaves = GEOMS[name]
    N, ns, bins = L + M - 1, len(slaves), (L + M - 1) // 2 + 1
    rng = np.random.default_rng(L + 7 * M)
    resp = responses(L, M, slaves)
    pool = pkg.engine.RealMiniPool(L, M, slaves, NINST)
    assert pool.capacity == NINST
    small = pkg.engine.RealMiniPool(L, M, slaves, CAP)           # n = 38 requests: two chunks in `pool`, three in this one
    try:
        insts = [pool.add() for _ in range(NINST)]
        assert sorted(insts) == list(range(NINST))
        for i in insts:
            for s in range(ns):
                pool.set_response(i, s, resp[s][rsel(i)])
        # the small pool's instance i % CAP stands in for instance i: both hold response set rsel(i)
        sm = [small.add() for _ in range(CAP)]
        for i in sm:
            for s in range(ns):
                small.set_response(i, s, resp[s][rsel(i)])
        streams = [ol.Stream(L, M, ol.REAL) for _ in range(NINST)]
        win = np.zeros((NINST, N), np.float32)
        refs = []
        if ol.have_ref():
            for i in range(NREF):
                rm = ol.RefMaster(L, M, ol.REAL)
                chans = []
                for s, (olen, typ) in enumerate(slaves):
                    ch = rm.channel(olen, typ)
                    ch.set_response(resp[s][rsel(i)])
                    chans.append(ch)
                refs.append((rm, chans))
        dup = 5                                                   # listed twice, with other shifts
        for blk in range(NBLOCKS):
            x = rng.standard_normal((NINST, L)).astype(np.float32)
            win[:, :M - 1] = win[:, L:].copy()
            win[:, M - 1:] = x
            spec = [streams[i].push(x[i], f64=True) for i in range(NINST)]
            req = list(range(NINST)) + [dup]
            n = len(req)
            shifts = np.zeros((n, ns), np.int32); isb = np.zeros((n, ns), np.uint8); mask = np.zeros(n, np.uint8)
            for r, i in enumerate(req):
                for s, (olen, typ) in enumerate(slaves):
                    menu = shift_menu(bins, N * olen // L)
                    shifts[r, s] = menu[(i + 3 * s + blk + (4 if r >= NINST else 0)) % len(menu)]
                    isb[r, s] = typ == C and (i + s) % 4 == 2
                mask[r] = (1 << ns) - 1
                if i % 4 == 1:
                    mask[r] = (1 << ns) - 2                       # leaves slave 0 out (the only slave: the request runs nothing)
                if i % 8 == 3 and ns > 2:
                    mask[r] = 1 << 1                              # the middle slave alone
            assert (shifts[NINST] != shifts[dup]).any()
            SENT = 7.0
            out = [np.full((n, olen), SENT, np.complex64 if typ == C else np.float32) for olen, typ in slaves]
            pool.execute([insts[i] for i in req], win[req], shifts, mask, isb, out)
            out2 = [np.full((n, olen), SENT, o.dtype) for o, (olen, typ) in zip(out, slaves)]
            small.execute([sm[i % CAP] for i in req], win[req], shifts, mask, isb, out2)
            for s in range(ns):
                assert np.array_equal(out2[s].view(np.uint8), out[s].view(np.uint8)), "the call in three chunks differs from the call in two"
            worst = 0.0
            for r, i in enumerate(req):
                for s, (olen, typ) in enumerate(slaves):
                    if not (mask[r] >> s) & 1:
                        assert (out[s][r] == SENT).all(), "a slave the mask leaves out was written"
                        continue
                    P = N * olen // L
                    want = want_f64(spec[i], P, olen, typ, int(shifts[r, s]), resp[s][rsel(i)], bool(isb[r, s]))
                    worst = max(worst, check_channel(out[s][r], want))
            print("%s block %d: worst rel-L2 vs float64 oracle %.3g" % (name, blk, worst))
            for i, (rm, chans) in enumerate(refs):
                rm.write(x[i])
                for s, ch in enumerate(chans):
                    ch.set_isb(bool(isb[i, s]))
                    want = ch.execute(int(shifts[i, s]))          # (every block: a slave of the reference that sits one out falls a job behind)
                    if (mask[i] >> s) & 1:
                        check_channel(out[s][i], want)
    finally:
        pool.close(); small.close()
        for rm, _ in (refs if "refs" in locals() else []):
            rm.close()


def test_strong_pilot_line_on_the_wfm_geometry(pkg):
    """Noise 1e-3 plus a 0.1 cosine exactly on the pilot's bin (19 kHz at 384 kHz, 25 Hz bins: bin 760), slaves run as wfm runs them:
    mono at 0, pilot at 760, L-R at 1520 (src/wfm.c:188-223).  The float32 transform's error in every bin is set by the line, so the
    allowance is the project's noise_floor(), nothing looser."""
    L, M, slaves = GEOMS["wfm"]
    N, ns = L + M - 1, len(slaves)
    rng = np.random.default_rng(19000)
    resp = [ol.set_filter(1920, 960, N, True, 0.0, 15000 / 48000, 3.0, R), ol.set_filter(1920, 960, N, True, -100 / 48000, 100 / 48000, 3.0, C),
            ol.set_filter(1920, 960, N, True, -15000 / 48000, 15000 / 48000, 3.0, C)]
    pool = pkg.engine.RealMiniPool(L, M, slaves, 4)
    try:
        insts = [pool.add() for _ in range(3)]
        for i in insts:
            for s in range(ns):
                pool.set_response(i, s, resp[s])
        streams = [ol.Stream(L, M, ol.REAL) for _ in insts]
        win = np.zeros((3, N), np.float32)
        shifts = np.tile(np.array([0, 760, 1520], np.int32), (3, 1))
        t = 0
        for blk in range(NBLOCKS):
            n = np.arange(t, t + L); t += L
            x = (1e-3 * rng.standard_normal((3, L)) + 0.1 * np.cos(2 * np.pi * 760 * n / N)[None, :]).astype(np.float32)
            win[:, :M - 1] = win[:, L:].copy(); win[:, M - 1:] = x
            out = pool.execute(insts, win, shifts)
            for i in range(3):
                spec = streams[i].push(x[i], f64=True)
                for s, (olen, typ) in enumerate(slaves):
                    want = want_f64(spec, 1920, olen, typ, int(shifts[i, s]), resp[s], False)
                    e = check_channel(out[s][i], want, noise_floor(spec, resp[s]))
                    print("pilot line block %d inst %d slave %d: rel-L2 %.3g" % (blk, i, s, e))
    finally:
        pool.close()


def test_same_request_alone_and_among_others_gives_identical_bits(pkg):
    L, M, slaves = GEOMS["stereod"]
    N, ns = L + M - 1, len(slaves)
    rng = np.random.default_rng(5)
    resp = responses(L, M, slaves)
    pool = pkg.engine.RealMiniPool(L, M, slaves, NINST)
    try:
        insts = [pool.add() for _ in range(NINST)]
        for i in insts:
            for s in range(ns):
                pool.set_response(i, s, resp[s][rsel(i)])
        win = rng.standard_normal((NINST, N)).astype(np.float32)
        shifts = rng.integers(-40, 900, (NINST, ns)).astype(np.int32)
        isb = np.zeros((NINST, ns), np.uint8); isb[:, 1] = 1
        among = pool.execute(insts, win, shifts, None, isb)
        k = 17
        alone = pool.execute([insts[k]], win[k:k + 1], shifts[k:k + 1], None, isb[k:k + 1])
        again = pool.execute(insts, win, shifts, None, isb)
        for s in range(ns):
            assert among[s][k].any()
            assert np.array_equal(alone[s][0].view(np.uint8), among[s][k].view(np.uint8))
            assert np.array_equal(again[s].view(np.uint8), among[s].view(np.uint8))
    finally:
        pool.close()


@pytest.mark.parametrize("why,args,word", [
    ("odd N", (8, 8, [(8, C)], 4), "even N"),
    ("N = 16386", (8193, 8194, [(8193, C)], 4), "16384"),
    ("non-integer P", (300, 101, [(7, C)], 4), "not an integer"),         # 400 * 7 / 300
    ("REAL slave with odd P", (8, 19, [(4, R)], 4), "even P"),            # N = 26, P = 13
    ("prime factor 17", (272, 273, [(272, C)], 4), "above 13"),           # N/2 = 272 = 16 * 17
    ("5 slaves", (1920, 1921, [(240, C)] * 5, 4), "1 to 4"),
])
def test_refusals_at_creation(pkg, why, args, word):
    L, M, slaves, cap = args
    with pytest.raises(pkg.engine.ChzError) as e:
        pkg.engine.RealMiniPool(L, M, slaves, cap)
    assert word in str(e.value), (why, str(e.value))


def test_a_slave_size_with_a_prime_factor_above_13_is_refused(pkg):
    with pytest.raises(pkg.engine.ChzError) as e:
        pkg.engine.RealMiniPool(40, 41, [(17, C)], 4)             # N = 80, P = 34 = 2 * 17
    assert "13" in str(e.value)


def test_full_pool_and_released_instance_are_refused(pkg):
    L, M, slaves = GEOMS["smallest"]
    pool = pkg.engine.RealMiniPool(L, M, slaves, 2)
    try:
        a, b = pool.add(), pool.add()
        with pytest.raises(pkg.engine.ChzError) as e:
            pool.add()
        assert "full" in str(e.value)
        pool.release(b)
        win = np.ones((1, L + M - 1), np.float32)
        with pytest.raises(pkg.engine.ChzError) as e:
            pool.execute([b], win)
        assert "not in use" in str(e.value)
        with pytest.raises(pkg.engine.ChzError) as e:
            pool.set_response(b, 0, np.zeros(16, np.complex64))
        assert "not in use" in str(e.value)
        with pytest.raises(pkg.engine.ChzError):
            pool.release(b)
        assert pool.add() == b
        pool.execute([a, b], np.ones((2, L + M - 1), np.float32))
    finally:
        pool.close()
