"""chan_any -- the one-workgroup-per-channel kernel behind every channel size outside the register-tiled menu -- in the modes the
suite only runs at menu sizes: ISB, fine tuning + bb_power, REAL output; at odd, Bluestein and global-scratch (BIG) sizes; on a REAL
and on a COMPLEX master.

Sizes (P = 1.25 olen on both masters): 75 and 225 odd and smooth, 85 odd Bluestein (5 x 17, M = 256), 170 even Bluestein (M = 512),
16200 smooth beyond the LDS (two P-point buffers in global scratch), 12750 = 2 x 3 x 5^3 x 17 Bluestein beyond the LDS (M = 32768).
The two BIG sizes run on the REAL master only, with four channels.

Each mode keeps the comparison and the bound of the test that pins it at a menu size (tests/test_gpu_parity.py):
  ISB           test_isb_slaves: ol.channel(.., isb=) on the float32 spectrum -- here the DEVICE's own (Engine.spectrum), so that the
                channel kernel alone is measured -- within 1e-5 relative + 2 sqrt(olen) noise_floor()
  tuned + power test_tuned_bank_follows_downconvert, check (1): Downconv("oracle") applied to a plain twin bank's own rows, never more
                than one float ulp apart, bb_power within 1e-6.  The share of bit-identical samples is printed, not asserted.
                (The channel swept DOWNWARDS at the two BIG sizes -- 30,600 oscillator steps in three blocks -- is what showed that the
                reference's sincospi() rounds a negative Doppler rate to a multiple of 2^-52 half-turns, src/sincospi.c:12-19: the
                exact closed form was 2 ulp and 94 % of the samples away from it until chz_finetune.h took the same step.)
  REAL output   test_real_output_slaves: ol.channel(.., out_type=REAL) on the oracle's float32 spectrum within 1e-5 relative +
                2e-8 max|X| ||H|| sqrt(olen); an odd P is refused.
"""
import numpy as np
import pytest

import oracle_lib as ol
from conftest import load_pkg
from test_gpu_parity import _ulp_close, noise_floor

pytestmark = pytest.mark.gpu

MASTERS = {"real": (25920, 6481, ol.REAL, 1.296e6), "complex": (11520, 2881, ol.COMPLEX, 576e3)}      # 20 ms blocks, 40 Hz bins, V = 5
SMALL = [(75, 60), (225, 180), (85, 68), (170, 136)]
BIG = [(16200, 12960), (12750, 10200)]
CASES = [(m, P, olen) for m in MASTERS for P, olen in SMALL] + [("real", P, olen) for P, olen in BIG]
EVEN = [c for c in CASES if c[1] % 2 == 0]
ids = lambda cases: ["%s-P%d" % (m, P) for m, P, olen in cases]


@pytest.fixture(scope="module")
def pkg():
    p = load_pkg()
    if p.engine.lib().chz_device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests cannot run (there is no CPU fallback)")
    ol.build()
    return p


def noise(rng, in_type, n):
    if in_type == ol.REAL:
        return rng.standard_normal(n).astype(np.float32)
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)


def nchan(P):
    return 4 if P > 10240 else 6


def responses(rng, P, olen, N, master_real, nch, out_type=ol.COMPLEX):
    """Kaiser filters of several widths; for COMPLEX output every other one is random, so that the bins next to the slave's Nyquist bin
    -- the innermost pair of the ISB unpack -- carry as much as any other"""
    kinds = [(-0.45, 0.45), (0.02, 0.4), (-0.3, 0.1), (-0.5, 0.5), (0.1, 0.25), (-0.2, 0.45)]
    out = []
    for i in range(nch):
        if out_type == ol.COMPLEX and i % 2 == 1:
            out.append(((rng.standard_normal(P) + 1j * rng.standard_normal(P)) * (0.5 / N)).astype(np.complex64))
        else:
            out.append(ol.set_filter(P, olen, N, master_real, kinds[i][0], kinds[i][1], 7.0, out_type))
    return np.stack(out)


@pytest.mark.parametrize("master,P,olen", CASES, ids=ids(CASES))
def test_isb_channels(pkg, master, P, olen):
    L, M, in_type, fs = MASTERS[master]
    N = L + M - 1
    nch = nchan(P)
    rng = np.random.default_rng(P + (in_type == ol.COMPLEX))
    eng = pkg.engine.Engine(L, M, in_type, ring_blocks=8)
    try:
        bins = eng.bins
        # 0, +-40, part of the passband outside the master (on the COMPLEX master: across each Nyquist seam), two inside
        if in_type == ol.REAL:
            shifts = [0, 40, -40, bins - P // 4, 3000, -7001][:nch]
        else:
            shifts = [0, 40, -40, N // 2 - P // 4, -(N // 2) + P // 4, 3001][:nch]
        flags = [np.array([1, 1, 0, 1, 1, 0][:nch], np.uint8), np.array([0, 1, 0, 1, 0, 1][:nch], np.uint8)]       # channel 2 stays plain
        resp = responses(rng, P, olen, N, in_type == ol.REAL, nch)
        bank = eng.bank(P, olen, nch)
        bank.set_responses(0, resp); bank.set_shifts(0, np.array(shifts, np.int32)); bank.set_active(nch)
        worst, live = 0.0, 0
        for blk in range(2):
            bank.set_isb(0, flags[blk])
            eng.write(noise(rng, in_type, L)); eng.step(blk)
            spec32 = eng.spectrum(blk % 4)
            got = bank.read_slot(blk % 4)
            for ch in range(nch):
                want = ol.channel(spec32, in_type, P, olen, shifts[ch], resp[ch], isb=bool(flags[blk][ch]))
                allow = 1e-5 * np.linalg.norm(want) + noise_floor(spec32.astype(np.complex128), resp[ch]) * np.sqrt(olen) * 2
                err = float(np.linalg.norm(got[ch] - want))
                print("%s P %d block %d ch %d shift %d isb %d: error %.3g of %.3g allowed" % (master, P, blk, ch, shifts[ch], flags[blk][ch], err, allow))
                assert err <= allow, (blk, ch)
                worst = max(worst, err / allow)
                live += bool(want.any())
                if flags[blk][ch]:
                    plain = ol.channel(spec32, in_type, P, olen, shifts[ch], resp[ch], isb=False)
                    assert np.linalg.norm(want - plain) > 0.1 * np.linalg.norm(want)          # the flag matters at this tuning
        assert live == 2 * nch
        print("%s P %d: worst error / allowed %.3g" % (master, P, worst))
    finally:
        eng.close()


@pytest.mark.parametrize("master,P,olen", CASES, ids=ids(CASES))
def test_tuned_channels_follow_downconvert(pkg, master, P, olen):
    L, M, in_type, fs_in = MASTERS[master]
    N = L + M - 1
    fs_out = olen / 0.02
    nch = nchan(P)
    rng = np.random.default_rng(7 * P + (in_type == ol.COMPLEX))
    f_hz = rng.uniform(50e3, 250e3, nch) * (1 if in_type == ol.REAL else np.where(np.arange(nch) % 2, -1, 1))
    f_hz[0] = 40.0 * 2500                      # on a bin, shift % V = 0: no rotation at all
    f_hz[1] = 40.0 * 2501                      # on a bin, shift % V = 1: block phase correction only
    sweep = np.zeros(nch); sweep[2] = 35.0; sweep[3] = -120.0          # Hz/s
    eng = pkg.engine.Engine(L, M, in_type, ring_blocks=8)
    try:
        resp = responses(rng, P, olen, N, in_type == ol.REAL, nch)
        tuned = eng.bank(P, olen, nch); plain = eng.bank(P, olen, nch)
        for b in (tuned, plain):
            b.set_responses(0, resp); b.set_active(nch)
        dco = [ol.Downconv(L, M, fs_out, "oracle") for _ in range(nch)]
        shifts = np.zeros(nch, np.int32); rems = np.zeros(nch)
        worst_ulp, worst_pw, shares = 0.0, 0.0, []
        for blk in range(3):
            if blk in (0, 1):                   # everything at block 0, a retune of channels 1 .. 3 (a plain, a swept up, a swept down) at block 1
                sel = range(nch) if blk == 0 else [1, 2, 3]
                for ch in sel:
                    if blk:
                        f_hz[ch] += rng.uniform(-3e3, 3e3)
                    r, sh, rem = ol.compute_tuning(N, fs_in, f_hz[ch])
                    assert r == 0
                    shifts[ch], rems[ch] = sh, rem
                lo, hi = min(sel), max(sel) + 1
                tuned.set_tuning(blk, lo, shifts[lo:hi], -rems[lo:hi] / fs_out, sweep[lo:hi] / fs_out ** 2)
                plain.set_shifts(0, shifts)
            eng.write(noise(rng, in_type, L)); eng.step(blk)
            got = tuned.read_slot(blk % 4); raw = plain.read_slot(blk % 4)
            pw = tuned.read_power(blk % 4)
            for ch in range(nch):
                assert raw[ch].any()
                want, wpw = dco[ch].block(raw[ch], shifts[ch], rems[ch], sweep[ch])
                worst, same = _ulp_close(got[ch], want)
                print("%s P %d block %d ch %d: worst %.3g ulp, %.4f bit-identical, power off by %.3g" % (master, P, blk, ch, worst, same, abs(pw[ch] - wpw) / wpw))
                assert worst <= 1.0, (blk, ch, worst)
                assert abs(pw[ch] - wpw) <= 1e-6 * wpw, (blk, ch)
                worst_ulp = max(worst_ulp, worst); worst_pw = max(worst_pw, abs(pw[ch] - wpw) / wpw); shares.append(same)
            assert not np.array_equal(got[2], raw[2])                  # the rotation is on
        print("%s P %d: worst %.3g ulp (1 allowed), power %.3g (1e-6 allowed), bit-identical share %.4f .. %.4f" % (master, P, worst_ulp, worst_pw, min(shares), max(shares)))
    finally:
        eng.close()


@pytest.mark.parametrize("master,P,olen", EVEN, ids=ids(EVEN))
def test_real_output_channels(pkg, master, P, olen):
    L, M, in_type, fs = MASTERS[master]
    N = L + M - 1
    nch = nchan(P)
    rng = np.random.default_rng(11 * P + (in_type == ol.COMPLEX))
    eng = pkg.engine.Engine(L, M, in_type, ring_blocks=8)
    try:
        B = eng.bins
        shifts = [0, 17, -5, B - P // 4, B // 3, -(B // 3)][:nch]
        resp = responses(rng, P, olen, N, in_type == ol.REAL, nch, ol.REAL)
        bank = eng.bank(P, olen, nch, real=True)
        bank.set_responses(0, resp); bank.set_shifts(0, np.array(shifts, np.int32)); bank.set_active(nch)
        st = ol.Stream(L, M, in_type)
        worst, live = 0.0, 0
        for blk in range(2):
            x = noise(rng, in_type, L)
            eng.write(x); eng.step(blk)
            spec = st.push(x)
            got = bank.read_slot(blk % 4)
            assert got.dtype == np.float32 and got.shape == (nch, olen)
            for ch in range(nch):
                want = ol.channel(spec, in_type, P, olen, shifts[ch], resp[ch], out_type=ol.REAL)
                nrm = float(np.linalg.norm(want))
                if nrm == 0:
                    assert not got[ch].any()
                    continue
                live += 1
                allow = 1e-5 * nrm + 2e-8 * float(np.abs(spec).max()) * float(np.linalg.norm(resp[ch])) * np.sqrt(olen)
                err = float(np.linalg.norm(got[ch] - want))
                print("%s P %d block %d ch %d shift %d: error %.3g of %.3g allowed" % (master, P, blk, ch, shifts[ch], err, allow))
                assert err <= allow, (blk, ch)
                worst = max(worst, err / allow)
        assert live >= 2 * (nch - 1)
        print("%s P %d REAL output: worst error / allowed %.3g" % (master, P, worst))
    finally:
        eng.close()


@pytest.mark.parametrize("master", list(MASTERS))
def test_real_output_with_an_odd_size_is_refused(pkg, master):
    L, M, in_type, fs = MASTERS[master]
    eng = pkg.engine.Engine(L, M, in_type, ring_blocks=8)
    try:
        for P, olen in [(75, 60), (225, 180), (85, 68)]:
            with pytest.raises(pkg.engine.ChzError):
                eng.bank(P, olen, 4, real=True)
    finally:
        eng.close()
