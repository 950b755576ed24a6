"""The demodulator stage on the device at block sizes and block times other than 240 / 480 samples at 20 ms.

Blocks are handed to the stage through chz_bank_write_block + chz_bank_demod (demod_auto off), so the kernels see exactly the arrays
the restated demodulators see (oracle/chz_oracle.c, pinned to the reference's linear.c / fm.c at these shapes by
tests/test_oracle_vs_reference.py); the master only has to exist.  What each test reaches:

  ragged last tiles (LIN_TILE = PLL_TILE = FMP_TILE = 16, FM_TILE = 32)      test_demodulators_at_other_block_shapes [250, 120, 8]
  the packed-store fallback for a partial tile (s16_mono / fm_s16, tn < 16)  test_pcm_row_strides [250, stride 2000]
  rows that are not 8-byte aligned ((pcm_stride & 7) != 0)                   test_pcm_row_strides [250: 500, 1004; 240: 964]
  everything that reads blocktime (sps, fm_alpha, 0.24 s in mid-block)       test_demodulators_at_other_block_shapes [120, 8, 1200, 960]
  more than 32 AGC slices a block: demod_lin_lanes / demod_linear_tail       test_demodulators_at_other_block_shapes [1200: 50 slices]
  ... and chan_ifft's epilogue (the peak tree of lanes 32..)                 test_agc_peak_of_the_channel_kernel_with_more_than_32_slices
  chz_bank_set_pcm_stride out of range                                       test_pcm_row_stride_out_of_range_is_refused
  a bank the demodulators cannot serve, and the engine afterwards            test_bank_beyond_the_noise_window_gets_no_demodulator
"""
import functools

import numpy as np
import pytest

import oracle_lib as ol
from conftest import load_pkg

pytestmark = pytest.mark.gpu

# P = olen * N / L must be whole and, for a bank with demodulators, at most the 2048-bin noise window: N / L = 2 serves every olen up
# to 1024, radiod's N / L = 5 / 4 the multiples of 4 up to 1636
OVERLAP2 = (11520, 11521)
OVERLAP5 = (25920, 6481)


@pytest.fixture(scope="module")
def pkg():
    p = load_pkg()
    if p.engine.lib().chz_device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests cannot run (there is no CPU fallback)")
    ol.build()
    return p


def _dparams(pkg, params):
    return [pkg.engine.DemodParams(*[getattr(p, f) for f, _ in ol.LinParams._fields_]) for p in params]


def _inject_bank(pkg, eng, olen, params, bt, stride=None):
    """A bank of len(params) channels whose demodulators are fed through inject() / demod_only()."""
    nch = len(params)
    P = olen * eng.N // eng.L
    assert P * eng.L == olen * eng.N
    bank = eng.bank(P, olen, nch)
    bank.set_responses(0, np.ones((nch, P), np.complex64) / P)
    bank.set_tuning(0, 0, np.full(nch, 2500, np.int32), np.zeros(nch))
    bank.set_active(nch); bank.enable_noise(50.0 * eng.L)
    bank.set_pcm_stride(8 * olen if stride is None else stride)
    bank.set_demod(0, 0, _dparams(pkg, params), bt)
    bank.demod_auto(False)
    return bank


def _status_tuple(st):
    return (st.frame, st.mute, st.squelch_state, st.pll_lock, st.tone_mute, st.output_power, st.gain)


def _restated(params, oracles, bbs, powers, ests, nblk, bt):
    """want[b][i] = (pcm or None, (frame, mute, squelch_state, pll_lock, tone_mute, output_power, gain)): computed once per case."""
    want = []
    for b in range(nblk):
        row = []
        for i in range(len(params)):
            pcm, st = oracles[i].block(bbs[i][b], powers[i][b], ests[i][b], bt)
            row.append((None if pcm is None else pcm.copy(), _status_tuple(st)))
        want.append(row)
    return want


@functools.lru_cache(maxsize=None)
def _sweep_case(N, bt):
    from test_kernels_emulated import random_demod_channels
    nblk = 30
    params, oracles, bbs, powers, ests = random_demod_channels(424242, nblk, N, blocktime=bt)
    return params, bbs, powers, ests, _restated(params, oracles, bbs, powers, ests, nblk, bt)


def _compare_block(b, params, want_row, pcm, status, N):
    """The existing device sweep's tolerances (test_demodulators_random_parameter_sweep_on_the_device) and its rule for a PLL that has
    lost its carrier; gain at the tolerances of test_linear_demodulator_on_the_device (1e-9) and of the PLL tests (1e-7)."""
    from test_oracle_vs_reference import _cmp_pcm
    for i, p in enumerate(params):
        want, (frame, mute, sq, lock, tmute, opower, gain) = want_row[i]
        got = status[i]
        strict = not (p.pll_enable and b >= 20)            # (a PLL without a carrier is chaotic)
        assert (got.frame, got.mute, got.squelch_state, got.tone_mute) == (frame, mute, sq, tmute), (b, i)
        if not strict:
            continue
        assert got.pll_lock == lock, (b, i)
        assert got.output_power == pytest.approx(opower, rel=1e-5, abs=1e-300), (b, i)
        if p.kind == ol.DEMOD_LINEAR or frame == ol.FRAME_DATA:
            assert got.gain == pytest.approx(gain, rel=1e-7 if p.pll_enable else 1e-9), (b, i)
        if frame == ol.FRAME_DATA:
            nb = ol.pcm_bytes(p.encoding, N * p.channels)
            assert _cmp_pcm(p, pcm[i, :nb], want, 1e-4 if (p.env and p.dc_alpha) else 8e-6), (b, i)


def _inject(bank, b, bbs, powers, ests):
    nch = len(bbs)
    bank.inject(b % 4, np.stack([bbs[i][b] for i in range(nch)]), np.array([powers[i][b] for i in range(nch)]), np.array([ests[i][b] for i in range(nch)]))
    bank.demod_only(b)


# (olen, blocktime, master): 250 = 15 * 16 + 10 = 7 * 32 + 26; 120 = 7 * 16 + 8 at 10 ms (0.24 s = 24 blocks, 2.4 samples a slice);
# 8 samples in 0.5 ms: less than one tile and less than one 2 ms slice (32 samples); 1200 at 0.1 s: 50 slices, the tone decision in
# mid-block (2.4 blocks); 960 at 50 ms: 25 slices, 4.8 blocks
SHAPES = [(250, .02, OVERLAP2), (120, .01, OVERLAP2), (8, .0005, OVERLAP2), (1200, .1, OVERLAP5), (960, .05, OVERLAP5)]


@pytest.mark.parametrize("N,bt,master", SHAPES, ids=["%d-%g" % s[:2] for s in SHAPES])
@pytest.mark.parametrize("path", ["lanes", "wave"])        # demod_lin_lanes + demod_fm_lanes (+ the PLL / tone passes) / demod_linear_tail
def test_demodulators_at_other_block_shapes(pkg, monkeypatch, path, N, bt, master):
    """The 24 randomly configured channels of random_demod_channels (linear and FM alternating, so that the one group of 64 lanes
    holds both kinds; all encodings, PLLs, tone squelch) at fs = N / blocktime, 30 blocks, against the restated demodulators."""
    monkeypatch.setenv("CHZ_DEMOD_WAVE", "1" if path == "wave" else "0")
    params, bbs, powers, ests, want = _sweep_case(N, bt)
    eng = pkg.engine.Engine(master[0], master[1], ol.REAL, ring_blocks=8)
    try:
        bank = _inject_bank(pkg, eng, N, params, bt)
        for b in range(len(want)):
            _inject(bank, b, bbs, powers, ests)
            pcm, status = bank.read_pcm(b % 4)
            _compare_block(b, params, want[b], pcm, status, N)
    finally:
        eng.close()


def _stride_channels(N, nblk):
    """24 channels, linear and FM alternating, every one mono S16 (so that every row fits the smallest stride and both lane kernels
    take their packed 8-byte stores where the rows allow it); squelched stretches leave rows unsent."""
    from test_oracle_vs_reference import _demod_case, _fm_case
    fs = float(round(N / 0.02))
    lin = [dict(), dict(env=True, dc_alpha=0.002, encoding=ol.PCM_S16LE), dict(agc=False, gain_db=30.0, shift=500.0, encoding=ol.PCM_S16LE),
           dict(snr_squelch=True, squelch_tail=2), dict(tuned=False), dict(encoding=ol.PCM_S16LE, hangtime=0.3)]
    fm = [dict(), dict(deemph_tc=0, encoding=ol.PCM_S16LE), dict(threshold_extend=True), dict(snr_squelch=True, squelch_tail=3, encoding=ol.PCM_S16LE),
          dict(tone_freq=100.0, squelch_tail=0), dict(pll=True, encoding=ol.PCM_S16LE)]
    rng = np.random.default_rng(250)
    params, oracles, bbs, powers, ests = [], [], [], [], []
    for i in range(24):
        if i % 2 == 0:
            kw = lin[(i // 2) % len(lin)]
            p = ol.lin_params(samprate=fs, **kw)
            bb, power = _demod_case(np.random.default_rng(2000 + i), nblk, N)
            power = power.copy()
            if kw.get("snr_squelch"):
                power[12:18] = 1e-12
            est = 1e-8 * (1 + 0.3 * rng.standard_normal(nblk)) / fs
            orc = ol.LinDemod(p)
        else:
            kw = fm[(i // 2) % len(fm)]
            p = ol.fm_params(samprate=fs, bandwidth=8000.0, **kw)
            bb, power = _fm_case(np.random.default_rng(3000 + i), nblk, N, fs, tone=kw.get("tone_freq", 0.0), last=26)
            est = (2 * 2e-3 ** 2 / fs) * (1 + 0.1 * rng.standard_normal(nblk))
            orc = ol.FmDemod(p)
        params.append(p); oracles.append(orc); bbs.append(bb); powers.append(power); ests.append(est)
    return params, oracles, bbs, powers, ests


@functools.lru_cache(maxsize=None)
def _stride_case(N):
    nblk = 30
    params, oracles, bbs, powers, ests = _stride_channels(N, nblk)
    return params, bbs, powers, ests, _restated(params, oracles, bbs, powers, ests, nblk, 0.02)


@pytest.mark.parametrize("N", [250, 240])
@pytest.mark.parametrize("path", ["lanes", "wave"])
def test_pcm_row_strides(pkg, monkeypatch, path, N):
    """Rows of 2 * olen bytes (the smallest that holds mono S16: 500 is no multiple of 8, 480 is), 4 * olen + 4 (never one) and
    8 * olen: the first against the restatement, every row of the others bit for bit equal to it; the bytes of a row beyond the
    encoding's length and the rows of channels that sent no DATA frame stay as a first read found them."""
    monkeypatch.setenv("CHZ_DEMOD_WAVE", "1" if path == "wave" else "0")
    params, bbs, powers, ests, want = _stride_case(N)
    nch, nblk = len(params), len(want)
    nb = 2 * N                                             # mono S16
    sent = 0
    eng = pkg.engine.Engine(OVERLAP2[0], OVERLAP2[1], ol.REAL, ring_blocks=8)
    try:
        first = None
        for stride in (2 * N, 4 * N + 4, 8 * N):
            bank = _inject_bank(pkg, eng, N, params, 0.02, stride)
            shadow = [bank.read_pcm(s)[0].copy() for s in range(4)]       # what the rows hold before anything ran
            assert shadow[0].shape == (nch, stride)
            rows = []
            for b in range(nblk):
                _inject(bank, b, bbs, powers, ests)
                pcm, status = bank.read_pcm(b % 4)
                if first is None:
                    _compare_block(b, params, want[b], pcm, status, N)
                else:
                    assert [_status_tuple(s) for s in status] == first[b][1], (stride, b)
                for i in range(nch):
                    if status[i].frame == ol.FRAME_DATA:
                        shadow[b % 4][i, :nb] = pcm[i, :nb]
                        sent += 1
                assert np.array_equal(pcm, shadow[b % 4]), (stride, b, np.argwhere(pcm != shadow[b % 4])[:4])
                rows.append((pcm[:, :nb].copy(), [_status_tuple(s) for s in status]))
            if first is None:
                first = rows
            else:
                for b in range(nblk):
                    assert np.array_equal(rows[b][0], first[b][0]), (stride, b)
            bank.destroy()
    finally:
        eng.close()
    assert 0 < sent < 3 * nch * nblk                       # both kinds of rows: sent and left alone


def test_pcm_row_stride_out_of_range_is_refused(pkg):
    eng = pkg.engine.Engine(OVERLAP2[0], OVERLAP2[1], ol.REAL, ring_blocks=8)
    try:
        for olen in (250, 240):
            bank = eng.bank(2 * olen, olen, 4)
            for bad in (olen - 4, 8 * olen + 4, 2 * olen + 2, 4 * olen + 1):
                with pytest.raises(pkg.engine.ChzError):
                    bank.set_pcm_stride(bad)
            assert pkg.engine.lib().chz_bank_pcm_stride(eng._h, bank.id) == 8 * olen      # the refusals left the default
            for good in (olen + (-olen) % 4, 4 * olen + 4, 8 * olen):
                bank.set_pcm_stride(good)
                assert pkg.engine.lib().chz_bank_pcm_stride(eng._h, bank.id) == good
    finally:
        eng.close()


def test_bank_beyond_the_noise_window_gets_no_demodulator(pkg):
    """A demodulator needs the channel's noise estimate, and the estimator's window is at most 2048 bins: chz_bank_enable_noise refuses
    a bank of P > 2048 (-3), chz_bank_set_demod a bank without the estimate (-1).  So blocks of more than 2048 samples never reach
    launch_demod through the C ABI -- its requests for more than 64 KB of LDS (olen > 4096) and its own limit of 10240 samples are
    out of reach.  Both refusals leave the engine usable: a bank the stage can serve runs afterwards."""
    L = pkg.engine.lib()
    params, bbs, powers, ests, want = _sweep_case(960, .05)
    eng = pkg.engine.Engine(OVERLAP5[0], OVERLAP5[1], ol.REAL, ring_blocks=8)
    try:
        for olen in (4800, 9600, 10240, 10244):            # P = 6000 .. 12805 of the master's 16201 bins
            big = eng.bank(olen * 5 // 4, olen, 2)
            big.set_tuning(0, 0, np.full(2, 2500, np.int32), np.zeros(2)); big.set_active(2)
            assert L.chz_bank_enable_noise(eng._h, big.id, 50.0 * eng.L) == -3
            arr = (pkg.engine.DemodParams * 2)(*_dparams(pkg, params[:2]))
            assert L.chz_bank_set_demod(eng._h, big.id, 0, 0, 2, arr, 0.1) == -1
            big.destroy()
        bank = _inject_bank(pkg, eng, 960, params, .05)
        for b in range(4):
            _inject(bank, b, bbs, powers, ests)
            pcm, status = bank.read_pcm(b % 4)
            _compare_block(b, params, want[b], pcm, status, 960)
    finally:
        eng.close()


def _slice_energies(x, sps):
    e = np.abs(x.astype(np.complex128)) ** 2
    n = (len(x) - 1) // sps                                # slices that end before the block's last sample (src/linear.c:199)
    return e[:n * sps].reshape(n, sps).sum(axis=1)


@pytest.mark.parametrize("P,olen", [(1200, 960), (1920, 1536)])
def test_agc_peak_of_the_channel_kernel_with_more_than_32_slices(pkg, monkeypatch, P, olen):
    """chan_ifft (staged rows) leaves the AGC's first look at the block -- the loudest 2 ms slice -- for demod_lin_lanes; its lanes take
    the slices in turn (40 lanes a channel at P = 1200, 48 at 1920) and a tree over the lanes picks the largest.  At a block time of
    0.1 s a block has 50 / 49 slices, and a burst whose loudest slice is number 34 or 35 is seen by that lane only: the tree has to
    start at distance 32.  The linear AGC cases of DEMOD_CASES on a level-stepped input; the restatement is fed the channel outputs, bb_power
    and noise estimates read back from the slot."""
    from test_kernels_emulated import DEMOD_CASES
    monkeypatch.setenv("CHZ_DEMOD_WAVE", "0"); monkeypatch.setenv("CHZ_CHAN_STAGE", "1")
    L, M = OVERLAP5
    bt, fs_out, nblk = 0.1, float(round(olen / 0.1)), 16
    sps = int(np.rint(olen * .002 / bt))
    assert (olen - 1) // sps > 32
    cases = [kw for kw in DEMOD_CASES if kw.get("agc", True)]
    nch = len(cases)
    rng = np.random.default_rng(77)
    t = np.arange(8 * L)
    env = np.ones(8 * L); env[:3 * L] = 0.02; env[6 * L:] = 0.1       # level steps walk the AGC branches
    env[5 * L + int(0.555 * L):5 * L + int(0.59 * L)] = 8.0          # and a short burst: slice 34 / 35 of the output block
    ring = ((0.05 * np.cos(2 * np.pi * (2501.3 / (L + M - 1)) * t) * env) + 1e-4 * rng.standard_normal(8 * L)).astype(np.float32)
    eng = pkg.engine.Engine(L, M, ol.REAL, ring_blocks=8)
    late_peaks = 0
    try:
        eng.write(ring[:8 * L - (M - 1)]); eng.write(ring[8 * L - (M - 1):])
        bank = eng.bank(P, olen, nch)
        bank.set_responses(0, np.stack([pkg.filterapi.design_response(P, olen, L + M - 1, True, -0.12, 0.12, 11.0)] * nch))
        bank.set_tuning(0, 0, np.array([2500 + 3 * i for i in range(nch)], np.int32), np.array([-(3.7 + i) / fs_out for i in range(nch)]))
        bank.set_active(nch); bank.enable_noise(50.0 * L)
        params = [ol.lin_params(samprate=fs_out, **kw) for kw in cases]
        bank.set_demod(0, 0, _dparams(pkg, params), bt)
        oracles = [ol.LinDemod(p) for p in params]
        from test_oracle_vs_reference import _cmp_pcm
        for b in range(nblk):
            eng.step(b)
            out = bank.read_slot(b % 4); power = bank.read_power(b % 4); noise = bank.read_noise(b % 4)
            pcm, status = bank.read_pcm(b % 4)
            for i, p in enumerate(params):
                want, st = oracles[i].block(out[i], power[i], noise[i], bt)
                # the restatement's own input: where is this block's loudest slice, and did the AGC act on it (:203-207: the gain is set
                # from the peak and stays for the block)
                e = _slice_energies(out[i], sps)
                k = int(np.argmax(e))
                if 32 <= k < 40 and st.gain == pytest.approx(np.sqrt(2) * p.headroom / np.sqrt(e[k] / sps), rel=1e-6):
                    late_peaks += 1
                got = status[i]
                assert (got.frame, got.mute, got.squelch_state) == (st.frame, st.mute, st.squelch_state), (b, i)
                assert got.gain == pytest.approx(st.gain, rel=1e-9), (b, i)
                assert got.output_power == pytest.approx(st.output_power, rel=1e-6, abs=1e-300), (b, i)
                if st.frame == ol.FRAME_DATA:
                    nb = ol.pcm_bytes(p.encoding, olen * p.channels)
                    assert _cmp_pcm(p, pcm[i, :nb], want, 1e-6), (b, i)
    finally:
        eng.close()
    assert late_peaks >= nch // 2, late_peaks      # the peak branch was taken on a slice that only lanes 32.. of the channel hold
