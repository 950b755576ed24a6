"""chz_bank_set_demod on a bank that has already demodulated blocks, against the restated demodulators.

The harness is that of tests/test_gpu_demod_shapes.py (chz_bank_write_block + chz_bank_demod with demod_auto off: the device and the
restatement see the same arrays); the restatement's set_params is pinned to the reference's own running loops by
tests/test_oracle_vs_reference.py (test_*_set_params_matches_the_running_reference_loop, same scenarios: tests/demod_midstream_cases.py),
its restart entry follows demod_thread() (src/radio.c:907-978, oracle/chz_oracle.c: o_chan).  Comparison: _compare_block's rules and
tolerances of test_gpu_demod_shapes.py, without its lenient blocks -- every PLL channel's carrier stays up.  What each test reaches in
chz_bank_set_demod:

  DemodState kept, dm_osc rebased, lock / lock_count / rotations and the tone detector reset      test_live_changes_on_a_running_bank
  fresh state after off -> on, restart on a kind change, channels beyond the old active count     test_restarts_on_a_running_bank
  dm_ext / dm_mix allocated late, dm_pll_lin / dm_fm_tone recounted                               test_late_pll_and_tone_state
  the demodulator stream alone is waited for; blocks before `job` keep their parameters           test_changes_between_pipelined_runs
  validation in front of every side effect                                                        test_refused_calls_leave_the_bank_as_it_was
"""
import ctypes as C

import numpy as np
import pytest

import demod_midstream_cases as mc
import oracle_lib as ol
from conftest import load_pkg
from test_gpu_demod_shapes import OVERLAP2, _dparams

pytestmark = pytest.mark.gpu

BT = mc.BT
OPEN_BITS = 1 | 2 | 16                                    # CHZ_FLAG_NO_SAMPLES | CHZ_FLAG_MUTE | CHZ_FLAG_PENDING: none of them = open


@pytest.fixture(scope="module")
def pkg():
    p = load_pkg()
    if p.engine.lib().chz_device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests cannot run (there is no CPU fallback)")
    ol.build()
    return p


def _compare(b, i, p, rec, pcm_row, got, N, pll_seen, pll_status=False, fm_before=False):
    """_compare_block (tests/test_gpu_demod_shapes.py) for one channel, every block strict.  The gain is a recurrence over the blocks:
    its tolerance is the PLL tests' (1e-7) from the first block the channel's PLL ran, whether or not it still runs, else 1e-9.
    pll_status: chan->pll.snr / .cphase / .rotations and chan->sig.foffset of a linear channel too, at the bounds of
    test_coherent_modes_and_tone_squelch_on_the_device (tests/test_gpu_pipeline.py) for a loop with a carrier to hold on to -- with the
    PLL switched off they are what its last block left (lock and rotations cleared, src/linear.c:150-154).  fm_before: demod_fm() has run on
    this chan_t.  chan->sig.foffset is then, with the PLL off, what demod_fm() left, and an FM channel's DATA frames report it: both at the
    bound that test has for an FM channel's foffset (rel 1e-5, abs 1e-5)."""
    from test_oracle_vs_reference import _cmp_pcm
    assert (got.frame, got.mute, got.squelch_state, got.tone_mute) == (rec.frame, rec.mute, rec.squelch_state, rec.tone_mute), (b, i)
    assert got.pll_lock == rec.pll_lock, (b, i)
    assert got.output_power == pytest.approx(rec.output_power, rel=1e-5, abs=1e-300), (b, i)
    if p.kind == ol.DEMOD_LINEAR or rec.frame == ol.FRAME_DATA:
        assert got.gain == pytest.approx(rec.gain, rel=1e-7 if pll_seen else 1e-9), (b, i)
    if rec.frame == ol.FRAME_DATA:
        nb = ol.pcm_bytes(p.encoding, N * p.channels)
        assert _cmp_pcm(p, pcm_row[:nb], np.frombuffer(rec.pcm, np.uint8), 1e-4 if (p.env and p.dc_alpha) else 8e-6), (b, i)
    if pll_status and p.kind == ol.DEMOD_LINEAR:
        assert got.pll_rotations == rec.pll_rotations, (b, i)
        assert abs(got.pll_snr - rec.pll_snr) / max(abs(rec.pll_snr), 1e-3) < 1e-9, (b, i, got.pll_snr, rec.pll_snr)
        if fm_before and not p.pll_enable:
            assert got.foffset == pytest.approx(rec.foffset, rel=1e-5, abs=1e-5), (b, i)
        else:
            assert abs(got.foffset - rec.foffset) < 1e-9, (b, i, got.foffset, rec.foffset)
        assert abs((got.pll_cphase - rec.pll_cphase + np.pi) % (2 * np.pi) - np.pi) < 1e-6, (b, i)
    if pll_status and p.kind == ol.DEMOD_FM and rec.frame == ol.FRAME_DATA:
        assert got.foffset == pytest.approx(rec.foffset, rel=1e-5, abs=1e-5), (b, i)


def _bank(pkg, eng, N, params, stride=None, active=None, cap=None):
    nch = cap or len(params)
    bank = eng.bank(2 * N, N, nch)
    bank.set_responses(0, np.ones((nch, 2 * N), np.complex64) / (2 * N))
    bank.set_tuning(0, 0, np.full(nch, 2500, np.int32), np.zeros(nch))
    bank.set_active(active or len(params)); bank.enable_noise(50.0 * eng.L)
    if stride:
        bank.set_pcm_stride(stride)
    bank.set_demod(0, 0, _dparams(pkg, params), BT)
    bank.demod_auto(False)
    return bank


def _drive(pkg, N, inputs, params, events, nblk, each=None, stride=None, active=None):
    """Runs nblk blocks of inputs[i] = (bb, power, est) through a bank that starts with params[: active]; events[b] = [(ch0, [LinParams]) |
    callable(bank)] applied as chz_bank_set_demod(job b) in front of block b.  Returns rows[b] = (pcm, [status], status bytes)."""
    eng = pkg.engine.Engine(OVERLAP2[0], OVERLAP2[1], ol.REAL, ring_blocks=8)
    rows = []
    try:
        bank = _bank(pkg, eng, N, params[:active or len(params)], stride, active, cap=len(inputs))
        for b in range(nblk):
            for ev in events.get(b, []):
                if callable(ev):
                    ev(bank)
                else:
                    bank.set_demod(b, ev[0], _dparams(pkg, ev[1]), BT)
            n = bank.active
            bank.inject(b % 4, np.stack([inputs[i][0][b] for i in range(n)]), np.array([inputs[i][1][b] for i in range(n)]),
                        np.array([inputs[i][2][b] for i in range(n)]))
            bank.demod_only(b)
            pcm, status = bank.read_pcm(b % 4)
            rows.append((pcm, list(status), bytes(status)))
            if each:
                each(bank, b, pcm, status)
    finally:
        eng.close()
    return rows


def _twins_equal(rows, base, twins, nblk):
    """An unchanged channel's bytes -- its whole PCM row and its status record -- are those of the run in which nothing was changed."""
    ss = C.sizeof(type(rows[0][1][0]))
    for b in range(nblk):
        for i in twins:
            assert np.array_equal(rows[b][0][i], base[b][0][i]), (b, i)
            assert rows[b][2][i * ss:(i + 1) * ss] == base[b][2][i * ss:(i + 1) * ss], (b, i)


# ---- A. live changes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [240, 250])                  # 250 = 15 * 16 + 10: ragged tiles
@pytest.mark.parametrize("half", ["a", "b"])
@pytest.mark.parametrize("path", ["lanes", "wave"])
def test_live_changes_on_a_running_bank(pkg, monkeypatch, path, half, N):
    """Channel 2k is scenario k of the half (demod_midstream_cases.SETS: linear and FM mixed), changed at its blocks with
    set_demod(J, 2k, ...); channel 2k + 1 is its twin: same input, never changed.  The changed channels against the restatement through
    set_params, the twins against the unchanged restatement and byte for byte against a run of the bank in which nobody was changed."""
    monkeypatch.setenv("CHZ_DEMOD_WAVE", "1" if path == "wave" else "0")
    cases = [mc.scenario(sc["name"], N) for sc in mc.SETS[half]]
    for c in cases:
        assert c["sc"]["cover"](c["S"], c["T"]), c["sc"]["name"]         # the scenario reaches its branch, by the restatement's own status
    inputs, params, events = [], [], {}
    for k, c in enumerate(cases):
        inputs += [(c["bb"], c["power"], c["est"])] * 2
        params += [c["sets"][0][1]] * 2
        for J, q in c["sets"][1:]:
            assert J > 0
            events.setdefault(J, []).append((2 * k, [q]))
    assert {p.kind for p in params} == {ol.DEMOD_LINEAR, ol.DEMOD_FM} and 16 <= len(params) <= 24
    rows = _drive(pkg, N, inputs, params, events, mc.NBLK)
    for b in range(mc.NBLK):
        pcm, status, _ = rows[b]
        for k, c in enumerate(cases):
            p = mc.params_at(c["sets"], b)
            seen = any(q.pll_enable for j, q in c["sets"] if j <= b)
            _compare(b, 2 * k, p, c["S"][b], pcm[2 * k], status[2 * k], N, seen, pll_status=True)
            _compare(b, 2 * k + 1, c["sets"][0][1], c["T"][b], pcm[2 * k + 1], status[2 * k + 1], N, bool(c["sets"][0][1].pll_enable))
    base = _drive(pkg, N, inputs, params, {}, mc.NBLK)
    _twins_equal(rows, base, range(1, len(params), 2), mc.NBLK)


# ---- B. restarts ----------------------------------------------------------------------------------------------------------
def _off(p):
    q = ol.LinParams.from_buffer_copy(bytes(p)); q.channels = 0
    return q


def _shifted(p, hz):
    q = ol.LinParams.from_buffer_copy(bytes(p)); q.shift = hz
    return q


def _restart_cases(N):
    """(input, [(block, LinParams or "off", how)]): how = "new" (a channel switched on: the restatement starts on a chan_t nobody has
    run) or "restart" (the other demodulator on the running channel: the restatement's restart entry, the chan_t carried over)."""
    fs = float(round(N / BT))
    lin = lambda **kw: ol.lin_params(samprate=fs, **kw)
    fm = lambda **kw: ol.fm_params(samprate=fs, bandwidth=8000.0, **kw)
    steady, levels, carrier = dict(sig="steady"), dict(sig="levels"), dict(sig="carrier")
    return [
        # off -> on in one call sequence for the same job: the same kind, and the other one
        (levels, [(0, lin(), "new"), (12, "off", None), (12, lin(), "new")]),
        (dict(tone=0.0), [(0, fm(), "new"), (12, "off", None), (12, lin(snr_squelch=True, encoding=ol.PCM_S16LE), "new")]),
        # off for several blocks -> on: the shift oscillator starts at phase 0 again, the tone detector muted
        (steady, [(0, lin(agc=False, gain_db=30.0, shift=517.0), "new"), (10, "off", None), (16, lin(agc=False, gain_db=30.0, shift=517.0), "new")]),
        (dict(tone=100.0), [(0, fm(tone_freq=100.0, squelch_tail=0), "new"), (33, "off", None), (37, fm(squelch_tail=0), "new")]),
        # the other demodulator without an off: the AGC's gain, hangcount and n0 go on; the squelch sequencer, am_dc, phase memory start over
        (levels, [(0, lin(env=True, dc_alpha=0.002), "new"), (14, fm(encoding=ol.PCM_S16LE), "restart"), (30, lin(env=True, dc_alpha=0.002), "restart")]),
        (dict(tone=0.0), [(0, fm(), "new"), (14, lin(snr_squelch=True, squelch_tail=2, encoding=ol.PCM_F32LE), "restart"), (28, fm(deemph_tc=0), "restart")]),
        # ... from a locked PLL: chan->sig.foffset (the loop's 30 Hz) is where demod_fm()'s offset average and PM carrier removal start,
        # and the lock survives the FM stretch (demod_fm() never touches chan->pll.lock; init_pll() only clears the loop)
        (carrier, [(0, lin(pll=True, squelch_tail=0), "new"), (30, fm(snr_squelch=True), "restart"), (40, lin(pll=True, squelch_tail=0), "restart")]),
        # what a linear demodulator WITHOUT its PLL writes into chan_t every block (lock = 0, lock_count = -limit, rotations = 0,
        # src/linear.c:150-154) is there when the PLL comes on after an FM stretch: 50 blocks to the lock, not 25 ...
        (carrier, [(0, lin(squelch_tail=0), "new"), (10, fm(), "restart"), (14, lin(pll=True, squelch_tail=0), "restart")]),
        # ... and it has cleared the lock of an earlier PLL life ("live": the same demodulator, parameters written into it)
        (carrier, [(0, lin(pll=True, squelch_tail=0), "new"), (26, lin(squelch_tail=0), "live"), (28, fm(snr_squelch=True), "restart"),
                   (32, lin(pll=True, squelch_tail=0), "restart")]),
        # the shift oscillator stands still while demod_fm() runs, whatever chan->tune.shift says (five blocks of 10.34 cycles)
        (steady, [(0, lin(agc=False, gain_db=30.0, shift=517.0), "new"), (13, _shifted(fm(), 517.0), "restart"),
                  (18, lin(agc=False, gain_db=30.0, shift=517.0), "restart")]),
        # demod_fm() with its PLL demodulator: chan->pll.was_on decides whether it sets the loop up (src/fm.c:178-184), and the loop is the
        # one demod_linear() uses -- at block 40 was_on is still set, and demod_fm() runs on the loop as init_pll() at :41 left it
        (carrier, [(0, fm(pll=True, snr_squelch=True), "new"), (12, lin(pll=True, squelch_tail=0), "restart"), (40, fm(pll=True, snr_squelch=True), "restart")]),
    ]


def _restated_restarts(sets, bb, power, est, nblk):
    """[Rec or None (off)] per block, the parameters in force per block."""
    d, recs, pars = None, [], []
    cur = None
    for b in range(nblk):
        for j, q, how in sets:
            if j != b:
                continue
            if q == "off":
                d, cur = None, None
            else:
                if how == "live":
                    d.set_params(q)
                else:
                    d = ol.demod(q, d if how == "restart" else None)
                cur = q
        recs.append(None if d is None else mc.Rec(*d.block(bb[b], power[b], est[b], BT)))
        pars.append(cur)
    return recs, pars


@pytest.mark.parametrize("N", [240, 250])
@pytest.mark.parametrize("path", ["lanes", "wave"])
def test_restarts_on_a_running_bank(pkg, monkeypatch, path, N):
    """Channels 2k / 2k + 1 as above for the cases of _restart_cases; at block 20 chz_bank_set_active brings four channels beyond the old
    active count in, set up by the same set_demod(20, ...): they are compared with a restatement that starts there.  While a channel is
    off no slot reports it open and the open read does not count it; the twins' rows stay those of the unchanged run."""
    monkeypatch.setenv("CHZ_DEMOD_WAVE", "1" if path == "wave" else "0")
    nblk = 48
    fs = float(round(N / BT))
    cases = _restart_cases(N)
    inputs, params, events, want = [], [], {}, []
    for k, (sig, sets) in enumerate(cases):
        inp = mc.signal(sig, N, 9100 + k)
        inputs += [inp, inp]
        params += [sets[0][1]] * 2
        for j, q, how in sets[1:]:
            events.setdefault(j, []).append((2 * k, [_off(sets[0][1]) if q == "off" else q]))
        want.append((_restated_restarts(sets, *inp, nblk), _restated_restarts(sets[:1], *inp, nblk)))
    old = len(params)
    late = [ol.lin_params(samprate=fs), ol.fm_params(samprate=fs, bandwidth=8000.0, tone_freq=100.0, squelch_tail=0),
            ol.lin_params(samprate=fs, pll=True, squelch_tail=0), ol.fm_params(samprate=fs, bandwidth=8000.0, pll=True)]
    late_in = [mc.signal(s, N, 9200 + i) for i, s in enumerate([dict(sig="levels"), dict(tone=100.0), dict(sig="carrier"), dict(tone=0.0)])]
    inputs += late_in
    events.setdefault(20, []).insert(0, lambda bank: bank.set_active(old + 4))
    events[20].append((old, late))
    late_want = [_restated_restarts([(20, q, "new")], *inp, nblk) for q, inp in zip(late, late_in)]
    # coverage, from the restatement: every restarted channel differs from its twin right after the restart and has sent DATA frames
    # in each of its lives; the carried-over members show
    for (recs, pars), (trecs, _) in want:
        starts = [b for b in range(1, nblk) if pars[b] is not None and pars[b] is not pars[b - 1]]
        assert starts
        for b in starts:
            assert any(r is not None and (r.status_tuple(), r.pcm) != (t.status_tuple(), t.pcm) for r, t in zip(recs[b:b + 8], trecs[b:b + 8])), b
    (r0, _), (t0, _) = want[0]
    assert r0[12].gain != t0[12].gain and r0[11].gain == t0[11].gain                  # off -> on: the AGC starts from q.gain again
    (r2, _), (t2, _) = want[2]
    assert r2[16].pcm != t2[16].pcm and r2[9].pcm == t2[9].pcm                        # ... and the shift oscillator from phase 0
    (r3, _), _ = want[3]
    assert [r.tone_mute for r in r3[30:33]] == [0, 0, 0] and all(r.frame == ol.FRAME_DATA for r in r3[37:44])
    (r4, p4), (t4, _) = want[4]
    assert r4[30].gain != pytest.approx(t4[30].gain, rel=1e-3) and r4[30].gain != p4[30].gain      # linear again: chan->output.gain is what demod_fm() left
    (r5, _), _ = want[5]
    assert r5[14].squelch_state == 6 and r5[28].squelch_state in (0, 6)               # fresh sequencers: tail + 4 of the SNR squelch, demod_fm()'s 0 or its maximum
    (r6, _), _ = want[6]
    assert r6[29].pll_lock == 1 and r6[40].pll_lock == 1 and any(r.frame == ol.FRAME_DATA for r in r6[30:40])
    (r7, _), _ = want[7]
    assert not any(r.pll_lock for r in r7) and r7[14].pll_snr > 10 and r7[47].pll_snr > 10                 # 14 + 25 < 48: a fresh lock_count would have locked
    (r8, _), _ = want[8]
    assert r8[25].pll_lock == 1 and not any(r.pll_lock for r in r8[26:]) and r8[47].pll_snr > 10
    (r9, _), (t9, _) = want[9]
    assert r9[12].pcm == t9[12].pcm and r9[18].pcm != t9[18].pcm and r9[18].pcm is not None
    (r10, p10), _ = want[10]
    assert sum(r.frame == ol.FRAME_DATA for r in r10[:12]) >= 8 and sum(r.frame == ol.FRAME_DATA for r in r10[40:]) == 8 and r10[39].pll_lock == 1
    assert {(r.frame, r.mute) for r in late_want[1][0][20:] if r} >= {mc.DATA, mc.CLOSED} and late_want[2][0][44].pll_lock == 1 and late_want[2][0][43].pll_lock == 0

    off_seen = []

    def each(bank, b, pcm, status):
        off = [2 * k for k, ((recs, _), _) in enumerate(want) if recs[b] is None]
        if not off:
            return
        _, fl = bank.read_pcm_flags(b % 4)
        count, idx, _, fl2 = bank.read_pcm_open(b % 4)
        assert np.array_equal(fl, fl2)
        for s in range(4):                                  # no slot: the ones of the blocks before the switch included
            st = bank.read_pcm(s)[1]
            flags = bank.read_pcm_flags(s)[1]
            for i in off:
                assert (st[i].frame, st[i].mute) == (ol.FRAME_SILENCE, 1) and flags[i] & OPEN_BITS, (b, s, i)
        assert not set(off) & set(idx[:count].tolist())
        assert count == sum(1 for i in range(bank.active) if not fl[i] & OPEN_BITS), b
        off_seen.append((b, tuple(off)))

    rows = _drive(pkg, N, inputs, params, events, nblk, each=each, active=old)
    assert len(off_seen) >= 10
    for b in range(nblk):
        pcm, status, _ = rows[b]
        for k, ((recs, pars), (trecs, tpars)) in enumerate(want):
            if recs[b] is not None:
                seen = any(q is not None and q.pll_enable for q in pars[:b + 1])
                fm_before = any(q is not None and q.kind == ol.DEMOD_FM for q in pars[:b + 1])
                _compare(b, 2 * k, pars[b], recs[b], pcm[2 * k], status[2 * k], N, seen, pll_status=True, fm_before=fm_before)
            _compare(b, 2 * k + 1, tpars[b], trecs[b], pcm[2 * k + 1], status[2 * k + 1], N, bool(tpars[b].pll_enable))
        if b >= 20:
            for i, (recs, pars) in enumerate(late_want):
                _compare(b, old + i, pars[b], recs[b], pcm[old + i], status[old + i], N, bool(pars[b].pll_enable))
    base = _drive(pkg, N, inputs, params, {}, nblk, active=old)
    _twins_equal(rows, base, range(1, old, 2), nblk)


# ---- C. orchestration -------------------------------------------------------------------------------------------------------
def _plain_bank(N):
    """12 channels, linear and FM alternating, no PLL and no tone squelch anywhere: dm_ext / dm_mix do not exist."""
    fs = float(round(N / BT))
    lin = [dict(squelch_tail=0), dict(env=True, dc_alpha=0.002, encoding=ol.PCM_S16LE), dict(agc=False, gain_db=30.0, shift=500.0),
           dict(snr_squelch=True, squelch_tail=2), dict(channels=2, encoding=ol.PCM_F32LE), dict(encoding=ol.PCM_MULAW)]
    fm = [dict(), dict(deemph_tc=0, encoding=ol.PCM_S16LE), dict(squelch_tail=0), dict(threshold_extend=True), dict(snr_squelch=True, squelch_tail=3), dict(encoding=ol.PCM_F16LE)]
    params, inputs = [], []
    for i in range(12):
        if i % 2 == 0:
            params.append(ol.lin_params(samprate=fs, **lin[i // 2]))
            inputs.append(mc.signal(dict(sig="carrier" if i == 0 else "levels"), N, 9300 + i))
        else:
            params.append(ol.fm_params(samprate=fs, bandwidth=8000.0, **fm[i // 2]))
            inputs.append(mc.signal(dict(tone=100.0 if i == 5 else 0.0), N, 9300 + i))
    return params, inputs, fs


@pytest.mark.parametrize("N", [240, 250])
@pytest.mark.parametrize("path", ["lanes", "wave"])
def test_late_pll_and_tone_state(pkg, monkeypatch, path, N):
    """Ten blocks without any PLL or tone squelch; then channel 0 turns its PLL on and channel 5 a tone squelch: the state both need is
    allocated now, the kernel passes they select run from now on.  The two against the restatement, every other channel's PCM row and
    status record byte for byte those of a run that never asked."""
    monkeypatch.setenv("CHZ_DEMOD_WAVE", "1" if path == "wave" else "0")
    J, nblk = 10, 48
    params, inputs, fs = _plain_bank(N)
    p0 = ol.lin_params(samprate=fs, squelch_tail=0, pll=True)
    p5 = ol.fm_params(samprate=fs, bandwidth=8000.0, squelch_tail=0, tone_freq=100.0)
    want = {0: mc.restated([(0, params[0]), (J, p0)], *inputs[0], upto=nblk), 5: mc.restated([(0, params[5]), (J, p5)], *inputs[5], upto=nblk)}
    # channel 1 becomes a linear demodulator while there is no PLL state (block 8: chan->sig.foffset is what demod_fm() left) and an FM
    # one again after it was allocated (block 20): demod_fm() picks its offset average up where it left it
    lin1 = ol.lin_params(samprate=fs, encoding=ol.PCM_S16LE)
    r1, p1 = _restated_restarts([(0, params[1], "new"), (8, lin1, "restart"), (20, params[1], "restart")], *inputs[1], nblk)
    assert abs(r1[7].foffset) > 10 and r1[8].foffset == r1[19].foffset == r1[7].foffset and r1[20].frame == ol.FRAME_DATA
    assert want[0][J + 4].pll_snr > 10 and not any(r.pll_snr for r in want[0][:J])
    assert [r.tone_mute for r in want[5][J - 1:J + 26]] == [0] + [1] * 23 + [0, 0, 0] and want[5][J + 30].frame == ol.FRAME_DATA
    rows = _drive(pkg, N, inputs, params, {8: [(1, [lin1])], J: [(0, [p0]), (5, [p5])], 20: [(1, [params[1]])]}, nblk)
    for b in range(nblk):
        pcm, status, _ = rows[b]
        _compare(b, 1, p1[b], r1[b], pcm[1], status[1], N, False, pll_status=True, fm_before=True)
        _compare(b, 0, p0 if b >= J else params[0], want[0][b], pcm[0], status[0], N, b >= J, pll_status=True)
        _compare(b, 5, p5 if b >= J else params[5], want[5][b], pcm[5], status[5], N, False)
    base = _drive(pkg, N, inputs, params, {}, nblk)
    _twins_equal(rows, base, [i for i in range(12) if i not in (0, 1, 5)], nblk)


@pytest.mark.parametrize("N", [240, 250])
@pytest.mark.parametrize("path", ["lanes", "wave"])
def test_refused_calls_leave_the_bank_as_it_was(pkg, monkeypatch, path, N):
    """A call that is refused for its LAST entry -- a bad encoding, PCM that does not fit the bank's rows, stereo FM, a PLL without a
    bandwidth, a tone above Nyquist -- has changed nothing for the good entries in front of it: the blocks that follow are byte for
    byte those of a run without the call."""
    monkeypatch.setenv("CHZ_DEMOD_WAVE", "1" if path == "wave" else "0")
    J, nblk = 6, 16
    params, inputs, fs = _plain_bank(N)
    params[8] = ol.lin_params(samprate=fs, encoding=ol.PCM_F32LE)          # (rows of 4 * N bytes: no stereo float)
    good = [ol.lin_params(samprate=fs, pll=True, agc=False, gain_db=10.0, shift=300.0, encoding=ol.PCM_ALAW),
            ol.fm_params(samprate=fs, bandwidth=8000.0, tone_freq=88.5, pll=True, encoding=ol.PCM_F32BE),
            _off(params[2])]

    def bad(**kw):
        q = ol.LinParams.from_buffer_copy(bytes(kw.pop("of")))
        for f, v in kw.items():
            setattr(q, f, v)
        return q
    bads = [bad(of=params[3], encoding=8), bad(of=params[3], encoding=-1),
            bad(of=ol.lin_params(samprate=fs, channels=2, encoding=ol.PCM_F32LE)),
            bad(of=params[3], channels=2), bad(of=ol.lin_params(samprate=fs, pll=True), pll_loop_bw=0.0),
            bad(of=params[3], tone_freq=fs / 2), bad(of=params[3], tone_freq=-1.0)]
    refused = []

    def call(bank, q):
        with pytest.raises(pkg.engine.ChzError):
            bank.set_demod(J, 0, _dparams(pkg, good + [q]), BT)
        refused.append(q)
    rows = _drive(pkg, N, inputs, params, {J: [lambda bank, q=q: call(bank, q) for q in bads]}, nblk, stride=4 * N)
    assert len(refused) == len(bads)
    base = _drive(pkg, N, inputs, params, {}, nblk, stride=4 * N)
    _twins_equal(rows, base, range(12), nblk)
    assert any(s.frame == ol.FRAME_DATA and not s.mute for s in rows[nblk - 1][1])


def test_changes_between_pipelined_runs(pkg):
    """A bank fed by the channelizer (the geometry of test_linear_demodulator_on_the_device): run_blocks(0, J), the changes,
    run_blocks(J, n) with no chz_sync in between must end where the same sequence stepped one block at a time ends -- status of every
    channel and the last block's PCM -- and the blocks before J keep the parameters they were enqueued with: channel 0's encoding changes
    at J, and slot (J - 1) % 4, read after the second call was issued, holds block J - 1 in the old one."""
    from test_kernels_emulated import DEMOD_CASES
    from test_gpu_pipeline import _demod_engine
    L, M, P, olen, fs_out = 25920, 6481, 300, 240, 12000.0
    J, n = 9, 3
    rng = np.random.default_rng(79)
    t = np.arange(8 * L)
    env = np.ones(8 * L); env[:3 * L] = 0.02; env[6 * L:] = 0.1
    ring = ((0.05 * np.cos(2 * np.pi * (2501.3 / (L + M - 1)) * t) * env) + 1e-4 * rng.standard_normal(8 * L)).astype(np.float32)
    changes = {0: dict(encoding=ol.PCM_F32LE), 2: dict(env=False), 4: dict(shift=410.0), 5: dict(squelch_open_db=60.0, squelch_close_db=59.0),
               6: dict(tuned=True), 7: dict(encoding=ol.PCM_S16LE), 8: dict(agc=False), 9: dict(channels=2)}

    def changed(bank, params):
        out = {}
        for i, kw in changes.items():
            base = DEMOD_CASES[i]
            out[i] = ol.lin_params(**dict(base, **kw))
            bank.set_demod(J, i, _dparams(pkg, [out[i]]), BT)
        return out
    results = []
    for pipelined in (False, True):
        eng, bank, params = _demod_engine(pkg, ring, L, M, P, olen, DEMOD_CASES, fs_out)
        try:
            if pipelined:
                eng.run_blocks(0, J)
                new = changed(bank, params)
                eng.run_blocks(J, n)
            else:
                for b in range(J):
                    eng.step(b)
                before = bank.read_pcm((J - 1) % 4)
                before = (before[0].copy(), bytes(before[1]))
                new = changed(bank, params)
                for b in range(J, J + n):
                    eng.step(b)
            prev = bank.read_pcm((J - 1) % 4)               # block J - 1: n < 4, no later block has used its slot
            last = bank.read_pcm((J + n - 1) % 4)
            results.append(((prev[0].copy(), bytes(prev[1])), (last[0].copy(), bytes(last[1])), before if not pipelined else None))
        finally:
            eng.close()
    (prev_s, last_s, before), (prev_p, last_p, _) = results
    nb16, nb32 = ol.pcm_bytes(ol.PCM_S16BE, olen), ol.pcm_bytes(ol.PCM_F32LE, olen)
    assert params[0].encoding != new[0].encoding and ol.pcm_bytes(params[0].encoding, olen) == nb16
    for got in (prev_s, prev_p):                            # block J - 1 as it was before anybody called set_demod
        assert np.array_equal(got[0], before[0]) and got[1] == before[1]
    assert np.array_equal(last_p[0], last_s[0]) and last_p[1] == last_s[1]
    # the change took: channel 0's last row holds float32 where block J - 1 holds 16-bit samples (the row's upper half is still zero there)
    assert not prev_p[0][0, nb16:nb32].any() and last_p[0][0, nb16:nb32].any()
