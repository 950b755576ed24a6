"""Parameter changes written into RUNNING demodulators: what tests/test_oracle_vs_reference.py (the reference's own loops against the
restatement's set_params), tests/test_gpu_demod_midstream.py (chz_bank_set_demod at a block J > 0 against the restatement) and the
emulated run of the latter share.

A scenario is one channel: its demodulator kind, its input, the parameters it starts with and a list of (block, changed members).  Every
input keeps what the scenario needs for the whole run (a PLL channel's carrier never goes away), so no block is compared leniently.
cover(S, T) says, from the RESTATEMENT's own status records of the changed channel (S) and of a twin that was never changed (T), that
the scenario reached the branch it is there for; it holds on the CPU before anything runs on a device."""
import functools

import numpy as np

import oracle_lib as ol

NBLK = 60
BT = 0.02


def _frames(S, lo, hi=NBLK):
    return {(s.frame, s.mute) for s in S[lo:hi]}


def _differs(S, T, lo, hi=NBLK):
    return any((s.frame, s.mute, s.gain, s.output_power, s.pcm) != (t.frame, t.mute, t.gain, t.output_power, t.pcm) for s, t in zip(S[lo:hi], T[lo:hi]))


def _same(S, T, lo, hi):
    return not _differs(S, T, lo, hi)


def _first_lock(S):
    return next((b for b, s in enumerate(S) if s.pll_lock), None)


def _ratio(S, b):
    return S[b + 1].gain / S[b].gain


DATA, SIL, CLOSED = (ol.FRAME_DATA, 0), (ol.FRAME_SILENCE, 0), (ol.FRAME_SILENCE, 1)

# ---- linear -----------------------------------------------------------------------------------------------------------------
# sig "levels": _demod_case (carrier fading in, a loud burst in block 9, the level dropping at block 14: hang, then recovery);
# "steady": the same without burst and drop; "carrier" / "bpsk": _coherent_case with the carrier up from block 0 to the end
LINEAR = [
    dict(name="shift", sig="steady", base=dict(agc=False, gain_db=30.0, shift=517.0, encoding=ol.PCM_S16LE),
         sw=[(10, dict(shift=730.0)), (22, dict(shift=0.0)), (34, dict(shift=-310.0))],
         # every stretch differs from the twin's 517 Hz (10.34 cycles a block: the phase at a change is no whole number); the 0 Hz stretch is the input times the gain (an oscillator at 0 Hz is not stepped)
         cover=lambda S, T: _same(S, T, 0, 10) and _differs(S, T, 10, 22) and _differs(S, T, 22, 34) and _differs(S, T, 34)),
    dict(name="agc_off_on", sig="levels", base=dict(),
         sw=[(16, dict(agc=False, gain_db=0.0)), (24, dict(agc=True, gain_db=-20.0))],
         # switched off in mid-recovery: the running gain stays (q.gain = 0 dB is ignored) while the twin's goes on, and moves again
         # afterwards from where it stood (q.gain = -20 dB is ignored)
         cover=lambda S, T: S[15].gain == T[15].gain != S[14].gain and {s.gain for s in S[16:24]} == {S[15].gain} and T[23].gain > 1.2 * T[15].gain and
         S[15].gain < S[24].gain < 1.1 * S[15].gain and S[40].gain > 1.5 * S[15].gain),
    dict(name="agc_recovery", sig="levels", base=dict(hangtime=0.1),
         sw=[(26, dict(hangtime=0.1, recovery_db_per_s=40.0, threshold_db=-12.0, headroom_db=-12.0))],
         # recovering at 20 dB/s before block 26 and at 40 dB/s after it: gain_change = recovery_rate ** (1 / samprate), a block is 20 ms
         cover=lambda S, T: abs(20 * np.log10(_ratio(S, 23)) - 0.4) < 1e-6 and abs(20 * np.log10(_ratio(S, 27)) - 0.8) < 1e-6),
    dict(name="snr_squelch", sig="steady", base=dict(squelch_tail=2),
         sw=[(8, dict(snr_squelch=True)), (16, dict(snr_squelch=True, squelch_open_db=60.0, squelch_close_db=59.0)),
             (17, dict(snr_squelch=True, squelch_open_db=60.0, squelch_close_db=59.0, squelch_tail=5)), (36, dict(snr_squelch=True, squelch_tail=5))],
         # open when it is switched on (8); after the thresholds went up (16) it counts down from tail + 4 = 6 -- two muted DATA frames,
         # three of silence, closed; the tail written at 17 does not touch the count (src/linear.c:333-337) and shows when it re-opens (36)
         cover=lambda S, T: _frames(S, 8, 16) == {DATA} and [s.squelch_state for s in S[16:23]] == [5, 4, 3, 2, 1, 0, 0] and
         {(ol.FRAME_DATA, 1), SIL, CLOSED} == _frames(S, 16, 36) and S[36].squelch_state == 9 and _frames(S, 36) == {DATA} and _frames(T, 0) == {DATA}),
    dict(name="env", sig="levels", base=dict(dc_alpha=0.002, encoding=ol.PCM_S16LE),
         sw=[(10, dict(env=True)), (20, dict(env=False))],
         cover=lambda S, T: _same(S, T, 0, 10) and _differs(S, T, 10, 20) and all(s.output_power != t.output_power for s, t in zip(S[10:20], T[10:20]))),
    dict(name="channels", sig="levels", base=dict(encoding=ol.PCM_F32LE),
         sw=[(10, dict(channels=2)), (20, dict(channels=1))],
         cover=lambda S, T: [len(s.pcm) for s in (S[9], S[10], S[19], S[20])] == [len(T[9].pcm), 2 * len(T[9].pcm), 2 * len(T[9].pcm), len(T[9].pcm)]),
    dict(name="encoding", sig="levels", base=dict(encoding=ol.PCM_S16BE),
         sw=[(10, dict(encoding=ol.PCM_F32LE)), (20, dict(encoding=ol.PCM_MULAW)), (30, dict(encoding=ol.PCM_F16LE))],
         cover=lambda S, T: [len(s.pcm) * 2 // len(T[0].pcm) for s in (S[9], S[10], S[20], S[30])] == [2, 4, 1, 2] and S[30].pcm != T[30].pcm),
    dict(name="pll_off_on", sig="carrier", base=dict(squelch_tail=0),
         sw=[(4, dict(pll=True))],
         # lock_count starts from -limit (src/linear.c:150-154): 2 * limit = fs samples = 50 blocks to the lock, not the 25 of a fresh one
         cover=lambda S, T: _first_lock(S) == 4 + 49 and _first_lock(T) is None and S[3].pll_snr == 0 and S[4].pll_snr > 10 and _frames(S, 0) == {DATA}),
    dict(name="pll_on_off_on", sig="carrier", base=dict(pll=True, squelch_tail=0),
         sw=[(2, dict(pll=False)), (4, dict(pll=True))],
         cover=lambda S, T: _first_lock(T) == 24 and _first_lock(S) == 4 + 49 and _frames(S, 2, 4) == {DATA}),
    dict(name="pll_square", sig="bpsk", base=dict(pll=True, square=True, pll_bw=20.0, channels=2, encoding=ol.PCM_F32LE),
         sw=[(34, dict(square=False)), (44, dict(square=True))],
         # (the locked loop is 2 Hz wide: ten blocks without the squaring move it, and do not unlock it)
         cover=lambda S, T: _first_lock(S) == 24 and _same(S, T, 0, 34) and all(s.pll_snr != t.pll_snr and s.pcm != t.pcm for s, t in zip(S[35:], T[35:])) and
         all(s.pll_lock for s in S[24:])),
    dict(name="pll_loop_bw", sig="carrier", base=dict(pll=True, pll_bw=100.0),
         sw=[(34, dict(pll_bw=15.0))],
         cover=lambda S, T: _first_lock(S) == 24 and S[33].pll_lock and _same(S, T, 0, 34) and _differs(S, T, 34) and all(s.pll_lock for s in S[34:])),
]

# ---- FM ---------------------------------------------------------------------------------------------------------------------
# the carrier comes up in block 6 and fades out over blocks 46..49 (_fm_case); "tone": a 100 Hz PL tone on it
FM = [
    dict(name="fm_squelch", tone=0.0, base=dict(squelch_tail=1),
         sw=[(14, dict(snr_squelch=True)), (24, dict(snr_squelch=True, squelch_open=1e6, squelch_close=1e5)),
             (25, dict(snr_squelch=True, squelch_open=1e6, squelch_close=1e5, squelch_tail=4)), (36, dict(snr_squelch=True, squelch_tail=4))],
         # tail + 5 = 6 when the thresholds go up (24); the count goes on under the longer tail (src/fm.c:152), which shows at the re-opening (36)
         cover=lambda S, T: _frames(S, 14, 24) == {DATA} and [s.squelch_state for s in S[23:31]] == [6, 5, 4, 3, 2, 1, 0, 0] and
         S[36].squelch_state == 9 and {DATA, SIL, CLOSED} <= _frames(S, 24) and _frames(T, 24, 44) == {DATA}),
    dict(name="fm_deemph", tone=0.0, base=dict(encoding=ol.PCM_S16LE),
         sw=[(15, dict(deemph_tc=0)), (25, dict(deemph_tc=530.5e-6, deemph_gain_db=6.0))],
         cover=lambda S, T: _same(S, T, 0, 15) and _differs(S, T, 15, 25) and _differs(S, T, 25, 44) and
         all(0.2 < s.output_power / t.output_power < 0.3 for s, t in zip(S[30:44], T[30:44]))),
    dict(name="fm_threshold_extend", tone=0.0, base=dict(encoding=ol.PCM_F32LE),
         sw=[(15, dict(threshold_extend=True)), (25, dict(threshold_extend=False))],
         # (what stays of it afterwards is chan->sig.foffset, which the weighted samples pulled: a time constant of one second)
         cover=lambda S, T: _same(S, T, 0, 15) and all(s.output_power < 0.9 * t.output_power for s, t in zip(S[15:25], T[15:25])) and
         all(s.output_power > 0.95 * t.output_power for s, t in zip(S[26:44], T[26:44]))),
    dict(name="fm_pll", tone=0.0, base=dict(),
         sw=[(15, dict(pll=True)), (30, dict(pll=False))],
         cover=lambda S, T: _same(S, T, 0, 15) and all(s.output_power < 0.9 * t.output_power for s, t in zip(S[15:30], T[15:30])) and _frames(S, 15, 44) == {DATA} and
         all(s.output_power > 0.95 * t.output_power for s, t in zip(S[31:44], T[31:44]))),
    dict(name="tone_on", tone=100.0, base=dict(squelch_tail=0),
         sw=[(8, dict(tone_freq=100.0))],
         # muted from the change until two integrations of 0.24 s (12 blocks each) have seen the tone with a steady phase (src/fm.c:285-298)
         cover=lambda S, T: [s.tone_mute for s in S[7:33]] == [0] + [1] * 23 + [0, 0] and _frames(S, 8, 31) == {CLOSED} and _frames(S, 31, 44) == {DATA} and _frames(T, 8, 44) == {DATA}),
    dict(name="tone_other", tone=100.0, base=dict(tone_freq=100.0, squelch_tail=0),
         sw=[(36, dict(tone_freq=123.0))],
         cover=lambda S, T: S[6].tone_mute == 1 and S[35].tone_mute == 0 and all(s.tone_mute for s in S[36:50]) and _frames(S, 30, 36) == {DATA} and
         DATA not in _frames(S, 36) and _frames(T, 36, 44) == {DATA}),
    dict(name="tone_off", tone=0.0, base=dict(tone_freq=100.0, squelch_tail=0),
         sw=[(20, dict(tone_freq=0.0))],
         cover=lambda S, T: DATA not in _frames(S, 0, 20) and _frames(S, 20, 44) == {DATA} and DATA not in _frames(T, 0)),
]

# two halves, each with linear and FM, changed and unchanged channels in the one group of 64 lanes
SETS = {"a": LINEAR[:6] + FM[:3], "b": LINEAR[6:] + FM[3:]}
SCENARIOS = {s["name"]: s for s in LINEAR + FM}


class Rec:
    """One block of one channel as the restatement reports it."""

    def __init__(self, pcm, st):
        self.pcm = None if pcm is None else pcm.tobytes()
        for f in ("frame", "mute", "squelch_state", "pll_lock", "tone_mute", "output_power", "gain", "pll_snr", "pll_rotations", "pll_cphase", "foffset"):
            setattr(self, f, getattr(st, f))

    def status_tuple(self):
        return (self.frame, self.mute, self.squelch_state, self.pll_lock, self.tone_mute, self.output_power, self.gain)


def is_fm(sc):
    return "tone" in sc


def params_of(sc, fs):
    """[(block, LinParams)]: the parameters the channel starts with (block 0) and every later set; a later set names the members that
    differ from the START (not from the set before it)."""
    make = (lambda **kw: ol.fm_params(samprate=fs, bandwidth=8000.0, **kw)) if is_fm(sc) else (lambda **kw: ol.lin_params(samprate=fs, **kw))
    return [(0, make(**sc["base"]))] + [(b, make(**dict(sc["base"], **upd))) for b, upd in sc["sw"]]


def signal(sc, N, seed):
    """(baseband complex64[NBLK][N], bb_power[NBLK], noise estimates[NBLK]) of the scenario's channel."""
    from test_oracle_vs_reference import _coherent_case, _demod_case, _fm_case
    fs = float(round(N / BT))
    r = np.random.default_rng(seed)
    if is_fm(sc):
        bb, power = _fm_case(r, NBLK, N, fs, tone=sc["tone"], last=50)
        est = (2 * 2e-3 ** 2 / fs) * (1 + 0.1 * r.standard_normal(NBLK))
    elif sc["sig"] in ("carrier", "bpsk"):
        bb, power = _coherent_case(r, NBLK, N, sc["sig"] == "bpsk", last=NBLK + 1, first=0)
        est = np.full(NBLK, 2 * 4e-4 ** 2 / fs)
    else:
        bb, power = _demod_case(r, NBLK, N, bursts=sc["sig"] == "levels")
        est = 1e-8 * (1 + 0.3 * r.standard_normal(NBLK)) / fs
    return bb, power, est


def restated(sets, bb, power, est, upto=NBLK):
    """The restatement through the switches: [Rec] per block."""
    d = ol.demod(sets[0][1])
    when = {b: q for b, q in sets[1:]}
    out = []
    for b in range(upto):
        if b in when:
            d.set_params(when[b])
        out.append(Rec(*d.block(bb[b], power[b], est[b], BT)))
    return out


def params_at(sets, b):
    return [q for j, q in sets if j <= b][-1]


@functools.lru_cache(maxsize=None)
def scenario(name, N):
    """Everything of one scenario at block size N, computed once: sets, the input, the restatement with (S) and without (T) the changes."""
    sc = SCENARIOS[name]
    fs = float(round(N / BT))
    sets = params_of(sc, fs)
    bb, power, est = signal(sc, N, 9000 + sorted(SCENARIOS).index(name))
    S = restated(sets, bb, power, est)
    T = restated(sets[:1], bb, power, est)
    return dict(sc=sc, sets=sets, bb=bb, power=power, est=est, S=S, T=T)
