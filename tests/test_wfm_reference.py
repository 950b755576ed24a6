"""Pins tests/wfm_oracle.py -- the checker of every device test of the WFM decoder pool -- to the reference's own src/wfm.c through the
reference-link mini-radiod (oracle/_ref/mini_radiod_ref: the reference's radio.c, wfm.c, filter.c ...).

Input: mr.wfm_channels() on mr.WFM_GEOM.  The baseband of ssrc 600-603 comes from the oracle channel on the oracle's float32 transform
(P 9600, olen 7680, the frame's bin_shift: all four frequencies have zero remainder and shifts divisible by the overlap factor 5, so
neither a fine oscillator nor a block phase correction turns), bb_power and n0 from the reference's own frames.  Frame kind, channels,
mute and nfloat must be equal on every frame; fm_snr, foffset, pdeviation, out_power and the float PCM are measured after WFM_SETTLE
frames and held to max(mini_radiod_lib.check's figure, 4 x the reference's own spread between its float64 and float32 transforms) --
check()'s rule.

Why the float32 transform and not the float64 one: in the very first block half of the channel filter's output is its precursor, 1e-10
of the signal.  A float32 transform buries that under its rounding noise (1e-8), the discriminator demodulates noise there and the pilot
filter finds "a pilot" in it -- in the reference on either of its transforms, so the pilot-less channel 602 sends ONE stereo frame.  A
float64 baseband keeps the precursor clean and that frame mono: equal frame kinds on EVERY frame need a baseband that rounds as a
channel's baseband does.  Measured with it: float PCM within 8e-8 of the reference's (relative L2), out_power within 1.3e-7."""
import os

import numpy as np
import pytest

import mini_radiod_lib as mr
import oracle_lib as ol
import wfm_oracle as wo

NBLOCKS, WFM_SETTLE = 16, 4
FLOAT_TOL, SCALAR_TOL, FACTOR = 1e-5, 1e-5, 4.0         # mini_radiod_lib.check: float_tol, n0_tol (its figure for a frame's scalars), factor
SCALARS = (("fm_snr", "snr"), ("foffset", "foffset"), ("pdeviation", "pdeviation"), ("out_power", "output_power"))

needs_ref_exe = pytest.mark.skipif(not os.path.exists(mr.REF_EXE), reason="oracle/_ref/mini_radiod_ref not built (needs the reference tree at build time)")


def rel(a, b):
    return abs(a - b) / max(abs(a), 1e-300)


def pcm_err(a, b, peak):
    """(relative L2, rms error over the channel's loudest frame) as mini_radiod_lib.diff measures a frame"""
    fa, fb = a.astype(np.float64), b.astype(np.float64)
    err = float(np.sqrt(np.mean((fa - fb) ** 2))); rms = float(np.sqrt(np.mean(fa ** 2)))
    return (err / rms if rms > 1e-3 * peak else 0.0), err / max(peak, 1e-300)


@needs_ref_exe
def test_the_restatement_equals_the_reference_s_wfm_c(tmp_path):
    ol.build()
    ch = mr.wfm_channels()
    fs, l, m = mr.WFM_GEOM
    l, m = int(l), int(m)
    N, P, olen = l + m - 1, 9600, 7680
    x = mr.synthesise(ch, fs, l, NBLOCKS, seed=41)
    A, _, _ = mr.run(mr.REF_EXE, str(tmp_path / "ref"), ch, x, fs, l, m, NBLOCKS)
    A32, _, _ = mr.run(mr.REF_EXE, str(tmp_path / "ref32"), ch, x, fs, l, m, NBLOCKS, env={"MINI_RADIOD_FFT_F32": "1"})
    stream = ol.Stream(l, m, ol.REAL)
    spec = [stream.push(x[b * l:(b + 1) * l]) for b in range(NBLOCKS)]
    chan_resp = ol.set_filter(P, olen, N, True, -110000.0 / wo.COMPOSITE_RATE, 110000.0 / wo.COMPOSITE_RATE, 11.0)       # the wfm preset's edges, DEFAULT_KAISER_BETA
    resp = wo.responses(0.02)
    by_ssrc = {c.ssrc: c for c in ch}
    worst = {}
    for ssrc in (600, 601, 602, 603):
        F, F32 = A[ssrc], A32[ssrc]
        assert len(F) == NBLOCKS == len(F32)
        stereo = "stereo=yes" in by_ssrc[ssrc].extra                                 # the preset says mono=yes (src/wfm.c:43-45)
        dec = wo.Decoder(0.02, resp, stereo_enable=stereo, squelch_open=10.0 ** 1.0, squelch_close=10.0 ** 0.6, squelch_tail=1, bandwidth=220000.0,
                         headroom=10 ** (-15 / 20), deemph_rate=float(-np.expm1(-1.0 / (75e-6 * 384000.0))), deemph_gain=1.0)
        peak = max([float(np.sqrt(np.mean(f["pcm_f"].astype(np.float64) ** 2))) for f in F if f["pcm_f"] is not None] or [0.0])
        w = {"float_rel": 0.0, "float_abs_over_peak": 0.0, **{k: 0.0 for k, _ in SCALARS}}
        own = dict(w)
        for blk, (f, f32) in enumerate(zip(F, F32)):
            bb = ol.channel(spec[blk], ol.REAL, P, olen, f["bin_shift"], chan_resp).astype(np.complex64)
            r = dec.block(bb, f["bb_power"], f["n0"])
            got = (r["frame"], r["channels"], r["mute"], 0 if r["pcm"] is None else r["pcm"].size)
            assert got == (f["isnull"], f["channels"], f["mute"], f["nfloat"]), (ssrc, blk, got, (f["isnull"], f["channels"], f["mute"], f["nfloat"]))
            if blk < WFM_SETTLE:
                continue
            same = (f["isnull"], f["channels"], f["mute"], f["nfloat"]) == (f32["isnull"], f32["channels"], f32["mute"], f32["nfloat"])
            for k, mine in SCALARS:
                if f[k] == 0 and r[mine] == 0:
                    continue
                w[k] = max(w[k], rel(f[k], r[mine]))
                own[k] = max(own[k], rel(f[k], f32[k]))
            if f["pcm_f"] is None:
                continue
            a, b = pcm_err(f["pcm_f"], r["pcm"], peak)
            w["float_rel"] = max(w["float_rel"], a); w["float_abs_over_peak"] = max(w["float_abs_over_peak"], b)
            if same and f32["pcm_f"] is not None:
                a, b = pcm_err(f["pcm_f"], f32["pcm_f"], peak)
                own["float_rel"] = max(own["float_rel"], a); own["float_abs_over_peak"] = max(own["float_abs_over_peak"], b)
        worst[ssrc] = (w, own)
        print("ssrc %d: restatement vs reference %s; reference float64 vs float32 transform %s" % (ssrc, w, own))
    for ssrc, (w, own) in worst.items():
        for k in w:
            lim = max(FLOAT_TOL if k.startswith("float") else SCALAR_TOL, FACTOR * own[k])
            assert w[k] <= lim, (ssrc, k, w[k], lim)
