"""Pins the numpy restatement of wideband_poll() (welch_ref in tests/test_gpu_welch.py, the checker of every device test of the
wideband analyser) to the reference's own src/spectrum.c: the reference-link mini-radiod (oracle/_ref/mini_radiod_ref: the reference's
radio.c, spectrum.c, filter.c ...) runs in lock step with wideband analysers on an input made only of stationary tones that are
bin-centred for their fft_n; EVERY wideband frame's bin data must equal the restatement applied to the known input for a window that
ends on one of the whole-block boundaries within the harness's slack of the frame's block.  Tolerance: 4 x the spread of the
reference's own steady-state frames among themselves (fft_n = 600 does not divide the block, so the tones' phases -- and with them the
small image terms and the roundings -- differ from frame to frame).

What the reference leaves undefined is not pinned: analyser 701 sits so low that the wrap at i == bin_count/2 (src/spectrum.c:400) takes
the read index below zero, where the reference reads in front of its array; only the bins it defines (i < bin_count/2) are compared
there, the restatement (and the device) give zeros for the others."""
import os

import numpy as np
import pytest

import mini_radiod_lib as mr
from test_gpu_welch import welch_ref

FS, L, M, NBLOCKS, SLACK = 1.296e6, 25920, 6481, 24, 2
FFT_N, RBW = 600, 2160.0                       # fft_n = lrint(samprate / rbw) (src/spectrum.c:614); 25920 / 600 is not an integer
TONES = ((100, 0.05, 0.3), (139, 0.1, 1.1), (150, 0.02, 2.0), (170, 0.2, 0.7), (12, 0.08, 0.1), (40, 0.03, 1.9))      # (bin, amplitude, phase)

needs_ref_exe = pytest.mark.skipif(not os.path.exists(mr.REF_EXE), reason="oracle/_ref/mini_radiod_ref not built (needs the reference tree at build time)")


def reference_window(fft_n, beta=7.0):
    """generate_window() with the defaults of src/modes.c:73-76 (Kaiser, beta 7): make_kaiserf() over fft_n + 1 points in float
    (src/window.c:217-238), normalize_windowf() over the first fft_n (src/window.c:240-254)"""
    w = np.kaiser(fft_n + 1, beta).astype(np.float32)[:fft_n]
    gain = np.float32(fft_n / w.astype(np.float64).sum())
    return w * gain


@needs_ref_exe
def test_every_wideband_frame_of_the_reference_equals_the_restatement(tmp_path):
    n = np.arange(NBLOCKS * L)
    x = np.zeros(n.size)
    for k, a, ph in TONES:
        x += a * np.cos(2 * np.pi * k * n / FFT_N + ph)
    x = x.astype(np.float32)
    spec = "demod=spectrum poll=1 rbw=%g" % RBW
    ch = [mr.Channel(700, 139 * RBW, "usb", spec + " bins=128 fft-avg=2", {"kind": "spectrum_wide"}),       # bins 75..202 of 0..300
          mr.Channel(701, 10 * RBW, "usb", spec + " bins=64 fft-avg=3", {"kind": "spectrum_wide"}),         # the wrap goes below bin 0
          mr.Channel(702, 170 * RBW, "usb", spec + " bins=101 fft-avg=1", {"kind": "spectrum_wide"})]       # odd bin count
    frames, meta, _ = mr.run(mr.REF_EXE, str(tmp_path / "ref"), ch, x, FS, L, M, NBLOCKS, slack=SLACK)
    # the input as the ring presents it: zeros in front of time 0 (a window reaching back before it wraps into the zeros appended here)
    ring = np.concatenate([x, np.zeros(8 * FFT_N, np.float32)])
    win = reference_window(FFT_N)
    seen = 0
    for c, avg in zip(ch, (2, 3, 1)):
        fr = frames[c.ssrc]
        assert len(fr) >= NBLOCKS - 2
        bins = fr[0]["nfloat"]
        defined = slice(0, bins // 2) if c.ssrc == 701 else slice(0, bins)
        assert all(int(round(f["gain"])) == FFT_N and f["nfloat"] == bins for f in fr)      # the harness reports fft_n in `gain`
        shift = int(fr[-1]["bin_shift"] * FFT_N // (L + M - 1))                             # src/spectrum.c:347
        got = np.stack([np.asarray(f["pcm_f"], np.float64)[defined] for f in fr])
        steady = got[[i for i, f in enumerate(fr) if f["next_jobnum"] > SLACK + 3]]
        spread = np.abs(steady - np.median(steady, axis=0)).max()
        assert spread > 0 and steady.max() > 1e-4
        tol = 4 * spread
        cand = {k: welch_ref(ring, k * L, True, FFT_N, win, shift, bins, avg, 0.0)[0].astype(np.float64)[defined] for k in range(NBLOCKS + 1)}
        worst, on_boundary = 0.0, 0
        for i, f in enumerate(fr):
            j = int(f["next_jobnum"])
            near = [k for k in cand if abs(k - j) <= SLACK + 1]
            err = {k: np.abs(got[i] - cand[k]).max() for k in near}
            k = min(err, key=err.get)
            assert err[k] <= tol, (c.ssrc, i, j, k, err[k], tol)
            worst = max(worst, err[k]); seen += 1
            on_boundary += 1
        print("WELCH-REF ssrc %d shift %d: %d frames, every one on a block boundary within %d of its block; worst |diff| %.3g, reference's own spread %.3g, strongest bin %.3g"
              % (c.ssrc, shift, on_boundary, SLACK + 1, worst, spread, steady.max()))
    assert seen == sum(len(frames[c.ssrc]) for c in ch)
