"""Driver for tests/c/mini_radiod.c: the reference's own radio.c / linear.c / fm.c on two filter.h implementations.

TEST INFRASTRUCTURE.  Builds the channel table (share/presets.conf's presets, restated here as key=value lists because
loadpreset() needs iniparser), synthesises the A/D samples, runs a mini-radiod binary and parses what its send_output() captured;
compare() is the A/B comparator of the two links.
"""
import os
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_EXE = os.path.join(ROOT, "oracle", "_ref", "mini_radiod_ref")           # the reference's filter.c (checker)
HIP_EXE = os.path.join(ROOT, "oracle", "_ref", "mini_radiod_hip")           # libka9q_filter_hip.so (product)
CALLER_OBJS = os.path.join(ROOT, "oracle", "_ref", "mini_radiod")           # the caller objects both are linked from (oracle/Makefile)

# /root/reference/share/presets.conf, the sections this test uses (line numbers of the section headers)
PRESETS = {
    "usb": "demod=linear samprate=12000 low=50 high=3000 filter2=0 pll=no square=no mono=yes shift=0 envelope=no conj=no hang-time=1.1 recovery-rate=20",   # :236
    "lsb": "demod=linear samprate=12000 low=-3000 high=-50 filter2=0 pll=no square=no mono=yes shift=0 envelope=no conj=no hang-time=1.1 recovery-rate=20",  # :254
    "cwu": "demod=linear samprate=12000 low=-200 high=200 filter2=4 shift=500 hang-time=0.2 pll=no square=no mono=yes envelope=no",                        # :196
    "cwl": "demod=linear samprate=12000 low=-200 high=200 filter2=4 shift=-500 hang-time=0.2 pll=no square=no mono=yes envelope=no conj=no",               # :217
    "am": "demod=linear samprate=12000 low=-5000 high=5000 filter2=0 recovery-rate=50 hang-time=0 envelope=yes pll=no square=no mono=yes shift=0",          # :120
    "sam": "demod=linear samprate=12000 low=-5000 high=5000 filter2=0 recovery-rate=50 hang-time=0 pll=yes square=no mono=yes squelch-open=8 squelch-close=7 shift=0",  # :139
    "ame": "demod=linear samprate=12000 low=-100 high=5000 filter2=0 recovery-rate=50 hang-time=0 pll=yes square=no mono=yes squelch-open=8 squelch-close=7 shift=0",  # :159
    "iq": "demod=linear samprate=12000 low=-5000 high=5000 filter2=0 stereo=yes pll=no shift=0 envelope=no conj=no hang-time=1.1 recovery-rate=20 agc=yes",  # :179
    "dsb": "demod=linear samprate=12000 low=-5000 high=5000 filter2=0 square=yes pll=no mono=yes shift=0 envelope=no conj=no hang-time=1.1",               # :272
    "fm": "demod=fm samprate=24000 low=-8000 high=8000 filter2=0 deemph-tc=0 deemph-gain=0 threshold-extend=no pll=no square=no mono=yes shift=0 conj=no",  # :67
    "nfm": "demod=fm samprate=24000 low=-6250 high=6250 filter2=0 deemph-tc=0 deemph-gain=0 threshold-extend=no pll=no square=no mono=yes shift=0 conj=no",  # :84
    "wfm": "demod=wfm samprate=384000 low=-110000 high=110000 filter2=0 threshold-extend=no deemph-tc=75.0 deemph-gain=0 pll=no square=no mono=yes shift=0 conj=no squelch-open=10 squelch-close=6 snr-squelch=no",  # :101
    "pm": "demod=fm samprate=24000 low=-8000 high=8000 filter2=0 squelch-tail=0 threshold-extend=yes deemph-tc=530.5 deemph-gain=12.0 pll=no square=no mono=yes shift=0",  # :7
}

HDR = struct.Struct("<4I8i4I12d")
HDR_FIELDS = ("ssrc call next_jobnum block_drops frames channels mute isnull encoding bin_shift pll_lock silent "
              "rtp_timestamp pcm_bytes nfloat olen n0 bb_power out_power gain pll_snr fm_snr foffset pdeviation cphase remainder "
              "tone_deviation tune_freq").split()


class Channel:
    def __init__(self, ssrc, freq, preset, extra="", signal=None):
        self.ssrc, self.freq, self.preset, self.extra = ssrc, float(freq), preset, extra
        self.signal = signal or {}

    def line(self):
        return "%d %.3f %s %s" % (self.ssrc, self.freq, PRESETS[self.preset], self.extra)


def standard_channels(fs=1.296e6):
    """48 channels of every kind of preset the reference's linear and FM demodulators serve, with a signal for each; the numbered
    cases the round-5 review asked for: one filter2 = 4 (the CW presets bring it), one ISB, one retune and one set_filter mid-stream."""
    ch = []
    kinds = ["usb", "lsb", "cwu", "am", "sam", "iq", "fm", "pm", "nfm", "dsb", "ame", "cwl"]
    f = 30000.0
    ssrc = 100
    for i in range(48):
        k = kinds[i % len(kinds)]
        extra = ""
        sig = {"kind": k, "amp": 0.02 + 0.004 * (i % 5)}
        if i % 3 == 1:
            extra += " encoding=f32le"
        if k in ("usb", "lsb") and i >= 24:
            extra += " snr-squelch=yes"
        ch.append(Channel(ssrc, f + 7.3 * i, k, extra.strip(), sig))        # off the bin raster: remainder != 0 -> the fine oscillator turns
        f += 11960.0 + 40.0 * (i % 4)
        ssrc += 1
    # an ISB channel (src/radio_status.c:630-637: stereo + filter2 forced on; conj = the preset key for filter2.out.isb)
    ch[5].extra = (ch[5].extra + " conj=yes filter2=1").strip()
    # a retune mid-stream (RADIO_FREQUENCY, src/radio_status.c:241): 3 bins + 11 Hz up at frame 9 -- the signal is wide enough to stay in the passband
    ch[0].extra = (ch[0].extra + " retune=9:%.3f" % (ch[0].freq + 131.0)).strip()
    ch[12].extra = (ch[12].extra + " retune=14:%.3f" % (ch[12].freq - 877.0)).strip()
    # new filter edges mid-stream (LOW_EDGE / HIGH_EDGE -> set_channel_filter -> set_filter, src/radio_status.c:640-659)
    ch[3].extra = (ch[3].extra + " edges=11:-2500:2500").strip()
    ch[6].extra = (ch[6].extra + " edges=7:-6000:6000").strip()
    ch[2].extra = (ch[2].extra + " edges=3:-150:150").strip()         # on the filter2 = 4 channel: rebuilds filter2 as well
    # an FM channel with a PL tone squelch whose tone is present, one whose tone is absent, one with no signal at all (squelch closed)
    ch[18].extra = (ch[18].extra + " tone=100.0").strip(); ch[18].signal["pl"] = 100.0
    ch[30].extra = (ch[30].extra + " tone=123.0").strip()
    ch[42].signal["amp"] = 0.0
    ch[7].signal["amp"] = 0.0                                          # a pm channel on noise only
    ch[16].signal["amp"] = 0.0                                         # a sam channel on noise only: the PLL never locks, squelch closed
    return ch


def synthesise(channels, fs, L, nblocks, seed=5, noise=0.002):
    """A/D samples: per channel a signal of its kind at its carrier + white noise.  float32, [nblocks * L]."""
    n = nblocks * L
    t = np.arange(n) / fs
    rng = np.random.default_rng(seed)
    x = noise * rng.standard_normal(n)
    for i, c in enumerate(channels):
        a, k, f = c.signal.get("amp", 0.0), c.signal.get("kind", ""), c.freq
        if a == 0.0:
            continue
        if k not in ("fm", "pm", "nfm", "wfm"):
            # slow fading, a different rate and phase per channel: with a STATIONARY signal the block AGC of src/linear.c:205-238 sits exactly
            # on its own decision boundary (after an attack, amplitude x gain == headroom to the last bit, and the next block's "above or
            # below?" is decided by rounding: 1 dB of gain per block either way) -- measured: the reference against itself on a float32
            # transform then differs by 39 % in gain.  Real signals are never stationary to 1e-7; neither are these.
            a = a * (1.0 + 0.35 * np.sin(2 * np.pi * (1.1 + 0.13 * (i % 7)) * t + 0.7 * i))
        if k in ("usb", "iq"):
            x += a * (np.cos(2 * np.pi * (f + 700.0) * t) + 0.6 * np.cos(2 * np.pi * (f + 1900.0) * t + 0.3))
        elif k == "ame":      # carrier + weak upper sideband: the lock detector takes sideband power in quadrature for noise
            x += 2 * a * np.cos(2 * np.pi * f * t + 0.2) + 0.1 * a * np.cos(2 * np.pi * (f + 700.0) * t)
        elif k == "lsb":
            x += a * (np.cos(2 * np.pi * (f - 600.0) * t) + 0.5 * np.cos(2 * np.pi * (f - 2100.0) * t + 1.0))
        elif k in ("cwu", "cwl"):
            key = ((t * 12.5).astype(np.int64) % 3 != 2).astype(np.float64)      # 80 ms elements, on-on-off
            x += a * key * np.cos(2 * np.pi * f * t)
        elif k in ("am", "sam"):
            x += a * (1.0 + 0.5 * np.cos(2 * np.pi * 1000.0 * t)) * np.cos(2 * np.pi * f * t + 0.4)
        elif k == "dsb":
            x += a * np.cos(2 * np.pi * 800.0 * t) * np.cos(2 * np.pi * f * t + 0.9)
        elif k == "wfm":      # broadcast FM: L + R, a 19 kHz pilot at 9 %, L - R on the suppressed 38 kHz subcarrier; 67.5 kHz peak deviation
            left, right = np.sin(2 * np.pi * 1000.0 * t), 0.6 * np.sin(2 * np.pi * 2600.0 * t + 0.5)
            mpx = 0.45 * (left + right) + 0.45 * (left - right) * np.sin(2 * np.pi * 38000.0 * t) * c.signal.get("stereo", 1.0) + 0.09 * np.sin(2 * np.pi * 19000.0 * t) * c.signal.get("stereo", 1.0)
            x += a * np.cos(2 * np.pi * f * t + 2 * np.pi * 75000.0 * np.cumsum(mpx) / fs)
        elif k in ("fm", "pm", "nfm"):
            dev, fmod = 2500.0, 1000.0
            ph = 2 * np.pi * f * t + (dev / fmod) * np.sin(2 * np.pi * fmod * t)
            pl = c.signal.get("pl")
            if pl:
                ph = ph + (500.0 / pl) * np.sin(2 * np.pi * pl * t)
            x += a * np.cos(ph)
    return x.astype(np.float32)


def run(exe, workdir, channels, x, fs, L, M, nblocks, paced=0, slack=2, env=None, timeout=900):
    """x: float32 samples of a real front end, or complex64 of a complex one"""
    os.makedirs(workdir, exist_ok=True)
    with open(os.path.join(workdir, "cfg.txt"), "w") as f:
        f.write("%.1f %d %d %d %d %d %d%s\n" % (fs, L, M, nblocks, len(channels), paced, slack, " complex" if np.iscomplexobj(x) else ""))
        for c in channels:
            f.write(c.line() + "\n")
    x.tofile(os.path.join(workdir, "in.f32"))
    r = subprocess.run([exe, workdir], capture_output=True, text=True, timeout=timeout, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    meta = open(os.path.join(workdir, "meta.txt")).read().split()
    meta = dict(zip(meta[::2], meta[1::2]))
    assert int(meta["hdr_bytes"]) == HDR.size
    return parse(os.path.join(workdir, "frames.bin")), meta, r.stderr


def parse(path):
    """-> {ssrc: [frame dicts in call order]}; a frame carries its header fields, 'pcm_f' (the float buffer handed to send_output) and
    'pcm' (the packed bytes of the channel's encoding), both None for muted / NULL frames"""
    buf = open(path, "rb").read()
    out, o = {}, 0
    while o < len(buf):
        h = dict(zip(HDR_FIELDS, HDR.unpack_from(buf, o))); o += HDR.size
        if h["nfloat"]:
            h["pcm_f"] = np.frombuffer(buf, np.float32, h["nfloat"], o).copy(); o += 4 * h["nfloat"]
            h["pcm"] = np.frombuffer(buf, np.uint8, h["pcm_bytes"], o).copy(); o += h["pcm_bytes"]
        else:
            h["pcm_f"] = h["pcm"] = None
        out.setdefault(h["ssrc"], []).append(h)
    return out


S16LE, S16BE, F32LE = 1, 2, 4       # src/rtp.h:27-41 enum encoding


DISCRETE = ("call", "next_jobnum", "block_drops", "frames", "channels", "mute", "isnull", "encoding", "bin_shift", "pll_lock",
            "silent", "rtp_timestamp", "pcm_bytes", "nfloat", "olen")


def diff(ref, got, upto=None, settle=None):
    """Frame by frame.  Everything discrete -- frame kinds, mute / squelch flags, PLL lock, RTP timestamps, bin shifts, block_drops, the
    tuning -- is compared for equality: st["agree"] = the number of leading frames of the channel on which the two runs agree in all of
    it (== st["frames"] when they never part), st["parted"] = (frame, field, value, value) where they first do not.  The continuous
    outputs are measured over those leading frames (and at most upto[ssrc] of them): "float_rel" worst relative L2 of a frame's float PCM
    (frames above 1e-3 of the channel's loudest), "n0_rel" / "bb_power_rel" / "gain_rel" worst relative differences, "lsb_frac" share of
    the int16 PCM samples that differ, "lsb_max" by how many LSB at most.  settle[ssrc] = leading frames of that channel whose continuous
    outputs are not measured (the discrete ones are): demod_wfm()'s discriminator takes the argument of a filter's near-zero precursor in the
    very first block -- rounding noise, in the reference too -- and its composite filter (2:1 overlap) remembers that for two more blocks."""
    assert sorted(ref) == sorted(got), (sorted(ref)[:5], sorted(got)[:5])
    out = {}
    for ssrc in sorted(ref):
        A, B = ref[ssrc], got[ssrc]
        assert len(A) == len(B), (ssrc, len(A), len(B))
        peak = max([float(np.sqrt(np.mean(a["pcm_f"].astype(np.float64) ** 2))) for a in A if a["pcm_f"] is not None] or [0.0])
        st = {"float_rel": 0.0, "float_abs_over_peak": 0.0, "n0_rel": 0.0, "bb_power_rel": 0.0, "gain_rel": 0.0, "lsb_frac": 0.0, "lsb_max": 0, "frames": len(A),
              "agree": len(A), "parted": None, "data": 0, "null": 0}
        nsamp = ndiff = 0
        for idx, (a, b) in enumerate(zip(A, B)):
            if upto is not None and idx >= upto[ssrc]:
                break
            bad = [k for k in DISCRETE if a[k] != b[k]]
            if not bad and not (a["tune_freq"] == b["tune_freq"] and (a["remainder"] == b["remainder"] or (np.isnan(a["remainder"]) and np.isnan(b["remainder"])))):
                bad = ["tune_freq"]
            if bad:
                st["agree"] = idx; st["parted"] = (idx, bad[0], a[bad[0]], b[bad[0]])
                break
            if settle and idx < settle.get(ssrc, 0):
                st["null" if a["pcm_f"] is None else "data"] += 1
                continue
            for k in ("n0", "bb_power", "gain"):
                if (a[k] == 0 and b[k] == 0) or (np.isnan(a[k]) and np.isnan(b[k])):
                    continue
                st[k + "_rel"] = max(st[k + "_rel"], abs(a[k] - b[k]) / max(abs(a[k]), 1e-300))
            if a["pcm_f"] is None:
                st["null"] += 1
                continue
            st["data"] += 1
            fa, fb = a["pcm_f"].astype(np.float64), b["pcm_f"].astype(np.float64)
            err = float(np.sqrt(np.mean((fa - fb) ** 2))); rms = float(np.sqrt(np.mean(fa ** 2)))
            st["float_abs_over_peak"] = max(st["float_abs_over_peak"], err / max(peak, 1e-300))
            if rms > 1e-3 * peak:
                st["float_rel"] = max(st["float_rel"], err / rms)
            if a["encoding"] in (S16BE, S16LE):
                dt = ">i2" if a["encoding"] == S16BE else "<i2"
                d = np.abs(a["pcm"].view(dt).astype(np.int32) - b["pcm"].view(dt).astype(np.int32))
                st["lsb_max"] = max(st["lsb_max"], int(d.max(initial=0)))
                nsamp += d.size; ndiff += int((d != 0).sum())
        st["lsb_frac"] = ndiff / nsamp if nsamp else 0.0
        out[ssrc] = st
    return out


def summary(d):
    keys = ("float_rel", "float_abs_over_peak", "n0_rel", "bb_power_rel", "gain_rel", "lsb_frac", "lsb_max")
    s = {k: max(v[k] for v in d.values()) for k in keys}
    s.update({k + "_median": float(np.median([v[k] for v in d.values()])) for k in ("float_rel", "n0_rel", "bb_power_rel")})
    s["data"] = sum(v["data"] for v in d.values()); s["null"] = sum(v["null"] for v in d.values())
    s["frames"] = sum(v["frames"] for v in d.values()); s["frames_in_agreement"] = sum(v["agree"] for v in d.values())
    s["parted"] = {k: v["parted"] for k, v in d.items() if v["parted"]}
    return s


def check(d, d_self=None, pll=(), float_tol=1e-5, n0_tol=1e-5, lsb_frac=1e-3, factor=4.0, n0_flip=0.0):
    """The bar of the round-5 review -- float PCM within 1e-5 relative L2, int16 PCM at most 1 LSB apart on at most 0.1 % of the samples,
    sig.n0 / bb_power within 1e-5 -- held wherever the REFERENCE ITSELF holds it.  d_self = diff(reference on a float64 transform,
    reference on a float32 transform) over the same samples says where it does not (measured, tests/test_mini_radiod.py):
      * estimate_noise() averages the bins under a threshold derived from a quantile (src/radio.c:1840-1864): one bin crossing that
        threshold moves n0 by ~1/bins_averaged however small the rounding difference that pushed it (reference vs itself: up to 1.2e-3,
        median 7e-7) -- n0 is held to `factor` x the reference's own worst spread, and its MEDIAN over the channels to n0_tol;
      * a PLL that is still acquiring amplifies its input differences (the coherent presets sam / ame / dsb: reference vs itself up to
        6.7e-4 in the first frames) -- channels in `pll` are held to `factor` x the reference's own worst spread on those channels;
      * an int16 sample flips when the float error crosses a rounding boundary: a share of 2 x |error in LSB| of the samples, 0.1-0.2 % for
        a full-scale signal at float32's 2.5e-7 (reference vs itself: 0.17 %) -- held to `factor` x the reference's own worst share;
    everything else (float PCM of the other channels, bb_power, gain) to the review's figures."""
    # Discrete outputs: the link under test must agree with the reference at least as long as the reference agrees with ITSELF on the other
    # transform (a squelch or lock decision taken on a marginal SNR -- a PLL still acquiring -- flips with the rounding of its input in the
    # reference too; from there on the two runs of that channel are different histories).  Without d_self: on every frame.
    for ssrc, st in d.items():
        need = d_self[ssrc]["agree"] if d_self else st["frames"]
        assert st["agree"] >= need, (ssrc, "discrete outputs part at frame", st["parted"], "the reference agrees with itself up to frame", need)
    if d_self:
        held = sum(v["agree"] for v in d_self.values()); total = sum(v["frames"] for v in d_self.values())
        assert held >= 0.95 * total, ("the reference itself is unstable on too much of this input to test with", held, total)
    own = summary(d_self) if d_self else None
    own_pll = max([d_self[s]["float_rel"] for s in pll] + [d_self[s]["float_abs_over_peak"] for s in pll] + [0.0]) if d_self else 0.0
    # the other channels: 1e-5 at the small geometry; at BASELINE's full rates (N = 1.62 M / 3.24 M, a hundred strong lines in the window) a float32
    # transform's error floor in a quiet channel is set by the strongest line of the WINDOW, not by what the channel holds --
    # the reference on a float32 transform shows it too (config 3: up to 8.7e-5, median 4e-6), and that spread is the yardstick
    own_plain = max([max(v["float_rel"], v["float_abs_over_peak"]) for k, v in d_self.items() if k not in pll] + [0.0]) if d_self else 0.0
    lim_n0 = max(n0_tol, n0_flip, factor * own["n0_rel"]) if own else max(n0_tol, n0_flip)      # n0_flip: what ONE bin crossing the threshold may move n0 by, where the caller can say (the median stays at n0_tol)
    lim_bb = max(n0_tol, factor * own["bb_power_rel"]) if own else n0_tol
    lim_lsb = max(lsb_frac, factor * own["lsb_frac"]) if own else lsb_frac
    lim_gain = max(10 * n0_tol, factor * own["gain_rel"]) if own else 10 * n0_tol      # the AGC's threshold follows n0 (src/linear.c:196-204)
    for ssrc, st in d.items():
        lim_f = max(float_tol, factor * own_pll) if ssrc in pll else max(float_tol, factor * own_plain)
        assert st["float_rel"] <= lim_f, (ssrc, "float_rel", st["float_rel"], lim_f)
        assert st["float_abs_over_peak"] <= lim_f, (ssrc, "float_abs_over_peak", st["float_abs_over_peak"], lim_f)
        assert st["n0_rel"] <= lim_n0, (ssrc, "n0_rel", st["n0_rel"], lim_n0)
        assert st["bb_power_rel"] <= lim_bb, (ssrc, "bb_power_rel", st["bb_power_rel"], lim_bb)
        assert st["gain_rel"] <= lim_gain, (ssrc, "gain_rel", st["gain_rel"], lim_gain)
        assert st["lsb_max"] <= 1, (ssrc, "lsb_max", st["lsb_max"])
        assert st["lsb_frac"] <= lim_lsb, (ssrc, "lsb_frac", st["lsb_frac"], lim_lsb)
    s = summary(d)
    assert s["n0_rel_median"] <= max(n0_tol, 2 * own["n0_rel_median"] if own else 0) and s["float_rel_median"] <= max(float_tol, 2 * own["float_rel_median"] if own else 0), s
    s["limits"] = {"float_rel": max(float_tol, factor * own_plain), "float_rel_pll_channels": max(float_tol, factor * own_pll), "n0_rel": lim_n0, "bb_power_rel": lim_bb,
                   "lsb_frac": lim_lsb, "gain_rel": lim_gain}
    return s


def compare(ref, got, **kw):
    return check(diff(ref, got), None, **kw)


# ---- BASELINE.json's own configurations through the reference's callers (config 2: 64.8 MS/s, 256 NBFM channels; config 3: 129.6 MS/s,
# 1024 mixed usb / cw / iq channels) -- the channel rasters of bench.py's workloads
def spectral_synth(lines, fs, n, noise, seed):
    """n real samples = white noise + the spectral lines [(Hz, amplitude, phase)], every frequency rounded to a bin of the whole run (one
    inverse transform instead of one cosine of n samples per line: 10^3 lines over 4 x 10^7 samples)."""
    S = np.zeros(n // 2 + 1, np.complex128)
    for f, a, ph in lines:
        k = int(round(f * n / fs))
        if 0 < k < n // 2:
            S[k] += 0.5 * a * n * np.exp(1j * ph)
    x = np.fft.irfft(S, n)
    del S
    rng = np.random.default_rng(seed)
    x += noise * rng.standard_normal(n)
    return x.astype(np.float32)


def config3_channels(nch=1024, every=8):
    """bench.py's channel_plan_config3 raster (1 MHz + i x 60 kHz + (i mod 40) Hz; thirds usb / cw / iq) as radiod channels: the usb and iq
    presets, and the cwu preset (filter2 = 4, +500 Hz shift) for the CW third; S16BE and F32LE; a signal on every `every`-th channel
    (two tones with slow fading sidebands -- see synthesise() on why nothing here is stationary), noise on the others."""
    ch, lines = [], []
    for i in range(nch):
        f = 1e6 + (i % 1040) * 60e3 + (i % 40)
        k = ("usb", "cwu", "iq")[i % 3]
        extra = "encoding=f32le" if i % 5 == 1 else ""
        ch.append(Channel(1000 + i, f, k, extra, {"kind": k}))
        if i % every == 0:
            a = 0.004 + 0.001 * (i % 3)
            tones = {"usb": [(700.0, 1.0), (1900.0, 0.6)], "cwu": [(0.0, 1.0)], "iq": [(-1300.0, 1.0), (2100.0, 0.7)]}[k]
            for df, rel in tones:
                ph = 0.37 * i + df * 1e-3
                lines.append((f + df, a * rel, ph))
                lines.append((f + df + 3.0 + 0.2 * (i % 5), 0.17 * a * rel, ph + 1.0))      # +- a few Hz: a slow beat = fading
                lines.append((f + df - 3.0 - 0.2 * (i % 5), 0.17 * a * rel, ph - 0.4))
    return ch, lines


def config2_channels(nch=256, every=4):
    """bench.py's channel_plan_config2 raster (10 MHz + i x 12.5 kHz) as 12 kHz NBFM channels (the fm preset at samprate 12 k, +-5 kHz);
    every `every`-th carries a carrier frequency-modulated by a 1 kHz tone (beta 1.5: the Bessel lines n = -7..7), the others noise."""
    from scipy.special import jv
    ch, lines = [], []
    fm12 = "samprate=12000 low=-5000 high=5000"
    for i in range(nch):
        f = 10e6 + i * 12.5e3
        k = "pm" if i % 3 == 2 else "fm"
        ch.append(Channel(2000 + i, f, k, fm12 + (" encoding=f32le" if i % 5 == 1 else "") + (" threshold-extend=yes" if i % 2 else ""), {"kind": k}))
        if i % every == 0:
            a, beta, fmod = 0.01, 1.5, 1000.0 + 10.0 * (i % 7)
            for n in range(-7, 8):
                lines.append((f + n * fmod, a * float(jv(n, beta)), 0.3 * i + (0.0 if n >= 0 or n % 2 == 0 else np.pi) * 0 + 0.0))
    return ch, lines


def config1_channels():
    """BASELINE config 1: sig_gen complex 2.4 MS/s, ONE IQ-mode channel (the reference's own CPU-runnable plumbing case; bench.py's
    workload_for(1): the channel at 100 kHz) -- plus one on the negative side of the complex spectrum, which a real front end cannot have."""
    ch = [Channel(3000, 100e3 + 3.7, "iq", "", {"kind": "iq"}), Channel(3001, -412e3 - 11.3, "usb", "encoding=f32le", {"kind": "usb"})]
    lines = [(100e3 + 3.7 - 1300.0, 0.02, 0.3), (100e3 + 3.7 + 2100.0, 0.014, 1.1), (100e3 + 3.7 + 2103.0, 0.004, 0.2),
             (-412e3 - 11.3 + 700.0, 0.02, 0.5), (-412e3 - 11.3 + 1900.0, 0.012, 2.0), (-412e3 - 11.3 + 1903.5, 0.003, 0.9)]
    return ch, lines


def complex_synth(lines, fs, n, noise, seed):
    """n complex samples: lines [(Hz, amplitude, phase)] as complex exponentials (negative frequencies allowed) + complex white noise"""
    S = np.zeros(n, np.complex128)
    for f, a, ph in lines:
        S[int(round(f * n / fs)) % n] += a * n * np.exp(1j * ph)
    x = np.fft.ifft(S)
    rng = np.random.default_rng(seed)
    x += noise * (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2)
    return x.astype(np.complex64)


def config4_channels(nch=2000, every=10):
    """BASELINE config 4's shape on what one radiod can hold: 24 kHz channels (P = 600) on bench.py's channel_plan_config4 raster
    (0.5 MHz + i x 7.8 kHz), Nchannels = 2000 of them (src/radio.h:356) -- behind ONE master whose slaves the drop-in shards over
    KA9Q_HIP_DEVICES 1024 at a time.  iq preset at 24 kHz (stereo frames), +-10 kHz; a two-tone signal on every `every`-th channel."""
    ch, lines = [], []
    for i in range(nch):
        f = 0.5e6 + i * 7.8e3
        # (channels on noise alone run with a fixed gain: stationary noise parks the block AGC on its own decision boundary -- see synthesise() --
        #  and the reference then differs from ITSELF by tens of per cent in gain on a float32 transform, which says nothing about anybody's filter)
        ch.append(Channel(4000 + i, f, "iq", "samprate=24000 low=-10000 high=10000" + (" encoding=f32le" if i % 5 == 1 else "") + ("" if i % every == 0 else " agc=no gain=40"), {"kind": "iq"}))
        if i % every == 0:
            a = 0.004
            for df, rel in ((-2600.0, 1.0), (4100.0, 0.7)):
                ph = 0.21 * i + df * 1e-3
                lines.append((f + df, a * rel, ph)); lines.append((f + df + 3.1, 0.2 * a * rel, ph + 1.0)); lines.append((f + df - 2.7, 0.2 * a * rel, ph - 0.5))
    return ch, lines


def churn_channels():
    """the standard 48-channel table with channels LEAVING mid-stream (their lifetime runs out: downconvert() returns -1, demod_thread()
    cleans up, close_chan() frees the Channel_list slot -- delete_filter_output while the others run) and channels JOINING mid-stream
    (lookup_or_create_chan() / start_demod() from the front-end thread, as radiod creates a dynamic channel: create_filter_output on a
    running master, a bank that grows and is warmed while blocks flow; the newcomers take over the slots the leavers freed)."""
    ch = standard_channels()
    for i, life in ((1, 6), (8, 9), (13, 9), (20, 14), (27, 4), (33, 17), (40, 11), (46, 22)):
        ch[i].extra = (ch[i].extra + " life=%d" % life).strip()
    # the newcomers tune to where the leavers (and two stayers) are: the front end covers 0 ... 609 kHz (0.47 x fs) and the table fills it;
    # they listen to the signal that is already there (no signal of their own: amp 0), 13 Hz off so that their fine oscillators turn
    spots = [ch[i].freq for i in (27, 1, 8, 13, 20, 33, 40, 46, 4, 22)]
    for j, (start, kind) in enumerate(((7, "usb"), (7, "fm"), (10, "iq"), (12, "cwu"), (15, "am"), (15, "nfm"), (19, "lsb"), (24, "sam"), (24, "pm"), (26, "usb"))):
        c = Channel(300 + j, spots[j] + 13.0, kind, ("start=%d" % start) + (" encoding=f32le" if j % 3 == 0 else ""), {"kind": kind, "amp": 0.0})
        ch.append(c)
    return ch


def spectrum_channels():
    """demod_spectrum() (src/spectrum.c) next to a few ordinary channels: narrowband analysers (rbw <= 200 Hz: a COMPLEX slave whose block
    size follows from rbw and the bin count -- sizes no other caller asks for --, set_filter(), downconvert(), the analysis transform through
    plan_complex()) and one wideband analyser (rbw > 200 Hz: a SPECTRUM slave as block clock; its bin data come from an ASYNCHRONOUS read of
    the A/D ring and are not compared).  One poll per block; every reply's bin data is a frame."""
    ch = standard_channels()[:12]
    spec = "demod=spectrum poll=1"
    ch.append(Channel(500, 200000.0 + 3.0, "usb", spec + " rbw=50 bins=200 fft-avg=2", {"kind": "spectrum"}))          # fft_n 216 -> samprate 10.8 kHz, P = 270
    ch.append(Channel(501, 352000.0 - 7.0, "usb", spec + " rbw=100 bins=256 fft-avg=1", {"kind": "spectrum"}))         # fft_n 260/264.. whatever the search gives
    ch.append(Channel(502, 120000.0, "usb", spec + " rbw=25 bins=100 fft-avg=3", {"kind": "spectrum"}))
    ch.append(Channel(503, 300000.0, "usb", spec + " rbw=2000 bins=128 fft-avg=2", {"kind": "spectrum_wide"}))
    return ch


def spectrum_signal(channels, fs, l, nblocks, seed=31):
    """the standard synthetic band plus, around every analyser's centre, two fading lines for the bins to show"""
    x = synthesise(channels, fs, l, nblocks, seed=seed)
    t = np.arange(nblocks * l) / fs
    for c in channels:
        if str(c.signal.get("kind", "")).startswith("spectrum"):
            f0 = round(c.freq, -3)
            x += (0.01 * np.cos(2 * np.pi * (f0 + 1234.0) * t) * (1 + 0.3 * np.sin(2 * np.pi * 2.3 * t)) + 0.004 * np.cos(2 * np.pi * (f0 - 2345.0) * t + 1.0)).astype(np.float32)
    return x


def split_wideband(frames, channels):
    """(frames without the wideband analysers, the wideband analysers' frames)"""
    wide = {c.ssrc for c in channels if c.signal.get("kind") == "spectrum_wide"}
    return {k: v for k, v in frames.items() if k not in wide}, {k: v for k, v in frames.items() if k in wide}


WFM_GEOM = (2.592e6, 51840, 12961)      # N = 64,800: 40 Hz bins, 20 ms blocks, overlap 5


def wfm_channels():
    """demod_wfm() (src/wfm.c): for a 2.592 MS/s front end (WFM_GEOM): a stereo broadcast signal received by a stereo channel and by a mono channel (channels = 1: the pilot is not looked for),
    a multiplex WITHOUT pilot received by a stereo channel (falls back to mono), an empty channel (squelch shut), next to eight ordinary channels"""
    ch = [c for c in standard_channels() if c.freq < 150e3][:8]
    ch.append(Channel(600, 400000.0, "wfm", "stereo=yes", {"kind": "wfm", "amp": 0.05}))
    ch.append(Channel(601, 400000.0 + 1200.0, "wfm", "", {"kind": "none"}))
    ch.append(Channel(602, 740000.0, "wfm", "stereo=yes", {"kind": "wfm", "amp": 0.04, "stereo": 0.0}))
    ch.append(Channel(603, 1080000.0, "wfm", "stereo=yes", {"kind": "none"}))
    return ch


FUNCUBE_GEOM = (192e3, 3840, 961)        # a Funcube dongle's COMPLEX 192 kHz front end: N = 4800 -- small enough to look like radiod's filter2 to create_filter_input


def funcube_channels():
    """seven channels of a 192 kHz COMPLEX front end (N = 4800 <= 8192: the drop-in's undecided small master, which the first decimating slave turns into an
    engine), one of them a CW channel whose filter2 = 4 is a real pooled inline master next to it; slowly beating two-tone signals (no AGC knife-edge)"""
    spec = [(4000, 30e3 + 2.1, "usb", ""), (4001, -45e3 - 7.7, "lsb", "encoding=f32le"), (4002, 12e3 + 0.9, "cwu", ""), (4003, -70e3 + 5.3, "iq", ""),
            (4004, 60e3 - 3.3, "am", ""), (4005, -20e3 + 1.7, "fm", ""),
            # two antennas on I and Q (src/modes.c:547-556 -> src/radio.c:938-940 -> the beam form of the gather, src/filter.c:756-775).  NB: demod_thread() sets the weights
            # BEFORE the demodulator creates the filter output, and create_filter_output() resets them to (1, 0) (src/filter.c:341): what runs is "A input only" with
            # out.beam set -- in both links alike, which is the point
            (4006, 45e3 + 4.4, "usb", "beam=yes a-amp=1.0 a-phase=0 b-amp=0.7 b-phase=90")]
    ch, lines = [], []
    for k, (ssrc, f, preset, extra) in enumerate(spec):
        ch.append(Channel(ssrc, f, preset, extra, {"kind": preset}))
        if preset == "fm":
            continue                                   # noise only: the squelch stays shut
        off = {"usb": 900.0, "lsb": -1100.0, "cwu": 0.0, "iq": 1500.0, "am": 0.0}[preset]
        lines += [(f + off, 0.02 + 0.002 * k, 0.3 + k), (f + off + 3.0 + 0.5 * k, 0.006, 1.1 * k)]
        if preset == "am":
            lines += [(f + 1000.0, 0.005, 0.2), (f - 1000.0, 0.005, 0.9)]
    return ch, lines


def _as_switch(frame, kv):
    """a preset's key=value list as the switch=frame:key~value,... command of tests/c/mini_radiod.c"""
    return "switch=%d:%s" % (frame, ",".join(t.replace("=", "~") for t in kv.split()))


def switch_channels():
    """what `control` does to a running channel (src/radio_status.c:168-181 PRESET, :215-230 OUTPUT_SAMPRATE, :310-319 DEMOD_TYPE): the decoder asks for a RESTART when
    the sample rate or the demodulator changed -- the channel's filter output is deleted and created again at the new size on the running master, by the same
    thread on the same struct -- and for new filters otherwise (a CW preset on a USB channel: filter2 appears mid-stream)"""
    base = [c for c in standard_channels() if c.preset in ("usb", "lsb", "am", "iq")][:6]
    ch = []
    for i, c in enumerate(base):
        ch.append(Channel(700 + i, c.freq, c.preset, c.extra.replace("snr-squelch=yes", "").strip(), dict(c.signal)))
    ch[0].extra = (ch[0].extra + " " + _as_switch(8, "samprate=24000")).strip()                       # usb at 12 kHz -> 24 kHz: P 300 -> 600
    ch[1].extra = (ch[1].extra + " " + _as_switch(10, PRESETS["fm"])).strip()                          # lsb -> the fm preset: another demodulator, another size
    ch[2].extra = (ch[2].extra + " " + _as_switch(12, PRESETS["cwu"])).strip()                         # -> cwu: same rate and demodulator, new edges + filter2 = 4 appears
    ch[3].extra = (ch[3].extra + " " + _as_switch(9, PRESETS["usb"]) + " " + _as_switch(21, "samprate=8000")).strip()     # twice: preset, then 8 kHz (P = 200)
    ch[4].extra = (ch[4].extra + " " + _as_switch(7, "conj=yes")).strip()                               # INDEPENDENT_SIDEBAND on a running usb channel: stereo, filter2 forced on (a pooled inline master appears)
    return ch


def beam_handover_channels():
    """the funcube table with its beam channel created mid-stream (so it is the LAST of its bank), one more plain channel created behind it, and the beam channel
    leaving before the end: delete_filter_output moves the last slave into the freed index -- where the device still holds the leaver's beam flag and weights
    (round 6: the plain channel inherited them until the host's record of what is uploaded there was invalidated)"""
    ch, lines = funcube_channels()
    beam = ch[-1]
    beam.extra += " start=3 life=10"
    ch.append(Channel(4007, -33e3 + 2.2, "usb", "start=6", {"kind": "usb"}))
    lines += [(-33e3 + 2.2 + 900.0, 0.02, 0.4), (-33e3 + 2.2 + 904.5, 0.006, 1.9)]
    return ch, lines
