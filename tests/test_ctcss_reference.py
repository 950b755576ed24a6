"""Pins tests/ctcss_oracle.py -- the checker of every device test of the PL tone decoder pool -- to the reference's own src/ctcss.c.

tests/c/ref_ctcss_wrap.c #includes the reference's ctcss.c where it lies (main renamed; setup_mcast_in, select and recvfrom redirected to a
feeder that makes RTP packets of a tenth of a block -- 480 samples at 24 kHz -- from a file of big-endian samples) and records, after every tenth
packet, the session's strongest_tone_index, strongest_tone_energy and current_pl_tone at full precision.  It is compiled into tmp_path as a
program with the reference's release flags (oracle/Makefile's REF_CFLAGS) together with the reference's filter window misc sched sincospi
osc gauss rtp and the oracle's FFT provider (oracle/_build/fftw_shim.o, dft_ref.o); the reference's transform runs in the caller's thread
(N_worker_threads = 0, for the reason tests/c/ref_packetd_wrap.c gives).

Input: instance 0 of tests/test_gpu_ctcss.py's scenario at 24 and 8 kHz and at the five rates of tests/test_gpu_ctcss_rates.py (11025, 22050, 40960,
16000 and 9999 Hz; the feeder is told how many packets make a block where ten do not divide it), on the reference's float64 transform and on its float32 one
(oracle_fft_set_precision).  On every block the restatement's index and sticky tone equal the reference's, and the energy is within the
device rule of tests/test_gpu_ctcss.py: 1e-6 relative to the block's largest energy, or 4 x the f32 twin's own distance on that block where
that is larger (the reference's float32 transform is compared with the restatement's float64 run, like a device).  The input condition of
tests/test_gpu_ctcss.py is asserted first."""
import os
import re
import subprocess

import numpy as np
import pytest

import afsk_oracle as ao
import ctcss_oracle as co
import oracle_lib as ol
import test_gpu_ctcss as tg
import test_gpu_ctcss_rates as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE = os.path.join(ROOT, "oracle")


def makefile_var(name):
    with open(os.path.join(ORACLE, "Makefile")) as f:
        m = re.search(r"^%s\s*\??=\s*(.*)$" % name, f.read(), re.M)
    return m.group(1).strip()


REF = os.environ.get("REF", makefile_var("REF"))
needs_ref = pytest.mark.skipif(not os.path.isfile(os.path.join(REF, "ctcss.c")), reason="the reference tree is not here")


@pytest.fixture(scope="module")
def refctcss(tmp_path_factory):
    ol.build()                          # oracle/_build/fftw_shim.o and dft_ref.o
    work = str(tmp_path_factory.mktemp("refctcss"))
    prog = os.path.join(work, "ref_ctcss")
    srcs = [os.path.join(REF, f + ".c") for f in "filter window misc sched sincospi osc gauss rtp".split()] + [os.path.join(ROOT, "tests", "c", "ref_ctcss_wrap.c")]
    git = ['-DGIT_%s="none"' % k for k in ("HASH", "BRANCH", "DATE", "VERSION", "REMOTE_URL")]
    # compiled with the reference's flags, linked without them (as oracle/Makefile links _ref/ and tests/test_afsk_reference.py its library)
    subprocess.run(["gcc"] + makefile_var("REF_CFLAGS").split() + git + ["-I", os.path.join(ORACLE, "shims"), "-iquote", REF, "-ffunction-sections",
                    "-fdata-sections", "-c"] + srcs, check=True, cwd=work)
    objs = [os.path.join(work, os.path.basename(f)[:-2] + ".o") for f in srcs]
    subprocess.run(["gcc", "-o", prog] + objs + [os.path.join(ORACLE, "_build", "fftw_shim.o"), os.path.join(ORACLE, "_build", "dft_ref.o"),
                    "-Wl,--gc-sections", "-l:libbsd.so.0", "-lm", "-lpthread"], check=True)
    return prog


def reference_records(prog, path, samprate, f32, out, per_block=10):
    r = subprocess.run([prog, path, str(int(samprate)), str(int(f32)), out, str(per_block)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-1500:])
    with open(out) as f:
        rows = [line.split() for line in f]
    return [(int(a), float(b), float(c)) for a, b, c in rows]


# the rates of tests/test_gpu_ctcss_rates.py: (rate, packets a block).  The feeder's packet must divide L: ten does not divide 2205 (nine packets of
# 245 samples do), and a sixteenth of 8192 is 512 samples, 1024 bytes, inside the reference's packet buffer
RATES = {"11k": 9, "22k": 10, "41k": 16, "16k": 10, "9999": 10}


@needs_ref
@pytest.mark.parametrize("shape", list(tg.SHAPES) + list(RATES))
def test_the_restatement_s_decisions_equal_the_reference_s(refctcss, tmp_path, shape):
    if shape in RATES:
        fs, per_block = tr.RATES[shape][0], RATES[shape]
        blocks, mine, twin = tr.scenario(shape)[0], tr.restatement(shape, False)[0], tr.restatement(shape, True)[0]
    else:
        fs, per_block = tg.SHAPES[shape], 10
        blocks, mine, twin = tg.scenario(shape)[0], tg.restatement(shape, False)[0], tg.restatement(shape, True)[0]
    floor, smallest, where = tg.input_condition(mine, twin, shape)
    path = str(tmp_path / "inst0.s16be")
    ao.to_wire(blocks.reshape(-1), big_endian=True).tofile(path)
    for f32 in (False, True):
        ref = reference_records(refctcss, path, fs, f32, str(tmp_path / ("records%d.txt" % f32)), per_block)
        assert len(ref) == len(mine) == 175
        worst = 0.0
        for blk, ((index, energy, current), r, t) in enumerate(zip(ref, mine, twin)):
            assert index == r["tone_index"], (shape, f32, blk, index, r["tone_index"])
            assert current == (co.TONES[r["current_index"]] if r["current_index"] >= 0 else 0.0), (shape, f32, blk, current, r["current_index"])
            top = float(r["energies"].max())
            if top == 0.0:
                assert energy == co.THRESHOLD
                continue
            lim = max(1e-6, 4 * float(np.abs(t["energies"] - r["energies"]).max()) / top)
            e = abs(energy - r["energy"]) / top
            worst = max(worst, e / lim)
            assert e <= lim, (shape, f32, blk, energy, r["energy"], e, lim)
        print("%s, the reference's %s transform: 175 blocks equal; FLOOR %.3g, smallest margin %.3g (block %d); worst measured / allowed %.2f"
              % (shape, "float32" if f32 else "float64", floor, smallest, where, worst))


def test_the_bank_steps_as_afsk_oracle_s_oscillators_do():
    """ctcss_oracle.Bank against afsk_oracle.Osc, bit for bit, across the first renormalisation (step 16384): the first, the last and the 150 Hz
    tone, whose step is exactly 1"""
    tones = (co.TONES[0], co.PL_SHIFT, co.TONES[-1])
    bank = co.Bank(tones).run(ao.RENORM + 200)
    for k, f in enumerate(tones):
        assert np.array_equal(bank[k], ao.Osc((f - co.PL_SHIFT) / co.PL_SAMPRATE).run(ao.RENORM + 200)), f
    assert (bank[1] == 1).all()
