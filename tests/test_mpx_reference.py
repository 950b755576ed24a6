"""Pins tests/mpx_oracle.py -- the checker of every device test of the FM-multiplex decoder pool -- to the reference's own src/stereod.c and
src/rdsd.c.

tests/c/ref_stereod_wrap.c and tests/c/ref_rdsd_wrap.c #include the reference's files where they lie (main renamed, sendto redirected to a
recorder, pthread_cond_timedwait answering ETIMEDOUT, pthread_detach a no-op), queue the whole input on a session as RTP packets of 384
samples and run decode() on a thread whose stack is fresh zero pages; stereod's wrapper sets Blocktime, Deemph_tc, Deemph_gain = 4 and
Deemph_rate as its main() does (a time constant of 0 stands for rate 0) and records deemph_state_left / right at full precision after every
block.  They are compiled into tmp_path as programs with the reference's release flags (oracle/Makefile's REF_CFLAGS) together with the
reference's filter window misc sched sincospi osc gauss rtp and the oracle's FFT provider (oracle/_build/fftw_shim.o, dft_ref.o); the
reference's transform runs in the caller's thread (N_worker_threads = 0, for the reason tests/c/ref_packetd_wrap.c gives).

stereod: all five instances of tests/test_gpu_mpx.py's scenario at 1, 5 and 20 ms and, for tests/test_gpu_mpx_shapes.py, at 2 and 10 ms;
rdsd: the RDS test's two instances at 5 ms (its Blocktime is a constant: the RDS pools at 1, 2 and 10 ms rest on the restatement's
parametrisation by the block time, which stereod's pin holds for the code the two share); each on the reference's float64 transform and on its float32 one (oracle_fft_set_precision).  EVERY PCM sample:
|pcm - 32767 clamp(y, -1, 1)| <= 1 + 32767 lim, y the restatement's float64 value and lim the block's max-abs limit of rule (A) in
tests/test_gpu_mpx.py; the recorded states: within lim of the restatement's.  The tests print the worst distance over the allowed, the share
of bit-equal samples in the last block and the time the reference's loop takes per block.

Measured: stereod 0.49 of the allowed at worst (PCM), 8e-7 of the block's rms (states), 99.0 - 100 % of the last block's samples bit-equal; rdsd 0.98
of the allowed -- its restatement differs from the reference by nothing but the packer's truncation, which the bound's "1 +" is for.

Where this departs from the issue's wording: the wrapper computes Deemph_rate as stereod's main() does except for a time constant of 0, which
stands for rate 0 (instance 2) without dividing by it; all five instances of the scenario are pinned, not one."""
import os
import re
import subprocess

import numpy as np
import pytest

import afsk_oracle as ao
import mpx_oracle as mo
import oracle_lib as ol
import test_gpu_mpx as tg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE = os.path.join(ROOT, "oracle")


def makefile_var(name):
    with open(os.path.join(ORACLE, "Makefile")) as f:
        m = re.search(r"^%s\s*\??=\s*(.*)$" % name, f.read(), re.M)
    return m.group(1).strip()


REF = os.environ.get("REF", makefile_var("REF"))
needs_ref = pytest.mark.skipif(not (os.path.isfile(os.path.join(REF, "stereod.c")) and os.path.isfile(os.path.join(REF, "rdsd.c"))), reason="the reference tree is not here")


@pytest.fixture(scope="module")
def refmpx(tmp_path_factory):
    """-> {"stereod": program, "rdsd": program}"""
    ol.build()                          # oracle/_build/fftw_shim.o and dft_ref.o
    work = str(tmp_path_factory.mktemp("refmpx"))
    wraps = {n: os.path.join(ROOT, "tests", "c", "ref_%s_wrap.c" % n) for n in ("stereod", "rdsd")}
    srcs = [os.path.join(REF, f + ".c") for f in "filter window misc sched sincospi osc gauss rtp".split()] + list(wraps.values())
    git = ['-DGIT_%s="none"' % k for k in ("HASH", "BRANCH", "DATE", "VERSION", "REMOTE_URL")]
    # compiled with the reference's flags, linked without them (as oracle/Makefile links _ref/ and tests/test_ctcss_reference.py its program);
    # neither main() of the reference is called, so the sections that hold them and the network code they reach are dropped at link time
    subprocess.run(["gcc"] + makefile_var("REF_CFLAGS").split() + git + ["-I", os.path.join(ORACLE, "shims"), "-iquote", REF, "-ffunction-sections",
                    "-fdata-sections", "-c"] + srcs, check=True, cwd=work)
    objs = [os.path.join(work, os.path.basename(f)[:-2] + ".o") for f in srcs]
    progs = {}
    for n in wraps:
        progs[n] = os.path.join(work, "ref_" + n)
        mine = [o for o in objs if not o.endswith("_wrap.o") or o.endswith("ref_%s_wrap.o" % n)]
        subprocess.run(["gcc", "-o", progs[n]] + mine + [os.path.join(ORACLE, "_build", "fftw_shim.o"), os.path.join(ORACLE, "_build", "dft_ref.o"),
                        "-Wl,--gc-sections", "-l:libbsd.so.0", "-lm", "-lpthread"], check=True)
    return progs


def compare(label, pcm, states, ref, lims, olen):
    """one reference run against the restatement -> prints the worst figures"""
    got = np.frombuffer(pcm, ">i2").astype(np.float64)
    assert got.shape[0] == len(ref) * 2 * olen, (label, got.shape[0], len(ref), olen)
    got = got.reshape(len(ref), 2 * olen)
    worst, worst_state = 0.0, 0.0
    for blk, (r, (rms, _, lim)) in enumerate(zip(ref, lims)):
        want = 32767.0 * np.clip(r["audio"], -1.0, 1.0)
        d = float(np.abs(got[blk] - want).max())
        allowed = 1 + 32767.0 * lim
        worst = max(worst, d / allowed)
        assert d <= allowed, (label, blk, d, allowed)
        if states is not None:
            se = max(abs(states[blk][0] - r["deemph_left"]), abs(states[blk][1] - r["deemph_right"]))
            assert se <= lim, (label, blk, "state", se, lim)
            if rms > 0:
                worst_state = max(worst_state, se / rms)
    equal = float(np.mean(got[-1] == np.frombuffer(ref[-1]["pcm"], ">i2")))
    print("%s: %d blocks; worst PCM distance %.2f of the allowed, worst state distance %.2g of the block's rms, %.1f %% of the last block's samples bit-equal"
          % (label, len(ref), worst, worst_state, 100 * equal))


@needs_ref
@pytest.mark.parametrize("shape", list(tg.SHAPES) + [0.002, 0.01])       # (2 and 10 ms: the shapes of tests/test_gpu_mpx_shapes.py)
def test_the_restatement_of_stereod_s_loop_against_stereod_c(refmpx, tmp_path, shape):
    bt = tg.block_time(shape)
    olen = mo.geometry(bt)["olen"]
    tcs = [75e-6, 50e-6, 0.0, 75e-6, 75e-6]
    for k, blocks in enumerate(tg.scenario(shape)):
        assert mo.rate_of(tcs[k]) == tg.SCENARIO[k][1]
        ref, twin = tg.restatement(shape, False)[k], tg.restatement(shape, True)[k]
        for blk, (r, t) in enumerate(zip(ref, twin)):
            assert r["zero_pilot"] == t["zero_pilot"], (shape, k, blk)
        lims = tg.limits(ref, twin, tg.whole_window_signal(tg.SCENARIO[k][2], tg.NBLOCKS))
        path = str(tmp_path / ("inst%d.s16be" % k))
        ao.to_wire(blocks.reshape(-1), big_endian=True).tofile(path)
        for f32 in (0, 1):
            pcm, st = str(tmp_path / ("pcm%d_%d" % (k, f32))), str(tmp_path / ("st%d_%d" % (k, f32)))
            r = subprocess.run([refmpx["stereod"], path, repr(bt), repr(tcs[k]), str(f32), pcm, st], capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, (r.returncode, r.stderr[-1500:])
            with open(st) as f:
                states = [tuple(float(v) for v in line.split()) for line in f]
            assert len(states) == tg.NBLOCKS
            with open(pcm, "rb") as f:
                compare("%s instance %d, stereod's %s transform (%s)" % (shape, k, "float32" if f32 else "float64", r.stdout.strip()), f.read(), states, ref, lims, olen)


@needs_ref
def test_the_restatement_of_rdsd_s_loop_against_rdsd_c(refmpx, tmp_path):
    bt = 0.005
    olen = mo.geometry(bt, mo.RDS)["olen"]
    for k, a in enumerate((0.2, 0.9)):
        blocks = mo.signal(tg.RDS_BLOCKS, bt, 10 + k, a, rds=True)
        ref, twin = (mo.run(blocks, bt, kind=mo.RDS, f32=f) for f in (False, True))
        lims = tg.limits(ref, twin)
        path = str(tmp_path / ("rds%d.s16be" % k))
        ao.to_wire(blocks.reshape(-1), big_endian=True).tofile(path)
        for f32 in (0, 1):
            pcm = str(tmp_path / ("rdspcm%d_%d" % (k, f32)))
            r = subprocess.run([refmpx["rdsd"], path, str(f32), pcm], capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, (r.returncode, r.stderr[-1500:])
            with open(pcm, "rb") as f:
                compare("5ms RDS instance %d, rdsd's %s transform (%s)" % (k, "float32" if f32 else "float64", r.stdout.strip()), f.read(), None, ref, lims, olen)


def test_scaleclip_and_the_geometry_table():
    """the packer's rule on its edges (src/misc.h:252-254), and geometry() on the block times the pool accepts"""
    x = np.array([0.0, 1.0, -1.0, 1.5, -1.5, np.nextafter(np.float32(1), np.float32(0)), -np.nextafter(np.float32(1), np.float32(0)), 0.5, -0.5, 3.0517578e-05, -3.0517578e-05, 2e-5], np.float32)
    assert mo.scaleclip(x).tolist() == [0, 32767, -32767, 32767, -32767, 32766, -32766, 16383, -16383, 0, 0, 0]
    assert mo.pack(np.array([0.5, -1.0], np.float32)) == bytes([0x3f, 0xff, 0x80, 0x01])
    assert tuple(mo.geometry(0.005).values()) == (1920, 1921, 3840, 240, 480, 190, 380)
    assert tuple(mo.geometry(0.005, mo.RDS).values()) == (1920, 1921, 3840, 240, 480, 190, 570)
    assert tuple(mo.geometry(0.001).values()) == (384, 385, 768, 48, 96, 38, 76) and tuple(mo.geometry(0.02).values()) == (7680, 7681, 15360, 960, 1920, 760, 1520)
