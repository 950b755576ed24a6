"""Pooled small REAL inline masters behind filter.h (ka9q_hip_pool_real_masters, include/ka9q_filter_hip_ext.h).

tests/c/rmini_harness.c runs one thread per master -- stereod-shaped (L 1920, M 1921; REAL + COMPLEX + COMPLEX slaves of olen 240) and
packetd-shaped (L 960, M 961; one COMPLEX slave of olen 960) -- in the callers' order: write_rfilter, then execute_filter_output per
slave with per-slave shifts; one slave per third thread moves to a new shift in mid-stream, odd threads delete the master before its
slaves, and one more master gets a fourth slave the pool cannot serve (P = 34) before its first block and must become an engine.
Once with the option on and once with it off; both must meet check_channel (tests/test_gpu_parity.py) against the float64 oracle, and
the pooled run must create exactly one engine: the fourth-slave master's.  Every run lives twice in one process (create, run, delete,
again): the pool instances of the first life must be free for the second (ka9q_hip_real_master_pools()).

GPU tier: 24 + 8 masters.  CPU tier: 4 + 2 masters with the drop-in linked on the emulated engine, the same under AddressSanitizer
(stand-alone program; the leak check covers the master-deleted-first order) and, with 2 + 1 masters, under ThreadSanitizer (stand-alone
program, engine host code instrumented too), and one run on the stub engine library, which has no
pools: the option changes nothing there.
"""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
from test_gpu_parity import check_channel
from test_gpu_rmini import real_channel_f64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ka9q-radio_amd")
CSRC = os.path.join(PKG, "csrc")
SRC = os.path.join(ROOT, "tests", "c", "rmini_harness.c")
NBLOCKS = 4
C, R = ol.COMPLEX, ol.REAL
# what tests/c/rmini_harness.c holds: (L, M, [(olen, type, shift, lo, hi)])
STEREOD = (1920, 1921, [(240, R, 0, 0.002, 0.3), (240, C, 152, -0.01, 0.01), (240, C, 304, -0.3, 0.3), (17, C, 40, -0.4, 0.4)])
PACKETD = (960, 961, [(960, C, 340, -0.2, 0.25)])


def _harness(exe, libdir, san=None):
    cmd = ["gcc", "-O1", "-g", "-std=gnu11", "-Wall", "-I", os.path.join(ROOT, "include"), SRC, "-o", exe,
           "-L", libdir, "-lka9q_filter_hip", "-lchz_hip", "-Wl,-rpath," + libdir, "-lpthread", "-lm"]
    if san:
        cmd.insert(1, "-fsanitize=" + san)
    subprocess.run(cmd, check=True)


def _dropin_on(engine_lib, libdir, san=None):
    os.makedirs(libdir, exist_ok=True)
    shutil.copy(engine_lib, os.path.join(libdir, "libchz_hip.so"))
    cmd = ["gcc", "-O1", "-g", "-std=gnu11", "-fPIC", "-shared", "-Wall", "-Wextra", "-Wno-unused-parameter", "-Wno-maybe-uninitialized",
           os.path.join(CSRC, "filter_hip.c"), "-o", os.path.join(libdir, "libka9q_filter_hip.so"), "-L", libdir, "-lchz_hip",
           "-Wl,-rpath,$ORIGIN", "-lm", "-lpthread"]
    if san:
        cmd.insert(1, "-fsanitize=" + san)
    subprocess.run(cmd, check=True)


def _shapes(ns, npk):
    out = []
    for t in range(ns + npk + 1):
        L, M, sl = STEREOD if (t < ns or t == ns + npk) else PACKETD
        out.append((L, M, sl if t == ns + npk else sl[:3] if L == 1920 else sl))
    return out


def _run_and_check(exe, tmp, ns, npk, env=None, expect_pooling=1):
    """both runs against the oracle; returns the engines each run created"""
    ol.build()
    shapes = _shapes(ns, npk)
    rng = np.random.default_rng(ns * 100 + npk)
    x = [rng.standard_normal(NBLOCKS * L).astype(np.float32) for L, M, sl in shapes]
    np.concatenate(x).tofile(os.path.join(tmp, "in.bin"))
    engines = {}
    for pool in (1, 0):
        r = subprocess.run([exe, tmp, str(pool), str(ns), str(npk), str(NBLOCKS), "2"], capture_output=True, text=True, timeout=600,
                           env=dict(os.environ, **(env or {})))
        assert r.returncode == 0, (pool, r.stdout[-500:], r.stderr[-3000:])
        m = re.search(r"pooling (\d+) engines (\d+) masters (\d+)", r.stdout)
        assert m and int(m.group(3)) == len(shapes), r.stdout
        assert int(m.group(1)) == (expect_pooling if pool else 0)
        engines[pool] = int(m.group(2))
        # two lives in one process, odd masters deleted before their slaves: every instance the first round took is free again (nothing
        # but the running masters of the second round is taken after its last block, nothing at the end), and no further pool appeared
        u = re.search(r"pools (\d+) in_use_running (\d+) in_use_end (\d+)", r.stdout)
        pooled = pool == 1 and expect_pooling == 1
        assert u and [int(v) for v in u.groups()] == ([len({(L, M) for L, M, sl in shapes}), ns + npk, 0] if pooled else [0, 0, 0]), r.stdout
        got = np.fromfile(os.path.join(tmp, "out%d.bin" % pool), np.float32)
        at = 0
        worst = 0.0
        for t, (L, M, sl) in enumerate(shapes):
            N = L + M - 1
            st = ol.Stream(L, M, ol.REAL)
            spec = [st.push(x[t][b * L:(b + 1) * L], f64=True) for b in range(NBLOCKS)]
            for k, (olen, typ, shift, lo, hi) in enumerate(sl):
                P = N * olen // L
                resp = ol.set_filter(P, olen, N, True, lo, hi, 5.0 + k, typ)
                n = olen * (1 if typ == R else 2)
                for b in range(NBLOCKS):
                    o = got[at:at + n]; at += n
                    o = o if typ == R else o.view(np.complex64)
                    sh = shift + 4 * (t % 5) + (8 if (k == 1 and t % 3 == 0 and b >= 2) else 0)
                    want = real_channel_f64(spec[b], P, olen, sh, resp) if typ == R else ol.channel(spec[b], ol.REAL, P, olen, sh, resp)
                    worst = max(worst, check_channel(o, want))
        assert at == got.shape[0]
        print("pool %d: %d engines for %d masters, worst rel-L2 %.3g" % (pool, engines[pool], len(shapes), worst))
    return engines, len(shapes)


@pytest.mark.gpu
def test_pooled_real_masters_behind_filter_h(tmp_path):
    subprocess.run(["make", "-s", "-C", CSRC, "all"], check=True)
    exe = str(tmp_path / "rmini_harness")
    _harness(exe, PKG)
    engines, masters = _run_and_check(exe, str(tmp_path), 24, 8)
    assert engines[0] == masters                # the parent's behaviour: one engine per master
    assert engines[1] == 1                      # pooled: only the master with the slave no pool serves became an engine


from test_engine_emulated import emulated_engine      # noqa: E402,F401  (the fixture that builds tests/hipemu/libchz_hip_emu.so)


def test_pooled_real_masters_behind_filter_h_on_the_emulated_engine(emulated_engine, tmp_path):
    libdir = str(tmp_path / "lib")
    _dropin_on(emulated_engine, libdir)
    exe = str(tmp_path / "rmini_harness")
    _harness(exe, libdir)
    engines, masters = _run_and_check(exe, str(tmp_path), 4, 2)
    assert engines[0] == masters and engines[1] == 1


def test_pooled_real_masters_host_code_under_address_sanitizer(emulated_engine, tmp_path):
    """The drop-in's host code and the harness built with -fsanitize=address as a stand-alone program on the emulated engine: no bad
    access, and nothing leaked when a master goes before its slaves or becomes an engine with slaves registered."""
    libdir = str(tmp_path / "lib")
    _dropin_on(emulated_engine, libdir, "address")
    exe = str(tmp_path / "rmini_harness_asan")
    _harness(exe, libdir, "address")
    _run_and_check(exe, str(tmp_path), 4, 2, env={"ASAN_OPTIONS": "detect_leaks=1 exitcode=67"})


def test_pooled_real_masters_host_code_under_thread_sanitizer(tmp_path):
    """The same stand-alone program with the engine's host code (its emulated kernels' fibers are announced to the race detector), the
    drop-in and the harness built with -fsanitize=thread: the batch-leader queue, the shared per-master state and the conversion to an
    engine must raise no report (one finding when this was written: the conversion took the engine context's lock under the master's
    mutex, the completion path's order reversed).  Runs by default, unlike the engine's own TSan drivers: 2 + 1 + 1 masters keep the
    run short, the instrumented build of the engine is most of its few minutes."""
    from test_engine_emulated import EMU
    libdir = str(tmp_path / "lib")
    os.makedirs(libdir)
    eng = os.path.join(libdir, "libchz_hip_tsan_build.so")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fPIC", "-shared", "-fsanitize=thread", "-DHIPEMU", "-DHIPEMU_HOST", "-I", EMU, "-I", CSRC, "-x", "c++",
                    os.path.join(CSRC, "chz_engine.hip"), "-o", eng, "-lpthread", "-ldl"], check=True)
    _dropin_on(eng, libdir, "thread")
    exe = str(tmp_path / "rmini_harness_tsan")
    _harness(exe, libdir, "thread")
    rng = np.random.default_rng(3)
    np.concatenate([rng.standard_normal(NBLOCKS * L).astype(np.float32) for L, M, sl in _shapes(2, 1)]).tofile(str(tmp_path / "in.bin"))
    r = subprocess.run([exe, str(tmp_path), "1", "2", "1", str(NBLOCKS), "2"], capture_output=True, text=True, timeout=1500,
                       env=dict(os.environ, TSAN_OPTIONS="halt_on_error=0 report_signal_unsafe=0 exitcode=66"))
    assert "WARNING: ThreadSanitizer" not in r.stderr, r.stderr[-5000:]
    assert r.returncode == 0 and "pooling 1 engines 1" in r.stdout, (r.stdout[-300:], r.stderr[-1500:])


def test_the_option_is_a_no_op_on_an_engine_library_without_the_pools(tmp_path):
    ol.build()
    libdir = str(tmp_path / "lib")
    os.makedirs(libdir)
    stub = os.path.join(libdir, "libchz_stub_build.so")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fPIC", "-shared", os.path.join(ROOT, "tests", "stub", "chz_stub.cpp"), "-o", stub,
                    "-L", os.path.join(ROOT, "oracle"), "-loracle", "-Wl,-rpath," + os.path.join(ROOT, "oracle"), "-lpthread"], check=True)
    _dropin_on(stub, libdir)
    exe = str(tmp_path / "rmini_harness")
    _harness(exe, libdir)
    engines, masters = _run_and_check(exe, str(tmp_path), 2, 1, expect_pooling=0)
    assert engines[0] == masters and engines[1] == masters
