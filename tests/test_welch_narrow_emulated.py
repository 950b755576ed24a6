"""CPU-tier twin of tests/test_gpu_welch_narrow.py: the engine's host code built for the CPU (tests/test_engine_emulated.py) runs the
narrowband analyser -- bb_ring_append, welch_seg on a baseband ring, welch_sum, and the ordering of appends and polls as far as a
synchronous runtime shows it -- against the restated narrowband_poll(), in a child process.  Nothing is left out: every case of the
GPU file runs (the graph refusal in test_refusals is answered before any capture starts)."""
import os
import subprocess

import pytest

from test_engine_emulated import emulated_engine, ROOT, EMU, CSRC      # noqa: F401  (the fixture that builds tests/hipemu/libchz_hip_emu.so)
from test_welch_emulated import _child


def test_narrowband_welch_on_the_emulator(emulated_engine):
    env = dict(os.environ, CHZ_LIB=emulated_engine, CHZ_ALLOW_EMULATED_ENGINE="1")
    _child([os.path.join(ROOT, "tests", "test_gpu_welch_narrow.py")], env, 36)


def _driver(lib, exe, san=None):
    cmd = ["gcc", "-O1", "-g", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "nb_welch_driver.c"), "-o", exe,
           "-L", os.path.dirname(lib), "-l:" + os.path.basename(lib), "-Wl,-rpath," + os.path.dirname(lib), "-lpthread"]
    if san:
        cmd.insert(1, "-fsanitize=" + san)
    subprocess.run(cmd, check=True)


def test_narrowband_threading_driver(emulated_engine, tmp_path):
    """tests/c/nb_welch_driver.c from plain C: analysers attached to two banks while blocks are pipelined from several issuing threads,
    polls, a partial re-run, detach / attach, a welch bank and a channel bank destroyed under the others -- must run to the end."""
    exe = str(tmp_path / "nb_driver")
    _driver(emulated_engine, exe)
    for thr in ("1", "2", "4"):
        r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, CHZ_ENQ_THREADS=thr))
        assert r.returncode == 0 and "driver ok blocks 52" in r.stdout, (thr, r.stdout[-300:], r.stderr[-1500:])


@pytest.mark.skipif(os.environ.get("CHZ_TEST_TSAN_ENGINE") != "1", reason="minutes of build and run: CHZ_TEST_TSAN_ENGINE=1 (TSAN=1 scripts/engine_emulated.sh)")
def test_narrowband_threading_driver_under_thread_sanitizer(tmp_path):
    """The same driver with the engine's host code built with -fsanitize=thread, 2 and 4 issuing threads."""
    lib = str(tmp_path / "libchz_hip_emu_tsan.so")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fPIC", "-shared", "-fsanitize=thread", "-DHIPEMU", "-DHIPEMU_HOST", "-I", EMU, "-I", CSRC, "-x", "c++",
                    os.path.join(CSRC, "chz_engine.hip"), "-o", lib, "-lpthread", "-ldl"], check=True)
    exe = str(tmp_path / "nb_driver_tsan")
    _driver(lib, exe, "thread")
    for thr in ("2", "4"):
        r = subprocess.run([exe], capture_output=True, text=True, timeout=1500,
                           env=dict(os.environ, CHZ_ENQ_THREADS=thr, TSAN_OPTIONS="halt_on_error=0 report_signal_unsafe=0 exitcode=66"))
        assert "WARNING: ThreadSanitizer" not in r.stderr, r.stderr[-5000:]
        assert r.returncode == 0 and "driver ok blocks 52" in r.stdout, (thr, r.stdout[-300:], r.stderr[-1500:])


def test_dropin_narrowband_spectrum_on_the_emulated_engine(emulated_engine, tmp_path):
    """tests/test_dropin_spectrum_narrow.py's device cases with the drop-in linked on the CPU build of the engine (its stub case runs in the CPU suite as it is)"""
    import shutil
    libdir = str(tmp_path / "lib")
    os.makedirs(libdir)
    shutil.copy(emulated_engine, os.path.join(libdir, "libchz_hip.so"))
    subprocess.run(["gcc", "-O2", "-std=gnu11", "-fPIC", "-shared", "-Wall", "-Wextra", "-Wno-unused-parameter", "-Wno-maybe-uninitialized",
                    os.path.join(CSRC, "filter_hip.c"), "-o", os.path.join(libdir, "libka9q_filter_hip.so"), "-L", libdir, "-lchz_hip",
                    "-Wl,-rpath,$ORIGIN", "-lm", "-lpthread"], check=True)
    _child([os.path.join(ROOT, "tests", "test_dropin_spectrum_narrow.py")], dict(os.environ, KA9Q_TEST_LIBDIR=libdir), 3)
