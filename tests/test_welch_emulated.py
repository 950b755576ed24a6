"""CPU-tier twins of tests/test_gpu_welch.py and tests/test_dropin_spectrum.py: the engine's host code built for the CPU
(tests/test_engine_emulated.py) runs the wideband analyser's kernels on the emulator -- every case but the 129.6 MS/s master's --
against the restated wideband_poll(), in a child process; the drop-in's ka9q_hip_spectrum() is linked on that build and driven the
same way."""
import os
import re
import shutil
import subprocess
import sys

from test_engine_emulated import emulated_engine, ROOT, CSRC      # noqa: F401  (the fixture that builds tests/hipemu/libchz_hip_emu.so)


def _child(args, env, want):
    r = subprocess.run([sys.executable, "-m", "pytest"] + args + ["-m", "gpu", "-q", "-x", "--timeout", "600", "-p", "no:cacheprovider"],
                       capture_output=True, text=True, env=env, timeout=1500, cwd=ROOT)
    tail = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else ""
    assert r.returncode == 0, (tail, r.stdout[-3000:], r.stderr[-1500:])
    m = re.search(r"(\d+) passed", tail)
    assert m and int(m.group(1)) == want, tail


def test_welch_on_the_emulator(emulated_engine):
    env = dict(os.environ, CHZ_LIB=emulated_engine, CHZ_ALLOW_EMULATED_ENGINE="1")
    _child([os.path.join(ROOT, "tests", "test_gpu_welch.py"), "-k", "not config3"], env, 45)


def test_dropin_spectrum_on_the_emulated_engine(emulated_engine, tmp_path):
    libdir = str(tmp_path / "lib")
    os.makedirs(libdir)
    shutil.copy(emulated_engine, os.path.join(libdir, "libchz_hip.so"))
    subprocess.run(["gcc", "-O2", "-std=gnu11", "-fPIC", "-shared", "-Wall", "-Wextra", "-Wno-unused-parameter", "-Wno-maybe-uninitialized",
                    os.path.join(CSRC, "filter_hip.c"), "-o", os.path.join(libdir, "libka9q_filter_hip.so"), "-L", libdir, "-lchz_hip",
                    "-Wl,-rpath,$ORIGIN", "-lm", "-lpthread"], check=True)
    _child([os.path.join(ROOT, "tests", "test_dropin_spectrum.py")], dict(os.environ, KA9Q_TEST_LIBDIR=libdir), 3)
