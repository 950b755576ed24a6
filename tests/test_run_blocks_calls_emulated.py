"""CPU-tier twin of tests/test_gpu_run_blocks_calls.py: the engine's host code built for the CPU (tests/test_engine_emulated.py)
runs the bitwise comparisons of chz_run_blocks calls against the same blocks stepped one at a time -- calls issued by the caller
alone, calls split over the issuing threads (kernels of two threads then really run side by side here), calls that do not fill
every lane, fifty one-block calls followed by a long one -- at the N = 32,400 geometry, in a child process."""
import os
import re
import subprocess
import sys

from test_engine_emulated import emulated_engine, ROOT      # noqa: F401  (the fixture that builds tests/hipemu/libchz_hip_emu.so)


def test_run_blocks_calls_on_the_emulator(emulated_engine):
    env = dict(os.environ, CHZ_LIB=emulated_engine, CHZ_ALLOW_EMULATED_ENGINE="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_run_blocks_calls.py"), "-m", "gpu", "-q", "-x",
                        "--timeout", "600", "-p", "no:cacheprovider", "-k", "small and (one_call_equals or fifty_one_block)",
                        "-n", str(max(1, min(6, (os.cpu_count() or 2) - 1)))],
                       capture_output=True, text=True, env=env, timeout=1500, cwd=ROOT)
    tail = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else ""
    assert r.returncode == 0, (tail, r.stdout[-3000:], r.stderr[-1500:])
    m = re.search(r"(\d+) passed", tail)
    assert m and int(m.group(1)) == 9, tail
