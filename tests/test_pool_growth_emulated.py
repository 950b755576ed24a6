"""CPU-tier twin of tests/test_gpu_pool_growth.py: the engine's host code and the unmodified afsk_ovs, ctcss_ovs and mpx_ovs kernels built for the CPU
(tests/test_engine_emulated.py) run that whole file in a child process -- the three pools' storage growing 2 -> 4 -> 8 under running decoders, against the
restatements and against pools that never grow, and a released index added again."""
import os
import re
import subprocess
import sys

from test_engine_emulated import emulated_engine, ROOT      # noqa: F401  (the fixture that builds tests/hipemu/libchz_hip_emu.so)


def test_storage_that_grows_under_running_decoders_on_the_emulator(emulated_engine):
    env = dict(os.environ, CHZ_LIB=emulated_engine, CHZ_ALLOW_EMULATED_ENGINE="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_pool_growth.py"), "-m", "gpu", "-q", "-x",
                        "--timeout", "600", "-p", "no:cacheprovider"], capture_output=True, text=True, env=env, timeout=1500, cwd=ROOT)
    tail = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else ""
    assert r.returncode == 0, (tail, r.stdout[-3000:], r.stderr[-1500:])
    m = re.search(r"(\d+) passed", tail)
    assert m and int(m.group(1)) == 3 and "skipped" not in tail and "deselected" not in tail, tail
