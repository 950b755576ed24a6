"""CPU-tier twin of tests/test_gpu_noise_select.py: the engine's host code and the unmodified noise_est / spec_energy kernels built for
the CPU (tests/test_engine_emulated.py) run that whole file in a child process -- every branch of the rank selection, the lane
placements, the seam windows and the guess script, from the spectrum and from the energy image.  The emulator's wave_* helpers are
plain shuffles, not the device's DPP steps: what this pins is the selection's logic (and, for the first time on the CPU, the guess
and the energy-image kernels on corner windows); the DPP steps are the GPU file's business.  Nothing is deselected."""
import os
import re
import subprocess
import sys

from test_engine_emulated import emulated_engine, ROOT      # noqa: F401  (the fixture that builds tests/hipemu/libchz_hip_emu.so)


def test_noise_selection_on_the_emulator(emulated_engine):
    env = dict(os.environ, CHZ_LIB=emulated_engine, CHZ_ALLOW_EMULATED_ENGINE="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_noise_select.py"), "-m", "gpu", "-q", "-x",
                        "--timeout", "600", "-p", "no:cacheprovider"], capture_output=True, text=True, env=env, timeout=1500, cwd=ROOT)
    tail = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else ""
    assert r.returncode == 0, (tail, r.stdout[-3000:], r.stderr[-1500:])
    m = re.search(r"(\d+) passed", tail)
    assert m and int(m.group(1)) == 57 and "skipped" not in tail and "deselected" not in tail, tail
