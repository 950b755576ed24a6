"""CPU-tier twin of tests/test_gpu_afsk_rates.py: the engine's host code and the unmodified afsk_ovs kernel built for the CPU
(tests/test_engine_emulated.py) run that whole file in a child process -- the six shapes (a truncated and an odd samppbit, the slipping clock and its control, histories shorter and longer than
the block), the frame longer than the HDLC's buffer beside a neighbour with an open frame (5592 blocks: 9 s of this test's 20 here, kept in) and the
refusals."""
import os
import re
import subprocess
import sys

from test_engine_emulated import emulated_engine, ROOT      # noqa: F401  (the fixture that builds tests/hipemu/libchz_hip_emu.so)


def test_afsk_pools_away_from_whole_samples_a_bit_on_the_emulator(emulated_engine):
    env = dict(os.environ, CHZ_LIB=emulated_engine, CHZ_ALLOW_EMULATED_ENGINE="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_afsk_rates.py"), "-m", "gpu", "-q", "-x",
                        "--timeout", "600", "-p", "no:cacheprovider"], capture_output=True, text=True, env=env, timeout=1500, cwd=ROOT)
    tail = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else ""
    assert r.returncode == 0, (tail, r.stdout[-3000:], r.stderr[-1500:])
    m = re.search(r"(\d+) passed", tail)
    assert m and int(m.group(1)) == 18 and "skipped" not in tail and "deselected" not in tail, tail
