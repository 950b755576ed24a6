"""CPU-tier twin of tests/test_gpu_raw_input.py: the engine's host code and the unmodified raw_unpack kernel built for the CPU
(tests/test_engine_emulated.py) run that whole file in a child process -- every format, every write size and start offset, the wrap, the
statistics and their tickets, the device form, every refusal.  The emulated runtime is synchronous: what this tier pins is the kernel's
unpacking, masking and index arithmetic and the host's bookkeeping, not the stream order.  And the binding's own numbers."""
import os
import re
import subprocess
import sys

import raw_oracle as ro
from conftest import load_pkg
from test_engine_emulated import emulated_engine, ROOT      # noqa: F401  (the fixture that builds tests/hipemu/libchz_hip_emu.so)


def test_raw_input_on_the_emulator(emulated_engine):
    env = dict(os.environ, CHZ_LIB=emulated_engine, CHZ_ALLOW_EMULATED_ENGINE="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_raw_input.py"), "-m", "gpu", "-q", "-x",
                        "--timeout", "600", "-p", "no:cacheprovider"], capture_output=True, text=True, env=env, timeout=1500, cwd=ROOT)
    tail = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else ""
    assert r.returncode == 0, (tail, r.stdout[-3000:], r.stderr[-1500:])
    m = re.search(r"(\d+) passed", tail)
    assert m and int(m.group(1)) == 24 and "skipped" not in tail and "deselected" not in tail, tail


def test_the_binding_numbers_the_formats_as_the_header_does():
    E = load_pkg().engine
    with open(os.path.join(ROOT, "include", "chz_engine.h")) as f:
        header = dict(re.findall(r"^#define CHZ_RAW_(\w+)\s+(\d+)", f.read(), re.M))
    assert int(header.pop("TICKETS")) == 8
    assert {k: int(v) for k, v in header.items()} == {ro.NAMES[f].upper(): f for f in range(8)}
    for f in range(8):
        assert getattr(E, "RAW_" + ro.NAMES[f].upper()) == f and E.RAW_BYTES[f] == ro.BYTES[f]
    for sym in ("chz_input_raw_check", "chz_input_write_raw", "chz_input_write_raw_device", "chz_input_raw_stats"):
        assert sym in E.SYMBOLS
