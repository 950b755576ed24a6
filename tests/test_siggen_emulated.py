"""CPU-tier twin of tests/test_gpu_siggen.py: the engine's host code and the unmodified siggen_fill kernel built for the CPU
(tests/test_engine_emulated.py) run that whole file in a child process -- every generate size and start offset, the wrap, the lane states
derived by the wavefront's ballots, the carrier, seek and tell, the energy sums and their tickets, every refusal.  The emulated runtime is
synchronous and its sincospi is the C library's: what this tier pins is the kernel's arithmetic, masking and index arithmetic and the host's
bookkeeping, not the stream order.  And that the binding lists the new calls."""
import os
import re
import subprocess
import sys

from conftest import load_pkg
from test_engine_emulated import emulated_engine, ROOT      # noqa: F401  (the fixture that builds tests/hipemu/libchz_hip_emu.so)


def test_the_generated_front_end_on_the_emulator(emulated_engine):
    env = dict(os.environ, CHZ_LIB=emulated_engine, CHZ_ALLOW_EMULATED_ENGINE="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_siggen.py"), "-m", "gpu", "-q", "-x",
                        "--timeout", "600", "-p", "no:cacheprovider"], capture_output=True, text=True, env=env, timeout=1500, cwd=ROOT)
    tail = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else ""
    assert r.returncode == 0, (tail, r.stdout[-3000:], r.stderr[-1500:])
    m = re.search(r"(\d+) passed", tail)
    assert m and int(m.group(1)) == 59 and "skipped" not in tail and "deselected" not in tail, tail


def test_the_binding_lists_the_new_calls():
    E = load_pkg().engine
    with open(os.path.join(ROOT, "include", "chz_engine.h")) as f:
        header = f.read()
    assert int(re.search(r"^#define CHZ_SIGGEN_RUN\s+(\d+)", header, re.M).group(1)) == E.SIGGEN_RUN
    for sym in ("chz_siggen_check", "chz_siggen_jump", "chz_siggen_seed", "chz_input_siggen_set", "chz_input_siggen_seek", "chz_input_siggen_tell",
                "chz_input_generate", "chz_input_generate_stats"):
        assert sym in E.SYMBOLS and re.search(r"\b%s\s*\(" % sym, header)
    for name in ("siggen", "siggen_seek", "siggen_tell", "generate", "generate_energy"):
        assert callable(getattr(E.Engine, name))
    assert callable(E.siggen_jump) and callable(E.siggen_seed)
