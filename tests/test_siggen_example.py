"""examples/chz_siggen.c: the device-side sig_gen front end from plain C (gcc, no Python in the process) -- it compiles against
include/chz_engine.h wherever the library has been built, and on the device it prints the analytic known answer (a bin-centred carrier through
one 12 kHz channel: |y| = amplitude scale / sqrt(2)) and exits 0 only if every output sample is within 1e-4 of it."""
import os
import re
import subprocess

import pytest

from conftest import load_pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_example(tmp_path):
    pkg = load_pkg()
    libdir = os.path.dirname(pkg.engine.LIB_PATH)
    exe = str(tmp_path / "chz_siggen")
    subprocess.run(["gcc", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "chz_siggen.c"),
                    "-L", libdir, "-lchz_hip", "-Wl,-rpath," + libdir, "-lm", "-o", exe], check=True)
    return exe


def test_the_example_compiles_from_plain_c(tmp_path):
    assert os.path.exists(build_example(tmp_path))


@pytest.mark.gpu
def test_the_example_prints_the_known_answer(tmp_path):
    r = subprocess.run([build_example(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    m = re.search(r"\|y\| = ([0-9.]+), a scale / sqrt\(2\) = ([0-9.]+), within ([0-9.e+-]+)", r.stdout)
    assert m and abs(float(m.group(1)) - 0.1 * 10 ** (3 / 20) / 2 ** 0.5) < 1e-5 and float(m.group(3)) < 1e-4, r.stdout
    assert "generated 7776000 samples" in r.stdout
