"""The host arithmetic of the device-side sig_gen front end (ka9q-radio_amd/csrc/chz_siggen.h) under AddressSanitizer and
UndefinedBehaviorSanitizer: tests/c/siggen_check.cpp, a stand-alone program with its own main, is built with g++ -fsanitize=address,undefined
into tmp_path and run as a child process -- jump-ahead against sequential stepping, additivity with carries into the high word, the kernel's
row tables against the columns they are transposed from, the phase bound.  Nothing is loaded into this process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_jump_ahead_and_phase_run_clean_under_the_sanitizers(tmp_path):
    prog = str(tmp_path / "siggen_check_san")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wall",
                    "-I", os.path.join(ROOT, "ka9q-radio_amd", "csrc"), os.path.join(ROOT, "tests", "c", "siggen_check.cpp"), "-o", prog, "-lpthread"], check=True)
    env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD"}
    r = subprocess.run([prog, "selftest"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "siggen_check: ok" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.stdout[-2000:], r.stderr[-3000:])
