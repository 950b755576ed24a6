"""The host half of the device-side sig_gen front end: chz_siggen_jump and chz_siggen_seed against the reference's own generator
(xoshiro256ss_next / _seed / _jump of src/gauss.c, compiled unmodified into oracle/_ref/libka9q_ref.so), the carrier phase of
ka9q-radio_amd/csrc/chz_siggen.h against rational arithmetic, and the pins tests/test_gpu_siggen.py stands on: tests/siggen_oracle.py's
restatement of the Gaussian equals the checker's floats bit for bit, and the checker equals the reference's loop at the GPU test's parameters."""
import ctypes as C
import fractions
import os
import random
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
import siggen_oracle as so
from conftest import load_pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_ref = pytest.mark.skipif(not ol.have_ref(), reason="oracle/_ref not built (needs the reference tree)")
COUNTS = (0, 1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 10 ** 6 + 7)
SEEDS = (1, 0, 0x123456789abcdef, (1 << 64) - 1)


class RefState(C.Structure):
    _fields_ = [("s", C.c_uint64 * 4)]


@pytest.fixture(scope="module")
def E():
    import __graft_entry__ as ge
    if not os.path.exists(os.path.join(ROOT, "ka9q-radio_amd", "libchz_hip.so")):
        ge.build()
    return load_pkg().engine


@pytest.fixture(scope="module")
def ref(oracle_built):
    L = ol.ref()
    L.xoshiro256ss_seed.argtypes = [C.POINTER(RefState), C.c_uint64]
    L.xoshiro256ss_next.argtypes = [C.POINTER(RefState)]; L.xoshiro256ss_next.restype = C.c_uint64
    L.xoshiro256ss_jump.argtypes = [C.POINTER(RefState)]
    return L


@needs_ref
@pytest.mark.parametrize("seed", SEEDS)
def test_seed_and_jump_equal_the_reference_s_sequential_stepping(E, ref, seed):
    st = RefState()
    ref.xoshiro256ss_seed(C.byref(st), seed)
    s0 = E.siggen_seed(seed)
    assert s0 == tuple(st.s) == so.seed(seed)
    done = 0
    for d in COUNTS:
        for _ in range(d - done):
            ref.xoshiro256ss_next(C.byref(st))
        done = d
        assert E.siggen_jump(s0, d) == tuple(st.s), d
    # the numpy restatement steps as the reference does
    st2 = RefState()
    ref.xoshiro256ss_seed(C.byref(st2), seed)
    want = [ref.xoshiro256ss_next(C.byref(st2)) for _ in range(300)]
    got, after = so.draws(s0, 300)
    assert got.tolist() == want and after == tuple(st2.s)


def test_jumps_add_with_carries_into_the_high_word(E):
    rng = random.Random(5)
    for i in range(24):
        a, b = rng.getrandbits(64) | 1 << 63, rng.getrandbits(64) | 1 << 63         # a + b carries
        a |= rng.getrandbits(60) << 64; b |= rng.getrandbits(60) << 64
        s = E.siggen_seed(i)
        assert E.siggen_jump(E.siggen_jump(s, a), b) == E.siggen_jump(s, a + b), (a, b)
        lo = (C.c_ulonglong * 4)(*s)
        assert E.lib().chz_siggen_jump(C.byref(lo), (a + b) & (1 << 64) - 1, (a + b) >> 64) == 0 and tuple(lo) == E.siggen_jump(s, a + b)
    assert E.siggen_jump(E.siggen_seed(1), 0) == E.siggen_seed(1)


@needs_ref
@pytest.mark.parametrize("seed", SEEDS)
def test_two_jumps_of_2_to_the_127_equal_the_reference_s_own_jump(E, ref, seed):
    st = RefState()
    ref.xoshiro256ss_seed(C.byref(st), seed)
    ref.xoshiro256ss_jump(C.byref(st))
    s = E.siggen_seed(seed)
    assert E.siggen_jump(E.siggen_jump(s, 1 << 127), 1 << 127) == tuple(st.s)


@pytest.fixture(scope="module")
def siggen_check(tmp_path_factory):
    prog = str(tmp_path_factory.mktemp("siggen_check") / "siggen_check")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "ka9q-radio_amd", "csrc"),
                    os.path.join(ROOT, "tests", "c", "siggen_check.cpp"), "-o", prog, "-lpthread"], check=True)
    return prog


def test_the_carrier_phase_is_within_2_to_the_minus_52_of_the_exact_product(siggen_check):
    ns = (0, 1, (1 << 20) + 3, (1 << 40) + 12345, (1 << 53) - 1)
    cases = [(so.step_cycles(f), n) for f in so.FREQS for n in ns]
    args = [x for a, n in cases for x in (float(a).hex(), str(n))]
    out = subprocess.run([siggen_check, "phase"] + args, capture_output=True, text=True, check=True, timeout=60).stdout.split()
    assert len(out) == len(cases)
    worst = fractions.Fraction(0)
    for (a, n), text in zip(cases, out):
        phi = float.fromhex(text)
        assert 0.0 <= phi <= 1.0
        d = abs(fractions.Fraction(phi) - so.exact_phase(a, n))
        d = min(d, 1 - d)                                   # an angle: 1.0 is 0
        worst = max(worst, d)
        assert d <= fractions.Fraction(1, 1 << 52), (a, n, phi, float(d))
    print("worst phase error %.3g cycles" % float(worst))
    # the step the engine takes for a frequency is the angle of the phasor the reference's set_osc makes: within a rounding of freq mod 1
    for f in so.FREQS:
        a = so.step_cycles(f)
        assert -0.5 <= a < 0.5 and abs((a - f + 0.5) % 1.0 - 0.5) <= 2.0 ** -52


@pytest.mark.parametrize("isreal", [True, False], ids=["real", "complex"])
def test_the_restated_gaussian_is_the_checker_s(oracle_built, isreal):
    """floats bit for bit: noise only, and a carrier that stands still plus noise"""
    n = 5000
    for amplitude in (0.0, 0.1):
        want = so.reference_stream(0.0, amplitude, 0.01, isreal, n)
        got = so.to_ring(so.samples_f0(so.seed(1), n, amplitude, 0.01, isreal), so.SCALE[isreal])
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert so.SCALE[True] == pytest.approx(1.41254, abs=1e-5) and so.SCALE[False] == 1.0


@needs_ref
@pytest.mark.parametrize("isreal", [True, False], ids=["real", "complex"])
@pytest.mark.parametrize("fi", range(len(so.FREQS)))
def test_the_checker_is_the_reference_s_loop_at_these_parameters(oracle_built, fi, isreal):
    """oracle_lib.SigGen against oracle_lib.RefSigGen (the reference's osc.c and gauss.c behind sig_gen's two statements) over 2^18 samples:
    the noise alone bit for bit, with the carrier to a float's rounding"""
    f, n = so.FREQS[fi], 1 << 18
    a = ol.SigGen(f, 0.0, 0.01, so.SCALE[isreal], isreal, seed=1).generate(n)
    b = ol.RefSigGen(f, 0.0, 0.01, so.SCALE[isreal], isreal, seed=1).generate(n)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    x = so.reference_stream(f, 0.1, 0.01, isreal, n)
    y = ol.RefSigGen(f, 0.1, 0.01, so.SCALE[isreal], isreal, seed=1).generate(n)
    xf, yf = x.view(np.float32), y.view(np.float32)
    assert np.abs(xf - yf).max() <= 2.0 ** -24 * 0.2 and np.mean(xf == yf) > 0.99
