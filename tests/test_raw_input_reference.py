"""Pins tests/raw_oracle.py -- the checker of chz_input_write_raw (tests/test_gpu_raw_input.py) -- to the reference's own conversion code,
compiled into tmp_path with the reference's release flags (oracle/Makefile's REF_CFLAGS) and never committed.

PACKED12: src/airspy-unpack.c alone, as a library; airspy_unpack() and, where the CPU has AVX2, airspy_unpack_avx2() on the GPU test's own
input (all 4096 codes in every one of a group's 8 places, then a random fill): output bits, energy and overrange count equal the
restatement's.

The integer formats of src/hydrasdr.c's rx_callback(), and its RAW case: tests/c/ref_hydrasdr_wrap.c #includes hydrasdr.c where it lies and is
built as a program against tests/c/shims/libhydrasdr/hydrasdr.h (declarations only; oracle/shims has iniparser's).  One callback per case of
the GPU test, on that test's own input: the floats and frontend->overranges equal the restatement's exactly, and the energy recovered from
frontend->if_power (started at 0: Power_alpha * energy / n) to 1e-15 relative."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import raw_oracle as ro
import test_gpu_raw_input as tg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE = os.path.join(ROOT, "oracle")


def makefile_var(name):
    with open(os.path.join(ORACLE, "Makefile")) as f:
        m = re.search(r"^%s\s*\??=\s*(.*)$" % name, f.read(), re.M)
    return m.group(1).strip()


REF = os.environ.get("REF", makefile_var("REF"))
needs_ref = pytest.mark.skipif(not os.path.isfile(os.path.join(REF, "hydrasdr.c")), reason="the reference tree is not here")
# hydrasdr.c's Sample_type_name[] order
SAMPLE_TYPE = {ro.S16_IQ: 2, ro.S16: 3, ro.U16: 4, ro.PACKED12: 5, ro.S8_IQ: 6, ro.U8_IQ: 7, ro.S8: 8, ro.U8: 9}


def aligned(n, dtype, align=32):
    """a zeroed array of n items whose first byte sits on an `align`-byte boundary"""
    raw = np.zeros(n * np.dtype(dtype).itemsize + align, np.uint8)
    off = (-raw.ctypes.data) % align
    return raw[off:off + n * np.dtype(dtype).itemsize].view(dtype)


@pytest.fixture(scope="module")
def refunpack(tmp_path_factory):
    work = str(tmp_path_factory.mktemp("refunpack"))
    lib = os.path.join(work, "libref_airspy_unpack.so")
    # compiled with the reference's flags, linked without them (as oracle/Makefile links _ref/): linking a library with the unsafe-math flags
    # would pull in the start-up code that switches subnormals off in whatever process loads it -- this one
    subprocess.run(["gcc"] + makefile_var("REF_CFLAGS").split() + ["-iquote", REF, "-c", os.path.join(REF, "airspy-unpack.c"), "-o", "airspy-unpack.o"], check=True, cwd=work)
    subprocess.run(["gcc", "-shared", "-o", lib, "airspy-unpack.o"], check=True, cwd=work)
    L = C.CDLL(lib)
    for name in ("airspy_unpack", "airspy_unpack_avx2"):
        if hasattr(L, name):
            getattr(L, name).argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.POINTER(C.c_uint64)]
    return L


@pytest.fixture(scope="module")
def refhydra(tmp_path_factory):
    work = str(tmp_path_factory.mktemp("refhydra"))
    prog = os.path.join(work, "ref_hydrasdr")
    srcs = [os.path.join(ROOT, "tests", "c", "ref_hydrasdr_wrap.c"), os.path.join(REF, "airspy-unpack.c")]
    git = ['-DGIT_%s="none"' % k for k in ("HASH", "BRANCH", "DATE", "VERSION", "REMOTE_URL")]
    subprocess.run(["gcc"] + makefile_var("REF_CFLAGS").split() + git + ["-I", os.path.join(ROOT, "tests", "c", "shims"), "-I", os.path.join(ORACLE, "shims"),
                    "-iquote", REF, "-ffunction-sections", "-fdata-sections", "-c"] + srcs, check=True, cwd=work)
    objs = [os.path.join(work, os.path.basename(f)[:-2] + ".o") for f in srcs]
    subprocess.run(["gcc", "-o", prog] + objs + ["-Wl,--gc-sections", "-lm", "-lpthread"], check=True)
    return prog


def has_avx2():
    try:
        with open("/proc/cpuinfo") as f:
            flags = f.read()
    except OSError:
        return False
    return " avx2" in flags and " popcnt" in flags


@needs_ref
def test_packed12_equals_airspy_unpack(refunpack):
    n = tg.raw_total(ro.PACKED12)
    raw = tg.raw_input(ro.PACKED12, 12, n)
    x = ro.integers(ro.PACKED12, raw, n)
    for place in range(8):
        assert np.array_equal(np.unique(x[place::8]), np.arange(-2048, 2048))
    want, energy, clip_s, clip_c = ro.convert(ro.PACKED12, raw, n, tg.SCALE)
    assert clip_s == clip_c
    words = aligned(raw.size // 4 + 4, np.uint32)
    words[:raw.size // 4] = raw.view("<u4")
    routines = ["airspy_unpack"] + (["airspy_unpack_avx2"] if has_avx2() and hasattr(refunpack, "airspy_unpack_avx2") else [])
    for name in routines:
        out = aligned(n, np.float32)
        en = C.c_uint64(0)
        over = getattr(refunpack, name)(out.ctypes.data, words.ctypes.data, n, C.c_float(np.float32(tg.SCALE)), C.byref(en))
        assert tg.same_bits(out, want), name
        assert (en.value, over) == (energy, clip_s), name
    print("PACKED12: %s equal the restatement on %d samples (energy %d, %d overranges)" % (" and ".join(routines), n, energy, clip_s))


@needs_ref
@pytest.mark.parametrize("fmt,bits", tg.CASES, ids=tg.IDS)
def test_the_integer_formats_equal_rx_callback(refhydra, tmp_path, fmt, bits):
    n = tg.raw_total(fmt)
    raw = tg.raw_input(fmt, bits, n)
    want, energy, clip_s, _ = ro.convert(fmt, raw, n, tg.SCALE, bits)
    src, dst = str(tmp_path / "raw.bin"), str(tmp_path / "floats.bin")
    raw.tofile(src)
    r = subprocess.run([refhydra, str(SAMPLE_TYPE[fmt]), str(bits), "0" if ro.is_iq(fmt) else "1", float(tg.SCALE).hex(), str(n), src, dst],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-1500:])
    over, if_power, alpha = r.stdout.split()
    got = np.fromfile(dst, np.float32)
    assert got.size == want.size and tg.same_bits(got, want)
    assert int(over) == clip_s
    ref_energy = float(if_power) * n / float(alpha)
    assert abs(ref_energy - energy) <= 1e-15 * energy, (ref_energy, energy)
