"""ka9q_hip_spectrum_narrow() of the filter.h drop-in (include/ka9q_filter_hip_ext.h): narrowband_poll() (src/spectrum.c:206-306)
computed on the device from the rows a COMPLEX slave's channel leaves there.  libka9q_filter_hip.so is driven by ctypes from a child
process: a real master and a COMPLEX slave with zero remainder (the drop-in's banks are untuned), the analyser attached by its first call
(zeros: a fresh ring), a known number of blocks fed through write_rfilter() and taken with execute_filter_output(), then the analyser
called; the bins must equal the float64 restatement (nb_ref, tests/test_gpu_welch_narrow.py) applied to the samples
execute_filter_output() delivered, at that file's tolerance (relative L2 <= 1e-5, every bin within 1e-5 of the strongest).  -1: a slave of
an inline master, a REAL slave, and -- without a GPU -- the drop-in linked with the stub engine (tests/stub/chz_stub.cpp), which has no analyser."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from test_gpu_welch import compare, kaiser_window
from test_gpu_welch_narrow import nb_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ka9q-radio_amd")
CSRC = os.path.join(PKG, "csrc")
LIBDIR = os.environ.get("KA9Q_TEST_LIBDIR", PKG)       # tests/test_welch_narrow_emulated.py: the drop-in linked with the CPU build of the engine

_CHILD = r"""
import ctypes as C, sys
import numpy as np
lib = C.CDLL(sys.argv[1])
out, L, M, olen, nblocks, shift, fft_n, bin_count, fft_avg, overlap = sys.argv[2], *[int(v) for v in sys.argv[3:11]], float(sys.argv[11])
vp = C.c_void_p
lib.create_filter_input.argtypes = [vp, C.c_int, C.c_int, C.c_int]
lib.create_filter_output.argtypes = [vp, vp, C.c_int, C.c_int]
lib.set_filter.argtypes = [vp, C.c_double, C.c_double, C.c_double]
lib.execute_filter_output.argtypes = [vp, C.c_int]
lib.write_rfilter.argtypes = [vp, vp, C.c_int]
lib.delete_filter_input.argtypes = [vp]; lib.delete_filter_output.argtypes = [vp]
lib.ka9q_hip_spectrum_narrow.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.c_double, vp, vp]
COMPLEX, REAL = 1, 2
x = np.load(out + "/x.npy"); win = np.load(out + "/win.npy")
master = C.create_string_buffer(4096); slave = C.create_string_buffer(4096); rslave = C.create_string_buffer(4096)   # opaque here (include/ka9q_filter_abi.h)
assert lib.create_filter_input(master, L, M, REAL) == 0
assert lib.create_filter_output(slave, master, olen, COMPLEX) == 0 and lib.set_filter(slave, -0.4, 0.4, 11.0) == 0
bins = np.zeros(bin_count, np.float32); mm = np.ones(2, np.float64)
def narrow(s, into, m):
    return lib.ka9q_hip_spectrum_narrow(s, fft_n, win.ctypes.data, bin_count, fft_avg, overlap, into.ctypes.data, m.ctypes.data if m is not None else None)
rc = [narrow(slave, bins, mm)]                          # attaches; the fresh ring is zeros
if rc[0] == -1:                                         # an engine library without the analyser (the stub)
    np.save(out + "/rc.npy", np.array(rc)); sys.exit(0)
assert rc[0] == fft_avg and not bins.any() and mm[0] == 0 and mm[1] == 0
hist = []
for b in range(nblocks):
    blk = np.ascontiguousarray(x[b * L:(b + 1) * L])
    assert lib.write_rfilter(master, blk.ctypes.data, L) >= 0
    assert lib.execute_filter_output(slave, shift) == 0
    p = C.cast(C.addressof(slave) + 136, C.POINTER(C.c_void_p))[0]          # slave->output.c
    hist.append(np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_float)), (2 * olen,)).copy().view(np.complex64))
rc.append(narrow(slave, bins, mm))
again = np.zeros(bin_count, np.float32)
rc.append(narrow(slave, again, None))
assert np.array_equal(again, bins)                      # the cached analyser and window, the same bits
assert lib.create_filter_output(rslave, master, olen, REAL) == 0
rc.append(narrow(rslave, again, None))                  # a REAL slave
mini = C.create_string_buffer(4096); mslave = C.create_string_buffer(4096)
assert lib.create_filter_input(mini, 480, 481, COMPLEX) == 0 and lib.create_filter_output(mslave, mini, 480, COMPLEX) == 0
rc.append(narrow(mslave, again, None))                  # the same-size slave of a small inline master (radiod's filter2)
lib.delete_filter_output(mslave); lib.delete_filter_input(mini)
lib.delete_filter_output(rslave); lib.delete_filter_output(slave); lib.delete_filter_input(master)
np.save(out + "/hist.npy", np.concatenate(hist)); np.save(out + "/bins.npy", bins); np.save(out + "/mm.npy", mm); np.save(out + "/rc.npy", np.array(rc))
"""

L_, M_, OLEN = 25920, 6481, 240


def _run(tmp_path, libdir, nblocks, shift, fft_n, bin_count, fft_avg, overlap, env=None):
    rng = np.random.default_rng(5)
    t = np.arange(nblocks * L_)
    f0 = shift * 40.0 / 1.296e6                                                       # bin `shift` of the 40 Hz forward transform: the channel's centre
    x = (0.2 * np.cos(2 * np.pi * (f0 + 1.1e-3) * t) + 0.05 * np.cos(2 * np.pi * (f0 - 2.3e-3) * t) + 0.02 * rng.standard_normal(t.size)).astype(np.float32)
    np.save(tmp_path / "x.npy", x); np.save(tmp_path / "win.npy", kaiser_window(fft_n, 7.0))
    script = tmp_path / "child.py"; script.write_text(_CHILD)
    r = subprocess.run([sys.executable, str(script), os.path.join(libdir, "libka9q_filter_hip.so"), str(tmp_path), str(L_), str(M_), str(OLEN), str(nblocks),
                        str(shift), str(fft_n), str(bin_count), str(fft_avg), repr(overlap)], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    return np.load(tmp_path / "rc.npy")


@pytest.mark.gpu
@pytest.mark.parametrize("nblocks,fft_n,bin_count,fft_avg,overlap", [(6, 300, 128, 3, 0.5), (11, 1000, 1000, 8, 0.75), (9, 75, 74, 8, 0.5)])
def test_dropin_narrowband_spectrum_matches_the_restated_reference(tmp_path, nblocks, fft_n, bin_count, fft_avg, overlap):
    if LIBDIR == PKG:
        subprocess.run(["make", "-s", "-C", CSRC, "all"], check=True)
    rc = _run(tmp_path, LIBDIR, nblocks, 2500, fft_n, bin_count, fft_avg, overlap)    # shift 2500 = 250 bins of the 400 Hz channel grid: remainder zero
    hist, bins, mm = np.load(tmp_path / "hist.npy"), np.load(tmp_path / "bins.npy"), np.load(tmp_path / "mm.npy")
    assert hist.size == nblocks * OLEN and np.abs(hist).max() > 0.01
    want, mn, mx = nb_ref(hist, fft_n, kaiser_window(fft_n, 7.0), bin_count, fft_avg, overlap)
    assert list(rc) == [fft_avg, fft_avg, fft_avg, -1, -1]                            # attach, poll, poll again, REAL slave, inline master
    compare(bins, want, "drop-in narrowband fft_n=%d" % fft_n)
    assert mm[0] == bins.min() and mm[1] == bins.max()


def test_dropin_narrowband_spectrum_reports_minus_one_on_the_stub_engine(tmp_path):
    """the drop-in binds the analyser's engine calls weakly: linked with an engine library that lacks them it answers -1"""
    import oracle_lib as ol
    ol.build()
    libdir = tempfile.mkdtemp(prefix="nb_stub_", dir=str(tmp_path))
    subprocess.run(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", os.path.join(ROOT, "tests", "stub", "chz_stub.cpp"), "-o", os.path.join(libdir, "libchz_hip.so"),
                    "-L", os.path.join(ROOT, "oracle"), "-loracle", "-Wl,-rpath," + os.path.join(ROOT, "oracle"), "-lpthread"], check=True)
    subprocess.run(["gcc", "-O1", "-std=gnu11", "-fPIC", "-shared", os.path.join(CSRC, "filter_hip.c"), "-o", os.path.join(libdir, "libka9q_filter_hip.so"),
                    "-L", libdir, "-lchz_hip", "-Wl,-rpath,$ORIGIN", "-lm", "-lpthread"], check=True)
    rc = _run(tmp_path, libdir, 1, 2500, 64, 64, 1, 0.0)
    assert list(rc) == [-1]
