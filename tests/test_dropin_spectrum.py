"""ka9q_hip_spectrum() of the filter.h drop-in (include/ka9q_filter_hip_ext.h): wideband_poll() (src/spectrum.c:308-522) computed on
the device from the samples the master's device ring holds.  libka9q_filter_hip.so is driven by ctypes from a child process: a real
master is created, several blocks are fed through write_rfilter(), the analyser is called; the bins must equal the float64 restatement
of wideband_poll() (tests/test_gpu_welch.py) applied to the samples fed, at that file's tolerance.  A small inline master has no device
ring: -1."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_welch import welch_ref, kaiser_window, compare, avg_limit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ka9q-radio_amd")
LIBDIR = os.environ.get("KA9Q_TEST_LIBDIR", PKG)       # tests/test_welch_emulated.py: the drop-in linked with the CPU build of the engine

pytestmark = pytest.mark.gpu

_CHILD = r"""
import ctypes as C, sys
import numpy as np
lib = C.CDLL(sys.argv[1])
out, L, M, nblocks, fft_n, shift, bin_count, fft_avg, overlap = sys.argv[2], *[int(v) for v in sys.argv[3:10]], float(sys.argv[10])
vp = C.c_void_p
lib.create_filter_input.argtypes = [vp, C.c_int, C.c_int, C.c_int]
lib.write_rfilter.argtypes = [vp, vp, C.c_int]
lib.delete_filter_input.argtypes = [vp]
lib.ka9q_hip_spectrum.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_double, vp, vp]
master = C.create_string_buffer(4096)                  # struct filter_in (include/ka9q_filter_abi.h), opaque here
x = np.load(out + "/x.npy"); win = np.load(out + "/win.npy")
assert lib.create_filter_input(master, L, M, 2) == 0   # REAL
for b in range(nblocks):
    blk = np.ascontiguousarray(x[b * L:(b + 1) * L])
    assert lib.write_rfilter(master, blk.ctypes.data, L) >= 0
bins = np.zeros(bin_count, np.float32); mm = np.zeros(2, np.float64)
eff = lib.ka9q_hip_spectrum(master, fft_n, win.ctypes.data, shift, bin_count, fft_avg, overlap, bins.ctypes.data, mm.ctypes.data)
again = np.zeros(bin_count, np.float32)
eff2 = lib.ka9q_hip_spectrum(master, fft_n, win.ctypes.data, shift, bin_count, fft_avg, overlap, again.ctypes.data, None)
assert eff2 == eff and np.array_equal(again, bins)     # the cached bank, the same bits
# a small inline master (radiod's filter2) has no device ring
mini = C.create_string_buffer(4096)
assert lib.create_filter_input(mini, 480, 481, 1) == 0
small = np.zeros(8, np.float32)
rc_mini = lib.ka9q_hip_spectrum(mini, 64, np.ones(64, np.float32).ctypes.data, 0, 8, 1, 0.0, small.ctypes.data, None)
lib.delete_filter_input(mini)
lib.delete_filter_input(master)
np.save(out + "/bins.npy", bins); np.save(out + "/mm.npy", mm); np.save(out + "/rc.npy", np.array([eff, rc_mini]))
"""


def _build_lib():
    if LIBDIR == PKG:
        subprocess.run(["make", "-s", "-C", os.path.join(PKG, "csrc"), "all"], check=True)


@pytest.mark.parametrize("fft_n,shift,bin_count,fft_avg,overlap", [(6480, 1000, 1620, 8, 0.5), (12960, -3000, 1621, 100, 0.75), (18514, 2000, 800, 3, 0.0)])
def test_dropin_spectrum_matches_the_restated_reference(tmp_path, fft_n, shift, bin_count, fft_avg, overlap):
    _build_lib()
    L, M, nblocks = 25920, 6481, 11
    R = 8 * L                                                                          # the engine's default device ring: 8 blocks
    rng = np.random.default_rng(4)
    t = np.arange(nblocks * L)
    x = (0.2 * np.cos(2 * np.pi * 0.11 * t) + 0.05 * np.cos(2 * np.pi * 0.3127 * t) + 0.02 * rng.standard_normal(t.size)).astype(np.float32)
    win = kaiser_window(fft_n, 7.0)
    np.save(tmp_path / "x.npy", x); np.save(tmp_path / "win.npy", win)
    script = tmp_path / "child.py"; script.write_text(_CHILD)
    r = subprocess.run([sys.executable, str(script), os.path.join(LIBDIR, "libka9q_filter_hip.so"), str(tmp_path), str(L), str(M), str(nblocks),
                        str(fft_n), str(shift), str(bin_count), str(fft_avg), repr(overlap)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    bins, mm, rc = np.load(tmp_path / "bins.npy"), np.load(tmp_path / "mm.npy"), np.load(tmp_path / "rc.npy")
    # the device ring as those blocks left it: the first sample lands on index M - 1 (src/filter.c:244)
    ring = np.zeros(R, np.float32)
    ring[(M - 1 + t) % R] = x                                                          # later samples overwrite earlier ones, as on the device
    end = (M - 1 + t.size) % R
    want, mn, mx, eff = welch_ref(ring, end, True, fft_n, win, shift, bin_count, fft_avg, overlap)
    assert rc[0] == eff == min(fft_avg, avg_limit(R, fft_n, overlap)) and rc[1] == -1
    compare(bins, want, "drop-in fft_n=%d" % fft_n)
    assert mm[0] == bins.min() and mm[1] == bins.max()
