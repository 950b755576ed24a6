"""Pins tests/afsk_oracle.py -- the checker of every device test of the packet decoder pool -- to the reference's own src/packetd.c.

tests/c/ref_packetd_wrap.c #includes the reference's packetd.c where it lies (main renamed, send() redirected into a buffer) and runs its
decode_task() over a file of samples; it is compiled into tmp_path with the reference's release flags (oracle/Makefile's REF_CFLAGS) together
with the reference's filter window misc sched sincospi osc gauss rtp ax25 and the oracle's FFT provider (oracle/_build/fftw_shim.o, dft_ref.o).
The wrapper runs the reference's transform in the task's own thread (N_worker_threads = 0): with filter.c's worker thread the first block of a
task is gathered without waiting for its transform (src/filter.c:224,681-683), and on a busy machine the task then decodes nothing at all.

Inputs: the strict instances 0-2 of tests/test_gpu_afsk.py's scenario at 48 and 24 kHz (packetd's block is 960 samples whatever the rate).
The restatement's frames -- byte sequences and order -- must equal the reference's on its float64 transform and on its float32 one
(oracle_fft_set_precision), and the restatement's f32 twin must deliver them too.
Input condition, asserted first: every decision of these inputs carries both margins above FLOOR = 100 x the largest distance between the
restatement's float64 and float32 runs on cur_val, relative to the largest |cur_val| -- measured 1.04e-5 to 1.14e-5 on these six inputs
(test_gpu_afsk.input_condition, which also says which decisions cannot carry a margin and why)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import afsk_oracle as ao
import oracle_lib as ol
import test_gpu_afsk as tg
import test_gpu_afsk_rates            # noqa: F401  (registers its shapes with test_gpu_afsk)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE = os.path.join(ROOT, "oracle")
RTP_HEADER = 12                         # hton_rtp() without CSRCs or extension


def makefile_var(name):
    with open(os.path.join(ORACLE, "Makefile")) as f:
        m = re.search(r"^%s\s*\??=\s*(.*)$" % name, f.read(), re.M)
    return m.group(1).strip()


REF = os.environ.get("REF", makefile_var("REF"))
needs_ref = pytest.mark.skipif(not os.path.isfile(os.path.join(REF, "packetd.c")), reason="the reference tree is not here")


@pytest.fixture(scope="module")
def refpkt(tmp_path_factory):
    ol.build()                          # oracle/_build/fftw_shim.o and dft_ref.o
    work = str(tmp_path_factory.mktemp("refpkt"))
    lib = os.path.join(work, "libref_packetd.so")
    srcs = [os.path.join(REF, f + ".c") for f in "filter window misc sched sincospi osc gauss rtp ax25".split()] + [os.path.join(ROOT, "tests", "c", "ref_packetd_wrap.c")]
    git = ['-DGIT_%s="none"' % k for k in ("HASH", "BRANCH", "DATE", "VERSION", "REMOTE_URL")]
    # compiled with the reference's flags, linked without them (as oracle/Makefile links _ref/): a link with -funsafe-math-optimizations brings in
    # crtfastmath.o, which would switch the whole test process to flush-to-zero when the library is loaded
    subprocess.run(["gcc"] + makefile_var("REF_CFLAGS").split() + git + ["-I", os.path.join(ORACLE, "shims"), "-iquote", REF, "-ffunction-sections",
                    "-fdata-sections", "-fvisibility=hidden", "-c"] + srcs, check=True, cwd=work)
    objs = [os.path.join(work, os.path.basename(f)[:-2] + ".o") for f in srcs]
    subprocess.run(["gcc", "-shared", "-o", lib] + objs + [os.path.join(ORACLE, "_build", "fftw_shim.o"), os.path.join(ORACLE, "_build", "dft_ref.o"),
                    "-Wl,--gc-sections", "-l:libbsd.so.0", "-lm", "-lpthread"], check=True)
    L = C.CDLL(lib)
    L.refpkt_run.argtypes = [C.c_char_p, C.c_int, C.c_void_p, C.c_long, C.c_void_p, C.c_int]
    L.oracle_fft_set_precision.argtypes = [C.c_int]
    L.refpkt_set_bitrate.argtypes = [C.c_double]
    L.refpkt_set_bitrate.restype = None
    return L


def reference_frames(refpkt, path, samprate, f32, bitrate=ao.BITRATE):
    out = np.zeros(1 << 16, np.uint8)
    lens = np.zeros(64, np.int32)
    refpkt.oracle_fft_set_precision(int(f32))
    refpkt.refpkt_set_bitrate(bitrate)
    try:
        n = refpkt.refpkt_run(path.encode(), int(samprate), out.ctypes.data, out.size, lens.ctypes.data, lens.size)
    finally:
        refpkt.oracle_fft_set_precision(0)
        refpkt.refpkt_set_bitrate(ao.BITRATE)
    assert 0 <= n <= lens.size, n
    at, frames = 0, []
    for k in range(n):
        frames.append(out[at + RTP_HEADER:at + lens[k]].tobytes())
        at += int(lens[k])
    return frames


@needs_ref
@pytest.mark.parametrize("shape", ["48k", "24k"])
def test_the_restatement_s_frames_equal_the_reference_s(refpkt, tmp_path, shape):
    L, M, fs = tg.SHAPES[shape]
    assert (L, M) == (960, 961)         # AL, AM of src/packetd.c:52-53
    blocks, want = tg.scenario(shape)
    for k in (0, 1, 2):
        floor, m1, m2, _ = tg.input_condition(shape, k)
        mine, twin = ao.frames_of(tg.restatement(shape, False)[k]), ao.frames_of(tg.restatement(shape, True)[k])
        assert mine == want[k] and twin == want[k], (shape, k)
        path = str(tmp_path / ("inst%d.s16be" % k))
        ao.to_wire(blocks[k].reshape(-1), big_endian=True).tofile(path)
        for f32 in (False, True):
            ref = reference_frames(refpkt, path, fs, f32)
            assert ref == mine, (shape, k, "float32 transform" if f32 else "float64 transform", [len(f) for f in ref], [len(f) for f in mine])
        print("%s instance %d: %d frames equal on both transforms; FLOOR %.3g, smallest margins %.3g / %.3g" % (shape, k, len(mine), floor, m1, m2))


@needs_ref
@pytest.mark.parametrize("shape", ["22k", "22k1225", "ref300"])
def test_the_restatement_s_frames_equal_the_reference_s_where_a_bit_is_no_whole_number_of_samples(refpkt, tmp_path, shape):
    """tests/test_gpu_afsk_rates.py's scenario (frames of 1, 17, 64 and 330 payload bytes, equal tones and the space tone 1.8 x the mark tone) at
    22050 / 1200 (samppbit 18 of 18.375: the reference's clock slips, and the restatement must lose the same frames in the same order), at 22050 /
    1225 (exactly 18: the control, all four frames) and at 16000 / 300 (53 of 53.33) with the tones packetd.c fixes; the wrapper sets packetd.c's
    file static Bitrate before the task starts.  The other shapes of that file (tones of 1600 / 1800 Hz, L 480, M - 1 != L: packetd.c's tones are
    const and its AL / AM fixed) rest on the restatement's parametrisation.
    Measured: 22k delivers the frames of [1, 17] payload bytes with one CRC failure at equal tones and [17, 64, 330] with the space tone raised;
    22k1225 delivers all four; ref300 (53 of 53.33 samples a bit, a clock that runs 0.6 % fast over frames of up to 2700 bits) delivers [1, 64] with
    five CRC failures at equal tones and [17, 64, 330] with the space tone raised -- the reference loses the same ones; FLOOR 0.8e-5 to 1.3e-5."""
    L, M, fs, br, mk, sp = tg.geom(shape)
    assert (L, M, mk, sp) == (960, 961, 1200.0, 2200.0)      # AL, AM, mark_tone, space_tone of src/packetd.c
    blocks, want = tg.scenario(shape)
    for k in (0, 1):
        floor, m1, m2, _ = tg.input_condition(shape, k)
        mine, twin = ao.frames_of(tg.restatement(shape, False)[k]), ao.frames_of(tg.restatement(shape, True)[k])
        assert twin == mine and len(mine) >= 1 and all(f in want[k] for f in mine), (shape, k, [len(f) for f in mine])
        assert (mine == want[k]) == (shape == "22k1225"), (shape, k, [len(f) for f in mine])
        path = str(tmp_path / ("inst%d.s16be" % k))
        ao.to_wire(blocks[k].reshape(-1), big_endian=True).tofile(path)
        for f32 in (False, True):
            ref = reference_frames(refpkt, path, fs, f32, bitrate=br)
            assert ref == mine, (shape, k, "float32 transform" if f32 else "float64 transform", [len(f) for f in ref], [len(f) for f in mine])
        print("%s instance %d: frames of %s bytes, equal on both transforms; FLOOR %.3g, smallest margins %.3g / %.3g" % (shape, k, [len(f) for f in mine], floor, m1, m2))


@needs_ref
def test_the_feeder_s_flush_rule_is_the_reference_s(refpkt, tmp_path):
    """instance 3 of the 48 kHz scenario: the reference reads the raw input and pads by its own rule (:540-546), the restatement runs on ao.feed()'s
    blocks.  Frames only: what the ring-down decides is rounding noise."""
    shape = "48k"
    L, M, fs = tg.SHAPES[shape]
    tx1, tx2, t1, t2 = tg.transmissions(shape)
    pad = lambda x: np.concatenate([x, np.zeros(-x.size % L, np.int16)])
    x3 = np.concatenate([pad(tx1), np.zeros(8 * L, np.int16), pad(tx2), np.zeros(L, np.int16)])
    assert np.array_equal(ao.feed(x3, L), tg.scenario(shape)[0][3])
    assert tg.decodes_from_every_clock_phase(shape)
    path = str(tmp_path / "inst3.s16be")
    ao.to_wire(x3, big_endian=True).tofile(path)
    mine = ao.frames_of(tg.restatement(shape, False)[3])
    for f32 in (False, True):
        assert reference_frames(refpkt, path, fs, f32) == mine == tg.scenario(shape)[1][3]
