"""Pools of AFSK / AX.25 packet decoders (chz_afsk_*, kernel afsk_ovs) away from 40, 20 and 10 samples a bit, against tests/afsk_oracle.py.

tests/test_gpu_afsk.py runs packetd's own rates (1200 bd, 1200 / 2200 Hz, M = L + 1, samprate / bitrate an integer).  afsk_check_geom takes any
(L, M, samprate, bitrate, mark, space) whose master rmini_check_geom takes, with at least 4 samples a bit, tones below Nyquist and at most 64
possible decisions a block.  The shapes here, through that file's helpers (run_pool, check_strict, input_condition, told the rates):
  22k     L 960, M 961   22050 / 1200 / 1200, 2200   samppbit = (int)18.375 = 18: a truncation.  Up to 54 of 64 decisions a block.  The reference's
                                                      clock runs 2 % fast and the Gardner step (one sample per transition) must make it up; it slips
  22k1225 L 960, M 961   22050 / 1225 / 1200, 2200   the control: exactly 18 samples a bit, every frame decodes
  hf300   L 960, M 961   16000 / 300 / 1600, 1800    samppbit 53 of 53.33, odd (half = 26), twist 0.889, tones 200 Hz apart
  11k     L 480, M 481   11025 / 1200 / 1200, 2200   samppbit 9 of 9.19, odd (half = 4); 60 decisions possible
  shortM  L 960, M 481   48000 / 1200 / 1200, 2200   N 1440: a history of 480 samples, shorter than the block
  longM   L 240, M 721   12000 / 1200 / 1200, 2200   N 960: a history of 720 samples, three blocks long; group delay 36 bit times
Each runs ONE strict scenario of two instances in a pool of capacity 2, the request order permuted per call: LEAD idle flags, frames of 1, 17,
64 and 330 payload bytes three flags apart, 40 flags; instance 0 with equal tones (amplitude 0.4), instance 1 with the space tone 1.8 x the
mark tone (amplitude 0.25).  The signal comes from afsk_oracle.modulate()'s true baud clock (sample n carries line bit floor(n bitrate /
samprate)).

Bounds and input condition: those of tests/test_gpu_afsk.py, through its check_strict() and input_condition(), unchanged -- every discrete
result equal on every block, last_val and mid_val within 1e-6 or 4 x the f32 twin's own distance (relative to the terms where the difference
cancels), every decision's margins above FLOOR = 100 x the twin's distance, asserted on the restatement before anything is compared; exempt
are the first decision of a session and those inside the first (M - 1) / 2 + samppbit samples, as there.

At 22k the reference's algorithm does not hold its clock, and that is the point of the case: the device must slip where the restatement
slips, block by block.  Not all frames are demanded there; equality with the restatement is, and the restatement must deliver at least one
frame and count at least one CRC failure (crc_failures on natural data).  tests/test_afsk_reference.py pins the restatement's frames to
packetd.c at 22050 / 1200, 22050 / 1225 and 16000 / 300 with the reference's 1200 / 2200 Hz tones (its tones are const, its AL / AM fixed at
960 / 961); hf300's tones, 11k, shortM and longM rest on the restatement's parametrisation.

Measured (restatement: FLOOR, smallest margins |cur last| / |(cur - last) mid| relative to the largest |cur_val|^2; MI355X: worst measured /
allowed of last_val, mid_val; instance 0, instance 1):
  22k      FLOOR 1.05e-5, 1.24e-5; margins 7.5e-4 / 1.4e-4, 6.0e-4 / 1.2e-4; 0.97, 0.42 and 0.39, 0.36; 54 decisions a block at most
           instance 0 delivers the frames of 1 and 17 payload bytes and counts one CRC failure (64 and 330 are lost), instance 1 delivers 17, 64 and 330 (1 is lost)
  22k1225  FLOOR 1.23e-5, 1.09e-5; margins 1.0e-3 / 4.7e-2, 1.7e-3 / 7.0e-5; 0.34, 0.49 and 0.41, 0.38; 54 decisions; all four frames
  hf300    FLOOR 1.12e-5, 1.23e-5; margins 1.5e-3 / 8.0e-5, 1.7e-4 / 3.4e-5; 0.49, 0.35 and 0.36, 0.34; 19 decisions; all four frames (45 flags in front:
           with 30 the 1-byte frame of instance 1 comes before the clock has settled and is lost, in the restatement)
  11k      FLOOR 1.20e-5, 1.13e-5; margins 4.7e-3 / 3.4e-5, 1.4e-2 / 1.2e-4; 0.43, 0.59 and 0.34, 0.39; 53 decisions; all four frames
  shortM   FLOOR 1.41e-5, 1.34e-5; margins 2.7e-4 / 1.5e-2, 8.8e-4 / 2.1e-4; 0.27, 0.51 and 0.45, 0.29; all four frames
  longM    FLOOR 1.41e-5, 1.25e-5; margins 0.11 / 0.082, 0.11 / 2.4e-4; 0.42, 0.60 and 0.38, 0.80; all four frames (60 flags in front)
Where the clock slips or drifts a decision can fall next to a bit edge, and last_val is then small against its terms (1 to 4 blocks of 22k, hf300 and
11k; never in tests/test_gpu_afsk.py, which asserts so).  The cancellation rule stays mid_val's alone: last_val is held relative to ITSELF on those blocks
too, and that is where the 0.97 comes from (0.51 at most on the CPU build of the engine, whose arithmetic rounds differently).

Also here: a frame longer than the HDLC's buffer beside a neighbour with a frame of its own open (test_a_frame_longer_than_the_buffer...),
and the refusals next to these shapes."""
import functools

import numpy as np
import pytest

import afsk_oracle as ao
import oracle_lib as ol
import test_gpu_afsk as ga
from conftest import load_pkg
from test_gpu_afsk import CAP, SENTINEL, STRIDE, buffers, check_strict, payloads, restatement, run_pool, status_dict, whole_blocks

pytestmark = pytest.mark.gpu

# name -> ((L, M, samprate, bitrate, mark, space), idle flags in front, samples dropped in front of instance 1)
SHAPES = {"22k": ((960, 961, 22050.0, 1200.0, 1200.0, 2200.0), 30, 0),
          "22k1225": ((960, 961, 22050.0, 1225.0, 1200.0, 2200.0), 30, 0),
          "hf300": ((960, 961, 16000.0, 300.0, 1600.0, 1800.0), 45, 0),       # (30 flags: the 1-byte frame of instance 1 comes before the clock has settled)
          "11k": ((480, 481, 11025.0, 1200.0, 1200.0, 2200.0), 30, 0),
          "shortM": ((960, 481, 48000.0, 1200.0, 1200.0, 2200.0), 30, 0),
          "longM": ((240, 721, 12000.0, 1200.0, 1200.0, 2200.0), 60, 0)}        # (the filter delays everything by 36 bit times: a longer lead)
# for tests/test_afsk_reference.py alone: 300 bd at 16 kHz with the tones packetd.c fixes (hf300's own tones cannot be given to the reference)
REFERENCE_ONLY = {"ref300": ((960, 961, 16000.0, 300.0, 1200.0, 2200.0), 71, 0)}       # (71 flags: of 30 .. 79 the lead with the widest margins on both instances)
SIZES = (1, 17, 64, 330)


def make_scenario(name):
    (L, M, fs, br, mk, sp), lead, offset = SHAPES[name] if name in SHAPES else REFERENCE_ONLY[name]
    pl = payloads(11, SIZES)
    items = [("flags", lead)]
    for p in pl:
        items += [("frame", p), ("flags", 3)]
    items += [("flags", 40)]
    bits = ao.line_bits(items)
    want = [p + ao.fcs(p) for p in pl]
    blocks = [whole_blocks(ao.modulate(bits, fs, br, mk, sp, amplitude=0.4), L),
              whole_blocks(ao.modulate(bits, fs, br, mk, sp, amplitude=0.25, space_gain=1.8, offset=offset), L)]
    return blocks, [want, want]


for _name, _shape in list(SHAPES.items()) + list(REFERENCE_ONLY.items()):
    ga.register(_name, _shape[0], functools.partial(make_scenario, _name))


@pytest.fixture(scope="module")
def pkg():
    p = load_pkg()
    if p.engine.lib().chz_device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests cannot run (there is no CPU fallback)")
    ol.build()
    return p


_device_runs = {}


def device_run(pkg, shape):
    if shape not in _device_runs:
        _device_runs[shape] = run_pool(pkg, shape, CAP, only=(0, 1))
    return _device_runs[shape]


@pytest.mark.parametrize("shape", list(SHAPES))
def test_geometry(pkg, shape):
    L, M, fs, br, mk, sp = SHAPES[shape][0]
    pool = pkg.engine.AfskPool(L, M, fs, CAP, bitrate=br, mark=mk, space=sp)
    try:
        assert pool.geometry == {"L": L, "M": M, "N": L + M - 1, "samppbit": int(fs / br)}
        assert pool.geometry["samppbit"] == {"22k": 18, "22k1225": 18, "hf300": 53, "11k": 9, "shortM": 40, "longM": 10}[shape]
    finally:
        pool.close()


def lost(shape, k):
    """which of the four frames the restatement delivers, in order, and its CRC failures"""
    ref = restatement(shape, False)[k]
    want = ga.scenario(shape)[1][k]
    got = ao.frames_of(ref)
    assert all(f in want for f in got) and [want.index(f) for f in got] == sorted(want.index(f) for f in got), (shape, k, "a frame that was not sent, or out of order")
    return [SIZES[want.index(f)] for f in got], sum(r["crc_failures"] for r in ref)


@pytest.mark.parametrize("shape", [s for s in SHAPES if s != "22k"])
def test_frames_of_1_17_64_and_330_bytes_where_the_clock_holds(pkg, shape):
    """every shape but 22k: the restatement delivers all four frames without a CRC failure, and both instances equal it on every block.  Figures per
    shape (FLOOR, smallest margins, worst measured / allowed on the MI355X): the module's docstring; the test prints its own."""
    got = device_run(pkg, shape)
    for k in (0, 1):
        assert lost(shape, k) == (list(SIZES), 0), (shape, k, lost(shape, k))
        check_strict(shape, k, got[k], last_val_may_cancel=True)
    ref = restatement(shape, False)
    print("%s: at most %d decisions in a block" % (shape, max(r["ndecisions"] for k in (0, 1) for r in ref[k])))


def test_the_clock_slips_at_18_of_18_375_samples_a_bit_where_the_restatement_s_slips(pkg):
    """22050 / 1200.  On the restatement instance 0 (equal tones) delivers the frames of 1 and 17 payload bytes and counts one CRC failure -- 64 and 330
    are lost --, instance 1 (space tone x 1.8) delivers 17, 64 and 330 and loses the first; packetd.c loses the same ones (tests/test_afsk_reference.py).
    FLOOR 1.05e-5 and 1.24e-5, smallest margins 1.4e-4 and 1.2e-4.  The device equals the restatement on every block, crc_failures included; worst
    measured / allowed on the MI355X: last_val 0.97 (one of the three blocks on which it cancels and is held relative to itself), mid_val 0.42."""
    shape = "22k"
    got = device_run(pkg, shape)
    total = 0
    for k in (0, 1):
        frames, crc = lost(shape, k)
        print("22k instance %d: the restatement delivers the frames of %s payload bytes of %s, %d CRC failures" % (k, frames, list(SIZES), crc))
        assert len(frames) >= 1 and len(frames) < len(SIZES), (k, frames)
        total += crc
        check_strict(shape, k, got[k], last_val_may_cancel=True)
        assert sum(st["crc_failures"] for st, _, _ in got[k]) == crc
    assert total >= 1, "no CRC failure on natural data"
    ref = restatement(shape, False)
    print("22k: at most %d decisions in a block" % max(r["ndecisions"] for k in (0, 1) for r in ref[k]))


REFUSALS = [((960, 961, 16000.0, 1200.0, 1200.0, 2200.0), "80 decisions"),            # samppbit 13: ceil(960 / 12) = 80
            ((193, 192, 4800.0, 1200.0, 1200.0, 2200.0), "65 decisions"),             # samppbit 4: ceil(193 / 3) = 65
            ((960, 961, 22050.0, 1200.0, 11025.0, 2200.0), "samprate / 2"),           # the mark tone at exactly samprate / 2
            ((960, 961, 16000.0, 300.0, 1600.0, 8000.0), "samprate / 2"),             # ... and the space tone
            ((192, 193, 4800.0, 1200.0, 1200.0, 2200.0), None)]                       # ceil(192 / 3) = 64: the accepted neighbour of the second row


@pytest.mark.parametrize("geom,word", REFUSALS)
def test_geometries_that_are_refused(pkg, geom, word):
    E = pkg.engine
    L, M, fs, br, mk, sp = geom
    if word is None:
        E.AfskPool.check(L, M, fs, br, mk, sp)
        pool = E.AfskPool(L, M, fs, CAP, bitrate=br, mark=mk, space=sp)
        try:
            assert pool.geometry == {"L": L, "M": M, "N": L + M - 1, "samppbit": 4}
        finally:
            pool.close()
        return
    for make in (lambda: E.AfskPool.check(L, M, fs, br, mk, sp), lambda: E.AfskPool(L, M, fs, CAP, bitrate=br, mark=mk, space=sp)):
        with pytest.raises(E.ChzError) as e:
            make()
        assert word in str(e.value), str(e.value)


# ---- a frame longer than the HDLC's buffer ----------------------------------------------------------------------------------------------
LONG = "toolong"
LONG_GEOM = (240, 241, 12000.0, 1200.0, 1200.0, 2200.0)
LONG_SIZES = (17, 16400, 9)
NEIGHBOUR_LEAD = 30                     # idle flags in front of the neighbour's 330-byte frame


@functools.lru_cache(maxsize=None)
def long_input():
    """instance 0: 30 flags, frames of 17, 16,400 and 9 payload bytes three flags apart, 40 flags -> (blocks, payloads)"""
    L, M, fs = LONG_GEOM[:3]
    pl = payloads(17, LONG_SIZES)
    items = [("flags", 30)]
    for p in pl:
        items += [("frame", p), ("flags", 3)]
    items += [("flags", 40)]
    return whole_blocks(ao.modulate(ao.line_bits(items), fs, amplitude=0.4), L), pl


@functools.lru_cache(maxsize=None)
def crossing():
    """the block in which instance 0's HDLC runs past bit 131,072 of its buffer and aborts the frame, on the restatement alone"""
    L, M, fs = LONG_GEOM[:3]
    ref = ao.run(long_input()[0], L, M, fs)
    at = [b for b in range(1, len(ref)) if ref[b - 1]["frame_bits"] > 8 * ao.FRAME_BYTES - 64 and ref[b]["frame_bits"] < ref[b - 1]["frame_bits"]]
    assert len(at) == 1 and ref[at[0]]["flag_seen"] == 0 and ref[at[0]]["nframes"] == 0 and ref[at[0]]["crc_failures"] == 0, at
    return at[0]


def neighbour_start():
    """the call at which the neighbour's first block runs: its frame of 330 payload bytes (about 2700 bit times, 112 blocks) lies around crossing()"""
    return crossing() - (8 * NEIGHBOUR_LEAD * 10) // 240 - 56


def long_scenario():
    L, M, fs = LONG_GEOM[:3]
    a, pl = long_input()
    q = payloads(19, (330,))[0]
    b = whole_blocks(ao.modulate(ao.line_bits([("flags", NEIGHBOUR_LEAD), ("frame", q), ("flags", 40)]), fs, amplitude=0.4, phase=0.7), L)
    return [a, b], [[p + ao.fcs(p) for p in (pl[0], pl[2])], [q + ao.fcs(q)]]


ga.register(LONG, LONG_GEOM, long_scenario)


def test_a_frame_longer_than_the_buffer_aborts_beside_a_neighbour_whose_own_frame_is_open(pkg):
    """The HDLC writes bit 131,072 -- byte 16384 of the frame buffer, one beyond the reference's own array -- before its "too long: abort" branch
    (frame_bits > 16384 x 8) is taken; CHZ_AFSK_FRAME_PITCH exists for that byte.  Instance i takes 30 flags, frames of 17, 16,400 and 9 payload
    bytes and 40 flags (5592 blocks of 240 samples at 12 kHz); instance i + 1, whose frame buffer follows i's in device memory, starts at the call
    that puts its own frame of 330 payload bytes around the block in which i crosses bit 131,072 (the restatement gives that block).  Both strict
    on every block; the bytes behind the delivered frames keep the sentinel.  A byte written one pitch too far would be byte 0 of the neighbour's
    open frame, and its CRC would fail.
    Measured on the restatement: the crossing falls in block 5567 of 5592 and the neighbour starts at call 5501; instance i delivers frames of 19 and 11 bytes, no CRC failure, and
    frame_bits returns to 0 behind bit 131,072; the neighbour holds 1329 bits of its frame in that block.  The figures of both instances (FLOOR,
    smallest margins, worst measured / allowed) are printed: FLOOR 1.51e-5 and 1.20e-5, smallest margins 0.075 and 0.099, worst measured / allowed on
    the MI355X last_val 0.51, mid_val 0.85 (instance i) and 0.38, 0.54 (the neighbour).  The restatement of the 5592 blocks takes 1.6 s per run; the whole
    test 2.8 s on the MI355X and 9.4 s on the CPU build of the engine.  With the pitch cut to 16384 bytes the neighbour's frame fails its CRC and this
    test fails (tried on the CPU build)."""
    L, M, fs = LONG_GEOM[:3]
    E = pkg.engine
    blocks, want = ga.scenario(LONG)
    ref = restatement(LONG, False)
    x, start = crossing(), neighbour_start()
    assert ao.frames_of(ref[0]) == want[0] and sum(r["crc_failures"] for r in ref[0]) == 0
    assert ref[0][x - 1]["frame_bits"] > 131072 - 64 and ref[0][x]["frame_bits"] == 0 and ref[0][x]["flag_seen"] == 0
    assert ao.frames_of(ref[1]) == want[1]
    nb = ref[1][x - start]
    assert nb["flag_seen"] == 1 and 800 < nb["frame_bits"] < 2000 and len(ref[1][x - start + 30]["frames"]) == 0, (x, start, nb["frame_bits"])
    assert 0 < start < x < start + len(blocks[1])
    print("the crossing falls in block %d of %d; the neighbour starts at call %d and holds %d bits of its frame there" % (x, len(blocks[0]), start, nb["frame_bits"]))
    pool = E.AfskPool(L, M, fs, CAP, frame_stride=STRIDE)
    try:
        resp = ao.response(L, M, fs)
        i = pool.add()
        j = pool.add()
        assert j == i + 1
        pool.set_response(i, resp); pool.set_response(j, resp)
        rng = np.random.default_rng(7)
        got = {0: [], 1: []}
        for blk in range(max(len(blocks[0]), start + len(blocks[1]))):
            due = ([0] if blk < len(blocks[0]) else []) + ([1] if start <= blk < start + len(blocks[1]) else [])
            order = [due[n] for n in rng.permutation(len(due))]
            rows = [ao.to_wire(blocks[k][blk - (start if k else 0)]) for k in order]
            raw, sraw = buffers(len(order))
            st, fr = pool.execute([(i, j)[k] for k in order], rows, frames_buf=raw, status_buf=sraw)
            for r, k in enumerate(order):
                used = [len(f) for f in fr[r]] + [0, 0]
                for n in range(2):
                    assert (raw[r, n * STRIDE + used[n]:(n + 1) * STRIDE] == SENTINEL).all(), "bytes behind a frame were written"
                got[k].append((status_dict(st[r]), sraw[r].tobytes(), fr[r]))
    finally:
        pool.close()
    for k in (0, 1):
        check_strict(LONG, k, got[k], last_val_may_cancel=True)
