"""Pools of AFSK / AX.25 packet decoders (chz_afsk_*, kernel afsk_ovs) against tests/afsk_oracle.py, the float64 restatement of packetd's
decode_task() that tests/test_afsk_reference.py pins to the reference.

Three shapes -- packetd's own (L 960, M 961 at 48 kHz, 40 samples a bit), the same at 24 kHz (20 samples a bit: up to 50 decisions and two
frames a block) and the smallest workable one (L 240, M 241 at 12 kHz, N 480: the history hand-over runs four times as often) -- each run
ONE scenario of 5 instances in a pool of capacity 2 (three launches per call while all are due), the order permuted from call to call:
  0  strict: frames of 1, 17, 64 and 330 payload bytes between idle flags, from sample 0 to the end
  1  strict: the same frames starting inside a bit, the space tone 1.8 x the mark tone
  2  strict, the hard cases: two frames sharing one flag, a frame with a wrong CRC, eight ones inside a frame and a good frame behind them,
     a payload of 0xFF bytes, two 3-byte frames behind one another (at 24 kHz they complete in one block)
  3  two transmissions with eight blocks of exact zeros between them, fed with the reference's flush rule
  4  the samples of instance 0 handed over in device memory
The scenario and its restatement (float64, and the f32 twin) are computed once per shape and shared by the tests.  The 330-byte frame
alone is 2700 bit times, so instances 0 and 1 take 169 blocks at 48 and 12 kHz and 84 at 24 kHz, where a block holds 48 bits; instance 2
takes 63 and 31, instance 3 with its flush blocks 111 and 88.

Bounds.  Strict instances, on every block: ndecisions, bits, symphase, flag_seen, frame_bits, crc_failures, nframes, the frames' lengths and
bytes equal the restatement's.  last_val and mid_val, on every block: the rule of tests/test_gpu_wfm.py -- within 1e-6 relative to the
restatement's value, or 4 x the f32 twin's own distance on that block where that is larger.  Both are differences a - twist b of two tone
energies, and the rounding error of a difference is relative to its terms, not to itself: where |a - twist b| is below a quarter of
a + twist b (cancellation amplifies the error by more than the rule's own factor of 4) the same rule is applied relative to a + twist b, for the
device and the twin alike.  That never happens to last_val (at a decision it keeps 0.5 to 0.8 of its terms); it happens to mid_val, the
integrator at a zero crossing, on 0 to 13 blocks of instances 0 and 2 and on 40 to 75 of instance 1, whose mid_val goes down to 6e-5 of its
terms -- there an error of 3e-7 of the terms is 5e-3 of the value, whatever computes it.  The tests print the worst measured / allowed.
Input condition, asserted on the restatement before anything is compared: every decision of a strict instance has |cur_val last_val| and,
on a transition, |(cur_val - last_val) mid_val| above FLOOR x (the largest |cur_val|)^2, where FLOOR = 100 x the largest distance between
the restatement's float64 and float32 runs on cur_val over the largest |cur_val|.  Measured: the distance is 0.9 to 1.5e-7, so FLOOR is
0.9 to 1.5e-5; the strict instances' smallest margins are printed by the tests.
TWO kinds of decisions cannot carry that margin and are held to something else, both for a reason that does not depend on any arithmetic:
  * the very first decision of a session multiplies by last_val = 0 exactly: cur_val * 0 >= 0 whatever cur_val is;
  * the signal runs from sample 0, and the filter's group delay is (M - 1) / 2 samples: until the first (M - 1) / 2 + samppbit samples
    have passed the integrators see the precursor of the impulse response, 1e-3 of the signal, and the products are 1e-13 to 1e-7 of
    the later ones.  No input that starts at sample 0 can do better.  These 12 or 13 (48 and 12 kHz) or 24 or 25 (24 kHz) decisions are asserted
    to come out the same in the f32 twin instead, and are compared with the device like all others.  They do leave the clock at a phase that
    rounding can move (the reference's own float32 transform moved it, and lost a frame that followed six flags): hence LEAD below.
Instance 3 is decided on rounding noise while a transmission rings down, in the reference too: only its frames (bytes, order) and the CRC
count at the end are compared, and the restatement must show every closing flag at least two bit times away from a block edge."""
import functools
import os

import numpy as np
import pytest

import afsk_oracle as ao
import oracle_lib as ol
from conftest import load_pkg

pytestmark = pytest.mark.gpu

SHAPES = {"48k": (960, 961, 48000.0), "24k": (960, 961, 24000.0), "12k": (240, 241, 12000.0)}
NINST, CAP = 5, 2
SENTINEL = 0xA5
STRIDE = 512                                    # bytes a frame may take in the caller's buffer (the longest here is 332)
# idle flags in front of instance 3's transmissions, per shape.  A transmission that follows silence finds the bit clock at any phase (the
# decisions inside the filter's delay are taken on the precursor, on rounding noise): the Gardner step moves it by one sample per transition,
# samppbit / 2 samples need as many transitions, a flag has two, and the filter delays everything by 12 bit times -- so 24 flags or more, as a
# transmitter's TXDELAY sends them.  Among those, chosen so that every closing flag ends two bit times away from a block edge.
LEAD3 = {"48k": (25, 26), "24k": (24, 26), "12k": (25, 26)}
# idle flags in front of the strict instances' first frame: the decisions inside the filter's delay leave the clock anywhere (see the docstring), and
# the first frame must not depend on where -- the same reasoning as for LEAD3
LEAD = 30
# samples dropped in front of instance 1 (a start inside a bit), and idle flags in front of instance 2's pair of 3-byte frames: chosen, on the
# restatement alone, so that every decision carries its margin and -- at 24 kHz -- both frames of the pair complete in one block
OFFSET1 = {"48k": 22, "24k": 10, "12k": 7}
PAIR_FLAGS = {"48k": 3, "24k": 3, "12k": 3}
# shapes of other test files (tests/test_gpu_afsk_rates.py), which run this file's helpers at rates and tones of their own:
# name -> ((L, M, samprate, bitrate, mark, space), a function that returns what scenario() returns for it)
EXTRA = {}


def register(name, geom6, make_scenario):
    assert name not in SHAPES and len(geom6) == 6
    EXTRA[name] = (tuple(geom6), make_scenario)


def geom(shape):
    """(L, M, samprate, bitrate, mark, space) of a shape: packetd's own rates and tones for the shapes of this file"""
    return EXTRA[shape][0] if shape in EXTRA else SHAPES[shape] + (ao.BITRATE, ao.MARK, ao.SPACE)


@pytest.fixture(scope="module")
def pkg():
    p = load_pkg()
    if p.engine.lib().chz_device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests cannot run (there is no CPU fallback)")
    ol.build()
    return p


def payloads(seed, sizes):
    rng = np.random.default_rng(seed)
    return [bytes(rng.integers(0, 256, n, dtype=np.uint8)) for n in sizes]


def whole_blocks(x, L):
    return x[:x.size // L * L].reshape(-1, L)


def transmissions(shape):
    """instance 3's two transmissions (int16) and their payloads.  The space tone is 1.8 x the mark tone, the pre-emphasis that twist = 1200 / 2200
    undoes (1.8^2 x 0.545 = 1.77): with tones of equal amplitude the reference's clock recovery has a dead band -- a transmission that finds the
    clock within 4 of 40 samples of mid-bit (1 of 10 at 12 kHz) never pulls it in, measured on the restatement -- and where the ring-down left the
    clock is decided on rounding noise."""
    fs = SHAPES[shape][2]
    t1, t2 = payloads(13, (17, 24))
    lead = LEAD3[shape]
    tx1 = ao.modulate(ao.line_bits([("flags", lead[0]), ("frame", t1), ("flags", 20)]), fs, amplitude=0.25, space_gain=1.8)
    tx2 = ao.modulate(ao.line_bits([("flags", lead[1]), ("frame", t2), ("flags", 20)]), fs, amplitude=0.25, space_gain=1.8, phase=1.0)
    return tx1, tx2, t1, t2


@functools.lru_cache(maxsize=None)
def decodes_from_every_clock_phase(shape):
    """the input condition of instance 3: each transmission, behind silence of one block and k = 0 .. samppbit - 1 samples, delivers its frame in
    the restatement -- whatever phase the ring-down before it left the clock at"""
    L, M, fs = SHAPES[shape]
    tx1, tx2, t1, t2 = transmissions(shape)
    for tx, t in ((tx1, t1), (tx2, t2)):
        for k in range(int(fs / ao.BITRATE)):
            x = np.concatenate([np.zeros(L + k, np.int16), tx])
            x = np.concatenate([x, np.zeros(-x.size % L + L, np.int16)])
            if ao.frames_of(ao.run(x.reshape(-1, L), L, M, fs)) != [t + ao.fcs(t)]:
                return False
    return True


@functools.lru_cache(maxsize=None)
def scenario(shape):
    """int16 blocks [nblocks][L] of instances 0-3 and the frames each must deliver"""
    if shape in EXTRA:
        return EXTRA[shape][1]()
    L, M, fs = SHAPES[shape]
    sps = int(fs / ao.BITRATE)
    pl = payloads(11, (1, 17, 64, 330))
    items = [("flags", LEAD)]
    for p in pl:
        items += [("frame", p), ("flags", 3)]
    items += [("flags", 40)]
    bits = ao.line_bits(items)
    want = [p + ao.fcs(p) for p in pl]
    a, b, c, d, e, f, g = payloads(12, (17, 5, 9, 12, 21, 1, 1))
    hard = [("flags", LEAD), ("frame", a), ("flags", 1), ("frame", b), ("flags", 4), ("badcrc", c), ("flags", 4),
            ("raw", ao.frame_bits(d)[:60] + [1] * 8), ("flags", 4), ("frame", e), ("flags", 3), ("frame", b"\xff" * 20), ("flags", PAIR_FLAGS[shape]),
            ("frame", f), ("flags", 1), ("frame", g), ("flags", 40)]
    want2 = [p + ao.fcs(p) for p in (a, b, e, b"\xff" * 20, f, g)]
    tx1, tx2, t1, t2 = transmissions(shape)
    pad = lambda x: np.concatenate([x, np.zeros(-x.size % L, np.int16)])
    x3 = np.concatenate([pad(tx1), np.zeros(8 * L, np.int16), pad(tx2), np.zeros(L, np.int16)])
    blocks = [whole_blocks(ao.modulate(bits, fs, amplitude=0.4), L),
              whole_blocks(ao.modulate(bits, fs, amplitude=0.25, space_gain=1.8, offset=OFFSET1[shape]), L),
              whole_blocks(ao.modulate(ao.line_bits(hard), fs, amplitude=0.4, phase=0.7), L),
              ao.feed(x3, L)]
    return blocks, [want, want, want2, [t1 + ao.fcs(t1), t2 + ao.fcs(t2)]]


@functools.lru_cache(maxsize=None)
def restatement(shape, f32):
    L, M, fs, br, mk, sp = geom(shape)
    return [ao.run(b, L, M, fs, f32=f32, bitrate=br, mark=mk, space=sp) for b in scenario(shape)[0]]


def status_dict(s):
    return {"ndecisions": s.ndecisions, "symphase": s.symphase, "bits": s.bits, "last_val": s.last_val, "mid_val": s.mid_val, "flag_seen": s.flag_seen,
            "frame_bits": s.frame_bits, "crc_failures": s.crc_failures, "nframes": s.nframes, "frame_len": [s.frame_len[0], s.frame_len[1]]}


def on_emulator():
    return os.environ.get("CHZ_ALLOW_EMULATED_ENGINE") == "1"


class DeviceRows:
    """16-bit words in device memory, allocated and filled through the HIP runtime the engine itself is linked to.  Not a torch tensor: the torch
    wheel carries HIP and HSA runtime libraries of its own (torch/lib/libamdhip64.so, libhsa-runtime64.so), and in a process in which the
    engine's runtime has opened the device torch.cuda finds "No HIP GPUs" -- INTEGRATION.md has the line.  AfskPool.execute takes any device
    address.  (On the CPU build of the engine device memory is host memory.)"""

    def __init__(self, words):
        words = np.ascontiguousarray(words)
        self.hip = None
        if on_emulator():
            self.keep = words
            self.base = words.ctypes.data
        else:
            import ctypes as C
            self.hip = C.CDLL("libamdhip64.so")
            self.hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
            self.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            self.hip.hipFree.argtypes = [C.c_void_p]
            ptr = C.c_void_p()
            assert self.hip.hipMalloc(C.byref(ptr), words.nbytes) == 0
            assert self.hip.hipMemcpy(ptr, words.ctypes.data, words.nbytes, 1) == 0          # hipMemcpyHostToDevice, complete on return
            self.base = ptr.value

    def free(self):
        if self.hip is not None:
            self.hip.hipFree(self.base)
            self.hip = None

    def row(self, i, L):
        return self.base + 2 * L * i


def buffers(n):
    """the caller's frame and status buffers of n requests, full of the sentinel"""
    return np.full((n, 2 * STRIDE), SENTINEL, np.uint8), np.full((n, 56), SENTINEL, np.uint8)


def run_pool(pkg, shape, cap, seed=7, big_endian=True, only=None):
    """the scenario through a pool of capacity `cap`: [inst] -> list over blocks of (status dict, raw status bytes, frames)"""
    L, M, fs, br, mk, sp = geom(shape)
    E = pkg.engine
    blocks = scenario(shape)[0]
    ks = list(range(NINST)) if only is None else list(only)
    src = {k: blocks[0 if k == 4 else k] for k in ks}
    pool = E.AfskPool(L, M, fs, cap, bitrate=br, mark=mk, space=sp, byte_order=E.AFSK_BE if big_endian else E.AFSK_LE, frame_stride=STRIDE)
    dev = None
    try:
        resp = ao.response(L, M, fs, br, mk, sp)
        inst = {k: pool.add() for k in ks}
        for k in ks:
            pool.set_response(inst[k], resp)
        dev = DeviceRows(ao.to_wire(src[4], big_endian)) if 4 in ks else None
        rng = np.random.default_rng(seed)
        out = {k: [] for k in ks}
        for blk in range(max(len(src[k]) for k in ks)):
            due = [k for k in ks if blk < len(src[k])]
            order = [due[i] for i in rng.permutation(len(due))]
            for group, on_device in (([k for k in order if k != 4], False), ([k for k in order if k == 4], True)):
                if not group:
                    continue
                rows = [dev.row(blk, L) for k in group] if on_device else [ao.to_wire(src[k][blk], big_endian) for k in group]
                raw, sraw = buffers(len(group))
                st, fr = pool.execute([inst[k] for k in group], rows, on_device=on_device, frames_buf=raw, status_buf=sraw)
                for r, k in enumerate(group):
                    used = [len(f) for f in fr[r]] + [0, 0]
                    for j in range(2):
                        assert (raw[r, j * STRIDE + used[j]:(j + 1) * STRIDE] == SENTINEL).all(), "bytes behind a frame were written"
                    out[k].append((status_dict(st[r]), sraw[r].tobytes(), fr[r]))
        return out
    finally:
        pool.close()
        if dev is not None:
            dev.free()


_device_runs = {}


def device_run(pkg, shape):
    if shape not in _device_runs:
        _device_runs[shape] = run_pool(pkg, shape, CAP)
    return _device_runs[shape]


def startup(shape):
    L, M, fs, br = geom(shape)[:4]
    return (M - 1) // 2 + int(fs / br)


def input_condition(shape, k):
    """the margins of strict instance k (see the module's docstring) -> (floor, smallest first margin, smallest second margin, largest |cur_val|)"""
    L = geom(shape)[0]
    ref, twin = restatement(shape, False)[k], restatement(shape, True)[k]
    cur = np.array([c for r in ref for c in r["cur"]]); tcur = np.array([c for r in twin for c in r["cur"]])
    assert cur.shape == tcur.shape, (shape, k, "the f32 twin takes another number of decisions: unusable input")
    top = float(np.abs(cur).max())
    floor = 100.0 * float(np.abs(cur - tcur).max()) / top
    m1 = m2 = np.inf
    for blk, (r, t) in enumerate(zip(ref, twin)):
        for f in ao.DISCRETE:
            assert t[f] == r[f], (shape, k, blk, f, "the f32 twin takes another decision: unusable input")
        for i, (a, b) in enumerate(r["margins"]):
            if blk * L + r["pos"][i] <= startup(shape):
                continue                                   # inside the filter's group delay: held to the twin's agreement, asserted above
            m1 = min(m1, a / top ** 2)
            if b is not None:
                m2 = min(m2, b / top ** 2)
            assert a / top ** 2 > floor, (shape, k, blk, i, "|cur_val last_val| below the floor", a / top ** 2, floor)
            assert b is None or b / top ** 2 > floor, (shape, k, blk, i, "|(cur_val - last_val) mid_val| below the floor", b / top ** 2, floor)
    return floor, m1, m2, top


CANCELLING = 0.25          # a difference below this share of its terms is held to the rule relative to the terms (see the docstring)


def check_strict(shape, k, got, kref=None, last_val_may_cancel=False):
    """last_val_may_cancel: an input whose clock slips takes decisions near bit edges, where last_val cancels too (this file's inputs never do,
    and that is asserted); last_val is then held to the rule relative to ITSELF all the same -- the cancellation rule stays mid_val's alone"""
    kref = k if kref is None else kref
    floor, m1, m2, top = input_condition(shape, kref)
    ref, twin = restatement(shape, False)[kref], restatement(shape, True)[kref]
    assert len(got) == len(ref)
    worst, cancelling = {f: 0.0 for f in ao.CONTINUOUS}, {f: 0 for f in ao.CONTINUOUS}
    for blk, (r, t, (st, _, frames)) in enumerate(zip(ref, twin, got)):
        for f in ao.DISCRETE:
            assert st[f] == r[f], (shape, k, blk, f, st[f], r[f])
        assert st["frame_len"] == r["frame_len"] and frames == r["frames"], (shape, k, blk, st["frame_len"], r["frame_len"])
        for f in ao.CONTINUOUS:
            terms = r[f.replace("_val", "_terms")]
            if terms == 0.0:                                                # nothing decided yet: the value is the initial zero
                assert st[f] == r[f] == 0.0, (shape, k, blk, f, st[f], r[f])
                continue
            scale = abs(r[f])
            if scale < CANCELLING * terms:
                cancelling[f] += 1
                if f == "mid_val" or not last_val_may_cancel:
                    scale = terms
            e, lim = abs(st[f] - r[f]) / scale, max(1e-6, 4 * abs(t[f] - r[f]) / scale)
            worst[f] = max(worst[f], e / lim)
            assert e <= lim, (shape, k, blk, f, st[f], r[f], e, lim)
    assert last_val_may_cancel or cancelling["last_val"] == 0
    print("%s instance %d: FLOOR %.3g, smallest margins %.3g / %.3g; worst measured / allowed: last_val %.2f, mid_val %.2f (%d of %d blocks relative to the terms)%s"
          % (shape, k, floor, m1, m2, worst["last_val"], worst["mid_val"], cancelling["mid_val"], len(ref),
             "; last_val below a quarter of its terms on %d blocks, held relative to itself" % cancelling["last_val"] if cancelling["last_val"] else ""))


@pytest.mark.parametrize("shape", list(SHAPES))
def test_geometry(pkg, shape):
    L, M, fs = SHAPES[shape]
    pool = pkg.engine.AfskPool(L, M, fs, CAP)
    try:
        assert pool.geometry == {"L": L, "M": M, "N": L + M - 1, "samppbit": int(fs / 1200.0)}
        assert pkg.engine.lib().chz_afsk_capacity(pool._h) == CAP
    finally:
        pool.close()


@pytest.mark.parametrize("shape", list(SHAPES))
def test_frames_of_1_17_64_and_330_bytes_on_the_bit_grid_and_off_it(pkg, shape):
    got = device_run(pkg, shape)
    want = scenario(shape)[1]
    for k in (0, 1):
        assert ao.frames_of(restatement(shape, False)[k]) == want[k]
        check_strict(shape, k, got[k])


@pytest.mark.parametrize("shape", list(SHAPES))
def test_shared_flag_bad_crc_abort_stuffing_and_two_frames_in_a_block(pkg, shape):
    ref = restatement(shape, False)[2]
    assert ao.frames_of(ref) == scenario(shape)[1][2]
    assert sum(r["crc_failures"] for r in ref) == 1                         # (the aborted fragment would be a second one had the eight ones not aborted it)
    assert (max(r["nframes"] for r in ref) == 2) == (shape == "24k")
    check_strict(shape, 2, device_run(pkg, shape)[2])


@pytest.mark.parametrize("shape", list(SHAPES))
def test_transmissions_between_silence_with_the_flush_rule(pkg, shape):
    L, M, fs = SHAPES[shape]
    sps = int(fs / ao.BITRATE)
    ref = restatement(shape, False)[3]
    want = scenario(shape)[1][3]
    assert ao.frames_of(ref) == want
    assert decodes_from_every_clock_phase(shape), (shape, "a transmission that does not decode from every clock phase: unusable input")
    for r in ref:
        for n in r["events"]:
            assert 2 * sps <= n <= L - 2 * sps, (shape, "a closing flag within two bit times of a block edge", n)
    got = device_run(pkg, shape)[3]
    assert len(got) == len(ref)
    assert [f for _, _, fr in got for f in fr] == want
    assert sum(st["crc_failures"] for st, _, _ in got) == sum(r["crc_failures"] for r in ref)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_samples_in_device_memory_give_the_same_bytes(pkg, shape):
    got = device_run(pkg, shape)
    assert len(got[4]) == len(got[0])
    for blk, (a, b) in enumerate(zip(got[0], got[4])):
        assert a[1] == b[1] and a[2] == b[2], (shape, blk)


def test_released_and_added_again_starts_from_zero(pkg):
    shape = "12k"
    L, M, fs = SHAPES[shape]
    blocks = scenario(shape)[0][0]
    pool = pkg.engine.AfskPool(L, M, fs, CAP, frame_stride=STRIDE)
    try:
        resp = ao.response(L, M, fs)
        other = pool.add()
        i = pool.add()
        pool.set_response(i, resp)
        for blk in range(40, 60):                                           # leave it in the middle of a frame, with history and a running clock
            pool.execute([i], [ao.to_wire(blocks[blk])])
        pool.release(i)
        j = pool.add()
        assert j == i and other != i
        pool.set_response(j, resp)
        got = []
        for blk in range(len(blocks)):
            st, fr = pool.execute([j], [ao.to_wire(blocks[blk])])
            got.append((status_dict(st[0]), None, fr[0]))
        check_strict(shape, 0, got)
    finally:
        pool.close()


def test_little_endian_samples(pkg):
    shape = "12k"
    be = device_run(pkg, shape)[2]
    le = run_pool(pkg, shape, CAP, big_endian=False, only=(2,))[2]
    assert len(le) == len(be)
    for blk, (a, b) in enumerate(zip(be, le)):
        assert a[1] == b[1] and a[2] == b[2], (shape, blk)


def test_refused_calls_leave_state_and_outputs_untouched(pkg):
    """an instance listed twice, an index that is not in use, one out of range and a null row among good requests, each between two good blocks of
    instance 1: status and frame buffers keep the sentinel, and the run matches the restatement as if nothing had happened"""
    shape = "12k"
    L, M, fs = SHAPES[shape]
    blocks = scenario(shape)[0][1]
    E = pkg.engine
    pool = E.AfskPool(L, M, fs, CAP, frame_stride=STRIDE)
    try:
        resp = ao.response(L, M, fs)
        a, b = pool.add(), pool.add()
        pool.set_response(a, resp); pool.set_response(b, resp)
        pool.release(b)
        got = []
        for blk in range(len(blocks)):
            row = ao.to_wire(blocks[blk])
            bad = {30: ([a, a], [row, row], "twice"), 31: ([a, b], [row, row], "not in use"), 32: ([a, 99], [row, row], "bad request"),
                   33: ([a, a], [row, None], "bad request")}.get(blk)
            if bad:
                raw, sraw = buffers(2)
                with pytest.raises(E.ChzError) as e:
                    pool.execute(bad[0], bad[1], frames_buf=raw, status_buf=sraw)
                assert bad[2] in str(e.value), str(e.value)
                assert (raw == SENTINEL).all() and (sraw == SENTINEL).all()
            st, fr = pool.execute([a], [row])
            got.append((status_dict(st[0]), None, fr[0]))
        check_strict(shape, 1, got)
    finally:
        pool.close()


REFUSALS = [((960, 962, 48000.0, 1200.0, 1200.0, 2200.0), "even N"),                  # what chz_rmini_check refuses: an odd N
            ((20000, 20001, 48000.0, 1200.0, 1200.0, 2200.0), "16384"),               # ... and a master beyond the pooled sizes
            ((960, 961, 4000.0, 1200.0, 1200.0, 1900.0), "4 samples a bit"),          # samppbit 3
            ((960, 961, 48000.0, 1200.0, 1200.0, 24000.0), "samprate / 2"),           # a tone at samprate / 2
            ((960, 961, 9600.0, 1200.0, 1200.0, 2200.0), "64"),                       # ceil(960 / 7) = 138 decisions a block
            ((960, 961, 48000.0, 1e-300, 1200.0, 2200.0), "bad AFSK rates"),          # a quotient no int holds
            ((960, 961, 48000.0, 1200.0, -1200.0, 2200.0), "bad AFSK rates"),         # a negative tone
            ((960, 961, float("nan"), 1200.0, 1200.0, 2200.0), "bad AFSK rates"),
            ((960, 961, 19200.0, 1200.0, 1200.0, 2200.0), None)]                      # ceil(960 / 15) = 64: the largest that fits


@pytest.mark.parametrize("geom,word", REFUSALS)
def test_geometries_that_are_refused(pkg, geom, word):
    E = pkg.engine
    L, M, fs, br, mk, sp = geom
    if word is None:
        E.AfskPool.check(L, M, fs, br, mk, sp)
        return
    for make in (lambda: E.AfskPool.check(L, M, fs, br, mk, sp), lambda: E.AfskPool(L, M, fs, CAP, bitrate=br, mark=mk, space=sp)):
        with pytest.raises(E.ChzError) as e:
            make()
        assert word in str(e.value), str(e.value)


def test_a_byte_order_that_is_neither_is_refused(pkg):
    E = pkg.engine
    for make in (lambda: E.AfskPool.check(960, 961, 48000.0, byte_order=2), lambda: E.AfskPool(960, 961, 48000.0, CAP, byte_order=-1)):
        with pytest.raises(E.ChzError) as e:
            make()
        assert "byte order" in str(e.value), str(e.value)


def test_capacity_8_gives_the_same_bits(pkg):
    shape = "24k"
    got = device_run(pkg, shape)
    again = run_pool(pkg, shape, 8)
    for k in range(NINST):
        assert len(again[k]) == len(got[k])
        for blk, (a, b) in enumerate(zip(got[k], again[k])):
            assert a[1] == b[1] and a[2] == b[2], (shape, k, blk)
