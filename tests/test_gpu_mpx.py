"""Pools of FM-multiplex decoders (chz_mpx_*, kernel mpx_ovs) against tests/mpx_oracle.py, the float64 restatement of stereod's and rdsd's
decode() loops that tests/test_mpx_reference.py pins to the reference.

Three shapes -- 1 ms (N 768: the smallest, 128 threads), 5 ms (N 3840: stereod's own) and 20 ms (N 15360: the largest, 1024 threads, about
120 KB of LDS) -- each run ONE STEREO scenario of 5 instances in a big-endian pool of capacity 2 (three launches per call) over 12 blocks,
the order permuted from call to call, gain 4, the signal of mpx_oracle.signal() with seed = the instance's number:
  0  A 0.2, 75 us
  1  A 0.2, 50 us
  2  A 0.2, rate 0 (no memory): the peaks reach just beyond +-1, the clip edge
  3  A 0.2, 75 us, the blocks scripted [0,0,0,1,1,1,1,0,0,1,1,1]: blocks 0-2 and 8 have an all-zero window (zero_pilot = olen, the PCM of
     blocks 0-2 all zero, block 8 the pure decay of the states), blocks 3, 7 and 9 are mixed windows
  4  A 0.5, 75 us: peaks beyond +-2, clipped samples in every block
The scenario and its restatement (float64, and the f32 twin) are computed once per shape and shared by the tests.

Input conditions, asserted on the restatement before anything is compared: the restatement and the twin report the same zero_pilot on every
block (0 everywhere but the all-zero windows, where it is olen); instance 4 clips in every block.

Bounds, on EVERY block.  zero_pilot: equal.  PCM bytes: mpx_oracle.pack() of the device's OWN audio floats, byte for byte (the packer is
exact; no allowance for rounding ties).  Rule (A), the audio floats against the restatement's float64 values: rel-L2 <= REL_L2 and max-abs <=
MAXABS_RMS x rms (tests/test_gpu_parity.py), or 4 x the f32 twin's own error on that block where the twin's error exceeds a quarter of the
figure (tests/test_gpu_wfm.py words it the same way).  rms is the restatement's over the block, or over the instance's last block so far whose
whole window was signal where that is larger: a decay tail is judged against the signal it is the tail of.  deemph_left / deemph_right: within
the block's max-abs limit.  The tests print the worst measured / allowed per instance.

Further: the same scenario from a little-endian pool with the samples in device memory (bytes equal to the big-endian host run), the bytes
behind a row keep the sentinel, audio = None gives the same PCM, release and re-add, set_params between blocks, refused calls, refused
geometries, and RDS pools at 5 and 1 ms (2 instances, 8 blocks, the signal plus 0.05 b(t) cos(2 pi 57000 t), b a +-1 sequence at 1187.5 baud).

Measured: on the MI355X the worst measured / allowed is 0.026 (an RDS pool's rel-L2; 0.017 for STEREO), on the emulated engine 0.027; the f32 twin
itself never exceeds a quarter of the fixed figures on these inputs, so the fixed figures are the limits throughout.

Where this departs from the issue's wording.  Instance 2's peaks (1.019 at 5 and 20 ms) are printed, not asserted: 12 blocks of 1 ms end before the
first peak beyond 1 (0.930 there), so the clip edge is met at 5 and 20 ms only.  Block 8 of instance 3 is the pure decay of the states, asserted on
the floats and the status record; its PCM is compared with the restatement's, because at 20 ms the states have fallen below a 16-bit step (and below
a float) by then and the bytes are all zero.  chz_mpx_set_params refuses a rate outside [0, 1) and values that are not finite (the issue names no
range); the test holds it to that."""
import ctypes as C
import functools

import numpy as np
import pytest

import afsk_oracle as ao
import mpx_oracle as mo
import oracle_lib as ol
from conftest import load_pkg
from test_gpu_afsk import DeviceRows
from test_gpu_parity import MAXABS_RMS, REL_L2

pytestmark = pytest.mark.gpu

SHAPES = {"1ms": 0.001, "5ms": 0.005, "20ms": 0.02}
NBLOCKS, CAP, SENTINEL = 12, 2, 0xA5
SCRIPT3 = [0, 0, 0, 1, 1, 1, 1, 0, 0, 1, 1, 1]
# per instance: (amplitude, de-emphasis rate, script)
SCENARIO = [(0.2, mo.RATE75, None), (0.2, mo.rate_of(50e-6), None), (0.2, 0.0, None), (0.2, mo.RATE75, SCRIPT3), (0.5, mo.RATE75, None)]


@pytest.fixture(scope="module")
def pkg():
    p = load_pkg()
    if p.engine.lib().chz_device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests cannot run (there is no CPU fallback)")
    ol.build()
    return p


def block_time(shape):
    """a shape is one of SHAPES' names, or (tests/test_gpu_mpx_shapes.py) a block time in seconds"""
    return SHAPES[shape] if isinstance(shape, str) else shape


@functools.lru_cache(maxsize=None)
def scenario(shape):
    """int16 blocks [NBLOCKS][L] per instance"""
    return [mo.signal(NBLOCKS, block_time(shape), k, a, script) for k, (a, _, script) in enumerate(SCENARIO)]


@functools.lru_cache(maxsize=None)
def restatement(shape, f32):
    return [mo.run(b, block_time(shape), rate=SCENARIO[k][1], f32=f32) for k, b in enumerate(scenario(shape))]


def whole_window_signal(script, nblocks):
    """per block: was its whole window (the block before it and itself) signal?"""
    s = [1] * nblocks if script is None else script
    return [bool(s[b]) and (b == 0 or bool(s[b - 1])) for b in range(nblocks)]


def limits(ref, twin, full=None):
    """rule (A) per block -> (rms, rel-L2 limit, max-abs limit); full: per block, whether its whole window was signal (None: every block's was)"""
    out, tail_rms = [], 0.0
    for blk, (r, t) in enumerate(zip(ref, twin)):
        w, tw = r["audio"], t["audio"]
        own = float(np.sqrt(np.mean(w ** 2)))
        if full is None or full[blk]:
            tail_rms = own
        rms = max(own, tail_rms)
        terr, tmx = float(np.sqrt(np.mean((tw - w) ** 2))), float(np.abs(tw - w).max())
        out.append((rms, REL_L2 * rms if terr <= 0.25 * REL_L2 * rms else 4 * terr, MAXABS_RMS * rms if tmx <= 0.25 * MAXABS_RMS * rms else 4 * tmx))
    return out


def check(ref, twin, got, label, full=None):
    """got: list over blocks of (pcm bytes, audio float32, (zero_pilot, deemph_left, deemph_right)) -> the worst measured / allowed"""
    assert len(got) == len(ref) == len(twin)
    for blk, (r, t) in enumerate(zip(ref, twin)):                           # the input condition, before anything is compared
        assert r["zero_pilot"] == t["zero_pilot"], (label, blk, "the f32 twin counts other zero pilots: unusable input", r["zero_pilot"], t["zero_pilot"])
    worst = {"rel_l2": 0.0, "maxabs": 0.0, "state": 0.0}
    for blk, (r, (rms, lim_l2, lim_mx), (pcm, audio, st)) in enumerate(zip(ref, limits(ref, twin, full), got)):
        assert st[0] == r["zero_pilot"], (label, blk, st[0], r["zero_pilot"])
        assert audio.dtype == np.float32 and pcm.tobytes() == mo.pack(audio), (label, blk, "the PCM is not scaleclip() of the device's own floats")
        g, w = audio.astype(np.float64), r["audio"]
        err, mx = float(np.sqrt(np.mean((g - w) ** 2))), float(np.abs(g - w).max())
        se = max(abs(st[1] - r["deemph_left"]), abs(st[2] - r["deemph_right"]))
        assert err <= lim_l2, (label, blk, "rel-L2", err, lim_l2, rms)
        assert mx <= lim_mx, (label, blk, "max-abs", mx, lim_mx, rms)
        assert se <= lim_mx, (label, blk, "de-emphasis state", se, lim_mx)
        if lim_l2 > 0:
            worst["rel_l2"] = max(worst["rel_l2"], err / lim_l2); worst["maxabs"] = max(worst["maxabs"], mx / lim_mx); worst["state"] = max(worst["state"], se / lim_mx)
    print("%s: worst measured / allowed over %d blocks: rel-L2 %.3g, max-abs %.3g, state %.3g" % (label, len(ref), worst["rel_l2"], worst["maxabs"], worst["state"]))
    return worst


def set_up(pool, kind, bt, params):
    """one instance with the oracle's responses and (rate, gain), or the defaults where params is None"""
    i = pool.add()
    for s, r in enumerate(mo.responses(bt, kind)):
        pool.set_response(i, s, r)
    if params is not None:
        pool.set_params(i, load_pkg().engine.MpxParams(params[0], params[1]))
    return i


def one_block(pool, inst, row, audio=True):
    pcm, au, st = pool.execute([inst], [row], audio=audio, fill=SENTINEL)
    assert (pool.last_raw[0, 4 * pool.olen:] == SENTINEL).all()
    return pcm[0], (au[0] if audio else None), (st[0].zero_pilot, st[0].deemph_left, st[0].deemph_right)


def run_pool(pkg, shape, cap, src, params, kind=mo.STEREO, big_endian=True, on_device=False, audio=True, seed=7):
    """src: {k: int16 blocks}, params: {k: (rate, gain)} -> {k: list over blocks of (pcm bytes, audio floats or None, status tuple)}"""
    E = pkg.engine
    bt = block_time(shape)
    ks = list(src)
    pool = E.MpxPool(bt, cap, kind=kind, byte_order=E.MPX_BE if big_endian else E.MPX_LE)
    dev = {}
    try:
        L, olen = pool.L, pool.olen
        inst = {k: set_up(pool, kind, bt, params[k]) for k in ks}
        if on_device:
            dev = {k: DeviceRows(ao.to_wire(src[k], big_endian)) for k in ks}
        rng = np.random.default_rng(seed)
        out = {k: [] for k in ks}
        for blk in range(max(len(src[k]) for k in ks)):
            due = [k for k in ks if blk < len(src[k])]
            order = [due[i] for i in rng.permutation(len(due))]
            rows = [dev[k].row(blk, L) for k in order] if on_device else [ao.to_wire(src[k][blk], big_endian) for k in order]
            pcm, au, st = pool.execute([inst[k] for k in order], rows, audio=audio, on_device=on_device, fill=SENTINEL)
            assert (pool.last_raw[:, 4 * olen:] == SENTINEL).all(), "bytes behind the PCM row were written"
            assert not audio or (pool.last_raw_audio[:, 2 * olen:].view(np.uint8) == SENTINEL).all(), "bytes behind the floats were written"
            for r, k in enumerate(order):
                out[k].append((pcm[r], au[r] if audio else None, (st[r].zero_pilot, st[r].deemph_left, st[r].deemph_right)))
        return out
    finally:
        pool.close()
        for d in dev.values():
            d.free()


_device_runs = {}


def device_run(pkg, shape):
    """the scenario's big-endian pool, samples from the host"""
    if shape not in _device_runs:
        b = scenario(shape)
        _device_runs[shape] = run_pool(pkg, shape, CAP, dict(enumerate(b)), {k: (s[1], mo.GAIN) for k, s in enumerate(SCENARIO)})
    return _device_runs[shape]


def check_instance(pkg, shape, k):
    full = whole_window_signal(SCENARIO[k][2], NBLOCKS)
    return check(restatement(shape, False)[k], restatement(shape, True)[k], device_run(pkg, shape)[k], "%s instance %d" % (shape, k), full)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_geometry(pkg, shape):
    E = pkg.engine
    for kind in (E.MPX_STEREO, E.MPX_RDS):
        pool = E.MpxPool(SHAPES[shape], CAP, kind=kind)
        try:
            assert pool.geometry == mo.geometry(SHAPES[shape], kind)
            assert E.lib().chz_mpx_capacity(pool._h) == CAP
            if shape == "5ms":
                assert tuple(pool.geometry.values()) == (1920, 1921, 3840, 240, 480, 190, 380 if kind == E.MPX_STEREO else 570)
        finally:
            pool.close()
    assert mo.geometry(SHAPES[shape])["N"] == {"1ms": 768, "5ms": 3840, "20ms": 15360}[shape]


@pytest.mark.parametrize("shape", list(SHAPES))
def test_the_scenario_does_what_it_is_meant_to_do_in_the_restatement(shape):
    ref, twin = restatement(shape, False), restatement(shape, True)
    olen = mo.geometry(SHAPES[shape])["olen"]
    for k in range(len(SCENARIO)):
        for blk in range(NBLOCKS):
            zero_window = k == 3 and blk in (0, 1, 2, 8)
            assert ref[k][blk]["zero_pilot"] == twin[k][blk]["zero_pilot"] == (olen if zero_window else 0), (shape, k, blk)
    for blk in range(NBLOCKS):
        clipped = int((np.abs(ref[4][blk]["audio"].astype(np.float32)) >= 1).sum())
        assert clipped > 0, (shape, blk, "instance 4 must clip in every block")
    peak2 = max(float(np.abs(r["audio"]).max()) for r in ref[2])              # (printed, not asserted: 12 blocks of 1 ms end before the first such peak)
    for blk in (0, 1, 2):
        assert not ref[3][blk]["audio"].any() and ref[3][blk]["pcm"] == bytes(4 * olen)
    r8, r7 = ref[3][8], ref[3][7]                                           # block 8: the pure decay of the states
    assert r8["audio"][0] == r7["deemph_left"] * mo.RATE75 and r8["audio"][1] == r7["deemph_right"] * mo.RATE75 and r8["audio"].any()
    print("%s: instance 2 peaks at %.3f, instance 4 at %.2f with %d to %d clipped values a block" % (
        shape, peak2, max(float(np.abs(r["audio"]).max()) for r in ref[4]),
        min(int((np.abs(r["audio"].astype(np.float32)) >= 1).sum()) for r in ref[4]), max(int((np.abs(r["audio"].astype(np.float32)) >= 1).sum()) for r in ref[4])))


@pytest.mark.parametrize("shape", list(SHAPES))
def test_three_time_constants_and_the_clip_edge(pkg, shape):
    for k in (0, 1, 2):
        check_instance(pkg, shape, k)
    edge = np.concatenate([np.frombuffer(pcm.tobytes(), ">i2") for pcm, _, _ in device_run(pkg, shape)[2]])
    peaks = np.concatenate([r["audio"] for r in restatement(shape, False)[2]])
    assert edge.min() >= -32767                                            # -32768 never
    if peaks.max() > 1.001:
        assert edge.max() == 32767
    if peaks.min() < -1.001:
        assert edge.min() == -32767


@pytest.mark.parametrize("shape", list(SHAPES))
def test_scripted_silence_zero_pilots_and_the_decay_of_the_states(pkg, shape):
    check_instance(pkg, shape, 3)
    got = device_run(pkg, shape)[3]
    olen = mo.geometry(SHAPES[shape])["olen"]
    assert [st[0] for _, _, st in got] == [olen if b in (0, 1, 2, 8) else 0 for b in range(NBLOCKS)]
    for blk in (0, 1, 2):
        assert not got[blk][0].any() and got[blk][2][1:] == (0.0, 0.0)
    # block 8 is the pure decay of the states (at 20 ms they have long fallen below a 16-bit step, and below a float, by then)
    assert got[8][1][0] == np.float32(got[7][2][1] * mo.RATE75) and got[8][1][1] == np.float32(got[7][2][2] * mo.RATE75)
    assert got[8][0].any() == any(restatement(shape, False)[3][8]["pcm"]) and 0 < abs(got[8][2][1]) < abs(got[7][2][1])


@pytest.mark.parametrize("shape", list(SHAPES))
def test_clipped_samples_in_every_block(pkg, shape):
    check_instance(pkg, shape, 4)
    for blk, (pcm, audio, _) in enumerate(device_run(pkg, shape)[4]):
        v = np.frombuffer(pcm.tobytes(), ">i2")
        assert (np.abs(audio) >= 1).any() and ((np.abs(v) == 32767) == (np.abs(audio) >= 1)).all(), (shape, blk)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_little_endian_samples_in_device_memory_give_the_same_bytes(pkg, shape):
    be = device_run(pkg, shape)
    le = run_pool(pkg, shape, CAP, dict(enumerate(scenario(shape))), {k: (s[1], mo.GAIN) for k, s in enumerate(SCENARIO)}, big_endian=False, on_device=True)
    for k in range(len(SCENARIO)):
        assert len(le[k]) == len(be[k]) == NBLOCKS
        for blk, (a, b) in enumerate(zip(be[k], le[k])):
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2], (shape, k, blk)


def test_without_the_floats_the_pcm_and_status_are_the_same(pkg):
    shape = "5ms"
    got = device_run(pkg, shape)
    b = scenario(shape)
    again = run_pool(pkg, shape, CAP, {k: b[k] for k in (1, 3, 4)}, {k: (SCENARIO[k][1], mo.GAIN) for k in (1, 3, 4)}, audio=False)
    for k in (1, 3, 4):
        for blk, (x, y) in enumerate(zip(got[k], again[k])):
            assert x[0].tobytes() == y[0].tobytes() and x[2] == y[2] and y[1] is None, (k, blk)


def test_capacity_8_gives_the_same_bytes(pkg):
    shape = "1ms"
    got = device_run(pkg, shape)
    again = run_pool(pkg, shape, 8, dict(enumerate(scenario(shape))), {k: (s[1], mo.GAIN) for k, s in enumerate(SCENARIO)})
    for k in range(len(SCENARIO)):
        for blk, (x, y) in enumerate(zip(got[k], again[k])):
            assert x[0].tobytes() == y[0].tobytes() and x[1].tobytes() == y[1].tobytes() and x[2] == y[2], (k, blk)


def test_released_and_added_again_starts_from_zero_with_the_default_parameters(pkg):
    shape = "1ms"
    bt = SHAPES[shape]
    blocks = scenario(shape)[0]
    pool = pkg.engine.MpxPool(bt, CAP)
    try:
        other = set_up(pool, mo.STEREO, bt, None)
        i = set_up(pool, mo.STEREO, bt, (0.5, 1.0))
        for blk in range(5):                                                # leave it with history, states and parameters of its own
            _, _, st = one_block(pool, i, ao.to_wire(blocks[blk]))
        assert st[1] != 0.0 and st[2] != 0.0
        pool.release(i)
        j = set_up(pool, mo.STEREO, bt, None)
        assert j == i and other != i
        got = [one_block(pool, j, ao.to_wire(blocks[blk])) for blk in range(3)]
        ref, twin = restatement(shape, False)[0][:3], restatement(shape, True)[0][:3]      # (instance 0 runs on the defaults: 75 us, gain 4)
        check(ref, twin, got, "1ms instance 0 after release and add")
        for blk in range(3):
            assert got[blk][0].tobytes() == device_run(pkg, shape)[0][blk][0].tobytes()
    finally:
        pool.close()


def test_set_params_between_blocks_takes_effect_on_the_next_block_and_the_states_carry_over(pkg):
    shape = "1ms"
    bt = SHAPES[shape]
    blocks = scenario(shape)[0]
    rate2, gain2 = mo.rate_of(50e-6), 2.0
    both = []
    for f32 in (False, True):
        d = mo.Decoder(bt, f32=f32)
        rows = [d.block(b) for b in blocks[:4]]
        d.rate, d.gain = rate2, gain2
        both.append(rows + [d.block(b) for b in blocks[4:8]])
    assert both[0][4]["audio"][0] != restatement(shape, False)[0][4]["audio"][0]
    pool = pkg.engine.MpxPool(bt, CAP)
    try:
        i = set_up(pool, mo.STEREO, bt, None)
        got = []
        for blk in range(8):
            if blk == 4:
                pool.set_params(i, pkg.engine.MpxParams(rate2, gain2))
            got.append(one_block(pool, i, ao.to_wire(blocks[blk])))
        check(both[0], both[1], got, "1ms instance 0, 75 us gain 4 -> 50 us gain 2 from block 4")
        for bad in ((1.0, 4.0), (-0.1, 4.0), (float("nan"), 4.0), (0.5, float("inf"))):
            with pytest.raises(pkg.engine.ChzError) as e:
                pool.set_params(i, pkg.engine.MpxParams(*bad))
            assert "out of range" in str(e.value), str(e.value)
    finally:
        pool.close()


def test_refused_calls_leave_state_and_outputs_untouched(pkg):
    """an instance listed twice, a released instance, a null row, n < 0 and a bad slave index, each between two good blocks of instance 0: the
    caller's buffers keep the sentinel, and the run matches the restatement (and the scenario's own run, byte for byte) as if nothing had happened"""
    shape = "1ms"
    bt = SHAPES[shape]
    blocks = scenario(shape)[0]
    E = pkg.engine
    pool = E.MpxPool(bt, CAP)
    try:
        a, b = set_up(pool, mo.STEREO, bt, None), set_up(pool, mo.STEREO, bt, None)
        pool.release(b)
        got = []
        for blk in range(NBLOCKS):
            row = ao.to_wire(blocks[blk])
            bad = {3: ([a, a], [row, row], "twice"), 4: ([a, b], [row, row], "not in use"), 5: ([a, a], [row, None], "bad request"),
                   6: ([a, 99], [row, row], "bad request")}.get(blk)
            if bad:
                with pytest.raises(E.ChzError) as e:
                    pool.execute(bad[0], bad[1], audio=True, fill=SENTINEL)
                assert bad[2] in str(e.value), str(e.value)
                assert (pool.last_raw == SENTINEL).all() and (pool.last_raw_audio.view(np.uint8) == SENTINEL).all()
            if blk == 7:                                                    # n < 0, on buffers of one request
                raw = np.full(4 * pool.olen, SENTINEL, np.uint8)
                st = np.full(C.sizeof(E.MpxStatus), SENTINEL, np.uint8)
                ii = np.array([a], np.int32)
                sp, pp = (C.c_void_p * 1)(row.ctypes.data), (C.c_void_p * 1)(raw.ctypes.data)
                assert E.lib().chz_mpx_execute(pool._h, -1, ii.ctypes.data, sp, 0, pp, None, st.ctypes.data) < 0
                assert "bad argument" in E.lib().chz_last_error().decode()
                assert (raw == SENTINEL).all() and (st == SENTINEL).all()
            if blk == 8:
                for slave in (-1, 3):
                    with pytest.raises(E.ChzError) as e:
                        pool.set_response(a, slave, mo.responses(bt)[0])
                    assert "slave" in str(e.value), str(e.value)
            got.append(one_block(pool, a, row))
        check(restatement(shape, False)[0], restatement(shape, True)[0], got, "1ms instance 0 between refused calls")
        for blk in range(NBLOCKS):
            assert got[blk][0].tobytes() == device_run(pkg, shape)[0][blk][0].tobytes() and got[blk][2] == device_run(pkg, shape)[0][blk][2], blk
    finally:
        pool.close()


NAN, INF = float("nan"), float("inf")
STEREO, RDS, BE, LE = 0, 1, 0, 1
REFUSALS = [((0.001, STEREO, BE), None), ((0.002, STEREO, BE), None), ((0.005, STEREO, LE), None), ((0.01, STEREO, BE), None), ((0.02, STEREO, BE), None),
            ((0.001, RDS, BE), None), ((0.005, RDS, LE), None), ((0.02, RDS, BE), None),
            ((0.0025, STEREO, BE), "19000 Hz between the even bins"),       # hzperbin 200: 19 kHz / 400 Hz = 47.5
            ((0.0025, RDS, BE), "between the even bins"),
            ((0.003, STEREO, BE), "384000 % 2304 != 0"),
            ((0.025, STEREO, BE), "16384"),                                 # N = 19200
            ((0.025, RDS, BE), "16384"),
            ((NAN, STEREO, BE), "block time"), ((INF, STEREO, BE), "block time"), ((0.0, STEREO, BE), "block time"), ((-0.005, STEREO, BE), "block time"),
            ((1e9, STEREO, BE), "16384"),
            ((0.005, 2, BE), "kind"), ((0.005, -1, BE), "kind"), ((0.005, STEREO, 2), "byte order"), ((0.005, RDS, -1), "byte order")]


@pytest.mark.parametrize("geom,word", REFUSALS)
def test_geometries_that_pass_and_that_are_refused(pkg, geom, word):
    E = pkg.engine
    bt, kind, order = geom
    if word is None:
        E.MpxPool.check(bt, kind, order)
        return
    for make in (lambda: E.MpxPool.check(bt, kind, order), lambda: E.MpxPool(bt, CAP, kind=kind, byte_order=order)):
        with pytest.raises(E.ChzError) as e:
            make()
        assert word in str(e.value), str(e.value)


RDS_BLOCKS = 8


@pytest.mark.parametrize("shape", ["5ms", "1ms"])
def test_rds_pools_pack_the_57_kHz_slave(pkg, shape):
    bt = SHAPES[shape]
    src = {k: mo.signal(RDS_BLOCKS, bt, 10 + k, a, rds=True) for k, a in enumerate((0.2, 0.9))}
    got = run_pool(pkg, shape, CAP, src, {0: None, 1: (0.0, 1.0)}, kind=mo.RDS)      # (the parameters are ignored)
    for k in src:
        ref, twin = (mo.run(src[k], bt, kind=mo.RDS, f32=f) for f in (False, True))
        assert all(r["audio"].any() for r in ref)
        check(ref, twin, got[k], "%s RDS instance %d" % (shape, k))
        assert all(st == (0, 0.0, 0.0) for _, _, st in got[k])
