"""Pools of stereo broadcast-FM decoders (chz_wfm_*, kernel wfm_ovs) against tests/wfm_oracle.py, the float64 restatement of
src/wfm.c:134-281 that tests/test_wfm_reference.py pins to the reference.

The two shapes that exist -- 10 ms (N = 7680, 61 KB of LDS) and 20 ms (N = 15360, 120 KB) -- each run ONE scenario of 5 instances
in a pool of capacity 2 (three launches per call) over 12 blocks, the order of the instances permuted from call to call:
  0  a stereo signal on a stereo instance, no de-emphasis
  1  a stereo signal on a stereo instance, 75 us de-emphasis
  2  the signal of instance 0 with stereo_enable = 0: the pilot slave must not decide anything
  3  pilot and L-R removed from block 5 and restored from block 9: channels 2 -> 1 -> 2, each de-emphasis state resumes where it stopped
  4  a scripted squelch (tail 2, open 10, close 6.3): snr 100, 100, 8 (held open), 1, 1 (tail), 1 (closed), 1, 8 (stays closed), 100 (reopens
     on the old history with phase_memory = 0), ...
The scenario and its restatement (float64, and the f32 twin) are computed once per shape and shared by the tests.

Bounds.  frame, mute, squelch_state, channels, pilot_present and gain: equal on every block.  snr, foffset, pdeviation, subc_amp,
output_power: 1e-6 relative, or 4 x the f32 twin's own distance from the float64 run where that is larger.  Float PCM per block:
rel-L2 <= REL_L2 and max-abs <= MAXABS_RMS x rms (tests/test_gpu_parity.py), or 4 x the twin's own error on that block where the
twin's error exceeds a quarter of the figure.  The first three executed blocks of an instance are compared discretely only: the
pilot filter's precursor is about 1e-23 there and p^2/|p|^2 normalises rounding noise, in the reference too.
Input conditions, asserted on the restatement before anything is compared: every phase difference at least 0.1 away from the +-1
wrap, subc_amp outside [1e-7, 1e-5], every scripted snr at least 10 % away from `open` and `close`."""
import functools

import numpy as np
import pytest

import oracle_lib as ol
import pcm_edge_cases as pe
import wfm_oracle as wo
from conftest import load_pkg
from test_gpu_parity import MAXABS_RMS, REL_L2

pytestmark = pytest.mark.gpu

SHAPES = {"10ms": 0.01, "20ms": 0.02}
NINST, CAP, NBLOCKS, SETTLE = 5, 2, 12, 3
RATE75 = float(-np.expm1(-1.0 / (75e-6 * wo.AUDIO_RATE)))       # chan->fm.rate of the wfm preset (deemph-tc = 75 us at 48 kHz)
BW, HEADROOM = 220000.0, 10 ** (-15 / 20)
SNR_SCRIPT = [100, 100, 8, 1, 1, 1, 1, 8, 100, 100, 100, 100]
STEREO_SCRIPT = [1] * 5 + [0] * 4 + [1] * 3
SENTINEL = 0xA5
# per instance: (signal seed, stereo script, stereo_enable, deemph_rate, snr script)
SCENARIO = [(1, None, 1, 0.0, None), (2, None, 1, RATE75, None), (1, None, 0, 0.0, None), (3, STEREO_SCRIPT, 1, RATE75, None), (4, None, 1, RATE75, SNR_SCRIPT)]


@pytest.fixture(scope="module")
def pkg():
    p = load_pkg()
    if p.engine.lib().chz_device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests cannot run (there is no CPU fallback)")
    ol.build()
    return p


@functools.lru_cache(maxsize=None)
def inputs(shape):
    """(bb complex64 [NINST][NBLOCKS][L], bb_power [NINST][NBLOCKS], n0 [NINST][NBLOCKS], responses)"""
    bt = SHAPES[shape]
    bb = np.stack([wo.synthesise(NBLOCKS, bt, seed, stereo) for seed, stereo, _, _, _ in SCENARIO])
    power = np.mean(np.abs(bb.astype(np.complex128)) ** 2, axis=2)
    snr = np.array([[100.0] * NBLOCKS if s[4] is None else s[4] for s in SCENARIO], np.float64)
    n0 = power / ((snr + 1) * BW)
    return bb, power, n0, wo.responses(bt)


def wfm_params(pkg, stereo_enable, rate, encoding):
    return pkg.engine.WfmParams(stereo_enable=stereo_enable, encoding=encoding, squelch_tail=2, squelch_open=10.0, squelch_close=6.3,
                                bandwidth=BW, headroom=HEADROOM, deemph_rate=rate, deemph_gain=1.0)


def status_tuple(s):
    return tuple(getattr(s, k) for k, _ in type(s)._fields_)


def run_pool(pkg, shape, cap, nblocks=NBLOCKS, seed=7):
    """the scenario through a pool of capacity `cap`: [inst][block] -> (PCM bytes, status tuple, the untouched rest of the buffer is the sentinel)"""
    bb, power, n0, resp = inputs(shape)
    pool = pkg.engine.WfmPool(SHAPES[shape], cap)
    try:
        insts = [pool.add() for _ in range(NINST)]
        for i, (_, _, st_en, rate, _) in zip(insts, SCENARIO):
            pool.set_params(i, wfm_params(pkg, st_en, rate, pkg.engine.PCM_F32LE))
            for s in range(3):
                pool.set_response(i, s, resp[s])
        rng = np.random.default_rng(seed)
        out = [[None] * nblocks for _ in range(NINST)]
        for blk in range(nblocks):
            order = rng.permutation(NINST)
            pcm, st = pool.execute([insts[k] for k in order], bb[order, blk], power[order, blk], n0[order, blk], fill=SENTINEL)
            for r, k in enumerate(order):
                assert (pool.last_raw[r, len(pcm[r]):] == SENTINEL).all(), "bytes behind the frame were written"
                out[k][blk] = (pcm[r], status_tuple(st[r]))
        return out
    finally:
        pool.close()


@functools.lru_cache(maxsize=None)
def restatement(shape, f32):
    bb, power, n0, resp = inputs(shape)
    out = []
    for k, (_, _, st_en, rate, _) in enumerate(SCENARIO):
        d = wo.Decoder(SHAPES[shape], resp, stereo_enable=st_en, squelch_open=10.0, squelch_close=6.3, squelch_tail=2, bandwidth=BW, headroom=HEADROOM,
                       deemph_rate=rate, deemph_gain=1.0, f32=f32)
        out.append([d.block(bb[k, blk], power[k, blk], n0[k, blk]) for blk in range(NBLOCKS)])
    return out


_device_runs = {}


def device_run(pkg, shape):
    if shape not in _device_runs:
        _device_runs[shape] = run_pool(pkg, shape, CAP)
    return _device_runs[shape]


def rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


def check_instance(shape, k, got, fields=wo.CONTINUOUS):
    """one instance of the scenario against the restatement; returns the worst measured / allowed ratios"""
    ref, twin = restatement(shape, False)[k], restatement(shape, True)[k]
    names = [n for n, _ in load_pkg().engine.WfmStatus._fields_]
    executed = 0
    worst = {"status": 0.0, "rel_l2": 0.0, "maxabs": 0.0}
    for blk in range(NBLOCKS):
        r, t = ref[blk], twin[blk]
        pcm, st = got[blk]
        st = dict(zip(names, st))
        # input conditions
        assert r["wrap_margin"] >= 0.1, (k, blk, "a phase difference within 0.1 of the wrap", r["wrap_margin"])
        assert SCENARIO[k][4] is None or r["snr_margin"] >= 0.1, (k, blk, "scripted snr too close to a threshold")
        if SCENARIO[k][2] and r["frame"] == 0:
            assert not 1e-7 <= r["subc_amp"] <= 1e-5, (k, blk, "pilot amplitude too close to the detector's threshold", r["subc_amp"])
        for f in wo.DISCRETE:
            assert st[f] == r[f], (shape, k, blk, f, st[f], r[f])
            assert t[f] == r[f], (shape, k, blk, f, "the f32 twin takes another decision: unusable input")
        assert st["gain"] == r["gain"], (shape, k, blk, st["gain"], r["gain"])
        if r["frame"]:
            assert len(pcm) == 0 and st["output_power"] == 0.0
            assert st["snr"] == r["snr"] or rel(st["snr"], r["snr"]) <= 1e-6
            for f in ("foffset", "pdeviation"):                           # reported unchanged while the squelch is closed
                lim = max(1e-6, 4 * rel(t[f], r[f]))
                e = rel(st[f], r[f]) if r[f] != 0 else abs(st[f])
                assert e <= lim, (shape, k, blk, f, "on a closed block", st[f], r[f], e, lim)
            continue
        executed += 1
        assert len(pcm) == 4 * wo.geometry(SHAPES[shape])[2] * r["channels"]
        if executed <= SETTLE:
            continue
        for f in fields:
            lim = max(1e-6, 4 * rel(t[f], r[f]))
            e = rel(st[f], r[f]) if r[f] != 0 else abs(st[f])
            worst["status"] = max(worst["status"], e / lim)
            assert e <= lim, (shape, k, blk, f, st[f], r[f], e, lim)
        g = np.frombuffer(pcm.tobytes(), "<f4").astype(np.float64)
        w, tw = r["pcm"].astype(np.float64), t["pcm"].astype(np.float64)
        rms = float(np.sqrt(np.mean(w ** 2)))
        err, terr = float(np.sqrt(np.mean((g - w) ** 2))), float(np.sqrt(np.mean((tw - w) ** 2)))
        mx, tmx = float(np.abs(g - w).max()), float(np.abs(tw - w).max())
        lim_l2 = REL_L2 * rms if terr <= 0.25 * REL_L2 * rms else 4 * terr
        lim_mx = MAXABS_RMS * rms if tmx <= 0.25 * MAXABS_RMS * rms else 4 * tmx
        worst["rel_l2"] = max(worst["rel_l2"], err / lim_l2); worst["maxabs"] = max(worst["maxabs"], mx / lim_mx)
        assert err <= lim_l2, (shape, k, blk, "rel-L2", err / rms, lim_l2 / rms)
        assert mx <= lim_mx, (shape, k, blk, "max-abs over rms", mx / rms, lim_mx / rms)
    print("%s instance %d: worst measured / allowed: status %.3g, PCM rel-L2 %.3g, PCM max-abs %.3g" % (shape, k, worst["status"], worst["rel_l2"], worst["maxabs"]))
    return worst


@pytest.mark.parametrize("shape", list(SHAPES))
def test_geometry_and_lds(pkg, shape):
    pool = pkg.engine.WfmPool(SHAPES[shape], CAP)
    try:
        assert tuple(pool.geometry.values()) == wo.geometry(SHAPES[shape])
        assert pool.geometry["pilot_shift"] % 4 == 0 and pool.geometry["subc_shift"] == 2 * pool.geometry["pilot_shift"]
    finally:
        pool.close()


@pytest.mark.parametrize("shape", list(SHAPES))
def test_stereo_signal_on_stereo_instances_with_and_without_deemphasis(pkg, shape):
    got = device_run(pkg, shape)
    for k in (0, 1):
        check_instance(shape, k, got[k])
        assert all(st[3] == 2 and st[4] == 1 for _, st in got[k])        # channels, pilot_present


@pytest.mark.parametrize("shape", list(SHAPES))
def test_stereo_disabled_the_pilot_decides_nothing(pkg, shape):
    got = device_run(pkg, shape)
    check_instance(shape, 2, got[2])
    assert all(st[3] == 1 and st[4] == 0 and st[-1] == 0.0 for _, st in got[2])


@pytest.mark.parametrize("shape", list(SHAPES))
def test_pilot_lost_and_restored(pkg, shape):
    got = device_run(pkg, shape)
    check_instance(shape, 3, got[3])
    ch = [st[3] for _, st in got[3]]
    assert ch[0] == 2 and 1 in ch[5:9] and ch[-1] == 2 and ch[6:9] == [1, 1, 1], ch


@pytest.mark.parametrize("shape", list(SHAPES))
def test_scripted_squelch(pkg, shape):
    got = device_run(pkg, shape)
    check_instance(shape, 4, got[4])
    assert [st[2] for _, st in got[4]] == [3, 3, 3, 2, 1, 0, 0, 0, 3, 3, 3, 3]
    assert [st[0] for _, st in got[4]] == [0] * 5 + [1] * 3 + [0] * 4     # frame: no samples while closed, the PCM buffer untouched (run_pool checks the sentinel)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_all_eight_encodings_pack_the_f32_instance_s_floats(pkg, shape):
    bb, power, n0, resp = inputs(shape)
    E = pkg.engine
    encs = [E.PCM_S16BE, E.PCM_S16LE, E.PCM_F32LE, E.PCM_F32BE, E.PCM_MULAW, E.PCM_ALAW, E.PCM_F16LE, E.PCM_F16BE]
    assert encs == [ol.PCM_S16BE, ol.PCM_S16LE, ol.PCM_F32LE, ol.PCM_F32BE, ol.PCM_MULAW, ol.PCM_ALAW, ol.PCM_F16LE, ol.PCM_F16BE]
    pool = E.WfmPool(SHAPES[shape], 8)
    try:
        insts = [pool.add() for _ in encs]
        for i, e in zip(insts, encs):
            pool.set_params(i, wfm_params(pkg, 1, RATE75, e))
            for s in range(3):
                pool.set_response(i, s, resp[s])
        for blk in range(4):
            k = 3 if blk == 3 else 1                      # a stereo signal, and one block of the signal without pilot (mono frames)
            sb = 6 if blk == 3 else blk
            pcm, st = pool.execute(insts, np.stack([bb[k, sb]] * 8), [power[k, sb]] * 8, [n0[k, sb]] * 8)
            floats = np.frombuffer(pcm[2].tobytes(), "<f4")
            assert floats.size == pool.olen * st[2].channels and floats.any()
            for j, e in enumerate(encs):
                assert np.array_equal(pcm[j], pe.pack(ol, e, floats)), (shape, blk, "encoding", e)
    finally:
        pool.close()


@pytest.mark.parametrize("shape", list(SHAPES))
def test_capacity_8_and_a_second_pool_give_the_same_bits(pkg, shape):
    got = device_run(pkg, shape)
    for cap in (8, CAP):
        again = run_pool(pkg, shape, cap)
        for k in range(NINST):
            for blk in range(NBLOCKS):
                assert np.array_equal(again[k][blk][0], got[k][blk][0]), (shape, cap, k, blk, "PCM")
                assert np.array(again[k][blk][1]).tobytes() == np.array(got[k][blk][1]).tobytes(), (shape, cap, k, blk, "status")


@pytest.mark.parametrize("lanes", [1, 7])
def test_other_deemphasis_lane_counts(pkg, lanes):
    """option wfm_deemph_lanes: one lane walking the block, and a count that does not divide it (480 samples in runs of 69, the last one short),
    against the restatement on the instances with de-emphasis -- stereo, mono after the pilot is lost, and through the squelch script"""
    L = pkg.engine.lib()
    pkg.engine._check(L.chz_set_option(b"wfm_deemph_lanes", str(lanes).encode()))
    try:
        got = run_pool(pkg, "10ms", CAP)
    finally:
        pkg.engine._check(L.chz_set_option(b"wfm_deemph_lanes", None))
    for k in (1, 3, 4):
        check_instance("10ms", k, got[k])


def test_instances_added_in_mid_stream_beyond_the_capacity(pkg):
    """a pool of capacity 2 whose storage grows twice while decoders run (2 -> 4 -> 8 instances): state, history and responses of the running
    instances move to the new arrays, the newcomers start from zero.  Instances 1 and 3 of the scenario run from the start, 0 joins at call 5 and
    2 at call 7; everybody's 12 blocks against the restatement."""
    shape = "10ms"
    bb, power, n0, resp = inputs(shape)
    E = pkg.engine
    pool = E.WfmPool(SHAPES[shape], CAP)
    try:
        inst, got, start = {}, {}, {1: 0, 3: 0, 0: 5, 2: 7, 4: 7}

        def join(k):
            inst[k] = pool.add(); got[k] = []
            pool.set_params(inst[k], wfm_params(pkg, SCENARIO[k][2], SCENARIO[k][3], E.PCM_F32LE))
            for s in range(3):
                pool.set_response(inst[k], s, resp[s])
        for call in range(7 + NBLOCKS):
            for k in sorted(start):
                if start[k] == call:
                    join(k)
            due = [k for k in sorted(inst) if len(got[k]) < NBLOCKS]
            blk = [len(got[k]) for k in due]
            pcm, st = pool.execute([inst[k] for k in due], np.stack([bb[k, b] for k, b in zip(due, blk)]), [power[k, b] for k, b in zip(due, blk)],
                                   [n0[k, b] for k, b in zip(due, blk)])
            for r, k in enumerate(due):
                got[k].append((pcm[r], status_tuple(st[r])))
        assert sorted(inst.values()) == list(range(5))
        for k in sorted(got):
            check_instance(shape, k, got[k])
    finally:
        pool.close()


def test_device_source_equals_host_source(pkg):
    """An Engine on mini_radiod_lib.WFM_GEOM with one bank of 3 WFM-sized channels (P 9600, olen 7680): execute(on_device=True) on the
    rows of chz_bank_output_device after chz_slot_sync against execute on the same rows read back with chz_bank_read."""
    import mini_radiod_lib as mr
    fs, L, M = mr.WFM_GEOM
    L, M = int(L), int(M)
    N, P, olen, nch, nblk = L + M - 1, 9600, 7680, 3, 3
    shifts = np.array([10000, 18500, 27000], np.int32)
    t = np.arange(nblk * L) / fs
    rng = np.random.default_rng(8)
    x = 0.002 * rng.standard_normal(t.size)
    for c, sh in enumerate(shifts):
        mpx = 0.45 * np.sin(2 * np.pi * (1000.0 + 300 * c) * t) + 0.09 * np.sin(2 * np.pi * 19000.0 * t) + 0.3 * np.sin(2 * np.pi * 1700.0 * t) * np.sin(2 * np.pi * 38000.0 * t)
        x += 0.05 * np.cos(2 * np.pi * sh * (fs / N) * t + 2 * np.pi * 75000.0 * np.cumsum(mpx) / fs)
    x = x.astype(np.float32)
    E = pkg.engine
    eng = E.Engine(L, M, ol.REAL)
    pools = [E.WfmPool(0.02, CAP), E.WfmPool(0.02, CAP)]
    try:
        bank = eng.bank(P, olen, nch)
        bank.set_responses(0, np.stack([ol.set_filter(P, olen, N, True, -110000.0 / 384000.0, 110000.0 / 384000.0, 11.0)] * nch))
        bank.set_active(nch); bank.set_tuning(0, 0, shifts, np.zeros(nch))       # (a tuned bank keeps bb_power; the remainders are zero)
        resp = inputs("20ms")[3]
        insts = []
        for pool in pools:
            ii = [pool.add() for _ in range(nch)]
            for c, i in enumerate(ii):
                pool.set_params(i, wfm_params(pkg, 1, RATE75, [E.PCM_S16BE, E.PCM_F32LE, E.PCM_S16LE][c]))
                for s in range(3):
                    pool.set_response(i, s, resp[s])
            insts.append(ii)
        for blk in range(nblk):
            eng.write(x[blk * L:(blk + 1) * L]); eng.step(blk)
            slot = blk % 4
            eng.slot_sync(slot)
            power = bank.read_power(slot)
            n0 = power / (101.0 * BW)
            rows = bank.read()
            base = bank.output_ptr(slot)
            dev, dst = pools[0].execute(insts[0], [base + 8 * olen * c for c in range(nch)], power, n0, on_device=True)
            host, hst = pools[1].execute(insts[1], rows, power, n0)
            for c in range(nch):
                assert dst[c].frame == 0 and len(dev[c]) > 0
                assert np.array_equal(dev[c], host[c]), (blk, c)
                assert status_tuple(dst[c]) == status_tuple(hst[c]), (blk, c)
    finally:
        for pool in pools:
            pool.close()
        eng.close()


@pytest.mark.parametrize("blocktime,word", [(0.005, "multiple of 4"), (0.04, "16384")])
def test_block_times_that_are_refused(pkg, blocktime, word):
    for make in (lambda: pkg.engine.WfmPool.check(blocktime), lambda: pkg.engine.WfmPool(blocktime, CAP)):
        with pytest.raises(pkg.engine.ChzError) as e:
            make()
        assert word in str(e.value), str(e.value)


def test_refused_calls_leave_state_and_outputs_untouched(pkg):
    """an instance listed twice, an instance not in use and a null row, each between two good blocks of instance 1 of the scenario: the
    block after the refusal matches the restatement as if nothing had happened"""
    shape = "10ms"
    bb, power, n0, resp = inputs(shape)
    E = pkg.engine
    pool = E.WfmPool(SHAPES[shape], CAP)
    try:
        a, b = pool.add(), pool.add()
        for i in (a, b):
            pool.set_params(i, wfm_params(pkg, SCENARIO[1][2], SCENARIO[1][3], E.PCM_F32LE))
            for s in range(3):
                pool.set_response(i, s, resp[s])
        pool.release(b)
        names = [n for n, _ in E.WfmStatus._fields_]
        got = []
        two = lambda blk: (np.stack([bb[1, blk]] * 2), [power[1, blk]] * 2, [n0[1, blk]] * 2)
        for blk in range(NBLOCKS):
            if blk in (4, 5, 6):
                x, pw, nz = two(blk)
                with pytest.raises(E.ChzError) as e:
                    if blk == 4:
                        pool.execute([a, a], x, pw, nz, fill=SENTINEL)
                    elif blk == 5:
                        pool.execute([a, b], x, pw, nz, fill=SENTINEL)
                    else:
                        pool.execute([a, a], [x[0], None], pw, nz, fill=SENTINEL)          # a null row on the host source
                assert ("twice", "not in use", "bad request")[blk - 4] in str(e.value), str(e.value)
                assert (pool.last_raw == SENTINEL).all()
            pcm, st = pool.execute([a], bb[1, blk:blk + 1], power[1, blk:blk + 1], n0[1, blk:blk + 1])
            got.append((pcm[0], status_tuple(st[0])))
        assert names[0] == "frame"
        check_instance(shape, 1, got)
    finally:
        pool.close()
