"""Instance storage that grows while decoders run: AfskPool, CtcssPool and MpxPool (STEREO), after
test_instances_added_in_mid_stream_beyond_the_capacity of tests/test_gpu_wfm.py.

All three pools double their instance storage when `add` finds it full (afsk_grow, ctcss_grow, mpx_grow: allocate, copy device-to-device,
swap pointers).  Every other test adds all its instances before the first block, so that copy has only ever moved zeros.  Here a pool of
capacity 2 runs instances 0 and 1 from call 0; 2, 3 and 4 join at later calls, so the storage goes 2 -> 4 -> 8 under running decoders; then the
index of instance 2 is released and added again as instance 5.  What the running instances hold at each growth is asserted on the restatement:
  AFSK   (L 480, M 481, 11025 Hz / 1200 bd: samppbit 9 of 9.19)  inside the 330-byte frame: frame_bits > 0, flag_seen = 1, symphase != 0
  CTCSS  (8 kHz)  after the first renormalisation of the oscillators (block 163), their step counter in mid-count, a sticky current tone
         (tone_index -1, current_index 54): instance 0 of tests/test_gpu_ctcss.py's scenario, and the same behind one block of zeros
  MPX    (2 ms, STEREO)  non-zero de-emphasis states, and parameters set by set_params that are not the defaults (50 us, gain 2; rate 0.5, gain 1)
Asserted: every instance's whole run equals the restatement under the rule of its pool's own test file (check_strict / check, unchanged); status
bytes and outputs are bit-identical to a second pool of capacity 8, whose storage never grows, fed the same calls; the re-added index starts from
zero (and, MPX, with the default parameters: it is given none).

The inputs are those of the pools' own files and meet their input conditions there (tests/test_gpu_afsk_rates.py, tests/test_gpu_ctcss.py) or
are checked here by the same functions; the tests print the same figures as those files.  Measured on the MI355X, worst measured / allowed: AFSK last_val 0.43,
mid_val 0.59 (FLOOR 1.2e-5, smallest margin 3.4e-5); CTCSS 0.69 (FLOOR 1.7e-5, smallest margin 9.0e-5, instance 1's in block 76: instance 0's block 75 behind
the block of zeros); MPX rel-L2 0.018, max-abs 0.006, states 0.005.  No defect found: the three grow functions copy what they must."""
import numpy as np
import pytest

import afsk_oracle as ao
import ctcss_oracle as co
import mpx_oracle as mo
import oracle_lib as ol
import test_gpu_afsk as ga
import test_gpu_afsk_rates            # noqa: F401  (registers the 11k shape with test_gpu_afsk)
import test_gpu_ctcss as gc
import test_gpu_mpx as gm
from conftest import load_pkg

pytestmark = pytest.mark.gpu

CAP = 2


@pytest.fixture(scope="module")
def pkg():
    p = load_pkg()
    if p.engine.lib().chz_device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests cannot run (there is no CPU fallback)")
    ol.build()
    return p


def drive(cap, start, nblocks, released, join, leave, step):
    """The calls of one pool.  start: {k: the call at which instance k joins}; released: {k: (call, j)}: at that call instance j's index is
    released and k takes it.  join(k) -> index, leave(index), step([(k, index, block)]) -> one comparable record per request.
    -> ({k: records}, {k: index})"""
    inst, got = {}, {k: [] for k in start}
    last = max(start[k] + nblocks[k] for k in start)
    for call in range(last):
        for k in sorted(start):
            if start[k] == call:
                if k in released:
                    assert len(got[released[k][1]]) == nblocks[released[k][1]], "the released instance has not finished"
                    leave(inst[released[k][1]])
                inst[k] = join(k)
                if k in released:
                    assert inst[k] == inst[released[k][1]], "the released index was not handed out again"
        due = [k for k in sorted(start) if k in inst and len(got[k]) < nblocks[k]]
        if due:
            for k, rec in zip(due, step([(k, inst[k], len(got[k])) for k in due])):
                got[k].append(rec)
    return got, inst


def same_bytes(a, b, raw):
    assert sorted(a) == sorted(b)
    for k in a:
        assert len(a[k]) == len(b[k])
        for blk, (x, y) in enumerate(zip(a[k], b[k])):
            assert raw(x) == raw(y), (k, blk, "a pool whose storage grew differs from one whose storage did not")


# ---- AFSK -------------------------------------------------------------------------------------------------------------------------------
AFSK_SHAPE = "11k"
AFSK_START = {0: 0, 1: 0, 2: 38, 3: 46, 4: 56, 5: 133}      # 2 -> 4 at call 38, 4 -> 8 at call 56; instance 2 (77 blocks from call 38) ends at call 115
AFSK_SRC = {0: 0, 1: 1, 2: 0, 3: 1, 4: 0, 5: 1}             # which of the scenario's two inputs an instance takes, from its block 0


def afsk_run(pkg, cap):
    L, M, fs, br, mk, sp = ga.geom(AFSK_SHAPE)
    blocks = ga.scenario(AFSK_SHAPE)[0]
    E = pkg.engine
    pool = E.AfskPool(L, M, fs, cap, bitrate=br, mark=mk, space=sp, frame_stride=ga.STRIDE)
    resp = ao.response(L, M, fs, br, mk, sp)
    try:
        def join(k):
            i = pool.add()
            pool.set_response(i, resp)
            return i

        def step(reqs):
            raw, sraw = ga.buffers(len(reqs))
            st, fr = pool.execute([i for _, i, _ in reqs], [ao.to_wire(blocks[AFSK_SRC[k]][b]) for k, _, b in reqs], frames_buf=raw, status_buf=sraw)
            return [(ga.status_dict(st[r]), sraw[r].tobytes() + raw[r].tobytes(), fr[r]) for r in range(len(reqs))]
        return drive(cap, AFSK_START, {k: len(blocks[AFSK_SRC[k]]) for k in AFSK_START}, {5: (AFSK_START[5], 2)}, join, pool.release, step)
    finally:
        pool.close()


def test_afsk_storage_grows_under_decoders_inside_a_frame(pkg):
    ref = ga.restatement(AFSK_SHAPE, False)
    for call in (AFSK_START[2], AFSK_START[4]):              # what the two running instances hold when the storage is copied
        for k in (0, 1):
            r = ref[k][call - 1]
            assert r["frame_bits"] > 500 and r["flag_seen"] == 1 and r["symphase"] != 0 and r["last_val"] != 0.0, (call, k, r["frame_bits"], r["symphase"])
    for k, call in ((2, AFSK_START[4]), (3, AFSK_START[4])):  # ... and the newcomers of the first growth at the second
        assert ref[AFSK_SRC[k]][call - AFSK_START[k] - 1]["ndecisions"] > 0
    got, inst = afsk_run(pkg, CAP)
    assert [inst[k] for k in range(5)] == [0, 1, 2, 3, 4] and inst[5] == inst[2]
    for k in sorted(got):
        ga.check_strict(AFSK_SHAPE, k, got[k], kref=AFSK_SRC[k], last_val_may_cancel=True)
    never_grew, _ = afsk_run(pkg, 8)
    same_bytes(got, never_grew, lambda rec: (rec[1], rec[2]))


# ---- CTCSS ------------------------------------------------------------------------------------------------------------------------------
CTCSS_FS = 8000.0
CTCSS_START = {0: 0, 1: 0, 2: 168, 3: 169, 4: 170, 5: 205}   # 2 -> 4 at call 168, 4 -> 8 at call 170; instance 2 (36 blocks) ends at call 204


def ctcss_inputs():
    b = gc.scenario("8k")
    behind = np.concatenate([np.zeros((1, b[0].shape[1]), np.int16), b[0]])      # instance 0's input behind one block of zeros
    return {0: b[0], 1: behind, 2: b[1], 3: b[2], 4: b[1], 5: b[2]}


def ctcss_run(pkg, cap, src):
    E = pkg.engine
    pool = E.CtcssPool(CTCSS_FS, cap)
    resp = co.response(CTCSS_FS)
    try:
        def join(k):
            i = pool.add()
            pool.set_response(i, resp)
            return i

        def step(reqs):
            sraw, en = gc.buffers(len(reqs))
            st = pool.execute([i for _, i, _ in reqs], [ao.to_wire(src[k][b]) for k, _, b in reqs], status_buf=sraw, energies=en)
            return [(E.CtcssStatus(st[r].tone_index, st[r].current_index, st[r].energy), en[r].copy(), sraw[r].tobytes()) for r in range(len(reqs))]
        return drive(cap, CTCSS_START, {k: len(src[k]) for k in CTCSS_START}, {5: (CTCSS_START[5], 2)}, join, pool.release, step)
    finally:
        pool.close()


def test_ctcss_storage_grows_under_decoders_with_a_sticky_tone_behind_the_first_renormalisation(pkg):
    src = ctcss_inputs()
    ref = {k: co.run(src[k], CTCSS_FS) for k in (0, 1)}
    twin = {k: co.run(src[k], CTCSS_FS, f32=True) for k in (0, 1)}
    for call in (CTCSS_START[2], CTCSS_START[4]):
        steps = co.OLEN * call                                # oscillator steps taken so far: past the first renormalisation, the counter in mid-count
        assert steps > ao.RENORM and steps % ao.RENORM != 0
        for k in (0, 1):
            r = ref[k][call - 1]
            assert (r["tone_index"], r["current_index"]) == (-1, 54), (call, k, r["tone_index"], r["current_index"])
    got, inst = ctcss_run(pkg, CAP, src)
    assert [inst[k] for k in range(5)] == [0, 1, 2, 3, 4] and inst[5] == inst[2]
    scen_ref, scen_twin = gc.restatement("8k", False), gc.restatement("8k", True)
    for k in sorted(got):
        r, t = (ref[k], twin[k]) if k in ref else (scen_ref[1 if k in (2, 4) else 2], scen_twin[1 if k in (2, 4) else 2])
        gc.check(r, t, gc.pairs(got[k]), "8k growth instance %d" % k)
    never_grew, _ = ctcss_run(pkg, 8, src)
    same_bytes(got, never_grew, lambda rec: (rec[2], rec[1].tobytes()))


# ---- MPX --------------------------------------------------------------------------------------------------------------------------------
MPX_BT = 0.002
MPX_BLOCKS = 24
MPX_START = {0: 0, 1: 0, 2: 6, 3: 9, 4: 12, 5: 31}           # 2 -> 4 at call 6, 4 -> 8 at call 12; instance 2 ends at call 30
# (amplitude, (rate, gain) or None for the defaults, which the re-added index must have)
MPX_SCEN = {0: (0.2, (mo.rate_of(50e-6), 2.0)), 1: (0.3, (0.5, 1.0)), 2: (0.2, (mo.rate_of(25e-6), 3.0)), 3: (0.2, None), 4: (0.5, (0.0, 1.0)), 5: (0.2, None)}


def mpx_run(pkg, cap, src):
    E = pkg.engine
    pool = E.MpxPool(MPX_BT, cap)
    try:
        def step(reqs):
            pcm, au, st = pool.execute([i for _, i, _ in reqs], [ao.to_wire(src[k][b]) for k, _, b in reqs], audio=True, fill=gm.SENTINEL)
            assert (pool.last_raw[:, 4 * pool.olen:] == gm.SENTINEL).all(), "bytes behind the PCM row were written"
            return [(pcm[r], au[r], (st[r].zero_pilot, st[r].deemph_left, st[r].deemph_right)) for r in range(len(reqs))]
        return drive(cap, MPX_START, {k: MPX_BLOCKS for k in MPX_START}, {5: (MPX_START[5], 2)}, lambda k: gm.set_up(pool, mo.STEREO, MPX_BT, MPX_SCEN[k][1]),
                     pool.release, step)
    finally:
        pool.close()


def test_mpx_storage_grows_under_decoders_with_states_and_parameters_of_their_own(pkg):
    src = {k: mo.signal(MPX_BLOCKS, MPX_BT, 20 + k, a) for k, (a, _) in MPX_SCEN.items()}
    par = {k: p if p is not None else (mo.RATE75, mo.GAIN) for k, (_, p) in MPX_SCEN.items()}
    ref = {k: mo.run(src[k], MPX_BT, rate=par[k][0], gain=par[k][1]) for k in src}
    twin = {k: mo.run(src[k], MPX_BT, rate=par[k][0], gain=par[k][1], f32=True) for k in src}
    for call in (MPX_START[2], MPX_START[4]):
        for k in (0, 1):
            r = ref[k][call - 1]
            assert abs(r["deemph_left"]) > 1e-3 and abs(r["deemph_right"]) > 1e-3 and par[k] != (mo.RATE75, mo.GAIN), (call, k)
    got, inst = mpx_run(pkg, CAP, src)
    assert [inst[k] for k in range(5)] == [0, 1, 2, 3, 4] and inst[5] == inst[2]
    assert par[2] != par[5] == (mo.RATE75, mo.GAIN)           # the index's former tenant had parameters of its own; the new one is given none
    for k in sorted(got):
        gm.check(ref[k], twin[k], got[k], "2 ms growth instance %d" % k)
    never_grew, _ = mpx_run(pkg, 8, src)
    same_bytes(got, never_grew, lambda rec: (rec[0].tobytes(), rec[1].tobytes(), rec[2]))
