"""Pools of FM-multiplex decoders (chz_mpx_*, kernel mpx_ovs) at the two block times mpx_check_geom passes and tests/test_gpu_mpx.py only
hands to the check call: 2 ms (L 768, N 1536, olen 96, P 192, shifts 76 / 152 / 228) and 10 ms (L 3840, N 7680, olen 480, P 960, shifts
380 / 760 / 1140).  Through that file's own helpers, unchanged: instances 0, 1 and 2 of its STEREO scenario (75 us, 50 us, no memory: the
clip edge) in a big-endian pool of capacity 2 together with instances 3 and 4 (the launches' companions, compared as well), 12 blocks, the
order permuted from call to call; and its RDS pools (2 instances, 8 blocks).

Bounds: those of tests/test_gpu_mpx.py -- zero_pilot equal, the PCM bytes mpx_oracle.pack() of the device's own floats byte for byte, the
floats by rule (A) against tests/mpx_oracle.py's float64 values, the de-emphasis states within the block's max-abs limit; the input
condition (the f32 twin counts the same zero pilots) is asserted by check() before anything is compared.

tests/mpx_oracle.py takes the block time alone (geometry(), responses() and signal() derive everything from it), and tests/test_mpx_reference.py
pins its STEREO loop to stereod.c at these two block times as at the other three.  rdsd's Blocktime is a constant of 5 ms: the RDS pools
here rest on the restatement's parametrisation, as the 1 ms RDS pool of tests/test_gpu_mpx.py does.

Measured: instance 2's peak is 1.005 at 2 ms and 1.019 at 10 ms, so the clip edge is met at both (asserted).  Worst measured / allowed on the
MI355X: rel-L2 0.016 (STEREO), 0.024 (RDS), max-abs 0.009, states 0.004 (the CPU build of the engine: 0.015, 0.024, 0.008, 0.003); the tests print theirs."""
import numpy as np
import pytest

import mpx_oracle as mo
import oracle_lib as ol
from conftest import load_pkg
from test_gpu_mpx import CAP, NBLOCKS, RDS_BLOCKS, check, check_instance, device_run, restatement, run_pool

pytestmark = pytest.mark.gpu

TIMES = [0.002, 0.01]
GEOMETRY = {0.002: (768, 769, 1536, 96, 192, 76, 152, 228), 0.01: (3840, 3841, 7680, 480, 960, 380, 760, 1140)}      # ..., pilot, 38 kHz, 57 kHz


@pytest.fixture(scope="module")
def pkg():
    p = load_pkg()
    if p.engine.lib().chz_device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests cannot run (there is no CPU fallback)")
    ol.build()
    return p


@pytest.mark.parametrize("bt", TIMES)
def test_geometry(pkg, bt):
    E = pkg.engine
    for kind in (E.MPX_STEREO, E.MPX_RDS):
        pool = E.MpxPool(bt, CAP, kind=kind)
        try:
            assert pool.geometry == mo.geometry(bt, kind)
            assert tuple(pool.geometry.values()) == GEOMETRY[bt][:6] + (GEOMETRY[bt][6 if kind == E.MPX_STEREO else 7],)
        finally:
            pool.close()


@pytest.mark.parametrize("bt", TIMES)
def test_three_time_constants_and_the_clip_edge(pkg, bt):
    for k in (0, 1, 2):
        check_instance(pkg, bt, k)
    edge = np.concatenate([np.frombuffer(pcm.tobytes(), ">i2") for pcm, _, _ in device_run(pkg, bt)[2]])
    peaks = np.concatenate([r["audio"] for r in restatement(bt, False)[2]])
    print("%g s: instance 2 peaks at %.3f" % (bt, float(np.abs(peaks).max())))
    assert edge.min() >= -32767                                            # -32768 never
    if peaks.max() > 1.001:
        assert edge.max() == 32767
    if peaks.min() < -1.001:
        assert edge.min() == -32767
    assert float(np.abs(peaks).max()) > 1.001                              # both block times meet the clip edge (12 blocks of 1 ms do not)


@pytest.mark.parametrize("bt", TIMES)
def test_the_launches_companions_scripted_silence_and_clipped_samples(pkg, bt):
    """instances 3 and 4 ride in the same launches as 0-2 (capacity 2, five requests a call) and are held to the same rule"""
    olen = mo.geometry(bt)["olen"]
    for k in (3, 4):
        check_instance(pkg, bt, k)
    assert [st[0] for _, _, st in device_run(pkg, bt)[3]] == [olen if b in (0, 1, 2, 8) else 0 for b in range(NBLOCKS)]


@pytest.mark.parametrize("bt", TIMES)
def test_rds_pools_pack_the_57_kHz_slave(pkg, bt):
    src = {k: mo.signal(RDS_BLOCKS, bt, 10 + k, a, rds=True) for k, a in enumerate((0.2, 0.9))}
    got = run_pool(pkg, bt, CAP, src, {0: None, 1: (0.0, 1.0)}, kind=mo.RDS)      # (the parameters are ignored)
    for k in src:
        ref, twin = (mo.run(src[k], bt, kind=mo.RDS, f32=f) for f in (False, True))
        assert all(r["audio"].any() for r in ref)
        check(ref, twin, got[k], "%g s RDS instance %d" % (bt, k))
        assert all(st == (0, 0.0, 0.0) for _, _, st in got[k])
