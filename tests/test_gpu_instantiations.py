"""Every compiled forward and channel kernel instantiation on the device.

The parity tests are deep where the benchmark lives (N = 3,240,000, P = 300 / 600); this module is wide instead: it walks the template
matrix the kernels are compiled into, at the smallest shapes that reach each instantiation.

  * forward: each (R1,R2) pair of CHZ_FWD_MENU as fwd_first_real, as fwd_cols on a COMPLEX master's first axis, as fwd_cols on axis b and
    as fwd_rows, through the explicit plans Ax16x16, 16xAx16 and 16x16xA (N = 256 A); the plan string proves which instantiation ran.
    144 is in the menu twice: (12,12) serves axes a and b, (9,16) axis c, so (9,16) is never a first or column axis and (12,12) never
    a row axis -- 26 reachable pairs in each position.
  * REAL masters whose first pass wants more than the 64 KB of dynamic LDS a kernel gets by default.
  * channels: chan_ifft<R1,R2,EPI> at the 14 sizes of CHZ_CHAN_MENU with the ISB / beam epilogue (EPI 2) and the fine-tuning / power
    epilogue (EPI 1), and chan_c2r<R1,R2> at the same sizes (EPI 0 at all 14: test_gpu_parity.py::test_channel_sizes_random_spectrum).

Oracle calls and tolerances are those of the tests in tests/test_gpu_parity.py each case is modelled on.
"""
import numpy as np
import pytest

import oracle_lib as ol
from conftest import load_pkg
from instantiation_cases import CHAN_SIZES, FWD_LENGTHS, FWD_PAIRS, lds1_bytes, parse_plan, sweep_LM, sweep_plans
from test_gpu_parity import SPEC_REL, _ulp_close, check_channel, noise_floor, rel

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    p = load_pkg()
    if p.engine.lib().chz_device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests cannot run (there is no CPU fallback)")
    ol.build()
    return p


# ------------------------------------------------------------------------------
# forward transform
# ------------------------------------------------------------------------------
def _forward_three_blocks(pkg, L, M, in_type, plan, seed):
    """test_forward_matches_oracle's comparison: three blocks, so that the history and the ring offset move.  Returns the plan string."""
    rng = np.random.default_rng(seed)
    eng = pkg.engine.Engine(L, M, in_type, plan=plan)
    st = ol.Stream(L, M, in_type)
    try:
        for job in range(3):
            if in_type == ol.REAL:
                x = rng.standard_normal(L).astype(np.float32)
            else:
                x = (rng.standard_normal(L) + 1j * rng.standard_normal(L)).astype(np.complex64)
            eng.write(x)
            eng.forward(job)
            got = eng.spectrum(job % 4)
            want = st.push(x, f64=True)
            assert rel(got, want) <= SPEC_REL, (job, eng.plan)
            # element-wise: no bin may be off by more than a few float32 ulps of the spectrum scale
            assert np.abs(got - want).max() <= 2e-5 * np.sqrt(np.mean(np.abs(want) ** 2)) * np.sqrt(np.log2(eng.N)), (job, eng.plan)
        return eng.plan
    finally:
        eng.close()


def test_the_sweep_reaches_every_pair_in_every_position():
    # sweep_plans(A): A as axis a (REAL, COMPLEX), as axis b (REAL, COMPLEX), as axis c (REAL, COMPLEX)
    cases = [sweep_plans(A) for A in FWD_LENGTHS]
    assert sum(len(c) for c in cases) == 156
    first_real = {c[0][2][0] for c in cases}; first_cplx = {c[1][2][0] for c in cases}
    assert all(c[0][1] == ol.REAL and c[1][1] == ol.COMPLEX for c in cases)
    cols_b = {c[k][2][1] for c in cases for k in (2, 3)}
    rows = {c[k][2][2] for c in cases for k in (4, 5)}
    assert first_real == first_cplx == cols_b == set(FWD_PAIRS) - {(9, 16)} and len(cols_b) == 26
    assert rows == set(FWD_PAIRS) - {(12, 12)} and len(rows) == 26


@pytest.mark.parametrize("A", FWD_LENGTHS)
def test_forward_instantiations(pkg, A):
    N = 256 * A
    L, M = sweep_LM(N)
    assert L % 2 == 0 and M % 2 == 1 and L + M - 1 == N
    for plan, in_type, want in sweep_plans(A):
        desc = _forward_three_blocks(pkg, L, M, in_type, plan, seed=A + in_type)
        p = parse_plan(desc)
        assert p["axes"] == tuple(int(v) for v in plan.split("x")) and p["real"] == (in_type == ol.REAL), desc
        assert p["radices"] == want, desc                    # the instantiations that ran


@pytest.mark.parametrize("N,lds1", [(11250, 90240),        # 225x50 with T1 = 25: a single workgroup on axis a
                                    (48000, 79200),         # 240x200: a 1.92 MS/s real input at 20 ms blocks, overlap 5
                                    (65536, 67584),         # 256x256
                                    (160000, 128640)])      # 400x400: the largest first pass of any automatic plan up to 4,000,000 points
def test_real_masters_with_a_first_pass_beyond_64_kb_of_lds(pkg, N, lds1):
    # fwd_first_real holds two regions of Na*T1 points; beyond 64 KB the launch needs the kernel's dynamic-LDS limit raised (the engine
    # does so when it creates the master).  Three of the sweep's plans are of this kind too: 256x16x16, 320x16x16 and 400x16x16 REAL
    # (67,584 / 83,968 / 104,960 bytes).
    L, M = sweep_LM(N)
    desc = _forward_three_blocks(pkg, L, M, ol.REAL, "", seed=N)
    assert lds1_bytes(desc) == lds1 and lds1 > 64 * 1024, desc


def test_sweep_plans_beyond_64_kb_of_lds():
    # (plan strings only: the transforms themselves run in test_forward_instantiations)
    big = {}
    for A in FWD_LENGTHS:
        for plan, in_type, want in sweep_plans(A):
            a, b, c = (int(v) for v in plan.split("x"))
            t1 = 16                                              # 128 packed / 256 complex columns: the planner's aligned 16-column tile
            lds = 8 * ((2 if in_type == ol.REAL else 1) * a * t1 + want[0][0] * ((t1 - want[0][1] * t1) % 32))
            if lds > 64 * 1024:
                big[(plan, in_type)] = lds
    assert big == {("256x16x16", ol.REAL): 67584, ("320x16x16", ol.REAL): 83968, ("400x16x16", ol.REAL): 104960}


# ------------------------------------------------------------------------------
# channels: 14 sizes x {ISB, tuned + power, REAL output, beam}
# ------------------------------------------------------------------------------
RL, RM = 25920, 6481           # the REAL master: N = 32400, olen = 0.8 P
CL, CM = 11520, 2881           # the COMPLEX master of the beam slaves: N = 14400, olen = 0.8 P


def _shifts(P, B, rng, edge, empty):
    """0, +-1, +-P/2, the last bin, one whose gather runs past the band edge (partly filled), the empty gather, a few seeded random ones."""
    return [0, 1, -1, P // 2, -(P // 2), B - 1, edge, empty] + [int(s) for s in rng.integers(-B + 1, B, 4)]


@pytest.mark.parametrize("P", CHAN_SIZES)
def test_isb_slaves_every_size(pkg, P):
    # chan_ifft<R1,R2,2> as test_isb_slaves runs it at P = 300
    L, M, olen = RL, RM, P * 4 // 5
    fa = pkg.filterapi
    rng = np.random.default_rng(77 + P)
    master = fa.create_filter_input(L, M, fa.REAL)
    st = ol.Stream(L, M, ol.REAL)
    B = master.bins
    shifts = _shifts(P, B, rng, edge=B + P // 4, empty=B + P)
    empty = shifts.index(B + P)
    slaves = [fa.create_filter_output(master, olen, fa.COMPLEX) for _ in shifts]
    try:
        for s in slaves:
            assert s is not None and s.points == P
            assert fa.set_filter(s, -0.45, 0.45, 9.0) == 0
        for blk in range(3):
            x = rng.standard_normal(L).astype(np.float32)
            assert fa.write_rfilter(master, x) == 1
            spec64 = st.push(x, f64=True)
            spec32 = spec64.astype(np.complex64)
            for i, (s, sh) in enumerate(zip(slaves, shifts)):
                s.isb = (i != 4) and (blk != 1 or i != 0)          # flags flip between blocks; one channel stays plain
                assert fa.execute_filter_output(s, sh) == 0
                want = ol.channel(spec32, ol.REAL, P, olen, sh, s.response, isb=bool(s.isb))
                assert np.linalg.norm(s.output - want) <= 1e-5 * np.linalg.norm(want) + noise_floor(spec64, s.response) * np.sqrt(olen) * 2, (blk, i, sh)
            assert not slaves[empty].output.any() and np.abs(slaves[0].output).max() > 0
    finally:
        fa.delete_filter_input(master)


@pytest.mark.parametrize("P", CHAN_SIZES)
def test_real_output_slaves_every_size(pkg, P):
    # chan_c2r<R1,R2> as test_real_output_slaves runs it (every menu size is even)
    L, M, olen = RL, RM, P * 4 // 5
    fa = pkg.filterapi
    rng = np.random.default_rng(P + L)
    master = fa.create_filter_input(L, M, fa.REAL)
    N = L + M - 1
    B = N // 2 + 1
    st = ol.Stream(L, M, ol.REAL)
    shifts = _shifts(P, B, rng, edge=B - P // 4, empty=B + P)        # (a REAL-output slave reads upward from its shift only)
    bands = [(0.0, 0.31), (0.02, 0.4), (0.1, 0.1), (0.0, 0.45), (0.2, 0.05), (0.0, 0.5)]
    slaves = []
    try:
        for i, sh in enumerate(shifts):
            lo, hi = bands[i % len(bands)]
            s = fa.create_filter_output(master, olen, fa.REAL)
            assert s is not None and s.bins == P // 2 + 1 and s.points == P
            assert fa.set_filter(s, lo, hi, 5.0) == 0
            ref = ol.set_filter(P, olen, N, True, lo, hi, 5.0, out_type=ol.REAL)
            assert np.abs(s.response - ref).max() <= 3e-7 * np.abs(ref).max()
            slaves.append(s)
        for blk in range(3):
            x = rng.standard_normal(L).astype(np.float32)
            assert fa.write_rfilter(master, x) == 1
            spec = st.push(x)
            seen = 0
            for s, sh in zip(slaves, shifts):
                assert fa.execute_filter_output(s, sh) == 0
                assert s.output.dtype == np.float32 and s.output.shape == (olen,)
                want = ol.channel(spec, ol.REAL, P, olen, sh, s.response, out_type=ol.REAL)
                nrm = float(np.linalg.norm(want))
                assert nrm > 0 or sh < 0 or sh == B + P, sh         # (most gathers below the band are empty too)
                if nrm == 0:
                    assert not s.output.any()
                else:
                    seen += 1
                    assert np.linalg.norm(s.output - want) <= 1e-5 * nrm + 2e-8 * float(np.abs(spec).max()) * float(np.linalg.norm(s.response)) * np.sqrt(olen), (blk, sh)
            assert seen >= 6 and not slaves[shifts.index(B + P)].output.any()
    finally:
        fa.delete_filter_input(master)


@pytest.mark.parametrize("P", CHAN_SIZES)
def test_beam_slaves_every_size(pkg, P):
    # chan_ifft<R1,R2,2> on a COMPLEX master as test_beam_slaves runs it at P = 300
    L, M, olen = CL, CM, P * 4 // 5
    fa = pkg.filterapi
    rng = np.random.default_rng(78 + P)
    master = fa.create_filter_input(L, M, fa.COMPLEX)
    st = ol.Stream(L, M, ol.COMPLEX)
    N = L + M - 1
    H = N // 2
    empty_shift = -(H + P)
    shifts = [0, 1, -1, P // 2, -(P // 2), H - 1, -H + P // 4, empty_shift] + [int(s) for s in rng.integers(-H + 1, H, 4)]
    kinds = [(1.0, 0.0), (0.0, 1.0), (0.7 + 0.2j, -0.3 + 0.6j), None]
    weights = [kinds[i % 4] for i in range(len(shifts))]
    weights[7] = kinds[2]                                           # the empty gather runs the beam arithmetic too
    slaves = [fa.create_filter_output(master, olen, fa.COMPLEX) for _ in shifts]
    try:
        for s, w in zip(slaves, weights):
            assert s is not None and s.points == P
            assert fa.set_filter(s, -0.4, 0.4, 9.0) == 0
            if w is not None:
                s.beam = True
                assert fa.set_filter_weights(s, *w) == 0
        for blk in range(3):
            x = (rng.standard_normal(L) + 1j * rng.standard_normal(L)).astype(np.complex64)
            assert fa.write_cfilter(master, x) == 1
            spec = st.push(x)
            if blk == 2:
                fa.set_filter_weights(slaves[0], 0.25, -0.5j)          # weights change mid-stream
            for s, w, sh in zip(slaves, weights, shifts):
                assert fa.execute_filter_output(s, sh) == 0
                if w is None:
                    want = ol.channel(spec, ol.COMPLEX, P, olen, sh, s.response)
                else:
                    want = ol.channel_beam(spec, P, olen, sh, s.response, s.alpha, s.beta)
                assert (np.linalg.norm(want) == 0) == (sh == empty_shift), sh
                assert np.linalg.norm(s.output - want) <= 1e-5 * np.linalg.norm(want), (blk, sh)
            assert not slaves[7].output.any() and np.abs(slaves[0].output).max() > 0
    finally:
        fa.delete_filter_input(master)


@pytest.mark.parametrize("P", CHAN_SIZES)
def test_tuned_bank_every_size(pkg, P):
    """chan_ifft<R1,R2,1>: per-channel fine oscillator, block phase correction, shift-change kick and bb_power as
    test_tuned_bank_follows_downconvert checks them at P = 300, five blocks with one retune.  Its share of bit-identical samples is a
    statistic of a 240-sample block; at 16 samples a block one last-bit difference would be 6 %, so here the same shares are taken over
    all samples of the run (fixed and swept oscillators apart); the one-ulp bound holds for every sample as there."""
    L, M, fs_in, olen, nch = RL, RM, 1.296e6, P * 4 // 5, 12
    fs_out = olen / 0.02
    N = L + M - 1
    B = N // 2 + 1
    rng = np.random.default_rng(71 + P)
    f_hz = 50e3 + rng.uniform(0, 500e3, nch)
    f_hz[0] = 40.0 * 2500                      # exactly on a bin whose shift is a multiple of V: no rotation at all
    f_hz[1] = 40.0 * 2501                      # on a bin, shift % V = 1: block phase correction only
    f_hz[2] = 0.0                              # shift 0: the lower half of the gather is off the band
    f_hz[3] = -40.0                            # shift -1: read downward, conjugated
    f_hz[4] = 40.0 * (B - 1) - 7.0             # the last bin, tuned a little below it
    fixed = {7: B + P}                         # past the band edge by more than the channel: the empty gather, all zeros, power 0
    sweep = np.zeros(nch); sweep[5] = 35.0; sweep[6] = -120.0     # Hz/s
    resp = np.stack([ol.set_filter(P, olen, N, True, -0.35, 0.35, 9.0)] * nch).astype(np.complex64)
    eng = pkg.engine.Engine(L, M, ol.REAL, ring_blocks=8)
    tuned = eng.bank(P, olen, nch); plain = eng.bank(P, olen, nch)
    for b in (tuned, plain):
        b.set_responses(0, resp); b.set_active(nch)
    st = ol.Stream(L, M, ol.REAL)
    dco = [ol.Downconv(L, M, fs_out, "oracle") for _ in range(nch)]
    dcr = [ol.Downconv(L, M, fs_out, "ref") for _ in range(nch)] if ol.have_ref() else None
    dce = [ol.Downconv(L, M, fs_out, "oracle") for _ in range(nch)]       # end-to-end chain on the float64 oracle
    job0 = 0xFFFFFFF8                          # ring-aligned (multiple of 8)
    shifts = np.zeros(nch, np.int32); rems = np.zeros(nch)
    same = {False: [0, 0], True: [0, 0]}       # swept? -> [bit-identical samples, samples]
    try:
        for blk in range(5):
            job = (job0 + blk) & 0xFFFFFFFF
            if blk in (0, 3):                  # retune: everything at 0, a few channels later
                sel = range(nch) if blk == 0 else [2, 3, 6, 9]
                for ch in sel:
                    if blk:
                        f_hz[ch] += rng.uniform(-3e3, 3e3)
                    _, sh, rem = ol.compute_tuning(N, fs_in, f_hz[ch])
                    shifts[ch], rems[ch] = (fixed[ch], 0.0) if ch in fixed else (sh, rem)
                sel = np.array(list(sel))
                lo, hi = int(sel.min()), int(sel.max()) + 1
                tuned.set_tuning(job, lo, shifts[lo:hi], -rems[lo:hi] / fs_out, sweep[lo:hi] / fs_out ** 2)
                plain.set_shifts(0, shifts)
            x = rng.standard_normal(L).astype(np.float32)
            eng.write(x)
            spec64 = st.push(x, f64=True)
            eng.step(job)
            got = tuned.read_slot(job % 4); raw = plain.read_slot(job % 4)
            pw = tuned.read_power(job % 4)
            for ch in range(nch):
                # (1) the rotation itself, applied to the GPU's own un-rotated samples: float-exact
                want, wpw = dco[ch].block(raw[ch], shifts[ch], rems[ch], sweep[ch])
                worst, frac = _ulp_close(got[ch], want)
                assert worst <= 1.0, (blk, ch, worst, frac)
                acc = same[bool(sweep[ch])]; acc[0] += frac * olen; acc[1] += olen
                assert abs(pw[ch] - wpw) <= 1e-6 * wpw
                if dcr is not None:
                    want_r, rpw = dcr[ch].block(raw[ch], shifts[ch], rems[ch], sweep[ch])
                    assert _ulp_close(want_r, want)[0] <= 1.0 and abs(rpw - wpw) <= 1e-9 * wpw
                # (2) end to end against the float64 oracle chain
                ideal = ol.channel(spec64, ol.REAL, P, olen, int(shifts[ch]), resp[ch])
                ideal, ipw = dce[ch].block(ideal, shifts[ch], rems[ch], sweep[ch])
                check_channel(got[ch], ideal, noise_floor(spec64, resp[ch]))
                assert abs(pw[ch] - ipw) <= 1e-4 * ipw
            assert not got[7].any() and pw[7] == 0 and np.abs(got[0]).max() > 0
        assert same[False][0] >= 0.97 * same[False][1] and same[True][0] >= 0.85 * same[True][1], same
    finally:
        eng.close()
