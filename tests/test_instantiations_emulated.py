"""The forward template matrix on the CPU: every (R1,R2) pair of CHZ_FWD_MENU in every position it can take, through the fiber emulator
(the twin of the device sweep in tests/test_gpu_instantiations.py), and the LDS every automatic plan asks for against what a CU has."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as ol
from instantiation_cases import FWD_LENGTHS, FWD_PAIRS, first_pair, parse_plan, rows_pair, sweep_plans
from test_kernels_emulated import emu, rel          # noqa: F401  (the module's fixture: builds and binds tests/hipemu/libchz_emu.so)

LDS_CU = 160 * 1024          # bytes of LDS a workgroup can get on gfx950
LDS_DEFAULT = 64 * 1024      # beyond this a kernel has to be told (hipFuncAttributeMaxDynamicSharedMemorySize)


def _plan_lds(emu, N, in_type, spec=b""):
    emu.emu_plan_lds.argtypes = [C.c_int, C.c_int, C.c_char_p, C.c_void_p]
    out = (C.c_long * 3)()
    return tuple(out) if emu.emu_plan_lds(N, in_type, spec, out) else None


def test_menu_positions_each_pair_can_take():
    # 144 is in the menu twice: the first entry (12,12) serves axes a and b, (9,16) -- R2 a multiple of 16 -- serves axis c; so
    # (9,16) is never a first or column axis and (12,12) never a row axis.  Every other pair can take every position.
    assert len(FWD_PAIRS) == 27 and len(FWD_LENGTHS) == 26
    assert {first_pair(n) for n in FWD_LENGTHS} == set(FWD_PAIRS) - {(9, 16)}
    assert {rows_pair(n) for n in FWD_LENGTHS} == set(FWD_PAIRS) - {(12, 12)}


def test_no_plan_asks_for_more_lds_than_a_cu_has(emu):
    """Every automatic plan of a two- or three-axis product of menu lengths up to 4,000,000 points, REAL and COMPLEX: no pass wants
    more than the 160 KB of a CU (finish_fwd_plan refuses such a geometry, so the planner cannot pick one and an explicit plan fails at
    create time).  More than the default 64 KB is legal -- the engine raises the kernel's limit when it creates the master -- and only the
    first pass of a REAL master (two regions of Na*T1 points) gets there."""
    lens = FWD_LENGTHS
    sizes = {a * b for a in lens for b in lens} | {a * b * c for a in lens for b in lens for c in lens}
    sizes = sorted(n for n in sizes if n <= 4_000_000)
    big = {}
    nplans = 0
    for n in sizes:
        for in_type in (ol.REAL, ol.COMPLEX):
            lds = _plan_lds(emu, n, in_type)
            if lds is None:
                assert in_type == ol.REAL and n % 2, (n, in_type)          # a product of menu axes always has a plan, odd REAL lengths aside
                continue
            nplans += 1
            assert max(lds) <= LDS_CU, (n, in_type, lds)
            if max(lds) > LDS_DEFAULT:
                assert in_type == ol.REAL and lds[1] <= LDS_DEFAULT and lds[2] <= LDS_DEFAULT, (n, in_type, lds)
                big[n] = lds[0]
    assert nplans > 1500
    # the masters tests/test_gpu_instantiations.py runs on the device, and the largest of all
    for n, want in ((11250, 90240), (48000, 79200), (64000, 104960), (65536, 67584), (96000, 96480), (160000, 128640)):
        assert big.get(n) == want, (n, big.get(n))
    assert max(big.values()) == 128640, big
    # an explicit geometry that cannot fit is no plan at all: 400 x 32 packed columns, twice, are 200 KB
    assert _plan_lds(emu, 102400, ol.REAL, b"400x16x16:32") is None
    assert _plan_lds(emu, 102400, ol.REAL, b"400x16x16")[0] == 104960          # T1 = 16: the sweep's largest


@pytest.mark.parametrize("A", FWD_LENGTHS)
def test_forward_sweep_on_the_emulator(emu, A):
    """Length A as first, middle and last axis between two 16-point axes, REAL and COMPLEX input (N = 256 A): the six plans against the
    float64 oracle, and the plan string names the (R1,R2) instantiations that ran."""
    N = 256 * A
    rng = np.random.default_rng(A)
    for spec, in_type, want in sweep_plans(A):
        per = 1 if in_type == ol.REAL else 2
        ring_len = (N + 2 * int(rng.integers(10, 600))) * per
        start = 2 * int(rng.integers(0, ring_len // 2))            # most windows straddle the end of the ring
        ring = rng.standard_normal(ring_len).astype(np.float32)
        win = ring[(start + np.arange(N * per)) % ring_len]
        out = np.zeros(N // 2 + 1 if in_type == ol.REAL else N, np.complex64)
        desc = C.create_string_buffer(256)
        assert emu.emu_forward(ring.ctypes.data, ring_len, start, N, in_type, spec.encode(), out.ctypes.data, desc, 256, None, None, 0, 0.0) == 0, (spec, in_type)
        p = parse_plan(desc.value)
        assert p["radices"] == want and p["real"] == (in_type == ol.REAL), desc.value
        ref = ol.forward(win if in_type == ol.REAL else win.view(np.complex64), in_type, f64=True)
        assert rel(out, ref) < 5e-7, desc.value
