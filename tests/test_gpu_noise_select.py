"""noise_est's rank selection on the device, branch by branch.

The other noise tests feed Gaussian noise through the forward transform: such a window has 50 to 90 values in the quantile's binade
and takes the two-register path of the compacted search, every time.  Here crafted spectra (tests/noise_window_cases.py) are written
straight into a spectrum slot, the bank is executed on that slot without a forward transform, and the estimate is compared with
the restatement of estimate_noise() (oracle/chz_oracle.c, pinned to src/radio.c by tests/test_oracle_vs_reference.py) on the very
same spectrum: rtol 1e-12, the figure of every noise test -- the order of the final double sum is all that may differ.  Which branch a
window takes is said by the classifier of noise_window_cases.py from counts alone (tests/test_noise_window_cases.py checks the
plans without a device); each test asserts from it that its inputs reach what it is there for BEFORE it compares anything.

  branches   one-, two- and four-register compaction, the full-width loop, the next order statistic beyond the binade, duplicates at
             the quantile, exponent 0 (zeros and subnormals), frac == 0 (COMPLEX master only: a REAL master's window always has all
             its entries, and no bank size is 1 modulo 10), in windows of 1000, 1200 and 1920 entries (noise_est<16>, <32> with
             much and with little padding), from the spectrum and from the energy image, on both master kinds; neighbouring
             wavefronts of a workgroup in different branches; a range launch from an odd channel equal to the whole-bank launch
  lanes      the binade's values in one lane, in one row of 16 lanes, in two rows, across a row boundary; the next order statistic
             alone in one lane: what the DPP reductions and the cross-row carry of the scan must get right
  seam       windows of 1, 2, 11, 63, 64, 65, 501, 1000 entries before the seam of a COMPLEX master, and windows that wrap
  guess      the binade guessed from the channel's last block: none, right, wrong, and windows at both edges of the test a guess
             has to pass -- bit-identical with the guess switched off
  energy     every case above gives the same bits from the energy image as from the spectrum

Seam-truncated windows rest on the restatement alone (noise_window_cases.py says why).  The CPU twin is
tests/test_noise_select_emulated.py."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

import noise_window_cases as nw
import oracle_lib as ol
from conftest import load_pkg

pytestmark = pytest.mark.gpu

RTOL = 1e-12
BANK_IDS = ["P%d" % P for P, _ in nw.BANKS]
GUESS_BANKS = nw.BANKS[:2]                      # noise_est<16> and <32>


@pytest.fixture(scope="module")
def pkg():
    p = load_pkg()
    if p.engine.lib().chz_device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests cannot run (there is no CPU fallback)")
    ol.build()
    assert (nw.REAL, nw.COMPLEX) == (ol.REAL, ol.COMPLEX)
    return p


def on_emulator():
    return os.environ.get("CHZ_ALLOW_EMULATED_ENGINE") == "1"


@contextlib.contextmanager
def options(**env):
    """engine options are read from the environment when an engine is created"""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


_hip = None


def inject(eng, slot, spectrum):
    """a spectrum in bin order into the pitched storage of a slot (on the CPU build of the engine device memory is host memory)"""
    global _hip
    na, pitch, off = eng.spec_layout
    k = np.arange(eng.bins)
    assert spectrum.shape == (eng.bins,)
    dev = np.zeros(eng.spec_elems, np.complex64)
    dev[(k // na) * pitch + off + k % na] = spectrum
    if on_emulator():
        C.memmove(eng.spectrum_ptr(slot), dev.ctypes.data, dev.nbytes)
        return
    if _hip is None:
        _hip = C.CDLL("libamdhip64.so")
        _hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert _hip.hipMemcpy(eng.spectrum_ptr(slot), dev.ctypes.data, dev.nbytes, 1) == 0      # hipMemcpyHostToDevice, complete on return


@contextlib.contextmanager
def noise_bank(pkg, in_type, P, olen, shifts, en, hint="1"):
    with options(CHZ_NOISE_ENERGY=en, CHZ_NOISE_HINT=hint):
        eng = pkg.engine.Engine(nw.ENGINE_L, nw.ENGINE_M, in_type, ring_blocks=8)
    try:
        assert eng.bins == nw.master_bins(in_type)
        nch = len(shifts)
        b = eng.bank(P, olen, nch)
        b.set_responses(0, np.ones((nch, P), np.complex64) / P); b.set_shifts(0, np.array(shifts, np.int32)); b.set_active(nch)
        b.enable_noise(nw.SAMPRATE)
        yield eng, b
    finally:
        eng.close()


def run_slot(eng, b, slot, spectrum):
    inject(eng, slot, spectrum)
    b.execute(slot)
    eng.sync()
    return b.read_noise(slot).copy()


_want, _got = {}, {}


def want_for(key, spectra, in_type, P, shifts):
    """the restatement's estimates [spectrum][channel], computed once per plan"""
    if key not in _want:
        _want[key] = np.array([[ol.estimate_noise(s, in_type, P, int(x), nw.SAMPRATE) for x in shifts] for s in spectra])
        _want[key].setflags(write=False)
    return _want[key]


def device_rows(pkg, key, spectra, in_type, P, olen, shifts, en, hint="1", ranged=False):
    """[spectrum][channel] from one bank that sees the spectra one after another, rotating through the slots; once per (plan, options).
    ranged: one more row -- the first spectrum again on a slot that last held the LAST one's estimates, only channels 3 .. nch - 2
    launched (execute_range from an odd channel)."""
    key = key + (en, hint)
    if key not in _got:
        with noise_bank(pkg, in_type, P, olen, shifts, en, hint) as (eng, b):
            rows = [run_slot(eng, b, i % 4, s) for i, s in enumerate(spectra)]
            if ranged:
                slot = len(spectra) % 4
                last = run_slot(eng, b, slot, spectra[-1])
                np.testing.assert_array_equal(last, rows[-1])
                inject(eng, slot, spectra[0])
                b.execute_range(slot, 3, len(shifts) - 4)
                eng.sync()
                rows.append(b.read_noise(slot).copy())
        _got[key] = np.stack(rows)
        _got[key].setflags(write=False)
    return _got[key]


def compare(got, want, what):
    """rtol 1e-12, atol 0; prints the worst measured / allowed"""
    assert got.shape == want.shape and np.all(np.isfinite(got))
    zero = want == 0
    assert np.array_equal(got[zero], want[zero]), what
    ratio = np.abs(got[~zero] - want[~zero]) / (RTOL * np.abs(want[~zero]))
    worst = float(ratio.max()) if ratio.size else 0.0
    print("%s: %d windows, worst measured / allowed %.3g" % (what, got.size, worst))
    assert worst <= 1.0, what
    return worst


def coverage(classes):
    got = {c["branch"] for c in classes}
    got |= {k for k in ("next_beyond", "duplicate") for c in classes if c[k]}
    got |= {"exponent0" for c in classes if c["exponent"] == 0}
    got |= {"frac0" if c["frac0"] else "frac" for c in classes}
    return got


def region_case(kind, master, P):
    in_type = nw.MASTERS[master]
    parts, shifts = (nw.branch_plan if kind == "branch" else nw.lane_plan)(in_type, P)
    return in_type, parts, shifts, [s for s, _ in parts]


@pytest.mark.parametrize("en", ["0", "1"], ids=["spectrum", "energy"])
@pytest.mark.parametrize("P,olen", nw.BANKS, ids=BANK_IDS)
@pytest.mark.parametrize("master", list(nw.MASTERS))
def test_every_branch_in_every_instantiation(pkg, master, P, olen, en):
    in_type, parts, shifts, spectra = region_case("branch", master, P)
    nch = len(shifts)
    assert nch % 4 != 0
    # the inputs first: together the channels take every branch
    classes = [nw.classify(s, in_type, P, x) for s in spectra for x in shifts]
    need = {"le64", "le128", "le256", "full", "next_beyond", "duplicate", "exponent0", "frac"} | ({"frac0"} if in_type == nw.COMPLEX else set())
    assert need <= coverage(classes), need - coverage(classes)
    for spec, regions in parts:                                 # ... and neighbours in a workgroup take different ones
        firsts = [nw.classify(spec, in_type, P, s[0])["branch"] for _, s in regions]
        assert len(regions) < 4 or len(set(firsts[:4])) >= 3
    want = want_for(("branch", master, P), spectra, in_type, P, shifts)
    got = device_rows(pkg, ("branch", master, P), spectra, in_type, P, olen, shifts, en, ranged=True)
    compare(got[:len(spectra)], want, "branches %s P=%d energy=%s" % (master, P, en))
    for i, (spec, regions) in enumerate(parts):
        for name, s in regions:
            if name == "mostly_zero":
                assert got[i][shifts.index(s[0])] == 0.0
    # the range launch: its channels bit for bit what the whole-bank launch gave them, the others untouched
    ranged, whole_first, whole_last = got[-1], got[0], got[len(spectra) - 1]
    np.testing.assert_array_equal(ranged[3:nch - 1], whole_first[3:nch - 1])
    np.testing.assert_array_equal(ranged[[0, 1, 2, nch - 1]], whole_last[[0, 1, 2, nch - 1]])


@pytest.mark.parametrize("en", ["0", "1"], ids=["spectrum", "energy"])
@pytest.mark.parametrize("P,olen", nw.BANKS, ids=BANK_IDS)
@pytest.mark.parametrize("master", list(nw.MASTERS))
def test_binade_values_in_chosen_lanes(pkg, master, P, olen, en):
    in_type, parts, shifts, spectra = region_case("lane", master, P)
    seen = set()
    for spec, regions in parts:
        for name, (s,) in regions:
            k = nw.classify(spec, in_type, P, s)
            lanes = nw.expected_lanes(name)
            assert k["branch"] == "le64" and (k["next_beyond"] if lanes is None else set(np.nonzero(k["lane_counts"])[0]) <= set(lanes)), name
            seen.add(name)
    assert seen == {name for name, _ in nw.LANE_CASES}
    want = want_for(("lane", master, P), spectra, in_type, P, shifts)
    got = device_rows(pkg, ("lane", master, P), spectra, in_type, P, olen, shifts, en)
    assert np.all(want > 0)
    compare(got, want, "lanes %s P=%d energy=%s" % (master, P, en))


def seam_case(P):
    plan = nw.seam_plan(P)
    shifts = [s for _, s, _ in plan[0][1]]
    assert all([s for _, s, _ in w] == shifts for _, w in plan)
    return plan, shifts, [s for s, _ in plan]


@pytest.mark.parametrize("en", ["0", "1"], ids=["spectrum", "energy"])
@pytest.mark.parametrize("P,olen", nw.BANKS, ids=BANK_IDS)
def test_windows_at_the_seam_of_a_complex_master(pkg, P, olen, en):
    plan, shifts, spectra = seam_case(P)
    assert len(shifts) % 4 != 0
    ns = [nw.classify(spectra[0], nw.COMPLEX, P, s)["n"] for s in shifts]
    assert set(nw.SEAM_N) <= set(ns) and sum(n < 64 for n in ns) >= 4
    fr = [nw.classify(spectra[0], nw.COMPLEX, P, s)["frac0"] for s in shifts]
    assert any(fr) and not all(fr)
    want = want_for(("seam", P), spectra, nw.COMPLEX, P, shifts)
    got = device_rows(pkg, ("seam", P), spectra, nw.COMPLEX, P, olen, shifts, en)
    assert np.all(want > 0)
    compare(got, want, "seam P=%d energy=%s" % (P, en))


@pytest.mark.parametrize("en", ["0", "1"], ids=["spectrum", "energy"])
@pytest.mark.parametrize("P,olen", GUESS_BANKS, ids=BANK_IDS[:2])
@pytest.mark.parametrize("master", list(nw.MASTERS))
def test_guessed_binade_is_never_a_result(pkg, master, P, olen, en):
    in_type = nw.MASTERS[master]
    spectra, shifts, names = nw.guess_plan(in_type, P)
    assert len(spectra) >= 8 and len(shifts) % 4 != 0
    kinds = set()
    for b, row in enumerate(nw.guess_events(spectra, in_type, P, shifts)):
        for c, (hint, c0, c1, qi, exponent) in enumerate(row):
            if hint is None:
                kinds.add("none")
                continue
            right = c0 <= qi < c1
            kinds.add(("right" if right else "wrong") + ("_at_exponent0" if right and exponent == 0 else ""))
            if hint == nw.GUESS_BASE and (c0 in (qi, qi + 1) or c1 in (qi, qi + 1)):
                kinds.add("c0=qi" if c0 == qi else "c0=qi+1" if c0 == qi + 1 else "c1=qi+1" if c1 == qi + 1 else "c1=qi")
    assert kinds >= {"none", "right", "wrong", "right_at_exponent0", "c0=qi", "c0=qi+1", "c1=qi+1", "c1=qi"}, kinds
    want = want_for(("guess", master, P), spectra, in_type, P, shifts)
    on = device_rows(pkg, ("guess", master, P), spectra, in_type, P, olen, shifts, en, "1")
    off = device_rows(pkg, ("guess", master, P), spectra, in_type, P, olen, shifts, en, "0")
    compare(on, want, "guess %s P=%d energy=%s" % (master, P, en))
    for b, row in enumerate(names):
        for c, name in enumerate(row):
            assert (on[b][c] == 0.0) == (name == "mostly_zero"), (b, c, name)
    np.testing.assert_array_equal(on, off)


ALL_PLANS = ([("branch", m, P, olen) for m in nw.MASTERS for P, olen in nw.BANKS] + [("lane", m, P, olen) for m in nw.MASTERS for P, olen in nw.BANKS] +
             [("seam", "complex", P, olen) for P, olen in nw.BANKS] + [("guess", m, P, olen) for m in nw.MASTERS for P, olen in GUESS_BANKS])


@pytest.mark.parametrize("kind,master,P,olen", ALL_PLANS, ids=["%s-%s-P%d" % p[:3] for p in ALL_PLANS])
def test_energy_image_gives_the_spectrum_paths_bits(pkg, kind, master, P, olen):
    """spec_energy takes |X|^2 once per bin with the same three roundings as the windows that read the spectrum themselves: every
    case of this file, bit for bit (the runs are those of the tests above, made once)"""
    in_type = nw.MASTERS[master]
    if kind == "seam":
        _, shifts, spectra = seam_case(P)
        key = ("seam", P)
    elif kind == "guess":
        spectra, shifts, _ = nw.guess_plan(in_type, P)
        key = ("guess", master, P)
    else:
        _, _, shifts, spectra = region_case(kind, master, P)
        key = (kind, master, P)
    rows = [device_rows(pkg, key, spectra, in_type, P, olen, shifts, en, ranged=kind == "branch") for en in ("0", "1")]
    assert rows[0].shape[1] == len(shifts) and np.any(rows[0] > 0)
    np.testing.assert_array_equal(rows[0], rows[1])
    print("energy image %s %s P=%d: %d windows bit-identical" % (kind, master, P, rows[0].size))
