"""The inputs of tests/test_gpu_noise_select.py are what their names say: every window that file injects (tests/noise_window_cases.py
builds them from fixed seeds) is classified here -- window placement and counting restated in numpy, nothing taken from the kernel --
and must land in the branch of noise_est it is named after; the restatement's estimate (oracle/chz_oracle.c, pinned to radio.c by
tests/test_oracle_vs_reference.py) must be finite and positive for it, or exactly 0 where most of the window is exact zeros.
Windows that stop at the seam of a COMPLEX master rest on the restatement alone: the reference reads entries nobody wrote there
(noise_window_cases.py has the lines)."""
import numpy as np
import pytest

import noise_window_cases as nw
import oracle_lib as ol

PARAMS = [(m, P) for m in nw.MASTERS for P, _ in nw.BANKS]
IDS = ["%s-P%d" % p for p in PARAMS]

# what each construction promises: branch (None: whichever), then the classifier's flags that must hold
PROMISE = {"le64": ("le64", {}), "le128": ("le128", {}), "le256": ("le256", {}), "full": ("full", {}),
           "all_equal": ("full", {"duplicate": True}), "two_values": ("full", {"duplicate": True}),
           "mostly_zero": ("full", {"duplicate": True, "exponent": 0}),
           "next_adjacent": ("le64", {"next_beyond": True}), "next_far": ("le64", {"next_beyond": True}),
           "binade_edge": (None, {"next_beyond": True, "exponent": 127, "below": 0}),
           "duplicate_at_q": ("le64", {"duplicate": True, "next_beyond": False}),
           "duplicate_pair": ("le64", {"duplicate": True, "next_beyond": False}), "wide_range": (None, {}),
           "huge": (None, {}), "subnormal": ("full", {"exponent": 0}), "subnormal_few": ("compact", {"exponent": 0})}


@pytest.fixture(scope="module")
def oracle(oracle_built):
    assert (nw.REAL, nw.COMPLEX) == (ol.REAL, ol.COMPLEX)
    return oracle_built


def estimate(spec, in_type, P, shift):
    return ol.estimate_noise(spec, in_type, P, int(shift), nw.SAMPRATE)


def covered(classes):
    """the branches and flags a set of classified windows hits"""
    got = {c["branch"] for c in classes}
    got |= {k for k in ("next_beyond", "duplicate") for c in classes if c[k]}
    got |= {"exponent0" for c in classes if c["exponent"] == 0}
    got |= {"frac0" if c["frac0"] else "frac" for c in classes}
    return got


@pytest.mark.parametrize("master,P", PARAMS, ids=IDS)
def test_branch_cases_land_in_their_branches(oracle, master, P):
    in_type = nw.MASTERS[master]
    parts, shifts = nw.branch_plan(in_type, P)
    assert len(shifts) % 4 != 0
    seen, classes = set(), []
    for spec, regions in parts:
        assert spec.shape == (nw.master_bins(in_type),) and np.all(np.isfinite(spec.view(np.float32)))
        for name, region_shifts in regions:
            k = nw.classify(spec, in_type, P, region_shifts[0])            # the constructed window itself
            want_branch, flags = PROMISE[name]
            assert k["n"] == nw.window_size(P) and (want_branch is None or k["branch"] == want_branch or (want_branch == "compact" and k["branch"] in ("le128", "le256"))), (name, k)
            for f, v in flags.items():
                assert k[f] == v, (name, f, k)
            if name == "duplicate_pair":
                order = np.sort(nw.window_energies(spec, in_type, P, region_shifts[0]))
                assert order[k["qi"] - 1] < order[k["qi"]] == order[k["qi"] + 1] < order[k["qi"] + 2]
            if name == "huge":
                assert k["exponent"] in (253, 254)
            if name == "subnormal":
                e = nw.window_energies(spec, in_type, P, region_shifts[0])
                assert np.sum(e == 0) >= 5 and np.sum((e > 0) & (e < np.finfo(np.float32).tiny)) > k["qi"]      # the quantile is a subnormal
            got = estimate(spec, in_type, P, region_shifts[0])
            assert np.isfinite(got) and (got == 0.0 if name == "mostly_zero" else got > 0), (name, got)
            seen.add(name)
        for s in shifts:
            classes.append(nw.classify(spec, in_type, P, s))
            assert np.isfinite(estimate(spec, in_type, P, s))
    assert seen == set(PROMISE)
    need = {"le64", "le128", "le256", "full", "next_beyond", "duplicate", "exponent0", "frac"} | ({"frac0"} if in_type == nw.COMPLEX else set())
    assert need <= covered(classes), need - covered(classes)
    assert any(c["n"] < 64 for c in classes) == (in_type == nw.COMPLEX)


@pytest.mark.parametrize("master,P", PARAMS, ids=IDS)
def test_lane_cases_sit_in_their_lanes(oracle, master, P):
    in_type = nw.MASTERS[master]
    parts, shifts = nw.lane_plan(in_type, P)
    assert len(shifts) % 4 != 0
    seen = set()
    for spec, regions in parts:
        for name, (shift,) in regions:
            k = nw.classify(spec, in_type, P, shift)
            lanes = nw.expected_lanes(name)
            assert k["branch"] == "le64" and k["exponent"] == 127, (name, k)
            if lanes is not None:
                assert set(np.nonzero(k["lane_counts"])[0]) <= set(lanes) and k["total"] >= min(15, len(lanes)) and not k["next_beyond"], (name, k)
                if len(lanes) > 2:
                    assert len(set(k["lane_counts"][lanes])) > 1                # the rows' counts differ
            else:
                assert k["next_beyond"], (name, k)
                e = nw.window_energies(spec, in_type, P, shift)
                at = np.nonzero((e >= 2.0) & (e < 4.0))[0]
                assert at.size == 1 and at[0] % 64 == int(name.rsplit("_", 1)[1]) and np.sum(e >= 4.0) == k["n"] - k["qi"] - 2
            got = estimate(spec, in_type, P, shift)
            assert np.isfinite(got) and got > 0
            seen.add(name)
    assert seen == {name for name, _ in nw.LANE_CASES}


@pytest.mark.parametrize("P", [P for P, _ in nw.BANKS])
def test_seam_cases_stop_where_they_say(oracle, P):
    N = nw.master_bins(nw.COMPLEX)
    for spec, windows in nw.seam_plan(P):
        ns = set()
        for label, shift, n in windows:
            mbin, got_n = nw.placement(N, nw.COMPLEX, P, shift)
            assert got_n == n, (label, shift)
            if label.startswith("stop"):
                assert mbin + n == N // 2
            if label.startswith("wrap"):
                assert mbin + n > N                                          # from the last bin on to bin 0
            k = nw.classify(spec, nw.COMPLEX, P, shift)
            assert k["frac0"] == (n % 10 == 1)
            got = estimate(spec, nw.COMPLEX, P, shift)
            assert np.isfinite(got) and got > 0, (label, got)
            ns.add(n)
        assert set(nw.SEAM_N) <= ns and nw.window_size(P) in ns


@pytest.mark.parametrize("master,P", [(m, P) for m in nw.MASTERS for P in (300, 1200)], ids=lambda v: str(v))
def test_guess_script_has_right_wrong_and_boundary_guesses(oracle, master, P):
    in_type = nw.MASTERS[master]
    spectra, shifts, names = nw.guess_plan(in_type, P)
    assert len(spectra) >= 8 and len(shifts) % 4 != 0
    events = nw.guess_events(spectra, in_type, P, shifts)
    kinds = set()
    for b, row in enumerate(events):
        for c, (hint, c0, c1, qi, exponent) in enumerate(row):
            name = names[b][c]
            got = estimate(spectra[b], in_type, P, shifts[c])
            assert np.isfinite(got) and (got == 0.0 if name == "mostly_zero" else got > 0), (b, c, name)
            if hint is None:
                kinds.add("none")
                continue
            right = c0 <= qi < c1
            assert right == (hint == exponent)
            kinds.add("right" if right else "wrong")
            if right and exponent == 0:
                kinds.add("right_at_exponent0")
            if name in ("A", "up"):
                assert exponent == nw.GUESS_BASE + (name == "up")
            if name.startswith("c") and hint == nw.GUESS_BASE:                  # the boundary windows behind an "A"
                want = {"c0_eq_qi": (c0 == qi and c1 > qi + 1, True), "c1_eq_qi1": (c1 == qi + 1 and c0 < qi, True),
                        "c0_eq_qi1": (c0 == qi + 1, False), "c1_eq_qi": (c1 == qi, False)}[name]
                assert want[0] and right == want[1], (name, c0, c1, qi)
                kinds.add(name)
            if name == "A" and b > 0 and names[b - 1][c] == "A":
                assert right                                                     # the same spectrum twice
    assert kinds >= {"none", "right", "wrong", "right_at_exponent0", "c0_eq_qi", "c1_eq_qi1", "c0_eq_qi1", "c1_eq_qi"}, kinds
