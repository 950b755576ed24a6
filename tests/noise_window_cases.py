"""Crafted noise windows for noise_est's rank selection, and a classifier that says which of the kernel's branches a window takes.

Pure numpy, no engine: tests/test_noise_window_cases.py checks here that every case is what its name says, tests/test_gpu_noise_select.py
then runs the cases on the device (and tests/test_noise_select_emulated.py the same file on the CPU build).

THE CLASSIFIER restates only where estimate_noise() (src/radio.c:1783-1866) puts its window and how many of the window's energies lie
where -- never anything the kernel computes.  Energies are re*re and im*im, each rounded to float32, then added in float32 (cnrmf).
A window entry i lives in lane i % 64, register i // 64 of the kernel's wavefront.

THE SEAM of a COMPLEX master: the fill stops when the walk reaches bin m_bins/2, so such a window has n = (bins to the seam) entries.
That is the restatement's rule (oracle/chz_oracle.c:chzo_estimate_noise).  The reference itself breaks out of the fill there but still
passes the full window size to quantile() (src/radio.c:1830-1846), which then reads entries nobody wrote: a seam-truncated window has
no defined value in the reference, and every expectation for one rests on the restatement, as the existing seam cases already do.

THE CONSTRUCTIONS are functions of (n, rng) that return n float32 magnitudes, for a window of exactly n entries; with_phases() turns
magnitudes into complex bins.  Magnitudes with the same bit pattern get the same phase, so that values meant to be bit-identical
(all_equal, two_values, duplicate_at_q) have bit-identical ENERGIES; all others get a phase of their own.  Energies are kept a few
percent away from the edges of a binade wherever a count has to be exact: rounding (a few 2^-24) cannot move one across."""
import math

import numpy as np

COMPLEX, REAL = 1, 2                  # oracle_lib.COMPLEX / .REAL
MIN_NOISE_BINS = 1000                 # src/radio.c:76
NQ = 0.10                             # src/radio.c:73
REGION = 2048 + 64                    # bins per region of a piecewise spectrum: the longest window and one more register row


# ------------------------------------------------------------------------------------------------
# the classifier
# ------------------------------------------------------------------------------------------------
def window_size(s_bins):
    return max(int(s_bins), MIN_NOISE_BINS)


def placement(m_bins, in_type, s_bins, shift):
    """(first master bin, entries filled) of the window of a channel `shift` bins from the master's centre; None: no window."""
    nbins = window_size(s_bins)
    if in_type == REAL:
        mbin = abs(int(shift)) - nbins // 2
        if mbin < 0:
            mbin = 0
        elif mbin + nbins > m_bins:
            mbin = m_bins - nbins
        return mbin, nbins
    mbin = int(shift) - nbins // 2
    if mbin < 0:
        mbin += m_bins
    elif mbin >= m_bins:
        mbin -= m_bins
    if mbin < 0 or mbin >= m_bins:
        return None
    half = m_bins // 2
    to_seam = half - mbin if mbin < half else half + m_bins - mbin
    return mbin, min(nbins, to_seam)


def shift_for(m_bins, in_type, s_bins, mbin):
    """the shift whose window starts at master bin mbin (REAL: mbin + nbins <= m_bins)"""
    nbins = window_size(s_bins)
    if in_type == REAL:
        assert 0 <= mbin <= m_bins - nbins
        return mbin + nbins // 2
    s = (mbin + nbins // 2) % m_bins
    return s - m_bins if s > m_bins // 2 else s


def energies(spectrum, idx):
    re = np.ascontiguousarray(spectrum.real[idx], np.float32)
    im = np.ascontiguousarray(spectrum.imag[idx], np.float32)
    return (re * re).astype(np.float32) + (im * im).astype(np.float32)


def rank(n):
    """(qi, frac) of quantile(.., n, 0.10) (src/radio.c:1760-1775), in the reference's own double arithmetic"""
    pos = NQ * (n - 1)
    qi = int(math.floor(pos))
    return qi, pos - qi


def window_energies(spectrum, in_type, s_bins, shift):
    mbin, n = placement(spectrum.shape[0], in_type, s_bins, shift)
    return energies(spectrum, (mbin + np.arange(n)) % spectrum.shape[0])


def classify(spectrum, in_type, s_bins, shift):
    """Which way a window goes through noise_est.  Keys: mbin, n, qi, frac0, exponent (the quantile's biased exponent field), below
    (values under that binade), total (values in it), branch ('le64' | 'le128' | 'le256' | 'full'), next_beyond (the interpolation's
    second order statistic lies above the binade), duplicate (it equals the first), lane_counts (the binade's values per lane)."""
    mbin, n = placement(spectrum.shape[0], in_type, s_bins, shift)
    e = window_energies(spectrum, in_type, s_bins, shift)
    assert np.all(np.isfinite(e))
    bits = e.view(np.uint32)
    order = np.sort(bits)
    qi, frac = rank(n)
    exponent = int(order[qi] >> 23)
    lo, hi = np.uint32(exponent << 23), np.uint32((exponent + 1) << 23)
    inside = (bits >= lo) & (bits < hi)
    below, total = int(np.sum(bits < lo)), int(np.sum(inside))
    assert below <= qi < below + total
    two = frac != 0.0 and qi + 1 < n
    return {"mbin": mbin, "n": n, "qi": qi, "frac0": frac == 0.0, "exponent": exponent, "below": below, "total": total,
            "branch": "le64" if total <= 64 else "le128" if total <= 128 else "le256" if total <= 256 else "full",
            "next_beyond": bool(two and below + total == qi + 1),
            "duplicate": bool(two and order[qi + 1] == order[qi]),
            "lane_counts": np.bincount(np.nonzero(inside)[0] % 64, minlength=64)}


def guess_counts(spectrum, in_type, s_bins, shift, exponent):
    """(c0, c1, qi): the window's values under binade `exponent` and under the next one -- what the kernel checks a guessed binade
    with (right if c0 <= qi < c1)"""
    bits = window_energies(spectrum, in_type, s_bins, shift).view(np.uint32)
    return int(np.sum(bits < np.uint32(exponent << 23))), int(np.sum(bits < np.uint32((exponent + 1) << 23))), rank(bits.size)[0]


# ------------------------------------------------------------------------------------------------
# window constructions: (n, rng) -> n float32 magnitudes
# ------------------------------------------------------------------------------------------------
def _mags(rng, *parts):
    """sqrt of the energies in `parts`, in random order"""
    e = np.concatenate([np.asarray(p, np.float64).reshape(-1) for p in parts])
    return np.sqrt(e[rng.permutation(e.size)]).astype(np.float32)


def _upper(rng, m):
    """m energies above the binade [1, 2): 40 % of them crowded into [2.05, 2.6], the rest in [4.2, 7.8].  The estimate is the mean of
    the energies up to 1.5 x quantile: with the quantile in the middle of [1, 2) that cut falls into the crowd, where the neighbouring
    order statistic taken for the quantile (a few hundredths off) moves it across a dozen values -- without the crowd the cut would
    lie in an empty stretch and the estimate would not notice"""
    k = (2 * m) // 5
    return np.concatenate([rng.uniform(2.05, 2.6, k), rng.uniform(4.2, 7.8, m - k)])


def _three_levels(n, rng, k_below, k_in, scale=1.0):
    """k_below energies in [0.25, 0.5), k_in in [1, 2), the rest above (_upper) (all times scale)"""
    return _mags(rng, scale * rng.uniform(0.26, 0.49, k_below), scale * rng.uniform(1.05, 1.95, k_in), scale * _upper(rng, n - k_below - k_in))


def le64(n, rng):
    k = max(1, min(round(0.04 * n), 60))
    return _three_levels(n, rng, rank(n)[0] - k // 2, k)


def white_noise(n, rng, scale=0.7):
    """exponential energies: |X|^2 of Gaussian noise.  (0.7: the 0.10 quantile, 0.105 x scale, sits low in its binade [0.0625, 0.125),
    where the binade holds the most values -- some 0.08 n)"""
    return np.sqrt(scale * rng.exponential(1.0, n)).astype(np.float32)


def le128(n, rng):
    m = white_noise(n, rng)
    e = np.sort((m * m).astype(np.float32))
    q = e[rank(n)[0]]
    inside = int(np.sum((e >= 2.0 ** math.floor(math.log2(q))) & (e < 2.0 ** (math.floor(math.log2(q)) + 1))))
    if 70 <= inside <= 120:
        return m
    k = min(max(round(0.1 * n), 70), 120)                   # (a long window of white noise has more than 128 there)
    return _three_levels(n, rng, rank(n)[0] - k // 2, k)


def le256(n, rng):
    return _three_levels(n, rng, round(0.08 * n), min(max(round(0.2 * n), 140), 250))


def one_binade(n, rng):
    return _mags(rng, rng.uniform(1.001, 1.999, n))


def all_equal(n, rng):
    return np.full(n, 3.0, np.float32)


def two_values(n, rng):
    return np.where(rng.random(n) < 0.5, 1.0, 4.0).astype(np.float32)


def mostly_zero(n, rng):
    return np.where(rng.random(n) < 0.85, 0.0, rng.uniform(0.5, 2.0, n)).astype(np.float32)


def next_binade(n, rng, gap=1):
    """exactly qi + 1 - below values in the quantile's binade [1, 2): rank qi is the binade's largest and rank qi + 1 lies `gap`
    binades higher"""
    qi = rank(n)[0]
    k = min(31, qi + 1)
    up = 2.0 ** gap
    return _mags(rng, rng.uniform(0.26, 0.49, qi + 1 - k), rng.uniform(1.05, 1.95, k), up * rng.uniform(1.05, 1.95, n - qi - 1))


def next_adjacent(n, rng):
    return next_binade(n, rng, 1)


def next_far(n, rng):
    return next_binade(n, rng, 40)


def binade_edge(n, rng):
    """the two order statistics straddle 2.0: ranks 0 .. qi just below it, everything else just above"""
    qi = rank(n)[0]
    return _mags(rng, rng.uniform(1.5, 1.9999, qi + 1), rng.uniform(2.0001, 2.5, n - qi - 1))


def duplicate_at_q(n, rng, before=3, after=5):
    """ranks qi - 3 .. qi + 5 bit-identical, with other values of the same binade on both sides"""
    qi = rank(n)[0]
    lower = min(20, qi - before)
    return _mags(rng, rng.uniform(0.26, 0.49, qi - before - lower), rng.uniform(1.05, 1.4, lower), np.full(before + after + 1, 1.5),
                 rng.uniform(1.6, 1.95, 30), _upper(rng, n - qi - after - 1 - 30))


def duplicate_pair(n, rng):
    """only ranks qi and qi + 1 bit-identical: the fewest values <= the quantile (qi + 2) at which the second order statistic is the
    first again"""
    return duplicate_at_q(n, rng, 0, 1)


def wide_range(n, rng):
    return (10.0 ** rng.uniform(-15, 15, n)).astype(np.float32)


def huge(n, rng):
    """energies in [1e38, 3e38]: biased exponents 253 and 254, nothing overflows"""
    return _mags(rng, rng.uniform(1e38, 3e38, n))


def subnormal(n, rng):
    """energies 1e-42 .. 1e-37 and a few exact zeros: the quantile is a subnormal float, its binade is exponent 0 (and holds most of
    the window: the full-width loop)"""
    e = 10.0 ** rng.uniform(-42, -37, n)
    e[:5] = 0.0
    return _mags(rng, e)


def subnormal_few(n, rng):
    """exponent 0 through the compacted path: a few more than qi values subnormal (three of them exact zeros; nothing lies below
    this binade, so it has to hold the quantile's rank itself: 105 values of 1000, 197 of 1920), the rest far above"""
    k = rank(n)[0] + 6
    e = 10.0 ** rng.uniform(-42, -38.2, k)
    e[:3] = 0.0
    return _mags(rng, e, 10.0 ** rng.uniform(-36, -30, n - k))


def scaled(build, factor):
    """the same construction with every ENERGY times factor (a power of two: the window's counts move with the binades)"""
    g = np.float32(math.sqrt(factor))
    return lambda n, rng: (build(n, rng) * g).astype(np.float32)


def guess_boundary(kind, exponent):
    """Windows at the edges of the test a guessed binade [t0, 2 t0) has to pass (c0 = values under t0, c1 = values under 2 t0; right if
    c0 <= qi < c1).  'c0_eq_qi' and 'c1_eq_qi1' are the last windows that pass, 'c0_eq_qi1' and 'c1_eq_qi' the first that do not."""
    t0 = 2.0 ** (exponent - 127)

    def build(n, rng):
        qi = rank(n)[0]
        if kind == "c0_eq_qi":                  # the quantile is the binade's smallest
            parts = (rng.uniform(0.13, 0.9, qi), rng.uniform(1.05, 1.95, 60), _upper(rng, n - qi - 60))
        elif kind == "c1_eq_qi1":               # ... its largest
            parts = (rng.uniform(0.13, 0.9, qi - 20), rng.uniform(1.05, 1.95, 21), rng.uniform(2.1, 7.8, n - qi - 1))
        elif kind == "c0_eq_qi1":               # one value too many below: the quantile is the largest of the binade below
            parts = (rng.uniform(0.52, 0.9, qi + 1), rng.uniform(1.05, 1.95, 40), _upper(rng, n - qi - 41))
        else:                                   # "c1_eq_qi": one too few under 2 t0: the quantile is the smallest of the binade above
            parts = (rng.uniform(0.13, 0.9, qi - 20), rng.uniform(1.05, 1.95, 20), rng.uniform(2.1, 3.9, n - qi))
        return _mags(rng, *[t0 * p for p in parts])
    return build


def placed(where, k=64):
    """An le64-sized window whose binade values sit at chosen places: where(i) says whether window entry i (lane i % 64) may hold
    one; at most k of them do (a random choice), the quantile in their middle."""
    def build(n, rng):
        qi = rank(n)[0]
        idx = np.array([i for i in range(n) if where(i)])
        if idx.size > k:
            idx = np.sort(rng.choice(idx, k, replace=False))
        rest = np.setdiff1d(np.arange(n), idx)
        rest = rest[rng.permutation(rest.size)]
        nb = qi - idx.size // 2
        assert 0 <= nb and nb + idx.size < n
        e = np.empty(n)
        e[idx] = rng.uniform(1.05, 1.95, idx.size)
        e[rest[:nb]] = rng.uniform(0.26, 0.49, nb)
        e[rest[nb:]] = _upper(rng, rest.size - nb)
        return np.sqrt(e).astype(np.float32)
    return build


def alone_above(lane):
    """next_binade with the one next-higher value alone in `lane`: every other value above the binade is at least twice as large"""
    def build(n, rng):
        qi = rank(n)[0]
        spot = lane + 64 * int(rng.integers(0, (n - lane + 63) // 64))
        rest = np.setdiff1d(np.arange(n), [spot])
        rest = rest[rng.permutation(rest.size)]
        e = np.empty(n)
        e[spot] = 2.5
        e[rest[:qi - 30]] = rng.uniform(0.26, 0.49, qi - 30)
        e[rest[qi - 30:qi + 1]] = rng.uniform(1.05, 1.95, 31)
        e[rest[qi + 1:]] = rng.uniform(5.5, 30.0, rest.size - qi - 1)
        return np.sqrt(e).astype(np.float32)
    return build


# (in this order a spectrum's first four regions -- one workgroup -- take at least three different branches)
BRANCH_CASES = [("le64", le64), ("le128", le128), ("le256", le256), ("full", one_binade), ("all_equal", all_equal), ("next_adjacent", next_adjacent),
                ("mostly_zero", mostly_zero), ("next_far", next_far), ("two_values", two_values), ("subnormal_few", subnormal_few),
                ("subnormal", subnormal), ("duplicate_at_q", duplicate_at_q), ("binade_edge", binade_edge), ("wide_range", wide_range),
                ("huge", huge), ("duplicate_pair", duplicate_pair)]

LANE_CASES = [("single_lane", placed(lambda i: i % 64 == 5)), ("lane0", placed(lambda i: i % 64 == 0)), ("lane63", placed(lambda i: i % 64 == 63)),
              ("row3_only", placed(lambda i: i % 64 >= 48, 60)), ("rows_0_and_3", placed(lambda i: i % 64 < 16 or i % 64 >= 48, 60)),
              ("lanes_15_16", placed(lambda i: i % 64 in (15, 16)))] + [("alone_above_%d" % ln, alone_above(ln)) for ln in (0, 15, 16, 47, 63)]


def expected_lanes(name):
    """the lanes a LANE_CASES window may have its binade's values in (alone_above: None, nothing is placed)"""
    return {"single_lane": [5], "lane0": [0], "lane63": [63], "row3_only": list(range(48, 64)), "rows_0_and_3": list(range(16)) + list(range(48, 64)),
            "lanes_15_16": [15, 16]}.get(name)


# ------------------------------------------------------------------------------------------------
# spectrum builders
# ------------------------------------------------------------------------------------------------
def with_phases(mag, rng):
    """complex64 bins of these magnitudes: a random phase per DISTINCT magnitude, so that both re and im contribute and equal
    magnitudes stay equal energies"""
    mag = np.ascontiguousarray(mag, np.float32)
    u, inv = np.unique(mag.view(np.uint32), return_inverse=True)
    ph = (2 * np.pi * rng.random(u.size))[inv.reshape(-1)]
    return (mag.astype(np.float64) * np.exp(1j * ph)).astype(np.complex64)


def region_starts(B, in_type):
    """first bins of the regions a spectrum of B bins has room for; none holds the seam bin B/2 of a COMPLEX master in its inside"""
    out, at = [], 0
    while at + REGION <= B:
        if in_type == COMPLEX and at < B // 2 < at + REGION:
            at = B // 2
            continue
        out.append(at)
        at += REGION
    return out


def piecewise_spectrum(B, in_type, s_bins, regions, rng, offsets=(0, 37, 64)):
    """Several constructions side by side over a background of white noise, REGION bins each: the region's first window_size(s_bins)
    bins are the construction's window, the rest further draws of it.  Returns (spectrum, [(name, [shifts])]): per region the shifts
    whose windows lie wholly inside it -- the first one IS the constructed window, the others lie `offsets` bins on --
    so that one launch has neighbouring wavefronts of a workgroup in different branches.  Every other region's first shift is negative
    on a REAL master (an inverted channel reads the same bins)."""
    n = window_size(s_bins)
    starts = region_starts(B, in_type)
    assert len(regions) <= len(starts) and n + 64 <= REGION
    spec = with_phases(white_noise(B, rng), rng)
    out = []
    for r, ((name, build), at) in enumerate(zip(regions, starts)):
        mag = np.concatenate([build(n, rng) for _ in range(-(-REGION // n))])[:REGION]
        spec[at:at + REGION] = with_phases(mag, rng)
        shifts = [shift_for(B, in_type, s_bins, at + o) for o in offsets if o + n <= REGION]
        if in_type == REAL and r % 2:
            shifts[0] = -shifts[0]
        out.append((name, shifts))
    return spec, out


def chunks(cases, B, in_type):
    """the case list in pieces of as many regions as one spectrum holds"""
    k = len(region_starts(B, in_type))
    return [cases[i:i + k] for i in range(0, len(cases), k)]


SEAM_N = (1, 2, 11, 63, 64, 65, 501, 1000)


def seam_spectrum(N, s_bins, rng, build=white_noise):
    """A COMPLEX master's spectrum and the shifts of windows at its seams.  Returns (spectrum, [(label, shift, n)]): windows that stop
    at bin N/2 after n = 1, 2, 11, 63, 64, 65, 501 and 1000 entries (11 and 501: frac == 0; under 64: whole rows of lanes hold only
    padding), one entry short of the whole window, windows that START at the seam and one bin past it, and windows that wrap from the
    last bin to bin 0."""
    nbins = window_size(s_bins)
    half = N // 2
    spec = with_phases(build(N, rng), rng)
    out = [("stop_%d" % k, shift_for(N, COMPLEX, s_bins, half - k), k) for k in sorted(set(SEAM_N + (nbins - 1,))) if k <= nbins]
    out += [("start_at_seam", shift_for(N, COMPLEX, s_bins, half), nbins), ("start_past_seam", shift_for(N, COMPLEX, s_bins, half + 1), nbins)]
    out += [("wrap_%d" % k, shift_for(N, COMPLEX, s_bins, N - k), nbins) for k in (1, 500, nbins - 1)]
    return spec, out


# ------------------------------------------------------------------------------------------------
# the plans of tests/test_gpu_noise_select.py: what it injects and which shifts it sets, from fixed seeds (tests/test_noise_window_cases.py
# checks the same plans without a device)
# ------------------------------------------------------------------------------------------------
ENGINE_L, ENGINE_M = 25920, 6481                       # 16201 bins on a REAL master, 32400 on a COMPLEX one
BANKS = [(300, 240), (1200, 960), (1920, 1536)]        # windows of 1000 bins (noise_est<16>), 1200 and 1920 of 2048 entries (noise_est<32>)
MASTERS = {"real": REAL, "complex": COMPLEX}
SAMPRATE = 50.0 * ENGINE_L


def master_bins(in_type):
    N = ENGINE_L + ENGINE_M - 1
    return N // 2 + 1 if in_type == REAL else N


def _odd_count(shifts, extra):
    """a channel count that is no multiple of 4 (four channels share a workgroup): one more shift if need be"""
    return shifts + [extra] if len(shifts) % 4 == 0 else shifts


def region_plan(cases, in_type, P, offsets, seed):
    """[(spectrum, [(name, shifts)])] for a case list, as many spectra as it takes, and all the shifts of all of them"""
    B = master_bins(in_type)
    parts = [piecewise_spectrum(B, in_type, P, part, np.random.default_rng([seed, in_type, P, i]), offsets)
             for i, part in enumerate(chunks(cases, B, in_type))]
    shifts = []
    for j in range(len(offsets)):                  # every region's first shift, then every region's second: the four channels of a
        for _, regions in parts:                   # workgroup are in four different regions
            shifts += [s[j] for _, s in regions if j < len(s) and s[j] not in shifts]
    return parts, shifts


def branch_plan(in_type, P):
    """BRANCH_CASES over one bank: (spectra with their regions, shifts).  A COMPLEX master adds two windows that stop at the seam after
    11 and 501 entries, in the white noise before it: frac == 0 (a REAL master's window always has all its max(P, 1000) entries, and
    none of the bank sizes is 1 modulo 10)."""
    parts, shifts = region_plan(BRANCH_CASES, in_type, P, (0, 37, 64), 1)
    B = master_bins(in_type)
    if in_type == COMPLEX:
        shifts += [shift_for(B, COMPLEX, P, B // 2 - k) for k in (11, 501)]
    return parts, _odd_count(shifts, 3)


def lane_plan(in_type, P):
    parts, shifts = region_plan(LANE_CASES, in_type, P, (0,), 2)
    return parts, _odd_count(shifts, 3)


def seam_plan(P):
    """[(spectrum, [(label, shift, n)])]: white noise and sixty orders of magnitude at the seams of the COMPLEX master"""
    N = master_bins(COMPLEX)
    return [seam_spectrum(N, P, np.random.default_rng([3, P, i]), build) for i, build in enumerate((white_noise, wide_range))]


GUESS_BASE = 127                                      # the quantile's exponent of window "A" below: its binade is [1, 2)


def _guess_a(n, rng):
    k = min(max(round(0.1 * n), 70), 120)
    return _three_levels(n, rng, rank(n)[0] - k // 2, k)


GUESS_SEQUENCE = [("A", _guess_a), ("A", _guess_a), ("up", scaled(_guess_a, 2.0)), ("mostly_zero", mostly_zero), ("subnormal", subnormal),
                  ("subnormal_few", subnormal_few), ("huge", huge), ("A", _guess_a), ("c0_eq_qi", guess_boundary("c0_eq_qi", GUESS_BASE)),
                  ("A", _guess_a), ("c1_eq_qi1", guess_boundary("c1_eq_qi1", GUESS_BASE)), ("A", _guess_a),
                  ("c0_eq_qi1", guess_boundary("c0_eq_qi1", GUESS_BASE)), ("A", _guess_a), ("c1_eq_qi", guess_boundary("c1_eq_qi", GUESS_BASE))]
GUESS_CHANNELS = 5


def guess_plan(in_type, P):
    """The script of the guess test: (spectra of consecutive blocks, shifts, names[block][channel]).  Channel c's window holds step
    (block + c) of GUESS_SEQUENCE, so the channels of a workgroup are at different steps in every block; one block more than the
    sequence is long, so every channel also goes from its last step back to its first.  Every "A" of a channel is the same window."""
    B = master_bins(in_type)
    n = window_size(P)
    starts = region_starts(B, in_type)[:GUESS_CHANNELS]
    rng = np.random.default_rng([4, in_type, P])
    background = with_phases(white_noise(B, rng), rng)
    made = {}
    spectra, names = [], []
    for b in range(len(GUESS_SEQUENCE) + 1):
        spec = background.copy()
        row = []
        for c, at in enumerate(starts):
            name, build = GUESS_SEQUENCE[(b + c) % len(GUESS_SEQUENCE)]
            if (c, name) not in made:
                made[c, name] = with_phases(build(n, rng), rng)
            spec[at:at + n] = made[c, name]
            row.append(name)
        spectra.append(spec)
        names.append(row)
    return spectra, [shift_for(B, in_type, P, at) for at in starts], names


def guess_events(spectra, in_type, P, shifts):
    """What the kernel's guess meets, block by block and channel by channel, from the counts alone: [block][channel] of
    (hint exponent or None, c0, c1, qi, this block's exponent).  The hint is the exponent of the channel's last block: the kernel
    stores a new one whenever its guess fails, and a guess that passes IS the block's exponent."""
    out, last = [], [None] * len(shifts)
    for spec in spectra:
        row = []
        for c, s in enumerate(shifts):
            k = classify(spec, in_type, P, s)
            c0, c1, qi = guess_counts(spec, in_type, P, s, last[c]) if last[c] is not None else (None, None, k["qi"])
            row.append((last[c], c0, c1, qi, k["exponent"]))
            last[c] = k["exponent"]
        out.append(row)
    return out
