"""Pools of CTCSS / PL tone decoders (chz_ctcss_*, kernel ctcss_ovs) at sample rates other than the 24, 8 and 32 kHz of tests/test_gpu_ctcss.py,
against tests/ctcss_oracle.py.  ctcss_check_geom derives everything from the rate, and these are the rates at which the derived master differs in kind:
  11k    11025 Hz   L 2205, N 4410    an odd L: N / 2 = 2205, a forward transform of radices 3 3 5 7 7, 2 L bytes of samples that are no multiple of 4
  22k    22050 Hz   L 4410, N 8820    70,560 B of LDS, the first of these beyond the 64 KB step (1024 threads), radices 2 3 3 5 7 7
  41k    40960 Hz   L 8192, N 16384   the largest master the pool can hold: 131,072 B of LDS, radix 4 alone (and one 2)
  16k    16000 Hz   L 3200, N 6400    51,200 B: beyond 40 KB (1024 threads) and below the 64 KB step
  9999   9999 Hz    L 2000, N 4000    0.2 x samprate = 1999.8 is rounded: L = lrint(1999.8) = 2000, the block is not 0.2 s
Each rate runs instances 0, 1 and 2 of tests/test_gpu_ctcss.py's scenario (the 55 tones in table order with the threshold and the first
renormalisation; two tones in noise; the full-scale square wave, exact zeros and a tone from mid-block -- one sample before the middle at
11025 Hz, where L is odd) and instance 0 again from device memory, in a big-endian pool of capacity 2, the order permuted from call to call.

Bounds and input condition: those of tests/test_gpu_ctcss.py, through its check() and input_condition(), unchanged -- indices equal on every
block, every energy within 1e-6 of the block's largest or 4 x the f32 twin's own distance, every decision FLOOR = 100 x the twin's distance
away from a tie, asserted on the restatement before anything is compared.

Measured on the restatement (FLOOR / smallest margin, the block it is in):
  instance 0   11k 1.55e-5 / 8.12e-5 (75)   22k 1.36e-5 / 7.89e-5 (75)   41k 1.54e-5 / 8.00e-5 (75)   16k 1.64e-5 / 8.33e-5 (75)   9999 1.42e-5 / 5.09e-3 (18)
  instance 1   FLOOR 1.0e-5 to 1.5e-5, smallest margin 1.95e-3 (16k) to 7.4e-3 (9999)
  instance 2   FLOOR 1.5e-4 to 2.7e-4 (full scale against a window of zeros), smallest margin 0.18 to 0.23, and 0.032 at 9999 Hz, whose "100 Hz" square
               wave (49 samples a half period) is one of 102.0 Hz, between 100.0 and 103.5: the test derives the expected tone from that frequency
Worst measured / allowed, printed by every test: on the MI355X 0.59 at most (instance 2 at 22050 Hz), 0.39 for instances 0 and 1 (9999 Hz); on the CPU
build of the engine 0.72 and 0.39.

The reference pin (tests/test_ctcss_reference.py) covers all five rates on both of the reference's transforms: its feeder takes the number
of packets a block (nine of 245 samples at 11025 Hz, sixteen of 512 at 40960 Hz), so no rate is left on the restatement alone."""
import functools

import pytest

import ctcss_oracle as co
import oracle_lib as ol
from conftest import load_pkg
from test_gpu_ctcss import CAP, T, PAIRS, check, instance1, instance2, pairs, run_pool

pytestmark = pytest.mark.gpu

RATES = {"11k": (11025.0, 2205), "22k": (22050.0, 4410), "41k": (40960.0, 8192), "16k": (16000.0, 3200), "9999": (9999.0, 2000)}


@pytest.fixture(scope="module")
def pkg():
    p = load_pkg()
    if p.engine.lib().chz_device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests cannot run (there is no CPU fallback)")
    ol.build()
    return p


@functools.lru_cache(maxsize=None)
def scenario(rate):
    """int16 blocks [nblocks][L] of instances 0-2"""
    fs = RATES[rate][0]
    return [co.instance0(fs), instance1(fs), instance2(fs)]


@functools.lru_cache(maxsize=None)
def restatement(rate, f32):
    return [co.run(b, RATES[rate][0], f32=f32) for b in scenario(rate)]


_device_runs = {}


def device_run(pkg, rate):
    """the scenario's big-endian pool: instances 0-2 and 3 (instance 0's samples in device memory)"""
    if rate not in _device_runs:
        b = scenario(rate)
        _device_runs[rate] = run_pool(pkg, RATES[rate][0], CAP, {0: b[0], 1: b[1], 2: b[2], 3: b[0]}, device=(3,))
    return _device_runs[rate]


@pytest.mark.parametrize("rate", list(RATES))
def test_geometry(pkg, rate):
    fs, L = RATES[rate]
    pool = pkg.engine.CtcssPool(fs, CAP)
    try:
        assert pool.geometry == co.geometry(fs)
        assert pool.geometry == {"L": L, "M": L + 1, "N": 2 * L, "olen": 100, "P": 200, "shift": 60, "ntones": 55}
        assert pkg.engine.lib().chz_ctcss_capacity(pool._h) == CAP
    finally:
        pool.close()
    assert 0.2 * 9999.0 != 2000 and (8 * 8820, 8 * 16384) == (70560, 131072)


@pytest.mark.parametrize("rate", list(RATES))
def test_every_standard_tone_in_table_order_the_threshold_and_the_first_renormalisation(pkg, rate):
    ref = restatement(rate, False)[0]
    assert len(ref) == 175
    for k in range(len(T)):
        assert [r["tone_index"] for r in ref[3 * k + 1:3 * k + 3]] == [k, k], (rate, k)
    assert [r["tone_index"] for r in ref[165:175]] == [54, -1, -1, -1, -1, 12, -1, 41, 41, 41]
    assert [r["current_index"] for r in ref[165:175]] == [54, 54, 54, 54, 54, 12, 12, 41, 41, 41]
    assert not ref[166]["energies"].any() and ref[166]["energy"] == co.THRESHOLD
    check(ref, restatement(rate, True)[0], pairs(device_run(pkg, rate)[0]), "%s instance 0" % rate)


@pytest.mark.parametrize("rate", list(RATES))
def test_two_tones_of_unequal_amplitude_in_noise(pkg, rate):
    ref = restatement(rate, False)[1]
    for k, (a, b) in enumerate(PAIRS):
        assert [r["tone_index"] for r in ref[3 * k + 1:3 * k + 3]] == [a, a], (rate, k)
    check(ref, restatement(rate, True)[1], pairs(device_run(pkg, rate)[1]), "%s instance 1" % rate)


@pytest.mark.parametrize("rate", list(RATES))
def test_full_scale_square_wave_exact_zeros_and_a_tone_from_mid_block(pkg, rate):
    fs = RATES[rate][0]
    blocks = scenario(rate)[2]
    assert blocks.shape == (12, RATES[rate][1]) and blocks.min() == -32768 and blocks.max() == 32767
    ref = restatement(rate, False)[2]
    square = fs / (2 * int(fs / 200))                                       # 100 Hz where 200 divides the rate; 100.2 Hz at 11025, 102.0 Hz at 9999 Hz
    nearest = min(range(len(T)), key=lambda k: abs(T[k] - square))
    assert nearest == (13 if rate == "9999" else 12)
    assert [r["tone_index"] for r in ref[1:3]] == [nearest, nearest] and not ref[5]["energies"].any() and ref[8]["tone_index"] == 21
    check(ref, restatement(rate, True)[2], pairs(device_run(pkg, rate)[2]), "%s instance 2" % rate)


@pytest.mark.parametrize("rate", list(RATES))
def test_samples_in_device_memory_give_the_same_bytes(pkg, rate):
    got = device_run(pkg, rate)
    assert len(got[3]) == len(got[0]) == 175
    for blk, (a, b) in enumerate(zip(got[0], got[3])):
        assert a[2] == b[2] and a[1].tobytes() == b[1].tobytes(), (rate, blk)


REFUSALS = [(44100.0, "16384"),                                              # L 8820, N 17,640
            (41000.0, "16384")]                                              # L 8200, N 16,400: sixteen points beyond the largest


@pytest.mark.parametrize("fs,word", REFUSALS)
def test_rates_that_are_refused(pkg, fs, word):
    E = pkg.engine
    for make in (lambda: E.CtcssPool.check(fs), lambda: E.CtcssPool(fs, CAP)):
        with pytest.raises(E.ChzError) as e:
            make()
        assert word in str(e.value), str(e.value)
