"""The signal generators of the pool tests, held to what they yielded before they were extended (no GPU, no engine).

afsk_oracle.modulate() has a true baud clock -- sample n carries line bit floor(n bitrate / samprate) -- for tests/test_gpu_afsk_rates.py; wherever
samprate / bitrate is an integer it must return the int16 values it returned when it repeated every bit that many times, so that the
scenarios of tests/test_gpu_afsk.py do not move.  test_gpu_ctcss.instance2() takes an odd L for tests/test_gpu_ctcss_rates.py; for an even L it must
yield what it yielded."""
import numpy as np
import pytest

import afsk_oracle as ao
import ctcss_oracle as co
import test_gpu_ctcss as gc


def modulate_by_repetition(bits, samprate, bitrate=ao.BITRATE, mark=ao.MARK, space=ao.SPACE, amplitude=0.5, space_gain=1.0, offset=0, phase=0.0):
    """the generator as it was while samprate / bitrate had to be an integer: every bit repeated samprate / bitrate times"""
    sps = int(round(samprate / bitrate))
    assert sps * bitrate == samprate
    tone, level = [], 0
    for b in bits:
        if not b:
            level ^= 1
        tone.append(level)
    tone = np.repeat(np.asarray(tone, np.int8), sps)
    freq = np.where(tone == 0, mark, space)
    ph = phase + 2 * np.pi * np.cumsum(freq) / samprate
    x = amplitude * np.where(tone == 0, 1.0, space_gain) * np.sin(ph)
    return np.rint(32767.0 * x[offset:]).astype(np.int16)


def some_bits():
    rng = np.random.default_rng(3)
    return ao.line_bits([("flags", 5), ("frame", bytes(rng.integers(0, 256, 40, dtype=np.uint8))), ("flags", 2), ("frame", b"\xff" * 9), ("flags", 3)])


@pytest.mark.parametrize("rates", [(48000.0, 1200.0, 1200.0, 2200.0), (24000.0, 1200.0, 1200.0, 2200.0), (12000.0, 1200.0, 1200.0, 2200.0),
                                   (22050.0, 1225.0, 1200.0, 2200.0), (16000.0, 400.0, 1600.0, 1800.0), (4800.0, 1200.0, 1200.0, 2200.0)])
def test_the_baud_clock_yields_the_same_samples_wherever_a_bit_is_a_whole_number_of_samples(rates):
    fs, br, mk, sp = rates
    bits = some_bits()
    for kw in ({}, {"amplitude": 0.4}, {"amplitude": 0.25, "space_gain": 1.8, "offset": 7}, {"amplitude": 0.25, "space_gain": 1.8, "phase": 1.0}, {"phase": 0.7, "offset": 3}):
        new, old = ao.modulate(bits, fs, br, mk, sp, **kw), modulate_by_repetition(bits, fs, br, mk, sp, **kw)
        assert new.dtype == np.int16 and np.array_equal(new, old), (rates, kw)


@pytest.mark.parametrize("rates", [(22050.0, 1200.0, 1200.0, 2200.0), (16000.0, 300.0, 1600.0, 1800.0), (11025.0, 1200.0, 1200.0, 2200.0)])
def test_sample_n_carries_line_bit_floor_n_bitrate_over_samprate(rates):
    """against a sample-by-sample statement of the rule, in integer arithmetic"""
    fs, br, mk, sp = rates
    bits = some_bits()
    level, tones = 0, []
    for b in bits:
        if not b:
            level ^= 1
        tones.append(level)
    n = 0
    x, ph = [], 0.0
    while n * int(br) // int(fs) < len(bits):
        t = tones[n * int(br) // int(fs)]
        ph += mk if t == 0 else sp                                          # (np.cumsum adds from the left as well)
        x.append(0.4 * (1.0 if t == 0 else 1.8) * np.sin(0.3 + 2 * np.pi * ph / fs))
        n += 1
    got = ao.modulate(bits, fs, br, mk, sp, amplitude=0.4, space_gain=1.8, phase=0.3)
    assert got.shape[0] == n == -(-len(bits) * int(fs) // int(br))
    assert np.array_equal(got, np.rint(32767.0 * np.array(x)).astype(np.int16))
    lengths = {int(v) for v in np.diff(-((-np.arange(len(bits) + 1) * int(fs)) // int(br)))}
    assert lengths == {int(fs // br), int(fs // br) + 1}                    # no bit is a whole number of samples off the others by more than one


@pytest.mark.parametrize("fs", [24000.0, 8000.0, 16000.0, 22050.0, 40960.0, 9999.0])
def test_instance_2_of_the_ctcss_scenario_is_unchanged_for_an_even_block(fs):
    L = co.geometry(fs)["L"]
    assert L % 2 == 0
    half = int(fs / 200)
    sq = np.where((np.arange(3 * L) // half) % 2 == 0, 32767, -32768).astype(np.int16).reshape(3, L)
    late = co.generate(fs, [(4, [(136.5, 0.3)], 0.0)])
    late = np.concatenate([np.zeros(L // 2, np.int16), late.reshape(-1)[:3 * L + L // 2]]).reshape(4, L)      # as it was written for an even L
    was = np.concatenate([sq, np.zeros((3, L), np.int16), late, np.zeros((2, L), np.int16)])
    assert np.array_equal(gc.instance2(fs), was)


def test_instance_2_of_the_ctcss_scenario_at_an_odd_block():
    fs, L = 11025.0, 2205
    b = gc.instance2(fs)
    assert b.shape == (12, L) and not b[3:6].any() and not b[6, :L // 2].any() and b[6, L // 2 + 1] != 0 and not b[10:].any()
    tone = co.generate(fs, [(4, [(136.5, 0.3)], 0.0)]).reshape(-1)
    assert np.array_equal(b[6:10].reshape(-1)[L // 2:], tone[:4 * L - L // 2])
