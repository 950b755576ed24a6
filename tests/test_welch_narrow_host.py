"""Host-side closed forms of the narrowband analyser (chz_bank_welch_steps exposes what chz_bank_welch_configure and the kernel
bb_ring_append compute): the ring position of a block across the wrap of the 32-bit block number, and the hop / adjust roundings
against the reference's expressions (src/spectrum.c:247, :259-264, :278)."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_pkg


@pytest.fixture(scope="module")
def steps():
    lib = load_pkg().engine.lib()

    def call(fft_n, fft_avg, overlap, job=0, job0=0, olen=1, ring_len=1):
        out = (C.c_longlong * 3)()
        assert lib.chz_bank_welch_steps(fft_n, fft_avg, overlap, job & 0xFFFFFFFF, job0 & 0xFFFFFFFF, olen, ring_len, C.byref(out)) == 0
        return int(out[0]), int(out[1]), int(out[2])
    return call


def test_ring_position_is_a_closed_form_across_the_wrap_of_the_block_number(steps):
    olen, ring_len = 240, 8 * 1000 + 5 * 240                                           # not a multiple of olen
    for job0 in (0, 7, 0xFFFFFFF0, 0xFFFFFFFF, 0x7FFFFFFF):
        for d in (0, 1, 15, 16, 17, 38, 39, 1000, 123456789, 0x7FFFFFFF):
            job = (job0 + d) & 0xFFFFFFFF
            assert steps(64, 1, 0.0, job, job0, olen, ring_len)[2] == d * olen % ring_len, (job0, d)
        # consecutive blocks follow each other in the ring, also across 2^32
        a = steps(64, 1, 0.0, job0 + 20, job0, olen, ring_len)[2]
        b = steps(64, 1, 0.0, job0 + 21, job0, olen, ring_len)[2]
        assert b == (a + olen) % ring_len
        # a block from before the attach writes nothing
        assert steps(64, 1, 0.0, job0 - 1, job0, olen, ring_len)[2] == -1
        assert steps(64, 1, 0.0, job0 - 1000, job0, olen, ring_len)[2] == -1
    # the product is formed in 64 bits: 2^31 - 1 blocks of 2^20 samples
    assert steps(64, 1, 0.0, 0x7FFFFFFF, 0, 1 << 20, (1 << 40) + 12345)[2] == (0x7FFFFFFF << 20) % ((1 << 40) + 12345)


def test_hop_and_adjust_round_as_the_reference_does(steps):
    assert steps(75, 3, 0.5)[0] == 37                                                  # 75 - lrint(37.5) = 75 - 38, not lrint(37.5) = 38
    differ = 0
    for fft_n in list(range(8, 140)) + [299, 300, 1000, 1031, 4097, 16384, 65535, 65536]:
        for overlap in (0.0, 0.1, 0.25, 1 / 3, 0.5, 0.625, 0.75, 0.9, 0.99):
            for fft_avg in (1, 2, 3, 8, 50):
                hop, adjust, _ = steps(fft_n, fft_avg, overlap)
                back = int(np.rint(fft_n * overlap))                                   # :278 (lrint: to nearest, ties to even)
                assert hop == fft_n - back                                             # fft_n forwards (:259-264), `back` back
                assert adjust == int(np.rint(fft_n * (1 + (fft_avg - 1) * (1 - overlap))))   # :247
                assert 0 <= hop <= fft_n and adjust <= fft_avg * fft_n                 # (the window never reaches past the reference's ring)
                differ += hop != int(np.rint(fft_n * (1 - overlap)))
    assert differ > 0                                                                  # (the wideband form's hop is another number)
