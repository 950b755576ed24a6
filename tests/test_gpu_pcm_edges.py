"""The device's PCM packers (demod_put, demod_s16, demod_g711, demod_f16_bits in chz_kernels.h) at the values where a packer goes wrong.

A linear channel at unit gain without AGC hands its input to the packer bit for bit (tests/pcm_edge_cases.py), so blocks written with
chz_bank_write_block put every value of F16_VALUES (every binary16 value, every rounding tie, the subnormal and overflow thresholds,
-0.0, an f32 subnormal, infinities; quiet NaNs with them) and of I16_VALUES (every 16-bit level, every x.5 tie with the floats on either
side, +-1.0, values beyond the clip, G.711's segment edges) in front of each of the eight encodings.  The PCM must be chzo_pcm_pack's
(oracle/chz_oracle.c) of the same floats, byte for byte; tests/test_oracle_vs_reference.py pins that packer to the reference's rtp.c /
import.h at the same values.  Blocks of 1024 samples under the master (11520, 11521): P = 2048, the largest a demodulator bank may have.

The same file runs on the fiber emulator (tests/test_engine_emulated.py), where demod_f16_bits is the hand-written bit routine and not
the hardware conversion the device compiles.  Nothing is thinned there: the whole file takes about 6 s on the emulator.

Which store reaches the row, and the test that feeds it:

  demod_put from demod_lin_lanes' generic store (mixed encodings in a wavefront)    test_every_encoding_packs_every_edge_value [lanes-1, lanes-2]
  demod_put from demod_linear_tail (one wavefront per channel), mono and stereo     test_every_encoding_packs_every_edge_value [wave-1, wave-2]
  demod_f16_bits: the device's conversion / the emulator's bit routine              test_every_encoding_packs_every_edge_value (F16LE, F16BE rows)
  the F32 encodings pass bit patterns through (f32 subnormals, -0.0)                test_every_encoding_packs_every_edge_value (F32LE, F32BE rows)
  demod_s16 in demod_lin_lanes' packed 8-byte store (s16_mono)                      test_packed_s16_stores_equal_the_generic_store [stride 8192]
  ... and the generic store of the same bank ((pcm_stride & 7) != 0)                test_packed_s16_stores_equal_the_generic_store [stride 2052]
  demod_s16 in demod_fm_lanes' packed 8-byte store (fm_s16), clipping               test_fm_pcm_at_the_clip [lanes-s16le, lanes-s16be: the uniform bank]
  demod_put from demod_fm_lanes' generic store, clipping                            test_fm_pcm_at_the_clip [lanes-*: the mixed bank]
  demod_put from demod_linear_tail's FM branch, clipping                            test_fm_pcm_at_the_clip [wave-*]
"""
import functools

import numpy as np
import pytest

import oracle_lib as ol
import pcm_edge_cases as pe
from conftest import load_pkg
from test_gpu_demod_shapes import OVERLAP2, _compare_block, _inject, _inject_bank, _restated

pytestmark = pytest.mark.gpu

N, BT = 1024, 0.02
FS = float(round(N / BT))
# float encodings at the even positions, integer ones at the odd: a wavefront of 64 neighbouring channels holds all eight
ENC8 = [ol.PCM_F16LE, ol.PCM_S16LE, ol.PCM_F32LE, ol.PCM_MULAW, ol.PCM_F16BE, ol.PCM_S16BE, ol.PCM_F32BE, ol.PCM_ALAW]
FLOAT_ENC = (ol.PCM_F16LE, ol.PCM_F16BE, ol.PCM_F32LE, ol.PCM_F32BE)


@pytest.fixture(scope="module")
def pkg():
    p = load_pkg()
    if p.engine.lib().chz_device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests cannot run (there is no CPU fallback)")
    ol.build()
    return p


def _pad_rows(r, nrows):
    return np.concatenate([r, np.zeros((nrows - len(r), r.shape[1]), np.complex64)])


def _row_status(rows, channels):
    """The restated demodulator's status for every row: [(frame, mute, output_power, gain)].  It does not depend on the encoding."""
    d = ol.LinDemod(pe.unit_gain_params(ol, channels, ol.PCM_F32LE, FS))
    out = []
    for r in rows:
        pcm, st = d.block(r, 1.0, 1e-12, BT)
        assert st.frame == ol.FRAME_DATA and st.gain == 1.0
        assert np.array_equal(pcm, pe.packer_input(r, channels).view(np.uint8))        # the restatement itself passes the bits through
        assert st.mute == (0 if r.view(np.float32).any() else 1)
        out.append((st.frame, st.mute, st.output_power, st.gain))
    return out


def _same_power(got, want):
    if np.isfinite(want):
        return got == pytest.approx(want, rel=1e-5, abs=1e-300)
    return got == want or (np.isnan(got) and np.isnan(want))


def _check_status(got, want, where):
    frame, mute, opower, gain = want
    assert (got.frame, got.mute, got.gain) == (frame, mute, gain), where
    assert _same_power(got.output_power, opower), (where, got.output_power, opower)


def _decode(enc, raw):
    """PCM bytes of a float encoding [.., bytes per sample] -> float64."""
    dt = {ol.PCM_F16LE: "<f2", ol.PCM_F16BE: ">f2", ol.PCM_F32LE: "<f4", ol.PCM_F32BE: ">f4"}[enc]
    return np.ascontiguousarray(raw).view(dt)[..., 0].astype(np.float64)


@functools.lru_cache(maxsize=None)
def _edge_case(channels):
    """(rows of the float class, rows of the integer class, want[enc] = uint8[R][bytes], NaN positions of the float rows, status per
    class and row): R rows each, a multiple of 8, the rows beyond a set all zero."""
    fl = pe.rows(np.concatenate([pe.F16_VALUES, pe.QUIET_NANS]), channels, N)
    it = pe.rows(pe.I16_VALUES, channels, N)
    R = -(-max(len(fl), len(it)) // 8) * 8
    fl, it = _pad_rows(fl, R), _pad_rows(it, R)
    want = {}
    for enc in ENC8:
        src = fl if enc in FLOAT_ENC else it
        want[enc] = np.stack([pe.pack(ol, enc, pe.packer_input(r, channels)) for r in src])
    nan = np.stack([np.isnan(pe.packer_input(r, channels)) for r in fl])
    assert nan.sum() == len(pe.QUIET_NANS) and not np.isnan(it.view(np.float32)).any()
    return fl, it, want, nan, (_row_status(fl, channels), _row_status(it, channels))


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("path", ["lanes", "wave"])
def test_every_encoding_packs_every_edge_value(pkg, monkeypatch, path, channels):
    """One bank of R channels, channel i in encoding ENC8[i % 8]; in block b (0..7) channel i is handed row (i + b) % R of its class's
    value set, so after eight blocks every encoding has packed every row.  No wavefront is all S16: every row leaves through demod_put."""
    monkeypatch.setenv("CHZ_DEMOD_WAVE", "1" if path == "wave" else "0")
    fl, it, want, nan, status_want = _edge_case(channels)
    R = len(fl)
    params = [pe.unit_gain_params(ol, channels, ENC8[i % 8], FS) for i in range(R)]
    is_float = np.array([ENC8[i % 8] in FLOAT_ENC for i in range(R)])
    seen = {enc: np.zeros(R, bool) for enc in ENC8}
    eng = pkg.engine.Engine(OVERLAP2[0], OVERLAP2[1], ol.REAL, ring_blocks=8)
    try:
        bank = _inject_bank(pkg, eng, N, params, BT)
        for b in range(8):
            idx = (np.arange(R) + b) % R
            bank.inject(b % 4, np.where(is_float[:, None], fl[idx], it[idx]), np.ones(R), np.full(R, 1e-12))
            bank.demod_only(b)
            pcm, status = bank.read_pcm(b % 4)
            for i in range(R):
                _check_status(status[i], status_want[0 if is_float[i] else 1][idx[i]], (b, i))
            for k, enc in enumerate(ENC8):
                ch = np.arange(k, R, 8)
                w = want[enc][idx[ch]]
                got = pcm[ch, :w.shape[1]]
                seen[enc][idx[ch]] = True
                if enc not in FLOAT_ENC:
                    assert np.array_equal(got, w), (b, enc, np.argwhere(got != w)[:4])
                    continue
                bps = w.shape[1] // (N * channels)
                got, w, m = got.reshape(len(ch), -1, bps), w.reshape(len(ch), -1, bps), nan[idx[ch]]
                assert np.array_equal(got[~m], w[~m]), (b, enc, np.argwhere((got != w).any(axis=2) & ~m)[:4])
                g = _decode(enc, got[m])                   # a NaN goes out as a NaN of the same sign; the payload is not compared
                x = np.stack([pe.packer_input(r, channels) for r in fl[idx[ch]]])[m]
                assert np.isnan(g).all() and np.array_equal(np.signbit(g), np.signbit(x)), (b, enc)
    finally:
        eng.close()
    assert all(s.all() for s in seen.values())


@functools.lru_cache(maxsize=None)
def _s16_case():
    it = pe.rows(pe.I16_VALUES, 1, N)
    nch = -(-len(it) // 128) * 128                         # an even number of groups of 64
    it = _pad_rows(it, nch)
    want = {enc: np.stack([pe.pack(ol, enc, pe.packer_input(r, 1)) for r in it]) for enc in (ol.PCM_S16LE, ol.PCM_S16BE)}
    return it, want, _row_status(it, 1)


def test_packed_s16_stores_equal_the_generic_store(pkg, monkeypatch):
    """Mono S16 only, groups of 64 channels alternately LE and BE, rows of 8192 bytes and blocks of 64 full tiles: demod_lin_lanes takes
    its packed 8-byte stores, which pack with demod_s16.  Two blocks, the rows moved on by 64 channels, hand every row to both
    encodings.  Then the same bank with rows of 2052 bytes (no multiple of 8: the generic store, demod_put's own S16 branch):
    against the restatement as well, so the bytes of the two stores are the same."""
    monkeypatch.setenv("CHZ_DEMOD_WAVE", "0")
    it, want, status_want = _s16_case()
    nch = len(it)
    encs = [ol.PCM_S16LE if (i // 64) % 2 == 0 else ol.PCM_S16BE for i in range(nch)]
    params = [pe.unit_gain_params(ol, 1, e, FS) for e in encs]
    eng = pkg.engine.Engine(OVERLAP2[0], OVERLAP2[1], ol.REAL, ring_blocks=8)
    try:
        first = None
        for stride in (8 * N, 2 * N + 4):
            assert (stride & 7 == 0) == (first is None)
            bank = _inject_bank(pkg, eng, N, params, BT, stride)
            blocks = []
            for b in range(2):
                idx = (np.arange(nch) + 64 * b) % nch
                bank.inject(b, it[idx], np.ones(nch), np.full(nch, 1e-12))
                bank.demod_only(b)
                pcm, status = bank.read_pcm(b)
                for i in range(nch):
                    _check_status(status[i], status_want[idx[i]], (stride, b, i))
                    w = want[encs[i]][idx[i]]
                    assert np.array_equal(pcm[i, :2 * N], w), (stride, b, i, np.flatnonzero(pcm[i, :2 * N] != w)[:4])
                blocks.append(pcm[:, :2 * N].copy())
            if first is None:
                first = blocks
            else:
                assert all(np.array_equal(a, c) for a, c in zip(first, blocks))
            bank.destroy()
    finally:
        eng.close()


FM_ENCODINGS = [ol.PCM_S16LE, ol.PCM_S16BE, ol.PCM_MULAW, ol.PCM_ALAW, ol.PCM_F16LE]


@functools.lru_cache(maxsize=None)
def _fm_case(encoding):
    """Channels 0, 1: the two clipping FM parameter sets in `encoding`; channels 2, 3: the same in F32LE (the mixed bank has them).
    The restated demodulator's frames for all four, and the share of its S16 samples (its G.711 codes) that sit at the clip."""
    nblk = pe.FM_CLIP_BLOCKS
    params, bbs, powers, ests = [], [], [], []
    for enc in (encoding, ol.PCM_F32LE):
        for j, kw in enumerate(pe.FM_CLIP_KW):
            bb, power, n0 = pe.fm_clip_case(7 + j)
            params.append(ol.fm_params(encoding=enc, samprate=pe.FM_CLIP_FS, **kw))
            bbs.append(bb); powers.append(power); ests.append(n0)
    want = _restated(params, [ol.FmDemod(p) for p in params], bbs, powers, ests, nblk, pe.FM_CLIP_BT)
    clipped = []
    for j, kw in enumerate(pe.FM_CLIP_KW):
        for enc in {ol.PCM_S16LE, encoding} - {ol.PCM_F16LE}:
            d = ol.FmDemod(ol.fm_params(encoding=enc, samprate=pe.FM_CLIP_FS, **kw))
            frames = [d.block(bbs[j][b], powers[j][b], ests[j][b], pe.FM_CLIP_BT)[0] for b in range(nblk)]
            frames = [f for f in frames if f is not None]
            assert len(frames) >= 8
            clipped.append(float(np.mean([pe.clipped_fraction(ol, enc, f) for f in frames])))
    return params, bbs, powers, ests, want, clipped


@pytest.mark.parametrize("encoding", FM_ENCODINGS, ids=["s16le", "s16be", "mulaw", "alaw", "f16le"])
@pytest.mark.parametrize("path", ["lanes", "wave"])
def test_fm_pcm_at_the_clip(pkg, monkeypatch, path, encoding):
    """FM audio driven beyond full scale (+6 dB of headroom with de-emphasis, 0 dB without: tests/pcm_edge_cases.py) against the
    restated FM demodulator, which tests/test_oracle_vs_reference.py pins to fm.c on this input, at the existing rule (_cmp_pcm: exact
    for S16, G.711 and binary16).  Twice: a bank of `encoding` alone -- for S16 demod_fm_lanes then packs with demod_s16 into 8-byte
    stores -- and a bank that holds F32LE channels too, whose rows all leave through demod_put.  Not vacuous: between 10 % and 90 % of
    the restatement's own S16 samples (G.711 codes) are at the clip."""
    monkeypatch.setenv("CHZ_DEMOD_WAVE", "1" if path == "wave" else "0")
    params, bbs, powers, ests, want, clipped = _fm_case(encoding)
    print("clipped share of the restatement's frames:", clipped)
    assert all(0.1 < c < 0.9 for c in clipped), clipped
    eng = pkg.engine.Engine(OVERLAP2[0], OVERLAP2[1], ol.REAL, ring_blocks=8)
    try:
        for nch in (2, 4):
            bank = _inject_bank(pkg, eng, pe.FM_CLIP_N, params[:nch], pe.FM_CLIP_BT)
            sent = 0
            for b in range(len(want)):
                _inject(bank, b, bbs[:nch], powers[:nch], ests[:nch])
                pcm, status = bank.read_pcm(b % 4)
                _compare_block(b, params[:nch], want[b][:nch], pcm, status, pe.FM_CLIP_N)
                sent += sum(s.frame == ol.FRAME_DATA for s in status)
            assert sent >= 8 * nch
            bank.destroy()
    finally:
        eng.close()
