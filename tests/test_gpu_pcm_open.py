"""The squelch-aware PCM read (chz_bank_read_pcm_open_async + chz_bank_pcm_open_wait, Bank.read_pcm_open; kernels pcm_open_count and
pcm_open_rows): of a range of channels only the OPEN ones' rows -- demodulator on, flag byte without NO_SAMPLES, MUTE and PENDING --
dense and in ascending channel order, with their channel numbers, the count and every channel's flag byte.

Reference: the existing read_pcm_flags on the same slot, the rows of the open channels picked on the host.  Everything is compared
byte for byte, the count exactly; no demodulator oracle is involved.  Banks are fed through inject() / demod_only() as in
tests/test_gpu_demod_shapes.py, 8 samples a block at 0.5 ms, so that the bb_power and n0 handed in per channel decide whose squelch
opens (SNR squelch, no tail: a channel is open in exactly the blocks whose power says so).  drive() asserts that read_pcm_flags shows
exactly the wanted pattern before the new call is used: the tests' input condition.

  ranges of 1, 63, 64, 65, T-1, T, T+1, 2T+37 channels at ch0 = 0 and 5, every pattern, rows of 16 / 20 / 64 bytes
                                                                   test_open_rows_of_every_range_and_pattern
  (16: one 16-byte word a row; 20: 4-byte words, rows aligned to 4 only; 64: four 16-byte words)
  demodulator-off channels (flag byte 0 from the allocation: "open" to anyone who does not look at the parameters) and FM channels
  muted by their tone squelch sit in every one of these banks
  stereo F32 and mu-law rows                                       test_open_rows_of_other_encodings
  a filter2 bank, blocking 4: pending blocks (count 0), firing     test_filter2_bank_pending_and_firing
  max_rows = count, count - 1, 0 with guard bytes; the slot's image afterwards
                                                                   test_max_rows_delivers_the_first_rows_only
  twelve blocks in the order async(j), wait(j-1)                   test_double_buffered_order_equals_one_at_a_time
  the slot demodulated again between the read and its wait         test_slot_demodulated_again_before_the_wait
  every refusal, each followed by a good read                      test_refusals_leave_the_state_alone
"""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as ol
from conftest import load_pkg

pytestmark = pytest.mark.gpu

MASTER = (11520, 11521)
OLEN, BT = 8, 0.0005
FS = OLEN / BT
T = 256                                  # PCMO_TILE of chz_kernels.h: channels a wavefront counts and scatters
RANGES = [1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 37]
CH0S = [0, 5]
NCH = 5 + 2 * T + 37 + 6                 # every range ends inside the bank
CLOSED = 1 | 2 | 16                      # FLAG_NO_SAMPLES | FLAG_MUTE | FLAG_PENDING
GUARD = 0xA5


@pytest.fixture(scope="module")
def pkg():
    p = load_pkg()
    if p.engine.lib().chz_device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests cannot run (there is no CPU fallback)")
    assert (p.engine.FLAG_NO_SAMPLES | p.engine.FLAG_MUTE | p.engine.FLAG_PENDING) == CLOSED
    L = p.engine.lib()
    vp, i = C.c_void_p, C.c_int
    L.chz_bank_read_pcm_open_async.argtypes = [vp, i, i, i, i, vp, vp, vp, i]
    L.chz_bank_pcm_open_wait.argtypes = [vp, i, i, C.POINTER(i)]
    L.chz_bank_read_pcm_flags_async.argtypes = [vp, i, i, i, i, vp, vp]
    L.chz_bank_pcm_wait.argtypes = [vp, i, i]
    return p


def _dparams(pkg, params):
    return [pkg.engine.DemodParams(*[getattr(p, f) for f, _ in ol.LinParams._fields_]) for p in params]


def _kinds(nch, extra=None):
    """lin / fm: SNR-squelched, open when the power says so; tone: FM behind a tone squelch that never hears its tone; off: no demodulator.
    The first channel of both ch0 and the last channel of every range can open."""
    k = np.array(["lin"] * nch, dtype=object)
    k[1::5] = "fm"
    k[3::11] = "off"
    k[7::37] = "tone"
    for c0 in CH0S:
        k[c0] = "lin"
        for n in RANGES:
            if c0 + n - 1 < nch:
                k[c0 + n - 1] = "lin"
    if extra:
        for c, v in extra.items():
            k[c] = v
    return k


def _params(kinds, lin_kw=None):
    out = []
    for k in kinds:
        if k == "off":
            out.append(ol.lin_params(channels=0, samprate=FS))
        elif k == "lin":
            out.append(ol.lin_params(samprate=FS, snr_squelch=True, squelch_tail=0, **(lin_kw or {})))
        else:
            enc = (lin_kw or {}).get("encoding", ol.PCM_S16BE)
            out.append(ol.fm_params(samprate=FS, bandwidth=8000.0, snr_squelch=True, squelch_tail=0, encoding=enc,
                                    tone_freq=100.0 if k == "tone" else 0.0))
    return out


def _bank(pkg, eng, kinds, stride, lin_kw=None):
    nch = len(kinds)
    P = OLEN * eng.N // eng.L
    bank = eng.bank(P, OLEN, nch)
    bank.set_responses(0, np.ones((nch, P), np.complex64) / P)
    bank.set_tuning(0, 0, np.full(nch, 2500, np.int32), np.zeros(nch))
    bank.set_active(nch); bank.enable_noise(50.0 * eng.L)
    bank.set_pcm_stride(stride)
    params = _params(kinds, lin_kw)
    bank.set_demod(0, 0, _dparams(pkg, params), BT)
    bank.demod_auto(False)
    bank.kinds = kinds
    bank.bw = np.array([p.bandwidth for p in params])
    bank.on = np.array([k != "off" for k in kinds])
    bank.can_open = np.array([k in ("lin", "fm") for k in kinds])
    return bank


def drive(bank, job, wanted):
    """Block `job` with the channels of `wanted` (bool [nch]) open and every other one closed: a tone of the channel's own frequency and
    phase (rows differ from channel to channel and from block to block), bb_power 20 dB above or 3 dB below the noise in the channel's
    bandwidth.  Returns read_pcm_flags' (pcm, flags) of the slot after asserting that they show exactly that pattern."""
    nch = len(bank.kinds)
    rng = np.random.default_rng(1000 + job)
    t = np.arange(OLEN)
    f = rng.uniform(-0.3, 0.3, nch)[:, None]; ph = rng.uniform(0, 2 * np.pi, nch)[:, None]
    x = (0.05 * np.exp(1j * (2 * np.pi * f * t + ph))).astype(np.complex64)
    n0 = np.full(nch, 1e-8 / FS)
    power = np.where(np.asarray(wanted, bool), 100.0, 0.5) * n0 * bank.bw
    bank.inject(job % 4, x, power, n0)
    bank.demod_only(job)
    pcm, fl = bank.read_pcm_flags(job % 4)
    is_open = (fl & CLOSED) == 0
    assert np.array_equal(is_open[bank.can_open], np.asarray(wanted, bool)[bank.can_open]), (job, np.flatnonzero(is_open != wanted)[:8])
    tone = bank.kinds == "tone"
    assert np.all(fl[tone & ~np.asarray(wanted, bool)] & CLOSED) and np.all((fl[tone & np.asarray(wanted, bool)] & 10) == 10), job   # MUTE + TONE_MUTE
    assert not fl[~bank.on].any(), job                   # the stale byte of a channel without a demodulator: it LOOKS open
    return pcm, fl


def reference(bank, pcm, fl, ch0, n):
    idx = np.array([c for c in range(ch0, ch0 + n) if bank.on[c] and not (fl[c] & CLOSED)], np.int32)
    return idx, pcm[idx], fl[ch0:ch0 + n]


def check_read(bank, slot, pcm, fl, ch0, n, tag):
    want_idx, want_rows, want_fl = reference(bank, pcm, fl, ch0, n)
    count, idx, rows, flags = bank.read_pcm_open(slot, ch0, n)
    assert count == len(want_idx), (tag, count, len(want_idx))
    assert idx.dtype == np.int32 and np.array_equal(idx, want_idx), tag
    assert rows.shape == want_rows.shape and np.array_equal(rows, want_rows), (tag, np.argwhere(rows != want_rows)[:4])
    assert np.array_equal(flags, want_fl), tag
    return count


def _patterns(nch):
    c = np.arange(nch)
    return {"none": np.zeros(nch, bool), "all": np.ones(nch, bool), "alternating": c % 2 == 0, "runs64+1": ((c + 1) // 64) % 2 == 0,
            "random": np.random.default_rng(99).random(nch) < 0.5}


@pytest.mark.parametrize("stride", [16, 20, 64])
def test_open_rows_of_every_range_and_pattern(pkg, stride):
    eng = pkg.engine.Engine(MASTER[0], MASTER[1], ol.REAL, ring_blocks=8)
    try:
        bank = _bank(pkg, eng, _kinds(NCH), stride)
        ranges = [(c0, n) for c0 in CH0S for n in RANGES]
        assert all(c0 + n <= NCH for c0, n in ranges)
        job, listed, closed = 0, 0, 0
        for name, wanted in _patterns(NCH).items():
            pcm, fl = drive(bank, job, wanted)
            for c0, n in ranges:
                k = check_read(bank, job % 4, pcm, fl, c0, n, (name, c0, n))
                listed += k; closed += n - k
                if name == "none":
                    assert k == 0
                if name == "all":
                    assert k == int(bank.can_open[c0:c0 + n].sum())
            job += 1
        for c0 in CH0S:                                  # only the first channel of the range open: one block serves every size
            w = np.zeros(NCH, bool); w[c0] = True
            pcm, fl = drive(bank, job, w)
            for n in RANGES:
                assert check_read(bank, job % 4, pcm, fl, c0, n, ("first", c0, n)) == 1
            job += 1
        for c0, n in ranges:                             # only the last: a block per range; the channel behind the range is open too
            w = np.zeros(NCH, bool); w[c0 + n - 1] = True; w[c0 + n] = True
            pcm, fl = drive(bank, job, w)
            assert check_read(bank, job % 4, pcm, fl, c0, n, ("last", c0, n)) == 1
            job += 1
        assert listed > 1000 and closed > 1000
    finally:
        eng.close()


@pytest.mark.parametrize("enc", ["f32-stereo", "mulaw"])
def test_open_rows_of_other_encodings(pkg, enc):
    """Stereo F32LE fills a 64-byte row to the last byte; mu-law leaves the second half of a 16-byte row as the allocation left it."""
    kw, stride = (dict(channels=2, encoding=ol.PCM_F32LE), 64) if enc == "f32-stereo" else (dict(encoding=ol.PCM_MULAW), 16)
    nch = T + 70
    kinds = _kinds(nch)
    if enc == "f32-stereo":
        kinds[kinds == "fm"] = "lin"; kinds[kinds == "tone"] = "off"       # (the FM demodulator is mono: its rows would be half empty)
    eng = pkg.engine.Engine(MASTER[0], MASTER[1], ol.REAL, ring_blocks=8)
    try:
        bank = _bank(pkg, eng, kinds, stride, kw)
        pats = _patterns(nch)
        for job, name in enumerate(["alternating", "random", "all"]):
            pcm, fl = drive(bank, job, pats[name])
            if enc == "f32-stereo" and name == "all":
                rows = pcm[bank.can_open].view("<f4")
                assert np.all(np.isfinite(rows)) and np.all(np.abs(rows).max(axis=1) > 0) and np.any(rows[:, 0::2] != rows[:, 1::2])
            for c0, n in [(0, nch), (5, T + 1), (5, 65)]:
                assert check_read(bank, job % 4, pcm, fl, c0, n, (enc, name, c0, n)) > 0
    finally:
        eng.close()


def test_filter2_bank_pending_and_firing(pkg):
    """filter2 with blocking 4 in front of the demodulators: blocks 0..2 and 4..6 are PENDING (every channel with a demodulator carries
    that flag alone: nothing is open), blocks 3 and 7 fire.  Some channels have no demodulator, some a squelch that cannot open."""
    Lm, Mm = MASTER
    nch, B = 70, 4
    rng = np.random.default_rng(5)
    t = np.arange(8 * Lm)
    ring = (0.05 * np.cos(2 * np.pi * (2500.3 / (Lm + Mm - 1)) * t) + 1e-4 * rng.standard_normal(8 * Lm)).astype(np.float32)
    eng = pkg.engine.Engine(Lm, Mm, ol.REAL, ring_blocks=8)
    try:
        eng.write(ring[:8 * Lm - (Mm - 1)]); eng.write(ring[8 * Lm - (Mm - 1):])
        P = OLEN * eng.N // eng.L
        bank = eng.bank(P, OLEN, nch)
        bank.set_responses(0, np.ones((nch, P), np.complex64) / P)
        bank.set_tuning(0, 0, np.full(nch, 2500, np.int32), np.zeros(nch))
        bank.set_active(nch); bank.enable_noise(50.0 * Lm)
        L2, M2, N2 = bank.set_filter2(0, B, 0)
        assert L2 == B * OLEN
        bank.set_filter2_responses(0, np.ones((nch, N2), np.complex64) / N2)
        bank.set_pcm_stride(2 * L2)
        kinds = np.array(["open"] * nch, dtype=object); kinds[2::9] = "off"; kinds[4::7] = "shut"
        params = [ol.lin_params(channels=0, samprate=FS) if k == "off" else
                  ol.lin_params(samprate=FS, snr_squelch=True, squelch_tail=0, squelch_open_db=150.0, squelch_close_db=149.0) if k == "shut" else
                  ol.lin_params(samprate=FS) for k in kinds]
        bank.set_demod(0, 0, _dparams(pkg, params), BT * B)
        bank.kinds = kinds; bank.on = kinds != "off"
        fired = 0
        for b in range(2 * B):
            eng.step(b)
            pcm, fl = bank.read_pcm_flags(b % 4)
            if (b + 1) % B:
                assert np.all(fl[bank.on] == pkg.engine.FLAG_PENDING) and not fl[~bank.on].any(), b
                for c0, n in [(0, nch), (5, 64)]:
                    assert check_read(bank, b % 4, pcm, fl, c0, n, ("pending", b, c0, n)) == 0
            else:
                assert np.all((fl[kinds == "open"] & CLOSED) == 0) and np.all(fl[kinds == "shut"] & CLOSED), (b, list(fl))
                for c0, n in [(0, nch), (5, 64), (5, 1)]:
                    assert check_read(bank, b % 4, pcm, fl, c0, n, ("firing", b, c0, n)) == int((kinds[c0:c0 + n] == "open").sum())
                fired += 1
        assert fired == 2
    finally:
        eng.close()


class OpenRead:
    """One chz_bank_read_pcm_open_async with buffers of its own: `extra` guard rows / entries behind max_rows, all of it pre-filled."""

    def __init__(self, pkg, eng, bank, slot, ch0, n, max_rows, extra=2, pcm_null=False, index_null=False):
        self.L, self.eng, self.bank, self.slot, self.max_rows = pkg.engine.lib(), eng, bank, slot, max_rows
        stride = self.L.chz_bank_pcm_stride(eng._h, bank.id)
        rows = max(max_rows, 0) + extra
        self.pcm = np.full((rows, stride), GUARD, np.uint8); self.idx = np.full(rows, -7, np.int32); self.fl = np.full(max(n, 0) + extra, GUARD, np.uint8)
        self.n = n
        self.rc = self.L.chz_bank_read_pcm_open_async(eng._h, bank.id, slot, ch0, n, None if pcm_null else self.pcm.ctypes.data,
                                                      None if index_null else self.idx.ctypes.data, self.fl.ctypes.data, max_rows)

    def wait(self):
        cnt = C.c_int(-1)
        assert self.L.chz_bank_pcm_open_wait(self.eng._h, self.bank.id, self.slot, C.byref(cnt)) == 0
        return cnt.value

    def untouched(self):
        return bool(np.all(self.pcm == GUARD) and np.all(self.idx == -7) and np.all(self.fl == GUARD))

    def check(self, count, want_idx, want_rows, want_fl, tag):
        k = min(count, self.max_rows)
        assert count == len(want_idx), (tag, count)
        assert np.array_equal(self.idx[:k], want_idx[:k]) and np.array_equal(self.pcm[:k], want_rows[:k]), tag
        assert np.all(self.idx[k:] == -7) and np.all(self.pcm[k:] == GUARD), tag           # nothing behind row min(count, max_rows)
        assert np.array_equal(self.fl[:self.n], want_fl) and np.all(self.fl[self.n:] == GUARD), tag


@pytest.mark.parametrize("stride", [16, 20])
def test_max_rows_delivers_the_first_rows_only(pkg, stride):
    nch = T + 70
    eng = pkg.engine.Engine(MASTER[0], MASTER[1], ol.REAL, ring_blocks=8)
    try:
        bank = _bank(pkg, eng, _kinds(nch), stride)
        pcm, fl = drive(bank, 0, _patterns(nch)["random"])
        for c0, n in [(0, nch), (5, T + 1)]:
            want = reference(bank, pcm, fl, c0, n)
            count = len(want[0])
            assert count > 64
            for max_rows in (count, count - 1, 0, count + 3):
                r = OpenRead(pkg, eng, bank, 0, c0, n, max_rows)
                assert r.rc == 0
                r.check(r.wait(), *want, (c0, n, max_rows))
            pcm2, fl2 = bank.read_pcm_flags(0)            # the slot's image is intact
            assert np.array_equal(pcm2, pcm) and np.array_equal(fl2, fl)
        # the existing calls on a slot with an open read outstanding keep their meaning
        r = OpenRead(pkg, eng, bank, 0, 0, nch, nch)
        assert r.rc == 0
        L = pkg.engine.lib()
        assert L.chz_bank_pcm_wait(eng._h, bank.id, 0) == 0
        assert r.untouched()                               # the first stage moves nothing to the host: everything arrives in the wait
        pcm3 = np.zeros_like(pcm); fl3 = np.zeros_like(fl)
        assert L.chz_bank_read_pcm_flags_async(eng._h, bank.id, 0, 0, nch, pcm3.ctypes.data, fl3.ctypes.data) == 0
        assert L.chz_bank_pcm_wait(eng._h, bank.id, 0) == 0
        assert np.array_equal(pcm3, pcm) and np.array_equal(fl3, fl)
        r.check(r.wait(), *reference(bank, pcm, fl, 0, nch), "after the existing calls")
    finally:
        eng.close()


def _twelve_patterns(nch):
    p = _patterns(nch)
    rng = np.random.default_rng(12)
    return [p["random"], p["alternating"], p["all"], p["runs64+1"], ~p["random"], p["none"], ~p["alternating"], ~p["runs64+1"]] + \
           [rng.random(nch) < q for q in (0.1, 0.9, 0.5, 0.3)]


def test_double_buffered_order_equals_one_at_a_time(pkg):
    """The host loop of a link-bound bank: block j's open read is issued, then block j-1's is waited for -- every slot is used three
    times, every block with another pattern.  The same twelve blocks run one at a time on a second engine, with read_pcm_flags of
    every block as the reference: counts, channel numbers, rows and flags agree bit for bit."""
    nch, nblk = T + 70, 12
    kinds, pats = _kinds(nch), _twelve_patterns(nch)
    eng_a = pkg.engine.Engine(MASTER[0], MASTER[1], ol.REAL, ring_blocks=8)
    eng_b = pkg.engine.Engine(MASTER[0], MASTER[1], ol.REAL, ring_blocks=8)
    try:
        a, b = _bank(pkg, eng_a, kinds, 16), _bank(pkg, eng_b, kinds, 16)
        want = []
        for j in range(nblk):                             # one at a time
            pcm, fl = drive(b, j, pats[j])
            want.append(reference(b, pcm, fl, 5, nch - 5))
            r = OpenRead(pkg, eng_b, b, j % 4, 5, nch - 5, nch)
            assert r.rc == 0
            r.check(r.wait(), *want[j], ("one at a time", j))
        assert len({len(w[0]) for w in want}) >= 8        # another pattern each block
        reads = []
        for j in range(nblk + 1):                         # async(j), wait(j - 1)
            if j < nblk:
                nchs = len(kinds)
                rng = np.random.default_rng(1000 + j)     # drive()'s block, without its reads
                t = np.arange(OLEN)
                f = rng.uniform(-0.3, 0.3, nchs)[:, None]; ph = rng.uniform(0, 2 * np.pi, nchs)[:, None]
                x = (0.05 * np.exp(1j * (2 * np.pi * f * t + ph))).astype(np.complex64)
                n0 = np.full(nchs, 1e-8 / FS)
                a.inject(j % 4, x, np.where(pats[j], 100.0, 0.5) * n0 * a.bw, n0)
                a.demod_only(j)
                reads.append(OpenRead(pkg, eng_a, a, j % 4, 5, nch - 5, nch))
                assert reads[j].rc == 0
            if j >= 1:
                reads[j - 1].check(reads[j - 1].wait(), *want[j - 1], ("double-buffered", j - 1))
    finally:
        eng_a.close(); eng_b.close()


def test_slot_demodulated_again_before_the_wait(pkg):
    """An open read is issued on slot 0, then the slot's next block is demodulated -- another pattern, other rows, other flags -- and only
    then is the read waited for: it delivers the block it was issued for (the kernels ran in front of the demodulator launch, and
    what they gathered, flag bytes included, lives in the read's own per-slot images)."""
    nch = T + 70
    eng = pkg.engine.Engine(MASTER[0], MASTER[1], ol.REAL, ring_blocks=8)
    try:
        bank = _bank(pkg, eng, _kinds(nch), 16)
        pats = _patterns(nch)
        pcm, fl = drive(bank, 0, pats["random"])
        want = reference(bank, pcm, fl, 5, nch - 5)
        r = OpenRead(pkg, eng, bank, 0, 5, nch - 5, nch)
        assert r.rc == 0
        pcm4, fl4 = drive(bank, 4, ~pats["random"])        # slot 0 again
        assert not np.array_equal(fl4, fl) and not np.array_equal(pcm4, pcm)
        r.check(r.wait(), *want, "block 0 after block 4")
        later = OpenRead(pkg, eng, bank, 0, 5, nch - 5, nch)
        assert later.rc == 0
        later.check(later.wait(), *reference(bank, pcm4, fl4, 5, nch - 5), "block 4")
    finally:
        eng.close()


def test_refusals_leave_the_state_alone(pkg):
    nch = 70
    eng = pkg.engine.Engine(MASTER[0], MASTER[1], ol.REAL, ring_blocks=8)
    L = pkg.engine.lib()
    try:
        bank = _bank(pkg, eng, _kinds(nch), 16)
        pcm, fl = drive(bank, 0, _patterns(nch)["alternating"])
        want = reference(bank, pcm, fl, 0, nch)

        def good(tag):
            r = OpenRead(pkg, eng, bank, 0, 0, nch, nch)
            assert r.rc == 0, (tag, L.chz_last_error())
            r.check(r.wait(), *want, tag)

        def refused(tag, **kw):
            args = dict(slot=0, ch0=0, n=nch, max_rows=nch)
            args.update(kw)
            r = OpenRead(pkg, eng, args.pop("bank", bank), **args)
            assert r.rc == -1 and L.chz_last_error(), tag
            assert r.untouched(), tag
            cnt = C.c_int(-1)                              # nothing was enqueued: there is nothing to wait for
            assert L.chz_bank_pcm_open_wait(eng._h, bank.id, max(0, min(3, args["slot"])), C.byref(cnt)) == -1 and cnt.value == -1, tag
            good(tag)

        plain = eng.bank(OLEN * eng.N // eng.L, OLEN, 8)           # a bank without demodulators
        refused("no demodulator", bank=plain, n=8, max_rows=8)
        cnt = C.c_int(-1)
        assert L.chz_bank_pcm_open_wait(eng._h, plain.id, 0, C.byref(cnt)) == -1
        refused("slot 4", slot=4)
        refused("slot -1", slot=-1)
        assert L.chz_bank_pcm_open_wait(eng._h, bank.id, 4, C.byref(cnt)) == -1 and L.chz_bank_pcm_open_wait(eng._h, bank.id, -1, C.byref(cnt)) == -1
        refused("range beyond the bank", ch0=5, n=nch - 4)
        refused("negative ch0", ch0=-1, n=4)
        refused("negative n", n=-1)
        refused("negative max_rows", max_rows=-1)
        refused("no row buffer", pcm_null=True)
        refused("no index buffer", index_null=True)
        assert L.chz_bank_pcm_open_wait(eng._h, bank.id, 0, C.byref(cnt)) == -1 and cnt.value == -1      # a wait with no read outstanding
        good("after a wait with nothing outstanding")
        # a second open read on a slot whose first was never waited for is refused, and the first arrives whole
        first = OpenRead(pkg, eng, bank, 0, 5, 33, 40)
        assert first.rc == 0
        second = OpenRead(pkg, eng, bank, 0, 0, nch, nch)
        assert second.rc == -1 and second.untouched()
        other = OpenRead(pkg, eng, bank, 1, 0, 0, 0, pcm_null=True, index_null=True)   # another slot is another matter; max_rows = 0 needs no buffers
        assert other.rc == 0 and other.wait() == 0
        first.check(first.wait(), *reference(bank, pcm, fl, 5, 33), "the first of two")
        assert second.untouched()
        zero = OpenRead(pkg, eng, bank, 0, 0, nch, 0, pcm_null=True, index_null=True)  # count and flags only
        assert zero.rc == 0
        zero.check(zero.wait(), *want, "max_rows = 0")
        good("at the end")
    finally:
        eng.close()
