"""filter2 resident on the device (chz_bank_set_filter2 & co., kernel f2_ovs): the channel's private second filter of downconvert()
(src/radio.c:1503-1513) as a stage of the block pipeline, between the channel kernel's rotated output and the demodulator.

The oracle chain is tests/oracle_lib.py's: Stream(L2, M2, COMPLEX).push(.., f64=True) fed the DEVICE's own first-filter rows
(Bank.read_slot), channel(.., isb=), set_filter, LinDemod / FmDemod fed the device's own filter2 output.  Bounds: the filter output
within 3e-6 relative L2 (the bound of test_gpu_pipeline.py's filter2 test for the same kernel arithmetic), bb_power within 1e-6 of the
float64 mean of the device's output, PCM / status with that test's tolerances (S16 identical, float 1e-6 of peak, gain 1e-9)."""
import numpy as np
import pytest

import oracle_lib as ol
from conftest import load_pkg
from test_kernels_emulated import _check_pcm

pytestmark = pytest.mark.gpu

L, M, FS = 25920, 6481, 1.296e6
N = L + M - 1
P, OLEN = 300, 240


@pytest.fixture(scope="module")
def pkg():
    p = load_pkg()
    if p.engine.lib().chz_device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests cannot run (there is no CPU fallback)")
    ol.build()
    return p


def am_signal(nblk, seed=31):
    """the amplitude-modulated carrier plus noise of test_gpu_pipeline.py's filter2 test"""
    rng = np.random.default_rng(seed)
    t = np.arange(nblk * L)
    return (0.05 * np.cos(2 * np.pi * (2500.3 / N) * t) * (1 + 0.4 * np.sin(2 * np.pi * 3e-4 * t)) + 1e-4 * rng.standard_normal(nblk * L)).astype(np.float32)


def fm_signal(nblk, seed=32):
    rng = np.random.default_rng(seed)
    t = np.arange(nblk * L)
    mod = (3000.0 / 1000.0) * np.cos(2 * np.pi * 1000.0 * t / FS)
    return (0.05 * np.cos(2 * np.pi * 300350.0 * t / FS - mod) + 4e-4 * rng.standard_normal(nblk * L)).astype(np.float32)


LIN4 = lambda: [ol.lin_params(), ol.lin_params(env=True, dc_alpha=0.002, encoding=ol.PCM_S16LE), ol.lin_params(channels=2, encoding=ol.PCM_F32LE),
                ol.lin_params(agc=False, gain_db=30.0)]
# shifts that are no multiple of the overlap factor 5, with a remainder: the rotator in front of filter2 is not the identity
SHIFTS4 = np.array([2501, 2499, 2502, 2498], np.int32)
FREQ4 = np.array([-7.0, 5.0, -11.0, 3.0]) / 12000.0


def to_dp(pkg, params):
    return [pkg.engine.DemodParams(*[getattr(p, f) for f, _ in ol.LinParams._fields_]) for p in params]


def first_bank(pkg, eng, nch, cap=None, shifts=None, freq=None, p=P, olen=OLEN, band=0.4):
    cap = cap or nch
    b = eng.bank(p, olen, cap)
    b.set_responses(0, np.stack([ol.set_filter(p, olen, N, True, -band, band, 9.0)] * cap).astype(np.complex64))
    sh = np.resize(SHIFTS4 if shifts is None else shifts, cap).astype(np.int32)
    fr = np.resize(FREQ4 if freq is None else freq, cap).astype(np.float64)
    b.set_tuning(0, 0, sh, fr); b.set_active(nch); b.enable_noise(FS)
    return b


def check_pcm(p, got, want, n, tag):
    nb = ol.pcm_bytes(p.encoding, n * p.channels)
    if p.encoding in (ol.PCM_S16BE, ol.PCM_S16LE):
        dt = ">i2" if p.encoding == ol.PCM_S16BE else "<i2"
        a, w = got[:nb].view(dt).astype(np.int32), want.view(dt).astype(np.int32)
        assert np.abs(a - w).max() <= 1 and np.mean(a != w) == 0, tag
    else:
        a, w = got[:nb].view("<f4").astype(np.float64), want.view("<f4").astype(np.float64)
        assert np.abs(a - w).max() <= 1e-6 * max(np.abs(w).max(), 1e-30), tag


class Chain:
    """One filter2 bank against the oracle, block after block.  resp2[i] None = the channel's filter2 response was never set."""

    def __init__(self, pkg, eng, bank, B, M2, resp2, isb=None, params=None, fm=False, exact_n0=False):
        self.pkg, self.eng, self.bank, self.B = pkg, eng, bank, B
        self.nch = len(resp2)
        self.L2, self.M2, self.N2 = bank.set_filter2(0, B, M2)
        assert bank.filter2_geometry() == (self.L2, self.M2, self.N2) and self.L2 == B * bank.olen
        self.resp2 = [None if r is None else np.asarray(r, np.complex64) for r in resp2]
        for i, r in enumerate(self.resp2):
            if r is not None:
                bank.set_filter2_responses(i, r)
        self.isb = np.zeros(self.nch, np.uint8) if isb is None else np.asarray(isb, np.uint8)
        if self.isb.any():
            bank.set_filter2_isb(0, self.isb)
        self.params = params
        if params is not None:
            bank.set_pcm_stride(8 * self.L2)
            bank.set_demod(0, 0, to_dp(pkg, params), 0.02)
            self.orc = [(ol.FmDemod if fm else ol.LinDemod)(p) for p in params]
        self.fm, self.exact_n0 = fm, exact_n0
        self.streams = [ol.Stream(self.L2, self.M2, ol.COMPLEX) for _ in range(self.nch)]
        self.pend = [[] for _ in range(self.nch)]
        self.last_power = np.zeros(self.nch)
        self.n0 = np.full(self.nch, np.nan)
        self.last_pcm = {}
        self.fired = 0
        self.frames = 0           # data frames held against the oracle's PCM
        self.worst = 0.0          # largest relative L2 error of a filter2 output so far

    def reset(self, job, ch0, n):
        self.bank.filter2_reset(job, ch0, n)
        for i in range(ch0, ch0 + n):
            self.streams[i] = ol.Stream(self.L2, self.M2, ol.COMPLEX)

    def swap(self, ch, resp):
        self.bank.set_filter2_responses(ch, resp)
        self.resp2[ch] = np.asarray(resp, np.complex64)

    def block(self, b, channels=None):
        """compare block b (already executed); channels: the sample of channels to hold against the oracle (default all)"""
        bank, s = self.bank, b % 4
        chans = range(self.nch) if channels is None else channels
        raw = bank.read_slot(s, 0, self.nch); power = bank.read_power(s, 0, self.nch)
        fire = (b + 1) % self.B == 0
        if self.params is not None:
            noise = bank.read_noise(s, 0, self.nch)
            self.n0 = np.where(np.isnan(self.n0), noise, self.n0 + 0.10 * (noise - self.n0))          # src/radio.c:1466-1473, every block
            pcm, status = bank.read_pcm(s, 0, self.nch)
            _, flags = bank.read_pcm_flags(s, 0, self.nch)
        for i in chans:
            self.pend[i].append(raw[i])
        if not fire:
            with pytest.raises(self.pkg.engine.ChzError):
                bank.read_filter2(s)
            assert np.array_equal(power, self.last_power), b                                          # the last firing block's, 0 before the first
            if self.params is not None:
                assert all(int(f) == self.pkg.engine.FLAG_PENDING for f in flags), (b, list(flags))
                assert all(status[i].frame == self.pkg.engine.FRAME_PENDING for i in range(self.nch)), b
                assert np.array_equal(pcm, self.last_pcm.get(s, np.zeros_like(pcm))), b               # PCM is left alone
                if self.exact_n0:
                    assert all(status[i].n0 == pytest.approx(self.n0[i], rel=1e-12) for i in range(self.nch)), b
            return
        self.fired += 1
        filt = bank.read_filter2(s, 0, self.nch)
        assert filt.shape == (self.nch, self.L2)
        for i in chans:
            x = np.concatenate(self.pend[i]); self.pend[i] = []
            if self.resp2[i] is None:
                assert not filt[i].any() and power[i] == 0.0, (b, i)                                  # a response never set: zeros
            else:
                want = ol.channel(self.streams[i].push(x, f64=True), ol.COMPLEX, self.N2, self.L2, 0, self.resp2[i], isb=bool(self.isb[i]))
                err = np.linalg.norm(filt[i] - want) / max(np.linalg.norm(want), 1e-12)
                self.worst = max(self.worst, err)
                assert err <= 3e-6, (b, i, err)
                assert np.linalg.norm(want) > 0
            assert power[i] == pytest.approx(np.mean(np.abs(filt[i].astype(np.complex128)) ** 2), rel=1e-6, abs=1e-300), (b, i)
        self.last_power = power.copy()
        if self.params is None:
            return
        self.last_pcm[s] = pcm.copy()
        for i in chans:
            p = self.params[i]
            want, st = self.orc[i].block(filt[i], power[i], noise[i], 0.02)
            got = status[i]
            assert (got.frame, got.mute, got.squelch_state) == (st.frame, st.mute, st.squelch_state), (b, i)
            assert int(flags[i]) == (st.frame & 1) | (st.mute & 1) << 1 | (st.pll_lock & 1) << 2 | (st.tone_mute & 1) << 3, (b, i)
            if self.exact_n0:
                assert got.n0 == pytest.approx(self.n0[i], rel=1e-12), (b, i)
            if self.fm:
                assert got.snr == pytest.approx(st.snr, rel=1e-5, abs=1e-9), (b, i)
                if st.frame == ol.FRAME_DATA:
                    assert got.output_power == pytest.approx(st.output_power, rel=4e-6), (b, i)
                    self.frames += 1
                    _check_pcm(p, pcm[i], want, self.L2, 8e-6)                                   # the existing FM chain test's comparison
                continue
            assert got.gain == pytest.approx(st.gain, rel=1e-9), (b, i)
            assert got.output_power == pytest.approx(st.output_power, rel=1e-6, abs=1e-300), (b, i)
            if st.frame == ol.FRAME_DATA:
                self.frames += 1
                check_pcm(p, pcm[i], want, self.L2, (b, i))


def lowpass(N2, L2, width=0.1, beta=7.0):
    return ol.set_filter(N2, L2, N2, False, -width, width, beta)


def test_b1_chain_next_to_a_plain_bank(pkg):
    """B = 1 (the isb preset's filter2 = 1): L2 = 240, N2 = 512.  14 blocks, the four lin_params variants, channel 2 an ISB channel,
    channel 3 without a filter2 response; a retune at block 7; a plain bank alongside; an execute_range re-run of a channel after block
    5 leaves the windows alone (the oracle's stream just goes on)."""
    nblk = 14
    x = am_signal(nblk)
    eng = pkg.engine.Engine(L, M, ol.REAL, ring_blocks=8)
    try:
        params = LIN4()
        f2b = first_bank(pkg, eng, 4)
        plain = first_bank(pkg, eng, 4)
        plain.set_pcm_stride(8 * OLEN); plain.set_demod(0, 0, to_dp(pkg, params), 0.02)
        r2 = lowpass(512, 240)
        ch = Chain(pkg, eng, f2b, 1, 0, [r2, r2, ol.set_filter(512, 240, 512, False, -0.2, 0.2, 7.0), None], isb=[0, 0, 1, 0], params=params)
        assert (ch.L2, ch.M2, ch.N2) == (240, 273, 512)
        o_plain = [ol.LinDemod(p) for p in params]
        for b in range(nblk):
            if b == 7:
                for bank in (f2b, plain):
                    bank.set_tuning(7, 0, SHIFTS4[::-1].copy(), FREQ4[::-1].copy())
            eng.write(x[b * L:(b + 1) * L]); eng.step(b)
            ch.block(b)
            if b == 5:
                f2b.execute_range(5, 1, 1)
            s = b % 4
            raw = plain.read_slot(s); pw = plain.read_power(s); ns = plain.read_noise(s); pcm, status = plain.read_pcm(s)
            for i, p in enumerate(params):
                want, st = o_plain[i].block(raw[i], pw[i], ns[i], 0.02)
                got = status[i]
                assert (got.frame, got.mute, got.squelch_state) == (st.frame, st.mute, st.squelch_state), (b, i)
                assert got.gain == pytest.approx(st.gain, rel=1e-9) and got.output_power == pytest.approx(st.output_power, rel=1e-6, abs=1e-300)
                if st.frame == ol.FRAME_DATA:
                    check_pcm(p, pcm[i], want, OLEN, (b, i))
        assert ch.fired == nblk and ch.frames >= 3 * (nblk - 2)
    finally:
        eng.close()


@pytest.mark.parametrize("B,geom", [(4, (960, 1089, 2048)), (3, (720, 1329, 2048))])
def test_blocking_cycles_with_pending_blocks(pkg, B, geom):
    """B = 4 (cwu / cwl: one slot fires) and B = 3 (every slot fires), 24 blocks: pending blocks carry flag 16, frame 2, untouched PCM
    and the repeated power; status.n0 follows the smoother over ALL blocks; PCM against LinDemod without AGC and SNR squelch."""
    nblk = 24
    x = am_signal(nblk)
    eng = pkg.engine.Engine(L, M, ol.REAL, ring_blocks=8)
    try:
        params = [ol.lin_params(agc=False, gain_db=30.0), ol.lin_params(agc=False, gain_db=40.0, encoding=ol.PCM_S16LE),
                  ol.lin_params(agc=False, gain_db=30.0, channels=2, encoding=ol.PCM_F32LE)]
        bank = first_bank(pkg, eng, 3)
        r2 = lowpass(geom[2], geom[0], 0.05)
        ch = Chain(pkg, eng, bank, B, 0, [r2] * 3, isb=[0, 0, 1], params=params, exact_n0=True)
        assert (ch.L2, ch.M2, ch.N2) == geom
        for b in range(nblk):
            eng.write(x[b * L:(b + 1) * L]); eng.step(b)
            ch.block(b)
        assert ch.fired == nblk // B and ch.frames >= 3 * (nblk // B - 1)
    finally:
        eng.close()


def test_fm_bank_behind_filter2(pkg):
    """one FM bank (olen 480, P 600, B = 1, N2 = 1024) against FmDemod"""
    nblk = 12
    x = fm_signal(nblk)
    eng = pkg.engine.Engine(L, M, ol.REAL, ring_blocks=8)
    try:
        params = [ol.fm_params(), ol.fm_params(deemph_tc=0.0)]
        bank = first_bank(pkg, eng, 2, shifts=np.array([7501, 7499], np.int32), freq=np.array([-3.0, 2.0]) / 24000.0, p=600, olen=480, band=8000 / 24000.0)
        r2 = ol.set_filter(1024, 480, 1024, False, -0.3, 0.3, 7.0)
        ch = Chain(pkg, eng, bank, 1, 0, [r2, r2], params=params, fm=True)
        assert (ch.L2, ch.M2, ch.N2) == (480, 545, 1024)
        for b in range(nblk):
            eng.write(x[b * L:(b + 1) * L]); eng.step(b)
            ch.block(b)
        assert ch.frames >= nblk
    finally:
        eng.close()


def test_an_odd_size_runs_radix_3_and_5(pkg):
    """M2 = 61: N2 = 300 = 4 * 3 * 5 * 5; filter output only, no demodulators"""
    x = am_signal(6)
    eng = pkg.engine.Engine(L, M, ol.REAL, ring_blocks=8)
    try:
        bank = first_bank(pkg, eng, 2)
        ch = Chain(pkg, eng, bank, 1, 61, [lowpass(300, 240), ol.set_filter(300, 240, 300, False, -0.3, 0.05, 5.0)])
        assert (ch.L2, ch.M2, ch.N2) == (240, 61, 300)
        for b in range(6):
            eng.write(x[b * L:(b + 1) * L]); eng.step(b)
            ch.block(b)
    finally:
        eng.close()


@pytest.mark.parametrize("B,M2,geom,nblk", [(1, 4, (240, 4, 243), 6), (3, 10, (720, 10, 729), 9)])
def test_an_odd_length_with_isb(pkg, B, M2, geom, nblk):
    """N2 = 243 = 3^5 (B = 1) and N2 = 729 = 3^6 (B = 3, with its pending blocks): an explicit M2 makes the filter2 transform odd, where
    the ISB unpack leaves the innermost pair (h, h + 1) of N2 = 2h + 1 alone (src/filter.c:899).  Three channels, the middle one ISB; the
    responses reach the Nyquist bins -- all-pass Kaiser on channel 0, random on the other two -- because that pair is where a wrong
    bound shows.  Filter output only."""
    x = am_signal(nblk)
    rng = np.random.default_rng(geom[2])
    eng = pkg.engine.Engine(L, M, ol.REAL, ring_blocks=8)
    try:
        bank = first_bank(pkg, eng, 3)
        rnd = (rng.standard_normal((2, geom[2])) + 1j * rng.standard_normal((2, geom[2]))).astype(np.complex64)
        ch = Chain(pkg, eng, bank, B, M2, [ol.set_filter(geom[2], geom[0], geom[2], False, -0.5, 0.5, 3.0), rnd[0], rnd[1]], isb=[0, 1, 0])
        assert (ch.L2, ch.M2, ch.N2) == geom and ch.N2 % 2 == 1
        for b in range(nblk):
            eng.write(x[b * L:(b + 1) * L]); eng.step(b)
            ch.block(b)
        assert ch.fired == nblk // B
        print("N2 %d: worst rel-L2 %.3g, %.3g of the bound" % (ch.N2, ch.worst, ch.worst / 3e-6))
    finally:
        eng.close()


def _snapshot(pkg, bank, slots):
    out = []
    for s in slots:
        try:
            f = bank.read_filter2(s).tobytes()
        except pkg.engine.ChzError:
            f = b"pending"
        pcm, status = bank.read_pcm(s)
        _, flags = bank.read_pcm_flags(s)
        out.append((f, bank.read_power(s).tobytes(), flags.tobytes(), bytes(status), pcm.tobytes()))
    return out


@pytest.mark.parametrize("B", [1, 3])
def test_blocks_in_flight_equal_blocks_stepped(pkg, B):
    """The same 24 blocks as 24 calls of chz_run_blocks(j, 1, 0) and as ONE chz_run_blocks(0, 24, 0), then one further cycle stepped in
    both: filter2 images, power, flags, status and PCM of the last four slots and of the extra cycle are byte-identical (the same
    kernel on the same data: any difference is an ordering fault)."""
    ring = am_signal(8, seed=5)
    runs = []
    for stepped in (True, False):
        eng = pkg.engine.Engine(L, M, ol.REAL, ring_blocks=8)
        try:
            eng.write(ring[:8 * L - (M - 1)]); eng.write(ring[8 * L - (M - 1):])
            bank = first_bank(pkg, eng, 4)
            L2, M2, N2 = bank.set_filter2(0, B, 0)
            bank.set_filter2_responses(0, np.stack([lowpass(N2, L2)] * 4)); bank.set_filter2_isb(0, np.array([0, 1, 0, 0], np.uint8))
            bank.set_pcm_stride(8 * L2); bank.set_demod(0, 0, to_dp(pkg, LIN4()), 0.02)
            if stepped:
                for j in range(24):
                    eng.run_blocks(j, 1)
            else:
                eng.run_blocks(0, 24)
            snap = _snapshot(pkg, bank, range(4))
            for j in range(24, 24 + B):
                eng.run_blocks(j, 1)
                snap += _snapshot(pkg, bank, [j % 4])
            runs.append(snap)
        finally:
            eng.close()
    assert any(r[0] != b"pending" for r in runs[0]) and any(np.frombuffer(r[4], np.uint8).any() for r in runs[0])
    assert runs[0] == runs[1]


def test_response_swap_and_reset_between_cycles(pkg):
    """B = 4: a response swap between two cycles and a filter2_reset at a cycle start, against the oracle with the same edits at the
    same blocks"""
    nblk = 20
    x = am_signal(nblk)
    eng = pkg.engine.Engine(L, M, ol.REAL, ring_blocks=8)
    try:
        bank = first_bank(pkg, eng, 3)
        r2 = lowpass(2048, 960, 0.05)
        ch = Chain(pkg, eng, bank, 4, 0, [r2] * 3)
        for b in range(nblk):
            if b == 8:
                ch.swap(1, ol.set_filter(2048, 960, 2048, False, -0.02, 0.08, 5.0))
            if b == 12:
                with pytest.raises(pkg.engine.ChzError):
                    bank.filter2_reset(13, 0, 2)                 # not a cycle start
                ch.reset(12, 0, 2)
            eng.write(x[b * L:(b + 1) * L]); eng.step(b)
            ch.block(b)
        assert ch.fired == 5
    finally:
        eng.close()


def test_grid_edges_257_channels_of_300(pkg):
    """257 active channels in a bank of capacity 300, B = 1, 6 blocks: 8 sampled channels (0, 255, 256 among them) against the
    oracle; the rows of channels >= 257 stay zero"""
    x = am_signal(6)
    eng = pkg.engine.Engine(L, M, ol.REAL, ring_blocks=8)
    try:
        nch, cap = 257, 300
        shifts = (2480 + np.arange(cap) % 41).astype(np.int32)
        bank = first_bank(pkg, eng, nch, cap=cap, shifts=shifts, freq=(np.arange(cap) % 7 - 3) / 12000.0)
        rs = [ol.set_filter(512, 240, 512, False, -0.05 - 0.001 * (i % 50), 0.05 + 0.002 * (i % 30), 7.0) for i in range(nch)]
        ch = Chain(pkg, eng, bank, 1, 0, rs)
        bank.set_filter2_responses(257, np.stack([rs[0]] * (cap - 257)))          # inactive channels have responses too: they must not run
        sample = [0, 1, 63, 64, 128, 255, 256, 200]
        for b in range(6):
            eng.write(x[b * L:(b + 1) * L]); eng.step(b)
            ch.block(b, sample)
            assert not bank.read_filter2(b % 4, 257, cap - 257).any()
    finally:
        eng.close()


def test_refusals(pkg):
    """each a return code and a message, nothing launched; chz_bank_filter2_check agrees with set_filter2 on every geometry"""
    E = pkg.engine
    eng = E.Engine(L, M, ol.REAL, ring_blocks=8)
    try:
        real = eng.bank(P, OLEN, 2, real=True)
        with pytest.raises(E.ChzError, match="COMPLEX"):
            real.set_filter2(0, 1)
        untuned = eng.bank(P, OLEN, 2)
        with pytest.raises(E.ChzError, match="chz_bank_set_tuning"):
            untuned.set_filter2(0, 1)
        for blocking, M2, ok in ((1, 0, True), (4, 0, True), (3, 0, True), (1, 61, True), (1, 8193 - 240 + 1, False), (1, 2 * 17 * 16 - 240 + 1, False),
                                 (0, 0, False), (1, -1, False), (40, 0, False), (1, 8192 - 240 + 1, True)):
            bank = first_bank(pkg, eng, 2)
            if ok:
                E.Bank.filter2_check(OLEN, blocking, M2)
                bank.set_filter2(0, blocking, M2)
            else:
                with pytest.raises(E.ChzError) as c1:
                    E.Bank.filter2_check(OLEN, blocking, M2)
                with pytest.raises(E.ChzError) as c2:
                    bank.set_filter2(0, blocking, M2)
                assert str(c1.value) == str(c2.value) and len(str(c1.value)) > 10
                with pytest.raises(E.ChzError, match="no filter2"):
                    bank.filter2_geometry()
            bank.destroy()
        late = first_bank(pkg, eng, 2)
        late.set_demod(0, 0, to_dp(pkg, LIN4()[:2]), 0.02)
        with pytest.raises(E.ChzError, match="before chz_bank_set_demod"):
            late.set_filter2(0, 1)
        bank = first_bank(pkg, eng, 2)
        assert bank.set_filter2(0, 4) == (960, 1089, 2048)
        for stride in (956, 8 * 960 + 4):
            with pytest.raises(E.ChzError, match="PCM rows hold 960..7680"):
                bank.set_pcm_stride(stride)
        bank.set_pcm_stride(960 * 2)
        with pytest.raises(E.ChzError, match="eager mode"):
            eng.run_blocks(0, 8, graph=True)
        with pytest.raises(E.ChzError, match="starts a cycle"):
            bank.filter2_reset(2, 0, 2)
        with pytest.raises(E.ChzError, match="pending"):
            bank.read_filter2(0)
        x = am_signal(1)
        eng.write(x); eng.step(0)                                   # block 0 of a cycle of four: pending
        with pytest.raises(E.ChzError, match="pending"):
            bank.read_filter2(0)
        assert not bank.read_power(0).any()
    finally:
        eng.close()
