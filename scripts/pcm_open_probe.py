#!/usr/bin/env python3
"""What the squelch-aware PCM read (chz_bank_read_pcm_open_async + chz_bank_pcm_open_wait) saves on the host link of one MI355X: the
numbers of profiles/pcm_open.txt.

The double-buffered loop of bench.py's c_rt_pcie leg on the same bank recipe -- config 3's tiled plan, tuning, noise estimate, linear
demodulators, mono S16BE in rows of 2 * olen bytes, 1.32 M channels: block j is handed to the device and its read issued, then the host
waits for block j-1's.  Every channel gets an SNR squelch that is either always open (thresholds below any SNR) or never (above any),
so that a chosen fraction of the channels is open; the fraction achieved is read back from the flag bytes.  For each fraction the
same process runs, on the same bank, first the existing path (chz_bank_read_pcm_flags_async + chz_bank_pcm_wait: every row, every
block) and then the new one; 200 blocks after 8 of warm-up each.  Reported: mean, p99 and worst time between two completions, D2H bytes
per block (new path: n flag bytes + 4 for the count + count * (stride + 4)), the two kernels' own times (chz_bank_pcm_open_times), and
after each run of the new path its last block against read_pcm_flags of the same slot, byte for byte.

The last three columns say where the host spent a block's time: in chz_input_write + chz_step, in issuing the read, in the wait.

  pcm_open_probe.py [channels [blocks [fractions]]]        defaults 1320960 200 0,0.01,0.1,0.5,1
"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FRACTIONS = [0.0, 0.01, 0.10, 0.50, 1.0]
WARM = 8
CLOSED = 1 | 2 | 16


def main():
    import bench
    import __graft_entry__ as ge
    pkg = ge.load()
    lib = pkg.engine.lib()
    nch = int(sys.argv[1]) if len(sys.argv) > 1 else 1_320_960
    blocks = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    fractions = [float(v) for v in sys.argv[3].split(",")] if len(sys.argv) > 3 else FRACTIONS
    wl = bench.workload_for(3, 0, 1, 1024)
    Lw, P, olen, tile = wl["L"], wl["P"], wl["olen"], 3072
    nch -= nch % tile
    stride = 2 * olen
    vp, ci = C.c_void_p, C.c_int
    lib.chz_host_alloc.argtypes = [C.POINTER(vp), C.c_size_t]
    lib.chz_bank_read_pcm_flags_async.argtypes = [vp, ci, ci, ci, ci, vp, vp]
    lib.chz_bank_pcm_wait.argtypes = [vp, ci, ci]
    lib.chz_bank_read_pcm_open_async.argtypes = [vp, ci, ci, ci, ci, vp, vp, vp, ci]
    lib.chz_bank_pcm_open_wait.argtypes = [vp, ci, ci, C.POINTER(ci)]
    lib.chz_bank_pcm_open_times.argtypes = [vp, ci, ci, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    eng = pkg.engine.Engine(wl["L"], wl["M"], pkg.engine.REAL, device=0, ring_blocks=bench.RING_BLOCKS)
    try:
        def pinned(nbytes):
            p = vp()
            assert lib.chz_host_alloc(C.byref(p), nbytes) == 0
            return p
        hin = pinned(4 * Lw)
        houts, hidx, hfls = [pinned(stride * nch) for _ in range(2)], [pinned(4 * nch) for _ in range(2)], [pinned(nch) for _ in range(2)]
        np.ctypeslib.as_array(C.cast(hin, C.POINTER(C.c_float)), shape=(Lw,))[:] = bench.comb_ring(wl)[:Lw]
        bank = eng.bank(P, olen, nch)
        plan = bench.channel_plan_config3(tile)
        resp = np.stack([pkg.filterapi.design_response(P, olen, wl["N"], True, lo, hi, 11.0) for _, lo, hi in plan[:3]])
        resp = np.ascontiguousarray(np.tile(resp, (tile // 3, 1)))
        shifts = np.array([p[0] for p in plan], np.int32)
        for c0 in range(0, nch, tile):
            bank.set_responses(c0, resp); bank.set_shifts(c0, shifts + (c0 // tile) % 7)
        eng.set_notches([0], 0.01)
        for c0 in range(0, nch, tile):
            bank.set_tuning(0, c0, shifts + (c0 // tile) % 7, np.full(tile, -3.3 / 12000.0))
        bank.enable_noise(wl["fs"])
        bank.set_pcm_stride(stride)
        v = lambda db: 10 ** (db / 20.0)

        def params(open_):
            return pkg.engine.DemodParams(channels=1, env=0, agc=1, encoding=pkg.engine.PCM_S16BE, snr_squelch=1, squelch_tail=0, tuned=1, kind=0,
                                          samprate=12000.0, headroom=v(-15.0), threshold=v(-15.0), recovery_rate=v(20.0), hangtime=1.1, dc_alpha=0.0,
                                          bandwidth=2950.0, shift=0.0, squelch_open=-2.0 if open_ else 1e30, squelch_close=-3.0 if open_ else 1e29,
                                          gain=v(50.0))
        p_open, p_shut = params(True), params(False)
        bank.set_active(nch)
        job = 0
        rng = np.random.default_rng(7)
        print("squelch-aware PCM read against the full read: %d channels, mono S16BE, rows of %d bytes, double-buffered loop, %d blocks after %d"
              % (nch, stride, blocks, WARM))
        print("%-8s %-9s %-5s %9s %9s %9s %14s %10s %10s %8s %8s %8s" % ("wanted", "achieved", "path", "mean ms", "p99 ms", "worst ms", "D2H B/block", "count us", "rows us",
                                                                        "step ms", "issue ms", "wait ms"))
        for frac in fractions:
            mask = rng.random(nch) < frac if 0.0 < frac < 1.0 else np.full(nch, frac >= 1.0)
            for c0 in range(0, nch, 65536):
                bank.set_demod(job, c0, [p_open if m else p_shut for m in mask[c0:c0 + 65536]], bench.BLOCKTIME)
            for path in ("full", "open"):
                times, last_done, d2h, kc, kr = [], None, [], [], []
                host = np.zeros(3)
                cnt = ci(0)
                lib.chz_bank_pcm_open_times(eng._h, bank.id, 0, None, None)        # (turns the kernels' timing on)
                for i in range(blocks + WARM + 1):
                    j = job + i
                    t0 = time.perf_counter()
                    if i < blocks + WARM:
                        assert lib.chz_input_write(eng._h, hin, Lw) == 0
                        assert lib.chz_step(eng._h, j) == 0
                        t1 = time.perf_counter()
                        if path == "full":
                            assert lib.chz_bank_read_pcm_flags_async(eng._h, bank.id, j % 4, 0, nch, houts[j % 2], hfls[j % 2]) == 0
                        else:
                            assert lib.chz_bank_read_pcm_open_async(eng._h, bank.id, j % 4, 0, nch, houts[j % 2], hidx[j % 2], hfls[j % 2], nch) == 0
                    t2 = time.perf_counter()
                    if i >= 1:
                        if path == "full":
                            assert lib.chz_bank_pcm_wait(eng._h, bank.id, (j - 1) % 4) == 0
                        else:
                            assert lib.chz_bank_pcm_open_wait(eng._h, bank.id, (j - 1) % 4, C.byref(cnt)) == 0
                        now = time.perf_counter()
                        if WARM < i < blocks + WARM:
                            host += (t1 - t0, t2 - t1, now - t2)
                        if i - 1 >= WARM:
                            times.append((now - last_done) * 1e3)
                            if path == "open":
                                d2h.append(nch + 4 + cnt.value * (stride + 4))
                                a, b = C.c_double(0), C.c_double(0)
                                if lib.chz_bank_pcm_open_times(eng._h, bank.id, (j - 1) % 4, C.byref(a), C.byref(b)) == 0:
                                    kc.append(a.value * 1e3); kr.append(b.value * 1e3)
                        last_done = now
                eng.sync()
                jl = job + blocks + WARM - 1                                        # the last block: whose flags say what fraction is open
                fl = np.ctypeslib.as_array(C.cast(hfls[jl % 2], C.POINTER(C.c_ubyte)), shape=(nch,)).copy()
                achieved = float(np.mean((fl & CLOSED) == 0))
                if path == "open":
                    k = cnt.value
                    idx = np.ctypeslib.as_array(C.cast(hidx[jl % 2], C.POINTER(C.c_int)), shape=(nch,))[:k].copy()
                    rows = np.ctypeslib.as_array(C.cast(houts[jl % 2], C.POINTER(C.c_ubyte)), shape=(nch, stride))[:k].copy()
                    assert lib.chz_bank_read_pcm_flags_async(eng._h, bank.id, jl % 4, 0, nch, houts[(jl + 1) % 2], hfls[(jl + 1) % 2]) == 0
                    assert lib.chz_bank_pcm_wait(eng._h, bank.id, jl % 4) == 0
                    full = np.ctypeslib.as_array(C.cast(houts[(jl + 1) % 2], C.POINTER(C.c_ubyte)), shape=(nch, stride))
                    fl2 = np.ctypeslib.as_array(C.cast(hfls[(jl + 1) % 2], C.POINTER(C.c_ubyte)), shape=(nch,))
                    want = np.flatnonzero((fl2 & CLOSED) == 0)
                    assert np.array_equal(fl, fl2) and np.array_equal(idx, want) and np.array_equal(rows, full[want]), "open read differs from the full read"
                t = np.array(times)
                host *= 1e3 / (blocks - 1)
                print("%-8s %-9s %-5s %9.3f %9.3f %9.3f %14d %10s %10s %8.3f %8.3f %8.3f" % (
                    "%g %%" % (100 * frac), "%.2f %%" % (100 * achieved), path, t.mean(), np.percentile(t, 99), t.max(),
                    nch * (stride + 1) if path == "full" else int(np.mean(d2h)),
                    "%.1f" % np.mean(kc) if kc else "-", "%.1f" % np.mean(kr) if kr else "-", host[0], host[1], host[2]))
                sys.stdout.flush()
                job += blocks + WARM
        print("new path, every run: last block's count, channel numbers, rows and flags equal to read_pcm_flags of the same slot")
    finally:
        eng.close()


if __name__ == "__main__":
    main()
