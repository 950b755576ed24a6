#!/usr/bin/env python3
"""What one block of WFM channels costs through the pooled decoders (chz_wfm_execute, device source) and through the path it replaces
(chz_bank_read of the rows, the discriminator on the host, chz_rmini_execute on the wfm geometry, the stereo loop on the host), on one
MI355X at 20 ms blocks.  The numbers of profiles/wfm_pool.txt.

  wfm_probe.py                      the table: for n = 1, 16, 64 channels the wall time of one chz_wfm_execute call (a host clock around a
                                    call that ends in a stream synchronise) with the de-emphasis shared by 64 lanes and walked by one
                                    lane, and the wall time and link bytes of the replaced path; medians of interleaved runs after a warm-up
  wfm_probe.py --kernel N LANES     only chz_wfm_execute, N channels, LANES de-emphasis lanes, 300 calls: the run to put under
                                    `rocprofv3 --kernel-trace --stats` for wfm_ovs's own time

The host stages of the replaced path are numpy stand-ins for the reference's C loops (src/wfm.c:153-185,225-281); scipy's lfilter runs
the de-emphasis recurrences where scipy is installed, otherwise they are left out and the line says so."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge      # noqa: E402

FS, L, M = 2.592e6, 51840, 12961           # a 2.592 MS/s front end: N = 64,800, 40 Hz bins, 20 ms blocks (tests/mini_radiod_lib.WFM_GEOM)
P, OLEN, NCH, BW = 9600, 7680, 64, 220000.0
RATE75 = float(-np.expm1(-1.0 / (75e-6 * 48000.0)))
WARM, REPS = int(os.environ.get("WFM_PROBE_WARM", "20")), int(os.environ.get("WFM_PROBE_REPS", "200"))


def median(v):
    return float(np.median(np.asarray(v[WARM:]))) * 1e6


def main():
    pkg = ge.load()
    E, fa = pkg.engine, pkg.filterapi
    only = None
    if len(sys.argv) > 1 and sys.argv[1] == "--kernel":
        only = (int(sys.argv[2]), int(sys.argv[3]))
    N = L + M - 1
    # every channel listens to the same broadcast signal (the time of a block does not depend on what the channels hold, the branch taken does: stereo)
    nb = 3
    t = np.arange(nb * L) / FS
    mpx = 0.45 * np.sin(2 * np.pi * 1000.0 * t) + 0.09 * np.sin(2 * np.pi * 19000.0 * t) + 0.3 * np.sin(2 * np.pi * 1700.0 * t) * np.sin(2 * np.pi * 38000.0 * t)
    shift = 10000
    x = (0.05 * np.cos(2 * np.pi * shift * (FS / N) * t + 2 * np.pi * 75000.0 * np.cumsum(mpx) / FS) + 0.002 * np.random.default_rng(1).standard_normal(t.size)).astype(np.float32)
    eng = E.Engine(L, M, E.REAL)
    bank = eng.bank(P, OLEN, NCH)
    bank.set_responses(0, np.stack([fa.design_response(P, OLEN, N, True, -110000.0 / 384000.0, 110000.0 / 384000.0, 11.0)] * NCH))
    bank.set_active(NCH); bank.set_tuning(0, 0, np.full(NCH, shift, np.int32), np.zeros(NCH))
    for blk in range(nb):
        eng.write(x[blk * L:(blk + 1) * L]); eng.step(blk)
    slot = (nb - 1) % 4
    eng.slot_sync(slot)
    power = bank.read_power(slot)
    n0 = power / (101.0 * BW)
    base = bank.output_ptr(slot)
    ptrs = [base + 8 * OLEN * c for c in range(NCH)]
    resp = [fa.design_response(1920, 960, 15360, True, 50.0 / 48000, 15000.0 / 48000, 11.0, fa.REAL),      # src/wfm.c:75-89
            fa.design_response(1920, 960, 15360, True, -100.0 / 48000, 100.0 / 48000, 11.0), fa.design_response(1920, 960, 15360, True, -15000.0 / 48000, 15000.0 / 48000, 11.0)]
    pools = {}
    for lanes in ((only[1],) if only else (64, 1)):
        E._check(E.lib().chz_set_option(b"wfm_deemph_lanes", str(lanes).encode()))
        pool = E.WfmPool(0.02, NCH)
        E._check(E.lib().chz_set_option(b"wfm_deemph_lanes", None))
        insts = [pool.add() for _ in range(NCH)]
        for i in insts:
            pool.set_params(i, E.WfmParams(stereo_enable=1, encoding=E.PCM_S16BE, squelch_tail=1, squelch_open=10.0, squelch_close=4.0, bandwidth=BW,
                                           headroom=10 ** (-15 / 20), deemph_rate=RATE75, deemph_gain=1.0))
            for s in range(3):
                pool.set_response(i, s, resp[s])
        pools[lanes] = (pool, insts)
    if only:
        n, lanes = only
        pool, insts = pools[lanes]
        for _ in range(300):
            pcm, st = pool.execute(insts[:n], ptrs[:n], power[:n], n0[:n], on_device=True)
        print("kernel run: %d calls of chz_wfm_execute, %d channels, %d de-emphasis lanes, channels %d pilot %d" % (300, n, lanes, st[0].channels, st[0].pilot_present))
        return
    # the replaced path: rows to the host, discriminator, composite back to the device (rmini_ovs), three slaves back, stereo loop
    rp = E.RealMiniPool(7680, 7681, [(960, E.REAL), (960, E.COMPLEX), (960, E.COMPLEX)], NCH)
    rinst = [rp.add() for _ in range(NCH)]
    for i in rinst:
        for s in range(3):
            rp.set_response(i, s, resp[s])
    try:
        from scipy.signal import lfilter
    except Exception:
        lfilter = None
    shifts = np.tile(np.array([0, 760, 1520], np.int32), (NCH, 1))
    win = np.zeros((NCH, 15360), np.float32)
    gain = 2 * 10 ** (-15 / 20) * 384000.0 / BW

    def old_path(n):
        rows = bank.read(0, n)                                                        # n x 61,440 B down
        ph = (1.0 / np.pi) * np.arctan2(rows.imag, rows.real).astype(np.float64)      # cargf per sample
        d = np.diff(ph, axis=1, prepend=0.0)
        d = np.where(d > 1, d - 2, np.where(d < -1, d + 2, d)).astype(np.float32)
        _ = (d.sum(axis=1), d.max(axis=1), d.min(axis=1))                             # the statistics loop
        win[:n, :7680] = win[:n, 7680:]; win[:n, 7680:] = d
        mono, pilot, lmr = rp.execute(rinst[:n], win[:n], shifts[:n])                 # n x 61,440 B up, n x 19,200 B down
        p = pilot.astype(np.complex128)
        amp = (np.abs(pilot) ** 2).mean(axis=1)
        subc = p * p / np.maximum(np.abs(p) ** 2, 1e-300)
        info = 2.0 * (np.conj(subc) * lmr).imag
        s = (mono + info) + 1j * (mono - info)
        if lfilter is not None:
            s = lfilter([RATE75], [1.0, -(1.0 - RATE75)], s, axis=1)
        buf = (s * gain).astype(np.complex64)
        pcm = np.clip(np.rint(buf.view(np.float32) * 32768.0), -32767, 32767).astype(">i2")
        return pcm, amp

    times = {}
    steps = [(kind, n, lanes) for n in (1, 16, 64) for kind, lanes in (("wfm", 64), ("wfm", 1), ("old", 0))]
    order = np.random.default_rng(2)
    for rep in range(WARM + REPS):
        for k in order.permutation(len(steps)):                                       # a new order every repetition: no configuration always follows the same neighbour
            kind, n, lanes = steps[k]                                                 # (the device call right behind the replaced path's 10 ms of host work at 64 channels reads 16-27 ms)
            t0 = time.perf_counter()
            if kind == "wfm":
                pool, insts = pools[lanes]
                pcm, st = pool.execute(insts[:n], ptrs[:n], power[:n], n0[:n], on_device=True)
                times.setdefault(("wfm", n, lanes), []).append(time.perf_counter() - t0)
            else:
                old_path(n)
                times.setdefault(("old", n), []).append(time.perf_counter() - t0)
    assert st[0].frame == 0 and st[0].channels == 2 and st[0].pilot_present == 1
    print("# one 20 ms block of n WFM channels (stereo, S16, 75 us de-emphasis), medians of %d interleaved calls after %d, us of wall time per call" % (REPS, WARM))
    print("#   n  chz_wfm_execute, device source: de-emphasis on 64 lanes / on 1 lane   replaced path (bank read + host discriminator + chz_rmini_execute + host stereo loop%s)   link bytes new / replaced" % ("" if lfilter is not None else ", WITHOUT de-emphasis: no scipy"))
    for n in (1, 16, 64):
        new_b = n * (960 * 2 * 2 + 72 + 96)                                              # PCM row, status record, request record
        old_b = n * (7680 * 8 + 15360 * 4 + 960 * 4 + 2 * 960 * 8)
        print("  %3d  %9.1f / %9.1f   %10.1f   %8d / %9d" % (n, median(times[("wfm", n, 64)]), median(times[("wfm", n, 1)]), median(times[("old", n)]), new_b, old_b))
    for pool, _ in pools.values():
        pool.close()
    rp.close(); eng.close()


if __name__ == "__main__":
    main()
