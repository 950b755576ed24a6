#!/usr/bin/env python3
"""Time per poll of the wideband analyser bank (chz_welch_*) on the config-3 ring (129.6 MS/s real, 8 blocks in HBM), and beside it
the host time of the same work done the reference's way: one float32 transform per segment (numpy's pocketfft on float32 input), window
multiply and |X|^2 accumulation included.  Each size runs with the full-length complex transform and with the packed half-length real transform (option welch_packed).  Prints one JSON line per row.  Wall clock around poll + synchronous read, median of `reps`
after two warm-up polls; the ring holds noise written once."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge


def host_way(ring, end, fft_n, win, shift, bins, avg, overlap):
    adjust = int(np.rint(fft_n * (1 + (avg - 1) * (1 - overlap)))); hop = int(np.rint(fft_n * (1 - overlap)))
    out = np.zeros(bins, np.float32); gain = 2.0 / (avg * fft_n * fft_n); pos = end - adjust
    for _ in range(avg):
        X = np.fft.rfft(win * ring[pos:pos + fft_n])
        out[:bins // 2] += (gain * np.abs(X[shift:shift + bins // 2]) ** 2).astype(np.float32)
        out[bins // 2:] += (gain * np.abs(X[shift - (bins - bins // 2):shift]) ** 2).astype(np.float32)
        pos += hop
    return out


def main():
    pkg = ge.load()
    L, M = 2592000, 648001
    eng = pkg.engine.Engine(L, M, pkg.engine.REAL, ring_blocks=8)
    rng = np.random.default_rng(1)
    x = (0.1 * rng.standard_normal(8 * L)).astype(np.float32)
    for b in range(8):
        eng.write(x[b * L:(b + 1) * L])
    ring = np.roll(x, M - 1)
    for fft_n, avg, counts in ((6480, 8, (1, 64, 1024)), (129600, 4, (1, 64))):
        bins, shift, overlap = 1620, fft_n // 4, 0.5
        win = np.ones(fft_n, np.float32)
        for n, packed in [(n, p) for n in counts for p in (False, True)]:
            w = eng.welch(fft_n, n, bins, avg, packed=packed)
            for s in range(n):
                w.set_window(s, win); w.configure(s, shift, bins, avg, overlap)
            end = 5 * L
            ts = []
            for r in range(12):
                t0 = time.perf_counter(); w.poll(end=end); pkg.engine._check(pkg.engine.lib().chz_slot_sync(eng._h, -2)); ts.append(time.perf_counter() - t0)
            w.close()
            t0 = time.perf_counter(); host_way(ring, end, fft_n, win, shift, bins, avg, overlap); th = time.perf_counter() - t0
            t0 = time.perf_counter(); host_way(ring, end, fft_n, win, shift, bins, avg, overlap); th = min(th, time.perf_counter() - t0)
            print(json.dumps({"fft_n": fft_n, "fft_avg": avg, "analysers": n, "bins": bins, "device_poll_ms_median": round(1e3 * float(np.median(ts[2:])), 4),
                              "device_poll_ms_min": round(1e3 * min(ts[2:]), 4), "host_one_analyser_ms": round(1e3 * th, 4),
                              "host_all_analysers_ms": round(1e3 * th * n, 3), "packed_real_transform": packed}), flush=True)
    # config 3's forward transform block by block (one-block chz_run_blocks calls), without and with a 64-analyser poll issued behind every block
    w = eng.welch(6480, 64, 1620, 8)
    for s in range(64):
        w.set_window(s, np.ones(6480, np.float32)); w.configure(s, 1620, 1620, 8, 0.5)
    for with_poll in (False, True, False, True):
        eng.sync()
        t0 = time.perf_counter()
        for j in range(200):
            eng.run_blocks(j, 1)
            if with_poll:
                w.poll(end=5 * L)
        eng.sync(); pkg.engine._check(pkg.engine.lib().chz_slot_sync(eng._h, -2))
        print(json.dumps({"blocks": 200, "poll_64_analysers_every_block": with_poll, "wall_us_per_block": round(1e6 * (time.perf_counter() - t0) / 200, 2)}), flush=True)
    w.close()
    eng.close()


if __name__ == "__main__":
    main()
