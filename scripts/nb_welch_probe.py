#!/usr/bin/env python3
"""What the narrowband analyser (chz_bank_welch_*) costs on config 3 (129.6 MS/s real, 1024 channels of P = 300 / olen = 240):
  appends -- device time per block of chz_run_blocks (chz_timing.total_ms: the span between the lanes' first begin event and last end event, measured
             by the device's own event timestamps, over 200 blocks) with 0, 16 and 256 analysers attached to the bank (each launch of bb_ring_append
             copies one 240-sample row per analyser behind the channel kernel), three runs each, interleaved;
  polls   -- wall time of one poll of 256 analysers at fft_n = 1024 and 16,384 with fft_avg = 8, overlap 0.5, every bin read
             (poll + wait on the polls' stream), median and minimum of 10 after two warm-up polls.
Prints one JSON line per row."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge


def main():
    pkg = ge.load()
    L, M, nch, P, olen = 2592000, 648001, 1024, 300, 240
    N = L + M - 1
    eng = pkg.engine.Engine(L, M, pkg.engine.REAL, ring_blocks=8)
    rng = np.random.default_rng(1)
    x = (0.1 * rng.standard_normal(8 * L)).astype(np.float32)
    for b in range(8):
        eng.write(x[b * L:(b + 1) * L])
    bank = eng.bank(P, olen, nch)
    bank.set_responses(0, ((rng.standard_normal((nch, P)) + 1j * rng.standard_normal((nch, P))) / P).astype(np.complex64))
    bank.set_shifts(0, (1000 + 300 * np.arange(nch)).astype(np.int32))
    bank.set_active(nch)
    sync_welch = lambda: pkg.engine._check(pkg.engine.lib().chz_slot_sync(eng._h, -2))
    job = 0
    eng.run_blocks(job, 16); job += 16                                                # warm-up; starts the issuing threads
    blocks = 200
    for rep in range(3):
        for attached in (0, 16, 256):
            sp = None
            if attached:
                sp = bank.spectrum(1024, attached, 1024, 8)
                for s in range(attached):
                    sp.attach(s, (s * 4) % nch, job)
            eng.run_blocks(job, 8); job += 8
            t = eng.run_blocks(job, blocks); job += blocks
            print(json.dumps({"what": "appends", "run": rep, "analysers_attached": attached, "blocks": blocks,
                              "device_us_per_block": round(1e3 * t.total_ms / blocks, 2)}), flush=True)
            if sp:
                sp.close()
    for fft_n in (1024, 16384):
        n, avg = 256, 8
        sp = bank.spectrum(fft_n, n, fft_n, avg)
        win = np.ones(fft_n, np.float32)
        for s in range(n):
            sp.attach(s, (s * 4) % nch, job); sp.set_window(s, win); sp.configure(s, fft_n, avg, 0.5)
        eng.run_blocks(job, 8); job += 8
        ts = []
        for r in range(12):
            t0 = time.perf_counter(); sp.poll(job=job - 1); sync_welch(); ts.append(time.perf_counter() - t0)
        print(json.dumps({"what": "poll", "fft_n": fft_n, "fft_avg": avg, "analysers": n, "bins": fft_n,
                          "poll_ms_median": round(1e3 * float(np.median(ts[2:])), 4), "poll_ms_min": round(1e3 * min(ts[2:]), 4)}), flush=True)
        sp.close()
    eng.close()


if __name__ == "__main__":
    main()
