#!/usr/bin/env python3
"""What one block of PL-tone sessions costs through the pooled CTCSS decoders (chz_ctcss_execute) and through the path without the pool
(chz_rmini_execute on ctcss's geometry for the filter, the 55 correlators on the host), on one MI355X at ctcss's documented shape
(24 kHz: L 4800, M 4801, N 9600, one COMPLEX slave of 100 samples, shift 60; 200 ms blocks).  The numbers of profiles/ctcss_pool.txt.

  ctcss_probe.py                  the table: for n = 1, 64 and 1024 sessions the wall time of one chz_ctcss_execute call (a host clock around a
                                  call that ends in a stream synchronise; samples from the host, no energies asked for), of one chz_rmini_execute
                                  call of the same n windows, and the bytes that cross the link per session and block, both ways; medians of
                                  interleaved runs after a warm-up
  ctcss_probe.py --kernel N       only chz_ctcss_execute, N sessions, 300 calls: the run to put under `rocprofv3 --kernel-trace --stats` for
                                  ctcss_ovs's own time
  ctcss_probe.py --kernel-rmini N    the same for chz_rmini_execute on the same master and slave, N windows: rmini_ovs's own time -- what is left of
                                  ctcss_ovs's is the sample conversion, the history hand-over and the correlators

Every session hears the same signal (the standard tones one after the other, three blocks each): a block's time does not depend on what the
sessions hear.  The host stage of the path without the pool -- 5500 double-precision complex steps per session and block -- is not timed
here: profiles/ctcss_pool.txt has the reference's own loop per block on one host core."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge      # noqa: E402
import afsk_oracle as ao          # noqa: E402  (sample packing only)
import ctcss_oracle as co         # noqa: E402  (signal generator and filter response only)

FS, CAP = 24000.0, 1024
G = co.geometry(FS)
L, M, N = G["L"], G["M"], G["N"]
WARM, REPS = int(os.environ.get("CTCSS_PROBE_WARM", "20")), int(os.environ.get("CTCSS_PROBE_REPS", "200"))
SIZES = (1, 64, 1024)


def median(v):
    return float(np.median(np.asarray(v[WARM:]))) * 1e6


def rmini_pool(E, n, resp):
    rp = E.RealMiniPool(L, M, [(co.OLEN, E.COMPLEX)], CAP)
    rinst = [rp.add() for _ in range(n)]
    for i in rinst:
        rp.set_response(i, 0, resp)
    return rp, rinst


def main():
    pkg = ge.load()
    E = pkg.engine
    resp = co.response(FS)
    if len(sys.argv) > 2 and sys.argv[1] == "--kernel-rmini":
        n = int(sys.argv[2])
        rp, rinst = rmini_pool(E, n, resp)
        win = (0.1 * np.random.default_rng(3).standard_normal((n, N))).astype(np.float32)
        shifts = np.full((n, 1), co.SHIFT, np.int32)
        for _ in range(300):
            rp.execute(rinst, win, shifts=shifts)
        print("kernel run: 300 calls of chz_rmini_execute, %d windows" % n)
        rp.close()
        return
    only = int(sys.argv[2]) if len(sys.argv) > 2 and sys.argv[1] == "--kernel" else None
    blocks = ao.to_wire(co.instance0(FS))
    pool = E.CtcssPool(FS, CAP)
    insts = [pool.add() for _ in range(only if only else sum(SIZES))]         # (the storage grows beyond `capacity`, the launch size)
    for i in insts:
        pool.set_response(i, resp)
    if only:
        found = 0
        for call in range(300):
            st = pool.execute(insts, [blocks[call % len(blocks)]] * only)
            found += st[0].tone_index >= 0
        print("kernel run: 300 calls of chz_ctcss_execute, %d sessions, session 0 named a tone in %d blocks" % (only, found))
        pool.close()
        return
    rp, rinst = rmini_pool(E, CAP, resp)
    win = np.zeros((CAP, N), np.float32)
    win[:, M - 1:] = ao.to_float(co.instance0(FS)[4])
    shifts = np.full((CAP, 1), co.SHIFT, np.int32)
    times, found = {}, 0
    steps = [(kind, n) for n in SIZES for kind in ("ctcss", "rmini")]
    mine = {1: insts[-1:], 64: insts[1024:1088], 1024: insts[:1024]}          # sessions of their own for every size: each hears the stream in order
    order = np.random.default_rng(2)
    for rep in range(WARM + REPS):
        for k in order.permutation(len(steps)):                 # a new order every repetition (scripts/wfm_probe.py has the reason)
            kind, n = steps[k]
            t0 = time.perf_counter()
            if kind == "ctcss":
                st = pool.execute(mine[n], [blocks[rep % len(blocks)]] * n)
                found += st[0].tone_index >= 0
            else:
                rp.execute(rinst[:n], win[:n], shifts=shifts[:n])
            times.setdefault((kind, n), []).append(time.perf_counter() - t0)
    assert found > 0
    print("# one 200 ms block of n PL-tone sessions at 24 kHz, medians of %d interleaved calls after %d, us of wall time per call" % (REPS, WARM))
    print("#     n  chz_ctcss_execute (samples from the host)   chz_rmini_execute alone (the filter of the path without the pool)   link bytes per session and block: pool down / up, without the pool down / up")
    for n in SIZES:
        print("  %5d  %10.1f   %10.1f   %d / %d (+ %d when the energies are asked for)   %d / %d" %
              (n, median(times[("ctcss", n)]), median(times[("rmini", n)]), 2 * L + 16, 16, 8 * G["ntones"], 4 * N + 160, 8 * co.OLEN))
    pool.close(); rp.close()


if __name__ == "__main__":
    main()
