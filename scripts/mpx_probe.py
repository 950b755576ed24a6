#!/usr/bin/env python3
"""What one block of FM-multiplex sessions costs through the pooled decoders (chz_mpx_execute) and through the path without the pool
(chz_rmini_execute on stereod's geometry for the filter, the stereo matrix, de-emphasis and packer on the host), on one MI355X at stereod's
own shape (5 ms: L 1920, M 1921, N 3840, a REAL and two COMPLEX slaves of 240 samples, shifts 0 / 190 / 380).  The numbers of
profiles/mpx_pool.txt.

  mpx_probe.py [--lanes K]        the table: for n = 1, 64 and 1024 sessions the wall time of one chz_mpx_execute call (a host clock around a
                                  call that ends in a stream synchronise; samples from the host, no floats asked for), of one chz_rmini_execute
                                  call of the same n windows, and the bytes that cross the link per session and block, both ways; medians of
                                  interleaved runs after a warm-up
  mpx_probe.py --kernel N [--lanes K] [--rds]
                                  only chz_mpx_execute, N sessions, 300 calls: the run to put under `rocprofv3 --kernel-trace --stats` for
                                  mpx_ovs's own time
  mpx_probe.py --kernel-rmini N   the same for chz_rmini_execute on the same master and slaves, N windows: rmini_ovs's own time -- what is left
                                  of mpx_ovs's is the sample conversion, the history hand-over, the matrix, the recurrences and the packer

--lanes K sets option mpx_deemph_lanes before the pool is created: 64 (the default) lanes share a block's two de-emphasis recurrences as an
affine scan, 1 walks them on one lane in the reference's order.  Every session hears the same signal: a block's time does not depend on
what the sessions hear.  The host stage of the path without the pool -- 240 double-precision matrix and de-emphasis steps per session
and block -- is not timed here: profiles/mpx_pool.txt has the reference's own loop per block on one host core."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge      # noqa: E402
import afsk_oracle as ao          # noqa: E402  (sample packing only)
import mpx_oracle as mo           # noqa: E402  (signal generator and filter responses only)

BT, CAP = 0.005, 1024
G = mo.geometry(BT)
L, M, N, OLEN = G["L"], G["M"], G["N"], G["olen"]
WARM, REPS = int(os.environ.get("MPX_PROBE_WARM", "20")), int(os.environ.get("MPX_PROBE_REPS", "200"))
SIZES = (1, 64, 1024)
NBLOCKS = 16


def median(v):
    return float(np.median(np.asarray(v[WARM:]))) * 1e6


def rmini_pool(E, n, resp):
    rp = E.RealMiniPool(L, M, [(OLEN, E.REAL), (OLEN, E.COMPLEX), (OLEN, E.COMPLEX)], CAP)
    rinst = [rp.add() for _ in range(n)]
    for i in rinst:
        for s in range(3):
            rp.set_response(i, s, resp[s])
    return rp, rinst


def mpx_pool(E, n, kind):
    pool = E.MpxPool(BT, CAP, kind=kind)
    insts = [pool.add() for _ in range(n)]                                  # (the storage grows beyond `capacity`, the launch size)
    for i in insts:
        for s, r in enumerate(mo.responses(BT, kind)):
            pool.set_response(i, s, r)
    return pool, insts


def main():
    args = sys.argv[1:]
    lanes = None
    if "--lanes" in args:
        lanes = int(args[args.index("--lanes") + 1])
        del args[args.index("--lanes"):args.index("--lanes") + 2]
    rds = "--rds" in args
    if rds:
        args.remove("--rds")
    pkg = ge.load()
    E = pkg.engine
    if lanes is not None:
        E._check(E.lib().chz_set_option(b"mpx_deemph_lanes", str(lanes).encode()))
    resp = mo.responses(BT)
    shifts3 = [0, G["pilot_shift"], G["subc_shift"]]
    if len(args) > 1 and args[0] == "--kernel-rmini":
        n = int(args[1])
        rp, rinst = rmini_pool(E, n, resp)
        win = (0.1 * np.random.default_rng(3).standard_normal((n, N))).astype(np.float32)
        shifts = np.tile(np.array(shifts3, np.int32), (n, 1))
        for _ in range(300):
            rp.execute(rinst, win, shifts=shifts)
        print("kernel run: 300 calls of chz_rmini_execute, %d windows" % n)
        rp.close()
        return
    only = int(args[1]) if len(args) > 1 and args[0] == "--kernel" else None
    blocks = ao.to_wire(mo.signal(NBLOCKS, BT, 1, 0.2, rds=rds))
    if only:
        pool, insts = mpx_pool(E, only, E.MPX_RDS if rds else E.MPX_STEREO)
        loud = 0
        for call in range(300):
            pcm, _, _ = pool.execute(insts, [blocks[call % NBLOCKS]] * only)
            loud += bool(pcm[0].any())
        print("kernel run: 300 calls of chz_mpx_execute (%s, %s de-emphasis lanes), %d sessions, session 0 sent sound in %d blocks"
              % ("RDS" if rds else "STEREO", lanes if lanes is not None else "default", only, loud))
        pool.close()
        return
    pool, insts = mpx_pool(E, sum(SIZES), E.MPX_STEREO)
    rp, rinst = rmini_pool(E, CAP, resp)
    win = np.zeros((CAP, N), np.float32)
    win[:, M - 1:] = mo.to_float(mo.signal(NBLOCKS, BT, 1, 0.2)[4], mo.STEREO)
    shifts = np.tile(np.array(shifts3, np.int32), (CAP, 1))
    times, loud = {}, 0
    steps = [(kind, n) for n in SIZES for kind in ("mpx", "rmini")]
    mine = {1: insts[-1:], 64: insts[1024:1088], 1024: insts[:1024]}          # sessions of their own for every size: each hears the stream in order
    order = np.random.default_rng(2)
    for rep in range(WARM + REPS):
        for k in order.permutation(len(steps)):                 # a new order every repetition (scripts/wfm_probe.py has the reason)
            kind, n = steps[k]
            t0 = time.perf_counter()
            if kind == "mpx":
                pcm, _, _ = pool.execute(mine[n], [blocks[rep % NBLOCKS]] * n)
                loud += bool(pcm[0].any())
            else:
                rp.execute(rinst[:n], win[:n], shifts=shifts[:n])
            times.setdefault((kind, n), []).append(time.perf_counter() - t0)
    assert loud > 0
    print("# one 5 ms block of n stereo sessions, %s de-emphasis lanes, medians of %d interleaved calls after %d, us of wall time per call"
          % (lanes if lanes is not None else "default (64)", REPS, WARM))
    print("#     n  chz_mpx_execute (samples from the host)   chz_rmini_execute alone (the filter of the path without the pool)   link bytes per session and block: pool down / up, without the pool down / up")
    for n in SIZES:
        print("  %5d  %10.1f   %10.1f   %d / %d (+ %d when the floats are asked for)   %d / %d" %
              (n, median(times[("mpx", n)]), median(times[("rmini", n)]), 2 * L + 16, 4 * OLEN + 24, 8 * OLEN, 4 * N + 160, 4 * OLEN + 16 * OLEN))
    pool.close(); rp.close()


if __name__ == "__main__":
    main()
