#!/usr/bin/env python3
"""What one block of packet-radio sessions costs through the pooled AFSK / AX.25 decoders (chz_afsk_execute) and through the path without
the pool (chz_rmini_execute on packetd's geometry for the filter, everything behind it on the host), on one MI355X at packetd's own shape
(L 960, M 961, 48 kHz, 20 ms blocks).  The numbers of profiles/afsk_pool.txt.

  afsk_probe.py                 the table: for n = 1, 64 and 1024 sessions the wall time of one chz_afsk_execute call (a host clock around a call
                                that ends in a stream synchronise; samples from the host), of one chz_rmini_execute call of the same n windows, and
                                the bytes that cross the link per session and block, both ways; medians of interleaved runs after a warm-up
  afsk_probe.py --kernel N      only chz_afsk_execute, N sessions, 300 calls: the run to put under `rocprofv3 --kernel-trace --stats` for
                                afsk_ovs's own time
  afsk_probe.py --kernel-rmini N   the same for chz_rmini_execute on the same geometry, N windows: rmini_ovs's own time, the filter's share of afsk_ovs

Every session hears the same signal (idle flags and frames of 64 bytes): a block's time does not depend on what the sessions decode, only
a completed frame adds its copy.  The host stage of the path without the pool -- 960 double-precision complex steps per session and block --
is not timed here: profiles/afsk_pool.txt has the reference's own decode_task() per block on one host core."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge      # noqa: E402
import afsk_oracle as ao          # noqa: E402  (signal generator and filter response only)

L, M, FS, CAP = 960, 961, 48000.0, 1024
WARM, REPS = int(os.environ.get("AFSK_PROBE_WARM", "20")), int(os.environ.get("AFSK_PROBE_REPS", "200"))
SIZES = (1, 64, 1024)


def median(v):
    return float(np.median(np.asarray(v[WARM:]))) * 1e6


def main():
    pkg = ge.load()
    E = pkg.engine
    only = int(sys.argv[2]) if len(sys.argv) > 2 and sys.argv[1] == "--kernel" else None
    if len(sys.argv) > 2 and sys.argv[1] == "--kernel-rmini":
        n = int(sys.argv[2])
        rp = E.RealMiniPool(L, M, [(L, E.COMPLEX)], CAP)
        rinst = [rp.add() for _ in range(n)]
        for i in rinst:
            rp.set_response(i, 0, ao.response(L, M, FS))
        win = np.random.default_rng(3).standard_normal((n, L + M - 1)).astype(np.float32)
        for _ in range(300):
            rp.execute(rinst, win)
        print("kernel run: 300 calls of chz_rmini_execute, %d windows" % n)
        rp.close()
        return
    rng = np.random.default_rng(5)
    items = [("flags", 30)]
    for _ in range(6):
        items += [("frame", bytes(rng.integers(0, 256, 64, dtype=np.uint8))), ("flags", 4)]
    x = ao.modulate(ao.line_bits(items), FS, amplitude=0.4)
    blocks = ao.to_wire(x[:x.size // L * L]).reshape(-1, L)
    resp = ao.response(L, M, FS)
    pool = E.AfskPool(L, M, FS, CAP, frame_stride=512)
    insts = [pool.add() for _ in range(sum(SIZES))]             # (the storage grows beyond `capacity`, the launch size)
    for i in insts:
        pool.set_response(i, resp)
    if only:
        frames = 0
        for call in range(300):
            st, fr = pool.execute(insts[:only], [blocks[call % len(blocks)]] * only)
            frames += len(fr[0])
        print("kernel run: 300 calls of chz_afsk_execute, %d sessions, session 0 delivered %d frames" % (only, frames))
        pool.close()
        return
    rp = E.RealMiniPool(L, M, [(L, E.COMPLEX)], CAP)
    rinst = [rp.add() for _ in range(CAP)]
    for i in rinst:
        rp.set_response(i, 0, resp)
    win = np.zeros((CAP, L + M - 1), np.float32)
    win[:, M - 1:] = ao.to_float(x[3 * L:4 * L])
    times, frames = {}, 0
    steps = [(kind, n) for n in SIZES for kind in ("afsk", "rmini")]
    mine = {1: insts[-1:], 64: insts[1024:1088], 1024: insts[:1024]}        # sessions of their own for every size: each hears the stream in order
    order = np.random.default_rng(2)
    for rep in range(WARM + REPS):
        for k in order.permutation(len(steps)):               # a new order every repetition (scripts/wfm_probe.py has the reason)
            kind, n = steps[k]
            t0 = time.perf_counter()
            if kind == "afsk":
                st, fr = pool.execute(mine[n], [blocks[rep % len(blocks)]] * n)
                frames += len(fr[0])
            else:
                rp.execute(rinst[:n], win[:n])
            times.setdefault((kind, n), []).append(time.perf_counter() - t0)
    assert frames > 0 or WARM + REPS < len(blocks)
    print("# one 20 ms block of n packet sessions at 48 kHz, medians of %d interleaved calls after %d, us of wall time per call" % (REPS, WARM))
    print("#     n  chz_afsk_execute (samples from the host)   chz_rmini_execute alone (the filter of the path without the pool)   link bytes per session and block: pool down / up, without the pool down / up")
    for n in SIZES:
        print("  %5d  %10.1f   %10.1f   %d / %d (+ a frame's bytes when one completes)   %d / %d" %
              (n, median(times[("afsk", n)]), median(times[("rmini", n)]), 2 * L + 16, 56, 4 * (L + M - 1) + 160, 8 * L))
    pool.close(); rp.close()


if __name__ == "__main__":
    main()
