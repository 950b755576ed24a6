#!/usr/bin/env python3
"""What filter2 costs as a stage of the block pipeline (chz_bank_set_filter2, kernel f2_ovs) on one MI355X: the numbers of
profiles/f2_stage.txt.

  f2_probe.py                     per-block wall time of 1024 filter2 channels with demodulators, new path against the one it replaces
                                  (Bank.read_slot, the window built on the host, MiniPool.execute, the power on the host, Bank.inject,
                                  Bank.demod_only), both fed one block at a time and alternated block by block; both end in the block's
                                  PCM and flag bytes on the host.  Blocking 1 (N2 = 512): the replaced path hands its demodulators olen
                                  samples at a time, so it cannot run blocking 4 at all.  The new path alone at blocking 4 follows.
  f2_probe.py --kernel            the run to put under `rocprofv3 --kernel-trace --output-format csv`: for 1 k, 16 k and 64 k channels and
                                  (blocking 1, N2 512), (blocking 4, N2 2048) a filter2 bank without demodulators runs 40 blocks, and
                                  MiniPool.execute runs mini_ovs three times on windows of the same size
  f2_probe.py --parse TRACE.csv   the table from that trace: median time per launch of f2_ovs (firing and pending launches apart) and
                                  of mini_ovs, with the bytes per second on the stage's algorithmic bytes per channel:
                                    firing   8 (olen + held + (M2 - 1) + N2 + L2), held = M2 - 1 + (blocking - 1) olen: the slot's new
                                             samples, the window read, the history written, the response, the output
                                    pending  16 olen (the samples read and appended)
                                    mini_ovs 8 (N + N + L): window, response, output
"""
import csv
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

L, M, FS = 25920, 6481, 1.296e6
N = L + M - 1
P, OLEN = 300, 240
CONFIGS = [(1, 240, 273, 512), (4, 960, 1089, 2048)]          # blocking, L2, M2, N2
SIZES = [int(v) for v in os.environ.get("F2_PROBE_SIZES", "1024,16384,65536").split(",")]
KBLOCKS = 40


def signal(nblk, seed=31):
    rng = np.random.default_rng(seed)
    t = np.arange(nblk * L)
    return (0.05 * np.cos(2 * np.pi * (2500.3 / N) * t) * (1 + 0.4 * np.sin(2 * np.pi * 3e-4 * t)) + 1e-4 * rng.standard_normal(nblk * L)).astype(np.float32)


def first_bank(pkg, eng, nch):
    fa = pkg.filterapi
    b = eng.bank(P, OLEN, nch)
    b.set_responses(0, np.tile(fa.design_response(P, OLEN, N, True, -0.4, 0.4, 9.0), (nch, 1)))
    b.set_tuning(0, 0, (2480 + np.arange(nch) % 41).astype(np.int32), (np.arange(nch) % 7 - 3) / 12000.0)
    b.set_active(nch); b.enable_noise(FS)
    return b


def demod_params(pkg, nch):
    import oracle_lib as ol
    p = ol.lin_params()
    return [pkg.engine.DemodParams(*[getattr(p, f) for f, _ in ol.LinParams._fields_])] * nch


def kernel_run(pkg):
    E, fa = pkg.engine, pkg.filterapi
    ring = signal(8)
    for B, L2, M2, N2 in CONFIGS:
        r2 = fa.design_response(N2, L2, N2, False, -0.1, 0.1, 7.0)
        for nch in SIZES:
            eng = E.Engine(L, M, E.REAL, ring_blocks=8)
            eng.write(ring[:8 * L - (M - 1)]); eng.write(ring[8 * L - (M - 1):])
            bank = first_bank(pkg, eng, nch)
            assert bank.set_filter2(0, B) == (L2, M2, N2)
            bank.set_filter2_responses(0, np.tile(r2, (nch, 1)))
            eng.run_blocks(0, KBLOCKS)
            out = bank.read_filter2((KBLOCKS - 1) % 4, 0, 4)
            eng.close()
            pool = E.MiniPool(L2, M2, nch)
            insts = [pool.add() for _ in range(nch)]
            pool.set_response(insts[0], r2)
            win = np.tile((np.random.default_rng(1).standard_normal(N2) + 0j).astype(np.complex64), (nch, 1))
            for _ in range(3):
                pool.execute(insts, win)
            pool.close()
            print("kernel run: blocking %d N2 %d, %d channels, %d blocks; |filter2 output| %.3g" % (B, N2, nch, KBLOCKS, float(np.abs(out).max())), flush=True)


def parse(path):
    rows = list(csv.DictReader(open(path, newline="")))
    col = lambda names: next(c for c in rows[0] if any(c.lower() == n for n in names))
    kn, t0, t1 = col(["kernel_name"]), col(["start_timestamp"]), col(["end_timestamp"])
    gx, wx = col(["grid_size_x", "grid_size"]), col(["workgroup_size_x", "workgroup_size"])
    groups = {}
    for r in rows:
        name = "f2_ovs" if "f2_ovs" in r[kn] else "mini_ovs" if "::mini_ovs" in r[kn] or r[kn].startswith("mini_ovs") else None
        if name is None:
            continue
        nwg = int(r[gx]) // int(r[wx])              # the trace gives the grid in threads; dynamic LDS is not in it: the two geometries differ in threads
        groups.setdefault((name, int(r[wx]), nwg), []).append((int(r[t0]), int(r[t1]) - int(r[t0])))
    print("# kernel      blocking  N2     channels   launches   median us   GB/s on the algorithmic bytes")
    for B, L2, M2, N2 in CONFIGS:
        kb = min(256, N2 // 4)                      # threads per workgroup of both kernels' launches
        for nch in SIZES:
            f = sorted(groups.get(("f2_ovs", kb, nch), []))
            fire = [d for i, (_, d) in enumerate(f) if (i + 1) % B == 0][2:]
            pend = [d for i, (_, d) in enumerate(f) if (i + 1) % B != 0][2:]
            held = M2 - 1 + (B - 1) * OLEN
            for tag, v, byt in (("f2_ovs fire", fire, 8 * (OLEN + held + (M2 - 1) + N2 + L2)), ("f2_ovs pend", pend, 16 * OLEN)):
                if v:
                    us = float(np.median(v)) / 1e3
                    print("  %-11s %4d    %5d  %8d   %8d   %9.1f   %8.1f" % (tag, B, N2, nch, len(v), us, byt * nch / us / 1e3))
            m = [d for _, d in sorted(groups.get(("mini_ovs", kb, nch), []))]
            if m:
                us = float(np.median(m)) / 1e3
                print("  %-11s %4s    %5d  %8d   %8d   %9.1f   %8.1f" % ("mini_ovs", "-", N2, nch, len(m), us, 8 * (2 * N2 + L2) * nch / us / 1e3))


def per_block(pkg, nch=1024, warm=20, reps=500):
    E, fa = pkg.engine, pkg.filterapi
    x = signal(8)
    L2, M2, N2 = 240, 273, 512
    r2 = fa.design_response(N2, L2, N2, False, -0.1, 0.1, 7.0)
    dp = demod_params(pkg, nch)
    e_new = E.Engine(L, M, E.REAL, ring_blocks=8); b_new = first_bank(pkg, e_new, nch)
    b_new.set_filter2(0, 1); b_new.set_filter2_responses(0, np.tile(r2, (nch, 1)))
    b_new.set_pcm_stride(2 * L2); b_new.set_demod(0, 0, dp, 0.02)
    e_old = E.Engine(L, M, E.REAL, ring_blocks=8); b_old = first_bank(pkg, e_old, nch)
    b_old.set_pcm_stride(2 * OLEN); b_old.set_demod(0, 0, dp, 0.02); b_old.demod_auto(False)
    pool = E.MiniPool(L2, M2, nch)
    insts = [pool.add() for _ in range(nch)]
    for i in insts:
        pool.set_response(i, r2)
    hist = np.zeros((nch, M2 - 1), np.complex64)
    e4 = E.Engine(L, M, E.REAL, ring_blocks=8); b4 = first_bank(pkg, e4, nch)
    g4 = b4.set_filter2(0, 4); b4.set_filter2_responses(0, np.tile(fa.design_response(g4[2], g4[0], g4[2], False, -0.05, 0.05, 7.0), (nch, 1)))
    b4.set_pcm_stride(2 * g4[0]); b4.set_demod(0, 0, dp, 0.02)
    t_new, t_old, t_b4 = [], [], []
    for b in range(warm + reps):
        blk = x[(b % 8) * L:(b % 8 + 1) * L]
        s = b % 4
        t0 = time.perf_counter()
        e_new.write(blk); e_new.step(b)
        pcm_n, fl_n = b_new.read_pcm_flags(s)
        t1 = time.perf_counter()
        e_old.write(blk); e_old.step(b)
        raw = b_old.read_slot(s); noise = b_old.read_noise(s)
        win = np.concatenate([hist, raw], axis=1)
        filt = pool.execute(insts, win)
        hist = win[:, L2:]
        pw = np.mean(np.abs(filt.astype(np.complex128)) ** 2, axis=1)
        b_old.inject(s, filt, pw, noise); b_old.demod_only(b)
        pcm_o, fl_o = b_old.read_pcm_flags(s)
        t2 = time.perf_counter()
        e4.write(blk); e4.step(b)
        b4.read_pcm_flags(s)
        t3 = time.perf_counter()
        t_new.append(t1 - t0); t_old.append(t2 - t1); t_b4.append(t3 - t2)
    same = float(np.mean(pcm_n == pcm_o))
    q = lambda v: tuple(float(np.percentile(np.asarray(v[warm:]) * 1e6, p)) for p in (50, 10, 90))
    print("# one block of %d filter2 channels with linear demodulators, S16 PCM and flag bytes back on the host; %d blocks after %d, alternated block by block" % (nch, reps, warm))
    print("# us of wall time per block: median (10th .. 90th percentile)")
    print("  blocking 1, in the pipeline (write, chz_step, read_pcm_flags)                     %9.1f (%.1f .. %.1f)" % q(t_new))
    print("  blocking 1, replaced path (+ read_slot, host window, MiniPool, inject, demod_only)  %9.1f (%.1f .. %.1f)" % q(t_old))
    print("  blocking 4, in the pipeline (the replaced path cannot run it)                      %9.1f (%.1f .. %.1f)" % q(t_b4))
    print("  last block: %.4f of the PCM bytes of the two blocking-1 paths agree; link bytes per channel and block %d against %d" % (
        same, 2 * L2 + 1, 8 * OLEN + 8 + 8 * N2 + 8 * L2 + 8 * L2 + 16 + 2 * L2 + 1))
    pool.close(); e_new.close(); e_old.close(); e4.close()


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--parse":
        return parse(sys.argv[2])
    import __graft_entry__ as ge
    pkg = ge.load()
    if len(sys.argv) > 1 and sys.argv[1] == "--kernel":
        return kernel_run(pkg)
    per_block(pkg, int(os.environ.get("F2_PROBE_CHANNELS", "1024")), int(os.environ.get("F2_PROBE_WARM", "20")), int(os.environ.get("F2_PROBE_REPS", "500")))


if __name__ == "__main__":
    main()
