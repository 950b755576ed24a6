#!/usr/bin/env python3
"""What chz_input_generate -- sig_gen's stream made on the device by siggen_fill -- costs on one MI355X for a whole block, next to the way
those samples got into the ring before it existed: chz_input_write of L floats from pinned host memory.  The numbers of profiles/siggen.txt
and DESIGN.md section 8.

Per case (129.6 MS/s REAL: L 2,592,000; 2.4 MS/s COMPLEX: L 48,000), after 20 untimed calls of each kind: the median of 100 single calls, each
between its own pair of HIP events on the engine's input stream, generate and copy alternating call by call in one process; and the mean over
10 batches of 20 back-to-back calls between one pair.  The write position advances and wraps as it would in service.

The share of the kernel's time that goes into deriving the lanes' generator states is measured with two A/B builds of the library
(make -C ka9q-radio_amd/csrc ../libchz_hip_sgp1.so ../libchz_hip_sgp2.so, loaded through CHZ_LIB in child processes of their own; where they
have not been built the lines say so): one derives the states and generates nothing, the other generates from the launch's state and derives
nothing.  For comparison only: the host time of the reference's own loop for one block (oracle_lib.RefSigGen, one core).

  siggen_probe.py [--out profiles/siggen.txt]        the parent process never touches the device; every measurement runs in a child
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# (label, L, M, in_type name, isreal)
CASES = [("129.6 MS/s REAL block", 2592000, 648001, "REAL", True), ("2.4 MS/s COMPLEX block", 48000, 12001, "COMPLEX", False)]
WARM, SINGLES, BATCHES, BATCH = 20, 100, 10, 20
FREQ, AMPLITUDE, NOISE = 10.00002e6 / 129.6e6, 0.1, 0.01
VARIANTS = {"sgp1": "states derived, nothing generated", "sgp2": "generated, no states derived"}


def child(with_copy):
    """measure in this process with whatever library CHZ_LIB names; prints one JSON line per case"""
    import __graft_entry__ as ge
    E = ge.load().engine
    lib = E.lib()
    hip = C.CDLL("libamdhip64.so")
    vp = C.c_void_p
    hip.hipEventCreate.argtypes = [C.POINTER(vp)]
    hip.hipEventRecord.argtypes = [vp, vp]
    hip.hipEventSynchronize.argtypes = [vp]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), vp, vp]
    lib.chz_host_alloc.argtypes = [C.POINTER(vp), C.c_size_t]
    lib.chz_host_free.argtypes = [vp]
    lib.chz_slot_stream.argtypes = [vp, C.c_int, C.POINTER(vp)]

    def ok(r):
        assert r == 0, (r, lib.chz_last_error())

    for label, Lm, Mm, kind, isreal in CASES:
        per = 1 if isreal else 2
        eng = E.Engine(Lm, Mm, getattr(E, kind), ring_blocks=8)
        eng.siggen(FREQ, AMPLITUDE, NOISE, 10 ** (3 / 20) if isreal else 1.0)
        stream, e0, e1 = vp(), vp(), vp()
        ok(lib.chz_slot_stream(eng._h, 0, C.byref(stream)))
        ok(hip.hipEventCreate(C.byref(e0))); ok(hip.hipEventCreate(C.byref(e1)))
        pinned = vp()
        ok(lib.chz_host_alloc(C.byref(pinned), 4 * Lm * per))
        C.memset(pinned, 0, 4 * Lm * per)

        def generate():
            ok(lib.chz_input_generate(eng._h, Lm, None))

        def copy():
            ok(lib.chz_input_write(eng._h, pinned, Lm))

        def timed(fn, calls):
            ok(hip.hipEventRecord(e0, stream))
            for _ in range(calls):
                fn()
            ok(hip.hipEventRecord(e1, stream))
            ok(hip.hipEventSynchronize(e1))
            ms = C.c_float(0)
            ok(hip.hipEventElapsedTime(C.byref(ms), e0, e1))
            return ms.value * 1e3 / calls

        fns = (generate, copy) if with_copy else (generate,)
        try:
            for fn in fns:
                for _ in range(WARM):
                    fn()
            eng.sync()
            single = {fn: [] for fn in fns}
            for _ in range(SINGLES):
                for fn in fns:
                    single[fn].append(timed(fn, 1))
            batch = {fn: [] for fn in fns}
            for _ in range(BATCHES):
                for fn in fns:
                    batch[fn].append(timed(fn, BATCH))
            eng.sync()
            out = {"case": label, "L": Lm, "floats": Lm * per,
                   "generate_single_us": float(np.median(single[generate])), "generate_single_min_us": float(np.min(single[generate])),
                   "generate_batch_us": float(np.mean(batch[generate]))}
            if with_copy:
                out.update(copy_single_us=float(np.median(single[copy])), copy_single_min_us=float(np.min(single[copy])), copy_batch_us=float(np.mean(batch[copy])))
            print("RESULT " + json.dumps(out))
            sys.stdout.flush()
        finally:
            eng.sync()
            lib.chz_host_free(pinned)
            eng.close()


def run_child(libpath, with_copy):
    env = dict(os.environ)
    if libpath:
        env["CHZ_LIB"] = libpath
    else:
        env.pop("CHZ_LIB", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--copy" if with_copy else "--no-copy"], capture_output=True, text=True, env=env, timeout=600)
    if r.returncode != 0:
        raise RuntimeError("the measuring child ended with %d:\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-3000:]))
    return [json.loads(line[7:]) for line in r.stdout.splitlines() if line.startswith("RESULT ")]


def reference_host_time(L, isreal):
    import oracle_lib as ol
    if not ol.have_ref():
        return None
    g = ol.RefSigGen(FREQ, AMPLITUDE, NOISE, 1.0, isreal, seed=1)
    g.generate(L)
    best = None
    for _ in range(3):
        t0 = time.perf_counter()
        g.generate(L)
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--copy", dest="copy", action="store_true", default=True)
    ap.add_argument("--no-copy", dest="copy", action="store_false")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "siggen.txt"))
    a = ap.parse_args()
    if a.child:
        return child(a.copy)
    import __graft_entry__ as ge
    R = ge.load().engine.SIGGEN_RUN
    lines = ["siggen_fill (chz_input_generate) against chz_input_write of the same floats from pinned host memory; one MI355X; HIP events on the input stream;",
             "%d single calls each, alternating (median, min) and %d x %d back to back (mean); R = CHZ_SIGGEN_RUN = %d floats a lane, one wavefront (64 x %d floats) a workgroup"
             % (SINGLES, BATCHES, BATCH, R, R), ""]
    main_res = run_child(None, True)
    lines.append("%-24s %10s | %12s %12s %8s | %12s %12s %8s" % ("case", "floats", "generate us", "copy us", "ratio", "generate us", "copy us", "ratio"))
    lines.append("%-24s %10s | %34s | %34s" % ("", "", "single: median (min)", "back to back, mean"))
    for r in main_res:
        lines.append("%-24s %10d | %6.1f (%5.1f) %6.1f (%5.1f) %7.2f | %12.1f %12.1f %8.2f   (the copy moves %.1f GB/s; %.2f ns a generated sample)"
                     % (r["case"], r["floats"], r["generate_single_us"], r["generate_single_min_us"], r["copy_single_us"], r["copy_single_min_us"],
                        r["generate_single_us"] / r["copy_single_us"], r["generate_batch_us"], r["copy_batch_us"], r["generate_batch_us"] / r["copy_batch_us"],
                        4 * r["floats"] / r["copy_batch_us"] / 1e3, 1e3 * r["generate_batch_us"] / r["L"]))
    lines.append("")
    var = {}
    for tag, what in VARIANTS.items():
        path = os.path.join(ROOT, "ka9q-radio_amd", "libchz_hip_%s.so" % tag)
        if os.path.exists(path):
            var[tag] = run_child(path, False)
        else:
            lines.append("A/B build %s (%s): not built here, not measured" % (tag, what))
    for i, r in enumerate(main_res):
        full = r["generate_batch_us"]
        for tag, what in VARIANTS.items():
            if tag in var:
                v = var[tag][i]["generate_batch_us"]
                lines.append("%-24s %-36s %8.1f us back to back = %.2f of the whole kernel's %.1f us" % (r["case"], what + ":", v, v / full, full))
        if "sgp2" in var:
            lines.append("%-24s share of the kernel's time spent deriving lane states: %.0f %% (1 - generated-only / whole)"
                         % (r["case"], 100 * (1 - var["sgp2"][i]["generate_batch_us"] / full)))
    lines.append("")
    for (label, Lm, Mm, kind, isreal), r in zip(CASES, main_res):
        t = reference_host_time(Lm, isreal)
        lines.append("%-24s the reference's own loop on one host core (RefSigGen, best of 3): %s"
                     % (label, "not measured (oracle/_ref is not built here)" if t is None else "%.0f us a block, %.2f ns a sample (the device: %.0fx faster)"
                        % (t, 1e3 * t / Lm, t / r["generate_batch_us"])))
    text = "\n".join(lines) + "\n"
    print(text)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
