#!/usr/bin/env python3
"""What raw_unpack -- the kernel behind chz_input_write_raw -- costs on one MI355X, next to the device-to-device copy that
chz_input_write_device makes of the same number of OUTPUT bytes (what handing over already converted samples costs): the numbers of
profiles/raw_input.txt and DESIGN.md section 7.

The raw samples already lie in device memory (chz_input_write_raw_device: no host copy in the timed region), so a timed region holds the
kernel launch alone; HIP events on the engine's input stream bracket it.  Two figures per case, after 20 untimed calls: the median of 200
single calls, each between its own pair of events, and the mean over 10 batches of 50 back-to-back calls between one pair (which leaves
the events' own cost out and shows the rate launches can follow each other at).  Raw writes and copies alternate batch by batch in one
process.  The write position advances and wraps as it would in service; all sizes are multiples of 8, so the float4 path is what runs.

  raw_input_probe.py        (through the usual GPU call: bash scripts/gpu/call.sh raw_input python scripts/raw_input_probe.py)
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (label, master (L, M, in_type name), format name, samples)
CASES = [("Airspy R2 block", (2592000, 648001, "REAL"), "RAW_PACKED12", 400_000),
         ("8-bit I/Q block", (11520, 2881, "COMPLEX"), "RAW_S8_IQ", 400_000),
         ("uint16, N of the 129.6 MS/s master", (2592000, 648001, "REAL"), "RAW_U16", 3_240_000),
         ("packed 12-bit, the same", (2592000, 648001, "REAL"), "RAW_PACKED12", 3_240_000)]
WARM, SINGLES, BATCHES, BATCH = 20, 200, 10, 50


def main():
    import __graft_entry__ as ge
    E = ge.load().engine
    lib = E.lib()
    hip = C.CDLL("libamdhip64.so")
    vp = C.c_void_p
    hip.hipMalloc.argtypes = [C.POINTER(vp), C.c_size_t]
    hip.hipMemcpy.argtypes = [vp, vp, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [vp]
    hip.hipEventCreate.argtypes = [C.POINTER(vp)]
    hip.hipEventRecord.argtypes = [vp, vp]
    hip.hipEventSynchronize.argtypes = [vp]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), vp, vp]

    def ok(r):
        assert r == 0, r

    print("raw_unpack against a device-to-device copy of its output bytes; HIP events on the input stream; %d single calls (median) and %d x %d back to back (mean)"
          % (SINGLES, BATCHES, BATCH))
    print("%-36s %-8s %10s %10s %10s | %10s %10s | %10s %10s %8s" % ("case", "format", "samples", "raw B", "float B", "unpack us", "copy us", "unpack us", "copy us", "ratio"))
    print("%-36s %-8s %10s %10s %10s | %21s | %30s" % ("", "", "", "", "", "single, median", "back to back, mean"))
    for label, (Lm, Mm, kind), fname, n in CASES:
        fmt = getattr(E, fname)
        num, den = E.RAW_BYTES[fmt]
        comps = n * (2 if kind == "COMPLEX" else 1)
        ring_blocks = max(8, -(-2 * n // Lm))
        eng = E.Engine(Lm, Mm, getattr(E, kind), ring_blocks=ring_blocks)
        raw = np.random.default_rng(1).integers(0, 256, n * num // den + 16, dtype=np.uint8)
        flt = np.zeros(comps, np.float32)
        draw, dflt, stream = vp(), vp(), vp()
        ok(hip.hipMalloc(C.byref(draw), raw.nbytes)); ok(hip.hipMalloc(C.byref(dflt), flt.nbytes))
        ok(hip.hipMemcpy(draw, raw.ctypes.data, raw.nbytes, 1)); ok(hip.hipMemcpy(dflt, flt.ctypes.data, flt.nbytes, 1))
        ok(lib.chz_slot_stream(eng._h, 0, C.byref(stream)))
        e0, e1 = vp(), vp()
        ok(hip.hipEventCreate(C.byref(e0))); ok(hip.hipEventCreate(C.byref(e1)))

        def unpack():
            ok(lib.chz_input_write_raw_device(eng._h, fmt, 12, draw, n, 1e-4, None))

        def copy():
            ok(lib.chz_input_write_device(eng._h, dflt, n))

        def timed(fn, calls):
            ok(hip.hipEventRecord(e0, stream))
            for _ in range(calls):
                fn()
            ok(hip.hipEventRecord(e1, stream))
            ok(hip.hipEventSynchronize(e1))
            ms = C.c_float(0)
            ok(hip.hipEventElapsedTime(C.byref(ms), e0, e1))
            return ms.value * 1e3 / calls

        try:
            for fn in (unpack, copy):
                for _ in range(WARM):
                    fn()
            eng.sync()
            single = {unpack: [], copy: []}
            for _ in range(SINGLES):
                for fn in (unpack, copy):
                    single[fn].append(timed(fn, 1))
            batch = {unpack: [], copy: []}
            for _ in range(BATCHES):
                for fn in (unpack, copy):
                    batch[fn].append(timed(fn, BATCH))
            eng.sync()
            en, cs, cc = eng.raw_stats(WARM + SINGLES + BATCHES * BATCH - 1)
            want = np.frombuffer(raw[:n * num // den].tobytes(), np.int8).astype(np.int64) if fmt == E.RAW_S8_IQ else None
            assert want is None or en == int((want * want).sum()), "the last write's energy is not the samples'"
            u1, c1, ub, cb = np.median(single[unpack]), np.median(single[copy]), np.mean(batch[unpack]), np.mean(batch[copy])
            print("%-36s %-8s %10d %10d %10d | %10.2f %10.2f | %10.2f %10.2f %8.2f   (back to back: %.0f GB/s read + written by the kernel, %.0f GB/s by the copy)"
                  % (label, fname[4:], n, n * num // den, 4 * comps, u1, c1, ub, cb, ub / cb,
                     (n * num // den + 4 * comps) / ub / 1e3, 8 * comps / cb / 1e3))
            sys.stdout.flush()
        finally:
            eng.sync()
            eng.close()
            hip.hipFree(draw); hip.hipFree(dflt)


if __name__ == "__main__":
    main()
