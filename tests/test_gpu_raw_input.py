"""The raw A/D formats of the front ends other than the RX888, converted on the device (chz_input_write_raw, kernel raw_unpack) --
against tests/raw_oracle.py, the numpy restatement of airspy_unpack() and of the switch of hydrasdr.c's rx_callback(), which
tests/test_raw_input_reference.py pins to the reference's own code on the inputs built here.

Golden geometries (L 11520, M 2881, N 14400; REAL and COMPLEX), the smallest ring the engine makes (3 blocks), so that the third block's
writes wrap.  For every format two engines: one takes the raw bytes through write_raw, the twin the restatement's floats through write.
After every write the float ring itself is read back and must equal a numpy model of it bit for bit (regions never written: zero) and the
write's statistics must equal the restatement's integers; after every completed block both engines transform it and the spectra are
compared as uint32 (the int16 path's own check, tests/test_golden.py).  tests/test_raw_input_emulated.py runs this file on the CPU build."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import oracle_lib as ol
import raw_oracle as ro
from conftest import load_pkg

pytestmark = pytest.mark.gpu

L, M = 11520, 2881
RING_BLOCKS = 3
SCALE = 2.7182818284590452e-05
SIZES = (1, 3, 7, 8, 9, 63, 64, 65, 511, 512, 513)
SIZES12 = (8, 16, 24, 504, 512, 520)
ROUNDS = 3
# (format, bits): bits is read by U16 only
CASES = [(ro.PACKED12, 12), (ro.U16, 12), (ro.U16, 14), (ro.U16, 16), (ro.S16, 12), (ro.U8, 12), (ro.S8, 12), (ro.S16_IQ, 12), (ro.U8_IQ, 12), (ro.S8_IQ, 12)]
IDS = ["%s%s" % (ro.NAMES[f], "_%dbit" % b if f == ro.U16 else "") for f, b in CASES]


def on_emulator():
    return os.environ.get("CHZ_ALLOW_EMULATED_ENGINE") == "1"


def in_type(fmt):
    return ol.COMPLEX if ro.is_iq(fmt) else ol.REAL


def per(fmt):
    return 2 if ro.is_iq(fmt) else 1


def schedule(fmt):
    """the writes of one engine: ("raw", n) and ("float", n).  PACKED12 writes are multiples of 8, so single float samples in between move
    its start offset through the four residues (and show that raw and float writes alternate)"""
    ops = []
    for rnd in range(ROUNDS):
        if fmt == ro.PACKED12:
            for i, n in enumerate(SIZES12 + (L,)):
                if i % 3 == 0:
                    ops.append(("float", 1))
                ops.append(("raw", n))
        else:
            # the same sizes every round, begun one further on: in the first order alone the start offsets never reach 2 mod 4
            ops += [("raw", n) for n in SIZES[rnd:] + SIZES[:rnd] + (L,)]
    return ops


@functools.lru_cache(maxsize=None)
def raw_input(fmt, bits, n):
    """n samples of the format as bytes: every code (8- and 12-bit; all 4096 in each of a group's 8 places), the clip points and their
    neighbours (16-bit), a seeded random fill"""
    rng = np.random.default_rng(1000 * fmt + bits)
    c = n * per(fmt)                                   # components
    if fmt == ro.PACKED12:
        codes = np.concatenate([np.roll(np.arange(4096), k) for k in range(8)] + [rng.integers(0, 4096, c)])[:c]
        assert c >= 8 * 4096
        return ro.pack12(codes).view(np.uint8).copy()
    if fmt in (ro.U8, ro.S8, ro.U8_IQ, ro.S8_IQ):
        # all 256 codes in a row, then once more one place further (every code as I and as Q), then random
        codes = np.concatenate([np.arange(256), [0], np.arange(256), rng.integers(0, 256, c)])[:c]
        return codes.astype(np.uint8)
    if fmt == ro.U16:
        off = 1 << (bits - 1)
        special = [off - 2, off - 1, 2 * off - 1, 2 * off - 2, 0, 1] + ([2 * off] if 2 * off <= 0xffff else [])
        codes = rng.integers(0, 2 * off, c)
        codes[:len(special)] = special
        codes[rng.choice(np.arange(64, c), 64 * len(special), replace=False)] = np.tile(special, 64)
        return codes.astype("<u2").view(np.uint8).copy()
    special = [32767, -32767, -32768, 32766, -32767, 0]
    codes = rng.integers(-32768, 32768, c)
    codes[:len(special)] = special
    codes[rng.choice(np.arange(64, c), 64 * len(special), replace=False)] = np.tile(special, 64)
    if fmt == ro.S16_IQ:
        # the reference sums x*x + y*y in int: (-32768, -32768) overflows it there; no such pair here
        both = (codes[0::2] == -32768) & (codes[1::2] == -32768)
        codes[1::2][both] = -32767
    return codes.astype("<i2").view(np.uint8).copy()


def raw_total(fmt):
    return sum(n for op, n in schedule(fmt) if op == "raw")


def float_fill(fmt, n, seed):
    """n float samples for the float writes in between"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n * per(fmt)) * 0.01).astype(np.float32)
    return x.view(np.complex64) if ro.is_iq(fmt) else x


def as_samples(fmt, floats):
    return floats.view(np.complex64) if ro.is_iq(fmt) else floats


_hip = None


def hip():
    global _hip
    if _hip is None:
        _hip = C.CDLL("libamdhip64.so")
        _hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        _hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _hip.hipFree.argtypes = [C.c_void_p]
    return _hip


def read_ring(eng):
    """the float ring itself (on the CPU build of the engine device memory is host memory)"""
    p, n = eng.ring()
    out = np.empty(n, np.float32)
    if on_emulator():
        C.memmove(out.ctypes.data, p, out.nbytes)
    else:
        assert hip().hipMemcpy(out.ctypes.data, p, out.nbytes, 2) == 0      # hipMemcpyDeviceToHost
    return out


class DeviceBytes:
    """bytes in device memory, 16-byte aligned and readable up to the next 16-byte boundary, through the runtime the engine is linked to"""

    def __init__(self, raw):
        size = (raw.size + 15) // 16 * 16 + 16
        if on_emulator():
            self.keep = np.zeros(size + 16, np.uint8)
            self.base = (self.keep.ctypes.data + 15) // 16 * 16
            C.memmove(self.base, raw.ctypes.data, raw.size)
            self.dev = False
        else:
            ptr = C.c_void_p()
            assert hip().hipMalloc(C.byref(ptr), size) == 0
            assert hip().hipMemcpy(ptr, raw.ctypes.data, raw.size, 1) == 0                # hipMemcpyHostToDevice, complete on return
            self.base, self.dev = ptr.value, True

    def free(self):
        if self.dev:
            hip().hipFree(self.base)
            self.dev = False


class Model:
    """what the float ring must hold"""

    def __init__(self, fmt):
        self.per = per(fmt)
        self.ring = np.zeros(RING_BLOCKS * L * self.per, np.float32)
        self.wpos = (M - 1) * self.per
        self.offsets, self.straddles = set(), 0

    def write(self, floats, raw=True):
        floats = np.ascontiguousarray(floats).view(np.float32).reshape(-1)
        if raw and floats.size:
            self.offsets.add(self.wpos % 4)
            self.straddles += self.wpos + floats.size > self.ring.size
        idx = (self.wpos + np.arange(floats.size)) % self.ring.size
        self.ring[idx] = floats
        self.wpos = int((self.wpos + floats.size) % self.ring.size)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def engines(pkg, fmt):
    return (pkg.engine.Engine(L, M, in_type(fmt), ring_blocks=RING_BLOCKS), pkg.engine.Engine(L, M, in_type(fmt), ring_blocks=RING_BLOCKS))


def test_the_inputs_hold_what_the_checks_need():
    """every code of the 8- and 12-bit formats, the clip points of the 16-bit ones, and for every non-packed format a sample on which
    (float)(scale * x) and (float)scale * (float)x differ, so that the wrong scaling rule cannot pass; for PACKED12 the float rule equals
    the double product of the float-rounded scale on every code"""
    for fmt, bits in CASES:
        n = raw_total(fmt)
        x = ro.integers(fmt, raw_input(fmt, bits, n), n, bits)
        if fmt == ro.PACKED12:
            for place in range(8):
                assert np.array_equal(np.unique(x[place::8]), np.arange(-2048, 2048))
            codes = np.arange(-2048, 2048)
            assert same_bits(ro.scale_float(codes, SCALE), ro.scale_double(codes, float(np.float32(SCALE))))
            continue
        assert not same_bits(ro.scale_double(x, SCALE), ro.scale_float(x, SCALE)), ro.NAMES[fmt]
        if fmt in (ro.U8, ro.S8):
            assert np.array_equal(np.unique(x), np.arange(-128, 128))
        elif fmt in (ro.U8_IQ, ro.S8_IQ):
            assert np.array_equal(np.unique(x[0::2]), np.arange(-128, 128)) and np.array_equal(np.unique(x[1::2]), np.arange(-128, 128))
        elif fmt == ro.U16:
            off = 1 << (bits - 1)
            want = {-2, -1, off - 1, off - 2, -off, 1 - off} | ({off} if bits < 16 else set())
            assert want <= set(x.tolist()), (bits, want - set(x.tolist()))
        else:
            assert {32767, -32767, -32768, 32766, 0} <= set(x.tolist())
            if fmt == ro.S16_IQ:
                assert not ((x[0::2] == -32768) & (x[1::2] == -32768)).any()
    # about a third of all codes tell the two rules apart at this scale
    for codes in (np.arange(-128, 128), np.arange(-2048, 2048), np.arange(-32768, 32768)):
        differ = (ro.scale_double(codes, SCALE).view(np.uint32) != ro.scale_float(codes, SCALE).view(np.uint32)).mean()
        assert 0.2 < differ < 0.5, differ


@pytest.mark.parametrize("fmt,bits", CASES, ids=IDS)
def test_raw_writes_fill_the_ring_as_the_restatement_s_floats_do(fmt, bits):
    pkg = load_pkg()
    raw = raw_input(fmt, bits, raw_total(fmt))
    num, den = ro.BYTES[fmt]
    er, ef = engines(pkg, fmt)
    try:
        assert er.ring()[1] == RING_BLOCKS * L * per(fmt)
        model, done, written, used, stats = Model(fmt), 0, 0, 0, []
        for k, (op, n) in enumerate(schedule(fmt)):
            if op == "float":
                x = float_fill(fmt, n, k)
                er.write(x); ef.write(x)
                model.write(x, raw=False)
            else:
                chunk = raw[used * num // den:(used + n) * num // den]
                used += n
                want, energy, clip_s, clip_c = ro.convert(fmt, chunk, n, SCALE, bits)
                t = er.write_raw(chunk, fmt, SCALE, bits)
                ef.write(as_samples(fmt, want))
                model.write(want)
                assert t == len(stats)
                stats.append((energy, clip_s, clip_c))
                assert er.raw_stats(t) == stats[t], (k, n, er.raw_stats(t), stats[t])
                # tickets count from 0: this was write number w = t + 1, after which tickets w - 8 .. w - 1 are kept and w - 9 is gone
                if t >= 7:
                    assert er.raw_stats(t - 7) == stats[t - 7]
                if t >= 8:
                    with pytest.raises(pkg.engine.ChzError, match="are gone"):
                        er.raw_stats(t - 8)
                with pytest.raises(pkg.engine.ChzError):
                    er.raw_stats(t + 1)                                                # not yet issued
            ring = read_ring(er)
            assert same_bits(ring, model.ring), (k, op, n, np.flatnonzero(ring.view(np.uint32) != model.ring.view(np.uint32))[:8])
            written += n
            while written >= (done + 1) * L:
                er.forward(done); ef.forward(done)
                assert same_bits(er.spectrum(done % 4), ef.spectrum(done % 4)), (k, done)
                done += 1
        assert done == ROUNDS and used == raw_total(fmt)
        assert same_bits(read_ring(ef), model.ring)
        assert model.straddles >= 1, "no raw write straddled the ring end"
        # float offsets: a COMPLEX ring's writes start at even floats; its SAMPLE offsets take all four residues (float offset mod 8)
        assert model.offsets == ({0, 2} if ro.is_iq(fmt) else {0, 1, 2, 3}), model.offsets
    finally:
        er.close(); ef.close()


@pytest.mark.parametrize("fmt", [ro.U8, ro.S8_IQ], ids=["u8", "s8_iq"])
def test_a_raw_write_then_a_float_write_is_their_concatenation(fmt):
    pkg = load_pkg()
    n1 = 4099
    raw = raw_input(fmt, 12, raw_total(fmt))
    er, ef = engines(pkg, fmt)
    try:
        head = ro.convert(fmt, raw, n1, SCALE)[0]
        tail = float_fill(fmt, L - n1, 5)
        er.write_raw(raw, fmt, SCALE, n=n1); er.write(tail)
        ef.write(np.concatenate([as_samples(fmt, head), tail]))
        er.forward(0); ef.forward(0)
        assert same_bits(er.spectrum(0), ef.spectrum(0))
        assert same_bits(read_ring(er), read_ring(ef))
    finally:
        er.close(); ef.close()


@pytest.mark.parametrize("fmt", list(range(8)), ids=[ro.NAMES[f] for f in range(8)])
def test_samples_in_device_memory_give_the_same_ring_and_statistics(fmt):
    pkg = load_pkg()
    sizes = (8, 24, 520, 4000) if fmt == ro.PACKED12 else (1, 9, 513, 4001)
    raw = raw_input(fmt, 12, raw_total(fmt))
    num, den = ro.BYTES[fmt]
    er = pkg.engine.Engine(L, M, in_type(fmt), ring_blocks=RING_BLOCKS)
    dev = []
    try:
        model, used = Model(fmt), 0
        for t, n in enumerate(sizes):
            chunk = raw[used * num // den:(used + n) * num // den]
            used += n
            want, energy, clip_s, clip_c = ro.convert(fmt, chunk, n, SCALE)
            dev.append(DeviceBytes(chunk))
            assert er.write_raw_device(dev[-1].base, n, fmt, SCALE) == t
            model.write(want)
            assert er.raw_stats(t) == (energy, clip_s, clip_c)
            assert same_bits(read_ring(er), model.ring), (t, n)
        with pytest.raises(pkg.engine.ChzError, match="16-byte"):
            er.write_raw_device(dev[-1].base + 4, 8, fmt, SCALE)
        t = er.write_raw_device(dev[-1].base, 8, fmt, SCALE)                           # the refusal moved nothing
        model.write(ro.convert(fmt, raw[used * num // den - sizes[-1] * num // den:], 8, SCALE)[0])
        assert t == len(sizes) and same_bits(read_ring(er), model.ring)
    finally:
        er.sync()
        er.close()
        for d in dev:
            d.free()


def refusals(fmt):
    """(format, bits, n) a master of fmt's kind must refuse, with what chz_last_error says"""
    other = ro.U8 if ro.is_iq(fmt) else ro.U8_IQ
    out = [(other, 12, 8, "master is"), (fmt, 12, -1, "samples"), (8, 12, 8, "unknown raw"), (-1, 12, 8, "unknown raw")]
    if not ro.is_iq(fmt):
        out += [(ro.PACKED12, 12, 12, "groups of 8"), (ro.U16, 1, 8, "bits"), (ro.U16, 17, 8, "bits"), (ro.U16, 0, 8, "bits")]
    return out


@pytest.mark.parametrize("fmt", [ro.S16, ro.S16_IQ], ids=["real", "complex"])
def test_refusals_leave_the_write_position_where_it_was(fmt):
    pkg = load_pkg()
    E = pkg.engine
    raw = raw_input(fmt, 12, raw_total(fmt))
    num, den = ro.BYTES[fmt]
    big = np.zeros(8 * (RING_BLOCKS * L + 8), np.uint8)
    er, ef = engines(pkg, fmt)
    try:
        job = 0
        for bad_fmt, bits, n, says in refusals(fmt) + [(fmt, 12, RING_BLOCKS * L + 1, "does not fit")]:
            if says != "does not fit":
                assert E.lib().chz_input_raw_check(in_type(fmt), bad_fmt, bits, n) < 0 and says in E.lib().chz_last_error().decode()
            with pytest.raises(E.ChzError, match=says):
                er.write_raw(big, bad_fmt, SCALE, bits, n=n)
            chunk = raw[(job % 3) * L * num // den:(job % 3 + 1) * L * num // den]
            er.write_raw(chunk, fmt, SCALE)
            ef.write(as_samples(fmt, ro.convert(fmt, chunk, L, SCALE)[0]))
            er.forward(job); ef.forward(job)
            assert same_bits(er.spectrum(job % 4), ef.spectrum(job % 4)), (bad_fmt, bits, n)
            job += 1
        assert same_bits(read_ring(er), read_ring(ef))
        assert len(er.raw_stats(job - 1)) == 3                                            # refused writes took no ticket
        with pytest.raises(E.ChzError):
            er.raw_stats(job)
        for f, b in CASES:
            assert E.lib().chz_input_raw_check(in_type(f), f, b, 8) == 0
        assert E.lib().chz_input_raw_check(ol.REAL, ro.U16, 2, 0) == 0 and E.lib().chz_input_raw_check(ol.REAL, ro.PACKED12, 0, 0) == 0
    finally:
        er.close(); ef.close()


def test_int16_input_and_raw_input_exclude_each_other():
    pkg = load_pkg()
    E = pkg.engine
    x16 = np.random.default_rng(3).integers(-32768, 32768, 2 * L).astype(np.int16)
    raw = raw_input(ro.S16, 12, raw_total(ro.S16))
    e16, t16 = engines(pkg, ro.S16)
    er, ef = engines(pkg, ro.S16)
    try:
        e16.write_i16(x16[:L], 1e-4); t16.write_i16(x16[:L], 1e-4)
        with pytest.raises(E.ChzError, match="cannot be mixed"):
            e16.write_raw(raw, ro.S16, SCALE, n=L)
        e16.write_i16(x16[L:], 1e-4); t16.write_i16(x16[L:], 1e-4)
        for job in (0, 1):
            e16.forward(job); t16.forward(job)
            assert same_bits(e16.spectrum(job), t16.spectrum(job))
        er.write_raw(raw, ro.S16, SCALE, n=L)
        ef.write(ro.convert(ro.S16, raw, L, SCALE)[0])
        with pytest.raises(E.ChzError, match="cannot be mixed"):
            er.write_i16(x16[:L], 1e-4)
        er.write_raw(raw[2 * L:], ro.S16, SCALE, n=L)
        ef.write(ro.convert(ro.S16, raw[2 * L:], L, SCALE)[0])
        for job in (0, 1):
            er.forward(job); ef.forward(job)
            assert same_bits(er.spectrum(job), ef.spectrum(job))
    finally:
        for e in (e16, t16, er, ef):
            e.close()
