"""packetd's decode_task() (src/packetd.c:485-629), hdlc_process() (:634-682) and crc_good() (src/ax25.c:139-155) restated in float64
Python / numpy: the checker of chz_afsk_* (tests/test_gpu_afsk.py), itself pinned to the reference's packetd.c by
tests/test_afsk_reference.py.

One Decoder is one session: blocks of L float samples in (16-bit values scaled by 2^-15, :551-552), per block the record that
chz_afsk_status carries, the frames that completed and, for every decision, cur_val and the raw margins |cur_val last_val| and -- on a
transition -- |(cur_val - last_val) mid_val| out.  The filter is the oracle's (ol.Stream, ol.channel: a REAL master of L, M with one
COMPLEX slave of olen L, P = N, shift 0), its output rounded to float32 as the reference stores it; everything behind it is double in the
reference and float64 here, in the reference's order: the oscillators step sample by sample (src/osc.c:28-70, renormalised every 16384
steps), the integrators add sample by sample (Python's sum() over a run adds from the left, starting at the carry).

f32=True runs the same statements on the oracle's float32 transform: the "f32 twin", which stands for how far the reference moves when
its own arithmetic rounds differently.

Also here: the AFSK signal generator (CRC, bit stuffing, NRZI, continuous phase, idle flags, a gain on the space tone, a start offset
inside a bit, any ratio of sample rate to bit rate) and the reference's input feeder (five blocks of zeros after a block that ends in 100 zero samples, :540-546)."""
import math

import numpy as np

import oracle_lib as ol

RENORM = 16384                     # Renorm_rate, src/osc.c:16
FRAME_BYTES = 16384                # sizeof(hdlc.frame)
BITRATE, MARK, SPACE = 1200.0, 1200.0, 2200.0


def response(L, M, samprate, bitrate=BITRATE, mark=MARK, space=SPACE):
    """set_filter(&filter_out, filter_low / samprate, filter_high / samprate, 3.0) (:496-498)"""
    N = L + M - 1
    lo, hi = min(mark, space) - bitrate / 4, max(mark, space) + bitrate / 4
    return ol.set_filter(N, L, N, True, lo / samprate, hi / samprate, 3.0, ol.COMPLEX)


def crc_good(frame):
    crc = 0xffff
    for byte in frame:
        for _ in range(8):
            feedback = 0x8408 if (crc ^ byte) & 1 else 0
            crc = (crc >> 1) ^ feedback
            byte >>= 1
    return crc == 0xf0b8


class Hdlc:
    def __init__(self):
        self.frame = bytearray(FRAME_BYTES + 1)      # :667 tests with >, so bit 131072 is still written
        self.frame_bits = self.flag_seen = self.last_bits = 0

    def process(self, bit):
        """> 0: bytes of a complete valid frame in self.frame (frame_bits already 0, as :617 leaves it); -1: a CRC failure"""
        self.last_bits = ((self.last_bits << 1) | (bit & 1)) & 0xff
        if self.last_bits == 0x7e:
            nbytes = (self.frame_bits - 7) >> 3
            self.frame_bits = 0
            if self.flag_seen and nbytes > 2:
                return nbytes if crc_good(self.frame[:nbytes]) else -1
            self.flag_seen = 1
            return 0
        if not self.flag_seen:
            return 0
        if (self.last_bits & 0x7f) == 0x7f:
            self.frame_bits = 0; self.flag_seen = 0
            return 0
        if (self.last_bits & 0x3f) == 0x3e:
            return 0
        if self.frame_bits > FRAME_BYTES << 3:
            self.frame_bits = 0; self.flag_seen = 0
            return 0
        if (self.frame_bits & 7) == 0:
            self.frame[self.frame_bits >> 3] = 0
        self.frame[self.frame_bits >> 3] |= (bit & 1) << (self.frame_bits & 7)
        self.frame_bits += 1
        return 0


class Osc:
    """set_osc(f, 0) on a zeroed struct osc, then step_osc() (src/osc.c)"""

    def __init__(self, f):
        self.phasor, self.steps = 1 + 0j, RENORM
        self.step = complex(math.cos(2 * math.pi * f), math.sin(2 * math.pi * f))

    def run(self, n):
        out = np.empty(n, np.complex128)
        ph, st, steps = self.phasor, self.step, self.steps
        for i in range(n):
            steps -= 1
            if steps <= 0:
                steps = RENORM
                ph /= abs(ph)
            out[i] = ph
            ph *= st
        self.phasor, self.steps = ph, steps
        return out


class Decoder:
    def __init__(self, L, M, samprate, resp=None, bitrate=BITRATE, mark=MARK, space=SPACE, f32=False):
        self.L, self.M, self.N, self.f32 = L, M, L + M - 1, f32
        self.resp = np.ascontiguousarray(response(L, M, samprate, bitrate, mark, space) if resp is None else resp, np.complex64)
        self.stream = ol.Stream(L, M, ol.REAL)
        self.twist = mark / space
        self.mark, self.space = Osc(-mark / samprate), Osc(-space / samprate)
        self.samppbit = int(samprate / bitrate)
        self.symphase = 0
        self.acc = [0j, 0j, 0j, 0j]          # mark, space, mark offset, space offset
        self.last_val = self.mid_val = 0.0
        self.last_terms = self.mid_terms = 0.0   # |mark|^2 + twist |space|^2 behind last_val and mid_val: what a rounding error of the difference is relative to
        self.hdlc = Hdlc()

    def block(self, samples):
        x = np.ascontiguousarray(samples, np.float32)
        L, sps, half = self.L, self.samppbit, self.samppbit // 2
        spec = self.stream.push(x, f64=not self.f32)
        y = ol.channel(spec, ol.REAL, self.N, L, 0, self.resp).astype(np.complex64).astype(np.complex128)
        pm, ps = (y * self.mark.run(L)).tolist(), (y * self.space.run(L)).tolist()
        rec = {"ndecisions": 0, "bits": 0, "crc_failures": 0, "nframes": 0, "frame_len": [0, 0], "frames": [], "cur": [], "margins": [], "pos": [], "events": []}
        cnrm = lambda z: z.real * z.real + z.imag * z.imag
        n = 0
        while n < L:
            k = sps - self.symphase
            if self.symphase < half:
                k = half - self.symphase
            k = min(k, L - n)
            m, s = pm[n:n + k], ps[n:n + k]
            self.acc = [sum(m, self.acc[0]), sum(s, self.acc[1]), sum(m, self.acc[2]), sum(s, self.acc[3])]
            n += k; self.symphase += k
            if self.symphase == half:
                self.mid_val = cnrm(self.acc[2]) - self.twist * cnrm(self.acc[3])
                self.mid_terms = cnrm(self.acc[2]) + self.twist * cnrm(self.acc[3])
                self.acc[2] = self.acc[3] = 0j
            if self.symphase < sps:
                continue
            cur = cnrm(self.acc[0]) - self.twist * cnrm(self.acc[1])
            self.last_terms = cnrm(self.acc[0]) + self.twist * cnrm(self.acc[1])
            self.acc[0] = self.acc[1] = 0j
            rec["cur"].append(cur); rec["pos"].append(n)          # pos: samples of this block consumed when the decision falls
            if cur * self.last_val >= 0:
                # (last_val is exactly zero before the first decision: x * 0 >= 0 whatever x is, so that decision has no margin to lose)
                rec["margins"].append((math.inf if self.last_val == 0.0 else abs(cur * self.last_val), None))
                self.symphase = 0
                rec["bits"] |= 1 << rec["ndecisions"]
                self.hdlc.process(1)
            else:
                rec["margins"].append((abs(cur * self.last_val), abs((cur - self.last_val) * self.mid_val)))
                self.symphase = 1 if (cur - self.last_val) * self.mid_val > 0 else -1
                nbytes = self.hdlc.process(0)
                if nbytes < 0:
                    rec["crc_failures"] += 1
                    rec["events"].append(n)
                elif nbytes > 0:
                    rec["frames"].append(bytes(self.hdlc.frame[:nbytes]))
                    rec["frame_len"][rec["nframes"]] = nbytes
                    rec["nframes"] += 1
                    rec["events"].append(n)
            rec["ndecisions"] += 1
            self.last_val = cur
        rec.update(symphase=self.symphase, last_val=self.last_val, mid_val=self.mid_val, last_terms=self.last_terms, mid_terms=self.mid_terms, flag_seen=self.hdlc.flag_seen, frame_bits=self.hdlc.frame_bits)
        return rec


DISCRETE = ("ndecisions", "bits", "symphase", "flag_seen", "frame_bits", "crc_failures", "nframes")
CONTINUOUS = ("last_val", "mid_val")


# ---- the signal ---------------------------------------------------------------------------------------------------------------------
def fcs(payload):
    """the two CRC bytes that make crc_good(payload + fcs) true (CRC-16/X.25, low byte first)"""
    crc = 0xffff
    for byte in payload:
        for _ in range(8):
            crc = (crc >> 1) ^ (0x8408 if (crc ^ byte) & 1 else 0)
            byte >>= 1
    crc ^= 0xffff
    return bytes([crc & 0xff, crc >> 8])


FLAG = [0, 1, 1, 1, 1, 1, 1, 0]


def frame_bits(payload, good_crc=True):
    """payload + CRC, least significant bit first, a zero stuffed behind every five ones"""
    tail = fcs(payload)
    if not good_crc:
        tail = bytes([tail[0] ^ 0x5a, tail[1]])
    out, ones = [], 0
    for byte in bytes(payload) + tail:
        for i in range(8):
            b = (byte >> i) & 1
            out.append(b)
            ones = ones + 1 if b else 0
            if ones == 5:
                out.append(0); ones = 0
    return out


def line_bits(items):
    """items: ("flags", n) | ("frame", payload) | ("badcrc", payload) | ("raw", [bits]) -> the bit sequence on the line before NRZI"""
    out = []
    for it in items:
        if it[0] == "flags":
            out += FLAG * it[1]
        elif it[0] == "frame":
            out += frame_bits(it[1])
        elif it[0] == "badcrc":
            out += frame_bits(it[1], good_crc=False)
        else:
            out += list(it[1])
    return out


def modulate(bits, samprate, bitrate=BITRATE, mark=MARK, space=SPACE, amplitude=0.5, space_gain=1.0, offset=0, phase=0.0):
    """NRZI (a zero toggles the tone), continuous phase, a true baud clock: sample n carries line bit floor(n bitrate / samprate), so samprate /
    bitrate need not be an integer (where it is, every bit has exactly that many samples); the first `offset` samples are dropped, so the block
    grid starts inside a bit.  -> int16 values"""
    tone, level = [], 0                         # level 0 = mark
    for b in bits:
        if not b:
            level ^= 1
        tone.append(level)
    tone = np.asarray(tone, np.int8)
    # the first sample of bit k is ceil(k samprate / bitrate): bit k's samples are those n with k <= n bitrate / samprate < k + 1.  Integer arithmetic
    # where the rates are whole numbers of Hz (every rate here), so that no sample falls on the wrong side of a bit edge by a rounding
    fs, br = float(samprate), float(bitrate)
    k = np.arange(tone.size + 1, dtype=np.int64)
    if fs.is_integer() and br.is_integer():
        first = -((-k * int(fs)) // int(br))
    else:
        first = np.ceil(k * (fs / br)).astype(np.int64)
    tone = np.repeat(tone, np.diff(first))
    freq = np.where(tone == 0, mark, space)
    ph = phase + 2 * np.pi * np.cumsum(freq) / samprate
    x = amplitude * np.where(tone == 0, 1.0, space_gain) * np.sin(ph)
    return np.rint(32767.0 * x[offset:]).astype(np.int16)


def to_wire(x, big_endian=True):
    """int16 values -> the 16-bit words as they lie in memory in that byte order"""
    return np.ascontiguousarray(np.asarray(x, np.int16).astype(">i2" if big_endian else "<i2")).view(np.uint16)


def to_float(x):
    return np.asarray(x, np.int16).astype(np.float32) * np.float32(1.0 / 32768.0)


def feed(x, L):
    """the reference's input feeder (:528-546): whole blocks of L samples (the rest of the input is not read), and five blocks of zeros
    after every block read from the input that ends in 100 zero samples -> int16 [nblocks][L]"""
    x = np.asarray(x, np.int16)
    out = []
    for b in range(x.shape[0] // L):
        blk = x[b * L:(b + 1) * L]
        out.append(blk)
        if not blk[L - 100:].any():
            out += [np.zeros(L, np.int16)] * 5
    return np.stack(out)


def run(blocks, L, M, samprate, f32=False, bitrate=BITRATE, mark=MARK, space=SPACE):
    """a fresh Decoder over int16 blocks -> the list of block records"""
    d = Decoder(L, M, samprate, bitrate=bitrate, mark=mark, space=space, f32=f32)
    return [d.block(to_float(b)) for b in blocks]


def frames_of(records):
    return [f for r in records for f in r["frames"]]


def margin_report(records, twin):
    """(floor, worst first margin, worst second margin, decisions) of a run against its f32 twin, margins relative to the square of the largest
    |cur_val|: floor = 100 x the largest distance between the two runs' cur_val over that largest |cur_val|"""
    cur = np.array([c for r in records for c in r["cur"]])
    tcur = np.array([c for r in twin for c in r["cur"]])
    assert cur.shape == tcur.shape, "the f32 twin takes another number of decisions: unusable input"
    top = float(np.abs(cur).max())
    floor = 100.0 * float(np.abs(cur - tcur).max()) / top
    m = [mm for r in records for mm in r["margins"]]
    m1 = min(a for a, _ in m) / top ** 2
    m2 = min([b for _, b in m if b is not None] or [math.inf]) / top ** 2
    return floor, m1, m2, len(m)
