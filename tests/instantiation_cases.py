"""What the instantiation sweeps (tests/test_gpu_instantiations.py on the device, tests/test_instantiations_emulated.py on the fiber
emulator) share: the (R1,R2) menus read from chz_plan.h, the explicit plans that put one forward pair into each position, the radices
such a plan must report, and the dynamic LDS of a plan's first pass worked out from the plan string."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ka9q-radio_amd", "csrc")
REAL, COMPLEX = 2, 1


def menu_pairs(name):
    """The (R1, R2) pairs of CHZ_FWD_MENU / CHZ_CHAN_MENU in the order the header lists them."""
    src = open(os.path.join(CSRC, "chz_plan.h")).read()
    body = re.search(r"#define %s\(X\)(.*?)\n(?://|\n)" % name, src, re.S).group(1)
    return [(int(a), int(b)) for a, b in re.findall(r"X\((\d+),\s*(\d+)\)", body)]


FWD_PAIRS = menu_pairs("CHZ_FWD_MENU")
FWD_LENGTHS = sorted({a * b for a, b in FWD_PAIRS})
CHAN_SIZES = sorted(a * b for a, b in menu_pairs("CHZ_CHAN_MENU"))


def first_pair(n):
    """fwd_menu_lookup: what axes a and b (fwd_first_real / fwd_cols) run for a length."""
    return next(p for p in FWD_PAIRS if p[0] * p[1] == n)


def rows_pair(n):
    """fwd_menu_lookup_c: axis c (fwd_rows) prefers a pair whose R2 is a multiple of 16."""
    return next((p for p in FWD_PAIRS if p[0] * p[1] == n and p[1] % 16 == 0), first_pair(n))


def sweep_plans(A):
    """[(plan, in_type, (ra, rb, rc))]: length A as first, middle and last axis between two 16-point axes, REAL and COMPLEX."""
    out = []
    for axes in ((A, 16, 16), (16, A, 16), (16, 16, A)):
        want = (first_pair(axes[0]), first_pair(axes[1]), rows_pair(axes[2]))
        for in_type in (REAL, COMPLEX):
            out.append(("%dx%dx%d" % axes, in_type, want))
    return out


def sweep_LM(N):
    """An odd M of about N/5; N is even here, so L = N - M + 1 is even, as every master of the suite has it."""
    M = (N // 5) | 1
    return N - M + 1, M


_PLAN = re.compile(r"N=(\d+) (real|complex) axes (\d+)x(\d+)x(\d+) radices \((\d+),(\d+)\)\((\d+),(\d+)\)\((\d+),(\d+)\) tiles T1=(\d+) T2=(\d+) Ta=(\d+)")


def parse_plan(desc):
    """eng.plan -> dict(N, real, axes, radices (ra, rb, rc), T1, T2, Ta)."""
    if isinstance(desc, bytes):
        desc = desc.decode()
    m = _PLAN.match(desc)
    assert m, desc
    g = [m.group(2)] + [int(m.group(i)) for i in (1,) + tuple(range(3, 15))]
    return dict(real=g[0] == "real", N=g[1], axes=tuple(g[2:5]), radices=((g[5], g[6]), (g[7], g[8]), (g[9], g[10])),
                T1=g[11], T2=g[12], Ta=g[13])


def lds1_bytes(desc):
    """Dynamic LDS of the first pass as finish_fwd_plan sizes it: Na*T1 points and R1 pads of (T1 - R2*T1) mod 32, and for a REAL
    master a second Na*T1 region for the Hermitian split; 8 bytes a point."""
    p = parse_plan(desc)
    (r1, r2), na, t1 = p["radices"][0], p["axes"][0], p["T1"]
    return 8 * ((2 if p["real"] else 1) * na * t1 + r1 * ((t1 - r2 * t1) % 32))
