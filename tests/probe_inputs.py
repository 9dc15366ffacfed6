"""Vectors and big-integer expectations for the field / curve-formula probe (tests/probe/p2e_probe.hip).

Every expected value here is Python integer arithmetic (`%`, `divmod`, `pow(x, -1, m)`) on the inputs; nothing is taken
from csrc/fe.hpp, the CPU emulation or the C oracle.  The integer restatements of a few reductions' INTERNAL steps
(`steps_*`) are only used to say which branch an input takes, so that a test can assert it really holds inputs of every
class it claims (the counts in `Case.counts`).

`case(name, field)` -> Case: the input words of one batch (n = 1 mod 64: a partial wave, and for the four-lane ops a lone
quad), and `check(out)` which compares every output word of every element (and of every lane).  test_field_probe_cpu.py
runs the host build of the probe on them, test_gpu_field_probe.py the device build.
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

from parity_checks import structured_values

HERE = os.path.dirname(os.path.abspath(__file__))
PROBE_DIR = os.path.join(HERE, "probe")

P = 2**256 - 2**32 - 977
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
P256 = 2**256 - 2**224 + 2**192 + 2**96 - 1
N256 = 0xFFFFFFFF00000000FFFFFFFFFFFFFFFFBCE6FAADA7179E84F3B9CAC2FC632551
M = (P, N, P256, N256)
FIELD_NAMES = ("k1p", "k1n", "p256p", "p256n")
W256 = 1 << 256
P_GL = 2**64 - 2**32 + 1
F29_M = (1 << 29) - 1
F29_T = (1 << 29) + (1 << 20)
U32 = (1 << 32) - 1
PATTERNS = (0xFFFFFFFF, 0x80000000, 0x7FFFFFFF, 0x55555555, 0xAAAAAAAA)


# ---- the libraries ---------------------------------------------------------------------------------------------------
class Probe:
    """ctypes face of libp2e_probe.so (device=True) or libp2e_probe_host.so; builds the library if it is missing and
    raises if that fails"""

    def __init__(self, device, directory=PROBE_DIR, stem="p2e_probe"):
        """directory, stem: another probe built to the same scheme (tests/probe_point)"""
        target = f"lib{stem}.so" if device else f"lib{stem}_host.so"
        path = os.path.join(directory, target)
        if not os.path.exists(path):
            subprocess.check_call(["make", "-s", "-C", directory, target])
        self.L = C.CDLL(path)
        self.L.probe_ops.restype = C.c_long
        self.L.probe_ops.argtypes = [C.c_long, C.c_char_p, C.c_size_t] + [C.POINTER(C.c_int)] * 5
        self.L.probe_run.restype = C.c_long
        self.L.probe_run.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t]
        assert self.L.probe_is_device() == (1 if device else 0)
        self.failed = None   # the first (op, status) the device refused or faulted on: nothing is launched after it
        self.table = {}
        k, count = 0, 1
        while k < count:
            name = C.create_string_buffer(64)
            v = [C.c_int() for _ in range(5)]
            count = self.L.probe_ops(k, name, 64, *[C.byref(x) for x in v])
            assert count > 0
            op, field, inb, outb, lanes = (x.value for x in v)
            self.table[name.value.decode(), field] = (op, inb // 4, outb // 4 // lanes, lanes)
            k += 1
        assert self.L.probe_ops(count, None, 0, None, None, None, None, None) == -1

    def run(self, name, field, inp):
        """inp (n, IN) uint32 -> (n, lanes, OUT) uint32"""
        assert self.failed is None, f"not launched: {self.failed[0]} ended with status {self.failed[1]} earlier in this process"
        op, inw, outw, lanes = self.table[name, field]
        inp = np.ascontiguousarray(inp, np.uint32)
        assert inp.ndim == 2 and inp.shape[1] == inw, (name, inp.shape, inw)
        out = np.full((inp.shape[0], lanes, outw), 0xDDDDDDDD, np.uint32)
        rc = self.L.probe_run(op, field, inp.ctypes.data, inw * 4, out.ctypes.data, lanes * outw * 4, inp.shape[0])
        if rc != 0:
            self.failed = (f"{name}/{field}", rc)
        assert rc == 0, f"probe_run({name}, {field}) returned {rc}"
        return out


# ---- words, limbs ----------------------------------------------------------------------------------------------------
def pack(vals, nwords):
    """ints -> (n, nwords) uint32, little-endian words"""
    raw = b"".join(int(v).to_bytes(4 * nwords, "little") for v in vals)
    return np.frombuffer(raw, np.uint32).reshape(len(vals), nwords).copy()


def unpack(arr):
    """(n, k) uint32 -> ints"""
    arr = np.ascontiguousarray(arr, np.uint32)
    return [int.from_bytes(r.tobytes(), "little") for r in arr]


def cat(*cols):
    return np.concatenate(cols, axis=1)


def limbs_std(v):
    """the 29-bit split of v < 2^261 (limb 8 takes what is left: f29_from_u256's form for v < 2^256)"""
    return [(v >> (29 * k)) & F29_M for k in range(8)] + [v >> 232]


def limb_value(l):
    return sum(int(x) << (29 * k) for k, x in enumerate(l))


def limb_values(arr):
    """(n, 9) uint32 -> the integers the limb forms stand for"""
    a = np.asarray(arr, np.uint64)
    lo = [int(x) for x in (a[:, 0] + (a[:, 1] << np.uint64(29)))]                      # < 2^62
    return [lo[i] + sum(int(a[i, k]) << (29 * k) for k in range(2, 9)) for i in range(len(a))]


def size_for(k, least=2049):
    """the batch size: >= k and >= least, 1 mod 64"""
    k = max(k, least)
    return k + (1 - k) % 64


def first_bad(got, want):
    bad = np.argwhere(np.asarray(got) != np.asarray(want))
    return None if bad.size == 0 else tuple(int(x) for x in bad[0])


class Case:
    def __init__(self, inp, check, counts=None, kinds=None):
        self.inp, self.check, self.counts, self.kinds = inp, check, counts or {}, kinds


def exact_case(inp, want, counts=None, kinds=None):
    """every output word of every lane equals `want` (n, OUT), bit for bit"""
    want = np.asarray(want, np.uint32)

    def check(out):
        assert out.shape == (want.shape[0], out.shape[1], want.shape[1]), (out.shape, want.shape)
        for lane in range(out.shape[1]):
            b = first_bad(out[:, lane, :], want)
            assert b is None, (f"element {b[0]} lane {lane} word {b[1]}" + (f" ({kinds[b[0]]})" if kinds else ""),
                               [hex(int(x)) for x in inp[b[0]]], hex(int(out[b[0], lane, b[1]])), hex(int(want[b])))
    return Case(inp, check, counts, kinds)


# ---- operand sets ----------------------------------------------------------------------------------------------------
def _dedupe(v):
    seen, out = set(), []
    for x in v:
        if x not in seen:
            seen.add(x)
            out.append(x)
    return out


@functools.lru_cache(maxsize=None)
def operand_set(field, noncanonical=False):
    """the operands the issue names, for modulus M[field]: below m, or (noncanonical) anywhere below 2^256"""
    m = M[field]
    v = [0, 1, 2, m - 1, m - 2, (m + 1) // 2]
    for k in range(257):
        v += [1 << k, (1 << k) - 1, m - (1 << k)]
    v += [sum(w << (32 * i) for i in range(8)) for w in PATTERNS]
    v += [w << (32 * pos) for pos in range(8) for w in (1, 0xFFFFFFFF, 0x80000000, 0x7FFFFFFF)]
    v += structured_values(100 + field, 300)
    rng = np.random.default_rng(700 + field)
    v += [int.from_bytes(rng.bytes(32), "little") for _ in range(100)]
    if noncanonical:
        v += [m, m + 1, m + 2, W256 - 1, W256 - 2, m + (W256 - m) // 2]
        return tuple(_dedupe(x for x in v if 0 <= x < W256))
    v += [x - m for x in v if m <= x < W256]
    return tuple(_dedupe(x for x in v if 0 <= x < m))


def edge_set(field):
    m = M[field]
    v = [0, 1, 2, m - 1, m - 2, (m + 1) // 2]
    for k in (31, 32, 33, 63, 64, 128, 224, 255):
        v += [1 << k, (1 << k) - 1]
    v += [m - (1 << k) for k in (1, 32, 64, 96, 128, 192, 224)]
    v += [sum(w << (32 * i) for i in range(8)) % m for w in PATTERNS]
    v += [0xFFFFFFFF << (32 * pos) for pos in (0, 3, 6)]
    return _dedupe(x for x in v if 0 <= x < m)


def pairs(field, constructed=(), noncanonical=False, least=2049):
    """operand pairs: the constructed ones first, every edge value against every edge value, every operand of the set at
    least once on either side, random pairings of the set up to the batch size"""
    ops = operand_set(field, noncanonical)
    e = edge_set(field) + ([W256 - 1, M[field], M[field] + 1] if noncanonical else [])
    out = list(constructed) + [(a, b) for a in e for b in e]
    out += [(ops[i], ops[(7 * i + 3) % len(ops)]) for i in range(len(ops))]
    rng = np.random.default_rng(900 + field)
    n = size_for(len(out), least)
    idx = rng.integers(0, len(ops), (n - len(out), 2))
    out += [(ops[i], ops[j]) for i, j in idx]
    return out


def singles(field, noncanonical=False, extra=(), least=2049):
    ops = list(extra) + list(operand_set(field, noncanonical))
    rng = np.random.default_rng(950 + field)
    n = size_for(len(ops), least)
    lim = W256 if noncanonical else M[field]
    ops += [int.from_bytes(rng.bytes(32), "little") % lim for _ in range(n - len(ops))]
    return ops


def exact_product_pairs(field):
    """canonical (a, b) with a b = k m + d, k = 1, 2, 3 and small d >= 0: a = 2^j, b = (k m + d) / 2^j with d the least
    residue that makes the division exact (plus multiples of 2^j).  The value before the last conditional subtraction of a
    fold-style reduction is then m + d (the folds take off floor(x / 2^256) = k - 1 multiples)."""
    m = M[field]
    c = W256 - m
    out = []
    for k in (1, 2, 3):
        for j in list(range(2, 34)) + [63, 64, 65, 127, 128, 200, 250]:
            d0 = (-k * m) % (1 << j)
            for t in (0, 1, 2):
                d = d0 + (t << j)
                b = (k * m + d) >> j
                if d < c and b < m and ((k * m + d) % (1 << j)) == 0:
                    out.append((1 << j, b))
                    out.append((b, 1 << j))
    return out


# ---- integer restatements of the reductions' steps (classification only) ------------------------------------------------
def steps_p16(x):
    """reduce_p16: the second fold's carry h2 and the final subtraction `ge`"""
    c = W256 - P
    t = (x % W256) + (x >> 256) * c
    h1, t = t >> 256, t % W256
    t += h1 * c
    h2, t = t >> 256, t % W256
    t += h2 * c
    assert t < W256
    return {"h2": h2 == 1, "ge": t >= P}


def steps_wide_n(x, nh=8):
    """reduce_wide<ModN>: is the fourth fold handed a non-zero word, is the final subtraction taken"""
    c = W256 - N
    lo, hi, his = x % W256, x >> 256, []
    for _ in range(4):
        t = hi * c + lo
        lo, hi = t % W256, t >> 256
        his.append(hi)
    assert hi == 0
    return {"fold4": his[2] != 0, "ge": lo >= N}


def steps_solinas(x):
    """reduce_p256_solinas: `top` after the first carry pass, what the first fold pass leaves for the second, the final
    subtraction"""
    c = [(x >> (32 * i)) & U32 for i in range(16)]
    s = [c[0] + c[8] + c[9] - c[11] - c[12] - c[13] - c[14],
         c[1] + c[9] + c[10] - c[12] - c[13] - c[14] - c[15],
         c[2] + c[10] + c[11] - c[13] - c[14] - c[15],
         c[3] + 2 * (c[11] + c[12]) + c[13] - c[15] - c[8] - c[9],
         c[4] + 2 * (c[12] + c[13]) + c[14] - c[9] - c[10],
         c[5] + 2 * (c[13] + c[14]) + c[15] - c[10] - c[11],
         c[6] + 3 * c[14] + 2 * c[15] + c[13] - c[8] - c[9],
         c[7] + 3 * c[15] + c[8] - c[10] - c[11] - c[12] - c[13]]
    v = sum(si << (32 * i) for i, si in enumerate(s))
    top, t = v >> 256, v % W256                                  # (Python's >> floors, as the signed running carry does)
    d = 2**224 - 2**192 - 2**96 + 1
    v = t + top * d
    second, t = v >> 256, v % W256
    v = t + second * d
    assert 0 <= v < W256
    return {"top": top, "second": second, "ge": v >= P256}


def steps_barrett(x, m):
    """reduce_barrett<MOD, 8>: the number of corrections (0, 1, 2) after the estimate"""
    mu = (1 << 512) // m
    q3 = ((x >> 224) * mu) >> 288
    k = x // m - q3
    assert 0 <= k <= 2
    return k


# ---- canonical words ---------------------------------------------------------------------------------------------------
def _binary(field, fn, constructed=(), counts=None, noncanonical=False):
    pr = pairs(field, constructed, noncanonical)
    inp = cat(pack([a for a, _ in pr], 8), pack([b for _, b in pr], 8))
    return exact_case(inp, pack([fn(a, b) for a, b in pr], 8), counts(pr) if counts else None)


def _mul_counts(field):
    def counts(pr):
        xs = [a * b for a, b in pr]
        if field == 0:
            st = [steps_p16(x) for x in xs]
            return {"h2": sum(s["h2"] for s in st), "ge": sum(s["ge"] for s in st)}
        if field == 1:
            return {"ge": sum(steps_wide_n(x)["ge"] for x in xs)}
        if field == 2:
            return {"ge": sum(steps_solinas(x)["ge"] for x in xs)}
        return {"corrected": sum(steps_barrett(x, N256) > 0 for x in xs)}
    return counts


def h2_product_pairs():
    """canonical (a, b) over secp256k1's p whose product takes reduce_p16's h2 == 1 branch: a b = hi 2^256 with
    hi = floor(((K + 1) 2^256 - 1) / C), so the first fold leaves 2^256 - 1 - rem (rem < C) with h1 = K, and adding K C
    carries out again"""
    c = W256 - P
    out = []
    for k in list(range(1, 41)) + [255, 256, 1000, 65535]:
        hi = ((k + 1) * W256 - 1) // c
        j = hi.bit_length() + 1
        if j <= 255 and (hi << (256 - j)) < P:
            out.append((1 << j, hi << (256 - j)))
            out.append((hi << (256 - j), 1 << j))
    return out


def case_fe_mul(field):
    m = M[field]
    con = exact_product_pairs(field) + (h2_product_pairs() if field == 0 else [])
    return _binary(field, lambda a, b: a * b % m, con, _mul_counts(field))


def case_fe_sqr(field):
    m = M[field]
    xs = singles(field)
    return exact_case(pack(xs, 8), pack([x * x % m for x in xs], 8))


def case_fe_add(field):
    m = M[field]
    c = W256 - m
    ops = operand_set(field)
    rng = np.random.default_rng(40 + field)
    con = []
    for i in range(80):                                                           # a + b = m
        x = ops[(11 * i + 5) % len(ops)] or 1
        con.append((x, m - x))
    for i in range(80):                                                           # m <= a + b < 2^256
        x = ops[(13 * i + 7) % len(ops)] or 1
        d = [0, 1, c - 1, c // 2][i % 4] if i < 8 else int.from_bytes(rng.bytes(32), "little") % c
        b = m + d - x
        if 0 <= b < m:
            con.append((x, b))
    for i in range(80):                                                           # a + b >= 2^256
        con.append((m - 1 - i, m - 1 - (i * i) % 7))
        con.append((m - 1 - i, c + i + (0 if i % 2 else 1 << 200)))

    def counts(pr):
        return {"carry": sum(a + b >= W256 for a, b in pr), "between": sum(m <= a + b < W256 for a, b in pr),
                "equal_m": sum(a + b == m for a, b in pr)}
    return _binary(field, lambda a, b: (a + b) % m, con, counts)


def case_fe_sub(field):
    m = M[field]
    ops = operand_set(field)
    con = [(ops[(5 * i) % len(ops)],) * 2 for i in range(80)] + [(0, ops[i]) for i in range(1, 40)] + [(i, m - 1 - i) for i in range(40)]

    def counts(pr):
        return {"borrow": sum(a < b for a, b in pr), "equal": sum(a == b for a, b in pr)}
    return _binary(field, lambda a, b: (a - b) % m, con, counts)


def case_fe_neg(field):
    m = M[field]
    xs = singles(field)
    return exact_case(pack(xs, 8), pack([-x % m for x in xs], 8))


def case_fe_canon(field):
    """one conditional subtraction: any x < 2^256 with x - m < m, which is every x for the P-256 pair (m > 2^255) and for
    secp256k1's (2 m > 2^256 as well)"""
    m = M[field]
    xs = singles(field, noncanonical=True, extra=[m + d for d in (0, 1, 2, W256 - m - 1)])
    return exact_case(pack(xs, 8), pack([x % m for x in xs], 8), {"noncanonical": sum(x >= m for x in xs)})


def case_fe_mul_small(field):
    m = M[field]
    xs = singles(field, noncanonical=True)
    fs = [0, 1, 2, 3, 977, 1 << 31, (1 << 31) - 1, U32, U32 - 1, 0x55555555, 0xAAAAAAAA, 1 << 16]
    rng = np.random.default_rng(60 + field)
    f = [fs[i % len(fs)] if i % 3 else int(rng.integers(0, 1 << 32)) for i in range(len(xs))]
    # x f = k m + d with the largest factors: the pre-canonical value sits in [m, 2^256)
    for i, k in enumerate(range(1, 200)):
        ff = fs[5 + i % 4]
        if ff and (k * m) // ff < W256:
            x = -(-(k * m) // ff)                                                 # ceil: x ff = k m + small
            if x < W256:
                xs[40 + i], f[40 + i] = x, ff
    inp = cat(pack(xs, 8), pack(f, 1))
    return exact_case(inp, pack([x * ff % m for x, ff in zip(xs, f)], 8))


def case_mul_wide(field):
    pr = pairs(0, exact_product_pairs(0), noncanonical=True)
    inp = cat(pack([a for a, _ in pr], 8), pack([b for _, b in pr], 8))
    return exact_case(inp, pack([a * b for a, b in pr], 16))


def case_sqr_wide8(field):
    """every operand of all four sets, canonical or not: 2^k - 1 and the word patterns put ones across every word boundary
    of the doubled cross sum, all-ones puts the cross sum just below 2^511"""
    xs = [W256 - 1]
    for f in range(4):
        xs += operand_set(f, True)
    xs = _dedupe(xs)
    rng = np.random.default_rng(77)
    xs += [int.from_bytes(rng.bytes(32), "little") | (0x80000000 << (32 * int(rng.integers(0, 8)))) for _ in range(size_for(len(xs)) - len(xs))]
    top = sum(any((x >> (32 * k + 31)) & 1 for k in range(8)) for x in xs)
    return exact_case(pack(xs, 8), pack([x * x for x in xs], 16), {"top_bit_words": top})


W512 = 1 << 512


@functools.lru_cache(maxsize=None)
def reduce16_inputs(field):
    """[(x, class)]: raw 512-bit values.  The class is what the constructor aimed at and the steps_* restatement confirmed."""
    m = M[field]
    c = W256 - m
    rng = np.random.default_rng(1600 + field)
    rnd = lambda bits=256: int.from_bytes(rng.bytes(bits // 8), "little")
    out = []
    qmax = lambda r: (W512 - 1 - r) // m
    rs = (0, 1, m - 1)
    for r in rs:
        for q in (0, 1, 2, 3, W256 - 1, W256 - 2, W256, 1 << 255, m, m - 1, qmax(r), qmax(r) - 1):
            if q * m + r < W512:
                out.append((q * m + r, "qm_r"))
    ones = [W512 - 1, (W256 - 1) << 256, W256 - 1, W512 - 2, ((W256 - 1) << 256) + 1, ((W256 - 1) << 256) - 1, 0, 1]
    ones += [W512 - 1 - (1 << k) for k in range(0, 512, 37)] + [((W256 - 1) << 256) + (1 << k) for k in range(0, 256, 37)]
    out += [(x, "ones") for x in ones]
    sv = structured_values(1700 + field, 400)
    out += [((sv[2 * i] << 256) | sv[2 * i + 1], "structured") for i in range(200)]
    if field == 0:
        for k in list(range(1, 30)) + [1000, 1 << 20, (1 << 33) - 1]:                # see h2_product_pairs
            hi = ((k + 1) * W256 - 1) // c
            for lo in (0, 1, 2):
                x = (hi << 256) + lo
                if hi < W256 and steps_p16(x)["h2"]:
                    out.append((x, "h2"))
        for _ in range(40):                                                       # any hi: lo chosen so the first fold ends just below 2^256
            hi = rnd()
            lo = (W256 - 1 - int(rng.integers(0, 1 << 30)) - hi * c) % W256
            x = (hi << 256) + lo
            if steps_p16(x)["h2"]:
                out.append((x, "h2"))
        for k in range(1, 60):
            x = k * m + [0, 1, c - 1, int(rng.integers(0, c))][k % 4]
            if steps_p16(x)["ge"]:
                out.append((x, "ge"))
    if field == 1:
        # the fourth fold: after the second fold lo must lie within h2 C of 2^256 AND h2 >= 1, which needs h1 C > 2^256,
        # i.e. hi near 2^256.  Work backwards from the value wanted after the second fold.
        tries = 0
        while sum(k == "fold4" for _, k in out) < 40 and tries < 4000:
            tries += 1
            hi = W256 - 1 - (rnd() >> int(rng.integers(1, 200)))
            target = W256 - 1 - int(rng.integers(0, 1 << 60))
            for h1 in ((hi * c) >> 256, ((hi * c) >> 256) + 1):
                lo1 = (target - h1 * c) % W256
                lo = (lo1 - hi * c) % W256
                x = (hi << 256) + lo
                if steps_wide_n(x)["fold4"]:
                    out.append((x, "fold4"))
                    break
        for k in range(1, 60):
            x = k * m + [0, 1, c - 1, rnd(64)][k % 4]
            if steps_wide_n(x)["ge"]:
                out.append((x, "ge"))
    if field == 2:
        # Solinas: choose the high words (they set `top`), then the low words so that the value after the first carry pass
        # is top 2^256 + t for a wanted t: near 2^256 (top > 0 then leaves +1), near 0 (top < 0 leaves -1), or just above p
        for trial in range(6000):
            hw = [[0, U32, int(rng.integers(0, 1 << 32))][int(rng.integers(0, 3))] for _ in range(8)]
            if trial < 256:                                                       # the corners, where `top` is extreme
                hw = [U32 if (trial >> k) & 1 else 0 for k in range(8)]
            elif trial < 2304:                                                    # ... and their neighbourhoods
                hw = [U32 - int(rng.integers(0, 1 << 16)) if (trial >> k) & 1 else int(rng.integers(0, 1 << 16)) for k in range(8)]
            hi = sum(w << (32 * k) for k, w in enumerate(hw))
            fh = _solinas_hi_sum(hi)
            for want in ("hi", "lo", "p", "any"):
                t = {"hi": W256 - 1 - int(rng.integers(0, 1 << 20)), "lo": int(rng.integers(0, 1 << 20)),
                     "p": P256 + int(rng.integers(0, 1 << 20)), "any": rnd()}[want]
                lo = (t - fh) % W256                                            # low words add straight into the sums
                x = (hi << 256) + lo
                s = steps_solinas(x)
                out.append((x, f"top{s['top']:+d}"))
                if s["second"]:
                    out.append((x, f"second{s['second']:+d}"))
                if s["ge"]:
                    out.append((x, "ge"))
        out = _cap_classes(out, 40)
    if field >= 2:
        # Barrett: x = q m + r.  The estimate q3 is short by one exactly when r / m is below the estimate's loss, so small r
        # take one correction and large r none; q anywhere up to the top of the range.  (Two corrections: barrett_loss_bound.)
        found = {0: 0, 1: 0}
        for trial in range(20000):
            if min(found.values()) >= 40:
                break
            r = [int(rng.integers(0, 4)), m - 1 - int(rng.integers(0, 4)), rnd() % m][trial % 3]
            q = qmax(r) - (rnd() >> int(rng.integers(0, 250))) if trial % 2 else rnd()
            x = q * m + r
            if not 0 <= x < W512:
                continue
            k = steps_barrett(x, m)
            if found[k] < 40:
                found[k] += 1
                out.append((x, f"barrett{k}"))
    n = size_for(len(out))
    out += [(rnd(512), "random") for _ in range(n - len(out))]
    return tuple(out)


def _solinas_hi_sum(hi):
    """the signed word sums of reduce_p256_solinas for the input hi 2^256 (low words zero), as one integer"""
    c = [0] * 8 + [(hi >> (32 * i)) & U32 for i in range(8)]
    s = [c[8] + c[9] - c[11] - c[12] - c[13] - c[14], c[9] + c[10] - c[12] - c[13] - c[14] - c[15], c[10] + c[11] - c[13] - c[14] - c[15],
         2 * (c[11] + c[12]) + c[13] - c[15] - c[8] - c[9], 2 * (c[12] + c[13]) + c[14] - c[9] - c[10],
         2 * (c[13] + c[14]) + c[15] - c[10] - c[11], 3 * c[14] + 2 * c[15] + c[13] - c[8] - c[9],
         3 * c[15] + c[8] - c[10] - c[11] - c[12] - c[13]]
    return sum(si << (32 * i) for i, si in enumerate(s))


def _cap_classes(items, cap):
    seen, out = {}, []
    for x, k in items:
        seen[k] = seen.get(k, 0) + 1
        if seen[k] <= cap:
            out.append((x, k))
    return out


@functools.lru_cache(maxsize=None)
def solinas_top_range():
    """every value `top` can take: the sums are monotone in every word, so the extremes are at the 0 / all-ones corners"""
    tops = set()
    for lo in (0, W256 - 1):
        for mask in range(256):
            hi = sum((U32 if (mask >> k) & 1 else 0) << (32 * k) for k in range(8))
            tops.add(steps_solinas((hi << 256) + lo)["top"])
    return list(range(min(tops), max(tops) + 1))


def barrett_loss_bound(m):
    """an upper bound (a fraction of m, as numerator / 2^64) of x / m - (x >> 224) mu / 2^288 over all x < 2^512: with
    x = q1 2^224 + x0 it is x0 / m + q1 (2^512 / m - mu) / 2^288 < 2^224 / m + frac(2^512 / m).  The estimate
    q3 = floor(x / m - loss) is short by two only if the loss can exceed one: HAC 14.42's second correction is then
    unreachable, and a test cannot construct an input for it."""
    return ((1 << 224) << 64) // m + 1 + (((1 << 512) % m) << 64) // m + 1


def reduce16_required_classes(name, field):
    """the classes (>= 20 inputs each) a reduce16 op must see: those of the algorithm behind (op, field)"""
    need = ["qm_r", "ones"]
    if field == 0:
        need += ["h2", "ge"]
    elif field == 1:
        need += ["fold4", "ge"]
    elif field == 2 and name == "reduce16_r":
        need += [f"top{t:+d}" for t in solinas_top_range()] + ["second+1", "second-1", "ge"]
    else:
        need += ["barrett0", "barrett1"]                                         # (no input takes two: barrett_loss_bound)
    return need


def _class_counts(items):
    counts = {}
    for _, k in items:
        counts[k] = counts.get(k, 0) + 1
    return counts


def case_reduce16_r(field):
    items = reduce16_inputs(field)
    m = M[field]
    return exact_case(pack([x for x, _ in items], 16), pack([x % m for x, _ in items], 8), _class_counts(items), [k for _, k in items])


def case_reduce16_rq(field):
    items = reduce16_inputs(field)
    m = M[field]
    want = cat(pack([x % m for x, _ in items], 8), pack([x // m for x, _ in items], 9))
    return exact_case(pack([x for x, _ in items], 16), want, _class_counts(items), [k for _, k in items])


def case_reduce_barrett_wide(field):
    """18-word values.  Domain: the first estimate's partial remainder must fit nine words (csrc/fe.hpp); the integer
    restatement below keeps only such inputs.  Products of two 261-bit operands always qualify; so does a window of values
    whose quotient needs more than nine words -- there the remainder is still exact and the quotient saturates to all-ones."""
    m = M[field]
    mu = (1 << 512) // m
    rng = np.random.default_rng(1800 + field)

    def in_domain(x):
        q3 = ((x >> 224) * mu) >> 288
        return 0 <= x - q3 * m < 1 << 288

    items = []
    big = [(1 << 261) - 1, (1 << 261) - 2, 1 << 260, m, m - 1, 0, 1, (1 << 288) - 1, W256 - 1, W256]
    ops = operand_set(field, True)
    for a in big:
        for b in big:
            if a < 1 << 261 and b < 1 << 261:
                items.append((a * b, "product"))
    for i in range(600):
        a = (ops[(3 * i) % len(ops)] << 5 | int(rng.integers(0, 32))) if i % 2 else int.from_bytes(rng.bytes(33), "little") >> 3
        b = (ops[(5 * i + 1) % len(ops)] << 5 | 31) if i % 3 else int.from_bytes(rng.bytes(33), "little") >> 3
        items.append((a * b, "product"))
    for q in (1, 1 << 64, (1 << 266) - 1, (1 << 288) - 1, (1 << 288) - 2):
        for r in (0, 1, m - 1):
            items.append((q * m + r, "qm_r"))
    for i in range(60):                                                           # quotient >= 2^288
        q = (1 << 288) + [0, 1, 2, 1 << 32, 1 << 200][i % 5] + (int(rng.integers(0, 1 << 62)) if i >= 5 else 0)
        r = [0, 1, m - 1, int.from_bytes(rng.bytes(32), "little") % m][i % 4]
        items.append((q * m + r, "saturate"))
    items = [(x, k) for x, k in items if x < 1 << 576 and in_domain(x)]
    n = size_for(len(items), 1025)
    while len(items) < n:
        x = (int.from_bytes(rng.bytes(33), "little") >> 3) * (int.from_bytes(rng.bytes(33), "little") >> 3)
        items.append((x, "random"))
    sat = (1 << 288) - 1
    want = cat(pack([x % m for x, _ in items], 8), pack([min(x // m, sat) if x // m < 1 << 288 else sat for x, _ in items], 9))
    return exact_case(pack([x for x, _ in items], 18), want, _class_counts(items), [k for _, k in items])


# ---- Goldilocks --------------------------------------------------------------------------------------------------------
def _gl_values(canonical):
    v = [0, 1, 2, P_GL - 1, P_GL - 2, 1 << 32, (1 << 32) - 1, (1 << 32) + 1, 1 << 63, (1 << 63) - 1, 0xFFFFFFFF00000000, 0x5555555555555555,
         0xAAAAAAAAAAAAAAAA] + [1 << k for k in range(64)] + [(1 << k) - 1 for k in range(64)]
    if not canonical:
        v += [P_GL, P_GL + 1, (1 << 64) - 1, (1 << 64) - 2]
    rng = np.random.default_rng(64)
    v += [int(x) for x in rng.integers(0, 1 << 63, 40)] + [int(x) | 1 << 63 for x in rng.integers(0, 1 << 63, 40)]
    lim = P_GL if canonical else 1 << 64
    return _dedupe(x for x in v if x < lim)


def _gl_pairs(canonical):
    v = _gl_values(canonical)
    e = v[:14] + v[-8:]
    pr = [(a, b) for a in e for b in e] + [(v[i], v[(5 * i + 1) % len(v)]) for i in range(len(v))]
    rng = np.random.default_rng(65)
    n = size_for(len(pr))
    pr += [(v[i], v[j]) for i, j in rng.integers(0, len(v), (n - len(pr), 2))]
    return pr


def case_gl_mul(field):
    pr = _gl_pairs(False)
    return exact_case(cat(pack([a for a, _ in pr], 2), pack([b for _, b in pr], 2)), pack([a * b % P_GL for a, b in pr], 2))


def case_gl_add(field):
    pr = _gl_pairs(True)
    counts = {"carry": sum(a + b >= 1 << 64 for a, b in pr), "between": sum(P_GL <= a + b < 1 << 64 for a, b in pr)}
    return exact_case(cat(pack([a for a, _ in pr], 2), pack([b for _, b in pr], 2)), pack([(a + b) % P_GL for a, b in pr], 2), counts)


def steps_gl_reduce128(lo, hi):
    hh, hl = hi >> 32, hi & U32
    borrow = lo < hh
    t0 = (lo - hh - (U32 if borrow else 0)) % (1 << 64)
    t1 = hl * U32
    carry = t0 + t1 >= 1 << 64
    r = (t0 + t1 + (U32 if carry else 0)) % (1 << 64)
    return {"borrow": borrow, "carry": carry, "final": r >= P_GL}


def case_gl_reduce128(field):
    pr = _gl_pairs(False)                                                          # (lo, hi)
    eps = (1 << 32) - 1
    con = [(d, (h << 32)) for d in range(12) for h in (1, 2, U32)]                                # lo < hh: borrow
    con += [((1 << 64) - 1 - d, h) for d in range(12) for h in (U32, U32 - 1, 1 << 31)]             # t0 + t1 wraps: carry
    con += [(P_GL + d, 0) for d in list(range(12)) + [eps - 1, eps - 2]]                            # r in [p, 2^64): final
    con += [(P_GL - 1 - d + 0, 0) for d in range(4)]
    pr = con + pr
    pr = pr[:len(pr) - (len(pr) - 1) % 64]
    st = [steps_gl_reduce128(lo, hi) for lo, hi in pr]
    counts = {k: sum(s[k] for s in st) for k in ("borrow", "carry", "final")}
    return exact_case(cat(pack([a for a, _ in pr], 2), pack([b for _, b in pr], 2)), pack([(lo + (hi << 64)) % P_GL for lo, hi in pr], 2), counts)


# ---- inversion ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inversion_inputs(field):
    """the operand set, and the distribution of the CPU stress loop restated: 64-bit words that are zero, all-ones, 32-bit
    or random, cut to a random bit length half of the time; m - small"""
    m = M[field]
    xs = [0] + [x for x in operand_set(field) if x]
    rng = np.random.default_rng(3000 + field)
    for i in range(1200):
        x = 0
        for k in range(4):
            pat = int(rng.integers(0, 8))
            w = int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2))
            w = 0 if pat == 0 else (1 << 64) - 1 if pat == 1 else w & U32 if pat == 2 else w
            x |= w << (64 * k)
        if i % 2:
            x &= (1 << int(rng.integers(1, 257))) - 1
        xs.append(x % m)
    xs += [m - d for d in range(1, 65)]
    xs += [0] * 3
    n = size_for(len(xs))
    xs += [int.from_bytes(rng.bytes(32), "little") % m for _ in range(n - len(xs))]
    return tuple(xs)


def _inv(x, m):
    return pow(x, -1, m) if x else 0


def case_inv_flag(field):
    """value and ok flag; zero is reported as not invertible (and its value word is zero: d = 0 / v = 0 never change)"""
    m = M[field]
    xs = inversion_inputs(field)
    want = cat(pack([_inv(x, m) for x in xs], 8), pack([1 if x else 0 for x in xs], 1))
    return exact_case(pack(xs, 8), want, {"zero": sum(x == 0 for x in xs)})


def case_inv(field):
    """fe_inv and the ladders: x^(m-2), which is 0 for 0"""
    m = M[field]
    xs = inversion_inputs(field)
    return exact_case(pack(xs, 8), pack([_inv(x, m) for x in xs], 8), {"zero": sum(x == 0 for x in xs)})


# ---- lazy limbs --------------------------------------------------------------------------------------------------------
def f29_subc(mcls):
    """K p for K = 33, 65, 97, 129 with borrowed limbs: the constant f29_sub<M> adds (csrc/fe29.hpp), re-derived: every
    limb in [M T, M T + 2^29)"""
    k = 32 * mcls + 1
    want_min = mcls * F29_T                                                       # limb i is lifted by borrowing from limb i + 1
    l = limbs_std(k * P)
    for i in range(8):
        need = 0
        while l[i] + (need << 29) < want_min:
            need += 1
        l[i] += need << 29
        l[i + 1] -= need
    assert limb_value(l) == k * P and all(want_min <= x < want_min + (1 << 29) for x in l), (mcls, [hex(x) for x in l])
    return l


def canon_forms():
    """(forms, expected values): limb forms whose folded value lands in [p, 2^256) -- only f29_canon's last conditional
    subtraction makes those canonical.  (1 + h) p + d for d = 0, 1, 2^32 + 976 (= 2^256 - 1 - p) and values within 2^32 of p
    on either side, h = 0 .. 127 (the bits above 2^256 that limb 8 may carry), split into 29-bit limbs and again with a
    borrow pushed into every limb (limbs up to 2^30, as sums of two tight values have); also p - 1, 2 p - 1, 0 and uniform
    limbs below 2^31.  Expected: the value mod p, Python integers."""
    p = P
    c = (1 << 256) - p
    rng = np.random.default_rng(29)
    ds = [0, 1, 2, 976, 977, 1 << 29, (1 << 32) - 1, 1 << 32, c - 2, c - 1] + [int(v) for v in rng.integers(0, c, 40)]
    values = [(1 + h) * p + d for d in ds for h in (0, 1, 2, 5, 64, 127) if (1 + h) * p + d < 128 << 256]
    values += [p - 1, p - 2, p - c, 2 * p - 1, 0, 1, (1 << 256) - 1, 1 << 256, (1 << 256) + c - 1]
    values += [p - int(v) for v in rng.integers(1, 1 << 32, 20)]
    forms = []
    for v in values:
        l = [(v >> (29 * k)) & F29_M for k in range(8)] + [v >> 232]
        assert l[8] < 1 << 31
        forms.append(l)
        for k in range(8):                                     # the same value with 2^29 borrowed from limb k + 1
            if l[k + 1]:
                b = list(l)
                b[k] += 1 << 29
                b[k + 1] -= 1
                forms.append(b)
        b = list(l)
        for k in range(8):                                     # ... and borrowed everywhere it can be
            if b[k + 1]:
                b[k] += 1 << 29
                b[k + 1] -= 1
        forms.append(b)
    for _ in range(2000):
        forms.append([int(v) for v in rng.integers(0, 1 << 31, 9)])
    want = [sum(x << (29 * k) for k, x in enumerate(l)) % p for l in forms]
    return forms, want


def f29_columns_ok(au, bu):
    """fe29.hpp's f29_reduce_bounds on the 17 column sums of limb bounds au, bu: does the emulation build's tracker accept
    the product"""
    cb = [sum(au[i] * bu[k - i] for i in range(9) if 0 <= k - i <= 8) for k in range(17)]
    t = 0
    hb = [F29_M] * 9
    for k in range(9, 17):
        t = (t >> 29) + cb[k]
        if t >= 1 << 64:
            return False
    hb[8] = t >> 29
    if hb[8] > U32:
        return False
    t = 0
    for k in range(9):
        t = (t >> 29) + cb[k] + hb[k] * 31264 + ((hb[k - 1] << 8) if k else 0)
        if t >= 1 << 64:
            return False
    e9 = (t >> 29) + (hb[8] << 8)
    return e9 * 31264 + F29_M < 1 << 64


def _largest(ok, hi):
    lo = 0
    while lo < hi:
        mid = (lo + hi + 1) // 2
        lo, hi = (mid, hi) if ok(mid) else (lo, mid - 1)
    return lo


@functools.lru_cache(maxsize=None)
def tight_forms():
    """limb forms as the chains hold them (every limb <= F29_T): the 29-bit split of the operand set, the two ceilings,
    borrowed forms, random limbs up to the ceiling"""
    rng = np.random.default_rng(2900)
    forms = [limbs_std(v) for v in operand_set(0, True)]
    forms += [[F29_T] * 9, [F29_M] * 9, [F29_T] * 8 + [0], [0] * 8 + [F29_T], [F29_M + 1] * 9]
    for v in operand_set(0, True)[:200]:
        l = limbs_std(v)
        for k in range(8):
            if l[k + 1] and l[k] <= 1 << 20:
                l[k] += 1 << 29
                l[k + 1] -= 1
        forms.append(l)
    forms += [[int(x) for x in rng.integers(0, F29_T + 1, 9)] for _ in range(300)]
    forms += [[F29_T - int(x) for x in rng.integers(0, 4, 9)] for _ in range(100)]
    return tuple(tuple(f) for f in forms)


def _limb_check(inp, want_values, nout=1, tight=True, counts=None):
    """lazy-limb outputs: the integer the output limbs stand for, mod p, and (tight) every limb <= F29_T"""
    def check(out):
        assert out.shape[1] == 1 and out.shape[2] == 9 * nout
        for j in range(nout):
            o = out[:, 0, 9 * j:9 * j + 9]
            got = limb_values(o)
            bad = [i for i in range(len(got)) if got[i] % P != want_values[j][i] % P]
            assert not bad, (len(bad), bad[0], j, [hex(int(x)) for x in inp[bad[0]]], [hex(int(x)) for x in o[bad[0]]])
            if tight:
                over = np.argwhere(o > F29_T)
                assert over.size == 0, ("limb above F29_T", over[0].tolist(), [hex(int(x)) for x in o[over[0][0]]])
    return Case(inp, check, counts)


def _fit(forms, rng_seed, filler):
    forms = [list(f) for f in forms]
    n = size_for(len(forms))
    rng = np.random.default_rng(rng_seed)
    while len(forms) < n:
        forms.append(filler(rng))
    return forms


def case_f29_from_u256(field):
    xs = singles(0, noncanonical=True)
    return _limb_check(pack(xs, 8), [xs])


def case_f29_norm(field):
    """any limbs in, tight limbs out"""
    forms = list(tight_forms()) + [[U32] * 9, [U32] * 8 + [0], [0] * 8 + [U32], [1 << 31] * 9, [7 << 29] * 9, [(7 << 29) | F29_M] * 9]
    forms += [[(U32 if (mask >> k) & 1 else F29_M) for k in range(9)] for mask in range(0, 512, 7)]
    forms = _fit(forms, 2901, lambda r: [int(x) for x in r.integers(0, 1 << 32, 9)])
    inp = np.array(forms, np.uint32)
    return _limb_check(inp, [[limb_value(f) for f in forms]], counts={"top_overflow": sum(f[8] >> 29 != 0 for f in forms)})


def _form_pairs(seed, la, lb, extra=()):
    """pairs of forms with limb k of the first <= la[k] and of the second <= lb[k]: both at the ceiling, one at the ceiling,
    tight forms where they fit, random below the ceilings"""
    t = [list(f) for f in tight_forms()]
    fits = lambda f, l: all(x <= y for x, y in zip(f, l))
    pr = [(list(a), list(b)) for a, b in extra]
    pr += [(list(la), list(lb)), (list(la), [0] * 9), ([0] * 9, list(lb)), ([0] * 9, [0] * 9)]
    ta, tb = [f for f in t if fits(f, la)], [f for f in t if fits(f, lb)]
    for i in range(min(700, len(ta), len(tb)) if ta and tb else 0):
        pr.append((ta[i], tb[(7 * i + 1) % len(tb)]))
    for f in ta[:150]:
        pr.append((f, list(lb)))
    for f in tb[:150]:
        pr.append((list(la), f))
    rng = np.random.default_rng(seed)
    n = size_for(len(pr))
    while len(pr) < n:
        k = len(pr) % 3
        a = [int(rng.integers(0, x + 1)) if k else x - int(rng.integers(0, min(x, 3) + 1)) for x in la]
        b = [int(rng.integers(0, x + 1)) if k != 1 else x - int(rng.integers(0, min(x, 3) + 1)) for x in lb]
        pr.append((a, b))
    return pr


def _pair_case(pr, fn, tight, counts=None):
    inp = cat(np.array([a for a, _ in pr], np.uint32), np.array([b for _, b in pr], np.uint32))
    return _limb_check(inp, [[fn(limb_value(a), limb_value(b)) for a, b in pr]], tight=tight, counts=counts)


def case_f29_add(field):
    pr = _form_pairs(2902, [(1 << 31) - 1] * 9, [1 << 31] * 9, extra=[([U32] * 9, [0] * 9), ([U32 - F29_T] * 9, [F29_T] * 9)])
    return _pair_case(pr, lambda a, b: a + b, tight=False)


def case_f29_sub(mcls):
    def build(field):
        sc = f29_subc(mcls)
        pr = _form_pairs(2903 + mcls, [U32 - x for x in sc], sc)
        above = sum(any(x > y for x, y in zip(b, f29_subc(mcls - 1))) for _, b in pr) if mcls > 1 else len(pr)
        return _pair_case(pr, lambda a, b: a - b, tight=False, counts={"ceiling": sum(b == sc for _, b in pr), "above_lower_class": above})
    return build


def case_f29_times(k):
    def build(field):
        lim = U32 // k
        forms = [f for f in tight_forms()] + [[lim] * 9, [lim] * 8 + [0], [0] * 8 + [lim]]
        forms = _fit(forms, 2910 + k, lambda r: [int(x) for x in r.integers(0, lim + 1, 9)])
        return _limb_check(np.array(forms, np.uint32), [[k * limb_value(f) for f in forms]], tight=False)
    return build


@functools.lru_cache(maxsize=None)
def mul_ceilings():
    """operand ceilings the bound tracker accepts for one multiplication, in the combinations the chains use"""
    t, s1 = [F29_T] * 9, f29_subc(1)
    out = {
        "sum_times_double": ([2 * F29_T] * 9, [2 * F29_T] * 9),                      # (a + b) (2 c)
        "norm_diff_times_diff": (t, [F29_T + x for x in s1]),                      # norm(a - b) (c - a)
        "tight_times_tight": (t, t),
    }
    lu = _largest(lambda v: f29_columns_ok([v] * 9, [v] * 9), U32)
    out["uniform_max"] = ([lu] * 9, [lu] * 9)
    la = _largest(lambda v: f29_columns_ok([U32] * 9, [v] * 9), U32)
    out["full_times_max"] = ([U32] * 9, [la] * 9)
    for a, b in out.values():
        assert f29_columns_ok(a, b)
    assert not f29_columns_ok([lu + 1] * 9, [lu + 1] * 9) and not f29_columns_ok([U32] * 9, [la + 1] * 9)
    return out


def case_f29_mul(field):
    pr = []
    cl = mul_ceilings()
    for name, (la, lb) in cl.items():
        sub = _form_pairs(2920 + len(pr) % 97, la, lb)
        pr += sub[:420] + sub[-60:]
        pr += [(b, a) for a, b in sub[:40]]
    pr = pr[:len(pr) - (len(pr) - 1) % 64]
    ceil = {(tuple(a), tuple(b)) for a, b in cl.values()}
    return _pair_case(pr, lambda a, b: a * b, tight=True, counts={"ceilings": len(ceil & {(tuple(a), tuple(b)) for a, b in pr})})


@functools.lru_cache(maxsize=None)
def sqr_ceiling():
    lim = _largest(lambda v: f29_columns_ok([v] * 9, [v] * 9), (1 << 31) - 1)
    assert f29_columns_ok([lim] * 9, [lim] * 9)
    return lim


def case_f29_sqr(field):
    lim = sqr_ceiling()
    forms = list(tight_forms()) + [[lim] * 9, [2 * F29_T] * 9, [lim] * 8 + [0], [0] * 8 + [lim], [lim - 1] * 9]
    forms += [[2 * x for x in f] for f in tight_forms()[:400]]                      # squares of sums
    forms = _fit(forms, 2930, lambda r: [int(x) for x in r.integers(0, lim + 1, 9)] if r.integers(0, 2) else [lim - int(x) for x in r.integers(0, 4, 9)])
    return _limb_check(np.array(forms, np.uint32), [[limb_value(f) ** 2 for f in forms]], tight=True)


def _canon_case():
    forms, want = canon_forms()
    forms = forms[:len(forms) - (len(forms) - 1) % 64]
    want = want[:len(forms)]
    between = sum(P <= limb_value(l) < W256 for l in forms)
    return forms, want, {"between_p_and_2_256": between}


def case_f29_canon(field):
    forms, want, counts = _canon_case()
    return exact_case(np.array(forms, np.uint32), pack(want, 8), counts)


def case_f29_is_zero(field):
    forms, want, counts = _canon_case()
    forms += [limbs_std(k * P) for k in range(0, 64)]
    want += [0] * 64
    counts["zero"] = sum(w == 0 for w in want)
    return exact_case(np.array(forms, np.uint32), pack([1 if w == 0 else 0 for w in want], 1), counts)


# ---- the formulas --------------------------------------------------------------------------------------------------------
def ref_dbl(m, a_is_zero, X, Y, Z):
    """ec.hpp jac_dbl_cv: X3, Y3, Z3, W = Z^4"""
    a, b = X * X % m, Y * Y % m
    c = b * b % m
    d = 2 * ((X + b) ** 2 - a - c) % m
    w = pow(Z, 4, m)
    e = 3 * a % m if a_is_zero else 3 * (a - w) % m
    x3 = (e * e - 2 * d) % m
    y3 = (e * (d - x3) - 8 * c) % m
    return x3, y3, 2 * Y * Z % m, w


def ref_add(m, X1, Y1, Z1, X2, Y2, Z2):
    """ec.hpp jac_add_cv (a Z known to be one is passed as 1): X3, Y3, Z3 = Z1 Z2 H, W = (Z1 Z2)^3"""
    u1, s1 = X1 * Z2 * Z2 % m, Y1 * pow(Z2, 3, m) % m
    u2, s2 = X2 * Z1 * Z1 % m, Y2 * pow(Z1, 3, m) % m
    h, r = (u2 - u1) % m, (s2 - s1) % m
    v = u1 * h * h % m
    x3 = (r * r - pow(h, 3, m) - 2 * v) % m
    y3 = (r * (v - x3) - s1 * pow(h, 3, m)) % m
    return x3, y3, Z1 * Z2 * h % m, pow(Z1 * Z2, 3, m)


N_FORMULA = 1025


@functools.lru_cache(maxsize=None)
def formula_points(field, variant):
    """N_FORMULA rows (X1, Y1, Z1, X2, Y2, Z2, zz_in, acc) of coordinates from the operand set (not curve points).
    variant = 2 Z1ONE + Z2ONE forces those Z to one.  Rows 0 .. 127: H = 0 (the second point is the first one, rescaled
    to its own Z); then Z1 / Z2 = 0 and 1, Y1 = 0, acc = 0 / 1 / m - 1 in turn."""
    m = M[field]
    ops = operand_set(field)
    nz = [x for x in ops if x]
    rng = np.random.default_rng(5000 + 16 * field + variant)
    pick = lambda pool=ops: pool[int(rng.integers(0, len(pool)))]
    rows = []
    for i in range(N_FORMULA):
        x1, y1, z1, x2, y2, z2, zz, acc = pick(), pick(), pick(), pick(), pick(), pick(), pick(), pick()
        if i % 8 == 1:
            z1 = (0, 1, 0, m - 1)[(i // 8) % 4]
        if i % 8 == 2:
            z2 = (0, 1, 1, 0)[(i // 8) % 4]
        if i % 8 == 3:
            acc = (0, 1, m - 1)[(i // 8) % 3]
        if i % 16 == 4:
            y1 = 0
        if variant & 2:
            z1 = 1
        if variant & 1:
            z2 = 1
        if i < 128:                                                                # equal operands: H = 0
            z1 = z1 or pick(nz)
            z2 = z2 or pick(nz)
            if variant & 2:
                z1 = 1
            if variant & 1:
                z2 = 1
            x2 = x1 * z2 * z2 * pow(z1 * z1, -1, m) % m
            if i % 2:
                y2 = y1 * pow(z2, 3, m) * pow(pow(z1, 3, m), -1, m) % m              # ... and R = 0 as well
        rows.append((x1, y1, z1, x2, y2, z2, zz, acc))
    return tuple(rows)


def _cols(rows, idx, nw=8):
    return cat(*[pack([r[k] for r in rows], nw) for k in idx])


def case_jac_dbl(field):
    m = M[field]
    rows = formula_points(field, 0)
    res = [ref_dbl(m, field == 0, r[0], r[1], r[2]) for r in rows]
    want = cat(*[pack([x[k] for x in res], 8) for k in range(4)])
    return exact_case(_cols(rows, (0, 1, 2)), want, {"z3_zero": sum(x[2] == 0 for x in res)})


def case_jac_add(variant):
    def build(field):
        m = M[field]
        rows = formula_points(field, variant)
        res = [ref_add(m, *r[:6]) for r in rows]
        want = cat(*[pack([x[k] for x in res], 8) for k in range(4)])
        return exact_case(_cols(rows, range(6)), want, {"z3_zero": sum(x[2] == 0 for x in res)})
    return build


def _quad_ref(m, res, zz1, acc):
    """(X3, Y3, Z3, W) -> the four-lane result: + Z3^2, Z1^2, the prefix product through the op (a zero Z3 counts as one), zero flag"""
    x3, y3, z3, w = res
    return x3, y3, z3, w, z3 * z3 % m, zz1, acc * (z3 or 1) % m, 1 if z3 == 0 else 0


def _quad_want(q):
    return cat(*[pack([x[k] for x in q], 8) for k in range(7)], pack([x[7] for x in q], 1))


def case_jac_dbl_quad(field):
    m = M[field]
    rows = formula_points(field, 0)
    q = [_quad_ref(m, ref_dbl(m, field == 0, r[0], r[1], r[2]), r[2] * r[2] % m, r[7]) for r in rows]
    return exact_case(_cols(rows, (0, 1, 2, 7)), _quad_want(q), {"z3_zero": sum(x[7] for x in q)})


def _add_quad_rows(field, variant, have):
    """rows with zz_in = Z1^2 where the op is told it has it; out zz1: Z1^2 where the op computes or was given it, else zz_in as passed"""
    m = M[field]
    rows = [list(r) for r in formula_points(field, variant)]
    computes = not (variant & 2) and (not (variant & 1) or not have)
    for r in rows:
        if have and not (variant & 2):
            r[6] = r[2] * r[2] % m
    zz1 = [r[2] * r[2] % m if computes else r[6] for r in rows]
    return rows, zz1


def case_jac_add_quad(variant, have):
    def build(field):
        m = M[field]
        rows, zz1 = _add_quad_rows(field, variant, have)
        q = [_quad_ref(m, ref_add(m, *r[:6]), z, r[7]) for r, z in zip(rows, zz1)]
        return exact_case(_cols(rows, range(8)), _quad_want(q), {"z3_zero": sum(x[7] for x in q)})
    return build


def _to_forms(rows, idx, seed):
    """coordinates as limb forms: the 29-bit split, and every fourth row as a tight form at or near the ceiling (the value
    changes with it: the expectation is computed from the forms)"""
    rng = np.random.default_rng(seed)
    out = []
    for i, r in enumerate(rows):
        f = [limbs_std(r[k]) for k in idx]
        if i >= 128 and i % 4 == 0:
            for j in range(len(f)):
                if r[idx[j]] not in (0, 1) or i % 8 == 0:
                    f[j] = [F29_T - int(x) for x in rng.integers(0, 3, 9)] if i % 3 else [int(x) for x in rng.integers(0, F29_T + 1, 9)]
        out.append(f)
    return out


def _forms_inp(forms):
    return np.array([[x for f in row for x in f] for row in forms], np.uint32)


def _limb_groups_check(inp, wants, counts, lanes=1, mine=None, flags=None):
    """wants: list of (offset, [values]) limb groups, all tight; lanes agree word for word on [0, common)"""
    def check(out):
        assert out.shape[1] == lanes
        for lane in range(lanes):
            for off, vals in wants:
                o = out[:, lane, off:off + 9]
                got = limb_values(o)
                bad = [i for i in range(len(got)) if got[i] % P != vals[i]]
                assert not bad, (len(bad), "element", bad[0], "lane", lane, "limb group at", off, [hex(int(x)) for x in o[bad[0]]])
                over = np.argwhere(o > F29_T)
                assert over.size == 0, ("limb above F29_T", lane, off, over[0].tolist())
            if mine is not None:
                b = first_bad(out[:, lane, 54:62], mine[lane])
                assert b is None, ("mine", "element", b[0], "lane", lane, "word", b[1])
                b = first_bad(out[:, lane, 62], flags)
                assert b is None, ("z3_zero", "element", b[0], "lane", lane)
                b = first_bad(out[:, lane, :54], out[:, 0, :54])
                assert b is None, ("lanes differ", "element", b[0], "lane", lane, "word", b[1])
    return Case(inp, check, counts)


def case_jac_dbl29(field):
    rows = formula_points(0, 0)
    forms = _to_forms(rows, (0, 1, 2), 6000)
    vals = [[limb_value(f) % P for f in row] for row in forms]
    res = [ref_dbl(P, True, *v) for v in vals]
    return _limb_groups_check(_forms_inp(forms), [(9 * k, [x[k] for x in res]) for k in range(4)], {"z3_zero": sum(x[2] == 0 for x in res)})


def case_jac_add29(variant):
    def build(field):
        rows = formula_points(0, variant)
        forms = _to_forms(rows, range(6), 6001 + variant)
        for f in forms:                                                            # a Z known to be one is the form of 1
            if variant & 2:
                f[2] = limbs_std(1)
            if variant & 1:
                f[5] = limbs_std(1)
        vals = [[limb_value(f) % P for f in row] for row in forms]
        res = [ref_add(P, *v) for v in vals]
        return _limb_groups_check(_forms_inp(forms), [(9 * k, [x[k] for x in res]) for k in range(4)], {"z3_zero": sum(x[2] == 0 for x in res)})
    return build


def _quad29_case(forms, q, acc_vals, no_affine):
    """q: _quad_ref tuples.  Output: X3, Y3, Z3, Z3^2, Z1^2, acc' as limbs, then `mine` -- role 0: X3 (Z3 again for
    no_affine), 1: the prefix product before the op, 2: Z3, 3: W -- and the zero flag"""
    wants = [(0, [x[0] for x in q]), (9, [x[1] for x in q]), (18, [x[2] for x in q]), (27, [x[4] for x in q]), (36, [x[5] for x in q]),
             (45, [x[6] for x in q])]
    mine = [pack([x[2] if no_affine else x[0] for x in q], 8), pack(acc_vals, 8), pack([x[2] for x in q], 8), pack([x[3] for x in q], 8)]
    return _limb_groups_check(_forms_inp(forms), wants, {"z3_zero": sum(x[7] for x in q)}, lanes=4, mine=mine,
                              flags=np.array([x[7] for x in q], np.uint32))


def case_jac_dbl_quad29(no_affine):
    def build(field):
        rows = formula_points(0, 0)
        forms = _to_forms(rows, (0, 1, 2, 7), 6100)
        vals = [[limb_value(f) % P for f in row] for row in forms]
        q = [_quad_ref(P, ref_dbl(P, True, *v[:3]), v[2] * v[2] % P, v[3]) for v in vals]
        return _quad29_case(forms, q, [v[3] for v in vals], no_affine)
    return build


def case_jac_add_quad29(variant, no_affine, have):
    def build(field):
        rows, _ = _add_quad_rows(0, variant, have)
        forms = _to_forms(rows, range(8), 6200 + variant)
        computes = not (variant & 2) and (not (variant & 1) or not have)
        for f in forms:                                                            # Z known to be one is the form of 1; a given Z1^2 is Z1^2
            if variant & 2:
                f[2] = limbs_std(1)
            if variant & 1:
                f[5] = limbs_std(1)
            if have and not (variant & 2):
                f[6] = limbs_std(limb_value(f[2]) ** 2 % P)
        vals = [[limb_value(x) % P for x in f] for f in forms]
        q = [_quad_ref(P, ref_add(P, *v[:6]), v[2] * v[2] % P if computes else v[6], v[7]) for v in vals]
        return _quad29_case(forms, q, [v[7] for v in vals], no_affine)
    return build


# ---- the table ---------------------------------------------------------------------------------------------------------
ALL4, BASE2, K1P = (0, 1, 2, 3), (0, 2), (0,)
TABLE = {}   # name -> (fields, builder(field) -> Case)


def _reg(name, fields, builder):
    TABLE[name] = (fields, builder)


for _n, _b in (("fe_mul", case_fe_mul), ("fe_sqr", case_fe_sqr), ("fe_add", case_fe_add), ("fe_sub", case_fe_sub), ("fe_neg", case_fe_neg),
               ("fe_canon", case_fe_canon), ("fe_mul_small", case_fe_mul_small), ("reduce16_r", case_reduce16_r),
               ("reduce16_rq", case_reduce16_rq), ("fe_inv_safegcd", case_inv_flag), ("fe_inv_bingcd", case_inv_flag), ("fe_inv", case_inv),
               ("fe_inv_fermat", case_inv)):
    _reg(_n, ALL4, _b)
_reg("mul_wide", K1P, case_mul_wide)
_reg("sqr_wide8", K1P, case_sqr_wide8)
_reg("reduce_barrett_wide", (2, 3), case_reduce_barrett_wide)
_reg("gl_mul", K1P, case_gl_mul)
_reg("gl_add", K1P, case_gl_add)
_reg("gl_reduce128", K1P, case_gl_reduce128)
_reg("fe_inv_p", (0,), case_inv)
_reg("fe_inv_n", (1,), case_inv)
_reg("f29_from_u256", K1P, case_f29_from_u256)
_reg("f29_norm", K1P, case_f29_norm)
_reg("f29_add", K1P, case_f29_add)
for _k in (1, 2, 3, 4):
    _reg(f"f29_sub{_k}", K1P, case_f29_sub(_k))
for _k in (2, 3, 4):
    _reg(f"f29_times{_k}", K1P, case_f29_times(_k))
for _n in ("f29_mul", "f29_mul_call"):
    _reg(_n, K1P, case_f29_mul)
for _n in ("f29_sqr", "f29_sqr_call"):
    _reg(_n, K1P, case_f29_sqr)
for _n in ("f29_canon", "f29_canon_call"):
    _reg(_n, K1P, case_f29_canon)
_reg("f29_is_zero", K1P, case_f29_is_zero)
_reg("jac_dbl", BASE2, case_jac_dbl)
_reg("jac_dbl_quad", BASE2, case_jac_dbl_quad)
_reg("jac_dbl29", K1P, case_jac_dbl29)
for _v in range(4):
    _z = f"z{_v >> 1}{_v & 1}"
    _reg(f"jac_add_{_z}", BASE2, case_jac_add(_v))
    _reg(f"jac_add29_{_z}", K1P, case_jac_add29(_v))
    for _h in (0, 1):
        _reg(f"jac_add_quad_{_z}_have{_h}", BASE2, case_jac_add_quad(_v, _h))
        for _na in (0, 1):
            _reg(f"jac_add_quad29_{_z}_na{_na}_have{_h}", K1P, case_jac_add_quad29(_v, _na, _h))
for _na in (0, 1):
    _reg(f"jac_dbl_quad29_na{_na}", K1P, case_jac_dbl_quad29(_na))

PAIRS = [(n, f) for n, (fields, _) in TABLE.items() for f in fields]
IDS = [f"{n}-{FIELD_NAMES[f]}" for n, f in PAIRS]


@functools.lru_cache(maxsize=8)
def case(name, field):
    return TABLE[name][1](field)


# what a batch must contain (name -> {count name: least}); checked on the CPU by the tests, from the inputs alone
def required_counts(name, field):
    if name == "fe_add":
        return {"carry": 50, "between": 50, "equal_m": 50}
    if name == "fe_sub":
        return {"borrow": 50, "equal": 50}
    if name in ("reduce16_r", "reduce16_rq"):
        return {k: 20 for k in reduce16_required_classes(name, field)}
    if name == "reduce_barrett_wide":
        return {"product": 100, "qm_r": 10, "saturate": 20}
    if name == "fe_mul":
        return {0: {"h2": 20, "ge": 50}, 1: {"ge": 50}, 2: {"ge": 50}, 3: {"corrected": 50}}[field]
    if name in ("f29_canon", "f29_canon_call", "f29_is_zero"):
        return {"between_p_and_2_256": 100}
    if name.startswith("f29_sub"):
        return {"ceiling": 100, "above_lower_class": 100}
    if name in ("f29_mul", "f29_mul_call"):
        return {"ceilings": 5}
    if name == "gl_reduce128":
        return {"borrow": 20, "carry": 20, "final": 10}
    if name.startswith("jac_"):
        return {"z3_zero": 50}
    if name in ("fe_inv_safegcd", "fe_inv_bingcd", "fe_inv"):
        return {"zero": 1}
    if name == "sqr_wide8":
        return {"top_bit_words": 500}
    return {}


def run_case(probe, name, field):
    """one (op, field): the batch is what it claims (counts), is a partial wave / lone quad, and every output word is right"""
    c = case(name, field)
    n = c.inp.shape[0]
    assert n % 64 == 1 and n >= 1025, n
    for k, least in required_counts(name, field).items():
        assert c.counts.get(k, 0) >= least, (name, field, k, c.counts.get(k, 0), least)
    c.check(probe.run(name, field, c.inp))
