"""Adversarial inputs of both verifiers and of the scalar-multiplication programs, shared by test_adversarial_cpu.py and
test_gpu_adversarial.py.  Nothing here uses the code under test: Python integers and oracle/p2e_ref.py only.

Random signatures give the verifiers uniform u1 = msg / s, u2 = r / s and a random public key.  The rows below force them:
for chosen u1, u2 != 0 and ANY curve point pk (no discrete log needed)

    R = u1 G + u2 pk,   r = R.x mod n,   s = r / u2 mod n,   msg = u1 s mod n

is a signature for which the circuit computes exactly these u1 and u2, and it verifies.  So every clean row built this way
carries the expectation "verdict 1" from the inputs alone, independent of every oracle.

Programs: "verify" (verify_secp256k1_message_circuit), "glv_mul", and per curve "windowed" (curve_scalar_mul_windowed),
"bitwise" (curve_scalar_mul), on P-256 also "verify" (verify_p256_message_circuit); the curve programs use the blinding
point blind(curve_id).  classes(program, curve_id) is the list of named rows, batch(program, curve_id) lays it out.

Every Case carries `kind` (its class), `args` ((msg, r, s, pkx, pky) or (px, py, k) as raw 256-bit integers), `flagged`
(the reference panics on it: inverse of zero) and `valid` (1 / 0 / None = no expectation from the inputs).

Expected flags.  From the inputs alone for u1 = 0, u2 = 0 (r = 0 mod n), s = 0 (mod n), k = 0 (mod n) -- the sum ends on
the blinding point's multiple and the unblinding add subtracts a point from itself --, pk.x = 0 in the built-in programs
(beta * 0 = 0: the MSM table adds p to q = +-p) and pk = +-(blinding point) (the first table add is a doubling or meets
the neutral element).  For the other relatives of the blinding points, whose collisions depend on the scalar, and for
(0, 0) in the curve programs the flag is what the Python gadget walk (p2e_ref.Walker) raises.  No implementation's flag is
ever used.

Expected verdicts.  1 on every clean row built as valid (this includes msg + n, s + n and x + p: mul_nonnative and the
inverse generator read raw limbs and reduce, so the circuit computes the same u1, u2 and point); 0 where pk is off the
curve (curve_assert_valid's connect), where r >= n (r + n and all-ones: the canonical x of the result cannot equal it; the
rows are built from R.x < n) and, in glv_mul, for k >= n (the decomposition's connect compares raw k with its reduced
recomposition); None for tampered and degenerate rows.  The windowed and bit-wise programs have no verdict: valid is 1 on
every clean row.
    CAVEAT on x + p and s + n: verdict 1 there is the behaviour of the reference's WITNESS GENERATORS, not a satisfiable
circuit.  sub_nonnative connects diff + b with the raw a, and an early table add has the non-canonical pk.x on its left;
the inverse generator takes its quotient from the canonical s while the constraint multiplies the raw s.  The reference's
own constraints reject both witnesses (test_adversarial_cpu.py pins both halves); msg + n passes them.  A verdict of 1 on such a row
never means "the proof verifies".

Row counts obtained are in COUNTS below: (rows of classes(), rows of batch(), flagged rows of the batch); the flagged share
is 7.7 % for the built-in verifier and 7.8 .. 8.0 % for the others (70 of the flagged rows are the placed lanes and the
wave; the cap is 8 %, and batch() adds filler until it holds).  test_adversarial_cpu.py keeps COUNTS current."""
import functools

import numpy as np

import p2e_ref as R
from msm_inputs import sparse_values
from parity_checks import structured_values

CURVES = [R.SECP256K1, R.P256]
LAMBDA = R.GLV_S                       # k = k1 + LAMBDA k2 (mod n): lambda (x, y) = (beta x, y)
FLAG_CAP = 0.08
M256 = (1 << 256) - 1
COUNTS = {("verify", 0): (526, 1217, 94), ("glv_mul", 0): (356, 1089, 86), ("verify", 1): (503, 1089, 86),
          ("windowed", 0): (354, 1025, 82), ("windowed", 1): (341, 1025, 80), ("bitwise", 0): (354, 1025, 82),
          ("bitwise", 1): (341, 1025, 80)}
WALKER_KINDS = ("pk_blind_relative", "pk_origin_cp")       # flags taken from the Python gadget walk


class Case:
    __slots__ = ("kind", "args", "flagged", "valid", "u1", "u2")

    def __init__(self, kind, args, flagged, valid, u1=None, u2=None):
        self.kind, self.args, self.flagged, self.valid, self.u1, self.u2 = kind, tuple(args), flagged, valid, u1, u2


# ---- curve arithmetic on Python integers (Jacobian: the affine Curve.mul of p2e_ref inverts in every step) --------------
def _jdouble(cv, pt):
    x, y, z = pt
    if not y:
        return (0, 1, 0)
    p = cv.p
    s = 4 * x * y * y % p
    m = (3 * x * x + cv.a * pow(z, 4, p)) % p
    x3 = (m * m - 2 * s) % p
    return (x3, (m * (s - x3) - 8 * pow(y, 4, p)) % p, 2 * y * z % p)


def _jadd(cv, a, b):
    if not a[2]:
        return b
    if not b[2]:
        return a
    p = cv.p
    z1, z2 = a[2] * a[2] % p, b[2] * b[2] % p
    u1, u2 = a[0] * z2 % p, b[0] * z1 % p
    s1, s2 = a[1] * z2 * b[2] % p, b[1] * z1 * a[2] % p
    if u1 == u2:
        return _jdouble(cv, a) if s1 == s2 else (0, 1, 0)
    h, r = (u2 - u1) % p, (s2 - s1) % p
    h2 = h * h % p
    h3, v = h * h2 % p, u1 * h2 % p
    x3 = (r * r - h3 - 2 * v) % p
    return (x3, (r * (v - x3) - s1 * h3) % p, h * a[2] * b[2] % p)


def mul(cv, k, pt):
    """k * pt (affine, None = the neutral element): equal to p2e_ref's Curve.mul, asserted by the CPU test"""
    acc, q = (0, 1, 0), (pt[0], pt[1], 1)
    while k:
        if k & 1:
            acc = _jadd(cv, acc, q)
        q = _jdouble(cv, q)
        k >>= 1
    if not acc[2]:
        return None
    zi = pow(acc[2], -1, cv.p)
    return (acc[0] * zi * zi % cv.p, acc[1] * zi * zi * zi % cv.p)


def lift(cv, x, odd):
    """the point with abscissa x (mod p) and the given parity of y, or None"""
    x %= cv.p
    t = (x * x * x + cv.a * x + cv.b) % cv.p
    y = pow(t, (cv.p + 1) // 4, cv.p)                     # both moduli are 3 (mod 4)
    if y * y % cv.p != t:
        return None
    return (x, y if (y & 1) == odd else cv.p - y)


@functools.lru_cache(maxsize=None)
def blind(curve_id):
    """the blinding point of the curve programs in these tests (precompute_window's g / curve_scalar_mul's rando)"""
    cv = CURVES[curve_id]
    return mul(cv, 0xAD5E0 + curve_id, cv.g)


def forced(cv, kind, u1, u2, pk, valid=1, flagged=False):
    """the signature on which the circuit computes u1 and u2 (u2 != 0), for the curve point pk"""
    n = cv.n
    u1, u2 = u1 % n, u2 % n
    assert u2 and cv.on_curve(pk)
    pt = cv.add(mul(cv, u1, cv.g), mul(cv, u2, pk))
    assert pt is not None and 0 < pt[0] < n, "R.x must be a canonical non-zero scalar (r + n rows rely on it)"
    r = pt[0]
    s = r * pow(u2, -1, n) % n
    return Case(kind, (u1 * s % n, r, s, pk[0], pk[1]), flagged or u1 == 0, None if flagged or u1 == 0 else valid, u1, u2)


# ---- the value lists ---------------------------------------------------------------------------------------------------
def u1_values(cv):
    n = cv.n
    out = [("u1_edge", v) for v in (0, 1, 15, 16, n - 1, n - 2, (1 << 255) % n)]
    out += [("u1_one_window", d << (4 * w)) for d in (1, 15) for w in (0, 1, 31, 62, 63)]
    out += [("u1_structured", v % n) for v in structured_values(0xA1, 64)]
    out += [("u1_sparse", v % n) for v in sparse_values(0xA2, 64)]
    return out


def glv_grid():
    """+-k1 +- lambda k2 (mod n): (label, value) for every sign combination"""
    vals = []
    for k1 in (0, 1, 5, (1 << 126) | 1):
        for k2 in (0, 1, 7, (1 << 125) | 3):
            for s1 in (1, -1):
                for s2 in (1, -1):
                    vals.append((s1 * k1 + s2 * LAMBDA * k2) % R.N)
    return [("glv_grid", v) for v in dict.fromkeys(vals)]           # (k1 = 0 or k2 = 0: two signs give one value)


def u2_values(curve_id):
    """(kind, u2) without u2 = 0 (that row is r = 0, a raw-range row)"""
    cv = CURVES[curve_id]
    n = cv.n
    out = [("u2_edge", v) for v in (1, 2, 3, n - 1, n - 2, (1 << 127), (1 << 128) - 1)]
    if curve_id == 0:
        out += [("u2_edge", v) for v in (LAMBDA, n - LAMBDA, LAMBDA + 1, (5 - 7 * LAMBDA) % n)]
        out += [(k, v) for k, v in glv_grid() if v]
    else:
        rng = R.SplitMix64(0xA3)
        out += [("u2_top_digit", (d << 252) | (rng.below(n) >> 8)) for d in range(16)]
        out += [("u2_bottom_digit", ((rng.below(n) >> 4) << 4 | d)) for d in range(16)]
    out += [("u2_structured", v % n or 1) for v in structured_values(0xA4, 64)]
    out += [("u2_sparse", v % n or 1) for v in sparse_values(0xA5, 64)]
    return out


def raw_scalars(curve_id):
    """(kind, k) of the programs that take the scalar directly: raw 256-bit values"""
    cv = CURVES[curve_id]
    n = cv.n
    out = [("k_edge", v) for v in (0, 1, 2, n - 1, n, n + 1, M256, 1 << 127, 1 << 255)]
    if curve_id == 0:
        out += [("k_edge", LAMBDA), ("k_edge", n - LAMBDA)] + glv_grid()
    else:
        out += [("k_edge", (1 << 128) - 1), ("k_edge", n >> 1)]
        out += [("k_top_digit", (d << 252) | 0x123456789) for d in range(16)] + [("k_bottom_digit", (0x77 << 200) | d) for d in range(16)]
    out += [("k_structured", v) for v in structured_values(0xA6, 64)]
    out += [("k_sparse", v) for v in sparse_values(0xA7, 64)]
    return out


def public_keys(program, curve_id):
    """(kind, (x, y), on_curve): raw coordinates.  The degenerate points come last."""
    cv = CURVES[curve_id]
    p = cv.p
    out = []
    pts = [q for q in (lift(cv, x, i & 1) for i, x in enumerate(structured_values(0xA8, 400))) if q][:104]
    assert len(pts) >= 100 and {q[1] & 1 for q in pts} == {0, 1}
    out += [("pk_structured", q, True) for q in pts]
    small = [q for x in list(range(1, 41)) + list(range(p - 40, p)) for q in (lift(cv, x, x & 1),) if q]
    out += [("pk_small_x" if q[0] <= 40 else "pk_x_near_p", q, True) for q in small]
    out += [("pk_x_plus_p", (q[0] + p, q[1]), True) for q in small if q[0] <= 40 and q[0] + p <= M256]
    out += [("pk_generator", cv.g, True), ("pk_generator", cv.neg(cv.g), True)]
    off = (pts[0][0], pts[0][1] ^ 1)
    out += [("pk_off_curve", off, False), ("pk_all_ones", (M256, M256), False)]
    if program in ("verify", "glv_mul") and curve_id == 0:
        rando = R.rando_point()
        out += [("pk_blind", rando, True), ("pk_blind", cv.neg(rando), True), ("pk_origin", (0, 0), False)]
        rel = [cv.double(rando), cv.neg(cv.double(rando)), mul(cv, 3, rando)]
    else:
        g = blind(curve_id)
        out += [("pk_blind", g, True), ("pk_blind", cv.neg(g), True), ("pk_origin_cp", (0, 0), False)]
        rel = [cv.double(g)]
    out += [("pk_blind_relative", q, True) for q in rel]
    return out


def _walk_flags(program, curve_id, args):
    """True where the Python gadget walk of the reference panics"""
    cv = CURVES[curve_id]
    try:
        if program == "verify":
            R.verify_witness(*args) if curve_id == 0 else R.verify_p256_witness(*args, blind(curve_id))
        elif program == "glv_mul":
            R.glv_mul_witness(*args)
        elif program == "windowed":
            R.windowed_mul_witness(cv, *args, blind(curve_id))
        else:
            R.scalar_mul_witness(cv, *args, blind(curve_id))
    except R.RefPanic:
        return True
    return False


# ---- the classes -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def classes(program, curve_id):
    """the named rows of one program (a tuple of Case); the eight rows of test_gpu_parity.py's
    test_edge_inputs_and_error_flags are among those of the built-in verifier (kind "parity_edge")"""
    cv = CURVES[curve_id]
    n, p = cv.n, cv.p
    rng = R.SplitMix64(0xADE0 + 16 * curve_id + len(program))
    keys = public_keys(program, curve_id)
    good = [q for kind, q, _on in keys if kind == "pk_structured"]
    out = []
    if program in ("glv_mul", "windowed", "bitwise"):
        nth = lambda i: good[i % len(good)]
        for i, (kind, k) in enumerate(raw_scalars(curve_id)):
            q = nth(i)
            kn = k % n
            valid = 0 if program == "glv_mul" and k >= n else 1
            out.append(Case(kind, (q[0], q[1], k), kn == 0, None if kn == 0 else valid))
        for kind, q, on in keys:
            k = rng.below(n)
            if kind in WALKER_KINDS:
                fl = _walk_flags(program, curve_id, (q[0], q[1], k))
            else:
                fl = kind == "pk_blind" or (kind == "pk_origin")
            # off the curve: these programs do not assert validity; their verdict is the decomposition's alone
            out.append(Case(kind, (q[0], q[1], k), fl, None if fl else 1))
        return tuple(out)
    # the verifiers
    some_key = lambda: good[rng.next() % len(good)]
    for kind, u1 in u1_values(cv):
        out.append(forced(cv, kind, u1, rng.below(n), some_key()))
    for kind, u2 in u2_values(curve_id):
        out.append(forced(cv, kind, rng.below(n), u2, some_key()))
    for kind, q, on in keys:
        u1, u2 = rng.below(n), rng.below(n)
        if on:
            base = forced(cv, kind, u1, u2, (q[0] % p, q[1]))
            args = base.args[:3] + (q[0], q[1])
        else:
            args = forced(cv, kind, u1, u2, good[0]).args[:3] + (q[0], q[1])
        if kind in WALKER_KINDS:
            fl = _walk_flags(program, curve_id, args)
        else:
            fl = kind == "pk_blind" or kind == "pk_origin"
        out.append(Case(kind, args, fl, None if fl else (1 if on else 0), u1, u2))
    # raw ranges.  v + n fits in 256 bits only for v < 2^256 - n (about 2^128 / 2^224), so msg and s are CHOSEN small on
    # a signature with a known key: pk = d G, R = k G, then s = (msg + r d) / k or msg = s k - r d.  A small r cannot be
    # built (it is an abscissa): r + n stands on a small r that belongs to no signature, verdict 0 either way.
    for j in range(2):
        d, k, small = rng.below(n), rng.below(n), rng.below(n) >> (156 - 20 * j)
        pk, pt = mul(cv, d, cv.g), mul(cv, k, cv.g)
        r = pt[0]
        assert 0 < r < n
        s_ = (small + r * d) * pow(k, -1, n) % n
        out.append(Case("msg_plus_n", (small + n, r, s_, pk[0], pk[1]), False, 1, small * pow(s_, -1, n) % n, r * pow(s_, -1, n) % n))
        m_ = (small * k - r * d) % n
        out.append(Case("s_plus_n", (m_, r, small + n, pk[0], pk[1]), False, 1, m_ * pow(small, -1, n) % n, r * pow(small, -1, n) % n))
        out.append(Case("r_plus_n", (m_, small + n, s_, pk[0], pk[1]), False, 0))
    assert all(max(c.args) <= M256 for c in out)
    c = forced(cv, "s_zero", rng.below(n), rng.below(n), some_key())
    out.append(Case("s_zero", c.args[:2] + (0,) + c.args[3:], True, None))
    out.append(Case("s_zero", c.args[:2] + (n,) + c.args[3:], True, None))
    out.append(Case("u2_zero", (c.args[0], 0) + c.args[2:], True, None))
    out.append(Case("u2_zero", (c.args[0], n) + c.args[2:], True, None))
    out.append(Case("all_ones", (M256,) * 5, False, 0))
    # untouched synthetic signatures, and the rows of the parity test's edge case
    synth = (lambda i: R.synth_signature_at(5, i)) if curve_id == 0 else (lambda i, g=R.SplitMix64(0x5E): R.synth_signature_curve(cv, g))
    for i in range(10):
        out.append(Case("synthetic", synth(i), False, 1))
    if curve_id == 0:
        sig = list(R.synth_signature_at(5, 0))
        rx, ry = R.rando_point()
        out.append(Case("parity_edge", (sig[0], (sig[1] + 1) % n) + tuple(sig[2:]), False, 0))      # does not verify
        out.append(Case("parity_edge", (sig[0], sig[1], 1, sig[3], sig[4]), False, None))             # s = 1
        out.append(Case("parity_edge", (sig[0], sig[1], sig[2], R.GX, R.GY), False, None))            # pk = G
        out.append(Case("parity_edge", (sig[0], sig[1], sig[2], rx, (-ry) % p), True, None))          # pk = -rando
        out.append(Case("parity_edge", (sig[0], sig[1], 0, sig[3], sig[4]), True, None))              # s = 0
        # (its first, seventh and eighth rows are "synthetic" 0, "all_ones" and "synthetic" 1 above)
    return tuple(out)


def filler(program, curve_id, count):
    """clean rows built as valid: forced signatures with sparse / structured u1, u2 on structured public keys"""
    cv = CURVES[curve_id]
    rng = R.SplitMix64(0xF111 + curve_id)
    good = [q for kind, q, _on in public_keys(program, curve_id) if kind == "pk_structured"]
    vals = [v % cv.n or 1 for v in structured_values(0xA9, count) + sparse_values(0xAA, count)]
    out = []
    for i in range(count):
        q = good[(7 * i) % len(good)]
        if program == "verify":
            out.append(forced(cv, "filler", vals[i] if i & 1 else rng.below(cv.n), vals[count + i], q))
        else:
            out.append(Case("filler", (q[0], q[1], vals[i] if i & 1 else rng.below(cv.n)), False, 1))
    return out


def flagged_rows(program, curve_id, count):
    """rows the reference panics on, by the simple rules, in turn: s = 0, u1 = 0, pk = -blinding point, u2 = 0 for the
    verifiers; k = 0, k = n, p = +-blinding point for the others.  (The placed lanes of the bit-wise program use k = 0 and
    k = n only, to keep two kinds of lane; p = +-blinding point is flagged there as well -- bit 0 always computes
    result + p -- and classes() has those rows.)"""
    cv = CURVES[curve_id]
    base = [c for c in classes(program, curve_id) if c.kind in ("u1_structured", "k_structured") and not c.flagged]
    bl = R.rando_point() if curve_id == 0 and program in ("verify", "glv_mul") else blind(curve_id)
    nb = cv.neg(bl)
    out = []
    for i in range(count):
        a = list(base[i % len(base)].args)
        j = i % 4
        if program == "verify":
            if j == 0:
                a[2] = 0
            elif j == 1:
                a[0] = 0
            elif j == 2:
                a[3], a[4] = nb
            else:
                a[1] = cv.n
        else:
            if j == 0 or (j >= 2 and program == "bitwise"):
                a[2] = 0
            elif j == 1:
                a[2] = cv.n
            else:
                a[0], a[1] = bl if j == 2 else nb
        out.append(Case("flagged_lane", a, True, None))
    return out


@functools.lru_cache(maxsize=None)
def batch(program, curve_id):
    """(cases, marks): the classes at the start of the batch and again, reversed, at its end, clean filler between, and
    flagged rows placed in the first lane, the last lane, lanes 63 and 64 (last / first signature of neighbouring
    four-lane workgroups), two adjacent lanes, and one whole aligned wave of 64 -- each with a clean row on either side.
    marks names those lanes.  The size is 1 (mod 64): ragged for every workgroup shape."""
    cl = list(classes(program, curve_id))
    # clean rows where a neighbour of a marked lane falls: rotate the classes so that rows 0, 61, 62 are clean
    clean = [c for c in cl if not c.flagged]
    dirty = [c for c in cl if c.flagged]
    cl = clean[:70] + [c for c in cl if c not in clean[:70]]
    assert len(cl) == len(clean) + len(dirty)
    fl = flagged_rows(program, curve_id, 64 + 6)
    extra = 0
    while True:                                             # more filler until the flagged share is under the cap
        rows = [fl[0]] + cl[:62] + [fl[1], fl[2]] + cl[62:]
        marks = {"first": 0, "pair_63_64": 63}
        fill = iter(filler(program, curve_id, 64 + 64 + 8 + extra + 64))
        rows.append(next(fill))
        marks["adjacent"] = len(rows)
        rows += [fl[3], fl[4], next(fill)]
        while len(rows) % 64:
            rows.append(next(fill))
        marks["wave"] = len(rows)
        rows += fl[6:70] + [next(fill) for _ in range(1 + extra)]
        rows += cl[::-1]
        while len(rows) % 64:                                   # then the last lane makes it 1 (mod 64)
            rows.append(next(fill))
        rows.append(fl[5])
        marks["last"] = len(rows) - 1
        if sum(c.flagged for c in rows) <= FLAG_CAP * len(rows):
            break
        extra += 64
    fs = [c.flagged for c in rows]
    for name, (a, k) in {"first": (0, 1), "pair_63_64": (63, 2), "adjacent": (marks["adjacent"], 2), "wave": (marks["wave"], 64),
                         "last": (len(rows) - 1, 1)}.items():
        assert all(fs[a:a + k]), name
        assert (a == 0 or not fs[a - 1]) and (a + k == len(rows) or not fs[a + k]), name + ": neighbours must be clean"
    assert marks["wave"] % 64 == 0 and len(rows) % 64 == 1
    assert sum(fs) <= FLAG_CAP * len(rows), (sum(fs), len(rows))
    return tuple(rows), marks


def arrays(cases):
    """list of Case -> the program's input arrays, each (n, 32) uint8 little-endian"""
    k = len(cases[0].args)
    return [np.frombuffer(b"".join(int(c.args[j]).to_bytes(32, "little") for c in cases), np.uint8).reshape(-1, 32).copy()
            for j in range(k)]


def expected(cases):
    """(flagged as a bool array, the indices with an expected verdict, those verdicts)"""
    fl = np.array([c.flagged for c in cases], bool)
    idx = np.array([i for i, c in enumerate(cases) if c.valid is not None and not c.flagged], np.int64)
    return fl, idx, np.array([cases[i].valid for i in idx], np.uint8)


def named_rows(program, curve_id):
    """{name: index into batch()} of clean valid rows with a property the other passes are run on"""
    cases, _ = batch(program, curve_id)
    cv = CURVES[curve_id]
    out = {}
    for i, c in enumerate(cases):
        if c.flagged or c.valid != 1:
            continue
        u2 = c.u2 if program == "verify" else c.args[2] % cv.n
        u1 = c.u1 if program == "verify" else None
        if curve_id == 0 and program in ("verify", "glv_mul") and u2:
            k1, k2, n1, n2 = R.glv_decompose(u2)
            if k1 == 0:
                out.setdefault("k1_zero", i)
            if k2 == 0:
                out.setdefault("k2_zero", i)
            if k1 and k2:
                out.setdefault(("no_sign", "n1_only", "n2_only", "both_signs")[n1 + 2 * n2], i)
        if u1 is not None:
            if c.kind == "u1_one_window":
                out.setdefault("one_window_u1", i)
            windows = [(u1 >> (4 * w)) & 15 for w in range(64)]
            if u1 >> 200 and all(0 in windows[g:g + 16] and any(windows[g:g + 16]) for g in range(0, 64, 16)):
                out.setdefault("zero_window_every_group", i)      # (and a non-zero one: no group is empty)
            if u1 == cv.n - 1:
                out.setdefault("u1_n_minus_1", i)
        if u2 == cv.n - 1:
            out.setdefault("u2_n_minus_1", i)
        if c.kind in ("pk_x_near_p", "pk_x_plus_p", "pk_small_x", "pk_generator", "msg_plus_n", "s_plus_n"):
            out.setdefault(c.kind, i)
        if c.kind in ("u2_sparse", "k_sparse"):
            out.setdefault("sparse", i)
        if c.kind in ("u2_structured", "k_structured"):
            out.setdefault("structured", i)
    return out
