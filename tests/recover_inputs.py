"""Inputs and independent expectations of the recovery tests (test_recover_cpu.py, test_gpu_recover.py).

Nothing here uses the code under test.

Set S (signatures with known keys): (msg, sk, k) batches of tests/sign_inputs.py (same seeds as the signing tests, so the
    per-session point cache is shared); pk = sk G and R = k G, both coordinates, from sign_inputs.base_points (the C oracle's
    fixed-base walk), s from Python integers, v from R.  Expected output: pk.  The expected flags come from the inputs alone:
    k = 0 (mod n) gives r = s = 0 -> NOT_RECOVERABLE; r = 0 or s = 0 -> NOT_RECOVERABLE; else sk = 0 (mod n) -> the key is
    the neutral element -> POINT_AT_INFINITY.  Every element has a twin in low-s form (r, n - s, v ^ 1), same expectation.
Set X (synthetic): expectation = recover_ref below, the definition of include/p2e.h written with Python integers and
    oracle/p2e_ref.py's Curve.mul / Curve.add.  The cases are built from R = k G with known k and chosen u1, u2 through
    s = u2 r, msg = -u1 r; for those the structural expectation ((u1 + u2 k) G, 2 u1 G, the neutral element) is asserted
    against recover_ref by test_recover_cpu.py::test_input_sets_cover_what_they_claim."""
import functools

import numpy as np

import p2e_ref as R
import sign_inputs as S

CURVES = S.CURVES
ERR_INVERSE_OF_ZERO, ERR_POINT_AT_INFINITY, ERR_NOT_RECOVERABLE = 4, 64, 128
# small r for which r + n is an abscissa (among 1 .. OVERFLOW_RANGE exactly these), and small non-residue abscissas
OVERFLOW_R = [[2, 4, 6], [3, 4, 6, 9]]
OVERFLOW_RANGE = [6, 9]
NON_RESIDUE_X = [[5, 7, 9, 10], [1, 2, 3, 4]]
DIGIT_WINDOWS = (0, 1, 63, 64, 126, 127)


def is_abscissa(cv, x):
    t = (x * x * x + cv.a * x + cv.b) % cv.p
    return x < cv.p and pow(t, (cv.p - 1) // 2, cv.p) in (0, 1)


def recover_ref(cv, msg, r, s, v):
    """((pkx, pky), err) of one raw (msg, r, s, v): zeros where err != 0"""
    n, p = cv.n, cv.p
    if r == 0 or r >= n or s == 0 or s >= n or v > 3:
        return (0, 0), ERR_NOT_RECOVERABLE
    x = r + n * (v >> 1)
    if x >= p or not is_abscissa(cv, x):
        return (0, 0), ERR_NOT_RECOVERABLE
    y = pow((x * x * x + cv.a * x + cv.b) % p, (p + 1) // 4, p)
    if y & 1 != v & 1:
        y = p - y
    assert cv.on_curve((x, y))
    rinv = pow(r, -1, n)
    u1, u2 = -(msg % n) * rinv % n, s * rinv % n
    pk = cv.add(cv.mul(u1, cv.g), cv.mul(u2, (x, y)))
    if pk is None:
        return (0, 0), ERR_POINT_AT_INFINITY
    return pk, 0


class Case:
    __slots__ = ("kind", "msg", "r", "s", "v", "pk", "err", "k", "u1", "u2")

    def __init__(self, kind, msg, r, s, v, pk, err, k=None, u1=None, u2=None):
        self.kind, self.msg, self.r, self.s, self.v, self.pk, self.err, self.k, self.u1, self.u2 = kind, msg, r, s, v, pk, err, k, u1, u2


@functools.lru_cache(maxsize=None)
def set_x(curve_id):
    """the synthetic cases of one curve, computed once per session (a tuple of Case)"""
    cv = CURVES[curve_id]
    n, p = cv.n, cv.p
    rng = R.SplitMix64(0xEC0 + curve_id)
    out = []

    def raw(kind, msg, r, s, v, **kw):
        pk, err = recover_ref(cv, msg, r, s, v)
        out.append(Case(kind, msg, r, s, v, pk, err, **kw))

    def forced(kind, u1, u2, k=None, flip=False):
        """the signature with R = k G (v ^ 1 if flip: R = -k G) for which the recovery computes u1 G + u2 R"""
        k = k or 1 + rng.below(n - 1)
        x, y = cv.mul(k, cv.g)
        r = x % n
        assert r and u2 % n
        v = (y & 1) | (2 if x >= n else 0)
        raw(kind, -u1 * r % n, r, u2 * r % n, v ^ 1 if flip else v, k=(n - k if flip else k), u1=u1 % n, u2=u2 % n)

    for u2 in (1, 2, 3, 4, 5, 15, 16, n - 1, n - 2, (1 << 255) % n):
        forced("u2_small", rng.below(n), u2)
        forced("u2_small_flip", rng.below(n), u2, flip=True)
    for w in DIGIT_WINDOWS:
        for d in (1, 2, 3):
            forced("u2_digit", rng.below(n), d << (2 * w))
    for _ in range(3):
        forced("u2_zero_top", rng.below(n), (rng.below(n) >> 2) | 1)
    for d in (1, 2, 3):
        forced("u2_top_only", rng.below(n), d << 254, flip=d == 2)
    for u1 in (0, 1, n - 1):
        forced("u1_edge", u1, 1 + rng.below(n - 1))
        forced("u1_edge_flip", u1, 1 + rng.below(n - 1), flip=True)
    for d, w in ((1, 0), (15, 0), (7, 31), (1, 63), (15, 63)):
        forced("u1_nibble", d << (4 * w), 1 + rng.below(n - 1))
    for j in range(4):
        k, u2 = 1 + rng.below(n - 1), (3, 1 + rng.below(n - 1), n - 1, 1 + rng.below(n - 1))[j]
        forced("doubling", u2 * k % n, u2, k=k)
    for j in range(4):
        k, u2 = 1 + rng.below(n - 1), (2, 1 + rng.below(n - 1), n - 1, 1 + rng.below(n - 1))[j]
        forced("neutral", -u2 * k % n, u2, k=k)
    for _ in range(20):
        forced("random", rng.below(n), 1 + rng.below(n - 1), flip=bool(rng.next() & 1))
    # the overflow bit: x = r + n
    small = sorted(set(OVERFLOW_R[curve_id]) | set(range(1, OVERFLOW_RANGE[curve_id] + 1)))
    for r in small:
        for v in (0, 1, 2, 3):
            raw("overflow" if v & 2 else "no_overflow", rng.below(n), r, 1 + rng.below(n - 1), v)
    for x in NON_RESIDUE_X[curve_id]:
        for v in (0, 1):
            raw("non_residue", rng.below(n), x, 1 + rng.below(n - 1), v)
    for r in (p - n, p - n + 5, n - 1, p - n - 1):          # the last: x = p - 1 < p, an abscissa or not as it may be
        for v in (2, 3):
            raw("x_ge_p" if r + n >= p else "x_below_p", rng.below(n), r, 1 + rng.below(n - 1), v)
    # ranges of r, s and v on an otherwise well-formed signature
    k = 1 + rng.below(n - 1)
    gx, gy = cv.mul(k, cv.g)
    good = dict(msg=rng.below(n), r=gx % n, s=1 + rng.below(n - 1), v=(gy & 1) | (2 if gx >= n else 0))
    raw("well_formed", **good)
    for r in (n, (1 << 256) - 1, 0):
        raw("r_range", **dict(good, r=r))
    for s in (n, 0, (1 << 256) - 1):
        raw("s_range", **dict(good, s=s))
    for v in (4, 27, 255, good["v"] | 4):
        raw("v_range", **dict(good, v=v))
    for m in (rng.below(n) % ((1 << 256) - n), 0, (1 << 256) - n - 1):
        raw("msg_ge_n", **dict(good, msg=n + m))
        raw("msg_reduced", **dict(good, msg=m))
    return tuple(out)


def set_s(curve_id, total, seeds, indices):
    """elements `indices` of the signing tests' batch (sign_inputs.batch with `seeds` = (sk, k, msg) seeds): list of Case,
    every element followed by nothing -- the twins come from low_s()"""
    cv = CURVES[curve_id]
    n = cv.n
    sk, k = S.batch(cv, total, seeds[0], shift=1), S.batch(cv, total, seeds[1])
    msg = S.batch(cv, total, seeds[2], shift=500)
    red = [(msg[i], sk[i] % n, k[i] % n) for i in indices]
    pts = S.base_points(curve_id, [d for _m, d, _k in red] + [kk for _m, _d, kk in red])
    out = []
    for m, d, kk in red:
        if kk == 0:
            out.append(Case("S_k_zero", m, 0, 0, 0, (0, 0), ERR_NOT_RECOVERABLE))
            continue
        x, y = pts[kk]
        r = x % n
        s = pow(kk, -1, n) * (m % n + r * d) % n
        v = (y & 1) | (2 if x >= n else 0)
        if r == 0 or s == 0:
            out.append(Case("S_zero", m, r, s, v, (0, 0), ERR_NOT_RECOVERABLE))
        elif d == 0:
            out.append(Case("S_sk_zero", m, r, s, v, (0, 0), ERR_POINT_AT_INFINITY))
        else:
            out.append(Case("S", m, r, s, v, pts[d], 0))
    return out


def low_s(curve_id, cases):
    """(r, n - s, v ^ 1) of every case, same expectation (n - 0 = n is as unrecoverable as 0)"""
    n = CURVES[curve_id].n
    return [Case(c.kind + "_twin", c.msg, c.r, n - c.s, c.v ^ 1, c.pk, c.err) for c in cases]


def arrays(cases):
    """list of Case -> dict of numpy arrays: msg, r, s (n, 32), v (n,), pkx, pky (n, 32), err (n,)"""
    return dict(msg=S.pack([c.msg for c in cases]), r=S.pack([c.r for c in cases]), s=S.pack([c.s for c in cases]),
                v=np.array([c.v for c in cases], np.uint8), pkx=S.pack([c.pk[0] for c in cases]),
                pky=S.pack([c.pk[1] for c in cases]), err=np.array([c.err for c in cases], np.uint8))


def selftest_vectors():
    """the text of tests/emu_recover/recover_vectors.inc: set X of both curves as C initialisers"""
    lines = ["// generated by tests/recover_inputs.py selftest_vectors() from set X (test_recover_cpu.py keeps it current)",
             "// {curve, msg, r, s, v, pkx, pky, err}: 256-bit values as big-endian hex"]
    for curve_id in (0, 1):
        for c in set_x(curve_id):
            lines.append('{%d, "%064x", "%064x", "%064x", %d, "%064x", "%064x", %d},' % (curve_id, c.msg, c.r, c.s, c.v, c.pk[0], c.pk[1], c.err))
    return "\n".join(lines) + "\n"
