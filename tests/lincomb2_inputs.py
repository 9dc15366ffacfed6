"""Inputs and independent expectations of the tests of include/p2e.h p2e_point_lincomb2_batch, out = a P + b Q
(test_lincomb2_cpu.py, test_gpu_lincomb2.py).  Nothing here uses the code under test.

The operands are those of point_arith_inputs.py (fixed points with known logarithms, edge scalars, scalars chosen by their GLV
decomposition, invalid points), extended to where ONE walk over two points can go wrong and two separate walks cannot: Q = +-P
and, on secp256k1, Q = +-lambda P (entries of the two operands coincide or cancel in the middle of the walk), a = b, a = n - b,
a P = -b Q (the neutral result), zero scalars, neutral operands, halves of the decompositions at the 128-bit bound.

The expectation is `expect`: the header's definition in Python integers on oracle/p2e_ref.py's Curve.mul / Curve.add.  Every
operand here is t G for a t this file knows (or neutral), so the expectation is cross-checked by a different multiplication:
a P + b Q = ((a t_P + b t_Q) mod n) G, the neutral element where that scalar is 0 (`cross_check`)."""
import functools

import numpy as np

import p2e_ref as R
import point_arith_inputs as PA
import sign_inputs as S

CURVES = PA.CURVES
WIRE_OK, WIRE_COORD_RANGE, WIRE_NOT_ON_CURVE, WIRE_INFINITY = 0, 3, 4, 5
PLANS = PA.PLANS
O = PA.O
LAMBDA = PA.LAMBDA
SIZES = (0, 1, 63, 64, 65, 257)


class Case:
    __slots__ = ("kind", "a", "b", "p", "q", "tp", "tq", "out", "err")

    def __init__(self, kind, a, b, p, q, tp, tq, out, err):
        self.kind, self.a, self.b, self.p, self.q, self.tp, self.tq, self.out, self.err = kind, a, b, p, q, tp, tq, out, err


def expect(cv, a, b, p, q):
    """((outx, outy), code) of one raw element: P is checked before Q, whatever the scalars are"""
    e = PA.check(cv, p) or PA.check(cv, q)
    if e:
        return O, e
    r = cv.add(cv.mul(a % cv.n, p) if p != O else None, cv.mul(b % cv.n, q) if q != O else None)
    return (O, WIRE_INFINITY) if r is None else (r, WIRE_OK)


def glv_bound_scalars():
    """secp256k1: scalars whose halves reach the bound of csrc/point_arith.hpp, |k1| <= (a1 + a2) / 2, |k2| <= (|b1| + b2) / 2:
    k = e1 v1 + e2 v2 with e1, e2 next to +-1/2 decomposes into the corner of the fundamental cell"""
    out = []
    a1, b1, a2, b2 = R.GLV_A1, -R.GLV_MINUS_B1, R.GLV_A2, R.GLV_A1     # v1 = (a1, b1), v2 = (a2, b2), b2 = a1
    for s1 in (1, -1):
        for s2 in (1, -1):
            for d in (0, 1, 2):
                k1 = (s1 * (a1 - d) + s2 * (a2 - d)) // 2
                k2 = (s1 * (b1 + d * s1) + s2 * (b2 - d)) // 2
                out.append((k1 + k2 * LAMBDA) % R.N)
    return out


@functools.lru_cache(maxsize=None)
def cases(curve_id):
    """the synthetic cases of one curve, computed once per session (a tuple of Case)"""
    cv = CURVES[curve_id]
    n = cv.n
    rng = R.SplitMix64(0x2B0B + curve_id)
    out = []

    def case(kind, a, b, p, q, tp=None, tq=None):
        o, e = expect(cv, a, b, p, q)
        out.append(Case(kind, a, b, p, q, tp, tq, o, e))

    def rnd():
        return 1 + rng.below(n - 1)

    pts = PA.fixed_points(curve_id)                                   # (kind, point, logarithm)
    bad = PA.invalid_points(curve_id)
    for pkind, pt, t in pts:
        a, b = rnd(), rnd()
        case("Q_eq_P/" + pkind, a, b, pt, pt, t, t)
        case("Q_eq_minus_P/" + pkind, a, b, pt, cv.neg(pt), t, n - t)
        case("Q_eq_P_a_eq_b/" + pkind, a, a, pt, pt, t, t)
        case("Q_eq_P_a_eq_n_minus_b/" + pkind, a, n - a, pt, pt, t, t)               # a P = -b Q: neutral
        case("Q_eq_minus_P_a_eq_b/" + pkind, a, a, pt, cv.neg(pt), t, n - t)         # neutral
        case("Q_eq_minus_P_a_eq_n_minus_b/" + pkind, a, n - a, pt, cv.neg(pt), t, n - t)   # doubled
        if curve_id == 0:
            lp, tl = (PA.BETA * pt[0] % cv.p, pt[1]), LAMBDA * t % n
            assert lp == cv.mul(LAMBDA, pt)
            case("Q_eq_lambda_P/" + pkind, a, b, pt, lp, t, tl)
            case("Q_eq_minus_lambda_P/" + pkind, a, b, pt, cv.neg(lp), t, n - tl)
            case("Q_eq_lambda_P_a_eq_b/" + pkind, a, a, pt, lp, t, tl)
            case("Q_eq_lambda_P_cancel/" + pkind, a * LAMBDA % n, n - a, pt, lp, t, tl)   # a lambda P - a (lambda P): neutral
            case("Q_eq_lambda_P_double/" + pkind, a * LAMBDA % n, a, pt, lp, t, tl)
            case("Q_eq_lambda_P_swap/" + pkind, LAMBDA, n - 1, pt, lp, t, tl)             # lambda P - lambda P
    for i, (pkind, pt, t) in enumerate(pts[:5:2]):                    # G, 2 G and a random point against random points
        qkind, qt, u = pts[3 + i]
        a, b = rnd(), rnd()
        case("generic/%s/%s" % (pkind, qkind), rng.below(1 << 256), rng.below(1 << 256), pt, qt, t, u)
        case("a_eq_b/" + pkind, a, a, pt, qt, t, u)
        case("a_eq_n_minus_b/" + pkind, a, n - a, pt, qt, t, u)
        case("opposite/" + pkind, a, (n - a * t * pow(u, -1, n)) % n, pt, qt, t, u)      # a P = -b Q
        case("doubling/" + pkind, a, a * t * pow(u, -1, n) % n, pt, qt, t, u)            # a P = b Q
        case("a_zero/" + pkind, 0, b, pt, qt, t, u)
        case("b_zero/" + pkind, a, 0, pt, qt, t, u)
        case("both_zero/" + pkind, 0, 0, pt, qt, t, u)
        case("both_n/" + pkind, n, n, pt, qt, t, u)
        case("P_neutral/" + pkind, a, b, O, qt, 0, u)
        case("Q_neutral/" + pkind, a, b, pt, O, t, 0)
        case("P_neutral_b_zero/" + pkind, a, 0, O, qt, 0, u)
    case("both_neutral", rnd(), rnd(), O, O, 0, 0)
    scalars = PA.edge_scalars(cv)                                     # 0, 1, 2, 3, n - 1, n, 2^256 - 1 among them
    assert {1, 2, 3, n - 1, n, (1 << 256) - 1} <= set(scalars)
    if curve_id == 0:
        scalars = scalars + [k for _kind, k in PA.glv_scalars()] + glv_bound_scalars()   # lambda and lambda^2 among them
        assert {LAMBDA, LAMBDA * LAMBDA % n} <= set(scalars)
    for j, k in enumerate(scalars):                                   # every scalar once as a and once as b
        _, pt, t = pts[3 + j % 3]
        _, qt, u = pts[3 + (j + 1) % 3]
        case("scalars", k, scalars[(j + 5) % len(scalars)], pt, qt, t, u)
    for pkind, pt in bad:
        case("P_invalid/" + pkind, rnd(), rnd(), pt, pts[3][1])
        case("Q_invalid/" + pkind, rnd(), rnd(), pts[4][1], pt)
        case("Q_invalid_P_neutral/" + pkind, 0, 0, O, pt)
    for (ka, pa), (kb, pb) in zip(bad, bad[1:] + bad[:1]):
        case("both_invalid/%s/%s" % (ka, kb), rnd(), rnd(), pa, pb)
    return tuple(out)


def cross_check(curve_id, cs):
    """a P + b Q = ((a t_P + b t_Q) mod n) G through the C oracle's fixed-base walk, for every case whose operands are valid"""
    cv = CURVES[curve_id]
    good = [c for c in cs if c.tp is not None]
    ks = [(c.a % cv.n * c.tp + c.b % cv.n * c.tq) % cv.n for c in good]
    pts = S.base_points(curve_id, ks)
    for c, k in zip(good, ks):
        want = (O, WIRE_INFINITY) if pts[k] is None else (pts[k], WIRE_OK)
        assert (c.out, c.err) == want, c.kind
    return len(good)


@functools.lru_cache(maxsize=None)
def _filler(curve_id, count):
    cv = CURVES[curve_id]
    rng = R.SplitMix64(0x2F11 + curve_id)
    ts = [1 + rng.below(cv.n - 1) for _ in range(count + 1)]
    pts = S.base_points(curve_id, ts)
    out = []
    for i in range(count):
        a, b = rng.below(1 << 256), rng.below(1 << 256)
        p, q = pts[ts[i]], pts[ts[i + 1]]
        o, e = expect(cv, a, b, p, q)
        out.append(Case("F", a, b, p, q, ts[i], ts[i + 1], o, e))
    return tuple(out)


def batch(curve_id, total):
    """`total` cases: the synthetic ones (cut where total is smaller; flagged and good lanes mix in the first wave), then filler"""
    x = list(cases(curve_id))
    # interleave so that a prefix of any length holds special cases of every group
    step = 7
    x = [x[(i * step) % len(x)] for i in range(len(x))] if len(x) % step else x
    if total <= len(x):
        return x[:total]
    return x + list(_filler(curve_id, total - len(x)))


def arrays(cs):
    """list of Case -> dict of (n, 32) uint8 arrays a, b, px, py, qx, qy, outx, outy and err (n,)"""
    pk = S.pack
    return dict(a=pk([c.a for c in cs]), b=pk([c.b for c in cs]), px=pk([c.p[0] for c in cs]), py=pk([c.p[1] for c in cs]),
                qx=pk([c.q[0] for c in cs]), qy=pk([c.q[1] for c in cs]), outx=pk([c.out[0] for c in cs]),
                outy=pk([c.out[1] for c in cs]), err=np.array([c.err for c in cs], np.uint8))
