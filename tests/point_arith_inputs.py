"""Inputs and independent expectations of the point-arithmetic tests (test_point_arith_cpu.py, test_gpu_point_arith.py):
include/p2e.h p2e_point_mul_batch (out = k P), p2e_point_lincomb_batch (out = a G + b P), p2e_point_add_batch (out = P + Q).

Nothing here uses the code under test.

Set X (synthetic, per curve and call): the expectation is `expect` below, the definition of include/p2e.h written with Python
    integers on oracle/p2e_ref.py's Curve.mul / Curve.add.  Scalars at the edges of the reduction and of the windows, on
    secp256k1 also scalars chosen by their GLV decomposition (p2e_ref.glv_decompose: lambda and its neighbours, every sign
    combination, an empty half, equal halves); G, -G, 2 G, fixed random points and the neutral element (0, 0); points out
    of range and off the curve; for a G + b P and P + Q every defined special case of the header.
Set F (filler): P_i = t_i G with known t_i drawn from a seed, Q_i = P_(i+1); the expectations (k_i t_i) G, (a_i + b_i t_i) G
    and (t_i + t_(i+1)) G come from the C oracle's fixed-base walk (sign_inputs.base_points), independent of any
    variable-base code."""
import functools

import numpy as np

import p2e_ref as R
import sign_inputs as S

CURVES = S.CURVES
WIRE_OK, WIRE_COORD_RANGE, WIRE_NOT_ON_CURVE, WIRE_INFINITY = 0, 3, 4, 5
PLAN_AUTO, PLAN_PLAIN, PLAN_GLV = 0, 1, 2
PLANS = [(PLAN_AUTO, PLAN_PLAIN, PLAN_GLV), (PLAN_AUTO, PLAN_PLAIN)]          # per curve
O = (0, 0)                                                                    # the neutral element on the wire
# lambda = a1 / (-b1) (mod n) from the basis of glv_decompose; beta: lambda G = (beta G.x, G.y)
LAMBDA = R.GLV_A1 * pow(R.GLV_MINUS_B1, -1, R.N) % R.N
BETA = R.SECP256K1.mul(LAMBDA, R.SECP256K1.g)[0] * pow(R.SECP256K1.g[0], -1, R.P) % R.P


class Case:
    __slots__ = ("op", "kind", "a", "b", "p", "q", "out", "err")

    def __init__(self, op, kind, a, b, p, q, out, err):
        self.op, self.kind, self.a, self.b, self.p, self.q, self.out, self.err = op, kind, a, b, p, q, out, err


def check(cv, pt):
    """the code of one operand: range first, then the curve equation; (0, 0) is fine"""
    if pt == O:
        return WIRE_OK
    if pt[0] >= cv.p or pt[1] >= cv.p:
        return WIRE_COORD_RANGE
    return WIRE_OK if cv.on_curve(pt) else WIRE_NOT_ON_CURVE


def _pt(pt):
    return None if pt == O else pt


def expect(cv, op, a, b, p, q):
    """((outx, outy), code) of one raw element: mul = b p, lincomb = a G + b p, add = p + q"""
    e = check(cv, p) or (check(cv, q) if op == "add" else WIRE_OK)
    if e:
        return O, e
    if op == "add":
        r = cv.add(_pt(p), _pt(q))
    else:
        r = cv.mul(b % cv.n, _pt(p)) if _pt(p) is not None else None
        if op == "lincomb":
            r = cv.add(cv.mul(a % cv.n, cv.g), r)
    return (O, WIRE_INFINITY) if r is None else (r, WIRE_OK)


def edge_scalars(cv):
    n = cv.n
    return [0, 1, 2, 3, n - 1, n, n + 1, (1 << 256) - 1, (n - 1) // 2, (n + 1) // 2, 1 << 127, (1 << 128) - 1, 1 << 128, (1 << 128) + 1]


@functools.lru_cache(maxsize=None)
def glv_scalars():
    """secp256k1 only: [(kind, k)] chosen by the decomposition k = s1 k1 + s2 k2 lambda"""
    n = R.N
    out = [("glv_lambda", LAMBDA), ("glv_lambda_plus", LAMBDA + 1), ("glv_lambda_minus", LAMBDA - 1), ("glv_minus_lambda", n - LAMBDA),
           ("glv_lambda_sq", LAMBDA * LAMBDA % n)]
    rng = R.SplitMix64(0x61F)
    want = {(0, 0), (0, 1), (1, 0), (1, 1)}
    while want:
        k = rng.below(n)
        k1, k2, n1, n2 = R.glv_decompose(k)
        if k1 and k2 and (n1, n2) in want:
            want.discard((n1, n2))
            out.append(("glv_signs_%d%d" % (n1, n2), k))
    for m in (1, 2, 3, 5, (1 << 100) + 1):
        out.append(("glv_k1_zero", m * LAMBDA % n))            # (k1, k2) = (0, m)
        out.append(("glv_k1_zero", (n - m) * LAMBDA % n))      # (0, -m)
        out.append(("glv_k1_eq_k2", m * (1 + LAMBDA) % n))     # (m, m)
        out.append(("glv_k1_eq_k2", (n - m) * (1 + LAMBDA) % n))
    for m in (5, 1 << 100, (1 << 126) + 12345):
        out.append(("glv_k2_zero", m))                         # (m, 0); 0 .. 3, 2^127 are among the edges
        out.append(("glv_k2_zero", n - m))
    found = 0
    while found < 3:                                           # the top digit (bits 126, 127) of both halves at once
        k = rng.below(n)
        k1, k2, _n1, _n2 = R.glv_decompose(k)
        if k1 >> 126 and k2 >> 126:
            found += 1
            out.append(("glv_top_digits", k))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def fixed_points(curve_id):
    """[(kind, affine point, its discrete logarithm)]: G, -G, 2 G, three fixed random points"""
    cv = CURVES[curve_id]
    rng = R.SplitMix64(0xA17 + curve_id)
    ts = [("G", 1), ("minus_G", cv.n - 1), ("two_G", 2)] + [("random", 1 + rng.below(cv.n - 1)) for _ in range(3)]
    return tuple((kind, cv.mul(t, cv.g), t) for kind, t in ts)


def invalid_points(curve_id):
    """[(kind, point)] with their expected codes decided by `check`"""
    cv = CURVES[curve_id]
    p = cv.p
    gx, gy = cv.g
    rhs = lambda x: (x * x * x + cv.a * x + cv.b) % p
    xs = next(x for x in range(1, 100) if pow(rhs(x), (p - 1) // 2, p) == 1)     # a small abscissa: xs + p < 2^256 on both curves
    ys = pow(rhs(xs), (p + 1) // 4, p)
    assert cv.on_curve((xs, ys)) and xs + p < 1 << 256 and not cv.on_curve(((p + 5) % p, gy))
    return [("x_eq_p", (p, gy)), ("y_eq_p", (gx, p)), ("x_ge_p_off_curve", (p + 5, gy)), ("x_ge_p_on_curve_mod_p", (xs + p, ys)),
            ("y_max", (gx, (1 << 256) - 1)), ("y_plus_one", (gx, gy + 1)), ("x_only", (gx, 0)), ("y_only", (0, gy))]


@functools.lru_cache(maxsize=None)
def set_x(curve_id, op):
    """the synthetic cases of one curve and call, computed once per session (a tuple of Case)"""
    cv = CURVES[curve_id]
    n = cv.n
    rng = R.SplitMix64(0xB0B + curve_id)
    out = []

    def case(kind, a=0, b=0, p=O, q=O):
        o, e = expect(cv, op, a, b, p, q)
        out.append(Case(op, kind, a, b, p, q, o, e))

    pts = fixed_points(curve_id)
    bad = invalid_points(curve_id)
    g = cv.g
    if op == "mul":
        scalars = [("edge", k) for k in edge_scalars(cv)] + (list(glv_scalars()) if curve_id == 0 else [])
        for j, (skind, k) in enumerate(scalars):                                 # every scalar on G and on a random point
            for pkind, pt, _t in (pts[0], pts[3 + j % 3]):
                case("%s/%s" % (skind, pkind), b=k, p=pt)
        for pkind, pt, _t in pts[1:3] + pts[4:]:                                 # every other point on a few edge scalars
            for k in edge_scalars(cv)[::3]:
                case("edge/%s" % pkind, b=k, p=pt)
        for skind, k in scalars[:14:3] + scalars[14:19]:
            case("%s/neutral" % skind, b=k, p=O)
        for pkind, pt in bad:
            for k in (0, 1 + rng.below(n - 1)):
                case("invalid/%s" % pkind, b=k, p=pt)
        for _ in range(16):
            case("random", b=rng.below(1 << 256), p=pts[3 + rng.next() % 3][1])
    elif op == "lincomb":
        for pkind, pt, t in pts:
            b = 1 + rng.below(n - 1)
            case("a_zero/" + pkind, a=0, b=b, p=pt)
            case("b_zero/" + pkind, a=1 + rng.below(n - 1), b=0, p=pt)
            case("both_zero/" + pkind, a=0, b=0, p=pt)
            case("both_n/" + pkind, a=n, b=n, p=pt)
            case("opposite/" + pkind, a=(n - b * t) % n, b=b, p=pt)              # a G = -b P
            case("doubling/" + pkind, a=b * t % n, b=b, p=pt)                    # a G = b P
            case("generic/" + pkind, a=rng.below(1 << 256), b=rng.below(1 << 256), p=pt)
        b = 1 + rng.below(n - 1)
        case("opposite_G", a=n - b, b=b, p=g)
        case("doubling_G", a=b, b=b, p=g)
        case("neutral_P", a=1 + rng.below(n - 1), b=1 + rng.below(n - 1), p=O)
        case("neutral_P_a_zero", a=0, b=1 + rng.below(n - 1), p=O)
        for k in edge_scalars(cv):
            case("edge_a", a=k, b=1 + rng.below(n - 1), p=pts[3][1])
            case("edge_b", a=1 + rng.below(n - 1), b=k, p=pts[4][1])
        if curve_id == 0:
            for skind, k in glv_scalars():
                case(skind, a=rng.below(n), b=k, p=pts[5][1])
        for pkind, pt in bad:
            case("invalid_b_zero/" + pkind, a=1 + rng.below(n - 1), b=0, p=pt)
            case("invalid/" + pkind, a=rng.below(n), b=1 + rng.below(n - 1), p=pt)
    else:
        for pkind, pt, _t in pts:
            case("P_plus_P/" + pkind, p=pt, q=pt)
            case("P_minus_P/" + pkind, p=pt, q=cv.neg(pt))
            case("P_plus_O/" + pkind, p=pt, q=O)
            case("O_plus_Q/" + pkind, p=O, q=pt)
        case("O_plus_O")
        for i in (0, 2, 3, 4):
            for j in (0, 2, 3, 4):
                if i != j:
                    case("generic", p=pts[i][1], q=pts[j][1])
        for (ka, pa), (kb, pb) in zip(bad, bad[1:] + bad[:1]):
            case("P_invalid/" + ka, p=pa, q=pts[3][1])
            case("Q_invalid/" + ka, p=pts[4][1], q=pa)
            case("Q_invalid_P_neutral/" + ka, p=O, q=pa)
            case("both_invalid/%s/%s" % (ka, kb), p=pa, q=pb)
    return tuple(out)


F_MAX = 4161


@functools.lru_cache(maxsize=None)
def _filler_scalars(curve_id):
    n = CURVES[curve_id].n
    rng = R.SplitMix64(0xF111 + curve_id)
    t = [1 + rng.below(n - 1) for _ in range(F_MAX + 1)]
    return t, [rng.below(1 << 256) for _ in range(F_MAX)], [rng.below(1 << 256) for _ in range(F_MAX)]


def set_f(curve_id, op, count):
    """`count` filler cases of one call (see the module docstring); the first `count` of one fixed sequence per curve"""
    cv = CURVES[curve_id]
    n = cv.n
    assert count <= F_MAX
    t, a, b = _filler_scalars(curve_id)
    if op == "mul":
        res = [b[i] % n * t[i] % n for i in range(count)]
    elif op == "lincomb":
        res = [(a[i] % n + b[i] % n * t[i]) % n for i in range(count)]
    else:
        res = [(t[i] + t[i + 1]) % n for i in range(count)]
    pts = S.base_points(curve_id, t[:count + 1] + res)
    out = []
    for i in range(count):
        r = pts[res[i]]
        o, e = (O, WIRE_INFINITY) if r is None else (r, WIRE_OK)
        out.append(Case(op, "F", a[i] if op == "lincomb" else 0, 0 if op == "add" else b[i], pts[t[i]], pts[t[i + 1]] if op == "add" else O, o, e))
    return out


def batch(curve_id, op, total):
    """X + F + X of one call: `total` cases"""
    x = list(set_x(curve_id, op))
    assert total >= 2 * len(x)
    return x + set_f(curve_id, op, total - 2 * len(x)) + x


def arrays(cases):
    """list of Case -> dict of (n, 32) uint8 arrays a, b, px, py, qx, qy, outx, outy and err (n,)"""
    pk = S.pack
    return dict(a=pk([c.a for c in cases]), b=pk([c.b for c in cases]), px=pk([c.p[0] for c in cases]), py=pk([c.p[1] for c in cases]),
                qx=pk([c.q[0] for c in cases]), qy=pk([c.q[1] for c in cases]), outx=pk([c.out[0] for c in cases]),
                outy=pk([c.out[1] for c in cases]), err=np.array([c.err for c in cases], np.uint8))


def selftest_vectors():
    """the text of tests/emu_point/point_vectors.inc: three cases of every kind of set X, both curves and the three calls, as
    macro calls (all of X runs through the same bodies in test_point_arith_cpu.py; the sanitizer program needs every path,
    not every value).
    P(curve, x, y): a distinct operand; V(curve, op, a, b, p, q, outx, outy_odd, err): one case, p and q indices into the P
    lines (in order, from 0), the expected point as its x and the parity of its y (which pin it: it is on the curve)"""
    cases, seen = [], {}
    for curve_id in (0, 1):
        for o, op in enumerate(("mul", "lincomb", "add")):
            for c in set_x(curve_id, op):      # the first three cases of every kind (the part before '/'; edge scalars: per point)
                key = (curve_id, op, c.kind if c.kind.startswith("edge/") else c.kind.split("/")[0])
                seen[key] = seen.get(key, 0) + 1
                if seen[key] <= 3:
                    cases.append((curve_id, o, c))
    index = {}
    for curve_id, _o, c in cases:
        for pt in (c.p, c.q):
            index.setdefault((curve_id, pt), len(index))
    lines = ["// generated by tests/point_arith_inputs.py selftest_vectors() from set X, three cases of every kind (test_point_arith_cpu.py keeps it current)",
             "// P(curve, x, y); V(curve, op (0 mul, 1 lincomb, 2 add), a, b, p, q, outx, outy & 1, err): values as big-endian hex"]
    lines += ['P(%d, "%x", "%x")' % (curve_id, pt[0], pt[1]) for (curve_id, pt) in index]
    lines += ['V(%d, %d, "%x", "%x", %d, %d, "%x", %d, %d)' % (curve_id, o, c.a, c.b, index[curve_id, c.p], index[curve_id, c.q], c.out[0],
                                                             c.out[1] & 1, c.err) for curve_id, o, c in cases]
    return "\n".join(lines) + "\n"
