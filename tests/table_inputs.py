"""Inputs and independent expectations of the point-table tests (test_point_table_cpu.py, test_gpu_point_table.py):
include/p2e.h p2e_point_table_create, p2e_point_table_read_window, p2e_point_table_mul_batch (out = k T[idx]),
p2e_point_table_lincomb_batch (out = a G + b T[idx]) and p2e_ecdsa_verify_table_batch.

Nothing here uses the code under test.

The table points of a curve are ONE fixed sequence t_j G with known t_j: G, -G, 2 G, then random keys; a table of m points
holds the first m of them.
Set X (synthetic, per curve, table size and call): the expectation is `expect` / `verdict` below, the definitions of
    include/p2e.h written with Python integers on oracle/p2e_ref.py's Curve.  Scalars 0, 1, n - 1, n, n + 1, 2^256 - 1; for
    every window w < 64 the scalars 1 * 16^w and 15 * 16^w, so that every table row is hit alone (their products are entries
    of `window_rows`, the table itself in Python integers); all nibbles 15 and alternating zero nibbles; for a G + b P the
    cases a G = b P, a G = -b P, a = 0, b = 0; idx values 0, m - 1, m and 0xFFFFFFFF; for the verifier signatures made here
    from (msg, t_j, nonce), untouched and with msg, r or s altered within range, and r, s at and beyond the range's ends.
Set F (filler): random scalars on random indices; the expectations (k t_j) G and (a + b t_j) G come from the C oracle's
    fixed-base walk (sign_inputs.base_points), and the filler signatures are valid by construction."""
import functools

import numpy as np

import p2e_ref as R
import point_arith_inputs as PI
import sign_inputs as S

CURVES = S.CURVES
WIRE_OK, WIRE_COORD_RANGE, WIRE_NOT_ON_CURVE, WIRE_INFINITY, WIRE_SCALAR_RANGE, WIRE_BAD_INDEX = 0, 3, 4, 5, 8, 10
FB_WINDOWS = 66                      # rows of one point's table (64 nibbles of a scalar and two spare rows)
IDX_MAX = 0xFFFFFFFF
POINT_BYTES = FB_WINDOWS * 16 * 64     # include/p2e.h P2E_POINT_TABLE_BYTES_PER_POINT
M_MAX = 65
O = PI.O
OPS = ("mul", "lincomb", "verify")
CODES = {"mul": {WIRE_OK, WIRE_INFINITY, WIRE_BAD_INDEX}, "lincomb": {WIRE_OK, WIRE_INFINITY, WIRE_BAD_INDEX},
         "verify": {WIRE_OK, WIRE_SCALAR_RANGE, WIRE_BAD_INDEX}}     # every code a call can emit


class Case:
    """mul: b = k.  lincomb: a, b.  verify: a = msg, b = r, s; out = (0, 0), valid = the verdict."""
    __slots__ = ("op", "kind", "idx", "a", "b", "s", "out", "err", "valid")

    def __init__(self, op, kind, idx, a, b, s, out, err, valid):
        self.op, self.kind, self.idx, self.a, self.b, self.s, self.out, self.err, self.valid = op, kind, idx, a, b, s, out, err, valid


@functools.lru_cache(maxsize=None)
def table_logs(curve_id):
    """t_j, j < M_MAX: 1, n - 1, 2, then random"""
    n = CURVES[curve_id].n
    rng = R.SplitMix64(0x7AB1E + curve_id)
    return (1, n - 1, 2) + tuple(1 + rng.below(n - 1) for _ in range(M_MAX - 3))


@functools.lru_cache(maxsize=None)
def table_points(curve_id, m=M_MAX):
    """the first m table points (affine, Python integers)"""
    cv = CURVES[curve_id]
    return tuple(cv.mul(t, cv.g) for t in table_logs(curve_id)[:m])


@functools.lru_cache(maxsize=None)
def window_rows(curve_id, pt):
    """rows[w][d] = d 16^w pt for w < 66, d = 0 .. 15 with slot 0 a copy of slot 1: the table of `pt` as the header defines it"""
    cv = CURVES[curve_id]
    rows, base = [], pt
    for _w in range(FB_WINDOWS):
        row = cv.fixed_base_window(base)
        rows.append((row[0],) + tuple(row))
        for _ in range(4):
            base = cv.double(base)
    return tuple(rows)


@functools.lru_cache(maxsize=None)
def _mul(curve_id, k, pt):
    cv = CURVES[curve_id]
    if k == 0:
        return None
    w = ((k & -k).bit_length() - 1) // 4
    if k >> (4 * w) < 16:                               # d 16^w: an entry of the table in integers
        return window_rows(curve_id, pt)[w][k >> (4 * w)]
    return cv.mul(k, pt)


def expect(curve_id, m, op, idx, a, b):
    """((outx, outy), code) of one raw element of mul (b T[idx]) or lincomb (a G + b T[idx])"""
    cv = CURVES[curve_id]
    if idx >= m:
        return O, WIRE_BAD_INDEX
    r = _mul(curve_id, b % cv.n, table_points(curve_id, m)[idx])
    if op == "lincomb":
        r = cv.add(_mul(curve_id, a % cv.n, cv.g), r)
    return (O, WIRE_INFINITY) if r is None else (r, WIRE_OK)


def verdict(curve_id, m, idx, msg, r, s):
    """(code, valid) of one raw signature: curve/ecdsa.rs:42-62 with the range checks of the header in front"""
    cv = CURVES[curve_id]
    n = cv.n
    if idx >= m:
        return WIRE_BAD_INDEX, 0
    if not (0 < r < n and 0 < s < n):
        return WIRE_SCALAR_RANGE, 0
    c = pow(s, -1, n)
    x = cv.add(cv.mul(msg % n * c % n, cv.g), cv.mul(r * c % n, table_points(curve_id, m)[idx]))
    return WIRE_OK, int(x is not None and x[0] % n == r)


def scalars(cv):
    """[(kind, k)]: the edges, every window alone with digit 1 and digit 15, the two nibble patterns"""
    n = cv.n
    out = [("edge", k) for k in (0, 1, n - 1, n, n + 1, (1 << 256) - 1)]
    for w in range(64):
        out += [("window_1", 1 << (4 * w)), ("window_15", 15 << (4 * w))]
    out.append(("all_15", int("f" * 63, 16)))                        # 63 nibbles: 2^252 - 1 < n is taken as it is
    out.append(("alternating", int("f0" * 32, 16) % n))              # zero nibbles between non-zero ones
    out.append(("alternating", int("0f" * 32, 16)))
    return out


def sign(curve_id, idx, msg, k):
    """(r, s) of sign_message under key t_idx with nonce k, Python integers"""
    cv = CURVES[curve_id]
    n = cv.n
    r = cv.mul(k, cv.g)[0] % n
    return r, pow(k, -1, n) * (msg % n + r * table_logs(curve_id)[idx]) % n


@functools.lru_cache(maxsize=None)
def set_x(curve_id, m, op):
    """the synthetic cases of one curve, table size and call (a tuple of Case)"""
    cv = CURVES[curve_id]
    n = cv.n
    logs = table_logs(curve_id)
    rng = R.SplitMix64(0x7AB + 16 * curve_id + m)
    out = []
    bad_idx = (m, m + 1, 1 << 31, IDX_MAX)
    some = sorted({0, m - 1, min(2, m - 1), min(3, m - 1)})          # G, -G, 2 G and the first random key where the table has them

    def case(kind, idx, a=0, b=0):
        o, e = expect(curve_id, m, op, idx, a, b)
        out.append(Case(op, kind, idx, a, b, 0, o, e, 0))

    def vcase(kind, idx, msg, r, s):
        e, v = verdict(curve_id, m, idx, msg, r, s)
        out.append(Case(op, kind, idx, msg, r, s, O, e, v))

    if op == "mul":
        for kind, k in scalars(cv):
            case("%s/last" % kind, m - 1, b=k)
            if kind == "edge":
                for j in some:
                    case("edge/%d" % j, j, b=k)
        for j in some:
            case("random/%d" % j, j, b=rng.below(1 << 256))
        for j in bad_idx:
            case("bad_index", j, b=1 + rng.below(n - 1))
            case("bad_index_zero_k", j, b=0)
    elif op == "lincomb":
        for j in some:
            t, b = logs[j], 1 + rng.below(n - 1)
            case("a_zero/%d" % j, j, a=0, b=b)
            case("b_zero/%d" % j, j, a=1 + rng.below(n - 1), b=0)
            case("both_zero/%d" % j, j, a=0, b=0)
            case("both_n/%d" % j, j, a=n, b=n)
            case("opposite/%d" % j, j, a=(n - b * t) % n, b=b)       # a G = -b P
            case("doubling/%d" % j, j, a=b * t % n, b=b)             # a G = b P
            case("generic/%d" % j, j, a=rng.below(1 << 256), b=rng.below(1 << 256))
        for kind, k in scalars(cv):
            if kind.startswith("window"):
                case("%s_b" % kind, m - 1, a=0, b=k)                 # one row of the point's table, nothing else
                case("%s_a" % kind, m - 1, a=k, b=0)                 # one row of the generator's
            else:
                case("%s_b" % kind, m - 1, a=1 + rng.below(n - 1), b=k)
                case("%s_a" % kind, 0, a=k, b=1 + rng.below(n - 1))
        for j in bad_idx:
            case("bad_index", j, a=rng.below(n), b=1 + rng.below(n - 1))
    else:
        for j in some:
            msg, k = rng.below(1 << 256), 1 + rng.below(n - 1)
            r, s = sign(curve_id, j, msg, k)
            vcase("valid/%d" % j, j, msg, r, s)
            vcase("valid_minus_s/%d" % j, j, msg, r, n - s)          # (r, -s) verifies too: -R has R's abscissa
            vcase("msg_plus_n/%d" % j, j, msg % n + n if msg % n + n < 1 << 256 else msg % n, r, s)   # msg is reduced
            vcase("msg_altered/%d" % j, j, (msg + 1) % (1 << 256), r, s)
            vcase("r_altered/%d" % j, j, msg, r % (n - 1) + 1, s)    # r + 1, or 1 for r = n - 1: in range
            vcase("s_altered/%d" % j, j, msg, r, s % (n - 1) + 1)
            vcase("wrong_key/%d" % j, (j + 1) % m, msg, r, s)        # (m = 1: the same key, valid)
            for kind, rr, ss in (("r_zero", 0, s), ("r_eq_n", n, s), ("r_above_n", n + 1, s), ("r_max", (1 << 256) - 1, s),
                                 ("s_zero", r, 0), ("s_eq_n", r, n), ("s_above_n", r, n + 1), ("s_max", r, (1 << 256) - 1),
                                 ("r_plus_n", r + n if r + n < 1 << 256 else n, s), ("both_zero", 0, 0)):
                vcase("%s/%d" % (kind, j), j, msg, rr, ss)
        msg, k = rng.below(n), 1 + rng.below(n - 1)
        r, s = sign(curve_id, 0, msg, k)
        vcase("msg_zero", 0, 0, *sign(curve_id, 0, 0, k))
        for j in bad_idx:
            vcase("bad_index", j, msg, r, s)
            vcase("bad_index_and_range", j, msg, 0, 0)               # the index is tested first
    assert {c.err for c in out} == CODES[op], "every code the call can emit occurs in set X"
    return tuple(out)


F_MAX = 4161


@functools.lru_cache(maxsize=None)
def _filler(curve_id):
    n = CURVES[curve_id].n
    rng = R.SplitMix64(0xF177 + curve_id)
    return ([rng.next() for _ in range(F_MAX)], [rng.below(1 << 256) for _ in range(F_MAX)], [rng.below(1 << 256) for _ in range(F_MAX)],
            [1 + rng.below(n - 1) for _ in range(F_MAX)])


def set_f(curve_id, m, op, count):
    """`count` filler cases (see the module docstring): the first `count` of one fixed sequence per curve, indices mod m"""
    cv = CURVES[curve_id]
    n = cv.n
    assert count <= F_MAX
    logs = table_logs(curve_id)
    j, a, b, k = _filler(curve_id)
    out = []
    if op == "verify":
        pts = S.base_points(curve_id, k[:count])
        for i in range(count):
            r = pts[k[i]][0] % n
            s = pow(k[i], -1, n) * (a[i] % n + r * logs[j[i] % m]) % n
            assert r and s
            out.append(Case(op, "F", j[i] % m, a[i], r, s, O, WIRE_OK, 1))
        return out
    if op == "mul":
        res = [b[i] % n * logs[j[i] % m] % n for i in range(count)]
    else:
        res = [(a[i] % n + b[i] % n * logs[j[i] % m]) % n for i in range(count)]
    pts = S.base_points(curve_id, res)
    for i in range(count):
        r = pts[res[i]]
        o, e = (O, WIRE_INFINITY) if r is None else (r, WIRE_OK)
        out.append(Case(op, "F", j[i] % m, a[i] if op == "lincomb" else 0, b[i], 0, o, e, 0))
    return out


def batch(curve_id, m, op, total):
    """the main batch of one call: set X, then filler up to `total` cases (at least all of X)"""
    x = list(set_x(curve_id, m, op))
    return x + set_f(curve_id, m, op, max(total - len(x), 0))


def arrays(cases):
    """list of Case -> dict: idx (n,) uint32; a, b, s, outx, outy (n, 32) uint8; err, valid (n,) uint8"""
    pk = S.pack
    return dict(idx=np.array([c.idx for c in cases], np.uint32), a=pk([c.a for c in cases]), b=pk([c.b for c in cases]),
                s=pk([c.s for c in cases]), outx=pk([c.out[0] for c in cases]), outy=pk([c.out[1] for c in cases]),
                err=np.array([c.err for c in cases], np.uint8), valid=np.array([c.valid for c in cases], np.uint8))


def point_arrays(curve_id, m):
    pts = table_points(curve_id, m)
    return S.pack([p[0] for p in pts]), S.pack([p[1] for p in pts])


def window_bytes(curve_id, pt, w):
    """what p2e_point_table_read_window writes for window w of `pt`: (16, 2, 32) uint8"""
    row = window_rows(curve_id, pt)[w]
    return np.stack([S.pack([e[0] for e in row]), S.pack([e[1] for e in row])], axis=1)


SELFTEST_M = 4


def selftest_vectors():
    """the text of tests/emu_table/table_vectors.inc: the table points of SELFTEST_M keys per curve and, per call, the first
    three cases of every kind of set X (the part before '/'), out-of-range indices among them, as macro calls.
    T(curve, x, y): table point, in order; V(curve, op, idx, a, b, s, outx, outy & 1, err, valid): one case"""
    lines = ["// generated by tests/table_inputs.py selftest_vectors() from set X at m = %d (test_point_table_cpu.py keeps it current)" % SELFTEST_M,
             "// T(curve, x, y); V(curve, op (0 mul, 1 lincomb, 2 verify), idx, a, b, s, outx, outy & 1, err, valid): values as big-endian hex"]
    for curve_id in (0, 1):
        lines += ['T(%d, "%x", "%x")' % (curve_id, p[0], p[1]) for p in table_points(curve_id, SELFTEST_M)]
    for curve_id in (0, 1):
        for o, op in enumerate(OPS):
            seen = {}
            for c in set_x(curve_id, SELFTEST_M, op):
                key = c.kind.split("/")[0]
                seen[key] = seen.get(key, 0) + 1
                if seen[key] <= 3:
                    lines.append('V(%d, %d, 0x%xu, "%x", "%x", "%x", "%x", %d, %d, %d)' % (curve_id, o, c.idx, c.a, c.b, c.s, c.out[0], c.out[1] & 1,
                                                                                    c.err, c.valid))
    return "\n".join(lines) + "\n"
