"""Vectors and big-integer expectations for the point-layer probe (tests/probe_point/p2e_probe_point.hip): csrc/sign.hpp,
recover.hpp, pmsm.hpp and the GLV rounding of wit.hpp, function by function.

Nothing here comes from the code under test.  Points with a known logarithm d G are sign_inputs.base_points (the C oracle's
fixed-base walk), so u (d G) = (u d mod n) G is one more lookup; points without one are lifted abscissas
(msm_native_inputs.lift) and are added and multiplied on Python integers (oracle/p2e_ref.py Curve.add / Curve.mul).  The point
ops return Jacobian triples: the POINT is compared (x = X / Z^2, y = Y / Z^3, Z != 0 mod p whenever `have`), and `have`, err
and flag words exactly.  Values (square roots, digits, quotients, affine coordinates) are compared word for word.

`case(name, field)` -> probe_inputs.Case with `counts`: how many elements of every required class the batch holds, counted
from the inputs alone; `required_counts` says how many there must be.  Every batch has n = 1 mod 64."""
import functools
import os

import numpy as np

import msm_native_inputs as MN
import p2e_ref as R
import probe_inputs as PI
import recover_inputs as RI
import sign_inputs as S
from probe_inputs import Case, cat, pack, unpack

PROBE_DIR = os.path.join(PI.HERE, "probe_point")
CURVE_FIELDS = (0, 2)            # field id of the probe's table -> curve id = field // 2
FIELD_NAMES = ("k1", "k1n", "p256")
N_VALUE, N_MUL = 1025, 129       # batch sizes: value ops; ops that multiply a point or reduce a chunk
LEAST = 20                       # elements of every operand class
FB_ROWS = 66
TABLE_OPS = ("sign_window_sum8", "sign_window_sum2", "body_base_mul_quad")
CHUNK_WIDTHS = (4, 7, 11, 12)
CHUNK_STRIDE = 7                 # the probe's lane of element k of a round: 7 k mod (windows chunks)
GLV_CONSTS = {"b2": R.GLV_B2, "mb1": R.GLV_MINUS_B1}


def curve(field):
    return S.CURVES[field // 2]


class PointProbe(PI.Probe):
    """the point probe's library; the fixed-base table of a curve is handed over before the first op that reads it"""

    def __init__(self, device):
        super().__init__(device, PROBE_DIR, "p2e_probe_point")
        self.L.probe_aux.restype = PI.C.c_long
        self.L.probe_aux.argtypes = [PI.C.c_int, PI.C.c_void_p, PI.C.c_size_t]
        self._tables = set()

    def run(self, name, field, inp):
        if name in TABLE_OPS and field not in self._tables:
            assert self.failed is None
            t = fb_table(field)
            rc = self.L.probe_aux(field, t.ctypes.data, t.nbytes)
            if rc != 0:
                self.failed = (f"probe_aux/{field}", rc)
            assert rc == 0, rc
            self._tables.add(field)
        return super().run(name, field, inp)


# ---- points ------------------------------------------------------------------------------------------------------------
def kG(field, scalars):
    """{k: k G or None}: the C oracle's fixed-base walk (sign_inputs.base_points)"""
    cv = curve(field)
    red = [k % cv.n for k in scalars]
    pts = S.base_points(field // 2, [k for k in red if k])
    return {k: (pts[k] if k else None) for k in red}


@functools.lru_cache(maxsize=None)
def fb_table(field):
    """T[w][d] = d 16^w G, d = 1 .. 15, slot 0 a copy of slot 1; 66 rows (sign.hpp), (66 * 16, 16) uint32"""
    cv = curve(field)
    ks = [[(max(d, 1) << (4 * w)) % cv.n for d in range(16)] for w in range(FB_ROWS)]
    pts = kG(field, [k for row in ks for k in row])
    flat = [pts[k] for row in ks for k in row]
    return np.ascontiguousarray(cat(pack([p[0] for p in flat], 8), pack([p[1] for p in flat], 8)))


@functools.lru_cache(maxsize=None)
def known_points(field):
    """[(d, d G)]: the MSM pool's first 256 points"""
    return tuple(MN.pool(field // 2)[:256])


@functools.lru_cache(maxsize=None)
def lifted_points(field, count=40):
    cv = curve(field)
    rng = R.SplitMix64(0x11F7 + field)
    return tuple(MN.lift(cv, rng.below(cv.p)) for _ in range(count))


def all_points(field):
    return [pt for _d, pt in known_points(field)] + list(lifted_points(field))


def to_affine(cv, X, Y, Z):
    zi = pow(Z, -1, cv.p)
    return X * zi * zi % cv.p, Y * zi * zi * zi % cv.p


# ---- encodings ---------------------------------------------------------------------------------------------------------
def tight_of(v, sel):
    """a tight limb form (every limb <= F29_T) of v mod p that is not the canonical split: v + p or v + 2 p, and 2^29 borrowed
    into the limbs that have room"""
    l = PI.limbs_std(v + PI.P * (1 + sel % 2))
    if sel % 3:
        for k in range(8):
            if l[k + 1] and l[k] <= 1 << 20:
                l[k] += 1 << 29
                l[k + 1] -= 1
    assert PI.limb_value(l) % PI.P == v % PI.P and all(0 <= x <= PI.F29_T for x in l)
    return l


@functools.lru_cache(maxsize=None)
def tight_z_forms():
    """probe_inputs.tight_forms() that stand for a non-zero value: the Z of the tight operands"""
    return tuple(f for f in PI.tight_forms() if PI.limb_value(f) % PI.P)


def slot(v):
    return [(v >> (32 * i)) & PI.U32 for i in range(8)] + [0]


class Pt:
    """an operand: the point (affine, or None), its Jacobian coordinates as values, `have`, and the words that carry it"""

    def __init__(self, point, X, Y, Z, have, words):
        self.point, self.X, self.Y, self.Z, self.have, self.words = point, X, Y, Z, have, words


def jac_operand(field, point, z, have=True, tight=False, sel=0):
    """`point` under Z = z (a value, or with tight=True a limb form from tight_z_forms())"""
    cv = curve(field)
    zv = PI.limb_value(z) % cv.p if tight else z
    X, Y = point[0] * zv * zv % cv.p, point[1] * pow(zv, 3, cv.p) % cv.p
    if tight:
        words = tight_of(X, sel) + tight_of(Y, sel + 1) + list(z) + [int(have) | 2]
    else:
        words = slot(X) + slot(Y) + slot(zv) + [int(have)]
    return Pt(point if have else None, X, Y, zv, have, words)


def garbage_operand(field, rng, tight=False):
    """an empty operand (`have` = 0) whose coordinates hold a non-zero pattern inside the field's contract"""
    cv = curve(field)
    pats = [cv.p - 1, 0x5555555555555555555555555555555555555555555555555555555555555555 % cv.p, 1, rng.below(cv.p) | 1]
    X, Y, Z = (pats[rng.next() % 4] for _ in range(3))
    if tight:
        forms = tight_z_forms()
        words = list(forms[rng.next() % len(forms)]) + tight_of(Y, 1) + list(forms[rng.next() % len(forms)]) + [2]
    else:
        words = slot(X) + slot(Y) + slot(Z) + [0]
    assert any(words[:27])
    return Pt(None, X, Y, Z, False, words)


def decode_points(cv, out):
    """(n, 25) words X, Y, Z, have -> [(have, Z mod p, affine point or None)]"""
    X, Y, Z = unpack(out[:, 0:8]), unpack(out[:, 8:16]), unpack(out[:, 16:24])
    res = []
    for i in range(out.shape[0]):
        z = Z[i] % cv.p
        res.append((int(out[i, 24]), z, to_affine(cv, X[i], Y[i], Z[i]) if z else None))
    return res


def point_check(field, inp, want, kinds, lanes=1, offset=0, lanes_equal=False):
    """want[i] (or want[i][lane]) = ("point", P): have = 1, Z != 0, the point P;  ("empty",): have = 0;  ("zero_z",): have = 1
    and Z = 0 mod p (an incomplete formula's defensive zero);  ("any",): not compared"""
    cv = curve(field)

    def check(out):
        assert out.shape[0] == len(want) and out.shape[1] == lanes, out.shape
        if lanes_equal:
            for lane in range(1, lanes):
                b = PI.first_bad(out[:, lane, :], out[:, 0, :])
                assert b is None, (f"lane {lane} differs from lane 0 at element {b[0]} word {b[1]}", kinds[b[0]])
        for lane in range(lanes):
            got = decode_points(cv, out[:, lane, offset:offset + 25])
            for i, (have, z, pt) in enumerate(got):
                w = want[i][lane] if lanes > 1 and not lanes_equal else want[i]
                ctx = (kinds[i], i, lane, [hex(int(x)) for x in inp[i]], [hex(int(x)) for x in out[i, lane]])
                if w[0] == "any":
                    continue
                if w[0] == "empty":
                    assert have == 0, ("have", ctx)
                elif w[0] == "zero_z":
                    assert have == 1 and z == 0, ("zero Z", ctx)
                else:
                    assert have == 1 and z != 0 and pt == w[1], ("point", w[1], pt, ctx)
    return check


def _count(kinds):
    c = {}
    for k in kinds:
        c[k] = c.get(k, 0) + 1
    return c


def _rand(rng, m):
    """uniform below m (SplitMix64.below draws 256-bit values until one is below m: only for m near 2^256)"""
    return ((rng.below(1 << 256) << 256) | rng.below(1 << 256)) % m


def _pad(n, least):
    return PI.size_for(n, least)


# ---- two-operand additions ------------------------------------------------------------------------------------------------
def operand_pairs(field, mixed=False, b_never_empty=False):
    """[(kind, a, b)]: the classes of the issue, each in canonical and (secp256k1) tight-limb form, LEAST of each, then
    unrelated filler"""
    cv = curve(field)
    pts = all_points(field)
    rng = R.SplitMix64(0xADD0 + field + (8 if mixed else 0) + (16 if b_never_empty else 0))
    tz = tight_z_forms()
    rows = []

    def z_for(tight, one=False):
        if one:
            return 1
        return tz[rng.next() % len(tz)] if tight else 2 + rng.below(cv.p - 2)

    def operand(pt, z, tight):
        if tight and z == 1:
            z = tuple(PI.limbs_std(1))
        return jac_operand(field, pt, z, True, tight, rng.next() % 6)

    forms = (False, True) if field == 0 else (False,)
    for tight in forms:
        tag = "_tight" if tight else ""
        for j in range(LEAST):
            p, q = pts[rng.next() % len(pts)], pts[rng.next() % len(pts)]
            if p[0] == q[0]:
                continue
            rows.append(("unrelated" + tag, operand(p, z_for(tight), tight), operand(q, z_for(tight, mixed), tight)))
        for j in range(LEAST + 2):
            p = pts[(7 * j + 3) % len(pts)]
            if not mixed:
                z1, z2 = z_for(tight), z_for(tight)
                if (PI.limb_value(z1) - PI.limb_value(z2)) % cv.p if tight else z1 != z2:
                    rows.append(("same_two_z" + tag, operand(p, z1, tight), operand(p, z2, tight)))
                rows.append(("same_equal_z" + tag, operand(p, z1, tight), operand(p, z1, tight)))
                rows.append(("opposite_two_z" + tag, operand(p, z1, tight), operand(cv.neg(p), z2, tight)))
            else:                                                     # b is affine: a under some Z, and a under Z = 1
                rows.append(("same_two_z" + tag, operand(p, z_for(tight), tight), operand(p, 1, tight)))
                rows.append(("same_equal_z" + tag, operand(p, 1, tight), operand(p, 1, tight)))
                rows.append(("opposite_two_z" + tag, operand(p, z_for(tight), tight), operand(cv.neg(p), 1, tight)))
        for j in range(LEAST):
            p = pts[(11 * j + 5) % len(pts)]
            rows.append(("a_empty" + tag, garbage_operand(field, rng, tight), operand(p, z_for(tight, mixed), tight)))
            if not b_never_empty:
                rows.append(("b_empty" + tag, operand(p, z_for(tight), tight), garbage_operand(field, rng, tight)))
                rows.append(("both_empty" + tag, garbage_operand(field, rng, tight), garbage_operand(field, rng, tight)))
    n = _pad(len(rows), N_VALUE)
    while len(rows) < n:
        p, q = pts[rng.next() % len(pts)], pts[rng.next() % len(pts)]
        if p[0] != q[0]:
            rows.append(("unrelated", operand(p, z_for(False), False), operand(q, z_for(False, mixed), False)))
    return rows


def add_classes(field, b_never_empty=False):
    base = ["unrelated", "same_two_z", "same_equal_z", "opposite_two_z", "a_empty"] + ([] if b_never_empty else ["b_empty", "both_empty"])
    return base + ([k + "_tight" for k in base] if field == 0 else [])


def _pairs_inp(rows):
    return np.array([a.words + b.words for _k, a, b in rows], np.uint32)


def case_msm_add(mixed):
    def build(field):
        cv = curve(field)
        rows = operand_pairs(field, mixed)
        kinds = [k for k, _a, _b in rows]
        want = []
        for _k, a, b in rows:
            s = cv.add(a.point, b.point)
            want.append(("point", s) if s else ("empty",))
        inp = _pairs_inp(rows)
        return Case(inp, point_check(field, inp, want, kinds), _count(kinds), kinds)
    return build


def case_sign_sum_add(field):
    """the incomplete addition under the `have` flags: equal or opposite operands are outside the signer's argument, and the
    header's defensive statement is what is checked there: Z3 = Z1 Z2 h = 0 under have = 1"""
    cv = curve(field)
    rows = operand_pairs(field)
    kinds = [k for k, _a, _b in rows]
    want = []
    for k, a, b in rows:
        if a.have and b.have:
            want.append(("point", cv.add(a.point, b.point)) if k.startswith("unrelated") else ("zero_z",))
        elif a.have or b.have:
            want.append(("point", a.point if a.have else b.point))
        else:
            want.append(("empty",))
    inp = _pairs_inp(rows)
    return Case(inp, point_check(field, inp, want, kinds), _count(kinds), kinds)


def case_recover_final_add(field):
    cv = curve(field)
    rows = operand_pairs(field, b_never_empty=True)
    kinds = [k for k, _a, _b in rows]
    want, err = [], []
    for k, a, b in rows:
        s = cv.add(a.point, b.point)
        err.append(S.ERR_POINT_AT_INFINITY if s is None else 0)
        want.append(("point", s) if s else ("any",))
    inp = _pairs_inp(rows)
    pts = point_check(field, inp, want, kinds, offset=1)

    def check(out):
        b = PI.first_bad(out[:, 0, 0], np.array(err, np.uint32))
        assert b is None, ("err", kinds[b[0]], b[0], int(out[b[0], 0, 0]), err[b[0]])
        pts(out)
    return Case(inp, check, _count(kinds), kinds)


# ---- one-operand point ops ------------------------------------------------------------------------------------------------
def single_operands(field, seed, zero_z=False, empties=True):
    cv = curve(field)
    pts = all_points(field)
    rng = R.SplitMix64(seed + field)
    tz = tight_z_forms()
    rows = []
    for tight in ((False, True) if field == 0 else (False,)):
        tag = "_tight" if tight else ""
        for j in range(2 * LEAST):
            p = pts[(5 * j + 1) % len(pts)]
            z = tz[rng.next() % len(tz)] if tight else (1 if j % 4 == 0 else 2 + rng.below(cv.p - 2))
            if tight and j % 4 == 0:
                z = tuple(PI.limbs_std(1))
            rows.append(("point" + tag, jac_operand(field, p, z, True, tight, j)))
        if empties:
            for j in range(LEAST):
                rows.append(("empty" + tag, garbage_operand(field, rng, tight)))
        if zero_z:
            for j in range(LEAST):
                X, Y = 1 + rng.below(cv.p - 1), 1 + rng.below(cv.p - 1)
                if tight:                                             # 0 as p or 2 p in limbs, plain and borrowed
                    words = tight_of(X, j) + tight_of(Y, j + 1) + tight_of(0, j) + [3]
                else:
                    words = slot(X) + slot(Y) + slot(0) + [1]
                rows.append(("zero_z" + tag, Pt(None, X, Y, 0, True, words)))
    n = _pad(len(rows), N_VALUE)
    while len(rows) < n:
        rows.append(("point", jac_operand(field, pts[rng.next() % len(pts)], 2 + rng.below(cv.p - 2))))
    return rows


def case_msm_dbl(field):
    cv = curve(field)
    rows = single_operands(field, 0xDB10)
    kinds = [k for k, _a in rows]
    want = [("point", cv.double(a.point)) if a.have else ("empty",) for _k, a in rows]
    inp = np.array([a.words for _k, a in rows], np.uint32)
    return Case(inp, point_check(field, inp, want, kinds), _count(kinds), kinds)


def case_sign_to_affine(want_y):
    def build(field):
        cv = curve(field)
        rows = single_operands(field, 0xAFF0, zero_z=True, empties=False)
        kinds = [k for k, _a in rows]
        want = []
        for k, a in rows:
            if a.Z % cv.p == 0:
                want.append([0] + [0] * 16)
            else:
                x, y = a.point
                want.append([1] + slot(x)[:8] + (slot(y)[:8] if want_y else [0] * 8))
        inp = np.array([a.words for _k, a in rows], np.uint32)
        return PI.exact_case(inp, np.array(want, np.uint32), _count(kinds), kinds)
    return build


# ---- the fixed-base sums ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def group_pattern_scalars(curve_id):
    """[(mask, k)]: for each of the 16 empty / non-empty patterns of the four 64-bit groups (bit j of mask: group j is not
    empty), two scalars below 2^254 < n"""
    rng = R.SplitMix64(0x6707 + curve_id)
    out = []
    for mask in range(16):
        for _ in range(2):
            g = [(rng.next() | 1) if (mask >> j) & 1 else 0 for j in range(4)]
            g[3] >>= 2
            if (mask >> 3) & 1:
                g[3] |= 1
            out.append((mask, sum(v << (64 * j) for j, v in enumerate(g))))
    return tuple(out)


def group_mask(k):
    return sum(1 << j for j in range(4) if (k >> (64 * j)) & (2**64 - 1))


@functools.lru_cache(maxsize=None)
def base_mul_scalars(field):
    """canonical scalars (< n): the 16 group patterns, every table entry once, k = 0, the edges, uniform filler"""
    cv = curve(field)
    ks = [k for _m, k in group_pattern_scalars(field // 2)]
    ks += [d << (4 * j) for j in range(64) for d in range(1, 16) if d << (4 * j) < cv.n]
    ks += [0, 1, 2, cv.n - 1, cv.n - 2, (cv.n - 1) // 2]
    rng = R.SplitMix64(0xBA5E + field)
    n = _pad(len(ks), N_VALUE)
    ks += [rng.below(cv.n) for _ in range(n - len(ks))]
    return tuple(ks)


def _base_mul_counts(field, ks):
    c = {f"groups_{m:04b}": 0 for m in range(16)}
    for k in ks:
        c[f"groups_{group_mask(k):04b}"] += 1
    entries = {d << (4 * j) for j in range(64) for d in range(1, 16) if d << (4 * j) < curve(field).n}
    c["table_entries"] = len(entries & set(ks))
    c["table_entries_all"] = len(entries)
    c["zero"] = sum(k == 0 for k in ks)
    return c


def case_base_mul(lanes):
    """k G from all 64 windows: sign_window_sum<CV, 8> (lanes = 1), body_base_mul_quad (lanes = 4: identical words in the
    four lanes)"""
    def build(field):
        ks = base_mul_scalars(field)
        pts = kG(field, ks)
        want = [("point", pts[k]) if k else ("empty",) for k in ks]
        kinds = [f"groups_{group_mask(k):04b}" for k in ks]
        inp = pack(ks, 8)
        return Case(inp, point_check(field, inp, want, kinds, lanes=lanes, lanes_equal=lanes == 4), _base_mul_counts(field, ks), kinds)
    return build


def case_window_sum2(field):
    """lane j: the sum over windows 16 j .. 16 j + 15 = (group j of k) 2^(64 j) G"""
    ks = base_mul_scalars(field)
    parts = [[((k >> (64 * j)) & (2**64 - 1)) << (64 * j) for j in range(4)] for k in ks]
    pts = kG(field, [v for row in parts for v in row])
    n = curve(field).n
    want = [[("point", pts[v % n]) if v else ("empty",) for v in row] for row in parts]
    kinds = [f"groups_{group_mask(k):04b}" for k in ks]
    inp = pack(ks, 8)
    return Case(inp, point_check(field, inp, want, kinds, lanes=4), _base_mul_counts(field, ks), kinds)


# ---- recovery -------------------------------------------------------------------------------------------------------------
def is_residue(p, t):
    return t % p == 0 or pow(t, (p - 1) // 2, p) == 1


def _sqrt_values(field):
    p = curve(field).p
    rng = R.SplitMix64(0x5097 + field)
    vals = [0, 1, 2, 4, p - 1, p - 2]
    vals += [rng.below(p) ** 2 % p for _ in range(250)]
    vals += list(PI.operand_set(field)[:300])
    while len(vals) < 900:
        vals.append(rng.below(p))
    return vals


def case_recover_sqrt(field):
    p = curve(field).p
    vals = _sqrt_values(field)
    rows = [slot(v) + [0] for v in vals]
    kinds = ["canonical"] * len(vals)
    if field == 0:
        forms = PI.tight_forms()
        for f in forms[::max(1, len(forms) // 120)]:
            vals.append(PI.limb_value(f) % p)
            rows.append(list(f) + [2])
            kinds.append("tight")
    rng = R.SplitMix64(0x5098 + field)
    n = _pad(len(vals), N_VALUE)
    while len(vals) < n:
        vals.append(rng.below(p))
        rows.append(slot(vals[-1]) + [0])
        kinds.append("canonical")
    counts = {"residue": sum(is_residue(p, v) for v in vals), "non_residue": sum(not is_residue(p, v) for v in vals),
              "tight": kinds.count("tight")}
    for v in (0, 1, 2, 4, p - 1, p - 2):
        counts[f"t_{v if v < 8 else v - p}"] = vals.count(v)
    return PI.exact_case(np.array(rows, np.uint32), pack([pow(v, (p + 1) // 4, p) for v in vals], 8), counts, kinds)


DECOMPRESS_CLASSES = ("residue_even", "residue_odd", "non_residue_even", "non_residue_odd")


def case_recover_decompress(field):
    cv = curve(field)
    p = cv.p
    rng = R.SplitMix64(0xDEC0 + field)
    xs = [0, 1, 2, 4, p - 1, p - 2] * 2 + [(1 << 255) + rng.below(p - (1 << 255)) for _ in range(100)]
    xs += list(PI.operand_set(field)[:200])
    n = _pad(len(xs), N_VALUE)
    xs += [rng.below(p) for _ in range(n - len(xs))]
    odd = [(i ^ (i >> 3)) & 1 for i in range(n)]
    odd[0:12] = [0] * 6 + [1] * 6
    want, kinds = [], []
    for x, o in zip(xs, odd):
        t = (x * x * x + cv.a * x + cv.b) % p
        y = pow(t, (p + 1) // 4, p)
        ok = y * y % p == t
        if (y & 1) != o:
            y = (p - y) % p
        want.append([int(ok)] + slot(x)[:8] + slot(y)[:8])
        kinds.append(("residue" if ok else "non_residue") + ("_odd" if o else "_even"))
    counts = _count(kinds)
    counts["x_ge_2_255"] = sum(x >= 1 << 255 for x in xs)
    for v in (0, 1, 2, 4, p - 1, p - 2):
        counts[f"x_{v if v < 8 else v - p}"] = sum(1 for x in xs if x == v)
    return PI.exact_case(cat(pack(xs, 8), pack(odd, 1)), np.array(want, np.uint32), counts, kinds)


ABSCISSA_CLASSES = ("hi_just_below_p", "hi_equal_p", "hi_above_p", "hi_crosses_2_256", "lo_ge_p", "lo_below_p")


def abscissa_kind(cv, r, hi):
    x = r + (cv.n if hi else 0)
    if not hi:
        return "lo_ge_p" if r >= cv.p else "lo_below_p"
    if x >= 1 << 256:
        return "hi_crosses_2_256"
    return "hi_equal_p" if x == cv.p else "hi_above_p" if x > cv.p else "hi_just_below_p" if cv.p - x <= 4 else "hi_below_p"


def case_recover_abscissa(field):
    cv = curve(field)
    p, n = cv.p, cv.n
    rows = [(p - n - d, 1) for d in (1, 2, 3, 4)] + [(p - n, 1)] * 4 + [(p - n + d, 1) for d in (1, 2, 3, 1 << 64)]
    rows += [((1 << 256) - n + d, 1) for d in (-2, -1, 0, 1, 2)] + [((1 << 256) - 1, 1), (n - 1, 1), (n, 1)]
    rows += [(v, 0) for v in (p - 1, p, p + 1, (1 << 256) - 1, n, n - 1, 0, 1, p + 2)]
    rng = R.SplitMix64(0xAB5C + field)
    total = _pad(len(rows), N_VALUE)
    while len(rows) < total:
        j = len(rows)
        r = rng.below(1 << 256) if j % 3 == 0 else rng.below(n) if j % 3 == 1 else _rand(rng, p - n)
        rows.append((r, j & 1))
    kinds = [abscissa_kind(cv, r, hi) for r, hi in rows]
    want = []
    for r, hi in rows:
        x = r + (n if hi else 0)
        want.append([int(x < p)] + slot(x % (1 << 256))[:8])
    inp = cat(pack([r for r, _ in rows], 8), pack([hi for _, hi in rows], 1))
    return PI.exact_case(inp, np.array(want, np.uint32), _count(kinds), kinds)


def var_mul_scalars(cv, rng):
    """[(kind, u2)]: recover_inputs' u2 patterns, below n; u2 = 0 is the function's own empty result"""
    n = cv.n
    out = [("digit", d << (2 * w)) for w in RI.DIGIT_WINDOWS for d in (1, 2, 3)]
    out += [("top_only", d << 254) for d in (1, 2, 3)]
    out += [("zero_top", (rng.below(n) >> 2) | 1) for _ in range(3)]
    out += [("n_minus_1", n - 1), ("n_minus_1", n - 2), ("zero", 0), ("zero", 0)]
    out += [("small", v) for v in (1, 2, 3, 4, 5, 15, 16)]
    assert all(u < n for _k, u in out)
    return out


def case_recover_var_mul(field):
    cv = curve(field)
    rng = R.SplitMix64(0x7A2 + field)
    known, lifted = known_points(field), lifted_points(field)
    rows = []                                                          # kind, point, its log or None, u2
    for j, (kind, u2) in enumerate(var_mul_scalars(cv, rng)):
        d, pt = known[(3 * j + 1) % len(known)]
        rows.append((kind, pt, d, u2))
    for j, pt in enumerate(lifted[:24]):
        if j % 6 == 5:
            rows.append(("lifted_zero", pt, None, 0))
        else:
            rows.append(("lifted", pt, None, (1 + j % 3) << (2 * (11 * j % 127)) if j % 2 else 1 + rng.below(cv.n - 1)))
    total = _pad(len(rows), N_MUL)
    while len(rows) < total:
        d, pt = known[rng.next() % len(known)]
        rows.append(("fill", pt, d, 1 + rng.below(cv.n - 1)))
    pts = kG(field, [u * d for _k, _p, d, u in rows if d is not None])
    want = []
    for _k, pt, d, u in rows:
        s = pts[u * d % cv.n] if d is not None else cv.mul(u, pt)
        want.append(("point", s) if u else ("empty",))
    kinds = [k for k, *_ in rows]
    inp = cat(pack([p[0] for _k, p, _d, _u in rows], 8), pack([p[1] for _k, p, _d, _u in rows], 8), pack([u for *_x, u in rows], 8))
    return Case(inp, point_check(field, inp, want, kinds), _count(kinds), kinds)


# ---- pmsm.hpp: digits, storage, the curve test, the chunk reduction ------------------------------------------------------------
def signed_digits(k, c):
    """the unique digits with k = sum d_w 2^(c w), -2^(c-1) < d_w <= 2^(c-1), w < 256 / c + 1"""
    out, carry = [], 0
    for _ in range(256 // c + 1):
        d = (k & ((1 << c) - 1)) + carry
        k >>= c
        carry = 1 if d > 1 << (c - 1) else 0
        out.append(d - (carry << c))
    assert k == 0 and carry == 0
    return out


def digit_scalars(field, c):
    cv = curve(field)
    half, windows = 1 << (c - 1), 256 // c + 1
    ks = [("edge", k) for k in MN.edge_scalars(cv)]
    ks += [("boundary", k) for k in MN.boundary_scalars(c)] + [("max_digit", k) for k in MN.max_digit_scalars(c)]
    rng = R.SplitMix64(0xD161 + 16 * field + c)
    for tag, w in (("half_bottom", 0), ("half_middle", windows // 2), ("half_top_but_one", windows - 2)):
        ks += [(tag, half << (c * w)), (tag, (half << (c * w)) | _rand(rng, 1 << (c * w)))]   # alone; over random lower windows
    ks += [("all_ones", (1 << 256) - 1), ("all_ones", (1 << 256) - 1)]
    ks += [("ge_n", cv.n + _rand(rng, (1 << 256) - cv.n)) for _ in range(20)] + [("ge_n", cv.n), ("ge_n", cv.n + 1), ("ge_n", (1 << 256) - 2)]
    n = _pad(len(ks), N_VALUE)
    ks += [("fill", rng.below(1 << 256)) for _ in range(n - len(ks))]
    return ks


def case_for_digits(c):
    def build(field):
        ks = digit_scalars(field, c)
        half, windows = 1 << (c - 1), 256 // c + 1
        kinds = [t for t, _k in ks]
        vals = [k for _t, k in ks]
        want = np.zeros((len(vals), 66), np.int64)
        for i, k in enumerate(vals):
            d = signed_digits(k, c)
            assert len(d) == windows and sum(x << (c * w) for w, x in enumerate(d)) == k and all(-half < x <= half for x in d)
            want[i, :windows] = d
        counts = _count(kinds)
        for tag, w in (("half_bottom", 0), ("half_middle", windows // 2), ("half_top_but_one", windows - 2)):   # from the inputs alone
            counts["raw_" + tag] = sum(1 for k in vals if (k >> (c * w)) & ((1 << c) - 1) == half)
        inp = pack(vals, 8)
        exact = PI.exact_case(inp, want.astype(np.uint32), counts, kinds)

        def check(out):
            got = out[:, 0, :].astype(np.int32).astype(object)
            for i, k in enumerate(vals):                               # the header's three statements, then every word
                d = [int(x) for x in got[i, :windows]]
                assert sum(x << (c * w) for w, x in enumerate(d)) == k, ("sum", kinds[i], hex(k), d)
                assert all(-half < x <= half for x in d), ("range", kinds[i], hex(k), d)
                assert not any(got[i, windows:]), ("windows", kinds[i], hex(k))
            exact.check(out)
        return Case(inp, check, counts, kinds)
    return build


def case_msm_load_store(field):
    cv = curve(field)
    rng = R.SplitMix64(0x1057 + field)
    ops = PI.operand_set(field)
    rows, kinds = [], []
    for j in range(N_VALUE):
        X, Y, Z = ops[rng.next() % len(ops)], ops[rng.next() % len(ops)], ops[rng.next() % len(ops)]
        if j % 4 == 0:
            X, Y, Z = (X or 1), (Y or 1), 0
        elif j % 4 == 1:
            Z = Z or 1
        elif j % 16 == 2:
            Z = 1
        rows.append((X, Y, Z))
        kinds.append("neutral" if Z == 0 else "point")
    want = [slot(X)[:8] + slot(Y)[:8] + slot(Z)[:8] + [1] if Z else [0] * 25 for X, Y, Z in rows]
    inp = cat(*[pack([r[k] for r in rows], 8) for k in range(3)])
    return PI.exact_case(inp, np.array(want, np.uint32), _count(kinds), kinds)


def case_msm_on_curve(field):
    cv = curve(field)
    p = cv.p
    pts = all_points(field)
    rng = R.SplitMix64(0x0C0C + field)
    rows = []
    for j, (x, y) in enumerate(pts):
        rows += [("on", x, y), ("on", x, p - y), ("off", x, (y + 1) % p), ("off", (x + 1) % p, y)]
        if j < 20:
            rows += [("x_ge_p", x + p if x + p < 1 << 256 else p, y), ("y_ge_p", x, y + p if y + p < 1 << 256 else p),
                     ("x_ge_p", (1 << 256) - 1, y), ("y_ge_p", x, p)]
    rows += [("off", 0, 0), ("off", 0, 1), ("off", 1, 0), ("x_ge_p", p, 0)]
    n = _pad(len(rows), N_VALUE)
    while len(rows) < n:
        rows.append(("off", rng.below(p), rng.below(p)))
    kinds = [k for k, _x, _y in rows]
    want = [[int(x < p and y < p and cv.on_curve((x, y)))] for _k, x, y in rows]
    assert all((w[0] == 1) == (k == "on") for w, k in zip(want, kinds))
    inp = cat(pack([x for _k, x, _y in rows], 8), pack([y for _k, _x, y in rows], 8))
    return PI.exact_case(inp, np.array(want, np.uint32), _count(kinds), kinds)


def chunk_geometry(c):
    """pmsm.hpp msm_plan: windows, buckets per window, buckets per chunk, chunks per window"""
    buckets = 1 << (c - 1)
    chunk = min(buckets, 32)
    return 256 // c + 1, buckets, chunk, buckets // chunk


CHUNK_CLASSES = ("all_neutral", "single_first", "single_middle", "single_last", "all_same", "alternating", "z_not_one", "mixture")


def case_msm_chunk(c):
    def build(field):
        cv = curve(field)
        windows, _buckets, chunk, chunks = chunk_geometry(c)
        lanes = windows * chunks
        known = known_points(field)
        rng = R.SplitMix64(0xC4A0 + 16 * field + c)
        elems, kinds = [], []                                           # per element: [(log or 0, Z)] per bucket
        for e in range(N_MUL):
            kind = CHUNK_CLASSES[e % len(CHUNK_CLASSES)]
            d0 = known[rng.next() % len(known)][0]
            if kind == "all_neutral":
                b = [(0, 0)] * chunk
            elif kind.startswith("single"):
                pos = {"single_first": 0, "single_middle": chunk // 2, "single_last": chunk - 1}[kind]
                b = [(d0, 1) if j == pos else (0, 0) for j in range(chunk)]
            elif kind == "all_same":
                b = [(d0, 1)] * chunk
            elif kind == "alternating":
                b = [(d0 if j % 2 == 0 else cv.n - d0, 1) for j in range(chunk)]
            elif kind == "z_not_one":
                b = [(known[rng.next() % len(known)][0], 2 + rng.below(cv.p - 2)) for j in range(chunk)]
            else:
                b = [(known[rng.next() % len(known)][0], 1 + rng.below(cv.p - 1)) if rng.next() % 3 else (0, 0) for j in range(chunk)]
            elems.append(b)
            kinds.append(kind)
        pts = kG(field, [d for b in elems for d, _z in b])
        rows, totals = [], []
        for e, b in enumerate(elems):
            a0 = ((e % lanes) * CHUNK_STRIDE % lanes) % chunks * chunk      # the chunk's first global bucket index
            words, total = [], 0
            for j, (d, z) in enumerate(b):
                if d == 0:
                    words += [0] * 24
                    continue
                x, y = pts[d]
                words += slot(x * z * z % cv.p)[:8] + slot(y * pow(z, 3, cv.p) % cv.p)[:8] + slot(z)[:8]
                total += (a0 + j + 1) * d
            rows.append(words)
            totals.append(total % cv.n)
        sums = kG(field, totals)
        want = [("point", sums[t]) if t else ("empty",) for t in totals]
        inp = np.array(rows, np.uint32)
        pc = point_check(field, inp, want, kinds)

        def check(out):                                                   # chunkpart: Z = 0 is the neutral element
            z = np.any(out[:, 0, 16:24] != 0, axis=1).astype(np.uint32)
            empty_ok = [i for i in range(len(z)) if z[i] == 0 and out[i, 0].any()]
            assert not empty_ok, ("a neutral chunkpart is stored as zeros", empty_ok[0])
            pc(np.concatenate([out, z.reshape(-1, 1, 1)], axis=2))
        counts = _count(kinds)
        counts["first_bucket_indices"] = len({((e % lanes) * CHUNK_STRIDE % lanes) % chunks for e in range(N_MUL)})
        return Case(inp, check, counts, kinds)
    return build


# ---- the GLV rounding ----------------------------------------------------------------------------------------------------
REMS = ("0", "1", "half_m1", "half", "half_p1", "half_p2", "n_m2", "n_m1")


def rounding_rems():
    n = R.N
    return dict(zip(REMS, (0, 1, (n - 1) // 2 - 1, (n - 1) // 2, (n + 1) // 2, (n + 1) // 2 + 1, n - 2, n - 1)))


def rounding_scalars():
    """[(class, constant name, k)]: the 16 scalars k = r c^-1 mod n whose product c k has remainder r at a place where
    glv_round_div rounds"""
    return [(f"{cn}_rem_{rn}", cn, r * pow(c, -1, R.N) % R.N) for cn, c in GLV_CONSTS.items() for rn, r in rounding_rems().items()]


def rounding_batch():
    """the 16 rounding-boundary scalars and their neighbours k - 1, k + 1 (mod n), with the class of each boundary scalar"""
    ks, kinds = [], []
    for kind, _cn, k in rounding_scalars():
        ks += [k, (k - 1) % R.N, (k + 1) % R.N]
        kinds += [kind, "neighbour", "neighbour"]
    return ks, kinds


def _rem_class(c, k):
    inv = {v: n for n, v in rounding_rems().items()}
    return inv.get(c * k % R.N)


def case_reduce_wide_n4(field):
    n = R.N
    rows = [(f"{cn}_rem_{_rem_class(c, k)}", c * k) for _kind, cn, k in rounding_scalars() for c in (GLV_CONSTS[cn],)]
    rows += [(f"{cn}_k_edge", c * k) for cn, c in GLV_CONSTS.items() for k in (0, 1, n - 1)]
    rows += [("all_ones", (1 << 384) - 1), ("all_ones", (1 << 384) - 1)]
    rows += [("word_pattern", sum(w << (32 * i) for i in range(12))) for w in PI.PATTERNS]
    rows += [("multiple_of_n", n * v) for v in (1, 2, (1 << 128) - 1, (1 << 128))] + [("multiple_of_n", n * v - 1) for v in (1, 2, 1 << 128)]
    rng = R.SplitMix64(0x91DE)
    total = _pad(len(rows), N_VALUE)
    while len(rows) < total:
        j = len(rows)
        rows.append(("product", _rand(rng, 1 << 128) * rng.below(n)) if j % 2 else ("fill", _rand(rng, 1 << 384)))
    kinds = [k for k, _v in rows]
    vals = [v for _k, v in rows]
    want = cat(pack([v % n for v in vals], 8), pack([v // n for v in vals], 9))
    return PI.exact_case(pack(vals, 12), want, _count(kinds), kinds)


def case_glv_round_div(cn):
    def build(field):
        n, c = R.N, GLV_CONSTS[cn]
        ks, _ = rounding_batch()
        ks += [0, 1, n - 1, n - 2, (n - 1) // 2, (n + 1) // 2]
        rng = R.SplitMix64(0x61F + (cn == "mb1"))
        ks += [rng.below(n) for _ in range(_pad(len(ks), N_VALUE) - len(ks))]
        kinds = [f"{cn}_rem_{_rem_class(c, k)}" if _rem_class(c, k) is not None else "other" for k in ks]
        counts = _count(kinds)
        counts["k_edges"] = sum(k in (0, 1, n - 1) for k in ks)
        return PI.exact_case(pack(ks, 8), pack([(2 * c * k + n) // (2 * n) for k in ks], 8), counts, kinds)
    return build


# ---- the table ---------------------------------------------------------------------------------------------------------
TABLE = {}   # name -> (fields, builder(field) -> Case)


def _reg(name, fields, builder):
    TABLE[name] = (fields, builder)


_reg("sign_window_sum8", CURVE_FIELDS, case_base_mul(1))
_reg("sign_window_sum2", CURVE_FIELDS, case_window_sum2)
_reg("sign_sum_add", CURVE_FIELDS, case_sign_sum_add)
_reg("body_base_mul_quad", CURVE_FIELDS, case_base_mul(4))
_reg("sign_to_affine_xy", CURVE_FIELDS, case_sign_to_affine(True))
_reg("sign_to_affine_x", CURVE_FIELDS, case_sign_to_affine(False))
_reg("recover_sqrt", CURVE_FIELDS, case_recover_sqrt)
_reg("recover_decompress", CURVE_FIELDS, case_recover_decompress)
_reg("recover_abscissa", CURVE_FIELDS, case_recover_abscissa)
_reg("recover_var_mul", CURVE_FIELDS, case_recover_var_mul)
_reg("recover_final_add", CURVE_FIELDS, case_recover_final_add)
for _c in range(4, 13):
    _reg(f"msm_for_digits_c{_c}", CURVE_FIELDS, case_for_digits(_c))
_reg("msm_add_mixed", CURVE_FIELDS, case_msm_add(True))
_reg("msm_add", CURVE_FIELDS, case_msm_add(False))
_reg("msm_dbl", CURVE_FIELDS, case_msm_dbl)
_reg("msm_load_store", CURVE_FIELDS, case_msm_load_store)
_reg("msm_on_curve", CURVE_FIELDS, case_msm_on_curve)
for _c in CHUNK_WIDTHS:
    _reg(f"body_msm_chunk_c{_c}", CURVE_FIELDS, case_msm_chunk(_c))
_reg("reduce_wide_n4", (1,), case_reduce_wide_n4)
_reg("glv_round_div_b2", (1,), case_glv_round_div("b2"))
_reg("glv_round_div_mb1", (1,), case_glv_round_div("mb1"))

PAIRS = [(n, f) for n, (fields, _) in TABLE.items() for f in fields]
IDS = [f"{n}-{FIELD_NAMES[f]}" for n, f in PAIRS]
MUL_OPS = ("recover_var_mul",) + tuple(f"body_msm_chunk_c{c}" for c in CHUNK_WIDTHS)


@functools.lru_cache(maxsize=None)
def case(name, field):
    return TABLE[name][1](field)


def required_counts(name, field):
    """what a batch must contain (count name -> least), checked from the inputs alone"""
    if name in ("msm_add", "msm_add_mixed", "sign_sum_add"):
        return {k: LEAST for k in add_classes(field)}
    if name == "recover_final_add":
        return {k: LEAST for k in add_classes(field, b_never_empty=True)}
    if name in TABLE_OPS:
        req = {f"groups_{m:04b}": 2 for m in range(16)}
        req.update(zero=1, table_entries=case(name, field).counts["table_entries_all"])
        return req
    if name.startswith("sign_to_affine"):
        return {k: LEAST for k in ("zero_z", "point") + (("zero_z_tight", "point_tight") if field == 0 else ())}
    if name == "msm_dbl":
        return {k: LEAST for k in ("empty", "point") + (("empty_tight", "point_tight") if field == 0 else ())}
    if name == "recover_sqrt":
        req = {"residue": 200, "non_residue": 200, "t_0": 1, "t_1": 1, "t_2": 1, "t_4": 1, "t_-1": 1, "t_-2": 1}
        if field == 0:
            req["tight"] = 100
        return req
    if name == "recover_decompress":
        req = {k: 100 for k in DECOMPRESS_CLASSES}
        req.update({"x_ge_2_255": 100, "x_0": 2, "x_1": 2, "x_2": 2, "x_4": 2, "x_-1": 2, "x_-2": 2})
        return req
    if name == "recover_abscissa":
        return {k: 4 for k in ABSCISSA_CLASSES}
    if name == "recover_var_mul":
        return {"digit": 3 * len(RI.DIGIT_WINDOWS), "top_only": 3, "zero_top": 3, "n_minus_1": 1, "zero": 1, "lifted": 10, "lifted_zero": 1}
    if name.startswith("msm_for_digits"):
        return {"edge": 8, "boundary": 3, "max_digit": 2, "raw_half_bottom": 2, "raw_half_middle": 2, "raw_half_top_but_one": 2,
                "all_ones": 1, "ge_n": 20, "fill": 500}
    if name == "msm_load_store":
        return {"neutral": 200, "point": 200}
    if name == "msm_on_curve":
        return {"on": 100, "off": 100, "x_ge_p": 20, "y_ge_p": 20}
    if name.startswith("body_msm_chunk"):
        req = {k: 8 for k in CHUNK_CLASSES}
        req["first_bucket_indices"] = chunk_geometry(int(name.rsplit("c", 1)[1]))[3]
        return req
    if name == "reduce_wide_n4":
        req = {f"{cn}_rem_{rn}": 1 for cn in GLV_CONSTS for rn in REMS}
        req.update({"b2_k_edge": 3, "mb1_k_edge": 3, "all_ones": 1, "fill": 300, "product": 300})
        return req
    if name.startswith("glv_round_div"):
        cn = name.rsplit("_", 1)[1]
        req = {f"{cn}_rem_{rn}": 1 for rn in REMS}
        req["k_edges"] = 3
        return req
    raise KeyError(name)


def check_counts(name, field):
    c = case(name, field)
    n = c.inp.shape[0]
    assert n % 64 == 1 and n >= (N_MUL if name in MUL_OPS else N_VALUE), (name, n)
    for k, least in required_counts(name, field).items():
        assert c.counts.get(k, 0) >= least, (name, field, k, c.counts.get(k, 0), least)
    return c


def run_case(probe, name, field):
    """one (op, field): the batch holds the classes it claims, is a partial wave / lone quad, and the outputs are right"""
    c = check_counts(name, field)
    c.check(probe.run(name, field, c.inp))
