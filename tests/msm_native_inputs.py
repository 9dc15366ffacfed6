"""Inputs and independent expectations of the bucket-method multi-scalar multiplication (include/p2e.h p2e_point_msm;
test_point_msm_cpu.py, test_gpu_point_msm.py).

Nothing here uses the code under test.  Points with known discrete logs, P_i = d_i G, come from sign_inputs.base_points (the
C oracle's fixed-base walk); then  sum k_i P_i = (sum k_i d_i mod n) G  is one more such point.  -P is (n - d) G.  Points
without a known logarithm (lifted abscissas) are summed on Python integers with oracle/p2e_ref.py's Curve.mul / Curve.add.
A case is a Case tuple; `point` None in the expectation means the neutral element (zeros and MSM_NEUTRAL)."""
from collections import namedtuple
from functools import lru_cache

import numpy as np

import p2e_ref as R
import sign_inputs as S

CURVES = S.CURVES
MSM_OK, MSM_NEUTRAL, MSM_BAD_POINT = 0, 1, 2
WINDOW_AUTO, WINDOW_MIN, WINDOW_MAX = 0, 4, 12
POOL = 1024                       # distinct discrete logs per curve
SMALL_SIZES = (0, 1, 2, 63, 64, 65, 257)
MIXED_N = 1500
BALANCE_N = 4161                  # 65 waves and one lane; above every segment length the plan uses at this size
BOUNDARY_WIDTHS = (WINDOW_MIN, 8, WINDOW_MAX)

# kind, scalars (raw ints < 2^256), points ((x, y) ints; (0, 0) = neutral), expected point or None, status, rejected
# count, point_err list
Case = namedtuple("Case", "kind k pts point status bad point_err")


@lru_cache(maxsize=None)
def pool(curve_id):
    """[(d, d G)] for POOL fixed pseudo-random d in [1, n)"""
    cv = CURVES[curve_id]
    rng = R.SplitMix64(0xB0C0 + curve_id)
    ds = [1 + rng.below(cv.n - 1) for _ in range(POOL)]
    pts = S.base_points(curve_id, ds)
    return [(d, pts[d]) for d in ds]


def _case(curve_id, kind, ks, ds):
    """points d_i G (d = 0: the (0, 0) encoding of the neutral element), expectation (sum k_i d_i mod n) G"""
    cv = CURVES[curve_id]
    pts = S.base_points(curve_id, [d % cv.n for d in ds])
    total = sum((k % cv.n) * (d % cv.n) for k, d in zip(ks, ds)) % cv.n
    point = S.base_points(curve_id, [total])[total] if total else None
    coords = [pts[d % cv.n] if d % cv.n else (0, 0) for d in ds]
    return Case(kind, list(ks), coords, point, MSM_OK if point else MSM_NEUTRAL, 0, [0] * len(ks))


def uniform(curve_id, n, seed, first=0):
    """n uniform 256-bit scalars on the pool's points, point i being pool entry (first + i) mod POOL"""
    rng = R.SplitMix64(seed)
    pl = pool(curve_id)
    return _case(curve_id, "uniform", [rng.below(1 << 256) for _ in range(n)], [pl[(first + i) % POOL][0] for i in range(n)])


def edge_scalars(cv):
    n = cv.n
    return [0, 1, 2, 3, n - 1, n, n + 1, (1 << 256) - 1]


def boundary_scalars(width):
    """a single set bit at every window boundary - 1, + 0, + 1 of the given width"""
    bits = sorted({b for w in range(1, 256 // width + 1) for b in (width * w - 1, width * w, width * w + 1) if 0 <= b < 256})
    return [1 << b for b in bits]


def max_digit_scalars(width):
    """every raw digit 2^width - 1 (all ones below the top window), and every raw digit 2^(width-1), the largest signed one:
    both below 2^252 < n, so the reduction leaves them as they are and the carry runs through every window"""
    top = 252 // width
    return [(1 << (width * top)) - 1, sum((1 << (width - 1)) << (width * w) for w in range(top))]


def mixed(curve_id):
    """MIXED_N elements: every scalar edge, boundary bits and maximal digits for the widths MIN, 8 and MAX, all-ones, forty
    copies of one point with one scalar, P and -P with equal scalars, (0, 0) points, uniform filler"""
    cv = CURVES[curve_id]
    pl = pool(curve_id)
    rng = R.SplitMix64(0xA11 + curve_id)
    ks, ds, tags = [], [], []

    def put(tag, k, d):
        ks.append(k), ds.append(d), tags.append(tag)

    for i, k in enumerate(edge_scalars(cv)):
        put("edge", k, pl[i][0])
    for width in BOUNDARY_WIDTHS:
        for i, k in enumerate(boundary_scalars(width)):
            put("boundary%d" % width, k, pl[(7 * i + width) % POOL][0])
        for i, k in enumerate(max_digit_scalars(width)):
            put("max_digit%d" % width, k, pl[(3 * i + width) % POOL][0])
    put("all_ones", (1 << 255) - 1, pl[77][0])
    same_k = rng.below(1 << 256)
    for _ in range(40):
        put("same", same_k, pl[500][0])
    for i in range(6):
        k = rng.below(1 << 256)
        put("opposite", k, pl[600 + i][0])
        put("opposite", k, cv.n - pl[600 + i][0])
    for i in range(10):
        put("neutral_point", rng.below(1 << 256), 0)
    while len(ks) < MIXED_N:
        put("fill", rng.below(1 << 256), pl[len(ks) % POOL][0])
    order = list(range(MIXED_N))
    for i in range(MIXED_N - 1, 0, -1):   # the special elements spread over the batch
        j = rng.next() % (i + 1)
        order[i], order[j] = order[j], order[i]
    c = _case(curve_id, "mixed", [ks[i] for i in order], [ds[i] for i in order])
    return c, [tags[i] for i in order]


def cancelling(curve_id):
    """(k, P), (n - k, P) as the whole batch: the neutral element"""
    cv = CURVES[curve_id]
    d = pool(curve_id)[9][0]
    k = R.SplitMix64(0xCA + curve_id).below(cv.n - 1) + 1
    return _case(curve_id, "cancelling", [k, cv.n - k], [d, d])


def only_neutral_points(curve_id):
    rng = R.SplitMix64(0x0E + curve_id)
    return _case(curve_id, "only_neutral", [rng.below(1 << 256) for _ in range(5)], [0] * 5)


def single(curve_id, k):
    """n = 1 (k = 3: the running sum of the bucket reduction meets itself)"""
    return _case(curve_id, "single%d" % k, [k], [pool(curve_id)[k][0]])


def equal_scalars(curve_id, n=BALANCE_N):
    """all scalars equal: every point of a window lands in one bucket (and the pool's points repeat inside it)"""
    cv = CURVES[curve_id]
    k = R.SplitMix64(0xE9 + curve_id).below(cv.n - 2) + 2
    pl = pool(curve_id)
    return _case(curve_id, "equal_scalars", [k] * n, [pl[i % POOL][0] for i in range(n)])


def lift(cv, x):
    """a point with abscissa >= x (both primes are 3 mod 4)"""
    while True:
        t = (x * x * x + cv.a * x + cv.b) % cv.p
        y = pow(t, (cv.p + 1) // 4, cv.p)
        if y * y % cv.p == t:
            return x, y
        x += 1


@lru_cache(maxsize=None)
def arbitrary(curve_id, n=40):
    """points without a known logarithm, summed on Python integers"""
    cv = CURVES[curve_id]
    rng = R.SplitMix64(0xAB + curve_id)
    pts = [lift(cv, rng.below(cv.p)) for _ in range(n)]
    ks = [rng.below(1 << 256) for _ in range(n)]
    total = None
    for k, pt in zip(ks, pts):
        total = cv.add(total, cv.mul(k % cv.n, pt))
    return Case("arbitrary", ks, pts, total, MSM_OK if total else MSM_NEUTRAL, 0, [0] * n)


REJECT_KINDS = ("x_eq_p", "y_eq_p", "x_all_ones", "off_curve")


def rejected(curve_id, kind, position, n=9):
    """a batch of n valid elements with one rejected point at `position` ('first', 'middle', 'last')"""
    cv = CURVES[curve_id]
    base = uniform(curve_id, n, 0x4E + curve_id, first=40)
    at = {"first": 0, "middle": n // 2, "last": n - 1}[position]
    x, y = base.pts[at]
    bad_pt = {"x_eq_p": (cv.p, y), "y_eq_p": (x, cv.p), "x_all_ones": ((1 << 256) - 1, y), "off_curve": (x, (y + 1) % cv.p)}[kind]
    pts = list(base.pts)
    pts[at] = bad_pt
    return Case("rejected_%s_%s" % (kind, position), base.k, pts, None, MSM_BAD_POINT, 1, [int(i == at) for i in range(n)])


def arrays(case):
    """(k, px, py) as (n, 32) little-endian bytes, and the expected (outx (32,), outy (32,))"""
    n = len(case.k)
    pack = lambda v: S.pack(v) if n else np.zeros((0, 32), np.uint8)
    want = case.point or (0, 0)
    return (pack(case.k), pack([p[0] for p in case.pts]), pack([p[1] for p in case.pts]),
            S.pack([want[0]])[0].copy(), S.pack([want[1]])[0].copy())


def selftest_cases(curve_id):
    """what tests/emu_msm/msm_selftest carries: small cases of every kind, each with the widths it is run at"""
    widths = (WINDOW_AUTO, WINDOW_MIN, 8, WINDOW_MAX)
    out = [(uniform(curve_id, n, 0x57 + n), widths) for n in (0, 1, 2, 65)]
    out += [(single(curve_id, k), widths) for k in (1, 2, 3, 4, 17)]
    out += [(cancelling(curve_id), widths), (only_neutral_points(curve_id), widths), (equal_scalars(curve_id, 70), widths)]
    out += [(rejected(curve_id, kind, "middle"), (WINDOW_AUTO,)) for kind in REJECT_KINDS]
    cv = CURVES[curve_id]
    pl = pool(curve_id)
    ks = edge_scalars(cv) + max_digit_scalars(WINDOW_MIN) + max_digit_scalars(8) + max_digit_scalars(WINDOW_MAX)
    out.append((_case(curve_id, "edges", ks, [pl[i][0] for i in range(len(ks))]), widths))
    return out


def selftest_vectors():
    """the text of tests/emu_msm/msm_vectors.inc"""
    lines = ["// generated by tests/msm_native_inputs.py selftest_vectors() (test_point_msm_cpu.py keeps it current)",
             "// MSM_CASE(curve, window_bits, n, outx, outy, status, rejected) followed by its n MSM_POINT(k, px, py);",
             "// 256-bit values as big-endian hex"]
    for curve_id in (0, 1):
        for case, widths in selftest_cases(curve_id):
            want = case.point or (0, 0)
            wb = -1 if len(widths) > 1 else widths[0]   # -1: AUTO, MIN, 8 and MAX in turn
            lines.append('MSM_CASE(%d, %d, %d, "%064x", "%064x", %d, %d)' % (curve_id, wb, len(case.k), want[0], want[1], case.status, case.bad))
            for k, (x, y) in zip(case.k, case.pts):
                lines.append('MSM_POINT("%064x", "%064x", "%064x")' % (k, x, y))
    return "\n".join(lines) + "\n"
