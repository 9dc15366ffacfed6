"""Inputs of the MSM and fixed-base curve programs shared by the CPU and GPU tests: the edge rows, the scalar mix of the
exhaustive comparisons (uniform / structured / sparse), the points that meet the gadgets' blinding point, and the list of
elements the reference panics on, constructed from the inputs alone (never from an implementation's flags)."""
import numpy as np

import p2e_ref as R
from parity_checks import structured_values

CURVES = [R.SECP256K1, R.P256]
FLAGGED = (7, 10, 11)   # of msm_inputs: n = m = 0, p = q, p = -q
EDGE_ROWS = 12          # rows of msm_inputs that carry an edge case
FB_EDGE = 6             # rows of exhaustive_fb_inputs that carry an edge case
FB_FLAGGED = (4,)       # of them: k = 0 (the unblinding add meets its own negative)


def b32(v):
    return np.frombuffer(int(v).to_bytes(32, "little"), np.uint8).copy()


def ints(a):
    return [int.from_bytes(bytes(bytearray(r)), "little") for r in np.asarray(a)]


def pack(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), np.uint8).reshape(-1, 32).copy()


def msm_inputs(curve_id, n, seed):
    """(px, py, qx, qy, n, m) as lists of ints: random points (public keys of synthetic signatures), random scalars, and
    the edge cases in the first EDGE_ROWS rows"""
    import plonky2_ecdsa_amd as p2e
    cv = CURVES[curve_id]
    a = p2e.synth_signatures_curve(curve_id, seed=seed, n=n)
    b = p2e.synth_signatures_curve(curve_id, seed=seed + 1, n=n)
    px, py, qx, qy = ints(a[3]), ints(a[4]), ints(b[3]), ints(b[4])
    ns, ms = ints(a[0]), ints(b[0])
    edge = [(1, 1), (cv.n - 1, 5), (7, cv.n - 1), ((1 << 255) + 12345, (1 << 255) | 3), (123456789, 0), (0, 987654321),
            (ns[6], ns[6]), (0, 0), (1, 2), ((1 << 256) - 1, 3)]
    for i, (x, y) in enumerate(edge):
        ns[i], ms[i] = x, y
    px[10], py[10] = qx[10], qy[10]                  # p = q: the table's p + q is a doubling (flagged)
    px[11], py[11] = qx[11], (cv.p - qy[11]) % cv.p  # p = -q (flagged)
    return [px, py, qx, qy, ns, ms]


def fb_inputs(cv, n, seed):
    rng = R.SplitMix64(seed)
    ks = [rng.below(cv.n) for _ in range(n)]
    ks[0], ks[1], ks[2], ks[3] = 1, cv.n - 1, 16, (1 << 255) + 99   # (k = 0 is the unblinding add's inverse of zero)
    return ks


def sparse_values(seed, count):
    """256-bit values with one to five non-zero 2-bit or 4-bit digits: the windows' should_add is 0 almost everywhere, so
    the conditional add's not_b products carry the point"""
    rng = np.random.default_rng(seed)
    vals = []
    for _ in range(count):
        width = 2 if rng.integers(0, 2) else 4
        v = 0
        for _k in range(int(rng.integers(1, 6))):
            pos = int(rng.integers(0, 256 // width))
            v |= int(rng.integers(1, 1 << width)) << (width * pos)
        vals.append(v)
    return vals


def mixed_scalars(seed, count):
    """(count, 32) bytes of raw 256-bit scalars: element i is uniform, structured (parity_checks.structured_values: runs of
    ones / zeros / alternating words, not reduced) or sparse for i % 3 = 0, 1, 2 -- interleaved, so every workgroup of a
    batch sees all three"""
    out = np.random.default_rng(seed).integers(0, 256, size=(count, 32), dtype=np.uint8)
    k1, k2 = len(range(1, count, 3)), len(range(2, count, 3))
    if k1:
        out[1::3] = pack(structured_values(seed + 1, k1))
    if k2:
        out[2::3] = pack(sparse_values(seed + 2, k2))
    return out


def exhaustive_msm_inputs(curve_id, n, seed):
    """([px, py, qx, qy, n, m] as (n, 32) byte arrays, flagged): distinct points per element, mixed_scalars, the edge rows
    of msm_inputs in the first EDGE_ROWS rows and again, in reverse order, in the last EDGE_ROWS rows (the last lanes of the
    tail workgroup; reversed so that the very last lane is an element whose columns are compared); flagged = the rows the
    reference panics on (n = m = 0, p = q, p = -q of each copy)"""
    import plonky2_ecdsa_amd as p2e
    assert n >= 2 * EDGE_ROWS
    cv = CURVES[curve_id]
    a = p2e.synth_signatures_curve(curve_id, seed=seed, n=n)
    b = p2e.synth_signatures_curve(curve_id, seed=seed + 1, n=n)
    px, py, qx, qy = a[3].copy(), a[4].copy(), b[3].copy(), b[4].copy()
    ns, ms = mixed_scalars(seed + 2, n), mixed_scalars(seed + 5, n)
    small = msm_inputs(curve_id, 32, seed)
    for row in (lambda k: k, lambda k: n - 1 - k):       # the second copy in reverse order: the last lane is a clean row
        for k in range(EDGE_ROWS):
            ns[row(k)], ms[row(k)] = b32(small[4][k]), b32(small[5][k])
        px[row(10)], py[row(10)] = qx[row(10)], qy[row(10)]
        px[row(11)] = qx[row(11)]
        py[row(11)] = b32((cv.p - ints(qy[row(11):row(11) + 1])[0]) % cv.p)
    flagged = sorted([k for k in FLAGGED] + [n - 1 - k for k in FLAGGED])
    return [px, py, qx, qy, ns, ms], flagged


def exhaustive_fb_inputs(curve_id, n, seed):
    """((n, 32) scalars, flagged): mixed_scalars with the edge rows of fb_inputs, k = 0 (flagged) and 2^256 - 1 in the
    first FB_EDGE rows and again in the last FB_EDGE rows"""
    assert n >= 2 * FB_EDGE
    cv = CURVES[curve_id]
    ks = mixed_scalars(seed, n)
    edge = pack(fb_inputs(cv, 4, seed)[:4] + [0, (1 << 256) - 1])
    for off in (0, n - FB_EDGE):
        ks[off:off + FB_EDGE] = edge
    return ks, sorted(off + k for off in (0, n - FB_EDGE) for k in FB_FLAGGED)


def blinding_bases(cv):
    """the bases / points that meet the blinding point KeccakHash::<32>(F::ZERO) * G of the curve's gadgets"""
    rando = cv.hash_point(32)
    return {"rando": rando, "-rando": cv.neg(rando), "2rando": cv.double(rando)}


def fb_flagged_on_a_rando_multiple(cv, c, ks):
    """fixed_base_curve_mul_circuit with base = c * rando: every point of the walk is a known multiple of rando, so the
    additions that meet equal x coordinates (the reference's inverse of zero) follow from the scalars alone.  Returns the
    flagged rows of the scalars ks (ints)."""
    n = cv.n
    out = []
    for row, k in enumerate(ks):
        acc, hit = 1, False                           # result = rando
        for w in range(66):
            d = (k >> (4 * w)) & 15
            add = c * pow(16, w, n) * (d or 1) % n    # slot 0 := slot 1; the add is computed whatever should_add is
            hit |= acc == add or (acc + add) % n == 0
            if d:
                acc = (acc + add) % n
        hit |= acc == n - 1 or acc == 1               # the unblinding add of -rando
        if hit:
            out.append(row)
    return out


def blinding_msm_inputs(curve_id, n, seed):
    """(inputs as byte arrays, flagged) of an MSM batch in which every 8th row from EDGE_ROWS on has p or q (alternating
    every three such rows) replaced by rando, -rando, 2 rando in turn; the other point stays a distinct synthetic public
    key.  The table's rando + p (or + q) is a doubling or lands on infinity for +-rando (flagged); 2 rando meets nothing
    for scalars that are not tiny."""
    cv = CURVES[curve_id]
    ins, flagged = exhaustive_msm_inputs(curve_id, n, seed)
    pts = list(blinding_bases(cv).values())
    flagged = set(flagged)
    for j, i in enumerate(range(EDGE_ROWS, n - EDGE_ROWS, 8)):
        pt = pts[j % 3]
        x, y = (ins[0], ins[1]) if (j // 3) % 2 == 0 else (ins[2], ins[3])
        x[i], y[i] = b32(pt[0]), b32(pt[1])
        ins[4][i, 31] |= 0x40                          # (scalars with a high digit: 2 rando cannot meet a small multiple)
        ins[5][i, 31] |= 0x40
        if j % 3 != 2:
            flagged.add(i)
    return ins, sorted(flagged)


def blinding_fb_inputs(curve_id, name, n, seed):
    """(scalars, flagged) of a fixed-base batch on base = blinding_bases()[name]: exhaustive_fb_inputs, with the lowest
    window forced to a digit >= 2 except in the edge rows and every 16th row (with +-rando a lowest digit of 0 or 1 makes
    the very first window addition a doubling / the point at infinity: one row in eight of a uniform batch), and on
    2 rando the scalar (n - 1) / 2, whose last addition lands on infinity; flagged from fb_flagged_on_a_rando_multiple"""
    cv = CURVES[curve_id]
    ks, _ = exhaustive_fb_inputs(curve_id, n, seed)
    for i in range(FB_EDGE, n - FB_EDGE):
        if i % 16:
            ks[i, 0] |= 2
    ks[FB_EDGE + 1] = b32((cv.n - 1) // 2)
    c = {"rando": 1, "-rando": cv.n - 1, "2rando": 2}[name]
    return ks, fb_flagged_on_a_rando_multiple(cv, c, ints(ks))
