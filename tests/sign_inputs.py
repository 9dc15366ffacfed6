"""Inputs and independent expectations of the key-derivation and signing tests (test_sign_cpu.py, test_gpu_sign.py).

Expectations are computed from nothing the code under test provides:
  points   k G and sk G from the C oracle's fixed-base walk (oracle/p2e_oracle.c p2e_oracle_curve_fixed_base with the curve's
           generator as the base), the final point extracted as tests/test_msm_fixed_base_cpu.py::_final_point does; an
           element the circuit oracle itself flags (k = 0, or a scalar whose partial sums meet the blinding point) gets
           the big-int value of oracle/p2e_ref.py's Curve.mul instead -- none is skipped;
  s        Python integers: pow(k, -1, n) * (msg + r * sk) % n;
  flags    from the inputs alone: {sk = 0 mod n} for the key call, {k = 0 mod n} for the signer.
Scalars are reduced modulo n before they reach the oracle (the calls under test take them modulo n)."""
import numpy as np

import oracle_c
import p2e_ref as R

CURVES = [R.SECP256K1, R.P256]
ERR_INVERSE_OF_ZERO, ERR_POINT_AT_INFINITY = 4, 64
PLAN_AUTO, PLAN_LANE, PLAN_QUAD = 0, 1, 2
NTHREADS = 16
_CHUNK = 1024           # elements per oracle call: 16 797 columns x 8 bytes each


def edges(cv):
    """input set E of one curve (raw 256-bit values; the last four are n, n + 1, 2^256 - 1 -- reduced, not flagged -- and 0)"""
    n = cv.n
    e = [d << (4 * j) for j in range(64) for d in range(1, 16)]                  # every table entry; three empty quad groups
    e += [1, 2, n - 1, n - 2, (n - 1) // 2, (1 << 255) % n]
    rng = R.SplitMix64(0xE0 + (cv.name == "p256"))

    def groups():                                                                # four non-zero 64-bit groups, value < 2^254 < n
        g = [rng.next() | 1 for _ in range(4)]
        g[3] = (g[3] >> 2) | 1
        return g

    for j in range(4):                                                           # exactly one non-empty 16-window group
        e.append(groups()[j] << (64 * j))
    for j in range(4):                                                           # exactly one empty group
        g = groups()
        g[j] = 0
        e.append(sum(v << (64 * i) for i, v in enumerate(g)))
    e += [n, n + 1, (1 << 256) - 1, 0]
    return e


def group_patterns(cv, seed=0x6707):
    """33 raw scalars: for each of the 16 empty / non-empty patterns of the four 64-bit groups (bit j of the index: group j is
    not empty; the six with exactly two empty groups are those where one level of the quad plan's tree adds and the other
    only selects) two values below 2^254 < n, pattern by pattern; then one more of pattern 1111 so that the batch ends in a
    lone quad"""
    rng = R.SplitMix64(seed + (cv.name == "p256"))
    out = []
    for mask in list(range(16)) * 2 + [15]:
        g = [(rng.next() | 1) if (mask >> j) & 1 else 0 for j in range(4)]
        g[3] = (g[3] >> 2) | ((mask >> 3) & 1)
        out.append(sum(v << (64 * j) for j, v in enumerate(g)))
    return out


def group_mask(v):
    return sum(1 << j for j in range(4) if (v >> (64 * j)) & ((1 << 64) - 1))


def batch(cv, total, seed, shift=0):
    """E (rotated by `shift`) at the start, random filler, E reversed at the end: `total` raw 256-bit values"""
    e = edges(cv)
    e = e[shift:] + e[:shift]
    rng = R.SplitMix64(seed)
    assert total >= 2 * len(e)
    fill = [rng.below(1 << 256) for _ in range(total - 2 * len(e))]
    return e + fill + e[::-1]


def pack(vals):
    return oracle_c.pack256(vals)


def unpack(arr):
    return oracle_c.unpack256(np.asarray(arr))


_points = [{}, {}]       # per curve: reduced scalar -> affine k G (None for 0), shared by every test of a session


def _limb_value(cols, row0):
    acc = np.zeros(cols.shape[1], dtype=object)
    for j in range(9):
        acc = acc + (cols[row0 + j].astype(object) << (29 * j))
    return acc


def base_points(curve_id, scalars):
    """{k: affine k G} for reduced scalars, through the C oracle (see the module docstring)"""
    cv = CURVES[curve_id]
    known = _points[curve_id]
    todo = sorted({int(k) for k in scalars} - set(known))
    for a in range(0, len(todo), _CHUNK):
        ks = todo[a:a + _CHUNK]
        cols, _aux, err, _flags = oracle_c.curve_fixed_base(curve_id, cv.g, pack(ks), nthreads=NTHREADS, lockstep=64, want_aux=False)
        end = cols.shape[0]
        xs, ys = _limb_value(cols, end - 10 - 51 - 10 - 10), _limb_value(cols, end - 10)
        for i, k in enumerate(ks):
            if err[i]:                      # the circuit panics here (k = 0 among them): the big-int value instead
                known[k] = cv.mul(k, cv.g)
            else:
                known[k] = (int(xs[i]), int(ys[i]))
    return known


def expect_keys(curve_id, sk):
    """sk: raw ints -> (pkx, pky) as (n, 32) bytes (zeros where flagged), err bytes"""
    cv = CURVES[curve_id]
    red = [v % cv.n for v in sk]
    pts = base_points(curve_id, red)
    err = np.array([ERR_POINT_AT_INFINITY if v == 0 else 0 for v in red], np.uint8)
    return (pack([0 if v == 0 else pts[v][0] for v in red]), pack([0 if v == 0 else pts[v][1] for v in red]), err)


def expect_sigs(curve_id, msg, sk, k):
    """raw ints -> (r, s) as (n, 32) bytes (zeros where flagged), err bytes"""
    cv = CURVES[curve_id]
    n = cv.n
    pts = base_points(curve_id, [v % n for v in k])
    rs, ss, err = [], [], []
    for m, d, kk in zip(msg, sk, k):
        m, d, kk = m % n, d % n, kk % n
        if kk == 0:
            rs.append(0), ss.append(0), err.append(ERR_INVERSE_OF_ZERO)
            continue
        r = pts[kk][0] % n
        rs.append(r), ss.append(pow(kk, -1, n) * (m + r * d) % n), err.append(0)
    return pack(rs), pack(ss), np.array(err, np.uint8)


def replay_synth(curve_id, seed, count):
    """(sk, msg, k) of the first `count` signatures of p2e_synth_signatures[_curve](seed, ...): the splitmix stream of
    csrc/consts.hpp synth_signature, first draw (a redraw happens only for r = 0 or s = 0; the caller checks msg)"""
    cv = CURVES[curve_id]
    out = []
    for i in range(count):
        rng = R.SplitMix64((seed ^ (0x9E3779B97F4A7C15 * (i + 1))) & ((1 << 64) - 1))
        out.append((rng.below(cv.n), rng.below(cv.n), rng.below(cv.n)))
    return [v[0] for v in out], [v[1] for v in out], [v[2] for v in out]
