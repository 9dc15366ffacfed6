"""Inputs and independent expectations of the wire-form tests (test_wire_cpu.py, test_gpu_wire.py): SEC1 keys, strict DER
and compact signatures on both curves (include/p2e.h p2e_point_decode_batch and the three calls after it).

Everything expected is computed with Python integers from the header's rules and nothing the code under test provides:
the square root is pow(t, (p + 1) // 4, p), the DER parser is written from the six rules, the encoders from SEC1 2.3.3
and X.690's minimal INTEGER.  Every element has an exact expected code and exact expected bytes: nothing is left out.

A main batch has N_MAIN = 4161 elements (65 full waves and one lane): the edge set cycled and shuffled with a fixed seed,
then the valid material (300 keys of the signing tests' batch in both forms; 300 signatures and their low-s twins).  The
expectations are taken from the bytes each element really has in the finished buffer."""
import functools

import numpy as np

import p2e_ref as R
import sign_inputs as S

CURVES = [R.SECP256K1, R.P256]
N_MAIN = 4161
N_VALID = 300
(OK, BAD_LENGTH, BAD_PREFIX, COORD_RANGE, NOT_ON_CURVE, INFINITY, DER_SYNTAX, DER_INTEGER, SCALAR_RANGE, HIGH_S) = range(10)
SEC1_COMPRESSED, SEC1_UNCOMPRESSED = 0, 1
SIG_DER, SIG_COMPACT64, SIG_COMPACT65 = 0, 1, 2
REQUIRE_LOW_S, NORMALIZE_S = 1, 2
DECODE_FLAGS = (0, REQUIRE_LOW_S, NORMALIZE_S)
ENCODE_FLAGS = (0, NORMALIZE_S)
DER_STRIDE = 72
POINT_STRIDE = {SEC1_COMPRESSED: 33, SEC1_UNCOMPRESSED: 65}
SIG_STRIDE = {SIG_DER: DER_STRIDE, SIG_COMPACT64: 64, SIG_COMPACT65: 65}
M256 = (1 << 256) - 1
REVERSED = None            # an element whose offsets run backwards by one byte

# SEC 2 (v2) 2.4.1 and 2.4.2: the generators as published, compressed and uncompressed
SEC2_G = [
    ("0279BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798",
     "0479BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8"),
    ("036B17D1F2E12C4247F8BCE6E563A440F277037D812DEB33A0F4A13945D898C296",
     "046B17D1F2E12C4247F8BCE6E563A440F277037D812DEB33A0F4A13945D898C2964FE342E2FE1A7F9B8EE7EB4A7C0F9E162BCE33576B315ECECBB6406837BF51F5"),
]


def be(v):
    return int(v).to_bytes(32, "big")


def pack(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), np.uint8).reshape(-1, 32).copy()


def unpack(arr):
    return [int.from_bytes(bytes(row), "little") for row in np.asarray(arr)]


# ---- the rules, in Python integers ----------------------------------------------------------------------------------
def cubic(cv, x):
    return (x * x * x + cv.a * x + cv.b) % cv.p


def lift_x(cv, x, odd):
    """the y of parity `odd` with y^2 = x^3 + a x + b, or None (both primes are 3 mod 4)"""
    t = cubic(cv, x)
    y = pow(t, (cv.p + 1) // 4, cv.p)
    if y * y % cv.p != t:
        return None
    return y if (y & 1) == odd else cv.p - y


def decode_point(cv, b):
    """-> (code, x, y)"""
    if len(b) not in (1, 33, 65):
        return BAD_LENGTH, 0, 0
    if len(b) == 1:
        return (INFINITY if b[0] == 0 else BAD_PREFIX), 0, 0
    if (len(b) == 33 and b[0] not in (2, 3)) or (len(b) == 65 and b[0] != 4):
        return BAD_PREFIX, 0, 0
    x = int.from_bytes(b[1:33], "big")
    y = int.from_bytes(b[33:65], "big") if len(b) == 65 else 0
    if x >= cv.p or y >= cv.p:
        return COORD_RANGE, 0, 0
    if len(b) == 33:
        y = lift_x(cv, x, b[0] & 1)
        return (NOT_ON_CURVE, 0, 0) if y is None else (OK, x, y)
    return (OK, x, y) if y * y % cv.p == cubic(cv, x) else (NOT_ON_CURVE, 0, 0)


def encode_point(cv, form, x, y):
    """-> (code, stride bytes)"""
    zeros = bytes(POINT_STRIDE[form])
    if x == 0 and y == 0:
        return INFINITY, zeros
    if x >= cv.p or y >= cv.p:
        return COORD_RANGE, zeros
    if y * y % cv.p != cubic(cv, x):
        return NOT_ON_CURVE, zeros
    return OK, (bytes([2 | (y & 1)]) + be(x)) if form == SEC1_COMPRESSED else (b"\x04" + be(x) + be(y))


def _low_s(cv, flags, s, v):
    """after the range checks: -> (code, s, v)"""
    if s > (cv.n - 1) // 2:
        if flags == REQUIRE_LOW_S:
            return HIGH_S, 0, 0
        if flags == NORMALIZE_S:
            return OK, cv.n - s, v ^ 1
    return OK, s, v


def parse_der(cv, b, flags=0):
    """strict DER, BIP-66's rules, the six checks of include/p2e.h in order -> (code, r, s)"""
    L = len(b)
    if L < 8 or L > 72:
        return BAD_LENGTH, 0, 0
    if b[0] != 0x30 or b[1] != L - 2:
        return DER_SYNTAX, 0, 0
    lr = b[3]
    if b[2] != 0x02 or lr == 0 or lr > 33 or lr + 7 > L:
        return DER_SYNTAX, 0, 0
    ls = b[5 + lr]
    if b[4 + lr] != 0x02 or ls == 0 or ls > 33 or lr + ls + 6 != L:
        return DER_SYNTAX, 0, 0
    rb, sb = b[4:4 + lr], b[6 + lr:6 + lr + ls]
    for i in (rb, sb):
        if i[0] >= 0x80 or (len(i) > 1 and i[0] == 0 and i[1] < 0x80):
            return DER_INTEGER, 0, 0
    r, s = int.from_bytes(rb, "big"), int.from_bytes(sb, "big")
    for v in (r, s):
        if v >> 256 or v == 0 or v >= cv.n:
            return SCALAR_RANGE, 0, 0
    code, s, _ = _low_s(cv, flags, s, 0)
    return (code, r, s) if code == OK else (code, 0, 0)


def decode_compact(cv, form, b, flags=0):
    """-> (code, r, s, v); v = 0 in COMPACT64"""
    r, s = int.from_bytes(b[:32], "big"), int.from_bytes(b[32:64], "big")
    v = b[64] if form == SIG_COMPACT65 else 0
    if r == 0 or r >= cv.n or s == 0 or s >= cv.n:
        return SCALAR_RANGE, 0, 0, 0
    code, s, v = _low_s(cv, flags, s, v)
    return (code, r, s, v) if code == OK else (code, 0, 0, 0)


def der_int(v):
    b = int(v).to_bytes((int(v).bit_length() + 7) // 8 or 1, "big")
    return (b"\x00" + b) if b[0] & 0x80 else b


def der_raw(rb, sb):
    """30 len 02 lr rb 02 ls sb with whatever bytes the caller gives as integers"""
    body = bytes([2, len(rb) & 0xFF]) + rb + bytes([2, len(sb) & 0xFF]) + sb
    return bytes([0x30, len(body) & 0xFF]) + body


def der(r, s):
    return der_raw(der_int(r), der_int(s))


def encode_sig(cv, form, flags, r, s, v):
    """-> (code, stride bytes, out_len (DER; 0 otherwise))"""
    if r == 0 or r >= cv.n or s == 0 or s >= cv.n:
        return SCALAR_RANGE, bytes(SIG_STRIDE[form]), 0
    if flags == NORMALIZE_S and s > (cv.n - 1) // 2:
        s, v = cv.n - s, v ^ 1
    if form == SIG_DER:
        d = der(r, s)
        return OK, d + bytes(DER_STRIDE - len(d)), len(d)
    return OK, be(r) + be(s) + (bytes([v]) if form == SIG_COMPACT65 else b""), 0


# ---- material ----------------------------------------------------------------------------------------------------------
def _jac_mul(cv, k, pt):
    """k pt with Jacobian coordinates in Python integers (one inversion): the keys of the valid material"""
    p, a = cv.p, cv.a

    def dbl(P):
        X, Y, Z = P
        if not Y:
            return (0, 1, 0)
        S_, M = 4 * X * Y * Y % p, (3 * X * X + a * pow(Z, 4, p)) % p
        X3 = (M * M - 2 * S_) % p
        return X3, (M * (S_ - X3) - 8 * pow(Y, 4, p)) % p, 2 * Y * Z % p

    def add(P, Q):
        if not P[2]:
            return Q
        if not Q[2]:
            return P
        Z1Z1, Z2Z2 = P[2] * P[2] % p, Q[2] * Q[2] % p
        U1, U2 = P[0] * Z2Z2 % p, Q[0] * Z1Z1 % p
        S1, S2 = P[1] * Z2Z2 * Q[2] % p, Q[1] * Z1Z1 * P[2] % p
        if U1 == U2:
            return dbl(P) if S1 == S2 else (0, 1, 0)
        H, Rr = (U2 - U1) % p, (S2 - S1) % p
        H2 = H * H % p
        H3, V = H * H2 % p, U1 * H2 % p
        X3 = (Rr * Rr - H3 - 2 * V) % p
        return X3, (Rr * (V - X3) - S1 * H3) % p, H * P[2] * Q[2] % p

    acc, base = (0, 1, 0), (pt[0], pt[1], 1)
    while k:
        if k & 1:
            acc = add(acc, base)
        base = dbl(base)
        k >>= 1
    zi = pow(acc[2], -1, p)
    return acc[0] * zi * zi % p, acc[1] * zi * zi * zi % p


@functools.lru_cache(maxsize=None)
def valid_keys(curve_id):
    """(sk, (x, y)) of the first N_VALID secret keys of the signing tests' batch that are not 0 mod n"""
    cv = CURVES[curve_id]
    sks = [v % cv.n for v in S.batch(cv, 2048, 0x51 + curve_id, shift=1) if v % cv.n][:N_VALID]
    pts = [_jac_mul(cv, k, cv.g) for k in sks]
    assert all(cv.on_curve(q) for q in pts) and _jac_mul(cv, 5, cv.g) == cv.mul(5, cv.g) and pts[0] == cv.mul(sks[0], cv.g)
    return sks, pts


@functools.lru_cache(maxsize=None)
def valid_sigs(curve_id):
    """N_VALID signatures (msg, r, s, v, key index): the nonce of signature i is the secret key i + 1 of valid_keys, so that
    R is a point already known; about half have a high s"""
    cv = CURVES[curve_id]
    sks, pts = valid_keys(curve_id)
    rng = R.SplitMix64(0x51C + curve_id)
    out = []
    for i in range(N_VALID):
        k, Rp = sks[(i + 1) % N_VALID], pts[(i + 1) % N_VALID]
        msg = rng.below(cv.n)
        r = Rp[0] % cv.n
        s = pow(k, -1, cv.n) * (msg + r * sks[i]) % cv.n
        assert r and s
        out.append((msg, r, s, (Rp[1] & 1) | (2 if Rp[0] >= cv.n else 0), i))
    return out


def non_residue_x(cv):
    """the smallest x >= 1 whose cubic is not a square: found by search"""
    x = 1
    while lift_x(cv, x, 0) is not None:
        x += 1
    return x


def _rand_bytes(rng, n):
    return bytes(rng.next() & 0xFF for _ in range(n))


def key_edges(curve_id):
    """list of units; a unit is a list of elements (bytes, or REVERSED) that stay adjacent"""
    cv = CURVES[curve_id]
    p = cv.p
    gx, gy = cv.g
    rng = R.SplitMix64(0xED6E + curve_id)
    comp = lambda pre, x: bytes([pre]) + be(x)
    unc = lambda pre, x, y: bytes([pre]) + be(x) + be(y)
    e = [comp(2 | (gy & 1), gx), unc(4, gx, gy)]                                   # G in both forms
    e += [comp(2, gx), comp(3, gx)]                                                # both parities
    nx = non_residue_x(cv)
    e += [comp(2, nx), comp(3, nx), unc(4, nx, 1)]
    for x in (0, 1, p - 1, p, M256):
        y = lift_x(cv, x % p, 0)
        e += [comp(2, x), comp(3, x), unc(4, x, 1 if y is None else y)]
    e += [unc(4, gx, gy + 1), unc(4, gx, p - gy), unc(4, gx, p), unc(4, gx, M256), unc(4, 0, 0)]
    for pre in (0, 1, 2, 3, 4, 5, 6, 7, 0xFF):                                     # every prefix at both lengths
        e += [comp(pre, gx), unc(pre, gx, gy)]
    e += [b"", b"\x00", b"\x02", b"\x04"]
    e += [comp(2, gx)[:32], comp(2, gx) + b"\x01", unc(4, gx, gy)[:64], unc(4, gx, gy) + b"\x01"]       # 32, 34, 64, 66
    units = [[x] for x in e]
    units.append([_rand_bytes(rng, 1000)])
    units.append([_rand_bytes(rng, 1000), REVERSED])                              # the next element begins one byte early
    return units


def _int_of_len(rng, n):
    """a valid minimal positive DER integer of exactly n bytes (n = 33: 00 and a value with its top bit set, below both orders)"""
    if n == 33:
        return b"\x00" + bytes([0x80 | rng.next() % 0x70]) + _rand_bytes(rng, 31)
    return bytes([1 + rng.next() % 0x7F]) + _rand_bytes(rng, n - 1)


def sig_values(curve_id):
    """(r, s) pairs of the value edges: the compact forms carry these as they are"""
    n = CURVES[curve_id].n
    vals = [1, n - 1, n, M256]
    pairs = [(r, s) for r in vals for s in vals]
    pairs += [(0, 1), (1, 0), (0, 0), (5, (n - 1) // 2), (5, (n + 1) // 2), ((n + 1) // 2, (n - 1) // 2), (n + 1, 5), (5, n + 1)]
    return pairs


def der_edges(curve_id):
    cv = CURVES[curve_id]
    n = cv.n
    rng = R.SplitMix64(0xDE2 + curve_id)
    e = []
    for lr in (1, 2, 31, 32, 33):
        for ls in (1, 2, 31, 32, 33):
            e.append(der_raw(_int_of_len(rng, lr), _int_of_len(rng, ls)))
    i33 = lambda v: int(v).to_bytes(33, "big")
    enc = lambda v: i33(v) if v == M256 else der_int(v)
    for r, s in sig_values(curve_id):
        e.append(der_raw(enc(r), enc(s)))                                          # 0 is 02 01 00
    e.append(der_raw((1 << 256).to_bytes(33, "big"), b"\x05"))                      # 33 bytes, first byte 01: >= 2^256
    good = _int_of_len(rng, 32)
    neg = bytes([0x80 | rng.next() % 0x80]) + _rand_bytes(rng, 31)
    for bad in (neg, b"\x80", b"\xff", b"\x00\x00" + _rand_bytes(rng, 30), b"\x00\x7f" + _rand_bytes(rng, 30), b"\x00\x00", b"\x00\x01"):
        e += [der_raw(bad, good), der_raw(good, bad)]
    e.append(der_raw(b"\x00", neg))                                                # r = 0 and a negative s: the integer rule first
    ok = der_raw(good, _int_of_len(rng, 32))
    e.append(b"\x30\x81" + bytes([len(ok) - 2]) + ok[2:])                          # long-form length
    lr = ok[3]
    for tag in (0x31, 0x03):
        for at in (0, 2, 4 + lr):
            e.append(ok[:at] + bytes([tag]) + ok[at + 1:])
    e += [ok[:1] + bytes([ok[1] + 1]) + ok[2:], ok[:1] + bytes([ok[1] - 1]) + ok[2:]]
    e += [ok + b"\x01", ok[:1] + bytes([ok[1] + 1]) + ok[2:] + b"\x01"]             # a trailing byte, b[1] as it was and adjusted
    e.append(ok[:3] + b"\x00" + ok[4:])                                            # lr = 0
    e += [ok[:3] + bytes([len(ok) - 6]) + ok[4:], ok[:3] + b"\x21" + ok[4:12], ok[:3] + b"\x40" + ok[4:]]       # lr past the end
    e += [der_raw(b"\x00" + _int_of_len(rng, 33), b"\x05"), der_raw(b"\x05", b"\x00" + _int_of_len(rng, 33))]   # 34-byte integers
    e += [b"", _rand_bytes(rng, 7), der_raw(b"\x01", b"\x01"), der_raw(_int_of_len(rng, 33), _int_of_len(rng, 33)),
          der_raw(_int_of_len(rng, 33), _int_of_len(rng, 33)) + b"\x00"]             # 0, 7, 8, 72, 73
    assert [len(x) for x in e[-5:]] == [0, 7, 8, 72, 73]
    units = [[x] for x in e]
    units.append([_rand_bytes(rng, 1000)])
    units.append([_rand_bytes(rng, 1000), REVERSED])
    return units


def _assemble(units, tail, seed):
    """the edge units cycled up to N_MAIN - len(tail) elements and shuffled, then `tail`
    -> (data uint8, offsets uint64 (N_MAIN + 1), [the bytes each element really has])"""
    rng = np.random.default_rng(seed)
    room = N_MAIN - len(tail)
    picked, count, j = [], 0, 0
    while count + len(units[j % len(units)]) <= room:
        picked.append(units[j % len(units)])
        count += len(picked[-1])
        j += 1
    picked += [[b"\x00"]] * (room - count)
    assert j >= 2 * len(units)                                   # every edge at least twice
    order = rng.permutation(len(picked))
    elems = [x for k in order for x in picked[k]] + list(tail)
    assert len(elems) == N_MAIN
    buf, offsets, pos = bytearray(), [0], 0
    for x in elems:
        if x is REVERSED:
            pos -= 1
        else:
            buf[pos:] = x                                        # (behind a reversed element: over the last byte before it)
            pos += len(x)
        offsets.append(pos)
    data = np.frombuffer(bytes(buf) + b"\x00", np.uint8).copy()
    raw = bytes(buf)
    real = [raw[a:b] if b >= a else b"" for a, b in zip(offsets[:-1], offsets[1:])]
    assert sum(1 for a, b in zip(offsets[:-1], offsets[1:]) if b < a) >= 2
    return data, np.array(offsets, np.uint64), real


@functools.lru_cache(maxsize=None)
def key_batch(curve_id):
    """(data, offsets, elements, want_x (N, 32), want_y (N, 32), want_err (N,))"""
    cv = CURVES[curve_id]
    _, pts = valid_keys(curve_id)
    tail = [bytes([2 | (y & 1)]) + be(x) for x, y in pts] + [b"\x04" + be(x) + be(y) for x, y in pts]
    data, offsets, real = _assemble(key_edges(curve_id), tail, 0x5EC1 + curve_id)
    want = [decode_point(cv, b) for b in real]
    assert {w[0] for w in want} == {OK, BAD_LENGTH, BAD_PREFIX, COORD_RANGE, NOT_ON_CURVE, INFINITY}
    return data, offsets, real, pack([w[1] for w in want]), pack([w[2] for w in want]), np.array([w[0] for w in want], np.uint8)


@functools.lru_cache(maxsize=None)
def der_batch(curve_id):
    """(data, offsets, elements); expectations per flag value from der_want"""
    cv = CURVES[curve_id]
    sigs = valid_sigs(curve_id)
    tail = [der(r, s) for _m, r, s, _v, _i in sigs] + [der(r, min(s, cv.n - s)) for _m, r, s, _v, _i in sigs]
    return _assemble(der_edges(curve_id), tail, 0xDE5 + curve_id)


@functools.lru_cache(maxsize=None)
def der_want(curve_id, flags):
    """(want_r (N, 32), want_s (N, 32), want_err (N,))"""
    cv = CURVES[curve_id]
    want = [parse_der(cv, b, flags) for b in der_batch(curve_id)[2]]
    codes = {w[0] for w in want}
    assert codes >= {OK, BAD_LENGTH, DER_SYNTAX, DER_INTEGER, SCALAR_RANGE} and (HIGH_S in codes) == (flags == REQUIRE_LOW_S)
    return pack([w[1] for w in want]), pack([w[2] for w in want]), np.array([w[0] for w in want], np.uint8)


@functools.lru_cache(maxsize=None)
def compact_values(curve_id):
    """N_MAIN (r, s, v): the value edges cycled and shuffled, then the valid signatures and their low-s twins"""
    cv = CURVES[curve_id]
    sigs = valid_sigs(curve_id)
    tail = [(r, s, v) for _m, r, s, v, _i in sigs]
    tail += [(r, cv.n - s, v ^ 1) if s > (cv.n - 1) // 2 else (r, s, v) for _m, r, s, v, _i in sigs]
    edge = sig_values(curve_id)
    vs = (0, 1, 2, 3, 27, 255)
    head = [edge[i % len(edge)] + (vs[i % len(vs)],) for i in range(N_MAIN - len(tail))]     # 24 pairs x 6: every pair meets every v
    order = np.random.default_rng(0xC0A + curve_id).permutation(len(head))
    return [head[k] for k in order] + tail


@functools.lru_cache(maxsize=None)
def compact_batch(curve_id, form):
    """(N_MAIN, 64 | 65) uint8"""
    rows = [be(r) + be(s) + (bytes([v]) if form == SIG_COMPACT65 else b"") for r, s, v in compact_values(curve_id)]
    return np.frombuffer(b"".join(rows), np.uint8).reshape(N_MAIN, SIG_STRIDE[form]).copy()


@functools.lru_cache(maxsize=None)
def compact_want(curve_id, form, flags):
    """(want_r, want_s, want_v (N,), want_err (N,))"""
    cv = CURVES[curve_id]
    want = [decode_compact(cv, form, bytes(row), flags) for row in compact_batch(curve_id, form)]
    return (pack([w[1] for w in want]), pack([w[2] for w in want]), np.array([w[3] for w in want], np.uint8),
            np.array([w[0] for w in want], np.uint8))


@functools.lru_cache(maxsize=None)
def point_values(curve_id):
    """N_MAIN (x, y) for the key encoder: the valid keys and the generator; zero, >= p and off-curve values"""
    cv = CURVES[curve_id]
    p = cv.p
    gx, gy = cv.g
    _, pts = valid_keys(curve_id)
    edge = [(gx, gy), (gx, p - gy), (0, 0), (0, 1), (1, 0), (p, gy), (gx, p), (M256, gy), (gx, M256), (gx + p if gx + p <= M256 else p, gy),
            (gx, gy + 1), (gx + 1, gy), (gy, gx), (p - 1, 1), (p, p), (M256, M256)]
    for x in (0, 1, p - 1):
        y = lift_x(cv, x, 1)
        if y is not None:
            edge.append((x, y))
    head = [edge[i % len(edge)] for i in range(N_MAIN - len(pts))]
    order = np.random.default_rng(0xE2C + curve_id).permutation(len(head))
    return [head[k] for k in order] + pts


@functools.lru_cache(maxsize=None)
def point_encode_want(curve_id, form):
    """(want_out (N, stride), want_err (N,))"""
    cv = CURVES[curve_id]
    want = [encode_point(cv, form, x, y) for x, y in point_values(curve_id)]
    assert {w[0] for w in want} == {OK, INFINITY, COORD_RANGE, NOT_ON_CURVE}
    return (np.frombuffer(b"".join(w[1] for w in want), np.uint8).reshape(N_MAIN, POINT_STRIDE[form]).copy(),
            np.array([w[0] for w in want], np.uint8))


@functools.lru_cache(maxsize=None)
def sig_encode_want(curve_id, form, flags):
    """the encoder over compact_values: (want_out (N, stride), want_len (N,), want_err (N,))"""
    cv = CURVES[curve_id]
    want = [encode_sig(cv, form, flags, r, s, v) for r, s, v in compact_values(curve_id)]
    assert {w[0] for w in want} == {OK, SCALAR_RANGE}
    return (np.frombuffer(b"".join(w[1] for w in want), np.uint8).reshape(N_MAIN, SIG_STRIDE[form]).copy(),
            np.array([w[2] for w in want], np.uint8), np.array([w[0] for w in want], np.uint8))
