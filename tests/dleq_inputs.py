"""The oracle and the input sets of the DLEQ tests (test_dleq_cpu.py, test_gpu_dleq.py): include/p2e.h p2e_dleq_prove_batch and
p2e_dleq_verify_batch restated in Python integers and hashlib on schnorr_inputs.py's curve helpers.  Nothing here uses the code
under test.

There are no published vectors here (the definition of include/p2e.h is the specification, and it has not been checked against
the vectors of BIP-374).  The oracle is pinned by test_dleq_cpu.py: (a) every proof it makes it accepts, (b) every B of the sets
is b G for a b this file knows, so R2 = s B - e C must equal (k b) G and C must equal (a b) G -- different multiplications that
agree only if all are right --, (c) the three midstates from hashlib, (d) the rejections.

Sets of 257 elements (one block and a lane), with and without a message.  The special elements sit at fixed places, most of
them in the first wave among good lanes."""
import functools
import hashlib

import numpy as np

import schnorr_inputs as SI

P, N, G = SI.P, SI.N, SI.G
TAGS = ("BIP0374/aux", "BIP0374/nonce", "BIP0374/challenge")
WIRE_OK, WIRE_COORD_RANGE, WIRE_NOT_ON_CURVE, WIRE_INFINITY, WIRE_SCALAR_RANGE = 0, 3, 4, 5, 8
N_SET = 257
SIZES = (0, 1, 63, 64, 65, 257)
O = (0, 0)
b32 = SI.b32
tag_midstate = SI.tag_midstate


# ---- the curve on affine points (None: the neutral element) -----------------------------------------------------------------------
def mul(k, pt):
    k %= N
    return None if k == 0 or pt is None else SI._affine(SI._jmul(k, pt))


def add(p, q):
    j = lambda a: None if a is None else (a[0], a[1], 1)
    return SI._affine(SI._jadd(j(p), j(q)))


def neg(pt):
    return None if pt is None else (pt[0], (P - pt[1]) % P)


def on_curve(pt):
    return (pt[1] * pt[1] - pt[0] ** 3 - 7) % P == 0


def point_code(pt):
    """a point that must not be neutral: (0, 0), then the range, then the curve"""
    if pt == O:
        return WIRE_INFINITY
    if pt[0] >= P or pt[1] >= P:
        return WIRE_COORD_RANGE
    return WIRE_OK if on_curve(pt) else WIRE_NOT_ON_CURVE


def cbytes(pt):
    return bytes([2 | (pt[1] & 1)]) + b32(pt[0])


# ---- the definition -------------------------------------------------------------------------------------------------------------
def nonce(a, aux, A, C, msg):
    t = bytes(x ^ y for x, y in zip(b32(a), SI.tagged_hash(TAGS[0], aux)))
    return int.from_bytes(SI.tagged_hash(TAGS[1], t + cbytes(A) + cbytes(C) + (msg or b"")), "big") % N


def challenge(A, B, C, R1, R2, msg):
    data = cbytes(A) + cbytes(B) + cbytes(C) + cbytes(G) + cbytes(R1) + cbytes(R2) + (msg or b"")
    return int.from_bytes(SI.tagged_hash(TAGS[2], data), "big")


def response(k, e, a):
    return (k + e * a) % N


def prove_with_nonce(a, A, B, C, k, msg):
    """(code, proof64) behind the nonce hash, for any k"""
    if k % N == 0:
        return WIRE_INFINITY, bytes(64)
    R1, R2 = SI.base_mul(k), mul(k, B)
    e = challenge(A, B, C, R1, R2, msg)
    return WIRE_OK, b32(e) + b32(response(k, e, a))


def prove(a, B, aux, msg):
    """(code, proof64, C as a wire point)"""
    code = WIRE_SCALAR_RANGE if a == 0 or a >= N else point_code(B)
    if code:
        return code, bytes(64), O
    A, C = SI.base_mul(a), mul(a, B)
    code, proof = prove_with_nonce(a, A, B, C, nonce(a, aux, A, C, msg), msg)
    return code, proof, (O if code else C)


def verify_points(A, B, C, e, s):
    """(R1, R2) = (s G - e A, s B - e C) behind the challenge, for any e; None where either is neutral"""
    R1 = add(SI.base_mul(s) if s % N else None, neg(mul(e, A)))
    R2 = add(mul(s, B), neg(mul(e, C)))
    return None if R1 is None or R2 is None else (R1, R2)


def verify(A, B, C, proof, msg):
    """(code, valid)"""
    code = point_code(A) or point_code(B) or point_code(C)
    e, s = int.from_bytes(proof[:32], "big"), int.from_bytes(proof[32:], "big")
    if not code and s >= N:
        code = WIRE_SCALAR_RANGE
    if code:
        return code, 0
    r = verify_points(A, B, C, e, s)
    return WIRE_OK, int(r is not None and challenge(A, B, C, r[0], r[1], msg) == e)


# ---- the sets --------------------------------------------------------------------------------------------------------------------
def _rand(label, i, mod=None):
    v = int.from_bytes(hashlib.sha256(b"dleq-inputs/%s/%d" % (label.encode(), i)).digest(), "big")
    return v if mod is None else 1 + v % (mod - 1)


def _off_curve():
    return (G[0], G[1] + 1)


def _x_ge_p():
    x = next(x for x in range(1, 100) if SI.lift_x(x) is not None)      # x + p < 2^256 names a curve point modulo p only
    return (x + P, SI.lift_x(x)[1])


# place -> (what, value): the prover's special elements; every other element is a random (a, b)
PROVER_SPECIALS = {1: ("a", 1), 2: ("a", 0), 4: ("a", 2), 5: ("B", "neutral"), 7: ("a", N - 1), 9: ("B", "off_curve"), 11: ("a", N),
                   13: ("B", "x_ge_p"), 17: ("b", 1), 19: ("b", N - 1), 23: ("a0_and_bad_B", None), 63: ("a", 0), 64: ("B", "neutral"),
                   65: ("a", N), 200: ("B", "off_curve"), 256: ("b", 1)}
BAD_POINTS = {"neutral": (lambda: O, WIRE_INFINITY), "off_curve": (_off_curve, WIRE_NOT_ON_CURVE), "x_ge_p": (_x_ge_p, WIRE_COORD_RANGE)}


@functools.lru_cache(maxsize=None)
def prover_set(with_msg):
    """list of dicts a, b (None where B is no multiple this file knows), B, aux, msg, code, proof, C"""
    out = []
    for i in range(N_SET):
        a, b = _rand("a", i, N), _rand("b", i, N)
        what, val = PROVER_SPECIALS.get(i, (None, None))
        if what == "a":
            a = val
        elif what == "b":
            b = val
        B = SI.base_mul(b)
        if what == "B":
            B, b = BAD_POINTS[val][0](), None
        elif what == "a0_and_bad_B":
            a, B, b = 0, _off_curve(), None
        aux = hashlib.sha256(b"dleq-inputs/aux/%d" % i).digest()
        msg = hashlib.sha256(b"dleq-inputs/msg/%d" % i).digest() if with_msg else None
        code, proof, C = prove(a, B, aux, msg)
        out.append(dict(a=a, b=b, B=B, aux=aux, msg=msg, code=code, proof=proof, C=C))
    return out


def _flip(data, bit):
    d = bytearray(data)
    d[bit // 8] ^= 1 << (bit % 8)
    return bytes(d)


# place -> kind: the verifier's special elements, made from the prover's good element at the same place
VERIFIER_SPECIALS = {0: "flip_e", 3: "A_neutral", 6: "B_off_curve", 8: "C_x_ge_p", 10: "s_eq_n", 12: "A_off_curve_B_neutral", 14: "s_zero",
                     15: "e_zero", 16: "e_ge_n", 18: "flip_s", 20: "C_plus_G", 21: "swap_A_C", 22: "B_neutral_C_off_curve", 24: "A_x_ge_p",
                     25: "B_x_ge_p", 26: "C_neutral", 27: "C_off_curve", 28: "B_neutral", 29: "s_max", 62: "flip_s", 66: "A_neutral",
                     130: "flip_e", 255: "s_eq_n"}


@functools.lru_cache(maxsize=None)
def verifier_set(with_msg):
    """list of dicts A, B, C, proof, msg, code, valid, kind: the prover's set with its codes cleared away (a flagged prover
    element becomes a fresh good one), then the special elements"""
    out = []
    for i, p in enumerate(prover_set(with_msg)):
        a, b, aux, msg = p["a"], p["b"], p["aux"], p["msg"]
        if p["code"]:
            a, b = _rand("va", i, N), _rand("vb", i, N)
        B = SI.base_mul(b)
        code, proof, C = prove(a, B, aux, msg)
        assert code == 0
        A = SI.base_mul(a)
        kind = VERIFIER_SPECIALS.get(i, "good")
        e, s = proof[:32], proof[32:]
        bad = lambda name: BAD_POINTS[name][0]()
        if kind == "flip_e":
            proof = _flip(proof, (37 * i) % 256)
        elif kind == "flip_s":
            proof = _flip(proof, 256 + (41 * i) % 256)        # (`verify` decides the code: s >= n would be a flag, not a rejection)
        elif kind == "s_eq_n":
            proof = e + b32(N)
        elif kind == "s_max":
            proof = e + b"\xff" * 32
        elif kind == "s_zero":
            proof = e + bytes(32)
        elif kind == "e_zero":
            proof = bytes(32) + s
        elif kind == "e_ge_n":
            proof = b32(N + 1 + i) + s
        elif kind == "C_plus_G":
            C = add(C, G)
        elif kind == "swap_A_C":
            A, C = C, A
        elif kind == "A_neutral":
            A = bad("neutral")
        elif kind == "A_x_ge_p":
            A = bad("x_ge_p")
        elif kind == "A_off_curve_B_neutral":
            A, B = bad("off_curve"), bad("neutral")
        elif kind == "B_off_curve":
            B = bad("off_curve")
        elif kind == "B_x_ge_p":
            B = bad("x_ge_p")
        elif kind == "B_neutral":
            B = bad("neutral")
        elif kind == "B_neutral_C_off_curve":
            B, C = bad("neutral"), bad("off_curve")
        elif kind == "C_x_ge_p":
            C = bad("x_ge_p")
        elif kind == "C_neutral":
            C = bad("neutral")
        elif kind == "C_off_curve":
            C = bad("off_curve")
        code, valid = verify(A, B, C, proof, msg)
        out.append(dict(A=A, B=B, C=C, proof=proof, msg=msg, code=code, valid=valid, kind=kind, a=a, b=b))
    return out


# ---- arrays ----------------------------------------------------------------------------------------------------------------------
def le32(v):
    return np.frombuffer(v.to_bytes(32, "little"), np.uint8)


def rows(items, width=32):
    return np.frombuffer(b"".join(items), np.uint8).reshape(len(items), width).copy() if items else np.zeros((0, width), np.uint8)


def points(pts):
    """(x, y) little-endian arrays of wire points"""
    return (np.stack([le32(p[0]) for p in pts]) if pts else np.zeros((0, 32), np.uint8),
            np.stack([le32(p[1]) for p in pts]) if pts else np.zeros((0, 32), np.uint8))


@functools.lru_cache(maxsize=None)
def prover_arrays(with_msg):
    S = prover_set(with_msg)
    bx, by = points([p["B"] for p in S])
    cx, cy = points([p["C"] for p in S])
    return dict(a=np.stack([le32(p["a"]) for p in S]), bx=bx, by=by, aux=rows([p["aux"] for p in S]),
                msg=rows([p["msg"] for p in S]) if with_msg else None, proof=rows([p["proof"] for p in S], 64), cx=cx, cy=cy,
                err=np.array([p["code"] for p in S], np.uint8))


@functools.lru_cache(maxsize=None)
def verifier_arrays(with_msg):
    S = verifier_set(with_msg)
    ax, ay = points([p["A"] for p in S])
    bx, by = points([p["B"] for p in S])
    cx, cy = points([p["C"] for p in S])
    return dict(ax=ax, ay=ay, bx=bx, by=by, cx=cx, cy=cy, proof=rows([p["proof"] for p in S], 64),
                msg=rows([p["msg"] for p in S]) if with_msg else None, err=np.array([p["code"] for p in S], np.uint8),
                valid=np.array([p["valid"] for p in S], np.uint8))


def forced_cases():
    """[(a, b, k, e)] for the arithmetic behind the hashes: k = 0, 1, n - 1, n (= 0 mod n), a random one; e = 0, 1, n - 1, n,
    n + 5 (= 5 mod n), 2^256 - 1, a random one"""
    ks = [0, 1, N - 1, N, _rand("fk", 0, N)]
    es = [0, 1, N - 1, N, N + 5, (1 << 256) - 1, _rand("fe", 0)]
    out = []
    for j, k in enumerate(ks):
        for i, e in enumerate(es):
            out.append((_rand("fa", 7 * j + i, N), _rand("fb", 7 * j + i, N), k, e))
    return out
