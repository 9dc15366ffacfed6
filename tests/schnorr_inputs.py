"""BIP-340 Schnorr signatures on secp256k1, restated from the standard in Python integers and hashlib: the oracle of
tests/test_schnorr_cpu.py and tests/test_gpu_schnorr.py, and the input sets both run.  Nothing here uses the code under test.

Wire forms are the standard's: 32-byte big-endian strings for sk, msg, aux, the x-only pk, and sig = bytes(r) || bytes(s).
Error bytes are include/p2e.h's P2E_WIRE_* codes, the first failing check in the header's order.

The aggregate check (include/p2e.h p2e_schnorr_verify_aggregate) is restated twice: as the AND of the per-element verdicts
(`aggregate_expected`) and as the randomised sum itself with the header's a_i (`aggregate_terms`, `sum_is_neutral`).
"""
import functools
import hashlib
import struct

import numpy as np

P = 2**256 - 2**32 - 977
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
G = (0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798,
     0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8)
WIRE_OK, WIRE_COORD_RANGE, WIRE_NOT_ON_CURVE, WIRE_INFINITY, WIRE_SCALAR_RANGE = 0, 3, 4, 5, 8
TAGS = ("BIP0340/aux", "BIP0340/nonce", "BIP0340/challenge")
LENGTHS = (1, 63, 64, 65, 257)       # array lengths every per-element test runs: one lane, a wave, a block's tail

KNOWN_SK = (3).to_bytes(32, "big")
KNOWN_PK = bytes.fromhex("F9308A019258C31049344F85F89D5229B531C845836F99B08601F113BCE036F9")
KNOWN_SIG = bytes.fromhex("E907831F80848D1069A5371B402410364BDF1C5F8307B0084C55F1CE2DCA8215"
                          "25F66A4A85EA8B71E482A74F382D2CE5EBEEE8FDB2172F477DF4900D310536C0")


# ---- the curve, in Jacobian coordinates (None: the neutral element) -------------------------------------------------------
def _jdbl(a):
    x, y, z = a
    s = 4 * x * y * y % P
    m = 3 * x * x % P
    x3 = (m * m - 2 * s) % P
    return x3, (m * (s - x3) - 8 * pow(y, 4, P)) % P, 2 * y * z % P


def _jadd(a, b):
    if a is None:
        return b
    if b is None:
        return a
    x1, y1, z1 = a
    x2, y2, z2 = b
    zz1, zz2 = z1 * z1 % P, z2 * z2 % P
    u1, u2 = x1 * zz2 % P, x2 * zz1 % P
    s1, s2 = y1 * zz2 * z2 % P, y2 * zz1 * z1 % P
    if u1 == u2:
        return _jdbl(a) if s1 == s2 else None
    h, r = (u2 - u1) % P, (s2 - s1) % P
    h2 = h * h % P
    h3, v = h2 * h % P, u1 * h2 % P
    x3 = (r * r - h3 - 2 * v) % P
    return x3, (r * (v - x3) - s1 * h3) % P, h * z1 * z2 % P


def _affine(a):
    if a is None:
        return None
    zi = pow(a[2], -1, P)
    return a[0] * zi * zi % P, a[1] * zi * zi * zi % P


def _jmul(k, pt):
    """k * pt for an affine pt, k >= 0 (any size), as a Jacobian point"""
    acc, base = None, (pt[0], pt[1], 1)
    for bit in bin(k)[2:]:
        acc = None if acc is None else _jdbl(acc)
        if bit == "1":
            acc = _jadd(acc, base)
    return acc


@functools.lru_cache(maxsize=None)
def _g_table():
    """d 16^w G for w < 64, d < 16 (None for d = 0): a multiple of G is then at most 64 additions"""
    rows, base = [], (G[0], G[1], 1)
    for _ in range(64):
        row, acc = [None], None
        for _ in range(15):
            acc = _jadd(acc, base)
            row.append(acc)
        rows.append(row)
        base = _jadd(acc, base)
    return rows


def _gmul(k):
    acc = None
    for w, row in enumerate(_g_table()):
        acc = _jadd(acc, row[(k >> (4 * w)) & 15])
    return acc


def base_mul(k):
    return _affine(_gmul(k % N))


def lift_x(x, odd=False):
    """the point with abscissa x and the wanted parity of y; None where x >= p or x^3 + 7 is no square"""
    if x >= P:
        return None
    c = (pow(x, 3, P) + 7) % P
    y = pow(c, (P + 1) // 4, P)
    if y * y % P != c:
        return None
    return x, (P - y if (y & 1) != odd else y)


# ---- hashes -----------------------------------------------------------------------------------------------------------------
def tagged_hash(tag, data):
    t = hashlib.sha256(tag.encode()).digest()
    return hashlib.sha256(t + t + data).digest()


_K = [0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be,
      0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa,
      0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85,
      0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3,
      0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f,
      0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2]
SHA256_IV = (0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19)


def sha256_compress(state, block):
    """FIPS 180-4 6.2.2 on one 64-byte block (hashlib does not expose the chaining value a midstate is)"""
    rotr = lambda x, n: ((x >> n) | (x << (32 - n))) & 0xFFFFFFFF
    w = list(struct.unpack(">16I", block))
    for t in range(16, 64):
        s0 = rotr(w[t - 15], 7) ^ rotr(w[t - 15], 18) ^ (w[t - 15] >> 3)
        s1 = rotr(w[t - 2], 17) ^ rotr(w[t - 2], 19) ^ (w[t - 2] >> 10)
        w.append((w[t - 16] + s0 + w[t - 7] + s1) & 0xFFFFFFFF)
    a, b, c, d, e, f, g, h = state
    for t in range(64):
        t1 = (h + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + _K[t] + w[t]) & 0xFFFFFFFF
        t2 = ((rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c))) & 0xFFFFFFFF
        a, b, c, d, e, f, g, h = (t1 + t2) & 0xFFFFFFFF, a, b, c, (d + t1) & 0xFFFFFFFF, e, f, g
    return tuple((x + y) & 0xFFFFFFFF for x, y in zip(state, (a, b, c, d, e, f, g, h)))


def sha256_from_midstate(mid, done, rest):
    """SHA-256 of a message whose first `done` bytes (a multiple of 64) led to the chaining value `mid`"""
    total = done + len(rest)
    rest = rest + b"\x80" + b"\x00" * ((55 - total) % 64) + struct.pack(">Q", 8 * total)
    for o in range(0, len(rest), 64):
        mid = sha256_compress(mid, rest[o:o + 64])
    return struct.pack(">8I", *mid)


def tag_midstate(tag):
    t = hashlib.sha256(tag.encode()).digest()
    return sha256_compress(SHA256_IV, t + t)


# ---- BIP-340 ------------------------------------------------------------------------------------------------------------------
def b32(v):
    return v.to_bytes(32, "big")


def public_key(sk):
    """(code, pk32)"""
    d = int.from_bytes(sk, "big")
    if d == 0 or d >= N:
        return WIRE_SCALAR_RANGE, bytes(32)
    return WIRE_OK, b32(base_mul(d)[0])


def challenge(rx, px, msg):
    return int.from_bytes(tagged_hash("BIP0340/challenge", b32(rx) + b32(px) + msg), "big") % N


def sign_with_nonce(d, px, msg, k0, negate=True):
    """the signature under the (already adjusted) key d with nonce k'; negate=False keeps k = k' whatever R.y is"""
    if k0 == 0:
        return WIRE_INFINITY, bytes(64)
    R = base_mul(k0)
    k = N - k0 if (negate and R[1] & 1) else k0
    return WIRE_OK, b32(R[0]) + b32((k + challenge(R[0], px, msg) * d) % N)


def nonce(sk, msg, aux):
    """(d adjusted, P.x, k'), or None where sk is out of range"""
    d0 = int.from_bytes(sk, "big")
    if d0 == 0 or d0 >= N:
        return None
    Pt = base_mul(d0)
    d = N - d0 if Pt[1] & 1 else d0
    t = b32(d ^ int.from_bytes(tagged_hash("BIP0340/aux", aux), "big"))
    return d, Pt[0], int.from_bytes(tagged_hash("BIP0340/nonce", t + b32(Pt[0]) + msg), "big") % N


def sign(msg, sk, aux):
    """BIP-340 default signing: (code, sig64)"""
    v = nonce(sk, msg, aux)
    if v is None:
        return WIRE_SCALAR_RANGE, bytes(64)
    return sign_with_nonce(v[0], v[1], msg, v[2])


@functools.lru_cache(maxsize=None)
def verify(msg, pk, sig):
    """(err, valid)"""
    px, r, s = int.from_bytes(pk, "big"), int.from_bytes(sig[:32], "big"), int.from_bytes(sig[32:], "big")
    if px >= P:
        return WIRE_COORD_RANGE, 0
    Pt = lift_x(px)
    if Pt is None:
        return WIRE_NOT_ON_CURVE, 0
    if r >= P:
        return WIRE_COORD_RANGE, 0
    if s >= N:
        return WIRE_SCALAR_RANGE, 0
    e = challenge(r, px, msg)
    X = _affine(_jadd(_gmul(s), _jmul((N - e) % N, Pt)))
    return WIRE_OK, int(X is not None and X[1] % 2 == 0 and X[0] == r)


def xonly_decode(pk):
    """(code, x, y) with even y; zeros where flagged"""
    px = int.from_bytes(pk, "big")
    if px >= P:
        return WIRE_COORD_RANGE, 0, 0
    Pt = lift_x(px)
    return (WIRE_NOT_ON_CURVE, 0, 0) if Pt is None else (WIRE_OK, Pt[0], Pt[1])


# ---- the aggregate check --------------------------------------------------------------------------------------------------------
def randomizer(seed, i):
    a = int.from_bytes(hashlib.sha256(seed + struct.pack("<Q", i)).digest()[:16], "big")
    return a or 1


def aggregate_err(msg, pk, sig):
    """the element's code in the aggregate call: the verifier's four checks, then the lift of r"""
    err, _ = verify(msg, pk, sig)
    if err == WIRE_OK and lift_x(int.from_bytes(sig[:32], "big")) is None:
        err = WIRE_NOT_ON_CURVE
    return err


def aggregate_terms(msgs, pks, sigs, seed):
    """(errs, scalars, points) of the 2 n + 1 terms in the header's order: [0] (sum a_i s_i mod n, G); [1 + i] (a_i, -R_i);
    [1 + n + i] (a_i e_i mod n, -P_i); a flagged element is (0, None) twice and adds nothing to term 0"""
    n = len(msgs)
    errs, scal, pts, total = [], [0] * (2 * n + 1), [None] * (2 * n + 1), 0
    for i, (msg, pk, sig) in enumerate(zip(msgs, pks, sigs)):
        err = aggregate_err(msg, pk, sig)
        errs.append(err)
        if err:
            continue
        px, r, s = int.from_bytes(pk, "big"), int.from_bytes(sig[:32], "big"), int.from_bytes(sig[32:], "big")
        a = randomizer(seed, i)
        total = (total + a * s) % N
        scal[1 + i], pts[1 + i] = a, lift_x(r, odd=True)
        scal[1 + n + i], pts[1 + n + i] = a * challenge(r, px, msg) % N, lift_x(px, odd=True)
    scal[0], pts[0] = total, G
    return errs, scal, pts


def sum_is_neutral(scalars, points):
    """sum k_i P_i == the neutral element, by buckets per c-bit window (the plain sum of products, only with fewer additions)"""
    c = 4 if len(scalars) < 200 else 8
    acc = None
    for w in reversed(range(0, 256, c)):
        for _ in range(c):
            acc = None if acc is None else _jdbl(acc)
        buckets = [None] * (1 << c)
        for k, pt in zip(scalars, points):
            d = ((k % N) >> w) & ((1 << c) - 1)
            if pt is not None and d:
                buckets[d] = _jadd(buckets[d], (pt[0], pt[1], 1))
        run = total = None
        for b in reversed(buckets[1:]):            # sum d B_d as the sum of the running sums
            run = _jadd(run, b)
            total = _jadd(total, run)
        acc = _jadd(acc, total)
    return acc is None


def aggregate_expected(msgs, pks, sigs):
    """(verdict, errs): the AND of the per-element verdicts, and the codes"""
    errs = [aggregate_err(m, p, s) for m, p, s in zip(msgs, pks, sigs)]
    return int(all(verify(m, p, s) == (WIRE_OK, 1) for m, p, s in zip(msgs, pks, sigs)) and not any(errs)), errs


# ---- input sets ---------------------------------------------------------------------------------------------------------------
def _rand(label, i):
    return hashlib.sha256(f"schnorr-inputs/{label}/{i}".encode()).digest()


class Signer:
    """one element of the signer set: inputs, and the oracle's outputs"""
    def __init__(self, kind, sk, msg, aux):
        self.kind, self.sk, self.msg, self.aux = kind, sk, msg, aux
        self.pk_err, self.pk = public_key(sk)
        self.err, self.sig = sign(msg, sk, aux)
        v = nonce(sk, msg, aux)
        self.key_odd = self.nonce_odd = None
        if v is not None:
            self.d, self.px, self.k0 = v
            self.key_odd = self.d != int.from_bytes(sk, "big")
            self.nonce_odd = bool(base_mul(self.k0)[1] & 1)


@functools.lru_cache(maxsize=None)
def signer_set():
    """257 elements: the known answer, sk in {1, n - 1} (computed) and {0, n, 2^256 - 1} (flagged), then random keys"""
    zero = bytes(32)
    out = [Signer("known", KNOWN_SK, zero, zero), Signer("sk_one", b32(1), _rand("m", 1), _rand("a", 1)),
           Signer("sk_n_minus_1", b32(N - 1), _rand("m", 2), _rand("a", 2)), Signer("sk_zero", zero, _rand("m", 3), _rand("a", 3)),
           Signer("sk_n", b32(N), _rand("m", 4), _rand("a", 4)), Signer("sk_max", b"\xff" * 32, _rand("m", 5), _rand("a", 5))]
    i = 0
    while len(out) < LENGTHS[-1]:
        out.append(Signer("random", b32(int.from_bytes(_rand("sk", i), "big") % (N - 1) + 1), _rand("msg", i), _rand("aux", i)))
        i += 1
    return tuple(out)


class Case:
    """one element of the verifier set with the oracle's (err, valid)"""
    def __init__(self, kind, msg, pk, sig):
        self.kind, self.msg, self.pk, self.sig = kind, msg, pk, sig
        self.err, self.valid = verify(msg, pk, sig)


def _flip(b, bit):
    v = bytearray(b)
    v[bit // 8] ^= 1 << (bit % 8)
    return bytes(v)


@functools.lru_cache(maxsize=None)
def verifier_set():
    """257 elements: every kind the issue lists, then the valid signatures of the signer set"""
    S = [s for s in signer_set() if s.err == 0]
    known = S[0]
    out = [Case("known", known.msg, KNOWN_PK, KNOWN_SIG)]
    a = S[10]
    r, s = a.sig[:32], int.from_bytes(a.sig[32:], "big")
    out.append(Case("s_negated", a.msg, a.pk, r + b32(N - s)))
    odd = next(x for x in S if x.nonce_odd and x.kind == "random")
    out.append(Case("nonce_not_negated", odd.msg, odd.pk, sign_with_nonce(odd.d, odd.px, odd.msg, odd.k0, negate=False)[1]))
    out.append(Case("x_neutral", a.msg, a.pk, r + b32(challenge(int.from_bytes(r, "big"), a.px, a.msg) * a.d % N)))
    off = next(x for x in range(2, 1000) if lift_x(x) is None)
    out.append(Case("r_off_curve", a.msg, a.pk, b32(off) + a.sig[32:]))
    out.append(Case("r_eq_p", a.msg, a.pk, b32(P) + a.sig[32:]))
    out.append(Case("r_max", a.msg, a.pk, b"\xff" * 32 + a.sig[32:]))
    out.append(Case("s_eq_n", a.msg, a.pk, r + b32(N)))
    out.append(Case("s_max", a.msg, a.pk, r + b"\xff" * 32))
    out.append(Case("s_zero", a.msg, a.pk, r + bytes(32)))
    out.append(Case("pk_zero", a.msg, bytes(32), a.sig))
    out.append(Case("pk_off_curve", a.msg, b32(off), a.sig))
    small = next(x for x in range(1, 1000) if lift_x(x) is not None)       # a valid key x with p + x < 2^256
    out.append(Case("pk_plus_p", a.msg, b32(P + small), a.sig))
    out.append(Case("pk_small", a.msg, b32(small), a.sig))                  # the same key unshifted: decodes, does not verify
    for j, b in enumerate(S[11:15]):
        out.append(Case("flip_msg", _flip(b.msg, 37 * j + 1), b.pk, b.sig))
        out.append(Case("flip_pk", b.msg, _flip(b.pk, 41 * j + 3), b.sig))
        out.append(Case("flip_r", b.msg, b.pk, _flip(b.sig, 43 * j + 5)))
        out.append(Case("flip_s", b.msg, b.pk, _flip(b.sig, 256 + 47 * j + 7)))
    for x in S:
        if len(out) == LENGTHS[-1]:
            break
        out.append(Case("valid", x.msg, x.pk, x.sig))
    return tuple(out)


def rows(items, width=32):
    """a list of byte strings as an (n, width) uint8 array"""
    return np.frombuffer(b"".join(items), np.uint8).reshape(len(items), width).copy()


def le32(v):
    return np.frombuffer(v.to_bytes(32, "little"), np.uint8)


@functools.lru_cache(maxsize=None)
def signer_arrays():
    """the signer set as arrays (shared: callers copy what they hand to the code under test)"""
    S = signer_set()
    return dict(msg=rows([s.msg for s in S]), sk=rows([s.sk for s in S]), aux=rows([s.aux for s in S]),
                pk=rows([s.pk for s in S]), pk_err=np.array([s.pk_err for s in S], np.uint8),
                sig=rows([s.sig for s in S], 64), err=np.array([s.err for s in S], np.uint8))


@functools.lru_cache(maxsize=None)
def verifier_arrays():
    """the verifier set as arrays, with the decode bridge's expectation (dx, dy little-endian, derr)"""
    V = verifier_set()
    dec = [xonly_decode(c.pk) for c in V]
    return dict(msg=rows([c.msg for c in V]), pk=rows([c.pk for c in V]), sig=rows([c.sig for c in V], 64),
                err=np.array([c.err for c in V], np.uint8), valid=np.array([c.valid for c in V], np.uint8),
                dx=np.stack([le32(d[1]) for d in dec]), dy=np.stack([le32(d[2]) for d in dec]),
                derr=np.array([d[0] for d in dec], np.uint8))


# ---- aggregate cases ----------------------------------------------------------------------------------------------------------
AGG_SIZES = (0, 1, 2, 65, 1000)
AGG_SEEDS = (hashlib.sha256(b"schnorr-inputs/seed/0").digest(), hashlib.sha256(b"schnorr-inputs/seed/1").digest())
AGG_FORCED_WINDOW = 7


@functools.lru_cache(maxsize=None)
def valid_batch(n):
    """n valid (msg, pk, sig): few keys, many messages (a key signs several times: the swap case needs it)"""
    keys = [s for s in signer_set() if s.err == 0][:16]
    out = []
    for i in range(n):
        k = keys[(i // 2) % len(keys)]               # elements 2 j and 2 j + 1 share a key
        msg = _rand("agg-msg", i)
        v = nonce(k.sk, msg, _rand("agg-aux", i))
        out.append((msg, k.pk, sign_with_nonce(v[0], v[1], msg, v[2])[1]))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def aggregate_cases(n):
    """{name: (msgs, pks, sigs)} for one batch size; every case but all_valid must give verdict 0"""
    base = [list(x) for x in zip(*valid_batch(n))] if n else [[], [], []]
    cases = {"all_valid": tuple(map(tuple, base))}
    if n == 0:
        return cases

    def variant(name, edits):
        m, p, s = [list(c) for c in base]
        for i, (what, val) in edits.items():
            {"msg": m, "pk": p, "sig": s}[what][i] = val
        cases[name] = (tuple(m), tuple(p), tuple(s))

    sig_s = lambda i: int.from_bytes(base[2][i][32:], "big")
    for name, i in (("bad_first", 0), ("bad_middle", n // 2), ("bad_last", n - 1)):
        variant(name, {i: ("sig", base[2][i][:32] + b32((sig_s(i) + 1) % N))})
    bad = verifier_set()
    for kind in ("r_eq_p", "s_eq_n", "pk_off_curve", "pk_plus_p", "r_off_curve"):
        c = next(x for x in bad if x.kind == kind)
        m, p, s = [list(col) for col in base]
        m[n // 2], p[n // 2], s[n // 2] = c.msg, c.pk, c.sig
        cases["err_" + kind] = (tuple(m), tuple(p), tuple(s))
    if n >= 2:
        i, j, delta = 0, 1, 0x1234567
        variant("delta_pair", {i: ("sig", base[2][i][:32] + b32((sig_s(i) + delta) % N)),
                               j: ("sig", base[2][j][:32] + b32((sig_s(j) - delta) % N))})
        variant("swapped_s", {i: ("sig", base[2][i][:32] + base[2][j][32:]), j: ("sig", base[2][j][:32] + base[2][i][32:])})
    return cases
