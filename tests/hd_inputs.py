"""BIP-32 key derivation and HASH160 on secp256k1, restated from the standards in Python integers, hmac and hashlib: the
oracle of tests/test_hd_cpu.py and tests/test_gpu_hd.py, and the input sets both run.  Nothing here uses the code under test.

  BIP-32       master key generation, CKDpriv, CKDpub (the public derivation of a non-hardened child);
  HASH160      RIPEMD-160(SHA-256(.)); RIPEMD-160 is written out below from the paper (Dobbertin, Bosselaers, Preneel 1996):
               the hashlib of many builds has none;
  SHA-512      hashlib for digests; the compression function is also written out (FIPS 180-4 section 6.4), because the two
               "Bitcoin seed" key states are chaining values and hashlib shows none.
The curve arithmetic is tests/schnorr_inputs.py's (Python integers, Jacobian coordinates).

Bytes, as include/p2e.h gives them: keys and coordinates are the library's 32-byte little-endian values, chain codes and
hashes are byte strings in their standard's order, an index is a uint32.  Error bytes are P2E_WIRE_* codes, the first
failing check in the header's order; a flagged element's outputs are all zeros."""
import functools
import hashlib
import hmac
import struct

import numpy as np

import schnorr_inputs as SI
from schnorr_inputs import G, N, P, le32, rows  # noqa: F401

WIRE_OK, WIRE_COORD_RANGE, WIRE_NOT_ON_CURVE, WIRE_INFINITY, WIRE_SCALAR_RANGE, WIRE_BAD_INDEX = 0, 3, 4, 5, 8, 10
SEC1_COMPRESSED, SEC1_UNCOMPRESSED = 0, 1
HARDENED = 1 << 31
LENGTHS = (0, 1, 63, 64, 65, 257)     # batch sizes of every call: nothing, one lane, a wave less one, a wave, a wave plus one, a block plus one
N_SET = 257

# ---- published answers ---------------------------------------------------------------------------------------------------------
# RIPEMD-160's own test vectors (the paper's appendix B).  "abc" ends in ...f15a0bfc there; a copy that reads ...f15a5bfc is a typo.
RIPEMD160_KAT = ((b"", "9c1185a5c5e9fc54612808977ee8f548b2258d31"), (b"abc", "8eb208f7e05d987a9b044a8e98c6b087f15a0bfc"),
                 (b"message digest", "5d0689ef49d2fae572b881b123a85ffa21595f36"),
                 (b"abcdefghijklmnopqrstuvwxyz", "f71c27109c692c1b56bbdceb5b9d2865b3708dbc"))
HASH160_OF_G = "751e76e8199196d454941c45d1b3a323f1433bd6"            # the compressed key of sk = 1
TV1_SEED = bytes(range(16))                                          # BIP-32 test vector 1
TV1_M = (0xe8f32e723decf4051aefac8e2c93c9c5b214313817cdb01a1494b917c8436b35,
         bytes.fromhex("873dff81c02f525623fd1fe5167eac3a55a049de3d314bb42ee227ffed37d508"))
TV1_M_0H = (0xedb2e14f9ee77d26dd93b4ecede8d16ed408ce149b6cd80b0715a2d911a0afea,
            bytes.fromhex("47fdacbd0f1097043b78c63c20c34ef4ed9a111d980047ad16282c7ae6236141"),
            bytes.fromhex("035a784662a4a20a65bf6aab9ae98a6c068a81c52e4b032c0fb5400c706cfccc56"))
TV1_M_0H_1 = (0x3c6cb8d0f6a264c91ea8b5030fadaa8e538b020f0a387421a12de9319dc93368,
              bytes.fromhex("2a7857631386ba23dacac34180dd1983734e444fdbf774041578e9b6adb37c19"),
              bytes.fromhex("03501e454bf00751f24b1b489aa925215d66af2234e3891c3b21a52bedb3cd711c"))


# ---- RIPEMD-160 ------------------------------------------------------------------------------------------------------------------
RIPEMD160_IV = (0x67452301, 0xEFCDAB89, 0x98BADCFE, 0x10325476, 0xC3D2E1F0)
_RL = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 7, 4, 13, 1, 10, 6, 15, 3, 12, 0, 9, 5, 2, 14, 11, 8,
       3, 10, 14, 4, 9, 15, 8, 1, 2, 7, 0, 6, 13, 11, 5, 12, 1, 9, 11, 10, 0, 8, 12, 4, 13, 3, 7, 15, 14, 5, 6, 2,
       4, 0, 5, 9, 7, 12, 2, 10, 14, 1, 3, 8, 11, 6, 15, 13]
_RR = [5, 14, 7, 0, 9, 2, 11, 4, 13, 6, 15, 8, 1, 10, 3, 12, 6, 11, 3, 7, 0, 13, 5, 10, 14, 15, 8, 12, 4, 9, 1, 2,
       15, 5, 1, 3, 7, 14, 6, 9, 11, 8, 12, 2, 10, 0, 4, 13, 8, 6, 4, 1, 3, 11, 15, 0, 5, 12, 2, 13, 9, 7, 10, 14,
       12, 15, 10, 4, 1, 5, 8, 7, 6, 2, 13, 14, 0, 3, 9, 11]
_SL = [11, 14, 15, 12, 5, 8, 7, 9, 11, 13, 14, 15, 6, 7, 9, 8, 7, 6, 8, 13, 11, 9, 7, 15, 7, 12, 15, 9, 11, 7, 13, 12,
       11, 13, 6, 7, 14, 9, 13, 15, 14, 8, 13, 6, 5, 12, 7, 5, 11, 12, 14, 15, 14, 15, 9, 8, 9, 14, 5, 6, 8, 6, 5, 12,
       9, 15, 5, 11, 6, 8, 13, 12, 5, 12, 13, 14, 11, 8, 5, 6]
_SR = [8, 9, 9, 11, 13, 15, 15, 5, 7, 7, 8, 11, 14, 14, 12, 6, 9, 13, 15, 7, 12, 8, 9, 11, 7, 7, 12, 7, 6, 15, 13, 11,
       9, 7, 15, 11, 8, 6, 6, 14, 12, 13, 5, 14, 13, 13, 7, 5, 15, 5, 8, 11, 14, 14, 6, 14, 6, 9, 12, 9, 12, 5, 15, 8,
       8, 5, 12, 9, 12, 5, 14, 6, 8, 13, 6, 5, 15, 13, 11, 11]
_KL = (0x00000000, 0x5A827999, 0x6ED9EBA1, 0x8F1BBCDC, 0xA953FD4E)
_KR = (0x50A28BE6, 0x5C4DD124, 0x6D703EF3, 0x7A6D76E9, 0x00000000)
_M32 = 0xFFFFFFFF


def _rol32(x, s):
    return ((x << s) | (x >> (32 - s))) & _M32


def _rmd_f(j, x, y, z):
    if j == 0:
        return x ^ y ^ z
    if j == 1:
        return (x & y) | (~x & _M32 & z)
    if j == 2:
        return (x | (~y & _M32)) ^ z
    if j == 3:
        return (x & z) | (y & ~z & _M32)
    return x ^ (y | (~z & _M32))


def ripemd160_compress(state, block):
    """one 64-byte block into the five chaining words"""
    x = struct.unpack("<16I", block)
    al, bl, cl, dl, el = state
    ar, br, cr, dr, er = state
    for j in range(80):
        t = (_rol32((al + _rmd_f(j // 16, bl, cl, dl) + x[_RL[j]] + _KL[j // 16]) & _M32, _SL[j]) + el) & _M32
        al, el, dl, cl, bl = el, dl, _rol32(cl, 10), bl, t
        t = (_rol32((ar + _rmd_f(4 - j // 16, br, cr, dr) + x[_RR[j]] + _KR[j // 16]) & _M32, _SR[j]) + er) & _M32
        ar, er, dr, cr, br = er, dr, _rol32(cr, 10), br, t
    h0, h1, h2, h3, h4 = state
    return ((h1 + cl + dr) & _M32, (h2 + dl + er) & _M32, (h3 + el + ar) & _M32, (h4 + al + br) & _M32, (h0 + bl + cr) & _M32)


def ripemd160_pad(length):
    """the bytes that follow a message of `length` bytes"""
    return b"\x80" + bytes((55 - length) % 64) + struct.pack("<Q", 8 * length)


def ripemd160(msg):
    data = msg + ripemd160_pad(len(msg))
    state = RIPEMD160_IV
    for at in range(0, len(data), 64):
        state = ripemd160_compress(state, data[at:at + 64])
    return struct.pack("<5I", *state)


def hash160(msg):
    return ripemd160(hashlib.sha256(msg).digest())


# ---- SHA-512's compression function ----------------------------------------------------------------------------------------------
def _frac_root(p, root, bits):
    """the first `bits` bits of the fractional part of p^(1/root), by integer bisection"""
    target, lo, hi = p << (root * bits), 0, 1 << (bits + 8)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if mid**root <= target else (lo, mid)
    return lo & ((1 << bits) - 1)


def _primes(count):
    out, c = [], 2
    while len(out) < count:
        if all(c % q for q in out):
            out.append(c)
        c += 1
    return out


SHA512_K = tuple(_frac_root(p, 3, 64) for p in _primes(80))
SHA512_IV = tuple(_frac_root(p, 2, 64) for p in _primes(8))
_M64 = (1 << 64) - 1


def _ror64(x, s):
    return ((x >> s) | (x << (64 - s))) & _M64


def sha512_compress(state, block):
    w = list(struct.unpack(">16Q", block))
    for t in range(16, 80):
        s0 = _ror64(w[t - 15], 1) ^ _ror64(w[t - 15], 8) ^ (w[t - 15] >> 7)
        s1 = _ror64(w[t - 2], 19) ^ _ror64(w[t - 2], 61) ^ (w[t - 2] >> 6)
        w.append((w[t - 16] + s0 + w[t - 7] + s1) & _M64)
    a, b, c, d, e, f, g, h = state
    for t in range(80):
        t1 = (h + (_ror64(e, 14) ^ _ror64(e, 18) ^ _ror64(e, 41)) + ((e & f) ^ (~e & _M64 & g)) + SHA512_K[t] + w[t]) & _M64
        t2 = ((_ror64(a, 28) ^ _ror64(a, 34) ^ _ror64(a, 39)) + ((a & b) ^ (a & c) ^ (b & c))) & _M64
        a, b, c, d, e, f, g, h = (t1 + t2) & _M64, a, b, c, (d + t1) & _M64, e, f, g
    return tuple((s + v) & _M64 for s, v in zip(state, (a, b, c, d, e, f, g, h)))


def sha512_pad(length):
    return b"\x80" + bytes((111 - length) % 128) + struct.pack(">QQ", 0, 8 * length)


def sha512_from_midstate(mid, done, rest):
    """SHA-512 continued from the chaining value `mid` reached after `done` bytes (a multiple of 128)"""
    data = rest + sha512_pad(done + len(rest))
    for at in range(0, len(data), 128):
        mid = sha512_compress(mid, data[at:at + 128])
    return struct.pack(">8Q", *mid)


def hmac512_key_states(key):
    """the chaining values after the ipad and the opad block of HMAC-SHA512 under `key` (at most 128 bytes)"""
    k = key + bytes(128 - len(key))
    return (sha512_compress(SHA512_IV, bytes(b ^ 0x36 for b in k)), sha512_compress(SHA512_IV, bytes(b ^ 0x5c for b in k)))


def hmac512(key, msg):
    return hmac.new(key, msg, hashlib.sha512).digest()


# ---- BIP-32 ------------------------------------------------------------------------------------------------------------------------
def base_mul(k):
    return SI.base_mul(k)


def ser_p(pt):
    return bytes([2 | (pt[1] & 1)]) + pt[0].to_bytes(32, "big")


def ser_u(pt):
    return b"\x04" + pt[0].to_bytes(32, "big") + pt[1].to_bytes(32, "big")


def split_i(i64):
    return int.from_bytes(i64[:32], "big"), i64[32:]


def master(seed):
    """(code, k, c): I_L = 0 or I_L >= n is WIRE_SCALAR_RANGE"""
    il, ir = split_i(hmac512(b"Bitcoin seed", seed))
    if il == 0 or il >= N:
        return WIRE_SCALAR_RANGE, 0, bytes(32)
    return WIRE_OK, il, ir


def finish_priv(il, k_par):
    """(code, k_child)"""
    if il >= N:
        return WIRE_SCALAR_RANGE, 0
    k = (il + k_par) % N
    return (WIRE_INFINITY, 0) if k == 0 else (WIRE_OK, k)


def finish_pub(il, kp):
    """(code, K_child) for a parent that passed its checks"""
    if il >= N:
        return WIRE_SCALAR_RANGE, (0, 0)
    pt = SI._affine(SI._jadd(SI._gmul(il), (kp[0], kp[1], 1)))
    return (WIRE_INFINITY, (0, 0)) if pt is None else (WIRE_OK, pt)


def priv_data(k, index):
    if index >= HARDENED:
        return b"\x00" + k.to_bytes(32, "big") + struct.pack(">I", index)
    return ser_p(base_mul(k)) + struct.pack(">I", index)


def ckd_priv(k, c, index):
    """(code, k_child, c_child)"""
    if k == 0 or k >= N:
        return WIRE_SCALAR_RANGE, 0, bytes(32)
    il, ir = split_i(hmac512(c, priv_data(k, index)))
    code, kc = finish_priv(il, k)
    return (code, 0, bytes(32)) if code else (code, kc, ir)


def pub_check(kp, index):
    if index >= HARDENED:
        return WIRE_BAD_INDEX
    if kp == (0, 0):
        return WIRE_INFINITY
    if kp[0] >= P or kp[1] >= P:
        return WIRE_COORD_RANGE
    if (kp[1] * kp[1] - kp[0]**3 - 7) % P:
        return WIRE_NOT_ON_CURVE
    return WIRE_OK


def ckd_pub(kp, c, index):
    """(code, K_child, c_child)"""
    code = pub_check(kp, index)
    if code:
        return code, (0, 0), bytes(32)
    il, ir = split_i(hmac512(c, ser_p(kp) + struct.pack(">I", index)))
    code, pt = finish_pub(il, kp)
    return (code, (0, 0), bytes(32)) if code else (code, pt, ir)


def key_hash160(kp, form):
    """HASH160 of the SEC1 string of ANY coordinate pair below 2^256 (nothing is checked, as for the Ethereum address)"""
    return hash160(ser_p(kp) if form == SEC1_COMPRESSED else ser_u(kp))


# ---- input sets ------------------------------------------------------------------------------------------------------------------
def _rand(label, i):
    return hashlib.sha256(f"hd-inputs/{label}/{i}".encode()).digest()


def _rand_int(label, i):
    return int.from_bytes(_rand(label, i), "big")


INDEX_EDGES = (0, 1, HARDENED - 1, HARDENED, HARDENED + 1, 2**32 - 1)


def _index(i):
    """the six edges and one arbitrary index, period 7; the arbitrary ones alternate between hardened and not"""
    if i % 7 < 6:
        return INDEX_EDGES[i % 7]
    return (_rand_int("index", i) % HARDENED) | (HARDENED if (i // 7) & 1 else 0)


@functools.lru_cache(maxsize=None)
def indices():
    return np.array([_index(i) for i in range(N_SET)], np.uint32)


def _priv_parent(i):
    """period 9 (coprime to the indices' 7): 1, n - 1, the three refused values, arbitrary keys"""
    fixed = {0: 1, 1: N - 1, 2: 0, 3: N, 4: 2**256 - 1}
    return fixed[i % 9] if i % 9 in fixed else _rand_int("parent-sk", i) % (N - 1) + 1


@functools.lru_cache(maxsize=None)
def priv_set():
    """{'sk', 'cc' (257, 32), 'index' (257,), expected 'out_sk', 'out_cc', 'err'} with one parent per element"""
    ks = [_priv_parent(i) for i in range(N_SET)]
    ccs = [_rand("parent-cc", i) for i in range(N_SET)]
    return _priv_arrays(ks, ccs, [int(v) for v in indices()])


def _priv_arrays(ks, ccs, idx):
    n_par = len(ks)
    out = [ckd_priv(ks[i % n_par if n_par > 1 else 0], ccs[i % n_par if n_par > 1 else 0], idx[i]) for i in range(len(idx))]
    return {"sk": np.stack([le32(k) for k in ks]), "cc": rows(ccs), "index": np.array(idx, np.uint32),
            "out_sk": np.stack([le32(o[1]) for o in out]), "out_cc": rows([o[2] for o in out]), "err": np.array([o[0] for o in out], np.uint8)}


@functools.lru_cache(maxsize=None)
def priv_set_one_parent():
    """the same indices under ONE parent, test vector 1's m/0' (n_parents = 1)"""
    return _priv_arrays([TV1_M_0H[0]], [TV1_M_0H[1]], [int(v) for v in indices()])


def _pub_parent(i):
    """period 9: (0, 0), x >= p, y >= p, off the curve, a y of each parity, arbitrary points"""
    kind = i % 9
    if kind == 0:
        return (0, 0)
    pt = base_mul(_rand_int("parent-pk", i) % (N - 1) + 1)
    if kind == 1:                                   # x + p still fits 256 bits only for a small x: look one up
        x = next(x for x in range(1, 100) if SI.lift_x(x))
        return (x + P, SI.lift_x(x)[1])
    if kind == 2:
        return (pt[0], 2**256 - 1)
    if kind == 3:
        return (pt[0], (pt[1] + 1) % P)
    if kind == 4:
        return pt if pt[1] & 1 else (pt[0], P - pt[1])
    if kind == 5:
        return pt if not pt[1] & 1 else (pt[0], P - pt[1])
    return pt


def _pub_arrays(kps, ccs, idx):
    one = len(kps) == 1
    out = [ckd_pub(kps[0 if one else i], ccs[0 if one else i], idx[i]) for i in range(len(idx))]
    return {"pkx": np.stack([le32(k[0]) for k in kps]), "pky": np.stack([le32(k[1]) for k in kps]), "cc": rows(ccs),
            "index": np.array(idx, np.uint32), "out_x": np.stack([le32(o[1][0]) for o in out]),
            "out_y": np.stack([le32(o[1][1]) for o in out]), "out_cc": rows([o[2] for o in out]),
            "err": np.array([o[0] for o in out], np.uint8)}


@functools.lru_cache(maxsize=None)
def pub_set():
    return _pub_arrays([_pub_parent(i) for i in range(N_SET)], [_rand("parent-cc", i) for i in range(N_SET)], [int(v) for v in indices()])


@functools.lru_cache(maxsize=None)
def pub_set_one_parent():
    """the xpub scan: every index under test vector 1's m/0' (hardened indices are refused)"""
    return _pub_arrays([base_mul(TV1_M_0H[0])], [TV1_M_0H[1]], [int(v) for v in indices()])


SEED_LENGTHS = (16, 32, 63, 64)


@functools.lru_cache(maxsize=None)
def master_set(seed_len):
    """{'seed' (257, seed_len), expected 'sk', 'cc', 'err'}; element 0 of the 16-byte set is test vector 1's seed"""
    seeds = [(_rand("seed-a", i) + _rand("seed-b", i))[:seed_len] for i in range(N_SET)]
    if seed_len == 16:
        seeds[0] = TV1_SEED
    out = [master(s) for s in seeds]
    return {"seed": rows(seeds, seed_len), "sk": np.stack([le32(o[1]) for o in out]), "cc": rows([o[2] for o in out]),
            "err": np.array([o[0] for o in out], np.uint8)}


HASH160_LENGTHS = (0, 1, 55, 56, 63, 64, 65, 119)
HASH160_REVERSED = 100          # the element whose offsets run backwards: hashed as the empty message, and counted


@functools.lru_cache(maxsize=None)
def hash160_arrays():
    """(data uint8, offsets uint64 (258,), expected (257, 20)) as the call takes them: message i = data[offsets[i], offsets[i + 1]),
    nothing between two messages.  The eight lengths come in shuffled rounds; five of them are odd, so the running sum puts
    every length at every start address modulo 4 (asserted below).  One element's offsets run backwards."""
    rng = np.random.default_rng(0x161)
    order = []
    for rep in range(N_SET // 8 + 1):            # lengths 1, 55, 63, 65, 119 are odd: the running sum meets every residue
        order += list(rng.permutation(8))
    lens = [HASH160_LENGTHS[j] for j in order[:N_SET]]
    offsets = np.zeros(N_SET + 1, np.uint64)
    offsets[1:] = np.cumsum(lens)
    data = rng.integers(0, 256, int(offsets[-1]), dtype=np.uint8)
    raw = data.tobytes()
    msgs = [raw[int(offsets[i]):int(offsets[i + 1])] for i in range(N_SET)]
    # the reversed element: offsets[r + 1] < offsets[r].  Element r is then empty, element r + 1 starts at the lower offset.
    r = HASH160_REVERSED
    offsets[r + 1] = offsets[r] - 3
    msgs[r] = b""
    msgs[r + 1] = raw[int(offsets[r + 1]):int(offsets[r + 2])]
    seen = {(len(m), int(offsets[i]) % 4) for i, m in enumerate(msgs)}
    assert all((ln, a) in seen for ln in HASH160_LENGTHS for a in range(4))
    want = rows([hash160(m) for m in msgs], 20)
    return data, offsets, want


@functools.lru_cache(maxsize=None)
def key_hash_set():
    """{'pkx', 'pky' (257, 32), 'err_in' (257,), expected 'c', 'u' (257, 20) without err_in, 'c_err', 'u_err' with it}:
    G first, then curve points of both parities and arbitrary pairs (HASH160 of any 33 / 65 bytes is defined)"""
    kps = [G] + [base_mul(_rand_int("hash-key", i) % (N - 1) + 1) if i % 3 else (_rand_int("hash-x", i), _rand_int("hash-y", i))
                 for i in range(1, N_SET)]
    err_in = np.array([(i % 5 == 2) * (1 + i % 250) for i in range(N_SET)], np.uint8)
    c = rows([key_hash160(k, SEC1_COMPRESSED) for k in kps], 20)
    u = rows([key_hash160(k, SEC1_UNCOMPRESSED) for k in kps], 20)
    flag = (err_in != 0)[:, None]
    return {"pkx": np.stack([le32(k[0]) for k in kps]), "pky": np.stack([le32(k[1]) for k in kps]), "err_in": err_in,
            "c": c, "u": u, "c_err": np.where(flag, 0, c).astype(np.uint8), "u_err": np.where(flag, 0, u).astype(np.uint8)}


# ---- the forced-I_L table of the issue ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def forced_priv():
    """[(name, I_L, k_par, code, k_child)]"""
    k = _rand_int("forced-k", 0) % (N - 1) + 1
    cases = [("il_n", N, k), ("il_n_plus_1", N + 1, k), ("il_max", 2**256 - 1, k), ("il_zero", 0, k), ("il_cancels", N - k, k),
             ("il_ordinary", _rand_int("forced-il", 0) % N, k), ("il_n_minus_1", N - 1, 2)]
    return [(name, il, kp) + finish_priv(il, kp) for name, il, kp in cases]


@functools.lru_cache(maxsize=None)
def forced_pub():
    """[(name, I_L, K_par, code, K_child)]"""
    k = _rand_int("forced-k", 1) % (N - 1) + 1
    il = _rand_int("forced-il", 1) % (N - 1) + 1
    kp = base_mul(k)
    cases = [("il_n", N, kp), ("il_n_plus_1", N + 1, kp), ("il_max", 2**256 - 1, kp), ("il_zero", 0, kp),
             ("parent_is_minus_il_g", il, base_mul(N - il)), ("parent_is_il_g", il, base_mul(il)), ("il_ordinary", il, kp),
             ("il_one_parent_g", 1, G), ("il_n_minus_1_parent_g", N - 1, G)]
    return [(name, i, p) + finish_pub(i, p) for name, i, p in cases]
