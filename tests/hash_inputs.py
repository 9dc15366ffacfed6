"""Inputs and independent expectations of the hashing, nonce and address tests (test_hash_cpu.py, test_gpu_hash.py).

Expectations use nothing of the code under test:
  SHA-256, SHA-256d   hashlib.sha256;
  Keccak-256          oracle/p2e_ref.py keccak256 (pinned by known answers in tests/test_oracle.py);
  RFC 6979            section 3.2 written out below with hmac and hashlib, the group order a parameter;
  keys, signatures    oracle/p2e_ref.py's big-int curves.
Every expectation is computed once per session and shared."""
import functools
import hashlib
import hmac

import numpy as np

import p2e_ref as R

SHA256, SHA256D, KECCAK256 = 0, 1, 2
DIGEST_BYTES, DIGEST_SCALAR = 0, 1
ALGS = (SHA256, SHA256D, KECCAK256)
CURVES = [R.SECP256K1, R.P256]
N_MAIN = 4161            # 65 full waves + one lane

# lengths around every place the padding changes shape
SHA_LENGTHS = [0, 1, 3, 55, 56, 57, 63, 64, 65, 119, 120, 121, 127, 128, 129, 1000]       # block 64, length field at 56
KECCAK_LENGTHS = [0, 1, 7, 8, 9, 135, 136, 137, 271, 272, 273, 1000]                     # rate 136

# published answers (FIPS 180-4 / the Keccak team's vectors / RFC 6979 A.2.5 / well-known secp256k1 values)
SHA256_ABC = "ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad"
KECCAK_EMPTY = "c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470"
KECCAK_ABC = "4e03657aea45a94fc7d47ba826c8d667c0d1e6e33a64a036ec44f58fa12d6c45"
A25_X = 0xC9AFA9D845BA75166B5C215767B1D6934E50C3DB36E89B127B8A622B120F6721
A25_SAMPLE_K = 0xA6E3C57DD01ABE90086538398355DD4C3B17AA873382B0F24D6129493D8AAD60
A25_SAMPLE_R = 0xEFD48B2AACB6A8FD1140DD9CD45E81D69D2C877B56AAF991C34D0EA84EAF3716
A25_SAMPLE_S = 0xF7CB1C942D657C41D436C7A1B6E29F65F3E900DBB9AFF4064DC4AB2F843ACDA8
A25_TEST_K = 0xD16B6AE827F17175E040871A1C7EC3500192C4C92677336EC2537ACAEE0008E0
SATOSHI_K = 0x8F8A276C19F4149656B280621E358CCE24F5F52542772691EE69063B74F15D15      # secp256k1, sk = 1, sha256("Satoshi Nakamoto")
ADDRESS_OF_G = "7e5f4552091a69125d5dfcb7b8c2659029395bdf"


def digest(alg, msg: bytes) -> bytes:
    if alg == KECCAK256:
        return R.keccak256(msg)
    d = hashlib.sha256(msg).digest()
    return hashlib.sha256(d).digest() if alg == SHA256D else d


def pack(vals):
    """ints -> (n, 32) uint8 little-endian"""
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), np.uint8).reshape(-1, 32).copy()


def unpack(arr):
    return [int.from_bytes(bytes(row), "little") for row in np.asarray(arr)]


def rfc6979(q, x, z):
    """RFC 6979 section 3.2 for qlen = hlen = 256: (k, number of candidates refused).  x < q; z any 256-bit value."""
    mac = lambda key, msg: hmac.new(key, msg, hashlib.sha256).digest()
    xh = x.to_bytes(32, "big") + (z - q if z >= q else z).to_bytes(32, "big")      # int2octets(x) || bits2octets(h1)
    v, k = b"\x01" * 32, b"\x00" * 32
    k = mac(k, v + b"\x00" + xh)
    v = mac(k, v)
    k = mac(k, v + b"\x01" + xh)
    v = mac(k, v)
    refused = 0
    while True:
        v = mac(k, v)
        cand = int.from_bytes(v, "big")
        if 1 <= cand < q:
            return cand, refused
        refused += 1
        k = mac(k, v + b"\x00")
        v = mac(k, v)


def address(x, y) -> bytes:
    return R.keccak256(x.to_bytes(32, "big") + y.to_bytes(32, "big"))[12:]


@functools.lru_cache(maxsize=None)
def message_batch(alg, n=N_MAIN):
    """One concatenated buffer of n messages without padding: the algorithm's edge lengths cycled, then shuffled with a
    fixed seed so that the lanes of a wave mix block counts and start offsets take every residue modulo 8.
    -> (data uint8, offsets uint64 (n + 1), [message bytes])"""
    lengths = KECCAK_LENGTHS if alg == KECCAK256 else SHA_LENGTHS
    rng = np.random.default_rng(0x4A5 + alg)
    lens = [lengths[i % len(lengths)] for i in range(n)]
    rng.shuffle(lens)
    offsets = np.zeros(n + 1, np.uint64)
    offsets[1:] = np.cumsum(lens)
    data = rng.integers(0, 256, int(offsets[-1]), dtype=np.uint8)
    raw = data.tobytes()
    msgs = [raw[int(offsets[i]):int(offsets[i + 1])] for i in range(n)]
    starts = offsets[:-1].astype(np.int64)
    assert set(starts % 8) == set(range(8)) and set(starts[:64] % 4) == set(range(4))
    for w in range(0, n - 63, 64 * 16):                      # waves mix block counts
        assert len(set(lens[w:w + 64])) > 4
    return data, offsets, msgs


@functools.lru_cache(maxsize=None)
def digests(alg, n=N_MAIN):
    """(n, 32) expected digest bytes of message_batch(alg, n)"""
    _, _, msgs = message_batch(alg, n)
    cache = {}
    rows = []
    for m in msgs:
        if m not in cache:
            cache[m] = digest(alg, m)
        rows.append(cache[m])
    return np.frombuffer(b"".join(rows), np.uint8).reshape(n, 32).copy()


def as_form(d, form):
    """expected out32 rows for an output form: DIGEST_SCALAR is the digest's bytes reversed"""
    return d[:, ::-1].copy() if form == DIGEST_SCALAR else d


@functools.lru_cache(maxsize=None)
def nonce_batch(curve_id, n=N_MAIN):
    """(msg ints, sk ints, expected k ints): every pair of {0, 1, n - 1, n, 2^256 - 1} first, random 256-bit values after"""
    cv = CURVES[curve_id]
    edge = [0, 1, cv.n - 1, cv.n, (1 << 256) - 1]
    rng = R.SplitMix64(0x6979 + curve_id)
    pairs = [(m, d) for m in edge for d in edge]
    pairs += [(rng.below(1 << 256), rng.below(1 << 256)) for _ in range(n - len(pairs))]
    msg, sk = [p[0] for p in pairs], [p[1] for p in pairs]
    want = [rfc6979(cv.n, d - cv.n if d >= cv.n else d, m)[0] for m, d in pairs]
    return msg, sk, want


# the retry branch: a synthetic order just above 2^255, under which about half of all candidates are refused
RETRY_Q = (1 << 255) + 1
RETRY_N = 200


@functools.lru_cache(maxsize=None)
def retry_set():
    """(x ints, z ints, expected k ints, expected refusal counts) for q = 2^255 + 1, x = i + 1, z = sha256(bytes([i]))"""
    xs = [i + 1 for i in range(RETRY_N)]
    zs = [int.from_bytes(hashlib.sha256(bytes([i])).digest(), "big") for i in range(RETRY_N)]
    out = [rfc6979(RETRY_Q, x, z) for x, z in zip(xs, zs)]
    return xs, zs, [o[0] for o in out], [o[1] for o in out]


@functools.lru_cache(maxsize=None)
def address_batch(n=N_MAIN):
    """(pkx (n, 32), pky (n, 32), expected (n, 20)): 1 G first, then n - 1 arbitrary coordinate pairs (the address of any 64
    bytes is defined: nothing here needs the pair to be a curve point)"""
    rng = R.SplitMix64(0xADD2)
    xs = [R.GX] + [rng.below(1 << 256) for _ in range(n - 1)]
    ys = [R.GY] + [rng.below(1 << 256) for _ in range(n - 1)]
    want = np.frombuffer(b"".join(address(x, y) for x, y in zip(xs, ys)), np.uint8).reshape(n, 20).copy()
    return pack(xs), pack(ys), want


def sign(cv, msg, sk, k):
    """sign_message with Python integers and the big-int curve: (r, s, v)"""
    pt = cv.mul(k, cv.g) if cv is not R.SECP256K1 else R.ec_mul(k, R.G)
    r = pt[0] % cv.n
    return r, pow(k, -1, cv.n) * (msg + r * sk) % cv.n, (pt[1] & 1) | (2 if pt[0] >= cv.n else 0)
