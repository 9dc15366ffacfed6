"""Taproot (BIP-341) leaf hashes, Merkle roots, key tweaks and the script-path commitment check, restated from the BIP's
text in Python integers and hashlib: the oracle of tests/test_taproot_cpu.py and tests/test_gpu_taproot.py, and the input
sets both run.  Nothing here uses the code under test; the curve helpers and tag_midstate are tests/schnorr_inputs.py's.

Wire forms are the standard's: 32-byte big-endian strings for keys, hashes and tweaks.  Error bytes are include/p2e.h's
P2E_WIRE_* codes, the first failing check in the header's order; a flagged element is all zeros.

The three PINS were computed independently (hashlib and big integers); the first three output keys, both roots and the leaf
hashes are those of BIP-341's wallet test vectors.
"""
import functools
import hashlib

import numpy as np

import schnorr_inputs as SI
from schnorr_inputs import N, P, b32, base_mul, lift_x, tag_midstate, tagged_hash  # noqa: F401

WIRE_OK, WIRE_BAD_LENGTH, WIRE_BAD_PREFIX, WIRE_COORD_RANGE, WIRE_NOT_ON_CURVE, WIRE_INFINITY, WIRE_SCALAR_RANGE = 0, 1, 2, 3, 4, 5, 8
TAGS = ("TapLeaf", "TapBranch", "TapTweak")
MAX_DEPTH = 128
COUNTS = (0, 1, 63, 64, 65, 257)     # array lengths every per-element test runs: empty, one lane, a wave, a block's tail
SCRIPT_LENGTHS = (0, 1, 53, 54, 55, 62, 117, 118, 119, 252, 253, 254, 0xFFFF, 0x10000)

PINS = (
    dict(internal="d6889cb081036e0faefa3a35157ad71086b123b2b144b649798b494c300a961d", leaves=(),
         root=None, tweak="b86e7be8f39bab32a6f2c0443abbc210f0edac0e2c53d501b36b64437d9c6c70",
         output="53a1f6e454df1aa2776a2814a721372d6258050de330b3c6d10ee8f4e0dda343", parity=1),
    dict(internal="187791b6f712a8ea41c8ecdd0ee77fab3e85263b37e1ec18a3651926b3a6cf27",
         leaves=((0xC0, "20d85a959b0290bf19bb89ed43c916be835475d013da4b362117393e25a48229b8ac",
                  "5b75adecf53548f3ec6ad7d78383bf84cc57b55a3127c72b9a2481752dd88b21"),),
         root="5b75adecf53548f3ec6ad7d78383bf84cc57b55a3127c72b9a2481752dd88b21",
         tweak="cbd8679ba636c1110ea247542cfbd964131a6be84f873f7f3b62a777528ed001",
         output="147c9c57132f6e7ecddba9800bb0c4449251c92a1e60371ee77557b6620f3ea3", parity=1),
    dict(internal="93478e9488f956df2396be2ce6c5cced75f900dfa18e7dabd2428aae78451820",
         leaves=((0xC0, "20387671353e273264c495656e27e39ba899ea8fee3bb69fb2a680e22093447d48ac",
                  "8ad69ec7cf41c2a4001fd1f738bf1e505ce2277acdcaa63fe4765192497f47a7"),
                 (0xFA, "06424950333431", "f224a923cd0021ab202ab139cc56802ddb92dcfc172b9212261a539df79a112a")),
         root="6c2dc106ab816b73f9d07e3cd1ef2c8c1256f519748e0813e4edd2405d277bef",
         tweak="086fa59904c93821fe5a117676ece79b495f3ca4eb98c9e55dfe9d25fc83c025",
         output="fb5c2771a52e84a51e097346361d30cab666fc34416e4b9f72a843e636f8d110", parity=1),
)


# ---- BIP-341, from its text ------------------------------------------------------------------------------------------------
def compact_size(n):
    if n < 253:
        return bytes([n])
    if n <= 0xFFFF:
        return b"\xfd" + n.to_bytes(2, "little")
    assert n < 1 << 32
    return b"\xfe" + n.to_bytes(4, "little")


def leaf_hash(version, script):
    """(code, leaf32): bit 0 of the version is the control block's parity bit and never part of a leaf version"""
    if version & 1:
        return WIRE_BAD_PREFIX, bytes(32)
    return WIRE_OK, tagged_hash("TapLeaf", bytes([version]) + compact_size(len(script)) + script)


def branch(a, b):
    return tagged_hash("TapBranch", min(a, b) + max(a, b))       # (bytes compare lexicographically)


def merkle_root(leaf, path):
    k = leaf
    for e in path:
        k = branch(k, e)
    return k


def tweak_int(pk, root):
    """int(H_TapTweak(pk || root)); root None: nothing is appended"""
    return int.from_bytes(tagged_hash("TapTweak", pk + (root or b"")), "big")


def _add_tG(Pt, t):
    """Pt + t G for an affine Pt, or None"""
    return SI._affine(SI._jadd(SI._gmul(t), (Pt[0], Pt[1], 1)))


def finish_pub(Pt, t):
    """(code, out_pk32, parity) for the point Pt and ANY 256-bit t"""
    if t >= N:
        return WIRE_SCALAR_RANGE, bytes(32), 0
    Q = _add_tG(Pt, t)
    if Q is None:
        return WIRE_INFINITY, bytes(32), 0
    return WIRE_OK, b32(Q[0]), Q[1] & 1


def finish_sec(d, t):
    """(code, out_sk32) for the adjusted key d and ANY 256-bit t"""
    if t >= N:
        return WIRE_SCALAR_RANGE, bytes(32)
    s = (d + t) % N
    return (WIRE_INFINITY, bytes(32)) if s == 0 else (WIRE_OK, b32(s))


def key_code(pk):
    """(code, point with even y or None) of an x-only key"""
    x = int.from_bytes(pk, "big")
    if x >= P:
        return WIRE_COORD_RANGE, None
    Pt = lift_x(x)
    return (WIRE_NOT_ON_CURVE, None) if Pt is None else (WIRE_OK, Pt)


def tweak_pubkey(pk, root):
    code, Pt = key_code(pk)
    if code:
        return code, bytes(32), 0
    return finish_pub(Pt, tweak_int(pk, root))


def tweak_seckey(sk, root):
    d = int.from_bytes(sk, "big")
    if d == 0 or d >= N:
        return WIRE_SCALAR_RANGE, bytes(32)
    Pt = base_mul(d)
    if Pt[1] & 1:
        d = N - d
    return finish_sec(d, tweak_int(b32(Pt[0]), root))


def verify_commitment(out_pk, out_parity, pk, leaf, path, depth, max_depth):
    """(code, valid); path: max_depth nodes, the first `depth` of them walked"""
    if out_parity > 1:
        return WIRE_BAD_PREFIX, 0
    if depth > max_depth:
        return WIRE_BAD_LENGTH, 0
    code, Pt = key_code(pk)
    if code:
        return code, 0
    code, q, par = finish_pub(Pt, tweak_int(pk, merkle_root(leaf, path[:depth])))
    if code:
        return code, 0
    return WIRE_OK, int(q == out_pk and par == out_parity)


# ---- input sets (deterministic) --------------------------------------------------------------------------------------------------
def _stream(label, nbytes):
    out, k = b"", 0
    while len(out) < nbytes:
        out += hashlib.sha256(b"taproot inputs/" + label.encode() + k.to_bytes(4, "big")).digest()
        k += 1
    return out[:nbytes]


def _rows(list_of_bytes, width=32):
    return np.frombuffer(b"".join(list_of_bytes), np.uint8).reshape(-1, width).copy() if list_of_bytes else np.zeros((0, width), np.uint8)


def _u8(v):
    return np.array(v, np.uint8)


def _xonly(label):
    """an x-only key that is on the curve"""
    d = int.from_bytes(_stream(label, 32), "big") % (N - 1) + 1
    return b32(base_mul(d)[0])


@functools.lru_cache(maxsize=None)
def script_set(lengths=SCRIPT_LENGTHS):
    """Every length at all four byte alignments of ONE concatenated buffer (a filler of 0 .. 3 bytes, an element of its own,
    moves the next start); behind the second length the pins' leaves, one odd version and one reversed pair of offsets (its
    end lies 5 bytes before its start; the element behind it reads those 5 bytes again).  Returns a dict: version (n,),
    data (bytes,), offsets (n + 1,), leaf (n, 32), err (n,); `front` bytes of 0xEE lie before offsets[0] and `back` behind
    offsets[n]: a lane must read none of them in a word that holds no byte of its own script."""
    front, back = 8, 8
    data, offsets, versions, scripts = b"\xEE" * front, [front], [], []

    def put(version, script):
        nonlocal data
        if script is None:                                        # the reversed pair, then the same bytes forwards
            offsets.append(offsets[-1] - 5), versions.append(version), scripts.append(None)
            script = data[-5:]
        else:
            data += script
        offsets.append(offsets[-1] + len(script)), versions.append(version), scripts.append(script)

    for k, L in enumerate(lengths):
        for al in range(4):
            put(0xC0, _stream(f"fill{k}.{L}.{al}", (al - len(data)) % 4))
            put((0xC0, 0xC2, 0xFA, 0x00)[al], _stream(f"script{k}.{L}.{al}", L))
        if k == min(1, len(lengths) - 1):
            for pin in PINS:
                for ver, script, _h in pin["leaves"]:
                    put(ver, bytes.fromhex(script))
            put(0xC1, _stream("odd version", 34))
            put(0xC0, None)
    data += b"\xEE" * back
    leaf, err = [], []
    for ver, s in zip(versions, scripts):
        code, h = (WIRE_BAD_PREFIX if ver & 1 else WIRE_BAD_LENGTH, bytes(32)) if s is None else leaf_hash(ver, s)
        leaf.append(h), err.append(code)
    return dict(version=_u8(versions), data=np.frombuffer(data, np.uint8).copy(), offsets=np.array(offsets, np.uint64),
                leaf=_rows(leaf), err=_u8(err), front=front, back=back)


SMALL_SCRIPT_LENGTHS = tuple(L for L in SCRIPT_LENGTHS if L < 0xFFFF) * 3      # 288 short elements and the special ones


def _near(k, delta):
    """k with its last byte moved by delta (no carry out of the byte)"""
    last = k[31]
    if not 0 <= last + delta <= 255:
        delta = -delta
    return k[:31] + bytes([last + delta])


@functools.lru_cache(maxsize=None)
def path_set(n=257, max_depth=MAX_DEPTH):
    """leaf (n, 32), path (n, max_depth, 32), depth (n,), root (n, 32), err (n,).  Depths 0, 1, 2, 7 and max_depth mixed (depth
    128 beside depth 0 in the first wave), nodes equal to the running hash and one last-byte step to either side of it, and
    depth > max_depth."""
    cycle = [d for d in (0, max_depth, 1, 2, 7, max_depth, 0, 3) if d <= max_depth] or [0]
    leaf, path, depth, root, err = [], [], [], [], []
    for i in range(n):
        lf = _stream(f"leaf{i}", 32)
        d = cycle[i % len(cycle)]
        nodes, k = [], lf
        for j in range(max_depth):
            e = _stream(f"node{i}.{j}", 32)
            if j < d and (i + j) % 5 == 1:
                e = (k, _near(k, 1), _near(k, -1))[(i // 5 + j) % 3]       # equal, just above, just below the running hash
            nodes.append(e)
            if j < d:
                k = branch(k, e)
        code = WIRE_OK
        if i % 29 == 17 and max_depth < 255:
            d, code, k = max_depth + 1 + (i % 3), WIRE_BAD_LENGTH, bytes(32)
        leaf.append(lf), path.append(b"".join(nodes)), depth.append(d), root.append(k), err.append(code)
    pa = np.frombuffer(b"".join(path), np.uint8).reshape(n, max_depth, 32).copy() if max_depth else np.zeros((n, 0, 32), np.uint8)
    return dict(leaf=_rows(leaf), path=pa, depth=_u8(depth), root=_rows(root), err=_u8(err), max_depth=max_depth)


def _off_curve_x():
    x = 2
    while lift_x(x) is not None:
        x += 1
    return x


@functools.lru_cache(maxsize=None)
def pubkey_set(n=257):
    """pk (n, 32), root (n, 32), and per form (with the roots / with no root): out (n, 32), parity (n,), err (n,)"""
    pk, root = [], []
    for i in range(n):
        pk.append(_xonly(f"pk{i}")), root.append(_stream(f"root{i}", 32))
    for j, pin in enumerate(PINS):
        pk[3 + j] = bytes.fromhex(pin["internal"])
        root[3 + j] = bytes.fromhex(pin["root"]) if pin["root"] else root[3 + j]
    special = [b32(P), b32(P + 5), b32(2**256 - 1), b32(_off_curve_x()), bytes(32)]     # (x = 0: 7 is no square mod p)
    for j, v in enumerate(special):
        if 10 + 7 * j < n:
            pk[10 + 7 * j] = v
    out = {"pk": _rows(pk), "root": _rows(root)}
    for form, roots in (("with_root", root), ("no_root", [None] * n)):
        res = [tweak_pubkey(k, r) for k, r in zip(pk, roots)]
        out[form] = dict(out=_rows([r[1] for r in res]), parity=_u8([r[2] for r in res]), err=_u8([r[0] for r in res]))
    return out


@functools.lru_cache(maxsize=None)
def seckey_set(n=257):
    """sk (n, 32), root (n, 32), and per form: out (n, 32), err (n,).  Keys 0, n, n - 1, 2^256 - 1 and points of both parities."""
    sk, root = [], []
    for i in range(n):
        sk.append(b32(int.from_bytes(_stream(f"sk{i}", 32), "big") % (N - 1) + 1)), root.append(_stream(f"root{i}", 32))
    for j, v in enumerate((0, N, N - 1, 2**256 - 1, 1, 2, 3)):
        if 2 + 9 * j < n:
            sk[2 + 9 * j] = b32(v)
    out = {"sk": _rows(sk), "root": _rows(root)}
    if n >= 64:
        par = {base_mul(int.from_bytes(k, "big"))[1] & 1 for k in sk if 0 < int.from_bytes(k, "big") < N}
        assert par == {0, 1}
    for form, roots in (("with_root", root), ("no_root", [None] * n)):
        res = [tweak_seckey(k, r) for k, r in zip(sk, roots)]
        out[form] = dict(out=_rows([r[1] for r in res]), err=_u8([r[0] for r in res]))
    return out


@functools.lru_cache(maxsize=None)
def commitment_set(n=257, max_depth=8):
    """out_pk (n, 32), out_parity (n,), pk (n, 32), leaf (n, 32), path (n, max_depth, 32), depth (n,), err (n,), valid (n,).
    Correct commitments (all three leaves of the pins among them), then by i mod 11: wrong parity, a wrong out_pk, out_pk >= p,
    one path node flipped, a wrong leaf, parity byte 2, depth > max_depth, a key >= p, a key off the curve."""
    rows = []
    for i in range(n):
        pk, leaf = _xonly(f"cpk{i}"), _stream(f"cleaf{i}", 32)
        depth = (0, 1, 2, max_depth, 3)[i % 5] if max_depth else 0
        depth = min(depth, max_depth)
        path = [_stream(f"cnode{i}.{j}", 32) for j in range(max_depth)]
        rows.append([pk, leaf, path, depth])
    pin2, pin3 = PINS[1], PINS[2]
    if n > 5 and max_depth >= 1:
        h = [bytes.fromhex(x[2]) for x in pin3["leaves"]]
        for at, (mine, other) in ((1, (h[0], h[1])), (2, (h[1], h[0]))):
            rows[at] = [bytes.fromhex(pin3["internal"]), mine, [other] + rows[at][2][1:], 1]
        rows[4] = [bytes.fromhex(pin2["internal"]), bytes.fromhex(pin2["leaves"][0][2]), rows[4][2], 0]
    cols = dict(out_pk=[], out_parity=[], pk=[], leaf=[], path=[], depth=[], err=[], valid=[])
    for i, (pk, leaf, path, depth) in enumerate(rows):
        code, q, par = tweak_pubkey(pk, merkle_root(leaf, path[:depth]))
        assert code == WIRE_OK
        kind = i % 11 if i > 5 else 0
        if kind == 1:
            par ^= 1
        elif kind == 2:
            q = _near(q, 1)
        elif kind == 3:
            q = b32(P + (i % 7))
        elif kind == 4 and depth:
            j = i % depth
            path = path[:j] + [bytes([path[j][0] ^ 0x80]) + path[j][1:]] + path[j + 1:]
        elif kind == 5:
            leaf = _near(leaf, 1)
        elif kind == 6:
            par = 2
        elif kind == 7:
            depth = max_depth + 1
        elif kind == 8:
            pk = b32(P + 1)
        elif kind == 9:
            pk = b32(_off_curve_x())
        code, valid = verify_commitment(q, par, pk, leaf, path, depth, max_depth)
        for key, v in zip(cols, (q, par, pk, leaf, b"".join(path), depth, code, valid)):
            cols[key].append(v)
    pa = (np.frombuffer(b"".join(cols["path"]), np.uint8).reshape(n, max_depth, 32).copy() if max_depth and n
          else np.zeros((n, max_depth, 32), np.uint8))
    out = dict(out_pk=_rows(cols["out_pk"]), out_parity=_u8(cols["out_parity"]), pk=_rows(cols["pk"]), leaf=_rows(cols["leaf"]), path=pa,
               depth=_u8(cols["depth"]), err=_u8(cols["err"]), valid=_u8(cols["valid"]), max_depth=max_depth)
    if n >= 64 and max_depth:
        assert {0, 1} <= set(out["valid"].tolist()) and {WIRE_OK, WIRE_BAD_PREFIX, WIRE_BAD_LENGTH, WIRE_COORD_RANGE,
                                                         WIRE_NOT_ON_CURVE} <= set(out["err"].tolist())
    return out


@functools.lru_cache(maxsize=None)
def forced_pub():
    """[(pk32, t32, code, out32, parity)]: values of t no hash will ever produce, behind the split at the hash"""
    rows = []
    for label in ("fa", "fb"):
        k = int.from_bytes(_stream(label, 32), "big") % (N - 1) + 1
        if base_mul(k)[1] & 1:
            k = N - k                                  # k G has even y: it IS lift_x of its abscissa
        Pt = base_mul(k)
        for t in (N, N + 1, 2**256 - 1, 0, k, N - k, 1, N - 1, (k + 1) % N, (N - k + 1) % N):
            rows.append((b32(Pt[0]), b32(t)) + finish_pub(Pt, t))
    codes = [r[2] for r in rows]
    assert codes.count(WIRE_SCALAR_RANGE) == 6 and codes.count(WIRE_INFINITY) == 2
    return rows


@functools.lru_cache(maxsize=None)
def forced_sec():
    """[(d32, t32, code, out32)]: d is the adjusted key, as taproot_finish_sec takes it"""
    rows = []
    for label in ("fc", "fd"):
        d = int.from_bytes(_stream(label, 32), "big") % (N - 1) + 1
        for t in (N, 2**256 - 1, 0, N - d, (N - d + 1) % N, (N - d - 1) % N, 1, N - 1):
            rows.append((b32(d), b32(t)) + finish_sec(d, t))
    rows.append((b32(N - 1), b32(1)) + finish_sec(N - 1, 1))
    rows.append((b32(1), b32(N - 1)) + finish_sec(1, N - 1))
    codes = [r[2] for r in rows]
    assert codes.count(WIRE_SCALAR_RANGE) == 4 and codes.count(WIRE_INFINITY) == 4
    return rows


def check_pins():
    """the oracle against the pins; returns the number of values compared"""
    seen = 0
    for pin in PINS:
        pk = bytes.fromhex(pin["internal"])
        hashes = []
        for ver, script, want in pin["leaves"]:
            code, h = leaf_hash(ver, bytes.fromhex(script))
            assert code == 0 and h.hex() == want
            hashes.append(h)
            seen += 1
        root = None
        if len(hashes) == 1:
            root = hashes[0]
        elif len(hashes) == 2:
            root = merkle_root(hashes[0], [hashes[1]])
            assert root == merkle_root(hashes[1], [hashes[0]])
        assert (root.hex() if root else None) == pin["root"]
        assert b32(tweak_int(pk, root)).hex() == pin["tweak"]
        code, q, par = tweak_pubkey(pk, root)
        assert (code, q.hex(), par) == (0, pin["output"], pin["parity"])
        seen += 3
        for k, h in enumerate(hashes):
            path = [hashes[1 - k]] if len(hashes) == 2 else []
            assert verify_commitment(q, par, pk, h, path, len(path), len(path)) == (0, 1)
            seen += 1
    return seen
