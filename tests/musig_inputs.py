"""MuSig2 (BIP-327): key aggregation, tweaks, nonce aggregation, session values, partial signatures, their verification and
the final signature, restated from include/p2e.h's definitions in Python integers and hashlib: the oracle of
tests/test_musig_cpu.py and tests/test_gpu_musig.py, and the input sets both run.  Nothing here uses the code under test; the
curve helpers and the BIP-340 verifier are tests/schnorr_inputs.py's.

Wire forms: points and secret scalars are 32-byte little-endian values, hashes, tweaks, messages, partial signatures, agg_pk32
and sig64 the standard's big-endian strings; keyagg192 and session128 are the records of include/p2e.h.  Error bytes are
P2E_WIRE_* codes, the first failing check in the header's order; a flagged element is all zeros.

What pins the oracle (tests/test_musig_cpu.py):
  (a) the standard's four key-aggregation vectors (KEYAGG_VECTORS): the two KeyAgg tags and the second-key rule;
  (b) the three tag midstates from hashlib;
  (c) every full round of the sets ends in a sig64 that tests/schnorr_inputs.py's BIP-340 verifier accepts under agg_pk32.
The tag "MuSig/noncecoef" is the standard's text; no recalled vector pins it, (c) pins everything else of the signing path.
"""
import functools
import hashlib

import numpy as np

import schnorr_inputs as SI
from schnorr_inputs import G, N, P, b32, base_mul, tag_midstate, tagged_hash  # noqa: F401

(WIRE_OK, WIRE_BAD_LENGTH, WIRE_BAD_PREFIX, WIRE_COORD_RANGE, WIRE_NOT_ON_CURVE, WIRE_INFINITY, WIRE_SCALAR_RANGE,
 WIRE_BAD_INDEX) = 0, 1, 2, 3, 4, 5, 8, 10
TAGS = ("KeyAgg list", "KeyAgg coefficient", "MuSig/noncecoef")
MAX_SIGNERS = 1024
TWEAK_PLAIN, TWEAK_XONLY, TWEAK_TAPROOT = 0, 1, 2
KA_GACC_NEG, KA_HAVE_PK2, KA_PK2_ODD = 1, 2, 4
COUNTS = (0, 1, 63, 64, 65, 257)     # array lengths every per-element test runs: empty, one lane, a wave, a block's tail
N_SET = 257

X1 = bytes.fromhex("02F9308A019258C31049344F85F89D5229B531C845836F99B08601F113BCE036F9")
X2 = bytes.fromhex("03DFF1D77F2A671C5F36183726DB2341BE58FEAE1DA2DECED843240F7B502BA659")
X3 = bytes.fromhex("023590A94E768F8E1815C2F24B4D80A8E3149316C3518CE7B7AD338368D038CA66")
KEYAGG_VECTORS = (    # (keys, xbytes(Q), y(Q) odd)
    ((X1, X2, X3), "90539EEDE565F5D054F32CC0C220126889ED1E5D193BAF15AEF344FE59D4610C", 0),
    ((X3, X2, X1), "6204DE8B083426DC6EAF9502D27024D53FC826BF7D2012148A0575435DF54B2B", 1),
    ((X1, X1, X1), "B436E3BAD62B8CD409969A224731C193D051162D8C5AE8B109306127DA3AA935", 0),
    ((X1, X1, X2, X2), "69BC22BFA5D106306E48A20679DE1D7389386124D07571D0D872686028C26A3E", 1),
)


# ---- helpers ---------------------------------------------------------------------------------------------------------------------
def point_code(pt):
    """the checks of a point that must not be neutral, in the header's order"""
    x, y = pt
    if x == 0 and y == 0:
        return WIRE_INFINITY
    if x >= P or y >= P:
        return WIRE_COORD_RANGE
    return WIRE_OK if (y * y - x * x * x - 7) % P == 0 else WIRE_NOT_ON_CURVE


def cbytes(pt):
    return bytes([2 | (pt[1] & 1)]) + b32(pt[0])


def cbytes_ext(pt):
    return bytes(33) if pt is None else cbytes(pt)


def cpoint(c):
    """the point of 33 compressed bytes"""
    return SI.lift_x(int.from_bytes(c[1:], "big"), odd=bool(c[0] & 1))


def point_mul(k, pt):
    return SI._affine(SI._jmul(k % N, pt)) if k % N else None


def point_add(a, b):
    ja = None if a is None else (a[0], a[1], 1)
    jb = None if b is None else (b[0], b[1], 1)
    return SI._affine(SI._jadd(ja, jb))


def point_neg(a):
    return None if a is None else (a[0], P - a[1])


def le(v):
    return v.to_bytes(32, "little")


def u32le(v):
    return v.to_bytes(4, "little")


# ---- the records ------------------------------------------------------------------------------------------------------------------
def keyagg_pack(Q, tacc, L, pk2, gacc_neg):
    flags = (KA_GACC_NEG if gacc_neg else 0) | (0 if pk2 is None else KA_HAVE_PK2 | (KA_PK2_ODD if pk2[0] & 1 else 0))
    return le(Q[0]) + le(Q[1]) + b32(tacc) + L + (bytes(32) if pk2 is None else pk2[1:]) + u32le(flags) + bytes(28)


def keyagg_parse(rec):
    """(code, dict): the checks of a record in the header's order"""
    Q = (int.from_bytes(rec[0:32], "little"), int.from_bytes(rec[32:64], "little"))
    tacc, L, pk2x = int.from_bytes(rec[64:96], "big"), rec[96:128], int.from_bytes(rec[128:160], "big")
    flags = int.from_bytes(rec[160:164], "little")
    code = point_code(Q)
    if not code and tacc >= N:
        code = WIRE_SCALAR_RANGE
    if not code and pk2x >= P:
        code = WIRE_COORD_RANGE
    if not code and flags & ~7:
        code = WIRE_BAD_PREFIX
    pk2 = bytes([3 if flags & KA_PK2_ODD else 2]) + rec[128:160] if flags & KA_HAVE_PK2 else None
    return code, dict(Q=Q, tacc=tacc, L=L, pk2=pk2, gacc_neg=bool(flags & KA_GACC_NEG))


def session_pack(b, e, rx, r_odd):
    return b32(b) + b32(e) + b32(rx) + u32le(1 if r_odd else 0) + bytes(28)


def session_parse(rec):
    b, e, rx = (int.from_bytes(rec[o:o + 32], "big") for o in (0, 32, 64))
    flags = int.from_bytes(rec[96:100], "little")
    if b >= N or e >= N:
        code = WIRE_SCALAR_RANGE
    elif rx == 0:
        code = WIRE_INFINITY
    elif rx >= P:
        code = WIRE_COORD_RANGE
    else:
        code = WIRE_BAD_PREFIX if flags & ~1 else WIRE_OK
    return code, dict(b=b, e=e, rx=rx, r_odd=bool(flags & 1))


def nonce_pack(R1, R2):
    return b"".join(le(c) for R in (R1, R2) for c in (R or (0, 0)))


def nonce_parse(rec):
    v = [int.from_bytes(rec[o:o + 32], "little") for o in (0, 32, 64, 96)]
    return (v[0], v[1]), (v[2], v[3])


# ---- BIP-327, from the header's definitions -------------------------------------------------------------------------------------------
def coefficient(L, pk2, pk):
    """a of the key with the compressed bytes pk"""
    return 1 if pk == pk2 else int.from_bytes(tagged_hash(TAGS[1], L + pk), "big") % N


def key_list(keys):
    """(L, pk2) of valid points"""
    pks = [cbytes(k) for k in keys]
    pk2 = next((p for p in pks if p != pks[0]), None)
    return tagged_hash(TAGS[0], b"".join(pks)), pk2


def key_agg(keys, coefs=None):
    """(code, keyagg192, agg_pk32) of a list of points (x, y); keys None: reversed offsets.  coefs: forced coefficients."""
    zero = (bytes(192), bytes(32))
    if keys is None or not 1 <= len(keys) <= MAX_SIGNERS:
        return (WIRE_BAD_LENGTH,) + zero
    for k in keys:
        if point_code(k):
            return (point_code(k),) + zero
    L, pk2 = key_list(keys)
    acc, memo = None, {}
    for j, k in enumerate(keys):
        a = coefficient(L, pk2, cbytes(k)) if coefs is None else coefs[j] % N
        if (a, k) not in memo:                     # (a list may hold one key a thousand times)
            memo[(a, k)] = k if a == 1 else point_mul(a, k)
        acc = point_add(acc, memo[(a, k)])
    if acc is None:
        return (WIRE_INFINITY,) + zero
    return WIRE_OK, keyagg_pack(acc, 0, L, pk2, False), b32(acc[0])


def taproot_t(qx, root):
    return int.from_bytes(tagged_hash("TapTweak", b32(qx) + (root or b"")), "big")


def apply_tweak(rec, tweak, mode):
    """(code, keyagg192, agg_pk32); tweak: 32 bytes, or None in mode 2"""
    zero = (bytes(192), bytes(32))
    code, r = keyagg_parse(rec)
    if code:
        return (code,) + zero
    t = taproot_t(r["Q"][0], tweak) if mode == TWEAK_TAPROOT else int.from_bytes(tweak, "big")
    return finish_tweak(r, t, mode != TWEAK_PLAIN)


def finish_tweak(r, t, xonly):
    zero = (bytes(192), bytes(32))
    neg = xonly and r["Q"][1] & 1
    if t >= N:
        return (WIRE_SCALAR_RANGE,) + zero
    Q = point_add(base_mul(t) if t else None, point_neg(r["Q"]) if neg else r["Q"])
    if Q is None:
        return (WIRE_INFINITY,) + zero
    tacc = (t + (N - r["tacc"] if neg else r["tacc"])) % N
    return WIRE_OK, keyagg_pack(Q, tacc, r["L"], r["pk2"], r["gacc_neg"] != bool(neg)), b32(Q[0])


def nonce_agg(nonces):
    """(code, aggnonce128) of a list of ((x, y), (x, y)); None: reversed offsets"""
    if nonces is None or not 1 <= len(nonces) <= MAX_SIGNERS:
        return WIRE_BAD_LENGTH, bytes(128)
    acc = [None, None]
    for pair in nonces:
        for R in pair:
            if point_code(R):
                return point_code(R), bytes(128)
        acc = [point_add(acc[h], pair[h]) for h in (0, 1)]
    return WIRE_OK, nonce_pack(acc[0], acc[1])


def agg_halves(aggnonce):
    """(code, R_1 or None, R_2 or None)"""
    out = []
    for R in nonce_parse(aggnonce):
        if R == (0, 0):
            out.append(None)
        elif point_code(R):
            return point_code(R), None, None
        else:
            out.append(R)
    return WIRE_OK, out[0], out[1]


def nonce_coef(R1, R2, qx, msg):
    return int.from_bytes(tagged_hash(TAGS[2], cbytes_ext(R1) + cbytes_ext(R2) + b32(qx) + msg), "big") % N


def session(rec, aggnonce, msg, b=None):
    """(code, session128); b: a forced coefficient"""
    code, r = keyagg_parse(rec)
    if code:
        return code, bytes(128)
    code, R1, R2 = agg_halves(aggnonce)
    if code:
        return code, bytes(128)
    qx = r["Q"][0]
    b = nonce_coef(R1, R2, qx, msg) if b is None else b % N
    R = point_add(R1, None if R2 is None else point_mul(b, R2)) or G
    return WIRE_OK, session_pack(b, SI.challenge(R[0], qx, msg), R[0], R[1] & 1)


def key_factor(r, s, pk):
    """e a g gacc mod n for the key with the compressed bytes pk"""
    c = s["e"] * coefficient(r["L"], r["pk2"], pk) % N
    return (N - c) % N if bool(r["Q"][1] & 1) != r["gacc_neg"] else c


def partial_sign(k1, k2, d, rec, ses):
    """(code, psig32): integers k1, k2, d"""
    for v in (k1, k2, d):
        if not 0 < v < N:
            return WIRE_SCALAR_RANGE, bytes(32)
    code, r = keyagg_parse(rec)
    if code:
        return code, bytes(32)
    code, s = session_parse(ses)
    if code:
        return code, bytes(32)
    if s["r_odd"]:
        k1, k2 = N - k1, N - k2
    return WIRE_OK, b32((k1 + s["b"] * k2 + key_factor(r, s, cbytes(base_mul(d))) * d) % N)


def partial_verify(psig, pubnonce, pk, rec, ses):
    """(code, valid): rec / ses None: the session index is out of range"""
    if rec is None:
        return WIRE_BAD_INDEX, 0
    sv = int.from_bytes(psig, "big")
    if sv >= N:
        return WIRE_SCALAR_RANGE, 0
    R1, R2 = nonce_parse(pubnonce)
    code = point_code(R1) or point_code(R2) or point_code(pk)
    if code:
        return code, 0
    code, r = keyagg_parse(rec)
    if code:
        return code, 0
    code, s = session_parse(ses)
    if code:
        return code, 0
    Re = point_add(R1, point_mul(s["b"], R2))
    if s["r_odd"]:
        Re = point_neg(Re)
    left = base_mul(sv) if sv else None
    return WIRE_OK, int(left == point_add(Re, point_mul(key_factor(r, s, cbytes(pk)), pk)))


def sig_agg(psigs, rec, ses):
    """(code, sig64); psigs None: reversed offsets"""
    if psigs is None or not 1 <= len(psigs) <= MAX_SIGNERS:
        return WIRE_BAD_LENGTH, bytes(64)
    code, r = keyagg_parse(rec)
    if code:
        return code, bytes(64)
    code, s = session_parse(ses)
    if code:
        return code, bytes(64)
    total = 0
    for p in psigs:
        v = int.from_bytes(p, "big")
        if v >= N:
            return WIRE_SCALAR_RANGE, bytes(64)
        total += v
    et = s["e"] * r["tacc"] % N
    total += N - et if r["Q"][1] & 1 else et
    return WIRE_OK, b32(s["rx"]) + b32(total % N)


# ---- input sets (deterministic) --------------------------------------------------------------------------------------------------
def _stream(label, nbytes):
    out, k = b"", 0
    while len(out) < nbytes:
        out += hashlib.sha256(b"musig inputs/" + label.encode() + k.to_bytes(4, "big")).digest()
        k += 1
    return out[:nbytes]


def _scalar(label):
    return int.from_bytes(_stream(label, 32), "big") % (N - 1) + 1


def rows(items, width):
    """a (len, width) uint8 array of byte strings"""
    return np.frombuffer(b"".join(items), np.uint8).reshape(-1, width).copy() if items else np.zeros((0, width), np.uint8)


def _off_curve():
    x = 5
    while SI.lift_x(x) is not None:
        x += 1
    return x, 1


BAD_POINTS = {"neutral": ((0, 0), WIRE_INFINITY), "off": (_off_curve(), WIRE_NOT_ON_CURVE), "range": ((P, 1), WIRE_COORD_RANGE)}
EDGE_SCALARS = (0, N - 1, N, 2**256 - 1)


def session_secrets(i):
    """the secret keys of session i of the chain.  The first wave mixes 1, 2, 3 and 17 signers and holds the duplicate lists
    [A, A, A] (no second key) and [A, A, B, B]; behind it sessions have one or two signers."""
    if i == 4:
        return [_scalar("sk/4/0")] * 3
    if i == 5:
        a, b = _scalar("sk/5/0"), _scalar("sk/5/1")
        return [a, a, b, b]
    u = (1, 2, 3, 17)[i % 4] if i < 64 else 1 + i % 2
    return [_scalar(f"sk/{i}/{j}") for j in range(u)]


CHAIN_BAD_KEYS = {7: (0, "neutral"), 9: (1, "off"), 11: (0, "range")}    # session: (signer, what its key is)
CHAIN_EMPTY = 13                                                          # a session without signers


def offsets_of(lists):
    return np.cumsum([0] + [len(v) for v in lists]).astype(np.uint64)


@functools.lru_cache(maxsize=None)
def chain(n=N_SET):
    """One full round per session: key aggregation, a plain then an x-only tweak, nonce aggregation, the session values, every
    signer's partial signature, its verification, the final signature -- inputs and the oracle's outputs of all seven calls,
    as arrays.  Sessions CHAIN_BAD_KEYS hold a bad key and CHAIN_EMPTY no signer: their flag travels down the chain."""
    c = dict(n=n, sks=[], keys=[], secnonces=[], pubnonces=[])
    for i in range(n):
        sks = [] if i == CHAIN_EMPTY else session_secrets(i)
        keys = [base_mul(d) for d in sks]
        if i in CHAIN_BAD_KEYS:
            keys[CHAIN_BAD_KEYS[i][0]] = BAD_POINTS[CHAIN_BAD_KEYS[i][1]][0]
        ks = [(_scalar(f"k1/{i}/{j}"), _scalar(f"k2/{i}/{j}")) for j in range(len(sks))]
        c["sks"].append(sks), c["keys"].append(keys), c["secnonces"].append(ks)
        c["pubnonces"].append([(base_mul(k1), base_mul(k2)) for k1, k2 in ks])
    c["offsets"] = offsets_of(c["keys"])
    c["owner"] = np.array([i for i in range(n) for _ in c["keys"][i]], np.uint32)
    c["tweak_a"] = [b32(_scalar(f"ta/{i}")) for i in range(n)]
    c["tweak_b"] = [b32(_scalar(f"tb/{i}")) for i in range(n)]
    c["msg"] = [_stream(f"msg/{i}", 32) for i in range(n)]
    ka = [key_agg(k) for k in c["keys"]]
    ta = [apply_tweak(ka[i][1], c["tweak_a"][i], TWEAK_PLAIN) for i in range(n)]
    tb = [apply_tweak(ta[i][1], c["tweak_b"][i], TWEAK_XONLY) for i in range(n)]
    na = [nonce_agg(p) for p in c["pubnonces"]]
    se = [session(tb[i][1], na[i][1], c["msg"][i]) for i in range(n)]
    ps = [[partial_sign(k[0], k[1], d, tb[i][1], se[i][1]) for k, d in zip(c["secnonces"][i], c["sks"][i])] for i in range(n)]
    pv = [[partial_verify(ps[i][j][1], nonce_pack(*c["pubnonces"][i][j]), c["keys"][i][j], tb[i][1], se[i][1])
           for j in range(len(c["keys"][i]))] for i in range(n)]
    sa = [sig_agg([p[1] for p in ps[i]], tb[i][1], se[i][1]) for i in range(n)]
    c.update(key_agg=ka, tweak_plain=ta, tweak_xonly=tb, nonce_agg=na, session=se, partial_sign=ps, partial_verify=pv, sig_agg=sa)
    return c


def good_sessions(c):
    return [i for i in range(c["n"]) if i != CHAIN_EMPTY and i not in CHAIN_BAD_KEYS]


def flat(lists):
    return [v for sub in lists for v in sub]


def points_xy(points):
    return rows([le(p[0]) for p in points], 32), rows([le(p[1]) for p in points], 32)


# Each set is (inputs, want): dicts of arrays under the argument names of include/p2e.h, for the whole chain; cut() takes the
# first `count` elements of one.  `per`: what an element of the call is.
def key_agg_set(lists):
    """lists: per session a list of points"""
    x, y = points_xy(flat(lists))
    res = [key_agg(k) for k in lists]
    return (dict(pkx32=x, pky32=y, key_offsets=offsets_of(lists)),
            dict(keyagg192=rows([r[1] for r in res], 192), agg_pk32=rows([r[2] for r in res], 32), err=np.array([r[0] for r in res], np.uint8)))


def apply_tweak_set(recs, tweaks, mode):
    res = [apply_tweak(r, t, mode) for r, t in zip(recs, tweaks)]
    return (dict(keyagg192_in=rows(recs, 192), tweak32=None if tweaks[0] is None else rows(tweaks, 32), mode=mode),
            dict(keyagg192_out=rows([r[1] for r in res], 192), agg_pk32=rows([r[2] for r in res], 32), err=np.array([r[0] for r in res], np.uint8)))


def nonce_agg_set(lists):
    """lists: per session a list of (R_1, R_2)"""
    res = [nonce_agg(p) for p in lists]
    return (dict(pubnonce128=rows([nonce_pack(*p) for p in flat(lists)], 128), key_offsets=offsets_of(lists)),
            dict(aggnonce128=rows([r[1] for r in res], 128), err=np.array([r[0] for r in res], np.uint8)))


def session_set(recs, aggs, msgs):
    res = [session(r, a, m) for r, a, m in zip(recs, aggs, msgs)]
    return (dict(keyagg192=rows(recs, 192), aggnonce128=rows(aggs, 128), msg32=rows(msgs, 32)),
            dict(session128=rows([r[1] for r in res], 128), err=np.array([r[0] for r in res], np.uint8)))


def partial_sign_set(secnonces, sks, recs, sess):
    res = [partial_sign(k[0], k[1], d, r, s) for k, d, r, s in zip(secnonces, sks, recs, sess)]
    return (dict(secnonce64=rows([le(k[0]) + le(k[1]) for k in secnonces], 64), sk32=rows([le(d) for d in sks], 32),
                 keyagg192=rows(recs, 192), session128=rows(sess, 128)),
            dict(psig32=rows([r[1] for r in res], 32), err=np.array([r[0] for r in res], np.uint8)))


def partial_verify_set(psigs, pubnonces, keys, index, recs, sess):
    """index: per partial signature its session (None: the identity); recs / sess: the n_sessions records"""
    at = list(range(len(psigs))) if index is None else index
    res = [partial_verify(p, nonce_pack(*R), k, recs[a] if a < len(recs) else None, sess[a] if a < len(recs) else None)
           for p, R, k, a in zip(psigs, pubnonces, keys, at)]
    x, y = points_xy(keys)
    return (dict(psig32=rows(psigs, 32), pubnonce128=rows([nonce_pack(*R) for R in pubnonces], 128), pkx32=x, pky32=y,
                 session_index=None if index is None else np.array(index, np.uint32), keyagg192=rows(recs, 192),
                 session128=rows(sess, 128), n_sessions=len(recs)),
            dict(err=np.array([r[0] for r in res], np.uint8), valid=np.array([r[1] for r in res], np.uint8)))


def sig_agg_set(lists, recs, sess):
    """lists: per session a list of psig32"""
    res = [sig_agg(p, r, s) for p, r, s in zip(lists, recs, sess)]
    return (dict(psig32=rows(flat(lists), 32), key_offsets=offsets_of(lists), keyagg192=rows(recs, 192), session128=rows(sess, 128)),
            dict(sig64=rows([r[1] for r in res], 64), err=np.array([r[0] for r in res], np.uint8)))


# the calls: name -> (per-element inputs, per-signer inputs, whole inputs, outputs with their bytes per element)
CALLS = {
    "key_agg": ((), ("pkx32", "pky32"), (), (("keyagg192", 192), ("agg_pk32", 32), ("err", 1))),
    "apply_tweak": (("keyagg192_in", "tweak32"), (), ("mode",), (("keyagg192_out", 192), ("agg_pk32", 32), ("err", 1))),
    "nonce_agg": ((), ("pubnonce128",), (), (("aggnonce128", 128), ("err", 1))),
    "session": (("keyagg192", "aggnonce128", "msg32"), (), (), (("session128", 128), ("err", 1))),
    "partial_sign": (("secnonce64", "sk32", "keyagg192", "session128"), (), (), (("psig32", 32), ("err", 1))),
    "partial_verify": (("psig32", "pubnonce128", "pkx32", "pky32", "session_index"), (), ("keyagg192", "session128", "n_sessions"),
                       (("err", 1), ("valid", 1))),
    "sig_agg": (("keyagg192", "session128"), ("psig32",), (), (("sig64", 64), ("err", 1))),
}


def cut(call, inputs, want, count):
    """the first `count` elements of a set (per-signer arrays stay whole: the offsets say what is read)"""
    per_element, _per_signer, _whole, _outs = CALLS[call]
    ins = dict(inputs)
    for name in per_element:
        if ins[name] is not None:
            ins[name] = ins[name][:count]
    if "key_offsets" in ins:
        ins["key_offsets"] = ins["key_offsets"][:count + 1]
    return ins, {k: v[:count] for k, v in want.items()}


@functools.lru_cache(maxsize=None)
def chain_sets():
    """the seven calls over the chain, in the header's order; apply_tweak three times (plain, x-only, Taproot with a root)"""
    c = chain()
    n = c["n"]
    recs0, recs1, recs2 = ([r[1] for r in c[k]] for k in ("key_agg", "tweak_plain", "tweak_xonly"))
    aggs, sess = [r[1] for r in c["nonce_agg"]], [r[1] for r in c["session"]]
    sets = {
        "key_agg": key_agg_set(c["keys"]),
        "apply_tweak": apply_tweak_set(recs0, c["tweak_a"], TWEAK_PLAIN),
        "apply_tweak/xonly": apply_tweak_set(recs1, c["tweak_b"], TWEAK_XONLY),
        "apply_tweak/taproot": apply_tweak_set(recs0, c["msg"], TWEAK_TAPROOT),
        "nonce_agg": nonce_agg_set(c["pubnonces"]),
        "session": session_set(recs2, aggs, c["msg"]),
        # the caller is the LAST signer of each session (the empty one signs with a key of its own: its records are zero)
        "partial_sign": partial_sign_set([k[-1] if k else (1, 1) for k in c["secnonces"]], [d[-1] if d else 1 for d in c["sks"]], recs2, sess),
        "partial_verify": partial_verify_set([p[1] for p in flat(c["partial_sign"])], flat(c["pubnonces"]), flat(c["keys"]),
                                             [int(v) for v in c["owner"]], recs2, sess),
        "sig_agg": sig_agg_set([[p[1] for p in ps] for ps in c["partial_sign"]], recs2, sess),
    }
    assert len(sets["session"][1]["err"]) == n
    return sets


# ---- the special cases real inputs reach ----------------------------------------------------------------------------------------------
def aggregate_secret(c, i):
    """q with Q = q G for the untweaked aggregate key of session i of the chain"""
    L, pk2 = key_list(c["keys"][i])
    return sum(coefficient(L, pk2, cbytes(k)) * d for k, d in zip(c["keys"][i], c["sks"][i])) % N


def _session_with_parity(c, odd, stage="key_agg"):
    return next(i for i in good_sessions(c) if keyagg_parse(c[stage][i][1])[1]["Q"][1] & 1 == odd)


@functools.lru_cache(maxsize=None)
def special_sets():
    """name -> (call, inputs, want): small sets of the cases the header names, each reached with real inputs"""
    c = chain()
    K, K2 = base_mul(_scalar("special/K")), base_mul(_scalar("special/K2"))
    bad = {k: v[0] for k, v in BAD_POINTS.items()}
    out = {}
    # key aggregation: bad keys at both ends of a list, no key, 1024 and 1025 keys, reversed offsets
    lists = [[bad["neutral"]], [K, bad["off"]], [bad["range"], K], [], [K] * MAX_SIGNERS, [K2] * (MAX_SIGNERS + 1), [K, K2]]
    out["key_agg"] = ("key_agg",) + key_agg_set(lists)
    x, y = points_xy([K, K2, K])
    res = [key_agg([K, K2]), key_agg(None), key_agg([K2, K])]
    out["key_agg/reversed"] = ("key_agg", dict(pkx32=x, pky32=y, key_offsets=np.array([0, 2, 1, 3], np.uint64)),
                               dict(keyagg192=rows([r[1] for r in res], 192), agg_pk32=rows([r[2] for r in res], 32),
                                    err=np.array([r[0] for r in res], np.uint8)))
    # tweaks: the edge scalars in both modes, Q' at infinity in both modes, records that are refused
    even, odd = _session_with_parity(c, 0), _session_with_parity(c, 1)
    rec_even, rec_odd = c["key_agg"][even][1], c["key_agg"][odd][1]
    q_even, q_odd = aggregate_secret(c, even), aggregate_secret(c, odd)
    assert base_mul(q_odd) == keyagg_parse(rec_odd)[1]["Q"]
    bad_flag = rec_even[:160] + u32le(8) + bytes(28)
    big_tacc = rec_even[:64] + b32(N) + rec_even[96:]
    recs = [rec_even] * 4 + [rec_odd, rec_even, bytes(192), bad_flag, big_tacc]
    tweaks = [b32(t) for t in EDGE_SCALARS] + [b32(N - q_odd), b32(N - q_even)] + [b32(1)] * 3
    out["apply_tweak/plain"] = ("apply_tweak",) + apply_tweak_set(recs, tweaks, TWEAK_PLAIN)
    tweaks = [b32(t) for t in EDGE_SCALARS] + [b32(q_odd), b32(N - q_even)] + [b32(1)] * 3       # (t = n - g q: g = n - 1 where y(Q) is odd)
    out["apply_tweak/xonly"] = ("apply_tweak",) + apply_tweak_set(recs, tweaks, TWEAK_XONLY)
    out["apply_tweak/bip86"] = ("apply_tweak",) + apply_tweak_set([rec_even, rec_odd, bytes(192)], [None] * 3, TWEAK_TAPROOT)
    # nonces: a bad contribution in either half, sums that are the point at infinity in one half and in both, no signer
    R, S = base_mul(_scalar("special/R")), base_mul(_scalar("special/S"))
    lists = [[(bad["neutral"], R)], [(R, bad["off"])], [(bad["range"], R)], [(R, S), (point_neg(R), K)], [(K, S), (R, point_neg(S))],
             [(R, S), (point_neg(R), point_neg(S))], [], [(R, S)]]
    out["nonce_agg"] = ("nonce_agg",) + nonce_agg_set(lists)
    # sessions: R = G, one half at infinity, a half off the curve, a zeroed record
    rec = c["tweak_xonly"][even][1]
    aggs = [nonce_pack(None, None), nonce_pack(R, None), nonce_pack(None, S), nonce_pack(bad["off"], S), nonce_pack(R, bad["range"]), nonce_pack(R, S)]
    out["session"] = ("session",) + session_set([rec] * 5 + [bytes(192)], aggs, [c["msg"][0]] * 6)
    assert int.from_bytes(out["session"][2]["session128"][0, 64:96].tobytes(), "big") == G[0]
    # the signer: every secret at the edge scalars, a zeroed session
    i = good_sessions(c)[1]
    rec, ses, k, d = c["tweak_xonly"][i][1], c["session"][i][1], c["secnonces"][i][-1], c["sks"][i][-1]
    secs = [(v, k[1]) for v in EDGE_SCALARS] + [(k[0], v) for v in EDGE_SCALARS] + [k] * 5
    sks = [d] * 8 + list(EDGE_SCALARS) + [d]
    out["partial_sign"] = ("partial_sign",) + partial_sign_set(secs, sks, [rec] * 13, [ses] * 12 + [bytes(128)])
    # the verifier: the index, the edge scalars, a bad key, and the three ways a signature is NOT valid
    a, b = next(i for i in good_sessions(c) if len(c["keys"][i]) == 3), next(i for i in good_sessions(c) if len(c["keys"][i]) == 2)
    recs, sess = [c["tweak_xonly"][a][1], c["tweak_xonly"][b][1]], [c["session"][a][1], c["session"][b][1]]
    ps, pn, pk = c["partial_sign"][a][0][1], c["pubnonces"][a][0], c["keys"][a][0]
    flipped = bytes([ps[0]]) + ps[1:31] + bytes([ps[31] ^ 1])
    cases = [(ps, pn, pk, 0), (flipped, pn, pk, 0), (ps, c["pubnonces"][a][1], pk, 0), (ps, pn, pk, 1), (ps, pn, pk, 2), (ps, pn, pk, 2**32 - 1),
             (ps, pn, bad["neutral"], 0), (ps, (bad["off"], pn[1]), pk, 0)] + [(b32(v), pn, pk, 0) for v in EDGE_SCALARS] + \
            [(c["partial_sign"][b][1][1], c["pubnonces"][b][1], c["keys"][b][1], 1)]
    out["partial_verify"] = ("partial_verify",) + partial_verify_set([v[0] for v in cases], [v[1] for v in cases], [v[2] for v in cases],
                                                                     [v[3] for v in cases], recs, sess)
    assert out["partial_verify"][2]["valid"].tolist() == [1, 0, 0, 0] + [0] * 8 + [1]
    # the aggregation: partial signatures at the edge scalars, no signer
    rec, ses = c["tweak_xonly"][a][1], c["session"][a][1]
    lists = [[b32(0), b32(N - 1)], [b32(1), b32(N)], [b32(2**256 - 1)], [], [p[1] for p in c["partial_sign"][a]]]
    out["sig_agg"] = ("sig_agg",) + sig_agg_set(lists, [rec] * 5, [ses] * 5)
    return out


@functools.lru_cache(maxsize=None)
def forced_sets():
    """what no hash produces: coefficients that cancel (Q at infinity) and b with R_1 = -b R_2.  -> (key_agg arguments and
    results, session arguments and results)"""
    c = chain()
    K, K2 = base_mul(_scalar("special/K")), base_mul(_scalar("special/K2"))
    lists = [[K, K], [K, K2, K], [K, K2]]
    coefs = [[5, N - 5], [7, 0, N - 7], [1, 3]]
    res = [key_agg(k, coefs=a) for k, a in zip(lists, coefs)]
    x, y = points_xy(flat(lists))
    want_q = [keyagg_parse(r[1])[1]["Q"] if not r[0] else (0, 0) for r in res]
    ka = (dict(pkx32=x, pky32=y, coef32=rows([b32(v) for v in flat(coefs)], 32), key_offsets=offsets_of(lists)),
          dict(code=np.array([r[0] for r in res], np.uint8), qx32=rows([le(q[0]) for q in want_q], 32), qy32=rows([le(q[1]) for q in want_q], 32)))
    i = good_sessions(c)[0]
    rec, msg = c["tweak_xonly"][i][1], c["msg"][i]
    r2 = _scalar("forced/r2")
    bs = [3, N - 3, 1, 0]
    aggs = [nonce_pack(point_neg(base_mul(3 * r2)), base_mul(r2)), nonce_pack(base_mul(3 * r2), base_mul(r2)),
            nonce_pack(base_mul(r2), base_mul(r2)), nonce_pack(None, base_mul(r2))]
    res = [session(rec, a, msg, b=b) for a, b in zip(aggs, bs)]
    se = (dict(keyagg192=rows([rec] * 4, 192), aggnonce128=rows(aggs, 128), msg32=rows([msg] * 4, 32), b32=rows([b32(b) for b in bs], 32)),
          dict(code=np.array([r[0] for r in res], np.uint8), session128=rows([r[1] for r in res], 128)))
    assert all(int.from_bytes(r[1][64:96], "big") == G[0] for r in (res[0], res[1], res[3])) and res[2][1][64:96] != b32(G[0])
    return ka, se


# ---- running a call (the CPU emulation's functions and the library's take the header's arguments in the header's order) -----------------
ORDER = {
    "key_agg": ("pkx32", "pky32", "key_offsets", "keyagg192", "agg_pk32", "count", "err"),
    "apply_tweak": ("keyagg192_in", "tweak32", "mode", "keyagg192_out", "agg_pk32", "count", "err"),
    "nonce_agg": ("pubnonce128", "key_offsets", "aggnonce128", "count", "err"),
    "session": ("keyagg192", "aggnonce128", "msg32", "session128", "count", "err"),
    "partial_sign": ("secnonce64", "sk32", "keyagg192", "session128", "psig32", "count", "err"),
    "partial_verify": ("psig32", "pubnonce128", "pkx32", "pky32", "session_index", "keyagg192", "session128", "n_sessions", "count", "err", "valid"),
    "sig_agg": ("psig32", "key_offsets", "keyagg192", "session128", "sig64", "count", "err"),
}


def invoke(fn, call, inputs, count, ctx=None):
    """fn(ctx?, arguments..) on the first `count` elements.  Every output is pre-filled with 0xAA and one element longer than the
    call may write.  -> (return value, outputs)"""
    import ctypes as C
    outs = {name: np.full((count + 1, width), 0xAA, np.uint8) for name, width in CALLS[call][3]}
    args = [] if ctx is None else [ctx]
    keep = []
    for name in ORDER[call]:
        if name in outs:
            args.append(outs[name].ctypes.data_as(C.c_void_p))
        elif name == "count":
            args.append(C.c_size_t(count))
        elif name == "n_sessions":
            args.append(C.c_size_t(inputs[name]))
        elif name == "mode":
            args.append(C.c_int(inputs[name]))
        elif inputs[name] is None:
            args.append(None)
        else:
            keep.append(np.ascontiguousarray(inputs[name]))
            args.append(keep[-1].ctypes.data_as(C.c_void_p))
    fn.restype = C.c_long
    return fn(*args), outs


def assert_matches(call, rc, outs, want, count):
    """every byte of the first `count` elements, the return value, the untouched element behind them, zeros where flagged"""
    err = outs["err"][:count, 0]
    diff = np.nonzero(err != want["err"][:count])[0]
    assert diff.size == 0, (call, [(int(i), int(err[i]), int(want["err"][i])) for i in diff[:8]])
    assert rc == np.count_nonzero(want["err"][:count]), (call, rc)
    for name, width in CALLS[call][3]:
        got, ref = outs[name], want[name][:count].reshape(count, width)
        bad = np.nonzero((got[:count] != ref).any(axis=1))[0]
        assert bad.size == 0, (call, name, [int(i) for i in bad[:8]])
        assert (got[count] == 0xAA).all(), (call, name)
        if name != "err":
            assert not got[:count][want["err"][:count] != 0].any(), (call, name)
