"""Silent payments (BIP-352): input hashes, labels, the sender's output keys and the receiver's scan loop, restated from
include/p2e.h's definitions in Python integers and hashlib: the oracle of tests/test_sp_cpu.py and tests/test_gpu_sp.py, and the
input sets both run.  Nothing here uses the code under test; the curve helpers are tests/schnorr_inputs.py's.

Wire forms: points and secret keys are 32-byte little-endian values, outpoints, input hashes, x-only outputs and tweaks the
standard's big-endian strings.  Error bytes are include/p2e.h's P2E_WIRE_* codes, the first failing check in the header's
order; a flagged element is all zeros.

There are no published vectors here.  What pins the oracle instead (tests/test_sp_cpu.py):
  (a) sender = receiver: every payment of the sets is made through a B_scan and found through b_scan A, two different
      scalar multiplications that meet only if both are right;
  (b) the three tag midstates from hashlib;
  (c) x((b_spend + t_k + l_j) G) equals the matched output.
"""
import functools
import hashlib

import numpy as np

import schnorr_inputs as SI
from schnorr_inputs import N, P, b32, base_mul, tag_midstate, tagged_hash  # noqa: F401

WIRE_OK, WIRE_BAD_LENGTH, WIRE_COORD_RANGE, WIRE_NOT_ON_CURVE, WIRE_INFINITY, WIRE_SCALAR_RANGE = 0, 1, 3, 4, 5, 8
TAGS = ("BIP0352/Inputs", "BIP0352/SharedSecret", "BIP0352/Label")
MAX_HITS, MAX_LABELS = 8, 16
COUNTS = (0, 1, 63, 64, 65, 257)     # array lengths every per-element test runs: empty, one lane, a wave, a block's tail
N_SET = 257


# ---- BIP-352, from the header's definitions ------------------------------------------------------------------------------------
def point_code(pt):
    """the checks of a point that must not be neutral, in the header's order"""
    x, y = pt
    if x == 0 and y == 0:
        return WIRE_INFINITY
    if x >= P or y >= P:
        return WIRE_COORD_RANGE
    return WIRE_OK if (y * y - x * x * x - 7) % P == 0 else WIRE_NOT_ON_CURVE


def scalar_code(v):
    return WIRE_OK if 0 < v < N else WIRE_SCALAR_RANGE


def ser_p(pt):
    return bytes([2 | (pt[1] & 1)]) + b32(pt[0])


def point_mul(k, pt):
    """k pt for an affine point, or None"""
    return SI._affine(SI._jmul(k % N, pt))


def point_add(a, b):
    """a + b for affine points (None: the neutral element)"""
    ja = None if a is None else (a[0], a[1], 1)
    jb = None if b is None else (b[0], b[1], 1)
    return SI._affine(SI._jadd(ja, jb))


def input_hash(outpoint, A):
    """(code, input_hash32)"""
    code = point_code(A)
    if code:
        return code, bytes(32)
    h = tagged_hash(TAGS[0], outpoint + ser_p(A))
    return (WIRE_SCALAR_RANGE, bytes(32)) if scalar_code(int.from_bytes(h, "big")) else (WIRE_OK, h)


def label(b_scan, m):
    """(code, label_tweak32, L_m or None)"""
    if scalar_code(b_scan):
        return WIRE_SCALAR_RANGE, bytes(32), None
    l = int.from_bytes(tagged_hash(TAGS[2], b32(b_scan) + m.to_bytes(4, "big")), "big")
    if scalar_code(l):
        return WIRE_SCALAR_RANGE, bytes(32), None
    return WIRE_OK, b32(l), base_mul(l)


def tweak(S, k):
    """t_k as an integer"""
    return int.from_bytes(tagged_hash(TAGS[1], ser_p(S) + k.to_bytes(4, "big")), "big")


def output_point(B_spend, t):
    """(code, P_k = B_spend + t G) for ANY 256-bit t"""
    if scalar_code(t):
        return WIRE_SCALAR_RANGE, None
    Pk = point_add(base_mul(t), B_spend)
    return (WIRE_INFINITY, None) if Pk is None else (WIRE_OK, Pk)


def finish_send(B_spend, t):
    code, Pk = output_point(B_spend, t)
    return (code, bytes(32)) if code else (WIRE_OK, b32(Pk[0]))


def send(a, ih, B_scan, B_spend, k):
    """(code, out_pk32): a and ih integers"""
    code = scalar_code(a) or scalar_code(ih) or point_code(B_scan) or point_code(B_spend)
    if code:
        return code, bytes(32)
    return finish_send(B_spend, tweak(point_mul(ih * a % N, B_scan), k))


def finish(B_spend, labels, t, outputs, taken):
    """one step of the scan loop behind t: (code, (output index, label) or None).  The candidates are P_k, then P_k + L_j; the
    hit is the lowest-index output not in `taken` that matches a candidate, under its first matching candidate."""
    code, Pk = output_point(B_spend, t)
    if code:
        return code, None
    cands = [Pk] + [point_add(Pk, L) for L in labels]
    for idx, o in enumerate(outputs):
        if idx in taken:
            continue
        v = int.from_bytes(o, "big")
        for c, C in enumerate(cands):
            if C is not None and C[0] == v:            # (an output >= p equals no abscissa)
                return WIRE_OK, (idx, c)
    return WIRE_OK, None


def shared_code(b_scan, B_spend, labels):
    code = scalar_code(b_scan) or point_code(B_spend)
    for L in labels:
        code = code or point_code(L)
    return code


def scan(b_scan, B_spend, labels, A, ih, outputs, max_hits, S=None):
    """(code, [(output index, label, t32)]); ih None: the scalar is b_scan alone; outputs None: reversed or too many offsets.
    S: the shared secret where the caller has it already (it is checked against nothing: a cache)"""
    code = shared_code(b_scan, B_spend, labels) or point_code(A) or (ih is not None and scalar_code(ih)) or 0
    if not code and outputs is None:
        code = WIRE_BAD_LENGTH
    if code:
        return code, []
    S = S or point_mul(b_scan if ih is None else ih * b_scan % N, A)
    hits = []
    while len(hits) < max_hits:
        t = tweak(S, len(hits))
        code, hit = finish(B_spend, labels, t, outputs, {h[0] for h in hits})
        if code:
            return code, []
        if hit is None:
            break
        hits.append((hit[0], hit[1], b32(t)))
    return WIRE_OK, hits


# ---- input sets (deterministic) --------------------------------------------------------------------------------------------------
def _stream(label_, nbytes):
    out, k = b"", 0
    while len(out) < nbytes:
        out += hashlib.sha256(b"sp inputs/" + label_.encode() + k.to_bytes(4, "big")).digest()
        k += 1
    return out[:nbytes]


def _scalar(label_):
    return int.from_bytes(_stream(label_, 32), "big") % (N - 1) + 1


def _shuffled(label_, items):
    keys = _stream(label_, 4 * len(items))
    return [v for _k, v in sorted((keys[4 * j:4 * j + 4], v) for j, v in enumerate(items))]


def le_rows(values):
    return np.frombuffer(b"".join(v.to_bytes(32, "little") for v in values), np.uint8).reshape(-1, 32).copy() if values else np.zeros((0, 32), np.uint8)


def be_rows(list_of_bytes, width=32):
    return np.frombuffer(b"".join(list_of_bytes), np.uint8).reshape(-1, width).copy() if list_of_bytes else np.zeros((0, width), np.uint8)


def _off_curve():
    x = 5
    while SI.lift_x(x) is not None:
        x += 1
    return x, 1


B_SCAN_SK, B_SPEND_SK = _scalar("b_scan"), _scalar("b_spend")
B_SCAN, B_SPEND = base_mul(B_SCAN_SK), base_mul(B_SPEND_SK)


@functools.lru_cache(maxsize=None)
def labels_all():
    """the 16 labels of the receiver: [(l_m, L_m)] for m = 0 .. 15"""
    out = []
    for m in range(MAX_LABELS):
        code, l, L = label(B_SCAN_SK, m)
        assert code == 0
        out.append((int.from_bytes(l, "big"), L))
    return out


# what a transaction of the sets is: (number of outputs, [label of payment k or None], specials)
KINDS = (
    dict(n_out=5, pays=[None, None, None]),                       # 0: three hits        (the first wave holds 0, 1 and 2 side by side)
    dict(n_out=0, pays=[]),                                       # 1: no outputs
    dict(n_out=40, pays=[]),                                      # 2: forty decoys
    dict(n_out=1, pays=[]),
    dict(n_out=1, pays=[None]),
    dict(n_out=2, pays=[]),
    dict(n_out=2, pays=[None]),
    dict(n_out=2, pays=[None, None]),
    dict(n_out=40, pays=[None, 0, 3]),                            # labelled payments: label 0 (found with n_labels = 1) and label 3
    dict(n_out=4, pays=[0]),
    dict(n_out=4, pays=[15, None]),
    dict(n_out=6, pays=[None, 7], duplicate=True),                # a copy of the paying output of k = 0 at another index
    dict(n_out=3, pays=[], decoy_p1=True),                        # x(P_1) present, x(P_0) not: no hit
    dict(n_out=4, pays=[None], above_p=True),                     # outputs >= p among the others
    dict(n_out=12, pays=[None] * 9),                              # more payments than any max_hits
    dict(n_out=3, pays=[1, 2]),
)
# elements with a code of their own (index in the set -> what is wrong); OFFSET_PAIR: out_offsets[r + 1] < out_offsets[r]
BAD_A = {20: "neutral", 37: "range_x", 52: "off_curve", 66: "range_y"}
BAD_HASH = {23: 0, 70: N, 71: 2**256 - 1}
OFFSET_PAIR = 41


@functools.lru_cache(maxsize=None)
def transactions(n=N_SET):
    """The sender's side of the sets, once: per element the input key a, A = a G, the outpoint, the input hash, the outputs and
    the payments planted in them [(output index, k, label or None)], and S computed the RECEIVER's way."""
    L = labels_all()
    txs = []
    for i in range(n):
        kind = KINDS[i % len(KINDS)]
        a = _scalar(f"a{i}")
        A = base_mul(a)
        outpoint = _stream(f"outpoint{i}", 36)
        if i in BAD_A:
            A = {"neutral": (0, 0), "range_x": (P + 1, A[1]), "off_curve": _off_curve(), "range_y": (A[0], P)}[BAD_A[i]]
        code, ih = input_hash(outpoint, A)
        ih_int = int.from_bytes(ih, "big")
        n_out, pays = kind["n_out"], kind["pays"]
        if i in (OFFSET_PAIR, OFFSET_PAIR + 1):
            n_out, pays = 0, []
        outputs = [_stream(f"decoy{i}/{j}", 32) for j in range(n_out)]
        if kind.get("above_p") and n_out:
            outputs[0], outputs[2] = b32(P), b32(2**256 - 1)
        planted = []
        S_send = None
        if not code:
            S_send = point_mul(ih_int * a % N, B_SCAN)                 # the sender's route: (input_hash a) B_scan
            slots = _shuffled(f"slots{i}", [j for j in range(n_out) if not (kind.get("above_p") and j in (0, 2))])
            for k, lab in enumerate(pays):
                B_m = B_SPEND if lab is None else point_add(B_SPEND, L[lab][1])
                c, out = finish_send(B_m, tweak(S_send, k))
                assert c == 0
                outputs[slots[k]] = out
                planted.append((slots[k], k, lab))
            if kind.get("duplicate"):
                free = [j for j in range(n_out) if j not in [p[0] for p in planted]]
                outputs[free[0]] = outputs[planted[0][0]]
                planted[0] = (min(free[0], planted[0][0]), 0, pays[0])      # the lower of the two is the hit, the other is no second one
            if kind.get("decoy_p1"):
                outputs[1] = finish_send(B_SPEND, tweak(S_send, 1))[1]
        txs.append(dict(a=a, A=A, outpoint=outpoint, ih=ih_int, code=code, outputs=outputs, planted=planted, S_send=S_send))
    return txs


@functools.lru_cache(maxsize=None)
def base_arrays(n=N_SET, huge=False):
    """The arrays every scan of the sets reads.  out_offsets[OFFSET_PAIR + 1] is one BELOW its neighbour (`huge`: 2^32 above,
    for runs that stage nothing): element OFFSET_PAIR is WIRE_BAD_LENGTH either way, element OFFSET_PAIR + 1 reads the
    last output of the transaction in front of the pair (or is WIRE_BAD_LENGTH too)."""
    txs = transactions(n)
    flat, offs = [], [0]
    for t in txs:
        flat += t["outputs"]
        offs.append(len(flat))
    if n > OFFSET_PAIR + 1:
        offs[OFFSET_PAIR + 1] = offs[OFFSET_PAIR] + (1 << 32) if huge else offs[OFFSET_PAIR] - 1
    ih = [b32(BAD_HASH.get(i, t["ih"])) for i, t in enumerate(txs)]
    tweaked = []                                                           # input_hash A, for the scans without input_hash32
    for i, t in enumerate(txs):
        tweaked.append(point_mul(t["ih"], t["A"]) if not t["code"] else t["A"])
    return dict(ax=le_rows([t["A"][0] for t in txs]), ay=le_rows([t["A"][1] for t in txs]), outpoint=be_rows([t["outpoint"] for t in txs], 36),
                input_hash=be_rows(ih), tax=le_rows([p[0] for p in tweaked]), tay=le_rows([p[1] for p in tweaked]),
                outputs=be_rows(flat + [bytes(32)]), out_offsets=np.array(offs, np.uint64),
                input_hash_good=be_rows([b32(t["ih"]) for t in txs]), input_hash_err=np.array([t["code"] for t in txs], np.uint8))


@functools.lru_cache(maxsize=None)
def _receiver_secret(i, with_hash, n):
    """S of element i computed the RECEIVER's way from the arrays' own values, or None where a check fails first"""
    t = transactions(n)[i]
    if t["code"]:
        return None
    if with_hash:
        ih = BAD_HASH.get(i, t["ih"])
        return None if scalar_code(ih) else point_mul(ih * B_SCAN_SK % N, t["A"])
    return point_mul(B_SCAN_SK, point_mul(t["ih"], t["A"]))


def shared_args(n_labels, bad=None):
    """(scan_sk (1, 32), spend_pkx, spend_pky (1, 32), label_x, label_y (n_labels, 32)) little-endian, and the same as integers;
    `bad`: one of SHARED_BAD, the argument that is wrong"""
    b, B = B_SCAN_SK, B_SPEND
    Ls = [L for _l, L in labels_all()[:n_labels]]
    if bad == "scan_zero":
        b = 0
    elif bad == "scan_n":
        b = N
    elif bad == "spend_neutral":
        B = (0, 0)
    elif bad == "spend_range":
        B = (B[0], P + 2)
    elif bad == "spend_off_curve":
        B = _off_curve()
    elif bad == "label_off_curve":
        Ls[-1] = (Ls[-1][0], Ls[-1][1] ^ 1)
    elif bad == "label_neutral":
        Ls[0] = (0, 0)
    arrays = (le_rows([b]), le_rows([B[0]]), le_rows([B[1]]), le_rows([L[0] for L in Ls]), le_rows([L[1] for L in Ls]))
    return arrays, (b, B, Ls)


SHARED_BAD = {"scan_zero": WIRE_SCALAR_RANGE, "scan_n": WIRE_SCALAR_RANGE, "spend_neutral": WIRE_INFINITY, "spend_range": WIRE_COORD_RANGE,
              "spend_off_curve": WIRE_NOT_ON_CURVE, "label_off_curve": WIRE_NOT_ON_CURVE, "label_neutral": WIRE_INFINITY}


@functools.lru_cache(maxsize=None)
def scan_set(max_hits=2, n_labels=1, with_hash=True, n=N_SET, huge=False, bad=None):
    """The scan's arguments and the oracle's outputs for the first n transactions.  with_hash False: ax, ay are input_hash A and
    input_hash32 is absent.  Shared: callers copy what they hand to the code under test."""
    B = base_arrays(N_SET, huge)
    (sk, spx, spy, lx, ly), (b, Bsp, Ls) = shared_args(n_labels, bad)
    ax, ay = (B["ax"], B["ay"]) if with_hash else (B["tax"], B["tay"])
    offs, flat = B["out_offsets"], B["outputs"]
    n_hits, hit_output = np.zeros(n, np.uint8), np.zeros((n, max_hits), np.uint32)
    hit_label, hit_tweak, err = np.zeros((n, max_hits), np.uint8), np.zeros((n, max_hits, 32), np.uint8), np.zeros(n, np.uint8)
    for i in range(n):
        A = (int.from_bytes(ax[i].tobytes(), "little"), int.from_bytes(ay[i].tobytes(), "little"))
        ih = int.from_bytes(B["input_hash"][i].tobytes(), "big") if with_hash else None
        lo, hi = int(offs[i]), int(offs[i + 1])
        outputs = None if hi < lo or hi - lo > 2**32 - 1 else [flat[j].tobytes() for j in range(lo, hi)]
        code, hits = scan(b, Bsp, Ls, A, ih, outputs, max_hits, S=None if bad else _receiver_secret(i, with_hash, N_SET))
        err[i], n_hits[i] = code, len(hits)
        for h, (idx, lab, t) in enumerate(hits):
            hit_output[i, h], hit_label[i, h], hit_tweak[i, h] = idx, lab, np.frombuffer(t, np.uint8)
    return dict(scan_sk=sk, spend_pkx=spx, spend_pky=spy, label_x=lx, label_y=ly, n_labels=n_labels, ax=ax[:max(n, 1)], ay=ay[:max(n, 1)],
                input_hash=B["input_hash"][:max(n, 1)] if with_hash else None, outputs=flat, out_offsets=offs[:n + 1], max_hits=max_hits,
                n_hits=n_hits, hit_output=hit_output, hit_label=hit_label, hit_tweak=hit_tweak, err=err)


@functools.lru_cache(maxsize=None)
def input_hash_set(n=N_SET):
    B = base_arrays(N_SET)
    return dict(outpoint=B["outpoint"][:n], ax=B["ax"][:n], ay=B["ay"][:n], input_hash=B["input_hash_good"][:n], err=B["input_hash_err"][:n])


LABEL_INDEX_EDGES = (0, 1, 2, 15, 255, 256, 2**31, 2**32 - 1)


@functools.lru_cache(maxsize=None)
def label_set(n=N_SET, bad_key=None):
    """label indices (the edges first, then a stream) under the receiver's scan key, or under a key that is refused"""
    idx = [LABEL_INDEX_EDGES[i] if i < len(LABEL_INDEX_EDGES) else int.from_bytes(_stream(f"label index{i}", 4), "big") for i in range(n)]
    b = B_SCAN_SK if bad_key is None else bad_key
    res = [label(b, m) for m in idx]
    return dict(scan_sk=le_rows([b]), index=np.array(idx, np.uint32), tweak=be_rows([r[1] for r in res]),
                x=le_rows([r[2][0] if r[2] else 0 for r in res]), y=le_rows([r[2][1] if r[2] else 0 for r in res]),
                err=np.array([r[0] for r in res], np.uint8))


# the sender's set: element i pays k = i % 3 (edge values of k further on) to a spend key that is labelled on every second element;
# one element for each code
SEND_BAD = {5: ("a", 0), 6: ("a", N), 7: ("ih", 0), 8: ("ih", N + 1), 9: ("scan", (0, 0)), 10: ("scan", (P, 1)), 11: ("scan", "off"),
            12: ("spend", (0, 0)), 13: ("spend", (3, P + 5)), 14: ("spend", "off")}
SEND_K_EDGES = {15: 255, 16: 256, 17: 2**31, 18: 2**32 - 1}


@functools.lru_cache(maxsize=None)
def send_set(n=N_SET):
    txs, L = transactions(N_SET), labels_all()
    a, ih, scan_pk, spend_pk, ks, out, err = [], [], [], [], [], [], []
    for i in range(n):
        t = txs[i if not txs[i]["code"] else 0]
        v = dict(a=t["a"], ih=t["ih"], scan=B_SCAN, spend=B_SPEND if i % 2 else point_add(B_SPEND, L[i % 16][1]))
        if i in SEND_BAD:
            which, val = SEND_BAD[i]
            v[which] = _off_curve() if val == "off" else val
        k = SEND_K_EDGES.get(i, i % 3)
        code, o = send(v["a"], v["ih"], v["scan"], v["spend"], k)
        a.append(v["a"]), ih.append(b32(v["ih"])), scan_pk.append(v["scan"]), spend_pk.append(v["spend"]), ks.append(k), out.append(o), err.append(code)
    return dict(a=le_rows(a), input_hash=be_rows(ih), scan_pkx=le_rows([p[0] for p in scan_pk]), scan_pky=le_rows([p[1] for p in scan_pk]),
                spend_pkx=le_rows([p[0] for p in spend_pk]), spend_pky=le_rows([p[1] for p in spend_pk]), k=np.array(ks, np.uint32),
                out=be_rows(out), err=np.array(err, np.uint8))


# ---- behind the hash: values of t no hash produces ---------------------------------------------------------------------------------
FORCED_LABELS, FORCED_OUTPUTS = 2, 3


@functools.lru_cache(maxsize=None)
def forced_finish():
    """[(B_spend, [L_0, L_1], t32, [3 outputs], code, found, output index, label)] for sp_finish with a forced t: t >= n, t = 0,
    t G = B_spend (the doubling), t G = -B_spend (neutral), P_k + L_0 neutral (no match, no flag; L_1 still matches),
    L_0 = P_k (the doubling inside a candidate), and two plain rows (a hit without a label, no hit at all)."""
    neg = lambda pt: (pt[0], P - pt[1])
    L = [labels_all()[0][1], labels_all()[1][1]]
    decoys = [_stream(f"forced decoy{j}", 32) for j in range(3)]
    t = _scalar("forced t")
    tG = base_mul(t)
    Pk = point_add(tG, B_SPEND)
    rows = []

    def row(B, labels, tv, outputs):
        code, hit = finish(B, labels, tv, outputs, set())
        rows.append((B, labels, b32(tv), outputs, code, int(hit is not None), hit[0] if hit else 0, hit[1] if hit else 0))
    row(B_SPEND, L, N, decoys)
    row(B_SPEND, L, 2**256 - 1, decoys)
    row(B_SPEND, L, 0, decoys)
    row(tG, L, t, [decoys[0], b32(point_add(tG, tG)[0]), decoys[2]])                              # the doubling
    row(neg(tG), L, t, decoys)                                                                    # the neutral element
    row(B_SPEND, [neg(Pk), L[1]], t, [decoys[0], decoys[1], b32(point_add(Pk, L[1])[0])])         # P_k + L_0 neutral, L_1 matches
    row(B_SPEND, [neg(Pk), L[1]], t, decoys)                                                      # ... and nothing matches
    row(B_SPEND, [Pk, L[1]], t, [b32(point_add(Pk, Pk)[0]), decoys[1], decoys[2]])                # L_0 = P_k
    row(B_SPEND, L, t, [decoys[0], decoys[1], b32(Pk[0])])
    row(B_SPEND, L, t, decoys)
    row(B_SPEND, L, t, [b32(point_add(Pk, L[1])[0]), b32(Pk[0]), b32(point_add(Pk, L[0])[0])])    # the lowest output wins, not the first candidate
    row(B_SPEND, L, t, [b32(2**256 - 1), b32(P), decoys[2]])                                      # outputs >= p are passed over
    assert [r[4] for r in rows[:5]] == [WIRE_SCALAR_RANGE] * 3 + [WIRE_OK, WIRE_INFINITY]
    assert [(r[5], r[6], r[7]) for r in rows[3:]] == [(1, 1, 0), (0, 0, 0), (1, 2, 2), (0, 0, 0), (1, 0, 1), (1, 2, 0), (0, 0, 0), (1, 0, 2), (0, 0, 0)]
    return tuple(rows)


def forced_arrays(rows):
    """the rows as the arrays of tests/emu_sp's emusp_finish and tests/probe_sp's probesp_finish"""
    return dict(bx=le_rows([r[0][0] for r in rows]), by=le_rows([r[0][1] for r in rows]),
                lx=le_rows([L[0] for r in rows for L in r[1]]), ly=le_rows([L[1] for r in rows for L in r[1]]),
                t=be_rows([r[2] for r in rows]), outputs=be_rows([o for r in rows for o in r[3]]),
                code=np.array([r[4] for r in rows], np.uint8), found=np.array([r[5] for r in rows], np.uint8),
                hit_output=np.array([r[6] for r in rows], np.uint32), hit_label=np.array([r[7] for r in rows], np.uint8))
