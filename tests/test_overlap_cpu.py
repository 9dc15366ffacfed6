"""BUFFER OVERLAP (include/p2e.h) without a GPU: the rule itself, and its use by every per-element entry point.

1. csrc/overlap.hpp alone.  tests/emu_overlap/overlap_selftest (a stand-alone program built with the address and
   undefined-behaviour sanitizers, built on demand) classifies span lists this file writes; the expectations are a
   restatement of the contract in Python integers (`classify` below), which shares nothing with the C++.
2. The entry points, through p2e.lib().  No context can be made without a device, so a handle that is never dereferenced
   stands in for one (as in tests/test_compact_passes_cpu.py): every refusal below must come before the first read of the
   context.  A call that gets PAST the overlap check meets the null-context test right behind it, so with a null context
   "null context" in p2e_last_error() is the proof that the arguments were accepted.
   The list of calls is derived from the header's declarations: a per-element call added later fails
   test_every_per_element_call_of_the_header_has_a_span_table until it has a row in CALLS."""
import ctypes as C
import itertools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import plonky2_ecdsa_amd as p2e
from test_ffi_surface import HEADER, _strip_c_comments

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "emu_overlap")
TOP = 1 << 64


# ---- 1. the rule, against Python integers ------------------------------------------------------------------------------------
def classify(spans):
    """spans: (ptr, bytes_per_element, count, is_output, broadcast).  -> (bad, a, b), the first refused pair in list order."""
    live = lambda s: s[0] != 0 and s[1] != 0 and s[2] != 0
    end = lambda s: s[0] + s[1] * s[2]
    for i, a in enumerate(spans):
        if not live(a):
            continue
        if end(a) >= TOP:                                   # the end wraps: no byte range at all
            return (1, i, i)
        for j in range(i + 1, len(spans)):
            b = spans[j]
            if not live(b) or not (a[3] or b[3]) or end(b) >= TOP:
                continue
            if max(a[0], b[0]) >= min(end(a), end(b)):      # no common byte (adjacent included)
                continue
            in_place = a[3] != b[3] and a[0] == b[0] and a[1] == b[1] and a[2] == b[2] and not (a[4] or b[4])
            if not in_place:
                return (1, i, j)
    return (0, -1, -1)


def span_pairs():
    """(name, x, y) with x, y = (ptr, bytes_per_element, count): the geometric cases of the contract."""
    base = 0x7000_0000_1000
    yield "disjoint", (base, 32, 8), (base + 4096, 32, 8)
    yield "adjacent", (base, 32, 8), (base + 256, 32, 8)
    yield "adjacent bytes", (base, 1, 8), (base + 8, 1, 8)
    yield "one byte shared", (base, 32, 8), (base + 255, 32, 8)
    yield "one byte shared, bytes", (base, 1, 8), (base + 7, 1, 8)
    yield "shifted by one element", (base, 32, 8), (base + 32, 32, 8)
    yield "contained", (base, 32, 8), (base + 64, 32, 2)
    yield "contained, one element at the start", (base, 32, 8), (base, 32, 1)
    yield "contained, one byte", (base, 32, 8), (base + 100, 1, 1)
    yield "identical", (base, 32, 8), (base, 32, 8)
    yield "identical bytes", (base, 1, 8), (base, 1, 8)
    yield "identical range, different stride", (base, 32, 8), (base, 64, 4)
    yield "same base, different stride", (base, 64, 8), (base, 32, 8)
    yield "same base, different count", (base, 32, 8), (base, 32, 7)
    yield "zero count inside", (base, 32, 8), (base + 32, 32, 0)
    yield "zero element size inside", (base, 32, 8), (base + 32, 0, 8)
    yield "null beside a span at address 0's neighbourhood", (32, 32, 8), (0, 32, 8)
    yield "wrapping end", (base, 32, 8), (TOP - 64, 32, 8)
    yield "end exactly at the top", (base, 32, 8), (TOP - 256, 32, 8)
    yield "last byte below the top", (base, 32, 8), (TOP - 257, 32, 8)
    yield "count * size overflows", (base, 32, 8), (base + 4096, 1 << 40, 1 << 40)
    yield "both at the top, overlapping", (TOP - 513, 32, 8), (TOP - 300, 1, 43)


def span_lists():
    filler = [(0x1000, 32, 8, 0, 0), (0x5000_0000, 1, 8, 1, 0)]          # an input and an output far from everything
    for _name, x, y in span_pairs():
        for first, second in ((x, y), (y, x)):
            for out1, out2, bc1, bc2 in itertools.product((0, 1), (0, 1), (0, 1), (0, 1)):
                if (out1 and bc1) or (out2 and bc2):                     # only an input is ever broadcast
                    continue
                pair = [first + (out1, bc1), second + (out2, bc2)]
                yield pair
                for p, q in itertools.permutations(range(4), 2):         # every position of a four-span list
                    lst, rest = [None] * 4, iter(filler)
                    lst[p], lst[q] = pair[0], pair[1]
                    yield [s if s is not None else next(rest) for s in lst]
    yield []
    yield [(0x1000, 32, 8, 1, 0)]
    yield [(TOP - 64, 32, 8, 0, 0)]                                       # a lone input whose end wraps is refused too
    # three clashes in one list: the first pair in list order is the one reported
    yield [(0x1000, 32, 8, 1, 0), (0x1000, 32, 8, 1, 0), (0x1000, 32, 8, 1, 0)]
    yield [(0x1000, 32, 8, 0, 0), (0x1000, 32, 8, 0, 0), (0x1020, 32, 8, 1, 0)]


def test_the_python_restatement_says_what_the_contract_says():
    base = 0x1000
    o, i, b = (1, 0), (0, 0), (0, 1)
    assert classify([(base, 32, 8) + i, (base, 32, 8) + o]) == (0, -1, -1)            # exactly in place
    assert classify([(base, 32, 8) + o, (base, 32, 8) + i]) == (0, -1, -1)
    assert classify([(base, 32, 8) + o, (base, 32, 8) + o]) == (1, 0, 1)              # two outputs
    assert classify([(base, 32, 8) + i, (base, 32, 8) + i]) == (0, -1, -1)            # two inputs
    assert classify([(base, 32, 1) + b, (base, 32, 1) + o]) == (1, 0, 1)              # a broadcast input
    assert classify([(base, 32, 8) + i, (base + 32, 32, 8) + o]) == (1, 0, 1)         # shifted
    assert classify([(base, 32, 8) + i, (base + 256, 32, 8) + o]) == (0, -1, -1)      # adjacent
    assert classify([(base, 32, 8) + i, (base, 64, 4) + o]) == (1, 0, 1)              # another stride
    assert classify([(base, 32, 8) + i, (base + 32, 32, 0) + o]) == (0, -1, -1)       # zero count
    assert classify([(0, 32, 8) + i, (0, 32, 8) + o]) == (0, -1, -1)                  # null
    assert classify([(base, 32, 8) + i, (TOP - 256, 32, 8) + o]) == (1, 1, 1)         # wraps


def test_overlap_selftest_agrees_with_python_integers(tmp_path):
    prog = os.path.join(HERE, "overlap_selftest")
    subprocess.check_call(["make", "-s", "-C", HERE])
    lists = list(span_lists())
    verdicts = [classify(l) for l in lists]
    assert len(lists) > 3000 and {v[0] for v in verdicts} == {0, 1} and any(v[0] and v[1] == v[2] for v in verdicts)
    path = tmp_path / "cases.txt"
    with open(path, "w") as f:
        for l, v in zip(lists, verdicts):
            f.write(" ".join([str(len(l))] + [str(x) for s in l for x in s] + [str(x) for x in v]) + "\n")
    r = subprocess.run([prog, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"{len(lists)} lists, 0 failures" in r.stdout
    # the program must be able to fail: one flipped expectation
    with open(path, "w") as f:
        f.write("2 4096 32 8 0 0 4128 32 8 1 0 0 -1 -1\n")
    assert subprocess.run([prog, str(path)], capture_output=True).returncode == 1


# ---- 1b. csrc/call_args.hpp alone: one buffer list, its null text, its spans and what it stages ---------------------------------
ROLES = {"in": 0, "out": 1, "shared": 2, "bcast": 3, "opaque": 4}


def buffer_lists():
    """(lanes, [(name, ptr, bytes_per_element, count, role, required)], form): lists shaped like the library's, n = 5; form:
    the name of the call's form where its list depends on one (the wire signatures), else None."""
    n, at = 5, lambda k: 0x7000_0000_0000 + 4096 * k
    req = lambda name, k, bpe, count, role: (name, at(k), bpe, count, role, 1)
    # an optional buffer, given and not given (sign_deterministic's v)
    for v in (at(3), 0):
        yield n, [req("msg32", 1, 32, n, "in"), req("r32", 2, 32, n, "out"), ("v", v, 1, n, "out", 0), req("err", 4, 1, n, "out")], None
    # counts of n + 1, n and 1 (hash_batch's offsets; the single sum of point_msm beside its per-point flags)
    yield n, [req("data", 1, 0, 0, "opaque"), req("offsets", 2, 8, n + 1, "in"), req("out32", 3, 32, n, "out")], None
    yield n, [req("k32", 1, 32, n, "shared"), req("outx32", 2, 32, 1, "out"), req("status", 3, 1, 1, "out"),
              ("point_err", at(4), 1, n, "out", 0)], None
    # the parents of a BIP-32 call: one for all lanes (broadcast), one per lane, and one lane with its one parent
    for n_parents, lanes in ((1, n), (n, n), (1, 1)):
        yield lanes, [req("par_sk32", 1, 32, n_parents, "bcast"), req("index", 2, 4, lanes, "in"), req("sk32", 3, 32, lanes, "out")], None
    # a zero count: no span, and nothing but an empty copy to stage
    yield 0, [req("sk32", 1, 32, 0, "in"), req("pk32", 2, 32, 0, "out"), req("seed32", 3, 32, 1, "shared")], None
    # missing pointers: every required name, every optional one behind the semicolon; one name alone
    yield n, [("a32", 0, 32, n, "in", 1), req("b32", 2, 32, n, "in"), ("idx", 0, 4, n, "in", 0), ("err", 0, 1, n, "out", 1),
              ("point_err", at(5), 1, n, "out", 0)], None
    yield n, [("plan", 0, 8, 6, "out", 1)], None
    yield n, [("table", 0, 0, 0, "opaque", 1), ("idx", 0, 4, n, "in", 0), req("k32", 3, 32, n, "in")], "FORM_X"
    yield n, [], None


def expected_of_list(k, lanes, bufs, form=None):
    join = lambda v: v[0] if len(v) == 1 else ", ".join(v[:-1]) + " and " + v[-1]
    need, may = [b[0] for b in bufs if b[5]], [b[0] for b in bufs if not b[5]]
    text = "-"
    if any(b[5] and b[1] == 0 for b in bufs):
        text = "null pointer (" + join(need) + (" is required" if len(need) == 1 else " are all required")
        text += f" with {form}" if form else ""
        text += ("; " + join(may) + " may be null" if may else "") + ")"
    lines, staged, slots = [f"list {k}", f"missing {text}"], [], []
    for name, ptr, bpe, count, role, _req in bufs:
        if role != "opaque" and ptr and count:
            broadcast = role == "shared" or (role == "bcast" and count == 1 and lanes > 1)
            lines.append(f"span {name} {ptr} {bpe} {count} {int(role == 'out')} {int(broadcast)}")
    for name, ptr, bpe, count, role, _req in bufs:
        if role != "opaque" and ptr:
            slots.append(f"slot {name} {0xD0000000 + 256 * (len(staged) + 1)}")
            staged.append(f"stage {name} {'out' if role == 'out' else 'in'} {bpe * count}")
        else:
            slots.append(f"slot {name} {ptr}")
    return lines + staged + slots


def test_one_buffer_list_gives_the_null_text_the_spans_and_the_staged_bytes(tmp_path):
    prog = os.path.join(HERE, "overlap_selftest")
    subprocess.check_call(["make", "-s", "-C", HERE])
    cases = list(buffer_lists())
    path = tmp_path / "lists.txt"
    with open(path, "w") as f:
        for lanes, bufs, form in cases:
            f.write(" ".join([form or "-", str(lanes), str(len(bufs))] + [f"{b[0]} {b[1]} {b[2]} {b[3]} {ROLES[b[4]]} {b[5]}" for b in bufs]) + "\n")
    r = subprocess.run([prog, "--lists", str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    want = [line for k, case in enumerate(cases) for line in expected_of_list(k, *case)]
    assert r.stdout.splitlines() == want
    # the cases hold what they are meant to: a broadcast parent and a plain one, an optional null, a zero count, one name alone
    out = r.stdout
    assert "span par_sk32 %d 32 1 0 1" % (0x7000_0000_0000 + 4096) in out and "span par_sk32 %d 32 5 0 0" % (0x7000_0000_0000 + 4096) in out
    assert "span par_sk32 %d 32 1 0 0" % (0x7000_0000_0000 + 4096) in out and "stage sk32 in 0" in out and "stage offsets in 48" in out
    assert "missing null pointer (plan is required)" in out
    assert "missing null pointer (a32, b32 and err are all required; idx and point_err may be null)" in out
    assert "missing null pointer (table and k32 are all required with FORM_X; idx may be null)" in out
    # every buffer that has both: the bytes staged are the bytes the span covers
    span, stage, k = {}, {}, -1
    for line in out.splitlines():
        w = line.split()
        if w[0] == "list":
            k = int(w[1])
        elif w[0] == "span":
            span[(k, w[1])] = int(w[3]) * int(w[4])
        elif w[0] == "stage":
            stage[(k, w[1])] = int(w[3])
    assert len(span) > 20 and all(stage[key] == b for key, b in span.items())
    assert all(key in span or b == 0 for key, b in stage.items())
    # a list the program cannot read is an error, not an empty success
    with open(path, "w") as f:
        f.write("- 5 1 msg32 4096 32 5 9 1\n")
    assert subprocess.run([prog, "--lists", str(path)], capture_output=True).returncode == 2


# ---- 2. the entry points -----------------------------------------------------------------------------------------------------
N = 4
# One row per per-element call: its arguments behind ctx, in the header's order.
#   ("in" | "out" | "shared", bytes per element, count)   a checked buffer; count: "n", "n+1" or 1
#   ("bcast", bytes)          an input of n_parents elements (a broadcast one where n_parents == 1 < n)
#   ("free",)                 a pointer the check does not look at (variable-length data, an opaque handle); never read here
#   ("off",)                  a pointer argument this form of the call does not use: passed as NULL
#   ("slot",)                 void **out of p2e_point_table_create: written (NULL) before anything else, so it must be real
#   ("n",), ("np",), int      the batch size, n_parents, a plain value
# A call with several forms (wire formats) has one row per form.
IN32, OUT32, ERR = ("in", 32, "n"), ("out", 32, "n"), ("out", 1, "n")
SH32 = ("shared", 32, "n")
CALLS = {
    "p2e_ecdsa_verify_batch": [[SH32, SH32, SH32, SH32, SH32, ("n",), ERR, ERR]],
    "p2e_p256_verify_batch": [[("free",), SH32, SH32, SH32, SH32, SH32, ("n",), ERR, ERR]],
    "p2e_ecdsa_public_key_batch": [[0, 0, IN32, OUT32, OUT32, ("n",), ERR]],
    "p2e_ecdsa_sign_batch": [[0, 0, IN32, IN32, IN32, OUT32, OUT32, ("n",), ERR]],
    "p2e_ecdsa_recover_batch": [[0, IN32, IN32, IN32, ("in", 1, "n"), OUT32, OUT32, ("n",), ERR]],
    "p2e_ecdsa_sign_recoverable_batch": [[0, 0, IN32, IN32, IN32, OUT32, OUT32, ERR, ("n",), ERR]],
    "p2e_hash_batch": [[0, 0, ("free",), ("in", 8, "n+1"), OUT32, ("n",)]],
    "p2e_ecdsa_nonce_rfc6979_batch": [[0, IN32, IN32, OUT32, ("n",)]],
    "p2e_ecdsa_sign_deterministic_batch": [[0, 0, IN32, IN32, OUT32, OUT32, ERR, ("n",), ERR]],
    "p2e_eth_address_batch": [[IN32, IN32, ("in", 1, "n"), ("out", 20, "n"), ("n",)]],
    "p2e_point_decode_batch": [[0, ("free",), ("in", 8, "n+1"), OUT32, OUT32, ("n",), ERR]],
    "p2e_point_encode_batch": [[0, 0, IN32, IN32, ("out", 33, "n"), ("n",), ERR], [0, 1, IN32, IN32, ("out", 65, "n"), ("n",), ERR]],
    "p2e_sig_decode_batch": [[0, 0, 0, ("free",), ("in", 8, "n+1"), OUT32, OUT32, ("off",), ("n",), ERR],
                             [0, 1, 0, ("in", 64, "n"), ("off",), OUT32, OUT32, ("off",), ("n",), ERR],
                             [0, 2, 0, ("in", 65, "n"), ("off",), OUT32, OUT32, ERR, ("n",), ERR]],
    "p2e_sig_encode_batch": [[0, 0, 0, IN32, IN32, ("off",), ("out", 72, "n"), ERR, ("n",), ERR],
                             [0, 1, 0, IN32, IN32, ("off",), ("out", 64, "n"), ("off",), ("n",), ERR],
                             [0, 2, 0, IN32, IN32, ("in", 1, "n"), ("out", 65, "n"), ("off",), ("n",), ERR]],
    "p2e_point_msm": [[0, 0, SH32, SH32, SH32, ("n",), ("out", 32, 1), ("out", 32, 1), ("out", 1, 1), ERR]],
    "p2e_point_mul_batch": [[0, 0, IN32, IN32, IN32, OUT32, OUT32, ("n",), ERR]],
    "p2e_point_lincomb_batch": [[0, 0, IN32, IN32, IN32, IN32, OUT32, OUT32, ("n",), ERR]],
    "p2e_point_add_batch": [[0, IN32, IN32, IN32, IN32, OUT32, OUT32, ("n",), ERR]],
    "p2e_point_table_create": [[0, SH32, SH32, ("n",), ERR, ("slot",)]],
    "p2e_point_table_mul_batch": [[("free",), ("in", 4, "n"), IN32, OUT32, OUT32, ("n",), ERR]],
    "p2e_point_table_lincomb_batch": [[("free",), ("in", 4, "n"), IN32, IN32, OUT32, OUT32, ("n",), ERR]],
    "p2e_ecdsa_verify_table_batch": [[("free",), ("in", 4, "n"), IN32, IN32, IN32, ("n",), ERR, ERR]],
    "p2e_schnorr_public_key_batch": [[IN32, OUT32, ("n",), ERR]],
    "p2e_schnorr_sign_batch": [[IN32, IN32, IN32, ("out", 64, "n"), ("n",), ERR]],
    "p2e_schnorr_verify_batch": [[IN32, IN32, ("in", 64, "n"), ("n",), ERR, ERR]],
    "p2e_xonly_decode_batch": [[IN32, OUT32, OUT32, ("n",), ERR]],
    "p2e_schnorr_verify_aggregate": [[SH32, SH32, ("shared", 64, "n"), ("n",), ("shared", 32, 1), 0, ("out", 1, 1), ERR]],
    "p2e_bip32_master_batch": [[("in", 32, "n"), 32, OUT32, OUT32, ("n",), ERR], [("in", 63, "n"), 63, OUT32, OUT32, ("n",), ERR]],
    "p2e_bip32_ckd_priv_batch": [[("bcast", 32), ("bcast", 32), ("np",), ("in", 4, "n"), OUT32, OUT32, ("n",), ERR]],
    "p2e_bip32_ckd_pub_batch": [[("bcast", 32), ("bcast", 32), ("bcast", 32), ("np",), ("in", 4, "n"), OUT32, OUT32, OUT32, ("n",), ERR]],
    "p2e_key_hash160_batch": [[0, IN32, IN32, ("in", 1, "n"), ("out", 20, "n"), ("n",)]],
    "p2e_hash160_batch": [[("free",), ("in", 8, "n+1"), ("out", 20, "n"), ("n",)]],
}
# the pointer arguments a call may be given as NULL (include/p2e.h); every other pointer of a row is required, the "free" and
# "slot" ones included.  ("off" arguments are not the form's own: they are NULL in every run.)
OPTIONAL = {
    "p2e_ecdsa_sign_deterministic_batch": {"v"},
    "p2e_eth_address_batch": {"err"},
    "p2e_sig_decode_batch": {"v"},
    "p2e_point_msm": {"point_err"},
    "p2e_point_table_create": {"point_err"},
    "p2e_point_table_mul_batch": {"idx"},
    "p2e_point_table_lincomb_batch": {"idx"},
    "p2e_ecdsa_verify_table_batch": {"idx"},
    "p2e_schnorr_verify_aggregate": {"err"},
    "p2e_key_hash160_batch": {"err_in"},
}
# exact in place, as the header lists it: (output, input) by argument name
ALLOWED = {
    "p2e_ecdsa_public_key_batch": [("pkx32", "sk32")],
    "p2e_ecdsa_sign_batch": [("r32", "msg32"), ("s32", "k32")],
    "p2e_ecdsa_sign_recoverable_batch": [("r32", "msg32"), ("s32", "k32")],
    "p2e_ecdsa_sign_deterministic_batch": [("r32", "msg32")],
    "p2e_ecdsa_nonce_rfc6979_batch": [("k32", "msg32")],
    "p2e_ecdsa_recover_batch": [("pkx32", "r32"), ("pky32", "s32")],
    "p2e_point_mul_batch": [("outx32", "px32"), ("outy32", "py32"), ("outx32", "k32")],
    "p2e_point_lincomb_batch": [("outx32", "px32"), ("outy32", "py32")],
    "p2e_point_add_batch": [("outx32", "px32"), ("outy32", "py32")],
    "p2e_point_table_mul_batch": [("outx32", "k32")],
    "p2e_point_table_lincomb_batch": [("outx32", "b32"), ("outx32", "a32")],
    "p2e_schnorr_public_key_batch": [("pk32", "sk32")],
    "p2e_xonly_decode_batch": [("px32", "pk32")],
    "p2e_bip32_ckd_priv_batch": [("sk32", "par_sk32"), ("cc32", "par_cc32")],
    "p2e_bip32_ckd_pub_batch": [("pkx32", "par_pkx32"), ("pky32", "par_pky32"), ("cc32", "par_cc32")],
}


def header_calls():
    """name -> [(type, parameter name)] for every declaration of include/p2e.h that returns long."""
    import re
    src = _strip_c_comments(open(HEADER).read())
    src = re.sub(r"^\s*#[^\n]*(\\\n[^\n]*)*", " ", src, flags=re.M)
    out = {}
    for m in re.finditer(r"\blong\s+(p2e_\w+)\s*\(([^;{}]*?)\)\s*;", src):
        params = []
        for a in m.group(2).split(","):
            mm = re.match(r"(.*?)(\w+)$", a.strip())
            params.append((mm.group(1).strip(), mm.group(2)))
        out[m.group(1)] = params
    return out


def per_element_calls():
    """The calls BUFFER OVERLAP covers, told from the column-matrix calls by their declarations alone: a context, a batch size
    n (m for the table), and no leading dimension, row stride or wire stride."""
    out = {}
    for name, params in header_calls().items():
        names = [p for _t, p in params]
        if not params[0][0].startswith("p2e_ctx") or not ({"n", "m"} & set(names)):
            continue
        if any(p == "ld" or p.startswith("ld_") or "row_ld" in p or "stride" in p for p in names):
            continue
        out[name] = params[1:]
    return out


def test_every_per_element_call_of_the_header_has_a_span_table():
    H = per_element_calls()
    assert len(H) >= 32 and sorted(H) == sorted(CALLS)
    for name, forms in CALLS.items():
        for row in forms:
            assert len(row) == len(H[name]), name
            for spec, (typ, pname) in zip(row, H[name]):
                assert ("*" in typ) == (isinstance(spec, tuple) and spec[0] not in ("n", "np")), (name, pname)
                if isinstance(spec, tuple) and spec[0] == "out":
                    assert "const" not in typ, (name, pname)
                if isinstance(spec, tuple) and spec[0] in ("in", "shared", "bcast"):
                    assert "const" in typ, (name, pname)
                if spec == ("n",):
                    assert pname in ("n", "m")
                if spec == ("np",):
                    assert pname == "n_parents"
    for name, pairs in ALLOWED.items():
        names = [p for _t, p in H[name]]
        assert all(o in names and i in names for o, i in pairs), name


SLOT = 1024


class Call:
    """One form of one call, its checked buffers carved out of one allocation, SLOT bytes apart."""

    def __init__(self, name, row, n_parents=None, n=N):
        self.name, self.row, self.n, self.n_parents = name, row, n, n if n_parents is None else n_parents
        self.pnames = [p for _t, p in per_element_calls()[name]]
        self.arena = np.zeros(SLOT * (len(row) + 2), np.uint8)
        self.slot = np.zeros(1, np.uint64)
        self.base = {}                                                    # position -> address
        for k, spec in enumerate(row):
            if isinstance(spec, tuple) and spec[0] in ("in", "out", "shared", "bcast", "free"):
                self.base[k] = self.arena.ctypes.data + SLOT * (k + 1)

    def geometry(self, k):
        spec = self.row[k]
        if spec[0] == "bcast":
            return spec[1], self.n_parents
        return spec[1], {"n": self.n, "n+1": self.n + 1, 1: 1}[spec[2]]

    def positions(self, *kinds):
        return [k for k, s in enumerate(self.row) if isinstance(s, tuple) and s[0] in kinds]

    def run(self, ctx, moved=None):
        L = p2e.lib()
        moved = moved or {}
        args = [ctx]
        for k, spec in enumerate(self.row):
            if not isinstance(spec, tuple):
                args.append(spec)
            elif spec[0] == "n":
                args.append(C.c_size_t(self.n))
            elif spec[0] == "np":
                args.append(C.c_size_t(self.n_parents))
            elif spec[0] == "off":
                args.append(None)
            elif spec[0] == "slot":
                args.append(C.c_void_p(moved.get(k, self.slot.ctypes.data)))
            else:
                args.append(C.c_void_p(moved.get(k, self.base[k])))
        rc = getattr(L, self.name)(*args)
        return rc, (L.p2e_last_error() or b"").decode()


def all_forms():
    for name, forms in CALLS.items():
        for row in forms:
            yield name, row


@pytest.fixture(scope="module")
def fake():
    one = np.zeros(64, np.uint64)
    yield C.c_void_p(one.ctypes.data)
    assert not one.any()


def _refused(call, fake, moved, a, b):
    rc, msg = call.run(fake, moved)
    assert rc == -1, (call.name, call.pnames[a], call.pnames[b], rc)
    assert "overlap" in msg and call.pnames[a] in msg and call.pnames[b] in msg, (call.name, msg)
    assert not call.arena.any() and not call.slot.any()


def test_disjoint_arguments_pass_the_check_and_meet_the_null_context():
    for name, row in all_forms():
        rc, msg = Call(name, row).run(None)
        assert rc == -1 and msg == "null context", (name, msg)
    for name in ("p2e_bip32_ckd_priv_batch", "p2e_bip32_ckd_pub_batch"):       # one parent, in its own bytes
        rc, msg = Call(name, CALLS[name][0], n_parents=1).run(None)
        assert rc == -1 and msg == "null context", (name, msg)


def test_a_null_required_pointer_is_named_and_a_null_optional_one_is_accepted():
    """Every pointer of every form, NULL in turn, with a null context: a required one is refused by name, an optional one gets
    as far as the context's own null test.  Each run follows an accepted one, so the text read is the refused call's own."""
    required = optional = 0
    assert set(OPTIONAL) <= set(CALLS)
    for name, row in all_forms():
        call = Call(name, row)
        pointers = call.positions("in", "out", "shared", "bcast", "free", "slot")
        assert OPTIONAL.get(name, set()) <= {call.pnames[k] for k in call.positions("in", "out", "shared", "bcast", "free", "slot", "off")}
        for k in pointers:
            pname = call.pnames[k]
            assert call.run(None) == (-1, "null context"), name
            rc, msg = call.run(None, {k: 0})
            if pname in OPTIONAL.get(name, ()):
                assert rc == -1 and msg == "null context", (name, pname, msg)
                optional += 1
            else:
                assert rc == -1 and msg.startswith("null pointer ("), (name, pname, msg)
                assert pname in re.findall(r"\w+", msg.split(";")[0]), (name, pname, msg)
                required += 1
            assert not call.arena.any() and not call.slot.any()
    assert required > 150 and optional >= 10


def test_every_output_shifted_onto_an_input_is_refused(fake):
    seen = 0
    for name, row in all_forms():
        call = Call(name, row)
        for i in call.positions("in", "shared", "bcast"):
            bpe, count = call.geometry(i)
            for o in call.positions("out"):
                _refused(call, fake, {o: call.base[i] + (bpe if count > 1 else 1)}, i, o)
                seen += 1
    assert seen > 200


def test_adjacent_buffers_are_no_overlap():
    for name, row in all_forms():
        call = Call(name, row)
        for i in call.positions("in", "shared", "bcast"):
            bpe, count = call.geometry(i)
            for o in call.positions("out"):
                obpe, ocount = call.geometry(o)
                for at in (call.base[i] + bpe * count, call.base[i] - obpe * ocount):     # right behind, right in front
                    rc, msg = call.run(None, {o: at})
                    assert rc == -1 and msg == "null context", (name, call.pnames[i], call.pnames[o], msg)


def test_every_pair_of_outputs_on_one_buffer_is_refused(fake):
    seen = 0
    for name, row in all_forms():
        call = Call(name, row)
        for a, b in itertools.combinations(call.positions("out"), 2):
            _refused(call, fake, {b: call.base[a]}, a, b)
            seen += 1
    assert seen > 60


def test_the_in_place_forms_of_the_header_pass_and_every_other_stride_does_not(fake):
    for name, pairs in ALLOWED.items():
        for row in CALLS[name]:
            call = Call(name, row)
            for o_name, i_name in pairs:
                o, i = call.pnames.index(o_name), call.pnames.index(i_name)
                rc, msg = call.run(None, {o: call.base[i]})
                assert rc == -1 and msg == "null context", (name, o_name, i_name, msg)
    # the same base with another element size or count is no in-place form
    for name, row in all_forms():
        call = Call(name, row)
        for i in call.positions("in", "shared", "bcast"):
            for o in call.positions("out"):
                same = call.geometry(i) == call.geometry(o) and row[i][0] in ("in", "bcast")
                rc, msg = call.run(None if same else fake, {o: call.base[i]})
                assert rc == -1 and (msg == "null context" if same else "overlap" in msg), (name, call.pnames[i], call.pnames[o], msg)


def test_a_broadcast_parent_may_not_be_overwritten(fake):
    for name in ("p2e_bip32_ckd_priv_batch", "p2e_bip32_ckd_pub_batch"):
        call = Call(name, CALLS[name][0], n_parents=1)
        for i in call.positions("bcast"):
            for o in call.positions("out"):
                if call.row[o][1] != 32:
                    continue
                _refused(call, fake, {o: call.base[i]}, i, o)            # child 0 on the parent: the form that was silently wrong
                _refused(call, fake, {o: call.base[i] - 32}, i, o)       # child 1 on the parent


def test_a_sum_may_not_land_in_its_terms_even_for_one_term(fake):
    call = Call("p2e_point_msm", CALLS["p2e_point_msm"][0], n=1)
    for i_name, o_name in (("k32", "outx32"), ("px32", "outx32"), ("py32", "outy32")):
        i, o = call.pnames.index(i_name), call.pnames.index(o_name)
        _refused(call, fake, {o: call.base[i]}, i, o)
    call = Call("p2e_schnorr_verify_aggregate", CALLS["p2e_schnorr_verify_aggregate"][0], n=1)
    i, o = call.pnames.index("seed32"), call.pnames.index("verdict")
    _refused(call, fake, {o: call.base[i]}, i, o)


# ---- 3. why the broadcast parent is refused: the bodies themselves, walked in order on the CPU --------------------------------
def test_the_emulation_shows_the_defect_the_refusal_prevents():
    """tests/emu_hd walks the elements of CKDpriv in order on one OpenMP thread.  Children written over their own parents
    (n_parents == n) are the oracle's; children written over the ONE parent are not: element 1 derives from child 0, with
    err == 0 -- what the library now refuses before it launches."""
    hd = os.path.join(ROOT, "tests", "emu_hd")
    lib = os.path.join(hd, "libp2e_emu_hd.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-s", "-C", hd, "libp2e_emu_hd.so"])
    code = ("import ctypes as C, sys, numpy as np\n"
            "sys.path.insert(0, sys.argv[2]); import hd_inputs as HI\n"
            "L = C.CDLL(sys.argv[1]); L.emuhd_ckd_priv.restype = C.c_long\n"
            "p = lambda a: a.ctypes.data_as(C.c_void_p)\n"
            "n = 65\n"
            "S = HI.priv_set(); sk, cc, idx, err = S['sk'][:n].copy(), S['cc'][:n].copy(), S['index'][:n].copy(), np.zeros(n, np.uint8)\n"
            "L.emuhd_ckd_priv(p(sk), p(cc), C.c_size_t(n), p(idx), p(sk), p(cc), C.c_size_t(n), p(err))\n"
            "own = np.array_equal(sk, S['out_sk'][:n]) and np.array_equal(cc, S['out_cc'][:n]) and np.array_equal(err, S['err'][:n])\n"
            "S = HI.priv_set_one_parent(); sk, cc = np.zeros((n, 32), np.uint8), np.zeros((n, 32), np.uint8)\n"
            "sk[0], cc[0] = S['sk'][0], S['cc'][0]\n"
            "L.emuhd_ckd_priv(p(sk), p(cc), C.c_size_t(1), p(idx), p(sk), p(cc), C.c_size_t(n), p(err))\n"
            "val = lambda r: int.from_bytes(r.tobytes(), 'little')\n"
            "first = np.array_equal(sk[0], S['out_sk'][0])\n"
            "second = HI.ckd_priv(val(S['out_sk'][0]), S['out_cc'][0].tobytes(), int(idx[1]))\n"
            "from_child = val(sk[1]) == second[1] and cc[1].tobytes() == second[2] and err[1] == 0\n"
            "print(int(own), int(first), int(from_child), int(np.array_equal(sk[1], S['out_sk'][1])))\n")
    env = dict(os.environ, OMP_NUM_THREADS="1")
    out = subprocess.run([sys.executable, "-c", code, lib, os.path.join(ROOT, "tests")], capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stderr
    own, first, from_child, right = [int(v) for v in out.stdout.split()]
    assert own == 1                      # one parent per child, in place: the oracle's children
    assert (first, from_child, right) == (1, 1, 0)      # one parent, in place: child 0 is right, child 1 derives from child 0
