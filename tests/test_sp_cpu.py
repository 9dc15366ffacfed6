"""Silent payments (include/p2e.h p2e_sp_input_hash_batch and the three calls after it) without a GPU.

The bodies of csrc/sp.hpp compiled with g++ (tests/emu_sp, built on demand, -DP2E_F29_BOUNDS: a violated limb bound of the lazy
29-bit arithmetic aborts the process) against the oracle of tests/sp_inputs.py, a restatement of BIP-352 in Python integers and
hashlib that uses nothing under test.  There are no published vectors here; the oracle is pinned by (a) sender = receiver --
every payment of the sets is made through a B_scan and found through b_scan A --, (b) the three midstates from hashlib and (c)
x((b_spend + t_k + l_j) G) == the matched output.  Then every byte of every body on the input sets, the arithmetic behind the
hash with a t no hash will ever produce, and the stand-alone sanitizer program of tests/emu_sp, which must exit 0.

BUFFER OVERLAP for the four calls is checked here through p2e.lib() with tests/test_overlap_cpu.py's machinery and a span table
of this file's own: the calls name their batch size `count`, so that file's list (derived from `n` / `m`) leaves them out."""
import ctypes as C
import itertools
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import plonky2_ecdsa_amd as p2e
import hd_inputs as HI
import sp_inputs as SP
from test_overlap_cpu import Call, _refused, fake, header_calls  # noqa: F401  (fake is a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "emu_sp")


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def filled(*shape, dtype=np.uint8):
    return np.full(shape, 0xAA if dtype == np.uint8 else 0xAAAAAAAA, dtype)


@pytest.fixture(scope="module")
def emu():
    lib, prog = os.path.join(HERE, "libp2e_emu_sp.so"), os.path.join(HERE, "sp_selftest")
    if not (os.path.exists(lib) and os.path.exists(prog)):
        subprocess.check_call(["make", "-s", "-C", HERE])
    L = C.CDLL(lib)
    for name in ("emusp_input_hash", "emusp_label", "emusp_send", "emusp_scan"):
        getattr(L, name).restype = C.c_long
    return L


def emu_scan(emu, S, n=None):
    """the scan body on the first n elements of a set: (flagged count, n_hits, hit_output, hit_label, hit_tweak, err), each one
    element longer than the call may write"""
    n = len(S["err"]) if n is None else n
    mh = S["max_hits"]
    out = filled(n + 1), filled(n + 1, mh, dtype=np.uint32), filled(n + 1, mh), filled(n + 1, mh, 32), filled(n + 1)
    bad = emu.emusp_scan(_p(S["scan_sk"]), _p(S["spend_pkx"]), _p(S["spend_pky"]), _p(S["label_x"]), _p(S["label_y"]), C.c_size_t(S["n_labels"]),
                         _p(S["ax"]), _p(S["ay"]), _p(S["input_hash"]), _p(S["outputs"]), _p(S["out_offsets"]), C.c_size_t(mh), _p(out[0]), _p(out[1]),
                         _p(out[2]), _p(out[3]), C.c_size_t(n), _p(out[4]))
    return (bad,) + out


def assert_scan_equals(S, got, n=None):
    n = len(S["err"]) if n is None else n
    bad, n_hits, hit_output, hit_label, hit_tweak, err = got
    diff = np.nonzero((err[:n] != S["err"][:n]) | (n_hits[:n] != S["n_hits"][:n]))[0]
    assert diff.size == 0, [(int(i), int(err[i]), int(S["err"][i]), int(n_hits[i]), int(S["n_hits"][i])) for i in diff[:8]]
    assert np.array_equal(hit_output[:n], S["hit_output"][:n]) and np.array_equal(hit_label[:n], S["hit_label"][:n])
    assert np.array_equal(hit_tweak[:n], S["hit_tweak"][:n]) and bad == np.count_nonzero(S["err"][:n])
    assert (n_hits[n] == 0xAA) and (hit_output[n] == 0xAAAAAAAA).all() and (hit_label[n] == 0xAA).all() and (hit_tweak[n] == 0xAA).all() and err[n] == 0xAA
    flagged = S["err"][:n] != 0
    assert not n_hits[:n][flagged].any() and not hit_output[:n][flagged].any() and not hit_label[:n][flagged].any() and not hit_tweak[:n][flagged].any()


# ---- the oracle first ---------------------------------------------------------------------------------------------------------
def test_sender_and_receiver_meet():
    """(a) and (c): every planted payment, made through (input_hash a) B_scan, is found by the scan through (input_hash b_scan) A
    at the planted output under the planted label, and the key b_spend + t_k + l_j spends it"""
    txs, S, L = SP.transactions(), SP.scan_set(max_hits=8, n_labels=16), SP.labels_all()
    found = labelled = 0
    for i, t in enumerate(txs):
        if S["err"][i] or i in SP.BAD_HASH:
            continue
        assert t["S_send"] == SP._receiver_secret(i, True, SP.N_SET), i
        want = sorted(t["planted"], key=lambda p: p[1])[:8]
        assert S["n_hits"][i] == len(want), i
        for h, (idx, k, lab) in enumerate(want):
            assert k == h and S["hit_output"][i, h] == idx and S["hit_label"][i, h] == (0 if lab is None else lab + 1), (i, h)
            tk = int.from_bytes(S["hit_tweak"][i, h].tobytes(), "big")
            assert tk == SP.tweak(t["S_send"], k)
            d = (SP.B_SPEND_SK + tk + (0 if lab is None else L[lab][0])) % SP.N
            assert SP.b32(SP.base_mul(d)[0]) == t["outputs"][idx]
            found += 1
            labelled += lab is not None
    assert found > 300 and labelled > 60


def test_midstates_are_the_tags_chaining_values(emu):
    got = np.zeros(24, np.uint32)
    emu.emusp_midstates(_p(got))
    for t, tag in enumerate(SP.TAGS):
        assert tuple(int(v) for v in got[8 * t:8 * t + 8]) == SP.tag_midstate(tag), tag


def test_input_sets_contain_what_they_claim():
    txs, S, L = SP.transactions(), SP.scan_set(max_hits=8, n_labels=16), SP.labels_all()
    n_out = [len(t["outputs"]) for t in txs]
    assert {0, 1, 2, 40} <= set(n_out) and {0, 1, 2, 3} <= {len(t["planted"]) for t in txs}
    assert sorted(n_out[:3]) == [0, 5, 40] and len(txs[0]["planted"]) == 3 and not txs[2]["planted"]      # the first wave's neighbours
    shuffled = sum(1 for t in txs if [p[0] for p in t["planted"]] != sorted(p[0] for p in t["planted"]))
    assert shuffled > 10
    parities = set()
    for i, t in enumerate(txs):                                    # labelled payments whose P_k + L_j has even and odd y
        for idx, k, lab in t["planted"]:
            if lab is not None and not S["err"][i]:
                d = (SP.B_SPEND_SK + SP.tweak(t["S_send"], k) + L[lab][0]) % SP.N
                parities.add(SP.base_mul(d)[1] & 1)
    assert parities == {0, 1}
    dup = [t for i, t in enumerate(txs) if SP.KINDS[i % 16].get("duplicate") and t["planted"]]
    assert dup and all(t["outputs"].count(t["outputs"][t["planted"][0][0]]) == 2 for t in dup)
    assert all(t["outputs"].index(t["outputs"][t["planted"][0][0]]) == t["planted"][0][0] for t in dup)
    decoy = [i for i, t in enumerate(txs) if SP.KINDS[i % 16].get("decoy_p1") and t["S_send"]]
    assert decoy and all(S["n_hits"][i] == 0 and txs[i]["outputs"][1] == SP.finish_send(SP.B_SPEND, SP.tweak(txs[i]["S_send"], 1))[1] for i in decoy)
    assert any(int.from_bytes(o, "big") >= SP.P for t in txs for o in t["outputs"])
    assert max(len(t["planted"]) for t in txs) == 9 > SP.MAX_HITS and (S["n_hits"] == 8).any()
    assert set(S["err"].tolist()) == {SP.WIRE_OK, SP.WIRE_BAD_LENGTH, SP.WIRE_COORD_RANGE, SP.WIRE_NOT_ON_CURVE, SP.WIRE_INFINITY, SP.WIRE_SCALAR_RANGE}
    assert S["err"][SP.OFFSET_PAIR] == SP.WIRE_BAD_LENGTH and S["err"][SP.OFFSET_PAIR + 1] == 0
    assert (SP.scan_set(huge=True)["err"][SP.OFFSET_PAIR:SP.OFFSET_PAIR + 2] == SP.WIRE_BAD_LENGTH).all()
    assert not SP.scan_set(with_hash=False)["err"][list(SP.BAD_HASH)].any() and SP.scan_set()["err"][list(SP.BAD_HASH)].all()
    # fewer labels find fewer payments; a cap below the payments saturates
    assert SP.scan_set(max_hits=8, n_labels=0)["n_hits"].sum() < SP.scan_set(max_hits=8, n_labels=1)["n_hits"].sum() < S["n_hits"].sum()
    assert (SP.scan_set(max_hits=1, n_labels=1)["n_hits"] <= 1).all() and (SP.scan_set(max_hits=2, n_labels=1)["n_hits"] == 2).any()
    K = SP.send_set()
    assert set(K["err"].tolist()) == {SP.WIRE_OK, SP.WIRE_SCALAR_RANGE, SP.WIRE_INFINITY, SP.WIRE_COORD_RANGE, SP.WIRE_NOT_ON_CURVE}
    assert set(SP.input_hash_set()["err"].tolist()) == {SP.WIRE_OK, SP.WIRE_INFINITY, SP.WIRE_COORD_RANGE, SP.WIRE_NOT_ON_CURVE}


# ---- every body on every set ---------------------------------------------------------------------------------------------------
def test_input_hash_body_on_its_set(emu):
    H = SP.input_hash_set()
    n = len(H["err"])
    out, err = filled(n + 1, 32), filled(n + 1)
    bad = emu.emusp_input_hash(_p(H["outpoint"]), _p(H["ax"]), _p(H["ay"]), _p(out), C.c_size_t(n), _p(err))
    assert np.array_equal(err[:n], H["err"]) and bad == np.count_nonzero(H["err"]) == 4 and np.array_equal(out[:n], H["input_hash"])
    assert not out[:n][H["err"] != 0].any() and (out[n] == 0xAA).all() and err[n] == 0xAA
    ax, err = H["ax"].copy(), filled(n)                               # in place: input_hash32 = ax32
    emu.emusp_input_hash(_p(H["outpoint"]), _p(ax), _p(H["ay"]), _p(ax), C.c_size_t(n), _p(err))
    assert np.array_equal(ax, H["input_hash"]) and np.array_equal(err, H["err"])


@pytest.mark.parametrize("bad_key", [None, 0, SP.N])
def test_label_body_on_its_set(emu, bad_key):
    S = SP.label_set(SP.N_SET if bad_key is None else 65, bad_key)
    n = len(S["err"])
    tw, x, y, err = filled(n + 1, 32), filled(n + 1, 32), filled(n + 1, 32), filled(n + 1)
    bad = emu.emusp_label(_p(S["scan_sk"]), _p(S["index"]), _p(tw), _p(x), _p(y), C.c_size_t(n), _p(err))
    assert np.array_equal(err[:n], S["err"]) and bad == np.count_nonzero(S["err"]) == (0 if bad_key is None else n)
    assert np.array_equal(tw[:n], S["tweak"]) and np.array_equal(x[:n], S["x"]) and np.array_equal(y[:n], S["y"])
    assert (tw[n] == 0xAA).all() and (x[n] == 0xAA).all() and (y[n] == 0xAA).all() and err[n] == 0xAA
    if bad_key is None:                                             # the labels of the scan sets are these labels
        assert np.array_equal(x[0], SP.scan_set()["label_x"][0]) and S["tweak"].any()


def test_send_body_on_its_set(emu):
    K = SP.send_set()
    n = len(K["err"])
    out, err = filled(n + 1, 32), filled(n + 1)
    bad = emu.emusp_send(_p(K["a"]), _p(K["input_hash"]), _p(K["scan_pkx"]), _p(K["scan_pky"]), _p(K["spend_pkx"]), _p(K["spend_pky"]), _p(K["k"]),
                         _p(out), C.c_size_t(n), _p(err))
    assert np.array_equal(err[:n], K["err"]) and bad == np.count_nonzero(K["err"]) == len(SP.SEND_BAD)
    assert np.array_equal(out[:n], K["out"]) and not out[:n][K["err"] != 0].any() and (out[n] == 0xAA).all() and err[n] == 0xAA
    ih, err = K["input_hash"].copy(), filled(n)                      # in place: out_pk32 = input_hash32
    emu.emusp_send(_p(K["a"]), _p(ih), _p(K["scan_pkx"]), _p(K["scan_pky"]), _p(K["spend_pkx"]), _p(K["spend_pky"]), _p(K["k"]), _p(ih), C.c_size_t(n),
                   _p(err))
    assert np.array_equal(ih, K["out"]) and np.array_equal(err, K["err"])


@pytest.mark.parametrize("max_hits,n_labels,with_hash", [(2, 1, True), (1, 1, True), (8, 1, True), (2, 0, True), (2, 16, True), (8, 16, False)])
def test_scan_body_on_the_transaction_set(emu, max_hits, n_labels, with_hash):
    S = SP.scan_set(max_hits, n_labels, with_hash)
    assert_scan_equals(S, emu_scan(emu, S))
    if n_labels == 0:                                               # no labels: the label pointers may be null
        S0 = dict(S, label_x=None, label_y=None)
        assert_scan_equals(S, emu_scan(emu, S0))


def test_scan_body_flags_reversed_and_oversized_offsets_before_it_reads(emu):
    S = SP.scan_set(huge=True)
    assert_scan_equals(S, emu_scan(emu, S))
    assert int(S["out_offsets"][SP.OFFSET_PAIR + 1]) - int(S["out_offsets"][SP.OFFSET_PAIR]) == 2**32


@pytest.mark.parametrize("bad", sorted(SP.SHARED_BAD))
def test_scan_body_flags_every_element_for_a_bad_shared_argument(emu, bad):
    n_labels = 16 if bad.startswith("label_off") else 2
    S = SP.scan_set(2, n_labels, True, 65, False, bad)
    assert (S["err"] == SP.SHARED_BAD[bad]).all()
    assert_scan_equals(S, emu_scan(emu, S))


def test_forced_tweaks_behind_the_hash(emu):
    """t >= n, t = 0, t G = B_spend (the doubling), t G = -B_spend (the neutral element), P_k + L_j neutral (no match, no flag),
    L_j = P_k (the doubling inside a candidate): no hash produces them"""
    rows = SP.forced_finish()
    F = SP.forced_arrays(rows)
    n = len(rows)
    code, found, out, lab = filled(n), filled(n), filled(n, dtype=np.uint32), filled(n)
    emu.emusp_finish(_p(F["bx"]), _p(F["by"]), _p(F["lx"]), _p(F["ly"]), C.c_size_t(SP.FORCED_LABELS), _p(F["t"]), _p(F["outputs"]),
                     C.c_size_t(SP.FORCED_OUTPUTS), _p(code), _p(found), _p(out), _p(lab), C.c_size_t(n))
    assert code.tolist() == F["code"].tolist() and found.tolist() == F["found"].tolist()
    assert out.tolist() == F["hit_output"].tolist() and lab.tolist() == F["hit_label"].tolist()
    assert {SP.WIRE_OK, SP.WIRE_SCALAR_RANGE, SP.WIRE_INFINITY} == set(code.tolist())


def vector_file(path, S):
    """a scan set and the oracle's outputs in tests/emu_sp/sp_selftest.cpp's layout"""
    n = len(S["err"])
    with open(path, "wb") as f:
        f.write(struct.pack("<QQQQQ", n, S["n_labels"], S["max_hits"], S["outputs"].shape[0], int(S["input_hash"] is not None)))
        arrays = [S["scan_sk"], S["spend_pkx"], S["spend_pky"], S["label_x"], S["label_y"], S["ax"], S["ay"]]
        arrays += [S["input_hash"]] if S["input_hash"] is not None else []
        arrays += [S["outputs"], S["out_offsets"], S["n_hits"], S["hit_output"], S["hit_label"], S["hit_tweak"], S["err"]]
        for a in arrays:
            f.write(np.ascontiguousarray(a).tobytes())


def test_sanitizer_program_exits_zero(emu, tmp_path):
    """tests/emu_sp/sp_selftest under -fsanitize=address,undefined: a round trip from small integers, the set in one buffer, and
    every transaction alone in allocations of exactly its own outputs and slots.  A stand-alone program: nothing is loaded
    into this process."""
    path = tmp_path / "sp_vectors.bin"
    vector_file(path, SP.scan_set(max_hits=2, n_labels=1))
    res = subprocess.run([os.path.join(HERE, "sp_selftest"), str(path)], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "round trip, 257 transactions in one buffer, 256 alone" in res.stdout
    with open(path, "r+b") as f:                                   # the program must be able to fail: one flipped expectation
        f.seek(-40, os.SEEK_END)
        b = f.read(1)
        f.seek(-40, os.SEEK_END)
        f.write(bytes([b[0] ^ 1]))
    assert subprocess.run([os.path.join(HERE, "sp_selftest"), str(path)], capture_output=True).returncode == 1


# ---- the entry points: declarations, nulls, overlap (BUFFER OVERLAP, include/p2e.h) -------------------------------------------
IN32, OUT32, OUT1, IN4 = ("in", 32, "n"), ("out", 32, "n"), ("out", 1, "n"), ("in", 4, "n")
ONE32 = ("shared", 32, 1)
SH32 = ("shared", 32, "n")
LABELS, HITS = C.c_size_t(2), C.c_size_t(1)                       # n_labels and max_hits of the rows (size_t: ctypes would pass a bare int as 32 bits)
LAB32 = ("shared", 32, "labels")                                  # (n_labels elements)
# One row per call: its arguments behind ctx, in the header's order (tests/test_overlap_cpu.py explains the entries)
CALLS = {
    "p2e_sp_input_hash_batch": [[("in", 36, "n"), IN32, IN32, OUT32, ("n",), OUT1]],
    "p2e_sp_label_batch": [[ONE32, IN4, OUT32, OUT32, OUT32, ("n",), OUT1]],
    "p2e_sp_send_batch": [[IN32, IN32, IN32, IN32, IN32, IN32, IN4, OUT32, ("n",), OUT1]],
    "p2e_sp_scan_batch": [[ONE32, ONE32, ONE32, LAB32, LAB32, LABELS, SH32, SH32, SH32, ("free",), ("in", 8, "n+1"), HITS, OUT1, ("out", 4, "n"),
                           OUT1, OUT32, ("n",), OUT1]],
}
OPTIONAL = {"p2e_sp_scan_batch": {"input_hash32"}}
ALLOWED = {"p2e_sp_input_hash_batch": [("input_hash32", "ax32")], "p2e_sp_send_batch": [("out_pk32", "input_hash32")]}
CHECKED_IN = ("in", "shared")


class SpCall(Call):
    """test_overlap_cpu.Call with the parameter names taken from header_calls(): per_element_calls() does not list a call
    whose batch size is not named n or m"""

    def __init__(self, name, row, n=4):
        self.name, self.row, self.n, self.n_parents = name, row, n, n
        self.pnames = [p for _t, p in header_calls()[name][1:]]
        self.arena = np.zeros(1024 * (len(row) + 2), np.uint8)
        self.slot = np.zeros(1, np.uint64)
        self.base = {k: self.arena.ctypes.data + 1024 * (k + 1) for k, spec in enumerate(row)
                     if isinstance(spec, tuple) and spec[0] in ("in", "out", "shared", "free")}

    def geometry(self, k):
        spec = self.row[k]
        return spec[1], {"n": self.n, "n+1": self.n + 1, 1: 1, "labels": LABELS.value}[spec[2]]


def all_forms():
    for name, forms in CALLS.items():
        for row in forms:
            yield name, row


def test_the_four_declarations_exist_with_a_count_parameter():
    H = header_calls()
    for name, forms in CALLS.items():
        assert name in H and name in p2e.EXPORTS, name
        params = H[name]
        assert params[0][0].startswith("p2e_ctx") and "count" in [p for _t, p in params] and not {"n", "m"} & {p for _t, p in params}
        for row in forms:
            assert len(row) == len(params) - 1, name
            for spec, (typ, pname) in zip(row, params[1:]):
                assert ("*" in typ) == (isinstance(spec, tuple) and spec[0] != "n"), (name, pname)
                if isinstance(spec, tuple) and spec[0] == "out":
                    assert "const" not in typ, (name, pname)
                if isinstance(spec, tuple) and spec[0] in ("in", "shared", "free"):
                    assert "const" in typ, (name, pname)
                if spec == ("n",):
                    assert pname == "count"
                if spec is LABELS:
                    assert pname == "n_labels"
                if spec is HITS:
                    assert pname == "max_hits"
    text = open(os.path.join(ROOT, "include", "p2e.h")).read()
    assert re.search(r"#define P2E_SP_MAX_HITS 8\b", text) and re.search(r"#define P2E_SP_MAX_LABELS 16\b", text)
    assert "LITTLE-endian" in text and "no parameter is named n or m" in text
    L = p2e.lib()
    assert all(getattr(L, name).restype is C.c_long for name in CALLS)
    assert (p2e.WIRE_BAD_LENGTH, p2e.WIRE_COORD_RANGE, p2e.WIRE_NOT_ON_CURVE, p2e.WIRE_INFINITY, p2e.WIRE_SCALAR_RANGE) == \
        (SP.WIRE_BAD_LENGTH, SP.WIRE_COORD_RANGE, SP.WIRE_NOT_ON_CURVE, SP.WIRE_INFINITY, SP.WIRE_SCALAR_RANGE)
    for method in ("sp_input_hash_batch", "sp_label_batch", "sp_send_batch", "sp_scan_batch"):
        assert callable(getattr(p2e.Context, method))


def test_disjoint_arguments_pass_the_check_and_meet_the_null_context():
    for name, row in all_forms():
        rc, msg = SpCall(name, row).run(None)
        assert rc == -1 and msg == "null context", (name, msg)


def test_a_null_required_pointer_is_named_and_the_nullable_ones_are_accepted():
    required = optional = 0
    for name, row in all_forms():
        call = SpCall(name, row)
        for k in call.positions("in", "out", "shared", "free"):
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
            assert not call.arena.any()
    assert required == 5 + 6 + 9 + 14 and optional == 1
    # n_labels == 0: the label pointers may be null; the two limits are refused by name
    name = "p2e_sp_scan_batch"
    row = [C.c_size_t(0) if spec is LABELS else spec for spec in CALLS[name][0]]
    call = SpCall(name, row)
    assert call.run(None, {call.pnames.index("label_x32"): 0, call.pnames.index("label_y32"): 0}) == (-1, "null context")
    for swap, value in ((LABELS, 17), (HITS, 0), (HITS, 9)):
        row = [C.c_size_t(value) if spec is swap else spec for spec in CALLS[name][0]]
        rc, msg = SpCall(name, row).run(None)
        assert rc == -1 and "max_hits" in msg and "n_labels" in msg, (value, msg)
    for value in (1, 8):
        row = [C.c_size_t(value) if spec is HITS else spec for spec in CALLS[name][0]]
        assert SpCall(name, row).run(None) == (-1, "null context")


def out_geometry(call, o):
    """bytes per element and count of an output; the scan's hit arrays hold max_hits slots per element"""
    bpe, count = call.geometry(o)
    return bpe, count * (HITS.value if call.pnames[o].startswith("hit_") else 1)


def test_every_output_shifted_onto_an_input_is_refused(fake):
    seen = 0
    for name, row in all_forms():
        call = SpCall(name, row)
        for i in call.positions(*CHECKED_IN):
            bpe, _count = call.geometry(i)
            for o in call.positions("out"):
                _refused(call, fake, {o: call.base[i] + min(bpe, 4)}, i, o)
                seen += 1
    assert seen == 3 * 2 + 2 * 4 + 7 * 2 + 9 * 5


def test_every_pair_of_outputs_on_one_buffer_is_refused(fake):
    seen = 0
    for name, row in all_forms():
        call = SpCall(name, row)
        for a, b in itertools.combinations(call.positions("out"), 2):
            _refused(call, fake, {b: call.base[a]}, a, b)
            seen += 1
    assert seen == 1 + 6 + 1 + 10


def test_the_in_place_forms_of_the_header_pass_and_the_scan_has_none(fake):
    for name, pairs in ALLOWED.items():
        call = SpCall(name, CALLS[name][0])
        for o_name, i_name in pairs:
            rc, msg = call.run(None, {call.pnames.index(o_name): call.base[call.pnames.index(i_name)]})
            assert rc == -1 and msg == "null context", (name, o_name, i_name, msg)
    text = open(os.path.join(ROOT, "include", "p2e.h")).read()
    assert all(f"{o} = {i}" in text for pairs in ALLOWED.values() for o, i in pairs) and "No in-place form" in text
    # an output exactly on an input: fine where lane i owns element i of both at the same stride; never in the scan, never on
    # the one scan key of the label call, never on label_index (4 bytes under 32)
    for name, row in all_forms():
        call = SpCall(name, row)
        for i in call.positions(*CHECKED_IN):
            for o in call.positions("out"):
                same = row[i][0] == "in" and call.geometry(i) == out_geometry(call, o)
                rc, msg = call.run(None if same else fake, {o: call.base[i]})
                assert rc == -1 and (msg == "null context" if same else "overlap" in msg), (name, call.pnames[i], call.pnames[o], msg)
                assert not same or name != "p2e_sp_scan_batch"
    call = SpCall("p2e_sp_label_batch", CALLS["p2e_sp_label_batch"][0])
    _refused(call, fake, {call.pnames.index("label_tweak32"): call.base[call.pnames.index("label_index")]}, 1, 2)


def test_adjacent_buffers_are_no_overlap():
    for name, row in all_forms():
        call = SpCall(name, row)
        for i in call.positions(*CHECKED_IN):
            bpe, count = call.geometry(i)
            for o in call.positions("out"):
                obpe, ocount = out_geometry(call, o)
                for at in (call.base[i] + bpe * count, call.base[i] - obpe * ocount):
                    rc, msg = call.run(None, {o: at})
                    assert rc == -1 and msg == "null context", (name, call.pnames[i], call.pnames[o], msg)


def test_count_zero_checks_nothing_but_the_pointers():
    L = p2e.lib()
    buf = np.zeros(64, np.uint8)
    zero, one = C.c_size_t(0), C.c_size_t(1)
    b = _p(buf)
    assert L.p2e_sp_scan_batch(None, b, b, b, None, None, zero, b, b, None, b, b, one, b, b, b, b, zero, b) == -1      # (null context)
    assert (L.p2e_last_error() or b"").decode() == "null context"


def test_example_compiles_against_the_header(tmp_path):
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                           os.path.join(ROOT, "examples", "sp_scan.c"), "-o", str(tmp_path / "sp_scan.o")])
    # the private key the example derives from is test vector 1's m/0' (tests/hd_inputs.py)
    src = open(os.path.join(ROOT, "examples", "sp_scan.c")).read()
    assert HI.TV1_M_0H[0].to_bytes(32, "big").hex() in src and HI.TV1_M_0H[1].hex() in src
