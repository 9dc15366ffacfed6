"""Taproot (include/p2e.h p2e_taproot_leaf_hash_batch and the four calls after it) without a GPU.

The bodies of csrc/taproot.hpp compiled with g++ (tests/emu_taproot, built on demand, -DP2E_F29_BOUNDS: a violated limb bound
of the lazy 29-bit arithmetic aborts the process) against the oracle of tests/taproot_inputs.py, a restatement of BIP-341 in
Python integers and hashlib that uses nothing under test: the three tag midstates, the prefixed absorption on every edge
length at every alignment, every byte of every body on the input sets, the arithmetic behind the hash with a t no hash will
ever produce, and the three pins.  The stand-alone sanitizer program of tests/emu_taproot must exit 0.

BUFFER OVERLAP for the five calls is checked here through p2e.lib() with tests/test_overlap_cpu.py's machinery and a span
table of this file's own: the calls name their batch size `count`, so that file's list (derived from `n` / `m`) leaves them out."""
import ctypes as C
import hashlib
import itertools
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import plonky2_ecdsa_amd as p2e
import hd_inputs as HI
import taproot_inputs as TI
from test_overlap_cpu import Call, _refused, fake, header_calls  # noqa: F401  (fake is a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "emu_taproot")


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def filled(*shape):
    return np.full(shape, 0xAA, np.uint8)


@pytest.fixture(scope="module")
def emu():
    lib, prog = os.path.join(HERE, "libp2e_emu_taproot.so"), os.path.join(HERE, "taproot_selftest")
    if not (os.path.exists(lib) and os.path.exists(prog)):
        subprocess.check_call(["make", "-s", "-C", HERE])
    L = C.CDLL(lib)
    for name in ("emutr_leaf_hash", "emutr_merkle_root", "emutr_tweak_pubkey", "emutr_tweak_seckey", "emutr_verify_commitment"):
        getattr(L, name).restype = C.c_long
    return L


# ---- the oracle first ---------------------------------------------------------------------------------------------------------
def test_oracle_reproduces_the_pins():
    """15 values: three leaf hashes, two roots (one absent), three tweaks, three output keys with parity, three commitments"""
    assert TI.check_pins() == 15
    assert TI.compact_size(252) == b"\xfc" and TI.compact_size(253) == b"\xfd\xfd\x00" and TI.compact_size(0xFFFF) == b"\xfd\xff\xff"
    assert TI.compact_size(0x10000) == b"\xfe\x00\x00\x01\x00"


def test_input_sets_contain_what_they_claim():
    S = TI.script_set()
    lens = (S["offsets"][1:].astype(np.int64) - S["offsets"][:-1].astype(np.int64)).tolist()
    for L in TI.SCRIPT_LENGTHS:
        starts = {int(S["offsets"][i]) & 3 for i, v in enumerate(lens) if v == L}
        assert starts >= {0, 1, 2, 3}, L
    assert sum(v < 0 for v in lens) == 1 and (S["version"] & 1).sum() == 1 and max(lens) == 0x10000
    assert sorted(set(S["err"].tolist())) == [TI.WIRE_OK, TI.WIRE_BAD_LENGTH, TI.WIRE_BAD_PREFIX]
    M = TI.path_set()
    assert {0, 1, 2, 7, 128} <= set(M["depth"].tolist()) and (M["depth"] > 128).any()
    assert (M["depth"][:64] == 128).any() and (M["depth"][:64] == 0).any()
    K = TI.pubkey_set()
    assert {TI.WIRE_OK, TI.WIRE_COORD_RANGE, TI.WIRE_NOT_ON_CURVE} == set(K["with_root"]["err"].tolist()) and {0, 1} == set(K["with_root"]["parity"].tolist())
    D = TI.seckey_set()
    assert (D["with_root"]["err"] == TI.WIRE_SCALAR_RANGE).sum() == 3


def test_path_set_holds_equal_and_neighbouring_nodes():
    M = TI.path_set()
    equal = above = below = 0
    for i in range(M["leaf"].shape[0]):
        d = int(M["depth"][i])
        if d > M["max_depth"]:
            continue
        k = M["leaf"][i].tobytes()
        for j in range(d):
            e = M["path"][i, j].tobytes()
            equal += e == k
            above += e[:31] == k[:31] and e[31] > k[31]
            below += e[:31] == k[:31] and e[31] < k[31]
            k = TI.branch(k, e)
    assert equal > 10 and above > 10 and below > 10


# ---- the constants and the absorption --------------------------------------------------------------------------------------------
def test_midstates_are_the_tags_chaining_values(emu):
    got = np.zeros(24, np.uint32)
    emu.emutr_midstates(_p(got))
    for t, tag in enumerate(TI.TAGS):
        assert tuple(int(v) for v in got[8 * t:8 * t + 8]) == TI.tag_midstate(tag), tag


@pytest.mark.parametrize("prefix_len", [0, 2, 4, 6, 8])
def test_prefixed_absorption_against_hashlib_on_every_length_and_alignment(emu, prefix_len):
    """SHA-256(prefix || message) from the IV.  The message sits between sentinel bytes whose value changes between two runs:
    a digest that depended on a byte outside the message would differ (a READ outside the message's words is what the
    sanitizer program's exact allocations catch)."""
    prefix = bytes(range(0xF1, 0xF1 + prefix_len))
    pbuf = np.frombuffer(prefix + bytes(8 - prefix_len), np.uint8).copy()
    lengths = [L for L in TI.SCRIPT_LENGTHS if L < 0xFFFF] + [183, 4096 + 57]
    for L in lengths:
        msg = TI._stream(f"absorb{L}", L)
        want = hashlib.sha256(prefix + msg).digest()
        for al in range(4):
            for sentinel in (0xEE, 0x11):
                buf = np.full(16 + al + L + 16, sentinel, np.uint8)
                base = (-buf.ctypes.data) % 4 + 8 + al            # the message starts at address = al (mod 4)
                buf[base:base + L] = np.frombuffer(msg, np.uint8)
                out = filled(32)
                emu.emutr_sha256_prefixed(_p(pbuf), C.c_uint(prefix_len), _p(buf), C.c_uint64(base), C.c_uint64(base + L), _p(out))
                assert out.tobytes() == want, (prefix_len, L, al, sentinel)


# ---- every body on every set ---------------------------------------------------------------------------------------------------
def test_leaf_hash_body_on_the_script_set(emu):
    S = TI.script_set()
    n = len(S["version"])
    leaf, err = filled(n, 32), filled(n)
    bad = emu.emutr_leaf_hash(_p(S["version"]), _p(S["data"]), _p(S["offsets"]), _p(leaf), C.c_size_t(n), _p(err))
    assert np.array_equal(err, S["err"]) and bad == int((S["err"] != 0).sum()) == 2
    assert np.array_equal(leaf, S["leaf"]) and not leaf[S["err"] != 0].any()


@pytest.mark.parametrize("max_depth", [0, 1, 128])
def test_merkle_root_body_on_the_path_set(emu, max_depth):
    M = TI.path_set(257 if max_depth == 128 else 65, max_depth)
    n = M["leaf"].shape[0]
    root, err = filled(n, 32), filled(n)
    path = np.ascontiguousarray(M["path"])
    bad = emu.emutr_merkle_root(_p(M["leaf"]), _p(path) if max_depth else None, _p(M["depth"]), C.c_size_t(max_depth), _p(root),
                                C.c_size_t(n), _p(err))
    assert np.array_equal(err, M["err"]) and bad == int((M["err"] != 0).sum()) > 0
    assert np.array_equal(root, M["root"]) and not root[M["err"] != 0].any()
    # in place: root32 = leaf32
    leaf, err = M["leaf"].copy(), filled(n)
    emu.emutr_merkle_root(_p(leaf), _p(path) if max_depth else None, _p(M["depth"]), C.c_size_t(max_depth), _p(leaf), C.c_size_t(n), _p(err))
    assert np.array_equal(leaf, M["root"]) and np.array_equal(err, M["err"])


@pytest.mark.parametrize("form", ["with_root", "no_root"])
def test_tweak_pubkey_body_on_the_key_set(emu, form):
    K = TI.pubkey_set()
    n, want = K["pk"].shape[0], K[form]
    root = K["root"] if form == "with_root" else None
    out, par, err = filled(n, 32), filled(n), filled(n)
    bad = emu.emutr_tweak_pubkey(_p(K["pk"]), _p(root), _p(out), _p(par), C.c_size_t(n), _p(err))
    assert np.array_equal(err, want["err"]) and bad == int((want["err"] != 0).sum()) == 5
    assert np.array_equal(out, want["out"]) and np.array_equal(par, want["parity"])
    pk, err = K["pk"].copy(), filled(n)                              # in place: out_pk32 = pk32
    emu.emutr_tweak_pubkey(_p(pk), _p(root), _p(pk), _p(par), C.c_size_t(n), _p(err))
    assert np.array_equal(pk, want["out"]) and np.array_equal(err, want["err"])


@pytest.mark.parametrize("form", ["with_root", "no_root"])
def test_tweak_seckey_body_on_the_key_set(emu, form):
    D = TI.seckey_set()
    n, want = D["sk"].shape[0], D[form]
    root = D["root"] if form == "with_root" else None
    out, err = filled(n, 32), filled(n)
    bad = emu.emutr_tweak_seckey(_p(D["sk"]), _p(root), _p(out), C.c_size_t(n), _p(err))
    assert np.array_equal(err, want["err"]) and bad == int((want["err"] != 0).sum()) == 3
    assert np.array_equal(out, want["out"])
    sk, err = D["sk"].copy(), filled(n)                              # in place: out_sk32 = sk32
    emu.emutr_tweak_seckey(_p(sk), _p(root), _p(sk), C.c_size_t(n), _p(err))
    assert np.array_equal(sk, want["out"]) and np.array_equal(err, want["err"])
    # the tweaked secret key is the key of the tweaked public key (the oracle's own consistency, on a few elements)
    for i in [i for i in range(n) if want["err"][i] == 0][:6]:
        pk = TI.b32(TI.base_mul(int.from_bytes(D["sk"][i].tobytes(), "big"))[0])
        code, q, _par = TI.tweak_pubkey(pk, root[i].tobytes() if root is not None else None)
        assert code == 0 and TI.b32(TI.base_mul(int.from_bytes(want["out"][i].tobytes(), "big"))[0]) == q


@pytest.mark.parametrize("max_depth", [0, 1, 8, 128])
def test_verify_commitment_body_on_the_commitment_set(emu, max_depth):
    S = TI.commitment_set(257 if max_depth == 8 else 65, max_depth)
    n = S["pk"].shape[0]
    err, valid = filled(n), filled(n)
    path = np.ascontiguousarray(S["path"])
    bad = emu.emutr_verify_commitment(_p(S["out_pk"]), _p(S["out_parity"]), _p(S["pk"]), _p(S["leaf"]), _p(path) if max_depth else None,
                                      _p(S["depth"]), C.c_size_t(max_depth), C.c_size_t(n), _p(err), _p(valid))
    assert np.array_equal(err, S["err"]) and np.array_equal(valid, S["valid"]) and bad == int((S["err"] != 0).sum())
    assert not valid[S["err"] != 0].any() and valid.sum() > 10


def test_the_three_pins_through_the_bodies(emu):
    for pin in TI.PINS:
        pk = np.frombuffer(bytes.fromhex(pin["internal"]), np.uint8).copy()
        leaves = []
        for ver, script, want in pin["leaves"]:
            s = bytes.fromhex(script)
            data = np.frombuffer(s + bytes(-len(s) % 4), np.uint8).copy()
            leaf, err = filled(32), filled(1)
            emu.emutr_leaf_hash(_p(np.array([ver], np.uint8)), _p(data), _p(np.array([0, len(s)], np.uint64)), _p(leaf), C.c_size_t(1), _p(err))
            assert err[0] == 0 and leaf.tobytes().hex() == want
            leaves.append(leaf)
        root = None
        for k, leaf in enumerate(leaves):
            path = leaves[1 - k] if len(leaves) == 2 else filled(32)
            depth, root, err = np.array([len(leaves) - 1], np.uint8), filled(32), filled(1)
            emu.emutr_merkle_root(_p(leaf), _p(path), _p(depth), C.c_size_t(1), _p(root), C.c_size_t(1), _p(err))
            assert err[0] == 0 and root.tobytes().hex() == pin["root"]
        out, par, err = filled(32), filled(1), filled(1)
        emu.emutr_tweak_pubkey(_p(pk), _p(root), _p(out), _p(par), C.c_size_t(1), _p(err))
        assert (err[0], out.tobytes().hex(), par[0]) == (0, pin["output"], pin["parity"])
        for k, leaf in enumerate(leaves):
            path = leaves[1 - k] if len(leaves) == 2 else filled(32)
            depth, err, valid = np.array([len(leaves) - 1], np.uint8), filled(1), filled(1)
            emu.emutr_verify_commitment(_p(out), _p(par), _p(pk), _p(leaf), _p(path), _p(depth), C.c_size_t(1), C.c_size_t(1), _p(err), _p(valid))
            assert (err[0], valid[0]) == (0, 1)


def test_forced_tweaks_behind_the_hash(emu):
    """t >= n, t = 0, t G = P (the doubling), t G = -P (the neutral element), d + t = 0 (mod n): no hash produces them"""
    for pk, t, code, want, parity in TI.forced_pub():
        out, par = filled(32), filled(1)
        got = emu.emutr_finish_pub(_p(np.frombuffer(pk, np.uint8).copy()), _p(np.frombuffer(t, np.uint8).copy()), _p(out), _p(par))
        assert got == code, (pk.hex(), t.hex())
        assert (out.tobytes(), par[0]) == ((want, parity) if code == 0 else (b"\xAA" * 32, 0xAA))
    for d, t, code, want in TI.forced_sec():
        out = filled(32)
        got = emu.emutr_finish_sec(_p(np.frombuffer(d, np.uint8).copy()), _p(np.frombuffer(t, np.uint8).copy()), _p(out))
        assert got == code and out.tobytes() == (want if code == 0 else b"\xAA" * 32), (d.hex(), t.hex())


def vector_file(path):
    """the script set and the oracle's leaf hashes in tests/emu_taproot/taproot_selftest.cpp's layout"""
    S = TI.script_set()
    with open(path, "wb") as f:
        f.write(struct.pack("<QQ", len(S["version"]), S["data"].size))
        for a in (S["version"], S["data"], S["offsets"], S["leaf"], S["err"]):
            f.write(np.ascontiguousarray(a).tobytes())


def test_sanitizer_program_exits_zero(emu, tmp_path):
    """tests/emu_taproot/taproot_selftest under -fsanitize=address,undefined: the pins, the script set in one buffer, and every
    script alone in an allocation of exactly its own words.  A stand-alone program: nothing is loaded into this process."""
    path = tmp_path / "taproot_vectors.bin"
    vector_file(path)
    res = subprocess.run([os.path.join(HERE, "taproot_selftest"), str(path)], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "3 pins" in res.stdout
    with open(path, "r+b") as f:                                   # the program must be able to fail: one flipped expectation
        f.seek(-40, os.SEEK_END)
        b = f.read(1)
        f.seek(-40, os.SEEK_END)
        f.write(bytes([b[0] ^ 1]))
    assert subprocess.run([os.path.join(HERE, "taproot_selftest"), str(path)], capture_output=True).returncode == 1


# ---- the entry points: declarations, nulls, overlap (BUFFER OVERLAP, include/p2e.h) -------------------------------------------
IN32, OUT32, IN1, OUT1 = ("in", 32, "n"), ("out", 32, "n"), ("in", 1, "n"), ("out", 1, "n")
DEPTH = C.c_size_t(3)                                              # max_depth of the rows (a size_t: ctypes would pass a bare int as 32 bits)
PATH = ("in", 32 * 3, "n")                                      # (its geometry here: n elements of 32 max_depth bytes)
# One row per call: its arguments behind ctx, in the header's order (tests/test_overlap_cpu.py explains the entries)
CALLS = {
    "p2e_taproot_leaf_hash_batch": [[IN1, ("free",), ("in", 8, "n+1"), OUT32, ("n",), OUT1]],
    "p2e_taproot_merkle_root_batch": [[IN32, PATH, IN1, DEPTH, OUT32, ("n",), OUT1]],
    "p2e_taproot_tweak_pubkey_batch": [[IN32, IN32, OUT32, OUT1, ("n",), OUT1]],
    "p2e_taproot_tweak_seckey_batch": [[IN32, IN32, OUT32, ("n",), OUT1]],
    "p2e_taproot_verify_commitment_batch": [[IN32, IN1, IN32, IN32, PATH, IN1, DEPTH, ("n",), OUT1, OUT1]],
}
OPTIONAL = {"p2e_taproot_tweak_pubkey_batch": {"root32"}, "p2e_taproot_tweak_seckey_batch": {"root32"}}
ALLOWED = {
    "p2e_taproot_tweak_pubkey_batch": [("out_pk32", "pk32")],
    "p2e_taproot_tweak_seckey_batch": [("out_sk32", "sk32")],
    "p2e_taproot_merkle_root_batch": [("root32", "leaf32")],
}


class TaprootCall(Call):
    """test_overlap_cpu.Call with the parameter names taken from header_calls(): per_element_calls() does not list a call
    whose batch size is not named n or m"""

    def __init__(self, name, row, n=4):
        self.name, self.row, self.n, self.n_parents = name, row, n, n
        self.pnames = [p for _t, p in header_calls()[name][1:]]
        self.arena = np.zeros(1024 * (len(row) + 2), np.uint8)
        self.slot = np.zeros(1, np.uint64)
        self.base = {k: self.arena.ctypes.data + 1024 * (k + 1) for k, spec in enumerate(row)
                     if isinstance(spec, tuple) and spec[0] in ("in", "out", "free")}


def all_forms():
    for name, forms in CALLS.items():
        for row in forms:
            yield name, row


def test_the_five_declarations_exist_with_a_count_parameter():
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
                if isinstance(spec, tuple) and spec[0] in ("in", "free"):
                    assert "const" in typ, (name, pname)
                if spec == ("n",):
                    assert pname == "count"
                if spec is DEPTH:
                    assert pname == "max_depth"
    text = open(os.path.join(ROOT, "include", "p2e.h")).read()
    assert re.search(r"named `count`, NOT `n`, on purpose", text)
    L = p2e.lib()
    assert all(getattr(L, name).restype is C.c_long for name in CALLS)
    assert (p2e.WIRE_BAD_LENGTH, p2e.WIRE_BAD_PREFIX, p2e.WIRE_COORD_RANGE, p2e.WIRE_NOT_ON_CURVE, p2e.WIRE_INFINITY, p2e.WIRE_SCALAR_RANGE) == \
        (TI.WIRE_BAD_LENGTH, TI.WIRE_BAD_PREFIX, TI.WIRE_COORD_RANGE, TI.WIRE_NOT_ON_CURVE, TI.WIRE_INFINITY, TI.WIRE_SCALAR_RANGE)


def test_disjoint_arguments_pass_the_check_and_meet_the_null_context():
    for name, row in all_forms():
        rc, msg = TaprootCall(name, row).run(None)
        assert rc == -1 and msg == "null context", (name, msg)


def test_a_null_required_pointer_is_named_and_a_null_root_is_accepted():
    required = optional = 0
    for name, row in all_forms():
        call = TaprootCall(name, row)
        for k in call.positions("in", "out", "free"):
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
    assert required == 25 and optional == 2
    # max_depth == 0: path32 may be null; max_depth == 129 is refused by name
    for name in ("p2e_taproot_merkle_root_batch", "p2e_taproot_verify_commitment_batch"):
        row = [C.c_size_t(0) if spec is DEPTH else spec for spec in CALLS[name][0]]
        call = TaprootCall(name, row)
        assert call.run(None, {call.pnames.index("path32"): 0}) == (-1, "null context")
        row = [C.c_size_t(129) if spec is DEPTH else spec for spec in CALLS[name][0]]
        rc, msg = TaprootCall(name, row).run(None)
        assert rc == -1 and "max_depth" in msg, (name, msg)


def test_every_output_shifted_onto_an_input_is_refused(fake):
    seen = 0
    for name, row in all_forms():
        call = TaprootCall(name, row)
        for i in call.positions("in"):
            bpe, _count = call.geometry(i)
            for o in call.positions("out"):
                _refused(call, fake, {o: call.base[i] + min(bpe, 32)}, i, o)
                seen += 1
    assert seen == 4 + 6 + 6 + 4 + 12


def test_every_pair_of_outputs_on_one_buffer_is_refused(fake):
    seen = 0
    for name, row in all_forms():
        call = TaprootCall(name, row)
        for a, b in itertools.combinations(call.positions("out"), 2):
            _refused(call, fake, {b: call.base[a]}, a, b)
            seen += 1
    assert seen == 1 + 1 + 3 + 1 + 1


def test_the_in_place_forms_of_the_header_pass_and_every_other_stride_does_not(fake):
    for name, pairs in ALLOWED.items():
        call = TaprootCall(name, CALLS[name][0])
        for o_name, i_name in pairs:
            rc, msg = call.run(None, {call.pnames.index(o_name): call.base[call.pnames.index(i_name)]})
            assert rc == -1 and msg == "null context", (name, o_name, i_name, msg)
    text = open(os.path.join(ROOT, "include", "p2e.h")).read()
    assert all(f"{o} = {i}" in text for pairs in ALLOWED.values() for o, i in pairs)
    # the same base with another element size or count is no in-place form (path32 under root32: 32 bytes on 96)
    for name, row in all_forms():
        call = TaprootCall(name, row)
        for i in call.positions("in"):
            for o in call.positions("out"):
                same = call.geometry(i) == call.geometry(o)
                rc, msg = call.run(None if same else fake, {o: call.base[i]})
                assert rc == -1 and (msg == "null context" if same else "overlap" in msg), (name, call.pnames[i], call.pnames[o], msg)


def test_adjacent_buffers_are_no_overlap():
    for name, row in all_forms():
        call = TaprootCall(name, row)
        for i in call.positions("in"):
            bpe, count = call.geometry(i)
            for o in call.positions("out"):
                obpe, ocount = call.geometry(o)
                for at in (call.base[i] + bpe * count, call.base[i] - obpe * ocount):
                    rc, msg = call.run(None, {o: at})
                    assert rc == -1 and msg == "null context", (name, call.pnames[i], call.pnames[o], msg)


def test_host_staged_script_may_not_touch_an_output():
    """BUFFER OVERLAP 5: the extent of `script` is known on the host only where the offsets are (host pointers); nothing can be
    staged without a device, so here only the declaration-level facts: count == 0 returns 0 before the context is read."""
    L = p2e.lib()
    buf = np.zeros(64, np.uint8)
    zero = C.c_size_t(0)
    assert L.p2e_taproot_leaf_hash_batch(None, _p(buf), _p(buf), _p(buf), _p(buf), zero, _p(buf)) == -1       # (null context)
    assert (L.p2e_last_error() or b"").decode() == "null context"


def test_example_compiles_against_the_header(tmp_path):
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                           os.path.join(ROOT, "examples", "taproot_scan.c"), "-o", str(tmp_path / "taproot_scan.o")])
    # the private key the example derives from is test vector 1's m/0' (tests/hd_inputs.py)
    src = open(os.path.join(ROOT, "examples", "taproot_scan.c")).read()
    assert HI.TV1_M_0H[0].to_bytes(32, "big").hex() in src and HI.TV1_M_0H[1].hex() in src
