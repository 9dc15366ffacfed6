"""MuSig2 (include/p2e.h p2e_musig_key_agg_batch and the six calls after it) without a GPU.

The bodies of csrc/musig.hpp compiled with g++ (tests/emu_musig, built on demand, -DP2E_F29_BOUNDS: a violated limb bound of
the lazy 29-bit arithmetic aborts the process) against the oracle of tests/musig_inputs.py, a restatement of BIP-327 in Python
integers and hashlib that uses nothing under test.  The oracle is pinned by (a) the standard's four key-aggregation vectors, (b)
the three midstates from hashlib, which must also be the constants in csrc/musig.hpp, and (c) every full round ending in a
signature that tests/schnorr_inputs.py's BIP-340 verifier accepts.  Then every byte of every body on the chain and on the special
sets, the arithmetic behind the hashes with coefficients no hash will ever produce, and the stand-alone sanitizer program of
tests/emu_musig, which must exit 0.

BUFFER OVERLAP for the seven calls is checked here through p2e.lib() with tests/test_overlap_cpu.py's machinery and a span table
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
import musig_inputs as M
import schnorr_inputs as SI
from test_overlap_cpu import Call, _refused, fake, header_calls  # noqa: F401  (fake is a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "emu_musig")


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def emu():
    lib, prog = os.path.join(HERE, "libp2e_emu_musig.so"), os.path.join(HERE, "musig_selftest")
    if not (os.path.exists(lib) and os.path.exists(prog)):
        subprocess.check_call(["make", "-s", "-C", HERE])
    return C.CDLL(lib)


def run_set(emu, call, inputs, want, count=None):
    count = len(want["err"]) if count is None else count
    ins, ref = M.cut(call, inputs, want, count)
    rc, outs = M.invoke(getattr(emu, "emumusig_" + call), call, ins, count)
    M.assert_matches(call, rc, outs, ref, count)


# ---- the oracle first ---------------------------------------------------------------------------------------------------------
def test_oracle_reproduces_the_key_aggregation_vectors():
    for keys, qx, odd in M.KEYAGG_VECTORS:
        code, rec, pk = M.key_agg([M.cpoint(k) for k in keys])
        assert code == 0 and pk.hex().upper() == qx and int.from_bytes(rec[32:64], "little") & 1 == odd, keys
    code, rec, _pk = M.key_agg([M.cpoint(M.X1)] * 3)
    assert not int.from_bytes(rec[160:164], "little") & M.KA_HAVE_PK2 and not any(rec[128:160])       # no second key exists


def test_every_full_round_ends_in_a_signature_the_bip340_verifier_accepts():
    c = M.chain()
    good, combos = M.good_sessions(c), set()
    assert len(good) == M.N_SET - 4
    for i in good:
        code, sig = c["sig_agg"][i]
        assert code == 0 and SI.verify(c["msg"][i], c["tweak_xonly"][i][2], sig) == (0, 1), i
        assert all(v == (0, 1) for v in c["partial_verify"][i]), i
        combos.add((M.session_parse(c["session"][i][1])[1]["r_odd"], M.keyagg_parse(c["tweak_xonly"][i][1])[1]["Q"][1] & 1))
    assert combos == {(False, 0), (False, 1), (True, 0), (True, 1)}      # y(R) and y(Q), odd and even, in all four combinations
    assert {len(k) for k in c["keys"][:64]} == {0, 1, 2, 3, 4, 17}       # the first wave's lanes diverge
    for i in (4, 5):                                                     # [A, A, A] and [A, A, B, B]
        assert len(set(c["keys"][i])) == (1 if i == 4 else 2) and c["key_agg"][i][0] == 0
    for i in list(M.CHAIN_BAD_KEYS) + [M.CHAIN_EMPTY]:                   # a flag travels down the chain
        assert c["key_agg"][i][0] and c["session"][i][0] == M.WIRE_INFINITY and c["sig_agg"][i][0]


def test_midstates_are_the_tags_chaining_values(emu):
    got = np.zeros(24, np.uint32)
    emu.emumusig_midstates(_p(got))
    src = open(os.path.join(ROOT, "plonky2-ecdsa_amd", "csrc", "musig.hpp")).read()
    body = src[src.index("P2E_HD Sha256State musig_midstate"):src.index("// a SHA-256 byte stream")]
    parsed = [int(v, 16) for v in re.findall(r"s\.h\[\d\] = (0x[0-9a-f]{8})u", body)]
    assert len(parsed) == 24
    for t, tag in enumerate(M.TAGS):
        assert tuple(int(v) for v in got[8 * t:8 * t + 8]) == M.tag_midstate(tag) == tuple(parsed[8 * t:8 * t + 8]), tag


# ---- every body on every set ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["key_agg", "apply_tweak", "apply_tweak/xonly", "apply_tweak/taproot", "nonce_agg", "session", "partial_sign",
                                  "partial_verify", "sig_agg"])
def test_body_on_the_chain(emu, name):
    inputs, want = M.chain_sets()[name]
    run_set(emu, name.split("/")[0], inputs, want)
    run_set(emu, name.split("/")[0], inputs, want, count=65)


def test_bodies_on_the_special_sets(emu):
    sets = M.special_sets()
    assert len(sets) == 10
    for _name, (call, inputs, want) in sets.items():
        run_set(emu, call, inputs, want)
    codes = {name: set(want["err"].tolist()) for name, (_c, _i, want) in sets.items()}
    assert codes["key_agg"] == {0, M.WIRE_BAD_LENGTH, M.WIRE_COORD_RANGE, M.WIRE_NOT_ON_CURVE, M.WIRE_INFINITY}
    assert codes["apply_tweak/plain"] == codes["apply_tweak/xonly"] == {0, M.WIRE_SCALAR_RANGE, M.WIRE_INFINITY, M.WIRE_BAD_PREFIX}
    assert M.WIRE_BAD_INDEX in codes["partial_verify"] and M.WIRE_SCALAR_RANGE in codes["sig_agg"]


def test_the_tweak_in_place_is_the_tweak(emu):
    inputs, want = M.chain_sets()["apply_tweak/xonly"]
    n = 65
    rec, pk, err = inputs["keyagg192_in"][:n].copy(), np.zeros((n, 32), np.uint8), np.zeros(n, np.uint8)
    emu.emumusig_apply_tweak.restype = C.c_long
    bad = emu.emumusig_apply_tweak(_p(rec), _p(inputs["tweak32"]), C.c_int(M.TWEAK_XONLY), _p(rec), _p(pk), C.c_size_t(n), _p(err))
    assert bad == np.count_nonzero(want["err"][:n]) and np.array_equal(rec, want["keyagg192_out"][:n]) and np.array_equal(pk, want["agg_pk32"][:n])


def test_forced_coefficients_behind_the_hashes(emu):
    """Q at infinity in the key aggregation and R_1 = -b R_2 in the session: no hash produces them"""
    (ka_in, ka_want), (se_in, se_want) = M.forced_sets()
    n = len(ka_want["code"])
    code, qx, qy = np.full(n, 0xAA, np.uint8), np.full((n, 32), 0xAA, np.uint8), np.full((n, 32), 0xAA, np.uint8)
    emu.emumusig_forced_key_agg(_p(ka_in["pkx32"]), _p(ka_in["pky32"]), _p(ka_in["coef32"]), _p(ka_in["key_offsets"]), _p(code), _p(qx), _p(qy),
                                C.c_size_t(n))
    assert code.tolist() == ka_want["code"].tolist() == [M.WIRE_INFINITY, M.WIRE_INFINITY, 0]
    assert np.array_equal(qx, ka_want["qx32"]) and np.array_equal(qy, ka_want["qy32"])
    n = len(se_want["code"])
    code, ses = np.full(n, 0xAA, np.uint8), np.full((n, 128), 0xAA, np.uint8)
    emu.emumusig_forced_session(_p(se_in["keyagg192"]), _p(se_in["aggnonce128"]), _p(se_in["msg32"]), _p(se_in["b32"]), _p(code), _p(ses), C.c_size_t(n))
    assert not code.any() and np.array_equal(ses, se_want["session128"])


def vector_file(path, inputs, want, n):
    """the first n sessions of a key-aggregation set and the oracle's outputs in tests/emu_musig/musig_selftest.cpp's layout"""
    total = int(inputs["key_offsets"][n])
    with open(path, "wb") as f:
        f.write(struct.pack("<QQ", n, total))
        for a in (inputs["pkx32"][:total], inputs["pky32"][:total], inputs["key_offsets"][:n + 1], want["keyagg192"][:n], want["agg_pk32"][:n],
                  want["err"][:n]):
            f.write(np.ascontiguousarray(a).tobytes())


def test_sanitizer_program_exits_zero(emu, tmp_path):
    """tests/emu_musig/musig_selftest under -fsanitize=address,undefined: a full round from small integers, the first wave of the
    chain in one buffer, and every session alone in allocations of exactly its own keys and record.  A stand-alone program:
    nothing is loaded into this process."""
    path = tmp_path / "musig_vectors.bin"
    inputs, want = M.chain_sets()["key_agg"]
    vector_file(path, inputs, want, 64)
    res = subprocess.run([os.path.join(HERE, "musig_selftest"), str(path)], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "round trip, 64 sessions in one buffer, 64 alone ok" in res.stdout
    with open(path, "r+b") as f:                                   # the program must be able to fail: one flipped expectation
        f.seek(-40, os.SEEK_END)
        b = f.read(1)
        f.seek(-40, os.SEEK_END)
        f.write(bytes([b[0] ^ 1]))
    assert subprocess.run([os.path.join(HERE, "musig_selftest"), str(path)], capture_output=True).returncode == 1


# ---- the entry points: declarations, nulls, overlap (BUFFER OVERLAP, include/p2e.h) -------------------------------------------
OUT1, OUT32, OUT64, OUT128, OUT192 = (("out", w, "n") for w in (1, 32, 64, 128, 192))
SH32, SH64, SH128, SH192 = (("shared", w, "n") for w in (32, 64, 128, 192))
OFFS = ("shared", 8, "n+1")
SESSIONS = C.c_size_t(3)                                          # n_sessions of the row (size_t: ctypes would pass a bare int as 32 bits)
SES128, SES192 = ("shared", 128, "sessions"), ("shared", 192, "sessions")
PLAIN, TAPROOT = C.c_int(M.TWEAK_PLAIN), C.c_int(M.TWEAK_TAPROOT)
# One row per form of a call: its arguments behind ctx, in the header's order (tests/test_overlap_cpu.py explains the entries);
# "free" is a per-signer array, whose extent only the device knows
CALLS = {
    "p2e_musig_key_agg_batch": [[("free",), ("free",), OFFS, OUT192, OUT32, ("n",), OUT1]],
    "p2e_musig_apply_tweak_batch": [[("in", 192, "n"), SH32, PLAIN, OUT192, OUT32, ("n",), OUT1],
                                    [("in", 192, "n"), SH32, TAPROOT, OUT192, OUT32, ("n",), OUT1]],
    "p2e_musig_nonce_agg_batch": [[("free",), OFFS, OUT128, ("n",), OUT1]],
    "p2e_musig_session_batch": [[SH192, SH128, SH32, OUT128, ("n",), OUT1]],
    "p2e_musig_partial_sign_batch": [[SH64, SH32, SH192, SH128, OUT32, ("n",), OUT1]],
    "p2e_musig_partial_verify_batch": [[SH32, SH128, SH32, SH32, ("shared", 4, "n"), SES192, SES128, SESSIONS, ("n",), OUT1, OUT1]],
    "p2e_musig_sig_agg_batch": [[("free",), OFFS, SH192, SH128, OUT64, ("n",), OUT1]],
}
OPTIONAL = {"p2e_musig_partial_verify_batch": {"session_index"}}
ALLOWED = {"p2e_musig_apply_tweak_batch": [("keyagg192_out", "keyagg192_in")]}
CHECKED_IN = ("in", "shared")


class MusigCall(Call):
    """test_overlap_cpu.Call with the parameter names taken from header_calls(): per_element_calls() does not list a call
    whose batch size is not named n or m"""

    def __init__(self, name, row, n=2):                            # (two 192-byte records side by side fit one 1024-byte slot)
        self.name, self.row, self.n, self.n_parents = name, row, n, n
        self.pnames = [p for _t, p in header_calls()[name][1:]]
        self.arena = np.zeros(1024 * (len(row) + 2), np.uint8)
        self.slot = np.zeros(1, np.uint64)
        self.base = {k: self.arena.ctypes.data + 1024 * (k + 1) for k, spec in enumerate(row)
                     if isinstance(spec, tuple) and spec[0] in ("in", "out", "shared", "free")}

    def geometry(self, k):
        spec = self.row[k]
        return spec[1], {"n": self.n, "n+1": self.n + 1, "sessions": SESSIONS.value}[spec[2]]


def all_forms():
    for name, forms in CALLS.items():
        for row in forms:
            yield name, row


def test_the_seven_declarations_exist_with_a_count_parameter():
    H = header_calls()
    assert len(CALLS) == 7
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
                if spec is SESSIONS:
                    assert pname == "n_sessions"
                if spec is PLAIN or spec is TAPROOT:
                    assert pname == "mode"
        assert [p for _t, p in params[1:]] == [a for a in M.ORDER[name[len("p2e_musig_"):-len("_batch")]]], name
    text = open(os.path.join(ROOT, "include", "p2e.h")).read()
    assert re.search(r"#define P2E_MUSIG_MAX_SIGNERS 1024\b", text)
    assert all(re.search(rf"#define P2E_MUSIG_TWEAK_{k} {v}\b", text) for k, v in (("PLAIN", 0), ("XONLY", 1), ("TAPROOT", 2)))
    assert "A SECRET NONCE MUST NEVER BE USED TWICE" in text and "TWO departures from the standard's Sign" in text
    L = p2e.lib()
    assert all(getattr(L, name).restype is C.c_long for name in CALLS)
    assert (p2e.WIRE_BAD_LENGTH, p2e.WIRE_BAD_PREFIX, p2e.WIRE_COORD_RANGE, p2e.WIRE_NOT_ON_CURVE, p2e.WIRE_INFINITY, p2e.WIRE_SCALAR_RANGE,
            p2e.WIRE_BAD_INDEX) == (M.WIRE_BAD_LENGTH, M.WIRE_BAD_PREFIX, M.WIRE_COORD_RANGE, M.WIRE_NOT_ON_CURVE, M.WIRE_INFINITY,
                                    M.WIRE_SCALAR_RANGE, M.WIRE_BAD_INDEX)
    assert (p2e.MUSIG_MAX_SIGNERS, p2e.MUSIG_TWEAK_PLAIN, p2e.MUSIG_TWEAK_XONLY, p2e.MUSIG_TWEAK_TAPROOT) == (1024, 0, 1, 2)
    for call in M.ORDER:
        assert callable(getattr(p2e.Context, f"musig_{call}_batch"))


def test_disjoint_arguments_pass_the_check_and_meet_the_null_context():
    for name, row in all_forms():
        rc, msg = MusigCall(name, row).run(None)
        assert rc == -1 and msg == "null context", (name, msg)


def test_a_null_required_pointer_is_named_and_the_nullable_ones_are_accepted():
    required = optional = 0
    for name, row in all_forms():
        call = MusigCall(name, row)
        for k in call.positions("in", "out", "shared", "free"):
            pname = call.pnames[k]
            rc, msg = call.run(None, {k: 0})
            if pname in OPTIONAL.get(name, ()) or (pname == "tweak32" and row[2] is TAPROOT):
                assert rc == -1 and msg == "null context", (name, pname, msg)
                optional += 1
            else:
                assert rc == -1 and msg.startswith("null pointer ("), (name, pname, msg)
                assert pname in re.findall(r"\w+", msg.split(";")[0]), (name, pname, msg)
                required += 1
            assert not call.arena.any()
    assert required == 6 + 5 + 4 + 4 + 5 + 6 + 8 + 6 and optional == 2
    # an unknown mode and n_sessions == 0 are refused by name
    name = "p2e_musig_apply_tweak_batch"
    rc, msg = MusigCall(name, [C.c_int(3) if spec is PLAIN else spec for spec in CALLS[name][0]]).run(None)
    assert rc == -1 and "mode" in msg
    name = "p2e_musig_partial_verify_batch"
    rc, msg = MusigCall(name, [C.c_size_t(0) if spec is SESSIONS else spec for spec in CALLS[name][0]]).run(None)
    assert rc == -1 and "n_sessions" in msg


def test_every_output_shifted_onto_an_input_is_refused(fake):
    seen = 0
    for name, row in all_forms():
        call = MusigCall(name, row)
        for i in call.positions(*CHECKED_IN):
            bpe, _count = call.geometry(i)
            for o in call.positions("out"):
                _refused(call, fake, {o: call.base[i] + min(bpe, 4)}, i, o)
                seen += 1
    assert seen == 1 * 3 + 2 * 2 * 3 + 1 * 2 + 3 * 2 + 4 * 2 + 7 * 2 + 3 * 2


def test_every_pair_of_outputs_on_one_buffer_is_refused(fake):
    seen = 0
    for name, row in all_forms():
        call = MusigCall(name, row)
        for a, b in itertools.combinations(call.positions("out"), 2):
            _refused(call, fake, {b: call.base[a]}, a, b)
            seen += 1
    assert seen == 3 + 3 + 3 + 1 + 1 + 1 + 1 + 1


def test_the_one_in_place_form_passes_and_nothing_else_does(fake):
    for name, pairs in ALLOWED.items():
        for row in CALLS[name]:
            call = MusigCall(name, row)
            for o_name, i_name in pairs:
                rc, msg = call.run(None, {call.pnames.index(o_name): call.base[call.pnames.index(i_name)]})
                assert rc == -1 and msg == "null context", (name, o_name, i_name, msg)
    text = open(os.path.join(ROOT, "include", "p2e.h")).read()
    assert "keyagg192_out = keyagg192_in" in text and "The ONE in-place form" in text
    allowed = 0
    for name, row in all_forms():
        call = MusigCall(name, row)
        for i in call.positions(*CHECKED_IN):
            for o in call.positions("out"):
                same = row[i][0] == "in" and call.geometry(i) == call.geometry(o)
                rc, msg = call.run(None if same else fake, {o: call.base[i]})
                assert rc == -1 and (msg == "null context" if same else "overlap" in msg), (name, call.pnames[i], call.pnames[o], msg)
                allowed += same
    assert allowed == 2                                            # keyagg192_out = keyagg192_in, in both forms of the call


def test_adjacent_buffers_are_no_overlap():
    for name, row in all_forms():
        call = MusigCall(name, row)
        for i in call.positions(*CHECKED_IN):
            bpe, count = call.geometry(i)
            for o in call.positions("out"):
                obpe, ocount = call.geometry(o)
                for at in (call.base[i] + bpe * count, call.base[i] - obpe * ocount):
                    rc, msg = call.run(None, {o: at})
                    assert rc == -1 and msg == "null context", (name, call.pnames[i], call.pnames[o], msg)


def test_count_zero_checks_nothing_but_the_pointers():
    L = p2e.lib()
    buf = np.zeros(64, np.uint8)
    zero, one = C.c_size_t(0), C.c_size_t(1)
    b = _p(buf)
    assert L.p2e_musig_partial_verify_batch(None, b, b, b, b, None, b, b, one, zero, b, b) == -1      # (null context)
    assert (L.p2e_last_error() or b"").decode() == "null context"
    assert L.p2e_musig_key_agg_batch(None, b, b, b, b, b, zero, b) == -1
    assert (L.p2e_last_error() or b"").decode() == "null context"


def test_example_compiles_against_the_header(tmp_path):
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                           os.path.join(ROOT, "examples", "musig_sign.c"), "-o", str(tmp_path / "musig_sign.o")])
