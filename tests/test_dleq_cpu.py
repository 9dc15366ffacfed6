"""DLEQ proofs (include/p2e.h p2e_dleq_prove_batch, p2e_dleq_verify_batch) without a GPU.

The bodies of csrc/dleq.hpp compiled with g++ (tests/emu_dleq, built on demand, -DP2E_F29_BOUNDS: a violated limb bound of the
lazy 29-bit arithmetic, or a GLV half of 2^128 or more, aborts the process) against the oracle of tests/dleq_inputs.py, a
restatement of the header's definition in Python integers and hashlib that uses nothing under test.  There are no published
vectors here; the oracle is pinned by (a) every proof it makes it accepts, (b) independent routes -- every B of the sets is b G
for a known b, so R2 = s B - e C must equal (k b) G and C must equal (a b) G --, (c) the three midstates from hashlib and (d) the
rejections.  Then every byte of both bodies on the input sets, the arithmetic behind the hashes with a k and an e no hash will
ever produce, and the stand-alone sanitizer program of tests/emu_dleq, which must exit 0.

BUFFER OVERLAP for p2e_point_lincomb2_batch and the two DLEQ calls is checked here through p2e.lib() with
tests/test_overlap_cpu.py's machinery and a span table of this file's own: the calls name their batch size `count`, so that
file's list (derived from `n` / `m`) leaves them out."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import plonky2_ecdsa_amd as p2e
import dleq_inputs as D
import schnorr_inputs as SI
from test_overlap_cpu import Call, _refused, fake, header_calls  # noqa: F401  (fake is a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "emu_dleq")


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def filled(*shape):
    return np.full(shape, 0xAA, np.uint8)


@pytest.fixture(scope="module")
def emu():
    lib, prog = os.path.join(HERE, "libp2e_emu_dleq.so"), os.path.join(HERE, "dleq_selftest")
    if not (os.path.exists(lib) and os.path.exists(prog)):
        subprocess.check_call(["make", "-s", "-C", HERE])
    L = C.CDLL(lib)
    for name in ("emud_prove", "emud_verify", "emud_lincomb2"):
        getattr(L, name).restype = C.c_long
    return L


# ---- the oracle first ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_msg", [False, True])
def test_the_oracle_accepts_its_own_proofs_and_independent_routes_meet(with_msg):
    """(a) and (b)"""
    good = 0
    for p in D.prover_set(with_msg):
        if p["code"]:
            continue
        a, b, B, C, msg = p["a"], p["b"], p["B"], p["C"], p["msg"]
        A = SI.base_mul(a)
        assert D.verify(A, B, C, p["proof"], msg) == (0, 1)
        assert C == SI.base_mul(a * b % D.N)                                  # C = (a b) G
        e, s = int.from_bytes(p["proof"][:32], "big"), int.from_bytes(p["proof"][32:], "big")
        k = D.nonce(a, p["aux"], A, C, msg)
        R1, R2 = D.verify_points(A, B, C, e, s)
        assert R1 == SI.base_mul(k) and R2 == SI.base_mul(k * b % D.N)        # s B - e C = (k b) G
        good += 1
    assert good == D.N_SET - 10                                                  # the ten flagged places of PROVER_SPECIALS


def test_midstates_are_the_tags_chaining_values(emu):
    """(c)"""
    got = np.zeros(24, np.uint32)
    emu.emud_midstates(_p(got))
    for t, tag in enumerate(D.TAGS):
        assert tuple(int(v) for v in got[8 * t:8 * t + 8]) == D.tag_midstate(tag), tag


def test_the_oracle_rejects_what_it_must():
    """(d): one flipped bit in e, one in s, C + G for C, A and C swapped, a message where none was proven and the reverse"""
    for with_msg in (False, True):
        V = D.verifier_set(with_msg)
        by_kind = {}
        for v in V:
            by_kind.setdefault(v["kind"], []).append(v)
        for kind in ("flip_e", "flip_s", "C_plus_G", "swap_A_C", "s_zero", "e_zero", "e_ge_n"):
            assert by_kind[kind] and all((v["code"], v["valid"]) == (0, 0) for v in by_kind[kind]), kind
        assert all((v["code"], v["valid"]) == (0, 1) for v in by_kind["good"]) and len(by_kind["good"]) > 200
        for v in by_kind["good"][:12]:
            assert D.verify(v["A"], v["B"], v["C"], v["proof"], None if with_msg else b"\x5a" * 32) == (0, 0)


def test_input_sets_contain_what_they_claim():
    for with_msg in (False, True):
        P, V = D.prover_set(with_msg), D.verifier_set(with_msg)
        assert len(P) == len(V) == 257
        assert {p["a"] for p in P} >= {0, 1, 2, D.N - 1, D.N}
        assert [P[i]["code"] for i in (2, 11, 5, 9, 13, 23)] == [8, 8, 5, 4, 3, 8] and P[17]["B"] == D.G and P[19]["B"] == D.neg(D.G)
        assert all(P[i]["code"] == 0 for i in (1, 4, 7, 17, 19))
        assert 0 < sum(p["code"] != 0 for p in P[:64]) < 32 and 0 < sum(v["code"] != 0 for v in V[:64]) < 32      # the first wave is mixed
        want = {"A_neutral": 5, "A_x_ge_p": 3, "A_off_curve_B_neutral": 4, "B_off_curve": 4, "B_x_ge_p": 3, "B_neutral": 5, "B_neutral_C_off_curve": 5,
                "C_x_ge_p": 3, "C_neutral": 5, "C_off_curve": 4, "s_eq_n": 8, "s_max": 8}
        for v in V:
            if v["kind"] in want:
                assert (v["code"], v["valid"]) == (want[v["kind"]], 0), v["kind"]
        assert set(want) <= {v["kind"] for v in V}
        assert any(int.from_bytes(v["proof"][:32], "big") >= D.N for v in V) and any(v["proof"][:32] == bytes(32) for v in V)


# ---- the bodies ---------------------------------------------------------------------------------------------------------------
def emu_prove(emu, A, n, want_c=True):
    proof, cx, cy, err = filled(n + 1, 64), filled(n + 1, 32), filled(n + 1, 32), filled(n + 1)
    bad = emu.emud_prove(_p(A["a"]), _p(A["bx"]), _p(A["by"]), _p(A["aux"]), _p(A["msg"]), _p(proof), _p(cx) if want_c else None,
                         _p(cy) if want_c else None, C.c_size_t(n), _p(err))
    return bad, proof, cx, cy, err


def emu_verify(emu, A, n, msg="own"):
    err, valid = filled(n + 1), filled(n + 1)
    bad = emu.emud_verify(_p(A["ax"]), _p(A["ay"]), _p(A["bx"]), _p(A["by"]), _p(A["cx"]), _p(A["cy"]), _p(A["proof"]),
                          _p(A["msg"] if isinstance(msg, str) else msg), C.c_size_t(n), _p(err), _p(valid))
    return bad, err, valid


@pytest.mark.parametrize("with_msg", [False, True])
def test_prove_writes_the_oracles_bytes_at_every_size(emu, with_msg):
    A = D.prover_arrays(with_msg)
    for n in D.SIZES:
        bad, proof, cx, cy, err = emu_prove(emu, A, n)
        diff = np.nonzero(err[:n] != A["err"][:n])[0]
        assert diff.size == 0, [(int(i), int(err[i]), int(A["err"][i])) for i in diff[:8]]
        assert np.array_equal(proof[:n], A["proof"][:n]) and np.array_equal(cx[:n], A["cx"][:n]) and np.array_equal(cy[:n], A["cy"][:n])
        assert bad == np.count_nonzero(A["err"][:n])
        assert (proof[n] == 0xAA).all() and (cx[n] == 0xAA).all() and (cy[n] == 0xAA).all() and err[n] == 0xAA
        flagged = A["err"][:n] != 0
        assert not proof[:n][flagged].any() and not cx[:n][flagged].any() and not cy[:n][flagged].any()
    bad, proof, cx, cy, err = emu_prove(emu, A, 65, want_c=False)                       # without the share: the same proofs
    assert np.array_equal(proof[:65], A["proof"][:65]) and (cx == 0xAA).all() and (cy == 0xAA).all()


@pytest.mark.parametrize("with_msg", [False, True])
def test_verify_writes_the_oracles_bytes_at_every_size(emu, with_msg):
    A = D.verifier_arrays(with_msg)
    for n in D.SIZES:
        bad, err, valid = emu_verify(emu, A, n)
        diff = np.nonzero((err[:n] != A["err"][:n]) | (valid[:n] != A["valid"][:n]))[0]
        assert diff.size == 0, [(int(i), D.verifier_set(with_msg)[i]["kind"], int(err[i]), int(valid[i])) for i in diff[:8]]
        assert bad == np.count_nonzero(A["err"][:n]) and err[n] == 0xAA and valid[n] == 0xAA
        assert not valid[:n][A["err"][:n] != 0].any()


def test_a_message_where_none_was_proven_and_the_reverse_are_rejected(emu):
    other = np.full((257, 32), 0x5A, np.uint8)
    bad, err, valid = emu_verify(emu, D.verifier_arrays(False), 257, msg=other)
    assert np.array_equal(err[:257], D.verifier_arrays(False)["err"]) and not valid[:257].any()
    bad, err, valid = emu_verify(emu, D.verifier_arrays(True), 257, msg=None)
    assert np.array_equal(err[:257], D.verifier_arrays(True)["err"]) and not valid[:257].any()


def test_prove_then_verify_and_the_share_in_place(emu):
    """the chain of the two bodies; (cx, cy) = (bx, by) gives the same bytes"""
    A = D.prover_arrays(True)
    n = 65
    ok = A["err"][:n] == 0
    ax, ay = D.points([SI.base_mul(p["a"]) if not p["code"] else (0, 0) for p in D.prover_set(True)[:n]])
    B = {k: (v[:n].copy() if v is not None else None) for k, v in A.items()}
    err, proof = filled(n), filled(n, 64)
    emu.emud_prove(_p(B["a"]), _p(B["bx"]), _p(B["by"]), _p(B["aux"]), _p(B["msg"]), _p(proof), _p(B["bx"]), _p(B["by"]), C.c_size_t(n), _p(err))
    assert np.array_equal(B["bx"], A["cx"][:n]) and np.array_equal(B["by"], A["cy"][:n]) and np.array_equal(proof, A["proof"][:n])
    verr, valid = filled(n), filled(n)
    emu.emud_verify(_p(ax), _p(ay), _p(A["bx"][:n].copy()), _p(A["by"][:n].copy()), _p(B["bx"]), _p(B["by"]), _p(proof), _p(B["msg"]), C.c_size_t(n),
                    _p(verr), _p(valid))
    assert np.array_equal(valid == 1, ok) and not verr[ok].any() and verr[~ok].all()


# ---- behind the hashes --------------------------------------------------------------------------------------------------------
def test_the_arithmetic_behind_the_hashes_with_forced_k_and_e(emu):
    cases = D.forced_cases()
    n = len(cases)
    A = [SI.base_mul(a) for a, b, k, e in cases]
    B = [SI.base_mul(b) for a, b, k, e in cases]
    Cs = [SI.base_mul(a * b % D.N) for a, b, k, e in cases]
    a32 = np.stack([D.le32(a) for a, b, k, e in cases])
    (ax, ay), (bx, by), (cx, cy) = D.points(A), D.points(B), D.points(Cs)
    k32 = D.rows([D.b32(k % D.N) for a, b, k, e in cases])                             # (a nonce is reduced before it is used)
    e32 = D.rows([D.b32(e) for a, b, k, e in cases])
    for msg in (None, np.full((n, 32), 0x77, np.uint8)):
        proof, code = filled(n, 64), filled(n)
        emu.emud_prove_with_nonce(_p(a32), _p(ax), _p(ay), _p(bx), _p(by), _p(cx), _p(cy), _p(k32), _p(msg), _p(proof), _p(code), C.c_size_t(n))
        for i, (a, b, k, e) in enumerate(cases):
            want = D.prove_with_nonce(a, A[i], B[i], Cs[i], k % D.N, None if msg is None else msg[i].tobytes())
            assert (int(code[i]), proof[i].tobytes()) == want, (i, k)
        assert sum(1 for c in code if c == D.WIRE_INFINITY) == sum(1 for a, b, k, e in cases if k % D.N == 0) > 0
    s32 = filled(n, 32)
    emu.emud_response(_p(k32), _p(e32), _p(a32), _p(s32), C.c_size_t(n))
    for i, (a, b, k, e) in enumerate(cases):
        assert s32[i].tobytes() == D.b32(D.response(k % D.N, e, a)), i
    # the verifier's points with the forced e and the matching s: R1 = k G, R2 = (k b) G -- and the neutral pair for k = 0
    r1x, r1y, r2x, r2y, ok = filled(n, 32), filled(n, 32), filled(n, 32), filled(n, 32), filled(n)
    emu.emud_verify_points(_p(ax), _p(ay), _p(bx), _p(by), _p(cx), _p(cy), _p(e32), _p(s32), _p(r1x), _p(r1y), _p(r2x), _p(r2y), _p(ok), C.c_size_t(n))
    for i, (a, b, k, e) in enumerate(cases):
        want = D.verify_points(A[i], B[i], Cs[i], e, D.response(k % D.N, e, a))
        assert (want is None) == (k % D.N == 0) and int(ok[i]) == (want is not None), i
        R1, R2 = want if want else ((0, 0), (0, 0))
        if want:
            assert R1 == SI.base_mul(k) and R2 == SI.base_mul(k * b % D.N)
        assert (r1x[i].tobytes(), r1y[i].tobytes(), r2x[i].tobytes(), r2y[i].tobytes()) == tuple(v.to_bytes(32, "little") for v in R1 + R2), i
    assert {e for a, b, k, e in cases} >= {0, D.N, D.N + 5, (1 << 256) - 1}            # e is used modulo n, whatever its size


def test_the_sanitizer_program_exits_zero(emu):
    r = subprocess.run([os.path.join(HERE, "dleq_selftest")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout


# ---- the entry points: declarations, nulls, overlap (BUFFER OVERLAP, include/p2e.h) -------------------------------------------
IN32, OUT32, OUT1 = ("in", 32, "n"), ("out", 32, "n"), ("out", 1, "n")
SH32, SH64, OUT64 = ("shared", 32, "n"), ("shared", 64, "n"), ("out", 64, "n")
# One row per call: its arguments behind ctx, in the header's order (tests/test_overlap_cpu.py explains the entries)
CALLS = {
    "p2e_point_lincomb2_batch": [[0, 0, IN32, SH32, IN32, IN32, IN32, IN32, OUT32, OUT32, ("n",), OUT1]],
    "p2e_dleq_prove_batch": [[SH32, IN32, IN32, SH32, SH32, OUT64, OUT32, OUT32, ("n",), OUT1]],
    "p2e_dleq_verify_batch": [[SH32, SH32, SH32, SH32, SH32, SH32, SH64, SH32, ("n",), OUT1, OUT1]],
}
OPTIONAL = {"p2e_dleq_prove_batch": {"msg32"}, "p2e_dleq_verify_batch": {"msg32"}}
ALLOWED = {"p2e_point_lincomb2_batch": [("outx32", "px32"), ("outy32", "py32"), ("outx32", "qx32"), ("outy32", "qy32"), ("outx32", "a32")],
           "p2e_dleq_prove_batch": [("cx32", "bx32"), ("cy32", "by32")]}
CHECKED_IN = ("in", "shared")


class DleqCall(Call):
    """test_overlap_cpu.Call with the parameter names taken from header_calls(): per_element_calls() does not list a call
    whose batch size is not named n or m"""

    def __init__(self, name, row, n=4):
        self.name, self.row, self.n, self.n_parents = name, row, n, n
        self.pnames = [p for _t, p in header_calls()[name][1:]]
        self.arena = np.zeros(1024 * (len(row) + 2), np.uint8)
        self.slot = np.zeros(1, np.uint64)
        self.base = {k: self.arena.ctypes.data + 1024 * (k + 1) for k, spec in enumerate(row)
                     if isinstance(spec, tuple) and spec[0] in ("in", "out", "shared")}


def all_forms():
    for name, forms in CALLS.items():
        for row in forms:
            yield name, row


def test_the_three_declarations_exist_with_a_count_parameter():
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
                if isinstance(spec, tuple) and spec[0] in ("in", "shared"):
                    assert "const" in typ, (name, pname)
                if spec == ("n",):
                    assert pname == "count"
    text = open(os.path.join(ROOT, "include", "p2e.h")).read()
    assert "has not been checked against the vectors published with BIP-374" in text
    L = p2e.lib()
    assert all(getattr(L, name).restype is C.c_long for name in CALLS)
    assert (p2e.WIRE_COORD_RANGE, p2e.WIRE_NOT_ON_CURVE, p2e.WIRE_INFINITY, p2e.WIRE_SCALAR_RANGE) == \
        (D.WIRE_COORD_RANGE, D.WIRE_NOT_ON_CURVE, D.WIRE_INFINITY, D.WIRE_SCALAR_RANGE)
    for method in ("point_lincomb2_batch", "dleq_prove_batch", "dleq_verify_batch"):
        assert callable(getattr(p2e.Context, method))


def test_disjoint_arguments_pass_the_check_and_meet_the_null_context():
    for name, row in all_forms():
        rc, msg = DleqCall(name, row).run(None)
        assert rc == -1 and msg == "null context", (name, msg)
    # the plan rule of p2e_point_mul_batch: P2E_MUL_PLAN_GLV on P-256 and an unknown plan are refused before the context is looked at
    row = CALLS["p2e_point_lincomb2_batch"][0]
    for curve, plan, word in ((1, 2, "P2E_MUL_PLAN_GLV"), (0, 3, "unknown plan")):
        rc, msg = DleqCall("p2e_point_lincomb2_batch", [curve, plan] + row[2:]).run(None)
        assert rc == -1 and word in msg, msg
    assert DleqCall("p2e_point_lincomb2_batch", [1, 1] + row[2:]).run(None) == (-1, "null context")
    assert DleqCall("p2e_point_lincomb2_batch", [0, 2] + row[2:]).run(None) == (-1, "null context")


def test_a_null_required_pointer_is_named_and_the_nullable_ones_are_accepted():
    required = optional = 0
    for name, row in all_forms():
        call = DleqCall(name, row)
        for k in call.positions("in", "out", "shared"):
            pname = call.pnames[k]
            if name == "p2e_dleq_prove_batch" and pname in ("cx32", "cy32"):
                continue
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
    assert required == 9 + 6 + 9 and optional == 2
    # the share: both of cx32, cy32 or neither
    call = DleqCall("p2e_dleq_prove_batch", CALLS["p2e_dleq_prove_batch"][0])
    cx, cy = call.pnames.index("cx32"), call.pnames.index("cy32")
    assert call.run(None, {cx: 0, cy: 0}) == (-1, "null context")
    for one in (cx, cy):
        rc, msg = call.run(None, {one: 0})
        assert rc == -1 and msg.startswith("null pointer (") and "cx32" in msg and "cy32" in msg, msg


def test_every_output_shifted_onto_an_input_is_refused(fake):
    seen = 0
    for name, row in all_forms():
        call = DleqCall(name, row)
        for i in call.positions(*CHECKED_IN):
            bpe, _count = call.geometry(i)
            for o in call.positions("out"):
                _refused(call, fake, {o: call.base[i] + min(bpe, 4)}, i, o)
                seen += 1
    assert seen == 6 * 3 + 5 * 4 + 8 * 2


def test_every_pair_of_outputs_on_one_buffer_is_refused(fake):
    seen = 0
    for name, row in all_forms():
        call = DleqCall(name, row)
        for a, b in itertools.combinations(call.positions("out"), 2):
            _refused(call, fake, {b: call.base[a]}, a, b)
            seen += 1
    assert seen == 3 + 6 + 1


def test_the_in_place_forms_of_the_header_pass_and_every_other_one_is_refused(fake):
    text = open(os.path.join(ROOT, "include", "p2e.h")).read()
    assert "(cx32, cy32) = (bx32, by32)" in text and "(outx32, outy32) = (px32, py32)" in text and "outx32 = a32" in text
    assert "No in-place form" in text
    for name, row in all_forms():
        call = DleqCall(name, row)
        allowed = {(call.pnames.index(o), call.pnames.index(i)) for o, i in ALLOWED.get(name, ())}
        passed = 0
        for i in call.positions(*CHECKED_IN):
            for o in call.positions("out"):
                same = (o, i) in allowed
                rc, msg = call.run(None if same else fake, {o: call.base[i]})
                assert rc == -1 and (msg == "null context" if same else "overlap" in msg), (name, call.pnames[i], call.pnames[o], msg)
                if not same:
                    assert call.pnames[i] in msg and call.pnames[o] in msg, (name, msg)
                passed += same
        assert passed == len(ALLOWED.get(name, ()))
    # both coordinates at once, as a caller writes it
    call = DleqCall("p2e_point_lincomb2_batch", CALLS["p2e_point_lincomb2_batch"][0])
    ix = call.pnames.index
    for x, y in (("px32", "py32"), ("qx32", "qy32")):
        assert call.run(None, {ix("outx32"): call.base[ix(x)], ix("outy32"): call.base[ix(y)]}) == (-1, "null context")
    call = DleqCall("p2e_dleq_prove_batch", CALLS["p2e_dleq_prove_batch"][0])
    ix = call.pnames.index
    assert call.run(None, {ix("cx32"): call.base[ix("bx32")], ix("cy32"): call.base[ix("by32")]}) == (-1, "null context")


def test_adjacent_buffers_are_no_overlap():
    for name, row in all_forms():
        call = DleqCall(name, row)
        for i in call.positions(*CHECKED_IN):
            bpe, count = call.geometry(i)
            for o in call.positions("out"):
                obpe, ocount = call.geometry(o)
                for at in (call.base[i] + bpe * count, call.base[i] - obpe * ocount):
                    rc, msg = call.run(None, {o: at})
                    assert rc == -1 and msg == "null context", (name, call.pnames[i], call.pnames[o], msg)


def test_count_zero_checks_no_overlap():
    for name, row in all_forms():
        call = DleqCall(name, row, n=0)
        for o in call.positions("out"):
            assert call.run(None, {o: call.base[call.positions(*CHECKED_IN)[1]]}) == (-1, "null context"), name
