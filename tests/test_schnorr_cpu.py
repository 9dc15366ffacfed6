"""BIP-340 Schnorr signatures (include/p2e.h p2e_schnorr_public_key_batch and the four calls after it) without a GPU.

The bodies of csrc/schnorr.hpp compiled with g++ (tests/emu_schnorr, built on demand, -DP2E_F29_BOUNDS: a violated limb bound
of the lazy 29-bit arithmetic aborts the process) against the oracle of tests/schnorr_inputs.py, a restatement of the standard
in Python integers and hashlib that uses nothing under test: every byte of the four per-element bodies, the three tag
midstates, the inner signer at k' = 0, and the aggregate's 2 n + 1 terms word for word -- which are then summed by the
oracle for the verdict.  The stand-alone sanitizer program of tests/emu_schnorr must exit 0."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import plonky2_ecdsa_amd as p2e
import schnorr_inputs as SI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "emu_schnorr")


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def emu():
    lib, prog = os.path.join(HERE, "libp2e_emu_schnorr.so"), os.path.join(HERE, "schnorr_selftest")
    if not (os.path.exists(lib) and os.path.exists(prog)):
        subprocess.check_call(["make", "-s", "-C", HERE])
    L = C.CDLL(lib)
    for name in ("emusch_public_key", "emusch_sign", "emusch_verify", "emusch_xonly_decode", "emusch_agg_prepare"):
        getattr(L, name).restype = C.c_long
    return L


def term_arrays(scalars, points):
    """the oracle's 2 n + 1 terms in the MSM's input layout: (k, px, py), each (2 n + 1, 32) little-endian"""
    k = np.stack([SI.le32(s) for s in scalars])
    px = np.stack([SI.le32(p[0] if p else 0) for p in points])
    py = np.stack([SI.le32(p[1] if p else 0) for p in points])
    return k, px, py


def terms_of(k, px, py):
    """the arrays back as integers and points, for the oracle's sum"""
    val = lambda row: int.from_bytes(row.tobytes(), "little")
    pts = [None if not (val(x) or val(y)) else (val(x), val(y)) for x, y in zip(px, py)]
    return [val(r) for r in k], pts


def test_input_sets_contain_what_they_claim():
    S, V = SI.signer_set(), SI.verifier_set()
    assert len(S) == len(V) == 257 == SI.LENGTHS[-1] and SI.LENGTHS == (1, 63, 64, 65, 257)
    # the known answer, restated by the oracle itself
    assert (S[0].sk, S[0].msg, S[0].aux) == (SI.KNOWN_SK, bytes(32), bytes(32)) and S[0].pk == SI.KNOWN_PK and S[0].sig == SI.KNOWN_SIG
    assert SI.verify(bytes(32), SI.KNOWN_PK, SI.KNOWN_SIG) == (0, 1)
    # keys and nonces of both parities: d and k negated or not, in every combination
    assert {(s.key_odd, s.nonce_odd) for s in S if s.err == 0} == {(False, False), (False, True), (True, False), (True, True)}
    kinds = {s.kind: s for s in S}
    assert int.from_bytes(kinds["sk_one"].sk, "big") == 1 and int.from_bytes(kinds["sk_n_minus_1"].sk, "big") == SI.N - 1
    assert kinds["sk_one"].err == kinds["sk_n_minus_1"].err == 0 and kinds["sk_one"].pk == SI.b32(SI.G[0]) == kinds["sk_n_minus_1"].pk
    assert [int.from_bytes(kinds[k].sk, "big") for k in ("sk_zero", "sk_n", "sk_max")] == [0, SI.N, 2**256 - 1]
    for k in ("sk_zero", "sk_n", "sk_max"):
        assert kinds[k].err == kinds[k].pk_err == SI.WIRE_SCALAR_RANGE and kinds[k].pk == bytes(32) and kinds[k].sig == bytes(64)
    assert all(SI.verify(s.msg, s.pk, s.sig) == (0, 1) for s in S if s.err == 0)         # what the oracle signs, it accepts
    # the verifier's cases, each with the (err, valid) the issue states
    want = {"known": (0, 1), "valid": (0, 1), "s_negated": (0, 0), "nonce_not_negated": (0, 0), "x_neutral": (0, 0), "r_off_curve": (0, 0),
            "r_eq_p": (SI.WIRE_COORD_RANGE, 0), "r_max": (SI.WIRE_COORD_RANGE, 0), "s_eq_n": (SI.WIRE_SCALAR_RANGE, 0),
            "s_max": (SI.WIRE_SCALAR_RANGE, 0), "s_zero": (0, 0), "pk_zero": (SI.WIRE_NOT_ON_CURVE, 0),
            "pk_off_curve": (SI.WIRE_NOT_ON_CURVE, 0), "pk_plus_p": (SI.WIRE_COORD_RANGE, 0), "pk_small": (0, 0), "flip_msg": (0, 0),
            "flip_r": (0, 0), "flip_s": (0, 0)}
    seen = {c.kind for c in V}
    assert seen == set(want) | {"flip_pk"}
    for c in V:
        if c.kind == "flip_pk":                       # a flipped key bit lands on the curve or off it: never valid
            assert (c.err, c.valid) in ((0, 0), (SI.WIRE_NOT_ON_CURVE, 0))
        else:
            assert (c.err, c.valid) == want[c.kind], c.kind
    by = {c.kind: c for c in V}
    r_of, s_of, pk_of = (lambda c: int.from_bytes(c.sig[:32], "big")), (lambda c: int.from_bytes(c.sig[32:], "big")), (lambda c: int.from_bytes(c.pk, "big"))
    assert [r_of(by["r_eq_p"]), r_of(by["r_max"]), s_of(by["s_eq_n"]), s_of(by["s_max"]), s_of(by["s_zero"]), pk_of(by["pk_zero"])] == \
        [SI.P, 2**256 - 1, SI.N, 2**256 - 1, 0, 0]
    assert SI.lift_x(r_of(by["r_off_curve"])) is None and SI.lift_x(pk_of(by["pk_off_curve"])) is None
    assert pk_of(by["pk_plus_p"]) == SI.P + pk_of(by["pk_small"]) and SI.lift_x(pk_of(by["pk_small"])) is not None
    # nonce_not_negated: X = R has odd y;  x_neutral: s G = e P
    c = by["nonce_not_negated"]
    Pt, e = SI.lift_x(pk_of(c)), SI.challenge(r_of(c), pk_of(c), c.msg)
    X = SI._affine(SI._jadd(SI._gmul(s_of(c)), SI._jmul(SI.N - e, Pt)))
    assert X[0] == r_of(c) and X[1] & 1
    c = by["x_neutral"]
    Pt, e = SI.lift_x(pk_of(c)), SI.challenge(r_of(c), pk_of(c), c.msg)
    assert SI._jadd(SI._gmul(s_of(c)), SI._jmul(SI.N - e, Pt)) is None
    # the aggregate cases: what each claims, and the two restatements agree
    assert SI.AGG_SIZES == (0, 1, 2, 65, 1000) and len(set(SI.AGG_SEEDS)) == 2
    for n in (0, 1, 2, 65):
        cases = SI.aggregate_cases(n)
        assert set(cases) >= ({"all_valid"} if n == 0 else {"all_valid", "bad_first", "bad_middle", "bad_last", "err_r_eq_p", "err_s_eq_n",
                                                            "err_pk_off_curve", "err_pk_plus_p", "err_r_off_curve"})
        assert (n < 2) or {"delta_pair", "swapped_s"} <= set(cases)
        for name, (m, p, s) in cases.items():
            verdict, errs = SI.aggregate_expected(m, p, s)
            assert verdict == (name == "all_valid") and (sum(1 for e in errs if e) == 1) == name.startswith("err_"), (n, name)
    m, p, s = SI.aggregate_cases(2)["swapped_s"]
    assert p[0] == p[1] and s[0][32:] == SI.valid_batch(2)[1][2][32:]
    m, p, s = SI.aggregate_cases(2)["delta_pair"]             # the plain sum of the s values is unchanged
    assert sum(int.from_bytes(x[32:], "big") for x in s) % SI.N == sum(int.from_bytes(x[2][32:], "big") for x in SI.valid_batch(2)) % SI.N


def test_python_compression_is_sha256():
    """the midstate helper the next test relies on, against hashlib"""
    import hashlib
    for data in (b"", b"abc", bytes(range(200)), b"\xff" * 119, b"x" * 64):
        assert SI.sha256_from_midstate(SI.SHA256_IV, 0, data) == hashlib.sha256(data).digest()
    for tag in SI.TAGS:
        for data in (b"", bytes(32), bytes(range(96))):
            assert SI.sha256_from_midstate(SI.tag_midstate(tag), 64, data) == SI.tagged_hash(tag, data)


def test_tag_midstates(emu):
    for tag_id, tag in enumerate(SI.TAGS):
        got = (C.c_uint32 * 8)()
        emu.emusch_midstate(tag_id, got)
        assert tuple(got) == SI.tag_midstate(tag), tag


@pytest.mark.parametrize("n", SI.LENGTHS)
def test_public_key_and_sign_bodies_equal_the_oracle(n, emu):
    a = SI.signer_arrays()
    sk, msg, aux = a["sk"][:n].copy(), a["msg"][:n].copy(), a["aux"][:n].copy()
    pk, err = np.full((n + 1, 32), 0xAA, np.uint8), np.full(n + 1, 0xAA, np.uint8)
    bad = emu.emusch_public_key(_p(sk), _p(pk), C.c_size_t(n), _p(err))
    assert np.array_equal(pk[:n], a["pk"][:n]) and np.array_equal(err[:n], a["pk_err"][:n]) and bad == np.count_nonzero(a["pk_err"][:n])
    assert (pk[n] == 0xAA).all() and err[n] == 0xAA
    sig, err = np.full((n + 1, 64), 0xAA, np.uint8), np.full(n + 1, 0xAA, np.uint8)
    bad = emu.emusch_sign(_p(msg), _p(sk), _p(aux), _p(sig), C.c_size_t(n), _p(err))
    diff = np.nonzero((sig[:n] != a["sig"][:n]).any(axis=1))[0]
    assert diff.size == 0, [(int(i), SI.signer_set()[i].kind) for i in diff[:8]]
    assert np.array_equal(err[:n], a["err"][:n]) and bad == np.count_nonzero(a["err"][:n]) and (sig[n] == 0xAA).all() and err[n] == 0xAA


@pytest.mark.parametrize("n", SI.LENGTHS)
def test_verify_and_decode_bodies_equal_the_oracle(n, emu):
    a = SI.verifier_arrays()
    msg, pk, sig = a["msg"][:n].copy(), a["pk"][:n].copy(), a["sig"][:n].copy()
    err, valid = np.full(n + 1, 0xAA, np.uint8), np.full(n + 1, 0xAA, np.uint8)
    bad = emu.emusch_verify(_p(msg), _p(pk), _p(sig), C.c_size_t(n), _p(err), _p(valid))
    diff = np.nonzero((err[:n] != a["err"][:n]) | (valid[:n] != a["valid"][:n]))[0]
    assert diff.size == 0, [(int(i), SI.verifier_set()[i].kind, int(err[i]), int(valid[i])) for i in diff[:8]]
    assert bad == np.count_nonzero(a["err"][:n]) and err[n] == 0xAA and valid[n] == 0xAA
    dx, dy, err = np.full((n + 1, 32), 0xAA, np.uint8), np.full((n + 1, 32), 0xAA, np.uint8), np.full(n + 1, 0xAA, np.uint8)
    bad = emu.emusch_xonly_decode(_p(pk), _p(dx), _p(dy), C.c_size_t(n), _p(err))
    assert np.array_equal(dx[:n], a["dx"][:n]) and np.array_equal(dy[:n], a["dy"][:n]) and np.array_equal(err[:n], a["derr"][:n])
    assert bad == np.count_nonzero(a["derr"][:n]) and (dx[n] == 0xAA).all() and (dy[n] == 0xAA).all() and err[n] == 0xAA
    assert all(int(y[0]) % 2 == 0 for y in dy[:n])


def test_inner_signer_refuses_a_zero_nonce(emu):
    s = SI.signer_set()[0]
    d, px = np.frombuffer(SI.b32(s.d), np.uint8).copy(), np.frombuffer(SI.b32(s.px), np.uint8).copy()
    msg, sig = np.frombuffer(s.msg, np.uint8).copy(), np.full(64, 0xAA, np.uint8)
    assert emu.emusch_sign_with_nonce(_p(d), _p(px), _p(msg), _p(np.zeros(32, np.uint8)), _p(sig)) == SI.WIRE_INFINITY == p2e.WIRE_INFINITY
    assert SI.sign_with_nonce(s.d, s.px, s.msg, 0) == (SI.WIRE_INFINITY, bytes(64))
    k0 = np.frombuffer(SI.b32(s.k0), np.uint8).copy()                      # and with the real nonce it is the known answer
    assert emu.emusch_sign_with_nonce(_p(d), _p(px), _p(msg), _p(k0), _p(sig)) == 0 and sig.tobytes() == SI.KNOWN_SIG


def run_prepare(emu, msgs, pks, sigs, seed, with_err=True):
    n = len(msgs)
    msg = SI.rows(list(msgs)) if n else np.zeros((1, 32), np.uint8)
    pk = SI.rows(list(pks)) if n else np.zeros((1, 32), np.uint8)
    sig = SI.rows(list(sigs), 64) if n else np.zeros((1, 64), np.uint8)
    t = 2 * n + 1
    k, px, py = (np.full((t + 1, 32), 0xAA, np.uint8) for _ in range(3))
    err = np.full(n + 1, 0xAA, np.uint8)
    bad = emu.emusch_agg_prepare(_p(msg), _p(pk), _p(sig), _p(np.frombuffer(seed, np.uint8).copy()), C.c_size_t(n), _p(k), _p(px), _p(py),
                                 _p(err) if with_err else None)
    assert (k[t] == 0xAA).all() and (px[t] == 0xAA).all() and (py[t] == 0xAA).all() and err[n] == 0xAA
    return k[:t], px[:t], py[:t], err[:n], bad


def check_aggregate(emu, n, name, seed):
    msgs, pks, sigs = SI.aggregate_cases(n)[name]
    expected, errs = SI.aggregate_expected(msgs, pks, sigs)
    o_errs, scalars, points = SI.aggregate_terms(msgs, pks, sigs, seed)
    assert o_errs == errs
    k, px, py, err, bad = run_prepare(emu, msgs, pks, sigs, seed)
    wk, wx, wy = term_arrays(scalars, points)
    assert np.array_equal(k, wk) and np.array_equal(px, wx) and np.array_equal(py, wy), (n, name)
    assert err.tolist() == errs and bad == sum(1 for e in errs if e)
    # the body's own terms, summed by the oracle: the verdict
    got_scalars, got_points = terms_of(k, px, py)
    status = 1 if SI.sum_is_neutral(got_scalars, got_points) else 0          # MSM_NEUTRAL = 1, MSM_OK = 0
    assert emu.emusch_agg_verdict(status, C.c_ulonglong(bad)) == expected, (n, name)
    assert expected == (name == "all_valid")


@pytest.mark.parametrize("seed", range(2))
@pytest.mark.parametrize("n", [0, 1, 2, 65])
def test_aggregate_terms_equal_the_oracle_and_sum_to_the_verdict(n, seed, emu):
    for name in SI.aggregate_cases(n):
        check_aggregate(emu, n, name, SI.AGG_SEEDS[seed])


@pytest.mark.parametrize("name", ["all_valid", "bad_middle"])
def test_aggregate_terms_at_one_thousand(name, emu):
    """four blocks of partial sums; the oracle's sum over 2001 terms takes a few seconds, so two cases and one seed"""
    check_aggregate(emu, 1000, name, SI.AGG_SEEDS[0])


def test_aggregate_on_the_verifier_set_and_without_err(emu):
    """every structural error at once, and err == NULL writes the same terms"""
    V = SI.verifier_set()
    msgs, pks, sigs = [c.msg for c in V], [c.pk for c in V], [c.sig for c in V]
    errs, scalars, points = SI.aggregate_terms(msgs, pks, sigs, SI.AGG_SEEDS[1])
    assert set(errs) == {0, SI.WIRE_COORD_RANGE, SI.WIRE_NOT_ON_CURVE, SI.WIRE_SCALAR_RANGE}
    assert errs[[c.kind for c in V].index("r_off_curve")] == SI.WIRE_NOT_ON_CURVE
    k, px, py, err, bad = run_prepare(emu, msgs, pks, sigs, SI.AGG_SEEDS[1])
    wk, wx, wy = term_arrays(scalars, points)
    assert np.array_equal(k, wk) and np.array_equal(px, wx) and np.array_equal(py, wy) and err.tolist() == errs
    k2, px2, py2, _, bad2 = run_prepare(emu, msgs, pks, sigs, SI.AGG_SEEDS[1], with_err=False)
    assert np.array_equal(k, k2) and np.array_equal(px, px2) and np.array_equal(py, py2) and bad == bad2 == sum(1 for e in errs if e)
    assert all(SI.randomizer(SI.AGG_SEEDS[1], i) < 2**128 for i in range(len(V)))
    assert all(p is None or p[1] & 1 for p in points[1:])                      # the odd root: -R and -P


def test_sanitizer_program_exits_zero(emu, tmp_path):
    """tests/emu_schnorr/schnorr_selftest under -fsanitize=address,undefined over both sets, in allocations of exactly their size"""
    s, v = SI.signer_arrays(), SI.verifier_arrays()
    V = SI.verifier_set()
    seed = SI.AGG_SEEDS[0]
    errs, scalars, points = SI.aggregate_terms([c.msg for c in V], [c.pk for c in V], [c.sig for c in V], seed)
    path = tmp_path / "schnorr_vectors.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<QQ", len(s["err"]), len(v["err"])))
        for a in (s["msg"], s["sk"], s["aux"], s["pk"], s["pk_err"], s["sig"], s["err"], v["msg"], v["pk"], v["sig"], v["err"], v["valid"],
                  v["dx"], v["dy"], v["derr"], np.frombuffer(seed, np.uint8), np.array(errs, np.uint8), *term_arrays(scalars, points)):
            f.write(np.ascontiguousarray(a).tobytes())
    res = subprocess.run([os.path.join(HERE, "schnorr_selftest"), str(path)], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr


def test_entry_points_exist_and_refuse_misuse_without_a_device():
    L = p2e.lib()
    names = ("p2e_schnorr_public_key_batch", "p2e_schnorr_sign_batch", "p2e_schnorr_verify_batch", "p2e_xonly_decode_batch",
             "p2e_schnorr_verify_aggregate")
    for name in names:
        assert name in p2e.EXPORTS and getattr(L, name).restype is C.c_long
    buf = np.zeros(64, np.uint8)
    assert L.p2e_schnorr_public_key_batch(None, _p(buf), _p(buf), C.c_size_t(1), _p(buf)) == -1
    assert L.p2e_schnorr_sign_batch(None, _p(buf), _p(buf), _p(buf), _p(buf), C.c_size_t(1), _p(buf)) == -1
    assert L.p2e_schnorr_verify_batch(None, _p(buf), _p(buf), _p(buf), C.c_size_t(1), _p(buf), _p(buf)) == -1
    assert L.p2e_xonly_decode_batch(None, _p(buf), _p(buf), _p(buf), C.c_size_t(1), _p(buf)) == -1
    assert L.p2e_schnorr_verify_aggregate(None, _p(buf), _p(buf), _p(buf), C.c_size_t(1), _p(buf), C.c_uint(0), _p(buf), None) == -1
    assert (p2e.WIRE_COORD_RANGE, p2e.WIRE_NOT_ON_CURVE, p2e.WIRE_INFINITY, p2e.WIRE_SCALAR_RANGE) == \
        (SI.WIRE_COORD_RANGE, SI.WIRE_NOT_ON_CURVE, SI.WIRE_INFINITY, SI.WIRE_SCALAR_RANGE)


def test_example_compiles_against_the_header(tmp_path):
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                           os.path.join(ROOT, "examples", "schnorr_verify.c"), "-o", str(tmp_path / "schnorr_verify.o")])
