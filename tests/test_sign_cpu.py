"""Batch key derivation and signing (include/p2e.h p2e_ecdsa_public_key_batch / p2e_ecdsa_sign_batch) without a GPU.

The kernel bodies of csrc/sign.hpp compiled with g++ (tests/emu_sign, built on demand, -DP2E_F29_BOUNDS: a violated limb
bound of the lazy 29-bit arithmetic aborts the process), in the lane-per-scalar plan and the four-lanes-per-scalar plan (the
quad exchange in its host form), on both curves, on input set E (tests/sign_inputs.py: every table entry, the values around
0 and n, scalars with one non-empty or one empty 16-window group, values >= n) at both ends of the batch plus 300 random
triples.  Every byte of pkx, pky, r, s against expectations that use nothing of the code under test (C oracle fixed-base
walk, Python integers, and oracle/p2e_ref.py's big-int multiplication on a 64-element sample); the flagged sets exactly
{sk = 0 mod n} and {k = 0 mod n}.  The stand-alone sanitizer program of tests/emu_sign must exit 0."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import p2e_ref as R
import plonky2_ecdsa_amd as p2e
import sign_inputs as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "emu_sign")
RANDOM = 300


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def emu():
    lib, prog = os.path.join(HERE, "libp2e_emu_sign.so"), os.path.join(HERE, "sign_selftest")
    if not (os.path.exists(lib) and os.path.exists(prog)):
        subprocess.check_call(["make", "-s", "-C", HERE])
    L = C.CDLL(lib)
    L.emus_public_key.restype = L.emus_sign.restype = C.c_long
    return L


@pytest.fixture(scope="module")
def cases():
    """per curve: raw inputs (ints and bytes) and the expectations, computed once"""
    out = []
    for curve_id, cv in enumerate(S.CURVES):
        total = 2 * len(S.edges(cv)) + RANDOM
        sk, k = S.batch(cv, total, 0x51 + curve_id, shift=1), S.batch(cv, total, 0x61 + curve_id)
        msg = S.batch(cv, total, 0x71 + curve_id, shift=500)
        out.append(dict(sk=sk, k=k, msg=msg, b=[S.pack(v) for v in (msg, sk, k)], keys=S.expect_keys(curve_id, sk),
                        sigs=S.expect_sigs(curve_id, msg, sk, k)))
    return out


def test_input_set_covers_what_it_claims():
    for cv in S.CURVES:
        e = S.edges(cv)
        assert len(set(e[:960])) == 960 and all(sum(1 for j in range(64) if (v >> (4 * j)) & 15) == 1 for v in e[:960])
        groups = lambda v: [(v >> (64 * g)) & ((1 << 64) - 1) != 0 for g in range(4)]
        assert sorted(groups(v).index(True) for v in e[966:970]) == [0, 1, 2, 3] and all(sum(groups(v)) == 1 for v in e[966:970])
        assert sorted(groups(v).index(False) for v in e[970:974]) == [0, 1, 2, 3] and all(sum(groups(v)) == 3 for v in e[970:974])
        assert e[974:] == [cv.n, cv.n + 1, (1 << 256) - 1, 0] and all(0 < v < cv.n for v in e[:974])
        b = S.batch(cv, 2 * len(e) + 5, 1)
        assert b[:len(e)] == e and b[-len(e):] == e[::-1]


@pytest.mark.parametrize("plan", [S.PLAN_LANE, S.PLAN_QUAD])
@pytest.mark.parametrize("curve_id", [0, 1])
def test_bodies_equal_the_expectation_on_every_element(curve_id, plan, emu, cases):
    c = cases[curve_id]
    msg, sk, k = c["b"]
    n = sk.shape[0]
    fill = lambda: np.full((n, 32), 0xAA, np.uint8)
    pkx, pky, r, s, e1, e2 = fill(), fill(), fill(), fill(), np.full(n, 0xAA, np.uint8), np.full(n, 0xAA, np.uint8)
    bad1 = emu.emus_public_key(curve_id, plan, _p(sk), _p(pkx), _p(pky), C.c_size_t(n), _p(e1))
    bad2 = emu.emus_sign(curve_id, plan, _p(msg), _p(sk), _p(k), _p(r), _p(s), C.c_size_t(n), _p(e2))
    wx, wy, we1 = c["keys"]
    wr, ws, we2 = c["sigs"]
    cv = S.CURVES[curve_id]
    assert np.nonzero(we1)[0].tolist() == [i for i, v in enumerate(c["sk"]) if v % cv.n == 0] and len(np.nonzero(we1)[0]) == 4
    assert np.array_equal(e1, we1) and np.array_equal(e2, we2) and bad1 == np.count_nonzero(we1) and bad2 == np.count_nonzero(we2)
    for got, want, what in ((pkx, wx, "pkx"), (pky, wy, "pky"), (r, wr, "r"), (s, ws, "s")):
        diff = np.nonzero((got != want).any(axis=1))[0]
        assert diff.size == 0, (curve_id, plan, what, diff[:8].tolist())


@pytest.mark.parametrize("curve_id", [0, 1])
def test_expectation_equals_big_integer_multiplication_on_a_sample(curve_id, cases):
    """64 elements spread over the batch: the oracle-derived expectation against Curve.mul / ec_mul and Python integers"""
    cv = S.CURVES[curve_id]
    c = cases[curve_id]
    n = len(c["sk"])
    wx, wy, _ = c["keys"]
    wr, ws, _ = c["sigs"]
    px, py, rr, ss = S.unpack(wx), S.unpack(wy), S.unpack(wr), S.unpack(ws)
    mul = (lambda v: R.ec_mul(v, R.G)) if curve_id == 0 else (lambda v: cv.mul(v, cv.g))
    for i in [j * (n - 1) // 63 for j in range(64)]:
        d, kk, m = c["sk"][i] % cv.n, c["k"][i] % cv.n, c["msg"][i] % cv.n
        assert (px[i], py[i]) == (mul(d) if d else (0, 0))
        if kk:
            r = mul(kk)[0] % cv.n
            assert (rr[i], ss[i]) == (r, pow(kk, -1, cv.n) * (m + r * d) % cv.n)
        else:
            assert (rr[i], ss[i]) == (0, 0)


def test_sanitizer_program_exits_zero(emu):
    """tests/emu_sign/sign_selftest: both bodies, both plans, both curves under -fsanitize=address,undefined"""
    res = subprocess.run([os.path.join(HERE, "sign_selftest")], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr


def test_entry_points_exist_and_refuse_misuse_without_a_device():
    L = p2e.lib()
    for name in ("p2e_ecdsa_public_key_batch", "p2e_ecdsa_sign_batch"):
        assert name in p2e.EXPORTS and getattr(L, name).restype is C.c_long
    buf = np.zeros(32, np.uint8)
    assert L.p2e_ecdsa_public_key_batch(None, 0, 0, _p(buf), _p(buf), _p(buf), C.c_size_t(1), _p(buf)) == -1
    assert L.p2e_ecdsa_sign_batch(None, 0, 0, _p(buf), _p(buf), _p(buf), _p(buf), _p(buf), C.c_size_t(1), _p(buf)) == -1
    assert (p2e.ERR_POINT_AT_INFINITY, p2e.SIGN_PLAN_AUTO, p2e.SIGN_PLAN_LANE, p2e.SIGN_PLAN_QUAD) == (64, 0, 1, 2)


@pytest.mark.parametrize("plan", [S.PLAN_LANE, S.PLAN_QUAD])
@pytest.mark.parametrize("curve_id", [0, 1])
def test_the_sixteen_group_patterns(curve_id, plan, emu):
    """all 16 empty / non-empty patterns of the scalar's four 64-bit groups as one small batch (the edge set has none of the
    six with exactly two empty groups, where one level of the quad tree adds and the other only selects)"""
    cv = S.CURVES[curve_id]
    sk_i = S.group_patterns(cv)
    k_i = S.group_patterns(cv, 0x6717)[::-1]
    rng = R.SplitMix64(0x6727 + curve_id)
    msg_i = [rng.below(1 << 256) for _ in sk_i]
    masks = [S.group_mask(v) for v in sk_i]
    assert sorted(set(masks)) == list(range(16)) and sum(1 for m in set(masks) if bin(m).count("1") == 2) == 6
    assert sorted({S.group_mask(v) for v in k_i}) == list(range(16)) and all(v < cv.n for v in sk_i + k_i)
    msg, sk, k = (S.pack(v) for v in (msg_i, sk_i, k_i))
    n = sk.shape[0]
    fill = lambda: np.full((n, 32), 0xAA, np.uint8)
    pkx, pky, r, s, e1, e2 = fill(), fill(), fill(), fill(), np.full(n, 0xAA, np.uint8), np.full(n, 0xAA, np.uint8)
    bad1 = emu.emus_public_key(curve_id, plan, _p(sk), _p(pkx), _p(pky), C.c_size_t(n), _p(e1))
    bad2 = emu.emus_sign(curve_id, plan, _p(msg), _p(sk), _p(k), _p(r), _p(s), C.c_size_t(n), _p(e2))
    wx, wy, we1 = S.expect_keys(curve_id, sk_i)
    wr, ws, we2 = S.expect_sigs(curve_id, msg_i, sk_i, k_i)
    assert np.array_equal(e1, we1) and np.array_equal(e2, we2) and (bad1, bad2) == (2, 2)   # pattern 0000, twice
    for got, want, what in ((pkx, wx, "pkx"), (pky, wy, "pky"), (r, wr, "r"), (s, ws, "s")):
        diff = np.nonzero((got != want).any(axis=1))[0]
        assert diff.size == 0, (curve_id, plan, what, diff[:8].tolist())
