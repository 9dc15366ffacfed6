"""a P + b Q per element (include/p2e.h p2e_point_lincomb2_batch) without a GPU.

body_point_lincomb2 of csrc/point_arith.hpp compiled with g++ (tests/emu_dleq, built on demand, -DP2E_F29_BOUNDS: a violated
limb bound of the lazy 29-bit arithmetic, or a GLV half of 2^128 or more, aborts the process) against tests/lincomb2_inputs.py:
the header's definition in Python integers, cross-checked through the logarithms of the operands.  Every plan, byte for byte
against the oracle and against each other, at every batch size the GPU tests use, in buffers one element longer than the call
may write."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import p2e_ref as R
import lincomb2_inputs as L2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "emu_dleq")


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def emu():
    lib, prog = os.path.join(HERE, "libp2e_emu_dleq.so"), os.path.join(HERE, "dleq_selftest")
    if not (os.path.exists(lib) and os.path.exists(prog)):
        subprocess.check_call(["make", "-s", "-C", HERE])
    L = C.CDLL(lib)
    L.emud_lincomb2.restype = C.c_long
    return L


def run(emu, curve_id, plan, A, n):
    """the body on the first n elements: (flagged count, outx, outy, err), each one element longer than the call may write"""
    ox, oy, err = np.full((n + 1, 32), 0xAA, np.uint8), np.full((n + 1, 32), 0xAA, np.uint8), np.full(n + 1, 0xAA, np.uint8)
    bad = emu.emud_lincomb2(curve_id, plan, _p(A["a"]), _p(A["b"]), _p(A["px"]), _p(A["py"]), _p(A["qx"]), _p(A["qy"]), _p(ox), _p(oy),
                            C.c_size_t(n), _p(err))
    return bad, ox, oy, err


def assert_equals(A, got, n):
    bad, ox, oy, err = got
    diff = np.nonzero(err[:n] != A["err"][:n])[0]
    assert diff.size == 0, [(int(i), int(err[i]), int(A["err"][i])) for i in diff[:8]]
    assert np.array_equal(ox[:n], A["outx"][:n]) and np.array_equal(oy[:n], A["outy"][:n]) and bad == np.count_nonzero(A["err"][:n])
    assert (ox[n] == 0xAA).all() and (oy[n] == 0xAA).all() and err[n] == 0xAA
    flagged = A["err"][:n] != 0
    assert not ox[:n][flagged].any() and not oy[:n][flagged].any()


@pytest.mark.parametrize("curve_id", [0, 1])
def test_the_expectations_meet_an_independent_multiplication(curve_id):
    """a P + b Q = ((a t_P + b t_Q) mod n) G through the C oracle's fixed-base walk, for every case with valid operands"""
    cs = L2.batch(curve_id, 257)
    assert len(cs) == 257 and L2.cross_check(curve_id, cs) > 200


@pytest.mark.parametrize("curve_id", [0, 1])
def test_the_set_contains_what_it_claims(curve_id):
    cs = L2.cases(curve_id)
    assert len(cs) <= 257
    kinds = {c.kind.split("/")[0] for c in cs}
    want = {"Q_eq_P", "Q_eq_minus_P", "a_eq_b", "a_eq_n_minus_b", "opposite", "doubling", "a_zero", "b_zero", "both_zero", "P_neutral", "Q_neutral",
            "both_neutral", "scalars", "P_invalid", "Q_invalid", "both_invalid", "generic"}
    if curve_id == 0:
        want |= {"Q_eq_lambda_P", "Q_eq_minus_lambda_P", "Q_eq_lambda_P_cancel", "Q_eq_lambda_P_double"}
    assert want <= kinds
    codes = {c.err for c in cs}
    assert codes == {L2.WIRE_OK, L2.WIRE_COORD_RANGE, L2.WIRE_NOT_ON_CURVE, L2.WIRE_INFINITY}
    assert all(c.err == L2.WIRE_INFINITY for c in cs if c.kind.split("/")[0] in ("opposite", "both_zero", "both_neutral", "Q_eq_lambda_P_cancel"))
    assert all(c.err == L2.WIRE_OK for c in cs if c.kind.split("/")[0] in ("doubling", "Q_eq_lambda_P_double", "generic"))
    both = [c for c in cs if c.kind.startswith("both_invalid")]
    assert both and all(c.err == L2.PA.check(L2.CURVES[curve_id], c.p) for c in both)          # P before Q
    first = L2.batch(curve_id, 64)
    assert 0 < sum(c.err != 0 for c in first) < 64                                             # the first wave mixes flagged and good lanes
    if curve_id == 0:                                                                          # halves at the 128-bit bound
        halves = [R.glv_decompose(k)[:2] for k in L2.glv_bound_scalars()]
        assert any(k1 >> 127 for k1, _ in halves) and any(k2 >> 127 for _, k2 in halves) and all(k1 < 1 << 128 and k2 < 1 << 128 for k1, k2 in halves)
        bound = set(L2.glv_bound_scalars())
        assert any(c.a in bound for c in cs) and any(c.b in bound for c in cs)


@pytest.mark.parametrize("curve_id", [0, 1])
def test_every_plan_writes_the_oracles_bytes_at_every_size(emu, curve_id):
    for n in L2.SIZES:
        A = L2.arrays(L2.batch(curve_id, max(n, 1)))
        outs = []
        for plan in L2.PLANS[curve_id]:
            got = run(emu, curve_id, plan, A, n)
            assert_equals(A, got, n)
            outs.append(got)
        for got in outs[1:]:
            assert all(np.array_equal(x, y) for x, y in zip(got[1:], outs[0][1:]))


def test_glv_on_p256_and_unknown_plans_are_refused(emu):
    A = L2.arrays(L2.batch(1, 1))
    for curve_id, plan in ((1, L2.PA.PLAN_GLV), (0, 3), (2, 0)):
        got = run(emu, curve_id, plan, A, 1)
        assert got[0] == -1 and all((x == 0xAA).all() for x in got[1:])


def test_in_place_forms_give_the_same_bytes(emu):
    """(outx, outy) = (px, py), = (qx, qy), outx = a: the body reads every input of element i before its first store"""
    for curve_id in (0, 1):
        A = L2.arrays(L2.batch(curve_id, 65))
        for ox_name, oy_name in (("px", "py"), ("qx", "qy"), ("a", None)):
            B = {k: v.copy() for k, v in A.items()}
            oy = B[oy_name] if oy_name else np.zeros((65, 32), np.uint8)
            err = np.zeros(65, np.uint8)
            emu.emud_lincomb2(curve_id, 0, _p(B["a"]), _p(B["b"]), _p(B["px"]), _p(B["py"]), _p(B["qx"]), _p(B["qy"]), _p(B[ox_name]), _p(oy),
                              C.c_size_t(65), _p(err))
            assert np.array_equal(B[ox_name], A["outx"]) and np.array_equal(oy, A["outy"]) and np.array_equal(err, A["err"])
