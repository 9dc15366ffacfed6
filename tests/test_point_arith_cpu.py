"""Per-element point arithmetic (include/p2e.h p2e_point_mul_batch, p2e_point_lincomb_batch, p2e_point_add_batch) without a
GPU.

The three kernel bodies of csrc/point_arith.hpp compiled with g++ (tests/emu_point, built on demand, -DP2E_F29_BOUNDS: a
violated limb bound of the lazy 29-bit arithmetic, or a GLV half of 2^128 or more, aborts the process), on both curves and
every plan, on input set X at both ends with 300 elements of set F between (tests/point_arith_inputs.py: nothing there uses
the code under test).  Every byte of the outputs and of err, flagged elements included.  The stand-alone sanitizer program of
tests/emu_point must exit 0."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import p2e_ref as R
import plonky2_ecdsa_amd as p2e
import point_arith_inputs as PI
import sign_inputs as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "emu_point")
F_COUNT = 300
OPS = ("mul", "lincomb", "add")


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def emu():
    lib, prog = os.path.join(HERE, "libp2e_emu_point.so"), os.path.join(HERE, "point_selftest")
    if not (os.path.exists(lib) and os.path.exists(prog)):
        subprocess.check_call(["make", "-s", "-C", HERE])
    L = C.CDLL(lib)
    L.emup_mul.restype = L.emup_lincomb.restype = L.emup_add.restype = C.c_long
    return L


@pytest.fixture(scope="module")
def batches():
    """{(curve, op): (cases, arrays)}: X + F + X, computed once"""
    out = {}
    for curve_id in (0, 1):
        for op in OPS:
            c = PI.batch(curve_id, op, 2 * len(PI.set_x(curve_id, op)) + F_COUNT)
            out[curve_id, op] = (c, PI.arrays(c))
    return out


def run(emu, curve_id, op, plan, a):
    n = a["err"].shape[0]
    ox, oy, err = np.full((n, 32), 0xAA, np.uint8), np.full((n, 32), 0xAA, np.uint8), np.full(n, 0xAA, np.uint8)
    if op == "mul":
        bad = emu.emup_mul(curve_id, plan, _p(a["b"]), _p(a["px"]), _p(a["py"]), _p(ox), _p(oy), C.c_size_t(n), _p(err))
    elif op == "lincomb":
        bad = emu.emup_lincomb(curve_id, plan, _p(a["a"]), _p(a["b"]), _p(a["px"]), _p(a["py"]), _p(ox), _p(oy), C.c_size_t(n), _p(err))
    else:
        bad = emu.emup_add(curve_id, _p(a["px"]), _p(a["py"]), _p(a["qx"]), _p(a["qy"]), _p(ox), _p(oy), C.c_size_t(n), _p(err))
    return ox, oy, err, bad


def test_lambda_and_beta_satisfy_their_defining_equations(emu):
    n, p, cv = R.N, R.P, R.SECP256K1
    lam, beta = np.zeros(32, np.uint8), np.zeros(32, np.uint8)
    emu.emup_glv_constants(_p(lam), _p(beta))
    lam, beta = int.from_bytes(lam.tobytes(), "little"), int.from_bytes(beta.tobytes(), "little")
    # the basis of glv_decompose: (a1, b1), (a2, b2) with b1 = -GLV_MINUS_B1, b2 = a1, determinant n, both in the lattice of lambda
    a1, b1, a2, b2 = R.GLV_A1, -R.GLV_MINUS_B1, R.GLV_A2, R.GLV_B2
    assert a1 * b2 - a2 * b1 == n
    assert lam == -a1 * pow(b1, -1, n) % n == PI.LAMBDA and (a1 + b1 * lam) % n == 0 and (a2 + b2 * lam) % n == 0
    assert (lam * lam + lam + 1) % n == 0 and lam not in (0, 1)
    assert pow(beta, 3, p) == 1 and beta != 1 and beta == PI.BETA
    assert cv.mul(lam, cv.g) == (beta * cv.g[0] % p, cv.g[1])
    # the bound the 64 windows rest on
    assert (a1 + a2) // 2 < 1 << 128 and (-b1 + b2) // 2 < 1 << 128


def test_input_sets_cover_what_they_claim():
    for curve_id, cv in enumerate(PI.CURVES):
        n, p = cv.n, cv.p
        X = {op: PI.set_x(curve_id, op) for op in OPS}
        kinds = lambda op, pre: [c for c in X[op] if c.kind.startswith(pre)]
        ks = {c.b for c in X["mul"]}
        assert ks >= {0, 1, 2, 3, n - 1, n, n + 1, (1 << 256) - 1, (n - 1) // 2, (n + 1) // 2, 1 << 127, (1 << 128) - 1, 1 << 128, (1 << 128) + 1}
        pts = {c.p for c in X["mul"]}
        assert pts >= {cv.g, cv.neg(cv.g), cv.mul(2, cv.g), PI.O}
        for op in OPS:
            assert {c.err for c in X[op]} == {0, PI.WIRE_COORD_RANGE, PI.WIRE_NOT_ON_CURVE, PI.WIRE_INFINITY}
            assert all((c.out == PI.O) == (c.err != 0) for c in X[op])
        bad = dict(PI.invalid_points(curve_id))
        assert bad["x_eq_p"][0] == p and bad["y_eq_p"][1] == p and cv.on_curve((bad["y_eq_p"][0], cv.g[1]))
        assert PI.check(cv, bad["x_ge_p_off_curve"]) == PI.check(cv, bad["x_ge_p_on_curve_mod_p"]) == PI.WIRE_COORD_RANGE
        assert not cv.on_curve((bad["x_ge_p_off_curve"][0] % p, bad["x_ge_p_off_curve"][1]))
        assert PI.check(cv, bad["y_plus_one"]) == PI.WIRE_NOT_ON_CURVE
        assert all(c.err == PI.WIRE_INFINITY for c in kinds("mul", "edge/") if c.b % n == 0)
        assert all(c.err == PI.WIRE_INFINITY for c in X["mul"] if c.kind.endswith("/neutral"))
        # a G + b P
        assert all(c.a == 0 and c.b and c.out == cv.mul(c.b, c.p) for c in kinds("lincomb", "a_zero/"))
        assert all(c.b == 0 and c.out == cv.mul(c.a, cv.g) for c in kinds("lincomb", "b_zero/"))
        assert all(c.err == PI.WIRE_INFINITY for c in kinds("lincomb", "both_") + kinds("lincomb", "opposite"))
        assert all(c.err == 0 and c.out == cv.mul(2 * c.a % n, cv.g) for c in kinds("lincomb", "doubling"))
        opp, dbl = kinds("lincomb", "opposite_G")[0], kinds("lincomb", "doubling_G")[0]
        assert opp.p == dbl.p == cv.g and opp.a == n - opp.b and dbl.a == dbl.b
        assert all(c.p == PI.O and c.err == (0 if c.a else PI.WIRE_INFINITY) for c in kinds("lincomb", "neutral_P"))
        assert len(kinds("lincomb", "invalid_b_zero/")) == 8 and all(c.b == 0 and c.err in (3, 4) for c in kinds("lincomb", "invalid_b_zero/"))
        # P + Q
        assert all(c.out == cv.mul(2, c.p) and c.err == 0 for c in kinds("add", "P_plus_P/"))
        assert all(c.err == PI.WIRE_INFINITY for c in kinds("add", "P_minus_P/") + kinds("add", "O_plus_O"))
        assert all(c.out == c.p for c in kinds("add", "P_plus_O/")) and all(c.out == c.q for c in kinds("add", "O_plus_Q/"))
        assert all(c.err == PI.check(cv, c.p) != 0 for c in kinds("add", "both_invalid/") + kinds("add", "P_invalid/"))
        assert all(c.err == PI.check(cv, c.q) != 0 for c in kinds("add", "Q_invalid"))
        assert {c.err for c in kinds("add", "both_invalid/")} == {3, 4} and any(PI.check(cv, c.p) != PI.check(cv, c.q) for c in kinds("add", "both_invalid/"))
        assert len(kinds("add", "generic")) == 12
    # the GLV kinds spell the decompositions they claim
    g = PI.glv_scalars()
    dec = {k: R.glv_decompose(k) for _kind, k in g}
    assert {k for kind, k in g if kind.startswith("glv_lambda") or kind == "glv_minus_lambda"} == {PI.LAMBDA, PI.LAMBDA + 1, PI.LAMBDA - 1, R.N - PI.LAMBDA, PI.LAMBDA ** 2 % R.N}
    assert {dec[k][2:] for kind, k in g if kind.startswith("glv_signs")} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert all(dec[k][0] == 0 and dec[k][1] for kind, k in g if kind == "glv_k1_zero")
    assert all(dec[k][1] == 0 and dec[k][0] for kind, k in g if kind == "glv_k2_zero")
    assert all(dec[k][0] == dec[k][1] != 0 for kind, k in g if kind == "glv_k1_eq_k2")
    assert all(dec[k][0] >> 126 and dec[k][1] >> 126 for kind, k in g if kind == "glv_top_digits") and len([1 for kind, _k in g if kind == "glv_top_digits"]) == 3


def test_decomposition_identity_and_bound_on_every_secp256k1_scalar(emu, batches):
    ks = np.concatenate([batches[0, "mul"][1]["b"], batches[0, "lincomb"][1]["b"]])
    n = ks.shape[0]
    k1, k2, n1, n2 = np.zeros((n, 32), np.uint8), np.zeros((n, 32), np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    emu.emup_glv_decompose(_p(ks), _p(k1), _p(k2), _p(n1), _p(n2), C.c_size_t(n))
    for k, a, b, s1, s2 in zip(S.unpack(ks), S.unpack(k1), S.unpack(k2), n1.tolist(), n2.tolist()):
        assert a < 1 << 128 and b < 1 << 128, hex(k)
        assert ((-a if s1 else a) + (-b if s2 else b) * PI.LAMBDA - k) % R.N == 0, hex(k)
        assert (a, b, s1, s2) == R.glv_decompose(k % R.N), hex(k)


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("curve_id", [0, 1])
def test_bodies_equal_the_expectation_on_every_element(curve_id, op, emu, batches):
    c, a = batches[curve_id, op]
    assert set(np.unique(a["err"])) == {0, 3, 4, 5} and sum(1 for x in c if x.kind == "F") == F_COUNT
    for plan in PI.PLANS[curve_id] if op != "add" else (0,):
        ox, oy, err, bad = run(emu, curve_id, op, plan, a)
        diff = np.nonzero(err != a["err"])[0]
        assert diff.size == 0, (curve_id, op, plan, "err", [(int(i), c[i].kind, int(err[i]), c[i].err) for i in diff[:8]])
        assert bad == np.count_nonzero(a["err"])
        for got, want, what in ((ox, a["outx"], "outx"), (oy, a["outy"], "outy")):
            diff = np.nonzero((got != want).any(axis=1))[0]
            assert diff.size == 0, (curve_id, op, plan, what, [(int(i), c[i].kind) for i in diff[:8]])


def test_glv_plan_on_p256_and_unknown_plans_are_refused(emu):
    buf = np.zeros(32, np.uint8)
    assert emu.emup_mul(1, PI.PLAN_GLV, _p(buf), _p(buf), _p(buf), _p(buf), _p(buf), C.c_size_t(1), _p(buf)) == -1
    assert emu.emup_lincomb(1, PI.PLAN_GLV, _p(buf), _p(buf), _p(buf), _p(buf), _p(buf), _p(buf), C.c_size_t(1), _p(buf)) == -1
    assert emu.emup_mul(0, 3, _p(buf), _p(buf), _p(buf), _p(buf), _p(buf), C.c_size_t(1), _p(buf)) == -1


def test_sanitizer_program_exits_zero(emu):
    """tests/emu_point/point_selftest under -fsanitize=address,undefined; its compiled-in vectors are drawn from set X as it is now"""
    with open(os.path.join(HERE, "point_vectors.inc")) as f:
        assert f.read() == PI.selftest_vectors(), "tests/emu_point/point_vectors.inc is stale: regenerate it from point_arith_inputs.selftest_vectors()"
    res = subprocess.run([os.path.join(HERE, "point_selftest")], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr


def test_entry_points_exist_and_refuse_misuse_without_a_device():
    L = p2e.lib()
    for name in ("p2e_point_mul_batch", "p2e_point_lincomb_batch", "p2e_point_add_batch"):
        assert name in p2e.EXPORTS and getattr(L, name).restype is C.c_long
    buf = np.zeros(32, np.uint8)
    assert L.p2e_point_mul_batch(None, 0, 0, _p(buf), _p(buf), _p(buf), _p(buf), _p(buf), C.c_size_t(1), _p(buf)) == -1
    assert L.p2e_point_lincomb_batch(None, 0, 0, _p(buf), _p(buf), _p(buf), _p(buf), _p(buf), _p(buf), C.c_size_t(1), _p(buf)) == -1
    assert L.p2e_point_add_batch(None, 0, _p(buf), _p(buf), _p(buf), _p(buf), _p(buf), _p(buf), C.c_size_t(1), _p(buf)) == -1
    assert (p2e.MUL_PLAN_AUTO, p2e.MUL_PLAN_PLAIN, p2e.MUL_PLAN_GLV) == (0, 1, 2)
    assert (p2e.WIRE_COORD_RANGE, p2e.WIRE_NOT_ON_CURVE, p2e.WIRE_INFINITY) == (PI.WIRE_COORD_RANGE, PI.WIRE_NOT_ON_CURVE, PI.WIRE_INFINITY)


def test_ecdh_example_compiles_against_the_header(tmp_path):
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                           os.path.join(ROOT, "examples", "ecdh.c"), "-o", str(tmp_path / "ecdh.o")])
