"""Public-key recovery and the recoverable signer (include/p2e.h p2e_ecdsa_recover_batch / p2e_ecdsa_sign_recoverable_batch)
without a GPU.

The kernel bodies of csrc/recover.hpp and the recoverable variant of csrc/sign.hpp's signer compiled with g++
(tests/emu_recover, built on demand, -DP2E_F29_BOUNDS: a violated limb bound of the lazy 29-bit arithmetic aborts the
process), on both curves, on input set X at both ends plus 300 elements of set S with their low-s twins between
(tests/recover_inputs.py: nothing there uses the code under test).  Every byte of pkx, pky and err, flagged elements
included.  The stand-alone sanitizer program of tests/emu_recover must exit 0."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import plonky2_ecdsa_amd as p2e
import recover_inputs as RI
import sign_inputs as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "emu_recover")
SIGN_HERE = os.path.join(ROOT, "tests", "emu_sign")
S_TOTAL = 2 * 978 + 300          # the batch of test_sign_cpu.py (same seeds: the point cache is shared)
S_INDICES = list(range(900, 1050)) + list(range(S_TOTAL - 1050, S_TOTAL - 900))   # both copies of E's tail (n, n + 1, 2^256 - 1, 0) and filler


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def emu():
    lib, prog = os.path.join(HERE, "libp2e_emu_recover.so"), os.path.join(HERE, "recover_selftest")
    if not (os.path.exists(lib) and os.path.exists(prog)):
        subprocess.check_call(["make", "-s", "-C", HERE])
    L = C.CDLL(lib)
    L.emur_recover.restype = L.emur_sign_recoverable.restype = C.c_long
    return L


@pytest.fixture(scope="module")
def cases():
    """per curve: X + S + twins of S + X as a list of Case, computed once"""
    out = []
    for curve_id in (0, 1):
        x = list(RI.set_x(curve_id))
        s = RI.set_s(curve_id, S_TOTAL, (0x51 + curve_id, 0x61 + curve_id, 0x71 + curve_id), S_INDICES)
        out.append(x + s + RI.low_s(curve_id, s) + x)
    return out


def test_input_sets_cover_what_they_claim():
    for curve_id, cv in enumerate(RI.CURVES):
        n, p, X = cv.n, cv.p, RI.set_x(curve_id)
        by = lambda kind: [c for c in X if c.kind == kind]
        assert 130 <= len(X) <= 170
        # the constants of the module: abscissas r + n among the small r, non-residue abscissas
        assert [r for r in range(1, RI.OVERFLOW_RANGE[curve_id] + 1) if RI.is_abscissa(cv, r + n)] == RI.OVERFLOW_R[curve_id]
        assert not any(RI.is_abscissa(cv, x) for x in RI.NON_RESIDUE_X[curve_id]) and p % 4 == 3
        # forced cases spell the scalars they claim: u1 = -msg / r, u2 = s / r, and the expectation has its structure
        for c in X:
            if c.u2 is None:
                continue
            rinv = pow(c.r, -1, n)
            assert (-c.msg * rinv % n, c.s * rinv % n) == (c.u1, c.u2) and c.u2 != 0
            want = cv.mul((c.u1 + c.u2 * c.k) % n, cv.g)
            assert (c.pk, c.err) == (((0, 0), RI.ERR_POINT_AT_INFINITY) if want is None else (want, 0)), c.kind
        assert {c.u2 for c in X if c.kind.startswith("u2_small")} == {1, 2, 3, 4, 5, 15, 16, n - 1, n - 2, (1 << 255) % n}
        assert sorted(c.u2 for c in by("u2_digit")) == sorted(d << (2 * w) for w in RI.DIGIT_WINDOWS for d in (1, 2, 3))
        assert all(c.u2 >> 254 == 0 for c in by("u2_zero_top")) and sorted(c.u2 for c in by("u2_top_only")) == [1 << 254, 2 << 254, 3 << 254]
        assert {c.u1 for c in X if c.kind.startswith("u1_edge")} == {0, 1, n - 1}
        assert all(sum(1 for j in range(64) if (c.u1 >> (4 * j)) & 15) == 1 for c in by("u1_nibble")) and len(by("u1_nibble")) == 5
        assert len(by("doubling")) == 4 and all(c.u1 == c.u2 * c.k % n and c.pk == cv.mul(2 * c.u1 % n, cv.g) for c in by("doubling"))
        assert len(by("neutral")) == 4 and all((c.u1 + c.u2 * c.k) % n == 0 and c.err == RI.ERR_POINT_AT_INFINITY for c in by("neutral"))
        assert {c.v & 1 for c in X if c.err == 0} == {0, 1} and {c.v for c in X if c.err == 0} >= {0, 1, 2, 3}
        over = by("overflow")
        assert {c.r for c in over if c.err == 0} == set(RI.OVERFLOW_R[curve_id]) and all(c.v & 2 for c in over)
        assert {c.r for c in by("no_overflow")} == {c.r for c in over} and {c.err for c in by("no_overflow")} == {0, RI.ERR_NOT_RECOVERABLE}
        assert {c.r for c in by("non_residue")} == set(RI.NON_RESIDUE_X[curve_id])
        assert all(c.err == RI.ERR_NOT_RECOVERABLE for c in by("non_residue") + by("x_ge_p") + by("r_range") + by("s_range") + by("v_range"))
        assert len(by("x_ge_p")) == 6 and {c.r for c in by("r_range")} == {n, (1 << 256) - 1, 0} and {c.s for c in by("s_range")} >= {n, 0}
        assert {c.v for c in by("v_range")} >= {4, 27, 255}
        good = by("well_formed")[0]
        assert good.err == 0 and all(c.msg >= n and c.err == 0 for c in by("msg_ge_n"))
        assert [c.pk for c in by("msg_ge_n")] == [c.pk for c in by("msg_reduced")]
        # set S: the flagged kinds the batch's own edges give, and twins with the same expectation
        s = RI.set_s(curve_id, S_TOTAL, (0x51 + curve_id, 0x61 + curve_id, 0x71 + curve_id), S_INDICES)
        kinds = [c.kind for c in s]
        assert kinds.count("S_k_zero") == 4 and kinds.count("S_sk_zero") >= 2 and kinds.count("S") >= 280 and len(s) == 300
        t = RI.low_s(curve_id, s)
        assert all((a.r, a.s + b.s, a.v ^ b.v, a.pk, a.err) == (b.r, n, 1, b.pk, b.err) for a, b in zip(s, t))


@pytest.mark.parametrize("curve_id", [0, 1])
def test_body_equals_the_expectation_on_every_element(curve_id, emu, cases):
    c = cases[curve_id]
    a = RI.arrays(c)
    n = len(c)
    pkx, pky, err = np.full((n, 32), 0xAA, np.uint8), np.full((n, 32), 0xAA, np.uint8), np.full(n, 0xAA, np.uint8)
    bad = emu.emur_recover(curve_id, _p(a["msg"]), _p(a["r"]), _p(a["s"]), _p(a["v"]), _p(pkx), _p(pky), C.c_size_t(n), _p(err))
    diff = np.nonzero(err != a["err"])[0]
    assert diff.size == 0, (curve_id, "err", [(int(i), c[i].kind, int(err[i]), c[i].err) for i in diff[:8]])
    assert bad == np.count_nonzero(a["err"]) and set(np.unique(a["err"])) == {0, RI.ERR_POINT_AT_INFINITY, RI.ERR_NOT_RECOVERABLE}
    for got, want, what in ((pkx, a["pkx"], "pkx"), (pky, a["pky"], "pky")):
        diff = np.nonzero((got != want).any(axis=1))[0]
        assert diff.size == 0, (curve_id, what, [(int(i), c[i].kind) for i in diff[:8]])


@pytest.mark.parametrize("plan", [S.PLAN_LANE, S.PLAN_QUAD])
@pytest.mark.parametrize("curve_id", [0, 1])
def test_recoverable_signer_equals_the_plain_signer_and_v_is_as_expected(curve_id, plan, emu):
    if not os.path.exists(os.path.join(SIGN_HERE, "libp2e_emu_sign.so")):
        subprocess.check_call(["make", "-s", "-C", SIGN_HERE])
    plain = C.CDLL(os.path.join(SIGN_HERE, "libp2e_emu_sign.so"))
    plain.emus_sign.restype = C.c_long
    cv = S.CURVES[curve_id]
    seeds = (0x51 + curve_id, 0x61 + curve_id, 0x71 + curve_id)
    sk, k = S.batch(cv, S_TOTAL, seeds[0], shift=1), S.batch(cv, S_TOTAL, seeds[1])
    msg = S.batch(cv, S_TOTAL, seeds[2], shift=500)
    msg, sk, k = [[v[i] for i in S_INDICES] for v in (msg, sk, k)]
    b = [S.pack(v) for v in (msg, sk, k)]
    n = len(msg)
    fill = lambda: np.full((n, 32), 0xAA, np.uint8)
    r0, s0, e0, r1, s1, e1, v1 = fill(), fill(), np.full(n, 0xAA, np.uint8), fill(), fill(), np.full(n, 0xAA, np.uint8), np.full(n, 0xAA, np.uint8)
    bad0 = plain.emus_sign(curve_id, plan, _p(b[0]), _p(b[1]), _p(b[2]), _p(r0), _p(s0), C.c_size_t(n), _p(e0))
    bad1 = emu.emur_sign_recoverable(curve_id, plan, _p(b[0]), _p(b[1]), _p(b[2]), _p(r1), _p(s1), _p(v1), C.c_size_t(n), _p(e1))
    assert bad0 == bad1 == 4 and np.array_equal(r0, r1) and np.array_equal(s0, s1) and np.array_equal(e0, e1)
    pts = S.base_points(curve_id, [kk % cv.n for kk in k])
    want_v = [0 if kk % cv.n == 0 else (pts[kk % cv.n][1] & 1) | (2 if pts[kk % cv.n][0] >= cv.n else 0) for kk in k]
    assert v1.tolist() == want_v


def test_sanitizer_program_exits_zero(emu):
    """tests/emu_recover/recover_selftest under -fsanitize=address,undefined; its compiled-in vectors are set X as it is now"""
    with open(os.path.join(HERE, "recover_vectors.inc")) as f:
        assert f.read() == RI.selftest_vectors(), "tests/emu_recover/recover_vectors.inc is stale: regenerate it from recover_inputs.selftest_vectors()"
    res = subprocess.run([os.path.join(HERE, "recover_selftest")], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr


def test_entry_points_exist_and_refuse_misuse_without_a_device():
    L = p2e.lib()
    for name in ("p2e_ecdsa_recover_batch", "p2e_ecdsa_sign_recoverable_batch"):
        assert name in p2e.EXPORTS and getattr(L, name).restype is C.c_long
    buf = np.zeros(32, np.uint8)
    assert L.p2e_ecdsa_recover_batch(None, 0, _p(buf), _p(buf), _p(buf), _p(buf), _p(buf), _p(buf), C.c_size_t(1), _p(buf)) == -1
    assert L.p2e_ecdsa_sign_recoverable_batch(None, 0, 0, _p(buf), _p(buf), _p(buf), _p(buf), _p(buf), _p(buf), C.c_size_t(1), _p(buf)) == -1
    assert (p2e.ERR_NOT_RECOVERABLE, p2e.ERR_POINT_AT_INFINITY) == (128, 64)
