"""a P + b Q per element on the GPU (include/p2e.h p2e_point_lincomb2_batch) through the C ABI.

Expectations come from tests/lincomb2_inputs.py alone (Python integers), and a second time from the device itself:
p2e_point_mul_batch, p2e_point_mul_batch and p2e_point_add_batch on the same operands must write the same bytes.  Every byte of
every element is compared; output buffers are pre-filled with 0xAA so that an unwritten byte shows, and hold one element more
than the call may write.

Shapes: count = 0, 1, 63, 64, 65 and 257 (nothing, one lane, a wave less one, a wave, a wave plus one, a block plus one), every
plan on both curves.  The set puts Q = +-P, Q = +-lambda P, neutral operands, zero scalars and invalid points into the first
wave beside ordinary lanes, so the additions of one wave take every branch of the complete formula."""
import ctypes as C

import numpy as np
import pytest
import torch

import plonky2_ecdsa_amd as p2e
import lincomb2_inputs as L2

pytestmark = pytest.mark.gpu
size = C.c_size_t


@pytest.fixture(scope="module")
def hctx():
    return p2e.Context(device=0, host_pointers=True)


def filled(*shape):
    return np.full(shape, 0xAA, np.uint8)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def rows_of(a, n):
    """the first n rows of an input array as its own buffer; one dummy row for n = 0 (a pointer the call must not follow)"""
    return np.ascontiguousarray(a[:max(n, 1)]).copy()


def call(hctx, curve_id, plan, A, n):
    ox, oy, err = filled(n + 1, 32), filled(n + 1, 32), filled(n + 1)
    rc = hctx._L.p2e_point_lincomb2_batch(hctx._h, curve_id, C.c_uint(plan), _p(rows_of(A["a"], n)), _p(rows_of(A["b"], n)), _p(rows_of(A["px"], n)),
                                          _p(rows_of(A["py"], n)), _p(rows_of(A["qx"], n)), _p(rows_of(A["qy"], n)), _p(ox), _p(oy), size(n), _p(err))
    return rc, ox, oy, err


def assert_equals(A, got, n):
    rc, ox, oy, err = got
    assert rc >= 0, p2e.lib().p2e_last_error()
    diff = np.nonzero((err[:n] != A["err"][:n]) | (ox[:n] != A["outx"][:n]).any(axis=1) | (oy[:n] != A["outy"][:n]).any(axis=1))[0]
    assert diff.size == 0, [(int(i), int(err[i]), int(A["err"][i])) for i in diff[:8]]
    assert rc == np.count_nonzero(A["err"][:n]) and (ox[n] == 0xAA).all() and (oy[n] == 0xAA).all() and err[n] == 0xAA
    flagged = A["err"][:n] != 0
    assert not ox[:n][flagged].any() and not oy[:n][flagged].any()


@pytest.mark.parametrize("n", L2.SIZES)
@pytest.mark.parametrize("curve_id", [0, 1])
def test_every_plan_equals_the_oracle(curve_id, n, hctx):
    A = L2.arrays(L2.batch(curve_id, max(n, 1)))
    for plan in L2.PLANS[curve_id]:
        assert_equals(A, call(hctx, curve_id, plan, A, n), n)


@pytest.mark.parametrize("curve_id", [0, 1])
def test_every_plan_equals_mul_mul_add_on_the_device(curve_id, hctx):
    n = 257
    cs = L2.batch(curve_id, n)
    A = L2.arrays(cs)
    assert {c.err for c in cs} == {0, 3, 4, 5}
    ax, ay, e1, _ = hctx.point_mul_batch(A["a"].copy(), A["px"].copy(), A["py"].copy(), curve=curve_id)
    bx, by, e2, _ = hctx.point_mul_batch(A["b"].copy(), A["qx"].copy(), A["qy"].copy(), curve=curve_id)
    sx, sy, e3, _ = hctx.point_add_batch(ax, ay, bx, by, curve=curve_id)
    # the three calls flag a neutral product (k P with k = 0 or P neutral) where a P + b Q goes on with the other term: their
    # codes are comparable where the operands are valid and the sum of two flagged products is the neutral element itself
    valid = (A["err"] == 0) | (A["err"] == 5)
    assert not ((e1 != 0) & (e1 != 5))[valid].any() and not ((e2 != 0) & (e2 != 5))[valid].any()
    for plan in L2.PLANS[curve_id]:
        rc, ox, oy, err = call(hctx, curve_id, plan, A, n)
        assert np.array_equal(ox[:n][valid], sx[valid]) and np.array_equal(oy[:n][valid], sy[valid]) and np.array_equal(err[:n][valid], e3[valid])
        bad = ~valid                                                  # an invalid operand: the code of the first bad one, P before Q
        first = np.where((e1[bad] == 3) | (e1[bad] == 4), e1[bad], e2[bad])   # (a 5 of the first product is no invalid operand)
        assert np.array_equal(err[:n][bad], first) and not ox[:n][bad].any() and not oy[:n][bad].any()


def test_refusals_and_the_in_place_forms(hctx):
    L, h = hctx._L, hctx._h
    A = L2.arrays(L2.batch(0, 65))
    n = 65
    bufs = {k: A[k].copy() for k in ("a", "b", "px", "py", "qx", "qy")}
    ox, oy, err = filled(n, 32), filled(n, 32), filled(n)

    def run(curve=0, plan=0, count=n, **swap):
        p = dict(bufs, outx=ox, outy=oy, err=err)
        p.update(swap)
        return L.p2e_point_lincomb2_batch(h, curve, C.c_uint(plan), _p(p["a"]), _p(p["b"]), _p(p["px"]), _p(p["py"]), _p(p["qx"]), _p(p["qy"]),
                                          _p(p["outx"]), _p(p["outy"]), size(count), _p(p["err"]))
    assert run(curve=1, plan=2) == -1 and "P2E_MUL_PLAN_GLV" in L.p2e_last_error().decode()
    assert run(plan=3) == -1 and run(curve=2) == -1
    assert run(count=0) == 0 and (ox == 0xAA).all()
    assert run(outx=bufs["b"]) == -1 and "overlap" in L.p2e_last_error().decode()
    assert run(outy=bufs["px"]) == -1 and "overlap" in L.p2e_last_error().decode()
    assert all((bufs[k] == A[k]).all() for k in bufs)
    for x, y in (("px", "py"), ("qx", "qy"), ("a", None)):
        bufs = {k: A[k].copy() for k in bufs}
        oy = filled(n, 32)
        rc = run(outx=bufs[x], outy=bufs[y] if y else oy)
        assert rc == np.count_nonzero(A["err"]) and np.array_equal(bufs[x], A["outx"]) and np.array_equal(bufs[y] if y else oy, A["outy"])
        assert np.array_equal(err, A["err"])


def test_device_pointers_and_the_python_method():
    n = 65
    ctx = p2e.Context(device=0)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    for curve_id in (0, 1):
        A = L2.arrays(L2.batch(curve_id, n))
        ox, oy, err, bad = ctx.point_lincomb2_batch(dev(A["a"]), dev(A["b"]), dev(A["px"]), dev(A["py"]), dev(A["qx"]), dev(A["qy"]), curve=curve_id)
        torch.cuda.synchronize()
        assert bad == np.count_nonzero(A["err"]) and np.array_equal(err.cpu().numpy(), A["err"])
        assert np.array_equal(ox.cpu().numpy(), A["outx"]) and np.array_equal(oy.cpu().numpy(), A["outy"])
    ctx.close()
