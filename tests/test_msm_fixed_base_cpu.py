"""The MSM and fixed-base curve programs on the CPU.

The first three tests check the test-side references themselves, not the library: the curve-generic restatement of
curve_msm_circuit (tests/msm_walk.py) and the oracle's Walker.fixed_base_curve_mul compute n p + m q and k base on both
curves, with the expected column, generator and aux counts, and raise where the reference panics.  The GPU tests
(test_gpu_msm_fixed_base.py) compare the library with these references.  The last test exercises the library's schedule
builder (compiled for the CPU in tests/emu): its sizes, its constants and the wiring of q."""
import numpy as np
import pytest

import msm_walk as W
import p2e_ref as R

CURVES = [R.SECP256K1, R.P256]


def _b32(v):
    return np.frombuffer(int(v).to_bytes(32, "little"), np.uint8).copy()


@pytest.fixture(scope="module")
def emu():
    from test_curve_programs import Emu
    return Emu()


@pytest.mark.parametrize("curve_id", [0, 1])
def test_msm_restatement_computes_n_p_plus_m_q(curve_id):
    cv = CURVES[curve_id]
    rng = R.SplitMix64(11 + curve_id)
    p, q = cv.mul(rng.below(cv.n), cv.g), cv.mul(rng.below(cv.n), cv.g)
    for n, m in ((rng.below(cv.n), rng.below(cv.n)), (1, cv.n - 1), ((1 << 255) + 7, 0), (5, 5)):
        cols, aux, ops, aux_ops, pt = W.msm_witness(cv, *p, *q, n, m)
        assert pt == cv.add(cv.mul(n, p), cv.mul(m, q))
        assert (len(cols), len(ops), len(aux)) == (W.MSM_COLS, W.MSM_GENS, W.MSM_AUX)
    assert sum(1 for o in aux_ops if o[0] == "index") == 131           # 9-limb scalars: 131 two-bit digits
    with pytest.raises(R.RefPanic):
        W.msm_witness(cv, *p, *q, 0, 0)                                  # the unblinding add meets its own negative
    with pytest.raises(R.RefPanic):
        W.msm_witness(cv, *p, *p, 3, 4)                                  # p = q: the table's p + q is a doubling


def test_msm_restatement_on_secp256k1_constants_match_the_oracle():
    """on secp256k1 the restatement's blinding point is the oracle's rando_point()"""
    assert R.SECP256K1.hash_point(32) == R.rando_point()


@pytest.mark.parametrize("curve_id", [0, 1])
def test_fixed_base_walk_computes_k_base(curve_id):
    cv = CURVES[curve_id]
    rng = R.SplitMix64(21 + curve_id)
    base = cv.mul(rng.below(cv.n), cv.g)
    for k in (rng.below(cv.n), 1, cv.n - 1, 0x1234):
        cols, aux, ops, _a, pt = W.fixed_base_witness(cv, base, k)
        assert pt == cv.mul(k, base)
        assert (len(cols), len(ops), len(aux)) == (W.FB_COLS, W.FB_GENS, W.FB_AUX)


@pytest.mark.parametrize("curve_id", [0, 1])
def test_builder_sizes_and_constants_of_the_two_programs(curve_id, emu):
    """the schedule builder's programs (through the CPU harness) have the restatement's sizes, the gadget's constants
    (rando, -rando, -2^262 rando) and the wiring of q through input slots 5 and 6"""
    import ctypes as C
    cv = CURVES[curve_id]
    base = cv.mul(0xC0FFEE, cv.g)
    blind = (_b32(base[0]), _b32(base[1]))
    assert emu.sizes(4, curve_id, blind) == (W.MSM_COLS, W.MSM_GENS, W.MSM_AUX)
    assert emu.sizes(5, curve_id, blind) == (W.FB_COLS, W.FB_GENS, W.FB_AUX)
    rando = cv.hash_point(32)
    spm = rando
    for _ in range(262):
        spm = cv.double(spm)

    def const(kind, cid):
        out = np.zeros(32, np.uint8)
        rc = emu.L.emu_curve_program_const(kind, curve_id, emu._p(blind[0]), emu._p(blind[1]), C.c_uint32(cid), emu._p(out))
        assert rc == 0
        return int.from_bytes(bytes(out), "little")

    assert (const(4, 0), const(4, 1)) == rando
    assert (const(4, 2), const(4, 3)) == cv.neg(rando)
    assert (const(4, 4), const(4, 5)) == cv.neg(spm)
    assert (const(5, 0), const(5, 1)) == rando
    _k, _f, first, ncols, src, nl = emu.gens(4, curve_id, blind)
    srcs = {int(s) for s in src.ravel()}
    assert 0x40000000 | 5 in srcs and 0x40000000 | 6 in srcs
