"""The MSM and fixed-base curve programs on the CPU: their witnesses computed three ways that must agree on every column.

1. the Python walk (tests/msm_walk.py, a curve-generic restatement of curve_msm_circuit over oracle/p2e_ref.py's Walker, and
   Walker.fixed_base_curve_mul), checked here to compute n p + m q and k base with the expected column, generator and aux
   counts and to raise where the reference panics;
2. the C oracle's kinds 4 and 5 (oracle/p2e_oracle.c p2e_oracle_curve_msm / p2e_oracle_curve_fixed_base), the fast
   restatement the GPU tests compare every element with (test_gpu_msm_fixed_base_exhaustive.py): equal to the Python walk
   on columns and aux, lock-step walk == faithful walk bit for bit, final point == host big integers on 512 elements;
3. the kernel bodies the GPU runs, compiled for the CPU (tests/emu, built with -DP2E_F29_BOUNDS: every limb bound of the
   lazy 29-bit arithmetic is asserted along the 262-doubling MSM chain and the 66 fixed-base windows), in the op-by-op and
   the run launch plans: every column, the aux and the gate-internal matrices against the oracle and the constraint
   replay's model, with the edge rows and the points that meet the blinding point in the batch.

The schedule builder's sizes, constants and the wiring of q are checked by the builder test."""
import ctypes as C
import multiprocessing as mp

import numpy as np
import pytest

import check_circuit as K
import msm_inputs as I
import msm_walk as W
import oracle_c
import p2e_ref as R

CURVES = [R.SECP256K1, R.P256]
NPROC = 16


def _b32(v):
    return np.frombuffer(int(v).to_bytes(32, "little"), np.uint8).copy()


@pytest.fixture(scope="module")
def emu():
    from test_curve_programs import Emu

    class MsmEmu(Emu):
        def run_msm(self, curve, ins, piece=32):
            """the MSM program through the kernel bodies: ins = (px, py, qx, qy, n, m) as (count, 32) bytes"""
            self.L.emu_curve_msm.restype = C.c_long
            ins = [np.ascontiguousarray(a) for a in ins]
            n = ins[0].shape[0]
            cols, err, valid = np.zeros((W.MSM_COLS, n), np.uint64), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
            bad = self.L.emu_curve_msm(curve, *[self._p(a) for a in ins], self._p(cols), C.c_size_t(n), C.c_size_t(n), self._p(err),
                                       self._p(valid), piece)
            return cols, err, valid, bad

    return MsmEmu()


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


# ---- the C oracle's kinds 4 and 5 ----------------------------------------------------------------------------------------
def _flagged_rows(ref):
    return [i for i, r in enumerate(ref) if r is None]


def _fb_job(args):
    try:
        return W.fixed_base_job(args)
    except R.RefPanic:
        return None


@pytest.fixture(scope="module")
def pool():
    with mp.get_context("spawn").Pool(NPROC) as p:
        yield p


@pytest.mark.parametrize("curve_id", [0, 1])
def test_c_oracle_msm_equals_the_python_walk(curve_id, pool):
    """columns AND aux of the twelve edge rows of msm_inputs and of 24 more elements (uniform, structured and sparse
    scalars), rows with p or q = +-rando / 2 rando among them; the oracle flags exactly the rows where the walk raises"""
    cv = CURVES[curve_id]
    assert oracle_c.curve_program_num_cols(oracle_c.CP_MSM, curve_id) == (W.MSM_COLS, W.MSM_AUX)
    ins, flagged = I.blinding_msm_inputs(curve_id, 48, 61 + curve_id)
    rows = list(range(36)) + list(range(48 - I.EDGE_ROWS, 48))
    vals = [I.ints(a) for a in ins]
    ref = pool.map(W.msm_job, [(cv.name, *[v[i] for v in vals]) for i in rows])
    cols, aux, err, flags = oracle_c.curve_msm(curve_id, *ins)
    assert [rows[j] for j in _flagged_rows(ref)] == flagged == np.nonzero(err)[0].tolist()
    assert all(err[i] == R.ERR_INVERSE_OF_ZERO for i in flagged) and np.array_equal(flags, (err == 0).astype(np.uint8))
    for j, i in enumerate(rows):
        if ref[j] is not None:
            assert np.array_equal(cols[:, i], np.asarray(ref[j][0], np.uint64)), (curve_id, i)
            assert np.array_equal(aux[:, i], np.asarray(ref[j][1], np.uint64)), (curve_id, i)


@pytest.mark.parametrize("curve_id", [0, 1])
def test_c_oracle_fixed_base_equals_the_python_walk(curve_id, pool):
    """a random base (32 elements with the edge rows at both ends, k = 0 flagged) and the bases rando, -rando, 2 rando (the
    edge rows and the rows whose first window meets the blinding point)"""
    cv = CURVES[curve_id]
    assert oracle_c.curve_program_num_cols(oracle_c.CP_FIXED_BASE_MUL, curve_id) == (W.FB_COLS, W.FB_AUX)
    cases = [(cv.mul(R.SplitMix64(71 + curve_id).below(cv.n), cv.g), *I.exhaustive_fb_inputs(curve_id, 32, 73 + curve_id))]
    for name, b in I.blinding_bases(cv).items():
        ks, fl = I.blinding_fb_inputs(curve_id, name, 40, 75 + curve_id)
        cases.append((b, ks[:20], [i for i in fl if i < 20]))
    for base, ks, flagged in cases:
        ref = pool.map(_fb_job, [(cv.name, base, k) for k in I.ints(ks)])
        cols, aux, err, flags = oracle_c.curve_fixed_base(curve_id, base, ks)
        assert _flagged_rows(ref) == flagged == np.nonzero(err)[0].tolist() and len(flagged) > 0
        assert np.array_equal(flags, (err == 0).astype(np.uint8))
        for i, r in enumerate(ref):
            if r is not None:
                assert np.array_equal(cols[:, i], np.asarray(r[0], np.uint64)), (curve_id, i)
                assert np.array_equal(aux[:, i], np.asarray(r[1], np.uint64)), (curve_id, i)


def _final_point(cols, i):
    """(x3, y3) of the unblinding add = the last curve_add of either program: its x3 and y3 sub generators are the 7th and
    the 10th of its ten generators (sub, sub, inv, mul, mul, add, sub, sub, mul, sub: 10+10+18+51+51+10+10+10+51+10 columns)"""
    end = cols.shape[0]
    x3, y3 = end - 10 - 51 - 10 - 10, end - 10
    return R.value_of([int(v) for v in cols[x3:x3 + 9, i]]), R.value_of([int(v) for v in cols[y3:y3 + 9, i]])


@pytest.mark.parametrize("curve_id", [0, 1])
def test_c_oracle_lockstep_equals_faithful_and_the_final_point_is_n_p_plus_m_q(curve_id, pool):
    """512 + 37 elements (not a multiple of the lock-step group of 64): the lock-step walk == the faithful walk bit for bit
    on a ragged sub-batch, and on EVERY element the final point == n p + m q / k base from Curve.mul / add (independent of
    any walk)"""
    cv = CURVES[curve_id]
    n = 512 + 37
    ins, flagged = I.exhaustive_msm_inputs(curve_id, n, 81 + curve_id)
    cols, aux, err, flags = oracle_c.curve_msm(curve_id, *ins, nthreads=NPROC, lockstep=64)
    assert np.nonzero(err)[0].tolist() == flagged
    sub = [a[n - 101:] for a in ins]                                    # 101 elements: one full group and a ragged one
    fc, fa, fe, ff = oracle_c.curve_msm(curve_id, *sub, nthreads=NPROC, lockstep=0)
    assert np.array_equal(fc, cols[:, n - 101:]) and np.array_equal(fa, aux[:, n - 101:])
    assert np.array_equal(fe, err[n - 101:]) and np.array_equal(ff, flags[n - 101:])
    vals = [I.ints(a) for a in ins]
    want = pool.map(W.native_msm_job, [(cv.name, (vals[0][i], vals[1][i]), (vals[2][i], vals[3][i]), vals[4][i], vals[5][i])
                                       for i in range(n)], chunksize=16)
    for i in range(n):
        if i not in flagged:
            assert _final_point(cols, i) == want[i], (curve_id, i)
    base = cv.mul(R.SplitMix64(83 + curve_id).below(cv.n), cv.g)
    ks, flagged = I.exhaustive_fb_inputs(curve_id, n, 85 + curve_id)
    cols, aux, err, flags = oracle_c.curve_fixed_base(curve_id, base, ks, nthreads=NPROC, lockstep=64)
    fc, fa, fe, ff = oracle_c.curve_fixed_base(curve_id, base, ks[n - 101:], nthreads=NPROC, lockstep=0)
    assert np.nonzero(err)[0].tolist() == flagged
    assert np.array_equal(fc, cols[:, n - 101:]) and np.array_equal(fa, aux[:, n - 101:]) and np.array_equal(fe, err[n - 101:])
    for i, k in enumerate(I.ints(ks)):
        if i not in flagged:
            assert _final_point(cols, i) == cv.mul(k % cv.n, base), (curve_id, i)


# ---- the kernel bodies on the CPU (tests/emu) ----------------------------------------------------------------------------
EMU_N = 300
OP_BY_OP = (32, 45)         # piece lengths of the op-by-op plan (the library's CP_PIECE_OPS and CP_PIECE_OPS_QUAD)
RUNS = (-1, -10, -7)        # run lengths of the run plan: 1, the library's 10 digits per run, and 7 (131 = 18 x 7 + 5)
REPLAYED = (0, 63, 64, 255, 299)


@pytest.mark.parametrize("curve_id", [0, 1])
def test_kernel_bodies_msm_equal_the_c_oracle(curve_id, emu):
    """body_cscalar's MSM branch, the chains, the inversion batches, body_expand and body_expand_run<.., 2> compiled for the
    CPU with -DP2E_F29_BOUNDS (limb-bound assertions active), in the launch order of run_curve_program: every column of 300
    elements == the C oracle in every plan, the flags too; aux == the oracle's aux; gate-internal == the constraint replay's.
    The batch holds the edge rows at both ends and rows with p or q = +-rando (flagged) and 2 rando."""
    ins, flagged = I.blinding_msm_inputs(curve_id, EMU_N, 91 + curve_id)
    want, want_aux, werr, wflags = oracle_c.curve_msm(curve_id, *ins, nthreads=NPROC, lockstep=64)
    assert np.nonzero(werr)[0].tolist() == flagged
    ok = werr == 0
    for piece in OP_BY_OP + RUNS:
        cols, err, valid, bad = emu.run_msm(curve_id, ins, piece)
        assert bad == len(flagged) and np.array_equal(err, werr) and np.array_equal(valid, wflags), piece
        assert np.array_equal(cols[:, ok], want[:, ok]), piece
    blind = (_b32(0), _b32(0))
    aux, aerr = emu.aux(4, curve_id, blind, (ins[4], ins[5], ins[4], ins[0], ins[1]), cols)
    assert not aerr[ok].any() and np.array_equal(aux[:, ok], want_aux[:, ok])
    gate = emu.gate(4, curve_id, blind, aux)
    cv = CURVES[curve_id]
    for i in [i for i in REPLAYED if ok[i]]:          # (the flagged edge rows are not among them)
        c, _pt = K.check_msm(cv, cols[:, i], *[I.ints(a[i:i + 1])[0] for a in ins], aux=aux[:, i])
        assert np.array_equal(gate[:, i], np.asarray(c.gate, np.uint64)), i


@pytest.mark.parametrize("name", ["random", "rando", "-rando", "2rando"])
@pytest.mark.parametrize("curve_id", [0, 1])
def test_kernel_bodies_fixed_base_equal_the_c_oracle(curve_id, name, emu):
    """the same for the fixed-base program (body_expand_fb_run on a table built from the caller's base in the run plan): a
    random base, and the bases that meet the blinding point, whose flagged rows follow from the scalars"""
    cv = CURVES[curve_id]
    if name == "random":
        base = cv.mul(R.SplitMix64(95 + curve_id).below(cv.n), cv.g)
        ks, flagged = I.exhaustive_fb_inputs(curve_id, EMU_N, 97 + curve_id)
    else:
        base = I.blinding_bases(cv)[name]
        ks, flagged = I.blinding_fb_inputs(curve_id, name, EMU_N, 97 + curve_id)
    want, want_aux, werr, wflags = oracle_c.curve_fixed_base(curve_id, base, ks, nthreads=NPROC, lockstep=64)
    assert np.nonzero(werr)[0].tolist() == flagged and 0 < len(flagged) <= 32
    ok = werr == 0
    blind = (_b32(base[0]), _b32(base[1]))
    for piece in OP_BY_OP + RUNS[:2]:
        cols, err, valid, bad = emu.run(5, curve_id, blind, (ks, ks, ks), piece)
        assert bad == len(flagged) and np.array_equal(err, werr) and np.array_equal(valid, wflags), piece
        assert np.array_equal(cols[:, ok], want[:, ok]), piece
    aux, aerr = emu.aux(5, curve_id, blind, (ks, ks, ks), cols)
    assert not aerr[ok].any() and np.array_equal(aux[:, ok], want_aux[:, ok])
    gate = emu.gate(5, curve_id, blind, aux)
    ux, uerr = emu.ux(5, curve_id, blind, (ks, ks, ks), cols, aux)
    for i in [i for i in REPLAYED if ok[i]]:
        c, _pt = K.check_fixed_base(cv, cols[:, i], base, I.ints(ks[i:i + 1])[0], aux=aux[:, i])
        assert np.array_equal(gate[:, i], np.asarray(c.gate, np.uint64)), i
        assert uerr[i] == 0 and np.array_equal(ux[:, i], np.asarray(c.ux, np.uint64)), i
