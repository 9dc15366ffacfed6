"""CPU: the adversarial rows of tests/adversarial_inputs.py (forced u1 / u2, structured public keys, relatives of the
blinding points, raw ranges, flagged lanes at the workgroup edges and a whole flagged wave) through the faithful C oracle,
its lock-step variant and the kernel bodies compiled for the CPU (tests/emu), with the expected flags and verdicts taken
from the inputs alone.  test_gpu_adversarial.py runs the same batches on the HIP kernels."""
import ctypes as C

import numpy as np
import pytest

import adversarial_inputs as A
import check_circuit as CC
import oracle_c
import p2e_ref as R

PROGRAMS = [("verify", 0), ("glv_mul", 0), ("verify", 1), ("windowed", 0), ("windowed", 1), ("bitwise", 0), ("bitwise", 1)]
IDS = [f"{p}-{('secp256k1', 'p256')[c]}" for p, c in PROGRAMS]
KIND = {"windowed": oracle_c.CP_WINDOWED_MUL, "bitwise": oracle_c.CP_SCALAR_MUL, "verify": oracle_c.CP_VERIFY}


def oracle(program, curve_id, arrs, lockstep=False):
    """(cols, aux, err, verdicts) of the C oracle; glv_mul has the faithful walk only"""
    if program == "verify" and curve_id == 0:
        return (oracle_c.verify_witness_aux_lockstep if lockstep else oracle_c.verify_witness_aux)(*arrs)
    if program == "glv_mul":
        return oracle_c.glv_mul_witness_aux(*arrs)
    return oracle_c.curve_program(KIND[program], curve_id, A.blind(curve_id), arrs, lockstep=64 if lockstep else 0)


@pytest.fixture(scope="module")
def emu():
    from backends import EmuBackend
    return EmuBackend()


@pytest.fixture(scope="module")
def cemu():
    from test_curve_programs import Emu
    return Emu()


def test_builder_multiplication_is_the_reference_curves():
    rng = R.SplitMix64(1)
    for cv in A.CURVES:
        for k in (1, 2, cv.n - 1, rng.below(cv.n), rng.below(cv.n)):
            assert A.mul(cv, k, cv.g) == cv.mul(k, cv.g)
        assert A.mul(cv, cv.n, cv.g) is None and cv.on_curve(A.blind(A.CURVES.index(cv)))


def test_input_sets_cover_what_they_claim():
    # built-in verifier: the forced u2 reach every GLV case and every MSM table index
    rows = [c for c in A.classes("verify", 0) if c.u2 and not c.flagged and c.valid == 1]
    signs, idx, zero1, zero2 = set(), set(), 0, 0
    for c in rows:
        k1, k2, n1, n2 = R.glv_decompose(c.u2)
        signs.add((n1, n2))
        zero1 += k1 == 0
        zero2 += k2 == 0
        top = (max(k1.bit_length(), k2.bit_length()) + 1) // 2          # digits below the highest non-zero one only:
        idx |= {4 * ((k2 >> (2 * d)) & 3) + ((k1 >> (2 * d)) & 3) for d in range(top)}    # index 0 = an interior empty digit
    grid = [R.glv_decompose(c.u2)[:2] for c in rows if c.kind == "glv_grid"]
    # the grid's own lowest digits: k1 in {0, 1, 5, 2^126 | 1} ends in 0 or 1, k2 in {0, 1, 7, 2^125 | 3} in 0, 1 or 3
    assert {4 * (k2 & 3) + (k1 & 3) for k1, k2 in grid} == {1, 4, 5, 12, 13}
    assert signs == {(0, 0), (0, 1), (1, 0), (1, 1)} and zero1 and zero2 and idx == set(range(16))
    ks = [c.args[2] % R.N for c in A.classes("glv_mul", 0) if not c.flagged]
    dec = [R.glv_decompose(k) for k in ks]
    assert {(d[2], d[3]) for d in dec} == {(0, 0), (0, 1), (1, 0), (1, 1)} and any(d[0] == 0 for d in dec) and any(d[1] == 0 for d in dec)
    # fixed-base walk: a zero window in every group of sixteen, single windows at both ends
    u1 = [c.u1 for c in A.classes("verify", 0) if c.kind == "u1_one_window"]
    assert {v.bit_length() for v in u1} >= {1, 4, 253, 256} and all(bin(v).count("1") in (1, 4) for v in u1)
    # P-256: every 4-bit digit in the top and in the bottom window of u2 / k
    for prog, vals in (("verify", [c.u2 for c in A.classes("verify", 1) if c.u2]), ("windowed", [c.args[2] for c in A.classes("windowed", 1)])):
        assert {v >> 252 for v in vals} == set(range(16)) and {v & 15 for v in vals} == set(range(16)), prog
    for prog, cid in PROGRAMS:
        cl = A.classes(prog, cid)
        kinds = {c.kind for c in cl}
        pk = (lambda c: c.args[3:5]) if prog == "verify" else (lambda c: c.args[0:2])
        cv = A.CURVES[cid]
        st = [pk(c) for c in cl if c.kind == "pk_structured"]
        assert len(st) >= 100 and {y & 1 for _x, y in st} == {0, 1} and all(cv.on_curve(q) for q in st)
        small = {pk(c)[0] for c in cl if c.kind in ("pk_small_x", "pk_x_near_p")}
        for x in list(range(1, 41)) + list(range(cv.p - 40, cv.p)):
            assert (A.lift(cv, x, 0) is not None) == (x in small)
        assert kinds >= {"pk_generator", "pk_blind", "pk_blind_relative", "pk_off_curve", "pk_all_ones", "pk_x_plus_p"}
        assert any(pk(c) == (0, 0) for c in cl)
        assert sum(c.kind.endswith("structured") and not c.kind.startswith("pk") for c in cl) >= 60
        assert sum(c.kind.endswith("sparse") for c in cl) >= 60
        if prog == "verify":
            assert kinds >= {"msg_plus_n", "r_plus_n", "s_plus_n", "s_zero", "u2_zero", "all_ones"}
            assert sum(c.kind == "synthetic" for c in cl) == 10
        rows, marks = A.batch(prog, cid)                       # (asserts the placement of the flagged lanes and the cap)
        assert len(rows) % 64 == 1 and marks["wave"] % 64 == 0
        assert (prog, cid) not in A.COUNTS or A.COUNTS[prog, cid] == (len(cl), len(rows), sum(c.flagged for c in rows))
    assert set(A.COUNTS) == set(PROGRAMS)


def test_lazy_limb_canonical_reduction_between_p_and_2_256(emu):
    """f29_canon (csrc/fe29.hpp: what every stored coordinate of the four-lane and lazy-limb chains goes through) on limb
    forms whose folded value lands in [p, 2^256): only its last conditional subtraction makes those canonical, and no
    signature row reaches it (a lazy product is p + small with probability 2^-224).  Forms: (1 + h) p + d for d = 0, 1,
    2^32 + 976 (= 2^256 - 1 - p) and values within 2^32 of p on either side, h = 0 .. 127 (the bits above 2^256 that limb 8
    may carry), split into 29-bit limbs and again with a borrow pushed into every limb (limbs up to 2^30, as sums of two
    tight values have); also p - 1, 2 p - 1, 0 and uniform limbs below 2^31.  Expected: the value mod p, Python integers."""
    import probe_inputs
    forms, want = probe_inputs.canon_forms()                   # (the builder is shared with the device probe's f29_canon ops)
    p = R.P
    arr = np.array(forms, np.uint32)
    out = np.zeros((len(forms), 32), np.uint8)
    emu.L.emu_f29_canon.restype = C.c_long
    assert emu.L.emu_f29_canon(arr.ctypes.data_as(C.c_void_p), C.c_size_t(len(forms)), out.ctypes.data_as(C.c_void_p)) == len(forms)
    got = oracle_c.unpack256(out)
    bad = [(i, forms[i]) for i in range(len(forms)) if got[i] != want[i]]
    assert not bad, (len(bad), bad[0])
    assert sum(p <= sum(x << (29 * k) for k, x in enumerate(l)) < 1 << 256 for l in forms) >= 100


@pytest.fixture(scope="module", params=PROGRAMS, ids=IDS)
def walked(request):
    """(program, curve, rows, arrays, and the faithful oracle's cols, aux, err, verdicts) of one batch.  A module-scoped
    parameter: every test of one program runs on one walk, and one matrix (0.8 GB for the verifier) is alive at a time"""
    program, curve_id = request.param
    rows, _marks = A.batch(program, curve_id)
    arrs = A.arrays(rows)
    return (program, curve_id, rows, arrs) + tuple(oracle(program, curve_id, arrs))


def test_expected_flags_and_verdicts(walked):
    """the set of flagged rows is EXACTLY the set the builder names from the inputs; the verdict is 1 on every clean row
    built as valid and 0 on off-curve / non-canonical rows"""
    program, curve_id, rows, arrs, _cols, _aux, err, verdict = walked
    want_flag, idx, want_verdict = A.expected(rows)
    got = err != 0
    assert np.array_equal(got, want_flag), [(i, rows[i].kind, int(err[i])) for i in np.nonzero(got != want_flag)[0][:10]]
    assert np.array_equal(err[got], np.full(int(got.sum()), R.ERR_INVERSE_OF_ZERO, np.uint8))
    bad = idx[verdict[idx] != want_verdict]
    assert len(bad) == 0, [(int(i), rows[i].kind, rows[i].valid) for i in bad[:10]]
    assert len(idx) > 0.85 * len(rows)
    assert program != "verify" or not verdict[got].any()       # a flagged signature never verifies


def test_oracles_and_kernel_bodies_agree_on_every_element(walked, emu, cemu):
    """faithful oracle == lock-step oracle == the kernel bodies (u64, compact and verdict-only forms; op-by-op expansion
    and run lengths 4, 9, 12 for each; the curve programs cut into pieces and walked as runs): err bytes and verdicts of every row,
    every column of every row the reference does not panic on"""
    import plonky2_ecdsa_amd as p2e
    program, curve_id, rows, arrs, cols, aux, err, verdict = walked
    clean = err == 0

    def same(name, gcols, gerr, gvalid):
        assert np.array_equal(gerr, err), name + ": err bytes"
        assert np.array_equal(gvalid[clean], verdict[clean]), name + ": verdicts"
        assert program != "verify" or not gvalid[~clean].any(), name + ": a flagged signature must not verify"
        if gcols is not None:
            ne = (gcols[:, clean] != cols[:, clean]).nonzero()
            assert len(ne[0]) == 0, f"{name}: first differing column {ne[0][0]}, row {np.nonzero(clean)[0][ne[1][0]]}"

    if program != "glv_mul":
        lcols, laux, lerr, lverdict = oracle(program, curve_id, arrs, lockstep=True)
        same("lock-step oracle", lcols, lerr, lverdict)
        assert np.array_equal(laux[:, clean], aux[:, clean])
        del lcols, laux
    if curve_id == 0 and program in ("verify", "glv_mul"):
        pid = 0 if program == "verify" else 1
        run = emu.verify if pid == 0 else emu.glv_mul
        _m, nn, nw = p2e.compact_layout(pid)
        for ri in (0, 4, 9, 12):
            gcols, gerr, gvalid = run(*arrs, run_iters=ri)
            same(f"kernel bodies, run length {ri}", gcols, gerr, gvalid)
            del gcols
        for ri in (0, 4, 9, 12):
            nar, wid, cerr, cvalid = emu.compact(pid, arrs, nn, nw, run_iters=ri)
            same(f"compact bodies, run length {ri}", p2e.compact_expand(pid, nar, wid), cerr, cvalid)
        if pid == 0:
            verr, vvalid = emu.verify_only(*arrs)
            same("verdict-only bodies", None, verr, vvalid)
        _c, gaux, gaerr = emu.aux(pid, arrs)
        assert np.array_equal(gaux[:, clean], aux[:, clean]) and not gaerr[clean].any()
    else:
        kind = KIND[program]
        b = A.arrays([A.Case("blind", A.blind(curve_id), False, None)])
        b = (b[0][0], b[1][0])
        for piece in (32, 7) + ((-6, -11) if kind != oracle_c.CP_SCALAR_MUL else ()):
            gcols, gerr, gvalid, bad = cemu.run(kind, curve_id, b, arrs, piece=piece)
            same(f"kernel bodies, piece {piece}", gcols, gerr, gvalid)
            assert bad == int((err != 0).sum())
        if kind == oracle_c.CP_VERIFY:
            cemu.L.emu_p256_verify_only.restype = C.c_long
            verr, vvalid = np.zeros(len(rows), np.uint8), np.zeros(len(rows), np.uint8)
            cemu.L.emu_p256_verify_only(cemu._p(b[0]), cemu._p(b[1]), *[cemu._p(a) for a in arrs], C.c_size_t(len(rows)), cemu._p(verr), cemu._p(vvalid))
            same("verdict-only bodies", None, verr, vvalid)


def _walker(program, curve_id, args):
    cv = A.CURVES[curve_id]
    if program == "verify":
        return R.verify_witness(*args)[0] if curve_id == 0 else R.verify_p256_witness(*args, A.blind(curve_id))[0]
    if program == "glv_mul":
        return R.glv_mul_witness(*args)[0]
    f = R.windowed_mul_witness if program == "windowed" else R.scalar_mul_witness
    return f(cv, *args, A.blind(curve_id))[0]


def test_python_walk_agrees_on_a_stride_sample(walked):
    """the big-int gadget walk against the C oracle's columns on about ten rows of each batch (a flagged row must raise)"""
    program, curve_id, rows, _arrs, cols, _aux, err, _verdict = walked
    for i in range(3, len(rows), len(rows) // 10):
        try:
            ref = _walker(program, curve_id, rows[i].args)
        except R.RefPanic:
            assert err[i] and rows[i].flagged
            continue
        assert err[i] == 0 and np.array_equal(cols[:, i], np.asarray(ref, np.uint64)), (i, rows[i].kind)


REPLAYED = ("k1_zero", "k2_zero", "both_signs", "n1_only", "n2_only", "one_window_u1", "zero_window_every_group", "u1_n_minus_1",
            "pk_x_near_p", "pk_x_plus_p", "msg_plus_n", "s_plus_n", "sparse", "structured", "pk_small_x", "u2_n_minus_1")


def test_named_rows_pass_the_constraint_replay(walked):
    """no oracle value decides: the columns of named clean valid rows (k1 = 0, k2 = 0, n1 alone, n2 alone, both GLV signs,
    a single non-zero window, a zero window in every group of the u1 walk, u1 = n - 1, pk.x next to p, pk.x + p, msg + n,
    s + n, a sparse scalar ...) go through the reference's constraint equations: the first twelve of REPLAYED a verifier
    or glv_mul has (a replay takes a second), the first four of the windowed and bit-wise programs"""
    program, curve_id, rows, _arrs, cols, aux, err, verdict = walked
    named = A.named_rows(program, curve_id)
    if program == "verify":
        assert set(named) >= {"one_window_u1", "zero_window_every_group", "u1_n_minus_1", "msg_plus_n", "s_plus_n"}
    if curve_id == 0 and program in ("verify", "glv_mul"):
        assert set(named) >= {"k1_zero", "k2_zero", "both_signs", "n1_only", "n2_only"}
    assert set(named) >= {"sparse", "structured", "pk_x_near_p", "pk_x_plus_p", "pk_small_x"}
    take = [k for k in REPLAYED if k in named][:12 if program in ("verify", "glv_mul") else 4]
    cv, g = A.CURVES[curve_id], A.blind(curve_id)
    for name in take:
        i = named[name]
        assert err[i] == 0 and verdict[i] == 1, name
        if program == "verify" and curve_id == 0:
            check = lambda: CC.check_verify(cols[:, i], *rows[i].args, aux=aux[:, i])
        elif program == "glv_mul":
            check = lambda: CC.check_glv_mul(cols[:, i], *rows[i].args, aux=aux[:, i])
        elif program == "verify":
            check = lambda: CC.check_verify_p256(cols[:, i], *rows[i].args, g, aux=aux[:, i])
        else:
            f = CC.check_windowed_mul if program == "windowed" else CC.check_scalar_mul
            check = lambda: f(cv, cols[:, i], *rows[i].args, g, aux=aux[:, i])
        if name in ("pk_x_plus_p", "s_plus_n"):
            # the generators run and the verdict is 1, but the circuit itself is not satisfiable: sub_nonnative connects
            # diff + b with the RAW a, and an early x - x' has the non-canonical pk.x on its left; the inverse generator
            # takes its quotient from the canonical s while the constraint multiplies the raw one
            with pytest.raises(CC.ConstraintViolation, match="sub_nonnative" if name == "pk_x_plus_p" else "inv_nonnative"):
                check()
        else:
            check()
