"""GPU (-m gpu): EVERY element and EVERY column of the MSM and fixed-base curve programs against the C oracle.

P2E_CP_MSM (curve_msm_circuit(p, q, n, m), gadgets/curve_msm.rs:21-79, 112 309 columns) and P2E_CP_FIXED_BASE_MUL
(fixed_base_curve_mul_circuit(base, k), gadgets/curve_fixed_base.rs:18-66, 16 797 columns) on secp256k1 and P-256, at the
sizes a sharded 2^16 batch produces and with NO plan-forcing environment variable: 2^13 (four lanes per element), 17 409
(the first size past the four-lane plan, ragged against the 256-lane workgroup: one lane per element, op by op), 2^15 (the
same plan, alternating inversion batches), 49 153 (the first size of the run plan, ragged: the tail-lane forms of the
run kernels, which 2^16 -- a whole number of workgroups -- never launches) and 2^16 (run kernels: kc_expand_runs2 for the
MSM, kc_expand_fb_run on the caller's table for the fixed-base program).  Each case is filled once into the u64 matrix (default padded stride) and once
into the compact container, and both are compared with oracle/p2e_oracle.c's lock-step walk (kinds 4 and 5; bit-identical
to the faithful walk and to the Python walk: tests/test_msm_fixed_base_cpu.py) on all n x num_cols elements, in chunks
of 4 096 elements (112 309 columns x 4 096 x 8 B = 3.7 GB of oracle columns at a time); the comparison itself runs on the
device.  The built-in-generator (aux) matrix derived from the u64 matrix is compared the same way (the curve programs have
no aux pass over the compact container), err / valid with the oracle's flags.

Inputs (tests/msm_inputs.py): distinct points per element; scalars one third uniform, one third structured (runs of ones /
zeros / alternating words, not reduced), one third sparse (a handful of non-zero digits); the edge rows in the first rows
and once more, in reverse order, in the last rows of the batch (the last lanes of the tail workgroup; reversed so that the
very last lane is an element whose columns are compared).

Exclusions cannot hide a failure: the columns of a flagged element are not compared (the reference panics there, it has
no value), but the set of flagged elements must equal a list built from the inputs alone (n = m = 0, p = q, p = -q;
k = 0; a point that meets the blinding point), the oracle's flags must equal that list too, and the list holds at most
32 elements.

Everything is integer work: every comparison is bit-exact.  Nothing here reads the reference tree.

Wall time per case on one MI355X with 16 host threads for the oracle (measured, first run; the oracle's walk is nearly
all of it):
    program, curve            2^13    17 409   2^15     49 153   2^16
    MSM, secp256k1            3.6 s   6.3 s    10.6 s   16.7 s   22.8 s
    MSM, P-256                2.8 s   5.9 s    10.5 s   15.8 s   21.1 s
    fixed-base, secp256k1     0.7 s   1.3 s    2.4 s    3.6 s    4.8 s
    fixed-base, P-256         0.5 s   1.2 s    2.0 s    3.1 s    4.2 s
(about 2.9 k MSM and 14 k fixed-base elements per second through the lock-step oracle; the 20 cases together 2.7 minutes).
No case of the matrix is dropped."""
import time

import numpy as np
import pytest

import check_circuit as K
import msm_inputs as I
import oracle_c
import p2e_ref as R

pytestmark = pytest.mark.gpu

CHUNK = 4096
NTHREADS = 16
GROUP = 64
MAX_FLAGGED = 32
SIZES = [1 << 13, 17408 + 1, 1 << 15, 49152 + 1, 1 << 16]
RUNS_MIN_N = 49152          # cp_runs_min_n, the default boundary of the run plan (include/p2e.h P2E_CP_RUNS_MIN_N)


def _first_difference(got, want, elements):
    ne = (got != want).nonzero()
    c, i = int(ne[0, 0]), int(ne[0, 1])
    return (f"{ne.shape[0]} differing values; first: column {c}, element {int(elements[i])}: got {int(got[c, i])} "
            f"want {int(want[c, i])}")


def compare_every_element(oracle, n, matrices, aux_matrices, err, valid, flagged, chunk=CHUNK):
    """oracle(a, b) -> (cols, aux, err, flags) of elements [a, b) by the C oracle.  matrices / aux_matrices: lists of
    (name, get(a, b) -> int64 cuda tensor of the product's values of elements [a, b), rows) for the witness / the aux
    columns; rows = None, or the index tensor of the oracle's columns that the matrix's rows hold (compact container).
    Walks the whole batch; the columns of the elements in `flagged` are left out, every other element is compared in full.
    Returns (number of compared witness values, list of failure messages naming matrix, column and element)."""
    import torch
    assert len(flagged) <= MAX_FLAGGED and sorted(set(flagged)) == list(flagged)
    e, v = err.cpu().numpy(), valid.cpu().numpy()
    assert np.nonzero(e)[0].tolist() == list(flagged), "the library flags other elements than the inputs' known edge rows"
    assert all(e[i] & R.ERR_INVERSE_OF_ZERO for i in flagged) and not v[list(flagged)].any() and v[e == 0].all()
    checked, failures = 0, []
    for a in range(0, n, chunk):
        b = min(n, a + chunk)
        want, want_aux, werr, wflags = oracle(a, b)
        assert np.nonzero(werr)[0].tolist() == [i - a for i in flagged if a <= i < b], f"oracle flags differ in [{a}, {b})"
        assert np.array_equal(e[a:b], werr), f"err flags differ in [{a}, {b})"
        assert np.array_equal(v[a:b], wflags), f"valid flags differ in [{a}, {b})"
        keep = np.nonzero(werr == 0)[0]
        keep_t = torch.from_numpy(keep).cuda()
        for wanted, mats in ((want, matrices), (want_aux, aux_matrices)):
            want_t = torch.from_numpy(wanted.view(np.int64)).cuda()
            if len(keep) != b - a:
                want_t = want_t.index_select(1, keep_t)
            for name, get, rows in mats:
                got = get(a, b)
                if len(keep) != b - a:
                    got = got.index_select(1, keep_t)
                w = want_t if rows is None else want_t.index_select(0, rows)
                if not torch.equal(got, w):
                    failures.append(f"{name}: " + _first_difference(got, w, keep + a))
                del got, w
            del want_t
        checked += len(keep) * want.shape[0]
        del want, want_aux
    return checked, failures


def _dev(arrs):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]


def _compact_rows(prog):
    """the witness columns (index tensors) that the rows of the compact container's narrow and wide matrices hold: the
    layout is in registration order, so row k of the narrow matrix is the k-th narrow column"""
    import torch
    import plonky2_ecdsa_amd as p2e
    cmap, nn, nw = prog.compact_layout()
    is_wide = (cmap & p2e.COMPACT_WIDE) != 0
    assert np.array_equal(cmap[~is_wide], np.arange(nn)) and np.array_equal(cmap[is_wide] & 0x7FFFFFFF, np.arange(nw))
    return torch.from_numpy(np.nonzero(~is_wide)[0]).cuda(), torch.from_numpy(np.nonzero(is_wide)[0]).cuda()


def _fill_and_compare(prog, ctx, kind, fill, fill_compact, aux_inputs, oracle, n, flagged, want_runs):
    """one case: the u64 matrix, the compact container and the aux matrix of a batch against the oracle; returns the
    number of compared witness values and the plan the call took"""
    import torch
    cols, err, valid, bad = fill()
    torch.cuda.synchronize()
    ph = ctx.last_phase_ms()
    runs_key = "runs_launches" if kind == "msm" else "fbrun_launches"
    other_key = "fbrun_launches" if kind == "msm" else "runs_launches"
    plan = f"run kernels ({int(ph[runs_key])} launches)" if ph[runs_key] > 0 else f"no run kernels ({int(ph['expand_launches'])} expand launches)"
    assert (ph[runs_key] > 0) == want_runs and ph[other_key] == 0, (n, ph)
    assert bad == len(flagged)
    nar, wid, cerr, cvalid, cbad = fill_compact()
    torch.cuda.synchronize()
    assert (ctx.last_phase_ms()[runs_key] > 0) == want_runs
    assert cbad == bad and torch.equal(cerr, err) and torch.equal(cvalid, valid)
    narrow_cols, wide_cols = _compact_rows(prog)
    aux, aerr, abad = prog.aux_witness_batch(aux_inputs, cols, n=n, ld=cols.stride(0))
    torch.cuda.synchronize()
    assert int(aerr.cpu().numpy()[err.cpu().numpy() == 0].sum()) == 0
    matrices = [("u64 matrix", lambda a, b: cols[:, a:b], None),
                ("compact container, narrow rows", lambda a, b: nar[:, a:b].to(torch.int64) & 0xFFFFFFFF, narrow_cols),
                ("compact container, wide rows", lambda a, b: wid[:, a:b], wide_cols)]
    checked, failures = compare_every_element(oracle, n, matrices, [("aux matrix", lambda a, b: aux[:, a:b], None)], err, valid,
                                              flagged)
    assert not failures, "\n".join(failures[:8])
    assert checked == (n - len(flagged)) * prog.num_cols
    del cols, nar, wid, aux, matrices
    torch.cuda.empty_cache()
    return checked, plan


def _msm_case(ctx, curve_id, n, ins, flagged, want_runs):
    import plonky2_ecdsa_amd as p2e
    prog = p2e.CurveProgram(ctx, p2e.CP_MSM, curve_id)
    assert (prog.num_cols, prog.num_aux_cols) == oracle_c.curve_program_num_cols(oracle_c.CP_MSM, curve_id)
    dev = _dev(ins)

    def oracle(a, b):
        return oracle_c.curve_msm(curve_id, *[x[a:b] for x in ins], nthreads=NTHREADS, lockstep=GROUP)

    out = _fill_and_compare(prog, ctx, "msm", lambda: prog.msm_witness_batch(*dev), lambda: prog.msm_witness_compact_batch(*dev),
                            tuple(dev), oracle, n, flagged, want_runs)
    prog.close()
    return out


def _fb_case(ctx, curve_id, base, n, ks, flagged, want_runs):
    import plonky2_ecdsa_amd as p2e
    prog = p2e.CurveProgram(ctx, p2e.CP_FIXED_BASE_MUL, curve_id, base=base)
    assert (prog.num_cols, prog.num_aux_cols) == oracle_c.curve_program_num_cols(oracle_c.CP_FIXED_BASE_MUL, curve_id)
    (k_dev,) = _dev([ks])

    def oracle(a, b):
        return oracle_c.curve_fixed_base(curve_id, base, ks[a:b], nthreads=NTHREADS, lockstep=GROUP)

    out = _fill_and_compare(prog, ctx, "fixed_base", lambda: prog.mul_witness_batch(None, None, k_dev),
                            lambda: prog.mul_witness_compact_batch(None, None, k_dev), (None, None, k_dev), oracle, n, flagged,
                            want_runs)
    prog.close()
    return out


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", ["msm", "fixed_base"])
@pytest.mark.parametrize("curve_id", [0, 1])
def test_every_element_and_column_of_the_default_plans(curve_id, kind, n, monkeypatch):
    import plonky2_ecdsa_amd as p2e
    for var in ("P2E_QUAD_MAX_N", "P2E_CP_RUNS_MIN_N", "P2E_CP_NO_RUNS", "P2E_BINV_ALT_MAX_N"):
        monkeypatch.delenv(var, raising=False)                    # the default plan of every size
    ctx = p2e.Context(device=0)
    t0 = time.time()
    if kind == "msm":
        ins, flagged = I.exhaustive_msm_inputs(curve_id, n, 1201 + curve_id)
        checked, plan = _msm_case(ctx, curve_id, n, ins, flagged, n >= RUNS_MIN_N)
    else:
        cv = I.CURVES[curve_id]
        base = cv.mul(R.SplitMix64(1301 + curve_id).below(cv.n), cv.g)
        ks, flagged = I.exhaustive_fb_inputs(curve_id, n, 1401 + curve_id)
        checked, plan = _fb_case(ctx, curve_id, base, n, ks, flagged, n >= RUNS_MIN_N)
    print(f"\n{kind} {I.CURVES[curve_id].name} n={n}: {checked} values compared ({n - len(flagged)} elements x all columns, "
          f"{len(flagged)} flagged), plan: {plan}, {time.time() - t0:.1f} s")


@pytest.mark.parametrize("plan", ["four_lanes", "op_by_op", "runs"])
@pytest.mark.parametrize("curve_id", [0, 1])
def test_msm_points_that_meet_the_blinding_point(curve_id, plan, monkeypatch):
    """p or q in {rando, -rando, 2 rando} (rando = KeccakHash::<32>(F::ZERO) * G of the curve): the table's first addition
    is a doubling or lands on infinity for +-rando, where the reference panics (inverse of zero).  The library flags exactly
    those elements (ERR_INVERSE_OF_ZERO, valid = 0) and every column of every other element is exact."""
    import plonky2_ecdsa_amd as p2e
    if plan == "op_by_op":
        monkeypatch.setenv("P2E_QUAD_MAX_N", "0")
    elif plan == "runs":
        monkeypatch.setenv("P2E_CP_RUNS_MIN_N", "1")
    n = 300
    ins, flagged = I.blinding_msm_inputs(curve_id, n, 1501 + curve_id)
    assert len(flagged) <= MAX_FLAGGED
    _msm_case(p2e.Context(device=0), curve_id, n, ins, flagged, plan == "runs")


@pytest.mark.parametrize("plan", ["four_lanes", "op_by_op", "runs"])
@pytest.mark.parametrize("name", ["rando", "-rando", "2rando"])
@pytest.mark.parametrize("curve_id", [0, 1])
def test_fixed_base_on_a_base_that_meets_the_blinding_point(curve_id, name, plan, monkeypatch):
    """the base is caller data: with base = +-rando the very first window addition (rando + t base) is a doubling or lands
    on infinity for the digits 0 and 1, with base = 2 rando the scalar (n - 1) / 2 ends on infinity.  The flagged rows
    follow from the scalars alone (msm_inputs.fb_flagged_on_a_rando_multiple)."""
    import plonky2_ecdsa_amd as p2e
    if plan == "op_by_op":
        monkeypatch.setenv("P2E_QUAD_MAX_N", "0")
    elif plan == "runs":
        monkeypatch.setenv("P2E_CP_RUNS_MIN_N", "1")
    n = 300
    ks, flagged = I.blinding_fb_inputs(curve_id, name, n, 1601 + curve_id)
    assert 0 < len(flagged) <= MAX_FLAGGED
    base = I.blinding_bases(I.CURVES[curve_id])[name]
    _fb_case(p2e.Context(device=0), curve_id, base, n, ks, flagged, plan == "runs")


REPLAYED = (0, 63, 64, 255, 299)


def _flip(vec, col, bit=0):
    out = list(vec)
    out[col] ^= 1 << bit
    return out


@pytest.mark.parametrize("curve_id", [0, 1])
def test_msm_gpu_output_passes_the_constraint_replay(curve_id):
    """five elements of a 300-element GPU batch through the reference's own equations (oracle/check_circuit.py check_msm)
    with the GPU's aux attached; the GPU's gate-internal matrix equals the replay's; a GPU column with one bit flipped is
    rejected"""
    import torch
    import plonky2_ecdsa_amd as p2e
    cv = I.CURVES[curve_id]
    n = 300
    ins, flagged = I.exhaustive_msm_inputs(curve_id, n, 1701 + curve_id)
    for k in flagged:                                    # clean rows only: row 0 and row 299 are replayed
        ins[4][k], ins[5][k] = I.b32(3 + k), I.b32(5 + k)
        ins[0][k], ins[1][k] = ins[0][k - 5 if k > 20 else k + 20], ins[1][k - 5 if k > 20 else k + 20]
    ctx = p2e.Context(device=0)
    prog = p2e.CurveProgram(ctx, p2e.CP_MSM, curve_id)
    dev = _dev(ins)
    cols, err, valid, bad = prog.msm_witness_batch(*dev)
    aux, aerr, abad = prog.aux_witness_batch(tuple(dev), cols, n=n, ld=p2e._ld(cols))
    gate = prog.gate_internal_batch(aux, n=n)
    torch.cuda.synchronize()
    assert bad == 0 and abad == 0
    cols, aux, gate = (t.cpu().numpy().view(np.uint64) for t in (cols, aux, gate))
    for i in REPLAYED:
        v = [I.ints(a[i:i + 1])[0] for a in ins]
        col_i = [int(x) for x in cols[:, i]]
        c, pt = K.check_msm(cv, col_i, *v, aux=[int(x) for x in aux[:, i]])
        assert pt == cv.add(cv.mul(v[4], (v[0], v[1])), cv.mul(v[5], (v[2], v[3])))
        assert np.array_equal(gate[:, i], np.asarray(c.gate, np.uint64)), (curve_id, i)
    with pytest.raises(K.ConstraintViolation):
        K.check_msm(cv, _flip(col_i, prog.num_cols // 2, 3), *v)
    with pytest.raises(K.ConstraintViolation):
        K.check_msm(cv, col_i, *v, aux=_flip([int(x) for x in aux[:, i]], prog.num_aux_cols - 40))
    prog.close()


@pytest.mark.parametrize("curve_id", [0, 1])
def test_fixed_base_gpu_output_passes_the_constraint_replay(curve_id):
    """the same for the fixed-base program on a RANDOM base (check_fixed_base), and the GPU's constraint-block (ux) matrix
    equals the replay's, value for value"""
    import torch
    import plonky2_ecdsa_amd as p2e
    cv = I.CURVES[curve_id]
    n = 300
    base = cv.mul(R.SplitMix64(1801 + curve_id).below(cv.n), cv.g)
    ks, flagged = I.exhaustive_fb_inputs(curve_id, n, 1901 + curve_id)
    for k in flagged:
        ks[k] = I.b32(77 + k)
    ctx = p2e.Context(device=0)
    prog = p2e.CurveProgram(ctx, p2e.CP_FIXED_BASE_MUL, curve_id, base=base)
    (k_dev,) = _dev([ks])
    cols, err, valid, bad = prog.mul_witness_batch(None, None, k_dev)
    aux, aerr, abad = prog.aux_witness_batch((None, None, k_dev), cols, n=n, ld=p2e._ld(cols))
    gate = prog.gate_internal_batch(aux, n=n)
    ux, uerr, ubad = prog.ux_witness_batch((None, None, k_dev), cols, aux, n=n, ld=p2e._ld(cols), u32=False)
    torch.cuda.synchronize()
    assert (bad, abad, ubad) == (0, 0, 0)
    cols, aux, gate, ux = (t.cpu().numpy().view(np.uint64) for t in (cols, aux, gate, ux))
    for i in REPLAYED:
        k = I.ints(ks[i:i + 1])[0]
        col_i = [int(x) for x in cols[:, i]]
        c, pt = K.check_fixed_base(cv, col_i, base, k, aux=[int(x) for x in aux[:, i]])
        assert pt == cv.mul(k, base)
        assert np.array_equal(gate[:, i], np.asarray(c.gate, np.uint64)), (curve_id, i)
        assert np.array_equal(ux[:, i], np.asarray(c.ux, np.uint64)), (curve_id, i)
    with pytest.raises(K.ConstraintViolation):
        K.check_fixed_base(cv, _flip(col_i, prog.num_cols // 2, 3), base, k)
    prog.close()


def test_the_chunked_comparison_reports_a_single_flipped_bit():
    """the comparison can fail: one bit flipped in a copy of a GPU matrix (last column, last unflagged element of a 2^13
    batch) is reported as exactly that (column, element)"""
    import torch
    import plonky2_ecdsa_amd as p2e
    curve_id, n = 0, 1 << 13
    cv = I.CURVES[curve_id]
    base = cv.mul(0xF11B, cv.g)
    ks, flagged = I.exhaustive_fb_inputs(curve_id, n, 2001)
    ctx = p2e.Context(device=0)
    prog = p2e.CurveProgram(ctx, p2e.CP_FIXED_BASE_MUL, curve_id, base=base)
    (k_dev,) = _dev([ks])
    cols, err, valid, bad = prog.mul_witness_batch(None, None, k_dev)
    aux, _aerr, _abad = prog.aux_witness_batch((None, None, k_dev), cols, n=n, ld=cols.stride(0))
    torch.cuda.synchronize()
    broken = cols.clone()
    col, elem = prog.num_cols - 1, n - 1
    assert elem not in flagged
    broken[col, elem] ^= 1 << 17

    def oracle(a, b):
        return oracle_c.curve_fixed_base(curve_id, base, ks[a:b], nthreads=NTHREADS, lockstep=GROUP)

    checked, failures = compare_every_element(oracle, n, [("good", lambda a, b: cols[:, a:b], None), ("broken", lambda a, b: broken[:, a:b], None)],
                                              [("aux", lambda a, b: aux[:, a:b], None)], err, valid, flagged)
    assert checked == (n - len(flagged)) * prog.num_cols
    assert len(failures) == 1 and failures[0].startswith(f"broken: 1 differing values; first: column {col}, element {elem}:"), failures
    prog.close()
