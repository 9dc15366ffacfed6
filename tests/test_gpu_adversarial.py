"""GPU (-m gpu): the adversarial batches of tests/adversarial_inputs.py on the HIP kernels, every element compared.

The verifier fills were compared with the oracle almost only on uniform u1 = msg / s, u2 = r / s and random public keys.
Here they get forced scalars (a zero window in every group, k1 = 0, k2 = 0, both GLV signs), structured public keys
(coordinates next to p, x + p), the blinding points and their relatives, raw ranges, and flagged rows in the first and last
lane, in lanes 63 / 64, in two adjacent lanes and in one whole aligned wave (an inversion sub-range of nothing but zeros).
Every launch plan a small batch can be forced into, both containers, the built-in-generator columns from both, err bytes
(exact), verdicts and the bad count; the comparison runs on the GPU against the uploaded oracle matrix.  A flagged row's
columns are not compared (the reference panics there); its err byte and zero verdict are, and its neighbours like any row.
test_adversarial_cpu.py holds the oracle itself to the expectations that come from the inputs alone."""
import numpy as np
import pytest

import adversarial_inputs as A
import oracle_c
import ux_oracle as UX
from test_adversarial_cpu import KIND, oracle

pytestmark = pytest.mark.gpu

BUILTIN_PLANS = {
    "default": {},
    "op_by_op": {"P2E_RUN_ITERS_SMALL": "0"},
    "lane_per_signature": {"P2E_QUAD_MAX_N": "0"},
    "lane_runs": {"P2E_QUAD_MAX_N": "0", "P2E_RUNS_MIN_N": "0"},
    "large_batch": {"P2E_QUAD_MAX_N": "0", "P2E_RUNS_MIN_N": "0", "P2E_BINV_ALT_MAX_N": "0"},
    "large_batch_fb_run": {"P2E_QUAD_MAX_N": "0", "P2E_RUNS_MIN_N": "0", "P2E_BINV_ALT_MAX_N": "0", "P2E_FB_RUN": "1"},
}
CURVE_PLANS = {"default": {}, "no_quad": {"P2E_CP_NO_QUAD": "1"}, "runs": {"P2E_CP_RUNS_MIN_N": "0"}}
_cache = {}


def reference(program, curve_id):
    """the lock-step oracle's matrices of one batch on the GPU (clean rows only), computed once per session"""
    import torch
    key = (program, curve_id)
    if key not in _cache:
        _cache.clear()                                       # one program's matrices at a time
        rows, marks = A.batch(program, curve_id)
        arrs = A.arrays(rows)
        cols, aux, err, verdict = oracle(program, curve_id, arrs, lockstep=True)
        want_flag, idx, want_verdict = A.expected(rows)
        assert np.array_equal(err != 0, want_flag) and np.array_equal(verdict[idx], want_verdict)
        clean = torch.from_numpy(np.nonzero(err == 0)[0]).cuda()
        to_dev = lambda m: torch.from_numpy(np.ascontiguousarray(m[:, err == 0]).view(np.int64)).cuda()
        _cache[key] = dict(rows=rows, marks=marks, arrs=arrs, dev=[torch.from_numpy(a).cuda() for a in arrs], cols=to_dev(cols),
                           aux=to_dev(aux), err=err, verifier=program == "verify", verdict=verdict, clean=clean, bad=int((err != 0).sum()))
    return _cache[key]


def pass_reference(program, curve_id):
    """the oracle's constraint-block and gate-internal matrices of one whole batch, uploaded (ux as int32: 1.2 GB for the
    built-in verifier), with the clean-row mask and the per-generator block list; one program's at a time"""
    import torch
    key = ("passes", program, curve_id)
    if key not in _cache:
        for k in [k for k in _cache if isinstance(k, tuple) and k[0] == "passes"]:
            del _cache[k]
        ref = reference(program, curve_id)
        if curve_id == 0 and program in ("verify", "glv_mul"):
            exp, lay = UX.builtin(0 if program == "verify" else 1, ref["arrs"]), UX.layout("builtin", 0 if program == "verify" else 1)
        else:
            exp = UX.curve_program(KIND[program], curve_id, A.blind(curve_id), ref["arrs"])
            lay = UX.layout("curve", KIND[program], curve_id)
        assert np.array_equal(exp["err"], ref["err"])
        del exp["cols"], exp["aux"]
        dexp = UX.to_device(torch, exp)
        dexp["blocks"] = lay["blocks"]
        _cache[key] = dexp
    return _cache[key]


def same_matrix(name, got, want, clean):
    import torch
    got = got.index_select(1, clean)
    if got.dtype == torch.int32:
        got = got.to(torch.int64) & 0xFFFFFFFF
    if not torch.equal(got, want):
        ne = (got != want).nonzero()
        c, i = int(ne[0, 0]), int(clean[ne[0, 1]])
        raise AssertionError(f"{name}: {ne.shape[0]} differing elements; first: column {c}, row {i}: got {int(got[c, ne[0, 1]])} "
                             f"want {int(want[c, ne[0, 1]])}")


def same_flags(name, ref, err, valid, bad):
    assert np.array_equal(err.cpu().numpy(), ref["err"]), name + ": err bytes"
    v, ok = valid.cpu().numpy(), ref["err"] == 0
    assert np.array_equal(v[ok], ref["verdict"][ok]), name + ": verdicts"
    assert not ref["verifier"] or not v[~ok].any(), name + ": a flagged signature must not verify"
    assert bad == ref["bad"], name + ": bad count"


@pytest.mark.parametrize("plan", list(BUILTIN_PLANS))
@pytest.mark.parametrize("program", ["verify", "glv_mul"])
def test_builtin_programs_on_adversarial_rows(program, plan, monkeypatch):
    import torch
    import plonky2_ecdsa_amd as p2e
    for k, v in BUILTIN_PLANS[plan].items():
        monkeypatch.setenv(k, v)
    ref = reference(program, 0)
    pid = p2e.PROGRAM_VERIFY if program == "verify" else 1
    ctx = p2e.Context(device=0)
    dev, clean, n = ref["dev"], ref["clean"], len(ref["rows"])
    fill, fill_compact = ((ctx.ecdsa_verify_witness_batch, ctx.ecdsa_verify_witness_compact_batch) if pid == 0 else
                          (ctx.glv_mul_witness_batch, ctx.glv_mul_witness_compact_batch))
    pky = dev[4] if pid == 0 else dev[1]
    cols, err, valid, bad = fill(*dev)
    aux, _aerr, _abad = ctx.aux_witness_batch(pid, pky, cols, n=n, ld=cols.stride(0))
    torch.cuda.synchronize()
    ph = ctx.last_phase_ms()
    assert ph["runs_launches"] > 0 or "P2E_RUNS_MIN_N" not in BUILTIN_PLANS[plan], "not the plan this case names"
    assert ph["fbrun_launches"] > 0 or not (plan == "large_batch_fb_run" and pid == 0)
    same_flags("u64 fill", ref, err, valid, bad)
    same_matrix("u64 matrix", cols, ref["cols"], clean)
    same_matrix("aux matrix", aux, ref["aux"], clean)
    del cols, aux
    nar, wid, cerr, cvalid, cbad = fill_compact(*dev)
    aux32, _e, _b = ctx.aux_witness_compact_batch(pid, pky, nar, n=n, ld_narrow=nar.stride(0))
    torch.cuda.synchronize()
    same_flags("compact fill", ref, cerr, cvalid, cbad)
    cmap, _nn, _nw = p2e.compact_layout(pid)
    is_wide = (cmap & p2e.COMPACT_WIDE) != 0
    same_matrix("compact container, narrow", nar, ref["cols"][torch.from_numpy(np.nonzero(~is_wide)[0]).cuda()], clean)
    same_matrix("compact container, wide", wid, ref["cols"][torch.from_numpy(np.nonzero(is_wide)[0]).cuda()], clean)
    same_matrix("aux matrix of the compact container", aux32, ref["aux"], clean)
    if pid == 0:
        verr, vvalid, vbad = ctx.ecdsa_verify_batch(*dev)
        torch.cuda.synchronize()
        same_flags("verdict-only call", ref, verr, vvalid, vbad)
    ctx.close()


CURVE_CASES = [(p, c, plan) for p, c in (("verify", 1), ("windowed", 0), ("windowed", 1), ("bitwise", 0), ("bitwise", 1))
               for plan in CURVE_PLANS if not (plan == "runs" and p == "bitwise")]      # (no window loop: one plan less)


@pytest.mark.parametrize("program,curve_id,plan", CURVE_CASES, ids=[f"{p}-{('secp256k1', 'p256')[c]}-{plan}" for p, c, plan in CURVE_CASES])
def test_curve_programs_on_adversarial_rows(program, curve_id, plan, monkeypatch):
    import torch
    import plonky2_ecdsa_amd as p2e
    for k, v in CURVE_PLANS[plan].items():
        monkeypatch.setenv(k, v)
    ref = reference(program, curve_id)
    ctx = p2e.Context(device=0)
    prog = p2e.CurveProgram(ctx, KIND[program], curve_id, A.blind(curve_id))
    dev, clean = ref["dev"], ref["clean"]
    fill, fill_compact = ((prog.verify_witness_batch, prog.verify_witness_compact_batch) if program == "verify" else
                          (prog.mul_witness_batch, prog.mul_witness_compact_batch))
    cols, err, valid, bad = fill(*dev)
    torch.cuda.synchronize()
    assert ctx.last_phase_ms()["runs_launches"] > 0 or plan != "runs", "not the plan this case names"
    same_flags("u64 fill", ref, err, valid, bad)
    same_matrix("u64 matrix", cols, ref["cols"], clean)
    aux, _aerr, _abad = prog.aux_witness_batch(dev, cols)
    torch.cuda.synchronize()
    same_matrix("aux matrix", aux, ref["aux"], clean)
    del cols, aux
    nar, wid, cerr, cvalid, cbad = fill_compact(*dev)
    torch.cuda.synchronize()
    same_flags("compact fill", ref, cerr, cvalid, cbad)
    cmap, _nn, _nw = prog.compact_layout()
    is_wide = (np.asarray(cmap) & p2e.COMPACT_WIDE) != 0
    same_matrix("compact container, narrow", nar, ref["cols"][torch.from_numpy(np.nonzero(~is_wide)[0]).cuda()], clean)
    same_matrix("compact container, wide", wid, ref["cols"][torch.from_numpy(np.nonzero(is_wide)[0]).cuda()], clean)
    if program == "verify":
        verr, vvalid, vbad = prog.verify_batch(*dev)
        torch.cuda.synchronize()
        same_flags("verdict-only call", ref, verr, vvalid, vbad)
    if plan == "default":
        # the constraint-block and gate-internal passes on the whole batch, both containers, against the oracle's walk
        n, ok = len(ref["rows"]), ref["err"] == 0
        dexp = pass_reference(program, curve_id)
        blocks = dexp["blocks"]
        assert [tuple(b) for b in prog.ux_describe()] == blocks
        aux32, _e, _b = prog.aux_witness_compact_batch(dev, nar, n=n)
        for u32 in (True, False):
            ux, uerr, _ub = prog.ux_witness_compact_batch(dev, nar, aux32, n=n, u32=u32)
            torch.cuda.synchronize()
            assert not uerr.cpu().numpy()[ok].any()
            UX.assert_same_device(torch, f"compact container, ux as {'u32' if u32 else 'u64'}", ux, dexp["ux32"], dexp, blocks)
            del ux
        if prog.num_gate_cols:
            UX.assert_same_device(torch, "u32 aux, gate", prog.gate_internal_compact_batch(aux32, n=n), dexp["gate"], dexp)
        del nar, wid
        cols, _e, _v, _b = fill(*dev)
        aux, _ae, _ab = prog.aux_witness_batch(dev, cols)
        for u32 in (True, False):
            ux, uerr, _ub = prog.ux_witness_batch(dev, cols, aux, n=n, ld=p2e._ld(cols), u32=u32)
            torch.cuda.synchronize()
            assert not uerr.cpu().numpy()[ok].any()
            UX.assert_same_device(torch, f"u64 matrices, ux as {'u32' if u32 else 'u64'}", ux, dexp["ux32"], dexp, blocks)
            del ux
        if prog.num_gate_cols:
            UX.assert_same_device(torch, "u64 aux, gate", prog.gate_internal_batch(aux, n=n), dexp["gate"], dexp)
    prog.close()
    ctx.close()


@pytest.mark.parametrize("program", ["verify", "glv_mul"])
def test_gate_internal_and_constraint_block_passes_on_named_rows(program):
    """the gate-internal and constraint-block passes on the GPU's own matrices of the adversarial batch: against the replay
    model on four named clean rows (k1 = 0, both GLV signs set, a u1 with a zero window in every group of sixteen or a sparse k
    for glv_mul, pk.x = p - small), and against the C oracle's walk on every column of every row the fill does not flag --
    u32 and u64 outputs, from the u64 matrices and from the compact container, padded strides with guard values"""
    import torch
    import check_circuit as CC
    import plonky2_ecdsa_amd as p2e
    ref = reference(program, 0)
    pid = 0 if program == "verify" else 1
    named = A.named_rows(program, 0)
    picks = [named["k1_zero"], named["both_signs"], named["zero_window_every_group" if pid == 0 else "sparse"], named["pk_x_near_p"]]
    ctx = p2e.Context(device=0)
    dev = ref["dev"]
    cols, _e, _v, _bad = (ctx.ecdsa_verify_witness_batch if pid == 0 else ctx.glv_mul_witness_batch)(*dev)
    aux, _ae, _ab = ctx.aux_witness_batch(pid, dev[4] if pid == 0 else dev[1], cols)
    ux, uerr, _ub = ctx.ux_witness_batch(pid, dev, cols, aux)
    gate = ctx.gate_internal_batch(pid, aux)
    torch.cuda.synchronize()
    assert not uerr.cpu().numpy()[ref["err"] == 0].any()          # (the pass range-checks; it does not repeat the fill's flags)
    for i in picks:
        ti = torch.tensor([i], device="cuda")
        col = lambda m, dt: m[:, ti].cpu().numpy().view(dt)[:, 0]
        check = CC.check_verify if pid == 0 else CC.check_glv_mul
        c = check(col(cols, np.uint64), *ref["rows"][i].args, aux=col(aux, np.uint64), ux=col(ux, np.uint32))
        assert np.array_equal(col(gate, np.uint64), np.array(c.gate, dtype=np.uint64)), ref["rows"][i].kind
    # every element and column against the oracle
    n, ok = len(ref["rows"]), ref["err"] == 0
    dexp = pass_reference(program, 0)
    blocks = dexp["blocks"]
    UX.assert_same_device(torch, "u64 matrices, ux as u32", ux, dexp["ux32"], dexp, blocks)
    UX.assert_same_device(torch, "u64 aux, gate", gate, dexp["gate"], dexp)
    del ux, gate
    k, kg = p2e.ux_num_cols(pid), dexp["gate"].shape[0]
    big64 = torch.full((k, n + 5), -1, dtype=torch.int64, device="cuda")          # odd stride: one element per store
    ux64, e64, _b = ctx.ux_witness_batch(pid, dev, cols, aux, ux=big64[:, :n])
    torch.cuda.synchronize()
    assert not e64.cpu().numpy()[ok].any() and bool((big64[:, n:] == -1).all())
    UX.assert_same_device(torch, "u64 matrices, ux as u64", ux64, dexp["ux32"], dexp, blocks)
    del ux64, big64, cols, aux
    nar, _wid, _e, _v, _b = (ctx.ecdsa_verify_witness_compact_batch if pid == 0 else ctx.glv_mul_witness_compact_batch)(*dev)
    aux32, _e, _b = ctx.aux_witness_compact_batch(pid, dev[4] if pid == 0 else dev[1], nar, n=n, ld_narrow=nar.stride(0))
    bigg = torch.full((kg, n + 10), -1, dtype=torch.int64, device="cuda")
    cgate = ctx.gate_internal_compact_batch(pid, aux32, gate=bigg[:, :n])
    torch.cuda.synchronize()
    assert bool((bigg[:, n:] == -1).all())
    UX.assert_same_device(torch, "u32 aux, gate", cgate, dexp["gate"], dexp)
    big32 = torch.full((k, n + 6), -1, dtype=torch.int32, device="cuda")           # even stride: paired stores + tail
    c32, ce32, _b = ctx.ux_witness_compact_batch(pid, dev, nar, aux32, ux=big32[:, :n])
    torch.cuda.synchronize()
    assert not ce32.cpu().numpy()[ok].any() and bool((big32[:, n:] == -1).all())
    UX.assert_same_device(torch, "compact container, ux as u32", c32, dexp["ux32"], dexp, blocks)
    del c32, big32
    c64, ce64, _b = ctx.ux_witness_compact_batch(pid, dev, nar, aux32, u32=False)
    torch.cuda.synchronize()
    assert not ce64.cpu().numpy()[ok].any()
    UX.assert_same_device(torch, "compact container, ux as u64", c64, dexp["ux32"], dexp, blocks)
    ctx.close()
