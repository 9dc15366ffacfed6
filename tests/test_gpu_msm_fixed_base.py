"""The MSM and fixed-base curve programs on the GPU (P2E_CP_MSM: curve_msm_circuit(p, q, n, m) gadgets/curve_msm.rs:21-79,
P2E_CP_FIXED_BASE_MUL: fixed_base_curve_mul_circuit(base, n) gadgets/curve_fixed_base.rs:18-66), on secp256k1 and P-256.

Every column against tests/msm_walk.py (a curve-generic restatement of the gadget over the oracle's Walker), in the three
launch plans (four lanes per element, one lane op by op, runs), the u64 matrix and the compact container; the MSM at full
size against its own op-by-op plan and the final point against host big integers; the fixed-base program with the
curve's generator against the P-256 verifier's fixed-base scope; the aux, gate-internal and segment passes; misuse."""
import multiprocessing as mp
import os

import numpy as np
import pytest

import msm_walk as W
import p2e_ref as R
from msm_inputs import FLAGGED, fb_inputs as _fb_inputs, msm_inputs as _msm_inputs   # (shared with the CPU tests)

CURVES = [R.SECP256K1, R.P256]
P_GL = 0xFFFFFFFF00000001
NPROC = 16


def _pool():
    return mp.get_context("spawn").Pool(NPROC)


def _b32(v):
    return np.frombuffer(int(v).to_bytes(32, "little"), np.uint8).copy()


def _ints(a):
    return [int.from_bytes(bytes(bytearray(r)), "little") for r in np.asarray(a)]


def _arr(vals):
    return np.stack([_b32(v) for v in vals])


def _ctx(monkeypatch, plan):
    import plonky2_ecdsa_amd as p2e
    if plan == "op_by_op":
        monkeypatch.setenv("P2E_QUAD_MAX_N", "0")
    elif plan == "runs":
        monkeypatch.setenv("P2E_CP_RUNS_MIN_N", "1")
    return p2e.Context(device=0)


SAMPLE = list(range(40)) + [100, 233, 255, 256, 257, 511, 600, 699]


@pytest.fixture(scope="module")
def msm_case():
    """per curve: the inputs of a ragged batch of 700 and the restatement's (cols, aux) of the 48 sampled elements"""
    out = {}
    with _pool() as pool:
        for cid, cv in enumerate(CURVES):
            ins = _msm_inputs(cid, 700, 31 + cid)
            jobs = [(cv.name, *[v[i] for v in ins]) for i in SAMPLE]
            out[cid] = (ins, dict(zip(SAMPLE, pool.map(W.msm_job, jobs))))
    return out


def _dev(ins):
    import torch
    return [torch.from_numpy(_arr(v)).cuda() for v in ins]


@pytest.mark.gpu
@pytest.mark.parametrize("plan", ["four_lanes", "op_by_op", "runs"])
@pytest.mark.parametrize("curve_id", [0, 1])
def test_gpu_msm_every_column_against_the_restatement(curve_id, plan, msm_case, monkeypatch):
    import torch
    import plonky2_ecdsa_amd as p2e
    ctx = _ctx(monkeypatch, plan)
    prog = p2e.CurveProgram(ctx, p2e.CP_MSM, curve_id)
    assert (prog.num_cols, len(prog.describe()), prog.num_aux_cols) == (W.MSM_COLS, W.MSM_GENS, W.MSM_AUX)
    ins, ref = msm_case[curve_id]
    n = len(ins[0])
    dev = _dev(ins)
    full = torch.full((prog.num_cols, n + 3), -1, dtype=torch.int64, device="cuda")
    cols, err, valid, bad = prog.msm_witness_batch(*dev, cols=full[:, :n], ld=n + 3)
    torch.cuda.synchronize()
    ph = ctx.last_phase_ms()
    assert (ph["runs_launches"] > 0) == (plan == "runs")
    got = full[:, :n].cpu().numpy().view(np.uint64)
    err, valid = err.cpu().numpy(), valid.cpu().numpy()
    assert bool((full[:, n:] == -1).all())
    flagged = np.nonzero(err)[0].tolist()
    assert flagged == list(FLAGGED) and bad == len(FLAGGED)
    assert all(err[i] & R.ERR_INVERSE_OF_ZERO for i in FLAGGED) and not valid[list(FLAGGED)].any()
    assert valid[err == 0].all()
    for i in SAMPLE:
        if i in FLAGGED:
            assert ref[i] is None, i            # the walk raises exactly where the GPU flags
            continue
        assert np.array_equal(got[:, i], np.asarray(ref[i][0], np.uint64)), (curve_id, plan, i)
    # the compact container of the same batch (padded strides): expanded, the same matrix
    cmap, nn, nw = prog.compact_layout()
    nar = torch.full((nn, n + 3), -1, dtype=torch.int32, device="cuda")
    wid = torch.full((nw, n + 5), -1, dtype=torch.int64, device="cuda")
    _, _, cerr, _, cbad = prog.msm_witness_compact_batch(*dev, narrow=nar[:, :n], wide=wid[:, :n], ld_narrow=n + 3, ld_wide=n + 5)
    torch.cuda.synchronize()
    exp = prog.compact_expand(nar[:, :n].cpu().numpy(), wid[:, :n].cpu().numpy())
    clean = err == 0
    assert cbad == bad and np.array_equal(cerr.cpu().numpy(), err)
    assert np.array_equal(exp[:, clean], got[:, clean])
    assert bool((nar[:, n:] == -1).all()) and bool((wid[:, n:] == -1).all())
    # segments: disjoint blocks covering every column once
    covered = np.zeros(prog.num_cols, np.int32)
    for c0, nc in ctx.segments():
        covered[c0:c0 + nc] += 1
    assert (covered == 1).all()
    prog.close()


@pytest.mark.gpu
def test_gpu_msm_other_passes_against_the_restatement(msm_case):
    """aux of the MSM program against Walker.aux, gate-internal values against their definition (include/p2e.h
    p2e_gate_internal_batch) derived in Python from the digits"""
    import torch
    import plonky2_ecdsa_amd as p2e
    ctx = p2e.Context(device=0)
    for cid in (0, 1):
        prog = p2e.CurveProgram(ctx, p2e.CP_MSM, cid)
        ins, ref = msm_case[cid]
        n = len(ins[0])
        dev = _dev(ins)
        cols, err, valid, bad = prog.msm_witness_batch(*dev)
        aux, aerr, abad = prog.aux_witness_batch(tuple(dev), cols, n=n, ld=p2e._ld(cols))
        gate = prog.gate_internal_batch(aux, n=n)
        torch.cuda.synchronize()
        aux, gate = aux.cpu().numpy().view(np.uint64), gate.cpu().numpy().view(np.uint64)
        assert abad == 0
        for i in SAMPLE[::4]:
            if i in FLAGGED:
                continue
            assert np.array_equal(aux[:, i], np.asarray(ref[i][1], np.uint64)), (cid, i)
            want = []
            for d in reversed(range(131)):     # random access first, then is_equal (gadgets/curve_msm.rs:68-70)
                idx = 4 * ((ins[5][i] >> (2 * d)) & 3) + ((ins[4][i] >> (2 * d)) & 3)
                want += [(idx >> b) & 1 for _ in range(18) for b in range(4)]
                want += [int(idx != 0), pow(idx, P_GL - 2, P_GL) if idx else 0, idx, int(idx != 0), idx]
            assert np.array_equal(gate[:, i], np.asarray(want, np.uint64)), (cid, i)
        prog.close()


@pytest.mark.gpu
@pytest.mark.parametrize("curve_id", [0, 1])
def test_gpu_fixed_base_every_column_against_the_walker(curve_id, monkeypatch):
    """a random base per curve: every column of every element against Walker.fixed_base_curve_mul, in the three plans;
    the aux and gate-internal passes; the segment blocks"""
    import torch
    import plonky2_ecdsa_amd as p2e
    cv = CURVES[curve_id]
    base = cv.mul(R.SplitMix64(77 + curve_id).below(cv.n), cv.g)
    n = 300 + 13
    ks = _fb_inputs(cv, n, 5 + curve_id)
    with _pool() as pool:
        ref = pool.map(W.fixed_base_job, [(cv.name, base, k) for k in ks])
    want = np.asarray([r[0] for r in ref], np.uint64).T
    want_aux = np.asarray([r[1] for r in ref], np.uint64).T
    k_dev = torch.from_numpy(_arr(ks)).cuda()
    for plan in ("four_lanes", "op_by_op", "runs"):
        with monkeypatch.context() as mpc:
            ctx = _ctx(mpc, plan)
            prog = p2e.CurveProgram(ctx, p2e.CP_FIXED_BASE_MUL, curve_id, base=base)
            assert (prog.num_cols, len(prog.describe()), prog.num_aux_cols) == (W.FB_COLS, W.FB_GENS, W.FB_AUX)
            full = torch.full((prog.num_cols, n + 1), -1, dtype=torch.int64, device="cuda")
            cols, err, valid, bad = prog.mul_witness_batch(None, None, k_dev, cols=full[:, :n], ld=n + 1)
            torch.cuda.synchronize()
            ph = ctx.last_phase_ms()
            assert (ph["fbrun_launches"] > 0) == (plan == "runs")
            assert bad == 0 and bool(valid.all()) and bool((full[:, n] == -1).all())
            assert np.array_equal(full[:, :n].cpu().numpy().view(np.uint64), want), plan
            covered = np.zeros(prog.num_cols, np.int32)
            for c0, nc in ctx.segments():
                covered[c0:c0 + nc] += 1
            assert (covered == 1).all()
            cmap, nn, nw = prog.compact_layout()
            nar, wid, _, _, cbad = prog.mul_witness_compact_batch(None, None, k_dev)
            torch.cuda.synchronize()
            assert cbad == 0 and np.array_equal(prog.compact_expand(nar.cpu().numpy(), wid.cpu().numpy()), want)
            if plan == "four_lanes":
                aux, aerr, abad = prog.aux_witness_batch((None, None, k_dev), cols, n=n, ld=n + 1)
                gate = prog.gate_internal_batch(aux, n=n)
                torch.cuda.synchronize()
                assert abad == 0 and np.array_equal(aux.cpu().numpy().view(np.uint64), want_aux)
                gate = gate.cpu().numpy().view(np.uint64)
                for i in (0, 2, 3, n - 1):
                    g = []
                    for w in range(66):          # is_equal first, then random access (gadgets/curve_fixed_base.rs:57-60)
                        d = (ks[i] >> (4 * w)) & 15
                        g += [int(d != 0), pow(d, P_GL - 2, P_GL) if d else 0, d, int(d != 0), d]
                        g += [(d >> b) & 1 for _ in range(18) for b in range(4)]
                    assert np.array_equal(gate[:, i], np.asarray(g, np.uint64)), i
                ux, uerr, ubad = prog.ux_witness_batch((None, None, k_dev), cols, aux, n=n, ld=n + 1)
                torch.cuda.synchronize()
                assert ubad == 0
            prog.close()


@pytest.mark.gpu
@pytest.mark.parametrize("curve_id", [0, 1])
def test_gpu_fixed_base_of_the_generator_equals_the_verifiers_scope(curve_id):
    """base = the curve's generator: the witness, aux and constraint-block (ux) columns of the fixed-base program equal the
    `fixed_base` scope of the curve's verifier (P-256: the verifier curve program; secp256k1: the built-in verify
    program) for the same u1"""
    import torch
    import plonky2_ecdsa_amd as p2e
    cv = CURVES[curve_id]
    ctx = p2e.Context(device=0)
    n = 200
    sig = p2e.synth_signatures_curve(curve_id, seed=8, n=n)
    sig_dev = [torch.from_numpy(a).cuda() for a in sig]
    msg, s = _ints(sig[0]), _ints(sig[2])
    u1 = [m * pow(x, -1, cv.n) % cv.n for m, x in zip(msg, s)]
    if curve_id == 1:
        ver = p2e.CurveProgram(ctx, p2e.CP_VERIFY, p2e.CURVE_P256, cv.mul(4242, cv.g))
        vcols, _, _, vbad = ver.verify_witness_batch(*sig_dev)
        vaux, _, vabad = ver.aux_witness_batch(tuple(sig_dev), vcols, n=n)
        vux, _, vubad = ver.ux_witness_batch(tuple(sig_dev), vcols, vaux, n=n)
        vdesc, vuxd, vaux_desc = ver.describe(), ver.ux_describe(), ver.aux_describe()
    else:
        vcols, _, _, vbad = ctx.ecdsa_verify_witness_batch(*sig_dev)
        vaux, _, vabad = ctx.aux_witness_batch(p2e.PROGRAM_VERIFY, sig_dev[4], vcols, n=n)
        vux, _, vubad = ctx.ux_witness_batch(p2e.PROGRAM_VERIFY, tuple(sig_dev), vcols, vaux, n=n)
        vdesc, vuxd = p2e.schedule_describe(p2e.PROGRAM_VERIFY), p2e.ux_describe(p2e.PROGRAM_VERIFY)
        vaux_desc = p2e.aux_describe(p2e.PROGRAM_VERIFY)
    fb = p2e.CurveProgram(ctx, p2e.CP_FIXED_BASE_MUL, curve_id, base=cv.g)
    k_dev = torch.from_numpy(_arr(u1)).cuda()
    fcols, _, _, fbad = fb.mul_witness_batch(None, None, k_dev)
    faux, _, fabad = fb.aux_witness_batch((None, None, k_dev), fcols, n=n)
    fux, _, fubad = fb.ux_witness_batch((None, None, k_dev), fcols, faux, n=n)
    torch.cuda.synchronize()
    assert (vbad, vabad, vubad, fbad, fabad, fubad) == (0, 0, 0, 0, 0, 0)
    # witness columns: the scope's generators are the program's, shifted
    g = [k for k, d in enumerate(vdesc) if d[4].startswith("fixed_base/")]
    assert g == list(range(g[0], g[-1] + 1)) and len(g) == len(fb.describe())
    c0, c1 = vdesc[g[0]][2], vdesc[g[-1]][2] + vdesc[g[-1]][3]
    assert [d[:2] + (d[2] - c0, d[3]) for d in (vdesc[k] for k in g)] == [d[:4] for d in fb.describe()]
    assert c1 - c0 == fb.num_cols and torch.equal(vcols[c0:c1], fcols)
    # constraint-block columns: the scope's ux blocks are contiguous and hold the program's whole ux matrix
    u0, u1_ = vuxd[g[0]][0], vuxd[g[-1]][0] + vuxd[g[-1]][1]
    assert u1_ - u0 == fb.num_ux_cols and [(a - u0, b) for a, b in (vuxd[k] for k in g)] == fb.ux_describe()
    assert torch.equal(vux[u0:u1_], fux)
    # aux columns: the scope's 4-bit split and its 66 windows
    sc = [d for d in vaux_desc if d[-1].startswith("fixed_base")]
    a0, a1 = sc[0][1], sc[-1][1] + sc[-1][2]
    assert a1 - a0 == fb.num_aux_cols and torch.equal(vaux[a0:a1], faux)
    fb.close()


@pytest.mark.gpu
def test_gpu_msm_full_size_p256():
    """2^16 distinct P-256 elements in the default plan (runs) bit-identical, every column, to the op-by-op plan (compared
    on the device); for every 8th element across the whole batch the final add's output equals n p + m q from host big
    integers"""
    import torch
    import plonky2_ecdsa_amd as p2e
    cv = R.P256
    N = 1 << 16
    ins = _msm_inputs(1, N, 901)
    for k in (7, 10, 11):                          # the flagged edge rows of _msm_inputs: fresh clean values here
        ins[4][k], ins[5][k] = 3 + k, 5 + k
        ins[0][k], ins[1][k] = ins[0][k + 20], ins[1][k + 20]
    check = list(range(0, N, 8)) + list(range(N - 64, N))
    with _pool() as pool:
        want = pool.map(W.native_msm_job, [(cv.name, (ins[0][i], ins[1][i]), (ins[2][i], ins[3][i]), ins[4][i], ins[5][i])
                                           for i in check], chunksize=64)
    dev = _dev(ins)
    ctx = p2e.Context(device=0)
    prog = p2e.CurveProgram(ctx, p2e.CP_MSM, p2e.CURVE_P256)
    a, err, valid, bad = prog.msm_witness_batch(*dev)
    torch.cuda.synchronize()
    assert bad == 0 and ctx.last_phase_ms()["runs_launches"] > 0
    last = prog.describe()[-10:]                    # the unblinding add: its x3, y3 sub generators
    x3 = last[6][2]
    y3 = last[9][2]
    idx = torch.tensor(check, device="cuda")
    got_x = a[x3:x3 + 9].index_select(1, idx).cpu().numpy().view(np.uint64)
    got_y = a[y3:y3 + 9].index_select(1, idx).cpu().numpy().view(np.uint64)
    for j, i in enumerate(check):
        assert want[j] is not None
        assert R.value_of([int(v) for v in got_x[:, j]]) == want[j][0] and R.value_of([int(v) for v in got_y[:, j]]) == want[j][1], i
    os.environ["P2E_CP_NO_RUNS"] = "1"
    try:
        b, err2, _, bad2 = prog.msm_witness_batch(*dev)
        torch.cuda.synchronize()
        assert ctx.last_phase_ms()["runs_launches"] == 0
    finally:
        del os.environ["P2E_CP_NO_RUNS"]
    assert bad2 == 0 and torch.equal(a, b)
    del a, b
    prog.close()


@pytest.mark.gpu
@pytest.mark.parametrize("plan", ["four_lanes", "op_by_op", "runs"])
@pytest.mark.parametrize("kind", ["msm", "fixed_base"])
def test_gpu_column_blocks_are_final_when_their_event_fires(kind, plan, monkeypatch):
    """include/p2e.h p2e_segments_describe / p2e_segment_stream_wait for the two programs: the blocks of an ASYNCHRONOUS
    fill are disjoint, cover every column once, and block k holds its final values as soon as its event has fired -- a copy
    stream waits for each block's event and copies it out of the (poisoned) output while later launches still run; the
    copies together must be the synchronous fill's matrix.  Both containers (the compact one through segment_sync)."""
    import torch
    import plonky2_ecdsa_amd as p2e
    from plonky2_ecdsa_amd.dist import compact_row_ranges
    curve_id = 1 if kind == "msm" else 0
    cv = CURVES[curve_id]
    n = 1000 + 77
    if plan == "op_by_op":
        monkeypatch.setenv("P2E_QUAD_MAX_N", "0")
    elif plan == "runs":
        monkeypatch.setenv("P2E_CP_RUNS_MIN_N", "1")
    if kind == "msm":
        ins = _msm_inputs(curve_id, n, 71)
        for k in FLAGGED:                           # clean inputs only
            ins[4][k], ins[5][k] = 3 + k, 5 + k
            ins[0][k], ins[1][k] = ins[0][k + 20], ins[1][k + 20]
        dev = _dev(ins)
        make = lambda c: p2e.CurveProgram(c, p2e.CP_MSM, curve_id)
        fill = lambda pr, **kw: pr.msm_witness_batch(*dev, **kw)
        fillc = lambda pr, **kw: pr.msm_witness_compact_batch(*dev, **kw)
    else:
        base = cv.mul(0xBA5E + 1, cv.g)
        k_dev = torch.from_numpy(_arr(_fb_inputs(cv, n, 13))).cuda()
        make = lambda c: p2e.CurveProgram(c, p2e.CP_FIXED_BASE_MUL, curve_id, base=base)
        fill = lambda pr, **kw: pr.mul_witness_batch(None, None, k_dev, **kw)
        fillc = lambda pr, **kw: pr.mul_witness_compact_batch(None, None, k_dev, **kw)
    sync_prog = make(p2e.Context(device=0))
    want_t, _, _, wbad = fill(sync_prog)
    torch.cuda.synchronize()
    assert wbad == 0
    want_t = want_t.contiguous()
    work, copy = torch.cuda.Stream(), torch.cuda.Stream()
    ctx = p2e.Context(device=0, stream=work.cuda_stream, asynchronous=True)
    prog = make(ctx)
    nc_all = prog.num_cols
    cols = torch.full((nc_all, n + 1), -1, dtype=torch.int64, device="cuda")
    snap = torch.full((nc_all, n), -2, dtype=torch.int64, device="cuda")
    err = torch.zeros(n, dtype=torch.uint8, device="cuda")
    valid = torch.zeros(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    fill(prog, cols=cols[:, :n], err=err, valid=valid, ld=n + 1)
    segs = ctx.segments()
    covered = np.zeros(nc_all, dtype=np.int32)
    with torch.cuda.stream(copy):
        for k, (c0, nc) in enumerate(segs):
            covered[c0:c0 + nc] += 1
            ctx.segment_stream_wait(k, copy.cuda_stream)
            snap[c0:c0 + nc].copy_(cols[c0:c0 + nc, :n], non_blocking=True)
    assert (covered == 1).all() and len(segs) >= 2
    copy.synchronize()
    assert ctx.sync() == 0
    ph = ctx.last_phase_ms()
    assert (ph["runs_launches"] + ph["fbrun_launches"] > 0) == (plan == "runs")
    assert torch.equal(snap, want_t) and torch.equal(cols[:, :n], want_t) and bool((cols[:, n] == -1).all())
    # the host-blocking form, and the compact container (a block of columns = a block of rows of each matrix)
    cmap, nn, nw = prog.compact_layout()
    nar = torch.full((nn, n + 1), -1, dtype=torch.int32, device="cuda")
    wid = torch.full((nw, n + 1), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    fillc(prog, narrow=nar[:, :n], wide=wid[:, :n], err=err, valid=valid, ld_narrow=n + 1, ld_wide=n + 1)
    segs2 = ctx.segments()
    nr, wr = compact_row_ranges(cmap, segs2)
    got_n, got_w = [], []
    for k in range(len(segs2)):
        ctx.segment_sync(k)
        with torch.cuda.stream(copy):
            got_n.append((nr[k], nar[nr[k][0]:nr[k][0] + nr[k][1], :n].clone()))
            got_w.append((wr[k], wid[wr[k][0]:wr[k][0] + wr[k][1], :n].clone()))
    copy.synchronize()
    assert ctx.sync() == 0
    is_wide = (cmap & p2e.COMPACT_WIDE) != 0
    want_n = want_t[torch.from_numpy(np.nonzero(~is_wide)[0]).cuda()]
    want_w = want_t[torch.from_numpy(np.nonzero(is_wide)[0]).cuda()]
    for (r0, rn), t in got_n:
        assert torch.equal(t.to(torch.int64) & 0xFFFFFFFF, want_n[r0:r0 + rn])
    for (r0, rn), t in got_w:
        assert torch.equal(t, want_w[r0:r0 + rn])
    assert sum(rn for (_, rn), _ in got_n) == nn and sum(rn for (_, rn), _ in got_w) == nw
    prog.close()
    sync_prog.close()


@pytest.mark.gpu
def test_gpu_msm_and_fixed_base_misuse():
    import torch
    import plonky2_ecdsa_amd as p2e
    ctx = p2e.Context(device=0)
    k1 = R.SECP256K1
    with pytest.raises(p2e.P2EError):
        p2e.CurveProgram(ctx, 9, p2e.CURVE_P256, R.P256.g)
    with pytest.raises(p2e.P2EError) as e:
        p2e.CurveProgram(ctx, p2e.CP_FIXED_BASE_MUL, p2e.CURVE_P256, base=((1 << 256) - 1, 5))
    assert "fixed-base point" in str(e.value)
    with pytest.raises(p2e.P2EError) as e:
        p2e.CurveProgram(ctx, p2e.CP_FIXED_BASE_MUL, p2e.CURVE_SECP256K1, base=(k1.g[0], k1.g[1] ^ 2))
    assert "fixed-base point is not on the curve" in str(e.value)
    with pytest.raises(p2e.P2EError):
        p2e.CurveProgram(ctx, p2e.CP_FIXED_BASE_MUL, p2e.CURVE_P256, base=k1.g)              # a point of the other curve
    with pytest.raises(p2e.P2EError):
        p2e.CurveProgram(ctx, p2e.CP_FIXED_BASE_MUL, p2e.CURVE_P256)                          # no base at all
    n = 16
    ins = _dev(_msm_inputs(0, n, 3))
    win = p2e.CurveProgram(ctx, p2e.CP_WINDOWED_MUL, p2e.CURVE_SECP256K1, k1.mul(5, k1.g))
    msm = p2e.CurveProgram(ctx, p2e.CP_MSM, p2e.CURVE_SECP256K1)
    with pytest.raises(p2e.P2EError):
        win.msm_witness_batch(*ins)                                                            # an MSM fill on a windowed program
    with pytest.raises(p2e.P2EError):
        msm.mul_witness_batch(ins[0], ins[1], ins[4])                                          # a mul fill on the MSM program
    with pytest.raises(p2e.P2EError):
        win.mul_witness_batch(None, None, ins[4])                                              # a windowed program needs its point
    cols, err, valid, bad = msm.msm_witness_batch(*ins)
    aux, _, _ = msm.aux_witness_batch(tuple(ins), cols, n=n, ld=p2e._ld(cols))
    with pytest.raises(p2e.P2EError) as e:
        msm.ux_witness_batch(tuple(ins), cols, aux, n=n, ld=p2e._ld(cols))                    # the ux pass: not for MSM yet
    assert "no slot for q" in str(e.value)
    cols, err, valid, bad = msm.msm_witness_batch(*ins)                                       # a valid call still works
    wcols, _, _, wbad = win.mul_witness_batch(ins[0], ins[1], ins[4])
    torch.cuda.synchronize()
    assert bad == 3 and wbad == 2      # (the MSM's three flagged rows; the windowed multiplication's scalar 0 in rows 5 and 7)
    win.close()
    msm.close()
