"""Column blocks of the curve programs whose generators are NOT laid out in op order (include/p2e.h p2e_segments_describe).

curve_scalar_mul_windowed, curve_scalar_mul and verify_p256_message_circuit place a 10-column scalar generator between the
columns of their last curve ops, so the last expansion launch completes two runs of columns with a scalar-phase block
between them.  The blocks must still be disjoint and cover every column once, and each must hold its final values when its
event fires: a copy stream waits per block and copies it out of a poisoned output while later launches still run.  The
expectation is the C oracle's matrix (oracle/p2e_oracle.c) on every column of every element.  Modelled on
test_gpu_column_blocks_are_final_when_their_event_fires of test_gpu_msm_fixed_base.py (the MSM and fixed-base programs,
whose generators are in op order)."""
import numpy as np
import pytest

import p2e_ref as R

CURVES = [R.SECP256K1, R.P256]
# name -> (kind of include/p2e.h P2E_CP_*, curve)
PROGRAMS = {"windowed_secp256k1": (1, 0), "scalar_mul_p256": (2, 1), "verify_p256": (3, 1)}
N = 313   # a full workgroup of paired stores and a ragged tail


@pytest.fixture(scope="module")
def oracle():
    """name -> (inputs, blinding point as ints, the C oracle's columns), computed once and left unchanged"""
    import oracle_c
    import plonky2_ecdsa_amd as p2e
    out = {}
    for name, (kind, curve) in PROGRAMS.items():
        cv = CURVES[curve]
        blind_i = cv.mul(R.SplitMix64(4100 + kind).below(cv.n), cv.g)
        sig = p2e.synth_signatures_curve(curve, seed=900 + kind, n=N)
        args = tuple(sig) if kind == 3 else (sig[3], sig[4], sig[0])   # (the public keys as points, the messages as scalars)
        cols, _aux, err, flags = oracle_c.curve_program(kind, curve, blind_i, args, want_aux=False)
        assert not err.any() and flags.all()                          # clean inputs only
        out[name] = (args, blind_i, cols)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name,plan", [(name, plan) for name in PROGRAMS for plan in ("four_lanes", "op_by_op", "runs")
                                       if not (plan == "runs" and PROGRAMS[name][0] == 2)])   # (curve_scalar_mul has no window loop: no run plan)
def test_gpu_column_blocks_of_programs_with_a_gap_are_disjoint_and_final_when_their_event_fires(name, plan, oracle, monkeypatch):
    import torch
    import plonky2_ecdsa_amd as p2e
    from plonky2_ecdsa_amd.dist import compact_row_ranges
    kind, curve = PROGRAMS[name]
    if plan == "op_by_op":
        monkeypatch.setenv("P2E_QUAD_MAX_N", "0")
    elif plan == "runs":
        monkeypatch.setenv("P2E_CP_RUNS_MIN_N", "1")
    args, blind_i, want = oracle[name]
    n = N
    want_t = torch.from_numpy(want.view(np.int64)).cuda()
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in args]
    work, copy = torch.cuda.Stream(), torch.cuda.Stream()
    ctx = p2e.Context(device=0, stream=work.cuda_stream, asynchronous=True)
    prog = p2e.CurveProgram(ctx, kind, curve, blind_i)
    fill = prog.verify_witness_batch if kind == 3 else prog.mul_witness_batch
    fillc = prog.verify_witness_compact_batch if kind == 3 else prog.mul_witness_compact_batch
    nc_all = prog.num_cols
    assert nc_all == want.shape[0]
    cols = torch.full((nc_all, n + 1), -1, dtype=torch.int64, device="cuda")
    snap = torch.full((nc_all, n), -2, dtype=torch.int64, device="cuda")
    err = torch.zeros(n, dtype=torch.uint8, device="cuda")
    valid = torch.zeros(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    fill(*dev, cols=cols[:, :n], err=err, valid=valid, ld=n + 1)
    segs = ctx.segments()
    covered = np.zeros(nc_all, dtype=np.int32)
    with torch.cuda.stream(copy):
        for k, (c0, nc) in enumerate(segs):
            covered[c0:c0 + nc] += 1
            ctx.segment_stream_wait(k, copy.cuda_stream)
            snap[c0:c0 + nc].copy_(cols[c0:c0 + nc, :n], non_blocking=True)
    copy.synchronize()
    assert ctx.sync() == 0
    twice = np.nonzero(covered != 1)[0]
    assert len(twice) == 0, f"columns not in exactly one block: {twice[0]}..{twice[-1]} ({len(twice)})"
    assert sum(nc for _c0, nc in segs) == nc_all and len(segs) >= 2
    ph = ctx.last_phase_ms()
    assert (ph["runs_launches"] > 0) == (plan == "runs")
    assert not err.any().item() and valid.all().item()
    assert torch.equal(snap, want_t) and torch.equal(cols[:, :n], want_t)
    assert bool((cols[:, n] == -1).all())
    # the host-blocking form, and the compact container (a block of columns = a block of rows of each matrix)
    cmap, nn, nw = prog.compact_layout()
    nar = torch.full((nn, n + 1), -1, dtype=torch.int32, device="cuda")
    wid = torch.full((nw, n + 1), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    fillc(*dev, narrow=nar[:, :n], wide=wid[:, :n], err=err, valid=valid, ld_narrow=n + 1, ld_wide=n + 1)
    segs2 = ctx.segments()
    assert segs2 == segs
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
    assert bool((nar[:, n] == -1).all()) and bool((wid[:, n] == -1).all())
    prog.close()
