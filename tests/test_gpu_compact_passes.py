"""The aux, gate-internal, constraint-block and wire-assembly passes on the compact container (u32 narrow + u64 wide
matrices, u32 aux matrix) against the same passes on the u64 matrices, on every element, for both built-in programs and
all five curve-program kinds on both curves; against the constraint replay (oracle/check_circuit.py) on columns rebuilt
from the compact container alone; and the MSM program's constraint-block pass, which reads q, in both forms."""
import numpy as np
import pytest

import check_circuit as CC
import oracle_c
import p2e_ref as R
import ux_oracle as UX

pytestmark = pytest.mark.gpu

CURVES = [R.SECP256K1, R.P256]
N = 300                                  # one full workgroup of paired stores + a 44-element tail
REPLAYED = (0, 1, 63, 64, 255, 299)
CURVE_PROGRAMS = [(kind, curve) for curve in (0, 1) for kind in (1, 2, 3, 4, 5) if not (kind == 3 and curve == 0)]


@pytest.fixture(scope="module")
def gpu():
    import torch
    import plonky2_ecdsa_amd as p2e
    return p2e, torch, p2e.Context(device=0)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _padded(torch, t, pad):
    """a copy of matrix t inside a wider one: a (rows, n) view with row stride n + pad, and the wider matrix"""
    big = torch.full((t.shape[0], t.shape[1] + pad), -1, dtype=t.dtype, device=t.device)
    big[:, :t.shape[1]].copy_(t)
    return big[:, :t.shape[1]], big


def _builtin_inputs(p2e, torch, program, n, seed):
    sigs = p2e.synth_signatures(seed=seed, n=n)
    dev = [torch.from_numpy(a).cuda() for a in sigs]
    if program == 0:
        return sigs, None, dev, dev[4]
    rng = R.SplitMix64(seed + 1)
    ks = [rng.below(R.N) for _ in range(n)]
    kd = torch.from_numpy(oracle_c.pack256(ks)).cuda()
    return sigs, ks, [dev[3], dev[4], kd], dev[4]


def _builtin_fills(ctx, program, inputs):
    if program == 0:
        cols, _e, _v, bad = ctx.ecdsa_verify_witness_batch(*inputs)
        narrow, wide, _e, _v, cbad = ctx.ecdsa_verify_witness_compact_batch(*inputs)
    else:
        cols, _e, _v, bad = ctx.glv_mul_witness_batch(*inputs)
        narrow, wide, _e, _v, cbad = ctx.glv_mul_witness_compact_batch(*inputs)
    assert bad == 0 and cbad == 0
    return cols, narrow, wide


# ---- 4. built-in programs ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("program", [0, 1])
def test_builtin_compact_chain_equals_the_u64_chain(program, gpu):
    p2e, torch, ctx = gpu
    n = N
    sigs, ks, inputs, pky = _builtin_inputs(p2e, torch, program, n, 6060 + program)
    cols, narrow, wide = _builtin_fills(ctx, program, inputs)
    aux, _e, abad = ctx.aux_witness_batch(program, pky, cols)
    gate = ctx.gate_internal_batch(program, aux)
    ux32, e32, b32 = ctx.ux_witness_batch(program, inputs, cols, aux, u32=True)
    ux64, e64, b64 = ctx.ux_witness_batch(program, inputs, cols, aux, u32=False)
    assert abad == b32 == b64 == 0
    k = p2e.ux_num_cols(program)
    # the oracle's own walk of the same inputs: every element and column of both passes, from both containers
    exp = UX.builtin(program, list(sigs) if program == 0 else [sigs[3], sigs[4], oracle_c.pack256(ks)])
    dexp, blocks = UX.to_device(torch, exp), UX.layout("builtin", program)["blocks"]
    assert not exp["err"].any() and [tuple(b) for b in p2e.ux_describe(program)] == blocks
    UX.assert_same_device(torch, "u64 matrices, ux as u32", ux32, dexp["ux32"], dexp, blocks)
    UX.assert_same_device(torch, "u64 matrices, ux as u64", ux64, dexp["ux32"], dexp, blocks)
    UX.assert_same_device(torch, "u64 aux, gate", gate, dexp["gate"], dexp)
    for pad in (3, 6):                              # the narrow source on an odd and on an even padded stride
        nar, _big = _padded(torch, narrow, pad)
        assert p2e._ld(nar) == n + pad
        aux32, _e, cabad = ctx.aux_witness_compact_batch(program, pky, nar)
        cgate = ctx.gate_internal_compact_batch(program, aux32)
        big32 = torch.full((k, n + 6), -1, dtype=torch.int32, device="cuda")    # even stride: paired stores + tail
        big64 = torch.full((k, n + 5), -1, dtype=torch.int64, device="cuda")    # odd stride: one element per store
        c32, ce32, cb32 = ctx.ux_witness_compact_batch(program, inputs, nar, aux32, ux=big32[:, :n])
        c64, ce64, cb64 = ctx.ux_witness_compact_batch(program, inputs, nar, aux32, ux=big64[:, :n])
        torch.cuda.synchronize()
        assert cabad == cb32 == cb64 == 0
        assert torch.equal(aux32.to(torch.int64), aux)
        assert torch.equal(cgate, gate)
        assert torch.equal(c32, ux32) and torch.equal(c64, ux64)
        assert torch.equal(ce32, e32) and torch.equal(ce64, e64)
        assert bool((big32[:, n:] == -1).all()) and bool((big64[:, n:] == -1).all())      # padding untouched
        UX.assert_same_device(torch, f"compact container (pad {pad}), ux as u32", c32, dexp["ux32"], dexp, blocks)
        UX.assert_same_device(torch, f"compact container (pad {pad}), ux as u64", c64, dexp["ux32"], dexp, blocks)
        UX.assert_same_device(torch, f"u32 aux (pad {pad}), gate", cgate, dexp["gate"], dexp)
    # independent check: columns rebuilt from the compact container alone, through the constraint replay
    h_cols = p2e.compact_expand(program, _u32(narrow), _u64(wide))
    h_aux, h_ux, h_gate = _u32(aux32), _u32(c32), _u64(cgate)
    for i in (0, 255, 256, 299):
        if program == 0:
            c = CC.check_verify(h_cols[:, i], *CC.unpack_inputs(sigs, i), aux=h_aux[:, i], ux=h_ux[:, i])
        else:
            px, py = CC.unpack_inputs(sigs[3:5], i)
            c = CC.check_glv_mul(h_cols[:, i], px, py, ks[i], aux=h_aux[:, i], ux=h_ux[:, i])
        assert len(c.ux) == k and np.array_equal(h_gate[:, i], np.array(c.gate, dtype=np.uint64))
    # staged host-pointer path on 3 signatures
    hctx = p2e.Context(device=0, host_pointers=True)
    hin = [a[:3].cpu().numpy() for a in inputs]
    if program == 0:
        hn, hw, _e, _v, hb = hctx.ecdsa_verify_witness_compact_batch(*hin)
    else:
        hn, hw, _e, _v, hb = hctx.glv_mul_witness_compact_batch(*hin)
    ha, _e, hab = hctx.aux_witness_compact_batch(program, hin[4] if program == 0 else hin[1], hn)
    hg = hctx.gate_internal_compact_batch(program, ha)
    hu, he, hub = hctx.ux_witness_compact_batch(program, hin, hn, ha)
    hu64, _e, _b = hctx.ux_witness_compact_batch(program, hin, hn, ha, u32=False)
    assert hb == hab == hub == 0 and not np.asarray(he).any()
    assert np.array_equal(np.asarray(ha), h_aux[:, :3]) and np.array_equal(np.asarray(hg), h_gate[:, :3])
    assert np.array_equal(np.asarray(hu), h_ux[:, :3]) and np.array_equal(np.asarray(hu64), h_ux[:, :3].astype(np.uint64))
    UX.assert_same_numpy("host-pointer context, ux as u32", np.asarray(hu).astype(np.uint64), exp["ux"][:, :3], blocks=blocks)
    UX.assert_same_numpy("host-pointer context, ux as u64", np.asarray(hu64).view(np.uint64), exp["ux"][:, :3], blocks=blocks)
    UX.assert_same_numpy("host-pointer context, gate", np.asarray(hg).view(np.uint64), exp["gate"][:, :3])
    hctx.close()


# ---- 5. the limb-range flag ------------------------------------------------------------------------------------------------
def test_a_limb_that_is_no_u29_value_is_flagged_by_both_sources(gpu):
    p2e, torch, ctx = gpu
    program, n, victim = 0, N, 257
    _sigs, _ks, inputs, pky = _builtin_inputs(p2e, torch, program, n, 7070)
    cols, narrow, _wide = _builtin_fills(ctx, program, inputs)
    aux, _e, _b = ctx.aux_witness_batch(program, pky, cols)
    aux32, _e, _b = ctx.aux_witness_compact_batch(program, pky, narrow)
    # the first result limb of the first add generator that is some later generator's operand
    desc, wiring = p2e.schedule_describe(program), p2e.schedule_wiring(program)
    operands = {src for ops, _rc in wiring for src, _nl in ops}
    col = next(d[2] for d in desc if d[0] == "add" and d[2] in operands)
    col_map, _nn, _nw = p2e.compact_layout(program)
    assert not col_map[col] & p2e.COMPACT_WIDE
    cols[col, victim] = 1 << 29
    narrow[int(col_map[col]), victim] = 1 << 29
    _ux, e64, b64 = ctx.ux_witness_batch(program, inputs, cols, aux)
    _ux, e32, b32 = ctx.ux_witness_compact_batch(program, inputs, narrow, aux32)
    torch.cuda.synchronize()
    want = np.zeros(n, np.uint8)
    want[victim] = p2e.ERR_LIMB_RANGE
    assert b64 == b32 == 1
    assert np.array_equal(e64.cpu().numpy(), want) and np.array_equal(e32.cpu().numpy(), want)


# ---- 6. wire assembly ------------------------------------------------------------------------------------------------------
def _scatter(n, mats, src, dst, cells):
    out = np.zeros((n, cells), dtype=np.uint64)
    kind, col = src >> 30, src & 0x3FFFFFFF
    for k, m in enumerate(mats):
        sel = kind == k
        if sel.any():
            out[:, dst[sel]] = m[col[sel]].T
    return out


def _names_narrow_and_wide(src, col_map, wide_flag):
    wit = src[(src >> 30) == 0]
    slots = col_map[wit]
    return bool(((slots & wide_flag) == 0).any()), bool(((slots & wide_flag) != 0).any())


def test_assemble_wires_compact_equals_the_u64_assembly_and_numpy(gpu):
    p2e, torch, ctx = gpu
    from plonky2_ecdsa_amd.wiremap import synthetic_wire_map, WIRE_SRC_AUX, WIRE_SRC_UX, WIRE_SRC_GATE
    n = 96                                           # one full 64-signature tile + a ragged one
    _sigs, _ks, dev, pky = _builtin_inputs(p2e, torch, 0, n, 8080)
    cols, narrow, wide = _builtin_fills(ctx, 0, dev)
    aux, _e, _b = ctx.aux_witness_batch(0, pky, cols)
    aux32, _e, _b = ctx.aux_witness_compact_batch(0, pky, narrow)
    gate = ctx.gate_internal_compact_batch(0, aux32)
    ux32, _e, _b = ctx.ux_witness_compact_batch(0, dev, narrow, aux32)
    ux64, _e, _b = ctx.ux_witness_compact_batch(0, dev, narrow, aux32, u32=False)
    torch.cuda.synchronize()
    mats = [_u64(cols), _u64(aux), _u32(ux32), _u64(gate)]
    col_map, _nn, _nw = p2e.compact_layout(0)
    # the synthetic placement with gate sources, ux as u32
    src, dst, nw, deg = synthetic_wire_map(0, with_gate=True)
    assert _names_narrow_and_wide(src, col_map, p2e.COMPACT_WIDE) == (True, True)
    wm = ctx.wire_map(0, src, dst, nw, deg)
    got = ctx.assemble_wires_compact(wm, narrow, wide, aux32, ux32, gate)
    ref = ctx.assemble_wires(wm, cols, aux, ux32, gate)
    torch.cuda.synchronize()
    assert torch.equal(got, ref)
    assert np.array_equal(_u64(got), _scatter(n, mats, src, dst, nw * deg))
    del got, ref
    # a random map over all four matrices, ux as u64; cells no entry names keep the caller's values
    rng = np.random.default_rng(15)
    cells, cnt = 1 << 18, 100_001
    q = cnt // 4
    rsrc = np.concatenate([rng.integers(0, p2e.VERIFY_COLS, q), WIRE_SRC_AUX | rng.integers(0, p2e.VERIFY_AUX_COLS, q),
                           WIRE_SRC_UX | rng.integers(0, p2e.VERIFY_UX_COLS, q),
                           WIRE_SRC_GATE | rng.integers(0, p2e.VERIFY_GATE_COLS, cnt - 3 * q)]).astype(np.uint32)
    rdst = rng.permutation(cells)[:cnt].astype(np.uint32)
    assert _names_narrow_and_wide(rsrc, col_map, p2e.COMPACT_WIDE) == (True, True)
    wm2 = ctx.wire_map(0, rsrc, rdst, 64, cells // 64)
    pre = torch.full((n, cells + 5), -7, dtype=torch.int64, device="cuda")
    ctx.assemble_wires_compact(wm2, narrow, wide, aux32, ux64, gate, wires=pre[:, :cells])
    ref = ctx.assemble_wires(wm2, cols, aux, ux64, gate)
    torch.cuda.synchronize()
    named = np.zeros(cells, dtype=bool)
    named[rdst] = True
    got = pre.cpu().numpy()
    want = _scatter(n, mats, rsrc, rdst, cells).view(np.int64)
    assert np.array_equal(got[:, :cells][:, named], want[:, named])
    assert np.array_equal(ref.cpu().numpy()[:, named], want[:, named])
    assert (got[:, :cells][:, ~named] == -7).all() and (got[:, cells:] == -7).all()
    # a map that names no wide column: wide may be NULL; one that names one must get it
    nsrc = np.nonzero((col_map & p2e.COMPACT_WIDE) == 0)[0][:500].astype(np.uint32)
    ndst = rng.permutation(1000)[:500].astype(np.uint32)
    only_narrow = ctx.wire_map(0, nsrc, ndst, 10, 100)
    w3 = ctx.assemble_wires_compact(only_narrow, narrow=narrow)
    torch.cuda.synchronize()
    assert np.array_equal(_u64(w3), _scatter(n, mats, nsrc, ndst, 1000))
    with pytest.raises(p2e.P2EError):
        ctx.assemble_wires_compact(wm2, narrow, None, aux32, ux64, gate)
    with pytest.raises(p2e.P2EError):                       # ld_narrow < n
        ctx.assemble_wires_compact(only_narrow, narrow=narrow[:, :n - 1].contiguous(), n=n)
    # staged host-pointer path
    hctx = p2e.Context(device=0, host_pointers=True)
    hw = hctx.assemble_wires_compact(hctx.wire_map(0, rsrc, rdst, 64, cells // 64), _u32(narrow)[:, :5].copy(), _u64(wide)[:, :5].copy(),
                                     _u32(aux32)[:, :5].copy(), _u32(ux32)[:, :5].copy(), _u64(gate)[:, :5].copy())
    assert np.array_equal(np.asarray(hw)[:, named], want[:5][:, named].view(np.uint64))
    hctx.close()


def test_assemble_wires_compact_of_the_p256_verifier(gpu):
    p2e, torch, ctx = gpu
    cv = R.P256
    prog = p2e.CurveProgram(ctx, p2e.CP_VERIFY, p2e.CURVE_P256, cv.mul(31337, cv.g))
    n = 80
    dev = [torch.from_numpy(a).cuda() for a in p2e.synth_signatures_curve(p2e.CURVE_P256, seed=18, n=n)]
    narrow, wide, _e, valid, bad = prog.verify_witness_compact_batch(*dev)
    aux32, _e, _b = prog.aux_witness_compact_batch(dev, narrow)
    ux, _e, _b = prog.ux_witness_compact_batch(dev, narrow, aux32)
    gate = prog.gate_internal_compact_batch(aux32)
    torch.cuda.synchronize()
    assert bad == 0 and int(valid.sum()) == n
    mats = [prog.compact_expand(_u32(narrow), _u64(wide)), _u32(aux32), _u32(ux), _u64(gate)]
    limits = [prog.num_cols, prog.num_aux_cols, prog.num_ux_cols, prog.num_gate_cols]
    rng = np.random.default_rng(19)
    cnt, cells = 60_003, 1 << 17
    kinds = rng.integers(0, 4, cnt).astype(np.uint32)
    colsel = np.array([rng.integers(0, limits[k]) for k in kinds], dtype=np.uint32)
    src, dst = (kinds << 30) | colsel, rng.permutation(cells)[:cnt].astype(np.uint32)
    assert _names_narrow_and_wide(src, prog.compact_layout()[0], p2e.COMPACT_WIDE) == (True, True)
    wires = ctx.assemble_wires_compact(prog.wire_map(src, dst, 128, cells // 128), narrow, wide, aux32, ux, gate)
    torch.cuda.synchronize()
    assert np.array_equal(_u64(wires), _scatter(n, mats, src, dst, cells))
    prog.close()


# ---- 7. curve programs -----------------------------------------------------------------------------------------------------
def _curve_case(p2e, torch, ctx, kind, curve, n, seed):
    """(program, replay inputs of element i, device input tuple, u64 fill, compact fill) with random, unflagged inputs"""
    cv = CURVES[curve]
    point = cv.mul(0xBEEF + kind, cv.g)                      # the blinding point, or the fixed base
    prog = p2e.CurveProgram(ctx, kind, curve, None if kind == p2e.CP_MSM else point)
    a = p2e.synth_signatures_curve(curve, seed=seed, n=n)
    b = p2e.synth_signatures_curve(curve, seed=seed + 1, n=n)
    d = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in a]
    if kind == p2e.CP_VERIFY:
        inputs, host = tuple(d), a
        fill, cfill = prog.verify_witness_batch(*d), prog.verify_witness_compact_batch(*d)
    elif kind == p2e.CP_MSM:
        host = [a[3], a[4], b[3], b[4], a[0], b[0]]          # (px, py, qx, qy, n, m)
        inputs = tuple(torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in host)
        fill, cfill = prog.msm_witness_batch(*inputs), prog.msm_witness_compact_batch(*inputs)
    else:
        px, py = (None, None) if kind == p2e.CP_FIXED_BASE_MUL else (d[3], d[4])
        inputs, host = (px, py, d[0]), [a[3], a[4], a[0]]
        fill, cfill = prog.mul_witness_batch(*inputs), prog.mul_witness_compact_batch(*inputs)
    assert fill[3] == 0 and cfill[4] == 0                    # nothing flagged: no element is left out of any comparison
    return prog, point, host, inputs, fill[0], cfill[0], cfill[1]


def _curve_replay(p2e, kind, curve, point, host, i, col_i, aux_i):
    cv = CURVES[curve]
    v = CC.unpack_inputs(host, i)
    if kind == p2e.CP_WINDOWED_MUL:
        return CC.check_windowed_mul(cv, col_i, *v, point, aux=aux_i)[0]
    if kind == p2e.CP_SCALAR_MUL:
        return CC.check_scalar_mul(cv, col_i, *v, point, aux=aux_i)[0]
    if kind == p2e.CP_VERIFY:
        return CC.check_verify_p256(col_i, *v, point, aux=aux_i)
    if kind == p2e.CP_MSM:
        return CC.check_msm(cv, col_i, *v, aux=aux_i)[0]
    return CC.check_fixed_base(cv, col_i, point, v[2], aux=aux_i)[0]


@pytest.mark.parametrize("kind,curve", CURVE_PROGRAMS)
def test_curve_program_compact_chain_equals_the_u64_chain(kind, curve, gpu):
    p2e, torch, ctx = gpu
    n = N
    prog, point, host, inputs, cols, narrow, wide = _curve_case(p2e, torch, ctx, kind, curve, n, 9090 + 10 * curve + kind)
    ld = p2e._ld(cols)
    ux_u64 = prog.msm_ux_witness_batch if kind == p2e.CP_MSM else prog.ux_witness_batch
    aux, _e, abad = prog.aux_witness_batch(inputs, cols, n=n, ld=ld)
    ux32, e32, b32 = ux_u64(inputs, cols, aux, n=n, ld=ld, u32=True)
    nar, _big = _padded(torch, narrow, 1 if curve else 4)    # odd stride on P-256, even on secp256k1
    aux32, _e, cabad = prog.aux_witness_compact_batch(inputs, nar, n=n)
    c32, ce32, cb32 = prog.ux_witness_compact_batch(inputs, nar, aux32, n=n, u32=True)
    assert abad == cabad == b32 == cb32 == 0
    assert torch.equal(aux32.to(torch.int64), aux)
    assert torch.equal(c32, ux32) and torch.equal(ce32, e32)
    # the oracle's own walk of the same inputs: every element and column, u32 and u64 outputs, both containers
    exp = UX.curve_program(kind, curve, point, host)
    dexp, blocks = UX.to_device(torch, exp), UX.layout("curve", kind, curve)["blocks"]
    assert not exp["err"].any() and [tuple(b) for b in prog.ux_describe()] == blocks
    assert (prog.num_ux_cols, prog.num_gate_cols) == (exp["ux"].shape[0], exp["gate"].shape[0])
    UX.assert_same_device(torch, "u64 matrices, ux as u32", ux32, dexp["ux32"], dexp, blocks)
    UX.assert_same_device(torch, "compact container, ux as u32", c32, dexp["ux32"], dexp, blocks)
    gate = None
    if prog.num_gate_cols:
        gate = prog.gate_internal_compact_batch(aux32, n=n)
        wgate = prog.gate_internal_batch(aux, n=n)
        assert torch.equal(gate, wgate)
        UX.assert_same_device(torch, "u32 aux, gate", gate, dexp["gate"], dexp)
        UX.assert_same_device(torch, "u64 aux, gate", wgate, dexp["gate"], dexp)
        del wgate
    ux64, _e, _b = ux_u64(inputs, cols, aux, n=n, ld=ld, u32=False)
    UX.assert_same_device(torch, "u64 matrices, ux as u64", ux64, dexp["ux32"], dexp, blocks)
    c64, _e, _b = prog.ux_witness_compact_batch(inputs, nar, aux32, n=n, u32=False)
    UX.assert_same_device(torch, "compact container, ux as u64", c64, dexp["ux32"], dexp, blocks)
    assert torch.equal(c64, ux64) and torch.equal(c64, c32.to(torch.int64))
    del ux64, c64
    torch.cuda.synchronize()
    h_cols = prog.compact_expand(_u32(narrow), _u64(wide))
    h_aux, h_ux = _u32(aux32), _u32(c32)
    assert np.array_equal(h_cols, _u64(cols))
    for i in REPLAYED:
        c = _curve_replay(p2e, kind, curve, point, host, i, h_cols[:, i], h_aux[:, i])
        assert np.array_equal(h_ux[:, i].astype(np.uint64), np.asarray(c.ux, np.uint64)), i
        if gate is not None:
            assert np.array_equal(_u64(gate)[:, i], np.asarray(c.gate, np.uint64)), i
    prog.close()


# ---- 8. the MSM program's constraint-block pass --------------------------------------------------------------------------
@pytest.mark.parametrize("curve", [0, 1])
def test_msm_constraint_block_pass_in_both_forms(curve, gpu):
    p2e, torch, ctx = gpu
    n = N
    prog, point, host, inputs, cols, narrow, wide = _curve_case(p2e, torch, ctx, p2e.CP_MSM, curve, n, 9190 + curve)
    ld = p2e._ld(cols)
    aux, _e, abad = prog.aux_witness_batch(inputs, cols, n=n, ld=ld)
    aux32, _e, cabad = prog.aux_witness_compact_batch(inputs, narrow, n=n)
    k = prog.num_ux_cols
    big = torch.full((k, n + 7), -1, dtype=torch.int32, device="cuda")
    ux32, e32, b32 = prog.msm_ux_witness_batch(inputs, cols, aux, n=n, ld=ld, ux=big[:, :n])
    ux64, e64, b64 = prog.msm_ux_witness_batch(inputs, cols, aux, n=n, ld=ld, u32=False)
    c32, ce32, cb32 = prog.ux_witness_compact_batch(inputs, narrow, aux32, n=n)
    torch.cuda.synchronize()
    assert abad == cabad == b32 == b64 == cb32 == 0 and not e32.any() and not e64.any() and not ce32.any()
    assert bool((big[:, n:] == -1).all())
    assert torch.equal(c32, ux32) and torch.equal(ux64, ux32.to(torch.int64))
    assert sum(nc for _first, nc in prog.ux_describe()) == k
    exp = UX.curve_program(p2e.CP_MSM, curve, None, host)
    dexp, blocks = UX.to_device(torch, exp), UX.layout("curve", p2e.CP_MSM, curve)["blocks"]
    assert not exp["err"].any() and [tuple(b) for b in prog.ux_describe()] == blocks
    UX.assert_same_device(torch, "p2e_curve_msm_ux_witness_batch, u32", ux32, dexp["ux32"], dexp, blocks)
    UX.assert_same_device(torch, "p2e_curve_msm_ux_witness_batch, u64", ux64, dexp["ux32"], dexp, blocks)
    UX.assert_same_device(torch, "compact container, u32", c32, dexp["ux32"], dexp, blocks)
    h_cols, h_aux, h_ux = _u64(cols), _u64(aux), _u32(ux32)
    for i in REPLAYED:
        c = _curve_replay(p2e, p2e.CP_MSM, curve, point, host, i, h_cols[:, i], h_aux[:, i])
        assert len(c.ux) == k and np.array_equal(h_ux[:, i].astype(np.uint64), np.asarray(c.ux, np.uint64)), i
    with pytest.raises(p2e.P2EError) as e:                  # the entry point without a slot for q still refuses the program
        prog.ux_witness_batch(inputs, cols, aux, n=n, ld=ld)
    assert "no slot for q" in str(e.value) and "p2e_curve_msm_ux_witness_batch" in str(e.value)
    with pytest.raises(p2e.P2EError):                       # ... and the compact pass refuses an MSM call without q
        prog.ux_witness_compact_batch((inputs[4], inputs[5], None, inputs[0], inputs[1]), narrow, aux32, n=n)
    prog.close()


# ---- misuse with real handles ------------------------------------------------------------------------------------------------
def test_every_stride_below_n_is_refused(gpu):
    """each of the seven entry points, each ld_* (and the wire stride) below n in turn, with a real context, curve program
    and wire map: P2E_E_INVALID with a text, before anything is read (the matrices are small dummies)"""
    import ctypes as C
    p2e, torch, ctx = gpu
    L, n = ctx._L, 8
    prog = p2e.CurveProgram(ctx, p2e.CP_MSM, p2e.CURVE_SECP256K1)
    from plonky2_ecdsa_amd.wiremap import WIRE_SRC_AUX, WIRE_SRC_UX, WIRE_SRC_GATE
    col_map, _nn, _nw = p2e.compact_layout(0)
    is_wide = (col_map & p2e.COMPACT_WIDE) != 0
    first_narrow, first_wide = int(np.nonzero(~is_wide)[0][0]), int(np.nonzero(is_wide)[0][0])
    wm = ctx.wire_map(0, np.array([first_narrow, first_wide, WIRE_SRC_AUX | 1, WIRE_SRC_UX | 1, WIRE_SRC_GATE | 1], np.uint32),
                      np.arange(5, dtype=np.uint32), 1, 8)                           # a map that reads all five matrices
    buf = torch.zeros(4096, dtype=torch.int64, device="cuda")
    b, x, z = C.c_void_p(buf.data_ptr()), C.c_size_t(n), C.c_size_t(n - 1)
    c, P, W = ctx._h, prog._h, wm._h
    cases = {
        "p2e_ux_witness_compact_batch": ((c, 0, b, b, b, b, b, b, x, b, x, b, 1, x, x, b), (8, 10, 13)),
        "p2e_gate_internal_compact_batch": ((c, 0, b, x, b, x, x), (3, 5)),
        "p2e_assemble_wires_compact": ((c, W, b, x, b, x, b, x, b, 1, x, b, x, b, x, x), (3, 5, 7, 10, 12, 14)),
        "p2e_curve_program_aux_witness_compact_batch": ((c, P, b, b, b, b, b, b, x, b, x, x, b), (8, 10)),
        "p2e_curve_program_gate_internal_compact_batch": ((c, P, b, x, b, x, x), (3, 5)),
        "p2e_curve_program_ux_witness_compact_batch": ((c, P, b, b, b, b, b, b, b, b, x, b, x, b, 1, x, x, b), (10, 12, 15)),
        "p2e_curve_msm_ux_witness_batch": ((c, P, b, b, b, b, b, b, b, x, b, x, b, 1, x, x, b), (9, 11, 14)),
    }
    for name, (args, positions) in cases.items():
        f = getattr(L, name)
        f.restype = C.c_long
        for pos in positions:
            assert args[pos] is x
            assert f(*(args[:pos] + (z,) + args[pos + 1:])) == -1, (name, pos)      # P2E_E_INVALID
            assert L.p2e_last_error(), (name, pos)
    # an MSM call without q, and one without p, are refused by both forms of its constraint-block pass
    null = C.c_void_p(0)
    a = cases["p2e_curve_program_ux_witness_compact_batch"][0]
    for pos in (5, 6, 7, 8):
        assert L.p2e_curve_program_ux_witness_compact_batch(*(a[:pos] + (null,) + a[pos + 1:])) == -1, pos
    a = cases["p2e_curve_msm_ux_witness_batch"][0]
    for pos in (2, 3, 4, 5):
        assert L.p2e_curve_msm_ux_witness_batch(*(a[:pos] + (null,) + a[pos + 1:])) == -1, pos
    wm.close()
    prog.close()
