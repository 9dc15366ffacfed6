"""Streaming passes beyond the fill: built-in-generator columns (k_aux), gate-internal values (k_gate), constraint-block
columns (k_ux, u32 and u64 output) and the wire-matrix assembly (k_assemble, chunk of signatures), each from the u64
matrices and from the compact container (u32 narrow + u64 wide matrices, u32 aux matrix) IN THE SAME PROCESS, the two
sources alternating repeat by repeat; then fill + aux + ux end to end from each container.  Built-in verify program at
batch 2^K (default 16), P-256 verifier program at 2^KC (default 14; KC=0 skips it).  Per leg: median, min and max of REPS
(default 7) timed calls in ms (host clock around a call that ends in a device synchronise), algorithmic GB/s written.
One JSON line per program."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import plonky2_ecdsa_amd as p2e
from plonky2_ecdsa_amd.wiremap import synthetic_wire_map
K = int(os.environ.get("K", 16)); KC = int(os.environ.get("KC", 14)); REPS = int(os.environ.get("REPS", 7))
ctx = p2e.Context(device=0)


def timed_pair(fa, fb, reps=REPS):
    """two variants of one job, alternating: {ms_median, ms_min, ms_max} each"""
    for f in (fa, fb):
        f(); torch.cuda.synchronize()
    ts = ([], [])
    for _ in range(reps):
        for k, f in enumerate((fa, fb)):
            t = time.perf_counter(); f(); torch.cuda.synchronize(); ts[k].append((time.perf_counter() - t) * 1e3)
    return [{"ms": round(sorted(t)[len(t) // 2], 3), "ms_min": round(min(t), 3), "ms_max": round(max(t), 3)} for t in ts]


def leg(out, name, fa, fb, bytes_a=None, bytes_b=None):
    """bytes_a / bytes_b: bytes the u64-source / compact-source variant writes (bytes_b defaults to bytes_a)"""
    a, b = timed_pair(fa, fb)
    for r, nbytes in ((a, bytes_a), (b, bytes_b if bytes_b is not None else bytes_a)):
        if nbytes is not None:
            r["GBps_written"] = round(nbytes / r["ms"] / 1e6, 1)
    out[name] = {"u64_source": a, "compact_source": b, "compact_over_u64": round(b["ms"] / a["ms"], 3)}


def pad(n):
    return n + 16 if (n >= 4096 and n & (n - 1) == 0) else n   # (a power-of-two column stride camps on the same HBM channels)


def mat(rows, n, dtype):
    return torch.empty((rows, pad(n)), dtype=dtype, device="cuda")[:, :n]


def passes(out, n, fill, cfill, aux_u64, aux_c, gate_u64, gate_c, ux_u64src, ux_csrc, num_aux, num_gate, num_ux):
    """the legs of one program; *_u64 / *_c: callables of the two sources writing into the given output matrix"""
    cols, narrow, wide = fill()[0], *cfill()[:2]
    aux, aux32 = mat(num_aux, n, torch.int64), mat(num_aux, n, torch.int32)
    leg(out, "aux", lambda: aux_u64(cols, aux), lambda: aux_c(narrow, aux32), num_aux * n * 8, num_aux * n * 4)
    assert torch.equal(aux32.to(torch.int64), aux)
    if num_gate:
        g1, g2 = mat(num_gate, n, torch.int64), mat(num_gate, n, torch.int64)
        leg(out, "gate_internal", lambda: gate_u64(aux, g1), lambda: gate_c(aux32, g2), num_gate * n * 8)
        assert torch.equal(g1, g2)
        del g1, g2
        torch.cuda.empty_cache()
    keep = None
    for u32 in (False, True):                          # (the u64 output first: it is the largest allocation)
        dt = torch.int32 if u32 else torch.int64
        u1 = mat(num_ux, n, dt)
        u2 = mat(num_ux, n, dt) if u32 or n <= 1 << 14 else u1     # 2^16, u64 output: 131 GB, one buffer for both
        leg(out, "ux_u32_out" if u32 else "ux_u64_out", lambda: ux_u64src(cols, aux, u1), lambda: ux_csrc(narrow, aux32, u2),
            num_ux * n * (4 if u32 else 8))
        if u2 is not u1:
            assert torch.equal(u1, u2)
        keep = u1
        del u2
        if not u32:
            del u1, keep
            torch.cuda.empty_cache()
    assert int((keep >> 29).ne(0).sum()) == 0          # every U29 value in range, whole batch
    # end to end: fill + aux + ux (u32 output) from each container
    leg(out, "fill_aux_ux_u32", lambda: (fill(), aux_u64(cols, aux), ux_u64src(cols, aux, keep)),
        lambda: (cfill(), aux_c(narrow, aux32), ux_csrc(narrow, aux32, keep)))
    leg(out, "fill", fill, cfill)
    return cols, narrow, wide, aux, aux32, keep


# ---- built-in verify program ------------------------------------------------------------------------------------------------
n = 1 << K
dev = [torch.from_numpy(a).cuda() for a in p2e.synth_signatures(seed=4, n=n)]
out = {"program": "verify_secp256k1", "n": n, "reps": REPS}
cols, narrow, wide, aux, aux32, ux = passes(
    out, n,
    lambda: ctx.ecdsa_verify_witness_batch(*dev), lambda: ctx.ecdsa_verify_witness_compact_batch(*dev),
    lambda c, a: ctx.aux_witness_batch(0, dev[4], c, aux=a), lambda nar, a: ctx.aux_witness_compact_batch(0, dev[4], nar, aux32=a),
    lambda a, g: ctx.gate_internal_batch(0, a, gate=g), lambda a, g: ctx.gate_internal_compact_batch(0, a, gate=g),
    lambda c, a, u: ctx.ux_witness_batch(0, dev, c, a, ux=u), lambda nar, a, u: ctx.ux_witness_compact_batch(0, dev, nar, a, ux=u),
    p2e.VERIFY_AUX_COLS, p2e.VERIFY_GATE_COLS, p2e.VERIFY_UX_COLS)
src, dst, nw, deg = synthetic_wire_map(0)
wm = ctx.wire_map(0, src, dst, nw, deg)
chunk = min(n, 2048)
w1 = torch.zeros((chunk, nw * deg), dtype=torch.int64, device="cuda")
w2 = torch.zeros((chunk, nw * deg), dtype=torch.int64, device="cuda")
leg(out, "assemble", lambda: ctx.assemble_wires(wm, cols[:, :chunk], aux[:, :chunk], ux[:, :chunk], wires=w1, n=chunk),
    lambda: ctx.assemble_wires_compact(wm, narrow[:, :chunk], wide[:, :chunk], aux32[:, :chunk], ux[:, :chunk], wires=w2, n=chunk),
    len(src) * chunk * 8)
assert torch.equal(w1, w2)
out["assemble"].update({"signatures": chunk, "entries": len(src)})
print(json.dumps(out), flush=True)
del cols, narrow, wide, aux, aux32, ux, w1, w2
torch.cuda.empty_cache()

# ---- P-256 verifier program -----------------------------------------------------------------------------------------------------
if KC:
    n = 1 << KC
    sig = p2e.synth_signatures_curve(p2e.CURVE_P256, seed=4, n=n)
    bsig = p2e.synth_signatures_curve(p2e.CURVE_P256, seed=99, n=1)     # a public key serves as the blinding point
    blind = (int.from_bytes(bytes(bsig[3][0]), "little"), int.from_bytes(bytes(bsig[4][0]), "little"))
    prog = p2e.CurveProgram(ctx, p2e.CP_VERIFY, p2e.CURVE_P256, blind)
    dev = tuple(torch.from_numpy(a).cuda() for a in sig)
    out = {"program": "verify_p256", "n": n, "reps": REPS}
    passes(out, n,
           lambda: prog.verify_witness_batch(*dev), lambda: prog.verify_witness_compact_batch(*dev),
           lambda c, a: prog.aux_witness_batch(dev, c, aux=a), lambda nar, a: prog.aux_witness_compact_batch(dev, nar, aux32=a),
           lambda a, g: prog.gate_internal_batch(a, gate=g), lambda a, g: prog.gate_internal_compact_batch(a, gate=g),
           lambda c, a, u: prog.ux_witness_batch(dev, c, a, ux=u, u32=u.element_size() == 4),
           lambda nar, a, u: prog.ux_witness_compact_batch(dev, nar, a, ux=u),
           prog.num_aux_cols, prog.num_gate_cols, prog.num_ux_cols)
    print(json.dumps(out), flush=True)
    prog.close()
