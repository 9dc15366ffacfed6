"""Point tables (include/p2e.h p2e_point_table_create and the three calls that walk a table): time per call, against the
general calls they replace for known points.

Table points are public keys made on the device by p2e_ecdsa_public_key_batch from random secret keys, scalars are random
bytes, signatures are made on the device by p2e_ecdsa_sign_batch under the table's keys; inputs and outputs stay on the
device.  A figure is the median of REPS (default 21) timed calls after WARMUP (3), measured with HIP events on the caller's
stream around the call alone; every point runs ROUNDS (2) times and `spread` is the relative difference between the
repeated medians.  Sections (one JSON line per point, both curves, n = 2^16 and 2^20):
  general  p2e_point_mul_batch and p2e_point_lincomb_batch under P2E_MUL_PLAN_AUTO on the points the table holds (element i:
           point idx_i), and the verdict-only verifier (secp256k1: p2e_ecdsa_verify_batch) on the same signatures
  table    the three table calls at m = 1 (idx = NULL) and m = 1024 (uniformly random idx), with the ratio to the general
           call of the same section run just before it in the same process
  create   p2e_point_table_create at m = 1 and m = 1024 (wall time of the synchronous call)
usage: python tools/bench_table.py [out.jsonl] [section ...]   (default profiles/point_table.jsonl, all sections)
The output file is appended to, so that the sections can run as one process each, every one under its own time limit."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import plonky2_ecdsa_amd as p2e

args = sys.argv[1:]
out_path = args.pop(0) if args and args[0].endswith(".jsonl") else os.path.join(ROOT, "profiles", "point_table.jsonl")
sections = args or ["table", "create"]
REPS, WARMUP, ROUNDS = int(os.environ.get("REPS", "21")), int(os.environ.get("WARMUP", "3")), int(os.environ.get("ROUNDS", "2"))
SIZES = [int(v) for v in os.environ.get("LOG2_SIZES", "16,20").split(",")]
TABLE_SIZES = [int(v) for v in os.environ.get("TABLE_SIZES", "1,1024").split(",")]
box = torch.cuda.get_device_name(0)
ctx = p2e.Context(device=0)
CURVES = ((p2e.CURVE_SECP256K1, "secp256k1"), (p2e.CURVE_P256, "p256"))


def timed(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def rounds(fn):
    med = [timed(fn) for _ in range(ROUNDS)]
    return {"ms": [round(x, 4) for x in med], "spread": round((max(med) - min(med)) / min(med), 4)}


def keys(curve, m):
    gen = torch.Generator(device="cuda").manual_seed(7000 + curve)
    sk = torch.randint(0, 256, (m, 32), dtype=torch.uint8, device="cuda", generator=gen)
    px, py, _err, bad = ctx.ecdsa_public_key_batch(sk, curve=curve)
    assert bad == 0
    return sk, px, py


def setup(curve, m, lg):
    """the table of m keys and, for 2^lg elements: idx (None at m = 1), scalars a, b, the elements' points, signatures"""
    n = 1 << lg
    sk, px, py = keys(curve, m)
    table = ctx.point_table(px, py, curve=curve)
    gen = torch.Generator(device="cuda").manual_seed(8000 + curve)
    a, b, nonce = [torch.randint(0, 256, (n, 32), dtype=torch.uint8, device="cuda", generator=gen) for _ in range(3)]
    j = torch.randint(0, m, (n,), dtype=torch.int64, device="cuda", generator=gen)
    idx = None if m == 1 else j.to(torch.int32)
    ex, ey = px[j].contiguous(), py[j].contiguous()
    r, s, _err, bad = ctx.ecdsa_sign_batch(a, sk[j].contiguous(), nonce, curve=curve)          # msg = a
    assert bad == 0
    return table, idx, a, b, ex, ey, r, s


def calls(curve, m, lg):
    """{name: (general call or None, table call)} on the same elements"""
    table, idx, a, b, ex, ey, r, s = setup(curve, m, lg)
    n = 1 << lg
    ox, oy = torch.empty_like(ex), torch.empty_like(ex)
    err, valid = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
    out = {
        "mul": (lambda: ctx.point_mul_batch(b, ex, ey, curve=curve, plan=p2e.MUL_PLAN_AUTO, outx=ox, outy=oy, err=err),
                lambda: ctx.point_table_mul_batch(table, b, idx=idx, outx=ox, outy=oy, err=err)),
        "lincomb": (lambda: ctx.point_lincomb_batch(a, b, ex, ey, curve=curve, plan=p2e.MUL_PLAN_AUTO, outx=ox, outy=oy, err=err),
                    lambda: ctx.point_table_lincomb_batch(table, a, b, idx=idx, outx=ox, outy=oy, err=err)),
        "verify": ((lambda: ctx.ecdsa_verify_batch(a, r, s, ex, ey, err=err, valid=valid)) if curve == p2e.CURVE_SECP256K1 else None,
                   lambda: ctx.ecdsa_verify_table_batch(table, a, r, s, idx=idx, err=err, valid=valid)),
    }
    for name, (general, tab) in out.items():                 # the two routes agree before anything is timed
        assert tab()[-1] == 0
        got = [t.clone() for t in ((valid,) if name == "verify" else (ox, oy))]
        if name == "verify":
            assert bool(valid.all())
        if general is not None:
            assert general()[-1] == 0 and all(torch.equal(g, w) for g, w in zip(got, (valid,) if name == "verify" else (ox, oy)))
    return table, out


with open(out_path, "a") as out:
    def emit(rec):
        line = json.dumps(dict({"box": box, "reps": REPS}, **rec))
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    for curve, cname in CURVES:
        if "general" in sections or "table" in sections:
            for lg in SIZES:
                for m in TABLE_SIZES:
                    table, fns = calls(curve, m, lg)
                    for name, (general, tab) in fns.items():
                        rec = {"section": "table", "curve": cname, "log2_n": lg, "m": m, "call": name}
                        if general is not None:
                            g = rounds(general)
                            rec.update({"general_ms": g["ms"], "general_spread": g["spread"]})
                        if "table" in sections:
                            t = rounds(tab)
                            rec.update({"table_ms": t["ms"], "table_spread": t["spread"]})
                            if general is not None:
                                rec["table_over_general"] = round(statistics.mean(t["ms"]) / statistics.mean(g["ms"]), 4)
                        emit(rec)
                    table.close()
        if "create" in sections:
            for m in TABLE_SIZES:
                _sk, px, py = keys(curve, m)
                ms = []
                for _ in range(WARMUP + REPS):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    t = ctx.point_table(px, py, curve=curve)
                    ms.append((time.perf_counter() - t0) * 1e3)
                    t.close()
                emit({"section": "create", "curve": cname, "m": m, "table_bytes": m * p2e.POINT_TABLE_BYTES_PER_POINT,
                      "ms": round(statistics.median(ms[WARMUP:]), 4)})
