"""Per-element point arithmetic (include/p2e.h p2e_point_mul_batch, p2e_point_lincomb_batch, p2e_point_add_batch): time per call.

Points are public keys made on the device by p2e_ecdsa_public_key_batch from random secret keys, scalars are random bytes;
inputs and outputs stay on the device.  A figure is the median of REPS (default 21) timed calls after WARMUP (3), measured
with HIP events on the caller's stream around the call alone; every point runs ROUNDS (2) times and `spread` is the
relative difference between the repeated medians.  Sections (one JSON line per point, both curves):
  calls   the three calls under every plan at n = 2^12, 2^16 and 2^20
  bar     p2e_point_mul_batch (PLAIN) against p2e_ecdsa_recover_batch on the same n, same process, at 2^16 and 2^20: the
          multiplication does strictly less per element, so it must be faster by more than the larger of the two spreads
  glv     on secp256k1, GLV against PLAIN at every size: what P2E_MUL_PLAN_AUTO is decided from
usage: python tools/bench_point.py [out.jsonl] [section ...]   (default profiles/point_arith.jsonl, all sections)
The output file is appended to, so that the sections can run as one process each, every one under its own time limit."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import plonky2_ecdsa_amd as p2e

args = sys.argv[1:]
out_path = args.pop(0) if args and args[0].endswith(".jsonl") else os.path.join(ROOT, "profiles", "point_arith.jsonl")
sections = args or ["calls", "bar", "glv"]
REPS, WARMUP, ROUNDS = int(os.environ.get("REPS", "21")), int(os.environ.get("WARMUP", "3")), int(os.environ.get("ROUNDS", "2"))
SIZES = [int(v) for v in os.environ.get("LOG2_SIZES", "12,16,20").split(",")]
box = torch.cuda.get_device_name(0)
ctx = p2e.Context(device=0)
CURVES = ((p2e.CURVE_SECP256K1, "secp256k1", (("plain", p2e.MUL_PLAN_PLAIN), ("glv", p2e.MUL_PLAN_GLV), ("auto", p2e.MUL_PLAN_AUTO))),
          (p2e.CURVE_P256, "p256", (("plain", p2e.MUL_PLAN_PLAIN), ("auto", p2e.MUL_PLAN_AUTO))))


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


_inputs = {}


def inputs(curve, lg):
    """(a, b, px, py, qx, qy) of 2^lg elements on the device; made once per curve at the largest size and sliced"""
    if curve not in _inputs:
        n = 1 << max(SIZES)
        gen = torch.Generator(device="cuda").manual_seed(5000 + curve)
        sk, sk2, a, b = [torch.randint(0, 256, (n, 32), dtype=torch.uint8, device="cuda", generator=gen) for _ in range(4)]
        px, py, _err, bad = ctx.ecdsa_public_key_batch(sk, curve=curve)
        qx, qy, _err, bad2 = ctx.ecdsa_public_key_batch(sk2, curve=curve)
        assert bad == 0 and bad2 == 0
        _inputs[curve] = (a, b, px, py, qx, qy)
    return [t[:1 << lg] for t in _inputs[curve]]


def point_call(curve, op, plan, lg):
    a, b, px, py, qx, qy = inputs(curve, lg)
    ox, oy = torch.empty_like(px), torch.empty_like(px)
    err = torch.empty(px.shape[0], dtype=torch.uint8, device="cuda")
    if op == "mul":
        fn = lambda: ctx.point_mul_batch(b, px, py, curve=curve, plan=plan, outx=ox, outy=oy, err=err)
    elif op == "lincomb":
        fn = lambda: ctx.point_lincomb_batch(a, b, px, py, curve=curve, plan=plan, outx=ox, outy=oy, err=err)
    else:
        fn = lambda: ctx.point_add_batch(px, py, qx, qy, curve=curve, outx=ox, outy=oy, err=err)
    assert fn()[3] == 0
    return fn


def recover_call(curve, lg):
    n = 1 << lg
    gen = torch.Generator(device="cuda").manual_seed(6000 + curve)
    msg, sk, nonce = [torch.randint(0, 256, (n, 32), dtype=torch.uint8, device="cuda", generator=gen) for _ in range(3)]
    r, s, v, err, _bad = ctx.ecdsa_sign_recoverable_batch(msg, sk, nonce, curve=curve)
    rx, ry = torch.empty_like(r), torch.empty_like(r)
    return lambda: ctx.ecdsa_recover_batch(msg, r, s, v, curve=curve, pkx=rx, pky=ry, err=err)


with open(out_path, "a") as out:
    def emit(rec):
        line = json.dumps(dict({"box": box, "reps": REPS}, **rec))
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    for curve, cname, plans in CURVES:
        for lg in SIZES:
            if "calls" in sections:
                for op in ("mul", "lincomb"):
                    for pname, plan in plans:
                        emit(dict({"section": "calls", "curve": cname, "log2_n": lg, "call": op, "plan": pname},
                                  **rounds(point_call(curve, op, plan, lg))))
                emit(dict({"section": "calls", "curve": cname, "log2_n": lg, "call": "add", "plan": "-"}, **rounds(point_call(curve, "add", 0, lg))))
            if "bar" in sections and lg >= 16:
                rec = rounds(recover_call(curve, lg))
                mul = rounds(point_call(curve, "mul", p2e.MUL_PLAN_PLAIN, lg))
                ratio = statistics.mean(mul["ms"]) / statistics.mean(rec["ms"])
                margin = max(rec["spread"], mul["spread"])
                emit({"section": "bar", "curve": cname, "log2_n": lg, "recover_ms": rec["ms"], "recover_spread": rec["spread"],
                      "mul_plain_ms": mul["ms"], "mul_plain_spread": mul["spread"], "mul_over_recover": round(ratio, 4),
                      "mul_faster_by_more_than_spread": ratio < 1.0 - margin})
            if "glv" in sections and curve == p2e.CURVE_SECP256K1:
                plain = rounds(point_call(curve, "mul", p2e.MUL_PLAN_PLAIN, lg))
                glv = rounds(point_call(curve, "mul", p2e.MUL_PLAN_GLV, lg))
                ratio = statistics.mean(glv["ms"]) / statistics.mean(plain["ms"])
                margin = max(plain["spread"], glv["spread"])
                emit({"section": "glv", "curve": cname, "log2_n": lg, "plain_ms": plain["ms"], "plain_spread": plain["spread"],
                      "glv_ms": glv["ms"], "glv_spread": glv["spread"], "glv_over_plain": round(ratio, 4),
                      "glv_faster_by_more_than_spread": ratio < 1.0 - margin})
