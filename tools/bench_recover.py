"""Public-key recovery (include/p2e.h p2e_ecdsa_recover_batch): recoveries per second, with the verdict-only verifier beside it.

For both curves and n = 2^13 and 2^16 per call: signatures made on the device by p2e_ecdsa_sign_recoverable_batch from random
(msg, sk, k), then the median of REPS (default 21) timed recovery calls after WARMUP (3), measured with HIP events on the
caller's stream around the call alone (inputs and outputs stay on the device).  Every point runs ROUNDS (2) times:
`spread` is the relative difference between the repeated medians.  For context, in the same process and at the same
sizes: the verdict-only verifier on the recovered keys (p2e_ecdsa_verify_batch; P-256: p2e_p256_verify_batch).
One JSON line per point; usage: python tools/bench_recover.py [out.jsonl] [log2 n ...]   (default profiles/recover_batch.jsonl)"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import torch
import plonky2_ecdsa_amd as p2e
import p2e_ref

args = sys.argv[1:]
out_path = args.pop(0) if args and not args[0].isdigit() else os.path.join(ROOT, "profiles", "recover_batch.jsonl")
logs = [int(a) for a in args] or [13, 16]
REPS, WARMUP, ROUNDS = int(os.environ.get("REPS", "21")), int(os.environ.get("WARMUP", "3")), int(os.environ.get("ROUNDS", "2"))
box = torch.cuda.get_device_name(0)
ctx = p2e.Context(device=0)


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


with open(out_path, "w") as out:
    for curve, cname in ((p2e.CURVE_SECP256K1, "secp256k1"), (p2e.CURVE_P256, "p256")):
        prog = None
        if curve == p2e.CURVE_P256:
            cv = p2e_ref.P256
            prog = p2e.CurveProgram(ctx, p2e.CP_VERIFY, p2e.CURVE_P256, blind=cv.mul(0xB11D, cv.g))
        for lg in logs:
            n = 1 << lg
            gen = torch.Generator(device="cuda").manual_seed(2000 * curve + lg)
            msg, sk, k = [torch.randint(0, 256, (n, 32), dtype=torch.uint8, device="cuda", generator=gen) for _ in range(3)]
            r, s, v, err, bad = ctx.ecdsa_sign_recoverable_batch(msg, sk, k, curve=curve)
            pkx, pky = torch.empty_like(r), torch.empty_like(r)
            valid = torch.empty(n, dtype=torch.uint8, device="cuda")
            recover = lambda: ctx.ecdsa_recover_batch(msg, r, s, v, curve=curve, pkx=pkx, pky=pky, err=err)
            if prog is None:
                verify = lambda: ctx.ecdsa_verify_batch(msg, r, s, pkx, pky, err=err, valid=valid)
            else:
                verify = lambda: prog.verify_batch(msg, r, s, pkx, pky, err=err, valid=valid)
            med = {"recover": [], "verify": []}
            for _round in range(ROUNDS):
                med["recover"].append(timed(recover))
                med["verify"].append(timed(verify))
            torch.cuda.synchronize()
            rec = {"box": box, "curve": cname, "log2_n": lg, "n": n, "reps": REPS, "flagged_by_signer": int(bad),
                   "all_verify": bool((valid == 1).all())}
            for name in ("recover", "verify"):
                rec[name + "_ms"] = [round(x, 4) for x in med[name]]
                rec[name + "_spread"] = round((max(med[name]) - min(med[name])) / min(med[name]), 4)
                rec[name + "_per_s"] = round(n / (statistics.mean(med[name]) * 1e-3))
            line = json.dumps(rec)
            print(line, flush=True)
            out.write(line + "\n")
            out.flush()
        if prog is not None:
            prog.close()
