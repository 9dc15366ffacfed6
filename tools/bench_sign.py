"""Batch key derivation and signing (include/p2e.h p2e_ecdsa_public_key_batch / p2e_ecdsa_sign_batch): time per call.

For both curves, both calls and n = 2^10 ... 2^18: the median of REPS (default 21) timed calls after WARMUP (3), per forced
plan and for P2E_SIGN_PLAN_AUTO, measured with HIP events on the caller's stream around the call alone (inputs and outputs
stay on the device).  The whole sweep of a (curve, call, n) point runs ROUNDS (2) times, plans interleaved, so every median
is there twice: `spread` is the relative difference between a plan's repeated medians.  Baseline: the wall time of the
host loop these calls replace, p2e_synth_signatures[_curve] for the same n on the machine's OpenMP threads (it derives the
key AND signs: compare it with the two device calls together, line "floor").
One JSON line per point; usage: python tools/bench_sign.py [out.jsonl] [log2 n ...]   (default profiles/sign_batch.jsonl)"""
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
out_path = args.pop(0) if args and not args[0].isdigit() else os.path.join(ROOT, "profiles", "sign_batch.jsonl")
logs = [int(a) for a in args] or list(range(10, 19))
REPS, WARMUP, ROUNDS = int(os.environ.get("REPS", "21")), int(os.environ.get("WARMUP", "3")), int(os.environ.get("ROUNDS", "2"))
PLANS = (("lane", p2e.SIGN_PLAN_LANE), ("quad", p2e.SIGN_PLAN_QUAD), ("auto", p2e.SIGN_PLAN_AUTO))
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
    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    for curve, cname in ((p2e.CURVE_SECP256K1, "secp256k1"), (p2e.CURVE_P256, "p256")):
        for lg in logs:
            n = 1 << lg
            t0 = time.perf_counter()
            if curve == p2e.CURVE_SECP256K1:
                p2e.synth_signatures(seed=4, n=n)
            else:
                p2e.synth_signatures_curve(curve, seed=4, n=n)
            host_ms = (time.perf_counter() - t0) * 1e3
            gen = torch.Generator(device="cuda").manual_seed(1000 * curve + lg)
            msg, sk, k = [torch.randint(0, 256, (n, 32), dtype=torch.uint8, device="cuda", generator=gen) for _ in range(3)]
            o1, o2 = torch.empty_like(sk), torch.empty_like(sk)
            err = torch.empty(n, dtype=torch.uint8, device="cuda")
            best = {}
            for call in ("public_key", "sign"):
                med = {name: [] for name, _ in PLANS}
                for _round in range(ROUNDS):
                    for name, plan in PLANS:
                        if call == "public_key":
                            fn = lambda: ctx.ecdsa_public_key_batch(sk, curve=curve, plan=plan, pkx=o1, pky=o2, err=err)
                        else:
                            fn = lambda: ctx.ecdsa_sign_batch(msg, sk, k, curve=curve, plan=plan, r=o1, s=o2, err=err)
                        med[name].append(timed(fn))
                rec = {"box": box, "curve": cname, "call": call, "log2_n": lg, "n": n, "reps": REPS, "host_synth_ms": round(host_ms, 3),
                       "host_threads": os.cpu_count() if not os.environ.get("OMP_NUM_THREADS") else int(os.environ["OMP_NUM_THREADS"])}
                for name, _ in PLANS:
                    rec[name + "_ms"] = [round(v, 4) for v in med[name]]
                    rec[name + "_spread"] = round((max(med[name]) - min(med[name])) / min(med[name]), 4)
                faster = "lane" if min(med["lane"]) <= min(med["quad"]) else "quad"
                rec["faster_forced_plan"] = faster
                rec["auto_over_faster"] = round(statistics.mean(med["auto"]) / statistics.mean(med[faster]), 4)
                rec["per_s_auto"] = round(n / (statistics.mean(med["auto"]) * 1e-3))
                best[call] = statistics.mean(med["auto"])
                emit(rec)
            emit({"box": box, "curve": cname, "call": "floor", "log2_n": lg, "n": n, "host_synth_ms": round(host_ms, 3),
                  "device_public_key_plus_sign_ms": round(best["public_key"] + best["sign"], 4),
                  "host_over_device": round(host_ms / (best["public_key"] + best["sign"]), 1)})
