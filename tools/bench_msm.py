"""The bucket-method multi-scalar multiplication (include/p2e.h p2e_point_msm): time per call.

Points are public keys made on the device by p2e_ecdsa_public_key_batch from random secret keys, scalars are random bytes;
inputs and outputs stay on the device.  A figure is the median of REPS (default 21) timed calls after WARMUP (3), measured
with HIP events on the caller's stream around the call alone; every point runs ROUNDS (2) times and `spread` is the
relative difference between the repeated medians.  Sections (one JSON line per point, both curves):
  auto    P2E_MSM_WINDOW_AUTO at n = 2^12 .. 2^20
  widths  every forced width at n = 2^16 and 2^20 (what the AUTO rule is derived from)
  tail    the n-independent part (bucket reduction, window combination, inversion): the call at n = 1 for every width, which
          runs the same reduction, combination and inversion launches on empty buckets
  equal   all scalars equal against uniform scalars at 2^20
  bar     p2e_ecdsa_recover_batch on 2^20 elements against p2e_point_msm on 2^20 points, same process
usage: python tools/bench_msm.py [out.jsonl] [section ...]   (default profiles/point_msm.jsonl, all sections)
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
out_path = args.pop(0) if args and args[0].endswith(".jsonl") else os.path.join(ROOT, "profiles", "point_msm.jsonl")
sections = args or ["auto", "widths", "tail", "equal", "bar"]
REPS, WARMUP, ROUNDS = int(os.environ.get("REPS", "21")), int(os.environ.get("WARMUP", "3")), int(os.environ.get("ROUNDS", "2"))
BIG = int(os.environ.get("LOG2_BIG", "20"))
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


_inputs = {}


def inputs(curve, lg):
    """(k, pkx, pky) of 2^lg points on the device; made once per curve at the largest size and sliced"""
    if curve not in _inputs:
        n = 1 << max(BIG, 16)
        gen = torch.Generator(device="cuda").manual_seed(3000 + curve)
        sk, k = [torch.randint(0, 256, (n, 32), dtype=torch.uint8, device="cuda", generator=gen) for _ in range(2)]
        pkx, pky, _err, bad = ctx.ecdsa_public_key_batch(sk, curve=curve)
        assert bad == 0
        _inputs[curve] = (k, pkx, pky)
    return [t[:1 << lg] for t in _inputs[curve]]


def msm_call(curve, k, pkx, pky, width):
    n = k.shape[0]
    outx, outy = [torch.empty(32, dtype=torch.uint8, device="cuda") for _ in range(2)]
    status = torch.empty(1, dtype=torch.uint8, device="cuda")
    perr = torch.empty(n, dtype=torch.uint8, device="cuda")
    fn = lambda: ctx.point_msm(k, pkx, pky, curve=curve, window_bits=width, outx=outx, outy=outy, status=status, point_err=perr)
    fn()
    assert int(status.cpu()[0]) == p2e.MSM_OK
    return fn


with open(out_path, "a") as out:
    def emit(rec):
        line = json.dumps(dict({"box": box, "reps": REPS}, **rec))
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    for curve, cname in CURVES:
        if "auto" in sections:
            for lg in range(12, BIG + 1, 2):
                k, pkx, pky = inputs(curve, lg)
                plan = p2e.point_msm_plan(1 << lg, curve)
                emit(dict({"section": "auto", "curve": cname, "log2_n": lg, "window_bits": plan["window_bits"], "seg": plan["seg"]},
                          **rounds(msm_call(curve, k, pkx, pky, p2e.MSM_WINDOW_AUTO))))
        if "widths" in sections:
            for lg in (16, BIG):
                k, pkx, pky = inputs(curve, lg)
                for width in range(p2e.MSM_WINDOW_MIN, p2e.MSM_WINDOW_MAX + 1):
                    emit(dict({"section": "widths", "curve": cname, "log2_n": lg, "window_bits": width},
                              **rounds(msm_call(curve, k, pkx, pky, width))))
        if "tail" in sections:
            k, pkx, pky = [t[:1] for t in inputs(curve, 16)]
            for width in range(p2e.MSM_WINDOW_MIN, p2e.MSM_WINDOW_MAX + 1):
                emit(dict({"section": "tail", "curve": cname, "n": 1, "window_bits": width}, **rounds(msm_call(curve, k, pkx, pky, width))))
        if "equal" in sections:
            k, pkx, pky = inputs(curve, BIG)
            same = k[:1].expand(k.shape[0], 32).contiguous()
            emit(dict({"section": "equal", "curve": cname, "log2_n": BIG, "scalars": "uniform"}, **rounds(msm_call(curve, k, pkx, pky, 0))))
            emit(dict({"section": "equal", "curve": cname, "log2_n": BIG, "scalars": "all_equal"}, **rounds(msm_call(curve, same, pkx, pky, 0))))
        if "bar" in sections:
            n = 1 << BIG
            k, pkx, pky = inputs(curve, BIG)
            gen = torch.Generator(device="cuda").manual_seed(4000 + curve)
            msg, sk, nonce = [torch.randint(0, 256, (n, 32), dtype=torch.uint8, device="cuda", generator=gen) for _ in range(3)]
            r, s, v, err, _bad = ctx.ecdsa_sign_recoverable_batch(msg, sk, nonce, curve=curve)
            rx, ry = torch.empty_like(r), torch.empty_like(r)
            rec = rounds(lambda: ctx.ecdsa_recover_batch(msg, r, s, v, curve=curve, pkx=rx, pky=ry, err=err))
            msm = rounds(msm_call(curve, k, pkx, pky, p2e.MSM_WINDOW_AUTO))
            ratio = statistics.mean(msm["ms"]) / statistics.mean(rec["ms"])
            emit({"section": "bar", "curve": cname, "log2_n": BIG, "recover_ms": rec["ms"], "recover_spread": rec["spread"],
                  "msm_ms": msm["ms"], "msm_spread": msm["spread"], "msm_over_recover": round(ratio, 4), "msm_faster": ratio < 1.0})
