"""BIP-340 Schnorr calls (include/p2e.h p2e_schnorr_public_key_batch and the four calls after it): time per call, against the
calls of this library that do comparable work.

The method of MEASUREMENTS.md section 17: inputs are made on the device (random bytes; secret keys with the top byte
cleared and the lowest bit set, so 0 < sk < n), keys and signatures by the calls under test, everything stays on the
device.  A figure is the median of REPS (default 21) timed calls after WARMUP (3), measured with HIP events on the caller's
stream around the call alone; every point runs ROUNDS (2) times and `spread` is the relative difference between the
repeated medians.  One process.  Before anything is timed the two verifying routes are compared on the whole batch: every
valid[i] = 1 and aggregate verdict 1, and after one corrupted signature exactly one valid[i] = 0 and verdict 0.
One JSON line per point, n = 2^12, 2^16, 2^20:
  keys       p2e_schnorr_public_key_batch against p2e_ecdsa_public_key_batch under P2E_SIGN_PLAN_LANE
  sign       p2e_schnorr_sign_batch against p2e_ecdsa_sign_batch under P2E_SIGN_PLAN_LANE
  verify     p2e_schnorr_verify_batch against the SUM of p2e_point_lincomb_batch (P2E_MUL_PLAN_AUTO) and
             p2e_point_decode_batch on the same keys in compressed form: the verifier does the work of those two calls plus
             two SHA-256 compressions; `verify_over_sum` is the ratio, the bar is 1.10
  aggregate  p2e_schnorr_verify_aggregate (P2E_MSM_WINDOW_AUTO) and its ratio to p2e_schnorr_verify_batch
usage: python tools/bench_schnorr.py [out.jsonl]   (default profiles/schnorr.jsonl; appended to)"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import plonky2_ecdsa_amd as p2e

args = sys.argv[1:]
out_path = args.pop(0) if args and args[0].endswith(".jsonl") else os.path.join(ROOT, "profiles", "schnorr.jsonl")
REPS, WARMUP, ROUNDS = int(os.environ.get("REPS", "21")), int(os.environ.get("WARMUP", "3")), int(os.environ.get("ROUNDS", "2"))
SIZES = [int(v) for v in os.environ.get("LOG2_SIZES", "12,16,20").split(",")]
box = torch.cuda.get_device_name(0)
ctx = p2e.Context(device=0)
K1 = p2e.CURVE_SECP256K1


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


def mean(r):
    return statistics.mean(r["ms"])


with open(out_path, "a") as out:
    def emit(rec):
        line = json.dumps(dict({"box": box, "reps": REPS}, **rec))
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    for lg in SIZES:
        n = 1 << lg
        gen = torch.Generator(device="cuda").manual_seed(340 + lg)
        rnd = lambda *shape: torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=gen)
        sk, msg, aux, a32, b32, seed = rnd(n, 32), rnd(n, 32), rnd(n, 32), rnd(n, 32), rnd(n, 32), rnd(32)
        sk[:, 0] = 0           # big-endian: below 2^248
        sk[:, 31] |= 1         # and not zero
        sk_le = sk.flip(1).contiguous()                       # the same keys as the ECDSA calls read them
        pk, err, bad = ctx.schnorr_public_key_batch(sk)
        assert bad == 0
        sig, err, bad = ctx.schnorr_sign_batch(msg, sk, aux)
        assert bad == 0
        px, py, err, bad = ctx.xonly_decode_batch(pk)
        assert bad == 0
        sec1 = torch.cat([torch.full((n, 1), 2, dtype=torch.uint8, device="cuda"), pk], dim=1).contiguous().reshape(-1)
        offsets = torch.arange(n + 1, dtype=torch.int64, device="cuda") * 33
        valid, verdict = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(1, dtype=torch.uint8, device="cuda")
        o1, o2, o3 = torch.empty_like(pk), torch.empty_like(pk), torch.empty_like(sig)
        # the two routes agree on the whole batch, valid and corrupted
        assert ctx.schnorr_verify_batch(msg, pk, sig, err=err, valid=valid)[-1] == 0 and bool((valid == 1).all())
        assert ctx.schnorr_verify_aggregate(msg, pk, sig, seed, verdict=verdict, err=err)[-1] == 0 and int(verdict[0]) == 1
        broken = sig.clone()
        broken[n // 3, 40] ^= 0x10
        assert ctx.schnorr_verify_batch(msg, pk, broken, err=err, valid=valid)[-1] == 0 and int((valid == 0).sum()) == 1 and int(valid[n // 3]) == 0
        assert ctx.schnorr_verify_aggregate(msg, pk, broken, seed, verdict=verdict, err=err)[-1] == 0 and int(verdict[0]) == 0
        dx, dy, derr, bad = ctx.point_decode_batch(sec1, offsets, curve=K1)
        assert bad == 0 and torch.equal(dx, px) and torch.equal(dy, py)          # 02 || x is the even-y lift

        s_keys = rounds(lambda: ctx.schnorr_public_key_batch(sk, pk=o1, err=err))
        e_keys = rounds(lambda: ctx.ecdsa_public_key_batch(sk_le, curve=K1, plan=p2e.SIGN_PLAN_LANE, pkx=o1, pky=o2, err=err))
        emit({"section": "keys", "log2_n": lg, "schnorr_ms": s_keys["ms"], "schnorr_spread": s_keys["spread"], "ecdsa_lane_ms": e_keys["ms"],
              "ecdsa_lane_spread": e_keys["spread"], "schnorr_over_ecdsa": round(mean(s_keys) / mean(e_keys), 4)})
        s_sign = rounds(lambda: ctx.schnorr_sign_batch(msg, sk, aux, sig=o3, err=err))
        e_sign = rounds(lambda: ctx.ecdsa_sign_batch(msg, sk_le, aux, curve=K1, plan=p2e.SIGN_PLAN_LANE, r=o1, s=o2, err=err))
        emit({"section": "sign", "log2_n": lg, "schnorr_ms": s_sign["ms"], "schnorr_spread": s_sign["spread"], "ecdsa_lane_ms": e_sign["ms"],
              "ecdsa_lane_spread": e_sign["spread"], "schnorr_over_ecdsa": round(mean(s_sign) / mean(e_sign), 4)})
        lin = rounds(lambda: ctx.point_lincomb_batch(a32, b32, px, py, curve=K1, plan=p2e.MUL_PLAN_AUTO, outx=o1, outy=o2, err=err))
        dec = rounds(lambda: ctx.point_decode_batch(sec1, offsets, curve=K1, px=o1, py=o2, err=err))
        ver = rounds(lambda: ctx.schnorr_verify_batch(msg, pk, sig, err=err, valid=valid))
        emit({"section": "verify", "log2_n": lg, "verify_ms": ver["ms"], "verify_spread": ver["spread"], "lincomb_ms": lin["ms"],
              "lincomb_spread": lin["spread"], "decode_ms": dec["ms"], "decode_spread": dec["spread"],
              "verify_over_sum": round(mean(ver) / (mean(lin) + mean(dec)), 4), "bar": 1.10})
        agg = rounds(lambda: ctx.schnorr_verify_aggregate(msg, pk, sig, seed, verdict=verdict, err=err))
        emit({"section": "aggregate", "log2_n": lg, "aggregate_ms": agg["ms"], "aggregate_spread": agg["spread"], "verify_ms": ver["ms"],
              "aggregate_over_verify": round(mean(agg) / mean(ver), 4),
              "window_bits": p2e.point_msm_plan(2 * n + 1)["window_bits"]})
