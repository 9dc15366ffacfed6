"""a P + b Q and DLEQ proofs (include/p2e.h p2e_point_lincomb2_batch, p2e_dleq_prove_batch, p2e_dleq_verify_batch): time per call,
against the calls of this library that do the same curve work on the same elements.

The method of MEASUREMENTS.md section 17, as tools/bench_sp.py applies it: inputs are made on the device (random bytes; secret
keys and scalars with the top byte cleared and the lowest bit set, so 0 < value < n; points are public keys of such values),
everything stays on the device.  A figure is the median of REPS (default 21) timed calls after WARMUP (3), measured with HIP
events on the caller's stream around the call alone; every point runs ROUNDS (2) times and `spread` is the relative difference
between the repeated medians.  One process.  Before anything is timed the new calls are checked on the whole batch: a P + b Q
equals the bytes of mul, mul, add under every plan, and every fresh proof verifies.
One JSON line per point, n = 2^12, 2^16, 2^20 elements:
  lincomb2   p2e_point_lincomb2_batch against p2e_point_mul_batch + p2e_point_mul_batch + p2e_point_add_batch with the same plan:
             secp256k1 under P2E_MUL_PLAN_PLAIN and P2E_MUL_PLAN_GLV (AUTO is GLV), P-256 under P2E_MUL_PLAN_PLAIN:
             `lincomb2_over_three_calls`; `yardstick_spread` is the largest spread of the three calls
  verify     p2e_dleq_verify_batch against p2e_point_lincomb_batch + p2e_point_mul_batch + p2e_point_mul_batch +
             p2e_point_add_batch (s G - e A; s B, -e C and their sum): `verify_over_four_calls`
  prove      p2e_dleq_prove_batch against p2e_ecdsa_public_key_batch x 2 (a G, k G) + p2e_point_mul_batch x 2 (a B, k B):
             `prove_over_four_calls`
usage: python tools/bench_dleq.py [out.jsonl]   (default profiles/dleq.jsonl; appended to)"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import plonky2_ecdsa_amd as p2e

args = sys.argv[1:]
out_path = args.pop(0) if args and args[0].endswith(".jsonl") else os.path.join(ROOT, "profiles", "dleq.jsonl")
REPS, WARMUP, ROUNDS = int(os.environ.get("REPS", "21")), int(os.environ.get("WARMUP", "3")), int(os.environ.get("ROUNDS", "2"))
SIZES = [int(v) for v in os.environ.get("LOG2_SIZES", "12,16,20").split(",")]
box = torch.cuda.get_device_name(0)
ctx = p2e.Context(device=0)
K1, P256 = p2e.CURVE_SECP256K1, p2e.CURVE_P256
PLAN_NAMES = {p2e.MUL_PLAN_PLAIN: "plain", p2e.MUL_PLAN_GLV: "glv"}


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


def rate(n, r):
    return round(n / (mean(r) * 1e-3))


with open(out_path, "a") as out:
    def emit(rec):
        line = json.dumps(dict({"box": box, "reps": REPS}, **rec))
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    for lg in SIZES:
        n = 1 << lg
        gen = torch.Generator(device="cuda").manual_seed(374 + lg)
        rnd = lambda *shape: torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=gen)

        def secret(*shape):                 # little-endian, 0 < value < 2^248
            v = rnd(*shape, 32)
            v[..., 31] = 0
            v[..., 0] |= 1
            return v
        buf = lambda w=32: torch.empty((n, w), dtype=torch.uint8, device="cuda")
        err = torch.empty(n, dtype=torch.uint8, device="cuda")
        o1, o2, o3, o4, o5, o6 = (buf() for _ in range(6))
        a, b = secret(n), secret(n)

        # ---- a P + b Q ------------------------------------------------------------------------------------------------------
        for curve, cname, plans in ((K1, "secp256k1", (p2e.MUL_PLAN_PLAIN, p2e.MUL_PLAN_GLV)), (P256, "p256", (p2e.MUL_PLAN_PLAIN,))):
            px, py, _e, bad1 = ctx.ecdsa_public_key_batch(secret(n), curve=curve)
            qx, qy, _e, bad2 = ctx.ecdsa_public_key_batch(secret(n), curve=curve)
            assert bad1 == 0 and bad2 == 0
            for plan in plans:
                def three():
                    ctx.point_mul_batch(a, px, py, curve=curve, plan=plan, outx=o1, outy=o2, err=err)
                    ctx.point_mul_batch(b, qx, qy, curve=curve, plan=plan, outx=o3, outy=o4, err=err)
                    return ctx.point_add_batch(o1, o2, o3, o4, curve=curve, outx=o5, outy=o6, err=err)
                assert three()[3] == 0
                wx, wy = o5.clone(), o6.clone()
                gx, gy, _e, bad = ctx.point_lincomb2_batch(a, b, px, py, qx, qy, curve=curve, plan=plan, outx=o5, outy=o6, err=err)
                assert bad == 0 and torch.equal(gx, wx) and torch.equal(gy, wy), "a P + b Q differs from mul, mul, add"
                new = rounds(lambda: ctx.point_lincomb2_batch(a, b, px, py, qx, qy, curve=curve, plan=plan, outx=o5, outy=o6, err=err))
                m1 = rounds(lambda: ctx.point_mul_batch(a, px, py, curve=curve, plan=plan, outx=o1, outy=o2, err=err))
                m2 = rounds(lambda: ctx.point_mul_batch(b, qx, qy, curve=curve, plan=plan, outx=o3, outy=o4, err=err))
                ad = rounds(lambda: ctx.point_add_batch(o1, o2, o3, o4, curve=curve, outx=o5, outy=o6, err=err))
                old = mean(m1) + mean(m2) + mean(ad)
                emit({"section": "lincomb2", "curve": cname, "plan": PLAN_NAMES[plan], "log2_n": lg, "lincomb2_ms": new["ms"],
                      "lincomb2_spread": new["spread"], "lincomb2_per_s": rate(n, new), "point_mul_a_ms": m1["ms"], "point_mul_b_ms": m2["ms"],
                      "point_add_ms": ad["ms"], "yardstick_spread": max(m1["spread"], m2["spread"], ad["spread"]),
                      "three_calls_ms": round(old, 4), "lincomb2_over_three_calls": round(mean(new) / old, 4)})

        # ---- DLEQ -----------------------------------------------------------------------------------------------------------
        if os.environ.get("ONLY_LINCOMB2"):   # (an A/B build of the walk under P2E_LIB needs no more)
            continue
        aux, msg = rnd(n, 32), rnd(n, 32)
        ax, ay, _e, bad1 = ctx.ecdsa_public_key_batch(a, curve=K1)
        bx, by, _e, bad2 = ctx.ecdsa_public_key_batch(b, curve=K1)
        assert bad1 == 0 and bad2 == 0
        proof, cx, cy, valid = buf(64), buf(), buf(), torch.empty(n, dtype=torch.uint8, device="cuda")
        assert ctx.dleq_prove_batch(a, bx, by, aux, msg=msg, proof=proof, cx=cx, cy=cy, err=err)[4] == 0
        assert ctx.dleq_verify_batch(ax, ay, bx, by, cx, cy, proof, msg=msg, err=err, valid=valid)[2] == 0 and bool((valid == 1).all())
        wrong = proof.clone()
        wrong[:, 40] ^= 1
        assert ctx.dleq_verify_batch(ax, ay, bx, by, cx, cy, wrong, msg=msg, err=err, valid=valid)[2] == 0 and not bool(valid.any())
        del wrong
        e_le, s_le = torch.flip(proof[:, :32], dims=[1]).contiguous(), torch.flip(proof[:, 32:], dims=[1]).contiguous()
        GLV = p2e.MUL_PLAN_GLV
        ver = rounds(lambda: ctx.dleq_verify_batch(ax, ay, bx, by, cx, cy, proof, msg=msg, err=err, valid=valid))
        lin = rounds(lambda: ctx.point_lincomb_batch(s_le, e_le, ax, ay, curve=K1, plan=GLV, outx=o1, outy=o2, err=err))
        m1 = rounds(lambda: ctx.point_mul_batch(s_le, bx, by, curve=K1, plan=GLV, outx=o1, outy=o2, err=err))
        m2 = rounds(lambda: ctx.point_mul_batch(e_le, cx, cy, curve=K1, plan=GLV, outx=o3, outy=o4, err=err))
        ad = rounds(lambda: ctx.point_add_batch(o1, o2, o3, o4, curve=K1, outx=o5, outy=o6, err=err))
        old = mean(lin) + mean(m1) + mean(m2) + mean(ad)
        emit({"section": "verify", "log2_n": lg, "verify_ms": ver["ms"], "verify_spread": ver["spread"], "verify_per_s": rate(n, ver),
              "point_lincomb_ms": lin["ms"], "point_mul_sB_ms": m1["ms"], "point_mul_eC_ms": m2["ms"], "point_add_ms": ad["ms"],
              "yardstick_spread": max(lin["spread"], m1["spread"], m2["spread"], ad["spread"]), "four_calls_ms": round(old, 4),
              "verify_over_four_calls": round(mean(ver) / old, 4)})
        prv = rounds(lambda: ctx.dleq_prove_batch(a, bx, by, aux, msg=msg, proof=proof, cx=cx, cy=cy, err=err))
        p1 = rounds(lambda: ctx.ecdsa_public_key_batch(a, curve=K1, pkx=o1, pky=o2, err=err))
        p2 = rounds(lambda: ctx.ecdsa_public_key_batch(s_le, curve=K1, pkx=o1, pky=o2, err=err))
        m1 = rounds(lambda: ctx.point_mul_batch(a, bx, by, curve=K1, plan=GLV, outx=o3, outy=o4, err=err))
        m2 = rounds(lambda: ctx.point_mul_batch(s_le, bx, by, curve=K1, plan=GLV, outx=o3, outy=o4, err=err))
        old = mean(p1) + mean(p2) + mean(m1) + mean(m2)
        emit({"section": "prove", "log2_n": lg, "prove_ms": prv["ms"], "prove_spread": prv["spread"], "prove_per_s": rate(n, prv),
              "public_key_a_ms": p1["ms"], "public_key_k_ms": p2["ms"], "point_mul_aB_ms": m1["ms"], "point_mul_kB_ms": m2["ms"],
              "yardstick_spread": max(p1["spread"], p2["spread"], m1["spread"], m2["spread"]), "four_calls_ms": round(old, 4),
              "prove_over_four_calls": round(mean(prv) / old, 4)})
        del aux, msg, proof
