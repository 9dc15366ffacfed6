"""Taproot (include/p2e.h p2e_taproot_leaf_hash_batch and the four calls after it): time per call, against the calls of this
library that do the same arithmetic on the same elements.

The method of MEASUREMENTS.md section 17, as tools/bench_hd.py applies it: inputs are made on the device (random bytes; secret
keys and stand-in tweaks with the top byte cleared and the lowest bit set, so 0 < value < n), everything stays on the device.
A figure is the median of REPS (default 21) timed calls after WARMUP (3), measured with HIP events on the caller's stream
around the call alone; every point runs ROUNDS (2) times and `spread` is the relative difference between the repeated medians.
One process.  Before anything is timed the two routes to an output key are compared on the whole batch (the key of the tweaked
secret key equals the tweaked public key) and every commitment made here is checked valid.
One JSON line per point, n = 2^12, 2^16, 2^20:
  tweak      p2e_taproot_tweak_pubkey_batch against today's route, p2e_xonly_decode_batch + p2e_point_lincomb_batch with a = t,
             b = 1 (t a stand-in scalar: its hash is outside the timed region), `pubkey_over_route`, and against its floor,
             p2e_schnorr_public_key_batch + p2e_xonly_decode_batch (one fixed-base walk, one square root), `pubkey_over_floor`;
             p2e_taproot_tweak_seckey_batch against p2e_schnorr_public_key_batch, `seckey_over_public_key`
  leaf       p2e_taproot_leaf_hash_batch against p2e_hash_batch (SHA-256) on the same 34-byte scripts, `leaf_over_hash`
  merkle     p2e_taproot_merkle_root_batch at depth 1 and depth 32 (max_depth = depth, the element-major layout), per level,
             against p2e_hash_batch on 64-byte messages: `level_over_hash64`; p2e_taproot_verify_commitment_batch against
             merkle_root + tweak_pubkey on the same elements: `verify_over_parts`
usage: python tools/bench_taproot.py [out.jsonl]   (default profiles/taproot.jsonl; appended to)"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import plonky2_ecdsa_amd as p2e

args = sys.argv[1:]
out_path = args.pop(0) if args and args[0].endswith(".jsonl") else os.path.join(ROOT, "profiles", "taproot.jsonl")
REPS, WARMUP, ROUNDS = int(os.environ.get("REPS", "21")), int(os.environ.get("WARMUP", "3")), int(os.environ.get("ROUNDS", "2"))
SIZES = [int(v) for v in os.environ.get("LOG2_SIZES", "12,16,20").split(",")]
DEPTHS = [int(v) for v in os.environ.get("DEPTHS", "1,32").split(",")]
SCRIPT_BYTES = 34                      # <32-byte push> OP_CHECKSIG: the single-key leaf
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
        gen = torch.Generator(device="cuda").manual_seed(341 + lg)
        rnd = lambda *shape: torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=gen)
        sk, root, t_le = rnd(n, 32), rnd(n, 32), rnd(n, 32)
        sk[:, 0] = 0           # big-endian: below 2^248
        sk[:, 31] |= 1         # and not zero
        t_le[:, 31] = 0        # the stand-in tweak of today's route, little-endian as point_lincomb_batch takes it
        t_le[:, 0] |= 1
        one_le = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
        one_le[:, 0] = 1
        pk, err, bad = ctx.schnorr_public_key_batch(sk)
        assert bad == 0
        o1, o2, o3, o4 = (torch.empty_like(sk) for _ in range(4))
        par, valid = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
        # the two routes to an output key agree on the whole batch
        tsk, err, bad = ctx.taproot_tweak_seckey_batch(sk, root)
        q_sec, err, bad2 = ctx.schnorr_public_key_batch(tsk)
        q_pub, q_par, err, bad3 = ctx.taproot_tweak_pubkey_batch(pk, root)
        assert bad == 0 and bad2 == 0 and bad3 == 0 and torch.equal(q_sec, q_pub)

        tweak = rounds(lambda: ctx.taproot_tweak_pubkey_batch(pk, root, out_pk=o1, out_parity=par, err=err))
        tweak0 = rounds(lambda: ctx.taproot_tweak_pubkey_batch(pk, None, out_pk=o1, out_parity=par, err=err))
        tsec = rounds(lambda: ctx.taproot_tweak_seckey_batch(sk, root, out_sk=o1, err=err))
        keys = rounds(lambda: ctx.schnorr_public_key_batch(sk, pk=o1, err=err))
        dec = rounds(lambda: ctx.xonly_decode_batch(pk, px=o2, py=o3, err=err))
        lin = rounds(lambda: ctx.point_lincomb_batch(t_le, one_le, o2, o3, curve=K1, outx=o1, outy=o4, err=err))
        route, floor = mean(dec) + mean(lin), mean(keys) + mean(dec)
        emit({"section": "tweak", "log2_n": lg, "tweak_pubkey_ms": tweak["ms"], "tweak_pubkey_spread": tweak["spread"],
              "tweak_pubkey_no_root_ms": tweak0["ms"], "tweak_pubkey_per_s": rate(n, tweak), "tweak_seckey_ms": tsec["ms"],
              "tweak_seckey_spread": tsec["spread"], "tweak_seckey_per_s": rate(n, tsec), "schnorr_public_key_ms": keys["ms"],
              "schnorr_public_key_spread": keys["spread"], "xonly_decode_ms": dec["ms"], "xonly_decode_spread": dec["spread"],
              "point_lincomb_b1_ms": lin["ms"], "point_lincomb_b1_spread": lin["spread"],
              "pubkey_over_route": round(mean(tweak) / route, 4), "pubkey_over_floor": round(mean(tweak) / floor, 4),
              "seckey_over_public_key": round(mean(tsec) / mean(keys), 4)})

        scripts = rnd(n * SCRIPT_BYTES)
        offsets = torch.arange(n + 1, dtype=torch.int64, device="cuda") * SCRIPT_BYTES
        version = torch.full((n,), 0xC0, dtype=torch.uint8, device="cuda")
        leaf, err, bad = ctx.taproot_leaf_hash_batch(version, scripts, offsets)
        assert bad == 0
        lh = rounds(lambda: ctx.taproot_leaf_hash_batch(version, scripts, offsets, leaf=o1, err=err))
        sha = rounds(lambda: ctx.hash_batch(scripts, offsets, alg=p2e.HASH_SHA256, out=o1))
        emit({"section": "leaf", "log2_n": lg, "script_bytes": SCRIPT_BYTES, "leaf_hash_ms": lh["ms"], "leaf_hash_spread": lh["spread"],
              "leaf_hash_per_s": rate(n, lh), "hash_batch_sha256_ms": sha["ms"], "hash_batch_sha256_spread": sha["spread"],
              "leaf_over_hash": round(mean(lh) / mean(sha), 4)})

        msg64 = rnd(n * 64)
        off64 = torch.arange(n + 1, dtype=torch.int64, device="cuda") * 64
        h64 = rounds(lambda: ctx.hash_batch(msg64, off64, alg=p2e.HASH_SHA256, out=o1))
        for depth in DEPTHS:
            path = rnd(n, depth, 32)
            dep = torch.full((n,), depth, dtype=torch.uint8, device="cuda")
            mroot, err, bad = ctx.taproot_merkle_root_batch(leaf, path, dep)
            q, qpar, err, bad2 = ctx.taproot_tweak_pubkey_batch(pk, mroot)
            err, valid, bad3 = ctx.taproot_verify_commitment_batch(q, qpar, pk, leaf, path, dep)
            assert bad == 0 and bad2 == 0 and bad3 == 0 and bool((valid == 1).all())
            mr = rounds(lambda: ctx.taproot_merkle_root_batch(leaf, path, dep, root=o1, err=err))
            tw = rounds(lambda: ctx.taproot_tweak_pubkey_batch(pk, mroot, out_pk=o2, out_parity=par, err=err))
            vc = rounds(lambda: ctx.taproot_verify_commitment_batch(q, qpar, pk, leaf, path, dep, err=err, valid=valid))
            emit({"section": "merkle", "log2_n": lg, "depth": depth, "merkle_root_ms": mr["ms"], "merkle_root_spread": mr["spread"],
                  "per_level_ms": round(mean(mr) / depth, 4), "hash_batch_64_ms": h64["ms"], "hash_batch_64_spread": h64["spread"],
                  "level_over_hash64": round(mean(mr) / depth / mean(h64), 4), "path_bytes_per_s": round(n * depth * 32 / (mean(mr) * 1e-3)),
                  "tweak_pubkey_ms": tw["ms"], "verify_commitment_ms": vc["ms"], "verify_commitment_spread": vc["spread"],
                  "verify_commitment_per_s": rate(n, vc), "verify_over_parts": round(mean(vc) / (mean(mr) + mean(tw)), 4)})
            del path
