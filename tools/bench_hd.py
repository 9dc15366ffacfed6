"""BIP-32 key derivation and HASH160 (include/p2e.h p2e_bip32_master_batch and the four calls after it): time per call,
against the calls of this library that do their curve work today.

The method of MEASUREMENTS.md section 17, as tools/bench_schnorr.py applies it: inputs are made on the device (random bytes;
secret keys with the top byte cleared and the lowest bit set, so 0 < sk < n), parent public keys by the library, everything
stays on the device.  A figure is the median of REPS (default 21) timed calls after WARMUP (3), measured with HIP events on
the caller's stream around the call alone; every point runs ROUNDS (2) times and `spread` is the relative difference between
the repeated medians.  One process.  Before anything is timed the private and the public derivation are compared on the
whole batch: the public key of CKDpriv's child equals CKDpub's child, and so do the chain codes.
One JSON line per point, n = 2^12, 2^16, 2^20:
  ckd        p2e_bip32_ckd_pub_batch, and p2e_bip32_ckd_priv_batch with non-hardened indices, against the SUM of
             p2e_ecdsa_public_key_batch (P2E_SIGN_PLAN_LANE) and p2e_point_add_batch on the same elements: `pub_over_sum`,
             `priv_over_sum`; above 1.10 wants an explanation.  Both with one parent per element and with one parent for the batch.
  hardened   p2e_bip32_ckd_priv_batch with hardened indices and p2e_bip32_master_batch (32-byte seeds), in elements per second
  hash160    p2e_key_hash160_batch (both forms) next to p2e_eth_address_batch on the same keys, and p2e_hash160_batch over
             the 33-byte keys, in elements per second
usage: python tools/bench_hd.py [out.jsonl]   (default profiles/hd.jsonl; appended to)"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import plonky2_ecdsa_amd as p2e

args = sys.argv[1:]
out_path = args.pop(0) if args and args[0].endswith(".jsonl") else os.path.join(ROOT, "profiles", "hd.jsonl")
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
        gen = torch.Generator(device="cuda").manual_seed(32 + lg)
        rnd = lambda *shape: torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=gen)
        sk, cc, seed = rnd(n, 32), rnd(n, 32), rnd(n, 32)
        sk[:, 31] = 0          # little-endian: below 2^248
        sk[:, 0] |= 1          # and not zero
        index = torch.randint(0, (1 << 31) - 1, (n,), dtype=torch.int32, device="cuda", generator=gen)       # non-hardened
        hardened = index | torch.tensor(-(1 << 31), dtype=torch.int32, device="cuda")
        px, py, err, bad = ctx.ecdsa_public_key_batch(sk, curve=K1, plan=p2e.SIGN_PLAN_LANE)
        assert bad == 0
        o1, o2, o3, o4, o5 = (torch.empty_like(sk) for _ in range(5))
        h20, a20 = torch.empty((n, 20), dtype=torch.uint8, device="cuda"), torch.empty((n, 20), dtype=torch.uint8, device="cuda")
        # the two derivations agree on the whole batch
        csk, ccc, err, bad = ctx.bip32_ckd_priv_batch(sk, cc, index)
        assert bad == 0
        cx, cy, err, bad = ctx.ecdsa_public_key_batch(csk, curve=K1, plan=p2e.SIGN_PLAN_LANE)
        qx, qy, qcc, err, bad2 = ctx.bip32_ckd_pub_batch(px, py, cc, index)
        assert bad == 0 and bad2 == 0 and torch.equal(cx, qx) and torch.equal(cy, qy) and torch.equal(ccc, qcc)

        pub = rounds(lambda: ctx.bip32_ckd_pub_batch(px, py, cc, index, pkx=o1, pky=o2, cc=o3, err=err))
        priv = rounds(lambda: ctx.bip32_ckd_priv_batch(sk, cc, index, sk=o1, cc=o3, err=err))
        pub1 = rounds(lambda: ctx.bip32_ckd_pub_batch(px[:1], py[:1], cc[:1], index, pkx=o1, pky=o2, cc=o3, err=err))
        priv1 = rounds(lambda: ctx.bip32_ckd_priv_batch(sk[:1], cc[:1], index, sk=o1, cc=o3, err=err))
        keys = rounds(lambda: ctx.ecdsa_public_key_batch(sk, curve=K1, plan=p2e.SIGN_PLAN_LANE, pkx=o4, pky=o5, err=err))
        add = rounds(lambda: ctx.point_add_batch(px, py, qx, qy, curve=K1, outx=o4, outy=o5, err=err))
        total = mean(keys) + mean(add)
        emit({"section": "ckd", "log2_n": lg, "ckd_pub_ms": pub["ms"], "ckd_pub_spread": pub["spread"], "ckd_priv_ms": priv["ms"],
              "ckd_priv_spread": priv["spread"], "ckd_pub_one_parent_ms": pub1["ms"], "ckd_priv_one_parent_ms": priv1["ms"],
              "public_key_lane_ms": keys["ms"], "public_key_lane_spread": keys["spread"], "point_add_ms": add["ms"],
              "point_add_spread": add["spread"], "pub_over_sum": round(mean(pub) / total, 4), "priv_over_sum": round(mean(priv) / total, 4),
              "pub_one_parent_over_sum": round(mean(pub1) / total, 4), "priv_one_parent_over_sum": round(mean(priv1) / total, 4), "bar": 1.10})
        hard = rounds(lambda: ctx.bip32_ckd_priv_batch(sk, cc, hardened, sk=o1, cc=o3, err=err))
        mast = rounds(lambda: ctx.bip32_master_batch(seed, sk=o1, cc=o3, err=err))
        emit({"section": "hardened", "log2_n": lg, "ckd_priv_hardened_ms": hard["ms"], "ckd_priv_hardened_spread": hard["spread"],
              "ckd_priv_hardened_per_s": rate(n, hard), "master_ms": mast["ms"], "master_spread": mast["spread"], "master_per_s": rate(n, mast)})
        sec1, err, bad = ctx.point_encode_batch(px, py, curve=K1, form=p2e.SEC1_COMPRESSED)
        assert bad == 0
        offsets = torch.arange(n + 1, dtype=torch.int64, device="cuda") * 33
        kc = rounds(lambda: ctx.key_hash160_batch(px, py, form=p2e.SEC1_COMPRESSED, out=h20))
        want = h20.clone()
        ku = rounds(lambda: ctx.key_hash160_batch(px, py, form=p2e.SEC1_UNCOMPRESSED, out=h20))
        eth = rounds(lambda: ctx.eth_address_batch(px, py, addr=a20))
        msg = rounds(lambda: ctx.hash160_batch(sec1, offsets, out=h20))
        assert torch.equal(h20, want)                                            # the message route over the same 33 bytes
        emit({"section": "hash160", "log2_n": lg, "key_hash160_compressed_ms": kc["ms"], "key_hash160_compressed_spread": kc["spread"],
              "key_hash160_compressed_per_s": rate(n, kc), "key_hash160_uncompressed_ms": ku["ms"], "key_hash160_uncompressed_per_s": rate(n, ku),
              "eth_address_ms": eth["ms"], "eth_address_spread": eth["spread"], "eth_address_per_s": rate(n, eth),
              "key_hash160_over_eth_address": round(mean(kc) / mean(eth), 4), "hash160_ms": msg["ms"], "hash160_spread": msg["spread"],
              "hash160_per_s": rate(n, msg)})
