"""Message hashing, RFC 6979 nonces, the deterministic signer and Ethereum addresses (include/p2e.h p2e_hash_batch and the
three calls after it): calls per second at n = 2^16.

  hash      per algorithm and message length (64, 200, 1024 bytes): hashes per second, beside the host's hashlib.sha256
            on THREADS (16) threads over the same buffer (see host_sha256 for what that figure is)
  nonce     p2e_ecdsa_nonce_rfc6979_batch per curve
  signer    p2e_ecdsa_sign_deterministic_batch beside p2e_ecdsa_sign_recoverable_batch on the same batch, same plan (AUTO):
            the difference should be the nonce call plus one memset of 32 n bytes
  address   p2e_eth_address_batch
Each figure: the median of REPS (default 21) calls after WARMUP (3), HIP events on the caller's stream around the call
alone (inputs and outputs stay on the device); every point runs ROUNDS (2) times and `spread` is the relative difference
between the repeated medians.  One JSON line per point; usage: python tools/bench_hash.py [out.jsonl] [log2 n]
(default profiles/hash_batch.jsonl, 16)"""
import hashlib
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import plonky2_ecdsa_amd as p2e

args = sys.argv[1:]
out_path = args.pop(0) if args and not args[0].isdigit() else os.path.join(ROOT, "profiles", "hash_batch.jsonl")
lg = int(args[0]) if args else 16
n = 1 << lg
REPS, WARMUP, ROUNDS = int(os.environ.get("REPS", "21")), int(os.environ.get("WARMUP", "3")), int(os.environ.get("ROUNDS", "2"))
THREADS = int(os.environ.get("THREADS", "16"))
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


def point(out, rec, fns):
    """fns: {name: callable}; adds <name>_ms (one median per round), <name>_spread, <name>_per_s"""
    med = {k: [] for k in fns}
    for _round in range(ROUNDS):
        for k, fn in fns.items():
            med[k].append(timed(fn))
    torch.cuda.synchronize()
    for k in fns:
        rec[k + "_ms"] = [round(x, 4) for x in med[k]]
        rec[k + "_spread"] = round((max(med[k]) - min(med[k])) / min(med[k]), 4)
        rec[k + "_per_s"] = round(n / (statistics.mean(med[k]) * 1e-3))
    line = json.dumps(rec)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


def host_sha256(raw, length):
    """hashlib.sha256 over the same n messages on THREADS threads (each thread a contiguous share): hashes per second,
    best of three.  Short messages hold the GIL, so this is what a Python host gets, not what 16 cores could do in C."""
    def share(t):
        lo, hi = t * n // THREADS, (t + 1) * n // THREADS
        view = memoryview(raw)
        return [hashlib.sha256(view[i * length:(i + 1) * length]).digest() for i in range(lo, hi)][-1]
    best = None
    with ThreadPoolExecutor(max_workers=THREADS) as ex:
        for _ in range(3):
            t0 = time.perf_counter()
            list(ex.map(share, range(THREADS)))
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
    return round(n / best)


with open(out_path, "w") as out:
    gen = torch.Generator(device="cuda").manual_seed(6979 + lg)
    for length in (64, 200, 1024):
        data = torch.randint(0, 256, (n * length + 3,), dtype=torch.uint8, device="cuda", generator=gen)[3:]   # first byte off the word grid
        offsets = torch.arange(n + 1, dtype=torch.int64, device="cuda") * length
        digest = torch.empty((n, 32), dtype=torch.uint8, device="cuda")
        raw = data.cpu().numpy().tobytes()
        fns = {name: (lambda alg=alg: ctx.hash_batch(data, offsets, alg=alg, out_form=p2e.DIGEST_SCALAR, out=digest))
               for name, alg in (("sha256", p2e.HASH_SHA256), ("sha256d", p2e.HASH_SHA256D), ("keccak256", p2e.HASH_KECCAK256))}
        point(out, {"box": box, "what": "hash", "log2_n": lg, "n": n, "bytes": length, "reps": REPS,
                    "host_sha256_per_s": host_sha256(raw, length), "host_threads": THREADS}, fns)
        del raw
    for curve, cname in ((p2e.CURVE_SECP256K1, "secp256k1"), (p2e.CURVE_P256, "p256")):
        msg, sk = [torch.randint(0, 256, (n, 32), dtype=torch.uint8, device="cuda", generator=gen) for _ in range(2)]
        k, r, s = [torch.empty_like(msg) for _ in range(3)]
        v, err = [torch.empty(n, dtype=torch.uint8, device="cuda") for _ in range(2)]
        ctx.ecdsa_nonce_rfc6979_batch(msg, sk, curve=curve, k=k)
        wipe = torch.empty(32 * n, dtype=torch.uint8, device="cuda")
        point(out, {"box": box, "what": "sign", "curve": cname, "log2_n": lg, "n": n, "reps": REPS},
              {"nonce": lambda: ctx.ecdsa_nonce_rfc6979_batch(msg, sk, curve=curve, k=k),
               "sign_recoverable": lambda: ctx.ecdsa_sign_recoverable_batch(msg, sk, k, curve=curve, r=r, s=s, v=v, err=err),
               "sign_deterministic": lambda: ctx.ecdsa_sign_deterministic_batch(msg, sk, curve=curve, r=r, s=s, v=v, err=err),
               "memset_32n": lambda: wipe.zero_()})
    pkx, pky = [torch.randint(0, 256, (n, 32), dtype=torch.uint8, device="cuda", generator=gen) for _ in range(2)]
    addr = torch.empty((n, 20), dtype=torch.uint8, device="cuda")
    err = torch.zeros(n, dtype=torch.uint8, device="cuda")
    point(out, {"box": box, "what": "address", "log2_n": lg, "n": n, "reps": REPS},
          {"address": lambda: ctx.eth_address_batch(pkx, pky, addr=addr), "address_with_err": lambda: ctx.eth_address_batch(pkx, pky, err=err, addr=addr)})
