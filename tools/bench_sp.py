"""Silent payments (include/p2e.h p2e_sp_input_hash_batch and the three calls after it): time per call, against the calls of this
library that do the same arithmetic on the same elements.

The method of MEASUREMENTS.md section 17, as tools/bench_taproot.py applies it: inputs are made on the device (random bytes;
secret keys and stand-in scalars with the top byte cleared and the lowest bit set, so 0 < value < n), everything stays on the
device.  A figure is the median of REPS (default 21) timed calls after WARMUP (3), measured with HIP events on the caller's
stream around the call alone; every point runs ROUNDS (2) times and `spread` is the relative difference between the repeated
medians.  One process.  Before anything is timed the sender's route and the receiver's route are compared on the whole batch:
every payment made by p2e_sp_send_batch is found by p2e_sp_scan_batch.
One JSON line per point, n = 2^12, 2^16, 2^20 transactions of OUTPUTS (2) outputs each:
  scan       p2e_sp_scan_batch (max_hits = 2) with no labels and no hits (the chain-scan case: one step), with 16 labels, and with
             one hit per transaction (two steps: the hit, then the step that finds nothing), against the PRIMARY yardstick on
             the same elements -- p2e_point_mul_batch (GLV plan) plus p2e_taproot_tweak_pubkey_batch with root32 = NULL (ONE
             step's work, so the one-hit figure carries a second step): `scan_over_primary`, `scan_labels_over_primary`,
             `scan_hit_over_primary` -- and against the full old route, point_mul + point_encode + hash_batch + xonly_decode +
             point_lincomb (b = 1), the host steps in between not counted: `scan_over_route`.  `yardstick_spread` is the larger
             of the two spreads of the primary yardstick's calls.
  send       p2e_sp_send_batch against the same primary sum: `send_over_primary`
  input_hash p2e_sp_input_hash_batch against p2e_hash_batch (SHA-256) on 69-byte messages: `input_hash_over_hash69`
  label      p2e_sp_label_batch against p2e_schnorr_public_key_batch: `label_over_public_key`
usage: python tools/bench_sp.py [out.jsonl]   (default profiles/sp.jsonl; appended to)"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import plonky2_ecdsa_amd as p2e

args = sys.argv[1:]
out_path = args.pop(0) if args and args[0].endswith(".jsonl") else os.path.join(ROOT, "profiles", "sp.jsonl")
REPS, WARMUP, ROUNDS = int(os.environ.get("REPS", "21")), int(os.environ.get("WARMUP", "3")), int(os.environ.get("ROUNDS", "2"))
SIZES = [int(v) for v in os.environ.get("LOG2_SIZES", "12,16,20").split(",")]
OUTPUTS = 2
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
        gen = torch.Generator(device="cuda").manual_seed(352 + lg)
        rnd = lambda *shape: torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=gen)

        def secret(*shape):                 # little-endian, 0 < value < 2^248
            v = rnd(*shape, 32)
            v[..., 31] = 0
            v[..., 0] |= 1
            return v
        a_sk, keys = secret(n), secret(2)
        scan_sk, spend_sk = keys[:1].contiguous(), keys[1:].contiguous()
        ax, ay, err, bad = ctx.ecdsa_public_key_batch(a_sk, curve=K1)
        rx, ry, _e, bad2 = ctx.ecdsa_public_key_batch(keys, curve=K1)
        assert bad == 0 and bad2 == 0
        scan_pkx, scan_pky = rx[:1].expand(n, 32).contiguous(), ry[:1].expand(n, 32).contiguous()
        spend_pkx, spend_pky = rx[1:].expand(n, 32).contiguous(), ry[1:].expand(n, 32).contiguous()
        outpoint = rnd(n, 36)
        ih, _e, bad = ctx.sp_input_hash_batch(outpoint, ax, ay)
        assert bad == 0
        k0 = torch.zeros(n, dtype=torch.int32, device="cuda")
        paid, _e, bad = ctx.sp_send_batch(a_sk, ih, scan_pkx, scan_pky, spend_pkx, spend_pky, k0)
        assert bad == 0
        idx16 = torch.arange(16, dtype=torch.int32, device="cuda")
        _t, lx, ly, _e, bad = ctx.sp_label_batch(scan_sk, idx16)
        assert bad == 0
        decoys = rnd(n * OUTPUTS, 32)
        hits = decoys.clone()
        hits[OUTPUTS - 1::OUTPUTS] = paid     # one payment per transaction, in its last output
        offsets = torch.arange(n + 1, dtype=torch.int64, device="cuda") * OUTPUTS
        MAX_HITS = 2                          # a hit is followed by the step k = 1 that finds nothing, as in a wallet's scan
        n_hits = torch.empty(n, dtype=torch.uint8, device="cuda")
        hit_output = torch.empty((n, MAX_HITS), dtype=torch.int32, device="cuda")
        hit_label = torch.empty((n, MAX_HITS), dtype=torch.uint8, device="cuda")
        hit_tweak = torch.empty((n, MAX_HITS, 32), dtype=torch.uint8, device="cuda")

        def scan(outputs, labels):
            kw = dict(label_x=lx, label_y=ly) if labels else {}
            return ctx.sp_scan_batch(scan_sk, rx[1:], ry[1:], ax, ay, outputs, offsets, input_hash=ih, max_hits=MAX_HITS, n_hits=n_hits,
                                     hit_output=hit_output, hit_label=hit_label, hit_tweak=hit_tweak, err=err, **kw)
        # sender = receiver on the whole batch, and no decoy is a hit
        assert scan(hits, False)[5] == 0 and bool((n_hits == 1).all()) and bool((hit_output[:, 0] == OUTPUTS - 1).all())
        assert scan(decoys, True)[5] == 0 and not bool(n_hits.any())

        o1, o2, o3, o4 = (torch.empty((n, 32), dtype=torch.uint8, device="cuda") for _ in range(4))
        par = torch.empty(n, dtype=torch.uint8, device="cuda")
        enc = torch.empty((n, 33), dtype=torch.uint8, device="cuda")
        k_le, one_le = secret(n), torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
        one_le[:, 0] = 1
        msg37, off37 = rnd(n * 37), torch.arange(n + 1, dtype=torch.int64, device="cuda") * 37
        msg69, off69 = rnd(n * 69), torch.arange(n + 1, dtype=torch.int64, device="cuda") * 69
        xonly, _e, bad = ctx.schnorr_public_key_batch(torch.flip(a_sk, dims=[1]).contiguous())
        assert bad == 0

        s_plain = rounds(lambda: scan(decoys, False))
        s_label = rounds(lambda: scan(decoys, True))
        s_hit = rounds(lambda: scan(hits, False))
        send = rounds(lambda: ctx.sp_send_batch(a_sk, ih, scan_pkx, scan_pky, spend_pkx, spend_pky, k0, out_pk=o1, err=err))
        mul = rounds(lambda: ctx.point_mul_batch(k_le, ax, ay, curve=K1, plan=p2e.MUL_PLAN_GLV, outx=o1, outy=o2, err=err))
        tweak = rounds(lambda: ctx.taproot_tweak_pubkey_batch(xonly, None, out_pk=o3, out_parity=par, err=err))
        encode = rounds(lambda: ctx.point_encode_batch(ax, ay, curve=K1, form=p2e.SEC1_COMPRESSED, out=enc, err=err))
        h37 = rounds(lambda: ctx.hash_batch(msg37, off37, alg=p2e.HASH_SHA256, out=o3))
        dec = rounds(lambda: ctx.xonly_decode_batch(xonly, px=o3, py=o4, err=err))
        lin = rounds(lambda: ctx.point_lincomb_batch(k_le, one_le, ax, ay, curve=K1, outx=o3, outy=o4, err=err))
        primary = mean(mul) + mean(tweak)
        route = mean(mul) + mean(encode) + mean(h37) + mean(dec) + mean(lin)
        emit({"section": "scan", "log2_n": lg, "outputs": OUTPUTS, "max_hits": MAX_HITS, "scan_ms": s_plain["ms"], "scan_spread": s_plain["spread"],
              "scan_per_s": rate(n, s_plain), "scan_labels16_ms": s_label["ms"], "scan_labels16_spread": s_label["spread"],
              "scan_hit_ms": s_hit["ms"], "scan_hit_spread": s_hit["spread"], "point_mul_glv_ms": mul["ms"], "point_mul_glv_spread": mul["spread"],
              "tweak_pubkey_no_root_ms": tweak["ms"], "tweak_pubkey_no_root_spread": tweak["spread"],
              "yardstick_spread": max(mul["spread"], tweak["spread"]), "point_encode_ms": encode["ms"], "hash_batch_37_ms": h37["ms"],
              "xonly_decode_ms": dec["ms"], "point_lincomb_b1_ms": lin["ms"], "scan_over_primary": round(mean(s_plain) / primary, 4),
              "scan_labels_over_primary": round(mean(s_label) / primary, 4), "scan_hit_over_primary": round(mean(s_hit) / primary, 4),
              "scan_over_route": round(mean(s_plain) / route, 4)})
        emit({"section": "send", "log2_n": lg, "send_ms": send["ms"], "send_spread": send["spread"], "send_per_s": rate(n, send),
              "send_over_primary": round(mean(send) / primary, 4)})

        ihr = rounds(lambda: ctx.sp_input_hash_batch(outpoint, ax, ay, input_hash=o1, err=err))
        h69 = rounds(lambda: ctx.hash_batch(msg69, off69, alg=p2e.HASH_SHA256, out=o1))
        emit({"section": "input_hash", "log2_n": lg, "input_hash_ms": ihr["ms"], "input_hash_spread": ihr["spread"], "input_hash_per_s": rate(n, ihr),
              "hash_batch_69_ms": h69["ms"], "hash_batch_69_spread": h69["spread"], "input_hash_over_hash69": round(mean(ihr) / mean(h69), 4)})

        index = torch.arange(n, dtype=torch.int32, device="cuda")
        sk_be = torch.flip(a_sk, dims=[1]).contiguous()
        lab = rounds(lambda: ctx.sp_label_batch(scan_sk, index, label_tweak=o1, label_x=o2, label_y=o3, err=err))
        pub = rounds(lambda: ctx.schnorr_public_key_batch(sk_be, pk=o1, err=err))
        emit({"section": "label", "log2_n": lg, "label_ms": lab["ms"], "label_spread": lab["spread"], "label_per_s": rate(n, lab),
              "schnorr_public_key_ms": pub["ms"], "schnorr_public_key_spread": pub["spread"],
              "label_over_public_key": round(mean(lab) / mean(pub), 4)})
        del decoys, hits, msg37, msg69
