"""MuSig2 (include/p2e.h p2e_musig_key_agg_batch and the six calls after it): time per call, against the calls of this library that
do the same curve work on the same elements in the same run.

The method of MEASUREMENTS.md section 17, as tools/bench_sp.py applies it: inputs are made on the device (random bytes; secret
keys, nonces and stand-in scalars with the top byte cleared and the lowest bit set, so 0 < value < n), everything stays on the
device.  A figure is the median of REPS (default 21) timed calls after WARMUP (3), measured with HIP events on the caller's
stream around the call alone; every point runs ROUNDS (2) times and `spread` is the relative difference between the repeated
medians.  One process.  Before anything is timed the whole chain runs once on the batch of two-signer sessions and every
signature is handed to p2e_schnorr_verify_batch.
One JSON line per point, n = 2^12, 2^16, 2^20 sessions:
  key_agg2    p2e_musig_key_agg_batch with 2 signers against p2e_point_mul_batch (GLV) + p2e_point_add_batch on n elements (the
              second key's coefficient is 1: one walk per session)
  key_agg16   the same with 16 signers against 15 x p2e_point_mul_batch on n elements (at 2^20: on 2^18 sessions, so that the
              per-signer arrays stay at 2^22 keys; the yardstick runs on the same 2^18)
  session     p2e_musig_session_batch against p2e_point_mul_batch + p2e_point_add_batch
  verify      p2e_musig_partial_verify_batch against p2e_point_mul_batch + p2e_point_lincomb_batch
  sign        p2e_musig_partial_sign_batch against p2e_ecdsa_public_key_batch + p2e_point_mul_batch (the yardstick the issue of
              this call names; the signer itself holds one fixed-base walk and no general-point walk)
  light       p2e_musig_apply_tweak_batch against p2e_taproot_tweak_pubkey_batch; p2e_musig_nonce_agg_batch (2 signers) and
              p2e_musig_sig_agg_batch (2 signers), without a yardstick
usage: python tools/bench_musig.py [out.jsonl]   (default profiles/musig.jsonl; appended to)"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import plonky2_ecdsa_amd as p2e

args = sys.argv[1:]
out_path = args.pop(0) if args and args[0].endswith(".jsonl") else os.path.join(ROOT, "profiles", "musig.jsonl")
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
        gen = torch.Generator(device="cuda").manual_seed(327 + lg)
        rnd = lambda *shape: torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=gen)
        buf = lambda *shape: torch.empty(shape, dtype=torch.uint8, device="cuda")

        def secret(*shape):                 # little-endian, 0 < value < 2^248
            v = rnd(*shape, 32)
            v[..., 31] = 0
            v[..., 0] |= 1
            return v
        # ---- two signers per session: the whole chain once, checked, then timed call by call
        sk, k = secret(2 * n), secret(4 * n)                       # signer j of session i at 2 i + j; its k_1, k_2 at 2 (2 i + j), + 1
        pkx, pky, _e, bad = ctx.ecdsa_public_key_batch(sk, curve=K1)
        kx, ky, _e, bad2 = ctx.ecdsa_public_key_batch(k, curve=K1)
        assert bad == 0 and bad2 == 0
        secnonce = k.reshape(2 * n, 64)
        pubnonce = torch.cat([kx.reshape(2 * n, 2, 32), ky.reshape(2 * n, 2, 32)], dim=2).reshape(2 * n, 128).contiguous()
        offsets = torch.arange(n + 1, dtype=torch.int64, device="cuda") * 2
        owner = (torch.arange(2 * n, dtype=torch.int32, device="cuda") // 2).contiguous()
        msg = rnd(n, 32)
        keyagg0, agg_pk0, err, bad = ctx.musig_key_agg_batch(pkx, pky, offsets)
        assert bad == 0
        keyagg, agg_pk, _e, bad = ctx.musig_apply_tweak_batch(keyagg0, None, p2e.MUSIG_TWEAK_TAPROOT)
        assert bad == 0
        aggnonce, _e, bad = ctx.musig_nonce_agg_batch(pubnonce, offsets)
        assert bad == 0
        session, _e, bad = ctx.musig_session_batch(keyagg, aggnonce, msg)
        assert bad == 0
        psig = buf(2 * n, 32)
        for j in range(2):
            part, _e, bad = ctx.musig_partial_sign_batch(secnonce[j::2].contiguous(), sk[j::2].contiguous(), keyagg, session)
            assert bad == 0
            psig[j::2] = part
        err2, valid, bad = ctx.musig_partial_verify_batch(psig, pubnonce, pkx, pky, keyagg, session, session_index=owner)
        assert bad == 0 and bool(valid.all())
        sig, _e, bad = ctx.musig_sig_agg_batch(psig, offsets, keyagg, session)
        assert bad == 0
        _e, ok, bad = ctx.schnorr_verify_batch(msg, agg_pk, sig)
        assert bad == 0 and bool(ok.all()), "a MuSig2 signature was refused by the BIP-340 verifier"

        o1, o2, o3, o4 = (buf(n, 32) for _ in range(4))
        rec_out, ses_out, agg_out, sig_out, par = buf(n, 192), buf(n, 128), buf(n, 128), buf(n, 64), buf(n)
        k_le = secret(n)
        ax, ay, bx, by = pkx[0::2].contiguous(), pky[0::2].contiguous(), pkx[1::2].contiguous(), pky[1::2].contiguous()
        sk0, sec0 = sk[0::2].contiguous(), secnonce[0::2].contiguous()
        mul = rounds(lambda: ctx.point_mul_batch(k_le, ax, ay, curve=K1, plan=p2e.MUL_PLAN_GLV, outx=o1, outy=o2, err=err))
        add = rounds(lambda: ctx.point_add_batch(ax, ay, bx, by, curve=K1, outx=o3, outy=o4, err=err))
        lin = rounds(lambda: ctx.point_lincomb_batch(k_le, k_le, ax, ay, curve=K1, outx=o3, outy=o4, err=err))
        pub = rounds(lambda: ctx.ecdsa_public_key_batch(sk0, curve=K1, pkx=o3, pky=o4, err=err))
        common = {"log2_n": lg, "point_mul_glv_ms": mul["ms"], "point_mul_glv_spread": mul["spread"]}

        ka2 = rounds(lambda: ctx.musig_key_agg_batch(pkx, pky, offsets, keyagg=rec_out, agg_pk=o3, err=err))
        emit(dict(common, section="key_agg2", signers=2, key_agg_ms=ka2["ms"], key_agg_spread=ka2["spread"], sessions_per_s=rate(n, ka2),
                  point_add_ms=add["ms"], point_add_spread=add["spread"], key_agg_over_mul_add=round(mean(ka2) / (mean(mul) + mean(add)), 4)))

        ses = rounds(lambda: ctx.musig_session_batch(keyagg, aggnonce, msg, session=ses_out, err=err))
        emit(dict(common, section="session", session_ms=ses["ms"], session_spread=ses["spread"], sessions_per_s=rate(n, ses),
                  point_add_ms=add["ms"], session_over_mul_add=round(mean(ses) / (mean(mul) + mean(add)), 4)))

        p0, n0 = psig[0::2].contiguous(), pubnonce[0::2].contiguous()
        ver = rounds(lambda: ctx.musig_partial_verify_batch(p0, n0, ax, ay, keyagg, session, err=err, valid=par))
        emit(dict(common, section="verify", verify_ms=ver["ms"], verify_spread=ver["spread"], signatures_per_s=rate(n, ver),
                  point_lincomb_ms=lin["ms"], point_lincomb_spread=lin["spread"], verify_over_mul_lincomb=round(mean(ver) / (mean(mul) + mean(lin)), 4)))

        sgn = rounds(lambda: ctx.musig_partial_sign_batch(sec0, sk0, keyagg, session, psig=o3, err=err))
        emit(dict(common, section="sign", sign_ms=sgn["ms"], sign_spread=sgn["spread"], signatures_per_s=rate(n, sgn),
                  public_key_ms=pub["ms"], public_key_spread=pub["spread"], sign_over_public_key_mul=round(mean(sgn) / (mean(pub) + mean(mul)), 4),
                  sign_over_public_key=round(mean(sgn) / mean(pub), 4)))

        twk = rounds(lambda: ctx.musig_apply_tweak_batch(keyagg0, None, p2e.MUSIG_TWEAK_TAPROOT, keyagg_out=rec_out, agg_pk=o3, err=err))
        tap = rounds(lambda: ctx.taproot_tweak_pubkey_batch(agg_pk0, None, out_pk=o3, out_parity=par, err=err))
        nag = rounds(lambda: ctx.musig_nonce_agg_batch(pubnonce, offsets, aggnonce=agg_out, err=err))
        sag = rounds(lambda: ctx.musig_sig_agg_batch(psig, offsets, keyagg, session, sig=sig_out, err=err))
        emit({"section": "light", "log2_n": lg, "apply_tweak_taproot_ms": twk["ms"], "apply_tweak_spread": twk["spread"],
              "taproot_tweak_pubkey_ms": tap["ms"], "taproot_tweak_pubkey_spread": tap["spread"],
              "apply_tweak_over_taproot_tweak_pubkey": round(mean(twk) / mean(tap), 4), "nonce_agg2_ms": nag["ms"], "nonce_agg2_spread": nag["spread"],
              "sig_agg2_ms": sag["ms"], "sig_agg2_spread": sag["spread"]})
        del sk, k, kx, ky, secnonce, pubnonce, psig

        # ---- sixteen signers per session
        m = min(n, 1 << 18)
        sk16 = secret(16 * m)
        x16, y16, _e, bad = ctx.ecdsa_public_key_batch(sk16, curve=K1)
        assert bad == 0
        off16 = torch.arange(m + 1, dtype=torch.int64, device="cuda") * 16
        e16 = buf(m)
        ka16 = rounds(lambda: ctx.musig_key_agg_batch(x16, y16, off16, keyagg=rec_out[:m], agg_pk=o3[:m], err=e16))
        mul16 = rounds(lambda: ctx.point_mul_batch(k_le[:m], ax[:m], ay[:m], curve=K1, plan=p2e.MUL_PLAN_GLV, outx=o1[:m], outy=o2[:m], err=e16))
        emit({"section": "key_agg16", "log2_n": lg, "log2_sessions": m.bit_length() - 1, "signers": 16, "key_agg_ms": ka16["ms"],
              "key_agg_spread": ka16["spread"], "sessions_per_s": rate(m, ka16), "point_mul_glv_ms": mul16["ms"], "point_mul_glv_spread": mul16["spread"],
              "key_agg_over_15_mul": round(mean(ka16) / (15 * mean(mul16)), 4)})
        del sk16, x16, y16
