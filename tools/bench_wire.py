"""The key and signature codecs (include/p2e.h p2e_point_decode_batch, p2e_point_encode_batch, p2e_sig_decode_batch,
p2e_sig_encode_batch): time per call.

Keys are made on the device by p2e_ecdsa_public_key_batch from random secret keys and encoded by the library; signatures
are made by p2e_ecdsa_sign_recoverable_batch and encoded by the library, the DER batch packed on the device without padding
(the signer's natural length mix: 70, 71 and 72 bytes for almost all).  Inputs and outputs stay on the device.  A figure
is the median of REPS (default 21) timed calls after WARMUP (3), measured with HIP events on the caller's stream around the
call alone; every point runs ROUNDS (2) times and `spread` is the relative difference between the repeated medians.
Sections (one JSON line per point, both curves, n = 2^16 and 2^20):
  point_decode   all keys compressed, all keys uncompressed
  point_encode   both forms
  sig_decode     DER, r || s, r || s || v, without flags and with P2E_SIG_NORMALIZE_S
  sig_encode     the same forms
  bar            p2e_ecdsa_recover_batch on 2^20 elements against p2e_point_decode_batch on 2^20 compressed keys, same process
usage: python tools/bench_wire.py [out.jsonl] [section ...]   (default profiles/wire_batch.jsonl, all sections)
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
out_path = args.pop(0) if args and args[0].endswith(".jsonl") else os.path.join(ROOT, "profiles", "wire_batch.jsonl")
sections = args or ["point_decode", "point_encode", "sig_decode", "sig_encode", "bar"]
REPS, WARMUP, ROUNDS = int(os.environ.get("REPS", "21")), int(os.environ.get("WARMUP", "3")), int(os.environ.get("ROUNDS", "2"))
BIG = int(os.environ.get("LOG2_BIG", "20"))
SIZES = sorted({min(16, BIG), BIG})
box = torch.cuda.get_device_name(0)
ctx = p2e.Context(device=0)
CURVES = ((p2e.CURVE_SECP256K1, "secp256k1"), (p2e.CURVE_P256, "p256"))
POINT_FORMS = ((p2e.SEC1_COMPRESSED, "compressed", 33), (p2e.SEC1_UNCOMPRESSED, "uncompressed", 65))
SIG_FORMS = ((p2e.SIG_DER, "der"), (p2e.SIG_COMPACT64, "compact64"), (p2e.SIG_COMPACT65, "compact65"))


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


def u8(*shape):
    return torch.empty(shape, dtype=torch.uint8, device="cuda")


_inputs = {}


def inputs(curve):
    """per curve, at the largest size: keys (pkx, pky) and recoverable signatures (msg, r, s, v), all on the device"""
    if curve not in _inputs:
        n = 1 << BIG
        gen = torch.Generator(device="cuda").manual_seed(5000 + curve)
        sk, msg, nonce = [torch.randint(0, 256, (n, 32), dtype=torch.uint8, device="cuda", generator=gen) for _ in range(3)]
        pkx, pky, _err, bad = ctx.ecdsa_public_key_batch(sk, curve=curve)
        r, s, v, _err, bad2 = ctx.ecdsa_sign_recoverable_batch(msg, sk, nonce, curve=curve)
        assert bad == 0 and bad2 == 0
        _inputs[curve] = dict(pkx=pkx, pky=pky, msg=msg, r=r, s=s, v=v)
    return _inputs[curve]


def packed_der(curve, n):
    """(data, offsets, lengths histogram) of the first n signatures as one DER buffer without padding, built on the device"""
    d = inputs(curve)
    out, out_len, _err, bad = ctx.sig_encode_batch(d["r"][:n], d["s"][:n], curve=curve, form=p2e.SIG_DER)
    assert bad == 0
    lens = out_len.to(torch.int64)
    offsets = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    offsets[1:] = torch.cumsum(lens, 0)
    keep = torch.arange(72, device="cuda")[None, :] < lens[:, None]
    data = torch.cat([out[keep], torch.zeros(4, dtype=torch.uint8, device="cuda")])   # row-major: the encodings in order
    hist = {int(k): int(c) for k, c in zip(*torch.unique(lens, return_counts=True))}
    return data, offsets, hist


with open(out_path, "a") as out_file:
    def emit(rec):
        line = json.dumps(dict({"box": box, "reps": REPS}, **rec))
        print(line, flush=True)
        out_file.write(line + "\n")
        out_file.flush()

    for curve, cname in CURVES:
        d = inputs(curve)
        for lg in SIZES:
            n = 1 << lg
            pkx, pky, r, s, v = d["pkx"][:n], d["pky"][:n], d["r"][:n], d["s"][:n], d["v"][:n]
            err = u8(n)
            for form, fname, stride in POINT_FORMS:
                wire, _e, bad = ctx.point_encode_batch(pkx, pky, curve=curve, form=form)
                assert bad == 0
                if "point_encode" in sections:
                    emit(dict({"section": "point_encode", "curve": cname, "log2_n": lg, "form": fname},
                              **rounds(lambda: ctx.point_encode_batch(pkx, pky, curve=curve, form=form, out=wire, err=err))))
                if "point_decode" in sections:
                    offsets = torch.arange(n + 1, dtype=torch.int64, device="cuda") * stride
                    ox, oy = u8(n, 32), u8(n, 32)
                    fn = lambda: ctx.point_decode_batch(wire.view(-1), offsets, curve=curve, px=ox, py=oy, err=err)
                    assert fn()[3] == 0 and torch.equal(ox, pkx) and torch.equal(oy, pky)
                    emit(dict({"section": "point_decode", "curve": cname, "log2_n": lg, "form": fname}, **rounds(fn)))
            for form, fname in SIG_FORMS:
                for flags, flname in ((0, "none"), (p2e.SIG_NORMALIZE_S, "normalize_s")):
                    if form == p2e.SIG_DER:
                        wire, offsets, hist = packed_der(curve, n)
                        extra = {"der_lengths": hist}
                    else:
                        wire, _l, _e, bad = ctx.sig_encode_batch(r, s, v, curve=curve, form=form)
                        offsets, extra = None, {}
                    if "sig_decode" in sections:
                        orr, os_, ov = u8(n, 32), u8(n, 32), u8(n)
                        fn = lambda: ctx.sig_decode_batch(wire, offsets, curve=curve, form=form, flags=flags, n=n, r=orr, s=os_, v=ov, err=err)
                        assert fn()[4] == 0 and torch.equal(orr, r) and (flags or torch.equal(os_, s))
                        emit(dict({"section": "sig_decode", "curve": cname, "log2_n": lg, "form": fname, "flags": flname}, **extra, **rounds(fn)))
                    if "sig_encode" in sections:
                        eout = u8(n, {p2e.SIG_DER: 72, p2e.SIG_COMPACT64: 64}.get(form, 65))
                        elen = u8(n)
                        fn = lambda: ctx.sig_encode_batch(r, s, v, curve=curve, form=form, flags=flags, out=eout, out_len=elen, err=err)
                        assert fn()[3] == 0
                        emit(dict({"section": "sig_encode", "curve": cname, "log2_n": lg, "form": fname, "flags": flname}, **rounds(fn)))
        if "bar" in sections:
            n = 1 << BIG
            wire, _e, bad = ctx.point_encode_batch(d["pkx"], d["pky"], curve=curve, form=p2e.SEC1_COMPRESSED)
            offsets = torch.arange(n + 1, dtype=torch.int64, device="cuda") * 33
            ox, oy, rx, ry, err = u8(n, 32), u8(n, 32), u8(n, 32), u8(n, 32), u8(n)
            rec = rounds(lambda: ctx.ecdsa_recover_batch(d["msg"], d["r"], d["s"], d["v"], curve=curve, pkx=rx, pky=ry, err=err))
            dec = rounds(lambda: ctx.point_decode_batch(wire.view(-1), offsets, curve=curve, px=ox, py=oy, err=err))
            torch.cuda.synchronize()
            assert torch.equal(ox, d["pkx"]) and torch.equal(oy, d["pky"]) and torch.equal(rx, d["pkx"])
            ratio = statistics.mean(dec["ms"]) / statistics.mean(rec["ms"])
            emit({"section": "bar", "curve": cname, "log2_n": BIG, "recover_ms": rec["ms"], "recover_spread": rec["spread"],
                  "point_decode_compressed_ms": dec["ms"], "point_decode_spread": dec["spread"], "decode_over_recover": round(ratio, 4),
                  "decode_faster": ratio < 1.0})
