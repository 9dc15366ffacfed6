"""BIP-39 seed derivation (include/p2e.h p2e_bip39_seed_batch): seeds per second, against three yardsticks.

The method of MEASUREMENTS.md section 17, as tools/bench_hd.py applies it: inputs are made once and stay on the device; a
figure is the median of REPS (default 11) timed calls after WARMUP (2), measured with HIP events on the caller's stream around
the call alone; every point runs ROUNDS (2) times and `spread` is the relative difference between the repeated medians.  One
process on the GPU.  Before anything is timed the library and the plain probe kernel are compared on the whole batch, and
four elements with hashlib.
Points: count = 2^12, 2^16, 2^18 x sentences of 12 words (at most 128 bytes: the key is used as it is) and of 24 words (more
than 128 bytes: the key is hashed first) x one passphrase for the batch and one per element.  Beside the measured rate:
  plain     tests/probe_kdf's kernel on the same inputs: the same PBKDF2 with hd.hpp's unchanged sha512_compress.  `over_plain`
            is the library's rate over its rate: what the specialised loop of csrc/kdf.hpp buys.
  hashlib   hashlib.pbkdf2_hmac in 16 processes on this box for about a second each (seeds per second, summed), taken before
            the GPU is opened.
  bound     the VALU issue bound: lanes x clock / (VALU instructions of one trip of the hot loop x 4 094 trips), one wave64
            VALU instruction per 2 cycles per SIMD-32 (tools/kdf_loop_count.py counts the trip in the built library's ISA
            listing).  `of_bound` is the measured rate over it.
usage: python tools/bench_kdf.py [out.jsonl]   (default profiles/kdf.jsonl; appended to)"""
import ctypes as C
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

args = sys.argv[1:]
out_path = args.pop(0) if args and args[0].endswith(".jsonl") else os.path.join(ROOT, "profiles", "kdf.jsonl")
REPS, WARMUP, ROUNDS = int(os.environ.get("REPS", "11")), int(os.environ.get("WARMUP", "2")), int(os.environ.get("ROUNDS", "2"))
SIZES = [int(v) for v in os.environ.get("LOG2_SIZES", "12,16,18").split(",")]
HOST_PROCS = 16
WORDS = ("abandon", "ability", "about", "above", "absent", "absorb", "abstract", "absurd")   # 5 .. 8 letters


def hashlib_rate():
    """seeds per second of hashlib.pbkdf2_hmac over HOST_PROCS processes, each running for about a second"""
    code = ("import hashlib, time\n"
            "m = b'abandon ability about above absent absorb abstract absurd abandon ability about above'\n"
            "t0 = time.perf_counter(); k = 0\n"
            "while time.perf_counter() - t0 < 1.0:\n"
            "    hashlib.pbkdf2_hmac('sha512', m, b'mnemonic%d' % k, 2048, 64); k += 1\n"
            "print(k / (time.perf_counter() - t0))\n")
    procs = [subprocess.Popen([sys.executable, "-c", code], stdout=subprocess.PIPE, text=True) for _ in range(HOST_PROCS)]
    return sum(float(p.communicate()[0]) for p in procs)


host_rate = hashlib_rate()                       # before the GPU is opened: the children never see it

import numpy as np
import torch
import plonky2_ecdsa_amd as p2e

try:
    import kdf_loop_count
    loops = kdf_loop_count.hot_loops(kdf_loop_count.listing(os.path.join(ROOT, "plonky2-ecdsa_amd", "libp2e_hip.so")))
    valu_per_trip = [v[0] for name, v in loops.items() if "ILi8E" in name][0]
    bound = kdf_loop_count.issue_bound(valu_per_trip)
except Exception as e:                           # no listing tool on this box: the bound is then not stated
    print(f"# VALU issue bound NOT MEASURED: {e}", file=sys.stderr)
    valu_per_trip, bound = None, None

probe_dir = os.path.join(ROOT, "tests", "probe_kdf")
if not os.path.exists(os.path.join(probe_dir, "libp2e_probe_kdf.so")):
    subprocess.check_call(["make", "-s", "-C", probe_dir])
PROBE = C.CDLL(os.path.join(probe_dir, "libp2e_probe_kdf.so"))
PROBE.probekdf_pbkdf2.restype = C.c_long

box = torch.cuda.get_device_name(0)
ctx = p2e.Context(device=0)
stream = torch.cuda.current_stream(0).cuda_stream


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


def sentences(n, words, seed):
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, len(WORDS), (n, words))
    return [" ".join(WORDS[k] for k in row).encode() for row in pick]


def upload(items):
    buf, off = p2e.pack_bytes(items)
    return torch.from_numpy(buf).cuda(), torch.from_numpy(off.view(np.int64)).cuda()


ptr = lambda t: C.c_void_p(t.data_ptr())

with open(out_path, "a") as out:
    def emit(rec):
        line = json.dumps(dict({"box": box, "reps": REPS}, **rec))
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    for lg in SIZES:
        n = 1 << lg
        for words in (12, 24):
            mn_host = sentences(n, words, 39 * lg + words)
            assert all(len(m) <= 128 for m in mn_host) if words == 12 else all(len(m) > 128 for m in mn_host)
            mn, mn_off = upload(mn_host)
            for per_element in (False, True):
                pp_host = [f"passphrase-{i}".encode() for i in range(n)] if per_element else [b"TREZOR"]
                pp, pp_off = upload(pp_host)
                n_pp = len(pp_host)
                seed = torch.empty((n, 64), dtype=torch.uint8, device="cuda")
                err = torch.empty(n, dtype=torch.uint8, device="cuda")
                plain, perr = torch.empty_like(seed), torch.empty_like(err)

                def lib_call():
                    ctx.bip39_seed_batch((mn, mn_off), (pp, pp_off), seed=seed, err=err)

                def probe_call():
                    rc = PROBE.probekdf_pbkdf2(C.c_int(1), ptr(mn), ptr(mn_off), C.c_size_t(n), ptr(pp), ptr(pp_off), C.c_size_t(n_pp),
                                               C.c_uint32(2048), C.c_size_t(64), ptr(plain), C.c_size_t(n), ptr(perr), C.c_void_p(stream))
                    assert rc == 0

                lib_call(), probe_call()
                torch.cuda.synchronize()
                assert torch.equal(seed, plain) and not err.any() and not perr.any()
                for i in (0, 1, n // 2, n - 1):
                    want = hashlib.pbkdf2_hmac("sha512", mn_host[i], b"mnemonic" + pp_host[i if per_element else 0], 2048, 64)
                    assert bytes(seed[i].cpu().numpy()) == want, i
                lib, prb = rounds(lib_call), rounds(probe_call)
                rate = n / (statistics.mean(lib["ms"]) * 1e-3)
                plain_rate = n / (statistics.mean(prb["ms"]) * 1e-3)
                emit({"section": "bip39_seed", "log2_n": lg, "words": words, "passphrases": "one per element" if per_element else "one",
                      "ms": lib["ms"], "spread": lib["spread"], "seeds_per_s": round(rate), "plain_ms": prb["ms"], "plain_spread": prb["spread"],
                      "plain_seeds_per_s": round(plain_rate), "over_plain": round(rate / plain_rate, 4),
                      "hashlib_16_procs_seeds_per_s": round(host_rate), "over_hashlib": round(rate / host_rate, 1),
                      "valu_per_trip": valu_per_trip, "issue_bound_seeds_per_s": round(bound) if bound else "NOT MEASURED",
                      "of_bound": round(rate / bound, 4) if bound else "NOT MEASURED"})
