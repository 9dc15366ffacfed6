"""The host-pointer path of every per-element call against its device-pointer path.

A P2E_CTX_HOST_POINTERS context copies every buffer of a call to the device and every output back; how many bytes, it takes
from the call's one buffer list (csrc/call_args.hpp), the list the overlap check reads too.  Here every form of every call in
tests/test_overlap_cpu.py's CALLS runs twice on the same input bytes at n = 5, once per kind of context:
  - the return values are equal and every output is byte for byte the same;
  - on the host side every output lies in one numpy arena with 64 guard bytes behind it, and no guard byte changes (a copy
    back longer than the buffer would land there); no input changes either.
The inputs are a chain: keys come from random secret keys, signatures from those keys, wire forms from the encoders, so that
most elements are valid and some are flagged in every call (secret key 0, a table index past the table, a zero-length
encoding, a corrupted signature).  What the outputs must BE is the business of the other GPU tests; this file holds the two
paths against each other.  Variable-length data starts at offsets[0] = 7 with element lengths 0 .. 80."""
import ctypes as C

import numpy as np
import pytest
import torch

import hash_inputs as H
import plonky2_ecdsa_amd as p2e
from test_overlap_cpu import CALLS, per_element_calls

pytestmark = pytest.mark.gpu

N, M = 5, 2
GUARD, FILL, PATTERN = 64, 0xAA, 0x5C
HANDLES = ("table", "prog")          # the "free" arguments that are no data


@pytest.fixture(scope="module")
def world():
    ctxs = {"device": p2e.Context(device=0), "host": p2e.Context(device=0, host_pointers=True)}
    cv = H.CURVES[1]
    progs = {m: p2e.CurveProgram(c, p2e.CP_VERIFY, p2e.CURVE_P256, blind=cv.mul(0xB11D, cv.g)) for m, c in ctxs.items()}
    w = dict(ctx=ctxs, prog={m: p._h.value for m, p in progs.items()}, table={}, seen=set(), params=per_element_calls())
    yield w
    for m, t in w["table"].items():
        p2e.lib().p2e_point_table_destroy(ctxs[m]._h, t)
    for p in progs.values():
        p.close()
    for c in ctxs.values():
        c.close()


def both(w, name, form, inputs, n=N, n_parents=None):
    """One form of one call on both contexts.  inputs: parameter name -> uint8 array.  -> (rc, {output name: bytes}) of the
    device-pointer run, after the comparison with the host-pointer run."""
    row, pnames = CALLS[name][form], [p for _t, p in w["params"][name]]
    w["seen"].add((name, form))
    count = lambda spec: {"n": n, "n+1": n + 1, 1: 1}[spec[2]]
    runs = {}
    for mode in ("device", "host"):
        out_bytes = [(k, spec[1] * count(spec)) for k, spec in enumerate(row) if isinstance(spec, tuple) and spec[0] == "out"]
        arena = np.full(sum(b + GUARD for _k, b in out_bytes) + GUARD, PATTERN, np.uint8)
        args, ins, outs, at, slot = [w["ctx"][mode]._h], {}, {}, GUARD, C.c_void_p()
        for k, spec in enumerate(row):
            pname = pnames[k]
            if not isinstance(spec, tuple):
                args.append(C.c_size_t(spec) if pname == "seed_len" else spec)
            elif spec[0] in ("n", "np"):
                args.append(C.c_size_t(n if spec[0] == "n" else n_parents))
            elif spec[0] == "off":
                args.append(None)
            elif spec[0] == "slot":
                args.append(C.byref(slot))
            elif spec[0] == "free" and pname in HANDLES:
                args.append(C.c_void_p(w[pname][mode]))
            elif spec[0] == "out":
                b = spec[1] * count(spec)
                if mode == "host":
                    outs[pname] = arena[at:at + b]
                    outs[pname][:] = FILL
                    at += b + GUARD
                else:
                    outs[pname] = torch.full((b,), FILL, dtype=torch.uint8, device="cuda")
                args.append(p2e._ptr(outs[pname]))
            else:
                a = np.ascontiguousarray(inputs[pname]).view(np.uint8).reshape(-1)
                if spec[0] != "free":
                    assert a.size == spec[1] * (n_parents if spec[0] == "bcast" else count(spec)), (name, pname, a.size)
                ins[pname] = a.copy() if mode == "host" else torch.from_numpy(a.copy()).cuda()
                args.append(p2e._ptr(ins[pname]))
        rc = getattr(p2e.lib(), name)(*args)
        torch.cuda.synchronize()
        assert rc >= 0, (name, form, mode, rc, p2e.lib().p2e_last_error().decode())
        if mode == "host":
            kept = np.ones(arena.size, bool)
            for v in outs.values():
                lo = v.ctypes.data - arena.ctypes.data
                kept[lo:lo + v.size] = False
            assert (arena[kept] == PATTERN).all(), (name, form, "a guard byte changed")
            assert all(np.array_equal(v, np.ascontiguousarray(inputs[p]).view(np.uint8).reshape(-1)) for p, v in ins.items()), (name, form)
            got = {p: v.copy() for p, v in outs.items()}
        else:
            got = {p: v.cpu().numpy() for p, v in outs.items()}
        if slot.value:
            w["table"][mode] = slot.value
        runs[mode] = (rc, got)
    (rc, dev), (rc_host, host) = runs["device"], runs["host"]
    assert rc == rc_host, (name, form, rc, rc_host)
    for p in dev:
        diff = np.nonzero(dev[p] != host[p])[0]
        assert diff.size == 0, (name, form, p, "first differing bytes", diff[:8].tolist())
    return rc, dev


def var_data(rng, elements):
    """(data, offsets) of variable-length elements behind 7 bytes that belong to no element"""
    lead = rng.integers(0, 256, 7, dtype=np.uint8)
    offsets = np.cumsum([lead.size] + [len(e) for e in elements]).astype(np.uint64)
    return np.concatenate([lead] + [np.asarray(e, np.uint8) for e in elements]), offsets


def test_every_call_gives_the_same_bytes_through_host_and_device_pointers(world):
    w, rng = world, np.random.default_rng(0x57A6ED)
    rand = lambda *shape: rng.integers(0, 256, shape, dtype=np.uint8)

    def scalars(n=N):                               # little-endian, below 2^248: in range on both curves
        a = rand(n, 32)
        a[:, 31] = 0
        return a

    sk, k, a32, b32, msg, aux = scalars(), scalars(), scalars(), scalars(), rand(N, 32), rand(N, 32)
    sk[0] = 0                                       # no key: flagged wherever it is used
    flagged = {}

    def run(name, inputs, form=0, **kw):
        rc, out = both(w, name, form, inputs, **kw)
        flagged[(name, form)] = rc
        return out

    # ECDSA keys, signatures, recovery, hashing
    pk = run("p2e_ecdsa_public_key_batch", {"sk32": sk})
    pkx, pky = pk["pkx32"].reshape(N, 32), pk["pky32"].reshape(N, 32)
    sig = run("p2e_ecdsa_sign_batch", {"msg32": msg, "sk32": sk, "k32": k})
    rec = run("p2e_ecdsa_sign_recoverable_batch", {"msg32": msg, "sk32": sk, "k32": k})
    run("p2e_ecdsa_recover_batch", {"msg32": msg, "r32": rec["r32"], "s32": rec["s32"], "v": rec["v"]})
    data, offsets = var_data(rng, [rand(l) for l in (0, 80, 1, 55, 64)])
    assert offsets[0] > 0
    run("p2e_hash_batch", {"data": data, "offsets": offsets})
    run("p2e_hash160_batch", {"data": data, "offsets": offsets})
    run("p2e_ecdsa_nonce_rfc6979_batch", {"msg32": msg, "sk32": sk})
    run("p2e_ecdsa_sign_deterministic_batch", {"msg32": msg, "sk32": sk})
    run("p2e_eth_address_batch", {"pkx32": pkx, "pky32": pky, "err": pk["err"]})
    run("p2e_key_hash160_batch", {"pkx32": pkx, "pky32": pky, "err_in": pk["err"]})
    good = list(p2e.synth_signatures(seed=11, n=N))
    good[2][3] ^= 1                                 # one signature that does not verify
    run("p2e_ecdsa_verify_batch", dict(zip(("msg32", "r32", "s32", "pkx32", "pky32"), good)))
    good = list(p2e.synth_signatures_curve(p2e.CURVE_P256, seed=12, n=N))
    good[1][2] ^= 1
    run("p2e_p256_verify_batch", dict(zip(("msg32", "r32", "s32", "pkx32", "pky32"), good)))

    # wire forms: what the encoders wrote is what the decoders read
    sec1 = [run("p2e_point_encode_batch", {"px32": pkx, "py32": pky}, form=f)["out"] for f in (0, 1)]
    c33, c65 = sec1[0].reshape(N, 33), sec1[1].reshape(N, 65)
    data, offsets = var_data(rng, [c33[1], c65[2], [], c33[3], c65[4]])
    run("p2e_point_decode_batch", {"data": data, "offsets": offsets})
    enc = [run("p2e_sig_encode_batch", {"r32": sig["r32"], "s32": sig["s32"], "v": rec["v"]}, form=f) for f in (0, 1, 2)]
    der, der_len = enc[0]["out"].reshape(N, 72), enc[0]["out_len"]
    data, offsets = var_data(rng, [der[i][:der_len[i]] for i in range(N)])
    run("p2e_sig_decode_batch", {"data": data, "offsets": offsets}, form=0)
    run("p2e_sig_decode_batch", {"data": enc[1]["out"]}, form=1)
    run("p2e_sig_decode_batch", {"data": enc[2]["out"]}, form=2)

    # point arithmetic, the sum, the tables
    run("p2e_point_msm", {"k32": k, "px32": pkx, "py32": pky})
    run("p2e_point_mul_batch", {"k32": k, "px32": pkx, "py32": pky})
    run("p2e_point_lincomb_batch", {"a32": a32, "b32": b32, "px32": pkx, "py32": pky})
    run("p2e_point_add_batch", {"px32": pkx, "py32": pky, "qx32": np.roll(pkx, 1, axis=0), "qy32": np.roll(pky, 1, axis=0)})
    run("p2e_point_table_create", {"px32": pkx[1:1 + M], "py32": pky[1:1 + M]}, n=M)
    assert set(w["table"]) == {"device", "host"}
    idx = np.array([0, 0, 1, 0, M], np.uint32)      # elements 1 and 2 meet their own keys; the last index is past the table
    run("p2e_point_table_mul_batch", {"idx": idx, "k32": k})
    run("p2e_point_table_lincomb_batch", {"idx": idx, "a32": a32, "b32": b32})
    run("p2e_ecdsa_verify_table_batch", {"idx": idx, "msg32": msg, "r32": sig["r32"], "s32": sig["s32"]})

    # BIP-340
    xpk = run("p2e_schnorr_public_key_batch", {"sk32": sk})["pk32"]
    ssig = run("p2e_schnorr_sign_batch", {"msg32": msg, "sk32": sk, "aux32": aux})["sig64"]
    run("p2e_schnorr_verify_batch", {"msg32": msg, "pk32": xpk, "sig64": ssig})
    run("p2e_xonly_decode_batch", {"pk32": xpk})
    run("p2e_schnorr_verify_aggregate", {"msg32": msg, "pk32": xpk, "sig64": ssig, "seed32": rand(32)})

    # BIP-32: one parent for all children, and one each
    master = [run("p2e_bip32_master_batch", {"seed": rand(N, l)}, form=f) for f, l in ((0, 32), (1, 63))][0]
    index = (rng.integers(0, 1 << 31, N, dtype=np.uint32) | np.array([0, 1 << 31, 0, 0, 0], np.uint32)).astype(np.uint32)
    for n_parents in (1, N):
        par = lambda a: np.ascontiguousarray(a).reshape(N, 32)[1:1 + n_parents] if n_parents == 1 else a
        run("p2e_bip32_ckd_priv_batch", {"par_sk32": par(master["sk32"]), "par_cc32": par(master["cc32"]), "index": index},
            n_parents=n_parents)
        run("p2e_bip32_ckd_pub_batch", {"par_pkx32": par(pkx), "par_pky32": par(pky), "par_cc32": par(master["cc32"]), "index": index},
            n_parents=n_parents)

    assert w["seen"] == {(name, f) for name, forms in CALLS.items() for f in range(len(forms))}
    # the chain holds what it is meant to: valid elements and flagged ones in the calls that count them
    assert 0 < flagged[("p2e_ecdsa_public_key_batch", 0)] < N and 0 < flagged[("p2e_ecdsa_verify_table_batch", 0)] < N
    assert 0 < flagged[("p2e_point_decode_batch", 0)] < N and flagged[("p2e_point_table_create", 0)] == 0
