"""MuSig2 on the GPU (include/p2e.h p2e_musig_key_agg_batch and the six calls after it) through the C ABI.

Expectations come from tests/musig_inputs.py alone: a restatement of BIP-327 in Python integers and hashlib, pinned by the
standard's key-aggregation vectors and by its own BIP-340 verifier (tests/test_musig_cpu.py).  Every byte of every element is
compared; output buffers are pre-filled with 0xAA so that an unwritten byte shows, and hold one element more than the call may
write; the return value is the number of flagged elements.

Shapes: every call at count = 0, 1, 63, 64, 65 and 257 (nothing, one lane, a wave less one, a wave, a wave plus one, a block
plus one) in host-pointer mode.  The first wave mixes sessions of 1, 2, 3 and 17 signers, the duplicate lists [A, A, A] and
[A, A, B, B], three sessions with a bad key and one without signers, so that its lanes diverge and a flag travels down the
chain.  What no hash produces -- a key sum at infinity, R_1 = -b R_2 -- runs with forced coefficients through tests/probe_musig
(built on demand with the library's flags).  The last test runs the whole chain on device pointers and hands every signature to
p2e_schnorr_verify_batch."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import plonky2_ecdsa_amd as p2e
import musig_inputs as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tests", "probe_musig")
CHAIN_SETS = ("key_agg", "apply_tweak", "apply_tweak/xonly", "apply_tweak/taproot", "nonce_agg", "session", "partial_sign", "partial_verify",
              "sig_agg")


@pytest.fixture(scope="module")
def hctx():
    return p2e.Context(device=0, host_pointers=True)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def run_set(hctx, call, inputs, want, count=None):
    count = len(want["err"]) if count is None else count
    ins, ref = M.cut(call, inputs, want, count)
    rc, outs = M.invoke(getattr(hctx._L, f"p2e_musig_{call}_batch"), call, ins, count, ctx=hctx._h)
    assert rc >= 0, p2e.lib().p2e_last_error()
    M.assert_matches(call, rc, outs, ref, count)
    return outs


# ---- every call against the oracle ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", M.COUNTS)
@pytest.mark.parametrize("name", CHAIN_SETS)
def test_call_equals_the_oracle_on_the_chain(name, count, hctx):
    inputs, want = M.chain_sets()[name]
    run_set(hctx, name.split("/")[0], inputs, want, count)
    if count == 257:       # three bad keys and an empty session, all in the first wave (the nonces of the bad keys' sessions are fine)
        assert np.count_nonzero(want["err"]) == {"partial_verify": 17 + 2 + 17, "nonce_agg": 1}.get(name, 4), name


@pytest.mark.parametrize("name", sorted(M.special_sets()))
def test_reachable_special_cases(name, hctx):
    """R = G, half an aggregate nonce at infinity, Q' at infinity, the edge scalars 0, n - 1, n, 2^256 - 1 as a tweak, a nonce, a key
    and a partial signature, bad keys and nonces, 1024 and 1025 signers, reversed offsets, an index out of range"""
    call, inputs, want = M.special_sets()[name]
    run_set(hctx, call, inputs, want)


def test_partial_verify_refuses_what_is_not_the_signers_signature(hctx):
    call, inputs, want = M.special_sets()["partial_verify"]
    outs = run_set(hctx, call, inputs, want)
    # [0] the signature itself; [1] one bit flipped; [2] against another signer's nonce; [3] against another session's records
    assert outs["valid"][:4, 0].tolist() == [1, 0, 0, 0] and not outs["err"][:4].any()
    assert outs["err"][4:6, 0].tolist() == [M.WIRE_BAD_INDEX] * 2


def test_the_tweak_in_place(hctx):
    inputs, want = M.chain_sets()["apply_tweak/xonly"]
    n = 65
    rec, pk, err = inputs["keyagg192_in"][:n].copy(), np.full((n, 32), 0xAA, np.uint8), np.full(n, 0xAA, np.uint8)
    bad = hctx._L.p2e_musig_apply_tweak_batch(hctx._h, _p(rec), _p(inputs["tweak32"][:n].copy()), C.c_int(M.TWEAK_XONLY), _p(rec), _p(pk), C.c_size_t(n),
                                              _p(err))
    assert bad == np.count_nonzero(want["err"][:n]) and np.array_equal(rec, want["keyagg192_out"][:n]) and np.array_equal(pk, want["agg_pk32"][:n])


@pytest.mark.parametrize("with_root", [True, False])
def test_taproot_mode_is_the_taproot_call_on_the_aggregate_key(with_root, hctx):
    c = M.chain()
    n = 65
    recs = M.rows([r[1] for r in c["key_agg"]][:n], 192)
    agg_pk = M.rows([r[2] for r in c["key_agg"]][:n], 32)
    roots = M.rows(c["msg"][:n], 32) if with_root else None
    out_rec, out_pk, err, bad = hctx.musig_apply_tweak_batch(recs, roots, p2e.MUSIG_TWEAK_TAPROOT)
    tap_pk, tap_parity, tap_err, tap_bad = hctx.taproot_tweak_pubkey_batch(agg_pk, roots)
    good = err == 0
    assert bad == tap_bad == 4 and good.sum() == n - 4 and np.array_equal(tap_err != 0, ~good)
    assert np.array_equal(out_pk[good], tap_pk[good]) and np.array_equal(out_rec[good][:, 32] & 1, tap_parity[good])
    want = [M.apply_tweak(bytes(r), None if roots is None else bytes(t), M.TWEAK_TAPROOT) for r, t in zip(recs, roots if with_root else [None] * n)]
    assert np.array_equal(out_rec, M.rows([w[1] for w in want], 192))


# ---- what no hash produces --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe():
    lib = os.path.join(PROBE, "libp2e_probe_musig.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-s", "-C", PROBE])
    L = C.CDLL(lib)
    L.probemusig_forced_key_agg.restype = L.probemusig_forced_session.restype = C.c_long
    return L


def test_forced_coefficients_on_the_device(probe):
    """Q at infinity in the key aggregation (coefficients that cancel) and R_1 = -b R_2 in the session (R becomes G)"""
    (ka_in, ka_want), (se_in, se_want) = M.forced_sets()
    n = len(ka_want["code"])
    code, qx, qy = np.full(n, 0xAA, np.uint8), np.full((n, 32), 0xAA, np.uint8), np.full((n, 32), 0xAA, np.uint8)
    assert probe.probemusig_forced_key_agg(_p(ka_in["pkx32"]), _p(ka_in["pky32"]), _p(ka_in["coef32"]), _p(ka_in["key_offsets"]), _p(code), _p(qx),
                                           _p(qy), C.c_size_t(n)) == 0
    assert code.tolist() == ka_want["code"].tolist() == [M.WIRE_INFINITY, M.WIRE_INFINITY, 0]
    assert np.array_equal(qx, ka_want["qx32"]) and np.array_equal(qy, ka_want["qy32"])
    n = len(se_want["code"])
    code, ses = np.full(n, 0xAA, np.uint8), np.full((n, 128), 0xAA, np.uint8)
    assert probe.probemusig_forced_session(_p(se_in["keyagg192"]), _p(se_in["aggnonce128"]), _p(se_in["msg32"]), _p(se_in["b32"]), _p(code), _p(ses),
                                           C.c_size_t(n)) == 0
    assert not code.any() and np.array_equal(ses, se_want["session128"])
    assert bytes(ses[0, 64:96]) == M.b32(M.G[0])                      # R_1 = -b R_2: R = G


# ---- the chain on device pointers -------------------------------------------------------------------------------------------------
def test_round_trip_on_device_pointers():
    """calls 1 -> 2 -> 3 -> 4 -> 5 (once per signer) -> 6 -> 7 on device memory, public nonces from p2e_ecdsa_public_key_batch; every
    signature must be accepted by p2e_schnorr_verify_batch under the tweaked aggregate key"""
    c = M.chain()
    ctx = p2e.Context(device=0)
    pick = [i for i in M.good_sessions(c) if len(c["sks"][i]) in (1, 2, 3)][:96]
    n, widest = len(pick), 3
    assert {len(c["sks"][i]) for i in pick} == {1, 2, 3}
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    sks = [c["sks"][i] for i in pick]
    offsets_h = M.offsets_of(sks)
    offsets = dev(offsets_h.view(np.int64))
    sk = dev(M.rows([M.le(d) for d in M.flat(sks)], 32))
    k = dev(M.rows([M.le(v) for i in pick for pair in c["secnonces"][i] for v in pair], 32))            # k_1, k_2 per signer
    total = sk.shape[0]
    pkx, pky, _e, bad = ctx.ecdsa_public_key_batch(sk)
    assert bad == 0
    kx, ky, _e, bad = ctx.ecdsa_public_key_batch(k)
    assert bad == 0
    secnonce = k.reshape(total, 64)
    pubnonce = torch.cat([kx.reshape(total, 2, 32), ky.reshape(total, 2, 32)], dim=2).reshape(total, 128).contiguous()
    keyagg, agg_pk, _e, bad = ctx.musig_key_agg_batch(pkx, pky, offsets)
    assert bad == 0
    keyagg, agg_pk, _e, bad = ctx.musig_apply_tweak_batch(keyagg, dev(M.rows([c["tweak_a"][i] for i in pick], 32)), p2e.MUSIG_TWEAK_PLAIN)
    assert bad == 0
    keyagg, agg_pk, _e, bad = ctx.musig_apply_tweak_batch(keyagg, dev(M.rows([c["tweak_b"][i] for i in pick], 32)), p2e.MUSIG_TWEAK_XONLY, keyagg_out=keyagg)
    assert bad == 0
    aggnonce, _e, bad = ctx.musig_nonce_agg_batch(pubnonce, offsets)
    assert bad == 0
    msg = dev(M.rows([c["msg"][i] for i in pick], 32))
    session, _e, bad = ctx.musig_session_batch(keyagg, aggnonce, msg)
    assert bad == 0
    psig = torch.zeros((total, 32), dtype=torch.uint8, device="cuda")
    for j in range(widest):                                            # signer j of every session that has one
        who = [s for s in range(n) if len(sks[s]) > j]
        at = torch.tensor([int(offsets_h[s]) + j for s in who], device="cuda")
        rows_ = torch.tensor(who, device="cuda")
        part, _e, bad = ctx.musig_partial_sign_batch(secnonce[at].contiguous(), sk[at].contiguous(), keyagg[rows_].contiguous(),
                                                     session[rows_].contiguous())
        assert bad == 0
        psig[at] = part
    owner = dev(np.array([s for s in range(n) for _ in sks[s]], np.uint32).view(np.int32))
    err, valid, bad = ctx.musig_partial_verify_batch(psig, pubnonce, pkx, pky, keyagg, session, session_index=owner)
    assert bad == 0 and bool(valid.cpu().numpy().all())
    sig, _e, bad = ctx.musig_sig_agg_batch(psig, offsets, keyagg, session)
    assert bad == 0
    verr, ok, bad = ctx.schnorr_verify_batch(msg, agg_pk, sig)
    torch.cuda.synchronize()
    assert bad == 0 and bool(ok.cpu().numpy().all())
    # and they are the oracle's signatures under the oracle's keys
    assert np.array_equal(sig.cpu().numpy(), M.rows([c["sig_agg"][i][1] for i in pick], 64))
    assert np.array_equal(agg_pk.cpu().numpy(), M.rows([c["tweak_xonly"][i][2] for i in pick], 32))
