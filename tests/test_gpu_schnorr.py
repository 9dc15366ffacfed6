"""BIP-340 Schnorr signatures on the GPU (include/p2e.h p2e_schnorr_public_key_batch, p2e_schnorr_sign_batch,
p2e_schnorr_verify_batch, p2e_xonly_decode_batch, p2e_schnorr_verify_aggregate) through the C ABI.

Expectations come from tests/schnorr_inputs.py alone: a restatement of the standard in Python integers and hashlib.  Every
byte of every element is compared; output buffers are pre-filled with 0xAA so that an unwritten byte shows.

Shapes: the per-element calls at n = 1, 63, 64, 65 and 257 (one lane, a wave less one, a wave, a wave plus one, a block plus
one); the aggregate at n = 0, 1, 2, 65 and 1000 (no term but G's, 3 to 2001 terms, four blocks of partial sums)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import plonky2_ecdsa_amd as p2e
import schnorr_inputs as SI

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hctx():
    return p2e.Context(device=0, host_pointers=True)


def filled(*shape):
    return np.full(shape, 0xAA, np.uint8)


def seed_array(seed):
    return np.frombuffer(seed, np.uint8).copy()


@functools.lru_cache(maxsize=None)
def case_arrays(n, name):
    """(msg, pk, sig, expected verdict, expected err) of one aggregate case, computed once"""
    msgs, pks, sigs = SI.aggregate_cases(n)[name]
    verdict, errs = SI.aggregate_expected(msgs, pks, sigs)
    if n == 0:
        return np.zeros((1, 32), np.uint8), np.zeros((1, 32), np.uint8), np.zeros((1, 64), np.uint8), verdict, np.zeros(0, np.uint8)
    return SI.rows(list(msgs)), SI.rows(list(pks)), SI.rows(list(sigs), 64), verdict, np.array(errs, np.uint8)


@pytest.mark.parametrize("n", SI.LENGTHS)
def test_public_key_and_sign_equal_the_oracle(n, hctx):
    a = SI.signer_arrays()
    pk, err, bad = hctx.schnorr_public_key_batch(a["sk"][:n].copy(), pk=filled(n, 32), err=filled(n))
    assert np.array_equal(pk, a["pk"][:n]) and np.array_equal(err, a["pk_err"][:n]) and bad == np.count_nonzero(a["pk_err"][:n])
    sig, err, bad = hctx.schnorr_sign_batch(a["msg"][:n].copy(), a["sk"][:n].copy(), a["aux"][:n].copy(), sig=filled(n, 64), err=filled(n))
    diff = np.nonzero((sig != a["sig"][:n]).any(axis=1))[0]
    assert diff.size == 0, [(int(i), SI.signer_set()[i].kind) for i in diff[:8]]
    assert np.array_equal(err, a["err"][:n]) and bad == np.count_nonzero(a["err"][:n])
    if n > 5:
        assert sig[0].tobytes() == SI.KNOWN_SIG and pk[0].tobytes() == SI.KNOWN_PK and (sig[3:6] == 0).all() and (pk[3:6] == 0).all()


@pytest.mark.parametrize("n", SI.LENGTHS)
def test_verify_and_decode_equal_the_oracle(n, hctx):
    a = SI.verifier_arrays()
    msg, pk, sig = a["msg"][:n].copy(), a["pk"][:n].copy(), a["sig"][:n].copy()
    err, valid, bad = hctx.schnorr_verify_batch(msg, pk, sig, err=filled(n), valid=filled(n))
    diff = np.nonzero((err != a["err"][:n]) | (valid != a["valid"][:n]))[0]
    assert diff.size == 0, [(int(i), SI.verifier_set()[i].kind, int(err[i]), int(valid[i])) for i in diff[:8]]
    assert bad == np.count_nonzero(a["err"][:n])              # a well-formed wrong signature is not counted
    px, py, err, bad = hctx.xonly_decode_batch(pk, px=filled(n, 32), py=filled(n, 32), err=filled(n))
    assert np.array_equal(px, a["dx"][:n]) and np.array_equal(py, a["dy"][:n]) and np.array_equal(err, a["derr"][:n])
    assert bad == np.count_nonzero(a["derr"][:n])


def test_decoded_keys_feed_the_point_layer(hctx):
    """the bridge: Taproot's P + t G through point_lincomb_batch on decoded keys equals the oracle's sum"""
    a = SI.verifier_arrays()
    idx = [i for i in range(len(a["derr"])) if a["derr"][i] == 0][:64]
    pk = a["pk"][idx].copy()
    px, py, err, bad = hctx.xonly_decode_batch(pk)
    assert bad == 0
    t = [int.from_bytes(SI._rand("tweak", i), "big") % SI.N for i in range(len(idx))]
    one = np.tile(SI.le32(1), (len(idx), 1))
    outx, outy, err, bad = hctx.point_lincomb_batch(np.stack([SI.le32(v) for v in t]), one, px, py)
    assert bad == 0
    for j, i in enumerate(idx):
        Pt = SI.lift_x(int.from_bytes(pk[j].tobytes(), "big"))
        want = SI._affine(SI._jadd(SI._gmul(t[j]), (Pt[0], Pt[1], 1)))
        assert (int.from_bytes(outx[j].tobytes(), "little"), int.from_bytes(outy[j].tobytes(), "little")) == want


@pytest.mark.parametrize("window", [p2e.MSM_WINDOW_AUTO, SI.AGG_FORCED_WINDOW])
@pytest.mark.parametrize("seed", range(2))
@pytest.mark.parametrize("n", SI.AGG_SIZES)
def test_aggregate_verdicts_and_codes(n, seed, window, hctx):
    for name in SI.aggregate_cases(n):
        msg, pk, sig, want, want_err = case_arrays(n, name)
        verdict, err, bad = hctx.schnorr_verify_aggregate(msg, pk, sig, seed_array(SI.AGG_SEEDS[seed]), window_bits=window,
                                                          verdict=filled(1), err=filled(max(n, 1))[:n], n=n)
        assert int(verdict[0]) == want == (name == "all_valid"), (n, name, int(verdict[0]))
        assert np.array_equal(err, want_err) and bad == np.count_nonzero(want_err), (n, name)
        if name.startswith("err_"):
            assert np.count_nonzero(want_err) == 1 and want_err[n // 2] != 0


def test_aggregate_without_err_and_on_the_verifier_set(hctx):
    V = SI.verifier_arrays()
    errs = np.array([SI.aggregate_err(c.msg, c.pk, c.sig) for c in SI.verifier_set()], np.uint8)
    verdict, err, bad = hctx.schnorr_verify_aggregate(V["msg"].copy(), V["pk"].copy(), V["sig"].copy(), seed_array(SI.AGG_SEEDS[0]),
                                                      verdict=filled(1), err=filled(len(errs)))
    assert int(verdict[0]) == 0 and np.array_equal(err, errs) and bad == np.count_nonzero(errs) > 0
    msg, pk, sig, want, _ = case_arrays(65, "all_valid")
    verdict, err, bad = hctx.schnorr_verify_aggregate(msg, pk, sig, seed_array(SI.AGG_SEEDS[0]), verdict=filled(1), want_err=False)
    assert err is None and int(verdict[0]) == 1 and bad == 0


@pytest.mark.parametrize("name", ["all_valid", "bad_middle", "delta_pair"])
def test_every_window_width_gives_the_same_verdict(name, hctx):
    msg, pk, sig, want, want_err = case_arrays(65, name)
    got = []
    for c in range(p2e.MSM_WINDOW_MIN, p2e.MSM_WINDOW_MAX + 1):
        verdict, err, bad = hctx.schnorr_verify_aggregate(msg, pk, sig, seed_array(SI.AGG_SEEDS[1]), window_bits=c, verdict=filled(1))
        got.append(int(verdict[0]))
        assert np.array_equal(err, want_err)
    assert got == [want] * (p2e.MSM_WINDOW_MAX - p2e.MSM_WINDOW_MIN + 1)


def test_scratch_regrows_from_a_small_batch_to_a_larger_one():
    ctx = p2e.Context(device=0, host_pointers=True)          # a fresh context: its first aggregate call allocates
    seed = seed_array(SI.AGG_SEEDS[0])
    for n, name in ((2, "all_valid"), (1000, "all_valid"), (1000, "bad_last"), (65, "swapped_s"), (1000, "all_valid")):
        msg, pk, sig, want, want_err = case_arrays(n, name)
        verdict, err, bad = ctx.schnorr_verify_aggregate(msg, pk, sig, seed, verdict=filled(1))
        assert int(verdict[0]) == want and np.array_equal(err, want_err), (n, name)
    ctx.close()


def test_chain_stays_on_the_device():
    """sign -> verify -> aggregate at n = 1000 on device pointers in async mode: nothing visits the host in between"""
    n = 1000
    ctx = p2e.Context(device=0, asynchronous=True)
    rows = lambda label: torch.from_numpy(SI.rows([SI._rand(label, i) for i in range(n)])).cuda()
    msg, aux = rows("chain-msg"), rows("chain-aux")
    sk_host = SI.rows([SI.b32(int.from_bytes(SI._rand("chain-sk", i), "big") % (SI.N - 1) + 1) for i in range(n)])
    sk = torch.from_numpy(sk_host).cuda()
    seed = torch.from_numpy(seed_array(SI.AGG_SEEDS[1])).cuda()
    full = lambda *shape: torch.full(shape, 0xAA, dtype=torch.uint8, device="cuda:0")
    pk, e1, _ = ctx.schnorr_public_key_batch(sk, pk=full(n, 32), err=full(n))
    sig, e2, _ = ctx.schnorr_sign_batch(msg, sk, aux, sig=full(n, 64), err=full(n))
    e3, valid, _ = ctx.schnorr_verify_batch(msg, pk, sig, err=full(n), valid=full(n))
    verdict, e4, _ = ctx.schnorr_verify_aggregate(msg, pk, sig, seed, verdict=full(1), err=full(n))
    sig_bad = sig.clone()
    sig_bad[n - 1, 63] ^= 1
    verdict_bad, _, _ = ctx.schnorr_verify_aggregate(msg, pk, sig_bad, seed, verdict=full(1), err=full(n))
    assert ctx.sync() == 0                                  # the last call's flag count
    torch.cuda.synchronize()
    for e in (e1, e2, e3, e4):
        assert not e.cpu().numpy().any()
    assert (valid.cpu().numpy() == 1).all() and int(verdict.cpu()[0]) == 1 and int(verdict_bad.cpu()[0]) == 0
    # three of the thousand against the oracle
    for i in (0, 499, 999):
        want_err, want_sig = SI.sign(bytes(msg[i].cpu().numpy()), bytes(sk_host[i]), bytes(aux[i].cpu().numpy()))
        assert want_err == 0 and bytes(sig[i].cpu().numpy()) == want_sig
    ctx.close()


def test_empty_batch_and_refused_arguments(hctx):
    L, h = hctx._L, hctx._h
    buf = np.zeros(64, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    verdict = filled(1)
    assert L.p2e_schnorr_verify_aggregate(h, p(buf), p(buf), p(buf), C.c_size_t(0), p(buf), C.c_uint(0), p(verdict), None) == 0 and verdict[0] == 1
    assert L.p2e_schnorr_verify_aggregate(h, None, p(buf), p(buf), C.c_size_t(0), p(buf), C.c_uint(0), p(verdict), None) == -1
    too_many = C.c_size_t(1 << 23)                                               # 2 n + 1 = 2^24 + 1 terms
    assert L.p2e_schnorr_verify_aggregate(h, p(buf), p(buf), p(buf), too_many, p(buf), C.c_uint(0), p(verdict), None) == -1
    assert L.p2e_schnorr_verify_aggregate(h, p(buf), p(buf), p(buf), C.c_size_t(1), p(buf), C.c_uint(13), p(verdict), None) == -1
    assert L.p2e_schnorr_verify_aggregate(h, p(buf), p(buf), p(buf), C.c_size_t(1), None, C.c_uint(0), p(verdict), None) == -1
    assert L.p2e_schnorr_verify_aggregate(h, p(buf), p(buf), p(buf), C.c_size_t(1), p(buf), C.c_uint(0), None, None) == -1
    assert L.p2e_schnorr_sign_batch(h, p(buf), p(buf), None, p(buf), C.c_size_t(1), p(buf)) == -1
    assert L.p2e_schnorr_verify_batch(h, p(buf), p(buf), p(buf), C.c_size_t(1), p(buf), None) == -1
    for call in (lambda: L.p2e_schnorr_public_key_batch(h, p(buf), p(buf), C.c_size_t(0), p(buf)),
                 lambda: L.p2e_xonly_decode_batch(h, p(buf), p(buf), p(buf), C.c_size_t(0), p(buf))):
        assert call() == 0
