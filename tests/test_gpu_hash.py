"""Message hashing, RFC 6979 nonces, the deterministic signer and Ethereum addresses on the GPU (include/p2e.h
p2e_hash_batch, p2e_ecdsa_nonce_rfc6979_batch, p2e_ecdsa_sign_deterministic_batch, p2e_eth_address_batch).

Expectations come from tests/hash_inputs.py (hashlib, oracle/p2e_ref.py's Keccak and big-int curves, RFC 6979 written with
hmac) and from the calls the project already has (the signers, the recovery, the two verifiers)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import hash_inputs as H
import plonky2_ecdsa_amd as p2e

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tests", "probe_hash")
N_MAIN = H.N_MAIN
PLANS = [p2e.SIGN_PLAN_LANE, p2e.SIGN_PLAN_QUAD]
E_INVALID = -1


@pytest.fixture(scope="module")
def ctx():
    return p2e.Context(device=0)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _pre(*shape):
    return torch.full(shape, 0xAA, dtype=torch.uint8, device="cuda")


def _buffer(alg):
    """the batch's bytes on the device, its first byte at misalignment alg + 1, and the offsets as int64"""
    data, offsets, _ = H.message_batch(alg)
    room = torch.zeros(data.size + 8, dtype=torch.uint8, device="cuda")
    view = room[alg + 1:alg + 1 + data.size]
    view.copy_(_dev(data))
    assert view.data_ptr() % 4 == alg + 1
    return view, _dev(offsets.astype(np.int64))


def _hash(ctx, alg, form, data, offsets):
    """out32 as numpy, with one 32-byte guard row before and after it checked untouched"""
    n = offsets.shape[0] - 1
    box = _pre(n + 2, 32)
    out, bad = ctx.hash_batch(data, offsets, alg=alg, out_form=form, out=box[1:n + 1])
    torch.cuda.synchronize()
    got = box.cpu().numpy()
    assert (got[0] == 0xAA).all() and (got[n + 1] == 0xAA).all(), "wrote outside out32"
    return got[1:n + 1], bad


@pytest.mark.parametrize("form", [H.DIGEST_BYTES, H.DIGEST_SCALAR])
@pytest.mark.parametrize("alg", H.ALGS)
def test_every_digest_byte_on_the_main_batch(alg, form, ctx):
    data, offsets = _buffer(alg)
    _, _, msgs = H.message_batch(alg)
    got, bad = _hash(ctx, alg, form, data, offsets)
    want = H.as_form(H.digests(alg), form)
    diff = np.nonzero((got != want).any(axis=1))[0]
    assert diff.size == 0, (alg, form, [(int(i), len(msgs[i])) for i in diff[:8]])
    assert bad == 0


@pytest.mark.parametrize("n", [1, 3, 64, 257])
@pytest.mark.parametrize("alg", H.ALGS)
def test_slices_at_the_head_and_the_tail(alg, n, ctx):
    data, offsets = _buffer(alg)
    for lo in (0, N_MAIN - n):
        for form in (H.DIGEST_BYTES, H.DIGEST_SCALAR):
            got, bad = _hash(ctx, alg, form, data, offsets[lo:lo + n + 1])
            assert bad == 0 and np.array_equal(got, H.as_form(H.digests(alg)[lo:lo + n], form)), (alg, n, lo, form)


@pytest.mark.parametrize("alg", H.ALGS)
def test_non_monotonic_offsets_are_empty_messages_and_counted(alg, ctx):
    data, offsets = _buffer(alg)
    n = 300
    off = offsets[:n + 1].clone()
    planted = [5, 64, 298]                       # inside a wave, a wave's first lane, near the batch's end
    for i in planted:
        off[i + 1] = off[i] - 1                  # (stays inside [offsets[0], offsets[n]]; the next element grows by it)
    off_host = off.cpu().numpy()
    # the elements behind a planted one start at its (moved) end: recompute what every element now is
    raw = H.message_batch(alg)[0].tobytes()
    want, count = [], 0
    for i in range(n):
        a, b = int(off_host[i]), int(off_host[i + 1])
        count += b < a
        want.append(H.digest(alg, raw[a:b] if b >= a else b""))
    assert count == 3
    got, bad = _hash(ctx, alg, H.DIGEST_BYTES, data, off)
    assert bad == 3
    assert [bytes(r) for r in got] == want
    assert all(bytes(got[i]) == H.digest(alg, b"") for i in planted)


def test_published_hash_answers(ctx):
    msgs = [b"abc", b"", b"abc"]
    data, offsets = _dev(np.frombuffer(b"abc" + b"abc", np.uint8)), _dev(np.array([0, 3, 3, 6], np.int64))
    sha, _ = _hash(ctx, H.SHA256, H.DIGEST_BYTES, data, offsets)
    kec, _ = _hash(ctx, H.KECCAK256, H.DIGEST_BYTES, data, offsets)
    assert len(msgs) == 3 and sha[0].tobytes().hex() == H.SHA256_ABC == sha[2].tobytes().hex()
    assert kec[1].tobytes().hex() == H.KECCAK_EMPTY and kec[0].tobytes().hex() == H.KECCAK_ABC == kec[2].tobytes().hex()


@pytest.mark.parametrize("curve_id", [0, 1])
def test_every_nonce_byte_on_the_main_batch(curve_id, ctx):
    msg, sk, want = H.nonce_batch(curve_id)
    box = _pre(N_MAIN + 2, 32)
    k, rc = ctx.ecdsa_nonce_rfc6979_batch(_dev(H.pack(msg)), _dev(H.pack(sk)), curve=curve_id, k=box[1:N_MAIN + 1])
    torch.cuda.synchronize()
    got = box.cpu().numpy()
    assert rc == 0 and (got[0] == 0xAA).all() and (got[-1] == 0xAA).all()
    diff = np.nonzero((got[1:-1] != H.pack(want)).any(axis=1))[0]
    assert diff.size == 0, (curve_id, diff[:8].tolist())
    for n in (1, 3, 64, 257):                                      # small launches, head and tail
        for lo in (0, N_MAIN - n):
            k, rc = ctx.ecdsa_nonce_rfc6979_batch(_dev(H.pack(msg[lo:lo + n])), _dev(H.pack(sk[lo:lo + n])), curve=curve_id)
            assert rc == 0 and np.array_equal(k.cpu().numpy(), H.pack(want[lo:lo + n]))


def test_published_nonces_and_the_a25_signature(ctx):
    import hashlib
    data = _dev(np.frombuffer(b"sampletestSatoshi Nakamoto", np.uint8))
    z, _ = ctx.hash_batch(data, _dev(np.array([0, 6, 10, 26], np.int64)), alg=p2e.HASH_SHA256, out_form=p2e.DIGEST_SCALAR)
    assert H.unpack(z.cpu().numpy())[0] == int.from_bytes(hashlib.sha256(b"sample").digest(), "big")
    x = _dev(H.pack([H.A25_X, H.A25_X]))
    k, _ = ctx.ecdsa_nonce_rfc6979_batch(z[:2], x, curve=p2e.CURVE_P256)
    assert H.unpack(k.cpu().numpy()) == [H.A25_SAMPLE_K, H.A25_TEST_K]
    k1, _ = ctx.ecdsa_nonce_rfc6979_batch(z[2:], _dev(H.pack([1])), curve=p2e.CURVE_SECP256K1)
    assert H.unpack(k1.cpu().numpy()) == [H.SATOSHI_K]
    for plan in PLANS:
        r, s, v, err, bad = ctx.ecdsa_sign_deterministic_batch(z[:1], x[:1], curve=p2e.CURVE_P256, plan=plan)
        assert bad == 0 and H.unpack(r.cpu().numpy()) == [H.A25_SAMPLE_R] and H.unpack(s.cpu().numpy()) == [H.A25_SAMPLE_S]


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("curve_id", [0, 1])
def test_deterministic_signer_equals_the_signers_fed_with_the_nonce_call(curve_id, plan, ctx):
    msg, sk, _ = H.nonce_batch(curve_id)                           # msg, sk in {0, 1, n - 1, n, 2^256 - 1} among them
    n = 1024
    dmsg, dsk = _dev(H.pack(msg[:n])), _dev(H.pack(sk[:n]))
    k, _ = ctx.ecdsa_nonce_rfc6979_batch(dmsg, dsk, curve=curve_id)
    want = ctx.ecdsa_sign_recoverable_batch(dmsg, dsk, k, curve=curve_id, plan=plan, r=_pre(n, 32), s=_pre(n, 32), v=_pre(n), err=_pre(n))
    got = ctx.ecdsa_sign_deterministic_batch(dmsg, dsk, curve=curve_id, plan=plan, r=_pre(n, 32), s=_pre(n, 32), v=_pre(n), err=_pre(n))
    torch.cuda.synchronize()
    assert got[4] == want[4] == 0
    for g, w, name in zip(got[:4], want[:4], "rsve"):
        assert torch.equal(g, w), (curve_id, plan, name)
    # v = NULL: the plain signer's outputs
    want = ctx.ecdsa_sign_batch(dmsg, dsk, k, curve=curve_id, plan=plan, r=_pre(n, 32), s=_pre(n, 32), err=_pre(n))
    r, s, v, err, bad = ctx.ecdsa_sign_deterministic_batch(dmsg, dsk, curve=curve_id, plan=plan, r=_pre(n, 32), s=_pre(n, 32), err=_pre(n),
                                                           recoverable=False)
    torch.cuda.synchronize()
    assert v is None and bad == want[3] == 0 and torch.equal(r, want[0]) and torch.equal(s, want[1]) and torch.equal(err, want[2])
    # and the same call again gives the same bytes (the scratch block was wiped and reused)
    again = ctx.ecdsa_sign_deterministic_batch(dmsg, dsk, curve=curve_id, plan=plan)
    torch.cuda.synchronize()
    assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1]) and torch.equal(again[2], got[2])


@pytest.mark.parametrize("curve_id", [0, 1])
def test_deterministic_signatures_verify_and_recover(curve_id, ctx):
    n = 1024
    cv = H.CURVES[curve_id]
    rng = H.R.SplitMix64(0xDE7 + curve_id)
    msg, sk = [_dev(H.pack([rng.below(cv.n) for _ in range(n)])) for _ in range(2)]
    r, s, v, e1, bad1 = ctx.ecdsa_sign_deterministic_batch(msg, sk, curve=curve_id)
    wx, wy, e2, bad2 = ctx.ecdsa_public_key_batch(sk, curve=curve_id)
    if curve_id == 0:
        e3, valid, bad3 = ctx.ecdsa_verify_batch(msg, r, s, wx, wy)
        pkx, pky, e4, bad4 = ctx.ecdsa_recover_batch(msg, r, s, v, curve=curve_id)
        torch.cuda.synchronize()
        assert bad4 == 0 and torch.equal(pkx, wx) and torch.equal(pky, wy)
    else:
        prog = p2e.CurveProgram(ctx, p2e.CP_VERIFY, p2e.CURVE_P256, blind=cv.mul(0xB11D, cv.g))
        e3, valid, bad3 = prog.verify_batch(msg, r, s, wx, wy)
        torch.cuda.synchronize()
        prog.close()
    torch.cuda.synchronize()
    assert (bad1, bad2, bad3) == (0, 0, 0) and bool((valid == 1).all())
    # a sample against Python: RFC 6979 nonce, then sign_message with integers
    mi, di = H.unpack(msg[:4].cpu().numpy()), H.unpack(sk[:4].cpu().numpy())
    want = [H.sign(cv, m, d, H.rfc6979(cv.n, d, m)[0]) for m, d in zip(mi, di)]
    assert list(zip(H.unpack(r[:4].cpu().numpy()), H.unpack(s[:4].cpu().numpy()), v[:4].cpu().tolist())) == want


def test_every_address_byte_on_the_main_batch(ctx):
    pkx, pky, want = H.address_batch()
    box = _pre(N_MAIN * 20 + 40)
    addr, rc = ctx.eth_address_batch(_dev(pkx), _dev(pky), addr=box[20:20 + 20 * N_MAIN].view(N_MAIN, 20))
    torch.cuda.synchronize()
    got = box.cpu().numpy()
    assert rc == 0 and (got[:20] == 0xAA).all() and (got[-20:] == 0xAA).all()
    got = got[20:-20].reshape(N_MAIN, 20)
    assert got[0].tobytes().hex() == H.ADDRESS_OF_G                     # the address of sk = 1
    diff = np.nonzero((got != want).any(axis=1))[0]
    assert diff.size == 0, diff[:8].tolist()
    sk1x, sk1y, _e, _b = ctx.ecdsa_public_key_batch(_dev(H.pack([1])))
    a1, _ = ctx.eth_address_batch(sk1x, sk1y)
    assert a1.cpu().numpy()[0].tobytes().hex() == H.ADDRESS_OF_G
    for n in (1, 3, 64, 257):
        for lo in (0, N_MAIN - n):
            a, _ = ctx.eth_address_batch(_dev(pkx[lo:lo + n]), _dev(pky[lo:lo + n]))
            assert np.array_equal(a.cpu().numpy(), want[lo:lo + n])


def test_addresses_of_a_recovery_with_flagged_lanes(ctx):
    """the err of a recover call: flagged lanes give twenty zero bytes, every other lane keccak(pk)[12:]"""
    n = 300
    cv = H.CURVES[0]
    rng = H.R.SplitMix64(0xF1A6)
    msg, sk = [_dev(H.pack([rng.below(cv.n) for _ in range(n)])) for _ in range(2)]
    r, s, v, _e, bad = ctx.ecdsa_sign_deterministic_batch(msg, sk)
    flagged = [0, 63, 64, 150, 299]
    for i in flagged[:3]:
        r[i] = 0                                                      # r = 0: not recoverable
    for i in flagged[3:]:
        v[i] = 7                                                      # v > 3: not recoverable
    pkx, pky, err, bad = ctx.ecdsa_recover_batch(msg, r, s, v)
    addr, rc = ctx.eth_address_batch(pkx, pky, err=err, addr=_pre(n, 20))
    torch.cuda.synchronize()
    assert bad == len(flagged) and np.nonzero(err.cpu().numpy())[0].tolist() == flagged and rc == 0
    xs, ys, got = H.unpack(pkx.cpu().numpy()), H.unpack(pky.cpu().numpy()), addr.cpu().numpy()
    for i in range(n):
        assert bytes(got[i]) == (bytes(20) if i in flagged else H.address(xs[i], ys[i])), i
    # without err the zero coordinates of a flagged lane DO hash to something: that is what err is for
    plain, _ = ctx.eth_address_batch(pkx, pky)
    assert bytes(plain.cpu().numpy()[0]) == H.address(0, 0) != bytes(20)


def test_host_pointer_and_async_contexts_give_the_same_bytes(ctx):
    n = 257
    alg = H.KECCAK256
    data, offsets, _ = H.message_batch(alg)
    off = offsets[100:100 + n + 1]                                   # offsets[0] != 0: the staging copy starts inside the buffer
    want_hash = H.as_form(H.digests(alg)[100:100 + n], H.DIGEST_SCALAR)
    msg, sk, want_k = [x[:n] for x in H.nonce_batch(0)]
    pmsg, psk = H.pack(msg), H.pack(sk)
    pkx, pky, want_addr = [x[:n] for x in H.address_batch()]
    ref = [t.cpu().numpy() for t in ctx.ecdsa_sign_deterministic_batch(_dev(pmsg), _dev(psk))[:4]]
    err = np.zeros(n, np.uint8)
    err[5] = 128

    hctx = p2e.Context(device=0, host_pointers=True)
    out, bad = hctx.hash_batch(data, off, alg=alg, out_form=H.DIGEST_SCALAR)
    assert bad == 0 and np.array_equal(out, want_hash)
    k, rc = hctx.ecdsa_nonce_rfc6979_batch(pmsg, psk)
    assert rc == 0 and np.array_equal(k, H.pack(want_k))
    got = hctx.ecdsa_sign_deterministic_batch(pmsg, psk)
    assert got[4] == 0 and all(np.array_equal(g, w) for g, w in zip(got[:4], ref))
    addr, rc = hctx.eth_address_batch(pkx, pky, err=err)
    assert rc == 0 and np.array_equal(addr, np.where(err[:, None] != 0, 0, want_addr))
    hctx.close()

    actx = p2e.Context(device=0, asynchronous=True)
    ddata, doff = _dev(data), _dev(off.astype(np.int64))
    bad_off = doff.clone()
    bad_off[3] = bad_off[2] - 1                                      # one element runs backwards: counted at sync time
    out, rc = actx.hash_batch(ddata, doff, alg=alg, out_form=H.DIGEST_SCALAR)
    assert rc == 0 and actx.sync() == 0 and np.array_equal(out.cpu().numpy(), want_hash)
    out, rc = actx.hash_batch(ddata, bad_off, alg=alg)
    assert rc == 0 and actx.sync() == 1
    k, rc = actx.ecdsa_nonce_rfc6979_batch(_dev(pmsg), _dev(psk))
    assert rc == 0 and actx.sync() == 0 and np.array_equal(k.cpu().numpy(), H.pack(want_k))
    got = actx.ecdsa_sign_deterministic_batch(_dev(pmsg), _dev(psk))
    assert got[4] == 0 and actx.sync() == 0 and all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got[:4], ref))
    addr, rc = actx.eth_address_batch(_dev(pkx), _dev(pky), err=_dev(err))
    assert rc == 0 and actx.sync() == 0 and np.array_equal(addr.cpu().numpy(), np.where(err[:, None] != 0, 0, want_addr))
    actx.close()


def test_misuse_is_refused_and_empty_batches_are_fine(ctx):
    L, h = ctx._L, ctx._h
    buf = torch.zeros(256, dtype=torch.uint8, device="cuda")
    p, null, one = C.c_void_p(buf.data_ptr()), C.c_void_p(0), C.c_size_t(1)
    # a null pointer, in every call
    assert L.p2e_hash_batch(h, 0, 0, null, p, p, one) == E_INVALID
    assert L.p2e_hash_batch(h, 0, 0, p, null, p, one) == E_INVALID
    assert L.p2e_hash_batch(h, 0, 0, p, p, null, one) == E_INVALID
    assert L.p2e_ecdsa_nonce_rfc6979_batch(h, 0, p, p, null, one) == E_INVALID
    assert L.p2e_ecdsa_sign_deterministic_batch(h, 0, 0, p, null, p, p, p, one, p) == E_INVALID
    assert L.p2e_ecdsa_sign_deterministic_batch(h, 0, 0, p, p, p, p, null, one, null) == E_INVALID      # err is required, v is not
    assert L.p2e_eth_address_batch(h, p, p, null, null, one) == E_INVALID
    # a bad alg, a bad out_form, a bad curve, a bad plan
    assert L.p2e_hash_batch(h, 3, 0, p, p, p, one) == E_INVALID
    assert L.p2e_hash_batch(h, -1, 0, p, p, p, one) == E_INVALID
    assert L.p2e_hash_batch(h, 0, 2, p, p, p, one) == E_INVALID
    assert L.p2e_ecdsa_nonce_rfc6979_batch(h, 2, p, p, p, one) == E_INVALID
    assert L.p2e_ecdsa_sign_deterministic_batch(h, 2, 0, p, p, p, p, p, one, p) == E_INVALID
    assert L.p2e_ecdsa_sign_deterministic_batch(h, 0, 3, p, p, p, p, p, one, p) == E_INVALID
    assert b"plan" in L.p2e_last_error()
    # n == 0
    zero = C.c_size_t(0)
    assert L.p2e_hash_batch(h, 0, 0, p, p, p, zero) == 0
    assert L.p2e_ecdsa_nonce_rfc6979_batch(h, 0, p, p, p, zero) == 0
    assert L.p2e_ecdsa_sign_deterministic_batch(h, 0, 0, p, p, p, p, p, zero, p) == 0
    assert L.p2e_eth_address_batch(h, p, p, null, p, zero) == 0
    torch.cuda.synchronize()
    assert not buf.any()                                              # nothing was written by any of them
    # the context still works
    out, bad = ctx.hash_batch(_dev(np.frombuffer(b"abc", np.uint8)), _dev(np.array([0, 3], np.int64)))
    assert bad == 0 and out.cpu().numpy()[0].tobytes().hex() == H.SHA256_ABC


def test_retry_branch_on_the_device():
    """tests/probe_hash: the 200 inputs of the synthetic order 2^255 + 1 as ONE launch, so that lanes which retry (102 of
    them, up to 7 times) and lanes which are done share waves; k and the number of refused candidates of every element"""
    lib = os.path.join(PROBE, "libp2e_probe_hash.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-s", "-C", PROBE, "libp2e_probe_hash.so"])
    L = C.CDLL(lib)
    L.probeh_nonce.restype = C.c_long
    xs, zs, ks, refused = H.retry_set()
    k, rej = np.full((H.RETRY_N, 32), 0xAA, np.uint8), np.full(H.RETRY_N, 0xAAAAAAAA, np.uint32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.probeh_nonce(ptr(H.pack([H.RETRY_Q])), ptr(H.pack(xs)), ptr(H.pack(zs)), ptr(k), ptr(rej), C.c_size_t(H.RETRY_N)) == 0
    assert sum(1 for r in refused if r) == 102 and max(refused) == 7
    assert H.unpack(k) == ks
    assert rej.tolist() == refused


def test_plain_c_client_hashes_signs_recovers_and_matches_addresses(tmp_path):
    """examples/eth_sender.c: device buffers from plain C through the six calls"""
    exe = str(tmp_path / "eth_sender")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "eth_sender.c"), "-L", os.path.join(ROOT, "plonky2-ecdsa_amd"), "-lp2e_hip",
                           "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe])
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "plonky2-ecdsa_amd") + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""),
               GPU_MAX_HW_QUEUES="8")
    r = subprocess.run([exe, "300"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "300 messages hashed (0 malformed), 300 signed (0 flagged), 300 keys recovered (0 flagged), 300 sender addresses match" in r.stdout
