"""DLEQ proofs on the GPU (include/p2e.h p2e_dleq_prove_batch, p2e_dleq_verify_batch) through the C ABI.

Expectations come from tests/dleq_inputs.py alone: the header's definition in Python integers and hashlib (test_dleq_cpu.py pins
that oracle).  Every byte of every element is compared; output buffers are pre-filled with 0xAA so that an unwritten byte shows,
and hold one element more than the call may write.

Shapes: both calls at count = 0, 1, 63, 64, 65 and 257, with and without a message.  The first wave mixes flagged and good
lanes.  The arithmetic behind the hashes runs with a forced k and a forced e through tests/probe_dleq (built on demand with the
library's flags): no hash output reaches k = 0 or e >= n."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import plonky2_ecdsa_amd as p2e
import dleq_inputs as D
import schnorr_inputs as SI
import sp_inputs as SP

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tests", "probe_dleq")
size = C.c_size_t


@pytest.fixture(scope="module")
def hctx():
    return p2e.Context(device=0, host_pointers=True)


def filled(*shape):
    return np.full(shape, 0xAA, np.uint8)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def rows_of(a, n):
    """the first n rows of an input array as its own buffer; one dummy row for n = 0; None stays None"""
    return None if a is None else np.ascontiguousarray(a[:max(n, 1)]).copy()


def prove_call(hctx, A, n, want_c=True):
    proof, cx, cy, err = filled(n + 1, 64), filled(n + 1, 32), filled(n + 1, 32), filled(n + 1)
    rc = hctx._L.p2e_dleq_prove_batch(hctx._h, _p(rows_of(A["a"], n)), _p(rows_of(A["bx"], n)), _p(rows_of(A["by"], n)), _p(rows_of(A["aux"], n)),
                                      _p(rows_of(A["msg"], n)), _p(proof), _p(cx) if want_c else None, _p(cy) if want_c else None, size(n), _p(err))
    return rc, proof, cx, cy, err


def verify_call(hctx, A, n, msg="own"):
    err, valid = filled(n + 1), filled(n + 1)
    m = rows_of(A["msg"], n) if isinstance(msg, str) else msg
    rc = hctx._L.p2e_dleq_verify_batch(hctx._h, _p(rows_of(A["ax"], n)), _p(rows_of(A["ay"], n)), _p(rows_of(A["bx"], n)), _p(rows_of(A["by"], n)),
                                       _p(rows_of(A["cx"], n)), _p(rows_of(A["cy"], n)), _p(rows_of(A["proof"], n)), _p(m), size(n), _p(err), _p(valid))
    return rc, err, valid


# ---- both calls against the oracle ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", D.SIZES)
@pytest.mark.parametrize("with_msg", [False, True])
def test_prove_equals_the_oracle(with_msg, n, hctx):
    A = D.prover_arrays(with_msg)
    rc, proof, cx, cy, err = prove_call(hctx, A, n)
    assert rc >= 0, p2e.lib().p2e_last_error()
    diff = np.nonzero((err[:n] != A["err"][:n]) | (proof[:n] != A["proof"][:n]).any(axis=1))[0]
    assert diff.size == 0, [(int(i), int(err[i]), int(A["err"][i])) for i in diff[:8]]
    assert np.array_equal(cx[:n], A["cx"][:n]) and np.array_equal(cy[:n], A["cy"][:n]) and rc == np.count_nonzero(A["err"][:n])
    assert (proof[n] == 0xAA).all() and (cx[n] == 0xAA).all() and (cy[n] == 0xAA).all() and err[n] == 0xAA
    flagged = A["err"][:n] != 0
    assert not proof[:n][flagged].any() and not cx[:n][flagged].any() and not cy[:n][flagged].any()
    assert n < 257 or rc == 10


@pytest.mark.parametrize("n", D.SIZES)
@pytest.mark.parametrize("with_msg", [False, True])
def test_verify_equals_the_oracle(with_msg, n, hctx):
    A = D.verifier_arrays(with_msg)
    rc, err, valid = verify_call(hctx, A, n)
    assert rc >= 0, p2e.lib().p2e_last_error()
    diff = np.nonzero((err[:n] != A["err"][:n]) | (valid[:n] != A["valid"][:n]))[0]
    assert diff.size == 0, [(int(i), D.verifier_set(with_msg)[i]["kind"], int(err[i]), int(valid[i])) for i in diff[:8]]
    assert rc == np.count_nonzero(A["err"][:n]) and err[n] == 0xAA and valid[n] == 0xAA and not valid[:n][A["err"][:n] != 0].any()
    if n == 257:                                           # (d) on the device: each rejection is err 0, valid 0, not counted
        kinds = np.array([v["kind"] for v in D.verifier_set(with_msg)])
        for kind in ("flip_e", "flip_s", "C_plus_G", "swap_A_C", "s_zero", "e_zero", "e_ge_n"):
            assert (kinds == kind).any() and not err[:n][kinds == kind].any() and not valid[:n][kinds == kind].any(), kind
        assert (valid[:n][kinds == "good"] == 1).all()


def test_a_message_where_none_was_proven_and_the_reverse_are_rejected(hctx):
    n = 65
    other = np.full((n, 32), 0x5A, np.uint8)
    for with_msg, msg in ((False, other), (True, None)):
        A = D.verifier_arrays(with_msg)
        rc, err, valid = verify_call(hctx, A, n, msg=msg)
        assert rc == np.count_nonzero(A["err"][:n]) and np.array_equal(err[:n], A["err"][:n]) and not valid[:n].any()


def test_prove_then_verify_on_the_device_and_the_share_in_place(hctx):
    """every good lane's fresh proof verifies; (cx32, cy32) = (bx32, by32) gives the same bytes; without the share the same proofs"""
    n = 257
    A = D.prover_arrays(True)
    good = A["err"] == 0
    ax, ay = D.points([SI.base_mul(p["a"]) or D.O for p in D.prover_set(True)])       # (a = 0 and a = n: flagged lanes, left out below)
    rc, proof, cx, cy, err = prove_call(hctx, A, n)
    verr, valid, vbad = hctx.dleq_verify_batch(ax[good], ay[good], A["bx"][good], A["by"][good], cx[:n][good], cy[:n][good], proof[:n][good],
                                               msg=A["msg"][good])
    assert vbad == 0 and not verr.any() and (valid == 1).all() and valid.size == 247
    bx, by = A["bx"].copy(), A["by"].copy()
    proof2, err2 = filled(n, 64), filled(n)
    rc2 = hctx._L.p2e_dleq_prove_batch(hctx._h, _p(A["a"].copy()), _p(bx), _p(by), _p(A["aux"].copy()), _p(A["msg"].copy()), _p(proof2), _p(bx), _p(by),
                                       size(n), _p(err2))
    assert rc2 == rc == 10 and np.array_equal(bx, A["cx"]) and np.array_equal(by, A["cy"]) and np.array_equal(proof2, A["proof"])
    rc3, proof3, cx3, cy3, err3 = prove_call(hctx, A, 65, want_c=False)
    assert rc3 == np.count_nonzero(A["err"][:65]) and np.array_equal(proof3[:65], A["proof"][:65]) and (cx3 == 0xAA).all() and (cy3 == 0xAA).all()


def test_refused_arguments(hctx):
    L, h = hctx._L, hctx._h
    bufs = [np.zeros(512, np.uint8) for _ in range(12)]
    p = [_p(b) for b in bufs]
    one, zero = size(1), size(0)
    assert L.p2e_dleq_prove_batch(h, p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], one, p[8]) == 1           # a = 0: one flag
    assert L.p2e_dleq_prove_batch(h, p[0], p[1], p[2], p[3], None, p[5], None, None, one, p[8]) == 1
    for k in (0, 1, 2, 3, 5, 8):
        a = p[:9]
        a[k] = None
        assert L.p2e_dleq_prove_batch(h, a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], one, a[8]) == -1
        assert "null pointer" in L.p2e_last_error().decode()
    assert L.p2e_dleq_prove_batch(h, p[0], p[1], p[2], p[3], p[4], p[5], p[6], None, one, p[8]) == -1         # cx32 without cy32
    assert L.p2e_dleq_verify_batch(h, p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], one, p[8], p[9]) == 1    # A neutral: one flag
    assert L.p2e_dleq_verify_batch(h, p[0], p[1], p[2], p[3], p[4], p[5], p[6], None, one, p[8], p[9]) == 1
    for k in (0, 1, 2, 3, 4, 5, 6, 8, 9):
        a = p[:10]
        a[k] = None
        assert L.p2e_dleq_verify_batch(h, a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], one, a[8], a[9]) == -1
    assert L.p2e_dleq_prove_batch(h, p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], zero, p[8]) == 0
    assert L.p2e_dleq_verify_batch(h, p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], zero, p[8], p[9]) == 0
    # an overlap is refused on a live context too, and the context stays usable
    assert L.p2e_dleq_prove_batch(h, p[0], p[1], p[2], p[3], p[4], p[5], p[2], p[1], one, p[8]) == -1 and "overlap" in L.p2e_last_error().decode()
    assert L.p2e_dleq_prove_batch(h, p[0], p[1], p[2], p[3], p[4], p[0], p[6], p[7], one, p[8]) == -1 and "overlap" in L.p2e_last_error().decode()
    assert L.p2e_dleq_verify_batch(h, p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], one, p[0], p[9]) == -1 and "overlap" in L.p2e_last_error().decode()
    assert L.p2e_dleq_verify_batch(h, p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], one, p[8], p[9]) == 1


# ---- device pointers ----------------------------------------------------------------------------------------------------------------
def test_a_silent_payment_senders_operands_are_proven_and_verified_on_the_device():
    """The operands of p2e_sp_send_batch (the sender's key a, the receiver's B_scan) -> p2e_ecdsa_public_key_batch (A = a G) ->
    p2e_dleq_prove_batch -> p2e_dleq_verify_batch, on device pointers in async mode: the share and the proof the prover writes are
    what the verifier reads, nothing visits the host in between.  The shares equal the oracle's a B_scan."""
    n = 65
    ctx = p2e.Context(device=0, asynchronous=True)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    full = lambda *shape: torch.full(shape, 0xAA, dtype=torch.uint8, device="cuda:0")
    K = SP.send_set()
    good = [i for i in range(SP.N_SET) if K["err"][i] == 0][:n]
    assert len(good) == n
    a, bx, by = dev(K["a"][good]), dev(K["scan_pkx"][good]), dev(K["scan_pky"][good])
    aux, msg = dev(D.rows([b"\x11" * 32] * n)), dev(D.rows([bytes([i]) * 32 for i in range(n)]))
    ax, ay, e0, _ = ctx.ecdsa_public_key_batch(a, pkx=full(n, 32), pky=full(n, 32), err=full(n))
    proof, cx, cy, e1, _ = ctx.dleq_prove_batch(a, bx, by, aux, msg=msg, proof=full(n, 64), cx=full(n, 32), cy=full(n, 32), err=full(n))
    e2, valid, _ = ctx.dleq_verify_batch(ax, ay, bx, by, cx, cy, proof, msg=msg, err=full(n), valid=full(n))
    assert ctx.sync() == 0
    torch.cuda.synchronize()
    for e in (e0, e1, e2):
        assert not e.cpu().numpy().any()
    assert (valid.cpu().numpy() == 1).all()
    cxh, cyh, ph = cx.cpu().numpy(), cy.cpu().numpy(), proof.cpu().numpy()
    for j, i in enumerate(good):
        sk = int.from_bytes(K["a"][i].tobytes(), "little")
        B = (int.from_bytes(K["scan_pkx"][i].tobytes(), "little"), int.from_bytes(K["scan_pky"][i].tobytes(), "little"))
        code, want, Cw = D.prove(sk, B, b"\x11" * 32, bytes([j]) * 32)
        assert code == 0 and ph[j].tobytes() == want and (cxh[j].tobytes(), cyh[j].tobytes()) == (Cw[0].to_bytes(32, "little"), Cw[1].to_bytes(32, "little"))
    ctx.close()


# ---- behind the hashes, on the device ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe():
    lib = os.path.join(PROBE, "libp2e_probe_dleq.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-s", "-C", PROBE, "libp2e_probe_dleq.so"])
    L = C.CDLL(lib)
    L.probedleq_prove_with_nonce.restype = L.probedleq_verify_points.restype = C.c_long
    return L


def test_forced_nonces_and_challenges_on_the_device(probe):
    """k = 0 flagged; e = 0, e = n, e = n + 5, e = 2^256 - 1 used modulo n; R1 = k G and R2 = (k b) G by an independent route; the
    neutral pair refused.  70 elements: the table twice, so that lanes of one wave take different branches."""
    cases = D.forced_cases() * 2
    n = len(cases)
    A = [SI.base_mul(a) for a, b, k, e in cases]
    B = [SI.base_mul(b) for a, b, k, e in cases]
    Cs = [SI.base_mul(a * b % D.N) for a, b, k, e in cases]
    a32 = np.stack([D.le32(a) for a, b, k, e in cases])
    (ax, ay), (bx, by), (cx, cy) = D.points(A), D.points(B), D.points(Cs)
    k32 = D.rows([D.b32(k % D.N) for a, b, k, e in cases])
    e32 = D.rows([D.b32(e) for a, b, k, e in cases])
    s32 = D.rows([D.b32(D.response(k % D.N, e, a)) for a, b, k, e in cases])
    for msg in (None, np.full((n, 32), 0x77, np.uint8)):
        proof, code = filled(n, 64), filled(n)
        assert probe.probedleq_prove_with_nonce(_p(a32), _p(ax), _p(ay), _p(bx), _p(by), _p(cx), _p(cy), _p(k32), _p(msg), _p(proof), _p(code), size(n)) == 0
        for i, (a, b, k, e) in enumerate(cases):
            want = D.prove_with_nonce(a, A[i], B[i], Cs[i], k % D.N, None if msg is None else msg[i].tobytes())
            assert (int(code[i]), proof[i].tobytes()) == want, (i, k)
        assert set(code.tolist()) == {D.WIRE_OK, D.WIRE_INFINITY}
    r1x, r1y, r2x, r2y, ok = filled(n, 32), filled(n, 32), filled(n, 32), filled(n, 32), filled(n)
    assert probe.probedleq_verify_points(_p(ax), _p(ay), _p(bx), _p(by), _p(cx), _p(cy), _p(e32), _p(s32), _p(r1x), _p(r1y), _p(r2x), _p(r2y), _p(ok),
                                         size(n)) == 0
    for i, (a, b, k, e) in enumerate(cases):
        neutral = k % D.N == 0
        R1, R2 = ((0, 0), (0, 0)) if neutral else (SI.base_mul(k), SI.base_mul(k * b % D.N))
        assert int(ok[i]) == (not neutral), i
        assert (r1x[i].tobytes(), r1y[i].tobytes(), r2x[i].tobytes(), r2y[i].tobytes()) == tuple(v.to_bytes(32, "little") for v in R1 + R2), i
    assert set(ok.tolist()) == {0, 1}


def test_c_example_proves_verifies_and_rejects_a_flipped_bit(tmp_path):
    """examples/dleq_share.c: keys from small integers, prove, verify, flip one bit, verify again"""
    exe = str(tmp_path / "dleq_share")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "dleq_share.c"), "-L", os.path.join(ROOT, "plonky2-ecdsa_amd"), "-lp2e_hip",
                           "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe])
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "plonky2-ecdsa_amd") + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    r = subprocess.run([exe, "200"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "200 shares proven (0 refused), 200 proofs valid; with one bit flipped in proof 100: 199 valid" in r.stdout
