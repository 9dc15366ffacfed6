"""Batch key derivation and signing on the GPU (include/p2e.h p2e_ecdsa_public_key_batch / p2e_ecdsa_sign_batch): to_public
and sign_message of curve/ecdsa.rs on secp256k1 and P-256, in the lane-per-scalar plan, the four-lanes-per-scalar plan and
the library's choice between them.

Expectations come from tests/sign_inputs.py (C oracle fixed-base walk for the points, Python integers for s, the flagged
sets from the inputs alone), from the host loop the calls replace (p2e_synth_signatures[_curve], bit for bit on the bench's
own batch) and from the verifiers the project already has (every GPU-made signature verifies, a tampered one does not)."""
import ctypes as C
import subprocess

import numpy as np
import pytest
import torch

import oracle_c
import plonky2_ecdsa_amd as p2e
import sign_inputs as S

pytestmark = pytest.mark.gpu

N_MAIN = 4161            # 65 full waves of scalars + one lane: the quad plan ends in a workgroup with a single live quad
PLANS = [S.PLAN_LANE, S.PLAN_QUAD]
AUTO_QUAD_MAX_N = 65536   # Tuning::sign_quad_max_n: P2E_SIGN_PLAN_AUTO takes the quad plan up to here


@pytest.fixture(scope="module")
def ctx():
    return p2e.Context(device=0)


@pytest.fixture(scope="module")
def main_cases():
    """per curve: the N_MAIN-element batch (E at both ends, random filler) and its expectations, computed once"""
    out = []
    for curve_id, cv in enumerate(S.CURVES):
        sk, k = S.batch(cv, N_MAIN, 0x151 + curve_id, shift=1), S.batch(cv, N_MAIN, 0x161 + curve_id)
        msg = S.batch(cv, N_MAIN, 0x171 + curve_id, shift=500)
        out.append(dict(ints=(msg, sk, k), b=[S.pack(v) for v in (msg, sk, k)], keys=S.expect_keys(curve_id, sk),
                        sigs=S.expect_sigs(curve_id, msg, sk, k)))
    return out


def _dev(arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _run(ctx, curve_id, plan, msg, sk, k):
    """both calls on device tensors -> (pkx, pky, e1, bad1, r, s, e2, bad2) as numpy"""
    d = _dev((msg, sk, k))
    n = d[0].shape[0]
    pre = lambda: torch.full((n, 32), 0xAA, dtype=torch.uint8, device="cuda")
    pkx, pky, e1, bad1 = ctx.ecdsa_public_key_batch(d[1], curve=curve_id, plan=plan, pkx=pre(), pky=pre())
    r, s, e2, bad2 = ctx.ecdsa_sign_batch(*d, curve=curve_id, plan=plan, r=pre(), s=pre())
    torch.cuda.synchronize()
    return tuple(v.cpu().numpy() if torch.is_tensor(v) else v for v in (pkx, pky, e1, bad1, r, s, e2, bad2))


def _assert_equal(got, want, what):
    diff = np.nonzero((got != want).any(axis=1))[0]
    assert diff.size == 0, (what, diff[:8].tolist())


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("curve_id", [0, 1])
def test_every_output_byte_on_the_edge_batch(curve_id, plan, ctx, main_cases):
    c = main_cases[curve_id]
    cv = S.CURVES[curve_id]
    pkx, pky, e1, bad1, r, s, e2, bad2 = _run(ctx, curve_id, plan, *c["b"])
    wx, wy, we1 = c["keys"]
    wr, ws, we2 = c["sigs"]
    msg, sk, k = c["ints"]
    assert np.nonzero(e1)[0].tolist() == [i for i, v in enumerate(sk) if v % cv.n == 0] and np.array_equal(e1, we1)
    assert np.nonzero(e2)[0].tolist() == [i for i, v in enumerate(k) if v % cv.n == 0] and np.array_equal(e2, we2)
    assert (bad1, bad2) == (4, 4)                       # n and 0 of E, at both ends of the batch
    # (flagged elements hold zeros in the expectation and in the output: every element is compared)
    for got, want, what in ((pkx, wx, "pkx"), (pky, wy, "pky"), (r, wr, "r"), (s, ws, "s")):
        _assert_equal(got, want, (curve_id, plan, what))


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("curve_id", [0, 1])
def test_tiny_batches(curve_id, plan, n, ctx, main_cases):
    c = main_cases[curve_id]
    lo = 1100                                            # random filler elements
    got = _run(ctx, curve_id, plan, *[a[lo:lo + n] for a in c["b"]])
    want = [a[lo:lo + n] for a in c["keys"]] + [a[lo:lo + n] for a in c["sigs"]]
    assert (got[3], got[7]) == (0, 0) and not got[2].any() and not got[6].any()
    for g, w, what in ((got[0], want[0], "pkx"), (got[1], want[1], "pky"), (got[4], want[3], "r"), (got[5], want[4], "s")):
        _assert_equal(g, w, (curve_id, plan, n, what))


@pytest.mark.parametrize("curve_id", [0, 1])
def test_the_bench_batch_equals_the_host_loop_bit_for_bit(curve_id, ctx):
    """the first 2 048 signatures of p2e_synth_signatures(4, ...) / p2e_synth_signatures_curve(curve, 4, ...): their
    (sk, msg, k) replayed from the splitmix stream, signed on the GPU, against the host loop's own output"""
    n = 2048
    host = p2e.synth_signatures(seed=4, n=n) if curve_id == 0 else p2e.synth_signatures_curve(curve_id, seed=4, n=n)
    sk, msg, k = S.replay_synth(curve_id, 4, n)
    assert np.array_equal(S.pack(msg), host[0]), "the replay does not reproduce the host stream"
    for plan in PLANS:
        pkx, pky, e1, bad1, r, s, e2, bad2 = _run(ctx, curve_id, plan, S.pack(msg), S.pack(sk), S.pack(k))
        assert (bad1, bad2) == (0, 0)
        for got, want, what in ((r, host[1], "r"), (s, host[2], "s"), (pkx, host[3], "pkx"), (pky, host[4], "pky")):
            _assert_equal(got, want, (curve_id, plan, what))


@pytest.mark.parametrize("curve_id", [0, 1])
def test_gpu_made_signatures_verify_and_tampered_ones_do_not(curve_id, ctx):
    n, tampered = 4096, (17, 4000)
    cv = S.CURVES[curve_id]
    rng = S.R.SplitMix64(0x5EED + curve_id)
    msg, sk, k = [S.pack([rng.below(cv.n) for _ in range(n)]) for _ in range(3)]
    d = _dev((msg, sk, k))
    pkx, pky, e1, bad1 = ctx.ecdsa_public_key_batch(d[1], curve=curve_id)
    r, s, e2, bad2 = ctx.ecdsa_sign_batch(*d, curve=curve_id)
    assert (bad1, bad2) == (0, 0)
    for i in tampered:
        d[0][i, 0] ^= 1
    if curve_id == 0:
        err, valid, bad = ctx.ecdsa_verify_batch(d[0], r, s, pkx, pky)
    else:
        blind = cv.mul(0xB11D, cv.g)
        prog = p2e.CurveProgram(ctx, p2e.CP_VERIFY, p2e.CURVE_P256, blind=blind)
        err, valid, bad = prog.verify_batch(d[0], r, s, pkx, pky)
        torch.cuda.synchronize()
        prog.close()
    torch.cuda.synchronize()
    assert bad == 0 and not err.cpu().numpy().any()
    assert np.nonzero(valid.cpu().numpy() != 1)[0].tolist() == list(tampered)


@pytest.mark.parametrize("curve_id", [0, 1])
def test_s_equal_zero_is_returned_unflagged(curve_id, ctx):
    """msg = -r sk (mod n) gives s = 0: returned as computed, as sign_message returns it"""
    cv = S.CURVES[curve_id]
    rng = S.R.SplitMix64(0x50 + curve_id)
    sk, k = [rng.below(cv.n) for _ in range(5)], [rng.below(cv.n) for _ in range(5)]
    pts = S.base_points(curve_id, k)
    msg = [(-(pts[kk][0] % cv.n) * d) % cv.n for kk, d in zip(k, sk)]
    for plan in PLANS:
        _x, _y, _e1, _b1, r, s, e2, bad2 = _run(ctx, curve_id, plan, S.pack(msg), S.pack(sk), S.pack(k))
        assert bad2 == 0 and not e2.any() and not s.any()
        assert S.unpack(r) == [pts[kk][0] % cv.n for kk in k]


@pytest.mark.parametrize("curve_id", [0, 1])
def test_auto_plan_equals_both_forced_plans_around_its_threshold(curve_id, ctx):
    """ragged batches on either side of the AUTO threshold (Tuning::sign_quad_max_n, MEASUREMENTS.md)"""
    threshold = AUTO_QUAD_MAX_N
    rng = np.random.default_rng(77 + curve_id)
    for n in (threshold - 61, threshold + 67):
        msg, sk, k = [rng.integers(0, 256, (n, 32), dtype=np.uint8) for _ in range(3)]
        runs = [_run(ctx, curve_id, plan, msg, sk, k) for plan in (S.PLAN_AUTO, S.PLAN_LANE, S.PLAN_QUAD)]
        for other in runs[1:]:
            for a, b in zip(runs[0], other):
                assert np.array_equal(a, b)
        assert runs[0][0].any() and runs[0][4].any()



def _raw(L, h, curve, plan, ptrs_key, ptrs_sign, n):
    a = L.p2e_ecdsa_public_key_batch(h, C.c_int(curve), C.c_uint(plan), *ptrs_key[:3], C.c_size_t(n), ptrs_key[3])
    b = L.p2e_ecdsa_sign_batch(h, C.c_int(curve), C.c_uint(plan), *ptrs_sign[:5], C.c_size_t(n), ptrs_sign[5])
    return a, b


def test_contexts_and_misuse(ctx, main_cases):
    """host-pointer and asynchronous contexts give the same bytes; misuse returns P2E_E_INVALID with a message and leaves
    the context usable: a witness fill on the same context (after the P-256 table was built lazily) matches the oracle"""
    n = 200
    for curve_id in (0, 1):
        c = main_cases[curve_id]
        msg, sk, k = [a[900:900 + n] for a in c["b"]]     # the tail of E (n, n + 1, 2^256 - 1, 0) and random filler
        want = _run(ctx, curve_id, S.PLAN_AUTO, msg, sk, k)
        hctx = p2e.Context(device=0, host_pointers=True)
        pkx, pky, e1, bad1 = hctx.ecdsa_public_key_batch(sk, curve=curve_id)
        r, s, e2, bad2 = hctx.ecdsa_sign_batch(msg, sk, k, curve=curve_id)
        for a, b in zip((pkx, pky, e1, bad1, r, s, e2, bad2), want):
            assert np.array_equal(a, b)
        assert bad1 == 2 and bad2 == 2
        hctx.close()
        actx = p2e.Context(device=0, asynchronous=True)
        d = _dev((msg, sk, k))
        pkx, pky, e1, rc1 = actx.ecdsa_public_key_batch(d[1], curve=curve_id)
        assert rc1 == 0 and actx.sync() == want[3]
        r, s, e2, rc2 = actx.ecdsa_sign_batch(*d, curve=curve_id)
        assert rc2 == 0 and actx.sync() == want[7]
        for a, b in zip((pkx, pky, e1, r, s, e2), want[0:3] + want[4:7]):
            assert np.array_equal(a.cpu().numpy(), b)
        actx.close()
    # misuse on the shared context
    L, h = ctx._L, ctx._h
    buf = torch.zeros((4, 32), dtype=torch.uint8, device="cuda")
    p, z = p2e._ptr(buf), C.c_void_p(0)
    good_key, good_sign = [p, p, p, p], [p, p, p, p, p, p]
    for curve, plan in ((7, 0), (0, 9), (-1, 0), (1, 3)):
        for rc in _raw(L, h, curve, plan, good_key, good_sign, 4):
            assert rc == -1 and L.p2e_last_error()
    for hole in range(4):
        ptrs = list(good_key)
        ptrs[hole] = z
        assert L.p2e_ecdsa_public_key_batch(h, 0, 0, *ptrs[:3], C.c_size_t(4), ptrs[3]) == -1 and b"null" in L.p2e_last_error()
    for hole in range(6):
        ptrs = list(good_sign)
        ptrs[hole] = z
        assert L.p2e_ecdsa_sign_batch(h, 1, 0, *ptrs[:5], C.c_size_t(4), ptrs[5]) == -1 and b"null" in L.p2e_last_error()
    assert _raw(L, h, 1, 0, good_key, good_sign, 0) == (0, 0)                   # n == 0
    # the context is still good for a fill, and the fill still matches the oracle
    sigs = p2e.synth_signatures(seed=9, n=64)
    cols, err, valid, bad = ctx.ecdsa_verify_witness_batch(*_dev(sigs))
    torch.cuda.synchronize()
    ref_cols, _aux, ref_err, _flags = oracle_c.verify_witness_aux(*sigs)
    assert bad == 0 and bool(valid.cpu().numpy().all())
    assert np.array_equal(cols.cpu().numpy().view(np.uint64)[:, :64], ref_cols)


def test_plain_c_client_signs_and_verifies(tmp_path):
    """examples/sign_verify.c: keys, signatures and the verifier's verdict from plain C"""
    from test_host import _build_c_example
    exe, env = _build_c_example(tmp_path, "sign_verify")
    r = subprocess.run([exe, "300"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "300 keys (0 flagged), 300 signatures (0 flagged), 299 verify, 0 flagged by the verifier" in r.stdout


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("curve_id", [0, 1])
def test_the_sixteen_group_patterns(curve_id, plan, ctx):
    """all 16 empty / non-empty patterns of the scalar's four 64-bit groups as one small batch (sign_inputs.edges has none of
    the six with exactly two empty groups): the secret key and the nonce walk the patterns, in opposite directions"""
    cv = S.CURVES[curve_id]
    sk = S.group_patterns(cv)
    k = S.group_patterns(cv, 0x6717)[::-1]
    rng = S.R.SplitMix64(0x6727 + curve_id)
    msg = [rng.below(1 << 256) for _ in sk]
    assert sorted({S.group_mask(v) for v in sk}) == list(range(16)) == sorted({S.group_mask(v) for v in k})
    pkx, pky, e1, bad1, r, s, e2, bad2 = _run(ctx, curve_id, plan, *[S.pack(v) for v in (msg, sk, k)])
    wx, wy, we1 = S.expect_keys(curve_id, sk)
    wr, ws, we2 = S.expect_sigs(curve_id, msg, sk, k)
    assert np.array_equal(e1, we1) and np.array_equal(e2, we2) and (bad1, bad2) == (2, 2)   # pattern 0000, twice
    for got, want, what in ((pkx, wx, "pkx"), (pky, wy, "pky"), (r, wr, "r"), (s, ws, "s")):
        _assert_equal(got, want, (curve_id, plan, what))
