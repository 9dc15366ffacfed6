"""Public-key recovery and the recoverable signer on the GPU (include/p2e.h p2e_ecdsa_recover_batch /
p2e_ecdsa_sign_recoverable_batch), both curves.

Expectations come from tests/recover_inputs.py (set X: the definition written with Python integers and oracle/p2e_ref.py's
big-int curve; set S: the signing tests' batch, points from the C oracle's fixed-base walk, low-s twins) and from the calls
the project already has (ecdsa_public_key_batch, ecdsa_sign_batch, the two verifiers)."""
import os
import subprocess

import numpy as np
import pytest
import torch

import plonky2_ecdsa_amd as p2e
import recover_inputs as RI
import sign_inputs as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_MAIN = 4161            # 65 full waves + one lane: the last workgroup has a single live lane
PLANS = [S.PLAN_LANE, S.PLAN_QUAD]


@pytest.fixture(scope="module")
def ctx():
    return p2e.Context(device=0)


@pytest.fixture(scope="module")
def main_cases():
    """per curve: X, S, the low-s twins of S, one more element of S, X -- N_MAIN cases and their arrays, computed once.
    S = elements of the signing tests' N_MAIN batch (same seeds): both copies of E's tail (0 and n among them) and filler."""
    out = []
    for curve_id in (0, 1):
        x = list(RI.set_x(curve_id))
        m = (N_MAIN - 2 * len(x)) // 2
        idx = list(range(900, 900 + (m + 1) // 2)) + list(range(N_MAIN - 900 - m // 2, N_MAIN - 900))
        s = RI.set_s(curve_id, N_MAIN, (0x151 + curve_id, 0x161 + curve_id, 0x171 + curve_id), idx)
        cases = x + s + RI.low_s(curve_id, s) + s[1000:1001] + x
        assert len(cases) == N_MAIN and len(s) == m
        out.append((cases, RI.arrays(cases)))
    return out


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _recover(ctx, curve_id, a, lo=0, hi=None):
    """(pkx, pky, err, bad) as numpy for elements lo .. hi of the arrays, outputs pre-filled with 0xAA"""
    d = [_dev(a[k][lo:hi]) for k in ("msg", "r", "s", "v")]
    n = d[0].shape[0]
    pre = lambda *shape: torch.full(shape, 0xAA, dtype=torch.uint8, device="cuda")
    pkx, pky, err, bad = ctx.ecdsa_recover_batch(*d, curve=curve_id, pkx=pre(n, 32), pky=pre(n, 32), err=pre(n))
    torch.cuda.synchronize()
    return pkx.cpu().numpy(), pky.cpu().numpy(), err.cpu().numpy(), bad


def _check(got, a, cases, lo, hi, what):
    pkx, pky, err, bad = got
    want_err = a["err"][lo:hi]
    diff = np.nonzero(err != want_err)[0]
    assert diff.size == 0, (what, "err", [(int(i), cases[lo + i].kind, int(err[i]), int(want_err[i])) for i in diff[:8]])
    assert bad == np.count_nonzero(want_err)
    for g, w, name in ((pkx, a["pkx"][lo:hi], "pkx"), (pky, a["pky"][lo:hi], "pky")):
        diff = np.nonzero((g != w).any(axis=1))[0]      # flagged elements hold zeros in both: every element is compared
        assert diff.size == 0, (what, name, [(int(i), cases[lo + i].kind) for i in diff[:8]])


@pytest.mark.parametrize("curve_id", [0, 1])
def test_every_output_byte_on_the_main_batch(curve_id, ctx, main_cases):
    cases, a = main_cases[curve_id]
    assert set(np.unique(a["err"])) == {0, RI.ERR_POINT_AT_INFINITY, RI.ERR_NOT_RECOVERABLE}
    _check(_recover(ctx, curve_id, a), a, cases, 0, N_MAIN, curve_id)


@pytest.mark.parametrize("n", [1, 3, 64, 257])
@pytest.mark.parametrize("curve_id", [0, 1])
def test_small_batches(curve_id, n, ctx, main_cases):
    cases, a = main_cases[curve_id]
    for lo in (0, len(RI.set_x(curve_id)) - 2, N_MAIN - n):      # the head of X, X into S, the tail
        _check(_recover(ctx, curve_id, a, lo, lo + n), a, cases, lo, lo + n, (curve_id, n, lo))


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("curve_id", [0, 1])
def test_device_round_trip_sign_recover_verify(curve_id, plan, ctx):
    """sign recoverably -> recover -> equals the key call's output and verifies; nothing passes through the host between"""
    n = 1024
    cv = S.CURVES[curve_id]
    rng = S.R.SplitMix64(0x7EC + curve_id)
    msg, sk, k = [_dev(S.pack([rng.below(cv.n) for _ in range(n)])) for _ in range(3)]
    r, s, v, e1, bad1 = ctx.ecdsa_sign_recoverable_batch(msg, sk, k, curve=curve_id, plan=plan)
    pkx, pky, e2, bad2 = ctx.ecdsa_recover_batch(msg, r, s, v, curve=curve_id)
    wx, wy, e3, bad3 = ctx.ecdsa_public_key_batch(sk, curve=curve_id, plan=plan)
    if curve_id == 0:
        e4, valid, bad4 = ctx.ecdsa_verify_batch(msg, r, s, pkx, pky)
    else:
        prog = p2e.CurveProgram(ctx, p2e.CP_VERIFY, p2e.CURVE_P256, blind=cv.mul(0xB11D, cv.g))
        e4, valid, bad4 = prog.verify_batch(msg, r, s, pkx, pky)
        torch.cuda.synchronize()
        prog.close()
    qx, qy, e5, bad5 = ctx.ecdsa_recover_batch(msg, r, s, v ^ 1, curve=curve_id)      # one bit of v flipped
    torch.cuda.synchronize()
    assert (bad1, bad2, bad3, bad4, bad5) == (0, 0, 0, 0, 0)
    assert torch.equal(pkx, wx) and torch.equal(pky, wy) and int(v.max()) <= 3
    assert bool((valid == 1).all())
    other = list(zip(S.unpack(qx.cpu().numpy()), S.unpack(qy.cpu().numpy())))
    mine = list(zip(S.unpack(pkx.cpu().numpy()), S.unpack(pky.cpu().numpy())))
    assert all(a != b and cv.on_curve(b) for a, b in zip(mine, other))


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("curve_id", [0, 1])
def test_recoverable_signer_equals_the_plain_signer_on_the_edge_batch(curve_id, plan, ctx):
    cv = S.CURVES[curve_id]
    sk, k = S.batch(cv, N_MAIN, 0x151 + curve_id, shift=1), S.batch(cv, N_MAIN, 0x161 + curve_id)
    msg = S.batch(cv, N_MAIN, 0x171 + curve_id, shift=500)
    d = [_dev(S.pack(x)) for x in (msg, sk, k)]
    pre = lambda *shape: torch.full(shape, 0xAA, dtype=torch.uint8, device="cuda")
    r0, s0, e0, bad0 = ctx.ecdsa_sign_batch(*d, curve=curve_id, plan=plan, r=pre(N_MAIN, 32), s=pre(N_MAIN, 32))
    r1, s1, v1, e1, bad1 = ctx.ecdsa_sign_recoverable_batch(*d, curve=curve_id, plan=plan, r=pre(N_MAIN, 32), s=pre(N_MAIN, 32), v=pre(N_MAIN))
    torch.cuda.synchronize()
    assert bad0 == bad1 == 4 and torch.equal(r0, r1) and torch.equal(s0, s1) and torch.equal(e0, e1)
    v1 = v1.cpu().numpy()
    assert int(v1.max()) <= 3 and not v1[e1.cpu().numpy() != 0].any()
    # v against the oracle's points on the elements of set S (the point cache already holds them)
    idx = list(range(900, 1100))
    pts = S.base_points(curve_id, [k[i] % cv.n for i in idx])
    want = [0 if k[i] % cv.n == 0 else (pts[k[i] % cv.n][1] & 1) | (2 if pts[k[i] % cv.n][0] >= cv.n else 0) for i in idx]
    assert v1[idx].tolist() == want


@pytest.mark.parametrize("curve_id", [0, 1])
def test_host_pointer_and_async_contexts_give_the_same_bytes(curve_id, ctx, main_cases):
    cases, a = main_cases[curve_id]
    n = 257
    want = _recover(ctx, curve_id, a, 0, n)
    _check(want, a, cases, 0, n, curve_id)
    host = [np.ascontiguousarray(a[k][:n]) for k in ("msg", "r", "s", "v")]
    hctx = p2e.Context(device=0, host_pointers=True)
    got = hctx.ecdsa_recover_batch(*host, curve=curve_id)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    cv = S.CURVES[curve_id]
    rng = S.R.SplitMix64(0xA5 + curve_id)
    trio = [S.pack([rng.below(cv.n) for _ in range(n)]) for _ in range(3)]
    sig_want = [t.cpu().numpy() if torch.is_tensor(t) else t for t in ctx.ecdsa_sign_recoverable_batch(*[_dev(t) for t in trio], curve=curve_id)]
    for g, w in zip(hctx.ecdsa_sign_recoverable_batch(*trio, curve=curve_id), sig_want):
        assert np.array_equal(g, w)
    hctx.close()
    actx = p2e.Context(device=0, asynchronous=True)
    pkx, pky, err, rc = actx.ecdsa_recover_batch(*[_dev(h) for h in host], curve=curve_id)
    assert rc == 0 and actx.sync() == want[3]
    for g, w in zip((pkx, pky, err), want):
        assert np.array_equal(g.cpu().numpy(), w)
    r, s, v, e, rc = actx.ecdsa_sign_recoverable_batch(*[_dev(t) for t in trio], curve=curve_id)
    assert rc == 0 and actx.sync() == 0
    for g, w in zip((r, s, v, e), sig_want):
        assert np.array_equal(g.cpu().numpy(), w)
    actx.close()


def test_plain_c_client_signs_recovers_and_verifies(tmp_path):
    """examples/recover_fill.c: device buffers from plain C through the three calls"""
    exe = str(tmp_path / "recover_fill")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "recover_fill.c"), "-L", os.path.join(ROOT, "plonky2-ecdsa_amd"), "-lp2e_hip",
                           "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe])
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "plonky2-ecdsa_amd") + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""),
               GPU_MAX_HW_QUEUES="8")
    r = subprocess.run([exe, "300"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "300 signatures (0 flagged), 300 keys recovered (0 flagged), 300 verify (0 flagged), recovered keys equal sk G" in r.stdout
