"""The bucket-method multi-scalar multiplication on the device (include/p2e.h p2e_point_msm) through the C ABI: the inputs
and expectations of tests/msm_native_inputs.py (nothing there uses the code under test), every byte of outx, outy, status
and point_err and the return value, on both curves; device pointers, host pointers and asynchronous contexts; scratch
reuse and regrowth; a device-only round trip through the key derivation; the plain C client."""
import os
import subprocess

import numpy as np
import pytest
import torch

import plonky2_ecdsa_amd as p2e
import msm_native_inputs as M
import sign_inputs as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (M.WINDOW_AUTO, M.WINDOW_MIN, 8, M.WINDOW_MAX)


@pytest.fixture(scope="module")
def ctx():
    return p2e.Context(device=0)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(t):
    return t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def check(c, curve_id, case, width, with_point_err=True, device=True, sync=None):
    """one call on 0xAA-filled outputs, everything checked"""
    k, px, py, wantx, wanty = M.arrays(case)
    n = len(case.k)
    put = _dev if device else (lambda a: np.ascontiguousarray(a))
    fill = lambda m: put(np.full(m, 0xAA, np.uint8))
    row = np.zeros((1, 32), np.uint8)                       # (n = 0: the buffers still exist)
    k, px, py = [np.concatenate([a, row]) for a in (k, px, py)]
    outx, outy, status, perr = fill(32), fill(32), fill(1), (fill(n + 1) if with_point_err else None)
    _, _, _, _, bad = c.point_msm(put(k), put(px), put(py), curve=curve_id, window_bits=width, outx=outx, outy=outy, status=status,
                                  point_err=perr, want_point_err=with_point_err, n=n)
    if sync is not None:
        assert bad == 0
        bad = sync()
    what = (curve_id, case.kind, n, width)
    assert bad == case.bad, what
    assert int(_host(status)[0]) == case.status, what
    assert _host(outx).tobytes() == wantx.tobytes() and _host(outy).tobytes() == wanty.tobytes(), what
    if with_point_err:
        got = _host(perr)
        assert got[:n].tolist() == case.point_err and got[n] == 0xAA, what


@pytest.fixture(scope="module")
def mixed_cases():
    return [M.mixed(c)[0] for c in (0, 1)]


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("curve_id", [0, 1])
def test_small_sizes_and_special_batches(curve_id, width, ctx):
    for n in M.SMALL_SIZES:
        check(ctx, curve_id, M.uniform(curve_id, n, 0x57 + n), width)
    check(ctx, curve_id, M.cancelling(curve_id), width)
    check(ctx, curve_id, M.only_neutral_points(curve_id), width)
    for k in range(1, 18):
        check(ctx, curve_id, M.single(curve_id, k), width)
    check(ctx, curve_id, M.arbitrary(curve_id), width)


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("curve_id", [0, 1])
def test_mixed_batch(curve_id, width, ctx, mixed_cases):
    check(ctx, curve_id, mixed_cases[curve_id], width)


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("curve_id", [0, 1])
def test_65_waves_and_one_lane(curve_id, width, ctx):
    """n = 4 161, uniform scalars and all scalars equal (every point of a window in one bucket, cut into segments)"""
    assert M.BALANCE_N > p2e.point_msm_plan(M.BALANCE_N, curve_id, width)["seg"]
    check(ctx, curve_id, M.uniform(curve_id, M.BALANCE_N, 0xBA1), width)
    check(ctx, curve_id, M.equal_scalars(curve_id), width)


@pytest.mark.parametrize("with_point_err", [True, False])
@pytest.mark.parametrize("curve_id", [0, 1])
def test_rejected_points(curve_id, with_point_err, ctx):
    for kind in M.REJECT_KINDS:
        for position in ("first", "middle", "last"):
            check(ctx, curve_id, M.rejected(curve_id, kind, position), M.WINDOW_AUTO, with_point_err)


@pytest.mark.parametrize("curve_id", [0, 1])
def test_host_pointer_and_async_contexts(curve_id, mixed_cases):
    cases = [mixed_cases[curve_id], M.uniform(curve_id, 65, 0x57 + 65), M.rejected(curve_id, "off_curve", "last"), M.uniform(curve_id, 0, 0x57)]
    hctx = p2e.Context(device=0, host_pointers=True)
    for case in cases:
        for with_point_err in (True, False):
            check(hctx, curve_id, case, M.WINDOW_AUTO, with_point_err, device=False)
    hctx.close()
    actx = p2e.Context(device=0, asynchronous=True)
    for case in cases:
        check(actx, curve_id, case, M.WINDOW_AUTO, sync=actx.sync)
    actx.close()


@pytest.mark.parametrize("curve_id", [0, 1])
def test_scratch_is_reused_and_regrown(curve_id, mixed_cases):
    """small, larger, small again on one context; then a wider plan (more scratch for the same n)"""
    c = p2e.Context(device=0)
    small, large = M.uniform(curve_id, 63, 0x57 + 63), mixed_cases[curve_id]
    assert p2e.point_msm_plan(63, curve_id)["scratch_bytes"] < p2e.point_msm_plan(M.MIXED_N, curve_id)["scratch_bytes"]
    for case in (small, large, small, large):
        check(c, curve_id, case, M.WINDOW_AUTO)
    check(c, curve_id, small, M.WINDOW_MAX)
    check(c, curve_id, small, M.WINDOW_AUTO)
    c.close()


@pytest.mark.parametrize("curve_id", [0, 1])
def test_device_round_trip_with_the_key_derivation(curve_id, ctx):
    """ecdsa_public_key_batch(sk) -> point_msm(k, pk) equals ecdsa_public_key_batch(sum k_i sk_i mod n); nothing visits the host"""
    cv = S.CURVES[curve_id]
    n = 3000
    rng = S.R.SplitMix64(0xD0 + curve_id)
    sk = [rng.below(1 << 256) for _ in range(n)]
    k = [rng.below(1 << 256) for _ in range(n)]
    sk[7] = cv.n                                   # a flagged key: (0, 0), the neutral element, contributes nothing
    total = sum((a % cv.n) * (b % cv.n) for a, b in zip(k, sk)) % cv.n
    pkx, pky, err, bad = ctx.ecdsa_public_key_batch(_dev(S.pack(sk)), curve=curve_id)
    assert bad == 1
    outx, outy, status, perr, rejected = ctx.point_msm(_dev(S.pack(k)), pkx, pky, curve=curve_id)
    wx, wy, werr, wbad = ctx.ecdsa_public_key_batch(_dev(S.pack([total])), curve=curve_id)
    assert rejected == 0 and wbad == 0 and int(_host(status)[0]) == M.MSM_OK and not _host(perr).any()
    assert _host(outx).tobytes() == _host(wx)[0].tobytes() and _host(outy).tobytes() == _host(wy)[0].tobytes()
    want = S.base_points(curve_id, [total])[total]
    assert int.from_bytes(_host(outx).tobytes(), "little") == want[0] and int.from_bytes(_host(outy).tobytes(), "little") == want[1]


@pytest.mark.parametrize("curve_id", [0, 1])
def test_uniform_batch_of_2_to_the_16(curve_id, ctx):
    check(ctx, curve_id, M.uniform(curve_id, 1 << 16, 0x1616 + curve_id), M.WINDOW_AUTO)


def test_misuse_is_refused(ctx):
    buf = _dev(np.zeros((1, 32), np.uint8))
    for kwargs in (dict(curve=2), dict(window_bits=M.WINDOW_MIN - 1), dict(window_bits=M.WINDOW_MAX + 1)):
        with pytest.raises(p2e.P2EError):
            ctx.point_msm(buf, buf, buf, **kwargs)


def test_plain_c_client_sums_keys(tmp_path):
    """examples/msm_sum.c: device buffers from plain C through the key derivation and the sum"""
    exe = str(tmp_path / "msm_sum")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "msm_sum.c"), "-L", os.path.join(ROOT, "plonky2-ecdsa_amd"), "-lp2e_hip",
                           "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe])
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "plonky2-ecdsa_amd") + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""),
               GPU_MAX_HW_QUEUES="8")
    r = subprocess.run([exe, "1000"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("1000 keys (0 flagged)") == 2 and r.stdout.count("the sum equals the key of the summed scalar") == 2


@pytest.mark.parametrize("width", [7, 11])
@pytest.mark.parametrize("curve_id", [0, 1])
def test_widths_seven_and_eleven(curve_id, width, ctx, mixed_cases):
    """the two forced widths no other device test takes (AUTO gives 5, 6, 9 or 10 at the sizes used): neither divides 256, and
    their windows have two (7 bits) and thirty-two (11 bits) chunks"""
    check(ctx, curve_id, mixed_cases[curve_id], width)
    check(ctx, curve_id, M.uniform(curve_id, 257, 0x57 + 257), width)
