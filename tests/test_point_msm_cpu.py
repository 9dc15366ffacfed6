"""The bucket-method multi-scalar multiplication (include/p2e.h p2e_point_msm) without a GPU.

The kernel bodies of csrc/pmsm.hpp compiled with g++ (tests/emu_msm, built on demand, -DP2E_F29_BOUNDS: a violated limb
bound of the lazy 29-bit arithmetic aborts the process) and run launch by launch with the device's plan, scratch layout and
index arithmetic, on both curves, on the inputs of tests/msm_native_inputs.py (nothing there uses the code under test).
Every byte of outx, outy, status and point_err and the return value are checked; the outputs are pre-filled with 0xAA.
The stand-alone sanitizer program of tests/emu_msm must exit 0."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import plonky2_ecdsa_amd as p2e
import msm_native_inputs as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "emu_msm")
ALL_WIDTHS = list(range(M.WINDOW_MIN, M.WINDOW_MAX + 1))


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def emu():
    lib, prog = os.path.join(HERE, "libp2e_emu_msm.so"), os.path.join(HERE, "msm_selftest")
    if not (os.path.exists(lib) and os.path.exists(prog)):
        subprocess.check_call(["make", "-s", "-C", HERE])
    L = C.CDLL(lib)
    L.emum_point_msm.restype = C.c_long
    return L


def plan_of(emu, curve_id, n, width):
    buf = (C.c_uint64 * 6)()
    assert emu.emum_plan(curve_id, C.c_size_t(n), C.c_uint(width), buf) == 0
    return dict(zip(("window_bits", "windows", "buckets", "seg", "scratch_bytes", "max_lane_additions"), [int(v) for v in buf]))


def run(emu, curve_id, case, width, with_point_err=True):
    """one call on 0xAA-filled outputs, everything checked; returns the per-launch maxima of one lane's point operations"""
    k, px, py, wantx, wanty = M.arrays(case)
    n = len(case.k)
    outx, outy, status = np.full(32, 0xAA, np.uint8), np.full(32, 0xAA, np.uint8), np.full(1, 0xAA, np.uint8)
    perr = np.full(n + 1, 0xAA, np.uint8) if with_point_err else None
    ops = (C.c_uint64 * 7)()
    pad = lambda a: np.concatenate([a, np.zeros((1, 32), np.uint8)])   # (n = 0: still a valid pointer)
    bad = emu.emum_point_msm(curve_id, C.c_uint(width), _p(pad(k)), _p(pad(px)), _p(pad(py)), C.c_size_t(n), _p(outx), _p(outy), _p(status),
                             _p(perr), ops)
    what = (curve_id, case.kind, n, width)
    assert bad == case.bad, what
    assert int(status[0]) == case.status, what
    assert outx.tobytes() == wantx.tobytes() and outy.tobytes() == wanty.tobytes(), what
    if case.status != M.MSM_OK:
        assert not outx.any() and not outy.any(), what
    if with_point_err:
        assert perr[:n].tolist() == case.point_err and perr[n] == 0xAA, what
    ops = [int(v) for v in ops]
    assert max(ops) <= plan_of(emu, curve_id, n, width)["max_lane_additions"], (what, ops)
    return ops


@pytest.fixture(scope="module")
def mixed_cases():
    return [M.mixed(c) for c in (0, 1)]


def test_input_sets_cover_what_they_claim(mixed_cases):
    assert (M.WINDOW_AUTO, M.WINDOW_MIN, M.WINDOW_MAX) == (p2e.MSM_WINDOW_AUTO, p2e.MSM_WINDOW_MIN, p2e.MSM_WINDOW_MAX)
    assert M.WINDOW_MIN <= 4 and M.WINDOW_MAX >= 12
    assert (M.MSM_OK, M.MSM_NEUTRAL, M.MSM_BAD_POINT) == (p2e.MSM_OK, p2e.MSM_NEUTRAL, p2e.MSM_BAD_POINT)
    for curve_id, cv in enumerate(M.CURVES):
        n, p = cv.n, cv.p
        pl = M.pool(curve_id)
        assert len({d for d, _ in pl}) == M.POOL and all(0 < d < n for d, _ in pl)
        assert all(cv.on_curve(pt) for _, pt in pl[:64]) and pl[3][1] == cv.mul(pl[3][0], cv.g)
        case, tags = mixed_cases[curve_id]
        assert len(case.k) == M.MIXED_N == len(tags) and case.status == M.MSM_OK and case.bad == 0
        by = lambda tag: [i for i, t in enumerate(tags) if t == tag]
        assert {case.k[i] for i in by("edge")} == {0, 1, 2, 3, n - 1, n, n + 1, (1 << 256) - 1}
        for width in M.BOUNDARY_WIDTHS:
            bits = {case.k[i].bit_length() - 1 for i in by("boundary%d" % width)}
            assert all(case.k[i] & (case.k[i] - 1) == 0 for i in by("boundary%d" % width))
            assert bits == {b for w in range(1, 256 // width + 1) for b in (width * w - 1, width * w, width * w + 1) if b < 256}
            halves, ones = sorted(case.k[i] for i in by("max_digit%d" % width))
            top = 252 // width
            assert ones < n and halves < n
            assert all((ones >> (width * w)) & ((1 << width) - 1) == (1 << width) - 1 for w in range(top))
            assert all((halves >> (width * w)) & ((1 << width) - 1) == 1 << (width - 1) for w in range(top))
        assert [case.k[i] for i in by("all_ones")] == [(1 << 255) - 1]
        same = by("same")
        assert len(same) == 40 and len({(case.k[i], case.pts[i]) for i in same}) == 1
        opp = by("opposite")
        pairs = {}
        for i in opp:
            pairs.setdefault((case.k[i], case.pts[i][0]), []).append(case.pts[i][1])
        assert len(pairs) == 6 and all(len(v) == 2 and sum(v) == p for v in pairs.values())
        assert len(by("neutral_point")) == 10 and all(case.pts[i] == (0, 0) for i in by("neutral_point"))
        assert all(cv.on_curve(pt) for i, pt in enumerate(case.pts) if tags[i] != "neutral_point")
        # the expectation of a small slice, summed on Python integers
        head = M.uniform(curve_id, 12, 0x77)
        total = None
        for k, pt in zip(head.k, head.pts):
            total = cv.add(total, cv.mul(k % n, pt))
        assert total == head.point
        c = M.cancelling(curve_id)
        assert c.point is None and c.status == M.MSM_NEUTRAL and (c.k[0] + c.k[1]) % n == 0 and c.pts[0] == c.pts[1]
        assert M.only_neutral_points(curve_id).status == M.MSM_NEUTRAL
        e = M.equal_scalars(curve_id, 70)
        assert len(set(e.k)) == 1 and e.status == M.MSM_OK
        a = M.arbitrary(curve_id)
        assert len(a.k) <= 200 and all(cv.on_curve(pt) for pt in a.pts)
        for kind in M.REJECT_KINDS:
            for position, at in (("first", 0), ("middle", 4), ("last", 8)):
                r = M.rejected(curve_id, kind, position)
                x, y = r.pts[at]
                assert r.point_err == [int(i == at) for i in range(9)] and (r.status, r.bad, r.point) == (M.MSM_BAD_POINT, 1, None)
                assert {"x_eq_p": x == p, "y_eq_p": y == p, "x_all_ones": x == (1 << 256) - 1,
                        "off_curve": x < p and y < p and not cv.on_curve((x, y))}[kind]
                assert all(cv.on_curve(pt) for i, pt in enumerate(r.pts) if i != at)


@pytest.mark.parametrize("n", M.SMALL_SIZES)
@pytest.mark.parametrize("curve_id", [0, 1])
def test_small_sizes(curve_id, n, emu):
    case = M.uniform(curve_id, n, 0x57 + n)
    for width in (M.WINDOW_AUTO, M.WINDOW_MIN, 8, M.WINDOW_MAX):
        run(emu, curve_id, case, width)


@pytest.mark.parametrize("curve_id", [0, 1])
def test_every_width_gives_the_same_bytes(curve_id, emu):
    case = M.uniform(curve_id, 257, 0x57 + 257)
    for width in [M.WINDOW_AUTO] + ALL_WIDTHS:
        run(emu, curve_id, case, width)
    assert plan_of(emu, curve_id, 257, M.WINDOW_AUTO)["window_bits"] in ALL_WIDTHS


@pytest.mark.parametrize("width", [M.WINDOW_AUTO, M.WINDOW_MIN, 8, M.WINDOW_MAX])
@pytest.mark.parametrize("curve_id", [0, 1])
def test_mixed_batch(curve_id, width, emu, mixed_cases):
    run(emu, curve_id, mixed_cases[curve_id][0], width)


@pytest.mark.parametrize("curve_id", [0, 1])
def test_neutral_sums_single_points_and_arbitrary_points(curve_id, emu):
    for width in (M.WINDOW_AUTO, M.WINDOW_MIN, 8, M.WINDOW_MAX):
        run(emu, curve_id, M.cancelling(curve_id), width)
        run(emu, curve_id, M.only_neutral_points(curve_id), width)
        for k in range(1, 18):
            run(emu, curve_id, M.single(curve_id, k), width)
    for width in (M.WINDOW_AUTO, 5, M.WINDOW_MAX):
        run(emu, curve_id, M.arbitrary(curve_id), width)


@pytest.mark.parametrize("with_point_err", [True, False])
@pytest.mark.parametrize("curve_id", [0, 1])
def test_rejected_points(curve_id, with_point_err, emu):
    for kind in M.REJECT_KINDS:
        for position in ("first", "middle", "last"):
            run(emu, curve_id, M.rejected(curve_id, kind, position), M.WINDOW_AUTO, with_point_err)
    run(emu, curve_id, M.rejected(curve_id, "off_curve", "middle"), M.WINDOW_MAX, with_point_err)


@pytest.mark.parametrize("curve_id", [0, 1])
def test_balance(curve_id, emu):
    """all scalars equal: every point of a window in one bucket, cut into segments; the counted operations of one lane stay
    inside the plan's bound for this input and for the uniform one"""
    plan = plan_of(emu, curve_id, M.BALANCE_N, M.WINDOW_AUTO)
    assert M.BALANCE_N > plan["seg"]
    ops_equal = run(emu, curve_id, M.equal_scalars(curve_id), M.WINDOW_AUTO)
    ops_uniform = run(emu, curve_id, M.uniform(curve_id, M.BALANCE_N, 0xBA1), M.WINDOW_AUTO)
    assert max(ops_equal) <= plan["max_lane_additions"] and max(ops_uniform) <= plan["max_lane_additions"]
    # launch 4 (segment sums) is cut at seg; launch 5 meets the whole bucket only as ceil(n / seg) partials
    assert ops_equal[3] == plan["seg"] and ops_equal[4] == -(-M.BALANCE_N // plan["seg"])


def test_plan_is_the_library_s_and_its_bound_is_small():
    L = p2e.lib()
    for curve_id in (0, 1):
        for n in (0, 1, 257, M.BALANCE_N, 1 << 16, 1 << 20):
            for width in [M.WINDOW_AUTO] + ALL_WIDTHS:
                plan = p2e.point_msm_plan(n, curve_id, width)
                assert plan["window_bits"] == (width or plan["window_bits"]) and M.WINDOW_MIN <= plan["window_bits"] <= M.WINDOW_MAX
                assert plan["windows"] * plan["window_bits"] >= 257 and plan["buckets"] == 1 << (plan["window_bits"] - 1)
                assert plan["seg"] >= 1 and plan["scratch_bytes"] > 0
        big = p2e.point_msm_plan(1 << 20, curve_id)
        # seg + n / seg at seg = 256 is 4 352; a lane-per-bucket design gives 2^20
        assert big["max_lane_additions"] < 1 << 14
    buf = (C.c_uint64 * 6)()
    assert L.p2e_point_msm_plan(2, C.c_size_t(1), C.c_uint(0), buf) == -1
    assert L.p2e_point_msm_plan(0, C.c_size_t(1), C.c_uint(M.WINDOW_MIN - 1), buf) == -1
    assert L.p2e_point_msm_plan(0, C.c_size_t(1), C.c_uint(M.WINDOW_MAX + 1), buf) == -1
    assert L.p2e_point_msm_plan(0, C.c_size_t(1), C.c_uint(0), None) == -1


def test_emulation_runs_the_library_s_plan(emu):
    for curve_id in (0, 1):
        for n in (0, 65, M.BALANCE_N, 1 << 20):
            for width in (M.WINDOW_AUTO, M.WINDOW_MIN, 8, M.WINDOW_MAX):
                assert plan_of(emu, curve_id, n, width) == p2e.point_msm_plan(n, curve_id, width)


def test_sanitizer_program_exits_zero(emu):
    """tests/emu_msm/msm_selftest under -fsanitize=address,undefined; its compiled-in vectors are the selftest cases as they are now"""
    with open(os.path.join(HERE, "msm_vectors.inc")) as f:
        assert f.read() == M.selftest_vectors(), "tests/emu_msm/msm_vectors.inc is stale: regenerate it from msm_native_inputs.selftest_vectors()"
    res = subprocess.run([os.path.join(HERE, "msm_selftest")], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr


def test_entry_points_exist_and_refuse_misuse_without_a_device():
    L = p2e.lib()
    assert "p2e_point_msm" in p2e.EXPORTS and "p2e_point_msm_plan" in p2e.EXPORTS and L.p2e_point_msm.restype is C.c_long
    buf = np.zeros(32, np.uint8)
    assert L.p2e_point_msm(None, 0, 0, _p(buf), _p(buf), _p(buf), C.c_size_t(1), _p(buf), _p(buf), _p(buf), None) == -1
