"""Point tables (include/p2e.h p2e_point_table_create and the calls that consume a table) without a GPU.

The bodies of csrc/point_table.hpp -- both build steps and the three calls -- compiled with g++ (tests/emu_table, built on
demand, -DP2E_F29_BOUNDS: a violated limb bound of the lazy 29-bit arithmetic aborts the process), on both curves.  The
built table of G against the generator's table byte for byte; every (w, d) entry of the keys against Python integers; every
byte of the three calls on the input set (tests/table_inputs.py: nothing there uses the code under test).  The stand-alone
sanitizer program of tests/emu_table must exit 0."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import plonky2_ecdsa_amd as p2e
import table_inputs as TI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "emu_table")
M = 4                  # G, -G, 2 G and a random key
F_COUNT = 200


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def emu():
    lib, prog = os.path.join(HERE, "libp2e_emu_table.so"), os.path.join(HERE, "table_selftest")
    if not (os.path.exists(lib) and os.path.exists(prog)):
        subprocess.check_call(["make", "-s", "-C", HERE])
    L = C.CDLL(lib)
    L.emut_build.restype = L.emut_call.restype = C.c_long
    L.emut_table_bytes.restype = C.c_size_t
    return L


@pytest.fixture(scope="module")
def tables(emu):
    """{curve: the table of the first M keys as (M, 66, 16, 2, 32) bytes}, built once"""
    out = {}
    for curve_id in (0, 1):
        px, py = TI.point_arrays(curve_id, M)
        tab = np.full(emu.emut_table_bytes(C.c_size_t(M)), 0xAA, np.uint8)
        perr = np.full(M, 0xAA, np.uint8)
        assert emu.emut_build(curve_id, _p(px), _p(py), C.c_size_t(M), _p(tab), _p(perr)) == 0 and not perr.any()
        out[curve_id] = tab
    return out


def call(emu, curve_id, op, tab, m, a, with_idx=True):
    n = a["err"].shape[0]
    o1, o2, err = np.full((n, 32), 0xAA, np.uint8), np.full((n, 32), 0xAA, np.uint8), np.full(n, 0xAA, np.uint8)
    bad = emu.emut_call(curve_id, TI.OPS.index(op), _p(tab), _p(a["idx"]) if with_idx else None, C.c_uint32(m), _p(a["a"]), _p(a["b"]),
                        _p(a["s"]), _p(o1), _p(o2), C.c_size_t(n), _p(err))
    return o1, o2, err, bad


def test_input_sets_cover_what_they_claim():
    for curve_id, cv in enumerate(TI.CURVES):
        n = cv.n
        for m in (1, 4, 65):
            X = {op: TI.set_x(curve_id, m, op) for op in TI.OPS}
            ks = {c.b for c in X["mul"]}
            assert ks >= {0, 1, n - 1, n, n + 1, (1 << 256) - 1, int("f" * 63, 16), int("0f" * 32, 16)}
            assert all({1 << (4 * w), 15 << (4 * w)} <= ks for w in range(64))
            assert all({1 << (4 * w), 15 << (4 * w)} <= {c.b for c in X["lincomb"] if c.a == 0} for w in range(64))
            assert all({1 << (4 * w), 15 << (4 * w)} <= {c.a for c in X["lincomb"] if c.b == 0} for w in range(64))
            for op in TI.OPS:
                assert {c.err for c in X[op]} == TI.CODES[op]                    # every code the call can emit
                assert {c.idx for c in X[op]} >= {0, m - 1, m, TI.IDX_MAX}
                assert all((c.err == TI.WIRE_BAD_INDEX) == (c.idx >= m) for c in X[op])
                assert all(c.out == TI.O and not c.valid for c in X[op] if c.err)
            kinds = lambda op, pre: [c for c in X[op] if c.kind.startswith(pre)]
            assert all(c.err == TI.WIRE_INFINITY for c in kinds("lincomb", "opposite") + kinds("lincomb", "both_"))
            assert all(c.err == 0 and c.out == cv.mul(2 * c.a % n, cv.g) for c in kinds("lincomb", "doubling"))
            assert all(c.a == 0 and c.err == 0 for c in kinds("lincomb", "a_zero")) and all(c.b == 0 and c.err == 0 for c in kinds("lincomb", "b_zero"))
            assert all(c.valid == 1 for c in kinds("verify", "valid") + kinds("verify", "msg_plus_n") + kinds("verify", "msg_zero"))
            assert all(c.valid == 0 and c.err == 0 for c in kinds("verify", "msg_altered") + kinds("verify", "r_altered") + kinds("verify", "s_altered"))
            assert all(c.err == TI.WIRE_SCALAR_RANGE for k in ("r_zero", "r_eq_n", "r_above_n", "r_max", "s_zero", "s_eq_n", "s_above_n", "s_max",
                                                               "r_plus_n", "both_zero") for c in kinds("verify", k))
        pts = TI.table_points(curve_id, 4)
        assert pts[:3] == (cv.g, cv.neg(cv.g), cv.mul(2, cv.g)) and all(cv.on_curve(p) for p in TI.table_points(curve_id))
        rows = TI.window_rows(curve_id, pts[3])
        assert rows[0][0] == rows[0][1] == pts[3] and rows[5][7] == cv.mul(7 << 20, pts[3]) and rows[65][15] == cv.mul(15 << 260, pts[3])


@pytest.mark.parametrize("curve_id", [0, 1])
def test_table_of_the_generator_is_the_library_s_own_table(curve_id, emu, tables):
    want = np.zeros(emu.emut_table_bytes(C.c_size_t(1)), np.uint8)
    emu.emut_generator_table(curve_id, _p(want))
    assert np.array_equal(tables[curve_id][:want.size], want)           # key 0 is G: byte for byte fixed_base_table_cv(G)
    assert TI.POINT_BYTES == want.size == p2e.POINT_TABLE_BYTES_PER_POINT


@pytest.mark.parametrize("curve_id", [0, 1])
def test_every_entry_of_every_key_equals_the_integers(curve_id, tables):
    tab = tables[curve_id].reshape(M, TI.FB_WINDOWS, 16, 2, 32)
    for j, pt in enumerate(TI.table_points(curve_id, M)):
        for w in range(TI.FB_WINDOWS):
            assert np.array_equal(tab[j, w], TI.window_bytes(curve_id, pt, w)), (curve_id, j, w)


@pytest.mark.parametrize("op", TI.OPS)
@pytest.mark.parametrize("curve_id", [0, 1])
def test_bodies_equal_the_expectation_on_every_element(curve_id, op, emu, tables):
    c = TI.batch(curve_id, M, op, len(TI.set_x(curve_id, M, op)) + F_COUNT)
    a = TI.arrays(c)
    assert set(np.unique(a["err"])) == TI.CODES[op] and sum(1 for x in c if x.kind == "F") == F_COUNT
    o1, o2, err, bad = call(emu, curve_id, op, tables[curve_id], M, a)
    diff = np.nonzero(err != a["err"])[0]
    assert diff.size == 0, (curve_id, op, "err", [(int(i), c[i].kind, int(err[i]), c[i].err) for i in diff[:8]])
    assert bad == np.count_nonzero(a["err"])
    if op == "verify":
        got = o1.reshape(-1)[:len(c)]
        diff = np.nonzero(got != a["valid"])[0]
        assert diff.size == 0, (curve_id, op, "valid", [(int(i), c[i].kind) for i in diff[:8]])
        assert (o1.reshape(-1)[len(c):] == 0xAA).all() and (o2 == 0xAA).all()      # n verdict bytes and nothing else
        return
    for got, want, what in ((o1, a["outx"], "outx"), (o2, a["outy"], "outy")):
        diff = np.nonzero((got != want).any(axis=1))[0]
        assert diff.size == 0, (curve_id, op, what, [(int(i), c[i].kind) for i in diff[:8]])


@pytest.mark.parametrize("curve_id", [0, 1])
def test_null_idx_means_point_zero(curve_id, emu, tables):
    c = [x for x in TI.set_x(curve_id, M, "mul") if x.idx == 0]
    a = TI.arrays(c)
    ox, oy, err, bad = call(emu, curve_id, "mul", tables[curve_id], M, a, with_idx=False)
    assert np.array_equal(ox, a["outx"]) and np.array_equal(oy, a["outy"]) and np.array_equal(err, a["err"]) and bad == np.count_nonzero(a["err"])


def test_a_rejected_point_builds_nothing(emu):
    for curve_id, cv in enumerate(TI.CURVES):
        px, py = TI.point_arrays(curve_id, M)
        px, py = px.copy(), py.copy()
        py[1, 0] ^= 1                       # off the curve
        px[2], py[2] = 0, 0                 # the neutral element
        px[3] = 0xFF                        # x = 2^256 - 1
        tab = np.full(emu.emut_table_bytes(C.c_size_t(M)), 0xAA, np.uint8)
        perr = np.full(M, 0xAA, np.uint8)
        assert emu.emut_build(curve_id, _p(px), _p(py), C.c_size_t(M), _p(tab), _p(perr)) == 3
        assert perr.tolist() == [0, TI.WIRE_NOT_ON_CURVE, TI.WIRE_INFINITY, TI.WIRE_COORD_RANGE] and (tab == 0xAA).all()


def test_sanitizer_program_exits_zero(emu):
    """tests/emu_table/table_selftest under -fsanitize=address,undefined; its compiled-in vectors are drawn from set X as it is
    now, lanes with idx >= m among them, against a table in an allocation of exactly its size"""
    with open(os.path.join(HERE, "table_vectors.inc")) as f:
        assert f.read() == TI.selftest_vectors(), "tests/emu_table/table_vectors.inc is stale: regenerate it from table_inputs.selftest_vectors()"
    res = subprocess.run([os.path.join(HERE, "table_selftest")], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr


def test_entry_points_exist_and_refuse_misuse_without_a_device():
    L = p2e.lib()
    for name in ("p2e_point_table_create", "p2e_point_table_num_points", "p2e_point_table_mul_batch", "p2e_point_table_lincomb_batch",
                 "p2e_ecdsa_verify_table_batch"):
        assert name in p2e.EXPORTS and getattr(L, name).restype is C.c_long
    buf = np.zeros(32, np.uint8)
    h = C.c_void_p(1)
    assert L.p2e_point_table_create(None, 0, _p(buf), _p(buf), C.c_size_t(1), None, C.byref(h)) == -1 and not h.value
    assert L.p2e_point_table_num_points(None) == -1 and L.p2e_point_table_curve(None) == -1
    assert L.p2e_point_table_read_window(None, None, C.c_size_t(0), 0, _p(buf)) == -1
    assert L.p2e_point_table_mul_batch(None, None, None, _p(buf), _p(buf), _p(buf), C.c_size_t(1), _p(buf)) == -1
    assert L.p2e_point_table_lincomb_batch(None, None, None, _p(buf), _p(buf), _p(buf), _p(buf), C.c_size_t(1), _p(buf)) == -1
    assert L.p2e_ecdsa_verify_table_batch(None, None, None, _p(buf), _p(buf), _p(buf), C.c_size_t(1), _p(buf), _p(buf)) == -1
    L.p2e_point_table_destroy(None, None)                                   # a null table: no-op
    assert (p2e.WIRE_BAD_INDEX, p2e.WIRE_SCALAR_RANGE, p2e.WIRE_INFINITY) == (TI.WIRE_BAD_INDEX, TI.WIRE_SCALAR_RANGE, TI.WIRE_INFINITY)
    assert p2e.POINT_TABLE_MAX_POINTS == 65536


def test_example_compiles_against_the_header(tmp_path):
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                           os.path.join(ROOT, "examples", "verify_known_keys.c"), "-o", str(tmp_path / "verify_known_keys.o")])
