"""SEC1 keys and DER / compact signatures in wire form (include/p2e.h p2e_point_decode_batch, p2e_point_encode_batch,
p2e_sig_decode_batch, p2e_sig_encode_batch) without a GPU.

The kernel bodies of csrc/wire.hpp compiled with g++ (tests/emu_wire, built on demand, limb-bound tracker on) against
tests/wire_inputs.py: the main batches of all four calls on both curves in every form and under every flag value -- every
output byte, every code, the return value, the concatenated buffer at all four alignments of its first byte, one guard row
of 0xAA on each side of every output; the published generators literally; the round trips; the stand-alone sanitizer
program of tests/emu_wire must exit 0; the committed resource file lists no private segment for any new kernel."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import plonky2_ecdsa_amd as p2e
import wire_inputs as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "emu_wire")
N = W.N_MAIN
CURVE_IDS = [0, 1]
POINT_FORMS = [W.SEC1_COMPRESSED, W.SEC1_UNCOMPRESSED]
SIG_FORMS = [W.SIG_DER, W.SIG_COMPACT64, W.SIG_COMPACT65]


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def emu():
    lib, prog = os.path.join(HERE, "libp2e_emu_wire.so"), os.path.join(HERE, "wire_selftest")
    if not (os.path.exists(lib) and os.path.exists(prog)):
        subprocess.check_call(["make", "-s", "-C", HERE])
    L = C.CDLL(lib)
    L.emuw_point_decode.restype = L.emuw_point_encode.restype = L.emuw_sig_decode.restype = L.emuw_sig_encode.restype = C.c_long
    return L


class Box:
    """an output of `rows` x `width` bytes between two guard rows of 0xAA"""

    def __init__(self, rows, width):
        self.all = np.full((rows + 2, width), 0xAA, np.uint8)
        self.out = self.all[1:rows + 1]

    def intact(self):
        return bool((self.all[0] == 0xAA).all() and (self.all[-1] == 0xAA).all())


def _rows_differ(got, want):
    return np.nonzero((np.asarray(got).reshape(len(want), -1) != np.asarray(want).reshape(len(want), -1)).any(axis=1))[0]


# ---- 1. main batches --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve_id", CURVE_IDS)
def test_every_key_of_the_main_batch_decodes_to_the_expected_bytes(curve_id, emu):
    data, offsets, real, wx, wy, werr = W.key_batch(curve_id)
    base = np.zeros(data.size + 32, np.uint8)
    for shift in range(4):
        start = (-base.ctypes.data) % 4 + 4 + shift
        view = base[start:start + data.size]
        view[:] = data
        assert view.ctypes.data % 4 == shift
        px, py, err = Box(N, 32), Box(N, 32), Box(N, 1)
        bad = emu.emuw_point_decode(curve_id, _p(view), _p(offsets), _p(px.out), _p(py.out), C.c_size_t(N), _p(err.out))
        diff = np.nonzero(err.out[:, 0] != werr)[0]
        assert diff.size == 0, (shift, [(int(i), real[i][:4].hex(), len(real[i]), int(err.out[i, 0]), int(werr[i])) for i in diff[:8]])
        assert _rows_differ(px.out, wx).size == 0 and _rows_differ(py.out, wy).size == 0
        assert bad == int((werr != 0).sum()) and px.intact() and py.intact() and err.intact()


@pytest.mark.parametrize("form", POINT_FORMS)
@pytest.mark.parametrize("curve_id", CURVE_IDS)
def test_every_key_of_the_main_batch_encodes_to_the_expected_bytes(curve_id, form, emu):
    pts = W.point_values(curve_id)
    want, werr = W.point_encode_want(curve_id, form)
    out, err = Box(N, W.POINT_STRIDE[form]), Box(N, 1)
    bad = emu.emuw_point_encode(curve_id, form, _p(W.pack([q[0] for q in pts])), _p(W.pack([q[1] for q in pts])), _p(out.out), C.c_size_t(N),
                                _p(err.out))
    assert np.array_equal(err.out[:, 0], werr) and _rows_differ(out.out, want).size == 0
    assert bad == int((werr != 0).sum()) and out.intact() and err.intact()


@pytest.mark.parametrize("flags", W.DECODE_FLAGS)
@pytest.mark.parametrize("curve_id", CURVE_IDS)
def test_every_der_signature_of_the_main_batch_decodes_to_the_expected_bytes(curve_id, flags, emu):
    data, offsets, real = W.der_batch(curve_id)
    wr, ws, werr = W.der_want(curve_id, flags)
    base = np.zeros(data.size + 32, np.uint8)
    for shift in range(4):
        start = (-base.ctypes.data) % 4 + 4 + shift
        view = base[start:start + data.size]
        view[:] = data
        r, s, err = Box(N, 32), Box(N, 32), Box(N, 1)
        bad = emu.emuw_sig_decode(curve_id, W.SIG_DER, flags, _p(view), _p(offsets), _p(r.out), _p(s.out), None, C.c_size_t(N), _p(err.out))
        diff = np.nonzero(err.out[:, 0] != werr)[0]
        assert diff.size == 0, (shift, [(int(i), real[i].hex(), int(err.out[i, 0]), int(werr[i])) for i in diff[:4]])
        assert _rows_differ(r.out, wr).size == 0 and _rows_differ(s.out, ws).size == 0
        assert bad == int((werr != 0).sum()) and r.intact() and s.intact() and err.intact()


@pytest.mark.parametrize("flags", W.DECODE_FLAGS)
@pytest.mark.parametrize("form", [W.SIG_COMPACT64, W.SIG_COMPACT65])
@pytest.mark.parametrize("curve_id", CURVE_IDS)
def test_every_compact_signature_of_the_main_batch_decodes_to_the_expected_bytes(curve_id, form, flags, emu):
    rows = W.compact_batch(curve_id, form)
    wr, ws, wv, werr = W.compact_want(curve_id, form, flags)
    base = np.zeros(rows.size + 32, np.uint8)
    for shift in range(4):
        start = (-base.ctypes.data) % 4 + 4 + shift
        view = base[start:start + rows.size]
        view[:] = rows.reshape(-1)
        r, s, v, err = Box(N, 32), Box(N, 32), Box(N, 1), Box(N, 1)
        bad = emu.emuw_sig_decode(curve_id, form, flags, _p(view), None, _p(r.out), _p(s.out), _p(v.out), C.c_size_t(N), _p(err.out))
        assert np.array_equal(err.out[:, 0], werr) and _rows_differ(r.out, wr).size == 0 and _rows_differ(s.out, ws).size == 0
        if form == W.SIG_COMPACT65:
            assert np.array_equal(v.out[:, 0], wv)
        else:
            assert (v.out == 0xAA).all()                                  # v is not looked at outside COMPACT65
        assert bad == int((werr != 0).sum()) and r.intact() and s.intact() and v.intact() and err.intact()
    # v is nullable in COMPACT65
    r, s, err = Box(N, 32), Box(N, 32), Box(N, 1)
    assert emu.emuw_sig_decode(curve_id, form, flags, _p(rows), None, _p(r.out), _p(s.out), None, C.c_size_t(N), _p(err.out)) == int((werr != 0).sum())
    assert _rows_differ(s.out, ws).size == 0


@pytest.mark.parametrize("flags", W.ENCODE_FLAGS)
@pytest.mark.parametrize("form", SIG_FORMS)
@pytest.mark.parametrize("curve_id", CURVE_IDS)
def test_every_signature_of_the_main_batch_encodes_to_the_expected_bytes(curve_id, form, flags, emu):
    vals = W.compact_values(curve_id)
    want, wlen, werr = W.sig_encode_want(curve_id, form, flags)
    out, out_len, err = Box(N, W.SIG_STRIDE[form]), Box(N, 1), Box(N, 1)
    v = np.array([q[2] for q in vals], np.uint8)
    bad = emu.emuw_sig_encode(curve_id, form, flags, _p(W.pack([q[0] for q in vals])), _p(W.pack([q[1] for q in vals])), _p(v), _p(out.out),
                              _p(out_len.out), C.c_size_t(N), _p(err.out))
    assert np.array_equal(err.out[:, 0], werr) and _rows_differ(out.out, want).size == 0
    if form == W.SIG_DER:
        assert np.array_equal(out_len.out[:, 0], wlen) and set(wlen[werr == 0]) <= set(range(8, 73)) and 8 in wlen
        assert (72 in wlen) == (flags == 0)                               # 72 bytes need a high s: r = s = n - 1
    else:
        assert (out_len.out == 0xAA).all()
    assert bad == int((werr != 0).sum()) and out.intact() and out_len.intact() and err.intact()


# ---- 2. published bytes -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve_id", CURVE_IDS)
def test_published_generators_decode_to_the_projects_constants_and_encode_back(curve_id, emu):
    comp, unc = (bytes.fromhex(h) for h in W.SEC2_G[curve_id])
    gx, gy = W.CURVES[curve_id].g
    data = np.frombuffer(comp + unc + b"\0", np.uint8).copy()
    offsets = np.array([0, 33, 98], np.uint64)
    px, py, err = np.zeros((2, 32), np.uint8), np.zeros((2, 32), np.uint8), np.zeros(2, np.uint8)
    assert emu.emuw_point_decode(curve_id, _p(data), _p(offsets), _p(px), _p(py), C.c_size_t(2), _p(err)) == 0
    assert W.unpack(px) == [gx, gx] and W.unpack(py) == [gy, gy] and not err.any()
    for form, want in ((W.SEC1_COMPRESSED, comp), (W.SEC1_UNCOMPRESSED, unc)):
        out = np.zeros((1, len(want)), np.uint8)
        assert emu.emuw_point_encode(curve_id, form, _p(W.pack([gx])), _p(W.pack([gy])), _p(out), C.c_size_t(1), _p(err)) == 0
        assert out.tobytes() == want


# ---- 3. round trips ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve_id", CURVE_IDS)
def test_key_round_trips(curve_id, emu):
    _, pts = W.valid_keys(curve_id)
    n = len(pts)
    x, y = W.pack([q[0] for q in pts]), W.pack([q[1] for q in pts])
    for form in POINT_FORMS:
        stride = W.POINT_STRIDE[form]
        out, err = np.zeros((n, stride), np.uint8), np.zeros(n, np.uint8)
        assert emu.emuw_point_encode(curve_id, form, _p(x), _p(y), _p(out), C.c_size_t(n), _p(err)) == 0
        offsets = (np.arange(n + 1, dtype=np.uint64) * stride)
        data = np.append(out.reshape(-1), np.zeros(4, np.uint8))
        bx, by = np.zeros((n, 32), np.uint8), np.zeros((n, 32), np.uint8)
        assert emu.emuw_point_decode(curve_id, _p(data), _p(offsets), _p(bx), _p(by), C.c_size_t(n), _p(err)) == 0
        assert np.array_equal(bx, x) and np.array_equal(by, y)                                   # decode(encode(x)) = x
    # encode(decode(b)) = b for every valid element of the main batch, in the form it came in
    data, offsets, real, wx, wy, werr = W.key_batch(curve_id)
    for form in POINT_FORMS:
        idx = [i for i in range(N) if werr[i] == 0 and len(real[i]) == W.POINT_STRIDE[form]]
        out, err = np.zeros((len(idx), W.POINT_STRIDE[form]), np.uint8), np.zeros(len(idx), np.uint8)
        px, py = np.ascontiguousarray(wx[idx]), np.ascontiguousarray(wy[idx])
        assert len(idx) > W.N_VALID
        assert emu.emuw_point_encode(curve_id, form, _p(px), _p(py), _p(out), C.c_size_t(len(idx)), _p(err)) == 0
        assert [bytes(row) for row in out] == [real[i] for i in idx]


@pytest.mark.parametrize("curve_id", CURVE_IDS)
def test_signature_round_trips_and_the_low_s_twin(curve_id, emu):
    cv = W.CURVES[curve_id]
    sigs = W.valid_sigs(curve_id)
    n = len(sigs)
    r, s = W.pack([q[1] for q in sigs]), W.pack([q[2] for q in sigs])
    v = np.array([q[3] for q in sigs], np.uint8)
    twin_s = W.pack([min(q[2], cv.n - q[2]) for q in sigs])
    twin_v = np.array([q[3] ^ (q[2] > (cv.n - 1) // 2) for q in sigs], np.uint8)
    assert 100 < int((twin_v != v).sum()) < 200
    for form in SIG_FORMS:
        stride = W.SIG_STRIDE[form]
        for flags in W.ENCODE_FLAGS:
            out, out_len, err = np.zeros((n, stride), np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
            assert emu.emuw_sig_encode(curve_id, form, flags, _p(r), _p(s), _p(v), _p(out), _p(out_len), C.c_size_t(n), _p(err)) == 0
            if form == W.SIG_DER:
                offsets = np.zeros(n + 1, np.uint64)
                offsets[1:] = np.cumsum(out_len)
                data = np.frombuffer(b"".join(bytes(out[i, :out_len[i]]) for i in range(n)) + b"\0\0\0\0", np.uint8).copy()
            else:
                offsets, data = None, out
            br, bs, bv = np.zeros((n, 32), np.uint8), np.zeros((n, 32), np.uint8), np.zeros(n, np.uint8)
            assert emu.emuw_sig_decode(curve_id, form, 0, _p(data), _p(offsets), _p(br), _p(bs), _p(bv), C.c_size_t(n), _p(err)) == 0
            assert np.array_equal(br, r) and np.array_equal(bs, twin_s if flags else s)          # NORMALIZE_S = the Python twin
            if form == W.SIG_COMPACT65:
                assert np.array_equal(bv, twin_v if flags else v)
            # decoding the plain encoding with NORMALIZE_S gives the same twin
            if not flags:
                assert emu.emuw_sig_decode(curve_id, form, W.NORMALIZE_S, _p(data), _p(offsets), _p(br), _p(bs), _p(bv), C.c_size_t(n), _p(err)) == 0
                assert np.array_equal(bs, twin_s) and (form != W.SIG_COMPACT65 or np.array_equal(bv, twin_v))
    # encode(decode(b)) = b for every valid DER element of the main batch: DER is canonical
    data, offsets, real = W.der_batch(curve_id)
    wr, ws, werr = W.der_want(curve_id, 0)
    idx = np.nonzero(werr == 0)[0]
    out, out_len, err = np.zeros((len(idx), 72), np.uint8), np.zeros(len(idx), np.uint8), np.zeros(len(idx), np.uint8)
    assert len(idx) > 2 * W.N_VALID
    assert emu.emuw_sig_encode(curve_id, W.SIG_DER, 0, _p(np.ascontiguousarray(wr[idx])), _p(np.ascontiguousarray(ws[idx])), None, _p(out),
                               _p(out_len), C.c_size_t(len(idx)), _p(err)) == 0
    assert [bytes(out[k, :out_len[k]]) for k in range(len(idx))] == [real[i] for i in idx]
    assert all(not out[k, out_len[k]:].any() for k in range(len(idx)))
    # and for every valid compact element
    for form in (W.SIG_COMPACT64, W.SIG_COMPACT65):
        rows = W.compact_batch(curve_id, form)
        wr, ws, wv, werr = W.compact_want(curve_id, form, 0)
        idx = np.nonzero(werr == 0)[0]
        out, err = np.zeros((len(idx), W.SIG_STRIDE[form]), np.uint8), np.zeros(len(idx), np.uint8)
        assert len(idx) > 2 * W.N_VALID
        assert emu.emuw_sig_encode(curve_id, form, 0, _p(np.ascontiguousarray(wr[idx])), _p(np.ascontiguousarray(ws[idx])),
                                   _p(np.ascontiguousarray(wv[idx])), _p(out), None, C.c_size_t(len(idx)), _p(err)) == 0
        assert np.array_equal(out, rows[idx])


def test_the_python_der_parser_on_hand_made_cases():
    """the expectations themselves: a few encodings whose verdict is known by hand"""
    cv = W.CURVES[0]
    assert W.parse_der(cv, bytes.fromhex("3006020101020101")) == (W.OK, 1, 1)
    assert W.parse_der(cv, bytes.fromhex("3006020100020101"))[0] == W.SCALAR_RANGE
    assert W.parse_der(cv, bytes.fromhex("3006020181020101"))[0] == W.DER_INTEGER
    assert W.parse_der(cv, bytes.fromhex("300702020001020101"))[0] == W.DER_INTEGER
    assert W.parse_der(cv, bytes.fromhex("300702020080020101")) == (W.OK, 0x80, 1)
    assert W.parse_der(cv, bytes.fromhex("308106020101020101"))[0] == W.DER_SYNTAX
    assert W.parse_der(cv, bytes.fromhex("30060201010201"))[0] == W.BAD_LENGTH
    assert W.der(1, 0x80) == bytes.fromhex("300702010102020080")
    assert W.parse_der(cv, W.der(5, cv.n - 1), W.REQUIRE_LOW_S)[0] == W.HIGH_S
    assert W.parse_der(cv, W.der(5, cv.n - 1), W.NORMALIZE_S) == (W.OK, 5, 1)
    assert W.lift_x(cv, cv.g[0], cv.g[1] & 1) == cv.g[1] and W.lift_x(cv, W.non_residue_x(cv), 0) is None


# ---- 4. the sanitizer program -----------------------------------------------------------------------------------------
def test_sanitizer_program_exits_zero(emu):
    """tests/emu_wire/wire_selftest: the edge sets from heap blocks that end at the last permitted aligned word, under
    -fsanitize=address,undefined, as a process of its own"""
    res = subprocess.run([os.path.join(HERE, "wire_selftest")], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr


# ---- 5. resources and surface -----------------------------------------------------------------------------------------
def test_committed_resource_file_lists_no_private_segment_for_the_new_kernels():
    text = open(os.path.join(ROOT, "profiles", "wire_kernel_resources.txt")).read()
    rows = re.findall(r"^(k_(?:point|sig)_(?:decode|encode)<[^>]*>)\s+.*?private_segment=(\d+)\s+.*?spill_vgpr=(\d+)\s+spill_sgpr=(\d+)", text, flags=re.M)
    names = {r[0] for r in rows}
    assert len(names) == 2 + 4 + 6 + 6, sorted(names)
    assert all(int(r[1]) == 0 and int(r[2]) == 0 and int(r[3]) == 0 for r in rows), rows


def test_entry_points_exist_and_refuse_misuse_without_a_device():
    L = p2e.lib()
    buf = np.zeros(128, np.uint8)
    for name in ("p2e_point_decode_batch", "p2e_point_encode_batch", "p2e_sig_decode_batch", "p2e_sig_encode_batch"):
        assert name in p2e.EXPORTS and getattr(L, name).restype is C.c_long
    one = C.c_size_t(1)
    assert L.p2e_point_decode_batch(None, 0, _p(buf), _p(buf), _p(buf), _p(buf), one, _p(buf)) == -1
    assert L.p2e_point_encode_batch(None, 0, 0, _p(buf), _p(buf), _p(buf), one, _p(buf)) == -1
    assert L.p2e_sig_decode_batch(None, 0, 0, C.c_uint(0), _p(buf), _p(buf), _p(buf), _p(buf), None, one, _p(buf)) == -1
    assert L.p2e_sig_encode_batch(None, 0, 0, C.c_uint(0), _p(buf), _p(buf), None, _p(buf), _p(buf), one, _p(buf)) == -1
    assert (p2e.WIRE_OK, p2e.WIRE_BAD_LENGTH, p2e.WIRE_INFINITY, p2e.WIRE_HIGH_S) == (0, 1, 5, 9)
    assert (p2e.SEC1_COMPRESSED, p2e.SEC1_UNCOMPRESSED, p2e.SIG_DER, p2e.SIG_COMPACT64, p2e.SIG_COMPACT65) == (0, 1, 0, 1, 2)
    assert (p2e.SIG_REQUIRE_LOW_S, p2e.SIG_NORMALIZE_S, p2e.SIG_DER_STRIDE) == (1, 2, 72)
