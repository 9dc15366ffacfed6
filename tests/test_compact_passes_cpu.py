"""The aux, gate-internal and constraint-block passes inside the compact container, without a GPU.

1. The layout property the compact-source kernels rest on: every witness column these passes read is a narrow column,
   and every limb group (a wired operand, a generator's result limbs with its overflow word or its div limbs) sits on
   consecutive narrow rows -- for both built-in programs through the library's host-only functions and for every
   curve-program kind on both curves through the schedule builder (tests/emu_compact; a program object needs a device).
2. The compact-source kernel bodies compiled with g++ (tests/emu_compact) against the u64-source bodies (tests/emu) on the
   committed verify golden, random signatures and 20 random MSM elements; the MSM constraint-block values, which have no
   u64 emulation, against the constraint replay (oracle/check_circuit.py) on every one of the 20.
3. The seven entry points exist and refuse a NULL context and ld < n with a negative status."""
import ctypes as C
import multiprocessing as mp
import os
import subprocess

import numpy as np
import pytest

import check_circuit as K
import msm_inputs as I
import p2e_ref as R
import parity_checks as pc
import plonky2_ecdsa_amd as p2e
from backends import EmuBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "emu_compact")
NL = 9
WIDE = p2e.COMPACT_WIDE
KIND_MASK = 0xE0000000          # include/p2e.h P2E_SRC_*: a source without these bits is a witness column
ADD, SUB, ADD_MANY, MUL, INV, GLV = range(6)
CURVES = [R.SECP256K1, R.P256]
# every curve-program kind on both curves (the verifier is P-256 only)
CURVE_PROGRAMS = [(kind, curve) for curve in (0, 1) for kind in (1, 2, 3, 4, 5) if not (kind == 3 and curve == 0)]
NEW_SYMBOLS = ("p2e_ux_witness_compact_batch", "p2e_gate_internal_compact_batch", "p2e_assemble_wires_compact",
               "p2e_curve_program_aux_witness_compact_batch", "p2e_curve_program_gate_internal_compact_batch",
               "p2e_curve_program_ux_witness_compact_batch", "p2e_curve_msm_ux_witness_batch")


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _sz(v):
    return C.c_size_t(v)


class CompactEmu:
    """tests/emu_compact/libp2e_emu_compact.so"""

    def __init__(self):
        lib = os.path.join(HERE, "libp2e_emu_compact.so")
        if not os.path.exists(lib):
            subprocess.check_call(["make", "-s", "-C", HERE])
        self.L = C.CDLL(lib)
        for f in ("emuc_ux", "emuc_gate", "emuc_curve_aux", "emuc_curve_gate", "emuc_curve_ux", "emuc_gens", "emuc_layout",
                  "emuc_curve_gens", "emuc_curve_layout"):
            getattr(self.L, f).restype = C.c_long

    # -- layout ------------------------------------------------------------------------------------------
    def _gens(self, call):
        ng = call(None, None, None, None, None, None, _sz(0))
        assert ng > 0
        kinds, nops = np.zeros(ng, np.int32), np.zeros(ng, np.int32)
        first, ncols = np.zeros(ng, np.uint32), np.zeros(ng, np.uint32)
        src, nl = np.zeros((ng, 4), np.uint32), np.zeros((ng, 4), np.uint8)
        assert call(_p(kinds), _p(first), _p(ncols), _p(nops), _p(src), _p(nl), _sz(ng)) == ng
        return [(int(kinds[g]), int(first[g]), int(ncols[g]), [(int(src[g, k]), int(nl[g, k])) for k in range(nops[g])])
                for g in range(ng)]

    def _layout(self, call):
        nn, nw, ok = C.c_uint32(), C.c_uint32(), C.c_int()
        ncols = call(None, _sz(0), None, None, None)
        m = np.zeros(ncols, np.uint32)
        assert call(_p(m), _sz(ncols), C.byref(nn), C.byref(nw), C.byref(ok)) == ncols
        return m, nn.value, nw.value, ok.value

    def curve_gens(self, kind, curve, blind):
        return self._gens(lambda *a: self.L.emuc_curve_gens(kind, curve, _p(blind[0]), _p(blind[1]), *a))

    def curve_layout(self, kind, curve, blind):
        return self._layout(lambda *a: self.L.emuc_curve_layout(kind, curve, _p(blind[0]), _p(blind[1]), *a))

    def layout(self, program):
        return self._layout(lambda *a: self.L.emuc_layout(program, *a))

    def curve_ux_describe(self, kind, curve, blind):
        """[(first ux column, number of columns)] per generator: what p2e_curve_program_ux_describe reports"""
        self.L.emuc_curve_ux_describe.restype = C.c_long
        b = [_p(blind[0]), _p(blind[1])]
        ng = self.L.emuc_curve_ux_describe(kind, curve, *b, None, None, _sz(0))
        first, count = np.zeros(ng, np.uint32), np.zeros(ng, np.uint32)
        assert self.L.emuc_curve_ux_describe(kind, curve, *b, _p(first), _p(count), _sz(ng)) == ng
        return [(int(a), int(c)) for a, c in zip(first, count)]

    def curve_ux_count(self, kind, curve, blind):
        return self.L.emuc_curve_ux(kind, curve, _p(blind[0]), _p(blind[1]), *([None] * 7), None, _sz(0), None, _sz(0), None, _sz(0),
                                    None, 0, _sz(0), _sz(0), None)

    def curve_gate_count(self, kind, curve, blind):
        return self.L.emuc_curve_gate(kind, curve, _p(blind[0]), _p(blind[1]), None, _sz(0), None, _sz(0), _sz(0))

    # -- bodies ------------------------------------------------------------------------------------------
    def ux(self, program, inputs, narrow, aux32, u32):
        if program == 0:
            msg, r, s, pkx, pky = [np.ascontiguousarray(a, np.uint8) for a in inputs]
        else:
            pkx, pky, msg = [np.ascontiguousarray(a, np.uint8) for a in inputs]
            r = s = None
        n = narrow.shape[1]
        k = p2e.ux_num_cols(program)
        ux, err = np.zeros((k, n), np.uint32 if u32 else np.uint64), np.zeros(n, np.uint8)
        assert self.L.emuc_ux(program, _p(msg), _p(r), _p(s), _p(pkx), _p(pky), _p(narrow), _sz(n), _p(aux32), _sz(n), _p(ux),
                              int(u32), _sz(n), _sz(n), _p(err)) == k
        return ux, err

    def gate(self, program, aux32):
        n = aux32.shape[1]
        k = self.L.emuc_gate(program, None, _sz(0), None, _sz(0), _sz(0))
        gate = np.zeros((k, n), np.uint64)
        assert self.L.emuc_gate(program, _p(aux32), _sz(n), _p(gate), _sz(n), _sz(n)) == k
        return gate

    def curve_aux(self, kind, curve, blind, args5, narrow):
        b = [_p(blind[0]), _p(blind[1])]
        n = narrow.shape[1]
        na = self.L.emuc_curve_aux(kind, curve, *b, None, None, None, None, None, None, _sz(0), None, _sz(0), _sz(0), None)
        aux32, err = np.zeros((na, n), np.uint32), np.zeros(n, np.uint8)
        self.L.emuc_curve_aux(kind, curve, *b, *[_p(a) for a in args5], _p(narrow), _sz(n), _p(aux32), _sz(n), _sz(n), _p(err))
        return aux32, err

    def curve_gate(self, kind, curve, blind, aux32):
        b = [_p(blind[0]), _p(blind[1])]
        n = aux32.shape[1]
        ng = self.L.emuc_curve_gate(kind, curve, *b, None, _sz(0), None, _sz(0), _sz(0))
        gate = np.zeros((ng, n), np.uint64)
        self.L.emuc_curve_gate(kind, curve, *b, _p(aux32), _sz(n), _p(gate), _sz(n), _sz(n))
        return gate

    def curve_ux(self, kind, curve, blind, args5, q, n, narrow=None, cols=None, aux=None, u32=True):
        """compact source (narrow, u32 aux) or u64 source (cols, u64 aux)"""
        b = [_p(blind[0]), _p(blind[1])]
        nu = self.L.emuc_curve_ux(kind, curve, *b, *([None] * 7), None, _sz(0), None, _sz(0), None, _sz(0), None, 0, _sz(0), _sz(0), None)
        ux, err = np.zeros((nu, n), np.uint32 if u32 else np.uint64), np.zeros(n, np.uint8)
        self.L.emuc_curve_ux(kind, curve, *b, *[_p(a) for a in args5], _p(q[0]), _p(q[1]), _p(narrow), _sz(n), _p(cols), _sz(n),
                             _p(aux), _sz(n), _p(ux), int(u32), _sz(n), _sz(n), _p(err))
        return ux, err


@pytest.fixture(scope="module")
def cemu():
    return CompactEmu()


@pytest.fixture(scope="module")
def emu():
    return EmuBackend()


@pytest.fixture(scope="module")
def curve_emu():
    from test_curve_programs import Emu
    return Emu()


def _blind(curve):
    pt = CURVES[curve].mul(0xC0FFEE, CURVES[curve].g)
    return I.b32(pt[0]), I.b32(pt[1])


def to_compact(cols, col_map, nn, nw):
    """the compact form of a u64 column matrix"""
    is_wide = (col_map & WIDE) != 0
    narrow, wide = np.zeros((nn, cols.shape[1]), np.uint32), np.zeros((nw, cols.shape[1]), np.uint64)
    assert not (cols[~is_wide] >> np.uint64(32)).any()
    narrow[col_map[~is_wide]] = cols[~is_wide].astype(np.uint32)
    wide[col_map[is_wide] & 0x7FFFFFFF] = cols[is_wide]
    return narrow, wide


# ---- 1. the layout property --------------------------------------------------------------------------------------------
def _assert_layout(gens, col_map, nn, nw, what):
    """gens: [(kind, first_col, num_cols, [(src, num_limbs)])]"""
    assert nn + nw == len(col_map) == sum(g[2] for g in gens), what

    def narrow_run(col, count, why):
        rows = [int(col_map[col + k]) for k in range(count)]
        assert all(not r & WIDE for r in rows), (what, why, col)
        assert rows == list(range(rows[0], rows[0] + count)), (what, why, col)

    groups = 0
    for kind, first, _ncols, ops in gens:
        for src, nl in ops:                      # every wired operand: its source column and the limbs after it
            if src & KIND_MASK == 0 and nl:
                narrow_run(src, nl, "operand")
                groups += 1
        if kind in (ADD, SUB, ADD_MANY):
            narrow_run(first, NL + 1, "result limbs + overflow word")
        elif kind == INV:
            narrow_run(first, 2 * NL, "inverse limbs + div limbs")
        elif kind == MUL:
            narrow_run(first, NL, "product limbs")
    assert groups > 0, what


@pytest.mark.parametrize("program", [0, 1])
def test_every_column_the_passes_read_is_narrow_and_consecutive_builtin(program, cemu):
    kinds = ("add", "sub", "add_many", "mul", "inv", "glv")
    desc, wiring = p2e.schedule_describe(program), p2e.schedule_wiring(program)
    gens = [(kinds.index(d[0]), d[2], d[3], w[0]) for d, w in zip(desc, wiring)]
    col_map, nn, nw = p2e.compact_layout(program)
    _assert_layout(gens, col_map, nn, nw, program)
    # the harness sees the same layout, and the library's own check (made when a context is created) accepts it ...
    m2, nn2, nw2, ok = cemu.layout(program)
    assert np.array_equal(m2, col_map) and (nn2, nw2, ok) == (nn, nw, 1)
    # ... and refuses one in which an operand's limbs are split by a wide column, with a text that names the generator
    broken = col_map.copy()
    src = next(s for k, _f, _n, ops in gens if k in (ADD, SUB) for s, nl in ops if s & KIND_MASK == 0 and nl == NL)
    broken[src + 3] = WIDE | 0
    why = C.create_string_buffer(200)
    assert cemu.L.emuc_ux_layout_ok(program, _p(broken), _sz(len(broken)), why, _sz(200)) == 0
    assert b"not consecutive narrow columns" in why.value


@pytest.mark.parametrize("kind,curve", CURVE_PROGRAMS)
def test_every_column_the_passes_read_is_narrow_and_consecutive_curve_programs(kind, curve, cemu):
    blind = _blind(curve)
    col_map, nn, nw, ok = cemu.curve_layout(kind, curve, blind)
    _assert_layout(cemu.curve_gens(kind, curve, blind), col_map, nn, nw, (kind, curve))
    assert ok == 1


# ---- 2. the compact bodies against the u64 bodies -------------------------------------------------------------------------
def _builtin_case(emu, cemu, program, inputs, cols):
    col_map, nn, nw = p2e.compact_layout(program)
    narrow, _wide = to_compact(cols, col_map, nn, nw)
    pky = inputs[4] if program == 0 else inputs[1]
    _c, aux, aerr = emu.aux(program, inputs)
    aux32, a32err = emu.aux_compact(program, pky, narrow)
    assert not aerr.any() and not a32err.any() and np.array_equal(aux32, aux)
    assert np.array_equal(cemu.gate(program, aux32), emu.gate(program, aux))
    want, werr = emu.ux(program, inputs, cols, aux)
    for u32 in (True, False):
        got, err = cemu.ux(program, inputs, narrow, aux32, u32)
        assert np.array_equal(err, werr) and not err.any()
        assert np.array_equal(got, want), u32
    return narrow, aux32, want


def test_compact_bodies_on_the_verify_golden(emu, cemu):
    cols, inputs, _valid = pc.load_verify_golden()
    args = [np.ascontiguousarray(inputs[:, k, :]) for k in range(5)]
    _builtin_case(emu, cemu, 0, args, np.ascontiguousarray(cols))


@pytest.mark.parametrize("program", [0, 1])
def test_compact_bodies_on_random_signatures(program, emu, cemu):
    msg, r, s, pkx, pky = p2e.synth_signatures(seed=4242 + program, n=5)
    inputs = [msg, r, s, pkx, pky] if program == 0 else [pkx, pky, msg]
    cols, err, _valid = (emu.verify if program == 0 else emu.glv_mul)(*inputs)
    assert not err.any()
    narrow, aux32, want = _builtin_case(emu, cemu, program, inputs, cols)
    # a limb that is no U29 value: flagged by both sources on that signature alone
    desc, wiring = p2e.schedule_describe(program), p2e.schedule_wiring(program)
    firsts = [d[2] for d in desc if d[0] == "add"]
    col = next(f for f in firsts if any(s == f for w in wiring for s, _nl in w[0]))
    col_map, _nn, _nw = p2e.compact_layout(program)
    cols2, narrow2 = cols.copy(), narrow.copy()
    cols2[col, 3] = narrow2[col_map[col], 3] = 1 << 29
    _ux, werr = emu.ux(program, inputs, cols2, aux32.astype(np.uint64))
    _ux, err = cemu.ux(program, inputs, narrow2, aux32, True)
    assert np.array_equal(err, werr) and np.nonzero(err)[0].tolist() == [3] and err[3] == p2e.ERR_LIMB_RANGE


MSM_N = 20


def _msm_replay_ux(job):
    curve_id, col_i, vals = job
    c, _pt = K.check_msm(CURVES[curve_id], col_i, *vals)
    return np.asarray(c.ux, np.uint64)


def test_compact_bodies_of_the_msm_program(cemu, curve_emu):
    """secp256k1 MSM, 20 random elements: aux, gate-internal and ux from the compact container; this covers q"""
    curve = 0
    a = p2e.synth_signatures_curve(curve, seed=777, n=MSM_N)
    b = p2e.synth_signatures_curve(curve, seed=778, n=MSM_N)
    ins = [a[3], a[4], b[3], b[4], a[0], b[0]]                    # (px, py, qx, qy, n, m)
    blind = (I.b32(0), I.b32(0))
    curve_emu.L.emu_curve_msm.restype = C.c_long
    ncols = curve_emu.sizes(4, curve, blind)[0]
    cols, err, valid = np.zeros((ncols, MSM_N), np.uint64), np.zeros(MSM_N, np.uint8), np.zeros(MSM_N, np.uint8)
    bad = curve_emu.L.emu_curve_msm(curve, *[_p(x) for x in ins], _p(cols), _sz(MSM_N), _sz(MSM_N), _p(err), _p(valid), 32)
    assert bad == 0 and not err.any()
    args5 = (ins[4], ins[5], None, ins[0], ins[1])                # (msg = n, r = m, s, pkx, pky)
    aux, aerr = curve_emu.aux(4, curve, blind, (ins[4], ins[5], ins[4], ins[0], ins[1]), cols)
    gate = curve_emu.gate(4, curve, blind, aux)
    col_map, nn, nw, _ok = cemu.curve_layout(4, curve, blind)
    narrow, _wide = to_compact(cols, col_map, nn, nw)
    aux32, a32err = cemu.curve_aux(4, curve, blind, args5, narrow)
    assert not aerr.any() and not a32err.any() and np.array_equal(aux32, aux)
    assert np.array_equal(cemu.curve_gate(4, curve, blind, aux32), gate)
    q = (ins[2], ins[3])
    ux32, e32 = cemu.curve_ux(4, curve, blind, args5, q, MSM_N, narrow=narrow, aux=aux32, u32=True)
    ux64, e64 = cemu.curve_ux(4, curve, blind, args5, q, MSM_N, narrow=narrow, aux=aux32, u32=False)
    uxw, ew = cemu.curve_ux(4, curve, blind, args5, q, MSM_N, cols=cols, aux=aux, u32=False)   # the u64-source body with q
    assert not e32.any() and not e64.any() and not ew.any()
    assert np.array_equal(ux32, ux64) and np.array_equal(ux64, uxw)
    vals = [I.ints(x) for x in ins]
    with mp.Pool(min(MSM_N, 16)) as pool:
        want = pool.map(_msm_replay_ux, [(curve, cols[:, i].copy(), [v[i] for v in vals]) for i in range(MSM_N)])
    for i in range(MSM_N):
        assert np.array_equal(ux64[:, i], want[i]), i


@pytest.mark.parametrize("kind,curve", [(1, 1), (5, 0)])
def test_compact_bodies_of_a_windowed_and_a_fixed_base_program(kind, curve, cemu, curve_emu):
    """the other item kinds of the curve aux pass (window, fixed-base window) from the compact container"""
    n = 6
    blind = _blind(curve)
    sig = p2e.synth_signatures_curve(curve, seed=900 + kind, n=n)
    args3 = (sig[3], sig[4], sig[0])
    cols, err, _valid, bad = curve_emu.run(kind, curve, blind, args3)
    assert bad == 0 and not err.any()
    aux, _aerr = curve_emu.aux(kind, curve, blind, args3, cols)
    col_map, nn, nw, _ok = cemu.curve_layout(kind, curve, blind)
    narrow, _wide = to_compact(cols, col_map, nn, nw)
    args5 = (sig[0], None, None, sig[3], sig[4])
    aux32, a32err = cemu.curve_aux(kind, curve, blind, args5, narrow)
    assert not a32err.any() and np.array_equal(aux32, aux)
    assert np.array_equal(cemu.curve_gate(kind, curve, blind, aux32), curve_emu.gate(kind, curve, blind, aux))
    want, werr = curve_emu.ux(kind, curve, blind, args3, cols, aux)
    got, gerr = cemu.curve_ux(kind, curve, blind, args5, (None, None), n, narrow=narrow, aux=aux32, u32=True)
    assert not werr.any() and not gerr.any() and np.array_equal(got, want)


# ---- 3. surface and misuse ---------------------------------------------------------------------------------------------------
def test_the_seven_entry_points_exist_and_refuse_misuse():
    L = p2e.lib()
    for name in NEW_SYMBOLS:
        assert name in p2e.EXPORTS and hasattr(L, name), name
        getattr(L, name).restype = C.c_long
    one = np.zeros(64, np.uint64)
    b, z, x = _p(one), _sz(0), _sz(4)   # a non-null buffer, ld = 0 (< n), n = 4
    # NULL context
    calls = {
        "p2e_ux_witness_compact_batch": (None, 0, b, b, b, b, b, b, x, b, x, b, 1, x, x, b),
        "p2e_gate_internal_compact_batch": (None, 0, b, x, b, x, x),
        "p2e_assemble_wires_compact": (None, None, b, x, b, x, b, x, b, 1, x, b, x, b, x, x),
        "p2e_curve_program_aux_witness_compact_batch": (None, None, b, b, b, b, b, b, x, b, x, x, b),
        "p2e_curve_program_gate_internal_compact_batch": (None, None, b, x, b, x, x),
        "p2e_curve_program_ux_witness_compact_batch": (None, None, b, b, b, b, b, b, b, b, x, b, x, b, 1, x, x, b),
        "p2e_curve_msm_ux_witness_batch": (None, None, b, b, b, b, b, b, b, x, b, x, b, 1, x, x, b),
    }
    assert set(calls) == set(NEW_SYMBOLS)
    for name, args in calls.items():
        assert getattr(L, name)(*args) < 0, name
    # every ld_* below n, one at a time.  No context can be made without a device, so a handle that is never dereferenced
    # stands in for one: each entry point validates its pointers and strides (bad_common and the tests beside it) before
    # its first read of the context, and returns from that validation here -- the handle points at a live numpy buffer
    # all the same.  (tests/test_gpu_compact_passes.py repeats this with a real context, program and wire map.)
    fake = C.c_void_p(one.ctypes.data)
    ld_args = {    # argument positions of the strides
        "p2e_ux_witness_compact_batch": ((fake, 0, b, b, b, b, b, b, x, b, x, b, 1, x, x, b), (8, 10, 13)),
        "p2e_gate_internal_compact_batch": ((fake, 0, b, x, b, x, x), (3, 5)),
        "p2e_curve_program_aux_witness_compact_batch": ((fake, None, b, b, b, b, b, b, x, b, x, x, b), (8, 10)),
        "p2e_curve_program_gate_internal_compact_batch": ((fake, None, b, x, b, x, x), (3, 5)),
        "p2e_curve_program_ux_witness_compact_batch": ((fake, None, b, b, b, b, b, b, b, b, x, b, x, b, 1, x, x, b), (10, 12, 15)),
        "p2e_curve_msm_ux_witness_batch": ((fake, None, b, b, b, b, b, b, b, x, b, x, b, 1, x, x, b), (9, 11, 14)),
        # (without a wire map the call is refused whatever the strides are: the map decides which matrices are read)
        "p2e_assemble_wires_compact": ((fake, None, b, x, b, x, b, x, b, 1, x, b, x, b, x, x), (3, 5, 7, 10, 12, 14)),
    }
    assert set(ld_args) == set(NEW_SYMBOLS)
    for name, (args, positions) in ld_args.items():
        for pos in positions:
            assert args[pos] is x
            short = args[:pos] + (z,) + args[pos + 1:]
            assert getattr(L, name)(*short) < 0, (name, pos)
            assert L.p2e_last_error(), (name, pos)
        if name != "p2e_assemble_wires_compact":
            first = positions[0]
            assert getattr(L, name)(*(args[:first] + (z,) + args[first + 1:])) < 0
            assert b"ld < n" in L.p2e_last_error(), name
