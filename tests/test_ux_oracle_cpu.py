"""The constraint-block (ux) and gate-internal passes against the C oracle on every element and every value, without a GPU.

1. The oracle is pinned first: its ux and gate matrices and its per-generator block list against the Python constraint
   replay (oracle/check_circuit.py: Circuit.ux, .gate, .ux_ops) for both built-in programs and the nine (kind, curve) curve
   programs -- 16 random elements each, every named row of the adversarial batches, and the golden rows behind
   tests/golden/ux_digest.json.  The replay runs on the oracle's own cols and aux.
2. The library's block lists (p2e_ux_describe, the schedule builder of every curve program) equal the oracle's, and so do
   the four column counts.
3. The kernel bodies compiled for the CPU (tests/emu: csrc/ux.hpp, csrc/aux.hpp; tests/emu_compact: the compact-source
   bodies and item tables) against the oracle: the WHOLE adversarial batch of both built-in programs and 64 random elements
   of every curve program, from the u64 matrices and from the compact container, u32 and u64 outputs.  Values on every row
   the fill does not flag; the pass's own err byte on every row.
test_gpu_parity.py, test_gpu_compact_passes.py and test_gpu_adversarial.py make the same comparison on the HIP kernels."""
import hashlib
import json
import multiprocessing as mp
import os

import numpy as np
import pytest

import adversarial_inputs as A
import check_circuit as K
import msm_inputs as I
import oracle_c
import p2e_ref as R
import parity_checks as pc
import plonky2_ecdsa_amd as p2e
import ux_oracle as UX
from test_compact_passes_cpu import CompactEmu, to_compact

CURVES = [R.SECP256K1, R.P256]
CURVE_PROGRAMS = [(kind, curve) for curve in (0, 1) for kind in (1, 2, 3, 4, 5) if not (kind == 3 and curve == 0)]
ALL_PROGRAMS = [("builtin", 0, 0), ("builtin", 1, 0)] + [("curve", k, c) for k, c in CURVE_PROGRAMS]
IDS = ["verify", "glv_mul"] + [f"{('windowed', 'bitwise', 'verify', 'msm', 'fixed_base')[k - 1]}-{('secp256k1', 'p256')[c]}" for k, c in CURVE_PROGRAMS]
ADVERSARIAL = {("builtin", 0, 0): "verify", ("builtin", 1, 0): "glv_mul", ("curve", 1, 0): "windowed", ("curve", 1, 1): "windowed",
               ("curve", 2, 0): "bitwise", ("curve", 2, 1): "bitwise", ("curve", 3, 1): "verify"}
# the two named rows whose witness the reference's own constraints reject (tests/adversarial_inputs.py, CAVEAT): the replay
# stops at the violated connect, and the values it derived up to there are compared
REJECTED = {"pk_x_plus_p": "sub_nonnative", "s_plus_n": "inv_nonnative"}
RANDOM_N = 16
EMU_CURVE_N = 64
CHUNK = 160                       # rows of an adversarial batch per emulator call: 0.3 GB per u64 ux matrix


def _point(fam, kind, curve):
    """the blinding point of kinds 1-3 (the one the adversarial batches use), the base of kind 5, as integers"""
    if fam == "builtin" or kind == 4:
        return None
    return A.blind(curve) if kind != 5 else CURVES[curve].mul(0xBA5E, CURVES[curve].g)


def _random_inputs(fam, kind, curve, n, seed):
    """the input arrays of n random valid elements, in the order of the program's fill"""
    if fam == "builtin":
        sig = p2e.synth_signatures(seed=seed, n=n)
        if kind == 0:
            return list(sig)
        rng = R.SplitMix64(seed + 1)
        return [sig[3], sig[4], oracle_c.pack256([rng.below(R.N) for _ in range(n)])]
    a = p2e.synth_signatures_curve(curve, seed=seed, n=n)
    if kind == 3:
        return list(a)
    if kind == 4:
        b = p2e.synth_signatures_curve(curve, seed=seed + 1, n=n)
        return [a[3], a[4], b[3], b[4], a[0], b[0]]
    return [a[3], a[4], a[0]]


def _walk(fam, kind, curve, arrs):
    if fam == "builtin":
        return UX.builtin(kind, arrs)
    return UX.curve_program(kind, curve, _point(fam, kind, curve), arrs)


# ---- 1. the oracle against the Python replay -------------------------------------------------------------------------------
def _replay(job):
    """one element through the constraint replay: (ux, gate, blocks, is-glv per generator, the violated constraint or None)"""
    fam, kind, curve, point, vals, cols, aux = job
    t = K.input_t
    c = K.Circuit(cols, aux=aux, curve=None if fam == "builtin" else CURVES[curve])
    violated = None
    try:
        if fam == "builtin" and kind == 0:
            msg, r, s, px, py = vals
            c.verify_secp256k1_message(t("msg", msg), t("r", r), t("s", s), (t("pkx", px), t("pky", py)))
        elif fam == "builtin":
            px, py, k = vals
            c.glv_mul((t("pkx", px), t("pky", py)), t("k", k))
        elif kind == 1:
            px, py, k = vals
            c.curve_scalar_mul_windowed((t("px", px), t("py", py)), t("k", k), point, True)
        elif kind == 2:
            px, py, k = vals
            c.curve_scalar_mul((t("px", px), t("py", py)), t("k", k), point, True)
        elif kind == 3:
            msg, r, s, px, py = vals
            c.verify_p256_message(t("msg", msg), t("r", r), t("s", s), (t("pkx", px), t("pky", py)), point)
        elif kind == 4:
            px, py, qx, qy, n, m = vals
            c.curve_msm((t("px", px), t("py", py)), (t("qx", qx), t("qy", qy)), t("n", n), t("m", m))
        else:
            c.fixed_base_curve_mul(point, t("k", vals[2]))
        c.finish()
    except K.ConstraintViolation as e:
        violated = str(e)
    return (np.asarray(c.ux, np.uint64), np.asarray(c.gate, np.uint64), [(a, b) for a, b, _l in c.ux_ops],
            [g[0] == "glv" for g in c.gens], violated)


@pytest.fixture(scope="module")
def pool():
    with mp.Pool(min(16, os.cpu_count() or 1)) as p:
        yield p


def _assert_oracle_is_the_replay(pool, fam, kind, curve, arrs, names):
    """names[i]: what element i is (for the message; a REJECTED name allows the replay to stop early)"""
    exp = _walk(fam, kind, curve, arrs)
    lay = UX.layout(fam, kind, curve)
    assert exp["ux"].shape[0] == lay["num_ux"] and exp["gate"].shape[0] == lay["num_gate"]
    n = len(names)
    assert not exp["err"].any(), [names[i] for i in np.nonzero(exp["err"])[0]]
    ints = [I.ints(a) for a in arrs]
    jobs = [(fam, kind, curve, _point(fam, kind, curve), [v[i] for v in ints], exp["cols"][:, i].copy(), exp["aux"][:, i].copy())
            for i in range(n)]
    full = 0
    for i, (ux, gate, blocks, glv, violated) in enumerate(pool.map(_replay, jobs)):
        what = (fam, kind, curve, names[i])
        if violated is not None:
            assert names[i] in REJECTED and REJECTED[names[i]] in violated, (what, violated)
            assert len(ux) > 0 and np.array_equal(exp["ux"][:len(ux), i], ux), what
            assert np.array_equal(exp["gate"][:len(gate), i], gate), what
            continue
        assert names[i] not in REJECTED, what
        UX.assert_same_numpy(f"{what}: ux", exp["ux"][:, i:i + 1], ux[:, None], blocks=lay["blocks"])
        UX.assert_same_numpy(f"{what}: gate", exp["gate"][:, i:i + 1], gate[:, None])
        assert len(glv) == len(lay["blocks"]), what
        assert [b for b, g in zip(lay["blocks"], glv) if not g] == blocks, what
        assert all(b[1] == 0 for b, g in zip(lay["blocks"], glv) if g), what
        full += 1
    return full


@pytest.mark.parametrize("fam,kind,curve", ALL_PROGRAMS, ids=IDS)
def test_oracle_ux_and_gate_equal_the_replay_on_random_elements(fam, kind, curve, pool):
    arrs = _random_inputs(fam, kind, curve, RANDOM_N, 5150 + 10 * curve + kind)
    assert _assert_oracle_is_the_replay(pool, fam, kind, curve, arrs, [f"random {i}" for i in range(RANDOM_N)]) == RANDOM_N


@pytest.mark.parametrize("fam,kind,curve", list(ADVERSARIAL), ids=[IDS[ALL_PROGRAMS.index(k)] for k in ADVERSARIAL])
def test_oracle_ux_and_gate_equal_the_replay_on_every_named_row(fam, kind, curve, pool):
    program = ADVERSARIAL[fam, kind, curve]
    rows, _marks = A.batch(program, curve)
    named = A.named_rows(program, curve)
    assert len(named) >= 5
    names = sorted(named)
    arrs = A.arrays([rows[named[k]] for k in names])
    full = _assert_oracle_is_the_replay(pool, fam, kind, curve, arrs, names)
    assert full == len(names) - sum(k in REJECTED for k in names)


@pytest.mark.parametrize("program", [0, 1])
def test_oracle_ux_hashes_to_the_golden_digests(program):
    dig = json.load(open(os.path.join(pc.GOLD, "ux_digest.json")))["verify" if program == 0 else "glv_mul"]
    if program == 0:
        _cols, inputs, _valid = pc.load_verify_golden()
    else:
        inputs = np.load(os.path.join(pc.GOLD, "glv_mul_golden.npz"))["inputs"]
    exp = UX.builtin(program, [np.ascontiguousarray(inputs[:, k, :]) for k in range(inputs.shape[1])])
    assert len(dig) == exp["ux"].shape[1] and not exp["err"].any()
    hashed = 0
    for i, d in enumerate(dig):
        if d is None:                                # the golden that does not verify has no replayed vector
            continue
        v = exp["ux"][:, i]
        assert len(v) == d["len"] and [int(x) for x in v[:8]] == d["head"]
        assert hashlib.sha256(v.astype("<u4").tobytes()).hexdigest() == d["sha256"], i
        hashed += 1
    assert hashed >= 2


# ---- 2. block lists and column counts -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cemu():
    return CompactEmu()


@pytest.fixture(scope="module")
def curve_emu():
    from test_curve_programs import Emu
    return Emu()


@pytest.fixture(scope="module")
def emu():
    from backends import EmuBackend
    return EmuBackend()


def _blind_bytes(fam, kind, curve):
    pt = _point(fam, kind, curve) or (0, 0)
    return I.b32(pt[0]), I.b32(pt[1])


def test_block_lists_and_column_counts_of_the_builtin_programs():
    for program, counts in ((0, (p2e.VERIFY_COLS, p2e.VERIFY_AUX_COLS, p2e.VERIFY_UX_COLS, p2e.VERIFY_GATE_COLS)),
                            (1, (oracle_c.GLV_MUL_COLS, p2e.GLV_MUL_AUX_COLS, p2e.GLV_MUL_UX_COLS, p2e.GLV_MUL_GATE_COLS))):
        lay = UX.layout("builtin", program)
        assert (lay["num_cols"], lay["num_aux"], lay["num_ux"], lay["num_gate"]) == counts
        assert p2e.ux_num_cols(program) == lay["num_ux"] and p2e.aux_num_cols(program) == lay["num_aux"]
        assert [tuple(b) for b in p2e.ux_describe(program)] == lay["blocks"]
        assert len(lay["blocks"]) == len(p2e.schedule_describe(program))


@pytest.mark.parametrize("kind,curve", CURVE_PROGRAMS, ids=IDS[2:])
def test_block_lists_and_column_counts_of_the_curve_programs(kind, curve, cemu, curve_emu):
    """p2e_curve_program_ux_describe needs a device; its list comes from host::ux_blocks over the program's schedule, which
    the emulator exposes (emuc_curve_ux_describe) -- test_gpu_compact_passes.py compares the entry point itself"""
    lay = UX.layout("curve", kind, curve)
    blind = _blind_bytes("curve", kind, curve)
    nc, ng, na = curve_emu.sizes(kind, curve, blind)
    assert (nc, na) == (lay["num_cols"], lay["num_aux"]) and ng == len(lay["blocks"])
    assert cemu.curve_ux_count(kind, curve, blind) == lay["num_ux"]
    assert cemu.curve_gate_count(kind, curve, blind) == lay["num_gate"]
    assert cemu.curve_ux_describe(kind, curve, blind) == lay["blocks"]


# ---- 3. the kernel bodies against the oracle --------------------------------------------------------------------------------
def _assert_bodies(what, exp, lay, runs):
    """runs: [(name, ux, err)] and [(name, gate)] of the bodies on the oracle's matrices"""
    clean = exp["err"] == 0
    for name, ux, err in runs["ux"]:
        assert not err.any(), f"{what}, {name}: the pass flags rows {np.nonzero(err)[0][:8].tolist()} whose operands are all U29 values"
        UX.assert_same_numpy(f"{what}, {name}", ux.astype(np.uint64), exp["ux"], clean, lay["blocks"])
    for name, gate in runs["gate"]:
        UX.assert_same_numpy(f"{what}, {name}", gate, exp["gate"], clean)


@pytest.mark.parametrize("program", [0, 1], ids=["verify", "glv_mul"])
def test_builtin_bodies_equal_the_oracle_on_the_whole_adversarial_batch(program, emu, cemu):
    rows, _marks = A.batch("verify" if program == 0 else "glv_mul", 0)
    arrs = A.arrays(rows)
    lay = UX.layout("builtin", program)
    col_map, nn, nw = p2e.compact_layout(program)
    flagged = 0
    for first in range(0, len(rows), CHUNK):
        part = [np.ascontiguousarray(a[first:first + CHUNK]) for a in arrs]
        exp = UX.builtin(program, part)
        flagged += int((exp["err"] != 0).sum())
        narrow, _wide = to_compact(exp["cols"], col_map, nn, nw)
        aux32 = exp["aux"].astype(np.uint32)
        assert np.array_equal(aux32.astype(np.uint64), exp["aux"])
        runs = {"ux": [("u64 source", *emu.ux(program, part, exp["cols"], exp["aux"])),
                       ("compact source, u32", *cemu.ux(program, part, narrow, aux32, True)),
                       ("compact source, u64", *cemu.ux(program, part, narrow, aux32, False))],
                "gate": [("u64 aux", emu.gate(program, exp["aux"])), ("u32 aux", cemu.gate(program, aux32))]}
        _assert_bodies(f"program {program}, rows {first}..", exp, lay, runs)
    assert flagged == A.COUNTS["verify" if program == 0 else "glv_mul", 0][2]


def test_range_check_of_a_value_equal_to_the_modulus(emu, cemu):
    """list_le on equal limbs.  No walk reaches it: a range-checked value equals its modulus only as a sum a + b = m of two
    canonical values (add keeps the sum when it is not GREATER than m), and the three range-checked adds of these programs
    cannot give it on a row that is not flagged -- x^3 + a x + b = 0 would be a point of order two on a curve of prime
    order, k1 + lambda k2 = n is k = 0, and a conditional negation adds zero to a canonical value.  So the case is given to
    the bodies directly: the result limbs of two range-checked multiplications of the verify golden (y^2 over the base
    field, u1 over the scalar field) are overwritten with m - 1, m and m + 1.  Expected from the model stated in
    oracle/check_circuit.py, list_le(a, b) = [a <= b]: 1, 1, 0; every other value stays what the oracle's walk gives."""
    cols, inputs, _valid = pc.load_verify_golden()
    args = [np.ascontiguousarray(np.repeat(inputs[:1, k, :], 3, axis=0)) for k in range(5)]
    exp = UX.builtin(0, args)
    desc, blocks = p2e.schedule_describe(0), p2e.ux_describe(0)
    picks = [next(g for g, d in enumerate(desc) if d[0] == "mul" and d[1] == f and blocks[g][1] == 1) for f in (0, 1)]
    cols3, want = exp["cols"].copy(), exp["ux"].copy()
    for g, m in zip(picks, (R.P, R.N)):
        assert not any(desc[g][2] in [s for s, _nl in w[0]] for w in p2e.schedule_wiring(0)), "the limbs must be nobody's operand"
        for i, v in enumerate((m - 1, m, m + 1)):
            cols3[desc[g][2]:desc[g][2] + 9, i] = R.limbs_of(v, 9)
            want[blocks[g][0], i] = int(v <= m)
    assert want[blocks[picks[0]][0]].tolist() == [1, 1, 0]
    col_map, nn, nw = p2e.compact_layout(0)
    narrow, _wide = to_compact(cols3, col_map, nn, nw)
    aux32 = exp["aux"].astype(np.uint32)
    for name, (ux, err) in (("u64 source", emu.ux(0, args, cols3, exp["aux"])), ("compact source", cemu.ux(0, args, narrow, aux32, True))):
        assert not err.any(), name
        UX.assert_same_numpy(name, ux.astype(np.uint64), want, blocks=[tuple(b) for b in blocks])


@pytest.mark.parametrize("kind,curve", CURVE_PROGRAMS, ids=IDS[2:])
def test_curve_program_bodies_equal_the_oracle_on_random_elements(kind, curve, cemu, curve_emu):
    n = EMU_CURVE_N
    host = _random_inputs("curve", kind, curve, n, 6260 + 10 * curve + kind)
    exp = UX.curve_program(kind, curve, _point("curve", kind, curve), host)
    assert not exp["err"].any()
    lay = UX.layout("curve", kind, curve)
    blind = _blind_bytes("curve", kind, curve)
    col_map, nn, nw, ok = cemu.curve_layout(kind, curve, blind)
    assert ok == 1
    narrow, _wide = to_compact(exp["cols"], col_map, nn, nw)
    aux32 = exp["aux"].astype(np.uint32)
    if kind == 3:
        args5, q = tuple(host), (None, None)
    elif kind == 4:
        args5, q = (host[4], host[5], None, host[0], host[1]), (host[2], host[3])
    else:
        args5, q = (host[2], None, None, host[0], host[1]), (None, None)
    runs = {"ux": [("u64 source", *cemu.curve_ux(kind, curve, blind, args5, q, n, cols=exp["cols"], aux=exp["aux"], u32=False)),
                   ("compact source, u32", *cemu.curve_ux(kind, curve, blind, args5, q, n, narrow=narrow, aux=aux32, u32=True)),
                   ("compact source, u64", *cemu.curve_ux(kind, curve, blind, args5, q, n, narrow=narrow, aux=aux32, u32=False))],
            "gate": []}
    if kind != 4:                                    # the u64-source entry point of tests/emu (no slot for q)
        runs["ux"].append(("u64 source, tests/emu", *curve_emu.ux(kind, curve, blind, host if kind == 3 else tuple(host), exp["cols"], exp["aux"])))
    if lay["num_gate"]:
        runs["gate"] = [("u64 aux", curve_emu.gate(kind, curve, blind, exp["aux"])), ("u32 aux", cemu.curve_gate(kind, curve, blind, aux32))]
    else:
        assert curve_emu.gate(kind, curve, blind, exp["aux"]).shape[0] == 0
    _assert_bodies(f"kind {kind}, curve {curve}", exp, lay, runs)
