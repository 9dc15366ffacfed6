"""The knob table of csrc/knobs.hpp without a GPU: read_tuning driven through tests/emu (emu_tuning) by (name, value) pairs in
place of the environment.  Every expected value is written out here, taken from what p2e_ctx_create did when each knob had a
getenv block of its own: the defaults, both ends of every accepted range (and one step outside each, which leaves the
default: out of range is ignored, never clamped), P2E_QUAD_MAX_N setting both thresholds, the P2E_SMALL_TAKES list."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "emu")

# emu_tuning's order
FIELDS = ("run_iters", "run_iters_mid", "run_iters_small", "fb_run", "runs_min_n", "quad_max_n", "cp_quad_max_n", "binv_alt_max_n",
          "cp_runs_min_n", "msm_pieces", "msm_pieces_mid", "msm_pieces_small", "fixed_pieces", "fixed_pieces_small",
          "binv_mid_split_log2", "binv_split_log2", "binv_split_log2_last", "binv_split_log2_fixed", "quad_b_first_on_fixed",
          "quad_few_waits", "expand_lds_small", "expand_lds")
DEFAULTS = dict(run_iters=9, run_iters_mid=12, run_iters_small=4, fb_run=0, runs_min_n=21505, quad_max_n=21504, cp_quad_max_n=17408,
                binv_alt_max_n=49152, cp_runs_min_n=49152, msm_pieces=8, msm_pieces_mid=5, msm_pieces_small=5, fixed_pieces=2,
                fixed_pieces_small=1, binv_mid_split_log2=1, binv_split_log2=2, binv_split_log2_last=3, binv_split_log2_fixed=3,
                quad_b_first_on_fixed=1, quad_few_waits=1, expand_lds_small=54000, expand_lds=0)
MAX_PIECES = 16
# variable, field, lowest and highest accepted value
RANGED = [("P2E_RUN_ITERS", "run_iters", 0, 73), ("P2E_RUN_ITERS_MID", "run_iters_mid", 0, 73),
          ("P2E_RUN_ITERS_SMALL", "run_iters_small", 0, 73),
          ("P2E_MSM_PIECES", "msm_pieces", 1, 16), ("P2E_MSM_PIECES_MID", "msm_pieces_mid", 1, 16),
          ("P2E_MSM_PIECES_SMALL", "msm_pieces_small", 1, 16), ("P2E_FIXED_PIECES", "fixed_pieces", 1, 16),
          ("P2E_FIXED_PIECES_SMALL", "fixed_pieces_small", 1, 16),
          ("P2E_BINV_MID_SPLIT_LOG2", "binv_mid_split_log2", 0, 3), ("P2E_BINV_SPLIT_LOG2", "binv_split_log2", 0, 4),
          ("P2E_BINV_SPLIT_LOG2_LAST", "binv_split_log2_last", 0, 4), ("P2E_BINV_SPLIT_LOG2_FIXED", "binv_split_log2_fixed", 0, 4)]
# variable, field(s), a value, what the field(s) then hold
UNCHECKED = [("P2E_FB_RUN", ("fb_run",), "1", 1), ("P2E_FB_RUN", ("fb_run",), "0", 0),
             ("P2E_QUAD_B_FIRST_ON_FIXED", ("quad_b_first_on_fixed",), "0", 0), ("P2E_QUAD_B_FIRST_ON_FIXED", ("quad_b_first_on_fixed",), "7", 1),
             ("P2E_QUAD_FEW_WAITS", ("quad_few_waits",), "0", 0),
             ("P2E_RUNS_MIN_N", ("runs_min_n",), "1", 1), ("P2E_RUNS_MIN_N", ("runs_min_n",), "5000000000", 5000000000),
             ("P2E_QUAD_MAX_N", ("quad_max_n", "cp_quad_max_n"), "0", 0), ("P2E_QUAD_MAX_N", ("quad_max_n", "cp_quad_max_n"), "30000", 30000),
             ("P2E_BINV_ALT_MAX_N", ("binv_alt_max_n",), "0", 0), ("P2E_CP_RUNS_MIN_N", ("cp_runs_min_n",), "8192", 8192),
             ("P2E_EXPAND_LDS_SMALL", ("expand_lds_small",), "160000", 160000), ("P2E_EXPAND_LDS", ("expand_lds",), "54000", 54000)]


@pytest.fixture(scope="module")
def tuning():
    subprocess.check_call(["make", "-s", "-C", HERE])   # (a harness built before the export existed is rebuilt)
    L = C.CDLL(os.path.join(HERE, "libp2e_emu.so"))
    L.emu_tuning.restype = C.c_long

    def read(**env):
        names = (C.c_char_p * len(env))(*[k.encode() for k in env])
        values = (C.c_char_p * len(env))(*[str(v).encode() for v in env.values()])
        out = (C.c_longlong * (len(FIELDS) + MAX_PIECES + 1))()
        assert L.emu_tuning(names, values, C.c_size_t(len(env)), out) == len(out)
        got = dict(zip(FIELDS, out[:len(FIELDS)]))
        got["small_takes"] = list(out[len(FIELDS):])
        return got

    return read


def _expect(**changed):
    return {**DEFAULTS, "small_takes": [0] * (MAX_PIECES + 1), **changed}


def test_defaults_hold_with_nothing_set(tuning):
    assert tuning() == _expect()
    assert tuning(P2E_NO_SUCH_KNOB=3, P2E_NARROW_STORES=1, P2E_CP_NO_RUNS=1) == _expect()   # (per-call switches are not in the table)


@pytest.mark.parametrize("name,field,lo,hi", RANGED)
def test_ranged_knob_takes_both_ends_and_ignores_one_step_outside(tuning, name, field, lo, hi):
    assert tuning(**{name: lo}) == _expect(**{field: lo})
    assert tuning(**{name: hi}) == _expect(**{field: hi})
    assert tuning(**{name: lo - 1}) == _expect()
    assert tuning(**{name: hi + 1}) == _expect()


@pytest.mark.parametrize("name,fields,value,want", UNCHECKED)
def test_flag_and_size_knobs(tuning, name, fields, value, want):
    assert tuning(**{name: value}) == _expect(**{f: want for f in fields})


def test_quad_max_n_zero_zeroes_both_thresholds(tuning):
    got = tuning(P2E_QUAD_MAX_N=0)
    assert (got["quad_max_n"], got["cp_quad_max_n"]) == (0, 0)


def test_small_takes_list(tuning):
    assert tuning(P2E_SMALL_TAKES="6,5,5,2")["small_takes"] == [6, 5, 5, 2] + [0] * 13
    twenty = ",".join(str(k) for k in range(1, 21))
    assert tuning(P2E_SMALL_TAKES=twenty)["small_takes"] == list(range(1, 17)) + [0]
    assert tuning(P2E_SMALL_TAKES="6,5,5,2") == _expect(small_takes=[6, 5, 5, 2] + [0] * 13)


def test_every_knob_at_once(tuning):
    """the rows do not interfere with each other"""
    env = {name: hi for name, _f, _lo, hi in RANGED}
    env.update(P2E_FB_RUN=1, P2E_QUAD_MAX_N=0, P2E_EXPAND_LDS=1000, P2E_SMALL_TAKES="3,2")
    want = {field: hi for _n, field, _lo, hi in RANGED}
    want.update(fb_run=1, quad_max_n=0, cp_quad_max_n=0, expand_lds=1000, small_takes=[3, 2] + [0] * 15)
    assert tuning(**env) == _expect(**want)


# ---- the launch plans choose + build make of the knobs (csrc/launch_plan.hpp) ---------------------------------------------
import plan_cases

CASES = plan_cases.cases()
PIECE_OPS = [dict(id=f"curve:{program}:piece_ops_{v}", family=1, prog=kind, curve=curve, env={"P2E_CP_PIECE_OPS_QUAD": str(v)}, n=plan_cases.N,
                  timing=False) for program, (kind, curve) in plan_cases.CURVE_PROGRAMS.items() for v in (8, 20, 45)]
TOO_MANY_PIECES = -1   # -(plan::TOO_MANY_PIECES)


@pytest.fixture(scope="module")
def plans():
    subprocess.check_call(["make", "-s", "-C", HERE])
    return plan_cases.Plans()


@pytest.fixture(scope="module")
def golden():
    return plan_cases.golden()


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_plan_is_the_sequence_the_library_issued_before_plans_were_data(plans, golden, case):
    """tests/golden/launch_plans.txt.gz: every kernel launch, event record and stream wait of one call per case, recorded on a GPU
    from the library as it was when run_program / run_curve_program issued them from control flow.  choose + build, dumped in
    the same text form, is that sequence line for line."""
    lines, _shape = plans.of(case)
    assert lines == golden[case["id"]]


def test_the_fixture_holds_exactly_the_case_table(golden):
    assert sorted(golden) == sorted(c["id"] for c in CASES)


def _fields(line):
    kind, *kv = line.split()
    return kind, dict(x.split("=") for x in kv)


def _check_sound(lines, shape):
    """every WAIT names an event an earlier step of the list records; the CHAIN steps, the BINV steps and the expansion steps
    each cover the ops of the program exactly once; no piece or expansion index beyond what the context has events for"""
    num_ops, fb_begin, fb_windows, loop_begin, loop_iters, stride, max_seg, max_expand = shape
    recorded = set()
    cover = {k: [0] * num_ops for k in ("CHAIN", "BINV", "EXPAND")}

    def mark(what, lo, hi):
        assert 0 <= lo < hi <= num_ops, (what, lo, hi)
        for t in range(lo, hi):
            cover[what][t] += 1

    kind, end = _fields(lines[-1])
    assert kind == "END" and 0 < int(end["n_seg"]) <= max_seg
    for line in lines[:-1]:
        kind, f = _fields(line)
        if kind in ("RECORD", "WAIT"):
            name, _, idx = f["ev"].partition("[")
            if idx:
                assert int(idx[:-1]) < (max_seg if name in ("piece", "binv") else max_expand), line
            if kind == "RECORD":
                recorded.add(f["ev"])
            else:
                assert f["ev"] in recorded, line + ": nothing before it records that event"
        elif kind == "CHAIN":
            lo = int(f["lo"])
            mark("CHAIN", lo, lo + int(f["rows"]) * int(f["count"]) if f["form"] == "rows" else int(f["hi"]))
        elif kind == "BINV":
            mark("BINV", int(f["lo"]), int(f["hi"]))
        elif kind == "EXPAND_OPS":
            mark("EXPAND", int(f["s_lo"]), int(f["s_hi"]))
        elif kind == "EXPAND_RUNS":
            assert int(f["run_iters"]) > 0 and 0 <= int(f["it0"]) < int(f["it1"]) <= loop_iters
            mark("EXPAND", loop_begin + stride * int(f["it0"]), loop_begin + stride * int(f["it1"]))
        elif kind == "EXPAND_FB_RUN":
            assert int(f["t_after"]) == fb_begin + fb_windows
            mark("EXPAND", fb_begin, fb_begin + fb_windows)
        else:
            assert kind in ("SCALAR", "FINALIZE"), line
    for what, c in cover.items():
        assert c == [1] * num_ops, (what, [t for t in range(num_ops) if c[t] != 1][:8])


@pytest.mark.parametrize("case", CASES + PIECE_OPS, ids=[c["id"] for c in CASES + PIECE_OPS])
def test_plan_is_sound(plans, case):
    """(a wait on an event this call has not recorded is no error to HIP: it counts as satisfied -- a silent race; a piece
    beyond the capacity was once dropped silently.)  Where the pieces would not fit, build must refuse: pieces of p ops make at
    least ceil(ops / p) of them and, with the table and the tail cut separately, at most four more."""
    lines, shape = plans.of(case)
    num_ops, max_seg = shape[0], shape[6]
    piece_ops = int(case["env"].get("P2E_CP_PIECE_OPS_QUAD", 0))
    least = -(-num_ops // piece_ops) if piece_ops else 0
    if least > max_seg:
        assert lines == TOO_MANY_PIECES
        return
    if isinstance(lines, int):
        assert lines == TOO_MANY_PIECES and least + 4 > max_seg
        return
    _check_sound(lines, shape)


def test_the_p256_verifier_in_pieces_of_8_ops_is_refused(plans):
    """429 ops in pieces of 8 are more than the 34 pieces a context has events for: the call fails (P2E_E_INVALID)"""
    lines, shape = plans.dump(1, 3, 1, {"P2E_CP_PIECE_OPS_QUAD": "8"}, plan_cases.N)
    assert shape[0] == 429 and shape[6] == 34 and lines == TOO_MANY_PIECES
