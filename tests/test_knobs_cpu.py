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
