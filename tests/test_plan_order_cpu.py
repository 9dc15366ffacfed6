"""Launch plans (csrc/launch_plan.hpp) checked for races without a GPU.

A plan orders its steps only through stream order and RECORD / WAIT pairs.  tests/emu executes the compute steps in list
order, so a missing wait cannot change its output, and a device run repeats calls on a scratch that still holds the previous
call's (correct) values.  This module asks the question directly, three ways:

  static     the happens-before relation of a plan, built from its text form, must contain every ordering that the DATA
             requires.  Who reads what is derived from the exported op table (emu_case_ops) by the rules of the table in
             DESIGN.md section 5 (What a plan must order), never from the planner's own piece list.
  blocks     the column blocks of p2e_segments_describe (plan::column_blocks, emu_case_blocks) are disjoint, cover every
             column once, and every step that writes a column of a block happens before the RECORD of the block's event.
  adversarial  the emulator runs the real bodies on a poisoned scratch in the orders E(X) = (the ancestors of X, X, everything
             else), one per compute step X: X as early as the waits permit.  Every E(X) must reproduce the list-order run byte
             for byte, and the list-order run is compared with the C oracle.

Mutations (one WAIT deleted) show that both checks notice a missing wait.  Mutated plans exist in the emulator only."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import plan_cases
from test_knobs_cpu import PIECE_OPS, TOO_MANY_PIECES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "emu")
sys.path.insert(0, os.path.join(ROOT, "oracle"))

CASES = plan_cases.cases()
CASES += [c for c in PIECE_OPS if c["id"] not in {x["id"] for x in CASES}]   # (piece_ops_20 is in both lists)
BY_ID = {c["id"]: c for c in CASES}
COMPUTE = ("SCALAR", "CHAIN", "BINV", "EXPAND_OPS", "EXPAND_RUNS", "EXPAND_FB_RUN")
EXPAND = ("EXPAND_OPS", "EXPAND_RUNS", "EXPAND_FB_RUN")
OP_ADD, OP_DBL, OP_CADD = 0, 1, 2
R_SLOT, R_CONST, R_DYN, R_FBTAB, R_MSMTAB, R_SELSLOT = range(6)
F_NO_AFFINE = 8
SHAPE = ("num_ops", "num_slots", "slot_p", "slot_sp", "num_cols", "num_chains", "cb0", "cb1", "cb2", "cb3", "ce0", "ce1", "ce2", "ce3",
         "loop_begin", "loop_iters", "stride", "fb_begin", "fb_windows", "cp_table_ops")


# ---- tests/emu: one case held open ----------------------------------------------------------------------------------------
class Case:
    """choose + build for a case of plan_cases (drop: the plan without step `drop`), through emu_case_open"""

    def __init__(self, plans, case, drop=-1):
        self.L, self.case = plans.L, case
        env = case["env"]
        names = (C.c_char_p * len(env))(*[k.encode() for k in env])
        values = (C.c_char_p * len(env))(*[str(v).encode() for v in env.values()])
        bx, by = plans.blind(case["curve"])
        if case.get("blind") is not None:
            bx, by = case["blind"]
        rc = C.c_long()
        self.L.emu_case_open.restype = C.c_void_p
        self.h = self.L.emu_case_open(C.c_int(case["family"]), C.c_int(case["prog"]), C.c_int(case["curve"]), bx.ctypes.data_as(C.c_void_p),
                                      by.ctypes.data_as(C.c_void_p), C.c_size_t(case["n"]), names, values, C.c_size_t(len(env)),
                                      C.c_int(1 if case["timing"] else 0), C.c_int(drop), C.byref(rc))
        self.error = rc.value
        if not self.h:
            return
        self.h = C.c_void_p(self.h)
        buf = C.create_string_buffer(1 << 18)
        self.L.emu_case_dump.restype = C.c_long
        assert self.L.emu_case_dump(self.h, buf, C.c_size_t(len(buf))) < len(buf)
        self.lines = buf.value.decode().splitlines()
        ops, shape = np.zeros((4096, 7), np.uint32), np.zeros(len(SHAPE) + 16, np.int64)
        self.L.emu_case_ops.restype = C.c_long
        k = self.L.emu_case_ops(self.h, ops.ctypes.data_as(C.c_void_p), C.c_size_t(len(ops)), shape.ctypes.data_as(C.c_void_p))
        assert 0 < k <= len(ops)
        self.ops = ops[:k].astype(np.int64)
        self.shape = dict(zip(SHAPE, (int(v) for v in shape)))
        self.msm_tab = [int(v) for v in shape[len(SHAPE):]]
        assert self.shape["num_ops"] == k
        blocks = np.zeros((1024, 3), np.int32)
        self.L.emu_case_blocks.restype = C.c_long
        k = self.L.emu_case_blocks(self.h, blocks.ctypes.data_as(C.c_void_p), C.c_size_t(len(blocks)))
        assert 0 < k <= len(blocks)
        self.blocks = [tuple(int(v) for v in b) for b in blocks[:k]]

    def close(self):
        if self.h:
            self.L.emu_case_close(self.h)
            self.h = None

    def run(self, inputs, order=None):
        """the plan on the rows of `inputs` (msg, r, s, pkx, pky, qx, qy; None where the program has none), poisoned scratch and
        output: (cols, err, valid, flagged count)"""
        n = next(a for a in inputs if a is not None).shape[0]
        cols = np.zeros((self.shape["num_cols"], n), np.uint64)
        err, valid = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        P = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
        o = np.ascontiguousarray(order, np.int32) if order is not None else None
        self.L.emu_case_exec.restype = C.c_long
        bad = self.L.emu_case_exec(self.h, *[P(a) for a in inputs], P(cols), C.c_size_t(n), C.c_size_t(n), P(err), P(valid), P(o),
                                   C.c_size_t(0 if o is None else len(o)), C.c_int(1))
        return cols, err, valid, bad


@pytest.fixture(scope="module")
def plans():
    subprocess.check_call(["make", "-s", "-C", HERE])   # (a harness built before the exports existed is rebuilt)
    return plan_cases.Plans()


@pytest.fixture(scope="module")
def opened(plans):
    """case id -> Case (None where build refuses), opened once"""
    cache = {}

    def get(cid):
        if cid not in cache:
            c = Case(plans, BY_ID[cid])
            assert c.h or c.error == TOO_MANY_PIECES, (cid, c.error)
            cache[cid] = c if c.h else None
        return cache[cid]

    yield get
    for c in cache.values():
        if c is not None:
            c.close()


# ---- the happens-before relation of a plan's text form -----------------------------------------------------------------------
def _fields(line):
    kind, *kv = line.split()
    return kind, dict(x.split("=") for x in kv)


class Order:
    """steps = the lines without END.  A step is ordered after the previous step on its stream; a WAIT after the most recent
    earlier RECORD of its event; anc[j] = the set (bit mask) of steps that happen before step j"""

    def __init__(self, lines):
        assert lines[-1].startswith("END ")
        self.steps = [_fields(x) for x in lines[:-1]]
        self.anc = []
        last_on, last_record = {}, {}
        for j, (kind, f) in enumerate(self.steps):
            preds = []
            if f["st"] in last_on:
                preds.append(last_on[f["st"]])
            if kind == "WAIT" and f["ev"] in last_record:   # (an event nothing has recorded counts as satisfied: no ordering)
                preds.append(last_record[f["ev"]])
            a = 0
            for p in preds:
                a |= self.anc[p] | (1 << p)
            self.anc.append(a)
            last_on[f["st"]] = j
            if kind == "RECORD":
                last_record[f["ev"]] = j
        self.compute = [j for j, (kind, _f) in enumerate(self.steps) if kind in COMPUTE]

    def before(self, a, b):
        return bool((self.anc[b] >> a) & 1)

    def records(self, ev):
        return [j for j, (kind, f) in enumerate(self.steps) if kind == "RECORD" and f["ev"] == ev]

    def early(self, x):
        """E(x): the ancestors of x in list order, x, every remaining step in list order -- a legal execution of the plan"""
        first = [j for j in range(x) if (self.anc[x] >> j) & 1]
        taken = set(first) | {x}
        return first + [x] + [j for j in range(len(self.steps)) if j not in taken]


# ---- who reads what: the table of DESIGN.md section 5 (What a plan must order), applied to the op table -------------------
class Model:
    """The steps of a plan by the ops they cover, and the orderings the data requires.  violations(): a list of strings."""

    def __init__(self, case, order):
        self.c, self.o, self.s = case, order, case.shape
        self.kind, self.flags, self.ref1, self.ref2, self.col, self.ncols, self.cadd = case.ops.T
        n = self.s["num_ops"]
        self.chain, self.binv, self.expand = [None] * n, [None] * n, [None] * n
        self.walk = {}      # CHAIN step -> its ops as rows of ops walked in order by one lane (rows are walked side by side)
        self.runs = {}      # EXPAND_RUNS / EXPAND_FB_RUN step -> its runs (each walked by one lane with the point in registers)
        self.problems, self._cands = [], {}
        self.scalar = None
        for j, (kind, f) in enumerate(order.steps):
            if kind == "SCALAR":
                self.scalar = j
            elif kind == "CHAIN":
                lo = int(f["lo"])
                if f["form"] == "rows":
                    rows, count = int(f["rows"]), int(f["count"])
                    self.walk[j] = [[lo + r + k * rows for k in range(count)] for r in range(rows)]
                else:
                    self.walk[j] = [list(range(lo, int(f["hi"])))]
                for row in self.walk[j]:
                    for t in row:
                        self._cover(self.chain, t, j)
            elif kind == "BINV":
                for t in range(int(f["lo"]), int(f["hi"])):
                    self._cover(self.binv, t, j)
            elif kind == "EXPAND_OPS":
                for t in range(int(f["s_lo"]), int(f["s_hi"])):
                    self._cover(self.expand, t, j)
            elif kind == "EXPAND_RUNS":
                st, lb, ri = self.s["stride"], self.s["loop_begin"], int(f["run_iters"])
                it0, it1 = int(f["it0"]), int(f["it1"])
                self.runs[j] = [list(range(lb + st * a, lb + st * min(a + ri, it1))) for a in range(it0, it1, ri)]
                for run in self.runs[j]:
                    for t in run:
                        self._cover(self.expand, t, j)
            elif kind == "EXPAND_FB_RUN":
                fb, fw = self.s["fb_begin"], self.s["fb_windows"]
                self.runs[j] = [list(range(fb, fb + fw))]
                for t in self.runs[j][0]:
                    self._cover(self.expand, t, j)
        self.dyn_of = {int(self.cadd[t]): t for t in range(n) if self.kind[t] == OP_CADD}
        self.finalize = [j for j, (kind, _f) in enumerate(order.steps) if kind == "FINALIZE"]

    def _cover(self, table, t, j):
        if not 0 <= t < len(table) or table[t] is not None:
            self.problems.append(f"op {t} is covered twice or lies outside the program (step {j})")
        else:
            table[t] = j

    # the ops whose result a reference may resolve to at run time (a conditional add passes its first operand on when its
    # digit is zero), and whether it may resolve to a slot the scalar phase wrote
    def cands(self, ref):
        if ref not in self._cands:
            self._cands[ref] = self._cands_of(ref)
        return self._cands[ref]

    def _cands_of(self, ref):
        kind, rid = ref >> 24, ref & 0xFFFFFF
        n = self.s["num_ops"]
        if kind == R_SLOT:
            return (frozenset([rid]), False) if rid < n else (frozenset(), True)
        if kind == R_SELSLOT:
            rid &= 0xFFF
            return (frozenset([rid]), False) if rid < n else (frozenset(), True)
        if kind == R_DYN:
            c = self.dyn_of[rid]
            ops, scalar = self.cands(int(self.ref1[c]))
            return ops | {c}, scalar
        if kind == R_MSMTAB:
            ops, scalar = set(), True      # (the digit and the resolved table entry are the scalar phase's)
            for r in self.c.msm_tab:
                o2, s2 = self.cands(int(r))
                ops |= o2
            return frozenset(ops), scalar
        if kind == R_FBTAB:
            return frozenset(), True       # (the window digit)
        return frozenset(), False          # R_CONST

    def need(self, writer, reader, why):
        if writer is None or reader is None:
            self.problems.append(f"{why}: no step does it")
        elif writer != reader and not self.o.before(writer, reader):
            self.problems.append(f"{why}: step {writer} [{self._show(writer)}] is not ordered before step {reader} [{self._show(reader)}]")

    def _show(self, j):
        kind, f = self.o.steps[j]
        return kind + " " + " ".join(f"{k}={v}" for k, v in f.items())

    def affine_writer(self, c):
        """the step that leaves the affine form of op c in memory: its inversion batch, or -- a fixed-base window of the
        one-run expansion -- that expansion (it stores the running point for the op after the windows); None: nobody"""
        if not self.flags[c] & F_NO_AFFINE:
            return self.binv[c]
        e = self.expand[c]
        return e if e is not None and self.o.steps[e][0] == "EXPAND_FB_RUN" else None

    def read_jacobian(self, ref, reader, earlier, t):
        ops, scalar = self.cands(ref)
        if scalar:
            self.need(self.scalar, reader, f"op {t} reads what the scalar phase wrote")
        for c in ops:
            if c in earlier:
                continue                   # carried in registers, or stored earlier by the same lane
            if self.chain[c] == reader:
                self.problems.append(f"op {t} reads the Jacobian result of op {c}, which the same launch computes in another lane or later")
            elif self.flags[c] & F_NO_AFFINE:
                self.problems.append(f"op {t} reads X, Y of op {c} from memory, which F_NO_AFFINE never stores")
            else:
                self.need(self.chain[c], reader, f"chain op {t} reads the Jacobian result of op {c}")

    def read_affine(self, ref, reader, t, carried=()):
        ops, scalar = self.cands(ref)
        if scalar:
            self.need(self.scalar, reader, f"op {t} reads what the scalar phase wrote")
        for c in ops:
            if c in carried:
                continue
            w = self.affine_writer(c)
            if w is None:
                self.problems.append(f"op {t} reads the affine form of op {c}, which nothing leaves in memory (F_NO_AFFINE)")
            elif w == reader:
                self.problems.append(f"op {t} reads the affine form of op {c}, which the same launch writes")
            else:
                self.need(w, reader, f"op {t} reads the affine form of op {c}")

    def violations(self):
        n = self.s["num_ops"]
        o = self.o
        # 1. everything happens before FINALIZE, which is on the caller's stream
        if len(self.finalize) != 1 or o.steps[self.finalize[0]][1]["st"] != "caller" or self.finalize[0] != len(o.steps) - 1:
            self.problems.append("FINALIZE is not the one last step on the caller's stream")
        else:
            for j in o.compute:
                self.need(j, self.finalize[0], "FINALIZE ends the call")
        if self.scalar is None or o.steps[self.scalar][1]["st"] != "caller":
            self.problems.append("no SCALAR step on the caller's stream")
        # 2. per op
        for t in range(n):
            self.need(self.scalar, self.chain[t], f"CHAIN of op {t} after SCALAR")
            self.need(self.chain[t], self.binv[t], f"BINV of op {t} after its CHAIN")
            self.need(self.binv[t], self.expand[t], f"EXPAND of op {t} after its BINV")
            self.need(self.chain[t], self.expand[t], f"EXPAND of op {t} after its CHAIN (resolved operand ids)")
        for j, rows in self.walk.items():
            f = o.steps[j][1]
            affine = f.get("affine") == "1"
            for row in rows:
                for k, t in enumerate(row):
                    earlier = set(row[:k])
                    self.read_jacobian(int(self.ref1[t]), j, earlier, t)
                    if self.kind[t] != OP_DBL:
                        if (int(self.ref2[t]) >> 24) == R_MSMTAB and affine:
                            self.read_affine(int(self.ref2[t]), j, t)
                        else:
                            self.read_jacobian(int(self.ref2[t]), j, earlier, t)
            if f.get("cont") == "1":    # the range extends the inversion batch of the op before it: reads its prefix product and Z
                lo = int(f["lo"])
                if lo < 1 or self.chain[lo - 1] == j:
                    self.problems.append(f"step {j} continues a prefix it computes itself")
                else:
                    self.need(self.chain[lo - 1], j, f"chain at op {lo} continues the prefix products of op {lo - 1}")
        for j, (kind, f) in enumerate(o.steps):
            if kind == "BINV" and f["prefix"] == "1":
                # the batch runs on phase A's prefix products: the chain launches over [lo, hi) must have formed ONE product, that is
                # a launch that starts at lo with a fresh product and launches that continue it
                lo, hi = int(f["lo"]), int(f["hi"])
                at = lo
                while at < hi:
                    cj = self.chain[at]
                    cf = o.steps[cj][1] if cj is not None else {}
                    if cj is None or cf.get("form") == "rows" or int(cf["lo"]) != at or (cf["cont"] == "1") != (at != lo):
                        self.problems.append(f"step {j}: the prefix products of [{lo}, {hi}) are not one product (at op {at})")
                        break
                    at = int(cf["hi"])
                if at > hi:
                    self.problems.append(f"step {j}: a chain launch runs past the inversion batch [{lo}, {hi})")
            elif kind == "EXPAND_OPS":
                for t in range(int(f["s_lo"]), int(f["s_hi"])):
                    self.read_affine(int(self.ref1[t]), j, t)
                    if self.kind[t] != OP_DBL:
                        self.read_affine(int(self.ref2[t]), j, t)
        for j, runs in self.runs.items():
            for run in runs:
                for k, t in enumerate(run):
                    if k == 0:
                        self.read_affine(int(self.ref1[t]), j, t)
                    else:   # the running point is in registers: the operand must be a result of this run
                        ops, _scalar = self.cands(int(self.ref1[t]))
                        first_ops, _s = self.cands(int(self.ref1[run[0]]))
                        if not ops <= set(run[:k]) | first_ops:
                            self.problems.append(f"op {t} of a run takes a first operand from outside its run")
                    if self.kind[t] != OP_DBL:
                        self.read_affine(int(self.ref2[t]), j, t)
            if o.steps[j][0] == "EXPAND_FB_RUN":
                # it leaves the running point in the affine slot of the first operand of op t_after: that slot must not be one an
                # inversion batch also writes, and the reader is ordered behind it by read_affine (affine_writer)
                t_after = int(o.steps[j][1]["t_after"])
                ops, _scalar = self.cands(int(self.ref1[t_after]))
                for c in ops:
                    if not self.flags[c] & F_NO_AFFINE:
                        self.problems.append(f"the fixed-base run may store over the affine form of op {c}, which an inversion batch writes")
        # an op without an affine form must be expanded inside a run
        for t in range(n):
            if self.flags[t] & F_NO_AFFINE and (self.expand[t] is None or self.expand[t] not in self.runs):
                self.problems.append(f"op {t} is F_NO_AFFINE but expanded on its own")
        return self.problems

    # ---- the segment contract ----
    def block_violations(self):
        blocks, num_cols = self.c.blocks, self.s["num_cols"]
        out = []
        covered = np.zeros(num_cols, np.int32)
        for c0, nc, _e in blocks:
            if nc <= 0 or c0 < 0 or c0 + nc > num_cols:
                out.append(f"block ({c0}, {nc}) lies outside the program")
            else:
                covered[c0:c0 + nc] += 1
        twice, never = np.nonzero(covered > 1)[0], np.nonzero(covered == 0)[0]
        if len(twice):
            out.append(f"columns listed twice: {_ranges(twice)}")
        if len(never):
            out.append(f"columns in no block: {_ranges(never)}")
        total = sum(nc for _c0, nc, _e in blocks)
        if total != num_cols:
            out.append(f"sum(num_cols) = {total}, the program has {num_cols} columns")
        events = [e for _c0, _nc, e in blocks]
        scalar_blocks = sum(1 for e in events if e < 0)
        if any(e >= 0 for e in events[:scalar_blocks]) or any(e < 0 for e in events[scalar_blocks:]):
            out.append("scalar-phase blocks are not first")
        # (expansion launches are numbered in issue order: the events must not decrease)
        if events[scalar_blocks:] != sorted(events[scalar_blocks:]):
            out.append("blocks are not in issue order")
        # the launch index of an expansion step = its rank among the expansion steps of the list
        launch = {}
        for j, (kind, _f) in enumerate(self.o.steps):
            if kind in EXPAND:
                launch[len(launch)] = j
        owner = np.full(num_cols, -1, np.int64)
        for t in range(self.s["num_ops"]):
            owner[self.col[t]:self.col[t] + self.ncols[t]] = t
        for c0, nc, e in blocks:
            rec = self.o.records("t1" if e < 0 else f"c1[{e}]")
            if len(rec) != 1:
                out.append(f"block ({c0}, {nc}): its event is recorded {len(rec)} times")
                continue
            if e >= 0 and (e not in launch or not self.o.before(launch[e], rec[0])):
                out.append(f"block ({c0}, {nc}): event c1[{e}] is not recorded behind expansion launch {e}")
            writers = set()
            for t in np.unique(owner[c0:c0 + nc]):
                writers.add(self.scalar if t < 0 else self.expand[int(t)])
            for w in writers:
                if w is None or not self.o.before(w, rec[0]):
                    out.append(f"block ({c0}, {nc}, event {e}): step {w} writes into it and is not ordered before the event's RECORD")
        return out


def _ranges(idx):
    idx = [int(v) for v in idx]
    out, a = [], idx[0]
    for x, y in zip(idx, idx[1:] + [None]):
        if y != x + 1:
            out.append(f"{a}..{x}")
            a = y
    return ", ".join(out)


# ---- B: static checks over every case ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c["id"] for c in CASES])
def test_waits_order_every_reader_behind_its_writer(opened, cid):
    """DESIGN.md section 5, What a plan must order: FINALIZE behind every compute step; per op CHAIN behind SCALAR, BINV behind CHAIN, EXPAND behind BINV; every
    operand that names another op's result read behind the step that wrote the form it is read in"""
    case = opened(cid)
    if case is None:   # build refuses this record (test_knobs_cpu.py checks when it must): there is no plan to check
        return
    problems = Model(case, Order(case.lines)).violations()
    assert not problems, "\n".join(problems[:12])


@pytest.mark.parametrize("cid", [c["id"] for c in CASES])
def test_column_blocks_are_disjoint_cover_the_program_and_are_final_at_their_event(opened, cid):
    """include/p2e.h p2e_segments_describe, from plan::column_blocks of the case's plan"""
    case = opened(cid)
    if case is None:   # build refuses this record (test_knobs_cpu.py checks when it must): there is no plan to check
        return
    problems = Model(case, Order(case.lines)).block_violations()
    assert not problems, "\n".join(problems[:12])
    assert sum(nc for _c0, nc, _e in case.blocks) == case.shape["num_cols"]


def test_the_case_api_dumps_what_emu_plan_dump_dumps(plans, opened):
    for cid in ("builtin:verify:default", "builtin:glv_mul:large", "curve:verify_p256:runs", "curve:msm_secp256k1:default"):
        lines, _shape = plans.of(BY_ID[cid])
        assert opened(cid).lines == lines


# ---- C: adversarial execution -------------------------------------------------------------------------------------------------------
EXEC_CASES = ([f"builtin:verify:{k}" for k in ("default", "lane", "lane_runs", "large", "large_fb_run", "many_waits", "layout_MFB2")] +
              [f"builtin:glv_mul:{k}" for k in ("default", "large")] +
              [f"curve:{p}:{k}" for p in ("windowed_secp256k1", "scalar_mul_p256", "verify_p256", "msm_p256", "fixed_base_secp256k1")
               for k in ("default", "no_quad", "runs", "fb_serial", "no_alt_b")])


def _pack(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), np.uint8).reshape(-1, 32).copy()


@functools.lru_cache(maxsize=None)
def _batch(program):
    """three elements, two clean and one flagged (the reference panics on it: inverse of zero), the blinding point, and the C
    oracle's (cols, err, verdicts) of them: (inputs of emu_case_exec, blind or None, want)"""
    import adversarial_inputs as A
    import oracle_c
    import plonky2_ecdsa_amd as p2e
    import p2e_ref as R
    name, _, cname = program.rpartition("_")
    curve = {"secp256k1": 0, "p256": 1}.get(cname)
    if curve is None:   # the built-in programs
        sig = [a[:3].copy() for a in p2e.synth_signatures(seed=77, n=3)]
        if program == "verify":
            sig[2][1] = 0                                         # s = 0
            want = oracle_c.verify_witness(*sig)
            return tuple(sig) + (None, None), None, want
        px, py, k = sig[3], sig[4], sig[0]
        k[1] = 0                                                  # k = 0
        want = oracle_c.glv_mul_witness(px, py, k)
        return (k, k, k, px, py, None, None), None, want
    cv = R.P256 if curve else R.SECP256K1
    blind = A.blind(curve)
    bl = (_pack([blind[0]])[0], _pack([blind[1]])[0])
    sig = [a.copy() for a in p2e.synth_signatures_curve(curve, seed=78, n=3)]
    if name == "verify":
        sig[2][1] = 0
        cols, _aux, err, flags = oracle_c.curve_program(oracle_c.CP_VERIFY, curve, blind, sig, want_aux=False)
        return tuple(sig) + (None, None), bl, (cols, err, flags)
    if name in ("windowed", "scalar_mul"):
        px, py, k = sig[3], sig[4], sig[0]
        k[1] = 0
        kind = oracle_c.CP_WINDOWED_MUL if name == "windowed" else oracle_c.CP_SCALAR_MUL
        cols, _aux, err, flags = oracle_c.curve_program(kind, curve, blind, (px, py, k), want_aux=False)
        return (k, k, k, px, py, None, None), bl, (cols, err, flags)
    if name == "msm":
        other = p2e.synth_signatures_curve(curve, seed=79, n=3)
        px, py, qx, qy, ns, ms = sig[3], sig[4], other[3].copy(), other[4].copy(), sig[0], other[0].copy()
        ns[1] = 0
        ms[1] = 0                                                 # n = m = 0
        cols, _aux, err, flags = oracle_c.curve_msm(curve, px, py, qx, qy, ns, ms, want_aux=False)
        return (ns, ms, ns, px, py, qx, qy), None, (cols, err, flags)
    assert name == "fixed_base"
    k = sig[0]
    k[1] = 0
    base = A.mul(cv, 0xBA5E + 1, cv.g)
    cols, _aux, err, flags = oracle_c.curve_fixed_base(curve, base, k, want_aux=False)
    return (k, k, k, k, k, None, None), (_pack([base[0]])[0], _pack([base[1]])[0]), (cols, err, flags)


def _open_for_exec(plans, cid, drop=-1):
    case = dict(BY_ID[cid])
    inputs, blind, want = _batch(case["program"])
    case["blind"] = blind
    c = Case(plans, case, drop)
    assert c.h, (cid, c.error)
    return c, inputs, want


def _differing(case, order, inputs, base):
    """the compute steps X whose E(X) does not reproduce `base` (the list-order run)"""
    out = []
    for x in order.compute:
        got = case.run(inputs, order.early(x))
        if not all(np.array_equal(a, b) for a, b in zip(got[:3], base[:3])) or got[3] != base[3]:
            out.append(x)
    return out


@pytest.mark.parametrize("cid", EXEC_CASES)
def test_every_order_the_waits_permit_computes_the_list_order_result(plans, cid):
    """The real bodies on a poisoned scratch.  For each compute step X the order E(X) runs X as early as the waits permit: a
    missing ordering of X behind a writer makes X read poison, a missing ordering of a reader behind X makes the reader read
    what X has overwritten.  The plan is the one the case's own n chooses, executed on three elements."""
    case, inputs, want = _open_for_exec(plans, cid)
    try:
        order = Order(case.lines)
        base = case.run(inputs)
        wcols, werr, wflags = want
        clean = werr == 0
        assert clean.tolist() == [True, False, True] and base[3] == 1        # the expectation is the C oracle's
        assert np.array_equal(base[1], werr) and np.array_equal(base[2][clean], wflags[clean]) and not base[2][~clean].any()
        assert np.array_equal(base[0][:, clean], wcols[:, clean])
        again = case.run(inputs, list(range(len(order.steps))))
        assert all(np.array_equal(a, b) for a, b in zip(again[:3], base[:3]))
        assert len(order.compute) >= 4
        bad = _differing(case, order, inputs, base)
        assert not bad, [(x, case.lines[x]) for x in bad]
    finally:
        case.close()


# ---- mutations: a deleted WAIT is noticed by both checks -----------------------------------------------------------------------------
MUTATED = ("builtin:verify:default", "builtin:verify:large", "curve:verify_p256:default")


def _waits(lines, streams, prefix):
    """indices of the WAIT steps of the given streams on events `prefix[k]`"""
    out = []
    for j, line in enumerate(lines[:-1]):
        kind, f = _fields(line)
        if kind == "WAIT" and f["ev"].startswith(prefix) and (streams is None or f["st"] in streams):
            out.append(j)
    return out


def _roles(lines):
    """stream -> the kinds of compute step it carries"""
    roles = {}
    for line in lines[:-1]:
        kind, f = _fields(line)
        if kind in COMPUTE:
            roles.setdefault(f["st"], set()).add("EXPAND" if kind in EXPAND else kind)
    return roles


def _mutations(cid, lines):
    """(name, step): the WAIT of an expansion stream on binv[k] that precedes the first expansion of piece k, the WAIT of an
    inversion stream on piece[k], for every piece; built-in verify: the WAIT of M on `fixed`"""
    roles = _roles(lines)
    out = []
    n_seg = int(_fields(lines[-1])[1]["n_seg"])
    for k in range(n_seg):
        # the binv[k] wait that guards piece k's own expansion: the last one before an expansion launch that follows BINV k in the
        # list (the four-lane plan waits for binv[k] again in front of later pieces: those are the few_waits / many_waits extras)
        own = [j for j in _waits(lines, None, f"binv[{k}]") if "EXPAND" in roles.get(_fields(lines[j])[1]["st"], ())]
        if own:
            out.append((f"expand_waits_binv[{k}]", own[0]))
        inv = [j for j in _waits(lines, None, f"piece[{k}]") if "BINV" in roles.get(_fields(lines[j])[1]["st"], ())]
        if inv:
            out.append((f"binv_waits_piece[{k}]", inv[0]))
    if cid.startswith("builtin:verify"):
        fx = _waits(lines, ("M",), "fixed")
        assert len(fx) == 1
        out.append(("final_add_waits_fixed", fx[0]))
    return out


def _orders_nothing(lines, drop):
    """the plan without step `drop` has the same happens-before relation on its other steps"""
    a, b = Order(lines), Order(lines[:drop] + lines[drop + 1:])
    low = (1 << drop) - 1

    def without(mask):
        return (mask & low) | ((mask >> (drop + 1)) << drop)

    return all(without(a.anc[j]) == b.anc[j - (j > drop)] for j in range(len(a.steps)) if j != drop)


def _mutation_outcome(plans, cid, drop):
    """(violations of the static check, compute steps whose early order differs from the UNMUTATED list-order result)"""
    ref, inputs, _want = _open_for_exec(plans, cid)
    case, _i, _w = _open_for_exec(plans, cid, drop)
    try:
        assert case.lines == ref.lines[:drop] + ref.lines[drop + 1:]
        order = Order(case.lines)
        model = Model(case, order)
        static = model.violations() + model.block_violations()
        base = ref.run(inputs)
        assert all(np.array_equal(a, b) for a, b in zip(case.run(inputs)[:3], base[:3]))   # (list order: the waits do not matter)
        return static, _differing(case, order, inputs, base)
    finally:
        ref.close()
        case.close()


@pytest.mark.parametrize("role", ["expand_waits_binv", "binv_waits_piece", "final_add_waits_fixed"])
@pytest.mark.parametrize("cid", MUTATED)
def test_a_deleted_wait_is_noticed_statically_and_by_an_early_order(plans, cid, role):
    """every piece's wait of that role, deleted in turn"""
    lines, _shape = plans.of(BY_ID[cid])
    todo = [(name, j) for name, j in _mutations(cid, lines) if name.startswith(role)]
    if role == "final_add_waits_fixed" and not cid.startswith("builtin:verify"):
        assert not todo
        return
    assert todo
    missed = []
    for name, drop in todo:
        assert lines[drop].startswith("WAIT "), lines[drop]
        if _orders_nothing(lines, drop):
            # a stream waiting for an event recorded on that same stream (the fixed-base pieces of the built-in verifier are
            # chained AND inverted on F): the queue orders the two launches, the wait adds nothing, and no check can miss it
            assert role == "binv_waits_piece" and cid.startswith("builtin:verify") and lines[drop].startswith("WAIT st=F ")
            continue
        static, dynamic = _mutation_outcome(plans, cid, drop)
        if not static:
            missed.append(f"{name}: the static check accepts the plan without step {drop} `{lines[drop]}`")
        if not dynamic:
            missed.append(f"{name}: no early order of the plan without step {drop} `{lines[drop]}` computes anything else")
    assert not missed, "\n".join(missed)


def test_every_piece_of_the_mutated_cases_has_both_waits(plans):
    """(so that the parametrisation above cannot shrink unnoticed: one expansion wait per piece, one inversion wait per piece
    whose batch is on another stream than its chain)"""
    for cid in MUTATED:
        lines, _shape = plans.of(BY_ID[cid])
        n_seg = int(_fields(lines[-1])[1]["n_seg"])
        names = [name for name, _j in _mutations(cid, lines)]
        assert sum(x.startswith("expand_waits_binv") for x in names) == n_seg
        # (at most the window table's batch runs on its chain's own stream and needs no wait)
        assert n_seg - 1 <= sum(x.startswith("binv_waits_piece") for x in names) <= n_seg
        assert ("final_add_waits_fixed" in names) == cid.startswith("builtin:verify")


def test_report_the_extra_waits_of_the_four_lane_plan(plans, capsys):
    """Not a pass / fail condition (What a plan must order records the outcome): the waits of an expansion stream on EARLIER inversion
    batches in the four-lane plan of the built-in verifier -- the few_waits pair and the many_waits list -- each dropped in turn:
    either the checks notice, or the remaining waits already imply it."""
    report = []
    for cid in ("builtin:verify:default", "builtin:verify:many_waits"):
        lines, _shape = plans.of(BY_ID[cid])
        own = {j for _name, j in _mutations(cid, lines)}
        roles = _roles(lines)
        extra = [j for j in _waits(lines, None, "binv[") if j not in own and "EXPAND" in roles.get(_fields(lines[j])[1]["st"], ())]
        caught_s = caught_d = 0
        for j in extra:
            static, dynamic = _mutation_outcome(plans, cid, j)
            caught_s += bool(static)
            caught_d += bool(dynamic)
            if static or dynamic:
                report.append(f"{cid}: needs step {j} `{lines[j]}` (static check: {'caught' if static else 'not caught'}, early "
                              f"orders: {'caught' if dynamic else 'not caught'})")
        report.append(f"{cid}: {len(extra)} extra waits; without one of them, in turn: {caught_s} noticed by the static check, {caught_d} by an "
                      f"early order; the others are implied by the remaining waits or order nothing a reader needs")
    with capsys.disabled():
        print("\n" + "\n".join(report))
