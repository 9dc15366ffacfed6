"""The launch plans that tests/golden/launch_plans.txt.gz pins, and the CPU side of reading them.

One case = (program, knobs and per-call switches, batch size, phase timing, container).  The fixture holds, per case, the
sequence of kernel launches, event records and stream waits the library issued for it, one line per step in the text form
of csrc/launch_plan.hpp (plan::dump); test_knobs_cpu.py compares choose + build with it line for line.  Thresholds are
crossed by the knob, not by a large batch: 700 elements are two full workgroups and a ragged tail."""
import ctypes as C
import gzip
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_plans.txt.gz")   # (9 000 lines of text: kept compressed, like the schedules)
N = 700
BUILTIN = {"verify": 0, "glv_mul": 1}
# (kind, curve) of include/p2e.h P2E_CP_* / P2E_CURVE_*: every kind on both curves (the verifier program is P-256 only)
CURVE_PROGRAMS = {f"{name}_{cname}": (kind, curve)
                  for name, kind in (("windowed", 1), ("scalar_mul", 2), ("verify", 3), ("msm", 4), ("fixed_base", 5))
                  for cname, curve in (("secp256k1", 0), ("p256", 1)) if not (kind == 3 and curve == 0)}

_LANE = {"P2E_QUAD_MAX_N": "0"}
_LANE_RUNS = {**_LANE, "P2E_RUNS_MIN_N": "0"}
_LARGE = {**_LANE_RUNS, "P2E_BINV_ALT_MAX_N": "0"}
BUILTIN_CASES = [
    ("default", {}, {}),
    ("lane", _LANE, {}),
    ("lane_runs", _LANE_RUNS, {}),
    ("large", _LARGE, {}),
    ("large_fb_run", {**_LARGE, "P2E_FB_RUN": "1"}, {}),
    ("op_by_op", {"P2E_RUN_ITERS_SMALL": "0"}, {}),
    ("takes_3_2", {"P2E_SMALL_TAKES": "3,2"}, {}),
    ("many_waits", {"P2E_QUAD_FEW_WAITS": "0"}, {}),
    ("b_first_on_binv", {"P2E_QUAD_B_FIRST_ON_FIXED": "0"}, {}),
    ("layout_1MFB2", {"P2E_STREAM_LAYOUT": "1MFB2"}, {}),
    ("layout_MFB2", {"P2E_STREAM_LAYOUT": "MFB2"}, {}),   # (no own expansion stream: the caller's carries the expansions)
    ("timing", {}, {"timing": True}),
    ("compact", {}, {"compact": True}),
    ("n8192", {}, {"n": 1 << 13}),
    ("n32768", {}, {"n": 1 << 15}),
    ("n65536", {}, {"n": 1 << 16}),
]
CURVE_CASES = [
    ("default", {}, {}),
    ("no_quad", {"P2E_CP_NO_QUAD": "1"}, {}),
    ("runs", {"P2E_CP_RUNS_MIN_N": "1"}, {}),
    ("fb_serial", {"P2E_CP_FB_SERIAL": "1"}, {}),
    ("no_alt_b", {"P2E_CP_NO_ALT_B": "1"}, {}),
    ("piece_ops_20", {"P2E_CP_PIECE_OPS_QUAD": "20"}, {}),
    ("tail_ops_0", {"P2E_CP_TAIL_OPS_QUAD": "0"}, {}),
]


def cases():
    """dicts: id, family (0 built-in, 1 curve), program (name), prog, curve, env, n, timing, compact"""
    out = []

    def add(family, program, prog, curve, name, env, extra):
        out.append(dict(id=f"{'curve' if family else 'builtin'}:{program}:{name}", family=family, program=program, prog=prog, curve=curve,
                        env=dict(env), n=extra.get("n", N), timing=extra.get("timing", False), compact=extra.get("compact", False)))

    for program, pid in BUILTIN.items():
        for name, env, extra in BUILTIN_CASES:
            add(0, program, pid, 0, name, env, extra)
    for program, (kind, curve) in CURVE_PROGRAMS.items():
        for name, env, extra in CURVE_CASES:
            add(1, program, kind, curve, name, env, extra)
    for n in (1 << 13, 1 << 16):
        add(1, "verify_p256", 3, 1, f"n{n}", {}, {"n": n})
    return out


def golden():
    """case id -> the fixture's lines for it"""
    got, cur = {}, None
    with gzip.open(GOLDEN, "rt") as f:
        for line in f:
            line = line.rstrip("\n")
            if line.startswith("# case "):
                cur = got.setdefault(line[len("# case "):], [])
            elif line and not line.startswith("#"):
                cur.append(line)
    return got


class Plans:
    """choose + build through tests/emu (emu_plan_dump)"""

    def __init__(self):
        self.L = C.CDLL(os.path.join(ROOT, "tests", "emu", "libp2e_emu.so"))
        self.L.emu_plan_dump.restype = C.c_long
        self._blind = {}

    def blind(self, curve):
        """a point of the curve (the plan does not depend on which)"""
        if curve not in self._blind:
            a = [np.zeros((1, 32), np.uint8) for _ in range(5)]
            self.L.emu_synth_signatures_curve(C.c_int(curve), C.c_uint64(99), C.c_size_t(0), C.c_size_t(1), *[x.ctypes.data_as(C.c_void_p) for x in a])
            self._blind[curve] = (a[3][0].copy(), a[4][0].copy())
        return self._blind[curve]

    def dump(self, family, prog, curve, env, n, timing=False):
        """(lines, shape) or (-error, shape); shape: num_ops, fb_begin, fb_windows, loop_begin, loop_iters, loop_stride, MAX_SEG, MAX_EXPAND"""
        names = (C.c_char_p * len(env))(*[k.encode() for k in env])
        values = (C.c_char_p * len(env))(*[str(v).encode() for v in env.values()])
        bx, by = self.blind(curve)
        buf, shape = C.create_string_buffer(1 << 18), (C.c_int32 * 8)()
        rc = self.L.emu_plan_dump(C.c_int(family), C.c_int(prog), C.c_int(curve), bx.ctypes.data_as(C.c_void_p), by.ctypes.data_as(C.c_void_p),
                                  C.c_size_t(n), names, values, C.c_size_t(len(env)), C.c_int(1 if timing else 0), buf, C.c_size_t(len(buf)),
                                  shape)
        assert rc < len(buf)
        return (buf.value.decode().splitlines() if rc >= 0 else rc), list(shape)

    def of(self, case):
        return self.dump(case["family"], case["prog"], case["curve"], case["env"], case["n"], case["timing"])


def mixed_batch(program, curve_id, synthetic):
    """96 rows for the emulator under the library's real plans: 64 synthetic valid rows (`synthetic`: the program's input
    arrays, 64 rows each) with 32 rows of tests/adversarial_inputs.py in their middle -- six flagged ones (two of them
    adjacent) and an even sample of the clean classes"""
    import adversarial_inputs as A
    rows, _marks = A.batch(program, curve_id)
    flagged = [c for c in rows if c.flagged][:6]
    clean = [c for c in rows if not c.flagged]
    adv = A.arrays(flagged[:2] + clean[::len(clean) // 26][:26] + flagged[2:])
    assert len(adv) == len(synthetic) and adv[0].shape[0] == 32 and all(a.shape[0] == 64 for a in synthetic)
    return [np.ascontiguousarray(np.concatenate([s[:40], a, s[40:]])) for s, a in zip(synthetic, adv)]
