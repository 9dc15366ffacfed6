"""The C oracle's constraint-block (ux) and gate-internal matrices as expectations, shared by the CPU and GPU tests that
compare those two passes on every element and column (oracle/p2e_oracle.h, the *_full walks).

Nothing here uses the code under test.  A program is named as the tests name it: ("builtin", 0 | 1) for the verifier and
glv_mul, ("curve", kind, curve) for a curve program.  An expectation holds u64 numpy matrices; to_device() uploads them once
in the forms the GPU outputs have (ux as int32 and as int64)."""
import bisect

import numpy as np

import oracle_c
import p2e_ref as R

CURVES = [R.SECP256K1, R.P256]
LOCKSTEP = 64            # the lock-step walk: the same values, one Fermat ladder per group and inverse


def layout(family, prog, curve=0):
    """the oracle's layout of a program: num_cols, num_aux, num_ux, num_gate, blocks (one per generator)"""
    if family == "builtin":
        return oracle_c.program_layout(oracle_c.PROG_VERIFY if prog == 0 else oracle_c.PROG_GLV_MUL, 0)
    return oracle_c.program_layout(prog, curve)


def builtin(program, arrs, nthreads=0):
    """dict(cols, aux, ux, gate, err, verdict) of a built-in program; arrs as the fill takes them"""
    if program == 0:
        out = oracle_c.verify_witness_full(*arrs, nthreads=nthreads, lockstep=LOCKSTEP)
    else:
        out = oracle_c.glv_mul_witness_full(*arrs, nthreads=nthreads)
    return dict(zip(("cols", "aux", "ux", "gate", "err", "verdict"), out))


def curve_program(kind, curve, point, host, nthreads=0):
    """the same for a curve program: point = the blinding point (kinds 1-3) or the base (kind 5), as integers; host = the
    input arrays in the order of the program's fill: (px, py, k), (msg, r, s, pkx, pky) or (px, py, qx, qy, n, m)"""
    if kind == oracle_c.CP_MSM:
        out = oracle_c.curve_msm_full(curve, *host, nthreads=nthreads, lockstep=LOCKSTEP)
    elif kind == oracle_c.CP_FIXED_BASE_MUL:
        out = oracle_c.curve_fixed_base_full(curve, point, host[-1], nthreads=nthreads, lockstep=LOCKSTEP)
    else:
        out = oracle_c.curve_program_full(kind, curve, point, host, nthreads=nthreads, lockstep=LOCKSTEP)
    return dict(zip(("cols", "aux", "ux", "gate", "err", "verdict"), out))


def generator_of(blocks, col):
    """index of the generator whose constraint block holds ux column col (blocks: [(first, count)] in column order)"""
    # (a block without columns shares its first column with the next one: the last block that starts at or before col)
    return bisect.bisect_right([b[0] for b in blocks], col) - 1


def differs(what, pairs, total, got_at, want_at, blocks=None, labels=None):
    """the report the hash tests give: how many, and the first few (column, element) pairs with the generator they belong to"""
    lines = [f"{what}: {total} differing values; first:"]
    for c, i in pairs[:6]:
        where = ""
        if blocks is not None:
            g = generator_of(blocks, c)
            where = f" (generator {g}" + (f" {labels[g]}" if labels else "") + f", column {c - blocks[g][0]} of its {blocks[g][1]})"
        lines.append(f"  column {c}{where}, element {i}: got {got_at(c, i)} want {want_at(c, i)}")
    return "\n".join(lines)


def assert_same_numpy(what, got, want, clean=None, blocks=None, labels=None):
    """got == want on every column of every element (of the clean ones, where a mask is given)"""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if clean is not None and not clean.all():
        got, want, index = got[:, clean], want[:, clean], np.nonzero(clean)[0]
    else:
        index = np.arange(got.shape[1])
    if np.array_equal(got, want):
        return
    cs, es = np.nonzero(got != want)
    pairs = [(int(c), int(e)) for c, e in zip(cs[:6], es[:6])]
    msg = differs(what, [(c, int(index[e])) for c, e in pairs], len(cs), lambda c, i: None, lambda c, i: None, blocks, labels)
    vals = "; ".join(f"got {int(got[c, e])} want {int(want[c, e])}" for c, e in pairs)
    raise AssertionError(msg + "\n  values: " + vals)


# ---- on the device -----------------------------------------------------------------------------------------------------
def to_device(torch, exp):
    """uploads one expectation: ux as int32 and int64 (every value is below 2^29), gate as int64, the clean-row mask"""
    assert int(exp["ux"].max()) < 1 << 29
    ux32 = torch.from_numpy(exp["ux"].astype(np.uint32).view(np.int32)).cuda()
    dev = dict(ux32=ux32, gate=torch.from_numpy(exp["gate"].view(np.int64)).cuda() if exp["gate"].shape[0] else None,
               clean=torch.from_numpy(exp["err"] == 0).cuda(), all_clean=not exp["err"].any())
    return dev


def assert_same_device(torch, what, got, want, dev, blocks=None):
    """got (int32 or int64 device matrix, any row stride) == want (int32 or int64) on every clean element; only the
    differing positions come back to the host"""
    assert tuple(got.shape) == tuple(want.shape), (what, tuple(got.shape), tuple(want.shape))
    if got.dtype != want.dtype:
        want = want.to(got.dtype)
    if dev["all_clean"] and torch.equal(got, want):
        return
    ne = got != want
    if not dev["all_clean"]:
        ne &= dev["clean"][None, :]
    total = int(ne.sum())
    if total == 0:
        return
    first = ne.nonzero()[:6].cpu().numpy()
    pairs = [(int(c), int(i)) for c, i in first]
    raise AssertionError(differs(what, pairs, total, lambda c, i: int(got[c, i]), lambda c, i: int(want[c, i]), blocks))
