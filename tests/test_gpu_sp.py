"""Silent payments on the GPU (include/p2e.h p2e_sp_input_hash_batch, p2e_sp_label_batch, p2e_sp_send_batch, p2e_sp_scan_batch)
through the C ABI.

Expectations come from tests/sp_inputs.py alone: a restatement of BIP-352 in Python integers and hashlib.  Every byte of every
element is compared; output buffers are pre-filled with 0xAA so that an unwritten byte shows, and hold one element more than the
call may write.

Shapes: every call at count = 0, 1, 63, 64, 65 and 257 (nothing, one lane, a wave less one, a wave, a wave plus one, a block
plus one).  The first wave of the scan holds a transaction with three hits beside one without outputs and one with forty
decoys, so the k loops of one wave diverge.  The arithmetic behind the hash runs with a forced t through tests/probe_sp (built
on demand with the library's flags): no hash output reaches those branches."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import plonky2_ecdsa_amd as p2e
import hd_inputs as HI
import sp_inputs as SP

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tests", "probe_sp")
INV = -1
size = C.c_size_t


@pytest.fixture(scope="module")
def hctx():
    return p2e.Context(device=0, host_pointers=True)


def filled(*shape, dtype=np.uint8):
    return np.full(shape, 0xAA if dtype == np.uint8 else 0xAAAAAAAA, dtype)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def rows_of(a, n):
    """the first n rows of an input array as its own buffer; one dummy row for n = 0 (a pointer the call must not follow)"""
    return np.ascontiguousarray(a[:max(n, 1)]).copy()


def scan_call(hctx, S, n):
    """p2e_sp_scan_batch on the first n transactions of a set in host-pointer mode: (return value, n_hits, hit_output, hit_label,
    hit_tweak, err), each one element longer than the call may write"""
    mh, nl = S["max_hits"], S["n_labels"]
    out = filled(n + 1), filled(n + 1, mh, dtype=np.uint32), filled(n + 1, mh), filled(n + 1, mh, 32), filled(n + 1)
    ih = None if S["input_hash"] is None else rows_of(S["input_hash"], n)
    lx, ly = (S["label_x"].copy(), S["label_y"].copy()) if nl else (None, None)
    rc = hctx._L.p2e_sp_scan_batch(hctx._h, _p(S["scan_sk"].copy()), _p(S["spend_pkx"].copy()), _p(S["spend_pky"].copy()), _p(lx), _p(ly), size(nl),
                                   _p(rows_of(S["ax"], n)), _p(rows_of(S["ay"], n)), _p(ih), _p(S["outputs"].copy()), _p(S["out_offsets"][:n + 1].copy()),
                                   size(mh), _p(out[0]), _p(out[1]), _p(out[2]), _p(out[3]), size(n), _p(out[4]))
    return (rc,) + out


def assert_scan_equals(S, got, n):
    rc, n_hits, hit_output, hit_label, hit_tweak, err = got
    assert rc >= 0, p2e.lib().p2e_last_error()
    diff = np.nonzero((err[:n] != S["err"][:n]) | (n_hits[:n] != S["n_hits"][:n]))[0]
    assert diff.size == 0, [(int(i), int(err[i]), int(S["err"][i]), int(n_hits[i]), int(S["n_hits"][i])) for i in diff[:8]]
    assert np.array_equal(hit_output[:n], S["hit_output"][:n]) and np.array_equal(hit_label[:n], S["hit_label"][:n])
    assert np.array_equal(hit_tweak[:n], S["hit_tweak"][:n]) and rc == np.count_nonzero(S["err"][:n])
    assert n_hits[n] == 0xAA and (hit_output[n] == 0xAAAAAAAA).all() and (hit_label[n] == 0xAA).all() and (hit_tweak[n] == 0xAA).all() and err[n] == 0xAA
    flagged = S["err"][:n] != 0
    assert not n_hits[:n][flagged].any() and not hit_output[:n][flagged].any() and not hit_label[:n][flagged].any() and not hit_tweak[:n][flagged].any()


# ---- every call against the oracle ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SP.COUNTS)
def test_input_hash_equals_the_oracle(n, hctx):
    H = SP.input_hash_set()
    out, err = filled(n + 1, 32), filled(n + 1)
    bad = hctx._L.p2e_sp_input_hash_batch(hctx._h, _p(rows_of(H["outpoint"], n)), _p(rows_of(H["ax"], n)), _p(rows_of(H["ay"], n)), _p(out), size(n),
                                          _p(err))
    diff = np.nonzero((out[:n] != H["input_hash"][:n]).any(axis=1) | (err[:n] != H["err"][:n]))[0]
    assert diff.size == 0, [(int(i), int(err[i]), int(H["err"][i])) for i in diff[:8]]
    assert bad == np.count_nonzero(H["err"][:n]) and not out[:n][H["err"][:n] != 0].any() and (out[n] == 0xAA).all() and err[n] == 0xAA
    assert n < 257 or bad == 4


@pytest.mark.parametrize("n", SP.COUNTS)
def test_labels_equal_the_oracle(n, hctx):
    S = SP.label_set()
    tw, x, y, err = filled(n + 1, 32), filled(n + 1, 32), filled(n + 1, 32), filled(n + 1)
    bad = hctx._L.p2e_sp_label_batch(hctx._h, _p(S["scan_sk"].copy()), _p(rows_of(S["index"], n)), _p(tw), _p(x), _p(y), size(n), _p(err))
    assert bad == 0 and not err[:n].any() and np.array_equal(tw[:n], S["tweak"][:n]) and np.array_equal(x[:n], S["x"][:n])
    assert np.array_equal(y[:n], S["y"][:n]) and (tw[n] == 0xAA).all() and (x[n] == 0xAA).all() and (y[n] == 0xAA).all() and err[n] == 0xAA


@pytest.mark.parametrize("bad_key", [0, SP.N])
def test_a_refused_scan_key_flags_every_label(bad_key, hctx):
    S = SP.label_set(65, bad_key)
    n = 65
    tw, x, y, err = filled(n, 32), filled(n, 32), filled(n, 32), filled(n)
    bad = hctx._L.p2e_sp_label_batch(hctx._h, _p(S["scan_sk"].copy()), _p(S["index"].copy()), _p(tw), _p(x), _p(y), size(n), _p(err))
    assert bad == n and (err == SP.WIRE_SCALAR_RANGE).all() and not tw.any() and not x.any() and not y.any()


@pytest.mark.parametrize("n", SP.COUNTS)
def test_send_equals_the_oracle(n, hctx):
    K = SP.send_set()
    out, err = filled(n + 1, 32), filled(n + 1)
    bad = hctx._L.p2e_sp_send_batch(hctx._h, _p(rows_of(K["a"], n)), _p(rows_of(K["input_hash"], n)), _p(rows_of(K["scan_pkx"], n)),
                                    _p(rows_of(K["scan_pky"], n)), _p(rows_of(K["spend_pkx"], n)), _p(rows_of(K["spend_pky"], n)), _p(rows_of(K["k"], n)),
                                    _p(out), size(n), _p(err))
    diff = np.nonzero((out[:n] != K["out"][:n]).any(axis=1) | (err[:n] != K["err"][:n]))[0]
    assert diff.size == 0, [(int(i), int(err[i]), int(K["err"][i])) for i in diff[:8]]
    assert bad == np.count_nonzero(K["err"][:n]) and not out[:n][K["err"][:n] != 0].any() and (out[n] == 0xAA).all() and err[n] == 0xAA
    assert n < 63 or bad == len(SP.SEND_BAD)


@pytest.mark.parametrize("n", SP.COUNTS)
def test_scan_equals_the_oracle(n, hctx):
    S = SP.scan_set(max_hits=3, n_labels=2)
    assert_scan_equals(S, scan_call(hctx, S, n), n)
    if n >= 64:                  # three hits beside no outputs and forty decoys in the first wave: its k loops diverge
        offs = S["out_offsets"]
        assert S["n_hits"][:3].tolist() == [3, 0, 0] and [int(offs[i + 1] - offs[i]) for i in range(3)] == [5, 0, 40]
        assert set(S["err"][:n].tolist()) >= {SP.WIRE_BAD_LENGTH, SP.WIRE_COORD_RANGE, SP.WIRE_NOT_ON_CURVE, SP.WIRE_INFINITY, SP.WIRE_SCALAR_RANGE} or n < 257


@pytest.mark.parametrize("max_hits", [1, 2, 8])
def test_scan_at_every_cap_with_the_saturating_transaction(max_hits, hctx):
    S = SP.scan_set(max_hits=max_hits, n_labels=1)
    n = 65
    assert (S["n_hits"][:n] == max_hits).any() and len(SP.transactions()[14]["planted"]) == 9
    assert_scan_equals(S, scan_call(hctx, S, n), n)


@pytest.mark.parametrize("n_labels", [0, 1, 16])
def test_scan_with_no_one_and_sixteen_labels(n_labels, hctx):
    S = SP.scan_set(max_hits=2, n_labels=n_labels)
    n = 65
    assert_scan_equals(S, scan_call(hctx, S, n), n)
    assert (S["hit_label"][:n] != 0).any() == (n_labels != 0)


def test_scan_without_an_input_hash_takes_tweak_data(hctx):
    S = SP.scan_set(max_hits=8, n_labels=16, with_hash=False)
    n = 65
    assert S["input_hash"] is None and (S["n_hits"][:n] == 8).any() and (S["hit_label"][:n] == 16).any()
    assert_scan_equals(S, scan_call(hctx, S, n), n)


@pytest.mark.parametrize("bad", sorted(SP.SHARED_BAD))
def test_a_refused_shared_argument_flags_every_transaction(bad, hctx):
    n_labels = 16 if bad.startswith("label_off") else 2
    S = SP.scan_set(2, n_labels, True, 65, False, bad)
    got = scan_call(hctx, S, 65)
    assert got[0] == 65 and (got[5][:65] == SP.SHARED_BAD[bad]).all()
    assert_scan_equals(S, got, 65)


# ---- refusals, the Python methods -------------------------------------------------------------------------------------------------
def test_refused_arguments(hctx):
    L, h = hctx._L, hctx._h
    bufs = [np.zeros(512, np.uint8) for _ in range(16)]
    p = [_p(b) for b in bufs]
    one, zero, two = size(1), size(0), size(2)
    offsets = np.array([0, 1], np.uint64)

    def scan(args, n_labels=zero, max_hits=one, count=one, offs=offsets):
        a = list(args)
        return L.p2e_sp_scan_batch(h, a[0], a[1], a[2], a[3], a[4], n_labels, a[5], a[6], a[7], a[8], _p(offs), max_hits, a[9], a[10], a[11], a[12],
                                   count, a[13])
    full = p[:14]
    # accepted with every pointer given (everything is zero: one flag each), refused with any required pointer null
    assert L.p2e_sp_input_hash_batch(h, p[0], p[1], p[2], p[3], one, p[4]) == 1
    for k in range(5):
        a = p[:5]
        a[k] = None
        assert L.p2e_sp_input_hash_batch(h, a[0], a[1], a[2], a[3], one, a[4]) == INV
    assert L.p2e_sp_label_batch(h, p[0], p[1], p[2], p[3], p[4], one, p[5]) == 1
    for k in range(6):
        a = p[:6]
        a[k] = None
        assert L.p2e_sp_label_batch(h, a[0], a[1], a[2], a[3], a[4], one, a[5]) == INV
    for buf in bufs:
        buf[:] = 0
    assert L.p2e_sp_send_batch(h, p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], one, p[8]) == 1
    for k in range(9):
        a = p[:9]
        a[k] = None
        assert L.p2e_sp_send_batch(h, a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], one, a[8]) == INV
    for buf in bufs:
        buf[:] = 0
    assert scan(full, n_labels=one) == 1
    for k in range(14):
        a = list(full)
        a[k] = None
        want = 1 if k == 7 else INV                       # input_hash32 alone is nullable
        assert scan(a, n_labels=one) == want, k
        assert want == 1 or "null pointer" in L.p2e_last_error().decode()
    a = list(full)
    a[3] = a[4] = None
    assert scan(a) == 1                                   # n_labels == 0: no label pointers
    # the limits
    for kw in (dict(max_hits=zero), dict(max_hits=size(9)), dict(n_labels=size(17))):
        assert scan(full, **kw) == INV and "max_hits" in L.p2e_last_error().decode()
    assert scan(full, max_hits=size(8), n_labels=size(16)) == 1
    # host staging reads the offsets: reversed ends, and an offset outside [out_offsets[0], out_offsets[count]]
    assert scan(full, offs=np.array([5, 3], np.uint64)) == INV
    assert scan(full, count=two, offs=np.array([1, 9, 2], np.uint64)) == INV and "out_offsets" in L.p2e_last_error().decode()
    # count == 0 returns 0
    assert L.p2e_sp_input_hash_batch(h, p[0], p[1], p[2], p[3], zero, p[4]) == 0
    assert L.p2e_sp_label_batch(h, p[0], p[1], p[2], p[3], p[4], zero, p[5]) == 0
    assert L.p2e_sp_send_batch(h, p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], zero, p[8]) == 0
    assert scan(full, count=zero) == 0
    # an overlap is refused on a live context too, and the context stays usable
    a = list(full)
    a[12] = a[5]                                          # hit_tweak32 on ax32: the scan has no in-place form
    assert scan(a) == INV and "overlap" in L.p2e_last_error().decode()
    a = list(full)
    a[12] = a[8]                                          # hit_tweak32 on the staged outputs
    assert scan(a) == INV and "overlap" in L.p2e_last_error().decode()
    assert scan(full) == 1


def test_python_methods_give_the_same_bytes(hctx):
    H, Lb, K, S = SP.input_hash_set(), SP.label_set(), SP.send_set(), SP.scan_set(max_hits=3, n_labels=2)
    ih, err, bad = hctx.sp_input_hash_batch(H["outpoint"].copy(), H["ax"].copy(), H["ay"].copy())
    assert np.array_equal(ih, H["input_hash"]) and np.array_equal(err, H["err"]) and bad == 4
    tw, x, y, err, bad = hctx.sp_label_batch(Lb["scan_sk"].copy(), Lb["index"].copy())
    assert np.array_equal(tw, Lb["tweak"]) and np.array_equal(x, Lb["x"]) and np.array_equal(y, Lb["y"]) and bad == 0
    out, err, bad = hctx.sp_send_batch(K["a"].copy(), K["input_hash"].copy(), K["scan_pkx"].copy(), K["scan_pky"].copy(), K["spend_pkx"].copy(),
                                       K["spend_pky"].copy(), K["k"].copy())
    assert np.array_equal(out, K["out"]) and np.array_equal(err, K["err"])
    n_hits, hit_output, hit_label, hit_tweak, err, bad = hctx.sp_scan_batch(
        S["scan_sk"].copy(), S["spend_pkx"].copy(), S["spend_pky"].copy(), S["ax"].copy(), S["ay"].copy(), S["outputs"].copy(), S["out_offsets"].copy(),
        input_hash=S["input_hash"].copy(), label_x=S["label_x"].copy(), label_y=S["label_y"].copy(), max_hits=3)
    assert np.array_equal(n_hits, S["n_hits"]) and np.array_equal(hit_output, S["hit_output"]) and np.array_equal(hit_label, S["hit_label"])
    assert np.array_equal(hit_tweak, S["hit_tweak"]) and np.array_equal(err, S["err"]) and bad == np.count_nonzero(S["err"])
    with pytest.raises(p2e.P2EError):
        hctx.sp_scan_batch(S["scan_sk"].copy(), S["spend_pkx"].copy(), S["spend_pky"].copy(), S["ax"].copy(), S["ay"].copy(), S["outputs"].copy(),
                           S["out_offsets"].copy(), max_hits=9)


# ---- device pointers ----------------------------------------------------------------------------------------------------------------
def test_send_then_scan_stays_on_the_device():
    """Input hashes -> the sender's output keys -> the receiver's scan, on device pointers in async mode: the keys p2e_sp_send_batch
    writes are the outputs p2e_sp_scan_batch reads (transaction i has the one output i), nothing visits the host in between.
    Every transaction is a hit at k = 0; every second one under label i % 16."""
    n = 65
    ctx = p2e.Context(device=0, asynchronous=True)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    full = lambda *shape: torch.full(shape, 0xAA, dtype=torch.uint8, device="cuda:0")
    H, K, S = SP.input_hash_set(), SP.send_set(), SP.scan_set(max_hits=2, n_labels=16)
    good = [i for i in range(SP.N_SET) if K["err"][i] == 0 and H["err"][i] == 0 and i not in SP.SEND_K_EDGES and K["k"][i] == 0][:n]
    assert len(good) == n
    txs = SP.transactions()
    ax, ay, outpoint = dev(H["ax"][good]), dev(H["ay"][good]), dev(H["outpoint"][good])
    ih, e1, _ = ctx.sp_input_hash_batch(outpoint, ax, ay, input_hash=full(n, 32), err=full(n))
    out_pk, e2, _ = ctx.sp_send_batch(dev(K["a"][good]), ih, dev(K["scan_pkx"][good]), dev(K["scan_pky"][good]), dev(K["spend_pkx"][good]),
                                      dev(K["spend_pky"][good]), dev(K["k"][good].view(np.int32)), out_pk=full(n, 32), err=full(n))
    offsets = dev(np.arange(n + 1, dtype=np.int64))
    n_hits, hit_output, hit_label, hit_tweak, e3, _ = ctx.sp_scan_batch(
        dev(S["scan_sk"]), dev(S["spend_pkx"]), dev(S["spend_pky"]), ax, ay, out_pk, offsets, input_hash=ih, label_x=dev(S["label_x"]),
        label_y=dev(S["label_y"]), max_hits=2, n_hits=full(n), hit_output=torch.full((n, 2), -1, dtype=torch.int32, device="cuda:0"),
        hit_label=full(n, 2), hit_tweak=full(n, 2, 32), err=full(n))
    assert ctx.sync() == 0
    torch.cuda.synchronize()
    for e in (e1, e2, e3):
        assert not e.cpu().numpy().any()
    assert np.array_equal(ih.cpu().numpy(), H["input_hash"][good]) and np.array_equal(out_pk.cpu().numpy(), K["out"][good])
    assert (n_hits.cpu().numpy() == 1).all() and not hit_output.cpu().numpy().any()
    labels = hit_label.cpu().numpy()
    assert labels[:, 0].tolist() == [0 if i % 2 else i % 16 + 1 for i in good] and not labels[:, 1].any()
    tweaks = hit_tweak.cpu().numpy()
    assert all(tweaks[j, 0].tobytes() == SP.b32(SP.tweak(txs[i]["S_send"], 0)) for j, i in enumerate(good)) and not tweaks[:, 1].any()
    ctx.close()


def test_host_and_device_pointer_paths_give_the_same_bytes():
    """The scan once per kind of context on the same input bytes, from transaction 36 on (out_offsets[0] is far from 0, the
    reversed pair among the elements): equal return values, equal outputs; on the host side every output lies in one arena with
    64 guard bytes behind it and no guard byte changes."""
    n, first, GUARD, PATTERN, mh = 9, 36, 64, 0x5C, 3
    S = SP.scan_set(max_hits=mh, n_labels=2)
    assert S["err"][first:first + n].tolist().count(SP.WIRE_BAD_LENGTH) == 1 and S["n_hits"][first:first + n].any() and int(S["out_offsets"][first]) > 100
    inputs = [S["scan_sk"], S["spend_pkx"], S["spend_pky"], S["label_x"], S["label_y"], S["ax"][first:first + n], S["ay"][first:first + n],
              S["input_hash"][first:first + n], S["outputs"], S["out_offsets"][first:first + n + 1]]
    widths = [1, 4 * mh, mh, 32 * mh, 1]                    # n_hits, hit_output, hit_label, hit_tweak32, err
    results = {}
    for mode in ("device", "host"):
        ctx = p2e.Context(device=0, host_pointers=(mode == "host"))
        ins = [np.ascontiguousarray(a).copy() for a in inputs]
        if mode == "device":
            held = [torch.from_numpy(a.view(np.uint8).reshape(-1)).cuda() for a in ins]
            outs = [torch.full((w * n,), 0xAA, dtype=torch.uint8, device="cuda") for w in widths]
        else:
            held = ins
            arena = np.full(sum(w * n + GUARD for w in widths) + GUARD, PATTERN, np.uint8)
            outs, at = [], GUARD
            for w in widths:
                outs.append(arena[at:at + w * n])
                outs[-1][:] = 0xAA
                at += w * n + GUARD
        ptr, optr = [p2e._ptr(a) for a in held], [p2e._ptr(o) for o in outs]
        rc = ctx._L.p2e_sp_scan_batch(ctx._h, ptr[0], ptr[1], ptr[2], ptr[3], ptr[4], size(2), ptr[5], ptr[6], ptr[7], ptr[8], ptr[9], size(mh),
                                      optr[0], optr[1], optr[2], optr[3], size(n), optr[4])
        assert rc >= 0, (mode, ctx._L.p2e_last_error())
        if mode == "device":
            torch.cuda.synchronize()
            got = [o.cpu().numpy().copy() for o in outs]
        else:
            got = [o.copy() for o in outs]
            mask = np.ones(arena.size, bool)
            at = GUARD
            for w in widths:
                mask[at:at + w * n] = False
                at += w * n + GUARD
            assert (arena[mask] == PATTERN).all()
            assert all(np.array_equal(a, np.ascontiguousarray(b)) for a, b in zip(ins, inputs))
        results[mode] = (rc, got)
        ctx.close()
    assert results["device"][0] == results["host"][0] == np.count_nonzero(S["err"][first:first + n])
    assert all(np.array_equal(a, b) for a, b in zip(results["device"][1], results["host"][1]))
    want = [S["n_hits"][first:first + n], S["hit_output"][first:first + n], S["hit_label"][first:first + n], S["hit_tweak"][first:first + n],
            S["err"][first:first + n]]
    assert all(np.array_equal(g, np.ascontiguousarray(w).view(np.uint8).reshape(-1)) for g, w in zip(results["host"][1], want))


# ---- behind the hash, on the device ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe():
    lib = os.path.join(PROBE, "libp2e_probe_sp.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-s", "-C", PROBE, "libp2e_probe_sp.so"])
    L = C.CDLL(lib)
    L.probesp_finish.restype = C.c_long
    return L


def test_forced_tweaks_on_the_device(probe):
    """t >= n and t = 0 refused, the doubling t G = B_spend computed, t G = -B_spend flagged, a neutral P_k + L_j passed over,
    L_j = P_k doubled.  65 elements: the table repeated, so that lanes of one wave take different branches."""
    table = SP.forced_finish()
    rows = tuple(table[i % len(table)] for i in range(65))
    F = SP.forced_arrays(rows)
    n = len(rows)
    code, found, out, lab = filled(n), filled(n), filled(n, dtype=np.uint32), filled(n)
    assert probe.probesp_finish(_p(F["bx"]), _p(F["by"]), _p(F["lx"]), _p(F["ly"]), size(SP.FORCED_LABELS), _p(F["t"]), _p(F["outputs"]),
                                size(SP.FORCED_OUTPUTS), _p(code), _p(found), _p(out), _p(lab), size(n)) == 0
    assert code.tolist() == F["code"].tolist(), [(i, int(g), int(w)) for i, (g, w) in enumerate(zip(code, F["code"])) if g != w][:8]
    assert found.tolist() == F["found"].tolist() and out.tolist() == F["hit_output"].tolist() and lab.tolist() == F["hit_label"].tolist()
    assert {SP.WIRE_OK, SP.WIRE_SCALAR_RANGE, SP.WIRE_INFINITY} == set(code.tolist())


def test_c_example_makes_a_payment_and_finds_it_again(tmp_path):
    """examples/sp_scan.c: 300 transactions, the receiver's keys from test vector 1's m/0', one payment in transaction 150"""
    exe = str(tmp_path / "sp_scan")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "sp_scan.c"), "-L", os.path.join(ROOT, "plonky2-ecdsa_amd"), "-lp2e_hip",
                           "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe])
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "plonky2-ecdsa_amd") + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    r = subprocess.run([exe, "300"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    # the same payment from the oracle: the receiver's keys are m/0'/0' and m/0'/1', the sender's input key is 151 + 2^64
    c0, b_scan, _ = HI.ckd_priv(HI.TV1_M_0H[0], HI.TV1_M_0H[1], HI.HARDENED)
    c1, b_spend, _ = HI.ckd_priv(HI.TV1_M_0H[0], HI.TV1_M_0H[1], HI.HARDENED + 1)
    a = 151 + 2**64
    outpoint = b"\x42" * 32 + (151).to_bytes(4, "little")
    code, ih = SP.input_hash(outpoint, SP.base_mul(a))
    code2, want = SP.send(a, int.from_bytes(ih, "big"), SP.base_mul(b_scan), SP.base_mul(b_spend), 0)
    assert (c0, c1, code, code2) == (0, 0, 0, 0)
    assert f"300 transactions scanned (0 refused): 1 payment found in transaction 150, output 1, key {want.hex()}" in r.stdout
