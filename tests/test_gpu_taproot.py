"""Taproot on the GPU (include/p2e.h p2e_taproot_leaf_hash_batch, p2e_taproot_merkle_root_batch, p2e_taproot_tweak_pubkey_batch,
p2e_taproot_tweak_seckey_batch, p2e_taproot_verify_commitment_batch) through the C ABI.

Expectations come from tests/taproot_inputs.py alone: a restatement of BIP-341 in Python integers and hashlib.  Every byte of
every element is compared; output buffers are pre-filled with 0xAA so that an unwritten byte shows, and hold one element
more than the call may write.

Shapes: every call at count = 0, 1, 63, 64, 65 and 257 (nothing, one lane, a wave less one, a wave, a wave plus one, a block
plus one); the full script set (every edge length at every alignment, the 0x10000-byte scripts included) once; depth 128
beside depth 0 in the first wave.  The arithmetic behind the hash runs with a forced t through tests/probe_taproot (built on
demand with the library's flags): no hash output reaches those branches."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import plonky2_ecdsa_amd as p2e
import hd_inputs as HI
import taproot_inputs as TI

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tests", "probe_taproot")
INV = -1


@pytest.fixture(scope="module")
def hctx():
    return p2e.Context(device=0, host_pointers=True)


def filled(*shape):
    return np.full(shape, 0xAA, np.uint8)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def rows_of(a, n):
    """the first n rows of an input array as its own buffer; one dummy row for n = 0 (a pointer the call must not follow)"""
    return np.ascontiguousarray(a[:max(n, 1)]).copy()


def flagged_are_zero(err, *outs):
    return all(not o[err != 0].any() for o in outs)


# ---- every call against the oracle ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", TI.COUNTS)
def test_leaf_hash_equals_the_oracle(n, hctx):
    S = TI.script_set(TI.SMALL_SCRIPT_LENGTHS)
    leaf, err = filled(n + 1, 32), filled(n + 1)
    bad = hctx._L.p2e_taproot_leaf_hash_batch(hctx._h, _p(rows_of(S["version"], n)), _p(S["data"].copy()), _p(S["offsets"][:n + 1].copy()),
                                              _p(leaf), C.c_size_t(n), _p(err))
    diff = np.nonzero((leaf[:n] != S["leaf"][:n]).any(axis=1) | (err[:n] != S["err"][:n]))[0]
    assert diff.size == 0, [(int(i), int(S["offsets"][i]) % 4, int(S["offsets"][i + 1]) - int(S["offsets"][i]), int(err[i])) for i in diff[:8]]
    assert bad == np.count_nonzero(S["err"][:n]) and flagged_are_zero(S["err"][:n], leaf[:n]) and (leaf[n] == 0xAA).all() and err[n] == 0xAA
    assert n < 64 or bad == 2


def test_leaf_hash_on_every_edge_length_and_alignment(hctx):
    """the whole script set on the device: 0 .. 0x10000 bytes at all four alignments; the prefix grows from 2 to 4 to 6 bytes"""
    S = TI.script_set()
    n = len(S["version"])
    leaf, err = filled(n + 1, 32), filled(n + 1)
    bad = hctx._L.p2e_taproot_leaf_hash_batch(hctx._h, _p(S["version"].copy()), _p(S["data"].copy()), _p(S["offsets"].copy()), _p(leaf),
                                              C.c_size_t(n), _p(err))
    diff = np.nonzero((leaf[:n] != S["leaf"]).any(axis=1) | (err[:n] != S["err"]))[0]
    assert diff.size == 0, [(int(i), int(S["offsets"][i]) % 4, int(S["offsets"][i + 1]) - int(S["offsets"][i]), int(err[i])) for i in diff[:8]]
    assert bad == 2 and (leaf[n] == 0xAA).all() and err[n] == 0xAA
    # device pointers: the sentinel bytes in front of and behind the scripts are on the device too, and nothing but the
    # scripts' own words is read (a lane that used a byte of them would give another hash)
    ctx = p2e.Context(device=0)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    offs = dev(S["offsets"].view(np.int64))
    got, gerr, gbad = ctx.taproot_leaf_hash_batch(dev(S["version"]), dev(S["data"]), offs)
    assert gbad == 2 and np.array_equal(got.cpu().numpy(), S["leaf"]) and np.array_equal(gerr.cpu().numpy(), S["err"])
    ctx.close()


@pytest.mark.parametrize("max_depth", [0, 1, 128])
@pytest.mark.parametrize("n", TI.COUNTS)
def test_merkle_root_equals_the_oracle(n, max_depth, hctx):
    M = TI.path_set(257, max_depth)
    root, err = filled(n + 1, 32), filled(n + 1)
    path = rows_of(M["path"], n) if max_depth else None
    bad = hctx._L.p2e_taproot_merkle_root_batch(hctx._h, _p(rows_of(M["leaf"], n)), _p(path), _p(rows_of(M["depth"], n)), C.c_size_t(max_depth),
                                                _p(root), C.c_size_t(n), _p(err))
    diff = np.nonzero((root[:n] != M["root"][:n]).any(axis=1) | (err[:n] != M["err"][:n]))[0]
    assert diff.size == 0, [(int(i), int(M["depth"][i]), int(err[i])) for i in diff[:8]]
    assert bad == np.count_nonzero(M["err"][:n]) and flagged_are_zero(M["err"][:n], root[:n]) and (root[n] == 0xAA).all() and err[n] == 0xAA
    if max_depth == 128 and n >= 64:                     # depth 128 beside depth 0 in one wave
        assert (M["depth"][:64] == 128).any() and (M["depth"][:64] == 0).any() and bad > 0


@pytest.mark.parametrize("form", ["with_root", "no_root"])
@pytest.mark.parametrize("n", TI.COUNTS)
def test_tweak_pubkey_equals_the_oracle(n, form, hctx):
    K = TI.pubkey_set()
    want = K[form]
    out, par, err = filled(n + 1, 32), filled(n + 1), filled(n + 1)
    root = rows_of(K["root"], n) if form == "with_root" else None
    bad = hctx._L.p2e_taproot_tweak_pubkey_batch(hctx._h, _p(rows_of(K["pk"], n)), _p(root), _p(out), _p(par), C.c_size_t(n), _p(err))
    diff = np.nonzero((out[:n] != want["out"][:n]).any(axis=1) | (par[:n] != want["parity"][:n]) | (err[:n] != want["err"][:n]))[0]
    assert diff.size == 0, [(int(i), int(err[i]), int(want["err"][i])) for i in diff[:8]]
    assert bad == np.count_nonzero(want["err"][:n]) and flagged_are_zero(want["err"][:n], out[:n], par[:n])
    assert (out[n] == 0xAA).all() and par[n] == 0xAA and err[n] == 0xAA
    if n > 5:                                            # the three pins are elements 3, 4, 5 (pin 1 under no root)
        pins = [(3, TI.PINS[0])] if form == "no_root" else [(4, TI.PINS[1]), (5, TI.PINS[2])]
        for i, pin in pins:
            assert (out[i].tobytes().hex(), par[i], err[i]) == (pin["output"], pin["parity"], 0)


@pytest.mark.parametrize("form", ["with_root", "no_root"])
@pytest.mark.parametrize("n", TI.COUNTS)
def test_tweak_seckey_equals_the_oracle(n, form, hctx):
    D = TI.seckey_set()
    want = D[form]
    out, err = filled(n + 1, 32), filled(n + 1)
    root = rows_of(D["root"], n) if form == "with_root" else None
    bad = hctx._L.p2e_taproot_tweak_seckey_batch(hctx._h, _p(rows_of(D["sk"], n)), _p(root), _p(out), C.c_size_t(n), _p(err))
    diff = np.nonzero((out[:n] != want["out"][:n]).any(axis=1) | (err[:n] != want["err"][:n]))[0]
    assert diff.size == 0, [(int(i), int(err[i]), int(want["err"][i])) for i in diff[:8]]
    assert bad == np.count_nonzero(want["err"][:n]) and flagged_are_zero(want["err"][:n], out[:n]) and (out[n] == 0xAA).all() and err[n] == 0xAA


@pytest.mark.parametrize("n", TI.COUNTS)
def test_verify_commitment_equals_the_oracle(n, hctx):
    S = TI.commitment_set()
    err, valid = filled(n + 1), filled(n + 1)
    bad = hctx._L.p2e_taproot_verify_commitment_batch(hctx._h, _p(rows_of(S["out_pk"], n)), _p(rows_of(S["out_parity"], n)), _p(rows_of(S["pk"], n)),
                                                      _p(rows_of(S["leaf"], n)), _p(rows_of(S["path"], n)), _p(rows_of(S["depth"], n)),
                                                      C.c_size_t(S["max_depth"]), C.c_size_t(n), _p(err), _p(valid))
    diff = np.nonzero((err[:n] != S["err"][:n]) | (valid[:n] != S["valid"][:n]))[0]
    assert diff.size == 0, [(int(i), int(err[i]), int(S["err"][i]), int(valid[i]), int(S["valid"][i])) for i in diff[:8]]
    assert bad == np.count_nonzero(S["err"][:n]) and flagged_are_zero(S["err"][:n], valid[:n]) and err[n] == 0xAA and valid[n] == 0xAA
    if n > 5:                                            # both leaves of pin 3 and the one leaf of pin 2
        assert valid[1] == valid[2] == valid[4] == 1


@pytest.mark.parametrize("max_depth", [0, 1, 128])
def test_verify_commitment_at_the_depth_limits(max_depth, hctx):
    S = TI.commitment_set(65, max_depth)
    n = 65
    err, valid = filled(n + 1), filled(n + 1)
    path = np.ascontiguousarray(S["path"]) if max_depth else None
    bad = hctx._L.p2e_taproot_verify_commitment_batch(hctx._h, _p(S["out_pk"]), _p(S["out_parity"]), _p(S["pk"]), _p(S["leaf"]), _p(path),
                                                      _p(S["depth"]), C.c_size_t(max_depth), C.c_size_t(n), _p(err), _p(valid))
    assert np.array_equal(err[:n], S["err"]) and np.array_equal(valid[:n], S["valid"]) and bad == np.count_nonzero(S["err"])
    assert err[n] == 0xAA and valid[n] == 0xAA and valid[:n].sum() > 10


# ---- in place, refusals, the Python methods --------------------------------------------------------------------------------------
def test_the_three_in_place_forms_equal_the_oracle(hctx):
    n = 257
    K, D, M = TI.pubkey_set(), TI.seckey_set(), TI.path_set(257, 128)
    pk, par, err = K["pk"].copy(), filled(n), filled(n)
    assert hctx._L.p2e_taproot_tweak_pubkey_batch(hctx._h, _p(pk), _p(K["root"].copy()), _p(pk), _p(par), C.c_size_t(n), _p(err)) == 5
    assert np.array_equal(pk, K["with_root"]["out"]) and np.array_equal(par, K["with_root"]["parity"]) and np.array_equal(err, K["with_root"]["err"])
    sk, err = D["sk"].copy(), filled(n)
    assert hctx._L.p2e_taproot_tweak_seckey_batch(hctx._h, _p(sk), None, _p(sk), C.c_size_t(n), _p(err)) == 3
    assert np.array_equal(sk, D["no_root"]["out"]) and np.array_equal(err, D["no_root"]["err"])
    leaf, err = M["leaf"].copy(), filled(n)
    bad = hctx._L.p2e_taproot_merkle_root_batch(hctx._h, _p(leaf), _p(np.ascontiguousarray(M["path"])), _p(M["depth"].copy()), C.c_size_t(128),
                                                _p(leaf), C.c_size_t(n), _p(err))
    assert bad == np.count_nonzero(M["err"]) and np.array_equal(leaf, M["root"]) and np.array_equal(err, M["err"])
    # device pointers, where in place IS in place (no staging copy in between)
    ctx = p2e.Context(device=0)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    pk = dev(K["pk"])
    ctx.taproot_tweak_pubkey_batch(pk, dev(K["root"]), out_pk=pk)
    sk = dev(D["sk"])
    ctx.taproot_tweak_seckey_batch(sk, None, out_sk=sk)
    leaf = dev(M["leaf"])
    ctx.taproot_merkle_root_batch(leaf, dev(M["path"]), dev(M["depth"]), root=leaf)
    assert np.array_equal(pk.cpu().numpy(), K["with_root"]["out"]) and np.array_equal(sk.cpu().numpy(), D["no_root"]["out"])
    assert np.array_equal(leaf.cpu().numpy(), M["root"])
    ctx.close()


def test_refused_arguments(hctx):
    L, h = hctx._L, hctx._h
    mk = lambda: np.zeros(512, np.uint8)
    one, zero, d1, d129 = C.c_size_t(1), C.c_size_t(0), C.c_size_t(1), C.c_size_t(129)
    offsets = np.array([0, 3], np.uint64)
    bufs = [mk() for _ in range(10)]
    p = [_p(b) for b in bufs]

    def clear():                                          # (an output of one call is an input of the next: zeros again)
        for buf in bufs:
            buf[:] = 0
    # accepted with every pointer given (outputs pairwise disjoint), refused with any required pointer null
    assert L.p2e_taproot_leaf_hash_batch(h, p[0], p[1], _p(offsets), p[2], one, p[3]) == 0
    for k in range(5):
        a = [p[0], p[1], _p(offsets), p[2], p[3]]
        a[k] = None
        assert L.p2e_taproot_leaf_hash_batch(h, a[0], a[1], a[2], a[3], one, a[4]) == INV
    clear()
    assert L.p2e_taproot_merkle_root_batch(h, p[0], p[1], p[2], d1, p[3], one, p[4]) == 0
    for k in range(5):
        a = [p[0], p[1], p[2], p[3], p[4]]
        a[k] = None
        assert L.p2e_taproot_merkle_root_batch(h, a[0], a[1], a[2], d1, a[3], one, a[4]) == INV
    clear()
    assert L.p2e_taproot_merkle_root_batch(h, p[0], None, p[2], zero, p[3], one, p[4]) == 0           # max_depth 0: no path
    assert L.p2e_taproot_merkle_root_batch(h, p[0], p[1], p[2], d129, p[3], one, p[4]) == INV
    assert "max_depth" in L.p2e_last_error().decode()
    clear()
    for k in range(5):
        a = [p[0], p[1], p[2], p[3], p[4]]
        a[k] = None
        want = 1 if k == 1 else INV                       # root32 alone is nullable (x = 0 is on no curve point: one flag)
        assert L.p2e_taproot_tweak_pubkey_batch(h, a[0], a[1], a[2], a[3], one, a[4]) == want
    clear()
    for k in range(4):
        a = [p[0], p[1], p[2], p[3]]
        a[k] = None
        assert L.p2e_taproot_tweak_seckey_batch(h, a[0], a[1], a[2], one, a[3]) == (1 if k == 1 else INV)
    clear()
    for k in range(8):
        a = list(p[:8])
        a[k] = None
        assert L.p2e_taproot_verify_commitment_batch(h, a[0], a[1], a[2], a[3], a[4], a[5], d1, one, a[6], a[7]) == INV
    clear()
    assert L.p2e_taproot_verify_commitment_batch(h, p[0], p[1], p[2], p[3], None, p[5], zero, one, p[6], p[7]) == 1
    assert L.p2e_taproot_verify_commitment_batch(h, p[0], p[1], p[2], p[3], p[4], p[5], d129, one, p[6], p[7]) == INV
    assert L.p2e_taproot_leaf_hash_batch(h, p[0], p[1], _p(np.array([5, 3], np.uint64)), p[2], one, p[3]) == INV   # host staging: offsets[n] < offsets[0]
    # count == 0 returns 0
    assert L.p2e_taproot_leaf_hash_batch(h, p[0], p[1], _p(offsets), p[2], zero, p[3]) == 0
    assert L.p2e_taproot_merkle_root_batch(h, p[0], p[1], p[2], d1, p[3], zero, p[4]) == 0
    assert L.p2e_taproot_tweak_pubkey_batch(h, p[0], None, p[2], p[3], zero, p[4]) == 0
    assert L.p2e_taproot_tweak_seckey_batch(h, p[0], None, p[2], zero, p[3]) == 0
    assert L.p2e_taproot_verify_commitment_batch(h, p[0], p[1], p[2], p[3], p[4], p[5], d1, zero, p[6], p[7]) == 0
    # an overlap is refused on a live context too, and the context stays usable
    assert L.p2e_taproot_tweak_pubkey_batch(h, p[0], None, _p(bufs[0][32:]), p[3], C.c_size_t(2), p[4]) == INV
    assert "overlap" in L.p2e_last_error().decode()
    assert L.p2e_taproot_tweak_seckey_batch(h, p[0], None, p[2], zero, p[3]) == 0


def test_python_methods_give_the_same_bytes(hctx):
    S, M, K, D, V = TI.script_set(TI.SMALL_SCRIPT_LENGTHS), TI.path_set(257, 1), TI.pubkey_set(), TI.seckey_set(), TI.commitment_set()
    leaf, err, bad = hctx.taproot_leaf_hash_batch(S["version"].copy(), S["data"].copy(), S["offsets"].copy())
    assert np.array_equal(leaf, S["leaf"]) and np.array_equal(err, S["err"]) and bad == 2
    root, err, bad = hctx.taproot_merkle_root_batch(M["leaf"].copy(), M["path"].copy(), M["depth"].copy())
    assert np.array_equal(root, M["root"]) and np.array_equal(err, M["err"])
    out, par, err, bad = hctx.taproot_tweak_pubkey_batch(K["pk"].copy())
    assert np.array_equal(out, K["no_root"]["out"]) and np.array_equal(par, K["no_root"]["parity"]) and bad == 5
    out, err, bad = hctx.taproot_tweak_seckey_batch(D["sk"].copy(), D["root"].copy())
    assert np.array_equal(out, D["with_root"]["out"]) and bad == 3
    err, valid, bad = hctx.taproot_verify_commitment_batch(V["out_pk"].copy(), V["out_parity"].copy(), V["pk"].copy(), V["leaf"].copy(),
                                                           V["path"].copy(), V["depth"].copy())
    assert np.array_equal(err, V["err"]) and np.array_equal(valid, V["valid"]) and bad == np.count_nonzero(V["err"])
    with pytest.raises(p2e.P2EError):
        hctx.taproot_merkle_root_batch(M["leaf"].copy(), M["path"][:5].copy(), M["depth"].copy())


# ---- host pointers against device pointers (tests/test_gpu_staging.py's method) ---------------------------------------------------
def test_host_and_device_pointer_paths_give_the_same_bytes():
    """Each call once per kind of context on the same input bytes at count = 5: equal return values, equal outputs; on the
    host side every output lies in one arena with 64 guard bytes behind it and no guard byte changes."""
    n, GUARD, PATTERN = 5, 64, 0x5C
    S, M, K, D, V = TI.script_set(TI.SMALL_SCRIPT_LENGTHS), TI.path_set(257, 128), TI.pubkey_set(), TI.seckey_set(), TI.commitment_set()
    first = 17                                            # scripts 17 .. 21: offsets[0] is far from 0; the odd version and the reversed pair among them
    assert np.count_nonzero(S["err"][first:first + n]) == 2
    size = C.c_size_t
    calls = [
        ("p2e_taproot_leaf_hash_batch", [S["version"][first:first + n], S["data"], S["offsets"][first:first + n + 1]], [], [32, 1], 0),
        ("p2e_taproot_merkle_root_batch", [M["leaf"][:n], M["path"][:n], M["depth"][:n]], [size(128)], [32, 1], 0),
        ("p2e_taproot_tweak_pubkey_batch", [K["pk"][8:8 + n], K["root"][8:8 + n]], [], [32, 1, 1], 0),
        ("p2e_taproot_tweak_seckey_batch", [D["sk"][:n], D["root"][:n]], [], [32, 1], 0),
        ("p2e_taproot_verify_commitment_batch", [V["out_pk"][6:6 + n], V["out_parity"][6:6 + n], V["pk"][6:6 + n], V["leaf"][6:6 + n],
                                                 V["path"][6:6 + n], V["depth"][6:6 + n]], [size(V["max_depth"])], [1, 1], 1),
    ]
    ctxs = {"device": p2e.Context(device=0), "host": p2e.Context(device=0, host_pointers=True)}
    flagged = 0
    for name, inputs, middle, out_widths, count_first in calls:
        results = {}
        for mode, ctx in ctxs.items():
            ins = [np.ascontiguousarray(a).copy() for a in inputs]
            if mode == "device":
                held = [torch.from_numpy(a.view(np.uint8).reshape(-1)).cuda() for a in ins]
                outs = [torch.full((w * n,), 0xAA, dtype=torch.uint8, device="cuda") for w in out_widths]
                arena = None
            else:
                held = ins
                arena = np.full(sum(w * n + GUARD for w in out_widths) + GUARD, PATTERN, np.uint8)
                outs, at = [], GUARD
                for w in out_widths:
                    outs.append(arena[at:at + w * n])
                    outs[-1][:] = 0xAA
                    at += w * n + GUARD
            ptr = [p2e._ptr(a) for a in held]
            optr = [p2e._ptr(o) for o in outs]
            # the header's order: inputs, (max_depth), then outputs around count
            if name == "p2e_taproot_leaf_hash_batch":
                args = ptr + [optr[0], size(n), optr[1]]
            elif name == "p2e_taproot_merkle_root_batch":
                args = ptr + middle + [optr[0], size(n), optr[1]]
            elif name == "p2e_taproot_tweak_pubkey_batch":
                args = ptr + [optr[0], optr[1], size(n), optr[2]]
            elif name == "p2e_taproot_tweak_seckey_batch":
                args = ptr + [optr[0], size(n), optr[1]]
            else:
                args = ptr + middle + [size(n)] + optr
            rc = getattr(ctx._L, name)(ctx._h, *args)
            assert rc >= 0, (name, mode, ctx._L.p2e_last_error())
            if mode == "device":
                torch.cuda.synchronize()
                got = [o.cpu().numpy().copy() for o in outs]
            else:
                got = [o.copy() for o in outs]
                mask = np.ones(arena.size, bool)
                at = GUARD
                for w in out_widths:
                    mask[at:at + w * n] = False
                    at += w * n + GUARD
                assert (arena[mask] == PATTERN).all(), name
                assert all(np.array_equal(a, np.ascontiguousarray(b)) for a, b in zip(ins, inputs)), name
            results[mode] = (rc, got)
        assert results["device"][0] == results["host"][0], name
        assert all(np.array_equal(a, b) for a, b in zip(results["device"][1], results["host"][1])), name
        assert not any((g == 0xAA).all() for g in results["device"][1] if g.size >= 32), name
        flagged += results["device"][0]
    assert flagged >= 3
    for c in ctxs.values():
        c.close()


# ---- chains on device pointers in async mode --------------------------------------------------------------------------------------
def test_key_path_chain_stays_on_the_device():
    """BIP-32 children -> tweaked secret keys -> BIP-340 signatures, verified under the tweaked PUBLIC keys of the children's
    x-only keys: two routes to the same output key, nothing visits the host in between."""
    n = 65
    ctx = p2e.Context(device=0, asynchronous=True)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    full = lambda *shape: torch.full(shape, 0xAA, dtype=torch.uint8, device="cuda:0")
    P = HI.priv_set_one_parent()
    index = dev(np.arange(n, dtype=np.uint32).view(np.int32))
    sk_le, cc, e1, _ = ctx.bip32_ckd_priv_batch(dev(P["sk"][:1]), dev(P["cc"][:1]), index, sk=full(n, 32), cc=full(n, 32), err=full(n))
    sk = torch.flip(sk_le, dims=[1]).contiguous()          # the library's little-endian key -> the standard's byte string
    msg, aux = dev(np.frombuffer(TI._stream("chain msg", 32 * n), np.uint8).reshape(n, 32)), dev(np.zeros((n, 32), np.uint8))
    tsk, e2, _ = ctx.taproot_tweak_seckey_batch(sk, None, out_sk=full(n, 32), err=full(n))
    sig, e3, _ = ctx.schnorr_sign_batch(msg, tsk, aux, sig=full(n, 64), err=full(n))
    pk, e4, _ = ctx.schnorr_public_key_batch(sk, pk=full(n, 32), err=full(n))
    out_pk, par, e5, _ = ctx.taproot_tweak_pubkey_batch(pk, None, out_pk=full(n, 32), out_parity=full(n), err=full(n))
    e6, valid, _ = ctx.schnorr_verify_batch(msg, out_pk, sig, err=full(n), valid=full(n))
    assert ctx.sync() == 0
    torch.cuda.synchronize()
    for e in (e1, e2, e3, e4, e5, e6):
        assert not e.cpu().numpy().any()
    assert (valid.cpu().numpy() == 1).all()
    for i in (0, 1, 64):                                                        # three against the oracle, step by step
        code, k, _c = HI.ckd_priv(int.from_bytes(P["sk"][0].tobytes(), "little"), P["cc"][0].tobytes(), i)
        assert code == 0 and TI.tweak_seckey(TI.b32(k), None) == (0, tsk.cpu().numpy()[i].tobytes())
        assert TI.tweak_pubkey(TI.b32(TI.base_mul(k)[0]), None)[1] == out_pk.cpu().numpy()[i].tobytes()
    ctx.close()


def test_script_path_chain_stays_on_the_device():
    """leaf hashes -> roots -> tweaked keys -> the commitment check, for both leaves of pin 3 and the one leaf of pin 2"""
    ctx = p2e.Context(device=0, asynchronous=True)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    full = lambda *shape: torch.full(shape, 0xAA, dtype=torch.uint8, device="cuda:0")
    pin2, pin3 = TI.PINS[1], TI.PINS[2]
    leaves = [pin3["leaves"][0], pin3["leaves"][1], pin2["leaves"][0]]
    scripts = [bytes.fromhex(s) for _v, s, _h in leaves]
    n = 3
    offsets = dev(np.cumsum([0] + [len(s) for s in scripts]).astype(np.int64))
    leaf, e1, _ = ctx.taproot_leaf_hash_batch(dev(np.array([v for v, _s, _h in leaves], np.uint8)), dev(np.frombuffer(b"".join(scripts), np.uint8)),
                                              offsets, leaf=full(n, 32), err=full(n))
    path = torch.stack([leaf[1], leaf[0], leaf[2]]).reshape(n, 1, 32).contiguous()        # each leaf's sibling (pin 2: unused)
    depth = dev(np.array([1, 1, 0], np.uint8))
    root, e2, _ = ctx.taproot_merkle_root_batch(leaf, path, depth, root=full(n, 32), err=full(n))
    pk = dev(np.frombuffer(bytes.fromhex(pin3["internal"] * 2 + pin2["internal"]), np.uint8).reshape(n, 32))
    out_pk, par, e3, _ = ctx.taproot_tweak_pubkey_batch(pk, root, out_pk=full(n, 32), out_parity=full(n), err=full(n))
    e4, valid, _ = ctx.taproot_verify_commitment_batch(out_pk, par, pk, leaf, path, depth, err=full(n), valid=full(n))
    assert ctx.sync() == 0
    torch.cuda.synchronize()
    for e in (e1, e2, e3, e4):
        assert not e.cpu().numpy().any()
    assert valid.cpu().numpy().tolist() == [1, 1, 1]
    assert [r.tobytes().hex() for r in leaf.cpu().numpy()] == [h for _v, _s, h in leaves]
    assert [r.tobytes().hex() for r in root.cpu().numpy()] == [pin3["root"], pin3["root"], pin2["root"]]
    assert [r.tobytes().hex() for r in out_pk.cpu().numpy()] == [pin3["output"], pin3["output"], pin2["output"]]
    assert par.cpu().numpy().tolist() == [1, 1, 1]
    ctx.close()


# ---- behind the hash, on the device ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe():
    lib = os.path.join(PROBE, "libp2e_probe_taproot.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-s", "-C", PROBE, "libp2e_probe_taproot.so"])
    L = C.CDLL(lib)
    L.probetr_finish_pub.restype = L.probetr_finish_sec.restype = C.c_long
    return L


def test_forced_tweaks_on_the_device(probe):
    """t >= n refused, t = 0 and the doubling t G = P computed, t G = -P and d + t = 0 flagged.  65 elements: the table
    repeated, so that lanes of one wave take different branches."""
    be = lambda vals: np.frombuffer(b"".join(vals), np.uint8).reshape(-1, 32).copy()
    fp = [TI.forced_pub()[i % len(TI.forced_pub())] for i in range(65)]
    out, par, code = filled(65, 32), filled(65), filled(65)
    assert probe.probetr_finish_pub(_p(be([c[0] for c in fp])), _p(be([c[1] for c in fp])), _p(out), _p(par), _p(code), C.c_size_t(65)) == 0
    assert code.tolist() == [c[2] for c in fp], [(c[1].hex(), int(g)) for c, g in zip(fp, code) if c[2] != g][:8]
    assert np.array_equal(out, be([c[3] for c in fp])) and par.tolist() == [c[4] for c in fp]
    assert {TI.WIRE_OK, TI.WIRE_SCALAR_RANGE, TI.WIRE_INFINITY} == set(code.tolist())
    fs = [TI.forced_sec()[i % len(TI.forced_sec())] for i in range(65)]
    out, code = filled(65, 32), filled(65)
    assert probe.probetr_finish_sec(_p(be([c[0] for c in fs])), _p(be([c[1] for c in fs])), _p(out), _p(code), C.c_size_t(65)) == 0
    assert code.tolist() == [c[2] for c in fs] and np.array_equal(out, be([c[3] for c in fs]))


def test_c_example_scans_an_extended_key_for_its_taproot_outputs(tmp_path):
    """examples/taproot_scan.c: 300 children of test vector 1's m/0' as BIP-86 output keys, and the key-path spend of child 1"""
    exe = str(tmp_path / "taproot_scan")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "taproot_scan.c"), "-L", os.path.join(ROOT, "plonky2-ecdsa_amd"), "-lp2e_hip",
                           "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe])
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "plonky2-ecdsa_amd") + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    r = subprocess.run([exe, "300"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    code, k, _c = HI.ckd_priv(HI.TV1_M_0H[0], HI.TV1_M_0H[1], 1)
    want = TI.tweak_pubkey(TI.b32(TI.base_mul(k)[0]), None)[1].hex()
    assert code == 0 and f"300 children of m/0' tweaked (0 refused); the key-path signature of child 1 verifies under output key {want}" in r.stdout
