"""BUFFER OVERLAP (include/p2e.h) on the GPU.

1. In place equals the oracle.  Every in-place form the header lists runs on DEVICE pointers (host staging would hide a race)
   at n = 65 and 257, both curves, every plan the call has, on the input sets of the other GPU tests, and is compared byte
   for byte with the expectations those modules compute -- never with an out-of-place run of the library.  Flagged elements
   are in every batch: zeros in place, the right err code.
2. Refused and untouched.  With a real context, every kind of refusal once per call family, the buffers carved out of one
   allocation filled with 0xAA with a spare row on either side of each: the call returns P2E_E_INVALID, names the overlap, not
   one byte changes, and the same context then reproduces the oracle.  Synchronous, asynchronous and host-pointer contexts.
3. The path-deepening case: one parent, 257 indices; in place with n_parents = 1 is refused, with the parent in its own bytes
   the oracle's children come out, and two more levels run in place with n_parents = n.

tests/test_overlap_cpu.py holds the rule itself and the refusals of every call without a GPU."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import hash_inputs as H
import hd_inputs as HI
import plonky2_ecdsa_amd as p2e
import point_arith_inputs as PI
import recover_inputs as RI
import schnorr_inputs as SI
import sign_inputs as S
import table_inputs as TI

pytestmark = pytest.mark.gpu

SIZES = (65, 257)        # a wave plus one lane; a 256-block plus one lane (the quad plans: 260 and 1028 lanes)
E_INVALID = -1
SIGN_PLANS = (S.PLAN_LANE, S.PLAN_QUAD)


@pytest.fixture(scope="module")
def ctx():
    c = p2e.Context(device=0)
    yield c
    c.close()


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def fresh(n, w=32):
    return torch.full((n, w) if w > 1 else (n,), 0xAA, dtype=torch.uint8, device="cuda")


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def same_rows(got, want, what):
    got = host(got) if torch.is_tensor(got) else got
    diff = np.nonzero((got != want).reshape(len(want), -1).any(axis=1))[0]
    assert diff.size == 0, (what, diff[:8].tolist())


# ---- 1. in place equals the oracle -------------------------------------------------------------------------------------------
def small_batch(cv, n, seed, shift):
    """n raw 256-bit values out of sign_inputs.edges: its tail (one-group and one-empty-group scalars, n, n + 1, 2^256 - 1, 0),
    a stride through its table entries, random filler; rotated by `shift` so that the flagged elements of sk, k and msg differ"""
    e = S.edges(cv)
    vals = e[-14:] + e[:960:41]
    rng = S.R.SplitMix64(seed)
    vals += [rng.below(1 << 256) for _ in range(n - len(vals))]
    assert len(vals) == n
    return vals[shift:] + vals[:shift]


@functools.lru_cache(maxsize=None)
def sign_case(curve_id, n):
    cv = S.CURVES[curve_id]
    sk, k, msg = small_batch(cv, n, 0x0551 + curve_id, 1), small_batch(cv, n, 0x0561 + curve_id, 0), small_batch(cv, n, 0x0571 + curve_id, 7)
    red = [v % cv.n for v in k]
    pts = S.base_points(curve_id, red)
    v = np.array([0 if kk == 0 else (pts[kk][1] & 1) | (2 if pts[kk][0] >= cv.n else 0) for kk in red], np.uint8)
    keys, sigs = S.expect_keys(curve_id, sk), S.expect_sigs(curve_id, msg, sk, k)
    assert keys[2].any() and not keys[2].all() and sigs[2].any() and not sigs[2].all()
    return dict(b=[S.pack(x) for x in (msg, sk, k)], keys=keys, sigs=sigs, v=v)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("curve_id", [0, 1])
def test_keys_and_signatures_in_place(curve_id, n, ctx):
    c = sign_case(curve_id, n)
    wx, wy, we1 = c["keys"]
    wr, ws, we2 = c["sigs"]
    for plan in SIGN_PLANS:
        what = (curve_id, n, plan)
        msg, sk, k = [dev(a) for a in c["b"]]
        pkx, pky, err, bad = ctx.ecdsa_public_key_batch(sk, curve=curve_id, plan=plan, pkx=sk, pky=fresh(n), err=fresh(n, 1))      # pkx = sk
        same_rows(sk, wx, what + ("pkx on sk",)), same_rows(pky, wy, what), same_rows(err, we1, what)
        assert bad == np.count_nonzero(we1)
        msg, sk, k = [dev(a) for a in c["b"]]
        r, s, err, bad = ctx.ecdsa_sign_batch(msg, sk, k, curve=curve_id, plan=plan, r=msg, s=k, err=fresh(n, 1))                  # r = msg, s = k
        same_rows(msg, wr, what + ("r on msg",)), same_rows(k, ws, what + ("s on k",)), same_rows(err, we2, what)
        assert bad == np.count_nonzero(we2) and np.array_equal(host(sk), c["b"][1])
        msg, sk, k = [dev(a) for a in c["b"]]
        r, s, v, err, bad = ctx.ecdsa_sign_recoverable_batch(msg, sk, k, curve=curve_id, plan=plan, r=msg, s=k, v=fresh(n, 1), err=fresh(n, 1))
        same_rows(msg, wr, what + ("recoverable r on msg",)), same_rows(k, ws, what + ("recoverable s on k",))
        same_rows(err, we2, what), same_rows(v, c["v"], what + ("v",))
        assert bad == np.count_nonzero(we2)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("curve_id", [0, 1])
def test_nonces_and_deterministic_signatures_in_place(curve_id, n, ctx):
    msg, sk, want_k = [list(x) for x in H.nonce_batch(curve_id, n)]
    m = dev(H.pack(msg))
    _k, rc = ctx.ecdsa_nonce_rfc6979_batch(m, dev(H.pack(sk)), curve=curve_id, k=m)                                                 # k = msg
    same_rows(m, H.pack(want_k), (curve_id, n, "k on msg"))
    assert rc == 0
    wr, ws, werr = S.expect_sigs(curve_id, msg, sk, want_k)
    assert not werr.any()                                     # (an RFC 6979 nonce is never 0: this signer flags nothing)
    for plan in SIGN_PLANS:
        m, d = dev(H.pack(msg)), dev(H.pack(sk))
        r, s, v, err, bad = ctx.ecdsa_sign_deterministic_batch(m, d, curve=curve_id, plan=plan, r=m, s=fresh(n), v=fresh(n, 1), err=fresh(n, 1))
        same_rows(m, wr, (curve_id, n, plan, "r on msg")), same_rows(s, ws, (curve_id, n, plan, "s"))
        assert bad == 0 and not host(err).any()


@functools.lru_cache(maxsize=None)
def recover_case(curve_id, n):
    x = list(RI.set_x(curve_id))
    cases = (x * (n // len(x) + 1))[:n]
    a = RI.arrays(cases)
    assert a["err"].any() and not a["err"].all()
    return a


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("curve_id", [0, 1])
def test_recovery_in_place(curve_id, n, ctx):
    a = recover_case(curve_id, n)
    msg, r, s, v = [dev(a[k]) for k in ("msg", "r", "s", "v")]
    pkx, pky, err, bad = ctx.ecdsa_recover_batch(msg, r, s, v, curve=curve_id, pkx=r, pky=s, err=fresh(n, 1))                       # pkx = r, pky = s
    same_rows(r, a["pkx"], (curve_id, n, "pkx on r")), same_rows(s, a["pky"], (curve_id, n, "pky on s")), same_rows(err, a["err"], "err")
    assert bad == np.count_nonzero(a["err"]) and np.array_equal(host(msg), a["msg"])


@functools.lru_cache(maxsize=None)
def point_case(curve_id, op, n):
    x = list(PI.set_x(curve_id, op))
    cases = (x[::2] + x[1::2])[:n // 2]                         # half edge cases (both halves of X's order), half filler
    cases += PI.set_f(curve_id, op, n - len(cases))
    a = PI.arrays(cases)
    assert len(cases) == n and a["err"].any() and not a["err"].all()
    return a


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("op", ["mul", "lincomb", "add"])
@pytest.mark.parametrize("curve_id", [0, 1])
def test_point_arithmetic_in_place(curve_id, op, n, ctx):
    a = point_case(curve_id, op, n)
    bad_want = np.count_nonzero(a["err"])
    for plan in (PI.PLANS[curve_id] if op != "add" else (PI.PLAN_AUTO,)):
        what = (curve_id, op, n, plan)
        px, py = dev(a["px"]), dev(a["py"])
        if op == "mul":                                         # out = P
            _x, _y, err, bad = ctx.point_mul_batch(dev(a["b"]), px, py, curve=curve_id, plan=plan, outx=px, outy=py, err=fresh(n, 1))
        elif op == "lincomb":
            _x, _y, err, bad = ctx.point_lincomb_batch(dev(a["a"]), dev(a["b"]), px, py, curve=curve_id, plan=plan, outx=px, outy=py, err=fresh(n, 1))
        else:
            _x, _y, err, bad = ctx.point_add_batch(px, py, dev(a["qx"]), dev(a["qy"]), curve=curve_id, outx=px, outy=py, err=fresh(n, 1))
        same_rows(px, a["outx"], what + ("outx on px",)), same_rows(py, a["outy"], what + ("outy on py",)), same_rows(err, a["err"], what)
        assert bad == bad_want
        if op == "mul":                                         # outx = k
            k = dev(a["b"])
            _x, oy, err, bad = ctx.point_mul_batch(k, dev(a["px"]), dev(a["py"]), curve=curve_id, plan=plan, outx=k, outy=fresh(n), err=fresh(n, 1))
            same_rows(k, a["outx"], what + ("outx on k",)), same_rows(oy, a["outy"], what), same_rows(err, a["err"], what)
            assert bad == bad_want


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("curve_id", [0, 1])
def test_table_calls_in_place(curve_id, n, ctx):
    m = 4
    px, py = TI.point_arrays(curve_id, m)
    table = ctx.point_table(dev(px), dev(py), curve=curve_id)
    try:
        for op in ("mul", "lincomb"):
            cases = TI.batch(curve_id, m, op, n)[:n]
            a = TI.arrays(cases)
            assert len(cases) == n and a["err"].any() and not a["err"].all()
            for on in (("b",) if op == "mul" else ("b", "a")):  # outx on the scalar of the table point; lincomb: on a as well
                ins = {k: dev(a[k]) for k in ("a", "b")}
                if op == "mul":
                    _x, oy, err, bad = ctx.point_table_mul_batch(table, ins["b"], idx=dev(a["idx"]), outx=ins[on], outy=fresh(n), err=fresh(n, 1))
                else:
                    _x, oy, err, bad = ctx.point_table_lincomb_batch(table, ins["a"], ins["b"], idx=dev(a["idx"]), outx=ins[on], outy=fresh(n),
                                                                     err=fresh(n, 1))
                what = (curve_id, n, op, on)
                same_rows(ins[on], a["outx"], what + ("outx on the scalar",)), same_rows(oy, a["outy"], what), same_rows(err, a["err"], what)
                assert bad == np.count_nonzero(a["err"])
    finally:
        table.close()


@pytest.mark.parametrize("n", SIZES)
def test_schnorr_keys_and_decoding_in_place(n, ctx):
    a, v = SI.signer_arrays(), SI.verifier_arrays()
    sk = dev(a["sk"][:n])
    _pk, err, bad = ctx.schnorr_public_key_batch(sk, pk=sk, err=fresh(n, 1))                                                        # pk = sk
    same_rows(sk, a["pk"][:n], (n, "pk on sk")), same_rows(err, a["pk_err"][:n], (n, "pk err"))
    assert bad == np.count_nonzero(a["pk_err"][:n]) > 0
    pk = dev(v["pk"][:n])
    _px, py, err, bad = ctx.xonly_decode_batch(pk, px=pk, py=fresh(n), err=fresh(n, 1))                                             # px = pk
    same_rows(pk, v["dx"][:n], (n, "px on pk")), same_rows(py, v["dy"][:n], (n, "py")), same_rows(err, v["derr"][:n], (n, "decode err"))
    assert bad == np.count_nonzero(v["derr"][:n]) > 0


@pytest.mark.parametrize("n", SIZES)
def test_children_over_parents(n, ctx):
    """n_parents == n: the children and their chain codes over the parents, privately and publicly"""
    P, Q = HI.priv_set(), HI.pub_set()
    sk, cc = dev(P["sk"][:n]), dev(P["cc"][:n])
    _s, _c, err, bad = ctx.bip32_ckd_priv_batch(sk, cc, dev(P["index"][:n]), sk=sk, cc=cc, err=fresh(n, 1))
    same_rows(sk, P["out_sk"][:n], (n, "sk on par_sk")), same_rows(cc, P["out_cc"][:n], (n, "cc on par_cc")), same_rows(err, P["err"][:n], n)
    assert bad == np.count_nonzero(P["err"][:n]) > 0
    x, y, cc = dev(Q["pkx"][:n]), dev(Q["pky"][:n]), dev(Q["cc"][:n])
    _x, _y, _c, err, bad = ctx.bip32_ckd_pub_batch(x, y, cc, dev(Q["index"][:n]), pkx=x, pky=y, cc=cc, err=fresh(n, 1))
    same_rows(x, Q["out_x"][:n], (n, "pkx on par_pkx")), same_rows(y, Q["out_y"][:n], (n, "pky on par_pky"))
    same_rows(cc, Q["out_cc"][:n], (n, "cc on par_cc")), same_rows(err, Q["err"][:n], n)
    assert bad == np.count_nonzero(Q["err"][:n]) > 0


# ---- 3. the path-deepening case ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def deeper_levels():
    """levels 2 and 3 under the one-parent sets: the oracle applied to its own children, flagged ones (zeros) included"""
    idx = [int(v) for v in HI.indices()]
    val = lambda row: int.from_bytes(row.tobytes(), "little")
    P, Q = HI.priv_set_one_parent(), HI.pub_set_one_parent()
    priv, pub = [P], [Q]
    for _level in range(2):
        prev = priv[-1]
        priv.append(HI._priv_arrays([val(r) for r in prev["out_sk"]], [r.tobytes() for r in prev["out_cc"]], idx))
        prev = pub[-1]
        pub.append(HI._pub_arrays([(val(a), val(b)) for a, b in zip(prev["out_x"], prev["out_y"])], [r.tobytes() for r in prev["out_cc"]], idx))
    return priv, pub


def test_deepening_a_path_in_place(ctx):
    n = HI.N_SET
    priv, pub = deeper_levels()
    L, h = ctx._L, ctx._h
    index = dev(HI.indices())
    assert any(v >= HI.HARDENED for v in HI.indices()) and any(v < HI.HARDENED for v in HI.indices())
    # private: the children over the single parent are refused, on the key and on the chain code
    arena = fresh(2 * (n + 2))
    sk, cc, err = arena[1:n + 1], arena[n + 3:2 * n + 3], fresh(n, 1)
    for osk, occ in ((sk, fresh(n)), (fresh(n), cc)):
        assert L.p2e_bip32_ckd_priv_batch(h, p2e._ptr(sk), p2e._ptr(cc), C.c_size_t(1), p2e._ptr(index), p2e._ptr(osk), p2e._ptr(occ), C.c_size_t(n),
                                          p2e._ptr(err)) == E_INVALID
        assert b"overlap" in L.p2e_last_error() and b"par_" in L.p2e_last_error()
    torch.cuda.synchronize()
    assert bool((arena == 0xAA).all()) and bool((err == 0xAA).all())
    # ... the parent in its own 32 + 32 bytes: the oracle's children; then two more levels in place, one parent per child
    sk, cc, err, bad = ctx.bip32_ckd_priv_batch(dev(priv[0]["sk"]), dev(priv[0]["cc"]), index, sk=fresh(n), cc=fresh(n), err=fresh(n, 1))
    same_rows(sk, priv[0]["out_sk"], "level 1 sk"), same_rows(cc, priv[0]["out_cc"], "level 1 cc"), same_rows(err, priv[0]["err"], "level 1 err")
    for level in (1, 2):
        assert np.array_equal(priv[level]["sk"], priv[level - 1]["out_sk"])
        _s, _c, err, bad = ctx.bip32_ckd_priv_batch(sk, cc, index, sk=sk, cc=cc, err=fresh(n, 1))
        same_rows(sk, priv[level]["out_sk"], (level, "sk")), same_rows(cc, priv[level]["out_cc"], (level, "cc")), same_rows(err, priv[level]["err"], level)
        assert bad == np.count_nonzero(priv[level]["err"])
    assert np.count_nonzero(priv[2]["err"] == 0) > 100
    # public
    x, y, cc, err = arena[1:n + 1], arena[n + 3:2 * n + 3], fresh(n), fresh(n, 1)
    assert L.p2e_bip32_ckd_pub_batch(h, p2e._ptr(x), p2e._ptr(y), p2e._ptr(cc), C.c_size_t(1), p2e._ptr(index), p2e._ptr(x), p2e._ptr(y), p2e._ptr(cc),
                                     C.c_size_t(n), p2e._ptr(err)) == E_INVALID and b"overlap" in L.p2e_last_error()
    torch.cuda.synchronize()
    assert bool((arena == 0xAA).all()) and bool((cc == 0xAA).all())
    x, y, cc, err, bad = ctx.bip32_ckd_pub_batch(dev(pub[0]["pkx"]), dev(pub[0]["pky"]), dev(pub[0]["cc"]), index, pkx=fresh(n), pky=fresh(n),
                                                 cc=fresh(n), err=fresh(n, 1))
    same_rows(x, pub[0]["out_x"], "level 1 x"), same_rows(y, pub[0]["out_y"], "level 1 y"), same_rows(cc, pub[0]["out_cc"], "level 1 cc")
    for level in (1, 2):
        _x, _y, _c, err, bad = ctx.bip32_ckd_pub_batch(x, y, cc, index, pkx=x, pky=y, cc=cc, err=fresh(n, 1))
        same_rows(x, pub[level]["out_x"], (level, "x")), same_rows(y, pub[level]["out_y"], (level, "y"))
        same_rows(cc, pub[level]["out_cc"], (level, "cc")), same_rows(err, pub[level]["err"], level)
        assert bad == np.count_nonzero(pub[level]["err"])
    assert np.count_nonzero(pub[2]["err"] == 0) > 50


# ---- 2. refused and untouched ------------------------------------------------------------------------------------------------
class Arena:
    """`slots` buffers of n rows of 32 bytes in ONE allocation of 0xAA, a spare row in front of and behind each: a refused call
    that wrote anywhere near its arguments would be seen.  Device memory, or host memory for a host-pointer context."""

    def __init__(self, slots, n, on_host=False):
        self.n, self.on_host = n, on_host
        shape = (slots * (n + 2), 32)
        self.mem = np.full(shape, 0xAA, np.uint8) if on_host else torch.full(shape, 0xAA, dtype=torch.uint8, device="cuda")
        self.base = self.mem.ctypes.data if on_host else self.mem.data_ptr()

    def at(self, slot, shift=0):
        """the address of buffer `slot`, moved by `shift` bytes"""
        return C.c_void_p(self.base + 32 * (slot * (self.n + 2) + 1) + shift)

    def untouched(self):
        if not self.on_host:
            torch.cuda.synchronize()
        return bool((self.mem == 0xAA).all())


def refusals(n):
    """(family, call name, arguments behind ctx as a function of an Arena, the two names the message must hold): every kind of
    refusal -- an output shifted onto an input, two outputs on one buffer, a broadcast or shared input under an output, an
    in-place form with another stride -- once per call family"""
    z = C.c_size_t(n)
    one = C.c_size_t(1)
    return [
        ("sign", "p2e_ecdsa_public_key_batch", lambda A: (0, 0, A.at(0), A.at(0, 32), A.at(1), z, A.at(2)), ("sk32", "pkx32")),
        ("sign", "p2e_ecdsa_sign_batch", lambda A: (0, 1, A.at(0), A.at(1), A.at(2), A.at(3), A.at(3), z, A.at(4)), ("r32", "s32")),
        ("sign", "p2e_ecdsa_sign_recoverable_batch", lambda A: (1, 2, A.at(0), A.at(1), A.at(2), A.at(3), A.at(4), A.at(5), z, A.at(5)), ("v", "err")),
        ("recover", "p2e_ecdsa_recover_batch", lambda A: (0, A.at(0), A.at(1), A.at(2), A.at(3), A.at(1, -32), A.at(4), z, A.at(5)), ("r32", "pkx32")),
        ("hash", "p2e_ecdsa_nonce_rfc6979_batch", lambda A: (0, A.at(0), A.at(1), A.at(1, 32), z), ("sk32", "k32")),
        ("hash", "p2e_ecdsa_sign_deterministic_batch", lambda A: (0, 0, A.at(0), A.at(1), A.at(2), A.at(2, 16), A.at(3), z, A.at(4)), ("r32", "s32")),
        ("hash", "p2e_eth_address_batch", lambda A: (A.at(0), A.at(1), None, A.at(0), z), ("pkx32", "addr20")),
        ("wire", "p2e_point_encode_batch", lambda A: (0, 0, A.at(0), A.at(1), A.at(1), z, A.at(2)), ("py32", "out")),
        ("wire", "p2e_sig_decode_batch", lambda A: (0, 1, 0, A.at(0), None, A.at(0), A.at(2), None, z, A.at(3)), ("data", "r32")),
        ("wire", "p2e_sig_encode_batch", lambda A: (0, 2, 0, A.at(0), A.at(1), A.at(2), A.at(3), None, z, A.at(2, 1)), ("v", "err")),
        ("msm", "p2e_point_msm", lambda A: (0, 0, A.at(0), A.at(1), A.at(2), z, A.at(1, 32), A.at(3), A.at(4), None), ("px32", "outx32")),
        ("point", "p2e_point_mul_batch", lambda A: (0, 0, A.at(0), A.at(1), A.at(2), A.at(1, 32), A.at(3), z, A.at(4)), ("px32", "outx32")),
        ("point", "p2e_point_lincomb_batch", lambda A: (0, 0, A.at(0), A.at(1), A.at(2), A.at(3), A.at(4), A.at(4), z, A.at(5)), ("outx32", "outy32")),
        ("point", "p2e_point_add_batch", lambda A: (1, A.at(0), A.at(1), A.at(2), A.at(3), A.at(4), A.at(3, -32), z, A.at(5)), ("qy32", "outy32")),
        ("schnorr", "p2e_schnorr_public_key_batch", lambda A: (A.at(0), A.at(0, 1), z, A.at(1)), ("sk32", "pk32")),
        ("schnorr", "p2e_schnorr_sign_batch", lambda A: (A.at(0), A.at(1), A.at(2), A.at(0), z, A.at(4)), ("msg32", "sig64")),
        ("schnorr", "p2e_xonly_decode_batch", lambda A: (A.at(0), A.at(1), A.at(1), z, A.at(2)), ("px32", "py32")),
        ("schnorr", "p2e_schnorr_verify_aggregate", lambda A: (A.at(0), A.at(1), A.at(2), z, A.at(4), 0, A.at(4, 31), None), ("seed32", "verdict")),
        ("hd", "p2e_bip32_master_batch", lambda A: (A.at(0), C.c_size_t(32), A.at(0), A.at(1), z, A.at(2)), None),     # in place is fine ...
        ("hd", "p2e_bip32_master_batch", lambda A: (A.at(0), C.c_size_t(16), A.at(0), A.at(1), z, A.at(2)), ("seed", "sk32")),   # ... at the same stride only
        ("hd", "p2e_bip32_ckd_priv_batch", lambda A: (A.at(0), A.at(1), one, A.at(2), A.at(0), A.at(3), z, A.at(4)), ("par_sk32", "sk32")),
        ("hd", "p2e_bip32_ckd_pub_batch", lambda A: (A.at(0), A.at(1), A.at(2), one, A.at(3), A.at(4), A.at(5), A.at(2), z, A.at(6)), ("par_cc32", "cc32")),
        ("hd", "p2e_key_hash160_batch", lambda A: (0, A.at(0), A.at(1), A.at(2), A.at(2), z), ("err_in", "out20")),
    ]


@pytest.mark.parametrize("mode", ["sync", "async", "host"])
def test_refused_calls_touch_nothing_and_leave_the_context_usable(mode):
    n = 65
    c = p2e.Context(device=0, asynchronous=mode == "async", host_pointers=mode == "host")
    try:
        L, h = c._L, c._h
        seen = set()
        for family, name, make, names in refusals(n):
            A = Arena(8, n, on_host=mode == "host")
            rc = getattr(L, name)(h, *make(A))
            if names is None:                                   # the in-place twin of the next row: accepted, and it writes
                assert rc >= 0, (name, L.p2e_last_error())
                assert c.sync() >= 0 if mode == "async" else True
                assert not A.untouched()
                continue
            msg = (L.p2e_last_error() or b"").decode()
            assert rc == E_INVALID and "overlap" in msg and all(w in msg for w in names), (name, rc, msg)
            assert A.untouched(), name
            if mode == "async":
                assert c.sync() == 0, name                      # nothing was queued
            seen.add(family)
        assert seen == {"sign", "recover", "hash", "wire", "msm", "point", "schnorr", "hd"}
        # the table calls need a table: refused with it, and the table still works
        px, py = TI.point_arrays(0, 4)
        table = c.point_table(px.copy() if mode == "host" else dev(px), py.copy() if mode == "host" else dev(py), curve=0)
        A = Arena(8, n, on_host=mode == "host")
        assert L.p2e_point_table_mul_batch(h, table._h, None, A.at(0), A.at(0, 32), A.at(1), C.c_size_t(n), A.at(2)) == E_INVALID
        assert b"overlap" in L.p2e_last_error() and b"k32" in L.p2e_last_error() and b"outx32" in L.p2e_last_error()
        assert L.p2e_ecdsa_verify_table_batch(h, table._h, A.at(0), A.at(1), A.at(2), A.at(3), C.c_size_t(n), A.at(4), A.at(4)) == E_INVALID
        assert b"overlap" in L.p2e_last_error() and b"valid" in L.p2e_last_error()
        assert L.p2e_point_table_create(h, 0, A.at(0), A.at(1), C.c_size_t(n), A.at(1, 8), C.byref(C.c_void_p())) == E_INVALID
        assert b"overlap" in L.p2e_last_error() and b"point_err" in L.p2e_last_error()
        assert A.untouched()
        if mode == "async":
            assert c.sync() == 0
        # n == 0 checks nothing and returns 0, whatever lies on whatever
        zero = C.c_size_t(0)
        assert L.p2e_ecdsa_sign_batch(h, 0, 0, A.at(0), A.at(0), A.at(0), A.at(0), A.at(0), zero, A.at(0)) == 0
        assert L.p2e_bip32_ckd_priv_batch(h, A.at(0), A.at(0), C.c_size_t(1), A.at(0), A.at(0), A.at(0), zero, A.at(0)) == 0
        assert L.p2e_point_table_mul_batch(h, table._h, None, A.at(0), A.at(0), A.at(0), zero, A.at(0)) == 0
        assert A.untouched()
        # the same context still reproduces the oracle: keys, and a table product
        case = sign_case(0, n)
        sk = case["b"][1].copy() if mode == "host" else dev(case["b"][1])
        pkx, pky, err, bad = c.ecdsa_public_key_batch(sk, curve=0, plan=S.PLAN_LANE)
        if mode == "async":
            assert bad == 0
            bad = c.sync()
        wx, wy, we = case["keys"]
        same_rows(pkx, wx, (mode, "pkx")), same_rows(pky, wy, (mode, "pky")), same_rows(err, we, (mode, "err"))
        assert bad == np.count_nonzero(we)
        a = TI.arrays(TI.batch(0, 4, "mul", n)[:n])
        k, idx = (a["b"].copy(), a["idx"].copy()) if mode == "host" else (dev(a["b"]), dev(a["idx"]))
        ox, oy, err, bad = c.point_table_mul_batch(table, k, idx=idx)
        if mode == "async":
            bad = c.sync()
        same_rows(ox, a["outx"], (mode, "table outx")), same_rows(oy, a["outy"], (mode, "table outy")), same_rows(err, a["err"], (mode, "table err"))
        assert bad == np.count_nonzero(a["err"])
        table.close()
    finally:
        c.close()


def test_variable_length_data_may_not_touch_an_output_where_the_host_knows_its_extent():
    """host-pointer staging reads offsets[0] and offsets[n] anyway: there the extent of data is checked against the outputs"""
    n = 5
    c = p2e.Context(device=0, host_pointers=True)
    try:
        L, h = c._L, c._h
        mem = np.full(4096, 0xAA, np.uint8)
        base = mem.ctypes.data
        at = lambda off: C.c_void_p(base + off)
        offsets = np.arange(n + 1, dtype=np.uint64) * 40 + 8           # data[8, 208)
        po, z = offsets.ctypes.data_as(C.c_void_p), C.c_size_t(n)
        calls = [
            ("p2e_hash_batch", lambda out: (0, 0, at(0), po, at(out), z)),
            ("p2e_hash160_batch", lambda out: (at(0), po, at(out), z)),
            ("p2e_point_decode_batch", lambda out: (0, at(0), po, at(out), at(1024), z, at(2048))),
            ("p2e_sig_decode_batch", lambda out: (0, 0, 0, at(0), po, at(1024), at(out), None, z, at(2048))),
        ]
        for name, make in calls:
            for out in (207, 100, 8):                                   # on the last byte of data, in its middle, on its first byte
                rc = getattr(L, name)(h, *make(out))
                msg = (L.p2e_last_error() or b"").decode()
                assert rc == E_INVALID and "overlap" in msg and "data" in msg, (name, out, rc, msg)
                assert (mem == 0xAA).all(), name
            assert getattr(L, name)(h, *make(208)) >= 0, (name, L.p2e_last_error())     # right behind the data: no overlap
            assert not (mem[208:] == 0xAA).all() and (mem[:208] == 0xAA).all()
            mem[:] = 0xAA
        # the context is still good
        a = SI.signer_arrays()
        pk, err, bad = c.schnorr_public_key_batch(a["sk"][:n].copy())
        assert np.array_equal(pk, a["pk"][:n])
    finally:
        c.close()
