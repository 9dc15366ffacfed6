"""BIP-32 key derivation and HASH160 on the GPU (include/p2e.h p2e_bip32_master_batch, p2e_bip32_ckd_priv_batch,
p2e_bip32_ckd_pub_batch, p2e_key_hash160_batch, p2e_hash160_batch) through the C ABI.

Expectations come from tests/hd_inputs.py alone: a restatement of the standards in Python integers, hmac and hashlib.  Every
byte of every element is compared; output buffers are pre-filled with 0xAA so that an unwritten byte shows.

Shapes: every call at n = 0, 1, 63, 64, 65 and 257 (nothing, one lane, a wave less one, a wave, a wave plus one, a block plus
one), both with one parent per element and with one parent for the batch.  The arithmetic behind the hash runs with a forced
I_L through tests/probe_hd (built on demand with the library's flags): no HMAC output reaches those branches."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import plonky2_ecdsa_amd as p2e
import hd_inputs as HI

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tests", "probe_hd")


@pytest.fixture(scope="module")
def hctx():
    return p2e.Context(device=0, host_pointers=True)


def filled(*shape):
    return np.full(shape, 0xAA, np.uint8)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def rows_of(a, n):
    """the first n rows of an input array as its own buffer; one dummy row for n = 0 (a pointer the call must not follow)"""
    return a[:max(n, 1)].copy()


@pytest.mark.parametrize("one_parent", [False, True])
@pytest.mark.parametrize("n", HI.LENGTHS)
def test_ckd_priv_equals_the_oracle(n, one_parent, hctx):
    S = HI.priv_set_one_parent() if one_parent else HI.priv_set()
    m = 1 if one_parent else n
    sk, cc, err = filled(n + 1, 32), filled(n + 1, 32), filled(n + 1)
    bad = hctx._L.p2e_bip32_ckd_priv_batch(hctx._h, _p(rows_of(S["sk"], m)), _p(rows_of(S["cc"], m)), C.c_size_t(m), _p(rows_of(S["index"], n)),
                                           _p(sk), _p(cc), C.c_size_t(n), _p(err))
    diff = np.nonzero((sk[:n] != S["out_sk"][:n]).any(axis=1) | (cc[:n] != S["out_cc"][:n]).any(axis=1) | (err[:n] != S["err"][:n]))[0]
    assert diff.size == 0, [(int(i), int(S["index"][i]), int(err[i]), int(S["err"][i])) for i in diff[:8]]
    assert bad == np.count_nonzero(S["err"][:n]) and (sk[n] == 0xAA).all() and (cc[n] == 0xAA).all() and err[n] == 0xAA


@pytest.mark.parametrize("one_parent", [False, True])
@pytest.mark.parametrize("n", HI.LENGTHS)
def test_ckd_pub_equals_the_oracle(n, one_parent, hctx):
    S = HI.pub_set_one_parent() if one_parent else HI.pub_set()
    m = 1 if one_parent else n
    x, y, cc, err = filled(n + 1, 32), filled(n + 1, 32), filled(n + 1, 32), filled(n + 1)
    bad = hctx._L.p2e_bip32_ckd_pub_batch(hctx._h, _p(rows_of(S["pkx"], m)), _p(rows_of(S["pky"], m)), _p(rows_of(S["cc"], m)), C.c_size_t(m),
                                          _p(rows_of(S["index"], n)), _p(x), _p(y), _p(cc), C.c_size_t(n), _p(err))
    diff = np.nonzero((x[:n] != S["out_x"][:n]).any(axis=1) | (y[:n] != S["out_y"][:n]).any(axis=1) |
                      (cc[:n] != S["out_cc"][:n]).any(axis=1) | (err[:n] != S["err"][:n]))[0]
    assert diff.size == 0, [(int(i), int(S["index"][i]), int(err[i]), int(S["err"][i])) for i in diff[:8]]
    assert bad == np.count_nonzero(S["err"][:n]) and (x[n] == 0xAA).all() and (y[n] == 0xAA).all() and (cc[n] == 0xAA).all() and err[n] == 0xAA


@pytest.mark.parametrize("seed_len", HI.SEED_LENGTHS)
@pytest.mark.parametrize("n", HI.LENGTHS)
def test_master_equals_the_oracle(n, seed_len, hctx):
    S = HI.master_set(seed_len)
    sk, cc, err = filled(n + 1, 32), filled(n + 1, 32), filled(n + 1)
    bad = hctx._L.p2e_bip32_master_batch(hctx._h, _p(rows_of(S["seed"], n)), C.c_size_t(seed_len), _p(sk), _p(cc), C.c_size_t(n), _p(err))
    assert np.array_equal(sk[:n], S["sk"][:n]) and np.array_equal(cc[:n], S["cc"][:n]) and np.array_equal(err[:n], S["err"][:n])
    assert bad == 0 and (sk[n] == 0xAA).all() and (cc[n] == 0xAA).all() and err[n] == 0xAA
    if seed_len == 16 and n:
        assert int.from_bytes(sk[0].tobytes(), "little") == HI.TV1_M[0] and cc[0].tobytes() == HI.TV1_M[1]


@pytest.mark.parametrize("n", HI.LENGTHS)
def test_hash160_calls_equal_the_oracle(n, hctx):
    data, offsets, want = HI.hash160_arrays()
    out = filled(n + 1, 20)
    bad = hctx._L.p2e_hash160_batch(hctx._h, _p(data.copy()), _p(offsets[:n + 1].copy()), _p(out), C.c_size_t(n))
    diff = np.nonzero((out[:n] != want[:n]).any(axis=1))[0]
    assert diff.size == 0, [(int(i), int(offsets[i]) % 4, int(offsets[i + 1]) - int(offsets[i])) for i in diff[:8]]
    assert bad == (1 if n > HI.HASH160_REVERSED else 0) and (out[n] == 0xAA).all()
    H = HI.key_hash_set()
    for form, plain, flagged in ((HI.SEC1_COMPRESSED, "c", "c_err"), (HI.SEC1_UNCOMPRESSED, "u", "u_err")):
        for err_in, key in ((None, plain), (rows_of(H["err_in"], n), flagged)):
            out = filled(n + 1, 20)
            assert hctx._L.p2e_key_hash160_batch(hctx._h, C.c_uint(form), _p(rows_of(H["pkx"], n)), _p(rows_of(H["pky"], n)), _p(err_in), _p(out),
                                                 C.c_size_t(n)) == 0
            assert np.array_equal(out[:n], H[key][:n]) and (out[n] == 0xAA).all(), (form, key)
    if n:
        assert H["c"][0].tobytes().hex() == HI.HASH160_OF_G


def test_python_methods_give_the_same_bytes(hctx):
    """the Context methods allocate their outputs and count the parents themselves"""
    S, Q, M, H = HI.priv_set(), HI.pub_set_one_parent(), HI.master_set(63), HI.key_hash_set()
    sk, cc, err, bad = hctx.bip32_ckd_priv_batch(S["sk"].copy(), S["cc"].copy(), S["index"].copy())
    assert np.array_equal(sk, S["out_sk"]) and np.array_equal(cc, S["out_cc"]) and np.array_equal(err, S["err"]) and bad == np.count_nonzero(S["err"])
    x, y, cc, err, bad = hctx.bip32_ckd_pub_batch(Q["pkx"].copy(), Q["pky"].copy(), Q["cc"].copy(), Q["index"].copy())
    assert np.array_equal(x, Q["out_x"]) and np.array_equal(y, Q["out_y"]) and np.array_equal(cc, Q["out_cc"]) and np.array_equal(err, Q["err"])
    sk, cc, err, bad = hctx.bip32_master_batch(M["seed"].copy())
    assert np.array_equal(sk, M["sk"]) and np.array_equal(cc, M["cc"]) and bad == 0
    out, rc = hctx.key_hash160_batch(H["pkx"].copy(), H["pky"].copy(), form=p2e.SEC1_UNCOMPRESSED, err=H["err_in"].copy())
    assert np.array_equal(out, H["u_err"]) and rc == 0
    data, offsets, want = HI.hash160_arrays()
    out, bad = hctx.hash160_batch(data.copy(), offsets.copy())
    assert np.array_equal(out, want) and bad == 1
    with pytest.raises(p2e.P2EError):
        hctx.bip32_ckd_priv_batch(S["sk"][:2].copy(), S["cc"][:2].copy(), S["index"].copy())


def test_refused_arguments(hctx):
    L, h = hctx._L, hctx._h
    buf, idx = np.zeros(256, np.uint8), np.zeros(8, np.uint32)
    p, one, two, three = _p(buf), C.c_size_t(1), C.c_size_t(2), C.c_size_t(3)
    INV = -1
    # seed_len outside 16 .. 64, null pointers
    for seed_len in (0, 15, 65, 1 << 20):
        assert L.p2e_bip32_master_batch(h, p, C.c_size_t(seed_len), p, p, one, p) == INV
    sk1, cc1, err1 = np.zeros(32, np.uint8), np.zeros(32, np.uint8), np.zeros(1, np.uint8)     # (outputs are pairwise disjoint)
    assert L.p2e_bip32_master_batch(h, p, C.c_size_t(16), _p(sk1), _p(cc1), one, _p(err1)) == 0
    for k in range(4):
        a = [p, p, p, p]
        a[k] = None
        assert L.p2e_bip32_master_batch(h, a[0], C.c_size_t(16), a[1], a[2], one, a[3]) == INV
    # n_parents is 1 or n
    for m in (0, 2, 4):
        assert L.p2e_bip32_ckd_priv_batch(h, p, p, C.c_size_t(m), _p(idx), p, p, three, p) == INV
        assert L.p2e_bip32_ckd_pub_batch(h, p, p, p, C.c_size_t(m), _p(idx), p, p, p, three, p) == INV
    for k in range(6):
        a = [p, p, _p(idx), p, p, p]
        a[k] = None
        assert L.p2e_bip32_ckd_priv_batch(h, a[0], a[1], one, a[2], a[3], a[4], two, a[5]) == INV
    for k in range(8):
        a = [p, p, p, _p(idx), p, p, p, p]
        a[k] = None
        assert L.p2e_bip32_ckd_pub_batch(h, a[0], a[1], a[2], one, a[3], a[4], a[5], a[6], two, a[7]) == INV
    # an unknown form; err_in alone is nullable
    assert L.p2e_key_hash160_batch(h, C.c_uint(2), p, p, None, p, one) == INV
    assert L.p2e_key_hash160_batch(h, C.c_uint(0), None, p, None, p, one) == INV
    assert L.p2e_key_hash160_batch(h, C.c_uint(0), p, None, None, p, one) == INV
    assert L.p2e_key_hash160_batch(h, C.c_uint(0), p, p, None, None, one) == INV
    offsets = np.array([0, 3], np.uint64)
    assert L.p2e_hash160_batch(h, None, _p(offsets), p, one) == INV
    assert L.p2e_hash160_batch(h, p, None, p, one) == INV
    assert L.p2e_hash160_batch(h, p, _p(offsets), None, one) == INV
    assert L.p2e_hash160_batch(h, p, _p(np.array([5, 3], np.uint64)), p, one) == INV        # host staging: offsets[n] < offsets[0]
    # n == 0 returns 0 and follows no pointer but the required ones' null test
    zero = C.c_size_t(0)
    assert L.p2e_bip32_master_batch(h, p, C.c_size_t(32), p, p, zero, p) == 0
    assert L.p2e_bip32_ckd_priv_batch(h, p, p, one, _p(idx), p, p, zero, p) == 0
    assert L.p2e_bip32_ckd_pub_batch(h, p, p, p, zero, _p(idx), p, p, p, zero, p) == 0
    assert L.p2e_key_hash160_batch(h, C.c_uint(1), p, p, None, p, zero) == 0
    assert L.p2e_hash160_batch(h, p, _p(offsets), p, zero) == 0


def test_chain_stays_on_the_device():
    """master -> m/0' -> m/0'/1 -> public key, against the public derivation from m/0''s public key, then both key hashes:
    device pointers in async mode, nothing visits the host in between.  Element 0 is BIP-32's test vector 1."""
    n = 65
    ctx = p2e.Context(device=0, asynchronous=True)
    seeds = HI.master_set(16)["seed"][:n].copy()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    full = lambda *shape: torch.full(shape, 0xAA, dtype=torch.uint8, device="cuda:0")
    hardened = dev(np.full(n, HI.HARDENED, np.uint32).view(np.int32))
    first = dev(np.full(n, 1, np.uint32).view(np.int32))
    sk_m, cc_m, e1, _ = ctx.bip32_master_batch(dev(seeds), sk=full(n, 32), cc=full(n, 32), err=full(n))
    sk_h, cc_h, e2, _ = ctx.bip32_ckd_priv_batch(sk_m, cc_m, hardened, sk=full(n, 32), cc=full(n, 32), err=full(n))
    sk_c, cc_c, e3, _ = ctx.bip32_ckd_priv_batch(sk_h, cc_h, first, sk=full(n, 32), cc=full(n, 32), err=full(n))
    x_c, y_c, e4, _ = ctx.ecdsa_public_key_batch(sk_c, plan=p2e.SIGN_PLAN_LANE, pkx=full(n, 32), pky=full(n, 32), err=full(n))
    x_h, y_h, e5, _ = ctx.ecdsa_public_key_batch(sk_h, plan=p2e.SIGN_PLAN_LANE, pkx=full(n, 32), pky=full(n, 32), err=full(n))
    x_p, y_p, cc_p, e6, _ = ctx.bip32_ckd_pub_batch(x_h, y_h, cc_h, first, pkx=full(n, 32), pky=full(n, 32), cc=full(n, 32), err=full(n))
    h_key, _ = ctx.key_hash160_batch(x_p, y_p, form=p2e.SEC1_COMPRESSED, err=e6, out=full(n, 20))
    sec1, e7, _ = ctx.point_encode_batch(x_p, y_p, form=p2e.SEC1_COMPRESSED, out=full(n, 33), err=full(n))
    offsets = dev(np.arange(n + 1, dtype=np.int64) * 33)
    h_msg, _ = ctx.hash160_batch(sec1, offsets, out=full(n, 20))
    assert ctx.sync() == 0
    torch.cuda.synchronize()
    for e in (e1, e2, e3, e4, e5, e6, e7):
        assert not e.cpu().numpy().any()
    host = lambda t: t.cpu().numpy()
    assert np.array_equal(host(x_c), host(x_p)) and np.array_equal(host(y_c), host(y_p)) and np.array_equal(host(cc_c), host(cc_p))
    assert np.array_equal(host(h_key), host(h_msg))
    val = lambda t, i: int.from_bytes(host(t)[i].tobytes(), "little")
    assert (val(sk_m, 0), host(cc_m)[0].tobytes()) == HI.TV1_M
    assert (val(sk_h, 0), host(cc_h)[0].tobytes()) == HI.TV1_M_0H[:2] and HI.ser_p((val(x_h, 0), val(y_h, 0))) == HI.TV1_M_0H[2]
    assert (val(sk_c, 0), host(cc_c)[0].tobytes()) == HI.TV1_M_0H_1[:2]
    assert host(sec1)[0].tobytes() == HI.TV1_M_0H_1[2] == HI.ser_p((val(x_p, 0), val(y_p, 0)))
    assert host(h_key)[0].tobytes() == HI.hash160(HI.TV1_M_0H_1[2])
    for i in (1, 33, 64):                                                       # three more against the oracle, step by step
        code, k, c = HI.master(seeds[i].tobytes())
        code, k, c = HI.ckd_priv(k, c, HI.HARDENED)
        code, k, c = HI.ckd_priv(k, c, 1)
        assert code == 0 and (val(sk_c, i), host(cc_c)[i].tobytes()) == (k, c) and (val(x_p, i), val(y_p, i)) == HI.base_mul(k)
    ctx.close()


@pytest.fixture(scope="module")
def probe():
    lib = os.path.join(PROBE, "libp2e_probe_hd.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-s", "-C", PROBE, "libp2e_probe_hd.so"])
    L = C.CDLL(lib)
    L.probehd_finish_priv.restype = L.probehd_finish_pub.restype = C.c_long
    return L


def test_forced_il_on_the_device(probe):
    """the issue's table: I_L >= n refused, I_L = 0 computed, a zero child key and a neutral child point flagged, the doubling
    computed.  65 elements: the table repeated, so that lanes of one wave take different branches."""
    le = lambda vals: np.stack([HI.le32(v) for v in vals])
    fp = [HI.forced_priv()[i % len(HI.forced_priv())] for i in range(65)]
    out, code = filled(65, 32), filled(65)
    assert probe.probehd_finish_priv(_p(le([c[1] for c in fp])), _p(le([c[2] for c in fp])), _p(out), _p(code), C.c_size_t(65)) == 0
    assert code.tolist() == [c[3] for c in fp]
    assert np.array_equal(out, le([c[4] for c in fp]))
    fq = [HI.forced_pub()[i % len(HI.forced_pub())] for i in range(65)]
    ox, oy, code = filled(65, 32), filled(65, 32), filled(65)
    assert probe.probehd_finish_pub(_p(le([c[1] for c in fq])), _p(le([c[2][0] for c in fq])), _p(le([c[2][1] for c in fq])), _p(ox), _p(oy),
                                    _p(code), C.c_size_t(65)) == 0
    assert code.tolist() == [c[3] for c in fq], [(c[0], int(g)) for c, g in zip(fq, code) if c[3] != g][:8]
    assert np.array_equal(ox, le([c[4][0] for c in fq])) and np.array_equal(oy, le([c[4][1] for c in fq]))
    kinds = {c[0]: c[3] for c in fq}
    assert kinds["parent_is_il_g"] == 0 and kinds["parent_is_minus_il_g"] == HI.WIRE_INFINITY and kinds["il_zero"] == 0


def test_c_example_scans_an_extended_key(tmp_path):
    """examples/hd_scan.c: one extended public key, 300 children, their key hashes; child 1 is test vector 1's m/0'/1"""
    exe = str(tmp_path / "hd_scan")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "hd_scan.c"), "-L", os.path.join(ROOT, "plonky2-ecdsa_amd"), "-lp2e_hip",
                           "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe])
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "plonky2-ecdsa_amd") + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    r = subprocess.run([exe, "300"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    want = HI.hash160(HI.TV1_M_0H_1[2]).hex()
    assert f"300 children of m/0' derived (0 refused), child 1 is m/0'/1 of test vector 1, its key hash {want}" in r.stdout
