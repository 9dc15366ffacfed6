"""BIP-32 key derivation and HASH160 (include/p2e.h p2e_bip32_master_batch and the four calls after it) without a GPU.

The bodies of csrc/hd.hpp compiled with g++ (tests/emu_hd, built on demand, -DP2E_F29_BOUNDS: a violated limb bound of the
lazy 29-bit arithmetic aborts the process) against the oracle of tests/hd_inputs.py, a restatement of the standards in Python
integers, hmac and hashlib that uses nothing under test: SHA-512 and RIPEMD-160 through their compression bodies, the two
constant "Bitcoin seed" key states, every byte of every body on the input sets, and the arithmetic behind the hash with an
I_L no HMAC will ever produce.  The stand-alone sanitizer program of tests/emu_hd must exit 0.

One published answer differs from the issue that asked for this layer: RIPEMD-160("abc") ends in ...f15a0bfc in the paper's
appendix B (and in every implementation); the issue's ...f15a5bfc is a transcription slip.  The oracle is pinned to the paper."""
import ctypes as C
import hashlib
import os
import struct
import subprocess

import numpy as np
import pytest

import plonky2_ecdsa_amd as p2e
import hd_inputs as HI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "emu_hd")


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def filled(*shape):
    return np.full(shape, 0xAA, np.uint8)


@pytest.fixture(scope="module")
def emu():
    lib, prog = os.path.join(HERE, "libp2e_emu_hd.so"), os.path.join(HERE, "hd_selftest")
    if not (os.path.exists(lib) and os.path.exists(prog)):
        subprocess.check_call(["make", "-s", "-C", HERE])
    L = C.CDLL(lib)
    for name in ("emuhd_master", "emuhd_ckd_priv", "emuhd_ckd_pub", "emuhd_key_hash160", "emuhd_hash160"):
        getattr(L, name).restype = C.c_long
    return L


# ---- the oracle first: it is trusted only once it reproduces the published answers -------------------------------------------
def test_oracle_reproduces_the_published_answers():
    for msg, want in HI.RIPEMD160_KAT:
        assert HI.ripemd160(msg).hex() == want
    assert HI.hash160(HI.ser_p(HI.G)).hex() == HI.HASH160_OF_G == HI.key_hash160(HI.base_mul(1), HI.SEC1_COMPRESSED).hex()
    assert (HI.SHA512_K[0], HI.SHA512_K[79], HI.SHA512_IV[0]) == (0x428a2f98d728ae22, 0x6c44198c4a475817, 0x6a09e667f3bcc908)
    for data in (b"", b"abc", bytes(range(200)), b"x" * 111, b"y" * 112, b"z" * 128):
        assert HI.sha512_from_midstate(HI.SHA512_IV, 0, data) == hashlib.sha512(data).digest()
    # BIP-32 test vector 1: m, m/0', m/0'/1, and the public derivation m/0' -> 1
    assert HI.master(HI.TV1_SEED) == (0,) + HI.TV1_M
    code, k, c = HI.ckd_priv(HI.TV1_M[0], HI.TV1_M[1], HI.HARDENED)
    assert (code, k, c) == (0,) + HI.TV1_M_0H[:2] and HI.ser_p(HI.base_mul(k)) == HI.TV1_M_0H[2]
    code, k1, c1 = HI.ckd_priv(k, c, 1)
    assert (code, k1, c1) == (0,) + HI.TV1_M_0H_1[:2] and HI.ser_p(HI.base_mul(k1)) == HI.TV1_M_0H_1[2]
    code, K1, c1p = HI.ckd_pub(HI.base_mul(k), c, 1)
    assert code == 0 and HI.ser_p(K1) == HI.TV1_M_0H_1[2] and c1p == c1
    inner, outer = HI.hmac512_key_states(b"Bitcoin seed")
    assert HI.sha512_from_midstate(outer, 128, HI.sha512_from_midstate(inner, 128, HI.TV1_SEED)) == HI.hmac512(b"Bitcoin seed", HI.TV1_SEED)


def test_input_sets_contain_what_they_claim():
    idx = [int(v) for v in HI.indices()]
    assert len(idx) == 257 == HI.LENGTHS[-1] and set(HI.INDEX_EDGES) <= set(idx[:7])
    assert any(v >= HI.HARDENED for v in idx[6::7]) and any(v < HI.HARDENED for v in idx[6::7])
    S = HI.priv_set()
    val = lambda row: int.from_bytes(row.tobytes(), "little")
    parents = [val(r) for r in S["sk"]]
    assert {1, HI.N - 1, 0, HI.N, 2**256 - 1} <= set(parents)
    for i, k in enumerate(parents):                      # the three refused parents are flagged whatever the index, no other is
        assert (S["err"][i] == HI.WIRE_SCALAR_RANGE) == (k == 0 or k >= HI.N)
        assert S["err"][i] == 0 or not (S["out_sk"][i].any() or S["out_cc"][i].any())
    for k in (1, HI.N - 1):                              # each edge parent meets a hardened and an ordinary index
        kinds = {idx[i] >= HI.HARDENED for i, v in enumerate(parents) if v == k}
        assert kinds == {True, False}
    Q = HI.pub_set()
    assert set(Q["err"].tolist()) == {0, HI.WIRE_BAD_INDEX, HI.WIRE_INFINITY, HI.WIRE_COORD_RANGE, HI.WIRE_NOT_ON_CURVE}
    ok = [i for i in range(257) if Q["err"][i] == 0]
    assert {int(Q["pky"][i][0]) & 1 for i in ok} == {0, 1}                   # parents with y of both parities
    assert all(e == (HI.WIRE_BAD_INDEX if idx[i] >= HI.HARDENED else 0) for i, e in enumerate(HI.pub_set_one_parent()["err"]))
    # one parent: element 1 (index 1) under m/0' is test vector 1's m/0'/1, privately and publicly
    P1, Q1 = HI.priv_set_one_parent(), HI.pub_set_one_parent()
    assert idx[1] == 1 and val(P1["out_sk"][1]) == HI.TV1_M_0H_1[0] and P1["out_cc"][1].tobytes() == Q1["out_cc"][1].tobytes() == HI.TV1_M_0H_1[1]
    assert HI.ser_p((val(Q1["out_x"][1]), val(Q1["out_y"][1]))) == HI.TV1_M_0H_1[2]
    assert HI.SEED_LENGTHS == (16, 32, 63, 64) and HI.master_set(16)["seed"][0].tobytes() == HI.TV1_SEED
    data, offsets, want = HI.hash160_arrays()
    r = HI.HASH160_REVERSED
    assert offsets[r + 1] < offsets[r] and want[r].tobytes() == HI.hash160(b"") and len(data) == int(offsets[-1])
    H = HI.key_hash_set()
    assert H["c"][0].tobytes().hex() == HI.HASH160_OF_G and 0 < np.count_nonzero(H["err_in"]) < 257
    assert not H["c_err"][H["err_in"] != 0].any() and np.array_equal(H["u_err"][H["err_in"] == 0], H["u"][H["err_in"] == 0])
    # the forced table: what each case claims
    fp = {c[0]: c for c in HI.forced_priv()}
    assert [fp[k][3] for k in ("il_n", "il_n_plus_1", "il_max")] == [HI.WIRE_SCALAR_RANGE] * 3
    assert fp["il_zero"][3:] == (0, fp["il_zero"][2]) and fp["il_cancels"][3] == HI.WIRE_INFINITY and fp["il_cancels"][1] == HI.N - fp["il_cancels"][2]
    fq = {c[0]: c for c in HI.forced_pub()}
    assert [fq[k][3] for k in ("il_n", "il_n_plus_1", "il_max")] == [HI.WIRE_SCALAR_RANGE] * 3
    assert fq["il_zero"][3:] == (0, fq["il_zero"][2]) and fq["parent_is_minus_il_g"][3] == HI.WIRE_INFINITY
    c = fq["parent_is_il_g"]
    assert c[2] == HI.base_mul(c[1]) and c[3:] == (0, HI.base_mul(2 * c[1]))                          # the doubling


# ---- the hash functions through their compression bodies ------------------------------------------------------------------
@pytest.mark.parametrize("length", [0, 1, 111, 112, 127, 128, 129, 240])
def test_sha512_through_the_compression_body(length, emu):
    msg = bytes((7 * i + length) & 0xFF for i in range(length))
    data = msg + HI.sha512_pad(length)
    st = (C.c_uint64 * 8)()
    emu.emuhd_sha512_iv(st)
    assert tuple(st) == HI.SHA512_IV
    for at in range(0, len(data), 128):
        emu.emuhd_sha512_compress(st, data[at:at + 128])
    assert struct.pack(">8Q", *st) == hashlib.sha512(msg).digest()


@pytest.mark.parametrize("length", [0, 55, 56, 64, 119])
def test_ripemd160_through_the_compression_body(length, emu):
    msg = bytes((11 * i + length) & 0xFF for i in range(length))
    data = msg + HI.ripemd160_pad(length)
    assert len(data) == (64 if length < 56 else 128)
    st = (C.c_uint32 * 5)()
    emu.emuhd_ripemd160_iv(st)
    for at in range(0, len(data), 64):
        emu.emuhd_ripemd160_compress(st, data[at:at + 64])
    assert struct.pack("<5I", *st) == HI.ripemd160(msg)


def test_ripemd160_known_answers_through_the_body(emu):
    for msg, want in HI.RIPEMD160_KAT:
        st = (C.c_uint32 * 5)()
        emu.emuhd_ripemd160_iv(st)
        emu.emuhd_ripemd160_compress(st, msg + HI.ripemd160_pad(len(msg)))
        assert struct.pack("<5I", *st).hex() == want
    out = filled(20)
    emu.emuhd_hash160_of_digest(hashlib.sha256(HI.ser_p(HI.G)).digest(), _p(out))
    assert out.tobytes().hex() == HI.HASH160_OF_G


def test_seed_key_states_and_keyed_states(emu):
    got = (C.c_uint64 * 16)()
    emu.emuhd_seed_key_states(got)
    inner, outer = HI.hmac512_key_states(b"Bitcoin seed")
    assert tuple(got[:8]) == inner and tuple(got[8:]) == outer
    for cc in (bytes(32), HI.TV1_M[1], bytes(range(224, 256))):
        emu.emuhd_key_states(cc, got)
        inner, outer = HI.hmac512_key_states(cc)
        assert tuple(got[:8]) == inner and tuple(got[8:]) == outer


def test_hmac_of_the_37_byte_data(emu):
    for i, (b0, v, index) in enumerate(((0, HI.TV1_M[0], HI.HARDENED), (2, HI.G[0], 0), (3, 2**256 - 1, 2**32 - 1), (0, 0, 0x01020304))):
        cc = HI._rand("hmac-cc", i)
        out = filled(64)
        emu.emuhd_bip32_I(cc, C.c_uint(b0), _p(HI.le32(v).copy()), C.c_uint32(index), _p(out))
        assert out.tobytes() == HI.hmac512(cc, bytes([b0]) + v.to_bytes(32, "big") + struct.pack(">I", index))


# ---- every body, byte for byte, on the input sets ------------------------------------------------------------------------------
@pytest.mark.parametrize("one_parent", [False, True])
@pytest.mark.parametrize("n", HI.LENGTHS)
def test_ckd_priv_body_equals_the_oracle(n, one_parent, emu):
    S = HI.priv_set_one_parent() if one_parent else HI.priv_set()
    m = 1 if one_parent else n
    sk, cc, err = filled(n + 1, 32), filled(n + 1, 32), filled(n + 1)
    bad = emu.emuhd_ckd_priv(_p(S["sk"][:max(m, 1)].copy()), _p(S["cc"][:max(m, 1)].copy()), C.c_size_t(m), _p(S["index"][:max(n, 1)].copy()),
                             _p(sk), _p(cc), C.c_size_t(n), _p(err))
    diff = np.nonzero((sk[:n] != S["out_sk"][:n]).any(axis=1) | (cc[:n] != S["out_cc"][:n]).any(axis=1) | (err[:n] != S["err"][:n]))[0]
    assert diff.size == 0, [(int(i), int(S["index"][i]), int(err[i])) for i in diff[:8]]
    assert bad == np.count_nonzero(S["err"][:n]) and (sk[n] == 0xAA).all() and (cc[n] == 0xAA).all() and err[n] == 0xAA


@pytest.mark.parametrize("one_parent", [False, True])
@pytest.mark.parametrize("n", HI.LENGTHS)
def test_ckd_pub_body_equals_the_oracle(n, one_parent, emu):
    S = HI.pub_set_one_parent() if one_parent else HI.pub_set()
    m = 1 if one_parent else n
    x, y, cc, err = filled(n + 1, 32), filled(n + 1, 32), filled(n + 1, 32), filled(n + 1)
    bad = emu.emuhd_ckd_pub(_p(S["pkx"][:max(m, 1)].copy()), _p(S["pky"][:max(m, 1)].copy()), _p(S["cc"][:max(m, 1)].copy()), C.c_size_t(m),
                            _p(S["index"][:max(n, 1)].copy()), _p(x), _p(y), _p(cc), C.c_size_t(n), _p(err))
    diff = np.nonzero((x[:n] != S["out_x"][:n]).any(axis=1) | (y[:n] != S["out_y"][:n]).any(axis=1) |
                      (cc[:n] != S["out_cc"][:n]).any(axis=1) | (err[:n] != S["err"][:n]))[0]
    assert diff.size == 0, [(int(i), int(S["index"][i]), int(err[i]), int(S["err"][i])) for i in diff[:8]]
    assert bad == np.count_nonzero(S["err"][:n]) and (x[n] == 0xAA).all() and (y[n] == 0xAA).all() and (cc[n] == 0xAA).all() and err[n] == 0xAA


@pytest.mark.parametrize("seed_len", HI.SEED_LENGTHS)
@pytest.mark.parametrize("n", HI.LENGTHS)
def test_master_body_equals_the_oracle(n, seed_len, emu):
    S = HI.master_set(seed_len)
    seed = np.zeros((n * seed_len + 3) // 4 * 4 + 4, np.uint8)               # (a lane reads aligned words)
    seed[:n * seed_len] = S["seed"][:n].reshape(-1)
    sk, cc, err = filled(n + 1, 32), filled(n + 1, 32), filled(n + 1)
    bad = emu.emuhd_master(_p(seed), C.c_size_t(seed_len), _p(sk), _p(cc), C.c_size_t(n), _p(err))
    assert np.array_equal(sk[:n], S["sk"][:n]) and np.array_equal(cc[:n], S["cc"][:n]) and np.array_equal(err[:n], S["err"][:n])
    assert bad == 0 and (sk[n] == 0xAA).all() and (cc[n] == 0xAA).all() and err[n] == 0xAA


@pytest.mark.parametrize("n", HI.LENGTHS)
def test_hash160_bodies_equal_the_oracle(n, emu):
    data, offsets, want = HI.hash160_arrays()
    padded = np.zeros((len(data) + 3) // 4 * 4, np.uint8)
    padded[:len(data)] = data
    out = filled(n + 1, 20)
    bad = emu.emuhd_hash160(_p(padded), _p(offsets), _p(out), C.c_size_t(n))
    diff = np.nonzero((out[:n] != want[:n]).any(axis=1))[0]
    assert diff.size == 0, [(int(i), int(offsets[i]) % 4, int(offsets[i + 1]) - int(offsets[i])) for i in diff[:8]]
    assert bad == (1 if n > HI.HASH160_REVERSED else 0) and (out[n] == 0xAA).all()
    H = HI.key_hash_set()
    for form, plain, flagged in ((HI.SEC1_COMPRESSED, "c", "c_err"), (HI.SEC1_UNCOMPRESSED, "u", "u_err")):
        for err_in, key in ((None, plain), (H["err_in"][:max(n, 1)].copy(), flagged)):
            out = filled(n + 1, 20)
            assert emu.emuhd_key_hash160(C.c_uint(form), _p(H["pkx"][:max(n, 1)].copy()), _p(H["pky"][:max(n, 1)].copy()), _p(err_in), _p(out),
                                         C.c_size_t(n)) == 0
            assert np.array_equal(out[:n], H[key][:n]) and (out[n] == 0xAA).all(), (form, key)


# ---- the arithmetic behind the hash, with a forced I_L ---------------------------------------------------------------------------
def test_finish_priv_with_a_forced_il(emu):
    for name, il, k, code, want in HI.forced_priv():
        out = filled(32)
        got = emu.emuhd_finish_priv(_p(HI.le32(il).copy()), _p(HI.le32(k).copy()), _p(out))
        assert got == code, name
        assert (out == 0xAA).all() if code else out.tobytes() == want.to_bytes(32, "little"), name


def test_finish_pub_with_a_forced_il(emu):
    for name, il, kp, code, want in HI.forced_pub():
        ox, oy = filled(32), filled(32)
        got = emu.emuhd_finish_pub(_p(HI.le32(il).copy()), _p(HI.le32(kp[0]).copy()), _p(HI.le32(kp[1]).copy()), _p(ox), _p(oy))
        assert got == code, name
        if code:
            assert (ox == 0xAA).all() and (oy == 0xAA).all(), name
        else:
            assert (ox.tobytes(), oy.tobytes()) == (want[0].to_bytes(32, "little"), want[1].to_bytes(32, "little")), name


def vector_file(path):
    """the input sets, the oracle's expectations and the forced table in tests/emu_hd/hd_selftest.cpp's layout"""
    P, P1, Q, Q1 = HI.priv_set(), HI.priv_set_one_parent(), HI.pub_set(), HI.pub_set_one_parent()
    data, offsets, want = HI.hash160_arrays()
    H, fp, fq = HI.key_hash_set(), HI.forced_priv(), HI.forced_pub()
    le = lambda vals: np.stack([HI.le32(v) for v in vals])
    parts = [P["sk"], P["cc"], P["index"], P["out_sk"], P["out_cc"], P["err"], P1["sk"], P1["cc"], P1["out_sk"], P1["out_cc"], P1["err"],
             Q["pkx"], Q["pky"], Q["cc"], Q["out_x"], Q["out_y"], Q["out_cc"], Q["err"],
             Q1["pkx"], Q1["pky"], Q1["cc"], Q1["out_x"], Q1["out_y"], Q1["out_cc"], Q1["err"]]
    for seed_len in HI.SEED_LENGTHS:
        M = HI.master_set(seed_len)
        parts += [M["seed"], M["sk"], M["cc"], M["err"]]
    parts += [data, offsets, want, np.array([1], np.uint64), H["pkx"], H["pky"], H["err_in"], H["c"], H["u"], H["c_err"], H["u_err"]]
    parts += [le([c[1] for c in fp]), le([c[2] for c in fp]), np.array([c[3] for c in fp], np.uint8), le([c[4] for c in fp])]
    parts += [le([c[1] for c in fq]), le([c[2][0] for c in fq]), le([c[2][1] for c in fq]), np.array([c[3] for c in fq], np.uint8),
              le([c[4][0] for c in fq]), le([c[4][1] for c in fq])]
    with open(path, "wb") as f:
        f.write(struct.pack("<QQQQ", HI.N_SET, len(data), len(fp), len(fq)))
        for a in parts:
            f.write(np.ascontiguousarray(a).tobytes())


def test_sanitizer_program_exits_zero(emu, tmp_path):
    """tests/emu_hd/hd_selftest under -fsanitize=address,undefined: two published answers, every set, the forced table"""
    path = tmp_path / "hd_vectors.bin"
    vector_file(path)
    res = subprocess.run([os.path.join(HERE, "hd_selftest"), str(path)], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr


def test_entry_points_exist_and_refuse_misuse_without_a_device():
    L = p2e.lib()
    names = ("p2e_bip32_master_batch", "p2e_bip32_ckd_priv_batch", "p2e_bip32_ckd_pub_batch", "p2e_key_hash160_batch", "p2e_hash160_batch")
    for name in names:
        assert name in p2e.EXPORTS and getattr(L, name).restype is C.c_long
    buf = np.zeros(64, np.uint8)
    one = C.c_size_t(1)
    assert L.p2e_bip32_master_batch(None, _p(buf), C.c_size_t(16), _p(buf), _p(buf), one, _p(buf)) == -1
    assert L.p2e_bip32_ckd_priv_batch(None, _p(buf), _p(buf), one, _p(buf), _p(buf), _p(buf), one, _p(buf)) == -1
    assert L.p2e_bip32_ckd_pub_batch(None, _p(buf), _p(buf), _p(buf), one, _p(buf), _p(buf), _p(buf), _p(buf), one, _p(buf)) == -1
    assert L.p2e_key_hash160_batch(None, C.c_uint(0), _p(buf), _p(buf), None, _p(buf), one) == -1
    assert L.p2e_hash160_batch(None, _p(buf), _p(buf), _p(buf), one) == -1
    assert (p2e.WIRE_BAD_INDEX, p2e.WIRE_COORD_RANGE, p2e.WIRE_NOT_ON_CURVE, p2e.WIRE_INFINITY, p2e.WIRE_SCALAR_RANGE) == \
        (HI.WIRE_BAD_INDEX, HI.WIRE_COORD_RANGE, HI.WIRE_NOT_ON_CURVE, HI.WIRE_INFINITY, HI.WIRE_SCALAR_RANGE)


def test_example_compiles_against_the_header(tmp_path):
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                           os.path.join(ROOT, "examples", "hd_scan.c"), "-o", str(tmp_path / "hd_scan.o")])
