"""Message hashing, RFC 6979 nonces and Ethereum addresses (include/p2e.h p2e_hash_batch, p2e_ecdsa_nonce_rfc6979_batch,
p2e_eth_address_batch) without a GPU.

The kernel bodies of csrc/hash.hpp compiled with g++ (tests/emu_hash, built on demand) against tests/hash_inputs.py: every
padding edge length of both hashes at every start residue in one concatenated buffer, both output forms, every byte; the
published answers literally; 300 nonces per curve against the Python RFC 6979; the retry set under the synthetic order
2^255 + 1 through tests/probe_hash's host build (value and number of refused candidates of every element).  The stand-alone
sanitizer program of tests/emu_hash must exit 0."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

import hash_inputs as H
import plonky2_ecdsa_amd as p2e

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "emu_hash")
PROBE = os.path.join(ROOT, "tests", "probe_hash")
N_CPU = 1040             # 16 wave-sized groups + 16: every edge length many times, every start residue
RANDOM = 300


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def emu():
    lib, prog = os.path.join(HERE, "libp2e_emu_hash.so"), os.path.join(HERE, "hash_selftest")
    if not (os.path.exists(lib) and os.path.exists(prog)):
        subprocess.check_call(["make", "-s", "-C", HERE])
    L = C.CDLL(lib)
    L.emuh_hash.restype = L.emuh_nonce.restype = L.emuh_nonce_order.restype = L.emuh_eth_address.restype = C.c_long
    return L


def _hash(emu, alg, form, msgs):
    data = np.frombuffer(b"".join(msgs) + b"\0", np.uint8).copy()
    offsets = np.zeros(len(msgs) + 1, np.uint64)
    offsets[1:] = np.cumsum([len(m) for m in msgs])
    out = np.zeros((len(msgs), 32), np.uint8)
    assert emu.emuh_hash(alg, form, _p(data), _p(offsets), _p(out), C.c_size_t(len(msgs))) == 0
    return out


@pytest.mark.parametrize("form", [H.DIGEST_BYTES, H.DIGEST_SCALAR])
@pytest.mark.parametrize("alg", H.ALGS)
def test_every_digest_byte_on_the_edge_lengths(alg, form, emu):
    data, offsets, msgs = H.message_batch(alg, N_CPU)
    assert {len(m) for m in msgs} == set(H.KECCAK_LENGTHS if alg == H.KECCAK256 else H.SHA_LENGTHS)
    out = np.full((N_CPU + 1, 32), 0xAA, np.uint8)
    for shift in (0, 1, 2, 3):                                   # the whole buffer at every alignment of its first byte
        room = np.zeros(data.size + 16, np.uint8)                # (the emulation reads the aligned words around the ends)
        view = room[8 - shift:8 - shift + data.size]
        view[:] = data
        out[:] = 0xAA
        assert emu.emuh_hash(alg, form, _p(view), _p(offsets), _p(out), C.c_size_t(N_CPU)) == 0
        want = H.as_form(H.digests(alg, N_CPU), form)
        diff = np.nonzero((out[:N_CPU] != want).any(axis=1))[0]
        assert diff.size == 0, (alg, form, shift, [(int(i), len(msgs[i])) for i in diff[:8]])
        assert (out[N_CPU] == 0xAA).all()


def test_published_answers(emu):
    assert _hash(emu, H.SHA256, 0, [b"abc"])[0].tobytes().hex() == H.SHA256_ABC
    assert _hash(emu, H.KECCAK256, 0, [b""])[0].tobytes().hex() == H.KECCAK_EMPTY
    assert _hash(emu, H.KECCAK256, 0, [b"abc"])[0].tobytes().hex() == H.KECCAK_ABC
    assert _hash(emu, H.SHA256D, 0, [b"abc"])[0].tobytes() == hashlib.sha256(hashlib.sha256(b"abc").digest()).digest()
    # RFC 6979 A.2.5 (P-256, SHA-256): the nonces of "sample" and "test", and the signature of "sample" they lead to
    z = _hash(emu, H.SHA256, H.DIGEST_SCALAR, [b"sample", b"test", b"Satoshi Nakamoto"])
    assert H.unpack(z)[0] == int.from_bytes(hashlib.sha256(b"sample").digest(), "big")
    x, k = H.pack([H.A25_X, H.A25_X]), np.zeros((2, 32), np.uint8)
    assert emu.emuh_nonce(1, _p(z), _p(x), _p(k), C.c_size_t(2)) == 0
    assert H.unpack(k) == [H.A25_SAMPLE_K, H.A25_TEST_K]
    assert H.sign(H.CURVES[1], H.unpack(z)[0], H.A25_X, H.A25_SAMPLE_K)[:2] == (H.A25_SAMPLE_R, H.A25_SAMPLE_S)
    # secp256k1, sk = 1
    one, k1 = H.pack([1]), np.zeros((1, 32), np.uint8)
    assert emu.emuh_nonce(0, _p(z[2:]), _p(one), _p(k1), C.c_size_t(1)) == 0
    assert H.unpack(k1) == [H.SATOSHI_K]
    # the same three through the Python RFC 6979 the other tests rely on
    assert H.rfc6979(H.CURVES[1].n, H.A25_X, H.unpack(z)[0]) == (H.A25_SAMPLE_K, 0)
    assert H.rfc6979(H.CURVES[1].n, H.A25_X, H.unpack(z)[1]) == (H.A25_TEST_K, 0)
    assert H.rfc6979(H.CURVES[0].n, 1, H.unpack(z)[2]) == (H.SATOSHI_K, 0)
    # the address of 1 G; a flagged element gives zeros
    pkx, pky, want = H.address_batch(8)
    addr = np.full((9, 20), 0xAA, np.uint8)
    err = np.array([0, 4, 0, 128, 0, 0, 64, 0], np.uint8)
    assert emu.emuh_eth_address(_p(pkx), _p(pky), None, _p(addr), C.c_size_t(8)) == 0
    assert addr[0].tobytes().hex() == H.ADDRESS_OF_G and np.array_equal(addr[:8], want) and (addr[8] == 0xAA).all()
    assert emu.emuh_eth_address(_p(pkx), _p(pky), _p(err), _p(addr), C.c_size_t(8)) == 0
    assert np.array_equal(addr[:8], np.where(err[:, None] != 0, 0, want)) and (addr[8] == 0xAA).all()


@pytest.mark.parametrize("curve_id", [0, 1])
def test_nonces_equal_the_python_rfc6979(curve_id, emu):
    """the 25 edge pairs of {0, 1, n - 1, n, 2^256 - 1} and 300 random pairs"""
    msg, sk, want = H.nonce_batch(curve_id, 25 + RANDOM)
    k = np.full((25 + RANDOM + 1, 32), 0xAA, np.uint8)
    assert emu.emuh_nonce(curve_id, _p(H.pack(msg)), _p(H.pack(sk)), _p(k), C.c_size_t(25 + RANDOM)) == 0
    got = H.unpack(k[:-1])
    assert got == want and (k[-1] == 0xAA).all()
    assert all(1 <= v < H.CURVES[curve_id].n for v in got)


def test_non_monotonic_offsets_are_empty_messages_and_counted(emu):
    data = np.arange(64, dtype=np.uint8)
    offsets = np.array([0, 10, 4, 4, 30, 20, 64], np.uint64)              # elements 1 and 4 run backwards
    out = np.zeros((6, 32), np.uint8)
    assert emu.emuh_hash(H.SHA256, 0, _p(data), _p(offsets), _p(out), C.c_size_t(6)) == 2
    raw = data.tobytes()
    want = [raw[0:10], b"", b"", raw[4:30], b"", raw[20:64]]
    assert [bytes(r) for r in out] == [hashlib.sha256(m).digest() for m in want]


@pytest.fixture(scope="module")
def probe_host():
    lib = os.path.join(PROBE, "libp2e_probe_hash_host.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-s", "-C", PROBE, "libp2e_probe_hash_host.so"])
    L = C.CDLL(lib)
    L.probeh_nonce.restype = C.c_long
    return L


def test_retry_set_statistics():
    """what the synthetic order is for: 102 of the 200 inputs refuse at least one candidate, the deepest refuses 7, and
    about half take the z >= q subtraction"""
    _xs, zs, _ks, refused = H.retry_set()
    assert sum(1 for r in refused if r) == 102 and max(refused) == 7
    assert 80 <= sum(1 for z in zs if z >= H.RETRY_Q) <= 120


def test_retry_branch_in_the_host_build(probe_host):
    xs, zs, ks, refused = H.retry_set()
    k, rej = np.full((H.RETRY_N, 32), 0xAA, np.uint8), np.full(H.RETRY_N, 0xAAAAAAAA, np.uint32)
    assert probe_host.probeh_nonce(_p(H.pack([H.RETRY_Q])), _p(H.pack(xs)), _p(H.pack(zs)), _p(k), _p(rej), C.c_size_t(H.RETRY_N)) == 0
    assert H.unpack(k) == ks
    assert rej.tolist() == refused


def test_sanitizer_program_exits_zero(emu):
    """tests/emu_hash/hash_selftest: answers, read bounds and the retry branch under -fsanitize=address,undefined"""
    res = subprocess.run([os.path.join(HERE, "hash_selftest")], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr


def test_entry_points_exist_and_refuse_misuse_without_a_device():
    L = p2e.lib()
    names = ("p2e_hash_batch", "p2e_ecdsa_nonce_rfc6979_batch", "p2e_ecdsa_sign_deterministic_batch", "p2e_eth_address_batch")
    for name in names:
        assert name in p2e.EXPORTS and getattr(L, name).restype is C.c_long
    buf = np.zeros(64, np.uint8)
    assert L.p2e_hash_batch(None, 0, 0, _p(buf), _p(buf), _p(buf), C.c_size_t(1)) == -1
    assert L.p2e_ecdsa_nonce_rfc6979_batch(None, 0, _p(buf), _p(buf), _p(buf), C.c_size_t(1)) == -1
    assert L.p2e_ecdsa_sign_deterministic_batch(None, 0, 0, _p(buf), _p(buf), _p(buf), _p(buf), _p(buf), C.c_size_t(1), _p(buf)) == -1
    assert L.p2e_eth_address_batch(None, _p(buf), _p(buf), None, _p(buf), C.c_size_t(1)) == -1
    assert (p2e.HASH_SHA256, p2e.HASH_SHA256D, p2e.HASH_KECCAK256, p2e.DIGEST_BYTES, p2e.DIGEST_SCALAR) == (0, 1, 2, 0, 1)
