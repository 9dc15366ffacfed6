"""PBKDF2-HMAC-SHA512 and BIP-39 seeds on the GPU (include/p2e.h p2e_pbkdf2_hmac_sha512_batch, p2e_bip39_seed_batch) through
the C ABI.

Expectations come from tests/kdf_inputs.py alone: hashlib.pbkdf2_hmac, trusted once it agrees with a PBKDF2 written out by
hand and with the pin (tests/test_kdf_cpu.py).  Every byte of every element is compared; output buffers are pre-filled with
0xAA and carry one guard row so that an unwritten byte and a byte written past the end both show.

Shapes: both calls at count = 0, 1, 63, 64, 65 and 257 (nothing, one lane, a wave less one, a wave, a wave plus one, a block
plus one); the general call at 1, 2, 3 and 2048 iterations and 4, 32 and 64 bytes out; one element for the whole batch, of
either operand; host pointers (staged) and device pointers, the latter at every start alignment of both buffers.
tests/probe_kdf (built on demand with the library's flags) is a second, plain implementation on the device, compared with
the same oracle on the same sets."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import plonky2_ecdsa_amd as p2e
import hd_inputs as HI
import kdf_inputs as KI

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tests", "probe_kdf")


@pytest.fixture(scope="module")
def hctx():
    return p2e.Context(device=0, host_pointers=True)


@pytest.fixture(scope="module")
def dctx():
    return p2e.Context(device=0)


def _p(a):
    if a is None:
        return None
    return a.ctypes.data_as(C.c_void_p) if isinstance(a, np.ndarray) else C.c_void_p(a.data_ptr())


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()


def filled(on_device, *shape):
    return torch.full(shape, 0xAA, dtype=torch.uint8, device="cuda:0") if on_device else np.full(shape, 0xAA, np.uint8)


def host(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


def run_call(ctx, bip39, S, n_pw, n_salt, iterations, dk_len, n, no_salt=False):
    """one call over the first n elements of set S with one guard row behind the outputs -> (dk, err, flagged) on the host;
    each operand is cut to the elements the call may read (a pointer it must not follow further)"""
    on_device = not ctx.host_pointers
    put = dev if on_device else (lambda a: a.copy())
    pw, pw_off = put(S["pw"]), put(S["pw_off"][:n_pw + 1])
    salt, salt_off = (None, None) if no_salt else (put(S["salt"]), put(S["salt_off"][:n_salt + 1]))
    n_salt = 0 if no_salt else n_salt
    dk, err = filled(on_device, n + 1, dk_len), filled(on_device, n + 1)
    if bip39:
        assert iterations == KI.BIP39_ITERATIONS and dk_len == 64
        bad = ctx._L.p2e_bip39_seed_batch(ctx._h, _p(pw), _p(pw_off), C.c_size_t(n_pw), _p(salt), _p(salt_off), C.c_size_t(n_salt), _p(dk),
                                          C.c_size_t(n), _p(err))
    else:
        bad = ctx._L.p2e_pbkdf2_hmac_sha512_batch(ctx._h, _p(pw), _p(pw_off), C.c_size_t(n_pw), _p(salt), _p(salt_off), C.c_size_t(n_salt),
                                                  C.c_uint32(iterations), C.c_size_t(dk_len), _p(dk), C.c_size_t(n), _p(err))
    if on_device:
        torch.cuda.synchronize()
    return host(dk), host(err), bad


def assert_rows(dk, err, bad, want_dk, want_err, n, dk_len):
    assert bad >= 0, p2e.lib().p2e_last_error()
    diff = np.nonzero((dk[:n] != want_dk[:n, :dk_len]).any(axis=1) | (err[:n] != want_err[:n]))[0]
    assert diff.size == 0, [(int(i), int(err[i]), int(want_err[i])) for i in diff[:8]]
    assert bad == np.count_nonzero(want_err[:n]) and (dk[n] == 0xAA).all() and err[n] == 0xAA
    assert not dk[:n][want_err[:n] != 0].any()


@pytest.mark.parametrize("on_device", [False, True])
@pytest.mark.parametrize("dk_len", KI.DK_LENGTHS)
@pytest.mark.parametrize("iterations", KI.ITERATIONS)
def test_pbkdf2_equals_the_oracle(iterations, dk_len, on_device, hctx, dctx):
    want_dk, want_err = KI.expected(False, iterations)
    S = KI.operands(False, 0)
    for n in KI.LENGTHS:
        dk, err, bad = run_call(dctx if on_device else hctx, 0, S, n, n, iterations, dk_len, n)
        assert_rows(dk, err, bad, want_dk, want_err, n, dk_len)


@pytest.mark.parametrize("on_device", [False, True])
def test_bip39_seeds_equal_the_oracle(on_device, hctx, dctx):
    want_dk, want_err = KI.expected(True, KI.BIP39_ITERATIONS)
    S = KI.operands(True, 0)
    for n in KI.LENGTHS:
        dk, err, bad = run_call(dctx if on_device else hctx, 1, S, n, n, KI.BIP39_ITERATIONS, 64, n)
        assert_rows(dk, err, bad, want_dk, want_err, n, 64)


@pytest.mark.parametrize("start", [1, 2, 3])
@pytest.mark.parametrize("bip39", [0, 1])
def test_every_start_alignment_of_both_buffers(bip39, start, dctx):
    """device pointers: the elements sit where the caller put them, `start` bytes (the salts one more) behind an aligned base"""
    iterations = KI.BIP39_ITERATIONS if bip39 else 3
    want_dk, want_err = KI.expected(bool(bip39), iterations)
    n = KI.N_SET
    dk, err, bad = run_call(dctx, bip39, KI.operands(bool(bip39), start), n, n, iterations, 64, n)
    assert_rows(dk, err, bad, want_dk, want_err, n, 64)


@pytest.mark.parametrize("on_device", [False, True])
@pytest.mark.parametrize("bip39,form", [(0, "one_pw"), (0, "one_salt"), (1, "one_pw"), (1, "one_salt"), (1, "no_salt")])
def test_broadcast_forms(bip39, form, on_device, hctx, dctx):
    """one password for every salt, one salt for every password; and for BIP-39 no passphrase at all (the null operand is
    p2e_bip39_seed_batch's alone)"""
    iterations = KI.BIP39_ITERATIONS if bip39 else 3
    want_dk, want_err = KI.expected(bool(bip39), iterations, form)
    S = KI.operands(bool(bip39), 0)
    for n in (1, 65, KI.N_SET):
        dk, err, bad = run_call(dctx if on_device else hctx, bip39, S, 1 if form == "one_pw" else n, 1 if form == "one_salt" else n, iterations, 64,
                                n, form == "no_salt")
        assert_rows(dk, err, bad, want_dk, want_err, n, 64)


def test_the_pin_end_to_end(dctx):
    """sentence and passphrase -> seed -> master key -> m/0', on the device throughout, against tests/hd_inputs.py's oracle fed
    the hashlib seed.  Element 0 is the pin; the others are the sentence under other passphrases."""
    passphrases = [KI.PIN_PASSPHRASE] + [b"", b"trezor", "paßwort Å"] + [f"candidate-{i}".encode() for i in range(61)]
    n = len(passphrases)
    seed, e0, bad0 = dctx.bip39_seed_batch([KI.PIN_MNEMONIC], passphrases)
    sk, cc, e1, bad1 = dctx.bip32_master_batch(seed)
    hardened = dev(np.full(n, HI.HARDENED, np.uint32).view(np.int32))
    sk1, cc1, e2, bad2 = dctx.bip32_ckd_priv_batch(sk, cc, hardened)
    torch.cuda.synchronize()
    assert (bad0, bad1, bad2) == (0, 0, 0) and host(seed)[0].tobytes() == KI.PIN_SEED
    import unicodedata
    for i, pp in enumerate(passphrases):
        raw = unicodedata.normalize("NFKD", pp).encode() if isinstance(pp, str) else pp
        want_seed = KI.bip39_seed(KI.PIN_MNEMONIC, raw)
        assert host(seed)[i].tobytes() == want_seed, i
        code, k, c = HI.master(want_seed)
        code1, k1, c1 = HI.ckd_priv(k, c, HI.HARDENED)
        assert code == 0 and code1 == 0
        assert int.from_bytes(host(sk1)[i].tobytes(), "little") == k1 and host(cc1)[i].tobytes() == c1, i


def test_python_methods_pack_and_count(hctx):
    """lists of bytes / str, (buffer, offsets) pairs, the batch size from the longer operand"""
    S = KI.operands(False, 0)
    want_dk, want_err = KI.expected(False, 2)
    dk, err, bad = hctx.pbkdf2_hmac_sha512_batch((S["pw"].copy(), S["pw_off"].copy()), (S["salt"].copy(), S["salt_off"].copy()), 2, dk_len=32)
    assert np.array_equal(dk, want_dk[:, :32]) and np.array_equal(err, want_err) and bad == 2
    dk, err, bad = hctx.pbkdf2_hmac_sha512_batch([b"password"], [b"salt", b"pepper", ""], 1)
    assert bad == 0 and [r.tobytes() for r in dk] == [KI.pbkdf2(b"password", s, 1) for s in (b"salt", b"pepper", b"")]
    seed, err, bad = hctx.bip39_seed_batch([KI.PIN_MNEMONIC.decode(), KI.PIN_MNEMONIC])
    assert bad == 0 and seed[0].tobytes() == seed[1].tobytes() == KI.bip39_seed(KI.PIN_MNEMONIC)
    with pytest.raises(p2e.P2EError):
        hctx.bip39_seed_batch([b"a", b"b"], [b"x", b"y", b"z"])
    with pytest.raises(p2e.P2EError):
        hctx.pbkdf2_hmac_sha512_batch([b"a"], [b"b"], 0)


def test_refused_arguments_leave_the_context_usable(hctx):
    """what needs a real context: host-staged data that touches an output (BUFFER OVERLAP 5), offsets whose last entry lies below
    the first; nothing is written, and the next call works"""
    L, h = hctx._L, hctx._h
    arena = np.zeros(4096, np.uint8)
    arena[:8] = np.frombuffer(b"password", np.uint8)
    arena[128:132] = np.frombuffer(b"salt", np.uint8)
    pw_off, salt_off = np.array([0, 8], np.uint64), np.array([128, 132], np.uint64)
    one = C.c_size_t(1)
    at = lambda k: C.c_void_p(arena.ctypes.data + k)
    err, dk = np.full(1, 0xAA, np.uint8), np.full(64, 0xAA, np.uint8)
    call = lambda dk_p, err_p, po=pw_off, so=salt_off: L.p2e_pbkdf2_hmac_sha512_batch(h, at(0), _p(po), one, at(0), _p(so), one, C.c_uint32(2),
                                                                                    C.c_size_t(64), dk_p, one, err_p)
    for dk_p, err_p, name in ((at(4), _p(err), "password"), (at(100), _p(err), "salt"), (_p(dk), at(7), "password"), (_p(dk), at(131), "salt")):
        before = arena.copy()
        assert call(dk_p, err_p) == -1
        msg = L.p2e_last_error().decode()
        assert "overlap" in msg and name in msg and "variable-length data may not touch an output" in msg, msg
        assert np.array_equal(arena, before) and (dk == 0xAA).all() and (err == 0xAA).all()
    assert call(at(8), _p(err)) == 0 and arena[8:72].tobytes() == KI.pbkdf2(b"password", b"salt", 2)   # adjacent is no overlap
    arena[8:64] = 0
    assert call(_p(dk), _p(err), po=np.array([8, 0], np.uint64)) == -1 and "password" in L.p2e_last_error().decode()
    assert call(_p(dk), _p(err), so=np.array([132, 128], np.uint64)) == -1 and "salt" in L.p2e_last_error().decode()
    assert (dk == 0xAA).all()
    assert call(_p(dk), _p(err)) == 0 and dk.tobytes() == KI.pbkdf2(b"password", b"salt", 2) and err[0] == 0


def test_async_mode_gives_the_same_bytes_after_sync():
    ctx = p2e.Context(device=0, asynchronous=True)
    S = KI.operands(True, 2)
    want_dk, want_err = KI.expected(True, KI.BIP39_ITERATIONS)
    n = KI.N_SET
    seed, err = filled(True, n + 1, 64), filled(True, n + 1)
    pw, pw_off, salt, salt_off = dev(S["pw"]), dev(S["pw_off"]), dev(S["salt"]), dev(S["salt_off"])
    rc = ctx._L.p2e_bip39_seed_batch(ctx._h, _p(pw), _p(pw_off), C.c_size_t(n), _p(salt), _p(salt_off), C.c_size_t(n), _p(seed), C.c_size_t(n),
                                     _p(err))
    assert rc == 0                                                  # (the count comes with the sync)
    assert ctx.sync() == 2
    torch.cuda.synchronize()
    assert_rows(host(seed), host(err), 2, want_dk, want_err, n, 64)
    ctx.close()


@pytest.fixture(scope="module")
def probe():
    lib = os.path.join(PROBE, "libp2e_probe_kdf.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-s", "-C", PROBE, "libp2e_probe_kdf.so"])
    L = C.CDLL(lib)
    L.probekdf_pbkdf2.restype = C.c_long
    return L


@pytest.mark.parametrize("bip39,iterations,form", [(0, 1, "each"), (0, 3, "each"), (0, 2048, "each"), (1, 2048, "each"), (0, 3, "one_pw"),
                                                   (1, 2048, "one_salt"), (1, 2048, "no_salt")])
def test_the_plain_probe_kernel_equals_the_oracle(bip39, iterations, form, probe):
    """the second implementation on the device: hd.hpp's unchanged compression, bytes gathered one by one"""
    want_dk, want_err = KI.expected(bool(bip39), iterations, form)
    S = KI.operands(bool(bip39), 1)
    n = KI.N_SET
    pw, pw_off, salt, salt_off = dev(S["pw"]), dev(S["pw_off"]), dev(S["salt"]), dev(S["salt_off"])
    for dk_len in ((4, 64) if iterations == 3 else (64,)):
        dk, err = filled(True, n + 1, dk_len), filled(True, n + 1)
        no_salt = form == "no_salt"
        rc = probe.probekdf_pbkdf2(C.c_int(bip39), _p(pw), _p(pw_off), C.c_size_t(1 if form == "one_pw" else n), _p(None if no_salt else salt),
                                   _p(None if no_salt else salt_off), C.c_size_t(0 if no_salt else 1 if form == "one_salt" else n),
                                   C.c_uint32(iterations), C.c_size_t(dk_len), _p(dk), C.c_size_t(n), _p(err), None)
        torch.cuda.synchronize()
        assert rc == 0
        assert_rows(host(dk), host(err), int(np.count_nonzero(want_err)), want_dk, want_err, n, dk_len)


def test_c_example_finds_the_passphrase(tmp_path):
    """examples/mnemonic_scan.c: 300 candidate passphrases against one sentence; TREZOR stands at index 100"""
    exe = str(tmp_path / "mnemonic_scan")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "mnemonic_scan.c"), "-L", os.path.join(ROOT, "plonky2-ecdsa_amd"), "-lp2e_hip",
                           "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe])
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "plonky2-ecdsa_amd") + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    r = subprocess.run([exe, "300"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "300 passphrases tried against one mnemonic (0 refused), 1 match the target key hash: index 100 (TREZOR)" in r.stdout
