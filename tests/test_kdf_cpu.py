"""PBKDF2-HMAC-SHA512 and BIP-39 seeds (include/p2e.h p2e_pbkdf2_hmac_sha512_batch, p2e_bip39_seed_batch) without a GPU.

The bodies of csrc/kdf.hpp compiled with g++ (tests/emu_kdf, built on demand) against the oracle of tests/kdf_inputs.py,
hashlib.pbkdf2_hmac, which is trusted once it agrees with a PBKDF2 written out by hand and with the pin: the streaming
absorber against hashlib.sha512 on every length 0 .. 260 at every alignment, from the IV and from behind a 128-byte block,
with and without the prefix and the block index; the fixed-shape compression against hd.hpp's general one on random states;
every byte of every element of the whole body at 1, 2, 3 and 2048 iterations and 4, 32 and 64 bytes out; both broadcast
forms.  The stand-alone sanitizer program of tests/emu_kdf must exit 0.

The two entry points are checked through p2e.lib() with tests/test_overlap_cpu.py's machinery and a span table of this file's
own: the calls name their batch size `count`, so that file's list (derived from `n` / `m`) leaves them out."""
import ctypes as C
import hashlib
import itertools
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import plonky2_ecdsa_amd as p2e
import hd_inputs as HI
import kdf_inputs as KI
from test_overlap_cpu import Call, _refused, fake, header_calls  # noqa: F401  (fake is a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "emu_kdf")


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def filled(*shape):
    return np.full(shape, 0xAA, np.uint8)


@pytest.fixture(scope="module")
def emu():
    lib, prog = os.path.join(HERE, "libp2e_emu_kdf.so"), os.path.join(HERE, "kdf_selftest")
    if not (os.path.exists(lib) and os.path.exists(prog)):
        subprocess.check_call(["make", "-s", "-C", HERE])
    L = C.CDLL(lib)
    L.emukdf_pbkdf2.restype = C.c_long
    return L


def run_body(emu, bip39, S, n_pw, n_salt, iterations, dk_len, n, no_salt=False):
    """the emulated call over the first n elements of set S (one guard row behind the outputs) -> (dk, err, flagged)"""
    dk, err = filled(n + 1, dk_len), filled(n + 1)
    salt, salt_off, n_salt = (None, None, 0) if no_salt else (S["salt"], S["salt_off"], n_salt)
    bad = emu.emukdf_pbkdf2(C.c_int(bip39), _p(S["pw"]), _p(S["pw_off"]), C.c_size_t(n_pw), _p(salt), _p(salt_off), C.c_size_t(n_salt),
                            C.c_uint32(iterations), C.c_size_t(dk_len), _p(dk), C.c_size_t(n), _p(err))
    return dk, err, bad


def assert_rows(dk, err, bad, want_dk, want_err, n, dk_len):
    diff = np.nonzero((dk[:n] != want_dk[:n, :dk_len]).any(axis=1) | (err[:n] != want_err[:n]))[0]
    assert diff.size == 0, [(int(i), int(err[i]), int(want_err[i])) for i in diff[:8]]
    assert bad == np.count_nonzero(want_err[:n]) and (dk[n] == 0xAA).all() and err[n] == 0xAA
    assert not dk[:n][want_err[:n] != 0].any()


# ---- the oracle first: it is trusted only once it reproduces the by-hand PBKDF2 and the pin -----------------------------------
def test_oracle_reproduces_the_by_hand_pbkdf2_and_the_pin():
    """hashlib.pbkdf2_hmac against RFC 8018 5.2 written out with hmac and hashlib.sha512, on every pair of edge lengths, and
    against the pin (abandon ... about / TREZOR).  Were a published vector ever to disagree with hashlib, hashlib wins."""
    assert KI.check_oracle() == len(KI.PW_LENGTHS) * 16 * 3 + 2
    assert KI.bip39_seed(KI.PIN_MNEMONIC, KI.PIN_PASSPHRASE) == KI.PIN_SEED


def test_a_long_password_and_its_digest_are_the_same_key():
    """RFC 2104: a key longer than the block is replaced by its SHA-512 digest"""
    S = KI.operands(False)
    pw = S["pws"][KI.LONG_PW]
    assert len(pw) == 129
    for salt in (b"", b"salt", S["salts"][KI.LONG_PW]):
        assert KI.pbkdf2(pw, salt, 3) == KI.pbkdf2(hashlib.sha512(pw).digest(), salt, 3)
    assert KI.pbkdf2(pw[:128], b"salt", 3) != KI.pbkdf2(hashlib.sha512(pw[:128]).digest(), b"salt", 3)   # 128 bytes are used as they are


def test_input_sets_contain_what_they_claim():
    for bip39, second in ((False, KI.SALT_LENGTHS), (True, KI.PP_LENGTHS)):
        base = KI.operands(bip39, 0)
        lens = lambda items: [None if x is None else len(x) for x in items]
        pairs = {(p, s) for p, s in zip(lens(base["pws"]), lens(base["salts"]))}
        assert pairs >= set(itertools.product(KI.PW_LENGTHS, second))             # every password length meets every salt length
        assert lens(base["pws"]).count(None) == 1 == lens(base["salts"]).count(None)
        assert base["pws"][KI.PW_REVERSED] is None and base["salts"][KI.SALT_REVERSED] is None
        starts = {}
        for start in range(4):
            S = KI.operands(bip39, start)
            assert S["pws"] == base["pws"] and S["salts"] == base["salts"]        # the same elements at every start
            assert len(S["pw_off"]) == len(S["salt_off"]) == KI.N_SET + 1 and len(S["pw"]) % 4 == 0 == len(S["salt"]) % 4
            assert int(S["pw_off"][0]) == start and int(S["salt_off"][0]) == (start + 1) % 4
            for name, off, items in (("pw", S["pw_off"], S["pws"]), ("salt", S["salt_off"], S["salts"])):
                for i, x in enumerate(items):
                    if x is not None:
                        starts.setdefault((name, len(x)), set()).add(int(off[i]) & 3)
        for L in KI.PW_LENGTHS:
            assert starts[("pw", L)] == {0, 1, 2, 3}, L                             # every length at every alignment
        for L in second:
            assert starts[("salt", L)] == {0, 1, 2, 3}, L
        dk, err = KI.expected(bip39, 1)
        assert err[KI.PW_REVERSED] == err[KI.SALT_REVERSED] == KI.WIRE_BAD_LENGTH and np.count_nonzero(err) == 2
        assert not dk[err != 0].any() and dk[err == 0].any(axis=1).all()
    # the ends of U_1's message behind the ipad block, modulo the block
    assert sorted({(L + 4) % 128 for L in KI.SALT_LENGTHS}) == sorted({4, 5, 111, 112, 127, 0, 1, 126})
    assert {(L + 8 + 4) % 128 for L in KI.PP_LENGTHS[2:]} == {(L + 4) % 128 for L in KI.SALT_LENGTHS[2:]}
    assert KI.expected(True, 2048, "one_pw")[0][0].tobytes() == KI.bip39_seed(KI.operands(True)["pws"][0], KI.operands(True)["salts"][0])


# ---- the pieces -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prefix_len", [0, 8])
def test_absorber_against_hashlib_on_every_length_and_alignment(emu, prefix_len):
    """SHA-512(first || prefix || message || INT(index)) with each part present and absent.  The message sits between sentinel
    bytes (a READ outside the message's words is what the sanitizer program's exact allocations catch)."""
    prefix = bytes(range(0xF1, 0xF1 + prefix_len))
    pbuf = np.frombuffer(prefix + bytes(8 - prefix_len), np.uint8).copy()
    first = bytes((5 * k + 1) & 0xFF for k in range(128))
    index = 0x01C2B3A4
    for L in range(261):
        msg = KI._stream(f"absorb{L}", L)
        for al in range(4):
            buf = np.full(16 + al + L + 16, 0xEE, np.uint8)
            base = (-buf.ctypes.data) % 4 + 8 + al                        # the message starts at address = al (mod 4)
            buf[base:base + L] = np.frombuffer(msg, np.uint8)
            for head, indexed in ((None, 0), (first, 1), (first, 0), (None, 1)):
                out = filled(64)
                rc = emu.emukdf_absorb(head, _p(pbuf), C.c_uint(prefix_len), _p(buf), C.c_uint64(base), C.c_uint64(base + L), C.c_int(indexed),
                                       C.c_uint32(index), _p(out))
                want = hashlib.sha512((head or b"") + prefix + msg + (struct.pack(">I", index) if indexed else b"")).digest()
                assert rc == 0 and out.tobytes() == want, (prefix_len, L, al, head is not None, indexed)


def test_fixed_shape_compression_equals_the_general_one(emu):
    """sha512_compress_digest against hd.hpp's sha512_compress of the same block, and against the oracle's own compression"""
    rng = np.random.default_rng(39)
    edge = [np.zeros(8, np.uint64), np.full(8, 2**64 - 1, np.uint64), np.array(HI.SHA512_IV, np.uint64)]
    for k in range(200):
        st = edge[k % 3] if k < 9 else rng.integers(0, 2**64, 8, dtype=np.uint64)
        dg = edge[(k // 3) % 3] if k < 9 else rng.integers(0, 2**64, 8, dtype=np.uint64)
        a, b = st.copy(), st.copy()
        emu.emukdf_compress_digest(_p(a), _p(dg.copy()), C.c_int(0))
        emu.emukdf_compress_digest(_p(b), _p(dg.copy()), C.c_int(1))
        assert np.array_equal(a, b), k
        if k < 20:
            block = struct.pack(">8Q", *[int(v) for v in dg]) + b"\x80" + bytes(55) + struct.pack(">Q", 1536)
            assert tuple(int(v) for v in a) == tuple(HI.sha512_compress(tuple(int(v) for v in st), block)), k


@pytest.mark.parametrize("length", [0, 1, 64, 127, 128, 129, 257])
def test_key_states_of_short_and_long_keys(emu, length):
    key = KI._stream("key", length)
    for al in range(4):
        buf = np.full(8 + length + 8, 0xEE, np.uint8)
        base = (-buf.ctypes.data) % 4 + 4 + al
        buf[base:base + length] = np.frombuffer(key, np.uint8)
        got = np.zeros(16, np.uint64)
        assert emu.emukdf_key_states(_p(buf), C.c_uint64(base), C.c_uint64(base + length), _p(got)) == 0
        inner, outer = HI.hmac512_key_states(key if length <= 128 else hashlib.sha512(key).digest())
        assert tuple(int(v) for v in got[:8]) == inner and tuple(int(v) for v in got[8:]) == outer, (length, al)


# ---- the whole body, byte for byte ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dk_len", KI.DK_LENGTHS)
@pytest.mark.parametrize("iterations", KI.ITERATIONS)
def test_pbkdf2_body_equals_the_oracle(emu, iterations, dk_len):
    want_dk, want_err = KI.expected(False, iterations)
    S = KI.operands(False, 0)
    for n in (KI.LENGTHS if iterations < 2048 else (KI.N_SET,)):
        dk, err, bad = run_body(emu, 0, S, n, n, iterations, dk_len, n)
        assert_rows(dk, err, bad, want_dk, want_err, n, dk_len)


def test_bip39_body_equals_the_oracle_and_the_pin(emu):
    want_dk, want_err = KI.expected(True, KI.BIP39_ITERATIONS)
    n = KI.N_SET
    dk, err, bad = run_body(emu, 1, KI.operands(True, 0), n, n, KI.BIP39_ITERATIONS, 64, n)
    assert_rows(dk, err, bad, want_dk, want_err, n, 64)
    mn, mn_off = KI.pack([KI.PIN_MNEMONIC])
    pp, pp_off = KI.pack([KI.PIN_PASSPHRASE])
    dk, err, bad = run_body(emu, 1, {"pw": mn, "pw_off": mn_off, "salt": pp, "salt_off": pp_off}, 1, 1, KI.BIP39_ITERATIONS, 64, 1)
    assert bad == 0 and err[0] == 0 and dk[0].tobytes() == KI.PIN_SEED


@pytest.mark.parametrize("start", [1, 2, 3])
@pytest.mark.parametrize("bip39", [0, 1])
def test_every_start_alignment_of_both_buffers(emu, bip39, start):
    """the same elements moved by 1, 2 and 3 bytes (the salts by one more): the same bytes out.  Three iterations: what depends
    on the alignment is the absorption in front of the loop."""
    want_dk, want_err = KI.expected(bool(bip39), 3)
    n = KI.N_SET
    dk, err, bad = run_body(emu, bip39, KI.operands(bool(bip39), start), n, n, 3, 64, n)
    assert_rows(dk, err, bad, want_dk, want_err, n, 64)


@pytest.mark.parametrize("form", ["one_pw", "one_salt", "no_salt"])
@pytest.mark.parametrize("bip39", [0, 1])
def test_broadcast_forms(emu, bip39, form):
    """one password for every salt, one salt for every password; and no salt at all, which is the empty one"""
    iterations = KI.BIP39_ITERATIONS if bip39 else 3
    want_dk, want_err = KI.expected(bool(bip39), iterations, form)
    S = KI.operands(bool(bip39), 0)
    for n in (65, KI.N_SET) if not bip39 else (65,):
        dk, err, bad = run_body(emu, bip39, S, 1 if form == "one_pw" else n, 1 if form == "one_salt" else n, iterations, 64, n, form == "no_salt")
        assert_rows(dk, err, bad, want_dk, want_err, n, 64)
    assert np.count_nonzero(want_err) == 1                      # (the one reversed element of the operand that is not shared)


def vector_file(path, bip39, iterations, dk_len, n):
    """the first n elements of a set and the oracle's expectations in tests/emu_kdf/kdf_selftest.cpp's layout"""
    S = KI.operands(bool(bip39), 1)
    want_dk, want_err = KI.expected(bool(bip39), iterations)
    with open(path, "wb") as f:
        f.write(struct.pack("<6Q", bip39, n, len(S["pw"]), len(S["salt"]), iterations, dk_len))
        for a in (S["pw"], S["pw_off"][:n + 1], S["salt"], S["salt_off"][:n + 1], want_dk[:n, :dk_len], want_err[:n]):
            f.write(np.ascontiguousarray(a).tobytes())


def test_sanitizer_program_exits_zero(emu, tmp_path):
    """tests/emu_kdf/kdf_selftest under -fsanitize=address,undefined: the pin at 2048 iterations, then a set together and every
    element alone in allocations of exactly its own words.  A stand-alone program: nothing is loaded into this process."""
    prog = os.path.join(HERE, "kdf_selftest")
    for bip39, iterations, dk_len in ((0, 3, 64), (1, 2, 32)):
        path = tmp_path / f"kdf_vectors{bip39}.bin"
        vector_file(path, bip39, iterations, dk_len, KI.N_SET)
        res = subprocess.run([prog, str(path)], capture_output=True, text=True)
        assert res.returncode == 0, res.stdout + res.stderr
        assert f"the pin, {KI.N_SET} elements together and alone, 0 failures" in res.stdout
    with open(path, "r+b") as f:                                   # the program must be able to fail: one flipped expectation
        f.seek(-KI.N_SET - 40, os.SEEK_END)
        b = f.read(1)
        f.seek(-KI.N_SET - 40, os.SEEK_END)
        f.write(bytes([b[0] ^ 1]))
    assert subprocess.run([prog, str(path)], capture_output=True).returncode == 1


# ---- the entry points: declarations, refusals, nulls, overlap (BUFFER OVERLAP, include/p2e.h) ----------------------------------
OFFS, ERR = ("shared", 8, "n+1"), ("out", 1, "n")
FOUR = C.c_size_t(4)                                               # n_x = count (a size_t: ctypes would pass a bare int as 32 bits)
# One row per call: its arguments behind ctx, in the header's order (tests/test_overlap_cpu.py explains the entries)
CALLS = {
    "p2e_pbkdf2_hmac_sha512_batch": [[("free",), OFFS, FOUR, ("free",), OFFS, FOUR, C.c_uint32(2), C.c_size_t(64), ("out", 64, "n"), ("n",), ERR]],
    "p2e_bip39_seed_batch": [[("free",), OFFS, FOUR, ("free",), OFFS, FOUR, ("out", 64, "n"), ("n",), ERR]],
}
VALUES = {"p2e_pbkdf2_hmac_sha512_batch": {2: "n_passwords", 5: "n_salts", 6: "iterations", 7: "dk_len"},
          "p2e_bip39_seed_batch": {2: "n_mnemonics", 5: "n_passphrases"}}


class KdfCall(Call):
    """test_overlap_cpu.Call with the parameter names taken from header_calls(): per_element_calls() does not list a call
    whose batch size is not named n or m"""

    def __init__(self, name, row, n=4):
        self.name, self.row, self.n, self.n_parents = name, row, n, n
        self.pnames = [p for _t, p in header_calls()[name][1:]]
        self.arena = np.zeros(1024 * (len(row) + 2), np.uint8)
        self.slot = np.zeros(1, np.uint64)
        self.base = {k: self.arena.ctypes.data + 1024 * (k + 1) for k, spec in enumerate(row)
                     if isinstance(spec, tuple) and spec[0] in ("in", "out", "shared", "free")}


def with_value(name, pname, value):
    """the call's row with one of its plain values replaced"""
    row = list(CALLS[name][0])
    k = {v: k for k, v in VALUES[name].items()}[pname]
    row[k] = type(row[k])(value)
    return KdfCall(name, row)


def all_forms():
    for name, forms in CALLS.items():
        for row in forms:
            yield name, row


def test_the_two_declarations_exist_with_a_count_parameter():
    H = header_calls()
    for name, forms in CALLS.items():
        assert name in H and name in p2e.EXPORTS, name
        params = H[name]
        assert params[0][0].startswith("p2e_ctx") and "count" in [p for _t, p in params] and not {"n", "m"} & {p for _t, p in params}
        for row in forms:
            assert len(row) == len(params) - 1, name
            for k, (spec, (typ, pname)) in enumerate(zip(row, params[1:])):
                assert ("*" in typ) == (isinstance(spec, tuple) and spec[0] != "n"), (name, pname)
                if isinstance(spec, tuple) and spec[0] == "out":
                    assert "const" not in typ, (name, pname)
                if isinstance(spec, tuple) and spec[0] in ("shared", "free"):
                    assert "const" in typ, (name, pname)
                if spec == ("n",):
                    assert pname == "count"
                if k in VALUES[name]:
                    assert pname == VALUES[name][k]
    text = open(os.path.join(ROOT, "include", "p2e.h")).read()
    assert re.search(r"#define P2E_PBKDF2_MAX_ITERATIONS \(1u << 20\)", text) and p2e.PBKDF2_MAX_ITERATIONS == 1 << 20
    assert "no parameter here is named n or m" in text and "grows with `iterations`" in text and "which is why there is a cap" in text
    L = p2e.lib()
    assert all(getattr(L, name).restype is C.c_long for name in CALLS)
    assert p2e.WIRE_BAD_LENGTH == KI.WIRE_BAD_LENGTH


def test_disjoint_arguments_pass_the_check_and_meet_the_null_context():
    for name, row in all_forms():
        rc, msg = KdfCall(name, row).run(None)
        assert rc == -1 and msg == "null context", (name, msg)
    # one element for the whole batch, of either operand and of both
    for name, a, b in (("p2e_pbkdf2_hmac_sha512_batch", "n_passwords", "n_salts"), ("p2e_bip39_seed_batch", "n_mnemonics", "n_passphrases")):
        assert with_value(name, a, 1).run(None) == (-1, "null context")
        assert with_value(name, b, 1).run(None) == (-1, "null context")


def test_every_invalid_argument_is_refused_with_its_message():
    G, B = "p2e_pbkdf2_hmac_sha512_batch", "p2e_bip39_seed_batch"
    for name, pname, bad_values, text in (
            (G, "n_passwords", (0, 2, 3, 5, 2**40), "n_passwords must be 1 or count"),
            (G, "n_salts", (0, 2, 3, 5, 2**40), "n_salts must be 1 or count"),
            (G, "iterations", (0, (1 << 20) + 1, 2**32 - 1), "iterations must be 1 .. P2E_PBKDF2_MAX_ITERATIONS (2^20)"),
            (G, "dk_len", (0, 1, 2, 3, 6, 63, 68, 128, 2**40), "dk_len must be a multiple of 4 in 4 .. 64"),
            (B, "n_mnemonics", (0, 2, 3, 5), "n_mnemonics must be 1 or count"),
            (B, "n_passphrases", (2, 3, 5), "n_passphrases must be 0, 1 or count")):
        for v in bad_values:
            call = with_value(name, pname, v)
            assert call.run(None) == (-1, text), (name, pname, v)
            assert not call.arena.any()
    for v in (1, 1 << 20):                                         # the ends of the range are accepted
        assert with_value(G, "iterations", v).run(None) == (-1, "null context")
    for v in range(4, 65, 4):
        row = list(CALLS[G][0])
        row[7], row[8] = C.c_size_t(v), ("out", v, "n")
        assert KdfCall(G, row).run(None) == (-1, "null context"), v
    # n_passphrases == 0 goes with two null pointers, and with nothing else
    call = with_value(B, "n_passphrases", 0)
    pp, off = call.pnames.index("passphrase"), call.pnames.index("pp_offsets")
    assert call.run(None, {pp: 0, off: 0}) == (-1, "null context")
    for moved in ({pp: 0}, {off: 0}, {}):
        assert call.run(None, moved) == (-1, "n_passphrases == 0 goes with a null passphrase and null pp_offsets"), moved
    # a batch beyond one launch
    row = list(CALLS[G][0])
    call = KdfCall(G, row, n=2**31 + 1)
    call.row[2] = call.row[5] = C.c_size_t(1)
    assert call.run(None) == (-1, "batch too large for one launch")


def test_a_null_required_pointer_is_named_and_the_null_passphrase_is_accepted():
    required = 0
    for name, row in all_forms():
        call = KdfCall(name, row)
        for k in call.positions("shared", "out", "free"):
            pname = call.pnames[k]
            assert call.run(None) == (-1, "null context"), name
            rc, msg = call.run(None, {k: 0})
            assert rc == -1 and msg.startswith("null pointer ("), (name, pname, msg)
            assert pname in re.findall(r"\w+", msg.split(";")[0]), (name, pname, msg)
            required += 1
            assert not call.arena.any()
    assert required == 6 + 6
    # without passphrases the other four pointers are still required, and the text says which form this is
    call = with_value("p2e_bip39_seed_batch", "n_passphrases", 0)
    pp, off = call.pnames.index("passphrase"), call.pnames.index("pp_offsets")
    for k in call.positions("shared", "out", "free"):
        if k in (pp, off):
            continue
        rc, msg = call.run(None, {pp: 0, off: 0, k: 0})
        assert rc == -1 and msg.startswith("null pointer (") and "n_passphrases == 0" in msg and "passphrase and pp_offsets may be null" in msg, msg
        assert call.pnames[k] in re.findall(r"\w+", msg.split(";")[0])


def test_every_output_on_or_shifted_onto_an_input_is_refused(fake):
    """no in-place form: an output at an input's base is refused like one shifted onto it"""
    seen = 0
    for name, row in all_forms():
        call = KdfCall(name, row)
        for i in call.positions("shared"):
            bpe, _count = call.geometry(i)
            for o in call.positions("out"):
                for shift in (0, bpe, 1, -1):
                    _refused(call, fake, {o: call.base[i] + shift}, i, o)
                    seen += 1
        # the same with one element for the whole batch: its two offsets
        for pname in list(VALUES[name].values())[:2]:
            one = with_value(name, pname, 1)
            i = one.pnames.index(pname) - 1
            for o in one.positions("out"):
                _refused(one, fake, {o: one.base[i] + 8}, i, o)
                seen += 1
    assert seen == 2 * (2 * 2 * 4 + 2 * 2)


def test_every_pair_of_outputs_on_one_buffer_is_refused(fake):
    for name, row in all_forms():
        call = KdfCall(name, row)
        (a, b), = itertools.combinations(call.positions("out"), 2)
        _refused(call, fake, {b: call.base[a]}, a, b)
        _refused(call, fake, {b: call.base[a] + 63}, a, b)


def test_adjacent_buffers_are_no_overlap():
    for name, row in all_forms():
        call = KdfCall(name, row)
        for i in call.positions("shared"):
            bpe, count = call.geometry(i)
            for o in call.positions("out"):
                obpe, ocount = call.geometry(o)
                for at in (call.base[i] + bpe * count, call.base[i] - obpe * ocount):
                    rc, msg = call.run(None, {o: at})
                    assert rc == -1 and msg == "null context", (name, call.pnames[i], call.pnames[o], msg)


def test_host_staged_data_may_not_touch_an_output():
    """BUFFER OVERLAP 5: the extent of the variable-length operands is known on the host only where the offsets are (host
    pointers); nothing can be staged without a device (tests/test_gpu_kdf.py has the refusal itself).  Here the
    declaration-level facts: the check sits behind the argument checks, and count == 0 meets the context's null test too."""
    L = p2e.lib()
    buf, out = np.zeros(64, np.uint8), np.zeros(64, np.uint8)
    zero, one = C.c_size_t(0), C.c_size_t(1)
    assert L.p2e_bip39_seed_batch(None, _p(buf), _p(buf), zero, None, None, zero, _p(out), zero, _p(out)) == -1
    assert (L.p2e_last_error() or b"").decode() == "null context"
    assert L.p2e_pbkdf2_hmac_sha512_batch(None, _p(buf), _p(buf), one, _p(buf), _p(buf), one, C.c_uint32(1), C.c_size_t(4), _p(out), zero,
                                          _p(out)) == -1
    assert (L.p2e_last_error() or b"").decode() == "null context"


def test_pack_bytes_normalises_str_and_keeps_bytes():
    buf, off = p2e.pack_bytes(["á", "á", b"\xc3\xa1", "", "Å"])      # a + combining acute; a-acute; raw UTF-8; empty; Angstrom
    items = [buf[int(off[i]):int(off[i + 1])].tobytes() for i in range(5)]
    assert items == [b"a\xcc\x81", b"a\xcc\x81", b"\xc3\xa1", b"", b"A\xcc\x8a"]
    assert off.dtype == np.uint64 and buf.dtype == np.uint8 and len(buf) % 4 == 0 and len(buf) >= int(off[-1])
    buf, off = p2e.pack_bytes([])
    assert off.tolist() == [0] and len(buf) % 4 == 0


def test_example_compiles_against_the_header(tmp_path):
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                           os.path.join(ROOT, "examples", "mnemonic_scan.c"), "-o", str(tmp_path / "mnemonic_scan.o")])
