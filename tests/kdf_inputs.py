"""Oracle and input sets of the PBKDF2-HMAC-SHA512 / BIP-39 calls (include/p2e.h p2e_pbkdf2_hmac_sha512_batch,
p2e_bip39_seed_batch), shared by tests/test_kdf_cpu.py and tests/test_gpu_kdf.py.

The oracle is hashlib.pbkdf2_hmac("sha512", ...) and nothing under test.  It is trusted once it reproduces (check_oracle)
  - a PBKDF2 written out by hand from RFC 8018 5.2 with hmac and hashlib.sha512, on every pair of edge lengths below;
  - the pin: the seed of "abandon ... about" under the passphrase TREZOR.  If a published vector ever disagrees with hashlib,
    hashlib wins.

Sets of 257 elements, nothing between two elements, lengths cycling through the edge lists so that every pair of a password
length and a salt length occurs (80 pairs in 257 elements).
  password lengths     0, 1, 111, 112, 127, 128, 129, 239, 240, 257: 128 is the longest key used as it is, 129 is hashed first;
                       111 / 112 and 239 / 240 straddle the padding boundary of that hash (one block or two, two or three).
  salt lengths         0, 1, 107, 108, 123, 124, 125, 250: with the four bytes of INT(1) the message of U_1's inner hash ends
                       at 111, 112, 127, 128, 129 (mod 128) bytes behind the ipad block.
  passphrase lengths   the salt lengths less the eight bytes of "mnemonic", which put the same ends behind the prefix: 99, 100,
                       115, 116, 117, 242 -- and 0 and 1 as they are (a length cannot go below zero).
`start` bytes of filler stand in front of the first element, so that with start = 0 .. 3 every element meets every address
alignment; several of the lengths are odd, so the elements of one set differ in alignment among themselves as well.
One element of each operand has its offsets reversed: WIRE_BAD_LENGTH, all-zero output, counted."""
import functools
import hashlib
import hmac

import numpy as np

WIRE_OK, WIRE_BAD_LENGTH = 0, 1
N_SET = 257
LENGTHS = (0, 1, 63, 64, 65, 257)     # batch sizes: nothing, one lane, a wave less one, a wave, a wave plus one, a block plus one
PW_LENGTHS = (0, 1, 111, 112, 127, 128, 129, 239, 240, 257)
SALT_LENGTHS = (0, 1, 107, 108, 123, 124, 125, 250)
PP_LENGTHS = (0, 1, 99, 100, 115, 116, 117, 242)
ITERATIONS = (1, 2, 3, 2048)
DK_LENGTHS = (4, 32, 64)
BIP39_ITERATIONS = 2048
PW_REVERSED, SALT_REVERSED = 40, 150        # the elements whose password / salt offsets run backwards
LONG_PW = 6                                 # an element with a 129-byte password (PW_LENGTHS[6]), used by the digest-as-key check

PIN_MNEMONIC = b"abandon abandon abandon abandon abandon abandon abandon abandon abandon abandon abandon about"
PIN_PASSPHRASE = b"TREZOR"
PIN_SEED = bytes.fromhex("c55257c360c07c72029aebc1b53c05ed0362ada38ead3e3e9efa3708e53495531f09a6987599d18264c1e1c92f2cf141"
                         "630c7a3c4ab7c81b2f001698e7463b04")


def pbkdf2(password, salt, iterations, dk_len=64):
    """the oracle"""
    return hashlib.pbkdf2_hmac("sha512", password, salt, iterations, dk_len)


def bip39_seed(mnemonic, passphrase=b""):
    return pbkdf2(mnemonic, b"mnemonic" + passphrase, BIP39_ITERATIONS, 64)


def pbkdf2_by_hand(password, salt, iterations, dk_len=64):
    """RFC 8018 5.2 for one block, written out: U_1 = PRF(P, S || INT(1)), U_j = PRF(P, U_{j-1}), T = U_1 ^ ... ^ U_c"""
    prf = lambda data: hmac.new(password, data, hashlib.sha512).digest()
    u = prf(salt + (1).to_bytes(4, "big"))
    t = int.from_bytes(u, "big")
    for _ in range(iterations - 1):
        u = prf(u)
        t ^= int.from_bytes(u, "big")
    return t.to_bytes(64, "big")[:dk_len]


def _stream(label, length):
    out, k = b"", 0
    while len(out) < length:
        out += hashlib.sha256(f"kdf-inputs/{label}/{k}".encode()).digest()
        k += 1
    return out[:length]


@functools.lru_cache(maxsize=None)
def check_oracle():
    """-> the number of answers compared"""
    seen = 0
    for pl in PW_LENGTHS:
        for sl in SALT_LENGTHS + PP_LENGTHS:
            pw, salt = _stream("check-pw", pl), _stream("check-salt", sl)
            for it in (1, 2, 3):
                assert pbkdf2(pw, salt, it) == pbkdf2_by_hand(pw, salt, it), (pl, sl, it)
                seen += 1
    assert pbkdf2(PIN_MNEMONIC, b"mnemonic" + PIN_PASSPHRASE, 2048) == pbkdf2_by_hand(PIN_MNEMONIC, b"mnemonic" + PIN_PASSPHRASE, 2048)
    assert bip39_seed(PIN_MNEMONIC, PIN_PASSPHRASE) == PIN_SEED
    return seen + 2


def pack(items, start=0, reversed_at=None):
    """(data uint8, offsets uint64) as the calls take them, `start` filler bytes in front; data is padded to whole words behind
    its last element (a lane reads aligned words; the padding is never used).  reversed_at: that element's end is put three
    bytes below its start, so the next element begins three bytes early (its bytes are those of the buffer)."""
    offsets = np.zeros(len(items) + 1, np.uint64)
    offsets[:] = start + np.concatenate([[0], np.cumsum([len(x) for x in items])])
    raw = bytes([0xC3]) * start + b"".join(items)
    data = np.zeros((len(raw) + 3) // 4 * 4 + 4, np.uint8)
    data[:len(raw)] = np.frombuffer(raw, np.uint8)
    data[len(raw):] = 0x3C
    if reversed_at is not None:
        assert int(offsets[reversed_at]) >= 3
        offsets[reversed_at + 1] = offsets[reversed_at] - 3
    return data, offsets


def elements(data, offsets):
    """what each element of (data, offsets) is: its bytes, or None where the pair is reversed"""
    out = []
    for i in range(len(offsets) - 1):
        lo, hi = int(offsets[i]), int(offsets[i + 1])
        out.append(None if hi < lo else data[lo:hi].tobytes())
    return out


def _lengths(i, second):
    return PW_LENGTHS[i % len(PW_LENGTHS)], second[(i // len(PW_LENGTHS)) % len(second)]


@functools.lru_cache(maxsize=None)
def operands(bip39, start=0):
    """{'pw', 'pw_off', 'salt', 'salt_off'} of one set, and 'pws' / 'salts': each element's bytes (None: reversed).  The bytes
    do not depend on `start` but for the two elements behind a reversed one, which begin three bytes early."""
    second = PP_LENGTHS if bip39 else SALT_LENGTHS
    kind = "bip39" if bip39 else "general"
    pws = [_stream(f"{kind}-pw-{i}", _lengths(i, second)[0]) for i in range(N_SET)]
    salts = [_stream(f"{kind}-salt-{i}", _lengths(i, second)[1]) for i in range(N_SET)]
    pw, pw_off = pack(pws, start, PW_REVERSED)
    salt, salt_off = pack(salts, (start + 1) % 4, SALT_REVERSED)
    return {"pw": pw, "pw_off": pw_off, "salt": salt, "salt_off": salt_off, "pws": elements(pw, pw_off), "salts": elements(salt, salt_off)}


@functools.lru_cache(maxsize=None)
def expected(bip39, iterations, form="each"):
    """(dk (257, 64), err (257,)) of the set under `form`: 'each' = password i with salt i, 'one_pw' = password 0 with salt i,
    'one_salt' = password i with salt 0, 'no_salt' = password i with the empty salt (BIP-39's absent passphrase).  A shorter
    dk_len is a prefix of these rows.  The elements are the same bytes at every `start` (asserted by the tests), so there is
    one answer per (set, iterations, form): computed once and never changed."""
    S = operands(bip39, 0)
    dk, err = np.zeros((N_SET, 64), np.uint8), np.zeros(N_SET, np.uint8)
    for i in range(N_SET):
        pw = S["pws"][0 if form == "one_pw" else i]
        salt = b"" if form == "no_salt" else S["salts"][0 if form == "one_salt" else i]
        if pw is None or salt is None:
            err[i] = WIRE_BAD_LENGTH
            continue
        dk[i] = np.frombuffer(pbkdf2(pw, (b"mnemonic" if bip39 else b"") + salt, iterations), np.uint8)
    dk.setflags(write=False), err.setflags(write=False)
    return dk, err
