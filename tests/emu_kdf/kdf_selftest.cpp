// Stand-alone run of the PBKDF2 / BIP-39 bodies under the address and undefined-behaviour sanitizers.  argv[1] is a file
// tests/test_kdf_cpu.py writes from tests/kdf_inputs.py: one input set with the oracle's expectations.
//   u64 bip39, n, pw_bytes, salt_bytes, iterations, dk_len
//   pw[pw_bytes] pw_offsets[8 (n + 1)] salt[salt_bytes] salt_offsets[8 (n + 1)] | dk[dk_len n] err[n]
// The set runs once as it is, every buffer in a heap allocation of its own size (pw_bytes and salt_bytes are whole words:
// a lane reads aligned words), and then element by element: each password and each salt ALONE in an allocation of exactly
// the aligned words that hold its bytes, at its own address alignment, each output row in an allocation of its own size.  A
// lane that read a word outside its element, or wrote outside its row, would stop the program.  Every byte is compared.
// The pin (the seed of "abandon ... about" under TREZOR) is checked before the file is opened.  Exit status 0 = all held.
#include <cstdio>
#include <cstring>
#include <vector>

#include "p2e_emu_kdf.cpp"

namespace {
typedef std::vector<uint8_t> Bytes;
FILE* g_file = nullptr;
bool g_ok = true;
Bytes take(size_t count) {
    Bytes b(count, 0);
    if (count && fread(b.data(), 1, count, g_file) != count) g_ok = false;
    return b;
}
std::vector<uint64_t> take_u64(size_t count) {
    std::vector<uint64_t> v(count, 0);
    if (count && fread(v.data(), 8, count, g_file) != count) g_ok = false;
    return v;
}
// element [lo, hi) of `data` alone: the words that hold it and nothing else, its first byte at the same address modulo 4
struct Alone {
    Bytes buf;
    uint64_t off[2];
};
Alone alone(const Bytes& data, uint64_t lo, uint64_t hi) {
    Alone a;
    if (hi < lo) {   // a reversed pair stays one; no byte belongs to it
        a.buf.assign(4, 0xEE);
        a.off[0] = 3, a.off[1] = 0;
        return a;
    }
    const uint64_t at = lo % 4, len = hi - lo;
    a.buf.assign(len ? (at + len + 3) / 4 * 4 : 4, 0xEE);
    if (len) memcpy(a.buf.data() + at, data.data() + lo, len);
    a.off[0] = at, a.off[1] = at + len;
    return a;
}

int pin() {
    const char* words = "abandon abandon abandon abandon abandon abandon abandon abandon abandon abandon abandon about";
    const uint8_t want[64] = {0xc5, 0x52, 0x57, 0xc3, 0x60, 0xc0, 0x7c, 0x72, 0x02, 0x9a, 0xeb, 0xc1, 0xb5, 0x3c, 0x05, 0xed,
                              0x03, 0x62, 0xad, 0xa3, 0x8e, 0xad, 0x3e, 0x3e, 0x9e, 0xfa, 0x37, 0x08, 0xe5, 0x34, 0x95, 0x53,
                              0x1f, 0x09, 0xa6, 0x98, 0x75, 0x99, 0xd1, 0x82, 0x64, 0xc1, 0xe1, 0xc9, 0x2f, 0x2c, 0xf1, 0x41,
                              0x63, 0x0c, 0x7a, 0x3c, 0x4a, 0xb7, 0xc8, 0x1b, 0x2f, 0x00, 0x16, 0x98, 0xe7, 0x46, 0x3b, 0x04};
    const size_t len = strlen(words);
    Bytes mn((len + 3) / 4 * 4, 0), pp(8, 0), seed(64, 0xAA), err(1, 0xAA);
    memcpy(mn.data(), words, len);
    memcpy(pp.data(), "TREZOR", 6);
    const uint64_t mo[2] = {0, len}, po[2] = {0, 6};
    const long bad = emukdf_pbkdf2(1, mn.data(), mo, 1, pp.data(), po, 1, 2048, 64, seed.data(), 1, err.data());
    if (bad != 0 || err[0] != 0 || memcmp(seed.data(), want, 64)) {
        fprintf(stderr, "FAIL the pin: abandon ... about / TREZOR\n");
        return 1;
    }
    return 0;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: kdf_selftest VECTORS\n");
        return 2;
    }
    int fails = pin();
    g_file = fopen(argv[1], "rb");
    uint64_t hdr[6] = {0, 0, 0, 0, 0, 0};
    if (!g_file || fread(hdr, 8, 6, g_file) != 6 || hdr[0] > 1 || hdr[1] < 1 || hdr[1] > 4096 || hdr[2] > (1u << 24) || hdr[2] % 4 ||
        hdr[3] > (1u << 24) || hdr[3] % 4 || hdr[4] < 1 || hdr[4] > 4096 || hdr[5] < 4 || hdr[5] > 64 || hdr[5] % 4) {
        fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    const int bip39 = (int)hdr[0];
    const size_t n = hdr[1], dk_len = hdr[5];
    const uint32_t iterations = (uint32_t)hdr[4];
    const Bytes pw = take(hdr[2]);
    const std::vector<uint64_t> pw_off = take_u64(n + 1);
    const Bytes salt = take(hdr[3]);
    const std::vector<uint64_t> salt_off = take_u64(n + 1);
    const Bytes want_dk = take(dk_len * n), want_err = take(n);
    if (!g_ok || fgetc(g_file) != EOF) {
        fprintf(stderr, "%s is not a vector file of this layout\n", argv[1]);
        return 2;
    }
    fclose(g_file);

    long flagged = 0;
    for (size_t i = 0; i < n; i++) flagged += want_err[i] != 0;
    {   // the whole set
        Bytes dk(dk_len * n, 0xAA), err(n, 0xAA);
        const long bad = emukdf_pbkdf2(bip39, pw.data(), pw_off.data(), n, salt.data(), salt_off.data(), n, iterations, dk_len, dk.data(), n, err.data());
        if (bad != flagged || dk != want_dk || err != want_err) fprintf(stderr, "FAIL the whole set (%ld flagged, %ld expected)\n", bad, flagged), fails++;
    }
    for (size_t i = 0; i < n; i++) {   // every element alone
        const Alone p = alone(pw, pw_off[i], pw_off[i + 1]), s = alone(salt, salt_off[i], salt_off[i + 1]);
        Bytes dk(dk_len, 0xAA), err(1, 0xAA);
        const long bad = emukdf_pbkdf2(bip39, p.buf.data(), p.off, 1, s.buf.data(), s.off, 1, iterations, dk_len, dk.data(), 1, err.data());
        if (bad != (want_err[i] != 0) || err[0] != want_err[i] || memcmp(dk.data(), want_dk.data() + dk_len * i, dk_len)) {
            fprintf(stderr, "FAIL element %zu alone\n", i);
            fails++;
        }
    }
    {   // the absent salt: no pointer to follow
        const Alone p = alone(pw, pw_off[0], pw_off[1]);
        Bytes a(dk_len, 0xAA), b(dk_len, 0xAA), err(1, 0xAA);
        const uint64_t none[2] = {0, 0};
        Bytes four(4, 0xEE);
        emukdf_pbkdf2(bip39, p.buf.data(), p.off, 1, nullptr, nullptr, 0, iterations, dk_len, a.data(), 1, err.data());
        emukdf_pbkdf2(bip39, p.buf.data(), p.off, 1, four.data(), none, 1, iterations, dk_len, b.data(), 1, err.data());
        if (a != b || err[0] != 0) fprintf(stderr, "FAIL the absent salt differs from the empty one\n"), fails++;
    }
    printf("kdf_selftest: the pin, %zu elements together and alone, %d failures\n", n, fails);
    return fails ? 1 : 0;
}
