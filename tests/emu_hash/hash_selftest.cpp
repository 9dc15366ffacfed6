// Stand-alone run of the hashing, nonce and address bodies under the address and undefined-behaviour sanitizers.
//   1. published answers: sha256("abc"), keccak256(""), keccak256("abc"), the RFC 6979 A.2.5 nonces of "sample" and "test"
//      (P-256), the secp256k1 nonce of sk = 1 over sha256("Satoshi Nakamoto"), the address of 1 G;
//   2. the read bounds: a buffer of messages of every length 0 .. 300 is hashed from a heap block that begins at the
//      aligned word holding the first byte and ends with the aligned word holding the last byte, at every misalignment
//      0 .. 3 of the first byte -- a read of any word outside those is a heap-buffer-overflow report -- and each digest
//      must equal the digest of the same message alone in a block of its own (three algorithms, both output forms);
//   3. the retry branch: 200 inputs under the order 2^255 + 1; every nonce lies in [1, q), 102 inputs refuse at least one
//      candidate and the deepest refuses 7 (the values themselves are compared with Python in tests/test_hash_cpu.py).
// Exit status 0 = all held.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "p2e_emu_hash.cpp"

namespace {
int fails = 0;
void fail(const char* what, long a = -1, long b = -1) {
    if (fails++ < 10) fprintf(stderr, "hash_selftest: %s (%ld, %ld)\n", what, a, b);
}
std::string hex(const uint8_t* p, size_t n) {
    static const char* d = "0123456789abcdef";
    std::string s;
    for (size_t i = 0; i < n; i++) s += d[p[i] >> 4], s += d[p[i] & 15];
    return s;
}
// big-endian hex of a 32-byte little-endian value
std::string hex_le(const uint8_t* p) {
    uint8_t r[32];
    for (int i = 0; i < 32; i++) r[i] = p[31 - i];
    return hex(r, 32);
}
void from_hex_le(const char* h, uint8_t* out) {   // 64 hex digits, big-endian -> 32 bytes little-endian
    for (int i = 0; i < 32; i++) {
        unsigned v;
        sscanf(h + 2 * i, "%2x", &v);
        out[31 - i] = (uint8_t)v;
    }
}
// digest of one message, read from a heap block of exactly the words that hold it, first byte at misalignment `mis`
std::string digest(int alg, unsigned form, const uint8_t* msg, size_t len, unsigned mis = 0) {
    // (the allocator rounds sizes up: the block sits at the END of the allocation, so its last word is the last one)
    const size_t block = (mis + len + 3) / 4 * 4, total = block ? (block + 15) / 16 * 16 : 16;
    uint8_t* raw = (uint8_t*)aligned_alloc(16, total);
    uint8_t* base = raw + (total - block);
    if (len) memcpy(base + mis, msg, len);
    const uint64_t off[2] = {0, len};
    alignas(4) uint8_t out[32];
    emuh_hash(alg, form, base + mis, off, out, 1);
    free(raw);
    return hex(out, 32);
}
void answers() {
    const uint8_t* abc = (const uint8_t*)"abc";
    if (digest(0, 0, abc, 3) != "ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad") fail("sha256(abc)");
    if (digest(2, 0, abc, 0) != "c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470") fail("keccak256()");
    if (digest(2, 0, abc, 3) != "4e03657aea45a94fc7d47ba826c8d667c0d1e6e33a64a036ec44f58fa12d6c45") fail("keccak256(abc)");
    // RFC 6979 A.2.5
    alignas(4) uint8_t x[32], z[32], k[32];
    from_hex_le("C9AFA9D845BA75166B5C215767B1D6934E50C3DB36E89B127B8A622B120F6721", x);
    const char* msgs[2] = {"sample", "test"};
    const char* want[2] = {"a6e3c57dd01abe90086538398355dd4c3b17aa873382b0f24d6129493d8aad60",
                           "d16b6ae827f17175e040871a1c7ec3500192c4c92677336ec2537acaee0008e0"};
    for (int t = 0; t < 2; t++) {
        const uint64_t off[2] = {0, strlen(msgs[t])};
        std::vector<uint8_t> m(8, 0);
        memcpy(m.data(), msgs[t], off[1]);
        emuh_hash(0, DIGEST_SCALAR, m.data(), off, z, 1);
        emuh_nonce(1, z, x, k, 1);
        if (hex_le(k) != want[t]) fail("RFC 6979 A.2.5 nonce", t);
    }
    {
        const char* s = "Satoshi Nakamoto";
        const uint64_t off[2] = {0, strlen(s)};
        std::vector<uint8_t> m(off[1]);
        memcpy(m.data(), s, off[1]);
        emuh_hash(0, DIGEST_SCALAR, m.data(), off, z, 1);
        memset(x, 0, 32);
        x[0] = 1;
        emuh_nonce(0, z, x, k, 1);
        if (hex_le(k) != "8f8a276c19f4149656b280621e358cce24f5f52542772691ee69063b74f15d15") fail("secp256k1 nonce of sk = 1");
    }
    alignas(4) uint8_t gx[32], gy[32], addr[40];
    from_hex_le("79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798", gx);
    from_hex_le("483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8", gy);
    emuh_eth_address(gx, gy, nullptr, addr, 1);
    if (hex(addr, 20) != "7e5f4552091a69125d5dfcb7b8c2659029395bdf") fail("address of 1 G");
    const uint8_t flag[1] = {4};
    memset(addr, 0xAA, 40);
    emuh_eth_address(gx, gy, flag, addr, 1);
    for (int i = 0; i < 20; i++)
        if (addr[i]) fail("flagged address not zero", i);
    if (addr[20] != 0xAA) fail("address call wrote past its 20 bytes");
}
void bounds() {
    const size_t L = 301;
    std::vector<uint8_t> all;
    std::vector<uint64_t> off(1, 0);
    uint32_t x = 12345;
    for (size_t len = 0; len < L; len++) {
        for (size_t j = 0; j < len; j++) all.push_back((uint8_t)((x = x * 1664525u + 1013904223u) >> 24));
        off.push_back(all.size());
    }
    for (int alg = 0; alg < 3; alg++)
        for (unsigned form = 0; form < 2; form++) {
            std::vector<std::string> alone(L);
            for (size_t len = 0; len < L; len++) alone[len] = digest(alg, form, all.data() + off[len], len, (unsigned)(len & 3));
            for (unsigned mis = 0; mis < 4; mis++) {
                const size_t block = (mis + all.size() + 3) / 4 * 4, total = (block + 15) / 16 * 16;
                uint8_t* raw = (uint8_t*)aligned_alloc(16, total);
                uint8_t* base = raw + (total - block);
                memcpy(base + mis, all.data(), all.size());
                std::vector<uint8_t> out(32 * L + 32, 0xAA);
                if (emuh_hash(alg, form, base + mis, off.data(), out.data(), L) != 0) fail("count of a monotonic batch");
                free(raw);
                for (size_t len = 0; len < L; len++)
                    if (hex(out.data() + 32 * len, 32) != alone[len]) fail("digest depends on the position", alg, (long)len);
                for (int j = 0; j < 32; j++)
                    if (out[32 * L + j] != 0xAA) fail("wrote past out32");
            }
        }
    // non-monotonic offsets: the empty message, counted
    const uint64_t bad_off[4] = {10, 5, 5, 2};
    alignas(4) uint8_t out[96];
    if (emuh_hash(0, 0, all.data(), bad_off, out, 3) != 2) fail("count of non-monotonic offsets");
    if (hex(out, 32) != digest(0, 0, all.data(), 0) || hex(out + 64, 32) != digest(0, 0, all.data(), 0)) fail("non-monotonic element is not the empty digest");
}
void retries() {
    const size_t n = 200;
    std::vector<uint8_t> q(32, 0), xs(32 * n, 0), zs(32 * n), ks(32 * n);
    std::vector<uint32_t> rej(n, 0xAAAAAAAAu);
    q[0] = 1, q[31] = 0x80;
    for (size_t i = 0; i < n; i++) {
        const uint32_t v = (uint32_t)i + 1;
        memcpy(&xs[32 * i], &v, 4);
        const uint8_t b = (uint8_t)i;
        const uint64_t off[2] = {0, 1};
        alignas(4) uint8_t m[4] = {b, 0, 0, 0};
        emuh_hash(0, DIGEST_SCALAR, m, off, &zs[32 * i], 1);
    }
    emuh_nonce_order(q.data(), xs.data(), zs.data(), ks.data(), rej.data(), n);
    uint32_t deepest = 0, some = 0;
    for (size_t i = 0; i < n; i++) {
        deepest = rej[i] > deepest ? rej[i] : deepest;
        some += rej[i] != 0;
        const U256 k = hash_load_packed(ks.data(), i);
        if (u256_is_zero(k) || (k.w[7] >> 31 && (k.w[7] != 0x80000000u || k.w[0] || k.w[1] || k.w[2] || k.w[3] || k.w[4] || k.w[5] || k.w[6])))
            fail("nonce outside [1, q)", (long)i);
    }
    if (some != 102 || deepest != 7) fail("retry statistics of the synthetic order", some, deepest);
}
}  // namespace

int main() {
    answers();
    bounds();
    retries();
    printf("hash_selftest: %d failures\n", fails);
    return fails ? 1 : 0;
}
