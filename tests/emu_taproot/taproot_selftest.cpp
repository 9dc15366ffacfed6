// Stand-alone run of the Taproot bodies under the address and undefined-behaviour sanitizers (and the limb-bound tracker).
// The three pins of tests/taproot_inputs.py (BIP-341's wallet vectors) are checked first, from the strings below.  argv[1] is a
// file tests/test_taproot_cpu.py writes: the script set (every edge length at every alignment) with the oracle's leaf hashes.
//   u64 n, data_bytes
//   version[n] data[data_bytes] offsets[8 (n + 1)] | leaf[32 n] err[n]
// The set is hashed once in its one buffer, then every script alone in a heap allocation that holds nothing but the aligned
// words of that script (its misalignment kept): a lane that read a word in front of or behind its script would stop the
// program.  Exit status 0 = all held.
#include <cstdio>
#include <cstring>
#include <string>

#include "p2e_emu_taproot.cpp"

namespace {
typedef std::vector<uint8_t> Bytes;
FILE* g_file = nullptr;
bool g_ok = true;
Bytes take(size_t count, size_t round = 1) {
    Bytes b((count + round - 1) / round * round, 0);
    if (count && fread(b.data(), 1, count, g_file) != count) g_ok = false;
    return b;
}
Bytes hex(const char* s) {
    Bytes b;
    for (size_t k = 0; s[k] && s[k + 1]; k += 2) b.push_back((uint8_t)std::stoul(std::string(s + k, 2), nullptr, 16));
    return b;
}
int differ(const char* what, const Bytes& got, const Bytes& want) {
    if (got == want) return 0;
    size_t at = 0;
    while (at < got.size() && at < want.size() && got[at] == want[at]) at++;
    fprintf(stderr, "FAIL %s: first difference at byte %zu\n", what, at);
    return 1;
}
Bytes leaf_of(uint8_t version, const Bytes& script, uint8_t want_err = 0) {
    Bytes buf = script, out(32, 0xAA), err(1, 0xAA);
    buf.resize((script.size() + 3) / 4 * 4);
    const uint64_t offsets[2] = {0, script.size()};
    emutr_leaf_hash(&version, buf.data(), offsets, out.data(), 1, err.data());
    if (err[0] != want_err) out.assign(32, 0xEE);
    return out;
}

struct Pin {
    const char *internal, *root, *output;
    int leaves;
    uint8_t version[2];
    const char *script[2], *leaf[2];
};
const Pin PINS[3] = {
    {"d6889cb081036e0faefa3a35157ad71086b123b2b144b649798b494c300a961d", nullptr,
     "53a1f6e454df1aa2776a2814a721372d6258050de330b3c6d10ee8f4e0dda343", 0, {0, 0}, {nullptr, nullptr}, {nullptr, nullptr}},
    {"187791b6f712a8ea41c8ecdd0ee77fab3e85263b37e1ec18a3651926b3a6cf27", "5b75adecf53548f3ec6ad7d78383bf84cc57b55a3127c72b9a2481752dd88b21",
     "147c9c57132f6e7ecddba9800bb0c4449251c92a1e60371ee77557b6620f3ea3", 1, {0xC0, 0},
     {"20d85a959b0290bf19bb89ed43c916be835475d013da4b362117393e25a48229b8ac", nullptr},
     {"5b75adecf53548f3ec6ad7d78383bf84cc57b55a3127c72b9a2481752dd88b21", nullptr}},
    {"93478e9488f956df2396be2ce6c5cced75f900dfa18e7dabd2428aae78451820", "6c2dc106ab816b73f9d07e3cd1ef2c8c1256f519748e0813e4edd2405d277bef",
     "fb5c2771a52e84a51e097346361d30cab666fc34416e4b9f72a843e636f8d110", 2, {0xC0, 0xFA},
     {"20387671353e273264c495656e27e39ba899ea8fee3bb69fb2a680e22093447d48ac", "06424950333431"},
     {"8ad69ec7cf41c2a4001fd1f738bf1e505ce2277acdcaa63fe4765192497f47a7", "f224a923cd0021ab202ab139cc56802ddb92dcfc172b9212261a539df79a112a"}},
};

int pins() {
    int fails = 0;
    for (const Pin& p : PINS) {
        Bytes leaf[2];
        for (int k = 0; k < p.leaves; k++) {
            leaf[k] = leaf_of(p.version[k], hex(p.script[k]));
            fails += differ("pin: leaf hash", leaf[k], hex(p.leaf[k]));
        }
        Bytes root;
        if (p.leaves) {
            // the root from either leaf (depth = leaves - 1), on a path array of max_depth 1
            for (int k = 0; k < p.leaves; k++) {
                const Bytes path = p.leaves == 2 ? leaf[1 - k] : Bytes(32, 0x55);
                const uint8_t depth = (uint8_t)(p.leaves - 1);
                Bytes r(32, 0xAA), err(1, 0xAA);
                emutr_merkle_root(leaf[k].data(), path.data(), &depth, 1, r.data(), 1, err.data());
                fails += differ("pin: root", r, hex(p.root)) + (err[0] != 0);
                root = r;
            }
        }
        const Bytes pk = hex(p.internal);
        Bytes out(32, 0xAA), par(1, 0xAA), err(1, 0xAA);
        emutr_tweak_pubkey(pk.data(), p.leaves ? root.data() : nullptr, out.data(), par.data(), 1, err.data());
        fails += differ("pin: output key", out, hex(p.output));
        if (err[0] != 0 || par[0] != 1) fprintf(stderr, "FAIL pin: parity or code\n"), fails++;
        for (int k = 0; k < p.leaves; k++) {
            const Bytes path = p.leaves == 2 ? leaf[1 - k] : Bytes(32, 0x55);
            const uint8_t depth = (uint8_t)(p.leaves - 1);
            Bytes v(1, 0xAA), e(1, 0xAA);
            emutr_verify_commitment(out.data(), par.data(), pk.data(), leaf[k].data(), path.data(), &depth, 1, 1, e.data(), v.data());
            if (e[0] != 0 || v[0] != 1) fprintf(stderr, "FAIL pin: commitment of leaf %d\n", k), fails++;
            Bytes wrong = par;
            wrong[0] ^= 1;
            emutr_verify_commitment(out.data(), wrong.data(), pk.data(), leaf[k].data(), path.data(), &depth, 1, 1, e.data(), v.data());
            if (e[0] != 0 || v[0] != 0) fprintf(stderr, "FAIL pin: commitment under the wrong parity\n"), fails++;
        }
    }
    // the secret side: the tweaked key of d is the key of the tweaked point, for a point of either parity
    for (uint8_t d = 1; d <= 8; d++) {
        Bytes sk(32, 0), root(32, d), pk(32, 0xAA), out_sk(32, 0xAA), out_pk(32, 0xAA), want(32, 0xAA), par(1, 0xAA), err(1, 0xAA);
        sk[31] = d;
        const Aff* T = gen_table();
        if (body_schnorr_public_key(T, sk.data(), pk.data(), 0)) fails++;
        emutr_tweak_seckey(sk.data(), root.data(), out_sk.data(), 1, err.data());
        if (err[0] || body_schnorr_public_key(T, out_sk.data(), out_pk.data(), 0)) fails++;
        emutr_tweak_pubkey(pk.data(), root.data(), want.data(), par.data(), 1, err.data());
        fails += differ("tweaked secret key against tweaked public key", out_pk, want) + (err[0] != 0);
    }
    return fails;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: taproot_selftest VECTORS\n");
        return 2;
    }
    int fails = pins();
    g_file = fopen(argv[1], "rb");
    uint64_t hdr[2] = {0, 0};
    if (!g_file || fread(hdr, 8, 2, g_file) != 2 || hdr[0] < 1 || hdr[0] > 4096 || hdr[1] > (1u << 24)) {
        fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    const size_t n = hdr[0], data_bytes = hdr[1];
    const Bytes version = take(n), data = take(data_bytes, 4), off_bytes = take(8 * (n + 1)), w_leaf = take(32 * n), w_err = take(n);
    const bool at_end = fgetc(g_file) == EOF;
    fclose(g_file);
    if (!g_ok || !at_end) {
        fprintf(stderr, "%s is not a vector file of this program\n", argv[1]);
        return 2;
    }
    std::vector<uint64_t> offsets(n + 1);
    memcpy(offsets.data(), off_bytes.data(), 8 * (n + 1));
    {
        Bytes leaf(32 * n, 0xAA), err(n, 0xAA);
        emutr_leaf_hash(version.data(), data.data(), offsets.data(), leaf.data(), n, err.data());
        fails += differ("leaf hashes of the set", leaf, w_leaf) + differ("leaf codes of the set", err, w_err);
    }
    size_t alone = 0;
    for (size_t i = 0; i < n; i++) {
        if (offsets[i + 1] < offsets[i] || offsets[i + 1] > data_bytes) continue;
        const size_t len = offsets[i + 1] - offsets[i], al = offsets[i] & 3;
        Bytes own((al + len + 3) / 4 * 4, 0);
        if (len) memcpy(own.data() + al, data.data() + offsets[i], len);
        const uint64_t o[2] = {al, al + len};
        Bytes leaf(32, 0xAA), err(1, 0xAA);
        emutr_leaf_hash(&version[i], own.data(), o, leaf.data(), 1, err.data());
        if (err[0] != w_err[i] || memcmp(leaf.data(), w_leaf.data() + 32 * i, 32)) fprintf(stderr, "FAIL script %zu alone\n", i), fails++;
        alone++;
    }
    if (fails) return 1;
    printf("taproot_selftest: 3 pins, %zu scripts in one buffer, %zu alone ok\n", n, alone);
    return 0;
}
