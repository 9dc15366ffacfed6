// Stand-alone run of the MuSig2 bodies under the address and undefined-behaviour sanitizers (and the limb-bound tracker).
// First, from nothing but small integers: three signers (two of them with one key) aggregate their keys, apply a plain and a
// Taproot tweak, sign, check each other's partial signatures and aggregate; the BIP-340 verifier body must accept the result,
// and must refuse it after one flipped bit.  Every buffer is a heap allocation of exactly the bytes the call may touch.
// argv[1] is a file tests/test_musig_cpu.py writes: one key-aggregation set with the oracle's outputs.
//   u64 n, total (signers in the buffers)
//   pkx[32 total] pky[32 total] key_offsets[8 (n + 1)] | keyagg[192 n] agg_pk[32 n] err[n]
// The set is aggregated once in its buffers, then every session alone in allocations that hold nothing but its own keys and
// its own record: a lane that read a neighbour's key, or wrote beyond its record, would stop the program.  Exit status 0 = all held.
#include <cstdio>
#include <cstring>

#include "p2e_emu_musig.cpp"

namespace {
typedef std::vector<uint8_t> Bytes;
FILE* g_file = nullptr;
bool g_ok = true;
Bytes take(size_t count) {
    Bytes b(count, 0);
    if (count && fread(b.data(), 1, count, g_file) != count) g_ok = false;
    return b;
}
int differ(const char* what, const Bytes& got, const Bytes& want) {
    if (got == want) return 0;
    size_t at = 0;
    while (at < got.size() && at < want.size() && got[at] == want[at]) at++;
    fprintf(stderr, "FAIL %s: first difference at byte %zu\n", what, at);
    return 1;
}
Bytes le_scalar(uint32_t v) {
    Bytes b(32, 0);
    memcpy(b.data(), &v, 4);
    return b;
}
// the public key of a small secret key appended to the little-endian arrays x and y
void public_key(uint32_t d, Bytes& x, Bytes& y) {
    const Bytes sk = le_scalar(d);
    Bytes px(32, 0), py(32, 0);
    body_public_key<Secp256k1, SIGN_PLAN_LANE>(gen_table(), sk.data(), px.data(), py.data(), 0, 0);
    x.insert(x.end(), px.begin(), px.end());
    y.insert(y.end(), py.begin(), py.end());
}

int round_trip() {
    int fails = 0;
    const uint32_t sks[3] = {11, 11, 13}, k1s[3] = {101, 103, 107}, k2s[3] = {201, 203, 207};
    const uint64_t offsets[2] = {0, 3};
    Bytes pkx, pky, err(1, 0xAA);
    for (uint32_t d : sks) public_key(d, pkx, pky);
    Bytes ka(192, 0xAA), pk(32, 0xAA);
    fails += emumusig_key_agg(pkx.data(), pky.data(), offsets, ka.data(), pk.data(), 1, err.data()) != 0;
    const Bytes tweak(32, 0x42);
    fails += emumusig_apply_tweak(ka.data(), tweak.data(), MUSIG_TWEAK_PLAIN, ka.data(), pk.data(), 1, err.data()) != 0;        // (in place)
    fails += emumusig_apply_tweak(ka.data(), nullptr, MUSIG_TWEAK_TAPROOT, ka.data(), pk.data(), 1, err.data()) != 0;
    Bytes pubnonce;   // x(R_1) || y(R_1) || x(R_2) || y(R_2) per signer
    for (int j = 0; j < 3; j++) {
        Bytes x, y;
        public_key(k1s[j], x, y), public_key(k2s[j], x, y);
        pubnonce.insert(pubnonce.end(), x.begin(), x.begin() + 32), pubnonce.insert(pubnonce.end(), y.begin(), y.begin() + 32);
        pubnonce.insert(pubnonce.end(), x.begin() + 32, x.end()), pubnonce.insert(pubnonce.end(), y.begin() + 32, y.end());
    }
    Bytes agg(128, 0xAA), ses(128, 0xAA);
    const Bytes msg(32, 0x17);
    fails += emumusig_nonce_agg(pubnonce.data(), offsets, agg.data(), 1, err.data()) != 0;
    fails += emumusig_session(ka.data(), agg.data(), msg.data(), ses.data(), 1, err.data()) != 0;
    Bytes psigs(3 * 32, 0xAA);
    for (int j = 0; j < 3; j++) {
        Bytes sec = le_scalar(k1s[j]);
        const Bytes k2 = le_scalar(k2s[j]), sk = le_scalar(sks[j]);
        sec.insert(sec.end(), k2.begin(), k2.end());
        Bytes one(32, 0xAA);
        fails += emumusig_partial_sign(sec.data(), sk.data(), ka.data(), ses.data(), one.data(), 1, err.data()) != 0;
        memcpy(psigs.data() + 32 * j, one.data(), 32);
    }
    const uint32_t index[3] = {0, 0, 0};
    Bytes verr(3, 0xAA), valid(3, 0xAA);
    fails += emumusig_partial_verify(psigs.data(), pubnonce.data(), pkx.data(), pky.data(), index, ka.data(), ses.data(), 1, 3, verr.data(), valid.data()) != 0;
    if (valid != Bytes(3, 1)) fprintf(stderr, "FAIL round trip: a partial signature does not verify\n"), fails++;
    Bytes sig(64, 0xAA), ok(1, 0xAA);
    fails += emumusig_sig_agg(psigs.data(), offsets, ka.data(), ses.data(), sig.data(), 1, err.data()) != 0;
    const uint8_t e = body_schnorr_verify(gen_table(), msg.data(), pk.data(), sig.data(), ok.data(), 0);
    if (e || ok[0] != 1) fprintf(stderr, "FAIL round trip: the BIP-340 verifier refuses the aggregate signature (code %d)\n", e), fails++;
    sig[40] ^= 1;
    body_schnorr_verify(gen_table(), msg.data(), pk.data(), sig.data(), ok.data(), 0);
    if (ok[0] != 0) fprintf(stderr, "FAIL round trip: the verifier accepts a flipped bit\n"), fails++;
    return fails;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: musig_selftest VECTORS\n");
        return 2;
    }
    int fails = round_trip();
    g_file = fopen(argv[1], "rb");
    uint64_t hdr[2] = {0, 0};
    if (!g_file || fread(hdr, 8, 2, g_file) != 2 || hdr[0] < 1 || hdr[0] > 4096 || hdr[1] > (1u << 20)) {
        fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    const size_t n = hdr[0], total = hdr[1];
    const Bytes pkx = take(32 * total), pky = take(32 * total), off_bytes = take(8 * (n + 1));
    const Bytes w_ka = take(192 * n), w_pk = take(32 * n), w_err = take(n);
    const bool at_end = fgetc(g_file) == EOF;
    fclose(g_file);
    if (!g_ok || !at_end) {
        fprintf(stderr, "%s is not a vector file of this program\n", argv[1]);
        return 2;
    }
    std::vector<uint64_t> offsets(n + 1);
    memcpy(offsets.data(), off_bytes.data(), 8 * (n + 1));
    {
        Bytes ka(192 * n, 0xAA), pk(32 * n, 0xAA), err(n, 0xAA);
        emumusig_key_agg(pkx.data(), pky.data(), offsets.data(), ka.data(), pk.data(), n, err.data());
        fails += differ("codes of the set", err, w_err) + differ("records of the set", ka, w_ka) + differ("keys of the set", pk, w_pk);
    }
    size_t alone = 0;
    for (size_t i = 0; i < n; i++) {
        if (offsets[i + 1] < offsets[i] || offsets[i + 1] > total) continue;
        const size_t cnt = offsets[i + 1] - offsets[i];
        const Bytes ox(pkx.begin() + 32 * offsets[i], pkx.begin() + 32 * offsets[i + 1]), oy(pky.begin() + 32 * offsets[i], pky.begin() + 32 * offsets[i + 1]);
        const uint64_t o[2] = {0, cnt};
        Bytes ka(192, 0xAA), pk(32, 0xAA), err(1, 0xAA);
        emumusig_key_agg(ox.data(), oy.data(), o, ka.data(), pk.data(), 1, err.data());
        if (err[0] != w_err[i] || memcmp(ka.data(), w_ka.data() + 192 * i, 192) || memcmp(pk.data(), w_pk.data() + 32 * i, 32))
            fprintf(stderr, "FAIL session %zu alone\n", i), fails++;
        alone++;
    }
    if (fails) return 1;
    printf("musig_selftest: round trip, %zu sessions in one buffer, %zu alone ok\n", n, alone);
    return 0;
}
