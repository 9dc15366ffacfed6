// Stand-alone run of the BIP-32 / HASH160 bodies under the address and undefined-behaviour sanitizers (and the limb-bound
// tracker).  argv[1] is a file tests/test_hd_cpu.py writes from tests/hd_inputs.py: the input sets with the oracle's
// expectations and the forced-I_L table.  Every input and output lives in a heap allocation of its own size (the two
// byte-addressed inputs, seeds and messages, rounded up to 4: a lane reads aligned words), so a lane that read or wrote past
// its element would stop the program.  Each call runs over the whole set and over its first element alone; every byte is
// compared.  Two published answers are checked before the file is opened.  Exit status 0 = all held.
//   u64 n, data_bytes, n_fp, n_fq
//   priv          par_sk[32 n] par_cc[32 n] index[4 n] | sk[32 n] cc[32 n] err[n]
//   priv, 1 par   par_sk[32] par_cc[32] | sk[32 n] cc[32 n] err[n]                       (the same indices)
//   pub           par_x[32 n] par_y[32 n] par_cc[32 n] | x[32 n] y[32 n] cc[32 n] err[n]
//   pub, 1 par    par_x[32] par_y[32] par_cc[32] | x[32 n] y[32 n] cc[32 n] err[n]
//   master        for L = 16, 32, 63, 64: seed[L n] | sk[32 n] cc[32 n] err[n]
//   hash160       data[data_bytes] offsets[8 (n + 1)] | out[20 n] u64 reversed
//   key hash      x[32 n] y[32 n] err_in[n] | compressed[20 n] uncompressed[20 n] compressed_err[20 n] uncompressed_err[20 n]
//   forced priv   il[32 n_fp] k[32 n_fp] | code[n_fp] out[32 n_fp]
//   forced pub    il[32 n_fq] x[32 n_fq] y[32 n_fq] | code[n_fq] outx[32 n_fq] outy[32 n_fq]
#include <cstdio>
#include <cstring>

#include "p2e_emu_hd.cpp"

namespace {
typedef std::vector<uint8_t> Bytes;
FILE* g_file = nullptr;
bool g_ok = true;
// `count` bytes of the file in an allocation of `count` bytes rounded up to `round`
Bytes take(size_t count, size_t round = 1) {
    Bytes b((count + round - 1) / round * round, 0);
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
Bytes head(const Bytes& b, size_t count) { return Bytes(b.begin(), b.begin() + (long)count); }
Bytes row(const Bytes& b, size_t j) { return Bytes(b.begin() + 32 * (long)j, b.begin() + 32 * (long)(j + 1)); }   // 32-byte row j, alone
const uint32_t* u32p(const Bytes& b) { return reinterpret_cast<const uint32_t*>(b.data()); }

int known_answers() {
    int fails = 0;
    // RIPEMD-160("abc") = 8eb208f7 e05d987a 9b044a8e 98c6b087 f15a0bfc (the paper's appendix B)
    uint8_t block[64] = {'a', 'b', 'c', 0x80};
    block[56] = 24;
    uint32_t st[5];
    emuhd_ripemd160_iv(st);
    emuhd_ripemd160_compress(st, block);
    const uint32_t want[5] = {0xf708b28eu, 0x7a985de0u, 0x8e4a049bu, 0x87b0c698u, 0xfc0b5af1u};
    if (memcmp(st, want, 20)) fprintf(stderr, "FAIL RIPEMD-160(abc)\n"), fails++;
    // BIP-32 test vector 1: the master key of the seed 00 .. 0f
    Bytes seed(16), sk(32, 0xAA), cc(32, 0xAA), err(1, 0xAA);
    for (int j = 0; j < 16; j++) seed[(size_t)j] = (uint8_t)j;
    emuhd_master(seed.data(), 16, sk.data(), cc.data(), 1, err.data());
    const uint8_t k_be[32] = {0xe8, 0xf3, 0x2e, 0x72, 0x3d, 0xec, 0xf4, 0x05, 0x1a, 0xef, 0xac, 0x8e, 0x2c, 0x93, 0xc9, 0xc5,
                              0xb2, 0x14, 0x31, 0x38, 0x17, 0xcd, 0xb0, 0x1a, 0x14, 0x94, 0xb9, 0x17, 0xc8, 0x43, 0x6b, 0x35};
    const uint8_t c[32] = {0x87, 0x3d, 0xff, 0x81, 0xc0, 0x2f, 0x52, 0x56, 0x23, 0xfd, 0x1f, 0xe5, 0x16, 0x7e, 0xac, 0x3a,
                           0x55, 0xa0, 0x49, 0xde, 0x3d, 0x31, 0x4b, 0xb4, 0x2e, 0xe2, 0x27, 0xff, 0xed, 0x37, 0xd5, 0x08};
    bool ok = err[0] == 0 && memcmp(cc.data(), c, 32) == 0;
    for (int j = 0; j < 32; j++) ok = ok && sk[(size_t)j] == k_be[31 - j];
    if (!ok) fprintf(stderr, "FAIL BIP-32 test vector 1, chain m\n"), fails++;
    return fails;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: hd_selftest VECTORS\n");
        return 2;
    }
    int fails = known_answers();
    g_file = fopen(argv[1], "rb");
    uint64_t hdr[4] = {0, 0, 0, 0};
    if (!g_file || fread(hdr, 8, 4, g_file) != 4 || hdr[0] < 1 || hdr[0] > 4096 || hdr[1] > (1u << 24) || hdr[2] > 64 || hdr[3] > 64) {
        fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    const size_t n = hdr[0], data_bytes = hdr[1], nfp = hdr[2], nfq = hdr[3];
    const Bytes p_sk = take(32 * n), p_cc = take(32 * n), index = take(4 * n), w_sk = take(32 * n), w_cc = take(32 * n), w_err = take(n);
    const Bytes p1_sk = take(32), p1_cc = take(32), w1_sk = take(32 * n), w1_cc = take(32 * n), w1_err = take(n);
    const Bytes q_x = take(32 * n), q_y = take(32 * n), q_cc = take(32 * n), v_x = take(32 * n), v_y = take(32 * n), v_cc = take(32 * n),
                v_err = take(n);
    const Bytes q1_x = take(32), q1_y = take(32), q1_cc = take(32), v1_x = take(32 * n), v1_y = take(32 * n), v1_cc = take(32 * n),
                v1_err = take(n);
    const size_t seed_lens[4] = {16, 32, 63, 64};
    Bytes seeds[4], m_sk[4], m_cc[4], m_err[4];
    for (int s = 0; s < 4; s++) seeds[s] = take(seed_lens[s] * n, 4), m_sk[s] = take(32 * n), m_cc[s] = take(32 * n), m_err[s] = take(n);
    const Bytes data = take(data_bytes, 4), offsets = take(8 * (n + 1)), w_h = take(20 * n), w_rev = take(8);
    const Bytes h_x = take(32 * n), h_y = take(32 * n), h_err = take(n), w_c = take(20 * n), w_u = take(20 * n), w_ce = take(20 * n),
                w_ue = take(20 * n);
    const Bytes f_il = take(32 * nfp), f_k = take(32 * nfp), f_code = take(nfp), f_out = take(32 * nfp);
    const Bytes g_il = take(32 * nfq), g_x = take(32 * nfq), g_y = take(32 * nfq), g_code = take(nfq), g_ox = take(32 * nfq), g_oy = take(32 * nfq);
    const bool at_end = fgetc(g_file) == EOF;
    fclose(g_file);
    if (!g_ok || !at_end) {
        fprintf(stderr, "%s is not a vector file of this program\n", argv[1]);
        return 2;
    }
    for (const size_t m : {n, (size_t)1}) {
        const Bytes idx = head(index, 4 * m);
        {
            Bytes sk(32 * m, 0xAA), cc(32 * m, 0xAA), err(m, 0xAA);
            emuhd_ckd_priv(head(p_sk, 32 * m).data(), head(p_cc, 32 * m).data(), m, u32p(idx), sk.data(), cc.data(), m, err.data());
            fails += differ("ckd_priv key", sk, head(w_sk, 32 * m)) + differ("ckd_priv chain code", cc, head(w_cc, 32 * m)) +
                     differ("ckd_priv err", err, head(w_err, m));
            sk.assign(32 * m, 0xAA), cc.assign(32 * m, 0xAA), err.assign(m, 0xAA);
            emuhd_ckd_priv(p1_sk.data(), p1_cc.data(), 1, u32p(idx), sk.data(), cc.data(), m, err.data());
            fails += differ("ckd_priv key, one parent", sk, head(w1_sk, 32 * m)) + differ("ckd_priv chain code, one parent", cc, head(w1_cc, 32 * m)) +
                     differ("ckd_priv err, one parent", err, head(w1_err, m));
        }
        {
            Bytes x(32 * m, 0xAA), y(32 * m, 0xAA), cc(32 * m, 0xAA), err(m, 0xAA);
            emuhd_ckd_pub(head(q_x, 32 * m).data(), head(q_y, 32 * m).data(), head(q_cc, 32 * m).data(), m, u32p(idx), x.data(), y.data(),
                          cc.data(), m, err.data());
            fails += differ("ckd_pub x", x, head(v_x, 32 * m)) + differ("ckd_pub y", y, head(v_y, 32 * m)) +
                     differ("ckd_pub chain code", cc, head(v_cc, 32 * m)) + differ("ckd_pub err", err, head(v_err, m));
            x.assign(32 * m, 0xAA), y.assign(32 * m, 0xAA), cc.assign(32 * m, 0xAA), err.assign(m, 0xAA);
            emuhd_ckd_pub(q1_x.data(), q1_y.data(), q1_cc.data(), 1, u32p(idx), x.data(), y.data(), cc.data(), m, err.data());
            fails += differ("ckd_pub x, one parent", x, head(v1_x, 32 * m)) + differ("ckd_pub y, one parent", y, head(v1_y, 32 * m)) +
                     differ("ckd_pub chain code, one parent", cc, head(v1_cc, 32 * m)) + differ("ckd_pub err, one parent", err, head(v1_err, m));
        }
        for (int s = 0; s < 4; s++) {
            Bytes in = head(seeds[s], seed_lens[s] * m);
            in.resize((in.size() + 3) / 4 * 4);
            Bytes sk(32 * m, 0xAA), cc(32 * m, 0xAA), err(m, 0xAA);
            emuhd_master(in.data(), seed_lens[s], sk.data(), cc.data(), m, err.data());
            fails += differ("master key", sk, head(m_sk[s], 32 * m)) + differ("master chain code", cc, head(m_cc[s], 32 * m)) +
                     differ("master err", err, head(m_err[s], m));
        }
        {
            Bytes out(20 * m, 0xAA);
            const long rev = emuhd_hash160(data.data(), reinterpret_cast<const uint64_t*>(offsets.data()), out.data(), m);
            uint64_t want_rev = 0;
            memcpy(&want_rev, w_rev.data(), 8);
            fails += differ("hash160", out, head(w_h, 20 * m));
            if (m == n && (uint64_t)rev != want_rev) fprintf(stderr, "FAIL hash160 reversed count\n"), fails++;
        }
        for (int form = 0; form < 2; form++) {
            Bytes out(20 * m, 0xAA);
            emuhd_key_hash160((unsigned)form, head(h_x, 32 * m).data(), head(h_y, 32 * m).data(), nullptr, out.data(), m);
            fails += differ("key hash160", out, head(form ? w_u : w_c, 20 * m));
            out.assign(20 * m, 0xAA);
            emuhd_key_hash160((unsigned)form, head(h_x, 32 * m).data(), head(h_y, 32 * m).data(), head(h_err, m).data(), out.data(), m);
            fails += differ("key hash160 with err_in", out, head(form ? w_ue : w_ce, 20 * m));
        }
    }
    for (size_t j = 0; j < nfp; j++) {
        Bytes out(32, 0);
        const int e = emuhd_finish_priv(row(f_il, j).data(), row(f_k, j).data(), out.data());
        if (e != f_code[j] || out != row(f_out, j)) fprintf(stderr, "FAIL forced priv %zu\n", j), fails++;
    }
    for (size_t j = 0; j < nfq; j++) {
        Bytes ox(32, 0), oy(32, 0);
        const int e = emuhd_finish_pub(row(g_il, j).data(), row(g_x, j).data(), row(g_y, j).data(), ox.data(), oy.data());
        if (e != g_code[j] || ox != row(g_ox, j) || oy != row(g_oy, j)) fprintf(stderr, "FAIL forced pub %zu\n", j), fails++;
    }
    if (fails) return 1;
    printf("hd_selftest: %zu elements per set, %zu + %zu forced cases ok\n", n, nfp, nfq);
    return 0;
}
