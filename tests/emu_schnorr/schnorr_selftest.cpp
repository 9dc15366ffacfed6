// Stand-alone run of the BIP-340 bodies under the address and undefined-behaviour sanitizers (and the limb-bound tracker).
// argv[1] is a file tests/test_schnorr_cpu.py writes from tests/schnorr_inputs.py: the signer set and the verifier set with
// the oracle's expectations.  Every input and output lives in a heap allocation of EXACTLY its size, so a lane that read or
// wrote past its element would stop the program.  Each body runs over the whole set and over its first element alone; every
// byte is compared.  Exit status 0 = all held.
//   u64 ns, nv
//   signer set    msg[32 ns] sk[32 ns] aux[32 ns] | pk[32 ns] pk_err[ns] sig[64 ns] sig_err[ns]
//   verifier set  msg[32 nv] pk[32 nv] sig[64 nv] | err[nv] valid[nv] | decode px[32 nv] py[32 nv] err[nv]
//   aggregate     seed[32] | err[nv] k[32 (2 nv + 1)] px[..] py[..]
#include <cstdio>
#include <cstring>

#include "p2e_emu_schnorr.cpp"

namespace {
typedef std::vector<uint8_t> Bytes;
bool take(FILE* f, Bytes& b, size_t count) {
    b.assign(count, 0);
    return count == 0 || fread(b.data(), 1, count, f) == count;
}
int differ(const char* what, const Bytes& got, const Bytes& want) {
    if (got == want) return 0;
    size_t at = 0;
    while (at < got.size() && got[at] == want[at]) at++;
    fprintf(stderr, "FAIL %s: first difference at byte %zu\n", what, at);
    return 1;
}
Bytes head(const Bytes& b, size_t count) { return Bytes(b.begin(), b.begin() + (long)count); }
}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: schnorr_selftest VECTORS\n");
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    uint64_t ns = 0, nv = 0;
    if (!f || fread(&ns, 8, 1, f) != 1 || fread(&nv, 8, 1, f) != 1 || ns < 1 || nv < 1 || ns > 4096 || nv > 4096) {
        fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    Bytes s_msg, s_sk, s_aux, w_pk, w_pkerr, w_sig, w_sigerr, v_msg, v_pk, v_sig, w_err, w_valid, w_dx, w_dy, w_derr, seed, w_aerr, w_ak, w_ax, w_ay;
    const size_t terms = 2 * nv + 1;
    bool ok = take(f, s_msg, 32 * ns) && take(f, s_sk, 32 * ns) && take(f, s_aux, 32 * ns) && take(f, w_pk, 32 * ns) && take(f, w_pkerr, ns) &&
              take(f, w_sig, 64 * ns) && take(f, w_sigerr, ns) && take(f, v_msg, 32 * nv) && take(f, v_pk, 32 * nv) && take(f, v_sig, 64 * nv) &&
              take(f, w_err, nv) && take(f, w_valid, nv) && take(f, w_dx, 32 * nv) && take(f, w_dy, 32 * nv) && take(f, w_derr, nv) &&
              take(f, seed, 32) && take(f, w_aerr, nv) && take(f, w_ak, 32 * terms) && take(f, w_ax, 32 * terms) && take(f, w_ay, 32 * terms);
    ok = ok && fgetc(f) == EOF;
    fclose(f);
    if (!ok) {
        fprintf(stderr, "%s is not a vector file of this program\n", argv[1]);
        return 2;
    }
    int fails = 0;
    for (const size_t n_s : {(size_t)ns, (size_t)1}) {
        Bytes pk(32 * n_s, 0xAA), err(n_s, 0xAA), sig(64 * n_s, 0xAA);
        const Bytes msg = head(s_msg, 32 * n_s), sk = head(s_sk, 32 * n_s), aux = head(s_aux, 32 * n_s);
        emusch_public_key(sk.data(), pk.data(), n_s, err.data());
        fails += differ("public key", pk, head(w_pk, 32 * n_s)) + differ("public key err", err, head(w_pkerr, n_s));
        err.assign(n_s, 0xAA);
        emusch_sign(msg.data(), sk.data(), aux.data(), sig.data(), n_s, err.data());
        fails += differ("sign", sig, head(w_sig, 64 * n_s)) + differ("sign err", err, head(w_sigerr, n_s));
    }
    for (const size_t n_v : {(size_t)nv, (size_t)1}) {
        const Bytes msg = head(v_msg, 32 * n_v), pk = head(v_pk, 32 * n_v), sig = head(v_sig, 64 * n_v);
        Bytes err(n_v, 0xAA), valid(n_v, 0xAA), dx(32 * n_v, 0xAA), dy(32 * n_v, 0xAA);
        emusch_verify(msg.data(), pk.data(), sig.data(), n_v, err.data(), valid.data());
        fails += differ("verify err", err, head(w_err, n_v)) + differ("verify valid", valid, head(w_valid, n_v));
        err.assign(n_v, 0xAA);
        emusch_xonly_decode(pk.data(), dx.data(), dy.data(), n_v, err.data());
        fails += differ("decode x", dx, head(w_dx, 32 * n_v)) + differ("decode y", dy, head(w_dy, 32 * n_v)) + differ("decode err", err, head(w_derr, n_v));
    }
    {
        Bytes err(nv, 0xAA), k(32 * terms, 0xAA), px(32 * terms, 0xAA), py(32 * terms, 0xAA);
        emusch_agg_prepare(v_msg.data(), v_pk.data(), v_sig.data(), seed.data(), nv, k.data(), px.data(), py.data(), err.data());
        fails += differ("aggregate err", err, w_aerr) + differ("aggregate scalars", k, w_ak) + differ("aggregate x", px, w_ax) +
                 differ("aggregate y", py, w_ay);
        Bytes k0(32, 0xAA), x0(32, 0xAA), y0(32, 0xAA);   // n = 0: term 0 alone, scalar 0
        emusch_agg_prepare(nullptr, nullptr, nullptr, seed.data(), 0, k0.data(), x0.data(), y0.data(), nullptr);
        fails += differ("aggregate n = 0 scalar", k0, Bytes(32, 0)) + differ("aggregate n = 0 x", x0, head(w_ax, 32));
    }
    // the inner signer with k' = 0
    {
        Bytes zero(32, 0), one(32, 0), sig(64, 0xAA);
        one[31] = 1;
        if (emusch_sign_with_nonce(one.data(), head(w_pk, 32).data(), zero.data(), zero.data(), sig.data()) != WIRE_INFINITY || sig != Bytes(64, 0xAA)) {
            fprintf(stderr, "FAIL k' = 0\n");
            fails++;
        }
    }
    if (fails) return 1;
    printf("schnorr_selftest: %llu signer and %llu verifier elements ok\n", (unsigned long long)ns, (unsigned long long)nv);
    return 0;
}
