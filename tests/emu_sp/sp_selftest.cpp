// Stand-alone run of the silent-payment bodies under the address and undefined-behaviour sanitizers (and the limb-bound
// tracker).  First, from nothing but small integers: a payment made by the sender's body is found by the receiver's body, with
// and without a label.  argv[1] is a file tests/test_sp_cpu.py writes: one scan set with the oracle's outputs.
//   u64 n, n_labels, max_hits, total (outputs in the buffer), with_hash
//   scan_sk[32] spend_pkx[32] spend_pky[32] label_x[32 n_labels] label_y[32 n_labels] ax[32 n] ay[32 n] input_hash[32 n, if with_hash]
//   outputs[32 total] out_offsets[8 (n + 1)] | n_hits[n] hit_output[4 n max_hits] hit_label[n max_hits] hit_tweak[32 n max_hits] err[n]
// The set is scanned once in its buffers, then every transaction alone in heap allocations that hold nothing but its own
// outputs and its own result slots: a lane that read an output of a neighbour, or wrote a slot beyond max_hits, would stop the
// program.  Exit status 0 = all held.
#include <cstdio>
#include <cstring>

#include "p2e_emu_sp.cpp"

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
// the public key of a small secret key, little-endian (x, y)
void public_key(uint32_t d, Bytes& x, Bytes& y) {
    x.assign(32, 0), y.assign(32, 0);
    const Bytes sk = le_scalar(d);
    body_public_key<Secp256k1, SIGN_PLAN_LANE>(gen_table(), sk.data(), x.data(), y.data(), 0, 0);
}

// sender = receiver: a pays b (scan key 5, spend key 7) at k = 0 and k = 1, the second under label 3, among two decoys
int round_trip() {
    int fails = 0;
    Bytes ax, ay, scx, scy, spx, spy;
    public_key(11, ax, ay), public_key(5, scx, scy), public_key(7, spx, spy);
    const Bytes a = le_scalar(11), b = le_scalar(5), outpoint(36, 0x42);
    Bytes ih(32, 0xAA), err(2, 0xAA);
    emusp_input_hash(outpoint.data(), ax.data(), ay.data(), ih.data(), 1, err.data());
    fails += err[0] != 0;
    const uint32_t m = 3;
    Bytes lt(32, 0xAA), lx(32, 0xAA), ly(32, 0xAA);
    emusp_label(b.data(), &m, lt.data(), lx.data(), ly.data(), 1, err.data());
    fails += err[0] != 0;
    Bytes lspx(32, 0xAA), lspy(32, 0xAA);   // the labelled spend key B_spend + L_3
    fails += body_point_add<Secp256k1>(spx.data(), spy.data(), lx.data(), ly.data(), lspx.data(), lspy.data(), 0) != 0;
    Bytes outputs(4 * 32, 0x33);
    const uint32_t k0 = 0, k1 = 1;
    emusp_send(a.data(), ih.data(), scx.data(), scy.data(), spx.data(), spy.data(), &k0, outputs.data() + 2 * 32, 1, err.data());
    fails += err[0] != 0;
    emusp_send(a.data(), ih.data(), scx.data(), scy.data(), lspx.data(), lspy.data(), &k1, outputs.data() + 1 * 32, 1, err.data());
    fails += err[0] != 0;
    const uint64_t offsets[2] = {0, 4};
    Bytes n_hits(1, 0xAA), hit_label(3, 0xAA), hit_tweak(3 * 32, 0xAA);
    std::vector<uint32_t> hit_output(3, 0xAAAAAAAAu);
    emusp_scan(b.data(), spx.data(), spy.data(), lx.data(), ly.data(), 1, ax.data(), ay.data(), ih.data(), outputs.data(), offsets, 3, n_hits.data(),
               hit_output.data(), hit_label.data(), hit_tweak.data(), 1, err.data());
    if (err[0] != 0 || n_hits[0] != 2 || hit_output[0] != 2 || hit_output[1] != 1 || hit_output[2] != 0 || hit_label[0] != 0 || hit_label[1] != 1 ||
        hit_label[2] != 0)
        fprintf(stderr, "FAIL round trip: code %d, %d hits\n", err[0], n_hits[0]), fails++;
    // without the label the second payment is not found, and the loop stops at k = 1
    emusp_scan(b.data(), spx.data(), spy.data(), nullptr, nullptr, 0, ax.data(), ay.data(), ih.data(), outputs.data(), offsets, 3, n_hits.data(),
               hit_output.data(), hit_label.data(), hit_tweak.data(), 1, err.data());
    if (err[0] != 0 || n_hits[0] != 1 || hit_output[0] != 2) fprintf(stderr, "FAIL round trip without labels\n"), fails++;
    return fails;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: sp_selftest VECTORS\n");
        return 2;
    }
    int fails = round_trip();
    g_file = fopen(argv[1], "rb");
    uint64_t hdr[5] = {0, 0, 0, 0, 0};
    if (!g_file || fread(hdr, 8, 5, g_file) != 5 || hdr[0] < 1 || hdr[0] > 4096 || hdr[1] > SP_MAX_LABELS || hdr[2] < 1 || hdr[2] > SP_MAX_HITS ||
        hdr[3] > (1u << 20) || hdr[4] > 1) {
        fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    const size_t n = hdr[0], nl = hdr[1], mh = hdr[2], total = hdr[3];
    const bool with_hash = hdr[4] != 0;
    const Bytes sk = take(32), spx = take(32), spy = take(32), lx = take(32 * nl), ly = take(32 * nl), ax = take(32 * n), ay = take(32 * n);
    const Bytes ih = take(with_hash ? 32 * n : 0), outputs = take(32 * total), off_bytes = take(8 * (n + 1));
    const Bytes w_hits = take(n), w_out = take(4 * n * mh), w_label = take(n * mh), w_tweak = take(32 * n * mh), w_err = take(n);
    const bool at_end = fgetc(g_file) == EOF;
    fclose(g_file);
    if (!g_ok || !at_end) {
        fprintf(stderr, "%s is not a vector file of this program\n", argv[1]);
        return 2;
    }
    std::vector<uint64_t> offsets(n + 1);
    memcpy(offsets.data(), off_bytes.data(), 8 * (n + 1));
    const uint8_t* ihp = with_hash ? ih.data() : nullptr;
    {
        Bytes n_hits(n, 0xAA), hit_out(4 * n * mh, 0xAA), hit_label(n * mh, 0xAA), hit_tweak(32 * n * mh, 0xAA), err(n, 0xAA);
        emusp_scan(sk.data(), spx.data(), spy.data(), lx.data(), ly.data(), nl, ax.data(), ay.data(), ihp, outputs.data(), offsets.data(), mh,
                   n_hits.data(), reinterpret_cast<uint32_t*>(hit_out.data()), hit_label.data(), hit_tweak.data(), n, err.data());
        fails += differ("codes of the set", err, w_err) + differ("hit counts of the set", n_hits, w_hits) + differ("hit outputs of the set", hit_out, w_out) +
                 differ("hit labels of the set", hit_label, w_label) + differ("hit tweaks of the set", hit_tweak, w_tweak);
    }
    size_t alone = 0, hits = 0;
    for (size_t i = 0; i < n; i++) {
        if (offsets[i + 1] < offsets[i] || offsets[i + 1] > total) continue;
        const size_t cnt = offsets[i + 1] - offsets[i];
        const Bytes own(outputs.begin() + 32 * offsets[i], outputs.begin() + 32 * offsets[i + 1]);
        const uint64_t o[2] = {0, cnt};
        Bytes n_hits(1, 0xAA), hit_out(4 * mh, 0xAA), hit_label(mh, 0xAA), hit_tweak(32 * mh, 0xAA), err(1, 0xAA);
        emusp_scan(sk.data(), spx.data(), spy.data(), lx.data(), ly.data(), nl, ax.data() + 32 * i, ay.data() + 32 * i, with_hash ? ihp + 32 * i : nullptr,
                   own.data(), o, mh, n_hits.data(), reinterpret_cast<uint32_t*>(hit_out.data()), hit_label.data(), hit_tweak.data(), 1, err.data());
        if (err[0] != w_err[i] || n_hits[0] != w_hits[i] || memcmp(hit_out.data(), w_out.data() + 4 * mh * i, 4 * mh) ||
            memcmp(hit_label.data(), w_label.data() + mh * i, mh) || memcmp(hit_tweak.data(), w_tweak.data() + 32 * mh * i, 32 * mh))
            fprintf(stderr, "FAIL transaction %zu alone\n", i), fails++;
        alone++;
        hits += n_hits[0];
    }
    if (fails) return 1;
    printf("sp_selftest: round trip, %zu transactions in one buffer, %zu alone with %zu hits ok\n", n, alone, hits);
    return 0;
}
