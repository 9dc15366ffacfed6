// Multi-scalar multiplication sum_i k_i P_i by the bucket (Pippenger) method, on either curve: the native many-point sum of
// curve/curve_msm.rs (msm_parallel / msm_execute), without its precomputation.  include/p2e.h p2e_point_msm.
//
// Plan (msm_plan: a function of n and the window width c alone, the same on the host, the device and the CPU build):
//   digits    signed, c bits: k = sum_w d_w 2^(c w), -2^(c-1) < d_w <= 2^(c-1), W = floor(256 / c) + 1 windows.  c W >= 257, so
//             the top window holds at least one bit above the scalar: its raw value is below 2^(c-1) and the carry that
//             enters it cannot leave it, for every k < 2^256.  B = 2^(c-1) buckets per window (bucket |d| - 1, d < 0
//             adds -P); digit 0 goes nowhere.
//   launches  1 digits    lane per point: range / on-curve check, skip[i], count[w B + b] by integer atomics
//             2 scan      one block: exclusive scans of count (-> off) and of ceil(count / seg) (-> segoff)
//             3 scatter   lane per point: idx[off[e] + cursor[e]++] = i | sign
//             4 segments  lane per segment of at most `seg` entries of ONE bucket: mixed additions -> partial[s]
//             5 buckets   lane per bucket: its partials summed -> bucket[e]
//             6 chunks    lane per `chunk` consecutive buckets of a window: running sums give sum (b - a0 + 1) B_b, plus
//                         a0 S by a short double-and-add (a0 < B) -> chunkpart
//             7 final     one block: lane per window sums its chunk partials; lane 0 walks the windows from the top
//                         (c doublings, one addition each), inverts Z once (safegcd) and stores the point and the status
// The balance: a lane of launch 4 adds at most seg points whatever the scalars are; with all scalars equal one bucket per
// window holds all n points, and launch 5 then adds ceil(n / seg) partials in one lane.  max_lane_additions (MsmPlan) is
// the maximum over the launches of the point operations (additions and doublings) of one lane; it depends on n, c only.
//
// The additions.  Launches 4-7 add points that are unrelated: equal operands (two copies of a point in a bucket; the
// running sum meeting the sum of running sums), opposite operands (P and -P in a bucket) and neutral operands (empty
// buckets, empty windows) occur for ordinary inputs.  msm_add is therefore complete: the neutral element is an explicit
// flag (SignSum::have, stored as Z = 0), and h = U2 - U1 and r = S2 - S1 are tested on canonical values: h != 0 -> the
// ordinary sum; h = 0, r = 0 -> a doubling (Z3 = 2 Y Z != 0: no point of order two on either curve); h = 0, r != 0 -> the
// neutral element.  The formula is written out on RecField<CV> (one text for both curves) instead of calling
// jac_add29 / jac_add_cv, so that h and r are computed once: the tests cost two canonical forms per addition, not a second
// set of cross products.  A zero Z never reaches a formula as if it were a point: every operand is used only under `have`.
#pragma once
#include "recover.hpp"

#ifndef P2E_MSM_NOTE_OP
#define P2E_MSM_NOTE_OP() ((void)0)   // the CPU build counts point operations per lane here
#endif

namespace p2e {

constexpr unsigned MSM_WINDOW_MIN = 4, MSM_WINDOW_MAX = 12;   // include/p2e.h P2E_MSM_WINDOW_MIN / _MAX
constexpr uint8_t MSM_OK = 0, MSM_NEUTRAL = 1, MSM_BAD_POINT = 2;
constexpr size_t MSM_MAX_N = (size_t)1 << 24;   // W n < 2^31: positions and the sign bit share a u32
constexpr u32 MSM_NEG = 0x80000000u;
constexpr u32 MSM_SCAN_LANES = 256, MSM_FINAL_LANES = 128;
constexpr u32 MSM_META_WORDS = 4;   // [0] rejected points, [1] segments in use

struct MsmPlan {
    u32 c, windows, buckets, seg, chunk, chunks, entries, max_segments;
    u32 n;
    size_t o_meta, o_count, o_cursor, o_off, o_segoff, o_skip, o_idx, o_partial, o_bucket, o_chunkpart, o_winsum, total;
    uint64_t max_lane_additions;
};

// AUTO (MEASUREMENTS.md section 12): floor(log2 n) - 4 within [5, 10], and 9 instead of 8.  10 is the fastest forced width of
// the sweep at n = 2^16 and at 2^20 on both curves.  Widths that divide 256 are avoided: their top window holds nothing but
// the carry, so half of all points meet in ONE bucket there, whose n / (2 seg) partials a single lane of launch 5 adds
// (8 bits at 2^20: 35.6 ms against 12.7 ms at 9 bits).  Below 2^15 the rule is reasoning, not measurement: fewer points
// than that do not fill the buckets of a wider window, and the n-independent tail grows with the width.
P2E_HD unsigned msm_auto_window(size_t n) {
    unsigned lg = 0;
    while (lg < 63 && ((size_t)2 << lg) <= n) lg++;   // floor(log2 n), 0 for n <= 1
    const unsigned c = lg > 4 ? lg - 4 : 0;
    return c < 5 ? 5 : c > 10 ? 10 : c == 8 ? 9 : c;
}

inline MsmPlan msm_plan(size_t n, unsigned c) {
    MsmPlan p;
    p.c = c;
    p.n = (u32)n;
    p.windows = 256 / c + 1;
    p.buckets = 1u << (c - 1);
    // seg: half of sqrt(n) as a power of two, within [32, 256]: both seg and the worst bucket's n / seg partials stay short
    unsigned lg = 0;
    while (lg < 63 && ((size_t)2 << lg) <= n) lg++;
    const u32 s = lg >= 2 ? 1u << (lg / 2 - 1) : 1;
    p.seg = s < 32 ? 32 : s > 256 ? 256 : s;
    p.chunk = p.buckets < 32 ? p.buckets : 32;
    p.chunks = p.buckets / p.chunk;
    p.entries = p.windows * p.buckets;
    p.max_segments = p.entries + (u32)(((uint64_t)p.windows * n) / p.seg);   // sum ceil(count_e / seg) <= entries + sum count_e / seg
    size_t at = 0;
    auto take = [&](size_t bytes) {
        const size_t o = at;
        at += (bytes + 255) & ~(size_t)255;
        return o;
    };
    p.o_meta = take(MSM_META_WORDS * 4);
    p.o_count = take((size_t)p.entries * 4);
    p.o_cursor = take((size_t)p.entries * 4);   // (meta, count, cursor: one memset per call)
    p.o_off = take(((size_t)p.entries + 1) * 4);
    p.o_segoff = take(((size_t)p.entries + 1) * 4);
    p.o_skip = take(n);
    p.o_idx = take((size_t)p.windows * n * 4);
    p.o_partial = take((size_t)p.max_segments * sizeof(Jac));
    p.o_bucket = take((size_t)p.entries * sizeof(Jac));
    p.o_chunkpart = take((size_t)p.windows * p.chunks * sizeof(Jac));
    p.o_winsum = take((size_t)p.windows * sizeof(Jac));
    p.total = at;
    // per launch: 4: seg additions; 5: ceil(n / seg) (a bucket holds at most n entries); 6: 2 chunk running-sum additions,
    // c - 1 doublings and c - 1 additions for a0 S (a0 < 2^(c-1)), one to join; 7: chunks additions per window lane, then
    // c W doublings and W additions in lane 0
    const uint64_t l4 = p.seg, l5 = (n + p.seg - 1) / p.seg, l6 = 2ull * p.chunk + 2ull * (c - 1) + 1;
    const uint64_t l7 = (uint64_t)p.chunks + (uint64_t)p.windows * (c + 1);
    uint64_t m = l4 > l5 ? l4 : l5;
    m = m > l6 ? m : l6;
    p.max_lane_additions = m > l7 ? m : l7;
    return p;
}

// what a kernel sees: the plan's numbers and the scratch pointers
struct MsmArgs {
    u32 c, windows, buckets, seg, chunk, chunks, entries, max_segments, n;
    const uint8_t *k32, *px32, *py32;
    u32 *meta, *count, *cursor, *off, *segoff, *idx;
    uint8_t* skip;
    Jac *partial, *bucket, *chunkpart, *winsum;
    uint8_t *outx32, *outy32, *status, *point_err;
    unsigned long long* counter;
};
inline MsmArgs msm_args(const MsmPlan& p, void* scratch) {
    char* b = static_cast<char*>(scratch);
    MsmArgs a = {};
    a.c = p.c, a.windows = p.windows, a.buckets = p.buckets, a.seg = p.seg, a.chunk = p.chunk, a.chunks = p.chunks;
    a.entries = p.entries, a.max_segments = p.max_segments, a.n = p.n;
    a.meta = (u32*)(b + p.o_meta), a.count = (u32*)(b + p.o_count), a.cursor = (u32*)(b + p.o_cursor);
    a.off = (u32*)(b + p.o_off), a.segoff = (u32*)(b + p.o_segoff), a.idx = (u32*)(b + p.o_idx);
    a.skip = (uint8_t*)(b + p.o_skip);
    a.partial = (Jac*)(b + p.o_partial), a.bucket = (Jac*)(b + p.o_bucket), a.chunkpart = (Jac*)(b + p.o_chunkpart);
    a.winsum = (Jac*)(b + p.o_winsum);
    return a;
}

P2E_HD u32 msm_fetch_add(u32* p, u32 v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return atomicAdd(p, v);
#else
    return __atomic_fetch_add(p, v, __ATOMIC_RELAXED);
#endif
}

// f(w, b, neg) for every non-zero signed digit of k (canonical), least significant window first; b = |d| - 1.
// The digit is always the low c bits of word 0: the words move down c bits per window (no dynamic register index).
template <class Fn>
P2E_HD void msm_for_digits(U256 k, u32 c, u32 windows, Fn&& f) {
    const u32 mask = (1u << c) - 1, half = 1u << (c - 1);
    u32 carry = 0;
    for (u32 w = 0; w < windows; w++) {
        const u32 d = (k.w[0] & mask) + carry;   // <= 2^c
        P2E_UNROLL
        for (int j = 0; j < 7; j++) k.w[j] = (k.w[j] >> c) | (k.w[j + 1] << (32 - c));
        k.w[7] >>= c;
        carry = d > half ? 1u : 0u;
        const u32 mag = carry ? (1u << c) - d : d;
        if (mag) f(w, mag - 1, carry != 0);
    }
}

// ---- points ------------------------------------------------------------------------------------------------------------
template <class CV>
P2E_HD SignSum<CV> msm_neutral() {
    SignSum<CV> s;
    s.p = SignArith<CV>::zero();
    s.have = false;
    return s;
}
template <class CV>
P2E_HD SignSum<CV> msm_load(const Jac* src) {   // Z = 0: the neutral element
    typedef RecField<CV> FA;
    const Jac j = *src;
    SignSum<CV> s;
    s.have = !u256_is_zero(j.Z);
    s.p.X = FA::from(j.X);
    s.p.Y = FA::from(j.Y);
    s.p.Z = FA::from(j.Z);
    return s;
}
template <class CV>
P2E_HD void msm_store(Jac* dst, const SignSum<CV>& s) {
    Jac j = SignArith<CV>::canon(s.p);
    if (!s.have) j.X = j.Y = j.Z = u256_zero();
    *dst = j;
}
template <class CV>
P2E_HD SignSum<CV> msm_select(bool c, const SignSum<CV>& t, const SignSum<CV>& f) {   // (register selects: no private memory)
    SignSum<CV> r;
    r.p = SignArith<CV>::select(c, t.p, f.p);
    r.have = c ? t.have : f.have;
    return r;
}
template <class CV>
P2E_HD SignSum<CV> msm_dbl(const SignSum<CV>& a) {
    P2E_MSM_NOTE_OP();
    SignSum<CV> r = a;
    if (a.have) r.p = SignArith<CV>::dbl(a.p);   // (Z3 = 2 Y Z != 0: Z != 0 under `have`, and y = 0 is on neither curve)
    return r;
}
// a + b, complete (see the header).  MIXED: b.p.Z = 1.
template <class CV, bool MIXED>
P2E_HD SignSum<CV> msm_add(const SignSum<CV>& a, const SignSum<CV>& b) {
    typedef SignArith<CV> A;
    typedef RecField<CV> FA;
    typedef typename FA::E E;
    P2E_MSM_NOTE_OP();
    if (!b.have) return a;
    if (!a.have) return b;
    const E zz1 = FA::sqr(a.p.Z);
    const E u2 = FA::mul(b.p.X, zz1), s2 = FA::mul(b.p.Y, FA::mul(zz1, a.p.Z));
    E u1 = a.p.X, s1 = a.p.Y;
    if (!MIXED) {
        const E zz2 = FA::sqr(b.p.Z);
        u1 = FA::mul(a.p.X, zz2);
        s1 = FA::mul(a.p.Y, FA::mul(zz2, b.p.Z));
    }
    const E h = FA::sub(u2, u1), r = FA::sub(s2, s1);
    SignSum<CV> o;
    if (!u256_is_zero(FA::canon(h))) {
        const E h2 = FA::sqr(h), h3 = FA::mul(h2, h), v = FA::mul(u1, h2);
        o.p.X = FA::sub(FA::sub(FA::sub(FA::sqr(r), h3), v), v);
        o.p.Y = FA::sub(FA::mul(r, FA::sub(v, o.p.X)), FA::mul(s1, h3));
        o.p.Z = FA::mul(MIXED ? a.p.Z : FA::mul(a.p.Z, b.p.Z), h);
        o.have = true;
    } else if (u256_is_zero(FA::canon(r))) {
        o.p = A::dbl(b.p);
        o.have = true;
    } else {
        o = msm_neutral<CV>();
    }
    return o;
}

// ---- launch 1: validate, count --------------------------------------------------------------------------------------------
template <class CV>
P2E_HD bool msm_on_curve(const U256& x, const U256& y) {
    typedef typename CV::Fp F;
    if (geq_mod<F>(x.w) || geq_mod<F>(y.w)) return false;
    U256 t = fe_mul<F>(fe_sqr<F>(x), x);
    if (!CV::kAZero) t = fe_add<F>(t, fe_mul<F>(CV::a(), x));
    t = fe_add<F>(t, CV::b());
    return u256_eq(fe_sqr<F>(y), t);
}
template <class CV>
P2E_HD void body_msm_digits(const MsmArgs& a, size_t i) {
    const U256 x = load_packed(a.px32, i), y = load_packed(a.py32, i);
    const bool neutral = u256_is_zero(x) && u256_is_zero(y);
    const bool bad = !neutral && !msm_on_curve<CV>(x, y);
    if (a.point_err) a.point_err[i] = bad ? 1 : 0;
    a.skip[i] = (neutral || bad) ? 1 : 0;
    if (bad) msm_fetch_add(&a.meta[0], 1u);
    if (neutral || bad) return;
    const U256 k = sign_scalar<CV>(a.k32, i);
    msm_for_digits(k, a.c, a.windows, [&](u32 w, u32 b, bool) { msm_fetch_add(&a.count[w * a.buckets + b], 1u); });
}

// ---- launch 2: scans (lane t of MSM_SCAN_LANES owns entries [t per, (t + 1) per)) ----------------------------------------------
P2E_HD u32 msm_scan_per(const MsmArgs& a) { return (a.entries + MSM_SCAN_LANES - 1) / MSM_SCAN_LANES; }
P2E_HD void body_msm_scan_local(const MsmArgs& a, u32 t, u32& cnt, u32& segs) {
    const u32 per = msm_scan_per(a);
    cnt = segs = 0;
    for (u32 e = t * per; e < (t + 1) * per && e < a.entries; e++) {
        cnt += a.count[e];
        segs += (a.count[e] + a.seg - 1) / a.seg;
    }
}
P2E_HD void body_msm_scan_write(const MsmArgs& a, u32 t, u32 cnt, u32 segs) {   // cnt, segs: the totals of the lanes below t
    const u32 per = msm_scan_per(a);
    for (u32 e = t * per; e < (t + 1) * per && e < a.entries; e++) {
        a.off[e] = cnt;
        a.segoff[e] = segs;
        cnt += a.count[e];
        segs += (a.count[e] + a.seg - 1) / a.seg;
    }
    if (t == MSM_SCAN_LANES - 1) {
        a.off[a.entries] = cnt;
        a.segoff[a.entries] = segs;
        a.meta[1] = segs;
    }
}

// ---- launch 3: scatter ----------------------------------------------------------------------------------------------------
template <class CV>
P2E_HD void body_msm_scatter(const MsmArgs& a, size_t i) {
    if (a.skip[i]) return;
    const U256 k = sign_scalar<CV>(a.k32, i);
    const u32 cap = a.windows * a.n;
    msm_for_digits(k, a.c, a.windows, [&](u32 w, u32 b, bool neg) {
        const u32 e = w * a.buckets + b;
        const u32 pos = a.off[e] + msm_fetch_add(&a.cursor[e], 1u);
        if (pos < cap) a.idx[pos] = (u32)i | (neg ? MSM_NEG : 0u);   // (always: the counts are those of launch 1)
    });
}

// ---- launch 4: segment sums ---------------------------------------------------------------------------------------------
template <class CV>
P2E_HD Aff msm_fetch_point(const MsmArgs& a, u32 id) {
    const size_t i = id & ~MSM_NEG;
    Aff p;
    p.x = load_packed(a.px32, i);
    p.y = load_packed(a.py32, i);
    if (id & MSM_NEG) p.y = fe_neg<typename CV::Fp>(p.y);
    return p;
}
template <class CV>
P2E_HD void body_msm_segment(const MsmArgs& a, u32 s) {
    if (s >= a.meta[1] || s >= a.max_segments) return;
    u32 lo = 0, hi = a.entries;   // the bucket e with segoff[e] <= s < segoff[e + 1]
    while (hi - lo > 1) {
        const u32 mid = (lo + hi) >> 1;
        if (a.segoff[mid] <= s)
            lo = mid;
        else
            hi = mid;
    }
    const u32 e = lo, end_e = a.off[e + 1];
    const u32 begin = a.off[e] + (s - a.segoff[e]) * a.seg;
    const u32 end = begin + a.seg < end_e ? begin + a.seg : end_e;
    SignSum<CV> acc = msm_neutral<CV>();
    Aff nxt = msm_fetch_point<CV>(a, a.idx[begin]);   // (begin < end: a segment in use is not empty)
    for (u32 t = begin; t < end; t++) {
        const Aff cur = nxt;
        if (t + 1 < end) nxt = msm_fetch_point<CV>(a, a.idx[t + 1]);   // fetched before the addition it follows
        SignSum<CV> q;
        q.p = SignArith<CV>::from_aff(cur);
        q.have = true;
        acc = msm_add<CV, true>(acc, q);
    }
    msm_store<CV>(&a.partial[s], acc);
}

// ---- launch 5: bucket sums ----------------------------------------------------------------------------------------------
template <class CV>
P2E_HD void body_msm_bucket(const MsmArgs& a, u32 e) {
    SignSum<CV> acc = msm_neutral<CV>();
    for (u32 s = a.segoff[e]; s < a.segoff[e + 1]; s++) acc = msm_add<CV, false>(acc, msm_load<CV>(&a.partial[s]));
    msm_store<CV>(&a.bucket[e], acc);
}

// ---- launch 6: chunk reduction (lane t = w chunks + ch) -----------------------------------------------------------------------
template <class CV>
P2E_HD void body_msm_chunk(const MsmArgs& a, u32 t) {
    const u32 w = t / a.chunks, ch = t % a.chunks, a0 = ch * a.chunk;
    const Jac* B = a.bucket + (size_t)w * a.buckets + a0;
    // run = B[chunk - 1] + ... + B[b], acc = sum of the runs = sum (b + 1) B[b]; one addition site serves both steps
    SignSum<CV> run = msm_neutral<CV>(), acc = msm_neutral<CV>();
    for (u32 it = 0; it < 2 * a.chunk; it++) {
        const bool second = (it & 1) != 0;
        const SignSum<CV> next = msm_load<CV>(&B[a.chunk - 1 - (it >> 1)]);
        const SignSum<CV> sum = msm_add<CV, false>(msm_select<CV>(second, acc, run), msm_select<CV>(second, run, next));
        acc = msm_select<CV>(second, sum, acc);
        run = msm_select<CV>(second, run, sum);
    }
    // a0 run, most significant bit first (a0 < 2^(c - 1))
    SignSum<CV> m = msm_neutral<CV>();
    for (int bit = (int)a.c - 2; bit >= 0; bit--) {
        m = msm_dbl<CV>(m);
        if ((a0 >> bit) & 1u) m = msm_add<CV, false>(m, run);
    }
    msm_store<CV>(&a.chunkpart[t], msm_add<CV, false>(acc, m));
}

// ---- launch 7: window sums, combination, the one inversion -------------------------------------------------------------------
template <class CV>
P2E_HD void body_msm_window(const MsmArgs& a, u32 w) {
    SignSum<CV> acc = msm_neutral<CV>();
    for (u32 ch = 0; ch < a.chunks; ch++) acc = msm_add<CV, false>(acc, msm_load<CV>(&a.chunkpart[w * a.chunks + ch]));
    msm_store<CV>(&a.winsum[w], acc);
}
template <class CV>
P2E_HD void body_msm_final(const MsmArgs& a) {
    const u32 bad = a.meta[0];
    U256 x = u256_zero(), y = u256_zero();
    uint8_t st = MSM_BAD_POINT;
    if (!bad) {
        SignSum<CV> acc = msm_neutral<CV>();
        for (int bit = (int)(a.windows * a.c) - 1; bit >= 0; bit--) {
            acc = msm_dbl<CV>(acc);
            if ((u32)bit % a.c == 0) acc = msm_add<CV, false>(acc, msm_load<CV>(&a.winsum[(u32)bit / a.c]));
        }
        st = MSM_NEUTRAL;
        if (acc.have && sign_to_affine<CV, true>(acc, x, y))
            st = MSM_OK;
        else
            x = y = u256_zero();   // (Z = 0 under `have` cannot occur; it would be the neutral element, never a point)
    }
    store_packed(a.outx32, 0, x);
    store_packed(a.outy32, 0, y);
    *a.status = st;
    *a.counter = bad;
}

#if defined(__HIPCC__)
template <class CV>
__global__ __launch_bounds__(256) void k_msm_digits(MsmArgs a) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < a.n) body_msm_digits<CV>(a, i);
}
template <int UNUSED = 0>   // (a template so that the translation units that include this file do not each define it)
__global__ __launch_bounds__(MSM_SCAN_LANES) void k_msm_scan(MsmArgs a) {
    __shared__ u32 cnt[MSM_SCAN_LANES], segs[MSM_SCAN_LANES];
    const u32 t = threadIdx.x;
    u32 c, s;
    body_msm_scan_local(a, t, c, s);
    cnt[t] = c;
    segs[t] = s;
    __syncthreads();
    u32 c0 = 0, s0 = 0;
    for (u32 j = 0; j < t; j++) {
        c0 += cnt[j];
        s0 += segs[j];
    }
    body_msm_scan_write(a, t, c0, s0);
}
template <class CV>
__global__ __launch_bounds__(256) void k_msm_scatter(MsmArgs a) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < a.n) body_msm_scatter<CV>(a, i);
}
template <class CV>
__global__ __launch_bounds__(256) void k_msm_segment(MsmArgs a) {
    const size_t s = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (s < a.max_segments) body_msm_segment<CV>(a, (u32)s);
}
template <class CV>
__global__ __launch_bounds__(256) void k_msm_bucket(MsmArgs a) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e < a.entries) body_msm_bucket<CV>(a, (u32)e);
}
template <class CV>
__global__ __launch_bounds__(256) void k_msm_chunk(MsmArgs a) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t < (size_t)a.windows * a.chunks) body_msm_chunk<CV>(a, (u32)t);
}
template <class CV>
__global__ __launch_bounds__(MSM_FINAL_LANES) void k_msm_final(MsmArgs a) {
    if (threadIdx.x < a.windows) body_msm_window<CV>(a, threadIdx.x);
    __syncthreads();   // (one block: the window sums written above are visible to lane 0)
    if (threadIdx.x == 0) body_msm_final<CV>(a);
}
#endif

}  // namespace p2e
