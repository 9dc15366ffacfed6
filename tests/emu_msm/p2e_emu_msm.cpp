// CPU harness of the multi-scalar multiplication (test infrastructure only): the kernel bodies of csrc/pmsm.hpp compiled
// with g++ against the library's headers, run launch by launch with the plan, the scratch layout and the index
// arithmetic of the device (msm_plan / msm_args), on either curve.  Every lane's point operations are counted; the
// maximum over the lanes of each of the seven launches is exported beside the result.
#include <cstdint>
#include <cstring>
#include <vector>

namespace {
thread_local unsigned long long msm_lane_ops;
}
#define P2E_MSM_NOTE_OP() (++msm_lane_ops)

#include "../../plonky2-ecdsa_amd/csrc/consts.hpp"
#include "../../plonky2-ecdsa_amd/csrc/curve_program.hpp"
#include "../../plonky2-ecdsa_amd/csrc/pmsm.hpp"

using namespace p2e;

namespace {
// body(lane) for every lane of a launch; returns the largest number of point operations one lane performed
template <class Body>
unsigned long long run_lanes(size_t lanes, Body&& body) {
    unsigned long long worst = 0;
#pragma omp parallel for schedule(dynamic, 16) reduction(max : worst)
    for (long long t = 0; t < (long long)lanes; t++) {
        msm_lane_ops = 0;
        body((size_t)t);
        if (msm_lane_ops > worst) worst = msm_lane_ops;
    }
    return worst;
}
bool bad_args(int curve, size_t n, unsigned wb) {
    return (curve != 0 && curve != 1) || (wb != 0 && (wb < MSM_WINDOW_MIN || wb > MSM_WINDOW_MAX)) || n > MSM_MAX_N;
}
template <class CV>
long run_msm(unsigned wb, const uint8_t* k, const uint8_t* px, const uint8_t* py, size_t n, uint8_t* outx, uint8_t* outy, uint8_t* status,
             uint8_t* point_err, uint64_t* lane_ops) {
    const MsmPlan P = msm_plan(n, wb ? wb : msm_auto_window(n));
    std::vector<unsigned char> scratch(P.total, 0xCD);   // (the device's block is not zeroed either)
    std::memset(scratch.data(), 0, P.o_off);             // meta, count, cursor: the call's one memset
    unsigned long long counter = 0;
    MsmArgs a = msm_args(P, scratch.data());
    a.k32 = k, a.px32 = px, a.py32 = py;
    a.outx32 = outx, a.outy32 = outy, a.status = status, a.point_err = point_err;
    a.counter = &counter;
    uint64_t ops[7] = {};
    ops[0] = run_lanes(n, [&](size_t i) { body_msm_digits<CV>(a, i); });
    u32 cnt[MSM_SCAN_LANES], segs[MSM_SCAN_LANES];
    for (u32 t = 0; t < MSM_SCAN_LANES; t++) body_msm_scan_local(a, t, cnt[t], segs[t]);
    for (u32 t = 0, c0 = 0, s0 = 0; t < MSM_SCAN_LANES; t++) {
        body_msm_scan_write(a, t, c0, s0);
        c0 += cnt[t];
        s0 += segs[t];
    }
    ops[2] = run_lanes(n, [&](size_t i) { body_msm_scatter<CV>(a, i); });
    if (n) ops[3] = run_lanes(a.max_segments, [&](size_t s) { body_msm_segment<CV>(a, (u32)s); });
    ops[4] = run_lanes(a.entries, [&](size_t e) { body_msm_bucket<CV>(a, (u32)e); });
    ops[5] = run_lanes((size_t)a.windows * a.chunks, [&](size_t t) { body_msm_chunk<CV>(a, (u32)t); });
    // the last launch: lanes [0, windows) sum their window, then lane 0 goes on alone (its operations add up)
    unsigned long long lane0 = 0;
    ops[6] = run_lanes(a.windows, [&](size_t w) {
        body_msm_window<CV>(a, (u32)w);
        if (w == 0) lane0 = msm_lane_ops;
    });
    msm_lane_ops = 0;
    body_msm_final<CV>(a);
    if (lane0 + msm_lane_ops > ops[6]) ops[6] = lane0 + msm_lane_ops;
    if (lane_ops) std::memcpy(lane_ops, ops, sizeof ops);
    return (long)counter;
}
}  // namespace

// include/p2e.h p2e_point_msm without a context; lane_ops (nullable): seven words, see the top of the file.  -1: bad arguments
extern "C" long emum_point_msm(int curve, unsigned window_bits, const uint8_t* k, const uint8_t* px, const uint8_t* py, size_t n,
                               uint8_t* outx, uint8_t* outy, uint8_t* status, uint8_t* point_err, uint64_t* lane_ops) {
    if (bad_args(curve, n, window_bits) || !k || !px || !py || !outx || !outy || !status) return -1;
    return curve == 0 ? run_msm<Secp256k1>(window_bits, k, px, py, n, outx, outy, status, point_err, lane_ops)
                      : run_msm<P256>(window_bits, k, px, py, n, outx, outy, status, point_err, lane_ops);
}
// the plan this build runs, in the order of include/p2e.h P2E_MSM_PLAN_*
extern "C" int emum_plan(int curve, size_t n, unsigned window_bits, uint64_t* plan) {
    if (bad_args(curve, n, window_bits) || !plan) return -1;
    const MsmPlan P = msm_plan(n, window_bits ? window_bits : msm_auto_window(n));
    const uint64_t v[6] = {P.c, P.windows, P.buckets, P.seg, P.total, P.max_lane_additions};
    std::memcpy(plan, v, sizeof v);
    return 0;
}
