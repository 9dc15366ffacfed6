// libp2e_hip.so: gfx950 kernels + the C ABI of include/p2e.h.
// One process drives one GPU; every entry point enqueues on the context's stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/p2e.h"
#include "aux.hpp"
#include "consts.hpp"
#include "device_array.hpp"
#include "knobs.hpp"
#include "overlap.hpp"
#include "call_args.hpp"
#include "launch_plan.hpp"
#include "pipeline.hpp"
#include "prims.hpp"
#include "quad.hpp"
#include "schedule.hpp"
#include "curve_program.hpp"
#include "sign.hpp"
#include "recover.hpp"
#include "pmsm.hpp"
#include "point_arith.hpp"
#include "point_table.hpp"
#include "schnorr.hpp"
#include "taproot.hpp"
#include "sp.hpp"
#include "dleq.hpp"
#include "musig.hpp"
#include "hd.hpp"
#include "kdf.hpp"
#include "hash.hpp"
#include "wire.hpp"

using namespace p2e;
using host::COMPACT_WIDE;

// The library is ONE source compiled as four translation units in parallel (plonky2_ecdsa_amd.build: -DP2E_PART=0..3),
// because a single hipcc job over all kernels takes five minutes:  0 = context, single generators, layout helpers,
// streaming passes, descriptions;  1 = the fused pipeline of the two built-in programs (run_program);  2 / 3 = the
// curve-program pipeline instantiated for secp256k1 / P-256 (run_curve_program<CV>).  Undefined = everything in one
// unit.  The hashing, nonce and address kernels (hash.hpp) and the key and signature codecs (wire.hpp) ride in part 1, the part that builds fastest; the BIP-340 and Taproot kernels (schnorr.hpp, taproot.hpp) ride in part 3; the BIP-32 and HASH160 kernels (hd.hpp) ride in part 1 with the other hashes, and so do the silent-payment and MuSig2 kernels (sp.hpp, musig.hpp), beside the point multiplication whose walk they hold.  Small static helpers (error text, staging, scratch) are compiled into every part.
#ifndef P2E_PART
#define P2E_PART (-1)
#endif
#define P2E_HAS(p) (P2E_PART < 0 || P2E_PART == (p))

// ====================================================================================================
// kernels
// ====================================================================================================
constexpr int BS = 256;          // 4 waves per workgroup

// Signature owned by this lane.  WIDE kernels (full workgroups only) give lanes l and l+32 of a wave
// adjacent signatures so that column pairs can be written with 16-byte stores (PairEmit); the narrow
// variants cover the ragged tail of the batch (first = first signature of the launch).
template <bool WIDE>
__device__ __forceinline__ size_t lane_sig(size_t first) {
    unsigned t = threadIdx.x;
    // (An XCD-contiguous remap of blockIdx -- every XCD owning one contiguous eighth of the batch -- was
    // measured 2.5 % SLOWER on k_expand than the plain round-robin order and is not used.)
    size_t base = first + (size_t)blockIdx.x * BS;
    if (WIDE) return base + (t & ~63u) + 2u * (t & 31u) + ((t >> 5) & 1u);
    return base + t;
}
// MODE of the emitting kernels: bit 0 = paired stores over full workgroups (else one signature per lane, ragged tail),
// bit 1 = compact container (u32 narrow + u64 wide matrices) instead of the u64 column matrix
template <int MODE> struct EmitOf;
template <> struct EmitOf<0> { typedef Emit type; };
template <> struct EmitOf<1> { typedef PairEmit type; };
template <> struct EmitOf<2> { typedef CompactEmit type; };
template <> struct EmitOf<3> { typedef CompactPairEmit type; };
template <> struct EmitOf<4> { typedef NullEmit type; };   // no witness: p2e_ecdsa_verify_batch
#if P2E_HAS(1)
template <int MODE>
__global__ __launch_bounds__(BS) void k_scalar(Program G, Buffers B, size_t first) {
    size_t i = lane_sig<(MODE & 1) != 0>(first);
    if ((MODE & 1) || i < B.n) body_scalar<typename EmitOf<MODE>::type>(G, B, i);
}
// ops [lo, hi) of a chain, sequential per lane
__global__ __launch_bounds__(BS) void k_chains(Program G, Buffers B, int lo, int hi, int table_affine, int continue_prefix) {
    // the chain is the critical path of the whole call and shares its SIMD with phase B/C waves of
    // earlier pieces: win every issue arbitration against them
    __builtin_amdgcn_s_setprio(3);
    size_t i = (size_t)blockIdx.x * BS + threadIdx.x;
#ifdef P2E_LDS_FBTAB
    // experiment: the fixed-base table rows of this piece's windows staged in LDS
    constexpr int MAXW = 36;
    __shared__ Aff s_fb[MAXW * 16];
    const OpDesc first = load_op(B.ops, lo);
    const bool fb = first.kind != OP_DBL && ref_kind(first.ref2) == R_FBTAB && hi - lo <= MAXW;
    const u32 w0 = ref_id(first.ref2);
    if (fb) {
        const int nwin = (hi - lo) < (int)(FB_WINDOWS - w0) ? (hi - lo) : (int)(FB_WINDOWS - w0);
        const u32* src = reinterpret_cast<const u32*>(B.fbtab + (size_t)w0 * 16);
        u32* dst = reinterpret_cast<u32*>(s_fb);
        for (int k = threadIdx.x; k < nwin * 16 * 16; k += BS) dst[k] = src[k];
    }
    __syncthreads();
    if (i < B.n) body_chain_range(G, B, i, lo, hi, table_affine != 0, continue_prefix != 0, fb ? s_fb : nullptr, w0);
#else
    if (i < B.n) body_chain_range(G, B, i, lo, hi, table_affine != 0, continue_prefix != 0);
#endif
}
// small batches: four lanes per signature (quad.hpp); the four lanes of a quad are consecutive threads
__global__ __launch_bounds__(BS) void k_chains_quad(Program G, Buffers B, int lo, int hi, int table_affine, int continue_prefix) {
    __builtin_amdgcn_s_setprio(3);
    const size_t g = (size_t)blockIdx.x * BS + threadIdx.x;
    const size_t i = g >> 2;
    if (i < B.n) body_chain_range_quad(G, B, i, (int)(g & 3), lo, hi, table_affine != 0, continue_prefix != 0);
}
// one inversion batch cut into 2^split_log2 sub-ranges, one lane each
__global__ __launch_bounds__(BS) void k_batch_inv_split(Program G, Buffers B, int lo, int hi, int have_prefix, int split_log2) {
    const size_t g = (size_t)blockIdx.x * BS + threadIdx.x;
    const size_t i = g >> split_log2;
    if (i < B.n) body_batch_inv_split(G, B, i, lo, hi, have_prefix != 0, (int)(g & ((1u << split_log2) - 1)), 1 << split_log2);
}
// independent interleaved sub-chains of a piece, one per blockIdx.y (the MSM window table)
__global__ __launch_bounds__(BS) void k_chain_rows(Program G, Buffers B, int lo, int count) {
    __builtin_amdgcn_s_setprio(3);
    size_t i = (size_t)blockIdx.x * BS + threadIdx.x;
    if (i < B.n) body_chain_rows(G, B, i, lo, (int)gridDim.y, (int)blockIdx.y, count);
}
// one inversion batch: ops [lo, hi); have_prefix: phase A has already left its prefix products in PREF
__global__ __launch_bounds__(BS) void k_batch_inv(Program G, Buffers B, int lo, int hi, int have_prefix) {
    size_t i = (size_t)blockIdx.x * BS + threadIdx.x;
    if (i < B.n) body_batch_inv(G, B, i, lo, hi, have_prefix != 0);
}
// op lo + blockIdx.y
template <int MODE>
__global__ __launch_bounds__(BS) void k_expand(Program G, Buffers B, int lo, size_t first) {
#ifdef P2E_EXPAND_PRIO
    __builtin_amdgcn_s_setprio(P2E_EXPAND_PRIO);   // experiment: issue priority of the expansion waves
#endif
    size_t i = lane_sig<(MODE & 1) != 0>(first);
#ifdef P2E_LDS_FBTAB
    // experiment: the 16 table entries of this op's window staged in LDS (one op per workgroup row)
    __shared__ Aff s_fb[16];
    const OpDesc op0 = load_op(B.ops, lo + (int)blockIdx.y);
    const bool fb = op0.kind != OP_DBL && ref_kind(op0.ref2) == R_FBTAB;
    if (fb) reinterpret_cast<u32*>(s_fb)[threadIdx.x] = reinterpret_cast<const u32*>(B.fbtab + (size_t)ref_id(op0.ref2) * 16)[threadIdx.x];
    __syncthreads();
    if ((MODE & 1) || i < B.n) body_expand<typename EmitOf<MODE>::type>(G, B, i, lo + (int)blockIdx.y, fb ? s_fb : nullptr);
#else
    if ((MODE & 1) || i < B.n) body_expand<typename EmitOf<MODE>::type>(G, B, i, lo + (int)blockIdx.y);
#endif
}
// runs of MSM-loop iterations: run blockIdx.y of the launch covers iterations [it_first + y*R, +R) capped at it_end
template <int MODE>
__global__ __launch_bounds__(BS) void k_expand_runs(Program G, Buffers B, int it_first, int run_iters, int it_end, size_t first) {
#ifdef P2E_EXPAND_PRIO
    __builtin_amdgcn_s_setprio(P2E_EXPAND_PRIO);
#endif
    size_t i = lane_sig<(MODE & 1) != 0>(first);
    int it0 = it_first + (int)blockIdx.y * run_iters;
    int it1 = it0 + run_iters < it_end ? it0 + run_iters : it_end;
    if ((MODE & 1) || i < B.n) body_expand_run<typename EmitOf<MODE>::type>(G, B, i, it0, it1);
}
// all fixed-base windows of a signature as one run (body_expand_fb_run); t_after: the unblinding add
template <int MODE>
__global__ __launch_bounds__(BS) void k_expand_fb_run(Program G, Buffers B, int t_after, size_t first) {
    size_t i = lane_sig<(MODE & 1) != 0>(first);
    if ((MODE & 1) || i < B.n) body_expand_fb_run<typename EmitOf<MODE>::type>(G, B, i, t_after);
}
// p2e_ecdsa_verify_batch: the connect r == x of gadgets/ecdsa.rs:48-52 on the final add's Jacobian result, without an
// inversion: x = X / Z^2 is canonical, so x == r  <=>  r < p and X == r * Z^2 (Z != 0, else phase A flagged the element)
__global__ __launch_bounds__(BS) void k_verify_check(Program G, Buffers B) {
    size_t i = (size_t)blockIdx.x * BS + threadIdx.x;
    if (i < B.n) body_verify_check(G, B, i);
}
#endif   // P2E_HAS(1)
// built-in-generator columns from the finished witness matrix: one (signature, item) per lane (aux.hpp)
// MODE bit 0 = paired stores over full workgroups, bit 1 = u32 output matrix
template <int MODE> struct AuxEmitOf;
template <> struct AuxEmitOf<0> { typedef Emit type; };
template <> struct AuxEmitOf<1> { typedef PairEmit type; };
template <> struct AuxEmitOf<2> { typedef Emit32 type; };
template <> struct AuxEmitOf<3> { typedef PairEmit32 type; };
#if P2E_HAS(0)
template <int MODE>
__global__ __launch_bounds__(BS) void k_aux(AuxArgs A, size_t first) {
    size_t i = lane_sig<(MODE & 1) != 0>(first);
    if ((MODE & 1) || i < A.n) body_aux<typename AuxEmitOf<MODE>::type>(A, (int)blockIdx.y, i);
}
// gate-internal values of the built-in gates, one (signature, window) per lane (aux.hpp body_gate); u64 only (the
// equality gadget's inverse is a full Goldilocks element)
template <int MODE>
__global__ __launch_bounds__(BS) void k_gate(GateArgs A, size_t first) {
    size_t i = lane_sig<(MODE & 1) != 0>(first);
    if ((MODE & 1) || i < A.n) body_gate<typename AuxEmitOf<MODE>::type>(A, (int)blockIdx.y, i);
}
// constraint-block columns from the finished matrices: one (signature, generator) per lane (ux.hpp)
template <int MODE>
__global__ __launch_bounds__(BS) void k_ux(UxArgs A, size_t first) {
    size_t i = lane_sig<(MODE & 1) != 0>(first);
    if ((MODE & 1) || i < A.n) body_ux<typename AuxEmitOf<MODE>::type>(A, (int)blockIdx.y, i);
}
// the same two passes inside the compact container: witness columns from the u32 narrow matrix, aux columns from the
// u32 aux matrix (kernels of their own, so that the u64-source ones stay the code they were)
template <int MODE>
__global__ __launch_bounds__(BS) void k_gate_compact(GateArgs A, size_t first) {
    size_t i = lane_sig<(MODE & 1) != 0>(first);
    if ((MODE & 1) || i < A.n) body_gate<typename AuxEmitOf<MODE>::type, true>(A, (int)blockIdx.y, i);
}
template <int MODE>
__global__ __launch_bounds__(BS) void k_ux_compact(UxArgs A, size_t first) {
    size_t i = lane_sig<(MODE & 1) != 0>(first);
    if ((MODE & 1) || i < A.n) body_ux<typename AuxEmitOf<MODE>::type, true>(A, (int)blockIdx.y, i);
}
#endif   // P2E_HAS(0)
// err words -> caller's err bytes, valid bytes, flagged count (every part launches it: internal linkage)
static __global__ __launch_bounds__(BS) void k_finalize(const u32* err32, const uint8_t* valid8, uint8_t* err_out,
                                                 uint8_t* valid_out, size_t n, unsigned long long* counter) {
    size_t i = (size_t)blockIdx.x * BS + threadIdx.x;
    bool bad = false;
    if (i < n) {
        u32 e = err32[i];
        bad = e != 0;
        if (err_out) err_out[i] = (uint8_t)e;
        if (valid_out) valid_out[i] = bad ? 0 : valid8[i];
    }
    unsigned long long m = __ballot(bad);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(counter, (unsigned long long)__popcll(m));
}

#if P2E_HAS(0)
// one empty wave: makes the runtime bind a hardware queue to a stream NOW (p2e_ctx_create), see there
__global__ void k_touch() {}
__device__ __forceinline__ void count_err(uint8_t e, unsigned long long* counter) {
    unsigned long long m = __ballot(e != 0);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(counter, (unsigned long long)__popcll(m));
}
template <class MOD>
__global__ __launch_bounds__(BS) void k_mul(const u64* x, const u64* y, u64* r, u64* q, u64* cs, u64* b, size_t n,
                                            size_t ld, uint8_t* err, unsigned long long* counter) {
    size_t i = (size_t)blockIdx.x * BS + threadIdx.x;
    uint8_t e = 0;
    if (i < n) {
        e = prim_mul<MOD>(x, y, r, q, cs, b, ld, i);
        err[i] = e;
    }
    count_err(e, counter);
}
__global__ __launch_bounds__(BS) void k_checksum(const u64* a, u64* b, size_t n, size_t ld, uint8_t* err,
                                                 unsigned long long* counter) {
    size_t i = (size_t)blockIdx.x * BS + threadIdx.x;
    uint8_t e = 0;
    if (i < n) {
        e = prim_checksum(a, b, ld, i);
        err[i] = e;
    }
    count_err(e, counter);
}
template <class MOD, bool IS_SUB>
__global__ __launch_bounds__(BS) void k_addsub(const u64* a, const u64* b, u64* out, u64* ov, size_t n, size_t ld,
                                               uint8_t* err, unsigned long long* counter) {
    size_t i = (size_t)blockIdx.x * BS + threadIdx.x;
    uint8_t e = 0;
    if (i < n) {
        e = prim_addsub<MOD, IS_SUB>(a, b, out, ov, ld, i);
        err[i] = e;
    }
    count_err(e, counter);
}
template <class MOD>
__global__ __launch_bounds__(BS) void k_add_many(const u64* s, int k, u64* out, u64* ov, size_t n, size_t ld,
                                                 uint8_t* err, unsigned long long* counter) {
    size_t i = (size_t)blockIdx.x * BS + threadIdx.x;
    uint8_t e = 0;
    if (i < n) {
        e = prim_add_many<MOD>(s, k, out, ov, ld, i);
        err[i] = e;
    }
    count_err(e, counter);
}
template <class MOD>
__global__ __launch_bounds__(BS) void k_inv(const u64* x, u64* inv, u64* div, size_t n, size_t ld, uint8_t* err,
                                            unsigned long long* counter) {
    size_t i = (size_t)blockIdx.x * BS + threadIdx.x;
    uint8_t e = 0;
    if (i < n) {
        e = prim_inv<MOD>(x, inv, div, ld, i);
        err[i] = e;
    }
    count_err(e, counter);
}
__global__ __launch_bounds__(BS) void k_div_rem(const u64* a, int na, const u64* b, int nb, u64* div, u64* rem, size_t n, size_t ld,
                                                uint8_t* err, unsigned long long* counter) {
    size_t i = (size_t)blockIdx.x * BS + threadIdx.x;
    uint8_t e = 0;
    if (i < n) {
        e = prim_div_rem(a, na, b, nb, div, rem, ld, i);
        err[i] = e;
    }
    count_err(e, counter);
}
__global__ __launch_bounds__(BS) void k_glv(const u64* k, u64* k1, u64* k2, u64* n1, u64* n2, size_t n, size_t ld,
                                            uint8_t* err, unsigned long long* counter) {
    size_t i = (size_t)blockIdx.x * BS + threadIdx.x;
    uint8_t e = 0;
    if (i < n) {
        e = prim_glv(k, k1, k2, n1, n2, ld, i);
        err[i] = e;
    }
    count_err(e, counter);
}
// 29-bit limb split: pure streaming, 32 B in + 72 B out per element.  Each lane converts two adjacent
// elements so that every global access is 16 B per lane (64 B contiguous loads, dwordx4 column stores).
__global__ __launch_bounds__(BS) void k_split(const uint8_t* packed, u64* limbs, size_t n, size_t ld) {
    size_t pairs = n >> 1;
    size_t stride = (size_t)gridDim.x * BS;
    bool aligned = ((ld & 1) == 0) && ((reinterpret_cast<uintptr_t>(limbs) & 15) == 0);
    for (size_t p = (size_t)blockIdx.x * BS + threadIdx.x; p < pairs; p += stride) {
        const uint4* src = reinterpret_cast<const uint4*>(packed + 64 * p);
        uint4 a0 = src[0], a1 = src[1], b0 = src[2], b1 = src[3];
        U256 va, vb;
        va.w[0] = a0.x; va.w[1] = a0.y; va.w[2] = a0.z; va.w[3] = a0.w;
        va.w[4] = a1.x; va.w[5] = a1.y; va.w[6] = a1.z; va.w[7] = a1.w;
        vb.w[0] = b0.x; vb.w[1] = b0.y; vb.w[2] = b0.z; vb.w[3] = b0.w;
        vb.w[4] = b1.x; vb.w[5] = b1.y; vb.w[6] = b1.z; vb.w[7] = b1.w;
        u32 la[NL], lb[NL];
        split29(va, la);
        split29(vb, lb);
        if (aligned) {
#pragma unroll
            for (int k = 0; k < NL; k++) {
                uint4 o = make_uint4(la[k], 0u, lb[k], 0u);
                *reinterpret_cast<uint4*>(limbs + (size_t)k * ld + 2 * p) = o;
            }
        } else {
#pragma unroll
            for (int k = 0; k < NL; k++) {
                limbs[(size_t)k * ld + 2 * p] = la[k];
                limbs[(size_t)k * ld + 2 * p + 1] = lb[k];
            }
        }
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) prim_split(packed, limbs, ld, n - 1);
}
__global__ __launch_bounds__(BS) void k_pack(const u64* limbs, uint8_t* packed, size_t n, size_t ld, uint8_t* err,
                                             unsigned long long* counter) {
    size_t i = (size_t)blockIdx.x * BS + threadIdx.x;
    uint8_t e = 0;
    if (i < n) {
        e = prim_pack(limbs, packed, ld, i);
        err[i] = e;
    }
    count_err(e, counter);
}

// Column-major witness matrix -> one contiguous row per signature (what a per-signature PartialWitness
// fill wants to read): 64 x 64 u64 tiles through LDS, both global sides coalesced 512-byte runs.
// Rows of the tile are padded to 65 elements so the transposed read walks distinct banks.
template <class T>
__global__ __launch_bounds__(BS) void k_transpose(const T* __restrict__ cols, size_t ld, size_t n, size_t ncols,
                                                  T* __restrict__ rows, size_t row_ld) {
    __shared__ T tile[64][65];
    const unsigned lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const size_t s0 = (size_t)blockIdx.x * 64, c0 = (size_t)blockIdx.y * 64;
#pragma unroll 4
    for (unsigned r = w; r < 64; r += 4) {   // column c0 + r, signatures s0 .. s0 + 63
        size_t c = c0 + r, sg = s0 + lane;
        if (c < ncols && sg < n) tile[r][lane] = cols[c * ld + sg];
    }
    __syncthreads();
#pragma unroll 4
    for (unsigned r = w; r < 64; r += 4) {   // signature s0 + r, columns c0 .. c0 + 63
        size_t sg = s0 + r, c = c0 + lane;
        if (sg < n && c < ncols) rows[sg * row_ld + c] = tile[lane][r];
    }
}

// Wire-matrix assembly (p2e_assemble_wires): out[sig][dst(e)] = M_src(e)[col(e)][sig] for the entries e of a map
// sorted by dst.  A tile of 64 entries x 64 signatures goes through LDS like k_transpose: the gather side reads 64
// consecutive signatures of one column per row (512 B runs), the scatter side writes, per signature, 64 entries whose
// destinations are consecutive wherever the map is (runs of rows of one wire).
struct AssembleArgs {
    const u64* cols;
    size_t ld;
    const u64* aux;
    size_t ald;
    const void* ux;
    size_t uld;
    int ux_u32;
    const u64* gate;
    size_t gld;
    const u32* src;   // [count]
    const u32* dst;   // [count], ascending
    size_t count;
    u64* wires;
    size_t stride, n;
    // compact sources (k_assemble_compact): src then holds witness entries in compact coordinates (WIRE_CSRC_WIDE | wide
    // row, or the narrow row), aux entries index aux32
    const u32* nar;
    size_t ldn;
    const u64* wide;
    size_t ldw;
    const u32* aux32;
};
constexpr u32 WIRE_CSRC_WIDE = 0x20000000u;   // a witness entry of the compact source table that names a wide row
template <bool CS>
__device__ __forceinline__ void assemble_tile(const AssembleArgs& A) {
    __shared__ u64 tile[64][65];
    const unsigned lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const size_t s0 = (size_t)blockIdx.x * 64, e0 = (size_t)blockIdx.y * 64;
#pragma unroll 4
    for (unsigned r = w; r < 64; r += 4) {   // entry e0 + r, signatures s0 .. s0 + 63
        const size_t e = e0 + r, sg = s0 + lane;
        if (e < A.count && sg < A.n) {
            const u32 s = A.src[e], c = s & 0x3FFFFFFFu;
            u64 v;
            if ((s >> 30) == 0) {
                if (!CS)
                    v = A.cols[(size_t)c * A.ld + sg];
                else if (c & WIRE_CSRC_WIDE)
                    v = A.wide[(size_t)(c & ~WIRE_CSRC_WIDE) * A.ldw + sg];
                else
                    v = A.nar[(size_t)c * A.ldn + sg];
            } else if ((s >> 30) == 1)
                v = CS ? (u64)A.aux32[(size_t)c * A.ald + sg] : A.aux[(size_t)c * A.ald + sg];
            else if ((s >> 30) == 2)
                v = A.ux_u32 ? (u64) static_cast<const u32*>(A.ux)[(size_t)c * A.uld + sg] : static_cast<const u64*>(A.ux)[(size_t)c * A.uld + sg];
            else
                v = A.gate[(size_t)c * A.gld + sg];
            tile[r][lane] = v;
        }
    }
    __syncthreads();
    const size_t e = e0 + lane;
    const u32 d = e < A.count ? A.dst[e] : 0u;
#pragma unroll 4
    for (unsigned r = w; r < 64; r += 4) {   // signature s0 + r, entries e0 .. e0 + 63
        const size_t sg = s0 + r;
        if (sg < A.n && e < A.count) A.wires[sg * A.stride + d] = tile[lane][r];
    }
}
__global__ __launch_bounds__(BS) void k_assemble(AssembleArgs A) { assemble_tile<false>(A); }
__global__ __launch_bounds__(BS) void k_assemble_compact(AssembleArgs A) { assemble_tile<true>(A); }

// Compact container for transfers (p2e_columns_compact): every column whose values are < 2^32 by construction
// (29-bit limbs, overflow words, flags: 57 % of the columns) is repacked as u32, the check_sum / carry columns of
// the mul generators stay u64.  map[c] = index of column c in its matrix | P2E_COMPACT_WIDE.  One lane moves two
// adjacent signatures (16-byte loads, 8- or 16-byte stores); blockIdx.y walks groups of 32 columns.
constexpr int COMPACT_GROUP = 32;
__global__ __launch_bounds__(BS) void k_compact(const u64* __restrict__ cols, size_t ld, size_t n, u32 ncols,
                                                const u32* __restrict__ map, u32* __restrict__ narrow, size_t ldn,
                                                u64* __restrict__ wide, size_t ldw, u32* err32, int pair_ok) {
    const size_t i = ((size_t)blockIdx.x * BS + threadIdx.x) * 2;
    if (i >= n) return;
    const bool two = pair_ok && i + 1 < n;
    const u32 c0 = blockIdx.y * COMPACT_GROUP;
    u32 bad_a = 0, bad_b = 0;   // high words seen in narrow columns, per signature of the lane
#pragma unroll 4
    for (u32 k = 0; k < COMPACT_GROUP; k++) {
        const u32 c = c0 + k;
        if (c >= ncols) break;
        const u32 m = map[c];
        const u64* src = cols + (size_t)c * ld + i;
        u64 a, b = 0;
        if (two) {
            const uint4 v = *reinterpret_cast<const uint4*>(src);
            a = (u64)v.x | ((u64)v.y << 32);
            b = (u64)v.z | ((u64)v.w << 32);
        } else {
            a = src[0];
            if (i + 1 < n) b = src[1];
        }
        if (m & COMPACT_WIDE) {
            u64* dst = wide + (size_t)(m & ~COMPACT_WIDE) * ldw + i;
            if (two) {
                *reinterpret_cast<uint4*>(dst) = make_uint4((u32)a, (u32)(a >> 32), (u32)b, (u32)(b >> 32));
            } else {
                dst[0] = a;
                if (i + 1 < n) dst[1] = b;
            }
        } else {
            bad_a |= (u32)(a >> 32);
            bad_b |= (u32)(b >> 32);
            u32* dst = narrow + (size_t)m * ldn + i;
            if (two) {
                *reinterpret_cast<uint2*>(dst) = make_uint2((u32)a, (u32)b);
            } else {
                dst[0] = (u32)a;
                if (i + 1 < n) dst[1] = (u32)b;
            }
        }
    }
    // a value that does not fit its 32-bit slot
    if (bad_a) atomicOr(&err32[i], (u32)ERR_LIMB_RANGE);
    if (bad_b) atomicOr(&err32[i + 1], (u32)ERR_LIMB_RANGE);
}
#endif   // P2E_HAS(0)

// ====================================================================================================
// context
// ====================================================================================================
#if P2E_HAS(0)
thread_local std::string g_last_error;
#else
extern thread_local std::string g_last_error;
#endif
static void set_error(const std::string& s) { g_last_error = s; }
// what: the text that names the failing call (HIP_TRY: the expression itself)
#define HIP_TRY_AS(what, expr)                                                               \
    do {                                                                                     \
        hipError_t _e = (expr);                                                              \
        if (_e != hipSuccess) {                                                              \
            set_error(std::string(what) + ": " + hipGetErrorString(_e));                     \
            return P2E_E_HIP;                                                                \
        }                                                                                    \
    } while (0)
#define HIP_TRY(expr) HIP_TRY_AS(#expr, expr)

// Entry points run on the context's device and leave the caller's current device as they found it (a multi-GPU
// process, or torch, keeps its own notion of "current device").
struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int device) {
        int cur = -1;
        if (hipGetDevice(&cur) == hipSuccess && cur != device) prev = cur;
        (void)hipSetDevice(device);
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};

// What a program IS (host side, immutable, shared by every context): the built schedule and its compact-container layout
struct HostProgram {
    host::ScheduleBuilder sb;
    host::CompactLayout compact;
};
// device tables of the passes behind a fill, the same set for a built-in program and a curve program
struct PassTables {
    DeviceArray<AuxItem> aux_items;   // built-in-generator columns (aux.hpp)
    DeviceArray<AuxTables> aux_tab;
    DeviceArray<GateItem> gate_items;
    DeviceArray<UxItem> ux_items;           // constraint-block columns (ux.hpp)
    DeviceArray<UxItem> ux_items_compact;   // the same table in compact coordinates (host::ux_items_compact)
    DeviceArray<u32> wide_before;   // [num_cols + 1]: wide columns before column c (Sink::wide_before)
    DeviceArray<u32> compact_map;   // per-column slot (p2e_columns_compact: built-in programs only)
    hipError_t upload(const host::ScheduleBuilder& sb, const host::CompactLayout& L, bool with_compact_map) {
        hipError_t e = aux_items.upload(sb.aux_items);
        if (e == hipSuccess) e = aux_tab.upload(&sb.aux_tab, 1);
        if (e == hipSuccess) e = gate_items.upload(sb.gate_items);
        if (e == hipSuccess) e = ux_items.upload(sb.ux_items);
        if (e == hipSuccess) e = ux_items_compact.upload(host::ux_items_compact(sb.ux_items, L.map));
        if (e == hipSuccess) e = wide_before.upload(L.wide_before);
        if (e == hipSuccess && with_compact_map) e = compact_map.upload(L.map);
        return e;
    }
};
// A built-in program inside one context: everything about the program itself is read through `host`
struct DeviceProgram {
    const HostProgram* host = nullptr;
    PassTables tab;
    DeviceArray<OpDesc> d_ops;        // with the run marks of tune.run_iters (F_NO_AFFINE)
    DeviceArray<OpDesc> d_ops_plain;  // without: every op expanded on its own (small batches)
    DeviceArray<OpDesc> d_ops_mid;    // with the run marks of tune.run_iters_mid (mid-size batches)
    DeviceArray<OpDesc> d_ops_small;  // with the run marks of tune.run_iters_small (four-lane plan)
    std::vector<OpDesc> h_ops;        // host copy of d_ops
};

struct p2e_ctx {
    int device = 0;
    unsigned flags = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    // The Jacobian chains are latency-bound (one wave per SIMD, strictly sequential) and leave most of the
    // ALU and all of the HBM bandwidth idle; the witness expansion is HBM-bound.  So the chains run on
    // their own high-priority streams, cut into pieces, and phases B/C of every finished piece run on the
    // caller's stream underneath the following pieces.
    static constexpr int MAX_SEG = plan::MAX_SEG;
    // st_binv, st_c2: second phase-B and second phase-C stream of the small-batch plan
    hipStream_t st_msm = nullptr, st_fixed = nullptr, st_binv = nullptr, st_c2 = nullptr;
    // st_c1: the library's OWN first expansion stream (stream_layout with a '1'): the caller's stream then only starts the
    // call (scalar phase) and ends it (finalisation); st_pad: spare streams that only exist to occupy hardware queues
    hipStream_t st_c1 = nullptr, st_pad[8] = {};
    // experiment (P2E_QUAD_EXPAND_CUS=k): expansion streams of the four-lane plan restricted to k compute units, so that
    // the latency-critical chain waves find SIMDs the HBM-bound expansions do not occupy
    hipStream_t st_c1q = nullptr, st_c2q = nullptr;
    hipEvent_t ev_c1join = nullptr;
    hipEvent_t ev_c2 = nullptr;
    hipEvent_t ev_fork = nullptr, ev_fixed = nullptr, ev_piece[MAX_SEG] = {}, ev_binv[MAX_SEG] = {};
    // one event pair around every expansion launch; kind 0 = k_expand (op by op), 1 = k_expand_runs, 2 = k_expand_fb_run
    static constexpr int MAX_EXPAND = plan::MAX_EXPAND;
    hipEvent_t ev_c0[MAX_EXPAND] = {}, ev_c1[MAX_EXPAND] = {};
    int n_expand = 0, n_seg = 0;
    double expand_cols[MAX_EXPAND] = {};
    int expand_kind[MAX_EXPAND] = {};
    // column blocks of the last fused call in issue order (p2e_segments_describe, plan::column_blocks): event < 0 = the
    // scalar phase (ev[1]), otherwise the block is final when ev_c1[event] has completed
    std::vector<plan::ColumnBlock> seg_blocks;
    Tuning tune;   // knobs.hpp: filled from the environment once, when the context is created
    DeviceArray<Aff> d_cpts, d_fbtab;
    DeviceArray<Aff> d_fbtab_p256;   // P-256 generator table of the key-derivation / signing calls: built and uploaded on first use
    DeviceArray<U256> d_constv;   // circuit constants by id (AUX_SRC_CONST | id), for the constraint-block pass
    DeviceProgram progs[2];
    void* scratch = nullptr;
    size_t scratch_bytes = 0;
    DeviceArray<unsigned char> d_msm;   // scratch of p2e_point_msm (pmsm.hpp MsmPlan): allocated on first need, kept, regrown
    size_t msm_bytes = 0;
    DeviceArray<unsigned char> d_schnorr;   // the 2 n + 1 terms of p2e_schnorr_verify_aggregate (SchnorrAggLayout): kept and regrown like d_msm
    size_t schnorr_bytes = 0;
    unsigned long long* d_counter = nullptr;
    unsigned long long* h_counter = nullptr;  // pinned
    hipEvent_t ev[6] = {};   // [0],[1] around k_scalar, [5] end of the call (2..4 unused)
    float phase_ms[12] = {0};   // [0] scalar, [4] whole call, per expansion kind k (launches, columns, summed ms): [1..3] k_expand,
                                // [5..7] k_expand_runs, [8..10] k_expand_fb_run
    bool have_phases = false;
};

#if P2E_HAS(0)
static_assert(Tuning::MAX_RUN_ITERS == MSM_DIGITS, "knobs.hpp: the bound of the P2E_RUN_ITERS* knobs");
static const HostProgram& host_program(int program) {
    static HostProgram P[2];
    static std::once_flag once;
    std::call_once(once, [] {
        P[0].sb.verify_secp256k1_message_circuit();
        P[1].sb.glv_mul_circuit();
        for (HostProgram& p : P) p.compact = host::compact_layout(p.sb.gens, (size_t)p.sb.prog.num_cols);
    });
    return P[program];
}
#endif   // P2E_HAS(0)

struct ScratchLayout {
    size_t px, py, pz, pw, pref, ax, ay, dig4, dig2, msrc, dyn, src, err32, valid8, total;
    // the scratch pointers of B inside the block at `base`
    void bind(Buffers& B, char* base) const {
        B.err = (u32*)(base + err32);
        B.valid = (uint8_t*)(base + valid8);
        B.PX = (U256*)(base + px);
        B.PY = (U256*)(base + py);
        B.PZ = (U256*)(base + pz);
        B.PW = (U256*)(base + pw);
        B.PREF = (U256*)(base + pref);
        B.AX = (U256*)(base + ax);
        B.AY = (U256*)(base + ay);
        B.dig4 = (uint8_t*)(base + dig4);
        B.dig2 = (uint8_t*)(base + dig2);
        B.msrc = (uint16_t*)(base + msrc);
        B.dyn = (uint16_t*)(base + dyn);
        B.src = (uint16_t*)(base + src);
    }
};
static ScratchLayout scratch_layout(const Program& G, size_t n) {
    ScratchLayout L{};
    size_t off = 0;
    auto take = [&](size_t bytes) {
        size_t o = off;
        off += (bytes + 255) & ~(size_t)255;
        return o;
    };
    L.px = take((size_t)G.num_slots * n * 32);
    L.py = take((size_t)G.num_slots * n * 32);
    L.pz = take((size_t)G.num_slots * n * 32);
    L.pw = take((size_t)G.num_ops * n * 32);
    L.pref = take((size_t)G.num_ops * n * 32);
    L.ax = take((size_t)G.num_slots * n * 32);
    L.ay = take((size_t)G.num_slots * n * 32);
    L.dig4 = take((size_t)FB_WINDOWS * n);
    const size_t rows = (size_t)(G.cp_rows > MSM_DIGITS ? G.cp_rows : MSM_DIGITS);   // curve programs: up to 261 bit rows
    L.dig2 = take(rows * n);
    L.msrc = take(rows * n * 2);
    L.dyn = take((size_t)G.num_cadd * n * 2);
    L.src = take((size_t)G.num_ops * 2 * n * 2);
    L.err32 = take(n * 4);
    L.valid8 = take(n);
    L.total = off;
    return L;
}

// Every internal stream of a context: its letter in the layout string (0: not made from the layout) and its priority
// class (+1 high, 0 normal, -1 low).  Creation, p2e_ctx_destroy and Staged::release all walk this one list.
template <class F>
static void each_internal_stream(p2e_ctx* c, F&& f) {
    f(c->st_msm, 'M', 1);
    f(c->st_fixed, 'F', 1);
    f(c->st_binv, 'B', 1);
    f(c->st_c2, '2', -1);
    f(c->st_c1, '1', 0);
    f(c->st_c1q, '\0', 0);
    f(c->st_c2q, '\0', 0);
    for (hipStream_t& st : c->st_pad) f(st, 'P', 0);
}

#if P2E_HAS(0)
extern "C" const char* p2e_last_error(void) { return g_last_error.c_str(); }

extern "C" size_t p2e_scratch_bytes(int program, size_t n) {
    if (program < 0 || program > 1) return 0;
    return scratch_layout(host_program(program).sb.prog, n).total;
}

// every event of a context with its creation flags (timed: only a P2E_CTX_PHASE_TIMING context pays for timestamps)
template <class F>
static void each_event(p2e_ctx* c, F&& f) {
    const unsigned timed = (c->flags & P2E_CTX_PHASE_TIMING) ? hipEventDefault : hipEventDisableTiming;
    // ev[1] closes the scalar phase's column block (p2e_segments_*): it exists either way, with a timestamp only on request
    for (auto& e : c->ev) f(e, timed);
    for (hipEvent_t* e : {&c->ev_c1join, &c->ev_c2, &c->ev_fork, &c->ev_fixed}) f(*e, hipEventDisableTiming);
    for (auto& e : c->ev_binv) f(e, hipEventDisableTiming);
    for (auto& e : c->ev_piece) f(e, hipEventDisableTiming);
    for (auto& e : c->ev_c0) f(e, hipEventDefault);
    for (auto& e : c->ev_c1) f(e, timed);
}

extern "C" int p2e_ctx_create(int device, unsigned flags, void* stream, p2e_ctx** out) {
    if (!out) return P2E_E_INVALID;
    // host-only check of the compact layout the compact-source ux pass walks, before anything is allocated
    for (int p = 0; p < 2; p++) {
        std::string why;
        if (!host::ux_items_compact_ok(host_program(p).sb.ux_items, host_program(p).compact.map, why)) {
            set_error(why);
            return P2E_E_INVALID;
        }
    }
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0) {
        set_error("no HIP device visible: libp2e_hip needs a gfx950 GPU (there is no CPU fallback)");
        return P2E_E_NO_DEVICE;
    }
    if (device < 0 || device >= count) {
        set_error("device index out of range");
        return P2E_E_INVALID;
    }
    DeviceGuard guard(device);
    // a failing HIP call below must not leak the context and what it already owns
    std::unique_ptr<p2e_ctx, void (*)(p2e_ctx*)> holder(new p2e_ctx(), p2e_ctx_destroy);
    p2e_ctx* c = holder.get();
    c->device = device;
    c->flags = flags;
    if (stream) {
        c->stream = (hipStream_t)stream;
    } else {
        // A BLOCKING stream: it keeps the implicit ordering with the legacy default stream, which is what a caller
        // that passes "its current stream" means when that stream is the default one (handle 0, indistinguishable
        // from NULL): e.g. torch.zeros(...) on torch's default stream followed by a call that writes the tensor.
        HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamDefault));
        c->own_stream = true;
    }
    const host::Consts& C = host::consts();
    HIP_TRY(c->d_cpts.upload(C.cpts, NUM_CONST_PTS));
    HIP_TRY(c->d_fbtab.upload(C.fbtab));
    {
        U256 cv[NUM_CONSTV];
        for (u32 id = 0; id < NUM_CONSTV; id++) cv[id] = host::ScheduleBuilder::const_value(id);
        HIP_TRY(c->d_constv.upload(cv, NUM_CONSTV));
    }
    read_tuning(c->tune, getenv);
    {   // never ask for more dynamic LDS than a workgroup may have on this device (160 KB on gfx950)
        int max_lds = 0;
        if (hipDeviceGetAttribute(&max_lds, hipDeviceAttributeMaxSharedMemoryPerBlock, device) != hipSuccess || max_lds <= 0) max_lds = 65536;
        (void)hipGetLastError();
        if (c->tune.expand_lds_small > (unsigned)max_lds) c->tune.expand_lds_small = (unsigned)max_lds;
        if (c->tune.expand_lds > (unsigned)max_lds) c->tune.expand_lds = (unsigned)max_lds;
    }
    for (int p = 0; p < 2; p++) {
        DeviceProgram& DP = c->progs[p];
        const host::ScheduleBuilder& sb = host_program(p).sb;
        DP.host = &host_program(p);
        DP.h_ops = sb.ops_with_runs(c->tune.run_iters, c->tune.fb_run);
        HIP_TRY(DP.d_ops.upload(DP.h_ops));
        HIP_TRY(DP.tab.upload(sb, DP.host->compact, true));
        HIP_TRY(DP.d_ops_mid.upload(sb.ops_with_runs(c->tune.run_iters_mid, c->tune.fb_run)));
        HIP_TRY(DP.d_ops_small.upload(sb.ops_with_runs(c->tune.run_iters_small, c->tune.fb_run)));
        HIP_TRY(DP.d_ops_plain.upload(sb.ops_with_runs(0)));
    }
    HIP_TRY(hipMalloc(&c->d_counter, sizeof(unsigned long long)));
    HIP_TRY(hipHostMalloc(&c->h_counter, sizeof(unsigned long long)));
    int prio_lo = 0, prio_hi = 0;
    HIP_TRY(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
    // Internal streams, created AND bound to their hardware queues (one empty launch each) in the order of the layout
    // string: M / F / B = the two chain streams and the second inversion stream (high priority), 2 = the second expansion
    // stream of the small-batch plan (low priority), 1 = an own first expansion stream (normal priority; without it the
    // caller's stream carries the expansions), P = a spare stream.  HIP binds a hardware queue to a stream at its first
    // launch and hands queues out in that order, and the step time of the small and mid-size plans depends on WHICH queues
    // the expansion, chain and inversion streams get relative to each other (profiles/r03_stream_order_*: the +-20 %
    // "creation order" effect of round 2 goes with the caller's queue sitting four positions from st_c2 in one order and
    // from st_binv in the other -- consistent with queues sharing a hardware pipe delaying each other's dispatch, though
    // the pipe assignment itself is not visible from here).  With every stream the pipeline dispatches on created here,
    // back to back, their relative placement no longer depends on what the caller did first.
    {
        const char* layout = getenv("P2E_STREAM_LAYOUT");
        // default: chain stream, OWN expansion stream, second chain stream, second inversion stream, second expansion
        // stream.  Of twelve layouts swept on two boxes (profiles/r03_stream_layout_sweep_box*.txt, one process per
        // setting) this is one of two whose step time is the same within 3 % whether the caller touched the GPU before
        // or after creating the context, at 2^13 ... 2^16 per call: 2.45 / 4.0-4.1 / 6.0-6.1 / 10.8 ms, against 2.29 or
        // 2.77 / 4.15 or 3.95 / 6.0 / 10.8 ms for the round-2 placement "MFB2" with the expansions on the caller's stream.
        if (!layout || !*layout) layout = "M1FB2";
        const char* tenv = getenv("P2E_TOUCH_STREAMS");
        const bool touch = !tenv || atoi(tenv) != 0;
        if (touch) {   // the legacy default stream first: a caller that has not touched the GPU yet gets its queue now
            hipLaunchKernelGGL(k_touch, dim3(1), dim3(64), 0, (hipStream_t)0);
            HIP_TRY(hipStreamSynchronize((hipStream_t)0));
            hipLaunchKernelGGL(k_touch, dim3(1), dim3(64), 0, c->stream);
            HIP_TRY(hipStreamSynchronize(c->stream));
        }
        hipError_t err = hipSuccess;
        const char* failed = "hipStreamCreateWithPriority";   // the call `err` came from
        auto create = [&](hipStream_t& st, int cls) {
            if (err == hipSuccess) err = hipStreamCreateWithPriority(&st, hipStreamNonBlocking, cls > 0 ? prio_hi : cls < 0 ? prio_lo : 0);
            return err == hipSuccess;
        };
        for (const char* p = layout; *p; p++) {   // the first free slot with this letter, if any
            bool made = false;
            each_internal_stream(c, [&](hipStream_t& st, char letter, int cls) {
                if (made || st || letter != *p) return;
                made = true;
                if (create(st, cls) && touch) {
                    hipLaunchKernelGGL(k_touch, dim3(1), dim3(64), 0, st);
                    err = hipStreamSynchronize(st);
                    if (err != hipSuccess) failed = "hipStreamSynchronize(internal stream)";
                }
            });
            HIP_TRY_AS(failed, err);
        }
        // the streams every plan needs, whatever the layout string left out
        each_internal_stream(c, [&](hipStream_t& st, char letter, int cls) {
            if (!st && letter && strchr("MFB2", letter)) create(st, cls);
        });
        HIP_TRY_AS(failed, err);
    }
    if (const char* env = getenv("P2E_QUAD_EXPAND_CUS")) {
        const int k = atoi(env);
        int ncu = 0;
        (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device);
        if (k > 0 && k < ncu) {
            const char* pat = getenv("P2E_QUAD_EXPAND_CU_PATTERN");   // "low" (default): CUs 0..k-1; "stride": every (ncu/k)-th
            std::vector<uint32_t> mask((size_t)(ncu + 31) / 32, 0u);
            for (int i = 0; i < k; i++) {
                const int cu = (pat && pat[0] == 's') ? (int)((long long)i * ncu / k) : i;
                mask[(size_t)cu >> 5] |= 1u << (cu & 31);
            }
            HIP_TRY(hipExtStreamCreateWithCUMask(&c->st_c1q, (uint32_t)mask.size(), mask.data()));
            HIP_TRY(hipExtStreamCreateWithCUMask(&c->st_c2q, (uint32_t)mask.size(), mask.data()));
        }
    }
    {
        hipError_t err = hipSuccess;
        each_event(c, [&](hipEvent_t& e, unsigned opt) {
            if (err == hipSuccess) err = hipEventCreateWithFlags(&e, opt);
        });
        HIP_TRY_AS("hipEventCreateWithFlags", err);
    }
    *out = holder.release();
    return 0;
}

extern "C" void p2e_ctx_destroy(p2e_ctx* c) {
    if (!c) return;
    DeviceGuard guard(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    each_internal_stream(c, [](hipStream_t& st, char, int) {
        if (!st) return;
        (void)hipStreamSynchronize(st);
        (void)hipStreamDestroy(st);
    });
    each_event(c, [](hipEvent_t& e, unsigned) {
        if (e) (void)hipEventDestroy(e);
    });
    (void)hipFree(c->scratch);
    (void)hipFree(c->d_counter);
    (void)hipHostFree(c->h_counter);
    if (c->own_stream) (void)hipStreamDestroy(c->stream);
    delete c;   // the device tables (DeviceArray members): nothing is running any more
}

// Which part of the fused pipeline an asynchronous failure (a kernel fault surfaces only when a stream is
// synchronised) had reached: the first recorded event of the call that did not complete.
static std::string pipeline_progress(p2e_ctx* c) {
    if (!c->have_phases) return "single-kernel call";
    if (hipEventQuery(c->ev[1]) != hipSuccess) return "scalar phase (k_scalar)";
    for (int k = 0; k < c->n_seg; k++) {
        if (hipEventQuery(c->ev_piece[k]) != hipSuccess) return "phase A (k_chains), chain piece " + std::to_string(k);
        if (hipEventQuery(c->ev_binv[k]) != hipSuccess) return "phase B (k_batch_inv), chain piece " + std::to_string(k);
    }
    for (int k = 0; k < c->n_expand; k++)
        if (hipEventQuery(c->ev_c1[k]) != hipSuccess)
            return std::string("phase C (") + (c->expand_kind[k] == 1 ? "k_expand_runs" : c->expand_kind[k] == 2 ? "k_expand_fb_run" : "k_expand") +
                   "), launch " + std::to_string(k);
    return "finalisation";
}

extern "C" int p2e_sync(p2e_ctx* c) {
    if (!c) return P2E_E_INVALID;
    DeviceGuard guard(c->device);
    hipError_t se = hipStreamSynchronize(c->stream);
    if (se != hipSuccess) {
        const std::string where = pipeline_progress(c);
        set_error(std::string("hipStreamSynchronize: ") + hipGetErrorString(se) + " [asynchronous failure; reached: " + where + "]");
        (void)hipGetLastError();
        return P2E_E_HIP;
    }
    if (c->have_phases) {   // launches and columns per kernel kind always; durations for P2E_CTX_PHASE_TIMING contexts
        const bool timed = (c->flags & P2E_CTX_PHASE_TIMING) != 0;
        c->phase_ms[0] = c->phase_ms[4] = 0.f;
        if (timed) {
            HIP_TRY(hipEventElapsedTime(&c->phase_ms[0], c->ev[0], c->ev[1]));   // scalar kernel
            HIP_TRY(hipEventElapsedTime(&c->phase_ms[4], c->ev[0], c->ev[5]));   // whole call
        }
        double cnt[3] = {0, 0, 0}, cols[3] = {0, 0, 0}, sum_ms[3] = {0, 0, 0};
        for (int k = 0; k < c->n_expand; k++) {
            float ms = 0.f;
            if (timed) HIP_TRY(hipEventElapsedTime(&ms, c->ev_c0[k], c->ev_c1[k]));
            const int kind = c->expand_kind[k];
            cnt[kind] += 1;
            cols[kind] += c->expand_cols[k];
            sum_ms[kind] += ms;
        }
        for (int kind = 0; kind < 3; kind++) {       // [1..3] k_expand, [5..7] k_expand_runs, [8..10] k_expand_fb_run
            const int o = kind == 0 ? 1 : kind == 1 ? 5 : 8;
            c->phase_ms[o] = (float)cnt[kind];       // launches
            c->phase_ms[o + 1] = (float)cols[kind];  // columns they wrote (per signature)
            c->phase_ms[o + 2] = (float)sum_ms[kind];  // their summed durations
        }
    }
    return (int)*c->h_counter;
}

extern "C" int p2e_last_phase_ms(p2e_ctx* c, float* out, int cap) {
    if (!c || !out) return P2E_E_INVALID;
    int k = cap < 12 ? cap : 12;
    for (int i = 0; i < k; i++) out[i] = c->phase_ms[i];
    return k;
}

extern "C" long p2e_segments_describe(p2e_ctx* c, p2e_segment_desc* out, size_t cap) {
    if (!c) return P2E_E_INVALID;
    for (size_t k = 0; out && k < c->seg_blocks.size() && k < cap; k++) {
        out[k].first_col = c->seg_blocks[k].first_col;
        out[k].num_cols = c->seg_blocks[k].num_cols;
    }
    return (long)c->seg_blocks.size();
}
static hipEvent_t segment_event(p2e_ctx* c, int k) {
    if (!c || k < 0 || (size_t)k >= c->seg_blocks.size()) return nullptr;
    const int e = c->seg_blocks[(size_t)k].event;
    return e < 0 ? c->ev[1] : c->ev_c1[e];
}
extern "C" int p2e_segment_stream_wait(p2e_ctx* c, int k, void* stream) {
    hipEvent_t ev = segment_event(c, k);
    if (!ev) {
        set_error("no such segment (p2e_segments_describe of the last fused call)");
        return P2E_E_INVALID;
    }
    DeviceGuard guard(c->device);
    HIP_TRY(hipStreamWaitEvent((hipStream_t)stream, ev, 0));
    return 0;
}
extern "C" int p2e_segment_sync(p2e_ctx* c, int k) {
    hipEvent_t ev = segment_event(c, k);
    if (!ev) {
        set_error("no such segment (p2e_segments_describe of the last fused call)");
        return P2E_E_INVALID;
    }
    DeviceGuard guard(c->device);
    HIP_TRY(hipEventSynchronize(ev));
    return 0;
}
#endif   // P2E_HAS(0)

static int ensure_scratch(p2e_ctx* c, size_t bytes) {
    if (bytes <= c->scratch_bytes) return 0;
    if (c->scratch) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(hipFree(c->scratch));
        c->scratch = nullptr;
        c->scratch_bytes = 0;
    }
    hipError_t e = hipMalloc(&c->scratch, bytes);
    if (e != hipSuccess) {
        c->scratch = nullptr;
        (void)hipGetLastError();   // handled here: must not resurface as the next call's "kernel launch" error
        set_error("scratch allocation of " + std::to_string(bytes) + " bytes failed: " + hipGetErrorString(e));
        return P2E_E_NOMEM;
    }
    c->scratch_bytes = bytes;
    return 0;
}

// the launches' status, and the flagged count on its way to the host
static long fetch_count(p2e_ctx* c) {
    hipError_t le = hipGetLastError();
    if (le != hipSuccess) {
        set_error(std::string("kernel launch: ") + hipGetErrorString(le));
        return P2E_E_HIP;
    }
    HIP_TRY(hipMemcpyAsync(c->h_counter, c->d_counter, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    return 0;
}
// finish a call: fetch the flagged count (synchronously unless the context is async)
static long finish_call(p2e_ctx* c) {
    if (long r = fetch_count(c)) return r;
    if (c->flags & P2E_CTX_ASYNC) return 0;
    int r = p2e_sync(c);
    return r;
}

#define ZERO_COUNTER(c) HIP_TRY(hipMemsetAsync((c)->d_counter, 0, sizeof(unsigned long long), (c)->stream))

// ---- host-pointer staging (slow path, used by ctypes-only callers) ----------------------------------
struct Staged {
    p2e_ctx* c;
    DeviceGuard guard;
    std::vector<void*> dev;
    struct Out {
        void* host;
        void* dev;
        size_t bytes;
    };
    std::vector<Out> outs;
    bool host;
    bool finished = false;
    int rc = 0;
    explicit Staged(p2e_ctx* ctx) : c(ctx), guard(ctx->device), host((ctx->flags & P2E_CTX_HOST_POINTERS) != 0) {}
    Staged(const Staged&) = delete;
    Staged& operator=(const Staged&) = delete;
    void* stage(size_t bytes) {
        void* d = nullptr;
        hipError_t e = hipMalloc(&d, bytes ? bytes : 1);
        if (e != hipSuccess) {
            (void)hipGetLastError();   // handled: must not resurface as the next call's launch error
            if (!rc) set_error("staging allocation of " + std::to_string(bytes) + " bytes failed: " + hipGetErrorString(e));
            rc = P2E_E_NOMEM;
            return nullptr;
        }
        dev.push_back(d);
        return d;
    }
    template <class T>
    const T* in(const T* p, size_t bytes) {
        if (!host || !p) return p;
        if (rc) return nullptr;        // an earlier buffer failed: do not touch the host side again
        void* d = stage(bytes);
        if (!d) return nullptr;
        hipError_t e = hipMemcpyAsync(d, p, bytes, hipMemcpyHostToDevice, c->stream);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            set_error(std::string("staging copy to the device failed: ") + hipGetErrorString(e));
            rc = P2E_E_HIP;
        }
        return (const T*)d;
    }
    template <class T>
    T* out(T* p, size_t bytes) {
        if (!host || !p) return p;
        if (rc) return nullptr;
        void* d = stage(bytes);
        if (!d) return nullptr;
        outs.push_back({p, d, bytes});
        return (T*)d;
    }
    // every exit of a staged entry point ends here: done(r) on the normal paths, the destructor on early error
    // returns (HIP_TRY / ZERO_COUNTER).  A failed call may have queued work on the internal streams: nothing of
    // it may still be running when the staged buffers are freed or the scratch is reused by the next call.
    void release(bool failed) {
        if (failed) {
            each_internal_stream(c, [](hipStream_t& st, char, int) {
                if (st) (void)hipStreamSynchronize(st);
            });
            (void)hipStreamSynchronize(c->stream);
            (void)hipGetLastError();
        }
        if (!dev.empty()) {
            if (!failed) (void)hipStreamSynchronize(c->stream);
            for (void* d : dev) (void)hipFree(d);
            dev.clear();
        }
        finished = true;
    }
    long done(long r) {
        if (host && r >= 0)
            for (auto& o : outs)
                if (hipMemcpyAsync(o.host, o.dev, o.bytes, hipMemcpyDeviceToHost, c->stream) != hipSuccess) {
                    set_error("staging copy to the host failed");
                    r = P2E_E_HIP;
                }
        release(r < 0);
        return r;
    }
    ~Staged() {
        if (!finished) release(true);
    }
    // what every per-element call does around its launches.  begin: the list's buffers staged, the phase times of an earlier
    // fused call dropped, the flagged count zeroed; nonzero = the call's return value.  end: the count fetched, the outputs home.
    long begin(call_args::List args) {
        call_args::stage(args, *this);
        if (rc) return done(rc);
        c->have_phases = false;
        ZERO_COUNTER(c);
        return 0;
    }
    long end() { return done(finish_call(c)); }
};

static bool bad_common(p2e_ctx* c, size_t n, size_t ld) {
    if (!c) {
        set_error("null context");
        return true;
    }
    if (ld < n) {
        set_error("ld < n");
        return true;
    }
    return false;
}
// BUFFER OVERLAP (include/p2e.h): what every fixed-stride per-element entry point does between its argument checks and its
// first read of the context.  The call lists its arguments once (call_args.hpp); n == 0 checks nothing.  The context's
// null test comes behind it, so that a call that passed the overlap check says so with "null context".
using Args = call_args::List;
// the null test of a call's list, in front of every other check (the wire-signature calls: behind curve and form)
static bool missing(Args args, const char* form = nullptr) {
    std::string text;
    if (!call_args::missing(args, text, form)) return false;
    set_error(text);
    return true;
}
static bool bad_overlap(size_t n, Args args) {
    if (n == 0) return false;
    overlap::Span spans[call_args::kMaxBufs];
    const overlap::Clash k = overlap::check(spans, call_args::spans(args, n, spans));
    if (!k.bad) return false;
    if (k.a == k.b)
        set_error(std::string("overlap: the end of ") + k.a + " wraps round the address space");
    else
        set_error(std::string("overlap: ") + k.a + " and " + k.b +
                  " share bytes (outputs are disjoint; an output may lie on an input only exactly in place, never on a broadcast one)");
    return true;
}
// bad_common for the calls that check overlap: the arguments first, the context's null test last (bad_ctx)
static bool bad_ctx(p2e_ctx* c) {
    if (c) return false;
    set_error("null context");
    return true;
}
static bool bad_curve(int curve) {
    if (curve == P2E_CURVE_SECP256K1 || curve == P2E_CURVE_P256) return false;
    set_error("unknown curve (P2E_CURVE_SECP256K1 or P2E_CURVE_P256)");
    return true;
}
// one launch covers at most 2^31 elements
static bool batch_too_large(size_t n) {
    if (n <= ((size_t)1 << 31)) return false;
    set_error("batch too large for one launch");
    return true;
}
static inline dim3 grid1(size_t n) { return dim3((unsigned)((n + BS - 1) / BS)); }

// ====================================================================================================
// single generators
// ====================================================================================================
#if P2E_HAS(0)
extern "C" long p2e_mul_witness_batch(p2e_ctx* c, int field, const uint64_t* x, const uint64_t* y, uint64_t* r,
                                      uint64_t* q, uint64_t* cs, uint64_t* b, size_t n, size_t ld, uint8_t* err) {
    if (bad_common(c, n, ld) || !x || !y || !r || !q || !cs || !b || !err || (field < 0 || field > 3)) return P2E_E_INVALID;
    if (n == 0) return 0;
    Staged S(c);
    size_t cb = ld * 8;
    x = S.in(x, 9 * cb);
    y = S.in(y, 9 * cb);
    r = S.out(r, 9 * cb);
    q = S.out(q, 9 * cb);
    cs = S.out(cs, 17 * cb);
    b = S.out(b, 16 * cb);
    err = S.out(err, n);
    if (S.rc) return S.done(S.rc);
    ZERO_COUNTER(c);
    if (field == P2E_FIELD_BASE)
        hipLaunchKernelGGL(k_mul<ModP>, grid1(n), dim3(BS), 0, c->stream, x, y, r, q, cs, b, n, ld, err, c->d_counter);
    else if (field == P2E_FIELD_SCALAR)
        hipLaunchKernelGGL(k_mul<ModN>, grid1(n), dim3(BS), 0, c->stream, x, y, r, q, cs, b, n, ld, err, c->d_counter);
    else if (field == P2E_FIELD_P256_BASE)
        hipLaunchKernelGGL(k_mul<ModP256>, grid1(n), dim3(BS), 0, c->stream, x, y, r, q, cs, b, n, ld, err, c->d_counter);
    else
        hipLaunchKernelGGL(k_mul<ModN256>, grid1(n), dim3(BS), 0, c->stream, x, y, r, q, cs, b, n, ld, err, c->d_counter);
    return S.done(finish_call(c));
}
extern "C" long p2e_checksum_witness_batch(p2e_ctx* c, const uint64_t* a, uint64_t* b, size_t n, size_t ld, uint8_t* err) {
    if (bad_common(c, n, ld) || !a || !b || !err) return P2E_E_INVALID;
    if (n == 0) return 0;
    Staged S(c);
    a = S.in(a, 17 * ld * 8);
    b = S.out(b, 16 * ld * 8);
    err = S.out(err, n);
    if (S.rc) return S.done(S.rc);
    ZERO_COUNTER(c);
    hipLaunchKernelGGL(k_checksum, grid1(n), dim3(BS), 0, c->stream, a, b, n, ld, err, c->d_counter);
    return S.done(finish_call(c));
}
static long addsub(p2e_ctx* c, int field, bool is_sub, const uint64_t* a, const uint64_t* b, uint64_t* out,
                   uint64_t* ov, size_t n, size_t ld, uint8_t* err) {
    if (bad_common(c, n, ld) || !a || !b || !out || !ov || !err || (field < 0 || field > 3)) return P2E_E_INVALID;
    if (n == 0) return 0;
    Staged S(c);
    a = S.in(a, 9 * ld * 8);
    b = S.in(b, 9 * ld * 8);
    out = S.out(out, 9 * ld * 8);
    ov = S.out(ov, n * 8);
    err = S.out(err, n);
    if (S.rc) return S.done(S.rc);
    ZERO_COUNTER(c);
    dim3 g = grid1(n), bs(BS);
    if (field == 0 && !is_sub) hipLaunchKernelGGL((k_addsub<ModP, false>), g, bs, 0, c->stream, a, b, out, ov, n, ld, err, c->d_counter);
    if (field == 0 && is_sub) hipLaunchKernelGGL((k_addsub<ModP, true>), g, bs, 0, c->stream, a, b, out, ov, n, ld, err, c->d_counter);
    if (field == 1 && !is_sub) hipLaunchKernelGGL((k_addsub<ModN, false>), g, bs, 0, c->stream, a, b, out, ov, n, ld, err, c->d_counter);
    if (field == 1 && is_sub) hipLaunchKernelGGL((k_addsub<ModN, true>), g, bs, 0, c->stream, a, b, out, ov, n, ld, err, c->d_counter);
    if (field == 2 && !is_sub) hipLaunchKernelGGL((k_addsub<ModP256, false>), g, bs, 0, c->stream, a, b, out, ov, n, ld, err, c->d_counter);
    if (field == 2 && is_sub) hipLaunchKernelGGL((k_addsub<ModP256, true>), g, bs, 0, c->stream, a, b, out, ov, n, ld, err, c->d_counter);
    if (field == 3 && !is_sub) hipLaunchKernelGGL((k_addsub<ModN256, false>), g, bs, 0, c->stream, a, b, out, ov, n, ld, err, c->d_counter);
    if (field == 3 && is_sub) hipLaunchKernelGGL((k_addsub<ModN256, true>), g, bs, 0, c->stream, a, b, out, ov, n, ld, err, c->d_counter);
    return S.done(finish_call(c));
}
extern "C" long p2e_add_witness_batch(p2e_ctx* c, int field, const uint64_t* a, const uint64_t* b, uint64_t* sum,
                                      uint64_t* ov, size_t n, size_t ld, uint8_t* err) {
    return addsub(c, field, false, a, b, sum, ov, n, ld, err);
}
extern "C" long p2e_sub_witness_batch(p2e_ctx* c, int field, const uint64_t* a, const uint64_t* b, uint64_t* diff,
                                      uint64_t* ov, size_t n, size_t ld, uint8_t* err) {
    return addsub(c, field, true, a, b, diff, ov, n, ld, err);
}
extern "C" long p2e_add_many_witness_batch(p2e_ctx* c, int field, const uint64_t* s, int k, uint64_t* sum,
                                           uint64_t* ov, size_t n, size_t ld, uint8_t* err) {
    if (bad_common(c, n, ld) || !s || !sum || !ov || !err || (field < 0 || field > 3) || k < 1 || k > 8) return P2E_E_INVALID;
    if (n == 0) return 0;
    Staged S(c);
    s = S.in(s, (size_t)k * 9 * ld * 8);
    sum = S.out(sum, 9 * ld * 8);
    ov = S.out(ov, n * 8);
    err = S.out(err, n);
    if (S.rc) return S.done(S.rc);
    ZERO_COUNTER(c);
    if (field == 0)
        hipLaunchKernelGGL(k_add_many<ModP>, grid1(n), dim3(BS), 0, c->stream, s, k, sum, ov, n, ld, err, c->d_counter);
    else if (field == 1)
        hipLaunchKernelGGL(k_add_many<ModN>, grid1(n), dim3(BS), 0, c->stream, s, k, sum, ov, n, ld, err, c->d_counter);
    else if (field == 2)
        hipLaunchKernelGGL(k_add_many<ModP256>, grid1(n), dim3(BS), 0, c->stream, s, k, sum, ov, n, ld, err, c->d_counter);
    else
        hipLaunchKernelGGL(k_add_many<ModN256>, grid1(n), dim3(BS), 0, c->stream, s, k, sum, ov, n, ld, err, c->d_counter);
    return S.done(finish_call(c));
}
extern "C" long p2e_inv_witness_batch(p2e_ctx* c, int field, const uint64_t* x, uint64_t* inv, uint64_t* div,
                                      size_t n, size_t ld, uint8_t* err) {
    if (bad_common(c, n, ld) || !x || !inv || !div || !err || (field < 0 || field > 3)) return P2E_E_INVALID;
    if (n == 0) return 0;
    Staged S(c);
    x = S.in(x, 9 * ld * 8);
    inv = S.out(inv, 9 * ld * 8);
    div = S.out(div, 9 * ld * 8);
    err = S.out(err, n);
    if (S.rc) return S.done(S.rc);
    ZERO_COUNTER(c);
    if (field == 0)
        hipLaunchKernelGGL(k_inv<ModP>, grid1(n), dim3(BS), 0, c->stream, x, inv, div, n, ld, err, c->d_counter);
    else if (field == 1)
        hipLaunchKernelGGL(k_inv<ModN>, grid1(n), dim3(BS), 0, c->stream, x, inv, div, n, ld, err, c->d_counter);
    else if (field == 2)
        hipLaunchKernelGGL(k_inv<ModP256>, grid1(n), dim3(BS), 0, c->stream, x, inv, div, n, ld, err, c->d_counter);
    else
        hipLaunchKernelGGL(k_inv<ModN256>, grid1(n), dim3(BS), 0, c->stream, x, inv, div, n, ld, err, c->d_counter);
    return S.done(finish_call(c));
}
extern "C" long p2e_biguint_div_rem_batch(p2e_ctx* c, const uint64_t* a, int na, const uint64_t* b, int nb, uint64_t* div,
                                          uint64_t* rem, size_t n, size_t ld, uint8_t* err) {
    const int nd = nb > na + 1 ? 0 : na - nb + 1;
    if (bad_common(c, n, ld) || na < 1 || na > 18 || nb < 1 || nb > 9 || !a || !b || (nd > 0 && !div) || !rem || !err)
        return P2E_E_INVALID;
    if (n == 0) return 0;
    Staged S(c);
    a = S.in(a, (size_t)na * ld * 8);
    b = S.in(b, (size_t)nb * ld * 8);
    if (nd > 0) div = S.out(div, (size_t)nd * ld * 8);
    rem = S.out(rem, (size_t)nb * ld * 8);
    err = S.out(err, n);
    if (S.rc) return S.done(S.rc);
    ZERO_COUNTER(c);
    hipLaunchKernelGGL(k_div_rem, grid1(n), dim3(BS), 0, c->stream, a, na, b, nb, div, rem, n, ld, err, c->d_counter);
    return S.done(finish_call(c));
}
extern "C" long p2e_glv_decompose_batch(p2e_ctx* c, const uint64_t* k, uint64_t* k1, uint64_t* k2, uint64_t* n1,
                                        uint64_t* n2, size_t n, size_t ld, uint8_t* err) {
    if (bad_common(c, n, ld) || !k || !k1 || !k2 || !n1 || !n2 || !err) return P2E_E_INVALID;
    if (n == 0) return 0;
    Staged S(c);
    k = S.in(k, 9 * ld * 8);
    k1 = S.out(k1, 5 * ld * 8);
    k2 = S.out(k2, 5 * ld * 8);
    n1 = S.out(n1, n * 8);
    n2 = S.out(n2, n * 8);
    err = S.out(err, n);
    if (S.rc) return S.done(S.rc);
    ZERO_COUNTER(c);
    hipLaunchKernelGGL(k_glv, grid1(n), dim3(BS), 0, c->stream, k, k1, k2, n1, n2, n, ld, err, c->d_counter);
    return S.done(finish_call(c));
}
extern "C" long p2e_limb_split(p2e_ctx* c, const uint8_t* packed, uint64_t* limbs, size_t n, size_t ld) {
    if (bad_common(c, n, ld) || !packed || !limbs) return P2E_E_INVALID;
    if (n == 0) return 0;
    Staged S(c);
    packed = S.in(packed, n * 32);
    limbs = S.out(limbs, 9 * ld * 8);
    if (S.rc) return S.done(S.rc);
    ZERO_COUNTER(c);
    size_t pairs = (n + 1) / 2;
    size_t blocks = (pairs + BS - 1) / BS;
    if (blocks > 256 * 16) blocks = 256 * 16;  // grid-stride above 16 workgroups per CU
    hipLaunchKernelGGL(k_split, dim3((unsigned)blocks), dim3(BS), 0, c->stream, packed, limbs, n, ld);
    return S.done(finish_call(c));
}
extern "C" long p2e_limb_pack(p2e_ctx* c, const uint64_t* limbs, uint8_t* packed, size_t n, size_t ld, uint8_t* err) {
    if (bad_common(c, n, ld) || !packed || !limbs || !err) return P2E_E_INVALID;
    if (n == 0) return 0;
    Staged S(c);
    limbs = S.in(limbs, 9 * ld * 8);
    packed = S.out(packed, n * 32);
    err = S.out(err, n);
    if (S.rc) return S.done(S.rc);
    ZERO_COUNTER(c);
    hipLaunchKernelGGL(k_pack, grid1(n), dim3(BS), 0, c->stream, limbs, packed, n, ld, err, c->d_counter);
    return S.done(finish_call(c));
}
#endif   // P2E_HAS(0)

// ====================================================================================================
// fused schedules
// ====================================================================================================
// The caller's pointers of a fused call; stage_fused replaces them by device pointers where the context stages.
struct FusedIO {
    const uint8_t* in[7];   // msg, r, s, pkx, pky, qx, qy (null: not an input of the program)
    uint64_t* cols;         // the u64 column matrix, or null: the compact container (narrow, wide) / no witness at all
    size_t ld;
    uint32_t* narrow;
    size_t ldn;
    uint64_t* wide;
    size_t ldw;
    uint8_t *err, *valid;
    // 16-byte column stores need full workgroups, an even column stride and a 16-byte aligned matrix
    // paired stores need full workgroups, even column strides and matrices aligned to two elements
    bool paired_stores_ok(bool compact) const {
        return compact ? (ldn % 2 == 0 && ldw % 2 == 0 && (reinterpret_cast<uintptr_t>(narrow) & 7) == 0 &&
                          (reinterpret_cast<uintptr_t>(wide) & 15) == 0)
                       : (ld % 2 == 0 && (reinterpret_cast<uintptr_t>(cols) & 15) == 0);
    }
};
// the common preface of the two launchers: inputs and outputs staged, the scratch sized and bound, B filled except for
// the tables (cpts, fbtab, ops)
static long stage_fused(p2e_ctx* c, Staged& S, const Program& G, const host::CompactLayout& CL, const u32* wide_before, bool compact,
                        bool verify_only, size_t n, FusedIO& io, Buffers& B) {
    for (const uint8_t*& p : io.in) p = S.in(p, n * 32);
    if (compact) {
        io.narrow = S.out(io.narrow, (size_t)CL.num_narrow * io.ldn * 4);
        io.wide = S.out(io.wide, (size_t)CL.num_wide * io.ldw * 8);
    } else if (!verify_only) {
        io.cols = S.out(io.cols, (size_t)G.num_cols * io.ld * 8);
    }
    io.err = S.out(io.err, n);
    io.valid = S.out(io.valid, n);
    if (S.rc) return S.rc;
    ScratchLayout L = scratch_layout(G, n);
    int rc = ensure_scratch(c, L.total);
    if (rc) return rc;
    B = Buffers{};
    B.msg = io.in[0];
    B.r = io.in[1];
    B.s = io.in[2];
    B.pkx = io.in[3];
    B.pky = io.in[4];
    B.qx = io.in[5];
    B.qy = io.in[6];
    B.sink = Sink{io.cols, io.ld, io.narrow, io.ldn, io.wide, io.ldw, wide_before};
    B.n = n;
    L.bind(B, (char*)c->scratch);
    return 0;
}
static plan::Layout stream_layout(const p2e_ctx* c) { return plan::Layout{c->st_c1 != nullptr, c->st_c1q != nullptr}; }
// what: "curve program" / "built-in program"; quad: the four-lane plan of a curve program (its piece length is a switch)
static void set_plan_error(plan::Error e, const std::string& what, bool quad) {
    set_error(e == plan::TOO_MANY_PIECES
                  ? what + " has too many pieces for the launch plan (at most " + std::to_string(plan::MAX_SEG) + ")" +
                        std::string(quad ? ": raise P2E_CP_PIECE_OPS_QUAD" : "")
              : e == plan::BAD_SHAPE ? what + " does not have the shape the run plan expects"
              : e == plan::BAD_ORDER ? what + ": phase C order names a piece the plan does not have"
                                     : what + ": the launch plan has more steps than a plan holds");
}

// The ONE place a plan becomes HIP calls: walks the steps in list order and does what each says.  K names the kernels of
// a family (BuiltinKernels, CurveKernels<CV>); no decision is taken here except the kernel variant of an emitting launch
// (EmitOf<MODE>: bit 0 = paired stores, bit 1 = compact container), which depends on pointer alignment (wide_ok): the
// paired launch over the full workgroups, the narrow one over the ragged tail.
// Keeps the books of p2e_last_phase_ms from the EXPAND_* steps; the column blocks of p2e_segments_describe are
// plan::column_blocks of the plan.
template <class K>
static long issue_plan(p2e_ctx* c, const plan::Plan& pl, const Program& G, const Buffers& B, const std::vector<OpDesc>& h_ops,
                       bool compact, bool wide_ok, uint8_t* err, uint8_t* valid) {
    using namespace plan;
    const size_t n = B.n;
    const unsigned gx = (unsigned)((n + BS - 1) / BS), gx4 = (unsigned)((4 * n + BS - 1) / BS);
    const size_t n_wide = wide_ok ? (n / BS) * BS : 0;
    const unsigned gx_wide = (unsigned)(n_wide / BS);
    const unsigned gx_tail = (unsigned)((n - n_wide + BS - 1) / BS);
    auto stream_of = [&](Stream s) -> hipStream_t {
        switch (s) {
        case ST_M: return c->st_msm;
        case ST_F: return c->st_fixed;
        case ST_B: return c->st_binv;
        case ST_C1: return pl.masked_expand ? c->st_c1q : c->st_c1 ? c->st_c1 : c->stream;
        case ST_C2: return pl.masked_expand ? c->st_c2q : c->st_c2;
        default: return c->stream;
        }
    };
    auto event_of = [&](Event e) -> hipEvent_t {
        switch (e.kind) {
        case EV_FORK: return c->ev_fork;
        case EV_FIXED: return c->ev_fixed;
        case EV_PIECE: return c->ev_piece[e.idx];
        case EV_BINV: return c->ev_binv[e.idx];
        case EV_C0: return c->ev_c0[e.idx];
        case EV_C1: return c->ev_c1[e.idx];
        case EV_C2: return c->ev_c2;
        case EV_C1JOIN: return c->ev_c1join;
        case EV_T0: return c->ev[0];
        case EV_T1: return c->ev[1];
        default: return c->ev[5];
        }
    };
    // launch(mode, workgroups, first signature) once per store form
    auto emit = [&](auto&& launch) {
        if (gx_wide) {
            if (compact) launch(std::integral_constant<int, 3>{}, gx_wide, (size_t)0);
            else launch(std::integral_constant<int, 1>{}, gx_wide, (size_t)0);
        }
        if (gx_tail) {
            if (compact) launch(std::integral_constant<int, 2>{}, gx_tail, n_wide);
            else launch(std::integral_constant<int, 0>{}, gx_tail, n_wide);
        }
    };
    // expansion launch e completes the columns of ops [lo, hi); kind 0 = op by op, 1 = loop runs, 2 = the fixed-base run
    auto note_expand = [&](int e, int kind, int lo, int hi) {
        double cw = 0;
        for (int t = lo; t < hi; t++) cw += op_cols(h_ops[t]);
        c->n_expand = e + 1;
        c->expand_kind[e] = kind;
        c->expand_cols[e] = cw;
    };
    c->n_seg = pl.n_seg;
    c->n_expand = 0;
    c->seg_blocks = column_blocks(G, h_ops, pl, K::loop_stride(G));
    const unsigned lds = pl.expand_lds;
    for (int k = 0; k < pl.n_steps; k++) {
        const Step& s = pl.steps[k];
        hipStream_t st = stream_of(s.stream);
        switch (s.kind) {
        case RECORD: HIP_TRY(hipEventRecord(event_of(s.ev), st)); break;
        case WAIT: HIP_TRY(hipStreamWaitEvent(st, event_of(s.ev), 0)); break;
        case SCALAR:
            emit([&](auto m, unsigned g, size_t first) { K::template scalar<decltype(m)::value>(dim3(g), st, G, B, first); });
            break;
        case CHAIN:
            if (s.form == ROWS) {
                if constexpr (K::has_rows) {
                    K::chain_rows(dim3(gx, (unsigned)s.b), st, G, B, s.a, s.c);
                } else {   // a missing kernel is an error, never a skipped step
                    set_error("launch plan: this kernel family has no row chains");
                    return P2E_E_INVALID;
                }
            } else if (s.form == QUAD)
                K::chain_quad(dim3(gx4), st, G, B, s.a, s.b, s.c, s.d);
            else
                K::chain_lane(dim3(gx), st, G, B, s.a, s.b, s.c, s.d);
            break;
        case BINV:
            if (s.d > 0)
                K::binv_split(dim3((unsigned)(((n << s.d) + BS - 1) / BS)), st, G, B, s.a, s.b, s.c, s.d);
            else
                K::binv(dim3(gx), st, G, B, s.a, s.b, s.c);
            break;
        case EXPAND_OPS:
            emit([&](auto m, unsigned g, size_t first) {
                K::template expand<decltype(m)::value>(dim3(g, (unsigned)(s.b - s.a)), lds, st, G, B, s.a, first);
            });
            note_expand(s.d, 0, s.a, s.b);
            break;
        case EXPAND_RUNS: {
            const unsigned nr = (unsigned)((s.b - s.a + s.c - 1) / s.c);
            emit([&](auto m, unsigned g, size_t first) {
                K::template expand_runs<decltype(m)::value>(dim3(g, nr), lds, st, G, B, s.a, s.c, s.b, first);
            });
            const int stride = K::loop_stride(G);
            note_expand(s.d, 1, G.msm_loop_begin + stride * s.a, G.msm_loop_begin + stride * s.b);
            break;
        }
        case EXPAND_FB_RUN:
            emit([&](auto m, unsigned g, size_t first) { K::template expand_fb_run<decltype(m)::value>(dim3(g), lds, st, G, B, s.a, first); });
            note_expand(s.d, 2, G.fb_begin, G.fb_begin + G.fb_windows);
            break;
        case FINALIZE:
            hipLaunchKernelGGL(k_finalize, dim3(gx), dim3(BS), 0, st, B.err, B.valid, err, valid, n, c->d_counter);
            break;
        }
    }
    c->have_phases = true;
    return 0;
}

#if P2E_HAS(1)
struct BuiltinKernels {
    static constexpr bool has_rows = true;
    static int loop_stride(const Program&) { return 3; }   // double, double, conditional add
    template <int MODE>
    static void scalar(dim3 g, hipStream_t st, const Program& G, const Buffers& B, size_t first) {
        hipLaunchKernelGGL(k_scalar<MODE>, g, dim3(BS), 0, st, G, B, first);
    }
    static void chain_lane(dim3 g, hipStream_t st, const Program& G, const Buffers& B, int lo, int hi, int table_affine, int cont) {
        hipLaunchKernelGGL(k_chains, g, dim3(BS), 0, st, G, B, lo, hi, table_affine, cont);
    }
    static void chain_quad(dim3 g, hipStream_t st, const Program& G, const Buffers& B, int lo, int hi, int table_affine, int cont) {
        hipLaunchKernelGGL(k_chains_quad, g, dim3(BS), 0, st, G, B, lo, hi, table_affine, cont);
    }
    static void chain_rows(dim3 g, hipStream_t st, const Program& G, const Buffers& B, int lo, int count) {
        hipLaunchKernelGGL(k_chain_rows, g, dim3(BS), 0, st, G, B, lo, count);
    }
    static void binv(dim3 g, hipStream_t st, const Program& G, const Buffers& B, int lo, int hi, int have_prefix) {
        hipLaunchKernelGGL(k_batch_inv, g, dim3(BS), 0, st, G, B, lo, hi, have_prefix);
    }
    static void binv_split(dim3 g, hipStream_t st, const Program& G, const Buffers& B, int lo, int hi, int have_prefix, int split_log2) {
        hipLaunchKernelGGL(k_batch_inv_split, g, dim3(BS), 0, st, G, B, lo, hi, have_prefix, split_log2);
    }
    template <int MODE>
    static void expand(dim3 g, unsigned lds, hipStream_t st, const Program& G, const Buffers& B, int lo, size_t first) {
        hipLaunchKernelGGL(k_expand<MODE>, g, dim3(BS), lds, st, G, B, lo, first);
    }
    template <int MODE>
    static void expand_runs(dim3 g, unsigned lds, hipStream_t st, const Program& G, const Buffers& B, int it0, int run_iters, int it1,
                            size_t first) {
        hipLaunchKernelGGL(k_expand_runs<MODE>, g, dim3(BS), lds, st, G, B, it0, run_iters, it1, first);
    }
    template <int MODE>
    static void expand_fb_run(dim3 g, unsigned lds, hipStream_t st, const Program& G, const Buffers& B, int t_after, size_t first) {
        hipLaunchKernelGGL(k_expand_fb_run<MODE>, g, dim3(BS), lds, st, G, B, t_after, first);
    }
};

// cols != nullptr: the u64 column matrix; otherwise the compact container (narrow, wide).  Stage, bind, build the plan, issue.
static long run_program(p2e_ctx* c, int program, const uint8_t* msg, const uint8_t* r, const uint8_t* s,
                        const uint8_t* pkx, const uint8_t* pky, uint64_t* cols, size_t n, size_t ld, uint8_t* err,
                        uint8_t* valid, uint32_t* narrow = nullptr, size_t ldn = 0, uint64_t* wide = nullptr, size_t ldw = 0,
                        bool verify_only = false) {
    const CallSwitches sw = read_call_switches(getenv);
    const bool compact = cols == nullptr && !verify_only;
    const DeviceProgram& DP = c->progs[program];
    const Program& G = DP.host->sb.prog;
    Staged S(c);
    FusedIO io{{msg, r, s, pkx, pky, nullptr, nullptr}, cols, ld, narrow, ldn, wide, ldw, err, valid};
    Buffers B;
    if (long rc = stage_fused(c, S, G, DP.host->compact, DP.tab.wide_before.get(), compact, verify_only, n, io, B)) return S.done(rc);
    B.cpts = c->d_cpts.get();
    B.fbtab = c->d_fbtab.get();
    ZERO_COUNTER(c);
    c->n_expand = 0;
    c->seg_blocks.clear();
    if (verify_only) {
        // the native verification alone: scalar phase without emission, the two chains side by side in Jacobian
        // coordinates (no batch inversion, no expansion), the final add, r == x on its Jacobian result
        const unsigned gx = (unsigned)((n + BS - 1) / BS);
        B.ops = DP.d_ops_plain.get();
        hipLaunchKernelGGL(k_scalar<4>, dim3(gx), dim3(BS), 0, c->stream, G, B, (size_t)0);
        HIP_TRY(hipEventRecord(c->ev_fork, c->stream));
        HIP_TRY(hipStreamWaitEvent(c->st_fixed, c->ev_fork, 0));
        hipLaunchKernelGGL(k_chains, dim3(gx), dim3(BS), 0, c->st_fixed, G, B, G.chain_begin[1], G.chain_end[1], 0, 0);
        HIP_TRY(hipEventRecord(c->ev_fixed, c->st_fixed));
        hipLaunchKernelGGL(k_chains, dim3(gx), dim3(BS), 0, c->stream, G, B, G.chain_begin[0], G.chain_end[0], 0, 0);
        HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_fixed, 0));
        hipLaunchKernelGGL(k_chains, dim3(gx), dim3(BS), 0, c->stream, G, B, G.chain_begin[2], G.chain_end[2], 0, 0);
        hipLaunchKernelGGL(k_verify_check, dim3(gx), dim3(BS), 0, c->stream, G, B);
        hipLaunchKernelGGL(k_finalize, dim3(gx), dim3(BS), 0, c->stream, B.err, B.valid, io.err, io.valid, n, c->d_counter);
        c->have_phases = false;
        return S.done(finish_call(c));
    }
    plan::Plan pl;
    if (!plan::build_builtin(G, plan::choose_builtin(G, c->tune, n, stream_layout(c), (c->flags & P2E_CTX_PHASE_TIMING) != 0), pl)) {
        set_plan_error(pl.error, "built-in program", false);
        return S.done(P2E_E_INVALID);
    }
    const DeviceArray<OpDesc>* tables[] = {&DP.d_ops_plain, &DP.d_ops, &DP.d_ops_mid, &DP.d_ops_small};   // by plan::OpTable
    B.ops = tables[pl.ops]->get();
    if (long rc = issue_plan<BuiltinKernels>(c, pl, G, B, DP.h_ops, compact, !sw.narrow_stores && io.paired_stores_ok(compact), io.err, io.valid))
        return rc;
    return S.done(finish_call(c));
}

extern "C" long p2e_ecdsa_verify_witness_batch(p2e_ctx* c, const uint8_t* msg32, const uint8_t* r32,
                                               const uint8_t* s32, const uint8_t* pkx32, const uint8_t* pky32,
                                               uint64_t* cols, size_t n, size_t ld, uint8_t* err, uint8_t* valid) {
    if (bad_common(c, n, ld) || !msg32 || !r32 || !s32 || !pkx32 || !pky32 || !cols || !err) return P2E_E_INVALID;
    if (n == 0) return 0;
    return run_program(c, 0, msg32, r32, s32, pkx32, pky32, cols, n, ld, err, valid);
}
extern "C" long p2e_ecdsa_verify_batch(p2e_ctx* c, const uint8_t* msg32, const uint8_t* r32, const uint8_t* s32,
                                       const uint8_t* pkx32, const uint8_t* pky32, size_t n, uint8_t* err, uint8_t* valid) {
    // (staging is run_program's own, as for the witness calls)
    const Args args = {ARG_SHARED(msg32, 32, n), ARG_SHARED(r32, 32, n), ARG_SHARED(s32, 32, n), ARG_SHARED(pkx32, 32, n),
                       ARG_SHARED(pky32, 32, n), ARG_OUT(err, 1, n), ARG_OUT(valid, 1, n)};
    if (missing(args) || bad_overlap(n, args) || bad_ctx(c)) return P2E_E_INVALID;
    if (n == 0) return 0;
    return run_program(c, 0, msg32, r32, s32, pkx32, pky32, nullptr, n, n, err, valid, nullptr, 0, nullptr, 0, true);
}
extern "C" long p2e_glv_mul_witness_batch(p2e_ctx* c, const uint8_t* px32, const uint8_t* py32, const uint8_t* k32,
                                          uint64_t* cols, size_t n, size_t ld, uint8_t* err, uint8_t* valid) {
    if (bad_common(c, n, ld) || !px32 || !py32 || !k32 || !cols || !err) return P2E_E_INVALID;
    if (n == 0) return 0;
    return run_program(c, 1, k32, k32, k32, px32, py32, cols, n, ld, err, valid);
}

extern "C" long p2e_ecdsa_verify_witness_compact_batch(p2e_ctx* c, const uint8_t* msg32, const uint8_t* r32, const uint8_t* s32,
                                                       const uint8_t* pkx32, const uint8_t* pky32, uint32_t* narrow, size_t ld_narrow,
                                                       uint64_t* wide, size_t ld_wide, size_t n, uint8_t* err, uint8_t* valid) {
    if (bad_common(c, n, ld_narrow) || ld_wide < n || !msg32 || !r32 || !s32 || !pkx32 || !pky32 || !narrow || !wide || !err)
        return P2E_E_INVALID;
    if (n == 0) return 0;
    return run_program(c, 0, msg32, r32, s32, pkx32, pky32, nullptr, n, 0, err, valid, narrow, ld_narrow, wide, ld_wide);
}
extern "C" long p2e_glv_mul_witness_compact_batch(p2e_ctx* c, const uint8_t* px32, const uint8_t* py32, const uint8_t* k32,
                                                  uint32_t* narrow, size_t ld_narrow, uint64_t* wide, size_t ld_wide, size_t n,
                                                  uint8_t* err, uint8_t* valid) {
    if (bad_common(c, n, ld_narrow) || ld_wide < n || !px32 || !py32 || !k32 || !narrow || !wide || !err) return P2E_E_INVALID;
    if (n == 0) return 0;
    return run_program(c, 1, k32, k32, k32, px32, py32, nullptr, n, 0, err, valid, narrow, ld_narrow, wide, ld_wide);
}
#endif   // P2E_HAS(1)

#if P2E_HAS(0)
extern "C" long p2e_columns_to_rows(p2e_ctx* c, const uint64_t* cols, size_t ld, size_t n, size_t ncols,
                                    uint64_t* rows, size_t row_ld) {
    if (bad_common(c, n, ld) || !cols || !rows || row_ld < ncols) return P2E_E_INVALID;
    if (n == 0 || ncols == 0) return 0;
    Staged S(c);
    cols = S.in(cols, ncols * ld * 8);
    rows = S.out(rows, n * row_ld * 8);
    if (S.rc) return S.done(S.rc);
    ZERO_COUNTER(c);
    dim3 grid((unsigned)((n + 63) / 64), (unsigned)((ncols + 63) / 64));
    hipLaunchKernelGGL(k_transpose<u64>, grid, dim3(BS), 0, c->stream, cols, ld, n, ncols, rows, row_ld);
    return S.done(finish_call(c));
}
extern "C" long p2e_compact_to_rows(p2e_ctx* c, int program, const uint32_t* narrow, size_t ld_narrow, const uint64_t* wide,
                                    size_t ld_wide, size_t n, uint32_t* rows_narrow, size_t row_ld_narrow, uint64_t* rows_wide,
                                    size_t row_ld_wide) {
    if (bad_common(c, n, ld_narrow) || program < 0 || program > 1 || ld_wide < n || !narrow || !wide || !rows_narrow || !rows_wide)
        return P2E_E_INVALID;
    const DeviceProgram& DP = c->progs[program];
    if (row_ld_narrow < DP.host->compact.num_narrow || row_ld_wide < DP.host->compact.num_wide) {
        set_error("row stride smaller than the matrix");
        return P2E_E_INVALID;
    }
    if (n == 0) return 0;
    Staged S(c);
    narrow = S.in(narrow, (size_t)DP.host->compact.num_narrow * ld_narrow * 4);
    wide = S.in(wide, (size_t)DP.host->compact.num_wide * ld_wide * 8);
    rows_narrow = S.out(rows_narrow, n * row_ld_narrow * 4);
    rows_wide = S.out(rows_wide, n * row_ld_wide * 8);
    if (S.rc) return S.done(S.rc);
    ZERO_COUNTER(c);
    const unsigned gx = (unsigned)((n + 63) / 64);
    hipLaunchKernelGGL(k_transpose<u32>, dim3(gx, (DP.host->compact.num_narrow + 63) / 64), dim3(BS), 0, c->stream, narrow, ld_narrow, n,
                       (size_t)DP.host->compact.num_narrow, rows_narrow, row_ld_narrow);
    hipLaunchKernelGGL(k_transpose<u64>, dim3(gx, (DP.host->compact.num_wide + 63) / 64), dim3(BS), 0, c->stream, wide, ld_wide, n,
                       (size_t)DP.host->compact.num_wide, rows_wide, row_ld_wide);
    return S.done(finish_call(c));
}

extern "C" long p2e_columns_compact(p2e_ctx* c, int program, const uint64_t* cols, size_t ld, size_t n, uint32_t* narrow,
                                    size_t ld_narrow, uint64_t* wide, size_t ld_wide, uint8_t* err) {
    if (bad_common(c, n, ld) || program < 0 || program > 1 || !cols || !narrow || !wide || !err || ld_narrow < n || ld_wide < n) {
        if (c && (ld_narrow < n || ld_wide < n)) set_error("ld_narrow / ld_wide < n");
        return P2E_E_INVALID;
    }
    if (n == 0) return 0;
    const DeviceProgram& DP = c->progs[program];
    Staged S(c);
    cols = S.in(cols, (size_t)DP.host->sb.prog.num_cols * ld * 8);
    narrow = S.out(narrow, (size_t)DP.host->compact.num_narrow * ld_narrow * 4);
    wide = S.out(wide, (size_t)DP.host->compact.num_wide * ld_wide * 8);
    err = S.out(err, n);
    if (S.rc) return S.done(S.rc);
    if (int rc = ensure_scratch(c, n * sizeof(u32))) return S.done(rc);
    ZERO_COUNTER(c);
    u32* err32 = (u32*)c->scratch;
    HIP_TRY(hipMemsetAsync(err32, 0, n * sizeof(u32), c->stream));
    const int pair_ok = ld % 2 == 0 && ld_narrow % 2 == 0 && ld_wide % 2 == 0 && (reinterpret_cast<uintptr_t>(cols) & 15) == 0 &&
                        (reinterpret_cast<uintptr_t>(narrow) & 7) == 0 && (reinterpret_cast<uintptr_t>(wide) & 15) == 0;
    const u32 ncols = (u32)DP.host->sb.prog.num_cols;
    dim3 grid((unsigned)((n + 2 * BS - 1) / (2 * BS)), (ncols + COMPACT_GROUP - 1) / COMPACT_GROUP);
    hipLaunchKernelGGL(k_compact, grid, dim3(BS), 0, c->stream, cols, ld, n, ncols, DP.tab.compact_map.get(), narrow, ld_narrow, wide,
                       ld_wide, err32, pair_ok);
    hipLaunchKernelGGL(k_finalize, dim3((unsigned)((n + BS - 1) / BS)), dim3(BS), 0, c->stream, err32, (const uint8_t*)nullptr,
                       err, (uint8_t*)nullptr, n, c->d_counter);
    c->have_phases = false;
    return S.done(finish_call(c));
}

// aux_u32: the output matrix is u32 (all values are limbs, bits and flags); cols == nullptr: read the compact
// container's narrow matrix instead of the u64 witness matrix
static long run_aux(p2e_ctx* c, int program, const uint8_t* pky32, const uint64_t* cols, size_t ld, const uint32_t* narrow,
                    size_t ldn, void* aux, bool aux_u32, size_t ld_aux, size_t n, uint8_t* err) {
    const DeviceProgram& DP = c->progs[program];
    Staged S(c);
    pky32 = S.in(pky32, 32 * n);
    if (cols) cols = S.in(cols, (size_t)DP.host->sb.prog.num_cols * ld * 8);
    if (narrow) narrow = S.in(narrow, (size_t)DP.host->compact.num_narrow * ldn * 4);
    aux = S.out((char*)aux, (size_t)DP.host->sb.aux_tab.num_aux_cols * ld_aux * (aux_u32 ? 4 : 8));
    err = S.out(err, n);
    if (S.rc) return S.done(S.rc);
    if (int rc = ensure_scratch(c, n * sizeof(u32))) return S.done(rc);
    ZERO_COUNTER(c);
    u32* err32 = (u32*)c->scratch;
    HIP_TRY(hipMemsetAsync(err32, 0, n * sizeof(u32), c->stream));
    AuxArgs A{cols, ld, aux, ld_aux, n, pky32, c->d_cpts.get(), c->d_fbtab.get(), DP.tab.aux_items.get(), DP.tab.aux_tab.get(), err32,
              narrow, ldn, DP.tab.wide_before.get()};
    const unsigned gx = (unsigned)((n + BS - 1) / BS), items = (unsigned)DP.host->sb.aux_items.size();
    // paired column stores for the full workgroups, one element per lane for the ragged tail
    const bool wide_ok = (ld_aux % 2 == 0) && ((reinterpret_cast<uintptr_t>(aux) & (aux_u32 ? 7 : 15)) == 0) &&
                         !narrow_stores_forced();
    const size_t n_wide = wide_ok ? (n / BS) * BS : 0;
    const dim3 gw((unsigned)(n_wide / BS), items), gt((unsigned)((n - n_wide + BS - 1) / BS), items);
    if (aux_u32) {
        if (n_wide) hipLaunchKernelGGL(k_aux<3>, gw, dim3(BS), 0, c->stream, A, (size_t)0);
        if (n > n_wide) hipLaunchKernelGGL(k_aux<2>, gt, dim3(BS), 0, c->stream, A, n_wide);
    } else {
        if (n_wide) hipLaunchKernelGGL(k_aux<1>, gw, dim3(BS), 0, c->stream, A, (size_t)0);
        if (n > n_wide) hipLaunchKernelGGL(k_aux<0>, gt, dim3(BS), 0, c->stream, A, n_wide);
    }
    hipLaunchKernelGGL(k_finalize, dim3(gx), dim3(BS), 0, c->stream, err32, (const uint8_t*)nullptr, err,
                       (uint8_t*)nullptr, n, c->d_counter);
    c->have_phases = false;
    return S.done(finish_call(c));
}
extern "C" long p2e_aux_witness_batch(p2e_ctx* c, int program, const uint8_t* pky32, const uint64_t* cols, size_t ld,
                                      uint64_t* aux, size_t ld_aux, size_t n, uint8_t* err) {
    if (bad_common(c, n, ld) || program < 0 || program > 1 || !pky32 || !cols || !aux || !err || ld_aux < n) {
        if (c && ld_aux < n) set_error("ld_aux < n");
        return P2E_E_INVALID;
    }
    if (n == 0) return 0;
    return run_aux(c, program, pky32, cols, ld, nullptr, 0, aux, false, ld_aux, n, err);
}
extern "C" long p2e_aux_witness_compact_batch(p2e_ctx* c, int program, const uint8_t* pky32, const uint32_t* narrow,
                                              size_t ld_narrow, uint32_t* aux32, size_t ld_aux, size_t n, uint8_t* err) {
    if (bad_common(c, n, ld_narrow) || program < 0 || program > 1 || !pky32 || !narrow || !aux32 || !err || ld_aux < n) {
        if (c && ld_aux < n) set_error("ld_aux < n");
        return P2E_E_INVALID;
    }
    if (n == 0) return 0;
    return run_aux(c, program, pky32, nullptr, 0, narrow, ld_narrow, aux32, true, ld_aux, n, err);
}

struct p2e_wire_map {
    int device = 0;
    u32 limit[4] = {0, 0, 0, 0};   // column counts of the four source matrices (witness, aux, ux, gate) of the map's program
    DeviceArray<u32> d_src;
    DeviceArray<u32> d_csrc;   // the same entries with the witness columns in compact coordinates (narrow row, or WIRE_CSRC_WIDE | wide row)
    DeviceArray<u32> d_dst;
    size_t count = 0;
    u32 num_wires = 0, degree = 0;
    bool uses[4] = {false, false, false, false};
    u32 num_narrow = 0, num_wide = 0;   // rows of the program's compact container
    bool uses_narrow = false, uses_wide = false;
};
// compact: the program's compact layout (p2e_compact_layout)
static int make_wire_map(p2e_ctx* c, const u32 limit[4], const host::CompactLayout& compact, const p2e_wire_map_entry* entries,
                         size_t count, uint32_t num_wires, uint32_t degree, p2e_wire_map** out) {
    if (!c || !out || (!entries && count) || !num_wires || !degree) return P2E_E_INVALID;
    const u64 cells = (u64)num_wires * degree;
    std::vector<p2e_wire_map_entry> v(entries, entries + count);
    std::stable_sort(v.begin(), v.end(), [](const p2e_wire_map_entry& a, const p2e_wire_map_entry& b) { return a.dst < b.dst; });
    std::unique_ptr<p2e_wire_map> m(new p2e_wire_map());
    for (size_t k = 0; k < count; k++) {
        const u32 kind = v[k].src >> 30, col = v[k].src & 0x3FFFFFFFu;
        if (col >= limit[kind] || v[k].dst >= cells || (k && v[k].dst == v[k - 1].dst)) {
            set_error(col >= limit[kind] ? "wire map: source column out of range"
                      : v[k].dst >= cells                          ? "wire map: destination outside num_wires * degree"
                                                                   : "wire map: two entries share a destination");
            return P2E_E_INVALID;
        }
        m->uses[kind] = true;
    }
    std::vector<u32> src(count), csrc(count), dst(count);
    for (size_t k = 0; k < count; k++) {
        src[k] = csrc[k] = v[k].src;
        dst[k] = v[k].dst;
        if ((v[k].src >> 30) == 0) {
            const u32 slot = compact.map[v[k].src];
            const bool wide = (slot & COMPACT_WIDE) != 0;
            csrc[k] = wide ? (WIRE_CSRC_WIDE | (slot & ~COMPACT_WIDE)) : slot;
            (wide ? m->uses_wide : m->uses_narrow) = true;
        }
    }
    DeviceGuard guard(c->device);
    m->device = c->device;
    for (int k = 0; k < 4; k++) m->limit[k] = limit[k];
    m->count = count;
    m->num_wires = num_wires;
    m->degree = degree;
    m->num_narrow = compact.num_narrow;
    m->num_wide = compact.num_wide;
    if (m->d_src.upload(src) != hipSuccess || m->d_csrc.upload(csrc) != hipSuccess || m->d_dst.upload(dst) != hipSuccess) {
        set_error("wire map: device allocation failed");
        return P2E_E_NOMEM;
    }
    *out = m.release();
    return 0;
}
extern "C" int p2e_wire_map_create(p2e_ctx* c, int program, const p2e_wire_map_entry* entries, size_t count, uint32_t num_wires,
                                   uint32_t degree, p2e_wire_map** out) {
    if (program < 0 || program > 1) return P2E_E_INVALID;
    const HostProgram& HP = host_program(program);
    const u32 limit[4] = {(u32)HP.sb.prog.num_cols, HP.sb.aux_tab.num_aux_cols, HP.sb.num_ux_cols, HP.sb.num_gate_cols};
    return make_wire_map(c, limit, HP.compact, entries, count, num_wires, degree, out);
}
extern "C" void p2e_wire_map_destroy(p2e_ctx* c, p2e_wire_map* m) {
    if (!m) return;
    DeviceGuard guard(m->device);
    if (c) (void)hipStreamSynchronize(c->stream);   // (no context: no stream that could still be reading the map)
    delete m;
}
// the launch of both assemblies: A holds the (staged) sources; the wire matrix is an in-out buffer
static long run_assemble(p2e_ctx* c, Staged& S, const p2e_wire_map* m, AssembleArgs A, bool compact, uint64_t* wires, size_t wire_stride,
                         size_t n) {
    uint64_t* const host_wires = wires;
    if (S.host) {   // in-out buffer: positions no entry names keep the caller's values
        void* d_stage = S.stage(n * wire_stride * 8);
        if (d_stage && hipMemcpyAsync(d_stage, host_wires, n * wire_stride * 8, hipMemcpyHostToDevice, c->stream) != hipSuccess) S.rc = P2E_E_HIP;
        if (d_stage) S.outs.push_back({host_wires, d_stage, n * wire_stride * 8});
        wires = (uint64_t*)d_stage;
    }
    if (S.rc) return S.done(S.rc);
    ZERO_COUNTER(c);
    A.src = compact ? m->d_csrc.get() : m->d_src.get();
    A.dst = m->d_dst.get();
    A.count = m->count;
    A.wires = wires;
    A.stride = wire_stride;
    A.n = n;
    dim3 grid((unsigned)((n + 63) / 64), (unsigned)((m->count + 63) / 64));
    if (compact)
        hipLaunchKernelGGL(k_assemble_compact, grid, dim3(BS), 0, c->stream, A);
    else
        hipLaunchKernelGGL(k_assemble, grid, dim3(BS), 0, c->stream, A);
    c->have_phases = false;
    return S.done(finish_call(c));
}
extern "C" long p2e_assemble_wires(p2e_ctx* c, const p2e_wire_map* m, const uint64_t* cols, size_t ld, const uint64_t* aux,
                                   size_t ld_aux, const void* ux, int ux_u32, size_t ld_ux, const uint64_t* gate, size_t ld_gate,
                                   uint64_t* wires, size_t wire_stride, size_t n) {
    if (!c || !m || !wires || wire_stride < (size_t)m->num_wires * m->degree || (m->uses[0] && (!cols || ld < n)) ||
        (m->uses[1] && (!aux || ld_aux < n)) || (m->uses[2] && (!ux || ld_ux < n)) || (m->uses[3] && (!gate || ld_gate < n))) {
        set_error("p2e_assemble_wires: null matrix the map reads, ld < n, or wire_stride < num_wires * degree");
        return P2E_E_INVALID;
    }
    if (n == 0 || m->count == 0) return 0;
    Staged S(c);
    if (cols) cols = S.in(cols, (size_t)m->limit[0] * ld * 8);
    if (aux) aux = S.in(aux, (size_t)m->limit[1] * ld_aux * 8);
    if (ux) ux = S.in((const char*)ux, (size_t)m->limit[2] * ld_ux * (ux_u32 ? 4 : 8));
    if (gate) gate = S.in(gate, (size_t)m->limit[3] * ld_gate * 8);
    AssembleArgs A{};
    A.cols = cols;
    A.ld = ld;
    A.aux = aux;
    A.ald = ld_aux;
    A.ux = ux;
    A.uld = ld_ux;
    A.ux_u32 = ux_u32;
    A.gate = gate;
    A.gld = ld_gate;
    return run_assemble(c, S, m, A, false, wires, wire_stride, n);
}
// the same scatter from the compact container and the u32 aux matrix (the map keeps its witness sources in both
// coordinates: a map made for one container works for the other)
extern "C" long p2e_assemble_wires_compact(p2e_ctx* c, const p2e_wire_map* m, const uint32_t* narrow, size_t ld_narrow,
                                           const uint64_t* wide, size_t ld_wide, const uint32_t* aux32, size_t ld_aux, const void* ux,
                                           int ux_u32, size_t ld_ux, const uint64_t* gate, size_t ld_gate, uint64_t* wires,
                                           size_t wire_stride, size_t n) {
    if (!c || !m || !wires || wire_stride < (size_t)m->num_wires * m->degree || (m->uses_narrow && (!narrow || ld_narrow < n)) ||
        (m->uses_wide && (!wide || ld_wide < n)) || (m->uses[1] && (!aux32 || ld_aux < n)) || (m->uses[2] && (!ux || ld_ux < n)) ||
        (m->uses[3] && (!gate || ld_gate < n))) {
        set_error("p2e_assemble_wires_compact: null matrix the map reads, ld < n, or wire_stride < num_wires * degree");
        return P2E_E_INVALID;
    }
    if (n == 0 || m->count == 0) return 0;
    Staged S(c);
    if (narrow) narrow = S.in(narrow, (size_t)m->num_narrow * ld_narrow * 4);
    if (wide) wide = S.in(wide, (size_t)m->num_wide * ld_wide * 8);
    if (aux32) aux32 = S.in(aux32, (size_t)m->limit[1] * ld_aux * 4);
    if (ux) ux = S.in((const char*)ux, (size_t)m->limit[2] * ld_ux * (ux_u32 ? 4 : 8));
    if (gate) gate = S.in(gate, (size_t)m->limit[3] * ld_gate * 8);
    AssembleArgs A{};
    A.nar = narrow;
    A.ldn = ld_narrow;
    A.wide = wide;
    A.ldw = ld_wide;
    A.aux32 = aux32;
    A.ald = ld_aux;
    A.ux = ux;
    A.uld = ld_ux;
    A.ux_u32 = ux_u32;
    A.gate = gate;
    A.gld = ld_gate;
    return run_assemble(c, S, m, A, true, wires, wire_stride, n);
}

static u64 gl_pow_host(u64 a, u64 e) {
    u64 r = 1;
    while (e) {
        if (e & 1) r = gl_mul(r, a);
        a = gl_mul(a, a);
        e >>= 1;
    }
    return r;
}
// the gate-internal pass of any program: aux is the u64 aux matrix, or (aux_u32) the u32 one of the compact aux pass
static long run_gate(p2e_ctx* c, const void* aux, bool aux_u32, size_t ld_aux, uint64_t* gate, size_t ld_gate, size_t n,
                     u32 num_aux_cols, u32 num_gate_cols, const GateItem* d_items, unsigned items) {
    Staged S(c);
    aux = S.in((const char*)aux, (size_t)num_aux_cols * ld_aux * (aux_u32 ? 4 : 8));
    gate = S.out(gate, (size_t)num_gate_cols * ld_gate * 8);
    if (S.rc) return S.done(S.rc);
    ZERO_COUNTER(c);
    GateArgs A{};
    if (aux_u32)
        A.aux32 = (const u32*)aux;
    else
        A.aux = (const u64*)aux;
    A.ald = ld_aux;
    A.gate = gate;
    A.gld = ld_gate;
    A.n = n;
    A.items = d_items;
    A.inv16[0] = 0;
    for (u64 d = 1; d < 16; d++) A.inv16[d] = gl_pow_host(d, P_GL - 2);
    const bool wide_ok = (ld_gate % 2 == 0) && ((reinterpret_cast<uintptr_t>(gate) & 15) == 0) && !narrow_stores_forced();
    const size_t n_wide = wide_ok ? (n / BS) * BS : 0;
    const dim3 gw((unsigned)(n_wide / BS), items), gt((unsigned)((n - n_wide + BS - 1) / BS), items);
    if (aux_u32) {
        if (n_wide) hipLaunchKernelGGL(k_gate_compact<1>, gw, dim3(BS), 0, c->stream, A, (size_t)0);
        if (n > n_wide) hipLaunchKernelGGL(k_gate_compact<0>, gt, dim3(BS), 0, c->stream, A, n_wide);
    } else {
        if (n_wide) hipLaunchKernelGGL(k_gate<1>, gw, dim3(BS), 0, c->stream, A, (size_t)0);
        if (n > n_wide) hipLaunchKernelGGL(k_gate<0>, gt, dim3(BS), 0, c->stream, A, n_wide);
    }
    c->have_phases = false;
    return S.done(finish_call(c));
}
extern "C" long p2e_gate_internal_batch(p2e_ctx* c, int program, const uint64_t* aux, size_t ld_aux, uint64_t* gate, size_t ld_gate,
                                        size_t n) {
    if (bad_common(c, n, ld_aux) || program < 0 || program > 1 || !aux || !gate || ld_gate < n) {
        if (c && ld_gate < n) set_error("ld_gate < n");
        return P2E_E_INVALID;
    }
    if (n == 0) return 0;
    const DeviceProgram& DP = c->progs[program];
    const host::ScheduleBuilder& sb = DP.host->sb;
    return run_gate(c, aux, false, ld_aux, gate, ld_gate, n, sb.aux_tab.num_aux_cols, sb.num_gate_cols, DP.tab.gate_items.get(),
                    (unsigned)sb.gate_items.size());
}
extern "C" long p2e_gate_internal_compact_batch(p2e_ctx* c, int program, const uint32_t* aux32, size_t ld_aux, uint64_t* gate,
                                                size_t ld_gate, size_t n) {
    if (bad_common(c, n, ld_aux) || program < 0 || program > 1 || !aux32 || !gate || ld_gate < n) {
        if (c && ld_gate < n) set_error("ld_gate < n");
        return P2E_E_INVALID;
    }
    if (n == 0) return 0;
    const DeviceProgram& DP = c->progs[program];
    const host::ScheduleBuilder& sb = DP.host->sb;
    return run_gate(c, aux32, true, ld_aux, gate, ld_gate, n, sb.aux_tab.num_aux_cols, sb.num_gate_cols, DP.tab.gate_items.get(),
                    (unsigned)sb.gate_items.size());
}
extern "C" long p2e_gate_internal_num_cols(int program) {
    if (program < 0 || program > 1) return P2E_E_INVALID;
    return (long)host_program(program).sb.num_gate_cols;
}

// The constraint-block pass of any program.  Source: the u64 matrices cols / aux, or (cols == nullptr) the compact
// container's narrow matrix and the u32 aux matrix.  kern[MODE]: the program family's kernels for that source
// (AuxEmitOf<MODE>: bit 0 = paired stores, bit 1 = u32 output).
typedef void (*UxKernel)(UxArgs, size_t);
struct UxCall {
    const uint8_t* in[7] = {};   // packed inputs by INPUT_* slot; null where the program has none
    const uint64_t* cols = nullptr;
    size_t ld = 0;
    const uint32_t* narrow = nullptr;
    size_t ldn = 0;
    const void* aux = nullptr;
    size_t ld_aux = 0;
    void* ux = nullptr;
    int ux_u32 = 0;
    size_t ld_ux = 0, n = 0;
    uint8_t* err = nullptr;
    // the program's
    u32 num_cols = 0, num_narrow = 0, num_aux_cols = 0, num_ux_cols = 0;
    const U256* d_consts = nullptr;
    const UxItem* d_items = nullptr;           // u64 source
    const UxItem* d_items_compact = nullptr;   // compact source: the table in compact coordinates
    unsigned items = 0;
};
static long run_ux(p2e_ctx* c, UxCall U, const UxKernel kern[4]) {
    const bool compact = U.cols == nullptr;
    const size_t n = U.n;
    Staged S(c);
    for (int k = 0; k < 7; k++)
        if (U.in[k]) U.in[k] = S.in(U.in[k], 32 * n);
    if (compact) {
        U.narrow = S.in(U.narrow, (size_t)U.num_narrow * U.ldn * 4);
        U.aux = S.in((const char*)U.aux, (size_t)U.num_aux_cols * U.ld_aux * 4);
    } else {
        U.cols = S.in(U.cols, (size_t)U.num_cols * U.ld * 8);
        U.aux = S.in((const char*)U.aux, (size_t)U.num_aux_cols * U.ld_aux * 8);
    }
    void* ux = S.out((char*)U.ux, (size_t)U.num_ux_cols * U.ld_ux * (U.ux_u32 ? 4 : 8));
    uint8_t* err = S.out(U.err, n);
    if (S.rc) return S.done(S.rc);
    if (int rc = ensure_scratch(c, n * sizeof(u32))) return S.done(rc);
    ZERO_COUNTER(c);
    u32* err32 = (u32*)c->scratch;
    HIP_TRY(hipMemsetAsync(err32, 0, n * sizeof(u32), c->stream));
    UxArgs A{};
    A.cols = U.cols;
    A.ld = U.ld;
    A.ald = U.ld_aux;
    if (compact) {
        A.nar = U.narrow;
        A.ldn = U.ldn;
        A.aux32 = (const u32*)U.aux;
    } else {
        A.aux = (const u64*)U.aux;
    }
    A.ux = ux;
    A.uld = U.ld_ux;
    A.n = n;
    for (int k = 0; k < 7; k++) A.in[k] = U.in[k];
    if (!A.in[INPUT_R]) A.in[INPUT_R] = A.in[INPUT_MSG];
    if (!A.in[INPUT_S]) A.in[INPUT_S] = A.in[INPUT_MSG];
    A.consts = U.d_consts;
    A.items = compact ? U.d_items_compact : U.d_items;
    A.err = err32;
    const unsigned gx = (unsigned)((n + BS - 1) / BS);
    const bool wide_ok = (U.ld_ux % 2 == 0) && ((reinterpret_cast<uintptr_t>(ux) & (U.ux_u32 ? 7 : 15)) == 0) && !narrow_stores_forced();
    const size_t n_wide = wide_ok ? (n / BS) * BS : 0;
    const dim3 gw((unsigned)(n_wide / BS), U.items), gt((unsigned)((n - n_wide + BS - 1) / BS), U.items);
    const int u32_bit = U.ux_u32 ? 2 : 0;
    if (n_wide) hipLaunchKernelGGL(kern[u32_bit | 1], gw, dim3(BS), 0, c->stream, A, (size_t)0);
    if (n > n_wide) hipLaunchKernelGGL(kern[u32_bit], gt, dim3(BS), 0, c->stream, A, n_wide);
    hipLaunchKernelGGL(k_finalize, dim3(gx), dim3(BS), 0, c->stream, err32, (const uint8_t*)nullptr, err, (uint8_t*)nullptr, n,
                       c->d_counter);
    c->have_phases = false;
    return S.done(finish_call(c));
}
static UxCall builtin_ux_call(p2e_ctx* c, int program, const uint8_t* msg32, const uint8_t* r32, const uint8_t* s32, const uint8_t* pkx32,
                              const uint8_t* pky32, void* ux, int ux_u32, size_t ld_ux, size_t n, uint8_t* err) {
    const DeviceProgram& DP = c->progs[program];
    UxCall U;
    U.in[INPUT_PY] = pky32;
    U.in[INPUT_PX] = pkx32;
    U.in[INPUT_MSG] = msg32;
    U.in[INPUT_R] = r32;
    U.in[INPUT_S] = s32;
    U.ux = ux;
    U.ux_u32 = ux_u32;
    U.ld_ux = ld_ux;
    U.n = n;
    U.err = err;
    U.num_cols = (u32)DP.host->sb.prog.num_cols;
    U.num_narrow = DP.host->compact.num_narrow;
    U.num_aux_cols = DP.host->sb.aux_tab.num_aux_cols;
    U.num_ux_cols = DP.host->sb.num_ux_cols;
    U.d_consts = c->d_constv.get();
    U.d_items = DP.tab.ux_items.get();
    U.d_items_compact = DP.tab.ux_items_compact.get();
    U.items = (unsigned)DP.host->sb.ux_items.size();
    return U;
}
extern "C" long p2e_ux_witness_batch(p2e_ctx* c, int program, const uint8_t* msg32, const uint8_t* r32, const uint8_t* s32,
                                     const uint8_t* pkx32, const uint8_t* pky32, const uint64_t* cols, size_t ld,
                                     const uint64_t* aux, size_t ld_aux, void* ux, int ux_u32, size_t ld_ux, size_t n, uint8_t* err) {
    if (bad_common(c, n, ld) || program < 0 || program > 1 || !msg32 || !pkx32 || !pky32 || (program == 0 && (!r32 || !s32)) ||
        !cols || !aux || !ux || !err || ld_aux < n || ld_ux < n) {
        if (c && (ld_aux < n || ld_ux < n)) set_error("ld_aux / ld_ux < n");
        return P2E_E_INVALID;
    }
    if (n == 0) return 0;
    UxCall U = builtin_ux_call(c, program, msg32, r32, s32, pkx32, pky32, ux, ux_u32, ld_ux, n, err);
    U.cols = cols;
    U.ld = ld;
    U.aux = aux;
    U.ld_aux = ld_aux;
    static const UxKernel kern[4] = {k_ux<0>, k_ux<1>, k_ux<2>, k_ux<3>};
    return run_ux(c, U, kern);
}
extern "C" long p2e_ux_witness_compact_batch(p2e_ctx* c, int program, const uint8_t* msg32, const uint8_t* r32, const uint8_t* s32,
                                             const uint8_t* pkx32, const uint8_t* pky32, const uint32_t* narrow, size_t ld_narrow,
                                             const uint32_t* aux32, size_t ld_aux, void* ux, int ux_u32, size_t ld_ux, size_t n,
                                             uint8_t* err) {
    if (bad_common(c, n, ld_narrow) || program < 0 || program > 1 || !msg32 || !pkx32 || !pky32 || (program == 0 && (!r32 || !s32)) ||
        !narrow || !aux32 || !ux || !err || ld_aux < n || ld_ux < n) {
        if (c && (ld_aux < n || ld_ux < n)) set_error("ld_aux / ld_ux < n");
        return P2E_E_INVALID;
    }
    if (n == 0) return 0;
    UxCall U = builtin_ux_call(c, program, msg32, r32, s32, pkx32, pky32, ux, ux_u32, ld_ux, n, err);
    U.narrow = narrow;
    U.ldn = ld_narrow;
    U.aux = aux32;
    U.ld_aux = ld_aux;
    static const UxKernel kern[4] = {k_ux_compact<0>, k_ux_compact<1>, k_ux_compact<2>, k_ux_compact<3>};
    return run_ux(c, U, kern);
}

// ====================================================================================================
// host-only entry points
// ====================================================================================================
extern "C" long p2e_ux_describe(int program, p2e_ux_desc* out, size_t cap) {
    if (program < 0 || program > 1) return P2E_E_INVALID;
    const host::ScheduleBuilder& sb = host_program(program).sb;
    for (size_t i = 0; i < sb.ux_first.size() && i < cap && out; i++) {
        out[i].first_col = sb.ux_first[i];
        out[i].num_cols = sb.ux_count[i];
    }
    return (long)sb.ux_first.size();
}
extern "C" long p2e_ux_num_cols(int program) {
    if (program < 0 || program > 1) return P2E_E_INVALID;
    return (long)host_program(program).sb.num_ux_cols;
}
extern "C" long p2e_aux_describe(int program, p2e_aux_desc* out, size_t cap) {
    if (program < 0 || program > 1) return P2E_E_INVALID;
    const auto& g = host_program(program).sb.aux_gens;
    for (size_t i = 0; i < g.size() && i < cap && out; i++) {
        out[i].kind = g[i].kind;
        out[i].first_col = g[i].col;
        out[i].num_cols = g[i].ncols;
        std::memset(out[i].label, 0, sizeof out[i].label);
        std::strncpy(out[i].label, g[i].label.c_str(), sizeof(out[i].label) - 1);
    }
    return (long)g.size();
}
extern "C" long p2e_compact_layout(int program, uint32_t* col_map, size_t cap, uint32_t* num_narrow, uint32_t* num_wide) {
    if (program < 0 || program > 1) return P2E_E_INVALID;
    const host::CompactLayout& L = host_program(program).compact;
    for (size_t i = 0; i < L.map.size() && i < cap && col_map; i++) col_map[i] = L.map[i];
    if (num_narrow) *num_narrow = L.num_narrow;
    if (num_wide) *num_wide = L.num_wide;
    return (long)L.map.size();
}
extern "C" long p2e_aux_num_cols(int program) {
    if (program < 0 || program > 1) return P2E_E_INVALID;
    return host_program(program).sb.aux_tab.num_aux_cols;
}
extern "C" long p2e_schedule_describe(int program, p2e_gen_desc* out, size_t cap) {
    if (program < 0 || program > 1) return P2E_E_INVALID;
    const auto& g = host_program(program).sb.gens;
    for (size_t i = 0; i < g.size() && i < cap && out; i++) {
        out[i].kind = g[i].kind;
        out[i].field = g[i].field;
        out[i].first_col = g[i].col;
        out[i].num_cols = g[i].ncols;
        std::memset(out[i].label, 0, sizeof out[i].label);
        std::strncpy(out[i].label, g[i].label.c_str(), sizeof(out[i].label) - 1);
    }
    return (long)g.size();
}
extern "C" long p2e_schedule_wiring(int program, p2e_gen_wiring* out, size_t cap) {
    if (program < 0 || program > 1) return P2E_E_INVALID;
    const auto& g = host_program(program).sb.gens;
    for (size_t i = 0; i < g.size() && i < cap && out; i++) {
        out[i].num_operands = g[i].nops;
        out[i].range_check = g[i].range_check ? 1 : 0;
        for (int k = 0; k < 4; k++) {
            out[i].src[k] = g[i].src[k];
            out[i].num_limbs[k] = g[i].nl[k];
        }
    }
    return (long)g.size();
}
extern "C" int p2e_wiring_const(uint32_t id, uint8_t out32[32]) {
    if (id >= NUM_CONSTV || !out32) return P2E_E_INVALID;
    const U256 v = host::ScheduleBuilder::const_value(id);
    std::memcpy(out32, v.w, 32);
    u32 l[NL];
    split29(v, l);
    int n = NL;
    while (n > 0 && l[n - 1] == 0) n--;
    return n;
}
extern "C" long p2e_schedule_num_cols(int program) {
    if (program < 0 || program > 1) return P2E_E_INVALID;
    return host_program(program).sb.prog.num_cols;
}
extern "C" int p2e_synth_signatures(uint64_t seed, size_t first, size_t n, uint8_t* msg32, uint8_t* r32, uint8_t* s32,
                                    uint8_t* pkx32, uint8_t* pky32) {
    if (!msg32 || !r32 || !s32 || !pkx32 || !pky32) return P2E_E_INVALID;
#pragma omp parallel for schedule(dynamic, 64)
    for (long long i = 0; i < (long long)n; i++) {
        U256 msg, r, s;
        Aff pk;
        host::synth_signature(seed, first + (size_t)i, msg, r, s, pk);
        std::memcpy(msg32 + 32 * i, msg.w, 32);
        std::memcpy(r32 + 32 * i, r.w, 32);
        std::memcpy(s32 + 32 * i, s.w, 32);
        std::memcpy(pkx32 + 32 * i, pk.x.w, 32);
        std::memcpy(pky32 + 32 * i, pk.y.w, 32);
    }
    return 0;
}
#endif   // P2E_HAS(0)

// ====================================================================================================
// key derivation and signing (sign.hpp): curve/ecdsa.rs:16-20 to_public, :25-40 sign_message
// ====================================================================================================
// one launch on the caller's stream; msg == nullptr: the key kernel (out1 / out2 = pk.x / pk.y), else the signer (r / s).
// Defined (and explicitly instantiated) where the curve's chain code lives: secp256k1 in part 2, P-256 in part 3.
template <class CV>
void launch_sign(p2e_ctx* c, int plan, const Aff* table, const uint8_t* msg, const uint8_t* sk, const uint8_t* k, uint8_t* out1,
                 uint8_t* out2, size_t n, uint8_t* err);
template <class CV>
void launch_sign_recoverable(p2e_ctx* c, int plan, const Aff* table, const uint8_t* msg, const uint8_t* sk, const uint8_t* k, uint8_t* r,
                             uint8_t* s, uint8_t* v, size_t n, uint8_t* err);
template <class CV>
void launch_recover(p2e_ctx* c, const Aff* table, const uint8_t* msg, const uint8_t* r, const uint8_t* s, const uint8_t* v, uint8_t* pkx,
                    uint8_t* pky, size_t n, uint8_t* err);
#if P2E_HAS(2) || P2E_HAS(3)
template <class CV>
void launch_sign(p2e_ctx* c, int plan, const Aff* table, const uint8_t* msg, const uint8_t* sk, const uint8_t* k, uint8_t* out1,
                 uint8_t* out2, size_t n, uint8_t* err) {
    const bool quad = plan == SIGN_PLAN_QUAD;
    const dim3 grid = grid1(quad ? 4 * n : n);
    if (!msg) {
        if (quad)
            hipLaunchKernelGGL((k_public_key<CV, SIGN_PLAN_QUAD>), grid, dim3(BS), 0, c->stream, table, sk, out1, out2, n, err, c->d_counter);
        else
            hipLaunchKernelGGL((k_public_key<CV, SIGN_PLAN_LANE>), grid, dim3(BS), 0, c->stream, table, sk, out1, out2, n, err, c->d_counter);
    } else if (quad) {
        hipLaunchKernelGGL((k_sign<CV, SIGN_PLAN_QUAD>), grid, dim3(BS), 0, c->stream, table, msg, sk, k, out1, out2, n, err, c->d_counter);
    } else {
        hipLaunchKernelGGL((k_sign<CV, SIGN_PLAN_LANE>), grid, dim3(BS), 0, c->stream, table, msg, sk, k, out1, out2, n, err, c->d_counter);
    }
}
// the signer with the recovery byte, and the recovery itself (recover.hpp): one lane per signature, one launch
template <class CV>
void launch_sign_recoverable(p2e_ctx* c, int plan, const Aff* table, const uint8_t* msg, const uint8_t* sk, const uint8_t* k, uint8_t* r,
                             uint8_t* s, uint8_t* v, size_t n, uint8_t* err) {
    if (plan == SIGN_PLAN_QUAD)
        hipLaunchKernelGGL((k_sign_recoverable<CV, SIGN_PLAN_QUAD>), grid1(4 * n), dim3(BS), 0, c->stream, table, msg, sk, k, r, s, v, n, err,
                           c->d_counter);
    else
        hipLaunchKernelGGL((k_sign_recoverable<CV, SIGN_PLAN_LANE>), grid1(n), dim3(BS), 0, c->stream, table, msg, sk, k, r, s, v, n, err,
                           c->d_counter);
}
template <class CV>
void launch_recover(p2e_ctx* c, const Aff* table, const uint8_t* msg, const uint8_t* r, const uint8_t* s, const uint8_t* v, uint8_t* pkx,
                    uint8_t* pky, size_t n, uint8_t* err) {
    hipLaunchKernelGGL((k_recover<CV>), grid1(n), dim3(BS), 0, c->stream, table, msg, r, s, v, pkx, pky, n, err, c->d_counter);
}
#if P2E_PART < 0 || P2E_PART == 2
template void launch_sign_recoverable<Secp256k1>(p2e_ctx*, int, const Aff*, const uint8_t*, const uint8_t*, const uint8_t*, uint8_t*, uint8_t*,
                                                 uint8_t*, size_t, uint8_t*);
template void launch_recover<Secp256k1>(p2e_ctx*, const Aff*, const uint8_t*, const uint8_t*, const uint8_t*, const uint8_t*, uint8_t*,
                                        uint8_t*, size_t, uint8_t*);
template void launch_sign<Secp256k1>(p2e_ctx*, int, const Aff*, const uint8_t*, const uint8_t*, const uint8_t*, uint8_t*, uint8_t*, size_t,
                                     uint8_t*);
#endif
#if P2E_PART < 0 || P2E_PART == 3
template void launch_sign_recoverable<P256>(p2e_ctx*, int, const Aff*, const uint8_t*, const uint8_t*, const uint8_t*, uint8_t*, uint8_t*, uint8_t*,
                                            size_t, uint8_t*);
template void launch_recover<P256>(p2e_ctx*, const Aff*, const uint8_t*, const uint8_t*, const uint8_t*, const uint8_t*, uint8_t*, uint8_t*,
                                   size_t, uint8_t*);
template void launch_sign<P256>(p2e_ctx*, int, const Aff*, const uint8_t*, const uint8_t*, const uint8_t*, uint8_t*, uint8_t*, size_t,
                                uint8_t*);
#endif
#endif   // P2E_HAS(2) || P2E_HAS(3)

#if P2E_HAS(0)
// curve / plan checks shared by the two calls, and the curve's generator table (P-256: made on first use, kept)
// `args`: the call's buffers for the overlap check, which runs behind the argument checks and before the context is read
static int sign_prepare(p2e_ctx* c, int curve, unsigned plan, size_t n, const Aff** table, int* chosen, Args args = {}) {
    if (bad_curve(curve)) return P2E_E_INVALID;
    if (plan != P2E_SIGN_PLAN_AUTO && plan != P2E_SIGN_PLAN_LANE && plan != P2E_SIGN_PLAN_QUAD) {
        set_error("unknown plan (P2E_SIGN_PLAN_AUTO, P2E_SIGN_PLAN_LANE or P2E_SIGN_PLAN_QUAD)");
        return P2E_E_INVALID;
    }
    if (batch_too_large(n) || bad_overlap(n, args) || bad_ctx(c)) return P2E_E_INVALID;
    *chosen = plan == P2E_SIGN_PLAN_AUTO ? (n <= c->tune.sign_quad_max_n ? SIGN_PLAN_QUAD : SIGN_PLAN_LANE) : (int)plan;
    if (curve == P2E_CURVE_SECP256K1) {
        *table = c->d_fbtab.get();
        return 0;
    }
    if (!c->d_fbtab_p256.get() && n) {
        DeviceGuard guard(c->device);
        static const std::vector<Aff> t = host::fixed_base_table_cv<P256>(host::generator_cv<P256>());
        hipError_t e = c->d_fbtab_p256.upload(t);
        if (e != hipSuccess) {
            set_error(std::string("upload of the P-256 generator table failed: ") + hipGetErrorString(e));
            return P2E_E_HIP;
        }
    }
    *table = c->d_fbtab_p256.get();
    return 0;
}
extern "C" long p2e_ecdsa_public_key_batch(p2e_ctx* c, int curve, unsigned plan, const uint8_t* sk32, uint8_t* pkx32, uint8_t* pky32,
                                           size_t n, uint8_t* err) {
    const Args args = {ARG_IN(sk32, 32, n), ARG_OUT(pkx32, 32, n), ARG_OUT(pky32, 32, n), ARG_OUT(err, 1, n)};
    if (missing(args)) return P2E_E_INVALID;
    const Aff* table = nullptr;
    int chosen = 0;
    if (int rc = sign_prepare(c, curve, plan, n, &table, &chosen, args)) return rc;
    if (n == 0) return 0;
    Staged S(c);
    if (long rc = S.begin(args)) return rc;
    if (curve == P2E_CURVE_P256)
        launch_sign<P256>(c, chosen, table, nullptr, sk32, nullptr, pkx32, pky32, n, err);
    else
        launch_sign<Secp256k1>(c, chosen, table, nullptr, sk32, nullptr, pkx32, pky32, n, err);
    return S.end();
}
extern "C" long p2e_ecdsa_sign_batch(p2e_ctx* c, int curve, unsigned plan, const uint8_t* msg32, const uint8_t* sk32, const uint8_t* k32,
                                     uint8_t* r32, uint8_t* s32, size_t n, uint8_t* err) {
    const Args args = {ARG_IN(msg32, 32, n), ARG_IN(sk32, 32, n), ARG_IN(k32, 32, n),
                       ARG_OUT(r32, 32, n), ARG_OUT(s32, 32, n), ARG_OUT(err, 1, n)};
    if (missing(args)) return P2E_E_INVALID;
    const Aff* table = nullptr;
    int chosen = 0;
    if (int rc = sign_prepare(c, curve, plan, n, &table, &chosen, args)) return rc;
    if (n == 0) return 0;
    Staged S(c);
    if (long rc = S.begin(args)) return rc;
    if (curve == P2E_CURVE_P256)
        launch_sign<P256>(c, chosen, table, msg32, sk32, k32, r32, s32, n, err);
    else
        launch_sign<Secp256k1>(c, chosen, table, msg32, sk32, k32, r32, s32, n, err);
    return S.end();
}
// sign_message with the recovery byte, and the recovery of the public key from (msg, r, s, v) (recover.hpp)
extern "C" long p2e_ecdsa_sign_recoverable_batch(p2e_ctx* c, int curve, unsigned plan, const uint8_t* msg32, const uint8_t* sk32,
                                                 const uint8_t* k32, uint8_t* r32, uint8_t* s32, uint8_t* v, size_t n, uint8_t* err) {
    const Args args = {ARG_IN(msg32, 32, n), ARG_IN(sk32, 32, n), ARG_IN(k32, 32, n), ARG_OUT(r32, 32, n),
                       ARG_OUT(s32, 32, n),  ARG_OUT(v, 1, n),    ARG_OUT(err, 1, n)};
    if (missing(args)) return P2E_E_INVALID;
    const Aff* table = nullptr;
    int chosen = 0;
    if (int rc = sign_prepare(c, curve, plan, n, &table, &chosen, args)) return rc;
    if (n == 0) return 0;
    Staged S(c);
    if (long rc = S.begin(args)) return rc;
    if (curve == P2E_CURVE_P256)
        launch_sign_recoverable<P256>(c, chosen, table, msg32, sk32, k32, r32, s32, v, n, err);
    else
        launch_sign_recoverable<Secp256k1>(c, chosen, table, msg32, sk32, k32, r32, s32, v, n, err);
    return S.end();
}
extern "C" long p2e_ecdsa_recover_batch(p2e_ctx* c, int curve, const uint8_t* msg32, const uint8_t* r32, const uint8_t* s32, const uint8_t* v,
                                        uint8_t* pkx32, uint8_t* pky32, size_t n, uint8_t* err) {
    const Args args = {ARG_IN(msg32, 32, n),  ARG_IN(r32, 32, n),    ARG_IN(s32, 32, n), ARG_IN(v, 1, n),
                       ARG_OUT(pkx32, 32, n), ARG_OUT(pky32, 32, n), ARG_OUT(err, 1, n)};
    if (missing(args)) return P2E_E_INVALID;
    const Aff* table = nullptr;
    int chosen = 0;
    if (int rc = sign_prepare(c, curve, P2E_SIGN_PLAN_LANE, n, &table, &chosen, args)) return rc;
    if (n == 0) return 0;
    Staged S(c);
    if (long rc = S.begin(args)) return rc;
    if (curve == P2E_CURVE_P256)
        launch_recover<P256>(c, table, msg32, r32, s32, v, pkx32, pky32, n, err);
    else
        launch_recover<Secp256k1>(c, table, msg32, r32, s32, v, pkx32, pky32, n, err);
    return S.end();
}
#endif   // P2E_HAS(0)

// ====================================================================================================
// message hashing, RFC 6979 nonces, Ethereum addresses (hash.hpp)
// ====================================================================================================
// one launch each on the caller's stream; defined in part 1 (the part that builds fastest), called from part 0
void launch_hash(p2e_ctx* c, int alg, unsigned form, const uint8_t* data, const uint64_t* offsets, uint8_t* out32, size_t n);
void launch_nonce_rfc6979(p2e_ctx* c, int curve, const uint8_t* msg32, const uint8_t* sk32, uint8_t* k32, size_t n);
void launch_eth_address(p2e_ctx* c, const uint8_t* pkx32, const uint8_t* pky32, const uint8_t* err, uint8_t* addr20, size_t n);
#if P2E_HAS(1)
void launch_hash(p2e_ctx* c, int alg, unsigned form, const uint8_t* data, const uint64_t* offsets, uint8_t* out32, size_t n) {
    if (alg == P2E_HASH_KECCAK256)
        hipLaunchKernelGGL((k_hash<HASH_KECCAK256>), grid1(n), dim3(BS), 0, c->stream, data, offsets, out32, n, form, c->d_counter);
    else if (alg == P2E_HASH_SHA256D)
        hipLaunchKernelGGL((k_hash<HASH_SHA256D>), grid1(n), dim3(BS), 0, c->stream, data, offsets, out32, n, form, c->d_counter);
    else
        hipLaunchKernelGGL((k_hash<HASH_SHA256>), grid1(n), dim3(BS), 0, c->stream, data, offsets, out32, n, form, c->d_counter);
}
void launch_nonce_rfc6979(p2e_ctx* c, int curve, const uint8_t* msg32, const uint8_t* sk32, uint8_t* k32, size_t n) {
    if (curve == P2E_CURVE_P256)
        hipLaunchKernelGGL((k_nonce_rfc6979<ModN256>), grid1(n), dim3(BS), 0, c->stream, msg32, sk32, k32, n);
    else
        hipLaunchKernelGGL((k_nonce_rfc6979<ModN>), grid1(n), dim3(BS), 0, c->stream, msg32, sk32, k32, n);
}
void launch_eth_address(p2e_ctx* c, const uint8_t* pkx32, const uint8_t* pky32, const uint8_t* err, uint8_t* addr20, size_t n) {
    if (err)
        hipLaunchKernelGGL((k_eth_address<true>), grid1(n), dim3(BS), 0, c->stream, pkx32, pky32, err, addr20, n);
    else
        hipLaunchKernelGGL((k_eth_address<false>), grid1(n), dim3(BS), 0, c->stream, pkx32, pky32, err, addr20, n);
}
#endif   // P2E_HAS(1)

#if P2E_HAS(0)
// the variable-length input of a staged call: the copy holds data[offsets[0], offsets[n]) and `data` becomes that copy moved
// back by offsets[0], as in p2e_hash_batch.  false: offsets[n] < offsets[0] (the error text is set)
// `args`: the call's list, not yet staged (offsets is read here on the host); the extent of data, known here alone, must
// not touch the list's outputs (BUFFER OVERLAP, include/p2e.h).  `name`: what the argument is called where a call has two
static bool wire_stage_elements(Staged& S, Args args, const uint8_t*& data, const uint64_t* offsets, size_t n, const char* name = "data") {
    if (!S.host) return true;
    const uint64_t first = offsets[0], last = offsets[n];
    if (last < first) {
        set_error(std::strcmp(name, "data") ? std::string("the last offset of ") + name + " lies below the first" : "offsets[n] < offsets[0]");
        return false;
    }
    overlap::Span spans[call_args::kMaxBufs + 1];
    size_t num = 0;
    for (size_t i = 0, all = call_args::spans(args, n, spans); i < all; i++)
        if (spans[i].is_output) spans[num++] = spans[i];
    spans[num++] = overlap::Span{name, data + first, 1, (size_t)(last - first), false, true};   // (no lane owns a byte of it)
    if (const overlap::Clash k = overlap::check(spans, num); k.bad) {
        set_error(std::string("overlap: ") + k.a + " and " + k.b + " share bytes (variable-length data may not touch an output)");
        return false;
    }
    const uint8_t* d = S.in(data + first, (size_t)(last - first));
    data = d ? d - first : nullptr;
    return true;
}
extern "C" long p2e_hash_batch(p2e_ctx* c, int alg, unsigned out_form, const uint8_t* data, const uint64_t* offsets, uint8_t* out32,
                               size_t n) {
    const Args args = {ARG_OPAQUE(data), ARG_IN(offsets, 8, n + 1), ARG_OUT(out32, 32, n)};
    if (missing(args)) return P2E_E_INVALID;
    if (alg != P2E_HASH_SHA256 && alg != P2E_HASH_SHA256D && alg != P2E_HASH_KECCAK256) {
        set_error("unknown alg (P2E_HASH_SHA256, P2E_HASH_SHA256D or P2E_HASH_KECCAK256)");
        return P2E_E_INVALID;
    }
    if (out_form != P2E_DIGEST_BYTES && out_form != P2E_DIGEST_SCALAR) {
        set_error("unknown out_form (P2E_DIGEST_BYTES or P2E_DIGEST_SCALAR)");
        return P2E_E_INVALID;
    }
    if (batch_too_large(n) || bad_overlap(n, args) || bad_ctx(c)) return P2E_E_INVALID;
    if (n == 0) return 0;
    Staged S(c);
    if (!wire_stage_elements(S, args, data, offsets, n)) return S.done(P2E_E_INVALID);
    if (long rc = S.begin(args)) return rc;
    launch_hash(c, alg, out_form, data, offsets, out32, n);
    return S.end();
}
extern "C" long p2e_ecdsa_nonce_rfc6979_batch(p2e_ctx* c, int curve, const uint8_t* msg32, const uint8_t* sk32, uint8_t* k32, size_t n) {
    const Args args = {ARG_IN(msg32, 32, n), ARG_IN(sk32, 32, n), ARG_OUT(k32, 32, n)};
    if (missing(args) || bad_curve(curve) || batch_too_large(n) || bad_overlap(n, args) || bad_ctx(c)) return P2E_E_INVALID;
    if (n == 0) return 0;
    Staged S(c);
    if (long rc = S.begin(args)) return rc;
    launch_nonce_rfc6979(c, curve, msg32, sk32, k32, n);
    return S.end();
}
// the nonce kernel into the context's scratch, the unchanged signer behind it, then the wipe: all on the caller's stream
extern "C" long p2e_ecdsa_sign_deterministic_batch(p2e_ctx* c, int curve, unsigned plan, const uint8_t* msg32, const uint8_t* sk32,
                                                   uint8_t* r32, uint8_t* s32, uint8_t* v, size_t n, uint8_t* err) {
    const Args args = {ARG_IN(msg32, 32, n), ARG_IN(sk32, 32, n),  ARG_OUT(r32, 32, n),
                       ARG_OUT(s32, 32, n),  ARG_OUT_OPT(v, 1, n), ARG_OUT(err, 1, n)};
    if (missing(args)) return P2E_E_INVALID;
    const Aff* table = nullptr;
    int chosen = 0;
    if (int rc = sign_prepare(c, curve, plan, n, &table, &chosen, args)) return rc;
    if (n == 0) return 0;
    Staged S(c);
    if (int rc = ensure_scratch(c, n * 32)) return S.done(rc);
    uint8_t* const k32 = static_cast<uint8_t*>(c->scratch);
    if (long rc = S.begin(args)) return rc;
    launch_nonce_rfc6979(c, curve, msg32, sk32, k32, n);
    if (curve == P2E_CURVE_P256) {
        if (v)
            launch_sign_recoverable<P256>(c, chosen, table, msg32, sk32, k32, r32, s32, v, n, err);
        else
            launch_sign<P256>(c, chosen, table, msg32, sk32, k32, r32, s32, n, err);
    } else {
        if (v)
            launch_sign_recoverable<Secp256k1>(c, chosen, table, msg32, sk32, k32, r32, s32, v, n, err);
        else
            launch_sign<Secp256k1>(c, chosen, table, msg32, sk32, k32, r32, s32, n, err);
    }
    HIP_TRY(hipMemsetAsync(k32, 0, n * 32, c->stream));   // the nonces are secret: gone once the signer has read them
    return S.end();
}
extern "C" long p2e_eth_address_batch(p2e_ctx* c, const uint8_t* pkx32, const uint8_t* pky32, const uint8_t* err, uint8_t* addr20,
                                      size_t n) {
    const Args args = {ARG_IN(pkx32, 32, n), ARG_IN(pky32, 32, n), ARG_IN_OPT(err, 1, n), ARG_OUT(addr20, 20, n)};
    if (missing(args) || batch_too_large(n) || bad_overlap(n, args) || bad_ctx(c)) return P2E_E_INVALID;
    if (n == 0) return 0;
    Staged S(c);
    if (long rc = S.begin(args)) return rc;
    launch_eth_address(c, pkx32, pky32, err, addr20, n);
    return S.end();
}
#endif   // P2E_HAS(0)

// ====================================================================================================
// SEC1 keys and DER / compact signatures in wire form (wire.hpp)
// ====================================================================================================
// one launch each on the caller's stream; defined in part 1 beside the hashing kernels, called from part 0
void launch_point_decode(p2e_ctx* c, int curve, const uint8_t* data, const uint64_t* offsets, uint8_t* px32, uint8_t* py32, size_t n,
                         uint8_t* err);
void launch_point_encode(p2e_ctx* c, int curve, int form, const uint8_t* px32, const uint8_t* py32, uint8_t* out, size_t n, uint8_t* err);
void launch_sig_decode(p2e_ctx* c, int curve, int form, unsigned flags, const uint8_t* data, const uint64_t* offsets, uint8_t* r32,
                       uint8_t* s32, uint8_t* v, size_t n, uint8_t* err);
void launch_sig_encode(p2e_ctx* c, int curve, int form, unsigned flags, const uint8_t* r32, const uint8_t* s32, const uint8_t* v,
                       uint8_t* out, uint8_t* out_len, size_t n, uint8_t* err);
#if P2E_HAS(1)
void launch_point_decode(p2e_ctx* c, int curve, const uint8_t* data, const uint64_t* offsets, uint8_t* px32, uint8_t* py32, size_t n,
                         uint8_t* err) {
    if (curve == P2E_CURVE_P256)
        hipLaunchKernelGGL((k_point_decode<P256>), grid1(n), dim3(BS), 0, c->stream, data, offsets, px32, py32, n, err, c->d_counter);
    else
        hipLaunchKernelGGL((k_point_decode<Secp256k1>), grid1(n), dim3(BS), 0, c->stream, data, offsets, px32, py32, n, err, c->d_counter);
}
template <class CV>
static void launch_point_encode_cv(p2e_ctx* c, int form, const uint8_t* px32, const uint8_t* py32, uint8_t* out, size_t n, uint8_t* err) {
    if (form == P2E_SEC1_COMPRESSED)
        hipLaunchKernelGGL((k_point_encode<CV, SEC1_COMPRESSED>), grid1(n), dim3(BS), 0, c->stream, px32, py32, out, n, err, c->d_counter);
    else
        hipLaunchKernelGGL((k_point_encode<CV, SEC1_UNCOMPRESSED>), grid1(n), dim3(BS), 0, c->stream, px32, py32, out, n, err, c->d_counter);
}
void launch_point_encode(p2e_ctx* c, int curve, int form, const uint8_t* px32, const uint8_t* py32, uint8_t* out, size_t n, uint8_t* err) {
    if (curve == P2E_CURVE_P256)
        launch_point_encode_cv<P256>(c, form, px32, py32, out, n, err);
    else
        launch_point_encode_cv<Secp256k1>(c, form, px32, py32, out, n, err);
}
template <class CV>
static void launch_sig_decode_cv(p2e_ctx* c, int form, unsigned flags, const uint8_t* data, const uint64_t* offsets, uint8_t* r32,
                                 uint8_t* s32, uint8_t* v, size_t n, uint8_t* err) {
    if (form == P2E_SIG_DER)
        hipLaunchKernelGGL((k_sig_decode<CV, SIG_DER>), grid1(n), dim3(BS), 0, c->stream, flags, data, offsets, r32, s32, v, n, err,
                           c->d_counter);
    else if (form == P2E_SIG_COMPACT64)
        hipLaunchKernelGGL((k_sig_decode<CV, SIG_COMPACT64>), grid1(n), dim3(BS), 0, c->stream, flags, data, offsets, r32, s32, v, n, err,
                           c->d_counter);
    else
        hipLaunchKernelGGL((k_sig_decode<CV, SIG_COMPACT65>), grid1(n), dim3(BS), 0, c->stream, flags, data, offsets, r32, s32, v, n, err,
                           c->d_counter);
}
void launch_sig_decode(p2e_ctx* c, int curve, int form, unsigned flags, const uint8_t* data, const uint64_t* offsets, uint8_t* r32,
                       uint8_t* s32, uint8_t* v, size_t n, uint8_t* err) {
    if (curve == P2E_CURVE_P256)
        launch_sig_decode_cv<P256>(c, form, flags, data, offsets, r32, s32, v, n, err);
    else
        launch_sig_decode_cv<Secp256k1>(c, form, flags, data, offsets, r32, s32, v, n, err);
}
template <class CV>
static void launch_sig_encode_cv(p2e_ctx* c, int form, unsigned flags, const uint8_t* r32, const uint8_t* s32, const uint8_t* v, uint8_t* out,
                                 uint8_t* out_len, size_t n, uint8_t* err) {
    if (form == P2E_SIG_DER)
        hipLaunchKernelGGL((k_sig_encode<CV, SIG_DER>), grid1(n), dim3(BS), 0, c->stream, flags, r32, s32, v, out, out_len, n, err,
                           c->d_counter);
    else if (form == P2E_SIG_COMPACT64)
        hipLaunchKernelGGL((k_sig_encode<CV, SIG_COMPACT64>), grid1(n), dim3(BS), 0, c->stream, flags, r32, s32, v, out, out_len, n, err,
                           c->d_counter);
    else
        hipLaunchKernelGGL((k_sig_encode<CV, SIG_COMPACT65>), grid1(n), dim3(BS), 0, c->stream, flags, r32, s32, v, out, out_len, n, err,
                           c->d_counter);
}
void launch_sig_encode(p2e_ctx* c, int curve, int form, unsigned flags, const uint8_t* r32, const uint8_t* s32, const uint8_t* v,
                       uint8_t* out, uint8_t* out_len, size_t n, uint8_t* err) {
    if (curve == P2E_CURVE_P256)
        launch_sig_encode_cv<P256>(c, form, flags, r32, s32, v, out, out_len, n, err);
    else
        launch_sig_encode_cv<Secp256k1>(c, form, flags, r32, s32, v, out, out_len, n, err);
}
#endif   // P2E_HAS(1)

#if P2E_HAS(0)
static_assert(P2E_WIRE_OK == WIRE_OK && P2E_WIRE_BAD_LENGTH == WIRE_BAD_LENGTH && P2E_WIRE_BAD_PREFIX == WIRE_BAD_PREFIX &&
                  P2E_WIRE_COORD_RANGE == WIRE_COORD_RANGE && P2E_WIRE_NOT_ON_CURVE == WIRE_NOT_ON_CURVE &&
                  P2E_WIRE_INFINITY == WIRE_INFINITY && P2E_WIRE_DER_SYNTAX == WIRE_DER_SYNTAX &&
                  P2E_WIRE_DER_INTEGER == WIRE_DER_INTEGER && P2E_WIRE_SCALAR_RANGE == WIRE_SCALAR_RANGE && P2E_WIRE_HIGH_S == WIRE_HIGH_S,
              "include/p2e.h and wire.hpp");
static_assert(P2E_SEC1_COMPRESSED == SEC1_COMPRESSED && P2E_SEC1_UNCOMPRESSED == SEC1_UNCOMPRESSED && P2E_SIG_DER == SIG_DER &&
                  P2E_SIG_COMPACT64 == SIG_COMPACT64 && P2E_SIG_COMPACT65 == SIG_COMPACT65 && P2E_SIG_REQUIRE_LOW_S == SIG_REQUIRE_LOW_S &&
                  P2E_SIG_NORMALIZE_S == SIG_NORMALIZE_S && P2E_SIG_DER_STRIDE == SIG_DER_STRIDE,
              "include/p2e.h and wire.hpp");
static bool wire_bad_curve(int curve, size_t n) { return bad_curve(curve) || batch_too_large(n); }
static bool wire_bad_sig_form(int form) {
    if (form == P2E_SIG_DER || form == P2E_SIG_COMPACT64 || form == P2E_SIG_COMPACT65) return false;
    set_error("unknown form (P2E_SIG_DER, P2E_SIG_COMPACT64 or P2E_SIG_COMPACT65)");
    return true;
}
static const char* wire_sig_form_name(int form) {
    return form == P2E_SIG_DER ? "P2E_SIG_DER" : form == P2E_SIG_COMPACT64 ? "P2E_SIG_COMPACT64" : "P2E_SIG_COMPACT65";
}
extern "C" long p2e_point_decode_batch(p2e_ctx* c, int curve, const uint8_t* data, const uint64_t* offsets, uint8_t* px32, uint8_t* py32,
                                       size_t n, uint8_t* err) {
    const Args args = {ARG_OPAQUE(data), ARG_IN(offsets, 8, n + 1), ARG_OUT(px32, 32, n), ARG_OUT(py32, 32, n), ARG_OUT(err, 1, n)};
    if (missing(args) || wire_bad_curve(curve, n) || bad_overlap(n, args) || bad_ctx(c)) return P2E_E_INVALID;
    if (n == 0) return 0;
    Staged S(c);
    if (!wire_stage_elements(S, args, data, offsets, n)) return S.done(P2E_E_INVALID);
    if (long rc = S.begin(args)) return rc;
    launch_point_decode(c, curve, data, offsets, px32, py32, n, err);
    return S.end();
}
extern "C" long p2e_point_encode_batch(p2e_ctx* c, int curve, int form, const uint8_t* px32, const uint8_t* py32, uint8_t* out, size_t n,
                                       uint8_t* err) {
    const Args args = {ARG_IN(px32, 32, n), ARG_IN(py32, 32, n), ARG_OUT(out, form == P2E_SEC1_COMPRESSED ? 33 : 65, n), ARG_OUT(err, 1, n)};
    if (missing(args) || wire_bad_curve(curve, n)) return P2E_E_INVALID;
    if (form != P2E_SEC1_COMPRESSED && form != P2E_SEC1_UNCOMPRESSED) {
        set_error("unknown form (P2E_SEC1_COMPRESSED or P2E_SEC1_UNCOMPRESSED)");
        return P2E_E_INVALID;
    }
    if (bad_overlap(n, args) || bad_ctx(c)) return P2E_E_INVALID;
    if (n == 0) return 0;
    Staged S(c);
    if (long rc = S.begin(args)) return rc;
    launch_point_encode(c, curve, form, px32, py32, out, n, err);
    return S.end();
}
extern "C" long p2e_sig_decode_batch(p2e_ctx* c, int curve, int form, unsigned flags, const uint8_t* data, const uint64_t* offsets,
                                     uint8_t* r32, uint8_t* s32, uint8_t* v, size_t n, uint8_t* err) {
    if (wire_bad_curve(curve, n) || wire_bad_sig_form(form)) return P2E_E_INVALID;
    // an argument its form does not use is ignored: offsets is DER's, v is COMPACT65's (and optional there)
    const bool der = form == P2E_SIG_DER;
    if (form != P2E_SIG_COMPACT65) v = nullptr;
    if (!der) offsets = nullptr;
    // (DER: the extent of data is known on the device alone; the compact forms have a stride)
    const Args args = {der ? ARG_OPAQUE(data) : ARG_IN(data, form == P2E_SIG_COMPACT64 ? 64 : 65, n),
                       ARG_IN_IF(der, offsets, 8, n + 1),
                       ARG_OUT(r32, 32, n),
                       ARG_OUT(s32, 32, n),
                       ARG_OUT_OPT(v, 1, n),
                       ARG_OUT(err, 1, n)};
    if (missing(args, wire_sig_form_name(form))) return P2E_E_INVALID;
    if (flags != 0 && flags != P2E_SIG_REQUIRE_LOW_S && flags != P2E_SIG_NORMALIZE_S) {
        set_error("unknown flags (0, P2E_SIG_REQUIRE_LOW_S or P2E_SIG_NORMALIZE_S)");
        return P2E_E_INVALID;
    }
    if (bad_overlap(n, args) || bad_ctx(c)) return P2E_E_INVALID;
    if (n == 0) return 0;
    Staged S(c);
    if (der && !wire_stage_elements(S, args, data, offsets, n)) return S.done(P2E_E_INVALID);
    if (long rc = S.begin(args)) return rc;
    launch_sig_decode(c, curve, form, flags, data, offsets, r32, s32, v, n, err);
    return S.end();
}
extern "C" long p2e_sig_encode_batch(p2e_ctx* c, int curve, int form, unsigned flags, const uint8_t* r32, const uint8_t* s32,
                                     const uint8_t* v, uint8_t* out, uint8_t* out_len, size_t n, uint8_t* err) {
    if (wire_bad_curve(curve, n) || wire_bad_sig_form(form)) return P2E_E_INVALID;
    // an argument its form does not use is ignored: v is COMPACT65's, out_len is DER's
    const bool der = form == P2E_SIG_DER, with_v = form == P2E_SIG_COMPACT65;
    if (!with_v) v = nullptr;
    if (!der) out_len = nullptr;
    const Args args = {ARG_IN(r32, 32, n),
                       ARG_IN(s32, 32, n),
                       ARG_IN_IF(with_v, v, 1, n),
                       ARG_OUT(out, der ? P2E_SIG_DER_STRIDE : form == P2E_SIG_COMPACT64 ? 64 : 65, n),
                       ARG_OUT_IF(der, out_len, 1, n),
                       ARG_OUT(err, 1, n)};
    if (missing(args, wire_sig_form_name(form))) return P2E_E_INVALID;
    if (flags != 0 && flags != P2E_SIG_NORMALIZE_S) {
        set_error("unknown flags (0 or P2E_SIG_NORMALIZE_S)");
        return P2E_E_INVALID;
    }
    if (bad_overlap(n, args) || bad_ctx(c)) return P2E_E_INVALID;
    if (n == 0) return 0;
    Staged S(c);
    if (long rc = S.begin(args)) return rc;
    launch_sig_encode(c, curve, form, flags, r32, s32, v, out, out_len, n, err);
    return S.end();
}
#endif   // P2E_HAS(0)

// ====================================================================================================
// bucket-method multi-scalar multiplication (pmsm.hpp)
// ====================================================================================================
// the seven launches of one call on the caller's stream; defined in part 1 beside the hashing kernels, called from part 0
template <class CV>
void launch_msm(p2e_ctx* c, const MsmArgs& a);
#if P2E_HAS(1)
template <class CV>
void launch_msm(p2e_ctx* c, const MsmArgs& a) {
    const dim3 bs(BS);
    if (a.n) hipLaunchKernelGGL((k_msm_digits<CV>), grid1(a.n), bs, 0, c->stream, a);
    hipLaunchKernelGGL((k_msm_scan<0>), dim3(1), dim3(MSM_SCAN_LANES), 0, c->stream, a);
    if (a.n) {
        hipLaunchKernelGGL((k_msm_scatter<CV>), grid1(a.n), bs, 0, c->stream, a);
        hipLaunchKernelGGL((k_msm_segment<CV>), grid1(a.max_segments), bs, 0, c->stream, a);
    }
    hipLaunchKernelGGL((k_msm_bucket<CV>), grid1(a.entries), bs, 0, c->stream, a);
    hipLaunchKernelGGL((k_msm_chunk<CV>), grid1((size_t)a.windows * a.chunks), bs, 0, c->stream, a);
    hipLaunchKernelGGL((k_msm_final<CV>), dim3(1), dim3(MSM_FINAL_LANES), 0, c->stream, a);
}
template void launch_msm<Secp256k1>(p2e_ctx*, const MsmArgs&);
template void launch_msm<P256>(p2e_ctx*, const MsmArgs&);
#endif   // P2E_HAS(1)

#if P2E_HAS(0)
static bool msm_bad_args(int curve, size_t n, unsigned window_bits) {
    if (bad_curve(curve)) return true;
    if (window_bits != P2E_MSM_WINDOW_AUTO && (window_bits < P2E_MSM_WINDOW_MIN || window_bits > P2E_MSM_WINDOW_MAX)) {
        set_error("window_bits outside P2E_MSM_WINDOW_AUTO, [P2E_MSM_WINDOW_MIN, P2E_MSM_WINDOW_MAX]");
        return true;
    }
    if (n > MSM_MAX_N) {
        set_error("batch too large for one sum (2^24 points)");
        return true;
    }
    return false;
}
static_assert(P2E_MSM_WINDOW_MIN == MSM_WINDOW_MIN && P2E_MSM_WINDOW_MAX == MSM_WINDOW_MAX, "include/p2e.h and pmsm.hpp");
static_assert(P2E_MSM_OK == MSM_OK && P2E_MSM_NEUTRAL == MSM_NEUTRAL && P2E_MSM_BAD_POINT == MSM_BAD_POINT, "include/p2e.h and pmsm.hpp");
extern "C" int p2e_point_msm_plan(int curve, size_t n, unsigned window_bits, uint64_t* plan) {
    if (!plan) {
        set_error("null pointer (plan is required)");
        return P2E_E_INVALID;
    }
    if (msm_bad_args(curve, n, window_bits)) return P2E_E_INVALID;
    const MsmPlan p = msm_plan(n, window_bits == P2E_MSM_WINDOW_AUTO ? msm_auto_window(n) : window_bits);
    plan[P2E_MSM_PLAN_WINDOW_BITS] = p.c;
    plan[P2E_MSM_PLAN_WINDOWS] = p.windows;
    plan[P2E_MSM_PLAN_BUCKETS] = p.buckets;
    plan[P2E_MSM_PLAN_SEG] = p.seg;
    plan[P2E_MSM_PLAN_SCRATCH_BYTES] = p.total;
    plan[P2E_MSM_PLAN_MAX_LANE_ADDITIONS] = p.max_lane_additions;
    return 0;
}
extern "C" long p2e_point_msm(p2e_ctx* c, int curve, unsigned window_bits, const uint8_t* k32, const uint8_t* px32, const uint8_t* py32,
                              size_t n, uint8_t* outx32, uint8_t* outy32, uint8_t* status, uint8_t* point_err) {
    const Args args = {ARG_SHARED(k32, 32, n), ARG_SHARED(px32, 32, n), ARG_SHARED(py32, 32, n),     ARG_OUT(outx32, 32, 1),
                       ARG_OUT(outy32, 32, 1), ARG_OUT(status, 1, 1),   ARG_OUT_OPT(point_err, 1, n)};
    if (missing(args) || msm_bad_args(curve, n, window_bits) || bad_overlap(n, args) || bad_ctx(c)) return P2E_E_INVALID;
    const MsmPlan P = msm_plan(n, window_bits == P2E_MSM_WINDOW_AUTO ? msm_auto_window(n) : window_bits);
    Staged S(c);
    if (P.total > c->msm_bytes) {
        HIP_TRY(hipStreamSynchronize(c->stream));   // an earlier asynchronous call may still use the block that goes
        c->msm_bytes = 0;
        hipError_t e = c->d_msm.alloc(P.total);
        if (e != hipSuccess) {
            set_error("scratch allocation of " + std::to_string(P.total) + " bytes failed: " + hipGetErrorString(e));
            return S.done(P2E_E_NOMEM);
        }
        c->msm_bytes = P.total;
    }
    if (long rc = S.begin(args)) return rc;
    MsmArgs a = msm_args(P, c->d_msm.get());
    a.k32 = k32, a.px32 = px32, a.py32 = py32;
    a.outx32 = outx32, a.outy32 = outy32, a.status = status, a.point_err = point_err;
    a.counter = c->d_counter;
    HIP_TRY(hipMemsetAsync(c->d_msm.get(), 0, P.o_off, c->stream));   // meta, count, cursor
    if (curve == P2E_CURVE_P256)
        launch_msm<P256>(c, a);
    else
        launch_msm<Secp256k1>(c, a);
    return S.end();
}
#endif   // P2E_HAS(0)

// ====================================================================================================
// per-element point arithmetic (point_arith.hpp): k P, a G + b P, P + Q
// ====================================================================================================
// one launch each on the caller's stream; defined in part 1 beside the many-point sum, called from part 0.
// plan: MUL_PLAN_PLAIN or MUL_PLAN_GLV (secp256k1 only), already chosen; table == nullptr: k P (b = the scalars), else a G + b P
template <class CV>
void launch_point_mul(p2e_ctx* c, int plan, const Aff* table, const uint8_t* a, const uint8_t* b, const uint8_t* px, const uint8_t* py,
                      uint8_t* outx, uint8_t* outy, size_t n, uint8_t* err);
template <class CV>
void launch_point_add(p2e_ctx* c, const uint8_t* px, const uint8_t* py, const uint8_t* qx, const uint8_t* qy, uint8_t* outx, uint8_t* outy,
                      size_t n, uint8_t* err);
#if P2E_HAS(1)
template <class CV, int PLAN>
static void launch_point_mul_plan(p2e_ctx* c, const Aff* table, const uint8_t* a, const uint8_t* b, const uint8_t* px, const uint8_t* py,
                                  uint8_t* outx, uint8_t* outy, size_t n, uint8_t* err) {
    if (table)
        hipLaunchKernelGGL((k_point_lincomb<CV, PLAN>), grid1(n), dim3(BS), 0, c->stream, table, a, b, px, py, outx, outy, n, err,
                           c->d_counter);
    else
        hipLaunchKernelGGL((k_point_mul<CV, PLAN>), grid1(n), dim3(BS), 0, c->stream, b, px, py, outx, outy, n, err, c->d_counter);
}
template <class CV>
void launch_point_mul(p2e_ctx* c, int plan, const Aff* table, const uint8_t* a, const uint8_t* b, const uint8_t* px, const uint8_t* py,
                      uint8_t* outx, uint8_t* outy, size_t n, uint8_t* err) {
    if constexpr (CV::kAZero) {
        if (plan == MUL_PLAN_GLV) return launch_point_mul_plan<CV, MUL_PLAN_GLV>(c, table, a, b, px, py, outx, outy, n, err);
    }
    launch_point_mul_plan<CV, MUL_PLAN_PLAIN>(c, table, a, b, px, py, outx, outy, n, err);
}
template <class CV>
void launch_point_add(p2e_ctx* c, const uint8_t* px, const uint8_t* py, const uint8_t* qx, const uint8_t* qy, uint8_t* outx, uint8_t* outy,
                      size_t n, uint8_t* err) {
    hipLaunchKernelGGL((k_point_add<CV>), grid1(n), dim3(BS), 0, c->stream, px, py, qx, qy, outx, outy, n, err, c->d_counter);
}
template void launch_point_mul<Secp256k1>(p2e_ctx*, int, const Aff*, const uint8_t*, const uint8_t*, const uint8_t*, const uint8_t*, uint8_t*,
                                          uint8_t*, size_t, uint8_t*);
template void launch_point_mul<P256>(p2e_ctx*, int, const Aff*, const uint8_t*, const uint8_t*, const uint8_t*, const uint8_t*, uint8_t*,
                                     uint8_t*, size_t, uint8_t*);
template void launch_point_add<Secp256k1>(p2e_ctx*, const uint8_t*, const uint8_t*, const uint8_t*, const uint8_t*, uint8_t*, uint8_t*, size_t,
                                          uint8_t*);
template void launch_point_add<P256>(p2e_ctx*, const uint8_t*, const uint8_t*, const uint8_t*, const uint8_t*, uint8_t*, uint8_t*, size_t,
                                     uint8_t*);
#endif   // P2E_HAS(1)

#if P2E_HAS(0)
static_assert(P2E_MUL_PLAN_AUTO == MUL_PLAN_AUTO && P2E_MUL_PLAN_PLAIN == MUL_PLAN_PLAIN && P2E_MUL_PLAN_GLV == MUL_PLAN_GLV,
              "include/p2e.h and point_arith.hpp");
// curve / plan checks of the two multiplying calls; *chosen = the walk.  AUTO on secp256k1 is GLV at every n: it is faster
// than PLAIN by far more than the spread at each measured size (MEASUREMENTS.md section 16: 0.83 of PLAIN's time at 2^12,
// 0.84 at 2^16, 0.63 at 2^20), and below 2^12 the call is one wave's dependent chain, which GLV halves.  P-256 has PLAIN only.
static int point_mul_prepare(int curve, unsigned plan, size_t n, int* chosen) {
    if (bad_curve(curve)) return P2E_E_INVALID;
    if (plan != P2E_MUL_PLAN_AUTO && plan != P2E_MUL_PLAN_PLAIN && plan != P2E_MUL_PLAN_GLV) {
        set_error("unknown plan (P2E_MUL_PLAN_AUTO, P2E_MUL_PLAN_PLAIN or P2E_MUL_PLAN_GLV)");
        return P2E_E_INVALID;
    }
    if (plan == P2E_MUL_PLAN_GLV && curve != P2E_CURVE_SECP256K1) {
        set_error("P2E_MUL_PLAN_GLV needs the endomorphism of secp256k1");
        return P2E_E_INVALID;
    }
    if (batch_too_large(n)) return P2E_E_INVALID;
    *chosen = plan == P2E_MUL_PLAN_AUTO ? (curve == P2E_CURVE_SECP256K1 ? MUL_PLAN_GLV : MUL_PLAN_PLAIN) : (int)plan;
    return 0;
}
extern "C" long p2e_point_mul_batch(p2e_ctx* c, int curve, unsigned plan, const uint8_t* k32, const uint8_t* px32, const uint8_t* py32,
                                    uint8_t* outx32, uint8_t* outy32, size_t n, uint8_t* err) {
    const Args args = {ARG_IN(k32, 32, n),     ARG_IN(px32, 32, n),    ARG_IN(py32, 32, n),
                       ARG_OUT(outx32, 32, n), ARG_OUT(outy32, 32, n), ARG_OUT(err, 1, n)};
    if (missing(args)) return P2E_E_INVALID;
    int chosen = 0;
    if (int rc = point_mul_prepare(curve, plan, n, &chosen)) return rc;
    if (bad_overlap(n, args) || bad_ctx(c)) return P2E_E_INVALID;
    if (n == 0) return 0;
    Staged S(c);
    if (long rc = S.begin(args)) return rc;
    if (curve == P2E_CURVE_P256)
        launch_point_mul<P256>(c, chosen, nullptr, nullptr, k32, px32, py32, outx32, outy32, n, err);
    else
        launch_point_mul<Secp256k1>(c, chosen, nullptr, nullptr, k32, px32, py32, outx32, outy32, n, err);
    return S.end();
}
extern "C" long p2e_point_lincomb_batch(p2e_ctx* c, int curve, unsigned plan, const uint8_t* a32, const uint8_t* b32, const uint8_t* px32,
                                        const uint8_t* py32, uint8_t* outx32, uint8_t* outy32, size_t n, uint8_t* err) {
    const Args args = {ARG_IN(a32, 32, n),     ARG_IN(b32, 32, n),     ARG_IN(px32, 32, n), ARG_IN(py32, 32, n),
                       ARG_OUT(outx32, 32, n), ARG_OUT(outy32, 32, n), ARG_OUT(err, 1, n)};
    if (missing(args)) return P2E_E_INVALID;
    int chosen = 0, lane = 0;
    if (int rc = point_mul_prepare(curve, plan, n, &chosen)) return rc;
    const Aff* table = nullptr;
    if (int rc = sign_prepare(c, curve, P2E_SIGN_PLAN_LANE, n, &table, &lane, args)) return rc;
    if (n == 0) return 0;
    Staged S(c);
    if (long rc = S.begin(args)) return rc;
    if (curve == P2E_CURVE_P256)
        launch_point_mul<P256>(c, chosen, table, a32, b32, px32, py32, outx32, outy32, n, err);
    else
        launch_point_mul<Secp256k1>(c, chosen, table, a32, b32, px32, py32, outx32, outy32, n, err);
    return S.end();
}
extern "C" long p2e_point_add_batch(p2e_ctx* c, int curve, const uint8_t* px32, const uint8_t* py32, const uint8_t* qx32, const uint8_t* qy32,
                                    uint8_t* outx32, uint8_t* outy32, size_t n, uint8_t* err) {
    const Args args = {ARG_IN(px32, 32, n),    ARG_IN(py32, 32, n),    ARG_IN(qx32, 32, n), ARG_IN(qy32, 32, n),
                       ARG_OUT(outx32, 32, n), ARG_OUT(outy32, 32, n), ARG_OUT(err, 1, n)};
    if (missing(args)) return P2E_E_INVALID;
    int chosen = 0;
    if (int rc = point_mul_prepare(curve, P2E_MUL_PLAN_PLAIN, n, &chosen)) return rc;
    if (bad_overlap(n, args) || bad_ctx(c)) return P2E_E_INVALID;
    if (n == 0) return 0;
    Staged S(c);
    if (long rc = S.begin(args)) return rc;
    if (curve == P2E_CURVE_P256)
        launch_point_add<P256>(c, px32, py32, qx32, qy32, outx32, outy32, n, err);
    else
        launch_point_add<Secp256k1>(c, px32, py32, qx32, qy32, outx32, outy32, n, err);
    return S.end();
}
#endif   // P2E_HAS(0)

// ====================================================================================================
// point tables (point_table.hpp): precomputed window tables of the caller's points, and the calls that walk them
// ====================================================================================================
// A table belongs to the device of the context that made it; `tab` is Aff[m][FB_WINDOWS][16].
struct PointTable {
    int curve = 0, device = 0;
    size_t m = 0;
    DeviceArray<Aff> tab;
};
// defined in part 1 beside the per-element point arithmetic, called from part 0.  All on the caller's stream.
// scratch: TABLE_POW_BYTES per (point, window), then one u32 flag per point (zeroed), then one err byte per point
template <class CV>
void launch_table_powers(p2e_ctx* c, const uint8_t* px, const uint8_t* py, void* pow, size_t m, uint8_t* perr);
template <class CV>
void launch_table_rows(p2e_ctx* c, const void* pow, Aff* tab, size_t m, u32* flag, uint8_t* perr);
// what: 0 = k T[idx] (b = the scalars), 1 = a G + b T[idx], 2 = the verdict (a = msg, b = r, s; out = valid)
template <class CV>
void launch_table_call(p2e_ctx* c, int what, const Aff* G, const Aff* tab, const u32* idx, u32 m, const uint8_t* a, const uint8_t* b,
                       const uint8_t* s, uint8_t* outx, uint8_t* outy, size_t n, uint8_t* err);
#if P2E_HAS(1)
template <class CV>
void launch_table_powers(p2e_ctx* c, const uint8_t* px, const uint8_t* py, void* pow, size_t m, uint8_t* perr) {
    hipLaunchKernelGGL((k_table_powers<CV>), grid1(m), dim3(BS), 0, c->stream, px, py, pow, m, perr, c->d_counter);
}
template <class CV>
void launch_table_rows(p2e_ctx* c, const void* pow, Aff* tab, size_t m, u32* flag, uint8_t* perr) {
    const size_t rows = m * FB_WINDOWS;
    hipLaunchKernelGGL((k_table_rows<CV>), grid1(rows), dim3(BS), 0, c->stream, pow, tab, rows, flag, perr, c->d_counter);
}
template <class CV>
void launch_table_call(p2e_ctx* c, int what, const Aff* G, const Aff* tab, const u32* idx, u32 m, const uint8_t* a, const uint8_t* b,
                       const uint8_t* s, uint8_t* outx, uint8_t* outy, size_t n, uint8_t* err) {
    if (what == 0)
        hipLaunchKernelGGL((k_table_mul<CV>), grid1(n), dim3(BS), 0, c->stream, tab, idx, m, b, outx, outy, n, err, c->d_counter);
    else if (what == 1)
        hipLaunchKernelGGL((k_table_lincomb<CV>), grid1(n), dim3(BS), 0, c->stream, G, tab, idx, m, a, b, outx, outy, n, err,
                           c->d_counter);
    else
        hipLaunchKernelGGL((k_table_verify<CV>), grid1(n), dim3(BS), 0, c->stream, G, tab, idx, m, a, b, s, n, err, outx, c->d_counter);
}
template void launch_table_powers<Secp256k1>(p2e_ctx*, const uint8_t*, const uint8_t*, void*, size_t, uint8_t*);
template void launch_table_powers<P256>(p2e_ctx*, const uint8_t*, const uint8_t*, void*, size_t, uint8_t*);
template void launch_table_rows<Secp256k1>(p2e_ctx*, const void*, Aff*, size_t, u32*, uint8_t*);
template void launch_table_rows<P256>(p2e_ctx*, const void*, Aff*, size_t, u32*, uint8_t*);
template void launch_table_call<Secp256k1>(p2e_ctx*, int, const Aff*, const Aff*, const u32*, u32, const uint8_t*, const uint8_t*,
                                           const uint8_t*, uint8_t*, uint8_t*, size_t, uint8_t*);
template void launch_table_call<P256>(p2e_ctx*, int, const Aff*, const Aff*, const u32*, u32, const uint8_t*, const uint8_t*, const uint8_t*,
                                      uint8_t*, uint8_t*, size_t, uint8_t*);
#endif   // P2E_HAS(1)

#if P2E_HAS(0)
static_assert(P2E_WIRE_BAD_INDEX == WIRE_BAD_INDEX && P2E_POINT_TABLE_MAX_POINTS == TABLE_MAX_POINTS &&
                  P2E_POINT_TABLE_BYTES_PER_POINT == TABLE_POINT_ENTRIES * sizeof(Aff),
              "include/p2e.h and point_table.hpp");
// the stream's work done and the flagged count on the host, whatever the context's mode (create must count rejections)
static long table_wait_count(p2e_ctx* c) {
    if (long r = fetch_count(c)) return r;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return (long)*c->h_counter;
}
extern "C" long p2e_point_table_create(p2e_ctx* c, int curve, const uint8_t* px32, const uint8_t* py32, size_t m, uint8_t* point_err,
                                       void** out) {
    if (out) *out = nullptr;
    // (each point's powers and rows are built by many lanes over two launches: nothing here is in place)
    const Args args = {ARG_SHARED(px32, 32, m), ARG_SHARED(py32, 32, m), ARG_OUT_OPT(point_err, 1, m), ARG_OPAQUE(out)};
    if (missing(args) || bad_curve(curve)) return P2E_E_INVALID;
    if (m < 1 || m > P2E_POINT_TABLE_MAX_POINTS) {
        set_error("a table holds 1 .. P2E_POINT_TABLE_MAX_POINTS points");
        return P2E_E_INVALID;
    }
    if (bad_overlap(m, args) || bad_ctx(c)) return P2E_E_INVALID;
    Staged S(c);   // (its guard puts the context's device in place and restores the caller's)
    std::unique_ptr<PointTable> t(new PointTable());
    t->curve = curve, t->device = c->device, t->m = m;
    const size_t rows = m * FB_WINDOWS, flag_off = (rows * TABLE_POW_BYTES + 3) & ~(size_t)3, err_off = flag_off + 4 * m;
    DeviceArray<unsigned char> scratch;
    hipError_t e = scratch.alloc(err_off + m);
    if (e == hipSuccess) e = t->tab.alloc(m * TABLE_POINT_ENTRIES);
    if (e != hipSuccess) {
        set_error("allocation of a table of " + std::to_string(m) + " points failed: " + hipGetErrorString(e));
        return S.done(P2E_E_NOMEM);
    }
    u32* flag = reinterpret_cast<u32*>(scratch.get() + flag_off);
    uint8_t* perr = scratch.get() + err_off;
    if (long rc = S.begin(args)) return rc;
    HIP_TRY(hipMemsetAsync(flag, 0, 4 * m, c->stream));
    if (curve == P2E_CURVE_P256)
        launch_table_powers<P256>(c, px32, py32, scratch.get(), m, perr);
    else
        launch_table_powers<Secp256k1>(c, px32, py32, scratch.get(), m, perr);
    long bad = table_wait_count(c);
    if (bad == 0) {   // every point is fine: build the rows (a zero Z there rejects its point, see point_table.hpp)
        if (curve == P2E_CURVE_P256)
            launch_table_rows<P256>(c, scratch.get(), t->tab.get(), m, flag, perr);
        else
            launch_table_rows<Secp256k1>(c, scratch.get(), t->tab.get(), m, flag, perr);
        bad = table_wait_count(c);
    }
    if (bad >= 0 && point_err) HIP_TRY(hipMemcpy(point_err, perr, m, hipMemcpyDefault));
    if (bad == 0) *out = t.release();
    return S.done(bad);
}
extern "C" void p2e_point_table_destroy(p2e_ctx* c, void* table) {
    PointTable* t = static_cast<PointTable*>(table);
    if (!t) return;
    DeviceGuard guard(t->device);
    if (c && c->stream) (void)hipStreamSynchronize(c->stream);   // a queued call must not outlive its table
    delete t;
}
extern "C" long p2e_point_table_num_points(const void* table) {
    return table ? (long)static_cast<const PointTable*>(table)->m : P2E_E_INVALID;
}
extern "C" int p2e_point_table_curve(const void* table) {
    return table ? static_cast<const PointTable*>(table)->curve : P2E_E_INVALID;
}
extern "C" int p2e_point_table_read_window(p2e_ctx* c, const void* table, size_t j, int w, uint8_t* out1024) {
    const PointTable* t = static_cast<const PointTable*>(table);
    if (!c || !t || !out1024) {
        set_error("null pointer (ctx, table and out1024 are all required)");
        return P2E_E_INVALID;
    }
    if (t->device != c->device || j >= t->m || w < 0 || w >= FB_WINDOWS) {
        set_error("no such window (the context's device, j < num_points, 0 <= w < 66)");
        return P2E_E_INVALID;
    }
    DeviceGuard guard(c->device);
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(out1024, t->tab.get() + (j * FB_WINDOWS + (size_t)w) * 16, 16 * sizeof(Aff), hipMemcpyDefault));
    return 0;
}
// The three calls that walk a table.  `args`: the caller's own list (table and idx in it); what: as for launch_table_call;
// `launch(G, tab, m, curve_is_p256)`: the caller's launch_table_call with its own arguments, staged by then.
template <class Launch>
static long table_call(p2e_ctx* c, const void* table, int what, size_t n, Args args, Launch&& launch) {
    if (missing(args) || bad_overlap(n, args) || bad_ctx(c)) return P2E_E_INVALID;
    const PointTable* t = static_cast<const PointTable*>(table);
    if (t->device != c->device) {
        set_error("the table belongs to another device than the context");
        return P2E_E_INVALID;
    }
    if (batch_too_large(n)) return P2E_E_INVALID;
    const Aff* G = nullptr;
    int lane = 0;
    if (what != 0)
        if (int rc = sign_prepare(c, t->curve, P2E_SIGN_PLAN_LANE, n, &G, &lane)) return rc;
    if (n == 0) return 0;
    Staged S(c);
    if (long rc = S.begin(args)) return rc;
    launch(G, t->tab.get(), (u32)t->m, t->curve == P2E_CURVE_P256);
    return S.end();
}
// a = a32 / msg32 (null for what == 0), b = k32 / b32 / r32, s = s32 (what == 2 only), out1 = outx32 / valid, out2 = outy32
#define TABLE_LAUNCH(what, a, b, s, out1, out2)                                                         \
    [&](const Aff* G, const Aff* tab, u32 m, bool p256) {                                               \
        if (p256)                                                                                       \
            launch_table_call<P256>(c, what, G, tab, idx, m, a, b, s, out1, out2, n, err);              \
        else                                                                                            \
            launch_table_call<Secp256k1>(c, what, G, tab, idx, m, a, b, s, out1, out2, n, err);         \
    }
extern "C" long p2e_point_table_mul_batch(p2e_ctx* c, const void* table, const uint32_t* idx, const uint8_t* k32, uint8_t* outx32,
                                          uint8_t* outy32, size_t n, uint8_t* err) {
    return table_call(c, table, 0, n,
                      {ARG_OPAQUE(table), ARG_IN_OPT(idx, 4, n), ARG_IN(k32, 32, n), ARG_OUT(outx32, 32, n), ARG_OUT(outy32, 32, n),
                       ARG_OUT(err, 1, n)},
                      TABLE_LAUNCH(0, nullptr, k32, nullptr, outx32, outy32));
}
extern "C" long p2e_point_table_lincomb_batch(p2e_ctx* c, const void* table, const uint32_t* idx, const uint8_t* a32, const uint8_t* b32,
                                              uint8_t* outx32, uint8_t* outy32, size_t n, uint8_t* err) {
    return table_call(c, table, 1, n,
                      {ARG_OPAQUE(table), ARG_IN_OPT(idx, 4, n), ARG_IN(a32, 32, n), ARG_IN(b32, 32, n), ARG_OUT(outx32, 32, n),
                       ARG_OUT(outy32, 32, n), ARG_OUT(err, 1, n)},
                      TABLE_LAUNCH(1, a32, b32, nullptr, outx32, outy32));
}
extern "C" long p2e_ecdsa_verify_table_batch(p2e_ctx* c, const void* table, const uint32_t* idx, const uint8_t* msg32, const uint8_t* r32,
                                             const uint8_t* s32, size_t n, uint8_t* err, uint8_t* valid) {
    return table_call(c, table, 2, n,
                      {ARG_OPAQUE(table), ARG_IN_OPT(idx, 4, n), ARG_IN(msg32, 32, n), ARG_IN(r32, 32, n), ARG_IN(s32, 32, n),
                       ARG_OUT(valid, 1, n), ARG_OUT(err, 1, n)},
                      TABLE_LAUNCH(2, msg32, r32, s32, valid, nullptr));
}
#undef TABLE_LAUNCH
#endif   // P2E_HAS(0)

// ====================================================================================================
// BIP-340 Schnorr signatures on secp256k1 (schnorr.hpp): keys, signing, the per-element verdict, the aggregate check
// ====================================================================================================
// The scratch block of the aggregate check: the 2 n + 1 terms in the MSM's input layout, the preparation kernel's per-block
// partial sums, and what the MSM writes besides its own scratch (the sum's coordinates, its status, its rejected count).
struct SchnorrAggLayout {
    size_t o_k, o_px, o_py, o_partial, o_outx, o_outy, o_status, o_rejected, total;
    u32 blocks;
    explicit SchnorrAggLayout(size_t n) {
        size_t at = 0;
        auto take = [&](size_t bytes) {
            const size_t o = at;
            at += (bytes + 255) & ~(size_t)255;
            return o;
        };
        const size_t terms = 2 * n + 1;
        blocks = (u32)((n + SCHNORR_AGG_LANES - 1) / SCHNORR_AGG_LANES);
        o_k = take(terms * 32), o_px = take(terms * 32), o_py = take(terms * 32);
        o_partial = take((size_t)(blocks ? blocks : 1) * sizeof(U256));
        o_outx = take(32), o_outy = take(32), o_status = take(1), o_rejected = take(sizeof(unsigned long long));
        total = at;
    }
};
// one launch each on the caller's stream, the aggregate's three kernels around launch_msm<Secp256k1>; defined in part 3,
// the part with the least code of its own, called from part 0
void launch_schnorr_public_key(p2e_ctx* c, const Aff* table, const uint8_t* sk, uint8_t* pk, size_t n, uint8_t* err);
void launch_schnorr_sign(p2e_ctx* c, const Aff* table, const uint8_t* msg, const uint8_t* sk, const uint8_t* aux, uint8_t* sig, size_t n,
                         uint8_t* err);
void launch_schnorr_verify(p2e_ctx* c, const Aff* table, const uint8_t* msg, const uint8_t* pk, const uint8_t* sig, size_t n, uint8_t* err,
                           uint8_t* valid);
void launch_xonly_decode(p2e_ctx* c, const uint8_t* pk, uint8_t* px, uint8_t* py, size_t n, uint8_t* err);
void launch_schnorr_agg_prepare(p2e_ctx* c, const Aff* table, const SchnorrAggLayout& L, unsigned char* block, const uint8_t* msg,
                                const uint8_t* pk, const uint8_t* sig, const uint8_t* seed, size_t n, uint8_t* err);
void launch_schnorr_agg_verdict(p2e_ctx* c, const SchnorrAggLayout& L, const unsigned char* block, uint8_t* verdict);
#if P2E_HAS(3)
void launch_schnorr_public_key(p2e_ctx* c, const Aff* table, const uint8_t* sk, uint8_t* pk, size_t n, uint8_t* err) {
    hipLaunchKernelGGL((k_schnorr_public_key<0>), grid1(n), dim3(BS), 0, c->stream, table, sk, pk, n, err, c->d_counter);
}
void launch_schnorr_sign(p2e_ctx* c, const Aff* table, const uint8_t* msg, const uint8_t* sk, const uint8_t* aux, uint8_t* sig, size_t n,
                         uint8_t* err) {
    hipLaunchKernelGGL((k_schnorr_sign<0>), grid1(n), dim3(BS), 0, c->stream, table, msg, sk, aux, sig, n, err, c->d_counter);
}
void launch_schnorr_verify(p2e_ctx* c, const Aff* table, const uint8_t* msg, const uint8_t* pk, const uint8_t* sig, size_t n, uint8_t* err,
                           uint8_t* valid) {
    hipLaunchKernelGGL((k_schnorr_verify<0>), grid1(n), dim3(BS), 0, c->stream, table, msg, pk, sig, n, err, valid, c->d_counter);
}
void launch_xonly_decode(p2e_ctx* c, const uint8_t* pk, uint8_t* px, uint8_t* py, size_t n, uint8_t* err) {
    hipLaunchKernelGGL((k_xonly_decode<0>), grid1(n), dim3(BS), 0, c->stream, pk, px, py, n, err, c->d_counter);
}
// the preparation kernel (n > 0) and the finishing kernel: afterwards the block holds all 2 n + 1 terms
void launch_schnorr_agg_prepare(p2e_ctx* c, const Aff* table, const SchnorrAggLayout& L, unsigned char* block, const uint8_t* msg,
                                const uint8_t* pk, const uint8_t* sig, const uint8_t* seed, size_t n, uint8_t* err) {
    static_assert(SCHNORR_AGG_LANES == BS, "the preparation kernel's block is the library's block");
    U256* partial = reinterpret_cast<U256*>(block + L.o_partial);
    if (n)
        hipLaunchKernelGGL((k_schnorr_agg_prepare<0>), dim3(L.blocks), dim3(SCHNORR_AGG_LANES), 0, c->stream, msg, pk, sig, seed, n,
                           block + L.o_k, block + L.o_px, block + L.o_py, partial, err, c->d_counter);
    hipLaunchKernelGGL((k_schnorr_agg_finish<0>), dim3(1), dim3(SCHNORR_AGG_LANES), 0, c->stream, table, partial, L.blocks, block + L.o_k,
                       block + L.o_px, block + L.o_py);
}
void launch_schnorr_agg_verdict(p2e_ctx* c, const SchnorrAggLayout& L, const unsigned char* block, uint8_t* verdict) {
    hipLaunchKernelGGL((k_schnorr_agg_verdict<0>), dim3(1), dim3(64), 0, c->stream, block + L.o_status, c->d_counter, verdict);
}
#endif   // P2E_HAS(3)

#if P2E_HAS(0)
// the generator's table; n beyond one launch is refused (sign_prepare's rule)
static int schnorr_prepare(p2e_ctx* c, size_t n, const Aff** table, Args args) {
    int lane = 0;
    return sign_prepare(c, P2E_CURVE_SECP256K1, P2E_SIGN_PLAN_LANE, n, table, &lane, args);
}
extern "C" long p2e_schnorr_public_key_batch(p2e_ctx* c, const uint8_t* sk32, uint8_t* pk32, size_t n, uint8_t* err) {
    const Args args = {ARG_IN(sk32, 32, n), ARG_OUT(pk32, 32, n), ARG_OUT(err, 1, n)};
    if (missing(args)) return P2E_E_INVALID;
    const Aff* table = nullptr;
    if (int rc = schnorr_prepare(c, n, &table, args)) return rc;
    if (n == 0) return 0;
    Staged S(c);
    if (long rc = S.begin(args)) return rc;
    launch_schnorr_public_key(c, table, sk32, pk32, n, err);
    return S.end();
}
extern "C" long p2e_schnorr_sign_batch(p2e_ctx* c, const uint8_t* msg32, const uint8_t* sk32, const uint8_t* aux32, uint8_t* sig64, size_t n,
                                       uint8_t* err) {
    const Args args = {ARG_IN(msg32, 32, n), ARG_IN(sk32, 32, n), ARG_IN(aux32, 32, n), ARG_OUT(sig64, 64, n), ARG_OUT(err, 1, n)};
    if (missing(args)) return P2E_E_INVALID;
    const Aff* table = nullptr;
    if (int rc = schnorr_prepare(c, n, &table, args)) return rc;
    if (n == 0) return 0;
    Staged S(c);
    if (long rc = S.begin(args)) return rc;
    launch_schnorr_sign(c, table, msg32, sk32, aux32, sig64, n, err);
    return S.end();
}
extern "C" long p2e_schnorr_verify_batch(p2e_ctx* c, const uint8_t* msg32, const uint8_t* pk32, const uint8_t* sig64, size_t n, uint8_t* err,
                                         uint8_t* valid) {
    const Args args = {ARG_IN(msg32, 32, n), ARG_IN(pk32, 32, n), ARG_IN(sig64, 64, n), ARG_OUT(err, 1, n), ARG_OUT(valid, 1, n)};
    if (missing(args)) return P2E_E_INVALID;
    const Aff* table = nullptr;
    if (int rc = schnorr_prepare(c, n, &table, args)) return rc;
    if (n == 0) return 0;
    Staged S(c);
    if (long rc = S.begin(args)) return rc;
    launch_schnorr_verify(c, table, msg32, pk32, sig64, n, err, valid);
    return S.end();
}
extern "C" long p2e_xonly_decode_batch(p2e_ctx* c, const uint8_t* pk32, uint8_t* px32, uint8_t* py32, size_t n, uint8_t* err) {
    const Args args = {ARG_IN(pk32, 32, n), ARG_OUT(px32, 32, n), ARG_OUT(py32, 32, n), ARG_OUT(err, 1, n)};
    if (missing(args) || batch_too_large(n) || bad_overlap(n, args) || bad_ctx(c)) return P2E_E_INVALID;
    if (n == 0) return 0;
    Staged S(c);
    if (long rc = S.begin(args)) return rc;
    launch_xonly_decode(c, pk32, px32, py32, n, err);
    return S.end();
}
// `have` bytes of `block` become at least `want`, behind a stream sync: an earlier asynchronous call may still use the block that goes
static long schnorr_grow(p2e_ctx* c, DeviceArray<unsigned char>& block, size_t& have, size_t want) {
    if (want <= have) return 0;
    HIP_TRY(hipStreamSynchronize(c->stream));
    have = 0;
    hipError_t e = block.alloc(want);
    if (e != hipSuccess) {
        set_error("scratch allocation of " + std::to_string(want) + " bytes failed: " + hipGetErrorString(e));
        return P2E_E_NOMEM;
    }
    have = want;
    return 0;
}
extern "C" long p2e_schnorr_verify_aggregate(p2e_ctx* c, const uint8_t* msg32, const uint8_t* pk32, const uint8_t* sig64, size_t n,
                                             const uint8_t* seed32, unsigned window_bits, uint8_t* verdict, uint8_t* err) {
    const Args args = {ARG_SHARED(msg32, 32, n),  ARG_SHARED(pk32, 32, n), ARG_SHARED(sig64, 64, n),
                       ARG_SHARED(seed32, 32, 1), ARG_OUT(verdict, 1, 1),  ARG_OUT_OPT(err, 1, n)};
    if (missing(args)) return P2E_E_INVALID;
    if (n > MSM_MAX_N / 2) {   // 2 n + 1 > 2^24, without the overflow of 2 n
        set_error("batch too large for one sum (2 n + 1 terms, at most 2^24)");
        return P2E_E_INVALID;
    }
    const size_t terms = 2 * n + 1;
    if (msm_bad_args(P2E_CURVE_SECP256K1, terms, window_bits)) return P2E_E_INVALID;
    const Aff* table = nullptr;
    if (int rc = schnorr_prepare(c, n, &table, args)) return rc;
    Staged S(c);
    if (n == 0) {   // the empty batch holds: nothing to sum
        if (long rc = S.begin(args)) return rc;
        HIP_TRY(hipMemsetAsync(verdict, 1, 1, c->stream));
        return S.end();
    }
    const MsmPlan P = msm_plan(terms, window_bits == P2E_MSM_WINDOW_AUTO ? msm_auto_window(terms) : window_bits);
    const SchnorrAggLayout L(n);
    if (long rc = schnorr_grow(c, c->d_schnorr, c->schnorr_bytes, L.total)) return S.done(rc);
    if (long rc = schnorr_grow(c, c->d_msm, c->msm_bytes, P.total)) return S.done(rc);
    if (long rc = S.begin(args)) return rc;
    unsigned char* block = c->d_schnorr.get();
    MsmArgs a = msm_args(P, c->d_msm.get());
    a.k32 = block + L.o_k, a.px32 = block + L.o_px, a.py32 = block + L.o_py;
    a.outx32 = block + L.o_outx, a.outy32 = block + L.o_outy, a.status = block + L.o_status, a.point_err = nullptr;
    a.counter = reinterpret_cast<unsigned long long*>(block + L.o_rejected);   // (the context's counter holds the flag count)
    HIP_TRY(hipMemsetAsync(c->d_msm.get(), 0, P.o_off, c->stream));   // meta, count, cursor
    launch_schnorr_agg_prepare(c, table, L, block, msg32, pk32, sig64, seed32, n, err);
    launch_msm<Secp256k1>(c, a);
    launch_schnorr_agg_verdict(c, L, block, verdict);
    return S.end();
}
#endif   // P2E_HAS(0)

// ====================================================================================================
// BIP-32 key derivation and HASH160 on secp256k1 (hd.hpp): master keys, CKDpriv, CKDpub, key hashes, message hashes
// ====================================================================================================
// one launch each on the caller's stream; defined in part 1 beside the other hashing kernels, called from part 0
void launch_bip32_master(p2e_ctx* c, const uint8_t* seed, size_t seed_len, uint8_t* sk, uint8_t* cc, size_t n, uint8_t* err);
void launch_bip32_ckd_priv(p2e_ctx* c, const Aff* table, const uint8_t* par_sk, const uint8_t* par_cc, bool broadcast, const uint32_t* index,
                           uint8_t* sk, uint8_t* cc, size_t n, uint8_t* err);
void launch_bip32_ckd_pub(p2e_ctx* c, const Aff* table, const uint8_t* par_pkx, const uint8_t* par_pky, const uint8_t* par_cc, bool broadcast,
                          const uint32_t* index, uint8_t* pkx, uint8_t* pky, uint8_t* cc, size_t n, uint8_t* err);
void launch_key_hash160(p2e_ctx* c, unsigned form, const uint8_t* pkx, const uint8_t* pky, const uint8_t* err, uint8_t* out20, size_t n);
void launch_hash160(p2e_ctx* c, const uint8_t* data, const uint64_t* offsets, uint8_t* out20, size_t n);
#if P2E_HAS(1)
void launch_bip32_master(p2e_ctx* c, const uint8_t* seed, size_t seed_len, uint8_t* sk, uint8_t* cc, size_t n, uint8_t* err) {
    hipLaunchKernelGGL((k_bip32_master<0>), grid1(n), dim3(BS), 0, c->stream, seed, (u32)seed_len, sk, cc, n, err, c->d_counter);
}
void launch_bip32_ckd_priv(p2e_ctx* c, const Aff* table, const uint8_t* par_sk, const uint8_t* par_cc, bool broadcast, const uint32_t* index,
                           uint8_t* sk, uint8_t* cc, size_t n, uint8_t* err) {
    hipLaunchKernelGGL((k_bip32_ckd_priv<0>), grid1(n), dim3(BS), 0, c->stream, table, par_sk, par_cc, broadcast ? 1 : 0, index, sk, cc, n, err,
                       c->d_counter);
}
void launch_bip32_ckd_pub(p2e_ctx* c, const Aff* table, const uint8_t* par_pkx, const uint8_t* par_pky, const uint8_t* par_cc, bool broadcast,
                          const uint32_t* index, uint8_t* pkx, uint8_t* pky, uint8_t* cc, size_t n, uint8_t* err) {
    hipLaunchKernelGGL((k_bip32_ckd_pub<0>), grid1(n), dim3(BS), 0, c->stream, table, par_pkx, par_pky, par_cc, broadcast ? 1 : 0, index, pkx,
                       pky, cc, n, err, c->d_counter);
}
void launch_key_hash160(p2e_ctx* c, unsigned form, const uint8_t* pkx, const uint8_t* pky, const uint8_t* err, uint8_t* out20, size_t n) {
    if (form == P2E_SEC1_COMPRESSED) {
        if (err)
            hipLaunchKernelGGL((k_key_hash160<SEC1_COMPRESSED, true>), grid1(n), dim3(BS), 0, c->stream, pkx, pky, err, out20, n);
        else
            hipLaunchKernelGGL((k_key_hash160<SEC1_COMPRESSED, false>), grid1(n), dim3(BS), 0, c->stream, pkx, pky, err, out20, n);
    } else {
        if (err)
            hipLaunchKernelGGL((k_key_hash160<SEC1_UNCOMPRESSED, true>), grid1(n), dim3(BS), 0, c->stream, pkx, pky, err, out20, n);
        else
            hipLaunchKernelGGL((k_key_hash160<SEC1_UNCOMPRESSED, false>), grid1(n), dim3(BS), 0, c->stream, pkx, pky, err, out20, n);
    }
}
void launch_hash160(p2e_ctx* c, const uint8_t* data, const uint64_t* offsets, uint8_t* out20, size_t n) {
    hipLaunchKernelGGL((k_hash160<0>), grid1(n), dim3(BS), 0, c->stream, data, offsets, out20, n, c->d_counter);
}
#endif   // P2E_HAS(1)

#if P2E_HAS(0)
static_assert(P2E_WIRE_BAD_INDEX == WIRE_BAD_INDEX, "include/p2e.h and point_table.hpp must agree");
// n_parents is 1 (one parent serves the whole batch) or n
static bool bip32_bad_parents(size_t n_parents, size_t n) {
    if (n_parents == 1 || n_parents == n) return false;
    set_error("n_parents must be 1 or n");
    return true;
}
extern "C" long p2e_bip32_master_batch(p2e_ctx* c, const uint8_t* seed, size_t seed_len, uint8_t* sk32, uint8_t* cc32, size_t n, uint8_t* err) {
    const Args args = {ARG_IN(seed, seed_len, n), ARG_OUT(sk32, 32, n), ARG_OUT(cc32, 32, n), ARG_OUT(err, 1, n)};
    if (missing(args)) return P2E_E_INVALID;
    if (seed_len < 16 || seed_len > 64) {
        set_error("seed_len must be 16 .. 64 bytes");
        return P2E_E_INVALID;
    }
    if (batch_too_large(n) || bad_overlap(n, args) || bad_ctx(c)) return P2E_E_INVALID;
    if (n == 0) return 0;
    Staged S(c);
    if (long rc = S.begin(args)) return rc;
    launch_bip32_master(c, seed, seed_len, sk32, cc32, n, err);
    return S.end();
}
extern "C" long p2e_bip32_ckd_priv_batch(p2e_ctx* c, const uint8_t* par_sk32, const uint8_t* par_cc32, size_t n_parents, const uint32_t* index,
                                         uint8_t* sk32, uint8_t* cc32, size_t n, uint8_t* err) {
    const Args args = {ARG_BCAST(par_sk32, 32, n_parents), ARG_BCAST(par_cc32, 32, n_parents), ARG_IN(index, 4, n),
                       ARG_OUT(sk32, 32, n),               ARG_OUT(cc32, 32, n),               ARG_OUT(err, 1, n)};
    if (missing(args) || bip32_bad_parents(n_parents, n)) return P2E_E_INVALID;
    const Aff* table = nullptr;
    if (int rc = schnorr_prepare(c, n, &table, args)) return rc;   // (the generator's table of secp256k1, lane plan)
    if (n == 0) return 0;
    Staged S(c);
    if (long rc = S.begin(args)) return rc;
    launch_bip32_ckd_priv(c, table, par_sk32, par_cc32, n_parents != n, index, sk32, cc32, n, err);
    return S.end();
}
extern "C" long p2e_bip32_ckd_pub_batch(p2e_ctx* c, const uint8_t* par_pkx32, const uint8_t* par_pky32, const uint8_t* par_cc32,
                                        size_t n_parents, const uint32_t* index, uint8_t* pkx32, uint8_t* pky32, uint8_t* cc32, size_t n,
                                        uint8_t* err) {
    const Args args = {ARG_BCAST(par_pkx32, 32, n_parents), ARG_BCAST(par_pky32, 32, n_parents), ARG_BCAST(par_cc32, 32, n_parents),
                       ARG_IN(index, 4, n),                 ARG_OUT(pkx32, 32, n),               ARG_OUT(pky32, 32, n),
                       ARG_OUT(cc32, 32, n),                ARG_OUT(err, 1, n)};
    if (missing(args) || bip32_bad_parents(n_parents, n)) return P2E_E_INVALID;
    const Aff* table = nullptr;
    if (int rc = schnorr_prepare(c, n, &table, args)) return rc;
    if (n == 0) return 0;
    Staged S(c);
    if (long rc = S.begin(args)) return rc;
    launch_bip32_ckd_pub(c, table, par_pkx32, par_pky32, par_cc32, n_parents != n, index, pkx32, pky32, cc32, n, err);
    return S.end();
}
extern "C" long p2e_key_hash160_batch(p2e_ctx* c, unsigned form, const uint8_t* pkx32, const uint8_t* pky32, const uint8_t* err_in,
                                      uint8_t* out20, size_t n) {
    const Args args = {ARG_IN(pkx32, 32, n), ARG_IN(pky32, 32, n), ARG_IN_OPT(err_in, 1, n), ARG_OUT(out20, 20, n)};
    if (missing(args)) return P2E_E_INVALID;
    if (form != P2E_SEC1_COMPRESSED && form != P2E_SEC1_UNCOMPRESSED) {
        set_error("unknown form (P2E_SEC1_COMPRESSED or P2E_SEC1_UNCOMPRESSED)");
        return P2E_E_INVALID;
    }
    if (batch_too_large(n) || bad_overlap(n, args) || bad_ctx(c)) return P2E_E_INVALID;
    if (n == 0) return 0;
    Staged S(c);
    if (long rc = S.begin(args)) return rc;
    launch_key_hash160(c, form, pkx32, pky32, err_in, out20, n);
    return S.end();
}
extern "C" long p2e_hash160_batch(p2e_ctx* c, const uint8_t* data, const uint64_t* offsets, uint8_t* out20, size_t n) {
    const Args args = {ARG_OPAQUE(data), ARG_IN(offsets, 8, n + 1), ARG_OUT(out20, 20, n)};
    if (missing(args) || batch_too_large(n) || bad_overlap(n, args) || bad_ctx(c)) return P2E_E_INVALID;
    if (n == 0) return 0;
    Staged S(c);
    if (!wire_stage_elements(S, args, data, offsets, n)) return S.done(P2E_E_INVALID);
    if (long rc = S.begin(args)) return rc;
    launch_hash160(c, data, offsets, out20, n);
    return S.end();
}
#endif   // P2E_HAS(0)

// ====================================================================================================
// PBKDF2-HMAC-SHA512 and BIP-39 seeds (kdf.hpp): the step in front of the master key
// ====================================================================================================
// one launch on the caller's stream; defined in part 1 beside the other hashing kernels, called from part 0
void launch_pbkdf2_sha512(p2e_ctx* c, bool bip39, const uint8_t* password, const uint64_t* pw_offsets, bool pw_bcast, const uint8_t* salt,
                          const uint64_t* salt_offsets, bool salt_bcast, uint32_t iterations, size_t dk_len, uint8_t* dk, size_t count,
                          uint8_t* err);
#if P2E_HAS(1)
void launch_pbkdf2_sha512(p2e_ctx* c, bool bip39, const uint8_t* password, const uint64_t* pw_offsets, bool pw_bcast, const uint8_t* salt,
                          const uint64_t* salt_offsets, bool salt_bcast, uint32_t iterations, size_t dk_len, uint8_t* dk, size_t count,
                          uint8_t* err) {
    if (bip39)
        hipLaunchKernelGGL((k_pbkdf2_sha512<8>), grid1(count), dim3(BS), 0, c->stream, password, pw_offsets, pw_bcast ? 1 : 0, salt, salt_offsets,
                           salt_bcast ? 1 : 0, iterations, (u32)(dk_len / 4), dk, count, err, c->d_counter);
    else
        hipLaunchKernelGGL((k_pbkdf2_sha512<0>), grid1(count), dim3(BS), 0, c->stream, password, pw_offsets, pw_bcast ? 1 : 0, salt, salt_offsets,
                           salt_bcast ? 1 : 0, iterations, (u32)(dk_len / 4), dk, count, err, c->d_counter);
}
#endif   // P2E_HAS(1)

#if P2E_HAS(0)
static_assert(P2E_PBKDF2_MAX_ITERATIONS == PBKDF2_MAX_ITERATIONS, "include/p2e.h and kdf.hpp must agree");
// an operand of n_x elements serves `count` lanes: one each, or one for all (`or_none`: or none at all)
static bool kdf_bad_elements(const char* what, size_t n_x, size_t count, bool or_none = false) {
    if (n_x == 1 || n_x == count || (or_none && n_x == 0)) return false;
    set_error(std::string(what) + (or_none ? " must be 0, 1 or count" : " must be 1 or count"));
    return true;
}
// the entries of an operand's offsets; 0 for counts that are refused anyway (so that the sum cannot wrap)
static size_t kdf_offsets(size_t n_x, size_t count) { return (n_x == 1 || n_x == count) && n_x <= ((size_t)1 << 31) ? n_x + 1 : 0; }
// both calls behind their argument checks.  The offsets are read by lanes that own no element of them (lane i reads entry
// i + 1, every lane reads a broadcast operand's two): never in place.  (the batch size is `count`: see include/p2e.h)
static long kdf_run(p2e_ctx* c, bool bip39, Args args, const char* pw_name, const uint8_t* password, const uint64_t* pw_offsets, size_t n_passwords,
                    const char* salt_name, const uint8_t* salt, const uint64_t* salt_offsets, size_t n_salts, uint32_t iterations, size_t dk_len,
                    uint8_t* dk, size_t count, uint8_t* err) {
    if (batch_too_large(count) || bad_overlap(count, args) || bad_ctx(c)) return P2E_E_INVALID;
    if (count == 0) return 0;
    Staged S(c);
    if (!wire_stage_elements(S, args, password, pw_offsets, n_passwords, pw_name)) return S.done(P2E_E_INVALID);
    if (salt_offsets && !wire_stage_elements(S, args, salt, salt_offsets, n_salts, salt_name)) return S.done(P2E_E_INVALID);
    // (the list's slots are the caller's variables: stage the offsets and outputs through copies of the same names)
    const Args staged = {ARG_SHARED(pw_offsets, 8, n_passwords + 1), ARG_IN_IF(salt_offsets != nullptr, salt_offsets, 8, n_salts + 1),
                         ARG_OUT(dk, dk_len, count), ARG_OUT(err, 1, count)};
    if (long rc = S.begin(staged)) return rc;
    launch_pbkdf2_sha512(c, bip39, password, pw_offsets, n_passwords != count, salt, salt_offsets, n_salts != count, iterations, dk_len, dk, count,
                         err);
    return S.end();
}
extern "C" long p2e_pbkdf2_hmac_sha512_batch(p2e_ctx* c, const uint8_t* password, const uint64_t* pw_offsets, size_t n_passwords,
                                             const uint8_t* salt, const uint64_t* salt_offsets, size_t n_salts, uint32_t iterations, size_t dk_len,
                                             uint8_t* dk, size_t count, uint8_t* err) {
    const bool dk_ok = dk_len >= 4 && dk_len <= 64 && dk_len % 4 == 0;
    const Args args = {ARG_OPAQUE(password), ARG_SHARED(pw_offsets, 8, kdf_offsets(n_passwords, count)),
                       ARG_OPAQUE(salt),     ARG_SHARED(salt_offsets, 8, kdf_offsets(n_salts, count)),
                       ARG_OUT(dk, dk_ok ? dk_len : 0, count), ARG_OUT(err, 1, count)};
    if (missing(args) || kdf_bad_elements("n_passwords", n_passwords, count) || kdf_bad_elements("n_salts", n_salts, count)) return P2E_E_INVALID;
    if (iterations == 0 || iterations > P2E_PBKDF2_MAX_ITERATIONS) {
        set_error("iterations must be 1 .. P2E_PBKDF2_MAX_ITERATIONS (2^20)");
        return P2E_E_INVALID;
    }
    if (!dk_ok) {
        set_error("dk_len must be a multiple of 4 in 4 .. 64");
        return P2E_E_INVALID;
    }
    return kdf_run(c, false, args, "password", password, pw_offsets, n_passwords, "salt", salt, salt_offsets, n_salts, iterations, dk_len, dk, count,
                   err);
}
extern "C" long p2e_bip39_seed_batch(p2e_ctx* c, const uint8_t* mnemonic, const uint64_t* mn_offsets, size_t n_mnemonics,
                                     const uint8_t* passphrase, const uint64_t* pp_offsets, size_t n_passphrases, uint8_t* seed64, size_t count,
                                     uint8_t* err) {
    const bool with_pp = n_passphrases != 0;
    const Args args = {ARG_OPAQUE(mnemonic),
                       ARG_SHARED(mn_offsets, 8, kdf_offsets(n_mnemonics, count)),
                       P2E_ARG(passphrase, 0, 0, Opaque, with_pp),
                       P2E_ARG(pp_offsets, 8, with_pp ? kdf_offsets(n_passphrases, count) : 0, Shared, with_pp),
                       ARG_OUT(seed64, 64, count),
                       ARG_OUT(err, 1, count)};
    if (missing(args, with_pp ? nullptr : "n_passphrases == 0") || kdf_bad_elements("n_mnemonics", n_mnemonics, count) ||
        kdf_bad_elements("n_passphrases", n_passphrases, count, true))
        return P2E_E_INVALID;
    if (!with_pp && (passphrase || pp_offsets) && count != 0) {
        set_error("n_passphrases == 0 goes with a null passphrase and null pp_offsets");
        return P2E_E_INVALID;
    }
    return kdf_run(c, true, args, "mnemonic", mnemonic, mn_offsets, n_mnemonics, "passphrase", with_pp ? passphrase : nullptr,
                   with_pp ? pp_offsets : nullptr, n_passphrases, BIP39_ITERATIONS, 64, seed64, count, err);
}
#endif   // P2E_HAS(0)

// ====================================================================================================
// Taproot on secp256k1 (taproot.hpp): leaf hashes, Merkle roots, key tweaks, the script-path commitment check
// ====================================================================================================
// one launch each on the caller's stream; defined in part 3 beside the BIP-340 kernels, called from part 0
void launch_taproot_leaf_hash(p2e_ctx* c, const uint8_t* version, const uint8_t* script, const uint64_t* offsets, uint8_t* leaf, size_t count,
                              uint8_t* err);
void launch_taproot_merkle_root(p2e_ctx* c, const uint8_t* leaf, const uint8_t* path, const uint8_t* depth, size_t max_depth, uint8_t* root,
                                size_t count, uint8_t* err);
void launch_taproot_tweak_pubkey(p2e_ctx* c, const Aff* table, const uint8_t* pk, const uint8_t* root, uint8_t* out_pk, uint8_t* out_parity,
                                 size_t count, uint8_t* err);
void launch_taproot_tweak_seckey(p2e_ctx* c, const Aff* table, const uint8_t* sk, const uint8_t* root, uint8_t* out_sk, size_t count,
                                 uint8_t* err);
void launch_taproot_verify_commitment(p2e_ctx* c, const Aff* table, const uint8_t* out_pk, const uint8_t* out_parity, const uint8_t* pk,
                                      const uint8_t* leaf, const uint8_t* path, const uint8_t* depth, size_t max_depth, size_t count,
                                      uint8_t* err, uint8_t* valid);
#if P2E_HAS(3)
void launch_taproot_leaf_hash(p2e_ctx* c, const uint8_t* version, const uint8_t* script, const uint64_t* offsets, uint8_t* leaf, size_t count,
                              uint8_t* err) {
    hipLaunchKernelGGL((k_taproot_leaf_hash<0>), grid1(count), dim3(BS), 0, c->stream, version, script, offsets, leaf, count, err,
                       c->d_counter);
}
void launch_taproot_merkle_root(p2e_ctx* c, const uint8_t* leaf, const uint8_t* path, const uint8_t* depth, size_t max_depth, uint8_t* root,
                                size_t count, uint8_t* err) {
    hipLaunchKernelGGL((k_taproot_merkle_root<0>), grid1(count), dim3(BS), 0, c->stream, leaf, path, depth, max_depth, root, count, err,
                       c->d_counter);
}
void launch_taproot_tweak_pubkey(p2e_ctx* c, const Aff* table, const uint8_t* pk, const uint8_t* root, uint8_t* out_pk, uint8_t* out_parity,
                                 size_t count, uint8_t* err) {
    hipLaunchKernelGGL((k_taproot_tweak_pubkey<0>), grid1(count), dim3(BS), 0, c->stream, table, pk, root, out_pk, out_parity, count, err,
                       c->d_counter);
}
void launch_taproot_tweak_seckey(p2e_ctx* c, const Aff* table, const uint8_t* sk, const uint8_t* root, uint8_t* out_sk, size_t count,
                                 uint8_t* err) {
    hipLaunchKernelGGL((k_taproot_tweak_seckey<0>), grid1(count), dim3(BS), 0, c->stream, table, sk, root, out_sk, count, err, c->d_counter);
}
void launch_taproot_verify_commitment(p2e_ctx* c, const Aff* table, const uint8_t* out_pk, const uint8_t* out_parity, const uint8_t* pk,
                                      const uint8_t* leaf, const uint8_t* path, const uint8_t* depth, size_t max_depth, size_t count,
                                      uint8_t* err, uint8_t* valid) {
    hipLaunchKernelGGL((k_taproot_verify_commitment<0>), grid1(count), dim3(BS), 0, c->stream, table, out_pk, out_parity, pk, leaf, path,
                       depth, max_depth, count, err, valid, c->d_counter);
}
#endif   // P2E_HAS(3)

#if P2E_HAS(0)
static bool taproot_bad_depth(size_t max_depth) {
    if (max_depth <= TAPROOT_MAX_DEPTH) return false;
    set_error("max_depth must be at most 128");
    return true;
}
// the elements of path32; 0 for arguments that are refused anyway (so that the product cannot overflow)
static size_t taproot_nodes(size_t count, size_t max_depth) {
    return (max_depth <= TAPROOT_MAX_DEPTH && count <= ((size_t)1 << 31)) ? count * max_depth : 0;
}
// (the batch size of these five calls is `count`: see include/p2e.h)
extern "C" long p2e_taproot_leaf_hash_batch(p2e_ctx* c, const uint8_t* leaf_version, const uint8_t* script, const uint64_t* offsets,
                                            uint8_t* leaf32, size_t count, uint8_t* err) {
    const Args args = {ARG_IN(leaf_version, 1, count), ARG_OPAQUE(script), ARG_IN(offsets, 8, count + 1), ARG_OUT(leaf32, 32, count),
                       ARG_OUT(err, 1, count)};
    if (missing(args) || batch_too_large(count) || bad_overlap(count, args) || bad_ctx(c)) return P2E_E_INVALID;
    if (count == 0) return 0;
    Staged S(c);
    if (!wire_stage_elements(S, args, script, offsets, count)) return S.done(P2E_E_INVALID);
    if (long rc = S.begin(args)) return rc;
    launch_taproot_leaf_hash(c, leaf_version, script, offsets, leaf32, count, err);
    return S.end();
}
extern "C" long p2e_taproot_merkle_root_batch(p2e_ctx* c, const uint8_t* leaf32, const uint8_t* path32, const uint8_t* depth, size_t max_depth,
                                              uint8_t* root32, size_t count, uint8_t* err) {
    const size_t nodes = taproot_nodes(count, max_depth);
    const Args args = {ARG_IN(leaf32, 32, count), ARG_IN_IF(max_depth != 0, path32, 32, nodes), ARG_IN(depth, 1, count),
                       ARG_OUT(root32, 32, count), ARG_OUT(err, 1, count)};
    if (missing(args) || taproot_bad_depth(max_depth) || batch_too_large(count) || bad_overlap(count, args) || bad_ctx(c)) return P2E_E_INVALID;
    if (count == 0) return 0;
    Staged S(c);
    if (long rc = S.begin(args)) return rc;
    launch_taproot_merkle_root(c, leaf32, path32, depth, max_depth, root32, count, err);
    return S.end();
}
extern "C" long p2e_taproot_tweak_pubkey_batch(p2e_ctx* c, const uint8_t* pk32, const uint8_t* root32, uint8_t* out_pk32, uint8_t* out_parity,
                                               size_t count, uint8_t* err) {
    const Args args = {ARG_IN(pk32, 32, count), ARG_IN_OPT(root32, 32, count), ARG_OUT(out_pk32, 32, count), ARG_OUT(out_parity, 1, count),
                       ARG_OUT(err, 1, count)};
    if (missing(args)) return P2E_E_INVALID;
    const Aff* table = nullptr;
    if (int rc = schnorr_prepare(c, count, &table, args)) return rc;
    if (count == 0) return 0;
    Staged S(c);
    if (long rc = S.begin(args)) return rc;
    launch_taproot_tweak_pubkey(c, table, pk32, root32, out_pk32, out_parity, count, err);
    return S.end();
}
extern "C" long p2e_taproot_tweak_seckey_batch(p2e_ctx* c, const uint8_t* sk32, const uint8_t* root32, uint8_t* out_sk32, size_t count,
                                               uint8_t* err) {
    const Args args = {ARG_IN(sk32, 32, count), ARG_IN_OPT(root32, 32, count), ARG_OUT(out_sk32, 32, count), ARG_OUT(err, 1, count)};
    if (missing(args)) return P2E_E_INVALID;
    const Aff* table = nullptr;
    if (int rc = schnorr_prepare(c, count, &table, args)) return rc;
    if (count == 0) return 0;
    Staged S(c);
    if (long rc = S.begin(args)) return rc;
    launch_taproot_tweak_seckey(c, table, sk32, root32, out_sk32, count, err);
    return S.end();
}
extern "C" long p2e_taproot_verify_commitment_batch(p2e_ctx* c, const uint8_t* out_pk32, const uint8_t* out_parity, const uint8_t* pk32,
                                                    const uint8_t* leaf32, const uint8_t* path32, const uint8_t* depth, size_t max_depth,
                                                    size_t count, uint8_t* err, uint8_t* valid) {
    const size_t nodes = taproot_nodes(count, max_depth);
    const Args args = {ARG_IN(out_pk32, 32, count), ARG_IN(out_parity, 1, count), ARG_IN(pk32, 32, count), ARG_IN(leaf32, 32, count),
                       ARG_IN_IF(max_depth != 0, path32, 32, nodes), ARG_IN(depth, 1, count), ARG_OUT(err, 1, count),
                       ARG_OUT(valid, 1, count)};
    if (missing(args) || taproot_bad_depth(max_depth)) return P2E_E_INVALID;
    const Aff* table = nullptr;
    if (int rc = schnorr_prepare(c, count, &table, args)) return rc;
    if (count == 0) return 0;
    Staged S(c);
    if (long rc = S.begin(args)) return rc;
    launch_taproot_verify_commitment(c, table, out_pk32, out_parity, pk32, leaf32, path32, depth, max_depth, count, err, valid);
    return S.end();
}
#endif   // P2E_HAS(0)

// ====================================================================================================
// Silent payments (BIP-352) on secp256k1 (sp.hpp): input hashes, labels, the sender's output keys, the receiver's scan
// ====================================================================================================
// one launch each on the caller's stream; defined in part 1 beside the point multiplication, called from part 0
void launch_sp_input_hash(p2e_ctx* c, const uint8_t* outpoint, const uint8_t* ax, const uint8_t* ay, uint8_t* input_hash, size_t count,
                          uint8_t* err);
void launch_sp_label(p2e_ctx* c, const Aff* table, const uint8_t* scan_sk, const uint32_t* label_index, uint8_t* label_tweak, uint8_t* label_x,
                     uint8_t* label_y, size_t count, uint8_t* err);
void launch_sp_send(p2e_ctx* c, const Aff* table, const uint8_t* a_sk, const uint8_t* input_hash, const uint8_t* scan_pkx, const uint8_t* scan_pky,
                    const uint8_t* spend_pkx, const uint8_t* spend_pky, const uint32_t* k, uint8_t* out_pk, size_t count, uint8_t* err);
void launch_sp_scan(p2e_ctx* c, const Aff* table, const uint8_t* scan_sk, const uint8_t* spend_pkx, const uint8_t* spend_pky,
                    const uint8_t* label_x, const uint8_t* label_y, size_t n_labels, const uint8_t* ax, const uint8_t* ay,
                    const uint8_t* input_hash, const uint8_t* outputs, const uint64_t* out_offsets, size_t max_hits, uint8_t* n_hits,
                    uint32_t* hit_output, uint8_t* hit_label, uint8_t* hit_tweak, size_t count, uint8_t* err);
#if P2E_HAS(1)
void launch_sp_input_hash(p2e_ctx* c, const uint8_t* outpoint, const uint8_t* ax, const uint8_t* ay, uint8_t* input_hash, size_t count,
                          uint8_t* err) {
    hipLaunchKernelGGL((k_sp_input_hash<0>), grid1(count), dim3(BS), 0, c->stream, outpoint, ax, ay, input_hash, count, err, c->d_counter);
}
void launch_sp_label(p2e_ctx* c, const Aff* table, const uint8_t* scan_sk, const uint32_t* label_index, uint8_t* label_tweak, uint8_t* label_x,
                     uint8_t* label_y, size_t count, uint8_t* err) {
    hipLaunchKernelGGL((k_sp_label<0>), grid1(count), dim3(BS), 0, c->stream, table, scan_sk, label_index, label_tweak, label_x, label_y, count,
                       err, c->d_counter);
}
void launch_sp_send(p2e_ctx* c, const Aff* table, const uint8_t* a_sk, const uint8_t* input_hash, const uint8_t* scan_pkx, const uint8_t* scan_pky,
                    const uint8_t* spend_pkx, const uint8_t* spend_pky, const uint32_t* k, uint8_t* out_pk, size_t count, uint8_t* err) {
    hipLaunchKernelGGL((k_sp_send<0>), grid1(count), dim3(BS), 0, c->stream, table, a_sk, input_hash, scan_pkx, scan_pky, spend_pkx, spend_pky, k,
                       out_pk, count, err, c->d_counter);
}
void launch_sp_scan(p2e_ctx* c, const Aff* table, const uint8_t* scan_sk, const uint8_t* spend_pkx, const uint8_t* spend_pky,
                    const uint8_t* label_x, const uint8_t* label_y, size_t n_labels, const uint8_t* ax, const uint8_t* ay,
                    const uint8_t* input_hash, const uint8_t* outputs, const uint64_t* out_offsets, size_t max_hits, uint8_t* n_hits,
                    uint32_t* hit_output, uint8_t* hit_label, uint8_t* hit_tweak, size_t count, uint8_t* err) {
    hipLaunchKernelGGL((k_sp_scan<0>), grid1(count), dim3(BS), 0, c->stream, table, scan_sk, spend_pkx, spend_pky, label_x, label_y,
                       (u32)n_labels, ax, ay, input_hash, outputs, out_offsets, (u32)max_hits, n_hits, hit_output, hit_label, hit_tweak, count,
                       err, c->d_counter);
}
#endif   // P2E_HAS(1)

#if P2E_HAS(0)
static bool sp_bad_limits(size_t max_hits, size_t n_labels) {
    if (max_hits >= 1 && max_hits <= SP_MAX_HITS && n_labels <= SP_MAX_LABELS) return false;
    set_error("max_hits must be 1 .. 8 (P2E_SP_MAX_HITS) and n_labels at most 16 (P2E_SP_MAX_LABELS)");
    return true;
}
// the outputs of a staged scan: the copy holds outputs32[32 out_offsets[0], 32 out_offsets[count]) and `outputs32` becomes that
// copy moved back by 32 out_offsets[0] (wire_stage_elements, for 32-byte elements).  Every offset must lie inside that
// range: a lane reads its own [out_offsets[i], out_offsets[i + 1]) of the copy.  false: the error text is set.
static bool sp_stage_outputs(Staged& S, Args args, const uint8_t*& outputs32, const uint64_t* out_offsets, size_t count) {
    if (!S.host) return true;
    const uint64_t first = out_offsets[0], last = out_offsets[count];
    if (last < first || last > ((uint64_t)1 << 56)) {
        set_error("out_offsets[count] < out_offsets[0], or beyond 2^56 outputs");
        return false;
    }
    for (size_t i = 0; i <= count; i++)
        if (out_offsets[i] < first || out_offsets[i] > last) {
            set_error("an element of out_offsets lies outside [out_offsets[0], out_offsets[count]]");
            return false;
        }
    overlap::Span spans[call_args::kMaxBufs + 1];
    size_t num = 0;
    for (size_t i = 0, all = call_args::spans(args, count, spans); i < all; i++)
        if (spans[i].is_output) spans[num++] = spans[i];
    spans[num++] = overlap::Span{"outputs32", outputs32 + 32 * first, 32, (size_t)(last - first), false, true};   // (no lane owns a byte of it)
    if (const overlap::Clash k = overlap::check(spans, num); k.bad) {
        set_error(std::string("overlap: ") + k.a + " and " + k.b + " share bytes (variable-length data may not touch an output)");
        return false;
    }
    const uint8_t* d = S.in(outputs32 + 32 * first, 32 * (size_t)(last - first));
    outputs32 = d ? d - 32 * first : nullptr;
    return true;
}
// (the batch size of these four calls is `count`: see include/p2e.h)
extern "C" long p2e_sp_input_hash_batch(p2e_ctx* c, const uint8_t* outpoint36, const uint8_t* ax32, const uint8_t* ay32, uint8_t* input_hash32,
                                        size_t count, uint8_t* err) {
    const Args args = {ARG_IN(outpoint36, 36, count), ARG_IN(ax32, 32, count), ARG_IN(ay32, 32, count), ARG_OUT(input_hash32, 32, count),
                       ARG_OUT(err, 1, count)};
    if (missing(args) || batch_too_large(count) || bad_overlap(count, args) || bad_ctx(c)) return P2E_E_INVALID;
    if (count == 0) return 0;
    Staged S(c);
    if (long rc = S.begin(args)) return rc;
    launch_sp_input_hash(c, outpoint36, ax32, ay32, input_hash32, count, err);
    return S.end();
}
extern "C" long p2e_sp_label_batch(p2e_ctx* c, const uint8_t* scan_sk32, const uint32_t* label_index, uint8_t* label_tweak32, uint8_t* label_x32,
                                   uint8_t* label_y32, size_t count, uint8_t* err) {
    const Args args = {ARG_SHARED(scan_sk32, 32, 1), ARG_IN(label_index, 4, count), ARG_OUT(label_tweak32, 32, count),
                       ARG_OUT(label_x32, 32, count), ARG_OUT(label_y32, 32, count), ARG_OUT(err, 1, count)};
    if (missing(args)) return P2E_E_INVALID;
    const Aff* table = nullptr;
    if (int rc = schnorr_prepare(c, count, &table, args)) return rc;
    if (count == 0) return 0;
    Staged S(c);
    if (long rc = S.begin(args)) return rc;
    launch_sp_label(c, table, scan_sk32, label_index, label_tweak32, label_x32, label_y32, count, err);
    return S.end();
}
extern "C" long p2e_sp_send_batch(p2e_ctx* c, const uint8_t* a_sk32, const uint8_t* input_hash32, const uint8_t* scan_pkx32,
                                  const uint8_t* scan_pky32, const uint8_t* spend_pkx32, const uint8_t* spend_pky32, const uint32_t* k,
                                  uint8_t* out_pk32, size_t count, uint8_t* err) {
    const Args args = {ARG_IN(a_sk32, 32, count),       ARG_IN(input_hash32, 32, count), ARG_IN(scan_pkx32, 32, count),
                       ARG_IN(scan_pky32, 32, count),   ARG_IN(spend_pkx32, 32, count),  ARG_IN(spend_pky32, 32, count),
                       ARG_IN(k, 4, count),             ARG_OUT(out_pk32, 32, count),    ARG_OUT(err, 1, count)};
    if (missing(args)) return P2E_E_INVALID;
    const Aff* table = nullptr;
    if (int rc = schnorr_prepare(c, count, &table, args)) return rc;
    if (count == 0) return 0;
    Staged S(c);
    if (long rc = S.begin(args)) return rc;
    launch_sp_send(c, table, a_sk32, input_hash32, scan_pkx32, scan_pky32, spend_pkx32, spend_pky32, k, out_pk32, count, err);
    return S.end();
}
extern "C" long p2e_sp_scan_batch(p2e_ctx* c, const uint8_t* scan_sk32, const uint8_t* spend_pkx32, const uint8_t* spend_pky32,
                                  const uint8_t* label_x32, const uint8_t* label_y32, size_t n_labels, const uint8_t* ax32, const uint8_t* ay32,
                                  const uint8_t* input_hash32, const uint8_t* outputs32, const uint64_t* out_offsets, size_t max_hits,
                                  uint8_t* n_hits, uint32_t* hit_output, uint8_t* hit_label, uint8_t* hit_tweak32, size_t count, uint8_t* err) {
    // the extents of refused arguments are 0, so that no product can overflow; nothing of the scan may be used in place
    const bool sane = max_hits >= 1 && max_hits <= SP_MAX_HITS && n_labels <= SP_MAX_LABELS && count <= ((size_t)1 << 31);
    const size_t slots = sane ? count * max_hits : 0, labels = sane ? n_labels : 0;
    const Args args = {ARG_SHARED(scan_sk32, 32, 1),
                       ARG_SHARED(spend_pkx32, 32, 1),
                       ARG_SHARED(spend_pky32, 32, 1),
                       P2E_ARG(label_x32, 32, labels, Shared, n_labels != 0),
                       P2E_ARG(label_y32, 32, labels, Shared, n_labels != 0),
                       ARG_SHARED(ax32, 32, count),
                       ARG_SHARED(ay32, 32, count),
                       P2E_ARG(input_hash32, 32, count, Shared, false),
                       ARG_OPAQUE(outputs32),
                       ARG_IN(out_offsets, 8, count + 1),
                       ARG_OUT(n_hits, 1, count),
                       ARG_OUT(hit_output, 4, slots),
                       ARG_OUT(hit_label, 1, slots),
                       ARG_OUT(hit_tweak32, 32, slots),
                       ARG_OUT(err, 1, count)};
    if (missing(args) || sp_bad_limits(max_hits, n_labels)) return P2E_E_INVALID;
    const Aff* table = nullptr;
    if (int rc = schnorr_prepare(c, count, &table, args)) return rc;
    if (count == 0) return 0;
    Staged S(c);
    if (!sp_stage_outputs(S, args, outputs32, out_offsets, count)) return S.done(P2E_E_INVALID);
    if (long rc = S.begin(args)) return rc;
    launch_sp_scan(c, table, scan_sk32, spend_pkx32, spend_pky32, n_labels ? label_x32 : nullptr, n_labels ? label_y32 : nullptr, n_labels, ax32,
                   ay32, input_hash32, outputs32, out_offsets, max_hits, n_hits, hit_output, hit_label, hit_tweak32, count, err);
    return S.end();
}
#endif   // P2E_HAS(0)

// ====================================================================================================
// a P + b Q per element (point_arith.hpp's joint walk) and DLEQ proofs (BIP-374) on secp256k1 (dleq.hpp)
// ====================================================================================================
// one launch each on the caller's stream; defined in part 1 beside the point multiplication, called from part 0.
// plan: MUL_PLAN_PLAIN or MUL_PLAN_GLV (secp256k1 only), already chosen
template <class CV>
void launch_point_lincomb2(p2e_ctx* c, int plan, const uint8_t* a, const uint8_t* b, const uint8_t* px, const uint8_t* py, const uint8_t* qx,
                           const uint8_t* qy, uint8_t* outx, uint8_t* outy, size_t count, uint8_t* err);
void launch_dleq_prove(p2e_ctx* c, const Aff* table, const uint8_t* a_sk, const uint8_t* bx, const uint8_t* by, const uint8_t* aux_rand,
                       const uint8_t* msg, uint8_t* proof, uint8_t* cx, uint8_t* cy, size_t count, uint8_t* err);
void launch_dleq_verify(p2e_ctx* c, const Aff* table, const uint8_t* ax, const uint8_t* ay, const uint8_t* bx, const uint8_t* by,
                        const uint8_t* cx, const uint8_t* cy, const uint8_t* proof, const uint8_t* msg, size_t count, uint8_t* err,
                        uint8_t* valid);
#if P2E_HAS(1)
template <class CV>
void launch_point_lincomb2(p2e_ctx* c, int plan, const uint8_t* a, const uint8_t* b, const uint8_t* px, const uint8_t* py, const uint8_t* qx,
                           const uint8_t* qy, uint8_t* outx, uint8_t* outy, size_t count, uint8_t* err) {
    if constexpr (CV::kAZero) {
        if (plan == MUL_PLAN_GLV) {
            hipLaunchKernelGGL((k_point_lincomb2<CV, MUL_PLAN_GLV>), grid1(count), dim3(BS), 0, c->stream, a, b, px, py, qx, qy, outx, outy,
                               count, err, c->d_counter);
            return;
        }
    }
    hipLaunchKernelGGL((k_point_lincomb2<CV, MUL_PLAN_PLAIN>), grid1(count), dim3(BS), 0, c->stream, a, b, px, py, qx, qy, outx, outy, count,
                       err, c->d_counter);
}
template void launch_point_lincomb2<Secp256k1>(p2e_ctx*, int, const uint8_t*, const uint8_t*, const uint8_t*, const uint8_t*, const uint8_t*,
                                               const uint8_t*, uint8_t*, uint8_t*, size_t, uint8_t*);
template void launch_point_lincomb2<P256>(p2e_ctx*, int, const uint8_t*, const uint8_t*, const uint8_t*, const uint8_t*, const uint8_t*,
                                          const uint8_t*, uint8_t*, uint8_t*, size_t, uint8_t*);
void launch_dleq_prove(p2e_ctx* c, const Aff* table, const uint8_t* a_sk, const uint8_t* bx, const uint8_t* by, const uint8_t* aux_rand,
                       const uint8_t* msg, uint8_t* proof, uint8_t* cx, uint8_t* cy, size_t count, uint8_t* err) {
    hipLaunchKernelGGL((k_dleq_prove<0>), grid1(count), dim3(BS), 0, c->stream, table, a_sk, bx, by, aux_rand, msg, proof, cx, cy, count, err,
                       c->d_counter);
}
void launch_dleq_verify(p2e_ctx* c, const Aff* table, const uint8_t* ax, const uint8_t* ay, const uint8_t* bx, const uint8_t* by,
                        const uint8_t* cx, const uint8_t* cy, const uint8_t* proof, const uint8_t* msg, size_t count, uint8_t* err,
                        uint8_t* valid) {
    hipLaunchKernelGGL((k_dleq_verify<0>), grid1(count), dim3(BS), 0, c->stream, table, ax, ay, bx, by, cx, cy, proof, msg, valid, count, err,
                       c->d_counter);
}
#endif   // P2E_HAS(1)

#if P2E_HAS(0)
// BUFFER OVERLAP passes every exact in-place pair of an output and a per-lane input; these calls list their forms (x on x, y on
// y), and an output exactly on any OTHER per-lane input is refused here, with the same text.  count == 0 checks nothing.
struct NamedPtr {
    const void* p;
    const char* name;
};
static bool unlisted_in_place(size_t count, const void* out, const char* out_name, std::initializer_list<NamedPtr> inputs) {
    if (count == 0 || !out) return false;
    for (const NamedPtr& in : inputs)
        if (in.p == out) {
            set_error(std::string("overlap: ") + in.name + " and " + out_name + " share bytes (not an in-place form of this call)");
            return true;
        }
    return false;
}
// (the batch size of these three calls is `count`: see include/p2e.h)
// b32 is Shared: of the scalars only a32 may carry the output (outx32 = a32, as p2e_point_mul_batch's outx32 = k32)
extern "C" long p2e_point_lincomb2_batch(p2e_ctx* c, int curve, unsigned plan, const uint8_t* a32, const uint8_t* b32, const uint8_t* px32,
                                         const uint8_t* py32, const uint8_t* qx32, const uint8_t* qy32, uint8_t* outx32, uint8_t* outy32,
                                         size_t count, uint8_t* err) {
    const Args args = {ARG_IN(a32, 32, count),  ARG_SHARED(b32, 32, count), ARG_IN(px32, 32, count),    ARG_IN(py32, 32, count),
                       ARG_IN(qx32, 32, count), ARG_IN(qy32, 32, count),    ARG_OUT(outx32, 32, count), ARG_OUT(outy32, 32, count),
                       ARG_OUT(err, 1, count)};
    if (missing(args)) return P2E_E_INVALID;
    int chosen = 0;
    if (int rc = point_mul_prepare(curve, plan, count, &chosen)) return rc;
    if (bad_overlap(count, args) || unlisted_in_place(count, outx32, "outx32", {{py32, "py32"}, {qy32, "qy32"}}) ||
        unlisted_in_place(count, outy32, "outy32", {{a32, "a32"}, {px32, "px32"}, {qx32, "qx32"}}) || bad_ctx(c))
        return P2E_E_INVALID;
    if (count == 0) return 0;
    Staged S(c);
    if (long rc = S.begin(args)) return rc;
    if (curve == P2E_CURVE_P256)
        launch_point_lincomb2<P256>(c, chosen, a32, b32, px32, py32, qx32, qy32, outx32, outy32, count, err);
    else
        launch_point_lincomb2<Secp256k1>(c, chosen, a32, b32, px32, py32, qx32, qy32, outx32, outy32, count, err);
    return S.end();
}
// the one in-place form: (cx32, cy32) = (bx32, by32); the secret, the randomness and the message are Shared (never in place)
extern "C" long p2e_dleq_prove_batch(p2e_ctx* c, const uint8_t* a_sk32, const uint8_t* bx32, const uint8_t* by32, const uint8_t* aux_rand32,
                                     const uint8_t* msg32, uint8_t* proof64, uint8_t* cx32, uint8_t* cy32, size_t count, uint8_t* err) {
    const bool want_c = cx32 != nullptr || cy32 != nullptr;
    const Args args = {ARG_SHARED(a_sk32, 32, count),
                       ARG_IN(bx32, 32, count),
                       ARG_IN(by32, 32, count),
                       ARG_SHARED(aux_rand32, 32, count),
                       P2E_ARG(msg32, 32, count, Shared, false),
                       ARG_OUT(proof64, 64, count),
                       ARG_OUT_IF(want_c, cx32, 32, count),
                       ARG_OUT_IF(want_c, cy32, 32, count),
                       ARG_OUT(err, 1, count)};
    if (missing(args, want_c ? "the share (cx32 and cy32 go together)" : nullptr)) return P2E_E_INVALID;
    if (unlisted_in_place(count, cx32, "cx32", {{by32, "by32"}}) || unlisted_in_place(count, cy32, "cy32", {{bx32, "bx32"}})) return P2E_E_INVALID;
    const Aff* table = nullptr;
    if (int rc = schnorr_prepare(c, count, &table, args)) return rc;
    if (count == 0) return 0;
    Staged S(c);
    if (long rc = S.begin(args)) return rc;
    launch_dleq_prove(c, table, a_sk32, bx32, by32, aux_rand32, msg32, proof64, cx32, cy32, count, err);
    return S.end();
}
// no in-place form: every input is Shared
extern "C" long p2e_dleq_verify_batch(p2e_ctx* c, const uint8_t* ax32, const uint8_t* ay32, const uint8_t* bx32, const uint8_t* by32,
                                      const uint8_t* cx32, const uint8_t* cy32, const uint8_t* proof64, const uint8_t* msg32, size_t count,
                                      uint8_t* err, uint8_t* valid) {
    const Args args = {ARG_SHARED(ax32, 32, count),
                       ARG_SHARED(ay32, 32, count),
                       ARG_SHARED(bx32, 32, count),
                       ARG_SHARED(by32, 32, count),
                       ARG_SHARED(cx32, 32, count),
                       ARG_SHARED(cy32, 32, count),
                       ARG_SHARED(proof64, 64, count),
                       P2E_ARG(msg32, 32, count, Shared, false),
                       ARG_OUT(err, 1, count),
                       ARG_OUT(valid, 1, count)};
    if (missing(args)) return P2E_E_INVALID;
    const Aff* table = nullptr;
    if (int rc = schnorr_prepare(c, count, &table, args)) return rc;
    if (count == 0) return 0;
    Staged S(c);
    if (long rc = S.begin(args)) return rc;
    launch_dleq_verify(c, table, ax32, ay32, bx32, by32, cx32, cy32, proof64, msg32, count, err, valid);
    return S.end();
}
#endif   // P2E_HAS(0)

// ====================================================================================================
// MuSig2 (BIP-327) on secp256k1 (musig.hpp): key aggregation, tweaks, nonce aggregation, session values, partial signatures,
// their verification and the final signature
// ====================================================================================================
// one launch each on the caller's stream; defined in part 1 beside the point multiplication, called from part 0
void launch_musig_key_agg(p2e_ctx* c, const uint8_t* pkx, const uint8_t* pky, const uint64_t* key_offsets, uint8_t* keyagg, uint8_t* agg_pk,
                          size_t count, uint8_t* err);
void launch_musig_apply_tweak(p2e_ctx* c, const Aff* table, const uint8_t* keyagg_in, const uint8_t* tweak, int mode, uint8_t* keyagg_out,
                              uint8_t* agg_pk, size_t count, uint8_t* err);
void launch_musig_nonce_agg(p2e_ctx* c, const uint8_t* pubnonce, const uint64_t* key_offsets, uint8_t* aggnonce, size_t count, uint8_t* err);
void launch_musig_session(p2e_ctx* c, const Aff* table, const uint8_t* keyagg, const uint8_t* aggnonce, const uint8_t* msg, uint8_t* session,
                          size_t count, uint8_t* err);
void launch_musig_partial_sign(p2e_ctx* c, const Aff* table, const uint8_t* secnonce, const uint8_t* sk, const uint8_t* keyagg,
                               const uint8_t* session, uint8_t* psig, size_t count, uint8_t* err);
void launch_musig_partial_verify(p2e_ctx* c, const Aff* table, const uint8_t* psig, const uint8_t* pubnonce, const uint8_t* pkx,
                                 const uint8_t* pky, const uint32_t* session_index, const uint8_t* keyagg, const uint8_t* session,
                                 size_t n_sessions, size_t count, uint8_t* err, uint8_t* valid);
void launch_musig_sig_agg(p2e_ctx* c, const uint8_t* psig, const uint64_t* key_offsets, const uint8_t* keyagg, const uint8_t* session,
                          uint8_t* sig, size_t count, uint8_t* err);
#if P2E_HAS(1)
void launch_musig_key_agg(p2e_ctx* c, const uint8_t* pkx, const uint8_t* pky, const uint64_t* key_offsets, uint8_t* keyagg, uint8_t* agg_pk,
                          size_t count, uint8_t* err) {
    hipLaunchKernelGGL((k_musig_key_agg<0>), grid1(count), dim3(BS), 0, c->stream, pkx, pky, key_offsets, keyagg, agg_pk, count, err,
                       c->d_counter);
}
void launch_musig_apply_tweak(p2e_ctx* c, const Aff* table, const uint8_t* keyagg_in, const uint8_t* tweak, int mode, uint8_t* keyagg_out,
                              uint8_t* agg_pk, size_t count, uint8_t* err) {
    hipLaunchKernelGGL((k_musig_apply_tweak<0>), grid1(count), dim3(BS), 0, c->stream, table, keyagg_in, tweak, mode, keyagg_out, agg_pk, count,
                       err, c->d_counter);
}
void launch_musig_nonce_agg(p2e_ctx* c, const uint8_t* pubnonce, const uint64_t* key_offsets, uint8_t* aggnonce, size_t count, uint8_t* err) {
    hipLaunchKernelGGL((k_musig_nonce_agg<0>), grid1(count), dim3(BS), 0, c->stream, pubnonce, key_offsets, aggnonce, count, err, c->d_counter);
}
void launch_musig_session(p2e_ctx* c, const Aff* table, const uint8_t* keyagg, const uint8_t* aggnonce, const uint8_t* msg, uint8_t* session,
                          size_t count, uint8_t* err) {
    hipLaunchKernelGGL((k_musig_session<0>), grid1(count), dim3(BS), 0, c->stream, table, keyagg, aggnonce, msg, session, count, err,
                       c->d_counter);
}
void launch_musig_partial_sign(p2e_ctx* c, const Aff* table, const uint8_t* secnonce, const uint8_t* sk, const uint8_t* keyagg,
                               const uint8_t* session, uint8_t* psig, size_t count, uint8_t* err) {
    hipLaunchKernelGGL((k_musig_partial_sign<0>), grid1(count), dim3(BS), 0, c->stream, table, secnonce, sk, keyagg, session, psig, count, err,
                       c->d_counter);
}
void launch_musig_partial_verify(p2e_ctx* c, const Aff* table, const uint8_t* psig, const uint8_t* pubnonce, const uint8_t* pkx,
                                 const uint8_t* pky, const uint32_t* session_index, const uint8_t* keyagg, const uint8_t* session,
                                 size_t n_sessions, size_t count, uint8_t* err, uint8_t* valid) {
    hipLaunchKernelGGL((k_musig_partial_verify<0>), grid1(count), dim3(BS), 0, c->stream, table, psig, pubnonce, pkx, pky, session_index, keyagg,
                       session, n_sessions, count, err, valid, c->d_counter);
}
void launch_musig_sig_agg(p2e_ctx* c, const uint8_t* psig, const uint64_t* key_offsets, const uint8_t* keyagg, const uint8_t* session,
                          uint8_t* sig, size_t count, uint8_t* err) {
    hipLaunchKernelGGL((k_musig_sig_agg<0>), grid1(count), dim3(BS), 0, c->stream, psig, key_offsets, keyagg, session, sig, count, err,
                       c->d_counter);
}
#endif   // P2E_HAS(1)

#if P2E_HAS(0)
// One per-signer array of a staged call (`stride` bytes per signer): the copy holds signers [key_offsets[0], key_offsets[count])
// and `p` becomes that copy moved back by stride * key_offsets[0], as sp_stage_outputs does for the outputs of a scan.  The
// offsets are checked once per call (`check`), the array against the call's outputs every time.  false: the error text is set.
static bool musig_stage_signers(Staged& S, Args args, const char* name, const uint8_t*& p, size_t stride, const uint64_t* key_offsets,
                                size_t count, bool check) {
    if (!S.host) return true;
    const uint64_t first = key_offsets[0], last = key_offsets[count];
    if (check) {
        if (last < first || last > ((uint64_t)1 << 48)) {
            set_error("key_offsets[count] < key_offsets[0], or beyond 2^48 signers");
            return false;
        }
        for (size_t i = 0; i <= count; i++)
            if (key_offsets[i] < first || key_offsets[i] > last) {
                set_error("an element of key_offsets lies outside [key_offsets[0], key_offsets[count]]");
                return false;
            }
    }
    overlap::Span spans[call_args::kMaxBufs + 1];
    size_t num = 0;
    for (size_t i = 0, all = call_args::spans(args, count, spans); i < all; i++)
        if (spans[i].is_output) spans[num++] = spans[i];
    spans[num++] = overlap::Span{name, p + stride * first, stride, (size_t)(last - first), false, true};   // (no lane owns a byte of it)
    if (const overlap::Clash k = overlap::check(spans, num); k.bad) {
        set_error(std::string("overlap: ") + k.a + " and " + k.b + " share bytes (per-signer data may not touch an output)");
        return false;
    }
    const uint8_t* d = S.in(p + stride * first, stride * (size_t)(last - first));
    p = d ? d - stride * first : nullptr;
    return true;
}
// (the batch size of these seven calls is `count`: see include/p2e.h)
extern "C" long p2e_musig_key_agg_batch(p2e_ctx* c, const uint8_t* pkx32, const uint8_t* pky32, const uint64_t* key_offsets, uint8_t* keyagg192,
                                        uint8_t* agg_pk32, size_t count, uint8_t* err) {
    const Args args = {ARG_OPAQUE(pkx32), ARG_OPAQUE(pky32), ARG_SHARED(key_offsets, 8, count + 1), ARG_OUT(keyagg192, 192, count),
                       ARG_OUT(agg_pk32, 32, count), ARG_OUT(err, 1, count)};
    if (missing(args) || batch_too_large(count) || bad_overlap(count, args) || bad_ctx(c)) return P2E_E_INVALID;
    if (count == 0) return 0;
    Staged S(c);
    if (!musig_stage_signers(S, args, "pkx32", pkx32, 32, key_offsets, count, true) ||
        !musig_stage_signers(S, args, "pky32", pky32, 32, key_offsets, count, false))
        return S.done(P2E_E_INVALID);
    if (long rc = S.begin(args)) return rc;
    launch_musig_key_agg(c, pkx32, pky32, key_offsets, keyagg192, agg_pk32, count, err);
    return S.end();
}
extern "C" long p2e_musig_apply_tweak_batch(p2e_ctx* c, const uint8_t* keyagg192_in, const uint8_t* tweak32, int mode, uint8_t* keyagg192_out,
                                            uint8_t* agg_pk32, size_t count, uint8_t* err) {
    const Args args = {ARG_IN(keyagg192_in, 192, count), P2E_ARG(tweak32, 32, count, Shared, mode != P2E_MUSIG_TWEAK_TAPROOT),
                       ARG_OUT(keyagg192_out, 192, count), ARG_OUT(agg_pk32, 32, count), ARG_OUT(err, 1, count)};
    if (mode != P2E_MUSIG_TWEAK_PLAIN && mode != P2E_MUSIG_TWEAK_XONLY && mode != P2E_MUSIG_TWEAK_TAPROOT) {
        set_error("unknown mode (P2E_MUSIG_TWEAK_PLAIN, P2E_MUSIG_TWEAK_XONLY or P2E_MUSIG_TWEAK_TAPROOT)");
        return P2E_E_INVALID;
    }
    if (missing(args)) return P2E_E_INVALID;
    const Aff* table = nullptr;
    if (int rc = schnorr_prepare(c, count, &table, args)) return rc;
    if (count == 0) return 0;
    Staged S(c);
    if (long rc = S.begin(args)) return rc;
    launch_musig_apply_tweak(c, table, keyagg192_in, tweak32, mode, keyagg192_out, agg_pk32, count, err);
    return S.end();
}
extern "C" long p2e_musig_nonce_agg_batch(p2e_ctx* c, const uint8_t* pubnonce128, const uint64_t* key_offsets, uint8_t* aggnonce128,
                                          size_t count, uint8_t* err) {
    const Args args = {ARG_OPAQUE(pubnonce128), ARG_SHARED(key_offsets, 8, count + 1), ARG_OUT(aggnonce128, 128, count), ARG_OUT(err, 1, count)};
    if (missing(args) || batch_too_large(count) || bad_overlap(count, args) || bad_ctx(c)) return P2E_E_INVALID;
    if (count == 0) return 0;
    Staged S(c);
    if (!musig_stage_signers(S, args, "pubnonce128", pubnonce128, 128, key_offsets, count, true)) return S.done(P2E_E_INVALID);
    if (long rc = S.begin(args)) return rc;
    launch_musig_nonce_agg(c, pubnonce128, key_offsets, aggnonce128, count, err);
    return S.end();
}
extern "C" long p2e_musig_session_batch(p2e_ctx* c, const uint8_t* keyagg192, const uint8_t* aggnonce128, const uint8_t* msg32,
                                        uint8_t* session128, size_t count, uint8_t* err) {
    const Args args = {ARG_SHARED(keyagg192, 192, count), ARG_SHARED(aggnonce128, 128, count), ARG_SHARED(msg32, 32, count),
                       ARG_OUT(session128, 128, count), ARG_OUT(err, 1, count)};
    if (missing(args)) return P2E_E_INVALID;
    const Aff* table = nullptr;
    if (int rc = schnorr_prepare(c, count, &table, args)) return rc;
    if (count == 0) return 0;
    Staged S(c);
    if (long rc = S.begin(args)) return rc;
    launch_musig_session(c, table, keyagg192, aggnonce128, msg32, session128, count, err);
    return S.end();
}
extern "C" long p2e_musig_partial_sign_batch(p2e_ctx* c, const uint8_t* secnonce64, const uint8_t* sk32, const uint8_t* keyagg192,
                                             const uint8_t* session128, uint8_t* psig32, size_t count, uint8_t* err) {
    const Args args = {ARG_SHARED(secnonce64, 64, count),   ARG_SHARED(sk32, 32, count), ARG_SHARED(keyagg192, 192, count),
                       ARG_SHARED(session128, 128, count), ARG_OUT(psig32, 32, count),  ARG_OUT(err, 1, count)};
    if (missing(args)) return P2E_E_INVALID;
    const Aff* table = nullptr;
    if (int rc = schnorr_prepare(c, count, &table, args)) return rc;
    if (count == 0) return 0;
    Staged S(c);
    if (long rc = S.begin(args)) return rc;
    launch_musig_partial_sign(c, table, secnonce64, sk32, keyagg192, session128, psig32, count, err);
    return S.end();
}
extern "C" long p2e_musig_partial_verify_batch(p2e_ctx* c, const uint8_t* psig32, const uint8_t* pubnonce128, const uint8_t* pkx32,
                                               const uint8_t* pky32, const uint32_t* session_index, const uint8_t* keyagg192,
                                               const uint8_t* session128, size_t n_sessions, size_t count, uint8_t* err, uint8_t* valid) {
    // (a refused n_sessions has the extent 0, so that no product can overflow)
    const size_t sessions = n_sessions <= ((size_t)1 << 32) ? n_sessions : 0;
    const Args args = {ARG_SHARED(psig32, 32, count),
                       ARG_SHARED(pubnonce128, 128, count),
                       ARG_SHARED(pkx32, 32, count),
                       ARG_SHARED(pky32, 32, count),
                       P2E_ARG(session_index, 4, count, Shared, false),
                       ARG_SHARED(keyagg192, 192, sessions),
                       ARG_SHARED(session128, 128, sessions),
                       ARG_OUT(err, 1, count),
                       ARG_OUT(valid, 1, count)};
    if (missing(args)) return P2E_E_INVALID;
    if (n_sessions == 0 || n_sessions > ((size_t)1 << 32)) {
        set_error("n_sessions must be 1 .. 2^32");
        return P2E_E_INVALID;
    }
    const Aff* table = nullptr;
    if (int rc = schnorr_prepare(c, count, &table, args)) return rc;
    if (count == 0) return 0;
    Staged S(c);
    if (long rc = S.begin(args)) return rc;
    launch_musig_partial_verify(c, table, psig32, pubnonce128, pkx32, pky32, session_index, keyagg192, session128, n_sessions, count, err,
                                valid);
    return S.end();
}
extern "C" long p2e_musig_sig_agg_batch(p2e_ctx* c, const uint8_t* psig32, const uint64_t* key_offsets, const uint8_t* keyagg192,
                                        const uint8_t* session128, uint8_t* sig64, size_t count, uint8_t* err) {
    const Args args = {ARG_OPAQUE(psig32),          ARG_SHARED(key_offsets, 8, count + 1), ARG_SHARED(keyagg192, 192, count), ARG_SHARED(session128, 128, count),
                       ARG_OUT(sig64, 64, count), ARG_OUT(err, 1, count)};
    if (missing(args) || batch_too_large(count) || bad_overlap(count, args) || bad_ctx(c)) return P2E_E_INVALID;
    if (count == 0) return 0;
    Staged S(c);
    if (!musig_stage_signers(S, args, "psig32", psig32, 32, key_offsets, count, true)) return S.done(P2E_E_INVALID);
    if (long rc = S.begin(args)) return rc;
    launch_musig_sig_agg(c, psig32, key_offsets, keyagg192, session128, sig64, count, err);
    return S.end();
}
#endif   // P2E_HAS(0)

#include "curve_api.inc"
