/* p2e -- MI355X-native batch witness generation for plonky2's secp256k1 ECDSA gadget.
 *
 * C ABI of libp2e_hip.so.  These entry points are what a plonky2-ecdsa (Rust) build would bind through
 * `extern "C"` to replace the bodies of its witness generators (see INTEGRATION.md for the stub).
 * Each entry point cites the reference interface it replaces; paths are relative to the reference
 * crate's src/ (Weobe/plonky2-ecdsa).
 *
 * DATA LAYOUT
 *   Goldilocks columns: canonical u64 values (< 2^64 - 2^32 + 1), column-major over the batch:
 *   element i of column c lives at base[c * ld + i] with ld >= n ("SoA": the 64 lanes of a wavefront
 *   are 64 consecutive batch elements, every access is one coalesced 512-byte transaction).
 *   A non-native value is 9 consecutive columns of 29-bit limbs, least significant first
 *   (gadgets/nonnative.rs:32 BITS = 29, gates/mul_nonnative.rs:37-39 num_limbs = 9).
 *   256-bit inputs of the fused entry points are packed 32-byte little-endian, element i at +32*i.
 *
 * MEMORY
 *   All data pointers are DEVICE pointers (hipMalloc / torch tensors) unless the context was created
 *   with P2E_CTX_HOST_POINTERS, in which case they are host pointers and the library stages them
 *   through its own device buffers (PCIe-inclusive; never the benchmarked configuration).
 *   The caller owns every buffer; the library owns only the p2e_ctx (stream, scratch, constant tables).
 *
 * BUFFER OVERLAP
 *   What a call may be handed when an output buffer shares bytes with another argument.  The rule below holds for the
 *   PER-ELEMENT calls: every entry point from p2e_ecdsa_public_key_batch to p2e_musig_sig_agg_batch (keys, signing,
 *   recovery, hashing, wire forms, point arithmetic, point tables, the many-point sum, Schnorr, BIP-32, PBKDF2 / BIP-39, Taproot, silent payments, a P + b Q and DLEQ proofs, MuSig2) and the two verdict-only
 *   verifiers p2e_ecdsa_verify_batch and p2e_p256_verify_batch.  It is checked on the host, behind the call's other argument
 *   checks and before the context is looked at, and it is the same with P2E_CTX_HOST_POINTERS (staging would hide the race;
 *   the contract does not depend on the mode).
 *   1. The outputs of one call are pairwise disjoint.
 *   2. An output may coincide with an input only EXACTLY IN PLACE: same base pointer, same bytes per element, one element per
 *      index (a 32-byte array on a 32-byte array, v / err bytes on bytes).  Lane i then only overwrites what lane i has
 *      already read: the kernels of these calls read every input of element i before their first store to element i.
 *      The forms that are tested on every plan, byte for byte:
 *        p2e_ecdsa_public_key_batch            pkx32 = sk32
 *        p2e_ecdsa_sign_batch, _sign_recoverable_batch          r32 = msg32, s32 = k32
 *        p2e_ecdsa_sign_deterministic_batch    r32 = msg32
 *        p2e_ecdsa_nonce_rfc6979_batch         k32 = msg32
 *        p2e_ecdsa_recover_batch               pkx32 = r32, pky32 = s32
 *        p2e_point_mul_batch, p2e_point_lincomb_batch, p2e_point_add_batch   (outx32, outy32) = (px32, py32); mul also outx32 = k32
 *        p2e_point_table_mul_batch             outx32 = k32;   p2e_point_table_lincomb_batch   outx32 = a32 or b32
 *        p2e_schnorr_public_key_batch          pk32 = sk32;    p2e_xonly_decode_batch          px32 = pk32
 *        p2e_bip32_ckd_priv_batch, p2e_bip32_ckd_pub_batch with n_parents == n: the children over the parents (sk32 = par_sk32,
 *            pkx32 = par_pkx32, pky32 = par_pky32, cc32 = par_cc32) -- how a path is deepened level by level
 *        p2e_taproot_tweak_pubkey_batch        out_pk32 = pk32;   p2e_taproot_tweak_seckey_batch   out_sk32 = sk32
 *        p2e_taproot_merkle_root_batch         root32 = leaf32
 *        p2e_sp_input_hash_batch               input_hash32 = ax32;   p2e_sp_send_batch   out_pk32 = input_hash32
 *            (p2e_sp_scan_batch offers no in-place form: every overlap of one of its outputs is refused)
 *        p2e_point_lincomb2_batch              (outx32, outy32) = (px32, py32) or (qx32, qy32); outx32 = a32   (no output on b32)
 *        p2e_dleq_prove_batch                  (cx32, cy32) = (bx32, by32)   (no output on a_sk32, aux_rand32 or msg32;
 *            p2e_dleq_verify_batch offers no in-place form)
 *        p2e_musig_apply_tweak_batch           keyagg192_out = keyagg192_in   (the only in-place form of the seven MuSig2 calls)
 *   3. Any other intersection of an output with an input is P2E_E_INVALID, with "overlap" and the two argument names in
 *      p2e_last_error(): a shifted overlap (out == in + 32), different bytes per element (r32 on the 64-byte data of
 *      P2E_SIG_COMPACT64, addr20 on pkx32), and every input that lanes other than "its own" read -- the single parent of a
 *      BIP-32 call with n_parents == 1 < n (lane 0 would store child 0 over the parent the other lanes have yet to read),
 *      the terms of p2e_point_msm and p2e_schnorr_verify_aggregate against their one-element outputs (for n == 1 too), the
 *      points of p2e_point_table_create, the inputs of the two verdict-only verifiers.  Nothing is launched, nothing is
 *      staged, no byte is written, and the context stays usable.
 *   4. Adjacent ranges (the end of one is the start of the other) do not overlap.  n == 0 checks nothing and returns 0 as
 *      before.  A null nullable argument, and an argument the chosen form does not use, is skipped.  A range whose end
 *      wraps round the address space is refused.  Inputs may overlap each other freely.
 *   5. Variable-length `data` (p2e_hash_batch, p2e_hash160_batch, p2e_point_decode_batch, P2E_SIG_DER in p2e_sig_decode_batch,
 *      the passwords, salts, mnemonics and passphrases of p2e_pbkdf2_hmac_sha512_batch and p2e_bip39_seed_batch)
 *      has an extent only the device knows.  It must not overlap any output: the CALLER's duty.  It is checked only where the
 *      call reads offsets[0] and offsets[n] on the host anyway (P2E_CTX_HOST_POINTERS), with the same error.
 *   6. The column-matrix calls (single generators, fused fills, aux / gate-internal / constraint-block passes, wire assembly,
 *      the layout helpers, the curve programs' fills and passes) are different: their inputs and outputs must not overlap at
 *      all, and this is NOT checked.
 *   In the calls the rule covers, a null context is reported behind the argument and overlap checks.
 *
 * ERRORS
 *   Return value: < 0 API misuse / HIP failure (p2e_last_error() has the text); >= 0 number of batch
 *   elements whose err byte is non-zero.  err[i] is a bit mask of P2E_ERR_* -- the conditions under
 *   which the reference generator panics.  Outputs of a flagged element are unspecified.
 *   (The four wire-form calls, p2e_point_decode_batch .. p2e_sig_encode_batch, the three point-arithmetic calls,
 *   p2e_point_mul_batch .. p2e_point_add_batch, and the point-table calls, p2e_point_table_create ..
 *   p2e_ecdsa_verify_table_batch, write a P2E_WIRE_* CODE instead.)
 *   Nothing ever unwinds or aborts across this boundary.
 *
 * THREADING  A p2e_ctx is not thread-safe: one context per (host thread, device).  Calls are
 *   synchronous on return unless P2E_CTX_ASYNC is set (then p2e_sync() completes them and returns the
 *   flagged-element count of the last call).  Every entry point runs on the context's device and restores the
 *   calling thread's current device before it returns.  A failed call (negative return) has released everything it
 *   staged and left no work queued on the context's streams; the context stays usable.
 */
#ifndef P2E_H
#define P2E_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define P2E_FIELD_BASE 0   /* plonky2 Secp256K1Base   (point coordinates)      */
#define P2E_FIELD_SCALAR 1 /* plonky2 Secp256K1Scalar (msg, r, s, u1, u2, k1, k2) */
#define P2E_FIELD_P256_BASE 2   /* the crate's P256Base   (field/p256_base.rs)   -- single-generator entry points only */
#define P2E_FIELD_P256_SCALAR 3 /* the crate's P256Scalar (field/p256_scalar.rs) */

/* per-element error bits */
#define P2E_ERR_LIMB_RANGE 1       /* limb >= 2^29: gates/mul_nonnative.rs:262,271,275-276; biguint.rs:456,473 */
#define P2E_ERR_VALUE_GE_2_256 2   /* from_noncanonical_biguint panics (template field/p256_base.rs:121-130)  */
#define P2E_ERR_INVERSE_OF_ZERO 4  /* gadgets/nonnative.rs:863 inverse() of zero                               */
#define P2E_ERR_CARRY_RANGE 8      /* gates/mul_nonnative.rs:527 carry not < 2^34                              */
#define P2E_ERR_DIVISION_BY_ZERO 32 /* BigUintDivRemGenerator: b == 0 (BigUint::div_rem panics)                        */
#define P2E_ERR_QUOTIENT_RANGE 16  /* x*y/m does not fit the gate's nine q wires (x, y far above the modulus)  */
#define P2E_ERR_POINT_AT_INFINITY 64 /* p2e_ecdsa_public_key_batch: sk = 0 (mod n), AffinePoint::ZERO has no 64-byte form */
#define P2E_ERR_NOT_RECOVERABLE 128  /* p2e_ecdsa_recover_batch: (r, s, v) names no curve point R (the last free bit) */

/* status codes (negative returns) */
#define P2E_E_INVALID (-1)   /* null pointer, ld < n, bad field id ...      */
#define P2E_E_HIP (-2)       /* a HIP call failed                             */
#define P2E_E_NO_DEVICE (-3) /* no gfx950 device / extension not usable       */
#define P2E_E_NOMEM (-4)

/* context flags */
#define P2E_CTX_HOST_POINTERS 1u
#define P2E_CTX_ASYNC 2u
/* Time every launch of a fused call with HIP events (p2e_last_phase_ms).  Off by default: a timing event is a barrier
 * packet in front of and behind every expansion launch, which costs nothing measurable at 2^16 signatures per call but
 * 6 % at 2^13 (2.04 -> 1.92 ms).  The column-block events of p2e_segments_* exist either way (without timestamps). */
#define P2E_CTX_PHASE_TIMING 4u

#define P2E_VERIFY_COLS 82615  /* hot-path generator outputs of one verify_secp256k1_message_circuit */
#define P2E_GLV_MUL_COLS 65243 /* ... of one glv_mul                                                 */

typedef struct p2e_ctx p2e_ctx;

/* ---- context ------------------------------------------------------------------------------------ */
/* `stream`: a hipStream_t to run on (e.g. torch's current stream), or NULL for a library-owned one.  The
 * library-owned stream is a blocking stream (hipStreamDefault): work the caller queued on the legacy default
 * stream before a call is ordered before it, and default-stream work queued after a call is ordered after it.
 * The fused entry points dispatch on five internal streams (two chain streams, a second inversion stream, two
 * expansion streams) which the context creates -- and binds to their hardware queues with one empty launch each --
 * back to back, in a fixed order; `stream` itself carries only the scalar phase and the finalisation of a fused call and
 * is ordered with the internal streams by events, so the call behaves like any other work queued on `stream`.  Creating
 * a context synchronises the legacy default stream once.  Export GPU_MAX_HW_QUEUES=8 before the process's first HIP call
 * so that the internal streams do not share a hardware queue with the caller's. */
int p2e_ctx_create(int device, unsigned flags, void *stream, p2e_ctx **out);
void p2e_ctx_destroy(p2e_ctx *ctx);
int p2e_sync(p2e_ctx *ctx);
const char *p2e_last_error(void);
/* bytes of device scratch the fused entry points need for a batch of n (allocated lazily, kept) */
size_t p2e_scratch_bytes(int program /*0 verify, 1 glv_mul*/, size_t n);
/* Timing of the last fused call, measured with hipEvents on the context's stream around every launch -- for contexts
 * created with P2E_CTX_PHASE_TIMING; otherwise every duration is 0 and only the launch and column counts are filled in.
 * The schedule is cut into segments whose Jacobian chains run on internal streams underneath; each
 * finished segment is expanded by k_expand (one curve op per workgroup row: window table, fixed-base
 * chain, trailing adds) and/or k_expand_runs (runs of MSM-loop iterations).
 * out[0] = ms of the scalar kernel, out[4] = ms of the whole call;
 * out[1], out[2], out[3] = k_expand: launches, witness columns per signature they wrote, summed ms;
 * out[5], out[6], out[7] = the same three for k_expand_runs; out[8], out[9], out[10] = for k_expand_fb_run (the
 * fixed-base windows as one run per signature: curve programs, and the verifier under P2E_FB_RUN=1).  The curve
 * programs report their kc_* kernels in the same slots.  Returns the number written (<= 12). */
int p2e_last_phase_ms(p2e_ctx *ctx, float *out, int cap);

/* ---- column blocks of a fused call, as they become final (the assembly step) -------- */
/* The reference fills a PartialWitness generator by generator; a batch consumer -- the RCCL exchange that assembles the
 * columns of a sharded batch on every rank, a D2H copy, a prover that starts on finished columns -- need not wait for
 * the whole call either.  Every fused entry point (p2e_ecdsa_verify_witness[_compact]_batch, p2e_glv_mul_witness
 * [_compact]_batch, p2e_curve_mul_witness[_compact]_batch, p2e_p256_verify_witness[_compact]_batch) leaves behind the blocks of
 * columns [first_col, first_col + num_cols) its launches complete, each with a HIP event recorded behind the launch that
 * completes it.  A launch may complete several blocks, which then share one event: the columns of consecutive curve ops
 * are not always adjacent (the curve programs place a scalar generator between their last ops), and a block never spans
 * columns another launch writes.  Blocks are disjoint, cover all columns of the program, and are listed in the order the
 * launches were issued (the scalar phase first, then the expansion of every schedule piece as its chain and inversion
 * batch finish; the blocks of one launch by ascending column).  In
 * the compact container block k is rows [narrow_before(first_col), narrow_before(first_col + num_cols)) of the narrow
 * matrix and the same of the wide one (p2e_compact_layout is monotonic in the column index).
 * p2e_segments_describe: returns the number of blocks of the LAST fused call issued on ctx (valid from the moment that
 * call returns -- with P2E_CTX_ASYNC that is before anything has run -- until the next call on ctx).
 * p2e_segment_stream_wait: `stream` (a hipStream_t of the same device) waits until block k is final; nothing blocks on
 * the host.  p2e_segment_sync: the host blocks until block k is final.  Both return 0, or P2E_E_INVALID / P2E_E_HIP. */
typedef struct p2e_segment_desc {
    uint32_t first_col, num_cols;
} p2e_segment_desc;
long p2e_segments_describe(p2e_ctx *ctx, p2e_segment_desc *out, size_t cap);
int p2e_segment_stream_wait(p2e_ctx *ctx, int segment, void *stream);
int p2e_segment_sync(p2e_ctx *ctx, int segment);

/* ---- single generators (one reference run_once body each) ----------------------------------------- */
/* MulNonnativeGenerator::run_once gates/mul_nonnative.rs:249-324 followed by
 * CheckSumGenerator::run_once :513-531.  x, y: the gate's 9+9 input wires.  Outputs in gate wire
 * order (:41-59, :384-390): r[9], q[9], check_sum[17], then b[16] of the CheckSumGate row. */
long p2e_mul_witness_batch(p2e_ctx *ctx, int field, const uint64_t *x, const uint64_t *y, uint64_t *r,
                           uint64_t *q, uint64_t *check_sum, uint64_t *b, size_t n, size_t ld, uint8_t *err);
/* CheckSumGenerator::run_once alone on arbitrary a[17] (true Goldilocks division by 2^29). */
long p2e_checksum_witness_batch(p2e_ctx *ctx, const uint64_t *a, uint64_t *b, size_t n, size_t ld,
                                uint8_t *err);
/* NonNativeAdditionGenerator::run_once gadgets/nonnative.rs:626-645: sum[9], overflow. */
long p2e_add_witness_batch(p2e_ctx *ctx, int field, const uint64_t *a, const uint64_t *b, uint64_t *sum,
                           uint64_t *overflow, size_t n, size_t ld, uint8_t *err);
/* NonNativeSubtractionGenerator::run_once gadgets/nonnative.rs:792-810: diff[9], overflow. */
long p2e_sub_witness_batch(p2e_ctx *ctx, int field, const uint64_t *a, const uint64_t *b, uint64_t *diff,
                           uint64_t *overflow, size_t n, size_t ld, uint8_t *err);
/* NonNativeMultipleAddsGenerator::run_once gadgets/nonnative.rs:696-728: summands[k][9][ld], 1 <= k <= 8. */
long p2e_add_many_witness_batch(p2e_ctx *ctx, int field, const uint64_t *summands, int k, uint64_t *sum,
                                uint64_t *overflow, size_t n, size_t ld, uint8_t *err);
/* NonNativeInverseGenerator::run_once gadgets/nonnative.rs:857-872: inv[9], div[9]. */
long p2e_inv_witness_batch(p2e_ctx *ctx, int field, const uint64_t *x, uint64_t *inv, uint64_t *div, size_t n,
                           size_t ld, uint8_t *err);
/* BigUintDivRemGenerator::run_once gadgets/biguint.rs:508-518 (the generator behind rem_biguint / reduce,
 * gadgets/nonnative.rs:539-548; not on the ECDSA path, here so that every generator of the crate has an entry):
 * a[na][ld] (1 <= na <= 18 limbs), b[nb][ld] (1 <= nb <= 9) -> div[max(0, na - nb + 1)][ld], rem[nb][ld], the limb
 * counts div_rem_biguint allocates (:391-397).  err: a limb >= 2^29 (LIMB_RANGE; the reference would sum arbitrary
 * field elements), b == 0 (DIVISION_BY_ZERO), a quotient set_biguint_target rejects (LIMB_RANGE; this includes
 * the reference's convert_base quirk: a D-digit value is handed over as floor(32 D / 29) limbs, zero ones included). */
long p2e_biguint_div_rem_batch(p2e_ctx *ctx, const uint64_t *a, int na, const uint64_t *b, int nb, uint64_t *div,
                               uint64_t *rem, size_t n, size_t ld, uint8_t *err);
/* GLVDecompositionGenerator::run_once gadgets/glv.rs:128-142 (curve/glv.rs:39-77): k1[5], k2[5], signs. */
long p2e_glv_decompose_batch(p2e_ctx *ctx, const uint64_t *k, uint64_t *k1, uint64_t *k2, uint64_t *k1_neg,
                             uint64_t *k2_neg, size_t n, size_t ld, uint8_t *err);
/* set_biguint_target gadgets/biguint.rs:454-463 (convert_base :27-51): packed[n][32] -> limbs[9][ld]. */
long p2e_limb_split(p2e_ctx *ctx, const uint8_t *packed, uint64_t *limbs, size_t n, size_t ld);
/* get_biguint_target gadgets/biguint.rs:444-452: limbs[9][ld] -> packed[n][32]. */
long p2e_limb_pack(p2e_ctx *ctx, const uint64_t *limbs, uint8_t *packed, size_t n, size_t ld, uint8_t *err);

/* ---- fused schedules ------------------------------------------------------------------------------ */
/* Every hot-path generator output of verify_secp256k1_message_circuit (gadgets/ecdsa.rs:30-53) for n
 * signatures: cols[P2E_VERIFY_COLS][ld], generator registration order (p2e_schedule_describe).
 * valid[i] (nullable) = 1 iff the three connect constraints hold (curve_assert_valid, GLV
 * reconstruction, r == x), i.e. the signature verifies. */
long p2e_ecdsa_verify_witness_batch(p2e_ctx *ctx, const uint8_t *msg32, const uint8_t *r32, const uint8_t *s32,
                                    const uint8_t *pkx32, const uint8_t *pky32, uint64_t *cols, size_t n,
                                    size_t ld, uint8_t *err, uint8_t *valid);
/* The same circuit evaluated for its verdict only (a pre-filter for invalid signatures before
 * the witness is worth filling; curve/ecdsa.rs:42-62 verify_message on the GPU): valid[i] and err[i] exactly as
 * p2e_ecdsa_verify_witness_batch would set them, no columns written. */
long p2e_ecdsa_verify_batch(p2e_ctx *ctx, const uint8_t *msg32, const uint8_t *r32, const uint8_t *s32,
                            const uint8_t *pkx32, const uint8_t *pky32, size_t n, uint8_t *err, uint8_t *valid);
/* glv_mul(p, k) gadgets/glv.rs:87-104: cols[P2E_GLV_MUL_COLS][ld]. */
long p2e_glv_mul_witness_batch(p2e_ctx *ctx, const uint8_t *px32, const uint8_t *py32, const uint8_t *k32,
                               uint64_t *cols, size_t n, size_t ld, uint8_t *err, uint8_t *valid);

/* ---- built-in-generator columns ------------------------------------------- */
/* The values of the targets that plonky2's OWN generators fill between the hot-path generators of the same
 * circuit, derived on the GPU from the finished witness matrix `cols` (as written by
 * p2e_ecdsa_verify_witness_batch for program 0 / p2e_glv_mul_witness_batch for program 1), the constant tables
 * and the pk.y input, in the order the gadgets create the targets:
 *   split_nonnative_to_4_bit_limbs / _2_bit_limbs  gadgets/split_nonnative.rs:25-72  split_le_base bits of every
 *        limb, then (lower, upper, limb) per 4-bit digit / the limb per 2-bit digit
 *   per fixed-base window  gadgets/curve_fixed_base.rs:56-61  is_equal(limb, zero), not(.), the
 *        random_access_curve_points selection (gadgets/curve_windowed_mul.rs:74-118: 9 x limbs, 9 y limbs)
 *   per MSM digit  gadgets/curve_msm.rs:67-71  index = mul_add(four, limb_m, limb_n), the selection, is_equal, not
 *   per curve_conditional_add  gadgets/curve.rs:232-238  not(b), then the mul_biguint_by_bool products
 *        (gadgets/biguint.rs:360-374) sum.x*b, sum.y*b, p1.x*not_b, p1.y*not_b
 *   per nonnative_conditional_neg  gadgets/nonnative.rs:590-593  not(b), neg*b, x*not_b
 * aux[P2E_VERIFY_AUX_COLS or P2E_GLV_MUL_AUX_COLS][ld_aux], column-major like cols.  err[i] gets
 * P2E_ERR_LIMB_RANGE where a split scalar has a limb >= 2^29 (split_le_base has no witness then).  Wire
 * placement of these targets is not part of this library (plonky2's gate sources are not available offline). */
#define P2E_VERIFY_AUX_COLS 8959
#define P2E_GLV_MUL_AUX_COLS 4738
long p2e_aux_witness_batch(p2e_ctx *ctx, int program, const uint8_t *pky32, const uint64_t *cols, size_t ld,
                           uint64_t *aux, size_t ld_aux, size_t n, uint8_t *err);
/* The same pass inside the compact container: reads only its narrow matrix (every column this pass needs is a limb
 * or a flag), writes aux as u32 aux32[P2E_*_AUX_COLS][ld_aux] (every value is a limb, a bit, a digit or a flag). */
long p2e_aux_witness_compact_batch(p2e_ctx *ctx, int program, const uint8_t *pky32, const uint32_t *narrow,
                                   size_t ld_narrow, uint32_t *aux32, size_t ld_aux, size_t n, uint8_t *err);
typedef struct p2e_aux_desc {
    int32_t kind; /* 0 split4, 1 split2, 2 fixed-base window, 3 MSM digit, 4 conditional neg */
    uint32_t first_col, num_cols;
    char label[48];
} p2e_aux_desc;
long p2e_aux_describe(int program, p2e_aux_desc *out, size_t cap);
long p2e_aux_num_cols(int program);

/* Gate-internal values of the built-in gates on the path, the rest of SURVEY.md 8(f) rank 1: what plonky2's own
 * generators write into wires of their gates beyond the targets the gadgets get back -- per window, in call order,
 *   is_equal(index, zero) (gadgets/curve_fixed_base.rs:57, gadgets/curve_msm.rs:70): not(equal), the
 *        EqualityGenerator's inv = index^-1 in Goldilocks (0 for index 0), diff, diff * inv, diff * (diff * inv)
 *   random_access_curve_points (gadgets/curve_windowed_mul.rs:96-103): per selected limb (9 x, 9 y) the 4 bit
 *        wires of its RandomAccessGate op's access index, least significant first
 * (fixed-base windows: is_equal first; MSM digits: random_access first) = 77 values per window, derived from the aux
 * matrix alone.  gate[P2E_VERIFY_GATE_COLS or P2E_GLV_MUL_GATE_COLS][ld_gate], u64.  [upstream-from-memory: plonky2's
 * is_equal / EqualityGenerator / RandomAccessGenerator are not in the container; "parity unpinned"] */
#define P2E_VERIFY_GATE_COLS 10703
#define P2E_GLV_MUL_GATE_COLS 5621
long p2e_gate_internal_batch(p2e_ctx *ctx, int program, const uint64_t *aux, size_t ld_aux, uint64_t *gate, size_t ld_gate,
                             size_t n);
long p2e_gate_internal_num_cols(int program);
/* the same pass from the u32 aux matrix of p2e_aux_witness_compact_batch (same values; the gate matrix stays u64: the
 * equality gadget's inverse is a full Goldilocks element) */
long p2e_gate_internal_compact_batch(p2e_ctx *ctx, int program, const uint32_t *aux32, size_t ld_aux, uint64_t *gate,
                                     size_t ld_gate, size_t n);

/* ---- constraint-block columns ---------------------------------------------- */
/* The values of the targets the plonky2_ux U29 gates fill INSIDE the constraint blocks of the non-native gadgets
 * (gadgets/nonnative.rs:262-273 add, :330-351 add_many, :373-386 sub, :518-530 inv, :462-463 mul's range check): what
 * add_biguint / sub_biguint / mul_biguint (gadgets/biguint.rs:240-323) receive back from add_many_ux, sub_ux, mul_ux
 * and add_uxs_with_carry (limb, carry / borrow), the mul_biguint_by_bool products modulus * overflow (:360-374), and
 * the cmp_biguint result of a range-checked gadget -- generator by generator, in the order the builder makes the
 * calls (p2e_ux_describe).  Derived on the GPU from the finished matrices `cols` and `aux` (p2e_aux_witness_batch),
 * the packed inputs and the circuit constants through the wiring of p2e_schedule_wiring.
 * ux[P2E_VERIFY_UX_COLS or P2E_GLV_MUL_UX_COLS][ld_ux]: u64 (ux_u32 = 0) or u32 (every value is < 2^29).
 * glv_mul program: k32 travels in msg32, r32 / s32 are ignored (may be NULL).  err[i] gets P2E_ERR_LIMB_RANGE where an
 * operand limb is not a U29 value.  plonky2_ux is not available offline: the gates are modelled by what they constrain
 * (oracle/check_circuit.py holds the same model; "parity unpinned"). */
#define P2E_VERIFY_UX_COLS 249385
#define P2E_GLV_MUL_UX_COLS 194361
long p2e_ux_witness_batch(p2e_ctx *ctx, int program, const uint8_t *msg32, const uint8_t *r32, const uint8_t *s32,
                          const uint8_t *pkx32, const uint8_t *pky32, const uint64_t *cols, size_t ld, const uint64_t *aux,
                          size_t ld_aux, void *ux, int ux_u32, size_t ld_ux, size_t n, uint8_t *err);
/* the same pass inside the compact container: every witness column it reads is a limb, an overflow word or a flag, so
 * it reads the u32 narrow matrix of the compact fills and the u32 aux matrix of p2e_aux_witness_compact_batch -- same
 * values, same err semantics, half the bytes read.  Any ld_narrow >= n works (no alignment assumption). */
long p2e_ux_witness_compact_batch(p2e_ctx *ctx, int program, const uint8_t *msg32, const uint8_t *r32, const uint8_t *s32,
                                  const uint8_t *pkx32, const uint8_t *pky32, const uint32_t *narrow, size_t ld_narrow,
                                  const uint32_t *aux32, size_t ld_aux, void *ux, int ux_u32, size_t ld_ux, size_t n, uint8_t *err);
typedef struct p2e_ux_desc {
    uint32_t first_col, num_cols; /* this generator's block (num_cols = 0: none, e.g. an unchecked mul) */
} p2e_ux_desc;
/* one entry per generator, same index as p2e_schedule_describe; returns the generator count */
long p2e_ux_describe(int program, p2e_ux_desc *out, size_t cap);
long p2e_ux_num_cols(int program);

/* ---- wire-matrix assembly -------------------------------------------------- */
/* plonky2's prover consumes one matrix per proof, wire_values[num_wires][degree] (PartitionWitness::full_witness,
 * [upstream-from-memory]); a generator's targets are Target::wire(row, column) of the gate rows the builder placed
 * (gates/mul_nonnative.rs:208-226) or virtual targets.  The placement belongs to the circuit build on the Rust side,
 * so it is an INPUT here: a map from library columns to wire-matrix positions, built once per circuit from the
 * targets the gadgets returned.  One entry copies one value; the same source may feed
 * several positions (copy constraints: the x / y wires of a MulNonnativeGate row repeat the operand's limbs).
 *   src = P2E_WIRE_SRC_COLS | c, P2E_WIRE_SRC_AUX | c, P2E_WIRE_SRC_UX | c or P2E_WIRE_SRC_GATE | c   (column c of that matrix)
 *   dst = wire * degree + row        (element index inside one signature's wire matrix)
 * p2e_wire_map_create sorts a copy by dst (coalesced scatter) and keeps it on the device; entries must be in range
 * (dst < num_wires * degree) and no two entries may share a dst.
 * p2e_assemble_wires: wires[i * wire_stride + dst] = value of signature i, for every map entry; positions no entry
 * names are left as they are (zero-fill once, re-use the buffer).  wire_stride >= num_wires * degree elements.
 * A matrix whose entries the map does not use may be NULL.  ux is the u64 or u32 matrix of p2e_ux_witness_batch, gate
 * the matrix of p2e_gate_internal_batch. */
#define P2E_WIRE_SRC_COLS 0x00000000u
#define P2E_WIRE_SRC_AUX 0x40000000u
#define P2E_WIRE_SRC_UX 0x80000000u
#define P2E_WIRE_SRC_GATE 0xC0000000u
typedef struct p2e_wire_map_entry {
    uint32_t src, dst;
} p2e_wire_map_entry;
typedef struct p2e_wire_map p2e_wire_map;
int p2e_wire_map_create(p2e_ctx *ctx, int program, const p2e_wire_map_entry *entries, size_t count, uint32_t num_wires,
                        uint32_t degree, p2e_wire_map **out);
void p2e_wire_map_destroy(p2e_ctx *ctx, p2e_wire_map *map);
long p2e_assemble_wires(p2e_ctx *ctx, const p2e_wire_map *map, const uint64_t *cols, size_t ld, const uint64_t *aux,
                        size_t ld_aux, const void *ux, int ux_u32, size_t ld_ux, const uint64_t *gate, size_t ld_gate,
                        uint64_t *wires, size_t wire_stride, size_t n);
/* The same scatter from the compact container: witness entries gather from narrow / wide, aux entries from the u32 aux
 * matrix.  A map keeps its witness sources in both coordinates (p2e_wire_map_create and
 * p2e_curve_program_wire_map_create know the program's compact layout), so one map serves both containers.  narrow or
 * wide may be NULL if no entry names a column of it. */
long p2e_assemble_wires_compact(p2e_ctx *ctx, const p2e_wire_map *map, const uint32_t *narrow, size_t ld_narrow,
                                const uint64_t *wide, size_t ld_wide, const uint32_t *aux32, size_t ld_aux, const void *ux,
                                int ux_u32, size_t ld_ux, const uint64_t *gate, size_t ld_gate, uint64_t *wires,
                                size_t wire_stride, size_t n);

/* ---- layout helper --------------------------------------------------------------------------------- */
/* cols[ncols][ld] (column-major over the batch) -> rows[n][row_ld], one contiguous witness per signature:
 * what a per-signature PartialWitness fill (pw.set_biguint_target ... gadgets/biguint.rs:454-463 per target,
 * INTEGRATION.md section 3) wants to read.  row_ld >= ncols. */
long p2e_columns_to_rows(p2e_ctx *ctx, const uint64_t *cols, size_t ld, size_t n, size_t ncols, uint64_t *rows,
                         size_t row_ld);

/* Compact container for transfers (BASELINE config 5 is bound by the host link, not by the GPU): 57 % of the
 * columns only ever hold values < 2^32 (29-bit limbs, overflow words, flags; set through set_ux_target /
 * set_bool_target in the reference, gadgets/nonnative.rs:643-644,726-727) and are repacked as u32 narrow[num_narrow][ld_narrow];
 * the check_sum[17] and b[16] columns of every mul generator (gates/mul_nonnative.rs:305-322,518-527) stay u64
 * wide[num_wide][ld_wide]: 474 KB instead of 661 KB per verify.  col_map[c] (p2e_compact_layout, host only) is the
 * index of witness column c inside its matrix, with P2E_COMPACT_WIDE set for the wide one.  err[i] gets
 * P2E_ERR_LIMB_RANGE if a narrow column of signature i holds a value >= 2^32 (cannot happen for this library's
 * own output). */
#define P2E_COMPACT_WIDE 0x80000000u
long p2e_compact_layout(int program, uint32_t *col_map, size_t cap, uint32_t *num_narrow, uint32_t *num_wide);
long p2e_columns_compact(p2e_ctx *ctx, int program, const uint64_t *cols, size_t ld, size_t n, uint32_t *narrow,
                         size_t ld_narrow, uint64_t *wide, size_t ld_wide, uint8_t *err);
/* The fused schedules writing the compact container directly (same values, same err / valid semantics as
 * p2e_ecdsa_verify_witness_batch / p2e_glv_mul_witness_batch; 28 % fewer bytes leave the kernels):
 * narrow[num_narrow][ld_narrow] u32, wide[num_wide][ld_wide] u64, ld_narrow >= n, ld_wide >= n. */
long p2e_ecdsa_verify_witness_compact_batch(p2e_ctx *ctx, const uint8_t *msg32, const uint8_t *r32, const uint8_t *s32,
                                            const uint8_t *pkx32, const uint8_t *pky32, uint32_t *narrow,
                                            size_t ld_narrow, uint64_t *wide, size_t ld_wide, size_t n, uint8_t *err,
                                            uint8_t *valid);
long p2e_glv_mul_witness_compact_batch(p2e_ctx *ctx, const uint8_t *px32, const uint8_t *py32, const uint8_t *k32,
                                       uint32_t *narrow, size_t ld_narrow, uint64_t *wide, size_t ld_wide, size_t n,
                                       uint8_t *err, uint8_t *valid);

/* p2e_columns_to_rows for the compact container: one contiguous run of num_narrow u32 and one of num_wide u64 per
 * signature (rows_narrow[n][row_ld_narrow], rows_wide[n][row_ld_wide]). */
long p2e_compact_to_rows(p2e_ctx *ctx, int program, const uint32_t *narrow, size_t ld_narrow, const uint64_t *wide,
                         size_t ld_wide, size_t n, uint32_t *rows_narrow, size_t row_ld_narrow, uint64_t *rows_wide,
                         size_t row_ld_wide);

/* ---- schedule description (column -> generator map, host only, no GPU needed) ---------------------- */
typedef struct p2e_gen_desc {
    int32_t kind;  /* 0 add, 1 sub, 2 add_many, 3 mul(+checksum), 4 inv, 5 glv_decomposition */
    int32_t field; /* P2E_FIELD_* */
    uint32_t first_col, num_cols;
    char label[48]; /* gadget path, e.g. "glv_mul/msm/digit72" */
} p2e_gen_desc;
/* program 0 = verify circuit, 1 = glv_mul.  Writes up to cap entries; returns the total count. */
long p2e_schedule_describe(int program, p2e_gen_desc *out, size_t cap);
long p2e_schedule_num_cols(int program);
/* Operand wiring of generator g (same index as p2e_schedule_describe): where the targets the gadget passed to it live.
 * This is what the reference fixes by handing targets from one CircuitBuilderNonNative call to the next
 * (gadgets/curve.rs:160-243, gadgets/glv.rs:53-104, gadgets/ecdsa.rs:30-53); the Rust side has it as Target lists
 * (dependencies(), gadgets/nonnative.rs:618-624), a batch consumer needs it as columns.  src[k]:
 *   c < 2^29                     first limb column c of the witness matrix (limbs in consecutive columns)
 *   P2E_SRC_AUX | c              column c of the built-in-generator matrix (a mul_biguint_by_bool product, a
 *                                random_access_curve_points selection: p2e_aux_witness_batch)
 *   P2E_SRC_INPUT | slot         a caller input: 0 pk.y, 1 pk.x, 2 msg (glv_mul: k), 3 r, 4 s (9-limb virtual targets);
 *                                the MSM curve program also 5 q.x, 6 q.y
 *   P2E_SRC_CONST | id           a circuit constant (constant_biguint, gadgets/biguint.rs:165-175): p2e_wiring_const
 * num_limbs[k]: limbs that target has (constants: convert_base's count, zero has none -- quirk Q5; k1, k2: 5).
 * range_check: the gadget's range_check flag (one more cmp_biguint in its constraint block, nonnative.rs:180-190). */
#define P2E_SRC_AUX 0x20000000u
#define P2E_SRC_INPUT 0x40000000u
#define P2E_SRC_CONST 0x80000000u
typedef struct p2e_gen_wiring {
    int32_t num_operands; /* add, sub: 2; add_many: 4; mul: 2; inv: 1; glv: 1 */
    uint32_t src[4];
    uint8_t num_limbs[4];
    int32_t range_check;
} p2e_gen_wiring;
long p2e_schedule_wiring(int program, p2e_gen_wiring *out, size_t cap);
/* value of constant `id` as 32 little-endian bytes; returns its limb count (0 for the zero constant), < 0: unknown id */
int p2e_wiring_const(uint32_t id, uint8_t out32[32]);

/* ---- curve programs --------------------------------------------------------- */
/* The crate's other scalar-multiplication gadgets, on either of its curves, through the same phases as the built-in
 * programs:
 *   P2E_CP_WINDOWED_MUL  curve_scalar_mul_windowed(p, n, true)  gadgets/curve_windowed_mul.rs:131-173   98 185 columns
 *   P2E_CP_SCALAR_MUL    curve_scalar_mul(p, n, true)           gadgets/curve.rs:245-285               139 354 columns
 *   P2E_CP_VERIFY        verify_p256_message_circuit            gadgets/ecdsa.rs:55-78 (P-256 only)    115 557 columns
 *   P2E_CP_MSM           curve_msm_circuit(p, q, n, m)          gadgets/curve_msm.rs:21-79             112 309 columns
 *   P2E_CP_FIXED_BASE_MUL  fixed_base_curve_mul_circuit(base, n)  gadgets/curve_fixed_base.rs:18-66     16 797 columns
 * Both gadgets blind with a point drawn by rand() WHILE THE CIRCUIT IS BUILT (precompute_window
 * gadgets/curve_windowed_mul.rs:57, curve_scalar_mul gadgets/curve.rs:253), so their witness depends on the build:
 * a program object stands for one built circuit and takes that point (canonical affine coordinates, 32 little-endian
 * bytes each) as an argument -- the Rust side passes the point its builder drew.  Column order = generator
 * registration order as for the built-in programs (p2e_curve_program_describe / _wiring mirror
 * p2e_schedule_describe / _wiring; constant ids of a program resolve through p2e_curve_program_const: 2c / 2c + 1 =
 * x / y of constant point c, 64 + j = scalar constant j).  The other targets of the same circuits have the same three
 * passes as the built-in programs: p2e_curve_program_aux_witness_batch (built-in-generator targets, layout
 * p2e_curve_program_aux_describe: kinds 0 split4, 2 fixed-base window, 5 window of the windowed multiplication
 * [selected x (9), selected y (9), is_zero, should_add, not_b, sum.x*b, sum.y*b, p1.x*not_b, p1.y*not_b], 6 bit split,
 * 7 bit of curve_scalar_mul [not_bit, sum.x*bit, result.x*not_bit, sum.y*bit, result.y*not_bit]),
 * p2e_curve_program_gate_internal_batch and p2e_curve_program_ux_witness_batch (+ _ux_describe).
 * A program belongs to the context's device.  Every fill and every pass exists for the u64 column matrix and for the
 * compact container (the *_compact_batch entry points below).
 * The MSM program has full 9-limb scalars (131 two-bit digits, MSB first) and no per-build randomness: its blinding point
 * is KeccakHash::<32>(F::ZERO) * G of its curve, so the point arguments of p2e_curve_program_create are ignored (may be
 * NULL) and its witness is a pure function of (p, q, n, m).  Fill: p2e_curve_msm_witness[_compact]_batch; aux kinds 1
 * split2 (261 bits + 131 digits per scalar) and 3 MSM digit [index, selected x (9), selected y (9), is_zero, should_add,
 * not_b, sum.x*b, sum.y*b, p1.x*not_b, p1.y*not_b]; its wiring reads q through P2E_SRC_INPUT slots 5 (q.x) and 6 (q.y).
 * Its constraint-block pass is p2e_curve_msm_ux_witness_batch (u64 matrices) or
 * p2e_curve_program_ux_witness_compact_batch; p2e_curve_program_ux_witness_batch has no slot for q and returns
 * P2E_E_INVALID for it.
 * The fixed-base program multiplies a CONSTANT base: the point arguments of p2e_curve_program_create are that base
 * (canonical, on the program's curve); its fill is p2e_curve_mul_witness[_compact]_batch with px32 = py32 = NULL. */
#define P2E_CURVE_SECP256K1 0
#define P2E_CURVE_P256 1
#define P2E_CP_WINDOWED_MUL 1
#define P2E_CP_SCALAR_MUL 2
#define P2E_CP_VERIFY 3
#define P2E_CP_MSM 4
#define P2E_CP_FIXED_BASE_MUL 5
typedef struct p2e_curve_program p2e_curve_program;
int p2e_curve_program_create(p2e_ctx *ctx, int kind, int curve, const uint8_t *blind_x32, const uint8_t *blind_y32,
                             p2e_curve_program **out);
void p2e_curve_program_destroy(p2e_ctx *ctx, p2e_curve_program *prog);
long p2e_curve_program_num_cols(const p2e_curve_program *prog);
long p2e_curve_program_num_aux_cols(const p2e_curve_program *prog);
size_t p2e_curve_program_scratch_bytes(const p2e_curve_program *prog, size_t n);
long p2e_curve_program_describe(const p2e_curve_program *prog, p2e_gen_desc *out, size_t cap);
long p2e_curve_program_wiring(const p2e_curve_program *prog, p2e_gen_wiring *out, size_t cap);
long p2e_curve_program_aux_describe(const p2e_curve_program *prog, p2e_aux_desc *out, size_t cap);
int p2e_curve_program_const(const p2e_curve_program *prog, uint32_t id, uint8_t out32[32]);
long p2e_curve_program_num_gate_cols(const p2e_curve_program *prog);
long p2e_curve_program_num_ux_cols(const p2e_curve_program *prog);
long p2e_curve_program_ux_describe(const p2e_curve_program *prog, p2e_ux_desc *out, size_t cap);
/* inputs as for the program's fill (multiplication programs: the scalar in msg32, r32 = s32 = NULL; the MSM program: n in
 * msg32, m in r32, s32 and the points may be NULL; the fixed-base program: the scalar in msg32, everything else may be NULL) */
/* the wire map of p2e_wire_map_create for this program's matrices (then p2e_assemble_wires / p2e_wire_map_destroy) */
int p2e_curve_program_wire_map_create(p2e_ctx *ctx, const p2e_curve_program *prog, const p2e_wire_map_entry *entries,
                                      size_t count, uint32_t num_wires, uint32_t degree, p2e_wire_map **out);
long p2e_curve_program_aux_witness_batch(p2e_ctx *ctx, const p2e_curve_program *prog, const uint8_t *msg32, const uint8_t *r32,
                                         const uint8_t *s32, const uint8_t *pkx32, const uint8_t *pky32, const uint64_t *cols,
                                         size_t ld, uint64_t *aux, size_t ld_aux, size_t n, uint8_t *err);
long p2e_curve_program_gate_internal_batch(p2e_ctx *ctx, const p2e_curve_program *prog, const uint64_t *aux, size_t ld_aux,
                                           uint64_t *gate, size_t ld_gate, size_t n);
long p2e_curve_program_ux_witness_batch(p2e_ctx *ctx, const p2e_curve_program *prog, const uint8_t *msg32, const uint8_t *r32,
                                        const uint8_t *s32, const uint8_t *pkx32, const uint8_t *pky32, const uint64_t *cols,
                                        size_t ld, const uint64_t *aux, size_t ld_aux, void *ux, int ux_u32, size_t ld_ux, size_t n,
                                        uint8_t *err);
/* the MSM program's constraint-block pass on the u64 matrices (argument order of p2e_curve_msm_witness_batch) */
long p2e_curve_msm_ux_witness_batch(p2e_ctx *ctx, const p2e_curve_program *prog, const uint8_t *px32, const uint8_t *py32,
                                    const uint8_t *qx32, const uint8_t *qy32, const uint8_t *n32, const uint8_t *m32,
                                    const uint64_t *cols, size_t ld, const uint64_t *aux, size_t ld_aux, void *ux, int ux_u32,
                                    size_t ld_ux, size_t n, uint8_t *err);
/* The three passes inside the compact container (as p2e_aux_witness_compact_batch / p2e_gate_internal_compact_batch /
 * p2e_ux_witness_compact_batch): narrow is the u32 matrix of the program's compact fill, aux32 the u32 aux matrix.  The
 * constraint-block pass takes every program kind: qx32 / qy32 are required for P2E_CP_MSM and ignored (may be NULL)
 * otherwise. */
long p2e_curve_program_aux_witness_compact_batch(p2e_ctx *ctx, const p2e_curve_program *prog, const uint8_t *msg32,
                                                 const uint8_t *r32, const uint8_t *s32, const uint8_t *pkx32,
                                                 const uint8_t *pky32, const uint32_t *narrow, size_t ld_narrow,
                                                 uint32_t *aux32, size_t ld_aux, size_t n, uint8_t *err);
long p2e_curve_program_gate_internal_compact_batch(p2e_ctx *ctx, const p2e_curve_program *prog, const uint32_t *aux32,
                                                   size_t ld_aux, uint64_t *gate, size_t ld_gate, size_t n);
long p2e_curve_program_ux_witness_compact_batch(p2e_ctx *ctx, const p2e_curve_program *prog, const uint8_t *msg32,
                                                const uint8_t *r32, const uint8_t *s32, const uint8_t *pkx32,
                                                const uint8_t *pky32, const uint8_t *qx32, const uint8_t *qy32,
                                                const uint32_t *narrow, size_t ld_narrow, const uint32_t *aux32, size_t ld_aux,
                                                void *ux, int ux_u32, size_t ld_ux, size_t n, uint8_t *err);
/* replaces the run_once bodies of every generator curve_scalar_mul_windowed / curve_scalar_mul registers for a batch
 * of (point, scalar) pairs; cols[num_cols][ld].  valid: always 1 unless flagged (the gadgets connect nothing).
 * The fixed-base program (P2E_CP_FIXED_BASE_MUL) takes the scalars alone: px32 = py32 = NULL (ignored if given); the
 * other two kinds fail with P2E_E_INVALID on a NULL point. */
long p2e_curve_mul_witness_batch(p2e_ctx *ctx, const p2e_curve_program *prog, const uint8_t *px32, const uint8_t *py32,
                                 const uint8_t *k32, uint64_t *cols, size_t n, size_t ld, uint8_t *err, uint8_t *valid);
/* curve_msm_circuit(p, q, n, m) = n p + m q for a batch (P2E_CP_MSM programs only): p in (px32, py32), q in (qx32, qy32),
 * n32 / m32 32-byte little-endian scalars (as k32 above); cols[num_cols][ld].  valid: 1 unless flagged; exceptional
 * additions (p = +-q, n = m = 0, ...) set P2E_ERR_INVERSE_OF_ZERO on that element. */
long p2e_curve_msm_witness_batch(p2e_ctx *ctx, const p2e_curve_program *prog, const uint8_t *px32, const uint8_t *py32,
                                 const uint8_t *qx32, const uint8_t *qy32, const uint8_t *n32, const uint8_t *m32, uint64_t *cols,
                                 size_t n, size_t ld, uint8_t *err, uint8_t *valid);
/* the same for verify_p256_message_circuit; valid = curve_assert_valid's connect and r == x both hold */
long p2e_p256_verify_witness_batch(p2e_ctx *ctx, const p2e_curve_program *prog, const uint8_t *msg32, const uint8_t *r32,
                                   const uint8_t *s32, const uint8_t *pkx32, const uint8_t *pky32, uint64_t *cols, size_t n,
                                   size_t ld, uint8_t *err, uint8_t *valid);
/* Both fills writing the COMPACT container instead (as p2e_ecdsa_verify_witness_compact_batch: u32 narrow[num_narrow]
 * [ld_narrow] for the columns that only ever hold values < 2^32 -- 29-bit limbs, overflow words, flags --, u64
 * wide[num_wide][ld_wide] for the check_sum / carry columns of the mul generators; both indices advance in generator
 * registration order).  p2e_curve_program_compact_layout: col_map[c] = narrow row of witness column c, or
 * P2E_COMPACT_WIDE | wide row; returns num_cols. */
long p2e_curve_mul_witness_compact_batch(p2e_ctx *ctx, const p2e_curve_program *prog, const uint8_t *px32, const uint8_t *py32,
                                         const uint8_t *k32, uint32_t *narrow, size_t ld_narrow, uint64_t *wide, size_t ld_wide,
                                         size_t n, uint8_t *err, uint8_t *valid);
long p2e_p256_verify_witness_compact_batch(p2e_ctx *ctx, const p2e_curve_program *prog, const uint8_t *msg32, const uint8_t *r32,
                                           const uint8_t *s32, const uint8_t *pkx32, const uint8_t *pky32, uint32_t *narrow,
                                           size_t ld_narrow, uint64_t *wide, size_t ld_wide, size_t n, uint8_t *err,
                                           uint8_t *valid);
long p2e_curve_msm_witness_compact_batch(p2e_ctx *ctx, const p2e_curve_program *prog, const uint8_t *px32, const uint8_t *py32,
                                         const uint8_t *qx32, const uint8_t *qy32, const uint8_t *n32, const uint8_t *m32,
                                         uint32_t *narrow, size_t ld_narrow, uint64_t *wide, size_t ld_wide, size_t n, uint8_t *err,
                                         uint8_t *valid);
long p2e_curve_program_compact_layout(const p2e_curve_program *prog, uint32_t *col_map, size_t cap, uint32_t *num_narrow,
                                      uint32_t *num_wide);
/* the P-256 verifier's verdict alone (the counterpart of p2e_ecdsa_verify_batch; native: curve/ecdsa.rs:42-62
 * verify_message with C = P256, with exactly the circuit's verdict): no witness, 2 bytes per signature */
long p2e_p256_verify_batch(p2e_ctx *ctx, const p2e_curve_program *prog, const uint8_t *msg32, const uint8_t *r32,
                           const uint8_t *s32, const uint8_t *pkx32, const uint8_t *pky32, size_t n, uint8_t *err,
                           uint8_t *valid);
/* synthetic valid signatures on a curve (host only; P2E_CURVE_*), same stream layout as p2e_synth_signatures */
int p2e_synth_signatures_curve(int curve, uint64_t seed, size_t first, size_t n, uint8_t *msg32, uint8_t *r32, uint8_t *s32,
                               uint8_t *pkx32, uint8_t *pky32);

/* ---- key derivation and signing: the other two functions of the crate's native front end (curve/ecdsa.rs), for a
 * batch, on either curve (P2E_CURVE_*).  sk32, msg32 and k32 are n x 32-byte little-endian values, each taken modulo the
 * group order n with one conditional subtraction (the reference's arguments are field elements; this is what
 * from_noncanonical_biguint yields below 2^256) -- a value >= n is reduced, not flagged.  Outputs are n x 32 bytes each.
 * plan: P2E_SIGN_PLAN_LANE = one lane per scalar (a 64-deep chain of mixed additions through the generator's fixed-base
 * table), P2E_SIGN_PLAN_QUAD = four lanes per scalar (16 windows each, then two levels of general additions),
 * P2E_SIGN_PLAN_AUTO = the library's choice by batch size.  Same results, bit for bit.
 * The calls run one kernel on the context's caller stream (no internal streams, no scratch).  Return value: number of
 * flagged elements; P2E_E_INVALID on a null pointer, an unknown curve or an unknown plan; n == 0 returns 0.
 * Outputs that share bytes with other arguments: BUFFER OVERLAP at the top (pkx32 = sk32, r32 = msg32 and s32 = k32 are fine).
 *
 * p2e_ecdsa_public_key_batch   ECDSASecretKey::to_public (curve/ecdsa.rs:16-20): (pkx, pky) = affine sk G.
 *     sk = 0 (mod n): the reference returns AffinePoint::ZERO (curve/curve_types.rs:163-171); zeros are written and
 *     err[i] = P2E_ERR_POINT_AT_INFINITY.
 * p2e_ecdsa_sign_batch         sign_message (curve/ecdsa.rs:25-40) with the nonce as an input: R = k G,
 *     r = R.x mod n, s = k^-1 (msg + r sk) mod n.  k = 0 (mod n), where the reference redraws its nonce (:29-32):
 *     zeros are written and err[i] = P2E_ERR_INVERSE_OF_ZERO.  r = 0 or s = 0 are returned as computed and NOT flagged,
 *     as sign_message returns them; such a signature does not verify.
 * A zero Z of a non-empty sum (impossible for k < n, see csrc/sign.hpp) would set P2E_ERR_INVERSE_OF_ZERO too. */
#define P2E_SIGN_PLAN_AUTO 0
#define P2E_SIGN_PLAN_LANE 1
#define P2E_SIGN_PLAN_QUAD 2
/* curve/ecdsa.rs:16-20 to_public */
long p2e_ecdsa_public_key_batch(p2e_ctx *ctx, int curve, unsigned plan, const uint8_t *sk32, uint8_t *pkx32, uint8_t *pky32,
                                size_t n, uint8_t *err);
/* curve/ecdsa.rs:25-40 sign_message, with the nonce as an input */
long p2e_ecdsa_sign_batch(p2e_ctx *ctx, int curve, unsigned plan, const uint8_t *msg32, const uint8_t *sk32,
                          const uint8_t *k32, uint8_t *r32, uint8_t *s32, size_t n, uint8_t *err);

/* ---- public-key recovery: (msg, r, s, v) -> pk, the form in which Ethereum-style batches arrive (no key, one byte v),
 * on either curve (P2E_CURVE_*).  All 32-byte values little-endian, element i at +32 i; v[i] is one byte:
 *     bit 0 = the parity of R.y,   bit 1 = "R.x = r + n" (the abscissa was >= n before base_to_scalar reduced it).
 * The caller subtracts Ethereum's 27 or the EIP-155 offset; the library does not guess.  msg32 is taken modulo n with one
 * conditional subtraction, exactly as p2e_ecdsa_sign_batch takes it (reduced, not flagged); r32 and s32 are not reduced.
 *
 * p2e_ecdsa_recover_batch      pk = r^-1 (s R - msg G) = u1 G + u2 R, u1 = -msg r^-1, u2 = s r^-1 (mod n), R the curve
 *     point with x = r + n (v >> 1) and y = v & 1 (mod 2); (pkx, pky) = its canonical affine coordinates.
 *     Flagged elements (zeros are written to both outputs):
 *     P2E_ERR_NOT_RECOVERABLE    r = 0, r >= n, s = 0, s >= n, v > 3, x >= p, or x^3 + a x + b is not a square;
 *     P2E_ERR_POINT_AT_INFINITY  u1 G + u2 R is the neutral element (s R = msg G).
 *     A recoverable signature of "someone else" is not an error: any well-formed (r, s, v) names some key.
 * p2e_ecdsa_sign_recoverable_batch   p2e_ecdsa_sign_batch plus v[i] = (R.y & 1) | (R.x >= n ? 2 : 0), 0 where flagged;
 *     r, s and err are bit for bit those of p2e_ecdsa_sign_batch for the same inputs and plan.
 * One kernel per call on the context's caller stream, one lane per signature in the recovery (no internal streams, no
 * scratch, no LDS).  Return value: number of flagged elements; P2E_E_INVALID on a null pointer, an unknown curve (or
 * plan); n == 0 returns 0.  Host pointers, async mode and the current device behave as for the signing calls; so does
 * BUFFER OVERLAP (pkx32 = r32 and pky32 = s32 are fine).
 * A zero Z at the end of the walk (impossible, see csrc/recover.hpp) would set P2E_ERR_INVERSE_OF_ZERO. */
long p2e_ecdsa_recover_batch(p2e_ctx *ctx, int curve, const uint8_t *msg32, const uint8_t *r32, const uint8_t *s32,
                             const uint8_t *v, uint8_t *pkx32, uint8_t *pky32, size_t n, uint8_t *err);
long p2e_ecdsa_sign_recoverable_batch(p2e_ctx *ctx, int curve, unsigned plan, const uint8_t *msg32, const uint8_t *sk32,
                                      const uint8_t *k32, uint8_t *r32, uint8_t *s32, uint8_t *v, size_t n, uint8_t *err);

/* ---- message hashing, deterministic nonces and Ethereum addresses: the two ends of the signing pipeline.  Raw bytes on
 * the device become msg32, then (r, s, v), then pk, then the sender's address, and nothing passes through the host.
 * The nearest reference counterpart is curve/ecdsa.rs:25-40 sign_message, which takes the message as a field element and
 * draws its nonce with rand() (:29-32): the reference neither hashes nor derives nonces, so what these calls compute is
 * defined by FIPS 180-4 (SHA-256), the Keccak submission as Ethereum uses it, and RFC 6979 section 3.2.
 *
 * p2e_hash_batch      out32[32 i ..] = hash of message i = data[offsets[i], offsets[i + 1]), i < n (offsets holds n + 1
 *     entries).  Messages are concatenated without padding; neither data nor any offset needs an alignment (out32 and
 *     offsets are aligned to 4 and 8 bytes, as arrays of their types).  The kernel reads aligned 4-byte words and only
 *     those that hold at least one byte of a message: nothing before data + offsets[i] rounded down to 4 and nothing from
 *     data + offsets[i + 1] rounded up to 4 on.  Every offset lies in [offsets[0], offsets[n]].
 *     alg: P2E_HASH_SHA256, P2E_HASH_SHA256D (SHA-256 of the SHA-256 digest), P2E_HASH_KECCAK256 (rate 136, the legacy
 *     0x01 padding: Ethereum's hash, NOT SHA3-256).  out_form: P2E_DIGEST_BYTES = the 32 digest bytes in the order the
 *     hash defines;  P2E_DIGEST_SCALAR = the same bytes reversed, i.e. the digest read as a big-endian integer and stored
 *     as the 32-byte little-endian msg32 of every other entry point.
 *     An element with offsets[i + 1] < offsets[i] is hashed as the empty message; the return value is the number of such
 *     elements (0 otherwise).  P2E_E_INVALID on a null pointer or an unknown alg or out_form; n == 0 returns 0.
 *     With P2E_CTX_HOST_POINTERS the library reads offsets[0] and offsets[n] on the host to size its staging copy of
 *     data[offsets[0], offsets[n]) (offsets[n] < offsets[0] is P2E_E_INVALID there).
 * p2e_ecdsa_nonce_rfc6979_batch   k32[32 i ..] = the RFC 6979 section 3.2 nonce (HMAC-SHA256; qlen = hlen = 256, so
 *     bits2int is the identity on both curves) for the key sk32[i] and the message hash msg32[i], both taken modulo n
 *     exactly as p2e_ecdsa_sign_batch takes them; 32 bytes little-endian, 1 <= k < n.  Returns 0.
 *     The output is secret and a nonce must never sign two different messages: both are the caller's concern.
 * p2e_ecdsa_sign_deterministic_batch   r, s, v and err are bit for bit what p2e_ecdsa_sign_recoverable_batch returns for
 *     the same inputs and plan with k32 taken from p2e_ecdsa_nonce_rfc6979_batch; v == NULL: no recovery byte is written
 *     (p2e_ecdsa_sign_batch's outputs).  Two launches on the caller's stream: the nonce kernel writes into the context's
 *     scratch block (32 n bytes, allocated on first need and kept), the unchanged signing kernel reads it, and a memset
 *     on the same stream wipes it behind the signer.  r = 0 or s = 0 are returned as computed and NOT flagged, as
 *     sign_message and p2e_ecdsa_sign_batch return them: RFC 6979 section 3.2's further retry for them (step h.3's "if r
 *     or s is zero, update K and V and loop") is NOT implemented.  sk = 0 (mod n) is defined and not flagged, as in the
 *     plain signer.  Return value: number of flagged elements (none for k in [1, n)).
 * p2e_eth_address_batch   addr20[20 i ..] = keccak256(BE32(pkx) || BE32(pky))[12..32], the inputs being this library's
 *     little-endian coordinates (each is reversed).  err (nullable): where err[i] != 0, twenty zero bytes are written --
 *     pass the err of p2e_ecdsa_recover_batch, whose flagged elements hold zero coordinates that must not turn into a
 *     plausible address.  addr20 is 4-byte aligned.  Returns 0.  secp256k1 by meaning: there is no curve argument.
 * Each call is one kernel (the deterministic signer: two and a memset) on the context's caller stream: no internal
 * streams, no LDS.  P2E_E_INVALID on a null pointer (other than the nullable ones), an unknown curve or plan; n == 0
 * returns 0.  Host pointers, async mode, the current device and failed calls behave as for the signing calls.  BUFFER OVERLAP
 * (top of this file): k32 = msg32 and r32 = msg32 are fine; addr20 and out32 have a stride of their own and lie on no input;
 * the variable-length data of p2e_hash_batch must not touch out32 (the caller's duty, checked with host pointers only). */
#define P2E_HASH_SHA256 0
#define P2E_HASH_SHA256D 1     /* SHA-256 of the SHA-256 digest (Bitcoin) */
#define P2E_HASH_KECCAK256 2   /* legacy 0x01 padding (Ethereum), not SHA3-256 */
#define P2E_DIGEST_BYTES 0     /* the 32 digest bytes as the hash defines them */
#define P2E_DIGEST_SCALAR 1    /* byte-reversed: the digest read as a big-endian integer, stored as the 32-byte
                                  little-endian msg32 every other entry point takes */
long p2e_hash_batch(p2e_ctx *ctx, int alg, unsigned out_form, const uint8_t *data, const uint64_t *offsets /* n + 1 */,
                    uint8_t *out32, size_t n);
long p2e_ecdsa_nonce_rfc6979_batch(p2e_ctx *ctx, int curve, const uint8_t *msg32, const uint8_t *sk32, uint8_t *k32,
                                   size_t n);
long p2e_ecdsa_sign_deterministic_batch(p2e_ctx *ctx, int curve, unsigned plan, const uint8_t *msg32,
                                        const uint8_t *sk32, uint8_t *r32, uint8_t *s32, uint8_t *v /* nullable */,
                                        size_t n, uint8_t *err);
long p2e_eth_address_batch(p2e_ctx *ctx, const uint8_t *pkx32, const uint8_t *pky32, const uint8_t *err /* nullable */,
                           uint8_t *addr20, size_t n);

/* ---- keys and signatures in wire form: SEC1 public keys and DER / compact ECDSA signatures, decoded and encoded on the
 * device, on either curve (P2E_CURVE_*).  A Bitcoin-style batch carries a DER signature and a 33-byte key, a WebAuthn /
 * X.509 / TLS batch a DER signature and a SEC1 key, an Ethereum typed transaction 65 bytes r || s || v: these calls turn
 * them into the 32-byte little-endian r32, s32, px32, py32 of every other entry point and back.  Everything in wire form
 * is big-endian as its standard defines.  The reference has no counterpart (curve/ecdsa.rs:7-23 holds field elements).
 * Below, p is the curve's field prime and n its group order.
 *
 * ERROR CODES.  P2E_ERR_NOT_RECOVERABLE took the last free bit of the error byte, so for these four calls err[i] is a
 * CODE (P2E_WIRE_*), NOT a set of P2E_ERR_* bits: the code of the first failing check in the order given below, 0 where
 * the element is fine.  A flagged element writes zeros to all its outputs.  The return value is the number of flagged
 * elements.
 *
 * VARIABLE-LENGTH INPUT (keys; DER signatures) follows p2e_hash_batch: element i = data[offsets[i], offsets[i + 1]),
 * offsets holds n + 1 entries, elements are concatenated without padding and need no alignment; offsets[i + 1] <
 * offsets[i] is an empty element (P2E_WIRE_BAD_LENGTH).  A lane reads aligned 4-byte words and only those that hold at
 * least one byte of its own element; it reads nothing for an element that is empty or longer than the form's maximum
 * (P2E_WIRE_BAD_LENGTH is decided from the offsets alone), and no word beyond those holding the bytes its checks have
 * admitted so far.
 *
 * p2e_point_decode_batch   SEC1 2.3.4.  Checks in order:
 *     1. length not in {1, 33, 65}: BAD_LENGTH;
 *     2. length 1: the byte 00 is the neutral element -- zeros and INFINITY (flagged: no key is the neutral element) --
 *        any other byte BAD_PREFIX;
 *     3. length 33 with a prefix other than 02 / 03, length 65 with a prefix other than 04: BAD_PREFIX (the hybrid
 *        prefixes 06 / 07 are refused here);
 *     4. x >= p, or for length 65 y >= p: COORD_RANGE;
 *     5. length 33: x^3 + a x + b is not a square: NOT_ON_CURVE; otherwise y is the root whose parity is prefix & 1
 *        (the recovery's square root, about 270 field multiplications);
 *     6. length 65: y^2 != x^3 + a x + b: NOT_ON_CURVE.   (Both curves have cofactor 1: on the curve is enough.)
 * p2e_point_encode_batch   form P2E_SEC1_COMPRESSED (stride 33) or P2E_SEC1_UNCOMPRESSED (stride 65): element i at
 *     out + stride i, no alignment needed.  (0, 0): zeros and INFINITY; a coordinate >= p: COORD_RANGE; off the curve:
 *     NOT_ON_CURVE.
 * p2e_sig_decode_batch     form P2E_SIG_DER (variable length, offsets required), P2E_SIG_COMPACT64 (r || s, stride 64,
 *     offsets NULL) or P2E_SIG_COMPACT65 (r || s || v, stride 65, offsets NULL).  COMPACT65: v[i] is the 65th byte as it
 *     is -- no 27 and no EIP-155 offset is subtracted, nothing about it is checked (see p2e_ecdsa_recover_batch); v is
 *     nullable there and ignored in the other forms.  flags: 0, P2E_SIG_REQUIRE_LOW_S or P2E_SIG_NORMALIZE_S (both:
 *     P2E_E_INVALID).  DER is strict, BIP-66's rules; a trailing sighash-type byte is not part of the element (the
 *     caller's offsets leave it out).  For an element b of length L, in order:
 *     1. L < 8 or L > 72: BAD_LENGTH;
 *     2. b[0] != 30 or b[1] != L - 2: DER_SYNTAX (long-form lengths are refused by this);
 *     3. b[2] != 02;  with lr = b[3]:  lr = 0, lr > 33 or lr + 7 > L: DER_SYNTAX;
 *     4. b[4 + lr] != 02;  with ls = b[5 + lr]:  ls = 0, ls > 33 or lr + ls + 6 != L: DER_SYNTAX;
 *     5. for r, then s: first byte >= 80 (negative), or length > 1 with first byte 00 and second byte < 80 (padded):
 *        DER_INTEGER;
 *     6. for r, then s: value >= 2^256 (33 bytes with a non-zero first byte), value = 0 or value >= n: SCALAR_RANGE.
 *     The compact forms start at check 6.  Then, s being high where s > (n - 1) / 2:  P2E_SIG_REQUIRE_LOW_S: HIGH_S;
 *     P2E_SIG_NORMALIZE_S: s := n - s, and in COMPACT65 v ^= 1 (the same key is recovered).
 * p2e_sig_encode_batch     the same forms.  DER writes the minimal encoding at stride P2E_SIG_DER_STRIDE (72), zeros
 *     behind it, and its length (8 .. 72) into out_len[i]; out_len is n bytes, required for DER and ignored otherwise.
 *     COMPACT65 needs v.  flags: 0 or P2E_SIG_NORMALIZE_S, as in decoding.  r or s zero or >= n: SCALAR_RANGE, zeros,
 *     out_len[i] = 0.
 * Each call is one kernel on the context's caller stream, one lane per element: no internal streams, no LDS, no scratch.
 * P2E_E_INVALID on a null pointer (other than the nullable ones), an unknown curve, form or flag combination; n == 0
 * returns 0.  Host pointers (the staging copy of data[offsets[0], offsets[n]) included), async mode, the current device
 * and failed calls behave as for p2e_hash_batch.  BUFFER OVERLAP (top of this file): wire forms and 32-byte arrays never
 * have the same stride, so no output of these four calls may lie on an input (r32 == data is refused for the compact forms;
 * for DER and for keys the extent of data is the caller's duty, checked with host pointers only). */
#define P2E_WIRE_OK 0
#define P2E_WIRE_BAD_LENGTH 1
#define P2E_WIRE_BAD_PREFIX 2
#define P2E_WIRE_COORD_RANGE 3
#define P2E_WIRE_NOT_ON_CURVE 4
#define P2E_WIRE_INFINITY 5
#define P2E_WIRE_DER_SYNTAX 6
#define P2E_WIRE_DER_INTEGER 7
#define P2E_WIRE_SCALAR_RANGE 8
#define P2E_WIRE_HIGH_S 9
#define P2E_SEC1_COMPRESSED 0     /* 02 / 03 || x, 33 bytes */
#define P2E_SEC1_UNCOMPRESSED 1   /* 04 || x || y, 65 bytes */
#define P2E_SIG_DER 0
#define P2E_SIG_COMPACT64 1       /* r || s */
#define P2E_SIG_COMPACT65 2       /* r || s || v */
#define P2E_SIG_REQUIRE_LOW_S 1u
#define P2E_SIG_NORMALIZE_S 2u
#define P2E_SIG_DER_STRIDE 72     /* bytes per element of an encoded DER batch: the longest strict signature */
long p2e_point_decode_batch(p2e_ctx *ctx, int curve, const uint8_t *data, const uint64_t *offsets /* n + 1 */,
                            uint8_t *px32, uint8_t *py32, size_t n, uint8_t *err);
long p2e_point_encode_batch(p2e_ctx *ctx, int curve, int form, const uint8_t *px32, const uint8_t *py32, uint8_t *out,
                            size_t n, uint8_t *err);
long p2e_sig_decode_batch(p2e_ctx *ctx, int curve, int form, unsigned flags, const uint8_t *data,
                          const uint64_t *offsets /* n + 1; DER only */, uint8_t *r32, uint8_t *s32,
                          uint8_t *v /* nullable */, size_t n, uint8_t *err);
long p2e_sig_encode_batch(p2e_ctx *ctx, int curve, int form, unsigned flags, const uint8_t *r32, const uint8_t *s32,
                          const uint8_t *v /* COMPACT65 only */, uint8_t *out, uint8_t *out_len /* DER only */, size_t n,
                          uint8_t *err);

/* ---- multi-scalar multiplication: out = sum_i k_i P_i over n points of one curve (P2E_CURVE_*), by the bucket
 * (Pippenger) method; the native many-point sum of curve/curve_msm.rs (msm_parallel / msm_execute) without its
 * precomputation.  All 32-byte values little-endian, element i at +32 i.
 *     k32      taken modulo the group order with one conditional subtraction, exactly as p2e_ecdsa_sign_batch takes its
 *              scalars (reduced, not flagged).
 *     points   (0, 0) is the neutral element -- the encoding p2e_ecdsa_public_key_batch and p2e_ecdsa_recover_batch write
 *              for flagged elements: it contributes nothing and is no error.  Any other point with a coordinate >= p, or
 *              not on the curve, is REJECTED: point_err[i] = 1 (0 for every other i; point_err is nullable), *status =
 *              P2E_MSM_BAD_POINT, both outputs zero, return value = the number of rejected points.  Nothing is summed
 *              "without" the rejected points.
 *     outputs  otherwise the canonical affine coordinates of the sum and P2E_MSM_OK, or, where the sum is the neutral
 *              element (n == 0 included), zeros and P2E_MSM_NEUTRAL; return value 0.  outx32 / outy32: 32 bytes each,
 *              4-byte aligned; status: one byte.  The outputs are written by every call that does not fail.
 *     window_bits   P2E_MSM_WINDOW_AUTO (the library chooses by n) or a width in [P2E_MSM_WINDOW_MIN, P2E_MSM_WINDOW_MAX];
 *              every width yields the same bytes.  n <= 2^24.
 * P2E_E_INVALID on a null pointer (other than point_err), an unknown curve, a window_bits outside the above, n > 2^24.
 * Seven launches on the context's caller stream (csrc/pmsm.hpp: digits and counts, scan, scatter, segment sums, bucket
 * sums, chunked bucket reduction, window combination with ONE inversion); scratch comes from the context, allocated on
 * first need, kept, and regrown when a later call needs more.  Host pointers, async mode (the return value then comes
 * from p2e_sync), the current device and failed calls behave as for the signing calls.
 * p2e_point_msm_plan (host only, no context): what a call with these arguments will use, as P2E_MSM_PLAN_WORDS 64-bit
 * words indexed by P2E_MSM_PLAN_*: the window width and the number of windows, buckets per window, the segment length
 * (a bucket is cut into segments of at most so many entries, one lane each), scratch bytes, and MAX_LANE_ADDITIONS: an
 * upper bound on the point operations (additions and doublings) any single lane performs in any launch of the call.
 * It depends on n and the plan only, never on the scalars.  Returns 0, or P2E_E_INVALID as above.
 * BUFFER OVERLAP: no output of p2e_point_msm may lie inside k32, px32 or py32 (every lane reads them; P2E_E_INVALID). */
#define P2E_MSM_WINDOW_AUTO 0
#define P2E_MSM_WINDOW_MIN 4
#define P2E_MSM_WINDOW_MAX 12
#define P2E_MSM_OK 0
#define P2E_MSM_NEUTRAL 1     /* the sum is the neutral element: zeros written */
#define P2E_MSM_BAD_POINT 2   /* at least one input point rejected: zeros written */
#define P2E_MSM_PLAN_WINDOW_BITS 0
#define P2E_MSM_PLAN_WINDOWS 1
#define P2E_MSM_PLAN_BUCKETS 2
#define P2E_MSM_PLAN_SEG 3
#define P2E_MSM_PLAN_SCRATCH_BYTES 4
#define P2E_MSM_PLAN_MAX_LANE_ADDITIONS 5
#define P2E_MSM_PLAN_WORDS 6
long p2e_point_msm(p2e_ctx *ctx, int curve, unsigned window_bits, const uint8_t *k32, const uint8_t *px32,
                   const uint8_t *py32, size_t n, uint8_t *outx32, uint8_t *outy32, uint8_t *status /* 1 byte */,
                   uint8_t *point_err /* nullable, n bytes */);
int p2e_point_msm_plan(int curve, size_t n, unsigned window_bits, uint64_t *plan /* P2E_MSM_PLAN_WORDS words */);

/* ---- per-element point arithmetic on either curve (P2E_CURVE_*): the native point layer under the calls above.
 *     p2e_point_mul_batch      out_i = k_i P_i          CurveScalar * ProjectivePoint (curve/curve_multiplication.rs:86-100),
 *                                                       on secp256k1 also the native glv_mul (curve/glv.rs:84-102)
 *     p2e_point_lincomb_batch  out_i = a_i G + b_i P_i  the verification equation with the caller's own scalars; P + t G
 *     p2e_point_add_batch      out_i = P_i + Q_i        the additions of curve/curve_adds.rs
 * All 32-byte values little-endian, element i at +32 i.
 *     scalars  taken modulo the group order with one conditional subtraction, exactly as p2e_ecdsa_sign_batch takes its
 *              scalars (reduced, not flagged).
 *     points   (0, 0) is the neutral element and a legal operand, as in p2e_point_msm -- what the key and recovery calls
 *              write for flagged elements, so the output of any call of this library can be fed in.  Any other point with a
 *              coordinate >= p, or not on the curve, is invalid.
 *     err[i]   all eight P2E_ERR_* bits are taken: a P2E_WIRE_* CODE, as for the four wire-form calls.  The first failing
 *              check of P2E_WIRE_COORD_RANGE, then P2E_WIRE_NOT_ON_CURVE (p2e_point_add_batch: P before Q; operands are
 *              checked whatever the scalars are); P2E_WIRE_INFINITY where the operands are fine and the RESULT is the
 *              neutral element, which 64 bytes cannot express (flagged as sk = 0 is by p2e_ecdsa_public_key_batch: an ECDH
 *              caller must see it).  Every non-zero code writes zeros to both outputs -- still the valid neutral operand
 *              of a next call.  Return value: the number of elements with a non-zero code.
 *     defined, none an error by itself: k = 0 (mod n), P neutral, a = 0, b = 0, a G = -b P, a G = b P (the last addition
 *              doubles), P = Q, P = -Q, P or Q neutral.
 *     plan     P2E_MUL_PLAN_AUTO (the library chooses), or a forced walk for k P / b P; all plans give the same bytes.
 *              P2E_MUL_PLAN_GLV on P2E_CURVE_P256 is P2E_E_INVALID.
 * P2E_E_INVALID on a null pointer, an unknown curve or plan; n == 0 returns 0.  One kernel per call on the context's caller
 * stream, one lane per element (csrc/point_arith.hpp): no internal streams, no scratch block, no table in LDS, nothing in the
 * private segment.  Host pointers, async mode (the return value then comes from p2e_sync), the current device and failed calls
 * behave as for the signing calls.  A zero Z at the end of a walk (impossible, see csrc/point_arith.hpp) would set
 * P2E_WIRE_INFINITY and write zeros.  BUFFER OVERLAP (top of this file): P += Q, P = k P and P = a G + b P in place are fine
 * (outx32 = px32, outy32 = py32), and so is outx32 = k32. */
#define P2E_MUL_PLAN_AUTO 0
#define P2E_MUL_PLAN_PLAIN 1   /* 128 two-bit windows over the 256-bit scalar (recover.hpp's walk), both curves */
#define P2E_MUL_PLAN_GLV 2     /* secp256k1 only: k = +-k1 +- k2 lambda, two 128-bit halves walked together */
long p2e_point_mul_batch(p2e_ctx *ctx, int curve, unsigned plan, const uint8_t *k32, const uint8_t *px32,
                         const uint8_t *py32, uint8_t *outx32, uint8_t *outy32, size_t n, uint8_t *err);
long p2e_point_lincomb_batch(p2e_ctx *ctx, int curve, unsigned plan, const uint8_t *a32, const uint8_t *b32,
                             const uint8_t *px32, const uint8_t *py32, uint8_t *outx32, uint8_t *outy32, size_t n,
                             uint8_t *err);
long p2e_point_add_batch(p2e_ctx *ctx, int curve, const uint8_t *px32, const uint8_t *py32, const uint8_t *qx32,
                         const uint8_t *qy32, uint8_t *outx32, uint8_t *outy32, size_t n, uint8_t *err);

/* ---- point tables on either curve: precompute the window table of m caller points once, then multiply and verify
 * without doublings (csrc/point_table.hpp; the reference's mul_precompute / mul_with_precomputation,
 * curve/curve_multiplication.rs:18-73, and MsmPrecomputation, curve/curve_msm.rs:19-54).  For batches with few distinct
 * points and many elements: a validator set, one CA key, the H of a Pedersen commitment, a static ECDH peer.
 *   table    Aff[m][66][16] in device memory, P2E_POINT_TABLE_BYTES_PER_POINT bytes per point: entry [j][w][d] =
 *            d 16^w P_j as 64 bytes (x then y, little-endian, canonical) for d = 1 .. 15; slot 0 is a copy of slot 1 --
 *            for P_j = G exactly the generator's table of the signing calls.  Built on the device.
 *   handle   p2e_point_table is an opaque object; the prototypes spell its pointer `void *` (p2e_point_table is a typedef
 *            of void), so `p2e_point_table *t; p2e_point_table_create(..., &t);` is what a caller writes.  A table
 *            belongs to the device of the context that made it and may be used by any context of that device.
 *   create   1 <= m <= P2E_POINT_TABLE_MAX_POINTS.  point_err[j] (nullable) is the P2E_WIRE_* code of point j, first
 *            failing check of: (0, 0) P2E_WIRE_INFINITY (the neutral element has no table), a coordinate >= p
 *            P2E_WIRE_COORD_RANGE, off the curve P2E_WIRE_NOT_ON_CURVE.  If any point is rejected nothing is built,
 *            *out = NULL and the return value is the number of rejected points (p2e_point_msm's rule); otherwise 0 and
 *            *out is set.  SYNCHRONOUS even on a P2E_CTX_ASYNC context (it counts rejections).  Honours
 *            P2E_CTX_HOST_POINTERS (px32, py32, point_err), restores the caller's current device.  P2E_E_NOMEM when the
 *            allocation fails (the context stays usable); P2E_E_INVALID on a null pointer, an unknown curve or a bad m.
 *   destroy  waits for the context's stream first, so a queued call cannot outlive its table.  NULL table: no-op.
 *   read_window  the 16 entries x 64 bytes of window w (0 .. 65) of point j to HOST memory (synchronous): for tests and
 *            for callers that persist a table.
 *   the three batch calls   idx == NULL means point 0 for every element; idx[i] >= m gives err[i] = P2E_WIRE_BAD_INDEX,
 *            zeros in the outputs, and no table word is read for that lane.  Scalars are taken modulo n with one
 *            conditional subtraction; outputs are canonical affine coordinates.  One kernel per call on the caller's
 *            stream, one lane per element: no internal streams, no LDS table, nothing in the private segment.  Host
 *            pointers, async mode, n == 0, null pointers (only idx may be null) and failed calls behave as for the
 *            point-arithmetic calls above.  The return value counts the non-zero err bytes.  BUFFER OVERLAP: outx32 on a
 *            scalar array is fine; point_err of create may not lie on the points.
 *     p2e_point_table_mul_batch      out_i = k_i T[idx_i]; k = 0 (mod n): zeros and P2E_WIRE_INFINITY.  Byte for byte
 *            what p2e_point_mul_batch writes for (k_i, P_idx_i) under every plan.
 *     p2e_point_table_lincomb_batch  out_i = a_i G + b_i T[idx_i]: two window sums and one complete addition (a G = b P
 *            doubles, a G = -b P is P2E_WIRE_INFINITY, either half may be empty).  The bytes of p2e_point_lincomb_batch.
 *     p2e_ecdsa_verify_table_batch   the textbook verdict of curve/ecdsa.rs:42-62 under key T[idx_i].  err[i]:
 *            P2E_WIRE_BAD_INDEX, then P2E_WIRE_SCALAR_RANGE for r = 0, r >= n, s = 0 or s >= n (r, s are not reduced,
 *            msg is).  Where err[i] = 0: c = 1 / s, X = (msg c) G + (r c) P, valid[i] = 1 iff X is not the neutral
 *            element and X.x mod n == r.  valid[i] = 0 wherever err[i] != 0; an invalid signature is NOT counted. */
#define P2E_WIRE_BAD_INDEX 10
#define P2E_POINT_TABLE_MAX_POINTS 65536
#define P2E_POINT_TABLE_BYTES_PER_POINT 67584
typedef void p2e_point_table;
long p2e_point_table_create(p2e_ctx *ctx, int curve, const uint8_t *px32, const uint8_t *py32, size_t m,
                            uint8_t *point_err /* nullable, m bytes */, void **out);
void p2e_point_table_destroy(p2e_ctx *ctx, void *table);
long p2e_point_table_num_points(const void *table);
int p2e_point_table_curve(const void *table);
int p2e_point_table_read_window(p2e_ctx *ctx, const void *table, size_t j, int w, uint8_t *out1024);
long p2e_point_table_mul_batch(p2e_ctx *ctx, const void *table, const uint32_t *idx /* nullable */, const uint8_t *k32,
                               uint8_t *outx32, uint8_t *outy32, size_t n, uint8_t *err);
long p2e_point_table_lincomb_batch(p2e_ctx *ctx, const void *table, const uint32_t *idx /* nullable */,
                                   const uint8_t *a32, const uint8_t *b32, uint8_t *outx32, uint8_t *outy32, size_t n,
                                   uint8_t *err);
long p2e_ecdsa_verify_table_batch(p2e_ctx *ctx, const void *table, const uint32_t *idx /* nullable */,
                                  const uint8_t *msg32, const uint8_t *r32, const uint8_t *s32, size_t n, uint8_t *err,
                                  uint8_t *valid);

/* ---- BIP-340 Schnorr signatures on secp256k1 (csrc/schnorr.hpp): x-only keys, default signing, the per-element verdict
 * and the standard's batch verification.  The curve is secp256k1 alone (no curve argument, as p2e_eth_address_batch).
 *   bytes    EVERY argument of these calls is the standard's byte string, BIG-endian (this header's rule for wire forms:
 *            these objects exist only in wire form and the tagged hashes consume exactly those bytes): sk32, msg32, aux32,
 *            the x-only pk32 (element i at +32 i) and sig64 = bytes(r) || bytes(s) (element i at +64 i); every array
 *            4-byte aligned.  msg32 is 32 opaque bytes, never reduced.  The only little-endian values are the px32, py32
 *            that p2e_xonly_decode_batch writes.
 *   err[i]   a P2E_WIRE_* CODE: the first failing check in the order given below; a flagged element writes zeros to all
 *            its outputs.  The return value counts the non-zero err bytes.  Null pointers, n == 0 (returns 0), host
 *            pointers, async mode, the current device, failed calls and BUFFER OVERLAP behave as for the point-arithmetic
 *            calls (pk32 = sk32 and px32 = pk32 are fine; sig64 has another stride than every input; verdict may not lie
 *            inside an input of the aggregate check).
 *   p2e_schnorr_public_key_batch   d = int(sk); d = 0 or d >= n: P2E_WIRE_SCALAR_RANGE (the standard fails here, nothing is
 *            reduced).  Otherwise pk = bytes(x(d G)).
 *   p2e_schnorr_sign_batch   the standard's "Default Signing"; all pointers required.  The range check of d as above; P = d G,
 *            d := n - d where P.y is odd; t = bytes(d) xor H_aux(aux); k' = int(H_nonce(t || bytes(P.x) || msg)) mod n,
 *            k' = 0: P2E_WIRE_INFINITY; R = k' G, k = n - k' where R.y is odd; e = int(H_challenge(bytes(R.x) || bytes(P.x)
 *            || msg)) mod n; sig = bytes(R.x) || bytes((k + e d) mod n).  The verification of the fresh signature that the
 *            standard recommends as a last step is NOT done: a caller that wants it runs p2e_schnorr_verify_batch.  d, t,
 *            k' and k never leave the lane's registers.
 *   p2e_schnorr_verify_batch   err[i], in order: pk >= p P2E_WIRE_COORD_RANGE; pk^3 + 7 not a square P2E_WIRE_NOT_ON_CURVE;
 *            r >= p P2E_WIRE_COORD_RANGE; s >= n P2E_WIRE_SCALAR_RANGE.  Where err[i] = 0: P = lift_x(pk) (even y), e as
 *            above, X = s G + (n - e) P; valid[i] = 1 iff X is not the neutral element, X.y is even and X.x == r.  A
 *            well-formed but wrong signature -- an r that is on no curve point and s G = e P among them -- has err = 0,
 *            valid = 0 and is NOT counted.  valid[i] = 0 wherever err[i] != 0.
 *   p2e_xonly_decode_batch   lift_x(pk) with even y as the library's little-endian affine point (px32, py32): the bridge to
 *            p2e_point_lincomb_batch (Taproot's P + t G), p2e_point_table_create, p2e_point_msm and
 *            p2e_point_encode_batch.  err[i]: the first two checks of the verifier.
 *   p2e_schnorr_verify_aggregate   the standard's "Batch Verification": ONE verdict byte for the whole batch.
 *            *verdict = 1 iff no element is flagged and
 *                (sum a_i s_i mod n) G + sum a_i (-R_i) + sum (a_i e_i mod n) (-P_i)   is the neutral element,
 *            R_i = lift_x(r_i), P_i = lift_x(pk_i), with the randomisers fixed here so that every implementation gives the
 *            same bytes: a_i = the first 16 bytes of SHA-256(seed32 || LE64(i)) read as a big-endian integer, 0 replaced
 *            by 1; no a_i is fixed at 1.  seed32 is the CALLER's and must be unpredictable to whoever produced the
 *            signatures -- fresh randomness, or a hash of the whole batch (every msg, pk and sig); with a seed the signer
 *            knows, cancelling errors pass.  The library neither draws nor checks it.
 *            err[i] (nullable): the verifier's four checks, then r^3 + 7 not a square: P2E_WIRE_NOT_ON_CURVE (the lift of r
 *            must exist here).  A flagged element contributes the neutral element and makes the verdict 0.  Return value:
 *            the number of flagged elements.  n == 0 gives verdict 1 (no pointer but err may be null even then);
 *            2 n + 1 > 2^24 is P2E_E_INVALID.  window_bits is p2e_point_msm's, taken for 2 n + 1 points.
 *            One preparation kernel (one lane per signature) and one small
 *            finishing kernel write the 2 n + 1 terms into a scratch block of the context (kept, regrown on need), then
 *            p2e_point_msm's seven launches and one verdict kernel run on the same stream; verdict is a device pointer
 *            unless the context stages host pointers.  There is NO fallback that locates a bad element: on verdict 0 the
 *            caller runs p2e_schnorr_verify_batch on the batch. */
long p2e_schnorr_public_key_batch(p2e_ctx *ctx, const uint8_t *sk32, uint8_t *pk32, size_t n, uint8_t *err);
long p2e_schnorr_sign_batch(p2e_ctx *ctx, const uint8_t *msg32, const uint8_t *sk32, const uint8_t *aux32, uint8_t *sig64,
                            size_t n, uint8_t *err);
long p2e_schnorr_verify_batch(p2e_ctx *ctx, const uint8_t *msg32, const uint8_t *pk32, const uint8_t *sig64, size_t n,
                              uint8_t *err, uint8_t *valid);
long p2e_xonly_decode_batch(p2e_ctx *ctx, const uint8_t *pk32, uint8_t *px32, uint8_t *py32, size_t n, uint8_t *err);
long p2e_schnorr_verify_aggregate(p2e_ctx *ctx, const uint8_t *msg32, const uint8_t *pk32, const uint8_t *sig64, size_t n,
                                  const uint8_t *seed32, unsigned window_bits, uint8_t *verdict,
                                  uint8_t *err /* nullable */);

/* ---- BIP-32 key derivation and Bitcoin key hashes on secp256k1: where a wallet's keys come from (one extended key, its
 * children) and where they go (HASH160, the payload of P2PKH / P2WPKH and the source of the BIP-32 fingerprint).  Defined by
 * BIP-32, FIPS 180-4 (SHA-512, SHA-256), RFC 2104 (HMAC) and the RIPEMD-160 paper.  The curve is secp256k1 alone (no curve
 * argument, as p2e_eth_address_batch).  An extended key on the device becomes n child keys, then n key hashes, and with the
 * signing, encoding and verifying calls signatures and witnesses, without visiting the host.
 *   bytes    keys and coordinates (sk32, pkx32, pky32 and the par_* ones) are this library's 32-byte LITTLE-endian values, so
 *            they chain into every other call.  Chain codes (cc32) are 32 bytes in the standard's order.  index is a uint32_t
 *            array; index >= 2^31 is a hardened child.  Hashes are in the order their standard defines.  Every array is 4-byte
 *            aligned but seed (any alignment, stride seed_len) and the data of p2e_hash160_batch (any alignment); both are read
 *            as p2e_hash_batch reads its data: aligned 4-byte words, and only words that hold a byte of the lane's element.
 *   parents  n_parents is 1 or n, anything else is P2E_E_INVALID.  With 1 every element derives from parent 0: the scan of
 *            one extended key (for n == 1 the two meanings coincide).  With n the children may be written over the
 *            parents, chain codes included; with 1 (and n > 1) an output on a parent array is P2E_E_INVALID: lane 0 would
 *            store child 0 where the other lanes have yet to read the parent (BUFFER OVERLAP at the top of this file).
 *   err[i]   a P2E_WIRE_* CODE: the first failing check in the order given below.  A flagged element writes zeros to ALL its
 *            outputs, the chain code included.  BIP-32's "proceed with the next index" is NOT done: the code tells the caller.
 *   p2e_bip32_master_batch   I = HMAC-SHA512(key = "Bitcoin seed", seed_i), seed_i = seed[seed_len i, seed_len (i + 1)), one
 *            seed_len of 16 .. 64 per call (anything else: P2E_E_INVALID).  I_L = 0 or I_L >= n: P2E_WIRE_SCALAR_RANGE.
 *            sk = I_L, cc = I_R.
 *   p2e_bip32_ckd_priv_batch   CKDpriv.  In order: parent k = 0 or k >= n: P2E_WIRE_SCALAR_RANGE (not reduced: BIP-32 keys
 *            lie in [1, n - 1]).  data = 00 || ser256(k) || ser32(index) for a hardened index, serP(k G) || ser32(index)
 *            otherwise (the lane walks the generator's table: the cost of p2e_ecdsa_public_key_batch).
 *            I = HMAC-SHA512(key = cc, data); I_L >= n: P2E_WIRE_SCALAR_RANGE; k_child = I_L + k mod n, 0:
 *            P2E_WIRE_INFINITY.  I_L = 0 is valid and computed.  cc_child = I_R.
 *   p2e_bip32_ckd_pub_batch   CKDpub.  In order: index >= 2^31: P2E_WIRE_BAD_INDEX (a public parent has no hardened child);
 *            parent (0, 0): P2E_WIRE_INFINITY; a parent coordinate >= p: P2E_WIRE_COORD_RANGE; parent off the curve:
 *            P2E_WIRE_NOT_ON_CURVE; I = HMAC-SHA512(key = cc, serP(K) || ser32(index)), I_L >= n: P2E_WIRE_SCALAR_RANGE;
 *            K_child = I_L G + K, the neutral element: P2E_WIRE_INFINITY.  I_L = 0 (child = parent) and I_L G = K (a
 *            doubling) are computed, not flagged.  The point and chain code are those CKDpriv's child has.
 *   p2e_key_hash160_batch   out20[20 i ..] = RIPEMD-160(SHA-256(the SEC1 string of (pkx, pky))), form P2E_SEC1_COMPRESSED
 *            (33 bytes) or P2E_SEC1_UNCOMPRESSED (65 bytes); an unknown form is P2E_E_INVALID.  Mirrors p2e_eth_address_batch:
 *            nothing is checked, and where err_in[i] != 0 (nullable) twenty zero bytes are written.  Returns 0.  Bytes 0 .. 3
 *            of the compressed form's output are the BIP-32 fingerprint of the key.
 *   p2e_hash160_batch   out20[20 i ..] = RIPEMD-160(SHA-256(message i)); messages, offsets, alignment, empty and reversed
 *            elements, the return value and host staging are exactly p2e_hash_batch's.
 * Each call is one kernel on the context's caller stream, one lane per element: no internal streams, no LDS, no scratch;
 * the secrets (parent key, I_L, child key) live in registers only.  Return value: the number of flagged elements
 * (p2e_hash160_batch: of reversed elements); P2E_E_INVALID on a null pointer (other than err_in) or a bad argument; n == 0
 * returns 0.  Host pointers, async mode, the current device and failed calls behave as for the signing calls. */
long p2e_bip32_master_batch(p2e_ctx *ctx, const uint8_t *seed, size_t seed_len, uint8_t *sk32, uint8_t *cc32, size_t n,
                            uint8_t *err);
long p2e_bip32_ckd_priv_batch(p2e_ctx *ctx, const uint8_t *par_sk32, const uint8_t *par_cc32, size_t n_parents,
                              const uint32_t *index, uint8_t *sk32, uint8_t *cc32, size_t n, uint8_t *err);
long p2e_bip32_ckd_pub_batch(p2e_ctx *ctx, const uint8_t *par_pkx32, const uint8_t *par_pky32, const uint8_t *par_cc32,
                             size_t n_parents, const uint32_t *index, uint8_t *pkx32, uint8_t *pky32, uint8_t *cc32,
                             size_t n, uint8_t *err);
long p2e_key_hash160_batch(p2e_ctx *ctx, unsigned form, const uint8_t *pkx32, const uint8_t *pky32,
                           const uint8_t *err_in /* nullable */, uint8_t *out20, size_t n);
long p2e_hash160_batch(p2e_ctx *ctx, const uint8_t *data, const uint64_t *offsets, uint8_t *out20, size_t n);

/* ---- PBKDF2-HMAC-SHA512 and BIP-39 seeds (csrc/kdf.hpp): the step in front of p2e_bip32_master_batch.  What a wallet holds
 * is a mnemonic sentence and a passphrase; seed = PBKDF2-HMAC-SHA512(sentence, "mnemonic" || passphrase, 2048, 64), about
 * 4 100 SHA-512 compressions where a hardened child costs four.  Defined by RFC 8018 5.2, RFC 2104, FIPS 180-4 and BIP-39.
 *   count    The batch size of these two calls is named `count`, as for the Taproot, silent-payment and MuSig2 calls and for
 *            the same reason: tests/test_overlap_cpu.py derives its list of per-element calls from the declarations with a
 *            parameter named n or m, so no parameter here is named n or m.  They carry their span table in
 *            tests/test_kdf_cpu.py.  BUFFER OVERLAP (top of this file) holds in full and there is NO in-place form: an output
 *            may touch no input.
 *   data     password, salt, mnemonic and passphrase are laid out exactly as the data of p2e_hash_batch: one concatenated
 *            buffer of any alignment, element i = [offsets[i], offsets[i + 1]); read as aligned 4-byte words, and only words
 *            that hold a byte of the lane's own element.  With host pointers the bytes [offsets[0], offsets[last]) are staged
 *            and may touch no output.  Bytes are taken as given: UTF-8 NFKD normalisation is the caller's job, and BIP-39's
 *            wordlist and checksum are not looked at (its seed derivation does not look at them either).
 *   broadcast   n_passwords, n_salts, n_mnemonics are 1 or count; with 1 < count every lane uses element 0 -- one mnemonic
 *            against many passphrases, many mnemonics against one passphrase.  n_passphrases is 0, 1 or count; 0 goes with
 *            passphrase == NULL and pp_offsets == NULL and means the empty passphrase.  Anything else is P2E_E_INVALID.
 *   p2e_pbkdf2_hmac_sha512_batch   The HMAC key is the password itself if it is at most 128 bytes, else its SHA-512 digest.
 *            U_1 = HMAC(P, S || 00 00 00 01), U_j = HMAC(P, U_{j-1}), T = U_1 ^ ... ^ U_iterations; dk[dk_len i ..] = the
 *            first dk_len bytes of T.  dk_len is a multiple of 4 in 4 .. 64 (one block of output), dk is 4-byte aligned.
 *            iterations == 0, iterations > P2E_PBKDF2_MAX_ITERATIONS or a bad dk_len is P2E_E_INVALID.  The call is ONE
 *            kernel whose running time grows with `iterations` -- 2 (iterations - 1) + 4 .. 8 compressions per lane, nothing
 *            else shares the launch and it cannot be interrupted --, which is why there is a cap: 2^20 iterations are about
 *            500 times a BIP-39 seed.
 *   p2e_bip39_seed_batch   The same kernel with the eight bytes "mnemonic" in front of the salt (a constant of the kernel,
 *            nothing is concatenated on the host), 2048 iterations and 64 bytes out: seed64[64 i ..] is what
 *            p2e_bip32_master_batch takes with seed_len = 64.
 *   err[i]   P2E_WIRE_BAD_LENGTH for a reversed offset pair or a length >= 2^32 of either operand (a broadcast operand
 *            flags every element alike).  A flagged element writes zeros to all its output bytes and runs no iteration.  The
 *            return value counts the flagged elements; count == 0 returns 0.  Null pointers, host pointers, async mode, the
 *            current device and failed calls behave as for the BIP-32 calls.
 * One kernel on the context's caller stream, one lane per element: no internal streams, no LDS, no scratch; passwords, key
 * states and every U_j live in registers only. */
#define P2E_PBKDF2_MAX_ITERATIONS (1u << 20)
long p2e_pbkdf2_hmac_sha512_batch(p2e_ctx *ctx, const uint8_t *password, const uint64_t *pw_offsets /* n_passwords + 1 */,
                                  size_t n_passwords /* 1 or count */, const uint8_t *salt,
                                  const uint64_t *salt_offsets /* n_salts + 1 */, size_t n_salts /* 1 or count */,
                                  uint32_t iterations, size_t dk_len, uint8_t *dk, size_t count, uint8_t *err);
long p2e_bip39_seed_batch(p2e_ctx *ctx, const uint8_t *mnemonic, const uint64_t *mn_offsets /* n_mnemonics + 1 */,
                          size_t n_mnemonics /* 1 or count */, const uint8_t *passphrase /* nullable */,
                          const uint64_t *pp_offsets /* nullable with it */, size_t n_passphrases /* 0, 1 or count */,
                          uint8_t *seed64, size_t count, uint8_t *err);

/* ---- Taproot (BIP-341) on secp256k1 (csrc/taproot.hpp): what lies between an x-only key and a BIP-340 signature.  An
 * xpub scan on the device (p2e_bip32_ckd_pub_batch) becomes Taproot output keys -- with p2e_point_encode_batch /
 * p2e_key_hash160_batch the witness programs --, a derived secret key becomes the key p2e_schnorr_sign_batch signs a
 * key-path spend with, and a batch of script-path spends is checked against its output keys, without visiting the host.
 *   count    The batch size of these five calls is named `count`, NOT `n`, on purpose: tests/test_overlap_cpu.py derives its
 *            list of per-element calls from the declarations that return long and have a parameter named n or m, and keeps
 *            one row per call in a table of its own; these calls carry their span table in tests/test_taproot_cpu.py until
 *            the rows are folded in (and the parameter renamed).  BUFFER OVERLAP (top of this file) holds for them in full.
 *   bytes    as for the Schnorr calls: every key, hash and tweak is the standard's BIG-endian 32-byte string, element i at
 *            +32 i, every array 4-byte aligned -- but `script` (any alignment; read as p2e_hash_batch reads its data: aligned
 *            4-byte words, and only words that hold a byte of the lane's own script) and the one-byte arrays.
 *   tagged hashes   H_tag(x) = SHA256(SHA256(tag) || SHA256(tag) || x) for "TapLeaf", "TapBranch" and "TapTweak".
 *   err[i]   a P2E_WIRE_* CODE: the first failing check in the order given below; a flagged element writes zeros to all its
 *            outputs.  The return value counts the flagged elements; count == 0 returns 0.  Null pointers, host pointers,
 *            async mode, the current device and failed calls behave as for the Schnorr calls.  In place, exactly:
 *            out_pk32 = pk32, out_sk32 = sk32 and root32 = leaf32 are fine (every body reads all of element i's inputs
 *            before its first store); every other overlap of an output is refused as BUFFER OVERLAP says.
 *   p2e_taproot_leaf_hash_batch   script i = script[offsets[i], offsets[i + 1]).  In order: leaf_version[i] odd:
 *            P2E_WIRE_BAD_PREFIX (bit 0 is the control block's parity bit); offsets[i + 1] < offsets[i] or a length >= 2^32:
 *            P2E_WIRE_BAD_LENGTH.  Otherwise leaf32 = H_TapLeaf(version || compact_size(length) || script), the compact
 *            size being one byte below 253, fd + 2 little-endian bytes up to 0xffff, fe + 4 bytes above.  With host
 *            pointers the bytes script[offsets[0], offsets[count]) are staged, as for p2e_hash_batch.
 *   p2e_taproot_merkle_root_batch   node j of element i is at path32 + 32 (i max_depth + j), j < depth[i].  max_depth > 128
 *            is P2E_E_INVALID; with max_depth == 0 path32 may be null.  depth[i] > max_depth: P2E_WIRE_BAD_LENGTH.
 *            k = leaf; for each node e: k = H_TapBranch(min(k, e) || max(k, e)), compared as 32-byte strings; root32 = k
 *            (the leaf itself at depth 0).  Two compressions per level.
 *   p2e_taproot_tweak_pubkey_batch   BIP-341 taproot_tweak_pubkey.  In order: pk >= p: P2E_WIRE_COORD_RANGE; pk^3 + 7 not a
 *            square: P2E_WIRE_NOT_ON_CURVE; t = int(H_TapTweak(pk || root)) -- with root32 == NULL nothing is appended: the
 *            key-path-only output of BIP-86 --, t >= n: P2E_WIRE_SCALAR_RANGE (not reduced); Q = lift_x(pk) + t G, the
 *            neutral element: P2E_WIRE_INFINITY.  out_pk32 = bytes(x(Q)), out_parity = y(Q) & 1.  t G = P (a doubling) and
 *            t = 0 are computed, not flagged.
 *   p2e_taproot_tweak_seckey_batch   BIP-341 taproot_tweak_seckey.  d = 0 or d >= n: P2E_WIRE_SCALAR_RANGE; P = d G,
 *            d := n - d where P.y is odd; t as above over bytes(P.x), t >= n: P2E_WIRE_SCALAR_RANGE; out_sk = (d + t) mod n,
 *            zero: P2E_WIRE_INFINITY.  p2e_schnorr_public_key_batch(out_sk32) equals the out_pk32 of the public call.  d, t
 *            and the sum never leave the lane's registers but for out_sk32.
 *   p2e_taproot_verify_commitment_batch   BIP-341's script-path rule behind the leaf hash, one kernel: Merkle walk, tweak,
 *            point, compare.  In order: out_parity[i] > 1: P2E_WIRE_BAD_PREFIX; depth[i] > max_depth: P2E_WIRE_BAD_LENGTH
 *            (max_depth and path32 as above); the two key checks of the pubkey call on the internal key pk32; t >= n and a
 *            neutral Q as there.  Where err[i] = 0: valid[i] = 1 iff bytes(x(Q)) == out_pk32[i] and y(Q) & 1 ==
 *            out_parity[i].  An out_pk32 >= p simply never matches and is not flagged; a well-formed mismatch has err = 0,
 *            valid = 0 and is NOT counted.  valid[i] = 0 wherever err[i] != 0.
 * Each call is one kernel on the context's caller stream, one lane per element: no internal streams, no LDS, no scratch. */
long p2e_taproot_leaf_hash_batch(p2e_ctx *ctx, const uint8_t *leaf_version, const uint8_t *script, const uint64_t *offsets,
                                 uint8_t *leaf32, size_t count, uint8_t *err);
long p2e_taproot_merkle_root_batch(p2e_ctx *ctx, const uint8_t *leaf32, const uint8_t *path32, const uint8_t *depth,
                                   size_t max_depth, uint8_t *root32, size_t count, uint8_t *err);
long p2e_taproot_tweak_pubkey_batch(p2e_ctx *ctx, const uint8_t *pk32, const uint8_t *root32 /* nullable */,
                                    uint8_t *out_pk32, uint8_t *out_parity, size_t count, uint8_t *err);
long p2e_taproot_tweak_seckey_batch(p2e_ctx *ctx, const uint8_t *sk32, const uint8_t *root32 /* nullable */,
                                    uint8_t *out_sk32, size_t count, uint8_t *err);
long p2e_taproot_verify_commitment_batch(p2e_ctx *ctx, const uint8_t *out_pk32, const uint8_t *out_parity,
                                         const uint8_t *pk32, const uint8_t *leaf32, const uint8_t *path32,
                                         const uint8_t *depth, size_t max_depth, size_t count, uint8_t *err, uint8_t *valid);

/* ---- Silent payments (BIP-352) on secp256k1 (csrc/sp.hpp): the sender's output keys and the receiver's scan.  A receiver does
 * one ECDH per eligible transaction -- a general-point multiplication by the scan key --, then per step k a tagged hash, a
 * fixed-base walk, an addition and a compare against the transaction's outputs; p2e_sp_scan_batch does all of it for one
 * transaction per lane without visiting the host.
 *   count    The batch size of these four calls is named `count`, as for the Taproot calls and for the same reason:
 *            no parameter is named n or m.  They carry their span table in tests/test_sp_cpu.py.  BUFFER OVERLAP holds in full.
 *   bytes    TWO orders, by where a value comes from.  Points and the secret scalars of the key layer are the library's
 *            LITTLE-endian 32-byte values, as in the BIP-32 calls (they chain with p2e_bip32_*, p2e_point_add_batch,
 *            p2e_ecdsa_public_key_batch): ax32 / ay32, scan_sk32, a_sk32, spend_pkx32 / spend_pky32, scan_pkx32 / scan_pky32,
 *            label_x32 / label_y32.  Everything BIP-352 defines as a byte string or a hash is the standard's BIG-endian
 *            string, as in the Schnorr and Taproot calls: outpoint36 (txid || vout, as serialised), input_hash32, the x-only
 *            outputs32, hit_tweak32 and label_tweak32.  label_index, k and hit_output are uint32 arrays; every array is
 *            4-byte aligned but the one-byte ones.
 *   hashes   H_tag(x) = SHA256(SHA256(tag) || SHA256(tag) || x) for "BIP0352/Inputs", "BIP0352/SharedSecret", "BIP0352/Label".
 *            serP is the 33-byte compressed point, ser32 four big-endian bytes, ser256 thirty-two.
 *              input_hash = int(H_Inputs(outpoint36 || serP(A)))
 *              S   = (input_hash b_scan mod n) A   for the receiver,   (input_hash a mod n) B_scan   for the sender
 *              t_k = int(H_SharedSecret(serP(S) || ser32(k))),   P_k = B_spend + t_k G,   the output is bytes(x(P_k))
 *              l_m = int(H_Label(ser256(b_scan) || ser32(m))),   L_m = l_m G   (B_spend + L_m is p2e_point_add_batch)
 *   err[i]   a P2E_WIRE_* CODE: the first failing check in the order given below; a flagged element writes zeros to all its
 *            outputs (n_hits = 0).  The return value counts the flagged elements; count == 0 returns 0.  Null pointers, host
 *            pointers, async mode, the current device and failed calls behave as for the Taproot calls.  An argument shared
 *            by the batch (one element) is checked by every lane and flags every element alike.  The checks: a secret scalar
 *            0 or >= n: P2E_WIRE_SCALAR_RANGE (never reduced); a point (0, 0): P2E_WIRE_INFINITY; a coordinate >= p:
 *            P2E_WIRE_COORD_RANGE; a point off the curve: P2E_WIRE_NOT_ON_CURVE.
 *   p2e_sp_input_hash_batch   the point checks on A (a neutral A is P2E_WIRE_INFINITY: BIP-352 skips such a transaction),
 *            then a hash of 0 or >= n: P2E_WIRE_SCALAR_RANGE.  In place: input_hash32 = ax32.
 *   p2e_sp_label_batch   scan_sk32 is ONE element.  The scan key check, then l_m = 0 or >= n: P2E_WIRE_SCALAR_RANGE.
 *            label_tweak32 = bytes(l_m), (label_x32, label_y32) = L_m.  No output may lie on label_index.
 *   p2e_sp_send_batch   In order: a_sk32, input_hash32 (0 or >= n: P2E_WIRE_SCALAR_RANGE), B_scan, B_spend; t_k = 0 or >= n:
 *            P2E_WIRE_SCALAR_RANGE; P_k neutral: P2E_WIRE_INFINITY.  out_pk32 = bytes(x(P_k)).  a, the product and S never
 *            leave the lane's registers.  In place: out_pk32 = input_hash32.
 *   p2e_sp_scan_batch   scan_sk32, spend_pkx32, spend_pky32 are ONE element each, label_x32 / label_y32 n_labels elements
 *            (n_labels <= P2E_SP_MAX_LABELS; with n_labels == 0 both may be null).  Transaction i has the outputs
 *            outputs32 + 32 j for out_offsets[i] <= j < out_offsets[i + 1] (out_offsets: count + 1 elements, in OUTPUTS, not
 *            bytes).  In order: the scan key, B_spend, labels 0 .. n_labels - 1 (these flag every element); A_i; input_hash32[i]
 *            if given (0 or >= n: P2E_WIRE_SCALAR_RANGE); out_offsets[i + 1] < out_offsets[i] or more than 2^32 - 1 outputs:
 *            P2E_WIRE_BAD_LENGTH; then per step t_k = 0 or >= n: P2E_WIRE_SCALAR_RANGE, P_k neutral: P2E_WIRE_INFINITY (BIP-352
 *            fails there too; a flag at a step k > 0 drops the hits already recorded).  With input_hash32 == NULL the scalar
 *            is b_scan alone: A is then the "tweak data" input_hash A that indexes serve to light clients.
 *            The scan loop of one transaction: k = 0; the candidates of step k are P_k, then P_k + L_j for j = 0 .. n_labels - 1
 *            (this covers BIP-352's label tests on output - P_k and -output - P_k); output o matches candidate C iff
 *            x(C) == o.  The hit is the lowest-index output not yet recorded that matches a candidate, under its first matching
 *            candidate; it becomes hit number k, k += 1, and the loop goes on unless k == max_hits.  Without a hit it stops.  A
 *            neutral candidate matches nothing, an output >= p never matches; neither is flagged.
 *            n_hits[i] <= max_hits (equal: the loop stopped at the cap); hit_output[max_hits i + h] the output's index within
 *            the transaction; hit_label[..] 0 for unlabelled, j + 1 for label j; hit_tweak32 + 32 (max_hits i + h) = bytes(t_h)
 *            (the spending key b_spend + t_h (+ l_j) is the host's addition).  Unused slots are zero.  max_hits outside
 *            1 .. P2E_SP_MAX_HITS or n_labels > P2E_SP_MAX_LABELS: P2E_E_INVALID.  No in-place form.  outputs32 has an extent
 *            only the device knows (BUFFER OVERLAP 5); with host pointers the bytes outputs32[32 out_offsets[0],
 *            32 out_offsets[count]) are staged, and an offset outside that range is P2E_E_INVALID.
 * Each call is one kernel on the context's caller stream, one lane per element: no internal streams, no scratch. */
#define P2E_SP_MAX_HITS 8
#define P2E_SP_MAX_LABELS 16
long p2e_sp_input_hash_batch(p2e_ctx *ctx, const uint8_t *outpoint36, const uint8_t *ax32, const uint8_t *ay32,
                             uint8_t *input_hash32, size_t count, uint8_t *err);
long p2e_sp_label_batch(p2e_ctx *ctx, const uint8_t *scan_sk32 /* 1 element */, const uint32_t *label_index,
                        uint8_t *label_tweak32, uint8_t *label_x32, uint8_t *label_y32, size_t count, uint8_t *err);
long p2e_sp_send_batch(p2e_ctx *ctx, const uint8_t *a_sk32, const uint8_t *input_hash32, const uint8_t *scan_pkx32,
                       const uint8_t *scan_pky32, const uint8_t *spend_pkx32, const uint8_t *spend_pky32, const uint32_t *k,
                       uint8_t *out_pk32, size_t count, uint8_t *err);
long p2e_sp_scan_batch(p2e_ctx *ctx, const uint8_t *scan_sk32 /* 1 */, const uint8_t *spend_pkx32 /* 1 */,
                       const uint8_t *spend_pky32 /* 1 */, const uint8_t *label_x32, const uint8_t *label_y32, size_t n_labels,
                       const uint8_t *ax32, const uint8_t *ay32, const uint8_t *input_hash32 /* nullable */,
                       const uint8_t *outputs32, const uint64_t *out_offsets /* count + 1, in outputs */, size_t max_hits,
                       uint8_t *n_hits, uint32_t *hit_output, uint8_t *hit_label, uint8_t *hit_tweak32, size_t count,
                       uint8_t *err);

/* ---- a P + b Q per element on either curve, and discrete-log-equality proofs (BIP-374) on secp256k1 (csrc/point_arith.hpp,
 * csrc/dleq.hpp).  A collaborative silent-payment sender (several signers, a hardware signer, PSBTs under BIP-375) publishes
 * its ECDH share C = a B_scan with a proof that C uses the a of its public key A = a G; the coordinator checks every proof
 * before it adds the shares.  The verifier's s B - e C is a linear combination of two general points: one joint walk.
 *   count    The batch size of these three calls is named `count`, as for the silent-payment calls and for the same reason.
 *            They carry their span table in tests/test_dleq_cpu.py.
 *   p2e_point_lincomb2_batch   out_i = a_i P_i + b_i Q_i.  The conventions are p2e_point_lincomb_batch's: little-endian values;
 *            scalars reduced with one conditional subtraction, not flagged; (0, 0) a legal neutral operand; P checked before Q
 *            (P2E_WIRE_COORD_RANGE, then P2E_WIRE_NOT_ON_CURVE; operands are checked whatever the scalars are); a neutral
 *            result is P2E_WIRE_INFINITY and zeros.  Defined, none an error by itself: a = 0, b = 0, P or Q neutral, Q = +-P,
 *            Q = +-lambda P, a P = b Q (doubled), a P = -b Q (the neutral result).  plan as for p2e_point_mul_batch
 *            (P2E_MUL_PLAN_GLV on P2E_CURVE_P256 is P2E_E_INVALID); every plan writes the bytes p2e_point_mul_batch,
 *            p2e_point_mul_batch and p2e_point_add_batch write for the same operands.  One walk per lane with one accumulator:
 *            256 doublings under P2E_MUL_PLAN_PLAIN, 128 under P2E_MUL_PLAN_GLV, against 512 / 256 of the three calls.
 *            In place: (outx32, outy32) = (px32, py32), (outx32, outy32) = (qx32, qy32), outx32 = a32.  No output on b32.
 *   DLEQ     bytes: points and a_sk32 are the library's LITTLE-endian 32-byte values (they chain with p2e_sp_*, p2e_bip32_* and
 *            the point calls); aux_rand32 and msg32 are byte strings; proof64 = bytes32(e) || bytes32(s), BIG-endian as the
 *            standard writes it.  G is the curve's generator.  H_tag(x) = SHA256(SHA256(tag) || SHA256(tag) || x) for
 *            "BIP0374/aux", "BIP0374/nonce", "BIP0374/challenge"; cbytes(X) = (02 | parity of y) || bytes32(x); m' is msg32[i], or
 *            empty where msg32 is NULL (for the whole batch).  err[i] is a P2E_WIRE_* CODE, the first failing check in the
 *            order given; a flagged element writes zeros to all its outputs; the return value counts the flagged elements.
 *            This definition has not been checked against the vectors published with BIP-374.
 *   p2e_dleq_prove_batch   In order: a = 0 or a >= n: P2E_WIRE_SCALAR_RANGE; B (0, 0): P2E_WIRE_INFINITY, a coordinate >= p:
 *            P2E_WIRE_COORD_RANGE, off the curve: P2E_WIRE_NOT_ON_CURVE.  A = a G, C = a B;
 *            t = bytes32(a) xor H_aux(aux_rand); k = int(H_nonce(t || cbytes(A) || cbytes(C) || m')) mod n, k = 0:
 *            P2E_WIRE_INFINITY; R1 = k G, R2 = k B;
 *            e = int(H_challenge(cbytes(A) || cbytes(B) || cbytes(C) || cbytes(G) || cbytes(R1) || cbytes(R2) || m')), not reduced
 *            for the wire; s = (k + e a) mod n.  proof64 and, where cx32 is given (cy32 then too), C are written.  a, t and k
 *            never leave the lane's registers.  The standard's last step -- verify the fresh proof -- is NOT done, as
 *            p2e_schnorr_sign_batch does not verify what it signed: chain p2e_dleq_verify_batch (examples/dleq_share.c).
 *            In place: (cx32, cy32) = (bx32, by32) and nothing else (no output on a_sk32, aux_rand32 or msg32).
 *   p2e_dleq_verify_batch   In order: A, then B, then C ((0, 0): P2E_WIRE_INFINITY; a coordinate >= p: P2E_WIRE_COORD_RANGE; off
 *            the curve: P2E_WIRE_NOT_ON_CURVE); s >= n: P2E_WIRE_SCALAR_RANGE.  e is any 256-bit value and is used modulo n.
 *            Where err[i] == 0: R1 = s G - e A, R2 = s B - e C; valid[i] = 1 iff neither is the neutral element and bytes32(e)
 *            equals the challenge hash over A, B, C, G, R1, R2, m'.  A well-formed but wrong proof has err = 0, valid = 0 and is
 *            NOT counted; valid[i] = 0 wherever err[i] != 0 (the contract of p2e_schnorr_verify_batch).  No in-place form.
 * Each call is one kernel on the context's caller stream, one lane per element: no internal streams, no scratch block, no table in
 * LDS, nothing in the private segment.  Null pointers, P2E_MUL_PLAN_*, host pointers, async mode, the
 * current device and failed calls behave as for the point-arithmetic and silent-payment calls; count == 0 returns 0. */
long p2e_point_lincomb2_batch(p2e_ctx *ctx, int curve, unsigned plan, const uint8_t *a32, const uint8_t *b32,
                              const uint8_t *px32, const uint8_t *py32, const uint8_t *qx32, const uint8_t *qy32,
                              uint8_t *outx32, uint8_t *outy32, size_t count, uint8_t *err);
long p2e_dleq_prove_batch(p2e_ctx *ctx, const uint8_t *a_sk32, const uint8_t *bx32, const uint8_t *by32,
                          const uint8_t *aux_rand32, const uint8_t *msg32 /* nullable */, uint8_t *proof64,
                          uint8_t *cx32 /* nullable */, uint8_t *cy32 /* nullable, with cx32 */, size_t count, uint8_t *err);
long p2e_dleq_verify_batch(p2e_ctx *ctx, const uint8_t *ax32, const uint8_t *ay32, const uint8_t *bx32, const uint8_t *by32,
                           const uint8_t *cx32, const uint8_t *cy32, const uint8_t *proof64, const uint8_t *msg32 /* nullable */,
                           size_t count, uint8_t *err, uint8_t *valid);

/* ---- MuSig2 (BIP-327) on secp256k1 (csrc/musig.hpp): the multi-party form of a BIP-340 signature, from the key list to the
 * final signature.  A co-signer does per session what these seven calls do per element: hash a key list, multiply general
 * points by 256-bit coefficients, combine nonces, produce or check a partial signature.  The finished sig64 is an ordinary
 * BIP-340 signature under agg_pk32: p2e_schnorr_verify_batch accepts it.
 *   count    The batch size of these seven calls is named `count`, as for the Taproot and silent-payment calls and for the
 *            same reason.  They carry their span table in tests/test_musig_cpu.py.  BUFFER OVERLAP holds in full; every body
 *            reads all inputs of element i before its first store.  The ONE in-place form is p2e_musig_apply_tweak_batch's
 *            keyagg192_out = keyagg192_in; every other overlap of an output is P2E_E_INVALID.
 *   bytes    TWO orders, as for the silent-payment calls.  Points and secret scalars of the key layer are the library's
 *            LITTLE-endian 32-byte values (they chain with p2e_bip32_* and p2e_ecdsa_public_key_batch): pkx32 / pky32, sk32,
 *            secnonce64 = k_1 || k_2, pubnonce128 and aggnonce128 = x(R_1) || y(R_1) || x(R_2) || y(R_2).  A signer's
 *            public nonce is what p2e_ecdsa_public_key_batch returns for k_1 and k_2.  Hashes, tweak32, msg32, psig32,
 *            agg_pk32 and sig64 are the standard's BIG-endian strings.  (0, 0) is the point at infinity where one is legal:
 *            the two halves of an AGGREGATE nonce only.  Every array is 4-byte aligned but the one-byte ones.
 *   signers  key_offsets has count + 1 uint64 elements, in SIGNERS, not bytes: session i owns the signers
 *            [key_offsets[i], key_offsets[i + 1]) of a per-signer array (pkx32 / pky32 of the key aggregation, pubnonce128 of the
 *            nonce aggregation, psig32 of the signature aggregation).  A session with no signer, with more than
 *            P2E_MUSIG_MAX_SIGNERS, or with key_offsets[i + 1] < key_offsets[i] is P2E_WIRE_BAD_LENGTH.  A per-signer array has
 *            an extent only the device knows (BUFFER OVERLAP 5); with host pointers the signers [key_offsets[0],
 *            key_offsets[count]) are staged, and an offset outside that range is P2E_E_INVALID.
 *   hashes   H_tag(x) = SHA256(SHA256(tag) || SHA256(tag) || x); cbytes(P) the 33-byte compressed point, cbytes_ext the same
 *            with 33 zero bytes for the point at infinity, xbytes(P) the 32-byte x.
 *              pk2 = the first key whose cbytes differ from pk_1's (none where all keys are equal)
 *              L   = H_"KeyAgg list"(cbytes(pk_1) || .. || cbytes(pk_u))
 *              a_i = 1 if cbytes(pk_i) == cbytes(pk2), else int(H_"KeyAgg coefficient"(L || cbytes(pk_i))) mod n
 *              Q   = sum a_i P_i;   gacc = 1, tacc = 0
 *              tweak: g = n - 1 if x-only and y(Q) odd, else 1;  Q' = g Q + t G, gacc' = g gacc, tacc' = t + g tacc mod n
 *              b   = int(H_"MuSig/noncecoef"(cbytes_ext(R_1) || cbytes_ext(R_2) || xbytes(Q) || msg)) mod n
 *              R   = R_1 + b R_2, or G where that is the point at infinity;  e = int(H_"BIP0340/challenge"(xbytes(R) || xbytes(Q) || msg)) mod n
 *              s_i = k_1' + b k_2' + e a_i g gacc d_i mod n  (k' = n - k where y(R) is odd, g from the parity of y(Q))
 *              s   = sum s_i + e g tacc mod n;  sig64 = xbytes(R) || bytes(s)
 *   keyagg192   +0 x(Q), +32 y(Q) little-endian; +64 tacc big-endian; +96 L; +128 x of pk2 big-endian (zeros where there is
 *            none); +160 uint32 flags: bit 0 = gacc is n - 1, bit 1 = pk2 present, bit 2 = y(pk2) odd; +164 .. 191 zero.  A call
 *            that reads a record checks it, in this order: the point ((0, 0), which is what a flagged element left:
 *            P2E_WIRE_INFINITY; a coordinate >= p: P2E_WIRE_COORD_RANGE; off the curve: P2E_WIRE_NOT_ON_CURVE), tacc >= n:
 *            P2E_WIRE_SCALAR_RANGE, x(pk2) >= p: P2E_WIRE_COORD_RANGE, an unknown flag bit: P2E_WIRE_BAD_PREFIX.
 *   session128  +0 b, +32 e big-endian; +64 xbytes(R); +96 uint32 flags: bit 0 = y(R) odd; +100 .. 127 zero.  Checked where it
 *            is read: b or e >= n: P2E_WIRE_SCALAR_RANGE; xbytes(R) all zero (a flagged element's): P2E_WIRE_INFINITY;
 *            x(R) >= p: P2E_WIRE_COORD_RANGE; an unknown flag bit: P2E_WIRE_BAD_PREFIX.
 *   err[i]   a P2E_WIRE_* CODE: the first failing check in the order given below; a flagged element writes zeros to all its
 *            outputs, so a flag travels down the chain (the next call finds a zeroed record).  The return value counts the
 *            flagged elements; count == 0 returns 0.  Null pointers, host pointers, async mode, the current device and failed
 *            calls behave as for the Taproot calls.  A point that must not be (0, 0) is checked as p2e_point_mul_batch would
 *            flag it: (0, 0): P2E_WIRE_INFINITY; a coordinate >= p: P2E_WIRE_COORD_RANGE; off the curve:
 *            P2E_WIRE_NOT_ON_CURVE.  Nothing >= n is ever reduced silently.
 *   p2e_musig_key_agg_batch   The length; the keys in their order (the first failing key gives the code); Q at infinity:
 *            P2E_WIRE_INFINITY.  agg_pk32 = xbytes(Q).
 *   p2e_musig_apply_tweak_batch   mode P2E_MUSIG_TWEAK_PLAIN: t = tweak32, g = 1; P2E_MUSIG_TWEAK_XONLY: t = tweak32, x-only;
 *            P2E_MUSIG_TWEAK_TAPROOT: x-only with t = int(H_"TapTweak"(xbytes(Q) || tweak32)), tweak32 the Merkle root, or, with
 *            tweak32 == NULL, nothing appended (BIP-86's key-path-only output) -- the key p2e_taproot_tweak_pubkey_batch gives
 *            for agg_pk32.  Any other mode, or a null tweak32 in modes 0 and 1, is P2E_E_INVALID.  The record; t >= n:
 *            P2E_WIRE_SCALAR_RANGE; Q' at infinity: P2E_WIRE_INFINITY.  Tweaks are applied one call after the other.
 *   p2e_musig_nonce_agg_batch   The length; per signer R_1 then R_2, neither may be (0, 0).  A sum at infinity is (0, 0), no error.
 *   p2e_musig_session_batch   The record; R_1 then R_2 of the aggregate nonce, each (0, 0) or on the curve.
 *   p2e_musig_partial_sign_batch   One lane per session, for the caller's own signer in it.  In order: k_1, k_2, sk32 (each 0 or
 *            >= n: P2E_WIRE_SCALAR_RANGE), the key record, the session record.  The signer's key d' G is computed here and its
 *            coefficient is taken from L and pk2 of the record.  k_1, k_2, d' and every product of them never leave the lane's
 *            registers.  TWO departures from the standard's Sign: secnonce64 carries no public key, so checking that the nonce
 *            was made for this key is the caller's; and the library cannot know whether d' G is in the key list (a key that is
 *            not gets a hashed coefficient like any other, and the aggregate signature does not verify).
 *            Checking the result with p2e_musig_partial_verify_batch catches both.  A SECRET NONCE MUST NEVER BE USED TWICE:
 *            two partial signatures with one secnonce64 under different b or e reveal the secret key.  The library keeps no
 *            state and cannot detect reuse; wipe secnonce64 after the call.
 *   p2e_musig_partial_verify_batch   One lane per partial signature; its session is session_index[i] (NULL: i) of the n_sessions
 *            records.  In order: session_index[i] >= n_sessions: P2E_WIRE_BAD_INDEX; psig32 >= n: P2E_WIRE_SCALAR_RANGE; R_1, R_2
 *            of the signer's pubnonce128; the signer's key; the key record; the session record.  valid[i] = 1 iff
 *            s G == Re + (e a g gacc mod n) P with Re = R_1 + b R_2, negated where y(R) is odd; 0 where err[i] != 0 (every
 *            element is written, as by p2e_schnorr_verify_batch).  n_sessions == 0 is P2E_E_INVALID.
 *   p2e_musig_sig_agg_batch   The length; the key record; the session record; the partial signatures in their order (>= n:
 *            P2E_WIRE_SCALAR_RANGE).
 * Each call is one kernel on the context's caller stream, one lane per element: no internal streams, no scratch. */
#define P2E_MUSIG_MAX_SIGNERS 1024
#define P2E_MUSIG_TWEAK_PLAIN 0
#define P2E_MUSIG_TWEAK_XONLY 1
#define P2E_MUSIG_TWEAK_TAPROOT 2
long p2e_musig_key_agg_batch(p2e_ctx *ctx, const uint8_t *pkx32 /* per signer */, const uint8_t *pky32 /* per signer */,
                             const uint64_t *key_offsets /* count + 1, in signers */, uint8_t *keyagg192, uint8_t *agg_pk32,
                             size_t count, uint8_t *err);
long p2e_musig_apply_tweak_batch(p2e_ctx *ctx, const uint8_t *keyagg192_in, const uint8_t *tweak32 /* nullable in mode 2 */,
                                 int mode, uint8_t *keyagg192_out, uint8_t *agg_pk32, size_t count, uint8_t *err);
long p2e_musig_nonce_agg_batch(p2e_ctx *ctx, const uint8_t *pubnonce128 /* per signer */,
                               const uint64_t *key_offsets /* count + 1, in signers */, uint8_t *aggnonce128, size_t count,
                               uint8_t *err);
long p2e_musig_session_batch(p2e_ctx *ctx, const uint8_t *keyagg192, const uint8_t *aggnonce128, const uint8_t *msg32,
                             uint8_t *session128, size_t count, uint8_t *err);
long p2e_musig_partial_sign_batch(p2e_ctx *ctx, const uint8_t *secnonce64, const uint8_t *sk32, const uint8_t *keyagg192,
                                  const uint8_t *session128, uint8_t *psig32, size_t count, uint8_t *err);
long p2e_musig_partial_verify_batch(p2e_ctx *ctx, const uint8_t *psig32, const uint8_t *pubnonce128, const uint8_t *pkx32,
                                    const uint8_t *pky32, const uint32_t *session_index /* nullable: identity */,
                                    const uint8_t *keyagg192 /* n_sessions */, const uint8_t *session128 /* n_sessions */,
                                    size_t n_sessions, size_t count, uint8_t *err, uint8_t *valid);
long p2e_musig_sig_agg_batch(p2e_ctx *ctx, const uint8_t *psig32 /* per signer */,
                             const uint64_t *key_offsets /* count + 1, in signers */, const uint8_t *keyagg192,
                             const uint8_t *session128, uint8_t *sig64, size_t count, uint8_t *err);

/* ---- synthetic inputs (host only): valid signatures per curve/ecdsa.rs:25-40 sign_message with
 * sk, msg, nonce drawn from splitmix64(seed, i).  Host buffers of n*32 bytes each. -------------------- */
int p2e_synth_signatures(uint64_t seed, size_t first, size_t n, uint8_t *msg32, uint8_t *r32, uint8_t *s32,
                         uint8_t *pkx32, uint8_t *pky32);

#ifdef __cplusplus
}
#endif
#endif /* P2E_H */
