/* C restatement of the plonky2-ecdsa hot-path witness generators -- TEST INFRASTRUCTURE ONLY.
 *
 * Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may link or call this.  The
 * product path (plonky2-ecdsa_amd/, include/p2e.h) never does.
 *
 * PARITY STATUS: "parity unpinned" against literal reference outputs (the reference holds no golden
 * vectors for these generators and cannot be built offline: SURVEY.md 8c).  Pinned instead by
 * (i) agreement with the independent Python big-int restatement oracle/p2e_ref.py on the committed
 * fixtures tests/golden/ (ii) the reference's constraint equations, re-evaluated in tests/.
 * The constraint-block (ux) and gate-internal matrices of the *_full walks are pinned by agreement with the Python
 * constraint replay oracle/check_circuit.py; their U29 gate model stays "upstream-from-memory" (see below).
 *
 * Data layout (same as include/p2e.h): Goldilocks-canonical u64 columns, column-major over the
 * batch: element (col, i) lives at base[col * ld + i], ld >= n.  256-bit inputs are packed 32-byte
 * little-endian, element i at base + 32*i.
 */
#ifndef P2E_ORACLE_H
#define P2E_ORACLE_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define P2E_O_FIELD_BASE 0   /* Secp256K1Base   */
#define P2E_O_FIELD_SCALAR 1 /* Secp256K1Scalar */
#define P2E_O_FIELD_P256_BASE 2   /* field/p256_base.rs   */
#define P2E_O_FIELD_P256_SCALAR 3 /* field/p256_scalar.rs */

#define P2E_O_ERR_LIMB_RANGE 1
#define P2E_O_ERR_VALUE_GE_2_256 2
#define P2E_O_ERR_INVERSE_OF_ZERO 4
#define P2E_O_ERR_CARRY_RANGE 8
#define P2E_O_ERR_QUOTIENT_RANGE 16
#define P2E_O_ERR_DIVISION_BY_ZERO 32

#define P2E_O_VERIFY_COLS 82615
#define P2E_O_GLV_MUL_COLS 65243
#define P2E_O_VERIFY_AUX 8959
#define P2E_O_GLV_MUL_AUX 4738

/* each returns the number of elements with err != 0 */
/* gates/mul_nonnative.rs:249-324 + :513-531 : x[9][n], y[9][n] -> r[9], q[9], cs[17], b[16] */
long p2e_oracle_mul_witness(int field, const uint64_t *x, const uint64_t *y, uint64_t *r, uint64_t *q,
                            uint64_t *cs, uint64_t *b, size_t n, size_t ld, uint8_t *err);
/* gates/mul_nonnative.rs:513-531 alone: a[17][n] -> b[16][n] (true Goldilocks field division) */
long p2e_oracle_checksum_witness(const uint64_t *a, uint64_t *b, size_t n, size_t ld, uint8_t *err);
/* gadgets/nonnative.rs:626-645 : a[9][n], b[9][n] -> sum[9][n], overflow[n] */
long p2e_oracle_add_witness(int field, const uint64_t *a, const uint64_t *b, uint64_t *sum, uint64_t *ov,
                            size_t n, size_t ld, uint8_t *err);
/* gadgets/nonnative.rs:792-810 */
long p2e_oracle_sub_witness(int field, const uint64_t *a, const uint64_t *b, uint64_t *diff, uint64_t *ov,
                            size_t n, size_t ld, uint8_t *err);
/* gadgets/nonnative.rs:696-728 : summands[k][9][n] */
long p2e_oracle_add_many_witness(int field, const uint64_t *summands, int k, uint64_t *sum, uint64_t *ov,
                                 size_t n, size_t ld, uint8_t *err);
/* gadgets/nonnative.rs:857-872 : x[9][n] -> inv[9][n], div[9][n] */
long p2e_oracle_inv_witness(int field, const uint64_t *x, uint64_t *inv, uint64_t *div, size_t n, size_t ld,
                            uint8_t *err);
/* gadgets/glv.rs:128-142 : k[9][n] -> k1[5][n], k2[5][n], k1_neg[n], k2_neg[n] */
long p2e_oracle_glv_decompose(const uint64_t *k, uint64_t *k1, uint64_t *k2, uint64_t *k1_neg,
                              uint64_t *k2_neg, size_t n, size_t ld, uint8_t *err);
/* gadgets/biguint.rs:508-518 BigUintDivRemGenerator: a[na][n] (na <= 18), b[nb][n] (nb <= 9) ->
 * div[max(0, na - nb + 1)][n], rem[nb][n].  Limbs must be < 2^29 (ERR_LIMB_RANGE), b != 0 (ERR_DIVISION_BY_ZERO),
 * div must fit its limbs (ERR_LIMB_RANGE: the reference's set_biguint_target assert). */
long p2e_oracle_div_rem(const uint64_t *a, int na, const uint64_t *b, int nb, uint64_t *div, uint64_t *rem, size_t n,
                        size_t ld, uint8_t *err);
/* gadgets/biguint.rs:27-51,454-463 : packed 32-byte LE -> limbs[9][n] and back (pack flags limbs >= 2^29
 * or value >= 2^256) */
long p2e_oracle_limb_split(const uint8_t *packed, uint64_t *limbs, size_t n, size_t ld);
long p2e_oracle_limb_pack(const uint64_t *limbs, uint8_t *packed, size_t n, size_t ld, uint8_t *err);

/* gadgets/ecdsa.rs:30-53 : cols[82615][n].  flags[i] bit0 = all three connect constraints hold
 * (curve_assert_valid, glv k reconstruction, r == x). nthreads <= 0 -> omp default. */
long p2e_oracle_verify_witness(const uint8_t *msg, const uint8_t *r, const uint8_t *s, const uint8_t *pkx,
                               const uint8_t *pky, uint64_t *cols, size_t n, size_t ld, uint8_t *err,
                               uint8_t *flags, int nthreads);
/* The same columns by the OPTIMISED CPU variant (BASELINE.md section 2 variant b; bench.py cpu_baseline_optimised):
 * signatures are walked in lock-step groups of `group` (<= 256, <= 0 -> 64) and every inverse generator's
 * FF::inverse() of a group is one Fermat ladder + 3 multiplications per signature (Montgomery's trick across
 * signatures at the same schedule step); everything else is the faithful-cost algorithm.  Returns -1 if the
 * per-thread coroutine stacks cannot be allocated. */
long p2e_oracle_verify_witness_lockstep(const uint8_t *msg, const uint8_t *r, const uint8_t *s, const uint8_t *pkx,
                                        const uint8_t *pky, uint64_t *cols, size_t n, size_t ld, uint8_t *err,
                                        uint8_t *flags, int nthreads, int group);
/* ... additionally recording aux[8959][n] (see p2e_oracle_verify_witness_aux below); aux == NULL: not recorded */
long p2e_oracle_verify_witness_aux_lockstep(const uint8_t *msg, const uint8_t *r, const uint8_t *s, const uint8_t *pkx,
                                            const uint8_t *pky, uint64_t *cols, size_t n, size_t ld, uint64_t *aux, size_t ald,
                                            uint8_t *err, uint8_t *flags, int nthreads, int group);
/* gadgets/glv.rs:87-104 : cols[65243][n] */
long p2e_oracle_glv_mul_witness(const uint8_t *px, const uint8_t *py, const uint8_t *k, uint64_t *cols,
                                size_t n, size_t ld, uint8_t *err, uint8_t *flags, int nthreads);

/* The same walks, additionally recording aux[8959][n] / aux[4738][n]: the values of the targets that plonky2's
 * BUILT-IN generators fill on this path, in the order the gadgets create them:
 * split_le_base bits and the 4-/2-bit digits built from them (gadgets/split_nonnative.rs:25-72), is_equal / not
 * results and the random_access_curve_points selection per window (gadgets/curve_fixed_base.rs:56-61,
 * gadgets/curve_msm.rs:67-71, gadgets/curve_windowed_mul.rs:74-118), not(b) and the mul_biguint_by_bool products
 * of every conditional add / negation (gadgets/curve.rs:225-243, gadgets/nonnative.rs:584-596,
 * gadgets/biguint.rs:360-374).  aux == NULL: not recorded. */
long p2e_oracle_verify_witness_aux(const uint8_t *msg, const uint8_t *r, const uint8_t *s, const uint8_t *pkx,
                                   const uint8_t *pky, uint64_t *cols, size_t n, size_t ld, uint64_t *aux,
                                   size_t ald, uint8_t *err, uint8_t *flags, int nthreads);
long p2e_oracle_glv_mul_witness_aux(const uint8_t *px, const uint8_t *py, const uint8_t *k, uint64_t *cols,
                                    size_t n, size_t ld, uint64_t *aux, size_t ald, uint8_t *err, uint8_t *flags,
                                    int nthreads);

/* ---- curve programs: the crate's other scalar multiplications, on both curves ------------
 * kind 1: curve_scalar_mul_windowed gadgets/curve_windowed_mul.rs:131-173 (precompute_window :52-72) -- 98 185 columns
 * kind 2: curve_scalar_mul          gadgets/curve.rs:245-285                                         -- 139 354 columns
 * kind 3: verify_p256_message_circuit gadgets/ecdsa.rs:55-78 (curve must be 1)                       -- 115 557 columns
 * curve 0 = secp256k1, 1 = P-256 (curve/p256.rs:15-57).  blind = the point the gadget draws with rand() while the
 * circuit is built (curve_windowed_mul.rs:57, curve.rs:253): an input here, like in include/p2e.h
 * p2e_curve_program_create.  Kinds 1, 2 read (k, -, -, p.x, p.y) from (msg, r, s, px, py); kind 3 reads all five.
 * aux (NULL: not recorded): the built-in-generator values of the same circuit in gadget creation order, as for the
 * built-in programs above (4 221 / 9 918 / 8 442 values).  flags: kinds 1, 2 always 1; kind 3 the two connects
 * (curve_assert_valid, r == x).  lockstep_group > 0: the optimised-CPU variant (one Fermat ladder per group and inverse
 * op), same columns bit for bit.  Returns the number of flagged elements, -1 on bad arguments, -2 if the coroutine
 * stacks cannot be allocated. */
#define P2E_O_CP_WINDOWED_MUL 1
#define P2E_O_CP_SCALAR_MUL 2
#define P2E_O_CP_VERIFY 3
long p2e_oracle_curve_program(int kind, int curve, const uint8_t *blind_x32, const uint8_t *blind_y32,
                              const uint8_t *msg, const uint8_t *r, const uint8_t *s, const uint8_t *px,
                              const uint8_t *py, uint64_t *cols, size_t n, size_t ld, uint64_t *aux, size_t ald,
                              uint8_t *err, uint8_t *flags, int nthreads, int lockstep_group);
/* kind 4: curve_msm_circuit(p, q, n, m) gadgets/curve_msm.rs:21-79 on its own, with two raw 256-bit scalars of 9 limbs
 *         each (261 bits padded to 262, 131 two-bit digits, MSB first); the blinding point is KeccakHash::<32>(F::ZERO) * G
 *         of the curve (:33-39) and the unblinding constant -2^262 times it          -- 112 309 columns, 8 382 aux values
 * kind 5: fixed_base_curve_mul_circuit(base, k) gadgets/curve_fixed_base.rs:18-66 with a caller-supplied affine base
 *         (66 windows of 16 entries built once per call, slot 0 := slot 1)           --  16 797 columns, 4 221 aux values
 * Both take raw scalars (no reduction).  err: P2E_O_ERR_INVERSE_OF_ZERO where the reference panics (an addition of two
 * points with the same x: p = +-q, n = m = 0, k = 0, a base or point that meets the blinding point); flags = (err == 0).
 * Same return values, aux, nthreads and lockstep_group as p2e_oracle_curve_program. */
#define P2E_O_CP_MSM 4
#define P2E_O_CP_FIXED_BASE_MUL 5
long p2e_oracle_curve_msm(int curve, const uint8_t *px, const uint8_t *py, const uint8_t *qx, const uint8_t *qy,
                          const uint8_t *n_scalar, const uint8_t *m_scalar, uint64_t *cols, size_t n, size_t ld,
                          uint64_t *aux, size_t ald, uint8_t *err, uint8_t *flags, int nthreads, int lockstep_group);
long p2e_oracle_curve_fixed_base(int curve, const uint8_t *base_x32, const uint8_t *base_y32, const uint8_t *k,
                                 uint64_t *cols, size_t n, size_t ld, uint64_t *aux, size_t ald, uint8_t *err,
                                 uint8_t *flags, int nthreads, int lockstep_group);
/* column counts of a curve program (kinds 1-5) by a dry walk: returns num_cols, *num_aux = built-in-generator values */
long p2e_oracle_curve_program_num_cols(int kind, int curve, long *num_aux);

/* ---- constraint-block (ux) and gate-internal (gate) matrices: SURVEY.md 8(f) rank 2 and the rest of rank 1 -----------
 * The *_full walks are the walks above, additionally recording
 *   ux[num_ux][n]     every value a plonky2_ux U29 gate returns inside the constraint block of a non-native gadget
 *                     (gadgets/nonnative.rs:262-273 add, :330-351 add_many, :373-386 sub, :462-463 mul's range check,
 *                     :518-530 inv; gadgets/biguint.rs:240-323 add / sub / mul_biguint, :360-374 modulus * overflow),
 *                     generator by generator in builder-call order.  The gates are modelled by what they constrain --
 *                     add_many_ux / add_uxs_with_carry -> (sum mod 2^29, sum >> 29), mul_ux -> (a b mod 2^29, a b >> 29),
 *                     sub_ux -> (x - y - borrow + 2^29 borrow_out, borrow_out), list_le -> [a <= b] -- the model stated at
 *                     the top of oracle/check_circuit.py [upstream-from-memory: plonky2_ux is not in the container]
 *   gate[num_gate][n] per window, in call order: is_equal(index, zero)'s five internal targets (not(equal), the
 *                     EqualityGenerator's inverse of the index in Goldilocks or 0, diff, diff * inv, diff * (diff * inv))
 *                     and, per selected limb of a random_access_curve_points (9 x, 9 y), the 4 bit wires of the access
 *                     index, least significant first [upstream-from-memory]
 * both u64, column-major with their own strides (uld, gld >= n); NULL = not recorded.  Operands are the limb vectors the
 * walk holds, with the limb count the target has in the reference (constants drop zero limbs on top); nothing is read
 * back through a wiring table.  Values of an element with err != 0 are unspecified.
 * PARITY STATUS of these two matrices: pinned by agreement with the Python constraint replay oracle/check_circuit.py
 * (Circuit.ux / .gate / .ux_ops) on random, named adversarial and golden elements of every program (tests/); the U29
 * gate model itself stays "upstream-from-memory". */
long p2e_oracle_verify_witness_full(const uint8_t *msg, const uint8_t *r, const uint8_t *s, const uint8_t *pkx,
                                    const uint8_t *pky, uint64_t *cols, size_t n, size_t ld, uint64_t *aux, size_t ald,
                                    uint64_t *ux, size_t uld, uint64_t *gate, size_t gld, uint8_t *err, uint8_t *flags,
                                    int nthreads, int lockstep_group);
long p2e_oracle_glv_mul_witness_full(const uint8_t *px, const uint8_t *py, const uint8_t *k, uint64_t *cols, size_t n,
                                     size_t ld, uint64_t *aux, size_t ald, uint64_t *ux, size_t uld, uint64_t *gate,
                                     size_t gld, uint8_t *err, uint8_t *flags, int nthreads);
long p2e_oracle_curve_program_full(int kind, int curve, const uint8_t *blind_x32, const uint8_t *blind_y32,
                                   const uint8_t *msg, const uint8_t *r, const uint8_t *s, const uint8_t *px,
                                   const uint8_t *py, uint64_t *cols, size_t n, size_t ld, uint64_t *aux, size_t ald,
                                   uint64_t *ux, size_t uld, uint64_t *gate, size_t gld, uint8_t *err, uint8_t *flags,
                                   int nthreads, int lockstep_group);
long p2e_oracle_curve_msm_full(int curve, const uint8_t *px, const uint8_t *py, const uint8_t *qx, const uint8_t *qy,
                               const uint8_t *n_scalar, const uint8_t *m_scalar, uint64_t *cols, size_t n, size_t ld,
                               uint64_t *aux, size_t ald, uint64_t *ux, size_t uld, uint64_t *gate, size_t gld, uint8_t *err,
                               uint8_t *flags, int nthreads, int lockstep_group);
long p2e_oracle_curve_fixed_base_full(int curve, const uint8_t *base_x32, const uint8_t *base_y32, const uint8_t *k,
                                      uint64_t *cols, size_t n, size_t ld, uint64_t *aux, size_t ald, uint64_t *ux, size_t uld,
                                      uint64_t *gate, size_t gld, uint8_t *err, uint8_t *flags, int nthreads,
                                      int lockstep_group);
/* Layout of a program by a dry walk: kind 1-5 a curve program on `curve`, P2E_O_PROG_VERIFY / P2E_O_PROG_GLV_MUL the two
 * built-in walks (curve 0).  Returns num_cols; *num_aux, *num_ux, *num_gate the other three column counts;
 * *num_generators the generator count.  blocks (cap pairs, may be NULL): (first ux column, number of ux columns) of every
 * generator in registration order -- 0 columns for a generator without a block (the GLV decomposition, a multiplication
 * that is not range-checked). */
#define P2E_O_PROG_VERIFY 0
#define P2E_O_PROG_GLV_MUL 6
long p2e_oracle_program_layout(int kind, int curve, long *num_aux, long *num_ux, long *num_gate, uint32_t *blocks, size_t cap,
                               long *num_generators);

/* constants computed at init (for tests): rando = keccak256(0u64 LE) as LE scalar * G */
void p2e_oracle_rando(uint8_t x32[32], uint8_t y32[32]);
int p2e_oracle_max_threads(void);

#ifdef __cplusplus
}
#endif
#endif
