//! `extern "C"` surface of libp2e_hip.so, mirroring include/p2e.h declaration by declaration.
//! Every function cites, in the header, the reference `run_once` body or gadget it stands in for.
use core::ffi::{c_char, c_void};

#[repr(C)]
pub struct P2eCtx {
    _private: [u8; 0],
}
#[repr(C)]
pub struct P2eWireMap {
    _private: [u8; 0],
}
#[repr(C)]
#[derive(Clone, Copy)]
pub struct P2eGenDesc {
    pub kind: i32, // 0 add, 1 sub, 2 add_many, 3 mul(+checksum), 4 inv, 5 glv_decomposition
    pub field: i32, // 0 Secp256K1Base, 1 Secp256K1Scalar
    pub first_col: u32,
    pub num_cols: u32,
    pub label: [u8; 48],
}
#[repr(C)]
#[derive(Clone, Copy)]
pub struct P2eGenWiring {
    pub num_operands: i32,
    pub src: [u32; 4],
    pub num_limbs: [u8; 4],
    pub range_check: i32,
}
#[repr(C)]
#[derive(Clone, Copy)]
pub struct P2eAuxDesc {
    pub kind: i32,
    pub first_col: u32,
    pub num_cols: u32,
    pub label: [u8; 48],
}
#[repr(C)]
#[derive(Clone, Copy)]
pub struct P2eUxDesc {
    pub first_col: u32,
    pub num_cols: u32,
}
#[repr(C)]
#[derive(Clone, Copy)]
pub struct P2eWireMapEntry {
    pub src: u32, // P2E_WIRE_SRC_{COLS,AUX,UX} | column
    pub dst: u32, // wire * degree + row
}

/// a block of witness columns completed by one launch of a fused call; a launch may complete several (include/p2e.h p2e_segments_describe)
#[repr(C)]
#[derive(Clone, Copy)]
pub struct P2eSegmentDesc {
    pub first_col: u32,
    pub num_cols: u32,
}

pub const P2E_CTX_HOST_POINTERS: u32 = 1;
pub const P2E_CTX_ASYNC: u32 = 2;
pub const P2E_CTX_PHASE_TIMING: u32 = 4;
pub const P2E_VERIFY_COLS: usize = 82_615;
pub const P2E_VERIFY_AUX_COLS: usize = 8_959;
pub const P2E_VERIFY_UX_COLS: usize = 249_385;
pub const P2E_SRC_AUX: u32 = 0x2000_0000;
pub const P2E_SRC_INPUT: u32 = 0x4000_0000;
pub const P2E_SRC_CONST: u32 = 0x8000_0000;
pub const P2E_WIRE_SRC_COLS: u32 = 0x0000_0000;
pub const P2E_WIRE_SRC_AUX: u32 = 0x4000_0000;
pub const P2E_WIRE_SRC_UX: u32 = 0x8000_0000;
pub const P2E_WIRE_SRC_GATE: u32 = 0xC000_0000;
pub const P2E_COMPACT_WIDE: u32 = 0x8000_0000;

/// one built circuit of a curve program (include/p2e.h p2e_curve_program)
#[repr(C)]
pub struct P2eCurveProgram {
    _private: [u8; 0],
}
pub const P2E_CURVE_SECP256K1: i32 = 0;
pub const P2E_CURVE_P256: i32 = 1;
pub const P2E_SIGN_PLAN_AUTO: u32 = 0;
pub const P2E_SIGN_PLAN_LANE: u32 = 1;
pub const P2E_SIGN_PLAN_QUAD: u32 = 2;
pub const P2E_HASH_SHA256: i32 = 0;
pub const P2E_HASH_SHA256D: i32 = 1;
pub const P2E_HASH_KECCAK256: i32 = 2;
pub const P2E_DIGEST_BYTES: u32 = 0;
pub const P2E_DIGEST_SCALAR: u32 = 1;
// err CODES (not bits) of the four wire-form calls
pub const P2E_WIRE_OK: u8 = 0;
pub const P2E_WIRE_BAD_LENGTH: u8 = 1;
pub const P2E_WIRE_BAD_PREFIX: u8 = 2;
pub const P2E_WIRE_COORD_RANGE: u8 = 3;
pub const P2E_WIRE_NOT_ON_CURVE: u8 = 4;
pub const P2E_WIRE_INFINITY: u8 = 5;
pub const P2E_WIRE_DER_SYNTAX: u8 = 6;
pub const P2E_WIRE_DER_INTEGER: u8 = 7;
pub const P2E_WIRE_SCALAR_RANGE: u8 = 8;
pub const P2E_WIRE_HIGH_S: u8 = 9;
pub const P2E_WIRE_BAD_INDEX: u8 = 10; // the point-table calls: idx[i] >= the table's point count
pub const P2E_POINT_TABLE_MAX_POINTS: usize = 65536;
pub const P2E_POINT_TABLE_BYTES_PER_POINT: usize = 67584;
pub const P2E_SEC1_COMPRESSED: i32 = 0;
pub const P2E_SEC1_UNCOMPRESSED: i32 = 1;
pub const P2E_SIG_DER: i32 = 0;
pub const P2E_SIG_COMPACT64: i32 = 1;
pub const P2E_SIG_COMPACT65: i32 = 2;
pub const P2E_SIG_REQUIRE_LOW_S: u32 = 1;
pub const P2E_SIG_NORMALIZE_S: u32 = 2;
pub const P2E_SIG_DER_STRIDE: usize = 72;
pub const P2E_MSM_WINDOW_AUTO: u32 = 0;
pub const P2E_MSM_WINDOW_MIN: u32 = 4;
pub const P2E_MSM_WINDOW_MAX: u32 = 12;
pub const P2E_MSM_OK: u8 = 0;
pub const P2E_MSM_NEUTRAL: u8 = 1;
pub const P2E_MSM_BAD_POINT: u8 = 2;
pub const P2E_MSM_PLAN_WINDOW_BITS: usize = 0;
pub const P2E_MSM_PLAN_WINDOWS: usize = 1;
pub const P2E_MSM_PLAN_BUCKETS: usize = 2;
pub const P2E_MSM_PLAN_SEG: usize = 3;
pub const P2E_MSM_PLAN_SCRATCH_BYTES: usize = 4;
pub const P2E_MSM_PLAN_MAX_LANE_ADDITIONS: usize = 5;
pub const P2E_MSM_PLAN_WORDS: usize = 6;
pub const P2E_ERR_POINT_AT_INFINITY: u8 = 64;
pub const P2E_CP_WINDOWED_MUL: i32 = 1;
pub const P2E_CP_SCALAR_MUL: i32 = 2;
pub const P2E_CP_VERIFY: i32 = 3;
pub const P2E_CP_MSM: i32 = 4;
pub const P2E_CP_FIXED_BASE_MUL: i32 = 5;

// tests/test_ffi_surface.py parses this block and include/p2e.h and requires the same symbols, argument counts and
// integer widths: add a declaration here whenever the header gains one.
#[link(name = "p2e_hip")]
extern "C" {
    // ---- context
    pub fn p2e_ctx_create(device: i32, flags: u32, stream: *mut c_void, out: *mut *mut P2eCtx) -> i32;
    pub fn p2e_ctx_destroy(ctx: *mut P2eCtx);
    pub fn p2e_sync(ctx: *mut P2eCtx) -> i32;
    pub fn p2e_last_error() -> *const c_char;
    pub fn p2e_scratch_bytes(program: i32, n: usize) -> usize;
    // per-phase / per-kernel HIP-event timings of the last fused call on this context (bench.py's roofline figures)
    pub fn p2e_last_phase_ms(ctx: *mut P2eCtx, out: *mut f32, cap: i32) -> i32;
    // column blocks of the last fused call as they become final: what an RCCL exchange / D2H copy / prover can start on
    pub fn p2e_segments_describe(ctx: *mut P2eCtx, out: *mut P2eSegmentDesc, cap: usize) -> i64;
    pub fn p2e_segment_stream_wait(ctx: *mut P2eCtx, segment: i32, stream: *mut c_void) -> i32;
    pub fn p2e_segment_sync(ctx: *mut P2eCtx, segment: i32) -> i32;

    // ---- the fused schedules: every hot-path run_once of one circuit instance per batch element
    // gadgets/ecdsa.rs:30-53 (gates/mul_nonnative.rs:249-324,513-531; gadgets/nonnative.rs:626-645,696-728,792-810,
    // 857-872; gadgets/glv.rs:128-142)
    pub fn p2e_ecdsa_verify_witness_batch(ctx: *mut P2eCtx, msg32: *const u8, r32: *const u8, s32: *const u8, pkx32: *const u8,
        pky32: *const u8, cols: *mut u64, n: usize, ld: usize, err: *mut u8, valid: *mut u8) -> i64;
    pub fn p2e_ecdsa_verify_witness_compact_batch(ctx: *mut P2eCtx, msg32: *const u8, r32: *const u8, s32: *const u8,
        pkx32: *const u8, pky32: *const u8, narrow: *mut u32, ld_narrow: usize, wide: *mut u64, ld_wide: usize, n: usize,
        err: *mut u8, valid: *mut u8) -> i64;
    pub fn p2e_glv_mul_witness_batch(ctx: *mut P2eCtx, px32: *const u8, py32: *const u8, k32: *const u8, cols: *mut u64,
        n: usize, ld: usize, err: *mut u8, valid: *mut u8) -> i64;
    pub fn p2e_glv_mul_witness_compact_batch(ctx: *mut P2eCtx, px32: *const u8, py32: *const u8, k32: *const u8,
        narrow: *mut u32, ld_narrow: usize, wide: *mut u64, ld_wide: usize, n: usize, err: *mut u8, valid: *mut u8) -> i64;
    // the circuit's verdict alone (curve/ecdsa.rs:42-62 verify_message with the circuit's semantics)
    pub fn p2e_ecdsa_verify_batch(ctx: *mut P2eCtx, msg32: *const u8, r32: *const u8, s32: *const u8, pkx32: *const u8,
        pky32: *const u8, n: usize, err: *mut u8, valid: *mut u8) -> i64;

    // ---- single generators (one run_once body each)
    pub fn p2e_mul_witness_batch(ctx: *mut P2eCtx, field: i32, x: *const u64, y: *const u64, r: *mut u64, q: *mut u64,
        check_sum: *mut u64, b: *mut u64, n: usize, ld: usize, err: *mut u8) -> i64;
    pub fn p2e_checksum_witness_batch(ctx: *mut P2eCtx, a: *const u64, b: *mut u64, n: usize, ld: usize, err: *mut u8) -> i64;
    pub fn p2e_add_witness_batch(ctx: *mut P2eCtx, field: i32, a: *const u64, b: *const u64, sum: *mut u64, overflow: *mut u64,
        n: usize, ld: usize, err: *mut u8) -> i64;
    pub fn p2e_sub_witness_batch(ctx: *mut P2eCtx, field: i32, a: *const u64, b: *const u64, diff: *mut u64, overflow: *mut u64,
        n: usize, ld: usize, err: *mut u8) -> i64;
    pub fn p2e_add_many_witness_batch(ctx: *mut P2eCtx, field: i32, summands: *const u64, k: i32, sum: *mut u64,
        overflow: *mut u64, n: usize, ld: usize, err: *mut u8) -> i64;
    pub fn p2e_inv_witness_batch(ctx: *mut P2eCtx, field: i32, x: *const u64, inv: *mut u64, div: *mut u64, n: usize, ld: usize,
        err: *mut u8) -> i64;
    pub fn p2e_biguint_div_rem_batch(ctx: *mut P2eCtx, a: *const u64, na: i32, b: *const u64, nb: i32, div: *mut u64,
        rem: *mut u64, n: usize, ld: usize, err: *mut u8) -> i64;
    pub fn p2e_glv_decompose_batch(ctx: *mut P2eCtx, k: *const u64, k1: *mut u64, k2: *mut u64, k1_neg: *mut u64,
        k2_neg: *mut u64, n: usize, ld: usize, err: *mut u8) -> i64;
    pub fn p2e_limb_split(ctx: *mut P2eCtx, packed: *const u8, limbs: *mut u64, n: usize, ld: usize) -> i64;
    pub fn p2e_limb_pack(ctx: *mut P2eCtx, limbs: *const u64, packed: *mut u8, n: usize, ld: usize, err: *mut u8) -> i64;

    // ---- the targets other generators fill on the same path
    pub fn p2e_aux_witness_batch(ctx: *mut P2eCtx, program: i32, pky32: *const u8, cols: *const u64, ld: usize, aux: *mut u64,
        ld_aux: usize, n: usize, err: *mut u8) -> i64;
    pub fn p2e_aux_witness_compact_batch(ctx: *mut P2eCtx, program: i32, pky32: *const u8, narrow: *const u32,
        ld_narrow: usize, aux32: *mut u32, ld_aux: usize, n: usize, err: *mut u8) -> i64;
    pub fn p2e_aux_describe(program: i32, out: *mut P2eAuxDesc, cap: usize) -> i64;
    pub fn p2e_aux_num_cols(program: i32) -> i64;
    pub fn p2e_ux_witness_batch(ctx: *mut P2eCtx, program: i32, msg32: *const u8, r32: *const u8, s32: *const u8,
        pkx32: *const u8, pky32: *const u8, cols: *const u64, ld: usize, aux: *const u64, ld_aux: usize, ux: *mut c_void,
        ux_u32: i32, ld_ux: usize, n: usize, err: *mut u8) -> i64;
    pub fn p2e_ux_describe(program: i32, out: *mut P2eUxDesc, cap: usize) -> i64;
    pub fn p2e_ux_num_cols(program: i32) -> i64;

    // ---- wire-matrix assembly (rank 3)
    pub fn p2e_wire_map_create(ctx: *mut P2eCtx, program: i32, entries: *const P2eWireMapEntry, count: usize, num_wires: u32,
        degree: u32, out: *mut *mut P2eWireMap) -> i32;
    pub fn p2e_wire_map_destroy(ctx: *mut P2eCtx, map: *mut P2eWireMap);
    pub fn p2e_assemble_wires(ctx: *mut P2eCtx, map: *const P2eWireMap, cols: *const u64, ld: usize, aux: *const u64,
        ld_aux: usize, ux: *const c_void, ux_u32: i32, ld_ux: usize, gate: *const u64, ld_gate: usize, wires: *mut u64,
        wire_stride: usize, n: usize) -> i64;
    pub fn p2e_gate_internal_batch(ctx: *mut P2eCtx, program: i32, aux: *const u64, ld_aux: usize, gate: *mut u64,
        ld_gate: usize, n: usize) -> i64;
    pub fn p2e_gate_internal_num_cols(program: i32) -> i64;
    // ---- the same passes inside the compact container (u32 narrow matrix, u32 aux matrix)
    pub fn p2e_ux_witness_compact_batch(ctx: *mut P2eCtx, program: i32, msg32: *const u8, r32: *const u8, s32: *const u8,
        pkx32: *const u8, pky32: *const u8, narrow: *const u32, ld_narrow: usize, aux32: *const u32, ld_aux: usize,
        ux: *mut c_void, ux_u32: i32, ld_ux: usize, n: usize, err: *mut u8) -> i64;
    pub fn p2e_gate_internal_compact_batch(ctx: *mut P2eCtx, program: i32, aux32: *const u32, ld_aux: usize, gate: *mut u64,
        ld_gate: usize, n: usize) -> i64;
    pub fn p2e_assemble_wires_compact(ctx: *mut P2eCtx, map: *const P2eWireMap, narrow: *const u32, ld_narrow: usize,
        wide: *const u64, ld_wide: usize, aux32: *const u32, ld_aux: usize, ux: *const c_void, ux_u32: i32, ld_ux: usize,
        gate: *const u64, ld_gate: usize, wires: *mut u64, wire_stride: usize, n: usize) -> i64;

    // ---- column maps (host only)
    pub fn p2e_schedule_describe(program: i32, out: *mut P2eGenDesc, cap: usize) -> i64;
    pub fn p2e_schedule_num_cols(program: i32) -> i64;
    pub fn p2e_schedule_wiring(program: i32, out: *mut P2eGenWiring, cap: usize) -> i64;
    pub fn p2e_wiring_const(id: u32, out32: *mut u8) -> i32;
    pub fn p2e_compact_layout(program: i32, col_map: *mut u32, cap: usize, num_narrow: *mut u32, num_wide: *mut u32) -> i64;

    // ---- layout helpers
    pub fn p2e_columns_to_rows(ctx: *mut P2eCtx, cols: *const u64, ld: usize, n: usize, ncols: usize, rows: *mut u64,
        row_ld: usize) -> i64;
    pub fn p2e_columns_compact(ctx: *mut P2eCtx, program: i32, cols: *const u64, ld: usize, n: usize, narrow: *mut u32,
        ld_narrow: usize, wide: *mut u64, ld_wide: usize, err: *mut u8) -> i64;
    pub fn p2e_compact_to_rows(ctx: *mut P2eCtx, program: i32, narrow: *const u32, ld_narrow: usize, wide: *const u64,
        ld_wide: usize, n: usize, rows_narrow: *mut u32, row_ld_narrow: usize, rows_wide: *mut u64, row_ld_wide: usize) -> i64;

    // ---- key derivation and signing on either curve: curve/ecdsa.rs:16-20 to_public, :25-40 sign_message (nonce as an input)
    pub fn p2e_ecdsa_public_key_batch(ctx: *mut P2eCtx, curve: i32, plan: u32, sk32: *const u8, pkx32: *mut u8, pky32: *mut u8,
        n: usize, err: *mut u8) -> i64;
    pub fn p2e_ecdsa_sign_batch(ctx: *mut P2eCtx, curve: i32, plan: u32, msg32: *const u8, sk32: *const u8, k32: *const u8,
        r32: *mut u8, s32: *mut u8, n: usize, err: *mut u8) -> i64;
    // ---- public-key recovery from (msg, r, s, v), and the signer that also writes v (bit 0: parity of R.y, bit 1: R.x >= n)
    pub fn p2e_ecdsa_recover_batch(ctx: *mut P2eCtx, curve: i32, msg32: *const u8, r32: *const u8, s32: *const u8, v: *const u8,
        pkx32: *mut u8, pky32: *mut u8, n: usize, err: *mut u8) -> i64;
    pub fn p2e_ecdsa_sign_recoverable_batch(ctx: *mut P2eCtx, curve: i32, plan: u32, msg32: *const u8, sk32: *const u8,
        k32: *const u8, r32: *mut u8, s32: *mut u8, v: *mut u8, n: usize, err: *mut u8) -> i64;

    // ---- message hashing, RFC 6979 nonces, the deterministic signer and Ethereum addresses (nearest reference counterpart:
    // curve/ecdsa.rs:25-40 sign_message, which draws its nonce with rand(), :29-32)
    pub fn p2e_hash_batch(ctx: *mut P2eCtx, alg: i32, out_form: u32, data: *const u8, offsets: *const u64, out32: *mut u8,
        n: usize) -> i64;
    pub fn p2e_ecdsa_nonce_rfc6979_batch(ctx: *mut P2eCtx, curve: i32, msg32: *const u8, sk32: *const u8, k32: *mut u8,
        n: usize) -> i64;
    pub fn p2e_ecdsa_sign_deterministic_batch(ctx: *mut P2eCtx, curve: i32, plan: u32, msg32: *const u8, sk32: *const u8,
        r32: *mut u8, s32: *mut u8, v: *mut u8, n: usize, err: *mut u8) -> i64;
    pub fn p2e_eth_address_batch(ctx: *mut P2eCtx, pkx32: *const u8, pky32: *const u8, err: *const u8, addr20: *mut u8,
        n: usize) -> i64;

    // ---- keys and signatures in wire form: SEC1 keys, strict DER / compact signatures; err[i] is a P2E_WIRE_* code
    pub fn p2e_point_decode_batch(ctx: *mut P2eCtx, curve: i32, data: *const u8, offsets: *const u64, px32: *mut u8, py32: *mut u8,
        n: usize, err: *mut u8) -> i64;
    pub fn p2e_point_encode_batch(ctx: *mut P2eCtx, curve: i32, form: i32, px32: *const u8, py32: *const u8, out: *mut u8, n: usize,
        err: *mut u8) -> i64;
    pub fn p2e_sig_decode_batch(ctx: *mut P2eCtx, curve: i32, form: i32, flags: u32, data: *const u8, offsets: *const u64,
        r32: *mut u8, s32: *mut u8, v: *mut u8, n: usize, err: *mut u8) -> i64;
    pub fn p2e_sig_encode_batch(ctx: *mut P2eCtx, curve: i32, form: i32, flags: u32, r32: *const u8, s32: *const u8, v: *const u8,
        out: *mut u8, out_len: *mut u8, n: usize, err: *mut u8) -> i64;

    // ---- bucket-method multi-scalar multiplication sum k_i P_i (curve/curve_msm.rs msm_parallel / msm_execute); `plan`:
    // P2E_MSM_PLAN_WORDS words indexed by P2E_MSM_PLAN_*
    pub fn p2e_point_msm(ctx: *mut P2eCtx, curve: i32, window_bits: u32, k32: *const u8, px32: *const u8, py32: *const u8,
        n: usize, outx32: *mut u8, outy32: *mut u8, status: *mut u8, point_err: *mut u8) -> i64;
    pub fn p2e_point_msm_plan(curve: i32, n: usize, window_bits: u32, plan: *mut u64) -> i32;

    // ---- per-element point arithmetic: k P (plan: P2E_MUL_PLAN_*), a G + b P, P + Q; err[i] is a P2E_WIRE_* code
    pub fn p2e_point_mul_batch(ctx: *mut P2eCtx, curve: i32, plan: u32, k32: *const u8, px32: *const u8, py32: *const u8,
        outx32: *mut u8, outy32: *mut u8, n: usize, err: *mut u8) -> i64;
    pub fn p2e_point_lincomb_batch(ctx: *mut P2eCtx, curve: i32, plan: u32, a32: *const u8, b32: *const u8, px32: *const u8,
        py32: *const u8, outx32: *mut u8, outy32: *mut u8, n: usize, err: *mut u8) -> i64;
    pub fn p2e_point_add_batch(ctx: *mut P2eCtx, curve: i32, px32: *const u8, py32: *const u8, qx32: *const u8, qy32: *const u8,
        outx32: *mut u8, outy32: *mut u8, n: usize, err: *mut u8) -> i64;

    // ---- point tables: window tables of caller points, built once on the device (the handle is an opaque `void *` in the
    // header; bind.rs wraps it in `PointTable`)
    pub fn p2e_point_table_create(ctx: *mut P2eCtx, curve: i32, px32: *const u8, py32: *const u8, m: usize, point_err: *mut u8,
        out: *mut *mut c_void) -> i64;
    pub fn p2e_point_table_destroy(ctx: *mut P2eCtx, table: *mut c_void);
    pub fn p2e_point_table_num_points(table: *const c_void) -> i64;
    pub fn p2e_point_table_curve(table: *const c_void) -> i32;
    pub fn p2e_point_table_read_window(ctx: *mut P2eCtx, table: *const c_void, j: usize, w: i32, out1024: *mut u8) -> i32;
    pub fn p2e_point_table_mul_batch(ctx: *mut P2eCtx, table: *const c_void, idx: *const u32, k32: *const u8, outx32: *mut u8,
        outy32: *mut u8, n: usize, err: *mut u8) -> i64;
    pub fn p2e_point_table_lincomb_batch(ctx: *mut P2eCtx, table: *const c_void, idx: *const u32, a32: *const u8, b32: *const u8,
        outx32: *mut u8, outy32: *mut u8, n: usize, err: *mut u8) -> i64;
    pub fn p2e_ecdsa_verify_table_batch(ctx: *mut P2eCtx, table: *const c_void, idx: *const u32, msg32: *const u8, r32: *const u8,
        s32: *const u8, n: usize, err: *mut u8, valid: *mut u8) -> i64;

    // ---- BIP-340 Schnorr signatures on secp256k1: every argument is the standard's BIG-endian byte string (sig64 = r || s);
    // err[i] is a P2E_WIRE_* code; the aggregate call writes ONE verdict byte (seed32 must be unpredictable to the signers)
    pub fn p2e_schnorr_public_key_batch(ctx: *mut P2eCtx, sk32: *const u8, pk32: *mut u8, n: usize, err: *mut u8) -> i64;
    pub fn p2e_schnorr_sign_batch(ctx: *mut P2eCtx, msg32: *const u8, sk32: *const u8, aux32: *const u8, sig64: *mut u8, n: usize,
        err: *mut u8) -> i64;
    pub fn p2e_schnorr_verify_batch(ctx: *mut P2eCtx, msg32: *const u8, pk32: *const u8, sig64: *const u8, n: usize, err: *mut u8,
        valid: *mut u8) -> i64;
    pub fn p2e_xonly_decode_batch(ctx: *mut P2eCtx, pk32: *const u8, px32: *mut u8, py32: *mut u8, n: usize, err: *mut u8) -> i64;
    pub fn p2e_schnorr_verify_aggregate(ctx: *mut P2eCtx, msg32: *const u8, pk32: *const u8, sig64: *const u8, n: usize,
        seed32: *const u8, window_bits: u32, verdict: *mut u8, err: *mut u8) -> i64;

    // ---- BIP-32 key derivation and HASH160 on secp256k1: keys and coordinates little-endian, chain codes and hashes in their
    // standard's byte order; n_parents is 1 (one parent for the batch) or n; err[i] is a P2E_WIRE_* code
    pub fn p2e_bip32_master_batch(ctx: *mut P2eCtx, seed: *const u8, seed_len: usize, sk32: *mut u8, cc32: *mut u8, n: usize,
        err: *mut u8) -> i64;
    pub fn p2e_bip32_ckd_priv_batch(ctx: *mut P2eCtx, par_sk32: *const u8, par_cc32: *const u8, n_parents: usize, index: *const u32,
        sk32: *mut u8, cc32: *mut u8, n: usize, err: *mut u8) -> i64;
    pub fn p2e_bip32_ckd_pub_batch(ctx: *mut P2eCtx, par_pkx32: *const u8, par_pky32: *const u8, par_cc32: *const u8, n_parents: usize,
        index: *const u32, pkx32: *mut u8, pky32: *mut u8, cc32: *mut u8, n: usize, err: *mut u8) -> i64;
    pub fn p2e_key_hash160_batch(ctx: *mut P2eCtx, form: u32, pkx32: *const u8, pky32: *const u8, err_in: *const u8, out20: *mut u8,
        n: usize) -> i64;
    pub fn p2e_hash160_batch(ctx: *mut P2eCtx, data: *const u8, offsets: *const u64, out20: *mut u8, n: usize) -> i64;

    // ---- PBKDF2-HMAC-SHA512 and BIP-39 seeds: operands laid out as the data of p2e_hash_batch, n_x = 1 (one element for the
    // batch) or count; passphrase and pp_offsets null with n_passphrases = 0; the batch size is `count` (include/p2e.h says
    // why); err[i] is P2E_WIRE_BAD_LENGTH or 0.  iterations <= P2E_PBKDF2_MAX_ITERATIONS = 1 << 20; dk_len a multiple of 4 in 4 ..= 64
    pub fn p2e_pbkdf2_hmac_sha512_batch(ctx: *mut P2eCtx, password: *const u8, pw_offsets: *const u64, n_passwords: usize,
        salt: *const u8, salt_offsets: *const u64, n_salts: usize, iterations: u32, dk_len: usize, dk: *mut u8, count: usize,
        err: *mut u8) -> i64;
    pub fn p2e_bip39_seed_batch(ctx: *mut P2eCtx, mnemonic: *const u8, mn_offsets: *const u64, n_mnemonics: usize,
        passphrase: *const u8, pp_offsets: *const u64, n_passphrases: usize, seed64: *mut u8, count: usize, err: *mut u8) -> i64;

    // ---- Taproot (BIP-341) on secp256k1: every key, hash and tweak the standard's big-endian 32 bytes; root32 may be null
    // (BIP-86's key-path-only output); the batch size is `count` (include/p2e.h says why); err[i] is a P2E_WIRE_* code
    pub fn p2e_taproot_leaf_hash_batch(ctx: *mut P2eCtx, leaf_version: *const u8, script: *const u8, offsets: *const u64,
        leaf32: *mut u8, count: usize, err: *mut u8) -> i64;
    pub fn p2e_taproot_merkle_root_batch(ctx: *mut P2eCtx, leaf32: *const u8, path32: *const u8, depth: *const u8, max_depth: usize,
        root32: *mut u8, count: usize, err: *mut u8) -> i64;
    pub fn p2e_taproot_tweak_pubkey_batch(ctx: *mut P2eCtx, pk32: *const u8, root32: *const u8, out_pk32: *mut u8,
        out_parity: *mut u8, count: usize, err: *mut u8) -> i64;
    pub fn p2e_taproot_tweak_seckey_batch(ctx: *mut P2eCtx, sk32: *const u8, root32: *const u8, out_sk32: *mut u8, count: usize,
        err: *mut u8) -> i64;
    pub fn p2e_taproot_verify_commitment_batch(ctx: *mut P2eCtx, out_pk32: *const u8, out_parity: *const u8, pk32: *const u8,
        leaf32: *const u8, path32: *const u8, depth: *const u8, max_depth: usize, count: usize, err: *mut u8,
        valid: *mut u8) -> i64;

    // ---- silent payments (BIP-352) on secp256k1: points and secret keys little-endian 32 bytes, outpoints, input hashes, x-only
    // outputs and tweaks the standard's big-endian strings; scan_sk32 / spend_pk* are ONE element, label_* n_labels elements;
    // input_hash32 of the scan may be null; out_offsets counts outputs; the batch size is `count`; err[i] is a P2E_WIRE_* code
    pub fn p2e_sp_input_hash_batch(ctx: *mut P2eCtx, outpoint36: *const u8, ax32: *const u8, ay32: *const u8, input_hash32: *mut u8,
        count: usize, err: *mut u8) -> i64;
    pub fn p2e_sp_label_batch(ctx: *mut P2eCtx, scan_sk32: *const u8, label_index: *const u32, label_tweak32: *mut u8,
        label_x32: *mut u8, label_y32: *mut u8, count: usize, err: *mut u8) -> i64;
    pub fn p2e_sp_send_batch(ctx: *mut P2eCtx, a_sk32: *const u8, input_hash32: *const u8, scan_pkx32: *const u8,
        scan_pky32: *const u8, spend_pkx32: *const u8, spend_pky32: *const u8, k: *const u32, out_pk32: *mut u8, count: usize,
        err: *mut u8) -> i64;
    pub fn p2e_sp_scan_batch(ctx: *mut P2eCtx, scan_sk32: *const u8, spend_pkx32: *const u8, spend_pky32: *const u8,
        label_x32: *const u8, label_y32: *const u8, n_labels: usize, ax32: *const u8, ay32: *const u8, input_hash32: *const u8,
        outputs32: *const u8, out_offsets: *const u64, max_hits: usize, n_hits: *mut u8, hit_output: *mut u32, hit_label: *mut u8,
        hit_tweak32: *mut u8, count: usize, err: *mut u8) -> i64;

    // ---- a P + b Q per element (either curve) and DLEQ proofs (BIP-374) on secp256k1: points and a_sk32 little-endian,
    // aux_rand32 / msg32 byte strings, proof64 = bytes32(e) || bytes32(s) big-endian; msg32, cx32 / cy32 nullable
    pub fn p2e_point_lincomb2_batch(ctx: *mut P2eCtx, curve: i32, plan: u32, a32: *const u8, b32: *const u8, px32: *const u8,
        py32: *const u8, qx32: *const u8, qy32: *const u8, outx32: *mut u8, outy32: *mut u8, count: usize, err: *mut u8) -> i64;
    pub fn p2e_dleq_prove_batch(ctx: *mut P2eCtx, a_sk32: *const u8, bx32: *const u8, by32: *const u8, aux_rand32: *const u8,
        msg32: *const u8, proof64: *mut u8, cx32: *mut u8, cy32: *mut u8, count: usize, err: *mut u8) -> i64;
    pub fn p2e_dleq_verify_batch(ctx: *mut P2eCtx, ax32: *const u8, ay32: *const u8, bx32: *const u8, by32: *const u8,
        cx32: *const u8, cy32: *const u8, proof64: *const u8, msg32: *const u8, count: usize, err: *mut u8,
        valid: *mut u8) -> i64;

    // ---- MuSig2 (BIP-327) on secp256k1: points, secret keys and nonces little-endian 32-byte values (pubnonce128 / aggnonce128 =
    // x(R_1) || y(R_1) || x(R_2) || y(R_2), secnonce64 = k_1 || k_2), tweaks, messages, partial signatures, agg_pk32 and sig64 the
    // standard's big-endian strings; keyagg192 and session128 are the records of include/p2e.h; key_offsets (count + 1) counts
    // signers; tweak32 may be null in mode 2, session_index may be null; the batch size is `count`; err[i] is a P2E_WIRE_* code
    pub fn p2e_musig_key_agg_batch(ctx: *mut P2eCtx, pkx32: *const u8, pky32: *const u8, key_offsets: *const u64, keyagg192: *mut u8,
        agg_pk32: *mut u8, count: usize, err: *mut u8) -> i64;
    pub fn p2e_musig_apply_tweak_batch(ctx: *mut P2eCtx, keyagg192_in: *const u8, tweak32: *const u8, mode: i32, keyagg192_out: *mut u8,
        agg_pk32: *mut u8, count: usize, err: *mut u8) -> i64;
    pub fn p2e_musig_nonce_agg_batch(ctx: *mut P2eCtx, pubnonce128: *const u8, key_offsets: *const u64, aggnonce128: *mut u8,
        count: usize, err: *mut u8) -> i64;
    pub fn p2e_musig_session_batch(ctx: *mut P2eCtx, keyagg192: *const u8, aggnonce128: *const u8, msg32: *const u8,
        session128: *mut u8, count: usize, err: *mut u8) -> i64;
    pub fn p2e_musig_partial_sign_batch(ctx: *mut P2eCtx, secnonce64: *const u8, sk32: *const u8, keyagg192: *const u8,
        session128: *const u8, psig32: *mut u8, count: usize, err: *mut u8) -> i64;
    pub fn p2e_musig_partial_verify_batch(ctx: *mut P2eCtx, psig32: *const u8, pubnonce128: *const u8, pkx32: *const u8,
        pky32: *const u8, session_index: *const u32, keyagg192: *const u8, session128: *const u8, n_sessions: usize, count: usize,
        err: *mut u8, valid: *mut u8) -> i64;
    pub fn p2e_musig_sig_agg_batch(ctx: *mut P2eCtx, psig32: *const u8, key_offsets: *const u64, keyagg192: *const u8,
        session128: *const u8, sig64: *mut u8, count: usize, err: *mut u8) -> i64;

    // ---- synthetic inputs (host only): valid signatures per curve/ecdsa.rs:25-40
    pub fn p2e_synth_signatures(seed: u64, first: usize, n: usize, msg32: *mut u8, r32: *mut u8, s32: *mut u8, pkx32: *mut u8,
        pky32: *mut u8) -> i32;
    pub fn p2e_synth_signatures_curve(curve: i32, seed: u64, first: usize, n: usize, msg32: *mut u8, r32: *mut u8, s32: *mut u8,
        pkx32: *mut u8, pky32: *mut u8) -> i32;

    // ---- curve programs (rank 4): curve_scalar_mul_windowed / curve_scalar_mul on either curve, verify_p256_message_circuit
    pub fn p2e_curve_program_create(ctx: *mut P2eCtx, kind: i32, curve: i32, blind_x32: *const u8, blind_y32: *const u8,
        out: *mut *mut P2eCurveProgram) -> i32;
    pub fn p2e_curve_program_destroy(ctx: *mut P2eCtx, prog: *mut P2eCurveProgram);
    pub fn p2e_curve_program_num_cols(prog: *const P2eCurveProgram) -> i64;
    pub fn p2e_curve_program_num_aux_cols(prog: *const P2eCurveProgram) -> i64;
    pub fn p2e_curve_program_scratch_bytes(prog: *const P2eCurveProgram, n: usize) -> usize;
    pub fn p2e_curve_program_describe(prog: *const P2eCurveProgram, out: *mut P2eGenDesc, cap: usize) -> i64;
    pub fn p2e_curve_program_wiring(prog: *const P2eCurveProgram, out: *mut P2eGenWiring, cap: usize) -> i64;
    pub fn p2e_curve_program_aux_describe(prog: *const P2eCurveProgram, out: *mut P2eAuxDesc, cap: usize) -> i64;
    pub fn p2e_curve_program_const(prog: *const P2eCurveProgram, id: u32, out32: *mut u8) -> i32;
    pub fn p2e_curve_program_num_gate_cols(prog: *const P2eCurveProgram) -> i64;
    pub fn p2e_curve_program_num_ux_cols(prog: *const P2eCurveProgram) -> i64;
    pub fn p2e_curve_program_ux_describe(prog: *const P2eCurveProgram, out: *mut P2eUxDesc, cap: usize) -> i64;
    pub fn p2e_curve_program_aux_witness_batch(ctx: *mut P2eCtx, prog: *const P2eCurveProgram, msg32: *const u8, r32: *const u8,
        s32: *const u8, pkx32: *const u8, pky32: *const u8, cols: *const u64, ld: usize, aux: *mut u64, ld_aux: usize, n: usize,
        err: *mut u8) -> i64;
    pub fn p2e_curve_program_gate_internal_batch(ctx: *mut P2eCtx, prog: *const P2eCurveProgram, aux: *const u64, ld_aux: usize,
        gate: *mut u64, ld_gate: usize, n: usize) -> i64;
    pub fn p2e_curve_program_ux_witness_batch(ctx: *mut P2eCtx, prog: *const P2eCurveProgram, msg32: *const u8, r32: *const u8,
        s32: *const u8, pkx32: *const u8, pky32: *const u8, cols: *const u64, ld: usize, aux: *const u64, ld_aux: usize,
        ux: *mut c_void, ux_u32: i32, ld_ux: usize, n: usize, err: *mut u8) -> i64;
    pub fn p2e_curve_program_wire_map_create(ctx: *mut P2eCtx, prog: *const P2eCurveProgram, entries: *const P2eWireMapEntry,
        count: usize, num_wires: u32, degree: u32, out: *mut *mut P2eWireMap) -> i32;
    pub fn p2e_p256_verify_batch(ctx: *mut P2eCtx, prog: *const P2eCurveProgram, msg32: *const u8, r32: *const u8, s32: *const u8,
        pkx32: *const u8, pky32: *const u8, n: usize, err: *mut u8, valid: *mut u8) -> i64;
    pub fn p2e_curve_mul_witness_batch(ctx: *mut P2eCtx, prog: *const P2eCurveProgram, px32: *const u8, py32: *const u8,
        k32: *const u8, cols: *mut u64, n: usize, ld: usize, err: *mut u8, valid: *mut u8) -> i64;
    pub fn p2e_p256_verify_witness_batch(ctx: *mut P2eCtx, prog: *const P2eCurveProgram, msg32: *const u8, r32: *const u8,
        s32: *const u8, pkx32: *const u8, pky32: *const u8, cols: *mut u64, n: usize, ld: usize, err: *mut u8,
        valid: *mut u8) -> i64;
    // curve_msm_circuit(p, q, n, m) (P2E_CP_MSM); the fixed-base program fills through p2e_curve_mul_witness_batch with
    // null points
    pub fn p2e_curve_msm_witness_batch(ctx: *mut P2eCtx, prog: *const P2eCurveProgram, px32: *const u8, py32: *const u8,
        qx32: *const u8, qy32: *const u8, n32: *const u8, m32: *const u8, cols: *mut u64, n: usize, ld: usize, err: *mut u8,
        valid: *mut u8) -> i64;
    // the same two fills into the compact container (u32 narrow + u64 wide matrices), and its column map
    pub fn p2e_curve_mul_witness_compact_batch(ctx: *mut P2eCtx, prog: *const P2eCurveProgram, px32: *const u8, py32: *const u8,
        k32: *const u8, narrow: *mut u32, ld_narrow: usize, wide: *mut u64, ld_wide: usize, n: usize, err: *mut u8,
        valid: *mut u8) -> i64;
    pub fn p2e_p256_verify_witness_compact_batch(ctx: *mut P2eCtx, prog: *const P2eCurveProgram, msg32: *const u8, r32: *const u8,
        s32: *const u8, pkx32: *const u8, pky32: *const u8, narrow: *mut u32, ld_narrow: usize, wide: *mut u64, ld_wide: usize,
        n: usize, err: *mut u8, valid: *mut u8) -> i64;
    pub fn p2e_curve_msm_witness_compact_batch(ctx: *mut P2eCtx, prog: *const P2eCurveProgram, px32: *const u8, py32: *const u8,
        qx32: *const u8, qy32: *const u8, n32: *const u8, m32: *const u8, narrow: *mut u32, ld_narrow: usize, wide: *mut u64,
        ld_wide: usize, n: usize, err: *mut u8, valid: *mut u8) -> i64;
    pub fn p2e_curve_program_compact_layout(prog: *const P2eCurveProgram, col_map: *mut u32, cap: usize, num_narrow: *mut u32,
        num_wide: *mut u32) -> i64;
    pub fn p2e_curve_msm_ux_witness_batch(ctx: *mut P2eCtx, prog: *const P2eCurveProgram, px32: *const u8, py32: *const u8,
        qx32: *const u8, qy32: *const u8, n32: *const u8, m32: *const u8, cols: *const u64, ld: usize, aux: *const u64,
        ld_aux: usize, ux: *mut c_void, ux_u32: i32, ld_ux: usize, n: usize, err: *mut u8) -> i64;
    pub fn p2e_curve_program_aux_witness_compact_batch(ctx: *mut P2eCtx, prog: *const P2eCurveProgram, msg32: *const u8,
        r32: *const u8, s32: *const u8, pkx32: *const u8, pky32: *const u8, narrow: *const u32, ld_narrow: usize,
        aux32: *mut u32, ld_aux: usize, n: usize, err: *mut u8) -> i64;
    pub fn p2e_curve_program_gate_internal_compact_batch(ctx: *mut P2eCtx, prog: *const P2eCurveProgram, aux32: *const u32,
        ld_aux: usize, gate: *mut u64, ld_gate: usize, n: usize) -> i64;
    pub fn p2e_curve_program_ux_witness_compact_batch(ctx: *mut P2eCtx, prog: *const P2eCurveProgram, msg32: *const u8,
        r32: *const u8, s32: *const u8, pkx32: *const u8, pky32: *const u8, qx32: *const u8, qy32: *const u8,
        narrow: *const u32, ld_narrow: usize, aux32: *const u32, ld_aux: usize, ux: *mut c_void, ux_u32: i32, ld_ux: usize,
        n: usize, err: *mut u8) -> i64;
}
