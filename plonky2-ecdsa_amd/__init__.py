"""plonky2-ecdsa_amd: MI355X-native batch witness generation for plonky2's secp256k1 ECDSA gadget.

Python host side of the C ABI in ``include/p2e.h`` (``libp2e_hip.so``, hand-written HIP for gfx950).
The names mirror the reference crate's generator / gadget interface for this path
(Weobe/plonky2-ecdsa: ``MulNonnativeGenerator``, ``NonNative{Addition,Subtraction,MultipleAdds,
Inverse}Generator``, ``GLVDecompositionGenerator``, ``glv_mul``, ``verify_secp256k1_message_circuit``),
with batches instead of single targets:

* Goldilocks columns are ``(num_cols, n)`` uint64 arrays / tensors, column-major over the batch.
* 256-bit inputs are ``(n, 32)`` uint8 little-endian.

There is NO CPU fallback: without the HIP extension and a GPU every compute call raises.
torch is used only for device memory / streams / torch.distributed plumbing.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

# HIP multiplexes streams onto GPU_MAX_HW_QUEUES hardware queues (default 4) and kernels sharing a queue
# run in order.  The fused entry points pipeline over three streams per context; with 8 queues they never
# collide with the caller's own streams (+5 % on the 2^16 verify batch).  Read once, when the HIP runtime
# starts: this only has an effect if nothing initialised HIP before this import.
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
# P2E_LIB: an alternative build of the same library (A/B experiments under tools/); never set in production
LIB_PATH = os.environ.get("P2E_LIB") or os.path.join(_HERE, "libp2e_hip.so")

FIELD_BASE = 0    # plonky2 Secp256K1Base
FIELD_SCALAR = 1  # plonky2 Secp256K1Scalar
FIELD_P256_BASE, FIELD_P256_SCALAR = 2, 3   # the crate's P256Base / P256Scalar (single-generator entry points)
ERR_LIMB_RANGE, ERR_VALUE_GE_2_256, ERR_INVERSE_OF_ZERO, ERR_CARRY_RANGE, ERR_QUOTIENT_RANGE = 1, 2, 4, 8, 16
ERR_DIVISION_BY_ZERO = 32
ERR_POINT_AT_INFINITY = 64   # ecdsa_public_key_batch: sk = 0 (mod n)
ERR_NOT_RECOVERABLE = 128    # ecdsa_recover_batch: (r, s, v) names no curve point
SIGN_PLAN_AUTO, SIGN_PLAN_LANE, SIGN_PLAN_QUAD = 0, 1, 2   # include/p2e.h P2E_SIGN_PLAN_*
HASH_SHA256, HASH_SHA256D, HASH_KECCAK256 = 0, 1, 2        # include/p2e.h P2E_HASH_*
DIGEST_BYTES, DIGEST_SCALAR = 0, 1                         # include/p2e.h P2E_DIGEST_*
MSM_WINDOW_AUTO, MSM_WINDOW_MIN, MSM_WINDOW_MAX = 0, 4, 12  # include/p2e.h P2E_MSM_WINDOW_*
MSM_OK, MSM_NEUTRAL, MSM_BAD_POINT = 0, 1, 2               # include/p2e.h P2E_MSM_* (the status byte of point_msm)
# include/p2e.h P2E_WIRE_*: the err CODE (not a bit set) of point_decode_batch, point_encode_batch, sig_decode_batch, sig_encode_batch
(WIRE_OK, WIRE_BAD_LENGTH, WIRE_BAD_PREFIX, WIRE_COORD_RANGE, WIRE_NOT_ON_CURVE, WIRE_INFINITY, WIRE_DER_SYNTAX, WIRE_DER_INTEGER,
 WIRE_SCALAR_RANGE, WIRE_HIGH_S) = range(10)
WIRE_BAD_INDEX = 10                                        # the three point-table calls: idx[i] >= the table's point count
POINT_TABLE_MAX_POINTS, POINT_TABLE_BYTES_PER_POINT = 65536, 67584   # include/p2e.h P2E_POINT_TABLE_*
MUL_PLAN_AUTO, MUL_PLAN_PLAIN, MUL_PLAN_GLV = 0, 1, 2       # include/p2e.h P2E_MUL_PLAN_* (point_mul_batch, point_lincomb_batch)
MUSIG_MAX_SIGNERS = 1024                                   # include/p2e.h P2E_MUSIG_MAX_SIGNERS
MUSIG_TWEAK_PLAIN, MUSIG_TWEAK_XONLY, MUSIG_TWEAK_TAPROOT = 0, 1, 2   # include/p2e.h P2E_MUSIG_TWEAK_*
SEC1_COMPRESSED, SEC1_UNCOMPRESSED = 0, 1                  # include/p2e.h P2E_SEC1_*
SIG_DER, SIG_COMPACT64, SIG_COMPACT65 = 0, 1, 2            # include/p2e.h P2E_SIG_*
SIG_REQUIRE_LOW_S, SIG_NORMALIZE_S = 1, 2
SIG_DER_STRIDE = 72
CTX_HOST_POINTERS, CTX_ASYNC, CTX_PHASE_TIMING = 1, 2, 4
VERIFY_COLS = 82615
GLV_MUL_COLS = 65243
VERIFY_AUX_COLS = 8959      # built-in-generator columns (include/p2e.h p2e_aux_witness_batch)
GLV_MUL_AUX_COLS = 4738
VERIFY_UX_COLS = 249385     # constraint-block (U29 gate) columns (include/p2e.h p2e_ux_witness_batch)
GLV_MUL_UX_COLS = 194361
VERIFY_GATE_COLS = 10703    # gate-internal values of the built-in gates (include/p2e.h p2e_gate_internal_batch)
GLV_MUL_GATE_COLS = 5621
PROGRAM_VERIFY, PROGRAM_GLV_MUL = 0, 1
# curve programs (include/p2e.h P2E_CURVE_* / P2E_CP_*)
CURVE_SECP256K1, CURVE_P256 = 0, 1
CP_WINDOWED_MUL, CP_SCALAR_MUL, CP_VERIFY, CP_MSM, CP_FIXED_BASE_MUL = 1, 2, 3, 4, 5
WINDOWED_MUL_COLS, SCALAR_MUL_COLS, P256_VERIFY_COLS, MSM_COLS, FIXED_BASE_MUL_COLS = 98185, 139354, 115557, 112309, 16797

# every symbol include/p2e.h declares
EXPORTS = (
    "p2e_ctx_create", "p2e_ctx_destroy", "p2e_sync", "p2e_last_error", "p2e_scratch_bytes", "p2e_last_phase_ms",
    "p2e_segments_describe", "p2e_segment_stream_wait", "p2e_segment_sync",
    "p2e_mul_witness_batch", "p2e_checksum_witness_batch", "p2e_add_witness_batch", "p2e_sub_witness_batch",
    "p2e_add_many_witness_batch", "p2e_inv_witness_batch", "p2e_glv_decompose_batch", "p2e_limb_split",
    "p2e_limb_pack", "p2e_ecdsa_verify_witness_batch", "p2e_glv_mul_witness_batch", "p2e_columns_to_rows",
    "p2e_schedule_describe", "p2e_schedule_wiring", "p2e_wiring_const", "p2e_ux_witness_batch", "p2e_ux_describe", "p2e_ux_num_cols",
    "p2e_wire_map_create", "p2e_wire_map_destroy", "p2e_assemble_wires", "p2e_gate_internal_batch", "p2e_gate_internal_num_cols",
    "p2e_schedule_num_cols", "p2e_synth_signatures", "p2e_aux_witness_batch", "p2e_aux_describe", "p2e_aux_num_cols",
    "p2e_compact_layout", "p2e_columns_compact", "p2e_ecdsa_verify_witness_compact_batch",
    "p2e_glv_mul_witness_compact_batch", "p2e_aux_witness_compact_batch", "p2e_compact_to_rows", "p2e_ecdsa_verify_batch", "p2e_biguint_div_rem_batch",
    "p2e_curve_program_create", "p2e_curve_program_destroy", "p2e_curve_program_num_cols", "p2e_curve_program_num_aux_cols",
    "p2e_curve_program_scratch_bytes", "p2e_curve_program_describe", "p2e_curve_program_wiring", "p2e_curve_program_aux_describe",
    "p2e_curve_program_const", "p2e_curve_mul_witness_batch", "p2e_p256_verify_witness_batch", "p2e_synth_signatures_curve",
    "p2e_curve_program_num_gate_cols", "p2e_curve_program_num_ux_cols", "p2e_curve_program_ux_describe",
    "p2e_curve_program_aux_witness_batch", "p2e_curve_program_gate_internal_batch", "p2e_curve_program_ux_witness_batch",
    "p2e_curve_program_wire_map_create", "p2e_p256_verify_batch",
    "p2e_curve_mul_witness_compact_batch", "p2e_p256_verify_witness_compact_batch", "p2e_curve_program_compact_layout",
    "p2e_curve_msm_witness_batch", "p2e_curve_msm_witness_compact_batch",
    "p2e_ux_witness_compact_batch", "p2e_gate_internal_compact_batch", "p2e_assemble_wires_compact",
    "p2e_curve_program_aux_witness_compact_batch", "p2e_curve_program_gate_internal_compact_batch",
    "p2e_curve_program_ux_witness_compact_batch", "p2e_curve_msm_ux_witness_batch",
    "p2e_ecdsa_public_key_batch", "p2e_ecdsa_sign_batch",
    "p2e_ecdsa_recover_batch", "p2e_ecdsa_sign_recoverable_batch",
    "p2e_hash_batch", "p2e_ecdsa_nonce_rfc6979_batch", "p2e_ecdsa_sign_deterministic_batch", "p2e_eth_address_batch",
    "p2e_point_msm", "p2e_point_msm_plan",
    "p2e_point_mul_batch", "p2e_point_lincomb_batch", "p2e_point_add_batch",
    "p2e_point_decode_batch", "p2e_point_encode_batch", "p2e_sig_decode_batch", "p2e_sig_encode_batch",
    "p2e_point_table_create", "p2e_point_table_destroy", "p2e_point_table_num_points", "p2e_point_table_curve",
    "p2e_point_table_read_window", "p2e_point_table_mul_batch", "p2e_point_table_lincomb_batch", "p2e_ecdsa_verify_table_batch",
    "p2e_schnorr_public_key_batch", "p2e_schnorr_sign_batch", "p2e_schnorr_verify_batch", "p2e_xonly_decode_batch",
    "p2e_schnorr_verify_aggregate",
    "p2e_bip32_master_batch", "p2e_bip32_ckd_priv_batch", "p2e_bip32_ckd_pub_batch", "p2e_key_hash160_batch", "p2e_hash160_batch",
    "p2e_pbkdf2_hmac_sha512_batch", "p2e_bip39_seed_batch",
    "p2e_taproot_leaf_hash_batch", "p2e_taproot_merkle_root_batch", "p2e_taproot_tweak_pubkey_batch", "p2e_taproot_tweak_seckey_batch",
    "p2e_taproot_verify_commitment_batch",
    "p2e_sp_input_hash_batch", "p2e_sp_label_batch", "p2e_sp_send_batch", "p2e_sp_scan_batch",
    "p2e_point_lincomb2_batch", "p2e_dleq_prove_batch", "p2e_dleq_verify_batch",
    "p2e_musig_key_agg_batch", "p2e_musig_apply_tweak_batch", "p2e_musig_nonce_agg_batch", "p2e_musig_session_batch",
    "p2e_musig_partial_sign_batch", "p2e_musig_partial_verify_batch", "p2e_musig_sig_agg_batch",
)


class P2EError(RuntimeError):
    pass


def build(verbose: bool = False, extra_flags=(), out: str | None = None) -> str:
    """Compile the HIP extension in-tree for gfx950 (hipcc cross-compiles without a GPU).  csrc/p2e_hip.hip is ONE source
    compiled as four translation units side by side (-DP2E_PART=0..3, see the top of the file) and linked into
    libp2e_hip.so.  ``extra_flags`` / ``out``: experimental builds for tools/ (never the product library)."""
    from concurrent.futures import ThreadPoolExecutor
    src = os.path.join(_HERE, "csrc", "p2e_hip.hip")
    lib_path = out or LIB_PATH
    deps = [os.path.join(_HERE, "csrc", f) for f in os.listdir(os.path.join(_HERE, "csrc"))]
    deps.append(os.path.join(_ROOT, "include", "p2e.h"))
    if not extra_flags and os.path.exists(lib_path) and all(os.path.getmtime(lib_path) >= os.path.getmtime(d) for d in deps):
        return lib_path
    objdir = os.path.join(_HERE, "build", os.path.basename(lib_path))
    os.makedirs(objdir, exist_ok=True)
    common = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fopenmp", *extra_flags]

    def compile_part(part):
        obj = os.path.join(objdir, f"part{part}.o")
        cmd = common + [f"-DP2E_PART={part}", "-c", "-o", obj, src]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
        return obj

    with ThreadPoolExecutor(max_workers=4) as ex:
        objs = list(ex.map(compile_part, range(4)))
    cmd = ["hipcc", "--offload-arch=gfx950", "-shared", "-fPIC", "-fopenmp", "-o", lib_path, *objs]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return lib_path


_lib = None


class _GenDesc(C.Structure):
    _fields_ = [("kind", C.c_int32), ("field", C.c_int32), ("first_col", C.c_uint32), ("num_cols", C.c_uint32),
                ("label", C.c_char * 48)]


def lib():
    """Load libp2e_hip.so (fails loudly if it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise P2EError(f"{LIB_PATH} is missing: run __graft_entry__.build() (there is no CPU fallback)")
        # torch ships its own libamdhip64 / libhsa-runtime64.  Import it FIRST so that libp2e_hip.so resolves
        # its libamdhip64.so.7 dependency to the runtime torch already loaded: device pointers and streams
        # are only meaningful inside one HIP runtime, and a second HSA runtime in the process finds no GPU
        # ("No HIP GPUs are available").
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        _lib = C.CDLL(LIB_PATH)
        experimental = bool(os.environ.get("P2E_LIB"))   # an A/B build under tools/ may predate newer entry points
        for name in EXPORTS:
            if experimental and not hasattr(_lib, name):
                continue
            getattr(_lib, name)  # AttributeError if a declared symbol is not exported
        _lib.p2e_last_error.restype = C.c_char_p
        _lib.p2e_scratch_bytes.restype = C.c_size_t
        _lib.p2e_scratch_bytes.argtypes = [C.c_int, C.c_size_t]
        for name in EXPORTS:
            if experimental and not hasattr(_lib, name):
                continue
            if name.endswith("_batch") or name in ("p2e_point_msm", "p2e_schnorr_verify_aggregate", "p2e_point_table_create", "p2e_point_table_num_points", "p2e_limb_split", "p2e_limb_pack", "p2e_columns_to_rows", "p2e_schedule_describe",
                                                   "p2e_schedule_num_cols", "p2e_aux_describe", "p2e_aux_num_cols", "p2e_compact_layout",
                                                   "p2e_columns_compact", "p2e_compact_to_rows", "p2e_curve_program_num_cols",
                                                   "p2e_curve_program_num_aux_cols", "p2e_curve_program_describe",
                                                   "p2e_curve_program_wiring", "p2e_curve_program_aux_describe",
                                                   "p2e_curve_program_num_gate_cols", "p2e_curve_program_num_ux_cols",
                                                   "p2e_curve_program_ux_describe", "p2e_curve_program_compact_layout",
                                                   "p2e_assemble_wires", "p2e_assemble_wires_compact"):
                getattr(_lib, name).restype = C.c_long
        _lib.p2e_curve_program_scratch_bytes.restype = C.c_size_t
        if hasattr(_lib, "p2e_point_table_destroy"):
            _lib.p2e_point_table_destroy.restype = None
            _lib.p2e_point_table_destroy.argtypes = [C.c_void_p, C.c_void_p]
            _lib.p2e_point_table_num_points.argtypes = _lib.p2e_point_table_curve.argtypes = [C.c_void_p]
    return _lib


def _ld(a):
    """Row stride, in elements, of a 2-D column matrix (numpy or torch): what the C ABI calls `ld`.  A view of a
    wider matrix (e.g. the padded output of ecdsa_verify_witness_batch) carries its stride with it; the inner
    (batch) dimension must be dense."""
    if isinstance(a, np.ndarray):
        if a.ndim != 2 or (a.shape[1] > 1 and a.strides[1] != a.itemsize):
            raise P2EError("column matrices must be 2-D with a dense batch dimension")
        return a.strides[0] // a.itemsize if a.shape[0] > 1 else max(a.shape[1], a.strides[0] // a.itemsize)
    if a.dim() != 2 or (a.shape[1] > 1 and a.stride(1) != 1):
        raise P2EError("column matrices must be 2-D with a dense batch dimension")
    return a.stride(0) if a.shape[0] > 1 else max(a.shape[1], a.stride(0))


def _dense(n, *arrays):
    """the single-generator entry points share ONE ld between inputs and outputs: inputs must be dense (k, n)"""
    for a in arrays:
        if _ld(a.reshape(-1, a.shape[-1]) if a.ndim == 3 else a) != n:
            raise P2EError("pass contiguous (k, n) limb-column arrays")


def _ptr(a):
    """device pointer of a torch tensor / host pointer of a numpy array / None"""
    if a is None:
        return C.c_void_p(0)
    if isinstance(a, np.ndarray):
        return a.ctypes.data_as(C.c_void_p)
    return C.c_void_p(a.data_ptr())


def _is_u32(a):
    return (a.dtype == np.uint32) if isinstance(a, np.ndarray) else (a.element_size() == 4)


def schedule_describe(program: int = PROGRAM_VERIFY):
    """Column map: list of (kind, field, first_col, num_cols, label) in generator registration order."""
    L = lib()
    n = L.p2e_schedule_describe(C.c_int(program), None, C.c_size_t(0))
    arr = (_GenDesc * n)()
    L.p2e_schedule_describe(C.c_int(program), arr, C.c_size_t(n))
    kinds = ("add", "sub", "add_many", "mul", "inv", "glv")
    return [(kinds[d.kind], d.field, d.first_col, d.num_cols, d.label.decode()) for d in arr]


SRC_AUX, SRC_INPUT, SRC_CONST = 0x20000000, 0x40000000, 0x80000000
INPUT_SLOTS = ("pky", "pkx", "msg", "r", "s")


class _GenWiring(C.Structure):
    _fields_ = [("num_operands", C.c_int32), ("src", C.c_uint32 * 4), ("num_limbs", C.c_uint8 * 4), ("range_check", C.c_int32)]


def schedule_wiring(program: int = PROGRAM_VERIFY):
    """Operand wiring per generator (include/p2e.h p2e_schedule_wiring): list of ([(src, num_limbs), ...], range_check)
    in the order of schedule_describe."""
    L = lib()
    L.p2e_schedule_wiring.restype = C.c_long
    n = L.p2e_schedule_wiring(C.c_int(program), None, C.c_size_t(0))
    arr = (_GenWiring * n)()
    L.p2e_schedule_wiring(C.c_int(program), arr, C.c_size_t(n))
    return [([(int(w.src[k]), int(w.num_limbs[k])) for k in range(w.num_operands)], bool(w.range_check)) for w in arr]


def wiring_const(const_id: int):
    """(value, num_limbs) of circuit constant `const_id` (SRC_CONST | const_id in schedule_wiring)."""
    buf = (C.c_uint8 * 32)()
    nl = lib().p2e_wiring_const(C.c_uint32(const_id), buf)
    if nl < 0:
        raise P2EError("unknown constant id")
    return int.from_bytes(bytes(buf), "little"), int(nl)


class _UxDesc(C.Structure):
    _fields_ = [("first_col", C.c_uint32), ("num_cols", C.c_uint32)]


def ux_describe(program: int = PROGRAM_VERIFY):
    """Per generator (order of schedule_describe): (first_col, num_cols) of its block in the constraint-block matrix."""
    L = lib()
    L.p2e_ux_describe.restype = C.c_long
    n = L.p2e_ux_describe(C.c_int(program), None, C.c_size_t(0))
    arr = (_UxDesc * n)()
    L.p2e_ux_describe(C.c_int(program), arr, C.c_size_t(n))
    return [(int(d.first_col), int(d.num_cols)) for d in arr]


def ux_num_cols(program: int = PROGRAM_VERIFY) -> int:
    L = lib()
    L.p2e_ux_num_cols.restype = C.c_long
    return int(L.p2e_ux_num_cols(C.c_int(program)))


def schedule_num_cols(program: int = PROGRAM_VERIFY) -> int:
    return int(lib().p2e_schedule_num_cols(C.c_int(program)))


class _AuxDesc(C.Structure):
    _fields_ = [("kind", C.c_int32), ("first_col", C.c_uint32), ("num_cols", C.c_uint32), ("label", C.c_char * 48)]


def aux_describe(program: int = PROGRAM_VERIFY):
    """Column map of the built-in-generator columns: (kind, first_col, num_cols, label) in gadget order."""
    L = lib()
    n = L.p2e_aux_describe(C.c_int(program), None, C.c_size_t(0))
    arr = (_AuxDesc * n)()
    L.p2e_aux_describe(C.c_int(program), arr, C.c_size_t(n))
    kinds = ("split4", "split2", "fixed_base_window", "msm_digit", "conditional_neg")
    return [(kinds[d.kind], d.first_col, d.num_cols, d.label.decode()) for d in arr]


COMPACT_WIDE = 0x80000000


def compact_layout(program: int = PROGRAM_VERIFY):
    """(col_map, num_narrow, num_wide) of the compact transfer container (include/p2e.h p2e_columns_compact):
    col_map[c] = index of witness column c in the u32 narrow matrix, or COMPACT_WIDE | index in the u64 wide one."""
    L = lib()
    ncols = schedule_num_cols(program)
    m = np.zeros(ncols, dtype=np.uint32)
    nn, nw = C.c_uint32(), C.c_uint32()
    L.p2e_compact_layout(C.c_int(program), _ptr(m), C.c_size_t(ncols), C.byref(nn), C.byref(nw))
    return m, int(nn.value), int(nw.value)


def compact_expand(program, narrow, wide):
    """Host-side inverse of Context.columns_compact (numpy): the (num_cols, n) u64 matrix."""
    m, nn, nw = compact_layout(program)
    out = np.empty((len(m), narrow.shape[1]), dtype=np.uint64)
    is_wide = (m & COMPACT_WIDE) != 0
    out[~is_wide] = np.asarray(narrow)[m[~is_wide]]
    out[is_wide] = np.asarray(wide).view(np.uint64)[m[is_wide] & 0x7FFFFFFF]
    return out


def aux_num_cols(program: int = PROGRAM_VERIFY) -> int:
    return int(lib().p2e_aux_num_cols(C.c_int(program)))


def point_msm_plan(n: int, curve: int = CURVE_SECP256K1, window_bits: int = MSM_WINDOW_AUTO) -> dict:
    """What Context.point_msm will use for n points (include/p2e.h p2e_point_msm_plan; host only): window_bits, windows,
    buckets (per window), seg, scratch_bytes, max_lane_additions (a bound on the point operations of one lane in one
    launch that depends on n and the plan alone)."""
    buf = (C.c_uint64 * 6)()
    rc = lib().p2e_point_msm_plan(C.c_int(curve), C.c_size_t(n), C.c_uint(window_bits), buf)
    if rc:
        raise P2EError(f"p2e_point_msm_plan failed ({rc}): {lib().p2e_last_error().decode()}")
    return dict(zip(("window_bits", "windows", "buckets", "seg", "scratch_bytes", "max_lane_additions"), [int(v) for v in buf]))


PBKDF2_MAX_ITERATIONS = 1 << 20    # include/p2e.h P2E_PBKDF2_MAX_ITERATIONS


def pack_bytes(items):
    """A list of bytes or str as (buffer uint8, offsets uint64 (len + 1,)): the variable-length layout of hash_batch and of
    the PBKDF2 / BIP-39 calls.  A str is normalised as BIP-39 asks, unicodedata.normalize("NFKD", s).encode(); bytes are
    taken as given.  The buffer is padded to whole 4-byte words (a lane reads aligned words; no padding byte is used)."""
    import unicodedata
    raw = [unicodedata.normalize("NFKD", s).encode() if isinstance(s, str) else bytes(s) for s in items]
    offsets = np.zeros(len(raw) + 1, dtype=np.uint64)
    if raw:
        offsets[1:] = np.cumsum([len(r) for r in raw], dtype=np.uint64)
    buf = np.zeros((int(offsets[-1]) + 3) // 4 * 4 + 4, dtype=np.uint8)
    buf[:int(offsets[-1])] = np.frombuffer(b"".join(raw), dtype=np.uint8)
    return buf, offsets


def synth_signatures(seed: int, n: int, first: int = 0):
    """Valid secp256k1 signatures (msg, r, s, pk.x, pk.y) as five (n, 32) uint8 arrays (host)."""
    out = [np.zeros((n, 32), dtype=np.uint8) for _ in range(5)]
    rc = lib().p2e_synth_signatures(C.c_uint64(seed), C.c_size_t(first), C.c_size_t(n), *[_ptr(a) for a in out])
    if rc:
        raise P2EError("p2e_synth_signatures failed")
    return out


def synth_signatures_curve(curve: int, seed: int, n: int, first: int = 0):
    """Valid signatures on a curve of the crate (CURVE_*): (msg, r, s, pk.x, pk.y) as five (n, 32) uint8 arrays (host)."""
    out = [np.zeros((n, 32), dtype=np.uint8) for _ in range(5)]
    rc = lib().p2e_synth_signatures_curve(C.c_int(curve), C.c_uint64(seed), C.c_size_t(first), C.c_size_t(n), *[_ptr(a) for a in out])
    if rc:
        raise P2EError("p2e_synth_signatures_curve failed")
    return out


class CurveProgram:
    """One built circuit of curve_scalar_mul_windowed / curve_scalar_mul / verify_p256_message_circuit /
    curve_msm_circuit / fixed_base_curve_mul_circuit (gadgets/curve_windowed_mul.rs:131-173, gadgets/curve.rs:245-285,
    gadgets/ecdsa.rs:55-78, gadgets/curve_msm.rs:21-79, gadgets/curve_fixed_base.rs:18-66) on CURVE_SECP256K1 or
    CURVE_P256.  ``blind`` = the point the gadget draws with rand() while the circuit is built, as (x, y) ints;
    CP_FIXED_BASE_MUL: ``base`` (or ``blind``) = the constant base; CP_MSM takes no point."""

    def __init__(self, ctx, kind: int, curve: int, blind=None, base=None):
        self._ctx, self.kind, self.curve = ctx, kind, curve
        pt = base if base is not None else blind
        bx = by = None
        if pt is not None:
            bx = np.frombuffer(int(pt[0]).to_bytes(32, "little"), np.uint8).copy()
            by = np.frombuffer(int(pt[1]).to_bytes(32, "little"), np.uint8).copy()
        h = C.c_void_p()
        rc = ctx._L.p2e_curve_program_create(ctx._h, C.c_int(kind), C.c_int(curve), _ptr(bx), _ptr(by), C.byref(h))
        if rc != 0:
            raise P2EError(f"p2e_curve_program_create failed ({rc}): {ctx._L.p2e_last_error().decode()}")
        self._h = h
        self.num_cols = int(ctx._L.p2e_curve_program_num_cols(h))
        self.num_aux_cols = int(ctx._L.p2e_curve_program_num_aux_cols(h))
        self.num_gate_cols = int(ctx._L.p2e_curve_program_num_gate_cols(h))
        self.num_ux_cols = int(ctx._L.p2e_curve_program_num_ux_cols(h))

    def close(self):
        if getattr(self, "_h", None) and getattr(self._ctx, "_h", None):
            self._ctx._L.p2e_curve_program_destroy(self._ctx._h, self._h)
        self._h = None

    __del__ = close

    def scratch_bytes(self, n):
        return int(self._ctx._L.p2e_curve_program_scratch_bytes(self._h, C.c_size_t(n)))

    def describe(self):
        """(kind, field, first_col, num_cols, label) per generator, registration order (as schedule_describe)."""
        L = self._ctx._L
        n = L.p2e_curve_program_describe(self._h, None, C.c_size_t(0))
        arr = (_GenDesc * n)()
        L.p2e_curve_program_describe(self._h, arr, C.c_size_t(n))
        kinds = ("add", "sub", "add_many", "mul", "inv", "glv")
        return [(kinds[d.kind], d.field, d.first_col, d.num_cols, d.label.decode()) for d in arr]

    def wiring(self):
        """([(src, num_limbs), ...], range_check) per generator (as schedule_wiring); constants through const()."""
        L = self._ctx._L
        n = L.p2e_curve_program_wiring(self._h, None, C.c_size_t(0))
        arr = (_GenWiring * n)()
        L.p2e_curve_program_wiring(self._h, arr, C.c_size_t(n))
        return [([(int(w.src[k]), int(w.num_limbs[k])) for k in range(w.num_operands)], bool(w.range_check)) for w in arr]

    def aux_describe(self):
        """(kind code, first_col, num_cols, label) of the built-in-generator targets the wiring refers to."""
        L = self._ctx._L
        n = L.p2e_curve_program_aux_describe(self._h, None, C.c_size_t(0))
        arr = (_AuxDesc * n)()
        L.p2e_curve_program_aux_describe(self._h, arr, C.c_size_t(n))
        return [(int(d.kind), d.first_col, d.num_cols, d.label.decode()) for d in arr]

    def const(self, const_id: int) -> int:
        buf = (C.c_uint8 * 32)()
        if self._ctx._L.p2e_curve_program_const(self._h, C.c_uint32(const_id), buf) != 0:
            raise P2EError("unknown constant id")
        return int.from_bytes(bytes(buf), "little")

    def _out(self, n, cols, err, valid, ld):
        ctx = self._ctx
        if cols is None:
            ld = n + 16 if (n >= 4096 and n & (n - 1) == 0) else n
            full = ctx._cols(self.num_cols, ld)
            cols = full[:, :n] if ld != n else full
        err = err if err is not None else ctx._vec(n, np.uint8)
        valid = valid if valid is not None else ctx._vec(n, np.uint8)
        return cols, err, valid, ld if ld is not None else _ld(cols)

    def mul_witness_batch(self, px, py, k, cols=None, err=None, valid=None, ld=None):
        """(num_cols, n) columns of every generator the gadget registers for n (point, scalar) pairs
        (CP_FIXED_BASE_MUL: px = py = None, the base is the program's)."""
        ctx = self._ctx
        n = ctx._shape(k)[0]
        cols, err, valid, ld = self._out(n, cols, err, valid, ld)
        bad = ctx._check(ctx._L.p2e_curve_mul_witness_batch(ctx._h, self._h, _ptr(px), _ptr(py), _ptr(k), _ptr(cols), C.c_size_t(n),
                                                            C.c_size_t(ld), _ptr(err), _ptr(valid)))
        return cols, err, valid, bad

    # ---- the compact container (include/p2e.h p2e_curve_program_compact_layout) -----------------------------------
    def compact_layout(self):
        """(col_map, num_narrow, num_wide): col_map[c] = row of witness column c in the u32 narrow matrix, or
        COMPACT_WIDE | row in the u64 wide one."""
        L = self._ctx._L
        m = np.zeros(self.num_cols, dtype=np.uint32)
        nn, nw = C.c_uint32(), C.c_uint32()
        L.p2e_curve_program_compact_layout(self._h, _ptr(m), C.c_size_t(self.num_cols), C.byref(nn), C.byref(nw))
        return m, int(nn.value), int(nw.value)

    def compact_expand(self, narrow, wide):
        """host-side inverse (numpy): the (num_cols, n) u64 matrix of a compact container of this program"""
        m, _nn, _nw = self.compact_layout()
        out = np.empty((len(m), narrow.shape[1]), dtype=np.uint64)
        is_wide = (m & COMPACT_WIDE) != 0
        out[~is_wide] = np.asarray(narrow).view(np.uint32)[m[~is_wide]]
        out[is_wide] = np.asarray(wide).view(np.uint64)[m[is_wide] & 0x7FFFFFFF]
        return out

    def _compact_out(self, n, narrow, wide, err, valid, ld_narrow, ld_wide):
        ctx = self._ctx
        _m, nn, nw = self.compact_layout()
        if narrow is None or wide is None:
            ldp = n + 16 if (not ctx.host_pointers and n >= 4096 and n & (n - 1) == 0) else n
            if ctx.host_pointers:
                narrow, wide = np.zeros((nn, ldp), dtype=np.uint32), np.zeros((nw, ldp), dtype=np.uint64)
            else:
                import torch
                dev = f"cuda:{ctx.device}"
                narrow = torch.empty((nn, ldp), dtype=torch.int32, device=dev)
                wide = torch.empty((nw, ldp), dtype=torch.int64, device=dev)
            narrow, wide = narrow[:, :n], wide[:, :n]
        err = err if err is not None else ctx._vec(n, np.uint8)
        valid = valid if valid is not None else ctx._vec(n, np.uint8)
        return narrow, wide, err, valid, ld_narrow or _ld(narrow), ld_wide or _ld(wide)

    def mul_witness_compact_batch(self, px, py, k, narrow=None, wide=None, err=None, valid=None, ld_narrow=None, ld_wide=None):
        """mul_witness_batch writing the compact container: (narrow u32, wide u64, err, valid, bad)"""
        ctx = self._ctx
        n = ctx._shape(k)[0]
        narrow, wide, err, valid, ldn, ldw = self._compact_out(n, narrow, wide, err, valid, ld_narrow, ld_wide)
        ctx._L.p2e_curve_mul_witness_compact_batch.restype = C.c_long
        bad = ctx._check(ctx._L.p2e_curve_mul_witness_compact_batch(ctx._h, self._h, _ptr(px), _ptr(py), _ptr(k), _ptr(narrow), C.c_size_t(ldn),
                                                                    _ptr(wide), C.c_size_t(ldw), C.c_size_t(n), _ptr(err), _ptr(valid)))
        return narrow, wide, err, valid, bad

    def msm_witness_batch(self, px, py, qx, qy, n_scalar, m_scalar, cols=None, err=None, valid=None, ld=None):
        """CP_MSM: (num_cols, n) columns of curve_msm_circuit(p, q, n, m) for a batch; points and scalars as (n, 32)
        little-endian byte arrays"""
        ctx = self._ctx
        n = ctx._shape(px)[0]
        cols, err, valid, ld = self._out(n, cols, err, valid, ld)
        bad = ctx._check(ctx._L.p2e_curve_msm_witness_batch(ctx._h, self._h, _ptr(px), _ptr(py), _ptr(qx), _ptr(qy), _ptr(n_scalar),
                                                            _ptr(m_scalar), _ptr(cols), C.c_size_t(n), C.c_size_t(ld), _ptr(err),
                                                            _ptr(valid)))
        return cols, err, valid, bad

    def msm_witness_compact_batch(self, px, py, qx, qy, n_scalar, m_scalar, narrow=None, wide=None, err=None, valid=None,
                                  ld_narrow=None, ld_wide=None):
        """msm_witness_batch writing the compact container: (narrow u32, wide u64, err, valid, bad)"""
        ctx = self._ctx
        n = ctx._shape(px)[0]
        narrow, wide, err, valid, ldn, ldw = self._compact_out(n, narrow, wide, err, valid, ld_narrow, ld_wide)
        bad = ctx._check(ctx._L.p2e_curve_msm_witness_compact_batch(ctx._h, self._h, _ptr(px), _ptr(py), _ptr(qx), _ptr(qy),
                                                                    _ptr(n_scalar), _ptr(m_scalar), _ptr(narrow), C.c_size_t(ldn),
                                                                    _ptr(wide), C.c_size_t(ldw), C.c_size_t(n), _ptr(err), _ptr(valid)))
        return narrow, wide, err, valid, bad

    def verify_witness_compact_batch(self, msg, r, s, pkx, pky, narrow=None, wide=None, err=None, valid=None, ld_narrow=None, ld_wide=None):
        """verify_witness_batch writing the compact container: (narrow u32, wide u64, err, valid, bad)"""
        ctx = self._ctx
        n = ctx._shape(msg)[0]
        narrow, wide, err, valid, ldn, ldw = self._compact_out(n, narrow, wide, err, valid, ld_narrow, ld_wide)
        ctx._L.p2e_p256_verify_witness_compact_batch.restype = C.c_long
        bad = ctx._check(ctx._L.p2e_p256_verify_witness_compact_batch(ctx._h, self._h, _ptr(msg), _ptr(r), _ptr(s), _ptr(pkx), _ptr(pky),
                                                                      _ptr(narrow), C.c_size_t(ldn), _ptr(wide), C.c_size_t(ldw), C.c_size_t(n),
                                                                      _ptr(err), _ptr(valid)))
        return narrow, wide, err, valid, bad

    def _inputs(self, inputs):
        """(msg, r, s, pkx, pky) pointers from the program's input tuple: (px, py, k) (fixed-base: px = py = None),
        (px, py, qx, qy, n, m) for CP_MSM, or (msg, r, s, pkx, pky)"""
        if len(inputs) == 3:
            px, py, k = inputs
            return k, None, None, px, py
        if len(inputs) == 6:
            px, py, _qx, _qy, n, m = inputs
            return n, m, None, px, py
        return tuple(inputs)

    def ux_describe(self):
        """(first_col, num_cols) of every generator's constraint block (order of describe())."""
        L = self._ctx._L
        n = L.p2e_curve_program_ux_describe(self._h, None, C.c_size_t(0))
        arr = (_UxDesc * n)()
        L.p2e_curve_program_ux_describe(self._h, arr, C.c_size_t(n))
        return [(int(d.first_col), int(d.num_cols)) for d in arr]

    def aux_witness_batch(self, inputs, cols, n=None, ld=None, aux=None, err=None):
        """built-in-generator targets of the program's circuit from its finished witness matrix: (num_aux_cols, n)"""
        ctx = self._ctx
        msg, r, s, px, py = self._inputs(inputs)
        n = n if n is not None else ctx._shape(msg)[0]
        ld = ld if ld is not None else _ld(cols)
        aux = aux if aux is not None else ctx._cols(self.num_aux_cols, n)
        err = err if err is not None else ctx._vec(n, np.uint8)
        bad = ctx._check(ctx._L.p2e_curve_program_aux_witness_batch(ctx._h, self._h, _ptr(msg), _ptr(r), _ptr(s), _ptr(px), _ptr(py),
                                                                    _ptr(cols), C.c_size_t(ld), _ptr(aux), C.c_size_t(_ld(aux)),
                                                                    C.c_size_t(n), _ptr(err)))
        return aux, err, bad

    def gate_internal_batch(self, aux, n=None, gate=None):
        """gate-internal values of the built-in gates behind the windows, from the aux matrix: (num_gate_cols, n)"""
        ctx = self._ctx
        n = n if n is not None else aux.shape[1]
        gate = gate if gate is not None else ctx._cols(self.num_gate_cols, n)
        ctx._check(ctx._L.p2e_curve_program_gate_internal_batch(ctx._h, self._h, _ptr(aux), C.c_size_t(_ld(aux)), _ptr(gate),
                                                                C.c_size_t(_ld(gate)), C.c_size_t(n)))
        return gate

    def ux_witness_batch(self, inputs, cols, aux, n=None, ld=None, ux=None, err=None, u32=True):
        """constraint-block (U29 gate) values from the finished witness and aux matrices: (num_ux_cols, n) u32 / u64"""
        ctx = self._ctx
        msg, r, s, px, py = self._inputs(inputs)
        n = n if n is not None else ctx._shape(msg)[0]
        ld = ld if ld is not None else _ld(cols)
        if ux is None:
            if ctx.host_pointers:
                ux = np.zeros((self.num_ux_cols, n), dtype=np.uint32 if u32 else np.uint64)
            else:
                import torch
                ux = torch.empty((self.num_ux_cols, n), dtype=torch.int32 if u32 else torch.int64, device=f"cuda:{ctx.device}")
        err = err if err is not None else ctx._vec(n, np.uint8)
        bad = ctx._check(ctx._L.p2e_curve_program_ux_witness_batch(ctx._h, self._h, _ptr(msg), _ptr(r), _ptr(s), _ptr(px), _ptr(py),
                                                                   _ptr(cols), C.c_size_t(ld), _ptr(aux), C.c_size_t(_ld(aux)), _ptr(ux),
                                                                   C.c_int(1 if u32 else 0), C.c_size_t(_ld(ux)), C.c_size_t(n), _ptr(err)))
        return ux, err, bad

    # ---- the same three passes inside the compact container (include/p2e.h *_compact_batch) -----------------------
    def _ux_out(self, n, ux, u32):
        ctx = self._ctx
        if ux is None:
            return ctx._mat(self.num_ux_cols, n, u32), u32
        return ux, _is_u32(ux)

    def aux_witness_compact_batch(self, inputs, narrow, n=None, ld_narrow=None, aux32=None, err=None):
        """aux_witness_batch reading the narrow u32 matrix of the program's compact fill: (num_aux_cols, n) u32"""
        ctx = self._ctx
        msg, r, s, px, py = self._inputs(inputs)
        n = n if n is not None else ctx._shape(msg)[0]
        ld_narrow = ld_narrow if ld_narrow is not None else _ld(narrow)
        aux32 = aux32 if aux32 is not None else ctx._mat(self.num_aux_cols, n, True)
        err = err if err is not None else ctx._vec(n, np.uint8)
        bad = ctx._check(ctx._L.p2e_curve_program_aux_witness_compact_batch(
            ctx._h, self._h, _ptr(msg), _ptr(r), _ptr(s), _ptr(px), _ptr(py), _ptr(narrow), C.c_size_t(ld_narrow), _ptr(aux32),
            C.c_size_t(_ld(aux32)), C.c_size_t(n), _ptr(err)))
        return aux32, err, bad

    def gate_internal_compact_batch(self, aux32, n=None, gate=None):
        """gate_internal_batch from the u32 aux matrix: (num_gate_cols, n) u64"""
        ctx = self._ctx
        n = n if n is not None else aux32.shape[1]
        gate = gate if gate is not None else ctx._cols(self.num_gate_cols, n)
        ctx._check(ctx._L.p2e_curve_program_gate_internal_compact_batch(ctx._h, self._h, _ptr(aux32), C.c_size_t(_ld(aux32)), _ptr(gate),
                                                                        C.c_size_t(_ld(gate)), C.c_size_t(n)))
        return gate

    def ux_witness_compact_batch(self, inputs, narrow, aux32, n=None, ld_narrow=None, ux=None, err=None, u32=True):
        """ux_witness_batch from the narrow u32 matrix and the u32 aux matrix; every program kind (the MSM program's
        6-tuple carries q): (num_ux_cols, n) u32 / u64"""
        ctx = self._ctx
        msg, r, s, px, py = self._inputs(inputs)
        qx, qy = (inputs[2], inputs[3]) if len(inputs) == 6 else (None, None)
        n = n if n is not None else ctx._shape(msg)[0]
        ld_narrow = ld_narrow if ld_narrow is not None else _ld(narrow)
        ux, u32 = self._ux_out(n, ux, u32)
        err = err if err is not None else ctx._vec(n, np.uint8)
        bad = ctx._check(ctx._L.p2e_curve_program_ux_witness_compact_batch(
            ctx._h, self._h, _ptr(msg), _ptr(r), _ptr(s), _ptr(px), _ptr(py), _ptr(qx), _ptr(qy), _ptr(narrow), C.c_size_t(ld_narrow),
            _ptr(aux32), C.c_size_t(_ld(aux32)), _ptr(ux), C.c_int(1 if u32 else 0), C.c_size_t(_ld(ux)), C.c_size_t(n), _ptr(err)))
        return ux, err, bad

    def msm_ux_witness_batch(self, inputs, cols, aux, n=None, ld=None, ux=None, err=None, u32=True):
        """CP_MSM: the constraint-block pass on the u64 matrices; inputs = (px, py, qx, qy, n, m)"""
        ctx = self._ctx
        px, py, qx, qy, ns, ms = inputs
        n = n if n is not None else ctx._shape(px)[0]
        ld = ld if ld is not None else _ld(cols)
        ux, u32 = self._ux_out(n, ux, u32)
        err = err if err is not None else ctx._vec(n, np.uint8)
        bad = ctx._check(ctx._L.p2e_curve_msm_ux_witness_batch(
            ctx._h, self._h, _ptr(px), _ptr(py), _ptr(qx), _ptr(qy), _ptr(ns), _ptr(ms), _ptr(cols), C.c_size_t(ld), _ptr(aux),
            C.c_size_t(_ld(aux)), _ptr(ux), C.c_int(1 if u32 else 0), C.c_size_t(_ld(ux)), C.c_size_t(n), _ptr(err)))
        return ux, err, bad

    def verify_batch(self, msg, r, s, pkx, pky, err=None, valid=None):
        """the verifier circuit's verdict alone (no witness): (err, valid, flagged count)"""
        ctx = self._ctx
        n = ctx._shape(msg)[0]
        err = err if err is not None else ctx._vec(n, np.uint8)
        valid = valid if valid is not None else ctx._vec(n, np.uint8)
        bad = ctx._check(ctx._L.p2e_p256_verify_batch(ctx._h, self._h, _ptr(msg), _ptr(r), _ptr(s), _ptr(pkx), _ptr(pky), C.c_size_t(n),
                                                      _ptr(err), _ptr(valid)))
        return err, valid, bad

    def wire_map(self, src, dst, num_wires, degree):
        """a column -> (wire, row) map over THIS program's four matrices, for Context.assemble_wires"""
        ctx = self._ctx
        src, dst = np.ascontiguousarray(src, np.uint32), np.ascontiguousarray(dst, np.uint32)
        ent = np.empty((len(src), 2), dtype=np.uint32)
        ent[:, 0], ent[:, 1] = src, dst
        h = C.c_void_p()
        rc = ctx._L.p2e_curve_program_wire_map_create(ctx._h, self._h, _ptr(ent), C.c_size_t(len(src)), C.c_uint32(num_wires),
                                                      C.c_uint32(degree), C.byref(h))
        if rc != 0:
            raise P2EError(f"p2e_curve_program_wire_map_create failed ({rc}): {ctx._L.p2e_last_error().decode()}")
        return _WireMap(ctx, h, -1, num_wires, degree, len(src))

    def verify_witness_batch(self, msg, r, s, pkx, pky, cols=None, err=None, valid=None, ld=None):
        """verify_p256_message_circuit: (115557, n) columns."""
        ctx = self._ctx
        n = ctx._shape(msg)[0]
        cols, err, valid, ld = self._out(n, cols, err, valid, ld)
        bad = ctx._check(ctx._L.p2e_p256_verify_witness_batch(ctx._h, self._h, _ptr(msg), _ptr(r), _ptr(s), _ptr(pkx), _ptr(pky),
                                                              _ptr(cols), C.c_size_t(n), C.c_size_t(ld), _ptr(err), _ptr(valid)))
        return cols, err, valid, bad


class _WireMap:
    def __init__(self, ctx, h, program, num_wires, degree, count):
        self._ctx, self._h, self.program, self.num_wires, self.degree, self.count = ctx, h, program, num_wires, degree, count

    def close(self):
        if self._h and getattr(self._ctx, "_h", None):
            self._ctx._L.p2e_wire_map_destroy(self._ctx._h, self._h)
        self._h = None

    __del__ = close


class PointTable:
    """The window tables of m caller points on one curve (include/p2e.h p2e_point_table_create): built once on the device,
    then walked by Context.point_table_mul_batch, point_table_lincomb_batch and ecdsa_verify_table_batch without doublings.
    px, py: (m, 32) little-endian, numpy on a host-pointer context, torch tensors otherwise.  A rejected point ((0, 0), a
    coordinate >= p, off the curve) builds nothing and raises P2EError; its `codes` attribute holds the WIRE_* code of every
    point and `rejected` their count.  The table lives until close() (or the context's end) and keeps its context alive."""

    def __init__(self, ctx, px, py, curve=CURVE_SECP256K1, point_err=None):
        self._ctx, self._h, self.curve = ctx, None, curve
        m = ctx._shape(px)[0]
        point_err = point_err if point_err is not None else ctx._vec(max(m, 1), np.uint8)[:m]
        h = C.c_void_p()
        rc = ctx._L.p2e_point_table_create(ctx._h, C.c_int(curve), _ptr(px), _ptr(py), C.c_size_t(m), _ptr(point_err), C.byref(h))
        if rc != 0:
            e = P2EError(f"p2e_point_table_create failed ({rc}): " +
                         (ctx._L.p2e_last_error().decode() if rc < 0 else f"{rc} of {m} points rejected"))
            e.rejected, e.codes = (int(rc), point_err) if rc > 0 else (0, None)
            raise e
        self._h = h
        self.point_err = point_err

    def __len__(self):
        return int(self._ctx._L.p2e_point_table_num_points(self._h)) if self._h else 0

    def read_window(self, j, w):
        """(16, 2, 32) uint8: entries d = 0 .. 15 of window w of point j, x then y, little-endian (entry 0 copies entry 1)"""
        out = np.zeros((16, 2, 32), np.uint8)
        self._ctx._check(self._ctx._L.p2e_point_table_read_window(self._ctx._h, self._h, C.c_size_t(j), C.c_int(w),
                                                                  out.ctypes.data_as(C.c_void_p)))
        return out

    def close(self):
        if self._h and getattr(self._ctx, "_h", None):
            self._ctx._L.p2e_point_table_destroy(self._ctx._h, self._h)
        self._h = None

    __del__ = close


class Context:
    """One p2e_ctx: one per (host thread, device).

    ``host_pointers=True`` makes every entry point take numpy arrays (staged through the library's own
    device buffers: convenient for tests, PCIe-inclusive, never benchmarked).  Otherwise arguments are
    torch CUDA tensors and the context runs on ``stream`` (default: torch's current stream).
    ``phase_timing=True`` (P2E_CTX_PHASE_TIMING) times every launch for last_phase_ms(); off by default, it costs 6 % at 2^13
    signatures per call."""

    def __init__(self, device: int = 0, host_pointers: bool = False, stream=None, asynchronous: bool = False,
                 phase_timing: bool = False):
        L = lib()
        self._L = L
        self.host_pointers = host_pointers
        flags = ((CTX_HOST_POINTERS if host_pointers else 0) | (CTX_ASYNC if asynchronous else 0)
                 | (CTX_PHASE_TIMING if phase_timing else 0))
        if stream is None and not host_pointers:
            import torch
            stream = torch.cuda.current_stream(device).cuda_stream
        h = C.c_void_p()
        rc = L.p2e_ctx_create(C.c_int(device), C.c_uint(flags), C.c_void_p(stream or 0), C.byref(h))
        if rc != 0:
            raise P2EError(f"p2e_ctx_create failed ({rc}): {L.p2e_last_error().decode()}")
        self._h = h
        self.device = device

    def close(self):
        if getattr(self, "_h", None):
            self._L.p2e_ctx_destroy(self._h)
            self._h = None

    __del__ = close

    def _check(self, rc):
        if rc < 0:
            raise P2EError(f"p2e call failed ({rc}): {self._L.p2e_last_error().decode()}")
        return int(rc)

    def sync(self):
        return self._check(self._L.p2e_sync(self._h))

    def last_phase_ms(self):
        """include/p2e.h p2e_last_phase_ms: `expand*` = k_expand launches, `runs*` = k_expand_runs launches, `fbrun*` =
        k_expand_fb_run launches (per kind: launches, columns written per signature, summed HIP-event durations in ms).
        Durations are 0 unless the context was created with phase_timing=True (launches and columns are always there)."""
        buf = (C.c_float * 12)()
        self._L.p2e_last_phase_ms(self._h, buf, C.c_int(12))
        return dict(zip(("scalar", "expand_launches", "expand_cols", "expand", "total", "runs_launches", "runs_cols",
                         "runs", "fbrun_launches", "fbrun_cols", "fbrun"), [float(x) for x in buf]))

    # ---- column blocks of the last fused call, as they become final (include/p2e.h p2e_segments_describe) -------------
    def segments(self):
        """[(first_col, num_cols)] of the last fused call issued on this context, in issue order: the scalar phase's
        blocks, then the blocks of every expansion launch (one per contiguous run of columns; they share the launch's
        event).  Disjoint; together every column of the program."""
        self._L.p2e_segments_describe.restype = C.c_long
        k = self._L.p2e_segments_describe(self._h, None, C.c_size_t(0))
        buf = (C.c_uint32 * (2 * max(k, 1)))()
        self._L.p2e_segments_describe(self._h, buf, C.c_size_t(k))
        return [(int(buf[2 * i]), int(buf[2 * i + 1])) for i in range(k)]

    def segment_stream_wait(self, k: int, stream: int):
        """`stream` (a raw hipStream_t handle, e.g. torch.cuda.Stream().cuda_stream) waits until block k is final."""
        if self._L.p2e_segment_stream_wait(self._h, C.c_int(k), C.c_void_p(stream)) != 0:
            raise P2EError(self._L.p2e_last_error().decode())

    def segment_sync(self, k: int):
        """the host blocks until block k is final"""
        if self._L.p2e_segment_sync(self._h, C.c_int(k)) != 0:
            raise P2EError(self._L.p2e_last_error().decode())

    # ---- allocation helpers -------------------------------------------------------------------------
    def _cols(self, k, n):
        if self.host_pointers:
            return np.zeros((k, n), dtype=np.uint64)
        import torch
        return torch.empty((k, n), dtype=torch.int64, device=f"cuda:{self.device}")

    def _mat(self, k, n, u32):
        """(k, n) u32 or u64 matrix"""
        if self.host_pointers:
            return np.zeros((k, n), dtype=np.uint32 if u32 else np.uint64)
        import torch
        return torch.empty((k, n), dtype=torch.int32 if u32 else torch.int64, device=f"cuda:{self.device}")

    def _vec(self, n, dtype=np.uint64):
        if self.host_pointers:
            return np.zeros(n, dtype=dtype)
        import torch
        td = {np.uint64: torch.int64, np.uint8: torch.uint8}[dtype]
        return torch.empty(n, dtype=td, device=f"cuda:{self.device}")

    @staticmethod
    def _shape(a):
        return tuple(a.shape)

    # ---- single generators ---------------------------------------------------------------------------
    def mul_witness_batch(self, field, x, y):
        """MulNonnativeGenerator + CheckSumGenerator (gates/mul_nonnative.rs:249-324, :513-531)."""
        n = self._shape(x)[1]
        _dense(n, x, y)
        r, q, cs, b, err = self._cols(9, n), self._cols(9, n), self._cols(17, n), self._cols(16, n), self._vec(n, np.uint8)
        bad = self._check(self._L.p2e_mul_witness_batch(self._h, C.c_int(field), _ptr(x), _ptr(y), _ptr(r), _ptr(q),
                                                        _ptr(cs), _ptr(b), C.c_size_t(n), C.c_size_t(n), _ptr(err)))
        return r, q, cs, b, err, bad

    def checksum_witness_batch(self, a):
        n = self._shape(a)[1]
        _dense(n, a)
        b, err = self._cols(16, n), self._vec(n, np.uint8)
        bad = self._check(self._L.p2e_checksum_witness_batch(self._h, _ptr(a), _ptr(b), C.c_size_t(n), C.c_size_t(n), _ptr(err)))
        return b, err, bad

    def _binop(self, fn, field, a, b):
        n = self._shape(a)[1]
        _dense(n, a, b)
        out, ov, err = self._cols(9, n), self._vec(n), self._vec(n, np.uint8)
        bad = self._check(fn(self._h, C.c_int(field), _ptr(a), _ptr(b), _ptr(out), _ptr(ov), C.c_size_t(n),
                             C.c_size_t(n), _ptr(err)))
        return out, ov, err, bad

    def add_witness_batch(self, field, a, b):
        """NonNativeAdditionGenerator (gadgets/nonnative.rs:626-645)."""
        return self._binop(self._L.p2e_add_witness_batch, field, a, b)

    def sub_witness_batch(self, field, a, b):
        """NonNativeSubtractionGenerator (gadgets/nonnative.rs:792-810)."""
        return self._binop(self._L.p2e_sub_witness_batch, field, a, b)

    def add_many_witness_batch(self, field, summands):
        """NonNativeMultipleAddsGenerator (gadgets/nonnative.rs:696-728); summands (k, 9, n)."""
        k, _, n = self._shape(summands)
        _dense(n, summands)
        out, ov, err = self._cols(9, n), self._vec(n), self._vec(n, np.uint8)
        bad = self._check(self._L.p2e_add_many_witness_batch(self._h, C.c_int(field), _ptr(summands), C.c_int(k),
                                                             _ptr(out), _ptr(ov), C.c_size_t(n), C.c_size_t(n), _ptr(err)))
        return out, ov, err, bad

    def inv_witness_batch(self, field, x):
        """NonNativeInverseGenerator (gadgets/nonnative.rs:857-872)."""
        n = self._shape(x)[1]
        _dense(n, x)
        inv, div, err = self._cols(9, n), self._cols(9, n), self._vec(n, np.uint8)
        bad = self._check(self._L.p2e_inv_witness_batch(self._h, C.c_int(field), _ptr(x), _ptr(inv), _ptr(div),
                                                        C.c_size_t(n), C.c_size_t(n), _ptr(err)))
        return inv, div, err, bad

    def biguint_div_rem_batch(self, a, b):
        """BigUintDivRemGenerator (gadgets/biguint.rs:508-518): a (na, n), b (nb, n) limb columns ->
        (div (max(0, na - nb + 1), n), rem (nb, n), err, flagged)."""
        na, n = self._shape(a)
        nb = self._shape(b)[0]
        _dense(n, a, b)
        nd = 0 if nb > na + 1 else na - nb + 1
        div, rem, err = self._cols(max(nd, 1), n), self._cols(nb, n), self._vec(n, np.uint8)
        bad = self._check(self._L.p2e_biguint_div_rem_batch(self._h, _ptr(a), C.c_int(na), _ptr(b), C.c_int(nb), _ptr(div),
                                                            _ptr(rem), C.c_size_t(n), C.c_size_t(n), _ptr(err)))
        return div[:nd], rem, err, bad

    def glv_decompose_batch(self, k):
        """GLVDecompositionGenerator (gadgets/glv.rs:128-142)."""
        n = self._shape(k)[1]
        _dense(n, k)
        k1, k2, n1, n2, err = self._cols(5, n), self._cols(5, n), self._vec(n), self._vec(n), self._vec(n, np.uint8)
        bad = self._check(self._L.p2e_glv_decompose_batch(self._h, _ptr(k), _ptr(k1), _ptr(k2), _ptr(n1), _ptr(n2),
                                                          C.c_size_t(n), C.c_size_t(n), _ptr(err)))
        return k1, k2, n1, n2, err, bad

    def limb_split(self, packed, out=None):
        """set_biguint_target (gadgets/biguint.rs:454-463): (n, 32) uint8 -> (9, n) limb columns."""
        n = self._shape(packed)[0]
        limbs = out if out is not None else self._cols(9, n)
        self._check(self._L.p2e_limb_split(self._h, _ptr(packed), _ptr(limbs), C.c_size_t(n), C.c_size_t(_ld(limbs))))
        return limbs

    def limb_pack(self, limbs):
        """get_biguint_target (gadgets/biguint.rs:444-452): (9, n) limb columns -> (n, 32) uint8."""
        n = self._shape(limbs)[1]
        ld = _ld(limbs)
        if self.host_pointers:
            packed = np.zeros((n, 32), dtype=np.uint8)
        else:
            import torch
            packed = torch.empty((n, 32), dtype=torch.uint8, device=f"cuda:{self.device}")
        err = self._vec(n, np.uint8)
        bad = self._check(self._L.p2e_limb_pack(self._h, _ptr(limbs), _ptr(packed), C.c_size_t(n), C.c_size_t(ld), _ptr(err)))
        return packed, err, bad

    def columns_to_rows(self, cols, n=None, ld=None, rows=None):
        """(ncols, ld) column-major matrix -> (n, ncols) matrix with one contiguous witness per signature."""
        ncols = self._shape(cols)[0]
        ld = ld if ld is not None else _ld(cols)
        n = n if n is not None else self._shape(cols)[1]
        if rows is None:
            if self.host_pointers:
                rows = np.zeros((n, ncols), dtype=np.uint64)
            else:
                import torch
                rows = torch.empty((n, ncols), dtype=torch.int64, device=f"cuda:{self.device}")
        self._check(self._L.p2e_columns_to_rows(self._h, _ptr(cols), C.c_size_t(ld), C.c_size_t(n), C.c_size_t(ncols),
                                                _ptr(rows), C.c_size_t(_ld(rows))))
        return rows

    def compact_to_rows(self, program, narrow, wide, n, ld_narrow=None, ld_wide=None, rows_narrow=None, rows_wide=None):
        """columns_to_rows for the compact container: ((n, num_narrow) u32, (n, num_wide) u64), one contiguous witness per signature."""
        _m, nn, nw = compact_layout(program)
        if rows_narrow is None or rows_wide is None:
            if self.host_pointers:
                rows_narrow, rows_wide = np.zeros((n, nn), dtype=np.uint32), np.zeros((n, nw), dtype=np.uint64)
            else:
                import torch
                dev = f"cuda:{self.device}"
                rows_narrow = torch.empty((n, nn), dtype=torch.int32, device=dev)
                rows_wide = torch.empty((n, nw), dtype=torch.int64, device=dev)
        self._check(self._L.p2e_compact_to_rows(self._h, C.c_int(program), _ptr(narrow), C.c_size_t(ld_narrow or _ld(narrow)),
                                                _ptr(wide), C.c_size_t(ld_wide or _ld(wide)), C.c_size_t(n),
                                                _ptr(rows_narrow), C.c_size_t(_ld(rows_narrow)), _ptr(rows_wide),
                                                C.c_size_t(_ld(rows_wide))))
        return rows_narrow, rows_wide

    # ---- fused schedules -----------------------------------------------------------------------------
    def ecdsa_verify_witness_batch(self, msg, r, s, pkx, pky, cols=None, err=None, valid=None, ld=None):
        """verify_secp256k1_message_circuit (gadgets/ecdsa.rs:30-53): (82615, n) Goldilocks columns.
        ``cols`` may be a column slice of a wider matrix: pass its row stride as ``ld``."""
        n = self._shape(msg)[0]
        if cols is None:
            # a power-of-two column stride makes consecutive columns camp on the same HBM channels (-9 %)
            ld = n + 16 if (n >= 4096 and n & (n - 1) == 0) else n
            full = self._cols(VERIFY_COLS, ld)
            cols = full[:, :n] if ld != n else full
        err = err if err is not None else self._vec(n, np.uint8)
        valid = valid if valid is not None else self._vec(n, np.uint8)
        ld = ld if ld is not None else _ld(cols)
        bad = self._check(self._L.p2e_ecdsa_verify_witness_batch(self._h, _ptr(msg), _ptr(r), _ptr(s), _ptr(pkx), _ptr(pky),
                                                                 _ptr(cols), C.c_size_t(n), C.c_size_t(ld), _ptr(err), _ptr(valid)))
        return cols, err, valid, bad

    def aux_witness_batch(self, program, pky, cols, n=None, ld=None, aux=None, err=None, ld_aux=None):
        """Built-in-generator columns (bool selects, window bits / digits, random-access selections, is_equal / not
        results: SURVEY.md 8(f) rank 1) derived from a finished witness matrix: (8959 | 4738, n) columns."""
        n = n if n is not None else self._shape(pky)[0]
        ld = ld if ld is not None else _ld(cols)
        if aux is None:
            aux = self._cols(VERIFY_AUX_COLS if program == PROGRAM_VERIFY else GLV_MUL_AUX_COLS, n)
        ld_aux = ld_aux if ld_aux is not None else _ld(aux)
        err = err if err is not None else self._vec(n, np.uint8)
        bad = self._check(self._L.p2e_aux_witness_batch(self._h, C.c_int(program), _ptr(pky), _ptr(cols), C.c_size_t(ld),
                                                        _ptr(aux), C.c_size_t(ld_aux), C.c_size_t(n), _ptr(err)))
        return aux, err, bad

    def ux_witness_batch(self, program, inputs, cols, aux, n=None, ld=None, ld_aux=None, ux=None, ld_ux=None, err=None, u32=True):
        """Constraint-block columns (what the U29 gates inside add / sub / add_many / inv / the
        range checks hand back, in builder-call order) from the finished witness and aux matrices.
        inputs: (msg, r, s, pk.x, pk.y) for the verify program, (pk.x, pk.y, k) for glv_mul.  (249385 | 194361, n)."""
        if program == PROGRAM_VERIFY:
            msg, r, s, pkx, pky = inputs
        else:
            pkx, pky, msg = inputs
            r = s = None
        n = n if n is not None else self._shape(pky)[0]
        ld = ld if ld is not None else _ld(cols)
        ld_aux = ld_aux if ld_aux is not None else _ld(aux)
        k = VERIFY_UX_COLS if program == PROGRAM_VERIFY else GLV_MUL_UX_COLS
        if ux is None:
            if self.host_pointers:
                ux = np.zeros((k, n), dtype=np.uint32 if u32 else np.uint64)
            else:
                import torch
                ux = torch.empty((k, n), dtype=torch.int32 if u32 else torch.int64, device=f"cuda:{self.device}")
        else:
            u32 = (ux.dtype == np.uint32) if isinstance(ux, np.ndarray) else (ux.element_size() == 4)
        ld_ux = ld_ux if ld_ux is not None else _ld(ux)
        err = err if err is not None else self._vec(n, np.uint8)
        self._L.p2e_ux_witness_batch.restype = C.c_long
        bad = self._check(self._L.p2e_ux_witness_batch(self._h, C.c_int(program), _ptr(msg), _ptr(r), _ptr(s), _ptr(pkx), _ptr(pky),
                                                       _ptr(cols), C.c_size_t(ld), _ptr(aux), C.c_size_t(ld_aux), _ptr(ux),
                                                       C.c_int(1 if u32 else 0), C.c_size_t(ld_ux), C.c_size_t(n), _ptr(err)))
        return ux, err, bad

    # ---- wire-matrix assembly --------------------------------------------------
    def wire_map(self, program, src, dst, num_wires, degree):
        """Upload a column -> (wire, row) map (include/p2e.h p2e_wire_map_create); returns an opaque handle for
        assemble_wires.  src / dst: uint32 arrays (plonky2_ecdsa_amd.wiremap has a synthetic generator)."""
        src, dst = np.ascontiguousarray(src, np.uint32), np.ascontiguousarray(dst, np.uint32)
        ent = np.empty((len(src), 2), dtype=np.uint32)
        ent[:, 0], ent[:, 1] = src, dst
        h = C.c_void_p()
        rc = self._L.p2e_wire_map_create(self._h, C.c_int(program), _ptr(ent), C.c_size_t(len(src)), C.c_uint32(num_wires),
                                         C.c_uint32(degree), C.byref(h))
        if rc != 0:
            raise P2EError(f"p2e_wire_map_create failed ({rc}): {self._L.p2e_last_error().decode()}")
        return _WireMap(self, h, program, num_wires, degree, len(src))

    def gate_internal_batch(self, program, aux, n=None, ld_aux=None, gate=None, ld_gate=None):
        """Gate-internal values of the built-in gates (equality gadget internals, RandomAccessGate index bits) from the
        aux matrix: (10703 | 5621, n) uint64."""
        n = n if n is not None else self._shape(aux)[1]
        ld_aux = ld_aux if ld_aux is not None else _ld(aux)
        if gate is None:
            gate = self._cols(VERIFY_GATE_COLS if program == PROGRAM_VERIFY else GLV_MUL_GATE_COLS, n)
        ld_gate = ld_gate if ld_gate is not None else _ld(gate)
        self._L.p2e_gate_internal_batch.restype = C.c_long
        self._check(self._L.p2e_gate_internal_batch(self._h, C.c_int(program), _ptr(aux), C.c_size_t(ld_aux), _ptr(gate),
                                                    C.c_size_t(ld_gate), C.c_size_t(n)))
        return gate

    def assemble_wires(self, wmap, cols=None, aux=None, ux=None, gate=None, wires=None, n=None):
        """wires[i, wire * degree + row] = the mapped value of signature i: (n, num_wires * degree) int64, one plonky2 wire
        matrix per signature (zero where the map names nothing, when allocated here)."""
        ref = next(m for m in (cols, aux, ux, gate) if m is not None)
        n = n if n is not None else self._shape(ref)[1]
        cells = wmap.num_wires * wmap.degree
        if wires is None:
            if self.host_pointers:
                wires = np.zeros((n, cells), dtype=np.uint64)
            else:
                import torch
                wires = torch.zeros((n, cells), dtype=torch.int64, device=f"cuda:{self.device}")
        u32 = 0
        if ux is not None:
            u32 = int((ux.dtype == np.uint32) if isinstance(ux, np.ndarray) else (ux.element_size() == 4))
        self._L.p2e_assemble_wires.restype = C.c_long
        self._check(self._L.p2e_assemble_wires(self._h, wmap._h, _ptr(cols), C.c_size_t(_ld(cols) if cols is not None else 0),
                                               _ptr(aux), C.c_size_t(_ld(aux) if aux is not None else 0), _ptr(ux), C.c_int(u32),
                                               C.c_size_t(_ld(ux) if ux is not None else 0), _ptr(gate),
                                               C.c_size_t(_ld(gate) if gate is not None else 0), _ptr(wires),
                                               C.c_size_t(_ld(wires)), C.c_size_t(n)))
        return wires

    def columns_compact(self, program, cols, n=None, ld=None, narrow=None, wide=None, err=None, ld_narrow=None, ld_wide=None):
        """Repack a finished witness matrix for transfers: (narrow u32 (num_narrow, n), wide u64 (num_wide, n), err, bad).
        Preallocated `narrow` / `wide` may be column slices of wider matrices: pass their row strides."""
        _m, nn, nw = compact_layout(program)
        ld = ld if ld is not None else _ld(cols)
        n = n if n is not None else self._shape(cols)[1]
        if narrow is None or wide is None:
            if self.host_pointers:
                narrow, wide = np.zeros((nn, n), dtype=np.uint32), np.zeros((nw, n), dtype=np.uint64)
            else:
                import torch
                dev = f"cuda:{self.device}"
                narrow = torch.empty((nn, n), dtype=torch.int32, device=dev)
                wide = torch.empty((nw, n), dtype=torch.int64, device=dev)
        err = err if err is not None else self._vec(n, np.uint8)
        bad = self._check(self._L.p2e_columns_compact(self._h, C.c_int(program), _ptr(cols), C.c_size_t(ld), C.c_size_t(n),
                                                      _ptr(narrow), C.c_size_t(ld_narrow or _ld(narrow)), _ptr(wide),
                                                      C.c_size_t(ld_wide or _ld(wide)), _ptr(err)))
        return narrow, wide, err, bad

    def ecdsa_verify_batch(self, msg, r, s, pkx, pky, err=None, valid=None):
        """The verdict alone (pre-filter, no witness): (err, valid, flagged count), as ecdsa_verify_witness_batch sets them."""
        n = self._shape(msg)[0]
        err = err if err is not None else self._vec(n, np.uint8)
        valid = valid if valid is not None else self._vec(n, np.uint8)
        bad = self._check(self._L.p2e_ecdsa_verify_batch(self._h, _ptr(msg), _ptr(r), _ptr(s), _ptr(pkx), _ptr(pky),
                                                         C.c_size_t(n), _ptr(err), _ptr(valid)))
        return err, valid, bad

    # ---- key derivation and signing (include/p2e.h p2e_ecdsa_public_key_batch / p2e_ecdsa_sign_batch) ----------------
    def _packed(self, n):
        if self.host_pointers:
            return np.zeros((n, 32), dtype=np.uint8)
        import torch
        return torch.empty((n, 32), dtype=torch.uint8, device=f"cuda:{self.device}")

    def ecdsa_public_key_batch(self, sk, curve=CURVE_SECP256K1, plan=SIGN_PLAN_AUTO, pkx=None, pky=None, err=None):
        """ECDSASecretKey::to_public (curve/ecdsa.rs:16-20) of (n, 32) little-endian secret keys, each taken modulo the group
        order: (pkx, pky, err, flagged count).  sk = 0 (mod n): zeros and ERR_POINT_AT_INFINITY."""
        n = self._shape(sk)[0]
        pkx = pkx if pkx is not None else self._packed(n)
        pky = pky if pky is not None else self._packed(n)
        err = err if err is not None else self._vec(n, np.uint8)
        bad = self._check(self._L.p2e_ecdsa_public_key_batch(self._h, C.c_int(curve), C.c_uint(plan), _ptr(sk), _ptr(pkx), _ptr(pky),
                                                             C.c_size_t(n), _ptr(err)))
        return pkx, pky, err, bad

    def ecdsa_sign_batch(self, msg, sk, k, curve=CURVE_SECP256K1, plan=SIGN_PLAN_AUTO, r=None, s=None, err=None):
        """sign_message (curve/ecdsa.rs:25-40) with the nonces k as an input; msg, sk, k are (n, 32) little-endian, each taken
        modulo the group order: (r, s, err, flagged count).  k = 0 (mod n): zeros and ERR_INVERSE_OF_ZERO; r = 0 or s = 0 are
        returned unflagged (they do not verify)."""
        n = self._shape(msg)[0]
        r = r if r is not None else self._packed(n)
        s = s if s is not None else self._packed(n)
        err = err if err is not None else self._vec(n, np.uint8)
        bad = self._check(self._L.p2e_ecdsa_sign_batch(self._h, C.c_int(curve), C.c_uint(plan), _ptr(msg), _ptr(sk), _ptr(k), _ptr(r),
                                                       _ptr(s), C.c_size_t(n), _ptr(err)))
        return r, s, err, bad

    def ecdsa_sign_recoverable_batch(self, msg, sk, k, curve=CURVE_SECP256K1, plan=SIGN_PLAN_AUTO, r=None, s=None, v=None, err=None):
        """ecdsa_sign_batch plus the recovery byte v (n,): bit 0 = parity of R.y, bit 1 = R.x >= n; 0 where flagged:
        (r, s, v, err, flagged count).  r, s, err are bit for bit those of ecdsa_sign_batch."""
        n = self._shape(msg)[0]
        r = r if r is not None else self._packed(n)
        s = s if s is not None else self._packed(n)
        v = v if v is not None else self._vec(n, np.uint8)
        err = err if err is not None else self._vec(n, np.uint8)
        bad = self._check(self._L.p2e_ecdsa_sign_recoverable_batch(self._h, C.c_int(curve), C.c_uint(plan), _ptr(msg), _ptr(sk), _ptr(k),
                                                                   _ptr(r), _ptr(s), _ptr(v), C.c_size_t(n), _ptr(err)))
        return r, s, v, err, bad

    def ecdsa_recover_batch(self, msg, r, s, v, curve=CURVE_SECP256K1, pkx=None, pky=None, err=None):
        """The public key of every (msg, r, s, v): pk = r^-1 (s R - msg G), R the point with x = r + n (v >> 1) and
        y = v & 1 (mod 2); v (n,) uint8 carries no offset (subtract Ethereum's 27 / the EIP-155 term first).
        (pkx, pky, err, flagged count); zeros and ERR_NOT_RECOVERABLE / ERR_POINT_AT_INFINITY where there is no key."""
        n = self._shape(msg)[0]
        pkx = pkx if pkx is not None else self._packed(n)
        pky = pky if pky is not None else self._packed(n)
        err = err if err is not None else self._vec(n, np.uint8)
        bad = self._check(self._L.p2e_ecdsa_recover_batch(self._h, C.c_int(curve), _ptr(msg), _ptr(r), _ptr(s), _ptr(v), _ptr(pkx),
                                                          _ptr(pky), C.c_size_t(n), _ptr(err)))
        return pkx, pky, err, bad

    # ---- the many-point sum (include/p2e.h p2e_point_msm) ---------------------------------------------------------------
    def point_msm(self, k, px, py, curve=CURVE_SECP256K1, window_bits=MSM_WINDOW_AUTO, outx=None, outy=None, status=None,
                  point_err=None, want_point_err=True, n=None):
        """sum_i k[i] * (px[i], py[i]) by the bucket method; k, px, py are (n, 32) little-endian, k taken modulo the group
        order, (0, 0) the neutral element.  (outx (32,), outy (32,), status (1,), point_err (n,) or None, rejected count):
        status MSM_OK and the canonical affine sum; MSM_NEUTRAL and zeros; MSM_BAD_POINT, zeros and point_err[i] = 1 where
        a point is not on the curve (nothing is summed without them).  want_point_err=False passes no point_err; n: the
        number of points where it is not k's first dimension (n = 0 still needs buffers that are not empty)."""
        n = self._shape(k)[0] if n is None else n
        outx = outx if outx is not None else self._packed(1)[0]
        outy = outy if outy is not None else self._packed(1)[0]
        status = status if status is not None else self._vec(1, np.uint8)
        if point_err is None and want_point_err:
            point_err = self._vec(max(n, 1), np.uint8)[:n]
        bad = self._check(self._L.p2e_point_msm(self._h, C.c_int(curve), C.c_uint(window_bits), _ptr(k), _ptr(px), _ptr(py),
                                                C.c_size_t(n), _ptr(outx), _ptr(outy), _ptr(status), _ptr(point_err)))
        return outx, outy, status, point_err, bad

    # ---- per-element point arithmetic (include/p2e.h p2e_point_mul_batch and the two after it) ----------------------------------
    def point_mul_batch(self, k, px, py, curve=CURVE_SECP256K1, plan=MUL_PLAN_AUTO, outx=None, outy=None, err=None):
        """k[i] * (px[i], py[i]) per element; k, px, py are (n, 32) little-endian, k taken modulo the group order, (0, 0) the
        neutral element: (outx, outy, err, flagged count).  err holds WIRE_* codes: WIRE_COORD_RANGE / WIRE_NOT_ON_CURVE for
        an invalid point, WIRE_INFINITY where the product is the neutral element (k = 0 mod n, P neutral); zeros are written
        where it is not 0.  plan: MUL_PLAN_AUTO, MUL_PLAN_PLAIN, MUL_PLAN_GLV (secp256k1 only); the bytes do not depend on it."""
        n = self._shape(k)[0]
        outx = outx if outx is not None else self._packed(n)
        outy = outy if outy is not None else self._packed(n)
        err = err if err is not None else self._vec(n, np.uint8)
        bad = self._check(self._L.p2e_point_mul_batch(self._h, C.c_int(curve), C.c_uint(plan), _ptr(k), _ptr(px), _ptr(py), _ptr(outx),
                                                      _ptr(outy), C.c_size_t(n), _ptr(err)))
        return outx, outy, err, bad

    def point_lincomb_batch(self, a, b, px, py, curve=CURVE_SECP256K1, plan=MUL_PLAN_AUTO, outx=None, outy=None, err=None):
        """a[i] * G + b[i] * (px[i], py[i]) per element, inputs and codes as for point_mul_batch (the point is checked whatever
        b is): (outx, outy, err, flagged count).  WIRE_INFINITY where the sum is the neutral element."""
        n = self._shape(a)[0]
        outx = outx if outx is not None else self._packed(n)
        outy = outy if outy is not None else self._packed(n)
        err = err if err is not None else self._vec(n, np.uint8)
        bad = self._check(self._L.p2e_point_lincomb_batch(self._h, C.c_int(curve), C.c_uint(plan), _ptr(a), _ptr(b), _ptr(px), _ptr(py),
                                                          _ptr(outx), _ptr(outy), C.c_size_t(n), _ptr(err)))
        return outx, outy, err, bad

    def point_add_batch(self, px, py, qx, qy, curve=CURVE_SECP256K1, outx=None, outy=None, err=None):
        """(px[i], py[i]) + (qx[i], qy[i]) per element, (0, 0) the neutral element: (outx, outy, err, flagged count).  P is
        checked before Q; WIRE_INFINITY where the sum is the neutral element (P = -Q, both neutral)."""
        n = self._shape(px)[0]
        outx = outx if outx is not None else self._packed(n)
        outy = outy if outy is not None else self._packed(n)
        err = err if err is not None else self._vec(n, np.uint8)
        bad = self._check(self._L.p2e_point_add_batch(self._h, C.c_int(curve), _ptr(px), _ptr(py), _ptr(qx), _ptr(qy), _ptr(outx),
                                                      _ptr(outy), C.c_size_t(n), _ptr(err)))
        return outx, outy, err, bad

    # ---- point tables (include/p2e.h p2e_point_table_create and the calls after it) -----------------------------------------
    def point_table(self, px, py, curve=CURVE_SECP256K1, point_err=None):
        """PointTable of the m points (px[j], py[j]), (m, 32) little-endian: see the class."""
        return PointTable(self, px, py, curve, point_err)

    def _table_args(self, table, idx, n):
        if table._h is None:
            raise P2EError("the point table is closed")
        if idx is not None and (self._shape(idx)[0] != n or not _is_u32(idx)):
            raise P2EError("idx must be (n,) uint32 (numpy) / int32 (torch)")

    def point_table_mul_batch(self, table, k, idx=None, outx=None, outy=None, err=None):
        """k[i] * T[idx[i]] per element (idx None: point 0 everywhere; (n,) uint32 / torch int32): (outx, outy, err, flagged
        count), the bytes of point_mul_batch.  WIRE_BAD_INDEX where idx[i] >= len(table), WIRE_INFINITY where k = 0 (mod n)."""
        n = self._shape(k)[0]
        self._table_args(table, idx, n)
        outx = outx if outx is not None else self._packed(n)
        outy = outy if outy is not None else self._packed(n)
        err = err if err is not None else self._vec(n, np.uint8)
        bad = self._check(self._L.p2e_point_table_mul_batch(self._h, table._h, _ptr(idx), _ptr(k), _ptr(outx), _ptr(outy),
                                                            C.c_size_t(n), _ptr(err)))
        return outx, outy, err, bad

    def point_table_lincomb_batch(self, table, a, b, idx=None, outx=None, outy=None, err=None):
        """a[i] * G + b[i] * T[idx[i]] per element: (outx, outy, err, flagged count), the bytes of point_lincomb_batch."""
        n = self._shape(a)[0]
        self._table_args(table, idx, n)
        outx = outx if outx is not None else self._packed(n)
        outy = outy if outy is not None else self._packed(n)
        err = err if err is not None else self._vec(n, np.uint8)
        bad = self._check(self._L.p2e_point_table_lincomb_batch(self._h, table._h, _ptr(idx), _ptr(a), _ptr(b), _ptr(outx), _ptr(outy),
                                                                C.c_size_t(n), _ptr(err)))
        return outx, outy, err, bad

    def ecdsa_verify_table_batch(self, table, msg, r, s, idx=None, err=None, valid=None):
        """The textbook verdict of (msg[i], r[i], s[i]) under key T[idx[i]]: (err, valid, flagged count).  err: WIRE_BAD_INDEX,
        then WIRE_SCALAR_RANGE for r or s outside [1, n); valid is 0 wherever err is not; invalid signatures are not counted."""
        n = self._shape(msg)[0]
        self._table_args(table, idx, n)
        err = err if err is not None else self._vec(n, np.uint8)
        valid = valid if valid is not None else self._vec(n, np.uint8)
        bad = self._check(self._L.p2e_ecdsa_verify_table_batch(self._h, table._h, _ptr(idx), _ptr(msg), _ptr(r), _ptr(s), C.c_size_t(n),
                                                               _ptr(err), _ptr(valid)))
        return err, valid, bad

    # ---- BIP-340 Schnorr signatures on secp256k1 (include/p2e.h p2e_schnorr_public_key_batch and the four calls after it) ------
    def _sig64(self, n):
        if self.host_pointers:
            return np.zeros((n, 64), dtype=np.uint8)
        import torch
        return torch.empty((n, 64), dtype=torch.uint8, device=f"cuda:{self.device}")

    def schnorr_public_key_batch(self, sk, pk=None, err=None):
        """The x-only public keys of (n, 32) BIG-endian secret keys: (pk (n, 32) big-endian, err, flagged count).  sk = 0 or
        sk >= n: zeros and WIRE_SCALAR_RANGE (nothing is reduced)."""
        n = self._shape(sk)[0]
        pk = pk if pk is not None else self._packed(n)
        err = err if err is not None else self._vec(n, np.uint8)
        bad = self._check(self._L.p2e_schnorr_public_key_batch(self._h, _ptr(sk), _ptr(pk), C.c_size_t(n), _ptr(err)))
        return pk, err, bad

    def schnorr_sign_batch(self, msg, sk, aux, sig=None, err=None):
        """BIP-340 default signing of (n, 32) messages under (n, 32) secret keys with (n, 32) auxiliary randomness, all the
        standard's big-endian byte strings: (sig (n, 64) = r || s, err, flagged count).  WIRE_SCALAR_RANGE for a key out of
        range, WIRE_INFINITY for a zero nonce; the fresh signature is not verified."""
        n = self._shape(msg)[0]
        sig = sig if sig is not None else self._sig64(n)
        err = err if err is not None else self._vec(n, np.uint8)
        bad = self._check(self._L.p2e_schnorr_sign_batch(self._h, _ptr(msg), _ptr(sk), _ptr(aux), _ptr(sig), C.c_size_t(n), _ptr(err)))
        return sig, err, bad

    def schnorr_verify_batch(self, msg, pk, sig, err=None, valid=None):
        """The BIP-340 verdict of every (msg (n, 32), pk (n, 32) x-only, sig (n, 64)): (err, valid, flagged count).  err holds
        WIRE_* codes for a malformed key or signature; a well-formed wrong signature has err 0, valid 0 and is not counted."""
        n = self._shape(msg)[0]
        err = err if err is not None else self._vec(n, np.uint8)
        valid = valid if valid is not None else self._vec(n, np.uint8)
        bad = self._check(self._L.p2e_schnorr_verify_batch(self._h, _ptr(msg), _ptr(pk), _ptr(sig), C.c_size_t(n), _ptr(err), _ptr(valid)))
        return err, valid, bad

    def xonly_decode_batch(self, pk, px=None, py=None, err=None):
        """lift_x of (n, 32) big-endian x-only keys: (px, py, err, flagged count), the library's LITTLE-endian affine point
        with even y -- what point_lincomb_batch, point_table, point_msm and point_encode_batch take."""
        n = self._shape(pk)[0]
        px = px if px is not None else self._packed(n)
        py = py if py is not None else self._packed(n)
        err = err if err is not None else self._vec(n, np.uint8)
        bad = self._check(self._L.p2e_xonly_decode_batch(self._h, _ptr(pk), _ptr(px), _ptr(py), C.c_size_t(n), _ptr(err)))
        return px, py, err, bad

    def schnorr_verify_aggregate(self, msg, pk, sig, seed, window_bits=MSM_WINDOW_AUTO, verdict=None, err=None, want_err=True, n=None):
        """BIP-340 batch verification: ONE verdict for the whole batch, (verdict (1,), err (n,) or None, flagged count).
        seed (32,) uint8 must be unpredictable to whoever made the signatures (fresh randomness or a hash of the whole
        batch).  verdict 1 iff nothing is flagged and the randomised sum is the neutral element; on 0 run
        schnorr_verify_batch to find the element.  n: the batch size where it is not msg's first dimension (n = 0)."""
        n = self._shape(msg)[0] if n is None else n
        verdict = verdict if verdict is not None else self._vec(1, np.uint8)
        if err is None and want_err:
            err = self._vec(max(n, 1), np.uint8)[:n]
        bad = self._check(self._L.p2e_schnorr_verify_aggregate(self._h, _ptr(msg), _ptr(pk), _ptr(sig), C.c_size_t(n), _ptr(seed),
                                                                C.c_uint(window_bits), _ptr(verdict), _ptr(err)))
        return verdict, err, bad

    # ---- BIP-32 key derivation and HASH160 on secp256k1 (include/p2e.h p2e_bip32_master_batch and the four calls after it) ------
    @staticmethod
    def _parents(par, n):
        """n_parents of a parent array: its rows, which must be 1 (one parent for the whole batch) or n"""
        m = par.shape[0]
        if m != 1 and m != n:
            raise P2EError("parents must have 1 row or one row per index")
        return m

    def bip32_master_batch(self, seed, sk=None, cc=None, err=None):
        """BIP-32 master keys of (n, seed_len) seeds, 16 <= seed_len <= 64: (sk (n, 32) little-endian, cc (n, 32) chain codes in
        the standard's byte order, err, flagged count).  I_L = 0 or I_L >= n: zeros and WIRE_SCALAR_RANGE."""
        n, seed_len = self._shape(seed)
        sk = sk if sk is not None else self._packed(n)
        cc = cc if cc is not None else self._packed(n)
        err = err if err is not None else self._vec(n, np.uint8)
        bad = self._check(self._L.p2e_bip32_master_batch(self._h, _ptr(seed), C.c_size_t(seed_len), _ptr(sk), _ptr(cc), C.c_size_t(n),
                                                         _ptr(err)))
        return sk, cc, err, bad

    def bip32_ckd_priv_batch(self, par_sk, par_cc, index, sk=None, cc=None, err=None):
        """CKDpriv: child index[i] (uint32; >= 2^31 hardened) of parent i, or of parent 0 where par_sk and par_cc have one row:
        (sk, cc, err, flagged count).  WIRE_SCALAR_RANGE for a parent key or an I_L out of range, WIRE_INFINITY for a zero
        child; a flagged element is all zeros, the chain code included."""
        n = self._shape(index)[0]
        m = self._parents(par_sk, n)
        sk = sk if sk is not None else self._packed(n)
        cc = cc if cc is not None else self._packed(n)
        err = err if err is not None else self._vec(n, np.uint8)
        bad = self._check(self._L.p2e_bip32_ckd_priv_batch(self._h, _ptr(par_sk), _ptr(par_cc), C.c_size_t(m), _ptr(index), _ptr(sk),
                                                           _ptr(cc), C.c_size_t(n), _ptr(err)))
        return sk, cc, err, bad

    def bip32_ckd_pub_batch(self, par_pkx, par_pky, par_cc, index, pkx=None, pky=None, cc=None, err=None):
        """CKDpub: the public key and chain code of the non-hardened child index[i] of parent i, or of parent 0 where the parent
        arrays have one row (the scan of one extended public key): (pkx, pky, cc, err, flagged count).  err, in order:
        WIRE_BAD_INDEX for a hardened index, WIRE_INFINITY / WIRE_COORD_RANGE / WIRE_NOT_ON_CURVE for the parent,
        WIRE_SCALAR_RANGE for I_L >= n, WIRE_INFINITY for a neutral child."""
        n = self._shape(index)[0]
        m = self._parents(par_pkx, n)
        pkx = pkx if pkx is not None else self._packed(n)
        pky = pky if pky is not None else self._packed(n)
        cc = cc if cc is not None else self._packed(n)
        err = err if err is not None else self._vec(n, np.uint8)
        bad = self._check(self._L.p2e_bip32_ckd_pub_batch(self._h, _ptr(par_pkx), _ptr(par_pky), _ptr(par_cc), C.c_size_t(m), _ptr(index),
                                                          _ptr(pkx), _ptr(pky), _ptr(cc), C.c_size_t(n), _ptr(err)))
        return pkx, pky, cc, err, bad

    def key_hash160_batch(self, pkx, pky, form=SEC1_COMPRESSED, err=None, out=None):
        """HASH160 = RIPEMD-160(SHA-256(.)) of the SEC1 form (SEC1_COMPRESSED or SEC1_UNCOMPRESSED) of (n, 32) little-endian
        secp256k1 coordinates: (out (n, 20), 0).  err (n,) uint8, optional: where err[i] != 0 the hash is twenty zero bytes.
        The first four bytes of the compressed form's hash are the key's BIP-32 fingerprint."""
        n = self._shape(pkx)[0]
        out = out if out is not None else self._bytes(n, 20)
        rc = self._check(self._L.p2e_key_hash160_batch(self._h, C.c_uint(form), _ptr(pkx), _ptr(pky), _ptr(err), _ptr(out), C.c_size_t(n)))
        return out, rc

    def hash160_batch(self, data, offsets, out=None):
        """HASH160 of message i = data[offsets[i]:offsets[i + 1]], laid out as for hash_batch: (out (n, 20), count of elements
        with offsets[i + 1] < offsets[i], which are hashed as the empty message)."""
        n = self._shape(offsets)[0] - 1
        out = out if out is not None else self._bytes(n, 20)
        bad = self._check(self._L.p2e_hash160_batch(self._h, _ptr(data), _ptr(offsets), _ptr(out), C.c_size_t(n)))
        return out, bad

    # ---- PBKDF2-HMAC-SHA512 and BIP-39 seeds (include/p2e.h p2e_pbkdf2_hmac_sha512_batch, p2e_bip39_seed_batch) -----------------
    def _var(self, items):
        """(buffer, offsets, elements) of a variable-length operand: a (buffer, offsets) pair as it is -- numpy arrays with
        host_pointers, torch CUDA tensors otherwise --, a list of bytes / str through pack_bytes (uploaded where the context
        takes device pointers)."""
        if isinstance(items, tuple):
            buf, offsets = items
            return buf, offsets, self._shape(offsets)[0] - 1
        buf, offsets = pack_bytes(items)
        if not self.host_pointers:
            import torch
            dev = f"cuda:{self.device}"
            buf, offsets = torch.from_numpy(buf).to(dev), torch.from_numpy(offsets.view(np.int64)).to(dev)
        return buf, offsets, len(items)

    @staticmethod
    def _lanes(what, counts, count):
        """the batch size of operands that hold one element or one per lane"""
        count = max(counts) if count is None else count
        if any(k != 1 and k != count for k in counts):
            raise P2EError(f"{what} must hold one element or one per lane")
        return count

    def pbkdf2_hmac_sha512_batch(self, passwords, salts, iterations, dk_len=64, count=None, dk=None, err=None):
        """PBKDF2-HMAC-SHA512 (RFC 8018), one output block: dk[i] = the first dk_len (a multiple of 4 in 4 .. 64) bytes of
        T = U_1 ^ ... ^ U_iterations under password i and salt i.  passwords and salts are lists of bytes / str (pack_bytes)
        or (buffer, offsets) pairs laid out as for hash_batch; one element serves the whole batch.  (dk (count, dk_len), err,
        flagged count): WIRE_BAD_LENGTH and zeros for reversed offsets or a length >= 2^32."""
        pw, pw_off, n_pw = self._var(passwords)
        sa, sa_off, n_sa = self._var(salts)
        count = self._lanes("passwords and salts", (n_pw, n_sa), count)
        dk = dk if dk is not None else self._bytes(count, dk_len)
        err = err if err is not None else self._vec(count, np.uint8)
        bad = self._check(self._L.p2e_pbkdf2_hmac_sha512_batch(self._h, _ptr(pw), _ptr(pw_off), C.c_size_t(n_pw), _ptr(sa), _ptr(sa_off),
                                                               C.c_size_t(n_sa), C.c_uint32(iterations), C.c_size_t(dk_len), _ptr(dk),
                                                               C.c_size_t(count), _ptr(err)))
        return dk, err, bad

    def bip39_seed_batch(self, mnemonics, passphrases=None, count=None, seed=None, err=None):
        """BIP-39 seeds: seed[i] = PBKDF2-HMAC-SHA512(mnemonic i, "mnemonic" || passphrase i, 2048, 64), what
        bip32_master_batch takes.  Operands as for pbkdf2_hmac_sha512_batch (a str is NFKD-normalised); passphrases=None is
        the empty passphrase.  The wordlist and the checksum are not looked at.  (seed (count, 64), err, flagged count)."""
        mn, mn_off, n_mn = self._var(mnemonics)
        pp, pp_off, n_pp = self._var(passphrases) if passphrases is not None else (None, None, 0)
        count = self._lanes("mnemonics and passphrases", (n_mn, n_pp) if n_pp else (n_mn,), count)
        seed = seed if seed is not None else self._bytes(count, 64)
        err = err if err is not None else self._vec(count, np.uint8)
        bad = self._check(self._L.p2e_bip39_seed_batch(self._h, _ptr(mn), _ptr(mn_off), C.c_size_t(n_mn), _ptr(pp), _ptr(pp_off),
                                                       C.c_size_t(n_pp), _ptr(seed), C.c_size_t(count), _ptr(err)))
        return seed, err, bad

    # ---- Taproot on secp256k1 (include/p2e.h p2e_taproot_leaf_hash_batch and the four calls after it) ---------------------------
    # Every key, hash and tweak is an (n, 32) array of the standard's big-endian byte strings, as in the Schnorr calls.
    def taproot_leaf_hash_batch(self, leaf_version, script, offsets, leaf=None, err=None):
        """H_TapLeaf(version || compact_size(len) || script i), script i = script[offsets[i]:offsets[i + 1]] laid out as for
        hash_batch: (leaf (n, 32), err, flagged count).  WIRE_BAD_PREFIX for an odd version, WIRE_BAD_LENGTH for reversed
        offsets or a length >= 2^32."""
        n = self._shape(offsets)[0] - 1
        leaf = leaf if leaf is not None else self._packed(n)
        err = err if err is not None else self._vec(n, np.uint8)
        bad = self._check(self._L.p2e_taproot_leaf_hash_batch(self._h, _ptr(leaf_version), _ptr(script), _ptr(offsets), _ptr(leaf),
                                                              C.c_size_t(n), _ptr(err)))
        return leaf, err, bad

    @staticmethod
    def _max_depth(path, n):
        """max_depth of a path array (n, max_depth, 32); None: no paths at all (max_depth 0)"""
        if path is None:
            return 0
        if len(path.shape) != 3 or path.shape[0] != n or path.shape[2] != 32:
            raise P2EError("path must be (n, max_depth, 32)")
        return path.shape[1]

    def taproot_merkle_root_batch(self, leaf, path, depth, root=None, err=None):
        """The Merkle root of every leaf (n, 32) under the first depth[i] nodes of path[i] ((n, max_depth, 32), max_depth <= 128;
        None for no paths): (root (n, 32), err, flagged count).  depth[i] > max_depth: zeros and WIRE_BAD_LENGTH."""
        n = self._shape(leaf)[0]
        max_depth = self._max_depth(path, n)
        root = root if root is not None else self._packed(n)
        err = err if err is not None else self._vec(n, np.uint8)
        bad = self._check(self._L.p2e_taproot_merkle_root_batch(self._h, _ptr(leaf), _ptr(path if max_depth else None), _ptr(depth),
                                                                C.c_size_t(max_depth), _ptr(root), C.c_size_t(n), _ptr(err)))
        return root, err, bad

    def taproot_tweak_pubkey_batch(self, pk, root=None, out_pk=None, out_parity=None, err=None):
        """BIP-341 taproot_tweak_pubkey of (n, 32) x-only keys under (n, 32) Merkle roots, or under no root (root=None, the
        key-path-only output of BIP-86): (out_pk (n, 32), out_parity (n,), err, flagged count)."""
        n = self._shape(pk)[0]
        out_pk = out_pk if out_pk is not None else self._packed(n)
        out_parity = out_parity if out_parity is not None else self._vec(n, np.uint8)
        err = err if err is not None else self._vec(n, np.uint8)
        bad = self._check(self._L.p2e_taproot_tweak_pubkey_batch(self._h, _ptr(pk), _ptr(root), _ptr(out_pk), _ptr(out_parity),
                                                                 C.c_size_t(n), _ptr(err)))
        return out_pk, out_parity, err, bad

    def taproot_tweak_seckey_batch(self, sk, root=None, out_sk=None, err=None):
        """BIP-341 taproot_tweak_seckey of (n, 32) secret keys: (out_sk (n, 32), err, flagged count) -- the key that
        schnorr_sign_batch signs a key-path spend with.  The output is secret."""
        n = self._shape(sk)[0]
        out_sk = out_sk if out_sk is not None else self._packed(n)
        err = err if err is not None else self._vec(n, np.uint8)
        bad = self._check(self._L.p2e_taproot_tweak_seckey_batch(self._h, _ptr(sk), _ptr(root), _ptr(out_sk), C.c_size_t(n), _ptr(err)))
        return out_sk, err, bad

    def taproot_verify_commitment_batch(self, out_pk, out_parity, pk, leaf, path, depth, err=None, valid=None):
        """BIP-341's script-path rule behind the leaf hash: does output key out_pk[i] with parity out_parity[i] commit to
        leaf[i] under internal key pk[i] and the first depth[i] nodes of path[i]?  (err, valid, flagged count); a well-formed
        mismatch has err 0, valid 0 and is not counted."""
        n = self._shape(pk)[0]
        max_depth = self._max_depth(path, n)
        err = err if err is not None else self._vec(n, np.uint8)
        valid = valid if valid is not None else self._vec(n, np.uint8)
        bad = self._check(self._L.p2e_taproot_verify_commitment_batch(self._h, _ptr(out_pk), _ptr(out_parity), _ptr(pk), _ptr(leaf),
                                                                      _ptr(path if max_depth else None), _ptr(depth), C.c_size_t(max_depth),
                                                                      C.c_size_t(n), _ptr(err), _ptr(valid)))
        return err, valid, bad

    # ---- silent payments on secp256k1 (include/p2e.h p2e_sp_input_hash_batch and the three calls after it) ----------------------
    # Points and secret keys are (n, 32) little-endian arrays as in the BIP-32 calls; outpoints, input hashes, x-only outputs
    # and tweaks are the standard's big-endian byte strings; label indices, k and hit_output are 32-bit integers.
    def _u32(self, *shape):
        if self.host_pointers:
            return np.zeros(shape, dtype=np.uint32)
        import torch
        return torch.empty(shape, dtype=torch.int32, device=f"cuda:{self.device}")

    def sp_input_hash_batch(self, outpoint, ax, ay, input_hash=None, err=None):
        """BIP-352 input_hash = H_Inputs(outpoint || serP(A)) of (n, 36) outpoints and the points A (ax, ay (n, 32)):
        (input_hash (n, 32) big-endian, err, flagged count)."""
        n = self._shape(ax)[0]
        input_hash = input_hash if input_hash is not None else self._packed(n)
        err = err if err is not None else self._vec(n, np.uint8)
        bad = self._check(self._L.p2e_sp_input_hash_batch(self._h, _ptr(outpoint), _ptr(ax), _ptr(ay), _ptr(input_hash), C.c_size_t(n),
                                                          _ptr(err)))
        return input_hash, err, bad

    def sp_label_batch(self, scan_sk, label_index, label_tweak=None, label_x=None, label_y=None, err=None):
        """The labels label_index (n,) 32-bit of the ONE scan key scan_sk (1, 32): (label_tweak (n, 32) big-endian = l_m,
        label_x, label_y (n, 32) = l_m G, err, flagged count)."""
        n = self._shape(label_index)[0]
        label_tweak = label_tweak if label_tweak is not None else self._packed(n)
        label_x = label_x if label_x is not None else self._packed(n)
        label_y = label_y if label_y is not None else self._packed(n)
        err = err if err is not None else self._vec(n, np.uint8)
        bad = self._check(self._L.p2e_sp_label_batch(self._h, _ptr(scan_sk), _ptr(label_index), _ptr(label_tweak), _ptr(label_x), _ptr(label_y),
                                                     C.c_size_t(n), _ptr(err)))
        return label_tweak, label_x, label_y, err, bad

    def sp_send_batch(self, a_sk, input_hash, scan_pkx, scan_pky, spend_pkx, spend_pky, k, out_pk=None, err=None):
        """The sender's output keys: out_pk[i] = x(B_spend + t_k G), t_k from S = (input_hash a) B_scan and k[i] (32-bit):
        (out_pk (n, 32) big-endian, err, flagged count)."""
        n = self._shape(a_sk)[0]
        out_pk = out_pk if out_pk is not None else self._packed(n)
        err = err if err is not None else self._vec(n, np.uint8)
        bad = self._check(self._L.p2e_sp_send_batch(self._h, _ptr(a_sk), _ptr(input_hash), _ptr(scan_pkx), _ptr(scan_pky), _ptr(spend_pkx),
                                                    _ptr(spend_pky), _ptr(k), _ptr(out_pk), C.c_size_t(n), _ptr(err)))
        return out_pk, err, bad

    def sp_scan_batch(self, scan_sk, spend_pkx, spend_pky, ax, ay, outputs, out_offsets, input_hash=None, label_x=None, label_y=None,
                      max_hits=1, n_hits=None, hit_output=None, hit_label=None, hit_tweak=None, err=None):
        """The receiver's scan of n transactions under ONE scan key and spend key ((1, 32) each) and the labels label_x, label_y
        ((n_labels, 32), or None): transaction i has the input point (ax[i], ay[i]), the input hash input_hash[i] (None: A is
        already multiplied by it) and the x-only outputs outputs[out_offsets[i]:out_offsets[i + 1]] ((total, 32) big-endian,
        out_offsets (n + 1,) 64-bit).  (n_hits (n,), hit_output (n, max_hits) 32-bit, hit_label (n, max_hits), hit_tweak
        (n, max_hits, 32) big-endian, err, flagged count)."""
        n = self._shape(ax)[0]
        n_labels = 0 if label_x is None else self._shape(label_x)[0]
        if not 1 <= max_hits <= 8:
            raise P2EError("max_hits must be 1 .. 8")
        n_hits = n_hits if n_hits is not None else self._vec(n, np.uint8)
        hit_output = hit_output if hit_output is not None else self._u32(n, max_hits)
        hit_label = hit_label if hit_label is not None else self._bytes(n, max_hits)
        hit_tweak = hit_tweak if hit_tweak is not None else self._bytes(n, max_hits, 32)
        err = err if err is not None else self._vec(n, np.uint8)
        bad = self._check(self._L.p2e_sp_scan_batch(self._h, _ptr(scan_sk), _ptr(spend_pkx), _ptr(spend_pky), _ptr(label_x), _ptr(label_y),
                                                    C.c_size_t(n_labels), _ptr(ax), _ptr(ay), _ptr(input_hash), _ptr(outputs), _ptr(out_offsets),
                                                    C.c_size_t(max_hits), _ptr(n_hits), _ptr(hit_output), _ptr(hit_label), _ptr(hit_tweak),
                                                    C.c_size_t(n), _ptr(err)))
        return n_hits, hit_output, hit_label, hit_tweak, err, bad

    # ---- a P + b Q and DLEQ proofs (include/p2e.h p2e_point_lincomb2_batch, p2e_dleq_prove_batch, p2e_dleq_verify_batch) ------------
    def point_lincomb2_batch(self, a, b, px, py, qx, qy, curve=CURVE_SECP256K1, plan=MUL_PLAN_AUTO, outx=None, outy=None, err=None):
        """a[i] * (px[i], py[i]) + b[i] * (qx[i], qy[i]) per element in one joint walk, inputs and codes as for
        point_lincomb_batch (P is checked before Q): (outx, outy, err, flagged count) -- the bytes of point_mul_batch,
        point_mul_batch and point_add_batch.  WIRE_INFINITY where the sum is the neutral element."""
        n = self._shape(a)[0]
        outx = outx if outx is not None else self._packed(n)
        outy = outy if outy is not None else self._packed(n)
        err = err if err is not None else self._vec(n, np.uint8)
        bad = self._check(self._L.p2e_point_lincomb2_batch(self._h, C.c_int(curve), C.c_uint(plan), _ptr(a), _ptr(b), _ptr(px), _ptr(py),
                                                           _ptr(qx), _ptr(qy), _ptr(outx), _ptr(outy), C.c_size_t(n), _ptr(err)))
        return outx, outy, err, bad

    def dleq_prove_batch(self, a_sk, bx, by, aux_rand, msg=None, proof=None, cx=None, cy=None, err=None, want_c=True):
        """The shares C[i] = a[i] B[i] and BIP-374 proofs that they use the a of A = a G: a_sk, bx, by (n, 32) little-endian,
        aux_rand and msg (n, 32) byte strings (msg None: no message): (proof (n, 64) = bytes32(e) || bytes32(s) big-endian,
        cx, cy (n, 32) little-endian or None with want_c=False, err, flagged count).  The fresh proof is not verified."""
        n = self._shape(a_sk)[0]
        proof = proof if proof is not None else self._bytes(n, 64)
        if want_c:
            cx = cx if cx is not None else self._packed(n)
            cy = cy if cy is not None else self._packed(n)
        err = err if err is not None else self._vec(n, np.uint8)
        bad = self._check(self._L.p2e_dleq_prove_batch(self._h, _ptr(a_sk), _ptr(bx), _ptr(by), _ptr(aux_rand), _ptr(msg), _ptr(proof),
                                                       _ptr(cx), _ptr(cy), C.c_size_t(n), _ptr(err)))
        return proof, cx, cy, err, bad

    def dleq_verify_batch(self, ax, ay, bx, by, cx, cy, proof, msg=None, err=None, valid=None):
        """valid[i] = 1 iff proof[i] shows log_G A[i] = log_B[i] C[i] (under msg[i], or no message): (err, valid, flagged
        count).  A well-formed wrong proof is err 0, valid 0 and not counted."""
        n = self._shape(ax)[0]
        err = err if err is not None else self._vec(n, np.uint8)
        valid = valid if valid is not None else self._vec(n, np.uint8)
        bad = self._check(self._L.p2e_dleq_verify_batch(self._h, _ptr(ax), _ptr(ay), _ptr(bx), _ptr(by), _ptr(cx), _ptr(cy), _ptr(proof),
                                                        _ptr(msg), C.c_size_t(n), _ptr(err), _ptr(valid)))
        return err, valid, bad

    # ---- MuSig2 on secp256k1 (include/p2e.h p2e_musig_key_agg_batch and the six calls after it) ------------------------------------
    # Points, secret keys and nonces are little-endian as in the BIP-32 calls (a public nonce is (n, 128) = x(R_1) || y(R_1) ||
    # x(R_2) || y(R_2)); tweaks, messages, partial signatures, agg_pk and sig are the standard's big-endian byte strings; keyagg
    # is the (n, 192) record and session the (n, 128) record of the header.  key_offsets is (n + 1,) 64-bit, in signers.
    def musig_key_agg_batch(self, pkx, pky, key_offsets, keyagg=None, agg_pk=None, err=None):
        """KeyAgg of n sessions: session i owns the keys pkx / pky[key_offsets[i]:key_offsets[i + 1]] ((total, 32)):
        (keyagg (n, 192), agg_pk (n, 32) big-endian, err, flagged count)."""
        n = self._shape(key_offsets)[0] - 1
        keyagg = keyagg if keyagg is not None else self._bytes(n, 192)
        agg_pk = agg_pk if agg_pk is not None else self._packed(n)
        err = err if err is not None else self._vec(n, np.uint8)
        bad = self._check(self._L.p2e_musig_key_agg_batch(self._h, _ptr(pkx), _ptr(pky), _ptr(key_offsets), _ptr(keyagg), _ptr(agg_pk),
                                                          C.c_size_t(n), _ptr(err)))
        return keyagg, agg_pk, err, bad

    def musig_apply_tweak_batch(self, keyagg, tweak, mode, keyagg_out=None, agg_pk=None, err=None):
        """ApplyTweak: mode MUSIG_TWEAK_PLAIN / MUSIG_TWEAK_XONLY with the tweaks tweak (n, 32) big-endian, or MUSIG_TWEAK_TAPROOT with
        tweak the Merkle roots or None (BIP-86).  keyagg_out may be keyagg itself: (keyagg_out, agg_pk, err, flagged count)."""
        n = self._shape(keyagg)[0]
        keyagg_out = keyagg_out if keyagg_out is not None else self._bytes(n, 192)
        agg_pk = agg_pk if agg_pk is not None else self._packed(n)
        err = err if err is not None else self._vec(n, np.uint8)
        bad = self._check(self._L.p2e_musig_apply_tweak_batch(self._h, _ptr(keyagg), _ptr(tweak), C.c_int(mode), _ptr(keyagg_out), _ptr(agg_pk),
                                                              C.c_size_t(n), _ptr(err)))
        return keyagg_out, agg_pk, err, bad

    def musig_nonce_agg_batch(self, pubnonce, key_offsets, aggnonce=None, err=None):
        """NonceAgg: session i sums the public nonces pubnonce[key_offsets[i]:key_offsets[i + 1]] ((total, 128)):
        (aggnonce (n, 128), err, flagged count)."""
        n = self._shape(key_offsets)[0] - 1
        aggnonce = aggnonce if aggnonce is not None else self._bytes(n, 128)
        err = err if err is not None else self._vec(n, np.uint8)
        bad = self._check(self._L.p2e_musig_nonce_agg_batch(self._h, _ptr(pubnonce), _ptr(key_offsets), _ptr(aggnonce), C.c_size_t(n), _ptr(err)))
        return aggnonce, err, bad

    def musig_session_batch(self, keyagg, aggnonce, msg, session=None, err=None):
        """The session values b, e and R of n sessions: (session (n, 128), err, flagged count)."""
        n = self._shape(keyagg)[0]
        session = session if session is not None else self._bytes(n, 128)
        err = err if err is not None else self._vec(n, np.uint8)
        bad = self._check(self._L.p2e_musig_session_batch(self._h, _ptr(keyagg), _ptr(aggnonce), _ptr(msg), _ptr(session), C.c_size_t(n),
                                                          _ptr(err)))
        return session, err, bad

    def musig_partial_sign_batch(self, secnonce, sk, keyagg, session, psig=None, err=None):
        """The caller's partial signature in each of n sessions from secnonce (n, 64) = k_1 || k_2 and sk (n, 32), little-endian.
        A secret nonce must never be used twice.  (psig (n, 32) big-endian, err, flagged count)."""
        n = self._shape(sk)[0]
        psig = psig if psig is not None else self._packed(n)
        err = err if err is not None else self._vec(n, np.uint8)
        bad = self._check(self._L.p2e_musig_partial_sign_batch(self._h, _ptr(secnonce), _ptr(sk), _ptr(keyagg), _ptr(session), _ptr(psig),
                                                               C.c_size_t(n), _ptr(err)))
        return psig, err, bad

    def musig_partial_verify_batch(self, psig, pubnonce, pkx, pky, keyagg, session, session_index=None, err=None, valid=None):
        """PartialSigVerify of n partial signatures; signature i belongs to session session_index[i] ((n,) 32-bit; None: i) of the
        records keyagg / session: (err, valid, flagged count)."""
        n = self._shape(psig)[0]
        err = err if err is not None else self._vec(n, np.uint8)
        valid = valid if valid is not None else self._vec(n, np.uint8)
        bad = self._check(self._L.p2e_musig_partial_verify_batch(self._h, _ptr(psig), _ptr(pubnonce), _ptr(pkx), _ptr(pky), _ptr(session_index),
                                                                 _ptr(keyagg), _ptr(session), C.c_size_t(self._shape(keyagg)[0]), C.c_size_t(n),
                                                                 _ptr(err), _ptr(valid)))
        return err, valid, bad

    def musig_sig_agg_batch(self, psig, key_offsets, keyagg, session, sig=None, err=None):
        """PartialSigAgg: session i sums psig[key_offsets[i]:key_offsets[i + 1]] ((total, 32) big-endian): (sig (n, 64), err,
        flagged count).  p2e_schnorr_verify_batch accepts sig under the session's agg_pk."""
        n = self._shape(key_offsets)[0] - 1
        sig = sig if sig is not None else self._bytes(n, 64)
        err = err if err is not None else self._vec(n, np.uint8)
        bad = self._check(self._L.p2e_musig_sig_agg_batch(self._h, _ptr(psig), _ptr(key_offsets), _ptr(keyagg), _ptr(session), _ptr(sig),
                                                          C.c_size_t(n), _ptr(err)))
        return sig, err, bad

    # ---- hashing, RFC 6979 nonces, the deterministic signer, addresses (include/p2e.h p2e_hash_batch and the three after it) ----
    def hash_batch(self, data, offsets, alg=HASH_SHA256, out_form=DIGEST_BYTES, out=None):
        """Hash message i = data[offsets[i]:offsets[i + 1]] for i < n = len(offsets) - 1: data a 1-D uint8 buffer (any
        alignment, messages concatenated without padding), offsets (n + 1,) int64 / uint64.  alg: HASH_SHA256, HASH_SHA256D,
        HASH_KECCAK256 (Ethereum's, not SHA3-256); out_form: DIGEST_BYTES, or DIGEST_SCALAR = the msg32 of the signing calls.
        (out (n, 32), count of elements with offsets[i + 1] < offsets[i]: those are hashed as the empty message)."""
        n = self._shape(offsets)[0] - 1
        out = out if out is not None else self._packed(n)
        bad = self._check(self._L.p2e_hash_batch(self._h, C.c_int(alg), C.c_uint(out_form), _ptr(data), _ptr(offsets), _ptr(out),
                                                 C.c_size_t(n)))
        return out, bad

    def ecdsa_nonce_rfc6979_batch(self, msg, sk, curve=CURVE_SECP256K1, k=None):
        """The RFC 6979 nonce (HMAC-SHA256) of every (msg, sk), both (n, 32) little-endian and taken modulo the group order as
        the signer takes them: (k (n, 32) little-endian with 1 <= k < n, 0).  The output is secret."""
        n = self._shape(msg)[0]
        k = k if k is not None else self._packed(n)
        rc = self._check(self._L.p2e_ecdsa_nonce_rfc6979_batch(self._h, C.c_int(curve), _ptr(msg), _ptr(sk), _ptr(k), C.c_size_t(n)))
        return k, rc

    def ecdsa_sign_deterministic_batch(self, msg, sk, curve=CURVE_SECP256K1, plan=SIGN_PLAN_AUTO, r=None, s=None, v=None, err=None,
                                       recoverable=True):
        """ecdsa_sign_recoverable_batch with the nonces of ecdsa_nonce_rfc6979_batch, which never leave the library:
        (r, s, v, err, flagged count), bit for bit.  recoverable=False: no v is written (None is returned in its place) and
        the outputs are ecdsa_sign_batch's.  r = 0 or s = 0 are returned unflagged (RFC 6979's retry for them is not done)."""
        n = self._shape(msg)[0]
        r = r if r is not None else self._packed(n)
        s = s if s is not None else self._packed(n)
        if recoverable:
            v = v if v is not None else self._vec(n, np.uint8)
        else:
            v = None
        err = err if err is not None else self._vec(n, np.uint8)
        bad = self._check(self._L.p2e_ecdsa_sign_deterministic_batch(self._h, C.c_int(curve), C.c_uint(plan), _ptr(msg), _ptr(sk), _ptr(r),
                                                                     _ptr(s), _ptr(v), C.c_size_t(n), _ptr(err)))
        return r, s, v, err, bad

    def eth_address_batch(self, pkx, pky, err=None, addr=None):
        """Ethereum addresses keccak256(BE32(pkx) || BE32(pky))[12:] of (n, 32) little-endian secp256k1 coordinates:
        (addr (n, 20), 0).  err (n,) uint8, optional: where err[i] != 0 the address is twenty zero bytes (pass
        ecdsa_recover_batch's err, whose flagged elements hold zero coordinates)."""
        n = self._shape(pkx)[0]
        if addr is None:
            if self.host_pointers:
                addr = np.zeros((n, 20), dtype=np.uint8)
            else:
                import torch
                addr = torch.empty((n, 20), dtype=torch.uint8, device=f"cuda:{self.device}")
        rc = self._check(self._L.p2e_eth_address_batch(self._h, _ptr(pkx), _ptr(pky), _ptr(err), _ptr(addr), C.c_size_t(n)))
        return addr, rc

    # ---- keys and signatures in wire form (include/p2e.h p2e_point_decode_batch and the three after it) ---------------
    def _bytes(self, *shape):
        if self.host_pointers:
            return np.zeros(shape, dtype=np.uint8)
        import torch
        return torch.empty(shape, dtype=torch.uint8, device=f"cuda:{self.device}")

    def point_decode_batch(self, data, offsets, curve=CURVE_SECP256K1, px=None, py=None, err=None):
        """SEC1 public keys (00 | 02 x | 03 x | 04 x y, big-endian) -> little-endian coordinates.  Key i =
        data[offsets[i]:offsets[i + 1]] as in hash_batch.  (px (n, 32), py (n, 32), err (n,), flagged count); err[i] is a
        WIRE_* code, zeros are written where it is not 0."""
        n = self._shape(offsets)[0] - 1
        px = px if px is not None else self._packed(n)
        py = py if py is not None else self._packed(n)
        err = err if err is not None else self._vec(n, np.uint8)
        bad = self._check(self._L.p2e_point_decode_batch(self._h, C.c_int(curve), _ptr(data), _ptr(offsets), _ptr(px), _ptr(py),
                                                         C.c_size_t(n), _ptr(err)))
        return px, py, err, bad

    def point_encode_batch(self, px, py, curve=CURVE_SECP256K1, form=SEC1_COMPRESSED, out=None, err=None):
        """Little-endian coordinates -> SEC1 keys at a fixed stride: (out (n, 33 | 65), err (n,) WIRE_* codes, flagged count)."""
        n = self._shape(px)[0]
        out = out if out is not None else self._bytes(n, 33 if form == SEC1_COMPRESSED else 65)
        err = err if err is not None else self._vec(n, np.uint8)
        bad = self._check(self._L.p2e_point_encode_batch(self._h, C.c_int(curve), C.c_int(form), _ptr(px), _ptr(py), _ptr(out),
                                                         C.c_size_t(n), _ptr(err)))
        return out, err, bad

    def sig_decode_batch(self, data, offsets=None, curve=CURVE_SECP256K1, form=SIG_DER, flags=0, n=None, r=None, s=None, v=None,
                         err=None, want_v=True):
        """Signatures in wire form -> (r, s, v, err, flagged count).  SIG_DER: strict DER, element i = data[offsets[i]:
        offsets[i + 1]];  SIG_COMPACT64 / SIG_COMPACT65: (n, 64) r || s or (n, 65) r || s || v, no offsets.  v is the 65th
        byte as it is (None outside SIG_COMPACT65 or with want_v=False).  flags: 0, SIG_REQUIRE_LOW_S or SIG_NORMALIZE_S."""
        if n is None:
            n = self._shape(offsets)[0] - 1 if form == SIG_DER else self._shape(data)[0]
        r = r if r is not None else self._packed(n)
        s = s if s is not None else self._packed(n)
        if form == SIG_COMPACT65 and want_v:
            v = v if v is not None else self._vec(n, np.uint8)
        else:
            v = None
        err = err if err is not None else self._vec(n, np.uint8)
        bad = self._check(self._L.p2e_sig_decode_batch(self._h, C.c_int(curve), C.c_int(form), C.c_uint(flags), _ptr(data),
                                                       _ptr(offsets), _ptr(r), _ptr(s), _ptr(v), C.c_size_t(n), _ptr(err)))
        return r, s, v, err, bad

    def sig_encode_batch(self, r, s, v=None, curve=CURVE_SECP256K1, form=SIG_DER, flags=0, out=None, out_len=None, err=None):
        """(r, s[, v]) -> wire form: (out, out_len, err, flagged count).  SIG_DER: out (n, 72), the minimal encoding
        zero-filled, out_len (n,) its length;  SIG_COMPACT64 / SIG_COMPACT65: out (n, 64 | 65), out_len None.
        flags: 0 or SIG_NORMALIZE_S."""
        n = self._shape(r)[0]
        out = out if out is not None else self._bytes(n, {SIG_DER: SIG_DER_STRIDE, SIG_COMPACT64: 64}.get(form, 65))
        if form == SIG_DER:
            out_len = out_len if out_len is not None else self._vec(n, np.uint8)
        else:
            out_len = None
        err = err if err is not None else self._vec(n, np.uint8)
        bad = self._check(self._L.p2e_sig_encode_batch(self._h, C.c_int(curve), C.c_int(form), C.c_uint(flags), _ptr(r), _ptr(s),
                                                       _ptr(v), _ptr(out), _ptr(out_len), C.c_size_t(n), _ptr(err)))
        return out, out_len, err, bad

    def _compact_out(self, program, n, narrow, wide, ld_narrow, ld_wide):
        _m, nn, nw = compact_layout(program)
        if narrow is None or wide is None:
            ldp = n + 16 if (not self.host_pointers and n >= 4096 and n & (n - 1) == 0) else n   # see ecdsa_verify_witness_batch
            if self.host_pointers:
                narrow, wide = np.zeros((nn, ldp), dtype=np.uint32), np.zeros((nw, ldp), dtype=np.uint64)
            else:
                import torch
                dev = f"cuda:{self.device}"
                narrow = torch.empty((nn, ldp), dtype=torch.int32, device=dev)
                wide = torch.empty((nw, ldp), dtype=torch.int64, device=dev)
            # same convention as ecdsa_verify_witness_batch: (k, n) views whose row stride is the padded one
            narrow, wide = narrow[:, :n], wide[:, :n]
        return narrow, wide, ld_narrow or _ld(narrow), ld_wide or _ld(wide)

    def ecdsa_verify_witness_compact_batch(self, msg, r, s, pkx, pky, narrow=None, wide=None, err=None, valid=None,
                                           ld_narrow=None, ld_wide=None):
        """ecdsa_verify_witness_batch writing the compact container (include/p2e.h): (narrow u32, wide u64, err, valid, bad)."""
        n = self._shape(msg)[0]
        narrow, wide, ldn, ldw = self._compact_out(PROGRAM_VERIFY, n, narrow, wide, ld_narrow, ld_wide)
        err = err if err is not None else self._vec(n, np.uint8)
        valid = valid if valid is not None else self._vec(n, np.uint8)
        bad = self._check(self._L.p2e_ecdsa_verify_witness_compact_batch(
            self._h, _ptr(msg), _ptr(r), _ptr(s), _ptr(pkx), _ptr(pky), _ptr(narrow), C.c_size_t(ldn), _ptr(wide), C.c_size_t(ldw),
            C.c_size_t(n), _ptr(err), _ptr(valid)))
        return narrow, wide, err, valid, bad

    def glv_mul_witness_compact_batch(self, px, py, k, narrow=None, wide=None, err=None, valid=None, ld_narrow=None, ld_wide=None):
        n = self._shape(px)[0]
        narrow, wide, ldn, ldw = self._compact_out(PROGRAM_GLV_MUL, n, narrow, wide, ld_narrow, ld_wide)
        err = err if err is not None else self._vec(n, np.uint8)
        valid = valid if valid is not None else self._vec(n, np.uint8)
        bad = self._check(self._L.p2e_glv_mul_witness_compact_batch(
            self._h, _ptr(px), _ptr(py), _ptr(k), _ptr(narrow), C.c_size_t(ldn), _ptr(wide), C.c_size_t(ldw), C.c_size_t(n),
            _ptr(err), _ptr(valid)))
        return narrow, wide, err, valid, bad

    def aux_witness_compact_batch(self, program, pky, narrow, n=None, ld_narrow=None, aux32=None, err=None, ld_aux=None):
        """aux_witness_batch inside the compact container: reads the narrow u32 matrix, writes a u32 aux matrix."""
        n = n if n is not None else self._shape(pky)[0]
        ld_narrow = ld_narrow if ld_narrow is not None else _ld(narrow)
        if aux32 is None:
            k = VERIFY_AUX_COLS if program == PROGRAM_VERIFY else GLV_MUL_AUX_COLS
            if self.host_pointers:
                aux32 = np.zeros((k, n), dtype=np.uint32)
            else:
                import torch
                aux32 = torch.empty((k, n), dtype=torch.int32, device=f"cuda:{self.device}")
        ld_aux = ld_aux if ld_aux is not None else _ld(aux32)
        err = err if err is not None else self._vec(n, np.uint8)
        bad = self._check(self._L.p2e_aux_witness_compact_batch(self._h, C.c_int(program), _ptr(pky), _ptr(narrow),
                                                                C.c_size_t(ld_narrow), _ptr(aux32), C.c_size_t(ld_aux),
                                                                C.c_size_t(n), _ptr(err)))
        return aux32, err, bad

    def gate_internal_compact_batch(self, program, aux32, n=None, ld_aux=None, gate=None, ld_gate=None):
        """gate_internal_batch from the u32 aux matrix of aux_witness_compact_batch: (10703 | 5621, n) uint64."""
        n = n if n is not None else self._shape(aux32)[1]
        ld_aux = ld_aux if ld_aux is not None else _ld(aux32)
        if gate is None:
            gate = self._cols(VERIFY_GATE_COLS if program == PROGRAM_VERIFY else GLV_MUL_GATE_COLS, n)
        ld_gate = ld_gate if ld_gate is not None else _ld(gate)
        self._check(self._L.p2e_gate_internal_compact_batch(self._h, C.c_int(program), _ptr(aux32), C.c_size_t(ld_aux), _ptr(gate),
                                                            C.c_size_t(ld_gate), C.c_size_t(n)))
        return gate

    def ux_witness_compact_batch(self, program, inputs, narrow, aux32, n=None, ld_narrow=None, ld_aux=None, ux=None, ld_ux=None,
                                 err=None, u32=True):
        """ux_witness_batch inside the compact container: reads the narrow u32 matrix and the u32 aux matrix (same values,
        half the bytes read).  inputs as ux_witness_batch."""
        if program == PROGRAM_VERIFY:
            msg, r, s, pkx, pky = inputs
        else:
            pkx, pky, msg = inputs
            r = s = None
        n = n if n is not None else self._shape(pky)[0]
        ld_narrow = ld_narrow if ld_narrow is not None else _ld(narrow)
        ld_aux = ld_aux if ld_aux is not None else _ld(aux32)
        if ux is None:
            ux = self._mat(VERIFY_UX_COLS if program == PROGRAM_VERIFY else GLV_MUL_UX_COLS, n, u32)
        else:
            u32 = _is_u32(ux)
        ld_ux = ld_ux if ld_ux is not None else _ld(ux)
        err = err if err is not None else self._vec(n, np.uint8)
        bad = self._check(self._L.p2e_ux_witness_compact_batch(
            self._h, C.c_int(program), _ptr(msg), _ptr(r), _ptr(s), _ptr(pkx), _ptr(pky), _ptr(narrow), C.c_size_t(ld_narrow),
            _ptr(aux32), C.c_size_t(ld_aux), _ptr(ux), C.c_int(1 if u32 else 0), C.c_size_t(ld_ux), C.c_size_t(n), _ptr(err)))
        return ux, err, bad

    def assemble_wires_compact(self, wmap, narrow=None, wide=None, aux32=None, ux=None, gate=None, wires=None, n=None):
        """assemble_wires from the compact container and the u32 aux matrix; the same map serves both.  narrow / wide may
        be None if no entry of the map names a column of it."""
        ref = next(m for m in (narrow, wide, aux32, ux, gate) if m is not None)
        n = n if n is not None else self._shape(ref)[1]
        cells = wmap.num_wires * wmap.degree
        if wires is None:
            if self.host_pointers:
                wires = np.zeros((n, cells), dtype=np.uint64)
            else:
                import torch
                wires = torch.zeros((n, cells), dtype=torch.int64, device=f"cuda:{self.device}")
        u32 = int(_is_u32(ux)) if ux is not None else 0

        def ld(m):
            return C.c_size_t(_ld(m) if m is not None else 0)

        self._check(self._L.p2e_assemble_wires_compact(self._h, wmap._h, _ptr(narrow), ld(narrow), _ptr(wide), ld(wide), _ptr(aux32),
                                                       ld(aux32), _ptr(ux), C.c_int(u32), ld(ux), _ptr(gate), ld(gate), _ptr(wires),
                                                       C.c_size_t(_ld(wires)), C.c_size_t(n)))
        return wires

    def glv_mul_witness_batch(self, px, py, k, cols=None, err=None, valid=None, ld=None):
        """glv_mul (gadgets/glv.rs:87-104): (65243, n) Goldilocks columns."""
        n = self._shape(px)[0]
        cols = cols if cols is not None else self._cols(GLV_MUL_COLS, n)
        err = err if err is not None else self._vec(n, np.uint8)
        valid = valid if valid is not None else self._vec(n, np.uint8)
        ld = ld if ld is not None else _ld(cols)
        bad = self._check(self._L.p2e_glv_mul_witness_batch(self._h, _ptr(px), _ptr(py), _ptr(k), _ptr(cols),
                                                            C.c_size_t(n), C.c_size_t(ld), _ptr(err), _ptr(valid)))
        return cols, err, valid, bad
