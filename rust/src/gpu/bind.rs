//! Column <-> Target binding and the batch fill.  Source only (see rust/README.md).
//!
//! While the circuit is built, every hot-path generator's output targets are recorded in registration order -- the
//! order `p2e_schedule_describe(0, ..)` lists, checked in the shipping repository against two independent walks of
//! the gadgets (tests/test_host.py, tests/test_check_circuit.py):
//!   NonNativeAddition / Subtraction (gadgets/nonnative.rs:254,365)   sum.value.limbs[0..9], overflow.target
//!   NonNativeMultipleAdds (:323)                                     sum.value.limbs[0..9], overflow.0
//!   NonNativeInverse (:511)                                          inv.limbs[0..9], div.limbs[0..9]
//!   MulNonnativeGate row, CheckSumGate row (:396-449)                wires r(0..9), q(0..9), check_sum(0..17), then b(0..16)
//!   GLVDecomposition (gadgets/glv.rs:67)                             k1.limbs[0..5], k2.limbs[0..5], k1_neg, k2_neg
use std::ffi::CStr;

use anyhow::{ensure, Result};
use num::BigUint;
use plonky2::field::types::{Field, PrimeField};
use plonky2::hash::hash_types::RichField;
use plonky2::iop::target::Target;
use plonky2::iop::witness::{PartialWitness, WitnessWrite};

use super::ffi::*;

/// Output targets of the 3 555 hot-path generators, in registration order (len == 82 615).
pub struct HotPathBinding {
    pub targets: Vec<Target>,
}

/// One signature's inputs as the circuit sees them (gadgets/ecdsa.rs:30-36).
pub struct VerifyInput {
    pub msg: BigUint,
    pub r: BigUint,
    pub s: BigUint,
    pub pk_x: BigUint,
    pub pk_y: BigUint,
}

fn pack32(vals: impl Iterator<Item = BigUint>, n: usize) -> Vec<u8> {
    let mut out = vec![0u8; 32 * n];
    for (i, v) in vals.enumerate() {
        let b = v.to_bytes_le();
        out[32 * i..32 * i + b.len()].copy_from_slice(&b); // values are < 2^256 (from_noncanonical_biguint would panic otherwise)
    }
    out
}

/// Pre-seeds one `PartialWitness` per signature with every hot-path generator output, so that
/// `generate_partial_witness` finds them set (a generator's `run_once` may then start with
/// `if witness.contains_all(&outputs) { return Ok(()) }`).  `ctx` was created with `P2E_CTX_HOST_POINTERS`.
pub fn fill_partial_witnesses<F: RichField>(
    binding: &HotPathBinding,
    ctx: *mut P2eCtx,
    sigs: &[VerifyInput],
    pws: &mut [PartialWitness<F>],
) -> Result<()> {
    let n = sigs.len();
    ensure!(binding.targets.len() == P2E_VERIFY_COLS && pws.len() == n);
    let msg = pack32(sigs.iter().map(|s| s.msg.clone()), n);
    let r = pack32(sigs.iter().map(|s| s.r.clone()), n);
    let s = pack32(sigs.iter().map(|s| s.s.clone()), n);
    let px = pack32(sigs.iter().map(|s| s.pk_x.clone()), n);
    let py = pack32(sigs.iter().map(|s| s.pk_y.clone()), n);
    let mut cols = vec![0u64; P2E_VERIFY_COLS * n]; // column-major over the batch: cols[c * n + i]
    let (mut err, mut valid) = (vec![0u8; n], vec![0u8; n]);
    let rc = unsafe {
        p2e_ecdsa_verify_witness_batch(ctx, msg.as_ptr(), r.as_ptr(), s.as_ptr(), px.as_ptr(), py.as_ptr(), cols.as_mut_ptr(),
                                       n, n, err.as_mut_ptr(), valid.as_mut_ptr())
    };
    ensure!(rc >= 0, "p2e: {}", unsafe { CStr::from_ptr(p2e_last_error()) }.to_string_lossy());
    for i in 0..n {
        // where err != 0 the reference generators panic (inverse of zero, limb range ...): surface it as Err
        ensure!(err[i] == 0, "signature {i}: witness generation error bits {:#x}", err[i]);
        for (c, t) in binding.targets.iter().enumerate() {
            pws[i].set_target(*t, F::from_canonical_u64(cols[c * n + i]))?;
        }
    }
    Ok(())
}

/// The wire map of `p2e_assemble_wires` / `p2e_assemble_wires_compact` from the same binding (one map serves the u64
/// matrices and the compact container): a target that is a gate wire lands at
/// `wire * degree + row` of the proof's wire matrix; virtual targets are reached through the copies plonky2
/// records for them and are left to `generate_partial_witness`.
pub fn wire_map_of(binding: &HotPathBinding, degree: usize) -> Vec<P2eWireMapEntry> {
    binding
        .targets
        .iter()
        .enumerate()
        .filter_map(|(c, t)| match t {
            Target::Wire(w) => Some(P2eWireMapEntry { src: P2E_WIRE_SRC_COLS | c as u32, dst: (w.column * degree + w.row) as u32 }),
            Target::VirtualTarget { .. } => None,
        })
        .collect()
}

/// `ECDSASecretKey::to_public` (curve/ecdsa.rs:16-20) for a batch, on `P2E_CURVE_SECP256K1` or `P2E_CURVE_P256`: affine
/// `(x, y)` of `sk * G` per key.  A key that is 0 modulo the group order has no affine public key (the reference returns
/// `AffinePoint::ZERO`): surfaced as `Err`.  `ctx` was created with `P2E_CTX_HOST_POINTERS`.
pub fn public_keys(ctx: *mut P2eCtx, curve: i32, sks: &[BigUint]) -> Result<Vec<(BigUint, BigUint)>> {
    let n = sks.len();
    let sk = pack32(sks.iter().cloned(), n);
    let (mut px, mut py, mut err) = (vec![0u8; 32 * n], vec![0u8; 32 * n], vec![0u8; n]);
    let rc = unsafe {
        p2e_ecdsa_public_key_batch(ctx, curve, P2E_SIGN_PLAN_AUTO, sk.as_ptr(), px.as_mut_ptr(), py.as_mut_ptr(), n, err.as_mut_ptr())
    };
    ensure!(rc >= 0, "p2e: {}", unsafe { CStr::from_ptr(p2e_last_error()) }.to_string_lossy());
    (0..n)
        .map(|i| {
            ensure!(err[i] == 0, "secret key {i}: no affine public key (error bits {:#x})", err[i]);
            Ok((BigUint::from_bytes_le(&px[32 * i..32 * i + 32]), BigUint::from_bytes_le(&py[32 * i..32 * i + 32])))
        })
        .collect()
}

/// `sign_message` (curve/ecdsa.rs:25-40) for a batch with the caller's nonces: `(r, s)` per `(msg, sk, k)`.  A nonce that
/// is 0 modulo the group order (where the reference draws another one) is surfaced as `Err`; `r == 0` or `s == 0` are
/// returned as computed, as the reference returns them.
pub fn sign_messages(ctx: *mut P2eCtx, curve: i32, msgs: &[BigUint], sks: &[BigUint], nonces: &[BigUint]) -> Result<Vec<(BigUint, BigUint)>> {
    let n = msgs.len();
    ensure!(sks.len() == n && nonces.len() == n);
    let (msg, sk, k) = (pack32(msgs.iter().cloned(), n), pack32(sks.iter().cloned(), n), pack32(nonces.iter().cloned(), n));
    let (mut r, mut s, mut err) = (vec![0u8; 32 * n], vec![0u8; 32 * n], vec![0u8; n]);
    let rc = unsafe {
        p2e_ecdsa_sign_batch(ctx, curve, P2E_SIGN_PLAN_AUTO, msg.as_ptr(), sk.as_ptr(), k.as_ptr(), r.as_mut_ptr(), s.as_mut_ptr(), n,
                             err.as_mut_ptr())
    };
    ensure!(rc >= 0, "p2e: {}", unsafe { CStr::from_ptr(p2e_last_error()) }.to_string_lossy());
    (0..n)
        .map(|i| {
            ensure!(err[i] == 0, "signature {i}: unusable nonce (error bits {:#x})", err[i]);
            Ok((BigUint::from_bytes_le(&r[32 * i..32 * i + 32]), BigUint::from_bytes_le(&s[32 * i..32 * i + 32])))
        })
        .collect()
}

/// Public keys of a batch of `(msg, r, s, v)` signatures (`p2e_ecdsa_recover_batch`, host-pointer context): `v` without any
/// offset (bit 0 = parity of R.y, bit 1 = R.x >= n).  `None` where the signature names no key (error bits in the library's
/// err byte: not recoverable, or the neutral element).
pub fn recover_public_keys(ctx: *mut P2eCtx, curve: i32, msgs: &[BigUint], sigs: &[(BigUint, BigUint, u8)]) -> Result<Vec<Option<(BigUint, BigUint)>>> {
    let n = msgs.len();
    ensure!(sigs.len() == n);
    let msg = pack32(msgs.iter().cloned(), n);
    let (r, s) = (pack32(sigs.iter().map(|t| t.0.clone()), n), pack32(sigs.iter().map(|t| t.1.clone()), n));
    let v: Vec<u8> = sigs.iter().map(|t| t.2).collect();
    let (mut pkx, mut pky, mut err) = (vec![0u8; 32 * n], vec![0u8; 32 * n], vec![0u8; n]);
    let rc = unsafe {
        p2e_ecdsa_recover_batch(ctx, curve, msg.as_ptr(), r.as_ptr(), s.as_ptr(), v.as_ptr(), pkx.as_mut_ptr(), pky.as_mut_ptr(), n,
                                err.as_mut_ptr())
    };
    ensure!(rc >= 0, "p2e: {}", unsafe { CStr::from_ptr(p2e_last_error()) }.to_string_lossy());
    Ok((0..n)
        .map(|i| {
            (err[i] == 0).then(|| (BigUint::from_bytes_le(&pkx[32 * i..32 * i + 32]), BigUint::from_bytes_le(&pky[32 * i..32 * i + 32])))
        })
        .collect())
}

/// `sign_messages` with the recovery byte: `(r, s, v)` per message (`p2e_ecdsa_sign_recoverable_batch`).
pub fn sign_messages_recoverable(ctx: *mut P2eCtx, curve: i32, msgs: &[BigUint], sks: &[BigUint], nonces: &[BigUint]) -> Result<Vec<(BigUint, BigUint, u8)>> {
    let n = msgs.len();
    ensure!(sks.len() == n && nonces.len() == n);
    let (msg, sk, k) = (pack32(msgs.iter().cloned(), n), pack32(sks.iter().cloned(), n), pack32(nonces.iter().cloned(), n));
    let (mut r, mut s, mut v, mut err) = (vec![0u8; 32 * n], vec![0u8; 32 * n], vec![0u8; n], vec![0u8; n]);
    let rc = unsafe {
        p2e_ecdsa_sign_recoverable_batch(ctx, curve, P2E_SIGN_PLAN_AUTO, msg.as_ptr(), sk.as_ptr(), k.as_ptr(), r.as_mut_ptr(),
                                         s.as_mut_ptr(), v.as_mut_ptr(), n, err.as_mut_ptr())
    };
    ensure!(rc >= 0, "p2e: {}", unsafe { CStr::from_ptr(p2e_last_error()) }.to_string_lossy());
    (0..n)
        .map(|i| {
            ensure!(err[i] == 0, "signature {i}: unusable nonce (error bits {:#x})", err[i]);
            Ok((BigUint::from_bytes_le(&r[32 * i..32 * i + 32]), BigUint::from_bytes_le(&s[32 * i..32 * i + 32]), v[i]))
        })
        .collect()
}

/// The sum `Σ k_i · P_i` of a batch of points (`p2e_point_msm`, host-pointer context), the many-point sum of
/// curve/curve_msm.rs `msm_parallel`.  A point `None` (or `(0, 0)`) is the neutral element and contributes nothing.
/// `Ok(None)`: the sum is the neutral element.  `Err`: the call failed, or some point is not on the curve (the message
/// names the first one); nothing is summed without the rejected points.
pub fn point_msm(ctx: *mut P2eCtx, curve: i32, scalars: &[BigUint], points: &[Option<(BigUint, BigUint)>]) -> Result<Option<(BigUint, BigUint)>> {
    let n = scalars.len();
    ensure!(points.len() == n);
    let zero = (BigUint::default(), BigUint::default());
    let k = pack32(scalars.iter().cloned(), n);
    let px = pack32(points.iter().map(|p| p.as_ref().unwrap_or(&zero).0.clone()), n);
    let py = pack32(points.iter().map(|p| p.as_ref().unwrap_or(&zero).1.clone()), n);
    let (mut outx, mut outy, mut status, mut point_err) = ([0u8; 32], [0u8; 32], 0u8, vec![0u8; n]);
    let rc = unsafe {
        p2e_point_msm(ctx, curve, P2E_MSM_WINDOW_AUTO, k.as_ptr(), px.as_ptr(), py.as_ptr(), n, outx.as_mut_ptr(), outy.as_mut_ptr(),
                      &mut status, point_err.as_mut_ptr())
    };
    ensure!(rc >= 0, "p2e: {}", unsafe { CStr::from_ptr(p2e_last_error()) }.to_string_lossy());
    ensure!(status != P2E_MSM_BAD_POINT, "{rc} points are not on the curve, the first at index {:?}", point_err.iter().position(|&e| e != 0));
    Ok((status == P2E_MSM_OK).then(|| (BigUint::from_bytes_le(&outx), BigUint::from_bytes_le(&outy))))
}

/// The window tables of a set of keys (`p2e_point_table_create`, host-pointer context): built once, then every
/// multiplication by one of the keys is at most 64 mixed additions.  The borrow of the context keeps it alive for as long
/// as the table exists; dropping the table waits for the context's stream and frees the device memory.
pub struct PointTable<'c> {
    ctx: &'c P2eCtx,
    table: *mut std::ffi::c_void,
}

impl<'c> PointTable<'c> {
    fn raw(&self) -> *mut P2eCtx {
        self.ctx as *const P2eCtx as *mut P2eCtx
    }

    /// `Err`: the call failed, or some key is the neutral element, out of range or off the curve (nothing is built then;
    /// the message names the first such key and its `P2E_WIRE_*` code).
    pub fn new(ctx: &'c P2eCtx, curve: i32, keys: &[(BigUint, BigUint)]) -> Result<Self> {
        let m = keys.len();
        let (px, py) = (pack32(keys.iter().map(|k| k.0.clone()), m), pack32(keys.iter().map(|k| k.1.clone()), m));
        let mut err = vec![0u8; m];
        let mut table = std::ptr::null_mut();
        let rc = unsafe {
            p2e_point_table_create(ctx as *const P2eCtx as *mut P2eCtx, curve, px.as_ptr(), py.as_ptr(), m, err.as_mut_ptr(), &mut table)
        };
        ensure!(rc >= 0, "p2e: {}", unsafe { CStr::from_ptr(p2e_last_error()) }.to_string_lossy());
        let first = err.iter().position(|&e| e != 0);
        ensure!(rc == 0, "{rc} keys rejected, the first at index {first:?} with code {:?}", first.map(|i| err[i]));
        Ok(PointTable { ctx, table })
    }

    pub fn len(&self) -> usize {
        unsafe { p2e_point_table_num_points(self.table) as usize }
    }

    /// `k_i · key[idx_i]` (`p2e_point_table_mul_batch`); `None`: the product is the neutral element.
    pub fn mul(&self, idx: &[u32], scalars: &[BigUint]) -> Result<Vec<Option<(BigUint, BigUint)>>> {
        let n = scalars.len();
        ensure!(idx.len() == n);
        let k = pack32(scalars.iter().cloned(), n);
        let (mut ox, mut oy, mut err) = (vec![0u8; 32 * n], vec![0u8; 32 * n], vec![0u8; n]);
        let rc = unsafe {
            p2e_point_table_mul_batch(self.raw(), self.table, idx.as_ptr(), k.as_ptr(), ox.as_mut_ptr(), oy.as_mut_ptr(), n, err.as_mut_ptr())
        };
        ensure!(rc >= 0, "p2e: {}", unsafe { CStr::from_ptr(p2e_last_error()) }.to_string_lossy());
        (0..n)
            .map(|i| match err[i] {
                P2E_WIRE_OK => Ok(Some((BigUint::from_bytes_le(&ox[32 * i..32 * i + 32]), BigUint::from_bytes_le(&oy[32 * i..32 * i + 32])))),
                P2E_WIRE_INFINITY => Ok(None),
                code => Err(anyhow::anyhow!("element {i}: code {code} (index {} of {} keys)", idx[i], self.len())),
            })
            .collect()
    }

    /// The verdicts of `(msg_i, r_i, s_i)` under `key[idx_i]` (`p2e_ecdsa_verify_table_batch`); a signature with `r` or `s`
    /// outside `[1, n)` is simply invalid here, a bad index is an error.
    pub fn verify(&self, idx: &[u32], sigs: &[(BigUint, BigUint, BigUint)]) -> Result<Vec<bool>> {
        let n = sigs.len();
        ensure!(idx.len() == n);
        let msg = pack32(sigs.iter().map(|g| g.0.clone()), n);
        let (r, s) = (pack32(sigs.iter().map(|g| g.1.clone()), n), pack32(sigs.iter().map(|g| g.2.clone()), n));
        let (mut err, mut valid) = (vec![0u8; n], vec![0u8; n]);
        let rc = unsafe {
            p2e_ecdsa_verify_table_batch(self.raw(), self.table, idx.as_ptr(), msg.as_ptr(), r.as_ptr(), s.as_ptr(), n, err.as_mut_ptr(),
                                         valid.as_mut_ptr())
        };
        ensure!(rc >= 0, "p2e: {}", unsafe { CStr::from_ptr(p2e_last_error()) }.to_string_lossy());
        ensure!(!err.contains(&P2E_WIRE_BAD_INDEX), "a key index is out of range ({} keys)", self.len());
        Ok(valid.iter().map(|&v| v != 0).collect())
    }
}

impl Drop for PointTable<'_> {
    fn drop(&mut self) {
        unsafe { p2e_point_table_destroy(self.raw(), self.table) }
    }
}

/// BIP-340 signatures of `msgs` under `sks` with auxiliary randomness `auxs` (`p2e_schnorr_sign_batch`, host-pointer
/// context); everything is the standard's byte string.  `Err`: the call failed or a key is out of range.
pub fn schnorr_sign(ctx: *mut P2eCtx, msgs: &[[u8; 32]], sks: &[[u8; 32]], auxs: &[[u8; 32]]) -> Result<Vec<[u8; 64]>> {
    let n = msgs.len();
    ensure!(sks.len() == n && auxs.len() == n);
    let (mut sig, mut err) = (vec![[0u8; 64]; n], vec![0u8; n]);
    let rc = unsafe {
        p2e_schnorr_sign_batch(ctx, msgs.as_ptr().cast(), sks.as_ptr().cast(), auxs.as_ptr().cast(), sig.as_mut_ptr().cast(), n, err.as_mut_ptr())
    };
    ensure!(rc >= 0, "p2e: {}", unsafe { CStr::from_ptr(p2e_last_error()) }.to_string_lossy());
    ensure!(rc == 0, "{rc} elements not signed, the first at index {:?}", err.iter().position(|&e| e != 0));
    Ok(sig)
}

/// The BIP-340 verdict of every `(msg, x-only pk, sig)` (`p2e_schnorr_verify_batch`, host-pointer context); a malformed key
/// or signature is simply invalid here.
pub fn schnorr_verify(ctx: *mut P2eCtx, msgs: &[[u8; 32]], pks: &[[u8; 32]], sigs: &[[u8; 64]]) -> Result<Vec<bool>> {
    let n = msgs.len();
    ensure!(pks.len() == n && sigs.len() == n);
    let (mut err, mut valid) = (vec![0u8; n], vec![0u8; n]);
    let rc = unsafe {
        p2e_schnorr_verify_batch(ctx, msgs.as_ptr().cast(), pks.as_ptr().cast(), sigs.as_ptr().cast(), n, err.as_mut_ptr(), valid.as_mut_ptr())
    };
    ensure!(rc >= 0, "p2e: {}", unsafe { CStr::from_ptr(p2e_last_error()) }.to_string_lossy());
    Ok(valid.iter().map(|&v| v != 0).collect())
}

/// One verdict for the whole batch (`p2e_schnorr_verify_aggregate`, host-pointer context).  `seed` must be unpredictable
/// to whoever produced the signatures: fresh randomness, or a hash of every message, key and signature of the batch.
/// `false` does not say which element failed: run `schnorr_verify` then.
pub fn schnorr_verify_aggregate(ctx: *mut P2eCtx, msgs: &[[u8; 32]], pks: &[[u8; 32]], sigs: &[[u8; 64]], seed: &[u8; 32]) -> Result<bool> {
    let n = msgs.len();
    ensure!(pks.len() == n && sigs.len() == n);
    let mut verdict = 0u8;
    let rc = unsafe {
        p2e_schnorr_verify_aggregate(ctx, msgs.as_ptr().cast(), pks.as_ptr().cast(), sigs.as_ptr().cast(), n, seed.as_ptr(),
                                     P2E_MSM_WINDOW_AUTO, &mut verdict, std::ptr::null_mut())
    };
    ensure!(rc >= 0, "p2e: {}", unsafe { CStr::from_ptr(p2e_last_error()) }.to_string_lossy());
    Ok(verdict == 1)
}

/// The scan of one extended public key (`p2e_bip32_ckd_pub_batch` with `n_parents = 1`, then `p2e_key_hash160_batch`,
/// host-pointer context): for every non-hardened `index` the child's point, its chain code (the standard's byte order) and
/// the HASH160 of its compressed key.  `Err(code)` carries the `P2E_WIRE_*` code of the first failed check
/// (`P2E_WIRE_BAD_INDEX` for a hardened index); BIP-32's "proceed with the next index" is the caller's.
#[allow(clippy::type_complexity)]
pub fn xpub_scan(ctx: *mut P2eCtx, key: &(BigUint, BigUint), chain_code: &[u8; 32], indices: &[u32])
                 -> Result<Vec<std::result::Result<((BigUint, BigUint), [u8; 32], [u8; 20]), u8>>> {
    let n = indices.len();
    let (px, py) = (pack32(std::iter::once(key.0.clone()), 1), pack32(std::iter::once(key.1.clone()), 1));
    let (mut x, mut y, mut cc, mut err, mut h) = (vec![0u8; 32 * n], vec![0u8; 32 * n], vec![[0u8; 32]; n], vec![0u8; n], vec![[0u8; 20]; n]);
    let rc = unsafe {
        p2e_bip32_ckd_pub_batch(ctx, px.as_ptr(), py.as_ptr(), chain_code.as_ptr(), 1, indices.as_ptr(), x.as_mut_ptr(), y.as_mut_ptr(),
                                cc.as_mut_ptr().cast(), n, err.as_mut_ptr())
    };
    ensure!(rc >= 0, "p2e: {}", unsafe { CStr::from_ptr(p2e_last_error()) }.to_string_lossy());
    let rc = unsafe { p2e_key_hash160_batch(ctx, P2E_SEC1_COMPRESSED as u32, x.as_ptr(), y.as_ptr(), err.as_ptr(), h.as_mut_ptr().cast(), n) };
    ensure!(rc >= 0, "p2e: {}", unsafe { CStr::from_ptr(p2e_last_error()) }.to_string_lossy());
    let le = |b: &[u8], i: usize| BigUint::from_bytes_le(&b[32 * i..32 * i + 32]);
    Ok((0..n).map(|i| if err[i] != 0 { Err(err[i]) } else { Ok(((le(&x, i), le(&y, i)), cc[i], h[i])) }).collect())
}

/// Hardened or ordinary private children (`p2e_bip32_ckd_priv_batch`, host-pointer context), one parent per index:
/// `(child key, child chain code)` or the `P2E_WIRE_*` code.  The keys are secrets: they are the caller's to wipe.
pub fn ckd_priv(ctx: *mut P2eCtx, parents: &[(BigUint, [u8; 32])], indices: &[u32]) -> Result<Vec<std::result::Result<(BigUint, [u8; 32]), u8>>> {
    let n = indices.len();
    ensure!(parents.len() == n || parents.len() == 1);
    let sk = pack32(parents.iter().map(|p| p.0.clone()), parents.len());
    let pcc: Vec<[u8; 32]> = parents.iter().map(|p| p.1).collect();
    let (mut out, mut cc, mut err) = (vec![0u8; 32 * n], vec![[0u8; 32]; n], vec![0u8; n]);
    let rc = unsafe {
        p2e_bip32_ckd_priv_batch(ctx, sk.as_ptr(), pcc.as_ptr().cast(), parents.len(), indices.as_ptr(), out.as_mut_ptr(),
                                 cc.as_mut_ptr().cast(), n, err.as_mut_ptr())
    };
    ensure!(rc >= 0, "p2e: {}", unsafe { CStr::from_ptr(p2e_last_error()) }.to_string_lossy());
    Ok((0..n).map(|i| if err[i] != 0 { Err(err[i]) } else { Ok((BigUint::from_bytes_le(&out[32 * i..32 * i + 32]), cc[i])) }).collect())
}

/// BIP-341 `taproot_tweak_pubkey` of x-only keys (`p2e_taproot_tweak_pubkey_batch`, host-pointer context) under one Merkle
/// root each, or under no root at all (`roots = None`: BIP-86's key-path-only output): `(output key, parity of its y)` or
/// the `P2E_WIRE_*` code.  All values are the standard's big-endian 32 bytes.
pub fn taproot_output_keys(ctx: *mut P2eCtx, pks: &[[u8; 32]], roots: Option<&[[u8; 32]]>) -> Result<Vec<std::result::Result<([u8; 32], u8), u8>>> {
    let n = pks.len();
    ensure!(roots.map_or(true, |r| r.len() == n));
    let (mut out, mut parity, mut err) = (vec![[0u8; 32]; n], vec![0u8; n], vec![0u8; n]);
    let root_ptr = roots.map_or(std::ptr::null(), |r| r.as_ptr().cast());
    let rc = unsafe {
        p2e_taproot_tweak_pubkey_batch(ctx, pks.as_ptr().cast(), root_ptr, out.as_mut_ptr().cast(), parity.as_mut_ptr(), n, err.as_mut_ptr())
    };
    ensure!(rc >= 0, "p2e: {}", unsafe { CStr::from_ptr(p2e_last_error()) }.to_string_lossy());
    Ok((0..n).map(|i| if err[i] != 0 { Err(err[i]) } else { Ok((out[i], parity[i])) }).collect())
}

/// BIP-341 `taproot_tweak_seckey` (`p2e_taproot_tweak_seckey_batch`, host-pointer context): the keys `schnorr_sign` signs a
/// key-path spend with.  The keys are secrets: they are the caller's to wipe.
pub fn taproot_tweak_secret_keys(ctx: *mut P2eCtx, sks: &[[u8; 32]], roots: Option<&[[u8; 32]]>) -> Result<Vec<std::result::Result<[u8; 32], u8>>> {
    let n = sks.len();
    ensure!(roots.map_or(true, |r| r.len() == n));
    let (mut out, mut err) = (vec![[0u8; 32]; n], vec![0u8; n]);
    let root_ptr = roots.map_or(std::ptr::null(), |r| r.as_ptr().cast());
    let rc = unsafe { p2e_taproot_tweak_seckey_batch(ctx, sks.as_ptr().cast(), root_ptr, out.as_mut_ptr().cast(), n, err.as_mut_ptr()) };
    ensure!(rc >= 0, "p2e: {}", unsafe { CStr::from_ptr(p2e_last_error()) }.to_string_lossy());
    Ok((0..n).map(|i| if err[i] != 0 { Err(err[i]) } else { Ok(out[i]) }).collect())
}

/// BIP-341's script-path rule for a batch of spends (`p2e_taproot_leaf_hash_batch`, then
/// `p2e_taproot_verify_commitment_batch`, host-pointer context): does `output.0` with parity `output.1` commit to the script
/// `leaf.1` of leaf version `leaf.0` under the internal key and the path's nodes?  A malformed element is simply `false`.
pub fn taproot_script_path_commits(ctx: *mut P2eCtx, outputs: &[([u8; 32], u8)], internal: &[[u8; 32]], leaves: &[(u8, &[u8])],
                                   paths: &[Vec<[u8; 32]>]) -> Result<Vec<bool>> {
    let n = outputs.len();
    ensure!(internal.len() == n && leaves.len() == n && paths.len() == n);
    let max_depth = paths.iter().map(|p| p.len()).max().unwrap_or(0);
    ensure!(max_depth <= 128, "a control block holds at most 128 nodes");
    let (mut versions, mut script, mut offsets) = (Vec::with_capacity(n), Vec::new(), vec![0u64]);
    for (v, s) in leaves {
        versions.push(*v);
        script.extend_from_slice(s);
        offsets.push(script.len() as u64);
    }
    script.resize((script.len() + 3) / 4 * 4 + 4, 0);     // the library reads aligned 4-byte words
    let (mut leaf, mut leaf_err) = (vec![[0u8; 32]; n], vec![0u8; n]);
    let rc = unsafe {
        p2e_taproot_leaf_hash_batch(ctx, versions.as_ptr(), script.as_ptr(), offsets.as_ptr(), leaf.as_mut_ptr().cast(), n, leaf_err.as_mut_ptr())
    };
    ensure!(rc >= 0, "p2e: {}", unsafe { CStr::from_ptr(p2e_last_error()) }.to_string_lossy());
    let mut nodes = vec![[0u8; 32]; n * max_depth];
    let mut depth = Vec::with_capacity(n);
    for (i, p) in paths.iter().enumerate() {
        nodes[i * max_depth..i * max_depth + p.len()].copy_from_slice(p);
        depth.push(p.len() as u8);
    }
    let (out_pk, out_parity): (Vec<[u8; 32]>, Vec<u8>) = outputs.iter().cloned().unzip();
    let (mut err, mut valid) = (vec![0u8; n], vec![0u8; n]);
    let path_ptr = if max_depth == 0 { std::ptr::null() } else { nodes.as_ptr().cast() };
    let rc = unsafe {
        p2e_taproot_verify_commitment_batch(ctx, out_pk.as_ptr().cast(), out_parity.as_ptr(), internal.as_ptr().cast(), leaf.as_ptr().cast(),
                                            path_ptr, depth.as_ptr(), max_depth, n, err.as_mut_ptr(), valid.as_mut_ptr())
    };
    ensure!(rc >= 0, "p2e: {}", unsafe { CStr::from_ptr(p2e_last_error()) }.to_string_lossy());
    Ok((0..n).map(|i| leaf_err[i] == 0 && valid[i] == 1).collect())
}

/// One hit of a silent-payment scan: the output's index within its transaction, 0 for an unlabelled hit or `j + 1` for label
/// `j`, and the big-endian tweak `t_k` (the spending key is `b_spend + t_k (+ l_j)`).
pub type SpHit = (u32, u8, [u8; 32]);

/// BIP-352 input hashes (`p2e_sp_input_hash_batch`, host-pointer context): `H_Inputs(outpoint || serP(A))` as big-endian
/// 32 bytes for each smallest outpoint (36 bytes as serialised) and summed input key `A` (little-endian), or the code.
pub fn sp_input_hashes(ctx: *mut P2eCtx, outpoints: &[[u8; 36]], inputs: &[([u8; 32], [u8; 32])]) -> Result<Vec<std::result::Result<[u8; 32], u8>>> {
    let n = outpoints.len();
    ensure!(inputs.len() == n);
    let (ax, ay): (Vec<[u8; 32]>, Vec<[u8; 32]>) = inputs.iter().cloned().unzip();
    let (mut out, mut err) = (vec![[0u8; 32]; n], vec![0u8; n]);
    let rc = unsafe {
        p2e_sp_input_hash_batch(ctx, outpoints.as_ptr().cast(), ax.as_ptr().cast(), ay.as_ptr().cast(), out.as_mut_ptr().cast(), n, err.as_mut_ptr())
    };
    ensure!(rc >= 0, "p2e: {}", unsafe { CStr::from_ptr(p2e_last_error()) }.to_string_lossy());
    Ok((0..n).map(|i| if err[i] != 0 { Err(err[i]) } else { Ok(out[i]) }).collect())
}

/// BIP-352 labels of one scan key (`p2e_sp_label_batch`, host-pointer context): `(l_m big-endian, (x, y) of l_m G
/// little-endian)` for each index `m`, or the code.  `scan_sk` is a secret: it is the caller's to wipe.
pub fn sp_labels(ctx: *mut P2eCtx, scan_sk: &[u8; 32], indices: &[u32]) -> Result<Vec<std::result::Result<([u8; 32], ([u8; 32], [u8; 32])), u8>>> {
    let n = indices.len();
    let (mut tweak, mut x, mut y, mut err) = (vec![[0u8; 32]; n], vec![[0u8; 32]; n], vec![[0u8; 32]; n], vec![0u8; n]);
    let rc = unsafe {
        p2e_sp_label_batch(ctx, scan_sk.as_ptr(), indices.as_ptr(), tweak.as_mut_ptr().cast(), x.as_mut_ptr().cast(), y.as_mut_ptr().cast(), n,
                           err.as_mut_ptr())
    };
    ensure!(rc >= 0, "p2e: {}", unsafe { CStr::from_ptr(p2e_last_error()) }.to_string_lossy());
    Ok((0..n).map(|i| if err[i] != 0 { Err(err[i]) } else { Ok((tweak[i], (x[i], y[i]))) }).collect())
}

/// BIP-352 output keys of a sender (`p2e_sp_send_batch`, host-pointer context): `x(B_spend + t_k G)` with `t_k` from
/// `(input_hash a) B_scan` and `k`, or the `P2E_WIRE_*` code.  Keys and points are little-endian, `input_hash` and the result
/// the standard's big-endian 32 bytes.  `a` is a secret: it is the caller's to wipe.
pub fn sp_output_keys(ctx: *mut P2eCtx, a: &[[u8; 32]], input_hash: &[[u8; 32]], scan_pk: &[([u8; 32], [u8; 32])],
                      spend_pk: &[([u8; 32], [u8; 32])], k: &[u32]) -> Result<Vec<std::result::Result<[u8; 32], u8>>> {
    let n = a.len();
    ensure!(input_hash.len() == n && scan_pk.len() == n && spend_pk.len() == n && k.len() == n);
    let (scx, scy): (Vec<[u8; 32]>, Vec<[u8; 32]>) = scan_pk.iter().cloned().unzip();
    let (spx, spy): (Vec<[u8; 32]>, Vec<[u8; 32]>) = spend_pk.iter().cloned().unzip();
    let (mut out, mut err) = (vec![[0u8; 32]; n], vec![0u8; n]);
    let rc = unsafe {
        p2e_sp_send_batch(ctx, a.as_ptr().cast(), input_hash.as_ptr().cast(), scx.as_ptr().cast(), scy.as_ptr().cast(), spx.as_ptr().cast(),
                          spy.as_ptr().cast(), k.as_ptr(), out.as_mut_ptr().cast(), n, err.as_mut_ptr())
    };
    ensure!(rc >= 0, "p2e: {}", unsafe { CStr::from_ptr(p2e_last_error()) }.to_string_lossy());
    Ok((0..n).map(|i| if err[i] != 0 { Err(err[i]) } else { Ok(out[i]) }).collect())
}

/// BIP-352 scan of a batch of transactions under one scan key, one spend key and up to 16 labels (`p2e_sp_input_hash_batch`
/// is the caller's, or the index's: `input_hash = None` takes `inputs` as tweak data).  Transaction `i` is the input point
/// `inputs[i]` and the x-only outputs `outputs[i]`; the result is its hits, at most `max_hits` (1 .. 8), or the
/// `P2E_WIRE_*` code.  `scan_sk` is a secret: it is the caller's to wipe.
pub fn sp_scan(ctx: *mut P2eCtx, scan_sk: &[u8; 32], spend_pk: &([u8; 32], [u8; 32]), labels: &[([u8; 32], [u8; 32])],
               inputs: &[([u8; 32], [u8; 32])], input_hash: Option<&[[u8; 32]]>, outputs: &[Vec<[u8; 32]>], max_hits: usize)
               -> Result<Vec<std::result::Result<Vec<SpHit>, u8>>> {
    let n = inputs.len();
    ensure!(outputs.len() == n && input_hash.map_or(true, |h| h.len() == n));
    ensure!((1..=8).contains(&max_hits) && labels.len() <= 16, "at most 8 hits per transaction and 16 labels");
    let (lx, ly): (Vec<[u8; 32]>, Vec<[u8; 32]>) = labels.iter().cloned().unzip();
    let (ax, ay): (Vec<[u8; 32]>, Vec<[u8; 32]>) = inputs.iter().cloned().unzip();
    let (mut flat, mut offsets) = (Vec::new(), vec![0u64]);
    for o in outputs {
        flat.extend_from_slice(o);
        offsets.push(flat.len() as u64);
    }
    flat.push([0u8; 32]); // never read: keeps the pointer of a batch without outputs valid
    let (mut n_hits, mut err) = (vec![0u8; n], vec![0u8; n]);
    let (mut hit_output, mut hit_label, mut hit_tweak) = (vec![0u32; n * max_hits], vec![0u8; n * max_hits], vec![[0u8; 32]; n * max_hits]);
    let label_ptr = |v: &Vec<[u8; 32]>| -> *const u8 { if labels.is_empty() { std::ptr::null() } else { v.as_ptr().cast() } };
    let hash_ptr: *const u8 = input_hash.map_or(std::ptr::null(), |h| h.as_ptr().cast());
    let rc = unsafe {
        p2e_sp_scan_batch(ctx, scan_sk.as_ptr(), spend_pk.0.as_ptr(), spend_pk.1.as_ptr(), label_ptr(&lx), label_ptr(&ly), labels.len(),
                          ax.as_ptr().cast(), ay.as_ptr().cast(), hash_ptr, flat.as_ptr().cast(), offsets.as_ptr(), max_hits,
                          n_hits.as_mut_ptr(), hit_output.as_mut_ptr(), hit_label.as_mut_ptr(), hit_tweak.as_mut_ptr().cast(), n,
                          err.as_mut_ptr())
    };
    ensure!(rc >= 0, "p2e: {}", unsafe { CStr::from_ptr(p2e_last_error()) }.to_string_lossy());
    Ok((0..n).map(|i| {
        if err[i] != 0 {
            return Err(err[i]);
        }
        Ok((0..n_hits[i] as usize).map(|h| (hit_output[max_hits * i + h], hit_label[max_hits * i + h], hit_tweak[max_hits * i + h])).collect())
    }).collect())
}

/// The `keyagg192` record of a MuSig2 session (include/p2e.h): the aggregate key with its tweak accumulators.
pub type MusigKeyAgg = [u8; 192];
/// The `session128` record of a MuSig2 session: `b`, `e`, `xbytes(R)` and the parity of `y(R)`.
pub type MusigSession = [u8; 128];
/// A public or an aggregate nonce: `x(R_1) || y(R_1) || x(R_2) || y(R_2)`, little-endian.
pub type MusigNonce = [u8; 128];

/// `key_offsets` of per-session lists: the flattened items and the `count + 1` offsets, in items.
fn musig_flatten<T: Clone>(lists: &[Vec<T>], pad: T) -> (Vec<T>, Vec<u64>) {
    let (mut flat, mut offsets) = (Vec::new(), vec![0u64]);
    for l in lists {
        flat.extend_from_slice(l);
        offsets.push(flat.len() as u64);
    }
    flat.push(pad); // never read: keeps the pointer of a batch without signers valid
    (flat, offsets)
}

/// BIP-327 KeyAgg (`p2e_musig_key_agg_batch`, host-pointer context): per session the record and the big-endian x-only
/// aggregate key of its public keys (little-endian `(x, y)`), or the `P2E_WIRE_*` code.
pub fn musig_key_agg(ctx: *mut P2eCtx, keys: &[Vec<([u8; 32], [u8; 32])>]) -> Result<Vec<std::result::Result<(MusigKeyAgg, [u8; 32]), u8>>> {
    let n = keys.len();
    let (flat, offsets) = musig_flatten(keys, ([0u8; 32], [0u8; 32]));
    let (x, y): (Vec<[u8; 32]>, Vec<[u8; 32]>) = flat.into_iter().unzip();
    let (mut rec, mut pk, mut err) = (vec![[0u8; 192]; n], vec![[0u8; 32]; n], vec![0u8; n]);
    let rc = unsafe {
        p2e_musig_key_agg_batch(ctx, x.as_ptr().cast(), y.as_ptr().cast(), offsets.as_ptr(), rec.as_mut_ptr().cast(), pk.as_mut_ptr().cast(), n,
                                err.as_mut_ptr())
    };
    ensure!(rc >= 0, "p2e: {}", unsafe { CStr::from_ptr(p2e_last_error()) }.to_string_lossy());
    Ok((0..n).map(|i| if err[i] != 0 { Err(err[i]) } else { Ok((rec[i], pk[i])) }).collect())
}

/// BIP-327 ApplyTweak (`p2e_musig_apply_tweak_batch`): `mode` is `P2E_MUSIG_TWEAK_PLAIN` (0), `_XONLY` (1) or `_TAPROOT` (2, where
/// `tweaks` are Merkle roots, or `None` for BIP-86's key-path-only output).  Per session the new record and x-only key, or the code.
pub fn musig_apply_tweak(ctx: *mut P2eCtx, records: &[MusigKeyAgg], tweaks: Option<&[[u8; 32]]>, mode: i32)
                         -> Result<Vec<std::result::Result<(MusigKeyAgg, [u8; 32]), u8>>> {
    let n = records.len();
    ensure!(tweaks.map_or(mode == 2, |t| t.len() == n), "one tweak per session (none only in the Taproot mode)");
    let tweak_ptr: *const u8 = tweaks.map_or(std::ptr::null(), |t| t.as_ptr().cast());
    let (mut rec, mut pk, mut err) = (vec![[0u8; 192]; n], vec![[0u8; 32]; n], vec![0u8; n]);
    let rc = unsafe {
        p2e_musig_apply_tweak_batch(ctx, records.as_ptr().cast(), tweak_ptr, mode, rec.as_mut_ptr().cast(), pk.as_mut_ptr().cast(), n, err.as_mut_ptr())
    };
    ensure!(rc >= 0, "p2e: {}", unsafe { CStr::from_ptr(p2e_last_error()) }.to_string_lossy());
    Ok((0..n).map(|i| if err[i] != 0 { Err(err[i]) } else { Ok((rec[i], pk[i])) }).collect())
}

/// BIP-327 NonceAgg (`p2e_musig_nonce_agg_batch`): per session the sum of its signers' public nonces, or the code.
pub fn musig_nonce_agg(ctx: *mut P2eCtx, nonces: &[Vec<MusigNonce>]) -> Result<Vec<std::result::Result<MusigNonce, u8>>> {
    let n = nonces.len();
    let (flat, offsets) = musig_flatten(nonces, [0u8; 128]);
    let (mut agg, mut err) = (vec![[0u8; 128]; n], vec![0u8; n]);
    let rc = unsafe { p2e_musig_nonce_agg_batch(ctx, flat.as_ptr().cast(), offsets.as_ptr(), agg.as_mut_ptr().cast(), n, err.as_mut_ptr()) };
    ensure!(rc >= 0, "p2e: {}", unsafe { CStr::from_ptr(p2e_last_error()) }.to_string_lossy());
    Ok((0..n).map(|i| if err[i] != 0 { Err(err[i]) } else { Ok(agg[i]) }).collect())
}

/// The session values of BIP-327 (`p2e_musig_session_batch`): per session the record of `b`, `e` and `R`, or the code.
pub fn musig_sessions(ctx: *mut P2eCtx, records: &[MusigKeyAgg], aggnonces: &[MusigNonce], msgs: &[[u8; 32]])
                      -> Result<Vec<std::result::Result<MusigSession, u8>>> {
    let n = records.len();
    ensure!(aggnonces.len() == n && msgs.len() == n);
    let (mut ses, mut err) = (vec![[0u8; 128]; n], vec![0u8; n]);
    let rc = unsafe {
        p2e_musig_session_batch(ctx, records.as_ptr().cast(), aggnonces.as_ptr().cast(), msgs.as_ptr().cast(), ses.as_mut_ptr().cast(), n,
                                err.as_mut_ptr())
    };
    ensure!(rc >= 0, "p2e: {}", unsafe { CStr::from_ptr(p2e_last_error()) }.to_string_lossy());
    Ok((0..n).map(|i| if err[i] != 0 { Err(err[i]) } else { Ok(ses[i]) }).collect())
}

/// The caller's partial signatures (`p2e_musig_partial_sign_batch`), one per session: `secnonces[i] = k_1 || k_2` and `sk[i]`
/// little-endian.  A secret nonce must never be used twice; both are secrets and the caller's to wipe.  Check the result with
/// [`musig_partial_verify`]: the library cannot know whether the key is in the session's list.
pub fn musig_partial_sign(ctx: *mut P2eCtx, secnonces: &[[u8; 64]], sk: &[[u8; 32]], records: &[MusigKeyAgg], sessions: &[MusigSession])
                          -> Result<Vec<std::result::Result<[u8; 32], u8>>> {
    let n = sk.len();
    ensure!(secnonces.len() == n && records.len() == n && sessions.len() == n);
    let (mut psig, mut err) = (vec![[0u8; 32]; n], vec![0u8; n]);
    let rc = unsafe {
        p2e_musig_partial_sign_batch(ctx, secnonces.as_ptr().cast(), sk.as_ptr().cast(), records.as_ptr().cast(), sessions.as_ptr().cast(),
                                     psig.as_mut_ptr().cast(), n, err.as_mut_ptr())
    };
    ensure!(rc >= 0, "p2e: {}", unsafe { CStr::from_ptr(p2e_last_error()) }.to_string_lossy());
    Ok((0..n).map(|i| if err[i] != 0 { Err(err[i]) } else { Ok(psig[i]) }).collect())
}

/// BIP-327 PartialSigVerify (`p2e_musig_partial_verify_batch`): partial signature `i` of the signer with the public nonce
/// `pubnonces[i]` and the key `keys[i]`, in session `index[i]` of the records.  `Ok(valid)`, or the code.
pub fn musig_partial_verify(ctx: *mut P2eCtx, psigs: &[[u8; 32]], pubnonces: &[MusigNonce], keys: &[([u8; 32], [u8; 32])], index: &[u32],
                            records: &[MusigKeyAgg], sessions: &[MusigSession]) -> Result<Vec<std::result::Result<bool, u8>>> {
    let n = psigs.len();
    ensure!(pubnonces.len() == n && keys.len() == n && index.len() == n && records.len() == sessions.len() && !records.is_empty());
    let (x, y): (Vec<[u8; 32]>, Vec<[u8; 32]>) = keys.iter().cloned().unzip();
    let (mut err, mut valid) = (vec![0u8; n], vec![0u8; n]);
    let rc = unsafe {
        p2e_musig_partial_verify_batch(ctx, psigs.as_ptr().cast(), pubnonces.as_ptr().cast(), x.as_ptr().cast(), y.as_ptr().cast(), index.as_ptr(),
                                       records.as_ptr().cast(), sessions.as_ptr().cast(), records.len(), n, err.as_mut_ptr(), valid.as_mut_ptr())
    };
    ensure!(rc >= 0, "p2e: {}", unsafe { CStr::from_ptr(p2e_last_error()) }.to_string_lossy());
    Ok((0..n).map(|i| if err[i] != 0 { Err(err[i]) } else { Ok(valid[i] == 1) }).collect())
}

/// BIP-327 PartialSigAgg (`p2e_musig_sig_agg_batch`): per session the BIP-340 signature made of its partial signatures, or
/// the code.  `schnorr_verify` accepts it under the session's x-only aggregate key.
pub fn musig_sig_agg(ctx: *mut P2eCtx, psigs: &[Vec<[u8; 32]>], records: &[MusigKeyAgg], sessions: &[MusigSession])
                     -> Result<Vec<std::result::Result<[u8; 64], u8>>> {
    let n = psigs.len();
    ensure!(records.len() == n && sessions.len() == n);
    let (flat, offsets) = musig_flatten(psigs, [0u8; 32]);
    let (mut sig, mut err) = (vec![[0u8; 64]; n], vec![0u8; n]);
    let rc = unsafe {
        p2e_musig_sig_agg_batch(ctx, flat.as_ptr().cast(), offsets.as_ptr(), records.as_ptr().cast(), sessions.as_ptr().cast(),
                                sig.as_mut_ptr().cast(), n, err.as_mut_ptr())
    };
    ensure!(rc >= 0, "p2e: {}", unsafe { CStr::from_ptr(p2e_last_error()) }.to_string_lossy());
    Ok((0..n).map(|i| if err[i] != 0 { Err(err[i]) } else { Ok(sig[i]) }).collect())
}

/// Hashes of a batch of byte strings as message scalars (`p2e_hash_batch` with `P2E_DIGEST_SCALAR`, host-pointer context):
/// the digest read as a big-endian integer, which is what `sign_messages*` and `recover_public_keys` take as `msg`.
/// `alg` is `P2E_HASH_SHA256`, `P2E_HASH_SHA256D` or `P2E_HASH_KECCAK256` (Ethereum's Keccak, not SHA3-256).
pub fn hash_messages(ctx: *mut P2eCtx, alg: i32, messages: &[&[u8]]) -> Result<Vec<BigUint>> {
    let n = messages.len();
    let mut offsets = Vec::with_capacity(n + 1);
    let mut data = Vec::new();
    offsets.push(0u64);
    for m in messages {
        data.extend_from_slice(m);
        offsets.push(data.len() as u64);
    }
    data.push(0); // never read: keeps the pointer of an all-empty batch valid
    let mut out = vec![0u8; 32 * n];
    let rc = unsafe { p2e_hash_batch(ctx, alg, P2E_DIGEST_SCALAR, data.as_ptr(), offsets.as_ptr(), out.as_mut_ptr(), n) };
    ensure!(rc >= 0, "p2e: {}", unsafe { CStr::from_ptr(p2e_last_error()) }.to_string_lossy());
    Ok((0..n).map(|i| BigUint::from_bytes_le(&out[32 * i..32 * i + 32])).collect())
}

/// `sign_messages_recoverable` with the nonces of RFC 6979 (`p2e_ecdsa_sign_deterministic_batch`) instead of the
/// `rand()` of curve/ecdsa.rs:29-32: the same `(msg, sk)` always gives the same `(r, s, v)`.
pub fn sign_messages_deterministic(ctx: *mut P2eCtx, curve: i32, msgs: &[BigUint], sks: &[BigUint]) -> Result<Vec<(BigUint, BigUint, u8)>> {
    let n = msgs.len();
    ensure!(sks.len() == n);
    let (msg, sk) = (pack32(msgs.iter().cloned(), n), pack32(sks.iter().cloned(), n));
    let (mut r, mut s, mut v, mut err) = (vec![0u8; 32 * n], vec![0u8; 32 * n], vec![0u8; n], vec![0u8; n]);
    let rc = unsafe {
        p2e_ecdsa_sign_deterministic_batch(ctx, curve, P2E_SIGN_PLAN_AUTO, msg.as_ptr(), sk.as_ptr(), r.as_mut_ptr(), s.as_mut_ptr(),
                                           v.as_mut_ptr(), n, err.as_mut_ptr())
    };
    ensure!(rc >= 0, "p2e: {}", unsafe { CStr::from_ptr(p2e_last_error()) }.to_string_lossy());
    (0..n)
        .map(|i| {
            ensure!(err[i] == 0, "signature {i}: error bits {:#x}", err[i]);
            Ok((BigUint::from_bytes_le(&r[32 * i..32 * i + 32]), BigUint::from_bytes_le(&s[32 * i..32 * i + 32]), v[i]))
        })
        .collect()
}

/// Ethereum addresses of recovered keys (`p2e_eth_address_batch`): `None` stays `None`, never the address of a zero key.
pub fn eth_addresses(ctx: *mut P2eCtx, keys: &[Option<(BigUint, BigUint)>]) -> Result<Vec<Option<[u8; 20]>>> {
    let n = keys.len();
    let zero = (BigUint::default(), BigUint::default());
    let pkx = pack32(keys.iter().map(|k| k.as_ref().unwrap_or(&zero).0.clone()), n);
    let pky = pack32(keys.iter().map(|k| k.as_ref().unwrap_or(&zero).1.clone()), n);
    let err: Vec<u8> = keys.iter().map(|k| k.is_none() as u8).collect();
    let mut addr = vec![0u8; 20 * n];
    let rc = unsafe { p2e_eth_address_batch(ctx, pkx.as_ptr(), pky.as_ptr(), err.as_ptr(), addr.as_mut_ptr(), n) };
    ensure!(rc >= 0, "p2e: {}", unsafe { CStr::from_ptr(p2e_last_error()) }.to_string_lossy());
    Ok((0..n).map(|i| keys[i].as_ref().map(|_| addr[20 * i..20 * i + 20].try_into().unwrap())).collect())
}

/// SEC1 public keys as they arrive on the wire (33-byte compressed, 65-byte uncompressed) to coordinates
/// (`p2e_point_decode_batch`, host-pointer context): `Err(code)` carries the `P2E_WIRE_*` code of the first failed check.
pub fn decode_public_keys(ctx: *mut P2eCtx, curve: i32, keys: &[&[u8]]) -> Result<Vec<std::result::Result<(BigUint, BigUint), u8>>> {
    let n = keys.len();
    let (mut offsets, mut data) = (vec![0u64], Vec::new());
    for k in keys {
        data.extend_from_slice(k);
        offsets.push(data.len() as u64);
    }
    data.push(0); // never read: keeps the pointer of an all-empty batch valid
    let (mut px, mut py, mut err) = (vec![0u8; 32 * n], vec![0u8; 32 * n], vec![0u8; n]);
    let rc = unsafe { p2e_point_decode_batch(ctx, curve, data.as_ptr(), offsets.as_ptr(), px.as_mut_ptr(), py.as_mut_ptr(), n, err.as_mut_ptr()) };
    ensure!(rc >= 0, "p2e: {}", unsafe { CStr::from_ptr(p2e_last_error()) }.to_string_lossy());
    Ok((0..n)
        .map(|i| match err[i] {
            P2E_WIRE_OK => Ok((BigUint::from_bytes_le(&px[32 * i..32 * i + 32]), BigUint::from_bytes_le(&py[32 * i..32 * i + 32]))),
            code => Err(code),
        })
        .collect())
}

/// Strict-DER signatures (BIP-66's rules) to `(r, s)` (`p2e_sig_decode_batch`, `P2E_SIG_DER`); `flags` is 0,
/// `P2E_SIG_REQUIRE_LOW_S` or `P2E_SIG_NORMALIZE_S`.  `Err(code)` as in `decode_public_keys`.
pub fn decode_der_signatures(ctx: *mut P2eCtx, curve: i32, flags: u32, sigs: &[&[u8]]) -> Result<Vec<std::result::Result<(BigUint, BigUint), u8>>> {
    let n = sigs.len();
    let (mut offsets, mut data) = (vec![0u64], Vec::new());
    for s in sigs {
        data.extend_from_slice(s);
        offsets.push(data.len() as u64);
    }
    data.push(0);
    let (mut r, mut s, mut err) = (vec![0u8; 32 * n], vec![0u8; 32 * n], vec![0u8; n]);
    let rc = unsafe {
        p2e_sig_decode_batch(ctx, curve, P2E_SIG_DER, flags, data.as_ptr(), offsets.as_ptr(), r.as_mut_ptr(), s.as_mut_ptr(),
                             std::ptr::null_mut(), n, err.as_mut_ptr())
    };
    ensure!(rc >= 0, "p2e: {}", unsafe { CStr::from_ptr(p2e_last_error()) }.to_string_lossy());
    Ok((0..n)
        .map(|i| match err[i] {
            P2E_WIRE_OK => Ok((BigUint::from_bytes_le(&r[32 * i..32 * i + 32]), BigUint::from_bytes_le(&s[32 * i..32 * i + 32]))),
            code => Err(code),
        })
        .collect())
}

/// Keys and signatures leaving the library: compressed SEC1 keys (`p2e_point_encode_batch`) and minimal DER signatures with
/// a low s (`p2e_sig_encode_batch`, `P2E_SIG_NORMALIZE_S`).  Any flagged element is an error here.
pub fn encode_keys_and_signatures(ctx: *mut P2eCtx, curve: i32, keys: &[(BigUint, BigUint)], sigs: &[(BigUint, BigUint)]) -> Result<(Vec<[u8; 33]>, Vec<Vec<u8>>)> {
    let (nk, ns) = (keys.len(), sigs.len());
    let (px, py) = (pack32(keys.iter().map(|k| k.0.clone()), nk), pack32(keys.iter().map(|k| k.1.clone()), nk));
    let (r, s) = (pack32(sigs.iter().map(|g| g.0.clone()), ns), pack32(sigs.iter().map(|g| g.1.clone()), ns));
    let (mut kout, mut kerr) = (vec![0u8; 33 * nk], vec![0u8; nk]);
    let (mut sout, mut slen, mut serr) = (vec![0u8; P2E_SIG_DER_STRIDE * ns], vec![0u8; ns], vec![0u8; ns]);
    let rc = unsafe { p2e_point_encode_batch(ctx, curve, P2E_SEC1_COMPRESSED, px.as_ptr(), py.as_ptr(), kout.as_mut_ptr(), nk, kerr.as_mut_ptr()) };
    ensure!(rc >= 0, "p2e: {}", unsafe { CStr::from_ptr(p2e_last_error()) }.to_string_lossy());
    ensure!(rc == 0, "{rc} keys have no SEC1 form, the first at index {:?}", kerr.iter().position(|&e| e != 0));
    let rc = unsafe {
        p2e_sig_encode_batch(ctx, curve, P2E_SIG_DER, P2E_SIG_NORMALIZE_S, r.as_ptr(), s.as_ptr(), std::ptr::null(), sout.as_mut_ptr(),
                             slen.as_mut_ptr(), ns, serr.as_mut_ptr())
    };
    ensure!(rc >= 0, "p2e: {}", unsafe { CStr::from_ptr(p2e_last_error()) }.to_string_lossy());
    ensure!(rc == 0, "{rc} signatures are out of range, the first at index {:?}", serr.iter().position(|&e| e != 0));
    Ok(((0..nk).map(|i| kout[33 * i..33 * i + 33].try_into().unwrap()).collect(),
        (0..ns).map(|i| sout[P2E_SIG_DER_STRIDE * i..P2E_SIG_DER_STRIDE * i + slen[i] as usize].to_vec()).collect()))
}

/// One built circuit of `verify_p256_message_circuit` (gadgets/ecdsa.rs:55-78): its hot-path output targets in
/// registration order (len == 115 557 = `p2e_curve_program_num_cols`) and the library's program object, which carries
/// the point `precompute_window` drew with `rand()` while THIS circuit was built (gadgets/curve_windowed_mul.rs:57).
pub struct P256Binding {
    pub targets: Vec<Target>,
    pub program: *mut P2eCurveProgram,
}

/// `blind` = that point (the builder wrapper kept it).  Call once per built circuit; free with
/// `p2e_curve_program_destroy`.
pub fn bind_p256_verifier(ctx: *mut P2eCtx, targets: Vec<Target>, blind_x: &BigUint, blind_y: &BigUint) -> Result<P256Binding> {
    let (bx, by) = (pack32(std::iter::once(blind_x.clone()), 1), pack32(std::iter::once(blind_y.clone()), 1));
    let mut program = std::ptr::null_mut();
    let rc = unsafe { p2e_curve_program_create(ctx, P2E_CP_VERIFY, P2E_CURVE_P256, bx.as_ptr(), by.as_ptr(), &mut program) };
    ensure!(rc == 0, "p2e: {}", unsafe { CStr::from_ptr(p2e_last_error()) }.to_string_lossy());
    ensure!(targets.len() as i64 == unsafe { p2e_curve_program_num_cols(program) });
    Ok(P256Binding { targets, program })
}

/// The P-256 counterpart of `fill_partial_witnesses` (same pre-seeding, same error mapping).
pub fn fill_partial_witnesses_p256<F: RichField>(
    binding: &P256Binding,
    ctx: *mut P2eCtx,
    sigs: &[VerifyInput],
    pws: &mut [PartialWitness<F>],
) -> Result<()> {
    let n = sigs.len();
    let ncols = binding.targets.len();
    ensure!(pws.len() == n);
    let msg = pack32(sigs.iter().map(|s| s.msg.clone()), n);
    let r = pack32(sigs.iter().map(|s| s.r.clone()), n);
    let s = pack32(sigs.iter().map(|s| s.s.clone()), n);
    let px = pack32(sigs.iter().map(|s| s.pk_x.clone()), n);
    let py = pack32(sigs.iter().map(|s| s.pk_y.clone()), n);
    let mut cols = vec![0u64; ncols * n];
    let (mut err, mut valid) = (vec![0u8; n], vec![0u8; n]);
    let rc = unsafe {
        p2e_p256_verify_witness_batch(ctx, binding.program, msg.as_ptr(), r.as_ptr(), s.as_ptr(), px.as_ptr(), py.as_ptr(),
                                      cols.as_mut_ptr(), n, n, err.as_mut_ptr(), valid.as_mut_ptr())
    };
    ensure!(rc >= 0, "p2e: {}", unsafe { CStr::from_ptr(p2e_last_error()) }.to_string_lossy());
    for i in 0..n {
        ensure!(err[i] == 0, "signature {i}: witness generation error bits {:#x}", err[i]);
        for (c, t) in binding.targets.iter().enumerate() {
            pws[i].set_target(*t, F::from_canonical_u64(cols[c * n + i]))?;
        }
    }
    Ok(())
}
