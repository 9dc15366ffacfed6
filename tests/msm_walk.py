"""A curve-generic restatement of curve_msm_circuit (gadgets/curve_msm.rs:21-79) for the MSM and fixed-base curve programs.

oracle/p2e_ref.py's Walker.curve_msm is tied to secp256k1 (its blinding point is rando_point(), and the unblinding
constant is doubled with the secp256k1 helpers); this subclass takes both from the walker's curve.  Everything else --
the generators, the split, the random access, the conditional adds -- is the oracle's own.  Walker.fixed_base_curve_mul
is already curve-generic and is used as it is.

Also the per-element helpers the tests run in worker processes (spawned: no GPU state is inherited)."""
import p2e_ref as R

NL = R.NL
MSM_COLS, MSM_GENS, MSM_AUX = 112309, 4694, 8382
FB_COLS, FB_GENS, FB_AUX = 16797, 802, 4221


class CurveWalker(R.Walker):
    def curve_msm(self, p, q, n, m):
        C = self.curve
        limbs_n = self.split_2(n)
        limbs_m = self.split_2(m)
        assert len(limbs_n) == len(limbs_m)
        num = len(limbs_n)
        rando = C.hash_point(32)                                 # KeccakHash::<32>(F::ZERO) * G of THIS curve (:33-39)
        rando_t = R.const_point(rando)
        neg_rando = R.const_point(C.neg(rando))
        pre = [p] * 16
        cur_p, cur_q = rando_t, rando_t
        with self.scope("table"):
            for i in range(4):
                pre[i] = cur_p
                pre[4 * i] = cur_q
                cur_p = self.curve_add(cur_p, p)
                cur_q = self.curve_add(cur_q, q)
            for i in range(1, 4):
                pre[i] = self.curve_add(pre[i], neg_rando)
                pre[4 * i] = self.curve_add(pre[4 * i], neg_rando)
            for i in range(1, 4):
                for j in range(1, 4):
                    pre[i + 4 * j] = self.curve_add(pre[i], pre[4 * j])
        result = rando_t
        for d in reversed(range(num)):                          # MSB first
            with self.scope(f"digit{d}"):
                result = self.curve_repeated_double(result, 2)
                idx = 4 * limbs_m[d] + limbs_n[d]               # mul_add(four, limb_m, limb_n)
                self._aux("index", [idx])
                r = self.random_access_point(idx, pre)
                should_add = self.not_(self.is_equal_zero(idx))
                result = self.curve_conditional_add(result, r, should_add)
        spm = rando
        for _ in range(2 * num):
            spm = C.double(spm)
        with self.scope("unblind"):
            return self.curve_add(result, R.const_point(C.neg(spm)))


def msm_witness(curve, px, py, qx, qy, n, m):
    """(cols, aux, ops, aux_ops, result point) of curve_msm_circuit(p, q, n, m) with full 9-limb scalars; raises
    R.RefPanic where the reference panics (an inverse of zero)"""
    w = CurveWalker(curve)
    pt = w.curve_msm((R.limbs_of(px, NL), R.limbs_of(py, NL)), (R.limbs_of(qx, NL), R.limbs_of(qy, NL)), R.limbs_of(n, NL),
                     R.limbs_of(m, NL))
    return w.cols, w.aux, w.ops, w.aux_ops, (R.value_of(pt[0]), R.value_of(pt[1]))


def fixed_base_witness(curve, base, k):
    """(cols, aux, ops, aux_ops, result point) of fixed_base_curve_mul_circuit(base, k)"""
    w = R.Walker(curve)
    pt = w.fixed_base_curve_mul(base, R.limbs_of(k, NL))
    return w.cols, w.aux, w.ops, w.aux_ops, (R.value_of(pt[0]), R.value_of(pt[1]))


def msm_job(args):
    """worker: (cols, aux) of one MSM element, or None where the walk panics"""
    curve_name, px, py, qx, qy, n, m = args
    try:
        cols, aux, _o, _a, _pt = msm_witness(R.CURVES[curve_name], px, py, qx, qy, n, m)
    except R.RefPanic:
        return None
    return cols, aux


def fixed_base_job(args):
    curve_name, base, k = args
    cols, aux, _o, _a, _pt = fixed_base_witness(R.CURVES[curve_name], base, k)
    return cols, aux


def native_msm_job(args):
    """worker: n p + m q with the curve's affine big-int formulas (None: the point at infinity)"""
    curve_name, p, q, n, m = args
    C = R.CURVES[curve_name]
    return C.add(C.mul(n, p), C.mul(m, q))
