//! The whole-vector field scans of `libcosnarks_hip.so` as free functions next to [`crate::hip_fast_msm`]: what the delegated
//! `eval_poly`, `inv_many`, `inv_many_in_place[_leaking_zeros]` of a `NoirUltraHonkProver` implementor (cold.rs) can be pointed at
//! ("field scans"). `field` is the `csh_curve_t` whose scalar field the elements live in (`sys::CSH_BN254` for
//! BN254 G1); `S` is a field element or a share made of field elements (`Rep3PrimeFieldShare`: two).
use ark_ff::PrimeField;
use co_groth16_hip::error::hip_ok;
use co_groth16_hip::layout::{limbs_mut, limbs_of, ncomp};
use cosnarks_hip_sys as sys;

/// `poly::eval_poly(coeffs, point)` (mpc-core rep3/poly.rs:39-68; co_shplemini_prover.rs:382-444): sum_i coeffs[i] point^i on
/// every component of the share.
pub fn hip_eval_poly<F: PrimeField, S: Copy + Default>(field: i32, coeffs: &[S], point: F) -> S {
    let mut out = S::default();
    let pt: *const F = &point;
    let res: *mut S = &mut out;
    hip_ok(unsafe { sys::csh_eval_poly(field, limbs_of(coeffs), coeffs.len(), ncomp::<S>(), pt.cast(), res.cast()) });
    out
}

/// v[i] <- v[i]^-1 with one field inversion for the whole slice; a zero stays zero. Returns the number of zeros, so that the strict
/// callers (`inv_many`, `inv_many_in_place`: co-noir-common/src/mpc/rep3.rs:208-235) can bail as the reference does.
pub fn hip_batch_inverse<F: PrimeField>(field: i32, v: &mut [F]) -> usize {
    let mut zeros = 0usize;
    let n = v.len();
    let p = limbs_mut(v);
    hip_ok(unsafe { sys::csh_vec_batch_inverse(field, p as *const u64, p, n, &mut zeros) });
    zeros
}

/// v[i] <- v[0] * ... * v[i]: the running product over an opened vector.
pub fn hip_prefix_product<F: PrimeField>(field: i32, v: &mut [F]) {
    let n = v.len();
    let p = limbs_mut(v);
    hip_ok(unsafe { sys::csh_vec_prefix_prod(field, p as *const u64, p, n) });
}

/// `Polynomial::factor_roots` / `SharedPolynomial::factor_roots` (co-noir-common/src/polynomials/polynomial.rs:183,
/// shared_polynomial.rs:92-140): p(X) / (X - root) in place, in the reference's direction -- b_i = (-root)^-1 (a_i - b_(i-1)), the last
/// element popped -- on every component of the share. `sub0`, when given, is taken off coefficient 0 on the way in (every call site
/// does `tmp[0] -= evaluation` first: lib.rs:43-47, co_shplemini_prover.rs:661-737). Root 0 is the shift, as there.
pub fn hip_factor_roots<F: PrimeField, S: Copy + Default>(field: i32, coeffs: &mut Vec<S>, root: F, sub0: Option<S>) {
    if root.is_zero() {
        coeffs.remove(0);
        return;
    }
    let n = coeffs.len();
    let rt: *const F = &root;
    let s0: *const u64 = sub0.as_ref().map_or(std::ptr::null(), |s| (s as *const S).cast());
    let p = limbs_mut(coeffs);
    hip_ok(unsafe { sys::csh_poly_div_linear(field, p as *const u64, n, ncomp::<S>(), rt.cast(), s0, p, std::ptr::null_mut()) });
    coeffs.pop();
}
