//! The whole-vector field scans of `libcosnarks_hip.so` as free functions of this crate: what the delegated
//! `evaluate_poly_public`, `inv_vec` and `array_prod_mul` of a `CircomPlonkProver` implementor (cold.rs) can be pointed at
//! ("field scans"). `field` is the `csh_curve_t` whose scalar field the elements live in (`sys::CSH_BN254` for
//! BN254 G1); `S` is a field element or a share made of field elements (`Rep3PrimeFieldShare`: two).
use ark_ff::PrimeField;
use co_groth16_hip::error::hip_ok;
use co_groth16_hip::layout::{limbs_mut, limbs_of, ncomp};
use cosnarks_hip_sys as sys;

/// `poly::eval_poly(coeffs, point)` (mpc-core rep3/poly.rs:39-68; evaluate_poly_public, co-plonk/src/round4.rs:126-132): sum_i coeffs[i] point^i on
/// every component of the share.
pub fn hip_eval_poly<F: PrimeField, S: Copy + Default>(field: i32, coeffs: &[S], point: F) -> S {
    let mut out = S::default();
    let pt: *const F = &point;
    let res: *mut S = &mut out;
    hip_ok(unsafe { sys::csh_eval_poly(field, limbs_of(coeffs), coeffs.len(), ncomp::<S>(), pt.cast(), res.cast()) });
    out
}

/// v[i] <- v[i]^-1 with one field inversion for the whole slice; a zero stays zero. Returns the number of zeros, so that the strict
/// callers (`inv_vec`: mpc-core rep3/arithmetic.rs:233-246) can bail as the reference does.
pub fn hip_batch_inverse<F: PrimeField>(field: i32, v: &mut [F]) -> usize {
    let mut zeros = 0usize;
    let n = v.len();
    let p = limbs_mut(v);
    hip_ok(unsafe { sys::csh_vec_batch_inverse(field, p as *const u64, p, n, &mut zeros) });
    zeros
}

/// v[i] <- v[0] * ... * v[i]: the serial loop of array_prod_mul over the opened vector (co-plonk/src/round2.rs:164-165, mpc/rep3.rs:211-213).
pub fn hip_prefix_product<F: PrimeField>(field: i32, v: &mut [F]) {
    let n = v.len();
    let p = limbs_mut(v);
    hip_ok(unsafe { sys::csh_vec_prefix_prod(field, p as *const u64, p, n) });
}

/// `Round5::div_by_zerofier(inout, 1, beta)` (co-plonk/src/round5.rs:78-91, called for W_xi and W_xiw at :255 and :274): the serial
/// `inout[i] = (inout[i - 1] - inout[i]) / beta` loop and the final resize, on every component of the share. Only n = 1 exists.
pub fn hip_div_by_zerofier<F: PrimeField, S: Copy + Default>(field: i32, inout: &mut Vec<S>, beta: F) {
    let n = inout.len();
    let rt: *const F = &beta;
    let p = limbs_mut(inout);
    hip_ok(unsafe { sys::csh_poly_div_linear(field, p as *const u64, n, ncomp::<S>(), rt.cast(), std::ptr::null(), p, std::ptr::null_mut()) });
    inout.pop();
}
