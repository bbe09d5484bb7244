//! The whole-vector field scans of `libcosnarks_hip.so` as free functions next to [`crate::hip_fast_msm`]: what the delegated
//! `eval_poly`, `inv_many`, `inv_many_in_place[_leaking_zeros]` of a `NoirUltraHonkProver` implementor (cold.rs) can be pointed at
//! ("field scans"). `field` is the `csh_curve_t` whose scalar field the elements live in (`sys::CSH_BN254` for
//! BN254 G1); `S` is a field element or a share made of field elements (`Rep3PrimeFieldShare`: two).
use ark_ff::PrimeField;
use co_groth16_hip::error::{check, hip_ok};
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

/// `partially_evaluate_init` / `partially_evaluate_inplace` (co-ultrahonk co_sumcheck_prover.rs:34-98, ultrahonk sumcheck_prover.rs:20-60):
/// one sumcheck round on a set of equally long polynomials, `dst[v][j] = src[v][2j] + u (src[v][2j+1] - src[v][2j])` on every component
/// of the share. A fold in place is refused by the library (a race between workgroups), so the reference's in-place loop becomes a
/// ping-pong: the caller swaps `src` and `dst` after the round, truncates, and pushes a zero if fewer than 2 elements are left, as there.
pub fn hip_partially_evaluate<F: PrimeField, S: Copy + Default>(field: i32, src: &[&[S]], dst: &mut [Vec<S>], round_size: usize, u: F) {
    let ins: Vec<*const u64> = src.iter().map(|p| limbs_of(&p[..round_size])).collect();
    let outs: Vec<*mut u64> = dst
        .iter_mut()
        .map(|p| {
            p.resize(round_size / 2, S::default());
            limbs_mut(p)
        })
        .collect();
    let ch: *const F = &u;
    hip_ok(unsafe { sys::csh_mle_fold(field, ins.as_ptr(), outs.as_ptr(), ins.len(), round_size, ncomp::<S>(), ch.cast()) });
}

/// The folds of `compute_fold_polynomials` (co_shplemini_prover.rs:236-312, shplemini_prover.rs:198): A_1 .. A_(log_n - 1) and
/// `final_eval`, all log_n rounds in one call. The constant folds of the virtual rounds are scalar arithmetic on `final_eval` and stay
/// with the caller.
pub fn hip_fold_polynomials<F: PrimeField, S: Copy + Default>(field: i32, log_n: usize, multilinear_challenge: &[F], a_0: &[S]) -> (Vec<Vec<S>>, S) {
    let n = 1usize << log_n;
    let mut levels = vec![S::default(); n - 1];
    let mut final_eval = S::default();
    let res: *mut S = &mut final_eval;
    hip_ok(unsafe {
        sys::csh_mle_fold_rounds(field, limbs_of(&a_0[..n]), n, ncomp::<S>(), limbs_of(&multilinear_challenge[..log_n]), log_n, limbs_mut(&mut levels), res.cast())
    });
    let folds = (1..log_n).map(|l| levels[n - (n >> (l - 1))..n - (n >> l)].to_vec()).collect();
    (folds, final_eval)
}

/// `Polynomial::evaluate_mle` / `SharedPolynomial::evaluate_mle` (co-noir-common/src/polynomials/polynomial.rs:270-312,
/// shared_polynomial.rs:154-199): 2^dim coefficients folded dim times, only the last level comes back; the (1 - u) factors of the
/// trivial dimensions are scalar arithmetic and stay with the caller.
pub fn hip_evaluate_mle<F: PrimeField, S: Copy + Default>(field: i32, coeffs: &[S], evaluation_points: &[F]) -> S {
    let dim = coeffs.len().trailing_zeros() as usize;
    let mut out = S::default();
    let res: *mut S = &mut out;
    hip_ok(unsafe {
        sys::csh_mle_fold_rounds(field, limbs_of(coeffs), coeffs.len(), ncomp::<S>(), limbs_of(&evaluation_points[..dim]), dim, std::ptr::null_mut(), res.cast())
    });
    out
}

/// The batched polynomials of Gemini, `compute_batched_polys` (co-ultrahonk co_decider/co_shplemini/co_shplemini_prover.rs:49-119): one of
/// `batched_unshifted` / `batched_to_be_shifted` = sum_j rho^(first + j) f_j over the precomputed (public) polynomials, promoted to a share,
/// plus the same over the shared ones -- the reference's `add_scaled_slice` loops and `promote_poly` as ONE call on device-resident
/// polynomials. `public` / `shared`: device pointers with their lengths in elements / shares (a polynomial shorter than `n` counts as
/// zero behind its end); `public_scalars` / `shared_scalars`: the powers of rho the reference's `running_scalar` takes for them; `out`: n
/// shares, another buffer. `party` = `state.id()` as 0, 1, 2 (0 for the plain and Shamir drivers). Stream-ordered on the calling thread's stream.
#[allow(clippy::too_many_arguments)]
pub fn hip_batched_polys_dev<F: PrimeField, S: Copy>(
    field: i32,
    party: u32,
    public: &[*const u64],
    public_lens: &[usize],
    public_scalars: &[F],
    shared: &[*const u64],
    shared_lens: &[usize],
    shared_scalars: &[F],
    out: *mut u64,
    n: usize,
) -> eyre::Result<()> {
    assert!(public.len() == public_lens.len() && public.len() == public_scalars.len());
    assert!(shared.len() == shared_lens.len() && shared.len() == shared_scalars.len());
    check(unsafe {
        sys::csh_poly_lincomb_dev(field, ncomp::<S>() - 1, party, shared.as_ptr(), shared_lens.as_ptr(), limbs_of(shared_scalars), shared.len(), public.as_ptr(), public_lens.as_ptr(), limbs_of(public_scalars), public.len(), std::ptr::null(), out, n, std::ptr::null_mut())
    })
}
