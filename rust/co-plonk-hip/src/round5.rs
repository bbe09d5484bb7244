//! `Round5::compute_r` and `compute_wxi` (co-circom/co-plonk/src/round5.rs:118-259) as ONE `csh_poly_lincomb_dev` call followed by
//! `hip_div_by_zerofier` (`scans.rs`), and `compute_wxiw` (:262-278) as `hip_div_by_zerofier` with `sub0 = eval_zw`. The reference makes about
//! twenty passes over vectors of n + 6 shares; what they compute is a ragged linear combination of seven shared and eight public
//! polynomials under public coefficients, and those coefficients -- the scalar part of compute_r, O(n_public + log n) -- are derived here
//! on the host. Conventions (`DevShares`, `S`, `party`): `round3.rs`.
use ark_ff::PrimeField;
use co_groth16_hip::error::check;
use co_groth16_hip::layout::{limbs, limbs_of, ncomp};
use cosnarks_hip_sys as sys;

pub use crate::round3::{DevPublic, DevShares};

/// What round 5 reads of the proof so far and of the challenges (Round4Proof, Round5Challenges, VerifyingKey).
pub struct Round5Scalars<F: PrimeField> {
    pub eval_a: F,
    pub eval_b: F,
    pub eval_c: F,
    pub eval_s1: F,
    pub eval_s2: F,
    pub eval_zw: F,
    pub beta: F,
    pub gamma: F,
    pub alpha: F,
    pub xi: F,
    pub v: [F; 5],
    pub k1: F,
    pub k2: F,
}

/// The coefficients of the one linear combination: for the shares [z, t1, t2, t3, a, b, c], for the public [qm, ql, qr, qo, qc, s3, s1, s2],
/// and the constant added to coefficient 0.
pub struct Round5Coefficients<F: PrimeField> {
    pub shares: [F; 7],
    pub public: [F; 8],
    pub const0: F,
}

/// round5.rs:129-152 and :200 with plonk_utils::calculate_lagrange_evaluations / calculate_pi (co-plonk/src/lib.rs:179-214), then the
/// constants compute_wxi adds to coefficient 0 (:249-253). `power` = zkey.pow, `root_of_unity_pow` = domains.root_of_unity_pow,
/// `public_inputs` = data.witness.public_inputs (without the leading constant).
pub fn round5_coefficients<F: PrimeField>(power: usize, root_of_unity_pow: F, public_inputs: &[F], s: &Round5Scalars<F>) -> Round5Coefficients<F> {
    let mut xin = s.xi;
    let mut domain_size = 1u64;
    for _ in 0..power {
        xin.square_in_place();
        domain_size *= 2;
    }
    let zh = xin - F::one();
    let n = F::from(domain_size);
    let mut w = F::one();
    let mut l = Vec::with_capacity(usize::max(1, public_inputs.len()));
    for _ in 0..usize::max(1, public_inputs.len()) {
        l.push((w * zh) / (n * (s.xi - w)));
        w *= root_of_unity_pow;
    }
    let mut eval_pi = F::zero();
    for (val, l) in public_inputs.iter().zip(l.iter()) {
        eval_pi -= *l * val;
    }
    let betaxi = s.beta * s.xi;
    let e2 = (s.eval_a + betaxi + s.gamma) * (s.eval_b + betaxi * s.k1 + s.gamma) * (s.eval_c + betaxi * s.k2 + s.gamma) * s.alpha;
    let e3 = (s.eval_a + s.beta * s.eval_s1 + s.gamma) * (s.eval_b + s.beta * s.eval_s2 + s.gamma) * s.eval_zw * s.alpha;
    let e4 = s.alpha.square() * l[0];
    let r0 = eval_pi - e3 * (s.eval_c + s.gamma) - e4;
    Round5Coefficients {
        shares: [e2 + e4, -zh, -(zh * xin), -(zh * xin.square()), s.v[0], s.v[1], s.v[2]],
        public: [s.eval_a * s.eval_b, s.eval_a, s.eval_b, s.eval_c, F::one(), -(e3 * s.beta), s.v[3], s.v[4]],
        const0: r0 - s.v[0] * s.eval_a - s.v[1] * s.eval_b - s.v[2] * s.eval_c - s.v[3] * s.eval_s1 - s.v[4] * s.eval_s2,
    }
}

/// out[i] = sum_j share_coeffs[j] shares[j][i] (+) (sum_j public_coeffs[j] public[j][i] + [i = 0] const0) for i < out_len, every vector read
/// as far as its length goes. `protocol` 0 = plain / Shamir, 1 = Rep3; `field` is the `csh_curve_t` of the scalar field.
#[allow(clippy::too_many_arguments)]
pub fn hip_poly_lincomb<F: PrimeField, S: Copy>(
    field: i32,
    party: u32,
    shares: &[DevPublic],
    share_lens: &[usize],
    share_coeffs: &[F],
    public: &[DevPublic],
    public_lens: &[usize],
    public_coeffs: &[F],
    const0: Option<F>,
    out: DevShares,
    out_len: usize,
) -> eyre::Result<()> {
    assert!(shares.len() == share_lens.len() && shares.len() == share_coeffs.len());
    assert!(public.len() == public_lens.len() && public.len() == public_coeffs.len());
    let c0 = const0.as_ref().map_or(core::ptr::null(), limbs);
    check(unsafe {
        sys::csh_poly_lincomb_dev(field, ncomp::<S>() - 1, party, shares.as_ptr(), share_lens.as_ptr(), limbs_of(share_coeffs), shares.len(), public.as_ptr(), public_lens.as_ptr(), limbs_of(public_coeffs), public.len(), c0, out, out_len, core::ptr::null_mut())
    })
}

/// The numerator of W_xi (compute_r + compute_wxi before div_by_zerofier): `shares` = the coefficient forms [z, t1, t2, t3, a, b, c] with
/// n + 3, n + 1, n + 1, n + 6, n + 2, n + 2, n + 2 shares; `public` = the n coefficients of [qm, ql, qr, qo, qc, s3, s1, s2] -> `out`,
/// n + 6 shares. `hip_div_by_zerofier(out, n + 6, xi)` makes W_xi of it.
pub fn hip_wxi_numerator<F: PrimeField, S: Copy>(field: i32, party: u32, n: usize, shares: &[DevPublic; 7], public: &[DevPublic; 8], c: &Round5Coefficients<F>, out: DevShares) -> eyre::Result<()> {
    let share_lens = [n + 3, n + 1, n + 1, n + 6, n + 2, n + 2, n + 2];
    hip_poly_lincomb::<F, S>(field, party, &shares[..], &share_lens, &c.shares, &public[..], &[n; 8], &c.public, Some(c.const0), out, n + 6)
}
