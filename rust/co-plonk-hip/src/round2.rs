//! `Round2::compute_z` (co-circom/co-plonk/src/round2.rs:96-193) between its network rounds, and `blind_coefficients`
//! (co-plonk/src/lib.rs:162-177) of rounds 1 and 2, as free functions over `csh_plonk_z_operands_dev`, `csh_vec_rotate_right_dev` and
//! `csh_plonk_blind_coefficients_dev`. The serial loop over w^i that builds n1, n2, n3, d1, d2, d3 (round2.rs:116-155) is one call; the two
//! `array_prod_mul` rounds and the `mul_vec` stay the driver's (for the plain driver: `hip_prefix_product` and `hip_batch_inverse` of
//! `scans.rs`); `buffer_z.rotate_right(1)` (:171) and the blinding of the polynomial the next MSM reads follow on the same stream, so nothing
//! comes back to the host between the witness buffers and the commitment. Conventions (`DevShares`, `S`, `party`): `round3.rs`.
use ark_ff::PrimeField;
use co_groth16_hip::domain::HipDomain;
use co_groth16_hip::error::check;
use co_groth16_hip::layout::{limbs_of, ncomp};
use cosnarks_hip_sys as sys;

pub use crate::round3::{DevPublic, DevShares};

fn protocol<S>() -> u32 {
    ncomp::<S>() - 1 // 0 = plain / Shamir (one element per share), 1 = Rep3 (two)
}

/// round2.rs:116-155. `ext` = the EXTENDED domain (4 n points, snarkjs root); `buffers` = polys.buffer_a, buffer_b, buffer_c (n shares);
/// `sigma` = the 4 n evaluations of zkey.s1_poly, s2_poly, s3_poly (read at 4 i); `challenges` = [beta, gamma, k1, k2]
/// -> `out` = [n1, n2, n3, d1, d2, d3] (n shares each).
pub fn hip_z_operands<F: PrimeField, S: Copy>(ext: &HipDomain, party: u32, buffers: &[DevShares; 3], sigma: &[DevPublic; 3], challenges: &[F; 4], out: &[DevShares; 6]) -> eyre::Result<()> {
    let sh: [*const u64; 3] = buffers.map(|p| p as *const u64);
    check(unsafe { sys::csh_plonk_z_operands_dev(ext.raw(), protocol::<S>(), party, sh.as_ptr(), sigma.as_ptr(), limbs_of(&challenges[..]), out.as_ptr(), core::ptr::null_mut()) })
}

/// `buffer_z.rotate_right(k)` (round2.rs:171 with k = 1): out[(i + k) mod n] = input[i]; `out` is another buffer. `field` is the
/// `csh_curve_t` of the scalar field.
pub fn hip_rotate_right<S: Copy>(field: i32, input: DevShares, out: DevShares, n: usize, k: usize) -> eyre::Result<()> {
    check(unsafe { sys::csh_vec_rotate_right_dev(field, input as *const u64, out, n, ncomp::<S>(), k, core::ptr::null_mut()) })
}

/// `blind_coefficients(poly, coeff_rev)` (co-plonk/src/lib.rs:162-177; round1.rs:132 with two blinders, round2.rs:181 with three) on a device
/// polynomial of n coefficients with room for n + coeff_rev.len().
pub fn hip_blind_coefficients<S: Copy>(field: i32, poly: DevShares, n: usize, coeff_rev: &[S]) -> eyre::Result<()> {
    check(unsafe { sys::csh_plonk_blind_coefficients_dev(field, poly, n, ncomp::<S>(), limbs_of(coeff_rev), coeff_rev.len(), core::ptr::null_mut()) })
}
