//! The element-wise stages of `Round3::compute_t` (co-circom/co-plonk/src/round3.rs:246-502) as free functions over
//! `csh_plonk_quot_{blinders,operands,combine,finish}_dev`. `compute_t` is an inherent function of the reference's round type, not a method
//! of `CircomPlonkProver`, so its call site is pointed at these ("PLONK quotient"); the `mul_vec` rounds between the stages
//! stay the driver's. The vectors are device-resident: `DevShares` is a device pointer to `N * ncomp::<S>()` field elements that the caller
//! keeps alive until the stream has run the call (`csh_malloc`, or the buffer an `fft` of this crate left its result in). `S` is the share
//! type (`P::ScalarField`, a Shamir share, or `Rep3PrimeFieldShare`: two elements); `party` is `state.id()` as 0, 1, 2 (0 for the plain
//! driver). Every call is stream-ordered on the calling thread's stream and refuses outputs that overlap an input or each other.
use ark_ff::PrimeField;
use co_groth16_hip::domain::HipDomain;
use co_groth16_hip::error::check;
use co_groth16_hip::layout::{limbs, limbs_of, ncomp};
use cosnarks_hip_sys as sys;

/// A device pointer to a vector of shares (or, for `DevPublic`, of field elements) on the extended domain.
pub type DevShares = *mut u64;
pub type DevPublic = *const u64;

fn protocol<S>() -> u32 {
    ncomp::<S>() - 1 // 0 = plain / Shamir (one element per share), 1 = Rep3 (two)
}

/// round3.rs:269-274 and 339-353: `b` = challenges.b[0..9] -> [ap, bp, cp, zp, zwp] on the extended domain `ext` (4 n points, snarkjs root).
pub fn hip_quotient_blinders<S: Copy>(ext: &HipDomain, party: u32, b: &[S; 9], out: &[DevShares; 5]) -> eyre::Result<()> {
    check(unsafe { sys::csh_plonk_quot_blinders_dev(ext.raw(), protocol::<S>(), party, limbs_of(&b[..]), out.as_ptr(), core::ptr::null_mut()) })
}

/// round3.rs:320-419. `shares` = [a, b, c, z, a_b, a_bp, ap_b, ap_bp, ap, bp, cp]; `public` = the zkey's 4 n evaluations [qm, ql, qr, qo, qc,
/// s1, s2, s3]; `lagrange` = the 4 n evaluations of zkey.lagrange[..]; `buffer_a` = polys.buffer_a (one share per Lagrange polynomial);
/// `challenges` = [beta, gamma, k1, k2] -> `out` = [pi, e1, e1z, e2a, e2b, e2c, e3a, e3b, e3c, e3d]. e2d is z itself.
pub fn hip_quotient_operands<F: PrimeField, S: Copy>(
    ext: &HipDomain,
    party: u32,
    shares: &[DevShares; 11],
    public: &[DevPublic; 8],
    lagrange: &[DevPublic],
    buffer_a: &[S],
    challenges: &[F; 4],
    out: &[DevShares; 10],
) -> eyre::Result<()> {
    assert_eq!(lagrange.len(), buffer_a.len());
    let sh: [*const u64; 11] = shares.map(|p| p as *const u64);
    check(unsafe {
        sys::csh_plonk_quot_operands_dev(ext.raw(), protocol::<S>(), party, sh.as_ptr(), public.as_ptr(), lagrange.as_ptr(), lagrange.len(), limbs_of(buffer_a), limbs_of(&challenges[..]), out.as_ptr(), core::ptr::null_mut())
    })
}

/// round3.rs:88-105 (mul4vec_post) and 435-467. `shares` = [e1, e1z, z, zp, e2, e2z_0, e2z_1, e2z_2, e2z_3, e3, e3z_0, e3z_1, e3z_2, e3z_3];
/// `lagrange1` = zkey.lagrange[0] -> `out` = [t, tz].
pub fn hip_quotient_combine<F: PrimeField, S: Copy>(ext: &HipDomain, party: u32, shares: &[DevShares; 14], lagrange1: DevPublic, alpha: F, out: &[DevShares; 2]) -> eyre::Result<()> {
    let sh: [*const u64; 14] = shares.map(|p| p as *const u64);
    check(unsafe { sys::csh_plonk_quot_combine_dev(ext.raw(), protocol::<S>(), party, sh.as_ptr(), lagrange1, limbs(&alpha), out.as_ptr(), core::ptr::null_mut()) })
}

/// round3.rs:468-498 after the two `ifft`s: `ct`, `ctz` = the 4 n coefficients of t and tz, `b9_b10` = challenges.b[9..11] -> t1 (n + 1 shares),
/// t2 (n + 1), t3 (n + 6). `field` is the `csh_curve_t` of the scalar field, `n` = zkey.domain_size.
pub fn hip_quotient_finish<S: Copy>(field: i32, n: usize, party: u32, ct: DevShares, ctz: DevShares, b9_b10: &[S; 2], t1: DevShares, t2: DevShares, t3: DevShares) -> eyre::Result<()> {
    check(unsafe { sys::csh_plonk_quot_finish_dev(field, n, protocol::<S>(), party, ct as *const u64, ctz as *const u64, limbs_of(&b9_b10[..]), t1, t2, t3, core::ptr::null_mut()) })
}
