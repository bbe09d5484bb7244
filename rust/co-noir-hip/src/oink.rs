//! The whole-trace loops of the Oink prover (co-noir/co-ultrahonk/src/co_oink/co_oink_prover.rs; plain twin
//! co-noir/ultrahonk/src/oink/oink_prover.rs) between [`crate::hip_fast_msm`] and the scans, as free functions over
//! `csh_honk_w4_records_dev`, `csh_honk_lookup_operands_dev`, `csh_honk_perm_operands_dev` and `csh_honk_z_perm_place_dev`. All four are
//! affine in the shares with public coefficients: the `mul_many`, `array_prod_mul` and `batch_invert` rounds between them stay the
//! driver's (for the plain driver: `csh_vec_mul_dev`, `hip_prefix_product` and `hip_batch_inverse` of `scans.rs`). Vectors are device
//! pointers: shares of `S` (n per polynomial), public polynomials of n field elements. `field` is the `csh_curve_t` of the scalar field,
//! `party` = `state.id()` as 0, 1, 2 (0 for the plain and Shamir drivers). Stream-ordered on the calling thread's stream.
use ark_ff::PrimeField;
use co_groth16_hip::error::check;
use co_groth16_hip::layout::{limbs_of, ncomp};
use cosnarks_hip_sys as sys;

fn protocol<S>() -> u32 {
    ncomp::<S>() - 1 // 0 = plain / Shamir (one element per share), 1 = Rep3 (two)
}

fn flat(ranges: &[(usize, usize)]) -> Vec<usize> {
    ranges.iter().flat_map(|r| [r.0, r.1]).collect()
}

/// The memory-record rows of a proving key as device lists of u32 (`memory_read_records`, `memory_write_records`, the rows of
/// `memory_records_shared`), uploaded once by the caller, who has checked that every row is below n and occurs once.
pub struct DevMemoryRecords {
    pub read: *const u32,
    pub n_read: usize,
    pub write: *const u32,
    pub n_write: usize,
    pub shared: *const u32,
    pub n_shared: usize,
}

/// `add_ram_rom_memory_records_to_wire_4` (co_oink_prover.rs:119-160 with `compute_w4_inner`, :98-117) on a device copy of w_4 of n
/// shares (the clone + resize of :133-137 is `hip_batched_polys_dev` with the one share term w_4 under coefficient one). `w` = w_l, w_r,
/// w_o; `etas` = [eta_1, eta_2, eta_3]; `type_shares` = the shares of `memory_records_shared`, in the order of `records.shared`.
pub fn hip_w4_records<F: PrimeField, S: Copy>(field: i32, party: u32, w: &[*const u64; 3], w4: *mut u64, n: usize, etas: &[F; 3], records: &DevMemoryRecords, type_shares: *const u64) -> eyre::Result<()> {
    check(unsafe {
        sys::csh_honk_w4_records_dev(field, protocol::<S>(), party, w.as_ptr(), w4, n, limbs_of(&etas[..]), records.read, records.n_read, records.write, records.n_write, records.shared, type_shares, records.n_shared, core::ptr::null_mut())
    })
}

/// The loop of `compute_logderivative_inverses` (co_oink_prover.rs:229-277 with `compute_lookup_term`, :162-211, and
/// `compute_table_term`, :214-227). `shares` = w_l, w_r, w_o, lookup_read_tags; `public` = q_r, q_m, q_c, q_o, table_1 .. table_4, q_lookup;
/// `challenges` = [beta, gamma] -> `out` = [write_term * read_term, q_lookup_mul_read_tag]: the operands of the `mul_many` of :278.
pub fn hip_lookup_operands<F: PrimeField, S: Copy>(field: i32, party: u32, shares: &[*const u64; 4], public: &[*const u64; 9], n: usize, challenges: &[F; 2], out: &[*mut u64; 2]) -> eyre::Result<()> {
    check(unsafe { sys::csh_honk_lookup_operands_dev(field, protocol::<S>(), party, shares.as_ptr(), public.as_ptr(), n, limbs_of(&challenges[..]), out.as_ptr(), core::ptr::null_mut()) })
}

/// The four `batched_grand_product_num_denom` loops of `compute_grand_product` (co_oink_prover.rs:344-451). `shares` = w_l, w_r, w_o, w_4;
/// `public` = id_1 .. id_4, sigma_1 .. sigma_4; `domain_size` = final_active_wire_idx + 1; `ranges` = the active ranges (empty: none);
/// `challenges` = [beta, gamma] -> `out` = n_1 .. n_4, d_1 .. d_4 of active_domain_size - 1 shares each.
#[allow(clippy::too_many_arguments)]
pub fn hip_perm_operands<F: PrimeField, S: Copy>(field: i32, party: u32, shares: &[*const u64; 4], public: &[*const u64; 8], n: usize, domain_size: usize, ranges: &[(usize, usize)], challenges: &[F; 2], out: &[*mut u64; 8]) -> eyre::Result<()> {
    let rg = flat(ranges);
    check(unsafe {
        sys::csh_honk_perm_operands_dev(field, protocol::<S>(), party, shares.as_ptr(), public.as_ptr(), n, domain_size, rg.as_ptr(), ranges.len(), limbs_of(&challenges[..]), out.as_ptr(), core::ptr::null_mut())
    })
}

/// The tail of `compute_grand_product` (co_oink_prover.rs:472-504): `mul` = numerator / denominator (active_domain_size - 1 shares) ->
/// every element of `z_perm` (n shares, another buffer).
#[allow(clippy::too_many_arguments)]
pub fn hip_z_perm_place<S: Copy>(field: i32, party: u32, mul: *const u64, z_perm: *mut u64, n: usize, domain_size: usize, ranges: &[(usize, usize)]) -> eyre::Result<()> {
    let rg = flat(ranges);
    check(unsafe { sys::csh_honk_z_perm_place_dev(field, protocol::<S>(), party, mul, z_perm, n, domain_size, rg.as_ptr(), ranges.len(), core::ptr::null_mut()) })
}
