//! The sumcheck round of the plain UltraHonk prover between two folds, over `csh_honk_sumcheck_accumulate_dev` and
//! `csh_honk_pow_table_dev`: the loop body of `SumcheckProverRound::compute_univariate_inner`
//! (co-noir/ultrahonk/src/decider/sumcheck/sumcheck_round_prover.rs:224-255) for the arithmetic, permutation, log-derivative lookup and
//! delta-range relations -- subrelations 0 .. 10 of the batching order (decider/relations/mod.rs:134-145) -- on columns that stay on the
//! device, and `GateSeparatorPolynomial::new`'s `beta_products` (decider/types.rs:53-67). The elliptic, memory, non-native field and
//! Poseidon2 relations and `batch_over_relations_univariates` (:109-122) stay with the caller, who adds their accumulators to these.
//! Plain field only: elements are field elements, one component. Stream-ordered on the calling thread's stream; the 57 result elements
//! come back with one copy.
use ark_ff::PrimeField;
use co_groth16_hip::error::check;
use co_groth16_hip::layout::{limbs_mut, limbs_of};
use cosnarks_hip_sys as sys;

/// Columns of `csh_honk_sumcheck_accumulate_dev`, in the order of the ABI: witness w_l, w_r, w_o, w_4, z_perm, lookup_inverses,
/// lookup_read_counts, lookup_read_tags; shifted witness w_l, w_r, w_o, w_4, z_perm; precomputed q_m, q_c, q_l, q_r, q_o, q_4, q_arith,
/// q_delta_range, q_lookup, sigma_1..4, id_1..4, table_1..4, lagrange_first, lagrange_last.
pub const SUMCHECK_COLUMNS: usize = 36;
/// Lengths of the eleven accumulators: arith.r0, arith.r1, perm.r0, perm.r1, lookup.r0, lookup.r1, lookup.r2, delta.r0 .. r3.
pub const ACC_LENGTHS: [usize; 11] = [6, 5, 6, 3, 5, 5, 3, 6, 6, 6, 6];
pub const ACC_ELEMS: usize = 57;

/// The accumulators of subrelations 0 .. 10 over the edges of `[edge_begin, edge_end)`; entry i of an accumulator is its evaluation at i.
pub struct UltraAccumulators<F> {
    pub flat: [F; ACC_ELEMS],
}

impl<F: PrimeField> UltraAccumulators<F> {
    /// accumulator s of the eleven
    pub fn subrelation(&self, s: usize) -> &[F] {
        let off: usize = ACC_LENGTHS[..s].iter().sum();
        &self.flat[off..off + ACC_LENGTHS[s]]
    }
}

/// The scaling factors of the round loop on the device: `beta_products` of `GateSeparatorPolynomial::new(betas, log_n)`
/// (decider/types.rs:53-67) into `out` (2^m elements, m = betas.len() <= 28).
pub fn hip_pow_table<F: PrimeField>(field: i32, betas: &[F], out: *mut u64) -> eyre::Result<()> {
    check(unsafe { sys::csh_honk_pow_table_dev(field, limbs_of(betas), betas.len(), out, core::ptr::null_mut()) })
}

/// The loop of `compute_univariate_inner` (:239-252) for `edge_idx in (edge_begin..edge_end).step_by(2)` with the per-relation skips
/// (:124-140). `cols` = the 36 device columns; `gate_separator` = (beta_products on the device, periodicity), or `None` for the factor
/// one (`compute_virtual_contribution`, :388-421); `params` = [beta, gamma, public_input_delta]. `acc_dev` = 57 elements of device
/// scratch. The round loop is `(0, round_size)`; `compute_disabled_contribution` (:340-386) is the last two or four elements.
pub fn hip_compute_univariate<F: PrimeField>(field: i32, cols: &[*const u64; SUMCHECK_COLUMNS], edge_begin: usize, edge_end: usize, gate_separator: Option<(*const u64, usize)>, params: &[F; 3], acc_dev: *mut u64) -> eyre::Result<UltraAccumulators<F>> {
    let (scaling, stride) = gate_separator.unwrap_or((core::ptr::null(), 1));
    check(unsafe { sys::csh_honk_sumcheck_accumulate_dev(field, cols.as_ptr(), edge_begin, edge_end, scaling, stride, limbs_of(&params[..]), acc_dev, core::ptr::null_mut()) })?;
    let mut flat = [F::zero(); ACC_ELEMS];
    check(unsafe { sys::csh_memcpy_d2h(limbs_mut(&mut flat[..]).cast(), acc_dev as *const core::ffi::c_void, 32 * ACC_ELEMS) })?;
    Ok(UltraAccumulators { flat })
}
