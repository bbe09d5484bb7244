//! The sumcheck round of the plain UltraHonk prover between two folds, over `csh_honk_sumcheck_accumulate_dev`,
//! `csh_honk_sumcheck_accumulate_gates_dev` and `csh_honk_pow_table_dev`: the loop body of
//! `SumcheckProverRound::compute_univariate_inner` (co-noir/ultrahonk/src/decider/sumcheck/sumcheck_round_prover.rs:224-255) on columns
//! that stay on the device -- `hip_compute_univariate` for the arithmetic, permutation, log-derivative lookup and delta-range relations,
//! subrelations 0 .. 10 of the batching order (decider/relations/mod.rs:134-145); `hip_compute_univariate_gates` for the elliptic,
//! memory, non-native field and Poseidon2 relations, subrelations 11 .. 27; `hip_compute_univariate_all` for the 28 accumulators of
//! `accumulate_relation_univariates` (:160-222) -- and `GateSeparatorPolynomial::new`'s `beta_products` (decider/types.rs:53-67).
//! `batch_over_relations_univariates` (:109-122), a few hundred scalar operations on the 28 accumulators, stays with the caller.
//! Plain field only: elements are field elements, one component. Stream-ordered on the calling thread's stream; the 57 and the 110
//! result elements come back with one copy each.
use ark_ff::{BigInteger, PrimeField};
use co_noir_common::honk_curve::HonkCurve;
use co_noir_common::honk_proof::TranscriptFieldType;
use mpc_core::gadgets::poseidon2::POSEIDON2_BN254_T4_PARAMS;
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

/// Columns of `csh_honk_sumcheck_accumulate_gates_dev`, in the order of the ABI: witness w_l, w_r, w_o, w_4; shifted witness w_l, w_r,
/// w_o, w_4; precomputed q_m, q_c, q_l, q_r, q_o, q_4; gate selectors q_elliptic, q_memory, q_nnf, q_poseidon2_external,
/// q_poseidon2_internal. The first fourteen are columns 0 .. 3, 8 .. 11 and 13 .. 18 of `SUMCHECK_COLUMNS`.
pub const GATES_COLUMNS: usize = 19;
/// Lengths of the seventeen accumulators: elliptic.r0, r1, memory.r0 .. r5, nnf.r0, poseidon2_external.r0 .. r3, poseidon2_internal.r0 .. r3.
pub const GATES_ACC_LENGTHS: [usize; 17] = [6, 6, 6, 6, 6, 6, 6, 6, 6, 7, 7, 7, 7, 7, 7, 7, 7];
pub const GATES_ACC_ELEMS: usize = 110;
/// eta_1, eta_2, eta_3, curve_b, mat_internal_diag_m_1[0..4)
pub const GATES_PARAMS: usize = 8;

/// The accumulators of subrelations 11 .. 27 over the edges of `[edge_begin, edge_end)`; entry i of an accumulator is its evaluation at i.
pub struct GateAccumulators<F> {
    pub flat: [F; GATES_ACC_ELEMS],
}

impl<F: PrimeField> GateAccumulators<F> {
    /// accumulator s of the seventeen
    pub fn subrelation(&self, s: usize) -> &[F] {
        let off: usize = GATES_ACC_LENGTHS[..s].iter().sum();
        &self.flat[off..off + GATES_ACC_LENGTHS[s]]
    }
}

/// What the five relations read beside the columns, made at run time from the reference's own values: the three etas of
/// `RelationParameters`, `P::get_curve_b()` (elliptic_relation.rs:134) and `POSEIDON2_BN254_T4_PARAMS.mat_internal_diag_m_1`
/// (poseidon2_internal_relation.rs:154-165, carried into `P::ScalarField` as the reference's `F::from(BigUint::from(..))` does).
pub fn gate_params<P: HonkCurve<TranscriptFieldType>>(eta_1: P::ScalarField, eta_2: P::ScalarField, eta_3: P::ScalarField) -> [P::ScalarField; GATES_PARAMS] {
    let diag = |i: usize| P::ScalarField::from_le_bytes_mod_order(&POSEIDON2_BN254_T4_PARAMS.mat_internal_diag_m_1[i].into_bigint().to_bytes_le());
    [eta_1, eta_2, eta_3, P::get_curve_b(), diag(0), diag(1), diag(2), diag(3)]
}

/// The same loop as `hip_compute_univariate` for the elliptic, memory, non-native field, Poseidon2 external and Poseidon2 internal
/// relations (elliptic_relation.rs:81-161, memory_relation.rs:145-358, non_native_field_relation.rs:85-177,
/// poseidon2_external_relation.rs:121-205, poseidon2_internal_relation.rs:118-200) with their skips: each is left out of an edge when
/// its own selector is zero at both ends. `cols` = the 19 device columns; `params` = `gate_params`; `acc_dev` = 110 elements of device
/// scratch. Range and `gate_separator` as in `hip_compute_univariate`.
pub fn hip_compute_univariate_gates<F: PrimeField>(field: i32, cols: &[*const u64; GATES_COLUMNS], edge_begin: usize, edge_end: usize, gate_separator: Option<(*const u64, usize)>, params: &[F; GATES_PARAMS], acc_dev: *mut u64) -> eyre::Result<GateAccumulators<F>> {
    let (scaling, stride) = gate_separator.unwrap_or((core::ptr::null(), 1));
    check(unsafe { sys::csh_honk_sumcheck_accumulate_gates_dev(field, cols.as_ptr(), edge_begin, edge_end, scaling, stride, limbs_of(&params[..]), acc_dev, core::ptr::null_mut()) })?;
    let mut flat = [F::zero(); GATES_ACC_ELEMS];
    check(unsafe { sys::csh_memcpy_d2h(limbs_mut(&mut flat[..]).cast(), acc_dev as *const core::ffi::c_void, 32 * GATES_ACC_ELEMS) })?;
    Ok(GateAccumulators { flat })
}

/// The 28 accumulators of `accumulate_relation_univariates` (:160-222) in the order of `AllRelationAcc` (relations/mod.rs:134-145):
/// arith, perm, lookup, delta, then elliptic, memory, nnf, poseidon2 external, poseidon2 internal. `AllRelationAcc` itself is private to
/// the reference's `ultrahonk` crate, so a caller inside it copies `subrelation(s)` into `r_arith.r0 .. r_pos_int.r3` in this order.
pub struct AllAccumulators<F> {
    pub ultra: UltraAccumulators<F>,
    pub gates: GateAccumulators<F>,
}

impl<F: PrimeField> AllAccumulators<F> {
    pub const SUBRELATIONS: usize = 28;
    /// accumulator s of the 28: the operand of alphas[s - 1] in `AllRelationAcc::scale` (s = 0: first_scalar)
    pub fn subrelation(&self, s: usize) -> &[F] {
        if s < ACC_LENGTHS.len() { self.ultra.subrelation(s) } else { self.gates.subrelation(s - ACC_LENGTHS.len()) }
    }
}

/// Both entries over one range: `cols` and `gate_cols` as above (fourteen device vectors are in both), `acc_dev` = 57 + 110 elements
/// of device scratch.
pub fn hip_compute_univariate_all<F: PrimeField>(field: i32, cols: &[*const u64; SUMCHECK_COLUMNS], gate_cols: &[*const u64; GATES_COLUMNS], edge_begin: usize, edge_end: usize, gate_separator: Option<(*const u64, usize)>, params: &[F; 3], gate_params: &[F; GATES_PARAMS], acc_dev: *mut u64) -> eyre::Result<AllAccumulators<F>> {
    let ultra = hip_compute_univariate(field, cols, edge_begin, edge_end, gate_separator, params, acc_dev)?;
    let gates = hip_compute_univariate_gates(field, gate_cols, edge_begin, edge_end, gate_separator, gate_params, unsafe { acc_dev.add(4 * ACC_ELEMS) })?;
    Ok(AllAccumulators { ultra, gates })
}
