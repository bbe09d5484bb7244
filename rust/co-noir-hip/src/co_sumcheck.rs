//! The sumcheck round of the collaborative UltraHonk prover on shares, over the `csh_honk_co_*_dev` entries: the stretches of local
//! arithmetic between the `T::mul_many` calls of `UltraArithmeticRelation`, `UltraPermutationRelation`, `DeltaRangeConstraintRelation`
//! and `LogDerivLookupRelation` (co-noir/co-ultrahonk/src/co_decider/relations/ultra_arithmetic_relation.rs:88-239,
//! permutation_relation.rs:70-150 and :202-249, delta_range_constraint_relation.rs:126-216, logderiv_lookup_relation.rs:77-168 and
//! :255-312), the `can_skip` edge selection and `fold_accumulator!` (relations/mod.rs:45-57), on columns that stay on the device after
//! `csh_mle_fold_dev`. The batch of `AllEntitiesBatchRelations` (7 m elements per column) is never built: every stage computes its
//! elements from the columns. The network stays the caller's: between two stages it runs the local product
//! (`csh_rep3_local_mul_vec_dev`, `csh_vec_mul_dev`) and its own exchange. The reference's relation types are `pub(crate)`, so the call
//! sites inside `co_decider` are pointed at these functions. Stream-ordered on the calling thread's stream.
use ark_ff::PrimeField;
use co_groth16_hip::error::check;
use co_groth16_hip::layout::limbs_of;
use cosnarks_hip_sys as sys;

use crate::sumcheck::{GATES_COLUMNS, GATES_PARAMS, SUMCHECK_COLUMNS};

/// Batch elements per kept edge (MAX_PARTIAL_RELATION_LENGTH).
pub const CO_POINTS: usize = 7;

/// What the stages of one relation's batch share. `protocol` 0 = plain / Shamir (one component per share), 1 = Rep3 ({a, b}
/// interleaved); `cols` = the 36 device columns in the order of `csh_honk_sumcheck_accumulate_dev`, the 13 witness columns as shares (a
/// pointer may be null for a column the stage does not read); `edge_idx` = (the device list of `hip_co_select_edges`, its count), or
/// `None` for every edge of the range; `gate_separator` = (beta_products on the device, periodicity), or `None` for the factor one;
/// `params` = [beta, gamma, public_input_delta].
pub struct CoBatch<'a, F: PrimeField> {
    pub field: i32,
    pub protocol: u32,
    pub party_id: u32,
    pub cols: &'a [*const u64; SUMCHECK_COLUMNS],
    pub edge_begin: usize,
    pub edge_end: usize,
    pub edge_idx: Option<(*const u32, usize)>,
    pub gate_separator: Option<(*const u64, usize)>,
    pub params: &'a [F; 3],
}

impl<'a, F: PrimeField> CoBatch<'a, F> {
    /// m: the kept edges
    pub fn kept(&self) -> usize {
        self.edge_idx.map(|(_, m)| m).unwrap_or((self.edge_end - self.edge_begin) / 2)
    }
    fn list(&self) -> *const u32 {
        self.edge_idx.map(|(p, _)| p).unwrap_or(core::ptr::null())
    }
    fn scaling(&self) -> (*const u64, usize) {
        self.gate_separator.unwrap_or((core::ptr::null(), 1))
    }
}

/// `can_skip` (ultra_arithmetic_relation.rs:247-249, delta_range_constraint_relation.rs:94-96): the kept `e >> 1` of the range into
/// `edge_idx_dev` (ascending), their number into `count_dev`, which is copied back and returned.
pub fn hip_co_select_edges(field: i32, selector: *const u64, edge_begin: usize, edge_end: usize, edge_idx_dev: *mut u32, count_dev: *mut u32) -> eyre::Result<usize> {
    check(unsafe { sys::csh_honk_co_select_edges_dev(field, selector, edge_begin, edge_end, edge_idx_dev, count_dev, core::ptr::null_mut()) })?;
    let mut count = 0u32;
    check(unsafe { sys::csh_memcpy_d2h((&mut count as *mut u32).cast(), count_dev as *const core::ffi::c_void, 4) })?;
    Ok(count as usize)
}

/// `UltraArithmeticRelation::accumulate`: `r0_dev` = 6 elements of one component (a half share: the caller reshares it,
/// relations/mod.rs:140-162), `r1_dev` = 5 shares. `mask_dev` = the 7 m mask elements of `local_mul_vec` for Rep3, null for protocol 0.
pub fn hip_co_arith<F: PrimeField>(b: &CoBatch<F>, mask_dev: *const u64, r0_dev: *mut u64, r1_dev: *mut u64) -> eyre::Result<()> {
    let (scaling, stride) = b.scaling();
    check(unsafe { sys::csh_honk_co_arith_dev(b.field, b.protocol, b.party_id, b.cols.as_ptr(), b.edge_begin, b.edge_end, b.list(), b.kept(), scaling, stride, mask_dev, r0_dev, r1_dev, core::ptr::null_mut()) })
}

/// Permutation stage (a): `lhs_dev` = [wid_1 | wsigma_1 | wid_3 | wsigma_3], `rhs_dev` = [wid_2 | wsigma_2 | wid_4 | wsigma_4], 4 * 7 m shares each.
pub fn hip_co_perm_operands<F: PrimeField>(b: &CoBatch<F>, lhs_dev: *mut u64, rhs_dev: *mut u64) -> eyre::Result<()> {
    check(unsafe { sys::csh_honk_co_perm_operands_dev(b.field, b.protocol, b.party_id, b.cols.as_ptr(), b.edge_begin, b.edge_end, b.list(), b.kept(), limbs_of(&b.params[..]), lhs_dev, rhs_dev, core::ptr::null_mut()) })
}

/// Permutation stage (b): `rhs_dev` = [z_perm (+) lagrange_first | z_perm_shift (+) lagrange_last public_input_delta], 2 * 7 m shares.
pub fn hip_co_perm_operands2<F: PrimeField>(b: &CoBatch<F>, rhs_dev: *mut u64) -> eyre::Result<()> {
    check(unsafe { sys::csh_honk_co_perm_operands2_dev(b.field, b.protocol, b.party_id, b.cols.as_ptr(), b.edge_begin, b.edge_end, b.list(), b.kept(), limbs_of(&b.params[..]), rhs_dev, core::ptr::null_mut()) })
}

/// Permutation stage (c): `prod_dev` = mul_many([numerator | denominator], rhs) -> `acc_dev` = perm.r0 (6 shares), perm.r1 (3 shares).
pub fn hip_co_perm_finish<F: PrimeField>(b: &CoBatch<F>, prod_dev: *const u64, acc_dev: *mut u64) -> eyre::Result<()> {
    let (scaling, stride) = b.scaling();
    check(unsafe { sys::csh_honk_co_perm_finish_dev(b.field, b.protocol, b.party_id, b.cols.as_ptr(), b.edge_begin, b.edge_end, b.list(), b.kept(), scaling, stride, prod_dev, acc_dev, core::ptr::null_mut()) })
}

/// Delta-range stage (a): `lhs_dev` = [D_1 - 1 | .. | D_4 - 1 | D_1 - 2 | .. | D_4 - 2], 8 * 7 m shares; the caller squares it.
pub fn hip_co_delta_operands<F: PrimeField>(b: &CoBatch<F>, lhs_dev: *mut u64) -> eyre::Result<()> {
    check(unsafe { sys::csh_honk_co_delta_operands_dev(b.field, b.protocol, b.party_id, b.cols.as_ptr(), b.edge_begin, b.edge_end, b.list(), b.kept(), lhs_dev, core::ptr::null_mut()) })
}

/// Delta-range stage (b): add_assign_public(-1) on the 8 * 7 m shares of `sqr_dev`, in place.
pub fn hip_co_delta_sub_one(field: i32, protocol: u32, party_id: u32, sqr_dev: *mut u64, m: usize) -> eyre::Result<()> {
    check(unsafe { sys::csh_honk_co_delta_sub_one_dev(field, protocol, party_id, sqr_dev, m, core::ptr::null_mut()) })
}

/// Delta-range stage (c): `mul_dev` = the product of the two halves, 4 * 7 m shares -> `acc_dev` = delta.r0 .. r3 (6 shares each).
pub fn hip_co_delta_finish<F: PrimeField>(b: &CoBatch<F>, mul_dev: *const u64, acc_dev: *mut u64) -> eyre::Result<()> {
    let (scaling, stride) = b.scaling();
    check(unsafe { sys::csh_honk_co_delta_finish_dev(b.field, b.protocol, b.party_id, b.cols.as_ptr(), b.edge_begin, b.edge_end, b.list(), b.kept(), scaling, stride, mul_dev, acc_dev, core::ptr::null_mut()) })
}

/// Lookup stage (a): `read_term_dev` and the extended `lookup_inverses` in `inverses_dev`, 7 m shares each.
pub fn hip_co_lookup_operands<F: PrimeField>(b: &CoBatch<F>, read_term_dev: *mut u64, inverses_dev: *mut u64) -> eyre::Result<()> {
    check(unsafe { sys::csh_honk_co_lookup_operands_dev(b.field, b.protocol, b.party_id, b.cols.as_ptr(), b.edge_begin, b.edge_end, b.list(), b.kept(), limbs_of(&b.params[..]), read_term_dev, inverses_dev, core::ptr::null_mut()) })
}

/// Lookup stage (b): `write_inverse_dev` = mul_many(read_term, inverses) -> `r0_dev` = lookup.r0 (5 shares), `lhs_dev` = [write_inverse |
/// read_tag], `rhs_dev` = [read_counts | read_tag], 2 * 7 m shares each.
pub fn hip_co_lookup_mid<F: PrimeField>(b: &CoBatch<F>, write_inverse_dev: *const u64, r0_dev: *mut u64, lhs_dev: *mut u64, rhs_dev: *mut u64) -> eyre::Result<()> {
    let (scaling, stride) = b.scaling();
    check(unsafe { sys::csh_honk_co_lookup_mid_dev(b.field, b.protocol, b.party_id, b.cols.as_ptr(), b.edge_begin, b.edge_end, b.list(), b.kept(), scaling, stride, limbs_of(&b.params[..]), write_inverse_dev, r0_dev, lhs_dev, rhs_dev, core::ptr::null_mut()) })
}

/// Lookup stage (c): `mul_dev` = mul_many(lhs, rhs) -> `acc_dev` = lookup.r1 (5 shares, no scaling factor), lookup.r2 (3 shares).
pub fn hip_co_lookup_finish<F: PrimeField>(b: &CoBatch<F>, mul_dev: *const u64, acc_dev: *mut u64) -> eyre::Result<()> {
    let (scaling, stride) = b.scaling();
    check(unsafe { sys::csh_honk_co_lookup_finish_dev(b.field, b.protocol, b.party_id, b.cols.as_ptr(), b.edge_begin, b.edge_end, b.list(), b.kept(), scaling, stride, limbs_of(&b.params[..]), mul_dev, acc_dev, core::ptr::null_mut()) })
}

// ---- the five gate relations (csrc/honk_co_gates.hip): elliptic_relation.rs:102-254, memory_relation.rs:166-457,
// non_native_field_relation.rs:109-215, poseidon2_external_relation.rs:141-228, poseidon2_internal_relation.rs:135-227 ----

/// `CoBatch` over the 19 device columns of `csh_honk_sumcheck_accumulate_gates_dev` (the eight witness and shifted-witness columns as
/// shares) and its eight parameters (`crate::sumcheck::gate_params`); `edge_idx` = the list of `hip_co_select_edges` on the relation's
/// own selector (q_elliptic, q_memory, q_nnf, q_poseidon2_external, q_poseidon2_internal).
pub struct CoGatesBatch<'a, F: PrimeField> {
    pub field: i32,
    pub protocol: u32,
    pub party_id: u32,
    pub cols: &'a [*const u64; GATES_COLUMNS],
    pub edge_begin: usize,
    pub edge_end: usize,
    pub edge_idx: Option<(*const u32, usize)>,
    pub gate_separator: Option<(*const u64, usize)>,
    pub params: &'a [F; GATES_PARAMS],
}

impl<'a, F: PrimeField> CoGatesBatch<'a, F> {
    /// m: the kept edges
    pub fn kept(&self) -> usize {
        self.edge_idx.map(|(_, m)| m).unwrap_or((self.edge_end - self.edge_begin) / 2)
    }
    fn list(&self) -> *const u32 {
        self.edge_idx.map(|(p, _)| p).unwrap_or(core::ptr::null())
    }
    fn scaling(&self) -> (*const u64, usize) {
        self.gate_separator.unwrap_or((core::ptr::null(), 1))
    }
}

/// Elliptic stage (a): `lhs_dev` = [y1 | y2 | y1 | x_diff | y1 + y3 | y_diff | 3 x1], `rhs_dev` = [y1 | y2 | y2 | x_diff | x_diff | x3 - x1 | x1], 7 * 7 m shares each.
pub fn hip_co_ell_operands<F: PrimeField>(b: &CoGatesBatch<F>, lhs_dev: *mut u64, rhs_dev: *mut u64) -> eyre::Result<()> {
    check(unsafe { sys::csh_honk_co_ell_operands_dev(b.field, b.protocol, b.party_id, b.cols.as_ptr(), b.edge_begin, b.edge_end, b.list(), b.kept(), lhs_dev, rhs_dev, core::ptr::null_mut()) })
}

/// Elliptic stage (b): `mul1_dev` = mul_many(lhs, rhs) -> the operands of the second product, 5 * 7 m shares each.
pub fn hip_co_ell_operands2<F: PrimeField>(b: &CoGatesBatch<F>, mul1_dev: *const u64, lhs_dev: *mut u64, rhs_dev: *mut u64) -> eyre::Result<()> {
    check(unsafe { sys::csh_honk_co_ell_operands2_dev(b.field, b.protocol, b.party_id, b.cols.as_ptr(), b.edge_begin, b.edge_end, b.list(), b.kept(), limbs_of(&b.params[..]), mul1_dev, lhs_dev, rhs_dev, core::ptr::null_mut()) })
}

/// Elliptic stage (c): `acc_dev` = elliptic.r0, r1 (6 shares each).
pub fn hip_co_ell_finish<F: PrimeField>(b: &CoGatesBatch<F>, mul1_dev: *const u64, mul2_dev: *const u64, acc_dev: *mut u64) -> eyre::Result<()> {
    let (scaling, stride) = b.scaling();
    check(unsafe { sys::csh_honk_co_ell_finish_dev(b.field, b.protocol, b.party_id, b.cols.as_ptr(), b.edge_begin, b.edge_end, b.list(), b.kept(), scaling, stride, mul1_dev, mul2_dev, acc_dev, core::ptr::null_mut()) })
}

/// Memory stage (a): `lhs_dev`, `rhs_dev` = 6 * 7 m shares each in the order of memory_relation.rs:272-357, `rhs2_dev` =
/// neg_next_gate_access_type (+) 1 (7 m shares). The caller runs mul = mul_many(lhs, rhs), then mul2 = mul_many(mul[3], rhs2).
pub fn hip_co_mem_operands<F: PrimeField>(b: &CoGatesBatch<F>, lhs_dev: *mut u64, rhs_dev: *mut u64, rhs2_dev: *mut u64) -> eyre::Result<()> {
    check(unsafe { sys::csh_honk_co_mem_operands_dev(b.field, b.protocol, b.party_id, b.cols.as_ptr(), b.edge_begin, b.edge_end, b.list(), b.kept(), limbs_of(&b.params[..]), lhs_dev, rhs_dev, rhs2_dev, core::ptr::null_mut()) })
}

/// Memory stage (b): `acc_dev` = memory.r0 .. r5 (6 shares each).
pub fn hip_co_mem_finish<F: PrimeField>(b: &CoGatesBatch<F>, mul_dev: *const u64, mul2_dev: *const u64, acc_dev: *mut u64) -> eyre::Result<()> {
    let (scaling, stride) = b.scaling();
    check(unsafe { sys::csh_honk_co_mem_finish_dev(b.field, b.protocol, b.party_id, b.cols.as_ptr(), b.edge_begin, b.edge_end, b.list(), b.kept(), scaling, stride, limbs_of(&b.params[..]), mul_dev, mul2_dev, acc_dev, core::ptr::null_mut()) })
}

/// Non-native field stage (a): `lhs_dev` = [w1 | w2 | w4 | w3 | w1'], `rhs_dev` = [w2' | w1' | w1 | w2 | w2'], 5 * 7 m shares each.
pub fn hip_co_nnf_operands<F: PrimeField>(b: &CoGatesBatch<F>, lhs_dev: *mut u64, rhs_dev: *mut u64) -> eyre::Result<()> {
    check(unsafe { sys::csh_honk_co_nnf_operands_dev(b.field, b.protocol, b.party_id, b.cols.as_ptr(), b.edge_begin, b.edge_end, b.list(), b.kept(), lhs_dev, rhs_dev, core::ptr::null_mut()) })
}

/// Non-native field stage (b): `acc_dev` = nnf.r0 (6 shares).
pub fn hip_co_nnf_finish<F: PrimeField>(b: &CoGatesBatch<F>, mul_dev: *const u64, acc_dev: *mut u64) -> eyre::Result<()> {
    let (scaling, stride) = b.scaling();
    check(unsafe { sys::csh_honk_co_nnf_finish_dev(b.field, b.protocol, b.party_id, b.cols.as_ptr(), b.edge_begin, b.edge_end, b.list(), b.kept(), scaling, stride, mul_dev, acc_dev, core::ptr::null_mut()) })
}

/// Poseidon2 external stage (a): `s_dev` = [s1 | s2 | s3 | s4], s_i = w_i (+) q_i, 4 * 7 m shares; the caller runs the s-box's three products.
pub fn hip_co_pos_ext_operands<F: PrimeField>(b: &CoGatesBatch<F>, s_dev: *mut u64) -> eyre::Result<()> {
    check(unsafe { sys::csh_honk_co_pos_ext_operands_dev(b.field, b.protocol, b.party_id, b.cols.as_ptr(), b.edge_begin, b.edge_end, b.list(), b.kept(), s_dev, core::ptr::null_mut()) })
}

/// Poseidon2 external stage (b): `u_dev` = s^5 -> `acc_dev` = poseidon2_external.r0 .. r3 (7 shares each).
pub fn hip_co_pos_ext_finish<F: PrimeField>(b: &CoGatesBatch<F>, u_dev: *const u64, acc_dev: *mut u64) -> eyre::Result<()> {
    let (scaling, stride) = b.scaling();
    check(unsafe { sys::csh_honk_co_pos_ext_finish_dev(b.field, b.protocol, b.party_id, b.cols.as_ptr(), b.edge_begin, b.edge_end, b.list(), b.kept(), scaling, stride, u_dev, acc_dev, core::ptr::null_mut()) })
}

/// Poseidon2 internal stage (a): `s1_dev` = w_l (+) q_l, 7 m shares.
pub fn hip_co_pos_int_operands<F: PrimeField>(b: &CoGatesBatch<F>, s1_dev: *mut u64) -> eyre::Result<()> {
    check(unsafe { sys::csh_honk_co_pos_int_operands_dev(b.field, b.protocol, b.party_id, b.cols.as_ptr(), b.edge_begin, b.edge_end, b.list(), b.kept(), s1_dev, core::ptr::null_mut()) })
}

/// Poseidon2 internal stage (b): `u1_dev` = s1^5 -> `acc_dev` = poseidon2_internal.r0 .. r3 (7 shares each).
pub fn hip_co_pos_int_finish<F: PrimeField>(b: &CoGatesBatch<F>, u1_dev: *const u64, acc_dev: *mut u64) -> eyre::Result<()> {
    let (scaling, stride) = b.scaling();
    check(unsafe { sys::csh_honk_co_pos_int_finish_dev(b.field, b.protocol, b.party_id, b.cols.as_ptr(), b.edge_begin, b.edge_end, b.list(), b.kept(), scaling, stride, limbs_of(&b.params[..]), u1_dev, acc_dev, core::ptr::null_mut()) })
}
