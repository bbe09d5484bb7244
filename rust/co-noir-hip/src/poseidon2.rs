//! The batched Poseidon2 entries of `libcosnarks_hip.so` (csrc/poseidon2.hip) as free functions: what the ACVM drivers' Poseidon2 call sites
//! can be pointed at -- `poseidon2_permutation` / the packed permutations with precomputation of co-noir/co-acvm/src/mpc/rep3.rs:1271-1305
//! and shamir.rs:737-775, co-noir-common/src/mpc/rep3.rs:321, and the Merkle trees of mpc-core/src/gadgets/merkle_tree/. d = 5, t = 2, 3, 4.
//! The library builds in no parameter set: [`Poseidon2Dev::new`] takes the fields of mpc-core's `Poseidon2Params`. Every pointer named
//! `*_dev` is device memory; the network rounds (`open_vec`, the reshares of the precomputation) stay the driver's.
use ark_ff::PrimeField;
use co_groth16_hip::error::check;
use co_groth16_hip::layout::limbs_of;
use cosnarks_hip_sys as sys;

pub const SPONGE: u32 = 0;
pub const COMPRESSION: u32 = 1;

/// One parameter set on the device (`csh_poseidon2_params_create`); freed on drop.
pub struct Poseidon2Dev {
    handle: sys::CshPoseidon2Params,
    pub field: i32,
    pub t: usize,
    pub rounds_f_beginning: usize,
    pub rounds_f_end: usize,
    pub rounds_p: usize,
}

impl Poseidon2Dev {
    /// `rc_external`: round after round, `t` constants each (`round_constants_external` flattened); `diag_m_1`: `mat_internal_diag_m_1`.
    pub fn new<F: PrimeField>(field: i32, t: usize, rounds_f_beginning: usize, rounds_f_end: usize, rc_external: &[F], rc_internal: &[F], diag_m_1: &[F]) -> eyre::Result<Self> {
        eyre::ensure!(rc_external.len() == (rounds_f_beginning + rounds_f_end) * t && diag_m_1.len() == t, "Poseidon2Dev: constant counts");
        let mut handle: sys::CshPoseidon2Params = core::ptr::null_mut();
        check(unsafe {
            sys::csh_poseidon2_params_create(field, t as u32, rounds_f_beginning as u32, rounds_f_end as u32, rc_internal.len() as u32, limbs_of(rc_external), limbs_of(rc_internal), limbs_of(diag_m_1), &mut handle)
        })?;
        Ok(Self { handle, field, t, rounds_f_beginning, rounds_f_end, rounds_p: rc_internal.len() })
    }

    /// `num_rounds()` of the reference: the collaborative permutation takes `rounds() + 1` steps.
    pub fn rounds(&self) -> usize {
        self.rounds_f_beginning + self.rounds_p + self.rounds_f_end
    }

    /// Precomputation entries round `r` consumes: what the caller advances `precomp.offset` by (poseidon2/rep3.rs:240).
    pub fn round_entries(&self, r: usize, n_perm: usize) -> usize {
        if r < self.rounds_f_beginning || r >= self.rounds_f_beginning + self.rounds_p { n_perm * self.t } else { n_perm }
    }

    /// `permutation_in_place` over `chunks_exact_mut(T)` of `n_perm` states; `out_dev` may be `state_dev`.
    pub fn permute_dev(&self, state_dev: *const u64, n_perm: usize, out_dev: *mut u64) -> eyre::Result<()> {
        check(unsafe { sys::csh_poseidon2_permute_dev(self.handle, state_dev, n_perm, out_dev, core::ptr::null_mut()) })
    }

    /// `merkle_tree_sponge` (`mode` = [`SPONGE`]) / `merkle_tree_compression` ([`COMPRESSION`]): `root_dev` receives one element;
    /// `work_dev`: 2 * (n_leaves / arity) elements.
    pub fn merkle_dev(&self, arity: usize, mode: u32, leaves_dev: *const u64, n_leaves: usize, root_dev: *mut u64, work_dev: *mut u64) -> eyre::Result<()> {
        check(unsafe { sys::csh_poseidon2_merkle_dev(self.handle, arity as u32, mode, leaves_dev, n_leaves, root_dev, work_dev, core::ptr::null_mut()) })
    }

    /// Step `step` of `rep3_permutation_in_place_with_precomputation_packed` / `shamir_..._packed`: the local stretch between two
    /// openings. `precomp_dev` = the five device vectors r, r^2, r^3, r^4, r^5; `precomp_offset` = `precomp.offset` at round `step`.
    #[allow(clippy::too_many_arguments)]
    pub fn co_round_dev(&self, protocol: u32, party_id: u32, step: usize, state_dev: *mut u64, n_perm: usize, y_dev: *const u64, precomp_dev: &[*const u64; 5], precomp_offset: usize, open_dev: *mut u64, ff_out_dev: *mut u64) -> eyre::Result<()> {
        check(unsafe {
            sys::csh_poseidon2_co_round_dev(self.field, protocol, party_id, self.handle, step as u32, state_dev, n_perm, y_dev, precomp_dev.as_ptr(), precomp_offset, open_dev, ff_out_dev, core::ptr::null_mut())
        })
    }

    /// The gather after a layer of `len` states of a collaborative tree (merkle_tree/rep3.rs:44-52, :99-111).
    pub fn layer_next_dev(&self, ncomp: u32, arity: usize, mode: u32, state_dev: *const u64, ff_dev: *const u64, next_dev: *mut u64, len: usize) -> eyre::Result<()> {
        check(unsafe { sys::csh_poseidon2_layer_next_dev(self.field, ncomp, self.t as u32, arity as u32, mode, state_dev, ff_dev, next_dev, len, core::ptr::null_mut()) })
    }
}

impl Drop for Poseidon2Dev {
    fn drop(&mut self) {
        unsafe { sys::csh_poseidon2_params_destroy(self.handle) };
    }
}
