//! MI355X-backed implementors of co-noir's driver seam `NoirUltraHonkProver<P>` (co-noir/co-noir-common/src/mpc/mod.rs:17-408) for the
//! plain, Rep3 and Shamir protocols, and [`hip_fast_msm`], the GPU counterpart of `HonkCurve::fast_msm`
//! (co-noir-common/src/honk_curve.rs:35, 81-83 BN254 G1, 175-177 Grumpkin). Hot methods: `local_mul_vec` (:236), `msm_public_points`
//! (:358), `fft` (:373), `ifft` (:379); the other fifty are generated delegations to the reference's drivers (`cold.rs`).
//!
//! `HonkCurve::fast_msm` is an associated function of the curve types themselves, so call sites inside co-noir that name
//! `P::fast_msm` directly (commitments of the plain prover) stay on the CPU unless they are pointed at [`hip_fast_msm`]; every MSM
//! that goes through the driver trait (`T::msm_public_points`, all of the MPC provers' commitments) is offloaded by the implementors
//! here with no upstream edit.
mod cold;
pub mod drivers;
pub use drivers::{hip_fast_msm, HipPlainUltraHonkDriver, HipRep3UltraHonkDriver, HipShamirUltraHonkDriver};
pub mod oink;
pub use oink::{hip_lookup_operands, hip_perm_operands, hip_w4_records, hip_z_perm_place, DevMemoryRecords};
pub mod sumcheck;
pub use sumcheck::{gate_params, hip_compute_univariate, hip_compute_univariate_all, hip_compute_univariate_gates, hip_pow_table, AllAccumulators, GateAccumulators, UltraAccumulators};
pub mod co_sumcheck;
pub use co_sumcheck::{hip_co_arith, hip_co_delta_finish, hip_co_delta_operands, hip_co_delta_sub_one, hip_co_lookup_finish, hip_co_lookup_mid, hip_co_lookup_operands, hip_co_perm_finish, hip_co_perm_operands, hip_co_perm_operands2, hip_co_select_edges, CoBatch};
pub use co_sumcheck::{hip_co_ell_finish, hip_co_ell_operands, hip_co_ell_operands2, hip_co_mem_finish, hip_co_mem_operands, hip_co_nnf_finish, hip_co_nnf_operands, hip_co_pos_ext_finish, hip_co_pos_ext_operands, hip_co_pos_int_finish, hip_co_pos_int_operands, CoGatesBatch};
pub mod scans;
pub use scans::{hip_batch_inverse, hip_batched_polys_dev, hip_eval_poly, hip_prefix_product, hip_factor_roots};
pub mod poseidon2;
pub use poseidon2::Poseidon2Dev;
