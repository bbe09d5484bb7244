// The collaborative UltraHonk sumcheck round on shares, subrelations 11 .. 27: one device stage per stretch of local
// arithmetic between two network products of co-noir/co-ultrahonk/src/co_decider/relations/ for the elliptic, memory, non-native field,
// Poseidon2 external and Poseidon2 internal relations, and fold_accumulator! (relations/mod.rs:45-57) at the end of each. The network
// stays the caller's (csh_rep3_local_mul_vec_dev / csh_vec_mul_dev and its own exchange); the edges are selected by
// csh_honk_co_select_edges_dev on the relation's own selector. Expressions and operand layouts: honk_co_gates.hpp; the kernels, the
// launchers and the argument rules: honk_co_stage.hpp. Every entry here is one stage.
// mem_finish folds its six subrelations in two launches of three running sums each (hgc_stage): one launch of six needs 218 VGPRs, which
// leaves two waves per SIMD. profiles/honk_co_stage_kernel_meta.csv: no scratch, no VGPR spill.
#include "honk_co_gates.hpp"

using namespace csh;

#define HGC_COMMON_PARAMS                                                                                                                    \
  csh_curve_t field_of, uint32_t protocol, uint32_t party_id, const uint64_t *const *cols_dev, size_t edge_begin, size_t edge_end,          \
      const uint32_t *edge_idx_dev, size_t m
#define HGC_CALL(scaling, stride, params) \
  CoCall { protocol, party_id, cols_dev, edge_begin, edge_end, edge_idx_dev, m, scaling, stride, params }

extern "C" {

int csh_honk_co_ell_operands_dev(HGC_COMMON_PARAMS, uint64_t* lhs_dev, uint64_t* rhs_dev, void* stream) {
  return co_entry<HgcFamily, HGC_ELL_OPS>(field_of, HGC_CALL(nullptr, 1, nullptr), CoIo{nullptr, nullptr, {lhs_dev, rhs_dev, nullptr}, nullptr},
                                "honk_co_ell_operands", stream);
}
int csh_honk_co_ell_operands2_dev(HGC_COMMON_PARAMS, const uint64_t* params, const uint64_t* mul1_dev, uint64_t* lhs_dev, uint64_t* rhs_dev,
                                  void* stream) {
  return co_entry<HgcFamily, HGC_ELL_OPS2>(field_of, HGC_CALL(nullptr, 1, params), CoIo{mul1_dev, nullptr, {lhs_dev, rhs_dev, nullptr}, nullptr},
                                 "honk_co_ell_operands2", stream);
}
int csh_honk_co_ell_finish_dev(HGC_COMMON_PARAMS, const uint64_t* scaling_dev, size_t scaling_stride, const uint64_t* mul1_dev,
                               const uint64_t* mul2_dev, uint64_t* acc_dev, void* stream) {
  return co_entry<HgcFamily, HGC_ELL_FINISH>(field_of, HGC_CALL(scaling_dev, scaling_stride, nullptr),
                                   CoIo{mul1_dev, mul2_dev, {nullptr, nullptr, nullptr}, acc_dev}, "honk_co_ell_finish", stream);
}
int csh_honk_co_mem_operands_dev(HGC_COMMON_PARAMS, const uint64_t* params, uint64_t* lhs_dev, uint64_t* rhs_dev, uint64_t* rhs2_dev,
                                 void* stream) {
  return co_entry<HgcFamily, HGC_MEM_OPS>(field_of, HGC_CALL(nullptr, 1, params), CoIo{nullptr, nullptr, {lhs_dev, rhs_dev, rhs2_dev}, nullptr},
                                "honk_co_mem_operands", stream);
}
int csh_honk_co_mem_finish_dev(HGC_COMMON_PARAMS, const uint64_t* scaling_dev, size_t scaling_stride, const uint64_t* params,
                               const uint64_t* mul_dev, const uint64_t* mul2_dev, uint64_t* acc_dev, void* stream) {
  return co_entry<HgcFamily, HGC_MEM_FINISH>(field_of, HGC_CALL(scaling_dev, scaling_stride, params),
                                   CoIo{mul_dev, mul2_dev, {nullptr, nullptr, nullptr}, acc_dev}, "honk_co_mem_finish", stream);
}
int csh_honk_co_nnf_operands_dev(HGC_COMMON_PARAMS, uint64_t* lhs_dev, uint64_t* rhs_dev, void* stream) {
  return co_entry<HgcFamily, HGC_NNF_OPS>(field_of, HGC_CALL(nullptr, 1, nullptr), CoIo{nullptr, nullptr, {lhs_dev, rhs_dev, nullptr}, nullptr},
                                "honk_co_nnf_operands", stream);
}
int csh_honk_co_nnf_finish_dev(HGC_COMMON_PARAMS, const uint64_t* scaling_dev, size_t scaling_stride, const uint64_t* mul_dev, uint64_t* acc_dev,
                               void* stream) {
  return co_entry<HgcFamily, HGC_NNF_FINISH>(field_of, HGC_CALL(scaling_dev, scaling_stride, nullptr),
                                   CoIo{mul_dev, nullptr, {nullptr, nullptr, nullptr}, acc_dev}, "honk_co_nnf_finish", stream);
}
int csh_honk_co_pos_ext_operands_dev(HGC_COMMON_PARAMS, uint64_t* s_dev, void* stream) {
  return co_entry<HgcFamily, HGC_POS_EXT_OPS>(field_of, HGC_CALL(nullptr, 1, nullptr), CoIo{nullptr, nullptr, {s_dev, nullptr, nullptr}, nullptr},
                                    "honk_co_pos_ext_operands", stream);
}
int csh_honk_co_pos_ext_finish_dev(HGC_COMMON_PARAMS, const uint64_t* scaling_dev, size_t scaling_stride, const uint64_t* u_dev, uint64_t* acc_dev,
                                   void* stream) {
  return co_entry<HgcFamily, HGC_POS_EXT_FINISH>(field_of, HGC_CALL(scaling_dev, scaling_stride, nullptr),
                                       CoIo{u_dev, nullptr, {nullptr, nullptr, nullptr}, acc_dev}, "honk_co_pos_ext_finish", stream);
}
int csh_honk_co_pos_int_operands_dev(HGC_COMMON_PARAMS, uint64_t* s1_dev, void* stream) {
  return co_entry<HgcFamily, HGC_POS_INT_OPS>(field_of, HGC_CALL(nullptr, 1, nullptr), CoIo{nullptr, nullptr, {s1_dev, nullptr, nullptr}, nullptr},
                                    "honk_co_pos_int_operands", stream);
}
int csh_honk_co_pos_int_finish_dev(HGC_COMMON_PARAMS, const uint64_t* scaling_dev, size_t scaling_stride, const uint64_t* params,
                                   const uint64_t* u1_dev, uint64_t* acc_dev, void* stream) {
  return co_entry<HgcFamily, HGC_POS_INT_FINISH>(field_of, HGC_CALL(scaling_dev, scaling_stride, params),
                                       CoIo{u1_dev, nullptr, {nullptr, nullptr, nullptr}, acc_dev}, "honk_co_pos_int_finish", stream);
}

}  // extern "C"

// Host run of the stage functions of honk_co_gates.hpp on host pointers (co_host_run) behind the rules of the device entries. `stage` is an
// HgcStage; in / in2 are the stage's product vectors, out0 .. out2 its outputs in the order of the device entry (a fold stage: out0 = the
// accumulators).
extern "C" {

int csh_selftest_honk_co_gates_host(int field_of, int stage, uint32_t protocol, uint32_t party_id, const uint64_t* const* cols, size_t edge_begin,
                                    size_t edge_end, const uint32_t* edge_idx, size_t m, const uint64_t* scaling, size_t scaling_stride,
                                    const uint64_t* params, const uint64_t* in, const uint64_t* in2, uint64_t* out0, uint64_t* out1,
                                    uint64_t* out2) {
  CSH_REQUIRE(stage >= 0 && stage < HGC_STAGES, "selftest_honk_co_gates: unknown stage");
  const CoCall c{protocol, party_id, cols, edge_begin, edge_end, edge_idx, m, scaling, scaling_stride, params};
  const CoIo io = co_host_io<HgcFamily>(stage, in, in2, out0, out1, out2);
  CSH_TRY(co_check<HgcFamily>((csh_curve_t)field_of, stage, c, io, "selftest_honk_co_gates"));
  return FR_CALL(field_of, co_host_run<HgcFamily, F>(stage, c, io) ? CSH_OK : CSH_ERR_INVALID);
}

}  // extern "C"
