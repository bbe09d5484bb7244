// The UltraHonk sumcheck round between two folds, subrelations 11 .. 27: the accumulators of the elliptic, memory,
// non-native field and Poseidon2 relations over a range of edges (SumcheckProverRound::compute_univariate_inner,
// co-noir/ultrahonk/src/decider/sumcheck/sumcheck_round_prover.rs:224-255, and its two other callers compute_disabled_contribution
// :340-386 and compute_virtual_contribution :388-421). Expressions, column order, groups, skips and bounds: honk_gates.hpp, shared with
// the host self-test.
//
// The entry is the three-group family HgFam through honk_stage.hpp's kernels (k_hs_accumulate<HgFam, F, G>, one launch per group G:
// elliptic + nnf, memory, Poseidon2; k_hs_finish<HgFam, F>: one workgroup per output element), argument rules and launcher. The launch
// bound asks for two waves per SIMD, as the first entry's kernel has: no instance uses scratch (profiles/honk_stage_kernel_meta.csv).
#include "honk_gates.hpp"

using namespace csh;

extern "C" {

int csh_honk_sumcheck_accumulate_gates_dev(csh_curve_t field_of, const uint64_t* const* cols_dev, size_t edge_begin, size_t edge_end,
                                           const uint64_t* scaling_dev, size_t scaling_stride, const uint64_t* params, uint64_t* acc_dev,
                                           void* stream) {
  return hs_entry<HgFam>(field_of, HsCall{cols_dev, edge_begin, edge_end, scaling_dev, scaling_stride, params, acc_dev}, "honk_sumcheck_accumulate_gates",
                         stream);
}

}  // extern "C"
