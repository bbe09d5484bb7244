// The UltraHonk sumcheck round between two folds: the accumulators of subrelations 0 .. 10 over a range of edges
// (SumcheckProverRound::compute_univariate_inner, co-noir/ultrahonk/src/decider/sumcheck/sumcheck_round_prover.rs:224-255, and its two other
// callers compute_disabled_contribution :340-386 and compute_virtual_contribution :388-421), and the gate-separator table
// (GateSeparatorPolynomial::new, decider/types.rs:53-67). Expressions, column order, skips and bounds: honk_relations.hpp, shared with the
// host self-test.
//
// The accumulate entry is the one-group family HrFam through honk_stage.hpp's kernels (k_hs_accumulate<HrFam, F, 0>: 6 x 42 lanes at work, 66
// partial sums per workgroup; k_hs_finish<HrFam, F>: one workgroup per (subrelation, point), 57 elements written), argument rules and launcher.
#include "honk_relations.hpp"

namespace csh {

constexpr int HR_WG = 256;

template <class F>
__global__ __launch_bounds__(HR_WG) void k_hr_pow_table(HrPowArgs<F> a) {
  for (size_t i = blockIdx.x * (size_t)HR_WG + threadIdx.x; i < a.count; i += (size_t)gridDim.x * HR_WG) a.out[i] = hr_pow_at(a, i);
}

template <class F>
static int pow_table_t(const uint64_t* betas, size_t m, uint64_t* out, hipStream_t st) {
  HrPowArgs<F> a;
  memset(&a, 0, sizeof a);
  for (size_t b = 0; b < m; ++b) a.betad[b] = fr_to_rprime(fr_load<F>(betas + 4 * b));
  a.one = F::one();
  a.out = (F*)out, a.count = size_t(1) << m, a.m = (uint32_t)m;
  hipLaunchKernelGGL(k_hr_pow_table<F>, dim3(fr_stream_grid(a.count, HR_WG)), dim3(HR_WG), 0, st, a);
  CSH_HIP(hipGetLastError());
  return CSH_OK;
}

}  // namespace csh

using namespace csh;

extern "C" {

int csh_honk_sumcheck_accumulate_dev(csh_curve_t field_of, const uint64_t* const* cols_dev, size_t edge_begin, size_t edge_end,
                                     const uint64_t* scaling_dev, size_t scaling_stride, const uint64_t* params, uint64_t* acc_dev, void* stream) {
  return hs_entry<HrFam>(field_of, HsCall{cols_dev, edge_begin, edge_end, scaling_dev, scaling_stride, params, acc_dev}, "honk_sumcheck_accumulate", stream);
}

int csh_honk_pow_table_dev(csh_curve_t field_of, const uint64_t* betas, size_t m, uint64_t* out_dev, void* stream) {
  FR_REQUIRE_FIELD(field_of);
  CSH_REQUIRE(m <= HR_MAX_BETAS, "honk_pow_table: m must be 0 .. 28");
  CSH_REQUIRE(out_dev && (betas || !m), "honk_pow_table: NULL argument");
  CSH_TRY(ensure_device());
  hipStream_t st = resolve_stream(stream);
  return FR_CALL(field_of, pow_table_t<F>(betas, m, out_dev, st));
}

}  // extern "C"
