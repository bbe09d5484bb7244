// The UltraHonk sumcheck round between two folds: the accumulators of subrelations 0 .. 10 over a range of edges
// (SumcheckProverRound::compute_univariate_inner, co-noir/ultrahonk/src/decider/sumcheck/sumcheck_round_prover.rs:224-255, and its two other
// callers compute_disabled_contribution :340-386 and compute_virtual_contribution :388-421), and the gate-separator table
// (GateSeparatorPolynomial::new, decider/types.rs:53-67). Expressions, column order, skips and bounds: honk_relations.hpp, shared with the
// host self-test.
//
// k_hr_accumulate: a workgroup of 256 lanes takes 42 edges at a time, lane t < 252 the point t / 42 of edge slot t % 42 -- the 42 lanes of a
// point read consecutive elements of a column, and every lane evaluates scalars. Lanes sum over a grid-stride loop (tune "vec_max_blocks",
// at most HR_MAX_BLOCKS), the workgroup reduces one subrelation at a time through 9 KiB of LDS (one plane per limb), and its 66 partial
// sums go to the stream's workspace. k_hr_finish, one workgroup per (subrelation, point), adds the workgroups' partials with the exact
// modular addition and writes the 57 elements. No atomics; the column pointers travel as kernel arguments.
#include "honk_relations.hpp"

namespace csh {

constexpr int HR_WG = 256;
constexpr int HR_EDGES_WG = 42;            // 6 x 42 = 252 lanes at work
constexpr int HR_MAX_BLOCKS = 1024;        // partial sums the finishing launch adds per output
constexpr int HR_ALL = 15;                 // all four relations in one launch

template <class F, int REL>
__global__ __launch_bounds__(HR_WG) void k_hr_accumulate(HrArgs<F> a, F* partial) {
  using LZ = typename LazyOf<F>::type;
  __shared__ int32_t planes[LZ::NL * HR_WG];
  const int t = threadIdx.x, k = t / HR_EDGES_WG, slot = t % HR_EDGES_WG;
  LZ acc[HR_SUBRELATIONS];
#pragma unroll
  for (int s = 0; s < HR_SUBRELATIONS; ++s) acc[s] = LZ::zero();
  if (k < HR_POINTS) {
#pragma unroll 1
    for (size_t j = blockIdx.x * (size_t)HR_EDGES_WG + slot; j < a.n_edges; j += (size_t)gridDim.x * HR_EDGES_WG)
      hr_accumulate_edge<REL>(a, j, k, acc);
  }
#pragma unroll
  for (int s = 0; s < HR_SUBRELATIONS; ++s) {
    if (s) __syncthreads();  // the sums of subrelation s - 1 have been read
#pragma unroll
    for (int i = 0; i < LZ::NL; ++i) planes[i * HR_WG + t] = acc[s].l[i];
    __syncthreads();
    if (t < HR_POINTS) {
      LZ sum = LZ::zero();
#pragma unroll 1
      for (int q = 0; q < HR_EDGES_WG; ++q) {
        LZ x;
#pragma unroll
        for (int i = 0; i < LZ::NL; ++i) x.l[i] = planes[i * HR_WG + t * HR_EDGES_WG + q];
        sum = LZ::add(sum, x).fold_top();
      }
      partial[((size_t)blockIdx.x * HR_SUBRELATIONS + s) * HR_POINTS + t] = sum.canonical_narrow().pack();
    }
  }
}

// blockIdx.x = s * HR_POINTS + k
template <class F>
__global__ __launch_bounds__(HR_WG) void k_hr_finish(const F* __restrict__ partial, uint32_t blocks, F* acc) {
  __shared__ F sums[HR_WG];
  const int s = blockIdx.x / HR_POINTS, k = blockIdx.x % HR_POINTS;
  if (k >= hr_acc_len(s)) return;  // uniform over the workgroup
  F sum = F::zero();
  for (uint32_t b = threadIdx.x; b < blocks; b += HR_WG) sum = F::add(sum, partial[(size_t)b * (HR_SUBRELATIONS * HR_POINTS) + blockIdx.x]);
  sums[threadIdx.x] = sum;
  __syncthreads();
  for (int w = HR_WG / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sums[threadIdx.x] = F::add(sums[threadIdx.x], sums[threadIdx.x + w]);
    __syncthreads();
  }
  if (threadIdx.x == 0) acc[hr_acc_off(s) + k] = sums[0];
}

template <class F>
__global__ __launch_bounds__(HR_WG) void k_hr_pow_table(HrPowArgs<F> a) {
  for (size_t i = blockIdx.x * (size_t)HR_WG + threadIdx.x; i < a.count; i += (size_t)gridDim.x * HR_WG) a.out[i] = hr_pow_at(a, i);
}

template <class F>
static int sumcheck_accumulate_t(const uint64_t* const* cols, size_t edge_begin, size_t edge_end, const uint64_t* scaling, size_t scaling_stride,
                                 const uint64_t* params, uint64_t* acc, hipStream_t st) {
  HrArgs<F> a;
  for (int c = 0; c < HR_COLS; ++c) a.col[c] = (const F*)cols[c];
  a.scaling = (const F*)scaling, a.scaling_stride = scaling_stride;
  a.edge_begin = edge_begin, a.n_edges = (edge_end - edge_begin) / 2;
  hr_consts(a, params);
  int mb = tune().vec_max_blocks.load(std::memory_order_relaxed);
  if (mb <= 0 || mb > HR_MAX_BLOCKS) mb = HR_MAX_BLOCKS;
  const int blocks = grid_for(a.n_edges, HR_EDGES_WG, mb);
  Arena& ar = arena_for(st);
  const size_t count = (size_t)blocks * HR_SUBRELATIONS * HR_POINTS;
  CSH_TRY(ar.reserve(Arena::padded(count * sizeof(F))));
  F* partial = ar.take<F>(count);
  hipLaunchKernelGGL((k_hr_accumulate<F, HR_ALL>), dim3(blocks), dim3(HR_WG), 0, st, a, partial);
  hipLaunchKernelGGL(k_hr_finish<F>, dim3(HR_SUBRELATIONS * HR_POINTS), dim3(HR_WG), 0, st, (const F*)partial, (uint32_t)blocks, (F*)acc);
  CSH_HIP(hipGetLastError());
  return CSH_OK;
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
  const char* what = "honk_sumcheck_accumulate";
  FR_REQUIRE_FIELD(field_of);
  CSH_REQUIRE(cols_dev && params && acc_dev, "honk_sumcheck_accumulate: NULL argument");
  CSH_TRY(fr_require_ptrs((const void* const*)cols_dev, HR_COLS, what));
  CSH_REQUIRE(edge_begin % 2 == 0 && edge_end % 2 == 0 && edge_begin < edge_end && edge_end <= HR_MAX_EDGE_END,
              "honk_sumcheck_accumulate: edge_begin and edge_end must be even, edge_begin < edge_end <= 2^28");
  CSH_REQUIRE(!scaling_dev || (scaling_stride >= 1 && scaling_stride <= HR_MAX_EDGE_END),
              "honk_sumcheck_accumulate: scaling_stride must be 1 .. 2^28");
  FrRanges in, out;
  for (int c = 0; c < HR_COLS; ++c) in.add((const char*)cols_dev[c] + 32 * edge_begin, 32 * (edge_end - edge_begin));
  if (scaling_dev) in.add((const char*)scaling_dev + 32 * (edge_begin >> 1) * scaling_stride, 32 * (((edge_end - edge_begin) >> 1) - 1) * scaling_stride + 32);
  out.add(acc_dev, 32 * HR_ACC_ELEMS);
  CSH_TRY(fr_check_ranges(in, out, what));
  CSH_TRY(ensure_device());
  hipStream_t st = resolve_stream(stream);
  return FR_CALL(field_of, sumcheck_accumulate_t<F>(cols_dev, edge_begin, edge_end, scaling_dev, scaling_stride, params, acc_dev, st));
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
