// The UltraHonk sumcheck round between two folds, subrelations 11 .. 27: the accumulators of the elliptic, memory,
// non-native field and Poseidon2 relations over a range of edges (SumcheckProverRound::compute_univariate_inner,
// co-noir/ultrahonk/src/decider/sumcheck/sumcheck_round_prover.rs:224-255, and its two other callers compute_disabled_contribution
// :340-386 and compute_virtual_contribution :388-421). Expressions, column order, groups, skips and bounds: honk_gates.hpp, shared with
// the host self-test.
//
// k_hg_accumulate<F, G>, one launch per group G (elliptic + nnf, memory, Poseidon2): a workgroup of 256 lanes takes EDGES_WG edges at a
// time, lane t < 252 the point t / EDGES_WG of edge slot t % EDGES_WG (6 x 42 or 7 x 36), so the lanes of a point read consecutive
// elements of a column and every lane evaluates scalars. Lanes sum over a grid-stride loop (tune "vec_max_blocks", at most
// HG_MAX_BLOCKS), the workgroup reduces one running sum at a time through 9 KiB of LDS (one plane per limb), and its SUMS x POINTS
// partial sums go to the stream's workspace. k_hg_finish, one workgroup per output element, adds the workgroups' partials with the exact
// modular addition and writes the 110 elements. No atomics; the column pointers travel as kernel arguments. The launch bound asks for
// two waves per SIMD, the occupancy of k_hr_accumulate: every instance fits without scratch (profiles/honk_gates_kernel_meta.csv).
#include "honk_gates.hpp"

namespace csh {

constexpr int HG_WG = 256;
constexpr int HG_MAX_BLOCKS = 1024;  // partial sums the finishing launch adds per output

template <class F, int G>
__global__ __launch_bounds__(HG_WG, 2) void k_hg_accumulate(HgArgs<F> a, F* partial) {
  using LZ = typename LazyOf<F>::type;
  using GR = HgGroup<G>;
  __shared__ int32_t planes[LZ::NL * HG_WG];
  const int t = threadIdx.x, k = t / GR::EDGES_WG, slot = t % GR::EDGES_WG;
  LZ acc[GR::SUMS];
#pragma unroll
  for (int s = 0; s < GR::SUMS; ++s) acc[s] = LZ::zero();
  if (k < GR::POINTS) {
#pragma unroll 1
    for (size_t j = blockIdx.x * (size_t)GR::EDGES_WG + slot; j < a.n_edges; j += (size_t)gridDim.x * GR::EDGES_WG)
      hg_accumulate_edge<G>(a, j, k, acc);
  }
#pragma unroll
  for (int s = 0; s < GR::SUMS; ++s) {
    if (s) __syncthreads();  // the sums of s - 1 have been read
#pragma unroll
    for (int i = 0; i < LZ::NL; ++i) planes[i * HG_WG + t] = acc[s].l[i];
    __syncthreads();
    if (t < GR::POINTS) {
      LZ sum = LZ::zero();
#pragma unroll 1
      for (int q = 0; q < GR::EDGES_WG; ++q) {
        LZ x;
#pragma unroll
        for (int i = 0; i < LZ::NL; ++i) x.l[i] = planes[i * HG_WG + t * GR::EDGES_WG + q];
        sum = LZ::add(sum, x).fold_top();
      }
      partial[((size_t)blockIdx.x * GR::SUMS + s) * GR::POINTS + t] = sum.canonical_narrow().pack();
    }
  }
}

// Where the groups' partial sums are, and how many workgroups wrote each
template <class F>
struct HgFinishArgs {
  const F* partial[HG_GROUPS];
  uint32_t blocks[HG_GROUPS];
};
// blockIdx.x: the 18 (sum, point) pairs of group EN, then the 36 of MEM, then the 56 of POS
template <class F>
__global__ __launch_bounds__(HG_WG) void k_hg_finish(HgFinishArgs<F> a, F* acc) {
  __shared__ F sums[HG_WG];
  constexpr int N0 = HgGroup<HG_EN>::SUMS * HgGroup<HG_EN>::POINTS, N1 = HgGroup<HG_MEM>::SUMS * HgGroup<HG_MEM>::POINTS;
  constexpr int N2 = HgGroup<HG_POS>::SUMS * HgGroup<HG_POS>::POINTS;
  static_assert(N0 + N1 + N2 == HG_ACC_ELEMS, "every output element has one workgroup");
  int g, q, per, out;  // uniform over the workgroup
  if ((int)blockIdx.x < N0) {
    g = HG_EN, q = blockIdx.x, per = N0;
    out = HgGroup<HG_EN>::off(q / HgGroup<HG_EN>::POINTS) + q % HgGroup<HG_EN>::POINTS;
  } else if ((int)blockIdx.x < N0 + N1) {
    g = HG_MEM, q = blockIdx.x - N0, per = N1;
    out = HgGroup<HG_MEM>::off(q / HgGroup<HG_MEM>::POINTS) + q % HgGroup<HG_MEM>::POINTS;
  } else {
    g = HG_POS, q = blockIdx.x - N0 - N1, per = N2;
    out = HgGroup<HG_POS>::off(q / HgGroup<HG_POS>::POINTS) + q % HgGroup<HG_POS>::POINTS;
  }
  const F* partial = a.partial[g];
  const uint32_t blocks = a.blocks[g];
  F sum = F::zero();
  for (uint32_t b = threadIdx.x; b < blocks; b += HG_WG) sum = F::add(sum, partial[(size_t)b * per + q]);
  sums[threadIdx.x] = sum;
  __syncthreads();
  for (int w = HG_WG / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sums[threadIdx.x] = F::add(sums[threadIdx.x], sums[threadIdx.x + w]);
    __syncthreads();
  }
  if (threadIdx.x == 0) acc[out] = sums[0];
}

template <class F, int G>
static void launch_group(const HgArgs<F>& a, int mb, Arena& ar, HgFinishArgs<F>& fin, hipStream_t st) {
  using GR = HgGroup<G>;
  const int blocks = grid_for(a.n_edges, GR::EDGES_WG, mb);
  F* partial = ar.take<F>((size_t)blocks * GR::SUMS * GR::POINTS);
  fin.partial[G] = partial, fin.blocks[G] = (uint32_t)blocks;
  hipLaunchKernelGGL((k_hg_accumulate<F, G>), dim3(blocks), dim3(HG_WG), 0, st, a, partial);
}

template <class F>
static int sumcheck_accumulate_gates_t(const uint64_t* const* cols, size_t edge_begin, size_t edge_end, const uint64_t* scaling, size_t scaling_stride,
                                       const uint64_t* params, uint64_t* acc, hipStream_t st) {
  HgArgs<F> a;
  for (int c = 0; c < HG_COLS; ++c) a.col[c] = (const F*)cols[c];
  a.scaling = (const F*)scaling, a.scaling_stride = scaling_stride;
  a.edge_begin = edge_begin, a.n_edges = (edge_end - edge_begin) / 2;
  hg_consts(a, params);
  int mb = tune().vec_max_blocks.load(std::memory_order_relaxed);
  if (mb <= 0 || mb > HG_MAX_BLOCKS) mb = HG_MAX_BLOCKS;
  Arena& ar = arena_for(st);
  size_t bytes = 0;  // what the three takes below use: every group has at most mb workgroups
  bytes += Arena::padded((size_t)grid_for(a.n_edges, HgGroup<HG_EN>::EDGES_WG, mb) * HgGroup<HG_EN>::SUMS * HgGroup<HG_EN>::POINTS * sizeof(F));
  bytes += Arena::padded((size_t)grid_for(a.n_edges, HgGroup<HG_MEM>::EDGES_WG, mb) * HgGroup<HG_MEM>::SUMS * HgGroup<HG_MEM>::POINTS * sizeof(F));
  bytes += Arena::padded((size_t)grid_for(a.n_edges, HgGroup<HG_POS>::EDGES_WG, mb) * HgGroup<HG_POS>::SUMS * HgGroup<HG_POS>::POINTS * sizeof(F));
  CSH_TRY(ar.reserve(bytes));
  HgFinishArgs<F> fin;
  launch_group<F, HG_EN>(a, mb, ar, fin, st);
  launch_group<F, HG_MEM>(a, mb, ar, fin, st);
  launch_group<F, HG_POS>(a, mb, ar, fin, st);
  hipLaunchKernelGGL(k_hg_finish<F>, dim3(HG_ACC_ELEMS), dim3(HG_WG), 0, st, fin, (F*)acc);
  CSH_HIP(hipGetLastError());
  return CSH_OK;
}

}  // namespace csh

using namespace csh;

extern "C" {

int csh_honk_sumcheck_accumulate_gates_dev(csh_curve_t field_of, const uint64_t* const* cols_dev, size_t edge_begin, size_t edge_end,
                                           const uint64_t* scaling_dev, size_t scaling_stride, const uint64_t* params, uint64_t* acc_dev,
                                           void* stream) {
  const char* what = "honk_sumcheck_accumulate_gates";
  FR_REQUIRE_FIELD(field_of);
  CSH_REQUIRE(cols_dev && params && acc_dev, "honk_sumcheck_accumulate_gates: NULL argument");
  CSH_TRY(fr_require_ptrs((const void* const*)cols_dev, HG_COLS, what));
  CSH_REQUIRE(edge_begin % 2 == 0 && edge_end % 2 == 0 && edge_begin < edge_end && edge_end <= HR_MAX_EDGE_END,
              "honk_sumcheck_accumulate_gates: edge_begin and edge_end must be even, edge_begin < edge_end <= 2^28");
  CSH_REQUIRE(!scaling_dev || (scaling_stride >= 1 && scaling_stride <= HR_MAX_EDGE_END),
              "honk_sumcheck_accumulate_gates: scaling_stride must be 1 .. 2^28");
  FrRanges in, out;
  for (int c = 0; c < HG_COLS; ++c) in.add((const char*)cols_dev[c] + 32 * edge_begin, 32 * (edge_end - edge_begin));
  if (scaling_dev) in.add((const char*)scaling_dev + 32 * (edge_begin >> 1) * scaling_stride, 32 * (((edge_end - edge_begin) >> 1) - 1) * scaling_stride + 32);
  out.add(acc_dev, 32 * HG_ACC_ELEMS);
  CSH_TRY(fr_check_ranges(in, out, what));
  CSH_TRY(ensure_device());
  hipStream_t st = resolve_stream(stream);
  return FR_CALL(field_of, sumcheck_accumulate_gates_t<F>(cols_dev, edge_begin, edge_end, scaling_dev, scaling_stride, params, acc_dev, st));
}

}  // extern "C"
