// The group framework of the plain UltraHonk sumcheck round: everything of the round that names no column and
// no relation. A family -- subrelations 0 .. 10 of honk_relations.hpp (one group), the five gate relations of honk_gates.hpp (three) --
// gives an argument struct on HsArgs, one HsGroup descriptor per group and the loop body accumulate_edge<G>; the per-point view, the two
// kernels (a lane per point of an edge slot, grid-stride loop, one running sum at a time through 9 KiB of LDS; then one workgroup per
// (group, sum, point) adds the workgroups' partials: exact modular additions, no atomics), the launcher, the argument rules and the
// host run are here, once.
#pragma once
#include "common.hpp"
#include "field.hpp"
#include "field29.hpp"
#include "fr_entry.hpp"

namespace csh {

constexpr int HS_WG = 256;
constexpr int HS_MAX_SUMS = 11;
constexpr int HS_MAX_BLOCKS = 1024;  // partial sums the finishing launch adds per output
constexpr size_t HR_MAX_EDGE_END = size_t(1) << 28;

// ---- what a group is --------------------------------------------------------------------------------------------------------------------
// The relations one launch takes, as data: its running sums, its points, its edges per pass of a workgroup, the waves per SIMD its launch
// bound asks for (0 = none asked), and each sum's place (first element) and length in the family's output. A sum is evaluated at all
// `points`; what lies at or behind its length is dropped when the result is written.
struct HsGroup {
  int sums, points, edges_wg, waves;
  int off[HS_MAX_SUMS], len[HS_MAX_SUMS];
};
// the places tile [0, ACC_ELEMS) without overlap, no length exceeds its group's points, and every (point, edge slot) has a lane
template <class FAM>
constexpr bool hs_family_ok() {
  int hits[FAM::ACC_ELEMS] = {};
  for (int g = 0; g < FAM::GROUPS; ++g) {
    const HsGroup d = FAM::group(g);
    if (d.sums > HS_MAX_SUMS || d.points * d.edges_wg > HS_WG) return false;
    for (int s = 0; s < d.sums; ++s) {
      if (d.len[s] > d.points || d.off[s] < 0 || d.off[s] + d.len[s] > FAM::ACC_ELEMS) return false;
      for (int k = 0; k < d.len[s]; ++k) ++hits[d.off[s] + k];
    }
  }
  for (int i = 0; i < FAM::ACC_ELEMS; ++i)
    if (hits[i] != 1) return false;
  return true;
}
// workgroups of the finishing launch: the (sum, point) pairs of every group
template <class FAM>
constexpr int hs_finish_grid() {
  int n = 0;
  for (int g = 0; g < FAM::GROUPS; ++g) n += FAM::group(g).sums * FAM::group(g).points;
  return n;
}

// What one call is told; a family adds its constants, `one` (filled in by hs_args) among them: its place decides the accumulate kernels'
// register rows. Edge j (0 <= j < n_edges) is the pair of elements edge_begin + 2 j, edge_begin + 2 j + 1 of every column.
template <class F, int COLS_>
struct HsArgs {
  using Field = F;
  const F* col[COLS_];
  const F* scaling;       // factor of edge j = scaling[((edge_begin >> 1) + j) * scaling_stride]; NULL = one
  size_t scaling_stride;
  size_t edge_begin, n_edges;
};

template <class LZ>
CSH_HD LZ hr_extend(const LZ& v0, const LZ& v1, int k);  // honk_relations.hpp

// The per-point view of one edge: what a lane (or the self-test's loop) hands to the relations. at(c) is the column's value at the point.
template <class A>
struct HsPoint {
  using LZ = typename LazyOf<typename A::Field>::type;
  const A& a;
  size_t j, e;  // the edge, and its first element
  int k;        // the point
  CSH_HD HsPoint(const A& a_, size_t j_, int k_) : a(a_), j(j_), e(a_.edge_begin + 2 * j_), k(k_) {}
  CSH_HD LZ at(int c) const { return hr_extend(LZ::unpack(a.col[c][e]), LZ::unpack(a.col[c][e + 1]), k); }
  CSH_HD LZ one() const { return LZ::unpack(a.one); }
  CSH_HD LZ scaling() const { return LZ::unpack(a.scaling ? a.scaling[((a.edge_begin >> 1) + j) * a.scaling_stride] : a.one); }
  // the edge's two elements are zero / equal to another column's (inputs are canonical: equal residues are equal words)
  CSH_HD bool zero_at_both_ends(int c) const { return a.col[c][e].is_zero() && a.col[c][e + 1].is_zero(); }
  CSH_HD bool same_at_both_ends(int c, int d) const { return a.col[c][e] == a.col[d][e] && a.col[c][e + 1] == a.col[d][e + 1]; }
};

// ---- kernels ----------------------------------------------------------------------------------------------------------------------------
// partial[(block * sums + s) * points + k]
template <class FAM, class F, int G>
__global__ __launch_bounds__(HS_WG, FAM::group(G).waves) void k_hs_accumulate(typename FAM::template Args<F> a, F* partial) {
  using LZ = typename LazyOf<F>::type;
  constexpr HsGroup D = FAM::group(G);
  constexpr int SUMS = D.sums, POINTS = D.points, EDGES_WG = D.edges_wg;
  __shared__ int32_t planes[LZ::NL * HS_WG];
  const int t = threadIdx.x, k = t / EDGES_WG, slot = t % EDGES_WG;
  LZ acc[SUMS];
#pragma unroll
  for (int s = 0; s < SUMS; ++s) acc[s] = LZ::zero();
  if (k < POINTS) {
#pragma unroll 1
    for (size_t j = blockIdx.x * (size_t)EDGES_WG + slot; j < a.n_edges; j += (size_t)gridDim.x * EDGES_WG)
      FAM::template accumulate_edge<G>(a, j, k, acc);
  }
#pragma unroll
  for (int s = 0; s < SUMS; ++s) {
    if (s) __syncthreads();  // the sums of s - 1 have been read
#pragma unroll
    for (int i = 0; i < LZ::NL; ++i) planes[i * HS_WG + t] = acc[s].l[i];
    __syncthreads();
    if (t < POINTS) {
      LZ sum = LZ::zero();
#pragma unroll 1
      for (int q = 0; q < EDGES_WG; ++q) {
        LZ x;
#pragma unroll
        for (int i = 0; i < LZ::NL; ++i) x.l[i] = planes[i * HS_WG + t * EDGES_WG + q];
        sum = LZ::add(sum, x).fold_top();
      }
      partial[((size_t)blockIdx.x * SUMS + s) * POINTS + t] = sum.canonical_narrow().pack();
    }
  }
}

// Where the groups' partial sums are, and how many workgroups wrote each
template <class F, int GROUPS>
struct HsFinish {
  const F* partial[GROUPS];
  uint32_t blocks[GROUPS];
};
// Workgroup r of the finishing launch, counted from group G's first -- the (sum, point) pairs of group 0, then those of group 1, ...:
// its group, its pair q of the group's `per`, and the output element it writes (-1: the point lies at or behind its sum's length)
template <class FAM, int G = 0>
CSH_HD void hs_finish_place(int r, int& g, int& q, int& per, int& out) {
  if constexpr (G < FAM::GROUPS) {
    constexpr HsGroup D = FAM::group(G);
    if (r >= D.sums * D.points) return hs_finish_place<FAM, G + 1>(r - D.sums * D.points, g, q, per, out);
    const int s = r / D.points, k = r % D.points;
    g = G, q = r, per = D.sums * D.points, out = k < D.len[s] ? D.off[s] + k : -1;
  }
}
template <class FAM, class F>
__global__ __launch_bounds__(HS_WG) void k_hs_finish(HsFinish<F, FAM::GROUPS> f, F* acc) {
  __shared__ F sums[HS_WG];
  int g = 0, q = 0, per = 0, out = -1;  // uniform over the workgroup
  hs_finish_place<FAM>(blockIdx.x, g, q, per, out);
  if (out < 0) return;
  const F* partial = f.partial[g];
  const uint32_t blocks = f.blocks[g];
  F sum = F::zero();
  for (uint32_t b = threadIdx.x; b < blocks; b += HS_WG) sum = F::add(sum, partial[(size_t)b * per + q]);
  sums[threadIdx.x] = sum;
  __syncthreads();
  for (int w = HS_WG / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sums[threadIdx.x] = F::add(sums[threadIdx.x], sums[threadIdx.x + w]);
    __syncthreads();
  }
  if (threadIdx.x == 0) acc[out] = sums[0];
}

// ---- launcher ---------------------------------------------------------------------------------------------------------------------------
struct HsCall {
  const uint64_t* const* cols;
  size_t edge_begin, edge_end;
  const uint64_t* scaling;
  size_t scaling_stride;
  const uint64_t* params;
  uint64_t* acc;
};
template <class FAM, class F>
inline typename FAM::template Args<F> hs_args(const HsCall& c) {
  typename FAM::template Args<F> a;
  for (int k = 0; k < FAM::COLS; ++k) a.col[k] = (const F*)c.cols[k];
  a.scaling = (const F*)c.scaling, a.scaling_stride = c.scaling_stride;
  a.edge_begin = c.edge_begin, a.n_edges = (c.edge_end - c.edge_begin) / 2;
  a.one = F::one();
  FAM::consts(a, c.params);
  return a;
}
// the groups from G on: with `fin`, launched in their order, each with its own partial sums; without, the bytes those take
template <class FAM, class F, int G = 0>
inline size_t hs_groups(const typename FAM::template Args<F>& a, int mb, Arena& ar, HsFinish<F, FAM::GROUPS>* fin, hipStream_t st) {
  if constexpr (G < FAM::GROUPS) {
    constexpr HsGroup D = FAM::group(G);
    const int blocks = grid_for(a.n_edges, D.edges_wg, mb);
    const size_t count = (size_t)blocks * D.sums * D.points;
    if (fin) {
      F* partial = ar.take<F>(count);
      fin->partial[G] = partial, fin->blocks[G] = (uint32_t)blocks;
      hipLaunchKernelGGL((k_hs_accumulate<FAM, F, G>), dim3(blocks), dim3(HS_WG), 0, st, a, partial);
    }
    return Arena::padded(count * sizeof(F)) + hs_groups<FAM, F, G + 1>(a, mb, ar, fin, st);
  }
  return 0;
}
template <class FAM, class F>
inline int hs_run(const HsCall& c, hipStream_t st) {
  const auto a = hs_args<FAM, F>(c);
  int mb = tune().vec_max_blocks.load(std::memory_order_relaxed);
  if (mb <= 0 || mb > HS_MAX_BLOCKS) mb = HS_MAX_BLOCKS;
  Arena& ar = arena_for(st);
  CSH_TRY(ar.reserve(hs_groups<FAM, F>(a, mb, ar, nullptr, st)));
  HsFinish<F, FAM::GROUPS> fin;
  hs_groups<FAM, F>(a, mb, ar, &fin, st);
  hipLaunchKernelGGL((k_hs_finish<FAM, F>), dim3(hs_finish_grid<FAM>()), dim3(HS_WG), 0, st, fin, (F*)c.acc);
  CSH_HIP(hipGetLastError());
  return CSH_OK;
}

// ---- argument rules and the entry -------------------------------------------------------------------------------------------------------
// In this order: field, NULL argument, the column pointers, the range, the stride, the overlaps.
template <class FAM>
inline int hs_check(csh_curve_t field_of, const HsCall& c, const char* what) {
  auto refuse = [&](const char* rule) { return set_error("%s: %s", what, rule), CSH_ERR_INVALID; };
  FR_REQUIRE_FIELD(field_of);
  if (!(c.cols && c.params && c.acc)) return refuse("NULL argument");
  CSH_TRY(fr_require_ptrs((const void* const*)c.cols, FAM::COLS, what));
  if (!(c.edge_begin % 2 == 0 && c.edge_end % 2 == 0 && c.edge_begin < c.edge_end && c.edge_end <= HR_MAX_EDGE_END))
    return refuse("edge_begin and edge_end must be even, edge_begin < edge_end <= 2^28");
  if (c.scaling && !(c.scaling_stride >= 1 && c.scaling_stride <= HR_MAX_EDGE_END)) return refuse("scaling_stride must be 1 .. 2^28");
  FrRanges in, out;
  const size_t n = c.edge_end - c.edge_begin;
  for (int k = 0; k < FAM::COLS; ++k) in.add((const char*)c.cols[k] + 32 * c.edge_begin, 32 * n);
  if (c.scaling) in.add((const char*)c.scaling + 32 * (c.edge_begin >> 1) * c.scaling_stride, 32 * ((n >> 1) - 1) * c.scaling_stride + 32);
  out.add(c.acc, 32 * FAM::ACC_ELEMS);
  return fr_check_ranges(in, out, what);
}
template <class FAM>
inline int hs_entry(csh_curve_t field_of, const HsCall& c, const char* what, void* stream) {
  CSH_TRY(hs_check<FAM>(field_of, c, what));
  CSH_TRY(ensure_device());
  hipStream_t st = resolve_stream(stream);
  return FR_CALL(field_of, hs_run<FAM, F>(c, st));
}

// ---- the host run of the self-tests: one lane's loop per point and group -- as many passes as the range has edges -- through the function
// a lane of k_hs_accumulate calls, on host pointers, written where k_hs_finish writes ------------------------------------------------------
template <class FAM, class F, int G = 0>
inline void hs_host_groups(const typename FAM::template Args<F>& a, F* acc_out) {
  using LZ = typename LazyOf<F>::type;
  if constexpr (G < FAM::GROUPS) {
    constexpr HsGroup D = FAM::group(G);
    for (int k = 0; k < D.points; ++k) {
      LZ acc[D.sums];
      for (int s = 0; s < D.sums; ++s) acc[s] = LZ::zero();
      for (size_t j = 0; j < a.n_edges; ++j) FAM::template accumulate_edge<G>(a, j, k, acc);
      for (int s = 0; s < D.sums; ++s)
        if (k < D.len[s]) acc_out[D.off[s] + k] = acc[s].canonical_narrow().pack();
    }
    hs_host_groups<FAM, F, G + 1>(a, acc_out);
  }
}
template <class FAM, class F>
inline int hs_host_run(const HsCall& c) {
  hs_host_groups<FAM, F>(hs_args<FAM, F>(c), (F*)c.acc);
  return CSH_OK;
}

}  // namespace csh
