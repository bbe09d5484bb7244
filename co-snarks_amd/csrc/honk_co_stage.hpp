// The stage framework of the collaborative UltraHonk sumcheck round on shares: everything of the round that names
// no column and no relation. The two families of stages -- the four relations of honk_co_relations.hpp and the five gate relations of
// honk_co_gates.hpp -- each give a stage enum, an argument struct on CoArgs with their constants, one CoStage descriptor per stage and the
// loop bodies ops_at / terms_at; the element rule, the three kernels, the launchers, the argument rules and the host run are here, once.
//
// The batch is never built. The reference's batch element t of a column (extend_edges + fold_and_filter + add_entities,
// co_sumcheck/co_sumcheck_round.rs:54-73, types_batch.rs:105-130, relations/mod.rs:69-80) belongs to kept edge j = t / 7 and point
// k = t % 7 and is col[e] + k (col[e + 1] - col[e]) per component, e = 2 edge_idx[j] with an edge list and edge_begin + 2 j without; its
// scaling element is scaling[(e >> 1) stride]. Every stage computes its elements from the columns through this rule (CoPoint); the only
// vectors in memory are the operands and results of the network products, in the reference's concatenation order.
//
// Shares. ncomp = 1 for protocol 0 (plain / Shamir), 2 for Rep3 ({a, b} interleaved); value (i, c) of a share vector is v[i ncomp + c].
// x (+) v adds the public v on the component pub_comp (a for protocol 0 and Rep3 party 0, b for Rep3 party 1, none for party 2).
//
// k_co_ops: a streaming kernel of the honk_oink.hip kind -- grid-stride over flat value indices, 256 lanes, no LDS, tune "vec_max_blocks".
// k_co_fold: a workgroup of 256 lanes takes edges_wg kept edges at a time, lane t < 252 the point t / edges_wg of edge slot t % edges_wg
// (6 x 42, or 7 x 36 for Poseidon2), blockIdx.y the component; lanes sum over a grid-stride loop (tune "vec_max_blocks", at most
// CO_MAX_BLOCKS), the workgroup reduces one subrelation at a time through 8 KiB of LDS and its partial sums go to the stream's workspace;
// k_co_finish, one workgroup per (subrelation, point, component), adds the workgroups' partials and places the entry in the stage's
// output. Every addition is the exact modular one on canonical elements, so the words do not depend on how edges are dealt to lanes,
// workgroups or passes. No atomics.
#pragma once
#include "honk_relations.hpp"
#include "plonk_quot.hpp"

namespace csh {

constexpr int HC_POINTS = 7;         // MAX_PARTIAL_RELATION_LENGTH: points per kept edge in an operand vector
constexpr int CO_WG = 256;
constexpr int CO_MAX_SUB = 4;        // subrelations a pass of a fold stage reduces at once
constexpr int CO_MAX_BLOCKS = 1024;  // partial sums per output; chunks of the edge selection (one scan workgroup)

// ---- what a stage is --------------------------------------------------------------------------------------------------------------------
// One launch of a fold stage: its subrelations, each with its place (first element) and its length in the stage's output.
struct CoPass {
  int ns;
  int off[CO_MAX_SUB], len[CO_MAX_SUB];
};
// A stage as data. An operand stage writes out[q] operand vectors of 7 m ncomp values to its output q; a fold stage (passes > 0) reduces
// the subrelations of its passes over the kept edges into its accumulators. in / in2: the parts of the product vectors in front of it.
struct CoStage {
  uint64_t cols;        // the columns read, as a mask
  int shares;           // the columns below this one are shares (ncomp values per element), the others public
  int out[3], in, in2;  // operand vectors per output (0 = not written) and per input
  bool params, scaling;
  int passes;           // fold stages: launches over the kept edges (mem_finish: two, of three running sums each)
  CoPass pass[2];
  int points, edges_wg;  // 6 x 42 or 7 x 36 lanes of 256: a lane of a six-point stage never sees the point 6
  bool one_comp;         // the grid runs over one component whatever ncomp is (a half share: arith_r0 reads both components itself)
};
constexpr CoStage co_ops(int shares, uint64_t cols, int out0, int out1, int out2, int in, bool params) {
  return CoStage{cols, shares, {out0, out1, out2}, in, 0, params, false, 0, {CoPass{}, CoPass{}}, 0, 0, false};
}
constexpr CoStage co_fold(int shares, uint64_t cols, int in, int in2, bool params, int points, CoPass pass0, CoPass pass1 = CoPass{}, bool one_comp = false) {
  return CoStage{cols, shares, {0, 0, 0}, in, in2, params, true, pass1.ns ? 2 : 1, {pass0, pass1}, points, points == 7 ? 36 : 42, one_comp};
}
constexpr bool co_is_ops(const CoStage& d) { return d.out[0] || d.out[1] || d.out[2]; }
// elements per component of a fold stage's output (0 for an operand stage), and the components it has
constexpr int co_acc_elems(const CoStage& d) {
  int n = 0;
  for (int p = 0; p < d.passes; ++p)
    for (int s = 0; s < d.pass[p].ns; ++s)
      if (d.pass[p].off[s] + d.pass[p].len[s] > n) n = d.pass[p].off[s] + d.pass[p].len[s];
  return n;
}
constexpr uint32_t co_grid_comps(const CoStage& d, uint32_t ncomp) { return d.one_comp ? 1 : ncomp; }
// the stages of one call behind one check: the fold stage `a` and the operand stage `b` (lookup_mid), or two fold stages (arith)
constexpr CoStage co_union(CoStage a, const CoStage& b) {
  a.cols |= b.cols, a.params = a.params || b.params, a.scaling = a.scaling || b.scaling;
  if (b.in > a.in) a.in = b.in;
  if (b.in2 > a.in2) a.in2 = b.in2;
  for (int q = 0; q < 3; ++q)
    if (b.out[q] > a.out[q]) a.out[q] = b.out[q];
  return a;
}

// What one call is told; a family adds its constants.
template <class F, int COLS_>
struct CoArgs {
  using Field = F;
  const F* col[COLS_];       // shares (ncomp values per element) in front of the public columns
  const uint32_t* edge_idx;  // the kept e >> 1, ascending; NULL = every edge of the range
  const F* scaling;          // NULL = one
  size_t scaling_stride;
  size_t edge_begin, m;      // m = kept edges
  uint32_t ncomp;
  int pub_comp;              // -1 = none
  F one;                     // arkworks-Montgomery
  const F* in;               // the result of the network product in front of the stage
  const F* in2;              // and of the second one (ell_finish, mem_finish)
  F* out[3];
  CSH_HD size_t n7() const { return HC_POINTS * m; }
};

// v0 + k (v1 - v0), 0 <= k <= 6: Univariate::extend_from of a pair (univariate.rs:57-178), by the reference's running sum
template <class F>
CSH_HD F hc_lerp(const F& v0, const F& v1, int k) {
  const F d = F::sub(v1, v0);
  F r = v0;
#pragma unroll 1
  for (int i = 0; i < k; ++i) r = F::add(r, d);
  return r;
}

// Batch element t = 7 j + k of the columns, on the component `comp`.
template <class A>
struct CoPoint {
  using F = typename A::Field;
  const A& a;
  size_t e;  // the edge's first element
  int k;
  unsigned comp;
  CSH_HD CoPoint(const A& a_, size_t j, int k_, unsigned comp_)
      : a(a_), e(a_.edge_idx ? 2 * (size_t)a_.edge_idx[j] : a_.edge_begin + 2 * j), k(k_), comp(comp_) {}
  CSH_HD F pub(int c) const { return hc_lerp(a.col[c][e], a.col[c][e + 1], k); }
  CSH_HD F sh(int c, unsigned cc) const { return hc_lerp(a.col[c][e * a.ncomp + cc], a.col[c][(e + 1) * a.ncomp + cc], k); }
  CSH_HD F sh(int c) const { return sh(c, comp); }
  CSH_HD bool is_pub() const { return (int)comp == a.pub_comp; }
  CSH_HD F plus(const F& x, const F& v) const { return is_pub() ? F::add(x, v) : x; }  // x (+) v
  CSH_HD F sc() const { return a.scaling ? a.scaling[(e >> 1) * a.scaling_stride] : a.one; }
};

// ---- kernels ----------------------------------------------------------------------------------------------------------------------------
template <class FAM, class F, int STAGE>
__global__ __launch_bounds__(CO_WG) void k_co_ops(typename FAM::template Args<F> a) {
  const size_t values = a.n7() * a.ncomp;
  for (size_t u = blockIdx.x * (size_t)CO_WG + threadIdx.x; u < values; u += (size_t)gridDim.x * CO_WG) FAM::template ops_at<STAGE>(a, u);
}

// partial[((block * gridDim.y + comp) * NS + s) * POINTS + k]
template <class FAM, class F, int STAGE, int PASS>
__global__ __launch_bounds__(CO_WG) void k_co_fold(typename FAM::template Args<F> a, F* partial) {
  constexpr CoStage D = FAM::stage(STAGE);
  constexpr int NS = D.pass[PASS].ns, POINTS = D.points, EDGES_WG = D.edges_wg;
  static_assert(PASS < D.passes && NS <= CO_MAX_SUB && POINTS * EDGES_WG <= CO_WG, "one lane per point of an edge slot");
  __shared__ F sums[CO_WG];
  const int t = threadIdx.x, k = t / EDGES_WG, slot = t % EDGES_WG;
  const unsigned comp = blockIdx.y;
  F acc[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) acc[s] = F::zero();
  if (k < POINTS) {
#pragma unroll 1
    for (size_t j = blockIdx.x * (size_t)EDGES_WG + slot; j < a.m; j += (size_t)gridDim.x * EDGES_WG) {
      F term[NS];
      FAM::template terms_at<STAGE, PASS>(a, j, k, comp, term);
#pragma unroll
      for (int s = 0; s < NS; ++s) acc[s] = F::add(acc[s], term[s]);
    }
  }
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    if (s) __syncthreads();  // the sums of subrelation s - 1 have been read
    sums[t] = acc[s];
    __syncthreads();
    if (t < POINTS) {
      F sum = F::zero();
#pragma unroll 1
      for (int q = 0; q < EDGES_WG; ++q) sum = F::add(sum, sums[t * EDGES_WG + q]);
      partial[(((size_t)blockIdx.x * gridDim.y + comp) * NS + s) * POINTS + t] = sum;
    }
  }
}

template <class F>
struct CoFinish {
  const F* partial;
  F* out;
  uint32_t blocks, ncomp, ns, points;
  uint32_t off[CO_MAX_SUB], len[CO_MAX_SUB];
};
// blockIdx.x = (s * points + k) * ncomp + comp; entry (k, comp) of subrelation s, k < len[s], is out[(off[s] + k) ncomp + comp]
template <class F>
__global__ __launch_bounds__(CO_WG) void k_co_finish(CoFinish<F> f) {
  __shared__ F sums[CO_WG];
  const unsigned comp = blockIdx.x % f.ncomp, sk = blockIdx.x / f.ncomp, s = sk / f.points, k = sk % f.points;
  uint32_t off = 0, len = 0;
#pragma unroll
  for (int q = 0; q < CO_MAX_SUB; ++q)
    if (q == (int)s) off = f.off[q], len = f.len[q];
  if (k >= len) return;  // uniform over the workgroup
  F sum = F::zero();
  for (uint32_t b = threadIdx.x; b < f.blocks; b += CO_WG) sum = F::add(sum, f.partial[((size_t)b * f.ncomp + comp) * f.ns * f.points + sk]);
  sums[threadIdx.x] = sum;
  __syncthreads();
  for (int w = CO_WG / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sums[threadIdx.x] = F::add(sums[threadIdx.x], sums[threadIdx.x + w]);
    __syncthreads();
  }
  if (threadIdx.x == 0) f.out[((size_t)off + k) * f.ncomp + comp] = sums[0];
}

// ---- launchers --------------------------------------------------------------------------------------------------------------------------
struct CoCall {
  uint32_t protocol, party;
  const uint64_t* const* cols;
  size_t edge_begin, edge_end;
  const uint32_t* edge_idx;
  size_t m;
  const uint64_t* scaling;
  size_t scaling_stride;
  const uint64_t* params;
};
// the vectors of a stage: in / in2 = the products in front of it, out = its operand vectors, acc = its accumulators
struct CoIo {
  const uint64_t* in;
  const uint64_t* in2;
  uint64_t* out[3];
  uint64_t* acc;
};
template <class FAM, class F>
inline typename FAM::template Args<F> co_args(const CoCall& c, const CoIo& io, int stage) {
  typename FAM::template Args<F> a;
  const uint64_t colmask = FAM::stage(stage).cols;
  for (int k = 0; k < FAM::COLS; ++k) a.col[k] = ((colmask >> k) & 1) ? (const F*)c.cols[k] : nullptr;
  a.edge_idx = c.edge_idx, a.scaling = (const F*)c.scaling, a.scaling_stride = c.scaling_stride;
  a.edge_begin = c.edge_begin, a.m = c.m;
  a.ncomp = c.protocol + 1, a.pub_comp = pq_pub_comp(c.protocol, c.party);
  a.one = F::one();
  a.in = (const F*)io.in, a.in2 = (const F*)io.in2;
  for (int q = 0; q < 3; ++q) a.out[q] = (F*)io.out[q];
  FAM::consts(a, c);
  return a;
}
inline int co_max_blocks() {
  const int mb = tune().vec_max_blocks.load(std::memory_order_relaxed);
  return mb <= 0 || mb > CO_MAX_BLOCKS ? CO_MAX_BLOCKS : mb;
}
template <class FAM, int STAGE, class A>
inline int co_ops_stage(const A& a, hipStream_t st) {
  using F = typename A::Field;
  if (a.m) hipLaunchKernelGGL((k_co_ops<FAM, F, STAGE>), dim3(fr_stream_grid(a.n7() * a.ncomp, CO_WG)), dim3(CO_WG), 0, st, a);
  CSH_HIP(hipGetLastError());
  return CSH_OK;
}
// one pass of a fold stage: the launch over the kept edges and the finishing launch; `partial` holds blocks * comps * NS * POINTS elements
template <class FAM, int STAGE, int PASS, class A>
inline void co_fold_pass(const A& a, int blocks, typename A::Field* partial, typename A::Field* acc, hipStream_t st) {
  using F = typename A::Field;
  constexpr CoStage D = FAM::stage(STAGE);
  constexpr CoPass P = D.pass[PASS];
  const uint32_t comps = co_grid_comps(D, a.ncomp);
  if (blocks) hipLaunchKernelGGL((k_co_fold<FAM, F, STAGE, PASS>), dim3(blocks, comps), dim3(CO_WG), 0, st, a, partial);
  CoFinish<F> f{partial, acc, (uint32_t)blocks, comps, (uint32_t)P.ns, (uint32_t)D.points, {0, 0, 0, 0}, {0, 0, 0, 0}};
  for (int s = 0; s < P.ns; ++s) f.off[s] = P.off[s], f.len[s] = P.len[s];
  hipLaunchKernelGGL(k_co_finish<F>, dim3(P.ns * D.points * comps), dim3(CO_WG), 0, st, f);
}
// a fold stage with m = 0 writes zero accumulators: the finishing launch adds no partials
template <class FAM, int STAGE, class A>
inline int co_fold_stage(const A& a, uint64_t* acc, hipStream_t st) {
  using F = typename A::Field;
  constexpr CoStage D = FAM::stage(STAGE);
  static_assert(D.pass[1].ns <= D.pass[0].ns, "the first pass sizes the partial sums");
  const int blocks = a.m ? grid_for(a.m, D.edges_wg, co_max_blocks()) : 0;
  // the passes follow each other on the stream and share the partial sums' place
  const size_t elems = (size_t)blocks * co_grid_comps(D, a.ncomp) * D.pass[0].ns * D.points + 1;
  Arena& ar = arena_for(st);
  CSH_TRY(ar.reserve(Arena::padded(elems * sizeof(F))));
  F* partial = ar.take<F>(elems);
  co_fold_pass<FAM, STAGE, 0>(a, blocks, partial, (F*)acc, st);
  if constexpr (D.passes == 2) co_fold_pass<FAM, STAGE, 1>(a, blocks, partial, (F*)acc, st);
  CSH_HIP(hipGetLastError());
  return CSH_OK;
}

// ---- argument rules ---------------------------------------------------------------------------------------------------------------------
inline int co_null(const char* what) {
  set_error("%s: NULL argument", what);
  return CSH_ERR_INVALID;
}
inline int co_range_ok(size_t edge_begin, size_t edge_end, const char* what) {
  if (!(edge_begin % 2 == 0 && edge_end % 2 == 0 && edge_begin < edge_end && edge_end <= HR_MAX_EDGE_END)) {
    set_error("%s: edge_begin and edge_end must be even, edge_begin < edge_end <= 2^28", what);
    return CSH_ERR_INVALID;
  }
  return CSH_OK;
}
// The rules every stage shares, in this order: field, protocol and party, NULL arguments, the range, m, the stride. Adds what the stage
// reads and writes to `in` and `out`; the caller adds what is its own and checks the overlaps.
inline int co_check(csh_curve_t field_of, const CoStage& d, int ncols, const CoCall& c, const CoIo& io, const char* what, FrRanges& in,
                    FrRanges& out) {
  FR_REQUIRE_FIELD(field_of);
  if (c.protocol > 1 || c.party > 2) {
    set_error("%s: protocol must be 0 (plain / Shamir) or 1 (Rep3), party_id 0, 1 or 2", what);
    return CSH_ERR_INVALID;
  }
  const int acc_elems = co_acc_elems(d);
  bool ok = c.cols != nullptr && (c.params || !d.params) && (io.acc || !acc_elems);
  for (int k = 0; ok && k < ncols; ++k) ok = !((d.cols >> k) & 1) || c.cols[k] != nullptr;
  if (c.m) {
    ok = ok && (io.in || !d.in) && (io.in2 || !d.in2);
    for (int q = 0; q < 3; ++q) ok = ok && (io.out[q] || !d.out[q]);
  }
  if (!ok) return co_null(what);
  CSH_TRY(co_range_ok(c.edge_begin, c.edge_end, what));
  const size_t n_edges = (c.edge_end - c.edge_begin) / 2;
  if (c.edge_idx ? c.m > n_edges : c.m != n_edges) {
    set_error("%s: m must be the number of edges of the range, or with an edge list at most that", what);
    return CSH_ERR_INVALID;
  }
  if (d.scaling && c.scaling && !(c.scaling_stride >= 1 && c.scaling_stride <= HR_MAX_EDGE_END)) {
    set_error("%s: scaling_stride must be 1 .. 2^28", what);
    return CSH_ERR_INVALID;
  }
  const size_t ncomp = c.protocol + 1, seg = 32 * HC_POINTS * c.m * ncomp;
  for (int k = 0; k < ncols; ++k)
    if ((d.cols >> k) & 1) {
      const size_t eb = 32 * (k < d.shares ? ncomp : 1);
      in.add((const char*)c.cols[k] + eb * c.edge_begin, eb * (c.edge_end - c.edge_begin));
    }
  if (c.edge_idx && c.m) in.add(c.edge_idx, 4 * c.m);
  if (d.scaling && c.scaling) in.add((const char*)c.scaling + 32 * (c.edge_begin >> 1) * c.scaling_stride, 32 * (n_edges - 1) * c.scaling_stride + 32);
  if (c.m) {
    if (d.in) in.add(io.in, d.in * seg);
    if (d.in2) in.add(io.in2, d.in2 * seg);
    for (int q = 0; q < 3; ++q)
      if (d.out[q]) out.add(io.out[q], d.out[q] * seg);
  }
  if (acc_elems) out.add(io.acc, 32 * (size_t)acc_elems * co_grid_comps(d, (uint32_t)ncomp));
  return CSH_OK;
}
template <class FAM>
inline int co_check(csh_curve_t field_of, int stage, const CoCall& c, const CoIo& io, const char* what) {
  FrRanges in, out;
  CSH_TRY(co_check(field_of, FAM::stage(stage), FAM::COLS, c, io, what, in, out));
  return fr_check_ranges(in, out, what);
}
// An entry of one stage. An operand stage with m = 0 has nothing to write and asks for no device.
template <class FAM, int STAGE>
inline int co_entry(csh_curve_t field_of, const CoCall& c, const CoIo& io, const char* what, void* stream) {
  constexpr CoStage D = FAM::stage(STAGE);
  CSH_TRY(co_check<FAM>(field_of, STAGE, c, io, what));
  if (!D.passes && !c.m) return CSH_OK;
  CSH_TRY(ensure_device());
  hipStream_t st = resolve_stream(stream);
  if constexpr (D.passes != 0)
    return FR_CALL(field_of, co_fold_stage<FAM, STAGE>(co_args<FAM, F>(c, io, STAGE), io.acc, st));
  else
    return FR_CALL(field_of, co_ops_stage<FAM, STAGE>(co_args<FAM, F>(c, io, STAGE), st));
}

// ---- the host run of the self-tests: the loop bodies the kernels call, on host pointers, dealt to no lanes -------------------------------
template <class FAM, int STAGE, class A>
inline void co_host_stage(const A& a, uint64_t* acc_words) {
  using F = typename A::Field;
  constexpr CoStage D = FAM::stage(STAGE);
  if constexpr (D.passes != 0) {
    F* acc = (F*)acc_words;
    const uint32_t comps = co_grid_comps(D, a.ncomp);
    for (size_t i = 0; i < (size_t)co_acc_elems(D) * comps; ++i) acc[i] = F::zero();
    auto pass = [&](auto pass_tag) {
      constexpr int PASS = decltype(pass_tag)::value;
      constexpr CoPass P = D.pass[PASS];
      for (size_t j = 0; j < a.m; ++j)
        for (int k = 0; k < D.points; ++k)
          for (uint32_t comp = 0; comp < comps; ++comp) {
            F term[P.ns];
            FAM::template terms_at<STAGE, PASS>(a, j, k, comp, term);
            for (int s = 0; s < P.ns; ++s)
              if (k < P.len[s]) {
                F& o = acc[(size_t)(P.off[s] + k) * comps + comp];
                o = F::add(o, term[s]);
              }
          }
    };
    pass(std::integral_constant<int, 0>{});
    if constexpr (D.passes == 2) pass(std::integral_constant<int, 1>{});
  } else if constexpr (co_is_ops(D)) {
    for (size_t u = 0; u < a.n7() * a.ncomp; ++u) FAM::template ops_at<STAGE>(a, u);
  }
}
// stage (a run-time value) -> co_host_stage<STAGE>; false if the family has no such fold or operand stage
template <class FAM, class F, int STAGE = 0>
inline bool co_host_run(int stage, const CoCall& c, const CoIo& io) {
  if constexpr (STAGE < FAM::STAGES) {
    constexpr CoStage D = FAM::stage(STAGE);
    if (stage != STAGE) return co_host_run<FAM, F, STAGE + 1>(stage, c, io);
    if constexpr (D.passes != 0 || co_is_ops(D)) {
      co_host_stage<FAM, STAGE>(co_args<FAM, F>(c, io, STAGE), io.acc);
      return true;
    } else {
      return false;
    }
  } else {
    return false;
  }
}
// the outputs of a self-test entry in the order of the device entry: a fold stage's out0 is its accumulators
template <class FAM>
inline CoIo co_host_io(int stage, const uint64_t* in, const uint64_t* in2, uint64_t* out0, uint64_t* out1, uint64_t* out2) {
  const bool fold = FAM::stage(stage).passes != 0;
  return CoIo{in, in2, {fold ? nullptr : out0, out1, out2}, fold ? out0 : nullptr};
}

}  // namespace csh
