// The collaborative UltraHonk sumcheck round on shares, subrelations 11 .. 27: one device stage per stretch of local
// arithmetic between two network products of co-noir/co-ultrahonk/src/co_decider/relations/ for the elliptic, memory, non-native field,
// Poseidon2 external and Poseidon2 internal relations, and fold_accumulator! (relations/mod.rs:45-57) at the end of each. The network
// stays the caller's (csh_rep3_local_mul_vec_dev / csh_vec_mul_dev and its own exchange); the edges are selected by
// csh_honk_co_select_edges_dev on the relation's own selector. Expressions, the element rule and the operand layouts: honk_co_gates.hpp,
// shared with the host self-test.
//
// k_hgc_ops: a streaming kernel of the k_hc_ops kind -- grid-stride over flat value indices, 256 lanes, no LDS, tune "vec_max_blocks".
// k_hgc_fold: a workgroup of 256 lanes takes EDGES_WG kept edges at a time, lane t < 252 the point t / EDGES_WG of edge slot
// t % EDGES_WG (6 x 42, or 7 x 36 for Poseidon2), blockIdx.y the component; lanes sum over a grid-stride loop (tune "vec_max_blocks", at
// most HGC_MAX_BLOCKS), the workgroup reduces one subrelation at a time through 8 KiB of LDS and its partial sums go to the stream's
// workspace; k_hgc_finish, one workgroup per (subrelation, point, component), adds the workgroups' partials. Every addition is the exact
// modular one on canonical elements, so the words do not depend on how edges are dealt to lanes, workgroups or passes. No atomics.
// mem_finish folds its six subrelations in two launches of three running sums each (HgcFold): one launch of six needs 218 VGPRs, which
// leaves two waves per SIMD. profiles/honk_co_gates_kernel_meta.csv: no scratch, no VGPR spill.
#include "honk_co_gates.hpp"

namespace csh {

constexpr int HGC_WG = 256;
constexpr int HGC_MAX_BLOCKS = 1024;  // partial sums the finishing launch adds per output

template <class F, int STAGE>
__global__ __launch_bounds__(HGC_WG) void k_hgc_ops(HgcArgs<F> a) {
  const size_t values = a.n7() * a.ncomp;
  for (size_t u = blockIdx.x * (size_t)HGC_WG + threadIdx.x; u < values; u += (size_t)gridDim.x * HGC_WG) hgc_ops_at<STAGE>(a, u);
}

// partial[((block * gridDim.y + comp) * NS + s) * POINTS + k]
template <class F, int STAGE, int PASS>
__global__ __launch_bounds__(HGC_WG) void k_hgc_fold(HgcArgs<F> a, F* partial) {
  using FD = HgcFold<STAGE, PASS>;
  __shared__ F sums[HGC_WG];
  const int t = threadIdx.x, k = t / FD::EDGES_WG, slot = t % FD::EDGES_WG;
  const unsigned comp = blockIdx.y;
  F acc[FD::NS];
#pragma unroll
  for (int s = 0; s < FD::NS; ++s) acc[s] = F::zero();
  if (k < FD::POINTS) {
#pragma unroll 1
    for (size_t j = blockIdx.x * (size_t)FD::EDGES_WG + slot; j < a.m; j += (size_t)gridDim.x * FD::EDGES_WG) {
      F term[FD::NS];
      hgc_terms_at<STAGE, PASS>(a, j, k, comp, term);
#pragma unroll
      for (int s = 0; s < FD::NS; ++s) acc[s] = F::add(acc[s], term[s]);
    }
  }
#pragma unroll
  for (int s = 0; s < FD::NS; ++s) {
    if (s) __syncthreads();  // the sums of subrelation s - 1 have been read
    sums[t] = acc[s];
    __syncthreads();
    if (t < FD::POINTS) {
      F sum = F::zero();
#pragma unroll 1
      for (int q = 0; q < FD::EDGES_WG; ++q) sum = F::add(sum, sums[t * FD::EDGES_WG + q]);
      partial[(((size_t)blockIdx.x * gridDim.y + comp) * FD::NS + s) * FD::POINTS + t] = sum;
    }
  }
}

constexpr int HGC_MAX_NS = 4;
template <class F>
struct HgcFinish {
  const F* partial;
  F* out;
  uint32_t blocks, ncomp, ns, points;
  uint32_t sub[HGC_MAX_NS];  // the accumulator of the stage that subrelation s of the pass is
};
// blockIdx.x = (s * points + k) * ncomp + comp; entry (k, comp) of accumulator sub[s] is out[(sub[s] points + k) ncomp + comp]
template <class F>
__global__ __launch_bounds__(HGC_WG) void k_hgc_finish(HgcFinish<F> f) {
  __shared__ F sums[HGC_WG];
  const unsigned comp = blockIdx.x % f.ncomp, sk = blockIdx.x / f.ncomp, s = sk / f.points, k = sk % f.points;
  uint32_t sub = 0;
#pragma unroll
  for (int q = 0; q < HGC_MAX_NS; ++q)
    if (q == (int)s) sub = f.sub[q];
  F sum = F::zero();
  for (uint32_t b = threadIdx.x; b < f.blocks; b += HGC_WG) sum = F::add(sum, f.partial[((size_t)b * f.ncomp + comp) * f.ns * f.points + sk]);
  sums[threadIdx.x] = sum;
  __syncthreads();
  for (int w = HGC_WG / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sums[threadIdx.x] = F::add(sums[threadIdx.x], sums[threadIdx.x + w]);
    __syncthreads();
  }
  if (threadIdx.x == 0) f.out[((size_t)sub * f.points + k) * f.ncomp + comp] = sums[0];
}

// ---- launchers ------------------------------------------------------------------------------------------------------------------------------
struct HgcCall {
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
struct HgcIo {
  const uint64_t* in;
  const uint64_t* in2;
  uint64_t* out[3];
  uint64_t* acc;
};
template <class F>
static HgcArgs<F> hgc_args(const HgcCall& c, const HgcIo& io, int stage) {
  HgcArgs<F> a;
  const uint32_t colmask = hgc_cols_of(stage);
  for (int k = 0; k < HG_COLS; ++k) a.col[k] = ((colmask >> k) & 1) ? (const F*)c.cols[k] : nullptr;
  a.edge_idx = c.edge_idx, a.scaling = (const F*)c.scaling, a.scaling_stride = c.scaling_stride;
  a.edge_begin = c.edge_begin, a.m = c.m;
  a.ncomp = c.protocol + 1, a.pub_comp = pq_pub_comp(c.protocol, c.party);
  hgc_consts(a, c.params);
  a.in = (const F*)io.in, a.in2 = (const F*)io.in2;
  for (int q = 0; q < 3; ++q) a.out[q] = (F*)io.out[q];
  return a;
}
template <int STAGE, class F>
static int hgc_ops_stage(const HgcCall& c, const HgcIo& io, hipStream_t st) {
  const HgcArgs<F> a = hgc_args<F>(c, io, STAGE);
  if (c.m) hipLaunchKernelGGL((k_hgc_ops<F, STAGE>), dim3(fr_stream_grid(a.n7() * a.ncomp, HGC_WG)), dim3(HGC_WG), 0, st, a);
  CSH_HIP(hipGetLastError());
  return CSH_OK;
}
// one pass of a fold stage: the launch over the kept edges and the finishing launch; `partial` holds blocks * ncomp * NS * POINTS elements
template <int STAGE, int PASS, class F>
static void hgc_fold_pass(const HgcArgs<F>& a, int blocks, F* partial, F* out, hipStream_t st) {
  using FD = HgcFold<STAGE, PASS>;
  static_assert(FD::NS <= HGC_MAX_NS, "the finishing launch's table");
  if (blocks) hipLaunchKernelGGL((k_hgc_fold<F, STAGE, PASS>), dim3(blocks, a.ncomp), dim3(HGC_WG), 0, st, a, partial);
  HgcFinish<F> f{partial, out, (uint32_t)blocks, a.ncomp, FD::NS, FD::POINTS, {0, 0, 0, 0}};
  for (int s = 0; s < FD::NS; ++s) f.sub[s] = FD::sub(s);
  hipLaunchKernelGGL(k_hgc_finish<F>, dim3(FD::NS * FD::POINTS * a.ncomp), dim3(HGC_WG), 0, st, f);
}
template <int STAGE, class F>
static int hgc_fold_stage(const HgcCall& c, const HgcIo& io, hipStream_t st) {
  using FD = HgcFold<STAGE>;
  const HgcArgs<F> a = hgc_args<F>(c, io, STAGE);
  int mb = tune().vec_max_blocks.load(std::memory_order_relaxed);
  if (mb <= 0 || mb > HGC_MAX_BLOCKS) mb = HGC_MAX_BLOCKS;
  const int blocks = c.m ? grid_for(c.m, FD::EDGES_WG, mb) : 0;
  // the passes follow each other on the stream and share the partial sums' place
  const size_t elems = (size_t)blocks * a.ncomp * FD::NS * FD::POINTS + 1;
  Arena& ar = arena_for(st);
  CSH_TRY(ar.reserve(Arena::padded(elems * sizeof(F))));
  F* partial = ar.take<F>(elems);
  hgc_fold_pass<STAGE, 0>(a, blocks, partial, (F*)io.acc, st);
  if constexpr (FD::PASSES == 2) hgc_fold_pass<STAGE, 1>(a, blocks, partial, (F*)io.acc, st);
  CSH_HIP(hipGetLastError());
  return CSH_OK;
}

// ---- argument rules: those of the csh_honk_co_* section, over the 19 columns -------------------------------------------------------------
static bool hgc_uses_params(int stage) {
  return stage == HGC_ELL_OPS2 || stage == HGC_MEM_OPS || stage == HGC_MEM_FINISH || stage == HGC_POS_INT_FINISH;
}
static int hgc_check(csh_curve_t field_of, int stage, const HgcCall& c, const HgcIo& io, const char* what) {
  FR_REQUIRE_FIELD(field_of);
  if (c.protocol > 1 || c.party > 2) {
    set_error("%s: protocol must be 0 (plain / Shamir) or 1 (Rep3), party_id 0, 1 or 2", what);
    return CSH_ERR_INVALID;
  }
  const uint32_t colmask = hgc_cols_of(stage);
  const HgcParts parts = hgc_parts_of(stage);
  const int acc_elems = hgc_acc_elems_of(stage);
  bool ok = c.cols != nullptr && (c.params || !hgc_uses_params(stage)) && (io.acc || !acc_elems);
  for (int k = 0; ok && k < HG_COLS; ++k) ok = !((colmask >> k) & 1) || c.cols[k] != nullptr;
  if (c.m) {
    ok = ok && (io.in || !parts.in) && (io.in2 || !parts.in2);
    for (int q = 0; q < 3; ++q) ok = ok && (io.out[q] || !parts.out[q]);
  }
  if (!ok) {
    set_error("%s: NULL argument", what);
    return CSH_ERR_INVALID;
  }
  if (!(c.edge_begin % 2 == 0 && c.edge_end % 2 == 0 && c.edge_begin < c.edge_end && c.edge_end <= HR_MAX_EDGE_END)) {
    set_error("%s: edge_begin and edge_end must be even, edge_begin < edge_end <= 2^28", what);
    return CSH_ERR_INVALID;
  }
  const size_t n_edges = (c.edge_end - c.edge_begin) / 2;
  if (c.edge_idx ? c.m > n_edges : c.m != n_edges) {
    set_error("%s: m must be the number of edges of the range, or with an edge list at most that", what);
    return CSH_ERR_INVALID;
  }
  const bool uses_scaling = acc_elems != 0;
  if (uses_scaling && c.scaling && !(c.scaling_stride >= 1 && c.scaling_stride <= HR_MAX_EDGE_END)) {
    set_error("%s: scaling_stride must be 1 .. 2^28", what);
    return CSH_ERR_INVALID;
  }
  const size_t ncomp = c.protocol + 1, seg = 32 * HC_POINTS * c.m * ncomp;
  FrRanges in, out;
  for (int k = 0; k < HG_COLS; ++k)
    if ((colmask >> k) & 1) {
      const size_t eb = 32 * (k < HG_Q_M ? ncomp : 1);
      in.add((const char*)c.cols[k] + eb * c.edge_begin, eb * (c.edge_end - c.edge_begin));
    }
  if (c.edge_idx && c.m) in.add(c.edge_idx, 4 * c.m);
  if (uses_scaling && c.scaling) in.add((const char*)c.scaling + 32 * (c.edge_begin >> 1) * c.scaling_stride, 32 * (n_edges - 1) * c.scaling_stride + 32);
  if (c.m) {
    if (parts.in) in.add(io.in, parts.in * seg);
    if (parts.in2) in.add(io.in2, parts.in2 * seg);
    for (int q = 0; q < 3; ++q)
      if (parts.out[q]) out.add(io.out[q], parts.out[q] * seg);
  }
  if (acc_elems) out.add(io.acc, 32 * acc_elems * ncomp);
  return fr_check_ranges(in, out, what);
}
template <int STAGE>
static int hgc_entry(csh_curve_t field_of, const HgcCall& c, const HgcIo& io, const char* what, void* stream) {
  CSH_TRY(hgc_check(field_of, STAGE, c, io, what));
  constexpr bool fold = STAGE == HGC_ELL_FINISH || STAGE == HGC_MEM_FINISH || STAGE == HGC_NNF_FINISH || STAGE == HGC_POS_EXT_FINISH ||
                        STAGE == HGC_POS_INT_FINISH;
  if (!fold && !c.m) return CSH_OK;
  CSH_TRY(ensure_device());
  hipStream_t st = resolve_stream(stream);
  if constexpr (fold)
    return FR_CALL(field_of, hgc_fold_stage<STAGE, F>(c, io, st));
  else
    return FR_CALL(field_of, hgc_ops_stage<STAGE, F>(c, io, st));
}

}  // namespace csh

using namespace csh;

#define HGC_COMMON_PARAMS                                                                                                                    \
  csh_curve_t field_of, uint32_t protocol, uint32_t party_id, const uint64_t *const *cols_dev, size_t edge_begin, size_t edge_end,          \
      const uint32_t *edge_idx_dev, size_t m
#define HGC_CALL(scaling, stride, params) \
  HgcCall { protocol, party_id, cols_dev, edge_begin, edge_end, edge_idx_dev, m, scaling, stride, params }

extern "C" {

int csh_honk_co_ell_operands_dev(HGC_COMMON_PARAMS, uint64_t* lhs_dev, uint64_t* rhs_dev, void* stream) {
  return hgc_entry<HGC_ELL_OPS>(field_of, HGC_CALL(nullptr, 1, nullptr), HgcIo{nullptr, nullptr, {lhs_dev, rhs_dev, nullptr}, nullptr},
                                "honk_co_ell_operands", stream);
}
int csh_honk_co_ell_operands2_dev(HGC_COMMON_PARAMS, const uint64_t* params, const uint64_t* mul1_dev, uint64_t* lhs_dev, uint64_t* rhs_dev,
                                  void* stream) {
  return hgc_entry<HGC_ELL_OPS2>(field_of, HGC_CALL(nullptr, 1, params), HgcIo{mul1_dev, nullptr, {lhs_dev, rhs_dev, nullptr}, nullptr},
                                 "honk_co_ell_operands2", stream);
}
int csh_honk_co_ell_finish_dev(HGC_COMMON_PARAMS, const uint64_t* scaling_dev, size_t scaling_stride, const uint64_t* mul1_dev,
                               const uint64_t* mul2_dev, uint64_t* acc_dev, void* stream) {
  return hgc_entry<HGC_ELL_FINISH>(field_of, HGC_CALL(scaling_dev, scaling_stride, nullptr),
                                   HgcIo{mul1_dev, mul2_dev, {nullptr, nullptr, nullptr}, acc_dev}, "honk_co_ell_finish", stream);
}
int csh_honk_co_mem_operands_dev(HGC_COMMON_PARAMS, const uint64_t* params, uint64_t* lhs_dev, uint64_t* rhs_dev, uint64_t* rhs2_dev,
                                 void* stream) {
  return hgc_entry<HGC_MEM_OPS>(field_of, HGC_CALL(nullptr, 1, params), HgcIo{nullptr, nullptr, {lhs_dev, rhs_dev, rhs2_dev}, nullptr},
                                "honk_co_mem_operands", stream);
}
int csh_honk_co_mem_finish_dev(HGC_COMMON_PARAMS, const uint64_t* scaling_dev, size_t scaling_stride, const uint64_t* params,
                               const uint64_t* mul_dev, const uint64_t* mul2_dev, uint64_t* acc_dev, void* stream) {
  return hgc_entry<HGC_MEM_FINISH>(field_of, HGC_CALL(scaling_dev, scaling_stride, params),
                                   HgcIo{mul_dev, mul2_dev, {nullptr, nullptr, nullptr}, acc_dev}, "honk_co_mem_finish", stream);
}
int csh_honk_co_nnf_operands_dev(HGC_COMMON_PARAMS, uint64_t* lhs_dev, uint64_t* rhs_dev, void* stream) {
  return hgc_entry<HGC_NNF_OPS>(field_of, HGC_CALL(nullptr, 1, nullptr), HgcIo{nullptr, nullptr, {lhs_dev, rhs_dev, nullptr}, nullptr},
                                "honk_co_nnf_operands", stream);
}
int csh_honk_co_nnf_finish_dev(HGC_COMMON_PARAMS, const uint64_t* scaling_dev, size_t scaling_stride, const uint64_t* mul_dev, uint64_t* acc_dev,
                               void* stream) {
  return hgc_entry<HGC_NNF_FINISH>(field_of, HGC_CALL(scaling_dev, scaling_stride, nullptr),
                                   HgcIo{mul_dev, nullptr, {nullptr, nullptr, nullptr}, acc_dev}, "honk_co_nnf_finish", stream);
}
int csh_honk_co_pos_ext_operands_dev(HGC_COMMON_PARAMS, uint64_t* s_dev, void* stream) {
  return hgc_entry<HGC_POS_EXT_OPS>(field_of, HGC_CALL(nullptr, 1, nullptr), HgcIo{nullptr, nullptr, {s_dev, nullptr, nullptr}, nullptr},
                                    "honk_co_pos_ext_operands", stream);
}
int csh_honk_co_pos_ext_finish_dev(HGC_COMMON_PARAMS, const uint64_t* scaling_dev, size_t scaling_stride, const uint64_t* u_dev, uint64_t* acc_dev,
                                   void* stream) {
  return hgc_entry<HGC_POS_EXT_FINISH>(field_of, HGC_CALL(scaling_dev, scaling_stride, nullptr),
                                       HgcIo{u_dev, nullptr, {nullptr, nullptr, nullptr}, acc_dev}, "honk_co_pos_ext_finish", stream);
}
int csh_honk_co_pos_int_operands_dev(HGC_COMMON_PARAMS, uint64_t* s1_dev, void* stream) {
  return hgc_entry<HGC_POS_INT_OPS>(field_of, HGC_CALL(nullptr, 1, nullptr), HgcIo{nullptr, nullptr, {s1_dev, nullptr, nullptr}, nullptr},
                                    "honk_co_pos_int_operands", stream);
}
int csh_honk_co_pos_int_finish_dev(HGC_COMMON_PARAMS, const uint64_t* scaling_dev, size_t scaling_stride, const uint64_t* params,
                                   const uint64_t* u1_dev, uint64_t* acc_dev, void* stream) {
  return hgc_entry<HGC_POS_INT_FINISH>(field_of, HGC_CALL(scaling_dev, scaling_stride, params),
                                       HgcIo{u1_dev, nullptr, {nullptr, nullptr, nullptr}, acc_dev}, "honk_co_pos_int_finish", stream);
}

}  // extern "C"

// Host run of the stage functions of honk_co_gates.hpp on host pointers: the loop bodies the kernels call, dealt to no lanes. `stage` is an
// HgcStage; in / in2 are the stage's product vectors, out0 .. out2 its outputs in the order of the device entry (a fold stage: out0 = the
// accumulators).
template <int STAGE, int PASS, class F>
static void hgc_host_fold(const HgcArgs<F>& a, F* acc) {
  using FD = HgcFold<STAGE, PASS>;
  for (int s = 0; s < FD::NS; ++s)
    for (int i = 0; i < FD::POINTS * (int)a.ncomp; ++i) acc[(size_t)FD::sub(s) * FD::POINTS * a.ncomp + i] = F::zero();
  for (size_t j = 0; j < a.m; ++j)
    for (int k = 0; k < FD::POINTS; ++k)
      for (uint32_t comp = 0; comp < a.ncomp; ++comp) {
        F term[FD::NS];
        hgc_terms_at<STAGE, PASS>(a, j, k, comp, term);
        for (int s = 0; s < FD::NS; ++s) {
          F& o = acc[(size_t)(FD::sub(s) * FD::POINTS + k) * a.ncomp + comp];
          o = F::add(o, term[s]);
        }
      }
}
template <int STAGE, class F>
static void hgc_host_stage(const HgcCall& c, const HgcIo& io) {
  const HgcArgs<F> a = hgc_args<F>(c, io, STAGE);
  if constexpr (STAGE == HGC_ELL_FINISH || STAGE == HGC_MEM_FINISH || STAGE == HGC_NNF_FINISH || STAGE == HGC_POS_EXT_FINISH ||
                STAGE == HGC_POS_INT_FINISH) {
    hgc_host_fold<STAGE, 0>(a, (F*)io.acc);
    if constexpr (HgcFold<STAGE>::PASSES == 2) hgc_host_fold<STAGE, 1>(a, (F*)io.acc);
  } else {
    for (size_t u = 0; u < a.n7() * a.ncomp; ++u) hgc_ops_at<STAGE>(a, u);
  }
}
template <class F>
static int hgc_host_t(int stage, const HgcCall& c, const HgcIo& io) {
  switch (stage) {
    case HGC_ELL_OPS: hgc_host_stage<HGC_ELL_OPS, F>(c, io); break;
    case HGC_ELL_OPS2: hgc_host_stage<HGC_ELL_OPS2, F>(c, io); break;
    case HGC_ELL_FINISH: hgc_host_stage<HGC_ELL_FINISH, F>(c, io); break;
    case HGC_MEM_OPS: hgc_host_stage<HGC_MEM_OPS, F>(c, io); break;
    case HGC_MEM_FINISH: hgc_host_stage<HGC_MEM_FINISH, F>(c, io); break;
    case HGC_NNF_OPS: hgc_host_stage<HGC_NNF_OPS, F>(c, io); break;
    case HGC_NNF_FINISH: hgc_host_stage<HGC_NNF_FINISH, F>(c, io); break;
    case HGC_POS_EXT_OPS: hgc_host_stage<HGC_POS_EXT_OPS, F>(c, io); break;
    case HGC_POS_EXT_FINISH: hgc_host_stage<HGC_POS_EXT_FINISH, F>(c, io); break;
    case HGC_POS_INT_OPS: hgc_host_stage<HGC_POS_INT_OPS, F>(c, io); break;
    case HGC_POS_INT_FINISH: hgc_host_stage<HGC_POS_INT_FINISH, F>(c, io); break;
    default: return CSH_ERR_INVALID;
  }
  return CSH_OK;
}

extern "C" {

int csh_selftest_honk_co_gates_host(int field_of, int stage, uint32_t protocol, uint32_t party_id, const uint64_t* const* cols, size_t edge_begin,
                                    size_t edge_end, const uint32_t* edge_idx, size_t m, const uint64_t* scaling, size_t scaling_stride,
                                    const uint64_t* params, const uint64_t* in, const uint64_t* in2, uint64_t* out0, uint64_t* out1,
                                    uint64_t* out2) {
  CSH_REQUIRE(stage >= 0 && stage < HGC_STAGES, "selftest_honk_co_gates: unknown stage");
  const HgcCall c{protocol, party_id, cols, edge_begin, edge_end, edge_idx, m, scaling, scaling_stride, params};
  const bool fold = hgc_acc_elems_of(stage) != 0;
  const HgcIo io{in, in2, {fold ? nullptr : out0, out1, out2}, fold ? out0 : nullptr};
  CSH_TRY(hgc_check((csh_curve_t)field_of, stage, c, io, "selftest_honk_co_gates"));
  return FR_CALL(field_of, hgc_host_t<F>(stage, c, io));
}

}  // extern "C"
