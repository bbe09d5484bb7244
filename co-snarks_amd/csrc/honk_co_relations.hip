// The sumcheck round of the collaborative UltraHonk prover on shares: one device stage per stretch of local arithmetic
// between two network rounds of co-noir/co-ultrahonk/src/co_decider/relations/ for the arithmetic, permutation, delta-range and
// log-derivative lookup relations, the edge selection of `can_skip`, and fold_accumulator! (relations/mod.rs:45-57). The network stays the
// caller's: a product between two stages is csh_rep3_local_mul_vec_dev + reshare (Rep3) or csh_vec_mul_dev + degree reduction (Shamir).
// Expressions and operand layouts: honk_co_relations.hpp; the kernels, the launchers and the argument rules of a stage:
// honk_co_stage.hpp. Here: the entries, of which four are not one stage each (arith, lookup_mid, delta_sub_one, select_edges), and
// k_hc_sub_one: a streaming kernel of the k_co_ops kind over the 8 * 7 m ncomp values of the squares.
// k_hc_sel_count / k_hc_sel_scan / k_hc_sel_write: a stable compaction -- every workgroup owns a contiguous chunk of the edges, counts its
// kept edges, one workgroup scans the counts, and every workgroup writes its chunk in order behind its offset.
#include "honk_co_relations.hpp"

namespace csh {

template <class F>
__global__ __launch_bounds__(CO_WG) void k_hc_sub_one(HcArgs<F> a) {
  const size_t values = 8 * a.n7() * a.ncomp;
  for (size_t u = blockIdx.x * (size_t)CO_WG + threadIdx.x; u < values; u += (size_t)gridDim.x * CO_WG) hc_sub_one_at(a, u);
}

// ---- edge selection -------------------------------------------------------------------------------------------------------------------------
// workgroup b owns the edges [b chunk, min((b + 1) chunk, n_edges))
template <class F>
__global__ __launch_bounds__(CO_WG) void k_hc_sel_count(const F* q, size_t edge_begin, size_t n_edges, size_t chunk, uint32_t* counts) {
  __shared__ uint32_t part[CO_WG];
  const size_t lo = blockIdx.x * chunk, hi = lo + chunk < n_edges ? lo + chunk : n_edges;
  uint32_t c = 0;
  for (size_t i = lo + threadIdx.x; i < hi; i += CO_WG) c += hc_keep(q, edge_begin + 2 * i) ? 1u : 0u;
  part[threadIdx.x] = c;
  __syncthreads();
  for (int w = CO_WG / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) counts[blockIdx.x] = part[0];
}
// one workgroup of CO_MAX_BLOCKS lanes: offsets[b] = the kept edges in front of chunk b, *total = all of them
__global__ __launch_bounds__(CO_MAX_BLOCKS) void k_hc_sel_scan(const uint32_t* counts, uint32_t blocks, uint32_t* offsets, uint32_t* total) {
  __shared__ uint32_t s[CO_MAX_BLOCKS];
  const uint32_t t = threadIdx.x, own = t < blocks ? counts[t] : 0u;
  s[t] = own;
  __syncthreads();
  for (uint32_t d = 1; d < CO_MAX_BLOCKS; d <<= 1) {
    const uint32_t v = t >= d ? s[t - d] : 0u;
    __syncthreads();
    s[t] += v;
    __syncthreads();
  }
  if (t < blocks) offsets[t] = s[t] - own;
  if (t == CO_MAX_BLOCKS - 1) *total = s[t];
}
template <class F>
__global__ __launch_bounds__(CO_WG) void k_hc_sel_write(const F* q, size_t edge_begin, size_t n_edges, size_t chunk, const uint32_t* offsets,
                                                        uint32_t* out) {
  __shared__ uint32_t wave_total[CO_WG / 64];
  const size_t lo = blockIdx.x * chunk, hi = lo + chunk < n_edges ? lo + chunk : n_edges;
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  size_t base = offsets[blockIdx.x];
#pragma unroll 1
  for (size_t tile = lo; tile < hi; tile += CO_WG) {  // uniform over the workgroup
    const size_t i = tile + threadIdx.x;
    const bool keep = i < hi && hc_keep(q, edge_begin + 2 * i);
    const unsigned long long ballot = __ballot(keep);
    const uint32_t before = (uint32_t)__popcll(ballot & ((1ull << lane) - 1ull));
    if (lane == 0) wave_total[wave] = (uint32_t)__popcll(ballot);
    __syncthreads();
    uint32_t in_front = 0, all = 0;
#pragma unroll
    for (unsigned w = 0; w < CO_WG / 64; ++w) {
      in_front += w < wave ? wave_total[w] : 0u;
      all += wave_total[w];
    }
    if (keep) out[base + in_front + before] = (uint32_t)((edge_begin >> 1) + i);
    base += all;
    __syncthreads();  // wave_total is rewritten by the next tile
  }
}

// ---- launchers ------------------------------------------------------------------------------------------------------------------------------
// two fold stages with an output each; arith_r0 is a half share
template <class F>
static int hc_arith_t(const CoCall& c, const uint64_t* mask, uint64_t* r0, uint64_t* r1, hipStream_t st) {
  HcArgs<F> a0 = co_args<HcFamily, F>(c, CoIo{}, HC_ARITH_R0);
  a0.mask = (const F*)mask;
  CSH_TRY((co_fold_stage<HcFamily, HC_ARITH_R0>(a0, r0, st)));
  return co_fold_stage<HcFamily, HC_ARITH_R1>(co_args<HcFamily, F>(c, CoIo{}, HC_ARITH_R1), r1, st);
}
template <class F>
static HcArgs<F> hc_sub_one_args(uint32_t protocol, uint32_t party, uint64_t* sqr, size_t m) {
  return co_args<HcFamily, F>(CoCall{protocol, party, nullptr, 0, 0, nullptr, m, nullptr, 1, nullptr}, CoIo{nullptr, nullptr, {sqr, nullptr, nullptr}, nullptr},
                              HC_DELTA_SUB_ONE);
}
template <class F>
static int hc_delta_sub_one_t(uint32_t protocol, uint32_t party, uint64_t* sqr, size_t m, hipStream_t st) {
  const HcArgs<F> a = hc_sub_one_args<F>(protocol, party, sqr, m);
  if (m && a.pub_comp >= 0) hipLaunchKernelGGL(k_hc_sub_one<F>, dim3(fr_stream_grid(8 * a.n7() * a.ncomp, CO_WG)), dim3(CO_WG), 0, st, a);
  CSH_HIP(hipGetLastError());
  return CSH_OK;
}
template <class F>
static int hc_select_t(const uint64_t* q, size_t edge_begin, size_t edge_end, uint32_t* out, uint32_t* count, hipStream_t st) {
  const size_t n_edges = (edge_end - edge_begin) / 2;
  const int blocks = grid_for(n_edges, CO_WG, co_max_blocks());
  const size_t chunk = (n_edges + blocks - 1) / blocks;
  Arena& ar = arena_for(st);
  CSH_TRY(ar.reserve(2 * Arena::padded((size_t)blocks * 4)));
  uint32_t* counts = ar.take<uint32_t>(blocks);
  uint32_t* offsets = ar.take<uint32_t>(blocks);
  hipLaunchKernelGGL(k_hc_sel_count<F>, dim3(blocks), dim3(CO_WG), 0, st, (const F*)q, edge_begin, n_edges, chunk, counts);
  hipLaunchKernelGGL(k_hc_sel_scan, dim3(1), dim3(CO_MAX_BLOCKS), 0, st, (const uint32_t*)counts, (uint32_t)blocks, offsets, count);
  hipLaunchKernelGGL(k_hc_sel_write<F>, dim3(blocks), dim3(CO_WG), 0, st, (const F*)q, edge_begin, n_edges, chunk, (const uint32_t*)offsets, out);
  CSH_HIP(hipGetLastError());
  return CSH_OK;
}

}  // namespace csh

using namespace csh;

#define HC_COMMON_PARAMS                                                                                                                     \
  csh_curve_t field_of, uint32_t protocol, uint32_t party_id, const uint64_t *const *cols_dev, size_t edge_begin, size_t edge_end,          \
      const uint32_t *edge_idx_dev, size_t m
#define HC_CALL(scaling, stride, params) \
  CoCall { protocol, party_id, cols_dev, edge_begin, edge_end, edge_idx_dev, m, scaling, stride, params }

extern "C" {

int csh_honk_co_select_edges_dev(csh_curve_t field_of, const uint64_t* selector_dev, size_t edge_begin, size_t edge_end, uint32_t* edge_idx_dev,
                                 uint32_t* count_dev, void* stream) {
  const char* what = "honk_co_select_edges";
  FR_REQUIRE_FIELD(field_of);
  if (!(selector_dev && edge_idx_dev && count_dev)) return co_null(what);
  CSH_TRY(co_range_ok(edge_begin, edge_end, what));
  FrRanges in, out;
  in.add((const char*)selector_dev + 32 * edge_begin, 32 * (edge_end - edge_begin));
  out.add(edge_idx_dev, 4 * ((edge_end - edge_begin) / 2));
  out.add(count_dev, 4);
  CSH_TRY(fr_check_ranges(in, out, what));
  CSH_TRY(ensure_device());
  hipStream_t st = resolve_stream(stream);
  return FR_CALL(field_of, hc_select_t<F>(selector_dev, edge_begin, edge_end, edge_idx_dev, count_dev, st));
}

int csh_honk_co_arith_dev(HC_COMMON_PARAMS, const uint64_t* scaling_dev, size_t scaling_stride, const uint64_t* mask_dev, uint64_t* r0_dev,
                          uint64_t* r1_dev, void* stream) {
  const char* what = "honk_co_arith";
  const CoCall c = HC_CALL(scaling_dev, scaling_stride, nullptr);
  constexpr CoStage R0 = hc_stage(HC_ARITH_R0), R1 = hc_stage(HC_ARITH_R1);
  // the rules of arith_r1 over both stages' columns; r0 and the mask are this entry's own
  FrRanges in, out;
  CSH_TRY(co_check(field_of, co_union(R1, R0), HR_COLS, c, CoIo{nullptr, nullptr, {nullptr, nullptr, nullptr}, r1_dev}, what, in, out));
  if (!r0_dev) return co_null(what);
  if (protocol == 1 ? (m && !mask_dev) : mask_dev != nullptr) {
    set_error("%s: the mask vector is required for Rep3 and must be NULL for protocol 0", what);
    return CSH_ERR_INVALID;
  }
  if (mask_dev && m) in.add(mask_dev, 32 * HC_POINTS * m);
  out.add(r0_dev, 32 * co_acc_elems(R0) * co_grid_comps(R0, protocol + 1));
  CSH_TRY(fr_check_ranges(in, out, what));
  CSH_TRY(ensure_device());
  hipStream_t st = resolve_stream(stream);
  return FR_CALL(field_of, hc_arith_t<F>(c, mask_dev, r0_dev, r1_dev, st));
}

int csh_honk_co_perm_operands_dev(HC_COMMON_PARAMS, const uint64_t* params, uint64_t* lhs_dev, uint64_t* rhs_dev, void* stream) {
  return co_entry<HcFamily, HC_PERM_OPS>(field_of, HC_CALL(nullptr, 1, params), CoIo{nullptr, nullptr, {lhs_dev, rhs_dev, nullptr}, nullptr},
                                         "honk_co_perm_operands", stream);
}
int csh_honk_co_perm_operands2_dev(HC_COMMON_PARAMS, const uint64_t* params, uint64_t* rhs_dev, void* stream) {
  return co_entry<HcFamily, HC_PERM_OPS2>(field_of, HC_CALL(nullptr, 1, params), CoIo{nullptr, nullptr, {rhs_dev, nullptr, nullptr}, nullptr},
                                          "honk_co_perm_operands2", stream);
}
int csh_honk_co_perm_finish_dev(HC_COMMON_PARAMS, const uint64_t* scaling_dev, size_t scaling_stride, const uint64_t* prod_dev, uint64_t* acc_dev,
                                void* stream) {
  return co_entry<HcFamily, HC_PERM_FINISH>(field_of, HC_CALL(scaling_dev, scaling_stride, nullptr),
                                            CoIo{prod_dev, nullptr, {nullptr, nullptr, nullptr}, acc_dev}, "honk_co_perm_finish", stream);
}
int csh_honk_co_delta_operands_dev(HC_COMMON_PARAMS, uint64_t* lhs_dev, void* stream) {
  return co_entry<HcFamily, HC_DELTA_OPS>(field_of, HC_CALL(nullptr, 1, nullptr), CoIo{nullptr, nullptr, {lhs_dev, nullptr, nullptr}, nullptr},
                                          "honk_co_delta_operands", stream);
}

// no columns: 8 * 7 m ncomp values in place, and no launch where the party holds no public component
int csh_honk_co_delta_sub_one_dev(csh_curve_t field_of, uint32_t protocol, uint32_t party_id, uint64_t* sqr_dev, size_t m, void* stream) {
  FR_REQUIRE_FIELD(field_of);
  CSH_REQUIRE(protocol <= 1 && party_id <= 2, "honk_co_delta_sub_one: protocol must be 0 (plain / Shamir) or 1 (Rep3), party_id 0, 1 or 2");
  CSH_REQUIRE(m <= HR_MAX_EDGE_END / 2, "honk_co_delta_sub_one: m must be at most 2^27");
  if (!sqr_dev && m) return co_null("honk_co_delta_sub_one");
  if (!m) return CSH_OK;
  CSH_TRY(ensure_device());
  hipStream_t st = resolve_stream(stream);
  return FR_CALL(field_of, hc_delta_sub_one_t<F>(protocol, party_id, sqr_dev, m, st));
}

int csh_honk_co_delta_finish_dev(HC_COMMON_PARAMS, const uint64_t* scaling_dev, size_t scaling_stride, const uint64_t* mul_dev, uint64_t* acc_dev,
                                 void* stream) {
  return co_entry<HcFamily, HC_DELTA_FINISH>(field_of, HC_CALL(scaling_dev, scaling_stride, nullptr),
                                             CoIo{mul_dev, nullptr, {nullptr, nullptr, nullptr}, acc_dev}, "honk_co_delta_finish", stream);
}
int csh_honk_co_lookup_operands_dev(HC_COMMON_PARAMS, const uint64_t* params, uint64_t* read_term_dev, uint64_t* inverses_dev, void* stream) {
  return co_entry<HcFamily, HC_LOOKUP_OPS>(field_of, HC_CALL(nullptr, 1, params),
                                           CoIo{nullptr, nullptr, {read_term_dev, inverses_dev, nullptr}, nullptr}, "honk_co_lookup_operands", stream);
}

// a fold stage and an operand stage behind one check
int csh_honk_co_lookup_mid_dev(HC_COMMON_PARAMS, const uint64_t* scaling_dev, size_t scaling_stride, const uint64_t* params,
                               const uint64_t* write_inverse_dev, uint64_t* r0_dev, uint64_t* lhs_dev, uint64_t* rhs_dev, void* stream) {
  const char* what = "honk_co_lookup_mid";
  const CoCall c = HC_CALL(scaling_dev, scaling_stride, params);
  const CoIo io{write_inverse_dev, nullptr, {nullptr, lhs_dev, rhs_dev}, r0_dev};
  FrRanges in, out;
  CSH_TRY(co_check(field_of, co_union(hc_stage(HC_LOOKUP_MID_R0), hc_stage(HC_LOOKUP_MID_OPS)), HR_COLS, c, io, what, in, out));
  CSH_TRY(fr_check_ranges(in, out, what));
  CSH_TRY(ensure_device());
  hipStream_t st = resolve_stream(stream);
  CSH_TRY(FR_CALL(field_of, co_fold_stage<HcFamily, HC_LOOKUP_MID_R0>(co_args<HcFamily, F>(c, io, HC_LOOKUP_MID_R0), r0_dev, st)));
  return FR_CALL(field_of, co_ops_stage<HcFamily, HC_LOOKUP_MID_OPS>(co_args<HcFamily, F>(c, io, HC_LOOKUP_MID_OPS), st));
}

int csh_honk_co_lookup_finish_dev(HC_COMMON_PARAMS, const uint64_t* scaling_dev, size_t scaling_stride, const uint64_t* params,
                                  const uint64_t* mul_dev, uint64_t* acc_dev, void* stream) {
  return co_entry<HcFamily, HC_LOOKUP_FINISH>(field_of, HC_CALL(scaling_dev, scaling_stride, params),
                                              CoIo{mul_dev, nullptr, {nullptr, nullptr, nullptr}, acc_dev}, "honk_co_lookup_finish", stream);
}

}  // extern "C"

// Host run of the stage functions of honk_co_relations.hpp on host pointers (co_host_run). `stage` is an HcStage; `in` is the stage's input
// vector (HC_SELECT: the selector column; HC_DELTA_SUB_ONE: none, out0 is updated in place), out0 .. out2 its outputs in the order of the
// device entry (HC_SELECT: out0 = the uint32_t list, out1 = the count word). The three stages that are not the framework's are run here.
template <class F>
static int hc_host_t(int stage, const CoCall& c, const uint64_t* in, const uint64_t* mask, uint64_t* o0, uint64_t* o1, uint64_t* o2) {
  if (stage == HC_SELECT) {
    uint32_t n = 0;
    for (size_t e = c.edge_begin; e < c.edge_end; e += 2)
      if (hc_keep((const F*)in, e)) ((uint32_t*)o0)[n++] = (uint32_t)(e >> 1);
    *(uint32_t*)o1 = n;
  } else if (stage == HC_DELTA_SUB_ONE) {
    const HcArgs<F> a = hc_sub_one_args<F>(c.protocol, c.party, o0, c.m);
    for (size_t u = 0; u < 8 * a.n7() * a.ncomp; ++u) hc_sub_one_at(a, u);
  } else if (stage == HC_ARITH_R0) {
    HcArgs<F> a = co_args<HcFamily, F>(c, CoIo{}, HC_ARITH_R0);
    a.mask = (const F*)mask;
    co_host_stage<HcFamily, HC_ARITH_R0>(a, o0);
  } else if (!co_host_run<HcFamily, F>(stage, c, co_host_io<HcFamily>(stage, in, nullptr, o0, o1, o2))) {
    set_error("selftest_honk_co_relations: unknown stage %d", stage);
    return CSH_ERR_INVALID;
  }
  return CSH_OK;
}

extern "C" {

int csh_selftest_honk_co_relations_host(int field_of, int stage, uint32_t protocol, uint32_t party_id, const uint64_t* const* cols, size_t edge_begin,
                                        size_t edge_end, const uint32_t* edge_idx, size_t m, const uint64_t* scaling, size_t scaling_stride,
                                        const uint64_t* params, const uint64_t* in, const uint64_t* mask, uint64_t* out0, uint64_t* out1,
                                        uint64_t* out2) {
  FR_REQUIRE_FIELD((csh_curve_t)field_of);
  CSH_REQUIRE(protocol <= 1 && party_id <= 2, "selftest_honk_co_relations: protocol 0 or 1, party_id 0, 1 or 2");
  const CoCall c{protocol, party_id, cols, edge_begin, edge_end, edge_idx, m, scaling, scaling_stride, params};
  return FR_CALL(field_of, hc_host_t<F>(stage, c, in, mask, out0, out1, out2));
}

}  // extern "C"
