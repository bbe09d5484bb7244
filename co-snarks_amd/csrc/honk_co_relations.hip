// The sumcheck round of the collaborative UltraHonk prover on shares: one device stage per stretch of local arithmetic
// between two network rounds of co-noir/co-ultrahonk/src/co_decider/relations/ for the arithmetic, permutation, delta-range and
// log-derivative lookup relations, the edge selection of `can_skip`, and fold_accumulator! (relations/mod.rs:45-57). The network stays the
// caller's: a product between two stages is csh_rep3_local_mul_vec_dev + reshare (Rep3) or csh_vec_mul_dev + degree reduction (Shamir).
// Expressions, the element rule and the operand layouts: honk_co_relations.hpp, shared with the host self-test.
//
// k_hc_ops / k_hc_sub_one: streaming kernels of the honk_oink.hip kind -- grid-stride over flat value indices, 256 lanes, no LDS, tune
// "vec_max_blocks". k_hc_fold: a workgroup of 256 lanes takes 42 kept edges at a time, lane t < 252 the point t / 42 of edge slot t % 42,
// blockIdx.y the component; lanes sum over a grid-stride loop (tune "vec_max_blocks", at most HC_MAX_BLOCKS), the workgroup reduces one
// subrelation at a time through 8 KiB of LDS and its partial sums go to the stream's workspace; k_hc_finish, one workgroup per
// (subrelation, point, component), adds the workgroups' partials. Every addition is the exact modular one on canonical elements, so the
// words do not depend on how edges are dealt to lanes, workgroups or passes. No atomics.
// k_hc_sel_count / k_hc_sel_scan / k_hc_sel_write: a stable compaction -- every workgroup owns a contiguous chunk of the edges, counts its
// kept edges, one workgroup scans the counts, and every workgroup writes its chunk in order behind its offset.
#include "honk_co_relations.hpp"

namespace csh {

constexpr int HC_WG = 256;
constexpr int HC_EDGES_WG = 42;       // 6 x 42 = 252 lanes at work
constexpr int HC_MAX_BLOCKS = 1024;   // partial sums per output; chunks of the compaction (one scan workgroup)

template <class F, int STAGE>
__global__ __launch_bounds__(HC_WG) void k_hc_ops(HcArgs<F> a) {
  const size_t values = a.n7() * a.ncomp;
  for (size_t u = blockIdx.x * (size_t)HC_WG + threadIdx.x; u < values; u += (size_t)gridDim.x * HC_WG) hc_ops_at<STAGE>(a, u);
}
template <class F>
__global__ __launch_bounds__(HC_WG) void k_hc_sub_one(HcArgs<F> a) {
  const size_t values = 8 * a.n7() * a.ncomp;
  for (size_t u = blockIdx.x * (size_t)HC_WG + threadIdx.x; u < values; u += (size_t)gridDim.x * HC_WG) hc_sub_one_at(a, u);
}

// partial[((block * gridDim.y + comp) * NS + s) * 6 + k]
template <class F, int STAGE>
__global__ __launch_bounds__(HC_WG) void k_hc_fold(HcArgs<F> a, F* partial) {
  constexpr int NS = HcNs<STAGE>::value;
  __shared__ F sums[HC_WG];
  const int t = threadIdx.x, k = t / HC_EDGES_WG, slot = t % HC_EDGES_WG;
  const unsigned comp = blockIdx.y;
  F acc[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) acc[s] = F::zero();
  if (k < HC_FOLD_POINTS) {
#pragma unroll 1
    for (size_t j = blockIdx.x * (size_t)HC_EDGES_WG + slot; j < a.m; j += (size_t)gridDim.x * HC_EDGES_WG) {
      F term[NS];
      hc_terms_at<STAGE>(a, j, k, comp, term);
#pragma unroll
      for (int s = 0; s < NS; ++s) acc[s] = F::add(acc[s], term[s]);
    }
  }
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    if (s) __syncthreads();  // the sums of subrelation s - 1 have been read
    sums[t] = acc[s];
    __syncthreads();
    if (t < HC_FOLD_POINTS) {
      F sum = F::zero();
#pragma unroll 1
      for (int q = 0; q < HC_EDGES_WG; ++q) sum = F::add(sum, sums[t * HC_EDGES_WG + q]);
      partial[(((size_t)blockIdx.x * gridDim.y + comp) * NS + s) * HC_FOLD_POINTS + t] = sum;
    }
  }
}

template <class F>
struct HcFinish {
  const F* partial;
  F* out[HC_MAX_SUB];
  int len[HC_MAX_SUB];
  int ns;
  uint32_t ncomp, blocks;
};
// blockIdx.x = (s * 6 + k) * ncomp + comp; entry (k, comp) of accumulator s is out[s][k ncomp + comp]
template <class F>
__global__ __launch_bounds__(HC_WG) void k_hc_finish(HcFinish<F> f) {
  __shared__ F sums[HC_WG];
  const unsigned comp = blockIdx.x % f.ncomp, sk = blockIdx.x / f.ncomp;
  const int s = sk / HC_FOLD_POINTS, k = sk % HC_FOLD_POINTS;
  int len = 0;
  F* out = nullptr;
#pragma unroll
  for (int q = 0; q < HC_MAX_SUB; ++q)
    if (q == s) len = f.len[q], out = f.out[q];
  if (k >= len) return;  // uniform over the workgroup
  F sum = F::zero();
  for (uint32_t b = threadIdx.x; b < f.blocks; b += HC_WG)
    sum = F::add(sum, f.partial[(((size_t)b * f.ncomp + comp) * f.ns + s) * HC_FOLD_POINTS + k]);
  sums[threadIdx.x] = sum;
  __syncthreads();
  for (int w = HC_WG / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sums[threadIdx.x] = F::add(sums[threadIdx.x], sums[threadIdx.x + w]);
    __syncthreads();
  }
  if (threadIdx.x == 0) out[(size_t)k * f.ncomp + comp] = sums[0];
}

// ---- edge selection -------------------------------------------------------------------------------------------------------------------------
// workgroup b owns the edges [b chunk, min((b + 1) chunk, n_edges))
template <class F>
__global__ __launch_bounds__(HC_WG) void k_hc_sel_count(const F* q, size_t edge_begin, size_t n_edges, size_t chunk, uint32_t* counts) {
  __shared__ uint32_t part[HC_WG];
  const size_t lo = blockIdx.x * chunk, hi = lo + chunk < n_edges ? lo + chunk : n_edges;
  uint32_t c = 0;
  for (size_t i = lo + threadIdx.x; i < hi; i += HC_WG) c += hc_keep(q, edge_begin + 2 * i) ? 1u : 0u;
  part[threadIdx.x] = c;
  __syncthreads();
  for (int w = HC_WG / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) counts[blockIdx.x] = part[0];
}
// one workgroup of HC_MAX_BLOCKS lanes: offsets[b] = the kept edges in front of chunk b, *total = all of them
__global__ __launch_bounds__(HC_MAX_BLOCKS) void k_hc_sel_scan(const uint32_t* counts, uint32_t blocks, uint32_t* offsets, uint32_t* total) {
  __shared__ uint32_t s[HC_MAX_BLOCKS];
  const uint32_t t = threadIdx.x, own = t < blocks ? counts[t] : 0u;
  s[t] = own;
  __syncthreads();
  for (uint32_t d = 1; d < HC_MAX_BLOCKS; d <<= 1) {
    const uint32_t v = t >= d ? s[t - d] : 0u;
    __syncthreads();
    s[t] += v;
    __syncthreads();
  }
  if (t < blocks) offsets[t] = s[t] - own;
  if (t == HC_MAX_BLOCKS - 1) *total = s[t];
}
template <class F>
__global__ __launch_bounds__(HC_WG) void k_hc_sel_write(const F* q, size_t edge_begin, size_t n_edges, size_t chunk, const uint32_t* offsets,
                                                        uint32_t* out) {
  __shared__ uint32_t wave_total[HC_WG / 64];
  const size_t lo = blockIdx.x * chunk, hi = lo + chunk < n_edges ? lo + chunk : n_edges;
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  size_t base = offsets[blockIdx.x];
#pragma unroll 1
  for (size_t tile = lo; tile < hi; tile += HC_WG) {  // uniform over the workgroup
    const size_t i = tile + threadIdx.x;
    const bool keep = i < hi && hc_keep(q, edge_begin + 2 * i);
    const unsigned long long ballot = __ballot(keep);
    const uint32_t before = (uint32_t)__popcll(ballot & ((1ull << lane) - 1ull));
    if (lane == 0) wave_total[wave] = (uint32_t)__popcll(ballot);
    __syncthreads();
    uint32_t in_front = 0, all = 0;
#pragma unroll
    for (unsigned w = 0; w < HC_WG / 64; ++w) {
      in_front += w < wave ? wave_total[w] : 0u;
      all += wave_total[w];
    }
    if (keep) out[base + in_front + before] = (uint32_t)((edge_begin >> 1) + i);
    base += all;
    __syncthreads();  // wave_total is rewritten by the next tile
  }
}

// ---- launchers ------------------------------------------------------------------------------------------------------------------------------
struct HcCall {
  uint32_t protocol, party;
  const uint64_t* const* cols;
  size_t edge_begin, edge_end;
  const uint32_t* edge_idx;
  size_t m;
  const uint64_t* scaling;
  size_t scaling_stride;
  const uint64_t* params;
};
template <class F>
static HcArgs<F> hc_args(const HcCall& c, uint64_t colmask) {
  HcArgs<F> a;
  for (int k = 0; k < HR_COLS; ++k) a.col[k] = ((colmask >> k) & 1) ? (const F*)c.cols[k] : nullptr;
  a.edge_idx = c.edge_idx, a.scaling = (const F*)c.scaling, a.scaling_stride = c.scaling_stride;
  a.edge_begin = c.edge_begin, a.m = c.m;
  a.ncomp = c.protocol + 1, a.protocol = c.protocol, a.party = c.party, a.pub_comp = pq_pub_comp(c.protocol, c.party);
  hc_consts(a, c.params);
  a.in = a.mask = nullptr;
  a.out[0] = a.out[1] = a.out[2] = nullptr;
  return a;
}
static int hc_fold_blocks(size_t m) {
  int mb = tune().vec_max_blocks.load(std::memory_order_relaxed);
  if (mb <= 0 || mb > HC_MAX_BLOCKS) mb = HC_MAX_BLOCKS;
  return m ? grid_for(m, HC_EDGES_WG, mb) : 0;
}
static size_t hc_partial_bytes(int blocks, uint32_t ncomp, int ns) { return Arena::padded((size_t)blocks * ncomp * ns * HC_FOLD_POINTS * 32 + 32); }
// the fold of one stage: `partial` holds blocks * ncomp_grid * NS * 6 elements
template <int STAGE, class F>
static void hc_fold(const HcArgs<F>& a, uint32_t ncomp_grid, int blocks, F* partial, F* const* outs, hipStream_t st) {
  const HcFold fd = hc_fold_of(STAGE);
  if (blocks) hipLaunchKernelGGL((k_hc_fold<F, STAGE>), dim3(blocks, ncomp_grid), dim3(HC_WG), 0, st, a, partial);
  HcFinish<F> f;
  f.partial = partial, f.ns = fd.ns, f.ncomp = ncomp_grid, f.blocks = (uint32_t)blocks;
  for (int s = 0; s < HC_MAX_SUB; ++s) f.len[s] = fd.len[s], f.out[s] = s < fd.ns ? outs[s] : nullptr;
  hipLaunchKernelGGL(k_hc_finish<F>, dim3(fd.ns * HC_FOLD_POINTS * ncomp_grid), dim3(HC_WG), 0, st, f);
}
// a fold stage whose accumulators lie back to back in acc (entry (k, comp) of accumulator s at acc[(off_s + k) ncomp + comp])
template <int STAGE, class F>
static int hc_fold_stage(const HcCall& c, const uint64_t* in, uint64_t* acc, hipStream_t st) {
  HcArgs<F> a = hc_args<F>(c, hc_cols_of(STAGE));
  a.in = (const F*)in;
  const HcFold fd = hc_fold_of(STAGE);
  const int blocks = hc_fold_blocks(c.m);
  Arena& ar = arena_for(st);
  CSH_TRY(ar.reserve(hc_partial_bytes(blocks, a.ncomp, fd.ns)));
  F* partial = ar.take<F>((size_t)blocks * a.ncomp * fd.ns * HC_FOLD_POINTS + 1);
  F* outs[HC_MAX_SUB];
  size_t off = 0;
  for (int s = 0; s < fd.ns; ++s) outs[s] = (F*)acc + off * a.ncomp, off += fd.len[s];
  hc_fold<STAGE>(a, a.ncomp, blocks, partial, outs, st);
  CSH_HIP(hipGetLastError());
  return CSH_OK;
}
template <int STAGE, class F>
static int hc_ops_stage(const HcCall& c, const uint64_t* in, uint64_t* o0, uint64_t* o1, uint64_t* o2, hipStream_t st) {
  HcArgs<F> a = hc_args<F>(c, hc_cols_of(STAGE));
  a.in = (const F*)in;
  a.out[0] = (F*)o0, a.out[1] = (F*)o1, a.out[2] = (F*)o2;
  if (c.m) hipLaunchKernelGGL((k_hc_ops<F, STAGE>), dim3(fr_stream_grid(a.n7() * a.ncomp, HC_WG)), dim3(HC_WG), 0, st, a);
  CSH_HIP(hipGetLastError());
  return CSH_OK;
}
template <class F>
static int hc_arith_t(const HcCall& c, const uint64_t* mask, uint64_t* r0, uint64_t* r1, hipStream_t st) {
  HcArgs<F> a0 = hc_args<F>(c, hc_cols_of(HC_ARITH_R0)), a1 = hc_args<F>(c, hc_cols_of(HC_ARITH_R1));
  a0.mask = (const F*)mask;
  const int blocks = hc_fold_blocks(c.m);
  Arena& ar = arena_for(st);
  CSH_TRY(ar.reserve(hc_partial_bytes(blocks, 1, 1) + hc_partial_bytes(blocks, a1.ncomp, 1)));
  F* p0 = ar.take<F>((size_t)blocks * HC_FOLD_POINTS + 1);
  F* p1 = ar.take<F>((size_t)blocks * a1.ncomp * HC_FOLD_POINTS + 1);
  F* o0[1] = {(F*)r0};
  F* o1[1] = {(F*)r1};
  hc_fold<HC_ARITH_R0>(a0, 1, blocks, p0, o0, st);
  hc_fold<HC_ARITH_R1>(a1, a1.ncomp, blocks, p1, o1, st);
  CSH_HIP(hipGetLastError());
  return CSH_OK;
}
template <class F>
static int hc_delta_sub_one_t(uint32_t protocol, uint32_t party, uint64_t* sqr, size_t m, hipStream_t st) {
  HcArgs<F> a;
  memset(&a, 0, sizeof a);
  a.m = m, a.ncomp = protocol + 1, a.protocol = protocol, a.party = party, a.pub_comp = pq_pub_comp(protocol, party);
  hc_consts(a, nullptr);
  a.out[0] = (F*)sqr;
  if (m && a.pub_comp >= 0) hipLaunchKernelGGL(k_hc_sub_one<F>, dim3(fr_stream_grid(8 * a.n7() * a.ncomp, HC_WG)), dim3(HC_WG), 0, st, a);
  CSH_HIP(hipGetLastError());
  return CSH_OK;
}
template <class F>
static int hc_select_t(const uint64_t* q, size_t edge_begin, size_t edge_end, uint32_t* out, uint32_t* count, hipStream_t st) {
  const size_t n_edges = (edge_end - edge_begin) / 2;
  int mb = tune().vec_max_blocks.load(std::memory_order_relaxed);
  if (mb <= 0 || mb > HC_MAX_BLOCKS) mb = HC_MAX_BLOCKS;
  const int blocks = grid_for(n_edges, HC_WG, mb);
  const size_t chunk = (n_edges + blocks - 1) / blocks;
  Arena& ar = arena_for(st);
  CSH_TRY(ar.reserve(2 * Arena::padded((size_t)blocks * 4)));
  uint32_t* counts = ar.take<uint32_t>(blocks);
  uint32_t* offsets = ar.take<uint32_t>(blocks);
  hipLaunchKernelGGL(k_hc_sel_count<F>, dim3(blocks), dim3(HC_WG), 0, st, (const F*)q, edge_begin, n_edges, chunk, counts);
  hipLaunchKernelGGL(k_hc_sel_scan, dim3(1), dim3(HC_MAX_BLOCKS), 0, st, (const uint32_t*)counts, (uint32_t)blocks, offsets, count);
  hipLaunchKernelGGL(k_hc_sel_write<F>, dim3(blocks), dim3(HC_WG), 0, st, (const F*)q, edge_begin, n_edges, chunk, (const uint32_t*)offsets, out);
  CSH_HIP(hipGetLastError());
  return CSH_OK;
}

// ---- argument rules -------------------------------------------------------------------------------------------------------------------------
static int hc_range_ok(size_t edge_begin, size_t edge_end, const char* what) {
  if (!(edge_begin % 2 == 0 && edge_end % 2 == 0 && edge_begin < edge_end && edge_end <= HR_MAX_EDGE_END)) {
    set_error("%s: edge_begin and edge_end must be even, edge_begin < edge_end <= 2^28", what);
    return CSH_ERR_INVALID;
  }
  return CSH_OK;
}
// the rules every stage shares; adds what the stage reads of the columns, the list and the scaling table to `in`
static int hc_check(csh_curve_t field_of, const HcCall& c, uint64_t colmask, bool uses_scaling, bool uses_params, const char* what, FrRanges& in) {
  FR_REQUIRE_FIELD(field_of);
  if (c.protocol > 1 || c.party > 2) {
    set_error("%s: protocol must be 0 (plain / Shamir) or 1 (Rep3), party_id 0, 1 or 2", what);
    return CSH_ERR_INVALID;
  }
  bool ok = c.cols != nullptr && (c.params || !uses_params);
  for (int k = 0; ok && k < HR_COLS; ++k) ok = !((colmask >> k) & 1) || c.cols[k] != nullptr;
  if (!ok) {
    set_error("%s: NULL argument", what);
    return CSH_ERR_INVALID;
  }
  CSH_TRY(hc_range_ok(c.edge_begin, c.edge_end, what));
  const size_t n_edges = (c.edge_end - c.edge_begin) / 2;
  if (c.edge_idx ? c.m > n_edges : c.m != n_edges) {
    set_error("%s: m must be the number of edges of the range, or with an edge list at most that", what);
    return CSH_ERR_INVALID;
  }
  if (uses_scaling && c.scaling && !(c.scaling_stride >= 1 && c.scaling_stride <= HR_MAX_EDGE_END)) {
    set_error("%s: scaling_stride must be 1 .. 2^28", what);
    return CSH_ERR_INVALID;
  }
  const size_t ncomp = c.protocol + 1;
  for (int k = 0; k < HR_COLS; ++k)
    if ((colmask >> k) & 1) {
      const size_t eb = 32 * (k < HR_Q_M ? ncomp : 1);
      in.add((const char*)c.cols[k] + eb * c.edge_begin, eb * (c.edge_end - c.edge_begin));
    }
  if (c.edge_idx && c.m) in.add(c.edge_idx, 4 * c.m);
  if (uses_scaling && c.scaling) in.add((const char*)c.scaling + 32 * (c.edge_begin >> 1) * c.scaling_stride, 32 * (n_edges - 1) * c.scaling_stride + 32);
  return CSH_OK;
}
static int hc_require(bool ok, const char* what) {
  if (!ok) set_error("%s: NULL argument", what);
  return ok ? CSH_OK : CSH_ERR_INVALID;
}

}  // namespace csh

using namespace csh;

#define HC_COMMON_PARAMS                                                                                                                     \
  csh_curve_t field_of, uint32_t protocol, uint32_t party_id, const uint64_t *const *cols_dev, size_t edge_begin, size_t edge_end,          \
      const uint32_t *edge_idx_dev, size_t m
#define HC_CALL(scaling, stride, params) \
  HcCall { protocol, party_id, cols_dev, edge_begin, edge_end, edge_idx_dev, m, scaling, stride, params }

extern "C" {

int csh_honk_co_select_edges_dev(csh_curve_t field_of, const uint64_t* selector_dev, size_t edge_begin, size_t edge_end, uint32_t* edge_idx_dev,
                                 uint32_t* count_dev, void* stream) {
  const char* what = "honk_co_select_edges";
  FR_REQUIRE_FIELD(field_of);
  CSH_TRY(hc_require(selector_dev && edge_idx_dev && count_dev, what));
  CSH_TRY(hc_range_ok(edge_begin, edge_end, what));
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
  const HcCall c = HC_CALL(scaling_dev, scaling_stride, nullptr);
  FrRanges in, out;
  CSH_TRY(hc_check(field_of, c, hc_cols_of(HC_ARITH_R0) | hc_cols_of(HC_ARITH_R1), true, false, what, in));
  CSH_TRY(hc_require(r0_dev && r1_dev, what));
  if (protocol == 1 ? (m && !mask_dev) : mask_dev != nullptr) {
    set_error("%s: the mask vector is required for Rep3 and must be NULL for protocol 0", what);
    return CSH_ERR_INVALID;
  }
  const size_t ncomp = protocol + 1;
  if (mask_dev && m) in.add(mask_dev, 32 * HC_POINTS * m);
  out.add(r0_dev, 32 * 6);
  out.add(r1_dev, 32 * 5 * ncomp);
  CSH_TRY(fr_check_ranges(in, out, what));
  CSH_TRY(ensure_device());
  hipStream_t st = resolve_stream(stream);
  return FR_CALL(field_of, hc_arith_t<F>(c, mask_dev, r0_dev, r1_dev, st));
}

int csh_honk_co_perm_operands_dev(HC_COMMON_PARAMS, const uint64_t* params, uint64_t* lhs_dev, uint64_t* rhs_dev, void* stream) {
  const char* what = "honk_co_perm_operands";
  const HcCall c = HC_CALL(nullptr, 1, params);
  FrRanges in, out;
  CSH_TRY(hc_check(field_of, c, hc_cols_of(HC_PERM_OPS), false, true, what, in));
  CSH_TRY(hc_require((lhs_dev && rhs_dev) || !m, what));
  if (!m) return CSH_OK;
  const size_t seg = 32 * HC_POINTS * m * (protocol + 1);
  out.add(lhs_dev, 4 * seg), out.add(rhs_dev, 4 * seg);
  CSH_TRY(fr_check_ranges(in, out, what));
  CSH_TRY(ensure_device());
  hipStream_t st = resolve_stream(stream);
  return FR_CALL(field_of, hc_ops_stage<HC_PERM_OPS, F>(c, nullptr, lhs_dev, rhs_dev, nullptr, st));
}

int csh_honk_co_perm_operands2_dev(HC_COMMON_PARAMS, const uint64_t* params, uint64_t* rhs_dev, void* stream) {
  const char* what = "honk_co_perm_operands2";
  const HcCall c = HC_CALL(nullptr, 1, params);
  FrRanges in, out;
  CSH_TRY(hc_check(field_of, c, hc_cols_of(HC_PERM_OPS2), false, true, what, in));
  CSH_TRY(hc_require(rhs_dev || !m, what));
  if (!m) return CSH_OK;
  out.add(rhs_dev, 2 * 32 * HC_POINTS * m * (protocol + 1));
  CSH_TRY(fr_check_ranges(in, out, what));
  CSH_TRY(ensure_device());
  hipStream_t st = resolve_stream(stream);
  return FR_CALL(field_of, hc_ops_stage<HC_PERM_OPS2, F>(c, nullptr, rhs_dev, nullptr, nullptr, st));
}

int csh_honk_co_perm_finish_dev(HC_COMMON_PARAMS, const uint64_t* scaling_dev, size_t scaling_stride, const uint64_t* prod_dev, uint64_t* acc_dev,
                                void* stream) {
  const char* what = "honk_co_perm_finish";
  const HcCall c = HC_CALL(scaling_dev, scaling_stride, nullptr);
  FrRanges in, out;
  CSH_TRY(hc_check(field_of, c, hc_cols_of(HC_PERM_FINISH), true, false, what, in));
  CSH_TRY(hc_require(acc_dev && (prod_dev || !m), what));
  const size_t ncomp = protocol + 1;
  if (m) in.add(prod_dev, 2 * 32 * HC_POINTS * m * ncomp);
  out.add(acc_dev, 32 * 9 * ncomp);
  CSH_TRY(fr_check_ranges(in, out, what));
  CSH_TRY(ensure_device());
  hipStream_t st = resolve_stream(stream);
  return FR_CALL(field_of, hc_fold_stage<HC_PERM_FINISH, F>(c, prod_dev, acc_dev, st));
}

int csh_honk_co_delta_operands_dev(HC_COMMON_PARAMS, uint64_t* lhs_dev, void* stream) {
  const char* what = "honk_co_delta_operands";
  const HcCall c = HC_CALL(nullptr, 1, nullptr);
  FrRanges in, out;
  CSH_TRY(hc_check(field_of, c, hc_cols_of(HC_DELTA_OPS), false, false, what, in));
  CSH_TRY(hc_require(lhs_dev || !m, what));
  if (!m) return CSH_OK;
  out.add(lhs_dev, 8 * 32 * HC_POINTS * m * (protocol + 1));
  CSH_TRY(fr_check_ranges(in, out, what));
  CSH_TRY(ensure_device());
  hipStream_t st = resolve_stream(stream);
  return FR_CALL(field_of, hc_ops_stage<HC_DELTA_OPS, F>(c, nullptr, lhs_dev, nullptr, nullptr, st));
}

int csh_honk_co_delta_sub_one_dev(csh_curve_t field_of, uint32_t protocol, uint32_t party_id, uint64_t* sqr_dev, size_t m, void* stream) {
  const char* what = "honk_co_delta_sub_one";
  FR_REQUIRE_FIELD(field_of);
  CSH_REQUIRE(protocol <= 1 && party_id <= 2, "honk_co_delta_sub_one: protocol must be 0 (plain / Shamir) or 1 (Rep3), party_id 0, 1 or 2");
  CSH_REQUIRE(m <= HR_MAX_EDGE_END / 2, "honk_co_delta_sub_one: m must be at most 2^27");
  CSH_TRY(hc_require(sqr_dev || !m, what));
  if (!m) return CSH_OK;
  CSH_TRY(ensure_device());
  hipStream_t st = resolve_stream(stream);
  return FR_CALL(field_of, hc_delta_sub_one_t<F>(protocol, party_id, sqr_dev, m, st));
}

int csh_honk_co_delta_finish_dev(HC_COMMON_PARAMS, const uint64_t* scaling_dev, size_t scaling_stride, const uint64_t* mul_dev, uint64_t* acc_dev,
                                 void* stream) {
  const char* what = "honk_co_delta_finish";
  const HcCall c = HC_CALL(scaling_dev, scaling_stride, nullptr);
  FrRanges in, out;
  CSH_TRY(hc_check(field_of, c, hc_cols_of(HC_DELTA_FINISH), true, false, what, in));
  CSH_TRY(hc_require(acc_dev && (mul_dev || !m), what));
  const size_t ncomp = protocol + 1;
  if (m) in.add(mul_dev, 4 * 32 * HC_POINTS * m * ncomp);
  out.add(acc_dev, 32 * 24 * ncomp);
  CSH_TRY(fr_check_ranges(in, out, what));
  CSH_TRY(ensure_device());
  hipStream_t st = resolve_stream(stream);
  return FR_CALL(field_of, hc_fold_stage<HC_DELTA_FINISH, F>(c, mul_dev, acc_dev, st));
}

int csh_honk_co_lookup_operands_dev(HC_COMMON_PARAMS, const uint64_t* params, uint64_t* read_term_dev, uint64_t* inverses_dev, void* stream) {
  const char* what = "honk_co_lookup_operands";
  const HcCall c = HC_CALL(nullptr, 1, params);
  FrRanges in, out;
  CSH_TRY(hc_check(field_of, c, hc_cols_of(HC_LOOKUP_OPS), false, true, what, in));
  CSH_TRY(hc_require((read_term_dev && inverses_dev) || !m, what));
  if (!m) return CSH_OK;
  const size_t seg = 32 * HC_POINTS * m * (protocol + 1);
  out.add(read_term_dev, seg), out.add(inverses_dev, seg);
  CSH_TRY(fr_check_ranges(in, out, what));
  CSH_TRY(ensure_device());
  hipStream_t st = resolve_stream(stream);
  return FR_CALL(field_of, hc_ops_stage<HC_LOOKUP_OPS, F>(c, nullptr, read_term_dev, inverses_dev, nullptr, st));
}

int csh_honk_co_lookup_mid_dev(HC_COMMON_PARAMS, const uint64_t* scaling_dev, size_t scaling_stride, const uint64_t* params,
                               const uint64_t* write_inverse_dev, uint64_t* r0_dev, uint64_t* lhs_dev, uint64_t* rhs_dev, void* stream) {
  const char* what = "honk_co_lookup_mid";
  const HcCall c = HC_CALL(scaling_dev, scaling_stride, params);
  FrRanges in, out;
  CSH_TRY(hc_check(field_of, c, hc_cols_of(HC_LOOKUP_MID_R0) | hc_cols_of(HC_LOOKUP_MID_OPS), true, true, what, in));
  CSH_TRY(hc_require(r0_dev && ((write_inverse_dev && lhs_dev && rhs_dev) || !m), what));
  const size_t ncomp = protocol + 1, seg = 32 * HC_POINTS * m * ncomp;
  if (m) in.add(write_inverse_dev, seg), out.add(lhs_dev, 2 * seg), out.add(rhs_dev, 2 * seg);
  out.add(r0_dev, 32 * 5 * ncomp);
  CSH_TRY(fr_check_ranges(in, out, what));
  CSH_TRY(ensure_device());
  hipStream_t st = resolve_stream(stream);
  CSH_TRY(FR_CALL(field_of, hc_fold_stage<HC_LOOKUP_MID_R0, F>(c, write_inverse_dev, r0_dev, st)));
  return FR_CALL(field_of, hc_ops_stage<HC_LOOKUP_MID_OPS, F>(c, write_inverse_dev, nullptr, lhs_dev, rhs_dev, st));
}

int csh_honk_co_lookup_finish_dev(HC_COMMON_PARAMS, const uint64_t* scaling_dev, size_t scaling_stride, const uint64_t* params,
                                  const uint64_t* mul_dev, uint64_t* acc_dev, void* stream) {
  const char* what = "honk_co_lookup_finish";
  const HcCall c = HC_CALL(scaling_dev, scaling_stride, params);
  FrRanges in, out;
  CSH_TRY(hc_check(field_of, c, hc_cols_of(HC_LOOKUP_FINISH), true, true, what, in));
  CSH_TRY(hc_require(acc_dev && (mul_dev || !m), what));
  const size_t ncomp = protocol + 1;
  if (m) in.add(mul_dev, 2 * 32 * HC_POINTS * m * ncomp);
  out.add(acc_dev, 32 * 8 * ncomp);
  CSH_TRY(fr_check_ranges(in, out, what));
  CSH_TRY(ensure_device());
  hipStream_t st = resolve_stream(stream);
  return FR_CALL(field_of, hc_fold_stage<HC_LOOKUP_FINISH, F>(c, mul_dev, acc_dev, st));
}

}  // extern "C"

// Host run of the stage functions of honk_co_relations.hpp on host pointers: the loop bodies the kernels call, dealt to no lanes. `stage` is
// an HcStage; `in` is the stage's input vector (HC_SELECT: the selector column; HC_DELTA_SUB_ONE: none, out0 is updated in place), out0 ..
// out2 its outputs in the order of the device entry (HC_SELECT: out0 = the uint32_t list, out1 = the count word).
template <int STAGE, class F>
static void hc_host_fold(HcArgs<F>& a, uint32_t ncomp_grid, uint64_t* acc) {
  const HcFold fd = hc_fold_of(STAGE);
  size_t off = 0;
  for (int s = 0; s < fd.ns; ++s) {
    for (int k = 0; k < fd.len[s]; ++k)
      for (uint32_t comp = 0; comp < ncomp_grid; ++comp) {
        F sum = F::zero();
        for (size_t j = 0; j < a.m; ++j) {
          F term[HC_MAX_SUB];
          hc_terms_at<STAGE>(a, j, k, comp, term);
          sum = F::add(sum, term[s]);
        }
        ((F*)acc)[(off + k) * ncomp_grid + comp] = sum;
      }
    off += fd.len[s];
  }
}
template <int STAGE, class F>
static void hc_host_ops(HcArgs<F>& a) {
  for (size_t u = 0; u < a.n7() * a.ncomp; ++u) hc_ops_at<STAGE>(a, u);
}
template <class F>
static int hc_host_t(int stage, const HcCall& c, const uint64_t* in, const uint64_t* mask, uint64_t* o0, uint64_t* o1, uint64_t* o2) {
  if (stage == HC_SELECT) {
    uint32_t n = 0;
    for (size_t e = c.edge_begin; e < c.edge_end; e += 2)
      if (hc_keep((const F*)in, e)) ((uint32_t*)o0)[n++] = (uint32_t)(e >> 1);
    *(uint32_t*)o1 = n;
    return CSH_OK;
  }
  HcArgs<F> a = hc_args<F>(c, hc_cols_of(stage));
  a.in = (const F*)in, a.mask = (const F*)mask;
  a.out[0] = (F*)o0, a.out[1] = (F*)o1, a.out[2] = (F*)o2;
  switch (stage) {
    case HC_ARITH_R0: hc_host_fold<HC_ARITH_R0>(a, 1, o0); break;
    case HC_ARITH_R1: hc_host_fold<HC_ARITH_R1>(a, a.ncomp, o0); break;
    case HC_PERM_OPS: hc_host_ops<HC_PERM_OPS>(a); break;
    case HC_PERM_OPS2: hc_host_ops<HC_PERM_OPS2>(a); break;
    case HC_PERM_FINISH: hc_host_fold<HC_PERM_FINISH>(a, a.ncomp, o0); break;
    case HC_DELTA_OPS: hc_host_ops<HC_DELTA_OPS>(a); break;
    case HC_DELTA_SUB_ONE:
      for (size_t u = 0; u < 8 * a.n7() * a.ncomp; ++u) hc_sub_one_at(a, u);
      break;
    case HC_DELTA_FINISH: hc_host_fold<HC_DELTA_FINISH>(a, a.ncomp, o0); break;
    case HC_LOOKUP_OPS: hc_host_ops<HC_LOOKUP_OPS>(a); break;
    case HC_LOOKUP_MID_R0: hc_host_fold<HC_LOOKUP_MID_R0>(a, a.ncomp, o0); break;
    case HC_LOOKUP_MID_OPS: hc_host_ops<HC_LOOKUP_MID_OPS>(a); break;
    case HC_LOOKUP_FINISH: hc_host_fold<HC_LOOKUP_FINISH>(a, a.ncomp, o0); break;
    default: set_error("selftest_honk_co_relations: unknown stage %d", stage); return CSH_ERR_INVALID;
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
  const HcCall c{protocol, party_id, cols, edge_begin, edge_end, edge_idx, m, scaling, scaling_stride, params};
  return FR_CALL(field_of, hc_host_t<F>(stage, c, in, mask, out0, out1, out2));
}

}  // extern "C"
