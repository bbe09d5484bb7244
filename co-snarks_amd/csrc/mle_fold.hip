// Multilinear folds out[j] = in[2j] + u (in[2j+1] - in[2j]): the whole-vector arithmetic under the sumcheck rounds
// (partially_evaluate, co_sumcheck_prover.rs:34-98), the Gemini fold polynomials (compute_fold_polynomials, co_shplemini_prover.rs:236-312)
// and evaluate_mle (co-noir-common polynomial.rs:270-312, shared_polynomial.rs:154-199).
//
// Two kernels. k_mle_fold: one round over k vectors, an HBM-bound streaming kernel of the k_vec_mul kind (64 B read, 32 B written, one lazy
// multiplication per output value). k_mle_fold_rounds: a workgroup takes a tile of 2^T consecutive elements (tune "fold_tile_log") and folds
// it up to T times on chip, so a chain of m rounds is ceil(m / T) launches that read every level once (levels above FOLD_FUSE_MAX_VALUES
// go through k_mle_fold first, one round per launch: mle_fold_rounds_t). Scale, bounds and the tile's index
// algebra: mle_fold.hpp, shared with the host self-test.
//
// On chip. Round 1 goes from the loaded pair straight to registers; its results and those of every later round pass through LDS, one
// plane per limb, ping-pong between two regions with one barrier per round. Wave shuffles were weighed against this for the levels that
// fit a wave and not taken: a fold is a compaction (lane j needs the values of lanes 2 j and 2 j + 1), which no DPP row operation
// expresses, so it would be ds_bpermute_b32 -- 18 of them per pair (2 operands x 9 limbs) through the same LDS crossbar, against
// 9 ds_read_b64 that deliver both operands of a limb at once from consecutive banks, plus 9 ds_write_b32. The barrier the LDS form pays
// per round is noise next to the ~400-instruction multiplication between two of them.
#include "mle_fold.hpp"

#include <string.h>

#include <vector>

namespace csh {

// the pointers of one launch, a kernel argument (1 KiB): k > FOLD_VECS_PER_LAUNCH vectors are several launches, nothing is copied to the device
template <class F>
struct FoldVecs {
  const F* in[FOLD_VECS_PER_LAUNCH];
  F* out[FOLD_VECS_PER_LAUNCH];
};

// one round, blockIdx.y = vector; n_out = (n / 2) ncomp output values per vector
template <class F>
__global__ __launch_bounds__(FOLD_WG) void k_mle_fold(FoldVecs<F> v, F ud, size_t n_out, uint32_t ncomp) {
  const F* __restrict__ in = v.in[blockIdx.y];
  F* out = v.out[blockIdx.y];
  for (size_t o = blockIdx.x * (size_t)FOLD_WG + threadIdx.x; o < n_out; o += (size_t)gridDim.x * FOLD_WG) {
    const size_t s = fold_src(o, ncomp);
    out[o] = elem_fold(in[s], in[s + ncomp], ud);
  }
}

// up to T rounds of one tile, blockIdx.x = tile
template <class F>
__global__ __launch_bounds__(FOLD_WG) void k_mle_fold_rounds(FoldRoundsArgs<F> a) {
  extern __shared__ __align__(8) int32_t fold_lds[];
#pragma unroll 1
  for (int r = 1; r <= a.rounds; ++r) {
    if (r > 1) __syncthreads();  // round r - 1 has filled what round r reads, and has read what round r overwrites
    fold_tile_round(a, blockIdx.x, r, threadIdx.x, FOLD_WG, fold_lds);
  }
}

static int fold_tile_log() {
  const int t = tune().fold_tile_log.load(std::memory_order_relaxed);
  return fold_tile_log_ok(t) ? t : FOLD_TILE_LOG_DEFAULT;  // csh_tune_set refuses other values; the environment is not validated
}

template <class F>
static int mle_fold_t(const uint64_t* const* in, uint64_t* const* out, size_t k, size_t n, uint32_t ncomp, const uint64_t u[4], hipStream_t st) {
  const F ud = fr_to_rprime(fr_load<F>(u));
  const size_t n_out = n / 2 * ncomp;
  const unsigned gx = (unsigned)fr_stream_grid(n_out, FOLD_WG);
  for (size_t v0 = 0; v0 < k; v0 += FOLD_VECS_PER_LAUNCH) {
    const size_t kk = k - v0 < (size_t)FOLD_VECS_PER_LAUNCH ? k - v0 : (size_t)FOLD_VECS_PER_LAUNCH;
    FoldVecs<F> vs;
    memset(&vs, 0, sizeof vs);
    for (size_t v = 0; v < kk; ++v) {
      vs.in[v] = (const F*)in[v0 + v];
      vs.out[v] = (F*)out[v0 + v];
    }
    hipLaunchKernelGGL(k_mle_fold<F>, dim3(gx, (unsigned)kk), dim3(FOLD_WG), 0, st, vs, ud, n_out, ncomp);
  }
  CSH_HIP(hipGetLastError());
  return CSH_OK;
}

// Above this many values (n ncomp) per level the fused kernel does not pay: measured it moves its 64 B per element at
// 2.6 - 3.2 TB/s where a one-round sweep moves 96 B at 5.8, and with two components a chain of 2^24 elements took 0.839 ms fused against
// 0.625 ms round by round. The rounds whose input is larger than this therefore go through k_mle_fold one at a time, the rest of the
// chain through k_mle_fold_rounds. Word for word the same results: both are canonical_wide() of the same sum.
constexpr size_t FOLD_FUSE_MAX_VALUES = size_t(1) << 21;

template <class F>
static void launch_fold(const F* in0, F* out0, F* out1, size_t n, uint32_t ncomp, const F& ud, hipStream_t st) {
  FoldVecs<F> vs;
  memset(&vs, 0, sizeof vs);
  vs.in[0] = vs.in[1] = in0;
  vs.out[0] = out0;
  vs.out[1] = out1;
  const size_t n_out = n / 2 * ncomp;
  hipLaunchKernelGGL(k_mle_fold<F>, dim3((unsigned)fr_stream_grid(n_out, FOLD_WG), out1 ? 2u : 1u), dim3(FOLD_WG), 0, st, vs, ud, n_out, ncomp);
}

template <class F>
static int mle_fold_rounds_t(const uint64_t* in, size_t n, uint32_t ncomp, const uint64_t* u, size_t m, uint64_t* levels, uint64_t* last,
                             hipStream_t st) {
  const int T = fold_tile_log();
  size_t lead = 0;  // rounds taken one at a time
  while (lead < m && (n >> lead) * ncomp > FOLD_FUSE_MAX_VALUES) ++lead;
  const size_t nf = n >> lead, mf = m - lead;  // what the fused kernel starts from, and its rounds
  const size_t launches = (mf + T - 1) / T;
  // Without `levels` a level that is only passed on lives in the stream's workspace: n / 2 and n / 4 elements for the leading rounds
  // (ping-pong), nf / 2^T and nf / 2^(2T) between the fused launches.
  F *lead_buf[2] = {nullptr, nullptr}, *mid[2] = {nullptr, nullptr};
  if (!levels) {
    const size_t l0 = lead ? (n >> 1) * ncomp : 0, l1 = lead > 1 ? (n >> 2) * ncomp : 0;
    const size_t m0 = launches > 1 ? (nf >> T) * ncomp : 0, m1 = launches > 1 ? ((nf >> T) >> T) * ncomp + 1 : 0;
    if (l0 + m0) {
      Arena& ar = arena_for(st);
      CSH_TRY(ar.reserve(Arena::padded(l0 * sizeof(F)) + Arena::padded(l1 * sizeof(F)) + Arena::padded(m0 * sizeof(F)) + Arena::padded(m1 * sizeof(F))));
      lead_buf[0] = ar.take<F>(l0);
      lead_buf[1] = ar.take<F>(l1);
      mid[0] = ar.take<F>(m0);
      mid[1] = ar.take<F>(m1);
    }
  }
  const F* src = (const F*)in;
  for (size_t l = 0; l < lead; ++l) {  // level l -> level l + 1
    const bool final_round = l + 1 == m;
    F* lvl = levels ? (F*)levels + fold_level_offset(n, (int)l + 1) * ncomp : nullptr;
    F* out0 = lvl ? lvl : (final_round ? (F*)last : lead_buf[l & 1]);
    F* out1 = (lvl && final_round) ? (F*)last : nullptr;  // both asked for: the same sweep writes level m twice
    launch_fold<F>(src, out0, out1, n >> l, ncomp, fr_to_rprime(fr_load<F>(u + 4 * l)), st);
    src = out0;
  }
  if (mf) {
    const size_t lds = sizeof(int32_t) * LzOf<F>::NL * (fold_plane_a(T, ncomp) + fold_plane_b(T, ncomp));
    if (lds > 48 * 1024) CSH_TRY(raise_lds_limit((const void*)k_mle_fold_rounds<F>, 160 * 1024));
    F* lev_f = levels ? (F*)levels + fold_level_offset(n, (int)lead + 1) * ncomp : nullptr;  // level lead + 1 = the fused chain's level 1
    for (size_t p = 0; p < launches; ++p) {
      FoldRoundsArgs<F> a;
      memset(&a, 0, sizeof a);
      a.rounds = (int)(mf - p * T < (size_t)T ? mf - p * T : (size_t)T);
      for (int r = 0; r < a.rounds; ++r) a.ud[r] = fr_to_rprime(fr_load<F>(u + 4 * (lead + p * T + r)));
      a.in = src;
      a.n_in = nf >> (p * T);
      a.ncomp = ncomp;
      a.tile_log = T;
      const bool final_launch = p + 1 == launches;
      a.levels = lev_f ? lev_f + fold_level_offset(nf, (int)(p * T) + 1) * ncomp : nullptr;
      a.last = final_launch ? (F*)last : (lev_f ? nullptr : mid[p & 1]);
      const size_t tiles = (a.n_in + ((size_t)1 << T) - 1) >> T;
      hipLaunchKernelGGL(k_mle_fold_rounds<F>, dim3((unsigned)tiles), dim3(FOLD_WG), a.rounds > 1 ? lds : 0, st, a);
      // the next launch reads this one's last level: from the levels array if it is kept, from the workspace otherwise
      src = lev_f ? (const F*)lev_f + fold_level_offset(nf, (int)(p * T) + a.rounds) * ncomp : mid[p & 1];
    }
  }
  CSH_HIP(hipGetLastError());
  return CSH_OK;
}

}  // namespace csh

using namespace csh;

// the argument rules, checked before either form asks for a device
static int fold_check_common(csh_curve_t f, size_t n, uint32_t ncomp) {
  FR_REQUIRE_FIELD(f);
  FR_REQUIRE_NCOMP(ncomp);
  FR_REQUIRE_N(n);
  return CSH_OK;
}
static int mle_fold_check(csh_curve_t f, const uint64_t* const* in, uint64_t* const* out, size_t k, size_t n, uint32_t ncomp, const uint64_t* u) {
  CSH_TRY(fold_check_common(f, n, ncomp));
  CSH_REQUIRE(n >= 2 && n % 2 == 0, "mle_fold: n must be even and at least 2");
  CSH_REQUIRE(k >= 1, "mle_fold: k must be at least 1");
  CSH_REQUIRE(u, "mle_fold: NULL argument");
  CSH_TRY(fr_require_ptrs((const void* const*)in, k, "mle_fold"));
  CSH_TRY(fr_require_ptrs((const void* const*)out, k, "mle_fold"));
  FrRanges ins, outs;  // an output may not overlap any vector's input: fold into a second buffer and swap
  ins.add((const void* const*)in, k, 32 * n * ncomp);
  outs.add((const void* const*)out, k, 16 * n * ncomp);
  return fr_check_ranges(ins, outs, "mle_fold", false);
}
static int mle_fold_rounds_check(csh_curve_t f, const uint64_t* in, size_t n, uint32_t ncomp, const uint64_t* u, size_t m, const uint64_t* levels,
                                 const uint64_t* last) {
  CSH_TRY(fold_check_common(f, n, ncomp));
  CSH_REQUIRE(m >= 1 && m <= 28 && n >= 2 && (n & ((size_t(1) << m) - 1)) == 0, "mle_fold_rounds: m must be at least 1 and 2^m must divide n");
  CSH_REQUIRE(in && u, "mle_fold_rounds: NULL argument");
  CSH_REQUIRE(levels || last, "mle_fold_rounds: one of levels and last must be given");
  FrRanges ins, outs;
  ins.add(in, 32 * n * ncomp);
  if (levels) outs.add(levels, 32 * (n - (n >> m)) * ncomp);
  if (last) outs.add(last, 32 * (n >> m) * ncomp);
  return fr_check_ranges(ins, outs, "mle_fold_rounds", false);
}

extern "C" {

int csh_mle_fold_dev(csh_curve_t f, const uint64_t* const* in, uint64_t* const* out, size_t k, size_t n, uint32_t ncomp, const uint64_t u[4],
                     void* stream) {
  CSH_TRY(mle_fold_check(f, in, out, k, n, ncomp, u));
  CSH_TRY(ensure_device());
  hipStream_t st = resolve_stream(stream);
  return FR_CALL(f, mle_fold_t<F>(in, out, k, n, ncomp, u, st));
}
int csh_mle_fold_rounds_dev(csh_curve_t f, const uint64_t* in, size_t n, uint32_t ncomp, const uint64_t* u, size_t m, uint64_t* levels,
                            uint64_t* last, void* stream) {
  CSH_TRY(mle_fold_rounds_check(f, in, n, ncomp, u, m, levels, last));
  CSH_TRY(ensure_device());
  hipStream_t st = resolve_stream(stream);
  return FR_CALL(f, mle_fold_rounds_t<F>(in, n, ncomp, u, m, levels, last, st));
}

// ---- host-pointer forms: H2D, compute, D2H on the thread's stream --------------------------------------------------------------------
int csh_mle_fold(csh_curve_t f, const uint64_t* const* in, uint64_t* const* out, size_t k, size_t n, uint32_t ncomp, const uint64_t u[4]) {
  CSH_TRY(mle_fold_check(f, in, out, k, n, ncomp, u));
  HostStage h;
  const size_t ib = 32 * n * ncomp, ob = ib / 2;
  CSH_TRY(h.begin(k * (Arena::padded(ib) + Arena::padded(ob))));
  std::vector<const uint64_t*> din(k);
  std::vector<uint64_t*> dout(k);
  for (size_t v = 0; v < k; ++v) {
    uint64_t* d;
    CSH_TRY(h.up(d, in[v], ib));
    din[v] = d;
    CSH_TRY(h.up(dout[v], nullptr, ob));
  }
  CSH_TRY(csh_mle_fold_dev(f, din.data(), dout.data(), k, n, ncomp, u, h.st));
  for (size_t v = 0; v < k; ++v) CSH_TRY(h.down(out[v], dout[v], ob));
  return CSH_OK;
}
int csh_mle_fold_rounds(csh_curve_t f, const uint64_t* in, size_t n, uint32_t ncomp, const uint64_t* u, size_t m, uint64_t* levels,
                        uint64_t* last) {
  CSH_TRY(mle_fold_rounds_check(f, in, n, ncomp, u, m, levels, last));
  HostStage h;
  const size_t ib = 32 * n * ncomp, lb = 32 * (n - (n >> m)) * ncomp, eb = 32 * (n >> m) * ncomp;
  CSH_TRY(h.begin(Arena::padded(ib) + Arena::padded(lb) + Arena::padded(eb)));
  uint64_t *din, *dlev = nullptr, *dlast = nullptr;
  CSH_TRY(h.up(din, in, ib));
  if (levels) CSH_TRY(h.up(dlev, nullptr, lb));
  if (last) CSH_TRY(h.up(dlast, nullptr, eb));
  CSH_TRY(csh_mle_fold_rounds_dev(f, din, n, ncomp, u, m, dlev, dlast, h.st));
  if (levels) CSH_TRY(h.down(levels, dlev, lb));
  if (last) CSH_TRY(h.down(last, dlast, eb));
  return CSH_OK;
}

}  // extern "C"
