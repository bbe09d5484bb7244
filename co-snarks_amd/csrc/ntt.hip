// Radix-2 NTT over Fr (BN254 / BLS12-381 / BLS12-377) on gfx950, LDS-tiled multi-pass.
//
// Conventions (the reference's taceo_ark_algebra::fft::Domain, see include/cosnarks_hip.h):
//   fft_out_to_in : bit-reversed coefficients -> natural-order evaluations   (decimation in time)
//   ifft_in_to_out: natural-order evaluations -> bit-reversed coefficients/n (decimation in frequency)
// Stage s (half-size m = 2^s) pairs index i (bit s clear) with i + m, twiddle w^((i mod m) * n/(2m)).
//
// A pass executes stages [s0, s0+k) for one tile entirely in LDS: the tile is the 2^k stage-bit values
// x 2^cb low "column" entries x ncomp components (ncomp = 2 for Rep3 shares), so every HBM access is a
// contiguous run of 2^cb * ncomp * 32 bytes (>= 64 B) and a 2^22 transform needs 3 read+write sweeps.
// Default path: butterflies in the signed lazy 9 x 29-bit field (limb-major LDS arrays), as radix-2 stages (k_ntt_pass_lazy) or as
// radix-4 rounds (k_ntt_pass_r4, transforms of >= 2^20 points); the 32-bit CIOS pass (k_ntt_pass: two 16-byte halves per element,
// conflict-free ds_read/write_b128) remains selectable with CSH_NTT_LAZY=0 for A/B measurements.
// Host side: a transform is planned ONCE per public call (NttPlan: one read of every tune knob, the pass list) and every launch of
// the call goes through launch_pass with that plan.
// the butterflies' products run with the pinned multiply-add order (field29.hpp): -5.5 % per transform, 52-61 VGPRs as before
#define CSH_PIN_MADS 3
#include <stdlib.h>

#include <memory>
#include <mutex>
#include <string.h>
#include <type_traits>

#include "common.hpp"
#include "field.hpp"
#include "field29.hpp"
#include "fr_entry.hpp"
#include "ntt_kernels.hpp"  // the device code: PassArgs, the tile map, the pass kernels

namespace csh {

struct Domain {
  csh_curve_t curve;
  int device;
  uint32_t log_n;
  size_t n;
  void* tw_fwd = nullptr;  // w^j, j < n/2
  void* tw_inv = nullptr;  // w^-j
  void* tw_fwd_lazy = nullptr;  // the powers the lazy butterflies use, as packed canonical w^j * R' (R' = 2^261), one contiguous run per stage
  void* tw_inv_lazy = nullptr;
  uint32_t n_inv_lazy[8];  // (1/n) * R', packed
  uint32_t gen[8], gen_inv[8], n_inv[8];  // Montgomery
  // The scaled coset table of the witness map (shift^i / n, ntt_coset_table_scaled) for the FIRST shift the domain is asked for: a reduction
  // always uses the same coset of its domain (reduction.rs:100), so every witness map after the first reads it instead of rebuilding it
  // (91 us of a 2^20 witness map). Another shift on the same domain is computed into the caller's scratch as before and is not cached.
  std::mutex cs_mu;
  uint64_t cs_shift[4] = {0, 0, 0, 0};
  void* cs_table = nullptr;
  hipEvent_t cs_ready = nullptr;

  Domain() = default;
  Domain(const Domain&) = delete;
  Domain& operator=(const Domain&) = delete;
  void release_natural_tables() {
    if (tw_fwd) (void)hipFree(tw_fwd);
    if (tw_inv) (void)hipFree(tw_inv);
    tw_fwd = tw_inv = nullptr;
  }
  ~Domain() {  // the one place that knows what a domain owns
    release_natural_tables();
    if (tw_fwd_lazy) (void)hipFree(tw_fwd_lazy);
    if (tw_inv_lazy) (void)hipFree(tw_inv_lazy);
    if (cs_table) (void)hipFree(cs_table);
    if (cs_ready) (void)hipEventDestroy(cs_ready);
  }
};

__device__ __forceinline__ uint32_t bitrev_n(uint32_t i, int log_n) { return log_n == 0 ? 0 : (__brev(i) >> (32 - log_n)); }

// in-place bit-reversal permutation of entries (ncomp elements each)
template <class F>
__global__ __launch_bounds__(256) void k_bit_reverse(F* data, int log_n, int ncomp) {
  const size_t n = size_t(1) << log_n;
  for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const size_t j = bitrev_n((uint32_t)i, log_n);
    if (i < j) {
      for (int c = 0; c < ncomp; ++c) {
        F a = data[i * ncomp + c];
        F b = data[j * ncomp + c];
        data[i * ncomp + c] = b;
        data[j * ncomp + c] = a;
      }
    }
  }
}

constexpr int POW_CHUNK = 32;
// out[perm(i)] = base^i, i < n; each thread produces POW_CHUNK consecutive powers
template <class F, bool BITREV>
__global__ __launch_bounds__(256) void k_powers(F* out, F base, size_t n, int log_n) {
  const size_t chunks = (n + POW_CHUNK - 1) / POW_CHUNK;
  for (size_t c = blockIdx.x * (size_t)256 + threadIdx.x; c < chunks; c += (size_t)gridDim.x * 256) {
    const size_t i0 = c * POW_CHUNK;
    F cur = F::pow_u64(base, (uint64_t)i0);
    for (int k = 0; k < POW_CHUNK; ++k) {
      const size_t i = i0 + k;
      if (i >= n) break;
      const size_t o = BITREV ? (size_t)bitrev_n((uint32_t)i, log_n) : i;
      out[o] = cur;
      cur = F::mul(cur, base);
    }
  }
}

// out[bitrev(i)] = storage form (packed canonical x * R', what the lazy passes multiply by) of scale * base^i: the coset table of
// a witness map with the inverse transform's 1/n folded in
template <class F, class LZ>
__global__ __launch_bounds__(256) void k_powers_lazy_scaled(F* out, F base, F scale, size_t n, int log_n) {
  const size_t chunks = (n + POW_CHUNK - 1) / POW_CHUNK;
  for (size_t c = blockIdx.x * (size_t)256 + threadIdx.x; c < chunks; c += (size_t)gridDim.x * 256) {
    const size_t i0 = c * POW_CHUNK;
    F cur = F::mul(F::pow_u64(base, (uint64_t)i0), scale);
    for (int k = 0; k < POW_CHUNK; ++k) {
      const size_t i = i0 + k;
      if (i >= n) break;
      out[bitrev_n((uint32_t)i, log_n)] = LZ::repack_for_storage(cur);
      cur = F::mul(cur, base);
    }
  }
}

// ---- host-side helpers (curve -> F, bytes -> F: fr_entry.hpp) ------------------------------------------
struct Pass {
  int s0, k, cb;
};

// log2(field elements per LDS tile) for a transform of 2^L entries of 2^ncomp_log elements. The tile is the unit of parallelism (one
// workgroup each): 2^11-element tiles give a 2^16-point transform 32 workgroups for 256 CUs and make every workgroup walk 11 dependent
// stages, so small transforms were latency-bound on a handful of CUs. Measured, interleaved (profiles/archive/r04_o_ntt_small.log, ms per
// transform, 2^11-element tiles -> best): 2^12 0.038 -> 0.015 (2^8), 2^14 0.043 -> 0.017 (2^8), 2^16 0.048 -> 0.021 (2^9), 2^17
// 0.052 -> 0.028 (2^9), 2^18 0.058 -> 0.039 (2^10); 2^19 .. 2^21 are best at 2^11 (more passes cost more than the parallelism gains);
// from 2^22 elements on 2^10-element tiles (four independent tiles per CU instead of two: their load / compute / store phases
// interleave) gain 1-4 % (r04_d_ntt_tile_ab.log, r04_k_ntt_tiles.log). tune "ntt_variant" bits 8-10 = v forces 2^(12-v) (A/B runs).
static int ntt_tile_log(int L, int ncomp_log, int forced_tile) {
  if (forced_tile >= 1 && forced_tile <= 4) return 12 - forced_tile;
  const int total = L + ncomp_log;
  if (total <= 15) return 8;
  if (total <= 17) return 9;
  if (total == 18) return 10;
  if (total >= 22) return 10;
  return NTT_TILE_LOG;
}

static int plan_passes(int L, int ncomp_log, int forced_tile, int forced_run, Pass* out) {
  const int TE = ntt_tile_log(L, ncomp_log, forced_tile) - ncomp_log;  // log2(entries per tile)
  // Contiguous run of a strided pass: 2^cb entries of ncomp x 32 bytes. 64-byte runs cost nothing against 256-byte ones and save a whole
  // sweep where the stages then fit two passes: 2^20 points 11 + 9 stages (128-byte runs) instead of 11 + 5 + 4, inverse / forward 0.143 / 0.135 ->
  // 0.132 / 0.123 ms, share pairs 0.258 / 0.259 -> 0.246 / 0.242 ms; 2^21 points 11 + 10 (64-byte runs) 0.268 / 0.285 -> 0.261 / 0.270
  // (profiles/archive/r03_q_ntt_runs.log, r03_r_ntt_tiles.log, r03_s_ntt_runs64.log).
  // 32-byte runs do not pay (2^22 as 11 + 11: 0.53 -> 0.60 ms), nor do 2^12-entry tiles at one tile per CU (2^22 as 12 + 10: 0.53 -> 0.55,
  // 2^24 2.2 -> 2.4 ms). tune "ntt_variant" bits 4-6 = log2(run entries) + 1 overrides the run length for A/B runs (0: this default).
  const int cb_min = forced_run ? (forced_run - 1 > ncomp_log ? forced_run - 1 - ncomp_log : 0) : (1 - ncomp_log);
  int np = 0;
  int k0 = L < TE ? L : TE;
  out[np++] = {0, k0, 0};
  int rem = L - k0;
  if (rem > 0) {
    const int kmax = TE - cb_min;
    const int npass = (rem + kmax - 1) / kmax;
    int s0 = k0;
    for (int i = 0; i < npass; ++i) {
      int k = rem / (npass - i);
      if (rem % (npass - i)) ++k;
      int cb = TE - k;
      if (cb > s0) cb = s0;
      out[np++] = {s0, k, cb};
      s0 += k;
      rem -= k;
    }
  }
  return np;
}

// Everything a public entry decides about a transform, decided ONCE: each tune knob is read one time here and every launch of the call
// uses this plan. (The knobs are process-wide atomics that tests and A/B tools flip at run time; a fused pair whose strided passes
// re-read them could run under another plan than its tile pass and skip the wrong stages.)
struct NttPlan {
  int L, ncomp_log;
  bool lazy;         // tune "ntt_lazy": the lazy-field kernels (default) or the 32-bit pass
  int max_threads;   // tune "ntt_threads": lanes per workgroup of the radix-2 kernels; 16 waves per 2^11-element tile measured best for both field representations
  bool pair;         // tune "ntt_pair" and "ntt_pair_min_log" allow the fused tile pass at this size
  int variant;       // tune "ntt_variant" as read, decoded below
  bool force_r4, force_r2;  // bit 0 / bit 1
  int forced_run;    // bits 4-6
  int forced_tile;   // bits 8-10
  int swz_mask;      // bit 11 switches the LDS bank swizzle off
  bool unit_rounds;  // bit 20 switches the unit-twiddle rounds off
  int only_pass;     // timing experiments (-DCSH_EXPERIMENTS only), WRONG RESULTS: bits 12-13 = run ONE pass of the plan,
  int ablate;        // bits 16-19 = PassArgs::ablate
  Pass passes[8];
  int np;

  NttPlan(int L_, uint32_t ncomp) : L(L_), ncomp_log(ncomp == 2 ? 1 : 0) {
    const Tune& t = tune();
    lazy = t.ntt_lazy.load(std::memory_order_relaxed) != 0;
    const int th = t.ntt_threads.load(std::memory_order_relaxed);
    max_threads = (th == 256 || th == 512 || th == 1024) ? th : 1024;
    pair = t.ntt_pair.load(std::memory_order_relaxed) != 0 && L >= t.ntt_pair_min_log.load(std::memory_order_relaxed);
    variant = t.ntt_variant.load(std::memory_order_relaxed);
    force_r4 = (variant & 1) != 0;
    force_r2 = (variant & 2) != 0;
    forced_run = (variant >> 4) & 7;
    forced_tile = (variant >> 8) & 7;
    swz_mask = (variant & 0x800) ? 0 : 31;
    unit_rounds = (variant & 0x100000) == 0;
    only_pass = kExperiments ? (variant >> 12) & 3 : 0;
    ablate = kExperiments ? (variant >> 16) & 0xf : 0;
    np = plan_passes(L, ncomp_log, forced_tile, forced_run, passes);
  }
  int tile_elems_log(const Pass& p) const { return p.k + p.cb + ncomp_log; }
  // Radix-4 pass (two stages per LDS round trip, 512 lanes per tile) or radix-2 pass. With the staged twiddle tables and two
  // folds per decimation-in-frequency round the radix-4 pass wins from 2^20 points on (one box, inverse / forward ms: 2^22
  // 0.583 / 0.541 -> 0.553 / 0.526, 2^24 2.36 / 2.04 -> 2.31 / 2.06, 2^20 0.153 / 0.142 -> 0.150 / 0.141; another box 2^22 forward
  // 0.549 -> 0.510) and ties or loses below (profiles/archive/r03_k_ntt_staged.log, r03_l_ntt_mix.log). Default: transforms of >= 2^20
  // points take it; tune "ntt_variant" 1 forces it everywhere, 2 forces the radix-2 pass.
  bool radix4(const Pass& p) const { return lazy && (force_r4 || (L >= 20 && !force_r2)) && p.k >= 2 && tile_elems_log(p) >= 2; }
  // the fused tile pass of a witness map's transform pair (k_ntt_pass_r4<.., PAIR>): the radix-4 kernel on contiguous tiles, default kernels otherwise
  bool fusable() const {
    const Pass& p = passes[0];
    return lazy && pair && p.s0 == 0 && p.cb == 0 && p.k >= 2 && tile_elems_log(p) >= 2 && (variant & ~0x100800) == 0;
  }
};

// this unit's instantiations of the pass kernels: the table every public entry launches from
template <class F>
static const void* product_kernels(PassForm form, bool dif) {
  using LZ = typename LazyOf<F>::type;
  switch (form) {
    case PassForm::Plain32: return dif ? (const void*)k_ntt_pass<F, true> : (const void*)k_ntt_pass<F, false>;
    case PassForm::LazyR2: return dif ? (const void*)k_ntt_pass_lazy<F, LZ, true> : (const void*)k_ntt_pass_lazy<F, LZ, false>;
    case PassForm::LazyR4: return dif ? (const void*)k_ntt_pass_r4<F, LZ, true> : (const void*)k_ntt_pass_r4<F, LZ, false>;
    case PassForm::LazyPair: return (const void*)k_ntt_pass_r4<F, LZ, true, true>;
  }
  return nullptr;
}

// The one launch site of the pass kernels: picks the instantiation, sizes the workgroup (radix-2 forms: one lane per butterfly of a stage,
// clamped to [64, max_threads]; radix-4 forms: one lane per 4-entry unit, clamped to [64, 512]), raises the kernel's LDS limit when the tile
// needs more than the default 48 KiB, launches. `kernels`: where the kernel comes from (product_kernels<F>, or the checked instantiations of
// the device self-test: same planning, tables and launch geometry).
template <class F>
static int launch_pass(PassForm form, bool dif, const PassArgs<F>& a, int max_threads, hipStream_t st, NttKernelTable kernels) {
  using LZ = typename LazyOf<F>::type;
  const void* kernel = kernels(form, dif);
  if (!kernel) {
    set_error("the kernel table has no kernel of pass form %d", (int)form);
    return CSH_ERR_INVALID;
  }
  const bool r4 = form == PassForm::LazyR4 || form == PassForm::LazyPair;
  const size_t elem_bytes = form == PassForm::Plain32 ? 32 : 4 * LZ::NL;
  const int elems_log = a.k + a.cb + a.ncomp_log;
  const size_t lanes = (size_t(1) << elems_log) >> (r4 ? 2 : 1);
  const size_t lane_max = r4 ? 512 : (size_t)max_threads;
  const int threads = lanes >= lane_max ? (int)lane_max : (lanes >= 64 ? (int)lanes : 64);
  const size_t lds_bytes = elem_bytes << elems_log;
  if (lds_bytes > 48 * 1024) CSH_TRY(raise_lds_limit(kernel, elem_bytes << NTT_TILE_LOG));
  const size_t tiles = (size_t(1) << a.L) >> (a.k + a.cb);
  PassArgs<F> args = a;
  void* by_struct[] = {&args};
  void* by_field[] = {&args.data, &args.tw, &args.scale_tbl, &args.L, &args.s0, &args.k, &args.cb, &args.ncomp_log, &args.swz_mask, &args.scale_out, &args.unit_rounds, &args.scale};  // k_ntt_pass_lazy
  (void)hipLaunchKernel(kernel, dim3((unsigned)tiles), dim3(threads), form == PassForm::LazyR2 ? by_field : by_struct, lds_bytes, st);
  CSH_HIP(hipGetLastError());
  return CSH_OK;
}

// tw_fwd / tw_inv = w^j / w^-j, j < max(n/2, 1): allocated and queued on st (a stream of the domain's device); the caller synchronises
// and, on any error, releases them (Domain::release_natural_tables)
template <class F>
static hipError_t build_natural_tables(Domain* d, hipStream_t st) {
  const size_t half = d->n / 2 ? d->n / 2 : 1;
  hipError_t e = hipMalloc(&d->tw_fwd, half * sizeof(F));
  if (e == hipSuccess) e = hipMalloc(&d->tw_inv, half * sizeof(F));
  if (e != hipSuccess) return e;
  const dim3 grid(grid_for((half + POW_CHUNK - 1) / POW_CHUNK, 256));
  hipLaunchKernelGGL((k_powers<F, false>), grid, dim3(256), 0, st, (F*)d->tw_fwd, fr_load<F>(d->gen), half, 0);
  hipLaunchKernelGGL((k_powers<F, false>), grid, dim3(256), 0, st, (F*)d->tw_inv, fr_load<F>(d->gen_inv), half, 0);
  return hipGetLastError();
}

// the natural-order twiddle tables of the 32-bit pass, (re)built when that pass is asked for on a domain that has released them
template <class F>
static int plain_tables(const Domain* cd) {
  // A Domain is shared across host threads (the mirror's DomainCache, the shim's Arc<HipDomain>): the pointers are only ever read or
  // written under this mutex (the former unlocked "already built?" test raced with the thread building them). Only the
  // CSH_NTT_LAZY = 0 A/B path comes here.
  static std::mutex mu;
  std::lock_guard<std::mutex> g(mu);
  Domain* d = const_cast<Domain*>(cd);
  if (d->tw_fwd && d->tw_inv) return CSH_OK;
  int prev_dev = -1;
  (void)hipGetDevice(&prev_dev);
  const bool switch_dev = prev_dev != d->device;
  if (switch_dev && hipSetDevice(d->device) != hipSuccess) {  // the tables live where the domain lives, whoever asks first
    set_error("hipSetDevice(%d) for the domain's twiddle tables failed", d->device);
    return CSH_ERR_HIP;
  }
  hipStream_t st = nullptr;
  hipError_t e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);  // a stream of the domain's device, not the caller's lane
  if (e == hipSuccess) e = build_natural_tables<F>(d, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (st) (void)hipStreamDestroy(st);
  if (e != hipSuccess) d->release_natural_tables();
  if (switch_dev && prev_dev >= 0) (void)hipSetDevice(prev_dev);
  if (e != hipSuccess) {
    set_error("building the natural-order twiddle tables failed: %s", hipGetErrorString(e));
    return e == hipErrorOutOfMemory ? CSH_ERR_OOM : CSH_ERR_HIP;
  }
  return CSH_OK;
}

// what pass `p` of `plan` is told: everything but the tables comes from the plan and the domain
template <class F>
static PassArgs<F> pass_args(const NttPlan& plan, const Domain* d, F* data, const Pass& p, const void* tw, bool scale_out, const F* scale_tbl) {
  PassArgs<F> a{};
  a.data = data;
  a.tw = reinterpret_cast<const F*>(tw);
  a.L = plan.L;
  a.s0 = p.s0;
  a.k = p.k;
  a.cb = p.cb;
  a.ncomp_log = plan.ncomp_log;
  a.scale = fr_load<F>(plan.lazy ? d->n_inv_lazy : d->n_inv);
  a.scale_tbl = scale_out ? scale_tbl : nullptr;
  a.scale_out = scale_out;
  a.swz_mask = plan.swz_mask;
  a.unit_rounds = plan.unit_rounds;
  if constexpr (kExperiments) a.ablate = plan.ablate;
  return a;
}

// The passes of one transform under `plan`, from pass `first` of the plan on (0: all of them; 1: the strided passes only, the pass over
// the contiguous tiles running fused with its neighbour of the other direction, run_ntt_pair). Decimation in frequency walks the plan backwards.
template <class F>
static int run_passes(const NttPlan& plan, const Domain* d, F* data, bool dif, hipStream_t st, const F* scale_tbl = nullptr, int first = 0,
                      NttKernelTable kernels = product_kernels<F>) {
  if (plan.L == 0) return CSH_OK;  // size-1 transform is the identity (1/n = 1)
  if (scale_tbl && (!plan.lazy || !dif)) {
    set_error("a scale table needs the lazy decimation-in-frequency passes");
    return CSH_ERR_INVALID;
  }
  // the tables of the 32-bit pass are read under plain_tables' rules: it takes the mutex and returns at once when both exist; the pointers
  // never change afterwards (freed with the domain)
  if (!plan.lazy) CSH_TRY(plain_tables<F>(d));
  const void* tw = plan.lazy ? (dif ? d->tw_inv_lazy : d->tw_fwd_lazy) : (dif ? d->tw_inv : d->tw_fwd);
  for (int i = first; i < plan.np; ++i) {
    const int pi = dif ? plan.np - 1 - (i - first) : i;
    if (plan.only_pass && pi != plan.only_pass - 1) continue;
    const Pass& p = plan.passes[pi];
    const PassForm form = !plan.lazy ? PassForm::Plain32 : (plan.radix4(p) ? PassForm::LazyR4 : PassForm::LazyR2);
    CSH_TRY(launch_pass<F>(form, dif, pass_args<F>(plan, d, data, p, tw, dif && p.s0 == 0, scale_tbl), plan.max_threads, st, kernels));
  }
  return CSH_OK;
}

template <class F>
static int create_domain_t(csh_curve_t curve, uint32_t log_n, const uint64_t* gen_words, Domain** out) {
  if (log_n > (uint32_t)F::Params::TWO_ADICITY) {
    set_error("Polynomial Degree too large");
    return CSH_ERR_DOMAIN;
  }
  F gen;
  if (gen_words) {
    gen = fr_load<F>(gen_words);
  } else {
    // GENERATOR^TRACE has order 2^TWO_ADICITY; TRACE = (p-1) >> TWO_ADICITY
    uint32_t tr[F::N];
    uint32_t pm1[F::N];
    for (int i = 0; i < F::N; ++i) pm1[i] = F::Params::MOD[i];
    pm1[0] -= 1;  // p is odd
    const int s = F::Params::TWO_ADICITY;
    for (int i = 0; i < F::N; ++i) {
      const int wi = i + s / 32;
      const uint64_t lo = wi < F::N ? pm1[wi] : 0;
      const uint64_t hi2 = wi + 1 < F::N ? pm1[wi + 1] : 0;
      tr[i] = (uint32_t)((lo | (hi2 << 32)) >> (s % 32));
    }
    F g = F::from_u64(std::is_same<F, Bn254Fr>::value ? 5 : std::is_same<F, Bls381Fr>::value ? 7 : 22);  // ark_{bn254, bls12_381, bls12_377}::Fr::GENERATOR
    gen = F::pow_limbs(g, tr, F::N);
    for (uint32_t i = log_n; i < (uint32_t)s; ++i) gen = F::sqr(gen);
  }
  // validate order: gen^(n) == 1 and gen^(n/2) != 1
  {
    F t = gen;
    for (uint32_t i = 0; i + 1 < log_n; ++i) t = F::sqr(t);
    F one = F::one();
    if (log_n >= 1) {
      if (t == one) {
        set_error("group_gen does not have order 2^%u", log_n);
        return CSH_ERR_DOMAIN;
      }
      t = F::sqr(t);
    }
    if (!(t == one)) {
      set_error("group_gen does not have order 2^%u", log_n);
      return CSH_ERR_DOMAIN;
    }
  }
  std::unique_ptr<Domain> d(new Domain());  // frees whatever exists on every error path
  d->curve = curve;
  if (hipGetDevice(&d->device) != hipSuccess) d->device = 0;
  d->log_n = log_n;
  d->n = size_t(1) << log_n;
  F gen_inv = F::inv(gen);
  F n_inv = F::inv(F::from_u64((uint64_t)d->n));
  memcpy(d->gen, &gen, 32);
  memcpy(d->gen_inv, &gen_inv, 32);
  memcpy(d->n_inv, &n_inv, 32);
  hipStream_t st = resolve_stream(nullptr);
  hipError_t e = build_natural_tables<F>(d.get(), st);
  if (e != hipSuccess) {
    set_error("building the natural-order twiddle tables failed: %s", hipGetErrorString(e));
    return e == hipErrorOutOfMemory ? CSH_ERR_OOM : CSH_ERR_HIP;
  }
  using LZ = typename LazyOf<F>::type;
  const size_t staged = d->n > 1 ? d->n - 1 : 1;  // one contiguous run per stage: 2^L - 1 entries
  hipError_t e4 = hipMalloc(&d->tw_fwd_lazy, staged * (sizeof(F) + sizeof(int32_t)));  // pre-sliced: 8 + 1 limbs per entry
  hipError_t e5 = hipMalloc(&d->tw_inv_lazy, staged * (sizeof(F) + sizeof(int32_t)));
  if (e4 == hipSuccess && e5 == hipSuccess && d->log_n >= 1) {
    hipLaunchKernelGGL((k_to_lazy_table<F, LZ>), dim3(grid_for(staged, 256)), dim3(256), 0, st, (const F*)d->tw_fwd, (F*)d->tw_fwd_lazy, (int)d->log_n);
    hipLaunchKernelGGL((k_to_lazy_table<F, LZ>), dim3(grid_for(staged, 256)), dim3(256), 0, st, (const F*)d->tw_inv, (F*)d->tw_inv_lazy, (int)d->log_n);
  }
  {
    const F nl = LZ::repack_for_storage(n_inv);  // host evaluation of the same template
    memcpy(d->n_inv_lazy, &nl, 32);
  }
  hipError_t e3 = hipStreamSynchronize(st);
  if (e3 != hipSuccess || e4 != hipSuccess || e5 != hipSuccess) {
    set_error("twiddle generation failed: %s", hipGetErrorString(e3 != hipSuccess ? e3 : (e4 != hipSuccess ? e4 : e5)));
    return e3 != hipSuccess ? CSH_ERR_HIP : CSH_ERR_OOM;
  }
  // Footprint: the staged, pre-sliced tables are (2^L - 1) x 36 bytes per direction (2^24: 1.2 GB for both, 2^26: 4.8 GB);
  // the natural tables they were made from (2^(L-1) x 32 bytes per direction) are only read by the 32-bit pass (CSH_NTT_LAZY=0, A/B
  // runs), so they are released here and rebuilt on demand (plain_tables) -- a third less per cached domain.
  if (tune().ntt_lazy.load(std::memory_order_relaxed) != 0) d->release_natural_tables();
  *out = d.release();
  return CSH_OK;
}

// exposed to other translation units (fused Groth16 h pipeline)
// ifft_in_to_out (its last pass multiplying entry i by scale_table[i], or by 1/n when the table is NULL) followed by fft_out_to_in
// on the same vector, the two passes over the contiguous tiles fused into ONE launch (k_ntt_pass_r4<.., PAIR>): reduction.rs:141-174 per
// vector. Falls back to the two transforms when the radix-4 pass does not apply to the plan's first pass (or tune "ntt_pair" = 0).
// One plan serves the fused pass and the strided passes on either side of it.
template <class F>
static int run_ntt_pair(const Domain* d, F* data, uint32_t ncomp, hipStream_t st, const F* scale_tbl, NttKernelTable kernels = product_kernels<F>) {
  const NttPlan plan((int)d->log_n, ncomp);
  if (plan.L == 0) return CSH_OK;
  if (!plan.fusable()) {
    CSH_TRY(run_passes<F>(plan, d, data, true, st, scale_tbl, 0, kernels));
    return run_passes<F>(plan, d, data, false, st, nullptr, 0, kernels);
  }
  CSH_TRY(run_passes<F>(plan, d, data, true, st, scale_tbl, 1, kernels));  // the strided passes of the inverse transform
  PassArgs<F> a = pass_args<F>(plan, d, data, plan.passes[0], d->tw_inv_lazy, true, scale_tbl);
  a.tw_fwd = reinterpret_cast<const F*>(d->tw_fwd_lazy);
  CSH_TRY(launch_pass<F>(PassForm::LazyPair, true, a, plan.max_threads, st, kernels));
  return run_passes<F>(plan, d, data, false, st, nullptr, 1, kernels);  // the strided passes of the forward transform
}
int ntt_run_pair_table(const Domain* d, uint64_t* data, uint32_t ncomp, const uint64_t* scale_table, hipStream_t st) {
  return FR_CALL(d->curve, run_ntt_pair<F>(d, (F*)data, ncomp, st, (const F*)scale_table));
}

int ntt_run(const Domain* d, uint64_t* data, uint32_t ncomp, bool dif, hipStream_t st) {
  return FR_CALL(d->curve, run_passes<F>(NttPlan((int)d->log_n, ncomp), d, (F*)data, dif, st));
}
// Device self-test (selftest_ntt_dev.hip): ntt_run (pair = false; dif chooses the direction) or ntt_run_pair_table (pair = true) with the
// pass kernels taken from `kernels` (one scalar field's: the domain's) instead of this unit's -- plan, tables and launch geometry are the
// product's.
int ntt_run_with_kernels(const Domain* d, uint64_t* data, uint32_t ncomp, bool pair, bool dif, const uint64_t* scale_table, NttKernelTable kernels,
                         hipStream_t st) {
  if (pair) return FR_CALL(d->curve, run_ntt_pair<F>(d, (F*)data, ncomp, st, (const F*)scale_table, kernels));
  return FR_CALL(d->curve, run_passes<F>(NttPlan((int)d->log_n, ncomp), d, (F*)data, dif, st, nullptr, 0, kernels));
}
// whether ntt_run_pair_table / ntt_coset_table_scaled apply (the table is in the lazy passes' storage form); false when the lazy
// passes are switched off (the caller then runs the unfused sequence)
bool ntt_scale_table_supported(const Domain* d) { return tune().ntt_lazy.load(std::memory_order_relaxed) != 0 && d->log_n >= 1; }
// table[bitrev(i)] = shift^i / n in the storage form of the lazy passes (the 1/n of the inverse transform folded into the coset table)
int ntt_coset_table_scaled(const Domain* d, const uint64_t* shift, uint64_t* out_dev, hipStream_t st) {
  return with_fr(d->curve, [&](auto fr) -> int {
    using F = typename decltype(fr)::type;
    hipLaunchKernelGGL((k_powers_lazy_scaled<F, LzOf<F>>), dim3(grid_for((d->n + POW_CHUNK - 1) / POW_CHUNK, 256)), dim3(256), 0, st, (F*)out_dev, fr_load<F>(shift),
                       fr_load<F>(d->n_inv), d->n, (int)d->log_n);
    CSH_HIP(hipGetLastError());
    return CSH_OK;
  });
}
// The same table, kept with the domain (see Domain::cs_table): *table = the cached copy, valid for work queued on `st` after this call
// (the builder's stream records an event every other stream waits for), or `scratch` freshly filled when the shift is not the cached one,
// the domain is too large to keep a copy (> 2^25 points = 1 GiB) or the allocation fails.
int ntt_coset_table_scaled_cached(const Domain* dc, const uint64_t* shift, uint64_t* scratch, hipStream_t st, const uint64_t** table) {
  Domain* d = const_cast<Domain*>(dc);
  *table = scratch;
  int cur = -1;
  if (d->log_n <= 25 && tune().h_table_cache.load(std::memory_order_relaxed) && hipGetDevice(&cur) == hipSuccess && cur == d->device) {  // (the copy is allocated on the domain's GPU)
    std::lock_guard<std::mutex> g(d->cs_mu);
    if (!d->cs_table) {
      void* buf = nullptr;
      hipEvent_t ev = nullptr;
      if (hipMalloc(&buf, 32 * d->n) == hipSuccess && hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess) {
        const int rc = ntt_coset_table_scaled(d, shift, static_cast<uint64_t*>(buf), st);
        if (rc == CSH_OK && hipEventRecord(ev, st) == hipSuccess) {
          memcpy(d->cs_shift, shift, 32);
          d->cs_table = buf;
          d->cs_ready = ev;
          *table = static_cast<const uint64_t*>(buf);
          return CSH_OK;
        }
      }
      (void)hipGetLastError();
      if (ev) (void)hipEventDestroy(ev);
      if (buf) (void)hipFree(buf);
    } else if (memcmp(d->cs_shift, shift, 32) == 0) {
      CSH_HIP(hipStreamWaitEvent(st, d->cs_ready, 0));
      *table = static_cast<const uint64_t*>(d->cs_table);
      return CSH_OK;
    }
  }
  return ntt_coset_table_scaled(d, shift, scratch, st);
}
int ntt_coset_table(const Domain* d, const uint64_t* shift, uint64_t* out_dev, hipStream_t st) {
  return with_fr(d->curve, [&](auto fr) -> int {
    using F = typename decltype(fr)::type;
    hipLaunchKernelGGL((k_powers<F, true>), dim3(grid_for((d->n + POW_CHUNK - 1) / POW_CHUNK, 256)), dim3(256), 0, st, (F*)out_dev, fr_load<F>(shift), d->n,
                       (int)d->log_n);
    CSH_HIP(hipGetLastError());
    return CSH_OK;
  });
}
int ntt_bit_reverse(csh_curve_t c, uint64_t* data, uint32_t log_n, uint32_t ncomp, hipStream_t st) {
  if (log_n == 0) return CSH_OK;
  return with_fr(c, [&](auto fr) -> int {
    using F = typename decltype(fr)::type;
    hipLaunchKernelGGL(k_bit_reverse<F>, dim3(grid_for(size_t(1) << log_n, 256)), dim3(256), 0, st, (F*)data, (int)log_n, (int)ncomp);
    CSH_HIP(hipGetLastError());
    return CSH_OK;
  });
}

size_t domain_size_of(const Domain* d) { return d->n; }
csh_curve_t domain_curve_of(const Domain* d) { return d->curve; }
const void* domain_gen_of(const Domain* d) { return d->gen; }
int domain_device_of(const Domain* d) { return d->device; }

}  // namespace csh

using namespace csh;

static int check_dom(csh_domain_t dom, uint32_t ncomp) {
  CSH_REQUIRE(dom, "domain is NULL");
  FR_REQUIRE_NCOMP(ncomp);
  int cur = -1;
  const Domain* d = reinterpret_cast<const Domain*>(dom);
  if (hipGetDevice(&cur) == hipSuccess && cur != d->device) {
    set_error("the domain's twiddle tables live on device %d but the calling thread is bound to device %d (csh_init)", d->device, cur);
    return CSH_ERR_INVALID;
  }
  return CSH_OK;
}

extern "C" {

int csh_domain_create(csh_curve_t field_of, uint32_t log_n, const uint64_t group_gen[4], csh_domain_t* out) {
  CSH_REQUIRE(out, "out is NULL");
  CSH_REQUIRE(log_n <= 31, "log_n too large");
  CSH_TRY(ensure_device());
  Domain* d = nullptr;
  CSH_TRY(FR_CALL(field_of, create_domain_t<F>(field_of, log_n, group_gen, &d)));
  *out = reinterpret_cast<csh_domain_t>(d);
  return CSH_OK;
}
int csh_domain_size(csh_domain_t dom, size_t* n) {
  CSH_REQUIRE(dom && n, "NULL argument");
  *n = reinterpret_cast<Domain*>(dom)->n;
  return CSH_OK;
}
int csh_domain_free(csh_domain_t dom) {
  if (!dom) return CSH_OK;
  Domain* d = reinterpret_cast<Domain*>(dom);
  delete d;
  return CSH_OK;
}

int csh_ifft_in_to_out_dev(csh_domain_t dom, uint64_t* data, uint32_t ncomp, void* stream) {
  CSH_TRY(check_dom(dom, ncomp));
  CSH_TRY(ensure_device());
  return ntt_run(reinterpret_cast<Domain*>(dom), data, ncomp, true, resolve_stream(stream));
}
int csh_fft_out_to_in_dev(csh_domain_t dom, uint64_t* data, uint32_t ncomp, void* stream) {
  CSH_TRY(check_dom(dom, ncomp));
  CSH_TRY(ensure_device());
  return ntt_run(reinterpret_cast<Domain*>(dom), data, ncomp, false, resolve_stream(stream));
}
int csh_fft_dev(csh_domain_t dom, uint64_t* data, uint32_t ncomp, void* stream) {
  CSH_TRY(check_dom(dom, ncomp));
  CSH_TRY(ensure_device());
  Domain* d = reinterpret_cast<Domain*>(dom);
  hipStream_t st = resolve_stream(stream);
  CSH_TRY(ntt_bit_reverse(d->curve, data, d->log_n, ncomp, st));
  return ntt_run(d, data, ncomp, false, st);
}
int csh_ifft_dev(csh_domain_t dom, uint64_t* data, uint32_t ncomp, void* stream) {
  CSH_TRY(check_dom(dom, ncomp));
  CSH_TRY(ensure_device());
  Domain* d = reinterpret_cast<Domain*>(dom);
  hipStream_t st = resolve_stream(stream);
  CSH_TRY(ntt_run(d, data, ncomp, true, st));
  return ntt_bit_reverse(d->curve, data, d->log_n, ncomp, st);
}
int csh_bit_reverse_dev(csh_curve_t field_of, uint64_t* data, uint32_t log_n, uint32_t ncomp, void* stream) {
  FR_REQUIRE_NCOMP(ncomp);
  CSH_REQUIRE(fr_known(field_of), "unknown curve");
  CSH_REQUIRE(log_n <= 31, "log_n too large");
  CSH_TRY(ensure_device());
  return ntt_bit_reverse(field_of, data, log_n, ncomp, resolve_stream(stream));
}
int csh_coset_table_dev(csh_domain_t dom, const uint64_t shift[4], uint64_t* out, void* stream) {
  CSH_REQUIRE(dom && shift && out, "NULL argument");
  CSH_TRY(ensure_device());
  return ntt_coset_table(reinterpret_cast<Domain*>(dom), shift, out, resolve_stream(stream));
}

// ---- host-pointer wrappers ---------------------------------------------------------------------------
static int host_transform(csh_domain_t dom, uint64_t* data, uint32_t ncomp, int which) {
  CSH_TRY(check_dom(dom, ncomp));
  Domain* d = reinterpret_cast<Domain*>(dom);
  HostStage h;
  const size_t bytes = d->n * ncomp * 32;
  CSH_TRY(h.begin(Arena::padded(bytes)));
  uint64_t* dd;
  CSH_TRY(h.up(dd, data, bytes));
  int rc = CSH_OK;
  switch (which) {
    case 0: rc = csh_ifft_in_to_out_dev(dom, dd, ncomp, h.st); break;
    case 1: rc = csh_fft_out_to_in_dev(dom, dd, ncomp, h.st); break;
    case 2: rc = csh_fft_dev(dom, dd, ncomp, h.st); break;
    default: rc = csh_ifft_dev(dom, dd, ncomp, h.st); break;
  }
  if (rc != CSH_OK) return rc;
  return h.down(data, dd, bytes);
}
int csh_ifft_in_to_out(csh_domain_t dom, uint64_t* data, uint32_t ncomp) { return host_transform(dom, data, ncomp, 0); }
int csh_fft_out_to_in(csh_domain_t dom, uint64_t* data, uint32_t ncomp) { return host_transform(dom, data, ncomp, 1); }
int csh_fft(csh_domain_t dom, uint64_t* data, uint32_t ncomp) { return host_transform(dom, data, ncomp, 2); }
int csh_ifft(csh_domain_t dom, uint64_t* data, uint32_t ncomp) { return host_transform(dom, data, ncomp, 3); }

int csh_bit_reverse(csh_curve_t field_of, uint64_t* data, uint32_t log_n, uint32_t ncomp) {
  CSH_REQUIRE(log_n <= 31, "log_n too large");
  HostStage h;
  const size_t bytes = (size_t(1) << log_n) * ncomp * 32;
  CSH_TRY(h.begin(Arena::padded(bytes)));
  uint64_t* dd;
  CSH_TRY(h.up(dd, data, bytes));
  CSH_TRY(csh_bit_reverse_dev(field_of, dd, log_n, ncomp, h.st));
  return h.down(data, dd, bytes);
}
int csh_coset_table(csh_domain_t dom, const uint64_t shift[4], uint64_t* out) {
  CSH_REQUIRE(dom && shift && out, "NULL argument");
  Domain* d = reinterpret_cast<Domain*>(dom);
  HostStage h;
  const size_t bytes = d->n * 32;
  CSH_TRY(h.begin(Arena::padded(bytes)));
  uint64_t* dd;
  CSH_TRY(h.up(dd, nullptr, bytes));
  CSH_TRY(csh_coset_table_dev(dom, shift, dd, h.st));
  return h.down(out, dd, bytes);
}

}  // extern "C"
