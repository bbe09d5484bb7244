// Device code of the NTT passes (host side: ntt.hip): what a pass launch is told, the tile <-> vector index map, the LDS tile of the lazy
// field, and the pass kernels -- the 32-bit pass, the radix-2 and the radix-4 / fused-pair passes in the signed lazy 9 x 29-bit field --
// plus the kernel that stages their twiddle tables.
// Two translation units instantiate these kernels: ntt.hip (the product) and selftest_ntt_dev.hip (the same text compiled with the
// device form of the limb-bound contract, field29.hpp CSH_CHECK_BOUNDS_DEVICE). A kernel template instantiated under one name in two
// units would be one host stub and two code objects, so everything here lives in an inline namespace whose name the including unit
// chooses (CSH_NTT_KERNEL_NS): the symbols differ, the text is one.
#pragma once
#include <type_traits>

#include "common.hpp"
#include "field.hpp"
#include "field29.hpp"

#ifndef CSH_NTT_KERNEL_NS
#define CSH_NTT_KERNEL_NS ntt_product
#endif

namespace csh {

// The kernel forms launch_pass chooses from, and where it takes their addresses from: (form, decimation in frequency?) -> the kernel of one
// scalar field, or NULL when the table has no such form. ntt.hip's own table is the default everywhere; the self-test unit hands its
// checked instantiations to ntt_run_with_kernels.
enum class PassForm { Plain32, LazyR2, LazyR4, LazyPair };
using NttKernelTable = const void* (*)(PassForm form, bool dif);
struct Domain;
int ntt_run_with_kernels(const Domain* d, uint64_t* data, uint32_t ncomp, bool pair, bool dif, const uint64_t* scale_table, NttKernelTable kernels,
                         hipStream_t st);  // ntt.hip

inline namespace CSH_NTT_KERNEL_NS {

constexpr int NTT_MAX_THREADS = 1024;
constexpr int NTT_TILE_LOG = 11;  // 2^11 field elements = 64 KiB of LDS per workgroup

// What one pass launch is told (by value to k_ntt_pass_r4 and k_ntt_pass, field by field to k_ntt_pass_lazy, see there). One pass = stages [s0, s0+k) of a size-2^L transform over tiles of 2^k x 2^cb entries of
// 2^ncomp_log elements. Every field is a run-time, wave-uniform value.
template <class F>
struct PassArgs {
  // (what a kernel reads before its first global load comes first and contiguous: the wavefront fetches it in one batch of scalar loads)
  F* data;
  const F* tw;         // the pass's twiddle table: staged w * R' (lazy kernels), natural-order Montgomery (32-bit pass)
  const F* tw_fwd;     // PAIR only: the staged table of the forward transform that follows
  const F* scale_tbl;  // lazy kernels: per-entry factor that replaces `scale` (1/n times the coset power), or NULL
  int L, s0, k, cb, ncomp_log;
  int swz_mask;        // LazyLds bank swizzle: 31, or 0 = off (tune "ntt_variant" bit 11, A/B runs)
  bool scale_out;      // multiply by the scale on store (last pass of an inverse transform)
  bool unit_rounds;    // global stage 0 (and 1 in the radix-4 rounds) skips its unit-twiddle multiplications (tune "ntt_variant" bit 20 = off)
#ifdef CSH_EXPERIMENTS
  int ablate;          // k_ntt_pass_r4 timing experiments (tune "ntt_variant" bits 16-19, WRONG RESULTS): 1 = no butterfly rounds, 2 = no global
                       // loads, 4 = no stores, 8 = no canonicalisation before the store
#endif
  F scale;             // 1/n, in the form of the kernel's multiplication (times R' for the lazy kernels)
};

// Tile <-> vector index map of a pass: LDS entry e = t * CC + cc (t: the k stage bits, cc: column and component, CC = 2^(cb + ncomp_log))
// is global element (((hi << k | t) << mid_bits | mid) * CC + cc, where tile = (hi << mid_bits) | mid and mid_bits = s0 - cb. With
// s0 = cb = 0 (the pass over the contiguous tiles) this is tile * E + e.
struct TileMap {
  int s0, k, cb, cc_log, ncomp_log, mid_bits;
  size_t mid, hi;
  __device__ __forceinline__ TileMap(size_t tile, int s0_, int k_, int cb_, int ncomp_log_)
      : s0(s0_), k(k_), cb(cb_), cc_log(cb_ + ncomp_log_), ncomp_log(ncomp_log_), mid_bits(s0_ - cb_), mid(tile & ((size_t(1) << (s0_ - cb_)) - 1)), hi(tile >> (s0_ - cb_)) {}
  __device__ __forceinline__ int entries() const { return 1 << (k + cc_log); }
  __device__ __forceinline__ size_t global_index(int e) const {
    const int cc = e & ((1 << cc_log) - 1);
    const size_t t = e >> cc_log;
    return (((((hi << k) | t) << mid_bits) | mid) << cc_log) + cc;
  }
  // i mod 2^s, s = s0 + q, of the butterfly whose lower entry has local stage bits t_lo (< 2^q) and column / component cc: (t_lo << s0) | (mid << cb) | col
  __device__ __forceinline__ size_t index_mod_stage(int t_lo, int cc) const { return ((size_t)t_lo << s0) | (mid << cb) | (size_t)(cc >> ncomp_log); }
};

template <class F>
__device__ __forceinline__ F lds_get(const uint4* lo, const uint4* hi, int e) {
  union { F f; uint4 q[2]; } u;
  u.q[0] = lo[e];
  u.q[1] = hi[e];
  return u.f;
}
template <class F>
__device__ __forceinline__ void lds_put(uint4* lo, uint4* hi, int e, const F& f) {
  union { F f; uint4 q[2]; } u;
  u.f = f;
  lo[e] = u.q[0];
  hi[e] = u.q[1];
}

// The 32-bit pass (independent arithmetic: CIOS Montgomery on 8 x u32, natural-order twiddle table).
template <class F, bool DIF>
__global__ __launch_bounds__(NTT_MAX_THREADS) void k_ntt_pass(const PassArgs<F> a) {
  static_assert(sizeof(F) == 32, "Fr is 8 x u32");
  extern __shared__ uint4 lds_raw[];
  const TileMap map(blockIdx.x, a.s0, a.k, a.cb, a.ncomp_log);
  const int cc_log = map.cc_log;
  const int CC = 1 << cc_log;
  const int E = map.entries();
  uint4* lo = lds_raw;
  uint4* hi = lds_raw + E;
  const int tid = threadIdx.x;
  const int NTT_THREADS = blockDim.x;

  for (int e = tid; e < E; e += NTT_THREADS) lds_put<F>(lo, hi, e, a.data[map.global_index(e)]);
  __syncthreads();

  const int half_E = E >> 1;
  for (int qq = 0; qq < a.k; ++qq) {
    const int q = DIF ? (a.k - 1 - qq) : qq;  // local stage; global stage s = s0 + q
    const int half = 1 << q;
    const int tw_shift = a.L - 1 - (a.s0 + q);
    for (int bidx = tid; bidx < half_E; bidx += NTT_THREADS) {
      const int cc = bidx & (CC - 1);
      const int tb = bidx >> cc_log;
      const int t_lo = tb & (half - 1);
      const int t0 = ((tb >> q) << (q + 1)) | t_lo;
      const int e0 = (t0 << cc_log) | cc;
      const int e1 = e0 + (half << cc_log);
      const F w = a.tw[map.index_mod_stage(t_lo, cc) << tw_shift];
      F u = lds_get<F>(lo, hi, e0);
      F v = lds_get<F>(lo, hi, e1);
      if (DIF) {
        F s = F::add(u, v);
        F d = F::mul(F::sub(u, v), w);
        lds_put<F>(lo, hi, e0, s);
        lds_put<F>(lo, hi, e1, d);
      } else {
        F x = F::mul(v, w);
        lds_put<F>(lo, hi, e0, F::add(u, x));
        lds_put<F>(lo, hi, e1, F::sub(u, x));
      }
    }
    __syncthreads();
  }

  for (int e = tid; e < E; e += NTT_THREADS) {
    F f = lds_get<F>(lo, hi, e);
    if (a.scale_out) f = F::mul(f, a.scale);
    a.data[map.global_index(e)] = f;
  }
}

// ---- lazy-field pass ---------------------------------------------------------------------------------------------
// Same tiling, butterflies in the signed 9 x 29-bit representation (field29.hpp): an element x*R (arkworks Montgomery,
// R = 2^256) is re-sliced into 29-bit limbs as is, the twiddle comes in the R' = 2^261 domain, so the lazy Montgomery
// product  (x R)(w R') / R' = (x w) R  stays in the arkworks domain with no conversion multiplication. A product costs
// 162 v_mad_i64_i32 instead of ~136 mads + ~300 carry instructions; sums are limb-wise + one parallel carry step. Values
// drift to at most ~(1 + k) p over the k <= 11 stages of a decimation-in-time pass (u' = u + v w: limbs stay normalised,
// the top limb absorbs the growth); in a decimation-in-frequency pass the sum output feeds the next sum and would double
// per stage, so it is folded back below 2p each stage (fold_top: a top-limb quotient estimate, no multiplication). The
// tile is brought back to [0, p) once per pass when it is stored (canonical_wide).
// limb-major LDS tile: limbs (2i, 2i+1) of element e live in an 8-byte slot of pair-array i (ds_read/write_b64, lane
// stride 8 bytes: conflict-free), the odd last limb in a 4-byte array behind them -- 5 LDS accesses per element instead of 9
// Entry idx of a staged twiddle table: limbs 0..7 of the canonical w * R' as the 8 words of slot idx (two 16-byte loads), limb 8
// in an int32 array behind the `slots` slots -- ready to multiply by, no re-slicing per butterfly.
template <class F, class LZ>
__device__ __forceinline__ LZ load_sliced_twiddle(const F* __restrict__ twl, size_t idx, size_t slots) {
  static_assert(LZ::NL == F::N + 1, "one limb more than 32-bit words");
  const F f = twl[idx];
  LZ r;
#pragma unroll
  for (int i = 0; i < F::N; ++i) r.l[i] = (int32_t)f.l[i];
  r.l[F::N] = reinterpret_cast<const int32_t*>(twl + slots)[idx];
  return r;
}

// Bank swizzle of the tile index: entry e lives at slot e ^ ((e >> 2) & 31). A radix-4 round at local stage q reads / writes, per lane, the
// entries t0 + j 2^q: for q = 0 the lanes of a wave touch every FOURTH 8-byte slot (8-way bank conflicts on ds_read_b64, whose 32-lane
// groups need 32 distinct slots mod 32, and on ds_write_b64, whose 16-lane groups need 16 distinct slots mod 16), for q = 1..4 runs of
// 2^q slots 2^(q+2) apart. XOR-ing bits 2..6 of the index into bits 0..4 makes every one of those patterns a bijection onto the slots of
// its lane group (checked exhaustively over GF(2) for all rounds q = 0..9, tile and strided passes, with one or two components per entry;
// only the 32-lane read of the single left-over radix-2 stage at q = 0 keeps a 2-way conflict), while runs of >= 32 consecutive entries
// (tile load / store, late rounds) stay conflict-free: the map permutes entries inside aligned blocks of 128. Two instructions per address.
// SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE of k_ntt_pass_r4 before: 0.28-0.30 (profiles/archive/r03_f_vecops_ntt_pmc_sq.csv).
template <class LZ>
struct LazyLds {
  int32_t* base;
  int E;
  int swz;  // 31, or 0 to switch the swizzle off (A/B runs: tune "ntt_variant" bit 11)
  static constexpr int NP = LZ::NL / 2;
  __device__ __forceinline__ int slot(int e) const { return e ^ ((e >> 2) & swz); }
  __device__ __forceinline__ LZ get(int e0) const {
    const int e = slot(e0);
    LZ r;
    const int2* pairs = reinterpret_cast<const int2*>(base);
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int2 v = pairs[i * E + e];
      r.l[2 * i] = v.x;
      r.l[2 * i + 1] = v.y;
    }
    if (LZ::NL & 1) r.l[LZ::NL - 1] = base[2 * NP * E + e];
    return r;
  }
  __device__ __forceinline__ void put(int e0, const LZ& v) const {
    const int e = slot(e0);
    int2* pairs = reinterpret_cast<int2*>(base);
#pragma unroll
    for (int i = 0; i < NP; ++i) pairs[i * E + e] = make_int2(v.l[2 * i], v.l[2 * i + 1]);
    if (LZ::NL & 1) base[2 * NP * E + e] = v.l[LZ::NL - 1];
  }
};

// ---- pieces shared by the lazy kernels ----------------------------------------------------------------------------
// twiddle of global stage s0 + q for the pair whose lower index has local stage bits t_lo (< 2^q); staged table: stage s starts at 2^s - 1
template <class F, class LZ>
__device__ __forceinline__ LZ staged_twiddle(const F* __restrict__ tw, const TileMap& map, int L, int q, int t_lo, int cc) {
  return load_sliced_twiddle<F, LZ>(tw, ((size_t(1) << (map.s0 + q)) - 1) + map.index_mod_stage(t_lo, cc), (size_t(1) << L) - 1);
}

// Tile load, four entries per lane with all four global loads issued before the first is consumed: written as one rolled loop
// (load, unpack, put per iteration) every lane paid four SERIAL trips to HBM per tile -- the 0.04-0.05 ms per sweep that no butterfly
// stage accounts for (profiles/archive/r04_e_ntt_per_pass.log; shortening the store tail by a third changed nothing, r04_l_ntt.log).
// `fill` (timing experiments only): the value every entry takes instead of its global load.
template <class F, class LZ>
__device__ __forceinline__ void load_tile(const LazyLds<LZ>& lds, const TileMap& map, const F* __restrict__ data, const F* fill = nullptr) {
  const int E = lds.E;
  const int tid = threadIdx.x;
  const int NT = blockDim.x;
  for (int base = 0; base < E; base += 4 * NT) {
    F raw[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = base + tid + i * NT;
      if (e < E) raw[i] = fill ? *fill : data[map.global_index(e)];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = base + tid + i * NT;
      if (e < E) lds.put(e, LZ::unpack(raw[i]));
    }
  }
  __syncthreads();
}

// the factor of global element g on the way out: the 1/n of the inverse transform (sc), or -- witness maps -- a per-entry table that
// already carries it (1/n times the coset power of the entry, in the pass's output order): the coset shift costs no sweep and no
// multiplication of its own
template <class F, class LZ>
__device__ __forceinline__ LZ out_scale(const PassArgs<F>& a, const LZ& sc, size_t g) {
  return a.scale_tbl ? LZ::unpack(a.scale_tbl[g >> a.ncomp_log]) : sc;
}

// Store tail: every entry scaled (scale_out), brought back to [0, p) and packed. ablate (timing experiments only): 4 = no stores,
// 8 = no canonicalisation.
template <class F, class LZ>
__device__ __forceinline__ void store_tile(const LazyLds<LZ>& lds, const TileMap& map, const PassArgs<F>& a, bool scale_out, int ablate = 0) {
  const LZ sc = LZ::unpack(a.scale);
  for (int e = threadIdx.x; e < lds.E; e += blockDim.x) {
    const size_t g = map.global_index(e);
    LZ f = lds.get(e);
    if (scale_out) f = LZ::mul(f, out_scale<F, LZ>(a, sc, g));
    if (ablate & 4) continue;
    a.data[g] = (ablate & 8) ? f.pack() : f.canonical_wide().pack();
  }
}

// One radix-2 butterfly stage (local stage q) over the tile. NORM: run the parallel carry step on the decimation-in-time outputs. x is
// a fresh product (limbs < 2^B) and u +- x of a normalised u is a two-term sum, still an admissible `a` operand of the next
// stage's product, so the carry step is only needed every second stage (and not after the last one: the tile leaves
// through mul / canonical_wide, which take two-term limbs).
template <bool DIF, bool NORM, class F, class LZ>
__device__ __forceinline__ void radix2_stage(const LazyLds<LZ>& lds, const TileMap& map, const F* __restrict__ tw, int L, int q, bool unit_rounds) {
  const int cc_log = map.cc_log;
  const int CC = 1 << cc_log;
  const int half_E = lds.E >> 1;
  const int half = 1 << q;
  for (int bidx = threadIdx.x; bidx < half_E; bidx += blockDim.x) {
    const int cc = bidx & (CC - 1);
    const int tb = bidx >> cc_log;
    const int t_lo = tb & (half - 1);
    const int t0 = ((tb >> q) << (q + 1)) | t_lo;
    const int e0 = (t0 << cc_log) | cc;
    const int e1 = e0 + (half << cc_log);
    const LZ w = staged_twiddle<F, LZ>(tw, map, L, q, t_lo, cc);
    const LZ u = lds.get(e0);
    const LZ v = lds.get(e1);
    if (unit_rounds && map.s0 + q == 0) {  // w = 1 for every butterfly of global stage 0 (wave-uniform branch)
      if (DIF) {
        lds.put(e0, LZ::add(u, v).fold_top());
        lds.put(e1, LZ::sub(u, v));            // the pass's last stage: leaves through mul / canonical_wide, which take two-term limbs
      } else {
        lds.put(e0, LZ::add(u, v));            // the pass's first stage: u, v are unpack() outputs, the sums two-term operands as after a product
        lds.put(e1, LZ::sub(u, v));
      }
      continue;
    }
    if (DIF) {
      lds.put(e0, LZ::add(u, v).fold_top());   // sums feed sums here: keep the value within (-p, 2p) every stage
      lds.put(e1, LZ::mul(LZ::sub(u, v), w));  // the two-term difference is an admissible product operand as is
    } else {
      const LZ x = LZ::mul(v, w);
      if (NORM) {
        lds.put(e0, LZ::add(u, x).normalized());
        lds.put(e1, LZ::sub(u, x).normalized());
      } else {
        lds.put(e0, LZ::add(u, x));
        lds.put(e1, LZ::sub(u, x));
      }
    }
  }
  __syncthreads();
}

template <class F, class LZ, bool DIF>
__global__ __launch_bounds__(NTT_MAX_THREADS) __attribute__((amdgpu_waves_per_eu(8))) void k_ntt_pass_lazy(F* data, const F* tw, const F* scale_tbl, int L, int s0, int k, int cb, int ncomp_log, int swz_mask,
                                                                                           bool scale_out, bool unit_rounds, F scale) {
  // PassArgs field by field (launch_pass unpacks it), put together again here: this kernel sits at its 64-VGPR cap and its decimation-in-
  // frequency form spills 4 VGPRs; with the arguments as one by-value struct the allocator puts a spill reload 11 instructions behind the
  // twiddle loads of the butterfly block, whose wait (in-order vmcnt) then exposes the twiddle latency: 2^16 inverse +7 %
  PassArgs<F> a{};
  a.data = data;
  a.tw = tw;
  a.scale_tbl = scale_tbl;
  a.L = L;
  a.s0 = s0;
  a.k = k;
  a.cb = cb;
  a.ncomp_log = ncomp_log;
  a.swz_mask = swz_mask;
  a.scale_out = scale_out;
  a.unit_rounds = unit_rounds;
  a.scale = scale;
  extern __shared__ uint4 lds_raw[];
  const TileMap map(blockIdx.x, a.s0, a.k, a.cb, a.ncomp_log);
  const LazyLds<LZ> lds{reinterpret_cast<int32_t*>(lds_raw), map.entries(), a.swz_mask};
  load_tile<F, LZ>(lds, map, a.data);
  for (int qq = 0; qq < a.k; ++qq) {
    const int q = DIF ? (a.k - 1 - qq) : qq;
    if (DIF || (qq & 1))
      radix2_stage<DIF, true, F, LZ>(lds, map, a.tw, a.L, q, a.unit_rounds);
    else
      radix2_stage<DIF, false, F, LZ>(lds, map, a.tw, a.L, q, a.unit_rounds);
  }
  store_tile<F, LZ>(lds, map, a, a.scale_out);
}

// ---- radix-4 form of the lazy pass ---------------------------------------------------------------------------------
// Two butterfly stages per LDS round trip: a lane owns the four tile entries that stages (q, q + 1) connect, keeps them in
// registers across both stages and touches LDS once per pair of stages (half the ds traffic, address arithmetic, waits and
// barriers of the radix-2 loop; three twiddle loads per four butterflies instead of four: the second stage's two twiddles are
// w and w * omega^(n/4), both straight from the table). 512 lanes per 2048-entry tile (one radix-4 unit per lane and round), two
// tiles per CU, up to 128 VGPRs per lane. The arithmetic per element is the radix-2 pass's, operation for operation (same
// operand classes: a round starts from normalised values, the second stage multiplies two-term sums, the outputs are normalised
// once; in decimation in frequency every sum is folded), so the limb-bound contracts checked by the host self-test carry over.
// An odd stage count leaves one radix-2 stage (last in DIT, last = local stage 0 in DIF).
// PAIR (round 6; DIF must be true, s0 = cb = 0): the LAST pass of an inverse transform (decimation in frequency, table `tw`) and the FIRST
// pass of the forward transform that follows it in a witness map (decimation in time, table `tw_fwd`) work on the same contiguous
// tiles -- ifft_in_to_out, coset table, fft_out_to_in of reduction.rs:141-174 -- so one launch keeps the tile in LDS across both:
// DIF rounds, the scale (1/n, or the per-entry table carrying 1/n times the coset power) and the canonical form a store + load would
// have left, DIT rounds, one store. One HBM sweep, one launch and one LDS fill less per pair; the field elements are the same.
template <class F, class LZ, bool DIF, bool PAIR = false>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_ntt_pass_r4(const PassArgs<F> a) {
  static_assert(!PAIR || DIF, "the pair kernel starts with the decimation-in-frequency half");
  extern __shared__ uint4 lds_raw[];
  const TileMap map(blockIdx.x, PAIR ? 0 : a.s0, a.k, PAIR ? 0 : a.cb, a.ncomp_log);
  const int s0 = map.s0;
  const int k = a.k;
  const int cc_log = map.cc_log;
  const int CC = 1 << cc_log;
  const int E = map.entries();
  const LazyLds<LZ> lds{reinterpret_cast<int32_t*>(lds_raw), E, a.swz_mask};
  const int tid = threadIdx.x;
  const int NT = blockDim.x;
  int ablate = 0;  // product builds: constant 0, the branches it guards fold away
  if constexpr (kExperiments) ablate = a.ablate;

  load_tile<F, LZ>(lds, map, a.data, (ablate & 2) ? &a.scale : nullptr);

  auto twiddle = [&](const F* __restrict__ tw, int q, int t_lo, int cc) { return staged_twiddle<F, LZ>(tw, map, a.L, q, t_lo, cc); };
  // stages (q, q + 1) on the four entries t0 + {0, 1, 2, 3} * 2^q of every unit
  auto round4 = [&](auto dif_c, const F* __restrict__ tw, int q) {
    constexpr bool D = decltype(dif_c)::value;
    const int quarter_E = E >> 2;
    for (int u = tid; u < quarter_E; u += NT) {
      const int cc = u & (CC - 1);
      const int tb = u >> cc_log;
      const int t_lo = tb & ((1 << q) - 1);
      const int t0 = ((tb >> q) << (q + 2)) | t_lo;
      const int e0 = (t0 << cc_log) | cc;
      const int st = 1 << (q + cc_log);
      LZ x0 = lds.get(e0), x1 = lds.get(e0 + st), x2 = lds.get(e0 + 2 * st), x3 = lds.get(e0 + 3 * st);
      if constexpr (D) {
        // Value / limb bounds of a round (inputs: normalised limbs, values within (-p, 2.2 p)): the first stage's sums stay below
        // 4.4 p and only take the parallel carry step (their differences, < 6.5 p in magnitude with two-term limbs, are admissible
        // product operands: the contract is |value| < 8 p); the second stage's sum of sums (< 8.8 p) is folded below 2 p; the sum of
        // the two fresh products (< 2.2 p) again only takes the carry step. Two folds per round instead of four.
        {  // stage q + 1: (x0, x2) with w, (x1, x3) with w * omega^(n/4)
          const LZ w2 = twiddle(tw, q + 1, t_lo, cc), w3 = twiddle(tw, q + 1, t_lo + (1 << q), cc);
          LZ d02, d13;  // the two products of a fold are independent: their multiply-adds alternate (FpS::mul2)
          LZ::mul2(LZ::sub(x0, x2), w2, LZ::sub(x1, x3), w3, d02, d13);
          x0 = LZ::add(x0, x2).normalized();
          x1 = LZ::add(x1, x3).normalized();
          x2 = d02;
          x3 = d13;
        }
        {  // stage q: (x0, x1), (x2, x3), one twiddle
          const LZ w1 = twiddle(tw, q, t_lo, cc);
          LZ d01, d23;
          LZ::mul2(LZ::sub(x0, x1), w1, LZ::sub(x2, x3), w1, d01, d23);
          x0 = LZ::add(x0, x1).fold_top();
          x2 = LZ::add(x2, x3).normalized();
          x1 = d01;
          x3 = d23;
        }
      } else {
        {  // stage q: inputs normalised, outputs two-term sums (admissible product operands as they are)
          const LZ w1 = twiddle(tw, q, t_lo, cc);
          LZ p1, p3;
          LZ::mul2(x1, w1, x3, w1, p1, p3);
          x1 = LZ::sub(x0, p1);
          x0 = LZ::add(x0, p1);
          x3 = LZ::sub(x2, p3);
          x2 = LZ::add(x2, p3);
        }
        {  // stage q + 1: the carry step runs once per round, on the outputs
          const LZ w2 = twiddle(tw, q + 1, t_lo, cc), w3 = twiddle(tw, q + 1, t_lo + (1 << q), cc);
          LZ p2, p3;
          LZ::mul2(x2, w2, x3, w3, p2, p3);
          x2 = LZ::sub(x0, p2).normalized();
          x0 = LZ::add(x0, p2).normalized();
          x3 = LZ::sub(x1, p3).normalized();
          x1 = LZ::add(x1, p3).normalized();
        }
      }
      lds.put(e0, x0);
      lds.put(e0 + st, x1);
      lds.put(e0 + 2 * st, x2);
      lds.put(e0 + 3 * st, x3);
    }
    __syncthreads();
  };
  // Global stages 0 and 1 of the whole transform (the pass with s0 = 0, local round q = 0): stage 0 has twiddle 1 everywhere, stage 1 has
  // 1 on its first pair and omega^(n/4) -- one table entry, the same for every lane -- on its second: ONE multiplication per unit
  // instead of four (3 of the 22 x 2 multiplications a 4-entry unit meets in a 2^22 transform). Limb / value bounds: decimation in time
  // meets this round first, on unpack() outputs (limbs 0..NL-2 in [0, 2^B), value in [0, p)): the four-term sum x0 + x1 + x2 + x3 stays
  // below 2^(B+2) <= 2^31 - 4 per limb and below 4 p, what the general round reaches with three fresh products. Decimation in frequency
  // meets it last, on normalised values within (-p, 2.2 p): sums are carried / folded stage by stage as in the general round; the two
  // differences that are no longer passed through a multiplication stay two- or (carried) three-term sums within (-6.4 p, 6.4 p) and
  // leave through the tail's mul / canonical_wide, whose contracts (two-term limbs, |value| < 8 p resp. 32 p) they meet.
  auto round4_unit = [&](auto dif_c, const F* __restrict__ tw) {
    constexpr bool D = decltype(dif_c)::value;
    const int quarter_E = E >> 2;
    const LZ w4 = twiddle(tw, 1, 1, 0);  // omega^(n/4) (forward table) / its inverse (inverse table): staged entry 2
    for (int u = tid; u < quarter_E; u += NT) {
      const int cc = u & (CC - 1);
      const int tb = u >> cc_log;
      const int e0 = ((tb << 2) << cc_log) | cc;
      const int st = 1 << cc_log;
      LZ x0 = lds.get(e0), x1 = lds.get(e0 + st), x2 = lds.get(e0 + 2 * st), x3 = lds.get(e0 + 3 * st);
      if constexpr (D) {
        const LZ d13 = LZ::mul(LZ::sub(x1, x3), w4);   // stage 1, second pair
        const LZ d02 = LZ::sub(x0, x2);                // stage 1, first pair: times 1
        x0 = LZ::add(x0, x2).normalized();
        x1 = LZ::add(x1, x3).normalized();
        const LZ o1 = LZ::sub(x0, x1);                 // stage 0: times 1
        x0 = LZ::add(x0, x1).fold_top();
        x1 = o1;
        x2 = LZ::add(d02, d13).normalized();
        x3 = LZ::sub(d02, d13).normalized();
      } else {
        const LZ a0 = LZ::add(x0, x1), a1 = LZ::sub(x0, x1), a2 = LZ::add(x2, x3), a3 = LZ::sub(x2, x3);  // stage 0: times 1
        const LZ p3 = LZ::mul(a3, w4);                                                                  // stage 1, second pair
        x0 = LZ::add(a0, a2).normalized();
        x2 = LZ::sub(a0, a2).normalized();
        x1 = LZ::add(a1, p3).normalized();
        x3 = LZ::sub(a1, p3).normalized();
      }
      lds.put(e0, x0);
      lds.put(e0 + st, x1);
      lds.put(e0 + 2 * st, x2);
      lds.put(e0 + 3 * st, x3);
    }
    __syncthreads();
  };
  // one radix-2 stage (odd stage counts): the radix-2 pass's butterfly without the carry step; in DIT it is the pass's last stage (outputs
  // leave through mul / canonical_wide, which take two-term limbs), in DIF its inputs come normalised out of the last round
  auto stage2 = [&](auto dif_c, const F* __restrict__ tw, int q) { radix2_stage<decltype(dif_c)::value, false, F, LZ>(lds, map, tw, a.L, q, a.unit_rounds); };
  const bool unit_round = a.unit_rounds && s0 == 0 && k >= 2;
  auto rounds = [&](auto dif_c, const F* __restrict__ tw) {
    constexpr bool D = decltype(dif_c)::value;
    if constexpr (D) {
      int q = k;
      for (; q >= 2; q -= 2) {
        if (q == 2 && unit_round) round4_unit(dif_c, tw);
        else round4(dif_c, tw, q - 2);
      }
      if (q == 1) stage2(dif_c, tw, 0);
    } else {
      int q = 0;
      for (; q + 2 <= k; q += 2) {
        if (q == 0 && unit_round) round4_unit(dif_c, tw);
        else round4(dif_c, tw, q);
      }
      if (q < k) stage2(dif_c, tw, q);
    }
  };
  if constexpr (PAIR) {
    rounds(std::true_type{}, a.tw);
    // between the two transforms: what the inverse transform's last pass would have stored (scaled, canonical) and the forward
    // transform's first pass would have loaded and unpacked -- each lane on the entries it will store, no traffic
    const LZ sc = LZ::unpack(a.scale);
    for (int e = tid; e < E; e += NT) {
      const LZ f = LZ::mul(lds.get(e), out_scale<F, LZ>(a, sc, map.global_index(e)));
      lds.put(e, LZ::unpack(f.canonical_wide().pack()));
    }
    __syncthreads();
    rounds(std::false_type{}, a.tw_fwd);
    store_tile<F, LZ>(lds, map, a, false);
  } else {
    if (!(ablate & 1)) rounds(std::integral_constant<bool, DIF>{}, a.tw);
    store_tile<F, LZ>(lds, map, a, a.scale_out, ablate);
  }
}

// out[i] = in[i] re-encoded from x * 2^256 to packed canonical x * R'
// Twiddle table of the lazy passes, STAGED: stage s (half-size m = 2^s) reads w^(j * n / 2m), j < 2^s, i.e. every 2^(L-1-s)-th
// entry of the natural table -- for the late stages of a tile, 64 lanes of a wave gathered 64 cache lines up to 64 KiB apart. Here
// every stage has its own contiguous run: out[(2^s - 1) + j] = storage form of in[j << (L - 1 - s)], 2^L - 1 entries in all (twice
// the natural table), so that neighbouring lanes (neighbouring j) read neighbouring 32-byte entries.
template <class F, class LZ>
__global__ __launch_bounds__(256) void k_to_lazy_table(const F* __restrict__ in, F* __restrict__ out, int L) {
  const size_t total = (size_t(1) << L) - 1;
  int32_t* top = reinterpret_cast<int32_t*>(out + total);  // limb 8 of every entry, behind the slots of limbs 0..7
  for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int s = 63 - __clzll((unsigned long long)(i + 1));  // stage: 2^s - 1 <= i < 2^(s+1) - 1
    const size_t j = i + 1 - (size_t(1) << s);
    const LZ v = LZ::from_fp(in[j << (L - 1 - s)]).canonical();
    F f;
#pragma unroll
    for (int k = 0; k < F::N; ++k) f.l[k] = (uint32_t)v.l[k];
    out[i] = f;
    top[i] = v.l[F::N];
  }
}

}  // inline namespace CSH_NTT_KERNEL_NS
}  // namespace csh
