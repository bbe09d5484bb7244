// The MSM planner: window widths, lane length, reduction segments and sort chunks of one MSM, from (n, scalar bits, occupancy) and, for
// bases with fixed-base tables, the table layout. Host code only (no kernel lives here) and pure: it reads the tune keys and the SIMD
// count of the calling thread's device and writes nothing -- the code that RUNS an MSM records csh_msm_last_params (msm_impl.hpp
// msm_record_params).
#pragma once
#include <math.h>

#include "common.hpp"
#include "msm_digits.hpp"
#include "msm_sort.hpp"

namespace csh {

// workgroup size of the accumulate kernels (the planner counts their waves)
#ifndef CSH_ACC_BLK
#define CSH_ACC_BLK 128
#endif
constexpr int ACC_BLK = CSH_ACC_BLK;

inline int choose_c(size_t n, int bits) {
  {
    const int c = tune().msm_c.load(std::memory_order_relaxed);
    if (c >= 2 && c <= 16) return c;
  }
  double best = 1e300;
  int best_c = 4;
  for (int c = 3; c <= 16; ++c) {  // digit codes are 15 bits + sign
    const double nb = double(size_t(1) << (c - 1));
    // per window: n mixed additions + the bucket stages, ~5 additions' worth per bucket (merge, running sums, segment multiple).
    // Re-checked after the one-round window reduction (profiles/archive/r02_g_csweep.log, r02_g_c1516.log): at 2^20 c = 15 and 16 tie
    // within 1-2 % (G1: 15 ahead, G2: 16 ahead), 2^17-2^19: 13 / 13 / 13-15, >= 2^21: 16.
    const double cost = windows_for(bits, c) * (double(n) + 5.0 * nb);
    if (cost < best) {
      best = cost;
      best_c = c;
    }
  }
  return best_c;
}

// L = sorted entries per accumulate lane. Every lane of every wave performs exactly L mixed additions and one wave of
// multiply-add code already saturates its SIMD's integer pipe, so the accumulate kernel takes ceil(waves / SIMDs) rounds of L
// additions: a sawtooth in L (measured, BN254 G1 2^22, 16 windows: L = 128 -> 8192 waves = 8.00 per SIMD, 4.82 ms; L = 112 ->
// 9.16 per SIMD = 10 rounds, 5.28 ms; L = 144 -> 5.36 ms; profiles/archive/r02_g_lsweep*.log). Longer lanes leave fewer partial sums
// to merge (n W / L of them, ~4.6e-5 addition rounds each); with few long rounds the last one is balanced less well (+~0.2 round).
// The plan takes the L in [16, 1024] with the smallest
//   (rounds(L) + 0.2) * L + 4.6e-5 * n * W / L.
// With 16 windows at the power-of-two sizes this lands on the former table (2^22 -> 128, 2^24 -> 256); it matters whenever
// n W / 64 is not a multiple of the SIMD count: 17 windows (BN254 at 2^20: L = 32 meant 8.5 waves per SIMD, 9 rounds of 32
// where 5 of 55 do, accumulate + merge 1.78 -> 1.73 ms; BN254 G2 5.48 -> 5.2 ms; 2^19: 1.33 -> 1.25 ms) and the arbitrary sizes of
// real proving keys.
// Small MSMs (round 4, profiles/archive/r04_zj_plan_sweep.log, r04_zk_short_lanes.log, interleaved): the round-count model above prices a
// SIMD with ONE wave on it, but a group whose accumulate kernel fits `occ` waves per SIMD (BN254 G1: 144 VGPRs -> 3) runs them
// interleaved, and with fewer than occ waves per SIMD in the whole launch the shorter lane wins: 2^15 c = 11 L = 16 -> 8 0.440 ->
// 0.371 ms, 2^16 c = 12 L = 23 -> 12 0.489 -> 0.426, 2^17 c = 13 L = 21 -> 12..16 0.569 -> 0.531..0.534; at 2^18 (L = 27 = exactly
// three waves per SIMD) and above the model's choice stands. Rule: never longer than the lane that fills occ waves per SIMD, down to 8
// entries (below ~6 10^5 entries the launch is latency, not throughput: left alone). occ = 1 (the G2 kernels, shared plans): unchanged.
inline uint32_t choose_lane_length(size_t n, int W, int occ = 1) {
  if (const int fl = tune().msm_l.load(std::memory_order_relaxed); fl > 0) return (uint32_t)fl;
  const double simds = (double)device_simds();
  const int wpb = ACC_BLK / 64;
  double best = 1e300;
  uint32_t best_L = 16;
  for (uint32_t L = 16; L <= 1024; ++L) {
    const uint64_t lanes = (n + L - 1) / L;
    const uint64_t waves = (uint64_t)W * ((lanes + ACC_BLK - 1) / ACC_BLK) * wpb;
    const double rounds = ceil((double)waves / simds);
    const double cost = (rounds + 0.2) * L + 4.6e-5 * (double)n * W / L;
    if (cost < best) {
      best = cost;
      best_L = L;
    }
    if (rounds <= 1) break;  // one round already: longer lanes only cost
  }
  // Round 5 (after balanced windows; profiles/archive/r05_f_ab_lane_floor.log, r05_g_ab_narrow_lane_length.log, r05_h_ab_lane_lengths_large.log,
  // interleaved, BN254 G1 / BLS12-381 G1 / Grumpkin): the lane that fills THREE waves per SIMD is the best or within 1 % of it on every G1
  // group at 2^15 .. 2^18, also where the kernel's registers only admit two (BLS12-381 G1 2^17: 14 against the former 20, -9.7 %; more,
  // shorter waves beat one full round), and from ~10^6 entries on a lane shorter than 12 entries loses to the partial sums it leaves the
  // merge kernel (2^16: 12 against 8, -4.3 % BN254 G1, -8.6 % BLS12-381 G1 against its former 11, -4.0 % Grumpkin); 2^15 stays at 8.
  const double entries = (double)n * W;
  if (occ >= 2 && entries >= 6e5) {
    uint32_t fill = (uint32_t)ceil(entries / (64.0 * simds * 3.0));
    const uint32_t floor_l = entries >= 1e6 ? 12 : 8;
    if (fill < floor_l) fill = floor_l;
    if (fill < best_L) best_L = fill;
  }
  return best_L;
}

// Window reduction: S segments of `per` consecutive buckets per window, `lanes_per_segment` lanes each (1, or 2 for the lane-pair
// form), a dependent chain of 2 per + ~21 point operations. One wave saturates its SIMD, so the stage takes
// ceil(W S lanes / 64 / SIMDs) rounds of that chain: as many segments as still fit ONE round (BN254 2^20: 17 windows x 3277
// segments of 5 buckets = 870 waves, chain 31 instead of 37 with the former 2048 x 8; a finer 4096 x 4 would need two rounds).
// tune "msm_seg_buckets" forces `per`.
inline uint32_t reduce_segments(uint32_t NB, int W, int lanes_per_segment) {
  int per = tune().msm_seg_buckets.load(std::memory_order_relaxed);
  if (per < 1 || per > 64) {
    const uint64_t s_max = (uint64_t)device_simds() * 64 / ((uint64_t)W * lanes_per_segment);
    per = (int)((NB + s_max - 1) / s_max);
    if (per < 2) per = 2;
  }
  const uint32_t S = (NB + per - 1) / per;
  return S < 1 ? 1 : S;
}

// Balanced windows (round 5). Uniform c-bit windows leave the top window whatever bits remain: 3 of 12 at 2^16 (c = 12, W = 22), 2 of 11 at
// 2^15, 8 of 13 at 2^17 / 2^18 -- a window that costs its n additions like every other, whose few buckets hold n / 4 .. n / 128 entries
// each (the oversized-bucket path: k_msm_giant_slices + k_msm_merge_giant 48 us of a 417 us MSM at 2^16, profiles/archive/r04_zp_msm_2p16_kernel_stats.csv)
// and whose bucket stage is sized like a full one. Here W windows share the bits + 1 bits evenly: c = ceil((bits + 1) / W), the low
// `wide` = bits + 1 - W (c - 1) windows take c bits, the others c - 1. c stays <= 16 (15-bit digit magnitudes). tune "msm_c" forces the
// uniform form (tests, A/B), "msm_balanced" = 0 turns this off, "msm_w" forces W.
struct WindowPlan {
  int c, W, wide;
};
inline WindowPlan choose_windows(size_t n, int bits) {
  const int forced_c = tune().msm_c.load(std::memory_order_relaxed);
  if ((forced_c >= 2 && forced_c <= 16) || tune().msm_balanced.load(std::memory_order_relaxed) == 0) {
    const int c = choose_c(n, bits);
    const int W = windows_for(bits, c);
    return {c, W, W};
  }
  const int total = bits + 1;  // one spare bit absorbs the final carry of the signed recoding
  auto balanced = [total](int W) {
    const int c = (total + W - 1) / W;
    return WindowPlan{c, W, total - W * (c - 1)};
  };
  const int forced_w = tune().msm_w.load(std::memory_order_relaxed);
  if (forced_w >= (total + 15) / 16 && forced_w <= MAX_WINDOWS && (total + forced_w - 1) / forced_w >= 3) return balanced(forced_w);
  // The number of windows is the one the uniform plan's width gives (choose_c: a cost model re-fitted by sweeps in rounds 2-4); the bits
  // are then spread evenly over them. Letting the cost model pick W freely was measured first and is worse where the model is least
  // exact: 2^19 took W = 18 (c = 15, 3 wide windows) for a modelled tie with the uniform W = 17 and ran 16 % slower, 2^18 W = 19 +1 %
  // (profiles/archive/r05_b_ab_balanced.log).
  return balanced(windows_for(bits, choose_c(n, bits)));
}
// width of window w / bit offset of window w in a plan
CSH_HD int window_bits(int c, int wide, int w) { return w < wide ? c : c - 1; }

// Merged-window mode (bases with fixed-base tables of g rows, table[k] = 2^(c W' k) P with W' = ceil(W / g)): the digit kernel
// still produces W windows of n codes, but window w is filed as row k = w / W' of sort window w' = w % W', every entry pointing
// at the precomputed multiple 2^(c W' k) P_i: the sort and bucket stages see W' windows of n g entries. g = W (one window, no
// Horner over windows afterwards) is the full merge; g = 2..4 keeps the sort in its efficient regime and halves / quarters the
// window reductions and the host Horner for g times the key memory.
struct MsmTable {
  int c, rows;            // window width and rows of the table (Bases::table_c, table_W)
  size_t stride, offset;  // points per row (Bases::n) and the first point of the call
};
struct MsmPlan {
  MsmParams dig;  // n points, W windows: digit kernel
  MsmParams srt;  // sort + bucket stages; merged: n g entries per window, W' windows. Plain plans have dig == srt
  bool merged;
};

// partial slots per window of the accumulate kernels (slot = bucket + lane) and the reduction segments the scratch is sized for, from
// p.NB, p.W and p.L: the one place both are decided -- msm_plan_tail below, and the device unit test of the bucket stage
// (msm_impl.hpp msm_buckets_selftest_t), which takes its lane length from the caller
inline void msm_plan_slots(MsmParams& p, uint64_t entries) {
  const uint32_t max_lanes = (uint32_t)((entries + p.L - 1) / p.L);
  p.tmax = p.NB + max_lanes + 2;  // partial slots per window: slot = bucket + lane
  p.S = reduce_segments(p.NB, p.W, 1);
}

// what both kinds of plan derive from (entries per window, W, NB): lane length, partial slots, reduction segments, sort chunks
inline void msm_plan_tail(MsmParams& p, uint64_t entries, int occ) {
  p.L = choose_lane_length((size_t)entries, p.W, occ);
  // Narrow windows (balanced plan) hold twice the entries per bucket; giving their lanes 2 L entries would leave k_msm_merge the same
  // number of partial sums per bucket as in a wide window. Measured (profiles/archive/r05_g_ab_narrow_lane_length.log, interleaved, 2^14 .. 2^18,
  // three groups): +6 .. +26 % -- at these sizes the accumulate launch is a dependent chain per lane, and doubling it costs more than the
  // merge saves. One length is the default; tune "msm_variant" bit 6 (64) selects the doubled form (kept parity-tested for A/B).
  p.Ln = (p.wide < p.W && p.L <= 32 && (tune().msm_variant.load(std::memory_order_relaxed) & 64) != 0) ? 2 * p.L : p.L;
  msm_plan_slots(p, entries);
  uint64_t ch = 512 / (uint64_t)p.W;
  const uint64_t by_size = entries / (2ull * p.NB);
  if (ch > by_size) ch = by_size;
  if (ch < 1) ch = 1;
  p.CH = (uint32_t)ch;
  p.chunk_len = (uint32_t)((entries + ch - 1) / ch);
}

// The plan of an n-point MSM. occ: accumulate waves of the group's kernel that fit one SIMD (1: shared plans, no device). table
// (nullable): the handle's fixed-base tables -- merged-window mode.
inline MsmPlan msm_plan(size_t n, int scalar_bits, int mont, int occ, const MsmTable* table = nullptr) {
  MsmPlan m;
  m.merged = table != nullptr;
  MsmParams& d = m.dig;
  d = MsmParams{};  // no lanes, segments or chunks, no remap, rows in window order
  d.n = (uint32_t)n;
  d.mont = mont;
  if (!table) {
    const WindowPlan wp = choose_windows(n, scalar_bits);
    d.c = wp.c;
    d.W = wp.W;
    d.wide = wp.wide;
    d.NB = 1u << (d.c - 1);
    msm_plan_tail(d, n, occ);
    m.srt = d;
    return m;
  }
  d.c = table->c;
  d.W = windows_for(scalar_bits, d.c);
  d.wide = d.W;  // table rows are 2^(c W' k) P: uniform windows
  d.NB = 1u << (d.c - 1);
  const int g = table->rows < 1 ? 1 : (table->rows > d.W ? d.W : table->rows);
  const int wp = (d.W + g - 1) / g;
  d.dig_g = (uint32_t)g;
  d.dig_wp = (uint32_t)wp;
  MsmParams& p = m.srt;
  p = MsmParams{};
  const uint64_t n2 = (uint64_t)n * g;
  p.n = (uint32_t)n2;
  p.c = d.c;
  p.W = wp;
  p.wide = p.W;
  p.NB = d.NB;
  p.mont = mont;
  p.remap_n = (uint32_t)n;
  p.remap_stride = (uint32_t)table->stride;
  p.remap_off = (uint32_t)table->offset;
  msm_plan_tail(p, n2, occ);
  return m;
}

}  // namespace csh
