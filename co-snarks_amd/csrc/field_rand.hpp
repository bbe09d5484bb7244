// F::rand over a ChaCha12 keystream, per candidate: the one function the kernels of field_rand.hip, the host self-test
// (csh_selftest_field_rand_host) and the window planner share. DESIGN.md section 3.3l.
//
// The rule (ark-ff 0.6.0 `Distribution<Fp> for Standard`, restated as in host/sharefile.hpp and the test suite's expand_seeded; ark-ff is
// not vendored and the reference commits no vector of it: PARITY UNPINNED):
//   candidate k of a stream = keystream bytes [32 k, 32 k + 32) = half (k & 1) of ChaCha12 block (k >> 1), read as little-endian limbs,
//   the top limb masked to the modulus bit size; it is accepted iff it is < p; the accepted limbs ARE the Montgomery representation (no
//   conversion); the i-th draw is the i-th accepted candidate. A 32-byte seed draw (rng.gen::<[u8; 32]>()) takes one candidate slot, so a
//   stream position counted in candidates describes every use mpc-core makes of these generators.
// Nothing here multiplies: a candidate is eight words, one mask and one eight-limb comparison.
#pragma once
#include <string.h>

#include "chacha.hpp"
#include "common.hpp"
#include "field.hpp"

namespace csh {

// limbs of candidate `half` of a block's sixteen keystream words; true iff accepted (< p), and then `out` is a canonical element
template <class F>
CSH_HD bool field_rand_candidate(const uint32_t words[16], int half, F& out) {
  static_assert(F::N == 8, "32-byte scalar fields only");
  constexpr uint32_t TOP_MASK = 0xffffffffu >> (256 - F::Params::BITS);
#pragma unroll
  for (int i = 0; i < 8; ++i) out.l[i] = words[8 * half + i];
  out.l[7] &= TOP_MASK;
  uint32_t m[8], t[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) m[i] = F::Params::MOD[i];
  return limbs_sub<8>(t, out.l, m) != 0;  // a borrow: out < p
}

// The window of candidates one pass of the three kernels looks at: [cand_lo, cand_hi), as the ChaCha blocks [blk_lo, blk_hi) with
// blk_lo = cand_lo >> 1 and blk_hi = (cand_hi + 1) >> 1; a candidate of those blocks outside the window counts as rejected. Workgroup b
// owns the blocks [blk_lo + b chunk, blk_lo + (b + 1) chunk) below blk_hi; chunk is a multiple of the workgroup's lanes.
constexpr int FRD_WG = 128;           // lanes of a workgroup: one ChaCha block = two candidates per lane and tile
constexpr int FRD_TILE = 2 * FRD_WG;  // candidates of a tile
constexpr int FRD_MAX_BLOCKS = 1024;  // workgroups of a window = lanes of the one-workgroup scan
constexpr uint64_t FRD_MAX_CAND = uint64_t(1) << 62;          // cand_begin above this is refused (positions stay far from wrapping)
static_assert(FRD_WINDOW_MIN == FRD_TILE, "the smallest window of tune \"field_rand_window\" (common.hpp) is one tile");

struct FrdWindow {
  uint32_t key[8];
  uint64_t cand_lo, cand_hi;
  uint64_t blk_lo, blk_hi, chunk;
  uint64_t need;  // accepted candidates wanted from this window: the write kernel stores output elements [0, need) only
  uint32_t blocks;
};

// p / 2^BITS, from the modulus: the chance that a masked candidate is accepted (BN254 0.756, BLS12-381 0.906, BLS12-377 0.583)
template <class F>
inline double field_rand_rate() {
  double v = 0.0;
  for (int i = 0; i < 8; ++i) v = v / 4294967296.0 + (double)F::Params::MOD[i];  // = MOD / 2^224, the top limb added last
  return v / (double)(uint64_t(1) << (F::Params::BITS - 224));
}

// Candidates of the window that is to yield `need` draws: the expectation plus eight standard deviations of the negative binomial count
// plus a tile, capped by tune "field_rand_window" (`cap`, 0 = none) and FRD_WINDOW_MAX. A window that falls short is followed by another.
inline uint64_t field_rand_window_cands(uint64_t need, double rate, uint64_t cap) {
  const double mean = (double)need / rate;
  double sd = 0.0, x = (double)need * (1.0 - rate);
  if (x > 0.0) {  // sqrt without <cmath> in device-visible headers: Newton, 40 steps from above
    sd = x < 1.0 ? 1.0 : x;
    for (int i = 0; i < 40; ++i) sd = 0.5 * (sd + x / sd);
  }
  double w = mean + 8.0 * sd / rate + (double)FRD_TILE;
  if (w > (double)FRD_WINDOW_MAX) w = (double)FRD_WINDOW_MAX;
  uint64_t c = (uint64_t)w;
  if (cap && c > cap) c = cap;
  return c < 1 ? 1 : c;
}

// the decomposition of [cand_lo, cand_lo + cands): blocks per workgroup in whole tiles, at most max_blocks workgroups
inline FrdWindow field_rand_plan(const uint8_t seed[32], uint64_t cand_lo, uint64_t cands, uint64_t need, int max_blocks) {
  FrdWindow w;
  memcpy(w.key, seed, 32);
  w.cand_lo = cand_lo, w.cand_hi = cand_lo + cands, w.need = need;
  w.blk_lo = w.cand_lo >> 1, w.blk_hi = (w.cand_hi + 1) >> 1;
  const uint64_t tiles = (w.blk_hi - w.blk_lo + FRD_WG - 1) / FRD_WG;
  if (max_blocks <= 0 || max_blocks > FRD_MAX_BLOCKS) max_blocks = FRD_MAX_BLOCKS;
  uint64_t g = tiles < (uint64_t)max_blocks ? tiles : (uint64_t)max_blocks;
  if (g < 1) g = 1;
  const uint64_t tiles_per = (tiles + g - 1) / g;
  w.chunk = tiles_per * FRD_WG;
  w.blocks = (uint32_t)((tiles + tiles_per - 1) / tiles_per);
  if (w.blocks < 1) w.blocks = 1;
  return w;
}

// The host loop the kernels are held against: the first n accepted candidates at or after cand_begin, through the same per-candidate
// function. Returns the index one past the last candidate consumed.
template <class F>
inline uint64_t field_rand_host(const uint8_t seed[32], uint64_t cand_begin, size_t n, F* out) {
  uint32_t key[8], words[16];
  memcpy(key, seed, 32);
  uint64_t k = cand_begin, have_blk = ~uint64_t(0);
  for (size_t i = 0; i < n;) {
    if ((k >> 1) != have_blk) chacha12_block(key, k >> 1, words), have_blk = k >> 1;
    F v;
    if (field_rand_candidate<F>(words, (int)(k & 1), v)) out[i++] = v;
    ++k;
  }
  return k;
}

}  // namespace csh
