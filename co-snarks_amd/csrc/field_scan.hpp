// Building block of the field scans (field_scan.hip): block-level scan / reduction of field elements in the signed lazy field
// (field29.hpp), and the one inversion a batch inverse needs. DESIGN.md section 3.3b.
//
// Scales. An arkworks element is x R (R = 2^256); the lazy product is mul(a, b) = a b / R' with R' = 2^261 = 32 R. Two encodings of a
// field value v are in use and every routine below says which it takes:
//   "R scale"   v R   : what unpack() of a loaded element gives, and what canonical_wide().pack() stores;
//   "R' domain" v R'  : closed under mul(), so partial products combine without any bookkeeping. unpack(x).times32() is an R'-domain
//                       representative of a loaded x (value < 32 p), to_domain() converts a lazy R-scale value with one multiplication.
// mul(R scale, R' domain) is R scale again. A lane's run is the chain acc = x0; acc = mul(acc, x_e.times32()): a product of k loaded
// operands with exactly k - 1 of them scaled, as k_vec_mul does for k = 2. times32() is only ever applied to LOADED (canonical) operands:
// on a reduction output (value up to p / (1 - p / 2^256), 1.83 p on BLS12-381 Fr) it would give 58 p, and products of two such values
// leave the range the reduction was derived for after three levels of a tree. Everything that crosses lanes is therefore in the R' domain,
// where the value bound is stable (alpha' = alpha beta p / R' + 1 < 1.06).
#pragma once
#include "common.hpp"
#include "field.hpp"
#include "field29.hpp"

namespace csh {

// lazy R-scale value -> R' domain (one multiplication by 32 R' mod p, the constant of from_fp())
template <class LP, class F32>
CSH_HD FpS<LP, F32> to_domain(const FpS<LP, F32>& a) {
  FpS<LP, F32> c;
#pragma unroll
  for (int i = 0; i < LP::NL; ++i) c.l[i] = (int32_t)LP::TO_LAZY[i];
  return FpS<LP, F32>::mul(a, c);
}
// R' domain -> lazy R-scale value (one multiplication by R mod p)
template <class LP, class F32>
CSH_HD FpS<LP, F32> from_domain(const FpS<LP, F32>& a) {
  FpS<LP, F32> c;
#pragma unroll
  for (int i = 0; i < LP::NL; ++i) c.l[i] = (int32_t)LP::FROM_LAZY[i];
  return FpS<LP, F32>::mul(a, c);
}

// ---- a^(p - 2) in the R' domain: fixed 4-bit windows, 16 table products + ceil(NL B / 4) x (4 squarings + at most 1 product) -------------
// The table and the exponent are indexed at run time, so they live in memory the caller names (LDS on the device, the stack on the host):
// in registers they would go to scratch. a: a reduction output (normalised limbs). 0 -> 0.
template <class LZ>
struct InvScratch {
  LZ tab[16];
  uint32_t e[LZ::NL];  // p - 2 in B-bit limbs
};
template <class LP, class F32>
CSH_HD FpS<LP, F32> lazy_inv(const FpS<LP, F32>& a, InvScratch<FpS<LP, F32>>& s) {
  using LZ = FpS<LP, F32>;
  constexpr int NL = LP::NL, B = LP::B;
  int32_t borrow = 2;
#pragma unroll 1
  for (int i = 0; i < NL; ++i) {
    int32_t v = (int32_t)LP::MOD[i] - borrow;
    borrow = 0;
    if (v < 0 && i < NL - 1) {
      v += (int32_t)1 << B;
      borrow = 1;
    }
    s.e[i] = (uint32_t)v;
  }
  s.tab[0] = LZ::one();
  s.tab[1] = a;
#pragma unroll 1
  for (int k = 2; k < 16; ++k) s.tab[k] = LZ::mul(s.tab[k - 1], a);
  LZ acc = LZ::one();
  bool started = false;  // leading zero windows: nothing to square yet
#pragma unroll 1
  for (int w = (NL * B + 3) / 4 - 1; w >= 0; --w) {
    const int bit = 4 * w, li = bit / B, off = bit % B;
    uint32_t d = s.e[li] >> off;
    if (off > B - 4 && li + 1 < NL) d |= s.e[li + 1] << (B - off);
    d &= 15u;
    if (started) {
#pragma unroll 1
      for (int q = 0; q < 4; ++q) acc = LZ::sqr(acc);
    }
    if (d) {
      acc = started ? LZ::mul(acc, s.tab[d]) : s.tab[d];
      started = true;
    }
  }
  return acc;
}

// ---- weighted sums: the algebra of a first-order linear recurrence s_i = a_i + w s_(i-1) ---------------------------------------------------
// pw.p[j] = w^(2^j), R' domain, canonical and packed: every length in the decomposition is a power of two, so these are all the powers
// (polynomial evaluation: w = the point; division by (X - r): w = 1 / r).
constexpr int SCAN_POWERS = 32;
template <class F>
struct PowTable {
  F p[SCAN_POWERS];
};
template <class LZ, class F>
CSH_HD PowTable<F> pow_table(LZ sq) {  // sq: R' domain; about 30 squarings, on the host: cheaper than a launch
  PowTable<F> pw;
  for (int j = 0; j < SCAN_POWERS; ++j) {
    pw.p[j] = sq.canonical().pack();
    sq = LZ::sqr(sq);
  }
  return pw;
}
// Two adjacent segments of the recurrence, `lo` the earlier one, each summarised by the s it ends with when it starts from 0: the pair
// ends with hi + w^(length of hi) lo. wpow: that power, R' domain, a loaded (canonical) value or a product; lo, hi: R scale.
// Bounds. Limbs: lo is a product's first operand, so it may be one two-term sum (LIM2); the sum has three terms' limbs at most
// (hi may itself be a two-term sum: 3 x 2^B < 2^31) and leaves with one carry step as a normalised value. Value: a product of a
// first operand within (-8 p, 8 p) and a wpow below 1.04 p lies in (-0.13 p, 1.13 p) (p / R' < 1 / 67 for the three scalar fields), so
// every level adds at most 1.13 p to |hi|. A lane's run ends within (-2.13 p, 2.13 p); after the 6 levels of a wave the operands of the
// products have stayed below 2.13 + 5 x 1.13 = 7.8 p and the result is below 8.9 p, where fold_top() (good to 64 p) brings it back into
// (-p, 2 p) before the at most 4 levels across waves (2 + 4 x 1.13 p). The callers below fold where this paragraph says.
template <class LZ>
CSH_HD LZ wsum_combine(const LZ& lo, const LZ& hi, const LZ& wpow) {
  return LZ::add(hi, LZ::mul(lo, wpow)).normalized();
}

#if defined(__HIPCC__)
template <class LZ>
__device__ __forceinline__ LZ lz_shfl_up(const LZ& v, int d) {
  LZ r;
#pragma unroll
  for (int i = 0; i < LZ::NL; ++i) r.l[i] = __shfl_up(v.l[i], d);
  return r;
}
template <class LZ>
__device__ __forceinline__ LZ lz_shfl_down(const LZ& v, int d) {
  LZ r;
#pragma unroll
  for (int i = 0; i < LZ::NL; ++i) r.l[i] = __shfl_down(v.l[i], d);
  return r;
}

// ---- block reduction under an associative operation with a level: op(lo, hi, k) combines `lo` with the aggregate `hi` of the 2^k
// positions behind it (lanes for k < 6, waves from k = 6 on). A product ignores k; a polynomial evaluation multiplies hi by x^(len 2^k).
// Every thread of the block calls it; blockDim.x = 64 .. 1024 lanes, a power of two. The result is valid in thread 0 only. lds: 16 elements.
template <class LZ, class Op>
__device__ __forceinline__ LZ block_reduce(LZ v, LZ* lds, const Op& op) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
#pragma unroll 1
  for (int k = 0; k < 6; ++k) v = op(v, lz_shfl_down(v, 1 << k), k);  // lanes whose partner is out of range get their own value: never used
  v = op.settle(v);
  __syncthreads();  // the previous user of lds is done with it
  if (lane == 0) lds[wv] = v;
  __syncthreads();
  if (wv == 0) {
    v = lane < nw ? lds[lane] : op.identity();
#pragma unroll 1
    for (int k = 0; (1 << k) < nw; ++k) v = op(v, lz_shfl_down(v, 1 << k), 6 + k);
    v = op.settle(v);
  }
  return v;
}
template <class LZ>
struct MulOp {
  __device__ __forceinline__ LZ operator()(const LZ& lo, const LZ& hi, int) const { return LZ::mul(lo, hi); }
  __device__ __forceinline__ LZ settle(const LZ& v) const { return v; }
  __device__ __forceinline__ LZ identity() const { return LZ::one(); }
};

// ---- block scan under multiplication ------------------------------------------------------------------------------------------------
// Lane totals by shuffles (9 per step: one element is 9 limbs), wave totals through LDS and a second shuffle scan in wave 0.
// REV = false: exclusive prefix over the block's threads in thread order; REV = true: exclusive suffix (the same code with lane and wave
// order mirrored). v: R' domain. carry: what precedes (follows) the block, R' domain or R scale -- the result and *total = carry x
// (product of all v) have the carry's scale. Every thread of the block calls it; three barriers inside.
template <class LZ>
struct ScanLds {
  LZ wtot[16];
  LZ wpre[17];
};
template <bool REV, class LZ>
__device__ __forceinline__ LZ block_excl_scan_mul(const LZ& v, const LZ& carry, ScanLds<LZ>& s, LZ* total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int ll = REV ? 63 - lane : lane, wl = REV ? nw - 1 - wv : wv;
  LZ incl = v;
#pragma unroll 1
  for (int d = 1; d < 64; d <<= 1) {
    const LZ m = LZ::mul(incl, REV ? lz_shfl_down(incl, d) : lz_shfl_up(incl, d));
    if (ll >= d) incl = m;
  }
  __syncthreads();  // the previous call's readers are done with s
  if (ll == 63) s.wtot[wl] = incl;
  __syncthreads();
  if (wv == 0) {
    LZ x = lane < nw ? s.wtot[lane] : LZ::one();
#pragma unroll 1
    for (int d = 1; d < 16; d <<= 1) {
      const LZ m = LZ::mul(x, lz_shfl_up(x, d));
      if (lane >= d) x = m;
    }
    x = LZ::mul(x, carry);
    if (lane < nw) s.wpre[lane + 1] = x;
    if (lane == 0) s.wpre[0] = carry;
  }
  __syncthreads();
  const LZ base = s.wpre[wl];
  const LZ m = LZ::mul(REV ? lz_shfl_down(incl, 1) : lz_shfl_up(incl, 1), base);
  *total = s.wpre[nw];
  return ll == 0 ? base : m;
}
// ---- block scan under the weighted sum ------------------------------------------------------------------------------------------------
// step^(lane), R' domain, in every wave: what a lane's value is weighted with when something from before its wave is added to it
template <class LZ>
__device__ __forceinline__ LZ lane_powers(const LZ& step) {
  const int lane = threadIdx.x & 63;
  LZ x = step;
#pragma unroll 1
  for (int d = 1; d < 64; d <<= 1) {
    const LZ m = LZ::mul(x, lz_shfl_up(x, d));
    if (lane >= d) x = m;
  }
  const LZ up = lz_shfl_up(x, 1);
  return lane == 0 ? LZ::one() : up;
}
// Exclusive prefix over the block's threads in thread order, the shape of block_excl_scan_mul: lane totals by shuffles (9 per step),
// wave totals through LDS, a second shuffle scan in wave 0. Every thread holds the summary v of 2^base positions (R scale, limbs of
// at most one two-term sum, |v| < 2.13 p); carry: the s that precedes the block (the same limits, |carry| < 3.2 p). The result is
// the s in front of the thread's positions and *total the s the block ends with; lane_w = w^(2^base lane) (lane_powers, or a table of
// them). Bounds as derived above wsum_combine: the carry enters wave 0's total as one more level (2 + 1.13 + 4 x 1.13 < 7.7 p), and
// the result is a folded prefix plus one product: within (-1.2 p, 3.2 p), limbs of one two-term sum -- a product's first operand.
// Every thread of the block calls it; three barriers inside.
template <class LZ, class Pw>
__device__ __forceinline__ LZ block_excl_scan_wsum(const LZ& v, const LZ& carry, const LZ& lane_w, const Pw& pw, int base, ScanLds<LZ>& s,
                                                   LZ* total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
  LZ incl = v;
#pragma unroll 1
  for (int k = 0; k < 6; ++k) {
    const LZ m = wsum_combine(lz_shfl_up(incl, 1 << k), incl, LZ::unpack(pw.p[base + k]));
    if (lane >= (1 << k)) incl = m;
  }
  incl = incl.fold_top();
  __syncthreads();  // the previous call's readers are done with s
  if (lane == 63) s.wtot[wv] = incl;
  __syncthreads();
  if (wv == 0) {
    LZ x = lane < nw ? s.wtot[lane] : LZ::zero();
    const LZ first = wsum_combine(carry, x, LZ::unpack(pw.p[base + 6]));  // the carry is a wave in front of wave 0
    if (lane == 0) x = first;
#pragma unroll 1
    for (int k = 0; k < 4; ++k) {
      const LZ m = wsum_combine(lz_shfl_up(x, 1 << k), x, LZ::unpack(pw.p[base + 6 + k]));
      if (lane >= (1 << k)) x = m;
    }
    x = x.fold_top();
    if (lane < nw) s.wpre[lane + 1] = x;
    if (lane == 0) s.wpre[0] = carry;
  }
  __syncthreads();
  const LZ before = s.wpre[wv];
  const LZ m = LZ::add(lz_shfl_up(incl, 1), LZ::mul(before, lane_w));
  *total = s.wpre[nw];
  return lane == 0 ? before : m;
}
#endif


}  // namespace csh
