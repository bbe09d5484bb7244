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
#endif

}  // namespace csh
