// Per-element expressions of the share-vector kernels (vec_ops.hip), one definition each. The kernels call them inside their
// grid-stride loops; the host self-test (selftest.hip, limb-bound contract checked on every call) calls the very same functions, so a
// change of an expression here is a change of what the self-test runs. All operands and results are arkworks-Montgomery elements of F;
// the products run in the signed lazy field (field29.hpp), one operand scaled by 2^5 = R'/2^256.
#pragma once
#include "field.hpp"
#include "field29.hpp"

namespace csh {

// a * b (k_vec_mul; k_vec_mul_table with b = the table entry)
template <class F>
CSH_HD F elem_mul(const F& a, const F& b) {
  using LZ = typename LazyOf<F>::type;
  return LZ::mul(LZ::unpack(a), LZ::unpack(b).times32()).canonical_wide().pack();
}

// a * b - c (k_vec_mul_sub; h = a b - c, reduction.rs:176-190): the difference is limb-wise on the reduced product
template <class F>
CSH_HD F elem_mul_sub(const F& a, const F& b, const F& c) {
  using LZ = typename LazyOf<F>::type;
  return LZ::sub(LZ::mul(LZ::unpack(a), LZ::unpack(b).times32()), LZ::unpack(c)).canonical_wide().pack();
}

// Rep3 local multiplication (mpc-core rep3/arithmetic/ops.rs:69-76) + mask[i] - sub[i] (k_rep3_local_mul); mask and sub are the
// operand vectors or NULL
template <class F>
CSH_HD F elem_rep3_local_mul(const F& la, const F& lb, const F& ra, const F& rb, const F* mask, const F* sub, size_t i) {
  // a*a' + a*b' + b*a' = la*(ra+rb) + lb*ra  (2 multiplications instead of 3; same field element)
  //   both products accumulate double-width before ONE reduction
  using LZ = typename LazyOf<F>::type;
  const LZ xa = LZ::unpack(la), xb = LZ::unpack(lb), ya = LZ::unpack(ra), yb = LZ::unpack(rb);
  LZ r = LZ::reduce(LZ::mul_add_wide(xa, LZ::add(ya, yb).times32(), xb, ya.times32()));
  if (mask) r = LZ::add(r, LZ::unpack(mask[i]));
  if (sub) r = LZ::sub(r, LZ::unpack(sub[i]));
  return r.canonical_wide().pack();
}

// a * x + b * y of a Rep3 share {a, b} and a party's translation points (k_rep3_to_shamir; bridges/rep3_to_shamir.rs:43-62)
template <class F>
CSH_HD F elem_rep3_to_shamir(const F& a, const F& b, const F& x, const F& y) {
  using LZ = typename LazyOf<F>::type;
  const LZ lx = LZ::unpack(x).times32(), ly = LZ::unpack(y).times32();
  return LZ::reduce(LZ::mul_add_wide(LZ::unpack(a), lx, LZ::unpack(b), ly)).canonical_wide().pack();
}

// a + u (b - a), the multilinear fold of one pair (k_mle_fold, k_mle_fold_rounds; partially_evaluate, co_sumcheck_prover.rs:34-98).
// ud: the challenge in the R' domain (u R' mod p, canonical and packed: fr_to_rprime() of fr_entry.hpp, once per call on the host), so
// mul(b - a, ud) comes out at the operands' scale and no loaded operand is scaled. fold_step is the same on lazy values, for the rounds that
// stay on chip: a, b within (-1.1 p, 2.1 p) with limbs 0..NL-2 in [0, 2^B) (loaded, or an earlier fold_step); bounds in mle_fold.hpp.
template <class LZ>
CSH_HD LZ fold_step(const LZ& a, const LZ& b, const LZ& ud) {
  return LZ::add(a, LZ::mul(LZ::sub(b, a), ud)).fold_top();
}
template <class F>
CSH_HD F elem_fold(const F& a, const F& b, const F& ud) {
  using LZ = typename LazyOf<F>::type;
  return fold_step(LZ::unpack(a), LZ::unpack(b), LZ::unpack(ud)).canonical_narrow().pack();
}

}  // namespace csh
