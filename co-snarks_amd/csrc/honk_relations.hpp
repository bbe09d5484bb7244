// The loop between two folds of co-noir's UltraHonk sumcheck prover (honk_relations.hip):
// SumcheckProverRound::compute_univariate_inner, co-noir/ultrahonk/src/decider/sumcheck/sumcheck_round_prover.rs:224-255, for the four
// relations every UltraHonk circuit exercises -- UltraArithmeticRelation (relations/ultra_arithmetic_relation.rs:126-175),
// UltraPermutationRelation (permutation_relation.rs:93-167), LogDerivLookupRelation (logderiv_lookup_relation.rs:77-183, :266-309) and
// DeltaRangeConstraintRelation (delta_range_constraint_relation.rs:112-177) -- and GateSeparatorPolynomial::new's beta_products
// (decider/types.rs:53-67). What the kernels and the host self-test (selftest.hip, limb-bound checks on) share: the column order, the
// argument struct and how the host fills it in, the extension of an edge to a point, the four relations at one point in the scalar shape
// of the reference's verify_accumulate, the per-edge skips, and the derivation of the lazy-field bounds.
//
// Column order of cols[36] (part of the ABI, include/cosnarks_hip.h):
//    0.. 7  witness          w_l, w_r, w_o, w_4, z_perm, lookup_inverses, lookup_read_counts, lookup_read_tags
//    8..12  shifted witness  w_l, w_r, w_o, w_4, z_perm
//   13..35  precomputed      q_m, q_c, q_l, q_r, q_o, q_4, q_arith, q_delta_range, q_lookup, sigma_1..4, id_1..4, table_1..4,
//                            lagrange_first, lagrange_last
// Accumulator order of acc[57]: arith.r0 (6), arith.r1 (5), perm.r0 (6), perm.r1 (3), lookup.r0 (5), lookup.r1 (5), lookup.r2 (3),
// delta.r0..r3 (6 each); entry i of an accumulator is its evaluation at the point i.
//
// Decomposition. A lane takes ONE point k (0..5) of one edge: it extends each column's pair (v0, v1) to v0 + k (v1 - v0) and evaluates
// scalars, so nothing of length 7 lives in registers. All eleven subrelations are evaluated at all six points; what lies at or behind an
// accumulator's length (the reference computes seven and adds the first `len`) is dropped when the result is written.
//
// Scale. Elements are arkworks-Montgomery (R = 2^256), R' = 2^261 = 32 R is the lazy field's radix. A product of two loaded (or derived)
// operands is hr_mul(x, y) = mul(x.times32(), y) = x y 32 / R' = x y / R: Montgomery again. A product by a constant of the call (beta,
// public_input_delta, -1/2) is hr_mulc(x, c') with c' = c R' mod p (fr_to_rprime, once per call on the host): x c R' / R', the operand's
// scale, nothing scaled by 32. gamma, 1, 2, 3 are only ever added: plain Montgomery.
//
// Bounds. p / R' < 1 / 64 for the three scalar fields; T = the top limb of p, below 2^23. Classes of a value that stays on chip:
//   U  unpack() of a canonical element: limbs in [0, 2^B), value in [0, p).
//   F  fold_top() output: limbs 0..NL-2 in [0, 2^B), small signed top limb, value in (-p - eps, 2 p + eps), eps < 1e-4 p. U is inside F.
//   M  hr_mulc() output before any fold: limbs as F, value in (-0.07 p, 1.07 p). M is inside F.
//   extension  hr_extend(v0, v1, k), k <= 5, v0, v1 in U: (1 - k) v0 + k v1 through one signed 64-bit carry chain (the limb-wise form
//     would reach 6 2^29 > 2^31): limbs 0..NL-2 in [0, 2^B), value in (-4 p, 5 p). fold_top() (|k| <= 5 of the 64 it is exact for): F.
//     Every column value a relation sees is F.
//   sums  at most three terms of F (and U, M) are added or subtracted limb-wise between two fold_top(): |limb| < 3 2^29 < 2^31, |value|
//     < 6.1 p; the one four-term sum (arith.r1: w_l + w_4 - w_l_shift + q_m) has one negative term: limbs in (-2^29, 3 2^29), |value|
//     < 8.1 p. fold_top(): F.
//   hr_mul(x, y), x a sum of at most two F (|x| < 4.03 p, any limbs: times32() carries in 64 bits), y in F.
//     x.times32(): limbs 0..NL-2 in [0, 2^B), |top limb| < 4.03 * 32 * (T + 1); with the largest T of the three fields (BLS12-381:
//     0x73eda7) that is 979.8e6 < LIM2 = 2^30 + 16 = 1073.7e6, the bound mul() checks on its first operand. y has |limb| <= 2^B < LIM1. |32 x y| < 32 * 4.03 * 2.01 p^2 = 259.3 p^2, so the reduced product lies in
//     (-259.3 p^2 / R', p + 259.3 p^2 / R') inside (-4.06 p, 5.06 p): inside mul's (-8 p, 8 p) and fold_top()'s exact range. fold_top(): F.
//     hr_mul always folds: F x F -> F, and a chain of any length (the permutation's (z_perm + lagrange_first) t_1 s t_2 t_3 t_4 is the
//     deepest, five products behind one another) has the same bound at every step.
//   hr_mulc(x, c'), x a sum of at most two F (limbs < 2^30 = LIM2's range, |x| < 4.03 p), c' in U: |x c'| < 4.03 p^2: M.
//   accumulators  acc_s in F; a term is F (hr_mul's output, or fold_top() of a difference of two): acc_s + term has limbs < 2^30, value in
//     (-2.1 p, 4.1 p); fold_top() after EVERY edge returns F. The grid-stride loop is the one place where a bound could depend on the
//     pass count, and with the fold per pass it does not: 2^27 passes of p - 1 leave acc_s in F like one. The workgroup's sum (42 lanes
//     per point) adds F to F and folds after every addition, the same step; its result leaves through canonical_narrow().pack() (F is
//     its input range). The finishing launch adds canonical elements with the exact modular F::add.
//   pow table  out[i] = the product of betas[b] over the set bits of i: the running product starts at 1 (U) and takes hr_mulc by beta_b':
//     M at every step, whatever m. canonical_wide().
// Field addition is exact and every output is canonical, so the 57 words do not depend on how edges are dealt to lanes, workgroups or
// passes. No bound depends on the range, the stride or the data. The only floating point is fold_top()'s quotient estimate.
#pragma once
#include "honk_stage.hpp"

namespace csh {

constexpr int HR_COLS = 36;
constexpr int HR_SUBRELATIONS = 11;
constexpr int HR_MAX_BETAS = 28;
constexpr int HR_ALL = 15;  // all four relations in one launch

enum HrCol : int {
  HR_W_L = 0, HR_W_R, HR_W_O, HR_W_4, HR_Z_PERM, HR_LOOKUP_INVERSES, HR_LOOKUP_READ_COUNTS, HR_LOOKUP_READ_TAGS,
  HR_W_L_SHIFT, HR_W_R_SHIFT, HR_W_O_SHIFT, HR_W_4_SHIFT, HR_Z_PERM_SHIFT,
  HR_Q_M, HR_Q_C, HR_Q_L, HR_Q_R, HR_Q_O, HR_Q_4, HR_Q_ARITH, HR_Q_DELTA_RANGE, HR_Q_LOOKUP,
  HR_SIGMA_1, HR_SIGMA_2, HR_SIGMA_3, HR_SIGMA_4, HR_ID_1, HR_ID_2, HR_ID_3, HR_ID_4,
  HR_TABLE_1, HR_TABLE_2, HR_TABLE_3, HR_TABLE_4, HR_LAGRANGE_FIRST, HR_LAGRANGE_LAST
};
enum HrSub : int { HR_ARITH_0 = 0, HR_ARITH_1, HR_PERM_0, HR_PERM_1, HR_LOOKUP_0, HR_LOOKUP_1, HR_LOOKUP_2, HR_DELTA_0, HR_DELTA_1, HR_DELTA_2, HR_DELTA_3 };

// The constants of a call beside HsArgs's; hr_consts finds a.one set (hs_args)
template <class F>
struct HrArgs : HsArgs<F, HR_COLS> {
  F betad, pidd, neg_halfd;  // beta R', public_input_delta R', (-1/2) R'
  F gamma, one, two, three;  // arkworks-Montgomery
};
template <class F>
inline void hr_consts(HrArgs<F>& a, const uint64_t* params) {
  a.betad = fr_to_rprime(fr_load<F>(params));
  a.gamma = fr_load<F>(params + 4);
  a.pidd = fr_to_rprime(fr_load<F>(params + 8));
  a.two = F::add(a.one, a.one);
  a.three = F::add(a.two, a.one);
  a.neg_halfd = fr_to_rprime(F::neg(F::inv(a.two)));
}

// (1 - k) v0 + k v1 for v0, v1 in U and 0 <= k <= 5, carried in 64 bits, folded: F
template <class LZ>
CSH_HD LZ hr_extend(const LZ& v0, const LZ& v1, int k) {
  LZ r;
  int64_t c = 0;
#pragma unroll
  for (int i = 0; i < LZ::NL - 1; ++i) {
    const int64_t t = (int64_t)v0.l[i] + (int64_t)k * (int64_t)(v1.l[i] - v0.l[i]) + c;
    r.l[i] = (int32_t)((uint32_t)t & (((uint32_t)1 << LZ::B) - 1u));
    c = t >> LZ::B;
  }
  r.l[LZ::NL - 1] = (int32_t)((int64_t)v0.l[LZ::NL - 1] + (int64_t)k * (int64_t)(v1.l[LZ::NL - 1] - v0.l[LZ::NL - 1]) + c);
  return r.fold_top();
}
// x y at the operands' scale; x: at most two terms of F, y: F. -> F
template <class LZ>
CSH_HD LZ hr_mul(const LZ& x, const LZ& y) {
  return LZ::mul(x.times32(), y).fold_top();
}
// x c for a constant of the call in the R' domain; x: at most two terms of F. -> M
template <class LZ>
CSH_HD LZ hr_mulc(const LZ& x, const LZ& cd) {
  return LZ::mul(x, cd);
}

template <class F>
using HrPoint = HsPoint<HrArgs<F>>;  // the per-point view of one edge (honk_stage.hpp)

// ---- the four relations at one point, in the shape of the reference's verify_accumulate; `sc` = the edge's scaling factor (U) ---------
// ultra_arithmetic_relation.rs:177-223
template <class F, class LZ>
CSH_HD void hr_arith_at(const HrPoint<F>& p, const LZ& sc, LZ& r0, LZ& r1) {
  const LZ qa = p.at(HR_Q_ARITH), w_l = p.at(HR_W_L), w_4 = p.at(HR_W_4), q_m = p.at(HR_Q_M), one = p.one();
  {
    const LZ w_r = p.at(HR_W_R);
    LZ t = hr_mul(hr_mul(q_m, w_r), w_l);
    t = hr_mulc(hr_mul(LZ::sub(qa, LZ::unpack(p.a.three)), t), LZ::unpack(p.a.neg_halfd));
    t = LZ::add(LZ::add(t, hr_mul(p.at(HR_Q_L), w_l)), hr_mul(p.at(HR_Q_R), w_r)).fold_top();
    t = LZ::add(LZ::add(t, hr_mul(p.at(HR_Q_O), p.at(HR_W_O))), hr_mul(p.at(HR_Q_4), w_4)).fold_top();
    t = LZ::add(LZ::add(t, p.at(HR_Q_C)), hr_mul(LZ::sub(qa, one), p.at(HR_W_4_SHIFT))).fold_top();
    r0 = hr_mul(hr_mul(t, qa), sc);
  }
  LZ u = LZ::add(LZ::sub(w_l, p.at(HR_W_L_SHIFT)), LZ::add(w_4, q_m)).fold_top();
  u = hr_mul(LZ::sub(qa, LZ::unpack(p.a.two)), u);
  u = hr_mul(LZ::sub(qa, one), u);
  r1 = hr_mul(hr_mul(u, qa), sc);
}
// permutation_relation.rs:169-237
template <class F, class LZ>
CSH_HD void hr_perm_at(const HrPoint<F>& p, const LZ& sc, LZ& r0, LZ& r1) {
  const LZ betad = LZ::unpack(p.a.betad), gamma = LZ::unpack(p.a.gamma);
  LZ num = sc, den = sc;
  for (int j = 0; j < 4; ++j) {
    const LZ wg = LZ::add(p.at(HR_W_L + j), gamma);
    num = hr_mul(num, LZ::add(hr_mulc(p.at(HR_ID_1 + j), betad), wg).fold_top());
    den = hr_mul(den, LZ::add(hr_mulc(p.at(HR_SIGMA_1 + j), betad), wg).fold_top());
  }
  const LZ last = p.at(HR_LAGRANGE_LAST), z_shift = p.at(HR_Z_PERM_SHIFT);
  const LZ public_input_term = LZ::add(hr_mulc(last, LZ::unpack(p.a.pidd)), z_shift);
  r0 = LZ::sub(hr_mul(LZ::add(p.at(HR_Z_PERM), p.at(HR_LAGRANGE_FIRST)), num), hr_mul(public_input_term, den)).fold_top();
  r1 = hr_mul(hr_mul(last, z_shift), sc);
}
// logderiv_lookup_relation.rs:86-91, :128-161, :185-204, :311-348. Read and write term in Horner form over beta: the same residues as the
// reference's sums of powers, and beta is the only power a lane holds.
template <class F, class LZ>
CSH_HD void hr_lookup_at(const HrPoint<F>& p, const LZ& sc, LZ& r0, LZ& r1, LZ& r2) {
  const LZ betad = LZ::unpack(p.a.betad), gamma = LZ::unpack(p.a.gamma);
  LZ read, write;
  {
    const LZ d3 = LZ::add(hr_mul(p.at(HR_Q_C), p.at(HR_W_O_SHIFT)), p.at(HR_W_O));
    const LZ h3 = LZ::add(d3, hr_mulc(p.at(HR_Q_O), betad)).fold_top();
    const LZ d2 = LZ::add(hr_mul(p.at(HR_Q_M), p.at(HR_W_R_SHIFT)), p.at(HR_W_R));
    const LZ h2 = LZ::add(d2, hr_mulc(h3, betad)).fold_top();
    const LZ d1 = LZ::add(LZ::add(p.at(HR_W_L), gamma), hr_mul(p.at(HR_Q_R), p.at(HR_W_L_SHIFT))).fold_top();
    read = LZ::add(d1, hr_mulc(h2, betad)).fold_top();
    const LZ t3 = LZ::add(p.at(HR_TABLE_3), hr_mulc(p.at(HR_TABLE_4), betad));
    const LZ t2 = LZ::add(p.at(HR_TABLE_2), hr_mulc(t3, betad));
    write = LZ::add(LZ::add(p.at(HR_TABLE_1), gamma), hr_mulc(t2, betad)).fold_top();
  }
  const LZ inverses = p.at(HR_LOOKUP_INVERSES), tag = p.at(HR_LOOKUP_READ_TAGS), q_lookup = p.at(HR_Q_LOOKUP);
  const LZ inverse_exists = LZ::sub(LZ::add(tag, q_lookup), hr_mul(tag, q_lookup)).fold_top();
  r0 = hr_mul(LZ::sub(hr_mul(hr_mul(read, write), inverses), inverse_exists), sc);
  const LZ read_inverse = hr_mul(write, inverses), write_inverse = hr_mul(read, inverses);
  r1 = LZ::sub(hr_mul(read_inverse, q_lookup), hr_mul(write_inverse, p.at(HR_LOOKUP_READ_COUNTS))).fold_top();  // no scaling factor
  r2 = hr_mul(LZ::sub(hr_mul(tag, tag), tag), sc);
}
// delta_range_constraint_relation.rs:179-236
template <class F, class LZ>
CSH_HD void hr_delta_at(const HrPoint<F>& p, const LZ& sc, LZ& r0, LZ& r1, LZ& r2, LZ& r3) {
  const LZ one = p.one(), two = LZ::unpack(p.a.two);
  const LZ qs = hr_mul(p.at(HR_Q_DELTA_RANGE), sc);
  auto term = [&](const LZ& hi, const LZ& lo) CSH_LAMBDA_INLINE {
    const LZ d = LZ::sub(hi, lo);
    const LZ a1 = LZ::sub(d, one).fold_top(), a2 = LZ::sub(d, two).fold_top();
    return hr_mul(hr_mul(LZ::sub(hr_mul(a1, a1), one), LZ::sub(hr_mul(a2, a2), one).fold_top()), qs);
  };
  const LZ w_1 = p.at(HR_W_L), w_2 = p.at(HR_W_R);
  r0 = term(w_2, w_1);
  const LZ w_3 = p.at(HR_W_O);
  r1 = term(w_3, w_2);
  const LZ w_4 = p.at(HR_W_4);
  r2 = term(w_4, w_3);
  r3 = term(p.at(HR_W_L_SHIFT), w_4);
}

// One edge at one point into the eleven running sums (each in F before and after): the body of the reference's loop, with its per-edge
// skips (Relation::skip: ultra_arithmetic_relation.rs:70-73, permutation_relation.rs:70-75, logderiv_lookup_relation.rs:213-216,
// delta_range_constraint_relation.rs:92-95) -- part of the result on data that does not satisfy the circuit. `rel` masks relations out
// (bit 0 arith, 1 perm, 2 lookup, 3 delta): the kernel is instantiated with all four.
template <int REL, class F, class LZ>
CSH_HD void hr_accumulate_edge(const HrArgs<F>& a, size_t j, int k, LZ (&acc)[HR_SUBRELATIONS]) {
  const HrPoint<F> p(a, j, k);
  const LZ sc = p.scaling();
  auto sum = [&](int s, const LZ& term) CSH_LAMBDA_INLINE { acc[s] = LZ::add(acc[s], term).fold_top(); };
  if ((REL & 1) && !p.zero_at_both_ends(HR_Q_ARITH)) {
    LZ r0, r1;
    hr_arith_at(p, sc, r0, r1);
    sum(HR_ARITH_0, r0), sum(HR_ARITH_1, r1);
  }
  if ((REL & 2) && !p.same_at_both_ends(HR_Z_PERM, HR_Z_PERM_SHIFT)) {
    LZ r0, r1;
    hr_perm_at(p, sc, r0, r1);
    sum(HR_PERM_0, r0), sum(HR_PERM_1, r1);
  }
  if ((REL & 4) && !(p.zero_at_both_ends(HR_Q_LOOKUP) && p.zero_at_both_ends(HR_LOOKUP_READ_COUNTS))) {
    LZ r0, r1, r2;
    hr_lookup_at(p, sc, r0, r1, r2);
    sum(HR_LOOKUP_0, r0), sum(HR_LOOKUP_1, r1), sum(HR_LOOKUP_2, r2);
  }
  if ((REL & 8) && !p.zero_at_both_ends(HR_Q_DELTA_RANGE)) {
    LZ r0, r1, r2, r3;
    hr_delta_at(p, sc, r0, r1, r2, r3);
    sum(HR_DELTA_0, r0), sum(HR_DELTA_1, r1), sum(HR_DELTA_2, r2), sum(HR_DELTA_3, r3);
  }
}

// The family, as honk_stage.hpp reads it
struct HrFam {
  template <class F>
  using Args = HrArgs<F>;
  static constexpr int COLS = HR_COLS, PARAMS = 3, ACC_ELEMS = 57, GROUPS = 1;  // params: beta, gamma, public_input_delta
  // one group: eleven running sums at six points (the longest accumulator), 42 edges per pass, no occupancy asked of the launch bound;
  // then the places and the lengths of the eleven accumulators in acc[57]
  static constexpr HsGroup group(int) {
    return HsGroup{HR_SUBRELATIONS, 6, 42, 0, {0, 6, 11, 17, 20, 25, 30, 33, 39, 45, 51}, {6, 5, 6, 3, 5, 5, 3, 6, 6, 6, 6}};
  }
  template <class F>
  static void consts(HrArgs<F>& a, const uint64_t* params) { hr_consts(a, params); }
  template <int G, class F, class LZ>
  CSH_HD static void accumulate_edge(const HrArgs<F>& a, size_t j, int k, LZ (&acc)[HR_SUBRELATIONS]) { hr_accumulate_edge<HR_ALL>(a, j, k, acc); }
};
static_assert(hs_family_ok<HrFam>(), "the accumulators tile acc[57], none is longer than its group's points, every (point, edge slot) has a lane");

// ---- the gate-separator table, decider/types.rs:53-67 -----------------------------------------------------------------------------------
template <class F>
struct HrPowArgs {
  F betad[HR_MAX_BETAS];  // beta_b R'
  F one;
  F* out;
  size_t count;  // 2^m
  uint32_t m;
};
template <class F>
CSH_HD F hr_pow_at(const HrPowArgs<F>& a, size_t i) {
  using LZ = typename LazyOf<F>::type;
  LZ v = LZ::unpack(a.one);
#pragma unroll 1
  for (uint32_t b = 0; b < a.m; ++b)
    if ((i >> b) & 1) v = hr_mulc(v, LZ::unpack(a.betad[b]));
  return v.canonical_wide().pack();
}

}  // namespace csh
