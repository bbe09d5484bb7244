// The sumcheck round of co-noir's collaborative UltraHonk prover on shares (honk_co_relations.hip): the stretches
// of local arithmetic between two network rounds of the four relations of subrelations 0 .. 10, in
// co-noir/co-ultrahonk/src/co_decider/relations/: UltraArithmeticRelation (ultra_arithmetic_relation.rs:88-239), UltraPermutationRelation
// (permutation_relation.rs:70-150, :202-249), DeltaRangeConstraintRelation (delta_range_constraint_relation.rs:126-216) and
// LogDerivLookupRelation (logderiv_lookup_relation.rs:77-168, :255-312), the `can_skip` selection of the edges, and the reduction that ends
// every relation, fold_accumulator! (relations/mod.rs:45-57). What the kernels and the host self-test share: the argument struct, the
// element rule, every stage's loop body.
//
// The batch is never built. The reference's batch element t of a column (extend_edges + fold_and_filter + add_entities,
// co_sumcheck/co_sumcheck_round.rs:54-73, types_batch.rs:105-130, relations/mod.rs:69-80) belongs to kept edge j = t / 7 and point
// k = t % 7 and is col[e] + k (col[e + 1] - col[e]) per component, e = 2 edge_idx[j] with an edge list and edge_begin + 2 j without; its
// scaling element is scaling[(e >> 1) stride]. Every stage computes its elements from the columns through this rule (HcPoint); the only
// vectors in memory are the operands and results of the network products, in the reference's concatenation order.
//
// Arithmetic. Unlike the plain kernels (honk_relations.hpp) the stages work in the exact 32-bit-limb field F: every value is canonical
// between two operations, so there are no limb bounds to derive and none that could depend on the data, the range or the stride. The
// longest chain of a lane is a dozen products; the stages stream operand vectors and are bound by them. Outputs are canonical.
//
// Shares. ncomp = 1 for protocol 0 (plain / Shamir), 2 for Rep3 ({a, b} interleaved); value (i, c) of a share vector is v[i ncomp + c].
// x (+) v adds the public v on the component pub_comp (a for protocol 0 and Rep3 party 0, b for Rep3 party 1, none for party 2).
#pragma once
#include "honk_relations.hpp"
#include "plonk_quot.hpp"

namespace csh {

constexpr int HC_POINTS = 7;        // MAX_PARTIAL_RELATION_LENGTH: points per kept edge in an operand vector
constexpr int HC_FOLD_POINTS = 6;   // the longest accumulator: fold_accumulator! drops the point 6
constexpr int HC_MAX_SUB = 4;       // subrelations a fold stage reduces at once

enum HcStage : int {
  HC_SELECT = 0,
  HC_ARITH_R0, HC_ARITH_R1,
  HC_PERM_OPS, HC_PERM_OPS2, HC_PERM_FINISH,
  HC_DELTA_OPS, HC_DELTA_SUB_ONE, HC_DELTA_FINISH,
  HC_LOOKUP_OPS, HC_LOOKUP_MID_R0, HC_LOOKUP_MID_OPS, HC_LOOKUP_FINISH
};

// the columns a stage reads, as a mask over HrCol
CSH_HD uint64_t hc_bit(int c) { return uint64_t(1) << c; }
inline uint64_t hc_cols_of(int stage) {
  const uint64_t wires = hc_bit(HR_W_L) | hc_bit(HR_W_R) | hc_bit(HR_W_O) | hc_bit(HR_W_4);
  const uint64_t tables = hc_bit(HR_TABLE_1) | hc_bit(HR_TABLE_2) | hc_bit(HR_TABLE_3) | hc_bit(HR_TABLE_4);
  switch (stage) {
    case HC_ARITH_R0:
      return wires | hc_bit(HR_W_4_SHIFT) | hc_bit(HR_Q_M) | hc_bit(HR_Q_C) | hc_bit(HR_Q_L) | hc_bit(HR_Q_R) | hc_bit(HR_Q_O) | hc_bit(HR_Q_4) |
             hc_bit(HR_Q_ARITH);
    case HC_ARITH_R1: return hc_bit(HR_W_L) | hc_bit(HR_W_4) | hc_bit(HR_W_L_SHIFT) | hc_bit(HR_Q_M) | hc_bit(HR_Q_ARITH);
    case HC_PERM_OPS:
      return wires | hc_bit(HR_SIGMA_1) | hc_bit(HR_SIGMA_2) | hc_bit(HR_SIGMA_3) | hc_bit(HR_SIGMA_4) | hc_bit(HR_ID_1) | hc_bit(HR_ID_2) |
             hc_bit(HR_ID_3) | hc_bit(HR_ID_4);
    case HC_PERM_OPS2: return hc_bit(HR_Z_PERM) | hc_bit(HR_Z_PERM_SHIFT) | hc_bit(HR_LAGRANGE_FIRST) | hc_bit(HR_LAGRANGE_LAST);
    case HC_PERM_FINISH: return hc_bit(HR_Z_PERM_SHIFT) | hc_bit(HR_LAGRANGE_LAST);
    case HC_DELTA_OPS: return wires | hc_bit(HR_W_L_SHIFT);
    case HC_DELTA_FINISH: return hc_bit(HR_Q_DELTA_RANGE);
    case HC_LOOKUP_OPS:
      return hc_bit(HR_W_L) | hc_bit(HR_W_R) | hc_bit(HR_W_O) | hc_bit(HR_W_L_SHIFT) | hc_bit(HR_W_R_SHIFT) | hc_bit(HR_W_O_SHIFT) | hc_bit(HR_Q_R) |
             hc_bit(HR_Q_M) | hc_bit(HR_Q_C) | hc_bit(HR_Q_O) | hc_bit(HR_LOOKUP_INVERSES);
    case HC_LOOKUP_MID_R0: return tables | hc_bit(HR_LOOKUP_READ_TAGS) | hc_bit(HR_Q_LOOKUP);
    case HC_LOOKUP_MID_OPS: return hc_bit(HR_LOOKUP_READ_TAGS) | hc_bit(HR_LOOKUP_READ_COUNTS);
    case HC_LOOKUP_FINISH: return tables | hc_bit(HR_Q_LOOKUP) | hc_bit(HR_LOOKUP_INVERSES) | hc_bit(HR_LOOKUP_READ_TAGS);
    default: return 0;
  }
}
// subrelations of a fold stage and their accumulator lengths (the reference's: 6, 5, 6, 3, 5, 5, 3, 6, 6, 6, 6)
struct HcFold {
  int ns;
  int len[HC_MAX_SUB];
};
inline HcFold hc_fold_of(int stage) {
  switch (stage) {
    case HC_ARITH_R0: return HcFold{1, {6, 0, 0, 0}};
    case HC_ARITH_R1: return HcFold{1, {5, 0, 0, 0}};
    case HC_PERM_FINISH: return HcFold{2, {6, 3, 0, 0}};
    case HC_DELTA_FINISH: return HcFold{4, {6, 6, 6, 6}};
    case HC_LOOKUP_MID_R0: return HcFold{1, {5, 0, 0, 0}};
    case HC_LOOKUP_FINISH: return HcFold{2, {5, 3, 0, 0}};
    default: return HcFold{0, {0, 0, 0, 0}};
  }
}
template <int STAGE>
struct HcNs {
  static constexpr int value = STAGE == HC_DELTA_FINISH ? 4 : ((STAGE == HC_PERM_FINISH || STAGE == HC_LOOKUP_FINISH) ? 2 : 1);
};

// What one call is told.
template <class F>
struct HcArgs {
  const F* col[HR_COLS];     // shares (0 .. 12, ncomp values per element) and public columns (13 .. 35)
  const uint32_t* edge_idx;  // the kept e >> 1, ascending; NULL = every edge of the range
  const F* scaling;          // NULL = one
  size_t scaling_stride;
  size_t edge_begin, m;      // m = kept edges
  uint32_t ncomp, protocol, party;
  int pub_comp;              // -1 = none
  F beta, gamma, pid, beta2, beta3, one, two, three, neg_half, neg_one, neg_two;  // arkworks-Montgomery
  const F* in;               // the result of the network product in front of the stage
  const F* mask;             // HC_ARITH_R0, Rep3: 7 m elements
  F* out[3];
  CSH_HD size_t n7() const { return HC_POINTS * m; }
};
// -1/2, the one constant that costs a field inversion: made once per field, not once per call
template <class F>
inline const F& hc_neg_half() {
  static const F v = F::neg(F::inv(F::add(F::one(), F::one())));
  return v;
}
template <class F>
inline void hc_consts(HcArgs<F>& a, const uint64_t* params) {
  a.one = F::one();
  a.two = F::add(a.one, a.one);
  a.three = F::add(a.two, a.one);
  a.neg_one = F::neg(a.one);
  a.neg_two = F::neg(a.two);
  a.neg_half = hc_neg_half<F>();
  a.beta = a.gamma = a.pid = a.beta2 = a.beta3 = F::zero();
  if (params) {
    a.beta = fr_load<F>(params), a.gamma = fr_load<F>(params + 4), a.pid = fr_load<F>(params + 8);
    a.beta2 = F::mul(a.beta, a.beta), a.beta3 = F::mul(a.beta2, a.beta);
  }
}

// v0 + k (v1 - v0), 0 <= k <= 6: Univariate::extend_from of a pair (univariate.rs:57-178), by the reference's running sum
template <class F>
CSH_HD F hc_lerp(const F& v0, const F& v1, int k) {
  const F d = F::sub(v1, v0);
  F r = v0;
#pragma unroll 1
  for (int i = 0; i < k; ++i) r = F::add(r, d);
  return r;
}

// Batch element t = 7 j + k of the columns, on the component `comp`.
template <class F>
struct HcPoint {
  const HcArgs<F>& a;
  size_t e;  // the edge's first element
  int k;
  unsigned comp;
  CSH_HD HcPoint(const HcArgs<F>& a_, size_t j, int k_, unsigned comp_)
      : a(a_), e(a_.edge_idx ? 2 * (size_t)a_.edge_idx[j] : a_.edge_begin + 2 * j), k(k_), comp(comp_) {}
  CSH_HD F pub(int c) const { return hc_lerp(a.col[c][e], a.col[c][e + 1], k); }
  CSH_HD F sh(int c, unsigned cc) const { return hc_lerp(a.col[c][e * a.ncomp + cc], a.col[c][(e + 1) * a.ncomp + cc], k); }
  CSH_HD F sh(int c) const { return sh(c, comp); }
  CSH_HD bool is_pub() const { return (int)comp == a.pub_comp; }
  CSH_HD F plus(const F& x, const F& v) const { return is_pub() ? F::add(x, v) : x; }  // x (+) v
  CSH_HD F sc() const { return a.scaling ? a.scaling[(e >> 1) * a.scaling_stride] : a.one; }
};

// can_skip of the arithmetic and the delta-range relation (ultra_arithmetic_relation.rs:247-249, delta_range_constraint_relation.rs:94-96):
// the extended selector is zero at all seven points exactly when it is zero at both ends
template <class F>
CSH_HD bool hc_keep(const F* q, size_t e) {
  return !(q[e].is_zero() && q[e + 1].is_zero());
}

// write_term, logderiv_lookup_relation.rs:142-168 (public)
template <class F>
CSH_HD F hc_write_term(const HcPoint<F>& p) {
  const HcArgs<F>& a = p.a;
  F w = F::add(p.pub(HR_TABLE_1), a.gamma);
  w = F::add(w, F::mul(p.pub(HR_TABLE_2), a.beta));
  w = F::add(w, F::mul(p.pub(HR_TABLE_3), a.beta2));
  return F::add(w, F::mul(p.pub(HR_TABLE_4), a.beta3));
}

// ---- operand stages: flat value index u over 7 m ncomp; operand q of an output starts at q 7 m ncomp ---------------------------------------
template <int STAGE, class F>
CSH_HD void hc_ops_at(const HcArgs<F>& a, size_t u) {
  const size_t t = a.ncomp == 1 ? u : u >> 1, seg = a.n7() * a.ncomp;
  const HcPoint<F> p(a, t / HC_POINTS, (int)(t % HC_POINTS), (unsigned)(u & (size_t)(a.ncomp - 1)));
  if constexpr (STAGE == HC_PERM_OPS) {
    // permutation_relation.rs:94-146: lhs = [wid1 | wsigma1 | wid3 | wsigma3], rhs = [wid2 | wsigma2 | wid4 | wsigma4]
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      F x = p.sh(HR_W_L + i), y = x;
      if (p.is_pub()) {
        x = F::add(x, F::add(F::mul(p.pub(HR_ID_1 + i), a.beta), a.gamma));
        y = F::add(y, F::add(F::mul(p.pub(HR_SIGMA_1 + i), a.beta), a.gamma));
      }
      F* o = a.out[i & 1];
      const size_t q = (i >> 1) * 2;
      o[q * seg + u] = x, o[(q + 1) * seg + u] = y;
    }
  } else if constexpr (STAGE == HC_PERM_OPS2) {
    // :227-234: rhs = [z_perm (+) lagrange_first | z_perm_shift (+) lagrange_last public_input_delta]
    F x = p.sh(HR_Z_PERM), y = p.sh(HR_Z_PERM_SHIFT);
    if (p.is_pub()) x = F::add(x, p.pub(HR_LAGRANGE_FIRST)), y = F::add(y, F::mul(p.pub(HR_LAGRANGE_LAST), a.pid));
    a.out[0][u] = x, a.out[0][seg + u] = y;
  } else if constexpr (STAGE == HC_DELTA_OPS) {
    // delta_range_constraint_relation.rs:146-177: lhs = [D_1 - 1 | .. | D_4 - 1 | D_1 - 2 | .. | D_4 - 2]
    F w[5];
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = p.sh(HR_W_L + i);
    w[4] = p.sh(HR_W_L_SHIFT);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const F d = F::sub(w[i + 1], w[i]);
      a.out[0][i * seg + u] = p.plus(d, a.neg_one), a.out[0][(4 + i) * seg + u] = p.plus(d, a.neg_two);
    }
  } else if constexpr (STAGE == HC_LOOKUP_OPS) {
    // logderiv_lookup_relation.rs:92-139 (read_term) and :263 (the extended inverses, the product's second operand)
    F d1 = F::add(F::mul(p.pub(HR_Q_R), p.sh(HR_W_L_SHIFT)), p.sh(HR_W_L));
    d1 = p.plus(d1, a.gamma);
    const F d2 = F::mul(F::add(F::mul(p.pub(HR_Q_M), p.sh(HR_W_R_SHIFT)), p.sh(HR_W_R)), a.beta);
    const F d3 = F::mul(F::add(F::mul(p.pub(HR_Q_C), p.sh(HR_W_O_SHIFT)), p.sh(HR_W_O)), a.beta2);
    d1 = F::add(F::add(d1, d2), d3);
    if (p.is_pub()) d1 = F::add(d1, F::mul(p.pub(HR_Q_O), a.beta3));
    a.out[0][u] = d1, a.out[1][u] = p.sh(HR_LOOKUP_INVERSES);
  } else {
    static_assert(STAGE == HC_LOOKUP_MID_OPS, "an operand stage");
    // :289-295: lhs = [write_inverse | read_tag], rhs = [read_counts | read_tag]
    const F tag = p.sh(HR_LOOKUP_READ_TAGS);
    a.out[1][u] = a.in[u], a.out[1][seg + u] = tag;
    a.out[2][u] = p.sh(HR_LOOKUP_READ_COUNTS), a.out[2][seg + u] = tag;
  }
}
// delta_range_constraint_relation.rs:181-183: add_assign_public(-1) on every element of the squares, in place; u over 8 * 7 m ncomp
template <class F>
CSH_HD void hc_sub_one_at(const HcArgs<F>& a, size_t u) {
  if ((int)(u & (size_t)(a.ncomp - 1)) == a.pub_comp) a.out[0][u] = F::add(a.out[0][u], a.neg_one);
}

// ---- fold stages: what batch element 7 j + k adds to the stage's accumulators on the component `comp` -------------------------------------
template <int STAGE, class F>
CSH_HD void hc_terms_at(const HcArgs<F>& a, size_t j, int k, unsigned comp, F* term) {
  const HcPoint<F> p(a, j, k, comp);
  const size_t t = HC_POINTS * j + k, seg = a.n7() * a.ncomp, u = t * a.ncomp + comp;
  if constexpr (STAGE == HC_ARITH_R0) {
    // ultra_arithmetic_relation.rs:88-189: a half share, one component per element
    const F la = p.sh(HR_W_L, 0), ra = p.sh(HR_W_R, 0);
    F mul;
    if (a.ncomp == 2) {  // rep3 local_mul_vec: a a' + a b' + b a' + mask
      const F lb = p.sh(HR_W_L, 1), rb = p.sh(HR_W_R, 1);
      mul = F::add(F::add(F::mul(la, F::add(ra, rb)), F::mul(lb, ra)), a.mask[t]);
    } else {
      mul = F::mul(la, ra);
    }
    const F qa = p.pub(HR_Q_ARITH);
    F tmp = F::mul(F::mul(F::mul(mul, p.pub(HR_Q_M)), F::sub(qa, a.three)), a.neg_half);
    tmp = F::add(tmp, F::mul(p.pub(HR_Q_L), la));
    tmp = F::add(tmp, F::mul(p.pub(HR_Q_R), ra));
    tmp = F::add(tmp, F::mul(p.pub(HR_Q_O), p.sh(HR_W_O, 0)));
    tmp = F::add(tmp, F::mul(p.pub(HR_Q_4), p.sh(HR_W_4, 0)));
    if (a.protocol == 0 || a.party == 0) tmp = F::add(tmp, p.pub(HR_Q_C));  // add_assign_public_half_share
    tmp = F::add(tmp, F::mul(F::sub(qa, a.one), p.sh(HR_W_4_SHIFT, 0)));
    term[0] = F::mul(F::mul(tmp, qa), p.sc());
  } else if constexpr (STAGE == HC_ARITH_R1) {
    // :190-239
    const F qa = p.pub(HR_Q_ARITH);
    F tmp = F::sub(F::add(p.sh(HR_W_L), p.sh(HR_W_4)), p.sh(HR_W_L_SHIFT));
    if (p.is_pub()) tmp = F::add(tmp, p.pub(HR_Q_M));
    tmp = F::mul(F::mul(F::mul(tmp, F::sub(qa, a.two)), F::sub(qa, a.one)), qa);
    term[0] = F::mul(tmp, p.sc());
  } else if constexpr (STAGE == HC_PERM_FINISH) {
    // permutation_relation.rs:236-246
    const F sc = p.sc();
    term[0] = F::mul(F::sub(a.in[u], a.in[seg + u]), sc);
    term[1] = F::mul(F::mul(p.pub(HR_LAGRANGE_LAST), p.sh(HR_Z_PERM_SHIFT)), sc);
  } else if constexpr (STAGE == HC_DELTA_FINISH) {
    // delta_range_constraint_relation.rs:187-214
    const F qs = F::mul(p.pub(HR_Q_DELTA_RANGE), p.sc());
#pragma unroll
    for (int i = 0; i < 4; ++i) term[i] = F::mul(a.in[i * seg + u], qs);
  } else if constexpr (STAGE == HC_LOOKUP_MID_R0) {
    // logderiv_lookup_relation.rs:77-90, :277-281
    const F tag = p.sh(HR_LOOKUP_READ_TAGS), ql = p.pub(HR_Q_LOOKUP);
    const F inverse_exists = p.plus(F::sub(tag, F::mul(ql, tag)), ql);
    term[0] = F::mul(F::sub(F::mul(hc_write_term(p), a.in[u]), inverse_exists), p.sc());
  } else {
    static_assert(STAGE == HC_LOOKUP_FINISH, "a fold stage");
    // :272, :296-309: r1 has no scaling factor
    const F read_inverse = F::mul(hc_write_term(p), p.sh(HR_LOOKUP_INVERSES));
    term[0] = F::sub(F::mul(p.pub(HR_Q_LOOKUP), read_inverse), a.in[u]);
    term[1] = F::mul(F::sub(a.in[seg + u], p.sh(HR_LOOKUP_READ_TAGS)), p.sc());
  }
}

}  // namespace csh
