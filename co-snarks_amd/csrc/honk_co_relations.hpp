// The four relations of the collaborative UltraHonk sumcheck round on shares (honk_co_relations.hip): the
// stretches of local arithmetic between two network rounds of the relations of subrelations 0 .. 10, in
// co-noir/co-ultrahonk/src/co_decider/relations/: UltraArithmeticRelation (ultra_arithmetic_relation.rs:88-239), UltraPermutationRelation
// (permutation_relation.rs:70-150, :202-249), DeltaRangeConstraintRelation (delta_range_constraint_relation.rs:126-216) and
// LogDerivLookupRelation (logderiv_lookup_relation.rs:77-168, :255-312), and the `can_skip` rule of the edge selection. What is this
// family's own in the stage framework of honk_co_stage.hpp: the stage enum, the stages' descriptors, the constants, and every stage's loop
// body, which the kernels and the host self-test share. The columns are the 36 of honk_relations.hpp (HrCol): 0 .. 12 shares, 13 .. 35
// public.
//
// Arithmetic. Unlike the plain kernels (honk_relations.hpp) the stages work in the exact 32-bit-limb field F: every value is canonical
// between two operations, so there are no limb bounds to derive and none that could depend on the data, the range or the stride. The
// longest chain of a lane is a dozen products; the stages stream operand vectors and are bound by them. Outputs are canonical.
#pragma once
#include "honk_co_stage.hpp"

namespace csh {

enum HcStage : int {
  HC_SELECT = 0,
  HC_ARITH_R0, HC_ARITH_R1,
  HC_PERM_OPS, HC_PERM_OPS2, HC_PERM_FINISH,
  HC_DELTA_OPS, HC_DELTA_SUB_ONE, HC_DELTA_FINISH,
  HC_LOOKUP_OPS, HC_LOOKUP_MID_R0, HC_LOOKUP_MID_OPS, HC_LOOKUP_FINISH
};

// The stages as data; the accumulator lengths are the reference's (6, 5, 6, 3, 5, 5, 3, 6, 6, 6, 6). HC_SELECT and HC_DELTA_SUB_ONE read no
// column and are neither an operand nor a fold stage. arith_r0 is a half share: one component per element, both components read.
constexpr uint64_t hc_bit(int c) { return uint64_t(1) << c; }
constexpr CoStage hc_stage(int stage) {
  constexpr int S = HR_Q_M;  // the columns in front of q_m are shares
  constexpr uint64_t wires = hc_bit(HR_W_L) | hc_bit(HR_W_R) | hc_bit(HR_W_O) | hc_bit(HR_W_4);
  constexpr uint64_t tables = hc_bit(HR_TABLE_1) | hc_bit(HR_TABLE_2) | hc_bit(HR_TABLE_3) | hc_bit(HR_TABLE_4);
  switch (stage) {
    case HC_ARITH_R0:
      return co_fold(S, wires | hc_bit(HR_W_4_SHIFT) | hc_bit(HR_Q_M) | hc_bit(HR_Q_C) | hc_bit(HR_Q_L) | hc_bit(HR_Q_R) | hc_bit(HR_Q_O) |
                            hc_bit(HR_Q_4) | hc_bit(HR_Q_ARITH),
                     0, 0, false, 6, CoPass{1, {0}, {6}}, CoPass{}, true);
    case HC_ARITH_R1:
      return co_fold(S, hc_bit(HR_W_L) | hc_bit(HR_W_4) | hc_bit(HR_W_L_SHIFT) | hc_bit(HR_Q_M) | hc_bit(HR_Q_ARITH), 0, 0, false, 6,
                     CoPass{1, {0}, {5}});
    case HC_PERM_OPS:
      return co_ops(S, wires | hc_bit(HR_SIGMA_1) | hc_bit(HR_SIGMA_2) | hc_bit(HR_SIGMA_3) | hc_bit(HR_SIGMA_4) | hc_bit(HR_ID_1) |
                           hc_bit(HR_ID_2) | hc_bit(HR_ID_3) | hc_bit(HR_ID_4),
                    4, 4, 0, 0, true);
    case HC_PERM_OPS2:
      return co_ops(S, hc_bit(HR_Z_PERM) | hc_bit(HR_Z_PERM_SHIFT) | hc_bit(HR_LAGRANGE_FIRST) | hc_bit(HR_LAGRANGE_LAST), 2, 0, 0, 0, true);
    case HC_PERM_FINISH: return co_fold(S, hc_bit(HR_Z_PERM_SHIFT) | hc_bit(HR_LAGRANGE_LAST), 2, 0, false, 6, CoPass{2, {0, 6}, {6, 3}});
    case HC_DELTA_OPS: return co_ops(S, wires | hc_bit(HR_W_L_SHIFT), 8, 0, 0, 0, false);
    case HC_DELTA_FINISH: return co_fold(S, hc_bit(HR_Q_DELTA_RANGE), 4, 0, false, 6, CoPass{4, {0, 6, 12, 18}, {6, 6, 6, 6}});
    case HC_LOOKUP_OPS:
      return co_ops(S, hc_bit(HR_W_L) | hc_bit(HR_W_R) | hc_bit(HR_W_O) | hc_bit(HR_W_L_SHIFT) | hc_bit(HR_W_R_SHIFT) | hc_bit(HR_W_O_SHIFT) |
                           hc_bit(HR_Q_R) | hc_bit(HR_Q_M) | hc_bit(HR_Q_C) | hc_bit(HR_Q_O) | hc_bit(HR_LOOKUP_INVERSES),
                    1, 1, 0, 0, true);
    case HC_LOOKUP_MID_R0: return co_fold(S, tables | hc_bit(HR_LOOKUP_READ_TAGS) | hc_bit(HR_Q_LOOKUP), 1, 0, true, 6, CoPass{1, {0}, {5}});
    case HC_LOOKUP_MID_OPS: return co_ops(S, hc_bit(HR_LOOKUP_READ_TAGS) | hc_bit(HR_LOOKUP_READ_COUNTS), 0, 2, 2, 1, false);
    case HC_LOOKUP_FINISH:
      return co_fold(S, tables | hc_bit(HR_Q_LOOKUP) | hc_bit(HR_LOOKUP_INVERSES) | hc_bit(HR_LOOKUP_READ_TAGS), 2, 0, true, 6,
                     CoPass{2, {0, 5}, {5, 3}});
    default: return co_ops(S, 0, 0, 0, 0, 0, false);
  }
}

template <class F>
struct HcArgs : CoArgs<F, HR_COLS> {
  uint32_t protocol, party;
  F beta, gamma, pid, beta2, beta3, two, three, neg_half, neg_one, neg_two;  // arkworks-Montgomery
  const F* mask;             // HC_ARITH_R0, Rep3: 7 m elements
};
// -1/2, the one constant that costs a field inversion: made once per field, not once per call
template <class F>
inline const F& hc_neg_half() {
  static const F v = F::neg(F::inv(F::add(F::one(), F::one())));
  return v;
}
template <class F>
inline void hc_consts(HcArgs<F>& a, const CoCall& c) {
  a.protocol = c.protocol, a.party = c.party, a.mask = nullptr;
  a.two = F::add(a.one, a.one);
  a.three = F::add(a.two, a.one);
  a.neg_one = F::neg(a.one);
  a.neg_two = F::neg(a.two);
  a.neg_half = hc_neg_half<F>();
  a.beta = a.gamma = a.pid = a.beta2 = a.beta3 = F::zero();
  if (c.params) {
    a.beta = fr_load<F>(c.params), a.gamma = fr_load<F>(c.params + 4), a.pid = fr_load<F>(c.params + 8);
    a.beta2 = F::mul(a.beta, a.beta), a.beta3 = F::mul(a.beta2, a.beta);
  }
}

// can_skip of the arithmetic and the delta-range relation (ultra_arithmetic_relation.rs:247-249, delta_range_constraint_relation.rs:94-96):
// the extended selector is zero at all seven points exactly when it is zero at both ends
template <class F>
CSH_HD bool hc_keep(const F* q, size_t e) {
  return !(q[e].is_zero() && q[e + 1].is_zero());
}

// write_term, logderiv_lookup_relation.rs:142-168 (public)
template <class F>
CSH_HD F hc_write_term(const CoPoint<HcArgs<F>>& p) {
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
  const CoPoint<HcArgs<F>> p(a, t / HC_POINTS, (int)(t % HC_POINTS), (unsigned)(u & (size_t)(a.ncomp - 1)));
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
template <int STAGE, int PASS, class F>
CSH_HD void hc_terms_at(const HcArgs<F>& a, size_t j, int k, unsigned comp, F* term) {
  const CoPoint<HcArgs<F>> p(a, j, k, comp);
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

struct HcFamily {
  template <class F>
  using Args = HcArgs<F>;
  static constexpr int COLS = HR_COLS, STAGES = HC_LOOKUP_FINISH + 1;
  static constexpr CoStage stage(int s) { return hc_stage(s); }
  template <class F>
  static void consts(HcArgs<F>& a, const CoCall& c) { hc_consts(a, c); }
  template <int STAGE, class F>
  CSH_HD static void ops_at(const HcArgs<F>& a, size_t u) { hc_ops_at<STAGE>(a, u); }
  template <int STAGE, int PASS, class F>
  CSH_HD static void terms_at(const HcArgs<F>& a, size_t j, int k, unsigned comp, F* term) { hc_terms_at<STAGE, PASS>(a, j, k, comp, term); }
};

}  // namespace csh
