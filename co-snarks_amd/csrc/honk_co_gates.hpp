// The other five relations of the collaborative UltraHonk sumcheck round on shares (honk_co_gates.hip): the
// stretches of local arithmetic between two network products of co-noir/co-ultrahonk/src/co_decider/relations/ for EllipticRelation
// (elliptic_relation.rs:102-254), MemoryRelation (memory_relation.rs:166-457), NonNativeFieldRelation
// (non_native_field_relation.rs:109-215), Poseidon2ExternalRelation (poseidon2_external_relation.rs:141-228) and
// Poseidon2InternalRelation (poseidon2_internal_relation.rs:135-227), subrelations 11 .. 27. What is this family's own in the stage
// framework of honk_co_stage.hpp: the stage enum, the stages' descriptors, the constants, and every stage's loop body, which the kernels
// and the host self-test share.
//
// The columns are the 19 of honk_gates.hpp (HgCol): 0 .. 7 shares, 8 .. 18 public. The parameters are the eight of the plain entry
// (eta_1..3, curve_b, mat_internal_diag_m_1[0..4)); 2^68 and 2^14 are made on the host per field. Every value is a canonical element of
// the exact 32-bit-limb field F between two operations.
#pragma once
#include "honk_co_stage.hpp"
#include "honk_gates.hpp"

namespace csh {

enum HgcStage : int {
  HGC_ELL_OPS = 0, HGC_ELL_OPS2, HGC_ELL_FINISH,
  HGC_MEM_OPS, HGC_MEM_FINISH,
  HGC_NNF_OPS, HGC_NNF_FINISH,
  HGC_POS_EXT_OPS, HGC_POS_EXT_FINISH,
  HGC_POS_INT_OPS, HGC_POS_INT_FINISH,
  HGC_STAGES
};

// The stages as data. Subrelation s of a fold stage is accumulator s of its output, entry k at element s POINTS + k: the Poseidon2
// accumulators keep seven points, the others six. mem_finish folds its six subrelations in two launches of three -- r1, r2, r4, which
// need neither the records nor the second product, and r0, r3, r5 -- so that a lane holds three running sums, not six.
constexpr CoStage hgc_stage(int stage) {
  constexpr int S = HG_Q_M;  // the columns in front of q_m are shares
  constexpr auto bit = [](int c) { return uint64_t(1) << c; };
  constexpr uint64_t wires = bit(HG_W_L) | bit(HG_W_R) | bit(HG_W_O) | bit(HG_W_4);
  constexpr uint64_t shifts = bit(HG_W_L_SHIFT) | bit(HG_W_R_SHIFT) | bit(HG_W_O_SHIFT) | bit(HG_W_4_SHIFT);
  constexpr CoPass four_of_seven{4, {0, 7, 14, 21}, {7, 7, 7, 7}};
  switch (stage) {
    case HGC_ELL_OPS: return co_ops(S, bit(HG_W_R) | bit(HG_W_O) | shifts | bit(HG_Q_L), 7, 7, 0, 0, false);
    case HGC_ELL_OPS2: return co_ops(S, bit(HG_W_R) | bit(HG_W_O) | bit(HG_W_L_SHIFT) | bit(HG_W_R_SHIFT) | bit(HG_W_O_SHIFT), 5, 5, 0, 7, true);
    case HGC_ELL_FINISH: return co_fold(S, bit(HG_Q_L) | bit(HG_Q_M) | bit(HG_Q_ELLIPTIC), 7, 5, false, 6, CoPass{2, {0, 6}, {6, 6}});
    case HGC_MEM_OPS: return co_ops(S, wires | shifts | bit(HG_Q_C), 6, 6, 1, 0, true);
    case HGC_MEM_FINISH:
      return co_fold(S, wires | shifts | bit(HG_Q_M) | bit(HG_Q_C) | bit(HG_Q_L) | bit(HG_Q_R) | bit(HG_Q_O) | bit(HG_Q_4) | bit(HG_Q_MEMORY), 6, 1,
                     true, 6, CoPass{3, {6, 12, 24}, {6, 6, 6}}, CoPass{3, {0, 18, 30}, {6, 6, 6}});
    case HGC_NNF_OPS: return co_ops(S, wires | bit(HG_W_L_SHIFT) | bit(HG_W_R_SHIFT), 5, 5, 0, 0, false);
    case HGC_NNF_FINISH:
      return co_fold(S, wires | shifts | bit(HG_Q_M) | bit(HG_Q_R) | bit(HG_Q_O) | bit(HG_Q_4) | bit(HG_Q_NNF), 5, 0, false, 6, CoPass{1, {0}, {6}});
    case HGC_POS_EXT_OPS: return co_ops(S, wires | bit(HG_Q_L) | bit(HG_Q_R) | bit(HG_Q_O) | bit(HG_Q_4), 4, 0, 0, 0, false);
    case HGC_POS_EXT_FINISH: return co_fold(S, shifts | bit(HG_Q_POSEIDON2_EXTERNAL), 4, 0, false, 7, four_of_seven);
    case HGC_POS_INT_OPS: return co_ops(S, bit(HG_W_L) | bit(HG_Q_L), 1, 0, 0, 0, false);
    case HGC_POS_INT_FINISH:
      return co_fold(S, bit(HG_W_R) | bit(HG_W_O) | bit(HG_W_4) | shifts | bit(HG_Q_POSEIDON2_INTERNAL), 1, 0, true, 7, four_of_seven);
    default: return co_ops(S, 0, 0, 0, 0, 0, false);
  }
}

template <class F>
struct HgcArgs : CoArgs<F, HG_COLS> {
  F eta[3], neg_curve_b, diag[4], limb, sublimb;  // arkworks-Montgomery
};
template <class F>
inline void hgc_consts(HgcArgs<F>& a, const CoCall& c) {
  const uint64_t* params = c.params;
  F pw = F::add(a.one, a.one);  // 2^14 and 2^68 by square and multiply on 2
  a.sublimb = a.limb = a.one;
  for (int bit = 0; bit < 7; ++bit, pw = F::mul(pw, pw)) {
    if ((14 >> bit) & 1) a.sublimb = F::mul(a.sublimb, pw);
    if ((68 >> bit) & 1) a.limb = F::mul(a.limb, pw);
  }
  for (int i = 0; i < 3; ++i) a.eta[i] = params ? fr_load<F>(params + 4 * i) : F::zero();
  a.neg_curve_b = params ? F::neg(fr_load<F>(params + 12)) : F::zero();
  for (int i = 0; i < 4; ++i) a.diag[i] = params ? fr_load<F>(params + 16 + 4 * i) : F::zero();
}

// w_3 eta_three + w_2 eta_two + w_1 eta of the four columns from `first` on (memory_relation.rs:241-243, :328-336)
template <class F>
CSH_HD F hgc_record(const CoPoint<HgcArgs<F>>& p, int first) {
  const HgcArgs<F>& a = p.a;
  F r = F::mul(p.sh(first + 2), a.eta[2]);
  r = F::add(r, F::mul(p.sh(first + 1), a.eta[1]));
  return F::add(r, F::mul(p.sh(first), a.eta[0]));
}
// (((x0 2^14 + x1) 2^14 + x2) 2^14 + x3) 2^14 of four columns (non_native_field_relation.rs:183-189, :195-201)
template <class F>
CSH_HD F hgc_limbs(const CoPoint<HgcArgs<F>>& p, int c0, int c1, int c2, int c3) {
  const F& s = p.a.sublimb;
  F r = F::mul(p.sh(c0), s);
  r = F::mul(F::add(r, p.sh(c1)), s);
  r = F::mul(F::add(r, p.sh(c2)), s);
  return F::mul(F::add(r, p.sh(c3)), s);
}

// ---- operand stages: flat value index u over 7 m ncomp; part q of an output starts at q 7 m ncomp -------------------------------------------
template <int STAGE, class F>
CSH_HD void hgc_ops_at(const HgcArgs<F>& a, size_t u) {
  const size_t t = a.ncomp == 1 ? u : u >> 1, seg = a.n7() * a.ncomp;
  const CoPoint<HgcArgs<F>> p(a, t / HC_POINTS, (int)(t % HC_POINTS), (unsigned)(u & (size_t)(a.ncomp - 1)));
  F* lhs = a.out[0];
  F* rhs = a.out[1];
  if constexpr (STAGE == HGC_ELL_OPS) {
    // elliptic_relation.rs:116-167: x_1 = w_r, y_1 = w_o, x_2 = w_l', y_2 = w_4', x_3 = w_r', y_3 = w_o', q_sign = q_l
    const F x_1 = p.sh(HG_W_R), y_1 = p.sh(HG_W_O), x_2 = p.sh(HG_W_L_SHIFT), y_2 = p.sh(HG_W_4_SHIFT);
    const F x_diff = F::sub(x_2, x_1);
    lhs[u] = y_1, lhs[seg + u] = y_2, lhs[2 * seg + u] = y_1, lhs[3 * seg + u] = x_diff;
    lhs[4 * seg + u] = F::add(y_1, p.sh(HG_W_O_SHIFT));
    lhs[5 * seg + u] = F::sub(F::mul(p.pub(HG_Q_L), y_2), y_1);
    lhs[6 * seg + u] = F::add(F::add(x_1, x_1), x_1);
    rhs[u] = y_1, rhs[seg + u] = y_2, rhs[2 * seg + u] = y_2, rhs[3 * seg + u] = x_diff, rhs[4 * seg + u] = x_diff;
    rhs[5 * seg + u] = F::sub(p.sh(HG_W_R_SHIFT), x_1);
    rhs[6 * seg + u] = x_1;
  } else if constexpr (STAGE == HGC_ELL_OPS2) {
    // :173-193: in = mul1 = [y1^2 | y2^2 | y1 y2 | x_diff^2 | (y1 + y3) x_diff | y_diff (x3 - x1) | 3 x1^2]
    const F x_1 = p.sh(HG_W_R), y_1 = p.sh(HG_W_O), x_3 = p.sh(HG_W_R_SHIFT);
    const F y1_sqr = a.in[u], y1_sqr_mul_2 = F::add(y1_sqr, y1_sqr);
    lhs[u] = F::add(F::add(x_3, p.sh(HG_W_L_SHIFT)), x_1);
    lhs[seg + u] = p.plus(y1_sqr, a.neg_curve_b);
    lhs[2 * seg + u] = F::add(F::add(x_3, x_1), x_1);
    lhs[3 * seg + u] = a.in[6 * seg + u];
    lhs[4 * seg + u] = F::add(y_1, y_1);
    rhs[u] = a.in[3 * seg + u];
    rhs[seg + u] = F::add(F::add(x_1, x_1), x_1);
    rhs[2 * seg + u] = F::add(y1_sqr_mul_2, y1_sqr_mul_2);
    rhs[3 * seg + u] = F::sub(x_1, x_3);
    rhs[4 * seg + u] = F::add(y_1, p.sh(HG_W_O_SHIFT));
  } else if constexpr (STAGE == HGC_MEM_OPS) {
    // memory_relation.rs:241-357: lhs = [neg_index_delta | index_delta_is_zero | neg_access_type | index_delta_is_zero |
    // neg_next_gate_access_type | index_delta_is_zero], rhs = [neg_index_delta | record_delta | neg_access_type | value_delta |
    // neg_next_gate_access_type | timestamp_delta]; out[2] = neg_next_gate_access_type (+) 1 (:398)
    const F w_4 = p.sh(HG_W_4), w_4_shift = p.sh(HG_W_4_SHIFT);
    const F neg_access_type = F::sub(p.plus(hgc_record(p, HG_W_L), p.pub(HG_Q_C)), w_4);
    const F neg_index_delta = F::sub(p.sh(HG_W_L), p.sh(HG_W_L_SHIFT)), index_delta_is_zero = p.plus(neg_index_delta, a.one);
    const F neg_next = F::sub(hgc_record(p, HG_W_L_SHIFT), w_4_shift);
    lhs[u] = neg_index_delta, rhs[u] = neg_index_delta;
    lhs[seg + u] = index_delta_is_zero, rhs[seg + u] = F::sub(w_4_shift, w_4);
    lhs[2 * seg + u] = neg_access_type, rhs[2 * seg + u] = neg_access_type;
    lhs[3 * seg + u] = index_delta_is_zero, rhs[3 * seg + u] = F::sub(p.sh(HG_W_O_SHIFT), p.sh(HG_W_O));
    lhs[4 * seg + u] = neg_next, rhs[4 * seg + u] = neg_next;
    lhs[5 * seg + u] = index_delta_is_zero, rhs[5 * seg + u] = F::sub(p.sh(HG_W_R_SHIFT), p.sh(HG_W_R));
    a.out[2][u] = p.plus(neg_next, a.one);
  } else if constexpr (STAGE == HGC_NNF_OPS) {
    // non_native_field_relation.rs:138-148: lhs = [w1 | w2 | w4 | w3 | w1'], rhs = [w2' | w1' | w1 | w2 | w2']
    const F w_1 = p.sh(HG_W_L), w_2 = p.sh(HG_W_R), w_1_shift = p.sh(HG_W_L_SHIFT), w_2_shift = p.sh(HG_W_R_SHIFT);
    lhs[u] = w_1, lhs[seg + u] = w_2, lhs[2 * seg + u] = p.sh(HG_W_4), lhs[3 * seg + u] = p.sh(HG_W_O), lhs[4 * seg + u] = w_1_shift;
    rhs[u] = w_2_shift, rhs[seg + u] = w_1_shift, rhs[2 * seg + u] = w_1, rhs[3 * seg + u] = w_2, rhs[4 * seg + u] = w_2_shift;
  } else if constexpr (STAGE == HGC_POS_EXT_OPS) {
    // poseidon2_external_relation.rs:165-174: s = [w_l (+) q_l | w_r (+) q_r | w_o (+) q_o | w_4 (+) q_4]
    const int q[4] = {HG_Q_L, HG_Q_R, HG_Q_O, HG_Q_4};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      F s = p.sh(HG_W_L + i);
      if (p.is_pub()) s = F::add(s, p.pub(q[i]));
      lhs[i * seg + u] = s;
    }
  } else {
    static_assert(STAGE == HGC_POS_INT_OPS, "an operand stage");
    // poseidon2_internal_relation.rs:155: s1 = w_l (+) q_l
    F s = p.sh(HG_W_L);
    if (p.is_pub()) s = F::add(s, p.pub(HG_Q_L));
    lhs[u] = s;
  }
}

// ---- fold stages: what batch element 7 j + k adds to the stage's accumulators on the component `comp` -------------------------------------
template <int STAGE, int PASS, class F>
CSH_HD void hgc_terms_at(const HgcArgs<F>& a, size_t j, int k, unsigned comp, F* term) {
  const CoPoint<HgcArgs<F>> p(a, j, k, comp);
  const size_t t = HC_POINTS * j + k, seg = a.n7() * a.ncomp, u = t * a.ncomp + comp;
  if constexpr (STAGE == HGC_ELL_FINISH) {
    // elliptic_relation.rs:199-252; in2 = mul2 = [(x3 + x2 + x1) x_diff^2 | (y1^2 - b) 3 x1 | (x3 + 2 x1) 4 y1^2 | 3 x1^2 (x1 - x3) |
    // 2 y1 (y1 + y3)]
    const F q_elliptic_by_scaling = F::mul(p.pub(HG_Q_ELLIPTIC), p.sc());
    const F q_double = F::mul(q_elliptic_by_scaling, p.pub(HG_Q_M)), q_not_double = F::sub(q_elliptic_by_scaling, q_double);
    const F y1y2 = F::mul(p.pub(HG_Q_L), a.in[2 * seg + u]);
    F x_add = F::sub(F::sub(a.in2[u], a.in[seg + u]), a.in[u]);
    x_add = F::add(F::add(x_add, y1y2), y1y2);
    const F x_pow_4_mul_3 = a.in2[seg + u];
    const F x_double = F::sub(a.in2[2 * seg + u], F::add(F::add(x_pow_4_mul_3, x_pow_4_mul_3), x_pow_4_mul_3));
    term[0] = F::add(F::mul(q_not_double, x_add), F::mul(q_double, x_double));
    const F y_add = F::add(a.in[4 * seg + u], a.in[5 * seg + u]), y_double = F::sub(a.in2[3 * seg + u], a.in2[4 * seg + u]);
    term[1] = F::add(F::mul(q_not_double, y_add), F::mul(q_double, y_double));
  } else if constexpr (STAGE == HGC_MEM_FINISH) {
    // memory_relation.rs:370-455; in = mul = [neg_index_delta^2 | index_delta_is_zero record_delta | neg_access_type^2 |
    // index_delta_is_zero value_delta | neg_next_gate_access_type^2 | index_delta_is_zero timestamp_delta], in2 = mul[3] (next (+) 1)
    const F q_memory_by_scaling = F::mul(p.sc(), p.pub(HG_Q_MEMORY)), q_1 = p.pub(HG_Q_L);
    const F q_3ms = F::mul(p.pub(HG_Q_O), q_memory_by_scaling);
    if constexpr (PASS == 0) {  // r1, r2, r4
      const F q_12ms = F::mul(F::mul(q_1, p.pub(HG_Q_R)), q_memory_by_scaling);
      const F monotone = F::add(a.in[u], F::sub(p.sh(HG_W_L), p.sh(HG_W_L_SHIFT)));
      term[0] = F::mul(q_12ms, a.in[seg + u]);
      term[1] = F::mul(q_12ms, monotone);
      term[2] = F::mul(q_3ms, monotone);
    } else {  // r0, r3, r5
      // the record check: the ROM identity and, through q_m q_1, the plain record gate
      const F record = F::sub(p.plus(hgc_record(p, HG_W_L), p.pub(HG_Q_C)), p.sh(HG_W_4));
      F identity = F::mul(F::mul(q_1, p.pub(HG_Q_R)), record);
      identity = F::add(identity, F::mul(F::mul(p.pub(HG_Q_4), q_1), F::sub(a.in[5 * seg + u], p.sh(HG_W_O))));
      identity = F::add(identity, F::mul(F::mul(p.pub(HG_Q_M), q_1), record));
      // :452-453: the RAM consistency term carries q_memory scaling already and is added after the product
      term[0] = F::add(F::mul(identity, q_memory_by_scaling), F::mul(q_3ms, F::add(a.in[2 * seg + u], record)));
      term[1] = F::mul(q_3ms, a.in2[u]);
      const F neg_next = F::sub(hgc_record(p, HG_W_L_SHIFT), p.sh(HG_W_4_SHIFT));
      term[2] = F::mul(q_3ms, F::add(a.in[4 * seg + u], neg_next));
    }
  } else if constexpr (STAGE == HGC_NNF_FINISH) {
    // non_native_field_relation.rs:154-213; in = mul = [w1 w2' | w2 w1' | w4 w1 | w3 w2 | w1' w2']
    const F w_3 = p.sh(HG_W_O), w_4 = p.sh(HG_W_4), w_3_shift = p.sh(HG_W_O_SHIFT), w_4_shift = p.sh(HG_W_4_SHIFT);
    const F q_3 = p.pub(HG_Q_O), q_4 = p.pub(HG_Q_4), q_m = p.pub(HG_Q_M);
    F limb_subproduct = F::add(a.in[u], a.in[seg + u]);
    F gate_2 = F::mul(F::sub(F::add(a.in[2 * seg + u], a.in[3 * seg + u]), w_3_shift), a.limb);
    gate_2 = F::mul(F::add(F::sub(gate_2, w_4_shift), limb_subproduct), q_4);
    limb_subproduct = F::add(F::mul(limb_subproduct, a.limb), a.in[4 * seg + u]);
    const F gate_1 = F::mul(F::sub(F::sub(limb_subproduct, w_3), w_4), q_3);
    const F gate_3 = F::mul(F::sub(F::sub(F::add(limb_subproduct, w_4), w_3_shift), w_4_shift), q_m);
    const F identity = F::mul(F::add(F::add(gate_1, gate_2), gate_3), p.pub(HG_Q_R));
    F acc_1 = hgc_limbs(p, HG_W_R_SHIFT, HG_W_L_SHIFT, HG_W_O, HG_W_R);
    acc_1 = F::mul(F::sub(F::add(acc_1, p.sh(HG_W_L)), w_4), q_4);
    F acc_2 = hgc_limbs(p, HG_W_O_SHIFT, HG_W_R_SHIFT, HG_W_L_SHIFT, HG_W_4);
    acc_2 = F::mul(F::sub(F::add(acc_2, w_3), w_4_shift), q_m);
    const F limb_accumulators = F::mul(F::add(acc_1, acc_2), q_3);
    term[0] = F::mul(F::mul(F::add(identity, limb_accumulators), p.pub(HG_Q_NNF)), p.sc());
  } else if constexpr (STAGE == HGC_POS_EXT_FINISH) {
    // poseidon2_external_relation.rs:181-226; in = u = [s1^5 | s2^5 | s3^5 | s4^5]: v = M_E u by the reference's fourteen additions
    const F u_1 = a.in[u], u_2 = a.in[seg + u], u_3 = a.in[2 * seg + u], u_4 = a.in[3 * seg + u];
    const F t_0 = F::add(u_1, u_2), t_1 = F::add(u_3, u_4);
    const F t_2 = F::add(F::add(u_2, u_2), t_1), t_3 = F::add(F::add(u_4, u_4), t_0);
    F v_4 = F::add(t_1, t_1);
    v_4 = F::add(F::add(v_4, v_4), t_3);
    F v_2 = F::add(t_0, t_0);
    v_2 = F::add(F::add(v_2, v_2), t_2);
    const F v_1 = F::add(t_3, v_2), v_3 = F::add(t_2, v_4);
    const F qs = F::mul(p.pub(HG_Q_POSEIDON2_EXTERNAL), p.sc());
    term[0] = F::mul(F::sub(v_1, p.sh(HG_W_L_SHIFT)), qs);
    term[1] = F::mul(F::sub(v_2, p.sh(HG_W_R_SHIFT)), qs);
    term[2] = F::mul(F::sub(v_3, p.sh(HG_W_O_SHIFT)), qs);
    term[3] = F::mul(F::sub(v_4, p.sh(HG_W_4_SHIFT)), qs);
  } else {
    static_assert(STAGE == HGC_POS_INT_FINISH, "a fold stage");
    // poseidon2_internal_relation.rs:163-223; in = u1 = s1^5: v = M_I u, the diagonal values from the host
    const F u_1 = a.in[u], u_2 = p.sh(HG_W_R), u_3 = p.sh(HG_W_O), u_4 = p.sh(HG_W_4);
    const F sum = F::add(F::add(F::add(u_1, u_2), u_3), u_4);
    const F qs = F::mul(p.pub(HG_Q_POSEIDON2_INTERNAL), p.sc());
    term[0] = F::mul(F::sub(F::add(F::mul(u_1, a.diag[0]), sum), p.sh(HG_W_L_SHIFT)), qs);
    term[1] = F::mul(F::sub(F::add(F::mul(u_2, a.diag[1]), sum), p.sh(HG_W_R_SHIFT)), qs);
    term[2] = F::mul(F::sub(F::add(F::mul(u_3, a.diag[2]), sum), p.sh(HG_W_O_SHIFT)), qs);
    term[3] = F::mul(F::sub(F::add(F::mul(u_4, a.diag[3]), sum), p.sh(HG_W_4_SHIFT)), qs);
  }
}

struct HgcFamily {
  template <class F>
  using Args = HgcArgs<F>;
  static constexpr int COLS = HG_COLS, STAGES = HGC_STAGES;
  static constexpr CoStage stage(int s) { return hgc_stage(s); }
  template <class F>
  static void consts(HgcArgs<F>& a, const CoCall& c) { hgc_consts(a, c); }
  template <int STAGE, class F>
  CSH_HD static void ops_at(const HgcArgs<F>& a, size_t u) { hgc_ops_at<STAGE>(a, u); }
  template <int STAGE, int PASS, class F>
  CSH_HD static void terms_at(const HgcArgs<F>& a, size_t j, int k, unsigned comp, F* term) { hgc_terms_at<STAGE, PASS>(a, j, k, comp, term); }
};

}  // namespace csh
