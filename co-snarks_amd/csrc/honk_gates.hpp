// The other five relations of co-noir's UltraHonk sumcheck round (honk_gates.hip): the loop body of
// SumcheckProverRound::compute_univariate_inner, co-noir/ultrahonk/src/decider/sumcheck/sumcheck_round_prover.rs:224-255, for
// EllipticRelation (relations/elliptic_relation.rs:81-161), MemoryRelation (memory_relation.rs:145-358), NonNativeFieldRelation
// (non_native_field_relation.rs:85-177), Poseidon2ExternalRelation (poseidon2_external_relation.rs:121-205) and Poseidon2InternalRelation
// (poseidon2_internal_relation.rs:118-200): subrelations 11 .. 27 of the batching order (relations/mod.rs:134-145). What the kernels and
// the host self-test (selftest.hip, limb-bound checks on) share: the column order, the argument struct and how the host fills it in, the
// five relations at one point in the scalar shape of each file's verify_accumulate, the per-edge skips and the bounds. The extension of
// an edge to a point, the two products and the scale conventions are honk_relations.hpp's (hr_extend, hr_mul, hr_mulc).
//
// Column order of cols[19] (part of the ABI, include/cosnarks_hip.h):
//    0.. 3  witness          w_l, w_r, w_o, w_4
//    4.. 7  shifted witness  w_l, w_r, w_o, w_4
//    8..13  precomputed      q_m, q_c, q_l, q_r, q_o, q_4
//   14..18  gate selectors   q_elliptic, q_memory, q_nnf, q_poseidon2_external, q_poseidon2_internal
// Accumulator order of acc[110]: elliptic.r0, r1 (6 each), memory.r0 .. r5 (6 each), nnf.r0 (6), poseidon2_external.r0 .. r3 (7 each),
// poseidon2_internal.r0 .. r3 (7 each); entry i of an accumulator is its evaluation at the point i.
//
// Groups. Seventeen running sums and the S-boxes do not fit under 256 VGPRs, so the relations are dealt to three launches of one kernel
// template (hg_group): EN = elliptic + nnf (3 sums, 6 points, 42 edges per pass), MEM = memory (6 sums, 6 points, 42 edges per pass), POS =
// Poseidon2 external + internal (8 sums, 7 points, 36 edges per pass). A lane takes ONE point of one edge, as in honk_relations.hpp.
//
// Skips. Each relation is left out of an edge when its own selector is zero at both ends (Relation::skip of the five files: the selector's
// univariate is zero, which for the extension of a pair means both ends are). Checked here: every one of the five selectors multiplies its
// WHOLE relation -- elliptic r0, r1 = (..) q_elliptic sc (1 - q_m) + (..) q_elliptic sc q_m; memory r1 .. r5 = (..) q_memory sc and
// r0 = (rom + timestamp + record) q_memory sc + access_check q_o q_memory sc (memory_relation.rs:347-353: the RAM term is added AFTER
// the multiplication, and carries the factor already); nnf r0 = (..) q_nnf sc; Poseidon2 r0 .. r3 = (v_i - w_i_shift) q sc. So a skip
// can only omit zeros, on any data; what a test can catch is a skip that fires when it should not (zero at one end only). The skip test
// reads two selector words ahead of every other load of the edge.
//
// Bounds, over the classes U, F, M of honk_relations.hpp (p / R' < 1 / 64; F = fold_top() output, value in (-p - eps, 2 p + eps)):
//   extension  hr_extend(v0, v1, k) with k <= 6 (the Poseidon2 accumulators have seven points): (1 - k) v0 + k v1 in (-5 p, 6 p), the
//     64-bit carry chain holds 6 2^29 < 2^32 per limb, and fold_top() is exact for a quotient up to 64: F, as for k <= 5.
//   sums  at most three terms of F (U, M) are added or subtracted limb-wise between two fold_top(), and each such sum is folded before it
//     is used as the SECOND operand of a product; |limb| < 3 2^29 < 2^31, |value| < 6.1 p. A sum of at most two terms may be the FIRST
//     operand of hr_mul / hr_mulc unfolded (|x| < 4.03 p: honk_relations.hpp's bound for times32() and mul()). Nothing wider is used:
//     3 x_1, 4 y_1^2, 9 x_1^4 and the external matrix's coefficients up to 7 (5 u_1 + 7 u_2 + u_3 + 3 u_4 ...) are built by the
//     reference's own chain of additions and doublings with a fold after each step of at most three terms, so every intermediate is F.
//   constants  2^68, 2^14, eta_1..3 and the four diagonal values are operands of hr_mulc in the R' domain (fr_to_rprime on the host, once
//     per call; U): x c with x at most two terms of F gives M. curve_b and 1 are only added: plain Montgomery, U.
//   products  hr_mul(x, y) always folds: F x F -> F at any depth (s^5 is three products, the memory and nnf chains at most five).
//   accumulators  as honk_relations.hpp: acc_s + term is folded after every edge, the workgroup's sum after every addition, and the
//     result leaves through canonical_narrow().pack(). No bound depends on the range, the stride, the pass count or the data.
#pragma once
#include "honk_relations.hpp"

namespace csh {

constexpr int HG_COLS = 19;

enum HgCol : int {
  HG_W_L = 0, HG_W_R, HG_W_O, HG_W_4, HG_W_L_SHIFT, HG_W_R_SHIFT, HG_W_O_SHIFT, HG_W_4_SHIFT,
  HG_Q_M, HG_Q_C, HG_Q_L, HG_Q_R, HG_Q_O, HG_Q_4,
  HG_Q_ELLIPTIC, HG_Q_MEMORY, HG_Q_NNF, HG_Q_POSEIDON2_EXTERNAL, HG_Q_POSEIDON2_INTERNAL
};

// The groups, as honk_stage.hpp reads them: running sums, points, edges per pass of a workgroup (6 x 42 = 7 x 36 = 252 lanes of 256 at
// work), two waves per SIMD asked of the launch bound, then where each sum lies in acc[110] and its length.
enum HgGroupId : int { HG_EN = 0, HG_MEM = 1, HG_POS = 2 };
constexpr HsGroup hg_group(int g) {
  return g == HG_EN    ? HsGroup{3, 6, 42, 2, {0, 6, 48}, {6, 6, 6}}  // elliptic.r0, r1, nnf.r0
         : g == HG_MEM ? HsGroup{6, 6, 42, 2, {12, 18, 24, 30, 36, 42}, {6, 6, 6, 6, 6, 6}}
                       : HsGroup{8, 7, 36, 2, {54, 61, 68, 75, 82, 89, 96, 103}, {7, 7, 7, 7, 7, 7, 7, 7}};
}

// The constants of a call beside HsArgs's; hg_consts finds a.one set (hs_args)
template <class F>
struct HgArgs : HsArgs<F, HG_COLS> {
  F etad[3], diagd[4], limbd, sublimbd;  // eta_1..3 R', mat_internal_diag_m_1[0..4) R', 2^68 R', 2^14 R'
  F curve_b, one;                        // arkworks-Montgomery
};
template <class F>
inline void hg_consts(HgArgs<F>& a, const uint64_t* params) {
  for (int i = 0; i < 3; ++i) a.etad[i] = fr_to_rprime(fr_load<F>(params + 4 * i));
  a.curve_b = fr_load<F>(params + 12);
  for (int i = 0; i < 4; ++i) a.diagd[i] = fr_to_rprime(fr_load<F>(params + 16 + 4 * i));
  F pw = F::add(a.one, a.one), sub = a.one, limb = a.one;  // 2^14 and 2^68 by square and multiply on 2
  for (int bit = 0; bit < 7; ++bit, pw = F::mul(pw, pw)) {
    if ((14 >> bit) & 1) sub = F::mul(sub, pw);
    if ((68 >> bit) & 1) limb = F::mul(limb, pw);
  }
  a.sublimbd = fr_to_rprime(sub);
  a.limbd = fr_to_rprime(limb);
}

template <class F>
using HgPoint = HsPoint<HgArgs<F>>;  // the per-point view of one edge (honk_stage.hpp)

// folded sums: F from at most three terms of F
template <class LZ>
CSH_HD LZ hg_add(const LZ& x, const LZ& y) {
  return LZ::add(x, y).fold_top();
}
template <class LZ>
CSH_HD LZ hg_sub(const LZ& x, const LZ& y) {
  return LZ::sub(x, y).fold_top();
}
template <class LZ>
CSH_HD LZ hg_add3(const LZ& x, const LZ& y, const LZ& z) {
  return LZ::add(LZ::add(x, y), z).fold_top();
}

// ---- the five relations at one point, in the shape of the reference's verify_accumulate; `sc` = the edge's scaling factor (U) ----------
// elliptic_relation.rs:163-240
template <class F, class LZ>
CSH_HD void hg_elliptic_at(const HgPoint<F>& p, const LZ& sc, LZ& r0, LZ& r1) {
  const LZ x_1 = p.at(HG_W_R), y_1 = p.at(HG_W_O), x_2 = p.at(HG_W_L_SHIFT), y_2 = p.at(HG_W_4_SHIFT);
  const LZ y_3 = p.at(HG_W_O_SHIFT), x_3 = p.at(HG_W_R_SHIFT), q_sign = p.at(HG_Q_L);
  const LZ qes = hr_mul(p.at(HG_Q_ELLIPTIC), sc);
  const LZ q_double = hr_mul(qes, p.at(HG_Q_M)), q_not_double = hg_sub(qes, q_double);
  const LZ x_diff = hg_sub(x_2, x_1), y1_sqr = hr_mul(y_1, y_1), y1_plus_y3 = hg_add(y_1, y_3);
  {  // point addition
    const LZ y1y2 = hr_mul(hr_mul(y_1, y_2), q_sign);
    LZ t = hr_mul(hg_add3(x_3, x_2, x_1), hr_mul(x_diff, x_diff));
    t = LZ::sub(LZ::sub(t, hr_mul(y_2, y_2)), y1_sqr).fold_top();
    t = hg_add3(t, y1y2, y1y2);
    r0 = hr_mul(t, q_not_double);
    const LZ y_diff = hg_sub(hr_mul(y_2, q_sign), y_1);
    r1 = hr_mul(LZ::add(hr_mul(y1_plus_y3, x_diff), hr_mul(LZ::sub(x_3, x_1), y_diff)), q_not_double);
  }
  // point doubling; x_1^3 = y_1^2 - curve_b lowers the degree by one
  const LZ x1_mul_3 = hg_add3(x_1, x_1, x_1);
  const LZ x_pow_4_mul_3 = hr_mul(LZ::sub(y1_sqr, LZ::unpack(p.a.curve_b)), x1_mul_3);
  LZ y1_sqr_mul_4 = hg_add(y1_sqr, y1_sqr);
  y1_sqr_mul_4 = hg_add(y1_sqr_mul_4, y1_sqr_mul_4);
  const LZ x1_pow_4_mul_9 = hg_add3(x_pow_4_mul_3, x_pow_4_mul_3, x_pow_4_mul_3);
  const LZ x_double = LZ::sub(hr_mul(hg_add3(x_3, x_1, x_1), y1_sqr_mul_4), x1_pow_4_mul_9);
  r0 = hg_add(r0, hr_mul(x_double, q_double));
  const LZ x1_sqr_mul_3 = hr_mul(x1_mul_3, x_1);
  const LZ y_double = LZ::sub(hr_mul(LZ::sub(x_1, x_3), x1_sqr_mul_3), hr_mul(LZ::add(y_1, y_1), y1_plus_y3));
  r1 = hg_add(r1, hr_mul(y_double, q_double));
}
// non_native_field_relation.rs:179-269
template <class F, class LZ>
CSH_HD void hg_nnf_at(const HgPoint<F>& p, const LZ& sc, LZ& r0) {
  const LZ limb = LZ::unpack(p.a.limbd), sub = LZ::unpack(p.a.sublimbd);
  const LZ w_1 = p.at(HG_W_L), w_2 = p.at(HG_W_R), w_3 = p.at(HG_W_O), w_4 = p.at(HG_W_4);
  const LZ w_1s = p.at(HG_W_L_SHIFT), w_2s = p.at(HG_W_R_SHIFT), w_3s = p.at(HG_W_O_SHIFT), w_4s = p.at(HG_W_4_SHIFT);
  const LZ q_4 = p.at(HG_Q_4), q_m = p.at(HG_Q_M), q_3 = p.at(HG_Q_O);
  LZ limb_subproduct = hg_add(hr_mul(w_1, w_2s), hr_mul(w_1s, w_2));
  LZ gate_2 = LZ::sub(LZ::add(hr_mul(w_1, w_4), hr_mul(w_2, w_3)), w_3s).fold_top();
  gate_2 = hr_mulc(gate_2, limb);
  gate_2 = hr_mul(LZ::add(LZ::sub(gate_2, w_4s), limb_subproduct).fold_top(), q_4);
  limb_subproduct = hg_add(hr_mulc(limb_subproduct, limb), hr_mul(w_1s, w_2s));
  const LZ gate_1 = hr_mul(LZ::sub(LZ::sub(limb_subproduct, w_3), w_4).fold_top(), q_3);
  LZ gate_3 = LZ::sub(LZ::add(limb_subproduct, w_4), w_3s).fold_top();
  gate_3 = hr_mul(LZ::sub(gate_3, w_4s), q_m);
  const LZ identity = hr_mul(hg_add3(gate_1, gate_2, gate_3), p.at(HG_Q_R));
  // ((((w2' 2^14 + w1') 2^14 + w3) 2^14 + w2) 2^14 + w1 - w4) q_4 and ((((w3' 2^14 + w2') 2^14 + w1') 2^14 + w4) 2^14 + w3 - w4') q_m
  LZ acc_1 = hr_mulc(w_2s, sub);
  acc_1 = hr_mulc(LZ::add(acc_1, w_1s), sub);
  acc_1 = hr_mulc(LZ::add(acc_1, w_3), sub);
  acc_1 = hr_mulc(LZ::add(acc_1, w_2), sub);
  acc_1 = hr_mul(LZ::sub(LZ::add(acc_1, w_1), w_4).fold_top(), q_4);
  LZ acc_2 = hr_mulc(w_3s, sub);
  acc_2 = hr_mulc(LZ::add(acc_2, w_2s), sub);
  acc_2 = hr_mulc(LZ::add(acc_2, w_1s), sub);
  acc_2 = hr_mulc(LZ::add(acc_2, w_4), sub);
  acc_2 = hr_mul(LZ::sub(LZ::add(acc_2, w_3), w_4s).fold_top(), q_m);
  const LZ limb_accumulators = hr_mul(LZ::add(acc_1, acc_2), q_3);
  r0 = hr_mul(hr_mul(LZ::add(identity, limb_accumulators), p.at(HG_Q_NNF)), sc);
}
// memory_relation.rs:360-561. The six terms go to sum(s, term) as soon as each is complete, and every wire is read where its last use
// begins, so that at most nine values are live beside the six running sums (the kernel's register budget).
template <class F, class LZ, class Sum>
CSH_HD void hg_memory_at(const HgPoint<F>& p, const LZ& sc, Sum&& sum) {
  const LZ eta = LZ::unpack(p.a.etad[0]), eta_two = LZ::unpack(p.a.etad[1]), eta_three = LZ::unpack(p.a.etad[2]), one = p.one();
  const LZ qms = hr_mul(p.at(HG_Q_MEMORY), sc);
  LZ record, index_delta_is_zero, monotone, timestamp, value_delta, record_delta, next_access;
  {
    const LZ w_4 = p.at(HG_W_4);
    {
      const LZ w_3 = p.at(HG_W_O);
      {
        const LZ w_2 = p.at(HG_W_R);
        {
          // q_c + w_1 eta + w_2 eta_two + w_3 eta_three - w_4: the record check, and the negated access type of the RAM check
          const LZ w_1 = p.at(HG_W_L);
          record = hg_add3(hr_mulc(w_3, eta_three), hr_mulc(w_2, eta_two), hr_mulc(w_1, eta));
          record = LZ::sub(LZ::add(record, p.at(HG_Q_C)), w_4).fold_top();
          const LZ w_1s = p.at(HG_W_L_SHIFT);
          const LZ neg_index_delta = hg_sub(w_1, w_1s);
          index_delta_is_zero = hg_add(neg_index_delta, one);
          monotone = hg_add(hr_mul(neg_index_delta, neg_index_delta), neg_index_delta);
          next_access = hr_mulc(w_1s, eta);
        }
        const LZ w_2s = p.at(HG_W_R_SHIFT);
        timestamp = hg_sub(hr_mul(LZ::sub(w_2s, w_2), index_delta_is_zero), w_3);
        next_access = hg_add(next_access, hr_mulc(w_2s, eta_two));
      }
      const LZ w_3s = p.at(HG_W_O_SHIFT);
      value_delta = hr_mul(LZ::sub(w_3s, w_3), index_delta_is_zero);
      next_access = hg_add(next_access, hr_mulc(w_3s, eta_three));
    }
    const LZ w_4s = p.at(HG_W_4_SHIFT);
    record_delta = hr_mul(LZ::sub(w_4s, w_4), index_delta_is_zero);
    next_access = hg_sub(next_access, w_4s);
  }
  LZ identity;
  {
    const LZ q_1 = p.at(HG_Q_L);
    {
      const LZ q_one_by_two = hr_mul(q_1, p.at(HG_Q_R)), q12ms = hr_mul(q_one_by_two, qms);
      sum(1, hr_mul(record_delta, q12ms));
      sum(2, hr_mul(monotone, q12ms));
      identity = hr_mul(record, q_one_by_two);
    }
    identity = hg_add3(identity, hr_mul(timestamp, hr_mul(p.at(HG_Q_4), q_1)), hr_mul(record, hr_mul(p.at(HG_Q_M), q_1)));
  }
  // memory_relation.rs:552-558: the three terms take q_memory sc here; the RAM term has it already (q3ms)
  identity = hr_mul(identity, qms);
  const LZ q3ms = hr_mul(p.at(HG_Q_O), qms);
  sum(0, hg_add(identity, hr_mul(hg_add(hr_mul(record, record), record), q3ms)));
  sum(3, hr_mul(hr_mul(value_delta, hg_add(next_access, one)), q3ms));
  sum(4, hr_mul(monotone, q3ms));
  sum(5, hr_mul(hg_add(hr_mul(next_access, next_access), next_access), q3ms));
}
// (w + q)^5
template <class LZ>
CSH_HD LZ hg_sbox(const LZ& w, const LZ& q) {
  const LZ s = hg_add(w, q), s2 = hr_mul(s, s);
  return hr_mul(hr_mul(s2, s2), s);
}
// poseidon2_external_relation.rs:207-281
template <class F, class LZ>
CSH_HD void hg_poseidon2_external_at(const HgPoint<F>& p, const LZ& sc, LZ& r0, LZ& r1, LZ& r2, LZ& r3) {
  const LZ u_1 = hg_sbox(p.at(HG_W_L), p.at(HG_Q_L)), u_2 = hg_sbox(p.at(HG_W_R), p.at(HG_Q_R));
  const LZ u_3 = hg_sbox(p.at(HG_W_O), p.at(HG_Q_O)), u_4 = hg_sbox(p.at(HG_W_4), p.at(HG_Q_4));
  // v = M_E u with the reference's fourteen additions, each folded
  const LZ t_0 = hg_add(u_1, u_2), t_1 = hg_add(u_3, u_4);
  const LZ t_2 = hg_add3(u_2, u_2, t_1), t_3 = hg_add3(u_4, u_4, t_0);
  LZ v_4 = hg_add(t_1, t_1);
  v_4 = hg_add3(v_4, v_4, t_3);
  LZ v_2 = hg_add(t_0, t_0);
  v_2 = hg_add3(v_2, v_2, t_2);
  const LZ v_1 = hg_add(t_3, v_2), v_3 = hg_add(t_2, v_4);
  const LZ qs = hr_mul(p.at(HG_Q_POSEIDON2_EXTERNAL), sc);
  r0 = hr_mul(LZ::sub(v_1, p.at(HG_W_L_SHIFT)), qs);
  r1 = hr_mul(LZ::sub(v_2, p.at(HG_W_R_SHIFT)), qs);
  r2 = hr_mul(LZ::sub(v_3, p.at(HG_W_O_SHIFT)), qs);
  r3 = hr_mul(LZ::sub(v_4, p.at(HG_W_4_SHIFT)), qs);
}
// poseidon2_internal_relation.rs:202-270
template <class F, class LZ>
CSH_HD void hg_poseidon2_internal_at(const HgPoint<F>& p, const LZ& sc, LZ& r0, LZ& r1, LZ& r2, LZ& r3) {
  const LZ u_1 = hg_sbox(p.at(HG_W_L), p.at(HG_Q_L)), u_2 = p.at(HG_W_R), u_3 = p.at(HG_W_O), u_4 = p.at(HG_W_4);
  const LZ sum = hg_add(hg_add(u_1, u_2), hg_add(u_3, u_4));
  const LZ qs = hr_mul(p.at(HG_Q_POSEIDON2_INTERNAL), sc);
  r0 = hr_mul(LZ::sub(hg_add(hr_mulc(u_1, LZ::unpack(p.a.diagd[0])), sum), p.at(HG_W_L_SHIFT)), qs);
  r1 = hr_mul(LZ::sub(hg_add(hr_mulc(u_2, LZ::unpack(p.a.diagd[1])), sum), p.at(HG_W_R_SHIFT)), qs);
  r2 = hr_mul(LZ::sub(hg_add(hr_mulc(u_3, LZ::unpack(p.a.diagd[2])), sum), p.at(HG_W_O_SHIFT)), qs);
  r3 = hr_mul(LZ::sub(hg_add(hr_mulc(u_4, LZ::unpack(p.a.diagd[3])), sum), p.at(HG_W_4_SHIFT)), qs);
}

// One edge at one point into the running sums of group G (each in F before and after): the body of the reference's loop with the skips
// of elliptic_relation.rs:63-69, memory_relation.rs:114-117, non_native_field_relation.rs:59-62, poseidon2_external_relation.rs:92-95
// and poseidon2_internal_relation.rs:94-97.
template <int G, class F, class LZ>
CSH_HD void hg_accumulate_edge(const HgArgs<F>& a, size_t j, int k, LZ (&acc)[hg_group(G).sums]) {
  const HgPoint<F> p(a, j, k);
  auto sum = [&](int s, const LZ& term) CSH_LAMBDA_INLINE { acc[s] = LZ::add(acc[s], term).fold_top(); };
  if (G == HG_EN) {
    if (!p.zero_at_both_ends(HG_Q_ELLIPTIC)) {
      LZ r0, r1;
      hg_elliptic_at(p, p.scaling(), r0, r1);
      sum(0, r0), sum(1, r1);
    }
    if (!p.zero_at_both_ends(HG_Q_NNF)) {
      LZ r0;
      hg_nnf_at(p, p.scaling(), r0);
      sum(2, r0);
    }
  } else if (G == HG_MEM) {
    if (!p.zero_at_both_ends(HG_Q_MEMORY)) hg_memory_at(p, p.scaling(), sum);
  } else {
    if (!p.zero_at_both_ends(HG_Q_POSEIDON2_EXTERNAL)) {
      LZ r0, r1, r2, r3;
      hg_poseidon2_external_at(p, p.scaling(), r0, r1, r2, r3);
      sum(0, r0), sum(1, r1), sum(2, r2), sum(3, r3);
    }
    if (!p.zero_at_both_ends(HG_Q_POSEIDON2_INTERNAL)) {
      LZ r0, r1, r2, r3;
      hg_poseidon2_internal_at(p, p.scaling(), r0, r1, r2, r3);
      sum(4, r0), sum(5, r1), sum(6, r2), sum(7, r3);
    }
  }
}

// The family, as honk_stage.hpp reads it
struct HgFam {
  template <class F>
  using Args = HgArgs<F>;
  static constexpr int COLS = HG_COLS, PARAMS = 8, ACC_ELEMS = 110, GROUPS = 3;  // params: eta_1..3, curve_b, the four diagonal values
  static constexpr HsGroup group(int g) { return hg_group(g); }
  template <class F>
  static void consts(HgArgs<F>& a, const uint64_t* params) { hg_consts(a, params); }
  template <int G, class F, class LZ>
  CSH_HD static void accumulate_edge(const HgArgs<F>& a, size_t j, int k, LZ (&acc)[hg_group(G).sums]) { hg_accumulate_edge<G>(a, j, k, acc); }
};
static_assert(hs_family_ok<HgFam>(), "the accumulators tile acc[110], none is longer than its group's points, every (point, edge slot) has a lane");

}  // namespace csh
