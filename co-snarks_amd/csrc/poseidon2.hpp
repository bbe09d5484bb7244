// Batched Poseidon2 (mpc-core/src/gadgets/poseidon2/, gadgets/merkle_tree/): what the kernels of poseidon2.hip and the
// host self-test (selftest.hip, limb-bound checks on) share -- the parameter table, the per-state functions and the bound derivation.
// d = 5, t = 2, 3, 4. The library builds in no parameter set: round numbers, round constants and the diagonal are the caller's.
//
// Scale. The plain permutation keeps its state in the R' domain of the signed lazy field (field29.hpp): from_fp() on the way in, to_fp() on
// the way out (two products against about 490 at t = 4), so the s-box squares need no scaling and the constants -- brought to R' once, at
// csh_poseidon2_params_create -- are added as they are. The collaborative step (p2_co_step_at) works on shares that come from and go back
// to memory every network round, so it stays at the arkworks scale R: every product there has one public factor (a power of the opened y,
// or the diagonal) in R' and one share in R, mul(share R, public R') = R; its round constants are the table's second, unconverted copy.
//
// Bounds. Invariant I of a state element between two linear layers: limbs 0..NL-2 in [0, 2^B), a small signed top limb, value within
// (-p - eps, 2 p + eps), eps < 1e-4 p: what unpack() of a loaded element, from_fp(), mul() and fold_top() return. p / R' < 1 / 67.
//   add_rc: x + rc, rc canonical: limbs < 2^(B+1), value in (-p, 3 p + eps). normalized() goes HERE, once per s-box input: limbs <= 2^B + 1
//       (LIM1, what sqr takes); the value is unchanged.
//   s-box: x2 = sqr(x) in (-0.14 p, 1.14 p) (|x|^2 <= 9.1 p^2, / R'), x4 = sqr(x2) in (-0.02 p, 1.02 p), x5 = mul(x4, x) in (-0.05 p, 1.05 p):
//       every operand inside mul's (-8 p, 8 p), every result with limbs 0..NL-2 in [0, 2^B). No fold_top() in the s-box.
//   linear layers (p2_lin): sum c_j x_j with non-negative weights of total W <= 17 -- matmul_m4's rows (coefficients up to 7, W = 16, 12),
//       circ(2, 1) / circ(2, 1, 1) (W = 3, 4), the internal matrices (W <= 5) and the five-term post-part r5 + 5 A + 10 B + y^5 (W = 17).
//       Limb sums are taken in 64 bits: |sum| <= 17 (2^B + 8) < 2^34, no 32-bit limb overflow whatever W <= 17 is; one signed carry sweep
//       leaves limbs 0..NL-2 in [0, 2^B); the value is within 17 (-p - eps, 2 p + eps), so fold_top()'s quotient is |k| <= 35 (exact to
//       +-1 up to 64). fold_top() goes HERE, at the end of every p2_lin: I again. (A 32-bit limb-wise M4 would overflow at weight 5:
//       5 2^29 > 2^31.)
//   t = 4 internal: m_i = mul(x_i, diag_i), diag canonical: (-0.05 p, 1.05 p); m_i + x_0 + .. + x_3 is a p2_lin of W = 5.
//   post-part: yd = from_fp(y), y2 = sqr(yd), y3 = mul(y2, yd), y4 = sqr(y2), all in (-0.02 p, 1.02 p) with limbs in [0, 2^B);
//       A = reduce(r4 yd + r y4), B = reduce(r3 y2 + r2 y3): two products of normalised operands in one column sum (mul_add_wide's
//       contract), |w| <= 2.1 p^2 < p R', results in (-p / 16, p + p / 16); y5 = mul(y4, unpack(y)).
//   pre-part: x (+) rc - r: limbs within (-2^B, 2^(B+1)), value in (-2 p - eps, 3 p + eps): canonical_wide().
// No bound depends on n, on the round numbers or on the data: every round starts from I and ends in I.
#pragma once
#include <vector>

#include "common.hpp"
#include "field.hpp"
#include "field29.hpp"
#include "fr_entry.hpp"

namespace csh {

// every per-state function is inlined into its kernel: a call would pass the state through memory (scratch)
#define P2_FN CSH_HD __attribute__((always_inline))

// f(0), .., f(T - 1) with the index a constant, written out: a "#pragma unroll" loop whose body holds several inlined products exceeds the
// compiler's pragma-unroll size threshold from t = 3 on and silently stays a loop, which puts the state into scratch (dynamic index)
template <int J>
struct P2Idx {
  static constexpr int value = J;
  CSH_HD constexpr operator int() const { return J; }
};
template <int T, class Fn>
P2_FN void p2_each(Fn&& f) {
  f(P2Idx<0>{});
  f(P2Idx<1>{});
  if constexpr (T > 2) f(P2Idx<2>{});
  if constexpr (T > 3) f(P2Idx<3>{});
}

constexpr int P2_SPONGE = 0, P2_COMPRESSION = 1;
constexpr uint32_t P2_MAX_ROUNDS = 1024;  // each of rounds_f_beginning, rounds_f_end, rounds_p

// The parameter table as a kernel sees it. The vectors live behind one allocation (device memory for the kernels, host memory for the
// self-test); the round index that addresses them is the same for every lane of a launch.
template <class F>
struct P2Table {
  const F* rc_ext_rp;  // (rf_b + rf_e) * t external round constants, R' domain
  const F* rc_int_rp;  // rp internal round constants, R' domain
  const F* rc_ext;     // the same, arkworks (the collaborative step adds them to shares)
  const F* rc_int;
  F diag_rp[4];        // mat_internal_diag_m_1, R' domain (read at t = 4 only)
  uint32_t t, rf_b, rf_e, rp;
  CSH_HD uint32_t rounds() const { return rf_b + rp + rf_e; }
  CSH_HD bool external(uint32_t r) const { return r < rf_b || r >= rf_b + rp; }
  // index of round r's constants: the end rounds go on at rounds_f_beginning (poseidon2_permutation.rs:209-213)
  CSH_HD uint32_t rc_index(uint32_t r) const { return r < rf_b ? r : (r < rf_b + rp ? r - rf_b : r - rp); }
  CSH_HD size_t elems() const { return 2 * ((size_t)(rf_b + rf_e) * t + rp); }
};
// [rc_ext R' | rc_int R' | rc_ext | rc_int] from the caller's arkworks words, and the diagonal
template <class F>
inline void p2_build_table(uint32_t t, uint32_t rf_b, uint32_t rf_e, uint32_t rp, const uint64_t* rc_ext, const uint64_t* rc_int, const uint64_t* diag,
                           std::vector<F>& store, P2Table<F>& tab) {
  const size_t ne = (size_t)(rf_b + rf_e) * t;
  store.resize(2 * (ne + rp));
  for (size_t i = 0; i < ne; ++i) store[ne + rp + i] = fr_load<F>(rc_ext + 4 * i), store[i] = fr_to_rprime(store[ne + rp + i]);
  for (size_t i = 0; i < rp; ++i) store[2 * ne + rp + i] = fr_load<F>(rc_int + 4 * i), store[ne + i] = fr_to_rprime(store[2 * ne + rp + i]);
  for (uint32_t i = 0; i < 4; ++i) tab.diag_rp[i] = i < t ? fr_to_rprime(fr_load<F>(diag + 4 * i)) : F::zero();
  tab.t = t, tab.rf_b = rf_b, tab.rf_e = rf_e, tab.rp = rp;
}
template <class F>
inline void p2_point_table(P2Table<F>& tab, const F* base) {
  const size_t ne = (size_t)(tab.rf_b + tab.rf_e) * tab.t;
  tab.rc_ext_rp = base, tab.rc_int_rp = base + ne, tab.rc_ext = base + ne + tab.rp, tab.rc_int = base + 2 * ne + tab.rp;
}

// ---- linear layers --------------------------------------------------------------------------------------------------------------------------
// sum c[j] x[j], c[j] >= 0 with total weight <= 17, every x[j] with limbs 0..NL-2 within LIM1 and value within (-p - eps, 2 p + eps):
// 64-bit limb sums, one signed carry sweep, fold_top(). The result satisfies I (see the head of the file).
template <class LZ, int N>
P2_FN LZ p2_lin(const LZ (&x)[N], const int (&c)[N]) {
  constexpr int NL = LZ::NL;
  constexpr uint32_t MASK = (uint32_t(1) << LZ::B) - 1;
#pragma unroll
  for (int j = 0; j < N; ++j) CSH_LIMB_BOUND(x[j], LZ::LIM1, "p2_lin(x)");
  LZ r;
  int64_t carry = 0;
#pragma unroll
  for (int i = 0; i < NL; ++i) {
    int64_t s = carry;
#pragma unroll
    for (int j = 0; j < N; ++j) s += (int64_t)c[j] * (int64_t)x[j].l[i];
    if (i < NL - 1) {
      r.l[i] = (int32_t)((uint32_t)s & MASK);
      carry = s >> LZ::B;
    } else {
      r.l[i] = (int32_t)s;
    }
  }
  return r.fold_top();
}

// matmul_external (poseidon2_permutation.rs:67-123), row by row: circ(2, 1), circ(2, 1, 1), and for t = 4 the rows that matmul_m4's
// t_6, t_5, t_7, t_4 spell out: (5 7 1 3), (4 6 1 1), (1 3 5 7), (1 1 4 6).
template <class LZ, int T>
P2_FN void p2_matmul_external(LZ (&s)[T]) {
  LZ o[T];
  if constexpr (T == 2) {
    o[0] = p2_lin<LZ, 2>(s, {2, 1});
    o[1] = p2_lin<LZ, 2>(s, {1, 2});
  } else if constexpr (T == 3) {
    o[0] = p2_lin<LZ, 3>(s, {2, 1, 1});
    o[1] = p2_lin<LZ, 3>(s, {1, 2, 1});
    o[2] = p2_lin<LZ, 3>(s, {1, 1, 2});
  } else {
    static_assert(T == 4, "t = 2, 3, 4");
    o[0] = p2_lin<LZ, 4>(s, {5, 7, 1, 3});
    o[1] = p2_lin<LZ, 4>(s, {4, 6, 1, 1});
    o[2] = p2_lin<LZ, 4>(s, {1, 3, 5, 7});
    o[3] = p2_lin<LZ, 4>(s, {1, 1, 4, 6});
  }
#pragma unroll
  for (int j = 0; j < T; ++j) s[j] = o[j];
}
// matmul_internal (:126-162): the fixed matrices [[2, 1], [1, 3]] and [[2, 1, 1], [1, 2, 1], [1, 1, 3]] for t = 2, 3 (the create entry
// refuses any other diagonal there); s_i diag_i + sum for t = 4, diag in the R' domain whatever the scale of s is.
template <class LZ, int T, class F>
P2_FN void p2_matmul_internal(LZ (&s)[T], const F (&diag_rp)[4]) {
  LZ o[T];
  if constexpr (T == 2) {
    o[0] = p2_lin<LZ, 2>(s, {2, 1});
    o[1] = p2_lin<LZ, 2>(s, {1, 3});
  } else if constexpr (T == 3) {
    o[0] = p2_lin<LZ, 3>(s, {2, 1, 1});
    o[1] = p2_lin<LZ, 3>(s, {1, 2, 1});
    o[2] = p2_lin<LZ, 3>(s, {1, 1, 3});
  } else {
    static_assert(T == 4, "t = 2, 3, 4");
    p2_each<4>([&](auto j) CSH_LAMBDA_INLINE {
      const LZ v[5] = {LZ::mul(s[j], LZ::unpack(diag_rp[j])), s[0], s[1], s[2], s[3]};
      o[j] = p2_lin<LZ, 5>(v, {1, 1, 1, 1, 1});
    });
  }
#pragma unroll
  for (int j = 0; j < T; ++j) s[j] = o[j];
}

// ---- the plain permutation, state in the R' domain -----------------------------------------------------------------------------------------
// (x + rc)^5, x within I, rc canonical (single_sbox, :33-43)
template <class LZ>
P2_FN LZ p2_sbox_rc(const LZ& x, const LZ& rc) {
  const LZ v = LZ::add(x, rc).normalized();
  const LZ v2 = LZ::sqr(v);
  return LZ::mul(LZ::sqr(v2), v);
}
// permutation_in_place (:194-214)
template <class F, int T>
P2_FN void p2_permute(const P2Table<F>& tab, LzOf<F> (&s)[T]) {
  using LZ = LzOf<F>;
  p2_matmul_external<LZ, T>(s);
  const uint32_t R = tab.rounds();
#pragma unroll 1
  for (uint32_t r = 0; r < R; ++r) {
    if (tab.external(r)) {
      const F* rc = tab.rc_ext_rp + (size_t)tab.rc_index(r) * T;
      p2_each<T>([&](auto j) CSH_LAMBDA_INLINE { s[j] = p2_sbox_rc(s[j], LZ::unpack(rc[j])); });
      p2_matmul_external<LZ, T>(s);
    } else {
      s[0] = p2_sbox_rc(s[0], LZ::unpack(tab.rc_int_rp[tab.rc_index(r)]));
      p2_matmul_internal<LZ, T>(s, tab.diag_rp);
    }
  }
}

// One launch of the plain kernel: state i takes its first `take` elements from src[i take ..) and zeros after them, is permuted, and
// either all t elements go to dst[i t ..) (the batch: take = t) or element 0 alone goes to dst[i], with src[i take] added in compression
// mode (a Merkle layer: merkle_tree/plain.rs:32-48, :135-152; the gather of the next layer is this one's `take`).
template <class F>
struct P2PlainArgs {
  P2Table<F> tab;
  const F* src;
  F* dst;
  size_t n;
  uint32_t take;
  uint32_t whole_state, feed_forward;
};
template <class F, int T>
P2_FN void p2_plain_at(const P2PlainArgs<F>& a, size_t i) {
  using LZ = LzOf<F>;
  LZ s[T];
  p2_each<T>([&](auto j) CSH_LAMBDA_INLINE { s[j] = j < (int)a.take ? LZ::from_fp(a.src[i * a.take + j]) : LZ::zero(); });
  const LZ ff = s[0];
  p2_permute<F, T>(a.tab, s);
  if (a.whole_state) {
    p2_each<T>([&](auto j) CSH_LAMBDA_INLINE { a.dst[i * T + j] = s[j].to_fp(); });
  } else {
    a.dst[i] = (a.feed_forward ? LZ::add(s[0], ff) : s[0]).to_fp();
  }
}

// ---- the collaborative step, shares at the arkworks scale ----------------------------------------------------------------------------------
// Step s of R + 1 on one component of one state (flat value u = i ncomp + comp): the post-part of round s - 1 (s >= 1), the pre-part of
// round s (s < R). The state that is stored is the one after the linear layer, before the round constant; the pre-part's values go to
// `open` alone, compactly. pre_off: the precomputation offset of round s (for step R: the offset after the last round); the post-part
// reads at pre_off minus the entries of round s - 1.
template <class F>
struct P2CoArgs {
  P2Table<F> tab;
  F* state;
  const F* y;
  const F* pre[5];  // r, r^2, r^3, r^4, r^5
  F* open;
  F* ff_out;
  size_t n_perm, pre_off;
  uint32_t step, ncomp;
  int pub_comp;
  CSH_HD size_t round_entries(uint32_t r) const { return tab.external(r) ? n_perm * tab.t : n_perm; }
};
// sbox_rep3_precomp_post (rep3.rs:358-388) / sbox_shamir_precomp_post (shamir.rs:137-153) on component `comp` of entry `idx`
template <class F>
P2_FN LzOf<F> p2_post(const P2CoArgs<F>& a, const F& y, size_t idx, uint32_t comp) {
  using LZ = LzOf<F>;
  const size_t e = idx * a.ncomp + comp;
  const LZ yd = LZ::from_fp(y), y2 = LZ::sqr(yd), y3 = LZ::mul(y2, yd), y4 = LZ::sqr(y2);
  const LZ A = LZ::reduce(LZ::mul_add_wide(LZ::unpack(a.pre[3][e]), yd, LZ::unpack(a.pre[0][e]), y4));
  const LZ B = LZ::reduce(LZ::mul_add_wide(LZ::unpack(a.pre[2][e]), y2, LZ::unpack(a.pre[1][e]), y3));
  LZ y5 = LZ::zero();
  if ((int)comp == a.pub_comp) y5 = LZ::mul(y4, LZ::unpack(y));
  const LZ v[4] = {LZ::unpack(a.pre[4][e]), A, B, y5};
  return p2_lin<LZ, 4>(v, {1, 5, 10, 1});
}
template <class F, int T>
P2_FN void p2_co_step_at(const P2CoArgs<F>& a, size_t u) {
  using LZ = LzOf<F>;
  const uint32_t comp = (uint32_t)(u & (size_t)(a.ncomp - 1));
  const size_t i = a.ncomp == 1 ? u : u >> 1;
  const bool pub = (int)comp == a.pub_comp;
  const uint32_t R = a.tab.rounds();
  F* st = a.state + (i * T) * a.ncomp + comp;
  LZ s[T];
  p2_each<T>([&](auto j) CSH_LAMBDA_INLINE { s[j] = LZ::unpack(st[(size_t)j * a.ncomp]); });
  if (a.step == 0) {
    if (a.ff_out) a.ff_out[u] = st[0];
    p2_matmul_external<LZ, T>(s);
  } else {
    const uint32_t r = a.step - 1;
    const size_t off = a.pre_off - a.round_entries(r);
    if (a.tab.external(r)) {
      p2_each<T>([&](auto j) CSH_LAMBDA_INLINE { s[j] = p2_post(a, a.y[i * T + j], off + i * T + j, comp); });
      p2_matmul_external<LZ, T>(s);
    } else {
      s[0] = p2_post(a, a.y[i], off + i, comp);
      p2_matmul_internal<LZ, T>(s, a.tab.diag_rp);
    }
  }
  // Every s[j] here left a p2_lin, i.e. a fold_top() with |k| <= 35: its value lies in (-p 1e-5, p (1 + 1e-5)) (field29.hpp at
  // canonical_narrow()), well inside the [-p, 2 p) that canonical_narrow() takes. The store does not rest on invariant I's wider range.
  p2_each<T>([&](auto j) CSH_LAMBDA_INLINE { st[(size_t)j * a.ncomp] = s[j].canonical_narrow().pack(); });
  if (a.step < R) {
    const uint32_t r = a.step, k = a.tab.rc_index(r);
    if (a.tab.external(r)) {
      p2_each<T>([&](auto j) CSH_LAMBDA_INLINE {
        LZ v = LZ::sub(s[j], LZ::unpack(a.pre[0][(a.pre_off + i * T + j) * a.ncomp + comp]));
        if (pub) v = LZ::add(v, LZ::unpack(a.tab.rc_ext[(size_t)k * T + j]));
        a.open[(i * T + j) * a.ncomp + comp] = v.canonical_wide().pack();
      });
    } else {
      LZ v = LZ::sub(s[0], LZ::unpack(a.pre[0][(a.pre_off + i) * a.ncomp + comp]));
      if (pub) v = LZ::add(v, LZ::unpack(a.tab.rc_int[k]));
      a.open[i * a.ncomp + comp] = v.canonical_wide().pack();
    }
  }
}

// ---- the next layer of a collaborative tree (merkle_tree/rep3.rs:44-52, :99-111; shamir.rs the same) ---------------------------------------
// state: len states of t shares (a layer after its permutation), ff: len shares (element 0 of every state before it) or NULL. Output value
// v = (i t + j) ncomp + comp of the len / arity next states: state (arity i + j)'s element 0 (+ its feed-forward) for j < arity, zero after.
// len == 1 is the root: one share, state 0's element 0 (+ ff[0]). Affine, the same for every party.
template <class F>
struct P2NextArgs {
  const F* state;
  const F* ff;
  F* next;
  size_t len;
  uint32_t ncomp, t, arity;
  CSH_HD size_t values() const { return len == 1 ? ncomp : len / arity * t * ncomp; }
};
template <class F>
P2_FN void p2_next_at(const P2NextArgs<F>& a, size_t v) {
  const size_t comp = v % a.ncomp, e = v / a.ncomp, i = e / a.t, j = e % a.t;
  if (a.len != 1 && j >= a.arity) {
    a.next[v] = F::zero();
    return;
  }
  const size_t srcs = a.len == 1 ? 0 : a.arity * i + j;
  F x = a.state[srcs * a.t * a.ncomp + comp];
  if (a.ff) x = F::add(x, a.ff[srcs * a.ncomp + comp]);
  a.next[v] = x;
}

}  // namespace csh
