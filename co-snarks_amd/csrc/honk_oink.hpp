// The whole-trace loops of co-noir's UltraHonk Oink prover that are affine in the shares (honk_oink.hip), all of
// co-noir/co-ultrahonk/src/co_oink/co_oink_prover.rs (plain twin: co-noir/ultrahonk/src/oink/oink_prover.rs): the memory records added to
// w_4 (add_ram_rom_memory_records_to_wire_4 + compute_w4_inner, :98-160), the operands of the log-derivative lookup inverses
// (compute_logderivative_inverses + compute_lookup_term + compute_table_term, :162-293), the operands of the permutation grand product
// (batched_grand_product_num_denom, :344-451) and the placement of z_perm (the tail of compute_grand_product, :472-504). What the kernels
// and the host self-test (selftest.hip, limb-bound checks on) share: the argument structs, how the host fills them in, the per-index loop
// bodies, and the derivation of the lazy-field bounds. Notation, scale and the classes U / M / T / D are those of plonk_quot.hpp; F is the
// result of fold_top() as in plonk_rounds.hpp (limbs 0..NL-2 in [0, 2^B), value in (-p - eps, 2 p + eps)).
//
// The reference's clone + resize of w_4 (:133-137) is csh_poly_lincomb_dev with one share term of coefficient one and out_len = n: there
// is no copy kernel here.
//
// Bounds. p / R' < 1 / 64 throughout.
//   w4 records: r = reduce(mul_add_wide(w_l, eta_1 R', w_r, eta_2 R')), all four U: the sum is below 2 p^2 < p R' / 32, r in (0, p + p / 16).
//     w_4 + r + mul(w_o, eta_3 R') is U + M + M, three terms (limbs < 3 2^29), normalized() (limbs <= 2^B + 3); the public one or the type
//     share (U) joins: limbs < 2^30 + 3, value in (-p / 8, 4.2 p). canonical_wide().
//   lookup read term, in Horner form: d_k = w_k + mul(sh(w_k), 32 q) is U + M (T as second operand): limbs < 2^30, value in (-p / 16, 2.1 p).
//     On the public component d_3 takes mul(q_o, beta R') (M): three terms, limbs < 3 2^29. d_3.normalized() (limbs <= 2^B + 3, LIM1) is the
//     first operand of the mul by beta R' (U), which gives M; h_2 = d_2 + M has three terms and is normalized() likewise; read = d_1 +
//     mul(h_2, beta R') has three terms, and where gamma (U) joins it is normalized() first: limbs < 2^30 + 3, value in (-p / 5, 4.2 p).
//     fold_top() (|k| <= 64) returns F.
//   lookup write term, in Horner form: table_3 + mul(table_4, beta R') and table_2 + mul(that, beta R') are U + M: limbs < 2^30, the LIM2
//     first operand of a single mul, value in (-p / 16, 2.1 p). table_1 + gamma + M: three terms, value in (-p / 16, 3.1 p).
//     canonical_wide() makes it U, times32() T.
//   prod = mul(F, T): |F| < 2.01 p, T in [0, 32 p): the product lies in (-64 p^2, 64 p^2), so the result is in (-p, 2 p): canonical_wide().
//   sel: 1 - q_lookup in the 32-bit field (canonical), mul(tag, 32 (1 - q)) is M; + q (U) on the public component: canonical_wide().
//   perm operands: pq_e3_elem of plonk_quot.hpp, unchanged: U + M + U through canonical_wide().
//   z_perm placement moves elements: no lazy values.
// No bound depends on n, on the ranges or on the data.
#pragma once
#include <vector>

#include "plonk_quot.hpp"

namespace csh {

constexpr size_t HO_MAX_RANGES = 32;           // one range per non-empty trace block (co-builder/src/keys/plain_proving_key.rs:137-142)
constexpr uint32_t HO_NONE = 0xFFFFFFFFu;      // ho_place_src: the element takes no grand-product value

// ---- active ranges ----------------------------------------------------------------------------------------------------------------------
// [start_r, end_r) with pre_r = the number of active indices before range r: idx(t) = start_r + (t - pre_r) for the last r with
// pre_r <= t (ActiveRegionData::get_idx). A call without ranges carries the one range [0, domain_size). 388 B of kernel arguments, read
// with a uniform loop counter.
struct HoRanges {
  uint32_t start[HO_MAX_RANGES], end[HO_MAX_RANGES], pre[HO_MAX_RANGES];
  uint32_t nr;      // >= 1
  uint32_t active;  // A = the sum of the lengths
};
// the rules of entries 3 and 4 for n, domain_size and the ranges; fills R
inline int ho_ranges(HoRanges& R, const size_t* ranges, size_t num_ranges, size_t n, size_t domain_size, const char* what) {
  memset(&R, 0, sizeof R);
  if (n < 2 || n > FR_MAX_N) {
    set_error("%s: n must be 2 .. 2^28", what);
    return CSH_ERR_INVALID;
  }
  if (domain_size < 1 || domain_size > n) {
    set_error("%s: domain_size must be 1 .. n", what);
    return CSH_ERR_INVALID;
  }
  if (num_ranges > HO_MAX_RANGES) {
    set_error("%s: at most 32 active ranges", what);
    return CSH_ERR_INVALID;
  }
  if (num_ranges && !ranges) {
    set_error("%s: NULL argument", what);
    return CSH_ERR_INVALID;
  }
  if (num_ranges == 0) {
    R.nr = 1, R.start[0] = 0, R.end[0] = R.active = (uint32_t)domain_size;
    return CSH_OK;
  }
  size_t prev_end = 0, count = 0;
  for (size_t r = 0; r < num_ranges; ++r) {
    const size_t s = ranges[2 * r], e = ranges[2 * r + 1];
    if (s >= e || s < prev_end || e > n) {
      set_error("%s: every active range must be non-empty, begin at or after the end of the one before it, and end at or before n", what);
      return CSH_ERR_INVALID;
    }
    R.start[r] = (uint32_t)s, R.end[r] = (uint32_t)e, R.pre[r] = (uint32_t)count;
    count += e - s;
    prev_end = e;
  }
  R.nr = (uint32_t)num_ranges, R.active = (uint32_t)count;
  return CSH_OK;
}
// idx(t), t < A
CSH_HD uint32_t ho_idx(const HoRanges& R, uint32_t t) {
  uint32_t j = t;
#pragma unroll 1
  for (uint32_t r = 0; r < R.nr; ++r)
    if (t >= R.pre[r]) j = R.start[r] + (t - R.pre[r]);
  return j;
}
// The gather form of :472-504. Index i of z_perm takes mul[src]: an active index at position t >= 1 takes mul[t - 1] (:479-486); an index
// below domain_size in the gap in front of range r >= 1 takes what start_r holds, mul[pre_r - 1] (:492-503; start_r is active at position
// pre_r >= 1, so the fill never reads an element that a fill wrote). Everything else -- position 0, in front of the first range, behind
// the last, the gaps at or above domain_size -- keeps the resize's zero, or the one of :476 at index 1: HO_NONE.
CSH_HD uint32_t ho_place_src(const HoRanges& R, uint32_t domain_size, uint32_t i) {
  uint32_t src = HO_NONE, prev_end = 0;
#pragma unroll 1
  for (uint32_t r = 0; r < R.nr; ++r) {
    const uint32_t s = R.start[r], e = R.end[r], pre = R.pre[r];
    if (i >= s && i < e) {
      const uint32_t t = pre + (i - s);
      src = t ? t - 1 : HO_NONE;
    }
    if (r && i >= prev_end && i < s && i < domain_size) src = pre - 1;
    prev_end = e;
  }
  return src;
}

// ---- 1. memory records into w_4, :98-160 -------------------------------------------------------------------------------------------------
// flat index e over (n_read + n_write + n_shared) ncomp: record k = e / ncomp of the three lists laid end to end. Contract: every index is
// below n and occurs once in the call (a duplicate is a race); a lane that reads an index >= n does nothing.
template <class F>
struct HoW4Args {
  const F* w[3];  // w_l, w_r, w_o
  F* w4;
  const uint32_t *read_idx, *write_idx, *shared_idx;
  const F* type_share;  // n_shared shares
  size_t n;
  uint32_t n_read, n_write, n_shared;
  F etad[3];  // eta_k R'
  F one;      // arkworks-Montgomery
  PqGeom g;   // N = n_read + n_write + n_shared
};
template <class F>
inline void ho_w4_consts(HoW4Args<F>& a, const uint64_t* etas) {
  for (int k = 0; k < 3; ++k) a.etad[k] = fr_to_rprime(fr_load<F>(etas + 4 * k));
  a.one = F::one();
}
template <class F>
CSH_HD void ho_w4_at(const HoW4Args<F>& a, size_t e) {
  using LZ = typename LazyOf<F>::type;
  const size_t k = a.g.point(e), c = a.g.comp(e);
  const bool is_read = k < a.n_read, is_write = !is_read && k < (size_t)a.n_read + a.n_write, is_shared = !is_read && !is_write;
  const uint32_t* list = is_read ? a.read_idx : (is_write ? a.write_idx : a.shared_idx);
  const size_t off = is_read ? k : (is_write ? k - a.n_read : k - a.n_read - a.n_write);
  const size_t row = list[off];
  if (row >= a.n) return;
  const size_t v = row * a.g.ncomp + c;
  const LZ r = LZ::reduce(LZ::mul_add_wide(LZ::unpack(a.w[0][v]), LZ::unpack(a.etad[0]), LZ::unpack(a.w[1][v]), LZ::unpack(a.etad[1])));
  LZ s = LZ::add(LZ::add(LZ::unpack(a.w4[v]), r), LZ::mul(LZ::unpack(a.w[2][v]), LZ::unpack(a.etad[2]))).normalized();
  if (is_write && a.g.pub(e)) s = LZ::add(s, LZ::unpack(a.one));
  if (is_shared) s = LZ::add(s, LZ::unpack(a.type_share[off * a.g.ncomp + c]));
  a.w4[v] = s.canonical_wide().pack();
}

// ---- 2. lookup operands, :162-293 -------------------------------------------------------------------------------------------------------
// flat index e over n ncomp. The product and the selector share are a kernel each: together their 15 pointers and 5 constants do not fit
// the scalar registers.
template <class F>
struct HoLookupArgs {
  const F* w[3];    // w_l, w_r, w_o: read at i and, shifted (polynomial.rs:170-176), at i + 1; zero behind the last row
  const F* q[3];    // q_r, q_m, q_c: the negative step sizes of columns 1, 2, 3
  const F* qo;      // q_o: the table index
  const F* tab[4];  // table_1 .. table_4
  F* prod;
  F betad;  // beta R'
  F gamma;
  PqGeom g;  // N = n
};
template <class F>
inline void ho_lookup_consts(HoLookupArgs<F>& a, const uint64_t* ch) {
  a.betad = fr_to_rprime(fr_load<F>(ch));
  a.gamma = fr_load<F>(ch + 4);
}
// Both terms in Horner form, so that beta and gamma are the only constants a lane holds (with beta^2 and beta^3 beside them the kernel
// spilled scalar registers): read = d_1 (+) gamma + beta (d_2 + beta (d_3 (+) beta q_o)), write = table_1 + gamma + beta (table_2 + beta
// (table_3 + beta table_4)). The same residues as the reference's sums of powers, and outputs are canonical, so the same words.
template <class F>
CSH_HD void ho_lookup_prod_at(const HoLookupArgs<F>& a, size_t e) {
  using LZ = typename LazyOf<F>::type;
  const size_t i = a.g.point(e);
  const bool last = i + 1 == a.g.N, pub = a.g.pub(e);
  const size_t es = last ? e : e + a.g.ncomp;  // the shifted read; not used at the last row
  const LZ gamma = LZ::unpack(a.gamma), betad = LZ::unpack(a.betad);
  LZ d[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const LZ sh = last ? LZ::zero() : LZ::unpack(a.w[k][es]);
    d[k] = LZ::add(LZ::unpack(a.w[k][e]), LZ::mul(sh, LZ::unpack(a.q[k][i]).times32()));
  }
  if (pub) d[2] = LZ::add(d[2], LZ::mul(LZ::unpack(a.qo[i]), betad));                   // (+) beta q_o: beta^3 q_o after the two steps below
  const LZ h2 = LZ::add(d[1], LZ::mul(d[2].normalized(), betad)).normalized();
  LZ read = LZ::add(d[0], LZ::mul(h2, betad));
  if (pub) read = LZ::add(read.normalized(), gamma);
  const LZ t3 = LZ::add(LZ::unpack(a.tab[2][i]), LZ::mul(LZ::unpack(a.tab[3][i]), betad));
  const LZ t2 = LZ::add(LZ::unpack(a.tab[1][i]), LZ::mul(t3, betad));
  const LZ write = LZ::add(LZ::add(LZ::unpack(a.tab[0][i]), gamma), LZ::mul(t2, betad)).canonical_wide();
  a.prod[e] = LZ::mul(read.fold_top(), write.times32()).canonical_wide().pack();
}
// sel = ((1 - q_lookup) tag) (+) q_lookup, :264-271
template <class F>
struct HoSelArgs {
  const F *tag, *qlookup;
  F* sel;
  F one;
  PqGeom g;  // N = n
};
template <class F>
CSH_HD void ho_lookup_sel_at(const HoSelArgs<F>& a, size_t e) {
  using LZ = typename LazyOf<F>::type;
  const F q = a.qlookup[a.g.point(e)];
  LZ s = LZ::mul(LZ::unpack(a.tag[e]), LZ::unpack(F::sub(a.one, q)).times32());
  if (a.g.pub(e)) s = LZ::add(s, LZ::unpack(q));
  a.sel[e] = s.canonical_wide().pack();
}

// ---- 3. permutation operands, :344-451 --------------------------------------------------------------------------------------------------
// flat index e over m ncomp, m = A - 1: out_k[t] = w_k[j] (+) (beta pub_k[j] + gamma), j = idx(t). The numerators (pub = id_1..4) and the
// denominators (pub = sigma_1..4) are two launches of the one kernel, so that neither keeps the other's pointers in scalar registers.
template <class F>
struct HoPermArgs {
  const F* w[4];    // w_l, w_r, w_o, w_4
  const F* pub[4];  // id_1..4 or sigma_1..4
  F* out[4];
  F betad, gamma;   // beta R'; gamma
  HoRanges R;
  PqGeom g;         // N = m
};
template <class F>
CSH_HD void ho_perm_at(const HoPermArgs<F>& a, size_t e) {
  const size_t j = ho_idx(a.R, (uint32_t)a.g.point(e)), src = j * a.g.ncomp + a.g.comp(e);
  const bool pub = a.g.pub(e);
#pragma unroll
  for (int k = 0; k < 4; ++k) a.out[k][e] = pub ? pq_e3_elem(a.w[k][src], a.pub[k][j], a.betad, a.gamma) : a.w[k][src];
}

// ---- 4. z_perm placement, :472-504 --------------------------------------------------------------------------------------------------------
// flat index e over n ncomp; a gather: every element of z is written once, by the lane that owns it
template <class F>
struct HoPlaceArgs {
  const F* mul;  // m shares
  F* z;          // n shares
  F one;         // arkworks-Montgomery: the trivial share of one holds it on the public component
  uint32_t domain_size;
  HoRanges R;
  PqGeom g;      // N = n
};
template <class F>
CSH_HD void ho_place_at(const HoPlaceArgs<F>& a, size_t e) {
  const uint32_t i = (uint32_t)a.g.point(e);
  const uint32_t src = ho_place_src(a.R, a.domain_size, i);
  if (src != HO_NONE) a.z[e] = a.mul[(size_t)src * a.g.ncomp + a.g.comp(e)];
  else a.z[e] = (i == 1 && a.g.pub(e)) ? a.one : F::zero();
}

}  // namespace csh
