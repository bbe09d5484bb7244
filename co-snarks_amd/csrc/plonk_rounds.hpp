// The whole-vector stretches of rounds 2 and 5 of the circom PLONK prover that are affine in the shares (plonk_rounds.hip; DESIGN.md section
// 3.3e): the operands of Round2::compute_z (co-circom/co-plonk/src/round2.rs:104-155) and its rotate_right(1) (:171), blind_coefficients
// (co-plonk/src/lib.rs:162-177), and the ragged linear combination of Round5::compute_r / compute_wxi (round5.rs:118-259). What the kernels
// and the host self-test (selftest.hip, limb-bound checks on) share: the argument structs, how the host fills them in, the per-index loop
// bodies, and the derivation of the lazy-field bounds. Notation, scale and the classes U / M / T / D are those of plonk_quot.hpp.
//
// Bounds.
//   z operands: pq_e2_elem and pq_e3_elem of plonk_quot.hpp, unchanged: U + M + U through canonical_wide().
//   linear combination: the accumulator is zero, U (const0, or what an earlier launch stored in `out`: canonical) or class
//     F  the result of fold_top(): limbs 0..NL-2 in [0, 2^B), small signed top limb, value in (-p - eps, 2 p + eps).
//   A term is U (a coefficient equal to one: the element itself) or M = mul(U, c R') with c R' in U: value in (-p / 16, p + p / 16).
//   F + M has limbs below 2^30 and a value in (-1.1 p - eps, 3.1 p + eps), far inside fold_top()'s |k| <= 64, and comes back as F. So the
//   step is pq_pi_step's, and no bound depends on ks, kp, the lengths or the data. The last fold_top() of a launch is followed by
//   canonical_narrow() (input in [-p, 2 p) with a wide margin), so `out` is canonical after every launch.
//   rotate and blind move elements or use the 32-bit field's sub (canonical in, canonical out): no lazy values.
#pragma once
#include <vector>

#include "plonk_quot.hpp"

namespace csh {

constexpr int PR_LC_CHUNK = 16;  // vectors per launch of the linear combination: 16 pointers, 16 lengths, 16 constants = 768 B of kernel arguments
constexpr size_t PR_LC_MAX_TERMS = 64;

// ---- z operands, round2.rs:116-155 ----------------------------------------------------------------------------------------------------
// flat index e over n ncomp; half 0 writes n1, n2, n3 (x (+) (bk w^i + gamma), w = w_ext^4, pq_e2_elem), half 1 writes d1, d2, d3
// (x (+) (beta S[4 i] + gamma), pq_e3_elem). Each half is a kernel of its own, so that neither keeps the other's pointers and constants in
// scalar registers (one kernel for both spilled eight of them).
template <class F>
struct PrZArgs {
  const F* in[3];     // buffer_a, buffer_b, buffer_c
  const F* sigma[3];  // S1, S2, S3 on the extended domain: 4 n evaluations, read at 4 i
  F* out[6];          // n1, n2, n3, d1, d2, d3
  F bk[3];            // beta, beta k1, beta k2 (arkworks-Montgomery)
  F betad, gamma;     // beta R'; gamma
  const F *hi, *lo;   // the power table of w = w_ext^4 over n points
  PqGeom g;           // N = n
};
template <class F>
inline void pr_z_consts(PrZArgs<F>& a, const uint64_t* ch) {
  const F beta = fr_load<F>(ch), gamma = fr_load<F>(ch + 4), k1 = fr_load<F>(ch + 8), k2 = fr_load<F>(ch + 12);
  a.bk[0] = beta, a.bk[1] = F::mul(beta, k1), a.bk[2] = F::mul(beta, k2);
  a.betad = fr_to_rprime(beta);
  a.gamma = gamma;
}
// the half that needs the powers: n1, n2, n3
template <class F>
CSH_HD void pr_z_num_at(const PrZArgs<F>& a, size_t e) {
  if (!a.g.pub(e)) {  // this component takes no public value
#pragma unroll
    for (int v = 0; v < 3; ++v) a.out[v][e] = a.in[v][e];
    return;
  }
  const auto w = pq_pow(a.hi, a.lo, a.g.point(e));
#pragma unroll
  for (int v = 0; v < 3; ++v) a.out[v][e] = pq_e2_elem(a.in[v][e], w, a.bk[v], a.gamma);
}
// the half that reads the permutation polynomials: d1, d2, d3
template <class F>
CSH_HD void pr_z_den_at(const PrZArgs<F>& a, size_t e) {
  const bool pub = a.g.pub(e);
  const size_t i = a.g.point(e);
#pragma unroll
  for (int v = 0; v < 3; ++v) a.out[3 + v][e] = pub ? pq_e3_elem(a.in[v][e], a.sigma[v][4 * i], a.betad, a.gamma) : a.in[v][e];
}

// ---- rotate_right(k), round2.rs:171 ---------------------------------------------------------------------------------------------------
template <class F>
struct PrRotArgs {
  const F* in;
  F* out;
  size_t n, k;  // k < n
  uint32_t ncomp;
};
// ncomp is 1 or 2 (FR_REQUIRE_NCOMP at the C entry): e >> 1 and e & (ncomp - 1) split the flat index only then
template <class F>
CSH_HD void pr_rotate_at(const PrRotArgs<F>& a, size_t e) {
  const size_t i = a.ncomp == 1 ? e : e >> 1, c = e & (size_t)(a.ncomp - 1);
  size_t j = i + a.k;
  if (j >= a.n) j -= a.n;
  a.out[j * a.ncomp + c] = a.in[e];
}

// ---- blind_coefficients, co-plonk/src/lib.rs:162-177 ----------------------------------------------------------------------------------
// flat index e over k ncomp: coefficient j = e / ncomp takes coeff_rev[k - 1 - j]. ncomp is 1 or 2, as in pr_rotate_at
template <class F>
struct PrBlindArgs {
  F* poly;     // n + k shares
  F c[3][2];   // coeff_rev[0..k) by component, arkworks-Montgomery
  size_t n;
  uint32_t ncomp, k;
};
template <class F>
inline void pr_blind_consts(PrBlindArgs<F>& a, const uint64_t* coeff_rev, uint32_t ncomp, uint32_t k) {
  for (uint32_t j = 0; j < 3; ++j) {
    a.c[j][0] = a.c[j][1] = F::zero();
    if (j < k) pq_share(a.c[j], coeff_rev + 4 * ncomp * j, ncomp);
  }
}
template <class F>
CSH_HD void pr_blind_at(const PrBlindArgs<F>& a, size_t e) {
  const size_t j = a.ncomp == 1 ? e : e >> 1, c = e & (size_t)(a.ncomp - 1);
  const uint32_t r = a.k - 1 - (uint32_t)j;  // word-wise selects, as pq_sel4: no lane-dependent index into the arguments
  const F c0 = pq_sel(c != 0, a.c[0][1], a.c[0][0]), c1 = pq_sel(c != 0, a.c[1][1], a.c[1][0]), c2 = pq_sel(c != 0, a.c[2][1], a.c[2][0]);
  const F v = pq_sel(r == 2, c2, pq_sel(r == 1, c1, c0));
  a.poly[e] = F::sub(a.poly[e], v);
  a.poly[a.n * a.ncomp + e] = v;
}

// ---- the ragged linear combination, round5.rs:118-259 ---------------------------------------------------------------------------------
// out[i] = sum_j cs_j S_j[i] (+) (sum_j cp_j P_j[i] + [i = 0] const0). One launch takes up to PR_LC_CHUNK terms, share and public terms
// alike; the first starts from zero (and const0), a later one from what `out` holds.
template <class F>
struct PrLcArgs {
  const F* v[PR_LC_CHUNK];
  F cd[PR_LC_CHUNK];        // coefficient R' (not read where one_mask has the bit)
  size_t len[PR_LC_CHUNK];  // shares or elements, >= 1
  uint32_t pub_mask;        // bit j: v[j] is a public vector (one element per point, added on the public component only)
  uint32_t one_mask;        // bit j: the coefficient is one
  int k, first, has_const;
  F const0;                 // arkworks-Montgomery
  F* out;
  PqGeom g;                 // N = out_len
};
// the launches of one call. Terms of length zero contribute nothing and are left out; there is always a first launch, which writes the zeros.
template <class F>
inline std::vector<PrLcArgs<F>> pr_lc_launches(uint32_t protocol, uint32_t party, const uint64_t* const* shares, const size_t* share_lens,
                                               const uint64_t* share_coeffs, size_t ks, const uint64_t* const* pub, const size_t* public_lens,
                                               const uint64_t* public_coeffs, size_t kp, const uint64_t* const0, uint64_t* out, size_t out_len) {
  std::vector<PrLcArgs<F>> ls;
  auto fresh = [&]() {
    PrLcArgs<F> a;
    memset((void*)&a, 0, sizeof a);
    a.first = ls.empty();
    a.has_const = a.first && const0 != nullptr;
    if (a.has_const) a.const0 = fr_load<F>(const0);
    a.out = (F*)out;
    a.g = PqGeom{out_len, protocol + 1, pq_pub_comp(protocol, party)};
    ls.push_back(a);
  };
  fresh();
  const F one = F::one();
  auto term = [&](const uint64_t* p, size_t len, const uint64_t* coeff, bool is_public) {
    if (!len) return;
    if (ls.back().k == PR_LC_CHUNK) fresh();
    PrLcArgs<F>& a = ls.back();
    const int j = a.k++;
    const F c = fr_load<F>(coeff);
    a.v[j] = (const F*)p;
    a.len[j] = len;
    if (memcmp(&c, &one, sizeof(F)) == 0) a.one_mask |= 1u << j;
    else a.cd[j] = fr_to_rprime(c);
    if (is_public) a.pub_mask |= 1u << j;
  };
  for (size_t j = 0; j < ks; ++j) term(shares[j], share_lens[j], share_coeffs + 4 * j, false);
  for (size_t j = 0; j < kp; ++j) term(pub[j], public_lens[j], public_coeffs + 4 * j, true);
  return ls;
}
template <class F>
CSH_HD void pr_lc_at(const PrLcArgs<F>& a, size_t e) {
  using LZ = typename LazyOf<F>::type;
  const size_t i = a.g.point(e);
  const bool pub = a.g.pub(e);
  LZ acc = a.first ? LZ::zero() : LZ::unpack(a.out[e]);
  if (a.has_const && pub && i == 0) acc = LZ::unpack(a.const0);
#pragma unroll 1
  for (int j = 0; j < a.k; ++j) {
    const bool is_public = (a.pub_mask >> j) & 1u;
    if (i >= a.len[j] || (is_public && !pub)) continue;
    LZ x = LZ::unpack(a.v[j][is_public ? i : e]);
    if (!((a.one_mask >> j) & 1u)) x = LZ::mul(x, LZ::unpack(a.cd[j]));
    acc = LZ::add(acc, x).fold_top();
  }
  a.out[e] = acc.fold_top().canonical_narrow().pack();
}

}  // namespace csh
