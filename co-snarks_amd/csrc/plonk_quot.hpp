// The element-wise stages of the circom PLONK quotient (plonk_quot.hip): Round3::compute_t,
// co-circom/co-plonk/src/round3.rs:246-502. What the kernels and the host self-test (selftest.hip, limb-bound checks on) share: the
// constants of a call, the per-element expressions, and the derivation of their lazy-field bounds.
//
// Notation. N = 4 n points of the extended domain, generator w; i the point, m = i mod 4, c the component of a share (ncomp 1 or 2), flat
// value index e = i ncomp + c. A public value is added to a share ("x (+) v", add_with_public, rep3/arithmetic.rs:41-49,
// shamir/arithmetic.rs:45) on component `pub_comp` only: 0 for plain / Shamir and Rep3 party 0, 1 for Rep3 party 1, none for party 2.
//
// Scale. Elements are arkworks-Montgomery (R = 2^256 scale) and are re-sliced into 9 x 29-bit limbs as they are (unpack). A constant of the
// call is brought to the R' = 2^261 domain once on the host (fr_to_rprime, fr_entry.hpp: c R' mod p, canonical and packed), so mul(x, c') = x c R R' / R' is at
// the operands' scale again. A product of two LOADED operands scales one of them by 2^5 = R' / R (times32()), as vec_elem.hpp does. The powers
// w^i are kept in the R' domain: mul(hi', lo') of two table entries is w^i R', and mul(share, that) is at R scale.
//
// Bounds. FpS::mul / reduce (field29.hpp) take operands whose limbs 0..NL-2 are within LIM1 = 2^B + 8 (one operand of a single mul may reach
// LIM2 = 2^(B+1) + 16) and return (w + q p) / R', 0 <= q < R': limbs 0..NL-2 in [0, 2^B), a small signed top limb, value in
// (w / R', w / R' + p). p < 2^255, so 32 p < R' / 2 and p / R' < 1 / 64. Classes of values used below:
//   U  an unpacked element or constant: limbs in [0, 2^B), value in [0, p).
//   M  mul(x, y) with |x| < 4 p, y in U:  value in (-p / 16, p + p / 16), limbs as above. A valid second operand.
//   T  times32() of U or M: limbs 0..NL-2 in [0, 2^B), top limb < 2^28, |value| < 34 p.  A valid second operand.
//   D  a difference of two U: |limb| < 2^B, |value| < p.  A valid first operand (LIM1).
// Two-product sums reduce(mul_add_wide(a, b, c, d)) need all four within LIM1 (18 products of 2^58 plus the reduction's 9 fit a signed
// 64-bit column; a LIM2 operand would not), and the result lies in (w / R', w / R' + p) for the sum w, which each
// expression below bounds. A sum of three lazy values has limbs below 3 2^29 < 2^31; wherever a fourth
// term joins, normalized() (one parallel carry step, limbs <= 2^B + 3) comes first. Every result leaves through canonical_wide()
// (|value| < 32 p), so outputs are canonical. No bound depends on N, on n_public or on the data.
#pragma once
#include <string.h>

#include "common.hpp"
#include "field.hpp"
#include "field29.hpp"
#include "fr_entry.hpp"

namespace csh {

constexpr int PQ_WG = 256;          // lanes of a workgroup, as vec_ops.hip
constexpr int PQ_POW_LO_LOG = 8;    // w^i = hi[i >> 8] * lo[i & 255]: the two-level power table (256 + N / 256 entries, built on the device per call)
constexpr int PQ_PI_CHUNK = 16;     // Lagrange vectors per launch of the public-input sum: 16 pointers + 32 constants = 1152 B of kernel arguments

// word-wise selects: a lane-dependent index into a kernel argument would put the argument into scratch memory
template <class F>
CSH_HD F pq_sel(bool s, const F& x, const F& y) {
  F r;
#pragma unroll
  for (int k = 0; k < F::N; ++k) r.l[k] = s ? x.l[k] : y.l[k];
  return r;
}
template <class F>
CSH_HD F pq_sel4(const F* t, unsigned m) {
  return pq_sel((m & 2u) != 0, pq_sel((m & 1u) != 0, t[3], t[2]), pq_sel((m & 1u) != 0, t[1], t[0]));
}

// ---- powers of the generator --------------------------------------------------------------------------------------------------------
// entry of a power table: g^e R', canonical and packed; gd = g R'. Square and multiply on class-M values (sqr and mul return M for M).
template <class F>
CSH_HD F pq_power_entry(const F& gd, size_t e) {
  using LZ = typename LazyOf<F>::type;
  LZ r = LZ::one(), b = LZ::unpack(gd);
  while (e) {
    if (e & 1) r = LZ::mul(r, b);
    b = LZ::sqr(b);
    e >>= 1;
  }
  return r.canonical().pack();
}
CSH_HD size_t pq_pow_hi_count(size_t N) { return (N >> PQ_POW_LO_LOG) ? (N >> PQ_POW_LO_LOG) : 1; }
// w^i R' (class M) from the two table entries of point i
template <class F>
CSH_HD typename LazyOf<F>::type pq_pow(const F* hi, const F* lo, size_t i) {
  using LZ = typename LazyOf<F>::type;
  return LZ::mul(LZ::unpack(hi[i >> PQ_POW_LO_LOG]), LZ::unpack(lo[i & ((size_t(1) << PQ_POW_LO_LOG) - 1)]));
}

// ---- the constants a call derives on the host ---------------------------------------------------------------------------------------
// z1, z2, z3 of round3.rs:212-242 from iota = w^(N/4), the primitive 4th root of unity (Domains::root_of_unity_2), arkworks-Montgomery
template <class F>
struct PqZ {
  F z1[4], z2[4], z3[4];
};
template <class F>
inline PqZ<F> pq_z_tables(const F& gen, size_t N) {
  const F iota = F::pow_u64(gen, (uint64_t)(N / 4));
  const F zero = F::zero(), one = F::one(), two = F::add(one, one), four = F::add(two, two), eight = F::add(four, four);
  const F neg1 = F::neg(one), neg2 = F::neg(two), ti = F::mul(two, iota);
  PqZ<F> z;
  z.z1[0] = zero, z.z1[1] = F::add(neg1, iota), z.z1[2] = neg2, z.z1[3] = F::sub(neg1, iota);
  z.z2[0] = zero, z.z2[1] = F::neg(ti), z.z2[2] = four, z.z2[3] = ti;
  z.z3[0] = zero, z.z3[1] = F::add(two, ti), z.z3[2] = F::neg(eight), z.z3[3] = F::sub(two, ti);
  return z;
}

// (a) blinders, round3.rs:269-274 and 339-353
template <class F>
struct PqBlindK {
  F b[9][2];  // b0..b8 by component, arkworks-Montgomery
  F w4d;      // w^4 R': w * root_of_unity_pow of round3.rs:346
};
// b_lo + w b_hi: U + M, value in (-p / 16, 2.1 p)
template <class LZ>
CSH_HD LZ pq_affine(const LZ& b_lo, const LZ& b_hi, const LZ& w) {
  return LZ::add(b_lo, LZ::mul(b_hi, w));
}
// b8 + w (b7 + w b6): the inner sum is U + M (limbs < 2^30: the LIM2 first operand of a single mul; |value| < 2.1 p)
template <class LZ>
CSH_HD LZ pq_quadratic(const LZ& b8, const LZ& b7, const LZ& b6, const LZ& w) {
  return LZ::add(b8, LZ::mul(pq_affine(b7, b6, w), w));
}
// output v of stage (a) for component c: ap, bp, cp (v = 0, 1, 2) = b_(2v+1) + w^i b_(2v); zp (3) and zwp (4) = b8 + x b7 + x^2 b6 at x = w^i
// and x = w^(i+4). v is the same for a whole workgroup (blockIdx.y), so only the shares that output needs are read from the arguments.
template <class F>
CSH_HD F pq_blinders_elem(const PqBlindK<F>& k, int v, unsigned c, const typename LazyOf<F>::type& w) {
  using LZ = typename LazyOf<F>::type;
  auto B = [&](int j) CSH_LAMBDA_INLINE { return LZ::unpack(pq_sel(c != 0, k.b[j][1], k.b[j][0])); };
  if (v < 3) return pq_affine(B(2 * v + 1), B(2 * v), w).canonical_wide().pack();
  const LZ x = v == 3 ? w : LZ::mul(w, LZ::unpack(k.w4d));  // w^(i+4) R', class M
  return pq_quadratic(B(8), B(7), B(6), x).canonical_wide().pack();
}

// (b) public-input sum, round3.rs:377-381: acc - L buffer_a, with nb = (-buffer_a) R' (U). acc is U or an earlier step's result
// (fold_top(): value in (-p - eps, 2 p + eps)); acc + M has limbs < 2^30 and value in (-1.1 p, 3.1 p), fold_top() brings it back. So the bound
// does not depend on the number of terms.
template <class LZ>
CSH_HD LZ pq_pi_step(const LZ& acc, const LZ& lagrange, const LZ& nb) {
  return LZ::add(acc, LZ::mul(lagrange, nb)).fold_top();
}

// (b) e1 = (qm a_b + ql a + qr b + qo c + pi) (+) qc, round3.rs:364-385. Shares are U, selectors T: each pair of products is below
// 2 p 32 p < p R', so each reduction is in (0, 2 p). r1 + r2 + pi: three terms; normalized() before qc joins.
template <class F>
CSH_HD F pq_e1_elem(const F& a_b, const F& a, const F& b, const F& c, const F& pi, const F& qm, const F& ql, const F& qr, const F& qo, const F& qc,
                    bool pub) {
  using LZ = typename LazyOf<F>::type;
  const LZ r1 = LZ::reduce(LZ::mul_add_wide(LZ::unpack(a_b), LZ::unpack(qm).times32(), LZ::unpack(a), LZ::unpack(ql).times32()));
  const LZ r2 = LZ::reduce(LZ::mul_add_wide(LZ::unpack(b), LZ::unpack(qr).times32(), LZ::unpack(c), LZ::unpack(qo).times32()));
  LZ s = LZ::add(LZ::add(r1, r2), LZ::unpack(pi)).normalized();
  if (pub) s = LZ::add(s, LZ::unpack(qc));
  return s.canonical_wide().pack();
}
// (b) e1z = qm (a_bp + ap_b + z1[m] ap_bp) + ql ap + qr bp + qo cp, round3.rs:355-375. z1d = z1[m] R' (U; zero for m = 0, which is the
// reference's skipped branch). u = U + U + M, normalized(): limbs <= 2^B + 3, value in (-p / 16, 3.1 p); u 32 qm + ap 32 ql < 4.1 p 32 p <
// 2.1 p R' -- so r1 is in (0, 3 p), r2 in (0, 2 p), the sum below 5 p.
template <class F>
CSH_HD F pq_e1z_elem(const F& a_bp, const F& ap_b, const F& ap_bp, const F& ap, const F& bp, const F& cp, const F& qm, const F& ql, const F& qr,
                     const F& qo, const F& z1d) {
  using LZ = typename LazyOf<F>::type;
  const LZ u = LZ::add(LZ::add(LZ::unpack(a_bp), LZ::unpack(ap_b)), LZ::mul(LZ::unpack(ap_bp), LZ::unpack(z1d))).normalized();
  const LZ r1 = LZ::reduce(LZ::mul_add_wide(u, LZ::unpack(qm).times32(), LZ::unpack(ap), LZ::unpack(ql).times32()));
  const LZ r2 = LZ::reduce(LZ::mul_add_wide(LZ::unpack(bp), LZ::unpack(qr).times32(), LZ::unpack(cp), LZ::unpack(qo).times32()));
  return LZ::add(r1, r2).canonical_wide().pack();
}
// (b) x (+) (bk w^i + gamma), round3.rs:388-399: w = w^i R' (M, first operand), bk = beta, beta k1 or beta k2 (U). U + M + U.
template <class F>
CSH_HD F pq_e2_elem(const F& x, const typename LazyOf<F>::type& w, const F& bk, const F& gamma) {
  using LZ = typename LazyOf<F>::type;
  return LZ::add(LZ::unpack(x), LZ::add(LZ::mul(w, LZ::unpack(bk)), LZ::unpack(gamma))).canonical_wide().pack();
}
// (b) x (+) (beta s + gamma), round3.rs:402-416: betad = beta R' (U). U + M + U.
template <class F>
CSH_HD F pq_e3_elem(const F& x, const F& s, const F& betad, const F& gamma) {
  using LZ = typename LazyOf<F>::type;
  return LZ::add(LZ::unpack(x), LZ::add(LZ::mul(LZ::unpack(s), LZ::unpack(betad)), LZ::unpack(gamma))).canonical_wide().pack();
}

// (c) combine, round3.rs:88-105 and 435-467
template <class F>
struct PqCombineK {
  F alphad, alpha2d;            // alpha R', alpha^2 R'
  F az1d[4], az2d[4], az3d[4];  // alpha z_k[m] R': alpha (X0 + z1 X1 + z2 X2 + z3 X3) = alpha X0 + sum (alpha z_k) X_k
};
template <class F>
inline PqCombineK<F> pq_combine_consts(const F& gen, size_t N, const F& alpha) {
  const PqZ<F> z = pq_z_tables(gen, N);
  PqCombineK<F> k;
  k.alphad = fr_to_rprime(alpha);
  k.alpha2d = fr_to_rprime(F::mul(alpha, alpha));
  for (int m = 0; m < 4; ++m) {
    k.az1d[m] = fr_to_rprime(F::mul(alpha, z.z1[m]));
    k.az2d[m] = fr_to_rprime(F::mul(alpha, z.z2[m]));
    k.az3d[m] = fr_to_rprime(F::mul(alpha, z.z3[m]));
  }
  return k;
}
// t = e1 + alpha (e2 - e3) + alpha^2 L1 (z (+) -1). la = alpha^2 L1 (M), la32 its times32() (T). (e2 - e3) alpha + z la32: D U + U T, below
// p^2 + 34 p^2 < p R', so r is in (-p, 2 p). Where the share takes the public -1, la is subtracted: e1 + r - la, three terms in (-2.1 p, 3.1 p).
template <class F>
CSH_HD F pq_t_elem(const F& e1, const F& e2, const F& e3, const F& z, const F& l1, const PqCombineK<F>& k, bool pub) {
  using LZ = typename LazyOf<F>::type;
  const LZ la = LZ::mul(LZ::unpack(l1), LZ::unpack(k.alpha2d));
  const LZ r = LZ::reduce(LZ::mul_add_wide(LZ::sub(LZ::unpack(e2), LZ::unpack(e3)), LZ::unpack(k.alphad), LZ::unpack(z), la.times32()));
  LZ s = LZ::add(LZ::unpack(e1), r);
  if (pub) s = LZ::sub(s, la);
  return s.canonical_wide().pack();
}
// tz = e1z + alpha (e2z - e3z) + alpha^2 L1 zp with X = X_0 + z1[m] X_1 + z2[m] X_2 + z3[m] X_3 (mul4vec_post). The differences
// D_k = e2z_k - e3z_k come first (class D), then D0 alpha + D1 (alpha z1) and D2 (alpha z2) + D3 (alpha z3): |sum| < 2 p^2, r1 and r2 in
// (-p / 16, p + p / 16). r3 = zp la32 is in (-p / 16, p + 34 p / 64). Three terms, normalized(), then e1z: below 5 p.
template <class F>
struct PqCombineLane {
  F az1d, az2d, az3d;  // alpha z_k[m] R' of the lane's m
};
template <class F>
CSH_HD F pq_tz_elem(const F& e1z, const F* x /* e2z_0..3 */, const F* y /* e3z_0..3 */, const F& zp, const F& l1, const PqCombineK<F>& k,
                    const PqCombineLane<F>& lk) {
  using LZ = typename LazyOf<F>::type;
  const LZ la32 = LZ::mul(LZ::unpack(l1), LZ::unpack(k.alpha2d)).times32();
  LZ d[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) d[j] = LZ::sub(LZ::unpack(x[j]), LZ::unpack(y[j]));
  const LZ r1 = LZ::reduce(LZ::mul_add_wide(d[0], LZ::unpack(k.alphad), d[1], LZ::unpack(lk.az1d)));
  const LZ r2 = LZ::reduce(LZ::mul_add_wide(d[2], LZ::unpack(lk.az2d), d[3], LZ::unpack(lk.az3d)));
  const LZ r3 = LZ::mul(LZ::unpack(zp), la32);
  return LZ::add(LZ::add(LZ::add(r1, r2), r3).normalized(), LZ::unpack(e1z)).canonical_wide().pack();
}

// (d) finish, round3.rs:468-498: column j of the coefficient form. Additions and subtractions only, in the 32-bit field (canonical in, canonical
// out). q_0 = -ct[j], q_k = q_(k-1) - ct[k n + j]; tf[k n + j] = q_k + ctz[k n + j].
template <class F>
struct PqFinishCol {
  F tf[4];
};
template <class F>
CSH_HD PqFinishCol<F> pq_finish_col(const F& ct0, const F& ct1, const F& ct2, const F& ct3, const F& z0, const F& z1, const F& z2, const F& z3) {
  PqFinishCol<F> o;
  F q = F::neg(ct0);
  o.tf[0] = F::add(q, z0);
  q = F::sub(q, ct1);
  o.tf[1] = F::add(q, z1);
  q = F::sub(q, ct2);
  o.tf[2] = F::add(q, z2);
  q = F::sub(q, ct3);
  o.tf[3] = F::add(q, z3);
  return o;
}

// ---- what one launch is told, how the host fills it in, and what a lane does with flat index e -----------------------------------------
// The kernels call pq_*_at() inside their grid-stride loops; the self-test calls the same functions index after index on host arrays.
CSH_HD int pq_pub_comp(uint32_t protocol, uint32_t party) { return protocol == 0 ? 0 : (party == 0 ? 0 : (party == 1 ? 1 : -1)); }
// a host share (ncomp elements) by component; the absent component of ncomp 1 is zero
template <class F>
inline void pq_share(F dst[2], const uint64_t* p, uint32_t ncomp) {
  dst[0] = fr_load<F>(p);
  dst[1] = ncomp == 2 ? fr_load<F>(p + 4) : F::zero();
}

struct PqGeom {
  size_t N;       // points of the extended domain (finish: 4 n)
  uint32_t ncomp;
  int pub_comp;   // the component that takes public values, -1 = none
  CSH_HD size_t values() const { return N * ncomp; }
  CSH_HD size_t point(size_t e) const { return ncomp == 1 ? e : e >> 1; }
  CSH_HD unsigned comp(size_t e) const { return (unsigned)(e & (size_t)(ncomp - 1)); }
  CSH_HD bool pub(size_t e) const { return (int)comp(e) == pub_comp; }
  CSH_HD unsigned m(size_t e) const { return (unsigned)(point(e) & 3); }
  CSH_HD size_t rot4(size_t e) const { return ((point(e) + 4) & (N - 1)) * ncomp + comp(e); }  // the value of point (i + 4) mod N
};

template <class F>
struct PqPowArgs {
  F gd;  // w R'
  F *hi, *lo;
  size_t n_hi;
};
template <class F>
CSH_HD void pq_pow_tables_at(const PqPowArgs<F>& a, size_t idx) {
  const size_t n_lo = size_t(1) << PQ_POW_LO_LOG;
  if (idx < n_lo) a.lo[idx] = pq_power_entry(a.gd, idx);
  else a.hi[idx - n_lo] = pq_power_entry(a.gd, (idx - n_lo) << PQ_POW_LO_LOG);
}

template <class F>
struct PqBlindArgs {
  PqBlindK<F> k;
  const F *hi, *lo;
  F* out[5];  // ap, bp, cp, zp, zwp
  PqGeom g;
};
template <class F>
inline void pq_blinders_consts(PqBlindArgs<F>& a, const F& gen, const uint64_t* blinders, uint32_t ncomp) {
  for (int j = 0; j < 9; ++j) pq_share(a.k.b[j], blinders + 4 * ncomp * j, ncomp);
  a.k.w4d = fr_to_rprime(F::pow_u64(gen, 4));
}
template <class F>
CSH_HD void pq_blinders_at(const PqBlindArgs<F>& a, int v, size_t e) {
  a.out[v][e] = pq_blinders_elem(a.k, v, a.g.comp(e), pq_pow(a.hi, a.lo, a.g.point(e)));
}

template <class F>
struct PqPiArgs {
  const F* lagrange[PQ_PI_CHUNK];
  F nbd[PQ_PI_CHUNK][2];  // (-buffer_a[j]) R' by component
  F* pi;
  int k, first;           // terms of this launch; first = start from zero, otherwise from what pi holds
  PqGeom g;
};
template <class F>
inline void pq_pi_consts(PqPiArgs<F>& a, const uint64_t* const* lagrange, const uint64_t* buffer_a, size_t j0, size_t n_public, uint32_t ncomp) {
  a.k = (int)(n_public - j0 < (size_t)PQ_PI_CHUNK ? n_public - j0 : (size_t)PQ_PI_CHUNK);
  a.first = j0 == 0;
  for (int j = 0; j < PQ_PI_CHUNK; ++j) {
    a.lagrange[j] = j < a.k ? (const F*)lagrange[j0 + j] : nullptr;
    a.nbd[j][0] = a.nbd[j][1] = F::zero();
    if (j < a.k) {
      F s[2];
      pq_share(s, buffer_a + 4 * ncomp * (j0 + j), ncomp);
      a.nbd[j][0] = fr_to_rprime(F::neg(s[0]));
      a.nbd[j][1] = fr_to_rprime(F::neg(s[1]));
    }
  }
}
template <class F>
CSH_HD void pq_pi_at(const PqPiArgs<F>& a, size_t e) {
  using LZ = typename LazyOf<F>::type;
  const size_t i = a.g.point(e);
  const bool c1 = a.g.comp(e) != 0;
  LZ acc = a.first ? LZ::zero() : LZ::unpack(a.pi[e]);
#pragma unroll 1
  for (int j = 0; j < a.k; ++j) acc = pq_pi_step(acc, LZ::unpack(a.lagrange[j][i]), LZ::unpack(pq_sel(c1, a.nbd[j][1], a.nbd[j][0])));
  a.pi[e] = acc.fold_top().canonical_narrow().pack();
}

template <class F>
struct PqE1Args {
  const F *a_b, *a, *b, *c, *pi, *a_bp, *ap_b, *ap_bp, *ap, *bp, *cp;  // shares
  const F *qm, *ql, *qr, *qo, *qc;                                   // public
  F *e1, *e1z;
  F z1d[4];  // z1[m] R'
  PqGeom g;
};
// m = i mod 4 is the same for every index of a lane's grid-stride loop (the stride is a multiple of 4 ncomp), so the kernels select the
// constants of m once per lane, before the loop, and the arguments need not stay in scalar registers
template <class F>
CSH_HD F pq_e1_lane(const PqE1Args<F>& a, size_t e) {
  return pq_sel4(a.z1d, a.g.m(e));
}
template <class F>
CSH_HD void pq_e1_at(const PqE1Args<F>& a, const F& z1d_m, size_t e) {
  const size_t i = a.g.point(e);
  const F qm = a.qm[i], ql = a.ql[i], qr = a.qr[i], qo = a.qo[i];
  a.e1[e] = pq_e1_elem(a.a_b[e], a.a[e], a.b[e], a.c[e], a.pi[e], qm, ql, qr, qo, a.qc[i], a.g.pub(e));
  a.e1z[e] = pq_e1z_elem(a.a_bp[e], a.ap_b[e], a.ap_bp[e], a.ap[e], a.bp[e], a.cp[e], qm, ql, qr, qo, z1d_m);
}

template <class F>
struct PqE2Args {
  const F* in[3];  // a, b, c
  F* out[3];       // e2a, e2b, e2c
  F bk[3];         // beta, beta k1, beta k2 (arkworks-Montgomery)
  F gamma;
  const F *hi, *lo;
  PqGeom g;
};
template <class F>
CSH_HD void pq_e2_at(const PqE2Args<F>& a, size_t e) {
  if (!a.g.pub(e)) {  // this component takes no public value: e2x = x
#pragma unroll
    for (int v = 0; v < 3; ++v) a.out[v][e] = a.in[v][e];
    return;
  }
  const auto w = pq_pow(a.hi, a.lo, a.g.point(e));
#pragma unroll
  for (int v = 0; v < 3; ++v) a.out[v][e] = pq_e2_elem(a.in[v][e], w, a.bk[v], a.gamma);
}

template <class F>
struct PqE3Args {
  const F* in[3];  // a, b, c
  const F* s[3];   // s1, s2, s3
  F* out[3];       // e3a, e3b, e3c
  const F* z;
  F* e3d;
  F betad, gamma;  // beta R'; gamma
  PqGeom g;
};
template <class F>
CSH_HD void pq_e3_at(const PqE3Args<F>& a, size_t e) {
  a.e3d[e] = a.z[a.g.rot4(e)];
  const bool pub = a.g.pub(e);
  const size_t i = a.g.point(e);
#pragma unroll
  for (int v = 0; v < 3; ++v) a.out[v][e] = pub ? pq_e3_elem(a.in[v][e], a.s[v][i], a.betad, a.gamma) : a.in[v][e];
}

template <class F>
struct PqCombineArgs {
  const F *e1, *e1z, *z, *zp, *e2, *e3, *l1;
  const F *e2z[4], *e3z[4];
  F *t, *tz;
  PqCombineK<F> k;
  PqGeom g;
};
template <class F>
CSH_HD PqCombineLane<F> pq_combine_lane(const PqCombineArgs<F>& a, size_t e) {
  const unsigned m = a.g.m(e);
  return PqCombineLane<F>{pq_sel4(a.k.az1d, m), pq_sel4(a.k.az2d, m), pq_sel4(a.k.az3d, m)};
}
template <class F>
CSH_HD void pq_combine_at(const PqCombineArgs<F>& a, const PqCombineLane<F>& lk, size_t e) {
  const size_t i = a.g.point(e);
  const F l1 = a.l1[i];
  a.t[e] = pq_t_elem(a.e1[e], a.e2[e], a.e3[e], a.z[e], l1, a.k, a.g.pub(e));
  F x[4], y[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) x[j] = a.e2z[j][e], y[j] = a.e3z[j][e];
  a.tz[e] = pq_tz_elem(a.e1z[e], x, y, a.zp[e], l1, a.k, lk);
}

template <class F>
struct PqFinishArgs {
  const F *ct, *ctz;
  F *t1, *t2, *t3;  // n + 1, n + 1, n + 6 shares
  F b9[2], b10[2];
  size_t n;
  uint32_t ncomp;
};
// flat index e over n ncomp: column j = e / ncomp, component c. t3's last six shares are columns 0..5 of the fourth chunk; the rest of that
// chunk is what the reference drops.
template <class F>
CSH_HD void pq_finish_at(const PqFinishArgs<F>& a, size_t e) {
  const size_t nv = a.n * a.ncomp, j = a.ncomp == 1 ? e : e >> 1;
  const bool c1 = (e & (size_t)(a.ncomp - 1)) != 0;
  const PqFinishCol<F> o = pq_finish_col(a.ct[e], a.ct[nv + e], a.ct[2 * nv + e], a.ct[3 * nv + e], a.ctz[e], a.ctz[nv + e], a.ctz[2 * nv + e],
                                         a.ctz[3 * nv + e]);
  const F b9 = pq_sel(c1, a.b9[1], a.b9[0]), b10 = pq_sel(c1, a.b10[1], a.b10[0]);
  a.t1[e] = o.tf[0];
  a.t2[e] = j == 0 ? F::sub(o.tf[1], b9) : o.tf[1];
  a.t3[e] = j == 0 ? F::sub(o.tf[2], b10) : o.tf[2];
  if (j < 6) a.t3[nv + e] = o.tf[3];
  if (j == 0) {
    a.t1[nv + e] = b9;
    a.t2[nv + e] = b10;
  }
}

// ---- the power tables on the device: the kernel and its launcher, for every unit that needs w^i (plonk_quot.hip, plonk_rounds.hip) ------
#if defined(__HIPCC__)
template <class F>
__global__ __launch_bounds__(PQ_WG) void k_pq_pow_tables(PqPowArgs<F> a) {
  const size_t total = a.n_hi + (size_t(1) << PQ_POW_LO_LOG);
  for (size_t i = blockIdx.x * (size_t)PQ_WG + threadIdx.x; i < total; i += (size_t)gridDim.x * PQ_WG) pq_pow_tables_at(a, i);
}
// the two-level power table of the domain's generator, in the stream's workspace (valid for work queued on `st` until the next call that
// takes workspace on it)
template <class F>
inline int pq_power_tables(const F& gen, size_t N, hipStream_t st, const F** hi, const F** lo) {
  PqPowArgs<F> a;
  a.gd = fr_to_rprime(gen);
  a.n_hi = pq_pow_hi_count(N);
  const size_t n_lo = size_t(1) << PQ_POW_LO_LOG;
  Arena& ar = arena_for(st);
  CSH_TRY(ar.reserve(Arena::padded(a.n_hi * sizeof(F)) + Arena::padded(n_lo * sizeof(F))));
  a.hi = ar.take<F>(a.n_hi);
  a.lo = ar.take<F>(n_lo);
  hipLaunchKernelGGL(k_pq_pow_tables<F>, dim3(fr_stream_grid(a.n_hi + n_lo, PQ_WG)), dim3(PQ_WG), 0, st, a);
  *hi = a.hi;
  *lo = a.lo;
  return CSH_OK;
}
#endif

}  // namespace csh
