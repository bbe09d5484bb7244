// Call sites of the MSM / NTT / share-vector kernels in the reference's other two provers, mirrored
// above the C ABI with the reference's method names and argument meaning:
//   CircomPlonkProver::{local_mul_vec, fft, ifft, msm_public_points_g1}      co-circom/co-plonk/src/mpc.rs:56-166,
//       impls co-plonk/src/mpc/{plain.rs:60-185, rep3.rs:60-175, shamir.rs}, Domains (co-plonk/src/types.rs:70-109)
//   NoirUltraHonkProver::{local_mul_vec, msm_public_points, fft, ifft}        co-noir/co-noir-common/src/mpc/mod.rs:236-379,
//       impls mpc/{plain.rs:271, rep3.rs:258-288, shamir.rs:255}, HonkCurve::fast_msm (honk_curve.rs:35, 81-83, 175-177)
//   CircomPlonkProver::{evaluate_poly_public, inv_vec, array_prod_mul (plain driver)}   co-plonk/src/mpc.rs, round2.rs:164-165, round4.rs:126-132
//   NoirUltraHonkProver::{eval_poly, inv_many_in_place, inv_many_in_place_leaking_zeros}  co-noir-common/src/mpc/rep3.rs:208-257, rep3/poly.rs:39-68
//   Polynomial / SharedPolynomial::factor_roots, compute_batched_quotient, Round5::div_by_zerofier(.., 1, beta)
//       co-noir-common/src/polynomials/polynomial.rs:183, shared_polynomial.rs:92-140, co_shplemini_prover.rs:661-737, co-plonk/src/round5.rs:78-91
//   partially_evaluate_init / partially_evaluate_inplace, compute_fold_polynomials, Polynomial / SharedPolynomial::evaluate_mle
//       co_sumcheck_prover.rs:34-98, co_shplemini_prover.rs:236-312, polynomial.rs:270-312, shared_polynomial.rs:154-199 (csh_mle_fold / csh_mle_fold_rounds)
//   Round2::compute_z, Round5::compute_r + compute_wxi, compute_wxiw for the plain driver
//       co-plonk/src/round2.rs:104-190, round5.rs:118-278 (csh_plonk_z_operands / csh_vec_rotate_right / csh_plonk_blind_coefficients / csh_poly_lincomb)
// These data-parallel methods are mirrored, the whole-vector scans among them (running product, batch inverse, polynomial
// evaluation, division by (X - z): csh_vec_prefix_prod / csh_vec_batch_inverse / csh_eval_poly / csh_poly_div_linear). The PLONK rounds / sumcheck / relations above them are
// control logic and stay in the Rust host (SURVEY.md 8 "out of scope"). NOT mirrored: the Rep3 / Shamir array_prod_mul
// (co-plonk/src/mpc/rep3.rs:187-260), which is four network multiplication rounds around the same running product -- its opened
// vector would go through csh_vec_prefix_prod exactly as the plain driver's does below.
#pragma once
#include <array>
#include <memory>

#include "groth16.hpp"

namespace cosnarks {

// ark_poly::Radix2EvaluationDomain<F> as the provers use it: size = a power of two, group_gen either arkworks' default
// or overwritten with the snarkjs root (co-plonk/src/types.rs:92-99). fft / ifft are natural -> natural, the input is
// zero-padded to the domain size (EvaluationDomain::fft semantics), ifft scales by 1/n.
template <class P>
struct EvaluationDomain {
  csh_domain_t dom = nullptr;
  size_t size = 0;
  uint32_t log_size = 0;
  EvaluationDomain() = default;
  EvaluationDomain(const EvaluationDomain&) = delete;
  EvaluationDomain& operator=(const EvaluationDomain&) = delete;
  EvaluationDomain(EvaluationDomain&& o) noexcept : dom(o.dom), size(o.size), log_size(o.log_size) { o.dom = nullptr; }
  EvaluationDomain& operator=(EvaluationDomain&& o) noexcept {
    if (this != &o) {
      if (dom) csh_domain_free(dom);
      dom = o.dom;
      size = o.size;
      log_size = o.log_size;
      o.dom = nullptr;
    }
    return *this;
  }
  ~EvaluationDomain() {
    if (dom) csh_domain_free(dom);
  }
  // Radix2EvaluationDomain::new(n): smallest power of two >= n, arkworks root
  static EvaluationDomain arkworks(size_t n) { return make(n, nullptr); }
  // ... with group_gen := snarkjs roots_of_unity[log2 size] (types.rs:92-99)
  static EvaluationDomain snarkjs(size_t n) {
    size_t s = 1;
    uint32_t lg = 0;
    while (s < n) {
      s <<= 1;
      ++lg;
    }
    typename P::Fr gen, shift;
    groth16_roots_of_unity<typename P::Fr>(lg, gen, shift);
    return make(n, (const uint64_t*)&gen);
  }

 private:
  static EvaluationDomain make(size_t n, const uint64_t* gen) {
    EvaluationDomain d;
    d.size = 1;
    while (d.size < n) {
      d.size <<= 1;
      ++d.log_size;
    }
    const int rc = csh_domain_create(P::ID, d.log_size, gen, &d.dom);
    if (rc == CSH_ERR_DOMAIN) throw Error("PolynomialDegreeTooLarge");
    check(rc, "csh_domain_create");
    return d;
  }
};

// co-plonk/src/types.rs:36-109: the two domains of a PLONK proof (n and 4n, snarkjs roots)
template <class P>
struct PlonkDomains {
  EvaluationDomain<P> domain, extended_domain;
  explicit PlonkDomains(size_t domain_size) {
    if (domain_size == 0 || (domain_size & (domain_size - 1))) throw Error("InvalidDomainSize");
    domain = EvaluationDomain<P>::snarkjs(domain_size);
    extended_domain = EvaluationDomain<P>::snarkjs(domain_size * 4);
  }
};

namespace detail {
template <class P, class Share>
inline std::vector<Share> transform(const std::vector<Share>& data, const EvaluationDomain<P>& d, bool inverse) {
  if (data.size() > d.size) throw Error("fft: input longer than the domain");
  std::vector<Share> v(d.size);  // value-initialised: zero padding
  std::copy(data.begin(), data.end(), v.begin());
  constexpr uint32_t ncomp = sizeof(Share) / sizeof(typename P::Fr);
  check(inverse ? csh_ifft(d.dom, (uint64_t*)v.data(), ncomp) : csh_fft(d.dom, (uint64_t*)v.data(), ncomp), inverse ? "csh_ifft" : "csh_fft");
  return v;
}
// taceo_ark_algebra::msm::msm_unchecked on host slices: the shorter of the two lengths (honk_curve.rs:33-35)
template <class F>
inline Proj<F> msm_unchecked(csh_curve_t curve, csh_group_t group, const std::vector<AffineT<F>>& points, const void* scalars_mont, size_t n) {
  const size_t cnt = n < points.size() ? n : points.size();
  if (cnt == 0) return Proj<F>::inf();
  csh_bases_t h = nullptr;
  check(csh_bases_upload(curve, group, points.data(), cnt, 0, &h), "csh_bases_upload");
  csh::Jac<F> out;
  const int rc = csh_msm(h, 0, cnt, reinterpret_cast<const uint64_t*>(scalars_mont), 1, &out);
  csh_bases_free(h);
  check(rc, "csh_msm");
  if (out.is_inf()) return Proj<F>::inf();
  return Proj<F>::from_affine(AffineT<F>{out.x, out.y});
}
// sum_i coeffs[i] point^i on every component of the share type (poly::eval_poly, rep3/poly.rs:39-68; DensePolynomial::evaluate)
template <class P, class Share>
inline Share eval_poly(const std::vector<Share>& coeffs, const typename P::Fr& point) {
  constexpr uint32_t ncomp = sizeof(Share) / sizeof(typename P::Fr);
  Share out{};
  check(csh_eval_poly(P::ID, (const uint64_t*)coeffs.data(), coeffs.size(), ncomp, (const uint64_t*)&point, (uint64_t*)&out), "csh_eval_poly");
  return out;
}
// p(X) / (X - root) in place, the popped last element dropped as the reference drops it (Polynomial::factor_roots, polynomial.rs:183;
// SharedPolynomial::factor_roots, shared_polynomial.rs:92-140: linear, so every component of a share alike). root == 0: remove(0).
template <class P, class Share>
inline void factor_roots(std::vector<Share>& coeffs, const typename P::Fr& root) {
  if (coeffs.empty()) throw Error("factor_roots: empty polynomial");
  if (root.is_zero()) {
    coeffs.erase(coeffs.begin());
    return;
  }
  constexpr uint32_t ncomp = sizeof(Share) / sizeof(typename P::Fr);
  uint64_t* v = (uint64_t*)coeffs.data();
  check(csh_poly_div_linear(P::ID, v, coeffs.size(), ncomp, (const uint64_t*)&root, nullptr, v, nullptr), "csh_poly_div_linear");
  coeffs.pop_back();
}
// Round5::div_by_zerofier (co-plonk/src/round5.rs:78-91): the same recurrence with c = -beta^-1; the reference calls it with n = 1 only
template <class P, class Share>
inline void div_by_zerofier(std::vector<Share>& inout, size_t n, const typename P::Fr& beta) {
  if (n != 1) throw Error("div_by_zerofier: only n = 1 (X - beta) is built");
  if (beta.is_zero()) throw Error("Highly unlikely to be zero");
  factor_roots<P, Share>(inout, beta);
}
struct DeviceMem {  // csh_malloc / csh_free
  void* p = nullptr;
  explicit DeviceMem(size_t bytes) { check(csh_malloc(&p, bytes ? bytes : 1), "csh_malloc"); }
  DeviceMem(const DeviceMem&) = delete;
  DeviceMem& operator=(const DeviceMem&) = delete;
  ~DeviceMem() { csh_free(p); }
};
// y[i] <- y[i]^-1 with ONE field inversion (zeros stay zero); returns how many zeros there were
template <class P>
inline size_t batch_inverse(std::vector<typename P::Fr>& y) {
  size_t zeros = 0;
  check(csh_vec_batch_inverse(P::ID, (const uint64_t*)y.data(), (uint64_t*)y.data(), y.size(), &zeros), "csh_vec_batch_inverse");
  return zeros;
}
// The shared tail of every MPC inversion (rep3/arithmetic.rs:233-246, shamir/arithmetic.rs:157-172, co-noir-common rep3.rs:216-257):
// y = open(a r) is public; the result is r y^-1 -- one batch inverse on y, one table multiplication on the shares of r. A zero makes
// the strict forms fail with the reference's message; the leaking form leaves the default (all-zero) share there, which r * 0 is.
template <class P, class Share>
inline std::vector<Share> unmask_inverse(std::vector<Share> r, std::vector<typename P::Fr> y, const char* zero_message) {
  const size_t zeros = batch_inverse<P>(y);
  if (zeros && zero_message) throw Error(zero_message);
  constexpr uint32_t ncomp = sizeof(Share) / sizeof(typename P::Fr);
  check(csh_vec_mul_table(P::ID, (uint64_t*)r.data(), (const uint64_t*)y.data(), r.size(), ncomp), "csh_vec_mul_table");
  return r;
}
// ---- multilinear folds (csh_mle_fold / csh_mle_fold_rounds): out[j] = in[2j] + u (in[2j+1] - in[2j]) on every component of the share type ----
// multiplication of every component of a share by a public value (T::mul_with_public), host arithmetic on single elements
template <class P, class Share>
inline Share mul_with_public(const typename P::Fr& k, Share s) {
  using Fr = typename P::Fr;
  Fr* c = reinterpret_cast<Fr*>(&s);
  for (size_t i = 0; i < sizeof(Share) / sizeof(Fr); ++i) c[i] = Fr::mul(c[i], k);
  return s;
}
// PartiallyEvaluatePolys as the sumcheck rounds use it (partially_evaluate_init / partially_evaluate_inplace,
// co_sumcheck_prover.rs:34-98, sumcheck_prover.rs:20-60): every polynomial, public and shared, stays on the device in two buffers that swap
// roles each round -- a fold in place would be a race between workgroups -- and one csh_mle_fold_dev call per share width folds them all.
// All buffers of the set are cut from ONE device allocation. round_size must be a power of two (the prover's is 2^log_n): every length on
// the way down is then even, which csh_mle_fold requires; the reference's limit % 2 branch for an odd length is NOT mirrored, such a
// round_size is refused here. The reference's "truncate, then push a zero if shorter than 2" rule is applied here, on the host side:
// the length is kept here, and the pushed zero is one element written behind the single one that is left.
template <class P, class Share>
class PartiallyEvaluatePolys {
  using Fr = typename P::Fr;
  struct Poly {
    size_t off[2];  // byte offsets of the two buffers in mem_
    uint32_t ncomp;
  };
  std::vector<Poly> polys_;  // the public ones first
  std::unique_ptr<DeviceMem> mem_;
  size_t n_public_ = 0, len_ = 0;
  int cur_ = 0;
  char* at(const Poly& q, int which) const { return (char*)mem_->p + q.off[which]; }
  void fold(size_t n, const Fr& u) {
    for (uint32_t ncomp = 1; ncomp <= 2; ++ncomp) {
      std::vector<const uint64_t*> in;
      std::vector<uint64_t*> out;
      for (const Poly& q : polys_)
        if (q.ncomp == ncomp) {
          in.push_back((const uint64_t*)at(q, cur_));
          out.push_back((uint64_t*)at(q, cur_ ^ 1));
        }
      if (!in.empty()) check(csh_mle_fold_dev(P::ID, in.data(), out.data(), in.size(), n, ncomp, (const uint64_t*)&u, nullptr), "csh_mle_fold_dev");
    }
    cur_ ^= 1;
    len_ = n / 2;
    if (len_ < 2) {  // poly.push(zero)
      check(csh_sync(nullptr), "csh_sync");
      const Fr zero[2] = {Fr::zero(), Fr::zero()};
      for (const Poly& q : polys_) check(csh_memcpy_h2d(at(q, cur_) + sizeof(Fr) * q.ncomp * len_, zero, sizeof(Fr) * q.ncomp), "csh_memcpy_h2d");
      len_ = 2;
    }
  }
  template <class E>
  std::vector<E> get(size_t i) const {
    std::vector<E> v(len_);
    check(csh_memcpy_d2h(v.data(), at(polys_[i], cur_), sizeof(E) * len_), "csh_memcpy_d2h");
    return v;
  }

 public:
  // partially_evaluate_init: the first round_size entries of every polynomial folded by the first round challenge
  PartiallyEvaluatePolys(const std::vector<std::vector<Fr>>& pub, const std::vector<std::vector<Share>>& shared, size_t round_size, const Fr& u) {
    if (round_size < 2 || (round_size & (round_size - 1))) throw Error("partially_evaluate: round_size must be a power of two, at least 2");
    for (const auto& v : pub)
      if (v.size() < round_size) throw Error("partially_evaluate: polynomial shorter than round_size");
    for (const auto& v : shared)
      if (v.size() < round_size) throw Error("partially_evaluate: polynomial shorter than round_size");
    const size_t half = round_size / 2 < 2 ? 2 : round_size / 2;
    size_t total = 0;
    auto place = [&](uint32_t ncomp) {
      Poly q;
      q.ncomp = ncomp;
      q.off[0] = total;
      total += (sizeof(Fr) * ncomp * round_size + 255) & ~size_t(255);
      q.off[1] = total;
      total += (sizeof(Fr) * ncomp * half + 255) & ~size_t(255);
      polys_.push_back(q);
    };
    for (size_t i = 0; i < pub.size(); ++i) place(1);
    for (size_t i = 0; i < shared.size(); ++i) place(sizeof(Share) / sizeof(Fr));
    n_public_ = pub.size();
    mem_.reset(new DeviceMem(total));
    for (size_t i = 0; i < pub.size(); ++i) check(csh_memcpy_h2d(at(polys_[i], 0), pub[i].data(), sizeof(Fr) * round_size), "csh_memcpy_h2d");
    for (size_t i = 0; i < shared.size(); ++i)
      check(csh_memcpy_h2d(at(polys_[n_public_ + i], 0), shared[i].data(), sizeof(Share) * round_size), "csh_memcpy_h2d");
    fold(round_size, u);
  }
  // partially_evaluate_inplace: every polynomial folded by the round challenge, truncated, a zero pushed if one element is left
  void partially_evaluate_inplace(const Fr& u) { fold(len_, u); }
  size_t len() const { return len_; }
  std::vector<Fr> public_poly(size_t i) const { return get<Fr>(i); }
  std::vector<Share> shared_poly(size_t i) const { return get<Share>(n_public_ + i); }
};
// compute_fold_polynomials (co_shplemini_prover.rs:236-312, shplemini_prover.rs:198): the list the reference returns -- A_1 .. A_(log_n-1),
// then the constant folds of the virtual rounds. ONE csh_mle_fold_rounds call with m = log_n keeps every level; its last level is
// final_eval, and the constant folds, the ZK zero factor included, are host arithmetic on that one value.
template <class P, class Share>
inline std::vector<std::vector<Share>> compute_fold_polynomials(size_t log_n, const std::vector<typename P::Fr>& multilinear_challenge,
                                                                const std::vector<Share>& a_0, bool has_zk) {
  using Fr = typename P::Fr;
  constexpr uint32_t ncomp = sizeof(Share) / sizeof(Fr);
  const size_t n = size_t(1) << log_n, virtual_log_n = multilinear_challenge.size();
  if (log_n < 2 || virtual_log_n < log_n || a_0.size() < n) throw Error("compute_fold_polynomials: needs log_n >= 2, log_n challenges and 2^log_n coefficients");
  std::vector<Share> levels(n - 1);
  Share final_eval{};
  check(csh_mle_fold_rounds(P::ID, (const uint64_t*)a_0.data(), n, ncomp, (const uint64_t*)multilinear_challenge.data(), log_n,
                            (uint64_t*)levels.data(), (uint64_t*)&final_eval),
        "csh_mle_fold_rounds");
  std::vector<std::vector<Share>> fold_polynomials;
  fold_polynomials.reserve(virtual_log_n);
  for (size_t l = 1; l < log_n; ++l) fold_polynomials.emplace_back(levels.begin() + (n - (n >> (l - 1))), levels.begin() + (n - (n >> l)));
  const Fr indicator = has_zk ? Fr::zero() : Fr::one();
  fold_polynomials.push_back({mul_with_public<P, Share>(indicator, final_eval)});
  Fr tail = Fr::one();
  for (size_t k = log_n; k + 1 < virtual_log_n; ++k) {
    tail = Fr::mul(tail, Fr::sub(Fr::one(), multilinear_challenge[k]));  // multiply by (1 - u_k)
    fold_polynomials.push_back({mul_with_public<P, Share>(indicator, mul_with_public<P, Share>(tail, final_eval))});
  }
  return fold_polynomials;
}
// Polynomial::evaluate_mle / SharedPolynomial::evaluate_mle (polynomial.rs:270-312, shared_polynomial.rs:154-199): 2^dim coefficients,
// dim <= the number of points; all dim rounds in one csh_mle_fold_rounds call that hands back the last level only, the (1 - u) factors
// of the trivial dimensions on the host. (The reference asserts dim == the number of points, which leaves its own trivial-dimension loop
// idle; the loop is mirrored as written.)
template <class P, class Share>
inline Share evaluate_mle(const std::vector<Share>& coefficients, const std::vector<typename P::Fr>& evaluation_points) {
  using Fr = typename P::Fr;
  constexpr uint32_t ncomp = sizeof(Share) / sizeof(Fr);
  if (coefficients.empty()) return Share{};
  size_t dim = 0;
  while ((size_t(1) << dim) < coefficients.size()) ++dim;
  if (dim == 0 || coefficients.size() != size_t(1) << dim || dim > evaluation_points.size())
    throw Error("evaluate_mle: needs 2^dim coefficients, 1 <= dim <= the number of evaluation points");
  Share result{};
  check(csh_mle_fold_rounds(P::ID, (const uint64_t*)coefficients.data(), coefficients.size(), ncomp, (const uint64_t*)evaluation_points.data(), dim,
                            nullptr, (uint64_t*)&result),
        "csh_mle_fold_rounds");
  for (size_t k = dim; k < evaluation_points.size(); ++k) result = mul_with_public<P, Share>(Fr::sub(Fr::one(), evaluation_points[k]), result);
  return result;
}
}  // namespace detail

// ShpleminiOpeningClaim as compute_batched_quotient reads it: f_j(X), the point x_j and (the share of) the evaluation v_j
template <class Fr, class Share>
struct OpeningClaim {
  std::vector<Share> polynomial;
  Fr challenge;
  Share evaluation;
};
// Q(X) = sum_j nu^j (f_j(X) - v_j) / (X - x_j) (compute_batched_quotient, co_shplemini_prover.rs:661-737; shplemini_prover.rs:594):
// every claim polynomial goes up once, its quotient is accumulated into the device-resident Q as it is formed (q.add_scaled(&tmp, &nu)
// without tmp), and Q comes back once. As long as the longest polynomial, like the reference's new_zero(max_poly_size).
template <class P, class Share>
inline std::vector<Share> shplonk_batched_quotient(const std::vector<OpeningClaim<typename P::Fr, Share>>& claims, const typename P::Fr& nu) {
  using Fr = typename P::Fr;
  constexpr uint32_t ncomp = sizeof(Share) / sizeof(Fr);
  size_t max_poly_size = 0;
  for (const auto& c : claims) max_poly_size = std::max(max_poly_size, c.polynomial.size());
  std::vector<Share> q(max_poly_size);  // value-initialised: zero
  if (max_poly_size == 0) return q;
  const size_t bytes = sizeof(Share) * max_poly_size;
  detail::DeviceMem dq(bytes), df(bytes);
  check(csh_memcpy_h2d(dq.p, q.data(), bytes), "csh_memcpy_h2d");
  Fr current_nu = Fr::one();
  for (const auto& c : claims) {
    if (c.challenge.is_zero()) throw Error("shplonk_batched_quotient: opening point 0");
    check(csh_sync(nullptr), "csh_sync");  // the previous claim's kernels are done with df
    check(csh_memcpy_h2d(df.p, c.polynomial.data(), sizeof(Share) * c.polynomial.size()), "csh_memcpy_h2d");
    check(csh_poly_div_linear_dev(P::ID, (const uint64_t*)df.p, c.polynomial.size(), ncomp, (const uint64_t*)&c.challenge,
                                  (const uint64_t*)&c.evaluation, (const uint64_t*)&current_nu, 1, (uint64_t*)dq.p, nullptr, nullptr),
          "csh_poly_div_linear_dev");
    current_nu = Fr::mul(current_nu, nu);
  }
  check(csh_memcpy_d2h(q.data(), dq.p, bytes), "csh_memcpy_d2h");
  return q;
}

template <class F>
struct Rep3PointShare {  // mpc-core/src/protocols/rep3/pointshare/types.rs:5-11
  Proj<F> a, b;
};

// A curve as the MSM entry points see it: BN254 / BLS12-381 G1 for PLONK and UltraHonk commitments, Grumpkin for the
// HonkCurve impl over the cycle curve.
template <class P>
struct G1Of {
  using Fr = typename P::Fr;
  using Fq = typename P::Fq;
  static constexpr csh_curve_t CURVE = P::ID;
  static constexpr csh_curve_t FIELD_OF = P::ID;
};
struct GrumpkinCurve {  // scalars live in BN254 Fq, coordinates in BN254 Fr
  using Fr = csh::Bn254Fq;
  using Fq = csh::Bn254Fr;
  static constexpr csh_curve_t CURVE = CSH_GRUMPKIN;
};

// HonkCurve::fast_msm (honk_curve.rs:35): msm_unchecked(bases, scalars)
template <class C>
inline Proj<typename C::Fq> fast_msm(const std::vector<AffineT<typename C::Fq>>& bases, const std::vector<typename C::Fr>& scalars) {
  return detail::msm_unchecked<typename C::Fq>(C::CURVE, CSH_G1, bases, scalars.data(), scalars.size());
}

// What Round3::compute_t (co-plonk/src/round3.rs:246-253) reads: of the zkey the 4 n evaluations of the selector, permutation and Lagrange
// polynomials and k1, k2; of Round2Polys the 4 n evaluations of a, b, c, z and buffer_a; of the challenges b[0..11), beta, gamma, alpha.
template <class Fr>
struct PlonkQuotientZkey {
  size_t domain_size = 0;
  std::vector<Fr> qm, ql, qr, qo, qc, s1, s2, s3;  // 4 n evaluations each
  std::vector<std::vector<Fr>> lagrange;           // n_public >= 1 vectors of 4 n evaluations
  Fr k1, k2;
};
template <class Fr, class Share>
struct PlonkQuotientInputs {
  std::vector<Share> a, b, c, z;  // poly_eval_*.eval, polys.z.eval: 4 n each
  std::vector<Share> buffer_a;    // n_public
  Share blinders[11];
  Fr beta, gamma, alpha;
};
// What Round2::compute_z (co-plonk/src/round2.rs:104-190) reads: the three wire buffers, of the zkey the 4 n evaluations of S1, S2, S3 and
// k1, k2, the challenges beta and gamma, and the blinders b7, b8, b9 in the order blind_coefficients takes them.
template <class Fr>
struct PlonkRound2Inputs {
  std::vector<Fr> buffer_a, buffer_b, buffer_c;  // n each
  std::vector<Fr> s1, s2, s3;                    // 4 n evaluations each
  Fr beta, gamma, k1, k2;
  Fr blinders[3];
};
template <class Fr>
struct PlonkPolyEval {  // types.rs PolyEval: n + k blinded coefficients, the 4 n evaluations of the unblinded polynomial
  std::vector<Fr> poly, eval;
};
// What Round5::compute_r + compute_wxi (round5.rs:118-259) read: the blinded polynomials of rounds 1-3, of the zkey the n coefficients of
// the selector and permutation polynomials and k1, k2, the public inputs, the round-4 evaluations and every challenge so far.
template <class Fr>
struct PlonkRound5Inputs {
  size_t domain_size = 0;
  std::vector<Fr> z, t1, t2, t3, a, b, c;          // n + 3, n + 1, n + 1, n + 6, n + 2, n + 2, n + 2 coefficients
  std::vector<Fr> qm, ql, qr, qo, qc, s1, s2, s3;  // n coefficients each
  std::vector<Fr> public_inputs;
  Fr eval_a, eval_b, eval_c, eval_s1, eval_s2, eval_zw;
  Fr beta, gamma, alpha, xi, v[5], k1, k2;
};

namespace detail {
// Round3::compute_t for the plain driver, device-resident from the upload to t1, t2, t3: the four stages of csh_plonk_quot_* with the
// reference's mul_vec rounds (round3.rs:283-295, and the two mul4vec! of 423-428) as csh_vec_mul_dev / csh_vec_add_dev between them and
// the two iffts (468, 480) as csh_ifft_dev. Nothing comes back to the host in between; every call is on the thread's stream.
template <class P>
inline std::array<std::vector<typename P::Fr>, 3> plain_compute_t(const PlonkDomains<P>& domains, const PlonkQuotientZkey<typename P::Fr>& zkey,
                                                                  const PlonkQuotientInputs<typename P::Fr, typename P::Fr>& in) {
  using Fr = typename P::Fr;
  const size_t n = zkey.domain_size, N = 4 * n, n_public = zkey.lagrange.size();
  if (n < 8 || (n & (n - 1)) || domains.extended_domain.size != N) throw Error("compute_t: domain_size must be a power of two >= 8 with its 4 n domain");
  if (n_public == 0 || in.buffer_a.size() != n_public) throw Error("compute_t: needs L_1 and one buffer_a share per Lagrange polynomial");
  const std::vector<Fr>* evals[] = {&in.a, &in.b, &in.c, &in.z, &zkey.qm, &zkey.ql, &zkey.qr, &zkey.qo, &zkey.qc, &zkey.s1, &zkey.s2, &zkey.s3};
  for (const auto* v : evals)
    if (v->size() != N) throw Error("compute_t: every evaluation vector has 4 n elements");
  for (const auto& l : zkey.lagrange)
    if (l.size() != N) throw Error("compute_t: every evaluation vector has 4 n elements");
  const csh_domain_t dom = domains.extended_domain.dom;
  std::vector<std::unique_ptr<DeviceMem>> pool;  // freed together at the end: nothing is released while the stream still works
  auto fresh = [&](size_t count = 0) {
    pool.emplace_back(new DeviceMem(sizeof(Fr) * (count ? count : N)));
    return (uint64_t*)pool.back()->p;
  };
  auto up = [&](const std::vector<Fr>& v) {
    uint64_t* d = fresh();
    check(csh_memcpy_h2d(d, v.data(), sizeof(Fr) * N), "csh_memcpy_h2d");
    return d;
  };
  auto mul = [&](const uint64_t* x, const uint64_t* y) {  // PlainPlonkDriver::mul_vec
    uint64_t* o = fresh();
    check(csh_vec_mul_dev(P::ID, x, y, o, N, nullptr), "csh_vec_mul_dev");
    return o;
  };
  auto add_mul = [&](const uint64_t* acc, const uint64_t* x, const uint64_t* y) {  // add_mul_vec
    uint64_t* o = fresh();
    check(csh_vec_add_dev(P::ID, acc, mul(x, y), o, N, 1, nullptr), "csh_vec_add_dev");
    return o;
  };
  const uint64_t *a = up(in.a), *b = up(in.b), *c = up(in.c), *z = up(in.z);
  const uint64_t* pub[8] = {up(zkey.qm), up(zkey.ql), up(zkey.qr), up(zkey.qo), up(zkey.qc), up(zkey.s1), up(zkey.s2), up(zkey.s3)};
  std::vector<const uint64_t*> lagrange;
  for (const auto& l : zkey.lagrange) lagrange.push_back(up(l));
  // (a)
  uint64_t* bl[5];
  for (auto& o : bl) o = fresh();
  check(csh_plonk_quot_blinders_dev(dom, 0, 0, (const uint64_t*)in.blinders, bl, nullptr), "csh_plonk_quot_blinders_dev");
  const uint64_t *ap = bl[0], *bp = bl[1], *cp = bl[2], *zp = bl[3], *zwp = bl[4];
  // round3.rs:283-295
  const uint64_t *a_b = mul(a, b), *a_bp = mul(a, bp), *ap_b = mul(b, ap), *ap_bp = mul(ap, bp);
  // (b)
  const uint64_t* sh[11] = {a, b, c, z, a_b, a_bp, ap_b, ap_bp, ap, bp, cp};
  uint64_t* op[10];
  for (auto& o : op) o = fresh();
  const Fr challenges[4] = {in.beta, in.gamma, zkey.k1, zkey.k2};
  check(csh_plonk_quot_operands_dev(dom, 0, 0, sh, pub, lagrange.data(), n_public, (const uint64_t*)in.buffer_a.data(), (const uint64_t*)challenges, op,
                                    nullptr),
        "csh_plonk_quot_operands_dev");
  // mul4vec! (round3.rs:20-86) -> r, a0, a1, a2, a3
  auto mul4vec = [&](const uint64_t* xa, const uint64_t* xb, const uint64_t* xc, const uint64_t* xd, const uint64_t* xdp, const uint64_t* r[5]) {
    const uint64_t *m_a_b = mul(xa, xb), *m_a_bp = mul(xa, bp), *m_ap_b = mul(ap, xb), *m_ap_bp = mul(ap, bp);
    const uint64_t *c_d = mul(xc, xd), *c_dp = mul(xc, xdp), *cp_d = mul(cp, xd), *cp_dp = mul(cp, xdp);
    r[0] = mul(m_a_b, c_d);
    r[1] = add_mul(add_mul(add_mul(mul(m_ap_b, c_d), m_a_bp, c_d), m_a_b, cp_d), m_a_b, c_dp);
    r[2] = add_mul(add_mul(add_mul(add_mul(add_mul(mul(m_ap_bp, c_d), m_ap_b, cp_d), m_ap_b, c_dp), m_a_bp, cp_d), m_a_bp, c_dp), m_a_b, cp_dp);
    r[3] = add_mul(add_mul(add_mul(mul(m_a_bp, cp_dp), m_ap_b, cp_dp), m_ap_bp, c_dp), m_ap_bp, cp_d);
    r[4] = mul(m_ap_bp, cp_dp);
  };
  const uint64_t *e2[5], *e3[5];
  mul4vec(op[3], op[4], op[5], z, zp, e2);        // e2a, e2b, e2c, e2d = z, dp = zp
  mul4vec(op[6], op[7], op[8], op[9], zwp, e3);   // e3a, e3b, e3c, e3d, dp = zwp
  // (c)
  const uint64_t* cs[14] = {op[1], op[2], z, zp, e2[0], e2[1], e2[2], e2[3], e2[4], e3[0], e3[1], e3[2], e3[3], e3[4]};
  uint64_t* tt[2] = {fresh(), fresh()};
  check(csh_plonk_quot_combine_dev(dom, 0, 0, cs, lagrange[0], (const uint64_t*)&in.alpha, tt, nullptr), "csh_plonk_quot_combine_dev");
  check(csh_ifft_dev(dom, tt[0], 1, nullptr), "csh_ifft_dev");
  check(csh_ifft_dev(dom, tt[1], 1, nullptr), "csh_ifft_dev");
  // (d)
  uint64_t *t1 = fresh(n + 1), *t2 = fresh(n + 1), *t3 = fresh(n + 6);
  check(csh_plonk_quot_finish_dev(P::ID, n, 0, 0, tt[0], tt[1], (const uint64_t*)&in.blinders[9], t1, t2, t3, nullptr), "csh_plonk_quot_finish_dev");
  std::array<std::vector<Fr>, 3> out = {std::vector<Fr>(n + 1), std::vector<Fr>(n + 1), std::vector<Fr>(n + 6)};
  check(csh_memcpy_d2h(out[0].data(), t1, sizeof(Fr) * (n + 1)), "csh_memcpy_d2h");
  check(csh_memcpy_d2h(out[1].data(), t2, sizeof(Fr) * (n + 1)), "csh_memcpy_d2h");
  check(csh_memcpy_d2h(out[2].data(), t3, sizeof(Fr) * (n + 6)), "csh_memcpy_d2h");
  return out;
}

// device buffers of one driver call, freed together at its end: nothing is released while the stream still works
struct DevicePool {
  std::vector<std::unique_ptr<DeviceMem>> mem;
  uint64_t* fresh(size_t bytes) {
    mem.emplace_back(new DeviceMem(bytes));
    return (uint64_t*)mem.back()->p;
  }
  template <class Fr>
  uint64_t* up(const std::vector<Fr>& v) {
    uint64_t* d = fresh(sizeof(Fr) * v.size());
    if (!v.empty()) check(csh_memcpy_h2d(d, v.data(), sizeof(Fr) * v.size()), "csh_memcpy_h2d");
    return d;
  }
};

// Round2::compute_z for the plain driver (round2.rs:104-190 with the array_prod_mul of co-plonk/src/mpc/plain.rs:195-247), device-resident
// from the upload of the wire buffers to the blinded polynomial and its 4 n evaluations: csh_plonk_z_operands_dev, the two triple products
// as csh_vec_mul_dev, their running products (csh_vec_prefix_prod_dev), the denominators' inverses (csh_vec_batch_inverse_dev), the last
// product, rotate_right(1) straight into the polynomial's buffer, ifft over n, a zero-padded copy with fft over 4 n, and the blinding.
// Nothing comes back to the host in between; every call is on the thread's stream.
template <class P>
inline PlonkPolyEval<typename P::Fr> plain_compute_z(const PlonkDomains<P>& domains, const PlonkRound2Inputs<typename P::Fr>& in) {
  using Fr = typename P::Fr;
  const size_t n = domains.domain.size, N = 4 * n;
  if (n < 8 || domains.extended_domain.size != N) throw Error("compute_z: domain_size must be a power of two >= 8 with its 4 n domain");
  for (const auto* v : {&in.buffer_a, &in.buffer_b, &in.buffer_c})
    if (v->size() != n) throw Error("compute_z: every wire buffer has n elements");
  for (const auto* v : {&in.s1, &in.s2, &in.s3})
    if (v->size() != N) throw Error("compute_z: every permutation polynomial has 4 n evaluations");
  DevicePool pool;
  auto fresh = [&](size_t count) { return pool.fresh(sizeof(Fr) * count); };
  auto mul = [&](const uint64_t* x, const uint64_t* y) {  // PlainPlonkDriver::mul_vec
    uint64_t* o = fresh(n);
    check(csh_vec_mul_dev(P::ID, x, y, o, n, nullptr), "csh_vec_mul_dev");
    return o;
  };
  const uint64_t* sh[3] = {pool.up(in.buffer_a), pool.up(in.buffer_b), pool.up(in.buffer_c)};
  const uint64_t* sigma[3] = {pool.up(in.s1), pool.up(in.s2), pool.up(in.s3)};
  uint64_t* op[6];
  for (auto& o : op) o = fresh(n);
  const Fr challenges[4] = {in.beta, in.gamma, in.k1, in.k2};
  check(csh_plonk_z_operands_dev(domains.extended_domain.dom, 0, 0, sh, sigma, (const uint64_t*)challenges, op, nullptr), "csh_plonk_z_operands_dev");
  // array_prod_mul: the running products of n1 n2 n3 and of d1 d2 d3, the latter inverted
  uint64_t *num = mul(mul(op[0], op[1]), op[2]), *den = mul(mul(op[3], op[4]), op[5]);
  uint64_t* zeros = pool.fresh(sizeof(uint64_t));
  check(csh_vec_prefix_prod_dev(P::ID, num, num, n, nullptr), "csh_vec_prefix_prod_dev");
  check(csh_vec_prefix_prod_dev(P::ID, den, den, n, nullptr), "csh_vec_prefix_prod_dev");
  check(csh_vec_batch_inverse_dev(P::ID, den, den, n, zeros, nullptr), "csh_vec_batch_inverse_dev");
  // buffer_z = (num * den).rotate_right(1) (round2.rs:166-171), written where the polynomial's first n coefficients will stand
  uint64_t *poly = fresh(n + 3), *eval = fresh(N);
  check(csh_vec_rotate_right_dev(P::ID, mul(num, den), poly, n, 1, 1, nullptr), "csh_vec_rotate_right_dev");
  check(csh_ifft_dev(domains.domain.dom, poly, 1, nullptr), "csh_ifft_dev");
  const uint64_t* coeffs[1] = {poly};
  const Fr one = Fr::one();
  check(csh_poly_lincomb_dev(P::ID, 0, 0, coeffs, &n, (const uint64_t*)&one, 1, nullptr, nullptr, nullptr, 0, nullptr, eval, N, nullptr), "csh_poly_lincomb_dev");
  check(csh_fft_dev(domains.extended_domain.dom, eval, 1, nullptr), "csh_fft_dev");
  check(csh_plonk_blind_coefficients_dev(P::ID, poly, n, 1, (const uint64_t*)in.blinders, 3, nullptr), "csh_plonk_blind_coefficients_dev");
  PlonkPolyEval<Fr> out{std::vector<Fr>(n + 3), std::vector<Fr>(N)};
  uint64_t zero_count = 0;
  check(csh_memcpy_d2h(out.poly.data(), poly, sizeof(Fr) * (n + 3)), "csh_memcpy_d2h");
  check(csh_memcpy_d2h(out.eval.data(), eval, sizeof(Fr) * N), "csh_memcpy_d2h");
  check(csh_memcpy_d2h(&zero_count, zeros, sizeof zero_count), "csh_memcpy_d2h");
  if (zero_count) throw Error("Cannot invert zero");
  return out;
}

// The scalar part of Round5::compute_r (round5.rs:118-190): calculate_lagrange_evaluations, calculate_pi, e2, e3, e4, r0 -- O(n_public +
// log n) host arithmetic -- as the coefficients of the one linear combination: cs for z, t1, t2, t3, a, b, c; cp for qm, ql, qr, qo, qc,
// s3, s1, s2; const0 for coefficient 0. xiw = xi w is compute_wxiw's root.
template <class Fr>
struct PlonkRound5Scalars {
  Fr cs[7], cp[8], const0, xiw;
};
template <class P>
inline PlonkRound5Scalars<typename P::Fr> round5_scalars(const PlonkRound5Inputs<typename P::Fr>& in) {
  using Fr = typename P::Fr;
  const size_t n = in.domain_size;
  if (n == 0 || (n & (n - 1))) throw Error("InvalidDomainSize");
  uint32_t lg = 0;
  while ((size_t(1) << lg) < n) ++lg;
  Fr w, shift;
  groth16_roots_of_unity<Fr>(lg, w, shift);
  auto neg = [](const Fr& x) { return Fr::sub(Fr::zero(), x); };
  Fr xin = in.xi;
  for (uint32_t i = 0; i < lg; ++i) xin = Fr::mul(xin, xin);
  const Fr zh = Fr::sub(xin, Fr::one()), nf = Fr::from_u64(n);
  // L_i(xi) = w^i zh / (n (xi - w^i)); pi = -sum L_i(xi) public_i
  Fr wi = Fr::one(), l1 = Fr::zero(), pi = Fr::zero();
  const size_t n_lagrange = in.public_inputs.empty() ? 1 : in.public_inputs.size();
  for (size_t i = 0; i < n_lagrange; ++i) {
    const Fr li = Fr::mul(Fr::mul(wi, zh), Fr::inv(Fr::mul(nf, Fr::sub(in.xi, wi))));
    if (i == 0) l1 = li;
    if (i < in.public_inputs.size()) pi = Fr::sub(pi, Fr::mul(li, in.public_inputs[i]));
    wi = Fr::mul(wi, w);
  }
  const Fr betaxi = Fr::mul(in.beta, in.xi);
  auto plus_gamma = [&](const Fr& e, const Fr& x) { return Fr::add(Fr::add(e, x), in.gamma); };
  const Fr e2 = Fr::mul(Fr::mul(Fr::mul(plus_gamma(in.eval_a, betaxi), plus_gamma(in.eval_b, Fr::mul(betaxi, in.k1))),
                                plus_gamma(in.eval_c, Fr::mul(betaxi, in.k2))), in.alpha);
  const Fr e3 = Fr::mul(Fr::mul(Fr::mul(plus_gamma(in.eval_a, Fr::mul(in.beta, in.eval_s1)), plus_gamma(in.eval_b, Fr::mul(in.beta, in.eval_s2))),
                                in.eval_zw), in.alpha);
  const Fr e4 = Fr::mul(Fr::mul(in.alpha, in.alpha), l1);
  const Fr r0 = Fr::sub(Fr::sub(pi, Fr::mul(e3, Fr::add(in.eval_c, in.gamma))), e4);
  PlonkRound5Scalars<Fr> s;
  const Fr mzh = neg(zh);
  const Fr cs[7] = {Fr::add(e2, e4), mzh, Fr::mul(mzh, xin), Fr::mul(Fr::mul(mzh, xin), xin), in.v[0], in.v[1], in.v[2]};
  const Fr cp[8] = {Fr::mul(in.eval_a, in.eval_b), in.eval_a, in.eval_b, in.eval_c, Fr::one(), neg(Fr::mul(e3, in.beta)), in.v[3], in.v[4]};
  std::copy(cs, cs + 7, s.cs);
  std::copy(cp, cp + 8, s.cp);
  const Fr evs[5] = {in.eval_a, in.eval_b, in.eval_c, in.eval_s1, in.eval_s2};
  s.const0 = r0;
  for (int j = 0; j < 5; ++j) s.const0 = Fr::sub(s.const0, Fr::mul(in.v[j], evs[j]));
  s.xiw = Fr::mul(in.xi, w);
  return s;
}
// Round5::compute_r + compute_wxi (round5.rs:118-259) for the plain driver: ONE csh_poly_lincomb_dev over the seven shared and eight
// public polynomials with const0 on coefficient 0, then div_by_zerofier(.., 1, xi) in place as csh_poly_div_linear_dev. -> W_xi, n + 5
// coefficients (the popped remainder dropped as the reference drops it).
template <class P>
inline std::vector<typename P::Fr> plain_compute_r_wxi(const PlonkRound5Inputs<typename P::Fr>& in) {
  using Fr = typename P::Fr;
  if (in.xi.is_zero()) throw Error("Highly unlikely to be zero");
  const PlonkRound5Scalars<Fr> s = round5_scalars<P>(in);
  const size_t out_len = in.domain_size + 6;
  const std::vector<Fr>* shares[7] = {&in.z, &in.t1, &in.t2, &in.t3, &in.a, &in.b, &in.c};
  const std::vector<Fr>* publics[8] = {&in.qm, &in.ql, &in.qr, &in.qo, &in.qc, &in.s3, &in.s1, &in.s2};
  DevicePool pool;
  const uint64_t *sp[7], *pp[8];
  size_t sl[7], pl[8];
  for (int j = 0; j < 7; ++j) sp[j] = pool.up(*shares[j]), sl[j] = shares[j]->size();
  for (int j = 0; j < 8; ++j) pp[j] = pool.up(*publics[j]), pl[j] = publics[j]->size();
  uint64_t* r = pool.fresh(sizeof(Fr) * out_len);
  check(csh_poly_lincomb_dev(P::ID, 0, 0, sp, sl, (const uint64_t*)s.cs, 7, pp, pl, (const uint64_t*)s.cp, 8, (const uint64_t*)&s.const0, r, out_len, nullptr),
        "csh_poly_lincomb_dev");
  check(csh_poly_div_linear_dev(P::ID, r, out_len, 1, (const uint64_t*)&in.xi, nullptr, nullptr, 0, r, nullptr, nullptr), "csh_poly_div_linear_dev");
  std::vector<Fr> wxi(out_len - 1);
  check(csh_memcpy_d2h(wxi.data(), r, sizeof(Fr) * wxi.size()), "csh_memcpy_d2h");
  return wxi;
}
// Round5::compute_wxiw (round5.rs:262-278): (z(X) - eval_zw) / (X - xi w), the subtraction on coefficient 0 as the division loads it
template <class P>
inline std::vector<typename P::Fr> plain_compute_wxiw(const PlonkRound5Inputs<typename P::Fr>& in) {
  using Fr = typename P::Fr;
  if (in.z.size() < 2) throw Error("compute_wxiw: z has fewer than two coefficients");
  const Fr xiw = round5_scalars<P>(in).xiw;
  if (xiw.is_zero()) throw Error("Highly unlikely to be zero");
  DevicePool pool;
  uint64_t* z = pool.up(in.z);
  check(csh_poly_div_linear_dev(P::ID, z, in.z.size(), 1, (const uint64_t*)&xiw, (const uint64_t*)&in.eval_zw, nullptr, 0, z, nullptr, nullptr),
        "csh_poly_div_linear_dev");
  std::vector<Fr> wxiw(in.z.size() - 1);
  check(csh_memcpy_d2h(wxiw.data(), z, sizeof(Fr) * wxiw.size()), "csh_memcpy_d2h");
  return wxiw;
}
}  // namespace detail

// What the whole-trace loops of the Oink prover read (co-noir/co-ultrahonk/src/co_oink/co_oink_prover.rs:98-504; plain twin
// co-noir/ultrahonk/src/oink/oink_prover.rs): of the proving key the witness and precomputed polynomials (circuit_size elements each;
// w_4 may be shorter, :133-137 resize it), the memory-record rows, final_active_wire_idx and the active ranges (empty: none); of the
// transcript eta_1..3, beta, gamma.
template <class Fr>
struct HonkOinkInputs {
  size_t circuit_size = 0, final_active_wire_idx = 0;
  std::vector<std::pair<size_t, size_t>> active_ranges;
  std::vector<Fr> w_l, w_r, w_o, w_4, lookup_read_tags;
  std::vector<Fr> q_r, q_m, q_c, q_o, table_1, table_2, table_3, table_4, q_lookup;
  std::vector<Fr> id[4], sigma[4];
  std::vector<uint32_t> memory_read_records, memory_write_records;
  std::vector<std::pair<uint32_t, Fr>> memory_records_shared;  // (row, type share)
  Fr eta_1, eta_2, eta_3, beta, gamma;
};

namespace detail {
inline std::vector<size_t> honk_flat_ranges(const std::vector<std::pair<size_t, size_t>>& ranges) {
  std::vector<size_t> flat;
  for (const auto& r : ranges) flat.push_back(r.first), flat.push_back(r.second);
  return flat;
}
// add_ram_rom_memory_records_to_wire_4 (co_oink_prover.rs:119-160) for the plain driver, device-resident from the upload to memory.w_4:
// the clone + resize of :133-137 as csh_poly_lincomb_dev (one share term, coefficient one, out_len = n), then csh_honk_w4_records_dev.
// The contract of that entry -- every row below n, no row twice -- is checked here, where the lists are uploaded.
template <class P>
inline std::vector<typename P::Fr> plain_compute_w4(const HonkOinkInputs<typename P::Fr>& in) {
  using Fr = typename P::Fr;
  const size_t n = in.circuit_size;
  if (n == 0 || in.w_l.size() != n || in.w_r.size() != n || in.w_o.size() != n || in.w_4.size() > n) throw Error("compute_w4: w_l, w_r, w_o have circuit_size elements, w_4 at most");
  std::vector<uint32_t> shared_rows;
  std::vector<Fr> type_shares;
  for (const auto& r : in.memory_records_shared) shared_rows.push_back(r.first), type_shares.push_back(r.second);
  std::vector<bool> seen(n, false);
  const std::vector<uint32_t>* lists[3] = {&in.memory_read_records, &in.memory_write_records, &shared_rows};
  for (const auto* list : lists)
    for (uint32_t row : *list) {
      if (row >= n || seen[row]) throw Error("compute_w4: a memory record is outside the trace or occurs twice");
      seen[row] = true;
    }
  DevicePool pool;
  const uint64_t* w[3] = {pool.up(in.w_l), pool.up(in.w_r), pool.up(in.w_o)};
  const uint64_t* src[1] = {pool.up(in.w_4)};
  const size_t len = in.w_4.size();
  const Fr one = Fr::one();
  uint64_t* w4 = pool.fresh(sizeof(Fr) * n);
  check(csh_poly_lincomb_dev(P::ID, 0, 0, src, &len, (const uint64_t*)&one, 1, nullptr, nullptr, nullptr, 0, nullptr, w4, n, nullptr), "csh_poly_lincomb_dev");
  const Fr etas[3] = {in.eta_1, in.eta_2, in.eta_3};
  check(csh_honk_w4_records_dev(P::ID, 0, 0, w, w4, n, (const uint64_t*)etas, (const uint32_t*)pool.up(in.memory_read_records), in.memory_read_records.size(),
                                (const uint32_t*)pool.up(in.memory_write_records), in.memory_write_records.size(), (const uint32_t*)pool.up(shared_rows),
                                pool.up(type_shares), shared_rows.size(), nullptr),
        "csh_honk_w4_records_dev");
  std::vector<Fr> out(n);
  check(csh_memcpy_d2h(out.data(), w4, sizeof(Fr) * n), "csh_memcpy_d2h");
  return out;
}
// compute_logderivative_inverses (co_oink_prover.rs:229-293) for the plain driver, device-resident from the upload to lookup_inverses:
// csh_honk_lookup_operands_dev, the mul_many of :278 as csh_vec_mul_dev, batch_invert_leaking_zeros as csh_vec_batch_inverse_dev (a zero
// stays zero). This is the co-prover's selector form, (1 - q_lookup) tag + q_lookup times the product; the plain prover
// (oink_prover.rs) instead skips a row unless q_lookup or the tag is one, which is the same when both are 0 or 1.
template <class P>
inline std::vector<typename P::Fr> plain_compute_logderivative_inverses(const HonkOinkInputs<typename P::Fr>& in) {
  using Fr = typename P::Fr;
  const size_t n = in.circuit_size;
  const std::vector<Fr>* shares[4] = {&in.w_l, &in.w_r, &in.w_o, &in.lookup_read_tags};
  const std::vector<Fr>* publics[9] = {&in.q_r, &in.q_m, &in.q_c, &in.q_o, &in.table_1, &in.table_2, &in.table_3, &in.table_4, &in.q_lookup};
  DevicePool pool;
  const uint64_t *sp[4], *pp[9];
  for (int j = 0; j < 4; ++j) {
    if (n == 0 || shares[j]->size() != n) throw Error("compute_logderivative_inverses: every polynomial has circuit_size elements");
    sp[j] = pool.up(*shares[j]);
  }
  for (int j = 0; j < 9; ++j) {
    if (publics[j]->size() != n) throw Error("compute_logderivative_inverses: every polynomial has circuit_size elements");
    pp[j] = pool.up(*publics[j]);
  }
  uint64_t* op[2] = {pool.fresh(sizeof(Fr) * n), pool.fresh(sizeof(Fr) * n)};
  const Fr challenges[2] = {in.beta, in.gamma};
  check(csh_honk_lookup_operands_dev(P::ID, 0, 0, sp, pp, n, (const uint64_t*)challenges, op, nullptr), "csh_honk_lookup_operands_dev");
  uint64_t* inv = pool.fresh(sizeof(Fr) * n);
  check(csh_vec_mul_dev(P::ID, op[0], op[1], inv, n, nullptr), "csh_vec_mul_dev");
  check(csh_vec_batch_inverse_dev(P::ID, inv, inv, n, nullptr, nullptr), "csh_vec_batch_inverse_dev");
  std::vector<Fr> out(n);
  check(csh_memcpy_d2h(out.data(), inv, sizeof(Fr) * n), "csh_memcpy_d2h");
  return out;
}
// compute_grand_product (co_oink_prover.rs:382-507) for the plain driver, device-resident from the upload to z_perm:
// csh_honk_perm_operands_dev, the products of the four numerators and of the four denominators as csh_vec_mul_dev, their running
// products (array_prod_mul: csh_vec_prefix_prod_dev), the denominators' inverses (batch_invert: csh_vec_batch_inverse_dev), the last
// product and csh_honk_z_perm_place_dev. w_4 is memory.w_4, what compute_w4 returned.
template <class P>
inline std::vector<typename P::Fr> plain_compute_grand_product(const HonkOinkInputs<typename P::Fr>& in, const std::vector<typename P::Fr>& w_4) {
  using Fr = typename P::Fr;
  const size_t n = in.circuit_size, domain_size = in.final_active_wire_idx + 1;
  const std::vector<Fr>* shares[4] = {&in.w_l, &in.w_r, &in.w_o, &w_4};
  DevicePool pool;
  const uint64_t *sp[4], *pp[8];
  for (int j = 0; j < 4; ++j) {
    if (n < 2 || shares[j]->size() != n || in.id[j].size() != n || in.sigma[j].size() != n) throw Error("compute_grand_product: every polynomial has circuit_size >= 2 elements");
    sp[j] = pool.up(*shares[j]), pp[j] = pool.up(in.id[j]), pp[4 + j] = pool.up(in.sigma[j]);
  }
  const std::vector<size_t> ranges = honk_flat_ranges(in.active_ranges);
  size_t active = domain_size;
  if (!in.active_ranges.empty()) {
    active = 0;
    for (const auto& r : in.active_ranges) active += r.second > r.first ? r.second - r.first : 0;
  }
  if (active == 0 || active > n) throw Error("compute_grand_product: the active domain must have 1 .. circuit_size indices");
  const size_t m = active - 1, mm = m ? m : 1;
  uint64_t* op[8];
  for (auto& o : op) o = pool.fresh(sizeof(Fr) * mm);
  const Fr challenges[2] = {in.beta, in.gamma};
  check(csh_honk_perm_operands_dev(P::ID, 0, 0, sp, pp, n, domain_size, ranges.data(), in.active_ranges.size(), (const uint64_t*)challenges, op, nullptr),
        "csh_honk_perm_operands_dev");
  auto mul = [&](const uint64_t* x, const uint64_t* y) {  // mul_many
    uint64_t* o = pool.fresh(sizeof(Fr) * mm);
    check(csh_vec_mul_dev(P::ID, x, y, o, m, nullptr), "csh_vec_mul_dev");
    return o;
  };
  uint64_t *quot = nullptr, *zeros = pool.fresh(sizeof(uint64_t));
  if (m) {  // a one-row active domain has no quotient: z_perm is zeros and the one
    uint64_t *num = mul(mul(op[0], op[1]), mul(op[2], op[3])), *den = mul(mul(op[4], op[5]), mul(op[6], op[7]));
    check(csh_vec_prefix_prod_dev(P::ID, num, num, m, nullptr), "csh_vec_prefix_prod_dev");
    check(csh_vec_prefix_prod_dev(P::ID, den, den, m, nullptr), "csh_vec_prefix_prod_dev");
    check(csh_vec_batch_inverse_dev(P::ID, den, den, m, zeros, nullptr), "csh_vec_batch_inverse_dev");
    quot = mul(num, den);
  }
  uint64_t* z = pool.fresh(sizeof(Fr) * n);
  check(csh_honk_z_perm_place_dev(P::ID, 0, 0, quot, z, n, domain_size, ranges.data(), in.active_ranges.size(), nullptr), "csh_honk_z_perm_place_dev");
  std::vector<Fr> out(n);
  uint64_t zero_count = 0;
  check(csh_memcpy_d2h(out.data(), z, sizeof(Fr) * n), "csh_memcpy_d2h");
  if (m) check(csh_memcpy_d2h(&zero_count, zeros, sizeof zero_count), "csh_memcpy_d2h");
  if (zero_count) throw Error("Cannot invert zero");
  return out;
}
}  // namespace detail

// What a sumcheck round of the plain UltraHonk prover reads between two folds (co-noir/ultrahonk/src/decider/sumcheck/
// sumcheck_round_prover.rs:224-255): the 36 columns of subrelations 0 .. 10 in the order of csh_honk_sumcheck_accumulate_dev (witness
// w_l, w_r, w_o, w_4, z_perm, lookup_inverses, lookup_read_counts, lookup_read_tags; shifted w_l, w_r, w_o, w_4, z_perm; precomputed q_m,
// q_c, q_l, q_r, q_o, q_4, q_arith, q_delta_range, q_lookup, sigma_1..4, id_1..4, table_1..4, lagrange_first, lagrange_last), the relation
// parameters, and the state of GateSeparatorPolynomial (decider/types.rs:44-112).
constexpr size_t HONK_SUMCHECK_COLUMNS = 36, HONK_ACC_ELEMS = 57, HONK_SUBRELATIONS = 11, HONK_BATCHED_RELATION_PARTIAL_LENGTH = 8;
constexpr size_t HONK_ACC_LENGTHS[HONK_SUBRELATIONS] = {6, 5, 6, 3, 5, 5, 3, 6, 6, 6, 6};
template <class Fr>
struct HonkRelationParameters {
  Fr beta, gamma, public_input_delta;
};
template <class Fr>
struct HonkGateSeparator {
  std::vector<Fr> betas;
  size_t log_num_monomials = 0;  // beta_products has 2^log_num_monomials elements
  Fr partial_evaluation_result = Fr::one();
  size_t current_element_idx = 0, periodicity = 2;
  void partially_evaluate(const Fr& u) {  // types.rs:96-102
    partial_evaluation_result = Fr::mul(partial_evaluation_result, Fr::add(Fr::one(), Fr::mul(u, Fr::sub(betas[current_element_idx], Fr::one()))));
    ++current_element_idx;
    periodicity *= 2;
  }
};
template <class Fr>
using HonkAccumulators = std::array<Fr, HONK_ACC_ELEMS>;  // the eleven accumulators back to back, HONK_ACC_LENGTHS

// The other five relations of the round (elliptic, memory, non-native field, Poseidon2 external and internal: subrelations 11 .. 27 of
// relations/mod.rs:134-145): the 19 columns in the order of csh_honk_sumcheck_accumulate_gates_dev (w_l, w_r, w_o, w_4; shifted w_l, w_r,
// w_o, w_4; q_m, q_c, q_l, q_r, q_o, q_4; q_elliptic, q_memory, q_nnf, q_poseidon2_external, q_poseidon2_internal), their eight parameters
// and their seventeen accumulators. With the first eleven these are the 28 of accumulate_relation_univariates
// (sumcheck_round_prover.rs:160-222), batched with NUM_ALPHAS = 27 challenges.
constexpr size_t HONK_GATES_COLUMNS = 19, HONK_GATES_ACC_ELEMS = 110, HONK_GATES_SUBRELATIONS = 17, HONK_NUM_ALPHAS = 27;
constexpr size_t HONK_GATES_ACC_LENGTHS[HONK_GATES_SUBRELATIONS] = {6, 6, 6, 6, 6, 6, 6, 6, 6, 7, 7, 7, 7, 7, 7, 7, 7};
template <class Fr>
struct HonkGateParameters {
  Fr eta_1, eta_2, eta_3;
  Fr curve_b;                               // HonkCurve::get_curve_b of the embedded curve
  std::array<Fr, 4> mat_internal_diag_m_1;  // of the Poseidon2 internal matrix
};
template <class Fr>
using HonkGateAccumulators = std::array<Fr, HONK_GATES_ACC_ELEMS>;  // the seventeen accumulators back to back, HONK_GATES_ACC_LENGTHS

namespace detail {
// what both entries of the round ask of their columns, range and gate separator; `who` = the caller's name, `ncols` = 36 or 19
template <class Fr>
inline void honk_check_round(const char* who, size_t ncols, const std::vector<std::vector<Fr>>& cols, size_t edge_begin, size_t edge_end,
                             const HonkGateSeparator<Fr>* gs) {
  const std::string w = std::string(who) + ": ";
  if (cols.size() != ncols) throw Error(w + std::to_string(ncols) + " columns");
  if ((edge_begin & 1) || (edge_end & 1) || edge_begin >= edge_end) throw Error(w + "an even, non-empty range");
  for (const auto& c : cols)
    if (c.size() < edge_end) throw Error(w + "a column is shorter than the range");
  if (gs && (gs->log_num_monomials > 28 || gs->betas.size() < gs->log_num_monomials || ((edge_end >> 1) - 1) * gs->periodicity >= (size_t(1) << gs->log_num_monomials)))
    throw Error(w + "the gate separator's table is shorter than the range reads");
}
// The loop of compute_univariate_inner (:239-252) on the device, for either entry of the round (`entry`, `entry_name`): the columns go up,
// beta_products is made there (csh_honk_pow_table_dev), the entry runs, its ACC elements come back. gs == nullptr: the factor one
// (compute_virtual_contribution, :388-421).
template <class P, size_t ACC, class Entry, size_t NP>
inline std::array<typename P::Fr, ACC> plain_round_device(const char* who, Entry entry, const char* entry_name, size_t ncols,
                                                          const std::vector<std::vector<typename P::Fr>>& cols, size_t edge_begin, size_t edge_end,
                                                          const HonkGateSeparator<typename P::Fr>* gs, const typename P::Fr (&pr)[NP]) {
  using Fr = typename P::Fr;
  honk_check_round(who, ncols, cols, edge_begin, edge_end, gs);
  DevicePool pool;
  std::vector<const uint64_t*> dc(ncols);
  for (size_t c = 0; c < ncols; ++c) dc[c] = pool.up(cols[c]);
  uint64_t* table = nullptr;
  if (gs) {
    table = pool.fresh(sizeof(Fr) << gs->log_num_monomials);
    check(csh_honk_pow_table_dev(P::ID, (const uint64_t*)gs->betas.data(), gs->log_num_monomials, table, nullptr), "csh_honk_pow_table_dev");
  }
  uint64_t* acc = pool.fresh(sizeof(Fr) * ACC);
  check(entry(P::ID, dc.data(), edge_begin, edge_end, table, gs ? gs->periodicity : 1, (const uint64_t*)pr, acc, nullptr), entry_name);
  std::array<Fr, ACC> out;
  check(csh_memcpy_d2h(out.data(), acc, sizeof(Fr) * ACC), "csh_memcpy_d2h");
  return out;
}
template <class P>
inline HonkAccumulators<typename P::Fr> plain_round_accumulators(const std::vector<std::vector<typename P::Fr>>& cols, size_t edge_begin, size_t edge_end,
                                                                 const HonkGateSeparator<typename P::Fr>* gs, const HonkRelationParameters<typename P::Fr>& params) {
  const typename P::Fr pr[3] = {params.beta, params.gamma, params.public_input_delta};
  return plain_round_device<P, HONK_ACC_ELEMS>("compute_round_accumulators", csh_honk_sumcheck_accumulate_dev, "csh_honk_sumcheck_accumulate_dev",
                                               HONK_SUMCHECK_COLUMNS, cols, edge_begin, edge_end, gs, pr);
}
template <class Fr>
inline std::vector<Fr> honk_beta_products(const std::vector<Fr>& betas, size_t log_num_monomials) {  // types.rs:53-67
  std::vector<Fr> out(size_t(1) << log_num_monomials, Fr::one());
  for (size_t i = 0; i < log_num_monomials; ++i) {
    const size_t index = size_t(1) << i;
    out[index] = betas[i];
    for (size_t j = 1; j < index; ++j) out[index + j] = Fr::mul(out[j], betas[i]);
  }
  return out;
}
// The same loop in plain C++ on one host thread, the relations in the scalar shape of verify_accumulate at each of the points 0 .. 5: what
// the mirror test holds the device against, and the host column of tools/honk_sumcheck_probe.py.
template <class Fr>
inline HonkAccumulators<Fr> host_round_accumulators(const std::vector<std::vector<Fr>>& cols, size_t edge_begin, size_t edge_end, const HonkGateSeparator<Fr>* gs,
                                                    const HonkRelationParameters<Fr>& params) {
  honk_check_round("compute_round_accumulators", HONK_SUMCHECK_COLUMNS, cols, edge_begin, edge_end, gs);
  const std::vector<Fr> table = gs ? honk_beta_products(gs->betas, gs->log_num_monomials) : std::vector<Fr>();
  const Fr one = Fr::one(), two = Fr::add(one, one), three = Fr::add(two, one), neg_half = Fr::sub(Fr::zero(), Fr::inv(two));
  const Fr beta = params.beta, gamma = params.gamma;
  Fr acc[HONK_SUBRELATIONS][6];
  for (auto& a : acc)
    for (auto& x : a) x = Fr::zero();
  auto both_zero = [&](size_t c, size_t e) { return cols[c][e].is_zero() && cols[c][e + 1].is_zero(); };
  for (size_t e = edge_begin; e < edge_end; e += 2) {
    const Fr sf = gs ? table[(e >> 1) * gs->periodicity] : one;
    const bool do_arith = !both_zero(19, e), do_delta = !both_zero(20, e), do_lookup = !(both_zero(21, e) && both_zero(6, e));
    const bool do_perm = !(cols[4][e] == cols[12][e] && cols[4][e + 1] == cols[12][e + 1]);
    Fr v[HONK_SUMCHECK_COLUMNS], delta[HONK_SUMCHECK_COLUMNS];
    for (size_t c = 0; c < HONK_SUMCHECK_COLUMNS; ++c) v[c] = cols[c][e], delta[c] = Fr::sub(cols[c][e + 1], cols[c][e]);
    for (int k = 0; k < 6; ++k) {
      if (k)
        for (size_t c = 0; c < HONK_SUMCHECK_COLUMNS; ++c) v[c] = Fr::add(v[c], delta[c]);  // extend_from of two points
      auto add = [&](int s, const Fr& x) { acc[s][k] = Fr::add(acc[s][k], x); };
      const Fr &w_l = v[0], &w_r = v[1], &w_o = v[2], &w_4 = v[3], &z = v[4], &inv = v[5], &counts = v[6], &tag = v[7];
      const Fr &w_ls = v[8], &w_rs = v[9], &w_os = v[10], &w_4s = v[11], &zs = v[12];
      const Fr &q_m = v[13], &q_c = v[14], &q_l = v[15], &q_r = v[16], &q_o = v[17], &q_4 = v[18], &qa = v[19], &q_delta = v[20], &q_lookup = v[21];
      if (do_arith) {
        Fr t = Fr::mul(Fr::mul(Fr::sub(qa, three), Fr::mul(Fr::mul(q_m, w_r), w_l)), neg_half);
        t = Fr::add(t, Fr::add(Fr::add(Fr::mul(q_l, w_l), Fr::mul(q_r, w_r)), Fr::add(Fr::mul(q_o, w_o), Fr::add(Fr::mul(q_4, w_4), q_c))));
        t = Fr::add(t, Fr::mul(Fr::sub(qa, one), w_4s));
        add(0, Fr::mul(Fr::mul(t, qa), sf));
        Fr u = Fr::add(Fr::sub(Fr::add(w_l, w_4), w_ls), q_m);
        u = Fr::mul(Fr::mul(Fr::mul(u, Fr::sub(qa, two)), Fr::sub(qa, one)), qa);
        add(1, Fr::mul(u, sf));
      }
      if (do_perm) {
        Fr num = sf, den = sf;
        for (int j = 0; j < 4; ++j) {
          const Fr wg = Fr::add(v[j], gamma);
          num = Fr::mul(num, Fr::add(Fr::mul(v[26 + j], beta), wg));
          den = Fr::mul(den, Fr::add(Fr::mul(v[22 + j], beta), wg));
        }
        const Fr pit = Fr::add(Fr::mul(v[35], params.public_input_delta), zs);
        add(2, Fr::sub(Fr::mul(Fr::add(z, v[34]), num), Fr::mul(pit, den)));
        add(3, Fr::mul(Fr::mul(v[35], zs), sf));
      }
      if (do_lookup) {
        const Fr b2 = Fr::mul(beta, beta), b3 = Fr::mul(b2, beta);
        const Fr read = Fr::add(Fr::add(Fr::add(Fr::add(w_l, gamma), Fr::mul(q_r, w_ls)), Fr::mul(Fr::add(Fr::mul(q_m, w_rs), w_r), beta)),
                                Fr::add(Fr::mul(Fr::add(Fr::mul(q_c, w_os), w_o), b2), Fr::mul(q_o, b3)));
        const Fr write = Fr::add(Fr::add(Fr::add(v[30], gamma), Fr::mul(v[31], beta)), Fr::add(Fr::mul(v[32], b2), Fr::mul(v[33], b3)));
        const Fr exists = Fr::sub(Fr::add(tag, q_lookup), Fr::mul(tag, q_lookup));
        add(4, Fr::mul(Fr::sub(Fr::mul(Fr::mul(read, write), inv), exists), sf));
        add(5, Fr::sub(Fr::mul(Fr::mul(write, inv), q_lookup), Fr::mul(Fr::mul(read, inv), counts)));
        add(6, Fr::mul(Fr::sub(Fr::mul(tag, tag), tag), sf));
      }
      if (do_delta) {
        const Fr* hi[4] = {&w_r, &w_o, &w_4, &w_ls};
        const Fr* lo[4] = {&w_l, &w_r, &w_o, &w_4};
        for (int j = 0; j < 4; ++j) {
          const Fr d = Fr::sub(*hi[j], *lo[j]), a1 = Fr::sub(d, one), a2 = Fr::sub(d, two);
          const Fr t = Fr::mul(Fr::sub(Fr::mul(a1, a1), one), Fr::sub(Fr::mul(a2, a2), one));
          add(7 + j, Fr::mul(Fr::mul(t, q_delta), sf));
        }
      }
    }
  }
  HonkAccumulators<Fr> out;
  size_t at = 0;
  for (size_t s = 0; s < HONK_SUBRELATIONS; ++s)
    for (size_t i = 0; i < HONK_ACC_LENGTHS[s]; ++i) out[at++] = acc[s][i];
  return out;
}
// Univariate::extend_from (univariate.rs:57-178) to `size` points: the polynomial of degree < len through the points 0 .. len - 1, which
// is what each of the reference's four branches evaluates
template <class Fr>
inline std::vector<Fr> honk_extend_from(const Fr* poly, size_t len, size_t size) {
  std::vector<Fr> out(poly, poly + len);
  auto small = [](long x) { return x >= 0 ? Fr::from_u64((uint64_t)x) : Fr::sub(Fr::zero(), Fr::from_u64((uint64_t)-x)); };
  for (size_t x = len; x < size; ++x) {
    Fr total = Fr::zero();
    for (size_t i = 0; i < len; ++i) {
      Fr num = Fr::one(), den = Fr::one();
      for (size_t j = 0; j < len; ++j)
        if (j != i) num = Fr::mul(num, small((long)x - (long)j)), den = Fr::mul(den, small((long)i - (long)j));
      total = Fr::add(total, Fr::mul(Fr::mul(poly[i], num), Fr::inv(den)));
    }
    out.push_back(total);
  }
  return out;
}
// batch_over_relations_univariates (:109-122) for subrelations 0 .. 10: scale by first_scalar = 1 and alphas[0..10), extend each
// accumulator to BATCHED_RELATION_PARTIAL_LENGTH, multiply by the extended [1, beta_i] and by partial_evaluation_result -- except
// lookup.r1, the linearly dependent subrelation -- and sum
template <class Fr>
inline std::array<Fr, HONK_BATCHED_RELATION_PARTIAL_LENGTH> honk_batch_over_relations(const HonkAccumulators<Fr>& acc, const std::vector<Fr>& alphas,
                                                                                       const HonkGateSeparator<Fr>& gs) {
  if (alphas.size() < HONK_SUBRELATIONS - 1 || gs.current_element_idx >= gs.betas.size()) throw Error("compute_univariate: ten alphas and a current gate challenge");
  const Fr pow[2] = {Fr::one(), gs.betas[gs.current_element_idx]};
  const std::vector<Fr> random = honk_extend_from(pow, 2, HONK_BATCHED_RELATION_PARTIAL_LENGTH);
  std::array<Fr, HONK_BATCHED_RELATION_PARTIAL_LENGTH> result;
  for (auto& x : result) x = Fr::zero();
  size_t at = 0;
  for (size_t s = 0; s < HONK_SUBRELATIONS; ++s) {
    std::vector<Fr> scaled(acc.begin() + at, acc.begin() + at + HONK_ACC_LENGTHS[s]);
    at += HONK_ACC_LENGTHS[s];
    if (s)
      for (auto& x : scaled) x = Fr::mul(x, alphas[s - 1]);
    const std::vector<Fr> ext = honk_extend_from(scaled.data(), scaled.size(), HONK_BATCHED_RELATION_PARTIAL_LENGTH);
    for (size_t i = 0; i < HONK_BATCHED_RELATION_PARTIAL_LENGTH; ++i)
      result[i] = Fr::add(result[i], s == 5 ? ext[i] : Fr::mul(Fr::mul(ext[i], random[i]), gs.partial_evaluation_result));
  }
  return result;
}
// The same loop for subrelations 11 .. 27 on the device: csh_honk_sumcheck_accumulate_gates_dev, 110 elements come back
template <class P>
inline HonkGateAccumulators<typename P::Fr> plain_round_accumulators_gates(const std::vector<std::vector<typename P::Fr>>& cols, size_t edge_begin, size_t edge_end,
                                                                           const HonkGateSeparator<typename P::Fr>* gs,
                                                                           const HonkGateParameters<typename P::Fr>& params) {
  const typename P::Fr pr[8] = {params.eta_1, params.eta_2, params.eta_3, params.curve_b, params.mat_internal_diag_m_1[0], params.mat_internal_diag_m_1[1],
                                params.mat_internal_diag_m_1[2], params.mat_internal_diag_m_1[3]};
  return plain_round_device<P, HONK_GATES_ACC_ELEMS>("compute_round_accumulators_gates", csh_honk_sumcheck_accumulate_gates_dev,
                                                     "csh_honk_sumcheck_accumulate_gates_dev", HONK_GATES_COLUMNS, cols, edge_begin, edge_end, gs, pr);
}
// The same loop in plain C++ on one host thread, the five relations in the scalar shape of each file's verify_accumulate at each of the
// points 0 .. 6 (elliptic_relation.rs:163-240, memory_relation.rs:360-561, non_native_field_relation.rs:179-269,
// poseidon2_external_relation.rs:207-281, poseidon2_internal_relation.rs:202-270): what the mirror test holds the device against, and
// the host column of tools/honk_sumcheck_probe.py
template <class Fr>
inline HonkGateAccumulators<Fr> host_round_accumulators_gates(const std::vector<std::vector<Fr>>& cols, size_t edge_begin, size_t edge_end,
                                                              const HonkGateSeparator<Fr>* gs, const HonkGateParameters<Fr>& params) {
  honk_check_round("compute_round_accumulators_gates", HONK_GATES_COLUMNS, cols, edge_begin, edge_end, gs);
  const std::vector<Fr> table = gs ? honk_beta_products(gs->betas, gs->log_num_monomials) : std::vector<Fr>();
  auto mul = [](const Fr& x, const Fr& y) { return Fr::mul(x, y); };
  auto add = [](const Fr& x, const Fr& y) { return Fr::add(x, y); };
  auto sub = [](const Fr& x, const Fr& y) { return Fr::sub(x, y); };
  auto pow5 = [&](const Fr& x) { const Fr x2 = mul(x, x); return mul(mul(x2, x2), x); };
  const Fr one = Fr::one();
  Fr limb_size = one, sublimb_shift = one;
  for (int i = 0; i < 68; ++i) limb_size = add(limb_size, limb_size);
  for (int i = 0; i < 14; ++i) sublimb_shift = add(sublimb_shift, sublimb_shift);
  Fr acc[HONK_GATES_SUBRELATIONS][7];
  for (auto& a : acc)
    for (auto& x : a) x = Fr::zero();
  auto both_zero = [&](size_t c, size_t e) { return cols[c][e].is_zero() && cols[c][e + 1].is_zero(); };
  for (size_t e = edge_begin; e < edge_end; e += 2) {
    const Fr sf = gs ? table[(e >> 1) * gs->periodicity] : one;
    const bool do_elliptic = !both_zero(14, e), do_memory = !both_zero(15, e), do_nnf = !both_zero(16, e), do_ext = !both_zero(17, e), do_int = !both_zero(18, e);
    if (!(do_elliptic || do_memory || do_nnf || do_ext || do_int)) continue;
    Fr v[HONK_GATES_COLUMNS], delta[HONK_GATES_COLUMNS];
    for (size_t c = 0; c < HONK_GATES_COLUMNS; ++c) v[c] = cols[c][e], delta[c] = sub(cols[c][e + 1], cols[c][e]);
    for (int k = 0; k < 7; ++k) {
      if (k)
        for (size_t c = 0; c < HONK_GATES_COLUMNS; ++c) v[c] = add(v[c], delta[c]);  // extend_from of two points
      auto put = [&](int s, const Fr& x) { acc[s][k] = add(acc[s][k], x); };
      const Fr &w_1 = v[0], &w_2 = v[1], &w_3 = v[2], &w_4 = v[3], &w_1s = v[4], &w_2s = v[5], &w_3s = v[6], &w_4s = v[7];
      const Fr &q_m = v[8], &q_c = v[9], &q_1 = v[10], &q_2 = v[11], &q_3 = v[12], &q_4 = v[13];
      if (do_elliptic) {
        const Fr &x_1 = w_2, &y_1 = w_3, &x_2 = w_1s, &y_2 = w_4s, &y_3 = w_3s, &x_3 = w_2s, &q_sign = q_1;
        const Fr x_diff = sub(x_2, x_1), y1_sqr = mul(y_1, y_1), y1y2 = mul(mul(y_1, y_2), q_sign);
        const Fr x_add = add(add(sub(sub(mul(add(add(x_3, x_2), x_1), mul(x_diff, x_diff)), mul(y_2, y_2)), y1_sqr), y1y2), y1y2);
        const Fr qes = mul(v[14], sf), q_double = mul(qes, q_m), q_add = sub(qes, q_double);
        const Fr y1_plus_y3 = add(y_1, y_3);
        const Fr y_add = add(mul(y1_plus_y3, x_diff), mul(sub(x_3, x_1), sub(mul(y_2, q_sign), y_1)));
        const Fr x1_mul_3 = add(add(x_1, x_1), x_1), x_pow_4_mul_3 = mul(sub(y1_sqr, params.curve_b), x1_mul_3);
        const Fr y1_sqr_mul_2 = add(y1_sqr, y1_sqr), y1_sqr_mul_4 = add(y1_sqr_mul_2, y1_sqr_mul_2);
        const Fr x_double = sub(mul(add(add(x_3, x_1), x_1), y1_sqr_mul_4), add(add(x_pow_4_mul_3, x_pow_4_mul_3), x_pow_4_mul_3));
        const Fr y_double = sub(mul(mul(x1_mul_3, x_1), sub(x_1, x_3)), mul(add(y_1, y_1), y1_plus_y3));
        put(0, add(mul(x_add, q_add), mul(x_double, q_double)));
        put(1, add(mul(y_add, q_add), mul(y_double, q_double)));
      }
      if (do_memory) {
        const Fr partial = add(add(add(mul(w_3, params.eta_3), mul(w_2, params.eta_2)), mul(w_1, params.eta_1)), q_c);
        const Fr record = sub(partial, w_4);
        const Fr neg_index_delta = sub(w_1, w_1s), index_delta_is_zero = add(neg_index_delta, one);
        const Fr monotone = add(mul(neg_index_delta, neg_index_delta), neg_index_delta);
        const Fr qms = mul(v[15], sf), q12 = mul(q_1, q_2), q12ms = mul(q12, qms), q3ms = mul(q_3, qms);
        put(3, mul(mul(index_delta_is_zero, sub(w_4s, w_4)), q12ms));
        put(4, mul(monotone, q12ms));
        const Fr next = sub(add(add(mul(w_3s, params.eta_3), mul(w_2s, params.eta_2)), mul(w_1s, params.eta_1)), w_4s);
        put(5, mul(mul(mul(index_delta_is_zero, sub(w_3s, w_3)), add(next, one)), q3ms));
        put(6, mul(monotone, q3ms));
        put(7, mul(add(mul(next, next), next), q3ms));
        const Fr timestamp = sub(mul(index_delta_is_zero, sub(w_2s, w_2)), w_3);
        Fr identity = add(add(mul(record, q12), mul(timestamp, mul(q_4, q_1))), mul(record, mul(q_m, q_1)));
        identity = mul(identity, qms);  // memory_relation.rs:557; the RAM term below has the factor already
        put(2, add(identity, mul(add(mul(record, record), record), q3ms)));
      }
      if (do_nnf) {
        Fr lo = add(mul(w_1, w_2s), mul(w_1s, w_2));
        Fr gate_2 = mul(sub(add(mul(w_1, w_4), mul(w_2, w_3)), w_3s), limb_size);
        gate_2 = mul(add(sub(gate_2, w_4s), lo), q_4);
        const Fr hi = add(mul(lo, limb_size), mul(w_1s, w_2s));
        const Fr gate_1 = mul(sub(hi, add(w_3, w_4)), q_3);
        const Fr gate_3 = mul(sub(add(hi, w_4), add(w_3s, w_4s)), q_m);
        const Fr identity = mul(add(add(gate_1, gate_2), gate_3), q_2);
        Fr la_1 = mul(w_2s, sublimb_shift), la_2 = mul(w_3s, sublimb_shift);
        for (const Fr* t : {&w_1s, &w_3, &w_2}) la_1 = mul(add(la_1, *t), sublimb_shift);
        for (const Fr* t : {&w_2s, &w_1s, &w_4}) la_2 = mul(add(la_2, *t), sublimb_shift);
        la_1 = mul(sub(add(la_1, w_1), w_4), q_4);
        la_2 = mul(sub(add(la_2, w_3), w_4s), q_m);
        put(8, mul(mul(add(identity, mul(add(la_1, la_2), q_3)), v[16]), sf));
      }
      if (do_ext) {
        const Fr u_1 = pow5(add(w_1, q_1)), u_2 = pow5(add(w_2, q_2)), u_3 = pow5(add(w_3, q_3)), u_4 = pow5(add(w_4, q_4));
        const Fr t_0 = add(u_1, u_2), t_1 = add(u_3, u_4), t_2 = add(add(u_2, u_2), t_1), t_3 = add(add(u_4, u_4), t_0);
        const Fr t_1x2 = add(t_1, t_1), t_0x2 = add(t_0, t_0);
        const Fr v_4 = add(add(t_1x2, t_1x2), t_3), v_2 = add(add(t_0x2, t_0x2), t_2), v_1 = add(t_3, v_2), v_3 = add(t_2, v_4);
        const Fr qs = mul(v[17], sf);
        put(9, mul(sub(v_1, w_1s), qs)), put(10, mul(sub(v_2, w_2s), qs)), put(11, mul(sub(v_3, w_3s), qs)), put(12, mul(sub(v_4, w_4s), qs));
      }
      if (do_int) {
        const Fr u[4] = {pow5(add(w_1, q_1)), w_2, w_3, w_4};
        const Fr total = add(add(u[0], u[1]), add(u[2], u[3])), qs = mul(v[18], sf);
        for (int i = 0; i < 4; ++i) put(13 + i, mul(sub(add(mul(u[i], params.mat_internal_diag_m_1[i]), total), v[4 + i]), qs));
      }
    }
  }
  HonkGateAccumulators<Fr> out;
  size_t at = 0;
  for (size_t s = 0; s < HONK_GATES_SUBRELATIONS; ++s)
    for (size_t i = 0; i < HONK_GATES_ACC_LENGTHS[s]; ++i) out[at++] = acc[s][i];
  return out;
}
// batch_over_relations_univariates (:109-122) over all 28 accumulators: AllRelationAcc::scale with first_scalar = 1 and alphas[0..27) in
// the order arith, perm, lookup, delta, elliptic, memory, nnf, poseidon2 external, poseidon2 internal (relations/mod.rs:134-145), then
// extend_and_batch_univariates (:147-198): every accumulator extended to BATCHED_RELATION_PARTIAL_LENGTH; all but lookup.r1 -- so all
// seventeen of the second entry, linearly independent in each of the five files -- take the extended [1, beta_i] and
// partial_evaluation_result
template <class Fr>
inline std::array<Fr, HONK_BATCHED_RELATION_PARTIAL_LENGTH> honk_batch_over_all_relations(const HonkAccumulators<Fr>& acc, const HonkGateAccumulators<Fr>& gates,
                                                                                           const std::vector<Fr>& alphas, const HonkGateSeparator<Fr>& gs) {
  if (alphas.size() < HONK_NUM_ALPHAS || gs.current_element_idx >= gs.betas.size()) throw Error("compute_univariate_all: 27 alphas and a current gate challenge");
  const Fr pow[2] = {Fr::one(), gs.betas[gs.current_element_idx]};
  const std::vector<Fr> random = honk_extend_from(pow, 2, HONK_BATCHED_RELATION_PARTIAL_LENGTH);
  std::array<Fr, HONK_BATCHED_RELATION_PARTIAL_LENGTH> result;
  for (auto& x : result) x = Fr::zero();
  size_t at = 0;
  for (size_t s = 0; s < HONK_SUBRELATIONS + HONK_GATES_SUBRELATIONS; ++s) {
    const bool first = s < HONK_SUBRELATIONS;
    const size_t len = first ? HONK_ACC_LENGTHS[s] : HONK_GATES_ACC_LENGTHS[s - HONK_SUBRELATIONS];
    if (s == HONK_SUBRELATIONS) at = 0;
    const Fr* from = first ? acc.data() + at : gates.data() + at;
    std::vector<Fr> scaled(from, from + len);
    at += len;
    if (s)
      for (auto& x : scaled) x = Fr::mul(x, alphas[s - 1]);
    const std::vector<Fr> ext = honk_extend_from(scaled.data(), scaled.size(), HONK_BATCHED_RELATION_PARTIAL_LENGTH);
    for (size_t i = 0; i < HONK_BATCHED_RELATION_PARTIAL_LENGTH; ++i)
      result[i] = Fr::add(result[i], s == 5 ? ext[i] : Fr::mul(Fr::mul(ext[i], random[i]), gs.partial_evaluation_result));
  }
  return result;
}
}  // namespace detail

// ---- plain drivers (co-plonk/src/mpc/plain.rs, co-noir-common/src/mpc/plain.rs) -----------------------------------
template <class P>
struct PlainPlonkDriver {
  using Fr = typename P::Fr;
  using Fq = typename P::Fq;
  using ArithmeticShare = Fr;
  using PointShareG1 = Proj<Fq>;
  using State = UnitState;
  static std::vector<Fr> local_mul_vec(const std::vector<Fr>& a, const std::vector<Fr>& b, State& st) {
    return PlainGroth16Driver<P>::local_mul_vec(a, b, st);
  }
  static std::vector<Fr> fft(const std::vector<Fr>& data, const EvaluationDomain<P>& d) { return detail::transform<P, Fr>(data, d, false); }
  static std::vector<Fr> ifft(const std::vector<Fr>& data, const EvaluationDomain<P>& d) { return detail::transform<P, Fr>(data, d, true); }
  static PointShareG1 msm_public_points_g1(const std::vector<AffineT<Fq>>& points, const std::vector<Fr>& scalars) {
    return detail::msm_unchecked<Fq>(P::ID, CSH_G1, points, scalars.data(), scalars.size());  // plain.rs:183
  }
  static PointShareG1 msm_public_points(const std::vector<AffineT<Fq>>& points, const std::vector<Fr>& scalars) {  // co-noir plain.rs:271
    return msm_public_points_g1(points, scalars);
  }
  // co-plonk plain.rs:186-193: (evaluation, the coefficients handed back)
  static std::pair<Fr, std::vector<Fr>> evaluate_poly_public(std::vector<Fr> coeffs, const Fr& point) {
    const Fr e = detail::eval_poly<P, Fr>(coeffs, point);
    return {e, std::move(coeffs)};
  }
  static Fr eval_poly(const std::vector<Fr>& coeffs, const Fr& point) { return detail::eval_poly<P, Fr>(coeffs, point); }
  // Polynomial::factor_roots (polynomial.rs:183) and Round5::div_by_zerofier(inout, 1, beta) (co-plonk round5.rs:78-91)
  static void factor_roots(std::vector<Fr>& coeffs, const Fr& root) { detail::factor_roots<P, Fr>(coeffs, root); }
  static void div_by_zerofier(std::vector<Fr>& inout, size_t n, const Fr& beta) { detail::div_by_zerofier<P, Fr>(inout, n, beta); }
  // the multilinear folds: sumcheck's partially_evaluate (co_sumcheck_prover.rs:34-98), Gemini's compute_fold_polynomials
  // (co_shplemini_prover.rs:236-312) and evaluate_mle (polynomial.rs:270-312, shared_polynomial.rs:154-199); linear, no network
  using PartiallyEvaluatePolys = detail::PartiallyEvaluatePolys<P, Fr>;
  static PartiallyEvaluatePolys partially_evaluate(const std::vector<std::vector<Fr>>& pub, const std::vector<std::vector<Fr>>& shared, size_t round_size, const Fr& u) {
    return PartiallyEvaluatePolys(pub, shared, round_size, u);
  }
  static std::vector<std::vector<Fr>> compute_fold_polynomials(size_t log_n, const std::vector<Fr>& multilinear_challenge, const std::vector<Fr>& a_0, bool has_zk) {
    return detail::compute_fold_polynomials<P, Fr>(log_n, multilinear_challenge, a_0, has_zk);
  }
  static Fr evaluate_mle(const std::vector<Fr>& coeffs, const std::vector<Fr>& points) { return detail::evaluate_mle<P, Fr>(coeffs, points); }
  // Round3::compute_t (co-plonk/src/round3.rs:246-502) -> [t1, t2, t3]; the Rep3 and Shamir drivers have none here: their mul_vec is the
  // network's, the stages themselves (csh_plonk_quot_*) take every share type
  static std::array<std::vector<Fr>, 3> compute_t(const PlonkDomains<P>& domains, const PlonkQuotientZkey<Fr>& zkey, const PlonkQuotientInputs<Fr, Fr>& in) {
    return detail::plain_compute_t<P>(domains, zkey, in);
  }
  // Round2::compute_z (round2.rs:104-190) -> the blinded z(X) and its 4 n evaluations; Round5::compute_r + compute_wxi (round5.rs:118-259)
  // -> W_xi; Round5::compute_wxiw (round5.rs:262-278) -> W_xiw. The Rep3 and Shamir drivers have no compute_z here: their array_prod_mul
  // is the network's; the stages themselves (csh_plonk_z_operands_dev, csh_poly_lincomb_dev, ...) take every share type
  static PlonkPolyEval<Fr> compute_z(const PlonkDomains<P>& domains, const PlonkRound2Inputs<Fr>& in) { return detail::plain_compute_z<P>(domains, in); }
  static std::vector<Fr> compute_r_wxi(const PlonkRound5Inputs<Fr>& in) { return detail::plain_compute_r_wxi<P>(in); }
  static std::vector<Fr> compute_wxiw(const PlonkRound5Inputs<Fr>& in) { return detail::plain_compute_wxiw<P>(in); }
  // The Oink phase of UltraHonk (co-ultrahonk/src/co_oink/co_oink_prover.rs): add_ram_rom_memory_records_to_wire_4 (:119-160) -> memory.w_4;
  // compute_logderivative_inverses (:229-293) -> lookup_inverses; compute_grand_product (:382-507) -> z_perm. Device-only chains of the
  // csh_honk_* entries and the scans. The Rep3 and Shamir drivers have none here: their mul_many and array_prod_mul are the network's;
  // the entries themselves take every share type
  static std::vector<Fr> compute_w4(const HonkOinkInputs<Fr>& in) { return detail::plain_compute_w4<P>(in); }
  static std::vector<Fr> compute_logderivative_inverses(const HonkOinkInputs<Fr>& in) { return detail::plain_compute_logderivative_inverses<P>(in); }
  static std::vector<Fr> compute_grand_product(const HonkOinkInputs<Fr>& in, const std::vector<Fr>& w_4) { return detail::plain_compute_grand_product<P>(in, w_4); }
  // The sumcheck round of UltraHonk between two folds (ultrahonk/src/decider/sumcheck/sumcheck_round_prover.rs): the loop of
  // compute_univariate_inner (:239-252) for subrelations 0 .. 10 over the edges [edge_begin, edge_end) on the device
  // (csh_honk_pow_table_dev, csh_honk_sumcheck_accumulate_dev) -> the eleven accumulators; gate_separator == nullptr is the factor one of
  // compute_virtual_contribution (:388-421). compute_univariate finishes on the host as batch_over_relations_univariates does (:109-122)
  // -> the univariate of subrelations 0 .. 10 at the points 0 .. 7. The five remaining relations: compute_round_accumulators_gates below.
  static HonkAccumulators<Fr> compute_round_accumulators(const std::vector<std::vector<Fr>>& cols, size_t edge_begin, size_t edge_end,
                                                         const HonkGateSeparator<Fr>* gate_separator, const HonkRelationParameters<Fr>& params) {
    return detail::plain_round_accumulators<P>(cols, edge_begin, edge_end, gate_separator, params);
  }
  static std::array<Fr, HONK_BATCHED_RELATION_PARTIAL_LENGTH> compute_univariate(const std::vector<std::vector<Fr>>& cols, size_t round_size,
                                                                                 const HonkGateSeparator<Fr>& gate_separator,
                                                                                 const HonkRelationParameters<Fr>& params, const std::vector<Fr>& alphas) {
    return detail::honk_batch_over_relations(compute_round_accumulators(cols, 0, round_size, &gate_separator, params), alphas, gate_separator);
  }
  // The other five relations of the round, subrelations 11 .. 27 (elliptic, memory, non-native field, Poseidon2 external and internal),
  // over the same range on the device (csh_honk_sumcheck_accumulate_gates_dev) -> the seventeen accumulators. compute_univariate_all is
  // the reference's round univariate: both entries, then batch_over_relations_univariates over all 28 accumulators with 27 alphas.
  static HonkGateAccumulators<Fr> compute_round_accumulators_gates(const std::vector<std::vector<Fr>>& gate_cols, size_t edge_begin, size_t edge_end,
                                                                   const HonkGateSeparator<Fr>* gate_separator, const HonkGateParameters<Fr>& params) {
    return detail::plain_round_accumulators_gates<P>(gate_cols, edge_begin, edge_end, gate_separator, params);
  }
  static std::array<Fr, HONK_BATCHED_RELATION_PARTIAL_LENGTH> compute_univariate_all(const std::vector<std::vector<Fr>>& cols, const std::vector<std::vector<Fr>>& gate_cols,
                                                                                     size_t round_size, const HonkGateSeparator<Fr>& gate_separator,
                                                                                     const HonkRelationParameters<Fr>& params, const HonkGateParameters<Fr>& gate_params,
                                                                                     const std::vector<Fr>& alphas) {
    return detail::honk_batch_over_all_relations(compute_round_accumulators(cols, 0, round_size, &gate_separator, params),
                                                 compute_round_accumulators_gates(gate_cols, 0, round_size, &gate_separator, gate_params), alphas, gate_separator);
  }
  // co-plonk plain.rs:127-140 / co-noir plain.rs:240-252: every element's own inverse() there
  static std::vector<Fr> inv_vec(std::vector<Fr> a) {
    if (detail::batch_inverse<P>(a)) throw Error("Cannot invert zero");
    return a;
  }
  static void inv_many_in_place(std::vector<Fr>& a) {
    a = inv_vec(std::move(a));
  }
  static void inv_many_in_place_leaking_zeros(std::vector<Fr>& a) { detail::batch_inverse<P>(a); }
  // co-plonk plain.rs:195-247: the blinding r cancels in the clear, what is left is the running product of a1 a2 a3 (or its inverses)
  static std::vector<Fr> array_prod_mul(bool inv, const std::vector<Fr>& a1, const std::vector<Fr>& a2, const std::vector<Fr>& a3) {
    const size_t n = std::min(a1.size(), std::min(a2.size(), a3.size()));  // izip!
    std::vector<Fr> v(n);
    check(csh_vec_mul(P::ID, (const uint64_t*)a1.data(), (const uint64_t*)a2.data(), (uint64_t*)v.data(), n), "csh_vec_mul");
    check(csh_vec_mul(P::ID, (const uint64_t*)v.data(), (const uint64_t*)a3.data(), (uint64_t*)v.data(), n), "csh_vec_mul");
    check(csh_vec_prefix_prod(P::ID, (const uint64_t*)v.data(), (uint64_t*)v.data(), n), "csh_vec_prefix_prod");
    return inv ? inv_vec(std::move(v)) : v;
  }
};

// ---- Rep3 drivers (co-plonk/src/mpc/rep3.rs, co-noir-common/src/mpc/rep3.rs) -------------------------------------------
template <class P>
struct Rep3PlonkDriver {
  using Fr = typename P::Fr;
  using Fq = typename P::Fq;
  using ArithmeticShare = Rep3PrimeFieldShare<Fr>;
  using PointShareG1 = Rep3PointShare<Fq>;
  using State = Rep3State;
  // arithmetic::local_mul_vec (rep3/arithmetic.rs:132-146): additive shares out, masked; io_round_mul_vec reshares them
  static std::vector<Fr> local_mul_vec(const std::vector<ArithmeticShare>& a, const std::vector<ArithmeticShare>& b, State& st) {
    return Rep3Groth16Driver<P>::local_mul_vec(a, b, st);
  }
  // DomainCoeff on a share: both components through the same transform (rep3.rs:140-152)
  static std::vector<ArithmeticShare> fft(const std::vector<ArithmeticShare>& data, const EvaluationDomain<P>& d) {
    return detail::transform<P, ArithmeticShare>(data, d, false);
  }
  static std::vector<ArithmeticShare> ifft(const std::vector<ArithmeticShare>& data, const EvaluationDomain<P>& d) {
    return detail::transform<P, ArithmeticShare>(data, d, true);
  }
  // pointshare::msm_public_points (rep3/pointshare.rs:201-222) / the fast_msm pair of co-noir rep3.rs:258-266: split the
  // shares into their a and b vectors, one MSM each
  static PointShareG1 msm_public_points_g1(const std::vector<AffineT<Fq>>& points, const std::vector<ArithmeticShare>& scalars) {
    const size_t cnt = std::min(scalars.size(), points.size());
    PointShareG1 out{Proj<Fq>::inf(), Proj<Fq>::inf()};
    if (cnt == 0) return out;
    csh_bases_t h = nullptr;
    check(csh_bases_upload(P::ID, CSH_G1, points.data(), cnt, 0, &h), "csh_bases_upload");  // uploaded once for both MSMs
    // the shares go up as they lie in memory ({a, b} pairs); the library cuts the two component vectors out on the device
    // (csh_msm_shares) instead of the host unzip + two uploads of the reference's call sites
    csh::Jac<Fq> ja, jb;
    void* outs[2] = {&ja, &jb};
    const int rc = csh_msm_shares(h, 0, cnt, reinterpret_cast<const uint64_t*>(scalars.data()), 2, 1, outs);
    csh_bases_free(h);
    check(rc, "csh_msm_shares");
    out.a = ja.is_inf() ? Proj<Fq>::inf() : Proj<Fq>::from_affine(AffineT<Fq>{ja.x, ja.y});
    out.b = jb.is_inf() ? Proj<Fq>::inf() : Proj<Fq>::from_affine(AffineT<Fq>{jb.x, jb.y});
    return out;
  }
  static PointShareG1 msm_public_points(const std::vector<AffineT<Fq>>& points, const std::vector<ArithmeticShare>& scalars) {
    return msm_public_points_g1(points, scalars);
  }
  // poly::eval_poly on {a, b} shares (rep3/poly.rs:39-68): a linear map, no network
  static std::pair<ArithmeticShare, std::vector<ArithmeticShare>> evaluate_poly_public(std::vector<ArithmeticShare> coeffs, const Fr& point) {  // co-plonk rep3.rs:177-183
    const ArithmeticShare e = detail::eval_poly<P, ArithmeticShare>(coeffs, point);
    return {e, std::move(coeffs)};
  }
  static ArithmeticShare eval_poly(const std::vector<ArithmeticShare>& coeffs, const Fr& point) { return detail::eval_poly<P, ArithmeticShare>(coeffs, point); }
  // SharedPolynomial::factor_roots (shared_polynomial.rs:92-140) / div_by_zerofier on {a, b} shares: linear, no network
  static void factor_roots(std::vector<ArithmeticShare>& coeffs, const Fr& root) { detail::factor_roots<P, ArithmeticShare>(coeffs, root); }
  static void div_by_zerofier(std::vector<ArithmeticShare>& inout, size_t n, const Fr& beta) { detail::div_by_zerofier<P, ArithmeticShare>(inout, n, beta); }
  // the multilinear folds: sumcheck's partially_evaluate (co_sumcheck_prover.rs:34-98), Gemini's compute_fold_polynomials
  // (co_shplemini_prover.rs:236-312) and evaluate_mle (polynomial.rs:270-312, shared_polynomial.rs:154-199); linear, no network
  using PartiallyEvaluatePolys = detail::PartiallyEvaluatePolys<P, ArithmeticShare>;
  static PartiallyEvaluatePolys partially_evaluate(const std::vector<std::vector<Fr>>& pub, const std::vector<std::vector<ArithmeticShare>>& shared, size_t round_size, const Fr& u) {
    return PartiallyEvaluatePolys(pub, shared, round_size, u);
  }
  static std::vector<std::vector<ArithmeticShare>> compute_fold_polynomials(size_t log_n, const std::vector<Fr>& multilinear_challenge, const std::vector<ArithmeticShare>& a_0, bool has_zk) {
    return detail::compute_fold_polynomials<P, ArithmeticShare>(log_n, multilinear_challenge, a_0, has_zk);
  }
  static ArithmeticShare evaluate_mle(const std::vector<ArithmeticShare>& coeffs, const std::vector<Fr>& points) { return detail::evaluate_mle<P, ArithmeticShare>(coeffs, points); }
  // arithmetic::mul_open_vec (rep3/arithmetic.rs:342-354): masked local products, broadcast, sum of the three
  static std::vector<Fr> mul_open_vec(const std::vector<ArithmeticShare>& a, const std::vector<ArithmeticShare>& b, const LocalNetwork& net, State& st) {
    const std::vector<Fr> mine = local_mul_vec(a, b, st);
    const size_t bytes = sizeof(Fr) * mine.size();
    Bytes m(bytes);
    if (bytes) memcpy(m.data(), mine.data(), bytes);
    net.send((net.id() + 1) % 3, m);
    net.send((net.id() + 2) % 3, std::move(m));
    const Bytes pv = net.recv((net.id() + 2) % 3), nx = net.recv((net.id() + 1) % 3);
    if (pv.size() != bytes || nx.size() != bytes) throw Error("mul_open_vec: invalid number of elements received");
    std::vector<Fr> y(mine.size());
    const uint64_t* parts[3] = {(const uint64_t*)mine.data(), (const uint64_t*)pv.data(), (const uint64_t*)nx.data()};
    const Fr ones[3] = {Fr::one(), Fr::one(), Fr::one()};
    check(csh_lincomb(P::ID, parts, (const uint64_t*)ones, 3, (uint64_t*)y.data(), y.size()), "csh_lincomb");
    return y;
  }
  static std::vector<ArithmeticShare> inverse_of(const std::vector<ArithmeticShare>& a, const LocalNetwork& net, State& st, const char* zero_message) {
    std::vector<ArithmeticShare> r(a.size());
    for (auto& x : r) x = Rep3Groth16Driver<P>::rand(&net, st);
    std::vector<Fr> y = mul_open_vec(a, r, net, st);
    return detail::unmask_inverse<P, ArithmeticShare>(std::move(r), std::move(y), zero_message);
  }
  static std::vector<ArithmeticShare> inv_vec(const std::vector<ArithmeticShare>& a, const LocalNetwork& net, State& st) {  // rep3/arithmetic.rs:233-246
    return inverse_of(a, net, st, "During execution of inverse in MPC: cannot compute inverse of zero");
  }
  static void inv_many_in_place(std::vector<ArithmeticShare>& a, const LocalNetwork& net, State& st) {  // co-noir-common rep3.rs:216-235
    a = inverse_of(a, net, st, "Cannot compute inverse of zero");
  }
  static void inv_many_in_place_leaking_zeros(std::vector<ArithmeticShare>& a, const LocalNetwork& net, State& st) {  // rep3.rs:237-257
    a = inverse_of(a, net, st, nullptr);
  }
};

// ---- Shamir drivers (co-plonk/src/mpc/shamir.rs, co-noir-common/src/mpc/shamir.rs) ----------------------------------
template <class P>
struct ShamirPlonkDriver {
  using Fr = typename P::Fr;
  using Fq = typename P::Fq;
  using ArithmeticShare = Fr;  // ShamirPrimeFieldShare is repr(transparent)
  using PointShareG1 = Proj<Fq>;
  template <class State>
  static std::vector<Fr> local_mul_vec(const std::vector<Fr>& a, const std::vector<Fr>& b, State&) {  // shamir/arithmetic.rs:73-79
    std::vector<Fr> out(a.size());
    check(csh_vec_mul(P::ID, (const uint64_t*)a.data(), (const uint64_t*)b.data(), (uint64_t*)out.data(), a.size()), "csh_vec_mul");
    return out;
  }
  static std::vector<Fr> fft(const std::vector<Fr>& data, const EvaluationDomain<P>& d) { return detail::transform<P, Fr>(data, d, false); }
  static std::vector<Fr> ifft(const std::vector<Fr>& data, const EvaluationDomain<P>& d) { return detail::transform<P, Fr>(data, d, true); }
  static PointShareG1 msm_public_points_g1(const std::vector<AffineT<Fq>>& points, const std::vector<Fr>& scalars) {  // shamir/pointshare.rs:207-225
    return detail::msm_unchecked<Fq>(P::ID, CSH_G1, points, scalars.data(), scalars.size());
  }
  static PointShareG1 msm_public_points(const std::vector<AffineT<Fq>>& points, const std::vector<Fr>& scalars) {  // co-noir shamir.rs:255
    return msm_public_points_g1(points, scalars);
  }
  // linear on the shares (shamir/poly.rs; co-plonk shamir.rs evaluate_poly_public)
  static std::pair<Fr, std::vector<Fr>> evaluate_poly_public(std::vector<Fr> coeffs, const Fr& point) {
    const Fr e = detail::eval_poly<P, Fr>(coeffs, point);
    return {e, std::move(coeffs)};
  }
  static Fr eval_poly(const std::vector<Fr>& coeffs, const Fr& point) { return detail::eval_poly<P, Fr>(coeffs, point); }
  // SharedPolynomial::factor_roots (shared_polynomial.rs:92-140) / div_by_zerofier on Shamir shares: linear, no network
  static void factor_roots(std::vector<Fr>& coeffs, const Fr& root) { detail::factor_roots<P, Fr>(coeffs, root); }
  static void div_by_zerofier(std::vector<Fr>& inout, size_t n, const Fr& beta) { detail::div_by_zerofier<P, Fr>(inout, n, beta); }
  // the multilinear folds: sumcheck's partially_evaluate (co_sumcheck_prover.rs:34-98), Gemini's compute_fold_polynomials
  // (co_shplemini_prover.rs:236-312) and evaluate_mle (polynomial.rs:270-312, shared_polynomial.rs:154-199); linear, no network
  using PartiallyEvaluatePolys = detail::PartiallyEvaluatePolys<P, Fr>;
  static PartiallyEvaluatePolys partially_evaluate(const std::vector<std::vector<Fr>>& pub, const std::vector<std::vector<Fr>>& shared, size_t round_size, const Fr& u) {
    return PartiallyEvaluatePolys(pub, shared, round_size, u);
  }
  static std::vector<std::vector<Fr>> compute_fold_polynomials(size_t log_n, const std::vector<Fr>& multilinear_challenge, const std::vector<Fr>& a_0, bool has_zk) {
    return detail::compute_fold_polynomials<P, Fr>(log_n, multilinear_challenge, a_0, has_zk);
  }
  static Fr evaluate_mle(const std::vector<Fr>& coeffs, const std::vector<Fr>& points) { return detail::evaluate_mle<P, Fr>(coeffs, points); }
  // arithmetic::mul_open_vec (shamir/arithmetic.rs:262-290): degree-2t products, broadcast_next(n, 2t + 1) (network.rs:96-126),
  // reconstruction with open_lagrange_2t
  static std::vector<Fr> mul_open_vec(const std::vector<Fr>& a, const std::vector<Fr>& b, const LocalNetwork& net, ShamirState<Fr>& st) {
    UnitState us;
    const std::vector<Fr> mine = local_mul_vec(a, b, us);
    const size_t n = st.num_parties, num = 2 * st.threshold + 1, bytes = sizeof(Fr) * mine.size();
    Bytes m(bytes);
    if (bytes) memcpy(m.data(), mine.data(), bytes);
    for (size_t s = 1; s < num; ++s) net.send((int)((st.id + s) % n), m);
    std::vector<Bytes> got;
    std::vector<const uint64_t*> parts{(const uint64_t*)mine.data()};
    for (size_t r = 1; r < num; ++r) {
      got.push_back(net.recv((int)((st.id + n - r) % n)));
      if (got.back().size() != bytes) throw Error("mul_open_vec: invalid number of elements received");
    }
    for (const Bytes& g : got) parts.push_back((const uint64_t*)g.data());
    std::vector<Fr> y(mine.size());
    check(csh_lincomb(P::ID, parts.data(), (const uint64_t*)st.open_lagrange_2t.data(), num, (uint64_t*)y.data(), y.size()), "csh_lincomb");
    return y;
  }
  static std::vector<Fr> inverse_of(const std::vector<Fr>& a, const LocalNetwork& net, ShamirState<Fr>& st, const char* zero_message) {
    std::vector<Fr> r(a.size());
    for (auto& x : r) x = ShamirGroth16Driver<P>::rand(&net, st);
    std::vector<Fr> y = mul_open_vec(a, r, net, st);
    return detail::unmask_inverse<P, Fr>(std::move(r), std::move(y), zero_message);
  }
  static std::vector<Fr> inv_vec(const std::vector<Fr>& a, const LocalNetwork& net, ShamirState<Fr>& st) {  // shamir/arithmetic.rs:157-172
    return inverse_of(a, net, st, "Cannot compute inverse of zero");
  }
  static void inv_many_in_place(std::vector<Fr>& a, const LocalNetwork& net, ShamirState<Fr>& st) {  // co-noir-common shamir.rs
    a = inverse_of(a, net, st, "Cannot compute inverse of zero");
  }
  static void inv_many_in_place_leaking_zeros(std::vector<Fr>& a, const LocalNetwork& net, ShamirState<Fr>& st) {  // shamir.rs:228-248
    a = inverse_of(a, net, st, nullptr);
  }
};

// ---- the sumcheck round on shares (csrc/honk_co_relations.hip) -------------------------------------------------------------------------
// accumulate_relation_univariates_batch (co-noir/co-ultrahonk/src/co_decider/co_sumcheck/co_sumcheck_round.rs:140-218) for the arithmetic,
// permutation, delta-range and lookup relations over one party's state and network: every stretch of local arithmetic is a device stage,
// T::mul_many is the device's local product plus the party's network round, and arith.r0 is reshared at the end (:292).
//
// A network policy is what T::mul_many, T::local_mul_vec's randomness and T::reshare are for one party:
//   PROTOCOL, party()        the protocol and party_id of the device entries
//   masks<P>(pool, n)        the n mask elements that local_mul_vec draws, on the device (nullptr for protocol 0)
//   mul_many<P>(pool, lhs, rhs, n)   device share vectors of n shares -> their product, n shares on the device
//   reshare(half)            host half shares -> shares (ncomp values each)
// Protocol 0 with the identity network: one party, the product of the shares is the share of the product.
struct HonkCoIdentityNet {
  static constexpr uint32_t PROTOCOL = 0;
  uint32_t party() const { return 0; }
  template <class P>
  const uint64_t* masks(detail::DevicePool&, size_t) {
    return nullptr;
  }
  template <class P>
  uint64_t* mul_many(detail::DevicePool& pool, const uint64_t* lhs, const uint64_t* rhs, size_t n) {
    uint64_t* out = pool.fresh(32 * n);
    check(csh_vec_mul_dev(P::ID, lhs, rhs, out, n, nullptr), "csh_vec_mul_dev");
    return out;
  }
  template <class Fr>
  std::vector<Fr> reshare(const std::vector<Fr>& half) {
    return half;
  }
};
// Rep3 (rep3/arithmetic.rs:132-161): masked local products on the device, the half shares to the next party, the previous party's back
struct HonkCoRep3Net {
  static constexpr uint32_t PROTOCOL = 1;
  const LocalNetwork& net;
  Rep3State& st;
  uint32_t party() const { return (uint32_t)st.id; }
  template <class P>
  const uint64_t* masks(detail::DevicePool& pool, size_t n) {
    using Fr = typename P::Fr;
    const UninitBuf<Fr> m = st.rand.template masking_field_elements_vec<Fr>(n);
    uint64_t* d = pool.fresh(sizeof(Fr) * n);
    if (n) check(csh_memcpy_h2d(d, m.p, sizeof(Fr) * n), "csh_memcpy_h2d");
    return d;
  }
  template <class Fr>
  std::vector<Fr> reshare(const std::vector<Fr>& half) {  // reshare_vec: -> {a = mine, b = the previous party's}
    const size_t bytes = sizeof(Fr) * half.size();
    Bytes b(bytes);
    if (bytes) memcpy(b.data(), half.data(), bytes);
    net.send((net.id() + 1) % 3, std::move(b));
    const Bytes r = net.recv((net.id() + 2) % 3);
    if (r.size() != bytes) throw Error("reshare_vec: invalid number of elements received");
    std::vector<Fr> out(2 * half.size());
    for (size_t i = 0; i < half.size(); ++i) {
      out[2 * i] = half[i];
      memcpy((void*)&out[2 * i + 1], r.data() + sizeof(Fr) * i, sizeof(Fr));
    }
    return out;
  }
  template <class P>
  uint64_t* mul_many(detail::DevicePool& pool, const uint64_t* lhs, const uint64_t* rhs, size_t n) {
    using Fr = typename P::Fr;
    const uint64_t* mask = masks<P>(pool, n);
    uint64_t* half = pool.fresh(sizeof(Fr) * n);
    std::vector<Fr> h(n);
    if (n) {
      check(csh_rep3_local_mul_vec_dev(P::ID, lhs, rhs, mask, half, n, nullptr), "csh_rep3_local_mul_vec_dev");
      check(csh_memcpy_d2h(h.data(), half, sizeof(Fr) * n), "csh_memcpy_d2h");
    }
    return pool.up(reshare(h));
  }
};

constexpr size_t HONK_CO_POINTS = 7;  // batch elements per kept edge
namespace detail {
// What the relations of one party's batch share -- the network policy, the device columns, the range, the gate separator's table -- and
// one method per relation: its device stages with T::mul_many between them. A method returns the relation's accumulators as shares.
// up36 / up19 upload the columns of the first four relations (csh_honk_sumcheck_accumulate_dev's order) and of the five gate relations
// (csh_honk_sumcheck_accumulate_gates_dev's order); a relation is called only after the upload it reads.
template <class P, class Net>
struct HonkCoRound {
  using Fr = typename P::Fr;
  Net& net;
  const uint32_t protocol, party;
  const size_t ncomp, edge_begin, edge_end, edges;
  const char* what;
  DevicePool pool;
  const uint64_t* dc[HONK_SUMCHECK_COLUMNS] = {};
  const uint64_t* dg[HONK_GATES_COLUMNS] = {};
  uint64_t* table = nullptr;
  size_t stride = 1;
  Fr pr[3], gp[8];

  HonkCoRound(Net& n, size_t b, size_t e, const HonkGateSeparator<Fr>* gs, const char* w)
      : net(n), protocol(Net::PROTOCOL), party(n.party()), ncomp(Net::PROTOCOL + 1), edge_begin(b), edge_end(e), edges((e - b) / 2), what(w) {
    if ((edge_begin & 1) || (edge_end & 1) || edge_begin >= edge_end) fail("an even, non-empty range");
    if (gs && (gs->log_num_monomials > 28 || gs->betas.size() < gs->log_num_monomials || ((edge_end >> 1) - 1) * gs->periodicity >= (size_t(1) << gs->log_num_monomials)))
      fail("the gate separator's table is shorter than the range reads");
    if (gs) {
      stride = gs->periodicity;
      table = pool.fresh(sizeof(Fr) << gs->log_num_monomials);
      check(csh_honk_pow_table_dev(P::ID, (const uint64_t*)gs->betas.data(), gs->log_num_monomials, table, nullptr), "csh_honk_pow_table_dev");
    }
  }
  [[noreturn]] void fail(const char* why) const { throw Error(std::string(what) + ": " + why); }
  // `shared` leading columns hold ncomp values per element
  void up(const std::vector<std::vector<Fr>>& cols, size_t count, size_t shared, const uint64_t** d, const char* columns) {
    if (cols.size() != count) fail(columns);
    for (size_t c = 0; c < count; ++c)
      if (cols[c].size() < edge_end * (c < shared ? ncomp : 1)) fail("a column is shorter than the range");
    for (size_t c = 0; c < count; ++c) d[c] = pool.up(cols[c]);
  }
  void up36(const std::vector<std::vector<Fr>>& cols, const HonkRelationParameters<Fr>& params) {
    up(cols, HONK_SUMCHECK_COLUMNS, 13, dc, "36 columns");
    pr[0] = params.beta, pr[1] = params.gamma, pr[2] = params.public_input_delta;
  }
  void up19(const std::vector<std::vector<Fr>>& cols, const HonkGateParameters<Fr>& g) {
    up(cols, HONK_GATES_COLUMNS, 8, dg, "19 gate columns");
    gp[0] = g.eta_1, gp[1] = g.eta_2, gp[2] = g.eta_3, gp[3] = g.curve_b;
    for (size_t i = 0; i < 4; ++i) gp[4 + i] = g.mat_internal_diag_m_1[i];
  }
  const uint64_t* prm() const { return (const uint64_t*)pr; }
  const uint64_t* gprm() const { return (const uint64_t*)gp; }
  uint64_t* shares(size_t vectors, size_t m) { return pool.fresh(sizeof(Fr) * vectors * HONK_CO_POINTS * m * ncomp); }
  uint64_t* acc_shares(size_t elems) { return pool.fresh(sizeof(Fr) * elems * ncomp); }
  std::vector<Fr> down(const uint64_t* d, size_t count) {
    std::vector<Fr> v(count);
    check(csh_memcpy_d2h(v.data(), d, sizeof(Fr) * count), "csh_memcpy_d2h");
    return v;
  }
  // part q of a device vector of 7 m shares per part
  const uint64_t* part(const uint64_t* v, size_t q, size_t m) const { return v + q * HONK_CO_POINTS * m * ncomp * 4; }
  uint64_t* mul_many(const uint64_t* lhs, const uint64_t* rhs, size_t parts, size_t m) {
    return net.template mul_many<P>(pool, lhs, rhs, parts * HONK_CO_POINTS * m);
  }
  // fold_and_filter: the edges a relation keeps, by its selector
  struct Kept {
    uint32_t* list;
    size_t m;
  };
  Kept select(const uint64_t* selector) {
    Kept k{(uint32_t*)pool.fresh(4 * edges), 0};
    uint32_t* count = (uint32_t*)pool.fresh(4);
    check(csh_honk_co_select_edges_dev(P::ID, selector, edge_begin, edge_end, k.list, count, nullptr), "csh_honk_co_select_edges_dev");
    uint32_t c = 0;
    check(csh_memcpy_d2h(&c, count, 4), "csh_memcpy_d2h");
    k.m = c;
    return k;
  }

  // UltraArithmeticRelation -> r1 (5 shares); r0_half = the 6 half shares of r0, reshared by the caller at the end of the round
  std::vector<Fr> arith(std::vector<Fr>& r0_half) {
    const Kept k = select(dc[19]);
    const uint64_t* mask = protocol == 1 ? net.template masks<P>(pool, HONK_CO_POINTS * k.m) : nullptr;
    uint64_t *r0 = pool.fresh(sizeof(Fr) * 6), *r1 = acc_shares(5);
    check(csh_honk_co_arith_dev(P::ID, protocol, party, dc, edge_begin, edge_end, k.list, k.m, table, stride, mask, r0, r1, nullptr), "csh_honk_co_arith_dev");
    r0_half = down(r0, 6);
    return down(r1, 5 * ncomp);
  }
  // UltraPermutationRelation: never skipped -> r0 (6), r1 (3)
  std::vector<Fr> perm() {
    uint64_t *lhs = shares(4, edges), *rhs = shares(4, edges), *rhs2 = shares(2, edges), *acc = acc_shares(9);
    check(csh_honk_co_perm_operands_dev(P::ID, protocol, party, dc, edge_begin, edge_end, nullptr, edges, prm(), lhs, rhs, nullptr), "csh_honk_co_perm_operands_dev");
    const uint64_t* mul1 = mul_many(lhs, rhs, 4, edges);
    const uint64_t* num_den = mul_many(mul1, part(mul1, 2, edges), 2, edges);
    check(csh_honk_co_perm_operands2_dev(P::ID, protocol, party, dc, edge_begin, edge_end, nullptr, edges, prm(), rhs2, nullptr), "csh_honk_co_perm_operands2_dev");
    const uint64_t* prod = mul_many(num_den, rhs2, 2, edges);
    check(csh_honk_co_perm_finish_dev(P::ID, protocol, party, dc, edge_begin, edge_end, nullptr, edges, table, stride, prod, acc, nullptr), "csh_honk_co_perm_finish_dev");
    return down(acc, 9 * ncomp);
  }
  // DeltaRangeConstraintRelation -> r0 .. r3 (6 each)
  std::vector<Fr> delta() {
    const Kept k = select(dc[20]);
    uint64_t* acc = acc_shares(24);
    const uint64_t* mul = nullptr;
    if (k.m) {
      uint64_t* lhs = shares(8, k.m);
      check(csh_honk_co_delta_operands_dev(P::ID, protocol, party, dc, edge_begin, edge_end, k.list, k.m, lhs, nullptr), "csh_honk_co_delta_operands_dev");
      uint64_t* sqr = mul_many(lhs, lhs, 8, k.m);
      check(csh_honk_co_delta_sub_one_dev(P::ID, protocol, party, sqr, k.m, nullptr), "csh_honk_co_delta_sub_one_dev");
      mul = mul_many(sqr, part(sqr, 4, k.m), 4, k.m);
    }
    check(csh_honk_co_delta_finish_dev(P::ID, protocol, party, dc, edge_begin, edge_end, k.list, k.m, table, stride, mul, acc, nullptr), "csh_honk_co_delta_finish_dev");
    return down(acc, 24 * ncomp);
  }
  // LogDerivLookupRelation: never skipped -> r0 (5), r1 (5), r2 (3)
  std::vector<Fr> lookup() {
    uint64_t *read_term = shares(1, edges), *inverses = shares(1, edges), *lhs = shares(2, edges), *rhs = shares(2, edges);
    uint64_t *r0 = acc_shares(5), *acc = acc_shares(8);
    check(csh_honk_co_lookup_operands_dev(P::ID, protocol, party, dc, edge_begin, edge_end, nullptr, edges, prm(), read_term, inverses, nullptr), "csh_honk_co_lookup_operands_dev");
    const uint64_t* write_inverse = mul_many(read_term, inverses, 1, edges);
    check(csh_honk_co_lookup_mid_dev(P::ID, protocol, party, dc, edge_begin, edge_end, nullptr, edges, table, stride, prm(), write_inverse, r0, lhs, rhs, nullptr),
          "csh_honk_co_lookup_mid_dev");
    const uint64_t* mul = mul_many(lhs, rhs, 2, edges);
    check(csh_honk_co_lookup_finish_dev(P::ID, protocol, party, dc, edge_begin, edge_end, nullptr, edges, table, stride, prm(), mul, acc, nullptr), "csh_honk_co_lookup_finish_dev");
    std::vector<Fr> out = down(r0, 5 * ncomp);
    const std::vector<Fr> rest = down(acc, 8 * ncomp);
    out.insert(out.end(), rest.begin(), rest.end());
    return out;
  }
  // EllipticRelation (csrc/honk_co_gates.hip) -> r0, r1 (6 each). A relation without kept edges makes no network call.
  std::vector<Fr> elliptic() {
    const Kept k = select(dg[14]);
    uint64_t* acc = acc_shares(12);
    const uint64_t *mul1 = nullptr, *mul2 = nullptr;
    if (k.m) {
      uint64_t *lhs = shares(7, k.m), *rhs = shares(7, k.m), *lhs2 = shares(5, k.m), *rhs2 = shares(5, k.m);
      check(csh_honk_co_ell_operands_dev(P::ID, protocol, party, dg, edge_begin, edge_end, k.list, k.m, lhs, rhs, nullptr), "csh_honk_co_ell_operands_dev");
      mul1 = mul_many(lhs, rhs, 7, k.m);
      check(csh_honk_co_ell_operands2_dev(P::ID, protocol, party, dg, edge_begin, edge_end, k.list, k.m, gprm(), mul1, lhs2, rhs2, nullptr), "csh_honk_co_ell_operands2_dev");
      mul2 = mul_many(lhs2, rhs2, 5, k.m);
    }
    check(csh_honk_co_ell_finish_dev(P::ID, protocol, party, dg, edge_begin, edge_end, k.list, k.m, table, stride, mul1, mul2, acc, nullptr), "csh_honk_co_ell_finish_dev");
    return down(acc, 12 * ncomp);
  }
  // MemoryRelation -> r0 .. r5 (6 each); the second product's left operand is part 3 of the first product in place
  std::vector<Fr> memory() {
    const Kept k = select(dg[15]);
    uint64_t* acc = acc_shares(36);
    const uint64_t *mul = nullptr, *mul2 = nullptr;
    if (k.m) {
      uint64_t *lhs = shares(6, k.m), *rhs = shares(6, k.m), *rhs2 = shares(1, k.m);
      check(csh_honk_co_mem_operands_dev(P::ID, protocol, party, dg, edge_begin, edge_end, k.list, k.m, gprm(), lhs, rhs, rhs2, nullptr), "csh_honk_co_mem_operands_dev");
      mul = mul_many(lhs, rhs, 6, k.m);
      mul2 = mul_many(part(mul, 3, k.m), rhs2, 1, k.m);
    }
    check(csh_honk_co_mem_finish_dev(P::ID, protocol, party, dg, edge_begin, edge_end, k.list, k.m, table, stride, gprm(), mul, mul2, acc, nullptr), "csh_honk_co_mem_finish_dev");
    return down(acc, 36 * ncomp);
  }
  // NonNativeFieldRelation -> r0 (6)
  std::vector<Fr> nnf() {
    const Kept k = select(dg[16]);
    uint64_t* acc = acc_shares(6);
    const uint64_t* mul = nullptr;
    if (k.m) {
      uint64_t *lhs = shares(5, k.m), *rhs = shares(5, k.m);
      check(csh_honk_co_nnf_operands_dev(P::ID, protocol, party, dg, edge_begin, edge_end, k.list, k.m, lhs, rhs, nullptr), "csh_honk_co_nnf_operands_dev");
      mul = mul_many(lhs, rhs, 5, k.m);
    }
    check(csh_honk_co_nnf_finish_dev(P::ID, protocol, party, dg, edge_begin, edge_end, k.list, k.m, table, stride, mul, acc, nullptr), "csh_honk_co_nnf_finish_dev");
    return down(acc, 6 * ncomp);
  }
  // x^5 as the reference does it: s s, that squared, then times s
  const uint64_t* sbox(const uint64_t* s, size_t parts, size_t m) {
    const uint64_t* u = mul_many(s, s, parts, m);
    u = mul_many(u, u, parts, m);
    return mul_many(u, s, parts, m);
  }
  // Poseidon2ExternalRelation -> r0 .. r3 (7 each)
  std::vector<Fr> poseidon2_external() {
    const Kept k = select(dg[17]);
    uint64_t* acc = acc_shares(28);
    const uint64_t* u = nullptr;
    if (k.m) {
      uint64_t* s = shares(4, k.m);
      check(csh_honk_co_pos_ext_operands_dev(P::ID, protocol, party, dg, edge_begin, edge_end, k.list, k.m, s, nullptr), "csh_honk_co_pos_ext_operands_dev");
      u = sbox(s, 4, k.m);
    }
    check(csh_honk_co_pos_ext_finish_dev(P::ID, protocol, party, dg, edge_begin, edge_end, k.list, k.m, table, stride, u, acc, nullptr), "csh_honk_co_pos_ext_finish_dev");
    return down(acc, 28 * ncomp);
  }
  // Poseidon2InternalRelation -> r0 .. r3 (7 each)
  std::vector<Fr> poseidon2_internal() {
    const Kept k = select(dg[18]);
    uint64_t* acc = acc_shares(28);
    const uint64_t* u = nullptr;
    if (k.m) {
      uint64_t* s = shares(1, k.m);
      check(csh_honk_co_pos_int_operands_dev(P::ID, protocol, party, dg, edge_begin, edge_end, k.list, k.m, s, nullptr), "csh_honk_co_pos_int_operands_dev");
      u = sbox(s, 1, k.m);
    }
    check(csh_honk_co_pos_int_finish_dev(P::ID, protocol, party, dg, edge_begin, edge_end, k.list, k.m, table, stride, gprm(), u, acc, nullptr), "csh_honk_co_pos_int_finish_dev");
    return down(acc, 28 * ncomp);
  }
};
template <class Fr>
inline void honk_co_append(std::vector<Fr>& out, const std::vector<Fr>& v) {
  out.insert(out.end(), v.begin(), v.end());
}
}  // namespace detail

// cols: the 36 columns of csh_honk_sumcheck_accumulate_dev as the party holds them -- the 13 witness and shifted-witness columns as shares
// (ncomp = PROTOCOL + 1 values per element), the 23 precomputed columns public. -> the eleven accumulators back to back as shares,
// HONK_ACC_ELEMS * ncomp values. gs == nullptr: the factor one.
template <class P, class Net>
inline std::vector<typename P::Fr> co_compute_round_accumulators(Net& net, const std::vector<std::vector<typename P::Fr>>& cols, size_t edge_begin, size_t edge_end,
                                                                 const HonkGateSeparator<typename P::Fr>* gs, const HonkRelationParameters<typename P::Fr>& params) {
  using Fr = typename P::Fr;
  detail::HonkCoRound<P, Net> round(net, edge_begin, edge_end, gs, "co_compute_round_accumulators");
  round.up36(cols, params);
  std::vector<Fr> r0_half;
  std::vector<Fr> out = round.arith(r0_half);  // everything behind arith.r0, which is reshared last
  detail::honk_co_append(out, round.perm());
  const std::vector<Fr> delta = round.delta();
  detail::honk_co_append(out, round.lookup());
  detail::honk_co_append(out, delta);
  // AllRelationAccHalfShared::reshare (relations/mod.rs:140-162, co_sumcheck_round.rs:292): the one network message of arith.r0, behind
  // every relation's rounds as in the reference
  std::vector<Fr> all = net.reshare(r0_half);
  detail::honk_co_append(all, out);
  return all;
}
// The same for all nine relations in the order of accumulate_relation_univariates_batch (co_sumcheck_round.rs:140-218): arithmetic,
// permutation, delta range, elliptic, memory, non-native field, lookup, Poseidon2 external, Poseidon2 internal, so that a reference party
// sees the reference's sequence of messages. gate_cols: the 19 columns of csh_honk_sumcheck_accumulate_gates_dev, the first eight as
// shares. -> the 28 accumulators as shares in subrelation order: the eleven of co_compute_round_accumulators (HONK_ACC_ELEMS * ncomp
// values), then the seventeen of the gate relations (HONK_GATES_ACC_ELEMS * ncomp values).
template <class P, class Net>
inline std::vector<typename P::Fr> co_compute_round_accumulators_all(Net& net, const std::vector<std::vector<typename P::Fr>>& cols,
                                                                     const std::vector<std::vector<typename P::Fr>>& gate_cols, size_t edge_begin, size_t edge_end,
                                                                     const HonkGateSeparator<typename P::Fr>* gs, const HonkRelationParameters<typename P::Fr>& params,
                                                                     const HonkGateParameters<typename P::Fr>& gate_params) {
  using Fr = typename P::Fr;
  detail::HonkCoRound<P, Net> round(net, edge_begin, edge_end, gs, "co_compute_round_accumulators_all");
  round.up36(cols, params);
  round.up19(gate_cols, gate_params);
  std::vector<Fr> r0_half;
  std::vector<Fr> first = round.arith(r0_half);
  detail::honk_co_append(first, round.perm());
  const std::vector<Fr> delta = round.delta();
  std::vector<Fr> gates = round.elliptic();
  detail::honk_co_append(gates, round.memory());
  detail::honk_co_append(gates, round.nnf());
  detail::honk_co_append(first, round.lookup());
  detail::honk_co_append(first, delta);
  detail::honk_co_append(gates, round.poseidon2_external());
  detail::honk_co_append(gates, round.poseidon2_internal());
  std::vector<Fr> all = net.reshare(r0_half);
  detail::honk_co_append(all, first);
  detail::honk_co_append(all, gates);
  return all;
}
// batch_over_relations_univariates on one party's shares (co_sumcheck_round.rs:121-138): scale and extend_and_batch_univariates are linear
// in the shares with public coefficients and no public addend, so component by component. -> the 8 shares of the round univariate
template <class Fr>
inline std::vector<Fr> co_batch_over_relations(const std::vector<Fr>& acc, size_t ncomp, const std::vector<Fr>& alphas, const HonkGateSeparator<Fr>& gs) {
  if (acc.size() != HONK_ACC_ELEMS * ncomp) throw Error("co_batch_over_relations: 57 shares");
  std::vector<Fr> out(HONK_BATCHED_RELATION_PARTIAL_LENGTH * ncomp);
  for (size_t c = 0; c < ncomp; ++c) {
    HonkAccumulators<Fr> one;
    for (size_t i = 0; i < HONK_ACC_ELEMS; ++i) one[i] = acc[i * ncomp + c];
    const auto res = detail::honk_batch_over_relations(one, alphas, gs);
    for (size_t i = 0; i < res.size(); ++i) out[i * ncomp + c] = res[i];
  }
  return out;
}
// batch_over_relations_univariates over all 28 accumulators on one party's shares: acc = what co_compute_round_accumulators_all returns.
// -> the 8 shares of the whole round's univariate
template <class Fr>
inline std::vector<Fr> co_batch_over_all_relations(const std::vector<Fr>& acc, size_t ncomp, const std::vector<Fr>& alphas, const HonkGateSeparator<Fr>& gs) {
  if (acc.size() != (HONK_ACC_ELEMS + HONK_GATES_ACC_ELEMS) * ncomp) throw Error("co_batch_over_all_relations: 167 shares");
  std::vector<Fr> out(HONK_BATCHED_RELATION_PARTIAL_LENGTH * ncomp);
  for (size_t c = 0; c < ncomp; ++c) {
    HonkAccumulators<Fr> first;
    HonkGateAccumulators<Fr> gates;
    for (size_t i = 0; i < HONK_ACC_ELEMS; ++i) first[i] = acc[i * ncomp + c];
    for (size_t i = 0; i < HONK_GATES_ACC_ELEMS; ++i) gates[i] = acc[(HONK_ACC_ELEMS + i) * ncomp + c];
    const auto res = detail::honk_batch_over_all_relations(first, gates, alphas, gs);
    for (size_t i = 0; i < res.size(); ++i) out[i * ncomp + c] = res[i];
  }
  return out;
}

}  // namespace cosnarks
