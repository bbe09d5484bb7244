// C entry points of the host mirror, PLONK / UltraHonk part: the driver call sites of plonk_honk.hpp on caller data. Plain values come
// in; for Rep3 (three parties) and Shamir (three parties, threshold 1) they are shared inside with `seed`, and the parties' results go
// out one after the other. What is linear runs party by party on the calling thread; what talks runs as in-process parties.
#include "capi_common.hpp"

using namespace cosnarks;
using namespace cosnarks::capi;

namespace {

template <class Fr>
using R3 = Rep3PrimeFieldShare<Fr>;
constexpr uint64_t REP3_VALUES = 3, SHAMIR_VALUES = 2, SHAMIR_DEALER = 12;  // ShareRng domains
constexpr int NP = 3, T1 = 1;                                               // the Shamir parties of these entries and their threshold

template <class Fr>
std::vector<Fr> elements(const uint64_t* limbs, size_t n) {
  std::vector<Fr> v(n);
  if (n) memcpy((void*)v.data(), limbs, 32 * n);
  return v;
}
template <class Fr>
Fr element(const uint64_t* limbs) {
  Fr x;
  memcpy((void*)&x, limbs, 32);
  return x;
}
// the next `v.size()` elements of `out`, which moves on
template <class V>
void put(uint64_t*& out, const V& v) {
  const size_t bytes = sizeof(v[0]) * v.size();
  if (bytes) memcpy(out, v.data(), bytes);
  out += bytes / 8;
}

template <class P>
int driver_fft_t(int driver, int inverse, int snarkjs, const uint64_t* data, size_t n_in, size_t domain_size, uint64_t seed, uint64_t* out) {
  using Fr = typename P::Fr;
  EvaluationDomain<P> d = snarkjs ? EvaluationDomain<P>::snarkjs(domain_size) : EvaluationDomain<P>::arkworks(domain_size);
  std::vector<Fr> v(n_in);
  memcpy((void*)v.data(), data, 32 * n_in);
  if (driver != 1) {
    std::vector<Fr> r = driver == 0 ? (inverse ? PlainPlonkDriver<P>::ifft(v, d) : PlainPlonkDriver<P>::fft(v, d))
                                    : (inverse ? ShamirPlonkDriver<P>::ifft(v, d) : ShamirPlonkDriver<P>::fft(v, d));
    memcpy(out, r.data(), 32 * r.size());
    return (int)r.size();
  }
  std::vector<R3<Fr>> sh[3];
  FieldRng<Fr>(seed, REP3_VALUES).rep3(v, sh);
  for (int p = 0; p < 3; ++p) {  // local operation: no network, no randomness
    auto r = inverse ? Rep3PlonkDriver<P>::ifft(sh[p], d) : Rep3PlonkDriver<P>::fft(sh[p], d);
    memcpy(out + 8 * d.size * p, r.data(), 64 * r.size());
  }
  return (int)d.size;
}

template <class P>
int driver_mul_t(int driver, const uint64_t* a, const uint64_t* b, size_t n, uint64_t seed, uint64_t* out) {
  using Fr = typename P::Fr;
  std::vector<Fr> va(n), vb(n);
  memcpy((void*)va.data(), a, 32 * n);
  memcpy((void*)vb.data(), b, 32 * n);
  UnitState us;
  if (driver == 0 || driver == 2) {
    std::vector<Fr> r = driver == 0 ? PlainPlonkDriver<P>::local_mul_vec(va, vb, us) : ShamirPlonkDriver<P>::local_mul_vec(va, vb, us);
    memcpy(out, r.data(), 32 * n);
    return 0;
  }
  std::vector<R3<Fr>> sa[3], sb[3];
  FieldRng<Fr> sharer(seed, REP3_VALUES);
  sharer.rep3(va, sa);
  sharer.rep3(vb, sb);
  run_parties<1>(3, on_device(0), [&](int p, const LocalNetwork& net) {
    Rep3State st = rep3_state(seed, p, net);
    std::vector<Fr> r = Rep3PlonkDriver<P>::local_mul_vec(sa[p], sb[p], st);
    memcpy(out + 4 * n * p, r.data(), 32 * n);
  });
  return 0;
}

// ::eval_poly / ::evaluate_poly_public. Plain / Shamir: 4 limbs (a linear map of whatever vector it is handed); Rep3: the coefficients
// are shared inside with `seed`, out = [party][component][limb].
template <class P>
int driver_eval_poly_t(int driver, const uint64_t* coeffs, size_t n, const uint64_t* point, uint64_t seed, uint64_t* out) {
  using Fr = typename P::Fr;
  const std::vector<Fr> v = elements<Fr>(coeffs, n);
  const Fr x = element<Fr>(point);
  if (driver != 1) {
    const Fr e = driver == 0 ? PlainPlonkDriver<P>::evaluate_poly_public(v, x).first : ShamirPlonkDriver<P>::eval_poly(v, x);
    memcpy(out, &e, 32);
    return 0;
  }
  std::vector<R3<Fr>> sh[3];
  FieldRng<Fr>(seed, REP3_VALUES).rep3(v, sh);
  for (int p = 0; p < 3; ++p) {  // local operation: no network, no randomness
    const auto e = p == 0 ? Rep3PlonkDriver<P>::evaluate_poly_public(sh[p], x).first : Rep3PlonkDriver<P>::eval_poly(sh[p], x);
    memcpy(out + 8 * p, &e, 64);
  }
  return 0;
}

// ::factor_roots (zerofier = 0) / Round5::div_by_zerofier(inout, 1, root) (zerofier = 1). Plain: (n - 1, 4); Rep3: [party][n - 1][component][limb];
// Shamir: [party][n - 1][limb]. The coefficients are shared inside with `seed`. Returns the length that is left.
template <class P>
int driver_factor_roots_t(int driver, int zerofier, const uint64_t* coeffs, size_t n, const uint64_t* root, uint64_t seed, uint64_t* out) {
  using Fr = typename P::Fr;
  std::vector<Fr> v = elements<Fr>(coeffs, n);
  const Fr x = element<Fr>(root);
  auto divide = [&](auto driver_tag, auto& poly) {
    using D = decltype(driver_tag);
    if (zerofier) D::div_by_zerofier(poly, 1, x);
    else D::factor_roots(poly, x);
    put(out, poly);
    return (int)poly.size();
  };
  if (driver == 0) return divide(PlainPlonkDriver<P>(), v);
  int len = 0;
  if (driver == 1) {
    std::vector<R3<Fr>> sh[3];
    FieldRng<Fr>(seed, REP3_VALUES).rep3(v, sh);
    for (int p = 0; p < 3; ++p) len = divide(Rep3PlonkDriver<P>(), sh[p]);  // local operation: no network, no randomness
    return len;
  }
  std::vector<std::vector<Fr>> sh = FieldRng<Fr>(seed, SHAMIR_VALUES).shamir(v, T1, NP);
  for (int p = 0; p < NP; ++p) len = divide(ShamirPlonkDriver<P>(), sh[p]);
  return len;
}

// shplonk_batched_quotient over k claims: polys = the claim polynomials one after the other (lens[j] coefficients each), points and
// evals k elements, nu the batching challenge. Output layouts as driver_factor_roots_t with the longest polynomial's length, which is returned;
// polynomials and evaluations are shared inside with `seed`: claim by claim, the coefficients and then the evaluation.
template <class P>
int driver_batched_quotient_t(int driver, const uint64_t* polys, const size_t* lens, size_t k, const uint64_t* points, const uint64_t* evals,
                              const uint64_t* nu, uint64_t seed, uint64_t* out) {
  using Fr = typename P::Fr;
  const Fr nu_f = element<Fr>(nu);
  std::vector<OpeningClaim<Fr, Fr>> plain(k);
  for (size_t j = 0, at = 0; j < k; at += lens[j], ++j) plain[j] = {elements<Fr>(polys + 4 * at, lens[j]), element<Fr>(points + 4 * j), element<Fr>(evals + 4 * j)};
  auto quotient = [&](auto share_tag, const auto& claims) {
    const auto q = shplonk_batched_quotient<P, decltype(share_tag)>(claims, nu_f);
    put(out, q);
    return (int)q.size();
  };
  if (driver == 0) return quotient(Fr{}, plain);
  int len = 0;
  if (driver == 1) {
    std::vector<OpeningClaim<Fr, R3<Fr>>> cl[3];
    FieldRng<Fr> sharer(seed, REP3_VALUES);
    for (size_t j = 0; j < k; ++j) {
      std::vector<R3<Fr>> f[3], e[3];
      sharer.rep3(plain[j].polynomial, f);
      sharer.rep3({plain[j].evaluation}, e);
      for (int p = 0; p < 3; ++p) cl[p].push_back({std::move(f[p]), plain[j].challenge, e[p][0]});
    }
    for (int p = 0; p < 3; ++p) len = quotient(R3<Fr>{}, cl[p]);
    return len;
  }
  FieldRng<Fr> sharer(seed, SHAMIR_VALUES);
  std::vector<OpeningClaim<Fr, Fr>> cl[NP];
  for (size_t j = 0; j < k; ++j) {
    auto f = sharer.shamir(plain[j].polynomial, T1, NP);
    const auto e = sharer.shamir(plain[j].evaluation, T1, NP);
    for (int p = 0; p < NP; ++p) cl[p].push_back({std::move(f[p]), plain[j].challenge, e[p]});
  }
  for (int p = 0; p < NP; ++p) len = quotient(Fr{}, cl[p]);
  return len;
}

// The multilinear-fold mirror (plonk_honk.hpp): op 0 = partially_evaluate over npub public + nshared shared polynomials of n elements each
// (polys: one after the other, the public ones first), the first challenge through partially_evaluate_init, the others in place; op 1 =
// compute_fold_polynomials on polys = A_0 (n = 2^log_n elements) with nch = virtual_log_n challenges and has_zk = flags; op 2 = evaluate_mle.
// Shared values are shared inside with `seed`. out, per party (one for the plain driver, three otherwise): op 0 the public polynomials
// [npub][len][limb], then the shared ones [nshared][len][component][limb]; op 1 the returned list flattened; op 2 one share. Returns the
// elements per polynomial (op 0), in the flattened list (op 1), 1 (op 2).
template <class P, class D, class Share>
int mle_fold_party_t(int op, const std::vector<std::vector<typename P::Fr>>& pub, const std::vector<std::vector<Share>>& shared, size_t n,
                     const std::vector<typename P::Fr>& ch, int flags, uint64_t*& out) {
  if (op == 0) {
    auto pe = D::partially_evaluate(pub, shared, n, ch.at(0));
    for (size_t r = 1; r < ch.size(); ++r) pe.partially_evaluate_inplace(ch[r]);
    auto put_n = [&](const auto& poly) {
      if (pe.len()) memcpy(out, poly.data(), sizeof(poly[0]) * pe.len());
      out += sizeof(poly[0]) / 8 * pe.len();
    };
    for (size_t i = 0; i < pub.size(); ++i) put_n(pe.public_poly(i));
    for (size_t i = 0; i < shared.size(); ++i) put_n(pe.shared_poly(i));
    return (int)pe.len();
  }
  if (op == 1) {
    size_t log_n = 0;
    while ((size_t(1) << log_n) < n) ++log_n;
    const auto list = D::compute_fold_polynomials(log_n, ch, shared.at(0), flags != 0);
    size_t total = 0;
    for (const auto& f : list) {
      put(out, f);
      total += f.size();
    }
    return (int)total;
  }
  const Share e = D::evaluate_mle(shared.at(0), ch);
  memcpy(out, &e, sizeof(Share));
  out += sizeof(Share) / 8;
  return 1;
}
template <class P>
int driver_mle_fold_t(int driver, int op, const uint64_t* polys, size_t npub, size_t nshared, size_t n, const uint64_t* challenges, size_t nch,
                      int flags, uint64_t seed, uint64_t* out) {
  using Fr = typename P::Fr;
  const std::vector<Fr> ch = elements<Fr>(challenges, nch);
  std::vector<std::vector<Fr>> pub, sec;
  for (size_t i = 0; i < npub + nshared; ++i) (i < npub ? pub : sec).push_back(elements<Fr>(polys + 4 * n * i, n));
  int len = 0;
  if (driver == 0) return mle_fold_party_t<P, PlainPlonkDriver<P>, Fr>(op, pub, sec, n, ch, flags, out);
  if (driver == 1) {
    std::vector<std::vector<R3<Fr>>> sh[3];
    FieldRng<Fr> sharer(seed, REP3_VALUES);
    for (const auto& v : sec) {
      std::vector<R3<Fr>> parts[3];
      sharer.rep3(v, parts);
      for (int p = 0; p < 3; ++p) sh[p].push_back(std::move(parts[p]));
    }
    for (int p = 0; p < 3; ++p) len = mle_fold_party_t<P, Rep3PlonkDriver<P>, R3<Fr>>(op, pub, sh[p], n, ch, flags, out);  // local: no network
    return len;
  }
  FieldRng<Fr> sharer(seed, SHAMIR_VALUES);
  std::vector<std::vector<Fr>> sh[NP];
  for (const auto& v : sec) {
    auto parts = sharer.shamir(v, T1, NP);
    for (int p = 0; p < NP; ++p) sh[p].push_back(std::move(parts[p]));
  }
  for (int p = 0; p < NP; ++p) len = mle_fold_party_t<P, ShamirPlonkDriver<P>, Fr>(op, pub, sh[p], n, ch, flags, out);
  return len;
}

// PlainPlonkDriver::compute_t (plonk_honk.hpp). evals: a, b, c, z, qm, ql, qr, qo, qc, s1, s2, s3, then the n_public Lagrange vectors, 4 n
// elements each; scalars: buffer_a (n_public), b0..b10, beta, gamma, alpha, k1, k2. out: t1 (n + 1), t2 (n + 1), t3 (n + 6). Returns 3 n + 8.
template <class P>
int plonk_compute_t_t(size_t n, size_t n_public, const uint64_t* evals, const uint64_t* scalars, uint64_t* out) {
  using Fr = typename P::Fr;
  const size_t N = 4 * n;
  PlonkQuotientZkey<Fr> zkey;
  PlonkQuotientInputs<Fr, Fr> in;
  zkey.domain_size = n;
  std::vector<Fr>* dst[] = {&in.a, &in.b, &in.c, &in.z, &zkey.qm, &zkey.ql, &zkey.qr, &zkey.qo, &zkey.qc, &zkey.s1, &zkey.s2, &zkey.s3};
  zkey.lagrange.resize(n_public);
  for (size_t v = 0; v < 12 + n_public; ++v) {
    std::vector<Fr>& d = v < 12 ? *dst[v] : zkey.lagrange[v - 12];
    d.resize(N);
    memcpy((void*)d.data(), evals + 4 * N * v, 32 * N);
  }
  const Fr* sc = reinterpret_cast<const Fr*>(scalars);
  in.buffer_a.assign(sc, sc + n_public);
  sc += n_public;
  for (int j = 0; j < 11; ++j) in.blinders[j] = sc[j];
  in.beta = sc[11], in.gamma = sc[12], in.alpha = sc[13], zkey.k1 = sc[14], zkey.k2 = sc[15];
  const PlonkDomains<P> domains(n);
  const auto t = PlainPlonkDriver<P>::compute_t(domains, zkey, in);
  for (const auto& v : t) put(out, v);
  return (int)(3 * n + 8);
}

// ::inv_vec (leaking_zeros = 0), ::inv_many_in_place_leaking_zeros (1) and ::inv_many_in_place (2: inv_vec's protocol, the noir
// drivers' name and message). Plain: (n, 4); Rep3: [party][n][component][limb]; Shamir: [party][n][limb]. The values are shared inside
// with `seed`; a dealer hands the Shamir parties their double sharings.
template <class P>
int driver_inv_vec_t(int driver, const uint64_t* a, size_t n, uint64_t seed, int leaking_zeros, uint64_t* out) {
  using Fr = typename P::Fr;
  std::vector<Fr> v = elements<Fr>(a, n);
  auto invert = [&](auto driver_tag, const auto& shares, auto&... net_and_state) {
    using D = decltype(driver_tag);
    auto r = shares;
    if (leaking_zeros == 1) D::inv_many_in_place_leaking_zeros(r, net_and_state...);
    else if (leaking_zeros == 2) D::inv_many_in_place(r, net_and_state...);
    else r = D::inv_vec(shares, net_and_state...);
    return r;
  };
  if (driver == 0) {
    v = invert(PlainPlonkDriver<P>(), v);
    if (n) memcpy(out, v.data(), 32 * n);
    return 0;
  }
  if (driver == 1) {
    std::vector<R3<Fr>> sh[3];
    FieldRng<Fr>(seed, REP3_VALUES).rep3(v, sh);
    run_parties<1>(3, on_device(0), [&](int p, const LocalNetwork& net) {
      Rep3State st = rep3_state(seed, p, net);  // its seed exchange is over before the protocol's first message: one network serves both
      const auto r = invert(Rep3PlonkDriver<P>(), sh[p], net, st);
      if (n) memcpy(out + 8 * n * p, r.data(), 64 * n);
    });
    return 0;
  }
  const std::vector<std::vector<Fr>> sh = FieldRng<Fr>(seed, SHAMIR_VALUES).shamir(v, T1, NP);
  FieldRng<Fr> dealer(seed, SHAMIR_DEALER);
  std::vector<std::deque<std::pair<Fr, Fr>>> pairs(NP);
  for (size_t i = 0; i < n; ++i) dealer.double_sharing(T1, pairs);
  run_parties<1>(NP, on_device(0), [&](int p, const LocalNetwork& net) {
    auto state = ShamirState<Fr>::create(p, NP, T1, pairs[p]);
    const auto r = invert(ShamirPlonkDriver<P>(), sh[p], net, state);
    if (n) memcpy(out + 4 * n * p, r.data(), 32 * n);
  });
  return 0;
}

// PlainPlonkDriver::array_prod_mul (co-plonk plain.rs:195-247): out (n, 4)
template <class P>
int driver_array_prod_mul_t(int inv, const uint64_t* a1, const uint64_t* a2, const uint64_t* a3, size_t n, uint64_t* out) {
  using Fr = typename P::Fr;
  const std::vector<Fr> r = PlainPlonkDriver<P>::array_prod_mul(inv != 0, elements<Fr>(a1, n), elements<Fr>(a2, n), elements<Fr>(a3, n));
  if (n) memcpy(out, r.data(), 32 * n);
  return 0;
}

template <class C, class P>
int driver_msm_t(int driver, const void* points, size_t n_points, const uint64_t* scalars, size_t n_scalars, uint64_t seed, void* out) {
  using Fr = typename C::Fr;
  using Fq = typename C::Fq;
  std::vector<AffineT<Fq>> pts(n_points);
  memcpy((void*)pts.data(), points, sizeof(AffineT<Fq>) * n_points);
  std::vector<Fr> sc(n_scalars);
  memcpy((void*)sc.data(), scalars, 32 * n_scalars);
  auto put_point = [&](size_t slot, const Proj<Fq>& pt) {
    AffineT<Fq> a = into_affine(pt);
    memcpy(static_cast<char*>(out) + slot * sizeof a, &a, sizeof a);
  };
  if (driver == 3) {  // HonkCurve::fast_msm (BN254 G1 or Grumpkin)
    put_point(0, fast_msm<C>(pts, sc));
    return 0;
  }
  if constexpr (!std::is_same<P, void>::value) {
    if (driver == 0) put_point(0, PlainPlonkDriver<P>::msm_public_points_g1(pts, sc));
    else if (driver == 2) put_point(0, ShamirPlonkDriver<P>::msm_public_points(pts, sc));
    else {
      std::vector<R3<Fr>> sh[3];
      FieldRng<Fr>(seed, REP3_VALUES).rep3(sc, sh);
      for (int p = 0; p < 3; ++p) {
        auto r = Rep3PlonkDriver<P>::msm_public_points_g1(pts, sh[p]);
        put_point(2 * p, r.a);
        put_point(2 * p + 1, r.b);
      }
    }
    return 0;
  }
  throw Error("driver not available for this curve");
}
struct Grumpkin {  // cog16_driver_msm's third curve: no pairing, so no P
  static constexpr csh_curve_t ID = CSH_GRUMPKIN;
};

}  // namespace

extern "C" {

// PLONK / UltraHonk driver methods on caller data. driver: 0 plain, 1 Rep3 (three in-process parties, values shared with
// `seed`), 2 Shamir (the vector is one party's share vector), 3 (msm only) HonkCurve::fast_msm; curve 2 = Grumpkin (msm).
int cog16_driver_fft(int curve, int driver, int inverse, int snarkjs, const uint64_t* data, size_t n_in, size_t domain_size, uint64_t seed,
                     uint64_t* out) {
  return entry<Bn254, Bls12_381>(curve, [&](auto tag) { return driver_fft_t<decltype(tag)>(driver, inverse, snarkjs, data, n_in, domain_size, seed, out); });
}
int cog16_driver_local_mul_vec(int curve, int driver, const uint64_t* a, const uint64_t* b, size_t n, uint64_t seed, uint64_t* out) {
  return entry<Bn254, Bls12_381>(curve, [&](auto tag) { return driver_mul_t<decltype(tag)>(driver, a, b, n, seed, out); });
}
int cog16_driver_eval_poly(int curve, int driver, const uint64_t* coeffs, size_t n, const uint64_t* point, uint64_t seed, uint64_t* out) {
  return entry<Bn254, Bls12_381>(curve, [&](auto tag) { return driver_eval_poly_t<decltype(tag)>(driver, coeffs, n, point, seed, out); });
}
int cog16_driver_factor_roots(int curve, int driver, int zerofier, const uint64_t* coeffs, size_t n, const uint64_t* root, uint64_t seed, uint64_t* out) {
  return entry<Bn254, Bls12_381>(curve, [&](auto tag) { return driver_factor_roots_t<decltype(tag)>(driver, zerofier, coeffs, n, root, seed, out); });
}
int cog16_driver_batched_quotient(int curve, int driver, const uint64_t* polys, const size_t* lens, size_t k, const uint64_t* points,
                                  const uint64_t* evals, const uint64_t* nu, uint64_t seed, uint64_t* out) {
  return entry<Bn254, Bls12_381>(curve, [&](auto tag) { return driver_batched_quotient_t<decltype(tag)>(driver, polys, lens, k, points, evals, nu, seed, out); });
}
int cog16_driver_mle_fold(int curve, int driver, int op, const uint64_t* polys, size_t npub, size_t nshared, size_t n, const uint64_t* challenges,
                          size_t nch, int flags, uint64_t seed, uint64_t* out) {
  return guarded([&] {
    if (op < 0 || op > 2 || (op != 0 && (npub != 0 || nshared != 1))) throw Error("mle_fold: op 0 .. 2; ops 1 and 2 take one shared polynomial");
    return with_curve<Bn254, Bls12_381>(curve, [&](auto tag) {
      return driver_mle_fold_t<decltype(tag)>(driver, op, polys, npub, nshared, n, challenges, nch, flags, seed, out);
    });
  });
}
int cog16_plonk_compute_t(int curve, size_t n, size_t n_public, const uint64_t* evals, const uint64_t* scalars, uint64_t* out) {
  return entry<Bn254, Bls12_381>(curve, [&](auto tag) { return plonk_compute_t_t<decltype(tag)>(n, n_public, evals, scalars, out); });
}
int cog16_driver_inv_vec(int curve, int driver, const uint64_t* a, size_t n, uint64_t seed, int leaking_zeros, uint64_t* out) {
  return entry<Bn254, Bls12_381>(curve, [&](auto tag) { return driver_inv_vec_t<decltype(tag)>(driver, a, n, seed, leaking_zeros, out); });
}
int cog16_driver_array_prod_mul(int curve, int inv, const uint64_t* a1, const uint64_t* a2, const uint64_t* a3, size_t n, uint64_t* out) {
  return entry<Bn254, Bls12_381>(curve, [&](auto tag) { return driver_array_prod_mul_t<decltype(tag)>(inv, a1, a2, a3, n, out); });
}
int cog16_driver_msm(int curve, int driver, const void* points, size_t n_points, const uint64_t* scalars, size_t n_scalars, uint64_t seed,
                     void* out) {
  return entry<Bn254, Bls12_381, Grumpkin>(curve, [&](auto tag) {
    using P = decltype(tag);
    if constexpr (std::is_same<P, Grumpkin>::value) return driver_msm_t<GrumpkinCurve, void>(driver, points, n_points, scalars, n_scalars, seed, out);
    else return driver_msm_t<G1Of<P>, P>(driver, points, n_points, scalars, n_scalars, seed, out);
  });
}

}  // extern "C"
