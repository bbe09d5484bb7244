// Drivers mirroring `CircomGroth16Prover<P>` (co-circom/co-groth16/src/mpc.rs:22-138) and its three
// implementors PlainGroth16Driver (mpc/plain.rs:13-134), Rep3Groth16Driver (mpc/rep3.rs:16-162) and
// ShamirGroth16Driver (mpc/shamir.rs:14-148, local methods). Same method names and argument meaning; the hot
// methods (local_mul_vec, distribute_powers_and_mul_by_const, msm_public_points_hs and the NTTs inside the
// reduction) call the C ABI of include/cosnarks_hip.h, everything else is host code as in the reference.
#pragma once
#include <deque>
#include <random>

#include "network.hpp"
#include "types.hpp"

namespace cosnarks {

// A slice of a device-resident query: the mirror of `&query[lo..]`
struct BasesView {
  csh_bases_t bases;
  size_t offset, len;
};

template <class F>
inline Proj<F> msm_device(const BasesView& v, const void* scalars_mont, size_t n) {
  csh::Jac<F> out;
  const size_t cnt = n < v.len ? n : v.len;  // msm_unchecked: the shorter of the two slices
  check(csh_msm(v.bases, v.offset, cnt, reinterpret_cast<const uint64_t*>(scalars_mont), 1, &out), "csh_msm");
  if (out.is_inf()) return Proj<F>::inf();
  return Proj<F>::from_affine(AffineT<F>{out.x, out.y});
}

// scalars already in HBM, given as a raw device pointer (a range of a resident vector)
template <class F>
inline Proj<F> msm_device_resident_ptr(const BasesView& v, const void* scalars_dev, size_t n) {
  csh::Jac<F> out;
  const size_t cnt = n < v.len ? n : v.len;
  check(csh_msm_dev(v.bases, v.offset, cnt, reinterpret_cast<const uint64_t*>(scalars_dev), 1, &out, nullptr), "csh_msm_dev");
  if (out.is_inf()) return Proj<F>::inf();
  return Proj<F>::from_affine(AffineT<F>{out.x, out.y});
}
template <class F>
inline Proj<F> msm_device_resident(const BasesView& v, const DeviceScalars& s) { return msm_device_resident_ptr<F>(v, s.dev, s.n); }

// ---- Rep3 types (mpc-core/src/protocols/rep3/arithmetic/types.rs:21-28, rngs.rs:83-187) -----------------------
template <class Fr>
struct Rep3PrimeFieldShare {
  Fr a, b;
};

struct Rep3Rand {
  ChaCha12 rng1, rng2;  // own key, previous party's key (rep3.rs:71-76 setup_prf)
  Rep3Rand(const uint8_t s1[32], const uint8_t s2[32]) : rng1(s1), rng2(s2) {}
  // rngs.rs:137-156. The reference fills its two byte vectors under rayon::join and converts them with par_chunks(..).with_min_len(512)
  // into a freshly collected Vec. The keystream is counter-mode, so the mirror cuts BOTH streams into the same element ranges over the
  // host's cores (same bytes, same elements, the generators end where a serial draw would leave them) and writes into memory that
  // is not zero-filled first -- this is the host cost a Rep3 party pays per local_mul_vec on the zero-upstream-edit path
  // (bench: rep3_trait_path.mask_draw_ms).
  template <class Fr>
  UninitBuf<Fr> masking_field_elements_vec(size_t len) {
    UninitBuf<Fr> out(len);
    const uint64_t p1 = rng1.byte_pos(), p2 = rng2.byte_pos();
    const ChaCha12 &r1 = rng1, &r2 = rng2;
    Fr* o = out.data();
    parallel_for(len, 1 << 13, [&r1, &r2, p1, p2, o](size_t lo, size_t hi) {
      ChaCha12 a = r1, b = r2;
      a.seek(p1 + 32 * (uint64_t)lo);
      b.seek(p2 + 32 * (uint64_t)lo);
      uint8_t x[32], y[32];
      for (size_t i = lo; i < hi; ++i) {
        a.fill_bytes(x, 32);
        b.fill_bytes(y, 32);
        o[i] = mask_element_from_be_bytes<Fr>(x, y);
      }
    });
    rng1.seek(p1 + 32 * (uint64_t)len);
    rng2.seek(p2 + 32 * (uint64_t)len);
    return out;
  }
  template <class Fr>
  std::pair<Fr, Fr> random_fes() {  // rngs.rs:109-113 (sampling restated as one 32-byte mod-order draw per stream)
    uint8_t a[32], b[32];
    rng1.fill_bytes(a, 32);
    rng2.fill_bytes(b, 32);
    return {from_be_bytes_mod_order<Fr>(a), from_be_bytes_mod_order<Fr>(b)};
  }
  // Hand a run of `n` mask elements to the device generator (csh_rep3_masks / csh_groth16_h_rep3_seeded): returns the
  // chunk offsets of the run in both streams and advances both generators by 32*n bytes, exactly what
  // masking_field_elements_vec(n) would have consumed.
  struct DeviceRun {
    uint8_t seed1[32], seed2[32];
    uint64_t off1, off2;
  };
  DeviceRun take_device_run(size_t n) {
    DeviceRun r;
    memcpy(r.seed1, rng1.key, 32);
    memcpy(r.seed2, rng2.key, 32);
    const uint64_t p1 = rng1.byte_pos(), p2 = rng2.byte_pos();
    if (p1 % 32 || p2 % 32) throw Error("Rep3Rand: stream position not aligned to a field-element chunk");
    r.off1 = p1 / 32;
    r.off2 = p2 / 32;
    rng1.seek(p1 + 32 * (uint64_t)n);
    rng2.seek(p2 + 32 * (uint64_t)n);
    return r;
  }
  // `rng.gen::<[u8; 32]>()` of rand 0.8 (the reference pins rand = "0.8", Cargo.toml:70; un-vendored): Standard samples an array element
  // by element and a u8 as `next_u32() as u8`, so a 32-byte seed consumes 32 keystream WORDS (128 bytes), one low byte each. Restated
  // from the published crate; no reference fixture pins it (it only matters if a mirror party ever shared a session with a reference
  // party after a fork -- the Rust shim runs the reference's own code here).
  static void gen_seed(ChaCha12& rng, uint8_t out[32]) {
    for (int i = 0; i < 32; ++i) {
      uint8_t w[4];
      rng.fill_bytes(w, 4);
      out[i] = w[0];  // little-endian word: the low byte
    }
  }
  // rngs.rs:233-237: one fresh seed from each generator. Party i's rng1 is party i+1's rng2 (rep3.rs:71-76), so the seed party i draws
  // from rng1 equals the one party i+1 draws from rng2: streams keyed with them are correlated exactly like the parents.
  void random_seeds(uint8_t s1[32], uint8_t s2[32]) {
    gen_seed(rng1, s1);
    gen_seed(rng2, s2);
  }
  Rep3Rand fork() {  // rngs.rs:96-100
    uint8_t s1[32], s2[32];
    random_seeds(s1, s2);
    return Rep3Rand(s1, s2);
  }
};

struct Rep3State {
  int id;
  Rep3Rand rand;
  // Rep3State::new (rep3.rs:56-76): draw a seed, send it to the next party, receive the previous party's
  static Rep3State create(const LocalNetwork& net, const uint8_t my_seed[32]) {
    struct Seed { uint8_t b[32]; } s, prev;
    memcpy(s.b, my_seed, 32);
    prev = net.reshare(s);
    return Rep3State{net.id(), Rep3Rand(s.b, prev.b)};
  }
  Rep3State fork(size_t) { return Rep3State{id, rand.fork()}; }
};

struct UnitState {
  int id = 0;
  UnitState fork(size_t) { return *this; }
};

// ================================= PlainGroth16Driver (mpc/plain.rs) =================================
template <class P>
struct PlainGroth16Driver {
  using Fr = typename P::Fr;
  using ArithmeticShare = Fr;
  using ArithmeticHalfShare = Fr;
  using State = UnitState;
  using Net = LocalNetwork;
  static constexpr int PROTOCOL = 0;   // csh_groth16_h protocol id
  static constexpr uint32_t NCOMP = 1;
  static constexpr bool DEVICE_MASKS = false;

  static ArithmeticShare rand(const Net*, State&) {  // mpc/plain.rs:23-26
    uint8_t b[32];
    secure_random_bytes(b, 32);  // thread_rng() in the reference: a CSPRNG
    return from_be_bytes_mod_order<Fr>(b);
  }
  static ArithmeticShare evaluate_constraint(int, const std::vector<std::pair<Fr, size_t>>& lhs, const std::vector<Fr>& pub,
                                             const std::vector<ArithmeticShare>& wit) {  // mpc/plain.rs:28-43
    Fr acc = Fr::zero();
    for (auto& [coeff, index] : lhs)
      acc = Fr::add(acc, Fr::mul(coeff, index < pub.size() ? pub[index] : wit[index - pub.size()]));
    return acc;
  }
  static std::vector<ArithmeticShare> promote_to_trivial_shares(int, const std::vector<Fr>& v) { return v; }
  static std::vector<Fr> local_mul_vec(const std::vector<ArithmeticShare>& a, const std::vector<ArithmeticShare>& b, State&) {
    std::vector<Fr> out(a.size());  // mpc/plain.rs:83-89
    check(csh_vec_mul(P::ID, (const uint64_t*)a.data(), (const uint64_t*)b.data(), (uint64_t*)out.data(), a.size()), "csh_vec_mul");
    return out;
  }
  static void distribute_powers_and_mul_by_const(std::vector<ArithmeticShare>& c, const std::vector<Fr>& roots) {
    check(csh_vec_mul_table(P::ID, (uint64_t*)c.data(), (const uint64_t*)roots.data(), c.size(), 1), "csh_vec_mul_table");
  }
  static ArithmeticHalfShare to_half_share(const ArithmeticShare& a) { return a; }
  static UninitBuf<Fr> masks(State&, size_t) { return {}; }
  template <class F>
  static Proj<F> msm_public_points_hs(const BasesView& pts, const std::vector<ArithmeticHalfShare>& s) {  // mpc/plain.rs:66-74
    return msm_device<F>(pts, s.data(), s.size());
  }
  template <class F>
  static Proj<F> msm_public_points_hs(const BasesView& pts, const DeviceScalars& s) {  // same MSM, scalars already in HBM
    return msm_device_resident<F>(pts, s);
  }
  template <class F>
  static Proj<F> scalar_mul_public_point_hs(const Proj<F>& a, const ArithmeticHalfShare& b) { return point_mul(a, b); }
  template <class F>
  static void add_assign_points_public_hs(int, Proj<F>& a, const Proj<F>& b) { a = point_add(a, b); }
  template <class F>
  static Proj<F> open_half_point(const Proj<F>& a, const Net*, State&) { return a; }
  template <class F>
  static Proj<F> scalar_mul(const Proj<F>& a, const ArithmeticShare& b, const Net*, State&) { return point_mul(a, b); }
};

// ================================= Rep3Groth16Driver (mpc/rep3.rs) =================================
template <class P>
struct Rep3Groth16Driver {
  using Fr = typename P::Fr;
  using ArithmeticShare = Rep3PrimeFieldShare<Fr>;
  using ArithmeticHalfShare = Fr;
  using State = Rep3State;
  using Net = LocalNetwork;
  static constexpr int PROTOCOL = 1;
  static constexpr uint32_t NCOMP = 2;
  static constexpr bool DEVICE_MASKS = true;  // masks of the big local_mul_vec calls are generated on the GPU ("next" row f2)

  static ArithmeticShare rand(const Net*, State& st) {  // mpc/rep3.rs:27-29 -> arithmetic::rand (arithmetic.rs:357-360)
    auto [a, b] = st.rand.template random_fes<Fr>();
    return {a, b};
  }
  static ArithmeticShare evaluate_constraint(int id, const std::vector<std::pair<Fr, size_t>>& lhs, const std::vector<Fr>& pub,
                                             const std::vector<ArithmeticShare>& wit) {  // mpc/rep3.rs:31-49
    ArithmeticShare acc{Fr::zero(), Fr::zero()};
    for (auto& [coeff, index] : lhs) {
      if (index < pub.size()) {
        Fr m = Fr::mul(pub[index], coeff);  // add_assign_public: party 0 -> a, party 1 -> b (arithmetic.rs:52-58)
        if (id == 0) acc.a = Fr::add(acc.a, m);
        else if (id == 1) acc.b = Fr::add(acc.b, m);
      } else {
        const ArithmeticShare& w = wit[index - pub.size()];
        acc.a = Fr::add(acc.a, Fr::mul(w.a, coeff));
        acc.b = Fr::add(acc.b, Fr::mul(w.b, coeff));
      }
    }
    return acc;
  }
  static std::vector<ArithmeticShare> promote_to_trivial_shares(int id, const std::vector<Fr>& v) {  // types.rs:69-82
    std::vector<ArithmeticShare> out(v.size(), {Fr::zero(), Fr::zero()});
    for (size_t i = 0; i < v.size(); ++i) {
      if (id == 0) out[i].a = v[i];
      else if (id == 1) out[i].b = v[i];
    }
    return out;
  }
  static UninitBuf<Fr> masks(State& st, size_t n) { return st.rand.template masking_field_elements_vec<Fr>(n); }
  static std::vector<Fr> local_mul_vec(const std::vector<ArithmeticShare>& a, const std::vector<ArithmeticShare>& b, State& st) {
    const UninitBuf<Fr> mask = masks(st, a.size());  // arithmetic.rs:132-146
    std::vector<Fr> out(a.size());
    check(csh_rep3_local_mul_vec(P::ID, (const uint64_t*)a.data(), (const uint64_t*)b.data(), (const uint64_t*)mask.data(),
                                 (uint64_t*)out.data(), a.size()), "csh_rep3_local_mul_vec");
    return out;
  }
  static void distribute_powers_and_mul_by_const(std::vector<ArithmeticShare>& c, const std::vector<Fr>& roots) {  // mpc/rep3.rs:95-106
    check(csh_vec_mul_table(P::ID, (uint64_t*)c.data(), (const uint64_t*)roots.data(), c.size(), 2), "csh_vec_mul_table");
  }
  static ArithmeticHalfShare to_half_share(const ArithmeticShare& a) { return a.a; }  // mpc/rep3.rs:120-122
  template <class F>
  static Proj<F> msm_public_points_hs(const BasesView& pts, const std::vector<ArithmeticHalfShare>& s) {  // mpc/rep3.rs:124-132
    return msm_device<F>(pts, s.data(), s.size());
  }
  template <class F>
  static Proj<F> msm_public_points_hs(const BasesView& pts, const DeviceScalars& s) {  // same MSM, scalars already in HBM
    return msm_device_resident<F>(pts, s);
  }
  template <class F>
  static Proj<F> scalar_mul_public_point_hs(const Proj<F>& a, const ArithmeticHalfShare& b) { return point_mul(a, b); }
  template <class F>
  static void add_assign_points_public_hs(int id, Proj<F>& a, const Proj<F>& b) {  // mpc/rep3.rs:108-118
    if (id == 0) a = point_add(a, b);
  }
  template <class F>
  static Proj<F> open_half_point(const Proj<F>& a, const Net* net, State&) {  // rep3/pointshare.rs:152-155
    AffineT<F> mine = into_affine(a);
    auto [pb, pc] = net->broadcast(mine);
    return point_add(point_add(a, into_group(pb)), into_group(pc));
  }
  template <class F>
  static Proj<F> scalar_mul(const Proj<F>& a, const ArithmeticShare& b, const Net* net, State& st) {  // mpc/rep3.rs:152-161
    AffineT<F> mine = into_affine(a);
    Proj<F> a_hs = into_group(net->reshare(mine));
    // b * point: rhs.a*self.a + rhs.b*self.a + rhs.a*self.b (rep3/pointshare/ops.rs:95-102) + masking_ec_element
    Proj<F> r = point_add(point_add(point_mul(a, b.a), point_mul(a_hs, b.a)), point_mul(a, b.b));
    // + masking_ec_element = C::rand(rng1) - C::rand(rng2) (rngs.rs:177-187, pointshare.rs:124): re-randomises the half share
    // before it is opened. A uniform group element per stream = a uniform multiple of the generator: (m1 - m2) * G, the three
    // parties' masks summing to the identity exactly as the reference's do.
    auto [m1, m2] = st.rand.template random_fes<Fr>();
    AffineT<F> gen;
    static_assert(sizeof(gen) == sizeof(AffineT<typename P::Fq>), "scalar_mul is only used on G1 (mpc.rs:131-137)");
    memcpy(&gen, P::g1_generator_words(), sizeof gen);
    return point_add(r, point_mul(into_group(gen), Fr::sub(m1, m2)));
  }
};

// ================================= Shamir (mpc-core/src/protocols/shamir*.rs) =================================
// lagrange_from_coeff (shamir.rs:442-460)
template <class Fr>
inline std::vector<Fr> lagrange_from_coeff(const std::vector<size_t>& coeffs) {
  std::vector<Fr> res;
  for (size_t i : coeffs) {
    Fr num = Fr::one(), den = Fr::one();
    const Fr fi = Fr::from_u64(i);
    for (size_t j : coeffs)
      if (i != j) {
        const Fr fj = Fr::from_u64(j);
        num = Fr::mul(num, fj);
        den = Fr::mul(den, Fr::sub(fj, fi));
      }
    res.push_back(Fr::mul(num, Fr::inv(den)));
  }
  return res;
}

template <class Fr>
struct ShamirState {
  int id = 0;
  size_t num_parties = 0, threshold = 0;
  std::vector<Fr> open_lagrange_t, open_lagrange_2t, mul_lagrange_2t;
  std::vector<Fr> mul_reconstruct_with_zeros;       // q(X): q(0) = 1, q(j) = 0 for j in num_non_zero+1..n
  std::deque<std::pair<Fr, Fr>> rng_buffer;         // (r_t, r_2t) double sharings (shamir/rngs.rs:12-60; dealt here)
  // From<ShamirPreprocessing> (shamir.rs:66-103)
  static ShamirState create(int id, size_t n, size_t t, std::deque<std::pair<Fr, Fr>> pairs) {
    ShamirState s;
    s.id = id;
    s.num_parties = n;
    s.threshold = t;
    auto ring = [&](size_t cnt) {
      std::vector<size_t> c;
      for (size_t i = 0; i < cnt; ++i) c.push_back((id + n - i) % n + 1);
      return c;
    };
    s.open_lagrange_t = lagrange_from_coeff<Fr>(ring(t + 1));
    s.open_lagrange_2t = lagrange_from_coeff<Fr>(ring(2 * t + 1));
    std::vector<size_t> first;
    for (size_t i = 1; i <= 2 * t + 1; ++i) first.push_back(i);
    s.mul_lagrange_2t = lagrange_from_coeff<Fr>(first);
    // interpolation_poly_from_zero_points (shamir.rs:568-586)
    const size_t num_non_zero = n - t;
    std::vector<Fr> num{Fr::one()};
    Fr d = Fr::one();
    for (size_t j = num_non_zero + 1; j <= n; ++j) {
      const Fr fj = Fr::from_u64(j);
      num.insert(num.begin(), Fr::zero());  // poly_times_root_inplace: num = num * (X - j)
      for (size_t k = 1; k < num.size(); ++k) num[k - 1] = Fr::sub(num[k - 1], Fr::mul(num[k], fj));
      d = Fr::mul(d, Fr::neg(fj));
    }
    const Fr c = Fr::inv(d);
    for (auto& x : num) x = Fr::mul(x, c);
    s.mul_reconstruct_with_zeros = num;
    s.rng_buffer = std::move(pairs);
    return s;
  }
  ShamirState fork(size_t amount) {  // ShamirState::fork: hands `amount` pairs to the forked state
    ShamirState s = *this;
    s.rng_buffer.clear();
    for (size_t i = 0; i < amount; ++i) {
      s.rng_buffer.push_back(rng_buffer.back());
      rng_buffer.pop_back();
    }
    return s;
  }
  std::pair<Fr, Fr> get_pair() {
    if (rng_buffer.empty()) throw Error("Shamir: out of preprocessed double sharings");
    auto p = rng_buffer.front();
    rng_buffer.pop_front();
    return p;
  }
};

template <class P>
struct ShamirGroth16Driver {
  using Fr = typename P::Fr;
  using ArithmeticShare = Fr;        // ShamirPrimeFieldShare is repr(transparent)
  using ArithmeticHalfShare = Fr;    // degree-2t sharing
  using State = ShamirState<Fr>;
  using Net = LocalNetwork;
  static constexpr int PROTOCOL = 0;
  static constexpr uint32_t NCOMP = 1;
  static constexpr bool DEVICE_MASKS = false;

  static ArithmeticShare rand(const Net*, State& st) { return st.get_pair().first; }  // ShamirState::rand: the degree-t half of a pair
  static ArithmeticShare evaluate_constraint(int, const std::vector<std::pair<Fr, size_t>>& lhs, const std::vector<Fr>& pub,
                                             const std::vector<ArithmeticShare>& wit) {  // mpc/shamir.rs:29-49: public values add to every share
    return PlainGroth16Driver<P>::evaluate_constraint(0, lhs, pub, wit);
  }
  static std::vector<ArithmeticShare> promote_to_trivial_shares(int, const std::vector<Fr>& v) { return v; }  // shamir/arithmetic.rs:229-231
  static UninitBuf<Fr> masks(State&, size_t) { return {}; }
  static std::vector<Fr> local_mul_vec(const std::vector<Fr>& a, const std::vector<Fr>& b, State&) {  // shamir/arithmetic.rs:73-79
    std::vector<Fr> out(a.size());
    check(csh_vec_mul(P::ID, (const uint64_t*)a.data(), (const uint64_t*)b.data(), (uint64_t*)out.data(), a.size()), "csh_vec_mul");
    return out;
  }
  static void distribute_powers_and_mul_by_const(std::vector<ArithmeticShare>& c, const std::vector<Fr>& roots) {  // mpc/shamir.rs:85-96
    check(csh_vec_mul_table(P::ID, (uint64_t*)c.data(), (const uint64_t*)roots.data(), c.size(), 1), "csh_vec_mul_table");
  }
  static ArithmeticHalfShare to_half_share(const ArithmeticShare& a) { return a; }  // mpc/shamir.rs:107-109
  template <class F>
  static Proj<F> msm_public_points_hs(const BasesView& pts, const std::vector<ArithmeticHalfShare>& s) {  // mpc/shamir.rs:111-119
    return msm_device<F>(pts, s.data(), s.size());
  }
  template <class F>
  static Proj<F> msm_public_points_hs(const BasesView& pts, const DeviceScalars& s) { return msm_device_resident<F>(pts, s); }
  template <class F>
  static Proj<F> scalar_mul_public_point_hs(const Proj<F>& a, const ArithmeticHalfShare& b) { return point_mul(a, b); }
  template <class F>
  static void add_assign_points_public_hs(int, Proj<F>& a, const Proj<F>& b) { a = point_add(a, b); }  // mpc/shamir.rs:98-105
  // shamir/pointshare.rs:102-110 + network.rs:96-126 broadcast_next(n, 2t+1)
  template <class F>
  static Proj<F> open_half_point(const Proj<F>& a, const Net* net, State& st) {
    const size_t n = st.num_parties, num = 2 * st.threshold + 1;
    AffineT<F> mine = into_affine(a);
    Bytes b(sizeof mine);
    memcpy(b.data(), &mine, sizeof mine);
    for (size_t s = 1; s < num; ++s) net->send((int)((st.id + s) % n), b);
    Proj<F> res = point_mul(a, st.open_lagrange_2t[0]);
    for (size_t r = 1; r < num; ++r) {
      Bytes rb = net->recv((int)((st.id + n - r) % n));
      AffineT<F> o;
      memcpy(&o, rb.data(), sizeof o);
      res = point_add(res, point_mul(into_group(o), st.open_lagrange_2t[r]));
    }
    return res;
  }
  // mpc/shamir.rs:139-147: degree_reduce_point (shamir/network.rs:246-309, king = party 0) then (b * a).a
  template <class F>
  static Proj<F> scalar_mul(const Proj<F>& a, const ArithmeticShare& b, const Net* net, State& st, const AffineT<F>& generator) {
    const size_t n = st.num_parties, t = st.threshold, num_non_zero = n - t;
    auto [r_t, r_2t] = st.get_pair();
    const Proj<F> g = into_group(generator);
    Proj<F> input = point_add(a, point_mul(g, r_2t));
    Proj<F> my_share = Proj<F>::inf();
    auto send_pt = [&](int to, const Proj<F>& p) {
      AffineT<F> af = into_affine(p);
      Bytes bb(sizeof af);
      memcpy(bb.data(), &af, sizeof af);
      net->send(to, std::move(bb));
    };
    auto recv_pt = [&](int from) {
      Bytes rb = net->recv(from);
      AffineT<F> o;
      memcpy(&o, rb.data(), sizeof o);
      return into_group(o);
    };
    if (st.id == 0) {
      Proj<F> acc = point_mul(input, st.mul_lagrange_2t[0]);
      for (size_t other = 1; other < st.mul_lagrange_2t.size(); ++other) acc = point_add(acc, point_mul(recv_pt((int)other), st.mul_lagrange_2t[other]));
      for (size_t id = 0; id < num_non_zero; ++id) {
        // evaluate acc * q(X) at X = id + 1 (poly_with_zeros_from_precomputed_point + evaluate_poly_point)
        Fr x = Fr::from_u64(id + 1), e = Fr::zero();
        for (size_t k = st.mul_reconstruct_with_zeros.size(); k-- > 0;) e = Fr::add(Fr::mul(e, x), st.mul_reconstruct_with_zeros[k]);
        Proj<F> val = point_mul(acc, e);
        if (id == 0) my_share = val;
        else send_pt((int)id, val);
      }
    } else {
      if ((size_t)st.id <= 2 * t) send_pt(0, input);
      if ((size_t)st.id < num_non_zero) my_share = recv_pt(0);
    }
    Proj<F> reduced = point_add(my_share, point_neg(point_mul(g, r_t)));
    return point_mul(reduced, b);  // scalar_mul_local (shamir/pointshare.rs:97-99)
  }
};

// ================================= Poseidon2 (mpc-core/src/gadgets/poseidon2, gadgets/merkle_tree) =================================
// One party of a Poseidon2 computation: what arithmetic::rand, arithmetic::mul_vec and arithmetic::open_vec are for it. A share vector is a
// flat vector of NCOMP field elements per share, the layout of the device entries (Rep3: a, b interleaved, which is Rep3PrimeFieldShare).
//   PROTOCOL, NCOMP, party()   the protocol, ncomp and party_id of the device entries
//   rand_vec(n)                n fresh random shares
//   mul_vec(a, b)              shares of the products: the local multiplication on the device and the party's network round
//   open_vec(x)                the opened values, one element per share
// Plain: one party holding the values themselves (the Poseidon2 of poseidon2_permutation.rs run through the same rounds).
template <class P>
struct Poseidon2PlainParty {
  using Fr = typename P::Fr;
  static constexpr uint32_t PROTOCOL = 0, NCOMP = 1;
  ChaCha12 rng;  // the caller's key
  explicit Poseidon2PlainParty(const uint8_t seed[32]) : rng(seed) {}
  uint32_t party() const { return 0; }
  std::vector<Fr> rand_vec(size_t n) {
    std::vector<Fr> r(n);
    for (auto& x : r) {
      uint8_t b[32];
      rng.fill_bytes(b, 32);
      x = from_be_bytes_mod_order<Fr>(b);
    }
    return r;
  }
  std::vector<Fr> mul_vec(const std::vector<Fr>& a, const std::vector<Fr>& b) {
    UnitState st;
    return PlainGroth16Driver<P>::local_mul_vec(a, b, st);
  }
  std::vector<Fr> open_vec(const std::vector<Fr>& x) { return x; }
};

// Rep3 (rep3/arithmetic.rs): rand :357-360, mul_vec :148-161 (local_mul_vec + reshare), open_vec :249-271
template <class P>
struct Poseidon2Rep3Party {
  using Fr = typename P::Fr;
  static constexpr uint32_t PROTOCOL = 1, NCOMP = 2;
  const LocalNetwork& net;
  Rep3State& st;
  uint32_t party() const { return (uint32_t)st.id; }
  std::vector<Fr> rand_vec(size_t n) {
    std::vector<Fr> r(2 * n);
    for (size_t i = 0; i < n; ++i) {
      auto [a, b] = st.rand.template random_fes<Fr>();
      r[2 * i] = a, r[2 * i + 1] = b;
    }
    return r;
  }
  std::vector<Fr> exchange(const std::vector<Fr>& mine) {  // reshare_many: to the next party, from the previous one
    const size_t bytes = sizeof(Fr) * mine.size();
    Bytes b(bytes);
    if (bytes) memcpy(b.data(), mine.data(), bytes);
    net.send((net.id() + 1) % 3, std::move(b));
    const Bytes r = net.recv((net.id() + 2) % 3);
    if (r.size() != bytes) throw Error("Poseidon2Rep3Party: invalid number of elements received");
    std::vector<Fr> prev(mine.size());
    if (bytes) memcpy((void*)prev.data(), r.data(), bytes);
    return prev;
  }
  std::vector<Fr> mul_vec(const std::vector<Fr>& a, const std::vector<Fr>& b) {
    const size_t n = a.size() / 2;
    const UninitBuf<Fr> mask = st.rand.template masking_field_elements_vec<Fr>(n);
    std::vector<Fr> half(n);
    check(csh_rep3_local_mul_vec(P::ID, (const uint64_t*)a.data(), (const uint64_t*)b.data(), (const uint64_t*)mask.data(), (uint64_t*)half.data(), n),
          "csh_rep3_local_mul_vec");
    const std::vector<Fr> prev = exchange(half);
    std::vector<Fr> out(2 * n);
    for (size_t i = 0; i < n; ++i) out[2 * i] = half[i], out[2 * i + 1] = prev[i];
    return out;
  }
  std::vector<Fr> open_vec(const std::vector<Fr>& x) {
    const size_t n = x.size() / 2;
    std::vector<Fr> bs(n);
    for (size_t i = 0; i < n; ++i) bs[i] = x[2 * i + 1];
    const std::vector<Fr> cs = exchange(bs);
    std::vector<Fr> y(n);
    for (size_t i = 0; i < n; ++i) y[i] = Fr::add(Fr::add(x[2 * i], x[2 * i + 1]), cs[i]);
    return y;
  }
};

// Shamir (shamir/arithmetic.rs): rand = the degree-t half of a double sharing, mul_vec :81-94 (local products + degree_reduce_many,
// shamir/network.rs:150-241, king = party 0), open_vec :233-247 (broadcast_next(n, t + 1), network.rs:96-126, and open_lagrange_t)
template <class P>
struct Poseidon2ShamirParty {
  using Fr = typename P::Fr;
  static constexpr uint32_t PROTOCOL = 0, NCOMP = 1;
  const LocalNetwork& net;
  ShamirState<Fr>& st;
  uint32_t party() const { return (uint32_t)st.id; }
  std::vector<Fr> rand_vec(size_t n) {
    std::vector<Fr> r(n);
    for (auto& x : r) x = st.get_pair().first;
    return r;
  }
  static Bytes pack(const std::vector<Fr>& v) {
    Bytes b(sizeof(Fr) * v.size());
    if (!v.empty()) memcpy(b.data(), v.data(), b.size());
    return b;
  }
  std::vector<Fr> recv_many(int from, size_t len) {
    const Bytes r = net.recv(from);
    if (r.size() != sizeof(Fr) * len) throw Error("Poseidon2ShamirParty: invalid number of elements received");
    std::vector<Fr> v(len);
    if (len) memcpy((void*)v.data(), r.data(), r.size());
    return v;
  }
  std::vector<Fr> mul_vec(const std::vector<Fr>& a, const std::vector<Fr>& b) {
    const size_t n = st.num_parties, t = st.threshold, num_non_zero = n - t, len = a.size();
    std::vector<Fr> in(len), r_ts(len);
    check(csh_vec_mul(P::ID, (const uint64_t*)a.data(), (const uint64_t*)b.data(), (uint64_t*)in.data(), len), "csh_vec_mul");
    for (size_t i = 0; i < len; ++i) {
      auto [r_t, r_2t] = st.get_pair();
      in[i] = Fr::add(in[i], r_2t);
      r_ts[i] = r_t;
    }
    std::vector<Fr> mine(len, Fr::zero());
    if (st.id == 0) {
      std::vector<std::vector<Fr>> got{in};
      for (size_t other = 1; other < st.mul_lagrange_2t.size(); ++other) got.push_back(recv_many((int)other, len));
      std::vector<const uint64_t*> parts;
      for (auto& g : got) parts.push_back((const uint64_t*)g.data());
      std::vector<Fr> acc(len);
      check(csh_lincomb(P::ID, parts.data(), (const uint64_t*)st.mul_lagrange_2t.data(), parts.size(), (uint64_t*)acc.data(), len), "csh_lincomb");
      for (size_t id = 0; id < num_non_zero; ++id) {  // acc * q(X) at X = id + 1: q(0) = 1 and the last t parties' shares are zero
        Fr x = Fr::from_u64(id + 1), e = Fr::zero();
        for (size_t k = st.mul_reconstruct_with_zeros.size(); k-- > 0;) e = Fr::add(Fr::mul(e, x), st.mul_reconstruct_with_zeros[k]);
        std::vector<Fr> vals(len);
        for (size_t i = 0; i < len; ++i) vals[i] = Fr::mul(acc[i], e);
        if (id == 0) mine = std::move(vals);
        else net.send((int)id, pack(vals));
      }
    } else {
      if ((size_t)st.id <= 2 * t) net.send(0, pack(in));
      if ((size_t)st.id < num_non_zero) mine = recv_many(0, len);
    }
    for (size_t i = 0; i < len; ++i) mine[i] = Fr::sub(mine[i], r_ts[i]);
    return mine;
  }
  std::vector<Fr> open_vec(const std::vector<Fr>& x) {
    const size_t n = st.num_parties, num = st.threshold + 1;
    for (size_t s = 1; s < num; ++s) net.send((int)((st.id + s) % n), pack(x));
    std::vector<std::vector<Fr>> got;
    for (size_t r = 1; r < num; ++r) got.push_back(recv_many((int)((st.id + n - r) % n), x.size()));
    std::vector<const uint64_t*> parts{(const uint64_t*)x.data()};
    for (auto& g : got) parts.push_back((const uint64_t*)g.data());
    std::vector<Fr> y(x.size());
    check(csh_lincomb(P::ID, parts.data(), (const uint64_t*)st.open_lagrange_t.data(), num, (uint64_t*)y.data(), y.size()), "csh_lincomb");
    return y;
  }
};

// ShamirPreprocessing (shamir.rs:26-64) with ShamirRng (shamir/rngs.rs) on the device: the shared streams, the public matrices and the
// buffers r_t / r_2t live in a csh_shamir_rng_t; this struct is the network around it -- get_shared_rngs (rngs.rs:98-139: same send /
// receive split, same seed order), the one exchange of random_double_share (rngs.rs:387-392) and fork_with_pairs (rngs.rs:74-96). The
// reference seeds the party's own generator from the operating system (RngType::from_entropy, shamir.rs:45); here the caller passes the
// 32 bytes. Stream positions are counted in 32-byte candidates (csh_field_rand_dev): a seed draw is one of them.
template <class P>
struct ShamirPreprocessingHip {
  using Fr = typename P::Fr;
  int id = 0;
  size_t num_parties = 0, threshold = 0;
  uint8_t rng_seed[32] = {0};  // the party's own generator (only ever draws seeds)
  uint64_t rng_pos = 0;
  csh_shamir_rng_t handle = nullptr;
  std::deque<std::pair<Fr, Fr>> inherited;  // a fork's pairs: the parent's drain(..amount), in front of whatever the fork generates itself

  ShamirPreprocessingHip() = default;
  ShamirPreprocessingHip(const ShamirPreprocessingHip&) = delete;
  ShamirPreprocessingHip& operator=(const ShamirPreprocessingHip&) = delete;
  ShamirPreprocessingHip(ShamirPreprocessingHip&& o) noexcept { *this = std::move(o); }
  ShamirPreprocessingHip& operator=(ShamirPreprocessingHip&& o) noexcept {
    if (this != &o) {
      csh_shamir_rng_destroy(handle);
      id = o.id, num_parties = o.num_parties, threshold = o.threshold, rng_pos = o.rng_pos, handle = o.handle;
      memcpy(rng_seed, o.rng_seed, 32);
      inherited = std::move(o.inherited);
      o.handle = nullptr;
    }
    return *this;
  }
  ~ShamirPreprocessingHip() { csh_shamir_rng_destroy(handle); }

  struct Dev {  // csh_malloc / csh_free
    void* p = nullptr;
    explicit Dev(size_t bytes) { check(csh_malloc(&p, bytes ? bytes : 1), "csh_malloc"); }
    Dev(const Dev&) = delete;
    Dev& operator=(const Dev&) = delete;
    ~Dev() { csh_free(p); }
    uint64_t* w() const { return (uint64_t*)p; }
  };
  // rng.gen::<[u8; 32]>() at candidate `pos` of ChaCha12Rng::from_seed(seed)
  static void gen_seed(const uint8_t seed[32], uint64_t& pos, uint8_t out[32]) {
    ChaCha12 c(seed);
    c.counter = pos >> 1;
    uint8_t blk[64];
    c.fill_bytes(blk, 64);
    memcpy(out, blk + 32 * (pos & 1), 32);
    ++pos;
  }
  size_t sending() const { return (num_parties - threshold - 2) + (num_parties - 2 * threshold - 1); }

  // ShamirPreprocessing::new: `amount` pairs at least (amount.div_ceil(t + 1) batch items of t + 1 pairs)
  static ShamirPreprocessingHip create(const LocalNetwork& net, size_t num_parties, size_t threshold, size_t amount, const uint8_t seed[32]) {
    if (2 * threshold + 1 > num_parties) throw Error("Threshold too large for number of parties");
    ShamirPreprocessingHip s;
    s.id = net.id(), s.num_parties = num_parties, s.threshold = threshold;
    memcpy(s.rng_seed, seed, 32);
    // get_shared_rngs
    const size_t n = num_parties, id = (size_t)s.id, interact = n - 1;
    std::vector<uint8_t> seeds(32 * n, 0);
    size_t send = interact / 2;
    if ((interact & 1) == 1 && id < n / 2) send += 1;
    const size_t receive = interact - send;
    for (size_t off = 1; off <= send; ++off) {
      const size_t rcv_id = (id + off) % n;
      gen_seed(s.rng_seed, s.rng_pos, &seeds[32 * rcv_id]);
      net.send((int)rcv_id, Bytes(seeds.begin() + 32 * rcv_id, seeds.begin() + 32 * rcv_id + 32));
    }
    for (size_t off = 1; off <= receive; ++off) {
      const size_t send_id = (id + n - off) % n;
      const Bytes b = net.recv((int)send_id);
      if (b.size() != 32) throw Error("get_shared_rngs: a seed is 32 bytes");
      memcpy(&seeds[32 * send_id], b.data(), 32);
    }
    seeds.erase(seeds.begin() + 32 * id, seeds.begin() + 32 * id + 32);  // seeds.split_off(id), skip(1)
    check(csh_shamir_rng_create(P::ID, (uint32_t)id, (uint32_t)n, (uint32_t)threshold, seeds.data(), nullptr, &s.handle), "csh_shamir_rng_create");
    if (amount) s.buffer_triples(net, (amount + threshold) / (threshold + 1));
    return s;
  }
  // buffer_triples (rngs.rs:401-428): `amount` batch items, (t + 1) pairs each
  void buffer_triples(const LocalNetwork& net, size_t amount) {
    const size_t n = num_parties, t = threshold, k = sending();
    Dev wire(sizeof(Fr) * k * amount);
    check(csh_shamir_double_share_local_dev(handle, amount, k ? wire.w() : nullptr, nullptr), "csh_shamir_double_share_local_dev");
    if (k) {
      std::vector<uint8_t> host(sizeof(Fr) * k * amount);
      check(csh_memcpy_d2h(host.data(), wire.p, host.size()), "csh_memcpy_d2h");
      const size_t per = sizeof(Fr) * amount;
      size_t q = 0;
      for (size_t i = 1; i <= n - t - 2; ++i, ++q) net.send((int)((id + i + t + 1) % n), Bytes(host.begin() + q * per, host.begin() + (q + 1) * per));
      for (size_t i = 1; i <= n - 2 * t - 1; ++i, ++q) net.send((int)((id + i + 2 * t) % n), Bytes(host.begin() + q * per, host.begin() + (q + 1) * per));
      q = 0;
      auto take = [&](size_t from) {
        const Bytes b = net.recv((int)from);
        if (b.size() != per) throw Error("random_double_share: invalid number of elements received");
        memcpy(host.data() + q++ * per, b.data(), per);
      };
      for (size_t i = 1; i <= n - t - 2; ++i) take((id + n - (t + 1) - i) % n);
      for (size_t i = 1; i <= n - 2 * t - 1; ++i) take((id + n - 2 * t - i) % n);
      check(csh_memcpy_h2d(wire.p, host.data(), host.size()), "csh_memcpy_h2d");
    }
    check(csh_shamir_double_share_finish_dev(handle, amount, k ? wire.w() : nullptr, nullptr), "csh_shamir_double_share_finish_dev");
  }
  size_t len() const {
    size_t l = 0;
    check(csh_shamir_pairs_len(handle, &l), "csh_shamir_pairs_len");
    return inherited.size() + l;
  }
  // `count` pairs off the front of the device buffers, in buffer order
  std::deque<std::pair<Fr, Fr>> drain(size_t count) {
    Dev a(sizeof(Fr) * count), b(sizeof(Fr) * count);
    check(csh_shamir_pairs_take_dev(handle, count, 1, a.w(), b.w(), nullptr), "csh_shamir_pairs_take_dev");
    std::vector<Fr> r_t(count), r_2t(count);
    if (count) {
      check(csh_memcpy_d2h(r_t.data(), a.p, sizeof(Fr) * count), "csh_memcpy_d2h");
      check(csh_memcpy_d2h(r_2t.data(), b.p, sizeof(Fr) * count), "csh_memcpy_d2h");
    }
    std::deque<std::pair<Fr, Fr>> out;
    for (size_t i = 0; i < count; ++i) out.push_back({r_t[i], r_2t[i]});
    return out;
  }
  // From<ShamirPreprocessing> for ShamirState (shamir.rs:66-103): every pair, in buffer order, into the host state the drivers consume
  ShamirState<Fr> into_state() {
    size_t l = 0;
    check(csh_shamir_pairs_len(handle, &l), "csh_shamir_pairs_len");
    std::deque<std::pair<Fr, Fr>> pairs = std::move(inherited);
    inherited.clear();
    for (auto& pr : drain(l)) pairs.push_back(pr);
    return ShamirState<Fr>::create(id, num_parties, threshold, std::move(pairs));
  }
  // fork_with_pairs (rngs.rs:74-96): the own generator's seed draw first, then one per shared stream; the first `amount` pairs move
  ShamirPreprocessingHip fork(size_t amount) {
    ShamirPreprocessingHip c;
    c.id = id, c.num_parties = num_parties, c.threshold = threshold;
    gen_seed(rng_seed, rng_pos, c.rng_seed);
    std::vector<uint8_t> seeds(32 * (num_parties - 1));
    check(csh_shamir_rng_fork_seeds(handle, seeds.data()), "csh_shamir_rng_fork_seeds");
    if (amount > len()) throw Error("not enough corr rand pairs");
    check(csh_shamir_rng_create(P::ID, (uint32_t)id, (uint32_t)num_parties, (uint32_t)threshold, seeds.data(), nullptr, &c.handle), "csh_shamir_rng_create");
    while (amount && !inherited.empty()) c.inherited.push_back(inherited.front()), inherited.pop_front(), --amount;
    for (auto& pr : drain(amount)) c.inherited.push_back(pr);
    return c;
  }
};

// Poseidon2<F, T, 5> over the device entries (csrc/poseidon2.hip): the caller's parameter set (the fields of Poseidon2Params) is uploaded once;
// the methods carry the reference's names. The collaborative ones take a party (above) and run every stretch of local arithmetic between two
// openings as one csh_poseidon2_co_round_dev; state and precomputation stay on the device, the shares to open and the opened values cross.
template <class P>
struct Poseidon2Hip {
  using Fr = typename P::Fr;
  static constexpr uint32_t SPONGE = 0, COMPRESSION = 1;
  struct Precomputations {  // Poseidon2Precomputations (poseidon2/mod.rs): five share vectors and the offset the next round reads at
    std::vector<Fr> r, r2, r3, r4, r5;
    size_t offset = 0;
  };
  struct Dev {  // csh_malloc / csh_free
    void* p = nullptr;
    explicit Dev(size_t bytes) { check(csh_malloc(&p, bytes ? bytes : 1), "csh_malloc"); }
    explicit Dev(const std::vector<Fr>& v) : Dev(sizeof(Fr) * v.size()) {
      if (!v.empty()) check(csh_memcpy_h2d(p, v.data(), sizeof(Fr) * v.size()), "csh_memcpy_h2d");
    }
    Dev(const Dev&) = delete;
    Dev& operator=(const Dev&) = delete;
    ~Dev() { csh_free(p); }
    uint64_t* w() const { return (uint64_t*)p; }
    std::vector<Fr> down(size_t count) const {
      std::vector<Fr> v(count);
      if (count) check(csh_memcpy_d2h(v.data(), p, sizeof(Fr) * count), "csh_memcpy_d2h");
      return v;
    }
  };

  const uint32_t t, rounds_f_beginning, rounds_f_end, rounds_p;
  const std::vector<Fr> rc_external, rc_internal, diag_m_1;  // the host's copy, for permutation_in_place
  csh_poseidon2_params_t handle = nullptr;

  Poseidon2Hip(uint32_t t_, uint32_t rf_b, uint32_t rf_e, uint32_t rp, const std::vector<Fr>& round_constants_external,
               const std::vector<Fr>& round_constants_internal, const std::vector<Fr>& mat_internal_diag_m_1)
      : t(t_), rounds_f_beginning(rf_b), rounds_f_end(rf_e), rounds_p(rp), rc_external(round_constants_external),
        rc_internal(round_constants_internal), diag_m_1(mat_internal_diag_m_1) {
    if (round_constants_external.size() != (size_t)(rf_b + rf_e) * t || round_constants_internal.size() != rp || mat_internal_diag_m_1.size() != t)
      throw Error("Poseidon2Hip: the constants do not have the lengths of the round numbers");
    check(csh_poseidon2_params_create(P::ID, t, rf_b, rf_e, rp, (const uint64_t*)round_constants_external.data(), (const uint64_t*)round_constants_internal.data(),
                                      (const uint64_t*)mat_internal_diag_m_1.data(), &handle), "csh_poseidon2_params_create");
  }
  Poseidon2Hip(const Poseidon2Hip&) = delete;
  Poseidon2Hip& operator=(const Poseidon2Hip&) = delete;
  ~Poseidon2Hip() { csh_poseidon2_params_destroy(handle); }

  size_t rounds() const { return (size_t)rounds_f_beginning + rounds_p + rounds_f_end; }
  size_t num_sbox() const { return (size_t)(rounds_f_beginning + rounds_f_end) * t + rounds_p; }  // poseidon2_permutation.rs:41-43
  bool is_external(size_t round) const { return round < rounds_f_beginning || round >= (size_t)rounds_f_beginning + rounds_p; }

  // The plain permutation of one state on the host, as the reference writes it (poseidon2_permutation.rs:67-214): what one thread of the
  // reference does per state, the baseline the device batch is measured against (tools/poseidon2_probe.py). Not a fall-back of anything.
  void matmul_external_host(Fr* s) const {
    if (t == 4) {  // matmul_m4, :67-80
      const Fr t0 = Fr::add(s[0], s[1]), t1 = Fr::add(s[2], s[3]);
      const Fr t2 = Fr::add(Fr::add(s[1], s[1]), t1), t3 = Fr::add(Fr::add(s[3], s[3]), t0);
      Fr t4 = Fr::add(t1, t1), t5 = Fr::add(t0, t0);
      t4 = Fr::add(Fr::add(t4, t4), t3), t5 = Fr::add(Fr::add(t5, t5), t2);
      s[0] = Fr::add(t3, t5), s[1] = t5, s[2] = Fr::add(t2, t4), s[3] = t4;
      return;
    }
    Fr sum = s[0];
    for (uint32_t i = 1; i < t; ++i) sum = Fr::add(sum, s[i]);
    for (uint32_t i = 0; i < t; ++i) s[i] = Fr::add(s[i], sum);
  }
  void matmul_internal_host(Fr* s) const {  // :126-162
    Fr sum = s[0];
    for (uint32_t i = 1; i < t; ++i) sum = Fr::add(sum, s[i]);
    if (t == 4) {
      for (uint32_t i = 0; i < 4; ++i) s[i] = Fr::add(Fr::mul(s[i], diag_m_1[i]), sum);
      return;
    }
    s[t - 1] = Fr::add(s[t - 1], s[t - 1]);
    for (uint32_t i = 0; i < t; ++i) s[i] = Fr::add(s[i], sum);
  }
  static Fr sbox_host(const Fr& x) {
    const Fr x2 = Fr::mul(x, x);
    return Fr::mul(Fr::mul(x2, x2), x);
  }
  void permutation_in_place(Fr* s) const {
    matmul_external_host(s);
    const size_t R = rounds();
    for (size_t r = 0; r < R; ++r) {
      if (is_external(r)) {
        const Fr* rc = &rc_external[(r < rounds_f_beginning ? r : r - rounds_p) * t];
        for (uint32_t i = 0; i < t; ++i) s[i] = sbox_host(Fr::add(s[i], rc[i]));
        matmul_external_host(s);
      } else {
        s[0] = sbox_host(Fr::add(s[0], rc_internal[r - rounds_f_beginning]));
        matmul_internal_host(s);
      }
    }
  }

  // permutation_in_place over chunks_exact_mut(T) of plain states (poseidon2_permutation.rs:194-214), one launch
  std::vector<Fr> permutation_packed(const std::vector<Fr>& states) const {
    if (states.size() % t) throw Error("Poseidon2Hip: the state vector is no multiple of t");
    Dev d(states);
    check(csh_poseidon2_permute_dev(handle, d.w(), states.size() / t, d.w(), nullptr), "csh_poseidon2_permute_dev");
    return d.down(states.size());
  }
  // merkle_tree_sponge / merkle_tree_compression on plain leaves (merkle_tree/plain.rs:15-50, :113-155)
  Fr merkle_tree_plain(const std::vector<Fr>& leaves, uint32_t arity, uint32_t mode) const {
    Dev in(leaves), root(sizeof(Fr)), work(2 * sizeof(Fr) * (leaves.size() / (arity ? arity : 1)));
    check(csh_poseidon2_merkle_dev(handle, arity, mode, in.w(), leaves.size(), root.w(), work.w(), nullptr), "csh_poseidon2_merkle_dev");
    return root.down(1)[0];
  }
  Fr merkle_tree_sponge(const std::vector<Fr>& leaves, uint32_t arity) const { return merkle_tree_plain(leaves, arity, SPONGE); }
  Fr merkle_tree_compression(const std::vector<Fr>& leaves, uint32_t arity) const { return merkle_tree_plain(leaves, arity, COMPRESSION); }

  // precompute_rep3 / precompute_shamir (rep3.rs:12-51, shamir.rs:35-73): r, then r^2, r^4 and [r^3 | r^5] = [r | r] [r^2 | r^4] by three
  // multiplications, each the existing local product on the device and the party's network round
  template <class Party>
  Precomputations precompute(Party& party, size_t num_poseidon) const {
    const size_t n = num_sbox() * num_poseidon, w = Party::NCOMP * n;
    Precomputations pre;
    pre.r = party.rand_vec(n);
    pre.r2 = party.mul_vec(pre.r, pre.r);
    pre.r4 = party.mul_vec(pre.r2, pre.r2);
    std::vector<Fr> lhs(pre.r), rhs(pre.r2);
    lhs.insert(lhs.end(), pre.r.begin(), pre.r.end());
    rhs.insert(rhs.end(), pre.r4.begin(), pre.r4.end());
    pre.r3 = party.mul_vec(lhs, rhs);
    pre.r5.assign(pre.r3.begin() + w, pre.r3.end());
    pre.r3.resize(w);
    return pre;
  }

  // the five vectors of a precomputation on the device, in the order of csh_poseidon2_co_round_dev
  struct DevicePrecomputations {
    Dev r, r2, r3, r4, r5;
    const uint64_t* ptrs[5];
    explicit DevicePrecomputations(const Precomputations& pre) : r(pre.r), r2(pre.r2), r3(pre.r3), r4(pre.r4), r5(pre.r5), ptrs{r.w(), r2.w(), r3.w(), r4.w(), r5.w()} {}
  };
  // {rep3,shamir}_permutation_in_place_with_precomputation_packed (rep3.rs:612-648, shamir.rs:326-365) on n_perm states on the device:
  // R + 1 steps with an opening between two of them. ff_dev (may be NULL): the feed-forward of the compression tree.
  template <class Party>
  void permutation_on_device(Party& party, uint64_t* state_dev, size_t n_perm, const DevicePrecomputations& pre, size_t entries, size_t& offset,
                             uint64_t* ff_dev) const {
    if (offset + num_sbox() * n_perm > entries) throw Error("Poseidon2Hip: the precomputation is too short for these permutations");
    const size_t R = rounds();
    Dev open_dev(sizeof(Fr) * Party::NCOMP * n_perm * t), y_dev(sizeof(Fr) * n_perm * t);
    for (size_t s = 0; s <= R; ++s) {
      check(csh_poseidon2_co_round_dev(P::ID, Party::PROTOCOL, party.party(), handle, (uint32_t)s, state_dev, n_perm, s ? y_dev.w() : nullptr, pre.ptrs, offset,
                                       s < R ? open_dev.w() : nullptr, s == 0 ? ff_dev : nullptr, nullptr), "csh_poseidon2_co_round_dev");
      if (s == R) break;
      const size_t count = is_external(s) ? n_perm * t : n_perm;
      const std::vector<Fr> y = party.open_vec(open_dev.down(Party::NCOMP * count));
      if (y.size() != count) throw Error("Poseidon2Hip: open_vec returned a vector of another length");
      if (count) check(csh_memcpy_h2d(y_dev.p, y.data(), sizeof(Fr) * count), "csh_memcpy_h2d");
      offset += count;
    }
    check(csh_sync(nullptr), "csh_sync");  // the last step still reads y_dev
  }
  template <class Party>
  void permutation_in_place_with_precomputation_packed(Party& party, std::vector<Fr>& state, Precomputations& pre) const {
    if (state.size() % ((size_t)Party::NCOMP * t)) throw Error("Poseidon2Hip: the state vector is no multiple of t shares");
    const size_t n_perm = state.size() / Party::NCOMP / t;
    Dev st(state);
    const DevicePrecomputations dpre(pre);
    permutation_on_device(party, st.w(), n_perm, dpre, pre.r.size() / Party::NCOMP, pre.offset, nullptr);
    state = st.down(state.size());
  }

  // merkle_tree_sponge_rep3 / merkle_tree_compression_rep3 (merkle_tree/rep3.rs:10-56, :59-115) and their Shamir forms (merkle_tree/shamir.rs):
  // the precomputation for all (len - 1) / (arity - 1) hashes, then layer after layer; the gather between two layers is
  // csh_poseidon2_layer_next_dev, so no layer returns to the host. -> the root's share
  template <class Party>
  std::vector<Fr> merkle_tree_shared(Party& party, const std::vector<Fr>& leaves, uint32_t arity, uint32_t mode) const {
    constexpr size_t nc = Party::NCOMP;
    size_t len = leaves.size() / nc, pw = 1;
    while (arity >= 2 && pw < len && len % (pw * arity) == 0) pw *= arity;
    if (arity < 2 || len < arity || pw != len || (mode == SPONGE ? t <= arity : t < arity) || mode > COMPRESSION)
      throw Error("Poseidon2Hip: the number of leaves must be a power of the arity; sponge mode needs t > arity, compression t >= arity");
    Precomputations pre = precompute(party, (len - 1) / (arity - 1));
    const DevicePrecomputations dpre(pre);
    const size_t entries = pre.r.size() / nc;
    // the first layer's states: `arity` leaves and zeros after them (:25-33, :74-87; nothing is padded at t == arity)
    std::vector<Fr> first(nc * (len / arity) * t, Fr::zero());
    for (size_t i = 0; i < len / arity; ++i)
      for (size_t j = 0; j < arity * nc; ++j) first[nc * i * t + j] = leaves[nc * i * arity + j];
    Dev a(first), b(sizeof(Fr) * first.size()), ff(sizeof(Fr) * nc * (len / arity));
    Dev *cur = &a, *nxt = &b;
    while (len > 1) {
      len /= arity;
      permutation_on_device(party, cur->w(), len, dpre, entries, pre.offset, mode == COMPRESSION ? ff.w() : nullptr);
      check(csh_poseidon2_layer_next_dev(P::ID, nc, t, arity, mode, cur->w(), mode == COMPRESSION ? ff.w() : nullptr, nxt->w(), len, nullptr),
            "csh_poseidon2_layer_next_dev");
      std::swap(cur, nxt);
    }
    if (pre.offset != entries) throw Error("Poseidon2Hip: the tree did not use up its precomputation");
    return cur->down(nc);
  }
  template <class Party>
  std::vector<Fr> merkle_tree_sponge_shared(Party& party, const std::vector<Fr>& leaves, uint32_t arity) const { return merkle_tree_shared(party, leaves, arity, SPONGE); }
  template <class Party>
  std::vector<Fr> merkle_tree_compression_shared(Party& party, const std::vector<Fr>& leaves, uint32_t arity) const {
    return merkle_tree_shared(party, leaves, arity, COMPRESSION);
  }
};

}  // namespace cosnarks
