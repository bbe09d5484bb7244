// C entry points of the host mirror, benchmark part: the synthetic large circuit with a known-trapdoor-style key, as an object
// (cog16_synth_*: what bench.py's `--workload groth16_prove` times) and as the whole-run benches (cog16_bench_*).
#include <atomic>
#include <chrono>
#include <map>

#include "capi_common.hpp"

using namespace cosnarks;
using namespace cosnarks::capi;

namespace {

// ---- synthetic large circuit with a known-trapdoor-style key: every query point is
// k_i * G with k_i = splitmix64(seed + i) | 1, so A, B, C have closed-form discrete logs and are checked with
// three scalar multiplications instead of a pairing. Constraints: w[j+1] * w[j+2] = w[j+3].
template <class F>
void synth_query(csh_curve_t curve, csh_group_t group, uint64_t seed, size_t n, Query<F>& q, size_t lead = 0) {
  void* dev = nullptr;
  const size_t pb = sizeof(AffineT<F>);
  if (lead > n) lead = 0;
  check(csh_malloc(&dev, (lead + n) * pb), "csh_malloc");
  char* pts = static_cast<char*>(dev) + lead * pb;
  check(csh_util_generate_bases_dev(curve, group, seed, n, pts, nullptr), "csh_util_generate_bases_dev");
  check(csh_sync(nullptr), "csh_sync");
  int cur = 0;
  check(csh_current_device(&cur), "csh_current_device");
  if (lead) check(csh_memcpy_peer(dev, cur, pts, cur, lead * pb, nullptr), "csh_memcpy_peer");  // Query::lead: padding = the first points again
  check(csh_sync(nullptr), "csh_sync");
  check(csh_bases_upload_dev(curve, group, dev, lead + n, 0, nullptr, &q.dev), "csh_bases_upload_dev");
  q.len = n;
  q.lead = lead;
  q.host.resize(n < 4 ? n : 4);
  check(csh_memcpy_d2h(q.host.data(), pts, q.host.size() * sizeof(AffineT<F>)), "csh_memcpy_d2h");
  csh_free(dev);
}

// The synthetic circuit with its known-dlog proving key resident on the device: built once, proved many times (bench.py times
// K calls of prove() between barriers), checked against the closed form.
struct SynthBase {
  virtual ~SynthBase() = default;
  virtual void prove(bool want_h) = 0;
  virtual bool closed_form() = 0;
  ProveTimes phases;
  double key_ms = 0;
};
template <class P>
struct SynthCircuit : SynthBase {
  using T = PlainGroth16Driver<P>;
  using Fr = typename P::Fr;
  using Fq = typename P::Fq;
  using Fq2 = typename P::Fq2;
  static constexpr uint64_t SA = 0x1000000000ull, SB1 = 0x2000000000ull, SB2 = 0x3000000000ull, SL = 0x4000000000ull, SH = 0x5000000000ull;
  static constexpr uint64_t d_alpha = 0x1111, d_beta = 0x2222, d_delta = 0x3333;
  size_t domain, nc, n_vars;
  AffineT<Fq> g1;
  AffineT<Fq2> g2;
  ProvingKey<P> pk;
  ConstraintMatrices<P> m;
  std::vector<Fr> w, h;
  SharedWitness<P, Fr> sw;
  Fr r, s;
  UnitState st0, st1;
  Proof<P> proof;
  SynthCircuit(int log_domain, const uint32_t* g1_words, const uint32_t* g2_words) {
    domain = size_t(1) << log_domain;
    nc = domain - 2;
    n_vars = nc + 3;
    memcpy(&g1, g1_words, sizeof g1);
    memcpy(&g2, g2_words, sizeof g2);
    auto t0 = std::chrono::steady_clock::now();
    synth_query<Fq>(P::ID, CSH_G1, SA, n_vars, pk.a_query);
    synth_query<Fq>(P::ID, CSH_G1, SB1, n_vars, pk.b_g1_query);
    synth_query<Fq2>(P::ID, CSH_G2, SB2, n_vars, pk.b_g2_query);
    synth_query<Fq>(P::ID, CSH_G1, SL, n_vars - 2, pk.l_query, 2);
    synth_query<Fq>(P::ID, CSH_G1, SH, domain, pk.h_query);
    pk.build_tables();
    pk.place_default();
    auto kG1 = [&](uint64_t k) { return into_affine(point_mul(into_group(g1), Fr::from_u64(k))); };
    auto kG2 = [&](uint64_t k) { return into_affine(point_mul(into_group(g2), Fr::from_u64(k))); };
    pk.alpha_g1 = kG1(d_alpha);
    pk.beta_g1 = kG1(d_beta);
    pk.beta_g2 = kG2(d_beta);
    pk.delta_g1 = kG1(d_delta);
    pk.delta_g2 = kG2(d_delta);
    key_ms = ms_since(t0);
    m.num_instance_variables = 2;
    m.num_witness_variables = n_vars - 2;
    m.num_constraints = nc;
    m.a.resize(nc);
    m.b.resize(nc);
    const Fr one = Fr::one();
    for (size_t j = 0; j < nc; ++j) {
      m.a[j].push_back({one, j + 1});
      m.b[j].push_back({one, j + 2});
    }
    m.upload();
    w.resize(n_vars);
    w[0] = one;
    w[1] = Fr::from_u64(3);
    w[2] = Fr::from_u64(5);
    for (size_t j = 0; j < nc; ++j) w[j + 3] = Fr::mul(w[j + 1], w[j + 2]);
    sw.public_inputs.assign(w.begin(), w.begin() + 2);
    sw.witness.assign(w.begin() + 2, w.end());
    r = Fr::from_u64(123456789);
    s = Fr::from_u64(987654321);
  }
  // h is only fetched (for the closed-form check) when asked: a prover does not need it on the host
  void prove(bool want_h) override {
    proof = CoGroth16<P, T>::template prove_inner<CircomReduction>(nullptr, nullptr, st0, st1, pk, m, sw, &r, &s, want_h ? &h : nullptr);
    phases = last_prove_times();
  }
  static bool eq1(const AffineT<Fq>& x, const AffineT<Fq>& y) { return x.x == y.x && x.y == y.y; }
  bool closed_form() override {
    if (h.size() != domain) prove(true);
    auto dl = [](uint64_t seed, size_t i) { return Fr::from_u64(csh_util_splitmix64(seed + i) | 1ull); };
    Fr sa = Fr::zero(), sb1 = Fr::zero(), sb2 = Fr::zero(), sl = Fr::zero(), sh = Fr::zero();
    for (size_t i = 0; i < n_vars; ++i) {
      sa = Fr::add(sa, Fr::mul(w[i], dl(SA, i)));
      sb1 = Fr::add(sb1, Fr::mul(w[i], dl(SB1, i)));
      sb2 = Fr::add(sb2, Fr::mul(w[i], dl(SB2, i)));
    }
    for (size_t j = 0; j + 2 < n_vars; ++j) sl = Fr::add(sl, Fr::mul(w[j + 2], dl(SL, j)));
    for (size_t i = 0; i < domain; ++i) sh = Fr::add(sh, Fr::mul(h[i], dl(SH, i)));
    const Fr dd = Fr::from_u64(d_delta);
    Fr dA = Fr::add(Fr::add(Fr::mul(r, dd), Fr::from_u64(d_alpha)), sa);
    Fr dB1 = Fr::add(Fr::add(Fr::mul(s, dd), Fr::from_u64(d_beta)), sb1);
    Fr dB2 = Fr::add(Fr::add(Fr::mul(s, dd), Fr::from_u64(d_beta)), sb2);
    Fr dC = Fr::add(Fr::add(Fr::sub(Fr::add(Fr::mul(s, dA), Fr::mul(r, dB1)), Fr::mul(Fr::mul(r, s), dd)), sl), sh);
    AffineT<Fq> wa = into_affine(point_mul(into_group(g1), dA)), wc = into_affine(point_mul(into_group(g1), dC));
    AffineT<Fq2> wb = into_affine(point_mul(into_group(g2), dB2));
    return eq1(wa, proof.a) && eq1(wc, proof.c) && wb.x == proof.b.x && wb.y == proof.b.y;
  }
};

// median of a sample and the index of the element that realises it (the phases reported beside a median are those of THAT run)
static size_t median_index(const std::vector<double>& v) {
  std::vector<size_t> idx(v.size());
  for (size_t i = 0; i < idx.size(); ++i) idx[i] = i;
  std::sort(idx.begin(), idx.end(), [&](size_t x, size_t y) { return v[x] < v[y]; });
  return idx[idx.size() / 2];
}

// Every figure is the MEDIAN of `iters` runs after warm-up runs (median of >= 20; rounds 1-4 reported the minimum, which hid
// a 17.7 -> 40 ms spread on one box, profiles/archive/r04_zd_trait_modes.log); *_min entries keep the minimum beside it.
// rep3_trait_out (nullable, 2 x 13 doubles: [0..12] host masks = the shim's default, [13..25] seeded device masks = its opt-in
// all-GPU-parties mode): {three parties on this GPU: wall ms median, min; party 0 of the median run: mask draw, witness map (incl. masks),
// to_half_share, five MSMs, finish; proofs equal the plain proof (1 / 0); ONE party alone on the GPU, no peers (witness map + to_half_share
// + five MSMs, the finish's three curve points left out): ms median, mask draw, witness map, to_half_share, five MSMs}.
template <class P>
int bench_synth_t(int log_domain, int iters, double* out_ms, int* check_ok, const uint32_t* g1_words, const uint32_t* g2_words, bool with_rep3,
                  double* phases_out = nullptr, double* trait_out = nullptr, double* rep3_trait_out = nullptr, double* mins_out = nullptr) {
  using T = PlainGroth16Driver<P>;
  using Fr = typename P::Fr;
  using Fq = typename P::Fq;
  // COG16_LEAK_BENCH_CIRCUIT=1 (diagnostics, tools/experiments/trait_stall_probe.py): the circuit of this call is never destroyed, so none of
  // the host memory the runtime has copied from / to is unmapped while later calls run
  std::unique_ptr<SynthCircuit<P>> sc_owner(new SynthCircuit<P>(log_domain, g1_words, g2_words));
  SynthCircuit<P>& sc = *sc_owner;
  struct Leak {
    std::unique_ptr<SynthCircuit<P>>& o;
    ~Leak() {
      if (getenv("COG16_LEAK_BENCH_CIRCUIT")) (void)o.release();
    }
  } leak{sc_owner};
  ProvingKey<P>& pk = sc.pk;
  ConstraintMatrices<P>& m = sc.m;
  SharedWitness<P, Fr>& sw = sc.sw;
  const Fr r = sc.r, s = sc.s;
  out_ms[3] = sc.key_ms;
  std::vector<double> hs, totals;
  std::vector<ProveTimes> phs;
  for (int it = 0; it < iters + 2; ++it) {  // two warm-up rounds (streams, arenas and pooled buffers of the worker threads)
    auto a0 = std::chrono::steady_clock::now();
    std::vector<Fr> hh = CircomReduction::witness_map_from_matrices<P, T>(sc.st0, m, sw.public_inputs, sw.witness);
    auto a1 = std::chrono::steady_clock::now();
    sc.prove(it + 1 == iters + 2);
    const double total = ms_since(a1);
    if (it < 2) continue;
    hs.push_back(std::chrono::duration<double, std::milli>(a1 - a0).count());
    totals.push_back(total);
    phs.push_back(sc.phases);
  }
  const size_t mi = median_index(totals);
  out_ms[0] = hs[median_index(hs)];  // host-facing witness_map_from_matrices alone (witness up, device pipeline, h down)
  out_ms[1] = phs[mi].msm_ms;        // the five MSM groups of the median prove (create_proof_device up to the join), host clock
  out_ms[2] = totals[mi];            // Groth16 prove (prove_inner), key resident on the device
  if (mins_out) mins_out[0] = *std::min_element(totals.begin(), totals.end());
  if (phases_out) {
    phases_out[0] = phs[mi].witness_ms;  // witness upload + device-resident witness map inside that prove
    phases_out[1] = phs[mi].msm_ms;
    phases_out[2] = phs[mi].finish_ms;
  }
  *check_ok = sc.closed_form();
  if (trait_out) {
    // The same circuit, key and witness through the "trait path" (groth16.hpp): the sequence rust/co-groth16-hip drives behind the unchanged
    // reference -- one host-slice witness-map call, h on the host, five concurrent host-scalar MSMs. trait_out = {prove ms (median of iters),
    // witness map ms, five MSMs ms, finish ms (of that prove), closed-form check of the trait-path proof (1 / 0)}.
    struct Restore {
      int prev = trait_path_flag().exchange(1);
      ~Restore() { trait_path_flag().store(prev); }
    } restore;
    std::vector<double> tt;
    std::vector<ProveTimes> tp;
    for (int it = 0; it < iters + 2; ++it) {
      auto a1 = std::chrono::steady_clock::now();
      sc.prove(false);
      if (it < 2) continue;  // warm the lanes of the five MSM threads
      tt.push_back(ms_since(a1));
      tp.push_back(sc.phases);
    }
    sc.prove(true);
    const size_t ti = median_index(tt);
    trait_out[0] = tt[ti];
    trait_out[1] = tp[ti].witness_ms;
    trait_out[2] = tp[ti].msm_ms;
    trait_out[3] = tp[ti].finish_ms;
    trait_out[4] = sc.closed_form() ? 1.0 : 0.0;
    if (mins_out) mins_out[1] = *std::min_element(tt.begin(), tt.end());
  }
  const Proof<P>& proof = sc.proof;
  auto eq1 = [](const AffineT<Fq>& x, const AffineT<Fq>& y) { return x.x == y.x && x.y == y.y; };

  // BASELINE config 4 at scale: three in-process Rep3 parties prove the same circuit with the same r, s; they share this GPU (or take
  // one GPU each when the node has several, with key copies per device). Wall time of the whole three-party run; the agreed proof
  // must equal the plain one. Three ways to drive a party: the device-resident mirror (device ChaCha12 masks from the party's own keys --
  // reachable only with an upstream edit, the generators of Rep3Rand are private), and the two modes of the zero-upstream-edit trait path.
  out_ms[4] = 0;
  out_ms[5] = 0;
  if (with_rep3) {
    using T3 = Rep3Groth16Driver<P>;
    using Share = Rep3PrimeFieldShare<Fr>;
    FieldRng<Fr> sharer(99, /*domain=*/3);
    std::vector<Share> wsh[3];
    sharer.rep3(sw.witness, wsh);
    Share r3[3], s3[3];
    {
      std::vector<Share> t[3];
      sharer.rep3({r, s}, t);
      for (int p = 0; p < 3; ++p) {
        r3[p] = t[p][0];
        s3[p] = t[p][1];
      }
    }
    SharedWitness<P, Share> sw3[3];
    for (int p = 0; p < 3; ++p) {
      sw3[p].public_inputs = sw.public_inputs;
      sw3[p].witness = std::move(wsh[p]);
    }
    const int iters3 = iters < 7 ? iters : 7;  // 40-60 ms per round
    // mode 0: device-resident mirror; 1: trait path with host masks; 2: trait path with seeded device masks
    auto three_parties = [&](int mode, double* med_out, double* min_out, ProveTimes* party0, bool* ok_out) {
      struct Restore {
        int prev;
        explicit Restore(int m) : prev(trait_path_flag().exchange(m)) {}
        ~Restore() { trait_path_flag().store(prev); }
      } restore(mode);
      std::vector<double> walls;
      std::vector<ProveTimes> p0;
      Proof<P> proofs[3];
      for (int it = 0; it < iters3 + 1; ++it) {  // one warm-up round
        auto nets0 = LocalNetwork::new_parties(3), nets1 = LocalNetwork::new_parties(3);
        std::string errs[3];
        ProveTimes times[3];
        auto b0 = std::chrono::steady_clock::now();
        std::vector<std::thread> th;
        for (int p = 0; p < 3; ++p) {
          th.emplace_back([&, p] {
            try {
              check(csh_init(0), "csh_init");
              uint8_t my_seed[32];
              ShareRng(4242ull + it, 100 + p).fill(my_seed, 32);
              Rep3State state0 = Rep3State::create(nets0[p], my_seed);
              Rep3State state1 = state0.fork(0);
              proofs[p] = CoGroth16<P, T3>::template prove_inner<CircomReduction>(&nets0[p], &nets1[p], state0, state1, pk, m, sw3[p], &r3[p], &s3[p]);
              times[p] = last_prove_times();
            } catch (const std::exception& e) {
              errs[p] = e.what();
              nets0[p].abort();  // let the other parties unwind instead of waiting on this one
              nets1[p].abort();
            }
          });
        }
        for (auto& t : th) t.join();
        const double wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - b0).count();
        for (int p = 0; p < 3; ++p)
          if (!errs[p].empty()) throw Error("rep3 party " + std::to_string(p) + ": " + errs[p]);
        if (it == 0) continue;
        walls.push_back(wall);
        p0.push_back(times[0]);
      }
      const size_t wi = median_index(walls);
      *med_out = walls[wi];
      *min_out = *std::min_element(walls.begin(), walls.end());
      if (party0) *party0 = p0[wi];
      bool ok3 = true;
      for (int p = 0; p < 3; ++p)
        ok3 = ok3 && eq1(proofs[p].a, proof.a) && eq1(proofs[p].c, proof.c) && proofs[p].b.x == proof.b.x && proofs[p].b.y == proof.b.y;
      *ok_out = ok3;
    };
    double med = 0, mn = 0;
    bool ok3 = false;
    three_parties(0, &med, &mn, nullptr, &ok3);
    out_ms[4] = med;
    out_ms[5] = ok3 ? 1.0 : 0.0;
    if (mins_out) mins_out[2] = mn;
    if (rep3_trait_out) {
      for (int mode = 1; mode <= 2; ++mode) {
        double* o = rep3_trait_out + 13 * (mode - 1);
        ProveTimes t0;
        three_parties(mode, &o[0], &o[1], &t0, &ok3);
        o[2] = t0.mask_ms;
        o[3] = t0.witness_ms;
        o[4] = t0.half_ms;
        o[5] = t0.msm_ms;
        o[6] = t0.finish_ms;
        o[7] = ok3 ? 1.0 : 0.0;
        // ONE party with the GPU to itself: what a party of a one-GPU-per-party deployment computes between its network rounds
        struct Restore {
          int prev;
          explicit Restore(int m) : prev(trait_path_flag().exchange(m)) {}
          ~Restore() { trait_path_flag().store(prev); }
        } restore(mode);
        uint8_t sd1[32], sd2[32];
        ShareRng(777, 1).fill(sd1, 32);
        ShareRng(777, 2).fill(sd2, 32);
        Rep3State st{0, Rep3Rand(sd1, sd2)};
        std::vector<double> alone;
        std::vector<ProveTimes> ap;
        for (int it = 0; it < iters + 2; ++it) {
          auto a0 = std::chrono::steady_clock::now();
          ProveTimes pt;
          UninitBuf<Fr> h = CircomReduction::witness_map_trait_path<P, T3>(st, m, sw3[0].public_inputs, sw3[0].witness);
          pt.mask_ms = last_prove_times().mask_ms;
          pt.witness_ms = ms_since(a0);
          auto a1 = std::chrono::steady_clock::now();
          UninitBuf<Fr> half(sw3[0].witness.size());
          parallel_for(half.size(), 1 << 16, [&](size_t lo, size_t hi) {
            for (size_t i = lo; i < hi; ++i) half.data()[i] = T3::to_half_share(sw3[0].witness[i]);
          });
          pt.half_ms = ms_since(a1);
          (void)CoGroth16<P, T3>::msm_groups_trait_path(0, pk, r3[0], s3[0], h.data(), h.size(), sw3[0].public_inputs, half.data(), half.size());
          pt.msm_ms = last_prove_times().msm_ms;
          if (it < 2) continue;
          alone.push_back(ms_since(a0));
          ap.push_back(pt);
        }
        const size_t ai = median_index(alone);
        o[8] = alone[ai];
        o[9] = ap[ai].mask_ms;
        o[10] = ap[ai].witness_ms;
        o[11] = ap[ai].half_ms;
        o[12] = ap[ai].msm_ms;
      }
    }
  }
  return 0;
}

// BASELINE config 4 at scale with ONE GPU PER PARTY: three in-process Rep3 parties prove the synthetic 2^log_domain circuit, party p bound
// to devices[p] with its own copy of the proving key and matrices on that GPU (independent instances: no data-path collective, the
// parties exchange three curve points over the in-process network). devices may repeat (the three parties folded onto fewer GPUs).
// out = {wall ms of the best of `iters` three-party proves, proofs agree and equal the plain proof (1 / 0), key setup ms per device}.
template <class P>
int bench_rep3_party_per_gpu_t(int log_domain, int iters, const int devices[3], double* out, const uint32_t* g1_words, const uint32_t* g2_words) {
  using T3 = Rep3Groth16Driver<P>;
  using Fr = typename P::Fr;
  using Fq = typename P::Fq;
  using Share = Rep3PrimeFieldShare<Fr>;
  int home = 0;
  (void)csh_current_device(&home);
  // one circuit (key + matrices + witness) per distinct device, built on that device
  std::map<int, std::unique_ptr<SynthCircuit<P>>> circuits;
  double key_ms = 0;
  for (int p = 0; p < 3; ++p) {
    if (circuits.count(devices[p])) continue;
    std::string err;
    Joined th([&] {
      check(csh_init(devices[p]), "csh_init");
      circuits[devices[p]].reset(new SynthCircuit<P>(log_domain, g1_words, g2_words));
    });
    th.join();
    key_ms = std::max(key_ms, circuits[devices[p]]->key_ms);
  }
  SynthCircuit<P>& c0 = *circuits[devices[0]];
  const Fr r = c0.r, s = c0.s;
  FieldRng<Fr> sharer(99, /*domain=*/3);
  std::vector<Share> wsh[3];
  sharer.rep3(c0.sw.witness, wsh);
  Share r3[3], s3[3];
  {
    std::vector<Share> t[3];
    sharer.rep3({r, s}, t);
    for (int p = 0; p < 3; ++p) r3[p] = t[p][0], s3[p] = t[p][1];
  }
  SharedWitness<P, Share> sw3[3];
  for (int p = 0; p < 3; ++p) {
    sw3[p].public_inputs = c0.sw.public_inputs;
    sw3[p].witness = std::move(wsh[p]);
  }
  double best3 = 1e30;
  Proof<P> proofs[3];
  for (int it = 0; it < iters + 1; ++it) {  // + 1 warm-up round (lanes, arenas and pooled buffers of every party thread)
    auto nets0 = LocalNetwork::new_parties(3), nets1 = LocalNetwork::new_parties(3);
    std::string errs[3];
    auto b0 = std::chrono::steady_clock::now();
    std::vector<std::thread> th;
    for (int p = 0; p < 3; ++p) {
      th.emplace_back([&, p] {
        try {
          check(csh_init(devices[p]), "csh_init");
          SynthCircuit<P>& c = *circuits[devices[p]];
          uint8_t my_seed[32];
          ShareRng(4242ull + it, 100 + p).fill(my_seed, 32);
          Rep3State state0 = Rep3State::create(nets0[p], my_seed);
          Rep3State state1 = state0.fork(0);
          proofs[p] = CoGroth16<P, T3>::template prove_inner<CircomReduction>(&nets0[p], &nets1[p], state0, state1, c.pk, c.m, sw3[p], &r3[p], &s3[p]);
        } catch (const std::exception& e) {
          errs[p] = e.what();
          nets0[p].abort();
          nets1[p].abort();
        }
      });
    }
    for (auto& t : th) t.join();
    if (it) best3 = std::min(best3, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - b0).count());
    for (int p = 0; p < 3; ++p)
      if (!errs[p].empty()) throw Error("rep3 party " + std::to_string(p) + ": " + errs[p]);
  }
  // the plain proof of the same circuit with the same r, s, on the home device's circuit
  check(csh_init(devices[0]), "csh_init");
  c0.prove(false);
  auto eq1 = [](const AffineT<Fq>& x, const AffineT<Fq>& y) { return x.x == y.x && x.y == y.y; };
  bool ok3 = true;
  for (int p = 0; p < 3; ++p)
    ok3 = ok3 && eq1(proofs[p].a, c0.proof.a) && eq1(proofs[p].c, c0.proof.c) && proofs[p].b.x == c0.proof.b.x && proofs[p].b.y == c0.proof.b.y;
  for (auto& kv : circuits) {  // free every device's key on a thread bound to that device
    Joined th([&] {
      check(csh_init(kv.first), "csh_init");
      kv.second.reset();
    });
    th.join();
  }
  check(csh_init(home), "csh_init");
  out[0] = best3;
  out[1] = ok3 ? 1.0 : 0.0;
  out[2] = key_ms;
  return 0;
}
}  // namespace

extern "C" {

// out_ms[6] = {witness_map ms, create_proof ms, total prove ms, key generation+upload ms, three-party Rep3 prove wall ms,
// Rep3 proofs == plain proof (1/0)}; best of `iters`.
int cog16_bench_synthetic2(int curve, int log_domain, int iters, double* out_ms /* 6 entries */, int* check_ok, int with_rep3,
                           double* phases_out /* 3 entries: witness, msm, finish ms of the best prove; nullable */);
int cog16_bench_synthetic3(int curve, int log_domain, int iters, double* out_ms, int* check_ok, int with_rep3, double* phases_out, double* trait_out);
int cog16_bench_synthetic4(int curve, int log_domain, int iters, double* out_ms, int* check_ok, int with_rep3, double* phases_out, double* trait_out,
                           double* rep3_trait_out, double* mins_out);
int cog16_bench_synthetic(int curve, int log_domain, int iters, double* out_ms /* 6 entries */, int* check_ok, int with_rep3) {
  return cog16_bench_synthetic2(curve, log_domain, iters, out_ms, check_ok, with_rep3, nullptr);
}
int cog16_bench_synthetic2(int curve, int log_domain, int iters, double* out_ms, int* check_ok, int with_rep3, double* phases_out) {
  return cog16_bench_synthetic3(curve, log_domain, iters, out_ms, check_ok, with_rep3, phases_out, nullptr);
}
// ... and trait_out (5 entries, nullable): the same prove through the trait path (see bench_synth_t)
int cog16_bench_synthetic3(int curve, int log_domain, int iters, double* out_ms, int* check_ok, int with_rep3, double* phases_out, double* trait_out) {
  return cog16_bench_synthetic4(curve, log_domain, iters, out_ms, check_ok, with_rep3, phases_out, trait_out, nullptr, nullptr);
}
// + rep3_trait_out (26 doubles, layout at bench_synth_t) and mins_out (3 doubles: minimum of prove, trait path, three Rep3 parties)
int cog16_bench_synthetic4(int curve, int log_domain, int iters, double* out_ms, int* check_ok, int with_rep3, double* phases_out, double* trait_out,
                           double* rep3_trait_out, double* mins_out) {
  return guarded([&] {
    if (iters < 1) throw Error("cog16_bench_synthetic: iters < 1");
    return with_curve<Bn254, Bls12_381>(curve, [&](auto tag) {
      using P = decltype(tag);
      return bench_synth_t<P>(log_domain, iters, out_ms, check_ok, P::g1_generator_words(), P::g2_generator_words(), with_rep3 != 0, phases_out, trait_out, rep3_trait_out, mins_out);
    });
  });
}

int cog16_bench_rep3_party_per_gpu(int curve, int log_domain, int iters, const int devices[3], double* out /* 3 entries */) {
  return guarded([&] {
    if (!devices || !out || iters < 1) throw Error("cog16_bench_rep3_party_per_gpu: bad arguments");
    return with_curve<Bn254, Bls12_381>(curve, [&](auto tag) {
      using P = decltype(tag);
      return bench_rep3_party_per_gpu_t<P>(log_domain, iters, devices, out, P::g1_generator_words(), P::g2_generator_words());
    });
  });
}

// The synthetic circuit as an object: open (key + matrices + witness resident), prove (one plain prove_inner, phases out),
// check (closed form), close. bench.py's `--workload groth16_prove` times K cog16_synth_prove calls between barriers.
int cog16_synth_open(int curve, int log_domain, void** out) {
  return guarded([&] {
    if (!out || log_domain < 3 || log_domain > 26) throw Error("cog16_synth_open: bad arguments");
    return with_curve<Bn254, Bls12_381>(curve, [&](auto tag) {
      using P = decltype(tag);
      *out = static_cast<SynthBase*>(new SynthCircuit<P>(log_domain, P::g1_generator_words(), P::g2_generator_words()));
      return 0;
    });
  });
}
int cog16_synth_prove(void* h, double* phases_out /* witness, msm, finish ms; nullable */, double* key_ms /* nullable */) {
  return guarded([&] {
    if (!h) throw Error("cog16_synth_prove: NULL handle");
    SynthBase* c = static_cast<SynthBase*>(h);
    c->prove(false);
    if (phases_out) {
      phases_out[0] = c->phases.witness_ms;
      phases_out[1] = c->phases.msm_ms;
      phases_out[2] = c->phases.finish_ms;
    }
    if (key_ms) *key_ms = c->key_ms;
    return 0;
  });
}
int cog16_synth_check(void* h, int* ok) {
  return guarded([&] {
    if (!h || !ok) throw Error("cog16_synth_check: NULL argument");
    SynthBase* c = static_cast<SynthBase*>(h);
    c->prove(true);
    *ok = c->closed_form() ? 1 : 0;
    return 0;
  });
}
int cog16_synth_close(void* h) {
  delete static_cast<SynthBase*>(h);
  return 0;
}

}  // extern "C"
