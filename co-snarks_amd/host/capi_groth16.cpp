// C entry points of the host mirror (for the Python tests / bench and as a template for the Rust shim), Groth16 part: the provers, the
// witness-share files either side of them, and the LibSnark reduction from the reference's file formats.
//   cog16_prove_plain  == Groth16::<P>::plain_prove::<CircomReduction>            (groth16.rs:484-490)
//   cog16_prove_rep3   == three parties in one process, each running Rep3CoGroth16::prove::<_, CircomReduction>
//                         (groth16.rs:360-379) over LocalNetwork pairs -- the layout of the reference's own
//                         e2e test (tests/tests/circom/e2e_tests/rep3.rs:57-69): asserts the three proofs agree.
// curve: 0 BN254, 1 BLS12-381, 3 BLS12-377 (the LibSnark entries and cog16_witness_map); the PLONK / Honk driver entries (capi_plonk.cpp)
// also take 2 = Grumpkin for the MSM. Which curves an entry serves is the template argument list of its `entry` / `with_curve` call.
// r/s: canonical little-endian 4 x u64, or NULL to draw them with T::rand.
#include "capi_common.hpp"

using namespace cosnarks;
using namespace cosnarks::capi;

namespace {

template <class P>
int prove_plain_t(const uint8_t* zkey, size_t zlen, const uint8_t* wtns, size_t wlen, const uint64_t* r, const uint64_t* s, char* out,
                  size_t cap, uint64_t* h_out, size_t h_cap) {
  using T = PlainGroth16Driver<P>;
  using Fr = typename P::Fr;
  ProvingKey<P> pk;
  ConstraintMatrices<P> m;
  parse_zkey<P>(zkey, zlen, pk, m);
  UnitState st0, st1;
  Fr rr, ss;
  if (r) rr = fr_from_canonical<P>(r);
  if (s) ss = fr_from_canonical<P>(s);
  std::vector<Fr> h;
  Proof<P> pr;
  if (getenv("COG16_HOST_WTNS") || trait_path_flag().load()) {  // witness values converted on the host, SharedWitness as in the reference's CLI
    std::vector<Fr> w = parse_wtns<P>(wtns, wlen);
    SharedWitness<P, Fr> sw;
    sw.public_inputs.assign(w.begin(), w.begin() + m.num_instance_variables);
    sw.witness.assign(w.begin() + m.num_instance_variables, w.end());
    pr = CoGroth16<P, T>::template prove_inner<CircomReduction>(nullptr, nullptr, st0, st1, pk, m, sw, r ? &rr : nullptr, s ? &ss : nullptr, &h);
  } else {
    // zkey queries and the wtns values go to the device straight from the file images; only the public
    // inputs (a handful of values) are decoded on the host
    std::vector<Fr> pub = parse_wtns_prefix<P>(wtns, wlen, m.num_instance_variables);
    const DeviceScalars wit_dev = parse_wtns_to_device<P>(wtns, wlen, m.num_instance_variables);
    pr = CoGroth16<P, T>::template prove_inner_device_witness<CircomReduction>(nullptr, nullptr, st0, st1, pk, m, pub, wit_dev, r ? &rr : nullptr,
                                                                               s ? &ss : nullptr, &h);
  }
  if (h_out) {
    if (h.size() > h_cap) throw Error("h_out too small");
    memcpy(h_out, h.data(), h.size() * 32);
  }
  return write_out(proof_to_json(pr), out, cap);
}

// CompressedRep3SharedWitness::share_rep3 (co-circom-types/src/lib.rs:279-333). compression as the reference's enum
// (lib.rs:150-161): 0 None (replicated), 1 HalfShares (additive), 2 SeededShares, 3 SeededHalfShares -- the seeded
// levels keep one explicit share vector and two ChaCha12 seeds (rep3.rs:455-533).
template <class P>
void split_witness_rep3(const std::vector<typename P::Fr>& w, size_t npub, int compression, uint64_t seed,
                        sharefile::CompressedRep3SharedWitness<P> out[3]) {
  using Fr = typename P::Fr;
  if (npub > w.size()) throw Error("num_inputs exceeds the witness length");
  if (compression < 0 || compression > 3) throw Error("compression must be 0 (none), 1 (half shares), 2 (seeded shares) or 3 (seeded half shares)");
  FieldRng<Fr> sh(seed, /*domain=*/1);
  static const sharefile::Rep3Variant kinds[4] = {sharefile::REPLICATED, sharefile::ADDITIVE, sharefile::SEEDED_REPLICATED, sharefile::SEEDED_ADDITIVE};
  for (int p = 0; p < 3; ++p) {
    out[p].public_inputs.assign(w.begin(), w.begin() + npub);
    out[p].kind = kinds[compression];
  }
  if (compression >= 2) {
    sharefile::SeededShare<Fr> a, b, c;
    b.is_seed = c.is_seed = true;
    b.len = c.len = w.size() - npub;
    for (int i = 0; i < 4; ++i) {
      uint64_t v = sh.gen(), u = sh.gen();
      memcpy(b.seed + 8 * i, &v, 8);
      memcpy(c.seed + 8 * i, &u, 8);
    }
    const std::vector<Fr> bv = b.expand(), cv = c.expand();
    for (size_t i = npub; i < w.size(); ++i) a.shares.push_back(Fr::sub(Fr::sub(w[i], bv[i - npub]), cv[i - npub]));
    if (compression == 3) {  // share_field_elements_additive_seeded: [a, b, c]
      out[0].sa = a;
      out[1].sa = b;
      out[2].sa = c;
    } else {  // share_field_elements_seeded: {a, c}, {b, a}, {c, b}
      out[0].sa = a; out[0].sb = c;
      out[1].sa = b; out[1].sb = a;
      out[2].sa = c; out[2].sb = b;
    }
    return;
  }
  for (size_t i = npub; i < w.size(); ++i) {
    Rep3PrimeFieldShare<Fr> t[3];
    sh.rep3(w[i], t);
    for (int p = 0; p < 3; ++p) {
      if (compression == 0) out[p].replicated.push_back(t[p]);
      else out[p].additive.push_back(t[p].a);
    }
  }
}

// SharedWitness::share_shamir (co-circom-types/src/lib.rs:362-381)
template <class P>
std::vector<SharedWitness<P, typename P::Fr>> split_witness_shamir(const std::vector<typename P::Fr>& w, size_t npub, int t, int n, uint64_t seed) {
  using Fr = typename P::Fr;
  if (npub > w.size()) throw Error("num_inputs exceeds the witness length");
  if (n < 2 * t + 1 || t < 1) throw Error("num_parties must be at least 2 * threshold + 1");
  std::vector<SharedWitness<P, Fr>> sw(n);
  std::vector<std::vector<Fr>> sh = FieldRng<Fr>(seed, /*domain=*/2).shamir(std::vector<Fr>(w.begin() + npub, w.end()), t, n);
  for (int p = 0; p < n; ++p) {
    sw[p].public_inputs.assign(w.begin(), w.begin() + npub);
    sw[p].witness = std::move(sh[p]);
  }
  return sw;
}

// ---- where a prover's key and matrices come from. A key source has
//   open(pk, m, upload) -> KeyCounts   on the thread that starts the parties: whatever it can refuse up front, and with `upload` the key
//                                      and matrices onto that thread's device (one GPU serves all parties);
//   load(pk, m)                        key + matrices onto the calling thread's device.
struct KeyCounts {
  size_t n_instance, n_witness;
};

template <class P>
struct ZkeyImage {
  const uint8_t* zkey;
  size_t zlen;
  void load(ProvingKey<P>& pk, ConstraintMatrices<P>& m) const { parse_zkey<P>(zkey, zlen, pk, m); }
  KeyCounts open(ProvingKey<P>& pk, ConstraintMatrices<P>& m, bool upload) const {  // parsed in either case: a bad key is refused before any party starts
    parse_zkey<P>(zkey, zlen, pk, m, upload);
    return {m.num_instance_variables, m.num_witness_variables};
  }
};

// the files the reference's LibSnark test reads (co-groth16/src/lib.rs:231-290): ark ProvingKey (deserialize_uncompressed_unchecked) and
// Matrix<F> blobs a / b / c; ConstraintMatrices filled in as :268-279 does (num_instance_variables = b_g1_query.len() - l_query.len(), ...)
template <class P>
struct LibsnarkFiles {
  const uint8_t* const* mats;
  const size_t* lens;
  const uint8_t* pkey;
  size_t pklen;
  void load(ProvingKey<P>& pk, ConstraintMatrices<P>& m) const {
    using Fr = typename P::Fr;
    ark::Reader rp(pkey, pklen);
    ark::read_proving_key<P>(rp, pk);
    if (!rp.done()) throw Error("trailing bytes after ProvingKey");
    if (pk.b_g1_query.host.size() < pk.l_query.host.size() || pk.a_query.host.size() != pk.b_g1_query.host.size() ||
        pk.b_g2_query.host.size() != pk.b_g1_query.host.size())
      throw Error("ProvingKey: query lengths are inconsistent");
    ark::Reader ra(mats[0], lens[0]), rb(mats[1], lens[1]), rc(mats[2], lens[2]);
    m.a = ark::read_matrix<Fr>(ra);
    m.b = ark::read_matrix<Fr>(rb);
    m.c = ark::read_matrix<Fr>(rc);
    if (!ra.done() || !rb.done() || !rc.done()) throw Error("trailing bytes after Matrix");
    if (m.a.size() != m.b.size() || m.a.size() != m.c.size()) throw Error("matrices disagree on the number of constraints");
    m.num_instance_variables = pk.b_g1_query.host.size() - pk.l_query.host.size();   // lib.rs:269
    m.num_witness_variables = pk.a_query.host.size() - m.num_instance_variables;     // lib.rs:270-271
    m.num_constraints = m.a.size();
    m.upload();
    pk.a_query.upload(P::ID, CSH_G1);
    pk.b_g1_query.upload(P::ID, CSH_G1);
    pk.l_query.upload(P::ID, CSH_G1, pk.b_g1_query.host.size() - pk.l_query.host.size());
    pk.h_query.upload(P::ID, CSH_G1);
    pk.b_g2_query.upload(P::ID, CSH_G2);
    pk.build_tables();
  }
  KeyCounts open(ProvingKey<P>& pk, ConstraintMatrices<P>& m, bool upload) const {
    if (upload) load(pk, m);
    ark::Reader rp(pkey, pklen);  // the instance count without uploading anything: ic = gamma_abc_g1
    ProvingKey<P> probe;
    ark::read_proving_key<P>(rp, probe);
    if (probe.b_g1_query.host.size() < probe.l_query.host.size()) throw Error("ProvingKey: query lengths are inconsistent");
    return {probe.b_g1_query.host.size() - probe.l_query.host.size(), probe.l_query.host.size()};  // l_query: one point per witness variable
  }
};

// One GPU per party when the node has them (BASELINE config 4): device memory is not shared between GPUs, so every party then uploads
// its own copy of the proving key and matrices onto its device; on one GPU a single copy serves all.
template <class P, class Key>
struct PartyKeys {
  struct Own {
    ProvingKey<P> pk;
    ConstraintMatrices<P> m;
  };
  const Key& key;
  int ndev = 1;
  bool per_party_keys;
  Own shared;
  KeyCounts counts;
  explicit PartyKeys(const Key& k) : key(k) {
    csh_device_count(&ndev);
    per_party_keys = ndev > 1;
    counts = key.open(shared.pk, shared.m, /*upload=*/!per_party_keys);
  }
  int device_of(int p) const { return ndev > 0 ? p % ndev : 0; }
  const Own& of_this_party(Own& own) const {  // on the party's thread, after it bound its device
    if (!per_party_keys) return shared;
    key.load(own.pk, own.m);
    return own;
  }
};

inline void check_share_counts(const KeyCounts& counts, size_t n_public, size_t n_witness) {
  if (n_public != counts.n_instance) throw Error("witness share: public input count does not match the proving key");
  if (n_witness != counts.n_witness) throw Error("witness share: the amount of private witness variables does not match the proving key");
}

template <class P>
const Proof<P>& agreed_proof(const Proof<P>* proofs, int n, const char* or_else) {
  const std::vector<uint8_t> b0 = ark::write_proof<P>(proofs[0]);
  for (int p = 1; p < n; ++p)
    if (b0 != ark::write_proof<P>(proofs[p])) throw Error(or_else);
  return proofs[0];
}

// the three parties' h half-share vectors, one after the other
template <class Fr>
int copy_h_shares(const std::vector<Fr> hs[3], uint64_t* out, size_t cap_elems, const char* or_else) {
  const size_t n = hs[0].size();
  if (3 * n > cap_elems) throw Error(or_else);
  for (int p = 0; p < 3; ++p) memcpy(out + 4 * n * p, hs[p].data(), 32 * n);
  return (int)n;
}

// Rep3CoGroth16::prove::<R> (groth16.rs:360-379) with three in-process parties, as the reference's Rep3 tests run theirs
// (tests/tests/circom/e2e_tests/rep3.rs:57-69). shares_for(counts, shares) hands over what party p read from its `.shared` file
// (co-circom.rs:1014-1016) as shares[p], after the key was opened and before anything is drawn; additive half shares are completed inside
// the party's thread. r / s are shared from `seed`; the three proofs must agree. hs (nullable): the parties' h half-share vectors.
template <class R, class P, class Key, class SharesFor>
Proof<P> prove_rep3(const Key& key, SharesFor shares_for, uint64_t seed, const uint64_t* r, const uint64_t* s, std::vector<typename P::Fr>* hs) {
  using T = Rep3Groth16Driver<P>;
  using Fr = typename P::Fr;
  using Share = Rep3PrimeFieldShare<Fr>;
  PartyKeys<P, Key> keys(key);
  sharefile::CompressedRep3SharedWitness<P> shares[3];
  shares_for(keys.counts, shares);  // checked up front for all parties: a party that bails out alone would leave the other two waiting on the network
  FieldRng<Fr> rs_sharer(seed, /*domain=*/11);
  Share r3[3], s3[3];
  if (r) rs_sharer.rep3(fr_from_canonical<P>(r), r3);
  if (s) rs_sharer.rep3(fr_from_canonical<P>(s), s3);
  Proof<P> proofs[3];
  run_parties<2>(3, [&](int p) { return keys.device_of(p); }, [&](int p, const LocalNetwork& net0, const LocalNetwork& net1) {
    typename PartyKeys<P, Key>::Own own;
    const auto& k = keys.of_this_party(own);
    Rep3State state0 = rep3_state(seed, p, net0);  // groth16.rs:371
    Rep3State state1 = state0.fork(0);             // :372
    SharedWitness<P, Share> sw = sharefile::uncompress<P>(std::move(shares[p]), net0);  // co-circom.rs:1016
    proofs[p] = CoGroth16<P, T>::template prove_inner<R>(&net0, &net1, state0, state1, k.pk, k.m, sw, r ? &r3[p] : nullptr, s ? &s3[p] : nullptr,
                                                         hs ? &hs[p] : nullptr);
  });
  return agreed_proof(proofs, 3, "the three parties disagree on the proof");
}

// ShamirCoGroth16::prove::<R> (groth16.rs:439-463) with n in-process parties of threshold t, party p holding shares_for(counts)[p], the share
// it read from its `.shared` file (co-circom.rs:1031-1035). Preprocessing (ShamirPreprocessing::new, DN07 double sharings) is replaced by a
// dealer that hands every party its three (degree-t, degree-2t) share pairs (two rand calls + one scalar_mul: groth16.rs:448-449); with
// r / s given, the first two pairs share exactly r and s, so the proof equals the plain one for the same r, s.
template <class R, class P, class Key, class SharesFor>
Proof<P> prove_shamir(const Key& key, int n, int t, SharesFor shares_for, uint64_t seed, const uint64_t* r, const uint64_t* s) {
  using T = ShamirGroth16Driver<P>;
  using Fr = typename P::Fr;
  if (n < 2 * t + 1 || t < 1) throw Error("num_parties must be at least 2 * threshold + 1");
  PartyKeys<P, Key> keys(key);
  std::vector<SharedWitness<P, Fr>> sw = shares_for(keys.counts);
  FieldRng<Fr> dealer(seed, /*domain=*/12);
  std::vector<std::deque<std::pair<Fr, Fr>>> pairs(n);
  Fr rr, ss;
  if (r) rr = fr_from_canonical<P>(r);
  if (s) ss = fr_from_canonical<P>(s);
  dealer.double_sharing(t, pairs, r ? &rr : nullptr);
  dealer.double_sharing(t, pairs, s ? &ss : nullptr);
  dealer.double_sharing(t, pairs);
  std::vector<Proof<P>> proofs(n);
  run_parties<2>(n, [&](int p) { return keys.device_of(p); }, [&](int p, const LocalNetwork& net0, const LocalNetwork& net1) {
    typename PartyKeys<P, Key>::Own own;
    const auto& k = keys.of_this_party(own);
    auto state0 = ShamirState<Fr>::create(p, n, t, pairs[p]);
    auto state1 = state0.fork(1);
    proofs[p] = CoGroth16<P, T>::template prove_inner<R>(&net0, &net1, state0, state1, k.pk, k.m, sw[p], nullptr, nullptr);
  });
  return agreed_proof(proofs.data(), n, "the parties disagree on the proof");
}

// ---- from a zkey image: the proof as JSON -------------------------------------------------------------------------------------------
template <class P>
int prove_rep3_zkey(const uint8_t* zkey, size_t zlen, sharefile::CompressedRep3SharedWitness<P> shares[3], uint64_t seed, const uint64_t* r,
                    const uint64_t* s, char* out, size_t cap, uint64_t* h_shares_out, size_t h_cap) {
  std::vector<typename P::Fr> hs[3];
  const Proof<P> proof = prove_rep3<CircomReduction, P>(ZkeyImage<P>{zkey, zlen}, [&](const KeyCounts& counts, sharefile::CompressedRep3SharedWitness<P> to[3]) {
    for (int p = 0; p < 3; ++p) check_share_counts(counts, shares[p].public_inputs.size(), shares[p].length());
    for (int p = 0; p < 3; ++p) to[p] = std::move(shares[p]);
  }, seed, r, s, hs);
  if (h_shares_out) copy_h_shares(hs, h_shares_out, h_cap, "h_shares_out too small");
  return write_out(proof_to_json(proof), out, cap);
}

template <class P>
int prove_rep3_t(const uint8_t* zkey, size_t zlen, const uint8_t* wtns, size_t wlen, uint64_t seed, const uint64_t* r, const uint64_t* s,
                 char* out, size_t cap, uint64_t* h_shares_out, size_t h_cap) {
  std::vector<typename P::Fr> w = parse_wtns<P>(wtns, wlen);
  sharefile::CompressedRep3SharedWitness<P> shares[3];
  split_witness_rep3<P>(w, zkey_num_instance_variables<P>(zkey, zlen), 0, seed, shares);
  return prove_rep3_zkey<P>(zkey, zlen, shares, seed, r, s, out, cap, h_shares_out, h_cap);
}

template <class P>
int prove_shamir_zkey(const uint8_t* zkey, size_t zlen, std::vector<SharedWitness<P, typename P::Fr>>& sw, int t, uint64_t seed, const uint64_t* r,
                      const uint64_t* s, char* out, size_t cap) {
  const Proof<P> proof = prove_shamir<CircomReduction, P>(ZkeyImage<P>{zkey, zlen}, (int)sw.size(), t, [&](const KeyCounts& counts) {
    for (auto& w : sw) check_share_counts(counts, w.public_inputs.size(), w.witness.size());
    return std::move(sw);
  }, seed, r, s);
  return write_out(proof_to_json(proof), out, cap);
}

// From a plain witness: ShamirCoGroth16::prove after share_shamir, or Rep3CoGroth16::prove_with_shamir_bridge
// (groth16.rs:394-417) when `bridge` is set.
template <class P>
int prove_shamir_t(const uint8_t* zkey, size_t zlen, const uint8_t* wtns, size_t wlen, int n, int t, uint64_t seed, const uint64_t* r,
                   const uint64_t* s, int bridge, char* out, size_t cap) {
  using Fr = typename P::Fr;
  if (n < 2 * t + 1 || t < 1) throw Error("num_parties must be at least 2 * threshold + 1");
  if (bridge && (n != 3 || t != 1)) throw Error("the Rep3 -> Shamir bridge is the 3-party, threshold-1 case");
  std::vector<Fr> w = parse_wtns<P>(wtns, wlen);
  const size_t npub = zkey_num_instance_variables<P>(zkey, zlen);
  if (!bridge) {
    auto sw = split_witness_shamir<P>(w, npub, t, n, seed);
    return prove_shamir_zkey<P>(zkey, zlen, sw, t, seed, r, s, out, cap);
  }
  if (npub > w.size()) throw Error("num_inputs exceeds the witness length");
  // Rep3 shares first (rep3.rs:281-292), then translate_primefield_repshare_vec on the device (bridges/rep3_to_shamir.rs:43-62)
  std::vector<SharedWitness<P, Fr>> sw(3);
  std::vector<Rep3PrimeFieldShare<Fr>> rs[3];
  FieldRng<Fr>(seed, /*domain=*/1).rep3(std::vector<Fr>(w.begin() + npub, w.end()), rs);
  for (int p = 0; p < 3; ++p) {
    sw[p].public_inputs.assign(w.begin(), w.begin() + npub);
    Fr x, y;
    rep3_to_shamir_points(p, x, y);
    sw[p].witness.resize(rs[p].size());
    check(csh_rep3_to_shamir_vec(P::ID, (const uint64_t*)rs[p].data(), (const uint64_t*)&x, (const uint64_t*)&y, (uint64_t*)sw[p].witness.data(),
                                 rs[p].size()), "csh_rep3_to_shamir_vec");
  }
  return prove_shamir_zkey<P>(zkey, zlen, sw, t, seed, r, s, out, cap);
}

// witness_map_from_matrices of either reduction on caller-supplied matrices (CSR) and a full witness: plain (mode 0) or
// three in-process Rep3 parties (mode 1; h_out receives the three parties' half-share vectors back to back).
template <class P>
int witness_map_t(int reduction, int mode, const uint64_t* const row_ptr[3], const uint32_t* const col[3], const uint64_t* const coef[3],
                  size_t n_rows, size_t n_instance, const uint64_t* witness_full, size_t n_vars, uint64_t seed, uint64_t* h_out, size_t h_cap) {
  using Fr = typename P::Fr;
  ConstraintMatrices<P> m;
  m.num_instance_variables = n_instance;
  m.num_witness_variables = n_vars - n_instance;
  m.num_constraints = n_rows;
  auto fill = [&](int k, std::vector<std::vector<std::pair<Fr, size_t>>>& dst) {
    if (!row_ptr[k]) return;
    dst.resize(n_rows);
    for (size_t i = 0; i < n_rows; ++i)
      for (uint64_t e = row_ptr[k][i]; e < row_ptr[k][i + 1]; ++e) {
        Fr c;
        memcpy(&c, coef[k] + 4 * e, 32);
        dst[i].push_back({c, (size_t)col[k][e]});
      }
  };
  fill(0, m.a);
  fill(1, m.b);
  fill(2, m.c);
  m.upload();
  std::vector<Fr> w(n_vars);
  memcpy(w.data(), witness_full, 32 * n_vars);
  std::vector<Fr> pub(w.begin(), w.begin() + n_instance), wit(w.begin() + n_instance, w.end());
  auto run = [&](auto driver_tag, auto& state, const auto& shares) {
    using T = decltype(driver_tag);
    if (reduction == 0) return CircomReduction::witness_map_from_matrices<P, T>(state, m, pub, shares);
    return LibSnarkReduction::witness_map_from_matrices<P, T>(state, m, pub, shares);
  };
  if (mode == 0) {
    UnitState st;
    std::vector<Fr> h = run(PlainGroth16Driver<P>{}, st, wit);
    if (h.size() > h_cap) throw Error("h_out too small");
    memcpy(h_out, h.data(), 32 * h.size());
    return (int)h.size();
  }
  std::vector<Rep3PrimeFieldShare<Fr>> wit3[3];
  FieldRng<Fr>(seed, /*domain=*/4).rep3(wit, wit3);
  std::vector<Fr> hs[3];
  run_parties<1>(3, on_device(0), [&](int p, const LocalNetwork& net) {
    Rep3State state = rep3_state(seed, p, net);
    hs[p] = run(Rep3Groth16Driver<P>{}, state, wit3[p]);
  });
  return copy_h_shares(hs, h_out, h_cap, "h_out too small");
}

// LibSnarkReduction straight from the reference's file formats (co-groth16/src/lib.rs:243-262): ark-serialize Matrix<F> blobs
// for a, b, c and a wtns container. h_out: plain h (Montgomery limbs); returns the domain size or -1.
template <class P>
int libsnark_from_files_t(const uint8_t* const mats[3], const size_t lens[3], const uint8_t* wtns, size_t wlen, size_t n_instance,
                          uint64_t* h_out, size_t h_cap) {
  using Fr = typename P::Fr;
  ConstraintMatrices<P> m;
  ark::Reader ra(mats[0], lens[0]), rb(mats[1], lens[1]), rc(mats[2], lens[2]);
  m.a = ark::read_matrix<Fr>(ra);
  m.b = ark::read_matrix<Fr>(rb);
  m.c = ark::read_matrix<Fr>(rc);
  if (!ra.done() || !rb.done() || !rc.done()) throw Error("trailing bytes after Matrix");
  if (m.a.size() != m.b.size() || m.a.size() != m.c.size()) throw Error("matrices disagree on the number of constraints");
  std::vector<Fr> w = ark::read_wtns_positional<Fr>(wtns, wlen);
  if (n_instance > w.size()) throw Error("more instance variables than witness values");
  m.num_instance_variables = n_instance;
  m.num_witness_variables = w.size() - n_instance;
  m.num_constraints = m.a.size();
  m.upload();
  UnitState st;
  std::vector<Fr> pub(w.begin(), w.begin() + n_instance), wit(w.begin() + n_instance, w.end());
  std::vector<Fr> h = LibSnarkReduction::witness_map_from_matrices<P, PlainGroth16Driver<P>>(st, m, pub, wit);
  if (h.size() > h_cap) throw Error("h_out too small");
  memcpy(h_out, h.data(), 32 * h.size());
  return (int)h.size();
}

// ---- from the LibSnark files: the proof as ark-serialize Proof {a, b, c}, uncompressed; these return its length -------------------------
template <class Fr>
std::vector<Fr> read_libsnark_witness(const uint8_t* wtns, size_t wlen, size_t n_instance) {
  std::vector<Fr> w = ark::read_wtns_positional<Fr>(wtns, wlen);
  if (n_instance > w.size()) throw Error("more instance variables than witness values");
  return w;
}

// Groth16::<P>::plain_prove::<LibSnarkReduction>. r, s: canonical limbs, nullable (drawn otherwise).
template <class P>
int prove_libsnark_t(const LibsnarkFiles<P>& files, const uint8_t* wtns, size_t wlen, const uint64_t* r, const uint64_t* s, uint8_t* out,
                     size_t cap, uint64_t* h_out, size_t h_cap) {
  using T = PlainGroth16Driver<P>;
  using Fr = typename P::Fr;
  ProvingKey<P> pk;
  ConstraintMatrices<P> m;
  files.load(pk, m);
  std::vector<Fr> w = read_libsnark_witness<Fr>(wtns, wlen, m.num_instance_variables);
  SharedWitness<P, Fr> sw;
  sw.public_inputs.assign(w.begin(), w.begin() + m.num_instance_variables);        // lib.rs:283-287
  sw.witness.assign(w.begin() + m.num_instance_variables, w.end());
  UnitState st0, st1;
  Fr rr, ss;
  if (r) rr = fr_from_canonical<P>(r);
  if (s) ss = fr_from_canonical<P>(s);
  std::vector<Fr> h;
  const Proof<P> pr = CoGroth16<P, T>::template prove_inner<LibSnarkReduction>(nullptr, nullptr, st0, st1, pk, m, sw, r ? &rr : nullptr,
                                                                                s ? &ss : nullptr, h_out ? &h : nullptr);
  if (h_out) {
    if (h.size() > h_cap) throw Error("h_out too small");
    memcpy(h_out, h.data(), h.size() * 32);
  }
  return copy_out(ark::write_proof<P>(pr), out, cap);
}

// mode: 0 plain, 1 Rep3 (the witness shared with share_field_elements semantics from `seed`; h_out: the three parties' h half-shares),
// 2 + 256 * parties + 65536 * threshold: Shamir (the witness shared with share_shamir semantics from `seed`)
template <class P>
int prove_libsnark_any(int mode, const uint8_t* const mats[3], const size_t lens[3], const uint8_t* wtns, size_t wlen, const uint8_t* pkey,
                       size_t pklen, uint64_t seed, const uint64_t* r, const uint64_t* s, uint8_t* out, size_t cap, uint64_t* h_out, size_t h_cap) {
  using Fr = typename P::Fr;
  const LibsnarkFiles<P> files{mats, lens, pkey, pklen};
  if (mode == 0) return prove_libsnark_t<P>(files, wtns, wlen, r, s, out, cap, h_out, h_cap);
  if ((mode & 255) == 2) {
    const int n = (mode >> 8) & 255, t = (mode >> 16) & 255;
    return copy_out(ark::write_proof<P>(prove_shamir<LibSnarkReduction, P>(files, n, t, [&](const KeyCounts& counts) {
      return split_witness_shamir<P>(read_libsnark_witness<Fr>(wtns, wlen, counts.n_instance), counts.n_instance, t, n, seed);
    }, seed, r, s)), out, cap);
  }
  std::vector<Fr> hs[3];
  const Proof<P> proof = prove_rep3<LibSnarkReduction, P>(files, [&](const KeyCounts& counts, sharefile::CompressedRep3SharedWitness<P> to[3]) {
    split_witness_rep3<P>(read_libsnark_witness<Fr>(wtns, wlen, counts.n_instance), counts.n_instance, 0, seed, to);
  }, seed, r, s, h_out ? hs : nullptr);
  if (h_out) copy_h_shares(hs, h_out, h_cap, "h_out too small");
  return copy_out(ark::write_proof<P>(proof), out, cap);
}
int prove_libsnark_entry(int curve, int mode, const uint8_t* a, size_t alen, const uint8_t* b, size_t blen, const uint8_t* c, size_t clen,
                         const uint8_t* wtns, size_t wlen, const uint8_t* pkey, size_t pklen, uint64_t seed, const uint64_t* r, const uint64_t* s,
                         uint8_t* out, size_t cap, uint64_t* h_out, size_t h_cap_elems) {
  const uint8_t* mats[3] = {a, b, c};
  const size_t lens[3] = {alen, blen, clen};
  return with_curve<Bn254, Bls12_381, Bls12_377>(curve, [&](auto tag) {
    return prove_libsnark_any<decltype(tag)>(mode, mats, lens, wtns, wlen, pkey, pklen, seed, r, s, out, cap, h_out, h_cap_elems);
  });
}

void require_protocol(int protocol) {
  if (protocol != 0 && protocol != 1) throw Error("protocol must be 0 (Rep3) or 1 (Shamir)");
}
}  // namespace

extern "C" {

int cog16_libsnark_from_files(int curve, const uint8_t* a, size_t alen, const uint8_t* b, size_t blen, const uint8_t* c, size_t clen,
                              const uint8_t* wtns, size_t wlen, size_t n_instance, uint64_t* h_out, size_t h_cap_elems) {
  const uint8_t* const mats[3] = {a, b, c};
  const size_t lens[3] = {alen, blen, clen};
  return entry<Bn254, Bls12_381, Bls12_377>(curve, [&](auto tag) {
    return libsnark_from_files_t<decltype(tag)>(mats, lens, wtns, wlen, n_instance, h_out, h_cap_elems);
  });
}

// proof_libsnark_penumbra_bls12_377 (co-groth16/src/lib.rs:231-290) and its counterparts on the other curves: see prove_libsnark_t;
// cog16_prove_libsnark_rep3: the same circuit through three in-process Rep3 parties, one GPU per party when the node has them
// (prove_rep3). Return the proof's byte length or -1.
int cog16_prove_libsnark(int curve, const uint8_t* a, size_t alen, const uint8_t* b, size_t blen, const uint8_t* c, size_t clen, const uint8_t* wtns,
                         size_t wlen, const uint8_t* pkey, size_t pklen, const uint64_t* r, const uint64_t* s, uint8_t* out, size_t cap,
                         uint64_t* h_out, size_t h_cap_elems) {
  return guarded([&] { return prove_libsnark_entry(curve, 0, a, alen, b, blen, c, clen, wtns, wlen, pkey, pklen, 0, r, s, out, cap, h_out, h_cap_elems); });
}
// ShamirCoGroth16::prove::<LibSnarkReduction> with num_parties in-process parties and the given threshold (prove_shamir)
int cog16_prove_libsnark_shamir(int curve, const uint8_t* a, size_t alen, const uint8_t* b, size_t blen, const uint8_t* c, size_t clen,
                                const uint8_t* wtns, size_t wlen, const uint8_t* pkey, size_t pklen, int num_parties, int threshold, uint64_t seed,
                                const uint64_t* r, const uint64_t* s, uint8_t* out, size_t cap) {
  return guarded([&] {
    if (num_parties < 3 || num_parties > 255 || threshold < 1 || threshold > 127) throw Error("num_parties / threshold out of range");
    return prove_libsnark_entry(curve, 2 + 256 * num_parties + 65536 * threshold, a, alen, b, blen, c, clen, wtns, wlen, pkey, pklen, seed, r, s, out,
                                cap, nullptr, 0);
  });
}
int cog16_prove_libsnark_rep3(int curve, const uint8_t* a, size_t alen, const uint8_t* b, size_t blen, const uint8_t* c, size_t clen,
                              const uint8_t* wtns, size_t wlen, const uint8_t* pkey, size_t pklen, uint64_t seed, const uint64_t* r, const uint64_t* s,
                              uint8_t* out, size_t cap, uint64_t* h_shares_out, size_t h_cap_elems) {
  return guarded([&] {
    return prove_libsnark_entry(curve, 1, a, alen, b, blen, c, clen, wtns, wlen, pkey, pklen, seed, r, s, out, cap, h_shares_out, h_cap_elems);
  });
}

// Returns the domain size (entries per party in h_out) or -1. reduction: 0 CircomReduction, 1 LibSnarkReduction (needs
// the C matrix); mode: 0 plain, 1 three Rep3 parties. CSR triples for a, b, c (c may be NULL for reduction 0).
int cog16_witness_map(int curve, int reduction, int mode, const uint64_t* const row_ptr[3], const uint32_t* const col[3],
                      const uint64_t* const coef[3], size_t n_rows, size_t n_instance, const uint64_t* witness_full, size_t n_vars, uint64_t seed,
                      uint64_t* h_out, size_t h_cap_elems) {
  return entry<Bn254, Bls12_381, Bls12_377>(curve, [&](auto tag) {
    return witness_map_t<decltype(tag)>(reduction, mode, row_ptr, col, coef, n_rows, n_instance, witness_full, n_vars, seed, h_out, h_cap_elems);
  });
}

// `co-circom split-witness` (co-circom.rs:660-740): protocol 0 = Rep3 (three files; compression 0 none, 1 half shares,
// 2 seeded shares, 3 seeded half shares = what the reference's CLI writes), 1 = Shamir (num_parties files of threshold `threshold`). The
// files are written back to back into `out`; sizes[i] is the length of party i's file. num_inputs counts the public inputs and the
// constant 1 (r1cs.num_inputs). Host-only (no device call). Returns the number of files or -1.
int cog16_split_witness(int curve, int protocol, const uint8_t* wtns, size_t wlen, size_t num_inputs, int compression, int threshold,
                        int num_parties, uint64_t seed, uint8_t* out, size_t cap, size_t* sizes) {
  return entry<Bn254, Bls12_381>(curve, [&](auto tag) {
    using P = decltype(tag);
    std::vector<std::vector<uint8_t>> files;
    std::vector<typename P::Fr> w = parse_wtns<P>(wtns, wlen);
    require_protocol(protocol);
    if (protocol == 0) {
      sharefile::CompressedRep3SharedWitness<P> sh[3];
      split_witness_rep3<P>(w, num_inputs, compression, seed, sh);
      for (int p = 0; p < 3; ++p) files.push_back(sharefile::write_rep3<P>(sh[p]));
    } else {
      for (auto& sw : split_witness_shamir<P>(w, num_inputs, threshold, num_parties, seed)) files.push_back(sharefile::write_shamir<P>(sw));
    }
    return copy_out(files, out, cap, sizes);
  });
}

// Parse one witness-share file and write it again (must reproduce the input byte for byte); reports the variant
// (Rep3: 0 replicated, 1 seeded replicated, 2 additive, 3 seeded additive; Shamir: 0) and the element counts. Host-only. Returns bytes written or -1.
int cog16_share_file_roundtrip(int curve, int protocol, const uint8_t* file, size_t len, uint8_t* out, size_t cap, uint32_t* variant,
                               size_t* n_public, size_t* n_witness) {
  return entry<Bn254, Bls12_381>(curve, [&](auto tag) {
    using P = decltype(tag);
    std::vector<uint8_t> buf;
    require_protocol(protocol);
    if (protocol == 0) {
      auto w = sharefile::read_rep3<P>(file, len);
      *variant = w.kind;
      *n_public = w.public_inputs.size();
      *n_witness = w.length();
      buf = sharefile::write_rep3<P>(w);
    } else {
      auto w = sharefile::read_shamir<P>(file, len);
      *variant = 0;
      *n_public = w.public_inputs.size();
      *n_witness = w.witness.size();
      buf = sharefile::write_shamir<P>(w);
    }
    return copy_out(buf, out, cap);
  });
}

// The public-input file `generate-proof` writes next to the proof (co-circom.rs:1120-1140): the share file's public
// inputs without the leading constant 1, as a compact JSON array of decimal strings. Host-only. Returns 0 or -1.
int cog16_public_inputs_json(int curve, int protocol, const uint8_t* file, size_t len, char* out_json, size_t cap) {
  return entry<Bn254, Bls12_381>(curve, [&](auto tag) {
    using P = decltype(tag);
    require_protocol(protocol);
    const std::vector<typename P::Fr> pub = protocol == 0 ? sharefile::read_rep3<P>(file, len).public_inputs : sharefile::read_shamir<P>(file, len).public_inputs;
    std::string j = "[";
    for (size_t i = 1; i < pub.size(); ++i) {
      if (i > 1) j += ",";
      j += "\"" + to_decimal(pub[i]) + "\"";
    }
    j += "]";
    return write_out(j, out_json, cap);
  });
}

// `co-circom generate-proof` from the parties' `.shared` files (co-circom.rs:1008-1050) with in-process parties:
// protocol 0 = Rep3 (exactly three files), 1 = Shamir (n files, threshold t).
int cog16_prove_from_shares(int curve, int protocol, const uint8_t* zkey, size_t zlen, const uint8_t* const* files, const size_t* lens,
                            int num_parties, int threshold, uint64_t seed, const uint64_t* r, const uint64_t* s, char* out_json, size_t cap) {
  return entry<Bn254, Bls12_381>(curve, [&](auto tag) {
    using P = decltype(tag);
    if (protocol == 0) {
      if (num_parties != 3 || threshold != 1) throw Error("REP3 only allows three parties and the threshold to be 1");
      sharefile::CompressedRep3SharedWitness<P> sh[3];
      for (int p = 0; p < 3; ++p) sh[p] = sharefile::read_rep3<P>(files[p], lens[p]);
      if (sh[0].kind != sh[1].kind || sh[0].kind != sh[2].kind) throw Error("the parties' share files use different compression");
      return prove_rep3_zkey<P>(zkey, zlen, sh, seed, r, s, out_json, cap, nullptr, 0);
    }
    require_protocol(protocol);
    std::vector<SharedWitness<P, typename P::Fr>> sw;
    for (int p = 0; p < num_parties; ++p) sw.push_back(sharefile::read_shamir<P>(files[p], lens[p]));
    return prove_shamir_zkey<P>(zkey, zlen, sw, threshold, seed, r, s, out_json, cap);
  });
}

// `co-circom translate-witness` (co-circom.rs:925-962, co_circom::translate_witness lib.rs:93-135): the three parties'
// Rep3 `.shared` files -> their 3-party, threshold-1 Shamir `.shared` files. Replicated shares are translated locally
// by translate_primefield_repshare_vec on the device (bridges/rep3_to_shamir.rs:43-62). Additive half shares are first
// completed with one reshare_vec round and then translated the same way -- the reference instead runs a degree
// reduction with fresh Shamir preprocessing (rep3_to_shamir.rs:79-95); both yield valid degree-1 sharings of the same
// witness, the share values are random in either case. Files written back to back into `out`; returns 3 or -1.
int cog16_translate_witness(int curve, const uint8_t* const* files, const size_t* lens, uint8_t* out, size_t cap, size_t* sizes) {
  return entry<Bn254, Bls12_381>(curve, [&](auto tag) {
    using P = decltype(tag);
    using Fr = typename P::Fr;
    std::vector<std::vector<uint8_t>> outs(3);
    sharefile::CompressedRep3SharedWitness<P> sh[3];
    for (int p = 0; p < 3; ++p) sh[p] = sharefile::read_rep3<P>(files[p], lens[p]);
    size_t len[3];
    for (int p = 0; p < 3; ++p) len[p] = sh[p].length();
    if (sh[0].kind != sh[1].kind || sh[0].kind != sh[2].kind) throw Error("the parties' share files use different compression");
    if (len[0] != len[1] || len[0] != len[2]) throw Error("the parties' share files differ in length");
    int dev = 0;
    check(csh_current_device(&dev), "csh_current_device");
    run_parties<1>(3, on_device(dev), [&](int p, const LocalNetwork& net) {
      auto rep = sharefile::uncompress<P>(std::move(sh[p]), net);
      SharedWitness<P, Fr> sw;
      sw.public_inputs = rep.public_inputs;
      sw.witness.resize(rep.witness.size());
      Fr x, y;
      rep3_to_shamir_points(p, x, y);
      if (!rep.witness.empty())
        check(csh_rep3_to_shamir_vec(P::ID, (const uint64_t*)rep.witness.data(), (const uint64_t*)&x, (const uint64_t*)&y,
                                     (uint64_t*)sw.witness.data(), rep.witness.size()), "csh_rep3_to_shamir_vec");
      outs[p] = sharefile::write_shamir<P>(sw);
    });
    return copy_out(outs, out, cap, sizes);
  });
}

int cog16_prove_shamir(int curve, const uint8_t* zkey, size_t zlen, const uint8_t* wtns, size_t wlen, int num_parties, int threshold,
                       uint64_t seed, const uint64_t* r, const uint64_t* s, int bridge, char* out_json, size_t cap) {
  return entry<Bn254, Bls12_381>(curve, [&](auto tag) {
    return prove_shamir_t<decltype(tag)>(zkey, zlen, wtns, wlen, num_parties, threshold, seed, r, s, bridge, out_json, cap);
  });
}

int cog16_prove_plain(int curve, const uint8_t* zkey, size_t zlen, const uint8_t* wtns, size_t wlen, const uint64_t* r, const uint64_t* s,
                      char* out_json, size_t cap, uint64_t* h_out, size_t h_cap_elems) {
  return entry<Bn254, Bls12_381>(curve, [&](auto tag) {
    return prove_plain_t<decltype(tag)>(zkey, zlen, wtns, wlen, r, s, out_json, cap, h_out, h_cap_elems);
  });
}

int cog16_prove_rep3(int curve, const uint8_t* zkey, size_t zlen, const uint8_t* wtns, size_t wlen, uint64_t seed, const uint64_t* r,
                     const uint64_t* s, char* out_json, size_t cap, uint64_t* h_shares_out, size_t h_cap_elems) {
  return entry<Bn254, Bls12_381>(curve, [&](auto tag) {
    return prove_rep3_t<decltype(tag)>(zkey, zlen, wtns, wlen, seed, r, s, out_json, cap, h_shares_out, h_cap_elems);
  });
}

}  // extern "C"
