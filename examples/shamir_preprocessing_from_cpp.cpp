// Shamir preprocessing from a C++ program through ShamirPreprocessingHip of co-snarks_amd/host/mpc.hpp (header-only, above the C ABI of
// include/cosnarks_hip.h): n parties with threshold t, each a thread with its own LocalNetwork end, exchange the seeds of their shared
// streams, generate DN07 double sharings on the device and hand them to the host ShamirState; the program opens every pair from its
// degree-t and from its degree-2t shares (they must agree), forks one pair off, runs one mul_vec on generated pairs through the Shamir party of the Poseidon2
// mirror and opens the product. It then expands a seeded share on the device (SeededShare::expand_dev) and on the host (expand()).
//
//   clang++ -O1 -std=c++17 examples/shamir_preprocessing_from_cpp.cpp -Lco-snarks_amd/lib -lcosnarks_hip -Wl,-rpath,co-snarks_amd/lib -lpthread -o shamir_pre
//   ./shamir_pre in.bin out.bin
//   ./shamir_pre --host-loop N     time SeededShare::expand() and a host buffer_triples (3 parties, t = 1) of N draws / N pairs on one thread (BN254)
//
// Both files are 64-bit little-endian words; a field element is four of them, arkworks-Montgomery. in.bin: curve (0 BN254, 1 BLS12-381),
// num_parties, threshold, amount (pairs wanted), m (length of the product), seeded_len, the 32-byte master seed (party p's own generator is
// seeded with candidate p of its stream), the 32-byte seed of the seeded share, then m elements a and m elements b. out.bin: the opened
// pairs in buffer order (amount.div_ceil(t + 1) * (t + 1) elements), the opened product (m), the expanded share (seeded_len), the t + 1
// opened pairs that a fork of one pair (fork_with_pairs) generated from its own streams.
// tests/test_gpu_shamir_rng_mirror.py writes one and checks the other.
#include <stdio.h>
#include <stdlib.h>

#include <chrono>
#include <vector>

#include "../co-snarks_amd/host/sharefile.hpp"

using namespace cosnarks;

namespace {

struct Reader {
  std::vector<uint64_t> words;
  size_t at = 0;
  uint64_t word() {
    if (at >= words.size()) throw Error("input file too short");
    return words[at++];
  }
  void bytes32(uint8_t out[32]) {
    for (int k = 0; k < 4; ++k) {
      const uint64_t w = word();
      memcpy(out + 8 * k, &w, 8);
    }
  }
  template <class Fr>
  std::vector<Fr> elements(size_t count) {
    if (count > (words.size() - at) / 4) throw Error("input file too short");
    std::vector<Fr> v(count);
    if (count) memcpy((void*)v.data(), &words[at], 32 * count);
    at += 4 * count;
    return v;
  }
};

// splitmix64 -> the coefficients of the input sharing: test randomness, not a party's
struct Sharing {
  uint64_t s;
  uint64_t next() {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  template <class Fr>
  Fr element() {
    return Fr::add(Fr::mul(Fr::mul(Fr::from_u64(next()), Fr::from_u64(next())), Fr::mul(Fr::from_u64(next()), Fr::from_u64(next()))), Fr::from_u64(next()));
  }
};

template <class Fr>
void write_elements(FILE* out, const std::vector<Fr>& v) {
  if (!v.empty() && fwrite(v.data(), sizeof(Fr), v.size(), out) != v.size()) throw Error("cannot write the output file");
}

// sum_i lagrange_i shares[ids_i][k]: the value at 0 of the polynomial through the parties `first .. first + count - 1` (points id + 1)
template <class Fr>
std::vector<Fr> open_from(const std::vector<std::vector<Fr>>& shares, size_t first, size_t count) {
  std::vector<size_t> pts;
  for (size_t i = 0; i < count; ++i) pts.push_back(first + i + 1);
  const std::vector<Fr> lag = lagrange_from_coeff<Fr>(pts);
  std::vector<Fr> v(shares[first].size(), Fr::zero());
  for (size_t i = 0; i < count; ++i)
    for (size_t k = 0; k < v.size(); ++k) v[k] = Fr::add(v[k], Fr::mul(lag[i], shares[first + i][k]));
  return v;
}

template <class P>
void run(Reader& in, size_t n, size_t t, size_t amount, size_t m, size_t seeded_len, FILE* out) {
  using Fr = typename P::Fr;
  uint8_t master[32], share_seed[32];
  in.bytes32(master);
  in.bytes32(share_seed);
  const std::vector<Fr> a = in.template elements<Fr>(m), b = in.template elements<Fr>(m);
  const size_t pairs = (amount + t) / (t + 1) * (t + 1);
  if (m + 1 > pairs) throw Error("the product is longer than the pairs left after the fork");
  // degree-t input sharings
  Sharing sharing{n * 1000 + t};
  std::vector<std::vector<Fr>> sa(n, std::vector<Fr>(m)), sb(n, std::vector<Fr>(m));
  for (const auto& pr : {std::make_pair(&a, &sa), std::make_pair(&b, &sb)})
    for (size_t k = 0; k < m; ++k) {
      std::vector<Fr> poly{(*pr.first)[k]};
      for (size_t d = 0; d < t; ++d) poly.push_back(sharing.element<Fr>());
      for (size_t p = 0; p < n; ++p) {
        Fr e = Fr::zero();
        for (size_t d = poly.size(); d-- > 0;) e = Fr::add(Fr::mul(e, Fr::from_u64(p + 1)), poly[d]);
        (*pr.second)[p][k] = e;
      }
    }
  const std::vector<LocalNetwork> nets = LocalNetwork::new_parties((int)n);
  std::vector<std::vector<Fr>> r_t(n), r_2t(n), prod(n), kid_t(n), kid_2t(n);
  std::vector<std::unique_ptr<Joined>> threads;
  for (size_t p = 0; p < n; ++p)
    threads.emplace_back(new Joined([&, p]() {
      try {
        uint8_t own[32];
        uint64_t pos = p;
        ShamirPreprocessingHip<P>::gen_seed(master, pos, own);
        ShamirPreprocessingHip<P> pre = ShamirPreprocessingHip<P>::create(nets[p], n, t, amount, own);
        if (pre.len() != pairs) throw Error("ShamirPreprocessing::new did not generate amount.div_ceil(t + 1) batches");
        // fork_with_pairs: the child takes the first pair and new streams, and generates one batch item of its own
        ShamirPreprocessingHip<P> kid = pre.fork(1);
        if (kid.len() != 1 || pre.len() != pairs - 1) throw Error("fork did not move one pair");
        kid.buffer_triples(nets[p], 1);
        ShamirState<Fr> kid_st = kid.into_state();
        for (auto& pr : kid_st.rng_buffer) kid_t[p].push_back(pr.first), kid_2t[p].push_back(pr.second);
        ShamirState<Fr> st = pre.into_state();
        r_t[p].push_back(kid_t[p][0]), r_2t[p].push_back(kid_2t[p][0]);  // buffer order: the forked pair was the first
        for (auto& pr : st.rng_buffer) r_t[p].push_back(pr.first), r_2t[p].push_back(pr.second);
        Poseidon2ShamirParty<P> party{nets[p], st};
        prod[p] = party.mul_vec(sa[p], sb[p]);
        if (st.rng_buffer.size() != pairs - 1 - m) throw Error("mul_vec did not consume one pair per product");
      } catch (...) {
        nets[p].abort();
        throw;
      }
    }));
  for (auto& th : threads) th->join();
  // every pair opens alike from t + 1 degree-t shares, from another t + 1 of them, and from 2t + 1 degree-2t shares
  const std::vector<Fr> opened = open_from(r_t, 0, t + 1);
  if (!(open_from(r_t, n - t - 1, t + 1) == opened) || !(open_from(r_2t, 0, 2 * t + 1) == opened) || !(open_from(r_2t, n - 2 * t - 1, 2 * t + 1) == opened))
    throw Error("a generated pair does not open to one value");
  write_elements(out, opened);
  const std::vector<Fr> product = open_from(prod, 0, t + 1);
  if (!(open_from(prod, n - t - 1, t + 1) == product)) throw Error("the product's shares do not lie on one polynomial of degree t");
  write_elements(out, product);
  // a seeded share on the device and on the host
  sharefile::SeededShare<Fr> seeded;
  seeded.is_seed = true, seeded.len = seeded_len;
  memcpy(seeded.seed, share_seed, 32);
  typename ShamirPreprocessingHip<P>::Dev dev(sizeof(Fr) * seeded_len);
  seeded.expand_dev(P::ID, dev.w(), nullptr);
  std::vector<Fr> on_dev(seeded_len);
  if (seeded_len) check(csh_memcpy_d2h(on_dev.data(), dev.p, sizeof(Fr) * seeded_len), "csh_memcpy_d2h");
  if (!(on_dev == seeded.expand())) throw Error("expand_dev differs from expand()");
  write_elements(out, on_dev);
  // the fork's pairs: the inherited one and the t + 1 it generated from its own streams
  const std::vector<Fr> kid_opened = open_from(kid_t, 0, t + 1);
  if (kid_opened.size() != t + 2 || !(open_from(kid_2t, n - 2 * t - 1, 2 * t + 1) == kid_opened) || !(kid_opened[0] == opened[0]))
    throw Error("the fork's pairs do not open to one value");
  write_elements(out, std::vector<Fr>(kid_opened.begin() + 1, kid_opened.end()));
}

// the mirror's host loops on one thread: what a caller of the mirror gains from the device path (not what a Rust caller would)
int host_loop(size_t count) {
  using Fr = Bn254::Fr;
  if (count < 1 || count > (size_t(1) << 24)) throw Error("--host-loop: N must be 1 .. 2^24");
  sharefile::SeededShare<Fr> seeded;
  seeded.is_seed = true, seeded.len = count;
  for (int k = 0; k < 32; ++k) seeded.seed[k] = (uint8_t)(17 + k);
  auto t0 = std::chrono::steady_clock::now();
  const std::vector<Fr> v = seeded.expand();
  const double expand_ns = std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count();
  // buffer_triples of one party of three with t = 1 for count / 2 batch items: 8 batches of draws, polys of degree 1 and 2, a 2 x 3 matrix
  const size_t items = (count + 1) / 2;
  sharefile::SeededShare<Fr> draws = seeded;
  draws.len = 8 * items;
  t0 = std::chrono::steady_clock::now();
  const std::vector<Fr> d = draws.expand();
  const Fr two = Fr::from_u64(2), three = Fr::from_u64(3);
  Fr sum = Fr::zero();
  for (size_t i = 0; i < items; ++i) {
    Fr rcv_t[3] = {d[i], d[items + i], Fr::add(d[2 * items + i], Fr::mul(two, d[3 * items + i]))};
    Fr rcv_2t[3] = {d[4 * items + i], d[5 * items + i], Fr::add(d[6 * items + i], Fr::mul(three, d[7 * items + i]))};
    for (auto* rcv : {rcv_t, rcv_2t}) {
      sum = Fr::add(sum, Fr::add(Fr::add(rcv[0], rcv[1]), rcv[2]));
      sum = Fr::add(sum, Fr::add(Fr::add(rcv[0], Fr::mul(two, rcv[1])), Fr::mul(three, rcv[2])));
    }
  }
  const double triples_ns = std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count();
  printf("host_loop n=%zu expand_ns_per_draw=%.1f buffer_triples_ns_per_pair=%.1f check=%08x\n", count, expand_ns / (double)count,
         triples_ns / (double)(2 * items), (unsigned)(sum.l[0] ^ v[0].l[0]));
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  try {
    if (argc == 3 && std::string(argv[1]) == "--host-loop") return host_loop((size_t)strtoull(argv[2], nullptr, 10));
    if (argc != 3) {
      fprintf(stderr, "usage: %s in.bin out.bin | --host-loop N\n", argv[0]);
      return 2;
    }
    Reader in;
    FILE* f = fopen(argv[1], "rb");
    if (!f) throw Error("cannot open the input file");
    uint64_t w;
    while (fread(&w, 8, 1, f) == 1) in.words.push_back(w);
    fclose(f);
    const uint64_t curve = in.word();
    const size_t n = in.word(), t = in.word(), amount = in.word(), m = in.word(), seeded_len = in.word();
    if (n < 3 || n > 16 || t < 1 || amount < 1 || amount > 65536 || m > 4096 || seeded_len > 65536) throw Error("shape out of range");
    check(csh_init(0), "csh_init");
    FILE* out = fopen(argv[2], "wb");
    if (!out) throw Error("cannot open the output file");
    if (curve == 0) run<Bn254>(in, n, t, amount, m, seeded_len, out);
    else if (curve == 1) run<Bls12_381>(in, n, t, amount, m, seeded_len, out);
    else throw Error("unknown curve");
    if (fclose(out) != 0) throw Error("cannot write the output file");
    if (in.at != in.words.size()) throw Error("input file too long");
  } catch (const std::exception& e) {
    fprintf(stderr, "shamir_preprocessing_from_cpp: %s\n", e.what());
    return 1;
  }
  printf("ok\n");
  return 0;
}
