// The whole sumcheck round of the collaborative UltraHonk prover from a C++ program: three Rep3 parties in one process, each a thread with
// its own LocalNetwork end and Rep3State, run co_compute_round_accumulators_all (all nine relations in the reference's order, every
// stretch of local arithmetic a device stage) and co_batch_over_all_relations of co-snarks_amd/host/plonk_honk.hpp (header-only, above the
// C ABI of include/cosnarks_hip.h) over their shares of the columns read from a file; the program opens the results and writes them to a
// file. The protocol-0 party with the identity network runs on the plain columns beside them.
//
//   clang++ -O1 -std=c++17 examples/honk_co_gates_from_cpp.cpp -Lco-snarks_amd/lib -lcosnarks_hip -Wl,-rpath,co-snarks_amd/lib -lpthread -o honk_co_gates
//   ./honk_co_gates in.bin out.bin
//
// Both files are 64-bit little-endian words; a field element is four of them, arkworks-Montgomery. in.bin: curve (0 BN254, 1 BLS12-381),
// n (a power of two: the round size and the length of every column), log_num_monomials, periodicity, current_element_idx, a seed for the
// sharing; then beta, gamma, public_input_delta, partial_evaluation_result, the log_num_monomials gate challenges, 27 alphas, eta_1,
// eta_2, eta_3, curve_b and the four internal diagonal values, the 36 columns (n each) in the order of csh_honk_sumcheck_accumulate_dev,
// and q_elliptic, q_memory, q_nnf, q_poseidon2_external, q_poseidon2_internal. out.bin: the 57 + 110 opened accumulators of the three
// Rep3 parties over [0, n), the 8 opened values of their round univariate, and the 57 + 110 accumulators of the protocol-0 party.
// tests/test_gpu_honk_co_gates_mirror.py writes one and checks the other.
#include <stdio.h>

#include <vector>

#include "../co-snarks_amd/host/plonk_honk.hpp"

using namespace cosnarks;

namespace {

struct Reader {
  std::vector<uint64_t> words;
  size_t at = 0;
  uint64_t word() {
    if (at >= words.size()) throw Error("input file too short");
    return words[at++];
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

// splitmix64 -> field elements for the sharing: test randomness, not a party's
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

// w_l .. w_4, their shifts and q_m .. q_4 are columns 0 .. 3, 8 .. 11 and 13 .. 18 of the first entry
constexpr size_t GATE_COLUMN_OF[14] = {0, 1, 2, 3, 8, 9, 10, 11, 13, 14, 15, 16, 17, 18};

template <class Fr>
std::vector<std::vector<Fr>> gate_columns(const std::vector<std::vector<Fr>>& cols, const std::vector<std::vector<Fr>>& selectors) {
  std::vector<std::vector<Fr>> g;
  for (size_t c : GATE_COLUMN_OF) g.push_back(cols[c]);
  g.insert(g.end(), selectors.begin(), selectors.end());
  return g;
}

template <class P>
void run(Reader& in, size_t n, FILE* out) {
  using Fr = typename P::Fr;
  HonkGateSeparator<Fr> gs;
  gs.log_num_monomials = in.word(), gs.periodicity = in.word(), gs.current_element_idx = in.word();
  if (gs.log_num_monomials > 28) throw Error("too many gate challenges");
  Sharing sharing{in.word()};
  const std::vector<Fr> head = in.elements<Fr>(4);
  const HonkRelationParameters<Fr> params{head[0], head[1], head[2]};
  gs.partial_evaluation_result = head[3];
  gs.betas = in.elements<Fr>(gs.log_num_monomials);
  const std::vector<Fr> alphas = in.elements<Fr>(HONK_NUM_ALPHAS);
  const std::vector<Fr> g = in.elements<Fr>(8);
  const HonkGateParameters<Fr> gate_params{g[0], g[1], g[2], g[3], {g[4], g[5], g[6], g[7]}};
  std::vector<std::vector<Fr>> cols, selectors;
  for (size_t c = 0; c < HONK_SUMCHECK_COLUMNS; ++c) cols.push_back(in.elements<Fr>(n));
  for (size_t c = 0; c < 5; ++c) selectors.push_back(in.elements<Fr>(n));

  // rep3::share_field_element on every element of the 13 witness columns: party i holds (x_i, x_(i-1))
  std::vector<std::vector<std::vector<Fr>>> party_cols(3, cols);
  for (size_t c = 0; c < 13; ++c) {
    for (auto& pc : party_cols) pc[c].assign(2 * n, Fr::zero());
    for (size_t i = 0; i < n; ++i) {
      const Fr a = sharing.element<Fr>(), b = sharing.element<Fr>(), cc = Fr::sub(Fr::sub(cols[c][i], a), b);
      const Fr x[3] = {a, b, cc};
      for (int p = 0; p < 3; ++p) party_cols[p][c][2 * i] = x[p], party_cols[p][c][2 * i + 1] = x[(p + 2) % 3];
    }
  }
  const std::vector<LocalNetwork> nets = LocalNetwork::new_parties(3);
  std::vector<std::vector<Fr>> acc(3), uni(3);
  {
    std::vector<std::unique_ptr<Joined>> threads;
    for (int p = 0; p < 3; ++p)
      threads.emplace_back(new Joined([&, p]() {
        try {
          uint8_t seed[32];
          for (int k = 0; k < 32; ++k) seed[k] = (uint8_t)(17 * p + k);
          Rep3State st = Rep3State::create(nets[p], seed);
          HonkCoRep3Net net{nets[p], st};
          acc[p] = co_compute_round_accumulators_all<P>(net, party_cols[p], gate_columns(party_cols[p], selectors), 0, n, &gs, params, gate_params);
          uni[p] = co_batch_over_all_relations(acc[p], 2, alphas, gs);
        } catch (...) {
          nets[p].abort();
          throw;
        }
      }));
    for (auto& t : threads) t->join();
  }
  auto open = [](const std::vector<std::vector<Fr>>& shares) {  // the sum of the three a components
    std::vector<Fr> v(shares[0].size() / 2);
    for (size_t i = 0; i < v.size(); ++i) v[i] = Fr::add(Fr::add(shares[0][2 * i], shares[1][2 * i]), shares[2][2 * i]);
    return v;
  };
  const std::vector<Fr> opened = open(acc), univariate = open(uni);
  HonkCoIdentityNet identity;
  const std::vector<Fr> plain = co_compute_round_accumulators_all<P>(identity, cols, gate_columns(cols, selectors), 0, n, &gs, params, gate_params);
  const size_t all = HONK_ACC_ELEMS + HONK_GATES_ACC_ELEMS;
  if (opened.size() != all || univariate.size() != HONK_BATCHED_RELATION_PARTIAL_LENGTH || plain.size() != all) throw Error("unexpected result sizes");
  if (fwrite(opened.data(), 32, opened.size(), out) != opened.size() || fwrite(univariate.data(), 32, univariate.size(), out) != univariate.size() ||
      fwrite(plain.data(), 32, plain.size(), out) != plain.size())
    throw Error("cannot write the output file");
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]);
    return 2;
  }
  try {
    Reader in;
    FILE* f = fopen(argv[1], "rb");
    if (!f) throw Error("cannot open the input file");
    uint64_t w;
    while (fread(&w, 8, 1, f) == 1) in.words.push_back(w);
    fclose(f);
    const uint64_t curve = in.word();
    const size_t n = in.word();
    if (n < 2 || n > (size_t(1) << 20) || (n & (n - 1))) throw Error("n must be a power of two, 2 .. 2^20");
    check(csh_init(0), "csh_init");
    FILE* out = fopen(argv[2], "wb");
    if (!out) throw Error("cannot open the output file");
    if (curve == 0) run<Bn254>(in, n, out);
    else if (curve == 1) run<Bls12_381>(in, n, out);
    else throw Error("unknown curve");
    if (fclose(out) != 0) throw Error("cannot write the output file");
    if (in.at != in.words.size()) throw Error("input file too long");
  } catch (const std::exception& e) {
    fprintf(stderr, "honk_co_gates_from_cpp: %s\n", e.what());
    return 1;
  }
  printf("ok\n");
  return 0;
}
