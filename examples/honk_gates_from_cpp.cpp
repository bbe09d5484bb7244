// The host mirror's complete sumcheck round of UltraHonk from a C++ program: PlainPlonkDriver::compute_round_accumulators_gates (the
// elliptic, memory, non-native field and Poseidon2 relations, csh_honk_sumcheck_accumulate_gates_dev) and compute_univariate_all (both
// device entries, then the reference's batching over all 28 accumulators with 27 alphas) of co-snarks_amd/host/plonk_honk.hpp
// (header-only, above the C ABI of include/cosnarks_hip.h) on data read from a file, results to a file, with the plain C++ loop of the
// same five relations beside them.
//
//   clang++ -O1 -std=c++17 examples/honk_gates_from_cpp.cpp -Lco-snarks_amd/lib -lcosnarks_hip -Wl,-rpath,co-snarks_amd/lib -lpthread -o honk_gates
//   ./honk_gates in.bin out.bin
//
// Both files are 64-bit little-endian words; a field element is four of them, arkworks-Montgomery. in.bin: curve (0 BN254, 1 BLS12-381),
// n (a power of two: the round size and the length of every column), edge_begin, edge_end, log_num_monomials, periodicity,
// current_element_idx; then beta, gamma, public_input_delta, partial_evaluation_result, the log_num_monomials gate challenges, 27
// alphas, eta_1, eta_2, eta_3, curve_b and the four internal diagonal values, the 36 columns (n each) in the order of
// csh_honk_sumcheck_accumulate_dev, and q_elliptic, q_memory, q_nnf, q_poseidon2_external, q_poseidon2_internal. out.bin: the 110
// accumulator elements of [edge_begin, edge_end) from the device, the same 110 from the plain C++ loop, the 8 values of the round
// univariate over [0, n), and the host loop's time as one word of microseconds. tests/test_gpu_honk_gates_mirror.py writes one and
// checks the other.
#include <stdio.h>

#include <chrono>
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
  Fr element() {
    if (at + 4 > words.size()) throw Error("input file too short");
    Fr x;
    memcpy((void*)&x, &words[at], 32);
    at += 4;
    return x;
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

template <class P>
void run(Reader& in, size_t n, FILE* out) {
  using Fr = typename P::Fr;
  const size_t edge_begin = in.word(), edge_end = in.word();
  HonkGateSeparator<Fr> gs;
  gs.log_num_monomials = in.word(), gs.periodicity = in.word(), gs.current_element_idx = in.word();
  if (gs.log_num_monomials > 28) throw Error("too many gate challenges");
  HonkRelationParameters<Fr> params;
  params.beta = in.element<Fr>(), params.gamma = in.element<Fr>(), params.public_input_delta = in.element<Fr>();
  gs.partial_evaluation_result = in.element<Fr>();
  gs.betas = in.elements<Fr>(gs.log_num_monomials);
  const std::vector<Fr> alphas = in.elements<Fr>(HONK_NUM_ALPHAS);
  HonkGateParameters<Fr> gate_params;
  gate_params.eta_1 = in.element<Fr>(), gate_params.eta_2 = in.element<Fr>(), gate_params.eta_3 = in.element<Fr>(), gate_params.curve_b = in.element<Fr>();
  for (auto& d : gate_params.mat_internal_diag_m_1) d = in.element<Fr>();
  std::vector<std::vector<Fr>> cols, gate_cols;
  for (size_t c = 0; c < HONK_SUMCHECK_COLUMNS; ++c) cols.push_back(in.elements<Fr>(n));
  // w_l .. w_4, their shifts and q_m .. q_4 are columns 0 .. 3, 8 .. 11 and 13 .. 18 of the first entry
  for (size_t c : {0, 1, 2, 3, 8, 9, 10, 11, 13, 14, 15, 16, 17, 18}) gate_cols.push_back(cols[c]);
  for (size_t c = 0; c < 5; ++c) gate_cols.push_back(in.elements<Fr>(n));

  const HonkGateAccumulators<Fr> dev = PlainPlonkDriver<P>::compute_round_accumulators_gates(gate_cols, edge_begin, edge_end, &gs, gate_params);
  const auto t0 = std::chrono::steady_clock::now();
  const HonkGateAccumulators<Fr> host = detail::host_round_accumulators_gates(gate_cols, edge_begin, edge_end, &gs, gate_params);
  const uint64_t host_us = (uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
  const auto univariate = PlainPlonkDriver<P>::compute_univariate_all(cols, gate_cols, n, gs, params, gate_params, alphas);
  if (fwrite(dev.data(), 32, dev.size(), out) != dev.size() || fwrite(host.data(), 32, host.size(), out) != host.size() ||
      fwrite(univariate.data(), 32, univariate.size(), out) != univariate.size() || fwrite(&host_us, 8, 1, out) != 1)
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
    if (n < 2 || n > (size_t(1) << 28)) throw Error("n must be 2 .. 2^28");
    check(csh_init(0), "csh_init");
    FILE* out = fopen(argv[2], "wb");
    if (!out) throw Error("cannot open the output file");
    if (curve == 0) run<Bn254>(in, n, out);
    else if (curve == 1) run<Bls12_381>(in, n, out);
    else throw Error("unknown curve");
    if (fclose(out) != 0) throw Error("cannot write the output file");
    if (in.at != in.words.size()) throw Error("input file too long");
  } catch (const std::exception& e) {
    fprintf(stderr, "honk_gates_from_cpp: %s\n", e.what());
    return 1;
  }
  printf("ok\n");
  return 0;
}
