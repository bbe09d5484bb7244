// The host mirror's Oink phase of UltraHonk from a C++ program: PlainPlonkDriver::compute_w4, compute_logderivative_inverses and
// compute_grand_product of co-snarks_amd/host/plonk_honk.hpp (header-only, above the C ABI of include/cosnarks_hip.h) on data read from a
// file, results to a file.
//
//   clang++ -O1 -std=c++17 examples/honk_oink_from_cpp.cpp -Lco-snarks_amd/lib -lcosnarks_hip -Wl,-rpath,co-snarks_amd/lib -lpthread -o honk_oink
//   ./honk_oink in.bin out.bin
//
// Both files are 64-bit little-endian words; a field element is four of them, arkworks-Montgomery. in.bin: curve (0 BN254, 1 BLS12-381),
// n, final_active_wire_idx, the length of w_4, the number of active ranges and the ranges (start, end each), the numbers of read, write
// and shared memory records and their rows (one word each), the type shares of the shared records; then w_l, w_r, w_o (n each), w_4,
// lookup_read_tags, q_r, q_m, q_c, q_o, table_1 .. table_4, q_lookup, id_1 .. id_4, sigma_1 .. sigma_4 (n each), eta_1, eta_2, eta_3, beta,
// gamma. out.bin: memory.w_4, lookup_inverses, z_perm (n each). tests/test_gpu_honk_oink_mirror.py writes one and checks the other.
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
  std::vector<uint32_t> rows(size_t count) {
    std::vector<uint32_t> v;
    for (size_t i = 0; i < count; ++i) v.push_back((uint32_t)word());
    return v;
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
  HonkOinkInputs<Fr> k;
  k.circuit_size = n;
  k.final_active_wire_idx = in.word();
  const size_t w4_len = in.word(), num_ranges = in.word();
  if (num_ranges > n) throw Error("too many ranges");
  for (size_t r = 0; r < num_ranges; ++r) {
    const size_t start = in.word(), end = in.word();
    k.active_ranges.push_back({start, end});
  }
  const size_t n_read = in.word(), n_write = in.word(), n_shared = in.word();
  if (n_read > n || n_write > n || n_shared > n) throw Error("too many memory records");
  k.memory_read_records = in.rows(n_read), k.memory_write_records = in.rows(n_write);
  const std::vector<uint32_t> shared_rows = in.rows(n_shared);
  for (uint32_t row : shared_rows) k.memory_records_shared.push_back({row, in.element<Fr>()});
  k.w_l = in.elements<Fr>(n), k.w_r = in.elements<Fr>(n), k.w_o = in.elements<Fr>(n), k.w_4 = in.elements<Fr>(w4_len);
  for (std::vector<Fr>* v : {&k.lookup_read_tags, &k.q_r, &k.q_m, &k.q_c, &k.q_o, &k.table_1, &k.table_2, &k.table_3, &k.table_4, &k.q_lookup}) *v = in.elements<Fr>(n);
  for (auto& v : k.id) v = in.elements<Fr>(n);
  for (auto& v : k.sigma) v = in.elements<Fr>(n);
  for (Fr* e : {&k.eta_1, &k.eta_2, &k.eta_3, &k.beta, &k.gamma}) *e = in.element<Fr>();

  const std::vector<Fr> w_4 = PlainPlonkDriver<P>::compute_w4(k);
  const std::vector<Fr> lookup_inverses = PlainPlonkDriver<P>::compute_logderivative_inverses(k);
  const std::vector<Fr> z_perm = PlainPlonkDriver<P>::compute_grand_product(k, w_4);
  for (const std::vector<Fr>* v : {&w_4, &lookup_inverses, &z_perm})
    if (fwrite(v->data(), 32, v->size(), out) != v->size()) throw Error("cannot write the output file");
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
    check(csh_init(0), "csh_init");
    FILE* out = fopen(argv[2], "wb");
    if (!out) throw Error("cannot open the output file");
    if (curve == 0) run<Bn254>(in, n, out);
    else if (curve == 1) run<Bls12_381>(in, n, out);
    else throw Error("unknown curve");
    if (fclose(out) != 0) throw Error("cannot write the output file");
    if (in.at != in.words.size()) throw Error("input file too long");
  } catch (const std::exception& e) {
    fprintf(stderr, "honk_oink_from_cpp: %s\n", e.what());
    return 1;
  }
  printf("ok\n");
  return 0;
}
