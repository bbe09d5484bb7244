// The host mirror's PLONK rounds 2 and 5 from a C++ program: PlainPlonkDriver::compute_z, compute_r_wxi and compute_wxiw of
// co-snarks_amd/host/plonk_honk.hpp (header-only, above the C ABI of include/cosnarks_hip.h) on data read from a file, results to a file.
//
//   clang++ -O1 -std=c++17 examples/plonk_rounds_from_cpp.cpp -Lco-snarks_amd/lib -lcosnarks_hip -Wl,-rpath,co-snarks_amd/lib -lpthread -o plonk_rounds
//   ./plonk_rounds in.bin out.bin
//
// Both files are 64-bit little-endian words; a field element is four of them, arkworks-Montgomery. in.bin: curve (0 BN254, 1 BLS12-381),
// n, n_public; then, for round 2, buffer_a, buffer_b, buffer_c (n each), the evaluations of S1, S2, S3 (4 n each), beta, gamma, k1, k2,
// b7, b8, b9; then, for round 5, the coefficients of z (n + 3), t1, t2 (n + 1), t3 (n + 6), a, b, c (n + 2), of qm, ql, qr, qo, qc, s1,
// s2, s3 (n each), the public inputs (n_public), the evaluations a, b, c, s1, s2, zw, then alpha, xi, v1 .. v5. out.bin: the blinded
// z(X) of compute_z (n + 3), its 4 n evaluations, W_xi (n + 5), W_xiw (n + 2). tests/test_gpu_plonk_mirror.py writes one and checks the other.
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
void run(Reader& in, size_t n, size_t n_public, FILE* out) {
  using Fr = typename P::Fr;
  PlonkRound2Inputs<Fr> r2;
  r2.buffer_a = in.elements<Fr>(n), r2.buffer_b = in.elements<Fr>(n), r2.buffer_c = in.elements<Fr>(n);
  r2.s1 = in.elements<Fr>(4 * n), r2.s2 = in.elements<Fr>(4 * n), r2.s3 = in.elements<Fr>(4 * n);
  r2.beta = in.element<Fr>(), r2.gamma = in.element<Fr>(), r2.k1 = in.element<Fr>(), r2.k2 = in.element<Fr>();
  for (Fr& b : r2.blinders) b = in.element<Fr>();
  PlonkRound5Inputs<Fr> r5;
  r5.domain_size = n;
  r5.z = in.elements<Fr>(n + 3), r5.t1 = in.elements<Fr>(n + 1), r5.t2 = in.elements<Fr>(n + 1), r5.t3 = in.elements<Fr>(n + 6);
  r5.a = in.elements<Fr>(n + 2), r5.b = in.elements<Fr>(n + 2), r5.c = in.elements<Fr>(n + 2);
  for (std::vector<Fr>* q : {&r5.qm, &r5.ql, &r5.qr, &r5.qo, &r5.qc, &r5.s1, &r5.s2, &r5.s3}) *q = in.elements<Fr>(n);
  r5.public_inputs = in.elements<Fr>(n_public);
  for (Fr* e : {&r5.eval_a, &r5.eval_b, &r5.eval_c, &r5.eval_s1, &r5.eval_s2, &r5.eval_zw, &r5.alpha, &r5.xi}) *e = in.element<Fr>();
  for (Fr& v : r5.v) v = in.element<Fr>();
  r5.beta = r2.beta, r5.gamma = r2.gamma, r5.k1 = r2.k1, r5.k2 = r2.k2;

  const PlonkDomains<P> domains(n);
  const PlonkPolyEval<Fr> z = PlainPlonkDriver<P>::compute_z(domains, r2);
  const std::vector<Fr> wxi = PlainPlonkDriver<P>::compute_r_wxi(r5), wxiw = PlainPlonkDriver<P>::compute_wxiw(r5);
  for (const std::vector<Fr>* v : {&z.poly, &z.eval, &wxi, &wxiw})
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
    const size_t n = in.word(), n_public = in.word();
    check(csh_init(0), "csh_init");
    FILE* out = fopen(argv[2], "wb");
    if (!out) throw Error("cannot open the output file");
    if (curve == 0) run<Bn254>(in, n, n_public, out);
    else if (curve == 1) run<Bls12_381>(in, n, n_public, out);
    else throw Error("unknown curve");
    if (fclose(out) != 0) throw Error("cannot write the output file");
    if (in.at != in.words.size()) throw Error("input file too long");
  } catch (const std::exception& e) {
    fprintf(stderr, "plonk_rounds_from_cpp: %s\n", e.what());
    return 1;
  }
  printf("ok\n");
  return 0;
}
