// Batched Poseidon2 from a C++ program through Poseidon2Hip of co-snarks_amd/host/mpc.hpp (header-only, above the C ABI of
// include/cosnarks_hip.h): the plain batch and a plain Merkle tree; then three Rep3 parties and three Shamir parties (threshold 1), each a
// thread with its own LocalNetwork end and state, run precompute, permutation_in_place_with_precomputation_packed and a collaborative Merkle
// tree over their shares. The program opens the results and writes them to a file.
//
//   clang++ -O1 -std=c++17 examples/poseidon2_from_cpp.cpp -Lco-snarks_amd/lib -lcosnarks_hip -Wl,-rpath,co-snarks_amd/lib -lpthread -o poseidon2
//   ./poseidon2 in.bin out.bin
//   ./poseidon2 --host-loop T N        time permutation_in_place on one host thread over N states (BN254, 4 + 4 external rounds, 56 internal)
//
// Both files are 64-bit little-endian words; a field element is four of them, arkworks-Montgomery. in.bin: curve (0 BN254, 1 BLS12-381), t,
// rounds_f_beginning, rounds_f_end, rounds_p, n_perm, arity, mode (0 sponge, 1 compression), n_leaves, a seed for the sharing; then the
// (rounds_f_beginning + rounds_f_end) t external round constants, the rounds_p internal ones, the t diagonal values, n_perm t state elements
// and n_leaves leaves. out.bin: permutation_packed of the states; permutation_in_place of the states on the host; the plain tree's root;
// then for Rep3 and after it for Shamir: the opened five precomputation vectors (num_sbox n_perm elements each), the opened states after the
// permutation, the opened root. tests/test_gpu_poseidon2_mirror.py writes one and checks the other.
#include <stdio.h>
#include <stdlib.h>

#include <chrono>
#include <vector>

#include "../co-snarks_amd/host/mpc.hpp"

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

// splitmix64 -> field elements for the sharing and the dealt double sharings: test randomness, not a party's
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

struct Shape {
  uint32_t t, rf_b, rf_e, rp, arity, mode;
  size_t n_perm, n_leaves;
};

// what one party brings back: its shares of the precomputation, of the permuted states and of the root
template <class Fr>
struct PartyResult {
  std::vector<Fr> pre[5], states, root;
};

template <class P, class Party>
PartyResult<typename P::Fr> run_party(const Poseidon2Hip<P>& pos, Party& party, const Shape& sh, std::vector<typename P::Fr> states,
                                      const std::vector<typename P::Fr>& leaves) {
  PartyResult<typename P::Fr> out;
  auto pre = pos.precompute(party, sh.n_perm);
  out.pre[0] = pre.r, out.pre[1] = pre.r2, out.pre[2] = pre.r3, out.pre[3] = pre.r4, out.pre[4] = pre.r5;
  pos.permutation_in_place_with_precomputation_packed(party, states, pre);
  if (pre.offset != pos.num_sbox() * sh.n_perm) throw Error("the permutation did not use up its precomputation");
  out.states = std::move(states);
  out.root = pos.merkle_tree_shared(party, leaves, sh.arity, sh.mode);
  return out;
}

template <class Fr, class Open>
void write_opened(const std::vector<PartyResult<Fr>>& res, Open open, FILE* out) {
  std::vector<std::vector<Fr>> all;
  for (int k = 0; k < 5; ++k) all.push_back(open([&](int p) -> const std::vector<Fr>& { return res[p].pre[k]; }));
  all.push_back(open([&](int p) -> const std::vector<Fr>& { return res[p].states; }));
  all.push_back(open([&](int p) -> const std::vector<Fr>& { return res[p].root; }));
  for (auto& v : all)
    if (fwrite(v.data(), 32, v.size(), out) != v.size()) throw Error("cannot write the output file");
}

template <class P>
void run(Reader& in, const Shape& sh, FILE* out) {
  using Fr = typename P::Fr;
  Sharing sharing{in.word()};
  const std::vector<Fr> rc_ext = in.elements<Fr>((size_t)(sh.rf_b + sh.rf_e) * sh.t), rc_int = in.elements<Fr>(sh.rp), diag = in.elements<Fr>(sh.t);
  const std::vector<Fr> states = in.elements<Fr>(sh.n_perm * sh.t), leaves = in.elements<Fr>(sh.n_leaves);
  const Poseidon2Hip<P> pos(sh.t, sh.rf_b, sh.rf_e, sh.rp, rc_ext, rc_int, diag);

  const std::vector<Fr> batch = pos.permutation_packed(states);
  std::vector<Fr> host = states;
  for (size_t i = 0; i < sh.n_perm; ++i) pos.permutation_in_place(&host[i * sh.t]);
  const Fr root = sh.mode == Poseidon2Hip<P>::SPONGE ? pos.merkle_tree_sponge(leaves, sh.arity) : pos.merkle_tree_compression(leaves, sh.arity);
  if (fwrite(batch.data(), 32, batch.size(), out) != batch.size() || fwrite(host.data(), 32, host.size(), out) != host.size() || fwrite(&root, 32, 1, out) != 1)
    throw Error("cannot write the output file");

  const size_t hashes = (sh.n_leaves - 1) / (sh.arity - 1);
  // rep3::share_field_element: party i holds (x_i, x_(i-1))
  auto share_rep3 = [&](const std::vector<Fr>& v) {
    std::vector<std::vector<Fr>> s(3, std::vector<Fr>(2 * v.size()));
    for (size_t i = 0; i < v.size(); ++i) {
      const Fr a = sharing.element<Fr>(), b = sharing.element<Fr>(), x[3] = {a, b, Fr::sub(Fr::sub(v[i], a), b)};
      for (int p = 0; p < 3; ++p) s[p][2 * i] = x[p], s[p][2 * i + 1] = x[(p + 2) % 3];
    }
    return s;
  };
  {
    const auto st_sh = share_rep3(states), lf_sh = share_rep3(leaves);
    const std::vector<LocalNetwork> nets = LocalNetwork::new_parties(3);
    std::vector<PartyResult<Fr>> res(3);
    std::vector<std::unique_ptr<Joined>> threads;
    for (int p = 0; p < 3; ++p)
      threads.emplace_back(new Joined([&, p]() {
        try {
          uint8_t seed[32];
          for (int k = 0; k < 32; ++k) seed[k] = (uint8_t)(17 * p + k);
          Rep3State st = Rep3State::create(nets[p], seed);
          Poseidon2Rep3Party<P> party{nets[p], st};
          res[p] = run_party(pos, party, sh, st_sh[p], lf_sh[p]);
        } catch (...) {
          nets[p].abort();
          throw;
        }
      }));
    for (auto& t : threads) t->join();
    write_opened<Fr>(res, [](auto of) {  // the sum of the three a components
      std::vector<Fr> v(of(0).size() / 2);
      for (size_t i = 0; i < v.size(); ++i) v[i] = Fr::add(Fr::add(of(0)[2 * i], of(1)[2 * i]), of(2)[2 * i]);
      return v;
    }, out);
  }
  {
    // shamir::share_field_element, threshold 1: party k holds f(k + 1), f = x + c X. A double sharing is the same r at degree 1 and degree 2.
    auto share_shamir = [&](const std::vector<Fr>& v) {
      std::vector<std::vector<Fr>> s(3, std::vector<Fr>(v.size()));
      for (size_t i = 0; i < v.size(); ++i) {
        const Fr c = sharing.element<Fr>();
        Fr acc = v[i];
        for (int p = 0; p < 3; ++p) s[p][i] = acc = Fr::add(acc, c);
      }
      return s;
    };
    const auto st_sh = share_shamir(states), lf_sh = share_shamir(leaves);
    const size_t pairs = 5 * pos.num_sbox() * (sh.n_perm + hashes);  // per precomputation: one draw and four products per s-box
    std::vector<std::deque<std::pair<Fr, Fr>>> dealt(3);
    for (size_t i = 0; i < pairs; ++i) {
      const Fr r = sharing.element<Fr>(), c1 = sharing.element<Fr>(), d1 = sharing.element<Fr>(), d2 = sharing.element<Fr>();
      for (int p = 0; p < 3; ++p) {
        const Fr x = Fr::from_u64(p + 1);
        dealt[p].push_back({Fr::add(r, Fr::mul(c1, x)), Fr::add(r, Fr::mul(x, Fr::add(d1, Fr::mul(d2, x))))});
      }
    }
    const std::vector<LocalNetwork> nets = LocalNetwork::new_parties(3);
    std::vector<PartyResult<Fr>> res(3);
    std::vector<std::unique_ptr<Joined>> threads;
    for (int p = 0; p < 3; ++p)
      threads.emplace_back(new Joined([&, p]() {
        try {
          ShamirState<Fr> st = ShamirState<Fr>::create(p, 3, 1, dealt[p]);
          Poseidon2ShamirParty<P> party{nets[p], st};
          res[p] = run_party(pos, party, sh, st_sh[p], lf_sh[p]);
          if (!st.rng_buffer.empty()) throw Error("the Shamir party did not use up its double sharings");
        } catch (...) {
          nets[p].abort();
          throw;
        }
      }));
    for (auto& t : threads) t->join();
    write_opened<Fr>(res, [](auto of) {  // degree 1 through the points 1 and 2: f(0) = 2 f(1) - f(2); party 2's share lies on the same line
      std::vector<Fr> v(of(0).size());
      for (size_t i = 0; i < v.size(); ++i) {
        v[i] = Fr::sub(Fr::add(of(0)[i], of(0)[i]), of(1)[i]);
        if (!(Fr::sub(Fr::add(of(1)[i], of(1)[i]), of(0)[i]) == of(2)[i]))  // f(3) = 2 f(2) - f(1)
          throw Error("the three Shamir shares do not lie on one line");
      }
      return v;
    }, out);
  }
  // the one-party form: the values themselves through the same rounds
  {
    uint8_t seed[32];
    for (int k = 0; k < 32; ++k) seed[k] = (uint8_t)(91 + k);
    Poseidon2PlainParty<P> party(seed);
    const PartyResult<Fr> one = run_party(pos, party, sh, states, leaves);
    if (!(one.states == batch) || !(one.root[0] == root)) throw Error("the one-party rounds differ from the plain batch");
  }
}

int host_loop(uint32_t t, size_t n) {
  using Fr = Bn254::Fr;
  if (t < 2 || t > 4 || n < 1 || n > (size_t(1) << 24)) throw Error("--host-loop: t must be 2, 3 or 4, n 1 .. 2^24");
  Sharing g{12345};
  std::vector<Fr> rc_ext(8 * t), rc_int(56), diag(t), states(n * t);
  for (auto* v : {&rc_ext, &rc_int, &diag, &states})
    for (auto& x : *v) x = g.element<Fr>();
  if (t < 4) {
    for (auto& x : diag) x = Fr::one();
    diag[t - 1] = Fr::from_u64(2);
  }
  const Poseidon2Hip<Bn254> pos(t, 4, 4, 56, rc_ext, rc_int, diag);
  const auto t0 = std::chrono::steady_clock::now();
  for (size_t i = 0; i < n; ++i) pos.permutation_in_place(&states[i * t]);
  const double ns = std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count();
  Fr sum = Fr::zero();
  for (auto& x : states) sum = Fr::add(sum, x);
  printf("host_loop t=%u n=%zu ns_per_permutation=%.1f check=%08x\n", t, n, ns / (double)n, (unsigned)sum.l[0]);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  try {
    if (argc == 4 && std::string(argv[1]) == "--host-loop") {
      check(csh_init(0), "csh_init");
      return host_loop((uint32_t)strtoul(argv[2], nullptr, 10), (size_t)strtoull(argv[3], nullptr, 10));
    }
    if (argc != 3) {
      fprintf(stderr, "usage: %s in.bin out.bin | --host-loop T N\n", argv[0]);
      return 2;
    }
    Reader in;
    FILE* f = fopen(argv[1], "rb");
    if (!f) throw Error("cannot open the input file");
    uint64_t w;
    while (fread(&w, 8, 1, f) == 1) in.words.push_back(w);
    fclose(f);
    const uint64_t curve = in.word();
    Shape sh;
    sh.t = (uint32_t)in.word(), sh.rf_b = (uint32_t)in.word(), sh.rf_e = (uint32_t)in.word(), sh.rp = (uint32_t)in.word();
    sh.n_perm = in.word(), sh.arity = (uint32_t)in.word(), sh.mode = (uint32_t)in.word(), sh.n_leaves = in.word();
    if (sh.t < 2 || sh.t > 4 || sh.rf_b > 64 || sh.rf_e > 64 || sh.rp > 256 || sh.n_perm < 1 || sh.n_perm > 4096 || sh.arity < 2 || sh.arity > 4 ||
        sh.n_leaves < sh.arity || sh.n_leaves > 4096)
      throw Error("shape out of range");
    check(csh_init(0), "csh_init");
    FILE* out = fopen(argv[2], "wb");
    if (!out) throw Error("cannot open the output file");
    if (curve == 0) run<Bn254>(in, sh, out);
    else if (curve == 1) run<Bls12_381>(in, sh, out);
    else throw Error("unknown curve");
    if (fclose(out) != 0) throw Error("cannot write the output file");
    if (in.at != in.words.size()) throw Error("input file too long");
  } catch (const std::exception& e) {
    fprintf(stderr, "poseidon2_from_cpp: %s\n", e.what());
    return 1;
  }
  printf("ok\n");
  return 0;
}
