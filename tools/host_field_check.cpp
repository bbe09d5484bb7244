// Stand-alone check and timing of the host field of the MSM fold (co-snarks_amd/csrc/host_fp64.hpp). No HIP, no library:
//
//   clang++ -O2 -std=c++17 -o host_field_check tools/host_field_check.cpp && ./host_field_check
//   clang++ -O1 -g -std=c++17 -fsanitize=address,undefined -o host_field_check_san tools/host_field_check.cpp && ./host_field_check_san
// (clang, or GCC from 14: field.hpp uses __builtin_addc; ROCm's clang++ will do. An optional argument is the number of random pairs.)
//
// For BN254 Fq / Fr (4 limbs) and BLS12-381 / BLS12-377 Fq (6 limbs): mul, sqr and inv against the looped CIOS kept beside them
// (mul_looped, inv_looped): mul and sqr on 10^5 random pairs, inv on every 100th of them (10^3 values, ~400 products each, also
// checked by inv(a) a = 1), all three on every pair of the edge values 0, 1, p - 1, R mod p; mul with an unreduced
// left operand (all words 2^64 - 1: the from-bytes reduction of host/network.hpp); then ns per operation of a dependent chain,
// the shape of the fold. Exit status 0: every word equal.
#include <stdio.h>
#include <stdlib.h>

#include <chrono>

#include "../co-snarks_amd/csrc/host_fp64.hpp"

namespace {

uint64_t rng_state = 0x9e3779b97f4a7c15ull;
uint64_t next64() {  // splitmix64
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

template <class F>
F random_elem() {  // uniform below 2^(bits of p), rejected until below p
  F r;
  int top_bits = 64;
  while (top_bits > 0 && !((F::K.mod[F::N - 1] >> (top_bits - 1)) & 1)) --top_bits;
  do {
    for (int i = 0; i < F::N; ++i) r.l[i] = next64();
    if (top_bits < 64) r.l[F::N - 1] &= ((uint64_t)1 << top_bits) - 1;
  } while (F::geq_mod(r.l));
  return r;
}

template <class F>
int check_pair(const F& a, const F& b, const char* what) {
  int bad = 0;
  if (F::mul(a, b) != F::mul_looped(a, b)) ++bad;
  if (F::mul(b, a) != F::mul_looped(b, a)) ++bad;
  if (F::sqr(a) != F::mul_looped(a, a)) ++bad;
  if (F::sqr(b) != F::mul_looped(b, b)) ++bad;
  if (bad) fprintf(stderr, "  mismatch (%s)\n", what);
  return bad;
}

template <class F>
double ns_per_op(F (*op)(const F&, const F&), const F& x0, const F& y, int iters, uint64_t* sink) {
  F x = x0;
  const auto t0 = std::chrono::steady_clock::now();
  for (int i = 0; i < iters; ++i) x = op(x, y);
  const auto t1 = std::chrono::steady_clock::now();
  *sink ^= x.l[0];
  return std::chrono::duration<double, std::nano>(t1 - t0).count() / iters;
}
template <class F>
F sqr_as_binary(const F& a, const F&) { return F::sqr(a); }
template <class F>
F sqr_looped_as_binary(const F& a, const F&) { return F::mul_looped(a, a); }

template <class F>
int run(const char* name, int pairs) {
  int bad = 0;
  F pm1;
  for (int i = 0; i < F::N; ++i) pm1.l[i] = F::K.mod[i];
  pm1.l[0] -= 1;  // every modulus is odd
  F plain_one = F::zero();
  plain_one.l[0] = 1;
  const F edges[4] = {F::zero(), plain_one, pm1, F::one()};  // the words 0, 1, p - 1 and R mod p
  for (const F& a : edges)
    for (const F& b : edges) bad += check_pair(a, b, "edge");
  for (const F& a : edges)
    if (F::inv(a) != F::inv_looped(a)) {
      ++bad;
      fprintf(stderr, "  inv mismatch (edge)\n");
    }
  F ones;  // an unreduced left operand
  for (int i = 0; i < F::N; ++i) ones.l[i] = ~(uint64_t)0;
  for (int k = 0; k < 1000; ++k) {
    const F b = random_elem<F>();
    if (F::mul(ones, b) != F::mul_looped(ones, b)) ++bad;
  }
  for (int k = 0; k < pairs; ++k) {
    const F a = random_elem<F>(), b = random_elem<F>();
    bad += check_pair(a, b, "random");
    if (k % 100 == 0) {  // 10^3 inversions: each one is ~400 products
      const F ia = F::inv(a);
      if (ia != F::inv_looped(a) || (!a.is_zero() && F::mul(ia, a) != F::one())) {
        ++bad;
        fprintf(stderr, "  inv mismatch (random)\n");
      }
    }
  }
  uint64_t sink = 0;
  const F x = random_elem<F>(), y = random_elem<F>();
  const int iters = 2000000;
  const double m_new = ns_per_op<F>(&F::mul, x, y, iters, &sink), m_old = ns_per_op<F>(&F::mul_looped, x, y, iters, &sink);
  const double s_new = ns_per_op<F>(&sqr_as_binary<F>, x, y, iters, &sink), s_old = ns_per_op<F>(&sqr_looped_as_binary<F>, x, y, iters, &sink);
  F z = x;
  const auto t0 = std::chrono::steady_clock::now();
  for (int i = 0; i < 200; ++i) z = F::inv(z);
  const auto t1 = std::chrono::steady_clock::now();
  for (int i = 0; i < 200; ++i) z = F::inv_looped(z);
  const auto t2 = std::chrono::steady_clock::now();
  sink ^= z.l[0];
  printf("%-12s %d limbs  %s  mul %.1f ns (looped %.1f)  sqr %.1f ns (looped %.1f)  inv %.2f us (looped %.2f)  [%llx]\n", name, F::N,
         bad ? "MISMATCH" : "ok", m_new, m_old, s_new, s_old, std::chrono::duration<double, std::micro>(t1 - t0).count() / 200,
         std::chrono::duration<double, std::micro>(t2 - t1).count() / 200, (unsigned long long)(sink & 0xfff));
  return bad;
}

}  // namespace

int main(int argc, char** argv) {
  const int pairs = argc > 1 ? atoi(argv[1]) : 100000;
  int bad = 0;
  bad += run<csh::Fp64<csh::Bn254FqParams>>("bn254 Fq", pairs);
  bad += run<csh::Fp64<csh::Bn254FrParams>>("bn254 Fr", pairs);
  bad += run<csh::Fp64<csh::Bls381FqParams>>("bls12-381 Fq", pairs);
  bad += run<csh::Fp64<csh::Bls377FqParams>>("bls12-377 Fq", pairs);
  if (bad) {
    fprintf(stderr, "host_field_check: %d mismatches\n", bad);
    return 1;
  }
  printf("host_field_check: ok\n");
  return 0;
}
