// What every C entry point of the host mirror (host/capi_*.cpp) does before and after its body, and what its bodies share: the error
// boundary and curve dispatch, the copy-out helpers, the seeded field RNG with the Rep3 / Shamir sharers on top of it, and the runner of
// in-process parties. Internal to those translation units; not installed.
#pragma once
#include <array>
#include <thread>

#include "groth16.hpp"
#include "arkwire.hpp"
#include "sharefile.hpp"
#include "plonk_honk.hpp"
#include "zkey.hpp"

namespace cosnarks {
namespace capi {

extern thread_local std::string g_err;  // what cog16_last_error() returns (defined in capi_formats.cpp)

// The error boundary of an extern "C" body: an exception becomes -1 and its message the thread's last error.
template <class Fn>
auto guarded(Fn fn) -> decltype(fn()) {
  try {
    return fn();
  } catch (const std::exception& e) {
    g_err = e.what();
    return -1;
  }
}

// The curve dispatch: fn(P{}) for the one P of Ps whose id is `curve`; the template arguments at the call site are the set of curves
// that the entry serves, any other id is "unknown curve".
template <class... Ps, class Fn>
int with_curve(int curve, Fn fn) {
  int rc = -1;
  if (!((curve == (int)Ps::ID ? (rc = fn(Ps{}), true) : false) || ...)) throw Error("unknown curve");
  return rc;
}
// ... and both in one, for the entries that look at the curve first
template <class... Ps, class Fn>
int entry(int curve, Fn fn) {
  return guarded([&] { return with_curve<Ps...>(curve, fn); });
}

template <class P>
typename P::Fr fr_from_canonical(const uint64_t v[4]) {
  typename P::Fr f;
  memcpy(&f, v, 32);
  return f.to_mont();
}

// `n` bytes to a caller's buffer of `cap` bytes; returns n
inline int copy_out(const void* bytes, size_t n, void* out, size_t cap) {
  if (n > cap) throw Error("output buffer too small");
  if (n) memcpy(out, bytes, n);
  return (int)n;
}
inline int copy_out(const std::vector<uint8_t>& bytes, void* out, size_t cap) { return copy_out(bytes.data(), bytes.size(), out, cap); }
// files back to back, sizes[i] = the length of file i; returns their number
inline int copy_out(const std::vector<std::vector<uint8_t>>& files, uint8_t* out, size_t cap, size_t* sizes) {
  size_t at = 0;
  for (size_t i = 0; i < files.size(); ++i) {
    at += sizes[i] = (size_t)copy_out(files[i], out + at, cap - at);
  }
  return (int)files.size();
}
// a string with its terminating NUL; returns 0
inline int write_out(const std::string& json, char* out, size_t cap) {
  copy_out(json.c_str(), json.size() + 1, out, cap);
  return 0;
}

// Field elements from a seeded generator, and the sharings drawn from it. seed 0 = OS entropy; a non-zero seed is for reproducible tests
// only. The ShareRng domain is the call site's: one generator per purpose.
template <class Fr>
struct FieldRng {
  using Rep3Share = Rep3PrimeFieldShare<Fr>;
  ShareRng gen;
  FieldRng(uint64_t seed, uint64_t domain) : gen(seed, domain) {}
  Fr rnd() {
    uint8_t b[32];
    for (int i = 0; i < 4; ++i) {
      uint64_t v = gen();
      memcpy(b + 8 * i, &v, 8);
    }
    return from_be_bytes_mod_order<Fr>(b);
  }
  // share_field_element(s) (mpc-core/src/protocols/rep3.rs:281-292, 375-389): two draws per element
  void rep3(const Fr& val, Rep3Share out3[3]) {
    Fr a = rnd(), b = rnd();
    Fr c = Fr::sub(Fr::sub(val, a), b);
    out3[0] = {a, c};
    out3[1] = {b, a};
    out3[2] = {c, b};
  }
  void rep3(const std::vector<Fr>& vals, std::vector<Rep3Share> out[3]) {  // appends
    for (auto& v : vals) {
      Rep3Share t[3];
      rep3(v, t);
      for (int p = 0; p < 3; ++p) out[p].push_back(t[p]);
    }
  }
  // shamir::share (shamir.rs:359-376): random degree-`deg` polynomial, shares = evaluations at 1..np
  std::vector<Fr> shamir(const Fr& secret, int deg, int np) {
    std::vector<Fr> coeffs{secret};
    for (int i = 0; i < deg; ++i) coeffs.push_back(rnd());
    std::vector<Fr> out(np);
    for (int p = 0; p < np; ++p) {
      Fr x = Fr::from_u64(p + 1), e = Fr::zero();
      for (size_t k = coeffs.size(); k-- > 0;) e = Fr::add(Fr::mul(e, x), coeffs[k]);
      out[p] = e;
    }
    return out;
  }
  std::vector<std::vector<Fr>> shamir(const std::vector<Fr>& vals, int deg, int np) {  // [party][element]
    std::vector<std::vector<Fr>> out(np, std::vector<Fr>(vals.size()));
    for (size_t i = 0; i < vals.size(); ++i) {
      const auto s = shamir(vals[i], deg, np);
      for (int p = 0; p < np; ++p) out[p][i] = s[p];
    }
    return out;
  }
  // the dealer that stands in for the DN07 preprocessing: one double sharing (degree t, degree 2t) of a random value, or of `fixed`
  // (the value is drawn either way), appended to every party's queue
  void double_sharing(int t, std::vector<std::deque<std::pair<Fr, Fr>>>& pairs, const Fr* fixed = nullptr) {
    Fr v = rnd();
    if (fixed) v = *fixed;
    const int np = (int)pairs.size();
    auto st = shamir(v, t, np), s2t = shamir(v, 2 * t, np);
    for (int p = 0; p < np; ++p) pairs[p].push_back({st[p], s2t[p]});
  }
};

// get_translation_points (mpc-core bridges/rep3_to_shamir.rs:14-28) of Rep3 party p: f(X) = 1 - X/z at its own point, for both of its shares
template <class Fr>
void rep3_to_shamir_points(int p, Fr& x, Fr& y) {
  const uint64_t e = p + 1, z1 = p == 0 ? 3 : p, z2 = p == 2 ? 1 : p + 2;
  x = Fr::sub(Fr::one(), Fr::mul(Fr::from_u64(e), Fr::inv(Fr::from_u64(z1))));
  y = Fr::sub(Fr::one(), Fr::mul(Fr::from_u64(e), Fr::inv(Fr::from_u64(z2))));
}

// the root cause first: parties that merely saw the abort of a failing peer report "network aborted"
inline void throw_first_party_error(const std::string* errs, int n) {
  for (int pass = 0; pass < 2; ++pass)
    for (int p = 0; p < n; ++p)
      if (!errs[p].empty() && (pass == 1 || errs[p].find("network aborted") == std::string::npos))
        throw Error("party " + std::to_string(p) + ": " + errs[p]);
}

// n in-process parties, one thread each, over NETS sets of LocalNetwork pairs: party p binds its thread to device_of(p) and runs
// fn(p, net...) with its end of every set. A party that fails aborts all sets, so that its peers unwind instead of waiting on it; the
// first root cause is thrown after all have joined.
template <size_t NETS, class DeviceOf, class Fn>
void run_parties(int n, DeviceOf device_of, Fn fn) {
  std::array<std::vector<LocalNetwork>, NETS> nets;
  for (auto& set : nets) set = LocalNetwork::new_parties(n);
  std::vector<std::string> errs(n);
  std::vector<std::thread> th;
  for (int p = 0; p < n; ++p) {
    th.emplace_back([&, p] {
      try {
        check(csh_init(device_of(p)), "csh_init");
        if constexpr (NETS == 1) fn(p, nets[0][p]);
        else fn(p, nets[0][p], nets[1][p]);
      } catch (const std::exception& e) {
        errs[p] = e.what();
        for (auto& set : nets) set[p].abort();
      }
    });
  }
  for (auto& t : th) t.join();
  throw_first_party_error(errs.data(), n);
}
inline auto on_device(int dev) {
  return [dev](int) { return dev; };
}

// Rep3State::new draws its seed from the OS rng (rep3.rs:56-76); here from ShareRng(seed, 100 + party), seed != 0: tests
inline Rep3State rep3_state(uint64_t seed, int p, const LocalNetwork& net) {
  uint8_t my_seed[32];
  ShareRng(seed, 100 + p).fill(my_seed, 32);
  return Rep3State::create(net, my_seed);
}

}  // namespace capi
}  // namespace cosnarks
