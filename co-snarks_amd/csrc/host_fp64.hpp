// Host-only Montgomery field on 64-bit limbs (unsigned __int128 CIOS) for the sequential tail of an MSM: the Horner
// fold of the W window sums (W*c doublings) and the final inversion. Same modulus, same R = 2^(32*N) = 2^(64*N/2) and
// the same little-endian bytes as Fp<P> (field.hpp), so device results are reinterpreted in place; a 64-bit limb product
// replaces four 32-bit ones on the CPU (the fold drops from ~270 us to ~60 us, 10% of a 2^20 MSM).
//
// The fold is one dependent chain of ~2000 field products, so the product itself is written for latency: modulus words and
// -p^-1 are compile-time constants, the limb loops have constant trip counts (4 or 6) and are unrolled, the product is the
// "no-carry" CIOS (no t[N], t[N + 1] words: every modulus here leaves its top bit free), and the square has its own routine
// (N (N + 1) / 2 limb products instead of N^2 before the reduction). mul_looped / inv_looped are the plain forms the fast
// ones are checked against (tools/host_field_check.cpp); every routine returns the same canonical words as they do.
#pragma once
#include <stdint.h>
#include <string.h>

#include "field.hpp"

#if defined(__clang__)
#define CSH_HOST_UNROLL _Pragma("unroll")
#elif defined(__GNUC__)
#define CSH_HOST_UNROLL _Pragma("GCC unroll 16")
#else
#define CSH_HOST_UNROLL
#endif

namespace csh {

template <int N>
struct Fp64Consts {
  uint64_t mod[N], one[N], pm2[N];
  uint64_t inv;  // -p^-1 mod 2^64
};
template <class P>
constexpr Fp64Consts<P::N / 2> fp64_consts() {
  Fp64Consts<P::N / 2> k{};
  for (int i = 0; i < P::N / 2; ++i) {
    k.mod[i] = (uint64_t)P::MOD[2 * i] | ((uint64_t)P::MOD[2 * i + 1] << 32);
    k.one[i] = (uint64_t)P::R1[2 * i] | ((uint64_t)P::R1[2 * i + 1] << 32);
    k.pm2[i] = (uint64_t)P::PM2[2 * i] | ((uint64_t)P::PM2[2 * i + 1] << 32);
  }
  uint64_t y = k.mod[0];  // Newton iteration on the low modulus word: p0 * p0 = 1 mod 8, the valid bits double per step
  for (int i = 0; i < 6; ++i) y *= 2 - k.mod[0] * y;
  k.inv = (uint64_t)0 - y;
  return k;
}

template <class P>
struct Fp64 {
  static_assert(P::N % 2 == 0, "limb count must be even");
  static constexpr int N = P::N / 2;
  using Params = P;
  using u128 = unsigned __int128;
  uint64_t l[N];

  static constexpr Fp64Consts<N> K = fp64_consts<P>();
  // what the no-carry product and the carry-less add rely on: 2 p < 2^(64 N), and the top word is not all ones below that bit
  static_assert((K.mod[N - 1] >> 63) == 0 && K.mod[N - 1] != 0x7fffffffffffffffull, "the modulus must leave its top bit free");
  static_assert((uint64_t)(K.mod[0] * K.inv) == ~(uint64_t)0, "inv must be -p^-1 mod 2^64");

  static uint64_t word(const uint32_t* w, int i) { return (uint64_t)w[2 * i] | ((uint64_t)w[2 * i + 1] << 32); }
  static constexpr uint64_t inv64() { return K.inv; }
  static Fp64 zero() {
    Fp64 r;
    for (int i = 0; i < N; ++i) r.l[i] = 0;
    return r;
  }
  static Fp64 one() {
    Fp64 r;
    for (int i = 0; i < N; ++i) r.l[i] = K.one[i];
    return r;
  }
  bool is_zero() const {
    uint64_t a = 0;
    for (int i = 0; i < N; ++i) a |= l[i];
    return a == 0;
  }
  bool operator==(const Fp64& b) const { return memcmp(l, b.l, sizeof l) == 0; }
  bool operator!=(const Fp64& b) const { return !(*this == b); }

  static bool geq_mod(const uint64_t* a) {
    CSH_HOST_UNROLL
    for (int i = N - 1; i >= 0; --i) {
      if (a[i] > K.mod[i]) return true;
      if (a[i] < K.mod[i]) return false;
    }
    return true;
  }
  static void sub_mod(uint64_t* a) {
    u128 br = 0;
    CSH_HOST_UNROLL
    for (int i = 0; i < N; ++i) {
      const u128 d = (u128)a[i] - K.mod[i] - (uint64_t)br;
      a[i] = (uint64_t)d;
      br = (d >> 64) & 1;
    }
  }
  static Fp64 add(const Fp64& a, const Fp64& b) {  // the spare top bit: no carry out
    Fp64 r;
    u128 c = 0;
    CSH_HOST_UNROLL
    for (int i = 0; i < N; ++i) {
      c += (u128)a.l[i] + b.l[i];
      r.l[i] = (uint64_t)c;
      c >>= 64;
    }
    if (geq_mod(r.l)) sub_mod(r.l);
    return r;
  }
  static Fp64 sub(const Fp64& a, const Fp64& b) {
    Fp64 r;
    uint64_t br = 0;
    CSH_HOST_UNROLL
    for (int i = 0; i < N; ++i) {
      const u128 d = (u128)a.l[i] - b.l[i] - br;
      r.l[i] = (uint64_t)d;
      br = (uint64_t)(d >> 64) & 1;
    }
    if (br) {
      u128 c = 0;
      CSH_HOST_UNROLL
      for (int i = 0; i < N; ++i) {
        c += (u128)r.l[i] + K.mod[i];
        r.l[i] = (uint64_t)c;
        c >>= 64;
      }
    }
    return r;
  }
  static Fp64 neg(const Fp64& a) { return a.is_zero() ? a : sub(zero(), a); }

  // a b / R mod p, canonical. No-carry CIOS: word i of `a` times all of `b`, one reduction step, both in one pass over t. With
  // b < p the running value stays below b + p < 2^(64 N), so the two carry chains of a pass add up without a carry out and t has
  // N words. `a` may be any N-word value (from-bytes reduction multiplies an unreduced draw by R^2); b must be reduced.
  static Fp64 mul(const Fp64& a, const Fp64& b) {
    uint64_t t[N];
    CSH_HOST_UNROLL
    for (int j = 0; j < N; ++j) t[j] = 0;
    CSH_HOST_UNROLL
    for (int i = 0; i < N; ++i) {
      u128 A = (u128)a.l[i] * b.l[0] + t[0];
      const uint64_t m = (uint64_t)A * K.inv;
      u128 C = (u128)m * K.mod[0] + (uint64_t)A;
      CSH_HOST_UNROLL
      for (int j = 1; j < N; ++j) {
        A = (u128)a.l[i] * b.l[j] + t[j] + (uint64_t)(A >> 64);
        C = (u128)m * K.mod[j] + (uint64_t)A + (uint64_t)(C >> 64);
        t[j - 1] = (uint64_t)C;
      }
      t[N - 1] = (uint64_t)(A >> 64) + (uint64_t)(C >> 64);
    }
    Fp64 r;
    CSH_HOST_UNROLL
    for (int i = 0; i < N; ++i) r.l[i] = t[i];
    if (geq_mod(r.l)) sub_mod(r.l);
    return r;
  }
  // a^2 / R mod p, canonical, for a < p: the 2 N-word square from N (N - 1) / 2 cross products (doubled) and N diagonal ones,
  // then N reduction steps. a^2 < p^2 keeps the reduced value below 2 p.
  static Fp64 sqr(const Fp64& a) {
    uint64_t t[2 * N];
    CSH_HOST_UNROLL
    for (int j = 0; j < 2 * N; ++j) t[j] = 0;
    CSH_HOST_UNROLL
    for (int i = 0; i < N - 1; ++i) {  // sum_{i < j} a_i a_j 2^(64 (i + j))
      uint64_t c = 0;
      CSH_HOST_UNROLL
      for (int j = i + 1; j < N; ++j) {
        const u128 v = (u128)a.l[i] * a.l[j] + t[i + j] + c;
        t[i + j] = (uint64_t)v;
        c = (uint64_t)(v >> 64);
      }
      t[i + N] = c;
    }
    CSH_HOST_UNROLL
    for (int j = 2 * N - 1; j > 0; --j) t[j] = (t[j] << 1) | (t[j - 1] >> 63);  // doubled: the sum is below 2^(128 N - 1)
    t[0] = 0;
    {
      uint64_t c = 0;
      CSH_HOST_UNROLL
      for (int i = 0; i < N; ++i) {  // + sum_i a_i^2 2^(128 i)
        const u128 d = (u128)a.l[i] * a.l[i];
        const u128 lo = (u128)t[2 * i] + (uint64_t)d + c;
        t[2 * i] = (uint64_t)lo;
        const u128 hi = (u128)t[2 * i + 1] + (uint64_t)(d >> 64) + (uint64_t)(lo >> 64);
        t[2 * i + 1] = (uint64_t)hi;
        c = (uint64_t)(hi >> 64);
      }
    }
    uint64_t top = 0;  // carries out of the words the reduction steps have finished with, into word i + N
    CSH_HOST_UNROLL
    for (int i = 0; i < N; ++i) {
      const uint64_t m = t[i] * K.inv;
      u128 C = (u128)m * K.mod[0] + t[i];
      CSH_HOST_UNROLL
      for (int j = 1; j < N; ++j) {
        C = (u128)m * K.mod[j] + t[i + j] + (uint64_t)(C >> 64);
        t[i + j] = (uint64_t)C;
      }
      const u128 s = (u128)t[i + N] + (uint64_t)(C >> 64) + top;
      t[i + N] = (uint64_t)s;
      top = (uint64_t)(s >> 64);
    }
    Fp64 r;  // (a^2 + sum m_i p 2^(64 i)) / 2^(64 N) < 2 p: `top` ends as zero
    CSH_HOST_UNROLL
    for (int i = 0; i < N; ++i) r.l[i] = t[i + N];
    if (geq_mod(r.l)) sub_mod(r.l);
    return r;
  }
  static Fp64 mul2(const Fp64& a) { return add(a, a); }
  static Fp64 mul3(const Fp64& a) { return add(add(a, a), a); }
  static Fp64 mul4(const Fp64& a) { return mul2(mul2(a)); }
  static Fp64 mul8(const Fp64& a) { return mul2(mul4(a)); }
  // a^(p-2), exponent read in 4-bit windows from the top: 14 products for a^2 .. a^15, then four squares and at most one
  // product per window -- 64 N squares and <= 16 N + 14 products where bit-by-bit square-and-multiply has ~32 N products.
  static Fp64 inv(const Fp64& a) {
    Fp64 pw[16];
    pw[0] = one();
    pw[1] = a;
    for (int i = 2; i < 16; ++i) pw[i] = (i & 1) ? mul(pw[i - 1], a) : sqr(pw[i / 2]);
    Fp64 r = one();
    bool started = false;
    for (int i = 16 * N - 1; i >= 0; --i) {
      const unsigned d = (unsigned)(K.pm2[i >> 4] >> (4 * (i & 15))) & 15u;
      if (started) r = sqr(sqr(sqr(sqr(r))));
      if (d) {
        r = started ? mul(r, pw[d]) : pw[d];
        started = true;
      }
    }
    return r;
  }

  // ---- the plain forms, kept as the check of the ones above -------------------------------------------------------------
  static Fp64 mul_looped(const Fp64& a, const Fp64& b) {  // CIOS with the two extra carry words
    uint64_t t[N + 2];
    for (int i = 0; i < N + 2; ++i) t[i] = 0;
    const uint64_t inv = K.inv;
    for (int i = 0; i < N; ++i) {
      u128 c = 0;
      for (int j = 0; j < N; ++j) {
        c += (u128)a.l[j] * b.l[i] + t[j];
        t[j] = (uint64_t)c;
        c >>= 64;
      }
      c += t[N];
      t[N] = (uint64_t)c;
      t[N + 1] = (uint64_t)(c >> 64);
      const uint64_t m = t[0] * inv;
      c = (u128)m * K.mod[0] + t[0];
      c >>= 64;
      for (int j = 1; j < N; ++j) {
        c += (u128)m * K.mod[j] + t[j];
        t[j - 1] = (uint64_t)c;
        c >>= 64;
      }
      c += t[N];
      t[N - 1] = (uint64_t)c;
      t[N] = t[N + 1] + (uint64_t)(c >> 64);
    }
    Fp64 r;
    for (int i = 0; i < N; ++i) r.l[i] = t[i];
    if (t[N] || geq_mod(r.l)) sub_mod(r.l);
    return r;
  }
  static Fp64 inv_looped(const Fp64& a) {  // a^(p-2), one bit at a time
    Fp64 r = one();
    for (int i = P::N * 32 - 1; i >= 0; --i) {
      r = mul_looped(r, r);
      if ((P::PM2[i >> 5] >> (i & 31)) & 1) r = mul_looped(r, a);
    }
    return r;
  }
};

// Fp<P> -> Fp64<P>, Fp2T<Fp<P>> -> Fp2T<Fp64<P>> (identical bytes)
template <class F>
struct Host64;
template <class P>
struct Host64<Fp<P>> {
  using type = Fp64<P>;
};
template <class P, int NR>
struct Host64<Fp2T<Fp<P>, NR>> {
  using type = Fp2T<Fp64<P>, NR>;
};

}  // namespace csh
