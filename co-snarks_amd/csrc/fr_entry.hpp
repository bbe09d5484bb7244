// The host-side layer every scalar-field entry point shares (vec_ops, field_scan, mle_fold, plonk_quot, sparse, groth16_h, ntt and the host
// self-tests of selftest.hip): the one way from a run-time curve to its scalar-field type, the argument rules, and the small conversions a
// launcher makes before it launches. Nothing here runs on the device. DESIGN.md section 3.3.
#pragma once
#include <string.h>

#include <vector>

#include "common.hpp"
#include "field.hpp"
#include "field29.hpp"

namespace csh {

// ---- curve -> F ---------------------------------------------------------------------------------------------------------------------------
// The scalar field of a curve, handed to a generic callable as a tag:
//   with_fr(curve, [&](auto fr) -> int { using F = typename decltype(fr)::type; ... })
// Grumpkin has no scalar-field entry points: it and any other value are refused.
template <class F>
struct FrTag {
  using type = F;
};
template <class Fn>
inline int with_fr(csh_curve_t curve, Fn&& f) {
  switch (curve) {
    case CSH_BN254: return f(FrTag<Bn254Fr>{});
    case CSH_BLS12_381: return f(FrTag<Bls381Fr>{});
    case CSH_BLS12_377: return f(FrTag<Bls377Fr>{});
    default: set_error("unknown curve %d", (int)curve); return CSH_ERR_INVALID;
  }
}
// with_fr() around one expression in F, the common case: return FR_CALL(field_of, vec_mul_t<F>(a, b, out, n, st));
#define FR_CALL(curve, ...) \
  csh::with_fr((csh_curve_t)(curve), [&](auto fr__) -> int { using F = typename decltype(fr__)::type; return __VA_ARGS__; })

// ---- argument rules -------------------------------------------------------------------------------------------------------------------------
constexpr size_t FR_MAX_N = size_t(1) << 28;  // the largest domain: BN254 Fr has two-adicity 28
inline bool fr_known(csh_curve_t f) { return f == CSH_BN254 || f == CSH_BLS12_381 || f == CSH_BLS12_377; }
#define FR_REQUIRE_FIELD(f) CSH_REQUIRE(csh::fr_known(f), "field_of: BN254, BLS12-381 or BLS12-377")
#define FR_REQUIRE_N(n) CSH_REQUIRE((n) <= csh::FR_MAX_N, "n exceeds 2^28, the largest domain")
#define FR_REQUIRE_NCOMP(ncomp) CSH_REQUIRE((ncomp) == 1 || (ncomp) == 2, "ncomp must be 1 or 2")

// p[0 .. k) are all there (and so is p, unless k = 0)
inline int fr_require_ptrs(const void* const* p, size_t k, const char* what) {
  bool ok = p || !k;
  for (size_t v = 0; ok && v < k; ++v) ok = p[v] != nullptr;
  if (!ok) set_error("%s: NULL argument", what);
  return ok ? CSH_OK : CSH_ERR_INVALID;
}

// Byte ranges of a call's vectors. No output may overlap an input, and (outputs_too) no output another output: a kernel that reads
// element j' for output j (a fold, a rotation, a chunked column) run in place is a race between workgroups.
struct FrRanges {
  struct Range {
    uintptr_t lo, hi;
  };
  std::vector<Range> r;
  void add(const void* p, size_t bytes) { r.push_back(Range{(uintptr_t)p, (uintptr_t)p + bytes}); }
  void add(const void* const* p, size_t k, size_t bytes) {
    r.reserve(r.size() + k);
    for (size_t v = 0; v < k; ++v) add(p[v], bytes);
  }
};
inline int fr_check_ranges(const FrRanges& in, const FrRanges& out, const char* what, bool outputs_too = true) {
  auto overlap = [](const FrRanges::Range& a, const FrRanges::Range& b) { return a.lo < b.hi && b.lo < a.hi; };
  for (size_t o = 0; o < out.r.size(); ++o) {
    for (const FrRanges::Range& i : in.r)
      if (overlap(out.r[o], i)) {
        set_error("%s: an output overlaps an input", what);
        return CSH_ERR_INVALID;
      }
    for (size_t q = 0; outputs_too && q < o; ++q)
      if (overlap(out.r[o], out.r[q])) {
        set_error("%s: two outputs overlap", what);
        return CSH_ERR_INVALID;
      }
  }
  return CSH_OK;
}

// ---- what a launcher does to its arguments ------------------------------------------------------------------------------------------------
// 32 bytes of the caller's (arkworks Montgomery words, any alignment) -> F
template <class F>
inline F fr_load(const void* p) {
  F f;
  memcpy(&f, p, sizeof(F));
  return f;
}
// c (arkworks Montgomery) -> c R' mod p, canonical and packed: the form in which a constant of a call is an operand of the lazy product
// (the storage form of the lazy field, for the F that the entry point was dispatched to)
template <class F>
inline F fr_to_rprime(const F& c) {
  return LzOf<F>::repack_for_storage(c);
}
// workgroups of a streaming kernel over `values` flat indices with `wg` lanes each (tune "vec_max_blocks"; 65536: up to one element per
// lane at 2^24, measured 8-10 % faster than 4096 blocks + grid stride)
inline int fr_stream_grid(size_t values, int wg) {
  int mb = tune().vec_max_blocks.load(std::memory_order_relaxed);
  if (mb <= 0) mb = 65536;
  return grid_for(values, wg, mb);
}

}  // namespace csh
