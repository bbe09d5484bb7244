// Multilinear folds out[j] = in[2j] + u (in[2j+1] - in[2j]) (mle_fold.hip): what the two kernels and the host
// self-test (selftest.hip, limb-bound checks on) share -- the challenge's scale, the index algebra of a tile, and the bound derivation.
//
// Scale. Elements are arkworks-Montgomery (R scale, field_scan.hpp). fr_to_rprime() (fr_entry.hpp) brings u to the R' domain once per call on the host;
// mul(b - a, ud) = (b - a) R u R' / R' is then R scale again, like a and b: no product multiplies two loaded operands, nothing is
// scaled by 32 on the device.
//
// Bounds over R lazy rounds (fold_step, vec_elem.hpp). Invariant of a value x that stays on chip: limbs 0..NL-2 in [0, 2^B), a small signed
// top limb, value within (-p - eps, 2 p + eps), eps < 1e-4 p -- what unpack() of a loaded element gives ([0, p)) and what fold_top() returns.
//   d = b - a: |limb| < 2^B (inside LIM1, so d may be mul's first operand, which allows LIM2), |d| < 3.1 p, inside mul's (-8 p, 8 p).
//   m = mul(d, ud), ud canonical: (d ud + q p) / R' with 0 <= q < R', so m lies in (-|d| p / R', p + |d| p / R') = (-0.05 p, 1.05 p)
//       (p / R' < 1 / 67 for the three scalar fields), limbs 0..NL-2 in [0, 2^B).
//   a + m: limbs below 2^(B+1) (no int32 overflow), value within (-1.1 p, 3.1 p).
//   fold_top(): full carry, then minus k p with |k| <= 4 (exact to +-1 up to 64): the invariant again.
// So the bound does not depend on the round: fold_top() sits at the END of every round, on the sum, because the sum is what grows (by up to
// 1.05 p per round without it: 28 rounds of u = p - 1 on a vector of p - 1 would leave mul's range after the 4th). normalized() is never
// needed on top of it: fold_top() already leaves every limb below 2^B. A level that is written out is that same value through
// canonical_narrow().pack() -- together canonical_wide().pack() of the sum -- and the chain goes on from the lazy value, which is the same
// residue: what is written never depends on how many rounds stayed on chip.
#pragma once
#include "common.hpp"
#include "field.hpp"
#include "field29.hpp"
#include "fr_entry.hpp"
#include "vec_elem.hpp"

namespace csh {

constexpr int FOLD_WG = 256;          // lanes of a k_mle_fold_rounds workgroup
constexpr int FOLD_MAX_ROUNDS = FOLD_TILE_LOG_MAX;
constexpr int FOLD_VECS_PER_LAUNCH = 64;  // vectors of one k_mle_fold launch (their pointers travel as kernel arguments)

// Flat indexing of a vector of n elements x ncomp interleaved components (ncomp 1 or 2). Output value o = j ncomp + c of a round reads
// the input values 2 o - c (element 2 j) and 2 o - c + ncomp (element 2 j + 1).
CSH_HD size_t fold_src(size_t o, uint32_t ncomp) { return 2 * o - (o & (size_t)(ncomp - 1)); }

// Levels 1..m of a chain on n elements lie back to back: level l starts at element n - n / 2^(l-1) (= sum of n / 2^i, i < l)
CSH_HD size_t fold_level_offset(size_t n, int l) { return n - (n >> (l - 1)); }

// On chip (LDS on the device) a level of cnt elements is kept component-major, value (j, c) at c cnt + j, one plane per limb: the pair of
// the next round is then two adjacent words of a plane for either ncomp. FoldPlanes is that storage behind one interface for the kernel
// (planes in LDS) and the self-test (planes in a vector).
template <class LZ>
struct FoldPlanes {
  int32_t* w;     // NL planes of `stride` words
  size_t stride;  // even: a pair is 8-byte aligned
  CSH_HD void put(size_t i, const LZ& v) const {
#pragma unroll
    for (int k = 0; k < LZ::NL; ++k) w[k * stride + i] = v.l[k];
  }
  // the values at i and i + 1, i even
  CSH_HD void pair(size_t i, LZ& a, LZ& b) const {
#pragma unroll
    for (int k = 0; k < LZ::NL; ++k) {
      const int32_t* q = w + k * stride + i;
#if defined(__HIP_DEVICE_COMPILE__)
      const int2 t = *reinterpret_cast<const int2*>(q);  // one 8-byte LDS read: consecutive lanes, consecutive banks
      a.l[k] = t.x;
      b.l[k] = t.y;
#else
      a.l[k] = q[0];
      b.l[k] = q[1];
#endif
    }
  }
};
// words of on-chip storage for a tile of 2^tile_log elements: level 1 (ncomp 2^(tile_log-1) values) and level 2 (half of that) ping-pong
CSH_HD size_t fold_plane_a(int tile_log, uint32_t ncomp) { return ((size_t)ncomp << (tile_log - 1)); }
CSH_HD size_t fold_plane_b(int tile_log, uint32_t ncomp) {
  const size_t b = fold_plane_a(tile_log, ncomp) >> 1;
  return b < 2 ? 2 : b;
}

// What one launch of k_mle_fold_rounds is told. It folds level 0 = `in` (n_in elements) R times; local level r has n_in >> r elements.
template <class F>
struct FoldRoundsArgs {
  F ud[FOLD_MAX_ROUNDS];  // the launch's challenges, R' domain
  const F* in;
  F* levels;              // local levels 1..R back to back (fold_level_offset(n_in, r)), or NULL
  F* last;                // local level R alone, or NULL
  size_t n_in;
  uint32_t ncomp;
  int rounds, tile_log;
};

// One tile of one launch, as lane `lane` of `lanes` sees round r (1-based): the outputs o = lane, lane + lanes, ... below cnt ncomp, cnt = the
// tile's elements at level r. Round 1 reads `in`, later rounds read the planes the round before filled; a kept level is written canonically,
// the value goes on lazily unless the round is the launch's last. The kernel calls this with a barrier between rounds; the self-test calls it for
// every lane in turn.
template <class F>
CSH_HD void fold_tile_round(const FoldRoundsArgs<F>& a, size_t tile, int r, size_t lane, size_t lanes, int32_t* planes) {
  using LZ = typename LazyOf<F>::type;
  const size_t first = tile << a.tile_log;  // the tile's first element at level 0
  const size_t cnt0 = a.n_in - first < ((size_t)1 << a.tile_log) ? a.n_in - first : (size_t)1 << a.tile_log;
  const size_t cnt = cnt0 >> r, cnt_prev = cnt0 >> (r - 1), nc = a.ncomp;
  const size_t sa = fold_plane_a(a.tile_log, a.ncomp), sb = fold_plane_b(a.tile_log, a.ncomp);
  const FoldPlanes<LZ> pa{planes, sa}, pb{planes + LZ::NL * sa, sb};
  const FoldPlanes<LZ>& src = (r & 1) ? pb : pa;  // round 1 fills A, round 2 reads A and fills B, ...
  const FoldPlanes<LZ>& dst = (r & 1) ? pa : pb;
  const LZ ud = LZ::unpack(a.ud[r - 1]);
  F* lvl = a.levels ? a.levels + (fold_level_offset(a.n_in, r) + (first >> r)) * nc : nullptr;
  F* lst = (a.last && r == a.rounds) ? a.last + (first >> r) * nc : nullptr;
#pragma unroll 1
  for (size_t o = lane; o < cnt * nc; o += lanes) {
    LZ x, y;
    size_t j, c;
    if (r == 1) {  // o = j ncomp + c: adjacent lanes read adjacent elements
      const size_t s = fold_src(o, a.ncomp);
      const F* p = a.in + first * nc;
      x = LZ::unpack(p[s]);
      y = LZ::unpack(p[s + nc]);
      j = nc == 1 ? o : o >> 1;
      c = o & (nc - 1);
    } else {  // o = c cnt + j: adjacent lanes read adjacent pairs of a plane
      c = o >= cnt ? 1 : 0;
      j = o - c * cnt;
      src.pair(c * cnt_prev + 2 * j, x, y);
    }
    const LZ v = fold_step(x, y, ud);
    if (r < a.rounds) dst.put(c * cnt + j, v);
    if (lvl || lst) {
      const F f = v.canonical_narrow().pack();
      if (lvl) lvl[j * nc + c] = f;
      if (lst) lst[j * nc + c] = f;
    }
  }
}

}  // namespace csh
