// Whole-vector field arithmetic that is a scan or a reduction: running product, batch inverse, polynomial evaluation, division by (X - r).
// Reference call sites: array_prod_mul (co-plonk/src/round2.rs:164-165), inv_vec / inv_many (co-noir-common/src/mpc/rep3.rs:208-257),
// evaluate_poly_public (co-plonk/src/round4.rs:126-132), eval_poly (rep3/poly.rs:39-68), factor_roots / div_by_zerofier (further down).
//
// One decomposition for all four: a lane takes a contiguous run of E elements (tune "scan_lane_run"), a tile is one workgroup of
// "scan_tile_lanes" lanes, and every operation is  per-tile totals -> a spine run by ONE workgroup that walks the totals "scan_spine_step"
// at a time with a running carry (any tile count, no recursion) -> a per-tile downsweep (the evaluation has none: its spine's carry is the
// result). Products run in the signed lazy field; field_scan.hpp says which scale every value has.
#include "field_scan.hpp"
#include "fr_entry.hpp"

#include <string.h>

#include <type_traits>

namespace csh {

constexpr int SCAN_TILE_MAX = 256;     // lanes of a tile kernel: 4 waves, so that the downsweep's register arrays need no occupancy
constexpr int SCAN_SPINE_MAX = 1024;   // lanes of the spine

struct ScanPlan {
  int E, lg_e, lanes, lg_lanes, spine, lg_spine;
  size_t tile, tiles;
};
static int ilog2(size_t v) {
  int l = 0;
  while ((size_t(1) << (l + 1)) <= v) ++l;
  return l;
}
static ScanPlan scan_plan(size_t n) {
  ScanPlan p;
  p.E = tune().scan_lane_run.load(std::memory_order_relaxed);
  p.lanes = tune().scan_tile_lanes.load(std::memory_order_relaxed);
  p.spine = tune().scan_spine_step.load(std::memory_order_relaxed);
  // csh_tune_set refuses other values; the environment is not validated, so anything else means the default here
  if (!scan_knob_ok(&Tune::scan_lane_run, p.E)) p.E = 8;
  if (!scan_knob_ok(&Tune::scan_tile_lanes, p.lanes)) p.lanes = 256;
  if (!scan_knob_ok(&Tune::scan_spine_step, p.spine)) p.spine = 1024;
  p.lg_e = ilog2(p.E);
  p.lg_lanes = ilog2(p.lanes);
  p.lg_spine = ilog2(p.spine);
  p.tile = (size_t)p.E * p.lanes;
  p.tiles = (n + p.tile - 1) / p.tile;
  return p;
}

// ---- products ---------------------------------------------------------------------------------------------------------------------------
// Launch 1: tot[tile] = product of the tile's elements, R' domain. INV: zeros count as 1 and are counted (one atomic per tile that has any).
template <class F, bool INV>
__global__ __launch_bounds__(SCAN_TILE_MAX) void k_scan_totals(const F* in, size_t n, int E, LzOf<F>* tot, unsigned long long* zero_count) {
  using LZ = LzOf<F>;
  __shared__ LZ lds[16];
  __shared__ unsigned zc;
  const size_t base = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * (size_t)E;
  unsigned zeros = 0;
  auto load = [&](size_t i) {
    F x = F::one();
    if (i < n) {
      x = in[i];
      if (INV && x.is_zero()) {
        x = F::one();
        ++zeros;
      }
    }
    return LZ::unpack(x);
  };
  LZ acc = load(base);
#pragma unroll 1
  for (int e = 1; e < E; ++e) acc = LZ::mul(acc, load(base + e).times32());
  const LZ total = block_reduce(to_domain(acc), lds, MulOp<LZ>());
  if (threadIdx.x == 0) tot[blockIdx.x] = total;
  if (INV) {
    if (threadIdx.x == 0) zc = 0;
    __syncthreads();
    if (zeros) atomicAdd(&zc, zeros);
    __syncthreads();
    if (threadIdx.x == 0 && zc && zero_count) atomicAdd(zero_count, (unsigned long long)zc);
  }
}

// Launch 2: pre[t] = product of tot[0 .. t) (R' domain). INV: also suf[t] = T^-1 x product of tot(t .. tiles), R scale, with T the
// product of everything: the one inversion of the batch, a dependent chain on lane 0.
template <class F, bool INV>
__global__ __launch_bounds__(SCAN_SPINE_MAX) void k_scan_spine(const LzOf<F>* tot, size_t tiles, LzOf<F>* pre, LzOf<F>* suf) {
  using LZ = LzOf<F>;
  __shared__ ScanLds<LZ> s;
  const size_t S = blockDim.x;
  LZ carry = LZ::one(), total;
  for (size_t c0 = 0; c0 < tiles; c0 += S) {
    const size_t i = c0 + threadIdx.x;
    const LZ p = block_excl_scan_mul<false>(i < tiles ? tot[i] : LZ::one(), carry, s, &total);
    if (i < tiles) pre[i] = p;
    carry = total;
  }
  if constexpr (INV) {
    __shared__ InvScratch<LZ> inv;
    __shared__ LZ tinv;
    if (threadIdx.x == 0) tinv = from_domain(lazy_inv(carry, inv));
    __syncthreads();
    carry = tinv;
    for (size_t c = (tiles + S - 1) / S; c-- > 0;) {
      const size_t i = c * S + threadIdx.x;
      const LZ p = block_excl_scan_mul<true>(i < tiles ? tot[i] : LZ::one(), carry, s, &total);
      if (i < tiles) suf[i] = p;
      carry = total;
    }
  }
}

// A loop over the lane's run with the index a compile-time constant: the bodies below hold whole multiplications, and a #pragma unroll
// loop of that size silently stays a loop -- the run's register arrays would then be indexed at run time and go to scratch.
template <int I, int N, class Fn>
__device__ __forceinline__ void run_for(Fn&& body) {
  if constexpr (I < N) {
    body(std::integral_constant<int, I>());
    run_for<I + 1, N>(body);
  }
}

// the lane's run: elements into registers (1 past the end; INV: 1 for a zero, its bit set in *zmask), lane total in the R' domain
template <class F, int E, bool INV>
__device__ __forceinline__ LzOf<F> load_run(const F* in, size_t n, size_t base, F (&x)[E], uint32_t* zmask) {
  using LZ = LzOf<F>;
  run_for<0, E>([&](auto ic) CSH_LAMBDA_INLINE {
    constexpr int e = decltype(ic)::value;
    x[e] = F::one();
    if (base + e < n) {
      x[e] = in[base + e];
      if (INV && x[e].is_zero()) {
        x[e] = F::one();
        *zmask |= 1u << e;
      }
    }
  });
  LZ acc = LZ::unpack(x[0]);
  run_for<1, E>([&](auto ic) CSH_LAMBDA_INLINE { acc = LZ::mul(acc, LZ::unpack(x[decltype(ic)::value]).times32()); });
  return to_domain(acc);
}

// Launch 3, running product: out[i] = in[0] ... in[i]. A lane reads its whole run before it writes any of it, and no lane touches
// another's: out may equal in.
template <class F, int E>
__global__ __launch_bounds__(SCAN_TILE_MAX) void k_prefix_down(const F* in, F* out, size_t n, const LzOf<F>* pre) {
  using LZ = LzOf<F>;
  __shared__ ScanLds<LZ> s;
  const size_t base = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * (size_t)E;
  F x[E];
  const LZ lane_total = load_run<F, E, false>(in, n, base, x, nullptr);
  LZ total;
  const LZ before = block_excl_scan_mul<false>(lane_total, pre[blockIdx.x], s, &total);
  LZ acc = LZ::mul(LZ::unpack(x[0]), before);  // R scale x R' domain: R scale
  run_for<0, E>([&](auto ic) CSH_LAMBDA_INLINE {
    constexpr int e = decltype(ic)::value;
    if (e) acc = LZ::mul(acc, LZ::unpack(x[e]).times32());
    if (base + e < n) out[base + e] = acc.canonical_wide().pack();
  });
}

// Launch 3, batch inverse: out[i] = T^-1 x (everything before i) x (everything after i); zeros stay zero.
template <class F, int E>
__global__ __launch_bounds__(SCAN_TILE_MAX) void k_inverse_down(const F* in, F* out, size_t n, const LzOf<F>* pre, const LzOf<F>* suf) {
  using LZ = LzOf<F>;
  __shared__ ScanLds<LZ> s;
  const size_t base = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * (size_t)E;
  F x[E];
  uint32_t zmask = 0;
  const LZ lane_total = load_run<F, E, true>(in, n, base, x, &zmask);
  LZ total;
  LZ f[E];  // f[e] = everything before element e, R' domain
  f[0] = block_excl_scan_mul<false>(lane_total, pre[blockIdx.x], s, &total);
  LZ after = block_excl_scan_mul<true>(lane_total, suf[blockIdx.x], s, &total);  // T^-1 x everything after the lane's run, R scale
  run_for<1, E>([&](auto ic) CSH_LAMBDA_INLINE {
    constexpr int e = decltype(ic)::value;
    f[e] = LZ::mul(f[e - 1], LZ::unpack(x[e - 1]).times32());
  });
  run_for<0, E>([&](auto ic) CSH_LAMBDA_INLINE {
    constexpr int e = E - 1 - decltype(ic)::value;
    const F r = LZ::mul(f[e], after).canonical_wide().pack();
    if (base + e < n) out[base + e] = ((zmask >> e) & 1u) ? F::zero() : r;
    if (e) after = LZ::mul(after, LZ::unpack(x[e]).times32());
  });
}

// ---- polynomial evaluation --------------------------------------------------------------------------------------------------------------
// pw (field_scan.hpp): pw.p[j] = x^(2^j), R' domain, canonical and packed.
// lo + x^(len 2^k) hi with len = 2^base positions per lane. Values are R scale; one carry step per level keeps the limbs inside the
// product's operand bound, fold_top() after the lane and the wave levels keeps the value below 8 p.
template <class F>
struct EvalOp {
  using LZ = LzOf<F>;
  const PowTable<F>* pw;
  int base;
  __device__ __forceinline__ LZ operator()(const LZ& lo, const LZ& hi, int k) const {
    return LZ::add(lo, LZ::mul(hi, LZ::unpack(pw->p[base + k]))).normalized();
  }
  __device__ __forceinline__ LZ settle(const LZ& v) const { return v.fold_top(); }
  __device__ __forceinline__ LZ identity() const { return LZ::zero(); }
};

// Launch 1: tot[comp][tile] = sum over the tile of coeffs[i][comp] x^(i - tile start); blockIdx.y = component
template <class F>
__global__ __launch_bounds__(SCAN_TILE_MAX) void k_eval_totals(const F* __restrict__ coeffs, size_t n, uint32_t ncomp, int E, int lg_e,
                                                                PowTable<F> pw, LzOf<F>* tot) {
  using LZ = LzOf<F>;
  __shared__ LZ lds[16];
  const size_t base = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * (size_t)E;
  const uint32_t comp = blockIdx.y;
  const LZ x = LZ::unpack(pw.p[0]);
  LZ v = LZ::zero();
#pragma unroll 1
  for (int e = E - 1; e >= 0; --e) {  // Horner over the lane's run
    const size_t i = base + e;
    const LZ c = i < n ? LZ::unpack(coeffs[i * ncomp + comp]) : LZ::zero();
    v = LZ::add(LZ::mul(v, x), c).normalized();
  }
  const LZ total = block_reduce(v, lds, EvalOp<F>{&pw, lg_e});
  if (threadIdx.x == 0) tot[(size_t)comp * gridDim.x + blockIdx.x] = total;
}
// Launch 2: Horner over the steps of the spine, highest first; blockIdx.x = component
template <class F>
__global__ __launch_bounds__(SCAN_SPINE_MAX) void k_eval_spine(const LzOf<F>* tot, size_t tiles, int lg_tile, int lg_spine, PowTable<F> pw, F* out) {
  using LZ = LzOf<F>;
  __shared__ LZ lds[16];
  const LZ* t = tot + (size_t)blockIdx.x * tiles;
  const size_t S = blockDim.x;
  const LZ xs = LZ::unpack(pw.p[lg_tile + lg_spine]);
  LZ acc = LZ::zero();
  for (size_t c = (tiles + S - 1) / S; c-- > 0;) {
    const size_t i = c * S + threadIdx.x;
    const LZ step = block_reduce(i < tiles ? t[i] : LZ::zero(), lds, EvalOp<F>{&pw, lg_tile});
    acc = LZ::add(step, LZ::mul(acc, xs)).fold_top();
  }
  if (threadIdx.x == 0) out[blockIdx.x] = acc.canonical_wide().pack();
}

// ---- division by (X - r) ------------------------------------------------------------------------------------------------------------------
// factor_roots (co-noir-common polynomial.rs:183, shared_polynomial.rs:92-140) and div_by_zerofier(.., 1, beta) (co-plonk round5.rs:78-91),
// in the reference's direction: c = (-r)^-1, b_(-1) = 0, b_i = c (a_i - b_(i-1)). With w = 1 / r = -c this is s_i = a_i + w s_(i-1),
// b_i = c s_i: an inclusive scan under wsum_combine (field_scan.hpp) -- EvalOp's algebra as a scan, in the other direction. Coefficients
// and every s and b are R scale; w's powers and c are R'-domain operands, so no product needs times32().
template <class F>
struct DivOp {
  using LZ = LzOf<F>;
  const PowTable<F>* pw;
  int base;
  __device__ __forceinline__ LZ operator()(const LZ& lo, const LZ& hi, int k) const { return wsum_combine(lo, hi, LZ::unpack(pw->p[base + k])); }
  __device__ __forceinline__ LZ settle(const LZ& v) const { return v.fold_top(); }
  __device__ __forceinline__ LZ identity() const { return LZ::zero(); }
};
// what one call carries besides its vectors: c and the output scale (R' domain, canonical and packed), the value taken off coefficient 0
template <class F>
struct DivArgs {
  F c, scale, sub0[2];
  int scaled, accumulate;
};
// coefficient i of component comp as it enters the recurrence: 0 past the end, sub0 off the constant term
template <class F>
__device__ __forceinline__ LzOf<F> div_coeff(const F* in, size_t n, uint32_t ncomp, uint32_t comp, size_t i, const DivArgs<F>& a) {
  using LZ = LzOf<F>;
  LZ v = i < n ? LZ::unpack(in[i * ncomp + comp]) : LZ::zero();
  if (i == 0) v = LZ::sub(v, LZ::unpack(a.sub0[comp]));
  return v;
}

// Launch 1: tot[comp][tile] = the s the tile ends with when it starts from 0; blockIdx.y = component
template <class F>
__global__ __launch_bounds__(SCAN_TILE_MAX) void k_div_totals(const F* in, size_t n, uint32_t ncomp, int E, int lg_e, PowTable<F> pw,
                                                               DivArgs<F> a, LzOf<F>* tot) {
  using LZ = LzOf<F>;
  __shared__ LZ lds[16];
  const size_t base = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * (size_t)E;
  const uint32_t comp = blockIdx.y;
  const LZ w = LZ::unpack(pw.p[0]);
  LZ s = LZ::zero();
#pragma unroll 1
  for (int e = 0; e < E; ++e) s = LZ::add(div_coeff(in, n, ncomp, comp, base + e, a), LZ::mul(s, w));
  const LZ total = block_reduce(s, lds, DivOp<F>{&pw, lg_e});
  if (threadIdx.x == 0) tot[(size_t)comp * gridDim.x + blockIdx.x] = total;
}
// Launch 2: pre[comp][t] = the s in front of tile t; blockIdx.x = component. The spine also leaves lane_w[l] = w^(E l), l < 64, for
// the downsweep: there every lane would otherwise pay the 6 products of lane_powers itself.
template <class F>
__global__ __launch_bounds__(SCAN_SPINE_MAX) void k_div_spine(const LzOf<F>* tot, size_t tiles, int lg_e, int lg_tile, PowTable<F> pw,
                                                               LzOf<F>* pre, LzOf<F>* lane_w) {
  using LZ = LzOf<F>;
  __shared__ ScanLds<LZ> s;
  const LZ* t = tot + (size_t)blockIdx.x * tiles;
  LZ* p = pre + (size_t)blockIdx.x * tiles;
  if (blockIdx.x == 0) {
    const LZ lw = lane_powers(LZ::unpack(pw.p[lg_e]));
    if (threadIdx.x < 64) lane_w[threadIdx.x] = lw;
  }
  const LZ tile_w = lane_powers(LZ::unpack(pw.p[lg_tile]));
  const size_t S = blockDim.x;
  LZ carry = LZ::zero(), total;
  for (size_t c0 = 0; c0 < tiles; c0 += S) {
    const size_t i = c0 + threadIdx.x;
    const LZ before = block_excl_scan_wsum(i < tiles ? t[i] : LZ::zero(), carry, tile_w, pw, lg_tile, s, &total);
    if (i < tiles) p[i] = before;
    carry = total;
  }
}
// Launch 3: out[i] = b_i for i < n - 1 (times scale, added to what is there: DivArgs), rem[comp] = b_(n-1). A lane reads its whole
// run before it writes any of it, and no lane touches another's: out may equal in. The last tile is padded with zeros, which keep
// multiplying s by w, so b_(n-1) is taken where it appears, not from the spine's last carry.
template <class F, int E>
__global__ __launch_bounds__(SCAN_TILE_MAX) void k_div_down(const F* in, F* out, size_t n, uint32_t ncomp, int lg_e, PowTable<F> pw,
                                                             DivArgs<F> a, const LzOf<F>* pre, const LzOf<F>* lane_w, F* rem) {
  using LZ = LzOf<F>;
  __shared__ ScanLds<LZ> s;
  const size_t base = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * (size_t)E;
  const uint32_t comp = blockIdx.y;
  const LZ w = LZ::unpack(pw.p[0]), c = LZ::unpack(a.c);
  LZ x[E];
  LZ run = LZ::zero();
  run_for<0, E>([&](auto ic) CSH_LAMBDA_INLINE {
    constexpr int e = decltype(ic)::value;
    x[e] = div_coeff(in, n, ncomp, comp, base + e, a);
    run = LZ::add(x[e], LZ::mul(run, w));
  });
  LZ total;
  const LZ before = block_excl_scan_wsum(run, pre[(size_t)comp * gridDim.x + blockIdx.x], lane_w[threadIdx.x & 63], pw, lg_e, s, &total);
  LZ b = LZ::mul(before, c);  // b at (run start - 1)
  run_for<0, E>([&](auto ic) CSH_LAMBDA_INLINE {
    constexpr int e = decltype(ic)::value;
    const size_t i = base + e;
    b = LZ::mul(LZ::sub(x[e], b), c);
    if (i + 1 < n) {
      F* o = out + i * ncomp + comp;
      LZ r = a.scaled ? LZ::mul(b, LZ::unpack(a.scale)) : b;
      if (a.accumulate) r = LZ::add(LZ::unpack(*o), r);
      *o = r.canonical_wide().pack();
    } else if (i + 1 == n && rem) {
      rem[comp] = b.canonical_wide().pack();
    }
  });
}

// ---- typed launchers ------------------------------------------------------------------------------------------------------------------
template <class F>
struct ScanScratch {
  LzOf<F>*tot, *pre, *suf;
};
template <class F>
static int scan_scratch(const ScanPlan& p, size_t arrays, size_t rows, hipStream_t st, ScanScratch<F>* s) {
  Arena& ar = arena_for(st);
  const size_t count = p.tiles * rows;
  CSH_TRY(ar.reserve(arrays * Arena::padded(count * sizeof(LzOf<F>))));
  s->tot = ar.take<LzOf<F>>(count);
  s->pre = arrays > 1 ? ar.take<LzOf<F>>(count) : nullptr;
  s->suf = arrays > 2 ? ar.take<LzOf<F>>(count) : nullptr;
  return CSH_OK;
}

template <class F>
static int prefix_prod_t(const uint64_t* in, uint64_t* out, size_t n, hipStream_t st) {
  if (n == 0) return CSH_OK;
  const ScanPlan p = scan_plan(n);
  ScanScratch<F> s;
  CSH_TRY(scan_scratch<F>(p, 2, 1, st, &s));
  const dim3 grid((unsigned)p.tiles), blk(p.lanes);
  hipLaunchKernelGGL((k_scan_totals<F, false>), grid, blk, 0, st, (const F*)in, n, p.E, s.tot, (unsigned long long*)nullptr);
  hipLaunchKernelGGL((k_scan_spine<F, false>), dim3(1), dim3(p.spine), 0, st, s.tot, p.tiles, s.pre, s.suf);
  if (p.E == 4) hipLaunchKernelGGL((k_prefix_down<F, 4>), grid, blk, 0, st, (const F*)in, (F*)out, n, s.pre);
  else hipLaunchKernelGGL((k_prefix_down<F, 8>), grid, blk, 0, st, (const F*)in, (F*)out, n, s.pre);
  CSH_HIP(hipGetLastError());
  return CSH_OK;
}

template <class F>
static int batch_inverse_t(const uint64_t* in, uint64_t* out, size_t n, uint64_t* zero_count, hipStream_t st) {
  if (zero_count) CSH_HIP(hipMemsetAsync(zero_count, 0, sizeof(uint64_t), st));
  if (n == 0) return CSH_OK;
  const ScanPlan p = scan_plan(n);
  ScanScratch<F> s;
  CSH_TRY(scan_scratch<F>(p, 3, 1, st, &s));
  const dim3 grid((unsigned)p.tiles), blk(p.lanes);
  hipLaunchKernelGGL((k_scan_totals<F, true>), grid, blk, 0, st, (const F*)in, n, p.E, s.tot, (unsigned long long*)zero_count);
  hipLaunchKernelGGL((k_scan_spine<F, true>), dim3(1), dim3(p.spine), 0, st, s.tot, p.tiles, s.pre, s.suf);
  if (p.E == 4) hipLaunchKernelGGL((k_inverse_down<F, 4>), grid, blk, 0, st, (const F*)in, (F*)out, n, s.pre, s.suf);
  else hipLaunchKernelGGL((k_inverse_down<F, 8>), grid, blk, 0, st, (const F*)in, (F*)out, n, s.pre, s.suf);
  CSH_HIP(hipGetLastError());
  return CSH_OK;
}

template <class F>
static int eval_poly_t(const uint64_t* coeffs, size_t n, uint32_t ncomp, const uint64_t point[4], uint64_t* out, hipStream_t st) {
  using LZ = LzOf<F>;
  if (n == 0) {
    CSH_HIP(hipMemsetAsync(out, 0, sizeof(F) * ncomp, st));
    return CSH_OK;
  }
  const F x = fr_load<F>(point);
  if (x.is_zero()) {  // the value at 0 is the constant term
    CSH_HIP(hipMemcpyAsync(out, coeffs, sizeof(F) * ncomp, hipMemcpyDeviceToDevice, st));
    return CSH_OK;
  }
  const PowTable<F> pw = pow_table<LZ, F>(LZ::from_fp(x));
  const ScanPlan p = scan_plan(n);
  ScanScratch<F> s;
  CSH_TRY(scan_scratch<F>(p, 1, ncomp, st, &s));
  hipLaunchKernelGGL(k_eval_totals<F>, dim3((unsigned)p.tiles, ncomp), dim3(p.lanes), 0, st, (const F*)coeffs, n, ncomp, p.E, p.lg_e, pw, s.tot);
  hipLaunchKernelGGL(k_eval_spine<F>, dim3(ncomp), dim3(p.spine), 0, st, s.tot, p.tiles, p.lg_e + p.lg_lanes, p.lg_spine, pw, (F*)out);
  CSH_HIP(hipGetLastError());
  return CSH_OK;
}

template <class F>
static int poly_div_linear_t(const uint64_t* in, size_t n, uint32_t ncomp, const uint64_t root[4], const uint64_t* sub0, const uint64_t* scale,
                             int accumulate, uint64_t* out, uint64_t* rem, hipStream_t st) {
  using LZ = LzOf<F>;
  if (n == 0) {
    if (rem) CSH_HIP(hipMemsetAsync(rem, 0, sizeof(F) * ncomp, st));
    return CSH_OK;
  }
  if (n == 1 && !rem) return CSH_OK;  // no quotient coefficient, and nobody asks for b_0
  const F w = F::inv(fr_load<F>(root));  // the one inversion, on the host
  const PowTable<F> pw = pow_table<LZ, F>(LZ::from_fp(w));
  DivArgs<F> a;
  a.c = fr_to_rprime(F::neg(w));
  a.scaled = scale != nullptr;
  a.accumulate = accumulate;
  a.scale = scale ? fr_to_rprime(fr_load<F>(scale)) : F::zero();
  memset(a.sub0, 0, sizeof a.sub0);
  if (sub0) memcpy(a.sub0, sub0, sizeof(F) * ncomp);
  const ScanPlan p = scan_plan(n);
  Arena& ar = arena_for(st);
  const size_t count = p.tiles * ncomp;
  CSH_TRY(ar.reserve(2 * Arena::padded(count * sizeof(LZ)) + Arena::padded(64 * sizeof(LZ))));
  LZ* tot = ar.take<LZ>(count);
  LZ* pre = ar.take<LZ>(count);
  LZ* lane_w = ar.take<LZ>(64);
  const dim3 grid((unsigned)p.tiles, ncomp), blk(p.lanes);
  hipLaunchKernelGGL(k_div_totals<F>, grid, blk, 0, st, (const F*)in, n, ncomp, p.E, p.lg_e, pw, a, tot);
  hipLaunchKernelGGL(k_div_spine<F>, dim3(ncomp), dim3(p.spine), 0, st, tot, p.tiles, p.lg_e, p.lg_e + p.lg_lanes, pw, pre, lane_w);
  if (p.E == 4) hipLaunchKernelGGL((k_div_down<F, 4>), grid, blk, 0, st, (const F*)in, (F*)out, n, ncomp, p.lg_e, pw, a, pre, lane_w, (F*)rem);
  else hipLaunchKernelGGL((k_div_down<F, 8>), grid, blk, 0, st, (const F*)in, (F*)out, n, ncomp, p.lg_e, pw, a, pre, lane_w, (F*)rem);
  CSH_HIP(hipGetLastError());
  return CSH_OK;
}

}  // namespace csh

using namespace csh;

// every entry point makes its argument checks (fr_entry.hpp) before it asks for a device
extern "C" {

int csh_vec_prefix_prod_dev(csh_curve_t f, const uint64_t* in, uint64_t* out, size_t n, void* stream) {
  FR_REQUIRE_FIELD(f);
  FR_REQUIRE_N(n);
  CSH_REQUIRE(n == 0 || (in && out), "vec_prefix_prod: NULL argument");
  CSH_TRY(ensure_device());
  hipStream_t st = resolve_stream(stream);
  return FR_CALL(f, prefix_prod_t<F>(in, out, n, st));
}
int csh_vec_batch_inverse_dev(csh_curve_t f, const uint64_t* in, uint64_t* out, size_t n, uint64_t* zero_count, void* stream) {
  FR_REQUIRE_FIELD(f);
  FR_REQUIRE_N(n);
  CSH_REQUIRE(n == 0 || (in && out), "vec_batch_inverse: NULL argument");
  CSH_TRY(ensure_device());
  hipStream_t st = resolve_stream(stream);
  return FR_CALL(f, batch_inverse_t<F>(in, out, n, zero_count, st));
}
int csh_eval_poly_dev(csh_curve_t f, const uint64_t* coeffs, size_t n, uint32_t ncomp, const uint64_t point[4], uint64_t* out, void* stream) {
  FR_REQUIRE_FIELD(f);
  FR_REQUIRE_N(n);
  FR_REQUIRE_NCOMP(ncomp);
  CSH_REQUIRE(point && out && (n == 0 || coeffs), "eval_poly: NULL argument");
  CSH_TRY(ensure_device());
  hipStream_t st = resolve_stream(stream);
  return FR_CALL(f, eval_poly_t<F>(coeffs, n, ncomp, point, out, st));
}

// the checks both forms of the division make before they ask for a device
static int poly_div_linear_check(csh_curve_t f, const uint64_t* in, size_t n, uint32_t ncomp, const uint64_t* root, int accumulate,
                                 const uint64_t* out) {
  FR_REQUIRE_FIELD(f);
  FR_REQUIRE_N(n);
  FR_REQUIRE_NCOMP(ncomp);
  CSH_REQUIRE(root && (n == 0 || in) && (n <= 1 || out), "poly_div_linear: NULL argument");
  CSH_REQUIRE(root[0] | root[1] | root[2] | root[3], "poly_div_linear: root is 0 -- the quotient by X is a shift of the coefficients, do that instead");
  CSH_REQUIRE(!(accumulate && out == in), "poly_div_linear: accumulate needs out != in");
  return CSH_OK;
}
int csh_poly_div_linear_dev(csh_curve_t f, const uint64_t* in, size_t n, uint32_t ncomp, const uint64_t root[4], const uint64_t* sub0,
                            const uint64_t* scale, int accumulate, uint64_t* out, uint64_t* rem, void* stream) {
  CSH_TRY(poly_div_linear_check(f, in, n, ncomp, root, accumulate, out));
  CSH_TRY(ensure_device());
  hipStream_t st = resolve_stream(stream);
  return FR_CALL(f, poly_div_linear_t<F>(in, n, ncomp, root, sub0, scale, accumulate, out, rem, st));
}

// ---- host-pointer forms: H2D, compute, D2H on the thread's stream ------------------------------------------------------------------------
int csh_vec_prefix_prod(csh_curve_t f, const uint64_t* in, uint64_t* out, size_t n) {
  FR_REQUIRE_FIELD(f);
  FR_REQUIRE_N(n);
  CSH_REQUIRE(n == 0 || (in && out), "vec_prefix_prod: NULL argument");
  HostStage h;
  const size_t eb = 32 * n;
  CSH_TRY(h.begin(Arena::padded(eb)));
  if (n == 0) return CSH_OK;
  uint64_t* d;
  CSH_TRY(h.up(d, in, eb));
  CSH_TRY(csh_vec_prefix_prod_dev(f, d, d, n, h.st));
  return h.down(out, d, eb);
}
int csh_vec_batch_inverse(csh_curve_t f, const uint64_t* in, uint64_t* out, size_t n, size_t* zero_count) {
  FR_REQUIRE_FIELD(f);
  FR_REQUIRE_N(n);
  CSH_REQUIRE(n == 0 || (in && out), "vec_batch_inverse: NULL argument");
  HostStage h;
  const size_t eb = 32 * n;
  CSH_TRY(h.begin(Arena::padded(eb) + Arena::padded(sizeof(uint64_t))));
  if (zero_count) *zero_count = 0;
  if (n == 0) return CSH_OK;
  uint64_t *d, *dz;
  CSH_TRY(h.up(d, in, eb));
  CSH_TRY(h.up(dz, nullptr, sizeof(uint64_t)));
  CSH_TRY(csh_vec_batch_inverse_dev(f, d, d, n, dz, h.st));
  uint64_t zc = 0;
  CSH_HIP(hipMemcpyAsync(&zc, dz, sizeof zc, hipMemcpyDeviceToHost, h.st));
  CSH_TRY(h.down(out, d, eb));
  CSH_HIP(hipStreamSynchronize(h.st));
  if (zero_count) *zero_count = (size_t)zc;
  return CSH_OK;
}
int csh_eval_poly(csh_curve_t f, const uint64_t* coeffs, size_t n, uint32_t ncomp, const uint64_t point[4], uint64_t* out) {
  FR_REQUIRE_FIELD(f);
  FR_REQUIRE_N(n);
  FR_REQUIRE_NCOMP(ncomp);
  CSH_REQUIRE(point && out && (n == 0 || coeffs), "eval_poly: NULL argument");
  HostStage h;
  const size_t cb = 32 * n * ncomp, ob = 32 * ncomp;
  CSH_TRY(h.begin(Arena::padded(cb) + Arena::padded(ob)));
  uint64_t *dc, *dout;
  CSH_TRY(h.up(dc, coeffs, cb));
  CSH_TRY(h.up(dout, nullptr, ob));
  CSH_TRY(csh_eval_poly_dev(f, dc, n, ncomp, point, dout, h.st));
  return h.down(out, dout, ob);
}

int csh_poly_div_linear(csh_curve_t f, const uint64_t* in, size_t n, uint32_t ncomp, const uint64_t root[4], const uint64_t* sub0, uint64_t* out,
                        uint64_t* rem) {
  CSH_TRY(poly_div_linear_check(f, in, n, ncomp, root, 0, out));
  HostStage h;
  const size_t cb = 32 * n * ncomp, ob = n ? 32 * (n - 1) * ncomp : 0, rb = 32 * ncomp;
  CSH_TRY(h.begin(Arena::padded(cb) + Arena::padded(rb)));
  uint64_t *d, *drem;
  CSH_TRY(h.up(d, in, cb));
  CSH_TRY(h.up(drem, nullptr, rb));
  CSH_TRY(csh_poly_div_linear_dev(f, d, n, ncomp, root, sub0, nullptr, 0, d, rem ? drem : nullptr, h.st));  // in place on the staged copy
  if (rem) CSH_HIP(hipMemcpyAsync(rem, drem, rb, hipMemcpyDeviceToHost, h.st));
  if (ob) CSH_TRY(h.down(out, d, ob));
  CSH_HIP(hipStreamSynchronize(h.st));
  return CSH_OK;
}

}  // extern "C"
