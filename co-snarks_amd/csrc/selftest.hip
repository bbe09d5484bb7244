// Host-executed self-test hooks: the SAME templates the gfx950 kernels instantiate (field.hpp, curve.hpp,
// field29.hpp, msm_digits.hpp) run on the CPU so that `pytest -m "not gpu"` can check them against the
// oracle without a device. Test infrastructure; not declared in include/cosnarks_hip.h.
#define CSH_CHECK_BOUNDS 1  // host-side limb-bound contract checks in field29.hpp
#include <string.h>

#include <functional>
#include <vector>

#include "common.hpp"
#include "curve.hpp"
#include "curve_lazy.hpp"
#include "chacha.hpp"
#include "field29.hpp"
#include "field_rand.hpp"
#include "field_scan.hpp"
#include "fr_entry.hpp"
#include "honk_oink.hpp"
#include "honk_relations.hpp"
#include "honk_gates.hpp"
#include "mle_fold.hpp"
#include "msm_digits.hpp"
#include "plonk_quot.hpp"
#include "plonk_rounds.hpp"
#include "poseidon2.hpp"
#include "shamir_rng.hpp"
#include "vec_elem.hpp"

using namespace csh;

namespace {

template <class F, bool IS_FP = true>
int field_op(int op, const void* a, const void* b, void* out) {
  F x, y, r;
  memcpy(&x, a, sizeof(F));
  if (b) memcpy(&y, b, sizeof(F)); else y = F::zero();
  switch (op) {
    case 0: r = F::add(x, y); break;
    case 1: r = F::sub(x, y); break;
    case 2: r = F::mul(x, y); break;
    case 3: r = F::inv(x); break;
    case 4: if constexpr (IS_FP) r = x.from_mont(); else return CSH_ERR_INVALID; break;
    case 5: if constexpr (IS_FP) r = x.to_mont(); else return CSH_ERR_INVALID; break;
    case 6: r = F::neg(x); break;
    case 7: r = F::sqr(x); break;
    default: return CSH_ERR_INVALID;
  }
  memcpy(out, &r, sizeof(F));
  return CSH_OK;
}

template <class Fq>
int curve_op(int op, const void* in1, const void* in2, uint32_t k, void* out) {
  XYZZ<Fq> acc, other;
  Affine<Fq> p;
  switch (op) {
    case 0:  // XYZZ += affine
      memcpy(&acc, in1, sizeof acc);
      memcpy(&p, in2, sizeof p);
      xyzz_madd(acc, p);
      memcpy(out, &acc, sizeof acc);
      return CSH_OK;
    case 1:  // XYZZ += XYZZ
      memcpy(&acc, in1, sizeof acc);
      memcpy(&other, in2, sizeof other);
      xyzz_add(acc, other);
      memcpy(out, &acc, sizeof acc);
      return CSH_OK;
    case 2:
      memcpy(&acc, in1, sizeof acc);
      acc = xyzz_dbl(acc);
      memcpy(out, &acc, sizeof acc);
      return CSH_OK;
    case 3:
      memcpy(&acc, in1, sizeof acc);
      acc = xyzz_mul_small(acc, k);
      memcpy(out, &acc, sizeof acc);
      return CSH_OK;
    case 4: {  // XYZZ -> affine
      memcpy(&acc, in1, sizeof acc);
      Affine<Fq> a = xyzz_to_affine(acc);
      memcpy(out, &a, sizeof a);
      return CSH_OK;
    }
    case 5: {  // affine -> XYZZ
      memcpy(&p, in1, sizeof p);
      acc = XYZZ<Fq>::from_affine(p);
      memcpy(out, &acc, sizeof acc);
      return CSH_OK;
    }
    default: return CSH_ERR_INVALID;
  }
}

// Lazy bucket accumulation on the host for any group: acc (empty) += sequence of `npts` affine points (negated
// where neg[i] != 0); out = XYZZ in arkworks words. Exercises exactly what k_msm_accum's lazy path does: storage
// repack, unpack, lazy_madd, export.
template <class L, class Fq>
int lazy_accumulate_t(const void* affine_pts, const uint8_t* neg, size_t npts, void* out_xyzz) {
  XYZZLazy<L> acc = XYZZLazy<L>::inf();
  const Affine<Fq>* pts = reinterpret_cast<const Affine<Fq>*>(affine_pts);
  for (size_t i = 0; i < npts; ++i) {
    Affine<Fq> p;
    memcpy(&p, pts + i, sizeof p);
    if (p.is_inf()) continue;
    Fq sx = L::repack_for_storage(p.x), sy = L::repack_for_storage(p.y);  // what Bases stores
    L x = L::unpack(sx), y = L::unpack(sy);
    if (neg && neg[i]) y = y.neg_unpacked();
    lazy_madd(acc, x, y);
  }
  XYZZ<Fq> r = lazy_to_xyzz<L, Fq>(acc);
  memcpy(out_xyzz, &r, sizeof r);
  return CSH_OK;
}

// Host run of the post-accumulation arithmetic (k_msm_merge / k_msm_reduce / k_msm_fold): groups of `group_len`
// points summed with lazy_madd, the group sums folded pairwise with lazy_add, the result times `weight`.
template <class L, class Fq>
int lazy_tree_t(const void* affine_pts, const uint8_t* neg, size_t npts, size_t group_len, uint32_t weight, void* out_xyzz) {
  const Affine<Fq>* pts = reinterpret_cast<const Affine<Fq>*>(affine_pts);
  std::vector<XYZZLazy<L>> parts;
  for (size_t g0 = 0; g0 < npts; g0 += group_len) {
    XYZZLazy<L> acc = XYZZLazy<L>::inf();
    for (size_t i = g0; i < npts && i < g0 + group_len; ++i) {
      Affine<Fq> p;
      memcpy(&p, pts + i, sizeof p);
      if (p.is_inf()) continue;
      L x = L::unpack(L::repack_for_storage(p.x)), y = L::unpack(L::repack_for_storage(p.y));
      if (neg && neg[i]) y = y.neg_unpacked();
      lazy_madd(acc, x, y);
    }
    parts.push_back(acc);
  }
  if (parts.empty()) parts.push_back(XYZZLazy<L>::inf());
  while (parts.size() > 1) {
    std::vector<XYZZLazy<L>> next;
    for (size_t i = 0; i + 1 < parts.size(); i += 2) {
      XYZZLazy<L> a = parts[i];
      if (i & 2) lazy_add_inl<L>(a, parts[i + 1]);  // both entry points
      else lazy_add_p<L>(&a, &parts[i + 1]);
      next.push_back(a);
    }
    if (parts.size() & 1) next.push_back(parts.back());
    parts.swap(next);
  }
  XYZZ<Fq> r = lazy_to_xyzz<L, Fq>(lazy_mul_small<L>(parts[0], weight));
  memcpy(out_xyzz, &r, sizeof r);
  return CSH_OK;
}

// Device-vs-host determinism check of the lazy bucket arithmetic: thread t accumulates the cyclic chain
// pts[(t + i) % n], i < len (sign from bit i of a hash) on the GPU; the host recomputes a sample of threads with the
// very same template code and compares the exported XYZZ words bit for bit.
template <class L, class Fq>
__host__ __device__ inline XYZZ<Fq> lazy_chain(const Affine<Fq>* pts, size_t n, size_t t, size_t len) {
  XYZZLazy<L> acc = XYZZLazy<L>::inf();
  len = 1 + (size_t)((t * 0x9E3779B1u) >> 8) % len;  // ragged chain lengths: lanes of a wave diverge, as in k_msm_accum
  for (size_t i = 0; i < len; ++i) {
    Affine<Fq> p = pts[(t + i) % n];
    if (p.is_inf()) continue;
    L x = L::unpack(p.x), y = L::unpack(p.y);
    if (((t * 2654435761u + i * 40503u) >> 7) & 1) y = y.neg_unpacked();
    lazy_madd(acc, x, y);
  }
  return lazy_to_xyzz<L, Fq>(acc);
}
template <class L, class Fq>
__global__ void k_lazy_chain(const Affine<Fq>* pts, size_t n, size_t len, size_t nthreads, XYZZ<Fq>* out) {
  const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (t < nthreads) out[t] = lazy_chain<L, Fq>(pts, n, t, len);
}
template <class L, class Fq>
int lazy_chain_check_t(const void* affine_pts, size_t n, size_t len, size_t nthreads, size_t host_samples, int* mismatches) {
  std::vector<Affine<Fq>> st(n);
  const Affine<Fq>* in = reinterpret_cast<const Affine<Fq>*>(affine_pts);
  for (size_t i = 0; i < n; ++i) {
    st[i] = in[i];
    if (!st[i].is_inf()) st[i] = {L::repack_for_storage(in[i].x), L::repack_for_storage(in[i].y)};
  }
  Affine<Fq>* dpts;
  XYZZ<Fq>* dout;
  CSH_HIP(hipMalloc((void**)&dpts, n * sizeof(Affine<Fq>)));
  CSH_HIP(hipMalloc((void**)&dout, nthreads * sizeof(XYZZ<Fq>)));
  CSH_HIP(hipMemcpy(dpts, st.data(), n * sizeof(Affine<Fq>), hipMemcpyHostToDevice));
  hipLaunchKernelGGL((k_lazy_chain<L, Fq>), dim3((unsigned)((nthreads + 127) / 128)), dim3(128), 0, 0, dpts, n, len, nthreads, dout);
  std::vector<XYZZ<Fq>> got(nthreads);
  CSH_HIP(hipMemcpy(got.data(), dout, nthreads * sizeof(XYZZ<Fq>), hipMemcpyDeviceToHost));
  (void)hipFree(dpts);
  (void)hipFree(dout);
  int bad = 0;
  const size_t step = nthreads / host_samples ? nthreads / host_samples : 1;
  for (size_t t = 0; t < nthreads; t += step) {
    XYZZ<Fq> want = lazy_chain<L, Fq>(st.data(), n, t, len);
    if (memcmp(&want, &got[t], sizeof want) != 0) ++bad;
  }
  *mismatches = bad;
  return CSH_OK;
}

}  // namespace

// Host run of the lazy NTT butterfly arithmetic (ntt.hip k_ntt_pass_lazy): a, b, w arkworks-Montgomery elements of the
// scalar field; k times  acc = (acc +/- b*w).normalized()  with the twiddle in the R' domain, then canonical_wide().pack().
// Expected: a +/- k*b*w (still arkworks-Montgomery). Exercises the value drift a pass accumulates and its reduction.
template <class F>
static int lazy_fr_chain_t(const uint64_t a[4], const uint64_t b[4], const uint64_t w[4], int k, int negative, uint64_t out[4]) {
  using LZ = LzOf<F>;
  LZ acc = LZ::unpack(fr_load<F>(a));
  const LZ lb = LZ::unpack(fr_load<F>(b));
  const LZ lw = LZ::unpack(LZ::repack_for_storage(fr_load<F>(w)));
  for (int i = 0; i < k; ++i) {  // as the decimation-in-time stages do: the carry step only every second stage
    const LZ x = LZ::mul(lb, lw);
    acc = negative ? LZ::sub(acc, x) : LZ::add(acc, x);
    if (i & 1) acc = acc.normalized();
    const LZ as_operand = LZ::mul(acc, lw);  // the other role of a stage output: `v` of the next product (limb-bound asserted)
    (void)as_operand;
  }
  {  // sums feeding sums (decimation in frequency): doubling with fold_top must stay exact and in range
    LZ d = acc;
    for (int i = 0; i < 12; ++i) d = LZ::add(d, d).fold_top();
    LZ two12 = LZ::unpack(LZ::repack_for_storage(F::from_u64(4096)));
    const F ra = LZ::mul(acc, two12).canonical_wide().pack(), rb = d.canonical_wide().pack();
    if (memcmp(&ra, &rb, 32) != 0) return 2;
  }
  // one more product with a drifted operand (what the next stage does with it), divided out again by w^-1 is not
  // available here: multiply by the R'-domain one instead (value unchanged, reduced)
  const LZ one = LZ::one();
  const LZ red = LZ::mul(acc, one);
  const F r1 = acc.canonical_wide().pack(), r2 = red.canonical_wide().pack();
  if (memcmp(&r1, &r2, 32) != 0) return 1;
  memcpy(out, &r1, 32);
  return CSH_OK;
}

// Host run of the share-vector kernels' per-element expressions: the functions of vec_elem.hpp that the kernels of vec_ops.hip call, with
// the limb-bound contract checked. op 0: a*b; 1: a*(c+d) + b*c + m (Rep3 local multiplication with la = a, lb = b, ra = c, rb = d, mask m);
// 2: a*b - c; 3: as 1 with the mask optional (m may be NULL) minus s (may be NULL); 4: a*c + b*d (Rep3 share {a, b} to Shamir with the
// translation points x = c, y = d). All arkworks-Montgomery in and out.
template <class F>
static int lazy_vec_t(int op, const uint64_t* a, const uint64_t* b, const uint64_t* c, const uint64_t* d, const uint64_t* m, const uint64_t* s, uint64_t* out) {
  if (op < 0 || op > 4 || !a || !b || !c || !out || (op != 0 && op != 2 && !d) || (op == 1 && !m)) return CSH_ERR_INVALID;
  const F fa = fr_load<F>(a), fb = fr_load<F>(b), fc = fr_load<F>(c), fd = d ? fr_load<F>(d) : F::zero(), fm = m ? fr_load<F>(m) : F::zero(),
          fs = op == 3 && s ? fr_load<F>(s) : F::zero();
  F r;
  switch (op) {
    case 0: r = elem_mul(fa, fb); break;
    case 1: r = elem_rep3_local_mul(fa, fb, fc, fd, &fm, (const F*)nullptr, 0); break;
    case 2: r = elem_mul_sub(fa, fb, fc); break;
    case 3: r = elem_rep3_local_mul(fa, fb, fc, fd, m ? &fm : nullptr, s ? &fs : nullptr, 0); break;
    default: r = elem_rep3_to_shamir(fa, fb, fc, fd); break;
  }
  memcpy(out, &r, 32);
  return CSH_OK;
}

// Fp2 products of the signed lazy field on RAW limbs (no conversion in front): the caller chooses every limb, so the column bound the
// routines were derived for can be driven to its edge (all limbs at +/-(2^B + 8)) -- the values are arbitrary integers, only defined mod p.
// limbs: 4 elements x 2 components x NL int32; op 0: a b, 1: a^2, 2: a^2 - b, 3: a b - c d. out: the result as arkworks Montgomery limbs.
template <class L2, class F2>
static int fp2s_raw_t(int op, const int32_t* limbs, uint64_t* out) {
  using LF = decltype(L2().c0);
  constexpr int NL = LF::NL;
  L2 v[4];
  for (int e = 0; e < 4; ++e)
    for (int i = 0; i < NL; ++i) {
      v[e].c0.l[i] = limbs[(2 * e) * NL + i];
      v[e].c1.l[i] = limbs[(2 * e + 1) * NL + i];
    }
  const L2 r = op == 0 ? L2::mul(v[0], v[1]) : op == 1 ? L2::sqr(v[0]) : op == 2 ? L2::sqr_sub(v[0], v[1]) : L2::mul_sub(v[0], v[1], v[2], v[3]);
  const F2 f = r.to_fp();
  memcpy(out, &f, sizeof f);
  return CSH_OK;
}

// The two halves of the lazy field's zero test, separately, on RAW signed limbs (n elements of NL int32 each; 2 NL for an Fp2S type):
// flags[i] = maybe_zero() | is_zero_slow() << 1 | is_zero() << 2. maybe_zero() looks at limb 0 only; the slow test decides.
template <class L>
static void zero_flags_one(const int32_t* limbs, L& v) {
  for (int i = 0; i < L::NL; ++i) v.l[i] = limbs[i];
}
template <class LF, class F2>
static void zero_flags_one(const int32_t* limbs, Fp2S<LF, F2>& v) {
  for (int i = 0; i < LF::NL; ++i) {
    v.c0.l[i] = limbs[i];
    v.c1.l[i] = limbs[LF::NL + i];
  }
}
template <class L>
static int zero_flags_t(const int32_t* limbs, size_t n, uint8_t* flags) {
  constexpr size_t words = sizeof(L) / sizeof(int32_t);
  for (size_t i = 0; i < n; ++i) {
    L v;
    zero_flags_one(limbs + i * words, v);
    flags[i] = (uint8_t)((v.maybe_zero() ? 1 : 0) | (v.is_zero_slow() ? 2 : 0) | (v.is_zero() ? 4 : 0));
  }
  return CSH_OK;
}
// Host run of the field scans' arithmetic (field_scan.hip) with the limb-bound checks on: the same routines and the same order of
// scales, lane after lane instead of side by side. op 0: running product; 1: batch inverse (zeros stay zero); 2: lazy_inv alone
// (n = 1). run = elements per lane. All arkworks-Montgomery in and out.
template <class F>
static int scan_host_t(int op, const uint64_t* in, size_t n, int run, uint64_t* out) {
  using LZ = LzOf<F>;
  std::vector<F> x(n);
  if (n) memcpy(x.data(), in, n * sizeof(F));
  InvScratch<LZ> scratch;
  if (op == 2) {
    for (size_t i = 0; i < n; ++i) {
      const F r = lazy_inv(LZ::from_fp(x[i]), scratch).to_fp();
      memcpy(out + 4 * i, &r, sizeof(F));
    }
    return CSH_OK;
  }
  std::vector<F> y(x);
  if (op == 1)
    for (F& v : y)
      if (v.is_zero()) v = F::one();
  const size_t lanes = (n + run - 1) / run;
  std::vector<LZ> tot(lanes), pre(lanes), suf(lanes);
  for (size_t l = 0; l < lanes; ++l) {  // k_scan_totals / load_run
    LZ acc = LZ::unpack(y[l * run]);
    for (size_t i = l * run + 1; i < n && i < (l + 1) * run; ++i) acc = LZ::mul(acc, LZ::unpack(y[i]).times32());
    tot[l] = to_domain(acc);
  }
  LZ carry = LZ::one();
  for (size_t l = 0; l < lanes; ++l) {  // block_excl_scan_mul<false>
    pre[l] = carry;
    carry = LZ::mul(carry, tot[l]);
  }
  if (op == 1) {
    carry = from_domain(lazy_inv(carry, scratch));  // k_scan_spine<INV>
    for (size_t l = lanes; l-- > 0;) {
      suf[l] = carry;
      carry = LZ::mul(carry, tot[l]);
    }
  }
  for (size_t l = 0; l < lanes; ++l) {
    const size_t lo = l * run, hi = (l + 1) * run < n ? (l + 1) * run : n;
    if (op == 0) {  // k_prefix_down
      LZ acc = LZ::mul(LZ::unpack(y[lo]), pre[l]);
      for (size_t i = lo; i < hi; ++i) {
        if (i > lo) acc = LZ::mul(acc, LZ::unpack(y[i]).times32());
        const F r = acc.canonical_wide().pack();
        memcpy(out + 4 * i, &r, sizeof(F));
      }
    } else {  // k_inverse_down
      std::vector<LZ> f(hi - lo);
      f[0] = pre[l];
      for (size_t i = lo + 1; i < hi; ++i) f[i - lo] = LZ::mul(f[i - lo - 1], LZ::unpack(y[i - 1]).times32());
      LZ after = suf[l];
      for (size_t i = hi; i-- > lo;) {
        const F r = x[i].is_zero() ? F::zero() : LZ::mul(f[i - lo], after).canonical_wide().pack();
        memcpy(out + 4 * i, &r, sizeof(F));
        after = LZ::mul(after, LZ::unpack(y[i]).times32());
      }
    }
  }
  return CSH_OK;
}
// Host run of the division by (X - r) (field_scan.hip: k_div_totals, block_excl_scan_wsum, k_div_down) with the limb-bound checks on:
// the same routines, the same levels and the same folds, lane after lane instead of side by side. One block of 64-lane waves (at most
// 16) after another, the carry handed on as the spine hands it to a tile. run = elements per lane, a power of two. out: b_0 .. b_(n-1)
// per component, the popped b_(n-1) included. All arkworks-Montgomery in and out.
template <class LZ>
static void hillis_steele(std::vector<LZ>& v, int levels, const std::function<LZ(const LZ& lo, const LZ& hi, int k)>& op) {
  for (int k = 0; k < levels; ++k) {
    const std::vector<LZ> old(v);
    for (size_t l = 0; l < v.size(); ++l) {
      const LZ m = op(old[l >= (size_t(1) << k) ? l - (size_t(1) << k) : l], old[l], k);  // a lane without a partner shuffles itself in
      if (l >= (size_t(1) << k)) v[l] = m;
    }
  }
}
template <class F>
static int divlin_host_t(const uint64_t* in, size_t n, uint32_t ncomp, int run, const uint64_t* root, const uint64_t* sub0, uint64_t* out) {
  using LZ = LzOf<F>;
  const F w = F::inv(fr_load<F>(root));
  const PowTable<F> pw = pow_table<LZ, F>(LZ::from_fp(w));
  const LZ wz = LZ::unpack(pw.p[0]), c = LZ::unpack(fr_to_rprime(F::neg(w)));
  int base = 0;
  while ((1 << base) < run) ++base;
  const size_t lanes = (n + run - 1) / run, block = 1024;
  for (uint32_t comp = 0; comp < ncomp; ++comp) {
    auto coeff = [&](size_t i) {
      const F x = i < n ? fr_load<F>(in + 4 * (i * ncomp + comp)) : F::zero(), s0 = i == 0 && sub0 ? fr_load<F>(sub0 + 4 * comp) : F::zero();
      return i == 0 ? LZ::sub(LZ::unpack(x), LZ::unpack(s0)) : LZ::unpack(x);
    };
    LZ carry = LZ::zero();
    for (size_t b0 = 0; b0 < lanes; b0 += block) {
      const size_t nl = ((lanes - b0 < block ? lanes - b0 : block) + 63) / 64 * 64, nw = nl / 64;
      std::vector<LZ> incl(nl), lane_w(64, LZ::unpack(pw.p[base])), wtot(16, LZ::zero());
      for (size_t l = 0; l < nl; ++l) {  // the lane runs
        LZ s = LZ::zero();
        for (int e = 0; e < run; ++e) s = LZ::add(coeff((b0 + l) * run + e), LZ::mul(s, wz));
        incl[l] = s;
      }
      hillis_steele<LZ>(lane_w, 6, [](const LZ& lo, const LZ& hi, int) { return LZ::mul(hi, lo); });  // lane_powers
      lane_w.insert(lane_w.begin(), LZ::one());
      for (size_t wv = 0; wv < nw; ++wv) {  // block_excl_scan_wsum
        std::vector<LZ> wave(incl.begin() + 64 * wv, incl.begin() + 64 * (wv + 1));
        hillis_steele<LZ>(wave, 6, [&](const LZ& lo, const LZ& hi, int k) { return wsum_combine(lo, hi, LZ::unpack(pw.p[base + k])); });
        for (size_t l = 0; l < 64; ++l) incl[64 * wv + l] = wave[l].fold_top();
        wtot[wv] = incl[64 * wv + 63];
      }
      wtot[0] = wsum_combine(carry, wtot[0], LZ::unpack(pw.p[base + 6]));
      hillis_steele<LZ>(wtot, 4, [&](const LZ& lo, const LZ& hi, int k) { return wsum_combine(lo, hi, LZ::unpack(pw.p[base + 6 + k])); });
      for (size_t l = 0; l < nl && (b0 + l) * run < n; ++l) {  // k_div_down
        const size_t wv = l / 64, ln = l % 64;
        const LZ before = wv ? wtot[wv - 1].fold_top() : carry;
        const LZ excl = ln ? LZ::add(incl[l - 1], LZ::mul(before, lane_w[ln])) : before;
        LZ b = LZ::mul(excl, c);
        for (size_t i = (b0 + l) * run; i < n && i < (b0 + l + 1) * run; ++i) {
          b = LZ::mul(LZ::sub(coeff(i), b), c);
          const F o = b.canonical_wide().pack();
          memcpy(out + 4 * (i * ncomp + comp), &o, sizeof(F));
        }
      }
      carry = wtot[nw - 1].fold_top();
    }
  }
  return CSH_OK;
}

// Host run of the multilinear folds (mle_fold.hip) with the limb-bound checks on: the launches, tiles and rounds of k_mle_fold_rounds with
// every level kept, fold_tile_round lane after lane instead of side by side, the limb planes in a vector instead of LDS -- and the same
// chain once more as m sweeps of k_mle_fold's elem_fold. The two must agree word for word (CSH_ERR_HIP otherwise: the decomposition changed
// a result). levels_out: levels 1..m back to back as csh_mle_fold_rounds lays them out. All arkworks-Montgomery in and out.
template <class F>
static int mle_fold_host_t(const uint64_t* in, size_t n, uint32_t ncomp, int T, const uint64_t* u, size_t m, uint64_t* levels_out) {
  using LZ = LzOf<F>;
  std::vector<F> src(n * ncomp), lev((n - (n >> m)) * ncomp);
  memcpy(src.data(), in, sizeof(F) * src.size());
  std::vector<int32_t> planes(LZ::NL * (fold_plane_a(T, ncomp) + fold_plane_b(T, ncomp)));
  const size_t launches = (m + T - 1) / T;
  for (size_t p = 0; p < launches; ++p) {
    FoldRoundsArgs<F> a;
    memset(&a, 0, sizeof a);
    a.rounds = (int)(m - p * T < (size_t)T ? m - p * T : (size_t)T);
    for (int r = 0; r < a.rounds; ++r) a.ud[r] = fr_to_rprime(fr_load<F>(u + 4 * (p * T + r)));
    a.in = p ? lev.data() + fold_level_offset(n, (int)(p * T)) * ncomp : src.data();
    a.n_in = n >> (p * T);
    a.ncomp = ncomp;
    a.tile_log = T;
    a.levels = lev.data() + fold_level_offset(n, (int)(p * T) + 1) * ncomp;
    a.last = nullptr;
    const size_t tiles = (a.n_in + ((size_t)1 << T) - 1) >> T;
    for (size_t tile = 0; tile < tiles; ++tile)
      for (int r = 1; r <= a.rounds; ++r)
        for (size_t lane = 0; lane < (size_t)FOLD_WG; ++lane) fold_tile_round(a, tile, r, lane, FOLD_WG, planes.data());
  }
  std::vector<F> cur(src), nxt;
  for (size_t l = 1; l <= m; ++l) {  // k_mle_fold, sweep after sweep
    const F ud = fr_to_rprime(fr_load<F>(u + 4 * (l - 1)));
    nxt.resize(cur.size() / 2);
    for (size_t o = 0; o < nxt.size(); ++o) {
      const size_t s = fold_src(o, ncomp);
      nxt[o] = elem_fold(cur[s], cur[s + ncomp], ud);
    }
    if (memcmp(nxt.data(), lev.data() + fold_level_offset(n, (int)l) * ncomp, sizeof(F) * nxt.size())) return CSH_ERR_HIP;
    cur.swap(nxt);
  }
  memcpy(levels_out, lev.data(), sizeof(F) * lev.size());
  return CSH_OK;
}

// fold_step (vec_elem.hpp) applied `rounds` times to a pair of LAZY values with nothing canonical in between, limb-bound checks on: what
// mle_fold.hpp claims about the bound not depending on the round, for any round count -- through the tiles a chain of R rounds needs 2^R
// elements. Each round (x, y) <- (x + u (y - x), y + u (x - y)); out receives both values after every round, canonical (copies: the
// chain goes on from the lazy ones).
template <class F>
static int fold_step_chain_t(const uint64_t* a, const uint64_t* b, const uint64_t* u, size_t rounds, uint64_t* out) {
  using LZ = LzOf<F>;
  const LZ ud = LZ::unpack(fr_to_rprime(fr_load<F>(u)));
  LZ x = LZ::unpack(fr_load<F>(a)), y = LZ::unpack(fr_load<F>(b));
  for (size_t r = 0; r < rounds; ++r) {
    const LZ nx = fold_step(x, y, ud), ny = fold_step(y, x, ud);
    x = nx;
    y = ny;
    const F ox = x.canonical_narrow().pack(), oy = y.canonical_narrow().pack();
    memcpy(out + 8 * r, &ox, sizeof(F));
    memcpy(out + 8 * r + 4, &oy, sizeof(F));
  }
  return CSH_OK;
}

// Host run of the PLONK quotient stages (plonk_quot.hip) with the limb-bound checks on: the argument structs are filled in by the same
// functions the launchers use, the power tables by pq_pow_tables_at, and every flat index goes through the pq_*_at() function its kernel
// calls -- on host arrays. `in`, `scalars` and `out` are laid out as the C entry point of the stage takes them (include/cosnarks_hip.h):
//   stage 0 blinders: scalars = b0..b8; out = ap, bp, cp, zp, zwp
//   stage 1 operands: in = the 11 shares, the 8 public vectors, then n_public Lagrange vectors; scalars = buffer_a (n_public shares), then
//                     beta, gamma, k1, k2; out = pi, e1, e1z, e2a, e2b, e2c, e3a, e3b, e3c, e3d
//   stage 2 combine:  in = the 14 shares, then L_1; scalars = alpha; out = t, tz
//   stage 3 finish:   N = 4 n; in = ct, ctz; scalars = b9, b10; out = t1, t2, t3
//   stage 4 tables:   out[0] = z1[0..4), z2[0..4), z3[0..4) as the library derives them from the generator (12 elements)
template <class F>
static int plonk_quot_host_t(int stage, const uint64_t* gen_w, size_t N, uint32_t protocol, uint32_t party, const uint64_t* const* in, size_t n_public,
                             const uint64_t* scalars, uint64_t* const* out) {
  const F gen = fr_load<F>(gen_w);
  const PqGeom g{N, protocol + 1, pq_pub_comp(protocol, party)};
  std::vector<F> hi(pq_pow_hi_count(N)), lo(size_t(1) << PQ_POW_LO_LOG);
  if (stage == 0 || stage == 1) {
    PqPowArgs<F> p;
    p.gd = fr_to_rprime(gen);
    p.hi = hi.data(), p.lo = lo.data(), p.n_hi = hi.size();
    for (size_t i = 0; i < hi.size() + lo.size(); ++i) pq_pow_tables_at(p, i);
  }
  switch (stage) {
    case 0: {
      PqBlindArgs<F> a;
      a.g = g;
      pq_blinders_consts(a, gen, scalars, g.ncomp);
      a.hi = hi.data(), a.lo = lo.data();
      for (int v = 0; v < 5; ++v) a.out[v] = (F*)out[v];
      for (int v = 0; v < 5; ++v)
        for (size_t e = 0; e < g.values(); ++e) pq_blinders_at(a, v, e);
      return CSH_OK;
    }
    case 1: {
      const uint64_t* const* pub = in + 11;
      const uint64_t* ch = scalars + 4 * g.ncomp * n_public;
      const F beta = fr_load<F>(ch), gamma = fr_load<F>(ch + 4), k1 = fr_load<F>(ch + 8), k2 = fr_load<F>(ch + 12);
      for (size_t j0 = 0; j0 == 0 || j0 < n_public; j0 += PQ_PI_CHUNK) {
        PqPiArgs<F> p;
        pq_pi_consts(p, in + 19, scalars, j0, n_public, g.ncomp);
        p.pi = (F*)out[0];
        p.g = g;
        for (size_t e = 0; e < g.values(); ++e) pq_pi_at(p, e);
      }
      {
        PqE1Args<F> a;
        const F** s[] = {&a.a, &a.b, &a.c, nullptr, &a.a_b, &a.a_bp, &a.ap_b, &a.ap_bp, &a.ap, &a.bp, &a.cp};
        for (int v = 0; v < 11; ++v)
          if (s[v]) *s[v] = (const F*)in[v];
        a.pi = (const F*)out[0];
        a.qm = (const F*)pub[0], a.ql = (const F*)pub[1], a.qr = (const F*)pub[2], a.qo = (const F*)pub[3], a.qc = (const F*)pub[4];
        a.e1 = (F*)out[1], a.e1z = (F*)out[2];
        const PqZ<F> z = pq_z_tables(gen, N);
        for (int m = 0; m < 4; ++m) a.z1d[m] = fr_to_rprime(z.z1[m]);
        a.g = g;
        for (size_t e = 0; e < g.values(); ++e) pq_e1_at(a, pq_e1_lane(a, e), e);
      }
      {
        PqE2Args<F> a;
        for (int v = 0; v < 3; ++v) a.in[v] = (const F*)in[v], a.out[v] = (F*)out[3 + v];
        a.bk[0] = beta, a.bk[1] = F::mul(beta, k1), a.bk[2] = F::mul(beta, k2);
        a.gamma = gamma;
        a.hi = hi.data(), a.lo = lo.data();
        a.g = g;
        for (size_t e = 0; e < g.values(); ++e) pq_e2_at(a, e);
      }
      {
        PqE3Args<F> a;
        for (int v = 0; v < 3; ++v) a.in[v] = (const F*)in[v], a.s[v] = (const F*)pub[5 + v], a.out[v] = (F*)out[6 + v];
        a.z = (const F*)in[3];
        a.e3d = (F*)out[9];
        a.betad = fr_to_rprime(beta);
        a.gamma = gamma;
        a.g = g;
        for (size_t e = 0; e < g.values(); ++e) pq_e3_at(a, e);
      }
      return CSH_OK;
    }
    case 2: {
      PqCombineArgs<F> a;
      a.g = g;
      a.e1 = (const F*)in[0], a.e1z = (const F*)in[1], a.z = (const F*)in[2], a.zp = (const F*)in[3], a.e2 = (const F*)in[4], a.e3 = (const F*)in[9];
      for (int j = 0; j < 4; ++j) a.e2z[j] = (const F*)in[5 + j], a.e3z[j] = (const F*)in[10 + j];
      a.l1 = (const F*)in[14];
      a.t = (F*)out[0], a.tz = (F*)out[1];
      a.k = pq_combine_consts(gen, N, fr_load<F>(scalars));
      for (size_t e = 0; e < g.values(); ++e) pq_combine_at(a, pq_combine_lane(a, e), e);
      return CSH_OK;
    }
    case 3: {
      PqFinishArgs<F> a;
      a.ct = (const F*)in[0], a.ctz = (const F*)in[1];
      a.t1 = (F*)out[0], a.t2 = (F*)out[1], a.t3 = (F*)out[2];
      pq_share(a.b9, scalars, g.ncomp);
      pq_share(a.b10, scalars + 4 * g.ncomp, g.ncomp);
      a.n = N / 4, a.ncomp = g.ncomp;
      for (size_t e = 0; e < a.n * a.ncomp; ++e) pq_finish_at(a, e);
      return CSH_OK;
    }
    case 4: {
      const PqZ<F> z = pq_z_tables(gen, N);
      memcpy(out[0], &z, sizeof z);
      return CSH_OK;
    }
  }
  return CSH_ERR_INVALID;
}

// Host run of the round-2 / round-5 stretches (plonk_rounds.hip) with the limb-bound checks on: the argument structs are filled in by the
// functions the launchers use and every flat index goes through the pr_*_at() function its kernel calls -- on host arrays.
//   entry 0 z operands: aux = the generator of the EXTENDED domain, n = its quarter; in = a, b, c (n shares), S1, S2, S3 (4 n elements);
//                       scalars = beta, gamma, k1, k2; out = n1, n2, n3, d1, d2, d3
//   entry 1 rotate:     in[0] (n shares) -> out[0], ks = k
//   entry 2 blind:      out[0] = the polynomial, n + k shares, in place; scalars = coeff_rev (k shares); ks = k
//   entry 3 lincomb:    n = out_len; in = the ks share vectors, then the kp public ones; lens = their lengths; scalars = the ks + kp
//                       coefficients; aux = const0 or NULL; out[0]
template <class F>
static int plonk_rounds_host_t(int entry, const uint64_t* aux, size_t n, uint32_t protocol, uint32_t party, const uint64_t* const* in,
                               const size_t* lens, const uint64_t* scalars, size_t ks, size_t kp, uint64_t* const* out) {
  const uint32_t ncomp = protocol + 1;
  switch (entry) {
    case 0: {
      PrZArgs<F> a;
      a.g = PqGeom{n, ncomp, pq_pub_comp(protocol, party)};
      std::vector<F> hi(pq_pow_hi_count(n)), lo(size_t(1) << PQ_POW_LO_LOG);
      PqPowArgs<F> p;
      p.gd = fr_to_rprime(F::pow_u64(fr_load<F>(aux), 4));
      p.hi = hi.data(), p.lo = lo.data(), p.n_hi = hi.size();
      for (size_t i = 0; i < hi.size() + lo.size(); ++i) pq_pow_tables_at(p, i);
      a.hi = hi.data(), a.lo = lo.data();
      for (int v = 0; v < 3; ++v) a.in[v] = (const F*)in[v], a.sigma[v] = (const F*)in[3 + v];
      for (int v = 0; v < 6; ++v) a.out[v] = (F*)out[v];
      pr_z_consts(a, scalars);
      for (size_t e = 0; e < a.g.values(); ++e) pr_z_num_at(a, e);
      for (size_t e = 0; e < a.g.values(); ++e) pr_z_den_at(a, e);
      return CSH_OK;
    }
    case 1: {
      if (ks >= n) return CSH_ERR_INVALID;
      PrRotArgs<F> a{(const F*)in[0], (F*)out[0], n, ks, ncomp};
      for (size_t e = 0; e < n * ncomp; ++e) pr_rotate_at(a, e);
      return CSH_OK;
    }
    case 2: {
      if (ks < 1 || ks > 3 || n < 3) return CSH_ERR_INVALID;
      PrBlindArgs<F> a;
      a.poly = (F*)out[0];
      a.n = n, a.ncomp = ncomp, a.k = (uint32_t)ks;
      pr_blind_consts(a, scalars, ncomp, a.k);
      for (size_t e = 0; e < ks * ncomp; ++e) pr_blind_at(a, e);
      return CSH_OK;
    }
    case 3: {
      if (ks > PR_LC_MAX_TERMS || kp > PR_LC_MAX_TERMS || ks + kp < 1) return CSH_ERR_INVALID;
      for (size_t j = 0; j < ks + kp; ++j)
        if (lens[j] > n) return CSH_ERR_INVALID;
      for (const PrLcArgs<F>& a : pr_lc_launches<F>(protocol, party, in, lens, scalars, ks, in + ks, lens + ks, scalars + 4 * ks, kp, aux, out[0], n))
        for (size_t e = 0; e < a.g.values(); ++e) pr_lc_at(a, e);
      return CSH_OK;
    }
  }
  return CSH_ERR_INVALID;
}

// Host run of the Oink stretches (honk_oink.hip) with the limb-bound checks on: the argument structs are filled in by the functions the
// launchers use and every flat index goes through the ho_*_at() function its kernel calls -- on host arrays.
//   entry 0 w4 records: in = w_l, w_r, w_o (n shares), type_share; idx = the read, write and shared lists, counts their lengths;
//                       scalars = eta_1, eta_2, eta_3; out[0] = w_4, in place
//   entry 1 lookup:     in = w_l, w_r, w_o, tags (n shares), then q_r, q_m, q_c, q_o, table_1..4, q_lookup (n elements); scalars = beta,
//                       gamma; out = prod, sel
//   entry 2 perm:       in = w_l, w_r, w_o, w_4 (n shares), then id_1..4, sigma_1..4; scalars = beta, gamma; out = n_1..4, d_1..4 (m shares)
//   entry 3 place:      in[0] = mul (m shares); out[0] = z (n shares)
template <class F>
static int honk_oink_host_t(int entry, size_t n, size_t domain_size, uint32_t protocol, uint32_t party, const uint64_t* const* in,
                            const uint32_t* const* idx, const size_t* counts, const size_t* ranges, size_t num_ranges, const uint64_t* scalars,
                            uint64_t* const* out) {
  const PqGeom rows{n, protocol + 1, pq_pub_comp(protocol, party)};
  switch (entry) {
    case 0: {
      if (!idx || !counts || counts[0] + counts[1] + counts[2] > n) return CSH_ERR_INVALID;
      HoW4Args<F> a;
      for (int k = 0; k < 3; ++k) a.w[k] = (const F*)in[k];
      a.w4 = (F*)out[0];
      a.read_idx = idx[0], a.write_idx = idx[1], a.shared_idx = idx[2];
      a.type_share = (const F*)in[3];
      a.n = n, a.n_read = (uint32_t)counts[0], a.n_write = (uint32_t)counts[1], a.n_shared = (uint32_t)counts[2];
      ho_w4_consts(a, scalars);
      a.g = PqGeom{counts[0] + counts[1] + counts[2], rows.ncomp, rows.pub_comp};
      for (size_t e = 0; e < a.g.values(); ++e) ho_w4_at(a, e);
      return CSH_OK;
    }
    case 1: {
      HoLookupArgs<F> a;
      HoSelArgs<F> s;
      a.g = s.g = rows;
      for (int k = 0; k < 3; ++k) a.w[k] = (const F*)in[k], a.q[k] = (const F*)in[4 + k];
      a.qo = (const F*)in[7];
      for (int k = 0; k < 4; ++k) a.tab[k] = (const F*)in[8 + k];
      a.prod = (F*)out[0];
      ho_lookup_consts(a, scalars);
      s.tag = (const F*)in[3], s.qlookup = (const F*)in[12], s.sel = (F*)out[1], s.one = F::one();
      for (size_t e = 0; e < rows.values(); ++e) ho_lookup_prod_at(a, e);
      for (size_t e = 0; e < rows.values(); ++e) ho_lookup_sel_at(s, e);
      return CSH_OK;
    }
    case 2: {
      HoPermArgs<F> a;
      CSH_TRY(ho_ranges(a.R, ranges, num_ranges, n, domain_size, "selftest_honk_oink"));
      a.g = PqGeom{(size_t)a.R.active - 1, rows.ncomp, rows.pub_comp};
      for (int k = 0; k < 4; ++k) a.w[k] = (const F*)in[k];
      a.betad = fr_to_rprime(fr_load<F>(scalars)), a.gamma = fr_load<F>(scalars + 4);
      for (int half = 0; half < 2; ++half) {
        for (int k = 0; k < 4; ++k) a.pub[k] = (const F*)in[4 + 4 * half + k], a.out[k] = (F*)out[4 * half + k];
        for (size_t e = 0; e < a.g.values(); ++e) ho_perm_at(a, e);
      }
      return CSH_OK;
    }
    case 3: {
      HoPlaceArgs<F> a;
      CSH_TRY(ho_ranges(a.R, ranges, num_ranges, n, domain_size, "selftest_honk_oink"));
      a.mul = (const F*)in[0], a.z = (F*)out[0];
      a.one = F::one();
      a.domain_size = (uint32_t)domain_size;
      a.g = rows;
      for (size_t e = 0; e < rows.values(); ++e) ho_place_at(a, e);
      return CSH_OK;
    }
  }
  return CSH_ERR_INVALID;
}

// The host runs of the sumcheck round's two entries (honk_relations.hip, honk_gates.hip) with the limb-bound checks on are
// honk_stage.hpp's hs_host_run: the argument struct is filled in by the function the launcher uses, and every edge of the range goes through
// the function a lane of k_hs_accumulate calls. acc = 57 and 110 elements.
template <class F>
static int honk_pow_table_host_t(const uint64_t* betas, size_t m, uint64_t* out) {
  HrPowArgs<F> a;
  memset(&a, 0, sizeof a);
  for (size_t b = 0; b < m; ++b) a.betad[b] = fr_to_rprime(fr_load<F>(betas + 4 * b));
  a.one = F::one();
  a.out = (F*)out, a.count = size_t(1) << m, a.m = (uint32_t)m;
  for (size_t i = 0; i < a.count; ++i) a.out[i] = hr_pow_at(a, i);
  return CSH_OK;
}

// The per-state functions of poseidon2.hpp on host arrays, dealt to no lanes, with the limb-bound checks of field29.hpp on.
// op 0: the plain kernel's body on n states (arg = take, flags bit 0 = the whole state is written, bit 1 = feed-forward): in -> out.
// op 1: step `arg` of the collaborative permutation on n states: `in` is copied to `out` (n t ncomp values), which is the state.
template <class F>
static int poseidon2_host_t(uint32_t t, uint32_t rf_b, uint32_t rf_e, uint32_t rp, const uint64_t* rc_ext, const uint64_t* rc_int, const uint64_t* diag,
                            int op, uint32_t protocol, uint32_t party, uint32_t arg, uint32_t flags, const uint64_t* in, size_t n, const uint64_t* y,
                            const uint64_t* const* pre, size_t pre_off, uint64_t* out, uint64_t* open, uint64_t* ff_out) {
  std::vector<F> store;
  P2Table<F> tab;
  p2_build_table(t, rf_b, rf_e, rp, rc_ext, rc_int, diag, store, tab);
  p2_point_table(tab, store.data());
  if (op == 0) {
    const P2PlainArgs<F> a{tab, (const F*)in, (F*)out, n, arg, flags & 1, (flags >> 1) & 1};
    for (size_t i = 0; i < n; ++i) t == 2 ? p2_plain_at<F, 2>(a, i) : t == 3 ? p2_plain_at<F, 3>(a, i) : p2_plain_at<F, 4>(a, i);
    return CSH_OK;
  }
  P2CoArgs<F> a;
  a.tab = tab, a.ncomp = protocol + 1, a.pub_comp = pq_pub_comp(protocol, party), a.step = arg, a.n_perm = n, a.pre_off = pre_off;
  memcpy(out, in, sizeof(F) * n * t * a.ncomp);
  a.state = (F*)out, a.y = (const F*)y, a.open = (F*)open, a.ff_out = arg == 0 ? (F*)ff_out : nullptr;
  for (int k = 0; k < 5; ++k) a.pre[k] = (const F*)pre[k];
  for (size_t u = 0; u < n * a.ncomp; ++u) t == 2 ? p2_co_step_at<F, 2>(a, u) : t == 3 ? p2_co_step_at<F, 3>(a, u) : p2_co_step_at<F, 4>(a, u);
  return CSH_OK;
}


// The stages of shamir_rng.hip on host arrays, dealt to no lanes: the same schedule, matrices, argument builders and per-element function.
// force: 0 = the draws of the shared streams (field_rand_host, the per-candidate function of the kernels; positions advance), 1 = every
// draw the limbs 0, 2 = every draw the limbs p - 1 (the matrix stage at the edges). send: the wire vectors (written); with recv given the finish stage runs
// too and r_t / r_2t receive amount * (t + 1) elements each.
template <class F>
static int shamir_rng_host_t(uint32_t id, uint32_t n, uint32_t t, const uint8_t* seeds, uint64_t* positions, size_t amount, int force, uint64_t* send,
                             const uint64_t* recv, bool finish, uint64_t* r_t, uint64_t* r_2t) {
  const ShamirSchedule s = shamir_schedule(n, t, id);
  const ShamirMatrices<F> m = shamir_matrices<F>(s);
  const ShamirWork w(s, amount);
  std::vector<F> work(w.total, F::zero());
  size_t off = 0;
  for (uint32_t q = 0; q + 1 < n; ++q) {
    const size_t cnt = s.per_stream[q] * amount;
    if (force == 0 && cnt) positions[q] = field_rand_host<F>(seeds + 32 * q, positions[q], cnt, work.data() + off);
    if (force == 2)
      for (size_t i = 0; i < cnt; ++i) work[off + i] = F::modulus(), work[off + i].l[0] -= 1;  // the limbs of p - 1 (p is odd)
    off += cnt;
  }
  auto run = [](const SmArgs<F>& a) {
    for (uint32_t tile = 0; tile < (a.R + SM_ROWS - 1) / SM_ROWS; ++tile)
      for (size_t i = 0; i < a.n; ++i) shamir_matmul_at(a, tile, i);
  };
  run(shamir_local_args<F>(s, 0, m.m.data() + m.off_t, m.rows_t, work.data(), amount, (F*)send));
  run(shamir_local_args<F>(s, 1, m.m.data() + m.off_2t, m.rows_2t, work.data(), amount, (F*)send));
  if (finish) {
    run(shamir_finish_args<F>(s, 0, m.m.data() + m.off_v, work.data(), amount, (const F*)recv, (F*)r_t));
    run(shamir_finish_args<F>(s, 1, m.m.data() + m.off_v, work.data(), amount, (const F*)recv, (F*)r_2t));
  }
  return CSH_OK;
}

extern "C" {

// the host loop over the kernels' per-candidate function (field_rand.hpp)
int csh_selftest_field_rand_host(int field_of, const uint8_t seed[32], uint64_t cand_begin, size_t n, uint64_t* out, uint64_t* cand_end) {
  if (!seed || (!out && n) || cand_begin > FRD_MAX_CAND) return CSH_ERR_INVALID;
  return FR_CALL(field_of, [&]() -> int {
    const uint64_t end = field_rand_host<F>(seed, cand_begin, n, (F*)out);
    if (cand_end) *cand_end = end;
    return CSH_OK;
  }());
}

// the per-candidate function on 32 given bytes (one half of a keystream block): *accepted and, if so, the element
int csh_selftest_field_rand_candidate(int field_of, const uint8_t bytes[32], uint64_t out[4], int* accepted) {
  if (!bytes || !out || !accepted) return CSH_ERR_INVALID;
  uint32_t words[16] = {0};
  memcpy(words + 8, bytes, 32);
  return FR_CALL(field_of, [&]() -> int {
    F v;
    *accepted = field_rand_candidate<F>(words, 1, v) ? 1 : 0;
    memcpy(out, &v, 32);
    return CSH_OK;
  }());
}

int csh_selftest_shamir_rng_host(int field_of, uint32_t id, uint32_t num_parties, uint32_t threshold, const uint8_t* seeds, uint64_t* positions,
                                 size_t amount, int force, uint64_t* send, const uint64_t* recv, int finish, uint64_t* r_t, uint64_t* r_2t) {
  if (shamir_params_refusal(id, num_parties, threshold) || !seeds || !positions || amount < 1 || force < 0 || force > 2) return CSH_ERR_INVALID;
  const bool wire = num_parties - threshold - 2 + num_parties - 2 * threshold - 1 != 0;
  if ((wire && (!send || (finish && !recv))) || (finish && (!r_t || !r_2t))) return CSH_ERR_INVALID;
  return FR_CALL(field_of, shamir_rng_host_t<F>(id, num_parties, threshold, seeds, positions, amount, force, send, recv, finish != 0, r_t, r_2t));
}

}

extern "C" {

int csh_selftest_poseidon2_host(int field_of, uint32_t t, uint32_t rf_b, uint32_t rf_e, uint32_t rp, const uint64_t* rc_ext, const uint64_t* rc_int,
                                const uint64_t* diag, int op, uint32_t protocol, uint32_t party, uint32_t arg, uint32_t flags, const uint64_t* in, size_t n,
                                const uint64_t* y, const uint64_t* const* pre, size_t pre_off, uint64_t* out, uint64_t* open, uint64_t* ff_out) {
  if (t < 2 || t > 4 || op < 0 || op > 1 || protocol > 1 || party > 2 || !diag || !in || !out || (op == 1 && !pre)) return CSH_ERR_INVALID;
  if (op == 0 && (arg < 1 || arg > t)) return CSH_ERR_INVALID;
  if (op == 1 && (arg > rf_b + rp + rf_e || pre_off < (arg ? ((arg - 1 < rf_b || arg - 1 >= rf_b + rp) ? n * t : n) : 0))) return CSH_ERR_INVALID;
  return FR_CALL(field_of, poseidon2_host_t<F>(t, rf_b, rf_e, rp, rc_ext, rc_int, diag, op, protocol, party, arg, flags, in, n, y, pre, pre_off, out, open, ff_out));
}

int csh_selftest_plonk_quot_host(int field_of, int stage, const uint64_t* gen, size_t N, uint32_t protocol, uint32_t party, const uint64_t* const* in,
                                 size_t n_public, const uint64_t* scalars, uint64_t* const* out) {
  if (!gen || !out || protocol > 1 || party > 2 || N < 32 || (N & (N - 1)) || stage < 0 || stage > 4) return CSH_ERR_INVALID;
  return FR_CALL(field_of, plonk_quot_host_t<F>(stage, gen, N, protocol, party, in, n_public, scalars, out));
}

int csh_selftest_plonk_rounds_host(int field_of, int entry, const uint64_t* aux, size_t n, uint32_t protocol, uint32_t party,
                                   const uint64_t* const* in, const size_t* lens, const uint64_t* scalars, size_t ks, size_t kp, uint64_t* const* out) {
  if (!out || protocol > 1 || party > 2 || entry < 0 || entry > 3 || (entry == 0 && (!aux || n < 8 || (n & (n - 1))))) return CSH_ERR_INVALID;
  return FR_CALL(field_of, plonk_rounds_host_t<F>(entry, aux, n, protocol, party, in, lens, scalars, ks, kp, out));
}

int csh_selftest_honk_oink_host(int field_of, int entry, size_t n, size_t domain_size, uint32_t protocol, uint32_t party, const uint64_t* const* in,
                                const uint32_t* const* idx, const size_t* counts, const size_t* ranges, size_t num_ranges, const uint64_t* scalars,
                                uint64_t* const* out) {
  if (!in || !out || protocol > 1 || party > 2 || entry < 0 || entry > 3 || (entry != 3 && !scalars) || n < 1 || n > FR_MAX_N) return CSH_ERR_INVALID;
  return FR_CALL(field_of, honk_oink_host_t<F>(entry, n, domain_size, protocol, party, in, idx, counts, ranges, num_ranges, scalars, out));
}

int csh_selftest_honk_relations_host(int field_of, const uint64_t* const* cols, size_t edge_begin, size_t edge_end, const uint64_t* scaling,
                                     size_t scaling_stride, const uint64_t* params, uint64_t* acc_out) {
  if (!cols || !params || !acc_out || (edge_begin & 1) || (edge_end & 1) || edge_begin >= edge_end || (scaling && !scaling_stride)) return CSH_ERR_INVALID;
  return FR_CALL(field_of, (hs_host_run<HrFam, F>(HsCall{cols, edge_begin, edge_end, scaling, scaling_stride, params, acc_out})));
}
int csh_selftest_honk_gates_host(int field_of, const uint64_t* const* cols, size_t edge_begin, size_t edge_end, const uint64_t* scaling,
                                 size_t scaling_stride, const uint64_t* params, uint64_t* acc_out) {
  if (!cols || !params || !acc_out || (edge_begin & 1) || (edge_end & 1) || edge_begin >= edge_end || (scaling && !scaling_stride)) return CSH_ERR_INVALID;
  return FR_CALL(field_of, (hs_host_run<HgFam, F>(HsCall{cols, edge_begin, edge_end, scaling, scaling_stride, params, acc_out})));
}
int csh_selftest_honk_pow_table_host(int field_of, const uint64_t* betas, size_t m, uint64_t* out) {
  if (!out || (m && !betas) || m > 20) return CSH_ERR_INVALID;
  return FR_CALL(field_of, honk_pow_table_host_t<F>(betas, m, out));
}

int csh_selftest_mle_fold_host(int field_of, const uint64_t* in, size_t n, uint32_t ncomp, int tile_log, const uint64_t* u, size_t m,
                               uint64_t* levels_out) {
  if (!in || !u || !levels_out || ncomp < 1 || ncomp > 2 || !fold_tile_log_ok(tile_log) || m < 1 || m > 28 || n < 2 ||
      (n & ((size_t(1) << m) - 1)))
    return CSH_ERR_INVALID;
  return FR_CALL(field_of, mle_fold_host_t<F>(in, n, ncomp, tile_log, u, m, levels_out));
}

int csh_selftest_fold_step_chain_host(int field_of, const uint64_t* a, const uint64_t* b, const uint64_t* u, size_t rounds, uint64_t* out) {
  if (!a || !b || !u || !out) return CSH_ERR_INVALID;
  return FR_CALL(field_of, fold_step_chain_t<F>(a, b, u, rounds, out));
}

int csh_selftest_divlin_host(int field_of, const uint64_t* in, size_t n, uint32_t ncomp, int run, const uint64_t* root, const uint64_t* sub0,
                             uint64_t* out) {
  if (run < 1 || (run & (run - 1)) || ncomp < 1 || ncomp > 2 || !root || !(root[0] | root[1] | root[2] | root[3])) return CSH_ERR_INVALID;
  return FR_CALL(field_of, divlin_host_t<F>(in, n, ncomp, run, root, sub0, out));
}

int csh_selftest_scan_host(int field_of, int op, const uint64_t* in, size_t n, int run, uint64_t* out) {
  if (op < 0 || op > 2 || run < 1) return CSH_ERR_INVALID;
  return FR_CALL(field_of, scan_host_t<F>(op, in, n, run, out));
}

// type: 0 Fq29s, 1 Fq28s, 2 Fr29s, 3 Fq28s377, 4 Fq29s2, 5 Fq28s2, 6 Fq28s377x2
int csh_selftest_zero_flags(int type, const int32_t* limbs, size_t n, uint8_t* flags) {
  switch (type) {
    case 0: return zero_flags_t<Fq29s>(limbs, n, flags);
    case 1: return zero_flags_t<Fq28s>(limbs, n, flags);
    case 2: return zero_flags_t<Fr29s>(limbs, n, flags);
    case 3: return zero_flags_t<Fq28s377>(limbs, n, flags);
    case 4: return zero_flags_t<Fq29s2>(limbs, n, flags);
    case 5: return zero_flags_t<Fq28s2>(limbs, n, flags);
    case 6: return zero_flags_t<Fq28s377x2>(limbs, n, flags);
    default: return CSH_ERR_INVALID;
  }
}

int csh_selftest_lazy_chain_dev(int curve, int group, const void* affine_pts, size_t n, size_t len, size_t nthreads, size_t host_samples,
                                int* mismatches) {
  CSH_TRY(ensure_device());
  if (curve == CSH_BN254 && group == CSH_G1) return lazy_chain_check_t<Fq29s, Bn254Fq>(affine_pts, n, len, nthreads, host_samples, mismatches);
  if (curve == CSH_BN254 && group == CSH_G2) return lazy_chain_check_t<Fq29s2, Bn254Fq2>(affine_pts, n, len, nthreads, host_samples, mismatches);
  if (curve == CSH_BLS12_381 && group == CSH_G1) return lazy_chain_check_t<Fq28s, Bls381Fq>(affine_pts, n, len, nthreads, host_samples, mismatches);
  if (curve == CSH_BLS12_381 && group == CSH_G2) return lazy_chain_check_t<Fq28s2, Bls381Fq2>(affine_pts, n, len, nthreads, host_samples, mismatches);
  if (curve == CSH_GRUMPKIN && group == CSH_G1) return lazy_chain_check_t<Fr29s, Bn254Fr>(affine_pts, n, len, nthreads, host_samples, mismatches);
  if (curve == CSH_BLS12_377 && group == CSH_G1) return lazy_chain_check_t<Fq28s377, Bls377Fq>(affine_pts, n, len, nthreads, host_samples, mismatches);
  if (curve == CSH_BLS12_377 && group == CSH_G2) return lazy_chain_check_t<Fq28s377x2, Bls377Fq2>(affine_pts, n, len, nthreads, host_samples, mismatches);
  return CSH_ERR_INVALID;
}


// field: 0 BN254 Fq, 1 BN254 Fr, 2 BLS12-381 Fq, 3 BLS12-381 Fr, 4 BLS12-377 Fq, 5 BLS12-377 Fr
int csh_selftest_field_op(int field, int op, const uint64_t* a, const uint64_t* b, uint64_t* out) {
  switch (field) {
    case 0: return field_op<Bn254Fq>(op, a, b, out);
    case 1: return field_op<Bn254Fr>(op, a, b, out);
    case 2: return field_op<Bls381Fq>(op, a, b, out);
    case 3: return field_op<Bls381Fr>(op, a, b, out);
    case 4: return field_op<Bls377Fq>(op, a, b, out);
    case 5: return field_op<Bls377Fr>(op, a, b, out);
    default: return CSH_ERR_INVALID;
  }
}

int csh_selftest_fp2_op(int curve, int op, const uint64_t* a, const uint64_t* b, uint64_t* out) {
  if (curve == CSH_BN254) return field_op<Bn254Fq2, false>(op, a, b, out);
  if (curve == CSH_BLS12_381) return field_op<Bls381Fq2, false>(op, a, b, out);
  if (curve == CSH_BLS12_377) return field_op<Bls377Fq2, false>(op, a, b, out);
  return CSH_ERR_INVALID;
}

int csh_selftest_curve_op(int curve, int group, int op, const void* in1, const void* in2, uint32_t k, void* out) {
  if (curve == CSH_BN254 && group == CSH_G1) return curve_op<Bn254Fq>(op, in1, in2, k, out);
  if (curve == CSH_BN254 && group == CSH_G2) return curve_op<Bn254Fq2>(op, in1, in2, k, out);
  if (curve == CSH_BLS12_381 && group == CSH_G1) return curve_op<Bls381Fq>(op, in1, in2, k, out);
  if (curve == CSH_BLS12_381 && group == CSH_G2) return curve_op<Bls381Fq2>(op, in1, in2, k, out);
  if (curve == CSH_GRUMPKIN && group == CSH_G1) return curve_op<Bn254Fr>(op, in1, in2, k, out);
  if (curve == CSH_BLS12_377 && group == CSH_G1) return curve_op<Bls377Fq>(op, in1, in2, k, out);
  if (curve == CSH_BLS12_377 && group == CSH_G2) return curve_op<Bls377Fq2>(op, in1, in2, k, out);
  return CSH_ERR_INVALID;
}

int csh_selftest_lazy_accumulate(int curve, int group, const void* affine_pts, const uint8_t* neg, size_t npts, void* out_xyzz) {
  if (curve == CSH_BN254 && group == CSH_G1) return lazy_accumulate_t<Fq29s, Bn254Fq>(affine_pts, neg, npts, out_xyzz);
  if (curve == CSH_BN254 && group == CSH_G2) return lazy_accumulate_t<Fq29s2, Bn254Fq2>(affine_pts, neg, npts, out_xyzz);
  if (curve == CSH_BLS12_381 && group == CSH_G1) return lazy_accumulate_t<Fq28s, Bls381Fq>(affine_pts, neg, npts, out_xyzz);
  if (curve == CSH_BLS12_381 && group == CSH_G2) return lazy_accumulate_t<Fq28s2, Bls381Fq2>(affine_pts, neg, npts, out_xyzz);
  if (curve == CSH_GRUMPKIN && group == CSH_G1) return lazy_accumulate_t<Fr29s, Bn254Fr>(affine_pts, neg, npts, out_xyzz);
  if (curve == CSH_BLS12_377 && group == CSH_G1) return lazy_accumulate_t<Fq28s377, Bls377Fq>(affine_pts, neg, npts, out_xyzz);
  if (curve == CSH_BLS12_377 && group == CSH_G2) return lazy_accumulate_t<Fq28s377x2, Bls377Fq2>(affine_pts, neg, npts, out_xyzz);
  return CSH_ERR_INVALID;
}

int csh_selftest_lazy_tree(int curve, int group, const void* affine_pts, const uint8_t* neg, size_t npts, size_t group_len, uint32_t weight,
                           void* out_xyzz) {
  if (group_len == 0) return CSH_ERR_INVALID;
  if (curve == CSH_BN254 && group == CSH_G1) return lazy_tree_t<Fq29s, Bn254Fq>(affine_pts, neg, npts, group_len, weight, out_xyzz);
  if (curve == CSH_BN254 && group == CSH_G2) return lazy_tree_t<Fq29s2, Bn254Fq2>(affine_pts, neg, npts, group_len, weight, out_xyzz);
  if (curve == CSH_BLS12_381 && group == CSH_G1) return lazy_tree_t<Fq28s, Bls381Fq>(affine_pts, neg, npts, group_len, weight, out_xyzz);
  if (curve == CSH_BLS12_381 && group == CSH_G2) return lazy_tree_t<Fq28s2, Bls381Fq2>(affine_pts, neg, npts, group_len, weight, out_xyzz);
  if (curve == CSH_GRUMPKIN && group == CSH_G1) return lazy_tree_t<Fr29s, Bn254Fr>(affine_pts, neg, npts, group_len, weight, out_xyzz);
  if (curve == CSH_BLS12_377 && group == CSH_G1) return lazy_tree_t<Fq28s377, Bls377Fq>(affine_pts, neg, npts, group_len, weight, out_xyzz);
  if (curve == CSH_BLS12_377 && group == CSH_G2) return lazy_tree_t<Fq28s377x2, Bls377Fq2>(affine_pts, neg, npts, group_len, weight, out_xyzz);
  return CSH_ERR_INVALID;
}

int csh_selftest_lazy_fr_chain(int field_of, const uint64_t a[4], const uint64_t b[4], const uint64_t w[4], int k, int negative, uint64_t out[4]) {
  return FR_CALL(field_of, lazy_fr_chain_t<F>(a, b, w, k, negative, out));
}

// s (the `sub` operand of op 3) comes last: ops 0 and 1 keep their numbers, their meaning and their arguments
int csh_selftest_lazy_vec(int field_of, int op, const uint64_t* a, const uint64_t* b, const uint64_t* c, const uint64_t* d, const uint64_t* m,
                          uint64_t* out, const uint64_t* s) {
  return FR_CALL(field_of, lazy_vec_t<F>(op, a, b, c, d, m, s, out));
}

// out = to_fp(mul(from_fp(a) (+/-) from_fp(b), from_fp(c))) for the signed lazy field: op 0: (a+b)*c, 1: (a-b)*c
int csh_selftest_lazys_op(int op, const uint64_t a[4], const uint64_t b[4], const uint64_t c[4], uint64_t out[4]) {
  using L = Fq29s;
  Bn254Fq fa, fb, fc;
  memcpy(&fa, a, 32);
  memcpy(&fb, b, 32);
  memcpy(&fc, c, 32);
  L la = L::from_fp(fa), lb = L::from_fp(fb), lc = L::from_fp(fc);
  L s = op == 0 ? L::add(la, lb) : L::sub(la, lb);
  Bn254Fq r = L::mul(s, lc).to_fp();
  memcpy(out, &r, 32);
  return s.is_zero() ? 1 : 0;   // also reports the zero test of (a +/- b)
}

int csh_selftest_fp2s_raw(int curve, int op, const int32_t* limbs, uint64_t* out) {
  if (curve == CSH_BN254) return fp2s_raw_t<Fq29s2, Bn254Fq2>(op, limbs, out);
  if (curve == CSH_BLS12_381) return fp2s_raw_t<Fq28s2, Bls381Fq2>(op, limbs, out);
  if (curve == CSH_BLS12_377) return fp2s_raw_t<Fq28s377x2, Bls377Fq2>(op, limbs, out);
  return CSH_ERR_INVALID;
}

// host execution of the on-device Rep3 mask generator (same template code as k_rep3_masks)
int csh_selftest_rep3_masks_host(int curve, const uint8_t seed1[32], uint64_t e1, const uint8_t seed2[32], uint64_t e2, uint64_t* out, size_t n) {
  uint32_t k1[8], k2[8];
  memcpy(k1, seed1, 32);
  memcpy(k2, seed2, 32);
  return with_fr((csh_curve_t)curve, [&](auto fr) -> int {
    for (size_t i = 0; i < n; ++i) {
      const auto v = rep3_mask_element<typename decltype(fr)::type>(k1, k2, e1 + i, e2 + i);
      memcpy(out + 4 * i, &v, 32);
    }
    return CSH_OK;
  });
}

// canonical scalar limbs -> signed digits (digits_out[w], w < *W_out)
int csh_selftest_digits(int curve, const uint64_t scalar[4], int c, int32_t* digits_out, int* W_out) {
  return with_fr((csh_curve_t)curve, [&](auto fr) -> int {
    const int W = windows_for(decltype(fr)::type::Params::BITS, c);
    uint32_t s[8];
    memcpy(s, scalar, 32);
    for (int w = 0; w < W; ++w) digits_out[w] = 0;
    for_each_digit<8>(s, c, W, [&](int w, uint32_t b, uint32_t neg) { digits_out[w] = neg ? -(int32_t)b : (int32_t)b; });
    *W_out = W;
    return CSH_OK;
  });
}

}  // extern "C"
