// Device-executed self-test hooks for the arithmetic that exists on the device only: curve_quad.hpp (one XYZZ point over a DPP
// quad) and curve_pair.hpp (one Fp2 value over a lane pair), plus a launcher of the real window-reduction and fold-tree kernels
// on bucket arrays the caller chooses, a runner of the MSM sort stage alone (digits, bucket offsets, bucket lists copied back), a runner of
// the bucket stage up to the per-bucket sums (the accumulate and merge launches of bucket_group on bucket lists the caller chooses), and host-pointer entry points around the two fused launchers that end a witness map
// (vec_ops.hip), which the C ABI reaches only through csh_groth16_h_dev. The kernels here are compiled with the device form of the limb-bound contract
// (field29.hpp, CSH_CHECK_BOUNDS_DEVICE): a violated operand bound is counted in g_bound_record, never trapped; every entry
// point hands the record back and clears it. Test infrastructure; not declared in include/cosnarks_hip.h.
#define CSH_CHECK_BOUNDS_DEVICE 1
#include <string.h>

#include <vector>

#include "msm_impl.hpp"

using namespace csh;

namespace csh {
// the tail launchers live with the kernels they launch (msm_inst_*.hip): no second instantiation of a k_msm_* kernel here
#define CSH_ST_TAIL_DECL(CFG)                                                                       \
  extern template int msm_tail_selftest_t<CFG>(const void*, uint32_t, uint32_t, int, void*); \
  extern template int msm_buckets_selftest_t<CFG>(const Bases*, int, int, const MsmParams*, const uint32_t*, const uint32_t*, const uint32_t*, BucketsSelftestRun<CFG>*);
CSH_ST_TAIL_DECL(Bn254G1Cfg)
CSH_ST_TAIL_DECL(Bn254G2Cfg)
CSH_ST_TAIL_DECL(Bls381G1Cfg)
CSH_ST_TAIL_DECL(Bls381G2Cfg)
CSH_ST_TAIL_DECL(GrumpkinG1Cfg)
CSH_ST_TAIL_DECL(Bls377G1Cfg)
CSH_ST_TAIL_DECL(Bls377G2Cfg)
// selftest_buckets_dev.hip, instantiated there for the seven configurations
template <class Cfg>
int st_bucket_export_launch(bool pair, const MsmParams& p, const uint32_t* start, const LazyPt<Cfg>* partial, const LazyPt<Cfg>* dense, LazyPt<Cfg>* out);
}  // namespace csh

namespace {

struct DevMem {
  void* p = nullptr;
  ~DevMem() {
    if (p) (void)hipFree(p);
  }
  int alloc(size_t bytes) {
    CSH_HIP(hipMalloc(&p, bytes ? bytes : 1));
    return CSH_OK;
  }
  template <class T>
  T* as() { return reinterpret_cast<T*>(p); }
};

int bound_record_clear() {
  const unsigned long long z[2] = {0, 0};
  CSH_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_bound_record), z, sizeof z));
  return CSH_OK;
}
// rec[0] = violating limbs, rec[1] = largest |limb|, rec[2] = its site (line of field29.hpp); the device record is cleared
int bound_record_take(uint64_t rec[3]) {
  unsigned long long r[2];
  CSH_HIP(hipDeviceSynchronize());
  CSH_HIP(hipMemcpyFromSymbol(r, HIP_SYMBOL(g_bound_record), sizeof r));
  rec[0] = r[0];
  rec[1] = r[1] >> 16;
  rec[2] = r[1] & 0xffff;
  return bound_record_clear();
}

// ---- positive control of the recorder: a raw-limb product whose first operand has every limb at 2^(B+2) -------------------
template <class LF>
__global__ void k_st_bound_control(int64_t* sink) {
  LF a, b;
  for (int i = 0; i < LF::NL; ++i) {
    a.l[i] = (int32_t)(1u << (LF::B + 2));
    b.l[i] = 3;
  }
  const typename LF::Wide w = LF::mul_wide(a, b);  // integer arithmetic on chosen inputs: 3 * 2^(B+2) * NL per column at most
  int64_t s = 0;
  for (int k = 0; k < 2 * LF::NL; ++k) s += w.t[k];
  sink[threadIdx.x] = s;
}
template <class LF>
int bound_control_t(uint64_t rec[3]) {
  DevMem sink;
  CSH_TRY(sink.alloc(64 * sizeof(int64_t)));
  CSH_TRY(bound_record_clear());
  hipLaunchKernelGGL(k_st_bound_control<LF>, dim3(1), dim3(64), 0, 0, sink.as<int64_t>());
  CSH_HIP(hipGetLastError());
  return bound_record_take(rec);
}

// ---- Fp2Pair products on raw limbs ---------------------------------------------------------------------------------------
// limbs: [npairs][4 elements][2 components][NL] int32; pair j = lanes 2j, 2j + 1. op 0: a b, 1: a^2, 2: a^2 - b, 3: a b - c d.
template <class LP, class F32>
__global__ __launch_bounds__(256) void k_st_fp2pair_raw(int op, const int32_t* __restrict__ limbs, uint32_t npairs, F32* out) {
  constexpr int NL = LP::NL;
  const uint32_t t = blockIdx.x * 256 + threadIdx.x, j = t >> 1;
  const int role = pair_role();
  if (j >= npairs) return;  // pair-uniform
  LP v[4];
  for (int e = 0; e < 4; ++e)
    for (int i = 0; i < NL; ++i) v[e].v.l[i] = limbs[(((size_t)j * 4 + e) * 2 + role) * NL + i];
  LP r;
  if (op == 0) r = LP::mul(v[0], v[1]);
  else if (op == 1) r = LP::sqr(v[0]);
  else if (op == 2) r = LP::sqr_sub(v[0], v[1]);
  else r = LP::mul_sub(v[0], v[1], v[2], v[3]);
  out[2 * (size_t)j + role] = r.v.to_fp();
}
template <class LP, class F32>
int fp2pair_raw_t(int op, const int32_t* limbs, size_t npairs, uint64_t* out, uint64_t rec[3]) {
  const size_t in_bytes = npairs * 8 * LP::NL * sizeof(int32_t), out_bytes = npairs * 2 * sizeof(F32);
  DevMem din, dout;
  CSH_TRY(din.alloc(in_bytes));
  CSH_TRY(dout.alloc(out_bytes));
  CSH_HIP(hipMemcpy(din.p, limbs, in_bytes, hipMemcpyHostToDevice));
  CSH_TRY(bound_record_clear());
  hipLaunchKernelGGL((k_st_fp2pair_raw<LP, F32>), dim3((unsigned)((2 * npairs + 255) / 256)), dim3(256), 0, 0, op, din.as<int32_t>(), (uint32_t)npairs,
                     dout.as<F32>());
  CSH_HIP(hipGetLastError());
  CSH_TRY(bound_record_take(rec));
  CSH_HIP(hipMemcpy(out, dout.p, out_bytes, hipMemcpyDeviceToHost));
  return CSH_OK;
}

// ---- the two zero tests of Fp2Pair on raw limbs --------------------------------------------------------------------------
// limbs: [npairs][2 components][NL]; flags[j] = maybe_zero() | is_zero_slow() << 1 | is_zero() << 2
template <class LP>
__global__ __launch_bounds__(256) void k_st_fp2pair_zero(const int32_t* __restrict__ limbs, uint32_t npairs, uint8_t* flags) {
  constexpr int NL = LP::NL;
  const uint32_t t = blockIdx.x * 256 + threadIdx.x, j = t >> 1;
  const int role = pair_role();
  if (j >= npairs) return;
  LP v;
  for (int i = 0; i < NL; ++i) v.v.l[i] = limbs[((size_t)j * 2 + role) * NL + i];
  const bool m = v.maybe_zero(), s = v.is_zero_slow(), z = v.is_zero();
  if (role == 0) flags[j] = (uint8_t)((m ? 1 : 0) | (s ? 2 : 0) | (z ? 4 : 0));
}
template <class LP>
int fp2pair_zero_t(const int32_t* limbs, size_t npairs, uint8_t* flags, uint64_t rec[3]) {
  const size_t in_bytes = npairs * 2 * LP::NL * sizeof(int32_t);
  DevMem din, dout;
  CSH_TRY(din.alloc(in_bytes));
  CSH_TRY(dout.alloc(npairs));
  CSH_HIP(hipMemcpy(din.p, limbs, in_bytes, hipMemcpyHostToDevice));
  CSH_TRY(bound_record_clear());
  hipLaunchKernelGGL(k_st_fp2pair_zero<LP>, dim3((unsigned)((2 * npairs + 255) / 256)), dim3(256), 0, 0, din.as<int32_t>(), (uint32_t)npairs, dout.as<uint8_t>());
  CSH_HIP(hipGetLastError());
  CSH_TRY(bound_record_take(rec));
  CSH_HIP(hipMemcpy(flags, dout.p, npairs, hipMemcpyDeviceToHost));
  return CSH_OK;
}

// ---- stored points, built on the host with the lane-serial templates ------------------------------------------------------
// slot s = the lazy_madd chain over pts[off[s] .. off[s + 1]) (negated where neg[i]): what the accumulate kernel leaves in a partial
// slot -- non-trivial zz / zzz from the second point on, `empty` with stale limbs after a cancellation, inf() for an empty range.
template <class L, class Fq>
void build_slots(const Affine<Fq>* pts, const uint8_t* neg, const uint32_t* off, size_t nslots, XYZZLazy<L>* out) {
  for (size_t s = 0; s < nslots; ++s) {
    XYZZLazy<L> acc = XYZZLazy<L>::inf();
    for (uint32_t i = off[s]; i < off[s + 1]; ++i) {
      Affine<Fq> p;
      memcpy(&p, pts + i, sizeof p);
      if (p.is_inf()) continue;
      L x = L::unpack(L::repack_for_storage(p.x)), y = L::unpack(L::repack_for_storage(p.y));
      if (neg && neg[i]) y = y.neg_unpacked();
      lazy_madd(acc, x, y);
    }
    memset(&out[s], 0, sizeof out[s]);  // the padding behind `empty` travels to the device too
    out[s].x = acc.x;
    out[s].y = acc.y;
    out[s].zz = acc.zz;
    out[s].zzz = acc.zzz;
    out[s].empty = acc.empty;
  }
}

// ---- scripted point operations: one script per quad / per pair -------------------------------------------------------------
// Two registers per unit (r0, r1; both start empty), an operation names its destination d: the other register is the source of
// ST_ADDR. A script is unit-uniform, so the lanes of a unit never diverge; adjacent units of one wave run different scripts.
struct StOp {
  uint32_t code, reg, arg, k;
};
enum : uint32_t {
  ST_LOAD = 0,  // d = slot[arg]
  ST_ADDP = 1,  // d += slot[arg]
  ST_ADDR = 2,  // d += the other register
  ST_ADDS = 3,  // d += d (the same words on both sides)
  ST_DBL = 4,   // d = 2 d
  ST_MULK = 5,  // d = k d
  ST_MADD = 6,  // d += stored affine point arg, negated if k (pair form only)
  ST_ADDK = 7,  // d += k * the other register (the window reduction's bridge over a gap)
  ST_NOPS = 8
};

// Every primitive has ONE call site in a kernel (an operation sets its operands up and falls into the shared sites): six inlined
// copies of the addition would take the compiler a quarter of an hour. The registers are plain variables, exchanged by value where an
// operation names r1 -- no indexed register arrays, no pointers into private memory.
template <class T>
__device__ __forceinline__ void st_swap(T& a, T& b) {
  const T t = a;
  a = b;
  b = t;
}

template <class L>
__global__ __launch_bounds__(256) void k_st_quad_ops(const XYZZLazy<L>* __restrict__ slots, const StOp* __restrict__ ops, const uint32_t* __restrict__ unit_off,
                                                     uint32_t nunits, XYZZLazy<L>* out) {
  const int role = threadIdx.x & 3;
  const uint32_t u = (blockIdx.x * 256 + threadIdx.x) >> 2;
  if (u >= nunits) return;  // quad-uniform
  QPt<L> d = qpt_inf<L>(), o = qpt_inf<L>();
  for (uint32_t i = unit_off[u]; i < unit_off[u + 1]; ++i) {
    const StOp op = ops[i];
    if (op.reg & 1) st_swap(d, o);
    QPt<L> p = qpt_inf<L>();
    bool add = false;
    if (op.code == ST_LOAD || op.code == ST_ADDP) {
      p = qpt_load<L>(&slots[op.arg], role);
      if (op.code == ST_LOAD) d = p;
      else add = true;
    } else if (op.code == ST_ADDR) {
      p = o;
      add = true;
    } else if (op.code == ST_ADDS) {
      p = d;
      add = true;
    } else if (op.code == ST_MULK || op.code == ST_ADDK) {
      p = qmul_small<L>(op.code == ST_ADDK ? o : d, op.k, role);
      if (op.code == ST_MULK) d = p;
      else add = true;
    }
    if (add) qadd<L>(d, p, role);
    if (op.code == ST_DBL) qdbl<L>(d, role);
    if (op.reg & 1) st_swap(d, o);
  }
  qpt_store<L>(&out[2 * (size_t)u], role, d);
  qpt_store<L>(&out[2 * (size_t)u + 1], role, o);
}

template <class LS, class LP, class Fq>  // LS: the whole-element type of the stored layout, LP: its lane-pair form
__global__ __launch_bounds__(256) void k_st_pair_ops(const XYZZLazy<LS>* __restrict__ slots, const Affine<Fq>* __restrict__ aff, const StOp* __restrict__ ops,
                                                     const uint32_t* __restrict__ unit_off, uint32_t nunits, XYZZLazy<LS>* out) {
  const int role = pair_role();
  const uint32_t u = (blockIdx.x * 256 + threadIdx.x) >> 1;
  if (u >= nunits) return;  // pair-uniform
  XYZZLazy<LP> d = XYZZLazy<LP>::inf(), o = XYZZLazy<LP>::inf();
  for (uint32_t i = unit_off[u]; i < unit_off[u + 1]; ++i) {
    const StOp op = ops[i];
    if (op.reg & 1) st_swap(d, o);
    XYZZLazy<LP> p = XYZZLazy<LP>::inf();
    bool add = false;
    if (op.code == ST_LOAD || op.code == ST_ADDP) {
      p = pair_load(&slots[op.arg], role);
      if (op.code == ST_LOAD) d = p;
      else add = true;
    } else if (op.code == ST_ADDR) {
      p = o;
      add = true;
    } else if (op.code == ST_ADDS) {
      p = d;
      add = true;
    } else if (op.code == ST_MULK || op.code == ST_ADDK) {
      p = lazy_mul_small<LP, true>(op.code == ST_ADDK ? o : d, op.k);
      if (op.code == ST_MULK) d = p;
      else add = true;
    } else if (op.code == ST_MADD) {  // as k_msm_accum_pair feeds lazy_madd
      LP x, y;
      pair_unpack_affine<LP, Affine<Fq>>(aff + op.arg, &x, &y);
      y = y.cneg_unpacked(op.k & 1u);
      lazy_madd<LP, Affine<Fq>>(d, x, y, aff + op.arg, op.k & 1u);
    }
    if (add) lazy_add_inl<LP>(d, p);
    if (op.code == ST_DBL) d = lazy_dbl_inl<LP>(d);
    if (op.reg & 1) st_swap(d, o);
  }
  pair_store(&out[2 * (size_t)u], role, d);
  pair_store(&out[2 * (size_t)u + 1], role, o);
}

template <class L, class Fq>
__global__ __launch_bounds__(128) void k_st_export(const XYZZLazy<L>* __restrict__ in, uint32_t n, XYZZ<Fq>* out) {
  const uint32_t i = blockIdx.x * 128 + threadIdx.x;
  if (i < n) out[i] = lazy_to_xyzz<L, Fq>(in[i]);
}

// form 1: four lanes per point (curve_quad.hpp), form 2: two lanes per Fp2 point (curve_pair.hpp; LP = void on the G1 groups)
template <class L, class LP, class Fq>
int point_ops_t(int form, const void* affine_pts, const uint8_t* neg, size_t npts, const uint32_t* slot_off, size_t nslots, const uint32_t* ops_words,
                const uint32_t* unit_off, size_t nunits, void* out_xyzz, uint64_t rec[3]) {
  constexpr bool HAS_PAIR = !std::is_void<LP>::value;
  if (form != 1 && !(form == 2 && HAS_PAIR)) return CSH_ERR_INVALID;
  if (!nunits || !nslots || nunits > (1u << 20) || nslots > (1u << 20)) return CSH_ERR_INVALID;
  const Affine<Fq>* pts = reinterpret_cast<const Affine<Fq>*>(affine_pts);
  for (size_t s = 0; s < nslots; ++s)
    if (slot_off[s] > slot_off[s + 1] || slot_off[s + 1] > npts) return CSH_ERR_INVALID;
  const size_t nops = unit_off[nunits];
  const StOp* ops = reinterpret_cast<const StOp*>(ops_words);
  for (size_t u = 0; u < nunits; ++u)
    if (unit_off[u] > unit_off[u + 1]) return CSH_ERR_INVALID;
  for (size_t i = 0; i < nops; ++i) {  // every index a kernel will use, checked here
    const StOp& o = ops[i];
    if (o.code >= ST_NOPS || o.reg > 1) return CSH_ERR_INVALID;
    if ((o.code == ST_LOAD || o.code == ST_ADDP) && o.arg >= nslots) return CSH_ERR_INVALID;
    if (o.code == ST_MADD) {
      if (form != 2 || o.arg >= npts) return CSH_ERR_INVALID;
      Affine<Fq> p;
      memcpy(&p, pts + o.arg, sizeof p);
      if (p.is_inf()) return CSH_ERR_INVALID;  // the accumulate kernel filters infinity before lazy_madd
    }
  }
  std::vector<XYZZLazy<L>> slots(nslots);
  build_slots<L, Fq>(pts, neg, slot_off, nslots, slots.data());
  std::vector<Affine<Fq>> stored(npts ? npts : 1);
  for (size_t i = 0; i < npts; ++i) {
    memcpy(&stored[i], pts + i, sizeof(Affine<Fq>));
    if (!stored[i].is_inf()) stored[i] = {L::repack_for_storage(stored[i].x), L::repack_for_storage(stored[i].y)};
  }
  DevMem dslots, daff, dops, doff, dout, dx;
  CSH_TRY(dslots.alloc(nslots * sizeof(XYZZLazy<L>)));
  CSH_TRY(daff.alloc(stored.size() * sizeof(Affine<Fq>)));
  CSH_TRY(dops.alloc(nops * sizeof(StOp)));
  CSH_TRY(doff.alloc((nunits + 1) * sizeof(uint32_t)));
  CSH_TRY(dout.alloc(2 * nunits * sizeof(XYZZLazy<L>)));
  CSH_TRY(dx.alloc(2 * nunits * sizeof(XYZZ<Fq>)));
  CSH_HIP(hipMemcpy(dslots.p, slots.data(), nslots * sizeof(XYZZLazy<L>), hipMemcpyHostToDevice));
  CSH_HIP(hipMemcpy(daff.p, stored.data(), stored.size() * sizeof(Affine<Fq>), hipMemcpyHostToDevice));
  if (nops) CSH_HIP(hipMemcpy(dops.p, ops, nops * sizeof(StOp), hipMemcpyHostToDevice));
  CSH_HIP(hipMemcpy(doff.p, unit_off, (nunits + 1) * sizeof(uint32_t), hipMemcpyHostToDevice));
  CSH_HIP(hipMemset(dout.p, 0, 2 * nunits * sizeof(XYZZLazy<L>)));
  CSH_TRY(bound_record_clear());
  if (form == 1) {
    hipLaunchKernelGGL(k_st_quad_ops<L>, dim3((unsigned)((4 * nunits + 255) / 256)), dim3(256), 0, 0, dslots.as<XYZZLazy<L>>(), dops.as<StOp>(),
                       doff.as<uint32_t>(), (uint32_t)nunits, dout.as<XYZZLazy<L>>());
  } else {
    if constexpr (HAS_PAIR)
      hipLaunchKernelGGL((k_st_pair_ops<L, LP, Fq>), dim3((unsigned)((2 * nunits + 255) / 256)), dim3(256), 0, 0, dslots.as<XYZZLazy<L>>(),
                         daff.as<Affine<Fq>>(), dops.as<StOp>(), doff.as<uint32_t>(), (uint32_t)nunits, dout.as<XYZZLazy<L>>());
  }
  CSH_HIP(hipGetLastError());
  hipLaunchKernelGGL((k_st_export<L, Fq>), dim3((unsigned)((2 * nunits + 127) / 128)), dim3(128), 0, 0, dout.as<XYZZLazy<L>>(), (uint32_t)(2 * nunits),
                     dx.as<XYZZ<Fq>>());
  CSH_HIP(hipGetLastError());
  CSH_TRY(bound_record_take(rec));
  CSH_HIP(hipMemcpy(out_xyzz, dx.p, 2 * nunits * sizeof(XYZZ<Fq>), hipMemcpyDeviceToHost));
  return CSH_OK;
}

// ---- the tail stages on chosen buckets --------------------------------------------------------------------------------------
// bucket ids[i] (1 .. NB, each at most once) = the chain over pts[off[i] .. off[i + 1]); every other bucket is empty
template <class Cfg>
int msm_tail_t(int form, const void* affine_pts, const uint8_t* neg, size_t npts, const uint32_t* ids, const uint32_t* off, size_t nocc, uint32_t NB, uint32_t S,
               void* out_xyzz) {
  using L = typename Cfg::L;
  using Fq = typename Cfg::Fq;
  if (NB < 1 || NB > (1u << 16) || S < 1 || S > (1u << 16) || nocc > NB) return CSH_ERR_INVALID;
  for (size_t i = 0; i < nocc; ++i)
    if (ids[i] < 1 || ids[i] > NB || off[i] > off[i + 1] || off[i + 1] > npts) return CSH_ERR_INVALID;
  std::vector<XYZZLazy<L>> occ(nocc ? nocc : 1);
  build_slots<L, Fq>(reinterpret_cast<const Affine<Fq>*>(affine_pts), neg, off, nocc, occ.data());
  std::vector<XYZZLazy<L>> dense((size_t)NB + 1);
  memset((void*)dense.data(), 0, dense.size() * sizeof(XYZZLazy<L>));
  for (auto& d : dense) d.empty = true;
  for (size_t i = 0; i < nocc; ++i) dense[ids[i]] = occ[i];
  return msm_tail_selftest_t<Cfg>(dense.data(), NB, S, form, out_xyzz);
}

// ---- the bucket stage up to the per-bucket sums --------------------------------------------------------------------------------
// Fused merge form: the two kernels that call qbucket_merged / pbucket_merged once per bucket live in selftest_buckets_dev.hip, a unit
// compiled as the product's are (without the limb-bound instrumentation of this one), so that the functions run in the form
// k_msm_reduce<Cfg, true> and k_msm_reduce_pair<Cfg, true> run them in. out: W * NB lazy points, bucket b of window w at [w * NB + b - 1].
// Plan words, scratch and launches are the product's (msm_buckets_selftest_t, instantiated next to the kernels, runs bucket_sums_launch
// as bucket_group does); this adds the export. merge_form 0: dense[w][1 .. NB] as k_msm_merge and k_msm_merge_giant left it; 1 / 2: the
// two kernels above after k_msm_mark_giant and the giant launches.
template <class Cfg>
int msm_buckets_t(const Bases* B, int acc_form, int merge_form, const MsmParams& in, const uint32_t* start, const uint32_t* sorted, const uint32_t* nlanes,
                  void* out_xyzz, uint32_t* giant_count, uint64_t rec[3]) {
  using L = typename Cfg::L;
  using Fq = typename Cfg::Fq;
  CSH_REQUIRE(acc_form >= 0 && acc_form <= 1 && merge_form >= 0 && merge_form <= 2, "selftest_msm_buckets: unknown form");
  CSH_REQUIRE(Cfg::PAIR || (acc_form == 0 && merge_form != 2), "selftest_msm_buckets: the lane-pair forms exist on the G2 groups only");
  BucketsSelftestRun<Cfg> run;
  CSH_TRY(msm_buckets_selftest_t<Cfg>(B, acc_form, merge_form != 0, &in, start, sorted, nlanes, &run));
  const MsmParams& p = run.p;
  const size_t nout = (size_t)p.W * p.NB;
  DevMem dlazy, dx;
  CSH_TRY(dx.alloc(nout * sizeof(XYZZ<Fq>)));
  CSH_TRY(bound_record_clear());
  if (merge_form == 0) {
    for (int w = 0; w < p.W; ++w)
      hipLaunchKernelGGL((k_st_export<L, Fq>), dim3((p.NB + 127) / 128), dim3(128), 0, 0, run.dense + (size_t)w * (p.NB + 1) + 1, p.NB, dx.as<XYZZ<Fq>>() + (size_t)w * p.NB);
  } else {
    CSH_TRY(dlazy.alloc(nout * sizeof(LazyPt<Cfg>)));
    CSH_TRY(st_bucket_export_launch<Cfg>(merge_form == 2, p, run.start, run.partial, run.dense, dlazy.as<LazyPt<Cfg>>()));
    hipLaunchKernelGGL((k_st_export<L, Fq>), dim3((unsigned)((nout + 127) / 128)), dim3(128), 0, 0, dlazy.as<LazyPt<Cfg>>(), (uint32_t)nout, dx.as<XYZZ<Fq>>());
  }
  CSH_HIP(hipGetLastError());
  CSH_TRY(bound_record_take(rec));
  CSH_HIP(hipMemcpy(out_xyzz, dx.p, nout * sizeof(XYZZ<Fq>), hipMemcpyDeviceToHost));
  giant_count[0] = run.giant_count[0];
  giant_count[1] = run.giant_count[1];
  return CSH_OK;
}

// ---- the sort stage alone -------------------------------------------------------------------------------------------------------
// Plan, scratch and launches are the product's own (msm_plan, msm_sort_bytes, GroupOps::sort = msm_sort_stage<Fr> as msm.hip instantiates
// it: no kernel of the stage gets a second home here); this only uploads the scalars, fills the scratch with 0xFF bytes (the arena of
// a real call is dirty too: nothing may rely on what a buffer held before) and copies the stage's three outputs back.
enum : int {
  SI_C = 0, SI_W, SI_WIDE, SI_NB, SI_L, SI_LN, SI_DIG_G, SI_DIG_WP, SI_REMAP_N, SI_REMAP_STRIDE, SI_REMAP_OFF,  // digit half + remap
  SI_SRT_N, SI_SRT_W, SI_SRT_WIDE,                                                                               // sort half
  SI_PATH,           // 0 single-level, 1 two-level, 2 wide
  SI_REC_BYTES,      // intermediate record of the two-level / wide path: 4 or 8 (0: single-level)
  SI_PER_PARTITION,  // two-level: 1 = level 2 with one block per partition
  SI_WIDE_LB,        // wide: log2 buckets per level-2 partition
  SI_CH, SI_CHUNK_LEN,  // chunks and scalars (wide) / entries (plain) per chunk
  SI_WORDS = 24
};
int msm_sort_selftest(csh_curve_t curve, const uint64_t* scalars, size_t n, int mont, const uint64_t* table, uint32_t* info, uint32_t* start, size_t start_words,
                      uint32_t* nlanes, uint32_t* sorted, size_t sorted_words) {
  const GroupOps* G = group_ops(curve, CSH_G1);
  if (!G) return CSH_ERR_INVALID;
  CSH_REQUIRE(scalars && info, "selftest_msm_sort: NULL argument");
  CSH_REQUIRE(n >= 1 && n <= (size_t(1) << 24), "selftest_msm_sort: n out of range");
  CSH_TRY(ensure_device());  // the planner reads the device's SIMD count
  MsmTable tb{};
  if (table) {
    CSH_REQUIRE(table[0] >= 2 && table[0] <= 22 && table[1] >= 1, "selftest_msm_sort: table window width or rows out of range");
    tb = MsmTable{(int)table[0], 0, (size_t)table[2], (size_t)table[3]};
    CSH_REQUIRE(table[1] <= (uint64_t)windows_for(G->scalar_bits, tb.c), "selftest_msm_sort: more table rows than windows");
    tb.rows = (int)table[1];
    CSH_REQUIRE(table[3] <= table[2] && n <= table[2] - table[3], "selftest_msm_sort: offset + n exceeds the table's stride");
    // entry ids fit 31 bits (bit 31 is the sign), as msm_use_table demands of a handle
    CSH_REQUIRE((uint64_t)tb.stride * tb.rows < (uint64_t(1) << 31) && (uint64_t)n * tb.rows < (uint64_t(1) << 31), "selftest_msm_sort: table ids exceed 31 bits");
  }
  const MsmPlan plan = msm_plan(n, G->scalar_bits, mont ? 1 : 0, 1, table ? &tb : nullptr);
  const MsmParams &p = plan.srt, &pd = plan.dig;
  const bool wide = msm_sort_is_wide(p);
  CSH_REQUIRE(p.c <= 16 || wide, "selftest_msm_sort: windows wider than 16 bits need one table row per window");
  memset(info, 0, SI_WORDS * sizeof(uint32_t));
  info[SI_C] = (uint32_t)pd.c, info[SI_W] = (uint32_t)pd.W, info[SI_WIDE] = (uint32_t)pd.wide, info[SI_NB] = p.NB, info[SI_L] = p.L, info[SI_LN] = p.Ln;
  info[SI_DIG_G] = pd.dig_g, info[SI_DIG_WP] = pd.dig_wp, info[SI_REMAP_N] = p.remap_n, info[SI_REMAP_STRIDE] = p.remap_stride, info[SI_REMAP_OFF] = p.remap_off;
  info[SI_SRT_N] = p.n, info[SI_SRT_W] = (uint32_t)p.W, info[SI_SRT_WIDE] = (uint32_t)p.wide;
  if (wide) {
    const WidePlan wp = msm_wide_plan(p, pd);
    info[SI_PATH] = 2, info[SI_REC_BYTES] = wp.rec4 ? 4 : 8, info[SI_WIDE_LB] = wp.lb, info[SI_CH] = wp.CH, info[SI_CHUNK_LEN] = wp.chunk_tiles * 512;
  } else {
    const SortPath sp = msm_sort_path(p);
    info[SI_PATH] = sp.two_level ? 1 : 0, info[SI_REC_BYTES] = sp.two_level ? (sp.rec4 ? 4 : 8) : 0, info[SI_PER_PARTITION] = sp.per_partition ? 1 : 0;
    info[SI_CH] = p.CH, info[SI_CHUNK_LEN] = p.chunk_len;
  }
  if (!start && !nlanes && !sorted) return CSH_OK;  // the plan only: the caller sizes its buffers from it
  const size_t nstart = ((size_t)p.NB + 2) * p.W, nsorted = (size_t)p.n * p.W;
  CSH_REQUIRE(start && nlanes && sorted && start_words >= nstart && sorted_words >= nsorted, "selftest_msm_sort: output buffers too small");
  DevMem dsc;
  CSH_TRY(dsc.alloc(32 * n));
  CSH_HIP(hipMemcpy(dsc.p, scalars, 32 * n, hipMemcpyHostToDevice));
  hipStream_t st = resolve_stream(nullptr);
  Arena& ar = arena_for(st);
  const size_t bytes = msm_sort_bytes(p, pd);
  CSH_TRY(ar.reserve(bytes));
  CSH_HIP(hipMemset(ar.base, 0xFF, bytes));
  CSH_HIP(hipDeviceSynchronize());  // upload and fill ran on the null stream, the stage runs on the thread's own
  SortOut so{};
  CSH_TRY(G->sort(p, pd, dsc.as<uint64_t>(), st, ar, &so, nullptr));
  CSH_HIP(hipGetLastError());
  CSH_HIP(hipStreamSynchronize(st));
  CSH_HIP(hipMemcpy(start, so.start, nstart * sizeof(uint32_t), hipMemcpyDeviceToHost));
  CSH_HIP(hipMemcpy(nlanes, so.nlanes, (size_t)p.W * sizeof(uint32_t), hipMemcpyDeviceToHost));
  CSH_HIP(hipMemcpy(sorted, so.sorted, nsorted * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return CSH_OK;
}

// ---- the two fused forms a witness map ends with (vec_ops.hip: vec_mul_sub_dev, rep3_local_mul_sub_dev) ----------------------------------
// Host pointers in and out around the product launcher `launch(subtrahend, out, stream)`: no kernel of its own. alias: the subtrahend is
// uploaded into the output buffer and the launcher is handed that buffer for both, as csh_groth16_h_dev does; otherwise the output
// buffer starts as 0xFF bytes (no field element), so an element the kernel skips shows.
template <class Launch>
int fused_form(const uint64_t* subtrahend, uint64_t* out, size_t n, int alias, Launch launch) {
  if (n == 0) return CSH_OK;
  const size_t eb = 32 * n;
  DevMem dsub, dout;
  CSH_TRY(dout.alloc(eb));
  if (alias) {
    CSH_HIP(hipMemcpy(dout.p, subtrahend, eb, hipMemcpyHostToDevice));
  } else {
    CSH_HIP(hipMemset(dout.p, 0xFF, eb));
    if (subtrahend) {
      CSH_TRY(dsub.alloc(eb));
      CSH_HIP(hipMemcpy(dsub.p, subtrahend, eb, hipMemcpyHostToDevice));
    }
  }
  CSH_HIP(hipDeviceSynchronize());  // the fill above ran on the null stream, the launcher runs on the thread's own
  hipStream_t st = resolve_stream(nullptr);
  CSH_TRY(launch(alias ? dout.as<uint64_t>() : dsub.as<uint64_t>(), dout.as<uint64_t>(), st));
  CSH_HIP(hipStreamSynchronize(st));
  CSH_HIP(hipMemcpy(out, dout.p, eb, hipMemcpyDeviceToHost));
  return CSH_OK;
}
int upload_operand(DevMem& d, const uint64_t* host, size_t bytes) {
  CSH_TRY(d.alloc(bytes));
  CSH_HIP(hipMemcpy(d.p, host, bytes, hipMemcpyHostToDevice));
  return CSH_OK;
}

}  // namespace

#define ST_GROUP_DISPATCH(curve, group, CALL)                                                                                                   \
  do {                                                                                                                                          \
    if ((curve) == CSH_BN254 && (group) == CSH_G1) { using Cfg = Bn254G1Cfg; using L = Fq29s; using LP = void; using Fq = Bn254Fq; return CALL; }           \
    if ((curve) == CSH_BN254 && (group) == CSH_G2) { using Cfg = Bn254G2Cfg; using L = Fq29s2; using LP = Bn254G2Cfg::LP; using Fq = Bn254Fq2; return CALL; } \
    if ((curve) == CSH_BLS12_381 && (group) == CSH_G1) { using Cfg = Bls381G1Cfg; using L = Fq28s; using LP = void; using Fq = Bls381Fq; return CALL; }     \
    if ((curve) == CSH_BLS12_381 && (group) == CSH_G2) { using Cfg = Bls381G2Cfg; using L = Fq28s2; using LP = Bls381G2Cfg::LP; using Fq = Bls381Fq2; return CALL; } \
    if ((curve) == CSH_GRUMPKIN && (group) == CSH_G1) { using Cfg = GrumpkinG1Cfg; using L = Fr29s; using LP = void; using Fq = Bn254Fr; return CALL; }      \
    if ((curve) == CSH_BLS12_377 && (group) == CSH_G1) { using Cfg = Bls377G1Cfg; using L = Fq28s377; using LP = void; using Fq = Bls377Fq; return CALL; }  \
    if ((curve) == CSH_BLS12_377 && (group) == CSH_G2) { using Cfg = Bls377G2Cfg; using L = Fq28s377x2; using LP = Bls377G2Cfg::LP; using Fq = Bls377Fq2; return CALL; } \
    return CSH_ERR_INVALID;                                                                                                                     \
  } while (0)

extern "C" {

// type: 0 Fq29s, 1 Fq28s, 2 Fr29s, 3 Fq28s377. rec: violations, largest |limb|, site (must come back non-zero: the operand is 2^(B+2))
int csh_selftest_bound_control_dev(int type, uint64_t rec[3]) {
  CSH_TRY(ensure_device());
  switch (type) {
    case 0: return bound_control_t<Fq29s>(rec);
    case 1: return bound_control_t<Fq28s>(rec);
    case 2: return bound_control_t<Fr29s>(rec);
    case 3: return bound_control_t<Fq28s377>(rec);
    default: return CSH_ERR_INVALID;
  }
}

int csh_selftest_fp2pair_raw_dev(int curve, int op, const int32_t* limbs, size_t npairs, uint64_t* out, uint64_t rec[3]) {
  CSH_TRY(ensure_device());
  if (op < 0 || op > 3 || !npairs || npairs > (1u << 20)) return CSH_ERR_INVALID;
  if (curve == CSH_BN254) return fp2pair_raw_t<Bn254G2Cfg::LP, Bn254Fq>(op, limbs, npairs, out, rec);
  if (curve == CSH_BLS12_381) return fp2pair_raw_t<Bls381G2Cfg::LP, Bls381Fq>(op, limbs, npairs, out, rec);
  if (curve == CSH_BLS12_377) return fp2pair_raw_t<Bls377G2Cfg::LP, Bls377Fq>(op, limbs, npairs, out, rec);
  return CSH_ERR_INVALID;
}

int csh_selftest_fp2pair_zero_dev(int curve, const int32_t* limbs, size_t npairs, uint8_t* flags, uint64_t rec[3]) {
  CSH_TRY(ensure_device());
  if (!npairs || npairs > (1u << 20)) return CSH_ERR_INVALID;
  if (curve == CSH_BN254) return fp2pair_zero_t<Bn254G2Cfg::LP>(limbs, npairs, flags, rec);
  if (curve == CSH_BLS12_381) return fp2pair_zero_t<Bls381G2Cfg::LP>(limbs, npairs, flags, rec);
  if (curve == CSH_BLS12_377) return fp2pair_zero_t<Bls377G2Cfg::LP>(limbs, npairs, flags, rec);
  return CSH_ERR_INVALID;
}

// Scripted point operations (see StOp): out_xyzz = 2 * nunits XYZZ points (r0, r1 of every unit) in arkworks words.
int csh_selftest_point_ops_dev(int curve, int group, int form, const void* affine_pts, const uint8_t* neg, size_t npts, const uint32_t* slot_off, size_t nslots,
                               const uint32_t* ops, const uint32_t* unit_off, size_t nunits, void* out_xyzz, uint64_t rec[3]) {
  CSH_TRY(ensure_device());
  ST_GROUP_DISPATCH(curve, group, (point_ops_t<L, LP, Fq>(form, affine_pts, neg, npts, slot_off, nslots, ops, unit_off, nunits, out_xyzz, rec)));
}

// The real window reduction (form 0: k_msm_reduce_serial, 1: k_msm_reduce<Cfg, false>, 2: k_msm_reduce_pair<Cfg, false>) and the real
// k_msm_fold_tree levels on one window of NB buckets in S segments; out_xyzz = the window sum, one XYZZ point in arkworks words.
int csh_selftest_msm_tail_dev(int curve, int group, int form, const void* affine_pts, const uint8_t* neg, size_t npts, const uint32_t* bucket_ids,
                              const uint32_t* bucket_off, size_t nocc, uint32_t NB, uint32_t S, void* out_xyzz) {
  CSH_TRY(ensure_device());
  ST_GROUP_DISPATCH(curve, group, (msm_tail_t<Cfg>(form, affine_pts, neg, npts, bucket_ids, bucket_off, nocc, NB, S, out_xyzz)));
}

// The bucket stage up to the per-bucket sums, through the launches bucket_group itself runs (msm_impl.hpp bucket_sums_launch): accumulate
// (acc_form 0: whole points per lane, 1: a lane pair, G2 only), then k_msm_merge (merge_form 0) or k_msm_mark_giant (1: the bucket sums
// then come from qbucket_merged, 2: from pbucket_merged, G2 only), then k_msm_giant_slices and k_msm_merge_giant. bases: a handle of
// csh_bases_upload. start = [W][NB + 2] and sorted = [W][n] host words as the sort stage leaves them (tests/msm_sort_ref.py); nlanes:
// NULL, or [W] words that must equal what the hook computes. W 1 .. 4, lane lengths L and Ln (L or 2 L; windows from `wide` on take Ln).
// CSH_ERR_INVALID, before any launch, unless start[0] == start[1] == 0, start is monotone, start[NB + 1] <= n and every id (bit 31 =
// the sign) is below the handle's length. out_xyzz: bucket b of window w at [w * NB + b - 1], XYZZ points in arkworks words;
// giant_count: queued buckets, sliced buckets.
int csh_selftest_msm_buckets_dev(csh_bases_t bases, int acc_form, int merge_form, int W, uint32_t NB, uint32_t n, uint32_t L, uint32_t Ln, int wide,
                                 const uint32_t* start, const uint32_t* sorted, const uint32_t* nlanes, void* out_xyzz, uint32_t* giant_count, uint64_t rec[3]) {
  CSH_REQUIRE(bases && start && sorted && out_xyzz && giant_count && rec, "selftest_msm_buckets: NULL argument");
  CSH_TRY(ensure_device());
  const Bases* B = reinterpret_cast<const Bases*>(bases);
  MsmParams in{};
  in.W = W, in.NB = NB, in.n = n, in.L = L, in.Ln = Ln, in.wide = wide;
  ST_GROUP_DISPATCH(B->curve, B->group, (msm_buckets_t<Cfg>(B, acc_form, merge_form, in, start, sorted, nlanes, out_xyzz, giant_count, rec)));
}

// The MSM sort stage alone (digits -> counting sort; plain single-level, plain two-level or wide, as msm_plan and the tune knobs decide)
// on n >= 1 host scalars of the curve's scalar field (BN254 Fr, BLS12-381 Fr, Grumpkin = BN254 Fq, BLS12-377 Fr). table: NULL, or
// {c, rows, stride, offset} of fixed-base tables as in MsmTable. info: 24 words, the plan that ran (SI_* above). With start, nlanes and
// sorted all NULL only info is filled; otherwise start = [W'][NB + 2], nlanes = [W'], sorted = [W'][n'] words (W' = info[SI_SRT_W],
// n' = info[SI_SRT_N]) as the bucket stage would read them.
int csh_selftest_msm_sort_dev(int curve, const uint64_t* scalars, size_t n, int mont, const uint64_t* table, uint32_t* info, uint32_t* start, size_t start_words,
                              uint32_t* nlanes, uint32_t* sorted, size_t sorted_words) {
  return msm_sort_selftest((csh_curve_t)curve, scalars, n, mont, table, info, start, start_words, nlanes, sorted, sorted_words);
}

// out = a * b - c through csh::vec_mul_sub_dev (k_vec_mul_sub), n elements, host pointers. c_aliases_out: c travels in the output buffer.
int csh_selftest_vec_mul_sub_dev(int curve, const uint64_t* a, const uint64_t* b, const uint64_t* c, uint64_t* out, size_t n, int c_aliases_out) {
  CSH_REQUIRE((a && b && c && out) || n == 0, "selftest_vec_mul_sub: NULL argument");
  CSH_TRY(ensure_device());
  DevMem da, db;
  if (n) {
    CSH_TRY(upload_operand(da, a, 32 * n));
    CSH_TRY(upload_operand(db, b, 32 * n));
  }
  return fused_form(c, out, n, c_aliases_out, [&](const uint64_t* dc, uint64_t* dout, hipStream_t st) {
    return vec_mul_sub_dev((csh_curve_t)curve, da.as<uint64_t>(), db.as<uint64_t>(), dc, dout, n, st);
  });
}

// out = rep3_local_mul(lhs, rhs) + mask - sub through csh::rep3_local_mul_sub_dev (k_rep3_local_mul), n shares {a, b} per side, host
// pointers. mask and sub may be NULL (the kernel takes either as absent); sub_aliases_out: sub travels in the output buffer.
int csh_selftest_rep3_local_mul_sub_dev(int curve, const uint64_t* lhs, const uint64_t* rhs, const uint64_t* mask, const uint64_t* sub, uint64_t* out, size_t n,
                                        int sub_aliases_out) {
  CSH_REQUIRE((lhs && rhs && out) || n == 0, "selftest_rep3_local_mul_sub: NULL argument");
  CSH_REQUIRE(sub || !sub_aliases_out, "selftest_rep3_local_mul_sub: no sub operand to put into the output buffer");
  CSH_TRY(ensure_device());
  DevMem dl, dr, dm;
  if (n) {
    CSH_TRY(upload_operand(dl, lhs, 64 * n));
    CSH_TRY(upload_operand(dr, rhs, 64 * n));
    if (mask) CSH_TRY(upload_operand(dm, mask, 32 * n));
  }
  return fused_form(sub, out, n, sub_aliases_out, [&](const uint64_t* ds, uint64_t* dout, hipStream_t st) {
    return rep3_local_mul_sub_dev((csh_curve_t)curve, dl.as<uint64_t>(), dr.as<uint64_t>(), dm.as<uint64_t>(), ds, dout, n, st);
  });
}

}  // extern "C"
