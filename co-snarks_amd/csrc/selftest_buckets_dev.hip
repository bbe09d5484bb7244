// The two export kernels of csh_selftest_msm_buckets_dev (selftest_dev.hip) for the fused merge form: what the fused reductions see as
// bucket b of window w -- qbucket_merged (k_msm_reduce<Cfg, true>), one quad per bucket, or pbucket_merged (k_msm_reduce_pair<Cfg, true>),
// one lane pair per bucket -- stored as a lazy point in out[w * NB + b - 1]. A unit of its own, compiled exactly as the product's units
// are (no CSH_CHECK_BOUNDS_DEVICE, the flags of msm_inst_*.hip): the two functions are inlined into their callers, so what is tested is
// their register-resident form, the one k_msm_reduce runs, and not the instrumented one of selftest_dev.hip (the paragraph
// on the device unit tests of the bucket stage, says what that build did to qbucket_merged on BLS12-377 G2). Test infrastructure.
#include "msm_impl.hpp"

namespace csh {

template <class Cfg>
__global__ __launch_bounds__(256) void k_st_bucket_quad(MsmParams p, const uint32_t* __restrict__ start, const LazyPt<Cfg>* __restrict__ partial,
                                                        const LazyPt<Cfg>* __restrict__ dense, LazyPt<Cfg>* out) {
  using L = typename Cfg::L;
  const int w = blockIdx.y, role = threadIdx.x & 3;
  const uint32_t b = blockIdx.x * 64 + (threadIdx.x >> 2) + 1;
  if (b > p.NB) return;  // quad-uniform
  const QPt<L> v = qbucket_merged<Cfg>(lane_len(p, w), start + (size_t)w * (p.NB + 2), partial + (size_t)w * p.tmax, dense + (size_t)w * (p.NB + 1), b, role);
  qpt_store<L>(&out[(size_t)w * p.NB + b - 1], role, v);
}
template <class Cfg>
__global__ __launch_bounds__(256) void k_st_bucket_pair(MsmParams p, const uint32_t* __restrict__ start, const LazyPt<Cfg>* __restrict__ partial,
                                                        const LazyPt<Cfg>* __restrict__ dense, LazyPt<Cfg>* out) {
  const int w = blockIdx.y, role = pair_role();
  const uint32_t b = blockIdx.x * 128 + (threadIdx.x >> 1) + 1;
  if (b > p.NB) return;  // pair-uniform
  const XYZZLazy<typename Cfg::LP> v =
      pbucket_merged<Cfg>(lane_len(p, w), start + (size_t)w * (p.NB + 2), partial + (size_t)w * p.tmax, dense + (size_t)w * (p.NB + 1), b, role);
  pair_store(&out[(size_t)w * p.NB + b - 1], role, v);
}

// out: W * NB lazy points on the device. pair: pbucket_merged (the G2 groups only), else qbucket_merged. Declared in selftest_dev.hip.
template <class Cfg>
int st_bucket_export_launch(bool pair, const MsmParams& p, const uint32_t* start, const LazyPt<Cfg>* partial, const LazyPt<Cfg>* dense, LazyPt<Cfg>* out) {
  if (pair) {
    if constexpr (Cfg::PAIR)
      hipLaunchKernelGGL(k_st_bucket_pair<Cfg>, dim3((p.NB + 127) / 128, p.W), dim3(256), 0, 0, p, start, partial, dense, out);
    else
      return CSH_ERR_INVALID;
  } else {
    hipLaunchKernelGGL(k_st_bucket_quad<Cfg>, dim3((p.NB + 63) / 64, p.W), dim3(256), 0, 0, p, start, partial, dense, out);
  }
  CSH_HIP(hipGetLastError());
  return CSH_OK;
}

#define CSH_ST_BUCKET_EXPORT(CFG) \
  template int st_bucket_export_launch<CFG>(bool, const MsmParams&, const uint32_t*, const LazyPt<CFG>*, const LazyPt<CFG>*, LazyPt<CFG>*);
CSH_ST_BUCKET_EXPORT(Bn254G1Cfg)
CSH_ST_BUCKET_EXPORT(Bn254G2Cfg)
CSH_ST_BUCKET_EXPORT(Bls381G1Cfg)
CSH_ST_BUCKET_EXPORT(Bls381G2Cfg)
CSH_ST_BUCKET_EXPORT(GrumpkinG1Cfg)
CSH_ST_BUCKET_EXPORT(Bls377G1Cfg)
CSH_ST_BUCKET_EXPORT(Bls377G2Cfg)

}  // namespace csh
