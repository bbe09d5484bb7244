// Device self-test hooks of the NTT: the lazy pass kernels of ntt_kernels.hpp -- radix-2, radix-4 and the fused pair, both directions,
// three scalar fields -- instantiated a second time with the device form of the limb-bound contract (field29.hpp,
// CSH_CHECK_BOUNDS_DEVICE: every product checks its operands' limbs, fold_top() its quotient estimate; a violation is counted in this
// unit's record, never trapped) and run through the product's own planning, tables and launch code (ntt_run_with_kernels). Each entry
// returns the transformed data and hands the record back, cleared. The 32-bit pass has no contract and no copy here. No CSH_PIN_MADS
// in this unit: the pin changes the order of a column's multiply-adds, not a value. Test infrastructure; not declared in
// include/cosnarks_hip.h.
#define CSH_CHECK_BOUNDS_DEVICE 1
#define CSH_BOUND_RECORD g_bound_record_ntt  // selftest_dev.hip owns g_bound_record
#define CSH_NTT_KERNEL_NS ntt_checked
#include "fr_entry.hpp"
#include "ntt_kernels.hpp"

using namespace csh;

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
};

int bound_record_clear() {
  const unsigned long long z[2] = {0, 0};
  CSH_HIP(hipMemcpyToSymbol(HIP_SYMBOL(CSH_BOUND_RECORD), z, sizeof z));
  return CSH_OK;
}
// rec[0] = violations, rec[1] = largest |limb| (or |scalar|), rec[2] = its site (line of field29.hpp); the device record is cleared
int bound_record_take(uint64_t rec[3]) {
  unsigned long long r[2];
  CSH_HIP(hipDeviceSynchronize());
  CSH_HIP(hipMemcpyFromSymbol(r, HIP_SYMBOL(CSH_BOUND_RECORD), sizeof r));
  rec[0] = r[0];
  rec[1] = r[1] >> 16;
  rec[2] = r[1] & 0xffff;
  return bound_record_clear();
}

template <class F>
const void* checked_kernels(PassForm form, bool dif) {
  using LZ = typename LazyOf<F>::type;
  switch (form) {
    case PassForm::Plain32: return nullptr;
    case PassForm::LazyR2: return dif ? (const void*)k_ntt_pass_lazy<F, LZ, true> : (const void*)k_ntt_pass_lazy<F, LZ, false>;
    case PassForm::LazyR4: return dif ? (const void*)k_ntt_pass_r4<F, LZ, true> : (const void*)k_ntt_pass_r4<F, LZ, false>;
    case PassForm::LazyPair: return (const void*)k_ntt_pass_r4<F, LZ, true, true>;
  }
  return nullptr;
}
NttKernelTable checked_table(csh_curve_t curve) {
  NttKernelTable t = nullptr;
  (void)with_fr(curve, [&](auto fr) -> int {
    t = checked_kernels<typename decltype(fr)::type>;
    return CSH_OK;
  });
  return t;
}

// positive control of this unit's recorder and of fold_top()'s site: the value R' = 2^(NL B) (top limb 2^B, the rest zero) asks for the
// quotient R' / p (about 170, 70, 440 for the three scalar fields), outside the documented |k| <= 64 -- integer arithmetic on a chosen
// input, one lane
template <class LZ>
__global__ void k_st_fold_control(int32_t* sink) {
  LZ a;
  for (int i = 0; i < LZ::NL; ++i) a.l[i] = 0;
  a.l[LZ::NL - 1] = (int32_t)(1u << LZ::B);
  const LZ r = a.fold_top();
  sink[0] = r.l[LZ::NL - 1];
}

int run_checked(csh_domain_t dom, bool pair, bool dif, const uint64_t* shift, uint64_t* data_host, uint32_t ncomp, uint64_t rec[3]) {
  CSH_REQUIRE(dom && data_host && rec, "NULL argument");
  FR_REQUIRE_NCOMP(ncomp);
  CSH_TRY(ensure_device());
  const Domain* d = reinterpret_cast<const Domain*>(dom);
  const NttKernelTable table = checked_table(domain_curve_of(d));
  if (!table) return CSH_ERR_INVALID;
  const size_t n = domain_size_of(d), bytes = n * ncomp * 32;
  hipStream_t st = resolve_stream(nullptr);
  DevMem data, scale;
  CSH_TRY(data.alloc(bytes));
  CSH_HIP(hipMemcpy(data.p, data_host, bytes, hipMemcpyHostToDevice));
  if (pair) {
    CSH_REQUIRE(shift, "shift is NULL");
    CSH_REQUIRE(ntt_scale_table_supported(d), "the fused pair needs the lazy passes and a domain of at least 2 points");
    CSH_TRY(scale.alloc(n * 32));
    CSH_TRY(ntt_coset_table_scaled(d, shift, static_cast<uint64_t*>(scale.p), st));
  }
  CSH_TRY(bound_record_clear());
  CSH_TRY(ntt_run_with_kernels(d, static_cast<uint64_t*>(data.p), ncomp, pair, dif, static_cast<const uint64_t*>(scale.p), table, st));
  CSH_TRY(bound_record_take(rec));
  CSH_HIP(hipMemcpy(data_host, data.p, bytes, hipMemcpyDeviceToHost));
  return CSH_OK;
}

}  // namespace

extern "C" {

// which: 0 = ifft_in_to_out, 1 = fft_out_to_in, in place on data_host (n x ncomp elements), under the tune knobs in force
int csh_selftest_ntt_dev(csh_domain_t dom, int which, uint64_t* data_host, uint32_t ncomp, uint64_t rec[3]) {
  CSH_REQUIRE(which == 0 || which == 1, "which: 0 = ifft_in_to_out, 1 = fft_out_to_in");
  return run_checked(dom, false, which == 0, nullptr, data_host, ncomp, rec);
}

// ifft_in_to_out, the coset table of `shift`, fft_out_to_in -- one vector of a witness map -- with the tile passes fused where the plan allows
int csh_selftest_ntt_pair_dev(csh_domain_t dom, const uint64_t shift[4], uint64_t* data_host, uint32_t ncomp, uint64_t rec[3]) {
  return run_checked(dom, true, true, shift, data_host, ncomp, rec);
}

int csh_selftest_ntt_bound_control_dev(csh_curve_t field_of, uint64_t rec[3]) {
  CSH_REQUIRE(rec, "rec is NULL");
  CSH_TRY(ensure_device());
  DevMem sink;
  CSH_TRY(sink.alloc(sizeof(int32_t)));
  CSH_TRY(bound_record_clear());
  CSH_TRY(with_fr(field_of, [&](auto fr) -> int {
    using LZ = LzOf<typename decltype(fr)::type>;
    hipLaunchKernelGGL(k_st_fold_control<LZ>, dim3(1), dim3(1), 0, 0, static_cast<int32_t*>(sink.p));
    CSH_HIP(hipGetLastError());
    return CSH_OK;
  }));
  return bound_record_take(rec);
}

}  // extern "C"
