// Rounds 2 and 5 of the circom PLONK prover between their network rounds: the operands of Round2::compute_z
// (co-circom/co-plonk/src/round2.rs:104-155), buffer_z.rotate_right(1) (:171), blind_coefficients (co-plonk/src/lib.rs:162-177) and the
// ragged linear combination of shared and public polynomials under public coefficients that is Round5::compute_r + compute_wxi
// (round5.rs:118-259). Affine in the shares: no network round, HBM-bound streaming kernels of the plonk_quot.hip kind -- grid-stride over
// flat value indices, 256 lanes, no LDS, tune "vec_max_blocks". Expressions, index algebra and bounds: plonk_rounds.hpp, shared with the
// host self-test. The powers of w = w_ext^4 come from the two-level table of plonk_quot.hpp, built on the device per call.
#include "plonk_rounds.hpp"

namespace csh {

template <class F>
__global__ __launch_bounds__(PQ_WG) void k_pr_z_num(PrZArgs<F> a) {
  for (size_t e = blockIdx.x * (size_t)PQ_WG + threadIdx.x; e < a.g.values(); e += (size_t)gridDim.x * PQ_WG) pr_z_num_at(a, e);
}
template <class F>
__global__ __launch_bounds__(PQ_WG) void k_pr_z_den(PrZArgs<F> a) {
  for (size_t e = blockIdx.x * (size_t)PQ_WG + threadIdx.x; e < a.g.values(); e += (size_t)gridDim.x * PQ_WG) pr_z_den_at(a, e);
}
template <class F>
__global__ __launch_bounds__(PQ_WG) void k_pr_rotate(PrRotArgs<F> a) {
  const size_t nv = a.n * a.ncomp;
  for (size_t e = blockIdx.x * (size_t)PQ_WG + threadIdx.x; e < nv; e += (size_t)gridDim.x * PQ_WG) pr_rotate_at(a, e);
}
template <class F>
__global__ __launch_bounds__(64) void k_pr_blind(PrBlindArgs<F> a) {
  if (threadIdx.x < a.k * a.ncomp) pr_blind_at(a, threadIdx.x);
}
template <class F>
__global__ __launch_bounds__(PQ_WG) void k_pr_lincomb(PrLcArgs<F> a) {
  for (size_t e = blockIdx.x * (size_t)PQ_WG + threadIdx.x; e < a.g.values(); e += (size_t)gridDim.x * PQ_WG) pr_lc_at(a, e);
}

template <class F>
static int z_operands_t(const Domain* d, uint32_t protocol, uint32_t party, const uint64_t* const* sh, const uint64_t* const* sigma,
                        const uint64_t* ch, uint64_t* const* out, hipStream_t st) {
  PrZArgs<F> a;
  const size_t n = domain_size_of(d) / 4;
  a.g = PqGeom{n, protocol + 1, pq_pub_comp(protocol, party)};
  for (int v = 0; v < 3; ++v) a.in[v] = (const F*)sh[v], a.sigma[v] = (const F*)sigma[v];
  for (int v = 0; v < 6; ++v) a.out[v] = (F*)out[v];
  pr_z_consts(a, ch);
  CSH_TRY(pq_power_tables<F>(F::pow_u64(fr_load<F>(domain_gen_of(d)), 4), n, st, &a.hi, &a.lo));
  const dim3 grid(fr_stream_grid(a.g.values(), PQ_WG)), wg(PQ_WG);
  hipLaunchKernelGGL(k_pr_z_num<F>, grid, wg, 0, st, a);
  hipLaunchKernelGGL(k_pr_z_den<F>, grid, wg, 0, st, a);
  CSH_HIP(hipGetLastError());
  return CSH_OK;
}

template <class F>
static int rotate_t(const uint64_t* in, uint64_t* out, size_t n, uint32_t ncomp, size_t k, hipStream_t st) {
  PrRotArgs<F> a{(const F*)in, (F*)out, n, k, ncomp};
  hipLaunchKernelGGL(k_pr_rotate<F>, dim3(fr_stream_grid(n * ncomp, PQ_WG)), dim3(PQ_WG), 0, st, a);
  CSH_HIP(hipGetLastError());
  return CSH_OK;
}

template <class F>
static int blind_t(uint64_t* poly, size_t n, uint32_t ncomp, const uint64_t* coeff_rev, uint32_t k, hipStream_t st) {
  PrBlindArgs<F> a;
  a.poly = (F*)poly;
  a.n = n, a.ncomp = ncomp, a.k = k;
  pr_blind_consts(a, coeff_rev, ncomp, k);
  hipLaunchKernelGGL(k_pr_blind<F>, dim3(1), dim3(64), 0, st, a);
  CSH_HIP(hipGetLastError());
  return CSH_OK;
}

template <class F>
static int lincomb_t(uint32_t protocol, uint32_t party, const uint64_t* const* shares, const size_t* share_lens, const uint64_t* share_coeffs,
                     size_t ks, const uint64_t* const* pub, const size_t* public_lens, const uint64_t* public_coeffs, size_t kp,
                     const uint64_t* const0, uint64_t* out, size_t out_len, hipStream_t st) {
  const auto launches = pr_lc_launches<F>(protocol, party, shares, share_lens, share_coeffs, ks, pub, public_lens, public_coeffs, kp, const0, out, out_len);
  for (const PrLcArgs<F>& a : launches)
    hipLaunchKernelGGL(k_pr_lincomb<F>, dim3(fr_stream_grid(a.g.values(), PQ_WG)), dim3(PQ_WG), 0, st, a);
  CSH_HIP(hipGetLastError());
  return CSH_OK;
}

}  // namespace csh

using namespace csh;

static int pr_check_party(uint32_t protocol, uint32_t party, const char* what) {
  if (protocol > 1 || party > 2) {
    set_error("%s: protocol must be 0 (plain / Shamir) or 1 (Rep3), party_id 0, 1 or 2", what);
    return CSH_ERR_INVALID;
  }
  return CSH_OK;
}

extern "C" {

int csh_plonk_z_operands_dev(csh_domain_t ext_dom, uint32_t protocol, uint32_t party_id, const uint64_t* const* shares_dev,
                             const uint64_t* const* sigma_dev, const uint64_t* challenges, uint64_t* const* out_dev, void* stream) {
  const char* what = "plonk_z_operands";
  CSH_TRY(pr_check_party(protocol, party_id, what));
  CSH_REQUIRE(ext_dom && shares_dev && sigma_dev && challenges && out_dev, "plonk_z_operands: NULL argument");
  CSH_TRY(fr_require_ptrs((const void* const*)shares_dev, 3, what));
  CSH_TRY(fr_require_ptrs((const void* const*)sigma_dev, 3, what));
  CSH_TRY(fr_require_ptrs((const void* const*)out_dev, 6, what));
  CSH_TRY(ensure_device());
  // a domain handle exists only in a process that has a device, so it is looked into after ensure_device() and before any launch
  const Domain* d = reinterpret_cast<const Domain*>(ext_dom);
  const size_t N = domain_size_of(d);
  if (N < 32 || N > FR_MAX_N) {
    set_error("%s: the extended domain must have 32 .. 2^28 points (n >= 8)", what);
    return CSH_ERR_INVALID;
  }
  int cur = -1;
  if (hipGetDevice(&cur) == hipSuccess && cur != domain_device_of(d)) {
    set_error("%s: the domain lives on device %d but the calling thread is bound to device %d (csh_init)", what, domain_device_of(d), cur);
    return CSH_ERR_INVALID;
  }
  const size_t sb = 32 * (N / 4) * (protocol + 1);
  FrRanges in, out;
  in.add((const void* const*)shares_dev, 3, sb);
  in.add((const void* const*)sigma_dev, 3, 32 * N);
  out.add((const void* const*)out_dev, 6, sb);
  CSH_TRY(fr_check_ranges(in, out, what));
  hipStream_t st = resolve_stream(stream);
  return FR_CALL(domain_curve_of(d), z_operands_t<F>(d, protocol, party_id, shares_dev, sigma_dev, challenges, out_dev, st));
}

int csh_vec_rotate_right_dev(csh_curve_t field_of, const uint64_t* in_dev, uint64_t* out_dev, size_t n, uint32_t ncomp, size_t k, void* stream) {
  const char* what = "vec_rotate_right";
  FR_REQUIRE_FIELD(field_of);
  FR_REQUIRE_NCOMP(ncomp);
  FR_REQUIRE_N(n);
  if (n == 0) return CSH_OK;
  CSH_REQUIRE(in_dev && out_dev, "vec_rotate_right: NULL argument");
  CSH_REQUIRE(k < n, "vec_rotate_right: k must be below n");
  FrRanges in, out;
  in.add(in_dev, 32 * n * ncomp), out.add(out_dev, 32 * n * ncomp);
  CSH_TRY(fr_check_ranges(in, out, what));
  CSH_TRY(ensure_device());
  hipStream_t st = resolve_stream(stream);
  return FR_CALL(field_of, rotate_t<F>(in_dev, out_dev, n, ncomp, k, st));
}

int csh_plonk_blind_coefficients_dev(csh_curve_t field_of, uint64_t* poly_dev, size_t n, uint32_t ncomp, const uint64_t* coeff_rev, size_t k,
                                     void* stream) {
  FR_REQUIRE_FIELD(field_of);
  FR_REQUIRE_NCOMP(ncomp);
  FR_REQUIRE_N(n);
  CSH_REQUIRE(poly_dev && coeff_rev, "plonk_blind_coefficients: NULL argument");
  CSH_REQUIRE(k >= 1 && k <= 3 && n >= 3, "plonk_blind_coefficients: 1 <= k <= 3 <= n");
  CSH_TRY(ensure_device());
  hipStream_t st = resolve_stream(stream);
  return FR_CALL(field_of, blind_t<F>(poly_dev, n, ncomp, coeff_rev, (uint32_t)k, st));
}

int csh_poly_lincomb_dev(csh_curve_t field_of, uint32_t protocol, uint32_t party_id, const uint64_t* const* shares_dev, const size_t* share_lens,
                         const uint64_t* share_coeffs, size_t ks, const uint64_t* const* public_dev, const size_t* public_lens,
                         const uint64_t* public_coeffs, size_t kp, const uint64_t* const0, uint64_t* out_dev, size_t out_len, void* stream) {
  const char* what = "poly_lincomb";
  FR_REQUIRE_FIELD(field_of);
  CSH_TRY(pr_check_party(protocol, party_id, what));
  CSH_REQUIRE(ks <= PR_LC_MAX_TERMS && kp <= PR_LC_MAX_TERMS && ks + kp >= 1, "poly_lincomb: ks and kp must be at most 64, and ks + kp at least 1");
  CSH_REQUIRE(out_dev && (!ks || (shares_dev && share_lens && share_coeffs)) && (!kp || (public_dev && public_lens && public_coeffs)),
              "poly_lincomb: NULL argument");
  FR_REQUIRE_N(out_len);
  const size_t ncomp = protocol + 1;
  FrRanges in, out;
  for (size_t j = 0; j < ks + kp; ++j) {
    const bool s = j < ks;
    const size_t len = s ? share_lens[j] : public_lens[j - ks];
    const uint64_t* p = s ? shares_dev[j] : public_dev[j - ks];
    CSH_REQUIRE(len <= out_len, "poly_lincomb: a length exceeds out_len");
    CSH_REQUIRE(p || !len, "poly_lincomb: NULL argument");
    if (len) in.add(p, 32 * len * (s ? ncomp : 1));
  }
  if (out_len == 0) return CSH_OK;
  out.add(out_dev, 32 * out_len * ncomp);
  CSH_TRY(fr_check_ranges(in, out, what));
  CSH_TRY(ensure_device());
  hipStream_t st = resolve_stream(stream);
  return FR_CALL(field_of, lincomb_t<F>(protocol, party_id, shares_dev, share_lens, share_coeffs, ks, public_dev, public_lens, public_coeffs, kp,
                                        const0, out_dev, out_len, st));
}

}  // extern "C"
