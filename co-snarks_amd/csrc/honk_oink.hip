// The Oink phase of co-noir's UltraHonk prover between its commitments and the scans, all of
// co-noir/co-ultrahonk/src/co_oink/co_oink_prover.rs: the memory records added to w_4 (:98-160), the operands of the log-derivative lookup
// inverses (:162-293), the operands of the permutation grand product gathered through the active ranges (:344-451) and the placement of
// z_perm (:472-504). Affine in the shares: no network round, HBM-bound streaming kernels of the plonk_rounds.hip kind -- grid-stride over
// flat value indices, 256 lanes, no LDS, tune "vec_max_blocks". Expressions, index algebra and bounds: honk_oink.hpp, shared with the host
// self-test. The active ranges travel as kernel arguments with their prefix counts; no index list is built, uploaded or read.
#include "honk_oink.hpp"

namespace csh {

template <class F>
__global__ __launch_bounds__(PQ_WG) void k_ho_w4(HoW4Args<F> a) {
  for (size_t e = blockIdx.x * (size_t)PQ_WG + threadIdx.x; e < a.g.values(); e += (size_t)gridDim.x * PQ_WG) ho_w4_at(a, e);
}
template <class F>
__global__ __launch_bounds__(PQ_WG) void k_ho_lookup_prod(HoLookupArgs<F> a) {
  for (size_t e = blockIdx.x * (size_t)PQ_WG + threadIdx.x; e < a.g.values(); e += (size_t)gridDim.x * PQ_WG) ho_lookup_prod_at(a, e);
}
template <class F>
__global__ __launch_bounds__(PQ_WG) void k_ho_lookup_sel(HoSelArgs<F> a) {
  for (size_t e = blockIdx.x * (size_t)PQ_WG + threadIdx.x; e < a.g.values(); e += (size_t)gridDim.x * PQ_WG) ho_lookup_sel_at(a, e);
}
template <class F>
__global__ __launch_bounds__(PQ_WG) void k_ho_perm(HoPermArgs<F> a) {
  for (size_t e = blockIdx.x * (size_t)PQ_WG + threadIdx.x; e < a.g.values(); e += (size_t)gridDim.x * PQ_WG) ho_perm_at(a, e);
}
template <class F>
__global__ __launch_bounds__(PQ_WG) void k_ho_place(HoPlaceArgs<F> a) {
  for (size_t e = blockIdx.x * (size_t)PQ_WG + threadIdx.x; e < a.g.values(); e += (size_t)gridDim.x * PQ_WG) ho_place_at(a, e);
}

template <class F>
static int w4_records_t(uint32_t protocol, uint32_t party, const uint64_t* const* w, uint64_t* w4, size_t n, const uint64_t* etas,
                        const uint32_t* read_idx, size_t n_read, const uint32_t* write_idx, size_t n_write, const uint32_t* shared_idx,
                        const uint64_t* type_share, size_t n_shared, hipStream_t st) {
  HoW4Args<F> a;
  for (int k = 0; k < 3; ++k) a.w[k] = (const F*)w[k];
  a.w4 = (F*)w4;
  a.read_idx = read_idx, a.write_idx = write_idx, a.shared_idx = shared_idx;
  a.type_share = (const F*)type_share;
  a.n = n, a.n_read = (uint32_t)n_read, a.n_write = (uint32_t)n_write, a.n_shared = (uint32_t)n_shared;
  ho_w4_consts(a, etas);
  a.g = PqGeom{n_read + n_write + n_shared, protocol + 1, pq_pub_comp(protocol, party)};
  hipLaunchKernelGGL(k_ho_w4<F>, dim3(fr_stream_grid(a.g.values(), PQ_WG)), dim3(PQ_WG), 0, st, a);
  CSH_HIP(hipGetLastError());
  return CSH_OK;
}

template <class F>
static int lookup_operands_t(uint32_t protocol, uint32_t party, const uint64_t* const* sh, const uint64_t* const* pub, size_t n,
                             const uint64_t* ch, uint64_t* const* out, hipStream_t st) {
  HoLookupArgs<F> a;
  HoSelArgs<F> s;
  a.g = s.g = PqGeom{n, protocol + 1, pq_pub_comp(protocol, party)};
  for (int k = 0; k < 3; ++k) a.w[k] = (const F*)sh[k], a.q[k] = (const F*)pub[k];
  a.qo = (const F*)pub[3];
  for (int k = 0; k < 4; ++k) a.tab[k] = (const F*)pub[4 + k];
  a.prod = (F*)out[0];
  ho_lookup_consts(a, ch);
  s.tag = (const F*)sh[3], s.qlookup = (const F*)pub[8], s.sel = (F*)out[1], s.one = F::one();
  const dim3 grid(fr_stream_grid(a.g.values(), PQ_WG)), wg(PQ_WG);
  hipLaunchKernelGGL(k_ho_lookup_prod<F>, grid, wg, 0, st, a);
  hipLaunchKernelGGL(k_ho_lookup_sel<F>, grid, wg, 0, st, s);
  CSH_HIP(hipGetLastError());
  return CSH_OK;
}

template <class F>
static int perm_operands_t(uint32_t protocol, uint32_t party, const uint64_t* const* sh, const uint64_t* const* pub, const HoRanges& R,
                           const uint64_t* ch, uint64_t* const* out, hipStream_t st) {
  HoPermArgs<F> a;
  a.g = PqGeom{(size_t)R.active - 1, protocol + 1, pq_pub_comp(protocol, party)};
  a.R = R;
  for (int k = 0; k < 4; ++k) a.w[k] = (const F*)sh[k];
  a.betad = fr_to_rprime(fr_load<F>(ch)), a.gamma = fr_load<F>(ch + 4);
  const dim3 grid(fr_stream_grid(a.g.values(), PQ_WG)), wg(PQ_WG);
  for (int half = 0; half < 2; ++half) {  // numerators, then denominators
    for (int k = 0; k < 4; ++k) a.pub[k] = (const F*)pub[4 * half + k], a.out[k] = (F*)out[4 * half + k];
    hipLaunchKernelGGL(k_ho_perm<F>, grid, wg, 0, st, a);
  }
  CSH_HIP(hipGetLastError());
  return CSH_OK;
}

template <class F>
static int z_perm_place_t(uint32_t protocol, uint32_t party, const uint64_t* mul, uint64_t* z, size_t n, size_t domain_size, const HoRanges& R,
                          hipStream_t st) {
  HoPlaceArgs<F> a;
  a.mul = (const F*)mul, a.z = (F*)z;
  a.one = F::one();
  a.domain_size = (uint32_t)domain_size;
  a.R = R;
  a.g = PqGeom{n, protocol + 1, pq_pub_comp(protocol, party)};
  hipLaunchKernelGGL(k_ho_place<F>, dim3(fr_stream_grid(a.g.values(), PQ_WG)), dim3(PQ_WG), 0, st, a);
  CSH_HIP(hipGetLastError());
  return CSH_OK;
}

}  // namespace csh

using namespace csh;

static int ho_check_party(uint32_t protocol, uint32_t party, const char* what) {
  if (protocol > 1 || party > 2) {
    set_error("%s: protocol must be 0 (plain / Shamir) or 1 (Rep3), party_id 0, 1 or 2", what);
    return CSH_ERR_INVALID;
  }
  return CSH_OK;
}

extern "C" {

int csh_honk_w4_records_dev(csh_curve_t field_of, uint32_t protocol, uint32_t party_id, const uint64_t* const* w_dev, uint64_t* w4_dev, size_t n,
                            const uint64_t* etas, const uint32_t* read_idx_dev, size_t n_read, const uint32_t* write_idx_dev, size_t n_write,
                            const uint32_t* shared_idx_dev, const uint64_t* type_share_dev, size_t n_shared, void* stream) {
  const char* what = "honk_w4_records";
  FR_REQUIRE_FIELD(field_of);
  CSH_TRY(ho_check_party(protocol, party_id, what));
  FR_REQUIRE_N(n);
  CSH_REQUIRE(n_read <= n && n_write <= n && n_shared <= n && n_read + n_write + n_shared <= n,
              "honk_w4_records: more records than rows (every index occurs at most once)");
  if (n_read + n_write + n_shared == 0) return CSH_OK;
  CSH_REQUIRE(w_dev && w4_dev && etas && (read_idx_dev || !n_read) && (write_idx_dev || !n_write) &&
                  ((shared_idx_dev && type_share_dev) || !n_shared),
              "honk_w4_records: NULL argument");
  CSH_TRY(fr_require_ptrs((const void* const*)w_dev, 3, what));
  const size_t ncomp = protocol + 1;
  FrRanges in, out;
  in.add((const void* const*)w_dev, 3, 32 * n * ncomp);
  if (n_read) in.add(read_idx_dev, 4 * n_read);
  if (n_write) in.add(write_idx_dev, 4 * n_write);
  if (n_shared) in.add(shared_idx_dev, 4 * n_shared), in.add(type_share_dev, 32 * n_shared * ncomp);
  out.add(w4_dev, 32 * n * ncomp);
  CSH_TRY(fr_check_ranges(in, out, what));
  CSH_TRY(ensure_device());
  hipStream_t st = resolve_stream(stream);
  return FR_CALL(field_of, w4_records_t<F>(protocol, party_id, w_dev, w4_dev, n, etas, read_idx_dev, n_read, write_idx_dev, n_write,
                                           shared_idx_dev, type_share_dev, n_shared, st));
}

int csh_honk_lookup_operands_dev(csh_curve_t field_of, uint32_t protocol, uint32_t party_id, const uint64_t* const* shares_dev,
                                 const uint64_t* const* public_dev, size_t n, const uint64_t* challenges, uint64_t* const* out_dev, void* stream) {
  const char* what = "honk_lookup_operands";
  FR_REQUIRE_FIELD(field_of);
  CSH_TRY(ho_check_party(protocol, party_id, what));
  CSH_REQUIRE(shares_dev && public_dev && challenges && out_dev, "honk_lookup_operands: NULL argument");
  CSH_TRY(fr_require_ptrs((const void* const*)shares_dev, 4, what));
  CSH_TRY(fr_require_ptrs((const void* const*)public_dev, 9, what));
  CSH_TRY(fr_require_ptrs((const void* const*)out_dev, 2, what));
  CSH_REQUIRE(n >= 1 && n <= FR_MAX_N, "honk_lookup_operands: n must be 1 .. 2^28");
  const size_t sb = 32 * n * (protocol + 1);
  FrRanges in, out;
  in.add((const void* const*)shares_dev, 4, sb);
  in.add((const void* const*)public_dev, 9, 32 * n);
  out.add((const void* const*)out_dev, 2, sb);
  CSH_TRY(fr_check_ranges(in, out, what));
  CSH_TRY(ensure_device());
  hipStream_t st = resolve_stream(stream);
  return FR_CALL(field_of, lookup_operands_t<F>(protocol, party_id, shares_dev, public_dev, n, challenges, out_dev, st));
}

int csh_honk_perm_operands_dev(csh_curve_t field_of, uint32_t protocol, uint32_t party_id, const uint64_t* const* shares_dev,
                               const uint64_t* const* public_dev, size_t n, size_t domain_size, const size_t* ranges, size_t num_ranges,
                               const uint64_t* challenges, uint64_t* const* out_dev, void* stream) {
  const char* what = "honk_perm_operands";
  FR_REQUIRE_FIELD(field_of);
  CSH_TRY(ho_check_party(protocol, party_id, what));
  CSH_REQUIRE(shares_dev && public_dev && challenges && out_dev, "honk_perm_operands: NULL argument");
  CSH_TRY(fr_require_ptrs((const void* const*)shares_dev, 4, what));
  CSH_TRY(fr_require_ptrs((const void* const*)public_dev, 8, what));
  CSH_TRY(fr_require_ptrs((const void* const*)out_dev, 8, what));
  HoRanges R;
  CSH_TRY(ho_ranges(R, ranges, num_ranges, n, domain_size, what));
  const size_t m = (size_t)R.active - 1, ncomp = protocol + 1;
  if (m == 0) return CSH_OK;
  FrRanges in, out;
  in.add((const void* const*)shares_dev, 4, 32 * n * ncomp);
  in.add((const void* const*)public_dev, 8, 32 * n);
  out.add((const void* const*)out_dev, 8, 32 * m * ncomp);
  CSH_TRY(fr_check_ranges(in, out, what));
  CSH_TRY(ensure_device());
  hipStream_t st = resolve_stream(stream);
  return FR_CALL(field_of, perm_operands_t<F>(protocol, party_id, shares_dev, public_dev, R, challenges, out_dev, st));
}

int csh_honk_z_perm_place_dev(csh_curve_t field_of, uint32_t protocol, uint32_t party_id, const uint64_t* mul_dev, uint64_t* z_dev, size_t n,
                              size_t domain_size, const size_t* ranges, size_t num_ranges, void* stream) {
  const char* what = "honk_z_perm_place";
  FR_REQUIRE_FIELD(field_of);
  CSH_TRY(ho_check_party(protocol, party_id, what));
  HoRanges R;
  CSH_TRY(ho_ranges(R, ranges, num_ranges, n, domain_size, what));
  const size_t m = (size_t)R.active - 1, ncomp = protocol + 1;
  CSH_REQUIRE(z_dev && (mul_dev || !m), "honk_z_perm_place: NULL argument");
  FrRanges in, out;
  if (m) in.add(mul_dev, 32 * m * ncomp);
  out.add(z_dev, 32 * n * ncomp);
  CSH_TRY(fr_check_ranges(in, out, what));
  CSH_TRY(ensure_device());
  hipStream_t st = resolve_stream(stream);
  return FR_CALL(field_of, z_perm_place_t<F>(protocol, party_id, mul_dev, z_dev, n, domain_size, R, st));
}

}  // extern "C"
