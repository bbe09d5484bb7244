// The element-wise stages of the circom PLONK quotient, Round3::compute_t (co-circom/co-plonk/src/round3.rs:246-502):
// (a) blinders, (b) gate and permutation operands, (c) combine, (d) division by Z_H on coefficient form and the split into t1 / t2 / t3.
// The reference's three for_each loops over the 4 n points are affine in the shares with public coefficients: no network round, HBM-bound
// streaming kernels of the vec_ops.hip kind -- grid-stride over flat value indices, 256 lanes, tune "vec_max_blocks". Stage (b) is four
// kernels (public-input sum, the e1 / e1z group, the e2 group, the e3 group) so that none holds twenty streams in registers. Expressions,
// index algebra and bounds: plonk_quot.hpp, shared with the host self-test.
//
// Powers w^i. A domain keeps no natural-order twiddle table by default (ntt.hip releases it once the staged tables are made), so every call
// that needs w^i builds the two-level table of plonk_quot.hpp on the device first: 256 + N / 256 entries, square-and-multiply per entry, in
// the stream's workspace. Nothing of size N is uploaded.
#include "plonk_quot.hpp"

#include <vector>

namespace csh {

template <class F>
__global__ __launch_bounds__(PQ_WG) void k_pq_blinders(PqBlindArgs<F> a) {
  for (size_t e = blockIdx.x * (size_t)PQ_WG + threadIdx.x; e < a.g.values(); e += (size_t)gridDim.x * PQ_WG)
    pq_blinders_at(a, (int)blockIdx.y, e);  // blockIdx.y = the output: ap, bp, cp, zp, zwp
}
template <class F>
__global__ __launch_bounds__(PQ_WG) void k_pq_pi(PqPiArgs<F> a) {
  for (size_t e = blockIdx.x * (size_t)PQ_WG + threadIdx.x; e < a.g.values(); e += (size_t)gridDim.x * PQ_WG) pq_pi_at(a, e);
}
template <class F>
__global__ __launch_bounds__(PQ_WG) void k_pq_e1(PqE1Args<F> a) {
  const size_t e0 = blockIdx.x * (size_t)PQ_WG + threadIdx.x;
  const F z1d_m = pq_e1_lane(a, e0);
  for (size_t e = e0; e < a.g.values(); e += (size_t)gridDim.x * PQ_WG) pq_e1_at(a, z1d_m, e);
}
template <class F>
__global__ __launch_bounds__(PQ_WG) void k_pq_e2(PqE2Args<F> a) {
  for (size_t e = blockIdx.x * (size_t)PQ_WG + threadIdx.x; e < a.g.values(); e += (size_t)gridDim.x * PQ_WG) pq_e2_at(a, e);
}
template <class F>
__global__ __launch_bounds__(PQ_WG) void k_pq_e3(PqE3Args<F> a) {
  for (size_t e = blockIdx.x * (size_t)PQ_WG + threadIdx.x; e < a.g.values(); e += (size_t)gridDim.x * PQ_WG) pq_e3_at(a, e);
}
template <class F>
__global__ __launch_bounds__(PQ_WG) void k_pq_combine(PqCombineArgs<F> a) {
  const size_t e0 = blockIdx.x * (size_t)PQ_WG + threadIdx.x;
  const PqCombineLane<F> lk = pq_combine_lane(a, e0);
  for (size_t e = e0; e < a.g.values(); e += (size_t)gridDim.x * PQ_WG) pq_combine_at(a, lk, e);
}
template <class F>
__global__ __launch_bounds__(PQ_WG) void k_pq_finish(PqFinishArgs<F> a) {
  const size_t nv = a.n * a.ncomp;
  for (size_t e = blockIdx.x * (size_t)PQ_WG + threadIdx.x; e < nv; e += (size_t)gridDim.x * PQ_WG) pq_finish_at(a, e);
}

static PqGeom pq_geom(size_t N, uint32_t protocol, uint32_t party) { return PqGeom{N, protocol + 1, pq_pub_comp(protocol, party)}; }

template <class F>
static int blinders_t(const Domain* d, uint32_t protocol, uint32_t party, const uint64_t* blinders, uint64_t* const* out, hipStream_t st) {
  const F gen = fr_load<F>(domain_gen_of(d));
  PqBlindArgs<F> a;
  a.g = pq_geom(domain_size_of(d), protocol, party);
  pq_blinders_consts(a, gen, blinders, a.g.ncomp);
  CSH_TRY(pq_power_tables<F>(gen, a.g.N, st, &a.hi, &a.lo));
  for (int v = 0; v < 5; ++v) a.out[v] = (F*)out[v];
  hipLaunchKernelGGL(k_pq_blinders<F>, dim3(fr_stream_grid(a.g.values(), PQ_WG), 5), dim3(PQ_WG), 0, st, a);
  CSH_HIP(hipGetLastError());
  return CSH_OK;
}

template <class F>
static int operands_t(const Domain* d, uint32_t protocol, uint32_t party, const uint64_t* const* sh, const uint64_t* const* pub,
                      const uint64_t* const* lagrange, size_t n_public, const uint64_t* buffer_a, const uint64_t* ch, uint64_t* const* out,
                      hipStream_t st) {
  const F gen = fr_load<F>(domain_gen_of(d));
  const PqGeom g = pq_geom(domain_size_of(d), protocol, party);
  const dim3 grid(fr_stream_grid(g.values(), PQ_WG)), wg(PQ_WG);
  const F beta = fr_load<F>(ch), gamma = fr_load<F>(ch + 4), k1 = fr_load<F>(ch + 8), k2 = fr_load<F>(ch + 12);
  // pi: ceil(n_public / PQ_PI_CHUNK) launches, at least one (n_public = 0 writes zeros)
  for (size_t j0 = 0; j0 == 0 || j0 < n_public; j0 += PQ_PI_CHUNK) {
    PqPiArgs<F> p;
    pq_pi_consts(p, lagrange, buffer_a, j0, n_public, g.ncomp);
    p.pi = (F*)out[0];
    p.g = g;
    hipLaunchKernelGGL(k_pq_pi<F>, grid, wg, 0, st, p);
  }
  {
    PqE1Args<F> a;
    const F** s[] = {&a.a, &a.b, &a.c, nullptr, &a.a_b, &a.a_bp, &a.ap_b, &a.ap_bp, &a.ap, &a.bp, &a.cp};
    for (int v = 0; v < 11; ++v)
      if (s[v]) *s[v] = (const F*)sh[v];
    a.pi = (const F*)out[0];
    a.qm = (const F*)pub[0], a.ql = (const F*)pub[1], a.qr = (const F*)pub[2], a.qo = (const F*)pub[3], a.qc = (const F*)pub[4];
    a.e1 = (F*)out[1], a.e1z = (F*)out[2];
    const PqZ<F> z = pq_z_tables(gen, g.N);
    for (int m = 0; m < 4; ++m) a.z1d[m] = fr_to_rprime(z.z1[m]);
    a.g = g;
    hipLaunchKernelGGL(k_pq_e1<F>, grid, wg, 0, st, a);
  }
  {
    PqE2Args<F> a;
    for (int v = 0; v < 3; ++v) a.in[v] = (const F*)sh[v], a.out[v] = (F*)out[3 + v];
    a.bk[0] = beta, a.bk[1] = F::mul(beta, k1), a.bk[2] = F::mul(beta, k2);
    a.gamma = gamma;
    a.g = g;
    CSH_TRY(pq_power_tables<F>(gen, g.N, st, &a.hi, &a.lo));
    hipLaunchKernelGGL(k_pq_e2<F>, grid, wg, 0, st, a);
  }
  {
    PqE3Args<F> a;
    for (int v = 0; v < 3; ++v) a.in[v] = (const F*)sh[v], a.s[v] = (const F*)pub[5 + v], a.out[v] = (F*)out[6 + v];
    a.z = (const F*)sh[3];
    a.e3d = (F*)out[9];
    a.betad = fr_to_rprime(beta);
    a.gamma = gamma;
    a.g = g;
    hipLaunchKernelGGL(k_pq_e3<F>, grid, wg, 0, st, a);
  }
  CSH_HIP(hipGetLastError());
  return CSH_OK;
}

template <class F>
static int combine_t(const Domain* d, uint32_t protocol, uint32_t party, const uint64_t* const* sh, const uint64_t* l1, const uint64_t* alpha,
                     uint64_t* const* out, hipStream_t st) {
  PqCombineArgs<F> a;
  a.g = pq_geom(domain_size_of(d), protocol, party);
  a.e1 = (const F*)sh[0], a.e1z = (const F*)sh[1], a.z = (const F*)sh[2], a.zp = (const F*)sh[3], a.e2 = (const F*)sh[4], a.e3 = (const F*)sh[9];
  for (int j = 0; j < 4; ++j) a.e2z[j] = (const F*)sh[5 + j], a.e3z[j] = (const F*)sh[10 + j];
  a.l1 = (const F*)l1;
  a.t = (F*)out[0], a.tz = (F*)out[1];
  a.k = pq_combine_consts(fr_load<F>(domain_gen_of(d)), a.g.N, fr_load<F>(alpha));
  hipLaunchKernelGGL(k_pq_combine<F>, dim3(fr_stream_grid(a.g.values(), PQ_WG)), dim3(PQ_WG), 0, st, a);
  CSH_HIP(hipGetLastError());
  return CSH_OK;
}

template <class F>
static int finish_t(size_t n, uint32_t ncomp, const uint64_t* ct, const uint64_t* ctz, const uint64_t* b9_b10, uint64_t* t1, uint64_t* t2,
                    uint64_t* t3, hipStream_t st) {
  PqFinishArgs<F> a;
  a.ct = (const F*)ct, a.ctz = (const F*)ctz;
  a.t1 = (F*)t1, a.t2 = (F*)t2, a.t3 = (F*)t3;
  pq_share(a.b9, b9_b10, ncomp);
  pq_share(a.b10, b9_b10 + 4 * ncomp, ncomp);
  a.n = n, a.ncomp = ncomp;
  hipLaunchKernelGGL(k_pq_finish<F>, dim3(fr_stream_grid(n * ncomp, PQ_WG)), dim3(PQ_WG), 0, st, a);
  CSH_HIP(hipGetLastError());
  return CSH_OK;
}

}  // namespace csh

using namespace csh;

// No output of a call may overlap an input or another output (fr_check_ranges): the rotations by 4 (zwp, e3d) and the chunked columns of
// the finish make a call in place a race between workgroups.

static int pq_check_party(uint32_t protocol, uint32_t party, const char* what) {
  if (protocol > 1 || party > 2) {
    set_error("%s: protocol must be 0 (plain / Shamir) or 1 (Rep3), party_id 0, 1 or 2", what);
    return CSH_ERR_INVALID;
  }
  return CSH_OK;
}
// a domain handle exists only in a process that has a device, so it is looked into after ensure_device() and before any launch
static int pq_check_domain(const Domain* d, const char* what) {
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
  return CSH_OK;
}

extern "C" {

int csh_plonk_quot_blinders_dev(csh_domain_t ext_dom, uint32_t protocol, uint32_t party_id, const uint64_t* blinders, uint64_t* const* out_dev,
                                void* stream) {
  const char* what = "plonk_quot_blinders";
  CSH_TRY(pq_check_party(protocol, party_id, what));
  CSH_REQUIRE(ext_dom && blinders && out_dev, "plonk_quot_blinders: NULL argument");
  CSH_TRY(fr_require_ptrs((const void* const*)out_dev, 5, what));
  CSH_TRY(ensure_device());
  const Domain* d = reinterpret_cast<const Domain*>(ext_dom);
  CSH_TRY(pq_check_domain(d, what));
  FrRanges in, out;
  out.add((const void* const*)out_dev, 5, 32 * domain_size_of(d) * (protocol + 1));
  CSH_TRY(fr_check_ranges(in, out, what));
  hipStream_t st = resolve_stream(stream);
  return FR_CALL(domain_curve_of(d), blinders_t<F>(d, protocol, party_id, blinders, out_dev, st));
}

int csh_plonk_quot_operands_dev(csh_domain_t ext_dom, uint32_t protocol, uint32_t party_id, const uint64_t* const* shares_dev,
                                const uint64_t* const* public_dev, const uint64_t* const* lagrange_dev, size_t n_public, const uint64_t* buffer_a,
                                const uint64_t* challenges, uint64_t* const* out_dev, void* stream) {
  const char* what = "plonk_quot_operands";
  CSH_TRY(pq_check_party(protocol, party_id, what));
  CSH_REQUIRE(ext_dom && shares_dev && public_dev && challenges && out_dev && (n_public == 0 || (lagrange_dev && buffer_a)),
              "plonk_quot_operands: NULL argument");
  CSH_REQUIRE(n_public <= (size_t(1) << 24), "plonk_quot_operands: n_public exceeds 2^24");
  CSH_TRY(fr_require_ptrs((const void* const*)shares_dev, 11, what));
  CSH_TRY(fr_require_ptrs((const void* const*)public_dev, 8, what));
  CSH_TRY(fr_require_ptrs((const void* const*)lagrange_dev, n_public, what));
  CSH_TRY(fr_require_ptrs((const void* const*)out_dev, 10, what));
  CSH_TRY(ensure_device());
  const Domain* d = reinterpret_cast<const Domain*>(ext_dom);
  CSH_TRY(pq_check_domain(d, what));
  const size_t pb = 32 * domain_size_of(d), sb = pb * (protocol + 1);
  FrRanges in, out;
  in.add((const void* const*)shares_dev, 11, sb);
  in.add((const void* const*)public_dev, 8, pb);
  in.add((const void* const*)lagrange_dev, n_public, pb);
  out.add((const void* const*)out_dev, 10, sb);
  CSH_TRY(fr_check_ranges(in, out, what));
  hipStream_t st = resolve_stream(stream);
  return FR_CALL(domain_curve_of(d),
                 operands_t<F>(d, protocol, party_id, shares_dev, public_dev, lagrange_dev, n_public, buffer_a, challenges, out_dev, st));
}

int csh_plonk_quot_combine_dev(csh_domain_t ext_dom, uint32_t protocol, uint32_t party_id, const uint64_t* const* shares_dev,
                               const uint64_t* lagrange1_dev, const uint64_t alpha[4], uint64_t* const* out_dev, void* stream) {
  const char* what = "plonk_quot_combine";
  CSH_TRY(pq_check_party(protocol, party_id, what));
  CSH_REQUIRE(ext_dom && shares_dev && lagrange1_dev && alpha && out_dev, "plonk_quot_combine: NULL argument");
  CSH_TRY(fr_require_ptrs((const void* const*)shares_dev, 14, what));
  CSH_TRY(fr_require_ptrs((const void* const*)out_dev, 2, what));
  CSH_TRY(ensure_device());
  const Domain* d = reinterpret_cast<const Domain*>(ext_dom);
  CSH_TRY(pq_check_domain(d, what));
  const size_t pb = 32 * domain_size_of(d), sb = pb * (protocol + 1);
  FrRanges in, out;
  in.add((const void* const*)shares_dev, 14, sb);
  in.add(lagrange1_dev, pb);
  out.add((const void* const*)out_dev, 2, sb);
  CSH_TRY(fr_check_ranges(in, out, what));
  hipStream_t st = resolve_stream(stream);
  return FR_CALL(domain_curve_of(d), combine_t<F>(d, protocol, party_id, shares_dev, lagrange1_dev, alpha, out_dev, st));
}

int csh_plonk_quot_finish_dev(csh_curve_t field_of, size_t n, uint32_t protocol, uint32_t party_id, const uint64_t* ct_dev, const uint64_t* ctz_dev,
                              const uint64_t* b9_b10, uint64_t* t1_dev, uint64_t* t2_dev, uint64_t* t3_dev, void* stream) {
  const char* what = "plonk_quot_finish";
  CSH_REQUIRE(fr_known(field_of), "plonk_quot_finish: field_of must be BN254, BLS12-381 or BLS12-377");
  CSH_TRY(pq_check_party(protocol, party_id, what));
  CSH_REQUIRE(ct_dev && ctz_dev && b9_b10 && t1_dev && t2_dev && t3_dev, "plonk_quot_finish: NULL argument");
  CSH_REQUIRE(n >= 8 && n <= FR_MAX_N / 4 && (n & (n - 1)) == 0, "plonk_quot_finish: n must be a power of two, 8 .. 2^26");
  const size_t sb = 32 * (size_t)(protocol + 1);
  FrRanges in, out;
  in.add(ct_dev, 4 * n * sb), in.add(ctz_dev, 4 * n * sb);
  out.add(t1_dev, (n + 1) * sb), out.add(t2_dev, (n + 1) * sb), out.add(t3_dev, (n + 6) * sb);
  CSH_TRY(fr_check_ranges(in, out, what));
  CSH_TRY(ensure_device());
  hipStream_t st = resolve_stream(stream);
  return FR_CALL(field_of, finish_t<F>(n, protocol + 1, ct_dev, ctz_dev, b9_b10, t1_dev, t2_dev, t3_dev, st));
}

}  // extern "C"
