// Batched Poseidon2 on the device: the packed permutations of mpc-core/src/gadgets/poseidon2/ and the Merkle trees of
// gadgets/merkle_tree/, plain and on Rep3 / Shamir shares. Per-state functions, the parameter table and the limb bounds: poseidon2.hpp,
// shared with the host self-test.
//
// k_p2_plain: one lane per state, the whole permutation in one launch with the state in registers (t x 9 limbs); grid-stride over the
// states, 256 lanes, no LDS, tune "vec_max_blocks". A Merkle tree is one launch of the same kernel per layer in its gathering form; only
// element 0 of a state is ever written, and nothing returns to the host between layers.
// k_p2_co_step: one lane per (state, component), the local stretch between two openings; k_p2_next: one lane per output value.
// The round constants are read through the kernel argument at a round index every lane shares.
// profiles/poseidon2_kernel_meta.csv: no scratch, no VGPR spill.
#include "plonk_quot.hpp"
#include "poseidon2.hpp"

namespace csh {

constexpr int P2_WG = 256;

template <class F, int T>
__global__ __launch_bounds__(P2_WG) void k_p2_plain(P2PlainArgs<F> a) {
  for (size_t i = blockIdx.x * (size_t)P2_WG + threadIdx.x; i < a.n; i += (size_t)gridDim.x * P2_WG) p2_plain_at<F, T>(a, i);
}
template <class F, int T>
__global__ __launch_bounds__(P2_WG) void k_p2_co_step(P2CoArgs<F> a) {
  const size_t values = a.n_perm * a.ncomp;
  for (size_t u = blockIdx.x * (size_t)P2_WG + threadIdx.x; u < values; u += (size_t)gridDim.x * P2_WG) p2_co_step_at<F, T>(a, u);
}
template <class F>
__global__ __launch_bounds__(P2_WG) void k_p2_next(P2NextArgs<F> a) {
  const size_t values = a.values();
  for (size_t v = blockIdx.x * (size_t)P2_WG + threadIdx.x; v < values; v += (size_t)gridDim.x * P2_WG) p2_next_at(a, v);
}

// ---- the parameter handle -------------------------------------------------------------------------------------------------------------------
struct P2Params {
  csh_curve_t field;
  int device;
  uint32_t t, rf_b, rf_e, rp;
  uint64_t diag_rp[16];  // four elements, R' domain
  void* table = nullptr;  // P2Table's vectors on the device
  ~P2Params() {
    if (table) (void)hipFree(table);
  }
};
template <class F>
static P2Table<F> p2_table_of(const P2Params* h) {
  P2Table<F> tab;
  memcpy(tab.diag_rp, h->diag_rp, sizeof(tab.diag_rp));
  tab.t = h->t, tab.rf_b = h->rf_b, tab.rf_e = h->rf_e, tab.rp = h->rp;
  p2_point_table(tab, (const F*)h->table);
  return tab;
}
static bool p2_fixed_diag_ok(csh_curve_t field_of, uint32_t t, const uint64_t* diag) {
  return FR_CALL(field_of, [&]() -> int {
           for (uint32_t i = 0; i < t; ++i) {
             const F want = i + 1 == t ? F::add(F::one(), F::one()) : F::one();
             if (memcmp(diag + 4 * i, &want, sizeof(F)) != 0) return 0;
           }
           return 1;
         }()) == 1;
}
template <class F>
static int p2_create_t(P2Params* h, const uint64_t* rc_ext, const uint64_t* rc_int, const uint64_t* diag, hipStream_t st) {
  std::vector<F> store;
  P2Table<F> tab;
  p2_build_table(h->t, h->rf_b, h->rf_e, h->rp, rc_ext, rc_int, diag, store, tab);
  memcpy(h->diag_rp, tab.diag_rp, sizeof(tab.diag_rp));
  CSH_HIP(hipMalloc(&h->table, store.size() * sizeof(F) + 32));
  CSH_HIP(hipMemcpyAsync(h->table, store.data(), store.size() * sizeof(F), hipMemcpyHostToDevice, st));
  CSH_HIP(hipStreamSynchronize(st));  // `store` leaves with this call
  return CSH_OK;
}
static int p2_handle(csh_poseidon2_params_t handle, const P2Params** out, const char* what) {
  if (!handle) {
    set_error("%s: the parameter handle is NULL", what);
    return CSH_ERR_INVALID;
  }
  const P2Params* h = reinterpret_cast<const P2Params*>(handle);
  int cur = 0;
  if (hipGetDevice(&cur) == hipSuccess && cur != h->device) {
    set_error("%s: the parameter table lives on device %d but the calling thread is bound to device %d (csh_init)", what, h->device, cur);
    return CSH_ERR_INVALID;
  }
  *out = h;
  return CSH_OK;
}

// ---- launchers ------------------------------------------------------------------------------------------------------------------------------
template <class F>
static int p2_plain_launch(const P2Params* h, const P2PlainArgs<F>& a, hipStream_t st) {
  const dim3 grid(fr_stream_grid(a.n, P2_WG)), wg(P2_WG);
  switch (h->t) {
    case 2: hipLaunchKernelGGL((k_p2_plain<F, 2>), grid, wg, 0, st, a); break;
    case 3: hipLaunchKernelGGL((k_p2_plain<F, 3>), grid, wg, 0, st, a); break;
    default: hipLaunchKernelGGL((k_p2_plain<F, 4>), grid, wg, 0, st, a); break;
  }
  return CSH_OK;
}
template <class F>
static int p2_permute_t(const P2Params* h, const uint64_t* state, size_t n, uint64_t* out, hipStream_t st) {
  const P2PlainArgs<F> a{p2_table_of<F>(h), (const F*)state, (F*)out, n, h->t, 1, 0};
  CSH_TRY(p2_plain_launch(h, a, st));
  CSH_HIP(hipGetLastError());
  return CSH_OK;
}
// layers n_leaves / arity, n_leaves / arity^2, .. , 1: the outputs ping-pong between the halves of `work`, the last goes to `root`
template <class F>
static int p2_merkle_t(const P2Params* h, uint32_t arity, uint32_t mode, const uint64_t* leaves, size_t n_leaves, uint64_t* root, uint64_t* work,
                       hipStream_t st) {
  if (n_leaves == 1) {
    CSH_HIP(hipMemcpyAsync(root, leaves, sizeof(F), hipMemcpyDeviceToDevice, st));
    return CSH_OK;
  }
  const size_t half = n_leaves / arity;
  const F* src = (const F*)leaves;
  int side = 0;
  for (size_t len = half; len >= 1; len /= arity) {
    F* dst = len == 1 ? (F*)root : (F*)work + (side ? half : 0);
    const P2PlainArgs<F> a{p2_table_of<F>(h), src, dst, len, arity, 0, mode == (uint32_t)P2_COMPRESSION};
    CSH_TRY(p2_plain_launch(h, a, st));
    src = dst, side ^= 1;
    if (len == 1) break;
  }
  CSH_HIP(hipGetLastError());
  return CSH_OK;
}
template <class F>
static int p2_co_round_t(const P2Params* h, const P2CoArgs<F>& proto, hipStream_t st) {
  P2CoArgs<F> a = proto;
  a.tab = p2_table_of<F>(h);
  const dim3 grid(fr_stream_grid(a.n_perm * a.ncomp, P2_WG)), wg(P2_WG);
  switch (h->t) {
    case 2: hipLaunchKernelGGL((k_p2_co_step<F, 2>), grid, wg, 0, st, a); break;
    case 3: hipLaunchKernelGGL((k_p2_co_step<F, 3>), grid, wg, 0, st, a); break;
    default: hipLaunchKernelGGL((k_p2_co_step<F, 4>), grid, wg, 0, st, a); break;
  }
  CSH_HIP(hipGetLastError());
  return CSH_OK;
}
template <class F>
static int p2_next_t(const P2NextArgs<F>& a, hipStream_t st) {
  hipLaunchKernelGGL(k_p2_next<F>, dim3(fr_stream_grid(a.values(), P2_WG)), dim3(P2_WG), 0, st, a);
  CSH_HIP(hipGetLastError());
  return CSH_OK;
}

// ---- argument rules -------------------------------------------------------------------------------------------------------------------------
static int p2_check_shape(uint32_t t, uint32_t rf_b, uint32_t rf_e, uint32_t rp, const char* what) {
  if (t < 2 || t > 4) {
    set_error("%s: t must be 2, 3 or 4 (d = 5)", what);
    return CSH_ERR_INVALID;
  }
  if (rf_b > P2_MAX_ROUNDS || rf_e > P2_MAX_ROUNDS || rp > P2_MAX_ROUNDS) {
    set_error("%s: a round count above %u", what, P2_MAX_ROUNDS);
    return CSH_ERR_INVALID;
  }
  return CSH_OK;
}
// n_leaves = arity^k, k >= 0; sponge needs t > arity, compression t >= arity
static int p2_check_tree(uint32_t t, uint32_t arity, uint32_t mode, size_t n_leaves, const char* what) {
  if (mode != (uint32_t)P2_SPONGE && mode != (uint32_t)P2_COMPRESSION) {
    set_error("%s: mode must be 0 (sponge) or 1 (compression)", what);
    return CSH_ERR_INVALID;
  }
  if (arity < 2 || (mode == (uint32_t)P2_SPONGE ? t <= arity : t < arity)) {
    set_error("%s: arity must be at least 2, below t in sponge mode and at most t in compression mode", what);
    return CSH_ERR_INVALID;
  }
  size_t v = n_leaves;
  while (v > 1 && v % arity == 0) v /= arity;
  if (v != 1 || n_leaves > FR_MAX_N) {
    set_error("%s: n_leaves must be a power of the arity, at most 2^28", what);
    return CSH_ERR_INVALID;
  }
  return CSH_OK;
}
// precomputation entries round r consumes: n_perm * t in an external round, n_perm in an internal one
static size_t p2_round_entries(const P2Params* h, uint32_t r, size_t n_perm) {
  const bool ext = r < h->rf_b || r >= h->rf_b + h->rp;
  return ext ? n_perm * h->t : n_perm;
}

static int p2_check_co(csh_curve_t field_of, uint32_t protocol, uint32_t party_id, const P2Params* h, uint32_t step, const uint64_t* state,
                       size_t n_perm, const uint64_t* y, const uint64_t* const* pre, size_t pre_off, const uint64_t* open, const uint64_t* ff_out) {
  const char* what = "poseidon2_co_round";
  FR_REQUIRE_FIELD(field_of);
  CSH_REQUIRE(field_of == h->field, "poseidon2_co_round: field_of is not the parameter table's field");
  CSH_REQUIRE(protocol <= 1 && party_id <= 2, "poseidon2_co_round: protocol must be 0 (plain / Shamir) or 1 (Rep3), party_id 0, 1 or 2");
  const uint32_t R = h->rf_b + h->rp + h->rf_e;
  CSH_REQUIRE(step <= R, "poseidon2_co_round: step must be 0 .. rounds_f_beginning + rounds_p + rounds_f_end");
  CSH_REQUIRE(n_perm <= FR_MAX_N / 4, "poseidon2_co_round: n_perm exceeds 2^26");
  CSH_REQUIRE(pre_off <= (size_t(1) << 40), "poseidon2_co_round: precomp_offset exceeds 2^40");
  if (!n_perm) return CSH_OK;
  const bool post = step > 0, prep = step < R;
  bool ok = state != nullptr && pre != nullptr && (y || !post) && (open || !prep);
  for (int k = 0; ok && k < 5; ++k) ok = pre[k] != nullptr || (k > 0 && !post);
  if (!ok) {
    set_error("%s: NULL argument", what);
    return CSH_ERR_INVALID;
  }
  const size_t back = post ? p2_round_entries(h, step - 1, n_perm) : 0, fwd = prep ? p2_round_entries(h, step, n_perm) : 0;
  CSH_REQUIRE(pre_off >= back, "poseidon2_co_round: precomp_offset lies below the entries of the round the step finishes");
  const size_t eb = 32 * (size_t)(protocol + 1);
  FrRanges in, out;
  if (post) {
    in.add(y, 32 * back);
    for (int k = 0; k < 5; ++k) in.add((const char*)pre[k] + eb * (pre_off - back), eb * back);
  }
  if (prep) in.add((const char*)pre[0] + eb * pre_off, eb * fwd);
  out.add(state, eb * n_perm * h->t);
  if (prep) out.add(open, eb * fwd);
  if (step == 0 && ff_out) out.add(ff_out, eb * n_perm);
  return fr_check_ranges(in, out, what);
}
static int p2_check_next(csh_curve_t field_of, uint32_t ncomp, uint32_t t, uint32_t arity, uint32_t mode, const uint64_t* state, const uint64_t* ff,
                         const uint64_t* next, size_t len) {
  const char* what = "poseidon2_layer_next";
  FR_REQUIRE_FIELD(field_of);
  FR_REQUIRE_NCOMP(ncomp);
  CSH_TRY(p2_check_shape(t, 0, 0, 0, what));
  CSH_TRY(p2_check_tree(t, arity, mode, 1, what));
  CSH_REQUIRE(len >= 1 && len <= FR_MAX_N && (len == 1 || len % arity == 0), "poseidon2_layer_next: len must be 1 or a multiple of the arity, at most 2^28");
  if (!state || !next || (mode == (uint32_t)P2_COMPRESSION && !ff)) {
    set_error("%s: NULL argument", what);
    return CSH_ERR_INVALID;
  }
  const size_t eb = 32 * (size_t)ncomp;
  FrRanges in, out;
  in.add(state, eb * len * t);
  if (mode == (uint32_t)P2_COMPRESSION) in.add(ff, eb * len);
  out.add(next, len == 1 ? eb : eb * (len / arity) * t);
  return fr_check_ranges(in, out, what);
}

}  // namespace csh

using namespace csh;

extern "C" {

int csh_poseidon2_params_create(csh_curve_t field_of, uint32_t t, uint32_t rounds_f_beginning, uint32_t rounds_f_end, uint32_t rounds_p,
                                const uint64_t* rc_external, const uint64_t* rc_internal, const uint64_t* diag_m_1, csh_poseidon2_params_t* handle) {
  CSH_REQUIRE(handle, "poseidon2_params_create: handle is NULL");
  *handle = nullptr;
  FR_REQUIRE_FIELD(field_of);
  CSH_TRY(p2_check_shape(t, rounds_f_beginning, rounds_f_end, rounds_p, "poseidon2_params_create"));
  CSH_REQUIRE(diag_m_1 && (rc_external || !(rounds_f_beginning + rounds_f_end)) && (rc_internal || !rounds_p), "poseidon2_params_create: NULL argument");
  CSH_REQUIRE(t == 4 || p2_fixed_diag_ok(field_of, t, diag_m_1),
              "poseidon2_params_create: at t = 2 and t = 3 the internal matrix is fixed: diag_m_1 must be (1, 2) or (1, 1, 2)");
  CSH_TRY(ensure_device());
  P2Params* h = new P2Params();
  h->field = field_of, h->t = t, h->rf_b = rounds_f_beginning, h->rf_e = rounds_f_end, h->rp = rounds_p;
  if (hipGetDevice(&h->device) != hipSuccess) h->device = 0;
  const int rc = FR_CALL(field_of, p2_create_t<F>(h, rc_external, rc_internal, diag_m_1, resolve_stream(nullptr)));
  if (rc != CSH_OK) {
    delete h;
    return rc;
  }
  *handle = reinterpret_cast<csh_poseidon2_params_t>(h);
  return CSH_OK;
}

int csh_poseidon2_params_destroy(csh_poseidon2_params_t handle) {
  delete reinterpret_cast<P2Params*>(handle);
  return CSH_OK;
}

int csh_poseidon2_permute_dev(csh_poseidon2_params_t handle, const uint64_t* state_dev, size_t n_perm, uint64_t* out_dev, void* stream) {
  CSH_REQUIRE(handle, "poseidon2_permute: the parameter handle is NULL");
  CSH_REQUIRE(n_perm <= FR_MAX_N / 4, "poseidon2_permute: n_perm exceeds 2^26");
  if (!n_perm) return CSH_OK;
  CSH_REQUIRE(state_dev && out_dev, "poseidon2_permute: NULL argument");
  const P2Params* h0 = reinterpret_cast<const P2Params*>(handle);
  if (out_dev != state_dev) {  // in place is a lane reading and writing its own state; any other overlap is a race
    FrRanges in, out;
    in.add(state_dev, 32 * n_perm * h0->t);
    out.add(out_dev, 32 * n_perm * h0->t);
    CSH_TRY(fr_check_ranges(in, out, "poseidon2_permute"));
  }
  CSH_TRY(ensure_device());
  const P2Params* h;
  CSH_TRY(p2_handle(handle, &h, "poseidon2_permute"));
  return FR_CALL(h->field, p2_permute_t<F>(h, state_dev, n_perm, out_dev, resolve_stream(stream)));
}

int csh_poseidon2_merkle_dev(csh_poseidon2_params_t handle, uint32_t arity, uint32_t mode, const uint64_t* leaves_dev, size_t n_leaves,
                             uint64_t* root_dev, uint64_t* work_dev, void* stream) {
  CSH_REQUIRE(handle, "poseidon2_merkle: the parameter handle is NULL");
  const P2Params* h0 = reinterpret_cast<const P2Params*>(handle);
  CSH_TRY(p2_check_tree(h0->t, arity, mode, n_leaves, "poseidon2_merkle"));
  const size_t half = n_leaves / arity;  // layers above the first ping-pong between work[0 .. half) and work[half .. 2 half)
  const bool uses_work = half > 1;
  CSH_REQUIRE(leaves_dev && root_dev && (work_dev || !uses_work), "poseidon2_merkle: NULL argument");
  FrRanges in, out;
  in.add(leaves_dev, 32 * n_leaves);
  out.add(root_dev, 32);
  if (uses_work) out.add(work_dev, 32 * 2 * half);
  CSH_TRY(fr_check_ranges(in, out, "poseidon2_merkle"));
  CSH_TRY(ensure_device());
  const P2Params* h;
  CSH_TRY(p2_handle(handle, &h, "poseidon2_merkle"));
  return FR_CALL(h->field, p2_merkle_t<F>(h, arity, mode, leaves_dev, n_leaves, root_dev, work_dev, resolve_stream(stream)));
}

int csh_poseidon2_co_round_dev(csh_curve_t field_of, uint32_t protocol, uint32_t party_id, csh_poseidon2_params_t handle, uint32_t step,
                               uint64_t* state_dev, size_t n_perm, const uint64_t* y_dev, const uint64_t* const* precomp_dev, size_t precomp_offset,
                               uint64_t* open_dev, uint64_t* ff_out_dev, void* stream) {
  CSH_REQUIRE(handle, "poseidon2_co_round: the parameter handle is NULL");
  const P2Params* h0 = reinterpret_cast<const P2Params*>(handle);
  CSH_TRY(p2_check_co(field_of, protocol, party_id, h0, step, state_dev, n_perm, y_dev, precomp_dev, precomp_offset, open_dev, ff_out_dev));
  if (!n_perm) return CSH_OK;
  CSH_TRY(ensure_device());
  const P2Params* h;
  CSH_TRY(p2_handle(handle, &h, "poseidon2_co_round"));
  return FR_CALL(field_of, [&]() -> int {
    P2CoArgs<F> a;
    a.state = (F*)state_dev, a.y = (const F*)y_dev, a.open = (F*)open_dev, a.ff_out = step == 0 ? (F*)ff_out_dev : nullptr;
    for (int k = 0; k < 5; ++k) a.pre[k] = (const F*)precomp_dev[k];
    a.n_perm = n_perm, a.pre_off = precomp_offset, a.step = step, a.ncomp = protocol + 1, a.pub_comp = pq_pub_comp(protocol, party_id);
    return p2_co_round_t<F>(h, a, resolve_stream(stream));
  }());
}

int csh_poseidon2_layer_next_dev(csh_curve_t field_of, uint32_t ncomp, uint32_t t, uint32_t arity, uint32_t mode, const uint64_t* state_dev,
                                 const uint64_t* ff_dev, uint64_t* next_dev, size_t len, void* stream) {
  CSH_TRY(p2_check_next(field_of, ncomp, t, arity, mode, state_dev, ff_dev, next_dev, len));
  CSH_TRY(ensure_device());
  return FR_CALL(field_of, p2_next_t<F>(P2NextArgs<F>{(const F*)state_dev, mode == (uint32_t)P2_COMPRESSION ? (const F*)ff_dev : nullptr, (F*)next_dev,
                                                       len, ncomp, t, arity},
                                        resolve_stream(stream)));
}

}  // extern "C"
