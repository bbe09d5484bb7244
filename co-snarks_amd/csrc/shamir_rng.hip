// DN07 double sharings on the device: the csh_shamir_rng_t handle and the two stream-ordered stages either
// side of the one network exchange of ShamirRng::random_double_share + buffer_triples (mpc-core/src/protocols/shamir/rngs.rs:334-428).
//   csh_shamir_double_share_local_dev   the draws (one F::rand stream call per shared stream: field_rand.hip), then polys_t, rands,
//                                       polys_2t, the own evaluations and the wire vectors as two launches of k_shamir_matmul;
//   csh_shamir_double_share_finish_dev  the Vandermonde matrix over the n columns of rcv_t and of rcv_2t: two launches, strided output
//                                       straight into the handle's buffers (the per-item rows rcv[b][0 .. n) are never stored);
//   csh_shamir_pairs_take_dev           get_pair's pops from the back / fork_with_pairs' drain from the front: k_shamir_take.
// k_shamir_matmul is the multi-output form of k_lincomb: a small dense public matrix in device memory times column vectors; a lane owns
// one element index and SM_ROWS rows (blockIdx.y = the row tile), grid-stride over the elements, 256 lanes, no LDS, tune "vec_max_blocks".
// The schedule, the matrices and the per-element function are shamir_rng.hpp, shared with the host self-test.
#include "shamir_rng.hpp"

#include <array>

#include "field_rand.hpp"
#include "fr_entry.hpp"

namespace csh {

template <class F>
int field_rand_t(const uint8_t* seed, uint64_t cand_begin, size_t n, uint64_t* out, uint64_t* cand_end, hipStream_t st);  // field_rand.hip

constexpr int SM_WG = 256;

template <class F>
__global__ __launch_bounds__(SM_WG) void k_shamir_matmul(SmArgs<F> a) {
  for (size_t i = blockIdx.x * (size_t)SM_WG + threadIdx.x; i < a.n; i += (size_t)gridDim.x * SM_WG) shamir_matmul_at(a, blockIdx.y, i);
}
// out element i = buffer element (from_front ? i : len - 1 - i), for both buffers
template <class F>
__global__ __launch_bounds__(SM_WG) void k_shamir_take(const F* r_t, const F* r_2t, size_t len, size_t count, int from_front, F* out_t, F* out_2t) {
  for (size_t i = blockIdx.x * (size_t)SM_WG + threadIdx.x; i < count; i += (size_t)gridDim.x * SM_WG) {
    const size_t src = from_front ? i : len - 1 - i;
    out_t[i] = r_t[src];
    out_2t[i] = r_2t[src];
  }
}

template <class F>
static int sm_launch(const SmArgs<F>& a, hipStream_t st) {
  if (a.n == 0 || a.R == 0) return CSH_OK;
  hipLaunchKernelGGL(k_shamir_matmul<F>, dim3(fr_stream_grid(a.n, SM_WG), (a.R + SM_ROWS - 1) / SM_ROWS), dim3(SM_WG), 0, st, a);
  CSH_HIP(hipGetLastError());
  return CSH_OK;
}

}  // namespace csh

using namespace csh;

struct csh_shamir_rng_s {
  csh_curve_t field;
  uint32_t id, n, t;
  int device;
  ShamirSchedule sched;
  std::vector<std::array<uint8_t, 32>> seeds;  // the n - 1 shared streams of get_shared_rngs
  std::vector<uint64_t> pos;                   // ... and their positions, in candidates
  uint64_t* mats = nullptr;                    // device: M_t, M_2t, V (shamir_rng.hpp)
  size_t off_t = 0, off_2t = 0, off_v = 0;     // in elements
  uint32_t rows_t = 0, rows_2t = 0;
  // r_t / r_2t: elements [head, head + len) of two device arrays of `cap` elements
  uint64_t *r_t = nullptr, *r_2t = nullptr;
  size_t head = 0, len = 0, cap = 0;
  // between local and finish: the draws (batches x amount), own evaluations t | 2t, rands
  uint64_t* work = nullptr;
  size_t work_cap = 0, pending = 0;
};

namespace csh {

static int shamir_check_device(csh_shamir_rng_t h, const char* what) {
  int cur = -1;
  CSH_HIP(hipGetDevice(&cur));
  if (cur != h->device) {
    set_error("%s: the handle lives on device %d, the calling thread is on device %d", what, h->device, cur);
    return CSH_ERR_INVALID;
  }
  return CSH_OK;
}
// room for `extra` more elements behind the present ones; the present ones move to the front of a new allocation when it grows
static int shamir_reserve(csh_shamir_rng_t h, size_t extra, hipStream_t st) {
  if (h->head + h->len + extra <= h->cap) return CSH_OK;
  const size_t want = h->len + extra, cap = want + (want >> 1);
  uint64_t* nb[2] = {nullptr, nullptr};
  uint64_t* old[2] = {h->r_t, h->r_2t};
  for (int k = 0; k < 2; ++k) {
    CSH_HIP(hipMalloc((void**)&nb[k], cap * 32));
    if (h->len) CSH_HIP(hipMemcpyAsync(nb[k], old[k] + 4 * h->head, h->len * 32, hipMemcpyDeviceToDevice, st));
  }
  if (h->len) CSH_HIP(hipStreamSynchronize(st));
  for (int k = 0; k < 2; ++k)
    if (old[k]) CSH_HIP(hipFree(old[k]));
  h->r_t = nb[0], h->r_2t = nb[1], h->head = 0, h->cap = cap;
  return CSH_OK;
}
template <class F>
static int shamir_local_t(csh_shamir_rng_t h, size_t amount, uint64_t* send, hipStream_t st) {
  const ShamirSchedule& s = h->sched;
  const ShamirWork w(s, amount);
  if (h->work_cap < w.total) {
    if (h->work) CSH_HIP(hipFree(h->work));
    h->work = nullptr, h->work_cap = 0;
    CSH_HIP(hipMalloc((void**)&h->work, w.total * 32));
    h->work_cap = w.total;
  }
  F* base = (F*)h->work;
  // the draws: every shared stream's batches of this call in one go, the position advances
  size_t off = 0;
  for (uint32_t q = 0; q + 1 < s.n; ++q) {
    const size_t cnt = s.per_stream[q] * amount;
    if (cnt) CSH_TRY(field_rand_t<F>(h->seeds[q].data(), h->pos[q], cnt, (uint64_t*)(base + off), &h->pos[q], st));
    off += cnt;
  }
  const F* mats = (const F*)h->mats;
  CSH_TRY(sm_launch(shamir_local_args<F>(s, 0, mats + h->off_t, h->rows_t, base, amount, (F*)send), st));    // polys_t at id + 1, at 0 (rands), at the receivers
  CSH_TRY(sm_launch(shamir_local_args<F>(s, 1, mats + h->off_2t, h->rows_2t, base, amount, (F*)send), st));  // polys_2t (share 0 = rands) at id + 1, at the receivers
  h->pending = amount;
  return CSH_OK;
}

template <class F>
static int shamir_finish_t(csh_shamir_rng_t h, size_t amount, const uint64_t* recv, hipStream_t st) {
  const ShamirSchedule& s = h->sched;
  const size_t size = s.t + 1;
  CSH_TRY(shamir_reserve(h, amount * size, st));
  F* base = (F*)h->work;
  uint64_t* bufs[2] = {h->r_t, h->r_2t};
  for (int d = 0; d < 2; ++d)
    CSH_TRY(sm_launch(shamir_finish_args<F>(s, d, (const F*)h->mats + h->off_v, base, amount, (const F*)recv, (F*)bufs[d] + h->head + h->len), st));
  h->len += amount * size;
  h->pending = 0;
  return CSH_OK;
}

template <class F>
static int shamir_take_t(csh_shamir_rng_t h, size_t count, int from_front, uint64_t* out_t, uint64_t* out_2t, hipStream_t st) {
  hipLaunchKernelGGL(k_shamir_take<F>, dim3(fr_stream_grid(count, SM_WG)), dim3(SM_WG), 0, st, (const F*)h->r_t + h->head, (const F*)h->r_2t + h->head,
                     h->len, count, from_front, (F*)out_t, (F*)out_2t);
  CSH_HIP(hipGetLastError());
  if (from_front) h->head += count;
  h->len -= count;
  if (h->len == 0) h->head = 0;  // an emptied buffer is refilled from its start (stream order keeps the take's reads ahead of the writes)
  return CSH_OK;
}

template <class F>
static int shamir_create_t(csh_shamir_rng_t h) {
  const ShamirMatrices<F> m = shamir_matrices<F>(h->sched);
  h->off_t = m.off_t, h->off_2t = m.off_2t, h->off_v = m.off_v, h->rows_t = m.rows_t, h->rows_2t = m.rows_2t;
  CSH_HIP(hipMalloc((void**)&h->mats, m.m.size() * sizeof(F)));
  CSH_HIP(hipMemcpy(h->mats, m.m.data(), m.m.size() * sizeof(F), hipMemcpyHostToDevice));
  return CSH_OK;
}

}  // namespace csh

extern "C" {

int csh_shamir_rng_create(csh_curve_t field_of, uint32_t id, uint32_t num_parties, uint32_t threshold, const uint8_t* seeds, const uint64_t* positions,
                          csh_shamir_rng_t* handle) {
  FR_REQUIRE_FIELD(field_of);
  CSH_REQUIRE(handle && seeds, "shamir_rng_create: NULL argument");
  *handle = nullptr;
  if (const char* why = shamir_params_refusal(id, num_parties, threshold)) {
    set_error("%s", why);
    return CSH_ERR_INVALID;
  }
  for (uint32_t q = 0; positions && q + 1 < num_parties; ++q) CSH_REQUIRE(positions[q] <= FRD_MAX_CAND, "shamir_rng_create: a stream position exceeds 2^62");
  CSH_TRY(ensure_device());
  csh_shamir_rng_s* h = new csh_shamir_rng_s();
  h->field = field_of, h->id = id, h->n = num_parties, h->t = threshold;
  h->sched = shamir_schedule(num_parties, threshold, id);
  h->seeds.resize(num_parties - 1);
  h->pos.assign(num_parties - 1, 0);
  for (uint32_t q = 0; q + 1 < num_parties; ++q) {
    memcpy(h->seeds[q].data(), seeds + 32 * q, 32);
    if (positions) h->pos[q] = positions[q];
  }
  int rc = hipGetDevice(&h->device) == hipSuccess ? CSH_OK : CSH_ERR_HIP;
  if (rc == CSH_OK) rc = FR_CALL(field_of, shamir_create_t<F>(h));
  if (rc != CSH_OK) {
    if (h->mats) (void)hipFree(h->mats);
    delete h;
    return rc;
  }
  *handle = h;
  return CSH_OK;
}

int csh_shamir_rng_destroy(csh_shamir_rng_t h) {
  if (!h) return CSH_OK;
  for (void* p : {(void*)h->mats, (void*)h->r_t, (void*)h->r_2t, (void*)h->work})
    if (p) (void)hipFree(p);
  delete h;
  return CSH_OK;
}

int csh_shamir_rng_positions(csh_shamir_rng_t h, uint64_t* positions) {
  CSH_REQUIRE(h && positions, "shamir_rng_positions: NULL argument");
  for (size_t q = 0; q < h->pos.size(); ++q) positions[q] = h->pos[q];
  return CSH_OK;
}

int csh_shamir_rng_fork_seeds(csh_shamir_rng_t h, uint8_t* seeds_out) {
  CSH_REQUIRE(h && seeds_out, "shamir_rng_fork_seeds: NULL argument");
  for (size_t q = 0; q < h->pos.size(); ++q) {
    uint32_t key[8], words[16];
    memcpy(key, h->seeds[q].data(), 32);
    chacha12_block(key, h->pos[q] >> 1, words);
    memcpy(seeds_out + 32 * q, words + 8 * (h->pos[q] & 1), 32);
    h->pos[q] += 1;
  }
  return CSH_OK;
}

int csh_shamir_pairs_len(csh_shamir_rng_t h, size_t* len) {
  CSH_REQUIRE(h && len, "shamir_pairs_len: NULL argument");
  *len = h->len;
  return CSH_OK;
}

int csh_shamir_double_share_local_dev(csh_shamir_rng_t h, size_t amount, uint64_t* send_dev, void* stream) {
  CSH_REQUIRE(h, "shamir_double_share_local: NULL handle");
  CSH_REQUIRE(amount >= 1 && amount <= SHAMIR_MAX_AMOUNT, "shamir_double_share_local: amount must be 1 .. 2^24");
  CSH_REQUIRE(send_dev || h->sched.n_send[0] + h->sched.n_send[1] == 0, "shamir_double_share_local: send_dev is NULL but this party sends");
  CSH_REQUIRE(h->pending == 0, "shamir_double_share_local: the previous local stage has not been finished");
  CSH_TRY(ensure_device());
  CSH_TRY(shamir_check_device(h, "shamir_double_share_local"));
  hipStream_t st = resolve_stream(stream);
  return FR_CALL(h->field, shamir_local_t<F>(h, amount, send_dev, st));
}

int csh_shamir_double_share_finish_dev(csh_shamir_rng_t h, size_t amount, const uint64_t* recv_dev, void* stream) {
  CSH_REQUIRE(h, "shamir_double_share_finish: NULL handle");
  CSH_REQUIRE(h->pending != 0 && amount == h->pending, "shamir_double_share_finish: amount is not that of the local stage before it");
  CSH_REQUIRE(recv_dev || h->sched.n_send[0] + h->sched.n_send[1] == 0, "shamir_double_share_finish: recv_dev is NULL but this party receives");
  CSH_TRY(ensure_device());
  CSH_TRY(shamir_check_device(h, "shamir_double_share_finish"));
  hipStream_t st = resolve_stream(stream);
  return FR_CALL(h->field, shamir_finish_t<F>(h, amount, recv_dev, st));
}

int csh_shamir_pairs_take_dev(csh_shamir_rng_t h, size_t count, int from_front, uint64_t* r_t_out_dev, uint64_t* r_2t_out_dev, void* stream) {
  CSH_REQUIRE(h, "shamir_pairs_take: NULL handle");
  if (count > h->len) {
    set_error("shamir_pairs_take: %zu pairs asked for, %zu present (refilling is the caller's decision)", count, h->len);
    return CSH_ERR_INVALID;
  }
  if (count == 0) return CSH_OK;
  CSH_REQUIRE(r_t_out_dev && r_2t_out_dev, "shamir_pairs_take: NULL output");
  CSH_TRY(ensure_device());
  CSH_TRY(shamir_check_device(h, "shamir_pairs_take"));
  hipStream_t st = resolve_stream(stream);
  return FR_CALL(h->field, shamir_take_t<F>(h, count, from_front, r_t_out_dev, r_2t_out_dev, st));
}

}
