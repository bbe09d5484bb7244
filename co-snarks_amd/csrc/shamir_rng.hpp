// The DN07 double-sharing stages of ShamirRng (mpc-core/src/protocols/shamir/rngs.rs:334-428) as public linear maps of draw vectors:
// the schedule of the draws, the small matrices and the per-element function that the kernel of shamir_rng.hip and the host self-test
// (csh_selftest_shamir_rng_host) share. DESIGN.md section 3.3l.
//
// random_double_share(amount) for party `id` of n with threshold t, in the reference's order (rngs.rs:344-384). A "batch" is `amount`
// consecutive F::rand draws of one shared stream (get_rng_mut: stream `other` for other < id, `other - 1` for other > id):
//   degree d = t + 1, then d = 2 t, each:
//     receive_seeded_next(d)   for i = 1 .. d, sender s = (id - i) mod n, s > id:  a batch of stream s  -> column s of rcv
//     the sender's draws       for i = 1 .. d, receiver r = (id + i) mod n:        a batch of stream r  -> share i - 1 (t) / share i (2t)
//     receive_seeded_prev(d)   for i = 1 .. d, sender s = (id - i) mod n, s < id:  a batch of stream s  -> column s of rcv
// A stream's batches follow each other in the stream whatever lies between them in this order, so one csh_field_rand_dev-style call per
// stream draws all of them and batch q of the stream is elements [q amount, (q + 1) amount) of its region.
// Everything else is linear and public. With L_j the Lagrange basis over the points of precompute_interpolation_polys
// (t: (id + i) mod n + 1, i = 1 .. t + 1; 2t: 0, then (id + i) mod n + 1, i = 1 .. 2 t), interpolate_poly_from_precomputed followed by
// evaluate_poly at x is sum_j share_j L_j(x), so
//   rands = p[0] = sum_j share_j L_j(0), own evaluation x = id + 1, the wire vectors x = receiver + 1 (send_share_of_randomness),
// and buffer_triples' matmul is the (t + 1) x n Vandermonde matrix over the n columns of rcv (seeded batches, the own evaluation,
// received vectors). The reference's coefficient form and this evaluation form are the same field elements: both are exact.
//
// Arithmetic: the exact canonical field (F::mul, F::add) as in honk_co_relations -- no lazy limbs, so no limb bound to derive; a sum of
// at most SHAMIR_MAX_PARTIES canonical products, canonical after every step.
#pragma once
#include <string.h>

#include <vector>

#include "common.hpp"
#include "field.hpp"

namespace csh {

constexpr int SHAMIR_MAX_PARTIES = 16;  // a limit of this library: the matrices are at most 16 x 16 and go to the kernel as they are
constexpr int SM_ROWS = 4;              // rows a lane accumulates in registers (4 x 8 limbs); blockIdx.y = the row tile
constexpr size_t SHAMIR_MAX_AMOUNT = size_t(1) << 24;  // batch items of one call: a stream draws at most 4 batches of them (<= 2^26 <= FR_MAX_N)

// out[r][i ostride] = sum_k mat[r K + k] in[k][i] for r < R, i < n. mat lives in device memory.
template <class F>
struct SmArgs {
  const F* in[SHAMIR_MAX_PARTIES];
  F* out[SHAMIR_MAX_PARTIES];
  const F* mat;
  uint32_t K, R;
  size_t ostride, n;
};
template <class F>
CSH_HD void shamir_matmul_at(const SmArgs<F>& a, uint32_t row_tile, size_t i) {
  const uint32_t r0 = row_tile * SM_ROWS;
  F acc[SM_ROWS];
#pragma unroll
  for (int q = 0; q < SM_ROWS; ++q) acc[q] = F::zero();
  for (uint32_t k = 0; k < a.K; ++k) {
    const F x = a.in[k][i];
#pragma unroll
    for (int q = 0; q < SM_ROWS; ++q)
      if (r0 + q < a.R) acc[q] = F::add(acc[q], F::mul(x, a.mat[(size_t)(r0 + q) * a.K + k]));
  }
#pragma unroll
  for (int q = 0; q < SM_ROWS; ++q)
    if (r0 + q < a.R) a.out[r0 + q][i * a.ostride] = acc[q];
}

// ---- the schedule (host) -------------------------------------------------------------------------------------------------------------------
struct ShamirBatch {
  uint32_t stream;  // index into the n - 1 shared streams
  uint32_t slot;    // the stream's slot-th batch of the call
};
struct ShamirSchedule {
  uint32_t n, t, id;
  uint32_t per_stream[SHAMIR_MAX_PARTIES];        // batches each shared stream draws in one double share
  // degree index 0 = t, 1 = 2t
  int col[2][SHAMIR_MAX_PARTIES];                 // column j of rcv: >= 0 a batch index into `batches`, -1 the own evaluation, -2 - w the w-th received vector of the block
  int share[2][SHAMIR_MAX_PARTIES];               // the sender's draws: share[0][0 .. t], share[1][1 .. 2t] (share[1][0] is rands)
  uint32_t send_to[2][SHAMIR_MAX_PARTIES], n_send[2];  // receivers in wire order
  std::vector<ShamirBatch> batches;
};
inline uint32_t shamir_stream_of(uint32_t id, uint32_t other) { return other < id ? other : other - 1; }
inline ShamirSchedule shamir_schedule(uint32_t n, uint32_t t, uint32_t id) {
  ShamirSchedule s;
  s.n = n, s.t = t, s.id = id;
  for (uint32_t j = 0; j < SHAMIR_MAX_PARTIES; ++j) s.per_stream[j] = 0;
  auto batch = [&](uint32_t other) {
    const uint32_t st = shamir_stream_of(id, other);
    s.batches.push_back(ShamirBatch{st, s.per_stream[st]++});
    return (int)s.batches.size() - 1;
  };
  for (int d = 0; d < 2; ++d) {
    const uint32_t deg = d == 0 ? t + 1 : 2 * t;
    for (uint32_t j = 0; j < SHAMIR_MAX_PARTIES; ++j) s.col[d][j] = s.share[d][j] = -1;
    for (uint32_t i = 1; i <= deg; ++i)  // receive_seeded_next
      if (const uint32_t snd = (id + n - i) % n; snd > id) s.col[d][snd] = batch(snd);
    for (uint32_t i = 1; i <= deg; ++i) s.share[d][d == 0 ? i - 1 : i] = batch((id + i) % n);
    for (uint32_t i = 1; i <= deg; ++i)  // receive_seeded_prev
      if (const uint32_t snd = (id + n - i) % n; snd < id) s.col[d][snd] = batch(snd);
    // send_share_of_randomness / receive_share_of_randomness with seeded = deg
    s.n_send[d] = n - deg - 1;
    for (uint32_t i = 1; i <= s.n_send[d]; ++i) {
      s.send_to[d][i - 1] = (id + i + deg) % n;
      s.col[d][(id + n - deg - i) % n] = -2 - (int)(i - 1);
    }
  }
  return s;
}

// ---- the matrices (host) -------------------------------------------------------------------------------------------------------------------
// L_j(x) over the points xs[0 .. m): prod_(k != j) (x - xs[k]) / (xs[j] - xs[k])
template <class F>
inline F shamir_lagrange_at(const uint32_t* xs, uint32_t m, uint32_t j, uint32_t x) {
  F num = F::one(), den = F::one();
  const F xf = F::from_u64(x), xj = F::from_u64(xs[j]);
  for (uint32_t k = 0; k < m; ++k) {
    if (k == j) continue;
    const F xk = F::from_u64(xs[k]);
    num = F::mul(num, F::sub(xf, xk));
    den = F::mul(den, F::sub(xj, xk));
  }
  return F::mul(num, F::inv(den));
}
// The three matrices of a party, row-major, back to back:
//   M_t   (2 + n_send[0]) x (t + 1):  rows = own evaluation, rands, one per receiver of the t block
//   M_2t  (1 + n_send[1]) x (2t + 1): rows = own evaluation, one per receiver of the 2t block
//   V     (t + 1) x n:                create_vandermonde_matrix, V[r][c] = (c + 1)^r
template <class F>
struct ShamirMatrices {
  std::vector<F> m;
  size_t off_t = 0, off_2t = 0, off_v = 0;
  uint32_t rows_t = 0, rows_2t = 0;
};
template <class F>
inline ShamirMatrices<F> shamir_matrices(const ShamirSchedule& s) {
  ShamirMatrices<F> o;
  const uint32_t n = s.n, t = s.t, id = s.id;
  uint32_t xs[SHAMIR_MAX_PARTIES + 1];
  // degree t: the points of the t + 1 seeded receivers
  for (uint32_t i = 1; i <= t + 1; ++i) xs[i - 1] = (id + i) % n + 1;
  o.rows_t = 2 + s.n_send[0];
  o.off_t = o.m.size();
  for (uint32_t r = 0; r < o.rows_t; ++r) {
    const uint32_t x = r == 0 ? id + 1 : r == 1 ? 0 : s.send_to[0][r - 2] + 1;
    for (uint32_t j = 0; j <= t; ++j) o.m.push_back(shamir_lagrange_at<F>(xs, t + 1, j, x));
  }
  // degree 2t: 0 (my randomness is the secret), then the 2t seeded receivers
  xs[0] = 0;
  for (uint32_t i = 1; i <= 2 * t; ++i) xs[i] = (id + i) % n + 1;
  o.rows_2t = 1 + s.n_send[1];
  o.off_2t = o.m.size();
  for (uint32_t r = 0; r < o.rows_2t; ++r) {
    const uint32_t x = r == 0 ? id + 1 : s.send_to[1][r - 1] + 1;
    for (uint32_t j = 0; j <= 2 * t; ++j) o.m.push_back(shamir_lagrange_at<F>(xs, 2 * t + 1, j, x));
  }
  o.off_v = o.m.size();
  for (uint32_t r = 0; r <= t; ++r)
    for (uint32_t c = 1; c <= n; ++c) o.m.push_back(F::pow_u64(F::from_u64(c), r));
  return o;
}

// ---- the stages' arguments (host) ----------------------------------------------------------------------------------------------------------
// element offsets inside a call's work area: the draws (the streams' regions follow each other, a stream's batches follow each other),
// the own evaluations of degree t and 2t, rands
struct ShamirWork {
  size_t draws, own[2], rands, total;
  ShamirWork(const ShamirSchedule& s, size_t amount) {
    draws = 0;
    own[0] = s.batches.size() * amount, own[1] = own[0] + amount, rands = own[1] + amount, total = rands + amount;
  }
};
inline size_t shamir_batch_offset(const ShamirSchedule& s, int b, size_t amount) {
  size_t off = 0;
  for (uint32_t q = 0; q < s.batches[b].stream; ++q) off += s.per_stream[q] * amount;
  return off + s.batches[b].slot * amount;
}
// d = 0: polys_t at id + 1, at 0 (rands) and at the receivers of the t block; d = 1: polys_2t (share 0 = rands) at id + 1 and at the
// receivers of the 2t block. mat: M_t or M_2t, rows: its row count; send: the wire vectors, t block then 2t block.
template <class F>
inline SmArgs<F> shamir_local_args(const ShamirSchedule& s, int d, const F* mat, uint32_t rows, F* work, size_t amount, F* send) {
  const ShamirWork w(s, amount);
  SmArgs<F> a;
  memset(&a, 0, sizeof a);
  a.K = d == 0 ? s.t + 1 : 2 * s.t + 1, a.R = rows, a.mat = mat, a.ostride = 1, a.n = amount;
  for (uint32_t j = 0; j < a.K; ++j) a.in[j] = d == 1 && j == 0 ? work + w.rands : work + shamir_batch_offset(s, s.share[d][j], amount);
  a.out[0] = work + w.own[d];
  if (d == 0) a.out[1] = work + w.rands;
  for (uint32_t q = 0; q < s.n_send[d]; ++q) a.out[(d == 0 ? 2 : 1) + q] = send + ((d ? s.n_send[0] : 0) + q) * amount;
  return a;
}
// the Vandermonde matrix over the n columns of rcv_t (d = 0) or rcv_2t (d = 1); out: where the amount * (t + 1) new elements begin,
// batch item b at [b (t + 1), (b + 1) (t + 1)) (chunks_exact_mut(size))
template <class F>
inline SmArgs<F> shamir_finish_args(const ShamirSchedule& s, int d, const F* mat_v, F* work, size_t amount, const F* recv, F* out) {
  const ShamirWork w(s, amount);
  SmArgs<F> a;
  memset(&a, 0, sizeof a);
  a.K = s.n, a.R = s.t + 1, a.mat = mat_v, a.ostride = s.t + 1, a.n = amount;
  for (uint32_t j = 0; j < s.n; ++j) {
    const int c = s.col[d][j];
    a.in[j] = c >= 0 ? work + shamir_batch_offset(s, c, amount) : c == -1 ? work + w.own[d] : recv + ((d ? s.n_send[0] : 0) + (size_t)(-2 - c)) * amount;
  }
  for (uint32_t r = 0; r <= s.t; ++r) a.out[r] = out + r;
  return a;
}

inline const char* shamir_params_refusal(uint32_t id, uint32_t n, uint32_t t) {
  if (n > SHAMIR_MAX_PARTIES) return "shamir_rng: num_parties exceeds 16, the limit of this library";
  if (t < 1 || 2 * t + 1 > n) return "shamir_rng: threshold must be at least 1 and 2 * threshold + 1 <= num_parties";
  if (id >= n) return "shamir_rng: id must be below num_parties";
  return nullptr;
}

}  // namespace csh
