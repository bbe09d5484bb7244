// F::rand over a ChaCha12 stream on the device: csh_field_rand_dev writes the first n accepted candidates at or
// after a stream position, in order. Rejection makes element i's place in the keystream depend on every draw before it, so this is a
// stable compaction of the k_hc_sel_count / _scan / _write kind (honk_co_relations.hip) over a window of candidates:
//   k_frd_count  every workgroup owns a contiguous chunk of ChaCha blocks, a lane computes one block (two candidates) per tile and the
//                workgroup adds its accepted candidates through LDS;
//   k_frd_scan   one workgroup: the chunks' offsets and the window's total; a window that falls short also gets its end reported here;
//   k_frd_write  recomputes the candidates (half a ChaCha12 block is a few hundred integer operations, against 64 bytes through HBM per
//                stored candidate: the rule of CoPoint) and writes the accepted ones behind the chunk's offset with a ballot scan. The
//                lane that writes the last wanted element reports its candidate index: one writer, no atomics.
// No atomics anywhere and the output words do not depend on the launch shape: tune "vec_max_blocks" (the grid cap) and
// "field_rand_window" (candidates per window) change the decomposition only. The per-candidate function and the window plan are
// field_rand.hpp, shared with the host self-test.
#include "field_rand.hpp"

#include "fr_entry.hpp"

namespace csh {

// the two candidates of block `blk`: acc[h] = accepted and inside the window
template <class F>
__device__ __forceinline__ void frd_block(const FrdWindow& w, uint64_t blk, bool valid, F c[2], bool acc[2]) {
  uint32_t words[16];
  chacha12_block(w.key, blk, words);
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const uint64_t k = 2 * blk + h;
    const bool ok = field_rand_candidate<F>(words, h, c[h]);
    acc[h] = valid && ok && k >= w.cand_lo && k < w.cand_hi;
  }
}

template <class F>
__global__ __launch_bounds__(FRD_WG) void k_frd_count(FrdWindow w, uint32_t* counts) {
  __shared__ uint32_t part[FRD_WG];
  const uint64_t lo = w.blk_lo + blockIdx.x * w.chunk, hi = lo + w.chunk < w.blk_hi ? lo + w.chunk : w.blk_hi;
  uint32_t c = 0;
#pragma unroll 1
  for (uint64_t blk = lo + threadIdx.x; blk < hi; blk += FRD_WG) {
    F v[2];
    bool acc[2];
    frd_block<F>(w, blk, true, v, acc);
    c += (acc[0] ? 1u : 0u) + (acc[1] ? 1u : 0u);
  }
  part[threadIdx.x] = c;
  __syncthreads();
  for (int s = FRD_WG / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) counts[blockIdx.x] = part[0];
}

// one workgroup of FRD_MAX_BLOCKS lanes: offsets[b] = the accepted candidates in front of chunk b; res[0] = all of the window's. When
// they are fewer than `need`, every candidate of the window is consumed and res[1] = cand_hi; otherwise k_frd_write reports res[1].
__global__ __launch_bounds__(FRD_MAX_BLOCKS) void k_frd_scan(const uint32_t* counts, uint32_t blocks, uint64_t need, uint64_t cand_hi,
                                                            uint32_t* offsets, uint64_t* res) {
  __shared__ uint32_t s[FRD_MAX_BLOCKS];
  const uint32_t t = threadIdx.x, own = t < blocks ? counts[t] : 0u;
  s[t] = own;
  __syncthreads();
  for (uint32_t d = 1; d < FRD_MAX_BLOCKS; d <<= 1) {
    const uint32_t v = t >= d ? s[t - d] : 0u;
    __syncthreads();
    s[t] += v;
    __syncthreads();
  }
  if (t < blocks) offsets[t] = s[t] - own;
  if (t == FRD_MAX_BLOCKS - 1) {
    res[0] = s[t];
    if ((uint64_t)s[t] < need) res[1] = cand_hi;
  }
}

template <class F>
__global__ __launch_bounds__(FRD_WG) void k_frd_write(FrdWindow w, const uint32_t* offsets, F* out, uint64_t* res) {
  __shared__ uint32_t wave_total[FRD_WG / 64];
  const uint64_t lo = w.blk_lo + blockIdx.x * w.chunk, hi = lo + w.chunk < w.blk_hi ? lo + w.chunk : w.blk_hi;
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint64_t base = offsets[blockIdx.x];
#pragma unroll 1
  for (uint64_t tile = lo; tile < hi; tile += FRD_WG) {  // uniform over the workgroup
    if (base >= w.need) break;                           // uniform too: nothing of this chunk is wanted any more
    const uint64_t blk = tile + threadIdx.x;
    F v[2];
    bool acc[2];
    frd_block<F>(w, blk, blk < hi, v, acc);
    // candidate order inside a wave: lane 0 half 0, lane 0 half 1, lane 1 half 0, ...
    const unsigned long long b0 = __ballot(acc[0]), b1 = __ballot(acc[1]), lt = (1ull << lane) - 1ull;
    const uint32_t before = (uint32_t)(__popcll(b0 & lt) + __popcll(b1 & lt));
    if (lane == 0) wave_total[wave] = (uint32_t)(__popcll(b0) + __popcll(b1));
    __syncthreads();
    uint32_t in_front = 0, all = 0;
#pragma unroll
    for (unsigned q = 0; q < FRD_WG / 64; ++q) {
      in_front += q < wave ? wave_total[q] : 0u;
      all += wave_total[q];
    }
    uint64_t pos = base + in_front + before;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      if (acc[h]) {
        if (pos < w.need) out[pos] = v[h];
        if (pos + 1 == w.need) res[1] = 2 * blk + h + 1;  // the one lane that holds the last wanted draw
        ++pos;
      }
    }
    base += all;
    __syncthreads();  // wave_total is rewritten by the next tile
  }
}

static int frd_grid_cap() {
  int mb = tune().vec_max_blocks.load(std::memory_order_relaxed);
  return (mb <= 0 || mb > FRD_MAX_BLOCKS) ? FRD_MAX_BLOCKS : mb;
}
static uint64_t frd_window_cap() {
  const int v = tune().field_rand_window.load(std::memory_order_relaxed);
  return field_rand_window_ok(v) ? (uint64_t)v : 0;  // csh_tune_set refuses other values; the environment is not validated
}

// The windows of one call. Reads two words back per window: the stream is synchronised once per window (one window, but for a
// shortfall of eight standard deviations or a shrunk "field_rand_window").
template <class F>
int field_rand_t(const uint8_t* seed, uint64_t cand_begin, size_t n, uint64_t* out, uint64_t* cand_end, hipStream_t st) {
  const double rate = field_rand_rate<F>();
  const int cap = frd_grid_cap();
  const uint64_t wcap = frd_window_cap();
  Arena& ar = arena_for(st);
  CSH_TRY(ar.reserve(2 * Arena::padded(FRD_MAX_BLOCKS * 4) + Arena::padded(16)));
  uint32_t* counts = ar.take<uint32_t>(FRD_MAX_BLOCKS);
  uint32_t* offsets = ar.take<uint32_t>(FRD_MAX_BLOCKS);
  uint64_t* res = ar.take<uint64_t>(2);
  uint64_t pos = cand_begin;
  size_t done = 0;
  while (done < n) {
    const uint64_t need = n - done;
    const FrdWindow w = field_rand_plan(seed, pos, field_rand_window_cands(need, rate, wcap), need, cap);
    hipLaunchKernelGGL(k_frd_count<F>, dim3(w.blocks), dim3(FRD_WG), 0, st, w, counts);
    hipLaunchKernelGGL(k_frd_scan, dim3(1), dim3(FRD_MAX_BLOCKS), 0, st, (const uint32_t*)counts, w.blocks, need, w.cand_hi, offsets, res);
    hipLaunchKernelGGL(k_frd_write<F>, dim3(w.blocks), dim3(FRD_WG), 0, st, w, (const uint32_t*)offsets, (F*)out + done, res);
    CSH_HIP(hipGetLastError());
    uint64_t back[2] = {0, 0};
    CSH_HIP(hipMemcpyAsync(back, res, sizeof back, hipMemcpyDeviceToHost, st));
    CSH_HIP(hipStreamSynchronize(st));
    if (back[1] <= pos || back[1] > w.cand_hi) {
      set_error("field_rand: the window [%llu, %llu) reported the position %llu", (unsigned long long)pos, (unsigned long long)w.cand_hi,
                (unsigned long long)back[1]);
      return CSH_ERR_HIP;
    }
    done += back[0] < need ? (size_t)back[0] : (size_t)need;
    pos = back[1];
  }
  if (cand_end) *cand_end = pos;
  return CSH_OK;
}
template int field_rand_t<Bn254Fr>(const uint8_t*, uint64_t, size_t, uint64_t*, uint64_t*, hipStream_t);
template int field_rand_t<Bls381Fr>(const uint8_t*, uint64_t, size_t, uint64_t*, uint64_t*, hipStream_t);
template int field_rand_t<Bls377Fr>(const uint8_t*, uint64_t, size_t, uint64_t*, uint64_t*, hipStream_t);

}  // namespace csh

using namespace csh;

extern "C" {

int csh_field_rand_dev(csh_curve_t field_of, const uint8_t seed[32], uint64_t cand_begin, size_t n, uint64_t* out_dev, uint64_t* cand_end, void* stream) {
  FR_REQUIRE_FIELD(field_of);
  FR_REQUIRE_N(n);
  CSH_REQUIRE(seed && (out_dev || n == 0), "field_rand: NULL argument");
  CSH_REQUIRE(cand_begin <= FRD_MAX_CAND, "field_rand: cand_begin exceeds 2^62");
  if (n == 0) {
    if (cand_end) *cand_end = cand_begin;
    return CSH_OK;
  }
  CSH_TRY(ensure_device());
  hipStream_t st = resolve_stream(stream);
  return FR_CALL(field_of, field_rand_t<F>(seed, cand_begin, n, out_dev, cand_end, st));
}

int csh_field_rand_plan(csh_curve_t field_of, size_t n, uint64_t cand_begin, uint64_t out[4]) {
  FR_REQUIRE_FIELD(field_of);
  FR_REQUIRE_N(n);
  CSH_REQUIRE(out && n > 0 && cand_begin <= FRD_MAX_CAND, "field_rand_plan: out is NULL, n is 0 or cand_begin exceeds 2^62");
  const uint8_t zero[32] = {0};
  double rate = 0.0;
  CSH_TRY(FR_CALL(field_of, (rate = field_rand_rate<F>(), CSH_OK)));
  const FrdWindow w = field_rand_plan(zero, cand_begin, field_rand_window_cands(n, rate, frd_window_cap()), n, frd_grid_cap());
  out[0] = w.cand_hi - w.cand_lo, out[1] = w.blocks, out[2] = 2 * w.chunk, out[3] = (uint64_t)(rate * 1e9);
  return CSH_OK;
}

}
