// Sort stage of the MSM: LDS counting sort of the signed-digit codes (see msm.hip for the pipeline).
#include <stdlib.h>

#include "msm_sort.hpp"

namespace csh {

// index written into the sorted list for flat position i of the digit array (identity unless merged-window mode)
__device__ __forceinline__ uint32_t entry_id(const MsmParams& p, size_t i) {
  if (p.remap_n == 0) return (uint32_t)i;
  const uint32_t f = (uint32_t)i;
  const uint32_t w = f / p.remap_n;
  return w * p.remap_stride + p.remap_off + (f - w * p.remap_n);
}

// Block (chunk ch, window w): LDS histogram of the chunk's digits -> blkcnt[w][ch][0..NB)
__global__ __launch_bounds__(SORT_BLK) void k_msm_hist_lds(MsmParams p, const uint16_t* __restrict__ dig, uint32_t* __restrict__ blkcnt,
                                                            uint32_t* __restrict__ part_cnt /* two-level mode: [w][ch][NB/256], else NULL */) {
  extern __shared__ uint32_t lds_cnt[];
  const uint32_t ch = blockIdx.x, w = blockIdx.y;
  for (uint32_t b = threadIdx.x; b < p.NB; b += SORT_BLK) lds_cnt[b] = 0;
  __syncthreads();
  const size_t lo = (size_t)ch * p.chunk_len;
  size_t hi = lo + p.chunk_len;
  if (hi > p.n) hi = p.n;
  const uint16_t* d = dig + (size_t)w * p.n;
  for (size_t i0 = lo; i0 < hi; i0 += 4 * SORT_BLK) {
    uint32_t code[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const size_t i = i0 + (size_t)k * SORT_BLK + threadIdx.x;
      code[k] = i < hi ? (uint32_t)d[i] : DIG_ZERO;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) (void)lds_slot(lds_cnt, code[k] & 0x7fffu, code[k] != DIG_ZERO);
  }
  __syncthreads();
  uint32_t* out = blkcnt + ((size_t)w * p.CH + ch) * p.NB;
  for (uint32_t b = threadIdx.x; b < p.NB; b += SORT_BLK) out[b] = lds_cnt[b];
  if (part_cnt) {  // entries of this chunk per partition of 256 adjacent buckets, straight from the LDS histogram (one wave each)
    const uint32_t P = p.NB / 256;
    const int lane = threadIdx.x & 63;
    for (uint32_t part = threadIdx.x >> 6; part < P; part += SORT_BLK / 64) {
      const uint32_t* c = lds_cnt + part * 256;
      uint32_t v = c[lane] + c[lane + 64] + c[lane + 128] + c[lane + 192];
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d);
      if (lane == 0) part_cnt[((size_t)w * p.CH + ch) * P + part] = v;
    }
  }
}

// Per (window, bucket): exclusive prefix over chunks (in place) and the bucket total -> hist[w][b+1]
__global__ __launch_bounds__(256) void k_msm_colscan(MsmParams p, uint32_t* __restrict__ blkcnt, uint32_t* __restrict__ hist) {
  const uint32_t w = blockIdx.y;
  const uint32_t b = blockIdx.x * 256 + threadIdx.x;
  if (b >= p.NB) return;
  // eight chunks per round: the loads of a round are issued together (a one-at-a-time walk paid one memory latency per chunk: 14 us)
  uint32_t acc = 0;
  uint32_t* col = blkcnt + (size_t)w * p.CH * p.NB + b;
  for (uint32_t ch0 = 0; ch0 < p.CH; ch0 += 8) {
    uint32_t t[8];
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j) t[j] = ch0 + j < p.CH ? col[(size_t)(ch0 + j) * p.NB] : 0u;
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j) {
      if (ch0 + j < p.CH) col[(size_t)(ch0 + j) * p.NB] = acc;
      acc += t[j];
    }
  }
  hist[(size_t)w * (p.NB + 2) + b + 1] = acc;
  if (b == 0) {  // the two border entries the scan reads as zero (no memset of the histogram per call)
    hist[(size_t)w * (p.NB + 2)] = 0;
    hist[(size_t)w * (p.NB + 2) + p.NB + 1] = 0;
  }
}

// One 1024-thread block per window. In: hist[w][0..NB+1] counts (index 0 and NB+1 unused = 0).
// Out: start[w][b] = first sorted slot of bucket b (start[w][NB+1] = total entries of the window) and
// nlanes[w] = ceil(total / L): the accumulate kernel cuts the sorted array into equal runs of L entries, one lane
// each, so every lane of a wave does the same number of mixed additions whatever the bucket sizes are.
// The counts are staged in LDS (coalesced loads / stores; each thread then walks its own contiguous run of counters in LDS, where
// the odd run length keeps the lanes on different banks) and the 1024 per-thread totals are scanned with wave shuffles + one
// LDS hop: 52 us -> ~10 us per launch at NB = 2^14 against the former strided global walk + 20-barrier Hillis-Steele scan.
__global__ __launch_bounds__(1024) void k_msm_scan(MsmParams p, uint32_t* hist, uint32_t* start, uint32_t* nlanes) {
  extern __shared__ uint32_t sc_lds[];  // len counters, then 16 wave totals
  const int w = blockIdx.x;
  const uint32_t len = p.NB + 2;
  uint32_t* h = hist + (size_t)w * len;
  uint32_t* st = start + (size_t)w * len;
  uint32_t* wave_tot = sc_lds + len;
  for (uint32_t b = threadIdx.x; b < len; b += 1024) sc_lds[b] = h[b];
  __syncthreads();
  const uint32_t per = (len + 1023) / 1024;
  const uint32_t b0 = threadIdx.x * per;
  uint32_t cnt = 0;
  for (uint32_t k = 0; k < per; ++k) {
    const uint32_t b = b0 + k;
    if (b < len) cnt += sc_lds[b];
  }
  // exclusive scan of cnt over the block: within the wave by shuffles, across the 16 waves through LDS
  uint32_t total;
  uint32_t run_c = block_excl_scan<16>(cnt, wave_tot, &total);  // exclusive prefix of this thread's run
  for (uint32_t k = 0; k < per; ++k) {
    const uint32_t b = b0 + k;
    if (b < len) {
      const uint32_t cv = sc_lds[b];
      sc_lds[b] = run_c;
      run_c += cv;
    }
  }
  __syncthreads();
  for (uint32_t b = threadIdx.x; b < len; b += 1024) {
    st[b] = sc_lds[b];
    h[b] = sc_lds[b];  // the same offsets again, as the global bucket cursors of the tile-parallel level-2 scatter (consumed by atomicAdd)
  }
  if (threadIdx.x == 0) nlanes[w] = (total + lane_len(p, w) - 1) / lane_len(p, w);
}

// Block (chunk ch, window w): LDS cursors = bucket start + this chunk's prefix; scatter (index | sign) into
// bucket order. No global atomics; the order inside a bucket is deterministic per chunk.
__global__ __launch_bounds__(SORT_BLK) void k_msm_scatter_lds(MsmParams p, const uint16_t* __restrict__ dig,
                                                               const uint32_t* __restrict__ start, const uint32_t* __restrict__ blkcnt,
                                                               uint32_t* __restrict__ sorted) {
  extern __shared__ uint32_t lds_cur[];
  const uint32_t ch = blockIdx.x, w = blockIdx.y;
  const uint32_t* st = start + (size_t)w * (p.NB + 2) + 1;
  const uint32_t* pre = blkcnt + ((size_t)w * p.CH + ch) * p.NB;
  for (uint32_t b = threadIdx.x; b < p.NB; b += SORT_BLK) lds_cur[b] = st[b] + pre[b];
  __syncthreads();
  const size_t lo = (size_t)ch * p.chunk_len;
  size_t hi = lo + p.chunk_len;
  if (hi > p.n) hi = p.n;
  const uint16_t* d = dig + (size_t)w * p.n;
  uint32_t* so = sorted + (size_t)w * p.n;
  for (size_t i0 = lo; i0 < hi; i0 += SORT_BLK) {
    const size_t i = i0 + threadIdx.x;
    uint32_t code = DIG_ZERO;
    if (i < hi) code = d[i];
    const bool valid = code != DIG_ZERO;
    const uint32_t pos = lds_slot(lds_cur, code & 0x7fffu, valid);
    if (valid) so[pos] = entry_id(p, i) | ((code >> 15) << 31);
  }
}


// ---- two-level scatter (large n): write-combining friendly ------------------------------------------------------
// A single-level scatter keeps 2^(c-1) open 4-byte write streams per block (HBM sees mostly partial-line writes:
// 6.2 ms at n = 2^24). Level 1 splits a chunk's entries into P = NB/256 partitions of 256 adjacent buckets (128 open
// streams of 8-byte records, consecutive positions -> full lines); level 2 sorts each partition by the low bucket
// byte with 256 open streams inside one contiguous output slice. All offsets come from the histogram already built.
constexpr uint32_t PART_BUCKETS = 256;
constexpr uint32_t PART_LB = 8;  // the lb of the record format (msm_sort.hpp): level 2 sorts by the low bucket byte
static_assert(PART_BUCKETS == 1u << PART_LB, "the record format's low key must hold a partition's bucket index");

// in place: part_cnt[w][ch][p] -> first intermediate slot of (chunk ch, partition p) = start of the partition's first
// bucket + entries of earlier chunks. (Folding this into k_msm_scan, 64 threads per window walking the chunks, was measured:
// 24 us against 7 + 10 us as two launches.)
__global__ __launch_bounds__(256) void k_msm_part_offsets(MsmParams p, const uint32_t* __restrict__ start, uint32_t* part_cnt) {
  const uint32_t P = p.NB / PART_BUCKETS;
  const uint32_t part = blockIdx.x * 256 + threadIdx.x, w = blockIdx.y;
  if (part >= P) return;
  uint32_t run = start[(size_t)w * (p.NB + 2) + (size_t)part * PART_BUCKETS + 1];
  uint32_t* col = part_cnt + (size_t)w * p.CH * P + part;
  for (uint32_t ch0 = 0; ch0 < p.CH; ch0 += 8) {  // loads of eight chunks in flight together, as in k_msm_colscan
    uint32_t c[8];
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j) c[j] = ch0 + j < p.CH ? col[(size_t)(ch0 + j) * P] : 0u;
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j) {
      if (ch0 + j < p.CH) col[(size_t)(ch0 + j) * P] = run;
      run += c[j];
    }
  }
}

// Level 1: block (chunk, window); tiles of L1_TILE digit codes are counting-sorted by partition inside LDS and
// written out as 8-byte records (index | sign << 31 | low bucket byte << 32) in runs of neighbouring addresses.
// REC = 1 (entry ids < 2^23, i.e. n <= 2^23 and no table remap): 4-byte records (index | sign << 23 | low bucket byte << 24)
// -- 14 instead of 22 bytes of HBM traffic per entry over the two levels. REC = 0: the 8-byte records. (rec_pack, msm_sort.hpp)
#ifndef CSH_L1_WPE
#define CSH_L1_WPE 8  // two 1024-lane blocks per CU (64 VGPRs instead of 75): one block's barriers and LDS phases under the other's loads;
                      // scatter stage 0.124 -> 0.110 ms at 2^20, 0.384 -> 0.351 at 2^22 (profiles/archive/r03_y_scatter_l1_occupancy.log)
#endif
#if CSH_L1_WPE > 0
#define CSH_L1_OCC __attribute__((amdgpu_waves_per_eu(CSH_L1_WPE)))
#else
#define CSH_L1_OCC
#endif
constexpr int L1_EPT = 8;
constexpr int L1_TILE = L1_EPT * SORT_BLK;
constexpr uint32_t MAXP = 128;  // partitions per window: NB <= 2^15
template <int REC>
__global__ __launch_bounds__(SORT_BLK) CSH_L1_OCC void k_msm_scatter_l1(MsmParams p, const uint16_t* __restrict__ dig, const uint32_t* __restrict__ part_off,
                                                             void* __restrict__ inter) {
  __shared__ uint32_t gcur[MAXP];
  __shared__ uint32_t cnt[MAXP];
  __shared__ uint32_t toff[MAXP];
  __shared__ uint32_t wsum[2];
  __shared__ uint32_t pay[L1_TILE];
  __shared__ uint8_t slo[L1_TILE];
  __shared__ uint8_t sbin[L1_TILE];
  const uint32_t ch = blockIdx.x, w = blockIdx.y, tid = threadIdx.x;
  const uint32_t P = p.NB / PART_BUCKETS;
  if (tid < MAXP) {
    gcur[tid] = tid < P ? part_off[((size_t)w * p.CH + ch) * P + tid] : 0;
    cnt[tid] = 0;
  }
  __syncthreads();
  const size_t lo = (size_t)ch * p.chunk_len;
  size_t hi = lo + p.chunk_len;
  if (hi > p.n) hi = p.n;
  const uint16_t* d = dig + (size_t)w * p.n;
  SortRec<REC>* out = reinterpret_cast<SortRec<REC>*>(inter) + (size_t)w * p.n;
  for (size_t t0 = lo; t0 < hi; t0 += L1_TILE) {
    uint32_t code[L1_EPT], rank[L1_EPT];
#pragma unroll
    for (int k = 0; k < L1_EPT; ++k) {
      const size_t i = t0 + (size_t)k * SORT_BLK + tid;
      code[k] = i < hi ? (uint32_t)__builtin_nontemporal_load(d + i) : DIG_ZERO;
    }
#pragma unroll
    for (int k = 0; k < L1_EPT; ++k) rank[k] = lds_slot(cnt, (code[k] & 0x7fffu) / PART_BUCKETS, code[k] != DIG_ZERO);
    __syncthreads();
    const uint32_t v = tid < MAXP ? cnt[tid] : 0;
    uint32_t tile_n;  // non-zero digits in this tile
    const uint32_t excl = block_excl_scan<MAXP / 64, SORT_BLK / 64>(v, wsum, &tile_n);
    if (tid < MAXP) toff[tid] = excl;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < L1_EPT; ++k) {
      if (code[k] != DIG_ZERO) {
        const uint32_t b0 = code[k] & 0x7fffu;
        const uint32_t slot = toff[b0 / PART_BUCKETS] + rank[k];
        pay[slot] = entry_id(p, t0 + (size_t)k * SORT_BLK + tid) | ((code[k] >> 15) << 31);
        slo[slot] = (uint8_t)(b0 % PART_BUCKETS);
        sbin[slot] = (uint8_t)(b0 / PART_BUCKETS);
      }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < L1_EPT; ++k) {
      const uint32_t sl = k * SORT_BLK + tid;
      if (sl < tile_n) {
        const uint32_t bin = sbin[sl];
        out[gcur[bin] + (sl - toff[bin])] = rec_pack<REC>(pay[sl], slo[sl], PART_LB);
      }
    }
    __syncthreads();
    if (tid < MAXP) {
      gcur[tid] += v;
      cnt[tid] = 0;
    }
    __syncthreads();
  }
}

// Level 2. A block works through a slice [lo, hi) of one partition's records in tiles of L2_TILE: each tile is
// counting-sorted by the low bucket byte inside LDS and then written out slot by slot, so neighbouring lanes write
// neighbouring addresses (runs of ~L2_TILE/256 entries per bucket) instead of 64 unrelated 4-byte stores per wave.
struct L2Lds {
  uint32_t obase[PART_BUCKETS];  // where the tile's entries of every bucket go in the sorted list
  uint32_t cnt[PART_BUCKETS];    // tile histogram
  uint32_t toff[PART_BUCKETS];   // tile-local exclusive offsets
  uint32_t wsum[4];
  uint32_t pay[L2_TILE];
  uint8_t sbin[L2_TILE];
};
// Where obase comes from -- the only difference between the two level-2 kernels. Both calls are made by thread b < PART_BUCKETS with
// v = the tile's entries of bucket b: reserve() before the tile is written out, advance() after.
struct L2OwnRuns {  // the block has the whole partition: obase (set to the buckets' starts by the kernel) is a running cursor
  __device__ void reserve(uint32_t*, uint32_t, uint32_t) const {}
  __device__ void advance(uint32_t* obase, uint32_t b, uint32_t v) const { obase[b] += v; }
};
struct L2SharedRuns {  // blocks share the partition: one atomicAdd per bucket and tile on the buckets' global cursors
  uint32_t* cur;
  __device__ void reserve(uint32_t* obase, uint32_t b, uint32_t v) const { obase[b] = v ? atomicAdd(&cur[b], v) : 0u; }
  __device__ void advance(uint32_t*, uint32_t, uint32_t) const {}
};
// s.cnt is zero on entry (and again on return); a barrier lies between the caller's LDS writes and the call
template <int REC, class Runs>
__device__ __forceinline__ void l2_sort_slice(L2Lds& s, const Runs runs, const SortRec<REC>* __restrict__ in, uint32_t lo, uint32_t hi,
                                              uint32_t* __restrict__ so) {
  const uint32_t tid = threadIdx.x;
  for (uint32_t t0 = lo; t0 < hi; t0 += L2_TILE) {
    SortRec<REC> e[L2_EPT];
    uint32_t rank[L2_EPT];
    l2_load_rank<REC>(in, t0, hi, PART_LB, s.cnt, e, rank);
    __syncthreads();
    uint32_t v = 0, total;
    if (tid < PART_BUCKETS) {
      v = s.cnt[tid];
      runs.reserve(s.obase, tid, v);
    }
    const uint32_t excl = block_excl_scan<PART_BUCKETS / 64, SORT_BLK / 64>(v, s.wsum, &total);  // waves 0..3, fully active: wave scan + 4 wave totals
    if (tid < PART_BUCKETS) s.toff[tid] = excl;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < L2_EPT; ++k) {
      if (t0 + k * SORT_BLK + tid < hi) {
        const uint32_t bin = rec_low<REC>(e[k], PART_LB);
        const uint32_t slot = s.toff[bin] + rank[k];
        s.pay[slot] = rec_entry<REC>(e[k], PART_LB);
        s.sbin[slot] = (uint8_t)bin;
      }
    }
    __syncthreads();
    const uint32_t tile_n = hi - t0 < (uint32_t)L2_TILE ? hi - t0 : (uint32_t)L2_TILE;
#pragma unroll
    for (int k = 0; k < L2_EPT; ++k) {
      const uint32_t sl = k * SORT_BLK + tid;
      if (sl < tile_n) {
        const uint32_t bin = s.sbin[sl];
        so[s.obase[bin] + (sl - s.toff[bin])] = s.pay[sl];
      }
    }
    __syncthreads();
    if (tid < PART_BUCKETS) {
      runs.advance(s.obase, tid, v);
      s.cnt[tid] = 0;
    }
    __syncthreads();
  }
}

// Level 2, block (partition, window): no atomics, the order inside a bucket is deterministic (tune "msm_variant" bit 5).
template <int REC>
__global__ __launch_bounds__(SORT_BLK) void k_msm_scatter_l2(MsmParams p, const uint32_t* __restrict__ start, const void* __restrict__ inter,
                                                             uint32_t* __restrict__ sorted) {
  __shared__ L2Lds s;
  const uint32_t part = blockIdx.x, w = blockIdx.y, tid = threadIdx.x;
  const uint32_t* st = start + (size_t)w * (p.NB + 2) + (size_t)part * PART_BUCKETS + 1;
  if (tid < PART_BUCKETS) {
    s.obase[tid] = st[tid];
    s.cnt[tid] = 0;
  }
  __syncthreads();
  l2_sort_slice<REC>(s, L2OwnRuns{}, reinterpret_cast<const SortRec<REC>*>(inter) + (size_t)w * p.n, st[0], st[PART_BUCKETS],
                     sorted + (size_t)w * p.n);
}

// Level 2, tile-parallel (the default since the end of round 3). The kernel above gives one block a whole partition, so a skewed
// digit distribution -- a 0/1-heavy witness puts every "1" into bucket 1 of window 0, a repeated value one bucket per window -- leaves
// ONE block to sort a quarter or half of a window's entries tile after tile while the rest of the chip is idle (scatter 0.11 -> 0.42 ms
// at 2^20 with half the scalars in {0, 1} and a quarter equal). Here every partition is cut into slices of about one tile, one block
// each: the block finds its (partition, slice) from the partitions' sizes (a 128-entry scan of `start`), counting-sorts its tiles by the
// low bucket byte in LDS as before, and reserves the output run of every bucket with ONE global atomicAdd per bucket and tile on the
// cursor array k_msm_scan left in `hist`. The order of the entries inside a bucket then depends on the order in which blocks reserve --
// the bucket sums are sums in a group, the results are bit-identical (parity suite), and `start` is untouched.
template <int REC>
__global__ __launch_bounds__(SORT_BLK) void k_msm_scatter_l2t(MsmParams p, const uint32_t* __restrict__ start, uint32_t* __restrict__ cursor,
                                                              const void* __restrict__ inter, uint32_t* __restrict__ sorted) {
  __shared__ L2Lds s;
  __shared__ uint32_t job[3];  // partition, first and one-past-last intermediate slot of this block's slice
  const uint32_t x = blockIdx.x, w = blockIdx.y, tid = threadIdx.x;
  const uint32_t P = p.NB / PART_BUCKETS;
  const uint32_t* stw = start + (size_t)w * (p.NB + 2);
  {  // which slice of which partition is block x: partitions get max(1, round(entries / tile)) blocks each (none when empty)
    uint32_t lo_p = 0, hi_p = 0, nb = 0, total;
    if (tid < P) {
      lo_p = stw[(size_t)tid * PART_BUCKETS + 1];
      hi_p = stw[(size_t)(tid + 1) * PART_BUCKETS + 1];
      const uint32_t c = hi_p - lo_p;
      nb = c ? (c + L2_TILE / 2) / L2_TILE : 0;
      if (c && nb == 0) nb = 1;
    }
    if (tid == 0) job[0] = 0xffffffffu;
    const uint32_t pre = block_excl_scan<MAXP / 64, SORT_BLK / 64>(nb, s.wsum, &total);  // blocks of earlier partitions
    if (nb && x >= pre && x < pre + nb) {
      const uint32_t c = hi_p - lo_p, slice = (c + nb - 1) / nb, j = x - pre;
      uint32_t a = lo_p + j * slice, b = a + slice;
      if (b > hi_p) b = hi_p;
      if (a > hi_p) a = hi_p;
      job[0] = tid;
      job[1] = a;
      job[2] = b;
    }
    __syncthreads();
  }
  const uint32_t part = job[0];
  if (part == 0xffffffffu) return;  // the grid is sized for the worst case (entries / tile + partitions blocks per window)
  if (tid < PART_BUCKETS) s.cnt[tid] = 0;
  __syncthreads();
  l2_sort_slice<REC>(s, L2SharedRuns{cursor + (size_t)w * (p.NB + 2) + (size_t)part * PART_BUCKETS + 1},
                     reinterpret_cast<const SortRec<REC>*>(inter) + (size_t)w * p.n, job[1], job[2], sorted + (size_t)w * p.n);
}

// Two-level mode pays off once a (partition, window) block has enough records to fill its tiles: n >= 2^20
// (measured: 2^20 0.22 -> 0.12 ms, 2^24 6.2 -> 2.1 ms; slower at 2^18). csh_tune_set("sort_two_level", 0/1) forces a mode (tests).
bool msm_sort_two_level(const MsmParams& p) {
  if (p.NB < 4 * PART_BUCKETS) return false;
  if (const int f = tune().sort_two_level.load(std::memory_order_relaxed); f >= 0) return f != 0;
  return p.n >= (1u << 20);
}

SortPath msm_sort_path(const MsmParams& p) {
  SortPath s{msm_sort_two_level(p), false, false};
  if (!s.two_level) return s;
  // 4-byte intermediate records when every stored entry id fits 23 bits (n, or rows x bases with tables, <= 2^23); tune "msm_variant"
  // bit 3 forces the 8-byte records (A/B runs, tests). (4-byte records + a separate sign byte for ids up to 2^24 were
  // measured and lose to the 8-byte records: scatter 2.29 against 2.10 ms on BN254 G1 2^24 -- byte-granular scattered
  // writes cost more than the 3 bytes per entry they save, profiles/archive/r02_g_rec_stages.log.)
  const uint64_t max_id = p.remap_n ? (uint64_t)(p.n / p.remap_n) * p.remap_stride : (uint64_t)p.n;  // stored ids: table indices
  const int variant = tune().msm_variant.load(std::memory_order_relaxed);
  s.rec4 = (variant & 8) == 0 && max_id <= (1u << (31 - PART_LB));
  s.per_partition = (variant & 32) != 0;
  return s;
}

// the two-level scatter with 4-byte (REC = 1) or 8-byte intermediate records
template <int REC>
static void launch_two_level(const MsmParams& p, const SortBuffers& b, bool per_partition, hipStream_t st) {
  const uint32_t nparts = p.NB / PART_BUCKETS;
  hipLaunchKernelGGL(k_msm_scatter_l1<REC>, dim3(p.CH, p.W), dim3(SORT_BLK), 0, st, p, b.dig, b.part_cnt, (void*)b.inter);
  // level 2: one block per slice of about one tile of a partition (default), or -- tune "msm_variant" bit 5 -- one block per partition
  if (per_partition) {
    hipLaunchKernelGGL(k_msm_scatter_l2<REC>, dim3(nparts, p.W), dim3(SORT_BLK), 0, st, p, b.start, (const void*)b.inter, b.sorted);
  } else {
    const uint32_t l2_blocks = (uint32_t)(p.n / L2_TILE) + nparts + 1;
    hipLaunchKernelGGL(k_msm_scatter_l2t<REC>, dim3(l2_blocks, p.W), dim3(SORT_BLK), 0, st, p, b.start, b.hist, (const void*)b.inter, b.sorted);
  }
}

int msm_sort_launch(const MsmParams& p, const SortBuffers& b, hipStream_t st, hipEvent_t* ev) {
  const SortPath path = msm_sort_path(p);
  const bool two_level = path.two_level;
  const size_t sort_lds = sizeof(uint32_t) * p.NB;
  if (sort_lds > 48 * 1024) {
    CSH_TRY(raise_lds_limit((const void*)k_msm_hist_lds, 128 * 1024));
    CSH_TRY(raise_lds_limit((const void*)k_msm_scatter_lds, 128 * 1024));
  }
  hipLaunchKernelGGL(k_msm_hist_lds, dim3(p.CH, p.W), dim3(SORT_BLK), sort_lds, st, p, b.dig, b.blkcnt, two_level ? b.part_cnt : nullptr);
  hipLaunchKernelGGL(k_msm_colscan, dim3((p.NB + 255) / 256, p.W), dim3(256), 0, st, p, b.blkcnt, b.hist);
  if (ev) CSH_HIP(hipEventRecord(ev[1], st));
  {
    const size_t scan_lds = sizeof(uint32_t) * ((size_t)p.NB + 2 + 16);
    if (scan_lds > 48 * 1024) CSH_TRY(raise_lds_limit((const void*)k_msm_scan, 136 * 1024));
    hipLaunchKernelGGL(k_msm_scan, dim3(p.W), dim3(1024), scan_lds, st, p, b.hist, b.start, b.nlanes);
  }
  if (ev) CSH_HIP(hipEventRecord(ev[2], st));
  if (two_level) {
    hipLaunchKernelGGL(k_msm_part_offsets, dim3((p.NB / PART_BUCKETS + 255) / 256, p.W), dim3(256), 0, st, p, b.start, b.part_cnt);
    path.rec4 ? launch_two_level<1>(p, b, path.per_partition, st) : launch_two_level<0>(p, b, path.per_partition, st);  // msm_sort_path
  } else {
    hipLaunchKernelGGL(k_msm_scatter_lds, dim3(p.CH, p.W), dim3(SORT_BLK), sort_lds, st, p, b.dig, b.start, b.blkcnt, b.sorted);
  }
  if (ev) CSH_HIP(hipEventRecord(ev[3], st));
  return CSH_OK;
}

}  // namespace csh
