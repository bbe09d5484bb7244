// C entry points of the host mirror, the part without a prover: wire-format round trips, the Rep3 randomness on its own, query placement
// and the process-wide settings; also the process-wide pieces that exist once (the allocator setup, the OS entropy source, the last error).
#include <malloc.h>
#include <sys/random.h>

#include "capi_common.hpp"

namespace {
// The prover's large host vectors (32 MB masks, h, half shares at 2^20) are malloc'ed and freed once per proof; glibc serves blocks of
// that size with mmap and returns them with munmap, so every proof pays tens of thousands of page faults and two or three multi-ms
// unmaps that stall every other thread of the process behind the address-space lock (round 6: freeing the two mask vectors of one Rep3
// witness map cost ~8 ms on the calling thread; moved to a background thread the same cost reappeared in the page faults of the next
// allocation, profiles/r06_m_retain_ab.log). The mirror therefore asks glibc to keep such blocks in its heap (no mmap per block, no
// trim): what jemalloc / mimalloc -- the allocators a Rust prover usually links -- do by default. Measured at 2^20 (same log): plain
// trait-path prove 16.8-18.2 -> 14.7-14.9 ms, a seeded Rep3 party 19.2 -> 16.8-17.0 ms, three of them on one GPU 64 -> 40-47 ms; the
// host-mask party 40-42 -> 39 ms (its mask draw gets SLOWER on retained pages, 12 -> 20 ms, while everything around it gets faster).
// COG16_MALLOC_RETAIN=0 leaves glibc alone.
struct MallocRetain {
  MallocRetain() {
    const char* e = getenv("COG16_MALLOC_RETAIN");
    if (e && atoi(e) == 0) return;
    (void)mallopt(M_MMAP_THRESHOLD, 1 << 30);
    (void)mallopt(M_TRIM_THRESHOLD, (int)((1u << 31) - 1));
    (void)mallopt(M_TOP_PAD, 64 << 20);
  }
} g_malloc_retain;
}  // namespace

namespace cosnarks {
void secure_random_bytes(void* out, size_t n) {
  uint8_t* p = static_cast<uint8_t*>(out);
  size_t got = 0;
  while (got < n) {
    const ssize_t r = getrandom(p + got, n - got, 0);
    if (r > 0) {
      got += (size_t)r;
      continue;
    }
    break;
  }
  if (got < n) {  // pre-3.17 kernels / seccomp without getrandom
    FILE* f = fopen("/dev/urandom", "rb");
    if (f) {
      got += fread(p + got, 1, n - got, f);
      fclose(f);
    }
  }
  if (got < n) throw Error("no OS entropy source (getrandom and /dev/urandom both failed)");
}

namespace capi {
thread_local std::string g_err;
}
}  // namespace cosnarks

using namespace cosnarks;
using namespace cosnarks::capi;

extern "C" {

const char* cog16_last_error(void) { return g_err.c_str(); }

// ark-serialize round trips of the host mirror (arkwire.hpp): mode 0 Vec<Fr> (in: Montgomery limbs of n elements ->
// out: serialized bytes, then parsed back and compared), mode 1 G1 affine points (n points, C-ABI layout). Returns the
// number of bytes written to `out`, or -1.
int cog16_ark_roundtrip(int curve, int mode, const void* in, size_t n, uint8_t* out, size_t cap) {
  return entry<Bn254, Bls12_381>(curve, [&](auto tag) {
    using P = decltype(tag);
    using Fr = typename P::Fr;
    using Fq = typename P::Fq;
    std::vector<uint8_t> buf;
    if (mode == 0) {
      std::vector<Fr> v(n);
      memcpy((void*)v.data(), in, sizeof(Fr) * n);
      ark::write_vec(buf, v);
      ark::Reader r(buf.data(), buf.size());
      std::vector<Fr> back = ark::read_vec<Fr>(r);
      if (!r.done() || back.size() != n || memcmp(back.data(), v.data(), sizeof(Fr) * n) != 0) throw Error("Vec<F> round trip mismatch");
    } else {
      std::vector<AffineT<Fq>> pts(n);
      memcpy((void*)pts.data(), in, sizeof(AffineT<Fq>) * n);
      for (auto& pt : pts) ark::write_g1(buf, pt);
      ark::Reader r(buf.data(), buf.size());
      for (auto& pt : pts) {
        AffineT<Fq> q = ark::read_g1<Fq>(r);
        if (memcmp(&q, &pt, sizeof q) != 0) throw Error("G1 round trip mismatch");
      }
      if (!r.done()) throw Error("trailing bytes");
    }
    return copy_out(buf, out, cap);
  });
}

// Rep3NetworkExt::{send_many, recv_many} payloads (arkwire.hpp). kind 0: field elements (Fr, Montgomery limbs on the C-ABI side), kind 1: G1
// affine points (C-ABI layout). op 0 = send_many: `in` holds n items -> message bytes in `out`, returns the message length; op 1 =
// recv_many: `in` holds a message of n BYTES -> items in `out` (cap in bytes), returns the item count. -1 on error.
long cog16_rep3_wire(int curve, int op, int kind, const void* in, size_t n, void* out, size_t cap) {
  long result = -1;
  auto items_in = [&](auto& v) {
    v.resize(n);
    if (n) memcpy((void*)v.data(), in, sizeof(v[0]) * n);
  };
  auto items_out = [&](const auto& v) {
    copy_out(v.data(), v.size() * sizeof(v[0]), out, cap);
    return (long)v.size();
  };
  const int rc = guarded([&] {
    if (op != 0 && op != 1) throw Error("op must be 0 (send_many) or 1 (recv_many)");
    if (kind != 0 && kind != 1) throw Error("kind must be 0 (field elements) or 1 (G1 affine points)");
    return with_curve<Bn254, Bls12_381>(curve, [&](auto tag) {
      using P = decltype(tag);
      using Fr = typename P::Fr;
      using Fq = typename P::Fq;
      if (op == 0) {
        std::vector<uint8_t> msg;
        if (kind == 0) {
          std::vector<Fr> v;
          items_in(v);
          msg = ark::send_many_fields(v);
        } else {
          std::vector<AffineT<Fq>> v;
          items_in(v);
          msg = ark::send_many_g1(v);
        }
        copy_out(msg, out, cap);
        result = (long)msg.size();
      } else if (kind == 0) {
        result = items_out(ark::recv_many_fields<Fr>(static_cast<const uint8_t*>(in), n));
      } else {
        result = items_out(ark::recv_many_g1<Fq>(static_cast<const uint8_t*>(in), n));
      }
      return 0;
    });
  });
  return rc < 0 ? -1 : result;
}

// The mirror's Rep3 randomness on its own (host only, no device): three parties with PRF keys k_p = keys[32 p ..] (party p holds its
// own key as rng1 and its predecessor's as rng2, rep3.rs:71-76). Per party, in this order: a mask vector of n elements
// (masking_field_elements_vec, rngs.rs:137-156; drawn in parallel over the host's cores), one random_seeds() pair (rngs.rs:233), a second
// mask vector of n2 elements (the generators must continue where a serial draw would have left them).
// masks_out: 3 x (n + n2) x 4 limbs (Montgomery); seeds_out: 3 x 64 bytes (seed1 || seed2).
int cog16_rep3_rand_selftest(int curve, const uint8_t keys[96], size_t n, size_t n2, uint64_t* masks_out, uint8_t* seeds_out) {
  return guarded([&] {
    if (!keys || !masks_out || !seeds_out) throw Error("cog16_rep3_rand_selftest: NULL argument");
    return with_curve<Bn254, Bls12_381>(curve, [&](auto tag) {
      using Fr = typename decltype(tag)::Fr;
      for (int p = 0; p < 3; ++p) {
        Rep3Rand r(keys + 32 * p, keys + 32 * ((p + 2) % 3));
        const UninitBuf<Fr> a = r.masking_field_elements_vec<Fr>(n);
        r.random_seeds(seeds_out + 64 * p, seeds_out + 64 * p + 32);
        const UninitBuf<Fr> b = r.masking_field_elements_vec<Fr>(n2);
        uint64_t* o = masks_out + 4 * (n + n2) * (size_t)p;
        if (n) memcpy(o, a.data(), 32 * n);
        if (n2) memcpy(o + 4 * n, b.data(), 32 * n2);
      }
      return 0;
    });
  });
}

// 1: every prove_inner of this process runs the "trait path" (groth16.hpp: the sequence rust/co-groth16-hip drives behind the unchanged
// reference -- host slices at every seam, one witness-map call, five concurrent host-scalar MSMs); 0: the device-resident prove.
// 2: the trait path with the shim's opt-in seeded Rep3 masks (groth16.hpp witness_map_trait_path).
int cog16_set_trait_path(int on) {
  trait_path_flag().store(on == 2 ? 2 : (on ? 1 : 0));
  return 0;
}
int cog16_get_trait_path(void) { return trait_path_flag().load(); }

// The placement plan for a key whose five queries (a, b_g1, b_g2, l, h) have `sizes` points, on `nslots` GPUs: host-only (no device
// needed). slots_out[q] = the slot of query q (by query), ranges_out[2 * slot + {0, 1}] = [lo, hi) of n_range entries (by range);
// returns the effective mode (1 by query, 2 by range) or -1.
int cog16_placement_plan(const size_t sizes[5], int nslots, int mode, size_t n_range, int slots_out[5], size_t* ranges_out) {
  return guarded([&] {
    if (!sizes || !slots_out || nslots < 1 || nslots > 64 || mode < 0 || mode > 2) throw Error("cog16_placement_plan: bad arguments");
    const int eff = plan_placement(sizes, (size_t)nslots, mode, slots_out);
    if (ranges_out)
      for (int sl = 0; sl < nslots; ++sl) {
        if (eff == PLACE_BY_RANGE && nslots > 1) plan_range(n_range, (size_t)nslots, (size_t)sl, &ranges_out[2 * sl], &ranges_out[2 * sl + 1]);
        else {
          ranges_out[2 * sl] = 0;
          ranges_out[2 * sl + 1] = n_range;
        }
      }
    return eff;
  });
}

// One prover's five query MSMs over several GPUs: keys built after this call clone their queries onto `devices` (entry 0 = the
// key's home GPU; a GPU may be listed more than once, which is how the single-GPU tests exercise the path). n <= 1 switches it off.
int cog16_set_prover_devices_mode(const int* devices, int n, int mode);
int cog16_set_prover_devices(const int* devices, int n) { return cog16_set_prover_devices_mode(devices, n, 0); }
// mode: 0 = automatic (whole queries per GPU up to two GPUs, ranges of every query from three on), 1 = whole queries, 2 = ranges
int cog16_set_prover_devices_mode(const int* devices, int n, int mode) {
  return guarded([&] {
    if (mode < 0 || mode > 2) throw Error("cog16_set_prover_devices: mode must be 0 (auto), 1 (by query) or 2 (by range)");
    int ndev = 0;
    check(csh_device_count(&ndev), "csh_device_count");
    std::vector<int> d;
    for (int i = 0; i < n; ++i) {
      if (!devices || devices[i] < 0 || devices[i] >= (ndev > 0 ? ndev : 1)) throw Error("cog16_set_prover_devices: device out of range");
      d.push_back(devices[i]);
    }
    std::lock_guard<std::mutex> g(ProverDevices::get().mu);
    ProverDevices::get().devices = d.size() > 1 ? d : std::vector<int>();
    ProverDevices::get().mode = mode;
    return 0;
  });
}

}  // extern "C"
