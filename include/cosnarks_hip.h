/*
 * cosnarks_hip.h -- C ABI of the MI355X (gfx950) proof-generation hot path for co-snarks.
 *
 * This is the drop-in boundary: the reference (TaceoLabs/co-snarks, 100 % Rust) has no FFI today; its
 * hot path sits behind Rust traits/free functions whose arithmetic lives in the un-vendored crates
 * taceo-ark-algebra 0.1.0 / ark-poly 0.6.0.  Each entry point below names the reference interface it
 * replaces (paths relative to the reference root).  INTEGRATION.md shows the Rust `extern "C"` block and
 * the trait implementors (`HipCircomReduction: R1CSToQAP`, `Hip*Groth16Driver: CircomGroth16Prover`)
 * that bind it.
 *
 * Data conventions (identical to arkworks' in-memory layout, so Rust slices can be passed as-is):
 *  - field element  = N64 little-endian u64 limbs of x*R mod p (Montgomery, R = 2^(64*N64));
 *                     Fr: 4 limbs (32 B) on every curve; Fq: 4 limbs (BN254) / 6 limbs (BLS12-381, BLS12-377).
 *                     Every field element the library returns (vectors, transforms, shares, masks, point
 *                     coordinates) is canonical arkworks Montgomery form: x*R mod p < p, never a lazy
 *                     representative such as x*R mod p + p, even where kernels compute in lazy form inside.
 *  - affine point   = x || y (G2: x.c0 || x.c1 || y.c0 || y.c1), Montgomery; infinity = all-zero bytes
 *                     (the zkey convention).  `stride_bytes` lets the caller pass arkworks `Affine`
 *                     (x, y, infinity flag, padding) without repacking -- the flag byte is ignored.
 *  - result point   = arkworks `Projective` = Jacobian (X, Y, Z), Montgomery; infinity = (1, 1, 0).
 *                     The library always returns Z in {0, 1} (normalised), which is a valid Jacobian
 *                     representative; the reference compares/serialises affine forms only
 *                     (co-circom/co-groth16/src/groth16.rs:333-337).
 *  - Rep3 share     = {a, b} = 2 consecutive Fr elements (64 B)
 *                     (mpc-core/src/protocols/rep3/arithmetic/types.rs:21-28).
 *  - Shamir share   = 1 Fr element (repr(transparent), shamir/arithmetic/types.rs:9-13).
 *
 * Pointers named `*_dev` / functions suffixed `_dev` take DEVICE pointers and a HIP stream (NULL = the
 * library's per-thread stream) and are asynchronous unless they return data to the host; all other
 * pointers are HOST pointers and the call is synchronous.  All functions return 0 on success or a
 * negative csh_status; csh_last_error() returns a thread-local message.  Every entry point is
 * re-entrant and thread-safe (the reference calls MSMs/NTTs concurrently from rayon workers:
 * groth16.rs:227-294, reduction.rs:135-178).  There is no CPU fallback: without a HIP device every
 * compute entry point fails with CSH_ERR_NO_DEVICE.
 *
 * Host threads the library itself starts (all joined before the call returns unless said otherwise; none touches caller memory after
 * the return):
 *  - entry points that move >= 4 MiB between caller memory and the device through HOST pointers -- csh_groth16_witness_map / _masks /
 *    _libsnark*, csh_groth16_h*, the host-pointer transforms and share-vector calls (no _dev suffix), csh_msm / csh_msm_shares with host
 *    scalars -- start ONE short-lived thread per result that populates the destination's pages while the device works ("host_populate"),
 *    and hand the chunks of a staged transfer ("host_d2h" / "host_h2d" = 1, the default) to a process-wide pool of up to eight parked
 *    copier threads, created on first use and kept for the life of the process; they touch caller memory only while the call that
 *    enlisted them is running. csh_tune_set("host_populate", 0) + ("host_d2h", 0) + ("host_h2d", 0) turns all of it off (the call then
 *    never leaves the calling thread, and the runtime pins the caller's pages itself);
 *  - csh_msm with host scalars ("msm_share_uploads" = 2, the default): a call that finds another call of the same process uploading the
 *    SAME scalar slice (pointer, length, device, curve, encoding) hands that call its request and blocks; the uploading call's thread
 *    runs both as one csh_msm_multi_dev and writes the result into the waiting call's `out` before either returns;
 *  - csh_comm_init_rank with nranks > 1 runs the collective ncclCommInitRank on a helper thread against "comm_timeout_ms"; a helper
 *    whose peers never arrive is ABANDONED (still blocked inside RCCL after the call returned its error): leave such a process
 *    through _exit.
 *  Everything else (csh_msm_dev / _multi_dev / _partial_dev, csh_msm_split*, every other *_dev entry point) runs on the calling thread
 *  only. Page-locked staging memory is bounded: at most 32 MiB per (thread lane, stream, slot) -- larger transfers cycle through a ring
 *  of 2 MiB chunks (round 6).
 */
#ifndef COSNARKS_HIP_H
#define COSNARKS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* CSH_GRUMPKIN (MSM entry points only, group CSH_G1): the BN254 cycle curve y^2 = x^3 - 17 over BN254 Fr with scalar field
 * BN254 Fq -- HonkCurve::fast_msm for short_weierstrass::Projective<GrumpkinConfig> (co-noir-common/src/honk_curve.rs:163-177). */
/* CSH_BLS12_377: the curve of the reference's LibSnarkReduction fixtures (Groth16::<Bls12_377>::plain_prove::<LibSnarkReduction>,
 * co-groth16/src/lib.rs:231-300): `field_of` of the NTT / share-vector / sparse-matrix / reduction entry points (its scalar field Fr)
 * and, since round 6, both MSM groups (G1: y^2 = x^3 + 1 over the 377-bit Fq, 96-byte affine points; G2 over Fq[u]/(u^2 + 5),
 * 192 bytes) through every csh_bases_* / csh_msm* entry point, tables and split ranges included. */
typedef enum { CSH_BN254 = 0, CSH_BLS12_381 = 1, CSH_GRUMPKIN = 2, CSH_BLS12_377 = 3 } csh_curve_t;
typedef enum { CSH_G1 = 0, CSH_G2 = 1 } csh_group_t;

typedef enum {
  CSH_OK = 0,
  CSH_ERR_INVALID = -1,    /* bad argument */
  CSH_ERR_NO_DEVICE = -2,  /* no HIP device / runtime failure at init */
  CSH_ERR_HIP = -3,        /* a HIP runtime call failed (see csh_last_error) */
  CSH_ERR_OOM = -4,
  CSH_ERR_DOMAIN = -5      /* "Polynomial Degree too large" (reduction.rs:87-94) */
} csh_status;

typedef struct csh_bases_s* csh_bases_t;   /* proving-key query resident on the device */
typedef struct csh_domain_s* csh_domain_t; /* radix-2 evaluation domain (twiddles on device) */
typedef struct csh_poseidon2_params_s* csh_poseidon2_params_t; /* one Poseidon2 parameter set on the device */
typedef struct csh_shamir_rng_s* csh_shamir_rng_t; /* one Shamir party's shared streams, public matrices and double-share buffers */

/* ---- context ------------------------------------------------------------------------------- */
int csh_init(int device);            /* select device for the calling thread, create context lazily */
int csh_shutdown(void);              /* free all cached workspaces/streams of every device */
const char* csh_last_error(void);
const char* csh_version(void);
int csh_device_count(int* count);
/* Process-wide tuning knobs for A/B runs and tests (initial values come from the environment once, at load: CSH_MSM_C ...;
 * no entry point reads the environment afterwards). Keys: "msm_c" (forced window width, 0 = cost model), "msm_l" (entries per
 * accumulate lane, 0 = round-count cost model), "msm_seg_buckets" (buckets per window-reduction segment, 0 = as many segments
 * as fit one round of waves), "msm_timing" (record csh_msm_last_timing), "msm_no_table", "msm_multi_overlap", "acc_blk",
 * "sort_two_level" (-1 auto), "vec_max_blocks", "ntt_lazy", "ntt_threads", "ntt_variant" (A/B forms with equal results; its timing-experiment
 * bits 12-13 / 16-19 and "allow_unmasked_rep3" return WRONG / unmasked results and exist only in builds with -DCSH_EXPERIMENTS: the product
 * library refuses them with CSH_ERR_INVALID and never takes them from the environment), "msm_wide_lb" / "msm_wide_chunks" (wide sort
 * stage of the fixed-base MSM: log2 buckets per second-level partition 8 .. 11, first-level blocks; 0 = defaults), "msm_variant" (bit mask of non-default kernel forms, same results: bit 0 = window reduction
 * lane-serial on G1 / four-lane on G2, bit 1 = the other form of the G2 accumulate kernel (BN254 G2: two lanes per point instead of whole points; BLS12-381 G2: whole
 * points instead of two lanes per point), bit 2 = lane-serial window
 * reduction on G2, bit 3 = 8-byte sort records at every size, bit 4 = merge fused into the window reduction, bit 5 = level 2 of the
 * two-level sort with one block per partition instead of one per tile-sized slice), "h_unfused", "h_table_cache" (1 = default: the witness map's scaled coset table stays with the
 * domain after the first call, 32 bytes per point up to 2^25 points; 0 = rebuilt per call), "comm_timeout_ms" (csh_comm_init_rank),
 * "host_populate" (results of >= 4 MiB handed back in pageable memory: low byte = host threads that populate the destination's
 * pages while the device works, 0 = none; bit 8 = transparent-huge-page hint on the range; default 0x101), "host_d2h" (the copy of such
 * a result: 0 = one DMA into the caller's pages, 1 = default since round 5: staged through the lane's page-locked buffer and moved on by
 * host threads, 2 = direct and timed; two stalled copies in a row on one lane -- the stream + scratch leased to one host thread at a time, so
 * concurrent callers do not race on the detector -- switch every large transfer of the process, both directions, to the staged paths for
 * the next 4096 transfers: the stall is a process-wide condition of the runtime having pinned caller memory that was unmapped since, and
 * it only goes away while the runtime sees no caller memory at all; counter "stat_stage_all_switches"),
 * "host_h2d" (uploads of >= 4 MiB from caller memory: 0 = one copy from the caller's pages, 1 = staged through the lane's page-locked
 * buffers in 2 MiB chunks copied by host threads -- the driver never pins caller memory; the default, 2 = direct and timed, feeding the same
 * process-wide switch as "host_d2h"; counters "stat_h2d_slow", "stat_h2d_staged". Staging is the default in both directions because a
 * process whose runtime has pinned caller memory that was unmapped afterwards can stall 10-30 ms per later call for the rest of its life
 * (DESIGN.md 3.4), and that state cannot be left once entered),
 * "msm_share_uploads" (concurrent csh_msm calls handed the same host scalar slice: 1 = they share one upload; 2 = default since round 6:
 * the calls that arrive while the first one is uploading are also RUN by it, as one csh_msm_multi_dev -- one digit sort for the handles of
 * equal length and offset -- and return when it has written their results; 0 = every call uploads and runs for itself; counter
 * "stat_uploads_shared"), "host_timing" (diagnostics: phase times of the host-facing witness map in "stat_wm_h2d_us" / "_dev_us" / "_d2h_us"),
 * "msm_balanced" (1 = default: the MSM's windows share the scalar bits evenly, widths c and c - 1; 0 = uniform c-bit windows),
 * "msm_w" (balanced windows: forced number of windows, 0 = the tuned count), "scan_lane_run" / "scan_tile_lanes" / "scan_spine_step"
 * (field scans, see there), "fold_tile_log" (multilinear folds, see there). Read-only counters
 * (csh_tune_get): "stat_arena_grows", "stat_lanes", "stat_populate_us", "stat_join_wait_us", "stat_finish_us", "stat_d2h_slow",
 * "stat_d2h_staged". */
int csh_tune_set(const char* key, int value);
int csh_tune_get(const char* key, int* value);

/* plain device-memory plumbing for harnesses without their own HIP binding (tests, the Rust shim) */
/* the device the calling thread is bound to (csh_init, default 0): handles (bases, domains, matrices) are per device */
int csh_current_device(int* device);
int csh_malloc(void** dev_ptr, size_t bytes);
int csh_free(void* dev_ptr);
int csh_memcpy_h2d(void* dev_dst, const void* host_src, size_t bytes);
/* waits first for whatever the CALLING thread queued with stream = NULL (its lane stream): a result some csh_*_dev call of this thread
 * is still producing is complete when the copy reads it */
int csh_memcpy_d2h(void* host_dst, const void* dev_src, size_t bytes);
/* device-to-device between GPUs (scalars of one prover to the GPU that runs one of its MSMs). stream NULL = synchronous. */
int csh_memcpy_peer(void* dst, int dst_device, const void* src, int src_device, size_t bytes, void* stream);
int csh_sync(void* stream);
/* out[i] = component `comp` of the i-th share (ncomp 32-byte field elements per share), device to device: the
 * `to_half_share` map over the witness (groth16.rs:159-163; Rep3 = take `.a`, mpc/rep3.rs:120-122) without a host pass. */
int csh_extract_component_dev(const uint64_t* shares_dev, uint32_t ncomp, uint32_t comp, size_t n, uint64_t* out_dev, void* stream);

/* ---- MSM ------------------------------------------------------------------------------------
 * Replaces taceo_ark_algebra::msm::msm_unchecked(&[Affine<C>], &[F]) -> Projective<C> and
 * msm::msm_bigint(&[Affine<C>], &[F::BigInt]); call sites groth16.rs:193-194, mpc/plain.rs:66-74,
 * mpc/rep3.rs:124-132, mpc/shamir.rs:111-119, mpc-core/src/protocols/rep3/pointshare.rs:201-222,
 * shamir/pointshare.rs:207-225, co-noir/co-noir-common/src/honk_curve.rs:81-83.
 * Bases (ProvingKey queries a_query/b_g1_query/b_g2_query/l_query/h_query, groth16.rs:219-290) are
 * uploaded once and reused across proofs. */
int csh_bases_upload(csh_curve_t curve, csh_group_t group, const void* affine_points, size_t n,
                     size_t stride_bytes /* 0 = packed */, csh_bases_t* out);
int csh_bases_upload_dev(csh_curve_t curve, csh_group_t group, const void* affine_points_dev, size_t n,
                         size_t stride_bytes, void* stream, csh_bases_t* out);
int csh_bases_len(csh_bases_t bases, size_t* n);
/* Optional, for bases reused across many MSMs (proving-key queries: uploaded once per key, groth16.rs:219-225): builds
 * fixed-base window tables 2^(c w) P_i on the device (c = 0: automatic; c in 4 .. 22; W x the memory of the points). MSMs on the
 * handle then put all windows into ONE set of 2^(c-1) buckets: one bucket reduction instead of W, no Horner over windows, and
 * -- with c = 17 .. 22, round 6 -- FEWER mixed additions per point than any plain plan (W = ceil((bits + 1) / c): 15 at c = 17, 13
 * at c = 20, against 17 / 16 at the plain plan's c = 15 / 16). Results are the same group elements. Handles with fewer than 1024
 * points are left unchanged. Measured on MI355X against the plain handle (profiles/r06_e_*, r06_f_*): BN254 G1 2^16 0.355 against
 * 0.40 ms, 2^18 0.56 / 0.71, 2^20 +15 %, 2^24 (c = 20) +15 .. 17 % points/s; BN254 G2 +14 %, BLS12-381 G1 / G2 +15 / +10 % at 2^20. */
int csh_bases_precompute(csh_bases_t bases, int c);
/* The same with `groups` (2..128) table rows instead of one per window: row k holds 2^(c W' k) P_i, W' = ceil(windows / groups),
 * so that windows w and w + W' k share a bucket set: W' bucket reductions instead of W and a host Horner over W' windows, for
 * groups x the memory of the points (c <= 16). groups >= the window count is the full merge above (the only form for c > 16).
 * Same results; replaces any tables already on the handle. */
int csh_bases_precompute_grouped(csh_bases_t bases, int c, int groups);
/* The table policy of the library for the queries of ONE proving key whose largest query has `key_points` points (host-only,
 * no device needed): window width *c_out and row count *rows_out to pass to csh_bases_precompute_grouped for every query of
 * the key (equal (c, rows) on all of them lets csh_msm_multi_dev share one digit pass), or *rows_out = 0 when tables do not pay
 * (keys below 2^14 or above 2^26 points). Round 6: one row per window (rows_out >= the window count of either scalar field), c = 17
 * from 2^15 to 3 * 2^20 points, c = 20 above; 2^14 .. 2^15: c <= 16. The C++ host mirror
 * (ProvingKey::build_tables) and the Rust bases cache (rust/co-groth16-hip/src/bases.rs) both take the policy from here. */
int csh_bases_table_policy(size_t key_points, int* c_out, int* rows_out);
/* Free the fixed-base tables of a handle (the plain points stay): the fallback when a key's tables do not fit the device. */
int csh_bases_drop_tables(csh_bases_t bases);
/* A copy of a handle -- points and fixed-base tables, as stored -- on GPU `device` (device-to-device, no re-encoding): how one
 * prover places its five independent query MSMs (groth16.rs:227-294, rayon_join5) on several GPUs, and how a party gets its own
 * copy of a key. Free with csh_bases_free. */
int csh_bases_clone(csh_bases_t bases, int device, csh_bases_t* out);
/* The same for the points [offset, offset + n) only (and the matching columns of every table row): a GPU that works on the k-th range
 * of every query (placement by range) holds 1/N of the key instead of all of it. Point i of the clone is point offset + i of the source. */
int csh_bases_clone_range(csh_bases_t bases, size_t offset, size_t n, int device, csh_bases_t* out);
int csh_bases_free(csh_bases_t bases);

/* sum_{i<n} scalars[i] * bases[offset+i].  "unchecked": the caller passes the shorter length
 * (honk_curve.rs:33-34).  scalars_are_montgomery=1 <=> msm_unchecked (&[F]); 0 <=> msm_bigint.
 * out_jacobian: 3 base-field elements (X, Y, Z) on the host. */
int csh_msm(csh_bases_t bases, size_t offset, size_t n, const uint64_t* scalars,
            int scalars_are_montgomery, void* out_jacobian);
/* One MSM per share component over the same bases, from ONE host vector of shares: shares = n entries of ncomp (1 or 2) consecutive
 * field elements, outs[c] = Jacobian result of component c. ncomp = 2 is the Rep3PointShare {a, b} of pointshare::msm_public_points
 * (mpc-core/src/protocols/rep3/pointshare.rs:201-222; call sites CircomPlonkProver::msm_public_points_g1, co-plonk/src/mpc/rep3.rs:170-175,
 * and NoirUltraHonkProver::msm_public_points, co-noir-common/src/mpc/rep3.rs:259-266, which unzip the shares on the host and run two
 * MSMs): here the share vector crosses PCIe once and the components are cut out on the device. */
int csh_msm_shares(csh_bases_t bases, size_t offset, size_t n, const uint64_t* shares, uint32_t ncomp, int scalars_are_montgomery,
                   void* const* outs_jacobian);
int csh_msm_dev(csh_bases_t bases, size_t offset, size_t n, const uint64_t* scalars_dev,
                int scalars_are_montgomery, void* out_jacobian_host, void* stream);
/* Split-MSM building blocks (the entry points below compose them): the un-normalised partial result of one range -- a
 * 32-byte header {magic, c, W} + up to 128 window sums as XYZZ points (4 base-field elements each, arkworks encoding) --
 * left ON THE DEVICE (synchronous: the buffer is complete when the call returns), and the host-side fold of gathered
 * partials. Ranges may use different window widths; an empty range (n = 0) folds as the identity. */
int csh_msm_partial_dev(csh_bases_t bases, size_t offset, size_t n, const uint64_t* scalars_dev,
                        int scalars_are_montgomery, void* out_xyzz_dev /* csh_msm_partial_bytes */,
                        void* stream);
/* ---- one MSM split over the GPUs of a node (BASELINE config 5) ---------------------------------------------
 * Same seam as csh_msm_dev -- the MSM closures of groth16.rs:227-294 -- for a query too large or too urgent for one GPU:
 * the points are cut into contiguous ranges (one csh_bases_t per GPU, uploaded once), every GPU reduces its range to window
 * sums, ONE exchange moves those partial buffers (csh_msm_partial_bytes each, <= 48 KiB) and the host folds them. The
 * exchange is RCCL ncclAllGather over xGMI (bound with dlopen: no link-time dependency, no torch), hipMemcpyPeer to a root
 * device, or one device-to-host copy per GPU. RCCL has no elliptic-curve reduction operator, so this is an all-gather. */
#define CSH_COMM_ID_BYTES 128
typedef struct csh_comm_s* csh_comm_t;
/* One process (or thread) per GPU: rank 0 draws an id (ncclGetUniqueId), ships the 128 bytes to the other ranks by whatever
 * channel the host has, every rank calls csh_comm_init_rank on the thread bound (csh_init) to its GPU. nranks == 1 with
 * id == NULL makes a local communicator without loading RCCL. A communicator is used by one thread at a time.
 * ncclCommInitRank is collective and cannot be interrupted, so with more than one rank the construction runs on a helper thread and the
 * caller waits for it against a deadline -- csh_tune_set("comm_timeout_ms", ms), default 120000, 0 = construct on the calling thread: a
 * rank whose peers never arrive gets CSH_ERR_HIP with "did not come up within ..." instead of a hang (the abandoned helper takes the
 * communicator down itself if the bootstrap ever completes). */
int csh_comm_unique_id(uint8_t id[CSH_COMM_ID_BYTES]);
int csh_comm_init_rank(const uint8_t id[CSH_COMM_ID_BYTES], int nranks, int rank, csh_comm_t* out);
/* One process driving `ndev` distinct GPUs (ncclCommInitAll): out[i] = rank i on devices[i]. */
int csh_comm_init_all(const int* devices, int ndev, csh_comm_t* out);
int csh_comm_info(csh_comm_t comm, int* rank, int* nranks, int* device); /* any out pointer may be NULL */
int csh_comm_destroy(csh_comm_t comm);
/* This rank's share of one split MSM: sum_{i<n} scalars[i] * bases[offset+i] over its own range -> window sums -> all-gather
 * over the communicator -> fold. Every rank receives the full result in out_jacobian (host, as csh_msm). Synchronous;
 * collective: every rank of the communicator must call it (n may be 0 on a rank). A rank whose own range fails on the device still
 * takes part in the exchange with an empty record, so that its peers return an error ("bad partial header") instead of waiting for
 * it; argument errors (NULL pointers, wrong device, range outside the bases) are reported before the collective and must be avoided
 * by the caller on every rank alike. */
int csh_msm_split_rank_dev(csh_comm_t comm, csh_bases_t bases, size_t offset, size_t n, const uint64_t* scalars_dev,
                           int scalars_are_montgomery, void* out_jacobian, void* stream);
/* One thread driving all GPUs: part i = counts[i] points from offsets[i] of bases[i] (a handle on any device; several parts
 * may share a device) with device scalars scalars_dev[i] on that device. The ranges run concurrently on their devices'
 * streams; `mode` picks the exchange. CSH_SPLIT_RCCL needs comms[i] = rank i of csh_comm_init_all over the parts' (distinct)
 * devices; `comms` is ignored otherwise. The calling thread's device binding is restored on return. Synchronous. */
typedef enum { CSH_SPLIT_PEER = 0 /* hipMemcpyPeerAsync to the first part's device */, CSH_SPLIT_HOST = 1 /* one D2H per part */,
               CSH_SPLIT_RCCL = 2 /* grouped ncclAllGather */ } csh_split_mode_t;
int csh_msm_split(const csh_bases_t* bases, const size_t* offsets, const size_t* counts, const uint64_t* const* scalars_dev,
                  size_t k, int scalars_are_montgomery, int mode, const csh_comm_t* comms, void* out_jacobian);

/* k MSMs over ONE device scalar vector -- the four aux-assignment MSMs of a Groth16 proof (a_query, b_g1_query, b_g2_query,
 * l_query: groth16.rs:237-284, calculate_coeff :179-203): the signed-digit decomposition and the bucket sort depend on the
 * scalars only and are computed once. bases[i]: handles of one curve (G1 and G2 may be mixed), each MSM takes n points
 * from offsets[i]; outs_host[i]: Jacobian as csh_msm. Synchronous.
 * On handles with fixed-base tables the sorted list holds table indices (row * handle length + offset + i), so consecutive handles
 * share it only while their (length, offset) pair repeats; a handle with another pair gets its own scatter (~0.2 ms at 2^20). A
 * prover that wants ONE sort for all four uploads the l query behind 1 + n_public padding points (any valid points; never read),
 * which gives it the length and the offset of the a / b queries: the C++ mirror does (host/types.hpp, Query::lead). */
int csh_msm_multi_dev(const csh_bases_t* bases, const size_t* offsets, size_t k, size_t n, const uint64_t* scalars_dev,
                      int scalars_are_montgomery, void* const* outs_host, void* stream);
int csh_msm_partial_bytes(csh_curve_t curve, csh_group_t group, size_t* bytes);
int csh_msm_fold_partials(csh_curve_t curve, csh_group_t group, const void* partials_host, size_t nparts,
                          void* out_jacobian);

/* ---- NTT ------------------------------------------------------------------------------------
 * Replaces taceo_ark_algebra::fft::Domain<F>::{new, with_group_gen, size, ifft_in_to_out,
 * fft_out_to_in}, fft::bit_reverse (reduction.rs:10, 93, 141-174, 249-328) and
 * ark_poly::EvaluationDomain::{fft, ifft} (co-plonk/src/mpc/plain.rs:149-161).
 * `ncomp` = field elements per entry: 1 for F / Shamir shares, 2 for Rep3 shares (DomainCoeff<F>). */
int csh_domain_create(csh_curve_t field_of, uint32_t log_n, const uint64_t group_gen[4] /* Montgomery; NULL =
                      arkworks default 2-adic root (Domain::new) */, csh_domain_t* out);
int csh_domain_size(csh_domain_t dom, size_t* n);
int csh_domain_free(csh_domain_t dom);
/* natural-order evaluations -> coefficients in bit-reversed order (scaled by 1/n) */
int csh_ifft_in_to_out(csh_domain_t dom, uint64_t* data, uint32_t ncomp);
/* bit-reversed coefficients -> natural-order evaluations */
int csh_fft_out_to_in(csh_domain_t dom, uint64_t* data, uint32_t ncomp);
/* natural -> natural (EvaluationDomain::{fft, ifft}); data holds exactly domain-size entries */
int csh_fft(csh_domain_t dom, uint64_t* data, uint32_t ncomp);
int csh_ifft(csh_domain_t dom, uint64_t* data, uint32_t ncomp);
int csh_bit_reverse(csh_curve_t field_of, uint64_t* data, uint32_t log_n, uint32_t ncomp);
/* bit_reversed_coset_table(shift, size) (reduction.rs:45-60): out[bitrev(i)] = shift^i */
int csh_coset_table(csh_domain_t dom, const uint64_t shift[4], uint64_t* out);

int csh_ifft_in_to_out_dev(csh_domain_t dom, uint64_t* data_dev, uint32_t ncomp, void* stream);
int csh_fft_out_to_in_dev(csh_domain_t dom, uint64_t* data_dev, uint32_t ncomp, void* stream);
int csh_fft_dev(csh_domain_t dom, uint64_t* data_dev, uint32_t ncomp, void* stream);
int csh_ifft_dev(csh_domain_t dom, uint64_t* data_dev, uint32_t ncomp, void* stream);
int csh_bit_reverse_dev(csh_curve_t field_of, uint64_t* data_dev, uint32_t log_n, uint32_t ncomp, void* stream);
int csh_coset_table_dev(csh_domain_t dom, const uint64_t shift[4], uint64_t* out_dev, void* stream);

/* ---- element-wise share arithmetic -----------------------------------------------------------
 * `field_of` selects Fr of the curve.  n = number of entries. In-place allowed (out == an input). */
/* out[i] = a[i]*b[i]: plain/Shamir local_mul_vec (mpc/plain.rs:83-89, shamir/arithmetic.rs:73-79) */
int csh_vec_mul(csh_curve_t field_of, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n);
/* out[i] = a[i] +/- b[i], ncomp components per entry (reduction.rs:185-190, rep3/arithmetic.rs:61-82) */
int csh_vec_add(csh_curve_t field_of, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n, uint32_t ncomp);
int csh_vec_sub(csh_curve_t field_of, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n, uint32_t ncomp);
/* v[i] *= table[i] for every component: distribute_powers_and_mul_by_const (mpc.rs:90-94,
 * mpc/rep3.rs:95-106, mpc/shamir.rs:85-96, mpc/plain.rs:91-98; half-share form reduction.rs:166-171) */
int csh_vec_mul_table(csh_curve_t field_of, uint64_t* v, const uint64_t* table, size_t n, uint32_t ncomp);
/* out[i] = l.a*r.a + l.a*r.b + l.b*r.a + mask[i]: Rep3 local_mul_vec (rep3/arithmetic.rs:132-146,
 * arithmetic/ops.rs:69-76); mask = Rep3Rand::masking_field_elements_vec (rngs.rs:137-156). The reference always adds the
 * mask: an unmasked product leaks cross terms once opened, so mask == NULL (and NULL masks / seeds of every protocol-1 entry
 * point below) is refused with CSH_ERR_INVALID (the override "allow_unmasked_rep3" exists only in builds with -DCSH_EXPERIMENTS; pass an all-zero mask vector to test the arithmetic). */
int csh_rep3_local_mul_vec(csh_curve_t field_of, const uint64_t* lhs_ab, const uint64_t* rhs_ab,
                           const uint64_t* mask, uint64_t* out, size_t n);
/* out[i] = in[i].a*x + in[i].b*y: translate_primefield_repshare_vec (bridges/rep3_to_shamir.rs:43-62) */
int csh_rep3_to_shamir_vec(csh_curve_t field_of, const uint64_t* in_ab, const uint64_t x[4],
                           const uint64_t y[4], uint64_t* out, size_t n);
/* out[i] = sum_k coeffs[k] * shares[k][i]: Shamir reconstruct / open_vec (shamir.rs:483-491,
 * shamir/arithmetic.rs:191-213); with coeffs = 1 it is Rep3 combine/open (rep3.rs:583-605,
 * rep3/arithmetic.rs:249-271). `shares` = k host pointers. */
int csh_lincomb(csh_curve_t field_of, const uint64_t* const* shares, const uint64_t* coeffs /* k*4 */,
                size_t k, uint64_t* out, size_t n);

/* ---- field scans: running product, batch inverse, polynomial evaluation, division by (X - z) -------------
 * The whole-vector steps between two transforms of a PLONK / UltraHonk proof that are a scan or a reduction, not element-wise.
 * `field_of`, the limbs, `ncomp` and `stream` as above; n = 0 .. 2^28 (the reference's largest domain). The _dev forms are
 * stream-ordered: no host synchronisation, scratch from the stream's workspace. Outputs are canonical. tune keys "scan_lane_run"
 * (4 or 8 elements per lane), "scan_tile_lanes" (64 / 128 / 256 lanes per tile; a tile is their product), "scan_spine_step"
 * (64 .. 1024, a power of two: tile totals per step of the one-workgroup spine) change the decomposition only, never a result;
 * csh_tune_set refuses other values. */
/* out[i] = in[0] * ... * in[i]: the serial running product of array_prod_mul (co-plonk/src/round2.rs:164-165, impls
 * co-plonk/src/mpc/rep3.rs:211-213, mpc/plain.rs, mpc/shamir.rs). out may equal in. */
int csh_vec_prefix_prod_dev(csh_curve_t field_of, const uint64_t* in_dev, uint64_t* out_dev, size_t n, void* stream);
int csh_vec_prefix_prod(csh_curve_t field_of, const uint64_t* in, uint64_t* out, size_t n);
/* out[i] = in[i]^-1 with ONE field inversion for the whole vector: the per-element y.inverse() of inv_vec / inv_many /
 * inv_many_in_place[_leaking_zeros] (co-noir-common/src/mpc/rep3.rs:208-257, mpc-core rep3/arithmetic.rs:233-246, rep3/detail.rs:487,
 * co-plonk/src/mpc/plain.rs:127-140). A zero stays zero (the rule of inv_many_in_place_leaking_zeros and of ark_ff::batch_inversion);
 * the number of zeros is reported so that inv_vec's caller can bail as the reference does -- CSH_OK either way. out may equal in;
 * zero_count(_dev) may be NULL. */
int csh_vec_batch_inverse_dev(csh_curve_t field_of, const uint64_t* in_dev, uint64_t* out_dev, size_t n, uint64_t* zero_count_dev, void* stream);
int csh_vec_batch_inverse(csh_curve_t field_of, const uint64_t* in, uint64_t* out, size_t n, size_t* zero_count);
/* out[c] = sum_i coeffs[i*ncomp + c] * point^i, c < ncomp (1 = plain / Shamir, 2 = a Rep3 share {a, b}): evaluate_poly_public
 * (co-plonk/src/round4.rs:126-132) and eval_poly (co-noir co_shplemini_prover.rs:382-444, 765; mpc-core rep3/poly.rs:39-68).
 * n == 0 gives 0, point == 0 gives coeffs[0]. `point` is read on the host during the call. */
int csh_eval_poly_dev(csh_curve_t field_of, const uint64_t* coeffs_dev, size_t n, uint32_t ncomp, const uint64_t point[4], uint64_t* out_dev, void* stream);
int csh_eval_poly(csh_curve_t field_of, const uint64_t* coeffs, size_t n, uint32_t ncomp, const uint64_t point[4], uint64_t* out);
/* Division by (X - root), the reference's recurrence from the low coefficients up: c = (-root)^-1, b_(-1) = 0, b_i = c (in[i] - b_(i-1));
 * out = b_0 .. b_(n-2) (n - 1 coefficients x ncomp), rem[c] = b_(n-1) = -root^-n p(root), the element the reference pops: 0 exactly when
 * the division is exact (the reference never checks; Horner from the top agrees with this only then). Polynomial::factor_roots
 * (co-noir/co-noir-common/src/polynomials/polynomial.rs:183) and SharedPolynomial::factor_roots (shared_polynomial.rs:92-140) as the KZG
 * opening (co-noir-common/src/lib.rs:43-47, 68-73) and the Shplonk batched quotient (co_shplemini_prover.rs:661-737,
 * shplemini_prover.rs:594) call them; Round5::div_by_zerofier(inout, 1, beta) for W_xi and W_xiw (co-circom/co-plonk/src/round5.rs:78-91,
 * called at :255 and :274), the same recurrence with c = -beta^-1. Linear, so it acts on every component of a share with no network
 * round. `root` and `sub0` are read on the host during the call. sub0 (ncomp elements, may be NULL) is taken off coefficient 0 as it
 * is loaded -- every call site does quotient[0] -= evaluation first --, `in` itself is not modified. scale (one element, NULL = 1) and
 * accumulate: out[i] = scale b_i, or out[i] += scale b_i (Shplonk's q.add_scaled(&tmp, &nu) without the quotient ever being stored);
 * only out[0 .. n-1) is touched. out may equal in unless accumulating (CSH_ERR_INVALID). rem(_dev) may be NULL. n == 0: nothing, rem =
 * 0; n == 1: no out, rem = c (in[0] - sub0). root == 0 is CSH_ERR_INVALID: that quotient is a shift of the coefficients
 * (factor_roots does remove(0)), which the caller does itself. NOT built: div_by_zerofier with a stride n > 1 (X^n - beta); the
 * reference only ever passes 1. */
int csh_poly_div_linear_dev(csh_curve_t field_of, const uint64_t* in_dev, size_t n, uint32_t ncomp, const uint64_t root[4], const uint64_t* sub0,
                            const uint64_t* scale, int accumulate, uint64_t* out_dev, uint64_t* rem_dev, void* stream);
int csh_poly_div_linear(csh_curve_t field_of, const uint64_t* in, size_t n, uint32_t ncomp, const uint64_t root[4], const uint64_t* sub0,
                        uint64_t* out, uint64_t* rem);

/* ---- multilinear folds: sumcheck and Gemini rounds, MLE evaluation -----------------------------------------
 * out[j] = in[2j] + u (in[2j+1] - in[2j]), the whole-vector arithmetic under an UltraHonk prover's sumcheck rounds and Gemini folds.
 * Linear with a public challenge, so it acts on every component of a Rep3 or Shamir share with no network round. `field_of` is one of the
 * three scalar fields, ncomp 1 or 2, n <= 2^28; challenges are arkworks-Montgomery elements read on the host during the call. An output
 * range that overlaps an input range of the same call is refused (CSH_ERR_INVALID): a fold in place is a race between workgroups, so the
 * reference's in-place loop becomes a ping-pong between two buffers in the caller. Inputs of one call may overlap each other. The _dev
 * forms are stream-ordered: no host synchronisation, scratch from the stream's workspace. Outputs are canonical. tune key "fold_tile_log"
 * (3 .. 11, default 10: a workgroup of the several-rounds kernel folds 2^this many elements on chip, which is also the rounds one launch
 * takes) changes the decomposition only, never a result; csh_tune_set refuses other values. The overlap check compares every output
 * with every input of the call on the host, k^2 comparisons: made for the k = 40 of a sumcheck round, not for thousands of vectors.
 * Outputs that overlap EACH OTHER are not looked for: that is the caller's race. */
/* one round on k vectors of n elements x ncomp: out[v][j] = in[v][2j] + u (in[v][2j+1] - in[v][2j]), j < n/2; n even and >= 2, k >= 1.
 * partially_evaluate_init / partially_evaluate_inplace, every prover polynomial by the round challenge
 * (co-noir/co-ultrahonk/src/co_decider/co_sumcheck/co_sumcheck_prover.rs:34-98, co-noir/ultrahonk/src/decider/sumcheck/sumcheck_prover.rs:20-60).
 * The k pointers travel as kernel arguments, 64 vectors per launch: k > 64 is several launches on the stream, nothing is copied to the device. */
int csh_mle_fold_dev(csh_curve_t field_of, const uint64_t* const* in_dev /* host array of k device ptrs */,
                     uint64_t* const* out_dev, size_t k, size_t n, uint32_t ncomp, const uint64_t u[4], void* stream);
int csh_mle_fold(csh_curve_t field_of, const uint64_t* const* in, uint64_t* const* out, size_t k, size_t n,
                 uint32_t ncomp, const uint64_t u[4]);
/* m rounds on one vector, challenges u[0..m) in order; m >= 1 and 2^m divides n (n need not be a power of two). Level l (1..m) has
 * n / 2^l elements.
 * levels(_dev), may be NULL: levels 1..m back to back, level l at element offset n - n / 2^(l-1), n - n / 2^m elements in all.
 * last(_dev), may be NULL: level m alone. At least one of the two is given.
 * Rounds whose input holds more than 2^21 values (n ncomp) run one per launch, the rest of the chain fused; without
 * levels those leading rounds take n / 2 + n / 4 elements of the stream's workspace.
 * compute_fold_polynomials keeps every level (co_shplemini_prover.rs:236-312, shplemini_prover.rs:198); Polynomial::evaluate_mle /
 * SharedPolynomial::evaluate_mle take `last` with n = 2^m (co-noir-common/src/polynomials/polynomial.rs:270-312,
 * shared_polynomial.rs:154-199; called at co_sumcheck_prover.rs:435 and sumcheck_prover.rs:334). */
int csh_mle_fold_rounds_dev(csh_curve_t field_of, const uint64_t* in_dev, size_t n, uint32_t ncomp, const uint64_t* u /* m*4 */,
                            size_t m, uint64_t* levels_dev, uint64_t* last_dev, void* stream);
int csh_mle_fold_rounds(csh_curve_t field_of, const uint64_t* in, size_t n, uint32_t ncomp, const uint64_t* u,
                        size_t m, uint64_t* levels, uint64_t* last);

/* ---- circom PLONK quotient: the element-wise stages of round 3 ---------------------------------------------
 * Round3::compute_t (co-circom/co-plonk/src/round3.rs:246-502) between its mul_vec network rounds: three loops over the N = 4 n points of the
 * extended domain, then the division by Z_H on coefficient form and the split into t1 / t2 / t3. Affine in the shares with public
 * coefficients, so no network round. protocol 0 = plain / Shamir (ncomp 1), 1 = Rep3 (ncomp 2, {a, b} interleaved), as
 * csh_evaluate_constraints_dev; party_id 0..2 decides where a public value is added (add_with_public, mpc-core/src/protocols/rep3/
 * arithmetic.rs:41-49, shamir/arithmetic.rs:45): protocol 0 and Rep3 party 0 on component a, Rep3 party 1 on b, Rep3 party 2 nowhere.
 * The first three calls take the EXTENDED domain (created with the snarkjs root roots[pow+2], as PlonkDomains does; at least 32 points);
 * the library derives root_of_unity_2 = w^(N/4) and the tables z1, z2, z3 (round3.rs:212-242) from its generator, and the powers w^i on
 * the device. Vectors travel as host arrays of device pointers in the fixed orders given below; a share vector has N ncomp elements, a
 * public vector N. Challenges and blinding shares are host pointers read during the call, arkworks-Montgomery. Stream-ordered: no host
 * synchronisation, scratch from the stream's workspace. Outputs are canonical. CSH_ERR_INVALID before any device work: a NULL pointer, a
 * protocol outside 0..1 or a party outside 0..2, a domain of fewer than 32 points, n < 8 or not a power of two (finish), and any output
 * range that overlaps an input range or another output of the same call -- the rotations by 4 make a call in place a race. */
/* (a) the blinding polynomials on the extended domain, round3.rs:269-274 and 339-353. blinders: the shares b0..b8 (9 ncomp elements).
 * out_dev[0..5) = ap, bp, cp, zp, zwp:  ap[i] = b1 + w^i b0, bp[i] = b3 + w^i b2, cp[i] = b5 + w^i b4, zp[i] = b8 + w^i b7 + w^(2i) b6,
 * zwp[i] = zp[(i + 4) mod N]. */
int csh_plonk_quot_blinders_dev(csh_domain_t ext_dom, uint32_t protocol, uint32_t party_id, const uint64_t* blinders /* host, 9 shares */,
                                uint64_t* const* out_dev /* host array of 5 device ptrs */, void* stream);
/* (b) gate and permutation operands, round3.rs:320-419.
 * shares_dev[0..11) = a, b, c, z, a_b, a_bp, ap_b, ap_bp, ap, bp, cp;  public_dev[0..8) = qm, ql, qr, qo, qc, s1, s2, s3 (the zkey's 4 n
 * evaluations);  lagrange_dev[0..n_public) = the 4 n evaluations of L_1..L_np and buffer_a the n_public shares polys.buffer_a[j] (both may
 * be NULL when n_public = 0);  challenges = beta, gamma, k1, k2 (4 x 4 words).
 * out_dev[0..10) = pi, e1, e1z, e2a, e2b, e2c, e3a, e3b, e3c, e3d:  pi = -sum_j L_(j+1) buffer_a[j];  e1 = (qm a_b + ql a + qr b + qo c + pi)
 * (+) qc;  e1z = qm (a_bp + ap_b + z1[i mod 4] ap_bp) + ql ap + qr bp + qo cp;  e2a, e2b, e2c = a (+) (beta w^i + gamma), b (+) (beta k1 w^i +
 * gamma), c (+) (beta k2 w^i + gamma);  e3a, e3b, e3c = a (+) (beta s1 + gamma), b (+) (beta s2 + gamma), c (+) (beta s3 + gamma);
 * e3d[i] = z[(i + 4) mod N]. e2d is z itself and is not copied. The public-input sum takes its Lagrange pointers as kernel arguments,
 * 16 per launch. */
int csh_plonk_quot_operands_dev(csh_domain_t ext_dom, uint32_t protocol, uint32_t party_id, const uint64_t* const* shares_dev /* 11 */,
                                const uint64_t* const* public_dev /* 8 */, const uint64_t* const* lagrange_dev /* n_public */, size_t n_public,
                                const uint64_t* buffer_a /* host, n_public shares */, const uint64_t* challenges /* host, 4 elements */,
                                uint64_t* const* out_dev /* 10 */, void* stream);
/* (c) combine, round3.rs:88-105 (mul4vec_post) and 435-467.
 * shares_dev[0..14) = e1, e1z, z, zp, e2, e2z_0, e2z_1, e2z_2, e2z_3, e3, e3z_0, e3z_1, e3z_2, e3z_3;  lagrange1_dev = the 4 n evaluations of
 * L_1;  alpha on the host.  out_dev[0..2) = t, tz:  with X = X_0 + z1[i mod 4] X_1 + z2[i mod 4] X_2 + z3[i mod 4] X_3 for X in {e2z, e3z},
 * t = e1 + alpha e2 - alpha e3 + alpha^2 L_1 (z (+) -1),  tz = e1z + alpha e2z - alpha e3z + alpha^2 L_1 zp. */
int csh_plonk_quot_combine_dev(csh_domain_t ext_dom, uint32_t protocol, uint32_t party_id, const uint64_t* const* shares_dev /* 14 */,
                               const uint64_t* lagrange1_dev, const uint64_t alpha[4], uint64_t* const* out_dev /* 2 */, void* stream);
/* (d) finish, round3.rs:468-498, on the coefficient forms ct = ifft(t), ctz = ifft(tz) (4 n shares each); n = zkey.domain_size, a power of two
 * >= 8; b9_b10 = the shares b9, b10 on the host. Division by Z_H per column j < n: q[j] = -ct[j], q[k n + j] = q[(k-1) n + j] - ct[k n + j]
 * (the reference's in-place loop; no divisibility check, as there); tf = q + ctz;  t1_dev (n + 1 shares) = tf[0..n) ++ [b9],
 * t2_dev (n + 1) = tf[n..2n) with t2[0] -= b9, ++ [b10],  t3_dev (n + 6) = tf[2n..3n+6) with t3[0] -= b10. */
int csh_plonk_quot_finish_dev(csh_curve_t field_of, size_t n, uint32_t protocol, uint32_t party_id, const uint64_t* ct_dev,
                              const uint64_t* ctz_dev, const uint64_t* b9_b10 /* host, 2 shares */, uint64_t* t1_dev, uint64_t* t2_dev,
                              uint64_t* t3_dev, void* stream);

/* ---- circom PLONK rounds 2 and 5: z operands, rotation, blinding, the linearisation and opening numerators ----
 * What a device-resident PLONK prover does to whole vectors between the network rounds of Round2::compute_z
 * (co-circom/co-plonk/src/round2.rs:104-155, its rotate_right at :171), in blind_coefficients (co-plonk/src/lib.rs:162-177, rounds 1 and 2)
 * and in Round5::compute_r + compute_wxi (round5.rs:118-259). Affine in the shares with public coefficients, so no network round.
 * protocol, party_id and the add_with_public rule (mpc-core/src/protocols/rep3/arithmetic.rs:41-49, shamir/arithmetic.rs:45) are those of
 * the quotient stages above: a public value goes to component a for protocol 0 and Rep3 party 0, to b for Rep3 party 1, nowhere for
 * Rep3 party 2. Challenges, coefficients and blinding shares are host pointers read during the call, arkworks-Montgomery.
 * Stream-ordered: no host synchronisation, scratch from the stream's workspace. Outputs are canonical. CSH_ERR_INVALID before any device
 * work: a NULL pointer, a protocol outside 0..1 or a party outside 0..2, a size outside the stated range, and any output range that
 * overlaps an input range or another output of the same call. */
/* The operands of the grand product, round2.rs:116-155 (the loop the reference marks "TODO: multithread me"). ext_dom is the EXTENDED
 * domain (N = 4 n >= 32 points, snarkjs root), as the quotient stages take it; w = w_ext^4 generates the n-point domain and its powers are
 * made on the device. shares_dev[0..3) = buffer_a, buffer_b, buffer_c (n shares); sigma_dev[0..3) = the zkey's 4 n evaluations of S1, S2, S3,
 * read at index 4 i; challenges = beta, gamma, k1, k2. out_dev[0..6) = n1, n2, n3, d1, d2, d3 (n shares), for i < n:
 * n1 = a (+) (beta w^i + gamma), n2 = b (+) (beta k1 w^i + gamma), n3 = c (+) (beta k2 w^i + gamma), d1 = a (+) (beta S1[4 i] + gamma),
 * d2 = b (+) (beta S2[4 i] + gamma), d3 = c (+) (beta S3[4 i] + gamma). */
int csh_plonk_z_operands_dev(csh_domain_t ext_dom, uint32_t protocol, uint32_t party_id, const uint64_t* const* shares_dev /* 3 */,
                             const uint64_t* const* sigma_dev /* 3 */, const uint64_t* challenges /* host, 4 elements */,
                             uint64_t* const* out_dev /* 6 */, void* stream);
/* out[(i + k) mod n] = in[i] for n shares of ncomp elements, k < n: buffer_z.rotate_right(1), round2.rs:171. out must not overlap in;
 * n == 0 does nothing. */
int csh_vec_rotate_right_dev(csh_curve_t field_of, const uint64_t* in_dev, uint64_t* out_dev, size_t n, uint32_t ncomp, size_t k, void* stream);
/* blind_coefficients, co-plonk/src/lib.rs:162-177 (called at round1.rs:132 and round2.rs:181), on the polynomial the next MSM reads:
 * poly[j] -= coeff_rev[k - 1 - j] and poly[n + j] = coeff_rev[k - 1 - j] for j < k. poly_dev has room for n + k shares; 1 <= k <= 3 <= n;
 * coeff_rev = k shares on the host. One small launch. */
int csh_plonk_blind_coefficients_dev(csh_curve_t field_of, uint64_t* poly_dev, size_t n, uint32_t ncomp, const uint64_t* coeff_rev /* host, k shares */,
                                     size_t k, void* stream);
/* A ragged linear combination of shared and public polynomials under public coefficients, for i < out_len:
 *   out[i] = sum_{j < ks, i < share_lens[j]} cs_j S_j[i]  (+)  (sum_{j < kp, i < public_lens[j]} cp_j P_j[i] + [i = 0] const0).
 * Lengths (shares, elements) may differ and may be 0 (the pointer is then not looked at); each is at most out_len <= 2^28; positions past
 * every input are written as zero. ks + kp >= 1, ks <= 64, kp <= 64. const0 may be NULL. A coefficient equal to one skips its
 * multiplication. Pointers, lengths and constants travel as kernel arguments, 16 vectors per launch; every input is read once and nothing
 * is copied. out may not overlap any input. Round5::compute_r and compute_wxi, round5.rs:118-259, are ONE call followed by
 * csh_poly_div_linear_dev(root = xi): shares z, t1, t2, t3, a, b, c under e24, -zh, -zh xi^n, -zh xi^2n, v0, v1, v2; public qm, ql, qr, qo,
 * qc, s3, s1, s2 under ea eb, ea, eb, ec, 1, -e3 beta, v3, v4; const0 = r0 - v0 ea - v1 eb - v2 ec - v3 es1 - v4 es2. The batched
 * polynomials of Gemini (shared and public polynomials under powers of rho, compute_batched_polys, co-noir/co-ultrahonk/src/co_decider/co_shplemini/co_shplemini_prover.rs:49-119)
 * are the same call. */
int csh_poly_lincomb_dev(csh_curve_t field_of, uint32_t protocol, uint32_t party_id, const uint64_t* const* shares_dev /* host array of ks device ptrs */,
                         const size_t* share_lens, const uint64_t* share_coeffs /* host, ks elements */, size_t ks,
                         const uint64_t* const* public_dev /* host array of kp device ptrs */, const size_t* public_lens,
                         const uint64_t* public_coeffs /* host, kp elements */, size_t kp, const uint64_t* const0 /* host, may be NULL */,
                         uint64_t* out_dev, size_t out_len, void* stream);

/* ---- co-noir UltraHonk, the Oink phase: w_4 memory records, lookup and z_perm operands, z_perm placement ----
 * The four loops over the whole trace of co-noir/co-ultrahonk/src/co_oink/co_oink_prover.rs (plain twin:
 * co-noir/ultrahonk/src/oink/oink_prover.rs) that sit between a commitment and csh_vec_mul_dev / csh_vec_prefix_prod_dev /
 * csh_vec_batch_inverse_dev. Affine in the shares with public coefficients, so no network round. protocol, party_id and the
 * add_with_public rule are those of the PLONK rounds 2 / 5 section above: protocol 0 = plain / Shamir (ncomp 1), 1 = Rep3 (ncomp 2,
 * {a, b} interleaved); a public value ("x (+) v") goes to component a for protocol 0 and Rep3 party 0, to b for Rep3 party 1, nowhere
 * for Rep3 party 2. Challenges are host pointers read during the call, arkworks-Montgomery. Stream-ordered: no host synchronisation.
 * Outputs are canonical. CSH_ERR_INVALID before any device work: a NULL pointer where one is required, a protocol outside 0..1 or a
 * party outside 0..2, a size outside the stated range, malformed ranges, and any output range that overlaps an input range or another
 * output of the same call.
 * Active ranges (entries 3 and 4): `ranges` is a host array of 2 num_ranges values [start_j, end_j), num_ranges <= 32 (one per
 * non-empty trace block, co-builder/src/keys/plain_proving_key.rs:137-142); every range is non-empty, start_j >= end_(j-1), end <= n.
 * A = sum (end_j - start_j) and idx(t) is the t-th index of the concatenated ranges (ActiveRegionData::get_idx); with num_ranges = 0,
 * idx(t) = t and A = domain_size (= final_active_wire_idx + 1). m = A - 1. The kernels derive idx from the ranges, which travel as kernel
 * arguments with their prefix counts: no index list is uploaded or read. */
/* add_ram_rom_memory_records_to_wire_4 + compute_w4_inner, co_oink_prover.rs:98-160. w_dev[0..3) = w_l, w_r, w_o (n shares), w4_dev (n
 * shares) in place, etas = eta_1, eta_2, eta_3. The index lists are uint32_t arrays on the device (proving-key data, uploaded once). For
 * a read record r: w4[r] += eta_1 w_l[r] + eta_2 w_r[r] + eta_3 w_o[r]; for a write record the same, then (+) 1; for shared record j the
 * same, then + type_share[j] (n_shared shares). One launch covers all n_read + n_write + n_shared records; with all three counts zero the
 * call does nothing. CONTRACT: every index is < n and no index occurs twice in the call, within a list or across lists -- a duplicate
 * would be a race; whoever uploads the lists checks them. The reference's clone + resize of w_4 (:133-137) is csh_poly_lincomb_dev with
 * one share term of coefficient one and out_len = n. */
int csh_honk_w4_records_dev(csh_curve_t field_of, uint32_t protocol, uint32_t party_id, const uint64_t* const* w_dev /* 3 */, uint64_t* w4_dev,
                            size_t n, const uint64_t* etas /* host, 3 elements */, const uint32_t* read_idx_dev, size_t n_read,
                            const uint32_t* write_idx_dev, size_t n_write, const uint32_t* shared_idx_dev, const uint64_t* type_share_dev,
                            size_t n_shared, void* stream);
/* compute_logderivative_inverses + compute_lookup_term + compute_table_term, co_oink_prover.rs:162-293. shares_dev[0..4) = w_l, w_r, w_o,
 * lookup_read_tags (n shares); public_dev[0..9) = q_r, q_m, q_c, q_o, table_1, table_2, table_3, table_4, q_lookup (n elements);
 * challenges = beta, gamma (beta^2, beta^3 are derived here); out_dev[0..2) = prod, sel (n shares); 1 <= n <= 2^28. With sh(w)[i] = w[i + 1]
 * and zero at the last row (Polynomial::shifted, co-noir-common/src/polynomials/polynomial.rs:170-176):
 *   read[i]  = (w_l[i] + q_r[i] sh(w_l)[i]) (+) gamma + beta (w_r[i] + q_m[i] sh(w_r)[i]) + beta^2 (w_o[i] + q_c[i] sh(w_o)[i]) (+) beta^3 q_o[i]
 *   write[i] = table_1[i] + gamma + beta table_2[i] + beta^2 table_3[i] + beta^3 table_4[i]            (public)
 *   prod[i]  = write[i] read[i]                                                                     (mul_with_public)
 *   sel[i]   = ((1 - q_lookup[i]) tag[i]) (+) q_lookup[i]
 * The caller's mul_many(prod, sel) and batch_invert_leaking_zeros are csh_vec_mul_dev (or the Rep3 product) and
 * csh_vec_batch_inverse_dev, which keeps a zero as zero. */
int csh_honk_lookup_operands_dev(csh_curve_t field_of, uint32_t protocol, uint32_t party_id, const uint64_t* const* shares_dev /* 4 */,
                                 const uint64_t* const* public_dev /* 9 */, size_t n, const uint64_t* challenges /* host, 2 elements */,
                                 uint64_t* const* out_dev /* 2 */, void* stream);
/* batched_grand_product_num_denom x 4, co_oink_prover.rs:344-451. shares_dev[0..4) = w_l, w_r, w_o, w_4 (n shares); public_dev[0..8) =
 * id_1..id_4, sigma_1..sigma_4 (n elements); challenges = beta, gamma; out_dev[0..8) = n_1..n_4, d_1..d_4 (m shares each). For t < m and
 * j = idx(t):  n_k[t] = w_k[j] (+) (beta id_k[j] + gamma),  d_k[t] = w_k[j] (+) (beta sigma_k[j] + gamma). 2 <= n <= 2^28,
 * 1 <= domain_size <= n; m = 0 does nothing. */
int csh_honk_perm_operands_dev(csh_curve_t field_of, uint32_t protocol, uint32_t party_id, const uint64_t* const* shares_dev /* 4 */,
                               const uint64_t* const* public_dev /* 8 */, size_t n, size_t domain_size, const size_t* ranges /* host */,
                               size_t num_ranges, const uint64_t* challenges /* host, 2 elements */, uint64_t* const* out_dev /* 8 */,
                               void* stream);
/* The tail of compute_grand_product, co_oink_prover.rs:472-504: mul_dev (m shares, the quotients numerator / denominator) -> z_dev (n
 * shares, every element written; it need not be initialised and may not overlap mul_dev). The result is what the reference leaves: zeros;
 * z[1] = the trivial share of one (0 (+) 1); then z[idx(t + 1)] = mul[t] for t < m, which overwrites z[1] when idx(t + 1) = 1; then, with
 * ranges, z[i] = z[start_(r+1)] for i < domain_size inside a gap [end_r, start_(r+1)). Computed as a gather: each element is written by
 * one lane. 2 <= n <= 2^28, 1 <= domain_size <= n; mul_dev may be NULL when m = 0. */
int csh_honk_z_perm_place_dev(csh_curve_t field_of, uint32_t protocol, uint32_t party_id, const uint64_t* mul_dev, uint64_t* z_dev, size_t n,
                              size_t domain_size, const size_t* ranges /* host */, size_t num_ranges, void* stream);

/* ---- co-noir UltraHonk, the sumcheck round: relation accumulators over the edges, the gate-separator table ----
 * What sits between two csh_mle_fold_dev calls of a device-resident UltraHonk prover (plain field: the `ultrahonk` crate's prover and
 * PlainUltraHonkDriver). Elements are arkworks-Montgomery, 4 words each, one component. Scalars are host pointers read during the call.
 * Stream-ordered: no host synchronisation, scratch from the stream's workspace; the column pointers travel as kernel arguments, nothing
 * is copied to the device for them. Outputs are canonical. CSH_ERR_INVALID before any device work: a NULL pointer where one is required,
 * a field other than BN254 / BLS12-381 / BLS12-377 Fr, a range or size outside the stated rules, an output that overlaps an input. */
/* The loop body of SumcheckProverRound::compute_univariate_inner, co-noir/ultrahonk/src/decider/sumcheck/sumcheck_round_prover.rs:224-255,
 * for edge_idx in (edge_begin..edge_end).step_by(2), restricted to subrelations 0 .. 10 of the batching order (relations/mod.rs:134-145):
 * UltraArithmeticRelation (ultra_arithmetic_relation.rs:126-175), UltraPermutationRelation (permutation_relation.rs:93-167),
 * LogDerivLookupRelation (logderiv_lookup_relation.rs:77-183, :266-309), DeltaRangeConstraintRelation
 * (delta_range_constraint_relation.rs:112-177). The elliptic, memory, non-native field and Poseidon2 relations are
 * csh_honk_sumcheck_accumulate_gates_dev below; the batching of the accumulators into the round univariate (:109-122) stays with the
 * caller.
 * cols_dev[0..36), in this order (part of the ABI):
 *   witness (8)          w_l, w_r, w_o, w_4, z_perm, lookup_inverses, lookup_read_counts, lookup_read_tags
 *   shifted witness (5)  w_l, w_r, w_o, w_4, z_perm  -- vectors of their own, as the reference folds them separately from round 1 on; in
 *                        round 0 a caller may pass `ptr + 1 element` where the length allows
 *   precomputed (23)     q_m, q_c, q_l, q_r, q_o, q_4, q_arith, q_delta_range, q_lookup, sigma_1..4, id_1..4, table_1..4, lagrange_first,
 *                        lagrange_last
 * edge_begin and edge_end are even, edge_begin < edge_end <= 2^28; elements [edge_begin, edge_end) of every column are read. The scaling
 * factor of edge e is scaling_dev[(e >> 1) * scaling_stride] (1 <= scaling_stride <= 2^28), or one for every edge when scaling_dev is NULL.
 * params = beta, gamma, public_input_delta. acc_dev[0..57) = the eleven accumulators back to back: arith.r0 (6), arith.r1 (5), perm.r0 (6),
 * perm.r1 (3), lookup.r0 (5), lookup.r1 (5), lookup.r2 (3), delta.r0 .. r3 (6 each); entry i of an accumulator is its evaluation at the
 * point i; every element is written. acc_dev may not overlap a column or the scaling elements that are read.
 * Per edge: extend_from of the pair col[e], col[e + 1] gives v0 + k (v1 - v0) at the point k; the scaling factor multiplies every
 * subrelation except lookup.r1 (the linearly dependent one); and the reference's skips are part of the result -- arith is left out when
 * q_arith is zero at both ends, perm when z_perm == z_perm_shift at both ends, lookup when q_lookup and lookup_read_counts are zero at both
 * ends, delta when q_delta_range is zero at both ends -- so the words are the reference's on data that does not satisfy the circuit too.
 * The three callers of the reference: the round loop is [0, round_size) with scaling_dev = beta_products and scaling_stride = periodicity;
 * compute_disabled_contribution (:340-386) is the last two or four elements; compute_virtual_contribution (:388-421) is [0, 2) with
 * scaling_dev = NULL. */
int csh_honk_sumcheck_accumulate_dev(csh_curve_t field_of, const uint64_t* const* cols_dev /* host array of 36 device ptrs */, size_t edge_begin,
                                     size_t edge_end, const uint64_t* scaling_dev, size_t scaling_stride,
                                     const uint64_t* params /* host, 3 elements */, uint64_t* acc_dev /* 57 elements */, void* stream);
/* The same loop body (sumcheck_round_prover.rs:224-255, and its callers :340-386 and :388-421) for subrelations 11 .. 27 of the batching
 * order (relations/mod.rs:134-145): EllipticRelation (elliptic_relation.rs:81-161), MemoryRelation (memory_relation.rs:145-358),
 * NonNativeFieldRelation (non_native_field_relation.rs:85-177), Poseidon2ExternalRelation (poseidon2_external_relation.rs:121-205) and
 * Poseidon2InternalRelation (poseidon2_internal_relation.rs:118-200). With csh_honk_sumcheck_accumulate_dev these are the 28 accumulators
 * of accumulate_relation_univariates (:160-222).
 * cols_dev[0..19), in this order (part of the ABI):
 *   witness (4)          w_l, w_r, w_o, w_4
 *   shifted witness (4)  w_l, w_r, w_o, w_4
 *   precomputed (6)      q_m, q_c, q_l, q_r, q_o, q_4
 *   gate selectors (5)   q_elliptic, q_memory, q_nnf, q_poseidon2_external, q_poseidon2_internal
 * The first fourteen are vectors a caller passes to csh_honk_sumcheck_accumulate_dev too. The range, scaling, stream, workspace and overlap
 * rules are that entry's, and so are the three callers. params = eta_1, eta_2, eta_3, curve_b (the constant of the embedded curve
 * y^2 = x^3 + curve_b; HonkCurve::get_curve_b), and the four mat_internal_diag_m_1 values of the Poseidon2 internal matrix: none is
 * built into the library, which is generic over the field. acc_dev[0..110) = seventeen accumulators back to back: elliptic.r0, r1 (6
 * each), memory.r0 .. r5 (6 each), nnf.r0 (6), poseidon2_external.r0 .. r3 (7 each), poseidon2_internal.r0 .. r3 (7 each); entry i of an
 * accumulator is its evaluation at the point i; every element is written. The scaling factor multiplies every subrelation (all seventeen
 * are linearly independent).
 * Skips are per edge and part of the result: each relation is left out when its own selector -- q_elliptic, q_memory, q_nnf,
 * q_poseidon2_external, q_poseidon2_internal -- is zero at both ends of the edge. Every one of these selectors multiplies its whole
 * relation (in memory.r0 the RAM consistency term is added after the product by q_memory * scaling, memory_relation.rs:347-353, and has
 * the factor already), so a skip omits zeros only and the words are the reference's on any data. */
int csh_honk_sumcheck_accumulate_gates_dev(csh_curve_t field_of, const uint64_t* const* cols_dev /* host array of 19 device ptrs */,
                                           size_t edge_begin, size_t edge_end, const uint64_t* scaling_dev, size_t scaling_stride,
                                           const uint64_t* params /* host, 8 elements */, uint64_t* acc_dev /* 110 elements */, void* stream);
/* GateSeparatorPolynomial::new's beta_products, co-noir/ultrahonk/src/decider/types.rs:53-67: out[i] = the product of betas[b] over the
 * set bits b of i, out[0] = 1; 0 <= m <= 28, out_dev holds 2^m elements. The scaling table of csh_honk_sumcheck_accumulate_dev, made where
 * it is read. partially_evaluate and partially_evaluate_with_padding (:96-112) are a few scalar operations per round and stay with the
 * caller. */
int csh_honk_pow_table_dev(csh_curve_t field_of, const uint64_t* betas /* host, m elements */, size_t m, uint64_t* out_dev /* 2^m elements */,
                           void* stream);

/* ---- co-noir UltraHonk, the sumcheck round on shares: the stretches between the network rounds of four relations ----
 * The collaborative prover's form of the round above (co-noir/co-ultrahonk/src/co_decider/; paths below are relative to it) for the
 * arithmetic, permutation, delta-range and log-derivative lookup relations, subrelations 0 .. 10. There a relation is evaluated over a flat
 * batch of 7 m elements per column (m = the kept edges) and calls T::mul_many -- a local product plus one network round -- between
 * stretches of local arithmetic. One entry per stretch; the network stays the caller's: the local product is csh_rep3_local_mul_vec_dev
 * (Rep3) or csh_vec_mul_dev (Shamir, plain), the exchange is the driver's.
 * protocol, party_id and x (+) v are those of the Oink section. cols_dev[0..36) is the column array of csh_honk_sumcheck_accumulate_dev in
 * the same order: the 13 witness and shifted-witness columns are shares (ncomp = protocol + 1 values per element), the 23 precomputed
 * columns are public; a pointer may be NULL for a column the stage does not read (each entry lists what it reads).
 * The batch is never built: batch element t of a column belongs to kept edge j = t / 7 and point k = t % 7 and is
 * col[e] + k (col[e + 1] - col[e]) per component, with e = 2 edge_idx_dev[j], or e = edge_begin + 2 j when edge_idx_dev is NULL (every edge
 * of the range kept, m = (edge_end - edge_begin) / 2). Its scaling element is scaling_dev[(e >> 1) scaling_stride], or one when scaling_dev
 * is NULL. This is extend_edges + fold_and_filter + add_entities (co_sumcheck/co_sumcheck_round.rs:54-73, types_batch.rs:105-130,
 * relations/mod.rs:69-80). CONTRACT: the m values of an edge list lie in [edge_begin / 2, edge_end / 2) -- it is what
 * csh_honk_co_select_edges_dev wrote for the same range.
 * An operand vector holds its parts back to back in the reference's concatenation order, 7 m shares each: the order is part of the ABI,
 * as it is what a reference CPU party puts on the wire.
 * An accumulator is fold_accumulator! (relations/mod.rs:45-57) into zero: entry k = the sum over j of element 7 j + k, cut to the
 * accumulator's length, ncomp values per entry; every entry is written, with m = 0 as zero. The caller adds the accumulators of successive
 * batches (MAX_ROUND_SIZE_PER_BATCH, co_sumcheck_round.rs:270-291). Reductions go through LDS and a finishing launch, with the exact
 * modular addition: the words do not depend on the launch shape. Outputs are canonical. Stream-ordered, no host synchronisation, scratch
 * from the stream's workspace. edge_begin and edge_end are even, edge_begin < edge_end <= 2^28. params = beta, gamma, public_input_delta on
 * the host. CSH_ERR_INVALID before any device work: the causes of csh_honk_sumcheck_accumulate_dev and of the Oink entries, an m that does
 * not fit the range, and an output that overlaps an input or another output. */
/* can_skip of the two relations that have one: selector_dev = q_arith (relations/ultra_arithmetic_relation.rs:247-249) or q_delta_range
 * (delta_range_constraint_relation.rs:94-96). An edge is kept unless the selector is zero at both ends. edge_idx_dev receives the kept
 * e >> 1 ascending (room for (edge_end - edge_begin) / 2 values; the compaction is stable, the order being the wire order), *count_dev
 * their number, which the caller copies back. Permutation and lookup never skip in the shared prover: they pass no list. */
int csh_honk_co_select_edges_dev(csh_curve_t field_of, const uint64_t* selector_dev, size_t edge_begin, size_t edge_end, uint32_t* edge_idx_dev,
                                 uint32_t* count_dev, void* stream);
/* UltraArithmeticRelation, relations/ultra_arithmetic_relation.rs:88-239, one stage, no network. r0_dev: 6 elements of ONE component, a
 * half share: local_mul_vec(w_l, w_r) (Rep3: + mask_dev[t], 7 m elements indexed by the batch element t as the reference draws them,
 * the elements at k = 6 included; protocol 0: the product of the shares, mask_dev NULL) times q_m (q_arith - 3) (-1/2), plus
 * mul_with_public_to_half_share (q w.a) of q_l w_l, q_r w_r, q_o w_o, q_4 w_4 and (q_arith - 1) w_4_shift, plus q_c
 * (add_assign_public_half_share: protocol 0, and Rep3 party 0 only), times q_arith and the scaling. The caller reshares r0
 * (relations/mod.rs:140-162). r1_dev: 5 shares, ((w_l + w_4 - w_l_shift) (+) q_m) (q_arith - 2) (q_arith - 1) q_arith scaling.
 * Reads w_l, w_r, w_o, w_4, w_l_shift, w_4_shift, q_m, q_c, q_l, q_r, q_o, q_4, q_arith. */
int csh_honk_co_arith_dev(csh_curve_t field_of, uint32_t protocol, uint32_t party_id, const uint64_t* const* cols_dev, size_t edge_begin,
                          size_t edge_end, const uint32_t* edge_idx_dev, size_t m, const uint64_t* scaling_dev, size_t scaling_stride,
                          const uint64_t* mask_dev, uint64_t* r0_dev, uint64_t* r1_dev, void* stream);
/* UltraPermutationRelation stage (a), relations/permutation_relation.rs:70-146. With wid_k = w_k (+) (beta id_k + gamma) and
 * wsigma_k = w_k (+) (beta sigma_k + gamma): lhs_dev = [wid_1 | wsigma_1 | wid_3 | wsigma_3], rhs_dev = [wid_2 | wsigma_2 | wid_4 |
 * wsigma_4], 4 * 7 m shares each. The caller runs mul_many(lhs, rhs), then mul_many of the two halves of the result: [numerator |
 * denominator] (:147-149). Reads w_l, w_r, w_o, w_4, sigma_1..4, id_1..4. */
int csh_honk_co_perm_operands_dev(csh_curve_t field_of, uint32_t protocol, uint32_t party_id, const uint64_t* const* cols_dev, size_t edge_begin,
                                  size_t edge_end, const uint32_t* edge_idx_dev, size_t m, const uint64_t* params, uint64_t* lhs_dev,
                                  uint64_t* rhs_dev, void* stream);
/* Stage (b), :226-234: rhs_dev = [z_perm (+) lagrange_first | z_perm_shift (+) lagrange_last public_input_delta], 2 * 7 m shares. The
 * caller runs mul_many([numerator | denominator], rhs). Reads z_perm, z_perm_shift, lagrange_first, lagrange_last. */
int csh_honk_co_perm_operands2_dev(csh_curve_t field_of, uint32_t protocol, uint32_t party_id, const uint64_t* const* cols_dev, size_t edge_begin,
                                   size_t edge_end, const uint32_t* edge_idx_dev, size_t m, const uint64_t* params, uint64_t* rhs_dev,
                                   void* stream);
/* Stage (c), :235-246: prod_dev = that product, 2 * 7 m shares. acc_dev[0..9) shares: perm.r0 (6) = the fold of (first half - second
 * half) scaling, perm.r1 (3) = the fold of lagrange_last z_perm_shift scaling. Reads z_perm_shift, lagrange_last. */
int csh_honk_co_perm_finish_dev(csh_curve_t field_of, uint32_t protocol, uint32_t party_id, const uint64_t* const* cols_dev, size_t edge_begin,
                                size_t edge_end, const uint32_t* edge_idx_dev, size_t m, const uint64_t* scaling_dev, size_t scaling_stride,
                                const uint64_t* prod_dev, uint64_t* acc_dev, void* stream);
/* DeltaRangeConstraintRelation stage (a), relations/delta_range_constraint_relation.rs:146-177. With D_1 = w_r - w_l, D_2 = w_o - w_r,
 * D_3 = w_4 - w_o, D_4 = w_l_shift - w_4: lhs_dev = [D_1 (+) -1 | D_2 (+) -1 | D_3 (+) -1 | D_4 (+) -1 | D_1 (+) -2 | .. | D_4 (+) -2],
 * 8 * 7 m shares. The caller squares it: mul_many(lhs, lhs). Reads w_l, w_r, w_o, w_4, w_l_shift. */
int csh_honk_co_delta_operands_dev(csh_curve_t field_of, uint32_t protocol, uint32_t party_id, const uint64_t* const* cols_dev, size_t edge_begin,
                                   size_t edge_end, const uint32_t* edge_idx_dev, size_t m, uint64_t* lhs_dev, void* stream);
/* Stage (b), :181-183: add_assign_public(-1) on each of the 8 * 7 m shares of sqr_dev, in place. The caller multiplies the two halves.
 * Reads no column; m <= 2^27. */
int csh_honk_co_delta_sub_one_dev(csh_curve_t field_of, uint32_t protocol, uint32_t party_id, uint64_t* sqr_dev, size_t m, void* stream);
/* Stage (c), :187-214: mul_dev = that product, 4 * 7 m shares; every quarter is multiplied by q_delta_range and by the scaling (both
 * cycled over the quarters) and quarter i folds into delta.r_i: acc_dev[0..24) shares, 6 each. Reads q_delta_range. */
int csh_honk_co_delta_finish_dev(csh_curve_t field_of, uint32_t protocol, uint32_t party_id, const uint64_t* const* cols_dev, size_t edge_begin,
                                 size_t edge_end, const uint32_t* edge_idx_dev, size_t m, const uint64_t* scaling_dev, size_t scaling_stride,
                                 const uint64_t* mul_dev, uint64_t* acc_dev, void* stream);
/* LogDerivLookupRelation stage (a), relations/logderiv_lookup_relation.rs:92-139, :263-271: read_term_dev = (q_r w_l_shift + w_l) (+) gamma
 * + beta (q_m w_r_shift + w_r) + beta^2 (q_c w_o_shift + w_o) (+) beta^3 q_o, and inverses_dev = the extended lookup_inverses, so that the
 * product's second operand exists in memory; 7 m shares each. The caller runs mul_many(read_term, inverses) = write_inverse.
 * Reads w_l, w_r, w_o, their shifts, q_r, q_m, q_c, q_o, lookup_inverses. */
int csh_honk_co_lookup_operands_dev(csh_curve_t field_of, uint32_t protocol, uint32_t party_id, const uint64_t* const* cols_dev, size_t edge_begin,
                                    size_t edge_end, const uint32_t* edge_idx_dev, size_t m, const uint64_t* params, uint64_t* read_term_dev,
                                    uint64_t* inverses_dev, void* stream);
/* Stage (b), :77-90, :142-168, :277-295: r0_dev (5 shares) = the fold of (write_term write_inverse - inverse_exists) scaling with
 * write_term = table_1 + gamma + beta table_2 + beta^2 table_3 + beta^3 table_4 and inverse_exists = (tag - q_lookup tag) (+) q_lookup;
 * lhs_dev = [write_inverse | read_tag], rhs_dev = [read_counts | read_tag], 2 * 7 m shares each. The caller runs mul_many(lhs, rhs).
 * Reads table_1..4, lookup_read_tags, lookup_read_counts, q_lookup. */
int csh_honk_co_lookup_mid_dev(csh_curve_t field_of, uint32_t protocol, uint32_t party_id, const uint64_t* const* cols_dev, size_t edge_begin,
                               size_t edge_end, const uint32_t* edge_idx_dev, size_t m, const uint64_t* scaling_dev, size_t scaling_stride,
                               const uint64_t* params, const uint64_t* write_inverse_dev, uint64_t* r0_dev, uint64_t* lhs_dev, uint64_t* rhs_dev,
                               void* stream);
/* Stage (c), :272, :296-309: mul_dev = that product, 2 * 7 m shares. acc_dev[0..8) shares: lookup.r1 (5) = the fold of q_lookup
 * write_term lookup_inverses - mul[0] with NO scaling (the linearly dependent subrelation), lookup.r2 (3) = the fold of (mul[1] -
 * read_tag) scaling. Reads table_1..4, q_lookup, lookup_inverses, lookup_read_tags. */
int csh_honk_co_lookup_finish_dev(csh_curve_t field_of, uint32_t protocol, uint32_t party_id, const uint64_t* const* cols_dev, size_t edge_begin,
                                  size_t edge_end, const uint32_t* edge_idx_dev, size_t m, const uint64_t* scaling_dev, size_t scaling_stride,
                                  const uint64_t* params, const uint64_t* mul_dev, uint64_t* acc_dev, void* stream);

/* ---- co-noir UltraHonk, the sumcheck round on shares: the five gate relations ----
 * The same for the elliptic, memory, non-native field, Poseidon2 external and Poseidon2 internal relations, subrelations 11 .. 27
 * (csrc/honk_co_gates.hip). Everything said above holds -- the element rule, the edge list, m, the scaling, the concatenation order, the
 * accumulators, the reductions, the refusals and the overlap rule -- with these differences. cols_dev[0..19) is the column array of
 * csh_honk_sumcheck_accumulate_gates_dev in the same order: the first eight (w_l, w_r, w_o, w_4 and their shifts) are shares, the other
 * eleven (q_m, q_c, q_l, q_r, q_o, q_4, q_elliptic, q_memory, q_nnf, q_poseidon2_external, q_poseidon2_internal) are public. params, where
 * an entry takes it, is the array of that entry too (eta_1, eta_2, eta_3, curve_b, mat_internal_diag_m_1[0..4); 8 elements on the host);
 * each entry says which of them it reads. The edges of a relation are those kept by csh_honk_co_select_edges_dev on the relation's own
 * selector (can_skip of relations/elliptic_relation.rs:71-73, memory_relation.rs:113-115, non_native_field_relation.rs:63-65,
 * poseidon2_external_relation.rs:92-94, poseidon2_internal_relation.rs:93-95). The Poseidon2 accumulators have 7 entries, all others 6:
 * the element at the point 6 of a batch never reaches a 6-long accumulator. */
/* EllipticRelation stage (a), relations/elliptic_relation.rs:116-168. With x_1 = w_r, y_1 = w_o, x_2 = w_l_shift, y_2 = w_4_shift,
 * x_3 = w_r_shift, y_3 = w_o_shift, x_diff = x_2 - x_1, y_diff = q_l y_2 - y_1: lhs_dev = [y_1 | y_2 | y_1 | x_diff | y_1 + y_3 | y_diff |
 * 3 x_1], rhs_dev = [y_1 | y_2 | y_2 | x_diff | x_diff | x_3 - x_1 | x_1], 7 * 7 m shares each. The caller runs mul1 = mul_many(lhs, rhs).
 * Reads w_r, w_o, the four shifts, q_l. */
int csh_honk_co_ell_operands_dev(csh_curve_t field_of, uint32_t protocol, uint32_t party_id, const uint64_t* const* cols_dev, size_t edge_begin,
                                 size_t edge_end, const uint32_t* edge_idx_dev, size_t m, uint64_t* lhs_dev, uint64_t* rhs_dev, void* stream);
/* Stage (b), :173-195: mul1_dev = that product. lhs_dev = [x_3 + x_2 + x_1 | mul1[0] (+) -curve_b | x_3 + 2 x_1 | mul1[6] | 2 y_1],
 * rhs_dev = [mul1[3] | 3 x_1 | 4 mul1[0] | x_1 - x_3 | y_1 + y_3], 5 * 7 m shares each. The caller runs mul2 = mul_many(lhs, rhs).
 * Reads w_r, w_o, w_l_shift, w_r_shift, w_o_shift; params: curve_b. */
int csh_honk_co_ell_operands2_dev(csh_curve_t field_of, uint32_t protocol, uint32_t party_id, const uint64_t* const* cols_dev, size_t edge_begin,
                                  size_t edge_end, const uint32_t* edge_idx_dev, size_t m, const uint64_t* params, const uint64_t* mul1_dev,
                                  uint64_t* lhs_dev, uint64_t* rhs_dev, void* stream);
/* Stage (c), :199-252. acc_dev[0..12) shares: elliptic.r0 (6) = the fold of (mul2[0] - mul1[1] - mul1[0] + 2 q_l mul1[2]) qn +
 * (mul2[2] - 3 mul2[1]) qd, elliptic.r1 (6) = the fold of (mul1[4] + mul1[5]) qn + (mul2[3] - mul2[4]) qd, with the public factors
 * qd = q_elliptic scaling q_m and qn = q_elliptic scaling - qd (:208-249). Reads q_l, q_m, q_elliptic. */
int csh_honk_co_ell_finish_dev(csh_curve_t field_of, uint32_t protocol, uint32_t party_id, const uint64_t* const* cols_dev, size_t edge_begin,
                               size_t edge_end, const uint32_t* edge_idx_dev, size_t m, const uint64_t* scaling_dev, size_t scaling_stride,
                               const uint64_t* mul1_dev, const uint64_t* mul2_dev, uint64_t* acc_dev, void* stream);
/* MemoryRelation stage (a), relations/memory_relation.rs:241-357. With record = (w_o eta_3 + w_r eta_2 + w_l eta_1) (+) q_c - w_4 (the
 * record check, and neg_access_type), next = w_o_shift eta_3 + w_r_shift eta_2 + w_l_shift eta_1 - w_4_shift, nid = w_l - w_l_shift,
 * idz = nid (+) 1: lhs_dev = [nid | idz | record | idz | next | idz], rhs_dev = [nid | w_4_shift - w_4 | record | w_o_shift - w_o | next |
 * w_r_shift - w_r], 6 * 7 m shares each, the order of :272-357; rhs2_dev = next (+) 1, 7 m shares (:398). The caller runs
 * mul = mul_many(lhs, rhs) and mul2 = mul_many(mul[3], rhs2), whose left operand is part 3 of mul in place. Reads the eight share
 * columns and q_c; params: eta_1, eta_2, eta_3. */
int csh_honk_co_mem_operands_dev(csh_curve_t field_of, uint32_t protocol, uint32_t party_id, const uint64_t* const* cols_dev, size_t edge_begin,
                                 size_t edge_end, const uint32_t* edge_idx_dev, size_t m, const uint64_t* params, uint64_t* lhs_dev,
                                 uint64_t* rhs_dev, uint64_t* rhs2_dev, void* stream);
/* Stage (b), :370-455: mul_dev = 6 * 7 m shares, mul2_dev = 7 m shares. acc_dev[0..36) shares, memory.r0 .. r5 (6 each), with
 * qms = q_memory scaling: r1 = mul[1] q_l q_r qms, r2 = (mul[0] + nid) q_l q_r qms, r3 = mul2 q_o qms, r4 = (mul[0] + nid) q_o qms,
 * r5 = (mul[4] + next) q_o qms, r0 = (record q_l q_r + (mul[5] - w_o) q_4 q_l + record q_m q_l) qms + (mul[2] + record) q_o qms: the RAM
 * consistency term carries q_memory scaling already and is added after the product (:452-453). Reads the eight share columns, q_m, q_c,
 * q_l, q_r, q_o, q_4, q_memory; params: eta_1, eta_2, eta_3. */
int csh_honk_co_mem_finish_dev(csh_curve_t field_of, uint32_t protocol, uint32_t party_id, const uint64_t* const* cols_dev, size_t edge_begin,
                               size_t edge_end, const uint32_t* edge_idx_dev, size_t m, const uint64_t* scaling_dev, size_t scaling_stride,
                               const uint64_t* params, const uint64_t* mul_dev, const uint64_t* mul2_dev, uint64_t* acc_dev, void* stream);
/* NonNativeFieldRelation stage (a), relations/non_native_field_relation.rs:138-150: lhs_dev = [w_l | w_r | w_4 | w_o | w_l_shift],
 * rhs_dev = [w_r_shift | w_l_shift | w_l | w_r | w_r_shift], 5 * 7 m shares each: the extended columns, so that the product's operands
 * exist in memory. The caller runs mul = mul_many(lhs, rhs). Reads w_l, w_r, w_o, w_4, w_l_shift, w_r_shift. */
int csh_honk_co_nnf_operands_dev(csh_curve_t field_of, uint32_t protocol, uint32_t party_id, const uint64_t* const* cols_dev, size_t edge_begin,
                                 size_t edge_end, const uint32_t* edge_idx_dev, size_t m, uint64_t* lhs_dev, uint64_t* rhs_dev, void* stream);
/* Stage (b), :154-213: mul_dev = 5 * 7 m shares. acc_dev[0..6) shares = nnf.r0, the fold of ((gate_1 + gate_2 + gate_3) q_r +
 * (limb_accumulator_1 + limb_accumulator_2) q_o) q_nnf scaling; the constants 2^68 and 2^14 are made on the host per field. Reads the
 * eight share columns, q_m, q_r, q_o, q_4, q_nnf. */
int csh_honk_co_nnf_finish_dev(csh_curve_t field_of, uint32_t protocol, uint32_t party_id, const uint64_t* const* cols_dev, size_t edge_begin,
                               size_t edge_end, const uint32_t* edge_idx_dev, size_t m, const uint64_t* scaling_dev, size_t scaling_stride,
                               const uint64_t* mul_dev, uint64_t* acc_dev, void* stream);
/* Poseidon2ExternalRelation stage (a), relations/poseidon2_external_relation.rs:165-174: s_dev = [w_l (+) q_l | w_r (+) q_r | w_o (+) q_o |
 * w_4 (+) q_4], 4 * 7 m shares. The caller runs the three products of the s-box on vectors it holds: s s, that squared, then times s
 * (:177-179). Reads w_l, w_r, w_o, w_4, q_l, q_r, q_o, q_4. */
int csh_honk_co_pos_ext_operands_dev(csh_curve_t field_of, uint32_t protocol, uint32_t party_id, const uint64_t* const* cols_dev, size_t edge_begin,
                                     size_t edge_end, const uint32_t* edge_idx_dev, size_t m, uint64_t* s_dev, void* stream);
/* Stage (b), :181-226: u_dev = s^5, 4 * 7 m shares. v = M_E u by the reference's 14 additions; acc_dev[0..28) shares:
 * poseidon2_external.r0 .. r3, SEVEN entries each, r_i = the fold of (v_i - w_i_shift) q_poseidon2_external scaling. Reads the four
 * shifts and q_poseidon2_external. */
int csh_honk_co_pos_ext_finish_dev(csh_curve_t field_of, uint32_t protocol, uint32_t party_id, const uint64_t* const* cols_dev, size_t edge_begin,
                                   size_t edge_end, const uint32_t* edge_idx_dev, size_t m, const uint64_t* scaling_dev, size_t scaling_stride,
                                   const uint64_t* u_dev, uint64_t* acc_dev, void* stream);
/* Poseidon2InternalRelation stage (a), relations/poseidon2_internal_relation.rs:155: s1_dev = w_l (+) q_l, 7 m shares. The caller runs the
 * three products of the s-box (:159-161). Reads w_l, q_l. */
int csh_honk_co_pos_int_operands_dev(csh_curve_t field_of, uint32_t protocol, uint32_t party_id, const uint64_t* const* cols_dev, size_t edge_begin,
                                     size_t edge_end, const uint32_t* edge_idx_dev, size_t m, uint64_t* s1_dev, void* stream);
/* Stage (b), :163-223: u1_dev = s1^5, 7 m shares. With u = (u1, w_r, w_o, w_4) and sum = u_1 + u_2 + u_3 + u_4: acc_dev[0..28) shares:
 * poseidon2_internal.r0 .. r3, SEVEN entries each, r_i = the fold of (u_i diag_i + sum - w_i_shift) q_poseidon2_internal scaling. The
 * library builds in no diagonal values. Reads w_r, w_o, w_4, the four shifts, q_poseidon2_internal; params: mat_internal_diag_m_1. */
int csh_honk_co_pos_int_finish_dev(csh_curve_t field_of, uint32_t protocol, uint32_t party_id, const uint64_t* const* cols_dev, size_t edge_begin,
                                   size_t edge_end, const uint32_t* edge_idx_dev, size_t m, const uint64_t* scaling_dev, size_t scaling_stride,
                                   const uint64_t* params, const uint64_t* u1_dev, uint64_t* acc_dev, void* stream);

/* ---- batched Poseidon2: plain, Rep3 and Shamir rounds, Merkle trees ------------------------------------------------
 * The Poseidon2 gadget of mpc-core/src/gadgets/ (paths below are relative to it), d = 5, t = 2, 3 or 4, over a batch of independent
 * states: state i is elements [i t, (i + 1) t) of a vector (chunks_exact_mut(T)). The library builds in no parameter set: the round
 * numbers, the round constants and the diagonal are the caller's (the fields of Poseidon2Params, poseidon2/poseidon2_params.rs).
 * Elements are arkworks Montgomery words, outputs are canonical, the _dev calls are stream-ordered without host synchronisation.
 * protocol, party_id and x (+) v (a public value goes to component a of party 0 and component b of party 1; with protocol 0 to the
 * one component of every party) are those of the Oink section; a share is ncomp = protocol + 1 values, interleaved.
 * CSH_ERR_INVALID before any device work: t outside 2 .. 4, a NULL pointer where one is required, an arity that does not go with the
 * mode, n_leaves that is no power of the arity, a step above the round count, an output range that overlaps an input range or another
 * output of the call. */
/* One parameter set on the device. rc_external: (rounds_f_beginning + rounds_f_end) * t host elements, round after round
 * (round_constants_external); rc_internal: rounds_p host elements; diag_m_1: t host elements (mat_internal_diag_m_1). At t = 2 and
 * t = 3 the internal matrix is the fixed one of matmul_internal (poseidon2/poseidon2_permutation.rs:126-147), so diag_m_1 must be
 * (1, 2) or (1, 1, 2) as the reference asserts there; at t = 4 it is used (:148-160). */
int csh_poseidon2_params_create(csh_curve_t field_of, uint32_t t, uint32_t rounds_f_beginning, uint32_t rounds_f_end, uint32_t rounds_p,
                                const uint64_t* rc_external, const uint64_t* rc_internal, const uint64_t* diag_m_1,
                                csh_poseidon2_params_t* handle);
int csh_poseidon2_params_destroy(csh_poseidon2_params_t handle);
/* permutation_in_place (poseidon2/poseidon2_permutation.rs:194-214) on each of n_perm states: the initial linear layer,
 * rounds_f_beginning external rounds, rounds_p internal rounds, rounds_f_end external rounds whose constants go on at index
 * rounds_f_beginning (:209-213); one launch. out_dev may be state_dev itself; any other overlap is refused. */
int csh_poseidon2_permute_dev(csh_poseidon2_params_t handle, const uint64_t* state_dev, size_t n_perm, uint64_t* out_dev, void* stream);
/* merkle_tree_sponge (mode 0, t > arity; merkle_tree/plain.rs:15-50) and merkle_tree_compression (mode 1, t >= arity; :113-155) of
 * n_leaves = arity^k leaves, k >= 0: root_dev receives one element. One launch per layer, nothing returns to the host in between.
 * work_dev: 2 * (n_leaves / arity) elements of scratch (may be NULL when n_leaves <= arity). */
int csh_poseidon2_merkle_dev(csh_poseidon2_params_t handle, uint32_t arity, uint32_t mode, const uint64_t* leaves_dev, size_t n_leaves,
                             uint64_t* root_dev, uint64_t* work_dev, void* stream);
/* The local stretches of rep3_permutation_in_place_with_precomputation_packed (poseidon2/rep3.rs:612-648, round bodies :516-575,
 * :220-243, :296-310, :358-388) and shamir_permutation_in_place_with_precomputation_packed (poseidon2/shamir.rs:326-365, :75-153,
 * :258-296), one call per network round. With R = rounds_f_beginning + rounds_p + rounds_f_end: step 0 = the initial linear layer and the
 * pre-part of round 0; step s in 1 .. R - 1 = the post-part of round s - 1 and the pre-part of round s; step R = the post-part of the
 * last round. Pre-part: state (+) round constant - r at the s-box positions, written compactly to open_dev (n_perm * t shares in an
 * external round, n_perm in an internal one); the caller opens them (open_vec) and passes the opened values as y_dev to the next step.
 * Post-part: r^5 + 5 y r^4 + 10 y^2 r^3 + 10 y^3 r^2 + 5 y^4 r (+) y^5 at the s-box positions (sbox_rep3_precomp_post,
 * sbox_shamir_precomp_post), then matmul_external or matmul_internal. state_dev (n_perm * t shares, in place) holds the state after
 * the linear layer. precomp_dev: host array of the five device vectors r, r^2, r^3, r^4, r^5 (Poseidon2Precomputations). precomp_offset:
 * precomp.offset at the round whose pre-part the step runs (at step R: after the last round) -- the caller advances it by n_perm * t
 * after an external round and by n_perm after an internal one (rep3.rs:240); an external round reads entry offset + flat state index,
 * an internal one offset + permutation index. ff_out_dev (step 0 only, may be NULL): n_perm shares, element 0 of every state before
 * the linear layer, the feed-forward of the compression tree. handle's field must be field_of. */
int csh_poseidon2_co_round_dev(csh_curve_t field_of, uint32_t protocol, uint32_t party_id, csh_poseidon2_params_t handle, uint32_t step,
                               uint64_t* state_dev, size_t n_perm, const uint64_t* y_dev, const uint64_t* const* precomp_dev /* 5 */,
                               size_t precomp_offset, uint64_t* open_dev, uint64_t* ff_out_dev, void* stream);
/* The next layer of a collaborative tree (merkle_tree/rep3.rs:44-52, :99-111, merkle_tree/shamir.rs the same): state_dev = the len
 * states of a layer after its permutation, ff_dev = len shares (mode 1; ignored in mode 0). next_dev: len / arity states, state i =
 * element 0 of states arity i .. arity i + arity - 1 (+ their feed-forward), zeros after them. len == 1: next_dev is one share, the root.
 * Affine and the same for every party. */
int csh_poseidon2_layer_next_dev(csh_curve_t field_of, uint32_t ncomp, uint32_t t, uint32_t arity, uint32_t mode, const uint64_t* state_dev,
                                 const uint64_t* ff_dev, uint64_t* next_dev, size_t len, void* stream);

/* Rep3 correlated masks generated on the device ("next" row f2): out[i] = from_be_bytes_mod_order(a_i) -
 * from_be_bytes_mod_order(b_i), a_i / b_i = the 32-byte chunks number elem_offset{1,2} + i of the ChaCha12 keystreams
 * of seed1 (own key) and seed2 (previous party's key): byte-compatible with Rep3Rand::masking_field_elements_vec
 * (mpc-core/src/protocols/rep3/rngs.rs:137-156; RngType = rand_chacha::ChaCha12Rng, mpc-core/src/lib.rs:13), so the
 * three parties' masks still cancel. The caller advances its two generators by 32*n bytes. */
int csh_rep3_masks(csh_curve_t field_of, const uint8_t seed1[32], uint64_t elem_offset1, const uint8_t seed2[32],
                   uint64_t elem_offset2, uint64_t* out, size_t n);
int csh_rep3_masks_dev(csh_curve_t field_of, const uint8_t seed1[32], uint64_t elem_offset1, const uint8_t seed2[32],
                       uint64_t elem_offset2, uint64_t* out_dev, size_t n, void* stream);

/* ---- F::rand over a ChaCha12 stream on the device -------------------------------------------------------------------
 * The draws of `F::rand(&mut rng)` for rng = ChaCha12Rng::from_seed(seed) (RngType, mpc-core/src/lib.rs:13): what SeededType::expand_vec
 * (mpc-core/src/protocols/rep3.rs:185-196) and every draw of ShamirRng (mpc-core/src/protocols/shamir/rngs.rs:334-428) make. Candidate k
 * of the stream is keystream bytes [32 k, 32 k + 32) as little-endian limbs with the top limb masked to the modulus bit size; it is
 * accepted iff it is below p, and the accepted limbs are the element's Montgomery words as they stand. ark-ff is not vendored and no
 * reference vector exists: PARITY UNPINNED, as for the seeded share files.
 * out_dev receives the first n accepted candidates at or after candidate cand_begin, in order, canonical by construction. *cand_end (a
 * HOST pointer, may be NULL) receives the index one past the last candidate consumed, so that a call with cand_begin = *cand_end
 * continues the stream; a 32-byte seed draw of the reference (rng.gen::<[u8; 32]>()) is one candidate slot. The output words do not
 * depend on the launch shape (tune "vec_max_blocks", "field_rand_window" change the decomposition only). Unlike the other _dev entries
 * this one reads two words back per window of candidates, so it SYNCHRONISES the stream: once, unless a window sized for n draws plus
 * eight standard deviations falls short (or "field_rand_window" shrinks it) and further windows follow for the remainder. Scratch: 8 KiB
 * of the stream's workspace. CSH_ERR_INVALID: unknown field, NULL seed, NULL out_dev with n > 0, n > 2^28, cand_begin > 2^62. */
int csh_field_rand_dev(csh_curve_t field_of, const uint8_t seed[32], uint64_t cand_begin, size_t n, uint64_t* out_dev, uint64_t* cand_end,
                       void* stream);
/* The decomposition csh_field_rand_dev would give the first window of n > 0 draws at cand_begin under the tune keys in force, without
 * running it: [candidates of the window, workgroups, candidates per workgroup, the field's acceptance rate p / 2^bits times 10^9].
 * Host-only: for tests of the window rule and of chunk boundaries. */
int csh_field_rand_plan(csh_curve_t field_of, size_t n, uint64_t cand_begin, uint64_t out[4]);

/* ---- DN07 double sharings: the preprocessing of a Shamir party -----------------------------------------------------------
 * ShamirRng of mpc-core/src/protocols/shamir/rngs.rs (paths below are relative to mpc-core/src/protocols/) without its network: the
 * handle holds the field, id, num_parties, threshold, the num_parties - 1 shared streams of get_shared_rngs (rngs.rs:98-139; stream q
 * is the one shared with party q for q < id and with party q + 1 otherwise) each as a seed and a position in candidates, the public
 * matrices on the device -- the interpolation polynomials of precompute_interpolation_polys (shamir.rs:503-525) for degree t and 2t
 * evaluated at the points the stages need, and create_vandermonde_matrix (rngs.rs:147-158) -- and the two growing device buffers r_t and
 * r_2t. Exchanging the seeds and the wire vectors is network traffic and stays in the caller. seeds: (num_parties - 1) * 32 host bytes;
 * positions: num_parties - 1 host words or NULL for zeros. CSH_ERR_INVALID: 2 * threshold + 1 > num_parties (ShamirPreprocessing::new,
 * shamir.rs:41-43), threshold 0, id >= num_parties, and num_parties > 16, a limit of this library (the matrices go to the kernel as
 * they are). A handle belongs to the device it was created on and is used by one thread at a time. */
int csh_shamir_rng_create(csh_curve_t field_of, uint32_t id, uint32_t num_parties, uint32_t threshold, const uint8_t* seeds,
                          const uint64_t* positions, csh_shamir_rng_t* handle);
int csh_shamir_rng_destroy(csh_shamir_rng_t handle);
/* The positions of the num_parties - 1 shared streams, in candidates (see csh_field_rand_dev). */
int csh_shamir_rng_positions(csh_shamir_rng_t handle, uint64_t* positions);
/* The shared-stream half of fork_with_pairs (rngs.rs:76-79): one 32-byte seed draw from every shared stream, in stream order, into
 * seeds_out ((num_parties - 1) * 32 host bytes); every position advances by one candidate. Host work only. The child is a new handle
 * created from these seeds; its pairs are a take from the front of this one. */
int csh_shamir_rng_fork_seeds(csh_shamir_rng_t handle, uint8_t* seeds_out);
/* random_double_share (rngs.rs:334-395) up to and including send_share_of_randomness, for `amount` batch items (1 .. 2^24). Per shared
 * stream the draws run in the order of rngs.rs:344-384 -- receive_seeded_next, the sender's draws, receive_seeded_prev, for degree
 * t + 1 and then for 2 t, `amount` draws each -- and advance the handle's positions; polys_t, rands = p[0], polys_2t, the party's own
 * evaluations and the evaluations for the receivers are public linear maps of those draw vectors. send_dev receives the vectors in
 * wire order: `amount` elements per receiver, (id + i + t + 1) mod n for i = 1 .. n - t - 2, then (id + i + 2 t) mod n for
 * i = 1 .. n - 2 t - 1 (rngs.rs:291-311, :387-388). With nothing to send (3 parties, t = 1) it may be NULL. Stream-ordered, but each
 * shared stream's draws synchronise the stream as csh_field_rand_dev does. */
int csh_shamir_double_share_local_dev(csh_shamir_rng_t handle, size_t amount, uint64_t* send_dev, void* stream);
/* The rest of random_double_share and buffer_triples (rngs.rs:390-427): recv_dev holds what receive_share_of_randomness receives, in
 * its order -- `amount` elements from (id - (t + 1) - i) mod n for i = 1 .. n - t - 2, then from (id - 2 t - i) mod n for
 * i = 1 .. n - 2 t - 1 (may be NULL when nothing is received). Applies the Vandermonde matrix to every rcv_t[b] and rcv_2t[b] and appends
 * amount * (threshold + 1) pairs to the handle's buffers, batch item b at [b * (t + 1), (b + 1) * (t + 1)) (chunks_exact_mut). `amount`
 * must be that of the local stage before it. The buffers grow by reallocation, which synchronises. */
int csh_shamir_double_share_finish_dev(csh_shamir_rng_t handle, size_t amount, const uint64_t* recv_dev, void* stream);
/* Hands out `count` pairs, element order. from_front == 0: the pops of get_pair (rngs.rs r_t.pop(); shamir/network.rs:150-167 gives
 * element i of a vector the i-th pop), output element i = buffer element len - 1 - i. from_front != 0: the drain(..count) of
 * fork_with_pairs (rngs.rs:93-94), buffer order. The buffers shrink by count. More than present: CSH_ERR_INVALID and nothing changes
 * (refilling is the caller's decision). With the outputs, csh_vec_mul_dev + csh_vec_add_dev of r_2t is the masked local product of
 * mul_vec and csh_vec_sub_dev of r_t ends the degree reduction. */
int csh_shamir_pairs_take_dev(csh_shamir_rng_t handle, size_t count, int from_front, uint64_t* r_t_out_dev, uint64_t* r_2t_out_dev,
                              void* stream);
int csh_shamir_pairs_len(csh_shamir_rng_t handle, size_t* len);

int csh_vec_mul_dev(csh_curve_t field_of, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n, void* stream);
int csh_vec_add_dev(csh_curve_t field_of, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n, uint32_t ncomp, void* stream);
int csh_vec_sub_dev(csh_curve_t field_of, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n, uint32_t ncomp, void* stream);
int csh_vec_mul_table_dev(csh_curve_t field_of, uint64_t* v, const uint64_t* table, size_t n, uint32_t ncomp, void* stream);
int csh_rep3_local_mul_vec_dev(csh_curve_t field_of, const uint64_t* lhs_ab, const uint64_t* rhs_ab,
                               const uint64_t* mask, uint64_t* out, size_t n, void* stream);
int csh_rep3_to_shamir_vec_dev(csh_curve_t field_of, const uint64_t* in_ab, const uint64_t x[4],
                               const uint64_t y[4], uint64_t* out, size_t n, void* stream);
int csh_lincomb_dev(csh_curve_t field_of, const uint64_t* const* shares_dev /* host array of k device ptrs */,
                    const uint64_t* coeffs, size_t k, uint64_t* out, size_t n, void* stream);

/* ---- fused CircomReduction tail (reduction.rs:135-192) -------------------------------------------
 * Given the constraint evaluations a, b (natural order, n = domain size, ncomp comps per entry) computes
 * h[i] = (A*B - C)(shift * w^i) entirely on the device: 6 NTTs + 2 local_mul_vec + 3 table muls + 1 sub.
 * protocol: 0 plain / Shamir (ncomp 1, out = a*b), 1 Rep3 (ncomp 2, local mul with masks).
 * mask_c / mask_ab: the two mask vectors drawn (in this order) by the two local_mul_vec calls
 * (reduction.rs:160 then :182); NULL for protocol 0.  a and b are clobbered. */
int csh_groth16_h(csh_domain_t dom, const uint64_t shift[4], int protocol, uint64_t* a, uint64_t* b,
                  const uint64_t* mask_c, const uint64_t* mask_ab, uint64_t* h_out);
int csh_groth16_h_dev(csh_domain_t dom, const uint64_t shift[4], int protocol, uint64_t* a_dev, uint64_t* b_dev,
                      const uint64_t* mask_c_dev, const uint64_t* mask_ab_dev, uint64_t* h_out_dev, void* stream);
/* Rep3 variant with the two mask vectors generated on the device from the party's ChaCha12 keys: mask_c = chunks
 * [off, off+n), mask_ab = chunks [off+n, off+2n) of each stream (the order of the two local_mul_vec calls,
 * reduction.rs:160 then :182). Host pointers for a, b, h. */
int csh_groth16_h_rep3_seeded(csh_domain_t dom, const uint64_t shift[4], uint64_t* a, uint64_t* b, const uint8_t seed1[32],
                              uint64_t elem_offset1, const uint8_t seed2[32], uint64_t elem_offset2, uint64_t* h_out);

/* ---- LibSnarkReduction tail (reduction.rs:255-342) -------------------------------------------------
 * a, b: constraint evaluations incl. the promoted public inputs (ncomp per entry), c: half-share evaluations of the C
 * matrix (evaluate_constraint_half_share, 1 component), natural order over Domain::new(n) (csh_domain_create with a
 * NULL generator). generator = F::GENERATOR (Montgomery). h_out[i] = i-th coefficient of (A*B - C)/Z (natural order):
 * 7 NTTs, 1 local_mul_vec (mask = its mask vector, NULL for protocol 0), 4 table multiplications. a, b, c are clobbered.
 * The reference's fixtures for this path (Penumbra BLS12-377 circuits) lack their proving keys: parity is against the
 * oracle's restatement, itself checked on that fixture data with the identity H(t) Z(t) = A(t) B(t) - C(t) (tests/). */
int csh_groth16_h_libsnark(csh_domain_t dom, const uint64_t generator[4], int protocol, uint64_t* a, uint64_t* b, uint64_t* c,
                           const uint64_t* mask, uint64_t* h_out);
int csh_groth16_h_libsnark_dev(csh_domain_t dom, const uint64_t generator[4], int protocol, uint64_t* a_dev, uint64_t* b_dev,
                               uint64_t* c_dev, const uint64_t* mask_dev, uint64_t* h_out_dev, void* stream);

/* ---- sparse constraint evaluation on the device ("next" row f3) ------------------------------------------------
 * Replaces evaluate_constraint over a ConstraintMatrices side (reduction.rs:196-210) + the driver row kernels
 * (mpc/plain.rs:28-43, mpc/rep3.rs:31-49, mpc/shamir.rs:29-49). The matrix (CSR: row_ptr[n_rows+1], col_idx[nnz],
 * Montgomery coeffs[nnz]) is uploaded once per circuit. values = public_inputs || private_witness by column index.
 * protocol 0: plain / Shamir (1 component per value; public terms are added to every share);
 * protocol 1: Rep3 (witness entries are {a, b}; a public term coeff*pub goes to component a on party 0, to component
 *             b on party 1, nowhere on party 2 -- rep3/arithmetic.rs:52-58).
 * out has n_out entries (ncomp components each); rows >= n_rows are zero (the resize to domain_size). */
typedef struct csh_matrix_s* csh_matrix_t;
int csh_matrix_upload(csh_curve_t field_of, const uint64_t* row_ptr, const uint32_t* col_idx, const uint64_t* coeffs,
                      size_t n_rows, size_t nnz, csh_matrix_t* out);
int csh_matrix_free(csh_matrix_t m);
/* rows, non-zeros, the largest column index (every entry point below checks it against the n_public + n_witness the caller
 * states, host or device pointers alike) and the device the handle lives on; any pointer may be NULL */
int csh_matrix_info(csh_matrix_t m, size_t* n_rows, size_t* nnz, uint32_t* max_column, int* device);
int csh_evaluate_constraints_dev(csh_matrix_t m, int protocol, int party_id, const uint64_t* public_dev, size_t n_public,
                                 const uint64_t* witness_dev, size_t n_witness, uint64_t* out_dev, size_t n_out, void* stream);
/* witness_map_from_matrices of CircomReduction (reduction.rs:77-193) entirely on the device: evaluate A and B rows,
 * overwrite the public-input slots a[num_constraints .. +n_public] with the promoted public inputs (:111-113), then the
 * fused pipeline of csh_groth16_h. Host pointers; witness = n_witness entries (1 or 2 components). For protocol 1 the
 * masks come from the ChaCha12 seeds as in csh_groth16_h_rep3_seeded (required for protocol 1; NULL for protocol 0). */
int csh_groth16_witness_map(csh_domain_t dom, const uint64_t shift[4], int protocol, int party_id, csh_matrix_t a, csh_matrix_t b,
                            size_t num_constraints, const uint64_t* public_inputs, size_t n_public, const uint64_t* witness,
                            size_t n_witness, const uint8_t seed1[32], uint64_t elem_offset1, const uint8_t seed2[32],
                            uint64_t elem_offset2, uint64_t* h_out);
/* Same with the witness shares already on the device and h left on the device (feeds csh_msm_dev of h_query directly,
 * groth16.rs:286-292): no PCIe traffic besides the n_public public inputs (host pointer). */
int csh_groth16_witness_map_dev(csh_domain_t dom, const uint64_t shift[4], int protocol, int party_id, csh_matrix_t a, csh_matrix_t b,
                                size_t num_constraints, const uint64_t* public_inputs, size_t n_public, const uint64_t* witness_dev,
                                size_t n_witness, const uint8_t seed1[32], uint64_t elem_offset1, const uint8_t seed2[32],
                                uint64_t elem_offset2, uint64_t* h_out_dev, void* stream);
/* The same map with the two Rep3 mask vectors handed over by the CALLER instead of ChaCha12 seeds: mask_c is the vector the
 * "c: local_mul_vec" draws (reduction.rs:160), mask_ab the one of the last product (:182), n = domain size elements each; NULL for
 * protocol 0. This is the form an unchanged reference can drive in ONE call per witness map: `Rep3Rand`'s generators are private
 * (mpc-core/src/protocols/rep3/rngs.rs:83-86) but `masking_field_elements_vec` (rngs.rs:137-156) is public, and for a generic
 * driver `T::local_mul_vec` of two zero vectors returns exactly the mask (rep3/arithmetic.rs:132-146) -- so the implementor of
 * R1CSToQAP (reduction.rs:27-36) draws both vectors through the public surface, in the reference's order, and passes them here.
 * Host pointers: witness shares (+ masks) up, h down; the pages of h_out are populated from host threads while the device works, so
 * h_out may be freshly allocated, uninitialised memory (Vec::with_capacity + set_len). The _dev variant takes device pointers for the
 * witness shares, the masks and h (public_inputs stays a host pointer) and is asynchronous on `stream` like csh_groth16_witness_map_dev. */
int csh_groth16_witness_map_masks(csh_domain_t dom, const uint64_t shift[4], int protocol, int party_id, csh_matrix_t a, csh_matrix_t b,
                                  size_t num_constraints, const uint64_t* public_inputs, size_t n_public, const uint64_t* witness,
                                  size_t n_witness, const uint64_t* mask_c, const uint64_t* mask_ab, uint64_t* h_out);
int csh_groth16_witness_map_masks_dev(csh_domain_t dom, const uint64_t shift[4], int protocol, int party_id, csh_matrix_t a, csh_matrix_t b,
                                      size_t num_constraints, const uint64_t* public_inputs, size_t n_public, const uint64_t* witness_dev,
                                      size_t n_witness, const uint64_t* mask_c_dev, const uint64_t* mask_ab_dev, uint64_t* h_out_dev,
                                      void* stream);
/* LibSnarkReduction::witness_map_from_matrices (reduction.rs:241-342) on the device: rows of a, b through
 * evaluate_constraint, rows of c through evaluate_constraint_half_share (mpc/rep3.rs:51-74, mpc/shamir.rs:51-68,
 * mpc/plain.rs:45-60), then csh_groth16_h_libsnark. dom = Domain::new (NULL generator at csh_domain_create),
 * generator = F::GENERATOR. Host pointers; one mask vector from the seeds (required for protocol 1). */
int csh_groth16_witness_map_libsnark(csh_domain_t dom, const uint64_t generator[4], int protocol, int party_id, csh_matrix_t a,
                                     csh_matrix_t b, csh_matrix_t c, size_t num_constraints, const uint64_t* public_inputs,
                                     size_t n_public, const uint64_t* witness, size_t n_witness, const uint8_t seed1[32],
                                     uint64_t elem_offset1, const uint8_t seed2[32], uint64_t elem_offset2, uint64_t* h_out);
/* ... and with its ONE mask vector (the local_mul_vec of reduction.rs:289) drawn by the caller, as for csh_groth16_witness_map_masks. */
int csh_groth16_witness_map_libsnark_masks(csh_domain_t dom, const uint64_t generator[4], int protocol, int party_id, csh_matrix_t a,
                                           csh_matrix_t b, csh_matrix_t c, size_t num_constraints, const uint64_t* public_inputs,
                                           size_t n_public, const uint64_t* witness, size_t n_witness, const uint64_t* mask, uint64_t* h_out);

/* ---- measurement hooks (bench.py / profiles) ----------------------------------------------------------
 * HIP-event timing on the stream the kernels are launched on. */
int csh_event_create(void** ev);
int csh_event_record(void* ev, void* stream);
int csh_event_elapsed_ms(void* ev_start, void* ev_stop, float* ms);
int csh_event_destroy(void* ev);
/* Per-MSM stage timings (ms) of the last csh_msm*_dev call on this thread: [digits+histogram, scan,
 * scatter, bucket accumulate, bucket reduce, total]; valid only while csh_tune_set("msm_timing", 1) is in effect. */
int csh_msm_last_timing(float out_ms[6]);
/* Pipeline parameters of the last csh_msm*_dev call on this thread: [window bits c, windows W, entries per lane L,
 * reduction segments S]. */
int csh_msm_last_params(uint32_t out[4]);
/* The plan an n-point MSM on `curve` would run with on the calling thread's device (no device: a 256-CU part is assumed), without
 * running it: [window bits c, windows W, entries per accumulate lane L, window-reduction segments S, accumulate waves, SIMDs].
 * The accumulate kernel takes ceil(waves / SIMDs) rounds of L mixed additions; L and S are chosen so that every SIMD runs a
 * whole number of equal rounds. This is the plan of the G2 groups and of plans shared by several groups
 * (csh_msm_multi_dev); a G1 MSM on its own whose launch would leave SIMDs with fewer accumulate waves than fit them together (below
 * ~2^18 points) runs with a shorter lane, down to 8 entries: csh_msm_last_params reports what ran. Host-only: for capacity planning
 * and for tests of the planner. */
int csh_msm_plan(csh_curve_t curve, size_t n, uint32_t out[6]);

/* ---- synthetic inputs (bench / full-size parity) -------------------------------------------------------
 * out[i] = k_i * G (affine, packed), k_i = csh_util_splitmix64(seed + i) | 1: known discrete logs, so an MSM
 * over them has the closed form (sum_i s_i k_i mod r) * G at any size (SURVEY 8d "known-dlog" family). */
uint64_t csh_util_splitmix64(uint64_t x);
int csh_util_generate_bases_dev(csh_curve_t curve, csh_group_t group, uint64_t seed, size_t n, void* out_dev,
                                void* stream);

#ifdef __cplusplus
}
#endif
#endif /* COSNARKS_HIP_H */
