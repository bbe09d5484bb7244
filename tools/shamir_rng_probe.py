#!/usr/bin/env python3
"""Device times of the F::rand stream and the DN07 double-share stages (csrc/field_rand.hip, csrc/shamir_rng.hip) on BN254 Fr:

    python tools/shamir_rng_probe.py [--log FILE] [--sizes 10,16,20,24] [--pairs 20,24] [--host-loop PROGRAM]

  host_loop    with --host-loop: the host mirror's loops on one thread at 2^16 -- SeededShare::expand() (host/sharefile.hpp) and a host
               buffer_triples of one party of three -- run by the built examples/shamir_preprocessing_from_cpp.cpp in processes of its own
               before anything is timed on the device. They say what the mirror's caller gains, not what a Rust caller would.
  field_rand   csh_field_rand_dev at 2^10 .. 2^24 draws: draws/s, candidates/s (two passes over them, one ChaCha12 block per two) and
               the bytes written; the call synchronises the stream once, which is inside the figure
  preprocess   the full (3, 1) preprocessing of one party for 2^20 and 2^24 pairs: csh_shamir_double_share_local_dev (two streams, four
               batches each) + csh_shamir_double_share_finish_dev, and the drain of the pairs (csh_shamir_pairs_take_dev) beside it
  vec_mul      csh_vec_mul_dev at 2^20 in the same process: a kernel that only loads, multiplies and stores

Every figure: the call back to back on the calling thread's stream between two HIP events, after bench.py's spin-up rule (untimed batches
for at least 0.3 s until two consecutive batch means agree within 2 %, 3 s at the most); the median of 7 such batches with the lowest and
the highest beside it. One JSON line per figure, one process. Needs a device."""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import cosnarks_amd as hip
from cosnarks_amd import bindings as B

ap = argparse.ArgumentParser()
ap.add_argument("--log", default=None, help="also append the lines to this file")
ap.add_argument("--sizes", default="10,16,20,24", help="log2 of the draw counts of csh_field_rand_dev")
ap.add_argument("--pairs", default="20,24", help="log2 of the pair counts of the (3, 1) preprocessing")
ap.add_argument("--host-loop", default=None, help="examples/shamir_preprocessing_from_cpp.cpp, built: adds the host mirror's one-thread loops")
args = ap.parse_args()
if not hip.have_device():
    raise SystemExit("shamir_rng_probe: no HIP device (there is no CPU path to time)")
L = hip.lib()
e0, e1 = B.Event(), B.Event()
SEED = bytes(range(40, 72))
lines = []


def batch_ms(fn, reps):
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    return e0.elapsed_ms(e1) / reps


def measure(fn, reps):
    fn()
    B.sync()
    t0, prev = time.perf_counter(), None
    while True:
        cur = batch_ms(fn, reps)
        el = time.perf_counter() - t0
        if el >= 3.0 or (el >= 0.3 and prev is not None and abs(cur - prev) <= 0.02 * prev):
            break
        prev = cur
    b = sorted(batch_ms(fn, reps) for _ in range(7))
    return statistics.median(b), b[0], b[-1]


def emit(op, m, **extra):
    ms, lo, hi = m
    line = {"op": op, "ms": round(ms, 5), "ms_min": round(lo, 5), "ms_max": round(hi, 5), **extra}
    lines.append(line)
    print(json.dumps(line), flush=True)


host = {}
if args.host_loop:
    runs = []
    for _ in range(7):
        r = subprocess.run([args.host_loop, "--host-loop", str(1 << 16)], capture_output=True, text=True, timeout=120, check=True)
        runs.append((float(re.search(r"expand_ns_per_draw=([0-9.]+)", r.stdout).group(1)), float(re.search(r"buffer_triples_ns_per_pair=([0-9.]+)", r.stdout).group(1))))
    ex, bt = sorted(x for x, _ in runs), sorted(y for _, y in runs)
    host = {"draws_per_s": 1e9 / ex[3], "pairs_per_s": 1e9 / bt[3]}
    line = {"op": "host_loop", "log_n": 16, "threads": 1, "expand_ns_per_draw": ex[3], "expand_ns_min": ex[0], "expand_ns_max": ex[-1],
            "buffer_triples_ns_per_pair": bt[3], "triples_ns_min": bt[0], "triples_ns_max": bt[-1]}
    lines.append(line)
    print(json.dumps(line), flush=True)

for lg in [int(x) for x in args.sizes.split(",")]:
    n = 1 << lg
    out = hip.DeviceBuffer(32 * n)
    _, end = hip.field_rand(hip.BN254, SEED, 0, n, out=out)
    m = measure(lambda: hip.field_rand(hip.BN254, SEED, 0, n, out=out), 20 if lg < 20 else 3)
    cands, wgs, chunk, rate = hip.field_rand_plan(hip.BN254, n)
    beside = {"times_host": round(n / m[0] * 1e3 / host["draws_per_s"], 1)} if host else {}
    emit("field_rand", m, log_n=lg, draws_per_s=round(n / m[0] * 1e3), window_cands=cands, cands_consumed=end, workgroups=wgs, launches=3,
         Gcand_per_s_two_passes=round(2 * cands / m[0] / 1e6, 3), GB_per_s_written=round(32 * n / m[0] / 1e6, 2), **beside)

n = 1 << 20
rs = np.random.RandomState(3)
raw = rs.randint(0, 2**63, size=(2 * n, 4), dtype=np.int64).astype(np.uint64)
raw[:, 3] &= np.uint64((1 << 60) - 1)
a, b, out = hip.DeviceBuffer.from_host(raw[:n].reshape(-1)), hip.DeviceBuffer.from_host(raw[n:].reshape(-1)), hip.DeviceBuffer(32 * n)
m = measure(lambda: B._check(L.csh_vec_mul_dev(hip.BN254, a.ptr, b.ptr, out.ptr, C.c_size_t(n), None)), 20)
emit("vec_mul", m, log_n=20, Gmul_per_s=round(n / m[0] / 1e6, 2))
del a, b, out

for lg in [int(x) for x in args.pairs.split(",")]:
    pairs = 1 << lg
    items = pairs // 2  # t + 1 = 2 pairs per batch item
    party = hip.ShamirRng(hip.BN254, 0, 3, 1, [SEED, bytes(range(1, 33))])
    r_t, r_2t = hip.DeviceBuffer(32 * pairs), hip.DeviceBuffer(32 * pairs)

    def generate():
        party.double_share_local(items)
        party.double_share_finish(items)

    def whole():
        generate()
        party.take(pairs, True, r_t, r_2t)

    mw = measure(whole, 1 if lg >= 24 else 3)
    generate()
    B.sync()

    def drain():
        party.take(pairs, True, r_t, r_2t)

    e0.record()
    drain()
    e1.record()
    drain_ms = e0.elapsed_ms(e1)
    beside = {"times_host": round(pairs / mw[0] * 1e3 / host["pairs_per_s"], 1)} if host else {}
    emit("preprocess", mw, parties=3, threshold=1, log_pairs=lg, draws=8 * items, pairs_per_s=round(pairs / mw[0] * 1e3), drain_ms_once=round(drain_ms, 5),
         stream_syncs=2, launches=2 * 3 + 4 + 1, **beside)
    party.free()
B.sync()
if args.log:
    with open(args.log, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
