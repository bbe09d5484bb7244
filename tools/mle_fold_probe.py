#!/usr/bin/env python3
"""Device times of the multilinear folds (csrc/mle_fold.hip) on BN254 Fr, one and two components:

  vec_mul          csh_vec_mul_dev at the same size in the same process: the HBM yardstick (one multiplication per 96 B)
  fold k=1, k=40   one csh_mle_fold_dev round on 1 and on 40 vectors (one multiplication per 64 B read + 32 B written)
  rounds           csh_mle_fold_rounds_dev, m = log2 n rounds, with every level kept and with none (last only), each next to the same
                   chain as m one-round calls (which keeps every level by construction)
  host             the same chain's arithmetic in oracle/c on ONE host thread (sub, mul, add per pair): the reference runs this loop
                   serially. A separate column: wall clock, not device events.

    python tools/mle_fold_probe.py [--log FILE] [--sizes 12,16,20,24] [--tune fold_tile_log=10]

Every device figure: the operation back to back on the calling thread's stream between two HIP events, after bench.py's spin-up rule
(untimed batches for at least 0.3 s until two consecutive batch means agree within 2 %, 3 s at the most); the median of 7 such batches.
One JSON line per (operation, size, ncomp); needs a device. TB/s counts the bytes the operation has to move: 96 B per output value of one
round."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import cosnarks_amd as hip
from cosnarks_amd import bindings as B

ap = argparse.ArgumentParser()
ap.add_argument("--log", default=None, help="also append the lines to this file")
ap.add_argument("--sizes", default="12,16,20,24")
ap.add_argument("--tune", default="", help="key=value,... set through csh_tune_set before anything runs (fold_tile_log=10, ...)")
ap.add_argument("--no-host", action="store_true", help="skip the host column")
ap.add_argument("--max-gib", type=float, default=16.0, help="skip k = 40 where its buffers would exceed this")
args = ap.parse_args()
if not hip.have_device():
    raise SystemExit("mle_fold_probe: no HIP device (there is no CPU path to time)")
L = hip.lib()
for kv in filter(None, args.tune.split(",")):
    B.tune_set(kv.split("=")[0], int(kv.split("=")[1]))
e0, e1 = B.Event(), B.Event()
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
    return statistics.median(batch_ms(fn, reps) for _ in range(7))


def emit(op, n, ncomp, ms, nbytes=None, **extra):
    line = {"op": op, "n": n, "ncomp": ncomp, "ms": round(ms, 5), **extra}
    if nbytes:
        line["TB_per_s"] = round(nbytes / ms / 1e9, 3)
    lines.append(line)
    print(json.dumps(line), flush=True)


def limbs(rs, n):
    """n canonical elements as (n, 4) u64: 252 random bits each, below p for BN254 Fr (any value < p is a valid Montgomery encoding)"""
    v = rs.randint(0, 2**64, size=(n, 4), dtype=np.uint64)
    v[:, 3] &= np.uint64((1 << 60) - 1)
    return v


def ptrs(addrs):
    return (C.c_void_p * len(addrs))(*addrs)


rs = np.random.RandomState(11)
settings = {k: B.tune_get(k) for k in ("fold_tile_log", "vec_max_blocks")}
print(json.dumps({"settings": settings}), flush=True)
lines.append({"settings": settings})
K = 40
for lg in [int(x) for x in args.sizes.split(",")]:
    n = 1 << lg
    reps = max(3, min(50, (1 << 24) // n * 3))
    us = limbs(rs, lg).reshape(-1)
    up = us.ctypes.data_as(C.c_void_p)
    for ncomp in (1, 2):
        vals = n * ncomp
        a = hip.DeviceBuffer.from_host(limbs(rs, vals))
        b = hip.DeviceBuffer.from_host(limbs(rs, vals))
        o = hip.DeviceBuffer(32 * vals)          # vec_mul's output; levels 1..m of a chain (n - 1 elements)
        last = hip.DeviceBuffer(32 * ncomp)
        cn = C.c_size_t(n)
        emit("vec_mul", vals, 1, measure(lambda: B._check(L.csh_vec_mul_dev(0, a.ptr, b.ptr, o.ptr, C.c_size_t(vals), None)), reps), 96 * vals)
        i1, o1 = ptrs([a.ptr.value]), ptrs([o.ptr.value])
        emit("fold k=1", n, ncomp, measure(lambda: B._check(L.csh_mle_fold_dev(0, i1, o1, C.c_size_t(1), cn, ncomp, up, None)), reps), 48 * vals)
        if K * 48 * vals <= args.max_gib * 2**30:
            big_in, big_out = hip.DeviceBuffer(K * 32 * vals), hip.DeviceBuffer(K * 16 * vals)   # not initialised: the kernel has no data-dependent path
            ik, ok = ptrs([big_in.ptr.value + v * 32 * vals for v in range(K)]), ptrs([big_out.ptr.value + v * 16 * vals for v in range(K)])
            emit("fold k=40", n, ncomp, measure(lambda: B._check(L.csh_mle_fold_dev(0, ik, ok, C.c_size_t(K), cn, ncomp, up, None)), max(3, reps // 8)),
                 K * 48 * vals)
            big_in.free()
            big_out.free()
        else:
            emit("fold k=40", n, ncomp, float("nan"), note="NOT MEASURED: buffers above --max-gib")

        def chain():
            src, at = a.ptr.value, 0
            for l in range(lg):
                dst = o.ptr.value + at
                B._check(L.csh_mle_fold_dev(0, ptrs([src]), ptrs([dst]), C.c_size_t(1), C.c_size_t(n >> l), ncomp, C.c_void_p(us.ctypes.data + 32 * l), None))
                src, at = dst, at + 32 * ncomp * (n >> (l + 1))
        chain_bytes = 96 * ncomp * (n - 1)       # every level read once and written once, round by round
        emit("chain of one-round calls", n, ncomp, measure(chain, max(3, reps // 4)), chain_bytes, rounds=lg)
        emit("rounds, levels kept", n, ncomp,
             measure(lambda: B._check(L.csh_mle_fold_rounds_dev(0, a.ptr, cn, ncomp, up, C.c_size_t(lg), o.ptr, last.ptr, None)), max(3, reps // 2)),
             64 * ncomp * n, rounds=lg)
        emit("rounds, last only", n, ncomp,
             measure(lambda: B._check(L.csh_mle_fold_rounds_dev(0, a.ptr, cn, ncomp, up, C.c_size_t(lg), None, last.ptr, None)), max(3, reps // 2)),
             32 * ncomp * n, rounds=lg)
        if not args.no_host:
            from oracle import cbridge as cb
            host = a.to_host().reshape(n, ncomp, 4)
            t = 0.0
            for l in range(lg):
                even, odd = np.ascontiguousarray(host[0::2]).reshape(-1), np.ascontiguousarray(host[1::2]).reshape(-1)
                ub = np.ascontiguousarray(np.broadcast_to(us[4 * l:4 * l + 4], (even.size // 4, 4))).reshape(-1)
                t0 = time.perf_counter()
                d = cb.vec_sub(0, odd, even, threads=1)
                d = cb.vec_mul(0, d, ub, threads=1)
                nxt = cb.vec_add(0, even, d, threads=1)
                t += time.perf_counter() - t0
                host = np.asarray(nxt).reshape(-1, ncomp, 4)
            got = last.to_host()
            emit("host chain, oracle/c, 1 thread", n, ncomp, t * 1e3, rounds=lg, agrees_with_device=bool(np.array_equal(got, host.reshape(-1))))
        for buf in (a, b, o, last):
            buf.free()
if args.log:
    with open(args.log, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
