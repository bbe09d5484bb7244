#!/usr/bin/env python3
"""Device times of the PLONK quotient stages (csrc/plonk_quot.hip) on BN254 Fr, one and two components per share:

  vec_mul     csh_vec_mul_dev on as many values in the same process: the HBM yardstick (one multiplication per 96 B)
  blinders    csh_plonk_quot_blinders_dev   (a): writes 5 share vectors, reads none
  operands    csh_plonk_quot_operands_dev   (b): 11 share + 8 public + n_public Lagrange vectors in, 10 share vectors out (n_public = 1)
  combine     csh_plonk_quot_combine_dev    (c): 14 share vectors + L_1 in, 2 out
  finish      csh_plonk_quot_finish_dev     (d): 2 x 4 n shares in, 3 n + 8 out (N = 4 n)
  compute_t   PlainPlonkDriver::compute_t of the C++ mirror at n = 2^20: wall clock of the whole call, upload and download included

    python tools/plonk_quot_probe.py [--log FILE] [--sizes 22,24] [--mirror-log-n 20]

Every device figure: the call back to back on the calling thread's stream between two HIP events, after bench.py's spin-up rule (untimed
batches for at least 0.3 s until two consecutive batch means agree within 2 %, 3 s at the most); the median of 7 such batches. One JSON line
per (stage, N, ncomp). `bytes` is what the stage MUST move -- every distinct input read once, every output written once -- and TB/s is that
over the time; a stage that reads an input in more than one of its kernels (operands reads a, b, c three times) moves more than that.
The buffers are not initialised: no kernel here has a data-dependent path. Needs a device."""
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
ap.add_argument("--sizes", default="22,24", help="log2 N of the extended domain")
ap.add_argument("--mirror-log-n", type=int, default=20, help="log2 n of the mirror's compute_t (0 = skip)")
args = ap.parse_args()
if not hip.have_device():
    raise SystemExit("plonk_quot_probe: no HIP device (there is no CPU path to time)")
L = hip.lib()
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


def emit(op, N, ncomp, ms, nbytes=None, **extra):
    line = {"op": op, "N": N, "ncomp": ncomp, "ms": round(ms, 5), **extra}
    if nbytes:
        line["bytes"] = nbytes
        line["TB_per_s"] = round(nbytes / ms / 1e9, 3)
    lines.append(line)
    print(json.dumps(line), flush=True)


def limbs(rs, n):
    """n canonical elements as (n, 4) u64: 252 random bits each, below p for BN254 Fr"""
    v = rs.randint(0, 2**64, size=(n, 4), dtype=np.uint64)
    v[:, 3] &= np.uint64((1 << 60) - 1)
    return v


def ptrs(addrs):
    return (C.c_void_p * len(addrs))(*addrs)


rs = np.random.RandomState(12)
settings = {k: B.tune_get(k) for k in ("vec_max_blocks",)}
print(json.dumps({"settings": settings}), flush=True)
lines.append({"settings": settings})
host = limbs(rs, 2 * 16).reshape(-1)   # blinders, buffer_a, challenges, alpha: read on the host during the call
hp = host.ctypes.data_as(C.c_void_p)
u32, sz = C.c_uint32, C.c_size_t
for lg in [int(x) for x in args.sizes.split(",")]:
    N = 1 << lg
    n = N // 4
    dom = hip.Domain(hip.BN254, lg)
    reps = max(3, min(24, (1 << 24) // N * 3))
    public = hip.DeviceBuffer(9 * 32 * N)   # 8 zkey vectors and L_1
    pub = [public.ptr.value + k * 32 * N for k in range(9)]
    for ncomp in (1, 2):
        vb = 32 * N * ncomp
        pool = hip.DeviceBuffer(21 * vb)
        slot = [pool.ptr.value + k * vb for k in range(21)]
        pr = ncomp - 1
        vals = N * ncomp
        emit("vec_mul", vals, 1, measure(lambda: B._check(L.csh_vec_mul_dev(0, C.c_void_p(slot[0]), C.c_void_p(slot[1]), C.c_void_p(slot[2]), sz(vals), None)), reps),
             96 * vals)
        o5 = ptrs(slot[:5])
        emit("blinders", N, ncomp, measure(lambda: B._check(L.csh_plonk_quot_blinders_dev(dom.h, u32(pr), u32(0), hp, o5, None)), reps), 5 * vb)
        sh11, pub8, lag1, o10 = ptrs(slot[:11]), ptrs(pub[:8]), ptrs(pub[8:9]), ptrs(slot[11:21])
        emit("operands", N, ncomp,
             measure(lambda: B._check(L.csh_plonk_quot_operands_dev(dom.h, u32(pr), u32(0), sh11, pub8, lag1, sz(1), hp, hp, o10, None)), reps),
             21 * vb + 9 * 32 * N, n_public=1)
        sh14, o2 = ptrs(slot[:14]), ptrs(slot[14:16])
        emit("combine", N, ncomp,
             measure(lambda: B._check(L.csh_plonk_quot_combine_dev(dom.h, u32(pr), u32(0), sh14, C.c_void_p(pub[8]), hp, o2, None)), reps), 16 * vb + 32 * N)
        t1, t2, t3 = slot[2], slot[3], slot[4]
        emit("finish", N, ncomp,
             measure(lambda: B._check(L.csh_plonk_quot_finish_dev(0, sz(n), u32(pr), u32(0), C.c_void_p(slot[0]), C.c_void_p(slot[1]), hp, C.c_void_p(t1),
                                                                  C.c_void_p(t2), C.c_void_p(t3), None)), reps),
             2 * vb + 32 * ncomp * (3 * n + 8))
        pool.free()
    public.free()
    dom.free()
if args.mirror_log_n:
    from cosnarks_amd import groth16 as dev
    n = 1 << args.mirror_log_n
    evals = limbs(rs, 13 * 4 * n).reshape(-1)   # a, b, c, z, the 8 zkey vectors, L_1
    scalars = limbs(rs, 17).reshape(-1)
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        dev.plonk_compute_t(hip.BN254, n, evals, scalars)
        times.append((time.perf_counter() - t0) * 1e3)
    emit("mirror compute_t (plain, wall clock, upload and download included)", 4 * n, 1, min(times), first_call_ms=round(times[0], 2), n=n, n_public=1)
if args.log:
    with open(args.log, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
