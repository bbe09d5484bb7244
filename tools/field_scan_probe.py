#!/usr/bin/env python3
"""Device times of the field scans (csrc/field_scan.hip) on BN254 Fr: running product, batch inverse, polynomial evaluation and division
by (X - r) (one and two components each), with csh_vec_mul_dev at the same size in the same process as the yardstick (one multiplication, 96 B per element), and the
batch inverse at n = 1, which is the latency of its single inversion plus three launches.

    python tools/field_scan_probe.py [--log FILE]

Every figure: the operation back to back on the calling thread's stream between two HIP events, after bench.py's spin-up rule (untimed
batches for at least 0.3 s until two consecutive batch means agree within 2 %, 3 s at the most); the median of 7 such batches. One JSON
line per (operation, size); needs a device."""
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
ap.add_argument("--tune", default="", help="key=value,... set through csh_tune_set before anything runs (scan_lane_run=4, ...)")
args = ap.parse_args()
if not hip.have_device():
    raise SystemExit("field_scan_probe: no HIP device (there is no CPU path to time)")
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


def emit(op, n, ms, **extra):
    line = {"op": op, "n": n, "ms": round(ms, 5), "ns_per_element": round(ms * 1e6 / n, 3), **extra}
    lines.append(line)
    print(json.dumps(line), flush=True)


def limbs(rs, n):
    """n canonical elements as (n, 4) u64: 253 random bits each, below p for BN254 Fr (any value < p is a valid Montgomery encoding)"""
    v = rs.randint(0, 2**64, size=(n, 4), dtype=np.uint64)
    v[:, 3] &= np.uint64((1 << 60) - 1)
    v[:, 0] |= np.uint64(1)   # never zero
    return v


rs = np.random.RandomState(7)
point = limbs(rs, 1).reshape(4)
settings = {k: B.tune_get(k) for k in ("scan_lane_run", "scan_tile_lanes", "scan_spine_step")}
print(json.dumps({"settings": settings}), flush=True)
lines.append({"settings": settings})
for lg in [int(x) for x in args.sizes.split(",")]:
    n = 1 << lg
    reps = max(3, min(50, (1 << 24) // n * 3))
    a = hip.DeviceBuffer.from_host(limbs(rs, 2 * n))     # 2 n: the two-component polynomial
    b = hip.DeviceBuffer.from_host(limbs(rs, n))
    o = hip.DeviceBuffer(32 * n)
    q = hip.DeviceBuffer(64 * n)                         # the two-component quotient, out of place: `a` stays what it is
    e = hip.DeviceBuffer(64)
    cn = C.c_size_t(n)
    ops = [
        ("vec_mul", lambda: B._check(L.csh_vec_mul_dev(0, a.ptr, b.ptr, o.ptr, cn, None))),
        ("vec_prefix_prod", lambda: B._check(L.csh_vec_prefix_prod_dev(0, a.ptr, o.ptr, cn, None))),
        ("vec_batch_inverse", lambda: B._check(L.csh_vec_batch_inverse_dev(0, a.ptr, o.ptr, cn, None, None))),
        ("eval_poly ncomp=1", lambda: B._check(L.csh_eval_poly_dev(0, a.ptr, cn, 1, point.ctypes.data_as(C.c_void_p), e.ptr, None))),
        ("eval_poly ncomp=2", lambda: B._check(L.csh_eval_poly_dev(0, a.ptr, cn, 2, point.ctypes.data_as(C.c_void_p), e.ptr, None))),
        ("poly_div_linear ncomp=1", lambda: B._check(L.csh_poly_div_linear_dev(0, a.ptr, cn, 1, point.ctypes.data_as(C.c_void_p), None, None, 0, q.ptr, e.ptr, None))),
        ("poly_div_linear ncomp=2", lambda: B._check(L.csh_poly_div_linear_dev(0, a.ptr, cn, 2, point.ctypes.data_as(C.c_void_p), None, None, 0, q.ptr, e.ptr, None))),
    ]
    for name, fn in ops:
        emit(name, n, measure(fn, reps))
    for buf in (a, b, o, q, e):
        buf.free()
one = hip.DeviceBuffer.from_host(limbs(rs, 1))
out1 = hip.DeviceBuffer(32)
emit("vec_batch_inverse", 1, measure(lambda: B._check(L.csh_vec_batch_inverse_dev(0, one.ptr, out1.ptr, C.c_size_t(1), None, None)), 50),
     note="one inversion (a chain of ~330 dependent multiplications on one lane) + three launches")
emit("vec_prefix_prod", 1, measure(lambda: B._check(L.csh_vec_prefix_prod_dev(0, one.ptr, out1.ptr, C.c_size_t(1), None)), 50),
     note="three launches, no inversion: the difference to the line above is the inversion")
two = hip.DeviceBuffer.from_host(limbs(rs, 2))
rem1 = hip.DeviceBuffer(64)
for ncomp in (1, 2):
    emit("poly_div_linear ncomp=%d" % ncomp, 1, measure(lambda: B._check(L.csh_poly_div_linear_dev(
        0, two.ptr, C.c_size_t(1), ncomp, point.ctypes.data_as(C.c_void_p), None, None, 0, None, rem1.ptr, None)), 50),
        note="one host inversion and ~30 host squarings + three launches")
if args.log:
    with open(args.log, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
