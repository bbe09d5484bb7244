#!/usr/bin/env python3
"""Device times of the Oink entries (csrc/honk_oink.hip) on BN254 Fr, one and two components per share:

  vec_mul          csh_vec_mul_dev on as many values in the same process: the HBM yardstick (one multiplication per 96 B)
  w4_records       csh_honk_w4_records_dev: n / 64 records (every 64th row; a third each read, write and shared)
  lookup_operands  csh_honk_lookup_operands_dev: 4 share vectors and 9 public vectors in, 2 share vectors out
  perm_operands    csh_honk_perm_operands_dev: 4 share vectors and 8 public vectors in, 8 share vectors out; without ranges
                   (domain_size = n) and with 10 active ranges that cover 7/8 of the trace
  z_perm_place     csh_honk_z_perm_place_dev, without and with the same ranges

    python tools/honk_oink_probe.py [--log FILE] [--sizes 20,22]

Every figure: the call back to back on the calling thread's stream between two HIP events, after bench.py's spin-up rule (untimed batches
for at least 0.3 s until two consecutive batch means agree within 2 %, 3 s at the most); the median of 7 such batches, with the lowest and
the highest of the 7 beside it. One JSON line per (stage, n, ncomp). `bytes` is what the stage MUST move -- every distinct input element
read once, every output written once -- and TB/s is that over the time. The field buffers are not initialised: no kernel here has a
data-dependent path. Needs a device."""
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
ap.add_argument("--sizes", default="20,22", help="log2 n of the trace")
args = ap.parse_args()
if not hip.have_device():
    raise SystemExit("honk_oink_probe: no HIP device (there is no CPU path to time)")
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
    b = sorted(batch_ms(fn, reps) for _ in range(7))
    return statistics.median(b), b[0], b[-1]


def emit(op, n, ncomp, m, nbytes=None, **extra):
    ms, lo, hi = m
    line = {"op": op, "n": n, "ncomp": ncomp, "ms": round(ms, 5), "ms_min": round(lo, 5), "ms_max": round(hi, 5), **extra}
    if nbytes:
        line["bytes"] = nbytes
        line["TB_per_s"] = round(nbytes / ms / 1e9, 3)
    lines.append(line)
    print(json.dumps(line), flush=True)


def ptrs(addrs):
    return (C.c_void_p * len(addrs))(*addrs)


rs = np.random.RandomState(13)
settings = {k: B.tune_get(k) for k in ("vec_max_blocks",)}
print(json.dumps({"settings": settings}), flush=True)
lines.append({"settings": settings})
host = rs.randint(0, 2**64, size=(16, 4), dtype=np.uint64)   # challenges: read on the host during the call
host[:, 3] &= np.uint64((1 << 60) - 1)                       # 252 random bits each: below p for BN254 Fr
hp = host.ctypes.data_as(C.c_void_p)
u32, sz = C.c_uint32, C.c_size_t
for lg in [int(x) for x in args.sizes.split(",")]:
    n = 1 << lg
    reps = max(3, min(24, (1 << 22) // n * 3))
    public = hip.DeviceBuffer(9 * 32 * n)
    pub = [public.ptr.value + k * 32 * n for k in range(9)]
    rows = np.arange(0, n, 64, dtype=np.uint32)
    third = rows.size // 3
    rec = hip.HonkMemoryRecords(n, rows[:third], rows[third:2 * third], rows[2 * third:])
    n_rec, n_shared = rows.size, rows.size - 2 * third
    step = n // 10
    ranges = [(j * step + step // 8, (j + 1) * step) for j in range(10)]   # 10 blocks, the first eighth of each inactive
    flat = (sz * 20)(*[x for r in ranges for x in r])
    active = sum(e - s for s, e in ranges)
    for ncomp in (1, 2):
        sb = 32 * ncomp
        vb = sb * n
        pool = hip.DeviceBuffer(13 * vb)
        slot = [pool.ptr.value + k * vb for k in range(13)]
        pr = ncomp - 1
        vals = n * ncomp
        emit("vec_mul", vals, 1, measure(lambda: B._check(L.csh_vec_mul_dev(0, C.c_void_p(slot[0]), C.c_void_p(slot[1]), C.c_void_p(slot[2]), sz(vals), None)), reps),
             96 * vals)
        w3 = ptrs(slot[:3])
        emit("w4_records", n, ncomp, measure(lambda: B._check(L.csh_honk_w4_records_dev(
            0, u32(pr), u32(0), w3, C.c_void_p(slot[3]), sz(n), hp, rec.bufs[0].ptr, sz(rec.counts[0]), rec.bufs[1].ptr, sz(rec.counts[1]), rec.bufs[2].ptr,
            C.c_void_p(slot[4]), sz(rec.counts[2]), None)), reps), n_rec * (5 * sb + 4) + n_shared * sb, records=int(n_rec))
        sh4, pb9, o2 = ptrs(slot[:4]), ptrs(pub), ptrs(slot[4:6])
        emit("lookup_operands", n, ncomp, measure(lambda: B._check(L.csh_honk_lookup_operands_dev(0, u32(pr), u32(0), sh4, pb9, sz(n), hp, o2, None)), reps),
             6 * sb * n + 9 * 32 * n)
        pb8, o8 = ptrs(pub[:8]), ptrs(slot[4:12])
        for name, rg, nr, m in (("no ranges", None, 0, n - 1), ("10 ranges", flat, 10, active - 1)):
            emit("perm_operands, " + name, n, ncomp, measure(lambda: B._check(L.csh_honk_perm_operands_dev(
                0, u32(pr), u32(0), sh4, pb8, sz(n), sz(n), rg, sz(nr), hp, o8, None)), reps), 12 * sb * m + 8 * 32 * m, rows=m)
            emit("z_perm_place, " + name, n, ncomp, measure(lambda: B._check(L.csh_honk_z_perm_place_dev(
                0, u32(pr), u32(0), C.c_void_p(slot[0]), C.c_void_p(slot[1]), sz(n), sz(n), rg, sz(nr), None)), reps), sb * m + sb * n, rows=m)
        pool.free()
    public.free()
if args.log:
    with open(args.log, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
