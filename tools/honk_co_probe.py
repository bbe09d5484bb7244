#!/usr/bin/env python3
"""Device times of the sumcheck round on shares (csrc/honk_co_relations.hip) for one Rep3 party (party 0) on BN254 Fr: every stage on its
own, and the party's whole round of the four relations -- the stages with the local products of T::mul_many between them
(csh_rep3_local_mul_vec_dev; the exchange of the halves is the network's and is not here: the product's output stands in for the
reshared vector).

    python tools/honk_co_probe.py [--log FILE] [--sizes 12,16,20] [--example EXE]

With --example (the built examples/honk_sumcheck_from_cpp) the mirror's plain C++ loop of the same four relations on one host thread is
timed at n = 2^12 and 2^16: the plain form (one value per element, no operand vectors, no products between stages), the only host loop of
these relations the mirror has.

Every figure: the call back to back on the calling thread's stream between two HIP events, after bench.py's spin-up rule (untimed batches
for at least 0.3 s until two consecutive batch means agree within 2 %, 3 s at the most); the median of 7 such batches, with the lowest and
the highest of the 7 beside it. One JSON line per (stage, n), one process. `bytes` is what the stage MUST move: the columns it reads once
(a share column 64 B per element, a public one 32 B), the n / 2 scaling elements where it has a factor, and the operand vectors it reads
and writes (7 elements per edge and vector, 64 B each). No edge is skipped (the selectors are non-zero), so m = n / 2. One random column
goes up and the others are running products of it made on the device. Needs a device."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import cosnarks_amd as hip
from cosnarks_amd import bindings as B

ap = argparse.ArgumentParser()
ap.add_argument("--log", default=None, help="also append the lines to this file")
ap.add_argument("--sizes", default="12,16,20", help="log2 of the round size")
ap.add_argument("--example", default=None, help="the built examples/honk_sumcheck_from_cpp, for the host loop")
args = ap.parse_args()
if not hip.have_device():
    raise SystemExit("honk_co_probe: no HIP device (there is no CPU path to time)")
L = hip.lib()
e0, e1 = B.Event(), B.Event()
lines = []
sz = C.c_size_t
COLS, SHARED = 36, 13
SH, PUB = 64, 32          # bytes per element of a Rep3 share column and of a public column


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


def emit(op, n, m, nbytes=None, **extra):
    ms, lo, hi = m
    line = {"op": op, "n": n, "ms": round(ms, 5), "ms_min": round(lo, 5), "ms_max": round(hi, 5), **extra}
    if nbytes:
        line["bytes"] = nbytes
        line["TB_per_s"] = round(nbytes / ms / 1e9, 3)
    lines.append(line)
    print(json.dumps(line), flush=True)


def random_elements(rs, count):
    a = rs.randint(0, 2**64, size=(count, 4), dtype=np.uint64)
    a[:, 3] &= np.uint64((1 << 60) - 1)   # 252 random bits each: below p for BN254 Fr
    return a


rs = np.random.RandomState(29)
settings = {k: B.tune_get(k) for k in ("vec_max_blocks",)}
print(json.dumps({"settings": settings}), flush=True)
lines.append({"settings": settings})
params = random_elements(rs, 3).reshape(-1)
betas = random_elements(rs, 28)
for lg in (int(x) for x in args.sizes.split(",")):
    n = 1 << lg
    m, n7 = n // 2, 7 * (n // 2)
    reps = max(2, min(24, (1 << 18) // n * 2))
    elems = SHARED * 2 * n + (COLS - SHARED) * n       # field elements of all 36 columns
    pool = hip.DeviceBuffer(32 * elems)
    B._check(L.csh_memcpy_h2d(pool.ptr, random_elements(rs, n).ctypes.data_as(C.c_void_p), sz(32 * n)))
    at = lambda k: C.c_void_p(pool.ptr.value + 32 * n * k)
    B._check(L.csh_vec_mul_dev(0, at(0), at(0), at(1), sz(n), None))
    for k in range(2, elems // n):
        B._check(L.csh_vec_mul_dev(0, at(k - 1), at(k - 2), at(k), sz(n), None))
    col = [pool.ptr.value + 32 * n * (2 * c if c < SHARED else SHARED + c) for c in range(COLS)]
    table = hip.DeviceBuffer(32 * n)
    B._check(L.csh_honk_pow_table_dev(0, betas.ctypes.data_as(C.c_void_p), sz(lg), table.ptr, None))
    b = hip.HonkCoBatch(0, 1, 0, col, 0, n, None, None, table, 2, params)
    vec = lambda k: hip.DeviceBuffer(SH * n7 * k)
    mask, half = vec(4), vec(4)                        # 8 * 7 m elements of one component each: the masks and the products' outputs
    B._check(L.csh_vec_mul_dev(0, at(0), at(1), mask.ptr, sz(min(n, 8 * n7)), None))
    lhs8, rhs4, acc, r0 = vec(8), vec(4), hip.DeviceBuffer(SH * 24), hip.DeviceBuffer(SH * 6)
    sc = PUB * m
    stages = [
        ("arith", lambda: hip.honk_co_arith(b, mask, r0, acc), 6 * SH * n + 7 * PUB * n + sc + 32 * n7),
        ("perm operands", lambda: hip.honk_co_perm_operands(b, lhs8, rhs4), 4 * SH * n + 8 * PUB * n + 8 * SH * n7),
        ("perm operands2", lambda: hip.honk_co_perm_operands2(b, rhs4), 2 * SH * n + 2 * PUB * n + 2 * SH * n7),
        ("perm finish", lambda: hip.honk_co_perm_finish(b, lhs8, acc), SH * n + PUB * n + sc + 2 * SH * n7),
        ("delta operands", lambda: hip.honk_co_delta_operands(b, lhs8), 5 * SH * n + 8 * SH * n7),
        ("delta sub_one", lambda: hip.honk_co_delta_sub_one(0, 1, 0, lhs8, m), 2 * 32 * 8 * n7),
        ("delta finish", lambda: hip.honk_co_delta_finish(b, lhs8, acc), PUB * n + sc + 4 * SH * n7),
        ("lookup operands", lambda: hip.honk_co_lookup_operands(b, rhs4, half), 7 * SH * n + 4 * PUB * n + 2 * SH * n7),
        ("lookup mid", lambda: hip.honk_co_lookup_mid(b, lhs8, r0, rhs4, half), 2 * SH * n + 5 * PUB * n + sc + 6 * SH * n7),
        ("lookup finish", lambda: hip.honk_co_lookup_finish(b, lhs8, acc), 2 * SH * n + 5 * PUB * n + sc + 2 * SH * n7),
    ]
    hip.honk_co_lookup_operands(b, rhs4, half)         # any canonical data will do as a stage's input
    hip.honk_co_delta_operands(b, lhs8)
    for name, fn, must in stages:
        emit(name, n, measure(fn, reps), must, edges=m)
        hip.honk_co_delta_operands(b, lhs8)            # canonical again after the in-place stage

    def local_mul(x, y, out, count):
        B._check(L.csh_rep3_local_mul_vec_dev(0, C.c_void_p(x), C.c_void_p(y), mask.ptr, out.ptr, sz(count), None))

    mul_out = vec(4)                                   # 8 * 7 m half shares; read back as 4 * 7 m shares by the stage behind it

    def whole_round():
        hip.honk_co_arith(b, mask, r0, acc)
        hip.honk_co_perm_operands(b, lhs8, rhs4)
        local_mul(lhs8.ptr.value, rhs4.ptr.value, mul_out, 4 * n7)
        local_mul(mul_out.ptr.value, mul_out.ptr.value + SH * n7, half, 2 * n7)
        hip.honk_co_perm_operands2(b, rhs4)
        local_mul(mul_out.ptr.value, rhs4.ptr.value, half, 2 * n7)
        hip.honk_co_perm_finish(b, mul_out, acc)
        hip.honk_co_delta_operands(b, lhs8)
        local_mul(lhs8.ptr.value, lhs8.ptr.value, mul_out, 8 * n7)
        hip.honk_co_delta_sub_one(0, 1, 0, lhs8, m)
        local_mul(lhs8.ptr.value, lhs8.ptr.value + 4 * SH * n7, mul_out, 4 * n7)
        hip.honk_co_delta_finish(b, lhs8, acc)
        hip.honk_co_lookup_operands(b, rhs4, half)
        local_mul(rhs4.ptr.value, half.ptr.value, mul_out, n7)
        hip.honk_co_lookup_mid(b, lhs8, r0, rhs4, half)
        local_mul(rhs4.ptr.value, half.ptr.value, mul_out, 2 * n7)
        hip.honk_co_lookup_finish(b, lhs8, acc)

    emit("whole round: ten stages + seven local products", n, measure(whole_round, max(2, reps // 4)), edges=m)
    for x in (pool, table, mask, half, lhs8, rhs4, mul_out):
        x.free()
if args.example:
    for lg in (12, 16):
        n = 1 << lg
        with tempfile.TemporaryDirectory() as d:
            head = np.array([0, n, 0, n, lg, 2, 0], dtype=np.uint64)
            one = np.array([1, 0, 0, 0], dtype=np.uint64)   # partial_evaluation_result: any canonical element does for a timing
            words = [head, params, one, random_elements(rs, lg).reshape(-1), random_elements(rs, 10).reshape(-1), random_elements(rs, COLS * n).reshape(-1)]
            fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
            np.concatenate(words).astype("<u8").tofile(fin)
            r = subprocess.run([args.example, fin, fout], capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                raise SystemExit("honk_co_probe: %s failed: %s" % (args.example, r.stderr))
            us_host = int(np.fromfile(fout, dtype="<u8")[-1])
        line = {"op": "host_loop (plain C++, one thread, the plain form of the four relations)", "n": n, "ms": round(us_host / 1000, 3), "edges": n // 2}
        lines.append(line)
        print(json.dumps(line), flush=True)
if args.log:
    with open(args.log, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
