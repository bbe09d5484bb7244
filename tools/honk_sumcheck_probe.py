#!/usr/bin/env python3
"""Device times of the plain sumcheck round's entries (csrc/honk_relations.hip, csrc/honk_gates.hip over csrc/honk_stage.hpp) on BN254 Fr:

  vec_mul       csh_vec_mul_dev on as many values as one column has, in the same process: the HBM yardstick (one multiplication per 96 B)
  pow_table     csh_honk_pow_table_dev for the table round 0 reads (log2 n betas)
  gates worst   csh_honk_sumcheck_accumulate_gates_dev over [0, n) with the gate-separator table at stride 2 (round 0), all five
                selectors non-zero on every row, so that no edge of any of the three launches is skipped
  gates mixed   the same call with each selector non-zero on a contiguous eighth of the rows of its own and zero elsewhere, as a circuit's
                mutually exclusive, sparse gate blocks are: most edges of each launch read two selector words and leave
  accumulate    csh_honk_sumcheck_accumulate_dev (subrelations 0 .. 10, 36 columns) on the same size, no edge skipped
  chain         rounds 0 .. log2 n - 1 of both entries + csh_mle_fold_dev of the 41 distinct columns (n = 2^20 only; worst-case columns)
  host_loop     the mirror's plain C++ loops on one host thread, through examples/honk_sumcheck_from_cpp (--example EXE) and
                examples/honk_gates_from_cpp (--gates-example EXE); n = 2^12, 2^16

    python tools/honk_sumcheck_probe.py [--log FILE] [--sizes 12,16,20,22] [--example EXE] [--gates-example EXE]

Every device figure: the call back to back on the calling thread's stream between two HIP events, after bench.py's spin-up rule (untimed
batches for at least 0.3 s until two consecutive batch means agree within 2 %, 3 s at the most); the median of 7 such batches, with the
lowest and the highest of the 7 beside it. One JSON line per (stage, n), one process. `bytes` is what the worst case MUST read -- the
entry's 19 or 36 columns x 32 B x n plus the n / 2 scaling elements. One random column goes up and the others are running products of it
made on the device (distinct, canonical, non-zero). Only the C ABI is called, so COSNARKS_HIP_LIB may name another build of the library
to time beside this one. Needs a device."""
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
ap.add_argument("--sizes", default="12,16,20,22", help="log2 of the round size")
ap.add_argument("--example", default=None, help="the built examples/honk_sumcheck_from_cpp, for the host loop of subrelations 0 .. 10")
ap.add_argument("--gates-example", default=None, help="the built examples/honk_gates_from_cpp, for the host loop of the five gate relations")
args = ap.parse_args()
if not hip.have_device():
    raise SystemExit("honk_sumcheck_probe: no HIP device (there is no CPU path to time)")
L = hip.lib()
e0, e1 = B.Event(), B.Event()
lines = []
sz = C.c_size_t
BASE_COLS, GATE_COLS, ALL_COLS = 36, 19, 41
GATE_FROM_BASE = [0, 1, 2, 3, 8, 9, 10, 11, 13, 14, 15, 16, 17, 18]   # w, shifted w, q_m .. q_4 among the first entry's columns


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


def ptrs(addrs):
    return (C.c_void_p * len(addrs))(*addrs)


rs = np.random.RandomState(23)
settings = {k: B.tune_get(k) for k in ("vec_max_blocks",)}
print(json.dumps({"settings": settings}), flush=True)
lines.append({"settings": settings})
params = random_elements(rs, 3)
gate_params = random_elements(rs, 8)
betas = random_elements(rs, 28)
sizes = [int(x) for x in args.sizes.split(",")]
for lg in sizes:
    n = 1 << lg
    reps = max(2, min(24, (1 << 20) // n * 2))
    pool = hip.DeviceBuffer(ALL_COLS * 32 * n)
    col = [pool.ptr.value + c * 32 * n for c in range(ALL_COLS)]      # 36 of the first entry, then the five gate selectors
    B._check(L.csh_memcpy_h2d(C.c_void_p(col[0]), random_elements(rs, n).ctypes.data_as(C.c_void_p), sz(32 * n)))
    B._check(L.csh_vec_mul_dev(0, C.c_void_p(col[0]), C.c_void_p(col[0]), C.c_void_p(col[1]), sz(n), None))
    for c in range(2, ALL_COLS):
        B._check(L.csh_vec_mul_dev(0, C.c_void_p(col[c - 1]), C.c_void_p(col[c - 2]), C.c_void_p(col[c]), sz(n), None))
    gate_col = [col[c] for c in GATE_FROM_BASE] + col[BASE_COLS:]
    # the mixed case: selector s keeps its values on rows [s n / 8, (s + 1) n / 8) and is zero elsewhere
    sparse = hip.DeviceBuffer(5 * 32 * n)
    eighth = n // 8
    for s in range(5):
        host = np.zeros((n, 4), dtype=np.uint64)
        host[s * eighth:(s + 1) * eighth] = random_elements(rs, eighth)
        B._check(L.csh_memcpy_h2d(C.c_void_p(sparse.ptr.value + s * 32 * n), host.ctypes.data_as(C.c_void_p), sz(32 * n)))
    mixed_col = gate_col[:14] + [sparse.ptr.value + s * 32 * n for s in range(5)]
    table, acc, gacc = hip.DeviceBuffer(32 * n), hip.DeviceBuffer(32 * 57), hip.DeviceBuffer(32 * 110)
    bp, pp, gp = (x.ctypes.data_as(C.c_void_p) for x in (betas, params, gate_params))
    emit("vec_mul", n, measure(lambda: B._check(L.csh_vec_mul_dev(0, C.c_void_p(col[0]), C.c_void_p(col[1]), C.c_void_p(col[2]), sz(n), None)), reps), 96 * n)
    B._check(L.csh_vec_mul_dev(0, C.c_void_p(col[1]), C.c_void_p(col[0]), C.c_void_p(col[2]), sz(n), None))   # col 2 as it was
    emit("pow_table", n, measure(lambda: B._check(L.csh_honk_pow_table_dev(0, bp, sz(lg), table.ptr, None)), reps), 32 * n)
    cp, gcp, mcp = ptrs(col[:BASE_COLS]), ptrs(gate_col), ptrs(mixed_col)
    must = GATE_COLS * 32 * n + 32 * (n // 2)
    emit("gates worst: no edge skipped", n, measure(lambda: B._check(L.csh_honk_sumcheck_accumulate_gates_dev(0, gcp, sz(0), sz(n), table.ptr, sz(2), gp, gacc.ptr, None)), reps),
         must, edges=n // 2)
    emit("gates mixed: each selector on an eighth of the rows", n,
         measure(lambda: B._check(L.csh_honk_sumcheck_accumulate_gates_dev(0, mcp, sz(0), sz(n), table.ptr, sz(2), gp, gacc.ptr, None)), reps), edges=n // 2)
    emit("accumulate (subrelations 0 .. 10)", n, measure(lambda: B._check(L.csh_honk_sumcheck_accumulate_dev(0, cp, sz(0), sz(n), table.ptr, sz(2), pp, acc.ptr, None)), reps),
         BASE_COLS * 32 * n + 32 * (n // 2), edges=n // 2)
    if lg == 20:
        other = hip.DeviceBuffer(ALL_COLS * 32 * n)   # every round's folded columns behind the round before: n / 2 + n / 4 + ... < n per column
        us = random_elements(rs, lg)

        def chain():
            src, size, stride, off = col, n, 2, 0
            for rnd in range(lg):
                B._check(L.csh_honk_sumcheck_accumulate_dev(0, ptrs(src[:BASE_COLS]), sz(0), sz(size), table.ptr, sz(stride), pp, acc.ptr, None))
                B._check(L.csh_honk_sumcheck_accumulate_gates_dev(0, ptrs([src[c] for c in GATE_FROM_BASE] + src[BASE_COLS:]), sz(0), sz(size), table.ptr,
                                                                  sz(stride), gp, gacc.ptr, None))
                if size == 2:
                    break
                dst = [other.ptr.value + off + c * 16 * size for c in range(ALL_COLS)]
                B._check(L.csh_mle_fold_dev(0, ptrs(src), ptrs(dst), sz(ALL_COLS), sz(size), C.c_uint32(1), us[rnd].ctypes.data_as(C.c_void_p), None))
                src, size, stride, off = dst, size // 2, stride * 2, off + ALL_COLS * 16 * size

        emit("chain: both entries + fold of 41 columns, every round", n, measure(chain, 2), rounds=lg)
        other.free()
    pool.free()
    sparse.free()
    table.free()
# the examples' input: head, params, partial_evaluation_result, log2 n betas, the alphas, (the gate parameters,) the columns
for exe, op, alphas, tail, cols in ((args.example, "host_loop (plain C++, one thread)", 10, [], BASE_COLS),
                                    (args.gates_example, "host_loop (plain C++, one thread, five relations)", 27, [gate_params.reshape(-1)], ALL_COLS)):
    for lg in (12, 16) if exe else ():
        n = 1 << lg
        with tempfile.TemporaryDirectory() as d:
            head = np.array([0, n, 0, n, lg, 2, 0], dtype=np.uint64)
            one = np.array([1, 0, 0, 0], dtype=np.uint64)   # partial_evaluation_result: any canonical element does for a timing
            words = [head, params.reshape(-1), one, random_elements(rs, lg).reshape(-1), random_elements(rs, alphas).reshape(-1)] + tail + \
                    [random_elements(rs, cols * n).reshape(-1)]
            fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
            np.concatenate(words).astype("<u8").tofile(fin)
            r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                raise SystemExit("honk_sumcheck_probe: %s failed: %s" % (exe, r.stderr))
            us_host = int(np.fromfile(fout, dtype="<u8")[-1])
        line = {"op": op, "n": n, "ms": round(us_host / 1000, 3), "edges": n // 2}
        lines.append(line)
        print(json.dumps(line), flush=True)
if args.log:
    with open(args.log, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
