#!/usr/bin/env python3
"""Device times of the sumcheck round on shares (csrc/honk_co_relations.hip) for one Rep3 party (party 0) on BN254 Fr: every stage on its
own, and the party's whole round of the four relations -- the stages with the local products of T::mul_many between them
(csh_rep3_local_mul_vec_dev; the exchange of the halves is the network's and is not here: the product's output stands in for the
reshared vector).

    python tools/honk_co_probe.py [--log FILE] [--sizes 12,16,20] [--example EXE] [--gates] [--gates-example EXE]

With --example (the built examples/honk_sumcheck_from_cpp) the mirror's plain C++ loop of the same four relations on one host thread is
timed at n = 2^12 and 2^16: the plain form (one value per element, no operand vectors, no products between stages), the only host loop of
these relations the mirror has.

With --gates the stages of the five gate relations (csrc/honk_co_gates.hip) are timed behind them, then those five relations' round and
the party's whole round of all nine relations; --gates-example (the built examples/honk_gates_from_cpp) adds the mirror's plain C++ loop
of the five gate relations at the same two sizes. The selectors of the gate relations are five of the non-zero precomputed columns.

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
ap.add_argument("--gates", action="store_true", help="also the five gate relations and the round of all nine")
ap.add_argument("--gates-example", default=None, help="the built examples/honk_gates_from_cpp, for the host loop of the five gate relations")
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
gate_params = random_elements(rs, 8).reshape(-1)
GATE_COLUMN_OF = [0, 1, 2, 3, 8, 9, 10, 11, 13, 14, 15, 16, 17, 18] + [19, 20, 21, 22, 23]    # the last five stand in for the gate selectors
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
    if args.gates:
        gb = hip.HonkCoGatesBatch(0, 1, 0, [col[c] for c in GATE_COLUMN_OF], 0, n, None, None, table, 2, gate_params)
        l7, r7, mul7, l5, r5, mul5, one, gacc = vec(7), vec(7), vec(7), vec(5), vec(5), vec(5), vec(1), hip.DeviceBuffer(SH * 36)
        hip.honk_co_ell_operands(gb, l7, r7)               # every vector canonical before it is a stage's input
        hip.honk_co_ell_operands(gb, mul7, r7)
        hip.honk_co_ell_operands2(gb, mul7, l5, r5)
        hip.honk_co_ell_operands2(gb, mul7, mul5, r5)
        hip.honk_co_mem_operands(gb, l7, r7, one)
        part = lambda v, q: C.c_void_p(v.ptr.value + q * SH * n7)
        gstages = [
            ("ell operands", lambda: hip.honk_co_ell_operands(gb, l7, r7), 6 * SH * n + PUB * n + 14 * SH * n7),
            ("ell operands2", lambda: hip.honk_co_ell_operands2(gb, mul7, l5, r5), 5 * SH * n + 13 * SH * n7),
            ("ell finish", lambda: hip.honk_co_ell_finish(gb, mul7, mul5, gacc), 3 * PUB * n + sc + 10 * SH * n7),
            ("mem operands", lambda: hip.honk_co_mem_operands(gb, l7, r7, one), 8 * SH * n + PUB * n + 13 * SH * n7),
            ("mem finish", lambda: hip.honk_co_mem_finish(gb, mul7, one, gacc), 8 * SH * n + 7 * PUB * n + sc + 7 * SH * n7),
            ("nnf operands", lambda: hip.honk_co_nnf_operands(gb, l5, r5), 6 * SH * n + 10 * SH * n7),
            ("nnf finish", lambda: hip.honk_co_nnf_finish(gb, mul5, gacc), 8 * SH * n + 5 * PUB * n + sc + 5 * SH * n7),
            ("pos_ext operands", lambda: hip.honk_co_pos_ext_operands(gb, l5), 4 * SH * n + 4 * PUB * n + 4 * SH * n7),
            ("pos_ext finish", lambda: hip.honk_co_pos_ext_finish(gb, mul5, gacc), 4 * SH * n + PUB * n + sc + 4 * SH * n7),
            ("pos_int operands", lambda: hip.honk_co_pos_int_operands(gb, one), SH * n + PUB * n + SH * n7),
            ("pos_int finish", lambda: hip.honk_co_pos_int_finish(gb, one, gacc), 7 * SH * n + PUB * n + sc + SH * n7),
        ]
        for name, fn, must in gstages:
            emit(name, n, measure(fn, reps), must, edges=m)

        def sbox(s, u, w, count):                          # s^5: three local products
            local_mul(s.ptr.value, s.ptr.value, u, count)
            local_mul(u.ptr.value, u.ptr.value, w, count)
            local_mul(w.ptr.value, s.ptr.value, u, count)

        def gates_round():
            hip.honk_co_ell_operands(gb, l7, r7)
            local_mul(l7.ptr.value, r7.ptr.value, mul7, 7 * n7)
            hip.honk_co_ell_operands2(gb, mul7, l5, r5)
            local_mul(l5.ptr.value, r5.ptr.value, mul5, 5 * n7)
            hip.honk_co_ell_finish(gb, mul7, mul5, gacc)
            hip.honk_co_mem_operands(gb, l7, r7, one)
            local_mul(l7.ptr.value, r7.ptr.value, mul7, 6 * n7)
            local_mul(part(mul7, 3).value, one.ptr.value, mul5, n7)
            hip.honk_co_mem_finish(gb, mul7, mul5, gacc)
            hip.honk_co_nnf_operands(gb, l5, r5)
            local_mul(l5.ptr.value, r5.ptr.value, mul5, 5 * n7)
            hip.honk_co_nnf_finish(gb, mul5, gacc)
            hip.honk_co_pos_ext_operands(gb, l5)
            sbox(l5, mul5, r5, 4 * n7)
            hip.honk_co_pos_ext_finish(gb, mul5, gacc)
            hip.honk_co_pos_int_operands(gb, one)
            sbox(one, mul5, r5, n7)
            hip.honk_co_pos_int_finish(gb, mul5, gacc)

        def nine_relations():
            whole_round()
            gates_round()

        emit("gate relations: eleven stages + eleven local products", n, measure(gates_round, max(2, reps // 4)), edges=m)
        emit("whole round of nine relations: 21 stages + 18 local products", n, measure(nine_relations, max(2, reps // 4)), edges=m)
        for x in (l7, r7, mul7, l5, r5, mul5, one):
            x.free()
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
if args.gates_example:
    for lg in (12, 16):
        n = 1 << lg
        with tempfile.TemporaryDirectory() as d:
            head = np.array([0, n, 0, n, lg, 2, 0], dtype=np.uint64)
            one = np.array([1, 0, 0, 0], dtype=np.uint64)
            words = [head, params, one, random_elements(rs, lg).reshape(-1), random_elements(rs, 27).reshape(-1), gate_params,
                     random_elements(rs, (COLS + 5) * n).reshape(-1)]
            fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
            np.concatenate(words).astype("<u8").tofile(fin)
            r = subprocess.run([args.gates_example, fin, fout], capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                raise SystemExit("honk_co_probe: %s failed: %s" % (args.gates_example, r.stderr))
            us_host = int(np.fromfile(fout, dtype="<u8")[-1])
        line = {"op": "host_loop (plain C++, one thread, the plain form of the five gate relations)", "n": n, "ms": round(us_host / 1000, 3), "edges": n // 2}
        lines.append(line)
        print(json.dumps(line), flush=True)
if args.log:
    with open(args.log, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
