#!/usr/bin/env python3
"""Device times of the round-2 / round-5 entries (csrc/plonk_rounds.hip) on BN254 Fr, one and two components per share:

  vec_mul      csh_vec_mul_dev on as many values in the same process: the HBM yardstick (one multiplication per 96 B)
  z_operands   csh_plonk_z_operands_dev: buffer_a, buffer_b, buffer_c and every fourth element of S1, S2, S3 in, 6 share vectors out
  rotate       csh_vec_rotate_right_dev, k = 1
  blind        csh_plonk_blind_coefficients_dev, k = 3: one launch of one workgroup (milliseconds only)
  lincomb      csh_poly_lincomb_dev in the round-5 shape: 7 share vectors of n + 1 .. n + 6, 8 public vectors of n, const0, out n + 6
  baseline     the same result through the entries that were there before (ncomp 1 only: they have no add_with_public rule, so a Rep3
               share cannot take the public sum on one component): 15 zero-padded copies to n + 6 (csh_lincomb_dev with one vector and
               coefficient one, the stream-ordered device copy those entries offer; the zero tails are written once, outside the timing),
               csh_lincomb_dev over the 7 shares, csh_lincomb_dev over the 8 public vectors, csh_vec_add_dev. const0 is left out of it.

    python tools/plonk_rounds_probe.py [--log FILE] [--sizes 20,22]

Every figure: the call back to back on the calling thread's stream between two HIP events, after bench.py's spin-up rule (untimed batches
for at least 0.3 s until two consecutive batch means agree within 2 %, 3 s at the most); the median of 7 such batches, with the lowest and
the highest of the 7 beside it. One JSON line per (stage, n, ncomp). `bytes` is what the stage MUST move -- every distinct input element
read once, every output written once -- and TB/s is that over the time. The buffers are not initialised: no kernel here has a
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
ap.add_argument("--sizes", default="20,22", help="log2 n of the domain")
args = ap.parse_args()
if not hip.have_device():
    raise SystemExit("plonk_rounds_probe: no HIP device (there is no CPU path to time)")
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


def limbs(rs, n):
    """n canonical elements as (n, 4) u64: 252 random bits each, below p for BN254 Fr"""
    v = rs.randint(0, 2**64, size=(n, 4), dtype=np.uint64)
    v[:, 3] &= np.uint64((1 << 60) - 1)
    return v


def ptrs(addrs):
    return (C.c_void_p * len(addrs))(*addrs)


rs = np.random.RandomState(13)
settings = {k: B.tune_get(k) for k in ("vec_max_blocks",)}
print(json.dumps({"settings": settings}), flush=True)
lines.append({"settings": settings})
host = limbs(rs, 2 * 16).reshape(-1)   # challenges, coefficients, blinders: read on the host during the call
hp = host.ctypes.data_as(C.c_void_p)
BN254_R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
one = np.array([((1 << 256) % BN254_R >> (64 * i)) & (2**64 - 1) for i in range(4)], dtype=np.uint64)   # 1 in arkworks-Montgomery form
onep = one.ctypes.data_as(C.c_void_p)
u32, sz = C.c_uint32, C.c_size_t
for lg in [int(x) for x in args.sizes.split(",")]:
    n = 1 << lg
    dom = hip.Domain(hip.BN254, lg + 2)
    reps = max(3, min(24, (1 << 22) // n * 3))
    m = n + 6
    public = hip.DeviceBuffer(8 * 32 * 4 * n)   # S1, S2, S3 on 4 n points; as 8 coefficient vectors of n for the linear combination
    sigma = [public.ptr.value + k * 32 * 4 * n for k in range(3)]
    pub = [public.ptr.value + k * 32 * n for k in range(8)]
    padded_pub = hip.DeviceBuffer(9 * 32 * m)   # 8 padded public vectors and their sum
    ppub = [padded_pub.ptr.value + k * 32 * m for k in range(9)]
    zeros = np.zeros(4 * 2 * 6, dtype=np.uint64)
    zp = zeros.ctypes.data_as(C.c_void_p)
    for k in range(8):
        B._check(L.csh_memcpy_h2d(C.c_void_p(ppub[k] + 32 * n), zp, sz(32 * 6)))
    for ncomp in (1, 2):
        sb = 32 * ncomp
        vb = sb * m
        pool = hip.DeviceBuffer(18 * vb)
        slot = [pool.ptr.value + k * vb for k in range(18)]
        pr = ncomp - 1
        vals = n * ncomp
        emit("vec_mul", vals, 1, measure(lambda: B._check(L.csh_vec_mul_dev(0, C.c_void_p(slot[0]), C.c_void_p(slot[1]), C.c_void_p(slot[2]), sz(vals), None)), reps),
             96 * vals)
        sh3, sg3, o6 = ptrs(slot[:3]), ptrs(sigma), ptrs(slot[3:9])
        emit("z_operands", n, ncomp, measure(lambda: B._check(L.csh_plonk_z_operands_dev(dom.h, u32(pr), u32(0), sh3, sg3, hp, o6, None)), reps),
             9 * sb * n + 3 * 32 * n)
        emit("rotate", n, ncomp, measure(lambda: B._check(L.csh_vec_rotate_right_dev(0, C.c_void_p(slot[0]), C.c_void_p(slot[1]), sz(n), u32(ncomp), sz(1), None)), reps),
             2 * sb * n)
        emit("blind", n, ncomp, measure(lambda: B._check(L.csh_plonk_blind_coefficients_dev(0, C.c_void_p(slot[0]), sz(n), u32(ncomp), hp, sz(3), None)), reps))
        lens = [n + 3, n + 1, n + 1, n + 6, n + 2, n + 2, n + 2]
        sl, pl = (sz * 7)(*lens), (sz * 8)(*([n] * 8))
        sh7, pb8 = ptrs(slot[:7]), ptrs(pub)
        out = C.c_void_p(slot[7])
        moved = sb * sum(lens) + 8 * 32 * n + sb * m
        new = measure(lambda: B._check(L.csh_poly_lincomb_dev(0, u32(pr), u32(0), sh7, sl, hp, sz(7), pb8, pl, hp, sz(8), hp, out, sz(m), None)), reps)
        emit("lincomb (round-5 shape)", n, ncomp, new, moved)
        if ncomp == 1:
            pad7 = ptrs(slot[8:15])
            for k in range(7):
                B._check(L.csh_memcpy_h2d(C.c_void_p(slot[8 + k] + sb * lens[k]), zp, sz(sb * (m - lens[k]))))
            pad8 = ptrs(ppub[:8])

            def baseline():
                for k in range(7):   # the copies; the tails of the padded buffers are zero and stay zero
                    B._check(L.csh_lincomb_dev(0, ptrs([slot[k]]), onep, sz(1), C.c_void_p(slot[8 + k]), sz(lens[k]), None))
                for k in range(8):
                    B._check(L.csh_lincomb_dev(0, ptrs([pub[k]]), onep, sz(1), C.c_void_p(ppub[k]), sz(n), None))
                B._check(L.csh_lincomb_dev(0, pad7, hp, sz(7), C.c_void_p(slot[15]), sz(m), None))
                B._check(L.csh_lincomb_dev(0, pad8, hp, sz(8), C.c_void_p(ppub[8]), sz(m), None))
                B._check(L.csh_vec_add_dev(0, C.c_void_p(slot[15]), C.c_void_p(ppub[8]), C.c_void_p(slot[16]), sz(m), u32(1), None))

            old = measure(baseline, reps)
            emit("baseline (copies + 2 csh_lincomb_dev + csh_vec_add_dev)", n, 1, old, moved, new_over_old=round(new[0] / old[0], 3),
                 ranges_apart=bool(new[2] < old[1]))
        pool.free()
    padded_pub.free()
    public.free()
    dom.free()
if args.log:
    with open(args.log, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
