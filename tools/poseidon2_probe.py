#!/usr/bin/env python3
"""Device times of the batched Poseidon2 entries (csrc/poseidon2.hip) on BN254 Fr with the reference's round numbers (4 + 4 external
rounds, 56 internal) and seeded constants of the tool's own:

    python tools/poseidon2_probe.py [--log FILE] [--sizes 10,16,20] [--host-loop PROGRAM]

  host_loop    with --host-loop: the host mirror's plain loop (Poseidon2Hip::permutation_in_place, co-snarks_amd/host/mpc.hpp) on one thread
               over 2^14 states, run by the built examples/poseidon2_from_cpp.cpp in processes of its own before anything is timed on the
               device; each permute row then carries that rate and the ratio to it
  permute      csh_poseidon2_permute_dev for t = 2, 3, 4 at 2^10, 2^16, 2^20 states: permutations/s and the field multiplications/s that
               is (3 per s-box, t diagonal products per internal round at t = 4, 2 t for the way in and out of the R' domain)
  merkle       the compression tree of 2^20 leaves, t = 2, arity 2 (20 launches)
  co_perm      one party's whole collaborative permutation at 2^16 states, t = 4, Rep3 party 0: the R + 1 steps back to back (the
               openings between them are the network's and are not here; y is a fixed vector)
  vec_mul      csh_vec_mul_dev at 2^20 in the same process: the multiplication rate of a kernel that only loads, multiplies and stores

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
from oracle import fields as fl

ap = argparse.ArgumentParser()
ap.add_argument("--log", default=None, help="also append the lines to this file")
ap.add_argument("--sizes", default="10,16,20", help="log2 of the batch sizes of the plain permutation")
ap.add_argument("--host-loop", default=None, help="examples/poseidon2_from_cpp.cpp, built: adds the host mirror's one-thread loop beside each permute row")
args = ap.parse_args()
if not hip.have_device():
    raise SystemExit("poseidon2_probe: no HIP device (there is no CPU path to time)")
L = hip.lib()
e0, e1 = B.Event(), B.Event()
F = fl.BN254_FR
RF_B, RF_E, RP = 4, 4, 56
rs = np.random.RandomState(2)
lines = []


def elems(n):
    """n raw elements below 2^252 (any value below p is a valid Montgomery encoding)"""
    a = rs.randint(0, 2**63, size=(n, 4), dtype=np.int64).astype(np.uint64)
    a[:, 3] &= np.uint64((1 << 60) - 1)
    return a.reshape(-1)


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


def make_params(t):
    diag = fl.pack(F, {2: [1, 2], 3: [1, 1, 2]}[t]).reshape(-1) if t < 4 else elems(4)
    return hip.Poseidon2Params(hip.BN254, t, RF_B, RF_E, RP, elems((RF_B + RF_E) * t), elems(RP), diag)


def muls_per_perm(t):
    return 3 * ((RF_B + RF_E) * t + RP) + (RP * t if t == 4 else 0) + 2 * t


def host_loop(t):
    """Poseidon2Hip::permutation_in_place over 2^14 states on one thread of the host, timed by the program itself: the median of 7 runs"""
    runs = []
    for _ in range(7):
        r = subprocess.run([args.host_loop, "--host-loop", str(t), str(1 << 14)], capture_output=True, text=True, timeout=120, check=True)
        runs.append(float(re.search(r"ns_per_permutation=([0-9.]+)", r.stdout).group(1)))
    ns = sorted(runs)
    line = {"op": "host_loop", "t": t, "log_n": 14, "threads": 1, "ns_per_perm": ns[3], "ns_min": ns[0], "ns_max": ns[-1], "perm_per_s": round(1e9 / ns[3])}
    lines.append(line)
    print(json.dumps(line), flush=True)
    return 1e9 / ns[3]


host_rate = {t: host_loop(t) for t in (2, 3, 4)} if args.host_loop else {}
par = {t: make_params(t) for t in (2, 3, 4)}
for lg in [int(x) for x in args.sizes.split(",")]:
    n = 1 << lg
    for t in (2, 3, 4):
        src, dst = hip.DeviceBuffer.from_host(elems(n * t)), hip.DeviceBuffer(32 * n * t)
        m = measure(lambda: hip.poseidon2_permute(par[t], src, n, out=dst), 20 if lg < 20 else 3)
        beside = {"host_perm_per_s": round(host_rate[t]), "times_host": round(n / m[0] * 1e3 / host_rate[t], 1)} if host_rate else {}
        emit("permute", m, t=t, log_n=lg, perm_per_s=round(n / m[0] * 1e3), Gmul_per_s=round(n * muls_per_perm(t) / m[0] / 1e6, 2), **beside)

n = 1 << 20
a, b, out = hip.DeviceBuffer.from_host(elems(n)), hip.DeviceBuffer.from_host(elems(n)), hip.DeviceBuffer(32 * n)
m = measure(lambda: B._check(L.csh_vec_mul_dev(hip.BN254, a.ptr, b.ptr, out.ptr, C.c_size_t(n), None)), 20)
emit("vec_mul", m, log_n=20, Gmul_per_s=round(n / m[0] / 1e6, 2))

root, work = hip.DeviceBuffer(32), hip.DeviceBuffer(32 * n)
m = measure(lambda: hip.poseidon2_merkle(par[2], 2, hip.bindings.POSEIDON2_COMPRESSION, a, n, root=root, work=work), 3)
emit("merkle", m, t=2, arity=2, mode="compression", log_leaves=20, hashes=n - 1, perm_per_s=round((n - 1) / m[0] * 1e3))

t, n = 4, 1 << 16
R = RF_B + RP + RF_E
entries = ((RF_B + RF_E) * t + RP) * n
state, y = hip.DeviceBuffer.from_host(elems(2 * n * t)), hip.DeviceBuffer.from_host(elems(n * t))
host = elems(2 * entries)
pre = [hip.DeviceBuffer.from_host(host) for _ in range(5)]
opened = hip.DeviceBuffer(64 * n * t)
offs = [0]
for r in range(R):
    offs.append(offs[-1] + par[t].round_entries(r, n))


def co_perm():
    for s in range(R + 1):
        hip.poseidon2_co_round(hip.BN254, 1, 0, par[t], s, state, n, y if s else None, pre, offs[s], open_out=opened if s < R else None)


m = measure(co_perm, 2)
emit("co_perm", m, t=t, log_n=16, protocol="rep3", party=0, steps=R + 1, ms_per_step=round(m[0] / (R + 1), 5), perm_per_s=round(n / m[0] * 1e3))
B.sync()
if args.log:
    with open(args.log, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
