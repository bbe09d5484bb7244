#!/usr/bin/env python3
"""One build, one shape: median / min ms of blocks of synchronous csh_msm_dev calls (host fold included). The library is the one
COSNARKS_HIP_LIB names (default: the tree's). --witness: a quarter 0, a quarter 1, a quarter one repeated value, a quarter uniform."""
import argparse
import ctypes as C
import hashlib
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
ap.add_argument("--job", default="0:0:20")
ap.add_argument("--witness", action="store_true")
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--blocks", type=int, default=5)
ap.add_argument("--tune", default="")
ap.add_argument("--tag", default="")
args = ap.parse_args()
L = hip.lib()
curve, group, logn = (int(x) for x in args.job.split(":"))
n = 1 << logn
pb = hip.point_bytes(curve, group)
buf = hip.DeviceBuffer(n * pb)
B._check(L.csh_util_generate_bases_dev(curve, group, C.c_uint64(1), C.c_size_t(n), buf.ptr, None))
B.sync()
h = C.c_void_p()
B._check(L.csh_bases_upload_dev(curve, group, buf.ptr, C.c_size_t(n), C.c_size_t(0), None, C.byref(h)))
buf.free()
rs = np.random.RandomState(1)
limbs = rs.randint(0, 1 << 63, size=(n, 4), dtype=np.uint64)
limbs[:, 3] >>= np.uint64(3)
if args.witness:
    kind = rs.randint(0, 4, size=n)
    rep = limbs[0].copy()
    limbs[kind == 0] = 0
    limbs[kind == 1] = np.array([1, 0, 0, 0], dtype=np.uint64)
    limbs[kind == 2] = rep
mont = 0 if args.witness else 1
sc = hip.DeviceBuffer.from_host(limbs)
out = np.zeros(3 * pb // 16, dtype=np.uint64)
for kv in filter(None, args.tune.split(",")):
    k, v = kv.split("=")
    B.tune_set(k, int(v))
call = lambda: B._check(L.csh_msm_dev(h, C.c_size_t(0), C.c_size_t(n), sc.ptr, mont, out.ctypes.data_as(C.c_void_p), None))
t_end = time.perf_counter() + 0.4
while time.perf_counter() < t_end:
    call()
ts = []
for _ in range(args.blocks):
    t0 = time.perf_counter()
    for _ in range(args.calls):
        call()
    ts.append((time.perf_counter() - t0) / args.calls * 1e3)
print(json.dumps({"tag": args.tag, "lib": os.environ.get("COSNARKS_HIP_LIB", "tree"), "job": args.job, "witness": args.witness, "tune": args.tune,
                  "params_c_W_L_S": B.msm_last_params(), "ms_median": round(statistics.median(ts), 5), "ms_min": round(min(ts), 5),
                  "result_sha": hashlib.sha256(out.tobytes()).hexdigest()[:16]}), flush=True)
