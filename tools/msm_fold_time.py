#!/usr/bin/env python3
"""us per csh_msm_fold_partials (host only; the library COSNARKS_HIP_LIB names, default the tree's) on one partial buffer: BN254 G1 / BLS12-381 G1 with the headline's layout (c = 15, W = 17), BLS12-381 G2."""
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import cosnarks_amd as hip
from oracle import curves as cv
from tests import helpers as H
from tests import test_host_fold_cpu as T

for curve, group, c, W, wide in (("bn254", 0, 15, 17, 17), ("bls12_381", 0, 15, 17, 17), ("bls12_381", 1, 13, 20, 12), ("bn254", 0, 12, 22, 3)):
    G = cv.CURVES[curve][group]
    cid = H.CURVE_IDS[curve]
    r = H.rng(5)
    pb = hip.point_bytes(cid, group)
    buf = T._partial(hip, cid, group, c, wide, [T._xyzz(G, P, T._rand_z(G.F, r), pb) for P in T._points(G, W, r)])
    out = np.zeros(3 * pb // 16, dtype=np.uint64)
    f = hip.lib().csh_msm_fold_partials
    call = lambda: f(cid, group, buf, C.c_size_t(1), out.ctypes.data_as(C.c_void_p))
    for _ in range(200):
        call()
    ts = []
    for _ in range(9):
        t0 = time.perf_counter()
        for _ in range(300):
            call()
        ts.append((time.perf_counter() - t0) / 300 * 1e6)
    print(json.dumps({"lib": os.environ.get("COSNARKS_HIP_LIB", "tree"), "curve": curve, "group": group, "c": c, "W": W, "wide": wide,
                      "fold_us_median": round(statistics.median(ts), 2), "fold_us_min": round(min(ts), 2), "out0": int(out[0])}), flush=True)
