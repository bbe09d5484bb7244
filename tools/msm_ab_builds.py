#!/usr/bin/env python3
"""Alternating timing of two builds of libcosnarks_hip.so (COSNARKS_HIP_LIB): per round one run of the parent's library, one of the
tree's and a second parent run (the control), one fresh process per measurement; the order rotates by one place every round and is
reversed every other round, so every run takes every position. Stops at the first child that does not exit 0.
    python tools/msm_ab_builds.py --parent PARENT/libcosnarks_hip.so --rounds 9 --what headline,2p16,2p18,bls381,witness
    python tools/msm_ab_builds.py --parent PARENT/libcosnarks_hip.so --rounds 8 --what 2p20 --extra-tune msm_l=69
headline = `python bench.py --gpus 1 --steps 20 --warmup 5`; the other shapes = tools/msm_time.py (median ms of blocks of synchronous
csh_msm_dev calls; witness = a quarter 0, a quarter 1, a quarter one repeated value, a quarter uniform)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--parent", required=True)
ap.add_argument("--rounds", type=int, default=8)
ap.add_argument("--what", default="headline")
ap.add_argument("--extra-tune", default="", help="a second 'new' variant with this tune string (msm_time shapes only)")
args = ap.parse_args()
parent = os.path.abspath(args.parent)
new = os.path.join(ROOT, "co-snarks_amd", "lib", "libcosnarks_hip.so")
SHAPES = {
    "headline": ("bench", [sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"]),
    "2p16": ("time", ["--job", "0:0:16", "--calls", "50"]),
    "2p18": ("time", ["--job", "0:0:18", "--calls", "40"]),
    "2p20": ("time", ["--job", "0:0:20", "--calls", "20"]),
    "bls381": ("time", ["--job", "1:0:20", "--calls", "15"]),
    "witness": ("time", ["--job", "0:0:20", "--calls", "20", "--witness"]),
}


def run(kind, argv, lib, tune=""):
    env = dict(os.environ, COSNARKS_HIP_LIB=lib)
    if kind == "bench":
        cmd = ["timeout", "-k", "10", "180"] + argv
    else:
        cmd = ["timeout", "-k", "10", "120", sys.executable, "tools/msm_time.py"] + argv + (["--tune", tune] if tune else [])
    r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        print("CHILD FAILED rc=%d: %s\n%s\n%s" % (r.returncode, " ".join(cmd), r.stdout[-2000:], r.stderr[-2000:]), flush=True)
        sys.exit(1)
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    return (line["ms_per_step"], None) if kind == "bench" else (line["ms_median"], line["result_sha"])


for what in args.what.split(","):
    kind, argv = SHAPES[what]
    order = [("parent", parent, ""), ("new", new, ""), ("parent2", parent, "")]
    if args.extra_tune and kind == "time":
        order.insert(2, ("new_tuned", new, args.extra_tune))
    ms = {k: [] for k, _, _ in order}
    shas = {}
    for rnd in range(args.rounds):
        k = rnd % len(order)
        seq = order[k:] + order[:k]
        for name, lib, tune in (seq if rnd % 2 == 0 else seq[::-1]):
            t, sha = run(kind, argv, lib, tune)
            ms[name].append(t)
            shas.setdefault(name, set()).add(sha)
        print(json.dumps({"what": what, "round": rnd, **{k: v[-1] for k, v in ms.items()}}), flush=True)
    row = {"what": what, "rounds": args.rounds, "ms_median": {k: round(statistics.median(v), 5) for k, v in ms.items()},
           "same_result_words": (len(set().union(*shas.values())) == 1) if kind == "time" else None}
    for name in ms:
        if name == "parent":
            continue
        d = [100 * (a - b) / b for a, b in zip(ms[name], ms["parent"])]
        row[name + "_vs_parent_pct"] = {"median": round(statistics.median(d), 3), "min": round(min(d), 3), "max": round(max(d), 3)}
    print("SUMMARY " + json.dumps(row), flush=True)
