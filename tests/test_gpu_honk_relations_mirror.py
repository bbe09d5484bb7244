"""The host mirror's sumcheck round (co-snarks_amd/host/plonk_honk.hpp: PlainPlonkDriver::compute_round_accumulators and
compute_univariate) on the device against tests/honk_relations_ref.py, through examples/honk_sumcheck_from_cpp.cpp: a C++ program that
calls the two driver methods, and the mirror's plain C++ loop of the same relations, on the words of a file. n = 8 (the satisfied trace
after one fold: a middle round, periodicity 4) and n = 2^10 (random data with planted skip edges, several workgroups). The device, the
plain C++ loop and the restatement must agree on all 57 values, and the round univariate on all 8."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import helpers as H
from tests import honk_relations_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _clangxx():
    """the clang++ that hipcc drives (the build needs it anyway), or one on PATH"""
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))))
    for cand in (os.path.join(rocm, "lib", "llvm", "bin", "clang++"), os.path.join(rocm, "llvm", "bin", "clang++"), shutil.which("clang++")):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("no clang++ beside hipcc or on PATH")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("honk_sumcheck_mirror") / "honk_sumcheck_from_cpp")
    libdir = os.path.join(ROOT, "co-snarks_amd", "lib")
    r = subprocess.run([_clangxx(), "-O1", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "examples", "honk_sumcheck_from_cpp.cpp"), "-L" + libdir,
                        "-lcosnarks_hip", "-Wl,-rpath," + libdir, "-lpthread", "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return exe


def run_program(program, tmp_path, curve, c):
    """c: n, polys, params, betas, alphas, edge_begin, edge_end, periodicity, current_element_idx, partial_evaluation_result
    -> (device accumulators, plain C++ accumulators, round univariate)"""
    F, n = H.FR[curve], c["n"]
    head = [H.CURVE_IDS[curve], n, c["edge_begin"], c["edge_end"], len(c["betas"]), c["periodicity"], c["current_element_idx"]]
    words = [np.array(head, dtype=np.uint64), H.pack(F, list(c["params"]) + [c["partial_evaluation_result"]] + c["betas"] + c["alphas"]).reshape(-1)]
    words += [H.pack(F, c["polys"][name]).reshape(-1) for name in R.COLS]
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    np.concatenate(words).astype("<u8").tofile(fin)
    r = subprocess.run([program, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)
    raw = np.fromfile(fout, dtype="<u8")
    assert raw.size == 4 * (57 + 57 + 8) + 1
    got = H.unpack(F, raw[:-1])   # strict: canonical
    return got[:57], got[57:114], got[114:]


def check(program, tmp_path, curve, c):
    p = H.FR[curve].p
    table = R.beta_products(p, c["betas"], len(c["betas"]))
    want = R.accumulate_range(p, c["polys"], c["edge_begin"], c["edge_end"], table, c["periodicity"], c["params"])
    whole = R.accumulate_range(p, c["polys"], 0, c["n"], table, c["periodicity"], c["params"])
    S = R.batch_over_relations_univariates(p, whole, c["alphas"], c["betas"][c["current_element_idx"]], c["partial_evaluation_result"])
    dev, host, uni = run_program(program, tmp_path, curve, c)
    assert dev == R.flat_acc(want), "compute_round_accumulators against the restatement"
    assert host == R.flat_acc(want), "the plain C++ loop against the restatement"
    assert uni == S, "compute_univariate against the restatement"
    return S


@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
def test_mirror_on_the_satisfied_trace_after_one_fold(gpu, program, tmp_path, curve):
    """n = 8: round 1 of the satisfied trace. S'(0) + S'(1) of what the program wrote equals S(u) of round 0 from the restatement."""
    p = H.FR[curve].p
    t = R.satisfied_trace(p)
    r = H.rng(51)
    betas, alphas, u = [r.randrange(1, p) for _ in range(4)], [r.randrange(1, p) for _ in range(10)], r.randrange(1, p)
    gs = R.GateSeparator(p, betas, 4)
    acc0 = R.accumulate_range(p, t["polys"], 0, 16, gs.beta_products, gs.periodicity, t["params"])
    S0 = R.batch_over_relations_univariates(p, acc0, alphas, gs.current_element(), gs.partial_evaluation_result)
    assert (S0[0] + S0[1]) % p == 0
    gs.partially_evaluate(u)
    folded = {c: R.fold(p, v, u) for c, v in t["polys"].items()}
    c = dict(n=8, polys=folded, params=t["params"], betas=betas, alphas=alphas, edge_begin=0, edge_end=8, periodicity=gs.periodicity,
             current_element_idx=gs.current_element_idx, partial_evaluation_result=gs.partial_evaluation_result)
    S1 = check(program, tmp_path, curve, c)
    assert (S1[0] + S1[1]) % p == R.lagrange_eval(p, S0, u)


@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
def test_mirror_at_two_to_the_ten(gpu, program, tmp_path, curve):
    """n = 2^10, random data with the planted skip edges; the accumulators of the disabled-rows range [n - 4, n) and the round univariate"""
    p, n = H.FR[curve].p, 1 << 10
    c = R.random_case(p, n, 9300)
    r = H.rng(52)
    c.update(betas=[r.randrange(1, p) for _ in range(10)], alphas=[r.randrange(1, p) for _ in range(10)], edge_begin=n - 4, edge_end=n, periodicity=2,
             current_element_idx=0, partial_evaluation_result=1)
    check(program, tmp_path, curve, c)
