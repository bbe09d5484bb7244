"""The host mirror's complete sumcheck round (co-snarks_amd/host/plonk_honk.hpp: PlainPlonkDriver::compute_round_accumulators_gates and
compute_univariate_all) on the device against tests/honk_gates_ref.py, through examples/honk_gates_from_cpp.cpp: a C++ program that calls
the two driver methods, and the mirror's plain C++ loop of the five relations, on the words of a file. n = 32 (the satisfied trace with
every gate kind after one fold: a middle round, periodicity 4) and n = 2^9 (random data with planted skip edges, several workgroups). The
device, the plain C++ loop and the restatement must agree on all 110 values, and the round univariate over all 28 accumulators on all 8."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import helpers as H
from tests import honk_gates_ref as G
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
    exe = str(tmp_path_factory.mktemp("honk_gates_mirror") / "honk_gates_from_cpp")
    libdir = os.path.join(ROOT, "co-snarks_amd", "lib")
    r = subprocess.run([_clangxx(), "-O1", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "examples", "honk_gates_from_cpp.cpp"), "-L" + libdir,
                        "-lcosnarks_hip", "-Wl,-rpath," + libdir, "-lpthread", "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return exe


def write_input(path, curve, c):
    """c: n, polys (41 columns), params, gate_params, betas, alphas (27), edge_begin, edge_end, periodicity, current_element_idx,
    partial_evaluation_result"""
    F = H.FR[curve]
    head = [H.CURVE_IDS[curve], c["n"], c["edge_begin"], c["edge_end"], len(c["betas"]), c["periodicity"], c["current_element_idx"]]
    scalars = list(c["params"]) + [c["partial_evaluation_result"]] + c["betas"] + c["alphas"] + list(c["gate_params"])
    words = [np.array(head, dtype=np.uint64), H.pack(F, scalars).reshape(-1)]
    words += [H.pack(F, c["polys"][name]).reshape(-1) for name in G.ALL_COLS]
    np.concatenate(words).astype("<u8").tofile(path)


def read_output(path, curve):
    """-> (device accumulators, plain C++ accumulators, round univariate)"""
    raw = np.fromfile(path, dtype="<u8")
    assert raw.size == 4 * (110 + 110 + 8) + 1
    got = H.unpack(H.FR[curve], raw[:-1])   # strict: canonical
    return got[:110], got[110:220], got[220:]


def expected(curve, c):
    """-> (the seventeen accumulators of the range, flat; the round univariate over [0, n) and all 28 accumulators)"""
    p = H.FR[curve].p
    table = R.beta_products(p, c["betas"], len(c["betas"]))
    want = G.accumulate_range(p, c["polys"], c["edge_begin"], c["edge_end"], table, c["periodicity"], c["gate_params"])
    whole = (R.accumulate_range(p, c["polys"], 0, c["n"], table, c["periodicity"], c["params"]) +
             G.accumulate_range(p, c["polys"], 0, c["n"], table, c["periodicity"], c["gate_params"]))
    S = G.batch_over_relations_univariates_all(p, whole, c["alphas"], c["betas"][c["current_element_idx"]], c["partial_evaluation_result"])
    return R.flat_acc(want), S


def check(program, tmp_path, curve, c):
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    write_input(fin, curve, c)
    r = subprocess.run([program, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)
    dev, host, uni = read_output(fout, curve)
    want, S = expected(curve, c)
    assert any(want)
    assert host == want, "the plain C++ loop against the restatement"
    assert dev == want, "compute_round_accumulators_gates against the restatement"
    assert dev == host, "the plain C++ loop equals the device entry"
    assert uni == S, "compute_univariate_all against the restatement"
    return S


def satisfied_case(p):
    """round 1 of the satisfied trace: -> (the case, S of round 0 from the restatement, the challenge u)"""
    t = G.satisfied_trace(p)
    r = H.rng(61)
    betas, alphas, u = [r.randrange(1, p) for _ in range(6)], [r.randrange(1, p) for _ in range(G.NUM_ALPHAS)], r.randrange(1, p)
    gs = R.GateSeparator(p, betas, 6)
    n = t["n"]
    acc0 = (R.accumulate_range(p, t["polys"], 0, n, gs.beta_products, gs.periodicity, t["params"]) +
            G.accumulate_range(p, t["polys"], 0, n, gs.beta_products, gs.periodicity, t["gate_params"]))
    S0 = G.batch_over_relations_univariates_all(p, acc0, alphas, gs.current_element(), gs.partial_evaluation_result)
    assert (S0[0] + S0[1]) % p == 0
    gs.partially_evaluate(u)
    folded = {c: R.fold(p, v, u) for c, v in t["polys"].items()}
    c = dict(n=n // 2, polys=folded, params=t["params"], gate_params=t["gate_params"], betas=betas, alphas=alphas, edge_begin=0, edge_end=n // 2,
             periodicity=gs.periodicity, current_element_idx=gs.current_element_idx, partial_evaluation_result=gs.partial_evaluation_result)
    return c, S0, u


def random_mirror_case(p, n=1 << 9):
    """random data with the planted skip edges of both restatements; the disabled-rows range [n - 4, n)"""
    c, base = G.random_case(p, n, 9400), R.random_case(p, n, 9401)
    polys = dict(base["polys"])
    polys.update(c["polys"])       # the nineteen columns of the second entry, its planted selectors among them
    r = H.rng(62)
    return dict(n=n, polys=polys, params=base["params"], gate_params=c["params"], betas=[r.randrange(1, p) for _ in range(9)],
                alphas=[r.randrange(1, p) for _ in range(G.NUM_ALPHAS)], edge_begin=n - 4, edge_end=n, periodicity=2, current_element_idx=0,
                partial_evaluation_result=1)


@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
def test_mirror_on_the_satisfied_trace_after_one_fold(gpu, program, tmp_path, curve):
    """n = 32: round 1 of the satisfied trace. S'(0) + S'(1) of what the program wrote equals S(u) of round 0 from the restatement."""
    p = H.FR[curve].p
    c, S0, u = satisfied_case(p)
    S1 = check(program, tmp_path, curve, c)
    assert (S1[0] + S1[1]) % p == R.lagrange_eval(p, S0, u)


def test_mirror_on_random_data(gpu, program, tmp_path):
    check(program, tmp_path, "bn254", random_mirror_case(H.FR["bn254"].p))
