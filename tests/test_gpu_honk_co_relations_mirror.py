"""The host mirror's sumcheck round on shares (co-snarks_amd/host/plonk_honk.hpp: co_compute_round_accumulators and
co_batch_over_relations) through examples/honk_co_sumcheck_from_cpp.cpp: three Rep3 parties in one process on
LocalNetwork::new_parties(3), every stage on the device, and the protocol-0 party with the identity network beside them. What the
program opens must equal tests/honk_co_relations_ref.py's plain side on all 57 values, and the round univariate on all 8."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import helpers as H
from tests import honk_co_relations_ref as CO
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
    exe = str(tmp_path_factory.mktemp("honk_co_sumcheck_mirror") / "honk_co_sumcheck_from_cpp")
    libdir = os.path.join(ROOT, "co-snarks_amd", "lib")
    r = subprocess.run([_clangxx(), "-O1", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "examples", "honk_co_sumcheck_from_cpp.cpp"), "-L" + libdir,
                        "-lcosnarks_hip", "-Wl,-rpath," + libdir, "-lpthread", "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return exe


def check(program, tmp_path, curve, n, polys, params, betas, alphas, seed):
    F = H.FR[curve]
    p = F.p
    gs = R.GateSeparator(p, betas, len(betas))
    head = [H.CURVE_IDS[curve], n, len(betas), gs.periodicity, gs.current_element_idx, seed]
    words = [np.array(head, dtype=np.uint64), H.pack(F, list(params) + [gs.partial_evaluation_result] + betas + alphas).reshape(-1)]
    words += [H.pack(F, polys[name]).reshape(-1) for name in R.COLS]
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    np.concatenate(words).astype("<u8").tofile(fin)
    r = subprocess.run([program, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)
    raw = np.fromfile(fout, dtype="<u8")
    assert raw.size == 4 * (57 + 8 + 57)
    got = H.unpack(F, raw)   # strict: canonical
    want = CO.plain_accumulate(p, polys, 0, n, gs.beta_products, gs.periodicity, params)
    S = R.batch_over_relations_univariates(p, want, alphas, gs.current_element(), gs.partial_evaluation_result)
    assert got[:57] == R.flat_acc(want), "the three Rep3 parties' opened accumulators"
    assert got[57:65] == S, "their opened round univariate"
    assert got[65:] == R.flat_acc(want), "the protocol-0 party with the identity network"
    return S


def test_mirror_on_the_satisfied_trace(gpu, program, tmp_path):
    p = H.FR["bn254"].p
    t = R.satisfied_trace(p)
    r = H.rng(71)
    S = check(program, tmp_path, "bn254", t["n"], t["polys"], t["params"], [r.randrange(1, p) for _ in range(4)], [r.randrange(1, p) for _ in range(10)], 5)
    assert (S[0] + S[1]) % p == 0 and any(S[2:])


@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
def test_mirror_at_two_to_the_eight(gpu, program, tmp_path, curve):
    """n = 2^8, random data with the planted q_arith / q_delta_range skips"""
    p, n = H.FR[curve].p, 1 << 8
    c = CO.random_case(p, n, 9400)
    r = H.rng(72)
    check(program, tmp_path, curve, n, c["polys"], c["params"], [r.randrange(1, p) for _ in range(8)], [r.randrange(1, p) for _ in range(10)], 6)
