"""The host mirror's whole sumcheck round on shares (co-snarks_amd/host/plonk_honk.hpp: co_compute_round_accumulators_all and
co_batch_over_all_relations) through examples/honk_co_gates_from_cpp.cpp: three Rep3 parties in one process on
LocalNetwork::new_parties(3), all nine relations in the reference's order, every stage on the device, and the protocol-0 party with the
identity network beside them. What the program opens must equal the plain sides (tests/honk_co_relations_ref.py,
tests/honk_gates_ref.py) on all 57 + 110 values, and the round univariate over the 28 accumulators on all 8."""
import os
import subprocess

import numpy as np
import pytest

from tests import helpers as H
from tests import honk_co_relations_ref as CO
from tests import honk_gates_ref as G
from tests import honk_relations_ref as R
from tests.test_gpu_honk_co_relations_mirror import _clangxx

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("honk_co_gates_mirror") / "honk_co_gates_from_cpp")
    libdir = os.path.join(ROOT, "co-snarks_amd", "lib")
    r = subprocess.run([_clangxx(), "-O1", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "examples", "honk_co_gates_from_cpp.cpp"), "-L" + libdir,
                        "-lcosnarks_hip", "-Wl,-rpath," + libdir, "-lpthread", "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return exe


def check(program, tmp_path, curve, n, polys, params, gate_params, betas, alphas, seed):
    F = H.FR[curve]
    p = F.p
    gs = R.GateSeparator(p, betas, len(betas))
    head = [H.CURVE_IDS[curve], n, len(betas), gs.periodicity, gs.current_element_idx, seed]
    words = [np.array(head, dtype=np.uint64), H.pack(F, list(params) + [gs.partial_evaluation_result] + betas + alphas + list(gate_params)).reshape(-1)]
    words += [H.pack(F, polys[name]).reshape(-1) for name in R.COLS + G.SELECTORS]
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    np.concatenate(words).astype("<u8").tofile(fin)
    r = subprocess.run([program, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)
    raw = np.fromfile(fout, dtype="<u8")
    assert raw.size == 4 * (167 + 8 + 167)
    got = H.unpack(F, raw)   # strict: canonical
    first = CO.plain_accumulate(p, polys, 0, n, gs.beta_products, gs.periodicity, params)   # perm and lookup never skip on shares
    gates = G.accumulate_range(p, polys, 0, n, gs.beta_products, gs.periodicity, gate_params)
    want = R.flat_acc(first) + [x for a in gates for x in a]
    S = G.batch_over_relations_univariates_all(p, first + gates, alphas, gs.current_element(), gs.partial_evaluation_result)
    assert got[:167] == want, "the three Rep3 parties' opened accumulators"
    assert got[167:175] == S, "their opened round univariate"
    assert got[175:] == want, "the protocol-0 party with the identity network"
    return S


def test_mirror_on_the_satisfied_trace(gpu, program, tmp_path):
    """rows of all five gate kinds"""
    p = H.FR["bn254"].p
    t = G.satisfied_trace(p)
    r = H.rng(71)
    S = check(program, tmp_path, "bn254", t["n"], t["polys"], t["params"], t["gate_params"], [r.randrange(1, p) for _ in range(6)],
              [r.randrange(1, p) for _ in range(G.NUM_ALPHAS)], 5)
    assert (S[0] + S[1]) % p == 0 and any(S[2:])


@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
def test_mirror_at_two_to_the_eight(gpu, program, tmp_path, curve):
    """n = 2^8, random data with the planted skips of all nine selectors' relations"""
    p, n = H.FR[curve].p, 1 << 8
    c = CO.random_case(p, n, 9400)
    g = G.random_case(p, n, 9401)
    polys = dict(c["polys"], **{sel: g["polys"][sel] for sel in G.SELECTORS})
    r = H.rng(72)
    check(program, tmp_path, curve, n, polys, c["params"], g["params"], [r.randrange(1, p) for _ in range(8)],
          [r.randrange(1, p) for _ in range(G.NUM_ALPHAS)], 6)
