"""The host mirror's Poseidon2 (co-snarks_amd/host/mpc.hpp: Poseidon2Hip and its three parties) through examples/poseidon2_from_cpp.cpp: the
plain batch on the device and on the host, a plain tree, then three Rep3 parties and three Shamir parties in one process on
LocalNetwork::new_parties(3) running precompute, permutation_in_place_with_precomputation_packed and a collaborative tree. Everything the
program opens is compared with tests/poseidon2_ref.py word for word; the opened precomputation must be the powers of its own r."""
import os
import subprocess

import numpy as np
import pytest

from tests import helpers as H
from tests import poseidon2_ref as P2
from tests.test_gpu_honk_co_relations_mirror import _clangxx
from tests.test_poseidon2_cpu import params

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("poseidon2_mirror") / "poseidon2_from_cpp")
    libdir = os.path.join(ROOT, "co-snarks_amd", "lib")
    r = subprocess.run([_clangxx(), "-O1", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "examples", "poseidon2_from_cpp.cpp"), "-L" + libdir,
                        "-lcosnarks_hip", "-Wl,-rpath," + libdir, "-lpthread", "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return exe


# t == arity in compression mode (nothing padded) over two layers; the reference's BN254 round numbers in sponge mode over three layers;
# t = 2 on another field
@pytest.mark.parametrize("curve,t,shape,n_perm,arity,mode,n_leaves", [
    ("bn254", 4, "short", 5, 4, P2.COMPRESSION, 16),
    ("bn254", 3, "bn254", 3, 2, P2.SPONGE, 8),
    ("bls12_381", 2, "short", 2, 2, P2.COMPRESSION, 4),
])
def test_mirror(gpu, program, tmp_path, curve, t, shape, n_perm, arity, mode, n_leaves):
    F, P = H.FR[curve], params(curve, t, shape)
    p = P.p
    r = H.rng(400 + 10 * t + n_perm)
    states = [0] * t + [r.randrange(p) for _ in range((n_perm - 2) * t)] + [p - 1] * t
    leaves = [r.randrange(p) for _ in range(n_leaves)]
    head = [H.CURVE_IDS[curve], t, P.rf_b, P.rf_e, P.rp, n_perm, arity, mode, n_leaves, 77]
    elements = [c for row in P.rc_ext for c in row] + P.rc_int + P.diag + states + leaves
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    np.concatenate([np.array(head, dtype=np.uint64), H.pack(F, elements).reshape(-1)]).astype("<u8").tofile(fin)
    run = subprocess.run([program, fin, fout], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip() == "ok", (run.returncode, run.stdout, run.stderr)
    raw = np.fromfile(fout, dtype="<u8")
    n, S = n_perm * t, P2.num_sbox(P) * n_perm
    assert raw.size == 4 * (2 * n + 1 + 2 * (5 * S + n + 1))
    got = H.unpack(F, raw)   # strict: canonical
    want, root = P2.permute_batch(P, states), P2.merkle_tree(P, leaves, arity, mode)
    assert got[:n] == want, "permutation_packed"
    assert got[n:2 * n] == want, "permutation_in_place on the host"
    assert got[2 * n] == root, "the plain tree"
    at = 2 * n + 1
    for kind in ("rep3", "shamir"):
        pre = [got[at + k * S:at + (k + 1) * S] for k in range(5)]
        assert len(set(pre[0])) == S, (kind, "r repeats")
        for k in range(1, 5):
            assert pre[k] == [pow(v, k + 1, p) for v in pre[0]], (kind, "r^%d" % (k + 1))
        at += 5 * S
        assert got[at:at + n] == want, (kind, "permutation_in_place_with_precomputation_packed")
        assert got[at + n] == root, (kind, "the collaborative tree")
        at += n + 1
