"""The host mirror's Shamir preprocessing (co-snarks_amd/host/mpc.hpp: ShamirPreprocessingHip; host/sharefile.hpp: SeededShare::expand_dev)
through examples/shamir_preprocessing_from_cpp.cpp: n parties as threads on LocalNetwork::new_parties(n) run get_shared_rngs, generate
their double sharings on the device, move them into the host ShamirState and run one mul_vec on them. The opened pairs and the opened
product are compared with tests/shamir_rng_ref.py word for word; the program itself checks that every pair opens alike from both degrees
and that expand_dev equals expand(); a fork of one pair (fork_with_pairs) generates a batch from its own streams."""
import os
import subprocess

import numpy as np
import pytest

from tests import helpers as H
from tests import shamir_rng_ref as R
from tests.test_gpu_honk_co_relations_mirror import _clangxx

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("shamir_rng_mirror") / "shamir_preprocessing_from_cpp")
    libdir = os.path.join(ROOT, "co-snarks_amd", "lib")
    r = subprocess.run([_clangxx(), "-O1", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "examples", "shamir_preprocessing_from_cpp.cpp"), "-L" + libdir,
                        "-lcosnarks_hip", "-Wl,-rpath," + libdir, "-lpthread", "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return exe


def words32(b):
    return np.frombuffer(b, dtype="<u8")


@pytest.mark.parametrize("curve,n,t,amount,m,seeded_len", [("bn254", 3, 1, 9, 9, 1), ("bls12_381", 5, 2, 7, 5, 1000)])
def test_mirror(gpu, program, tmp_path, curve, n, t, amount, m, seeded_len):
    F = H.FR[curve]
    rnd = H.rng(10 * n + t)
    master, share_seed = bytes(rnd.randrange(256) for _ in range(32)), bytes(rnd.randrange(256) for _ in range(32))
    a, b = H.rand_elems(F, m - 2, rnd) + [0, F.p - 1], H.rand_elems(F, m, rnd)
    head = np.array([H.CURVE_IDS[curve], n, t, amount, m, seeded_len], dtype=np.uint64)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    np.concatenate([head, words32(master), words32(share_seed), H.pack(F, a + b).reshape(-1)]).astype("<u8").tofile(fin)
    run = subprocess.run([program, fin, fout], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip() == "ok", (run.returncode, run.stdout, run.stderr)
    got = H.unpack(F, np.fromfile(fout, dtype="<u8"))  # strict: canonical
    items = -(-amount // (t + 1))
    pairs = items * (t + 1)
    assert len(got) == pairs + m + seeded_len + t + 1
    ref, _ = R.make_parties(F, n, t, master)  # party p's own generator: candidate p of the master stream, as in the program
    R.run_double_share(ref, items, n, t)
    want, want_2t = R.open_pairs(F, ref, n, t, 0)
    assert want == want_2t and got[:pairs] == want, "the opened pairs"
    assert got[pairs:pairs + m] == [x * y % F.p for x, y in zip(a, b)], "mul_vec on generated pairs"
    raw, _ = R.field_rand_ref(F, share_seed, 0, seeded_len)
    assert got[pairs + m:pairs + m + seeded_len] == [v * F.Rinv % F.p for v in raw], "expand_dev"
    kids = [p.fork_with_pairs(1) for p in ref]
    R.run_double_share(kids, 1, n, t)
    kid_t, kid_2t = R.open_pairs(F, kids, n, t, 0)
    assert kid_t == kid_2t and kid_t[0] == want[0] and got[pairs + m + seeded_len:] == kid_t[1:], "fork_with_pairs and the fork's own double share"
