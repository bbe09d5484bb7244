"""The host mirror's rounds 2 and 5 (co-snarks_amd/host/plonk_honk.hpp: PlainPlonkDriver::compute_z, compute_r_wxi, compute_wxiw) on the
device against tests/plonk_rounds_ref.py, through examples/plonk_rounds_from_cpp.cpp: a C++ program that calls the three driver methods on
the words of a file. At n = 8 the data is the chain on the reference's multiplier2 circuit (so W_xi and W_xiw are the proof's own opening
quotients), at n = 2^10 it is random (a power table with more than one high entry, more than one workgroup, a division whose remainder
is not zero). Every comparison is exact and covers every element."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import helpers as H
from tests import plonk_rounds_ref as R

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
    exe = str(tmp_path_factory.mktemp("plonk_mirror") / "plonk_rounds_from_cpp")
    libdir = os.path.join(ROOT, "co-snarks_amd", "lib")
    r = subprocess.run([_clangxx(), "-O1", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "examples", "plonk_rounds_from_cpp.cpp"), "-L" + libdir,
                        "-lcosnarks_hip", "-Wl,-rpath," + libdir, "-lpthread", "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return exe


def restated(F, n, w_ext, c):
    """what the three driver methods return for the inputs `c`, from the restatement"""
    from oracle import ntt
    p = F.p
    T = R.Ops(p, 0, 0)
    w = pow(w_ext, 4, p)
    dom, ext = ntt.Domain(F, n, w), ntt.Domain(F, 4 * n, w_ext)
    sh = lambda v: [(x,) for x in v]
    un = lambda v: [x[0] for x in v]
    ops = [un(o) for o in R.z_operands(T, n, w, sh(c["buffer_a"]), sh(c["buffer_b"]), sh(c["buffer_c"]), *c["sigma"], c["beta"], c["gamma"], c["k1"], c["k2"])]
    num, den, z = 1, 1, []
    for i in range(n):
        num = num * ops[0][i] * ops[1][i] * ops[2][i] % p
        den = den * ops[3][i] * ops[4][i] * ops[5][i] % p
        z.append(num * pow(den, -1, p) % p)
    coeffs = dom.ifft(R.rotate_right(z, 1))
    want = {"z_poly": un(R.blind_coefficients(T, sh(coeffs), sh(c["blinders"]))), "z_eval": ext.fft(coeffs + [0] * (3 * n))}
    cs, cp, const0 = R.round5_coefficients(p, n, w, c["public_inputs"], c["ev"], c["beta"], c["gamma"], c["alpha"], c["xi"], c["v"], c["k1"], c["k2"])
    numer = R.poly_lincomb(T, [sh(c["poly"][k]) for k in ("z", "t1", "t2", "t3", "a", "b", "c")], cs,
                           [c["zkey"][k] for k in ("qm", "ql", "qr", "qo", "qc", "s3", "s1", "s2")], cp, const0, n + 6)
    want["wxi"] = un(R.div_linear(T, numer, c["xi"])[0])
    zs = list(c["poly"]["z"])
    zs[0] = (zs[0] - c["ev"]["zw"]) % p
    want["wxiw"] = un(R.div_linear(T, sh(zs), c["xi"] * w % p)[0])
    return want


def run_program(program, tmp_path, curve, n, c):
    F = H.FR[curve]
    words = [np.array([H.CURVE_IDS[curve], n, len(c["public_inputs"])], dtype=np.uint64)]
    el = lambda *xs: words.append(H.pack(F, list(xs)).reshape(-1))
    for v in (c["buffer_a"], c["buffer_b"], c["buffer_c"], *c["sigma"]):
        el(*v)
    el(c["beta"], c["gamma"], c["k1"], c["k2"], *c["blinders"])
    for k in ("z", "t1", "t2", "t3", "a", "b", "c"):
        el(*c["poly"][k])
    for k in ("qm", "ql", "qr", "qo", "qc", "s1", "s2", "s3"):
        el(*c["zkey"][k])
    el(*c["public_inputs"])
    el(*[c["ev"][k] for k in ("a", "b", "c", "s1", "s2", "zw")], c["alpha"], c["xi"], *c["v"])
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    np.concatenate(words).astype("<u8").tofile(fin)
    r = subprocess.run([program, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)
    got = H.unpack(F, np.fromfile(fout, dtype="<u8"))   # strict: canonical
    lens = (("z_poly", n + 3), ("z_eval", 4 * n), ("wxi", n + 5), ("wxiw", n + 2))
    assert len(got) == sum(ln for _, ln in lens)
    out, at = {}, 0
    for name, ln in lens:
        out[name], at = got[at:at + ln], at + ln
    return out


def same(got, want):
    for name in ("z_poly", "z_eval", "wxi", "wxiw"):
        diff = [i for i, (g, w) in enumerate(zip(got[name], want[name])) if g != w]
        assert len(got[name]) == len(want[name]) and not diff, (name, "first difference at", diff[0] if diff else None, "of", len(want[name]))


@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
def test_mirror_on_multiplier2(gpu, program, tmp_path, curve):
    """n = 8, the reference's circuit: compute_z gives the chain's blinded z(X), and the two quotients are the chain's W_xi and W_xiw, which
    its own divisions left with remainder 0"""
    F, o = H.FR[curve], R.fixture_chain(curve)
    zk, n = o["zk"], o["zk"].domain_size
    bufs = R.wire_buffers(F.p, zk, o["additions"], o["maps"], o["witness"])
    c = {"buffer_a": bufs[0], "buffer_b": bufs[1], "buffer_c": bufs[2], "sigma": [zk.polys[k][1] for k in ("S1", "S2", "S3")], "beta": o["beta"],
         "gamma": o["gamma"], "alpha": o["alpha"], "xi": o["xi"], "v": o["v"], "k1": zk.k1, "k2": zk.k2, "blinders": o["b"][6:9], "poly": o["poly"],
         "zkey": {k.lower(): zk.polys[k][0] for k in ("Qm", "Ql", "Qr", "Qo", "Qc", "S1", "S2", "S3")},
         "public_inputs": list(o["witness"][1:zk.n_public + 1]), "ev": o["evals"]}
    got = run_program(program, tmp_path, curve, n, c)
    want = restated(F, n, R.ext_generator(F, n), c)
    same(got, want)
    assert o["wxi_rem"] == 0 and o["wxiw_rem"] == 0
    assert got["z_poly"] == o["poly"]["z"] and got["wxi"] == o["wxi"] and got["wxiw"] == o["wxiw"]


@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
def test_mirror_at_two_to_the_ten(gpu, program, tmp_path, curve):
    """n = 2^10, random data, three public inputs"""
    F = H.FR[curve]
    p, n = F.p, 1 << 10
    r = H.rng(9100)
    el = lambda: r.randrange(1, p)
    vec = lambda k: [el() for _ in range(k)]
    c = {"buffer_a": vec(n), "buffer_b": vec(n), "buffer_c": vec(n), "sigma": [vec(4 * n) for _ in range(3)], "beta": el(), "gamma": el(), "alpha": el(),
         "xi": el(), "v": vec(5), "k1": el(), "k2": el(), "blinders": vec(3),
         "poly": {"z": vec(n + 3), "t1": vec(n + 1), "t2": vec(n + 1), "t3": vec(n + 6), "a": vec(n + 2), "b": vec(n + 2), "c": vec(n + 2)},
         "zkey": {k: vec(n) for k in ("qm", "ql", "qr", "qo", "qc", "s1", "s2", "s3")}, "public_inputs": vec(3),
         "ev": {k: el() for k in ("a", "b", "c", "s1", "s2", "zw")}}
    same(run_program(program, tmp_path, curve, n, c), restated(F, n, R.ext_generator(F, n), c))
