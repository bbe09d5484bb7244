"""The host mirror's Oink phase (co-snarks_amd/host/plonk_honk.hpp: PlainPlonkDriver::compute_w4, compute_logderivative_inverses,
compute_grand_product) on the device against tests/honk_oink_ref.py, through examples/honk_oink_from_cpp.cpp: a C++ program that calls the
three driver methods on the words of a file. The data: the two closed permutation instances with the closed lookup instance at n = 16 (so
z_perm and the inverses satisfy their closed forms), and random data at n = 2^10 (more than one workgroup, ranges with gaps, a w_4 shorter
than the trace). Every comparison is exact and covers every element."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import helpers as H
from tests import honk_oink_ref as R

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
    exe = str(tmp_path_factory.mktemp("honk_mirror") / "honk_oink_from_cpp")
    libdir = os.path.join(ROOT, "co-snarks_amd", "lib")
    r = subprocess.run([_clangxx(), "-O1", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "examples", "honk_oink_from_cpp.cpp"), "-L" + libdir,
                        "-lcosnarks_hip", "-Wl,-rpath," + libdir, "-lpthread", "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return exe


def restated(p, c):
    """what the three driver methods return for the inputs `c` (integers), from the restatement"""
    T = R.Ops(p, 0, 0)
    sh = lambda v: [(x,) for x in v]
    n = c["n"]
    w4 = sh(c["w_4"]) + [T.default()] * (n - len(c["w_4"]))   # :133-137
    w4 = [x[0] for x in R.w4_records(T, sh(c["w"][0]), sh(c["w"][1]), sh(c["w"][2]), w4, c["etas"], c["read"], c["write"],
                                     [(g, (t,)) for g, t in c["shared"]])]
    inv = R.lookup_inverses_plain(p, *c["w"], c["tags"], *c["q"], c["tables"], c["q_lookup"], c["beta"], c["gamma"])[2]
    z = R.grand_product_plain(p, n, c["w"] + [w4], c["ident"], c["sigma"], c["beta"], c["gamma"], c["final_active_wire_idx"] + 1, c["ranges"])[1]
    return {"w_4": w4, "lookup_inverses": inv, "z_perm": z}


def run_program(program, tmp_path, curve, c):
    F, n = H.FR[curve], c["n"]
    ranges = c["ranges"] or []
    head = [H.CURVE_IDS[curve], n, c["final_active_wire_idx"], len(c["w_4"]), len(ranges)] + [x for r in ranges for x in r]
    head += [len(c["read"]), len(c["write"]), len(c["shared"])] + list(c["read"]) + list(c["write"]) + [g for g, _ in c["shared"]]
    words = [np.array(head, dtype=np.uint64)]
    el = lambda *xs: words.append(H.pack(F, list(xs)).reshape(-1)) if xs else None
    el(*[t for _, t in c["shared"]])
    for v in (*c["w"], c["w_4"], c["tags"], *c["q"], *c["tables"], c["q_lookup"], *c["ident"], *c["sigma"]):
        el(*v)
    el(*c["etas"], c["beta"], c["gamma"])
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    np.concatenate(words).astype("<u8").tofile(fin)
    r = subprocess.run([program, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)
    got = H.unpack(F, np.fromfile(fout, dtype="<u8"))   # strict: canonical
    assert len(got) == 3 * n
    return {"w_4": got[:n], "lookup_inverses": got[n:2 * n], "z_perm": got[2 * n:]}


def same(got, want):
    for name in ("w_4", "lookup_inverses", "z_perm"):
        diff = [i for i, (g, w) in enumerate(zip(got[name], want[name])) if g != w]
        assert len(got[name]) == len(want[name]) and not diff, (name, "first difference at", diff[0] if diff else None, "of", len(want[name]))


@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
@pytest.mark.parametrize("with_ranges", [False, True])
def test_mirror_on_the_closed_instances(gpu, program, tmp_path, curve, with_ranges):
    """n = 16: the permutation is satisfied with the w_4 that compute_w4 leaves (no memory record touches it), the lookup is satisfied;
    both closed forms hold on what the program wrote"""
    p = H.FR[curve].p
    pc, lc = R.perm_closed(p, with_ranges), R.lookup_closed(p)
    # the lookup instance and the permutation instance are independent circuits: the grand product reads the permutation's wires
    c = dict(n=16, final_active_wire_idx=pc["domain_size"] - 1, ranges=pc["ranges"], w=pc["w"][:3], w_4=pc["w"][3], tags=lc["tags"], q=lc["q"],
             tables=lc["tables"], q_lookup=lc["q_lookup"], ident=pc["ident"], sigma=pc["sigma"], etas=[3, 5, 7], beta=pc["beta"], gamma=pc["gamma"],
             read=[], write=[], shared=[])
    got = run_program(program, tmp_path, curve, c)
    same(got, restated(p, c))
    assert got["w_4"] == pc["w"][3] and got["z_perm"] == pc["z"]
    R.check_perm_closed_form(p, got["z_perm"], pc["w"], pc["ident"], pc["sigma"], pc["beta"], pc["gamma"], pc["rows"], 16, pc["ranges"])
    c = dict(c, w=lc["w"], beta=lc["beta"], gamma=lc["gamma"], read=[0, 9], write=[15], shared=[(4, 1)])
    got = run_program(program, tmp_path, curve, c)
    same(got, restated(p, c))
    assert got["lookup_inverses"] == lc["inv"]
    R.check_lookup_closed_form(p, dict(lc, inv=got["lookup_inverses"]))


@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
@pytest.mark.parametrize("with_ranges", [False, True])
def test_mirror_at_two_to_the_ten(gpu, program, tmp_path, curve, with_ranges):
    """n = 2^10, random data; selectors and tags in {0, 1}, so that some products are zero and stay zero"""
    p, n = H.FR[curve].p, 1 << 10
    r = H.rng(9200 + with_ranges)
    el = lambda: r.randrange(1, p)
    vec = lambda k: [el() for _ in range(k)]
    bits = lambda k: [r.randrange(2) for _ in range(k)]
    rows = [0, n - 1] + r.sample(range(1, n - 1), 40)
    c = dict(n=n, final_active_wire_idx=900, ranges=[(1, 300), (300, 420), (500, 501), (640, 1024)] if with_ranges else None, w=[vec(n) for _ in range(3)],
             w_4=vec(n - 24), tags=bits(n), q=[vec(n) for _ in range(4)], tables=[vec(n) for _ in range(4)], q_lookup=bits(n),
             ident=[vec(n) for _ in range(4)], sigma=[vec(n) for _ in range(4)], etas=vec(3), beta=el(), gamma=el(),
             read=rows[:20], write=rows[20:37], shared=[(g, r.randrange(2)) for g in rows[37:]])
    got = run_program(program, tmp_path, curve, c)
    same(got, restated(p, c))
    assert got["lookup_inverses"].count(0) > n // 8
