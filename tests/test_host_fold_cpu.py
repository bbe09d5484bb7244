"""CPU tests of the host fold of an MSM (csh_msm_fold_partials: Horner over the window sums on 64-bit limbs, csrc/host_fp64.hpp, one
inversion at the end): partial buffers built here from oracle points in XYZZ form with random ZZ / ZZZ, compared with
sum_w 2^offset(w) S_w from the oracle. Balanced window layouts (wide < W), infinity windows, the all-infinity buffer, and window sums at
the edges of the field (x = 0, stored coordinate words p - 1, coordinate value p - 1)."""
import ctypes as C
import struct

import numpy as np
import pytest

from oracle import curves as cv
from oracle import fields as fl
from tests import helpers as H

GROUPS = [("bn254", 0), ("bn254", 1), ("bls12_381", 0), ("bls12_381", 1), ("bls12_377", 0)]
MAGIC, MAX_WINDOWS = 0x4D534D50, 128


def _base(F):
    return F.base if isinstance(F, fl.Fp2) else F


def _elem_bytes(F, v):
    b = _base(F)
    return b"".join(b.to_mont(c).to_bytes(b.nbytes, "little") for c in F.coeffs(v))


def _xyzz(G, P, z, point_bytes):
    """(x z^2, y z^3, z^2, z^3) of the affine point P; all-zero bytes for infinity. z is an element of the coordinate field."""
    if P is None:
        return bytes(2 * point_bytes)
    F = G.F
    zz = F.sqr(z)
    zzz = F.mul(zz, z)
    return b"".join(_elem_bytes(F, v) for v in (F.mul(P[0], zz), F.mul(P[1], zzz), zz, zzz))


def _rand_z(F, r):
    b = _base(F)
    return F.from_coeffs([r.randrange(1, b.p) for _ in range(F.ncoeff())])


def _partial(hip, cid, group, c, wide, entries):
    """PartialHeader (magic, c, W, wide) + W window sums + padding to the fixed stride. entries: XYZZ byte strings."""
    pb = hip.point_bytes(cid, group)
    total = hip.msm_partial_bytes(cid, group)
    hdr = struct.pack("<4I", MAGIC, c, len(entries), wide).ljust(total - MAX_WINDOWS * 2 * pb, b"\0")
    return hdr + b"".join(entries) + bytes(2 * pb * (MAX_WINDOWS - len(entries)))


def _fold(hip, cid, group, buf, nparts):
    out = np.zeros(3 * hip.point_bytes(cid, group) // 16, dtype=np.uint64)
    assert hip.lib().csh_msm_fold_partials(cid, group, buf, C.c_size_t(nparts), out.ctypes.data_as(C.c_void_p)) == 0
    return out


def _horner(G, c, wide, pts):
    """sum_w 2^offset(w) S_w: window w holds c bits for w < wide and c - 1 above (wide = 0: every window c bits)."""
    wide = wide or len(pts)
    acc = None
    for w in reversed(range(len(pts))):
        for _ in range(c if w < wide else c - 1):
            acc = G.double(acc)
        acc = G.add(acc, pts[w])
    return acc


def _points(G, n, r):
    return [G.mul(G.gen, r.randrange(1, G.order)) for _ in range(n)]


@pytest.mark.parametrize("curve,group", GROUPS)
def test_fold_partials_random_zz_matches_oracle(hip, curve, group):
    G = cv.CURVES[curve][group]
    cid = H.CURVE_IDS[curve]
    pb = hip.point_bytes(cid, group)
    r = H.rng(9100 + 2 * cid + group)
    enc = lambda pts: [_xyzz(G, P, _rand_z(G.F, r), pb) for P in pts]
    # uniform windows (wide == W and the legacy wide == 0), balanced windows (wide < W, wide == 1), windows at infinity in the
    # middle, at the bottom and at the top
    layouts = [(5, 6, 6, ()), (5, 6, 0, (2,)), (9, 7, 3, (0,)), (13, 5, 1, (4,)), (4, 9, 8, (3, 4, 8)), (16, 3, 2, ())]
    for c, W, wide, holes in layouts:
        pts = _points(G, W, r)
        for h in holes:
            pts[h] = None
        got = H.jac_to_affine(G, _fold(hip, cid, group, _partial(hip, cid, group, c, wide, enc(pts)), 1))
        assert G.eq(got, _horner(G, c, wide, pts)), (c, W, wide, holes)
    # several partials: two with one layout (summed window by window first), one with another, one empty (W = 0)
    a, b, d = _points(G, 6, r), _points(G, 6, r), _points(G, 4, r)
    b[0] = None
    buf = (_partial(hip, cid, group, 7, 4, enc(a)) + _partial(hip, cid, group, 7, 4, enc(b)) + _partial(hip, cid, group, 0, 0, [])
           + _partial(hip, cid, group, 11, 4, enc(d)))
    want = G.add(G.add(_horner(G, 7, 4, a), _horner(G, 7, 4, b)), _horner(G, 11, 4, d))
    assert G.eq(H.jac_to_affine(G, _fold(hip, cid, group, buf, 4)), want)
    # the same window sum under two different Z: the addition's doubling branch; under Z and with -P: cancellation to (1, 1, 0)
    buf = _partial(hip, cid, group, 7, 4, enc(a)) + _partial(hip, cid, group, 7, 4, enc(a))
    assert G.eq(H.jac_to_affine(G, _fold(hip, cid, group, buf, 2)), G.double(_horner(G, 7, 4, a)))
    buf = _partial(hip, cid, group, 7, 4, enc(a)) + _partial(hip, cid, group, 7, 4, enc([G.neg(P) for P in a]))
    assert H.jac_to_affine(G, _fold(hip, cid, group, buf, 2)) is None


@pytest.mark.parametrize("curve,group", GROUPS)
def test_fold_partials_all_infinity(hip, curve, group):
    G = cv.CURVES[curve][group]
    cid = H.CURVE_IDS[curve]
    pb = hip.point_bytes(cid, group)
    for c, W, wide in ((5, 6, 6), (12, 22, 3)):
        out = _fold(hip, cid, group, _partial(hip, cid, group, c, wide, [bytes(2 * pb)] * W), 1)
        assert H.jac_to_affine(G, out) is None
        one = _elem_bytes(G.F, G.F.one)
        assert out.tobytes() == one + one + bytes(len(one)), "infinity is encoded (1, 1, 0)"


def _x_zero_point(G):
    """(0, sqrt(b)) where b is a square of the base field (it has order 3: the fold is curve arithmetic, no subgroup is assumed)."""
    y = G.F.sqrt(G.b)
    return None if y is None else (0, y)


@pytest.mark.parametrize("curve", ["bn254", "bls12_381", "bls12_377"])
def test_fold_partials_field_edge_values(hip, curve):
    """G1 window sums whose stored coordinates sit at the edges of the base field: x = 0 (where the curve has such a point), and the X
    coordinate x z^2 steered by the choice of z to the stored words p - 1 (value -1 / R) and to the value p - 1 (z^2 = t / x needs t / x
    to be a square: half of the random points)."""
    G = cv.CURVES[curve][0]
    F = G.F
    cid = H.CURVE_IDS[curve]
    pb = hip.point_bytes(cid, 0)
    r = H.rng(9200 + cid)
    pm1_words = (F.p - 1).to_bytes(F.nbytes, "little")
    edge = []                                          # (affine point, z)
    for target in (F.from_mont(F.p - 1), F.p - 1):
        while True:
            P = G.mul(G.gen, r.randrange(1, G.order))
            z = F.sqrt(F.mul(target, F.inv(P[0])))
            if z:
                break
        assert F.mul(P[0], F.sqr(z)) == target
        edge.append((P, z))
    assert _xyzz(G, *edge[0], pb)[:F.nbytes] == pm1_words
    x0 = _x_zero_point(G)
    if x0 is not None:
        assert G.is_on_curve(x0)
        edge += [(x0, 1), (x0, _rand_z(F, r))]
    assert curve == "bn254" or x0 is not None, "BLS12-381 (b = 4) and BLS12-377 (b = 1) have a point with x = 0"
    filler = _points(G, 4, r)
    for c, wide in ((6, 5), (3, 2)):
        for k, (P, z) in enumerate(edge):
            for pos in (0, 2, 4):                      # bottom window (added last), middle, top window (doubled from the start)
                pts = list(filler) + [None]
                pts[pos] = P
                entries = [_xyzz(G, Q, z if w == pos else _rand_z(F, r), pb) for w, Q in enumerate(pts)]
                got = H.jac_to_affine(G, _fold(hip, cid, 0, _partial(hip, cid, 0, c, wide, entries), 1))
                assert G.eq(got, _horner(G, c, wide, pts)), (c, wide, k, pos)
    # every window the same edge sum
    for P, z in edge:
        pts = [P] * 5
        got = H.jac_to_affine(G, _fold(hip, cid, 0, _partial(hip, cid, 0, 4, 5, [_xyzz(G, P, z, pb)] * 5), 1))
        assert G.eq(got, _horner(G, 4, 5, pts))


def _clangxx():
    """The clang++ that hipcc drives (the build needs it anyway), or one on PATH."""
    import os
    import shutil
    hipcc = os.path.realpath(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
    rocm = os.path.dirname(os.path.dirname(hipcc))
    for cand in (os.path.join(rocm, "lib", "llvm", "bin", "clang++"), os.path.join(rocm, "llvm", "bin", "clang++"), shutil.which("clang++")):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("no clang++ beside hipcc or on PATH")


def test_host_field_check_tool(tmp_path):
    """tools/host_field_check.cpp (no HIP, its own main): the unrolled mul / sqr / windowed inv of host_fp64.hpp against the looped forms
    kept beside them, on the 4- and 6-limb fields; built here without the library and run on 2000 random pairs (10^5 by default)."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "host_field_check")
    subprocess.run([_clangxx(), "-O2", "-std=c++17", "-o", exe, os.path.join(root, "tools", "host_field_check.cpp")], check=True, timeout=300)
    r = subprocess.run([exe, "2000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "host_field_check: ok" in r.stdout, (r.returncode, r.stdout, r.stderr)
