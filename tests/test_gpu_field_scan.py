"""GPU tests of the field scans (csh_vec_prefix_prod, csh_vec_batch_inverse, csh_eval_poly) against Python integers.

Sizes come from the tune keys: with L = "scan_lane_run", W = 64 L (a wave) and B = L x "scan_tile_lanes" (a tile) the set is
{0, 1, 2, 3} + {L, W, B, 2 B} +- 1 + {2^15 + 3}. One seeded vector of 2^15 + 3 elements per field serves every size: the running product
and the inverses of its first n elements are prefixes of the same two oracle vectors, computed once."""
import numpy as np
import pytest

from oracle import ntt
from tests import helpers as H

pytestmark = pytest.mark.gpu
CURVES = ["bn254", "bls12_381", "bls12_377"]
NMAX = (1 << 15) + 3


def _sizes(hip):
    L = hip.tune_get("scan_lane_run")
    W, B = 64 * L, L * hip.tune_get("scan_tile_lanes")
    return L, W, B, sorted({0, 1, 2, 3, NMAX} | {s + d for s in (L, W, B, 2 * B) for d in (-1, 0, 1)})


def _batch_inverse_ints(p, xs):
    """Montgomery's trick on Python integers (zeros stay zero): 3 n products and one pow instead of n."""
    pre, acc = [], 1
    for x in xs:
        pre.append(acc)
        if x:
            acc = acc * x % p
    inv = pow(acc, -1, p)
    out = [0] * len(xs)
    for i in range(len(xs) - 1, -1, -1):
        if xs[i]:
            out[i] = inv * pre[i] % p
            inv = inv * xs[i] % p
    return out


@pytest.fixture(scope="module")
def vectors():
    """curve -> (F, values, packed values, packed running products, packed inverses); nothing in them is zero."""
    out = {}
    for k, curve in enumerate(CURVES):
        F = H.FR[curve]
        r = H.rng(4100 + k)
        xs = [v % F.p for v in H.edge_elems(F) if v % F.p] + [r.randrange(1, F.p) for _ in range(NMAX)]
        xs = xs[:NMAX]
        prod, acc = [], 1
        for x in xs:
            acc = acc * x % F.p
            prod.append(acc)
        inv = _batch_inverse_ints(F.p, xs)
        assert inv[5] == pow(xs[5], -1, F.p) and inv[-1] == pow(xs[-1], -1, F.p)
        out[curve] = (F, xs, H.pack(F, xs), H.pack(F, prod), H.pack(F, inv))
    return out


def _same(F, got, want, ctx):
    H.assert_canonical(F, got)
    assert np.array_equal(np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)), ctx


@pytest.mark.parametrize("curve", CURVES)
def test_prefix_product(gpu, vectors, curve):
    F, xs, px, pprod, _ = vectors[curve]
    cid = H.CURVE_IDS[curve]
    L, W, B, sizes = _sizes(gpu)
    for n in sizes:
        _same(F, gpu.vec_prefix_prod(cid, px[:4 * n]), pprod[:4 * n], (curve, n))
    # ones; a zero in the middle: everything from there on is 0
    n = 2 * B + 1
    one = H.pack(F, [1])
    _same(F, gpu.vec_prefix_prod(cid, np.tile(one, n)), np.tile(one, n), (curve, "ones"))
    z = B + W + 3
    v = px[:4 * n].copy()
    v[4 * z:4 * z + 4] = 0
    want = pprod[:4 * n].copy()
    want[4 * z:] = 0
    _same(F, gpu.vec_prefix_prod(cid, v), want, (curve, "zero in the middle"))
    # device forms: in place, and into a second buffer with the input left alone
    for n in (W + 1, NMAX):
        d = gpu.DeviceBuffer.from_host(px[:4 * n])
        assert gpu.vec_prefix_prod(cid, d, n=n) is d
        _same(F, d.to_host(), pprod[:4 * n], (curve, n, "in place"))
        d = gpu.DeviceBuffer.from_host(px[:4 * n])
        o = gpu.DeviceBuffer(32 * n)
        gpu.vec_prefix_prod(cid, d, n=n, out=o)
        _same(F, o.to_host(), pprod[:4 * n], (curve, n, "out of place"))
        assert np.array_equal(d.to_host(), px[:4 * n])


@pytest.mark.parametrize("curve", CURVES)
def test_batch_inverse(gpu, vectors, curve):
    F, xs, px, _, pinv = vectors[curve]
    cid = H.CURVE_IDS[curve]
    L, W, B, sizes = _sizes(gpu)
    for n in sizes:
        got, zc = gpu.vec_batch_inverse(cid, px[:4 * n])
        _same(F, got, pinv[:4 * n], (curve, n))
        assert zc == 0
    # zeros at both ends, on the two sides of a tile boundary, two adjacent; one zero alone; only zeros
    n = 2 * B + 1
    for zeros in ([0, n - 1, B - 1, B, W + 5, W + 6], [0], [n - 1], [B - 1], [B], list(range(n))):
        v, want = px[:4 * n].copy(), pinv[:4 * n].copy()
        for z in zeros:
            v[4 * z:4 * z + 4] = 0
            want[4 * z:4 * z + 4] = 0
        got, zc = gpu.vec_batch_inverse(cid, v)
        _same(F, got, want, (curve, zeros[:6]))
        assert zc == len(zeros), (curve, zeros[:6], zc)
    # device forms: in place with a counter, out of place without one (NULL)
    n = NMAX
    v, want = px[:4 * n].copy(), pinv[:4 * n].copy()
    for z in (3, B, n - 2):
        v[4 * z:4 * z + 4] = 0
        want[4 * z:4 * z + 4] = 0
    d = gpu.DeviceBuffer.from_host(v)
    cnt = gpu.DeviceBuffer.from_host(np.array([0xdeadbeef], dtype=np.uint64))   # the call zeroes it
    gpu.vec_batch_inverse(cid, d, n=n, zero_count=cnt)
    _same(F, d.to_host(), want, (curve, "in place"))
    assert int(cnt.to_host()[0]) == 3
    d = gpu.DeviceBuffer.from_host(v)
    o = gpu.DeviceBuffer(32 * n)
    gpu.vec_batch_inverse(cid, d, n=n, out=o, zero_count=None)
    _same(F, o.to_host(), want, (curve, "out of place, no counter"))
    assert np.array_equal(d.to_host(), v)
    got, zc = gpu.vec_batch_inverse(cid, np.zeros(0, dtype=np.uint64))
    assert got.size == 0 and zc == 0


def _eval(F, coeffs, x):
    return ntt.eval_poly_at(F, coeffs, x)


@pytest.mark.parametrize("curve", CURVES)
def test_eval_poly(gpu, vectors, curve):
    F, xs, px, _, _ = vectors[curve]
    cid = H.CURVE_IDS[curve]
    L, W, B, sizes = _sizes(gpu)
    r = H.rng(99)
    x = r.randrange(2, F.p)
    pt = lambda v: H.pack(F, [v])
    # every size at a random point, one component; the coefficients start with edge_elems
    for n in sizes:
        got = H.unpack(F, gpu.eval_poly(cid, px[:4 * n], pt(x)))
        assert got == [_eval(F, xs[:n], x) if n else 0], (curve, n)
    # edge_elems (zero included) at both ends; points 0, 1, p - 1, random and a root of unity whose order divides the lane run,
    # so that x^L = 1 and every power the lanes, waves and tiles combine with collapses to 1; both component counts
    lg = L.bit_length() - 1
    root = ntt.roots_of_unity(F)[1][lg]
    assert pow(root, L, F.p) == 1 and pow(root, L // 2, F.p) != 1
    edge = [v % F.p for v in H.edge_elems(F)]
    for n in (B + 1, NMAX):
        for ncomp in (1, 2):
            co = (edge + xs[:n * ncomp - 2 * len(edge)] + edge[::-1])[:n * ncomp]
            pc = H.pack(F, co)
            for point in (0, 1, F.p - 1, x, root):
                got = H.unpack(F, gpu.eval_poly(cid, pc, pt(point), ncomp=ncomp))
                assert got == [_eval(F, co[c::ncomp], point) for c in range(ncomp)], (curve, n, ncomp, hex(point))
    for ncomp in (1, 2):   # no coefficients: 0
        assert H.unpack(F, gpu.eval_poly(cid, np.zeros(0, dtype=np.uint64), pt(x), ncomp=ncomp)) == [0] * ncomp
    # device form
    n = NMAX // 2
    d = gpu.DeviceBuffer.from_host(px[:8 * n])
    o = gpu.eval_poly(cid, d, pt(x), ncomp=2, n=n)
    assert H.unpack(F, o.to_host()) == [_eval(F, xs[:2 * n][c::2], x) for c in range(2)]


def test_decomposition_does_not_change_results(gpu, vectors):
    """The smallest tile and spine step make the spine walk its totals in several steps at 2^15 + 3 elements (129 and 65 tiles, 64 per
    step), with both lane runs: all three operations give the default setting's bytes, and the oracle's."""
    curve = "bls12_381"
    F, xs, px, pprod, pinv = vectors[curve]
    cid = H.CURVE_IDS[curve]
    n = NMAX
    v, winv = px.copy(), pinv.copy()
    for z in (0, 700, n - 1):
        v[4 * z:4 * z + 4] = 0
        winv[4 * z:4 * z + 4] = 0
    x = H.rng(5).randrange(2, F.p)
    pt = H.pack(F, [x])
    run = lambda: (gpu.vec_prefix_prod(cid, px), gpu.vec_batch_inverse(cid, v), gpu.eval_poly(cid, px[:4 * (n // 2) * 2], pt, ncomp=2))
    base = run()
    _same(F, base[0], pprod, "default prefix product")
    _same(F, base[1][0], winv, "default batch inverse")
    assert base[1][1] == 3
    assert H.unpack(F, base[2]) == [_eval(F, xs[:2 * (n // 2)][c::2], x) for c in range(2)]
    for lane_run in (4, 8):
        with gpu.tuned(scan_lane_run=lane_run, scan_tile_lanes=64, scan_spine_step=64):
            assert -(-n // (lane_run * 64)) > 64          # more tiles than one spine step takes
            got = run()
        assert np.array_equal(got[0], base[0]) and np.array_equal(got[1][0], base[1][0]) and got[1][1] == 3 and np.array_equal(got[2], base[2]), lane_run


# ---- the drivers of the host mirror (host/plonk_honk.hpp) ------------------------------------------------------------------------------
def _rep3_open(F, sh):
    """(3, n, 2, 4) Rep3 shares -> values; checks the replication b[i] == a[i - 1]."""
    a = [H.unpack(F, sh[p, :, 0, :]) for p in range(3)]
    b = [H.unpack(F, sh[p, :, 1, :]) for p in range(3)]
    assert b[0] == a[2] and b[1] == a[0] and b[2] == a[1]
    return [(x + y + z) % F.p for x, y, z in zip(*a)], a


def _shamir_open(F, sh):
    """(3, n, 4) degree-1 Shamir shares at x = 1, 2, 3 -> values, from parties (0, 1) and checked against parties (1, 2)."""
    s = [H.unpack(F, sh[p]) for p in range(3)]
    v01 = [(2 * x - y) % F.p for x, y in zip(s[0], s[1])]
    v12 = [(3 * y - 2 * z) % F.p for y, z in zip(s[1], s[2])]
    assert v01 == v12
    return v01


@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
def test_driver_eval_poly(gpu, curve):
    from cosnarks_amd import groth16 as dev
    F = H.FR[curve]
    cid = H.CURVE_IDS[curve]
    r = H.rng(61)
    n = 777
    co, x = H.rand_elems(F, n, r), r.randrange(F.p)
    want = _eval(F, co, x)
    for drv in (dev.PLAIN, dev.SHAMIR):
        assert H.unpack(F, dev.driver_eval_poly(cid, drv, H.pack(F, co), H.pack(F, [x]))) == [want]
    sh = dev.driver_eval_poly(cid, dev.REP3, H.pack(F, co), H.pack(F, [x]), seed=9)
    got, a = _rep3_open(F, sh.reshape(3, 1, 2, 4))
    assert got == [want] and a[0] != [want]


@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
def test_driver_inv_vec(gpu, curve):
    from cosnarks_amd import groth16 as dev
    F = H.FR[curve]
    cid = H.CURVE_IDS[curve]
    r = H.rng(62)
    n = 777
    vals = [r.randrange(1, F.p) for _ in range(n)]
    want = [pow(v, -1, F.p) for v in vals]
    data = H.pack(F, vals)
    assert H.unpack(F, dev.driver_inv_vec(cid, dev.PLAIN, data)) == want
    assert H.unpack(F, dev.driver_inv_vec(cid, dev.PLAIN, data, in_place=True)) == want
    got, a = _rep3_open(F, dev.driver_inv_vec(cid, dev.REP3, data, seed=5))
    assert got == want and a[0] != want
    assert _rep3_open(F, dev.driver_inv_vec(cid, dev.REP3, data, seed=6, in_place=True))[0] == want
    assert _shamir_open(F, dev.driver_inv_vec(cid, dev.SHAMIR, data, seed=7)) == want
    assert _shamir_open(F, dev.driver_inv_vec(cid, dev.SHAMIR, data, seed=8, in_place=True)) == want
    # one zero: the strict forms fail with the reference's words, the leaking form leaves the zero share there
    z = 300
    vals[z], want[z] = 0, 0
    data = H.pack(F, vals)
    for drv, in_place, msg in ((dev.PLAIN, False, "Cannot invert zero"), (dev.PLAIN, True, "Cannot invert zero"),
                               (dev.REP3, False, "During execution of inverse in MPC: cannot compute inverse of zero"),
                               (dev.REP3, True, "Cannot compute inverse of zero"), (dev.SHAMIR, False, "Cannot compute inverse of zero"),
                               (dev.SHAMIR, True, "Cannot compute inverse of zero")):
        with pytest.raises(gpu.CoSnarksHipError, match=msg):
            dev.driver_inv_vec(cid, drv, data, seed=3, in_place=in_place)
    assert H.unpack(F, dev.driver_inv_vec(cid, dev.PLAIN, data, leaking_zeros=True)) == want
    sh = dev.driver_inv_vec(cid, dev.REP3, data, seed=11, leaking_zeros=True)
    assert _rep3_open(F, sh)[0] == want and not sh[:, z].any()
    sh = dev.driver_inv_vec(cid, dev.SHAMIR, data, seed=12, leaking_zeros=True)
    assert _shamir_open(F, sh) == want and not sh[:, z].any()


@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
def test_driver_array_prod_mul_plain(gpu, curve):
    from cosnarks_amd import groth16 as dev
    F = H.FR[curve]
    cid = H.CURVE_IDS[curve]
    r = H.rng(63)
    n = 777
    arrs = [[r.randrange(1, F.p) for _ in range(n)] for _ in range(3)]
    want, acc = [], 1
    for a, b, c in zip(*arrs):
        acc = acc * a * b * c % F.p
        want.append(acc)
    packed = [H.pack(F, a) for a in arrs]
    assert H.unpack(F, dev.driver_array_prod_mul(cid, *packed)) == want
    assert H.unpack(F, dev.driver_array_prod_mul(cid, *packed, inv=True)) == [pow(v, -1, F.p) for v in want]
