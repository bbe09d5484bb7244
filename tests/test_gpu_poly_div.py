"""GPU tests of the division by (X - r) (csh_poly_div_linear) against Python integers: the reference's loop, written as the reference
writes it.

Sizes come from the tune keys, as in test_gpu_field_scan.py: with L = "scan_lane_run", W = 64 L (a wave) and B = L x "scan_tile_lanes"
(a tile) the set is {0, 1, 2, 3} + {L, W, B, 2 B} +- 1 + {2^15 + 3}: the lengths at which a lane, wave, tile or spine boundary can be off
by one. One seeded vector of 2^15 + 3 elements per field, starting with edge_elems, serves every case."""
import numpy as np
import pytest

from oracle import ntt
from tests import helpers as H

pytestmark = pytest.mark.gpu
CURVES = ["bn254", "bls12_381", "bls12_377"]
NMAX = (1 << 15) + 3


def reference_recurrence(p, coeffs, root):
    """polynomial.rs:183 ff.: b_i = (a_i - b_(i-1)) (-r)^-1, all n of them -- the quotient is b[:-1], the popped element b[-1]."""
    root_inverse = pow(-root % p, -1, p)
    out, temp = [], 0
    for a in coeffs:
        temp = (a - temp) % p
        temp = temp * root_inverse % p
        out.append(temp)
    return out


def _sizes(hip):
    L = hip.tune_get("scan_lane_run")
    W, B = 64 * L, L * hip.tune_get("scan_tile_lanes")
    return L, W, B, sorted({0, 1, 2, 3, NMAX} | {s + d for s in (L, W, B, 2 * B) for d in (-1, 0, 1)})


@pytest.fixture(scope="module")
def vectors():
    """curve -> (F, values, packed values, random root, the recurrence over all values at that root)."""
    out = {}
    for k, curve in enumerate(CURVES):
        F = H.FR[curve]
        r = H.rng(5200 + k)
        xs = ([v % F.p for v in H.edge_elems(F)] + H.rand_elems(F, NMAX, r))[:NMAX]
        root = r.randrange(2, F.p - 1)
        out[curve] = (F, xs, H.pack(F, xs), root, reference_recurrence(F.p, xs, root))
    return out


def _same(F, got, want_ints, ctx):
    H.assert_canonical(F, got)
    assert np.array_equal(np.asarray(got).reshape(-1), H.pack(F, want_ints)), ctx


def _check(gpu, F, cid, vals, ncomp, root, ctx, sub0=None):
    """Host form on n x ncomp interleaved integers: out and rem against the recurrence of every component."""
    n = len(vals) // ncomp
    out, rem = gpu.poly_div_linear(cid, H.pack(F, vals) if vals else np.zeros(0, dtype=np.uint64), H.pack(F, [root]), ncomp=ncomp,
                                   sub0=H.pack(F, sub0) if sub0 is not None else None)
    src = list(vals)
    if sub0 is not None and n:
        for c in range(ncomp):
            src[c] = (src[c] - sub0[c]) % F.p
    b = [None] * len(vals)
    for c in range(ncomp):
        b[c::ncomp] = reference_recurrence(F.p, src[c::ncomp], root)
    _same(F, out, b[:max(n - 1, 0) * ncomp], ctx)
    _same(F, rem, b[(n - 1) * ncomp:] if n else [0] * ncomp, (ctx, "rem"))
    return out, rem


@pytest.mark.parametrize("curve", CURVES)
def test_every_size_against_the_recurrence(gpu, vectors, curve):
    F, xs, px, root, b = vectors[curve]
    cid = H.CURVE_IDS[curve]
    L, W, B, sizes = _sizes(gpu)
    pr = H.pack(F, [root])
    for n in sizes:   # one component: the recurrence over a prefix is a prefix of the recurrence
        out, rem = gpu.poly_div_linear(cid, px[:4 * n], pr)
        _same(F, out, b[:max(n - 1, 0)], (curve, n))
        _same(F, rem, [b[n - 1] if n else 0], (curve, n, "rem"))
    two = xs + xs[::-1]
    for n in sizes:   # two components, n coefficients each
        _check(gpu, F, cid, two[:2 * n], 2, root, (curve, n, "ncomp 2"))


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("ncomp", [1, 2])
def test_roots_whose_powers_collapse(gpu, vectors, curve, ncomp):
    """1 and p - 1, and a root of unity whose order divides the lane run (and its inverse): every power the lanes, waves and tiles
    combine with is +-1 or 1. Edge values at both ends of the coefficients."""
    F, xs, px, root, _ = vectors[curve]
    cid = H.CURVE_IDS[curve]
    L, W, B, _ = _sizes(gpu)
    omega = ntt.roots_of_unity(F)[1][L.bit_length() - 1]
    assert pow(omega, L, F.p) == 1 and pow(omega, L // 2, F.p) != 1
    edge = [v % F.p for v in H.edge_elems(F)]
    for n in (B + 1, NMAX // ncomp):
        co = (xs[:n * ncomp - len(edge)] + edge[::-1])[:n * ncomp]
        for rt in (1, F.p - 1, omega, pow(omega, -1, F.p)):
            _check(gpu, F, cid, co, ncomp, rt, (curve, n, ncomp, hex(rt)))


@pytest.mark.parametrize("curve", CURVES)
def test_exact_and_inexact_division(gpu, vectors, curve):
    """p = (X - r) q from a random q: the quotient is q and rem is 0. With coefficient 0 changed rem is not 0 and out is still the
    recurrence (Horner from the top would give something else: the reference never checks divisibility)."""
    F, xs, px, root, _ = vectors[curve]
    cid = H.CURVE_IDS[curve]
    L, W, B, _ = _sizes(gpu)
    n = 2 * B + 5
    q = xs[100:100 + n - 1]
    pc = [(-root * q[0]) % F.p] + [(q[i - 1] - root * q[i]) % F.p for i in range(1, n - 1)] + [q[-1]]
    out, rem = _check(gpu, F, cid, pc, 1, root, (curve, "exact"))
    assert H.unpack(F, out) == q and H.unpack(F, rem) == [0]
    pc[0] = (pc[0] + 1) % F.p
    out, rem = _check(gpu, F, cid, pc, 1, root, (curve, "inexact"))
    assert H.unpack(F, rem) != [0] and H.unpack(F, out) != q


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("ncomp", [1, 2])
def test_sub0_is_taken_off_coefficient_zero(gpu, vectors, curve, ncomp):
    F, xs, px, root, _ = vectors[curve]
    cid = H.CURVE_IDS[curve]
    L, W, B, _ = _sizes(gpu)
    r = H.rng(17)
    for n in (1, 2, W + 1):
        vals = xs[:n * ncomp]
        v = [F.p - 1, r.randrange(F.p)][:ncomp]
        packed = H.pack(F, vals)
        before = packed.copy()
        out, rem = _check(gpu, F, cid, vals, ncomp, root, (curve, n, ncomp, "sub0"), sub0=v)
        assert np.array_equal(packed, before)
        moved = list(vals)
        for c in range(ncomp):
            moved[c] = (moved[c] - v[c]) % F.p
        out2, rem2 = gpu.poly_div_linear(cid, H.pack(F, moved), H.pack(F, [root]), ncomp=ncomp)
        assert np.array_equal(out, out2) and np.array_equal(rem, rem2)
        # the device form leaves the input buffer alone
        d = gpu.DeviceBuffer.from_host(packed)
        o = gpu.DeviceBuffer(max(32 * ncomp * (n - 1), 32))
        gpu.poly_div_linear(cid, d, H.pack(F, [root]), ncomp=ncomp, sub0=H.pack(F, v), n=n, out=o)
        assert np.array_equal(d.to_host(), packed)
        assert np.array_equal(o.to_host()[:4 * ncomp * (n - 1)], out)


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("ncomp", [1, 2])
def test_device_forms(gpu, vectors, curve, ncomp):
    F, xs, px, root, _ = vectors[curve]
    cid = H.CURVE_IDS[curve]
    L, W, B, _ = _sizes(gpu)
    pr = H.pack(F, [root])
    r = H.rng(23)
    for n in (W + 1, NMAX // ncomp):
        vals = xs[:n * ncomp]
        packed = px[:4 * n * ncomp]
        b = [None] * len(vals)
        for c in range(ncomp):
            b[c::ncomp] = reference_recurrence(F.p, vals[c::ncomp], root)
        quot, last = b[:(n - 1) * ncomp], b[(n - 1) * ncomp:]
        # in place, with rem: coefficient n - 1 of the buffer is not written
        d = gpu.DeviceBuffer.from_host(packed)
        rem = gpu.DeviceBuffer.from_host(np.full(4 * ncomp, 0xdeadbeef, dtype=np.uint64))
        o, rr = gpu.poly_div_linear(cid, d, pr, ncomp=ncomp, n=n, rem=rem)
        assert o is d and rr is rem
        got = d.to_host()
        _same(F, got[:4 * ncomp * (n - 1)], quot, (curve, n, "in place"))
        assert np.array_equal(got[4 * ncomp * (n - 1):], packed[4 * ncomp * (n - 1):])
        _same(F, rem.to_host(), last, (curve, n, "rem"))
        # out of place, rem = None: the input is left alone
        d = gpu.DeviceBuffer.from_host(packed)
        o = gpu.DeviceBuffer(32 * ncomp * (n - 1))
        gpu.poly_div_linear(cid, d, pr, ncomp=ncomp, n=n, out=o, rem=None)
        _same(F, o.to_host(), quot, (curve, n, "out of place"))
        assert np.array_equal(d.to_host(), packed)
        # accumulate into a longer prefilled buffer with a random scale: out[i] += scale b_i for i < n - 1, nothing else touched
        scale = r.randrange(2, F.p)
        fill = H.rand_elems(F, (n + 5) * ncomp, r)
        acc = gpu.DeviceBuffer.from_host(H.pack(F, fill))
        gpu.poly_div_linear(cid, d, pr, ncomp=ncomp, n=n, out=acc, scale=H.pack(F, [scale]), accumulate=True)
        want = [(f + scale * q) % F.p for f, q in zip(fill, quot)] + fill[(n - 1) * ncomp:]
        _same(F, acc.to_host(), want, (curve, n, "accumulate"))
        # accumulate without a scale: 1
        acc = gpu.DeviceBuffer.from_host(H.pack(F, fill))
        gpu.poly_div_linear(cid, d, pr, ncomp=ncomp, n=n, out=acc, accumulate=True)
        _same(F, acc.to_host(), [(f + q) % F.p for f, q in zip(fill, quot)] + fill[(n - 1) * ncomp:], (curve, n, "accumulate, scale 1"))
        # a scale without accumulate writes scale b_i
        o = gpu.DeviceBuffer.from_host(H.pack(F, fill))
        gpu.poly_div_linear(cid, d, pr, ncomp=ncomp, n=n, out=o, scale=H.pack(F, [scale]))
        _same(F, o.to_host(), [scale * q % F.p for q in quot] + fill[(n - 1) * ncomp:], (curve, n, "scale"))
        assert np.array_equal(d.to_host(), packed)
    with pytest.raises(gpu.CoSnarksHipError, match="accumulate"):
        gpu.poly_div_linear(cid, d, pr, ncomp=ncomp, n=n, accumulate=True)


def test_decomposition_does_not_change_results(gpu, vectors):
    """The smallest tile and spine step make the spine walk its totals in several steps at 2^15 + 3 elements (129 and 65 tiles, 64 per
    step), with both lane runs: the default setting's bytes, and the recurrence."""
    curve = "bls12_381"
    F, xs, px, root, b = vectors[curve]
    cid = H.CURVE_IDS[curve]
    pr = H.pack(F, [root])
    two = np.concatenate([px, px.reshape(-1, 4)[::-1].reshape(-1)])   # NMAX coefficients of two components
    run = lambda: gpu.poly_div_linear(cid, px, pr) + gpu.poly_div_linear(cid, two, pr, ncomp=2, sub0=H.pack(F, [7, F.p - 1]))
    base = run()
    _same(F, base[0], b[:-1], "default")
    _same(F, base[1], b[-1:], "default rem")
    both = xs + xs[::-1]
    both[0], both[1] = (both[0] - 7) % F.p, (both[1] + 1) % F.p
    b2 = [None] * len(both)
    for c in range(2):
        b2[c::2] = reference_recurrence(F.p, both[c::2], root)
    _same(F, base[2], b2[:-2], "default, two components")
    _same(F, base[3], b2[-2:], "default rem, two components")
    for lane_run in (4, 8):
        with gpu.tuned(scan_lane_run=lane_run, scan_tile_lanes=64, scan_spine_step=64):
            assert -(-NMAX // (lane_run * 64)) > 64          # more tiles than one spine step takes
            got = run()
        assert all(np.array_equal(g, w) for g, w in zip(got, base)), lane_run


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
def test_driver_factor_roots(gpu, curve):
    from cosnarks_amd import groth16 as dev
    F = H.FR[curve]
    cid = H.CURVE_IDS[curve]
    r = H.rng(71)
    n = 777
    co, x = H.rand_elems(F, n, r), r.randrange(1, F.p)
    want = reference_recurrence(F.p, co, x)[:-1]
    data, px = H.pack(F, co), H.pack(F, [x])
    for zerofier in (False, True):   # Round5::div_by_zerofier(inout, 1, beta) is the same recurrence
        assert H.unpack(F, dev.driver_factor_roots(cid, dev.PLAIN, data, px, zerofier=zerofier)) == want
        got, a = _rep3_open(F, dev.driver_factor_roots(cid, dev.REP3, data, px, seed=9, zerofier=zerofier))
        assert got == want and a[0] != want
        assert _shamir_open(F, dev.driver_factor_roots(cid, dev.SHAMIR, data, px, seed=10, zerofier=zerofier)) == want
    # root 0: the shift
    zero = H.pack(F, [0])
    assert H.unpack(F, dev.driver_factor_roots(cid, dev.PLAIN, data, zero)) == co[1:]
    assert _rep3_open(F, dev.driver_factor_roots(cid, dev.REP3, data, zero, seed=11))[0] == co[1:]
    assert _shamir_open(F, dev.driver_factor_roots(cid, dev.SHAMIR, data, zero, seed=12)) == co[1:]
    with pytest.raises(gpu.CoSnarksHipError, match="Highly unlikely to be zero"):
        dev.driver_factor_roots(cid, dev.PLAIN, data, zero, zerofier=True)


@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
def test_driver_batched_quotient(gpu, curve):
    """Q = sum_j nu^j (f_j - v_j) / (X - x_j) over five claims of lengths 512, 256, 256, 128 and 3 at distinct points, accumulated on the
    device; v_j = f_j(x_j) for all but one claim (that one's quotient is still the recurrence)."""
    from cosnarks_amd import groth16 as dev
    F = H.FR[curve]
    cid = H.CURVE_IDS[curve]
    r = H.rng(72)
    lens = [512, 256, 256, 128, 3]
    polys = [H.rand_elems(F, n, r) for n in lens]
    points = [r.randrange(1, F.p) for _ in lens]
    assert len(set(points)) == len(points)
    evals = [ntt.eval_poly_at(F, f, x) for f, x in zip(polys, points)]
    evals[2] = (evals[2] + 5) % F.p
    nu = r.randrange(2, F.p)
    want, cur = [0] * max(lens), 1
    for f, x, v in zip(polys, points, evals):
        q = reference_recurrence(F.p, [(f[0] - v) % F.p] + f[1:], x)[:-1]
        for i, c in enumerate(q):
            want[i] = (want[i] + cur * c) % F.p
        cur = cur * nu % F.p
    args = ([H.pack(F, f) for f in polys], H.pack(F, points), H.pack(F, evals), H.pack(F, [nu]))
    assert H.unpack(F, dev.driver_batched_quotient(cid, dev.PLAIN, *args)) == want
    got, a = _rep3_open(F, dev.driver_batched_quotient(cid, dev.REP3, *args, seed=13))
    assert got == want and a[0] != want
    assert _shamir_open(F, dev.driver_batched_quotient(cid, dev.SHAMIR, *args, seed=14)) == want
