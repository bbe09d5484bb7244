"""GPU tests of the multilinear folds (csh_mle_fold, csh_mle_fold_rounds and the mirror above them) against Python integers: the
reference's loops, written as the reference writes them. Results are compared word for word and checked canonical; every device output
buffer carries a guard behind it that must come back untouched."""
import ctypes as C

import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu
CURVES = ["bn254", "bls12_381", "bls12_377"]
ONE_ROUND_SIZES = [2, 4, 62, 64, 66, 510, 512, 514, (1 << 13) + 2]   # around a wave and a workgroup of pairs, and a ragged last block
KS = [1, 3, 40]
GUARD = np.full(8, 0xDEADBEEFCAFEF00D, dtype=np.uint64)


def reference_fold(p, poly, round_challenge):
    """co_sumcheck_prover.rs:48-50, co_shplemini_prover.rs:260-269."""
    out = [0] * (len(poly) // 2)
    for i in range(0, len(poly) - 1, 2):
        out[i >> 1] = (poly[i] + (poly[i + 1] - poly[i]) * round_challenge) % p
    return out


def reference_levels(p, poly, challenges):
    levels, a_l = [], poly
    for u_l in challenges:
        a_l = reference_fold(p, a_l, u_l)
        levels.append(a_l)
    return levels


def reference_evaluate_mle(p, coefficients, evaluation_points):
    """polynomial.rs:270-312 for 2^dim coefficients, dim <= len(evaluation_points)."""
    dim = (len(coefficients) - 1).bit_length()
    tmp = list(coefficients)
    for val in evaluation_points[:dim]:
        tmp = reference_fold(p, tmp, val)
    result = tmp[0]
    for point in evaluation_points[dim:]:
        result = result * (1 - point) % p
    return result


def reference_fold_polynomials(p, log_n, multilinear_challenge, a_0, has_zk):
    """compute_fold_polynomials (co_shplemini_prover.rs:236-312): the list it returns."""
    fold_polynomials, a_l = [], a_0
    for u_l in multilinear_challenge[:log_n - 1]:
        a_l = reference_fold(p, a_l, u_l)
        fold_polynomials.append(a_l)
    last = fold_polynomials[-1]
    final_eval = (last[0] + multilinear_challenge[log_n - 1] * (last[1] - last[0])) % p
    ind = 0 if has_zk else 1
    fold_polynomials.append([ind * final_eval % p])
    tail = 1
    for challenge in multilinear_challenge[log_n:len(multilinear_challenge) - 1]:
        tail = tail * (1 - challenge) % p
        fold_polynomials.append([ind * (tail * final_eval % p) % p])
    return fold_polynomials


def reference_partially_evaluate(p, poly, round_size, challenges):
    """partially_evaluate_init, then partially_evaluate_inplace per further challenge (co_sumcheck_prover.rs:34-98)."""
    des = reference_fold(p, poly[:round_size], challenges[0])
    for u in challenges[1:]:
        limit = len(des)
        des = reference_fold(p, des, u)[:limit // 2 + limit % 2]
        if len(des) < 2:
            des.append(0)
    return des


def _interleave(per_comp):
    out = [None] * (len(per_comp) * len(per_comp[0]))
    for c, v in enumerate(per_comp):
        out[c::len(per_comp)] = v
    return out


def _levels_want(F, vals, ncomp, us):
    per = [reference_levels(F.p, vals[c::ncomp], us) for c in range(ncomp)]
    return [_interleave([per[c][l] for c in range(ncomp)]) for l in range(len(us))]


def _same(F, got, want_ints, ctx):
    H.assert_canonical(F, got)
    assert np.array_equal(np.asarray(got).reshape(-1), H.pack(F, want_ints)), ctx


class Guarded:
    """A device buffer of `words` u64 with a guard behind it."""

    def __init__(self, gpu, words):
        self.words = words
        self.buf = gpu.DeviceBuffer.from_host(np.concatenate([np.zeros(words, dtype=np.uint64), GUARD]))

    def get(self):
        a = self.buf.to_host()
        assert np.array_equal(a[self.words:], GUARD), "guard word overwritten"
        return a[:self.words]


def _addr(buf, word_offset=0):
    return buf.ptr.value + 8 * word_offset


def fold_dev(gpu, cid, ins, outs, n, ncomp, u_packed):
    """csh_mle_fold_dev on raw device addresses."""
    k = len(ins)
    rc = gpu.lib().csh_mle_fold_dev(cid, (C.c_void_p * k)(*ins), (C.c_void_p * k)(*outs), C.c_size_t(k), C.c_size_t(n), C.c_uint32(ncomp),
                                    u_packed.ctypes.data_as(C.c_void_p), None)
    assert rc == 0, gpu.lib().csh_last_error()


def rounds_dev(gpu, cid, d_in, n, ncomp, us_packed, levels=True, last=True):
    """csh_mle_fold_rounds_dev into guarded buffers -> (levels words or None, last words or None)."""
    m = us_packed.size // 4
    lv = Guarded(gpu, 4 * ncomp * (n - (n >> m))) if levels else None
    la = Guarded(gpu, 4 * ncomp * (n >> m)) if last else None
    gpu.mle_fold_rounds(cid, d_in, us_packed, ncomp=ncomp, n=n, levels=lv.buf if lv else None, last=la.buf if la else None)
    return (lv.get() if lv else None), (la.get() if la else None)


def chain_dev(gpu, cid, d_in, n, ncomp, us_packed):
    """The same chain as m one-round calls -> levels words."""
    m = us_packed.size // 4
    out = Guarded(gpu, 4 * ncomp * (n - (n >> m)))
    src, at = _addr(d_in), 0
    for l in range(m):
        dst = _addr(out.buf, at)
        fold_dev(gpu, cid, [src], [dst], n >> l, ncomp, us_packed[4 * l:4 * l + 4])
        src, at = dst, at + 4 * ncomp * (n >> (l + 1))
    return out.get()


@pytest.fixture(scope="module")
def base():
    """curve -> (F, values, packed, challenge pool): edge values followed by random ones; challenges 0, 1, p - 1 and random."""
    out = {}
    nb = (3 << 13) + 128   # two components of 3 * 2^12 elements, the largest case
    for k, curve in enumerate(CURVES):
        F = H.FR[curve]
        r = H.rng(6100 + k)
        xs = ([v % F.p for v in H.edge_elems(F)] * 2 + H.rand_elems(F, nb, r))[:nb]
        out[curve] = (F, xs, H.pack(F, xs), [0, 1, F.p - 1, r.randrange(2, F.p - 1), r.randrange(2, F.p - 1)])
    return out


@pytest.fixture(scope="module")
def windows(base):
    """(curve, ncomp, u) -> the fold of every pair of elements (i, i + 1), i = 0 .. : a vector that starts at element v folds to the
    entries v, v + 2, ... of it. Computed once."""
    cache = {}

    def get(curve, ncomp, u):
        key = (curve, ncomp, u)
        if key not in cache:
            F, xs, _, _ = base[curve]
            ne = len(xs) // ncomp
            cache[key] = [[(xs[i * ncomp + c] + (xs[(i + 1) * ncomp + c] - xs[i * ncomp + c]) * u) % F.p for c in range(ncomp)] for i in range(ne - 1)]
        return cache[key]
    return get


def _one_round(gpu, base, windows, curve, ncomp, sizes, ks):
    F, xs, px, pool = base[curve]
    cid = H.CURVE_IDS[curve]
    d_in = gpu.DeviceBuffer.from_host(px)
    case = 0
    for n in sizes:
        for k in ks:
            u = pool[case % len(pool)]
            case += 1
            half = 4 * ncomp * (n // 2)
            out = Guarded(gpu, k * half)
            # vector v starts at element v of the shared buffer: the inputs of one call overlap each other
            fold_dev(gpu, cid, [_addr(d_in, 4 * ncomp * v) for v in range(k)], [_addr(out.buf, v * half) for v in range(k)], n, ncomp, H.pack(F, [u]))
            w = windows(curve, ncomp, u)
            want = [x for v in range(k) for j in range(n // 2) for x in w[v + 2 * j]]
            _same(F, out.get(), want, (curve, ncomp, n, k, hex(u)))


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("ncomp", [1, 2])
def test_one_round(gpu, base, windows, curve, ncomp):
    _one_round(gpu, base, windows, curve, ncomp, ONE_ROUND_SIZES, KS)


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("ncomp", [1, 2])
@pytest.mark.parametrize("max_blocks", [1, 3])
def test_one_round_grid_stride(gpu, base, windows, curve, ncomp, max_blocks):
    """vec_max_blocks = 1 and 3: the grid-stride loop iterates, with a ragged last pass."""
    with gpu.tuned(vec_max_blocks=max_blocks):
        _one_round(gpu, base, windows, curve, ncomp, ONE_ROUND_SIZES, KS)


def _rounds_case(gpu, F, cid, vals, packed, n, ncomp, us, ctx):
    """levels only, last only and both, against the round-by-round chain; n = 2^m: last is evaluate_mle."""
    m = len(us)
    pu = H.pack(F, us)
    want = _levels_want(F, vals[:n * ncomp], ncomp, us)
    flat = [x for lv in want for x in lv]
    d_in = gpu.DeviceBuffer.from_host(packed[:4 * n * ncomp])
    for levels, last in ((True, False), (False, True), (True, True)):
        lv, la = rounds_dev(gpu, cid, d_in, n, ncomp, pu, levels, last)
        if levels:
            _same(F, lv, flat, (ctx, "levels", levels, last))
        if last:
            _same(F, la, want[-1], (ctx, "last", levels, last))
            if n == 1 << m:
                assert H.unpack(F, la) == [reference_evaluate_mle(F.p, vals[c:n * ncomp:ncomp], us) for c in range(ncomp)]
    assert np.array_equal(d_in.to_host(), packed[:4 * n * ncomp])


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("ncomp", [1, 2])
def test_rounds_smallest_tile(gpu, base, curve, ncomp):
    """fold_tile_log = 3: n = 2^m for m = 1 .. 9 reaches 1, 2 and 3 launches."""
    F, xs, px, pool = base[curve]
    with gpu.tuned(fold_tile_log=3):
        for m in range(1, 10):
            us = [pool[(m + 2 * i) % len(pool)] for i in range(m)]
            _rounds_case(gpu, F, H.CURVE_IDS[curve], xs, px, 1 << m, ncomp, us, (curve, ncomp, m))


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("ncomp", [1, 2])
def test_rounds_default_tile(gpu, base, curve, ncomp):
    """One full tile, two tiles and a second launch, twelve tiles with a ragged second launch (3 * 2^12, m = 12), one short tile (5 * 2^4, m = 2)."""
    F, xs, px, pool = base[curve]
    assert gpu.tune_get("fold_tile_log") == 10
    r = H.rng(31)
    for n, m in ((1 << 10, 10), (1 << 11, 11), (3 << 12, 12), (5 << 4, 2)):
        us = [pool[(m + i) % len(pool)] if i % 3 == 0 else r.randrange(F.p) for i in range(m)]
        _rounds_case(gpu, F, H.CURVE_IDS[curve], xs, px, n, ncomp, us, (curve, ncomp, n, m))


@pytest.mark.parametrize("curve,ncomp", [("bn254", 1), ("bls12_381", 1), ("bls12_377", 1), ("bn254", 2)])
def test_rounds_three_launches_at_the_default_tile(gpu, curve, ncomp):
    """n = 2^21, m = 21: launches of 10, 10 and 1 rounds (with two components the first round's input is above the fused kernel's size
    limit and goes through the one-round kernel first: 1 + 10 + 10). Levels and last, asked for together and each alone, equal the same
    chain as 21 one-round calls word for word. For levels 1 .. 10 that check is indirect -- against the one-round kernel, which
    test_one_round holds against Python -- because 2^21 Python products per case are too slow here; from level 11 on (2^10 elements and
    fewer) the levels also equal the Python chain continued from the device's level 10."""
    F = H.FR[curve]
    cid = H.CURVE_IDS[curve]
    n, m = 1 << 21, 21
    rs = np.random.RandomState(77)
    packed = H.uniform_limbs(F, rs, n * ncomp).reshape(-1)
    r = H.rng(78)
    us = [0, 1, F.p - 1] + H.rand_elems(F, m - 3, r)
    r.shuffle(us)
    pu = H.pack(F, us)
    d_in = gpu.DeviceBuffer.from_host(packed)
    lv, la = rounds_dev(gpu, cid, d_in, n, ncomp, pu, True, True)
    _, la2 = rounds_dev(gpu, cid, d_in, n, ncomp, pu, False, True)
    lv2, _ = rounds_dev(gpu, cid, d_in, n, ncomp, pu, True, False)
    chain = chain_dev(gpu, cid, d_in, n, ncomp, pu)
    H.assert_canonical(F, lv)
    assert np.array_equal(lv, chain) and np.array_equal(lv2, chain)
    assert np.array_equal(la, lv[-4 * ncomp:]) and np.array_equal(la2, la)
    off = lambda l: 4 * ncomp * (n - (n >> (l - 1)))
    level10 = H.unpack(F, lv[off(10):off(11)])
    want = _levels_want(F, level10, ncomp, us[10:])
    _same(F, lv[off(11):], [x for w in want for x in w], (curve, "levels 11 .. 21"))


@pytest.mark.parametrize("n,m,ncomp", [(3 << 12, 12, 2), (1 << 13, 13, 1)])
def test_decomposition_does_not_change_results(gpu, base, n, m, ncomp):
    """fold_tile_log 3, 6, 10 and 11 give identical words, equal to m calls of the one-round entry and to the Python chain."""
    curve = "bls12_381"
    F, xs, px, pool = base[curve]
    cid = H.CURVE_IDS[curve]
    r = H.rng(41)
    us = [F.p - 1, 0, 1] + H.rand_elems(F, m - 3, r)
    pu = H.pack(F, us)
    d_in = gpu.DeviceBuffer.from_host(px[:4 * n * ncomp])
    chain = chain_dev(gpu, cid, d_in, n, ncomp, pu)
    _same(F, chain, [x for w in _levels_want(F, xs[:n * ncomp], ncomp, us) for x in w], "chain")
    for t in (3, 6, 10, 11):
        with gpu.tuned(fold_tile_log=t):
            lv, la = rounds_dev(gpu, cid, d_in, n, ncomp, pu, True, True)
            _, la2 = rounds_dev(gpu, cid, d_in, n, ncomp, pu, False, True)
        assert np.array_equal(lv, chain), t
        assert np.array_equal(la, chain[-4 * ncomp * (n >> m):]) and np.array_equal(la2, la), t


@pytest.mark.parametrize("n,m,ncomp", [(1 << 22, 22, 1), (1 << 23, 12, 1), (1 << 22, 2, 2), (1 << 22, 1, 2), (3 << 20, 20, 2)])
def test_large_levels_go_one_round_at_a_time(gpu, n, m, ncomp):
    """Above 2^21 values per level csh_mle_fold_rounds runs its leading rounds through the one-round kernel (one, two, two, one and two
    of them here; in the third and fourth case nothing is left to fuse, in the last the fused part ends with one ragged tile of 768). Levels and last,
    together and each alone, equal m one-round calls word for word; the last eleven levels (2^10 elements and fewer) also equal the
    Python chain continued from the device's level m - 11 where the chain is that long."""
    curve = "bls12_381"
    F = H.FR[curve]
    cid = H.CURVE_IDS[curve]
    rs = np.random.RandomState(91)
    packed = H.uniform_limbs(F, rs, n * ncomp).reshape(-1)
    r = H.rng(92)
    us = ([F.p - 1, 0, 1] + H.rand_elems(F, m, r))[:m]
    r.shuffle(us)
    pu = H.pack(F, us)
    d_in = gpu.DeviceBuffer.from_host(packed)
    chain = chain_dev(gpu, cid, d_in, n, ncomp, pu)
    H.assert_canonical(F, chain)
    lv, la = rounds_dev(gpu, cid, d_in, n, ncomp, pu, True, True)
    lv2, _ = rounds_dev(gpu, cid, d_in, n, ncomp, pu, True, False)
    _, la2 = rounds_dev(gpu, cid, d_in, n, ncomp, pu, False, True)
    assert np.array_equal(lv, chain) and np.array_equal(lv2, chain)
    assert np.array_equal(la, chain[-4 * ncomp * (n >> m):]) and np.array_equal(la2, la)
    assert np.array_equal(d_in.to_host(), packed)
    if m > 12:
        off = lambda l: 4 * ncomp * (n - (n >> (l - 1)))
        start = H.unpack(F, lv[off(m - 11):off(m - 10)])
        want = _levels_want(F, start, ncomp, us[m - 11:])
        _same(F, lv[off(m - 10):], [x for w in want for x in w], (n, m, ncomp))


@pytest.mark.parametrize("curve", CURVES)
def test_host_forms_equal_device_forms(gpu, base, curve):
    """Host-pointer forms against the device forms, small and with one vector above the 4 MiB staging threshold (2^18 elements = 8 MiB)."""
    F, xs, px, pool = base[curve]
    cid = H.CURVE_IDS[curve]
    rs = np.random.RandomState(5)
    big = H.uniform_limbs(F, rs, 1 << 18).reshape(-1)
    r = H.rng(6)
    for packed, n, ncomp, m in ((px, 3 << 11, 2, 11), (px, 80, 1, 2), (big, 1 << 18, 1, 18), (big, 1 << 17, 2, 3)):
        data = packed[:4 * n * ncomp]
        us = H.pack(F, [F.p - 1] + H.rand_elems(F, m - 1, r))
        d_in = gpu.DeviceBuffer.from_host(data)
        lv, la = rounds_dev(gpu, cid, d_in, n, ncomp, us, True, True)
        for levels, last in ((True, True), (True, False), (False, True)):
            hl, ha = gpu.mle_fold_rounds(cid, data, us, ncomp=ncomp, levels=levels, last=last)
            assert (hl is None) == (not levels) and (ha is None) == (not last)
            assert hl is None or np.array_equal(hl, lv)
            assert ha is None or np.array_equal(ha, la)
        # one round, two vectors: the two halves (n / 2 elements each)
        h = n // 2
        got = gpu.mle_fold(cid, [data[:4 * ncomp * h], data[4 * ncomp * h:]], us[:4], ncomp=ncomp)
        out = Guarded(gpu, 4 * ncomp * h)
        fold_dev(gpu, cid, [_addr(d_in), _addr(d_in, 4 * ncomp * h)], [_addr(out.buf), _addr(out.buf, 2 * ncomp * h)], h, ncomp, us[:4])
        assert np.array_equal(np.concatenate(got), out.get())
        H.assert_canonical(F, got[0])


@pytest.mark.parametrize("curve", CURVES)
def test_stream_order(gpu, base, curve):
    """fold -> fold -> rounds -> D2H on the calling thread's stream with no synchronisation in between gives the chain's result."""
    F, xs, px, pool = base[curve]
    cid = H.CURVE_IDS[curve]
    n, ncomp = 1 << 13, 2
    r = H.rng(9)
    us = H.rand_elems(F, 13, r)
    pu = H.pack(F, us)
    d_in = gpu.DeviceBuffer.from_host(px[:4 * n * ncomp])
    b1, b2, last = Guarded(gpu, 2 * n * ncomp), Guarded(gpu, n * ncomp), Guarded(gpu, 4 * ncomp)
    fold_dev(gpu, cid, [_addr(d_in)], [_addr(b1.buf)], n, ncomp, pu[0:4])
    fold_dev(gpu, cid, [_addr(b1.buf)], [_addr(b2.buf)], n // 2, ncomp, pu[4:8])
    gpu.mle_fold_rounds(cid, b2.buf, pu[8:], ncomp=ncomp, n=n // 4, levels=None, last=last.buf)
    want = _levels_want(F, xs[:n * ncomp], ncomp, us)
    _same(F, last.get(), want[-1], curve)
    _same(F, b2.get(), want[1], curve)
    _same(F, b1.get(), want[0], curve)


def test_overlap_is_refused_on_the_device_too(gpu, base):
    F, xs, px, pool = base["bn254"]
    d = gpu.DeviceBuffer.from_host(px[:4 * 64])
    u = H.pack(F, [5, 6])
    with pytest.raises(gpu.CoSnarksHipError, match="overlaps"):
        gpu.mle_fold(0, [d], u[:4], n=64, outs=[d])
    with pytest.raises(gpu.CoSnarksHipError, match="overlaps"):
        gpu.mle_fold_rounds(0, d, u, n=64, levels=d, last=None)
    assert np.array_equal(d.to_host(), px[:4 * 64])


# ---- the mirror (host/plonk_honk.hpp) through cog16_driver_mle_fold -------------------------------------------------------------------
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


def _open_all(dev, F, driver, arr):
    if driver == dev.PLAIN:
        return H.unpack(F, arr)
    if driver == dev.REP3:
        return _rep3_open(F, arr.reshape(3, -1, 2, 4))[0]
    return _shamir_open(F, arr.reshape(3, -1, 4))


@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
def test_mirror_compute_fold_polynomials(gpu, curve):
    """log n = 6 and 8 challenges: A_1 .. A_5, the constant fold of round 6, and the constant fold of the one further virtual round the
    reference's take(virtual_log_n - 1) leaves; with ZK the last two are 0."""
    from cosnarks_amd import groth16 as dev
    F = H.FR[curve]
    cid = H.CURVE_IDS[curve]
    r = H.rng(81)
    log_n = 6
    a_0 = H.rand_elems(F, 1 << log_n, r)
    ch = H.rand_elems(F, 8, r)
    for has_zk in (False, True):
        want_list = reference_fold_polynomials(F.p, log_n, ch, a_0, has_zk)
        assert [len(f) for f in want_list] == [32, 16, 8, 4, 2, 1, 1]
        want = [x for f in want_list for x in f]
        assert (want[-2:] == [0, 0]) == has_zk
        for k, driver in enumerate((dev.PLAIN, dev.REP3, dev.SHAMIR)):
            got = dev.driver_mle_fold(cid, driver, "fold_polynomials", [H.pack(F, a_0)], H.pack(F, ch), has_zk=has_zk, seed=20 + k)
            assert _open_all(dev, F, driver, got) == want, (curve, driver, has_zk)
            if driver != dev.PLAIN:
                assert H.unpack(F, got[0].reshape(-1, 4))[:62] != want[:62]   # a share, not the value


@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
def test_mirror_partially_evaluate(gpu, curve):
    """Three sumcheck rounds over 5 public + 7 shared polynomials of 64 entries, and of 4 entries: there the second round leaves one element
    and the reference pushes a zero."""
    from cosnarks_amd import groth16 as dev
    F = H.FR[curve]
    cid = H.CURVE_IDS[curve]
    r = H.rng(82)
    for n in (64, 4):
        polys = [H.rand_elems(F, n, r) for _ in range(12)]
        ch = [r.randrange(F.p), F.p - 1, r.randrange(F.p)]
        want = [reference_partially_evaluate(F.p, f, n, ch) for f in polys]
        m = len(want[0])
        assert m == max(n // 8, 2)
        for k, driver in enumerate((dev.PLAIN, dev.REP3, dev.SHAMIR)):
            pub, sh = dev.driver_mle_fold(cid, driver, "partially_evaluate", [H.pack(F, f) for f in polys], H.pack(F, ch), npub=5, seed=30 + k)
            parties = 1 if driver == dev.PLAIN else 3
            for party in range(parties):   # public polynomials are public: every party holds the values
                assert H.unpack(F, (pub if parties == 1 else pub[party]).reshape(-1, 4)) == [x for f in want[:5] for x in f]
            assert _open_all(dev, F, driver, sh) == [x for f in want[5:] for x in f], (curve, driver, n)
    with pytest.raises(gpu.CoSnarksHipError, match="power of two"):   # a length that would become odd on the way down
        dev.driver_mle_fold(cid, dev.PLAIN, "partially_evaluate", [H.pack(F, H.rand_elems(F, 6, r)) for _ in range(2)], H.pack(F, ch), npub=1)


@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
def test_mirror_evaluate_mle(gpu, curve):
    """2^5 coefficients at 5 points (the reference's own case) and at 8 points: three trivial dimensions, a factor (1 - u) each."""
    from cosnarks_amd import groth16 as dev
    F = H.FR[curve]
    cid = H.CURVE_IDS[curve]
    r = H.rng(83)
    co = H.rand_elems(F, 32, r)
    for npts in (5, 8):
        pts = H.rand_elems(F, npts, r)
        want = [reference_evaluate_mle(F.p, co, pts)]
        for k, driver in enumerate((dev.PLAIN, dev.REP3, dev.SHAMIR)):
            got = dev.driver_mle_fold(cid, driver, "evaluate_mle", [H.pack(F, co)], H.pack(F, pts), seed=40 + k)
            assert _open_all(dev, F, driver, got) == want, (curve, driver, npts)
    with pytest.raises(gpu.CoSnarksHipError, match="evaluate_mle"):
        dev.driver_mle_fold(cid, dev.PLAIN, "evaluate_mle", [H.pack(F, co)], H.pack(F, pts[:4]))
