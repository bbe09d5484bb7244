"""GPU parity of the element-wise kernels (vec_ops.hip, the row kernel of sparse.hip, k_bit_reverse / k_powers of ntt.hip) against
Python integers and the oracle: edge values, grid-stride loops that iterate more than once, natural-order transforms and coset
tables beyond 2^13, csh_lincomb at its limits. Every comparison is exact."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import cbridge, chacha, mpc, ntt
from oracle import groth16 as og
from tests import helpers as H
from tests.test_gpu_fullsize import _structured

pytestmark = pytest.mark.gpu
CURVES = ["bn254", "bls12_381", "bls12_377"]


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _padded_len(n):
    """n + 37 seeded random elements behind the cases, and never a multiple of the 256-lane workgroup"""
    n += 37
    return n + 1 if n % 256 == 0 else n


def _pad(F, r, col, n):
    """a column of case operands (None = the operand is absent in that case: any element) -> n integers, the tail seeded random"""
    return [r.randrange(F.p) if v is None else v for v in col] + H.rand_elems(F, n - len(col), r)


def _exact(F, got, want):
    H.assert_canonical(F, got)
    assert H.unpack(F, got) == want


def vec_mul_sub(gpu, cid, a, b, c, alias):
    """csh_selftest_vec_mul_sub_dev: the launcher csh_groth16_h_dev ends a plain / Shamir witness map with; alias: c is the output buffer"""
    out = np.empty_like(a)
    gpu.bindings._check(gpu.lib().csh_selftest_vec_mul_sub_dev(cid, _ptr(a), _ptr(b), _ptr(c), _ptr(out), C.c_size_t(a.size // 4), int(alias)))
    return out


def rep3_local_mul_sub(gpu, cid, lhs, rhs, mask, sub, alias):
    """csh_selftest_rep3_local_mul_sub_dev: the launcher a Rep3 witness map ends with; mask / sub may be None; alias: sub is the output buffer"""
    n = lhs.size // 8
    out = np.empty(4 * n, dtype=np.uint64)
    gpu.bindings._check(gpu.lib().csh_selftest_rep3_local_mul_sub_dev(cid, _ptr(lhs), _ptr(rhs), _ptr(mask), _ptr(sub), _ptr(out), C.c_size_t(n), int(alias)))
    return out


def rep3_masks(gpu, cid, k1, e1, k2, e2, n):
    out = np.zeros(4 * n, dtype=np.uint64)
    gpu.bindings._check(gpu.lib().csh_rep3_masks(cid, k1, C.c_uint64(e1), k2, C.c_uint64(e2), _ptr(out), C.c_size_t(n)))
    return out


# ---- D1: edge values on the device -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_two_operand_kernels_at_the_edges_of_the_field(gpu, curve):
    """vec_mul, vec_add, vec_sub, vec_mul_table (one and two components) on all pairs of the edge set, padded with random elements to a
    length that is no multiple of 256: exact and canonical."""
    F, cid = H.FR[curve], H.CURVE_IDS[curve]
    p = F.p
    r = H.rng(9100)
    pairs = H.elementwise_cases(F)["pairs"]
    n = _padded_len(len(pairs))
    a, b = _pad(F, r, [x for x, _ in pairs], n), _pad(F, r, [y for _, y in pairs], n)
    pa, pb = H.pack(F, a), H.pack(F, b)
    _exact(F, gpu.vec_mul(cid, pa, pb), [x * y % p for x, y in zip(a, b)])
    _exact(F, gpu.vec_add(cid, pa, pb), [(x + y) % p for x, y in zip(a, b)])
    _exact(F, gpu.vec_sub(cid, pa, pb), [(x - y) % p for x, y in zip(a, b)])
    _exact(F, gpu.vec_mul_table(cid, pa, pb), [x * y % p for x, y in zip(a, b)])
    # two components: the share {a[i], a2[i]} times table[i]; both components see every edge pair
    a2 = a[::-1]
    sh = H.pack_shares(F, list(zip(a, a2)))
    want = [v for x, x2, y in zip(a, a2, b) for v in (x * y % p, x2 * y % p)]
    _exact(F, gpu.vec_mul_table(cid, sh, pb, ncomp=2), want)
    _exact(F, gpu.vec_add(cid, sh, H.pack_shares(F, list(zip(b, a))), ncomp=2), [v for x, x2, y in zip(a, a2, b) for v in ((x + y) % p, (x2 + x) % p)])
    _exact(F, gpu.vec_sub(cid, sh, H.pack_shares(F, list(zip(b, a))), ncomp=2), [v for x, x2, y in zip(a, a2, b) for v in ((x - y) % p, (x2 - x) % p)])


@pytest.mark.parametrize("curve", CURVES)
def test_mul_sub_at_the_edges_of_the_field(gpu, curve):
    """a b - c through the launcher of the h pipeline (k_vec_mul_sub): every edge pair, results of exactly 0, 1 and p - 1 included, with c in
    a buffer of its own and with c in the output buffer (how csh_groth16_h_dev calls it)."""
    F, cid = H.FR[curve], H.CURVE_IDS[curve]
    r = H.rng(9200)
    cases = H.elementwise_cases(F)["mul_sub"]
    n = _padded_len(len(cases))
    a, b, c = (_pad(F, r, [t[k] for t in cases], n) for k in range(3))
    want = [(x * y - z) % F.p for x, y, z in zip(a, b, c)]
    assert want[:len(cases)] == [t[3] for t in cases]
    pa, pb, pc = H.pack(F, a), H.pack(F, b), H.pack(F, c)
    for alias in (0, 1):
        _exact(F, vec_mul_sub(gpu, cid, pa, pb, pc, alias), want)


@pytest.mark.parametrize("curve", CURVES)
def test_rep3_local_mul_at_the_edges_of_the_field(gpu, curve):
    """The Rep3 product plus mask minus sub (k_rep3_local_mul) on the case list of the host self-test: through csh_rep3_local_mul_vec (no
    sub operand) and through the launcher of the h pipeline with mask and sub, with each of them absent, and with sub in the output buffer."""
    F, cid = H.FR[curve], H.CURVE_IDS[curve]
    p = F.p
    r = H.rng(9300)
    cases = H.elementwise_cases(F)["rep3"]
    for with_mask, with_sub in ((True, True), (True, False), (False, True)):
        sel = [t for t in cases if (t[4] is not None) == with_mask and (t[5] is not None) == with_sub]
        assert len(sel) == len(cases) // 3
        n = _padded_len(len(sel))
        la, lb, ra, rb, m, s = (_pad(F, r, [t[k] for t in sel], n) for k in range(6))
        want = [(w * (y + z) + x * y + (mm if with_mask else 0) - (ss if with_sub else 0)) % p for w, x, y, z, mm, ss in zip(la, lb, ra, rb, m, s)]
        assert want[:len(sel)] == [t[6] for t in sel]
        pl, pr = H.pack_shares(F, list(zip(la, lb))), H.pack_shares(F, list(zip(ra, rb)))
        pm, ps = H.pack(F, m) if with_mask else None, H.pack(F, s) if with_sub else None
        _exact(F, rep3_local_mul_sub(gpu, cid, pl, pr, pm, ps, 0), want)
        if with_sub:
            _exact(F, rep3_local_mul_sub(gpu, cid, pl, pr, pm, ps, 1), want)
        else:
            _exact(F, gpu.rep3_local_mul_vec(cid, pl, pr, pm), want)


@pytest.mark.parametrize("curve", CURVES)
def test_rep3_to_shamir_at_the_edges_of_the_field(gpu, curve):
    """a x + b y (k_rep3_to_shamir): every edge pair as the share, the three parties' translation points and (0, 0), (1, p - 1), (p - 1, p - 1)."""
    F, cid = H.FR[curve], H.CURVE_IDS[curve]
    r = H.rng(9400)
    cases = H.elementwise_cases(F)["to_shamir"]
    points = sorted(set((t[2], t[3]) for t in cases))
    assert len(points) == 6
    for x, y in points:
        sel = [t for t in cases if (t[2], t[3]) == (x, y)]
        n = _padded_len(len(sel))
        a, b = _pad(F, r, [t[0] for t in sel], n), _pad(F, r, [t[1] for t in sel], n)
        want = [(u * x + v * y) % F.p for u, v in zip(a, b)]
        assert want[:len(sel)] == [t[4] for t in sel]
        _exact(F, gpu.rep3_to_shamir_vec(cid, H.pack_shares(F, list(zip(a, b))), H.pack(F, [x]), H.pack(F, [y])), want)


# ---- D2: capped grids --------------------------------------------------------------------------------------------------------------
_CAP_N = 2000   # one block: eight passes, the last with 208 lanes; three blocks (stride 768): three, three and two passes


@functools.lru_cache(maxsize=None)
def _capped_inputs(curve):
    F = H.FR[curve]
    p = F.p
    r = H.rng(9500)
    n = _CAP_N
    v = {k: H.rand_elems(F, n, r) for k in ("a", "b", "c", "la", "lb", "ra", "rb", "m", "s", "t")}
    x, y = mpc.rep3_to_shamir_points(F, 1)
    coeffs = [1, 0, p - 1] + H.rand_elems(F, 2, r)
    want = {
        "mul": [a * b % p for a, b in zip(v["a"], v["b"])],
        "add": [(a + b) % p for a, b in zip(v["a"], v["b"])],
        "sub": [(a - b) % p for a, b in zip(v["a"], v["b"])],
        "table2": [w for la, lb, t in zip(v["la"], v["lb"], v["t"]) for w in (la * t % p, lb * t % p)],
        "rep3": [(la * (ra + rb) + lb * ra + m) % p for la, lb, ra, rb, m in zip(v["la"], v["lb"], v["ra"], v["rb"], v["m"])],
        "shamir": [(la * x + lb * y) % p for la, lb in zip(v["la"], v["lb"])],
        "lin_unit": [(a + b + c) % p for a, b, c in zip(v["a"], v["b"], v["c"])],
        "lin_mul": [sum(k * e for k, e in zip(coeffs, es)) % p for es in zip(v["a"], v["b"], v["c"], v["m"], v["s"])],
        "mul_sub": [(a * b - c) % p for a, b, c in zip(v["a"], v["b"], v["c"])],
        "rep3_sub": [(la * (ra + rb) + lb * ra + m - s) % p for la, lb, ra, rb, m, s in zip(v["la"], v["lb"], v["ra"], v["rb"], v["m"], v["s"])],
    }
    packed = {k: H.pack(F, e) for k, e in v.items()}
    packed["l"], packed["r"] = H.pack_shares(F, list(zip(v["la"], v["lb"]))), H.pack_shares(F, list(zip(v["ra"], v["rb"])))
    packed["x"], packed["y"], packed["coeffs"] = H.pack(F, [x]), H.pack(F, [y]), H.pack(F, coeffs)
    keys = (bytes(range(1, 33)), bytes(range(101, 133)))
    e1, e2 = 7, 11
    fs = 32   # bytes of keystream per element: ceil(MODULUS_BIT_SIZE / 8) on all three fields
    want["masks"] = mpc.masks_from_streams(F, chacha.keystream(keys[0], fs * n, start_byte=fs * e1), chacha.keystream(keys[1], fs * n, start_byte=fs * e2), n)
    return packed, want, keys, (e1, e2)


def _capped_run(gpu, curve):
    """every kernel of vec_ops.hip at n = 2000 under the current vec_max_blocks -> {name: raw output}"""
    cid = H.CURVE_IDS[curve]
    pk, _, keys, (e1, e2) = _capped_inputs(curve)
    one3 = H.pack(H.FR[curve], [1, 1, 1])
    return {
        "mul": gpu.vec_mul(cid, pk["a"], pk["b"]),
        "add": gpu.vec_add(cid, pk["a"], pk["b"]),
        "sub": gpu.vec_sub(cid, pk["a"], pk["b"]),
        "table1": gpu.vec_mul_table(cid, pk["a"], pk["b"]),
        "table2": gpu.vec_mul_table(cid, pk["l"], pk["t"], ncomp=2),
        "rep3": gpu.rep3_local_mul_vec(cid, pk["l"], pk["r"], pk["m"]),
        "shamir": gpu.rep3_to_shamir_vec(cid, pk["l"], pk["x"], pk["y"]),
        "masks": rep3_masks(gpu, cid, keys[0], e1, keys[1], e2, _CAP_N),
        "lin_unit": gpu.lincomb(cid, [pk["a"], pk["b"], pk["c"]], one3),
        "lin_mul": gpu.lincomb(cid, [pk["a"], pk["b"], pk["c"], pk["m"], pk["s"]], pk["coeffs"]),
        "mul_sub": vec_mul_sub(gpu, cid, pk["a"], pk["b"], pk["c"], 0),
        "mul_sub_alias": vec_mul_sub(gpu, cid, pk["a"], pk["b"], pk["c"], 1),
        "rep3_sub": rep3_local_mul_sub(gpu, cid, pk["l"], pk["r"], pk["m"], pk["s"], 0),
        "rep3_sub_alias": rep3_local_mul_sub(gpu, cid, pk["l"], pk["r"], pk["m"], pk["s"], 1),
    }


@pytest.fixture(scope="module")
def default_launch(gpu):
    """The default launch (one element per lane at this size) of every kernel per curve, checked against the oracle once."""
    cache = {}

    def get(curve):
        if curve not in cache:
            F = H.FR[curve]
            assert gpu.bindings.tune_get("vec_max_blocks") >= 8
            out = _capped_run(gpu, curve)
            want = _capped_inputs(curve)[1]
            for name, got in out.items():
                _exact(F, got, want[{"table1": "mul", "mul_sub_alias": "mul_sub", "rep3_sub_alias": "rep3_sub"}.get(name, name)])
            cache[curve] = out
        return cache[curve]
    return get


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("max_blocks", [1, 3])
def test_grid_stride_loops_under_a_capped_grid(gpu, default_launch, curve, max_blocks):
    """Tune vec_max_blocks = 1 and 3 at n = 2000: every grid-stride loop of vec_ops.hip makes several passes with a ragged last one (one
    block: eight passes, the last with 208 lanes; three blocks: stride 768 and unequal pass counts). Byte for byte what the default
    launch returns, which equals the oracle; the masks' stream offsets are e + i, so a wrong i shows there too."""
    base = default_launch(curve)
    with gpu.tuned(vec_max_blocks=max_blocks):
        capped = _capped_run(gpu, curve)
    assert gpu.bindings.tune_get("vec_max_blocks") >= 8
    for name, got in capped.items():
        assert np.array_equal(got, base[name]), (name, max_blocks, int(np.nonzero(got.reshape(-1, 4) != base[name].reshape(-1, 4))[0][0]))


# ---- D3: csh_lincomb ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("k", [1, 16])
def test_lincomb_at_its_limits(gpu, curve, k):
    """k = 1 and k = 16 (MAX_LINCOMB) share vectors of 1000 elements; coefficients all one (the unit path: plain sums), all one except a
    single p - 1 (one coefficient switches to the multiply path), all zero, and a mix of 0, 1, p - 1 and random."""
    F, cid = H.FR[curve], H.CURVE_IDS[curve]
    p = F.p
    r = H.rng(9600 + k)
    n = 1000
    edge = H.elementwise_edge_set(F)
    shares = [(edge[j % len(edge):] + H.rand_elems(F, n, r))[:n] for j in range(k)]
    packed = [H.pack(F, s) for s in shares]
    mix = [(0, 1, p - 1, r.randrange(p))[j % 4] for j in range(k)]
    for coeffs in ([1] * k, [1] * (k - 1) + [p - 1], [1] * (k // 2) + [p - 1] + [1] * (k - k // 2 - 1), [0] * k, mix):
        want = [sum(c * s[i] for c, s in zip(coeffs, shares)) % p for i in range(n)]
        _exact(F, gpu.lincomb(cid, packed, H.pack(F, coeffs)), want)


@pytest.mark.parametrize("k", [0, 17])
def test_lincomb_refuses_k_outside_its_limits(gpu, k):
    """k = 0 and k = 17 are refused with the limit in the message, before anything is launched (the output is left as it was)."""
    F, cid = H.FR["bn254"], H.CURVE_IDS["bn254"]
    n = 8
    sh = [H.pack(F, list(range(1, n + 1))) for _ in range(max(k, 1))]
    arr = (C.c_void_p * len(sh))(*[s.ctypes.data for s in sh])
    co = H.pack(F, [1] * max(k, 1))
    out = np.full(4 * n, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    with pytest.raises(gpu.CoSnarksHipError, match="1 <= k <= 16"):
        gpu.bindings._check(gpu.lib().csh_lincomb(cid, arr, _ptr(co), C.c_size_t(k), _ptr(out), C.c_size_t(n)))
    assert (out == 0x5A5A5A5A5A5A5A5A).all()


# ---- D4: the row kernel beyond 2^20 rows -------------------------------------------------------------------------------------------
_ROWS, _ROWS_OUT, _NPUB, _NWIT = (1 << 20) + 300, (1 << 20) + 513, 5, 1019


@pytest.fixture(scope="module")
def big_matrix(gpu):
    """CSR arrays built with numpy and uploaded once: every row one term with coefficient one at a random column (publics and
    witnesses alike); every 4096th row and the last three rows carry three terms with random coefficients."""
    F, cid = H.FR["bn254"], H.CURVE_IDS["bn254"]
    rs = np.random.RandomState(9700)
    r = H.rng(9700)
    special = sorted(set(range(0, _ROWS, 4096)) | {_ROWS - 3, _ROWS - 2, _ROWS - 1})
    counts = np.ones(_ROWS, dtype=np.uint64)
    counts[special] = 3
    row_ptr = np.zeros(_ROWS + 1, dtype=np.uint64)
    np.cumsum(counts, out=row_ptr[1:])
    nnz = int(row_ptr[-1])
    col = rs.randint(0, _NPUB + _NWIT, size=nnz).astype(np.uint32)
    col[row_ptr[:-1][::7].astype(np.int64)] = rs.randint(0, _NPUB, size=len(row_ptr[:-1][::7])).astype(np.uint32)   # publics are 5 columns in 1024: every 7th row reads one
    coeffs = np.tile(H.pack(F, [1]), (nnz, 1))
    rows = {}
    for i in special:
        lo = int(row_ptr[i])
        cs = H.rand_elems(F, 3, r)
        coeffs[lo:lo + 3] = H.pack(F, cs).reshape(3, 4)
        rows[i] = [(c, int(col[lo + j])) for j, c in enumerate(cs)]
    h = C.c_void_p()
    gpu.bindings._check(gpu.lib().csh_matrix_upload(cid, _ptr(row_ptr), _ptr(col), _ptr(coeffs), C.c_size_t(_ROWS), C.c_size_t(nnz), C.byref(h)))
    M = object.__new__(gpu.bindings.Matrix)   # the handle without Matrix.__init__, which packs row by row
    M.curve, M.n_rows, M.h = cid, _ROWS, h
    first = col[row_ptr[:-1].astype(np.int64)]   # the column of every row's first term
    pub = [1] + H.rand_elems(F, _NPUB - 1, r)
    wit_limbs = H.uniform_limbs(F, rs, 2 * _NWIT).reshape(_NWIT, 2, 4)   # Rep3 shares; component a doubles as the plain witness
    yield F, M, first, rows, pub, wit_limbs
    M.free()


@pytest.mark.parametrize("protocol,party", [(0, 0), (1, 0), (1, 1), (1, 2)])
def test_row_kernel_beyond_2p20_rows(gpu, big_matrix, protocol, party):
    """k_eval_rows with n_rows = 2^20 + 300 and n_out = 2^20 + 513: its grid is capped at 4096 blocks (2^20 lanes), so the loop's second
    pass holds real rows and the zero tail. One-term rows with coefficient one are a gather (a public column on Rep3 lands in component a
    on party 0, in b on party 1, nowhere on party 2); the three-term rows come from the oracle's drivers. The whole output is compared."""
    F, M, first, rows, pub, wit_limbs = big_matrix
    ppub = H.pack(F, pub).reshape(_NPUB, 4)
    zeros = np.zeros((_NPUB, 4), dtype=np.uint64)
    if protocol == 0:
        wit = np.ascontiguousarray(wit_limbs[:, 0, :])
        table = np.concatenate([ppub, wit])
        want = np.zeros((_ROWS_OUT, 4), dtype=np.uint64)
        want[:_ROWS] = table[first]
        drv, w_int = og.PlainDriver(F), H.unpack(F, wit)
        for i, row in rows.items():
            want[i] = H.pack(F, [drv.eval_row(row, pub, w_int)]).reshape(4)
    else:
        wit = wit_limbs
        ta = np.concatenate([ppub if party == 0 else zeros, wit[:, 0, :]])
        tb = np.concatenate([ppub if party == 1 else zeros, wit[:, 1, :]])
        want = np.zeros((_ROWS_OUT, 2, 4), dtype=np.uint64)
        want[:_ROWS, 0], want[:_ROWS, 1] = ta[first], tb[first]
        drv, w_int = og.Rep3Driver(F, party), H.unpack_shares(F, wit)
        for i, row in rows.items():
            want[i] = H.pack(F, list(drv.eval_row(row, pub, w_int))).reshape(2, 4)
    got = M.evaluate(protocol, party, ppub, wit, _ROWS_OUT).reshape(want.shape)
    H.assert_canonical(F, got)
    bad = np.nonzero((got != want).reshape(_ROWS_OUT, -1).any(axis=1))[0]
    assert bad.size == 0, (bad.size, int(bad[0]))


# ---- D5: bit reversal --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logn,ncomp", [(21, 1), (21, 2), (5, 2), (12, 2)])
def test_bit_reverse_two_grid_passes_and_two_components(gpu, logn, ncomp):
    """csh_bit_reverse on random 64-bit words against a numpy index permutation: 2^21 entries make the 4096-block grid pass twice;
    ncomp = 2 is what csh_fft / csh_ifft run on share vectors."""
    n = 1 << logn
    rs = np.random.RandomState(9800 + logn + ncomp)
    data = rs.randint(0, 2**64, size=(n, 4 * ncomp), dtype=np.uint64)
    i = np.arange(n, dtype=np.uint64)
    rev = np.zeros(n, dtype=np.uint64)
    for _ in range(logn):
        rev = (rev << np.uint64(1)) | (i & np.uint64(1))
        i >>= np.uint64(1)
    got = gpu.bindings.bit_reverse(H.CURVE_IDS["bn254"], data, logn, ncomp=ncomp).reshape(n, 4 * ncomp)
    assert np.array_equal(got, data[rev.astype(np.int64)])


# ---- D6: natural-order transforms --------------------------------------------------------------------------------------------------
def _oracle_fft(cid, x, logn, pg, ncomp):
    """natural coefficients -> natural evaluations: the bit reversal, then the decimation-in-time transform of oracle/c"""
    return cbridge.ntt(cid, cbridge.bit_reverse(x, logn, ncomp), logn, pg, ncomp=ncomp, dif=False)


def _oracle_ifft(cid, x, logn, pg, ncomp):
    return cbridge.bit_reverse(cbridge.ntt(cid, x, logn, pg, ncomp=ncomp, dif=True), logn, ncomp)


@functools.lru_cache(maxsize=None)
def _composition_is_the_python_oracle(curve):
    """the composition above == oracle.ntt.Domain.fft / .ifft at 2^10"""
    F, cid = H.FR[curve], H.CURVE_IDS[curve]
    logn = 10
    gen = ntt.roots_of_unity(F)[1][logn]
    do, pg = ntt.Domain(F, 1 << logn, gen), H.pack(F, [gen])
    v = H.rand_elems(F, 1 << logn, H.rng(9900))
    pv = H.pack(F, v)
    assert H.unpack(F, _oracle_fft(cid, pv, logn, pg, 1)) == do.fft(v)
    assert H.unpack(F, _oracle_ifft(cid, pv, logn, pg, 1)) == do.ifft(v)
    return True


@pytest.mark.parametrize("curve,logn,ncomp", [("bn254", 14, 1), ("bn254", 14, 2), ("bn254", 17, 1), ("bn254", 17, 2), ("bls12_377", 14, 1)])
def test_natural_order_transforms_match_the_oracle(gpu, curve, logn, ncomp):
    """csh_fft / csh_ifft (natural order in and out: the PLONK / Honk driver path) at 2^14 and 2^17 on uniform field elements and on the
    structured vectors (all zeros, all p - 1, alternating, a constant), against oracle/c's transform composed with its bit reversal; the
    composition is first checked against the Python oracle's Domain.fft / .ifft at 2^10."""
    assert _composition_is_the_python_oracle(curve)
    F, cid = H.FR[curve], H.CURVE_IDS[curve]
    n = 1 << logn
    pg = H.pack(F, [ntt.roots_of_unity(F)[1][logn]])
    dom = gpu.Domain(cid, logn, pg)
    inputs = dict(_structured(F, n * ncomp), uniform=H.uniform_limbs(F, np.random.RandomState(9900 + logn + ncomp), n * ncomp))
    for key, x in inputs.items():
        for name, got, want in (("fft", dom.fft(x, ncomp=ncomp), _oracle_fft(cid, x, logn, pg, ncomp)),
                                ("ifft", dom.ifft(x, ncomp=ncomp), _oracle_ifft(cid, x, logn, pg, ncomp))):
            got, want = np.asarray(got).reshape(-1, 4), np.asarray(want).reshape(-1, 4)
            H.assert_canonical(F, got)
            bad = np.nonzero((got != want).any(axis=1))[0]
            assert bad.size == 0, (name, key, bad.size, int(bad[0]))
    dom.free()


# ---- D7: coset table ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
@pytest.mark.parametrize("shift", ["groth16", "one", "p-1", "full-width"])
def test_coset_table_at_2p17(gpu, curve, shift):
    """csh_coset_table (k_powers, bit-reversed) at 2^17 against ntt.bit_reversed_coset_table: the Groth16 coset shift, 1 (all ones), p - 1
    (alternating 1 / p - 1) and a seeded full-width shift."""
    F, cid = H.FR[curve], H.CURVE_IDS[curve]
    logn = 17
    s = {"groth16": ntt.groth16_roots_of_unity(F, logn)[1], "one": 1, "p-1": F.p - 1, "full-width": H.rng(10000).randrange(F.p >> 1, F.p)}[shift]
    dom = gpu.Domain(cid, logn, H.pack(F, [ntt.roots_of_unity(F)[1][logn]]))
    got = dom.coset_table(H.pack(F, [s]))
    dom.free()
    H.assert_canonical(F, got)
    want = H.pack(F, ntt.bit_reversed_coset_table(F, s, 1 << logn))
    bad = np.nonzero((got.reshape(-1, 4) != want.reshape(-1, 4)).any(axis=1))[0]
    assert bad.size == 0, (bad.size, int(bad[0]))
