"""Device tests of the round-2 / round-5 entries (csrc/plonk_rounds.hip): csh_plonk_z_operands_dev, csh_vec_rotate_right_dev,
csh_plonk_blind_coefficients_dev and csh_poly_lincomb_dev against tests/plonk_rounds_ref.py, and the closed chain on the reference's
multiplier2 circuit through device entry points only. Every comparison is exact and covers every element."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import helpers as H
from tests import plonk_rounds_ref as R

pytestmark = pytest.mark.gpu
CURVES = ["bn254", "bls12_381", "bls12_377"]
PARTIES = [(0, 0), (1, 0), (1, 1), (1, 2)]   # (protocol, party)
GUARD = np.uint64(0x5A5AC3C3A5A53C3C)
INVALID = -1
sz, u32 = C.c_size_t, C.c_uint32


def _vec(F, v):
    return H.pack(F, R.flat(v))


def _up(hip, arr):
    return hip.DeviceBuffer.from_host(arr)


def _out(hip, ncomp, count, guard=8):
    """an output buffer of `count` shares filled with the guard word, `guard` words of it behind"""
    return _up(hip, np.full(4 * ncomp * count + guard, GUARD, dtype=np.uint64))


def _down(F, T, buf, count, guard=8):
    """-> the shares, after checking that the words behind them still hold the guard (nothing written past the end)"""
    raw = buf.to_host()
    assert raw.size == 4 * T.ncomp * count + guard and (raw[4 * T.ncomp * count:] == GUARD).all(), "written past the end of an output"
    v = H.unpack(F, raw[:4 * T.ncomp * count])   # strict: canonical
    return [tuple(v[i * T.ncomp:(i + 1) * T.ncomp]) for i in range(count)]


def first_difference(got, want):
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            return i
    return None


def same(got, want, what):
    assert len(got) == len(want) and got == want, (what, "first difference at share", first_difference(got, want), "of", len(want))


def domain_for(hip, curve, n):
    F = H.FR[curve]
    return hip.Domain(H.CURVE_IDS[curve], (4 * n).bit_length() - 1, H.pack(F, [R.ext_generator(F, n)]))


def dev_z_operands(hip, curve, T, dom, n, c):
    F = H.FR[curve]
    outs = [_out(hip, T.ncomp, n) for _ in range(6)]
    hip.plonk_z_operands(dom, T.protocol, T.party, [_up(hip, _vec(F, c[k])) for k in "abc"], [_up(hip, H.pack(F, s)) for s in c["sigma"]],
                         H.pack(F, c["ch"]), outs)
    hip.bindings.sync()
    return [_down(F, T, o, n) for o in outs]


def dev_rotate(hip, curve, T, v, k):
    F = H.FR[curve]
    out = _out(hip, T.ncomp, len(v))
    hip.vec_rotate_right(H.CURVE_IDS[curve], _up(hip, _vec(F, v)), out, len(v), T.ncomp, k)
    hip.bindings.sync()
    return _down(F, T, out, len(v))


def dev_blind(hip, curve, T, poly, coeff_rev):
    F = H.FR[curve]
    k = len(coeff_rev)
    buf = _up(hip, np.concatenate([_vec(F, poly), np.full(4 * T.ncomp * k + 8, GUARD, dtype=np.uint64)]))
    hip.plonk_blind_coefficients(H.CURVE_IDS[curve], buf, len(poly), _vec(F, coeff_rev), T.ncomp)
    hip.bindings.sync()
    return _down(F, T, buf, len(poly) + k)


def dev_lincomb(hip, curve, T, shares, cs, publics, cp, const0, out_len):
    F = H.FR[curve]
    out = _out(hip, T.ncomp, out_len)
    up = lambda a: _up(hip, a) if a.size else None
    hip.poly_lincomb(H.CURVE_IDS[curve], T.protocol, T.party, [up(_vec(F, s)) for s in shares], [len(s) for s in shares], H.pack(F, cs),
                     [up(H.pack(F, v)) for v in publics], [len(v) for v in publics], H.pack(F, cp), out, out_len,
                     const0=H.pack(F, [const0]) if const0 is not None else None)
    hip.bindings.sync()
    return _down(F, T, out, out_len)


def check_entries(hip, curve, T, c):
    n = c["n"]
    dom = domain_for(hip, curve, n)
    for name, g, w in zip(("n1", "n2", "n3", "d1", "d2", "d3"), dev_z_operands(hip, curve, T, dom, n, c), c["want_z"]):
        same(g, w, name)
    for k in (1, n - 1):
        same(dev_rotate(hip, curve, T, c["a"], k), R.rotate_right(c["a"], k), ("rotate", k))
    for cr, want in zip(c["blind"], c["want_blind"]):
        same(dev_blind(hip, curve, T, c["a"], cr), want, ("blind", len(cr)))
    same(dev_lincomb(hip, curve, T, c["shares"], c["cs"], c["publics"], c["cp"], c["const0"], n + 6), c["want_lc"], "lincomb")


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("protocol,party", PARTIES)
def test_every_entry_at_the_smallest_domain(gpu, curve, protocol, party):
    """n = 8, N = 32: the smallest domain the round-3 calls accept; one ragged workgroup"""
    F, T = H.FR[curve], R.Ops(H.FR[curve].p, protocol, party)
    r = H.rng(6000 + 10 * protocol + party)
    check_entries(gpu, curve, T, R.entries_case(F.p, T, 8, lambda: r.randrange(F.p), pow(R.ext_generator(F, 8), 4, F.p)))


@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
@pytest.mark.parametrize("protocol,party", PARTIES)
def test_edges_of_the_field(gpu, curve, protocol, party):
    F, T = H.FR[curve], R.Ops(H.FR[curve].p, protocol, party)
    for v in (F.p - 1, 0):
        check_entries(gpu, curve, T, R.entries_case(F.p, T, 8, lambda: v, pow(R.ext_generator(F, 8), 4, F.p)))


@functools.lru_cache(maxsize=None)
def large_case(curve, protocol, party, log_n):
    F, T = H.FR[curve], R.Ops(H.FR[curve].p, protocol, party)
    r = H.rng(7000 + log_n)
    n = 1 << log_n
    return T, R.entries_case(F.p, T, n, lambda: r.randrange(F.p), pow(R.ext_generator(F, n), 4, F.p))


@pytest.mark.parametrize("curve,protocol,party", [("bn254", 1, 1), ("bls12_381", 0, 0), ("bls12_377", 1, 0)])
def test_z_operands_use_the_high_level_of_the_power_table(gpu, curve, protocol, party):
    """n = 2^10: points 256 .. 1023 take entries 1 .. 3 of the table's high level"""
    T, c = large_case(curve, protocol, party, 10)
    for name, g, w in zip(("n1", "n2", "n3", "d1", "d2", "d3"), dev_z_operands(gpu, curve, T, domain_for(gpu, curve, c["n"]), c["n"], c), c["want_z"]):
        same(g, w, name)


@pytest.mark.parametrize("curve,protocol,party", [("bn254", 1, 0), ("bls12_381", 1, 1)])
def test_capped_grids(gpu, curve, protocol, party):
    """n = 2^12 with one and three workgroups: every lane's grid-stride loop takes many passes with a ragged last one"""
    T, c = large_case(curve, protocol, party, 12)
    n = c["n"]
    dom = domain_for(gpu, curve, n)
    for mb in (1, 3):
        with gpu.tuned(vec_max_blocks=mb):
            for name, g, w in zip(("n1", "n2", "n3", "d1", "d2", "d3"), dev_z_operands(gpu, curve, T, dom, n, c), c["want_z"]):
                same(g, w, (name, mb))
            same(dev_lincomb(gpu, curve, T, c["shares"], c["cs"], c["publics"], c["cp"], c["const0"], n + 6), c["want_lc"], ("lincomb", mb))
            same(dev_rotate(gpu, curve, T, c["a"], 1), R.rotate_right(c["a"], 1), ("rotate", mb))


@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
@pytest.mark.parametrize("protocol,party", [(0, 0), (1, 1), (1, 2)])
@pytest.mark.parametrize("with_const", [False, True])
def test_lincomb_ragged_lengths_across_a_launch_boundary(gpu, curve, protocol, party, with_const):
    """lengths n + 1, n + 2, n + 3, n + 6 and 0; 9 share and 8 public vectors: 17 terms, the last one alone in a second launch"""
    F, T = H.FR[curve], R.Ops(H.FR[curve].p, protocol, party)
    p, n = F.p, 8
    r = H.rng(810 + 10 * protocol + party)
    vec = lambda k: [tuple(r.randrange(p) for _ in range(T.ncomp)) for _ in range(k)]
    pub = lambda k: [r.randrange(p) for _ in range(k)]
    lens_s, lens_p = [n + 1, n + 2, n + 3, n + 6, 0, n, n + 1, 3, n + 6], [n, 0, n + 6, n + 1, n + 2, n + 3, 1, n]
    shares, publics = [vec(k) for k in lens_s], [pub(k) for k in lens_p]
    cs, cp = pub(9), pub(7) + [1]
    const0 = r.randrange(p) if with_const else None
    for out_len in (n + 6, n + 9):
        same(dev_lincomb(gpu, curve, T, shares, cs, publics, cp, const0, out_len), R.poly_lincomb(T, shares, cs, publics, cp, const0, out_len), out_len)


@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
def test_rep3_parties_add_up_to_the_plain_result(gpu, curve):
    """Rep3 party k holds {x_k, x_(k-1)}: the a-components of the three parties' outputs sum to the plain output on the summed inputs --
    which fails when a public value lands on the wrong party or component, or on more than one."""
    F = H.FR[curve]
    p, n = F.p, 8
    r = H.rng(56)
    w = pow(R.ext_generator(F, n), 4, p)
    plain_T = R.Ops(p, 0, 0)
    plain = R.entries_case(p, plain_T, n, lambda: r.randrange(p), w)

    def split(x):
        a0, a1 = r.randrange(p), r.randrange(p)
        a = [a0, a1, (x - a0 - a1) % p]
        return [(a[k], a[k - 1]) for k in range(3)]

    def split_vec(v):
        parts = [split(s[0]) for s in v]
        return [[q[k] for q in parts] for k in range(3)]

    cases = [dict(plain) for _ in range(3)]
    for name in "abc":
        for k, sv in enumerate(split_vec(plain[name])):
            cases[k][name] = sv
    per_share = [split_vec(s) for s in plain["shares"]]
    for k in range(3):
        cases[k]["shares"] = [ps[k] for ps in per_share]
    dom = domain_for(gpu, curve, n)
    want_z = dev_z_operands(gpu, curve, plain_T, dom, n, plain)
    want_lc = dev_lincomb(gpu, curve, plain_T, plain["shares"], plain["cs"], plain["publics"], plain["cp"], plain["const0"], n + 6)
    assert want_z == plain["want_z"] and want_lc == plain["want_lc"]
    Ts = [R.Ops(p, 1, k) for k in range(3)]
    got_z = [dev_z_operands(gpu, curve, Ts[k], dom, n, cases[k]) for k in range(3)]
    got_lc = [dev_lincomb(gpu, curve, Ts[k], cases[k]["shares"], plain["cs"], plain["publics"], plain["cp"], plain["const0"], n + 6) for k in range(3)]
    vectors = [([g[v] for g in got_z], want_z[v]) for v in range(6)] + [(got_lc, want_lc)]
    for j, (got, want) in enumerate(vectors):
        summed = [((got[0][i][0] + got[1][i][0] + got[2][i][0]) % p,) for i in range(len(want))]
        same(summed, want, j)
        for k in range(3):   # and the sharing stays replicated: party k's b is party k-1's a
            assert [s[1] for s in got[k]] == [s[0] for s in got[k - 1]], (j, k)


@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
@pytest.mark.parametrize("ncomp", [1, 2])
@pytest.mark.parametrize("n", [8, 1000, 1 << 12])
def test_rotate(gpu, curve, ncomp, n):
    F, T = H.FR[curve], R.Ops(H.FR[curve].p, ncomp - 1, 0)
    r = H.rng(n + ncomp)
    v = [tuple(r.randrange(F.p) for _ in range(ncomp)) for _ in range(n)]
    for k in (1, n - 1):
        same(dev_rotate(gpu, curve, T, v, k), R.rotate_right(v, k), k)


@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
@pytest.mark.parametrize("ncomp", [1, 2])
@pytest.mark.parametrize("k", [2, 3])
def test_blind_writes_k_coefficients_and_nothing_else(gpu, curve, ncomp, k):
    F, T = H.FR[curve], R.Ops(H.FR[curve].p, ncomp - 1, 0)
    r = H.rng(40 + k + ncomp)
    sh = lambda: tuple(r.randrange(F.p) for _ in range(ncomp))
    poly, cr = [sh() for _ in range(8)], [sh() for _ in range(k)]
    got = dev_blind(gpu, curve, T, poly, cr)      # checks the guard words behind the n + k shares
    same(got, R.blind_coefficients(T, poly, cr), k)
    assert got[k:8] == poly[k:]


def test_refusals_with_device_pointers(gpu):
    """the rules that need a device: the size of the domain, and every overlap rule, with the buffers untouched afterwards"""
    F = H.FR["bn254"]
    L = gpu.lib()
    n, N = 8, 32
    dom = domain_for(gpu, "bn254", 8)
    small = domain_for(gpu, "bn254", 4)
    fill = np.arange(4 * 2 * N * 16, dtype=np.uint64)
    pool = gpu.DeviceBuffer.from_host(fill)
    base = pool.ptr.value
    vb = 32 * 2 * n                      # bytes of a Rep3 share vector of n shares
    slot = lambda k: base + k * 4 * vb   # slots of 4 n Rep3 shares: room for a public vector of 4 n elements, too
    arr = lambda addrs: (C.c_void_p * len(addrs))(*addrs)
    host = np.ones(4 * 2 * 16, dtype=np.uint64)
    hp = host.ctypes.data_as(C.c_void_p)
    err = lambda: L.csh_last_error()
    sh3, sg3, out6 = [slot(k) for k in range(3)], [slot(3 + k) for k in range(3)], [slot(6 + k) for k in range(6)]

    def zop(d, sh, sg, outs):
        return L.csh_plonk_z_operands_dev(d.h, u32(1), u32(0), arr(sh), arr(sg), hp, arr(outs), None)

    def rot(i, o, k=1):
        return L.csh_vec_rotate_right_dev(0, C.c_void_p(i), C.c_void_p(o), sz(n), u32(2), sz(k), None)

    def lc(sh, sl, pb, pl, out, out_len):
        return L.csh_poly_lincomb_dev(0, u32(1), u32(0), arr(sh), (sz * len(sl))(*sl), hp, sz(len(sh)), arr(pb), (sz * len(pl))(*pl), hp, sz(len(pb)),
                                      hp, C.c_void_p(out), sz(out_len), None)

    assert zop(small, sh3, sg3, out6) == INVALID and b"32" in err(), err()
    swap = lambda lst, k, v: lst[:k] + [v] + lst[k + 1:]
    for call, msg in ((lambda: zop(dom, sh3, sg3, swap(out6, 0, slot(0))), b"overlaps an input"),                   # n1 in place of a
                      (lambda: zop(dom, sh3, sg3, swap(out6, 3, slot(1) + vb - 32)), b"overlaps an input"),         # d1 begins in b's last share
                      (lambda: zop(dom, sh3, sg3, swap(out6, 5, slot(5) + 32 * N - 32)), b"overlaps an input"),     # d3 begins in S3's last element
                      (lambda: zop(dom, sh3, sg3, swap(out6, 4, slot(6))), b"two outputs overlap"),
                      (lambda: zop(dom, sh3, sg3, swap(out6, 2, slot(7) + vb - 32)), b"two outputs overlap"),
                      (lambda: rot(slot(0), slot(0)), b"overlaps an input"),
                      (lambda: rot(slot(0), slot(0) + vb - 32), b"overlaps an input"),
                      (lambda: lc([slot(0), slot(1)], [n + 6, n], [slot(3)], [n], slot(1) + vb - 64, n + 6), b"overlaps an input"),
                      (lambda: lc([slot(0), slot(1)], [n + 6, n], [slot(3)], [n], slot(3) + 32 * n - 32, n + 6), b"overlaps an input")):
        rc = call()   # one at a time: the message read below is this call's
        assert rc == INVALID and msg in err(), (msg, err())
    gpu.bindings.sync()
    assert (pool.to_host() == fill).all(), "a refused call wrote to its buffers"
    # next to each other is no overlap; a zero-length vector's pointer is not compared
    assert zop(dom, sh3, sg3, out6) == 0 and rot(slot(0), slot(0) + vb) == 0
    assert lc([slot(0), slot(12)], [n, 0], [slot(3)], [n], slot(12), n + 6) == 0
    gpu.bindings.sync()


# ---- the closed chain on the reference's circuit ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
def test_closed_chain_on_multiplier2(gpu, curve):
    """Rounds 1-5 of the plain prover on tests/golden/Plonk/<curve>/multiplier2 with fixed challenges, between the wire buffers and the two
    opening quotients through device entry points only: the new calls, the transforms, the scans, csh_eval_poly_dev, and the mirror's
    compute_t for round 3. buffer_z[0] = 1 after the rotation, both opening divisions leave remainder 0, and both quotients are the
    restatement's bit for bit."""
    from cosnarks_amd import groth16 as dev
    hip, F, cid = gpu, H.FR[curve], H.CURVE_IDS[curve]
    o = R.fixture_chain(curve)
    zk, p = o["zk"], F.p
    n = zk.domain_size
    L = hip.lib()
    T = R.Ops(p, 0, 0)
    one = H.pack(F, [1])
    dom_n = hip.Domain(cid, n.bit_length() - 1, H.pack(F, [pow(R.ext_generator(F, n), 4, p)]))
    dom_4n = domain_for(hip, curve, n)
    el = lambda x: H.pack(F, [x])

    def padded_copy(src, length, out_len):
        """a device copy of `length` elements into a fresh buffer of out_len, zeros behind: a linear combination of one vector"""
        return hip.poly_lincomb(cid, 0, 0, [src], [length], one, [], [], np.zeros(0, dtype=np.uint64), hip.DeviceBuffer(32 * out_len), out_len)

    def mul(x, y):
        out = hip.DeviceBuffer(32 * n)
        assert L.csh_vec_mul_dev(cid, x.ptr, y.ptr, out.ptr, sz(n), None) == 0
        return out

    def poly_and_eval(buffer_dev, blinders):
        k = len(blinders)
        poly = padded_copy(buffer_dev, n, n + k)
        dom_n.ifft_dev(poly)                                   # the first n elements
        ev = padded_copy(poly, n, 4 * n)
        dom_4n.fft_dev(ev)
        hip.plonk_blind_coefficients(cid, poly, n, H.pack(F, blinders))
        return poly, ev

    # round 1: the wire buffers are the chain's input (witness additions and the map gather are host work)
    bufs = [_up(hip, H.pack(F, v)) for v in R.wire_buffers(p, zk, o["additions"], o["maps"], o["witness"])]
    b = o["b"]
    poly, ev = {}, {}
    for name, buf, j in zip("abc", bufs, (0, 2, 4)):
        poly[name], ev[name] = poly_and_eval(buf, b[j:j + 2])
    # round 2
    sigma = [_up(hip, H.pack(F, zk.polys[k][1])) for k in ("S1", "S2", "S3")]
    ops = hip.plonk_z_operands(dom_4n, 0, 0, bufs, sigma, H.pack(F, [o["beta"], o["gamma"], zk.k1, zk.k2]), [hip.DeviceBuffer(32 * n) for _ in range(6)])
    num = hip.vec_prefix_prod(cid, mul(mul(ops[0], ops[1]), ops[2]), n)
    den, _ = hip.vec_batch_inverse(cid, hip.vec_prefix_prod(cid, mul(mul(ops[3], ops[4]), ops[5]), n), n)
    buffer_z = hip.vec_rotate_right(cid, mul(num, den), hip.DeviceBuffer(32 * n), n, 1, 1)
    poly["z"], ev["z"] = poly_and_eval(buffer_z, b[6:9])
    hip.bindings.sync()
    bz = H.unpack(F, buffer_z.to_host())
    assert bz[0] == 1 and bz == o["buffer_z"]
    # round 3: the mirror's compute_t (host vectors in and out)
    evals = [ev[k].to_host() for k in "abcz"] + [H.pack(F, zk.polys[k][1]) for k in ("Qm", "Ql", "Qr", "Qo", "Qc", "S1", "S2", "S3")]
    evals += [H.pack(F, l[1]) for l in zk.lagrange]
    buffer_a = bufs[0].to_host()[:4 * len(zk.lagrange)]
    scalars = np.concatenate([buffer_a, H.pack(F, b + [o["beta"], o["gamma"], o["alpha"], zk.k1, zk.k2])])
    for name, t in zip(("t1", "t2", "t3"), dev.plonk_compute_t(cid, n, evals, scalars)):
        poly[name] = _up(hip, t.reshape(-1))
    lens = {"a": n + 2, "b": n + 2, "c": n + 2, "z": n + 3, "t1": n + 1, "t2": n + 1, "t3": n + 6}
    for k, ln in lens.items():
        assert H.unpack(F, poly[k].to_host()[:4 * ln]) == o["poly"][k], k
    # round 4: the six evaluations (opened values: they come to the host)
    xi, xiw = o["xi"], o["xi"] * pow(R.ext_generator(F, n), 4, p) % p
    s1c, s2c = (_up(hip, H.pack(F, zk.polys[k][0])) for k in ("S1", "S2"))
    at = lambda buf, ln, x: H.unpack(F, hip.eval_poly(cid, buf, el(x), 1, ln).to_host())[0]
    e = {"a": at(poly["a"], n + 2, xi), "b": at(poly["b"], n + 2, xi), "c": at(poly["c"], n + 2, xi), "s1": at(s1c, n, xi), "s2": at(s2c, n, xi),
         "zw": at(poly["z"], n + 3, xiw)}
    assert e == o["evals"]
    # round 5: scalars on the host, one linear combination, two divisions
    cs, cp, const0 = R.round5_coefficients(p, n, pow(R.ext_generator(F, n), 4, p), list(o["witness"][1:zk.n_public + 1]), e, o["beta"], o["gamma"],
                                           o["alpha"], xi, o["v"], zk.k1, zk.k2)
    names = ("z", "t1", "t2", "t3", "a", "b", "c")
    publics = [_up(hip, H.pack(F, zk.polys[k][0])) for k in ("Qm", "Ql", "Qr", "Qo", "Qc", "S3")] + [s1c, s2c]
    numer = hip.poly_lincomb(cid, 0, 0, [poly[k] for k in names], [lens[k] for k in names], H.pack(F, cs), publics, [n] * 8, H.pack(F, cp),
                             hip.DeviceBuffer(32 * (n + 6)), n + 6, const0=el(const0))
    wxi, rem_xi = hip.poly_div_linear(cid, numer, el(xi), 1, n=n + 6, out=_out(hip, 1, n + 5), rem=hip.DeviceBuffer(32))
    wxiw, rem_xiw = hip.poly_div_linear(cid, poly["z"], el(xiw), 1, sub0=el(e["zw"]), n=n + 3, out=_out(hip, 1, n + 2), rem=hip.DeviceBuffer(32))
    hip.bindings.sync()
    assert H.unpack(F, rem_xi.to_host()) == [0] and H.unpack(F, rem_xiw.to_host()) == [0]
    same(_down(F, T, wxi, n + 5), [(x,) for x in o["wxi"]], "W_xi")
    same(_down(F, T, wxiw, n + 2), [(x,) for x in o["wxiw"]], "W_xiw")
