"""CPU tests of the round-2 / round-5 entries (csrc/plonk_rounds.hip: csh_plonk_z_operands_dev, csh_vec_rotate_right_dev,
csh_plonk_blind_coefficients_dev, csh_poly_lincomb_dev): the C boundary without a device, and the arithmetic itself run on the host through
csh_selftest_plonk_rounds_host -- the argument builders and the per-index functions the gfx950 kernels call, with the limb-bound contract
checks of selftest.hip on (a violated bound aborts the process). Truth is tests/plonk_rounds_ref.py. Every comparison is exact."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import helpers as H
from tests import plonk_rounds_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVES = ["bn254", "bls12_381", "bls12_377"]
PARTIES = [(0, 0), (1, 0), (1, 1), (1, 2)]   # (protocol, party)
NO_DEVICE, INVALID = -2, -1
ENTRY = {"csh_plonk_z_operands_dev": ["round2.rs:116-155"], "csh_vec_rotate_right_dev": ["round2.rs:171"],
         "csh_plonk_blind_coefficients_dev": ["co-plonk/src/lib.rs:162-177"], "csh_poly_lincomb_dev": ["round5.rs:118-259"]}
sz, u32 = C.c_size_t, C.c_uint32
FILL = np.uint64(0xA5A5A5A5A5A5A5A5)


def _p(x):
    return x.ctypes.data_as(C.c_void_p) if x is not None else None


def _ptrs(arrs):
    return (C.c_void_p * len(arrs))(*[a.ctypes.data if a is not None else None for a in arrs]) if len(arrs) else None


def _vec(F, v):
    return H.pack(F, R.flat(v))


def _shares(F, T, arr):
    v = H.unpack(F, arr)   # strict: canonical
    return [tuple(v[i * T.ncomp:(i + 1) * T.ncomp]) for i in range(len(v) // T.ncomp)]


def _host(hip, curve, entry, T, n, ins, outs, aux=None, lens=None, scalars=None, ks=0, kp=0):
    F = H.FR[curve]
    ln = (sz * len(lens))(*lens) if lens else None
    return hip.lib().csh_selftest_plonk_rounds_host(H.CURVE_IDS[curve], entry, _p(H.pack(F, [aux])) if aux is not None else None, sz(n),
                                                    u32(T.protocol), u32(T.party), _ptrs(ins), ln, _p(H.pack(F, scalars)) if scalars else None,
                                                    sz(ks), sz(kp), _ptrs(outs))


def host_z_operands(hip, curve, T, n, a, b, c, sigma, ch):
    F = H.FR[curve]
    outs = [np.full(4 * T.ncomp * n, FILL, dtype=np.uint64) for _ in range(6)]
    ins = [_vec(F, a), _vec(F, b), _vec(F, c)] + [H.pack(F, s) for s in sigma]
    assert _host(hip, curve, 0, T, n, ins, outs, aux=R.ext_generator(F, n), scalars=list(ch)) == 0
    return [_shares(F, T, o) for o in outs]


def host_rotate(hip, curve, T, v, k):
    F = H.FR[curve]
    out = np.full(4 * T.ncomp * len(v), FILL, dtype=np.uint64)
    assert _host(hip, curve, 1, T, len(v), [_vec(F, v)], [out], ks=k) == 0
    return _shares(F, T, out)


def host_blind(hip, curve, T, poly, coeff_rev):
    F = H.FR[curve]
    k = len(coeff_rev)
    buf = np.concatenate([_vec(F, poly), H.pack(F, [0] * (k * T.ncomp))])
    assert _host(hip, curve, 2, T, len(poly), [], [buf], scalars=R.flat(coeff_rev), ks=k) == 0
    return _shares(F, T, buf)


def host_lincomb(hip, curve, T, shares, cs, publics, cp, const0, out_len):
    F = H.FR[curve]
    out = np.full(4 * T.ncomp * out_len, FILL, dtype=np.uint64)
    ins = [_vec(F, s) if s else None for s in shares] + [H.pack(F, v) if v else None for v in publics]
    lens = [len(s) for s in shares] + [len(v) for v in publics]
    assert _host(hip, curve, 3, T, out_len, ins, [out], aux=const0, lens=lens, scalars=list(cs) + list(cp), ks=len(shares), kp=len(publics)) == 0
    return _shares(F, T, out)


def check_entries_on_host(hip, curve, T, c):
    assert host_z_operands(hip, curve, T, c["n"], c["a"], c["b"], c["c"], c["sigma"], c["ch"]) == c["want_z"]
    for k in (0, 1, c["n"] - 1):
        assert host_rotate(hip, curve, T, c["a"], k) == R.rotate_right(c["a"], k), k
    assert host_rotate(hip, curve, T, c["shares"][3][:11], 4) == R.rotate_right(c["shares"][3][:11], 4)   # n no power of two
    for cr, want in zip(c["blind"], c["want_blind"]):
        assert host_blind(hip, curve, T, c["a"], cr) == want, len(cr)
    assert host_lincomb(hip, curve, T, c["shares"], c["cs"], c["publics"], c["cp"], c["const0"], c["n"] + 6) == c["want_lc"]


def test_header_bindings_and_sys_crate_declare_the_entry_points(hip):
    from cosnarks_amd import bindings
    txt = open(bindings.header_path()).read()
    declared = bindings.declared_symbols()
    sys_rs = open(os.path.join(ROOT, "rust", "cosnarks-hip-sys", "src", "lib.rs")).read()
    L = hip.lib()
    for name, cites in ENTRY.items():
        assert name in declared and hasattr(L, name), name
        at = txt.index("int %s(" % name)
        comment = txt[txt.rindex("/*", 0, at):at]
        for c in cites:
            assert c in comment, (name, c)
        assert "pub fn %s(" % name in sys_rs
        assert hasattr(hip, name[4:-4]) and name in open(bindings.__file__).read()
    assert "csh_selftest_plonk_rounds_host" not in declared and hasattr(L, "csh_selftest_plonk_rounds_host")


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("protocol,party", PARTIES)
def test_entries_match_the_restatement(hip, curve, protocol, party):
    F, T = H.FR[curve], R.Ops(H.FR[curve].p, protocol, party)
    r = H.rng(2000 + 10 * protocol + party)
    w_ext = R.ext_generator(F, 8)
    check_entries_on_host(hip, curve, T, R.entries_case(F.p, T, 8, lambda: r.randrange(F.p), pow(w_ext, 4, F.p)))


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("protocol,party", PARTIES)
@pytest.mark.parametrize("fill", ["p-1", "0"])
def test_entries_at_the_edges_of_the_field(hip, curve, protocol, party, fill):
    """every operand p - 1 (shares, public vectors, challenges, coefficients, const0), and every operand 0; bound checks on"""
    F, T = H.FR[curve], R.Ops(H.FR[curve].p, protocol, party)
    v = F.p - 1 if fill == "p-1" else 0
    c = R.entries_case(F.p, T, 8, lambda: v, pow(R.ext_generator(F, 8), 4, F.p))
    check_entries_on_host(hip, curve, T, c)


@pytest.mark.parametrize("curve", CURVES)
def test_z_operands_cross_the_power_table(hip, curve):
    """n = 2^9: points 256 .. 511 take the second entry of the table's high level"""
    F, T = H.FR[curve], R.Ops(H.FR[curve].p, 1, 1)
    r = H.rng(9)
    n = 512
    c = R.entries_case(F.p, T, n, lambda: r.randrange(F.p), pow(R.ext_generator(F, n), 4, F.p))
    assert host_z_operands(hip, curve, T, n, c["a"], c["b"], c["c"], c["sigma"], c["ch"]) == c["want_z"]


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("protocol,party", PARTIES)
def test_lincomb_shapes(hip, curve, protocol, party):
    F, T = H.FR[curve], R.Ops(H.FR[curve].p, protocol, party)
    p = F.p
    r = H.rng(300 + 10 * protocol + party)
    sh = lambda: tuple(r.randrange(p) for _ in range(T.ncomp))
    vec = lambda k: [sh() for _ in range(k)]
    pub = lambda k: [r.randrange(p) for _ in range(k)]
    top = lambda k: [(p - 1,) * T.ncomp for _ in range(k)]
    shapes = [
        ("ks = 0", [], [], [pub(5), pub(9)], pub(2), None, 9),
        ("kp = 0", [vec(9), vec(4)], pub(2), [], [], r.randrange(p), 9),
        ("a zero-length vector of each kind", [vec(6), [], vec(3)], pub(3), [[], pub(6)], pub(2), None, 6),
        ("only zero-length vectors", [[]], pub(1), [[]], pub(1), r.randrange(p), 4),
        ("out_len beyond every input", [vec(3)], pub(1), [pub(2)], pub(1), r.randrange(p), 12),
        ("ks = 33: three launches", [vec(1 + j % 7) for j in range(33)], pub(33), [pub(7)], [1], None, 7),
        ("17 terms across a launch boundary, coefficients one", [vec(5) for _ in range(9)], [1] * 9, [pub(5) for _ in range(8)], [1] * 8, 1, 5),
        ("64 + 64 terms of (p - 1)(p - 1)", [top(3)] * 64, [p - 1] * 64, [[p - 1] * 3] * 64, [p - 1] * 64, p - 1, 3),
    ]
    for name, shares, cs, publics, cp, const0, out_len in shapes:
        got = host_lincomb(hip, curve, T, shares, cs, publics, cp, const0, out_len)
        assert got == R.poly_lincomb(T, shares, cs, publics, cp, const0, out_len), name


def test_refusals_come_before_the_device(hip):
    """Every rule of the three calls that take no domain, and the pointer, protocol and party rules of the one that does, answer
    CSH_ERR_INVALID on any machine; what is recorded is the status and the message."""
    L = hip.lib()
    err = lambda: L.csh_last_error()
    n = 8
    buf = lambda k: np.zeros(4 * 2 * k, dtype=np.uint64)
    host = np.ones(4 * 2 * 16, dtype=np.uint64)
    hp = _p(host)
    fake_dom = C.c_void_p(host.ctypes.data)   # never looked into: each call below is refused before that
    sh3, sg3, out6 = [buf(n) for _ in range(3)], [buf(4 * n) for _ in range(3)], [buf(n) for _ in range(6)]
    hole = lambda arrs, k: _ptrs(arrs[:k] + [None] + arrs[k + 1:])

    def zop(dom, pr, pa, sh, sg, ch, outs):
        return L.csh_plonk_z_operands_dev(dom, u32(pr), u32(pa), sh, sg, ch, outs, None)

    def rot(f, i, o, n_, nc, k):
        return L.csh_vec_rotate_right_dev(f, i, o, sz(n_), u32(nc), sz(k), None)

    def blind(f, poly, n_, nc, cr, k):
        return L.csh_plonk_blind_coefficients_dev(f, poly, sz(n_), u32(nc), cr, sz(k), None)

    def lc(f, pr, pa, sh, sl, cs, ks, pb, pl, cp, kp, c0, out, out_len):
        return L.csh_poly_lincomb_dev(f, u32(pr), u32(pa), sh, (sz * len(sl))(*sl) if sl is not None else None, cs, sz(ks), pb,
                                      (sz * len(pl))(*pl) if pl is not None else None, cp, sz(kp), c0, out, sz(out_len), None)

    s2, p2, out = [buf(n + 6), buf(n + 6)], [buf(n), buf(n)], buf(n + 6)
    good_lc = dict(f=0, pr=1, pa=0, sh=_ptrs(s2), sl=[n + 6, n + 2], cs=hp, ks=2, pb=_ptrs(p2), pl=[n, n], cp=hp, kp=2, c0=hp, out=_p(out), out_len=n + 6)
    lcw = lambda **kw: lc(**{**good_lc, **kw})
    # protocol and party
    for pr, pa in ((2, 0), (0, 3), (1, 3), (7, 7)):
        for rc in (zop(fake_dom, pr, pa, _ptrs(sh3), _ptrs(sg3), hp, _ptrs(out6)), lcw(pr=pr, pa=pa)):
            assert rc == INVALID and b"protocol" in err(), (rc, err())
    # NULL pointers, the arrays and their entries
    calls = [zop(None, 1, 0, _ptrs(sh3), _ptrs(sg3), hp, _ptrs(out6)), zop(fake_dom, 1, 0, None, _ptrs(sg3), hp, _ptrs(out6)),
             zop(fake_dom, 1, 0, _ptrs(sh3), None, hp, _ptrs(out6)), zop(fake_dom, 1, 0, _ptrs(sh3), _ptrs(sg3), None, _ptrs(out6)),
             zop(fake_dom, 1, 0, _ptrs(sh3), _ptrs(sg3), hp, None), zop(fake_dom, 1, 0, hole(sh3, 2), _ptrs(sg3), hp, _ptrs(out6)),
             zop(fake_dom, 1, 0, _ptrs(sh3), hole(sg3, 0), hp, _ptrs(out6)), zop(fake_dom, 1, 0, _ptrs(sh3), _ptrs(sg3), hp, hole(out6, 5)),
             rot(0, None, _p(out), n, 2, 1), rot(0, _p(s2[0]), None, n, 2, 1),
             blind(0, None, n, 2, hp, 2), blind(0, _p(out), n, 2, None, 2),
             lcw(sh=None), lcw(sl=None), lcw(cs=None), lcw(pb=None), lcw(pl=None), lcw(cp=None), lcw(out=None), lcw(sh=hole(s2, 1)), lcw(pb=hole(p2, 0))]
    for i, rc in enumerate(calls):
        assert rc == INVALID and b"NULL" in err(), (i, rc, err())
    # the field, ncomp and the sizes
    for f in (2, 9):
        for rc in (rot(f, _p(s2[0]), _p(out), n, 2, 1), blind(f, _p(out), n, 2, hp, 2), lcw(f=f)):
            assert rc == INVALID and b"field_of" in err(), err()
    for nc in (0, 3):
        assert rot(0, _p(s2[0]), _p(out), n, nc, 1) == INVALID and b"ncomp" in err()
        assert blind(0, _p(out), n, nc, hp, 2) == INVALID and b"ncomp" in err()
    for k in (n, n + 1, 1 << 40):
        assert rot(0, _p(s2[0]), _p(out), n, 2, k) == INVALID and b"k must be below n" in err(), k
    assert rot(0, _p(s2[0]), _p(out), (1 << 28) + 1, 1, 1) == INVALID and b"2^28" in err()
    assert rot(0, None, None, 0, 2, 0) == 0   # n = 0 does nothing
    for n_, k in ((n, 0), (n, 4), (2, 3), (2, 2), (1, 1), (0, 1)):
        assert blind(0, _p(out), n_, 2, hp, k) == INVALID and b"1 <= k <= 3 <= n" in err(), (n_, k)
    assert lcw(sl=[n + 7, n]) == INVALID and b"a length exceeds out_len" in err()
    assert lcw(pl=[n, n + 7]) == INVALID and b"a length exceeds out_len" in err()
    assert lcw(out_len=(1 << 28) + 1) == INVALID and b"2^28" in err()
    many = [s2[0]] * 65
    assert lcw(sh=_ptrs(many), sl=[1] * 65, ks=65) == INVALID and b"at most 64" in err()
    assert lcw(pb=_ptrs(many), pl=[1] * 65, kp=65) == INVALID and b"at most 64" in err()
    assert lcw(ks=0, kp=0) == INVALID and b"at least 1" in err()
    # overlap: rotate in place or shifted by one share; lincomb's output on a share vector, on the tail of a public vector
    big = buf(4 * n)
    at = lambda share: _p(big[8 * share:])
    assert rot(0, at(0), at(0), n, 2, 1) == INVALID and b"overlaps an input" in err()
    assert rot(0, at(0), at(n - 1), n, 2, 1) == INVALID and b"overlaps an input" in err()
    assert lcw(sh=_ptrs([big, s2[1]]), out=at(n + 5)) == INVALID and b"overlaps an input" in err()
    pbig = np.zeros(4 * 2 * n, dtype=np.uint64)
    assert lcw(pb=_ptrs([pbig, p2[1]]), out=_p(pbig[4 * (n - 1):])) == INVALID and b"overlaps an input" in err()


def test_no_device_no_result(hip):
    """Without a device every valid call fails with the no-device error: there is no CPU path."""
    if hip.have_device():
        pytest.skip("a HIP device is present")
    L = hip.lib()
    n = 8
    buf = lambda k: np.zeros(4 * 2 * k, dtype=np.uint64)
    host = np.ones(4 * 2 * 16, dtype=np.uint64)
    hp = _p(host)
    big = buf(2 * n)
    s2, p2, out = [buf(n + 6), buf(0)], [buf(n)], buf(n + 6)
    for rc in (L.csh_plonk_z_operands_dev(C.c_void_p(host.ctypes.data), u32(1), u32(2), _ptrs([buf(n)] * 3), _ptrs([buf(4 * n)] * 3), hp,
                                          _ptrs([buf(n) for _ in range(6)]), None),
               L.csh_vec_rotate_right_dev(0, _p(big), _p(big[8 * n:]), sz(n), u32(2), sz(n - 1), None),   # back to back is no overlap
               L.csh_plonk_blind_coefficients_dev(3, _p(out), sz(n), u32(2), hp, sz(3), None),
               L.csh_poly_lincomb_dev(1, u32(0), u32(0), _ptrs([s2[0], None]), (sz * 2)(n + 6, 0), hp, sz(2), _ptrs(p2), (sz * 1)(n), hp, sz(1),
                                      None, _p(out), sz(n + 6), None)):
        assert rc == NO_DEVICE
        assert re.search(b"no HIP device|no CPU fallback", L.csh_last_error())


# ---- the reference's own circuit -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
def test_fixture_chain_closes(curve):
    """On a satisfied circuit, for any challenges: the grand product returns to one, and both opening divisions are exact."""
    o = R.fixture_chain(curve)
    zk = o["zk"]
    assert zk.domain_size == 8 and len(o["witness"]) == zk.n_vars - zk.n_additions
    assert o["buffer_z"][0] == 1
    assert o["wxi_rem"] == 0
    assert o["wxiw_rem"] == 0
    assert len(o["wxi"]) == zk.domain_size + 5 and len(o["wxiw"]) == zk.domain_size + 2 and any(o["wxi"]) and any(o["wxiw"])


@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
def test_fixture_chain_on_the_host_kernels(hip, curve):
    """the round-2 operands and the round-5 combination of the fixture through the kernels' own functions"""
    F, T = H.FR[curve], R.Ops(H.FR[curve].p, 0, 0)
    o = R.fixture_chain(curve)
    zk, n = o["zk"], o["zk"].domain_size
    sh = lambda v: [(x,) for x in v]
    bufs = R.wire_buffers(F.p, zk, o["additions"], o["maps"], o["witness"])
    got = host_z_operands(hip, curve, T, n, sh(bufs[0]), sh(bufs[1]), sh(bufs[2]), [zk.polys[k][1] for k in ("S1", "S2", "S3")],
                          [o["beta"], o["gamma"], zk.k1, zk.k2])
    assert got == [sh(v) for v in o["operands"]]
    cs, cp, const0 = o["coefficients"]
    shares = [sh(o["poly"][k]) for k in ("z", "t1", "t2", "t3", "a", "b", "c")]
    publics = [zk.polys[k][0] for k in ("Qm", "Ql", "Qr", "Qo", "Qc", "S3", "S1", "S2")]
    assert host_lincomb(hip, curve, T, shares, cs, publics, cp, const0, n + 6) == sh(o["wxi_num"])
