"""CPU tests of the Oink entries (csrc/honk_oink.hip: csh_honk_w4_records_dev, csh_honk_lookup_operands_dev, csh_honk_perm_operands_dev,
csh_honk_z_perm_place_dev): closed forms on the restatement tests/honk_oink_ref.py itself, Rep3 consistency, the arithmetic run on the host
through csh_selftest_honk_oink_host -- the argument builders and the per-index functions the gfx950 kernels call, with the limb-bound
contract checks of selftest.hip on (a violated bound aborts the process) -- and the C boundary without a device. Every comparison is exact
and covers every element."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import helpers as H
from tests import honk_oink_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVES = ["bn254", "bls12_381", "bls12_377"]
PARTIES = [(0, 0), (1, 0), (1, 1), (1, 2)]   # (protocol, party)
NO_DEVICE, INVALID = -2, -1
ENTRY = {"csh_honk_w4_records_dev": ["co_oink_prover.rs:98-160"], "csh_honk_lookup_operands_dev": ["co_oink_prover.rs:162-293"],
         "csh_honk_perm_operands_dev": ["co_oink_prover.rs:344-451"], "csh_honk_z_perm_place_dev": ["co_oink_prover.rs:472-504"]}
RANGE_SETS = [None, R.RANGES_3, [(1, 4), (4, 9), (12, 15)], [(2, 6), (9, 16)]]
sz, u32 = C.c_size_t, C.c_uint32
FILL = np.uint64(0xA5A5A5A5A5A5A5A5)
BN = H.FR["bn254"].p


def _p(x):
    return x.ctypes.data_as(C.c_void_p) if x is not None else None


def _ptrs(arrs):
    return (C.c_void_p * len(arrs))(*[a.ctypes.data if a is not None else None for a in arrs]) if len(arrs) else None


def _vec(F, v):
    return H.pack(F, R.flat(v))


def _shares(F, T, arr):
    v = H.unpack(F, arr)   # strict: canonical
    return [tuple(v[i * T.ncomp:(i + 1) * T.ncomp]) for i in range(len(v) // T.ncomp)]


def _ranges(ranges):
    flat = [x for r in (ranges or ()) for x in r]
    return ((sz * len(flat))(*flat) if flat else None), len(flat) // 2


def _host(hip, curve, entry, T, n, ins, outs, scalars=None, domain_size=0, ranges=None, idx=None):
    F = H.FR[curve]
    rg, nr = _ranges(ranges)
    lists = [np.asarray(v, dtype=np.uint32) for v in idx] if idx is not None else None
    counts = (sz * 3)(*[len(v) for v in idx]) if idx is not None else None
    return hip.lib().csh_selftest_honk_oink_host(H.CURVE_IDS[curve], entry, sz(n), sz(domain_size), u32(T.protocol), u32(T.party), _ptrs(ins),
                                                 _ptrs(lists) if lists is not None else None, counts, rg, sz(nr),
                                                 _p(H.pack(F, scalars)) if scalars else None, _ptrs(outs))


def host_w4(hip, curve, T, c):
    F = H.FR[curve]
    w4 = _vec(F, c["w"][3])
    ins = [_vec(F, c["w"][k]) for k in range(3)] + [_vec(F, c["type_share"]) if c["type_share"] else np.zeros(4, dtype=np.uint64)]
    assert _host(hip, curve, 0, T, c["n"], ins, [w4], scalars=c["etas"], idx=c["records"]) == 0
    return _shares(F, T, w4)


def host_lookup(hip, curve, T, c):
    F, n = H.FR[curve], c["n"]
    outs = [np.full(4 * T.ncomp * n, FILL, dtype=np.uint64) for _ in range(2)]
    ins = [_vec(F, c["w"][k]) for k in range(3)] + [_vec(F, c["tags"])] + [H.pack(F, v) for v in c["q"] + c["tables"] + [c["q_lookup"]]]
    assert _host(hip, curve, 1, T, n, ins, outs, scalars=c["ch"]) == 0
    return tuple(_shares(F, T, o) for o in outs)


def host_perm(hip, curve, T, c):
    F, n = H.FR[curve], c["n"]
    m = len(c["want_perm"][0])
    outs = [np.full(4 * T.ncomp * m, FILL, dtype=np.uint64) for _ in range(8)]
    ins = [_vec(F, v) for v in c["w"]] + [H.pack(F, v) for v in c["ident"] + c["sigma"]]
    assert _host(hip, curve, 2, T, n, ins, outs, scalars=c["ch"], domain_size=c["domain_size"], ranges=c["ranges"]) == 0
    return [_shares(F, T, o) for o in outs]


def host_place(hip, curve, T, c):
    F, n = H.FR[curve], c["n"]
    z = np.full(4 * T.ncomp * n, FILL, dtype=np.uint64)
    mul = _vec(F, c["mul"]) if c["mul"] else np.zeros(4, dtype=np.uint64)
    assert _host(hip, curve, 3, T, n, [mul], [z], domain_size=c["domain_size"], ranges=c["ranges"]) == 0
    return _shares(F, T, z)


def check_entries_on_host(hip, curve, T, c):
    assert host_w4(hip, curve, T, c) == c["want_w4"]
    assert host_lookup(hip, curve, T, c) == c["want_lookup"]
    assert host_perm(hip, curve, T, c) == c["want_perm"]
    assert host_place(hip, curve, T, c) == c["want_z"]


# ---- closed forms on the restatement itself ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_ranges", [False, True])
def test_permutation_closes(with_ranges):
    """a satisfied permutation, any challenges: z[1] = 1, the recurrence between consecutive active rows, one again at the last active row,
    constant gaps that hold the next range's first value, zeros behind"""
    c = R.perm_closed(BN, with_ranges)
    z = c["z"]
    R.check_perm_closed_form(BN, z, c["w"], c["ident"], c["sigma"], c["beta"], c["gamma"], c["rows"], c["n"], c["ranges"])
    if with_ranges:
        assert z[15] == 1 and z[5] == z[6] == z[7] == z[8] and z[11] == z[12] == z[13] == z[14]
    else:
        assert z[12] == 1 and z[13:] == [0, 0, 0]


def test_lookup_closes():
    c = R.lookup_closed(BN)
    assert sum(c["q_lookup"]) == 6 and c["q_lookup"][15] == 1 and sum(c["counts"]) == 6
    R.check_lookup_closed_form(BN, c)


def test_selector_form_is_the_plain_provers_continue_rule():
    """oink_prover.rs skips a row unless q_lookup or the tag is one; with both in {0, 1} the selector (1 - q) tag + q is that rule"""
    for q in (0, 1):
        for tag in (0, 1):
            assert ((1 - q) * tag + q) % BN == int(bool(q or tag))


def test_placement_keeps_the_one_at_an_inactive_index_1():
    T = R.Ops(BN, 0, 0)
    mul = [(10 + t,) for t in range(10)]
    z = R.z_perm_place(T, mul, 16, 16, [(2, 6), (9, 16)])   # 11 active indices
    assert z[0] == (0,) and z[1] == (1,) and z[2] == (0,) and z[3] == (10,) and z[6] == z[7] == z[8] == z[9] == (13,) and z[15] == (19,)
    # a set that starts at 1: index 1 is the active index of position 0, which no quotient overwrites
    z = R.z_perm_place(T, mul, 16, 16, [(1, 4), (4, 9), (12, 15)])
    assert z[1] == (1,) and z[2] == (10,) and z[9] == z[10] == z[11] == z[12] == (17,) and z[14] == (19,) and z[15] == (0,)
    # a set that starts at 0: the quotient of position 1 overwrites the one
    z = R.z_perm_place(T, mul[:4], 16, 16, [(0, 5)])
    assert z[:6] == [(0,), (10,), (11,), (12,), (13,), (0,)]


# ---- Rep3 consistency ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ranges", RANGE_SETS[:2])
def test_rep3_parties_add_up_to_the_plain_result(ranges):
    """Rep3 party k holds {x_k, x_(k-1)}: the a-components of the three parties' outputs sum to the plain output on the summed inputs"""
    p, n = BN, 16
    r = H.rng(77)
    plain_T = R.Ops(p, 0, 0)
    plain = R.entries_case(p, plain_T, n, lambda: r.randrange(p), 13, ranges)

    def split_vec(v):
        parts = []
        for s in v:
            a0, a1 = r.randrange(p), r.randrange(p)
            a = [a0, a1, (s[0] - a0 - a1) % p]
            parts.append([(a[k], a[k - 1]) for k in range(3)])
        return [[q[k] for q in parts] for k in range(3)]

    split = {name: split_vec(plain[name]) for name in ("tags", "type_share", "mul")}
    split_w = [split_vec(v) for v in plain["w"]]
    got = []
    for k in range(3):
        T = R.Ops(p, 1, k)
        w = [sw[k] for sw in split_w]
        got.append([
            R.w4_records(T, w[0], w[1], w[2], w[3], plain["etas"], plain["records"][0], plain["records"][1],
                         list(zip(plain["records"][2], split["type_share"][k]))),
            *R.lookup_operands(T, w[0], w[1], w[2], split["tags"][k], *plain["q"], plain["tables"], plain["q_lookup"], *plain["ch"]),
            *R.perm_operands(T, w, plain["ident"], plain["sigma"], *plain["ch"], 13, ranges),
            R.z_perm_place(T, split["mul"][k], n, 13, ranges)])
    want = [plain["want_w4"], *plain["want_lookup"], *plain["want_perm"], plain["want_z"]]
    assert len(want) == 12
    for j, wv in enumerate(want):
        vs = [got[k][j] for k in range(3)]
        assert [((vs[0][i][0] + vs[1][i][0] + vs[2][i][0]) % p,) for i in range(len(wv))] == wv, j
        for k in range(3):   # and the sharing stays replicated: party k's b is party k-1's a
            assert [s[1] for s in vs[k]] == [s[0] for s in vs[k - 1]], (j, k)


# ---- the kernels' own functions on the host ----------------------------------------------------------------------------------------------
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
    assert "csh_selftest_honk_oink_host" not in declared and hasattr(L, "csh_selftest_honk_oink_host")
    hpp = open(os.path.join(ROOT, "co-snarks_amd", "csrc", "honk_oink.hpp")).read()
    for cites in ENTRY.values():
        assert cites[0].split(":")[1] in hpp


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("protocol,party", PARTIES)
def test_entries_match_the_restatement(hip, curve, protocol, party):
    F, T = H.FR[curve], R.Ops(H.FR[curve].p, protocol, party)
    r = H.rng(3000 + 10 * protocol + party)
    for j, ranges in enumerate(RANGE_SETS):
        check_entries_on_host(hip, curve, T, R.entries_case(F.p, T, 16, lambda: r.randrange(F.p), 16 if ranges else 13, ranges))


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("protocol,party", PARTIES)
@pytest.mark.parametrize("fill", ["p-1", "0"])
def test_entries_at_the_edges_of_the_field(hip, curve, protocol, party, fill):
    """every share, public input and challenge p - 1, and every one 0; bound checks on"""
    F, T = H.FR[curve], R.Ops(H.FR[curve].p, protocol, party)
    v = F.p - 1 if fill == "p-1" else 0
    for ranges in (None, R.RANGES_3):
        check_entries_on_host(hip, curve, T, R.entries_case(F.p, T, 16, lambda: v, 16, ranges))


@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
def test_thirty_two_single_row_ranges_and_the_smallest_sizes(hip, curve):
    F, T = H.FR[curve], R.Ops(H.FR[curve].p, 1, 1)
    r = H.rng(32)
    c = R.entries_case(F.p, T, 64, lambda: r.randrange(F.p), 64, [(2 * j, 2 * j + 1) for j in range(32)])
    assert host_perm(hip, curve, T, c) == c["want_perm"] and host_place(hip, curve, T, c) == c["want_z"]
    # n = 2 with domain_size 1 and 2; one single-row range: m = 0, the one stays at index 1
    for ds, ranges in ((1, None), (2, None), (2, [(1, 2)]), (2, [(0, 1)])):
        c = R.entries_case(F.p, T, 2, lambda: r.randrange(F.p), ds, ranges, records=([1], [], []))
        assert len(c["mul"]) == (1 if (ds == 2 and not ranges) else 0)
        assert host_place(hip, curve, T, c) == c["want_z"], (ds, ranges)
        assert host_perm(hip, curve, T, c) == c["want_perm"], (ds, ranges)
        assert host_lookup(hip, curve, T, c) == c["want_lookup"]
        assert host_w4(hip, curve, T, c) == c["want_w4"]


@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
def test_closed_instances_on_the_host_kernels(hip, curve):
    """the operands of the closed instances through the kernels' functions, and the placement of the restatement's quotients"""
    F = H.FR[curve]
    p, T = F.p, R.Ops(F.p, 0, 0)
    sh = lambda v: [(x,) for x in v]
    for with_ranges in (False, True):
        c = R.perm_closed(p, with_ranges)
        m = len(c["ops"][0])
        case = dict(n=c["n"], domain_size=c["domain_size"], ranges=c["ranges"], w=[sh(v) for v in c["w"]], ident=c["ident"], sigma=c["sigma"],
                    ch=[c["beta"], c["gamma"]], want_perm=[sh(v) for v in c["ops"]])
        assert host_perm(hip, curve, T, case) == case["want_perm"]
        rows = c["rows"]
        case["mul"] = sh([c["z"][i] for i in rows[1:]])
        assert len(case["mul"]) == m
        assert host_place(hip, curve, T, case) == sh(c["z"])
    c = R.lookup_closed(p)
    case = dict(n=c["n"], w=[sh(v) for v in c["w"]], tags=sh(c["tags"]), q=c["q"], tables=c["tables"], q_lookup=c["q_lookup"], ch=[c["beta"], c["gamma"]])
    assert host_lookup(hip, curve, T, case) == (sh(c["prod"]), sh(c["sel"]))


# ---- the C boundary without a device -----------------------------------------------------------------------------------------------------
def test_refusals_come_before_the_device(hip):
    """every rule of the four calls answers CSH_ERR_INVALID on any machine; what is recorded is the status and the message"""
    L = hip.lib()
    err = lambda: L.csh_last_error()
    n = 16
    buf = lambda k: np.zeros(4 * 2 * k, dtype=np.uint64)
    host = np.ones(4 * 2 * 16, dtype=np.uint64)
    hp = _p(host)
    hole = lambda arrs, k: _ptrs(arrs[:k] + [None] + arrs[k + 1:])
    w3, w4 = [buf(n) for _ in range(3)], buf(n)
    lists = [np.zeros(4, dtype=np.uint32) for _ in range(3)]
    ts = buf(4)
    sh4, pub9, pub8, out2, out8 = [buf(n) for _ in range(4)], [buf(n) for _ in range(9)], [buf(n) for _ in range(8)], [buf(n) for _ in range(2)], [buf(n) for _ in range(8)]
    mul, z = buf(n), buf(n)

    good_w4 = dict(f=0, pr=1, pa=0, w=_ptrs(w3), w4=_p(w4), n=n, et=hp, ri=_p(lists[0]), nr=4, wi=_p(lists[1]), nw=4, si=_p(lists[2]), ts=_p(ts), ns=4)
    good_lk = dict(f=0, pr=1, pa=0, sh=_ptrs(sh4), pb=_ptrs(pub9), n=n, ch=hp, out=_ptrs(out2))
    good_pm = dict(f=0, pr=1, pa=0, sh=_ptrs(sh4), pb=_ptrs(pub8), n=n, ds=n, rg=None, ch=hp, out=_ptrs(out8))
    good_pl = dict(f=0, pr=1, pa=0, mul=_p(mul), z=_p(z), n=n, ds=n, rg=None)

    def w4c(**kw):
        a = {**good_w4, **kw}
        return L.csh_honk_w4_records_dev(a["f"], u32(a["pr"]), u32(a["pa"]), a["w"], a["w4"], sz(a["n"]), a["et"], a["ri"], sz(a["nr"]), a["wi"],
                                         sz(a["nw"]), a["si"], a["ts"], sz(a["ns"]), None)

    def lkc(**kw):
        a = {**good_lk, **kw}
        return L.csh_honk_lookup_operands_dev(a["f"], u32(a["pr"]), u32(a["pa"]), a["sh"], a["pb"], sz(a["n"]), a["ch"], a["out"], None)

    def pmc(**kw):
        a = {**good_pm, **kw}
        rg, nr = _ranges(a["rg"])
        rg = a.get("rg_ptr", rg)
        return L.csh_honk_perm_operands_dev(a["f"], u32(a["pr"]), u32(a["pa"]), a["sh"], a["pb"], sz(a["n"]), sz(a["ds"]), rg, sz(a.get("nrg", nr)), a["ch"],
                                            a["out"], None)

    def plc(**kw):
        a = {**good_pl, **kw}
        rg, nr = _ranges(a["rg"])
        rg = a.get("rg_ptr", rg)
        return L.csh_honk_z_perm_place_dev(a["f"], u32(a["pr"]), u32(a["pa"]), a["mul"], a["z"], sz(a["n"]), sz(a["ds"]), rg, sz(a.get("nrg", nr)), None)

    calls4 = (w4c, lkc, pmc, plc)
    # protocol and party, the field
    for pr, pa in ((2, 0), (0, 3), (1, 3), (7, 7)):
        for call in calls4:
            assert call(pr=pr, pa=pa) == INVALID and b"protocol" in err(), (pr, pa, err())
    for f in (2, 9):
        for call in calls4:
            assert call(f=f) == INVALID and b"field_of" in err(), err()
    # NULL pointers, the arrays and their entries
    nulls = [w4c(w=None), w4c(w4=None), w4c(et=None), w4c(ri=None), w4c(wi=None), w4c(si=None), w4c(ts=None), w4c(w=hole(w3, 1)),
             lkc(sh=None), lkc(pb=None), lkc(ch=None), lkc(out=None), lkc(sh=hole(sh4, 3)), lkc(pb=hole(pub9, 8)), lkc(out=hole(out2, 1)),
             pmc(sh=None), pmc(pb=None), pmc(ch=None), pmc(out=None), pmc(sh=hole(sh4, 0)), pmc(pb=hole(pub8, 7)), pmc(out=hole(out8, 4)),
             pmc(rg_ptr=None, nrg=2), plc(mul=None), plc(z=None), plc(rg_ptr=None, nrg=1)]
    for i, rc in enumerate(nulls):
        assert rc == INVALID and b"NULL" in err(), (i, rc, err())
    # sizes
    assert w4c(n=(1 << 28) + 1) == INVALID and b"2^28" in err()
    assert w4c(nr=n, nw=1, ns=0) == INVALID and b"more records than rows" in err()
    assert w4c(nr=1 << 63, nw=1 << 63, ns=0) == INVALID and b"more records than rows" in err()
    assert w4c(nr=0, nw=0, ns=0, w=None, w4=None, et=None) == 0   # no record: nothing to do, nothing looked at
    for bad in (0, (1 << 28) + 1):
        assert lkc(n=bad) == INVALID and b"n must be 1 .. 2^28" in err()
    for call in (pmc, plc):
        for bad in (0, 1, (1 << 28) + 1):
            assert call(n=bad, ds=1) == INVALID and b"n must be 2 .. 2^28" in err(), bad
        for ds in (0, n + 1, 1 << 40):
            assert call(ds=ds) == INVALID and b"domain_size must be 1 .. n" in err(), ds
        # malformed ranges: 33 of them, an empty one, an overlapping one, a decreasing one, one that ends behind n
        assert call(n=64, ds=64, rg=[(j, j + 1) for j in range(33)]) == INVALID and b"at most 32" in err()
        for rg in ([(0, 5), (7, 7)], [(3, 2)], [(0, 5), (4, 8)], [(8, 11), (0, 5)], [(0, 5), (14, 17)], [(16, 17)]):
            assert call(rg=rg) == INVALID and b"every active range" in err(), rg
    # overlaps: an output on an input, two outputs on each other
    big = buf(4 * n)
    at = lambda share: _p(big[8 * share:])
    assert w4c(w4=_p(w3[2])) == INVALID and b"overlaps an input" in err()
    assert w4c(w=_ptrs([w3[0], w3[1], big]), w4=at(n - 1)) == INVALID and b"overlaps an input" in err()
    assert w4c(ts=_p(w4[8 * (n - 1):])) == INVALID and b"overlaps an input" in err()
    assert lkc(out=_ptrs([sh4[3], out2[1]])) == INVALID and b"overlaps an input" in err()
    assert lkc(pb=_ptrs(pub9[:8] + [big]), out=_ptrs([out2[0], big[4 * (n - 1):]])) == INVALID and b"overlaps an input" in err()
    assert lkc(out=_ptrs([big, big[8 * (n - 1):]])) == INVALID and b"two outputs overlap" in err()
    assert pmc(out=_ptrs(out8[:7] + [sh4[0]])) == INVALID and b"overlaps an input" in err()
    assert pmc(out=_ptrs(out8[:6] + [big, big[8 * (n - 2):]])) == INVALID and b"two outputs overlap" in err()
    assert plc(z=_p(mul)) == INVALID and b"overlaps an input" in err()
    assert plc(mul=at(n - 1), z=at(0)) == INVALID and b"overlaps an input" in err()


def test_no_device_no_result(hip):
    """Without a device every valid call fails with the no-device error: there is no CPU path."""
    if hip.have_device():
        pytest.skip("a HIP device is present")
    L = hip.lib()
    n = 16
    buf = lambda k: np.zeros(4 * 2 * k, dtype=np.uint64)
    host = np.ones(4 * 2 * 16, dtype=np.uint64)
    hp = _p(host)
    idx = np.zeros(2, dtype=np.uint32)
    rg, nr = _ranges(R.RANGES_3)
    big = buf(2 * n)
    ins, outs = [buf(n) for _ in range(9)], [buf(n) for _ in range(8)]   # kept alive: the overlap rules compare their addresses
    for rc in (L.csh_honk_w4_records_dev(0, u32(1), u32(2), _ptrs(ins[:3]), _p(outs[0]), sz(n), hp, _p(idx), sz(2), None, sz(0), None, None, sz(0), None),
               L.csh_honk_lookup_operands_dev(1, u32(0), u32(0), _ptrs(ins[:4]), _ptrs(ins), sz(n), hp, _ptrs(outs[:2]), None),
               L.csh_honk_perm_operands_dev(3, u32(1), u32(1), _ptrs(ins[:4]), _ptrs(ins[:8]), sz(n), sz(n), rg, sz(nr), hp, _ptrs(outs), None),
               # back to back is no overlap: mul (n - 1 shares) directly in front of z
               L.csh_honk_z_perm_place_dev(0, u32(1), u32(0), _p(big), _p(big[8 * (n - 1):]), sz(n), sz(n), None, sz(0), None)):
        assert rc == NO_DEVICE
        assert re.search(b"no HIP device|no CPU fallback", L.csh_last_error())


def test_the_wrapper_checks_the_record_lists(hip):
    """HonkMemoryRecords refuses an index outside the trace and a duplicate, within a list or across lists, before anything is uploaded"""
    for read, write, shared in (([16], [], []), ([0, 3], [3], []), ([1, 1], [], []), ([2], [5], [5]), ([-1], [], [])):
        with pytest.raises(hip.CoSnarksHipError, match="outside|twice"):
            hip.HonkMemoryRecords(16, read, write, shared)
