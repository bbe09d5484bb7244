"""CPU tests of the sumcheck round on shares (csrc/honk_co_relations.hip): the restatement tests/honk_co_relations_ref.py
run by three Rep3 parties, three Shamir parties and one plain party over the in-process networks against the plain restatement
(tests/honk_relations_ref.py) on all 57 values; the stage functions of honk_co_relations.hpp run on the host through
csh_selftest_honk_co_relations_host against the restatement, word for word; and the C boundary without a device. The first two tests
compare restatements only and need no library: they check the reference that every other test, here and on the device, is held against."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from tests import helpers as H
from tests import honk_co_relations_ref as CO
from tests import honk_relations_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVES = ["bn254", "bls12_381", "bls12_377"]
NO_DEVICE, INVALID = -2, -1
sz, u32 = C.c_size_t, C.c_uint32
FILL = np.uint64(0xA5A5A5A5A5A5A5A5)
STAGE = {"select": 0, "arith_r0": 1, "arith_r1": 2, "perm_operands": 3, "perm_operands2": 4, "perm_finish": 5, "delta_operands": 6,
         "delta_sub_one": 7, "delta_finish": 8, "lookup_operands": 9, "lookup_mid_r0": 10, "lookup_mid_ops": 11, "lookup_finish": 12}
ENTRY = {
    "csh_honk_co_select_edges_dev": ["ultra_arithmetic_relation.rs:247-249", "delta_range_constraint_relation.rs:94-96"],
    "csh_honk_co_arith_dev": ["ultra_arithmetic_relation.rs:88-239", "relations/mod.rs:140-162"],
    "csh_honk_co_perm_operands_dev": ["permutation_relation.rs:70-146"],
    "csh_honk_co_perm_operands2_dev": [":226-234"],
    "csh_honk_co_perm_finish_dev": [":235-246"],
    "csh_honk_co_delta_operands_dev": ["delta_range_constraint_relation.rs:146-177"],
    "csh_honk_co_delta_sub_one_dev": [":181-183"],
    "csh_honk_co_delta_finish_dev": [":187-214"],
    "csh_honk_co_lookup_operands_dev": ["logderiv_lookup_relation.rs:92-139"],
    "csh_honk_co_lookup_mid_dev": [":277-295"],
    "csh_honk_co_lookup_finish_dev": [":296-309"],
}


def _p(x):
    return x.ctypes.data_as(C.c_void_p) if x is not None else None


def _ptrs(arrs):
    return (C.c_void_p * len(arrs))(*[a.ctypes.data if a is not None else None for a in arrs])


@functools.lru_cache(maxsize=None)
def case(curve, n, seed=0):
    return CO.random_case(H.FR[curve].p, n, 31 * n + seed)


def table_of(p, c, n, stride):
    assert c["n"] == n
    return CO.table_of(p, c, stride)


# ---- the restatement: parties over the in-process networks open to the plain accumulators ----------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("kind", ["plain", "rep3", "shamir"])
def test_parties_open_to_the_plain_accumulators(curve, kind):
    p = H.FR[curve].p
    n = 14
    c = case(curve, n)
    assert sorted(c["planted"]) == ["arith.one_end", "arith.skip", "delta.one_end", "delta.skip"]
    for (b, e, stride, scaled) in ((0, n, 2, True), (0, n, 1, False), (4, 10, 1, True)):
        table = table_of(p, c, n, stride) if scaled else None
        want = CO.plain_accumulate(p, c["polys"], b, e, table, stride, c["params"])
        assert want == R.accumulate_range(p, c["polys"], b, e, table, stride, c["params"], honour_skip=False), "arith and delta skips omit zeros only"
        assert all(any(a) for a in want)
        rnd = H.rng(5)
        net = CO.NETS[kind](p, rnd)
        views = CO.make_views(p, CO.share_polys(p, c["polys"], kind, rnd), net.protocol, c["params"], b, e, table, stride)
        got = CO.open_round(net, CO.run_round(net, CO.RefStages(views)))
        assert got == want, (kind, b, e)
    # the one-end edges are kept and count
    assert CO.one_end_edges_count(p, c["polys"], "q_arith", "arith", 0, n, None, 1, c["params"]) == [c["planted"]["arith.one_end"]]
    assert CO.one_end_edges_count(p, c["polys"], "q_delta_range", "delta", 0, n, None, 1, c["params"]) == [c["planted"]["delta.one_end"]]
    lists = CO.select_edges(c["polys"], "q_arith", 0, n)
    assert c["planted"]["arith.skip"] >> 1 not in lists and c["planted"]["arith.one_end"] >> 1 in lists and lists == sorted(lists)


@pytest.mark.parametrize("kind", ["rep3", "shamir"])
def test_batched_round_univariate_of_a_satisfied_trace_sums_to_zero(kind):
    """the share-wise batch_over_relations_univariates: S(0) + S(1) = 0 on the opened univariate, which is not trivially zero"""
    p = H.FR["bn254"].p
    t = R.satisfied_trace(p)
    rnd = H.rng(8)
    betas, alphas = [rnd.randrange(1, p) for _ in range(4)], [rnd.randrange(1, p) for _ in range(10)]
    gs = R.GateSeparator(p, betas, 4)
    net = CO.NETS[kind](p, rnd)
    views = CO.make_views(p, CO.share_polys(p, t["polys"], kind, rnd), net.protocol, t["params"], 0, t["n"], gs.beta_products, gs.periodicity)
    acc = CO.run_round(net, CO.RefStages(views))
    assert CO.open_round(net, acc) == CO.plain_accumulate(p, t["polys"], 0, t["n"], gs.beta_products, gs.periodicity, t["params"])
    S = net.open([CO.batch_over_relations_shares(p, acc[i], net.protocol + 1, CO.pub_comp(net.protocol, i), alphas, gs.current_element(),
                                                 gs.partial_evaluation_result) for i in range(3)])
    assert (S[0] + S[1]) % p == 0 and any(S[2:])


# ---- the stage functions of honk_co_relations.hpp on the host ----------------------------------------------------------------------------
class HostStages:
    """csh_selftest_honk_co_relations_host over the parties' views, with the interface of CO.RefStages"""

    def __init__(self, hip, curve, views):
        self.hip, self.curve, self.F, self.views = hip, curve, H.FR[curve], views

    def m(self, rel):
        return self.views[rel][0].m

    def call(self, stage, v, outs, inp=None, mask=None):
        """outs: element counts (0 = absent), or an array to update in place. -> the output lists"""
        F = self.F
        cols = [H.pack(F, v.polys[c]) for c in R.COLS]
        idx = np.array(v.edge_list, dtype=np.uint32) if v.edge_list is not None else None
        if idx is not None and idx.size == 0:
            idx = np.zeros(1, dtype=np.uint32)
        bufs = [o if isinstance(o, np.ndarray) else (np.full(4 * o + 4, FILL, dtype=np.uint64) if o else None) for o in outs] + [None] * (3 - len(outs))
        rc = self.hip.lib().csh_selftest_honk_co_relations_host(
            H.CURVE_IDS[self.curve], STAGE[stage], u32(v.protocol), u32(v.party), _ptrs(cols), sz(v.edge_begin), sz(v.edge_end), _p(idx), sz(v.m),
            _p(H.pack(F, v.scaling)) if v.scaling is not None else None, sz(v.stride), _p(H.pack(F, list(v.params))),
            _p(H.pack(F, inp)) if inp else None, _p(H.pack(F, mask)) if mask else None, *[_p(b) for b in bufs])
        assert rc == 0, self.hip.lib().csh_last_error()
        res = []
        for o, b in zip(outs, bufs):
            if b is None:
                res.append(None)
            elif isinstance(o, np.ndarray):
                res.append(H.unpack(F, b))
            else:
                assert (b[4 * o:] == FILL).all(), (stage, "written past the end")
                res.append(H.unpack(F, b[:4 * o]))          # strict: canonical
        return res

    def arith(self, i, mask):
        v = self.views["arith"][i]
        return self.call("arith_r0", v, [6], mask=mask)[0], self.call("arith_r1", v, [5 * v.ncomp])[0]

    def perm_operands(self, i):
        v = self.views["perm"][i]
        return tuple(self.call("perm_operands", v, [28 * v.m * v.ncomp] * 2))

    def perm_operands2(self, i):
        v = self.views["perm"][i]
        return self.call("perm_operands2", v, [14 * v.m * v.ncomp])[0]

    def perm_finish(self, i, prod):
        v = self.views["perm"][i]
        return self.call("perm_finish", v, [9 * v.ncomp], prod)[0]

    def delta_operands(self, i):
        v = self.views["delta"][i]
        return self.call("delta_operands", v, [56 * v.m * v.ncomp])[0]

    def delta_sub_one(self, i, sqr):
        v = self.views["delta"][i]
        return self.call("delta_sub_one", v, [H.pack(self.F, sqr).copy()])[0]

    def delta_finish(self, i, mul):
        v = self.views["delta"][i]
        return self.call("delta_finish", v, [24 * v.ncomp], mul)[0]

    def lookup_operands(self, i):
        v = self.views["lookup"][i]
        return tuple(self.call("lookup_operands", v, [7 * v.m * v.ncomp] * 2))

    def lookup_mid(self, i, wi):
        v = self.views["lookup"][i]
        r0 = self.call("lookup_mid_r0", v, [5 * v.ncomp], wi)[0]
        _, lhs, rhs = self.call("lookup_mid_ops", v, [0, 14 * v.m * v.ncomp, 14 * v.m * v.ncomp], wi)
        return r0, lhs, rhs

    def lookup_finish(self, i, mul):
        v = self.views["lookup"][i]
        return self.call("lookup_finish", v, [8 * v.ncomp], mul)[0]


def check_stages(hip, curve, polys, params, kind, b, e, scaling, stride, make_other, seed=3):
    p = H.FR[curve].p
    rnd = H.rng(seed)
    net = CO.NETS[kind](p, rnd)
    views = CO.make_views(p, CO.share_polys(p, polys, kind, rnd), net.protocol, params, b, e, scaling, stride)
    both = CO.Both(CO.RefStages(views), make_other(views))
    got = CO.open_round(net, CO.run_round(net, both))
    assert both.compared >= 8 * net.n
    return got, views


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("kind", ["plain", "rep3", "shamir"])
def test_host_stages_equal_the_restatement_on_random_data(hip, curve, kind):
    p = H.FR[curve].p
    n = 12
    c = case(curve, n, seed=1)
    for (b, e, stride, scaled) in ((0, n, 4, True), (2, 8, 1, False)):
        table = table_of(p, c, n, stride) if scaled else None
        got, _ = check_stages(hip, curve, c["polys"], c["params"], kind, b, e, table, stride, lambda views: HostStages(hip, curve, views))
        assert got == CO.plain_accumulate(p, c["polys"], b, e, table, stride, c["params"])


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("fill", ["0", "1", "p-1"])
def test_host_stages_at_the_edges_of_the_field(hip, curve, fill):
    """every column, share component, scaling factor, parameter and mask 0, 1 or p - 1"""
    p = H.FR[curve].p
    x = {"0": 0, "1": 1, "p-1": p - 1}[fill]
    n = 6
    polys = {c: [x] * n for c in R.COLS}
    polys["q_arith"][2] = polys["q_delta_range"][4] = 1                 # so that with fill 0 one edge of each list is kept
    scaling = [x] * n
    for protocol, parties in ((0, (0,)), (1, (0, 1, 2))):
        for party in parties:
            shared = {c: (v if c not in CO.SHARED else [x] * (n * (protocol + 1))) for c, v in polys.items()}
            views = CO.make_views(p, [shared] * (party + 1), protocol, (x, x, x), 0, n, scaling, 1)
            views = {rel: [vs[party]] * 3 for rel, vs in views.items()}
            ref, host = CO.RefStages(views), HostStages(hip, curve, views)
            nc, m7 = protocol + 1, 7 * (n // 2)
            vec = lambda count: [x] * (count * m7 * nc)
            mask = [x] * (7 * ref.m("arith")) if protocol else None
            assert host.arith(party, mask) == ref.arith(party, mask)
            assert host.perm_operands(party) == ref.perm_operands(party)
            assert host.perm_operands2(party) == ref.perm_operands2(party)
            assert host.perm_finish(party, vec(2)) == ref.perm_finish(party, vec(2))
            dm = 7 * ref.m("delta") * nc
            assert host.delta_operands(party) == ref.delta_operands(party)
            assert host.delta_sub_one(party, [x] * (8 * dm)) == ref.delta_sub_one(party, [x] * (8 * dm))
            assert host.delta_finish(party, [x] * (4 * dm)) == ref.delta_finish(party, [x] * (4 * dm))
            assert host.lookup_operands(party) == ref.lookup_operands(party)
            assert host.lookup_mid(party, vec(1)) == ref.lookup_mid(party, vec(1))
            assert host.lookup_finish(party, vec(2)) == ref.lookup_finish(party, vec(2))


@pytest.mark.parametrize("curve", CURVES)
def test_host_edge_selection(hip, curve):
    F = H.FR[curve]
    n = 40
    r = H.rng(4)
    q = [r.choice((0, 0, 1, F.p - 1, r.randrange(F.p))) for _ in range(n)]
    for b, e in ((0, n), (6, 30), (38, 40)):
        out, count = np.full(n // 2 + 2, 0xFFFFFFFF, dtype=np.uint32), np.zeros(1, dtype=np.uint32)
        rc = hip.lib().csh_selftest_honk_co_relations_host(H.CURVE_IDS[curve], STAGE["select"], u32(0), u32(0), None, sz(b), sz(e), None, sz(0), None, sz(1),
                                                           None, _p(H.pack(F, q)), None, _p(out), _p(count), None)
        want = CO.select_edges({"q": q}, "q", b, e)
        assert rc == 0 and int(count[0]) == len(want) and list(out[:len(want)]) == want and (out[len(want):] == 0xFFFFFFFF).all()
    assert 0 < len(CO.select_edges({"q": q}, "q", 0, n)) < n // 2


# ---- the C boundary without a device -----------------------------------------------------------------------------------------------------
def test_refusals_come_before_the_device(hip):
    L = hip.lib()
    err = lambda: L.csh_last_error()
    n, m = 16, 8
    cols = [np.zeros(8 * n, dtype=np.uint64) for _ in range(36)]
    par, table, idx = np.ones(12, dtype=np.uint64), np.zeros(4 * n, dtype=np.uint64), np.zeros(m, dtype=np.uint32)
    vec = lambda k: np.zeros(8 * 7 * m * k, dtype=np.uint64)
    acc = np.zeros(8 * 24, dtype=np.uint64)

    def common(f=0, protocol=1, party=0, cols_=cols, b=0, e=n, idx_=None, m_=m):
        return (f, u32(protocol), u32(party), _ptrs(cols_) if cols_ is not None else None, sz(b), sz(e), _p(idx_), sz(m_))

    calls = {
        "arith": lambda scaling=_p(table), stride=1, protocol=1, mask=vec(1), **kw: L.csh_honk_co_arith_dev(
            *common(protocol=protocol, **kw), scaling, sz(stride), _p(mask), _p(acc), _p(acc[64:]), None),
        "perm_operands": lambda **kw: L.csh_honk_co_perm_operands_dev(*common(**kw), _p(par), _p(vec(4)), _p(vec(4)), None),
        "perm_operands2": lambda **kw: L.csh_honk_co_perm_operands2_dev(*common(**kw), _p(par), _p(vec(2)), None),
        "perm_finish": lambda scaling=_p(table), stride=1, **kw: L.csh_honk_co_perm_finish_dev(*common(**kw), scaling, sz(stride), _p(vec(2)), _p(acc), None),
        "delta_operands": lambda **kw: L.csh_honk_co_delta_operands_dev(*common(**kw), _p(vec(8)), None),
        "delta_finish": lambda scaling=_p(table), stride=1, **kw: L.csh_honk_co_delta_finish_dev(*common(**kw), scaling, sz(stride), _p(vec(4)), _p(acc), None),
        "lookup_operands": lambda **kw: L.csh_honk_co_lookup_operands_dev(*common(**kw), _p(par), _p(vec(1)), _p(vec(1)), None),
        "lookup_mid": lambda scaling=_p(table), stride=1, **kw: L.csh_honk_co_lookup_mid_dev(
            *common(**kw), scaling, sz(stride), _p(par), _p(vec(1)), _p(acc), _p(vec(2)), _p(vec(2)), None),
        "lookup_finish": lambda scaling=_p(table), stride=1, **kw: L.csh_honk_co_lookup_finish_dev(*common(**kw), scaling, sz(stride), _p(par), _p(vec(2)), _p(acc), None),
    }
    for name, call in calls.items():
        for f in (2, 9):
            assert call(f=f) == INVALID and b"field_of" in err(), name
        assert call(party=3) == INVALID and b"party_id" in err(), name
        for b, e in ((1, 4), (0, 3), (4, 4), (6, 2), (0, (1 << 28) + 2)):
            assert call(b=b, e=e) == INVALID and b"even" in err(), (name, b, e)
        assert call(cols_=None) == INVALID and b"NULL" in err(), name
        assert call(cols_=[None] * 36) == INVALID and b"NULL" in err(), name
        assert call(m_=m - 1) == INVALID and b"m must be" in err(), name           # no list: every edge of the range
        assert call(idx_=idx, m_=m + 1) == INVALID and b"m must be" in err(), name
        if name in ("arith", "perm_finish", "delta_finish", "lookup_mid", "lookup_finish"):
            for stride in (0, (1 << 28) + 1):
                assert call(stride=stride) == INVALID and b"scaling_stride" in err(), name
        if not hip.have_device():
            assert call() == NO_DEVICE and call(idx_=idx, m_=3) == NO_DEVICE, name      # valid: as far as asking for a device
    # the mask: required for Rep3, refused for protocol 0
    assert calls["arith"](mask=None) == INVALID and b"mask" in err()
    assert calls["arith"](protocol=0) == INVALID and b"mask" in err()
    # an output on an input, an output on another output
    big = vec(9)
    assert L.csh_honk_co_perm_operands_dev(*common(), _p(par), _p(big), _p(big[8 * 7 * m * 4 - 4:]), None) == INVALID and b"two outputs overlap" in err()
    assert L.csh_honk_co_perm_finish_dev(*common(), _p(table), sz(1), _p(big), _p(big[8 * 7 * m * 2 - 4:]), None) == INVALID and b"overlaps an input" in err()
    assert L.csh_honk_co_delta_operands_dev(*common(), _p(cols[0]), None) == INVALID and b"overlaps an input" in err()
    assert L.csh_honk_co_lookup_mid_dev(*common(), _p(table), sz(1), _p(par), _p(big), _p(acc), _p(vec(2)), _p(big[8 * 7 * m - 4:]), None) == INVALID
    assert b"overlaps an input" in err()
    # edge selection and the in-place stage
    sel = lambda f=0, q=_p(table), b=0, e=n, out=_p(idx), cnt=_p(np.zeros(1, dtype=np.uint32)): L.csh_honk_co_select_edges_dev(f, q, sz(b), sz(e), out, cnt, None)
    assert sel(f=2) == INVALID and b"field_of" in err()
    assert sel(q=None) == INVALID and sel(out=None) == INVALID and sel(cnt=None) == INVALID and b"NULL" in err()
    assert sel(b=1) == INVALID and b"even" in err()
    assert sel(cnt=_p(idx[2:])) == INVALID and b"two outputs overlap" in err()
    assert L.csh_honk_co_delta_sub_one_dev(0, u32(2), u32(0), _p(big), sz(1), None) == INVALID and b"protocol" in err()
    assert L.csh_honk_co_delta_sub_one_dev(0, u32(0), u32(0), None, sz(1), None) == INVALID and b"NULL" in err()
    assert L.csh_honk_co_delta_sub_one_dev(0, u32(0), u32(0), _p(big), sz((1 << 27) + 1), None) == INVALID and b"2^27" in err()
    if not hip.have_device():
        assert sel() == NO_DEVICE and L.csh_honk_co_delta_sub_one_dev(0, u32(1), u32(1), _p(big), sz(1), None) == NO_DEVICE


def test_the_wrappers_check_the_column_count_and_the_range(hip):
    cols = [1 << 20] * 36
    par = np.ones(12, dtype=np.uint64)
    with pytest.raises(hip.CoSnarksHipError, match="columns"):
        hip.HonkCoBatch(0, 1, 0, cols[:35], 0, 2, params=par)
    for b, e in ((1, 4), (0, 3), (2, 2), (0, (1 << 28) + 2), (-2, 2)):
        with pytest.raises(hip.CoSnarksHipError, match="even"):
            hip.HonkCoBatch(0, 1, 0, cols, b, e, params=par)
        with pytest.raises(hip.CoSnarksHipError, match="even"):
            hip.honk_co_select_edges(0, 1 << 20, b, e, edge_idx=1 << 21, count=1 << 22)
    with pytest.raises(hip.CoSnarksHipError, match="scaling_stride"):
        hip.HonkCoBatch(0, 1, 0, cols, 0, 2, scaling=1 << 22, scaling_stride=0)
    with pytest.raises(hip.CoSnarksHipError, match="protocol"):
        hip.HonkCoBatch(0, 2, 0, cols, 0, 2)
    for idx, m in ((None, 3), (1 << 21, 5)):
        with pytest.raises(hip.CoSnarksHipError, match="m must be"):
            hip.HonkCoBatch(0, 1, 0, cols, 0, 8, edge_idx=idx, m=m)
    with pytest.raises(hip.CoSnarksHipError, match="params"):
        hip.HonkCoBatch(0, 1, 0, cols, 0, 8, params=np.ones(8, dtype=np.uint64))
    with pytest.raises(hip.CoSnarksHipError, match="mask"):
        hip.honk_co_arith(hip.HonkCoBatch(0, 1, 0, cols, 0, 8), mask=None, r0=1 << 21, r1=1 << 22)
    with pytest.raises(hip.CoSnarksHipError, match="mask"):
        hip.honk_co_arith(hip.HonkCoBatch(0, 0, 0, cols, 0, 8), mask=1 << 23, r0=1 << 21, r1=1 << 22)
    with pytest.raises(hip.CoSnarksHipError, match="2\\^27"):
        hip.honk_co_delta_sub_one(0, 0, 0, 1 << 21, (1 << 27) + 1)


def test_header_bindings_and_sys_crate_declare_the_entry_points(hip):
    from cosnarks_amd import bindings
    txt = open(bindings.header_path()).read()
    declared = bindings.declared_symbols()
    sys_rs = open(os.path.join(ROOT, "rust", "cosnarks-hip-sys", "src", "lib.rs")).read()
    src = open(bindings.__file__).read()
    L = hip.lib()
    for name, cites in ENTRY.items():
        assert name in declared and hasattr(L, name), name
        at = txt.index("int %s(" % name)
        comment = txt[txt.rindex("/*", 0, at):at]
        for c in cites:
            assert c in comment, (name, c)
        assert "pub fn %s(" % name in sys_rs
        assert hasattr(hip, name[4:-4]) and "lib().%s(" % name in src
    assert "co-noir UltraHonk, the sumcheck round on shares" in txt
    assert "csh_selftest_honk_co_relations_host" not in declared and hasattr(L, "csh_selftest_honk_co_relations_host")
    assert "honk_co_relations.hip" in open(os.path.join(ROOT, "co-snarks_amd", "build.py")).read()
    # the stage numbers of this file are the enum's
    hpp = open(os.path.join(ROOT, "co-snarks_amd", "csrc", "honk_co_relations.hpp")).read()
    import re
    enum = re.search(r"enum HcStage : int \{(.*?)\};", hpp, re.S).group(1)
    names = [x.strip().split(" ")[0] for x in enum.split(",")]
    assert names == ["HC_SELECT", "HC_ARITH_R0", "HC_ARITH_R1", "HC_PERM_OPS", "HC_PERM_OPS2", "HC_PERM_FINISH", "HC_DELTA_OPS", "HC_DELTA_SUB_ONE",
                     "HC_DELTA_FINISH", "HC_LOOKUP_OPS", "HC_LOOKUP_MID_R0", "HC_LOOKUP_MID_OPS", "HC_LOOKUP_FINISH"] and list(STAGE.values()) == list(range(13))
