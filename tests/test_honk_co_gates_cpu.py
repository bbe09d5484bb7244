"""CPU tests of the five gate relations of the sumcheck round on shares (csrc/honk_co_gates.hip): the restatement
tests/honk_co_gates_ref.py run by one plain party, three Rep3 parties and three Shamir parties over the in-process networks against the
plain restatement (tests/honk_gates_ref.py) on all 110 values; the stage functions of honk_co_gates.hpp run on the host through
csh_selftest_honk_co_gates_host against the restatement, word for word; and the C boundary without a device.
test_parties_open_to_the_plain_accumulators and test_batched_round_univariate_over_all_28_accumulators compare restatements only and
need no library: they pass on the parent commit too, and check the reference that every other test, here and on the device, is held
against. Every other test calls entries that the parent does not have."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from tests import helpers as H
from tests import honk_co_gates_ref as CG
from tests import honk_co_relations_ref as CO
from tests import honk_gates_ref as G
from tests import honk_relations_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVES = ["bn254", "bls12_381", "bls12_377"]
NO_DEVICE, INVALID = -2, -1
sz, u32 = C.c_size_t, C.c_uint32
FILL = np.uint64(0xA5A5A5A5A5A5A5A5)
STAGE = {"ell_operands": 0, "ell_operands2": 1, "ell_finish": 2, "mem_operands": 3, "mem_finish": 4, "nnf_operands": 5, "nnf_finish": 6,
         "pos_ext_operands": 7, "pos_ext_finish": 8, "pos_int_operands": 9, "pos_int_finish": 10}
# stage -> (relation, parts of in, parts of in2, parts of each output or the accumulator's elements, a fold stage)
SHAPE = {"ell_operands": ("elliptic", 0, 0, [7, 7], False), "ell_operands2": ("elliptic", 7, 0, [5, 5], False),
         "ell_finish": ("elliptic", 7, 5, [12], True), "mem_operands": ("memory", 0, 0, [6, 6, 1], False),
         "mem_finish": ("memory", 6, 1, [36], True), "nnf_operands": ("nnf", 0, 0, [5, 5], False), "nnf_finish": ("nnf", 5, 0, [6], True),
         "pos_ext_operands": ("poseidon2_external", 0, 0, [4], False), "pos_ext_finish": ("poseidon2_external", 4, 0, [28], True),
         "pos_int_operands": ("poseidon2_internal", 0, 0, [1], False), "pos_int_finish": ("poseidon2_internal", 1, 0, [28], True)}
ENTRY = {
    "csh_honk_co_ell_operands_dev": ["elliptic_relation.rs:116-168"],
    "csh_honk_co_ell_operands2_dev": [":173-195"],
    "csh_honk_co_ell_finish_dev": [":199-252", ":208-249"],
    "csh_honk_co_mem_operands_dev": ["memory_relation.rs:241-357", ":272-357"],
    "csh_honk_co_mem_finish_dev": [":370-455"],
    "csh_honk_co_nnf_operands_dev": ["non_native_field_relation.rs:138-150"],
    "csh_honk_co_nnf_finish_dev": [":154-213"],
    "csh_honk_co_pos_ext_operands_dev": ["poseidon2_external_relation.rs:165-174"],
    "csh_honk_co_pos_ext_finish_dev": [":181-226"],
    "csh_honk_co_pos_int_operands_dev": ["poseidon2_internal_relation.rs:155"],
    "csh_honk_co_pos_int_finish_dev": [":163-223"],
}


def _p(x):
    return x.ctypes.data_as(C.c_void_p) if x is not None else None


def _ptrs(arrs):
    return (C.c_void_p * len(arrs))(*[a.ctypes.data if a is not None else None for a in arrs])


@functools.lru_cache(maxsize=None)
def case(curve, n, seed=0):
    return G.random_case(H.FR[curve].p, n, 37 * n + seed)


@functools.lru_cache(maxsize=None)
def table_of(curve, n, stride):
    """the gate-separator products that reach every edge of n elements at this stride"""
    p = H.FR[curve].p
    r = H.rng(91)
    return R.beta_products(p, [r.randrange(1, p) for _ in range(12)], max(1, ((n // 2 - 1) * stride).bit_length()))


# ---- the restatement: parties over the in-process networks open to the plain accumulators ----------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("kind", ["plain", "rep3", "shamir"])
def test_parties_open_to_the_plain_accumulators(curve, kind):
    """the shared and the plain skip are the same rule here (selector zero at both ends), so the 110 values are those of
    G.accumulate_range as it stands. Needs no library."""
    p = H.FR[curve].p
    n = 24
    c = case(curve, n)
    assert sorted(c["planted"]) == sorted(G.PLANTS)
    for (b, e, stride, scaled) in ((0, n, 2, True), (0, n, 1, False), (2, 22, 1, True)):
        table = table_of(curve, n, stride) if scaled else None
        want = G.accumulate_range(p, c["polys"], b, e, table, stride, c["params"])
        assert want == G.accumulate_range(p, c["polys"], b, e, table, stride, c["params"], honour_skip=False), "the skips omit zeros only"
        assert want != G.accumulate_range(p, c["polys"], b, e, table, stride, c["params"], eager_skip=True), "the one-end edges count"
        assert all(any(a) for a in want)
        rnd = H.rng(5)
        net = CO.NETS[kind](p, rnd)
        views = CG.make_views(p, CO.share_polys(p, c["polys"], kind, rnd), net.protocol, c["params"], b, e, table, stride)
        got = CG.open_round_gates(net, CG.run_round_gates(net, CG.RefStages(views)))
        assert got == want, (kind, b, e)
    lists = CG.select_lists(c["polys"], 0, n)
    for rel in G.RELATIONS:
        assert c["planted"][rel + ".skip"] >> 1 not in lists[rel] and c["planted"][rel + ".one_end"] >> 1 in lists[rel]
        assert lists[rel] == sorted(lists[rel]) and len(lists[rel]) == n // 2 - 1


@pytest.mark.parametrize("kind", ["rep3", "shamir"])
def test_batched_round_univariate_over_all_28_accumulators(kind):
    """the nine relations in the reference's order on a satisfied trace with rows of every gate kind: the parties' accumulators open to
    the plain ones, and the share-wise batch_over_relations_univariates opens to the plain round univariate, with S(0) + S(1) = 0.
    Needs no library."""
    p = H.FR["bn254"].p
    t = G.satisfied_trace(p)
    n = t["n"]
    rnd = H.rng(8)
    betas, alphas = [rnd.randrange(1, p) for _ in range(6)], [rnd.randrange(1, p) for _ in range(G.NUM_ALPHAS)]
    gs = R.GateSeparator(p, betas, 6)
    net = CO.NETS[kind](p, rnd)
    shared = CO.share_polys(p, t["polys"], kind, rnd)
    views = CO.make_views(p, shared, net.protocol, t["params"], 0, n, gs.beta_products, gs.periodicity)
    gviews = CG.make_views(p, shared, net.protocol, t["gate_params"], 0, n, gs.beta_products, gs.periodicity)
    assert all(gviews[rel][0].m for rel in G.RELATIONS), "the trace has rows of all five gate kinds"
    first, gates = CO.run_round(net, CO.RefStages(views)), CG.run_round_gates(net, CG.RefStages(gviews))
    acc = [first[i] + gates[i] for i in range(net.n)]
    want = (R.accumulate_range(p, t["polys"], 0, n, gs.beta_products, gs.periodicity, t["params"]) +
            G.accumulate_range(p, t["polys"], 0, n, gs.beta_products, gs.periodicity, t["gate_params"]))
    assert CO.open_round(net, first) + CG.open_round_gates(net, gates) == want
    S = net.open([CG.batch_over_relations_shares_all(p, acc[i], net.protocol + 1, alphas, gs.current_element(), gs.partial_evaluation_result)
                  for i in range(net.n)])
    assert S == G.batch_over_relations_univariates_all(p, want, alphas, gs.current_element(), gs.partial_evaluation_result)
    assert (S[0] + S[1]) % p == 0 and any(S[2:])


# ---- the stage functions of honk_co_gates.hpp on the host ----------------------------------------------------------------------------------
class HostStages:
    """csh_selftest_honk_co_gates_host over the parties' views, with the interface of CG.RefStages"""

    def __init__(self, hip, curve, views):
        self.hip, self.curve, self.F, self.views = hip, curve, H.FR[curve], views

    def m(self, rel):
        return self.views[rel][0].m

    def __getattr__(self, name):
        if name not in STAGE:
            raise AttributeError(name)
        rel, n_in, n_in2, outs, is_fold = SHAPE[name]

        def stage(i, *ins):
            F, v = self.F, self.views[rel][i]
            seg = 7 * v.m * v.ncomp
            assert [len(x) for x in ins] == [k * seg for k in (n_in, n_in2) if k], name
            cols = [H.pack(F, v.polys[c]) for c in G.COLS]
            idx = np.array(v.edge_list if v.edge_list else [0], dtype=np.uint32) if v.edge_list is not None else None
            counts = [o * v.ncomp if is_fold else o * seg for o in outs]
            bufs = [np.full(4 * k + 4, FILL, dtype=np.uint64) for k in counts] + [None] * (3 - len(outs))
            packed = [H.pack(F, x) if len(x) else None for x in ins] + [None, None]
            rc = self.hip.lib().csh_selftest_honk_co_gates_host(
                H.CURVE_IDS[self.curve], STAGE[name], u32(v.protocol), u32(v.party), _ptrs(cols), sz(v.edge_begin), sz(v.edge_end), _p(idx), sz(v.m),
                _p(H.pack(F, v.scaling)) if v.scaling is not None else None, sz(v.stride), _p(H.pack(F, list(v.params))), _p(packed[0]), _p(packed[1]),
                *[_p(b) for b in bufs])
            assert rc == 0, self.hip.lib().csh_last_error()
            res = []
            for k, b in zip(counts, bufs):
                assert (b[4 * k:] == FILL).all(), (name, "written past the end")
                res.append(H.unpack(F, b[:4 * k]))                      # strict: canonical
            return res[0] if len(res) == 1 else tuple(res)
        return stage


def check_stages(curve, polys, gate_params, kind, b, e, scaling, stride, make_other, seed=3):
    p = H.FR[curve].p
    rnd = H.rng(seed)
    net = CO.NETS[kind](p, rnd)
    views = CG.make_views(p, CO.share_polys(p, polys, kind, rnd), net.protocol, gate_params, b, e, scaling, stride)
    both = CG.Both(CG.RefStages(views), make_other(views))
    got = CG.open_round_gates(net, CG.run_round_gates(net, both))
    assert both.compared == len(STAGE) * net.n
    return got, views


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("kind", ["plain", "rep3", "shamir"])
def test_host_stages_equal_the_restatement_on_random_data(hip, curve, kind):
    p = H.FR[curve].p
    n = 24
    c = case(curve, n, seed=1)
    for (b, e, stride, scaled) in ((0, n, 4, True), (2, 20, 1, False)):
        table = table_of(curve, n, stride) if scaled else None
        got, _ = check_stages(curve, c["polys"], c["params"], kind, b, e, table, stride, lambda views: HostStages(hip, curve, views))
        assert got == G.accumulate_range(p, c["polys"], b, e, table, stride, c["params"])


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("fill", ["0", "1", "p-1"])
def test_host_stages_at_the_edges_of_the_field(hip, curve, fill):
    """every column, share component, scaling factor, parameter and product vector 0, 1 or p - 1"""
    p = H.FR[curve].p
    x = {"0": 0, "1": 1, "p-1": p - 1}[fill]
    n = 6
    polys = {c: [x] * n for c in G.COLS}
    for k, sel in enumerate(G.SELECTORS):
        polys[sel][2 + (k & 1)] = 1                                    # so that with fill 0 one edge of every list is kept
    scaling = [x] * n
    for protocol, parties in ((0, (0,)), (1, (0, 1, 2))):
        for party in parties:
            shared = {c: (v if c not in CO.SHARED else [x] * (n * (protocol + 1))) for c, v in polys.items()}
            views = CG.make_views(p, [shared] * (party + 1), protocol, (x,) * 8, 0, n, scaling, 1)
            views = {rel: [vs[party]] * 3 for rel, vs in views.items()}
            ref, host = CG.RefStages(views), HostStages(hip, curve, views)
            for name, (rel, n_in, n_in2, _, _) in SHAPE.items():
                seg = 7 * ref.m(rel) * (protocol + 1)
                assert seg, (name, "an edge is kept")
                ins = [[x] * (k * seg) for k in (n_in, n_in2) if k]
                assert getattr(host, name)(party, *ins) == getattr(ref, name)(party, *ins), (name, protocol, party)


def test_point_six_does_not_reach_a_six_long_accumulator(hip):
    """one kept edge whose product vectors are zero but at the point 6: the 6-long accumulators are zero, the restatement agrees, and the
    same data at the point 5 is seen"""
    curve = "bn254"
    p = H.FR[curve].p
    c = G.random_case(p, 4, 11, plants=False)
    views = CG.make_views(p, [c["polys"]], 0, c["params"], 0, 2)
    ref, host = CG.RefStages(views), HostStages(hip, curve, views)
    # with the share columns and q_c zero, every term is driven by the product vectors alone
    zero_cols = {k: [0] * 4 for k in G.WITNESS + G.SHIFTED + ["q_c"]}
    zviews = CG.make_views(p, [dict(c["polys"], **zero_cols)], 0, c["params"], 0, 2)
    zref, zhost = CG.RefStages(zviews), HostStages(hip, curve, zviews)
    for name in ("ell_finish", "mem_finish", "nnf_finish"):
        rel, n_in, n_in2, outs, _ = SHAPE[name]
        assert ref.m(rel) == zref.m(rel) == 1
        for point, seen in ((6, False), (5, True)):
            # part q of a product vector: 7 + q at `point`, zero elsewhere
            ins = [[7 + i // 7 if i % 7 == point else 0 for i in range(7 * k)] for k in (n_in, n_in2) if k]
            got = getattr(zhost, name)(0, *ins)
            assert got == getattr(zref, name)(0, *ins), name
            assert any(got) == seen, (name, point)
            if seen:
                assert all(got[s * 6 + 5] for s in range(outs[0] // 6)) and not any(got[s * 6 + k] for s in range(outs[0] // 6) for k in range(5))
            assert getattr(host, name)(0, *ins) == getattr(ref, name)(0, *ins), name


# ---- the C boundary without a device -----------------------------------------------------------------------------------------------------
def test_refusals_come_before_the_device(hip):
    L = hip.lib()
    err = lambda: L.csh_last_error()
    n, m = 16, 8
    cols = [np.zeros(8 * n, dtype=np.uint64) for _ in range(19)]
    par, table, idx = np.ones(32, dtype=np.uint64), np.zeros(4 * n, dtype=np.uint64), np.zeros(m, dtype=np.uint32)
    vec = lambda k: np.zeros(8 * 7 * m * k, dtype=np.uint64)
    acc = np.zeros(8 * 36, dtype=np.uint64)

    def common(f=0, protocol=1, party=0, cols_=cols, b=0, e=n, idx_=None, m_=m):
        return (f, u32(protocol), u32(party), _ptrs(cols_) if cols_ is not None else None, sz(b), sz(e), _p(idx_), sz(m_))

    calls = {
        "ell_operands": lambda **kw: L.csh_honk_co_ell_operands_dev(*common(**kw), _p(vec(7)), _p(vec(7)), None),
        "ell_operands2": lambda **kw: L.csh_honk_co_ell_operands2_dev(*common(**kw), _p(par), _p(vec(7)), _p(vec(5)), _p(vec(5)), None),
        "ell_finish": lambda scaling=_p(table), stride=1, **kw: L.csh_honk_co_ell_finish_dev(*common(**kw), scaling, sz(stride), _p(vec(7)), _p(vec(5)), _p(acc), None),
        "mem_operands": lambda **kw: L.csh_honk_co_mem_operands_dev(*common(**kw), _p(par), _p(vec(6)), _p(vec(6)), _p(vec(1)), None),
        "mem_finish": lambda scaling=_p(table), stride=1, **kw: L.csh_honk_co_mem_finish_dev(
            *common(**kw), scaling, sz(stride), _p(par), _p(vec(6)), _p(vec(1)), _p(acc), None),
        "nnf_operands": lambda **kw: L.csh_honk_co_nnf_operands_dev(*common(**kw), _p(vec(5)), _p(vec(5)), None),
        "nnf_finish": lambda scaling=_p(table), stride=1, **kw: L.csh_honk_co_nnf_finish_dev(*common(**kw), scaling, sz(stride), _p(vec(5)), _p(acc), None),
        "pos_ext_operands": lambda **kw: L.csh_honk_co_pos_ext_operands_dev(*common(**kw), _p(vec(4)), None),
        "pos_ext_finish": lambda scaling=_p(table), stride=1, **kw: L.csh_honk_co_pos_ext_finish_dev(*common(**kw), scaling, sz(stride), _p(vec(4)), _p(acc), None),
        "pos_int_operands": lambda **kw: L.csh_honk_co_pos_int_operands_dev(*common(**kw), _p(vec(1)), None),
        "pos_int_finish": lambda scaling=_p(table), stride=1, **kw: L.csh_honk_co_pos_int_finish_dev(
            *common(**kw), scaling, sz(stride), _p(par), _p(vec(1)), _p(acc), None),
    }
    assert sorted(calls) == sorted(STAGE)
    for name, call in calls.items():
        for f in (2, 9):
            assert call(f=f) == INVALID and b"field_of" in err(), name
        assert call(party=3) == INVALID and b"party_id" in err(), name
        assert call(protocol=2) == INVALID and b"protocol" in err(), name
        for b, e in ((1, 4), (0, 3), (4, 4), (6, 2), (0, (1 << 28) + 2)):
            assert call(b=b, e=e) == INVALID and b"even" in err(), (name, b, e)
        assert call(cols_=None) == INVALID and b"NULL" in err(), name
        assert call(cols_=[None] * 19) == INVALID and b"NULL" in err(), name
        assert call(m_=m - 1) == INVALID and b"m must be" in err(), name           # no list: every edge of the range
        assert call(idx_=idx, m_=m + 1) == INVALID and b"m must be" in err(), name
        if name.endswith("finish"):
            for stride in (0, (1 << 28) + 1):
                assert call(stride=stride) == INVALID and b"scaling_stride" in err(), name
        if not hip.have_device():
            assert call() == NO_DEVICE and call(idx_=idx, m_=3) == NO_DEVICE, name      # valid: as far as asking for a device
    # required vectors and parameters
    assert L.csh_honk_co_ell_operands_dev(*common(), None, _p(vec(7)), None) == INVALID and b"NULL" in err()
    assert L.csh_honk_co_ell_operands2_dev(*common(), None, _p(vec(7)), _p(vec(5)), _p(vec(5)), None) == INVALID and b"NULL" in err()
    assert L.csh_honk_co_ell_finish_dev(*common(), _p(table), sz(1), _p(vec(7)), None, _p(acc), None) == INVALID and b"NULL" in err()
    assert L.csh_honk_co_mem_operands_dev(*common(), _p(par), _p(vec(6)), _p(vec(6)), None, None) == INVALID and b"NULL" in err()
    assert L.csh_honk_co_mem_finish_dev(*common(), _p(table), sz(1), None, _p(vec(6)), _p(vec(1)), _p(acc), None) == INVALID and b"NULL" in err()
    assert L.csh_honk_co_nnf_finish_dev(*common(), _p(table), sz(1), _p(vec(5)), None, None) == INVALID and b"NULL" in err()
    assert L.csh_honk_co_pos_int_finish_dev(*common(), _p(table), sz(1), None, _p(vec(1)), _p(acc), None) == INVALID and b"NULL" in err()
    # an output on an input, an output on another output
    big = vec(15)
    assert L.csh_honk_co_ell_operands_dev(*common(), _p(big), _p(big[8 * 7 * m * 7 - 4:]), None) == INVALID and b"two outputs overlap" in err()
    assert L.csh_honk_co_ell_operands2_dev(*common(), _p(par), _p(big), _p(big[8 * 7 * m * 7 - 4:]), _p(vec(5)), None) == INVALID
    assert b"overlaps an input" in err()
    assert L.csh_honk_co_mem_finish_dev(*common(), _p(table), sz(1), _p(par), _p(big), _p(vec(1)), _p(big[8 * 7 * m * 6 - 4:]), None) == INVALID
    assert b"overlaps an input" in err()
    assert L.csh_honk_co_nnf_operands_dev(*common(), _p(cols[0]), _p(vec(5)), None) == INVALID and b"overlaps an input" in err()
    assert L.csh_honk_co_mem_operands_dev(*common(), _p(par), _p(vec(6)), _p(big), _p(big[8 * 7 * m * 6 - 4:]), None) == INVALID
    assert b"two outputs overlap" in err()
    # the selftest export refuses an unknown stage
    assert L.csh_selftest_honk_co_gates_host(0, 11, u32(0), u32(0), _ptrs(cols), sz(0), sz(n), None, sz(m), None, sz(1), _p(par), None, None,
                                             _p(vec(7)), _p(vec(7)), None) == INVALID and b"unknown stage" in err()


def test_the_wrappers_check_the_column_count_and_the_range(hip):
    cols = [1 << 20] * 19
    par = np.ones(32, dtype=np.uint64)
    with pytest.raises(hip.CoSnarksHipError, match="columns"):
        hip.HonkCoGatesBatch(0, 1, 0, [1 << 20] * 36, 0, 2, params=par)
    for b, e in ((1, 4), (0, 3), (2, 2), (0, (1 << 28) + 2), (-2, 2)):
        with pytest.raises(hip.CoSnarksHipError, match="even"):
            hip.HonkCoGatesBatch(0, 1, 0, cols, b, e, params=par)
    with pytest.raises(hip.CoSnarksHipError, match="scaling_stride"):
        hip.HonkCoGatesBatch(0, 1, 0, cols, 0, 2, scaling=1 << 22, scaling_stride=0)
    with pytest.raises(hip.CoSnarksHipError, match="protocol"):
        hip.HonkCoGatesBatch(0, 2, 0, cols, 0, 2)
    for idx, m in ((None, 3), (1 << 21, 5)):
        with pytest.raises(hip.CoSnarksHipError, match="m must be"):
            hip.HonkCoGatesBatch(0, 1, 0, cols, 0, 8, edge_idx=idx, m=m)
    with pytest.raises(hip.CoSnarksHipError, match="params are eta_1"):
        hip.HonkCoGatesBatch(0, 1, 0, cols, 0, 8, params=np.ones(12, dtype=np.uint64))
    b = hip.HonkCoGatesBatch(0, 1, 0, cols, 0, 8)
    for call in (lambda: hip.honk_co_ell_operands2(b, 1 << 21, lhs=1 << 22, rhs=1 << 23), lambda: hip.honk_co_mem_operands(b, 1 << 21, 1 << 22, 1 << 23),
                 lambda: hip.honk_co_mem_finish(b, 1 << 21, 1 << 22, acc=1 << 23), lambda: hip.honk_co_pos_int_finish(b, 1 << 21, acc=1 << 23)):
        with pytest.raises(hip.CoSnarksHipError, match="no params"):
            call()
    # the batch of the first four relations keeps its own rules
    with pytest.raises(hip.CoSnarksHipError, match="params are beta"):
        hip.HonkCoBatch(0, 1, 0, [1 << 20] * 36, 0, 8, params=par)


def test_header_bindings_and_sys_crate_declare_the_entry_points(hip):
    from cosnarks_amd import bindings
    txt = open(bindings.header_path()).read()
    declared = bindings.declared_symbols()
    sys_rs = open(os.path.join(ROOT, "rust", "cosnarks-hip-sys", "src", "lib.rs")).read()
    co_rs = open(os.path.join(ROOT, "rust", "co-noir-hip", "src", "co_sumcheck.rs")).read()
    src = open(bindings.__file__).read()
    L = hip.lib()
    for name, cites in ENTRY.items():
        assert name in declared and hasattr(L, name), name
        at = txt.index("int %s(" % name)
        comment = txt[txt.rindex("/*", 0, at):at]
        for c in cites:
            assert c in comment, (name, c)
        assert "pub fn %s(" % name in sys_rs and "sys::%s(" % name in co_rs
        assert hasattr(hip, name[4:-4]) and "lib().%s(" % name in src
    assert sorted(n[len("csh_honk_co_"):-len("_dev")] for n in ENTRY) == sorted(STAGE)
    assert "the sumcheck round on shares: the five gate relations" in txt
    assert "csh_selftest_honk_co_gates_host" not in declared and hasattr(L, "csh_selftest_honk_co_gates_host")
    assert "honk_co_gates.hip" in open(os.path.join(ROOT, "co-snarks_amd", "build.py")).read()
    # the stage numbers of this file are the enum's
    hpp = open(os.path.join(ROOT, "co-snarks_amd", "csrc", "honk_co_gates.hpp")).read()
    enum = re.search(r"enum HgcStage : int \{(.*?)\};", hpp, re.S).group(1)
    names = [x.strip().split(" ")[0] for x in enum.split(",")]
    assert names == ["HGC_ELL_OPS", "HGC_ELL_OPS2", "HGC_ELL_FINISH", "HGC_MEM_OPS", "HGC_MEM_FINISH", "HGC_NNF_OPS", "HGC_NNF_FINISH",
                     "HGC_POS_EXT_OPS", "HGC_POS_EXT_FINISH", "HGC_POS_INT_OPS", "HGC_POS_INT_FINISH", "HGC_STAGES"]
    assert list(STAGE.values()) == list(range(11))
