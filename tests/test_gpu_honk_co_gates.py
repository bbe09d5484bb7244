"""Device tests of the five gate relations of the sumcheck round on shares (csrc/honk_co_gates.hip) against
tests/honk_co_gates_ref.py and against the plain entry csh_honk_sumcheck_accumulate_gates_dev. Every comparison is exact; every output
has guard words behind it and is checked to be canonical. The network between two stages is the device's local product (csh_vec_mul_dev,
csh_rep3_local_mul_vec_dev) with the in-process harness of the restatement rotating the halves. Every test calls entries that the parent
commit does not have."""
import functools

import numpy as np
import pytest

from tests import helpers as H
from tests import honk_co_gates_ref as CG
from tests import honk_co_relations_ref as CO
from tests import honk_gates_ref as G
from tests import honk_relations_ref as R
from tests.test_gpu_honk_co_relations import DevStages as FirstFourDevStages
from tests.test_gpu_honk_co_relations import _down, _guarded, dev_select, device_local_mul
from tests.test_honk_co_gates_cpu import SHAPE, table_of

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def case(curve, edges, plants=False):
    """without plants every relation keeps every edge: `edges` is the kept-edge count of all five"""
    return G.random_case(H.FR[curve].p, 2 * edges, 983 * edges + len(curve), plants=plants)


class DevStages:
    """the device entries over the parties' views, with the interface of CG.RefStages; columns are uploaded once per party"""

    def __init__(self, hip, curve, views, cols=None):
        self.hip, self.curve, self.F, self.cid, self.views = hip, curve, H.FR[curve], H.CURVE_IDS[curve], views
        parties = views["elliptic"]
        self.cols = cols or [[hip.DeviceBuffer.from_host(H.pack(self.F, v.polys[c])) for c in G.COLS] for v in parties]
        self.batches = {}
        v0 = parties[0]
        self.scaling = hip.DeviceBuffer.from_host(H.pack(self.F, v0.scaling)) if v0.scaling is not None else None
        self.lists = {rel: hip.DeviceBuffer.from_host(np.array(vs[0].edge_list + [0], dtype=np.uint32)) for rel, vs in views.items()}

    def m(self, rel):
        return self.views[rel][0].m

    def batch(self, rel, i):
        if (rel, i) not in self.batches:
            v = self.views[rel][i]
            self.batches[rel, i] = self.hip.HonkCoGatesBatch(self.cid, v.protocol, v.party, self.cols[i], v.edge_begin, v.edge_end, self.lists[rel], v.m,
                                                             self.scaling, v.stride, H.pack(self.F, list(v.params)))
        return self.batches[rel, i]

    def __getattr__(self, name):
        if name not in SHAPE:
            raise AttributeError(name)
        rel, n_in, n_in2, outs, is_fold = SHAPE[name]

        def stage(i, *ins):
            b = self.batch(rel, i)
            seg = 7 * b.m * b.ncomp
            assert [len(x) for x in ins] == [k * seg for k in (n_in, n_in2) if k], name
            counts = [o * b.ncomp if is_fold else o * seg for o in outs]
            ups = [self.hip.DeviceBuffer.from_host(H.pack(self.F, x) if x else np.zeros(4, dtype=np.uint64)) for x in ins]
            bufs = [_guarded(self.hip, 4 * k) for k in counts]
            getattr(self.hip, "honk_co_" + name)(b, *ups, *bufs)
            self.hip.bindings.sync()
            res = [_down(self.F, buf, 4 * k, name) for buf, k in zip(bufs, counts)]
            return res[0] if len(res) == 1 else tuple(res)
        return stage


def dev_lists(hip, curve, polys, b, e):
    """the five edge lists from csh_honk_co_select_edges_dev on each relation's own selector, checked against the restatement"""
    F = H.FR[curve]
    lists = {rel: dev_select(hip, curve, hip.DeviceBuffer.from_host(H.pack(F, polys[G.SELECTOR_OF[rel]])), b, e) for rel in G.RELATIONS}
    assert lists == CG.select_lists(polys, b, e)
    return lists


def run_case(hip, curve, kind, c, b, e, stride=1, scaled=True, device_net=False, parity=True, seed=3):
    """the five relations of `kind` parties on the device; parity: every stage output of every party against the restatement.
    -> (opened, the plain restatement's 17 accumulators, the device stages)"""
    p = H.FR[curve].p
    rnd = H.rng(seed)
    net = CO.NETS[kind](p, rnd, device_local_mul(hip, curve, CO.NETS[kind].protocol) if device_net else None)
    table = table_of(curve, c["n"], stride) if scaled else None
    party_polys = CO.share_polys(p, c["polys"], kind, rnd)
    views = CG.make_views(p, party_polys, net.protocol, c["params"], b, e, table, stride, dev_lists(hip, curve, c["polys"], b, e))
    dev = DevStages(hip, curve, views)
    st = CG.Both(CG.RefStages(views), dev) if parity else dev
    got = CG.open_round_gates(net, CG.run_round_gates(net, st))
    if parity:   # a relation without kept edges runs its fold stage only
        assert st.compared == net.n * sum(sum(1 for r, *_ in SHAPE.values() if r == rel) if dev.m(rel) else 1 for rel in G.RELATIONS)
    return got, G.accumulate_range(p, c["polys"], b, e, table, stride, c["params"]), dev


# 1, 2, 3 edges; 35 .. 37 and 41 .. 43: across the 36 and the 42 edge slots of a workgroup's pass; 257: several passes
@pytest.mark.parametrize("kind", ["rep3", "plain"])
@pytest.mark.parametrize("edges", [1, 2, 3, 35, 36, 37, 41, 42, 43, 257])
def test_stage_parity_on_bn254(gpu, kind, edges):
    got, want, dev = run_case(gpu, "bn254", kind, case("bn254", edges), 0, 2 * edges)
    assert all(dev.m(rel) == edges for rel in G.RELATIONS)
    assert got == want


@pytest.mark.parametrize("kind", ["rep3", "plain"])
@pytest.mark.parametrize("curve", ["bls12_381", "bls12_377"])
@pytest.mark.parametrize("edges", [1, 37])
def test_stage_parity_on_the_other_fields(gpu, curve, kind, edges):
    got, want, dev = run_case(gpu, curve, kind, case(curve, edges), 0, 2 * edges)
    assert all(dev.m(rel) == edges for rel in G.RELATIONS)
    assert got == want


@pytest.mark.parametrize("mb", [1, 2])
def test_capped_grids(gpu, mb):
    """257 edges with one and two workgroups: every grid-stride loop iterates more than once"""
    with gpu.tuned(vec_max_blocks=mb):
        got, want, _ = run_case(gpu, "bn254", "rep3", case("bn254", 257), 0, 514, stride=2)
    assert got == want


def test_a_sub_range(gpu):
    """edge_begin > 0 in the column index, the scaling index and the edge lists"""
    got, want, _ = run_case(gpu, "bn254", "rep3", case("bn254", 37, plants=True), 10, 60, stride=2)
    assert got == want


@pytest.mark.parametrize("stride", [1, 2, 4])
def test_scaling_strides(gpu, stride):
    got, want, _ = run_case(gpu, "bn254", "rep3", case("bn254", 12, plants=True), 0, 24, stride=stride)
    assert got == want


# ---- edge selection ---------------------------------------------------------------------------------------------------------------------------
def test_planted_selector_pairs(gpu):
    """per relation: zero/zero is left out; zero/non-zero and non-zero/zero are kept, and the one-end edges count"""
    curve, edges = "bn254", 12
    p, c = H.FR[curve].p, case(curve, edges)
    polys = {k: list(v) for k, v in c["polys"].items()}
    for sel in G.SELECTORS:
        polys[sel][2], polys[sel][3] = 0, 0
        polys[sel][6] = 0                      # zero / non-zero
        polys[sel][11] = 0                     # non-zero / zero
    lists = dev_lists(gpu, curve, polys, 0, 2 * edges)
    for rel in G.RELATIONS:
        assert 1 not in lists[rel] and 3 in lists[rel] and 5 in lists[rel] and len(lists[rel]) == edges - 1
    got, want, _ = run_case(gpu, curve, "rep3", dict(c, polys=polys), 0, 2 * edges)
    assert got == want
    assert want != G.accumulate_range(p, polys, 0, 2 * edges, table_of(curve, 2 * edges, 1), 1, c["params"], eager_skip=True), "the one-end edges count"


def test_an_all_skipped_range(gpu):
    """m = 0 with an edge list: no operand stage runs, and every accumulator entry is written as zero"""
    curve, edges = "bn254", 5
    c = case(curve, edges)
    polys = dict(c["polys"], **{sel: [0] * (2 * edges) for sel in G.SELECTORS})
    for kind in ("rep3", "plain"):
        got, want, dev = run_case(gpu, curve, kind, dict(c, polys=polys), 0, 2 * edges)
        assert all(dev.m(rel) == 0 for rel in G.RELATIONS)
        assert got == want and not any(any(a) for a in got)


# ---- the point 6 --------------------------------------------------------------------------------------------------------------------------------
def test_point_six_does_not_reach_a_six_long_accumulator(gpu):
    """product vectors that are zero but at the point 6 of 43 kept edges (so that a workgroup's second pass and its idle lanes are in
    play): the 6-long accumulators are zero while the point-6 sum is not (the 7-long Poseidon2 accumulators show it); at the point 5 the
    same data is seen"""
    curve, edges = "bn254", 43
    p = H.FR[curve].p
    c = case(curve, edges)
    zero_cols = {k: [0] * (2 * edges) for k in G.WITNESS + G.SHIFTED + ["q_c"]}
    views = CG.make_views(p, [dict(c["polys"], **zero_cols)], 0, c["params"], 0, 2 * edges)
    ref, dev = CG.RefStages(views), DevStages(gpu, curve, views)
    for name in ("ell_finish", "mem_finish", "nnf_finish", "pos_ext_finish", "pos_int_finish"):
        rel, n_in, n_in2, outs, _ = SHAPE[name]
        ln = 7 if name.startswith("pos") else 6
        for point in (6, 5):
            ins = [[7 + i // 7 if i % 7 == point else 0 for i in range(7 * edges * k)] for k in (n_in, n_in2) if k]
            got = getattr(dev, name)(0, *ins)
            assert got == getattr(ref, name)(0, *ins), (name, point)
            for s in range(outs[0] // ln):
                assert [bool(x) for x in got[s * ln:(s + 1) * ln]] == [k == point for k in range(ln)], (name, point, s)


# ---- against the plain entry ------------------------------------------------------------------------------------------------------------------
def _plain_entry(hip, curve, cols, b, e, params, scaling, stride):
    F = H.FR[curve]
    acc = hip.honk_sumcheck_accumulate_gates(H.CURVE_IDS[curve], cols, b, e, H.pack(F, list(params)), acc=_guarded(hip, 4 * 110), scaling=scaling,
                                             scaling_stride=stride)
    hip.bindings.sync()
    return G.split_acc(_down(F, acc, 4 * 110, "plain acc"))


@pytest.mark.parametrize("edges,stride", [(37, 1), (66, 4)])
def test_the_protocol_0_chain_equals_the_plain_entry(gpu, edges, stride):
    """csh_vec_mul_dev as the network; the same device columns go to csh_honk_sumcheck_accumulate_gates_dev: 110 words"""
    curve = "bn254"
    c = case(curve, edges, plants=True)
    assert len(c["planted"]) == 10
    got, want, dev = run_case(gpu, curve, "plain", c, 0, 2 * edges, stride=stride, device_net=True, parity=False)
    assert got == _plain_entry(gpu, curve, dev.cols[0], 0, 2 * edges, c["params"], dev.scaling, stride) and got == want


def test_null_scaling_is_the_factor_one(gpu):
    curve, edges = "bn254", 6
    c = case(curve, edges)
    got, want, dev = run_case(gpu, curve, "plain", c, 0, 2 * edges, scaled=False, device_net=True)
    assert dev.scaling is None
    assert got == want and got == _plain_entry(gpu, curve, dev.cols[0], 0, 2 * edges, c["params"], None, 1)


# ---- three Rep3 parties on the device -----------------------------------------------------------------------------------------------------------
def test_three_rep3_parties_open_to_the_plain_entry(gpu):
    curve, edges = "bn254", 37
    F = H.FR[curve]
    c = case(curve, edges, plants=True)
    got, want, dev = run_case(gpu, curve, "rep3", c, 0, 2 * edges, stride=4, device_net=True, parity=False)
    cols = [gpu.DeviceBuffer.from_host(H.pack(F, c["polys"][name])) for name in G.COLS]
    assert got == want and got == _plain_entry(gpu, curve, cols, 0, 2 * edges, c["params"], dev.scaling, 4)


def test_three_rep3_parties_on_a_satisfied_trace_and_the_whole_round(gpu):
    """rows of all five gate kinds. The seventeen opened accumulators equal the plain device entry's 110 words; with the first four
    relations' device stages, the whole round's batched univariate of the opened shares equals batch_over_relations_univariates_all on
    the plain accumulators, and S(0) + S(1) = 0, not trivially"""
    curve = "bn254"
    F = H.FR[curve]
    p = F.p
    t = G.satisfied_trace(p)
    n = t["n"]
    rnd = H.rng(21)
    betas, alphas = [rnd.randrange(1, p) for _ in range(6)], [rnd.randrange(1, p) for _ in range(G.NUM_ALPHAS)]
    gs = R.GateSeparator(p, betas, 6)
    net = CO.Rep3Net(p, rnd, device_local_mul(gpu, curve, 1))
    shared = CO.share_polys(p, t["polys"], "rep3", rnd)
    gviews = CG.make_views(p, shared, 1, t["gate_params"], 0, n, gs.beta_products, gs.periodicity, dev_lists(gpu, curve, t["polys"], 0, n))
    assert all(gviews[rel][0].m for rel in G.RELATIONS)
    gates = CG.run_round_gates(net, DevStages(gpu, curve, gviews))
    opened = CG.open_round_gates(net, gates)
    cols = [gpu.DeviceBuffer.from_host(H.pack(F, t["polys"][name])) for name in G.COLS]
    table = gpu.DeviceBuffer.from_host(H.pack(F, gs.beta_products))
    assert opened == _plain_entry(gpu, curve, cols, 0, n, t["gate_params"], table, gs.periodicity)
    assert opened == G.accumulate_range(p, t["polys"], 0, n, gs.beta_products, gs.periodicity, t["gate_params"])
    for s, a in enumerate(opened):
        assert a[0] == 0 and a[1] == 0, G.SUBRELATIONS[s]
    views = CO.make_views(p, shared, 1, t["params"], 0, n, gs.beta_products, gs.periodicity)
    first = CO.run_round(net, FirstFourDevStages(gpu, curve, views))
    acc = [first[i] + gates[i] for i in range(3)]
    S = net.open([CG.batch_over_relations_shares_all(p, acc[i], 2, alphas, gs.current_element(), gs.partial_evaluation_result) for i in range(3)])
    want = CO.open_round(net, first) + opened
    assert S == G.batch_over_relations_univariates_all(p, want, alphas, gs.current_element(), gs.partial_evaluation_result)
    assert (S[0] + S[1]) % p == 0 and any(S[2:])


# ---- shifted columns ------------------------------------------------------------------------------------------------------------------------
def test_shifted_columns_as_an_offset_into_a_longer_vector(gpu):
    """round 0: the four shifted witness columns passed as `ptr + 1 share` of vectors of n + 1 shares"""
    curve, edges = "bn254", 9
    F = H.FR[curve]
    p, n = F.p, 2 * edges
    c = case(curve, edges)
    r = H.rng(66)
    polys = {k: list(v) for k, v in c["polys"].items()}
    long = {k: polys[k] + [r.randrange(1, p)] for k in G.WITNESS}
    for k in long:
        polys[k + "_shift"] = long[k][1:]
    rnd = H.rng(67)
    net = CO.Rep3Net(p, rnd)
    shared_long = CO.share_polys(p, long, "rep3", rnd)
    party_polys = []
    for i in range(3):
        d = {k: v for k, v in polys.items() if k not in CO.SHARED}
        for k in long:
            d[k], d[k + "_shift"] = shared_long[i][k][:2 * n], shared_long[i][k][2:]
        party_polys.append(d)
    views = CG.make_views(p, party_polys, 1, c["params"], 0, n)
    cols = []
    for i in range(3):
        bufs = {k: gpu.DeviceBuffer.from_host(H.pack(F, shared_long[i][k])) for k in long}
        row = []
        for name in G.COLS:
            if name in bufs:
                row.append(bufs[name])
            elif name.endswith("_shift"):
                row.append(bufs[name[:-6]].ptr.value + 64)
            else:
                row.append(gpu.DeviceBuffer.from_host(H.pack(F, party_polys[i][name])))
        cols.append(row)
    dev = DevStages(gpu, curve, views, cols)
    dev.keep = cols
    got = CG.open_round_gates(net, CG.run_round_gates(net, CG.Both(CG.RefStages(views), dev)))
    assert got == G.accumulate_range(p, polys, 0, n, None, 1, c["params"])
