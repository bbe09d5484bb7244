"""Device tests of the sumcheck round on shares (csrc/honk_co_relations.hip) against tests/honk_co_relations_ref.py and
against the plain entry csh_honk_sumcheck_accumulate_dev. Every comparison is exact; every output has guard words behind it and is
checked to be canonical. The network between two stages is the device's local product (csh_vec_mul_dev, csh_rep3_local_mul_vec_dev)
with the in-process harness of the restatement rotating the halves."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import helpers as H
from tests import honk_co_relations_ref as CO
from tests import honk_relations_ref as R

pytestmark = pytest.mark.gpu
GUARD = np.uint64(0x5A5AC3C3A5A53C3C)
NGUARD = 8
sz = C.c_size_t


@functools.lru_cache(maxsize=None)
def case(curve, edges):
    return CO.random_case(H.FR[curve].p, 2 * edges, 977 * edges + len(curve))


def _guarded(hip, words):
    return hip.DeviceBuffer.from_host(np.full(words + NGUARD, GUARD, dtype=np.uint64))


def _down(F, buf, words, what):
    raw = buf.to_host()
    assert raw.size == words + NGUARD and (raw[words:] == GUARD).all(), (what, "written past the end")
    return H.unpack(F, raw[:words])          # strict: canonical


class DevStages:
    """the device entries over the parties' views, with the interface of CO.RefStages; columns are uploaded once per party"""

    def __init__(self, hip, curve, views, cols=None):
        self.hip, self.curve, self.F, self.cid, self.views = hip, curve, H.FR[curve], H.CURVE_IDS[curve], views
        parties = views["perm"]
        self.cols = cols or [[hip.DeviceBuffer.from_host(H.pack(self.F, v.polys[c])) for c in R.COLS] for v in parties]
        self.batches = {}
        v0 = parties[0]
        self.scaling = hip.DeviceBuffer.from_host(H.pack(self.F, v0.scaling)) if v0.scaling is not None else None
        self.lists = {rel: (hip.DeviceBuffer.from_host(np.array(vs[0].edge_list + [0], dtype=np.uint32)) if vs[0].edge_list is not None else None)
                      for rel, vs in views.items()}

    def m(self, rel):
        return self.views[rel][0].m

    def batch(self, rel, i):
        if (rel, i) not in self.batches:
            v = self.views[rel][i]
            self.batches[rel, i] = self.hip.HonkCoBatch(self.cid, v.protocol, v.party, self.cols[i], v.edge_begin, v.edge_end, self.lists[rel], v.m,
                                                        self.scaling, v.stride, H.pack(self.F, list(v.params)))
        return self.batches[rel, i]

    def up(self, vals):
        return self.hip.DeviceBuffer.from_host(H.pack(self.F, vals) if vals else np.zeros(4, dtype=np.uint64))

    def out(self, elems):
        return _guarded(self.hip, 4 * elems)

    def down(self, buf, elems, what):
        self.hip.bindings.sync()
        return _down(self.F, buf, 4 * elems, what)

    def arith(self, i, mask):
        b = self.batch("arith", i)
        r0, r1 = self.hip.honk_co_arith(b, self.up(mask) if b.protocol == 1 else None, self.out(6), self.out(5 * b.ncomp))
        return self.down(r0, 6, "arith.r0"), self.down(r1, 5 * b.ncomp, "arith.r1")

    def perm_operands(self, i):
        b = self.batch("perm", i)
        n = 28 * b.m * b.ncomp
        lhs, rhs = self.hip.honk_co_perm_operands(b, self.out(n), self.out(n))
        return self.down(lhs, n, "perm lhs"), self.down(rhs, n, "perm rhs")

    def perm_operands2(self, i):
        b = self.batch("perm", i)
        n = 14 * b.m * b.ncomp
        return self.down(self.hip.honk_co_perm_operands2(b, self.out(n)), n, "perm rhs2")

    def perm_finish(self, i, prod):
        b = self.batch("perm", i)
        return self.down(self.hip.honk_co_perm_finish(b, self.up(prod), self.out(9 * b.ncomp)), 9 * b.ncomp, "perm acc")

    def delta_operands(self, i):
        b = self.batch("delta", i)
        n = 56 * b.m * b.ncomp
        return self.down(self.hip.honk_co_delta_operands(b, self.out(n)), n, "delta lhs")

    def delta_sub_one(self, i, sqr):
        b = self.batch("delta", i)
        buf = self.hip.DeviceBuffer.from_host(np.concatenate([H.pack(self.F, sqr), np.full(NGUARD, GUARD, dtype=np.uint64)]))
        self.hip.honk_co_delta_sub_one(self.cid, b.protocol, b.party, buf, b.m)
        return self.down(buf, len(sqr), "delta sqr")

    def delta_finish(self, i, mul):
        b = self.batch("delta", i)
        return self.down(self.hip.honk_co_delta_finish(b, self.up(mul), self.out(24 * b.ncomp)), 24 * b.ncomp, "delta acc")

    def lookup_operands(self, i):
        b = self.batch("lookup", i)
        n = 7 * b.m * b.ncomp
        rt, inv = self.hip.honk_co_lookup_operands(b, self.out(n), self.out(n))
        return self.down(rt, n, "read_term"), self.down(inv, n, "inverses")

    def lookup_mid(self, i, wi):
        b = self.batch("lookup", i)
        n = 14 * b.m * b.ncomp
        r0, lhs, rhs = self.hip.honk_co_lookup_mid(b, self.up(wi), self.out(5 * b.ncomp), self.out(n), self.out(n))
        return self.down(r0, 5 * b.ncomp, "lookup.r0"), self.down(lhs, n, "lookup lhs"), self.down(rhs, n, "lookup rhs")

    def lookup_finish(self, i, mul):
        b = self.batch("lookup", i)
        return self.down(self.hip.honk_co_lookup_finish(b, self.up(mul), self.out(8 * b.ncomp)), 8 * b.ncomp, "lookup acc")


def device_local_mul(hip, curve, protocol):
    """the local product of T::mul_many on the device: csh_vec_mul_dev, or csh_rep3_local_mul_vec_dev with the harness's masks"""
    F, cid = H.FR[curve], H.CURVE_IDS[curve]

    def mul(i, x, y, mask):
        if not x:
            return []
        n = len(x) // (protocol + 1)
        dx, dy, out = hip.DeviceBuffer.from_host(H.pack(F, x)), hip.DeviceBuffer.from_host(H.pack(F, y)), _guarded(hip, 4 * n)
        if protocol == 1:
            dm = hip.DeviceBuffer.from_host(H.pack(F, mask))
            assert hip.lib().csh_rep3_local_mul_vec_dev(cid, dx.ptr, dy.ptr, dm.ptr, out.ptr, sz(n), None) == 0
        else:
            assert hip.lib().csh_vec_mul_dev(cid, dx.ptr, dy.ptr, out.ptr, sz(n), None) == 0
        hip.bindings.sync()
        return _down(F, out, 4 * n, "local product")
    return mul


def dev_select(hip, curve, qbuf, b, e):
    """-> the kept e >> 1 of the device, after checking the count word and that nothing behind the count was written"""
    edges = (e - b) // 2
    idx = hip.DeviceBuffer.from_host(np.full(edges + 2, 0xFFFFFFFF, dtype=np.uint32))
    cnt = hip.DeviceBuffer.from_host(np.full(4, 0xFFFFFFFF, dtype=np.uint32))
    hip.honk_co_select_edges(H.CURVE_IDS[curve], qbuf, b, e, idx, cnt)
    hip.bindings.sync()
    c, out = cnt.to_host(np.uint32), idx.to_host(np.uint32)
    assert (c[1:] == 0xFFFFFFFF).all() and c[0] <= edges and (out[c[0]:] == 0xFFFFFFFF).all()
    return [int(x) for x in out[:c[0]]]


def run_case(hip, curve, kind, c, b, e, stride=1, scaled=True, device_net=False, parity=True, seed=3):
    """the round of `kind` parties on the device; parity: every stage output of every party against the restatement. -> (opened, want)"""
    p = H.FR[curve].p
    rnd = H.rng(seed)
    net = CO.NETS[kind](p, rnd, device_local_mul(hip, curve, CO.NETS[kind].protocol) if device_net else None)
    table = CO.table_of(p, c, stride) if scaled else None
    party_polys = CO.share_polys(p, c["polys"], kind, rnd)
    # the edge lists come from the device
    q = {col: hip.DeviceBuffer.from_host(H.pack(H.FR[curve], c["polys"][col])) for col in ("q_arith", "q_delta_range")}
    lists = {"arith": dev_select(hip, curve, q["q_arith"], b, e), "delta": dev_select(hip, curve, q["q_delta_range"], b, e)}
    assert lists["arith"] == CO.select_edges(c["polys"], "q_arith", b, e) and lists["delta"] == CO.select_edges(c["polys"], "q_delta_range", b, e)
    views = CO.make_views(p, party_polys, net.protocol, c["params"], b, e, table, stride, lists)
    dev = DevStages(hip, curve, views)
    st = CO.Both(CO.RefStages(views), dev) if parity else dev
    got = CO.open_round(net, CO.run_round(net, st))
    if parity:
        assert st.compared >= 8 * net.n
    return got, CO.plain_accumulate(p, c["polys"], b, e, table, stride, c["params"]), dev


# 1, 2, 3 edges; 36 and 37: the 7 m values of a plain operand vector across the 256 lanes of a workgroup (252, 259); 41 .. 43: across the
# 42 edge slots of a workgroup's pass of the fold; 257: several passes
@pytest.mark.parametrize("kind", ["rep3", "plain"])
@pytest.mark.parametrize("edges", [1, 2, 3, 36, 37, 41, 42, 43, 257])
def test_stage_parity_on_bn254(gpu, kind, edges):
    got, want, _ = run_case(gpu, "bn254", kind, case("bn254", edges), 0, 2 * edges)
    assert got == want


@pytest.mark.parametrize("kind", ["rep3", "plain"])
@pytest.mark.parametrize("curve", ["bls12_381", "bls12_377"])
@pytest.mark.parametrize("edges", [1, 37])
def test_stage_parity_on_the_other_fields(gpu, curve, kind, edges):
    got, want, _ = run_case(gpu, curve, kind, case(curve, edges), 0, 2 * edges)
    assert got == want


@pytest.mark.parametrize("mb", [1, 2])
def test_capped_grids(gpu, mb):
    """257 edges with one and two workgroups: every grid-stride loop and the compaction's tiles iterate more than once"""
    with gpu.tuned(vec_max_blocks=mb):
        got, want, _ = run_case(gpu, "bn254", "rep3", case("bn254", 257), 0, 514, stride=2)
    assert got == want


def test_a_sub_range(gpu):
    """edge_begin > 0 in the column index, the scaling index and the edge lists"""
    got, want, _ = run_case(gpu, "bn254", "rep3", case("bn254", 37), 10, 60, stride=2)
    assert got == want


# ---- edge selection ---------------------------------------------------------------------------------------------------------------------------
def test_planted_selector_pairs(gpu):
    """zero/zero is left out; zero/non-zero and non-zero/zero are kept, and each adds a non-zero value to every subrelation of its relation"""
    curve, edges = "bn254", 12
    F = H.FR[curve]
    p, c = F.p, case(curve, edges)
    polys = {k: list(v) for k, v in c["polys"].items()}
    for col, rel in (("q_arith", "arith"), ("q_delta_range", "delta")):
        polys[col][2], polys[col][3] = 0, 0
        polys[col][6] = 0                      # zero / non-zero
        polys[col][11] = 0                     # non-zero / zero
        one_end = CO.one_end_edges_count(p, polys, col, rel, 0, 2 * edges, None, 1, c["params"])
        assert {6, 10} <= set(one_end)
        kept = dev_select(gpu, curve, gpu.DeviceBuffer.from_host(H.pack(F, polys[col])), 0, 2 * edges)
        assert kept == CO.select_edges(polys, col, 0, 2 * edges) and 1 not in kept and 3 in kept and 5 in kept
    got, want, _ = run_case(gpu, curve, "rep3", dict(c, polys=polys), 0, 2 * edges)
    assert got == want


def test_an_all_skipped_range(gpu):
    """count 0, and the accumulators of the two relations are zero (every entry written)"""
    curve, edges = "bn254", 5
    p, c = H.FR[curve].p, case(curve, edges)
    polys = dict(c["polys"], q_arith=[0] * (2 * edges), q_delta_range=[0] * (2 * edges))
    for kind in ("rep3", "plain"):
        got, want, dev = run_case(gpu, curve, kind, dict(c, polys=polys), 0, 2 * edges)
        assert dev.m("arith") == 0 and dev.m("delta") == 0
        assert got == want and not any(any(a) for s in (0, 1, 7, 8, 9, 10) for a in [got[s]]) and all(any(got[s]) for s in (2, 3, 4, 5, 6))


@pytest.mark.parametrize("mb", [0, 1, 2])
def test_stable_order_at_257_edges(gpu, mb):
    curve, edges = "bn254", 257
    F = H.FR[curve]
    r = H.rng(257)
    q = [r.choice((0, 0, 0, 1, r.randrange(F.p))) for _ in range(2 * edges)]
    want = CO.select_edges({"q": q}, "q", 0, 2 * edges)
    assert 40 < len(want) < 200
    buf = gpu.DeviceBuffer.from_host(H.pack(F, q))
    if mb:
        with gpu.tuned(vec_max_blocks=mb):
            got = dev_select(gpu, curve, buf, 0, 2 * edges)
    else:
        got = dev_select(gpu, curve, buf, 0, 2 * edges)
    assert got == want and got == sorted(got)
    assert dev_select(gpu, curve, buf, 100, 300) == CO.select_edges({"q": q}, "q", 100, 300)


# ---- masks ------------------------------------------------------------------------------------------------------------------------------------
def test_the_arithmetic_stage_reads_mask_element_7j_plus_k(gpu):
    """a mask vector that is non-zero at one element t only: arith.r0 moves at the point t % 7 by that element times what the reference
    multiplies it with, and not at all for t % 7 == 6 (the fold drops the point)"""
    curve, edges = "bn254", 5
    F = H.FR[curve]
    p, c = F.p, case(curve, edges)
    rnd = H.rng(11)
    polys = CO.share_polys(p, c["polys"], "rep3", rnd)
    views = CO.make_views(p, polys, 1, c["params"], 0, 2 * edges)
    m = views["arith"][0].m
    assert m == 4
    dev, ref = DevStages(gpu, curve, views), CO.RefStages(views)
    base = ref.arith(1, [0] * (7 * m))[0]
    seen = set()
    for t in (0, 3, 6, 8, 12, 13, 16, 7 * m - 3, 7 * m - 1):
        mask = [0] * (7 * m)
        mask[t] = rnd.randrange(1, p)
        got, want = dev.arith(1, mask), ref.arith(1, mask)
        assert got == want, t
        moved = [k for k in range(6) if got[0][k] != base[k]]
        assert moved == ([] if t % 7 == 6 else [t % 7]), t
        seen.add(t % 7)
    assert seen == set(range(7))


# ---- against the plain entry ------------------------------------------------------------------------------------------------------------------
def _plain_entry(hip, curve, cols, b, e, params, scaling, stride):
    F = H.FR[curve]
    acc = hip.honk_sumcheck_accumulate(H.CURVE_IDS[curve], cols, b, e, H.pack(F, list(params)), acc=_guarded(hip, 4 * 57), scaling=scaling, scaling_stride=stride)
    hip.bindings.sync()
    flat, out, at = _down(F, acc, 4 * 57, "plain acc"), [], 0
    for ln in R.ACC_LEN:
        out.append(flat[at:at + ln])
        at += ln
    return out


@pytest.mark.parametrize("edges,stride", [(37, 1), (66, 4)])
def test_the_protocol_0_chain_equals_the_plain_entry(gpu, edges, stride):
    """csh_vec_mul_dev as the network; the same device columns go to csh_honk_sumcheck_accumulate_dev. random_case asserts that no edge
    meets the plain skips of perm and lookup; the planted q_arith / q_delta_range skips are in both."""
    curve = "bn254"
    c = case(curve, edges)
    assert len(c["planted"]) == 4
    got, want, dev = run_case(gpu, curve, "plain", c, 0, 2 * edges, stride=stride, device_net=True, parity=False)
    assert got == _plain_entry(gpu, curve, dev.cols[0], 0, 2 * edges, c["params"], dev.scaling, stride) and got == want


def test_null_scaling_is_the_factor_one(gpu):
    curve, edges = "bn254", 6
    c = case(curve, edges)
    got, want, dev = run_case(gpu, curve, "plain", c, 0, 2 * edges, scaled=False, device_net=True)
    assert got == want and got == _plain_entry(gpu, curve, dev.cols[0], 0, 2 * edges, c["params"], None, 1)


# ---- three Rep3 parties on the device -----------------------------------------------------------------------------------------------------------
def test_three_rep3_parties_open_to_the_plain_entry(gpu):
    curve, edges = "bn254", 37
    F = H.FR[curve]
    c = case(curve, edges)
    got, want, dev = run_case(gpu, curve, "rep3", c, 0, 2 * edges, stride=4, device_net=True, parity=False)
    cols = [gpu.DeviceBuffer.from_host(H.pack(F, c["polys"][name])) for name in R.COLS]
    assert got == want and got == _plain_entry(gpu, curve, cols, 0, 2 * edges, c["params"], dev.scaling, 4)


def test_three_rep3_parties_on_a_satisfied_trace(gpu):
    """the batched round univariate of the opened shares: S(0) + S(1) = 0, not trivially"""
    curve = "bn254"
    p = H.FR[curve].p
    t = R.satisfied_trace(p)
    rnd = H.rng(21)
    betas, alphas = [rnd.randrange(1, p) for _ in range(4)], [rnd.randrange(1, p) for _ in range(10)]
    gs = R.GateSeparator(p, betas, 4)
    net = CO.Rep3Net(p, rnd, device_local_mul(gpu, curve, 1))
    views = CO.make_views(p, CO.share_polys(p, t["polys"], "rep3", rnd), 1, t["params"], 0, t["n"], gs.beta_products, gs.periodicity)
    acc = CO.run_round(net, DevStages(gpu, curve, views))
    opened = CO.open_round(net, acc)
    assert opened == CO.plain_accumulate(p, t["polys"], 0, t["n"], gs.beta_products, gs.periodicity, t["params"])
    for s, a in enumerate(opened):
        assert (a[0] + a[1]) % p == 0 if s == R.LINEARLY_DEPENDENT else (a[0] == 0 and a[1] == 0), R.SUBRELATIONS[s]
    S = net.open([CO.batch_over_relations_shares(p, acc[i], 2, CO.pub_comp(1, i), alphas, gs.current_element(), gs.partial_evaluation_result) for i in range(3)])
    assert (S[0] + S[1]) % p == 0 and any(S[2:])


# ---- shifted columns ------------------------------------------------------------------------------------------------------------------------
def test_shifted_columns_as_an_offset_into_a_longer_vector(gpu):
    """round 0: the shifted witness columns passed as `ptr + 1 share` of vectors of n + 1 shares"""
    curve, edges = "bn254", 9
    F = H.FR[curve]
    p, n = F.p, 2 * edges
    c = case(curve, edges)
    r = H.rng(66)
    polys = {k: list(v) for k, v in c["polys"].items()}
    long = {k: polys[k] + [r.randrange(1, p)] for k in R.WITNESS[:5]}
    for k in long:
        polys[k + "_shift"] = long[k][1:]
    rnd = H.rng(67)
    net = CO.Rep3Net(p, rnd)
    shared_long = CO.share_polys(p, long, "rep3", rnd)
    party_polys = []
    for i in range(3):
        d = {k: v for k, v in polys.items() if k not in CO.SHARED}
        for k in R.WITNESS[5:]:
            d[k] = [x for v in polys[k] for x in ((v, 0) if i == 0 else (0, v) if i == 1 else (0, 0))]     # the trivial sharing
        for k in long:
            d[k], d[k + "_shift"] = shared_long[i][k][:2 * n], shared_long[i][k][2:]
        party_polys.append(d)
    views = CO.make_views(p, party_polys, 1, c["params"], 0, n)
    cols = []
    for i in range(3):
        bufs = {k: gpu.DeviceBuffer.from_host(H.pack(F, shared_long[i][k])) for k in long}
        row = []
        for name in R.COLS:
            if name in bufs:
                row.append(bufs[name])
            elif name.endswith("_shift"):
                row.append(bufs[name[:-6]].ptr.value + 64)
            else:
                row.append(gpu.DeviceBuffer.from_host(H.pack(F, party_polys[i][name])))
        cols.append(row)
    dev = DevStages(gpu, curve, views, cols)
    dev.keep = cols
    got = CO.open_round(net, CO.run_round(net, CO.Both(CO.RefStages(views), dev)))
    assert got == CO.plain_accumulate(p, polys, 0, n, None, 1, c["params"])
