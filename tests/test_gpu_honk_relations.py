"""Device tests of the sumcheck-round entries (csrc/honk_relations.hip): csh_honk_sumcheck_accumulate_dev and csh_honk_pow_table_dev
against tests/honk_relations_ref.py, and the sumcheck identities of a satisfied trace through device entries only (Oink entries and scans
for z_perm and the inverses, csh_mle_fold_dev between rounds). Every comparison is exact on all 57 values; every output has guard words
behind it. The data is random (unsatisfied), so that every term is non-zero, with edges planted for each skip predicate."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import helpers as H
from tests import honk_relations_ref as R

pytestmark = pytest.mark.gpu
CURVES = ["bn254", "bls12_381", "bls12_377"]
GUARD = np.uint64(0x5A5AC3C3A5A53C3C)
sz = C.c_size_t


def _up(hip, arr):
    return hip.DeviceBuffer.from_host(arr)


def _cols(hip, F, polys):
    return [_up(hip, H.pack(F, polys[c])) for c in R.COLS]


def _acc_buf(hip):
    return _up(hip, np.full(4 * 57 + 8, GUARD, dtype=np.uint64))


def _acc_down(F, buf):
    """-> the eleven accumulators, after checking the guard behind the 57 elements; strict: every element canonical"""
    raw = buf.to_host()
    assert raw.size == 4 * 57 + 8 and (raw[4 * 57:] == GUARD).all(), "written past the end of acc"
    flat, acc, at = H.unpack(F, raw[:4 * 57]), [], 0
    for ln in R.ACC_LEN:
        acc.append(flat[at:at + ln])
        at += ln
    return acc


def dev_accumulate(hip, curve, cols, b, e, params, scaling=None, stride=1):
    F = H.FR[curve]
    acc = hip.honk_sumcheck_accumulate(H.CURVE_IDS[curve], cols, b, e, H.pack(F, list(params)), acc=_acc_buf(hip), scaling=scaling, scaling_stride=stride)
    hip.bindings.sync()
    return _acc_down(F, acc)


def dev_pow_table(hip, curve, betas):
    """-> (the DeviceBuffer, its 2^m elements), after checking the guard behind them"""
    F, m = H.FR[curve], len(betas)
    buf = _up(hip, np.full((4 << m) + 8, GUARD, dtype=np.uint64))
    hip.honk_pow_table(H.CURVE_IDS[curve], H.pack(F, betas) if m else None, out=buf)
    hip.bindings.sync()
    raw = buf.to_host()
    assert (raw[4 << m:] == GUARD).all(), "written past the end of the table"
    return buf, H.unpack(F, raw[:4 << m])


def same(got, want, what):
    for name, g, w in zip(R.SUBRELATIONS, got, want):
        assert g == w, (what, name)


@functools.lru_cache(maxsize=None)
def case(curve, n, seed=0):
    """a random case, its betas, and (computed once per range) the restatement's accumulators"""
    p = H.FR[curve].p
    c = R.random_case(p, n, 1000 * n + seed)
    r = H.rng(n + 17)
    c["betas"] = [r.randrange(1, p) for _ in range(13)]
    return c


@functools.lru_cache(maxsize=None)
def want(curve, n, b, e, m, stride):
    """m = the number of betas of the table, or -1 for no scaling"""
    p, c = H.FR[curve].p, case(curve, n)
    table = R.beta_products(p, c["betas"], m) if m >= 0 else None
    return R.accumulate_range(p, c["polys"], b, e, table, stride, c["params"])


def table_log(n, stride):
    return max(1, ((n // 2 - 1) * stride).bit_length())


def check_range(hip, curve, n, b, e, stride=1, scaled=True, what=None):
    c = case(curve, n)
    m = table_log(n, stride) if scaled else -1
    table = dev_pow_table(hip, curve, c["betas"][:m])[0] if scaled else None
    cols = _cols(hip, H.FR[curve], c["polys"])
    same(dev_accumulate(hip, curve, cols, b, e, c["params"], table, stride), want(curve, n, b, e, m, stride), (what, n, b, e, stride))


# the smallest shapes at which the kernel can go wrong: one edge; 2 and 3 edges; the disabled-rows call [12, 16) of 16; 65 and 66 edges,
# across a wave; 257 edges, across a workgroup's 42 edges per pass several times over and across 256; 41, 42 and 43 edges, around one pass
SHAPES = [(2, 0, 2), (4, 0, 4), (6, 0, 6), (16, 12, 16), (130, 0, 130), (132, 0, 132), (514, 0, 514), (82, 0, 82), (84, 0, 84), (86, 0, 86)]


@pytest.mark.parametrize("n,b,e", SHAPES)
def test_ranges_on_bn254(gpu, n, b, e):
    check_range(gpu, "bn254", n, b, e)


@pytest.mark.parametrize("curve", ["bls12_381", "bls12_377"])
@pytest.mark.parametrize("n,b,e", [(2, 0, 2), (132, 0, 132)])
def test_one_edge_and_66_edges_on_the_other_fields(gpu, curve, n, b, e):
    check_range(gpu, curve, n, b, e)


@pytest.mark.parametrize("curve", CURVES)
def test_capped_grids(gpu, curve):
    """2^11 edges with one and three workgroups: 49 and 17 grid-stride passes with a ragged last one; scaling_stride 2"""
    for mb in (1, 3):
        with gpu.tuned(vec_max_blocks=mb):
            check_range(gpu, curve, 4096, 0, 4096, stride=2, what=mb)


def test_planted_skip_edges_are_left_out_and_their_contribution_is_not_zero(gpu):
    """For each skip predicate one edge where it holds at both ends (left out) and one where it holds at one end only (counted). A
    skipped permutation or lookup edge would have contributed a non-zero value, so a device that ignored the skips would differ; q_arith
    and q_delta_range multiply their whole relation, so what their skips leave out is zero by construction -- asserted as such."""
    curve, n = "bn254", 132
    p, c = H.FR[curve].p, case(curve, n)
    assert sorted(c["planted"]) == sorted(R.PLANTS)
    table = R.beta_products(p, c["betas"], table_log(n, 1))
    for name, e in c["planted"].items():
        rel, kind = name.split(".")
        sf = R.scaling_of(p, e, table, 1)
        counted = R.edge_contribution(p, c["polys"], e, c["params"], sf, rel)
        omitted = R.edge_contribution(p, c["polys"], e, c["params"], sf, rel, honour_skip=False)
        if kind == "one_end":
            assert counted == omitted and all(any(a) for a in counted), name
        else:
            assert not any(any(a) for a in counted), name
            assert any(any(a) for a in omitted) == (rel in ("perm", "lookup")), name
    with_skips = want(curve, n, 0, n, table_log(n, 1), 1)
    without = R.accumulate_range(p, c["polys"], 0, n, table, 1, c["params"], honour_skip=False)
    for s in (2, 3, 4, 6):   # perm.r0, perm.r1, lookup.r0, lookup.r2 (lookup.r1 is zero on an edge without reads and counts)
        assert with_skips[s] != without[s], R.SUBRELATIONS[s]
    check_range(gpu, curve, n, 0, n)
    # one planted edge alone, through the device: the skipped ones give 57 zeros for their relation
    cols = _cols(gpu, H.FR[curve], c["polys"])
    for name in ("perm.skip", "lookup.skip"):
        e = c["planted"][name]
        got = dev_accumulate(gpu, curve, cols, e, e + 2, c["params"])
        same(got, R.accumulate_range(p, c["polys"], e, e + 2, None, 1, c["params"]), name)
        assert all(not any(got[s]) for s in R.RELATION_OF[name.split(".")[0]])


@pytest.mark.parametrize("stride", [1, 2, 8])
def test_scaling_strides_read_the_table_where_the_reference_reads_it(gpu, stride):
    check_range(gpu, "bn254", 64, 0, 64, stride=stride)


def test_null_scaling_is_the_factor_one(gpu):
    check_range(gpu, "bn254", 16, 0, 2, scaled=False)      # compute_virtual_contribution
    check_range(gpu, "bn254", 132, 0, 132, scaled=False)


def test_shifted_columns_as_an_offset_into_a_longer_vector(gpu):
    """round 0: the shifted witness columns passed as `ptr + 1 element` of vectors of n + 1 elements"""
    curve, n = "bn254", 66
    F = H.FR[curve]
    r = H.rng(66)
    polys = {c: [r.randrange(1, F.p) for _ in range(n)] for c in R.COLS}
    long = {c: polys[c] + [r.randrange(1, F.p)] for c in R.WITNESS[:5]}
    for c in R.WITNESS[:5]:
        polys[c + "_shift"] = long[c][1:]
    params = tuple(r.randrange(1, F.p) for _ in range(3))
    bufs = {c: _up(gpu, H.pack(F, long[c])) for c in long}
    cols = []
    for c in R.COLS:
        if c in long:
            cols.append(bufs[c])
        elif c.endswith("_shift"):
            cols.append(bufs[c[:-6]].ptr.value + 32)
        else:
            cols.append(_up(gpu, H.pack(F, polys[c])))
    same(dev_accumulate(gpu, curve, cols, 0, n, params), R.accumulate_range(F.p, polys, 0, n, None, 1, params), "offset")


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("m", [0, 1, 2, 7, 13])
def test_pow_table(gpu, curve, m):
    F = H.FR[curve]
    r = H.rng(100 + m)
    betas = [F.p - 1 if b == 1 else r.randrange(F.p) for b in range(m)]
    assert dev_pow_table(gpu, curve, betas)[1] == R.beta_products(F.p, betas, m)


def test_adjacent_ranges_add_up_to_their_union(gpu):
    """fixes the range arithmetic (edge_begin in the column index and in the scaling index) independently of the restatement"""
    curve, n = "bn254", 132
    F, c = H.FR[curve], case(curve, n)
    p = F.p
    table = dev_pow_table(gpu, curve, c["betas"][:table_log(n, 2)])[0]
    cols = _cols(gpu, F, c["polys"])
    whole = dev_accumulate(gpu, curve, cols, 0, n, c["params"], table, 2)
    for cut in (2, 84, 130):
        lo, hi = dev_accumulate(gpu, curve, cols, 0, cut, c["params"], table, 2), dev_accumulate(gpu, curve, cols, cut, n, c["params"], table, 2)
        assert [[(x + y) % p for x, y in zip(a, b)] for a, b in zip(lo, hi)] == whole, cut


# ---- the closed chain through device entries only -----------------------------------------------------------------------------------------
def _mul(hip, cid, x, y, n):
    out = hip.DeviceBuffer(32 * n)
    assert hip.lib().csh_vec_mul_dev(cid, x.ptr, y.ptr, out.ptr, sz(n), None) == 0
    return out


@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
def test_satisfied_trace_through_device_entries_only(gpu, curve):
    """z_perm from perm operands -> products -> prefix products -> batch inverse -> placement, the inverses from the lookup operands ->
    product -> batch inverse, as the Oink closed chains; then four rounds of accumulate + fold. Round 0: entries 0 and 1 of every
    accumulator but lookup.r1 are zero; every round: S'(0) + S'(1) = S(u)."""
    hip, F, cid = gpu, H.FR[curve], H.CURVE_IDS[curve]
    p, t = F.p, R.satisfied_trace(H.FR[curve].p)
    n, polys, (beta, gamma, _) = t["n"], t["polys"], t["params"]
    ch = H.pack(F, [beta, gamma])
    zeros = lambda k: _up(hip, np.zeros(4 * k, dtype=np.uint64))
    # the witness columns with one zero element behind them: the shifted columns of round 0 are `ptr + 1 element`
    wit = {c: _up(hip, H.pack(F, polys[c] + [0])) for c in ("w_l", "w_r", "w_o", "w_4")}
    pre = {c: _up(hip, H.pack(F, polys[c])) for c in R.PRECOMPUTED}
    m = t["last"]
    ops = hip.honk_perm_operands(cid, 0, 0, [wit[c] for c in ("w_l", "w_r", "w_o", "w_4")], [pre["id_%d" % k] for k in range(1, 5)] + [pre["sigma_%d" % k] for k in range(1, 5)],
                                 n, m + 1, None, ch, [hip.DeviceBuffer(32 * m) for _ in range(8)])
    num = hip.vec_prefix_prod(cid, _mul(hip, cid, _mul(hip, cid, ops[0], ops[1], m), _mul(hip, cid, ops[2], ops[3], m), m), m)
    den, _ = hip.vec_batch_inverse(cid, hip.vec_prefix_prod(cid, _mul(hip, cid, _mul(hip, cid, ops[4], ops[5], m), _mul(hip, cid, ops[6], ops[7], m), m), m), m)
    z = hip.honk_z_perm_place(cid, 0, 0, _mul(hip, cid, num, den, m), zeros(n + 1), n, m + 1, None)
    tags, counts = _up(hip, H.pack(F, polys["lookup_read_tags"])), _up(hip, H.pack(F, polys["lookup_read_counts"]))
    prod, sel = hip.honk_lookup_operands(cid, 0, 0, [wit["w_l"], wit["w_r"], wit["w_o"], tags],
                                         [pre[c] for c in ("q_r", "q_m", "q_c", "q_o", "table_1", "table_2", "table_3", "table_4", "q_lookup")], n, ch,
                                         [hip.DeviceBuffer(32 * n) for _ in range(2)])
    inv, _ = hip.vec_batch_inverse(cid, _mul(hip, cid, prod, sel, n), n)
    hip.bindings.sync()
    assert H.unpack(F, z.to_host())[:n] == polys["z_perm"] and H.unpack(F, inv.to_host()) == polys["lookup_inverses"]
    witness = {"w_l": wit["w_l"], "w_r": wit["w_r"], "w_o": wit["w_o"], "w_4": wit["w_4"], "z_perm": z, "lookup_inverses": inv,
               "lookup_read_counts": counts, "lookup_read_tags": tags}
    state = {"cols": [witness[c] if c in witness else (witness[c[:-6]].ptr.value + 32 if c.endswith("_shift") else pre[c]) for c in R.COLS], "size": n}
    r = H.rng(43)
    betas, alphas, us = ([r.randrange(1, p) for _ in range(k)] for k in (4, 10, 4))
    table, table_host = dev_pow_table(hip, curve, betas)
    assert table_host == R.beta_products(p, betas, 4)

    def acc_of(rnd, size, gs):
        assert size == state["size"]
        return dev_accumulate(hip, curve, state["cols"], 0, size, t["params"], table, gs.periodicity)

    def fold_all(u):
        half = state["size"] // 2
        outs = [hip.DeviceBuffer(32 * half) for _ in R.COLS]
        ins = state["cols"]
        if not isinstance(ins[0], hip.DeviceBuffer):
            raise AssertionError("column 0 is a buffer")
        hip.mle_fold(cid, ins, H.pack(F, [u]), 1, state["size"], outs)
        hip.bindings.sync()
        state["cols"], state["size"], state["keep"] = outs, half, ins

    R.check_round_chain(p, n, betas, alphas, us, acc_of, fold_all)
