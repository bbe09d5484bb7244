"""Device tests of csh_honk_sumcheck_accumulate_gates_dev (csrc/honk_gates.hip), the elliptic, memory, non-native field and Poseidon2
relations of the sumcheck round, against tests/honk_gates_ref.py, and the sumcheck identities of a satisfied trace with every gate kind
through device entries only (both accumulate entries, csh_honk_pow_table_dev, csh_mle_fold_dev of the 41 columns between rounds). Every
comparison is exact on all 110 values; every output has guard words behind it. The data is random (unsatisfied), so that every term is
non-zero, with edges planted for each of the five skips."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import helpers as H
from tests import honk_gates_ref as G
from tests import honk_relations_ref as R

pytestmark = pytest.mark.gpu
CURVES = ["bn254", "bls12_381", "bls12_377"]
GUARD = np.uint64(0x5A5AC3C3A5A53C3C)
sz = C.c_size_t


def _up(hip, arr):
    return hip.DeviceBuffer.from_host(arr)


def _cols(hip, F, polys, names=G.COLS):
    return [_up(hip, H.pack(F, polys[c])) for c in names]


def _down(F, buf, elems):
    """-> the elements, after checking the guard behind them; strict: every element canonical"""
    raw = buf.to_host()
    assert raw.size == 4 * elems + 8 and (raw[4 * elems:] == GUARD).all(), "written past the end of acc"
    return H.unpack(F, raw[:4 * elems])


def dev_accumulate(hip, curve, cols, b, e, params, scaling=None, stride=1):
    F = H.FR[curve]
    acc = _up(hip, np.full(4 * 110 + 8, GUARD, dtype=np.uint64))
    hip.honk_sumcheck_accumulate_gates(H.CURVE_IDS[curve], cols, b, e, H.pack(F, list(params)), acc=acc, scaling=scaling, scaling_stride=stride)
    hip.bindings.sync()
    return G.split_acc(_down(F, acc, 110))


def dev_pow_table(hip, curve, betas):
    F, m = H.FR[curve], len(betas)
    buf = _up(hip, np.full((4 << m) + 8, GUARD, dtype=np.uint64))
    hip.honk_pow_table(H.CURVE_IDS[curve], H.pack(F, betas) if m else None, out=buf)
    return buf


def same(got, want, what):
    for name, g, w in zip(G.SUBRELATIONS, got, want):
        assert g == w, (what, name)


@functools.lru_cache(maxsize=None)
def case(curve, n, seed=0):
    """a random case and its betas"""
    p = H.FR[curve].p
    c = G.random_case(p, n, 2000 * n + seed)
    r = H.rng(n + 19)
    c["betas"] = [r.randrange(1, p) for _ in range(13)]
    return c


@functools.lru_cache(maxsize=None)
def want(curve, n, b, e, m, stride):
    """the restatement's accumulators, computed once per range; m = the number of betas of the table, or -1 for no scaling"""
    p, c = H.FR[curve].p, case(curve, n)
    table = R.beta_products(p, c["betas"], m) if m >= 0 else None
    return G.accumulate_range(p, c["polys"], b, e, table, stride, c["params"])


def table_log(n, stride):
    return max(1, ((n // 2 - 1) * stride).bit_length())


def check_range(hip, curve, n, b, e, stride=1, scaled=True, what=None):
    c = case(curve, n)
    m = table_log(n, stride) if scaled else -1
    table = dev_pow_table(hip, curve, c["betas"][:m]) if scaled else None
    cols = _cols(hip, H.FR[curve], c["polys"])
    same(dev_accumulate(hip, curve, cols, b, e, c["params"], table, stride), want(curve, n, b, e, m, stride), (what, n, b, e, stride))


# The smallest shapes at which the kernels can go wrong: one, two and three edges; the disabled-rows call [12, 16) of 16; 35, 36 and 37
# edges around one pass of the Poseidon2 group's 36 edges (its lanes of one point, 36 k .. 36 k + 35, straddle two waves); 42 and 43 edges
# around one pass of the other two groups' 42; 257 edges, several passes of either
SHAPES = [(2, 0, 2), (4, 0, 4), (6, 0, 6), (16, 12, 16), (70, 0, 70), (72, 0, 72), (74, 0, 74), (84, 0, 84), (86, 0, 86), (514, 0, 514)]


@pytest.mark.parametrize("n,b,e", SHAPES)
def test_ranges_on_bn254(gpu, n, b, e):
    check_range(gpu, "bn254", n, b, e)


@pytest.mark.parametrize("curve", ["bls12_381", "bls12_377"])
@pytest.mark.parametrize("n,b,e", [(2, 0, 2), (86, 0, 86)])
def test_one_edge_and_43_edges_on_the_other_fields(gpu, curve, n, b, e):
    check_range(gpu, curve, n, b, e)


@pytest.mark.parametrize("curve", CURVES)
def test_capped_grids(gpu, curve):
    """2^11 edges with one and three workgroups: 49 and 17 grid-stride passes of 42 edges, 57 and 19 of 36, with a ragged last one;
    scaling_stride 2"""
    for mb in (1, 3):
        with gpu.tuned(vec_max_blocks=mb):
            check_range(gpu, curve, 4096, 0, 4096, stride=2, what=mb)


def test_null_scaling_is_the_factor_one(gpu):
    check_range(gpu, "bn254", 16, 0, 2, scaled=False)      # compute_virtual_contribution


def test_planted_edges_skipped_ones_add_nothing_and_one_end_edges_are_counted(gpu):
    """For each of the five selectors one edge where it is zero at both ends (left out) and one where it is zero at the first end only
    (counted). Every selector multiplies its whole relation, so a skipped edge would have added zeros; what the comparison must tell
    apart is a skip that fires too eagerly, and it can: every one-end edge adds a non-zero value to every subrelation of its relation."""
    curve, n = "bn254", 86
    p, c = H.FR[curve].p, case(curve, n)
    assert sorted(c["planted"]) == sorted(G.PLANTS)
    m = table_log(n, 1)
    table = R.beta_products(p, c["betas"], m)
    for name, e in c["planted"].items():
        rel, kind = name.split(".")
        sf = R.scaling_of(p, e, table, 1)
        counted = G.edge_contribution(p, c["polys"], e, c["params"], sf, rel)
        unskipped = G.edge_contribution(p, c["polys"], e, c["params"], sf, rel, honour_skip=False)
        assert counted == unskipped, name
        if kind == "one_end":
            assert all(any(a) for a in counted), name
            assert not any(any(a) for a in G.edge_contribution(p, c["polys"], e, c["params"], sf, rel, eager_skip=True))
        else:
            assert not any(any(a) for a in counted), name
    with_skips = want(curve, n, 0, n, m, 1)
    eager = G.accumulate_range(p, c["polys"], 0, n, table, 1, c["params"], eager_skip=True)
    assert all(a != b for a, b in zip(with_skips, eager)), "a too eager skip changes every one of the seventeen accumulators"
    check_range(gpu, curve, n, 0, n)
    # one planted edge alone, through the device
    cols = _cols(gpu, H.FR[curve], c["polys"])
    for name, e in c["planted"].items():
        rel, kind = name.split(".")
        got = dev_accumulate(gpu, curve, cols, e, e + 2, c["params"])
        same(got, G.accumulate_range(p, c["polys"], e, e + 2, None, 1, c["params"]), name)
        assert all(any(got[s]) == (kind == "one_end") for s in G.RELATION_OF[rel]), name


def test_adjacent_ranges_add_up_to_their_union(gpu):
    """fixes the range arithmetic (edge_begin in the column index and in the scaling index) independently of the restatement"""
    curve, n = "bn254", 86
    F, c = H.FR[curve], case(curve, n)
    p = F.p
    table = dev_pow_table(gpu, curve, c["betas"][:table_log(n, 2)])
    cols = _cols(gpu, F, c["polys"])
    whole = dev_accumulate(gpu, curve, cols, 0, n, c["params"], table, 2)
    for cut in (2, 72, 84):
        lo, hi = dev_accumulate(gpu, curve, cols, 0, cut, c["params"], table, 2), dev_accumulate(gpu, curve, cols, cut, n, c["params"], table, 2)
        assert [[(x + y) % p for x, y in zip(a, b)] for a, b in zip(lo, hi)] == whole, cut


# ---- the closed chain through device entries only -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
def test_satisfied_trace_through_device_entries_only(gpu, curve):
    """six rounds of both accumulate entries and the fold of the 41 distinct columns. Round 0: entries 0 and 1 of every accumulator but
    lookup.r1 are zero; every round: S'(0) + S'(1) = S(u), S batched over all 28 accumulators with 27 alphas."""
    hip, F, cid = gpu, H.FR[curve], H.CURVE_IDS[curve]
    p, t = F.p, G.satisfied_trace(F.p)
    n = t["n"]
    state = {"cols": dict(zip(G.ALL_COLS, _cols(hip, F, t["polys"], G.ALL_COLS))), "size": n}
    r = H.rng(44)
    betas, alphas, us = ([r.randrange(1, p) for _ in range(k)] for k in (6, G.NUM_ALPHAS, 6))
    table = dev_pow_table(hip, curve, betas)
    base_params = H.pack(F, list(t["params"]))

    def acc_of(rnd, size, gs):
        assert size == state["size"]
        cols = state["cols"]
        acc = _up(hip, np.full(4 * 57 + 8, GUARD, dtype=np.uint64))
        hip.honk_sumcheck_accumulate(cid, [cols[c] for c in R.COLS], 0, size, base_params, acc=acc, scaling=table, scaling_stride=gs.periodicity)
        gates = dev_accumulate(hip, curve, [cols[c] for c in G.COLS], 0, size, t["gate_params"], table, gs.periodicity)
        flat, base, at = _down(F, acc, 57), [], 0
        for ln in R.ACC_LEN:
            base.append(flat[at:at + ln])
            at += ln
        return base + gates

    def fold_all(u):
        half = state["size"] // 2
        outs = [hip.DeviceBuffer(32 * half) for _ in G.ALL_COLS]
        hip.mle_fold(cid, [state["cols"][c] for c in G.ALL_COLS], H.pack(F, [u]), 1, state["size"], outs)
        hip.bindings.sync()
        state["cols"], state["size"] = dict(zip(G.ALL_COLS, outs)), half

    G.check_round_chain_all(p, n, betas, alphas, us, acc_of, fold_all)
