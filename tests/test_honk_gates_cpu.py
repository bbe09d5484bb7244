"""CPU tests of csh_honk_sumcheck_accumulate_gates_dev (csrc/honk_gates.hip), the elliptic, memory, non-native field and Poseidon2
relations of the sumcheck round: the restatement tests/honk_gates_ref.py against itself (the prover's univariate shape against the
verifier's scalar shape at all seven points), a satisfied trace with every gate kind in closed form through all six rounds on all 28
accumulators, the arithmetic run on the host through csh_selftest_honk_gates_host -- the argument builder and the per-point functions the
gfx950 kernels call, with the limb-bound contract checks of selftest.hip on (a violated bound aborts the process) -- and the C boundary
without a device. Every comparison is exact and covers all 110 values."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import helpers as H
from tests import honk_gates_ref as G
from tests import honk_relations_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVES = ["bn254", "bls12_381", "bls12_377"]
NO_DEVICE, INVALID = -2, -1
CITES = ["sumcheck_round_prover.rs:224-255", ":340-386", ":388-421", ":160-222", "relations/mod.rs:134-145", "elliptic_relation.rs:81-161",
         "memory_relation.rs:145-358", "non_native_field_relation.rs:85-177", "poseidon2_external_relation.rs:121-205",
         "poseidon2_internal_relation.rs:118-200", "memory_relation.rs:347-353"]
sz = C.c_size_t
FILL = np.uint64(0xA5A5A5A5A5A5A5A5)


def _p(x):
    return x.ctypes.data_as(C.c_void_p) if x is not None else None


def _ptrs(arrs):
    return (C.c_void_p * len(arrs))(*[a.ctypes.data if a is not None else None for a in arrs])


def host_accumulate(hip, curve, polys, edge_begin, edge_end, scaling, stride, params):
    """the kernels' functions on host arrays -> the seventeen accumulators"""
    F = H.FR[curve]
    cols = [H.pack(F, polys[c]) for c in G.COLS]
    sc = H.pack(F, scaling) if scaling is not None else None
    out = np.full(4 * 110 + 8, FILL, dtype=np.uint64)
    rc = hip.lib().csh_selftest_honk_gates_host(H.CURVE_IDS[curve], _ptrs(cols), sz(edge_begin), sz(edge_end), _p(sc), sz(stride),
                                                _p(H.pack(F, list(params))), _p(out))
    assert rc == 0 and (out[4 * 110:] == FILL).all()
    return G.split_acc(H.unpack(F, out[:4 * 110]))   # strict: canonical


# ---- the restatement against itself ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_scalar_shape_equals_univariate_shape_at_every_point(curve):
    """verify_accumulate on the extended values at the point k = entry k of accumulate's univariates, for all seven points"""
    p = H.FR[curve].p
    c = G.random_case(p, 4, 78, plants=False)
    sf = 0x7654321 % p
    for edge_idx in (0, 2):
        e = G.extend_edges(p, c["polys"], edge_idx)
        uni = [u for rel in G.RELATIONS for u in G.ACCUMULATE[rel](p, e, c["params"], sf)]
        assert len(uni) == 17
        for k in range(G.MAX_PARTIAL_RELATION_LENGTH):
            scalars = G.relations_at_point(p, {name: e[name].ev[k] for name in G.COLS}, c["params"], sf)
            assert scalars == [u.ev[k] for u in uni], k
            assert all(scalars), "random data: every subrelation is non-zero"


def test_every_selector_multiplies_its_whole_relation():
    """what the header states about the skips: with the selector zero at a point every subrelation of the relation is zero there, whatever
    the other columns hold -- so a skip (zero at both ends, hence at every point) omits zeros only"""
    p = H.FR["bn254"].p
    c = G.random_case(p, 2, 5, plants=False)
    v = {name: c["polys"][name][0] for name in G.COLS}
    for rel in G.RELATIONS:
        out = G.relations_at_point(p, {**v, G.SELECTOR_OF[rel]: 0}, c["params"], 12345)
        for s in range(17):
            assert (out[s] == 0) == (s in G.RELATION_OF[rel]), (rel, G.SUBRELATIONS[s])


# ---- a satisfied trace in closed form -----------------------------------------------------------------------------------------------------------
def _chain(p, seed, accumulate_gates):
    """all six rounds on the satisfied trace; the first eleven accumulators from the restatement, the other seventeen from
    accumulate_gates(polys, size, scaling, stride, params)"""
    t = G.satisfied_trace(p)
    r = H.rng(seed)
    n = t["n"]
    betas, alphas, us = ([r.randrange(1, p) for _ in range(k)] for k in (6, G.NUM_ALPHAS, 6))
    state = {"polys": {c: list(v) for c, v in t["polys"].items()}}

    def acc_of(rnd, size, gs):
        base = R.accumulate_range(p, state["polys"], 0, size, gs.beta_products, gs.periodicity, t["params"])
        return base + accumulate_gates(state["polys"], size, gs.beta_products, gs.periodicity, t["gate_params"])

    def fold_all(u):
        state["polys"] = {c: R.fold(p, v, u) for c, v in state["polys"].items()}

    G.check_round_chain_all(p, n, betas, alphas, us, acc_of, fold_all)


@pytest.mark.parametrize("curve", CURVES)
def test_satisfied_trace_through_all_rounds_on_the_restatement(curve):
    p = H.FR[curve].p
    t = G.satisfied_trace(p)
    polys = t["polys"]
    assert sorted(t["rows"]) == sorted(G.GATE_KINDS) and t["n"] == 64
    for rel, sel in G.SELECTOR_OF.items():      # every relation has its gates, each followed by a row without selectors
        rows = [i for i, v in enumerate(polys[sel]) if v]
        assert rows == sorted(g for kind, g in t["rows"].items() if kind.split(".")[0] == rel) and rows
        assert all(not any(polys[s][g + 1] for s in G.SELECTORS) for g in rows)
    g = t["rows"]["elliptic.sub"]
    assert polys["q_l"][g] == p - 1 and polys["q_l"][t["rows"]["elliptic.add"]] == 1 and polys["q_m"][t["rows"]["elliptic.double"]] == 1
    x, y = polys["w_r"][g], polys["w_o"][g]
    assert (y * y - x * x * x - t["gate_params"][3]) % p == 0, "a point of the curve"
    if curve == "bn254":
        assert t["gate_params"][3] == p - 17
    _chain(p, 51, lambda polys, size, sc, stride, params: G.accumulate_range(p, polys, 0, size, sc, stride, params))


@pytest.mark.parametrize("curve", CURVES)
def test_satisfied_trace_through_all_rounds_on_the_host_kernels(hip, curve):
    """the same chain with the seventeen accumulators from the kernels' per-point functions (folds in Python integers)"""
    p = H.FR[curve].p
    _chain(p, 52, lambda polys, size, sc, stride, params: host_accumulate(hip, curve, polys, 0, size, sc, stride, params))


# ---- the kernels' own functions on the host ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_host_kernels_match_the_restatement_on_random_data_with_planted_skips(hip, curve):
    p = H.FR[curve].p
    c = G.random_case(p, 24, 501)
    assert len(c["planted"]) == 10
    betas = [H.rng(10).randrange(1, p) for _ in range(5)]
    table = R.beta_products(p, betas, 5)
    for (b, e, sc, stride) in ((0, 24, table, 2), (0, 24, None, 1), (20, 24, table, 1), (0, 2, None, 1), (2, 8, table, 4)):
        want = G.accumulate_range(p, c["polys"], b, e, sc, stride, c["params"])
        assert host_accumulate(hip, curve, c["polys"], b, e, sc, stride, c["params"]) == want, (b, e, stride)
    # a skip omits zeros only; a skip that fires on zero at one end changes every accumulator
    full = G.accumulate_range(p, c["polys"], 0, 24, table, 2, c["params"])
    assert full == G.accumulate_range(p, c["polys"], 0, 24, table, 2, c["params"], honour_skip=False)
    eager = G.accumulate_range(p, c["polys"], 0, 24, table, 2, c["params"], eager_skip=True)
    assert all(a != b for a, b in zip(full, eager))


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("fill", ["0", "1", "p-1"])
def test_host_kernels_at_the_edges_of_the_field(hip, curve, fill):
    """every column, scaling factor and parameter 0, 1 or p - 1 at both ends, and mixed with random at the other end; many passes of p - 1
    through one lane's running sums; bound checks on"""
    p = H.FR[curve].p
    v = {"0": 0, "1": 1, "p-1": p - 1}[fill]
    r = H.rng(8)
    n = 64
    polys = {c: [v] * n for c in G.COLS}
    for c in G.COLS:            # the second half: the edge value at one end, random at the other
        for i in range(n // 2, n):
            if (i + len(c)) % 2:
                polys[c][i] = r.randrange(p)
    params = (v,) * 8
    scaling = [v if v else 1] * (n // 2)
    want = G.accumulate_range(p, polys, 0, n, scaling, 1, params)
    assert any(any(a) for a in want)
    assert host_accumulate(hip, curve, polys, 0, n, scaling, 1, params) == want


# ---- the C boundary without a device -----------------------------------------------------------------------------------------------------
def _call(L, cols, b, e, scaling, stride, params, acc, f=0):
    return L.csh_honk_sumcheck_accumulate_gates_dev(f, cols, sz(b), sz(e), scaling, sz(stride), params, acc, None)


def test_refusals_come_before_the_device(hip):
    L = hip.lib()
    err = lambda: L.csh_last_error()
    n = 16
    cols = [np.zeros(4 * n, dtype=np.uint64) for _ in range(19)]
    acc, par, table = np.zeros(4 * 110, dtype=np.uint64), np.ones(32, dtype=np.uint64), np.zeros(4 * n, dtype=np.uint64)
    good = lambda **kw: _call(L, **{**dict(cols=_ptrs(cols), b=0, e=n, scaling=_p(table), stride=1, params=_p(par), acc=_p(acc)), **kw})
    for f in (2, 9):
        assert good(f=f) == INVALID and b"field_of" in err()
    for b, e in ((1, 4), (0, 3), (4, 4), (6, 2), (0, 0), (0, (1 << 28) + 2)):   # odd, empty, reversed, too long
        assert good(b=b, e=e) == INVALID and b"even" in err(), (b, e)
    nulls = [good(cols=None), good(params=None), good(acc=None)] + [good(cols=_ptrs(cols[:i] + [None] + cols[i + 1:])) for i in range(19)]
    for rc in nulls:
        assert rc == INVALID and b"NULL" in err()
    for stride in (0, (1 << 28) + 1):
        assert good(stride=stride) == INVALID and b"scaling_stride" in err()
    # acc on a column's elements that are read, on the scaling elements that are read; right behind them is no overlap
    big = np.zeros(4 * (n + 110), dtype=np.uint64)
    assert good(cols=_ptrs(cols[:18] + [big]), acc=_p(big[4 * (n - 1):])) == INVALID and b"overlaps an input" in err()
    assert good(cols=_ptrs([big] + cols[1:]), b=4, e=8, acc=_p(big[4 * 7:])) == INVALID and b"overlaps an input" in err()
    assert good(scaling=_p(big), stride=2, acc=_p(big[4 * 14:])) == INVALID and b"overlaps an input" in err()
    ok = [good(cols=_ptrs(cols[:18] + [big]), acc=_p(big[4 * n:])), good(cols=_ptrs([big] + cols[1:]), b=4, e=8, acc=_p(big[4 * 8:])),
          good(scaling=_p(big), stride=2, acc=_p(big[4 * 15:])), good(scaling=None, stride=0)]
    if not hip.have_device():
        assert ok == [NO_DEVICE] * 4   # valid calls: they get as far as asking for a device, and there is no CPU path


def test_the_wrapper_checks_the_column_count_the_parameter_count_and_the_range(hip):
    cols = [1 << 20] * 19
    par = np.ones(32, dtype=np.uint64)
    for bad in (cols[:18], cols + cols[:1], [1 << 20] * 36):
        with pytest.raises(hip.CoSnarksHipError, match="columns"):
            hip.honk_sumcheck_accumulate_gates(0, bad, 0, 2, par, acc=1 << 21)
    for bad in (par[:12], par[:28], np.ones(36, dtype=np.uint64)):
        with pytest.raises(hip.CoSnarksHipError, match="parameter"):
            hip.honk_sumcheck_accumulate_gates(0, cols, 0, 2, bad, acc=1 << 21)
    for b, e in ((1, 4), (0, 3), (2, 2), (0, (1 << 28) + 2), (-2, 2)):
        with pytest.raises(hip.CoSnarksHipError, match="even"):
            hip.honk_sumcheck_accumulate_gates(0, cols, b, e, par, acc=1 << 21)
    with pytest.raises(hip.CoSnarksHipError, match="scaling_stride"):
        hip.honk_sumcheck_accumulate_gates(0, cols, 0, 2, par, acc=1 << 21, scaling=1 << 22, scaling_stride=0)


# ---- ABI text audits ----------------------------------------------------------------------------------------------------------------------------
def test_header_bindings_and_sys_crate_declare_the_entry_point(hip):
    import re

    from cosnarks_amd import bindings
    name = "csh_honk_sumcheck_accumulate_gates_dev"
    txt = open(bindings.header_path()).read()
    sys_rs = open(os.path.join(ROOT, "rust", "cosnarks-hip-sys", "src", "lib.rs")).read()
    L = hip.lib()
    assert name in bindings.declared_symbols() and hasattr(L, name)
    at = txt.index("int %s(" % name)
    comment = txt[txt.rindex("/*", 0, at):at]
    for c in CITES:
        assert c in comment, c
    assert "multiplies its whole" in comment and "host array of 19 device ptrs" in txt[at:at + 400] and "110 elements" in txt[at:at + 600]
    assert "pub fn %s(" % name in sys_rs
    assert hasattr(hip, "honk_sumcheck_accumulate_gates") and name in open(bindings.__file__).read()
    assert "csh_selftest_honk_gates_host" not in bindings.declared_symbols() and hasattr(L, "csh_selftest_honk_gates_host")
    # the header no longer leaves these relations with the caller
    first = txt[txt.rindex("/*", 0, txt.index("int csh_honk_sumcheck_accumulate_dev(")):txt.index("int csh_honk_sumcheck_accumulate_dev(")]
    assert "Poseidon2 relations are" in first and name in first
    # the column order of the header, the kernels' header and the restatement is one order
    flat = lambda s: [x.strip() for x in s.split(",") if x.strip()]
    w = flat(re.search(r"witness \(4\)\s+(.*?)\n", comment).group(1))
    sh = flat(re.search(r"shifted witness \(4\)\s+(.*?)\n", comment).group(1))
    pre = flat(re.search(r"precomputed \(6\)\s+(.*?)\n", comment).group(1))
    sel = flat(re.search(r"gate selectors \(5\)\s+(.*?)\n", comment).group(1))
    assert w == G.WITNESS and [x + "_shift" for x in sh] == G.SHIFTED and pre == G.PRECOMPUTED and sel == G.SELECTORS
    hpp = open(os.path.join(ROOT, "co-snarks_amd", "csrc", "honk_gates.hpp")).read()
    enum = re.search(r"enum HgCol : int \{(.*?)\};", hpp, re.S).group(1)
    assert [x.strip().split(" ")[0][3:].lower() for x in enum.split(",")] == G.COLS
    assert "honk_gates.hip" in open(os.path.join(ROOT, "co-snarks_amd", "build.py")).read()
    assert '#include "honk_relations.hpp"' in hpp


def test_rust_shim_and_mirror_call_the_entry_with_the_abi_counts():
    import re
    src = open(os.path.join(ROOT, "rust", "co-noir-hip", "src", "sumcheck.rs")).read()
    lib_rs = open(os.path.join(ROOT, "rust", "co-noir-hip", "src", "lib.rs")).read()
    for name in ("hip_compute_univariate_gates", "hip_compute_univariate_all", "gate_params"):
        assert "pub fn %s<" % name in src and name in lib_rs, name
    assert "sys::csh_honk_sumcheck_accumulate_gates_dev(" in src
    assert "pub const GATES_COLUMNS: usize = 19;" in src and "pub const GATES_ACC_ELEMS: usize = 110;" in src and "pub const GATES_PARAMS: usize = 8;" in src
    lens = re.search(r"GATES_ACC_LENGTHS: \[usize; 17\] = \[(.*?)\]", src).group(1)
    assert [int(x) for x in lens.split(",")] == G.ACC_LEN
    assert "P::get_curve_b()" in src and "POSEIDON2_BN254_T4_PARAMS.mat_internal_diag_m_1" in src
    assert "stay with the caller, who adds" not in src, "the doc comment no longer leaves the five relations with the caller"
    for cite in CITES[5:10]:
        assert cite in src, cite
    hpp = open(os.path.join(ROOT, "co-snarks_amd", "host", "plonk_honk.hpp")).read()
    for name in ("compute_round_accumulators_gates", "compute_univariate_all", "host_round_accumulators_gates", "struct HonkGateParameters"):
        assert name in hpp, name
    lens = re.search(r"HONK_GATES_ACC_LENGTHS\[HONK_GATES_SUBRELATIONS\] = \{(.*?)\}", hpp).group(1)
    assert [int(x) for x in lens.split(",")] == G.ACC_LEN and "HONK_NUM_ALPHAS = 27" in hpp
    loop = hpp[hpp.index("inline HonkGateAccumulators<Fr> host_round_accumulators_gates"):hpp.index("honk_batch_over_all_relations")]
    assert "hg_" not in loop and "honk_gates.hpp" not in hpp, "the plain C++ loop shares no code with the kernels' header"
