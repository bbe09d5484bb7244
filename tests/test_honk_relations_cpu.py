"""CPU tests of the sumcheck-round entries (csrc/honk_relations.hip: csh_honk_sumcheck_accumulate_dev, csh_honk_pow_table_dev): the
restatement tests/honk_relations_ref.py against itself (the prover's univariate shape against the verifier's scalar shape), a satisfied
trace in closed form through all four rounds, the arithmetic run on the host through csh_selftest_honk_relations_host -- the argument
builder and the per-point functions the gfx950 kernel calls, with the limb-bound contract checks of selftest.hip on (a violated bound
aborts the process) -- and the C boundary without a device. Every comparison is exact and covers all 57 values."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import helpers as H
from tests import honk_relations_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVES = ["bn254", "bls12_381", "bls12_377"]
NO_DEVICE, INVALID = -2, -1
ENTRY = {"csh_honk_sumcheck_accumulate_dev": ["sumcheck_round_prover.rs:224-255", "ultra_arithmetic_relation.rs:126-175", "permutation_relation.rs:93-167",
                                              "logderiv_lookup_relation.rs:77-183", "delta_range_constraint_relation.rs:112-177", ":340-386", ":388-421"],
         "csh_honk_pow_table_dev": ["decider/types.rs:53-67"]}
sz = C.c_size_t
FILL = np.uint64(0xA5A5A5A5A5A5A5A5)


def _p(x):
    return x.ctypes.data_as(C.c_void_p) if x is not None else None


def _ptrs(arrs):
    return (C.c_void_p * len(arrs))(*[a.ctypes.data if a is not None else None for a in arrs])


def host_accumulate(hip, curve, polys, edge_begin, edge_end, scaling, stride, params):
    """the kernel's functions on host arrays -> the eleven accumulators"""
    F = H.FR[curve]
    cols = [H.pack(F, polys[c]) for c in R.COLS]
    sc = H.pack(F, scaling) if scaling is not None else None
    out = np.full(4 * 57 + 8, FILL, dtype=np.uint64)
    rc = hip.lib().csh_selftest_honk_relations_host(H.CURVE_IDS[curve], _ptrs(cols), sz(edge_begin), sz(edge_end), _p(sc), sz(stride),
                                                    _p(H.pack(F, list(params))), _p(out))
    assert rc == 0 and (out[4 * 57:] == FILL).all()
    flat = H.unpack(F, out[:4 * 57])   # strict: canonical
    acc, at = [], 0
    for ln in R.ACC_LEN:
        acc.append(flat[at:at + ln])
        at += ln
    return acc


# ---- the restatement against itself ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_scalar_shape_equals_univariate_shape_at_every_point(curve):
    """verify_accumulate on the extended values at the point k = entry k of accumulate's univariates, for all seven points"""
    p = H.FR[curve].p
    c = R.random_case(p, 4, 77, plants=False)
    sf = 0x1234567 % p
    for edge_idx in (0, 2):
        e = R.extend_edges(p, c["polys"], edge_idx)
        uni = [u for rel in ("arith", "perm", "lookup", "delta") for u in R.ACCUMULATE[rel](p, e, c["params"], sf)]
        assert len(uni) == 11
        for k in range(R.MAX_PARTIAL_RELATION_LENGTH):
            scalars = R.relations_at_point(p, {name: e[name].ev[k] for name in R.COLS}, c["params"], sf)
            assert scalars == [u.ev[k] for u in uni], k
            assert all(scalars), "random data: every subrelation is non-zero"
    # extend_from of two points is the line through them; the general form reproduces a polynomial of its degree
    assert R.extend_from(p, [5, 3], 7) == [(5 - 2 * k) % p for k in range(7)]
    cubic = lambda x: (7 * x ** 3 + p - 2 * x * x + 11) % p
    for ln in (4, 5, 6):
        assert R.extend_from(p, [cubic(x) for x in range(ln)], 8) == [cubic(x) for x in range(8)]


def test_beta_products_are_the_products_over_the_set_bits():
    p = H.FR["bn254"].p
    betas = [3, 5, 7, 11]
    assert R.beta_products(p, betas, 0) == [1] and R.beta_products(p, betas, 3) == [1, 3, 5, 15, 7, 21, 35, 105]


# ---- a satisfied trace in closed form -----------------------------------------------------------------------------------------------------------
def _chain(p, seed, accumulate):
    """all four rounds on the satisfied trace; accumulate(polys, size, scaling, stride, params) -> the eleven accumulators"""
    t = R.satisfied_trace(p)
    r = H.rng(seed)
    n = t["n"]
    betas = [r.randrange(1, p) for _ in range(4)]
    alphas = [r.randrange(1, p) for _ in range(10)]
    us = [r.randrange(1, p) for _ in range(4)]
    state = {"polys": {c: list(v) for c, v in t["polys"].items()}}

    def acc_of(rnd, size, gs):
        return accumulate(state["polys"], size, gs.beta_products, gs.periodicity, t["params"])

    def fold_all(u):
        state["polys"] = {c: R.fold(p, v, u) for c, v in state["polys"].items()}

    R.check_round_chain(p, n, betas, alphas, us, acc_of, fold_all)


@pytest.mark.parametrize("curve", CURVES)
def test_satisfied_trace_through_all_rounds_on_the_restatement(curve):
    p = H.FR[curve].p
    t = R.satisfied_trace(p)
    w, polys = t["w"], t["polys"]
    assert sorted(set(polys["q_arith"])) == [0, 1, 2, 3] and sum(polys["q_delta_range"]) == 1 and sum(polys["q_lookup"]) == 1
    assert [(w[k + 1][5] - w[k][5]) % p for k in range(3)] + [(w[0][6] - w[3][5]) % p] == [1, 2, 3, 0]
    assert polys["z_perm"][1] == 1 and polys["z_perm"][t["last"]] == 1 and len(set(polys["z_perm"])) > 6
    assert [i for i, v in enumerate(polys["lookup_inverses"]) if v] == [7, 10]
    _chain(p, 41, lambda polys, size, sc, stride, params: R.accumulate_range(p, polys, 0, size, sc, stride, params))


@pytest.mark.parametrize("curve", CURVES)
def test_satisfied_trace_through_all_rounds_on_the_host_kernels(hip, curve):
    """the same chain with the accumulators from the kernel's per-point functions (folds in Python integers)"""
    p = H.FR[curve].p
    _chain(p, 42, lambda polys, size, sc, stride, params: host_accumulate(hip, curve, polys, 0, size, sc, stride, params))


# ---- the kernel's own functions on the host ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_host_kernels_match_the_restatement_on_random_data_with_planted_skips(hip, curve):
    p = H.FR[curve].p
    c = R.random_case(p, 24, 500)
    assert len(c["planted"]) == 8
    betas = [H.rng(9).randrange(1, p) for _ in range(5)]
    table = R.beta_products(p, betas, 5)
    for (b, e, sc, stride) in ((0, 24, table, 2), (0, 24, None, 1), (20, 24, table, 1), (0, 2, None, 1), (2, 8, table, 4)):
        want = R.accumulate_range(p, c["polys"], b, e, sc, stride, c["params"])
        assert host_accumulate(hip, curve, c["polys"], b, e, sc, stride, c["params"]) == want, (b, e, stride)
    # the skips are part of the result: without them the permutation and the lookup accumulators differ
    full = R.accumulate_range(p, c["polys"], 0, 24, table, 2, c["params"])
    unskipped = R.accumulate_range(p, c["polys"], 0, 24, table, 2, c["params"], honour_skip=False)
    assert full[2] != unskipped[2] and full[4] != unskipped[4] and full[0] == unskipped[0] and full[7:] == unskipped[7:]


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("fill", ["0", "1", "p-1"])
def test_host_kernels_at_the_edges_of_the_field(hip, curve, fill):
    """every column, scaling factor and parameter 0, 1 or p - 1 at both ends, and mixed with random at the other end; many passes of p - 1
    through one lane's running sums; bound checks on"""
    p = H.FR[curve].p
    v = {"0": 0, "1": 1, "p-1": p - 1}[fill]
    r = H.rng(7)
    n = 64
    polys = {c: [v] * n for c in R.COLS}
    for c in R.COLS:            # the second half: the edge value at one end, random at the other
        for i in range(n // 2, n):
            if (i + len(c)) % 2:
                polys[c][i] = r.randrange(p)
    polys["z_perm_shift"][0] = (v + 1) % p   # so that the all-equal edges are not all skipped by the permutation
    params = (v, v, v)
    scaling = [v if v else 1] * (n // 2)
    want = R.accumulate_range(p, polys, 0, n, scaling, 1, params)
    assert host_accumulate(hip, curve, polys, 0, n, scaling, 1, params) == want


@pytest.mark.parametrize("curve", CURVES)
def test_both_host_runs_place_every_element_where_the_restatement_has_it(hip, curve):
    """[4, 90): 43 edges, one more than a pass of 42, behind a begin offset, through both self-test entries. Random data without planted
    skips, so every one of the 57 and of the 110 elements is non-zero in the restatement: an element written to another's place cannot hide
    behind a zero. The words are compared, not the residues."""
    from tests import honk_gates_ref as G
    F = H.FR[curve]
    p, n, b, e = F.p, 90, 4, 90
    table = R.beta_products(p, [H.rng(21).randrange(1, p) for _ in range(6)], 6)
    for ref, entry, elems, seed in ((R, "csh_selftest_honk_relations_host", 57, 901), (G, "csh_selftest_honk_gates_host", 110, 902)):
        c = ref.random_case(p, n, seed, plants=False)
        flat = [v for acc in ref.accumulate_range(p, c["polys"], b, e, table, 1, c["params"]) for v in acc]
        assert len(flat) == elems and all(flat), entry
        out = np.full(4 * elems + 8, FILL, dtype=np.uint64)
        cols, sc, pr = [H.pack(F, c["polys"][name]) for name in ref.COLS], H.pack(F, table), H.pack(F, list(c["params"]))
        rc = getattr(hip.lib(), entry)(H.CURVE_IDS[curve], _ptrs(cols), sz(b), sz(e), _p(sc), sz(1), _p(pr), _p(out))
        assert rc == 0 and (out[4 * elems:] == FILL).all(), entry
        assert (out[:4 * elems] == H.pack(F, flat)).all(), entry


@pytest.mark.parametrize("curve", CURVES)
def test_pow_table_on_the_host(hip, curve):
    F = H.FR[curve]
    r = H.rng(13)
    for m in (0, 1, 2, 7):
        betas = [F.p - 1 if b == 0 else r.randrange(F.p) for b in range(m)]
        out = np.full(4 * (1 << m) + 4, FILL, dtype=np.uint64)
        rc = hip.lib().csh_selftest_honk_pow_table_host(H.CURVE_IDS[curve], _p(H.pack(F, betas)) if m else None, sz(m), _p(out))
        assert rc == 0 and (out[4 << m:] == FILL).all()
        assert H.unpack(F, out[:4 << m]) == R.beta_products(F.p, betas, m), m


# ---- the C boundary without a device -----------------------------------------------------------------------------------------------------
def _call(L, cols, b, e, scaling, stride, params, acc, f=0):
    return L.csh_honk_sumcheck_accumulate_dev(f, cols, sz(b), sz(e), scaling, sz(stride), params, acc, None)


def test_refusals_come_before_the_device(hip):
    L = hip.lib()
    err = lambda: L.csh_last_error()
    n = 16
    cols = [np.zeros(4 * n, dtype=np.uint64) for _ in range(36)]
    acc, par, table = np.zeros(4 * 57, dtype=np.uint64), np.ones(12, dtype=np.uint64), np.zeros(4 * n, dtype=np.uint64)
    good = lambda **kw: _call(L, **{**dict(cols=_ptrs(cols), b=0, e=n, scaling=_p(table), stride=1, params=_p(par), acc=_p(acc)), **kw})
    for f in (2, 9):
        assert good(f=f) == INVALID and b"field_of" in err()
    for b, e in ((1, 4), (0, 3), (4, 4), (6, 2), (0, 0), (0, (1 << 28) + 2)):   # odd, empty, reversed, too long
        assert good(b=b, e=e) == INVALID and b"even" in err(), (b, e)
    for rc in (good(cols=None), good(params=None), good(acc=None), good(cols=_ptrs(cols[:20] + [None] + cols[21:]))):
        assert rc == INVALID and b"NULL" in err()
    for stride in (0, (1 << 28) + 1):
        assert good(stride=stride) == INVALID and b"scaling_stride" in err()
    # acc on a column's elements that are read, on the scaling elements that are read; right behind them is no overlap
    big = np.zeros(4 * (n + 57), dtype=np.uint64)
    assert good(cols=_ptrs(cols[:35] + [big]), acc=_p(big[4 * (n - 1):])) == INVALID and b"overlaps an input" in err()
    assert good(cols=_ptrs([big] + cols[1:]), b=4, e=8, acc=_p(big[4 * 7:])) == INVALID and b"overlaps an input" in err()
    assert good(scaling=_p(big), stride=2, acc=_p(big[4 * 14:])) == INVALID and b"overlaps an input" in err()
    ok = [good(cols=_ptrs(cols[:35] + [big]), acc=_p(big[4 * n:])), good(cols=_ptrs([big] + cols[1:]), b=4, e=8, acc=_p(big[4 * 8:])),
          good(scaling=_p(big), stride=2, acc=_p(big[4 * 15:])), good(scaling=None, stride=0)]
    if not hip.have_device():
        assert ok == [NO_DEVICE] * 4   # valid calls: they get as far as asking for a device, and there is no CPU path
    # the table
    out, betas = np.zeros(4 * 4, dtype=np.uint64), np.ones(4 * 29, dtype=np.uint64)
    assert L.csh_honk_pow_table_dev(0, _p(betas), sz(29), _p(out), None) == INVALID and b"m must be 0 .. 28" in err()
    assert L.csh_honk_pow_table_dev(2, _p(betas), sz(2), _p(out), None) == INVALID and b"field_of" in err()
    assert L.csh_honk_pow_table_dev(0, None, sz(2), _p(out), None) == INVALID and b"NULL" in err()
    assert L.csh_honk_pow_table_dev(0, _p(betas), sz(2), None, None) == INVALID and b"NULL" in err()
    if not hip.have_device():
        assert L.csh_honk_pow_table_dev(0, None, sz(0), _p(out), None) == NO_DEVICE


def test_the_wrappers_check_the_column_count_and_the_range(hip):
    cols = [1 << 20] * 36
    par = np.ones(12, dtype=np.uint64)
    with pytest.raises(hip.CoSnarksHipError, match="columns"):
        hip.honk_sumcheck_accumulate(0, cols[:35], 0, 2, par, acc=1 << 21)
    for b, e in ((1, 4), (0, 3), (2, 2), (0, (1 << 28) + 2), (-2, 2)):
        with pytest.raises(hip.CoSnarksHipError, match="even"):
            hip.honk_sumcheck_accumulate(0, cols, b, e, par, acc=1 << 21)
    with pytest.raises(hip.CoSnarksHipError, match="scaling_stride"):
        hip.honk_sumcheck_accumulate(0, cols, 0, 2, par, acc=1 << 21, scaling=1 << 22, scaling_stride=0)
    with pytest.raises(hip.CoSnarksHipError, match="m must be"):
        hip.honk_pow_table(0, np.ones(4 * 29, dtype=np.uint64), out=1 << 21)


# ---- ABI and Rust text audits ----------------------------------------------------------------------------------------------------------------
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
    assert "co-noir UltraHonk, the sumcheck round" in txt
    for name in ("csh_selftest_honk_relations_host", "csh_selftest_honk_pow_table_host"):
        assert name not in declared and hasattr(L, name)
    # the column order of the header, the kernel's header and the restatement is one order
    at = txt.index("int csh_honk_sumcheck_accumulate_dev(")
    comment = txt[txt.rindex("/*", 0, at):at]
    names = lambda s: re.sub(r"(\w+)_1\.\.4", lambda m: ", ".join("%s_%d" % (m.group(1), k) for k in range(1, 5)), s)
    w = re.search(r"witness \(8\)\s+(.*?)\n", comment).group(1)
    sh = re.search(r"shifted witness \(5\)\s+(.*?)\s+--", comment).group(1)
    pre = re.search(r"precomputed \(23\)\s+(.*?)\n \* edge_begin", comment, re.S).group(1)
    flat = lambda s: [x.strip() for x in re.sub(r"[\s*]+", " ", names(s)).split(",") if x.strip()]
    assert flat(w) == R.WITNESS and [x + "_shift" for x in flat(sh)] == R.SHIFTED and flat(pre) == R.PRECOMPUTED
    hpp = open(os.path.join(ROOT, "co-snarks_amd", "csrc", "honk_relations.hpp")).read()
    enum = re.search(r"enum HrCol : int \{(.*?)\};", hpp, re.S).group(1)
    assert [x.strip().split(" ")[0][3:].lower() for x in enum.split(",")] == R.COLS
    assert "CSH_CHECK_BOUNDS" in open(os.path.join(ROOT, "co-snarks_amd", "csrc", "selftest.hip")).read()
    assert "honk_relations.hip" in open(os.path.join(ROOT, "co-snarks_amd", "build.py")).read()


def test_rust_shim_calls_both_entries_with_the_abi_column_count():
    src = open(os.path.join(ROOT, "rust", "co-noir-hip", "src", "sumcheck.rs")).read()
    lib_rs = open(os.path.join(ROOT, "rust", "co-noir-hip", "src", "lib.rs")).read()
    assert "pub mod sumcheck;" in lib_rs and "hip_compute_univariate" in lib_rs
    assert "sys::csh_honk_sumcheck_accumulate_dev(" in src and "sys::csh_honk_pow_table_dev(" in src
    assert "pub const SUMCHECK_COLUMNS: usize = 36;" in src and "pub const ACC_ELEMS: usize = 57;" in src
    lens = re.search(r"ACC_LENGTHS: \[usize; 11\] = \[(.*?)\]", src).group(1)
    assert [int(x) for x in lens.split(",")] == R.ACC_LEN
    assert "sumcheck_round_prover.rs:224-255" in src and "decider/types.rs:53-67" in src
