"""CPU tests of the Poseidon2 restatement (tests/poseidon2_ref.py) and of the host self-test of csrc/poseidon2.hpp. The first group needs no
library: it is what makes the restatement a reference for the device tests. The second runs the per-state functions the kernels call on
the host with the limb-bound checks of field29.hpp on (a violated bound aborts the process)."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import helpers as H
from tests import poseidon2_ref as P2

CURVES = ["bn254", "bls12_381", "bls12_377"]
TREES = [(2, 2, P2.COMPRESSION), (3, 2, P2.SPONGE), (3, 2, P2.COMPRESSION), (4, 2, P2.SPONGE), (4, 2, P2.COMPRESSION), (4, 4, P2.COMPRESSION)]


@functools.lru_cache(maxsize=None)
def params(curve, t, shape):
    return P2.make_params(H.FR[curve].p, t, shape)


def flat(shares):
    return [c for s in shares for c in s]


def unflat(vals, nc):
    return [tuple(vals[i:i + nc]) for i in range(0, len(vals), nc)]


def shared_case(P, kind, n_perm, seed, values=None):
    """-> (net, plain states, the parties' states, the parties' precomputation)"""
    rnd = H.rng(seed)
    net = P2.NETS[kind](P.p)
    plain = values if values is not None else [rnd.randrange(P.p) for _ in range(n_perm * P.t)]
    return net, plain, net.share(plain, rnd), P2.precompute(P, net, n_perm, rnd)


class Both:
    """two steppers side by side: every output of every step of every party is compared"""

    def __init__(self, ref, other):
        self.ref, self.other, self.compared = ref, other, 0

    def step(self, *a):
        want, got = self.ref.step(*a), self.other.step(*a)
        assert got[0] == want[0], ("state", a[0], a[1])
        assert got[1] == want[1], ("open", a[0], a[1])
        assert a[1] != 0 or got[2] == want[2], ("feed-forward", a[0])
        self.compared += 1
        return want

    def layer_next(self, *a):
        want, got = self.ref.layer_next(*a), self.other.layer_next(*a)
        assert got == want, ("layer_next", a[0])
        self.compared += 1
        return want


# ---- the restatement against itself ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["rep3", "shamir"])
@pytest.mark.parametrize("shape", ["short", "bn254"])
@pytest.mark.parametrize("t", [2, 3, 4])
def test_packed_permutation_with_precomputation_reconstructs_to_the_plain_one(t, shape, kind):
    P = params("bn254", t, shape)
    net, plain, states, pre = shared_case(P, kind, 3, 11 * t)
    out, off, _ = P2.co_permutation(P, net, P2.RefStepper(P, net), states, pre, 0)
    assert net.open(out) == P2.permute_batch(P, plain)
    assert off == P2.num_sbox(P) * 3


def test_a_starting_offset_shifts_every_read():
    P = params("bn254", 4, "short")
    net, plain, states, pre = shared_case(P, "rep3", 2, 5)
    pad = [[[(7, 9)] * 13 + v for v in party] for party in pre]
    out, off, _ = P2.co_permutation(P, net, P2.RefStepper(P, net), states, pad, 13)
    assert net.open(out) == P2.permute_batch(P, plain) and off == 13 + P2.num_sbox(P) * 2


@pytest.mark.parametrize("t,arity,mode", TREES)
def test_both_tree_modes_equal_the_tree_that_hashes_every_node(t, arity, mode):
    P = params("bn254", t, "short")
    rnd = H.rng(t * 10 + arity)
    for k in (1, 2, 3):
        leaves = [rnd.randrange(P.p) for _ in range(arity ** k)]
        assert P2.merkle_tree(P, leaves, arity, mode) == P2.trivial_merkle_tree(P, leaves, arity, mode)
    assert P2.merkle_tree(P, [5], arity, mode) == 5


@pytest.mark.parametrize("kind", ["rep3", "shamir"])
@pytest.mark.parametrize("t,arity,mode", TREES)
def test_collaborative_tree_and_its_precomputation_offset(t, arity, mode, kind):
    P = params("bn254", t, "short")
    rnd = H.rng(100 + t)
    net = P2.NETS[kind](P.p)
    n = arity ** 2
    leaves = [rnd.randrange(P.p) for _ in range(n)]
    hashes = P2.num_hashes(n, arity)
    pre = P2.precompute(P, net, hashes, rnd)
    root, off = P2.co_merkle_tree(P, net, P2.RefStepper(P, net), net.share(leaves, rnd), arity, mode, pre)
    assert net.open([[r] for r in root]) == [P2.merkle_tree(P, leaves, arity, mode)]
    assert off == P2.num_sbox(P) * hashes == len(pre[0][0])


def test_end_rounds_read_on_from_rounds_f_beginning():
    """a permutation whose end rounds restarted at constant 0 differs (the restatement is sensitive to what mutation 1 changes)"""
    P = params("bn254", 3, "short")
    Q = P._replace(rc_ext=P.rc_ext[:P.rf_b] + P.rc_ext[:P.rf_e])
    assert P2.permutation(P, [1, 2, 3]) != P2.permutation(Q, [1, 2, 3])


# ---- the host self-test: the kernels' per-state functions with the bound checks on ------------------------------------------------------------
def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _table(F, P):
    return (H.pack(F, [c for row in P.rc_ext for c in row]) if P.rc_ext else None, H.pack(F, P.rc_int) if P.rc_int else None, H.pack(F, P.diag))


def host_plain(hip, curve, P, values, take, whole, feed_forward):
    F = H.FR[curve]
    ext, inn, diag = _table(F, P)
    n = len(values) // take
    out = np.zeros(4 * (n * P.t if whole else n), dtype=np.uint64)
    src = H.pack(F, values)
    rc = hip.lib().csh_selftest_poseidon2_host(H.CURVE_IDS[curve], C.c_uint32(P.t), C.c_uint32(P.rf_b), C.c_uint32(P.rf_e), C.c_uint32(P.rp), _p(ext), _p(inn),
                                               _p(diag), 0, C.c_uint32(0), C.c_uint32(0), C.c_uint32(take), C.c_uint32(int(whole) | int(feed_forward) << 1),
                                               _p(src), C.c_size_t(n), None, None, C.c_size_t(0), _p(out), None, None)
    assert rc == 0
    return H.unpack(F, out)


class HostStepper:
    """csh_selftest_poseidon2_host, op 1, behind the stepper interface"""

    def __init__(self, hip, curve, P, net):
        self.hip, self.curve, self.F, self.P, self.net = hip, curve, H.FR[curve], P, net
        self.table = _table(self.F, P)

    def step(self, party, step, state, n_perm, y, pre, off):
        F, P, nc = self.F, self.P, self.net.protocol + 1
        ext, inn, diag = self.table
        R = P2.rounds(P)
        src = H.pack(F, flat(state))
        out = np.zeros_like(src)
        n_open = P2.round_entries(P, step, n_perm) if step < R else 0
        opened = np.zeros(4 * nc * max(n_open, 1), dtype=np.uint64)
        ff = np.zeros(4 * nc * n_perm, dtype=np.uint64)
        yy = H.pack(F, y) if y is not None else None
        pv = [H.pack(F, flat(v)) for v in pre]
        ptrs = (C.c_void_p * 5)(*[v.ctypes.data for v in pv])
        rc = self.hip.lib().csh_selftest_poseidon2_host(H.CURVE_IDS[self.curve], C.c_uint32(P.t), C.c_uint32(P.rf_b), C.c_uint32(P.rf_e), C.c_uint32(P.rp),
                                                        _p(ext), _p(inn), _p(diag), 1, C.c_uint32(self.net.protocol), C.c_uint32(party), C.c_uint32(step),
                                                        C.c_uint32(0), _p(src), C.c_size_t(n_perm), _p(yy), ptrs, C.c_size_t(off), _p(out), _p(opened), _p(ff))
        assert rc == 0
        return (unflat(H.unpack(F, out), nc), unflat(H.unpack(F, opened), nc)[:n_open], unflat(H.unpack(F, ff), nc) if step == 0 else None)

    def layer_next(self, party, state, ff, arity, mode, ln):
        return P2.layer_next(self.P, state, ff, arity, mode, ln)


def edge_states(p, t, rnd):
    """all 0, all 1, all p - 1, and random states"""
    return [0] * t + [1] * t + [p - 1] * t + [rnd.randrange(p) for _ in range(3 * t)]


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("t", [2, 3, 4])
def test_host_selftest_plain_permutation_within_the_bounds(hip, curve, t):
    for shape in ("short", "bn254"):
        P = params(curve, t, shape)
        values = edge_states(P.p, t, H.rng(t))
        assert host_plain(hip, curve, P, values, t, True, False) == P2.permute_batch(P, values)


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("t,arity,mode", TREES)
def test_host_selftest_gathering_form(hip, curve, t, arity, mode):
    """a tree layer: `arity` elements taken, zeros after them, element 0 written, the feed-forward in compression mode"""
    P = params(curve, t, "short")
    values = edge_states(P.p, arity, H.rng(arity))
    want = []
    for i in range(0, len(values), arity):
        st = values[i:i + arity] + [0] * (t - arity)
        want.append((P2.permutation(P, st)[0] + (st[0] if mode == P2.COMPRESSION else 0)) % P.p)
    assert host_plain(hip, curve, P, values, arity, False, mode == P2.COMPRESSION) == want


@pytest.mark.parametrize("kind", ["rep3", "shamir", "plain"])
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("t", [2, 3, 4])
def test_host_selftest_collaborative_steps_within_the_bounds(hip, curve, t, kind):
    """every step of every party against the restatement; the states are the edge values (their shares are random), and one run has
    every share component and every precomputed value at p - 1 or 0"""
    P = params(curve, t, "short")
    plain = edge_states(P.p, t, H.rng(t + 1))
    net, plain, states, pre = shared_case(P, kind, len(plain) // t, 3 * t, values=plain)
    st = Both(P2.RefStepper(P, net), HostStepper(hip, curve, P, net))
    out, off, _ = P2.co_permutation(P, net, st, states, pre, 0)
    assert st.compared == net.n * (P2.rounds(P) + 1)
    assert net.open(out) == P2.permute_batch(P, plain)
    # extreme components: not a sharing of anything, the local stretch is compared step by step all the same
    nc = net.protocol + 1
    for v in (P.p - 1, 0):
        state = [tuple([v] * nc)] * (2 * t)
        prex = [[tuple([v] * nc)] * (P2.num_sbox(P) * 2)] * 5
        ref, host = P2.RefStepper(P, net), HostStepper(hip, curve, P, net)
        off = 0
        for s in range(P2.rounds(P) + 1):
            y = [v] * (P2.round_entries(P, s - 1, 2)) if s else None
            want, got = ref.step(0, s, state, 2, y, prex, off), host.step(0, s, state, 2, y, prex, off)
            assert got[:2] == want[:2], (v, s)
            state = want[0]
            off += P2.round_entries(P, s, 2) if s < P2.rounds(P) else 0


def test_refusals_that_need_no_device(hip):
    L = hip.lib()
    one = np.zeros(64, dtype=np.uint64)
    h = C.c_void_p()
    err = lambda: L.csh_last_error()
    assert L.csh_poseidon2_params_create(0, C.c_uint32(5), C.c_uint32(1), C.c_uint32(1), C.c_uint32(1), _p(one), _p(one), _p(one), C.byref(h)) == -1
    assert b"t must be 2, 3 or 4" in err() and not h
    assert L.csh_poseidon2_params_create(0, C.c_uint32(4), C.c_uint32(1), C.c_uint32(1), C.c_uint32(1), _p(one), _p(one), None, C.byref(h)) == -1
    assert b"NULL" in err()
    assert L.csh_poseidon2_params_create(0, C.c_uint32(2), C.c_uint32(1), C.c_uint32(1), C.c_uint32(1), _p(one), _p(one), _p(one), C.byref(h)) == -1
    assert b"fixed" in err()
    assert L.csh_poseidon2_permute_dev(None, _p(one), C.c_size_t(1), _p(one), None) == -1 and b"handle" in err()
    assert L.csh_poseidon2_layer_next_dev(0, C.c_uint32(2), C.c_uint32(3), C.c_uint32(3), C.c_uint32(0), _p(one), None, _p(one[32:]), C.c_size_t(3), None) == -1
    assert b"arity" in err()
    assert L.csh_poseidon2_layer_next_dev(0, C.c_uint32(1), C.c_uint32(3), C.c_uint32(2), C.c_uint32(1), _p(one), None, _p(one[32:]), C.c_size_t(2), None) == -1
    assert b"NULL" in err()
    assert L.csh_poseidon2_layer_next_dev(0, C.c_uint32(1), C.c_uint32(3), C.c_uint32(2), C.c_uint32(0), _p(one), None, _p(one[4:]), C.c_size_t(2), None) == -1
    assert b"overlaps an input" in err()
    with pytest.raises(hip.CoSnarksHipError, match="t must be"):
        hip.Poseidon2Params(0, 5, 1, 1, 1, one[:40], one[:4], one[:20])
    with pytest.raises(hip.CoSnarksHipError, match="rc_external holds"):
        hip.Poseidon2Params(0, 4, 1, 1, 1, one[:28], one[:4], one[:16])
    with pytest.raises(hip.CoSnarksHipError, match="arity"):
        hip.poseidon2_layer_next(0, 1, 3, 3, 0, 1 << 20, None, 3)


def test_header_and_bindings_declare_the_entry_points(hip):
    from cosnarks_amd import bindings
    txt = open(bindings.header_path()).read()
    declared = bindings.declared_symbols()
    src = open(bindings.__file__).read()
    cites = {"csh_poseidon2_params_create": ["poseidon2_permutation.rs:126-147"], "csh_poseidon2_permute_dev": ["poseidon2_permutation.rs:194-214", ":209-213"],
             "csh_poseidon2_merkle_dev": ["merkle_tree/plain.rs:15-50", ":113-155"],
             "csh_poseidon2_co_round_dev": ["rep3.rs:612-648", "shamir.rs:326-365", ":358-388", "rep3.rs:240"],
             "csh_poseidon2_layer_next_dev": ["merkle_tree/rep3.rs:44-52", ":99-111"]}
    L = hip.lib()
    for name, cs in cites.items():
        assert name in declared and hasattr(L, name), name
        at = txt.index("int %s(" % name)
        comment = txt[txt.rindex("/*", 0, at):at]
        for c in cs:
            assert c in comment, (name, c)
        assert "lib().%s(" % name in src
    assert "csh_selftest_poseidon2_host" not in declared and hasattr(L, "csh_selftest_poseidon2_host")
