"""Device tests of the batched Poseidon2 entries (csrc/poseidon2.hip) against tests/poseidon2_ref.py. Every comparison is
exact and covers every word; every output has guard words behind it and is checked to be canonical. Every test calls entries that the
parent commit does not have."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import helpers as H
from tests import poseidon2_ref as P2
from tests.test_poseidon2_cpu import TREES, Both, flat, params, shared_case, unflat

pytestmark = pytest.mark.gpu

GUARD, NGUARD = np.uint64(0x5A5A5A5A5A5A5A5A), 8
sz, u32 = C.c_size_t, C.c_uint32
INVALID = -1


def guarded(hip, words):
    return hip.DeviceBuffer.from_host(np.full(words + NGUARD, GUARD, dtype=np.uint64))


def down(F, buf, words, what):
    raw = buf.to_host()
    assert raw.size == words + NGUARD and (raw[words:] == GUARD).all(), (what, "written past the end")
    return H.unpack(F, raw[:words])          # strict: canonical


def guards_intact(buf, words, what):
    raw = buf.to_host()
    assert raw.size == words + NGUARD and (raw[words:] == GUARD).all(), (what, "written past the end")


def up(hip, F, vals):
    return hip.DeviceBuffer.from_host(H.pack(F, vals) if vals else np.zeros(4, dtype=np.uint64))


@functools.lru_cache(maxsize=None)
def dev_params(hip, curve, t, shape):
    F, P = H.FR[curve], params(curve, t, shape)
    return hip.Poseidon2Params(H.CURVE_IDS[curve], t, P.rf_b, P.rf_e, P.rp, H.pack(F, [c for row in P.rc_ext for c in row]), H.pack(F, P.rc_int),
                               H.pack(F, P.diag))


@functools.lru_cache(maxsize=None)
def batch(curve, t, shape, n):
    """seeded states and their permutation, computed once"""
    P = params(curve, t, shape)
    r = H.rng(1000 * t + n)
    values = [r.randrange(P.p) for _ in range(n * t)]
    return values, P2.permute_batch(P, values)


def dev_permute(hip, curve, t, shape, values, in_place=False):
    F = H.FR[curve]
    n = len(values) // t
    if in_place:
        buf = hip.DeviceBuffer.from_host(np.concatenate([H.pack(F, values), np.full(NGUARD, GUARD, dtype=np.uint64)]))
        hip.poseidon2_permute(dev_params(hip, curve, t, shape), buf, n)
    else:
        src, buf = up(hip, F, values), guarded(hip, 4 * n * t)
        hip.poseidon2_permute(dev_params(hip, curve, t, shape), src, n, out=buf)
        assert (src.to_host()[:4 * n * t] == H.pack(F, values)).all()
    hip.bindings.sync()
    return down(F, buf, 4 * n * t, "permute")


# ---- plain batch -----------------------------------------------------------------------------------------------------------------------------
# 1, 3: less than a wave; 65: across a wave; 257: across a workgroup of 256 lanes
@pytest.mark.parametrize("n", [1, 3, 65, 257])
@pytest.mark.parametrize("shape", ["short", "bn254"])
@pytest.mark.parametrize("t", [2, 3, 4])
def test_plain_batch(gpu, t, shape, n):
    values, want = batch("bn254", t, shape, n)
    assert dev_permute(gpu, "bn254", t, shape, values) == want
    if n in (3, 257):
        assert dev_permute(gpu, "bn254", t, shape, values, in_place=True) == want


@pytest.mark.parametrize("t", [2, 3, 4])
def test_plain_batch_over_a_capped_grid(gpu, t):
    """1000 states on two workgroups of 256 lanes: the grid-stride loop runs twice for every lane"""
    values, want = batch("bn254", t, "bn254", 1000)
    with gpu.tuned(vec_max_blocks=2):
        assert dev_permute(gpu, "bn254", t, "bn254", values) == want
        assert dev_permute(gpu, "bn254", t, "bn254", values, in_place=True) == want


@pytest.mark.parametrize("shape", ["short", "bn254"])
@pytest.mark.parametrize("t", [2, 3, 4])
def test_plain_batch_at_the_edges_of_the_field(gpu, t, shape):
    P = params("bn254", t, shape)
    values = [0] * t + [P.p - 1] * t + [1] * t
    assert dev_permute(gpu, "bn254", t, shape, values) == P2.permute_batch(P, values)


@pytest.mark.parametrize("curve", ["bls12_381", "bls12_377"])
def test_plain_batch_on_the_other_fields(gpu, curve):
    for t in (2, 3, 4):
        P = params(curve, t, "bn254")
        values, want = batch(curve, t, "bn254", 65)
        assert dev_permute(gpu, curve, t, "bn254", values + [P.p - 1] * t) == want + P2.permutation(P, [P.p - 1] * t)


# ---- Merkle trees ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tree(curve, t, arity, mode, n):
    P = params(curve, t, "short")
    r = H.rng(7 * n + t)
    leaves = [r.randrange(P.p) for _ in range(n)]
    return leaves, P2.merkle_tree(P, leaves, arity, mode)


def dev_merkle(hip, curve, t, arity, mode, leaves):
    F = H.FR[curve]
    n = len(leaves)
    src, root, work = up(hip, F, leaves), guarded(hip, 4), guarded(hip, 4 * 2 * max(n // arity, 1))
    hip.poseidon2_merkle(dev_params(hip, curve, t, "short"), arity, mode, src, n, root=root, work=work)
    hip.bindings.sync()
    guards_intact(work, 4 * 2 * max(n // arity, 1), "merkle work")
    assert (src.to_host()[:4 * n] == H.pack(F, leaves)).all()
    return down(F, root, 4, "merkle root")[0]


@pytest.mark.parametrize("t,arity,mode", TREES)
def test_merkle_trees(gpu, t, arity, mode):
    for n in {2: (1, 2, 8, 128), 4: (4, 64)}[arity]:
        leaves, want = tree("bn254", t, arity, mode, n)
        assert dev_merkle(gpu, "bn254", t, arity, mode, leaves) == want, n


def test_merkle_tree_over_a_capped_grid_and_on_bls12_381(gpu):
    leaves, want = tree("bn254", 3, 2, P2.SPONGE, 1024)
    with gpu.tuned(vec_max_blocks=1):
        assert dev_merkle(gpu, "bn254", 3, 2, P2.SPONGE, leaves) == want
    leaves, want = tree("bls12_381", 4, 4, P2.COMPRESSION, 16)
    assert dev_merkle(gpu, "bls12_381", 4, 4, P2.COMPRESSION, leaves) == want


# ---- the collaborative round step ------------------------------------------------------------------------------------------------------------
class DevStepper:
    """csh_poseidon2_co_round_dev / csh_poseidon2_layer_next_dev behind the stepper interface of the restatement; the precomputation is
    uploaded once per party"""

    def __init__(self, hip, curve, t, shape, net, pre):
        self.hip, self.curve, self.F, self.cid, self.net = hip, curve, H.FR[curve], H.CURVE_IDS[curve], net
        self.P, self.par = params(curve, t, shape), dev_params(hip, curve, t, shape)
        self.pre = [[up(hip, self.F, flat(v)) for v in party] for party in pre]

    def step(self, party, step, state, n_perm, y, pre, off):
        hip, F, P, nc = self.hip, self.F, self.P, self.net.protocol + 1
        R = P2.rounds(P)
        words = 4 * nc * n_perm * P.t
        st = hip.DeviceBuffer.from_host(np.concatenate([H.pack(F, flat(state)), np.full(NGUARD, GUARD, dtype=np.uint64)]))
        n_open = P2.round_entries(P, step, n_perm) if step < R else 0
        opened, ff = guarded(hip, 4 * nc * n_open), guarded(hip, 4 * nc * n_perm)
        yy = up(hip, F, y) if y is not None else None
        hip.poseidon2_co_round(self.cid, self.net.protocol, party, self.par, step, st, n_perm, yy, self.pre[party], off,
                               open_out=opened if step < R else None, ff_out=ff if step == 0 else None)
        hip.bindings.sync()
        got_ff = unflat(down(F, ff, 4 * nc * n_perm if step == 0 else 0, "ff")[:nc * n_perm], nc) if step == 0 else None
        if step:
            assert (ff.to_host() == GUARD).all(), "ff_out written after step 0"
        guards_intact(opened, 4 * nc * n_open, "open")
        got_open = unflat(down(F, opened, 4 * nc * n_open, "open"), nc) if n_open else []
        return unflat(down(F, st, words, "state"), nc), got_open, got_ff

    def layer_next(self, party, state, ff, arity, mode, ln):
        hip, F, P, nc = self.hip, self.F, self.P, self.net.protocol + 1
        count = nc * (1 if ln == 1 else ln // arity * P.t)
        out = guarded(hip, 4 * count)
        hip.poseidon2_layer_next(self.cid, nc, P.t, arity, mode, up(hip, F, flat(state)), up(hip, F, flat(ff)) if mode == P2.COMPRESSION else None, ln,
                                 next_out=out)
        hip.bindings.sync()
        return unflat(down(F, out, 4 * count, "layer_next"), nc)


def run_steps(hip, curve, t, shape, kind, n_perm, seed, start=0):
    P = params(curve, t, shape)
    net, plain, states, pre = shared_case(P, kind, n_perm, seed)
    if start:
        junk = tuple([3] * (net.protocol + 1))
        pre = [[[junk] * start + v for v in party] for party in pre]
    st = Both(P2.RefStepper(P, net), DevStepper(hip, curve, t, shape, net, pre))
    out, off, _ = P2.co_permutation(P, net, st, states, pre, start)
    assert st.compared == net.n * (P2.rounds(P) + 1)
    assert off == start + P2.num_sbox(P) * n_perm
    assert net.open(out) == P2.permute_batch(P, plain)


# every step's open_dev and state of every party (Rep3: 0, 1, 2) against the restatement. 1, 5: less than a wave; 130: two workgroups of
# Rep3 values (260), across a wave and a half of Shamir values
@pytest.mark.parametrize("kind", ["rep3", "shamir"])
@pytest.mark.parametrize("n_perm", [1, 5, 130])
@pytest.mark.parametrize("t", [2, 3, 4])
def test_round_steps(gpu, t, n_perm, kind):
    run_steps(gpu, "bn254", t, "short", kind, n_perm, 31 * t + n_perm)


@pytest.mark.parametrize("kind", ["rep3", "shamir"])
def test_round_steps_on_the_bn254_round_numbers(gpu, kind):
    run_steps(gpu, "bn254", 4, "bn254", kind, 5, 77)


def test_round_steps_from_a_starting_offset_over_a_capped_grid(gpu):
    with gpu.tuned(vec_max_blocks=1):
        run_steps(gpu, "bn254", 3, "short", "rep3", 130, 5, start=37)


def test_round_steps_on_bls12_381(gpu):
    run_steps(gpu, "bls12_381", 4, "short", "rep3", 5, 9)


@pytest.mark.parametrize("kind", ["rep3", "shamir"])
def test_closed_chain_through_device_entries(gpu, kind):
    """state, opened values and precomputation stay on the device from the first step to the last, and nothing is synchronised before the
    end; openings are csh_lincomb_dev (Rep3: the three a components add up, csh_extract_component_dev then keeps one value per share;
    Shamir: the Lagrange combination is the opened vector itself); the reconstructed result equals csh_poseidon2_permute_dev on the
    reconstructed input, word for word"""
    hip, curve, t, n_perm = gpu, "bn254", 4, 130
    F, cid, P = H.FR[curve], H.CURVE_IDS[curve], params(curve, t, "short")
    net, plain, states, pre = shared_case(P, kind, n_perm, 99)
    nc, par, R = net.protocol + 1, dev_params(hip, curve, t, "short"), P2.rounds(P)
    coeffs = H.pack(F, net.lagrange if kind == "shamir" else [1, 1, 1])
    L, alive = hip.lib(), []

    def reconstruct(bufs, n_shares):
        out = hip.DeviceBuffer(32 * nc * n_shares)
        arr = (C.c_void_p * 3)(*[b.ptr.value for b in bufs])
        assert L.csh_lincomb_dev(cid, arr, coeffs.ctypes.data_as(C.c_void_p), sz(3), out.ptr, sz(nc * n_shares), None) == 0
        if nc == 1:
            return out
        thin = hip.DeviceBuffer(32 * n_shares)
        alive.append(out)   # read by a queued kernel: kept until the final synchronisation
        assert L.csh_extract_component_dev(out.ptr, u32(2), u32(0), sz(n_shares), thin.ptr, None) == 0
        return thin

    st = [up(hip, F, flat(s)) for s in states]
    dpre = [[up(hip, F, flat(v)) for v in party] for party in pre]
    want = hip.poseidon2_permute(par, reconstruct(st, n_perm * t), n_perm, out=hip.DeviceBuffer(32 * n_perm * t))
    y, off = None, 0
    for s in range(R + 1):
        opened = [hip.poseidon2_co_round(cid, net.protocol, k, par, s, st[k], n_perm, y, dpre[k], off) for k in range(3)]
        if s < R:
            y = reconstruct(opened, P2.round_entries(P, s, n_perm))
            off += P2.round_entries(P, s, n_perm)
    got = reconstruct(st, n_perm * t)
    hip.bindings.sync()
    assert off == P2.num_sbox(P) * n_perm
    assert (got.to_host() == want.to_host()).all()
    assert H.unpack(F, got.to_host()) == P2.permute_batch(P, plain)


# ---- the collaborative tree ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["rep3", "shamir"])
@pytest.mark.parametrize("t,arity,mode", [(2, 2, P2.COMPRESSION), (3, 2, P2.SPONGE)])
def test_collaborative_tree(gpu, t, arity, mode, kind):
    """8 leaves through co_round + layer_next: the opened root is csh_poseidon2_merkle_dev's on the reconstructed leaves"""
    curve, n = "bn254", 8
    P = params(curve, t, "short")
    rnd = H.rng(55 + t)
    net = P2.NETS[kind](P.p)
    leaves = [rnd.randrange(P.p) for _ in range(n)]
    hashes = P2.num_hashes(n, arity)
    pre = P2.precompute(P, net, hashes, rnd)
    st = Both(P2.RefStepper(P, net), DevStepper(gpu, curve, t, "short", net, pre))
    root, off = P2.co_merkle_tree(P, net, st, net.share(leaves, rnd), arity, mode, pre)
    assert off == P2.num_sbox(P) * hashes
    assert net.open([[r] for r in root]) == [dev_merkle(gpu, curve, t, arity, mode, leaves)]


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
def test_refusals(gpu):
    hip, L = gpu, gpu.lib()
    F = H.FR["bn254"]
    err = lambda: L.csh_last_error()
    one = H.pack(F, [1, 2] * 8)
    h = C.c_void_p()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for t in (1, 5, 16):
        assert L.csh_poseidon2_params_create(0, u32(t), u32(1), u32(1), u32(1), p(one), p(one), p(one), C.byref(h)) == INVALID and b"t must be" in err()
    assert L.csh_poseidon2_params_create(0, u32(3), u32(1), u32(1), u32(1), p(one), p(one), p(one), C.byref(h)) == INVALID and b"fixed" in err()
    assert L.csh_poseidon2_params_create(7, u32(4), u32(1), u32(1), u32(1), p(one), p(one), p(one), C.byref(h)) == INVALID
    assert L.csh_poseidon2_params_create(0, u32(4), u32(1), u32(1), u32(1), None, p(one), p(one), C.byref(h)) == INVALID and b"NULL" in err()
    par3, par4 = dev_params(hip, "bn254", 3, "short"), dev_params(hip, "bn254", 4, "short")
    buf = hip.DeviceBuffer.from_host(np.zeros(4 * 64, dtype=np.uint64))
    at = lambda k: C.c_void_p(buf.ptr.value + 32 * k)
    # arity against mode, n_leaves no power of the arity
    for par, arity, mode, n in ((par3, 3, 0, 3), (par3, 4, 1, 4), (par4, 1, 1, 1), (par4, 2, 2, 2), (par4, 2, 0, 6), (par4, 4, 1, 8), (par3, 2, 0, 0)):
        assert L.csh_poseidon2_merkle_dev(par.h, u32(arity), u32(mode), at(0), sz(n), at(40), at(48), None) == INVALID, (arity, mode, n)
    with pytest.raises(hip.CoSnarksHipError, match="power of the arity"):
        hip.poseidon2_merkle(par4, 2, 0, buf, 6)
    with pytest.raises(hip.CoSnarksHipError, match="arity"):
        hip.poseidon2_merkle(par3, 3, 0, buf, 3)
    # overlaps: the batch may run in place, and in no other overlapping way; tree outputs off the leaves and off each other
    assert L.csh_poseidon2_permute_dev(par4.h, at(0), sz(4), at(0), None) == 0
    assert L.csh_poseidon2_permute_dev(par4.h, at(0), sz(4), at(1), None) == INVALID and b"overlaps an input" in err()
    assert L.csh_poseidon2_merkle_dev(par4.h, u32(2), u32(0), at(0), sz(8), at(7), at(16), None) == INVALID and b"overlaps an input" in err()
    assert L.csh_poseidon2_merkle_dev(par4.h, u32(2), u32(0), at(0), sz(8), at(8), at(4), None) == INVALID and b"overlaps an input" in err()
    assert L.csh_poseidon2_merkle_dev(par4.h, u32(2), u32(0), at(0), sz(8), at(20), at(16), None) == INVALID and b"two outputs overlap" in err()
    pre = (C.c_void_p * 5)(*[at(32).value] * 5)
    co = lambda step, state, y, pr, off, op, ff, proto=1, party=0, field=0, par=par4: L.csh_poseidon2_co_round_dev(
        field, u32(proto), u32(party), par.h, u32(step), state, sz(1), y, pr, sz(off), op, ff, None)
    assert co(0, at(0), None, pre, 0, at(8), None) == 0
    assert co(0, at(0), None, pre, 0, at(7), None) == INVALID and b"two outputs overlap" in err()
    assert co(0, at(0), None, pre, 0, at(8), at(15)) == INVALID and b"two outputs overlap" in err()
    assert co(0, at(0), None, pre, 0, at(32), None) == INVALID and b"overlaps an input" in err()
    assert co(1, at(0), at(4), pre, 4, at(8), None) == INVALID and b"overlaps an input" in err()
    assert co(8, at(0), at(16), pre, 0, at(8), None) == INVALID and b"step must be" in err()
    assert co(1, at(0), at(16), pre, 3, at(8), None) == INVALID and b"lies below" in err()
    assert co(0, at(0), None, pre, 0, at(8), None, proto=2) == INVALID and co(0, at(0), None, pre, 0, at(8), None, party=3) == INVALID
    assert co(0, at(0), None, pre, 0, at(8), None, field=1) == INVALID and b"field" in err()
    # NULL arguments
    assert co(0, None, None, pre, 0, at(8), None) == INVALID and b"NULL" in err()
    assert co(0, at(0), None, pre, 0, None, None) == INVALID and b"NULL" in err()
    assert co(1, at(0), None, pre, 4, at(8), None) == INVALID and b"NULL" in err()
    assert co(0, at(0), None, None, 0, at(8), None) == INVALID and b"NULL" in err()
    assert L.csh_poseidon2_permute_dev(par4.h, None, sz(4), at(0), None) == INVALID and b"NULL" in err()
    assert L.csh_poseidon2_permute_dev(None, at(0), sz(4), at(0), None) == INVALID
    assert L.csh_poseidon2_merkle_dev(par4.h, u32(2), u32(0), at(0), sz(8), None, at(16), None) == INVALID and b"NULL" in err()
    assert L.csh_poseidon2_merkle_dev(par4.h, u32(2), u32(0), at(0), sz(8), at(8), None, None) == INVALID and b"NULL" in err()
    assert L.csh_poseidon2_layer_next_dev(0, u32(2), u32(3), u32(2), u32(1), at(0), None, at(40), sz(2), None) == INVALID and b"NULL" in err()
    assert L.csh_poseidon2_layer_next_dev(0, u32(2), u32(3), u32(2), u32(0), at(0), None, at(40), sz(3), None) == INVALID and b"multiple" in err()
    assert L.csh_poseidon2_layer_next_dev(0, u32(3), u32(3), u32(2), u32(0), at(0), None, at(40), sz(2), None) == INVALID
    with pytest.raises(hip.CoSnarksHipError, match="step must be"):
        hip.poseidon2_co_round(0, 1, 0, par4, 8, buf, 1, None, [buf] * 5, 0)
    hip.bindings.sync()
