"""CPU tests of the Shamir preprocessing restatement (tests/shamir_rng_ref.py) and of the host self-tests of csrc/field_rand.hpp and
csrc/shamir_rng.hpp. The first group needs no library and passes without the feature: it holds the restatement against the protocol's
own property (every pair opens to the same value from its degree-t and its degree-2t shares), which is what makes it a reference for the
device tests. The second runs the per-candidate and per-element functions the kernels call on the host, word for word against it.
Parity with ark-ff's sampler is by restatement only (PARITY UNPINNED: no reference vector)."""
import ctypes as C

import numpy as np
import pytest

from oracle import arkfmt, chacha
from tests import helpers as H
from tests import shamir_rng_ref as R

CURVES = ["bn254", "bls12_381", "bls12_377"]
SHAPES = [(3, 1), (4, 1), (5, 2), (7, 3)]

# Planted seeds: the smallest counter i whose 32 little-endian bytes, as a seed, have the property (searched on the CPU with
# shamir_rng_ref.candidates / accepted, i = 0, 1, 2, ...; the properties are asserted in test_planted_seeds_have_their_properties).
SEED_CAND0_REJECTED = (12).to_bytes(32, "little")        # BN254: candidate 0 is rejected
SEED_TILE_EDGE_REJECTED = (9).to_bytes(32, "little")     # BN254: candidates 255 and 256 are both rejected (a tile boundary)
SEED_CHUNK_EDGE = (4).to_bytes(32, "little")             # BN254: candidate 255 accepted, 256 rejected (last of a chunk / first of the next)
SEED_RUN_OF_REJECTIONS = (0).to_bytes(32, "little")      # BLS12-377: candidates 186 .. 192 are all rejected (a run of seven)
PLANTED = [SEED_CAND0_REJECTED, SEED_TILE_EDGE_REJECTED, SEED_CHUNK_EDGE]


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def mask_of(F, seed, n):
    return [R.accepted(F, v) is not None for v in R.candidates(seed, 0, n)]


# ---- the restatement against itself and the oracle ---------------------------------------------------------------------------------------
def test_vectorised_keystream_is_the_oracles():
    key = bytes(range(7, 39))
    for first, count in ((0, 1), (5, 3), ((1 << 32) - 1, 3)):
        got = R.chacha12_blocks(key, first, count)
        for k in range(count):
            assert got[k].tobytes() == chacha.block(key, first + k, 12)


@pytest.mark.parametrize("curve", CURVES)
def test_field_rand_ref_is_expand_seeded(curve):
    F = H.FR[curve]
    seed = bytes(range(32))
    raw, end = R.field_rand_ref(F, seed, 0, 300)
    assert [v * F.Rinv % F.p for v in raw] == arkfmt.expand_seeded(("seed", seed, 300), F.p, F.p.bit_length(), F.R)
    # a stream continues at cand_end, and a seed draw is one candidate slot
    a, mid = R.field_rand_ref(F, seed, 0, 100)
    b, end2 = R.field_rand_ref(F, seed, mid, 200)
    assert a + b == raw and end2 == end
    s = R.Stream(F, seed)
    assert [s.rand() for _ in range(5)] == [v * F.Rinv % F.p for v in raw[:5]]
    pos = s.pos
    assert s.gen_seed() == chacha.keystream(seed, 32, 32 * pos) and s.pos == pos + 1


def test_planted_seeds_have_their_properties():
    F, F7 = H.FR["bn254"], H.FR["bls12_377"]
    assert not mask_of(F, SEED_CAND0_REJECTED, 1)[0]
    m = mask_of(F, SEED_TILE_EDGE_REJECTED, 257)
    assert not m[255] and not m[256]
    m = mask_of(F, SEED_CHUNK_EDGE, 257)
    assert m[255] and not m[256]
    assert not any(mask_of(F7, SEED_RUN_OF_REJECTIONS, 193)[186:193])


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n,t", SHAPES)
def test_generated_pairs_open_alike_from_both_degrees(curve, n, t):
    F = H.FR[curve]
    parties, shared = R.make_parties(F, n, t, bytes([n, t]) * 16)
    for a in range(n):  # get_shared_rngs: both ends of a pair hold the same seed, and nobody else does
        for b in range(n):
            if a != b:
                assert shared[a][b if b < a else b - 1] == shared[b][a if a < b else a - 1]
    assert len({s for row in shared for s in row}) == n * (n - 1) // 2
    R.run_double_share(parties, 3, n, t)
    R.run_double_share(parties, 2, n, t)  # positions continue, buffers grow
    for ring in range(n):
        from_t, from_2t = R.open_pairs(F, parties, n, t, ring)
        assert from_t == from_2t and len(from_t) == 5 * (t + 1)
    assert len(set(from_t)) == len(from_t)
    # get_pair pops from the back; fork_with_pairs drains the front and draws one seed per stream
    want = [(p.r_t[-1], p.r_2t[-1]) for p in parties]
    assert [p.get_pair() for p in parties] == want
    before = [p.positions() for p in parties]
    kids = [p.fork_with_pairs(2) for p in parties]
    assert [p.positions() for p in parties] == [[x + 1 for x in row] for row in before]
    for ring in (0, n - 1):
        a, b = R.open_pairs(F, kids, n, t, ring)
        assert a == b == from_t[:2]
    R.run_double_share(kids, 1, n, t)  # the children's streams are consistent among themselves
    a, b = R.open_pairs(F, kids, n, t, 0)
    assert a == b and len(a) == 2 + (t + 1)
    with pytest.raises(ValueError):
        R.ShamirRngRef(F, 0, 2 * t, t, [])


# ---- the host self-tests: the functions the kernels call --------------------------------------------------------------------------------
def field_rand_host(hip, curve, seed, begin, n):
    out = np.zeros(4 * n + 4, dtype=np.uint64)
    out[4 * n:] = 0xA5A5A5A5A5A5A5A5
    end = C.c_uint64(0)
    assert hip.lib().csh_selftest_field_rand_host(H.CURVE_IDS[curve], seed, C.c_uint64(begin), C.c_size_t(n), _p(out), C.byref(end)) == 0
    assert (out[4 * n:] == 0xA5A5A5A5A5A5A5A5).all()
    return out[:4 * n], end.value


@pytest.mark.parametrize("curve", CURVES)
def test_field_rand_host_is_the_restatement(hip, curve):
    F = H.FR[curve]
    seeds = PLANTED + [SEED_RUN_OF_REJECTIONS, bytes(range(32))]
    for seed in seeds:
        for begin, n in ((0, 1), (0, 300), (1, 257), (255, 3), (186, 40)):
            raw, end = R.field_rand_ref(F, seed, begin, n)
            got, got_end = field_rand_host(hip, curve, seed, begin, n)
            H.assert_canonical(F, got)
            assert got.tolist() == H.pack(F, raw, mont=False).tolist() and got_end == end, (seed[:1], begin, n)


@pytest.mark.parametrize("curve", CURVES)
def test_candidate_edges(hip, curve):
    """the per-candidate function at the edges of the acceptance test: p - 1 is a draw, p is not; bits above the modulus size are masked
    off before the comparison (p + 2^bits is p again, 2^bits - 1 + 2^255 is the masked all-ones value, which is >= p)"""
    F = H.FR[curve]
    bits = F.p.bit_length()
    cases = [(0, 0), (1, 1), (F.p - 1, F.p - 1), (F.p, None), (F.p + 1, None), ((1 << bits) - 1, None), (F.p - 1 + (1 << bits), F.p - 1 if bits < 256 else None),
             ((1 << 256) - 1, None), (5 + (1 << 255) + (1 << bits), 5)]
    for raw, want in cases:
        out, acc = np.zeros(4, dtype=np.uint64), C.c_int(-1)
        assert hip.lib().csh_selftest_field_rand_candidate(H.CURVE_IDS[curve], (raw % (1 << 256)).to_bytes(32, "little"), _p(out), C.byref(acc)) == 0
        assert acc.value == (want is not None), hex(raw)
        assert R.accepted(F, raw % (1 << 256)) == want  # the restatement takes the same decision
        if want is not None:
            assert int.from_bytes(out.tobytes(), "little") == want


def test_field_rand_plan_and_window_key(hip):
    rates = {"bn254": 0.756, "bls12_381": 0.906, "bls12_377": 0.583}
    for curve, want in rates.items():
        F = H.FR[curve]
        cands, wgs, chunk, rate = hip.field_rand_plan(H.CURVE_IDS[curve], 1000)
        assert abs(rate - F.p / (1 << F.p.bit_length())) < 1e-8 and abs(rate - want) < 1e-3
        assert cands > 1000 / rate and chunk == 256 and wgs == -(-((cands + 1) // 2) // 128)
    cands, wgs, chunk, _ = hip.field_rand_plan(0, 1 << 24)  # the grid cap: at most 1024 chunks, whole tiles each
    assert 1000 < wgs <= 1024 and chunk % 256 == 0 and (wgs - 1) * chunk < cands <= wgs * chunk
    with hip.tuned(vec_max_blocks=2):
        assert hip.field_rand_plan(0, 5000)[1] == 2
    with hip.tuned(field_rand_window=256):
        assert hip.field_rand_plan(0, 1000)[:3] == (256, 1, 256)
    for bad in (1, 255, (1 << 30) + 1, -1):
        with pytest.raises(hip.CoSnarksHipError, match="field_rand_window"):
            hip.tune_set("field_rand_window", bad)
    assert hip.tune_get("field_rand_window") == 0


class HostParty:
    """csh_selftest_shamir_rng_host behind the local / finish interface of shamir_rng_ref.run_double_share"""

    def __init__(self, hip, curve, pid, n, t, seeds, force=0):
        self.hip, self.curve, self.F, self.id, self.n, self.t, self.force = hip, curve, H.FR[curve], pid, n, t, force
        self.seeds = b"".join(seeds)
        self.pos = (C.c_uint64 * (n - 1))()
        self.n_send = (n - t - 2) + (n - 2 * t - 1)
        self.r_t, self.r_2t = [], []

    def _call(self, amount, recv, finish):
        pos = (C.c_uint64 * (self.n - 1))(*self.pos)
        send = np.zeros(4 * max(self.n_send * amount, 1), dtype=np.uint64)
        r_t, r_2t = (np.zeros(4 * amount * (self.t + 1), dtype=np.uint64) for _ in range(2))
        rc = self.hip.lib().csh_selftest_shamir_rng_host(H.CURVE_IDS[self.curve], C.c_uint32(self.id), C.c_uint32(self.n), C.c_uint32(self.t), self.seeds,
                                                        pos, C.c_size_t(amount), self.force, _p(send), _p(recv), int(finish), _p(r_t), _p(r_2t))
        assert rc == 0
        return pos, send, r_t, r_2t

    def local(self, amount):
        self._pos_before = list(self.pos)
        pos, send, _, _ = self._call(amount, None, False)
        self._pos_after = pos
        return [H.unpack(self.F, send[4 * q * amount:4 * (q + 1) * amount]) for q in range(self.n_send)]

    def finish(self, amount, received):
        recv = H.pack(self.F, [v for vec in received for v in vec]) if received else None
        _, _, r_t, r_2t = self._call(amount, recv, True)  # stateless: the draws are made again from the same positions
        self.pos = self._pos_after
        self.r_t += H.unpack(self.F, r_t)
        self.r_2t += H.unpack(self.F, r_2t)

    def positions(self):
        return list(self.pos)


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n,t", SHAPES + [(16, 7)])
def test_shamir_host_stages_are_the_restatement(hip, curve, n, t):
    F = H.FR[curve]
    ref, shared = R.make_parties(F, n, t, bytes([n, t, 7]) * 10 + b"\0\0")
    host = [HostParty(hip, curve, pid, n, t, shared[pid]) for pid in range(n)]
    for amount in (1, 3):
        want_sent, _ = R.run_double_share(ref, amount, n, t)
        got_sent, _ = R.run_double_share(host, amount, n, t)
        assert got_sent == want_sent
        for h, r in zip(host, ref):
            assert h.positions() == r.positions() and h.r_t == r.r_t and h.r_2t == r.r_2t


class ForcedStream:
    def __init__(self, value):
        self.value, self.pos = value, 0

    def rand(self):
        return self.value


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("force", [1, 2])
def test_shamir_host_stages_at_the_edges(hip, curve, force):
    """every draw forced to the limbs 0 and to the limbs p - 1: the matrix stage with the largest operands"""
    F = H.FR[curve]
    n, t = 5, 2
    value = 0 if force == 1 else (F.p - 1) * F.Rinv % F.p
    ref = [R.ShamirRngRef(F, pid, n, t, [ForcedStream(value) for _ in range(n - 1)]) for pid in range(n)]
    host = [HostParty(hip, curve, pid, n, t, [bytes(32)] * (n - 1), force) for pid in range(n)]
    want_sent, _ = R.run_double_share(ref, 2, n, t)
    got_sent, _ = R.run_double_share(host, 2, n, t)
    assert got_sent == want_sent
    for h, r in zip(host, ref):
        assert h.r_t == r.r_t and h.r_2t == r.r_2t
    if force == 1:
        assert all(v == 0 for h in host for v in h.r_t + h.r_2t)


# ---- refusals that need no device, header and bindings --------------------------------------------------------------------------------
def test_refusals_before_any_device_work(hip):
    L = hip.lib()
    err = L.csh_last_error
    seed, out, end = bytes(32), np.zeros(8, dtype=np.uint64), C.c_uint64(0)
    assert L.csh_field_rand_dev(2, seed, C.c_uint64(0), C.c_size_t(1), _p(out), C.byref(end), None) == -1 and b"field_of" in err()
    assert L.csh_field_rand_dev(0, None, C.c_uint64(0), C.c_size_t(1), _p(out), C.byref(end), None) == -1 and b"NULL" in err()
    assert L.csh_field_rand_dev(0, seed, C.c_uint64(0), C.c_size_t(1), None, C.byref(end), None) == -1 and b"NULL" in err()
    assert L.csh_field_rand_dev(0, seed, C.c_uint64(0), C.c_size_t((1 << 28) + 1), _p(out), C.byref(end), None) == -1 and b"2^28" in err()
    assert L.csh_field_rand_dev(0, seed, C.c_uint64((1 << 62) + 1), C.c_size_t(1), _p(out), C.byref(end), None) == -1 and b"2^62" in err()
    assert L.csh_field_rand_dev(0, seed, C.c_uint64(77), C.c_size_t(0), None, C.byref(end), None) == 0 and end.value == 77  # nothing drawn, no device asked for
    h = C.c_void_p()
    mk = lambda pid, n, t: L.csh_shamir_rng_create(0, C.c_uint32(pid), C.c_uint32(n), C.c_uint32(t), bytes(32 * 16), None, C.byref(h))
    assert mk(0, 4, 2) == -1 and b"2 * threshold + 1" in err()
    assert mk(0, 17, 1) == -1 and b"16" in err()
    assert mk(3, 3, 1) == -1 and b"id" in err()
    assert mk(0, 3, 0) == -1 and b"threshold" in err()
    assert L.csh_shamir_rng_create(2, C.c_uint32(0), C.c_uint32(3), C.c_uint32(1), bytes(64), None, C.byref(h)) == -1 and b"field_of" in err()
    assert L.csh_shamir_rng_create(0, C.c_uint32(0), C.c_uint32(3), C.c_uint32(1), None, None, C.byref(h)) == -1 and b"NULL" in err()
    assert L.csh_shamir_double_share_local_dev(None, C.c_size_t(1), None, None) == -1 and b"handle" in err()
    assert L.csh_shamir_double_share_finish_dev(None, C.c_size_t(1), None, None) == -1 and b"handle" in err()
    assert L.csh_shamir_pairs_take_dev(None, C.c_size_t(1), 0, None, None, None) == -1 and b"handle" in err()
    assert L.csh_shamir_rng_destroy(None) == 0
    with pytest.raises(hip.CoSnarksHipError, match="32 bytes"):
        hip.field_rand(0, bytes(31), 0, 1)
    with pytest.raises(hip.CoSnarksHipError, match="cand_begin"):
        hip.field_rand(0, bytes(32), -1, 1)
    with pytest.raises(hip.CoSnarksHipError, match="threshold"):
        hip.ShamirRng(0, 0, 4, 2, [bytes(32)] * 3)
    with pytest.raises(hip.CoSnarksHipError, match="16"):
        hip.ShamirRng(0, 0, 17, 1, [bytes(32)] * 16)
    with pytest.raises(hip.CoSnarksHipError, match="num_parties - 1 seeds"):
        hip.ShamirRng(0, 0, 3, 1, [bytes(32)] * 3)


def test_header_and_bindings_declare_the_entry_points(hip):
    from cosnarks_amd import bindings
    txt = open(bindings.header_path()).read()
    declared = bindings.declared_symbols()
    src = open(bindings.__file__).read()
    cites = {"csh_field_rand_dev": ["rep3.rs:185-196", "rngs.rs:334-428", "PARITY UNPINNED", "SYNCHRONISES"],
             "csh_shamir_rng_create": ["rngs.rs:98-139", "shamir.rs:503-525", "rngs.rs:147-158", "shamir.rs:41-43", "limit of this library"],
             "csh_shamir_rng_fork_seeds": ["rngs.rs:76-79"],
             "csh_shamir_double_share_local_dev": ["rngs.rs:334-395", "rngs.rs:344-384", "rngs.rs:291-311"],
             "csh_shamir_double_share_finish_dev": ["rngs.rs:390-427", "chunks_exact_mut"],
             "csh_shamir_pairs_take_dev": ["shamir/network.rs:150-167", "rngs.rs:93-94"]}
    L = hip.lib()
    for name, cs in cites.items():
        assert name in declared and hasattr(L, name), name
        at = txt.index("int %s(" % name)
        comment = txt[txt.rindex("/*", 0, at):at]
        for c in cs:
            assert c in comment, (name, c)
        assert "lib().%s(" % name in src
    for name in ("csh_field_rand_plan", "csh_shamir_rng_destroy", "csh_shamir_rng_positions", "csh_shamir_pairs_len"):
        assert name in declared and hasattr(L, name) and "lib().%s(" % name in src
    for name in ("csh_selftest_field_rand_host", "csh_selftest_field_rand_candidate", "csh_selftest_shamir_rng_host"):
        assert name not in declared and hasattr(L, name)
