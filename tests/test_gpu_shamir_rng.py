"""Device tests of csh_field_rand_dev and the DN07 double-share stages (csrc/field_rand.hip, csrc/shamir_rng.hip) against the big-integer
restatement of tests/shamir_rng_ref.py: every output word-exact, guard words behind every output. The restatement is held against the
protocol's own property in tests/test_shamir_rng_cpu.py. Parity with ark-ff's sampler is by restatement only (PARITY UNPINNED)."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import helpers as H
from tests import shamir_rng_ref as R
from tests.test_shamir_rng_cpu import PLANTED, SEED_CAND0_REJECTED, SEED_CHUNK_EDGE, SEED_RUN_OF_REJECTIONS, SEED_TILE_EDGE_REJECTED

pytestmark = pytest.mark.gpu

GUARD = np.uint64(0xC3C3C3C3C3C3C3C3)
GENERIC = bytes(range(100, 132))


@functools.lru_cache(maxsize=None)
def ref_draws(curve, seed, begin, n):
    raw, end = R.field_rand_ref(H.FR[curve], seed, begin, n)
    return H.pack(H.FR[curve], raw, mont=False).tolist(), end


def guarded(gpu, n_elems):
    """a device buffer of n_elems elements followed by four guard words, all set to the guard pattern"""
    return gpu.DeviceBuffer.from_host(np.full(4 * n_elems + 4, GUARD, dtype=np.uint64))


def read_guarded(buf, n_elems):
    a = buf.to_host()
    assert (a[4 * n_elems:] == GUARD).all(), "the guard words behind the output were written"
    return a[:4 * n_elems]


def draw(gpu, curve, seed, begin, n):
    buf = guarded(gpu, n)
    _, end = gpu.field_rand(H.CURVE_IDS[curve], seed, begin, n, out=buf)
    got = read_guarded(buf, n)
    H.assert_canonical(H.FR[curve], got)
    return got.tolist(), end


def check(gpu, curve, seed, begin, n):
    assert draw(gpu, curve, seed, begin, n) == ref_draws(curve, seed, begin, n), (curve, seed[:1], begin, n)


# ---- csh_field_rand_dev ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 1000])
def test_field_rand_sizes_and_planted_seeds(gpu, n):
    if n == 1000:  # more than one workgroup, chunks of one tile: SEED_CHUNK_EDGE has the last candidate of chunk 0 accepted, the first of chunk 1 rejected
        cands, wgs, chunk, _ = gpu.field_rand_plan(0, n)
        assert wgs > 1 and chunk == 256
    for seed in PLANTED + [GENERIC]:
        check(gpu, "bn254", seed, 0, n)


@pytest.mark.parametrize("cap", [1, 2])
def test_field_rand_over_a_capped_grid(gpu, cap):
    with gpu.tuned(vec_max_blocks=cap):
        assert gpu.field_rand_plan(0, 5000)[1] == cap
        for seed in (GENERIC, SEED_CHUNK_EDGE):
            check(gpu, "bn254", seed, 0, 5000)


def test_field_rand_begins(gpu):
    for seed, begin in ((GENERIC, 0), (GENERIC, 7), (GENERIC, 1 << 40), (SEED_CAND0_REJECTED, 0), (SEED_TILE_EDGE_REJECTED, 255), (SEED_TILE_EDGE_REJECTED, 256),
                        (SEED_CHUNK_EDGE, 256), (SEED_CHUNK_EDGE, 255)):
        for n in (1, 300):
            check(gpu, "bn254", seed, begin, n)
    buf = guarded(gpu, 1)
    assert gpu.field_rand(0, GENERIC, 77, 0, out=buf)[1] == 77 and (buf.to_host() == GUARD).all()  # nothing drawn, nothing written


def test_field_rand_two_calls_are_one(gpu):
    for curve in ("bn254", "bls12_377"):
        whole, end = ref_draws(curve, GENERIC, 3, 1000)
        a, mid = draw(gpu, curve, GENERIC, 3, 300)
        b, got_end = draw(gpu, curve, GENERIC, mid, 700)
        assert a + b == whole and got_end == end and mid == ref_draws(curve, GENERIC, 3, 300)[1]


def test_field_rand_smallest_window(gpu):
    """tune "field_rand_window" at its minimum: 1000 draws take at least three windows (four candidates of five are accepted at best)"""
    with gpu.tuned(field_rand_window=256):
        assert gpu.field_rand_plan(0, 1000)[0] == 256
        for seed in PLANTED + [GENERIC]:
            check(gpu, "bn254", seed, 0, 1000)
        check(gpu, "bn254", GENERIC, 129, 257)
        check(gpu, "bls12_377", SEED_RUN_OF_REJECTIONS, 0, 600)


@pytest.mark.parametrize("curve", ["bls12_381", "bls12_377"])
def test_field_rand_on_the_other_fields(gpu, curve):
    for seed in (GENERIC, SEED_RUN_OF_REJECTIONS):
        for begin, n in ((0, 1), (0, 257), (186, 257)):
            check(gpu, curve, seed, begin, n)


# ---- the double-share stages -------------------------------------------------------------------------------------------------------------
class DevParty:
    """csh_shamir_rng_t behind the local / finish interface of shamir_rng_ref.run_double_share"""

    def __init__(self, gpu, curve, pid, n, t, seeds):
        self.gpu, self.F = gpu, H.FR[curve]
        self.rng = gpu.ShamirRng(H.CURVE_IDS[curve], pid, n, t, seeds)

    def local(self, amount):
        k = self.rng.n_send
        send = guarded(self.gpu, k * amount) if k else None
        self.rng.double_share_local(amount, send)
        if not k:
            return []
        got = H.unpack(self.F, read_guarded(send, k * amount))
        return [got[q * amount:(q + 1) * amount] for q in range(k)]

    def finish(self, amount, received):
        recv = self.gpu.DeviceBuffer.from_host(H.pack(self.F, [v for vec in received for v in vec])) if received else None
        self.rng.double_share_finish(amount, recv)

    def positions(self):
        return self.rng.positions()

    def take(self, count, from_front=False):
        r_t, r_2t = guarded(self.gpu, count), guarded(self.gpu, count)
        self.rng.take(count, from_front, r_t, r_2t)
        return H.unpack(self.F, read_guarded(r_t, count)), H.unpack(self.F, read_guarded(r_2t, count))


def parties_for(gpu, curve, n, t, on_device, master=b"\x2a" * 32):
    ref, shared = R.make_parties(H.FR[curve], n, t, master)
    twin, _ = R.make_parties(H.FR[curve], n, t, master)
    mixed = [DevParty(gpu, curve, pid, n, t, shared[pid]) if pid in on_device else twin[pid] for pid in range(n)]
    return ref, mixed


@pytest.mark.parametrize("curve,n,t,on_device", [("bn254", 3, 1, (0, 1, 2)), ("bn254", 5, 2, (0, 1, 2, 3, 4)), ("bn254", 4, 1, (0, 3)),
                                                 ("bls12_381", 5, 2, (0, 4)), ("bls12_377", 3, 1, (1,))])
def test_double_share_stages(gpu, curve, n, t, on_device):
    """amounts 1, 2, 129 and 1000 one after the other on the same handles: the wire vectors, the positions and the lengths after every
    call, the appended buffers at the end (a drain of everything). Parties not on the device are the restatement's."""
    ref, mixed = parties_for(gpu, curve, n, t, on_device)
    total = 0
    for amount in (1, 2, 129, 1000) if curve == "bn254" else (1, 129):
        want_sent, _ = R.run_double_share(ref, amount, n, t)
        got_sent, _ = R.run_double_share(mixed, amount, n, t)
        assert got_sent == want_sent, amount
        total += amount * (t + 1)
        for pid in on_device:
            assert mixed[pid].positions() == ref[pid].positions() and len(mixed[pid].rng) == total
    for pid in on_device:
        assert mixed[pid].take(total, from_front=True) == (ref[pid].r_t, ref[pid].r_2t), pid
        assert len(mixed[pid].rng) == 0


def test_take(gpu):
    n, t = 3, 1
    ref, dev = parties_for(gpu, "bn254", n, t, (0, 1, 2))
    R.run_double_share(ref, 10, n, t)
    R.run_double_share(dev, 10, n, t)
    for r, d in zip(ref, dev):
        pops = [r.get_pair() for _ in range(3)]
        assert d.take(3) == ([a for a, _ in pops], [b for _, b in pops])
        kid = r.fork_with_pairs(4)
        assert d.take(4, from_front=True) == (kid.r_t, kid.r_2t)
        assert d.rng.fork_seeds() == [s.seed for s in kid.shared_rngs] and d.positions() == r.positions()
        assert len(d.rng) == 13
        with pytest.raises(gpu.CoSnarksHipError, match="14 pairs asked for, 13 present"):
            d.rng.take(14)
        assert len(d.rng) == 13  # refused, nothing changed
        pops = [r.get_pair() for _ in range(13)]
        assert d.take(13) == ([a for a, _ in pops], [b for _, b in pops]) and len(d.rng) == 0
        assert d.rng.take(0)[0] is not None and len(d.rng) == 0
    R.run_double_share(ref, 5, n, t)  # after a drain and an emptied buffer the next pairs land where the reference puts them
    R.run_double_share(dev, 5, n, t)
    for r, d in zip(ref, dev):
        assert d.take(10, from_front=True) == (r.r_t, r.r_2t)


@pytest.mark.parametrize("n,t", [(3, 1), (5, 2)])
def test_mul_vec_chain_on_generated_pairs(gpu, n, t):
    """generated pairs -> csh_vec_mul_dev + csh_vec_add_dev (r_2t) on the device; the king's reconstruction and the reshare are this
    test's network; csh_vec_sub_dev (r_t) must open to the product of the opened inputs"""
    F, L, m = H.FR["bn254"], gpu.lib(), 7
    p = F.p
    rnd = H.rng(n)
    _, dev = parties_for(gpu, "bn254", n, t, tuple(range(n)), master=b"\x07" * 32)
    R.run_double_share(dev, -(-m // (t + 1)), n, t)
    a, b = H.rand_elems(F, m, rnd), H.rand_elems(F, m, rnd)

    def share(v):  # a random degree-t polynomial with the secret at 0, evaluated at 1 .. n
        poly = [v] + H.rand_elems(F, t, rnd)
        return [R.evaluate_poly(F, poly, x) for x in range(1, n + 1)]

    sa, sb = [share(v) for v in a], [share(v) for v in b]
    up = lambda vals: gpu.DeviceBuffer.from_host(H.pack(F, vals))
    masked, r_ts = [], []
    for pid in range(n):
        da, db, prod = up([s[pid] for s in sa]), up([s[pid] for s in sb]), guarded(gpu, m)
        r_t, r_2t = dev[pid].rng.take(m)
        assert L.csh_vec_mul_dev(0, da.ptr, db.ptr, prod.ptr, C.c_size_t(m), None) == 0
        assert L.csh_vec_add_dev(0, prod.ptr, r_2t.ptr, prod.ptr, C.c_size_t(m), C.c_uint32(1), None) == 0
        masked.append(H.unpack(F, read_guarded(prod, m)))
        r_ts.append(r_t)
    lag = R.lagrange_from_coeff(F, list(range(1, 2 * t + 2)))  # mul_lagrange_2t: the king opens from parties 0 .. 2t
    z = [sum(l * masked[pid][k] for pid, l in enumerate(lag)) % p for k in range(m)]
    opened = []
    for pid in range(n):  # the king's fresh degree-t sharing of the public z (here: the constant polynomial), minus r_t on the device
        dz, out = up(z), guarded(gpu, m)
        assert L.csh_vec_sub_dev(0, dz.ptr, r_ts[pid].ptr, out.ptr, C.c_size_t(m), C.c_uint32(1), None) == 0
        opened.append(H.unpack(F, read_guarded(out, m)))
    lag_t = R.lagrange_from_coeff(F, list(range(1, t + 2)))
    for ids in (range(t + 1),):
        got = [sum(l * opened[pid][k] for pid, l in zip(ids, lag_t)) % p for k in range(m)]
        assert got == [x * y % p for x, y in zip(a, b)]
    last = list(range(n - t - 1, n))
    lag_last = R.lagrange_from_coeff(F, [i + 1 for i in last])
    assert [sum(l * opened[pid][k] for pid, l in zip(last, lag_last)) % p for k in range(m)] == [x * y % p for x, y in zip(a, b)]


def test_refusals_on_the_device(gpu):
    L = gpu.lib()
    err = L.csh_last_error
    five = gpu.ShamirRng(0, 0, 5, 2, [bytes([q]) * 32 for q in range(4)])
    assert L.csh_shamir_double_share_finish_dev(five.h, C.c_size_t(1), None, None) == -1 and b"local stage" in err()
    assert L.csh_shamir_double_share_local_dev(five.h, C.c_size_t(1), None, None) == -1 and b"send_dev is NULL" in err()
    assert L.csh_shamir_double_share_local_dev(five.h, C.c_size_t(0), None, None) == -1 and b"amount" in err()
    assert L.csh_shamir_double_share_local_dev(five.h, C.c_size_t((1 << 24) + 1), None, None) == -1 and b"amount" in err()
    assert five.positions() == [0, 0, 0, 0]
    send = five.double_share_local(2)
    pos = five.positions()
    assert min(pos) > 0
    assert L.csh_shamir_double_share_local_dev(five.h, C.c_size_t(2), send.ptr, None) == -1 and b"has not been finished" in err()
    assert L.csh_shamir_double_share_finish_dev(five.h, C.c_size_t(3), send.ptr, None) == -1 and b"local stage" in err()
    assert L.csh_shamir_double_share_finish_dev(five.h, C.c_size_t(2), None, None) == -1 and b"recv_dev is NULL" in err()
    assert five.positions() == pos and len(five) == 0
    five.double_share_finish(2, send)
    assert len(five) == 6
    out = gpu.DeviceBuffer(32 * 8)
    assert L.csh_shamir_pairs_take_dev(five.h, C.c_size_t(2), 0, None, out.ptr, None) == -1 and b"NULL output" in err()
    assert L.csh_shamir_pairs_take_dev(five.h, C.c_size_t(7), 0, out.ptr, out.ptr, None) == -1 and b"7 pairs asked for, 6 present" in err()
    assert len(five) == 6
