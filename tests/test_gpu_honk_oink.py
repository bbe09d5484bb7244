"""Device tests of the Oink entries (csrc/honk_oink.hip): csh_honk_w4_records_dev, csh_honk_lookup_operands_dev,
csh_honk_perm_operands_dev and csh_honk_z_perm_place_dev against tests/honk_oink_ref.py, and the closed permutation and lookup chains
through device entry points only. Every comparison is exact and covers every element; every output has guard words behind it."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import helpers as H
from tests import honk_oink_ref as R

pytestmark = pytest.mark.gpu
CURVES = ["bn254", "bls12_381", "bls12_377"]
PARTIES = [(0, 0), (1, 0), (1, 1), (1, 2)]   # (protocol, party)
GUARD = np.uint64(0x5A5AC3C3A5A53C3C)
sz, u32 = C.c_size_t, C.c_uint32
# n = 16: none; three ranges with two gaps; a set starting at 1 (index 1 takes no quotient: position 0); a set starting at 2 (index 1 is
# inactive and keeps the one)
RANGE_SETS_16 = [None, R.RANGES_3, [(1, 4), (4, 9), (12, 15)], [(2, 6), (9, 16)]]


def _vec(F, v):
    return H.pack(F, R.flat(v))


def _up(hip, arr):
    return hip.DeviceBuffer.from_host(arr)


def _out(hip, ncomp, count, guard=8):
    """an output buffer of `count` shares filled with the guard word, `guard` words of it behind"""
    return _up(hip, np.full(4 * ncomp * count + guard, GUARD, dtype=np.uint64))


def _with_guard(hip, arr, guard=8):
    return _up(hip, np.concatenate([arr, np.full(guard, GUARD, dtype=np.uint64)]))


def _down(F, T, buf, count, guard=8):
    """-> the shares, after checking that the words behind them still hold the guard (nothing written past the end)"""
    raw = buf.to_host()
    assert raw.size == 4 * T.ncomp * count + guard and (raw[4 * T.ncomp * count:] == GUARD).all(), "written past the end of an output"
    v = H.unpack(F, raw[:4 * T.ncomp * count])   # strict: canonical
    return [tuple(v[i * T.ncomp:(i + 1) * T.ncomp]) for i in range(count)]


def first_difference(got, want):
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            return i
    return None


def same(got, want, what):
    assert len(got) == len(want) and got == want, (what, "first difference at share", first_difference(got, want), "of", len(want))


def dev_w4(hip, curve, T, c):
    F, n = H.FR[curve], c["n"]
    w4 = _with_guard(hip, _vec(F, c["w"][3]))
    rec = hip.HonkMemoryRecords(n, *c["records"])
    ts = _up(hip, _vec(F, c["type_share"])) if c["type_share"] else None
    hip.honk_w4_records(H.CURVE_IDS[curve], T.protocol, T.party, [_up(hip, _vec(F, c["w"][k])) for k in range(3)], w4, n, H.pack(F, c["etas"]), rec, ts)
    hip.bindings.sync()
    return _down(F, T, w4, n)


def dev_lookup(hip, curve, T, c):
    F, n = H.FR[curve], c["n"]
    outs = [_out(hip, T.ncomp, n) for _ in range(2)]
    shares = [_up(hip, _vec(F, v)) for v in c["w"][:3] + [c["tags"]]]
    public = [_up(hip, H.pack(F, v)) for v in c["q"] + c["tables"] + [c["q_lookup"]]]
    hip.honk_lookup_operands(H.CURVE_IDS[curve], T.protocol, T.party, shares, public, n, H.pack(F, c["ch"]), outs)
    hip.bindings.sync()
    return tuple(_down(F, T, o, n) for o in outs)


def dev_perm(hip, curve, T, c):
    F, n = H.FR[curve], c["n"]
    m = len(c["want_perm"][0])
    outs = [_out(hip, T.ncomp, m) for _ in range(8)]
    shares = [_up(hip, _vec(F, v)) for v in c["w"]]
    public = [_up(hip, H.pack(F, v)) for v in c["ident"] + c["sigma"]]
    hip.honk_perm_operands(H.CURVE_IDS[curve], T.protocol, T.party, shares, public, n, c["domain_size"], c["ranges"], H.pack(F, c["ch"]), outs)
    hip.bindings.sync()
    return [_down(F, T, o, m) for o in outs]


def dev_place(hip, curve, T, c):
    F, n = H.FR[curve], c["n"]
    z = _out(hip, T.ncomp, n)
    mul = _up(hip, _vec(F, c["mul"])) if c["mul"] else None
    hip.honk_z_perm_place(H.CURVE_IDS[curve], T.protocol, T.party, mul, z, n, c["domain_size"], c["ranges"])
    hip.bindings.sync()
    return _down(F, T, z, n)


def check_entries(hip, curve, T, c, what=None):
    same(dev_w4(hip, curve, T, c), c["want_w4"], ("w4", what))
    for name, g, w in zip(("prod", "sel"), dev_lookup(hip, curve, T, c), c["want_lookup"]):
        same(g, w, (name, what))
    check_perm_and_place(hip, curve, T, c, what)


def check_perm_and_place(hip, curve, T, c, what=None):
    for name, g, w in zip(("n1", "n2", "n3", "n4", "d1", "d2", "d3", "d4"), dev_perm(hip, curve, T, c), c["want_perm"]):
        same(g, w, (name, what))
    same(dev_place(hip, curve, T, c), c["want_z"], ("z_perm", what))


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("protocol,party", PARTIES)
def test_every_entry_at_one_ragged_workgroup(gpu, curve, protocol, party):
    """n = 16: one ragged workgroup and the shifted read at the last row; w4 and lookup once, the range entries for every range set"""
    F, T = H.FR[curve], R.Ops(H.FR[curve].p, protocol, party)
    r = H.rng(8000 + 10 * protocol + party)
    for j, ranges in enumerate(RANGE_SETS_16):
        c = R.entries_case(F.p, T, 16, lambda: r.randrange(F.p), 16 if ranges else 13, ranges)
        (check_entries if j == 0 else check_perm_and_place)(gpu, curve, T, c, ranges)


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("protocol,party", PARTIES)
def test_thirty_two_single_row_ranges(gpu, curve, protocol, party):
    """n = 64, every second row a range of its own: the most ranges a call takes, every gap one row wide"""
    F, T = H.FR[curve], R.Ops(H.FR[curve].p, protocol, party)
    r = H.rng(8100 + 10 * protocol + party)
    c = R.entries_case(F.p, T, 64, lambda: r.randrange(F.p), 61, [(2 * j, 2 * j + 1) for j in range(32)])
    check_perm_and_place(gpu, curve, T, c)


@functools.lru_cache(maxsize=None)
def large_case(curve, protocol, party):
    """n = 1000; ranges with gaps (and one pair that touches); 37 read, 41 write and 5 shared records with rows 0 and n - 1 among them"""
    F, T = H.FR[curve], R.Ops(H.FR[curve].p, protocol, party)
    r = H.rng(9000)
    n = 1000
    rows = [0, n - 1] + r.sample(range(1, n - 1), 81)
    r.shuffle(rows)
    records = (rows[:37], rows[37:78], rows[78:])
    ranges = [(3, 260), (260, 301), (400, 401), (517, 777), (900, 1000)]
    return T, R.entries_case(F.p, T, n, lambda: r.randrange(F.p), 950, ranges, records=records)


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("protocol,party", PARTIES)
def test_capped_grids(gpu, curve, protocol, party):
    """n = 1000 with one and three workgroups: every grid-stride loop makes several passes with a ragged last one"""
    T, c = large_case(curve, protocol, party)
    assert [len(v) for v in c["records"]] == [37, 41, 5] and {0, 999} <= set(sum(c["records"], []))
    for mb in (1, 3):
        with gpu.tuned(vec_max_blocks=mb):
            check_entries(gpu, curve, T, c, mb)


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("protocol,party", PARTIES)
def test_edges_of_the_field(gpu, curve, protocol, party):
    """every share, public input and challenge p - 1"""
    F, T = H.FR[curve], R.Ops(H.FR[curve].p, protocol, party)
    check_entries(gpu, curve, T, R.entries_case(F.p, T, 16, lambda: F.p - 1, 16, R.RANGES_3))


def test_no_record_and_no_quotient_do_nothing(gpu):
    """all three record counts zero: w_4 untouched; m = 0: no operand written, and the placement leaves zeros and the one"""
    F, T = H.FR["bn254"], R.Ops(H.FR["bn254"].p, 1, 0)
    r = H.rng(5)
    c = R.entries_case(F.p, T, 2, lambda: r.randrange(F.p), 1, None, records=([], [], []))
    assert c["want_w4"] == c["w"][3] and c["mul"] == [] and c["want_z"] == [(0, 0), (1, 0)]
    same(dev_w4(gpu, "bn254", T, c), c["want_w4"], "w4")
    check_perm_and_place(gpu, "bn254", T, c)


# ---- the closed chains through device entries only ------------------------------------------------------------------------------------------
def _mul(hip, cid, x, y, n):
    out = hip.DeviceBuffer(32 * n)
    assert hip.lib().csh_vec_mul_dev(cid, x.ptr, y.ptr, out.ptr, sz(n), None) == 0
    return out


@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
@pytest.mark.parametrize("with_ranges", [False, True])
def test_closed_permutation_chain(gpu, curve, with_ranges):
    """plain protocol: operands -> vec_mul -> prefix_prod -> batch_inverse -> vec_mul -> place. z_perm satisfies the closed form of a
    satisfied permutation and is the restatement's bit for bit."""
    hip, F, cid = gpu, H.FR[curve], H.CURVE_IDS[curve]
    p, T = F.p, R.Ops(F.p, 0, 0)
    c = R.perm_closed(p, with_ranges)
    n, m = c["n"], len(c["ops"][0])
    shares = [_up(hip, H.pack(F, v)) for v in c["w"]]
    public = [_up(hip, H.pack(F, v)) for v in c["ident"] + c["sigma"]]
    ops = hip.honk_perm_operands(cid, 0, 0, shares, public, n, c["domain_size"], c["ranges"], H.pack(F, [c["beta"], c["gamma"]]),
                                 [hip.DeviceBuffer(32 * m) for _ in range(8)])
    num = hip.vec_prefix_prod(cid, _mul(hip, cid, _mul(hip, cid, ops[0], ops[1], m), _mul(hip, cid, ops[2], ops[3], m), m), m)
    den, _ = hip.vec_batch_inverse(cid, hip.vec_prefix_prod(cid, _mul(hip, cid, _mul(hip, cid, ops[4], ops[5], m), _mul(hip, cid, ops[6], ops[7], m), m), m), m)
    z = hip.honk_z_perm_place(cid, 0, 0, _mul(hip, cid, num, den, m), _out(hip, 1, n), n, c["domain_size"], c["ranges"])
    hip.bindings.sync()
    for g, w in zip(ops, c["ops"]):
        assert H.unpack(F, g.to_host()) == w
    got = [x[0] for x in _down(F, T, z, n)]
    R.check_perm_closed_form(p, got, c["w"], c["ident"], c["sigma"], c["beta"], c["gamma"], c["rows"], n, c["ranges"])
    assert got == c["z"]


@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
def test_closed_lookup_chain(gpu, curve):
    """plain protocol: operands -> vec_mul -> batch_inverse (a zero stays zero). I != 0 exactly where q_lookup or the tag is one, the
    log-derivative sum vanishes, and I is the restatement's bit for bit."""
    hip, F, cid = gpu, H.FR[curve], H.CURVE_IDS[curve]
    p = F.p
    c = R.lookup_closed(p)
    n = c["n"]
    shares = [_up(hip, H.pack(F, v)) for v in c["w"] + [c["tags"]]]
    public = [_up(hip, H.pack(F, v)) for v in c["q"] + c["tables"] + [c["q_lookup"]]]
    prod, sel = hip.honk_lookup_operands(cid, 0, 0, shares, public, n, H.pack(F, [c["beta"], c["gamma"]]), [hip.DeviceBuffer(32 * n) for _ in range(2)])
    inv, _ = hip.vec_batch_inverse(cid, _mul(hip, cid, prod, sel, n), n)
    hip.bindings.sync()
    got = dict(c, prod=H.unpack(F, prod.to_host()), sel=H.unpack(F, sel.to_host()), inv=H.unpack(F, inv.to_host()))
    R.check_lookup_closed_form(p, got)
    assert (got["prod"], got["sel"], got["inv"]) == (c["prod"], c["sel"], c["inv"])


def test_refusals_leave_device_buffers_untouched(gpu):
    """overlap rules on device addresses: a refused call writes nothing; buffers next to each other are no overlap"""
    L = gpu.lib()
    n = 16
    fill = np.arange(4 * 2 * n * 24, dtype=np.uint64)
    pool = gpu.DeviceBuffer.from_host(fill)
    vb = 32 * 2 * n
    slot = lambda k: pool.ptr.value + k * vb
    arr = lambda addrs: (C.c_void_p * len(addrs))(*addrs)
    host = np.ones(4 * 8, dtype=np.uint64)
    hp = host.ctypes.data_as(C.c_void_p)
    err = lambda: L.csh_last_error()
    sh4, pub8, out8 = [slot(k) for k in range(4)], [slot(4 + k) for k in range(8)], [slot(12 + k) for k in range(8)]
    swap = lambda lst, k, v: lst[:k] + [v] + lst[k + 1:]

    def pm(outs):
        return L.csh_honk_perm_operands_dev(0, u32(1), u32(0), arr(sh4), arr(pub8), sz(n), sz(n), None, sz(0), hp, arr(outs), None)

    def pl(mul, z):
        return L.csh_honk_z_perm_place_dev(0, u32(1), u32(0), C.c_void_p(mul), C.c_void_p(z), sz(n), sz(n), None, sz(0), None)

    for call, msg in ((lambda: pm(swap(out8, 0, slot(3) + vb - 32)), b"overlaps an input"),            # n_1 begins in w_4's last share
                      (lambda: pm(swap(out8, 7, slot(11) + 32 * n - 32)), b"overlaps an input"),       # d_4 begins in sigma_4's last element
                      (lambda: pm(swap(out8, 5, slot(12) + vb - 96)), b"two outputs overlap"),         # d_2 begins in n_1's last share (m = n - 1)
                      (lambda: pl(slot(0), slot(0) + vb - 96), b"overlaps an input")):
        rc = call()
        assert rc == -1 and msg in err(), (msg, err())
    gpu.bindings.sync()
    assert (pool.to_host() == fill).all(), "a refused call wrote to its buffers"
    assert pm(out8) == 0 and pl(slot(0), slot(0) + vb - 64) == 0   # z directly behind the m = n - 1 shares of mul
    gpu.bindings.sync()
