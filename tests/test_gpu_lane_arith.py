"""Device unit tests of the arithmetic that exists on the device only -- curve_quad.hpp (one XYZZ point over a DPP quad: qadd, qdbl,
qmul_small) and curve_pair.hpp (Fp2Pair: one Fp2 value over a lane pair) -- and of the MSM tail stages built on it (k_msm_reduce,
k_msm_reduce_serial, k_msm_reduce_pair, k_msm_fold_tree), through the entry points of csrc/selftest_dev.hip.

Every comparison is exact: group equality with the Python oracle on the affine result, equality of Montgomery words, integer counters
equal to zero. The kernels of selftest_dev.hip are compiled with the device form of the limb-bound contract (field29.hpp): each launch
returns the record (violating limbs, largest |limb|, site = line of field29.hpp), which must be empty."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import curves as cv
from tests import helpers as H

pytestmark = pytest.mark.gpu

GROUPS = [("bn254", 0), ("bn254", 1), ("bls12_381", 0), ("bls12_381", 1), ("grumpkin", 0), ("bls12_377", 0), ("bls12_377", 1)]
G2_CURVES = ["bn254", "bls12_381", "bls12_377"]
FORM_SERIAL, FORM_QUAD, FORM_PAIR = 0, 1, 2
# (group, form) of the scripted point operations: every group over a quad (the G2 groups too: k_msm_fold_tree and the quad reduction
# run QPt<Fp2S>), the G2 groups over a lane pair
POINT_FORMS = [(c, g, FORM_QUAD) for c, g in GROUPS] + [(c, 1, FORM_PAIR) for c in G2_CURVES]
TAIL_FORMS = [(c, g, f) for c, g in GROUPS for f in ((FORM_SERIAL, FORM_QUAD, FORM_PAIR) if g else (FORM_SERIAL, FORM_QUAD))]

LOAD, ADDP, ADDR, ADDS, DBL, MULK, MADD, ADDK = range(8)                # StOp codes of selftest_dev.hip
SMALL_K = [0, 1, 2, 3, 5, 1 << 15, (1 << 16) + 1, (1 << 21) - 1, 1 << 21]

_FIELD29 = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "co-snarks_amd", "csrc", "field29.hpp")


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _err(hip):
    return hip.lib().csh_last_error().decode(errors="replace")


def _site(line):
    try:
        return open(_FIELD29).read().split("\n")[line - 1].strip()
    except (OSError, IndexError):
        return "?"


def _assert_no_bound_violation(rec, what):
    n, limb, line = (int(x) for x in rec)
    assert n == 0, "%s: %d operand limbs outside their bound, largest |limb| = %d (2^%.2f) at field29.hpp:%d  %s" % (
        what, n, limb, np.log2(max(limb, 1)), line, _site(line))


_xyzz_to_affine = H.xyzz_to_affine                                         # shared with tests/test_gpu_msm_buckets.py


def _xyzz_words(hip, curve, group):
    return 2 * hip.point_bytes(H.CURVE_IDS[curve], group) // 8


_known_points = H.known_points


# ---- 1(a): the recorder itself ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("typ,B,NL", [(0, 29, 9), (1, 28, 14), (2, 29, 9), (3, 28, 14)], ids=["Fq29s", "Fq28s", "Fr29s", "Fq28s377"])
def test_bound_recorder_reports_an_oversized_operand(gpu, typ, B, NL):
    """Positive control: a raw-limb product whose first operand has every limb at 2^(B+2) (integer arithmetic on chosen inputs) must be
    recorded -- 64 lanes x NL limbs, the limb value, and the site of mul_wide's first-operand bound. A dead recorder cannot pass."""
    rec = (C.c_uint64 * 3)()
    assert gpu.lib().csh_selftest_bound_control_dev(typ, rec) == 0
    assert rec[0] == 64 * NL and rec[1] == 1 << (B + 2), list(rec)
    assert "mul_wide(a)" in _site(int(rec[2])), (int(rec[2]), _site(int(rec[2])))
    assert gpu.lib().csh_selftest_bound_control_dev(typ, rec) == 0      # and the record was cleared in between: the same count again
    assert rec[0] == 64 * NL


# ---- 1(b): Fp2Pair products on raw limbs ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", G2_CURVES)
def test_fp2pair_products_at_the_edge_of_their_column_bound(gpu, curve):
    """Fp2Pair mul / sqr / sqr_sub / mul_sub on raw signed limbs, limbs 0 .. NL-2 at +/-(2^B + 8): the device twin of
    test_lazy_fp2_products_at_the_edge_of_their_column_bound. One launch of 384 pairs, every pair with its own operands (a wrong quad_perm
    control reads the neighbouring pair), against big-integer arithmetic on the values the limbs spell. With NR = 5 (BLS12-377) the
    operand hi_signed() moves is five times a normalised one: its bound is LIM_SCALED (curve_pair.hpp), and the record stays empty."""
    G2 = cv.CURVES[curve][1]
    F2, Fq = G2.F, G2.F.base
    npairs = 384
    els, flat = H.fp2_raw_operands(curve, Fq.p, H.rng(40377), npairs)
    B, NL = H.LAZY_LIMBS[curve]
    Rinv = pow(1 << (B * NL), -1, Fq.p)
    val = lambda l: sum(int(x) << (B * i) for i, x in enumerate(l))
    rep = lambda e: (val(e[0]) * Rinv % Fq.p, val(e[1]) * Rinv % Fq.p)
    for op in range(4):
        out = np.zeros(npairs * 2 * Fq.nlimbs, dtype=np.uint64)
        rec = (C.c_uint64 * 3)()
        assert gpu.lib().csh_selftest_fp2pair_raw_dev(H.CURVE_IDS[curve], op, _ptr(flat), C.c_size_t(npairs), _ptr(out), rec) == 0
        got = H.unpack(Fq, out)
        for j, e in enumerate(els):
            a, b, c, d = (rep(x) for x in e)
            want = [F2.mul(a, b), F2.sqr(a), F2.sub(F2.sqr(a), b), F2.sub(F2.mul(a, b), F2.mul(c, d))][op]
            assert (got[2 * j], got[2 * j + 1]) == want, (op, j)
        _assert_no_bound_violation(rec, "Fp2Pair op %d on %s" % (op, curve))


# ---- 2: the zero tests of Fp2Pair -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", G2_CURVES)
def test_fp2pair_zero_tests_on_every_spelling_of_a_multiple_of_p(gpu, curve):
    """maybe_zero() and is_zero_slow() of Fp2Pair, separately, each component zero / non-zero independently (tests/helpers.py
    zero_test_cases: k p for k in -7 .. 7 in many spellings, k p + d, random non-multiples)."""
    Fq = cv.CURVES[curve][1].F.base
    B, NL = H.LAZY_LIMBS[curve]
    cases = H.zero_test_cases(Fq.p, B, NL, H.rng(2377), spellings=6)
    r = H.rng(99)
    pairs = [(c0, c1) for c0 in cases for c1 in r.sample(cases, 3)]
    flat = np.array([x for c0, c1 in pairs for comp in (c0, c1) for x in comp[0]], dtype=np.int32)
    flags = np.zeros(len(pairs), dtype=np.uint8)
    rec = (C.c_uint64 * 3)()
    assert gpu.lib().csh_selftest_fp2pair_zero_dev(H.CURVE_IDS[curve], _ptr(flat), C.c_size_t(len(pairs)), _ptr(flags), rec) == 0
    for j, (c0, c1) in enumerate(pairs):
        H.check_zero_flags(int(flags[j]), [c0, c1], (curve, j))
    _assert_no_bound_violation(rec, "Fp2Pair zero tests on %s" % curve)


# ---- 1(c): scripted point operations ----------------------------------------------------------------------------------------------
class _Script:
    """Slots (lazy_madd chains the host builds), units (one script per quad / pair) and the oracle's value of both registers."""

    def __init__(self, G, pts):
        self.G, self.pts = G, pts
        self.chain_pts, self.chain_neg, self.slot_off, self.slot_val = [], [], [0], []
        self.extra = []                                                  # affine operands of MADD: behind the chain material, in no slot
        self.units, self.want, self.names = [], [], []

    def slot(self, chain):
        """chain: [(point index, negate)] -> slot id"""
        val = None
        for i, ng in chain:
            self.chain_pts.append(self.pts[i])
            self.chain_neg.append(ng)
            val = self.G.add(val, self.G.neg(self.pts[i]) if ng else self.pts[i])
        self.slot_off.append(len(self.chain_pts))
        self.slot_val.append(val)
        return len(self.slot_val) - 1

    def affine(self, P):
        self.extra.append(P)
        return len(self.extra) - 1

    def unit(self, name, ops):
        G = self.G
        reg = [None, None]
        for code, d, arg, k in ops:
            if code == LOAD:
                reg[d] = self.slot_val[arg]
            elif code == ADDP:
                reg[d] = G.add(reg[d], self.slot_val[arg])
            elif code == ADDR:
                reg[d] = G.add(reg[d], reg[1 - d])
            elif code == ADDS:
                reg[d] = G.add(reg[d], reg[d])
            elif code == DBL:
                reg[d] = G.double(reg[d])
            elif code == MULK:
                reg[d] = G.mul(reg[d], k)
            elif code == MADD:
                reg[d] = G.add(reg[d], G.neg(self.extra[arg]) if k else self.extra[arg])
            elif code == ADDK:
                reg[d] = G.add(reg[d], G.mul(reg[1 - d], k))
            else:
                raise ValueError(code)
        self.units.append(ops)
        self.want.append(tuple(reg))
        self.names.append(name)

    def run(self, hip, curve, group, form):
        G = self.G
        base = len(self.chain_pts)
        allpts = self.chain_pts + self.extra
        ap = cv.pack_points(G, allpts).reshape(-1)
        ng = np.array(self.chain_neg + [0] * len(self.extra), dtype=np.uint8)
        so = np.array(self.slot_off, dtype=np.uint32)
        flat = [x for ops in self.units for code, d, arg, k in ops for x in (code, d, arg + base if code == MADD else arg, k)]
        ops = np.array(flat, dtype=np.uint32)
        uo = np.cumsum([0] + [len(ops_) for ops_ in self.units]).astype(np.uint32)
        nunits = len(self.units)
        out = np.zeros(2 * nunits * _xyzz_words(hip, curve, group), dtype=np.uint64)
        rec = (C.c_uint64 * 3)()
        rc = hip.lib().csh_selftest_point_ops_dev(H.CURVE_IDS[curve], group, form, _ptr(ap), _ptr(ng), C.c_size_t(len(allpts)), _ptr(so),
                                                  C.c_size_t(len(self.slot_val)), _ptr(ops), _ptr(uo), C.c_size_t(nunits), _ptr(out), rec)
        assert rc == 0, (rc, _err(hip))
        got = _xyzz_to_affine(G, out, 2 * nunits)
        bad = [(u, self.names[u], r) for u in range(nunits) for r in (0, 1) if not G.eq(got[2 * u + r], self.want[u][r])]
        assert not bad, "wrong group element in %d of %d units; first: unit %d (%s), register %d" % (len(bad), nunits, bad[0][0], bad[0][1], bad[0][2])
        _assert_no_bound_violation(rec, "point operations on %s group %d form %d" % (curve, group, form))
        return nunits


def _branch_units(s, r, form, rounds):
    """One unit per branch of the addition / doubling / small multiple, `rounds` times over with fresh operands, laid out so that adjacent
    units (quads / pairs of one wave) take different branches in the same launch."""
    G, pts = s.G, s.pts
    n = len(pts)
    empty = s.slot([])
    for rd in range(rounds):
        i, j, k3 = r.sample(range(n), 3)
        A = s.slot([(i, 0), (j, 1)])                                     # P - Q: non-trivial zz / zzz
        Bs = s.slot([(j, 0), (k3, 0), (i, 1)])
        single = s.slot([(i, r.randrange(2))])                           # zz = zzz = 1
        S1 = s.slot([(i, 0), (j, 0), (k3, 0)])                           # P + Q + R ...
        S2 = s.slot([(k3, 0), (j, 0), (i, 0)])                           # ... in the other order: the same group element, another zz
        N1 = s.slot([(i, 1), (j, 1), (k3, 1)])                           # -(P + Q + R), the spelling of S1 mirrored
        N2 = s.slot([(k3, 1), (i, 1), (j, 1)])                           # and with another zz
        stale = s.slot([(i, 0), (i, 1)])                                 # cancelled on the host: empty, with stale limbs
        tag = "round %d: " % rd
        s.unit(tag + "ordinary add", [(LOAD, 0, A, 0), (ADDP, 0, Bs, 0)])
        s.unit(tag + "acc empty", [(ADDP, 0, Bs, 0)])
        s.unit(tag + "p == acc, same stored words", [(LOAD, 0, A, 0), (ADDP, 0, A, 0)])
        s.unit(tag + "p empty", [(LOAD, 0, A, 0), (ADDP, 0, empty, 0)])
        s.unit(tag + "p == -acc, mirrored spelling", [(LOAD, 0, S1, 0), (ADDP, 0, N1, 0)])
        s.unit(tag + "both empty", [(ADDP, 0, empty, 0)])
        s.unit(tag + "p == acc, another zz", [(LOAD, 0, S1, 0), (ADDP, 0, S2, 0)])
        s.unit(tag + "p empty with stale limbs", [(LOAD, 0, Bs, 0), (ADDP, 0, stale, 0)])
        s.unit(tag + "p == -acc, another zz", [(LOAD, 0, S1, 0), (ADDP, 0, N2, 0)])
        s.unit(tag + "acc += acc (one register)", [(LOAD, 0, Bs, 0), (ADDS, 0, 0, 0)])
        s.unit(tag + "double", [(LOAD, 0, A, 0), (DBL, 0, 0, 0)])
        s.unit(tag + "double of empty", [(LOAD, 0, stale, 0), (DBL, 0, 0, 0)])
        s.unit(tag + "zz = 1 operands", [(LOAD, 0, single, 0), (ADDP, 0, A, 0), (LOAD, 1, A, 0), (ADDP, 1, single, 0)])
        s.unit(tag + "register add, then doubled", [(LOAD, 0, A, 0), (LOAD, 1, Bs, 0), (ADDR, 0, 0, 0), (ADDR, 1, 0, 0), (DBL, 1, 0, 0)])
        s.unit(tag + "empty after cancellation, then add", [(LOAD, 0, S2, 0), (ADDP, 0, N1, 0), (ADDP, 0, A, 0)])
        kk = SMALL_K[rd % len(SMALL_K)]
        s.unit(tag + "k acc, k = %d" % kk, [(LOAD, 0, A, 0), (MULK, 0, 0, kk)])
        s.unit(tag + "k empty", [(MULK, 0, 0, SMALL_K[(rd + 4) % len(SMALL_K)])])
        kk = SMALL_K[(rd + 5) % len(SMALL_K)]
        s.unit(tag + "k acc on zz = 1, k = %d" % kk, [(LOAD, 1, single, 0), (MULK, 1, 0, kk), (ADDP, 1, S1, 0)])
        if form == FORM_PAIR:
            P, Q = pts[i], pts[j]
            aP, aQ, aPQ = s.affine(P), s.affine(Q), s.affine(G.add(P, Q))
            s.unit(tag + "madd onto a sum", [(LOAD, 0, A, 0), (MADD, 0, aQ, 0)])
            s.unit(tag + "madd onto empty, twice: doubling of zz = 1", [(MADD, 0, aP, 1), (MADD, 0, aP, 1)])
            s.unit(tag + "madd P then -P", [(MADD, 0, aP, 0), (MADD, 0, aP, 1), (MADD, 1, aQ, 1)])
            s.unit(tag + "madd of the accumulated sum: doubling with zz != 1", [(MADD, 0, aP, 0), (MADD, 0, aQ, 0), (MADD, 0, aPQ, 0)])
            s.unit(tag + "madd of minus the accumulated sum", [(MADD, 0, aQ, 0), (MADD, 0, aP, 0), (MADD, 0, aPQ, 1), (MADD, 0, aQ, 0)])


def _chain_units(s, r, form, length):
    """The window reduction's walk, a few hundred operations long: running (r1) += bucket, acc (r0) += running once per empty bucket in
    between, or acc += gap * running over a longer gap -- the value drift of acc / running reaches whatever it reaches."""
    n = len(s.pts)
    pool = [s.slot([(r.randrange(n), r.randrange(2)) for _ in range(r.randrange(1, 4))]) for _ in range(24)]
    madd = [s.affine(P) for P in s.pts[:6]] if form == FORM_PAIR else []
    for variant in range(4):
        ops = []
        for step in range(length):
            b = pool[r.randrange(len(pool))]
            if variant == 1 and step % 7 == 3:
                ops.append((ADDP, 1, b, 0))                              # the same bucket sum twice in a row
            ops.append((ADDP, 1, b, 0))                                  # running += bucket
            gap = 1 if variant == 0 else r.choice((1, 1, 2, 4, 5, 9, 300, 40000, (1 << 21) - 1))
            if gap <= 4:
                ops += [(ADDR, 0, 0, 0)] * gap
            else:
                ops.append((ADDK, 0, 0, gap))
            if variant == 2 and step % 11 == 5:
                ops += [(DBL, 1, 0, 0), (ADDS, 0, 0, 0)]
            if madd and step % 5 == 1:
                ops.append((MADD, 1, madd[r.randrange(len(madd))], r.randrange(2)))
        s.unit("reduction-like chain %d (%d operations)" % (variant, len(ops)), ops)


@pytest.mark.parametrize("curve,group,form", POINT_FORMS)
def test_point_operations_every_branch_in_one_launch(gpu, curve, group, form):
    """qadd / qdbl / qmul_small over a quad (form 1) and lazy_add_inl / lazy_dbl_inl / lazy_mul_small / lazy_madd over Fp2Pair (form 2) on
    stored points with the representation the accumulate kernel leaves, every branch, adjacent units on different branches."""
    G = cv.CURVES[curve][group]
    r = H.rng(7100 + 10 * group + form)
    pts = H.rand_points(G, 12, r)
    s = _Script(G, pts)
    _branch_units(s, r, form, rounds=9)                                  # 9 rounds: every k of SMALL_K in each of the three multiple cases
    nunits = s.run(gpu, curve, group, form)
    assert nunits >= (128 if form == FORM_PAIR else 64)                  # at least one full 256-thread block


@pytest.mark.parametrize("curve,group,form", POINT_FORMS)
def test_point_operation_chains_like_the_window_reduction(gpu, curve, group, form):
    G = cv.CURVES[curve][group]
    r = H.rng(7300 + 10 * group + form)
    pts = H.rand_points(G, 10, r)
    s = _Script(G, pts)
    _chain_units(s, r, form, length=110)
    _branch_units(s, r, form, rounds=1)                                  # short units next to the long ones: the wave stays divergent
    s.run(gpu, curve, group, form)


# ---- 1(d): the tail stages on chosen buckets --------------------------------------------------------------------------------------
def _tail_layouts(r):
    """(name, NB, S, {bucket: [(point index, negate)]}) over 1100 known points."""
    ch = lambda *idx: [(i, 0) for i in idx]
    L = []
    L.append(("all empty", 8, 1, {}))
    L.append(("all empty, folded", 8, 4, {}))
    L.append(("only bucket 1", 8, 2, {1: ch(0, 1)}))
    L.append(("only bucket NB", 8, 1, {8: ch(2)}))
    L.append(("only bucket NB, four segments", 8, 4, {8: ch(2, 3)}))
    L.append(("gaps of exactly 1, 4 and 5", 64, 1, {60: ch(0, 1), 59: ch(2), 55: ch(3, 4), 50: ch(5), 49: ch(6, 7), 44: ch(8), 40: ch(9)}))
    L.append(("gap above 2^15", 1 << 16, 1, {1 << 16: ch(0, 1), 30000: ch(2), 29999: ch(3, 4), 3: ch(5)}))
    L.append(("gap above 2^15 inside one of four segments", 1 << 16, 2, {65000: ch(0), 32769: ch(1, 2), 32767: ch(3), 2: ch(4, 5), 1: ch(6)}))
    L.append(("running == -acc: B_top = P, B_(top-1) = -2P", 16, 1, {16: ch(0), 15: [(0, 1), (0, 1)], 14: ch(1), 9: ch(2, 3)}))
    L.append(("acc == running, the same words: top bucket, then a gap of 2", 32, 1, {32: ch(0, 1), 30: ch(2), 27: ch(3)}))
    L.append(("fully dense", 128, 1, {b: ch(b, b + 128) for b in range(1, 129)}))
    L.append(("fully dense, 16 segments", 1 << 10, 16, {b: ch(b) for b in range(1, (1 << 10) + 1)}))
    occ = {b: ch(b, (3 * b) % 1000) for b in range(1, 101) if r.randrange(4)}
    L.append(("NB not a multiple of S", 100, 8, occ))
    L.append(("S > NB", 8, 64, {b: ch(b) for b in (1, 2, 5, 8)}))
    L.append(("fold count 200: not a multiple of 128, two levels", 1 << 10, 200, {b: ch(b) for b in range(1, (1 << 10) + 1) if b % 3}))
    L.append(("fold count 129", 600, 129, {b: ch(b) for b in range(1, 601) if r.randrange(2)}))
    L.append(("fold count 128: one full block", 512, 128, {b: ch(b, b + 512) for b in range(1, 513) if b % 5}))
    L.append(("equal neighbours: every bucket the same point", 24, 2, {b: ch(7) for b in range(1, 25)}))
    return L


_TAIL_POINTS = {}


def _tail_points(curve, group):
    key = (curve, group)
    if key not in _TAIL_POINTS:
        _TAIL_POINTS[key] = _known_points(cv.CURVES[curve][group], 1100, H.rng(8100 + group))
    return _TAIL_POINTS[key]


@pytest.mark.parametrize("curve,group,form", TAIL_FORMS)
def test_window_reduction_and_fold_tree_on_chosen_buckets(gpu, curve, group, form):
    """The real k_msm_reduce<Cfg, false> (form 1), k_msm_reduce_serial (0), k_msm_reduce_pair<Cfg, false> (2) and k_msm_fold_tree on one
    window's dense bucket array built on the host: window sum == sum_b b * B_b."""
    G = cv.CURVES[curve][group]
    pts, sc = _tail_points(curve, group)
    packed = cv.pack_points(G, pts)
    words = _xyzz_words(gpu, curve, group)
    for name, NB, S, buckets in _tail_layouts(H.rng(8200)):
        ids = sorted(buckets)
        idx = [i for b in ids for i, _ in buckets[b]]
        ng = np.array([n for b in ids for _, n in buckets[b]] or [0], dtype=np.uint8)
        off = np.cumsum([0] + [len(buckets[b]) for b in ids]).astype(np.uint32)
        ap = np.ascontiguousarray(packed[idx]).reshape(-1) if idx else np.zeros(1, dtype=np.uint64)
        idv = np.array(ids or [0], dtype=np.uint32)
        out = np.zeros(words, dtype=np.uint64)
        rc = gpu.lib().csh_selftest_msm_tail_dev(H.CURVE_IDS[curve], group, form, _ptr(ap), _ptr(ng), C.c_size_t(len(idx)), _ptr(idv), _ptr(off),
                                                 C.c_size_t(len(ids)), C.c_uint32(NB), C.c_uint32(S), _ptr(out))
        assert rc == 0, (name, rc, _err(gpu))
        total = sum(b * sum(-sc[i] if n else sc[i] for i, n in buckets[b]) for b in ids) % G.order
        want = G.mul(G.gen, total) if total else None
        got = _xyzz_to_affine(G, out, 1)[0]
        assert G.eq(got, want), "window sum wrong: layout '%s' (NB = %d, S = %d), form %d" % (name, NB, S, form)


# ---- 3: the device-versus-host chain check of the lane-serial bucket arithmetic ------------------------------------------------------
@pytest.mark.parametrize("curve,group", GROUPS)
def test_lazy_madd_chains_device_equals_host_bit_for_bit(gpu, curve, group):
    """csh_selftest_lazy_chain_dev: ragged lazy_madd chains per thread on the device, a sample recomputed by the same template code on the
    host, exported XYZZ words compared bit for bit. The points include infinities and a duplicate (adjacent in the cyclic chain: doubling,
    or cancellation when the signs differ)."""
    G = cv.CURVES[curve][group]
    pts = H.rand_points(G, 64, H.rng(1), with_inf=True)
    pts[9] = pts[8]
    pts[41] = G.neg(pts[40])
    ap = cv.pack_points(G, pts).reshape(-1)
    bad = C.c_int(-1)
    rc = gpu.lib().csh_selftest_lazy_chain_dev(H.CURVE_IDS[curve], group, _ptr(ap), C.c_size_t(64), C.c_size_t(200), C.c_size_t(16384), C.c_size_t(1024), C.byref(bad))
    assert rc == 0
    assert bad.value == 0, "%d of 1024 sampled threads differ between device and host" % bad.value
