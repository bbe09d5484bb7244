"""Device unit tests of the MSM bucket stage up to the per-bucket sums: k_msm_accum / k_msm_accum_pair, then k_msm_merge or
k_msm_mark_giant, k_msm_giant_slices and k_msm_merge_giant, and qbucket_merged / pbucket_merged for the fused form, run ALONE through
csh_selftest_msm_buckets_dev (csrc/selftest_dev.hip): the launches are bucket_group's own (msm_impl.hpp bucket_sums_launch), on bucket
lists this file builds by hand, so a lane boundary, an equal or opposite pair of partial sums or a point at infinity falls where a case
puts it and not where a planner happens to.

Truth: the points have known discrete logarithms, so bucket b of window w is (sum of +/- s_i mod the order) * G, or empty when that sum
is 0 -- one scalar multiple per bucket, compared by group equality on the affine value after the strict canonical check and
ZZ^3 == ZZZ^2 (tests/helpers.py xyzz_to_affine). A failure names the window, the bucket and its partial slots. Every case also asserts
the two words of giant_count (queued buckets, sliced buckets) against the value derived from its own bucket lists, so a case named
after the sliced path cannot pass on the walk. The export to canonical words (k_st_export of selftest_dev.hip) carries the device form
of the limb-bound contract: the record must come back empty. The two kernels that call qbucket_merged / pbucket_merged are compiled as
the product's units are (csrc/selftest_buckets_dev.hip), so the fused forms run the code k_msm_reduce<Cfg, true> runs."""
import ctypes as C

import numpy as np
import pytest

from oracle import curves as cv
from tests import helpers as H
from tests import msm_sort_ref as R

pytestmark = pytest.mark.gpu

# the constants of csrc/msm_impl.hpp the cases are built around
MERGE_Q = 64            # msm_impl.hpp:265  buckets per block of k_msm_merge
MERGE_CAP = 16          # msm_impl.hpp:273  more partials than this: queued for k_msm_merge_giant
GIANT_BIG = 256         # msm_impl.hpp:279  at least this many partials: sliced (k_msm_giant_slices)
GIANT_SLICES = 16       # msm_impl.hpp:279
CSH_ERR_INVALID = -1

GROUPS = [("bn254", 0), ("bn254", 1), ("bls12_381", 0), ("bls12_381", 1), ("grumpkin", 0), ("bls12_377", 0), ("bls12_377", 1)]
ACC_WHOLE, ACC_PAIR = 0, 1                                  # accumulate form: whole points per lane / a lane pair (G2)
MERGE_LAUNCH, FUSED_QUAD, FUSED_PAIR = 0, 1, 2              # merge form: k_msm_merge / qbucket_merged / pbucket_merged (G2)
ACC_FORMS = [(c, g, ACC_WHOLE) for c, g in GROUPS] + [(c, g, ACC_PAIR) for c, g in GROUPS if g]


def merge_forms(group):
    return (MERGE_LAUNCH, FUSED_QUAD, FUSED_PAIR) if group else (MERGE_LAUNCH, FUSED_QUAD)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _err(hip):
    return hip.lib().csh_last_error().decode(errors="replace")


# ---- the points: 40 with known logarithms, infinity, negated bases, two sums ----------------------------------------------------------
NREG = 40
INF = NREG                                                  # the point at infinity, stored as (0, 0)
NEGB = NREG + 1                                             # NEGB + j = -P_j as a base of its own, j < 8
SUM01, SUM23 = NREG + 9, NREG + 10                          # P_0 + P_1 and P_2 + P_3 as bases
_POOL = {}


class _Pool:
    def __init__(self, curve, group):
        G = self.G = cv.CURVES[curve][group]
        pts, sc = H.known_points(G, NREG, H.rng(9100 + group))
        pts, sc = pts + [None], sc + [0]
        pts, sc = pts + [G.neg(pts[j]) for j in range(8)], sc + [-sc[j] for j in range(8)]
        pts, sc = pts + [G.add(pts[0], pts[1]), G.add(pts[2], pts[3])], sc + [sc[0] + sc[1], sc[2] + sc[3]]
        self.pts, self.sc, self.packed = pts, sc, cv.pack_points(G, pts)
        self.multiples, self.expected = {}, {}

    def multiple(self, k):
        """k * G (None for 0), each k once"""
        k %= self.G.order
        if k not in self.multiples:
            self.multiples[k] = self.G.mul(self.G.gen, k) if k else None
        return self.multiples[k]

    def bucket_sums(self, key, wins):
        """{(w, b): expected point} of a case's windows; computed once per case and shared by every form and lane length"""
        if key not in self.expected:
            self.expected[key] = {(w, b): self.multiple(sum(-self.sc[i] if ng else self.sc[i] for i, ng in ent))
                                  for w, win in enumerate(wins) for b, ent in win.items()}
        return self.expected[key]


def pool(curve, group):
    if (curve, group) not in _POOL:
        _POOL[(curve, group)] = _Pool(curve, group)
    return _POOL[(curve, group)]


def P(*idx):
    return [(i, 0) for i in idx]


def N(*idx):
    """the same points with the sign bit of the entry set"""
    return [(i, 1) for i in idx]


def neg(entries):
    return [(i, 1 - ng) for i, ng in entries]


# ---- a case: bucket lists per window -> start / sorted, expected sums, expected giant_count -------------------------------------------
class Case:
    """wins: one {bucket: [(point id, sign)]} per window, entries in the order they are filed (that order and L place the lane
    boundaries). n: the stride of `sorted` (default: the largest window total, at least 1). giant: the expected (queued, sliced)."""

    def __init__(self, name, NB, L, wins, giant=(0, 0), Ln=None, wide=None, n=None, pass_nlanes=False):
        self.name, self.NB, self.L, self.wins, self.giant = name, NB, L, wins, giant
        self.W = len(wins)
        self.Ln = Ln or L
        self.wide = self.W if wide is None else wide
        self.pass_nlanes = pass_nlanes
        totals = [sum(len(e) for e in win.values()) for win in wins]
        self.n = n or max(totals + [1])
        self.start = np.zeros((self.W, NB + 2), dtype=np.uint32)
        self.sorted = np.full((self.W, self.n), 0xA5A5A5A5, dtype=np.uint32)      # past a window's total: never read
        for w, win in enumerate(wins):
            assert all(1 <= b <= NB for b in win)
            pos = 0
            for b in range(1, NB + 1):
                self.start[w, b] = pos
                for i, ng in win.get(b, ()):
                    self.sorted[w, pos] = i | (ng << 31)
                    pos += 1
            self.start[w, NB + 1] = pos
        self.nlanes = np.array([-(-totals[w] // self.lane(w)) for w in range(self.W)], dtype=np.uint32)

    def lane(self, w):
        return self.Ln if w >= self.wide else self.L

    def parts(self, w, b):
        """(first lane, last lane) that hold entries of bucket b: its partial slots are b + first .. b + last"""
        lo, hi = int(self.start[w, b]), int(self.start[w, b + 1])
        return (lo // self.lane(w), (hi - 1) // self.lane(w)) if hi > lo else None

    def nparts(self, w, b):
        p = self.parts(w, b)
        return p[1] - p[0] + 1 if p else 0

    def derived_giant(self):
        counts = [self.nparts(w, b) for w in range(self.W) for b in range(1, self.NB + 1)]
        return (sum(c > MERGE_CAP for c in counts), sum(c >= GIANT_BIG for c in counts))


def run(gpu, bases, case, acc_form, merge_form, nlanes=None):
    """-> (return code, XYZZ words of the W * NB buckets, giant_count, bound record)"""
    words = 2 * gpu.point_bytes(bases.curve, bases.group) // 8
    out = np.full(case.W * case.NB * words, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    giant = np.full(2, 0xA5A5A5A5, dtype=np.uint32)
    rec = (C.c_uint64 * 3)()
    if nlanes is None and case.pass_nlanes:
        nlanes = case.nlanes
    rc = gpu.lib().csh_selftest_msm_buckets_dev(bases.h, acc_form, merge_form, case.W, C.c_uint32(case.NB), C.c_uint32(case.n), C.c_uint32(case.L),
                                                C.c_uint32(case.Ln), case.wide, _ptr(case.start), _ptr(case.sorted), _ptr(nlanes), _ptr(out), _ptr(giant), rec)
    return rc, out, giant, rec


def check(gpu, bases, pl, case, acc_form, merge_form, key=None):
    """One run of a case under one pair of forms: giant_count, every bucket of every window, the bound record."""
    G = pl.G
    assert case.derived_giant() == case.giant, "case '%s' is not on the path it is named after: %s" % (case.name, case.derived_giant())
    what = "case '%s' (L = %d, Ln = %d), accumulate form %d, merge form %d" % (case.name, case.L, case.Ln, acc_form, merge_form)
    rc, out, giant, rec = run(gpu, bases, case, acc_form, merge_form)
    assert rc == 0, (what, rc, _err(gpu))
    assert tuple(int(x) for x in giant) == case.giant, "%s: giant_count = %s, expected %s" % (what, list(giant), case.giant)
    want = pl.bucket_sums(key or case.name, case.wins)
    got = H.xyzz_to_affine(G, out, case.W * case.NB)
    bad = []
    for w in range(case.W):
        for b in range(1, case.NB + 1):
            if not G.eq(got[w * case.NB + b - 1], want.get((w, b))):
                p = case.parts(w, b)
                bad.append("bucket %d of window %d (%d entries, %s)" % (b, w, len(case.wins[w].get(b, ())),
                                                                        "partial slots of lanes %d .. %d" % p if p else "no entries"))
    assert not bad, "%s: %d wrong bucket sums; first: %s" % (what, len(bad), bad[0])
    n, limb, line = (int(x) for x in rec)
    assert n == 0, "%s: %d operand limbs outside their bound, largest |limb| = %d at field29.hpp:%d" % (what, n, limb, line)


def upload(gpu, curve, group):
    pl = pool(curve, group)
    return pl, gpu.Bases(H.CURVE_IDS[curve], group, pl.packed)


# ---- accumulate cases -----------------------------------------------------------------------------------------------------------------
ACC_L = (1, 2, 3, 5, 8)                                     # every bucket list under every lane length: runs of 1, 2, 3, short last lanes


def accumulate_wins():
    """(name, NB, wins): bucket lists whose sums do not depend on the lane length; ACC_L moves the lane boundaries through them."""
    A = []
    # opening entry: a bucket opened by infinity and followed by real points, infinity only, in the middle, last; infinity with the sign set
    A.append(("infinity entries", 8, [{1: P(INF, 0, 1), 2: P(INF, INF), 3: P(2, INF, 3), 4: P(4, 5, INF), 5: P(INF), 7: P(6) + N(INF), 8: N(INF) + P(7, 8)}]))
    # P then P: the doubling of lazy_madd with a fresh accumulator (bucket 1) and a non-trivial one (bucket 2: P0 + P1, then that sum as
    # a base); P then -P in both spellings, followed by further points (3 .. 6) and ending the bucket (7)
    A.append(("doublings and cancellations", 8, [{1: P(0, 0), 2: P(0, 1, SUM01, 4), 3: P(0, 1) + N(SUM01) + P(4, 5), 4: P(2, 3, NEGB + 2, NEGB + 3, 6),
                                                   5: P(5) + N(5) + P(6, 7), 6: P(5, NEGB + 5, 6), 7: P(6) + N(6), 8: P(9, 9, 9) + N(9, 9) + P(10)}]))
    # 24 entries (a multiple of 1, 2, 3 and 8) and 27 (last lanes of 1, 2 and 3 entries)
    A.append(("total of 24", 6, [{1: P(0, 1, 2, 3, 4), 2: P(5, 6, 7), 3: P(8, 9, 10, 11, 12, 13, 14), 5: P(15, 16, 17, 18), 6: P(19, 20, 21, 22, 23)}]))
    A.append(("total of 27", 6, [{1: P(0, 1, 2, 3, 4), 2: P(5, 6, 7), 3: P(8, 9, 10, 11, 12, 13, 14), 5: P(15, 16, 17, 18), 6: P(19, 20, 21, 22, 23, 24, 25, 26)}]))
    # runs of empty buckets before, between and after occupied ones, bucket 1 and bucket NB; a lane crossing many one-entry buckets
    A.append(("sparse, first and last bucket", 64, [{1: P(0), 2: P(1, 2), 30: P(3), 31: N(4) + P(5), 64: P(6, 7, 8)}]))
    A.append(("sparse, empty ends", 64, [dict([(5, P(0, 1))] + [(10 + j, P(2 + j)) for j in range(17)] + [(40, P(20, 21, 22))])]))
    # three windows with different totals, one of them without entries
    A.append(("three windows", 16, [{1: P(0, 1, 2), 3: P(3, 3) + N(4), 9: P(5, 6, 7, 8, 9, 10, 11)}, {},
                                    {2: P(12, 13), 3: P(14), 4: N(15, 16, 17, 18, 19), 16: P(20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33)}]))
    return A


def accumulate_cases():
    out = []
    for name, NB, wins in accumulate_wins():
        for L in ACC_L:
            out.append((name, Case("%s, L = %d" % (name, L), NB, L, wins, pass_nlanes=L == 3)))
        if len(wins) == 3:                                  # windows from `wide` on take Ln = 2 L: 13 entries at L, none, 22 at 2 L
            out.append((name, Case("%s, wide = 1, Ln = 2 L" % name, NB, 2, wins, Ln=4, wide=1, pass_nlanes=True)))
            out.append((name, Case("%s, wide = 0, Ln = 2 L" % name, NB, 3, wins, Ln=6, wide=0)))
    # the cancelling / doubling pair as the LAST two entries of a lane and as its FIRST two (one bucket of four lanes of 4)
    ends = {1: P(0, 1, 2) + N(2) + P(3) + N(3) + P(4, 5) + P(6, 6, 7, 8) + P(9, 10, 11, 11), 2: P(12, NEGB + 1, 1, 13) + P(NEGB + 4, 4, 14, 15)}
    out.append(("pair at lane ends", Case("pair at lane ends", 4, 4, [ends])))
    # lane boundaries at 4, 8, 12, 16 against bucket boundaries at 4 (coincides), 7 (lane boundary one entry after), 9, 13 (one entry before), 16
    co = Case("boundary coincidence", 8, 4, [{1: P(0, 1, 2, 3), 2: P(4, 5, 6), 3: P(7, 8), 4: P(9, 10, 11, 12), 5: P(13, 14, 15), 8: P(16, 17)}])
    assert [int(x) for x in co.start[0, 1:7]] == [0, 4, 7, 9, 13, 16]
    out.append((co.name, co))
    # a grid wider than nlanes: 7 lanes in a launch sized for n = 1000 entries (8 blocks of 128 lanes; 16 with the lane pair)
    out.append(("oversized grid", Case("oversized grid", 8, 1, [{2: P(0, 1, 2), 5: P(3) + N(3), 8: P(4, 5)}], n=1000)))
    return out


@pytest.mark.parametrize("curve,group,acc_form", ACC_FORMS)
def test_accumulate_on_chosen_bucket_lists(gpu, curve, group, acc_form):
    """k_msm_accum (form 0) / k_msm_accum_pair (form 1) on hand-built bucket lists, every list at L = 1, 2, 3, 5 and 8 and under every
    merge form: infinity opening / inside / ending a bucket, P then P on a fresh and on a non-trivial accumulator, P then -P in both
    spellings, run lengths 1 .. 3, short last lanes, lane boundaries on / before / after a bucket boundary, runs of empty buckets,
    windows with different totals and lane lengths, an empty window, a grid wider than nlanes. No bucket has more than MERGE_CAP partials."""
    pl, bases = upload(gpu, curve, group)
    try:
        for key, case in accumulate_cases():
            assert max(case.nparts(w, b) for w in range(case.W) for b in range(1, case.NB + 1)) <= MERGE_CAP
            for mf in merge_forms(group):
                check(gpu, bases, pl, case, acc_form, mf, key=key)
    finally:
        bases.free()


# ---- merge cases ----------------------------------------------------------------------------------------------------------------------
def lanes_bucket(lanes):
    return [e for lane in lanes for e in lane]


def ordinary_lanes(count, L, shift=0):
    """count full lanes of distinct regular points (no two neighbours equal)"""
    return [P(*[(shift + j * L + k) % NREG for k in range(L)]) for j in range(count)]


def merge_cases():
    """Buckets given lane by lane; every bucket starts on a lane boundary (asserted through the partial counts)."""
    M = []
    L = 2
    # phase boundaries of k_msm_merge: 1 and 2 partials (phase 1 only), 3 (one to phase 2), MERGE_CAP (still the quad path), MERGE_CAP + 1
    counts = {1: 1, 2: 2, 3: 3, 5: 4, 6: MERGE_CAP, 7: MERGE_CAP + 1, 9: 2}
    c = Case("phase boundaries", 10, L, [{b: lanes_bucket(ordinary_lanes(k, L, 3 * b)) for b, k in counts.items()}], giant=(1, 0))
    assert all(c.nparts(0, b) == k for b, k in counts.items())
    M.append(c)
    # exceptional partials in phase 1 (slots 0, 1) and phase 2 (slots 2 ..): equal (another zz: P0 + P1 against P1 + P0; the same words),
    # opposite followed by more, a partial whose own sum cancelled
    a, b2, e = P(0, 1), P(2, 3), P(4) + N(4)
    ex = {1: [a, P(1, 0)], 2: [a, a], 3: [a, neg(a), P(5, 6)], 4: [e, P(5, 6)], 5: [P(5, 6), e], 6: [e, e, P(7, 8)],
          7: [a, b2, P(SUM01, SUM23), P(9, 10)],          # phase 2 adds (P0 + P1) + (P2 + P3) to itself
          8: [a, b2, N(SUM01, SUM23), P(9, 10)],          # ... and its opposite, then more onto the empty sum
          9: [a, b2, e, P(11, 12)], 10: [a, neg(a), e], 11: [a, b2, P(NEGB + 0, NEGB + 1), P(NEGB + 2, NEGB + 3)]}
    c = Case("exceptional partials in both phases", 12, L, [{b: lanes_bucket(v) for b, v in ex.items()}])
    assert all(c.nparts(0, b) == len(v) for b, v in ex.items())
    M.append(c)
    # the LDS tree of k_msm_merge_giant, 40 partials = 40 quads with one partial each: level one adds quad q + 32 to quad q, the last
    # level adds the sum of the odd partials to the sum of the even ones
    def tree(first, last):
        ln = ordinary_lanes(40, L, 1)
        if first:
            ln[32 + 3] = ln[3]                               # equal at the first level
            ln[32 + 5] = neg(ln[5])                          # opposite at the first level
            ln[7] = P(6) + N(6)                              # an empty partial
        if last:
            for j in range(0, 40, 2):
                ln[j + 1] = ln[j] if last > 0 else neg(ln[j])
        return lanes_bucket(ln)
    c = Case("giant tree", 8, L, [{1: P(0, 9), 2: tree(True, 0), 4: tree(False, 1), 5: tree(False, -1), 6: tree(True, 0)[:2 * (MERGE_CAP + 1)], 8: P(1, 2, 3)}], giant=(4, 0))
    assert [c.nparts(0, b) for b in (2, 4, 5, 6)] == [40, 40, 40, MERGE_CAP + 1]
    M.append(c)
    # the strided private sums of k_msm_merge_giant, 130 partials: quad q adds partials q, q + 64, q + 128
    ln = ordinary_lanes(130, L, 2)
    ln[64 + 3] = ln[3]
    ln[64 + 1], ln[128 + 1] = neg(ln[1]), P(20, 21)
    ln[64 + 7] = P(8) + N(8)
    ln[9], ln[64 + 9] = P(8, NEGB + 0), P(0) + N(8)      # opposite sums: a negated base on one side, the sign bit on the other
    c = Case("giant strided sums", 4, L, [{2: lanes_bucket(ln), 3: P(5)}], giant=(1, 0))
    assert c.nparts(0, 2) == 130
    M.append(c)
    # block boundaries of k_msm_merge (64 buckets) and k_msm_mark_giant (256)
    L1 = 1
    occ = {64: 3, 65: 2, 128: MERGE_CAP + 1, 256: MERGE_CAP + 1, 257: MERGE_CAP + 2, 300: 3}
    c = Case("block boundaries", 300, L1, [{b: lanes_bucket(ordinary_lanes(k, L1, b)) for b, k in occ.items()}], giant=(3, 0))
    assert all(c.nparts(0, b) == k for b, k in occ.items())
    M.append(c)
    # one block of k_msm_merge whose 64 buckets ALL go to the phase-2 list (buckets 65 .. 128), its neighbours with one partial
    full = {b: lanes_bucket(ordinary_lanes(3, L1, b)) for b in range(MERGE_Q + 1, 2 * MERGE_Q + 1)}
    full[MERGE_Q], full[2 * MERGE_Q + 1] = P(0), P(1)
    M.append(Case("a full phase-2 list", 2 * MERGE_Q + 2, L1, [full]))
    return M


def sliced_cases():
    S = []
    L = 2
    # 256 partials, 16 per slice = 16 quads with one partial each: the first level of the slice's tree that adds two sums is quad q + 8
    # to quad q; k_msm_merge_giant then adds slice sum q + 8 to slice sum q
    ln = ordinary_lanes(GIANT_BIG, L, 3)
    ln[8 + 2] = ln[2]                                        # equal inside slice 0
    ln[16 + 8 + 3] = neg(ln[16 + 3])                         # opposite inside slice 1
    ln[32 + 5] = P(7) + N(7)                                 # an empty partial in slice 2
    ln[8 * 16:9 * 16] = ln[0:16]                             # slice 8 == slice 0: equal slice sums
    ln[9 * 16:10 * 16] = [neg(x) for x in ln[16:32]]         # slice 9 == -slice 1: opposite slice sums
    ln[11 * 16:12 * 16] = [neg(x) for x in ln[3 * 16:4 * 16]]
    ln[3 * 16:4 * 16] = [P(9) + N(9)] * 16                   # slice 3 sums to nothing, slice 11 stays
    c = Case("sliced, exceptional partials", 6, L, [{1: P(0, 1), 2: P(3, 4), 3: lanes_bucket(ln), 4: lanes_bucket(ordinary_lanes(MERGE_CAP + 1, L)), 5: P(5)}], giant=(2, 1))
    assert c.nparts(0, 3) == GIANT_BIG and c.nparts(0, 4) == MERGE_CAP + 1
    S.append(c)
    # counts 256, 257 (per = 17: the last slice holds 2 partials) and 271, two sliced buckets in different windows, L = 1
    w0 = {2: lanes_bucket(ordinary_lanes(GIANT_BIG + 1, 1, 5)), 3: P(0, 1)}
    w1 = {1: P(2), 7: lanes_bucket(ordinary_lanes(GIANT_BIG, 1, 7)), 8: lanes_bucket(ordinary_lanes(271, 1, 11))}
    c = Case("sliced in two windows", 8, 1, [w0, w1], giant=(3, 3))
    assert [c.nparts(0, 2), c.nparts(1, 7), c.nparts(1, 8)] == [257, 256, 271]
    S.append(c)
    # 1040 partials, 65 per slice: quad 0 of a slice adds its partials 0 and 64
    ln = ordinary_lanes(1040, 1, 1)
    ln[64] = ln[0]                                           # equal in the strided sum of slice 0
    ln[65 + 64] = neg(ln[65])                                # opposite in slice 1
    c = Case("sliced strided sums", 4, 1, [{1: P(3), 4: lanes_bucket(ln)}], giant=(1, 1))
    assert c.nparts(0, 4) == 1040
    S.append(c)
    return S


def test_no_sliced_bucket_has_an_empty_slice():
    """per = ceil(count / GIANT_SLICES), and the last slice starts at per * (GIANT_SLICES - 1): that is >= count only for
    count <= (GIANT_SLICES - 1)^2 = 225 < GIANT_BIG. A sliced bucket therefore never has an empty slice; the shortest last slice is the
    one partial of count = 16 k + 1 with per * 15 = count - 1, which needs k = 14: not sliced either. 257 leaves it two partials."""
    for count in range(GIANT_BIG, 4 * GIANT_BIG):
        per = -(-count // GIANT_SLICES)
        assert per * (GIANT_SLICES - 1) < count
    assert 257 - 17 * (GIANT_SLICES - 1) == 2


@pytest.mark.parametrize("curve,group,acc_form", ACC_FORMS)
def test_merge_on_chosen_partial_counts(gpu, curve, group, acc_form):
    """k_msm_merge (both phases), k_msm_mark_giant + qbucket_merged / pbucket_merged, and k_msm_merge_giant on buckets of 1, 2, 3, 4,
    MERGE_CAP, MERGE_CAP + 1, 40 and 130 partials, with equal, opposite and cancelled partial sums in phase 1, phase 2, the strided sums
    and the first and last level of the block tree; NB = 300 with buckets at the block boundaries; a block whose 64 buckets all reach
    phase 2. giant_count is asserted in every run."""
    pl, bases = upload(gpu, curve, group)
    try:
        for case in merge_cases():
            for mf in merge_forms(group):
                check(gpu, bases, pl, case, acc_form, mf)
    finally:
        bases.free()


@pytest.mark.parametrize("curve,group,acc_form", ACC_FORMS)
def test_sliced_buckets(gpu, curve, group, acc_form):
    """Buckets of 256, 257, 271 and 1040 partials (k_msm_giant_slices, the sliced branch of k_msm_merge_giant): equal, opposite and
    cancelled sums inside a slice and between two slice sums, a short last slice, sliced buckets in two windows and next to ordinary
    and queued ones in one block."""
    pl, bases = upload(gpu, curve, group)
    try:
        for case in sliced_cases():
            for mf in merge_forms(group):
                check(gpu, bases, pl, case, acc_form, mf)
    finally:
        bases.free()


# ---- chained with the sort stage ------------------------------------------------------------------------------------------------------
def _sort(gpu, curve, ints):
    F = H.FR[curve]
    sc = H.pack(F, ints, mont=False)
    info = np.zeros(R.INFO_WORDS, dtype=np.uint32)
    call = lambda st, nl, so: gpu.lib().csh_selftest_msm_sort_dev(H.CURVE_IDS[curve], _ptr(sc), C.c_size_t(len(ints)), 0, None, _ptr(info), _ptr(st),
                                                                C.c_size_t(0 if st is None else st.size), _ptr(nl), _ptr(so), C.c_size_t(0 if so is None else so.size))
    assert call(None, None, None) == 0, _err(gpu)
    plan = R.plan_from_info(info)
    start = np.zeros(plan.srt_W * (plan.NB + 2), dtype=np.uint32)
    nlanes = np.zeros(plan.srt_W, dtype=np.uint32)
    sorted_ = np.zeros(plan.srt_W * plan.srt_n, dtype=np.uint32)
    assert call(start, nlanes, sorted_) == 0, _err(gpu)
    return plan, start.reshape(plan.srt_W, plan.NB + 2), nlanes, sorted_.reshape(plan.srt_W, plan.srt_n)


@pytest.mark.parametrize("curve,group,acc_form", [("bn254", 0, ACC_WHOLE), ("bls12_381", 1, ACC_PAIR)])
@pytest.mark.parametrize("knobs", [{}, {"msm_l": 3}, {"msm_variant": 64, "msm_l": 4, "msm_c": 0, "msm_w": 37}], ids=["plain", "l3", "variant64-l4"])
def test_chained_behind_the_sort_stage(gpu, curve, group, acc_form, knobs):
    """csh_selftest_msm_sort_dev on 200 scalars (uniform, and the skewed set of test_msm_window_sizes), its start / nlanes / sorted fed
    to the bucket stage with the plan's NB, L, Ln and wide: windows 0 and 1, and the two windows around the wide / narrow boundary (the
    last two of a uniform plan). Plain: 7-bit windows at the planner's lane length; msm_l = 3: the skewed set reaches the giant queue;
    msm_variant bit 6 on 37 balanced windows: the narrow windows take Ln = 2 L. Expected buckets: the bucket lists of
    tests/msm_sort_ref.py over points with known logarithms, scalar i filed with point i mod 40."""
    pl, bases = upload(gpu, curve, group)
    r = H.FR[curve].p
    rnd = H.rng(77)
    uniform = [rnd.randrange(r) for _ in range(200)]
    sets = {"uniform": uniform, "skewed": [1] * 80 + [r - 1] * 50 + [5 << 200] * 40 + uniform[:30]}
    kv = dict(msm_c=7, msm_w=0, msm_balanced=1, msm_l=0, msm_variant=0, sort_two_level=-1)
    kv.update(knobs)
    try:
        for name, ints in sets.items():
            with gpu.tuned(**kv):
                plan, start, nlanes, sorted_ = _sort(gpu, curve, ints)
            assert plan.srt_n == 200 and plan.srt_W == plan.W and plan.NB == 64 and plan.path == R.PATH_SINGLE, plan
            if "msm_variant" in knobs:
                assert plan.Ln == 2 * plan.L and plan.srt_wide < plan.W, plan
            ref = R.sort_reference(R.limbs_of(ints), plan)
            for w0 in (0, plan.srt_wide - 1 if plan.srt_wide < plan.W else plan.W - 2):
                wins = []
                for w in (w0, w0 + 1):
                    tot = int(ref[w].start[-1])
                    assert np.array_equal(start[w], ref[w].start) and int(nlanes[w]) == ref[w].nlanes
                    so = sorted_[w, :tot]                    # the device's own order inside a bucket
                    assert sorted(int(e) for e in so) == sorted(int(e) for e in ref[w].entries)
                    wins.append({b: [((int(e) & 0x7fffffff) % NREG, int(e) >> 31) for e in so[int(start[w, b]):int(start[w, b + 1])]]
                                 for b in range(1, plan.NB + 1) if start[w, b + 1] > start[w, b]})
                case = Case("%s, windows %d and %d" % (name, w0, w0 + 1), plan.NB, plan.L, wins, Ln=plan.Ln, wide=min(max(plan.srt_wide - w0, 0), 2), n=200,
                            pass_nlanes=True)
                case.giant = case.derived_giant()            # what the plan's lane length makes of the set: the device must agree
                assert np.array_equal(case.start, start[w0:w0 + 2]) and np.array_equal(case.nlanes, nlanes[w0:w0 + 2])
                if name == "skewed" and w0 == 0 and "msm_l" in knobs:
                    assert case.giant[0] >= 1, case.giant    # the 80 ones in bucket 1 of window 0
                for mf in merge_forms(group):
                    check(gpu, bases, pl, case, acc_form, mf, key=(name, w0, plan.c, plan.W, plan.wide))
    finally:
        bases.free()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals(gpu):
    """CSH_ERR_INVALID, with the output and giant_count untouched, for a start that is not monotone, start[1] != 0, an id at the
    handle's length, the lane pair on a G1 group and an nlanes that disagrees; the untouched arguments run."""
    pl, bases = upload(gpu, "bn254", 0)
    wins = [{1: P(0, 1, 2), 3: P(3, 4)}]
    try:
        def refused(case, acc_form=ACC_WHOLE, merge_form=MERGE_LAUNCH, nlanes=None):
            rc, out, giant, rec = run(gpu, bases, case, acc_form, merge_form, nlanes=nlanes)
            assert rc == CSH_ERR_INVALID, rc
            assert np.all(out == 0x5A5A5A5A5A5A5A5A) and np.all(giant == 0xA5A5A5A5)
        good = Case("good", 4, 2, wins)
        check(gpu, bases, pl, good, ACC_WHOLE, MERGE_LAUNCH)
        c = Case("not monotone", 4, 2, wins)
        c.start[0, 3] = 2                                    # start[2] = 3
        refused(c)
        c = Case("start[1] != 0", 4, 2, wins)
        c.start[0, 1] = 1
        refused(c)
        c = Case("total above n", 4, 2, wins)
        c.start[0, 5] = 6
        refused(c)
        c = Case("id out of range", 4, 2, wins)
        c.sorted[0, 4] = len(pl.pts) | (1 << 31)             # the sign bit is masked off before the comparison
        refused(c)
        c.sorted[0, 4] = (len(pl.pts) - 1) | (1 << 31)
        assert run(gpu, bases, c, ACC_WHOLE, MERGE_LAUNCH)[0] == 0
        refused(good, acc_form=ACC_PAIR)
        refused(good, merge_form=FUSED_PAIR)
        refused(good, nlanes=np.array([2], dtype=np.uint32))
        assert run(gpu, bases, good, ACC_WHOLE, MERGE_LAUNCH, nlanes=np.array([3], dtype=np.uint32))[0] == 0
    finally:
        bases.free()
