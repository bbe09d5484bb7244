"""Device unit tests of the MSM sort stage: the digit recoding (k_msm_digits, and wide_codes of the wide sort), the bucket offsets
`start`, the lane counts `nlanes` and the bucket lists `sorted` of the plain counting sort (single-level; two-level with 4- and 8-byte
records, tile-parallel and per-partition level 2) and of the wide sort (each record size, each lb), run ALONE through
csh_selftest_msm_sort_dev (csrc/selftest_dev.hip): the product's own plan, scratch sizes and launches on host scalars, nothing of the
bucket stage behind it.

Every comparison is exact and against tests/msm_sort_ref.py (numpy, from the definition; checked on the CPU in
tests/test_msm_sort_ref_cpu.py): `start` and `nlanes` word for word, the entries of every bucket as a multiset (the order inside a bucket is
run-dependent by design: SortBuffers, msm_sort.hpp). Each case asserts the path the harness reports, so a case cannot pass on another
kernel than the one it is named after."""
import ctypes as C

import numpy as np
import pytest

from tests import helpers as H
from tests import msm_sort_ref as R

pytestmark = pytest.mark.gpu

CURVES = ["bn254", "bls12_381", "grumpkin", "bls12_377"]       # scalar fields: BN254 Fr, BLS12-381 Fr, BN254 Fq, BLS12-377 Fr
CSH_ERR_INVALID = -1
# every knob the planner and the sorts read, at its default: a case states only what it changes
KNOBS = dict(msm_c=0, msm_w=0, msm_balanced=1, msm_l=0, msm_variant=0, sort_two_level=-1, msm_wide_lb=0, msm_wide_chunks=0)
L2_TILE = 8192                                                  # records per level-2 tile / job of both sorts (msm_sort.hpp)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _err(hip):
    return hip.lib().csh_last_error().decode(errors="replace")


def _call(gpu, curve, sc, n, mont, table, info, start=None, nlanes=None, sorted_=None):
    tb = np.array(table, dtype=np.uint64) if table is not None else None
    return gpu.lib().csh_selftest_msm_sort_dev(H.CURVE_IDS[curve], _ptr(sc), C.c_size_t(n), int(mont), _ptr(tb), _ptr(info), _ptr(start),
                                               C.c_size_t(0 if start is None else start.size), _ptr(nlanes), _ptr(sorted_),
                                               C.c_size_t(0 if sorted_ is None else sorted_.size))


def run_sort(gpu, curve, ints, mont, table=None):
    """The sort stage on the scalars `ints` (canonical integers), handed over in Montgomery form (mont = 1) or as they are.
    -> (Plan, start [W'][NB + 2], nlanes [W'], sorted [W'][n'])"""
    F = H.FR[curve]
    sc = H.pack(F, ints, mont=bool(mont))
    info = np.zeros(R.INFO_WORDS, dtype=np.uint32)
    assert _call(gpu, curve, sc, len(ints), mont, table, info) == 0, _err(gpu)
    plan = R.plan_from_info(info)
    start = np.full(plan.srt_W * (plan.NB + 2), 0xA5A5A5A5, dtype=np.uint32)
    nlanes = np.full(plan.srt_W, 0xA5A5A5A5, dtype=np.uint32)
    sorted_ = np.full(plan.srt_W * plan.srt_n, 0xA5A5A5A5, dtype=np.uint32)
    info2 = np.zeros_like(info)
    assert _call(gpu, curve, sc, len(ints), mont, table, info2, start, nlanes, sorted_) == 0, _err(gpu)
    assert np.array_equal(info, info2)
    return plan, start.reshape(plan.srt_W, plan.NB + 2), nlanes, sorted_.reshape(plan.srt_W, plan.srt_n)


def check_against_reference(plan, ref, start, nlanes, sorted_, what):
    """The one comparison of a harness result with the reference: start and nlanes exactly, the entries of every bucket as a multiset
    (one lexsort over (bucket of the position, entry) per window); positions past a window's total are not looked at."""
    for ws, r in enumerate(ref):
        if not np.array_equal(start[ws], r.start):
            b = int(np.nonzero(start[ws] != r.start)[0][0])
            pytest.fail("%s: sort window %d: start[%d] = %d, expected %d (%d entries expected in the window)"
                        % (what, ws, b, int(start[ws][b]), int(r.start[b]), int(r.start[-1])))
        assert int(nlanes[ws]) == r.nlanes, "%s: sort window %d: nlanes = %d, expected %d" % (what, ws, int(nlanes[ws]), r.nlanes)
        total = int(r.start[-1])
        got = sorted_[ws, :total]
        bucket_of_pos = np.repeat(np.arange(r.counts.size), r.counts)
        got = got[np.lexsort((got, bucket_of_pos))]
        if not np.array_equal(got, r.entries):
            k = int(np.nonzero(got != r.entries)[0][0])
            b = int(bucket_of_pos[k])
            pytest.fail("%s: sort window %d, bucket %d: holds entry %#010x where %#010x is expected (entry %d of %d in the bucket, values ascending)"
                        % (what, ws, b, int(got[k]), int(r.entries[k]), k - int(r.start[b]), int(r.counts[b])))


def run_case(gpu, curve, n, sets, knobs=None, table=None, expect=None, seed=1, layouts=None, both_forms=False):
    """Every named scalar set at n scalars through the harness under `knobs`, each run checked against the reference (computed once per
    set). Input forms: the first set goes in as Montgomery words (mont = 1) and as plain integers (mont = 0), the others alternate
    between the two -- every case sees both forms, the product set x form is taken only with both_forms (the recoder case F).
    expect: Plan fields that must hold -- the path above all. layouts: the window layouts (c, W, wide) the sets are built for
    (default: the plan's own); with several, a result is keyed "set@c". -> {set name: (Plan, reference)}"""
    kv = dict(KNOBS)
    kv.update(knobs or {})
    r = H.FR[curve].p
    out = {}
    with gpu.tuned(**kv):
        sc0 = H.pack(H.FR[curve], [0] * n, mont=False)
        info = np.zeros(R.INFO_WORDS, dtype=np.uint32)
        assert _call(gpu, curve, sc0, n, 0, table, info) == 0, _err(gpu)
        p0 = R.plan_from_info(info)                             # the scalar sets are built for the windows of the plan that runs
        lays = layouts or [(p0.c, p0.W, p0.wide)]
        ran = set()
        for k, (lay, name) in enumerate((lay, name) for lay in lays for name in dict.fromkeys(sets)):
            ints = R.scalar_set(name, r, n, lay[0], lay[1], lay[2], seed)
            assert len(ints) == n and all(0 <= v < r for v in ints)
            if tuple(ints) in ran:                               # a set that does not depend on the layout, already run
                continue
            ran.add(tuple(ints))
            ref = None
            name = name if len(lays) == 1 else "%s@%d" % (name, lay[0])
            for mont in ((1, 0) if both_forms or k == 0 else (k & 1,)):
                what = "%s n=%d set=%s mont=%d %s table=%s" % (curve, n, name, mont, knobs or {}, table)
                plan, start, nlanes, sorted_ = run_sort(gpu, curve, ints, mont, table)
                assert plan == p0, what
                for key, v in (expect or {}).items():
                    assert getattr(plan, key) == v, "%s: plan.%s = %d, expected %d" % (what, key, getattr(plan, key), v)
                if ref is None:
                    ref = R.sort_reference(R.limbs_of(ints), plan)
                check_against_reference(plan, ref, start, nlanes, sorted_, what)
            out[name] = (plan, ref)
    return out


def _rotating_sets(j, shift=0, per=3):
    """`per` scalar sets for the j-th shape of a case: over five shapes every set comes up, whatever the shift"""
    return ["uniform"] + [R.SET_NAMES[(per * j + k + shift) % len(R.SET_NAMES)] for k in range(per)]


# ---- A: single-level plain sort, uniform windows ------------------------------------------------------------------------------------
A_C = [2, 3, 8, 11, 15, 16]
A_N = [1, 65, 1025, 4097, 12291]


@pytest.mark.parametrize("c", A_C)
def test_single_level_uniform_windows(gpu, c):
    """c = 2: 128 windows (MAX_WINDOWS); c = 16: the top digit code 0x7FFF. n = 12291: several chunks, their length no multiple of the
    4096-entry histogram step, the last one short (wherever the planner cuts chunks at all: c <= 11)."""
    bits = H.FR["bn254"].p.bit_length()
    W = R.windows_for(bits, c)
    seen = set()
    for j, n in enumerate(A_N):
        sets = _rotating_sets(j, A_C.index(c)) + (["runs"] if c >= 11 and n in (1025, 4097) else [])
        res = run_case(gpu, "bn254", n, sets, dict(msm_c=c), expect=dict(c=c, W=W, wide=W, NB=1 << (c - 1), path=R.PATH_SINGLE, rec_bytes=0, srt_W=W, srt_n=n))
        seen.update(res)
        plan = res["uniform"][0]
        if n == 12291 and c <= 11:
            assert plan.CH > 1 and plan.chunk_len % 4096 != 0 and n % plan.chunk_len != 0, plan
        if c == 16 and "halfchunk" in res and n >= 65:          # bucket 2^15 (code 0x7FFF, positive) holds every scalar in the filled windows
            assert int(res["halfchunk"][1][0].counts[1 << 15]) == n
    assert seen == set(R.SET_NAMES)
    assert W == 128 or c != 2
    if c >= 15:
        # one chunk (the planner cuts none at 2^14 buckets and more), so a wave of k_msm_hist_lds / k_msm_scatter_lds is a block of 64
        # consecutive scalars: the "runs" set puts every path of the wave-aggregated counter into such waves (model: R.wave_peels)
        assert plan.CH == 1
        d = R.signed_digits(R.limbs_of(R.scalar_set("runs", H.FR["bn254"].p, 4097, c, W, W, 1)), c, W, W)
        for w in (0, W // 2):
            prof = R.wave_profiles(d[w])
            assert any(p == 2 and stop == 7 for p, stop, left in prof), prof                  # two peels, then a group of 7
            assert any(p == 0 and stop == 7 and left >= 9 for p, stop, left in prof), prof    # a leading group of 7: no peel
            assert any(p == 4 and left >= 8 for p, stop, left in prof), prof                  # the 4-round limit with a run left


@pytest.mark.parametrize("curve", CURVES[1:])
def test_single_level_other_fields(gpu, curve):
    W = R.windows_for(H.FR[curve].p.bit_length(), 11)
    for n in (65, 4097):
        run_case(gpu, curve, n, R.SET_NAMES, dict(msm_c=11), expect=dict(c=11, W=W, wide=W, path=R.PATH_SINGLE))


# ---- B: balanced windows ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1025, 8192, 32775])
def test_balanced_default_plan(gpu, n):
    sets = R.SET_NAMES if n == 1025 else ("uniform", "equal", "runs")
    res = run_case(gpu, "bn254", n, sets, expect=dict(path=R.PATH_SINGLE))
    plan = res["uniform"][0]
    assert plan.wide + plan.W * (plan.c - 1) == 255 and 1 <= plan.wide <= plan.W and plan.srt_wide == plan.wide, plan


@pytest.mark.parametrize("w,c,wide", [(16, 16, 15), (17, 15, 17), (85, 3, 85), (127, 3, 1)])
def test_balanced_forced_window_count(gpu, w, c, wide):
    """msm_w = 127: one 3-bit window and 126 2-bit ones; 16: fifteen 16-bit windows and one of 15 bits."""
    run_case(gpu, "bn254", 1025, R.SET_NAMES, dict(msm_w=w), expect=dict(W=w, c=c, wide=wide, path=R.PATH_SINGLE))
    run_case(gpu, "bls12_381", 4097, ("uniform", "bounds", "halfchunk", "halfchunk1"), dict(msm_w=w), expect=dict(W=w, path=R.PATH_SINGLE))


@pytest.mark.parametrize("n", [1025, 8192])
def test_narrow_windows_take_their_own_lane_length(gpu, n):
    """msm_variant bit 6 with a short lane: Ln = 2 L in the narrow windows, so their nlanes differ from a wide window's with as many entries."""
    res = run_case(gpu, "bn254", n, ("uniform", "equal", "runs", "zero", "one", "halfchunk1"), dict(msm_variant=64, msm_l=4), expect=dict(L=4, Ln=8, path=R.PATH_SINGLE))
    plan, ref = res["uniform"]
    assert plan.srt_wide < plan.W
    wide_w, narrow_w = ref[0], ref[plan.W - 2]
    assert wide_w.nlanes == -(-int(wide_w.start[-1]) // 4) and narrow_w.nlanes == -(-int(narrow_w.start[-1]) // 8) and narrow_w.nlanes < wide_w.nlanes


@pytest.mark.parametrize("n", [1025, 4097])
def test_lane_length_three(gpu, n):
    run_case(gpu, "bn254", n, ("uniform", "equal", "runs", "zero", "small", "rm1"), dict(msm_l=3), expect=dict(L=3, Ln=3, path=R.PATH_SINGLE))


# ---- C: two-level plain sort ----------------------------------------------------------------------------------------------------------
# every c and every variant; all four variants (record size x level-2 form) at c = 16, where a window has the most partitions
TWO_LEVEL_CASES = [(11, 0), (11, 40), (14, 8), (14, 32), (16, 0), (16, 8), (16, 32), (16, 40)]


@pytest.mark.parametrize("c,variant", TWO_LEVEL_CASES)
def test_two_level(gpu, c, variant):
    """variant bit 3: 8-byte records, bit 5: one block per partition in level 2. "small" at n = 24577 puts three level-2 tiles of
    window 0 into partition 0 and leaves every other window empty; "equal" puts a whole window into one bucket."""
    flip = TWO_LEVEL_CASES.index((c, variant)) & 1
    n_a, n_b = (8197, 24577) if flip else (24577, 8197)
    exp = dict(c=c, path=R.PATH_TWO_LEVEL, rec_bytes=8 if variant & 8 else 4, per_partition=1 if variant & 32 else 0)
    knobs = dict(msm_c=c, sort_two_level=1, msm_variant=variant)
    extra = c == 16 and variant in (0, 40)                  # the default path and the one furthest from it take two more sets
    run_case(gpu, "bn254", n_a, ("uniform", "halfchunk1") if extra else ("uniform",), knobs, expect=exp)
    run_case(gpu, "bn254", n_b, ("equal", "runs") if extra else ("equal",), knobs, expect=exp)
    res = run_case(gpu, "bn254", 24577, ("small",), knobs, expect=exp)
    plan, ref = res["small"]
    assert int(ref[0].counts[1:257].sum()) == int(ref[0].start[-1]) > 2 * L2_TILE and all(int(r.start[-1]) == 0 for r in ref[1:])


# ---- D: the 4-byte / 8-byte record switch of the plain two-level sort, through the table remap --------------------------------------------
@pytest.mark.parametrize("rows", [2, 4])
def test_two_level_record_switch_at_2p23(gpu, rows):
    """rows * stride == 2^23: 4-byte records, and the last scalar of the last row is stored as id 2^23 - 1 (all 23 id bits set, the sign
    bit of the record right above them); one point more per row: 8-byte records."""
    n, c = 8203, 13
    knobs = dict(sort_two_level=1)
    for stride, rec in (((1 << 23) // rows, 4), ((1 << 23) // rows + 1, 8)):
        table = (c, rows, stride, stride - n)
        exp = dict(c=c, path=R.PATH_TWO_LEVEL, rec_bytes=rec, dig_g=rows, srt_n=rows * n, remap_stride=stride, remap_off=stride - n)
        res = run_case(gpu, "bn254", n, ("uniform", "halfchunk1", "equal", "rm1"), knobs, table=table, expect=exp)
        top = rows * stride - 1
        plan, ref = res["halfchunk1"]
        entries = np.concatenate([r.entries for r in ref])
        assert (top | 1 << 31) in entries and int((entries & 0x7fffffff).max()) == top      # the largest id is stored, with the sign set
        assert top == (1 << 23) - 1 or rec == 8


def test_harness_refusals(gpu):
    sc = H.pack(H.FR["bn254"], [1] * 16, mont=False)
    info = np.zeros(R.INFO_WORDS, dtype=np.uint32)
    assert _call(gpu, "bn254", sc, 0, 0, None, info) == CSH_ERR_INVALID
    assert _call(gpu, "bn254", sc, 16, 0, (13, 2, 100, 85), info) == CSH_ERR_INVALID          # offset + n > stride
    assert _call(gpu, "bn254", sc, 16, 0, (13, 2, 100, 84), info) == 0, _err(gpu)
    assert _call(gpu, "bn254", sc, 16, 0, (17, 2, 100, 0), info) == CSH_ERR_INVALID           # wide windows need one row per window
    assert _call(gpu, "bn254", sc, 16, 0, (13, 2, 1 << 30, 0), info) == CSH_ERR_INVALID       # ids past 31 bits


# ---- E: the wide sort ---------------------------------------------------------------------------------------------------------------
# every pair (c, lb); every field, n, chunk target at least once; BLS12-381 Fr at c = 17 has 16 digits (WS_MAXW)
WIDE_CASES = [(17, 0, "bn254", 5000, 0), (17, 8, "bls12_381", 513, 1), (17, 11, "grumpkin", 512, 3),
              (20, 0, "bls12_377", 511, 3), (20, 8, "bn254", 1, 0), (20, 11, "bls12_381", 5000, 1),
              (22, 0, "grumpkin", 513, 1), (22, 8, "bls12_377", 5000, 3), (22, 11, "bn254", 512, 0)]


@pytest.mark.parametrize("c,lb,curve,n,chunks", WIDE_CASES)
def test_wide_sort(gpu, c, lb, curve, n, chunks):
    """n = 511 / 512 / 513: a last level-1 tile of 511, 512 and 1 live scalars. n = 5000: "halfchunk" puts every digit of every scalar
    into ONE bucket (several level-2 jobs on one partition), "equal" one bucket per table row."""
    W = R.windows_for(H.FR[curve].p.bit_length(), c)
    stride = 6000
    table = (c, W, stride, stride - n)                      # one row per window; the call is the tail of the table
    exp = dict(c=c, W=W, wide=W, NB=1 << (c - 1), path=R.PATH_WIDE, rec_bytes=4, wide_lb=lb or 10, srt_W=1, srt_n=n * W, dig_g=W, remap_off=stride - n)
    sets = R.SET_NAMES if n == 5000 else ("uniform", "halfchunk", "halfchunk1", "bounds", "rm1", "zero")
    res = run_case(gpu, curve, n, sets, dict(msm_wide_lb=lb, msm_wide_chunks=chunks), table=table, expect=exp)
    plan, ref = res["halfchunk"]
    assert W <= 16 and (curve != "bls12_381" or c != 17 or W == 16)
    if chunks:
        assert plan.CH == min(chunks, -(-n // 512))
    if n == 5000:
        assert int(ref[0].counts.max()) > 4 * L2_TILE and np.count_nonzero(ref[0].counts) <= 2      # one bucket (and the top carry's)
        assert np.count_nonzero(res["equal"][1][0].counts) > 2


@pytest.mark.parametrize("lb", [8, 11])
def test_wide_record_switch(gpu, lb):
    """Both sides of W * stride + offset == 2^(31 - lb) (BN254 Fr, c = 17: W = 15; 16 offset + 15 n = 2^(31 - lb) with stride = offset + n)."""
    c, W, n = 17, 15, 512
    off = ((1 << (31 - lb)) - 15 * n) // 16
    stride = off + n
    assert W * stride + off == 1 << (31 - lb)
    for o, rec in ((off, 4), (off + 1, 8)):
        table = (c, W, stride + (o - off), o)
        exp = dict(c=c, W=W, path=R.PATH_WIDE, rec_bytes=rec, wide_lb=lb, remap_stride=stride + (o - off), remap_off=o)
        run_case(gpu, "bn254", n, ("uniform", "halfchunk", "halfchunk1", "equal", "rm1", "runs"), dict(msm_wide_lb=lb), table=table, expect=exp)


def test_wide_forced_long_records(gpu):
    """msm_variant bit 3 forces the 8-byte records of the wide sort too"""
    run_case(gpu, "bls12_381", 5000, ("uniform", "halfchunk", "small"), dict(msm_variant=8, msm_wide_chunks=3), table=(17, 16, 5000, 0),
             expect=dict(path=R.PATH_WIDE, rec_bytes=8, W=16))


# ---- F: the two device recoders at the same scalars ---------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_both_device_recoders_at_the_edge_scalars(gpu, curve):
    """k_msm_digits (plain plan, c = 16) and wide_codes (wide plan, c = 17) on the same scalar sets, each against the reference."""
    bits = H.FR[curve].p.bit_length()
    n = 1025
    W16, W17 = R.windows_for(bits, 16), R.windows_for(bits, 17)
    lays = [(16, W16, W16), (17, W17, W17)]                 # the sets that follow the window boundaries, for both layouts, through both plans
    run_case(gpu, curve, n, R.SET_NAMES, dict(msm_c=16), expect=dict(c=16, W=W16, path=R.PATH_SINGLE), seed=7, layouts=lays, both_forms=True)
    run_case(gpu, curve, n, R.SET_NAMES, table=(17, W17, n, 0), expect=dict(c=17, W=W17, path=R.PATH_WIDE), seed=7, layouts=lays, both_forms=True)
