"""GPU parity of the MSM tail (k_msm_merge, k_msm_reduce) at bucket shapes chosen through the tune keys: csh_msm_dev on BN254 G1 and
BLS12-381 G2 against the CPU oracle (oracle/c's Pippenger on the same bases and scalars), compared as group elements.

k_msm_merge works in two phases: every quad of a 64-bucket block folds the first two partial sums of its bucket, buckets with three
or more (and fewer than MERGE_CAP = 16 + 1) go on a block-local list, and the list is then served by the first quads of the block. The
shapes below give a bucket 2, 3, 4-5, ~8, ~13 and >= 17 partials, blocks whose list holds every bucket (64 > one wave's 16 quads), exactly
one bucket, and none. k_msm_reduce multiplies the running sum by the lowest bucket index of its segment and by gaps above 4 with a
2-bit windowed multiple: the segment widths below put every 2-bit digit, leading zero digits and the multiplier 1 into one wave."""
import numpy as np
import pytest

from oracle import cbridge as cb
from oracle import curves as cv
from tests import helpers as H

pytestmark = pytest.mark.gpu
GROUPS = [("bn254", 0), ("bls12_381", 1)]
_CASES = {}


def _limbs(values):
    return np.array([[(v >> (64 * i)) & (2**64 - 1) for i in range(4)] for v in values], dtype=np.uint64)


def _uniform(seed, n):
    rs = np.random.RandomState(seed)
    limbs = rs.randint(0, 1 << 63, size=(n, 4), dtype=np.uint64)
    limbs[:, 3] >>= np.uint64(3)                                    # canonical values < 2^252
    return limbs


def _scalars(kind, n):
    if kind == "uniform":
        return _uniform(n, n)
    if kind == "repeated":                                           # one value 2000 times among uniform ones, spread over the vector
        limbs = _uniform(n + 1, n)
        limbs[np.random.RandomState(5).permutation(n)[:2000]] = limbs[17]
        return limbs
    if kind == "sparse_digits":
        # every 11-bit digit of every scalar is one of a few widely spaced values (all <= 2^10; the signed recoding borrows only above
        # 2^(c-1) = 1024, msm_digits.hpp `v > half`, so each value is its own bucket index):
        # inside a 64-bucket segment the non-empty buckets are 44 .. 63 apart, inside a 7-bucket one 5 .. 6 apart or adjacent
        digits = [1, 7, 13, 14, 20, 64, 70, 127, 129, 200, 256, 262, 320, 383, 512, 1000, 1024]
        r = H.rng(n)
        return _limbs([sum(r.choice(digits) << (11 * w) for w in range(22)) for _ in range(n)])
    raise KeyError(kind)


def _case(curve, group, kind, n):
    """Bases, scalars (canonical limbs) and the oracle's result, made once per (group, scalar kind, n) and only read afterwards."""
    key = (curve, group, kind, n)
    if key not in _CASES:
        cid = H.CURVE_IDS[curve]
        G = cv.CURVES[curve][group]
        pts = cb.generate_bases_wide(cid, group, 0x7A11 + group, n)
        limbs = _scalars(kind, n)
        want = cv.unpack_points(G, cb.msm_fast(cid, group, pts, limbs, montgomery=False))[0]
        _CASES[key] = (pts, limbs, want)
    return _CASES[key]


def _check(gpu, curve, group, kind, n, settings):
    cid = H.CURVE_IDS[curve]
    G = cv.CURVES[curve][group]
    pts, limbs, want = _case(curve, group, kind, n)
    bases = gpu.Bases(cid, group, pts)
    dsc = gpu.DeviceBuffer.from_host(limbs)
    try:
        for kv in settings:
            with gpu.tuned(**kv):
                got = bases.msm_dev(dsc, n, montgomery=False)
                ran = gpu.bindings.msm_last_params()
            assert G.eq(H.jac_to_affine(G, got), want), kv
            if "msm_c" in kv:
                assert ran[0] == kv["msm_c"], (kv, ran)
            if "msm_l" in kv:
                assert ran[2] == kv["msm_l"], (kv, ran)
    finally:
        dsc.free()
        bases.free()


@pytest.mark.parametrize("curve,group", GROUPS)
def test_merge_partials_per_bucket(gpu, curve, group):
    """n = 2^12, c = 4: 8 buckets of ~500 entries per window (one block of 8 live quads); lane lengths 300 .. 16 give a bucket 2, 3, 4-5,
    ~8, ~13 and >= 17 partial sums, the last one past MERGE_CAP into the block-wide tree. c = 7, lane length 16: 64 buckets of ~64 entries,
    4-5 partials each: every quad of the block is on the list, four waves of second-phase work. c = 7, lane length 200: buckets span one
    or two lanes, the list stays empty."""
    settings = [dict(msm_c=4, msm_l=l) for l in (300, 200, 120, 64, 40, 16)] + [dict(msm_c=7, msm_l=16), dict(msm_c=7, msm_l=200)]
    _check(gpu, curve, group, "uniform", 1 << 12, settings)


@pytest.mark.parametrize("curve,group", GROUPS)
def test_merge_one_long_bucket_in_a_block(gpu, curve, group):
    """n = 2^13, c = 10, lane length 160: 512 buckets of ~16 entries (one partial, two where a lane boundary falls inside) in 8 blocks per
    window; one scalar value repeated 2000 times adds one bucket of 13-14 partials to each window: its block's list has exactly one entry,
    the other blocks' lists none. Lane length 64 sends the same bucket (32 partials) to the block-wide tree instead."""
    _check(gpu, curve, group, "repeated", 1 << 13, [dict(msm_c=10, msm_l=160), dict(msm_c=10, msm_l=64)])


@pytest.mark.parametrize("curve,group", GROUPS)
@pytest.mark.parametrize("kind", ["uniform", "sparse_digits"])
def test_reduce_segment_multiples(gpu, curve, group, kind):
    """n = 2^12, c = 11 (1024 buckets), segments of 2, 3, 7 and 64 buckets: the multipliers 1 + 2 k, 1 + 3 k, 1 + 7 k, 1 + 64 k of the 16
    segments of a wave (uniform scalars: nearly every bucket is occupied, the lowest one of a segment is its first) cover every 2-bit digit
    at every position, widths of 1 .. 10 bits side by side and the multiplier 1. The sparse digit set leaves gaps of 5 .. 63 buckets
    inside the wider segments: the gap multiple. On G2 the four-lane reduction is msm_variant bit 0; both forms run."""
    variants = (0, 1) if group else (0,)
    settings = [dict(msm_c=11, msm_l=128, msm_seg_buckets=per, msm_variant=v) for per in (2, 3, 7, 64) for v in variants]
    _check(gpu, curve, group, kind, 1 << 12, settings)


@pytest.mark.parametrize("variant", [16, 1])
def test_other_reduction_forms_share_the_tail(gpu, variant):
    """msm_variant bit 4 (the reduction merges a bucket's partial slots itself; shares the windowed multiple) and bit 0 (lane-serial
    reduction on G1; reads the dense array of the two-phase merge), once each on one shape with 3-partial buckets and gaps above 4."""
    _check(gpu, "bn254", 0, "sparse_digits", 1 << 12, [dict(msm_c=11, msm_l=96, msm_seg_buckets=64, msm_variant=variant)])
