"""CPU tests of tests/msm_sort_ref.py, the reference of the device sort-stage tests (tests/test_gpu_msm_sort.py): its digits against the
host recoder for_each_digit (csh_selftest_digits) wherever that one has something to say -- uniform windows, c = 2 .. 16 -- and its own
reconstruction identity for the balanced plans, plus hand-worked filings and negative controls of its checks."""
import ctypes as C

import numpy as np
import pytest

from tests import helpers as H
from tests import msm_sort_ref as R

# csh_selftest_digits knows the three curves with scalar-field entry points; for_each_digit itself sees limbs and a window count only, so
# Grumpkin's scalars (BN254 Fq, 254 bits like BN254 Fr) go through the BN254 entry
HOST_CURVE = {"bn254": "bn254", "bls12_381": "bls12_381", "grumpkin": "bn254", "bls12_377": "bls12_377"}


def _host_digits(hip, curve, c, scalar):
    digits = (C.c_int32 * 200)()
    W = C.c_int(0)
    sc = R.limbs_of([scalar])
    assert hip.lib().csh_selftest_digits(H.CURVE_IDS[HOST_CURVE[curve]], sc.ctypes.data_as(C.c_void_p), c, digits, C.byref(W)) == 0
    return list(digits)[:W.value]


def _edge_scalars(r, c, W, wide, seed):
    """every scalar set of the device tests at a small n, duplicates removed (order kept)"""
    vals = []
    for name in R.SET_NAMES:
        vals += R.scalar_set(name, r, 67, c, W, wide, seed)
    return list(dict.fromkeys(vals))


@pytest.mark.parametrize("curve", ["bn254", "bls12_381", "grumpkin", "bls12_377"])
@pytest.mark.parametrize("c", list(range(2, 17)))
def test_reference_digits_match_host_recoder(hip, curve, c):
    r = H.FR[curve].p
    bits = r.bit_length()
    assert bits == H.FR[HOST_CURVE[curve]].p.bit_length()
    W = R.windows_for(bits, c)
    vals = _edge_scalars(r, c, W, W, 5)
    assert all(0 <= v < r for v in vals)
    got = R.signed_digits(R.limbs_of(vals), c, W, W)
    for i, v in enumerate(vals):
        want = _host_digits(hip, curve, c, v)
        assert len(want) == W
        assert got[:, i].tolist() == want, "c = %d, scalar %#x" % (c, v)
    if c == 16:                                              # the top code of the 16-bit digit format is reached: digit +2^15
        assert int(got.max()) == 1 << 15 and int(got.min()) >= -(1 << 15) + 1


@pytest.mark.parametrize("curve", ["bn254", "bls12_381", "grumpkin", "bls12_377"])
def test_balanced_plans_reconstruct(curve):
    """Balanced windows (msm_plan.hpp choose_windows): c = ceil(total / W), the low total - W (c - 1) windows c bits wide, the others c - 1.
    The host recoder cannot express them; the reference checks sum digit_w 2^(offset_w) == scalar itself, here for every W the planner
    accepts at some c <= 16."""
    r = H.FR[curve].p
    total = r.bit_length() + 1
    for W in range((total + 15) // 16, 129):
        c = -(-total // W)
        if c < 3:
            continue
        wide = total - W * (c - 1)
        assert 1 <= wide <= W
        widths, offs = R.window_layout(c, W, wide)
        assert offs[-1] + widths[-1] == total
        vals = _edge_scalars(r, c, W, wide, W)
        d = R.signed_digits(R.limbs_of(vals), c, W, wide)    # asserts the identity and |digit| <= half
        assert [sum(int(d[w, i]) << offs[w] for w in range(W)) for i in range(0, len(vals), 7)] == vals[::7]


def test_digit_check_catches_a_wrong_digit():
    r = H.FR["bn254"].p
    vals = [r - 1, 12345, (r + 1) // 2]
    a = R.limbs_of(vals)
    widths, offs = R.window_layout(11, 24, 24)
    d = R.signed_digits(a, 11, 24, 24)
    for w, delta in ((0, 1), (23, -1), (7, 2048)):
        bad = d.copy()
        bad[w, 1] += delta
        with pytest.raises(AssertionError):
            R.check_digits(a, bad, widths, offs)
    # v > half, not v >= half: a chunk equal to half stays positive
    assert R.signed_digits(R.limbs_of([1024]), 11, 24, 24)[:2, 0].tolist() == [1024, 0]
    assert R.signed_digits(R.limbs_of([1025]), 11, 24, 24)[:2, 0].tolist() == [-1023, 1]


def _plan(**kw):
    base = dict.fromkeys(R.INFO_FIELDS, 0)
    base.update(kw)
    return R.Plan(**base)


def test_filing_by_hand():
    """c = 3 (half = 4, NB = 4), three windows: 5 = -3 + 1 * 8, 4 = +4, 60 = 4 + 7 * 8 = 4 - 8 + 64 = (+4, -1, +1), 0 has no entry."""
    a = R.limbs_of([5, 4, 60, 0])
    plain = _plan(c=3, W=3, wide=3, NB=4, L=2, Ln=2, srt_n=4, srt_W=3, srt_wide=3)
    w0, w1, w2 = R.sort_reference(a, plain)
    S = 1 << 31
    assert w0.start.tolist() == [0, 0, 0, 0, 1, 3] and w0.entries.tolist() == [0 | S, 1, 2] and w0.nlanes == 2
    assert w1.start.tolist() == [0, 0, 2, 2, 2, 2] and w1.entries.tolist() == [0, 2 | S] and w1.nlanes == 1
    assert w2.start.tolist() == [0, 0, 1, 1, 1, 1] and w2.entries.tolist() == [2] and w2.nlanes == 1
    # the same digits filed through a two-row table (W' = 2: windows 0 and 2 share sort window 0, row 1 starts at id 100 + 10)
    tab = _plan(c=3, W=3, wide=3, NB=4, L=2, Ln=2, dig_g=2, dig_wp=2, remap_n=4, remap_stride=100, remap_off=10, srt_n=8, srt_W=2, srt_wide=2)
    t0, t1 = R.sort_reference(a, tab)
    assert t0.start.tolist() == [0, 0, 1, 1, 2, 4] and t0.entries.tolist() == [112, 10 | S, 11, 12] and t0.nlanes == 2
    assert t1.start.tolist() == [0, 0, 2, 2, 2, 2] and t1.entries.tolist() == [10, 12 | S] and t1.nlanes == 1
    # narrow windows of a balanced plan take their own lane length
    bal = _plan(c=3, W=4, wide=1, NB=4, L=1, Ln=2, srt_n=4, srt_W=4, srt_wide=1)
    refs = R.sort_reference(a, bal)
    for ws, ref in enumerate(refs):
        total = int(ref.start[-1])
        assert ref.nlanes == (total if ws == 0 else (total + 1) // 2)


def assert_runs_reach_the_peel_paths(digit_row):
    """The "runs" set in a window with many buckets: a wave that peels twice and stops at a group of 7, one whose leading group of 7
    stops the rounds at once with groups of 8 and 9 behind it, and one that peels four times with a group of 8 or more left over."""
    prof = R.wave_profiles(digit_row)
    assert any(p == 2 and stop == 7 for p, stop, left in prof), prof
    assert any(p == 0 and stop == 7 and left >= 9 for p, stop, left in prof), prof
    assert any(p == 4 and left >= 8 for p, stop, left in prof), prof


def test_wave_model_and_the_runs_set():
    assert R.wave_peels([5] * 7 + [0] * 57) == (0, 7, 7)
    assert R.wave_peels([5] * 8 + [6] * 56) == (2, 0, 0)
    assert R.wave_peels([9] + [5] * 63) == (0, 1, 63)                      # a single lane in front ends the peeling
    assert R.wave_peels([k for k in range(1, 9) for _ in range(8)]) == (4, 0, 8)
    r = H.FR["bn254"].p
    for c in (11, 15, 16):
        W = R.windows_for(254, c)
        d = R.signed_digits(R.limbs_of(R.scalar_set("runs", r, 1025, c, W, W, 1)), c, W, W)
        assert_runs_reach_the_peel_paths(d[0])
        assert_runs_reach_the_peel_paths(d[W // 2])


def test_reference_is_vectorised():
    """2^15 scalars in 128 windows, digits with their check and the whole filing, well under a second (best of three: the bound is
    about the algorithm -- numpy steps per window, none per scalar -- not about the load of the machine)."""
    import time
    a = H.uniform_limbs(H.FR["bn254"], np.random.RandomState(3), 1 << 15)
    plan = _plan(c=2, W=128, wide=128, NB=2, L=16, Ln=16, srt_n=1 << 15, srt_W=128, srt_wide=128)
    best = 1e9
    for _ in range(3):
        t = time.perf_counter()
        ref = R.sort_reference(a, plan)
        best = min(best, time.perf_counter() - t)
    assert len(ref) == 128 and all(int(w.start[-1]) <= 1 << 15 for w in ref)
    assert best < 1.0, "reference took %.2f s" % best
